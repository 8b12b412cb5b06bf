#!/usr/bin/env python3
"""time the Burgers data generator's rollout kernel against the score check's, and the generator end to end:
    python tools/burgers_datagen_time.py [N ...]            (default 256 4096 32768; s = 128, Nt = 10, T = 1: 10 000 Euler steps)

Per N, interleaved in every round:
  (a) solvers.burgers_numeric_solve_free          sdc_burgers_rollout: one workgroup per trajectory, u in LDS, a barrier per step
  (b) burgers_datagen.burgers_numeric_solve_free_wave    sdc_burgers_rollout_wave: one wave per trajectory, u in registers, at the
      library's waves per block and at each of --wpb (default 1 2 4 8 16)
Times are device times between two events around the one launch (inputs converted beforehand), min - max over --rounds (default 5)
after one untimed round; the outputs of all arms are compared bit for bit.
--sizes S ...   then (a) against (b) at the other cell counts a wave covers (default 1 64 65 256 257 512), N = 256 and 32768.
--generate N    then BurgersDataGenerator().generate(0.9 N, 0.1 N, force="device") end to end (default 100000; 0 skips it), once
                untimed and once timed, synthesis / rollouts / shuffle listed separately.

SDC_LIB_PATH=<another build> replaces the library the package itself loads."""
import _libsel  # noqa: F401,E402  (SDC_LIB_PATH -> safediffcon_amd._lib.use_library, tools only)
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safediffcon_amd import burgers_datagen as bd, solvers  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("N", nargs="*", type=int)
ap.add_argument("--wpb", nargs="*", type=int, default=[1, 2, 4, 8, 16])
ap.add_argument("--sizes", nargs="*", type=int, default=[1, 64, 65, 256, 257, 512])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--generate", type=int, default=100000)
ap.add_argument("--chunk", type=int, default=8192)
args = ap.parse_args()
dev = torch.device("cuda:0")
S, NT = 128, 10
print(f"device: {torch.cuda.get_device_name(0)}; s = {S}, Nt = {NT}, T = 1, dt = 1e-4; {args.rounds} rounds after one untimed", flush=True)


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def inputs(N, s):
    """s = 128: white noise of amplitude 0.3 as in the tests; other sizes: two sine modes per sample, which stay finite at visc = 0.01
    on every grid up to 512 cells (visc dt / dx^2 <= 0.27)"""
    g = torch.Generator().manual_seed(N + s)
    if s == 128:
        return (0.3 * torch.randn(N, s, generator=g)).to(dev), (0.3 * torch.randn(N, NT, s, generator=g)).to(dev)
    x = (torch.arange(1, s + 1, dtype=torch.float64) / (s + 1)).to(dev)
    k = torch.randint(1, 5, (N, 1), generator=g).to(dev)
    ph = (6.28 * torch.rand(N, NT, 1, generator=g)).to(dev)
    return (0.3 * torch.sin(6.283185307179586 * k * x)).float(), (0.3 * torch.sin(3.141592653589793 * k[:, None] * x + ph)).float()


def compare(N, s, wpbs):
    u0, f = inputs(N, s)
    arms = {"(a) sdc_burgers_rollout": lambda: solvers.burgers_numeric_solve_free(u0, f, 0.01, 1.0, dt=1e-4, num_t=NT),
            "(b) sdc_burgers_rollout_wave": lambda: bd.burgers_numeric_solve_free_wave(u0, f, 0.01, 1.0, dt=1e-4, num_t=NT)}
    for w in wpbs:
        arms[f"(b) waves_per_block {w}"] = lambda w=w: bd.burgers_numeric_solve_free_wave(u0, f, 0.01, 1.0, dt=1e-4, num_t=NT, waves_per_block=w)
    times = {k: [] for k in arms}
    want = None
    for r in range(args.rounds + 1):
        for k, fn in arms.items():
            ms, out = device_ms(fn)
            if r:
                times[k].append(ms)
            elif want is None:
                want = out
                if not bool(torch.isfinite(want).all()):
                    raise SystemExit(f"N = {N}, s = {s}: the rollout is not finite")
            elif not torch.equal(out, want):
                raise SystemExit(f"N = {N}, s = {s}: {k} differs from (a)")
            del out
    base = min(times["(a) sdc_burgers_rollout"])
    print(f"N = {N}, s = {s}  (outputs finite and bit-identical across the arms)", flush=True)
    for k, v in times.items():
        print(f"  {k:32s} {min(v):9.2f} - {max(v):9.2f} ms   min / (a) min = {min(v) / base:.3f}", flush=True)


for N in args.N or [256, 4096, 32768]:
    compare(N, S, args.wpb)
for s in args.sizes:                                     # the other lane maps: K = 1, 4, 8 and ragged last lanes
    for N in (256, 32768):
        compare(N, s, [])

if args.generate:
    n = args.generate
    gen = bd.BurgersDataGenerator(device=dev)
    for r in range(2):
        timing = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = gen.generate(n - n // 10, n // 10, seed=0, force="device", chunk=args.chunk, timing=timing)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        ok = all(bool(torch.isfinite(v).all()) for sp in out.values() for k, v in sp.items() if k != "attrs")
        del out
        print(f"generate({n - n // 10}, {n // 10}, force='device', chunk={args.chunk}) run {r}: {total:.2f} s total; "
              + "; ".join(f"{k[:-2]} {v:.2f} s" for k, v in timing.items()) + f"; rest (draws, copies) {total - sum(timing.values()):.2f} s; finite: {ok}",
              flush=True)
