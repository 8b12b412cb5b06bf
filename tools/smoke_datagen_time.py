#!/usr/bin/env python3
"""time the smoke data generator (SmokeDataGenerator.generate: pass 1, decision, pass 2 of the accepted) for batches of seeds:
    python tools/smoke_datagen_time.py [B ...]                (default 1 64 256; the shipped 256-step / 32-frame / 64-cell shape)

--modes reference device   which noise modes to time (default both).  "reference" lists the host's draw time and the upload time
                           separately (each sample's upload is synchronised to be timed, so its total is an upper bound).
--chunk N                  samples per launch (default 64, generate's default)
--other-lib PATH           a second build of libsdc_hip.so (the parent commit's, say) loaded beside the first: both builds'
                           sdc_smoke_rollout -- the score check's kernel, which the generator's kernel shares its source with --
                           run interleaved on the same device buffers at --rollout-B samples (default 64), the other build
                           twice per round so that its own run-to-run spread is on record; the rows are compared bit for bit
--rounds N                 timed rounds for the --other-lib comparison (default 5)

SDC_LIB_PATH=<another build> replaces the library the package itself loads."""
import _libsel  # noqa: F401,E402  (SDC_LIB_PATH -> safediffcon_amd._lib.use_library, tools only)
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safediffcon_amd import _lib, smoke_datagen, smoke_solver  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="*", type=int)
ap.add_argument("--modes", nargs="*", default=["reference", "device"])
ap.add_argument("--chunk", type=int, default=64)
ap.add_argument("--other-lib")
ap.add_argument("--rollout-B", type=int, default=64)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


if args.other_lib:
    lib = _lib.get_lib()
    other = C.CDLL(os.path.abspath(args.other_lib)).sdc_smoke_rollout
    other.restype, other.argtypes = _lib.SIGNATURES["sdc_smoke_rollout"]
    B, nt, nx, T = args.rollout_B, 32, 64, 256
    g = torch.Generator().manual_seed(B)
    c = (torch.randn(2, B, nt, nx, nx, generator=g) * 2.0).to(dev)
    c[:, :, :, 8:56, 8:56] = 0
    d0 = torch.zeros(B, nx, nx)
    d0[:, 10:16, 20:44] = 1.0
    d0 = d0.to(dev)
    v0 = torch.from_numpy(smoke_solver.init_velocity_()).to(dev).reshape(128, 128, 2).contiguous()
    sim = smoke_solver.init_sim_128()
    lab_n, nb_n, lab_s, nb_s = smoke_solver._device_labels(dev)
    fluid = sim.fluid_mask_device(dev)
    wbytes = lib.sdc_smoke_rollout_workspace_bytes(B)
    work = torch.empty(wbytes, dtype=torch.uint8, device=dev)

    def entry(fn):
        out = torch.empty(B, nt, 7, nx, nx, dtype=torch.float64, device=dev)
        outz = torch.empty(B, nt, nx, nx, dtype=torch.float64, device=dev)
        rc = fn(c[0].data_ptr(), c[1].data_ptr(), c[0].stride(0), c[0].stride(1), d0.data_ptr(), d0.stride(0), v0.data_ptr(), 0,
                fluid.data_ptr(), lab_n.data_ptr(), lab_s.data_ptr(), nb_n, nb_s, out.data_ptr(), outz.data_ptr(), work.data_ptr(), wbytes,
                B, nt, nx, T, 16, 112, 1e-8, 500, torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0, f"sdc_smoke_rollout returned {rc}"
        return out, outz
    a, b = entry(lib.sdc_smoke_rollout), entry(other)
    same = all(torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)) for x, y in zip(a, b))
    print(f"sdc_smoke_rollout B={B}, 256 steps: rows of the two libraries are {'bit-identical' if same else 'DIFFERENT'}", flush=True)
    arms = {"this lib": lambda: entry(lib.sdc_smoke_rollout), "other lib": lambda: entry(other), "other lib (repeat)": lambda: entry(other)}
    ms = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            ms[k].append(timed(fn)[0] * 1e3)
    for k, v in ms.items():
        print(f"sdc_smoke_rollout B={B} {k}: median {statistics.median(v):.2f} ms, min {min(v):.2f} ms, max {max(v):.2f} ms over {len(v)} rounds",
              flush=True)

gen = smoke_datagen.SmokeDataGenerator(device=dev)
timed(lambda: gen.generate([0], noise="device", chunk=1))                  # warm-up: library load, LDS opt-in, allocator
for B in args.B or [1, 64, 256]:
    for mode in args.modes:
        timing = {}
        dt, res = timed(lambda: gen.generate(range(1000, 1000 + B), noise=mode, chunk=args.chunk, timing=timing if mode == "reference" else None))
        acc = int(res["accepted"].sum())
        passes = B + acc
        extra = (f", of it host draw {timing.get('host_draw_s', 0):.2f} s and upload {timing.get('upload_s', 0):.2f} s"
                 f" ({passes * 256 * 128 * 128 * 2 * 8 / 2 ** 30:.1f} GiB)") if mode == "reference" else ""
        print(f"generate B={B} noise={mode} chunk={args.chunk}: {dt:.2f} s for {passes} passes ({acc} of {B} seeds accepted){extra}; "
              f"{dt / passes * 1e3:.0f} ms per pass", flush=True)
