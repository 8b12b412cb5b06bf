#!/usr/bin/env python3
"""Same-box A/B of the optimizer tail of a fine-tuning iteration (clip_grad_norm_ + Adam + EMA twin) on the parameter lists of the
C2 / C3 / C4 nets, random gradients, one process:

  (a) torch.nn.utils.clip_grad_norm_ + torch.optim.Adam(capturable=True) + a per-parameter lerp_ EMA
  (b) the same with torch.optim.Adam(fused=True)
  (c) sdc.FusedOptimizer (clip, Adam and EMA in sdc_optim_step's three launches)

  python tools/optim_ab.py [--workloads c2,c3,c4] [--steps 20] [--warmup 5] [--rounds 3] [--graphed c3,c4]

Part 1 times the tail alone, with the EMA updated on every step (all arms alike; the reference updates it every 10th) and
without an EMA.  "bytes" is what ONE pass needs -- 4 n x (read g for the norm; read p, g, m, v, ema; write p, m, v, ema), 4 n x 8
without the EMA -- and "of HBM" that count over the time over 6.29 TB/s (the measured float4 copy): the arms that make more
passes move more bytes than that, so for them it is an effective figure, not the bus load.
Part 2 times the replayed GraphedLossStep (loss + backward + optimizer.step()) of C3 at B = 64 and C4 at B = 4 with torch's Adam
recorded behind the backward pass against FusedOptimizer: Adam alone (a captured torch optimizer has no clipping and no EMA),
and FusedOptimizer with clipping and an EMA twin updated every 10th step, which torch's arm cannot record.
Arms alternate round by round; medians; shader clock and socket power sampled over each timed region (bench.GpuSensors)."""
import _libsel  # noqa: F401  (SDC_LIB_PATH -> safediffcon_amd._lib.use_library, tools only)
import argparse
import statistics
import time

import torch

import bench
import safediffcon_amd as sdc
from f16_train_step import DEV, FT_B, make

HBM = 6.29e12
LR, BETAS = 1e-4, (0.9, 0.99)


def _nets(name):
    torch.manual_seed(0)
    if name == "c2":
        return sdc.Unet2D(dim=64, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1)
    if name == "c3":
        return sdc.Unet1D(dim=256, dim_mults=(1, 2, 4, 8), channels=12, resnet_block_groups=1)
    return sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7)


def _timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    sens = bench.GpuSensors(0)
    sens.start()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    ck = sens.stop() or {}
    return a.elapsed_time(b) / steps, wall, ck


def _arm(kind, shapes, ema):
    """fresh parameters / gradients / EMA twin of one arm and the function that runs its tail once"""
    gen = torch.Generator(device=DEV).manual_seed(1)
    ps = [0.05 * torch.randn(s, device=DEV, generator=gen) for s in shapes]
    for p in ps:
        p.grad = 1e-2 * torch.randn(p.shape, device=DEV, generator=gen)
    es = [p.clone() for p in ps] if ema else None
    if kind == "c":
        opt = sdc.FusedOptimizer(ps, kind="adam", lr=LR, betas=BETAS, max_grad_norm=1.0)
        if ema:
            opt.attach_ema(es, beta=0.995, update_every=1, update_after_step=0)
        return opt.step, (ps, es, opt)
    opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, capturable=True) if kind == "a" else torch.optim.Adam(ps, lr=LR, betas=BETAS, fused=True)

    def tail():
        torch.nn.utils.clip_grad_norm_(ps, 1.0)
        opt.step()
        if ema:
            with torch.no_grad():
                for e, p in zip(es, ps):
                    e.lerp_(p, 1.0 - 0.995)
    return tail, (ps, es, opt)


def tails(names, steps, warmup, rounds):
    for name in names:
        shapes = [tuple(p.shape) for p in _nets(name).parameters() if p.requires_grad]
        n = sum(int(torch.Size(s).numel()) for s in shapes)
        print(f"[measured] {name}: {len(shapes)} tensors, {n / 1e6:.1f} M elements, {4 * n / 1e6:.0f} MB", flush=True)
        for ema in (True, False):
            nbytes = 4 * n * (10 if ema else 8)
            arms = {k: _arm(k, shapes, ema) for k in "abc"}
            res = {k: [] for k in arms}
            for r in range(rounds):
                for k in ("abc", "cba", "bca")[r % 3]:
                    ms, wall, ck = _timed(arms[k][0], steps, warmup)
                    res[k].append(ms)
                    print(f"[measured] {name} {'clip+adam+ema' if ema else 'clip+adam'} ({k}) round {r}: {ms:.3f} ms/step (host wall {wall:.3f})  "
                          f"sclk median {ck.get('sclk_mhz_median')} MHz  power mean {ck.get('power_w_mean')} W", flush=True)
            med = {k: statistics.median(v) for k, v in res.items()}
            for k in "abc":
                print(f"[measured] {name} {'clip+adam+ema' if ema else 'clip+adam'} ({k}): median {med[k]:.3f} ms/step, one-pass bytes "
                      f"{nbytes / 1e6:.0f} MB, {nbytes / (med[k] * 1e-3) / HBM * 100:.1f} % of HBM 6.29 TB/s", flush=True)
            best = min(med["a"], med["b"])
            print(f"[measured] {name} {'clip+adam+ema' if ema else 'clip+adam'}: (c) / faster of (a), (b) = {med['c']:.3f} / {best:.3f} ms = "
                  f"{med['c'] / best:.3f}", flush=True)
            del arms
            torch.cuda.empty_cache()


def graphed(names, steps, warmup, rounds):
    for name in names:
        B = FT_B[name]
        arms = {}
        for k in ("a", "b", "c", "c+clip+ema"):
            net, gd, state, t, noise = make(name, B)
            ps = [p for p in net.parameters() if p.requires_grad]
            if k == "a":
                opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, capturable=True)
            elif k == "b":
                opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, capturable=True, fused=True)
            else:
                opt = sdc.FusedOptimizer(ps, kind="adam", lr=LR, betas=BETAS, max_grad_norm=1.0 if k != "c" else 0.0)
                if k != "c":
                    opt.attach_ema([p.detach().clone() for p in ps], beta=0.995, update_every=10)
            arms[k] = (sdc.GraphedLossStep(gd, state, t=t, noise=noise, optimizer=opt), opt)
        net, gd, state, t, noise = make(name, B)
        arms["no optimizer"] = (sdc.GraphedLossStep(gd, state, t=t, noise=noise), None)
        res = {k: [] for k in arms}
        order = list(arms)
        for r in range(rounds):
            for k in (order if r % 2 == 0 else order[::-1]):
                ms, wall, ck = _timed(arms[k][0], steps, warmup)
                res[k].append(ms)
                print(f"[measured] {name} B={B} GraphedLossStep ({k}) round {r}: {ms:.3f} ms/step (host wall {wall:.3f})  sclk median "
                      f"{ck.get('sclk_mhz_median')} MHz  power mean {ck.get('power_w_mean')} W", flush=True)
        med = {k: statistics.median(v) for k, v in res.items()}
        base = med["no optimizer"]
        for k in order:
            print(f"[measured] {name} B={B} GraphedLossStep ({k}): median {med[k]:.3f} ms/step, {med[k] - base:+.3f} ms over loss + backward alone",
                  flush=True)
        best = min(med["a"], med["b"])
        print(f"[measured] {name} B={B} GraphedLossStep: (c) / faster of (a), (b) = {med['c']:.3f} / {best:.3f} ms = {med['c'] / best:.3f}", flush=True)
        for st, _ in arms.values():
            st.close()
        del arms
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c3,c4")
    ap.add_argument("--graphed", default="c3,c4")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(DEV)
    print(f"[measured] torch {torch.__version__}, {torch.cuda.get_device_name(0)}; {a.steps} steps per timed region after {a.warmup} warm-up "
          f"steps, {a.rounds} alternating rounds, medians", flush=True)
    if a.workloads:
        tails(a.workloads.split(","), a.steps, a.warmup, a.rounds)
    if a.graphed:
        graphed(a.graphed.split(","), a.steps, a.warmup, a.rounds)


if __name__ == "__main__":
    main()
