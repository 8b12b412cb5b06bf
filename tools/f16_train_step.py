#!/usr/bin/env python3
"""Same-box A/B of fine-tuning at the default precision against net.train_precision = 6 / 7 (fp16 operands on the 3-tap convs in all
three directions: csrc/sdc_conv_f16.hip, csrc/sdc_wgrad_f16.hip).

  python tools/f16_train_step.py [--workloads c4,c2,c3] [--steps 10] [--warmup 3] [--rounds 2] [--arm 6|7]
      the replayed GraphedLossStep (loss = mean(w_b p_losses_b); loss.backward()) of each workload at its fine-tuning batch
      (C4 B = 4, C2 / C3 B = 64), default against the arm, interleaved round by round; ms/step with the shader clock and socket
      power sampled over each timed region (bench.GpuSensors)
  python tools/f16_train_step.py --shapes [--workloads ...]
      every weight gradient and data gradient of one eager step at train_precision 7 that the fp16 kernels cover: fp32 against fp16,
      median of 10 launches each -- the data of the dispatch tables
  python tools/f16_train_step.py --one ARM [--workloads c4]
      replays the step of one arm only (for a rocprofv3 --kernel-trace --stats run per arm)
"""
import _libsel  # noqa: F401  (SDC_LIB_PATH -> safediffcon_amd._lib.use_library, tools only)
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import safediffcon_amd as sdc  # noqa: E402
from safediffcon_amd import autograd, grad_ops  # noqa: E402
from oracle.detweights import det_tensor  # noqa: E402

DEV = torch.device("cuda:0")
FT_B = {"c4": 4, "c2": 64, "c3": 64}


def make(name, B):
    torch.manual_seed(0)
    if name == "c2":
        net = sdc.Unet2D(dim=64, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1).to(DEV)
        gd = sdc.GaussianDiffusionBurgers(net, seq_length=(16, 128), timesteps=1000, temporal=True, use_conv2d=True,
                                          is_condition_u0=True, is_condition_uT=True, condition_idx=10).to(DEV)
        shape = (3, 16, 128)
    elif name == "c3":
        net = sdc.Unet1D(dim=256, dim_mults=(1, 2, 4, 8), channels=12, resnet_block_groups=1).to(DEV)
        gd = sdc.GaussianDiffusionTokamak(net, seq_length=128, nt=122, timesteps=1000).to(DEV)
        shape = (12, 128)
    else:
        net = sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7).to(DEV)
        gd = sdc.GaussianDiffusionSmoke(net, image_size=64, frames=32, timesteps=1000, loss_type="l2").to(DEV)
        shape = (32, 7, 64, 64)
    state = det_tensor((B, *shape), 9, 0.3).to(DEV)
    t = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(3)).to(DEV)
    noise = det_tensor((B, *shape), 10).to(DEV)
    return net, gd, state, t, noise


def _arm_name(a):
    return "default" if a is None else f"train_precision {a}"


def step_ab(names, steps, warmup, rounds, arm):
    for name in names:
        B = FT_B[name]
        steps_by_arm = {}
        for a in (None, arm):
            net, gd, state, t, noise = make(name, B)
            net.train_precision = a
            steps_by_arm[a] = sdc.GraphedLossStep(gd, state, t=t, noise=noise)
        res = {None: [], arm: []}
        for r in range(rounds):
            for a in ((None, arm) if r % 2 == 0 else (arm, None)):
                st = steps_by_arm[a]
                for _ in range(warmup):
                    st()
                torch.cuda.synchronize()
                sens = bench.GpuSensors(0)
                sens.start()
                t0 = time.perf_counter()
                for _ in range(steps):
                    st()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3 / steps
                ck = sens.stop() or {}
                res[a].append(ms)
                print(f"[measured] {name} B={B} {_arm_name(a)} round {r}: {ms:.2f} ms/step  sclk median {ck.get('sclk_mhz_median')} MHz "
                      f"(min {ck.get('sclk_mhz_min')})  power mean {ck.get('power_w_mean')} W (max {ck.get('power_w_max')})", flush=True)
        m0, m1 = statistics.median(res[None]), statistics.median(res[arm])
        print(f"[measured] {name} B={B}: train_precision {arm} / default = {m1:.2f} / {m0:.2f} ms/step = {m1 / m0:.3f}", flush=True)
        for st in steps_by_arm.values():
            st.close()
        del steps_by_arm
        torch.cuda.empty_cache()


def one(name, arm, steps):
    net, gd, state, t, noise = make(name, FT_B[name])
    net.train_precision = None if arm == 0 else arm
    st = sdc.GraphedLossStep(gd, state, t=t, noise=noise)
    for _ in range(steps):
        st()
    torch.cuda.synchronize()
    st.close()


def _median_ms(fn, n=10):
    for _ in range(2):
        fn()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in evs)


def shapes(names):
    for name in names:
        net, gd, state, t, noise = make(name, FT_B[name])
        net.train_precision = 7
        wcalls, dcalls = [], []
        real_wgrad, real_raw = grad_ops.conv_wgrad, autograd.conv_raw

        def rec_wgrad(g, x, k, stride=(1, 1, 1), pad=(0, 0, 0), up=(1, 1, 1), bias=True, precision=0, exp=None):
            if precision in (6, 7):
                wcalls.append((g, x, k, pad, bias, exp))
            return real_wgrad(g, x, k, stride, pad, up, bias=bias, precision=precision, exp=exp)

        def rec_raw(x, wp, bias, cout, k, **kw):
            if kw.get("gexp") is not None:
                dcalls.append((x, wp, cout, k, kw["pad"], kw["gexp"]))
            return real_raw(x, wp, bias, cout, k, **kw)
        grad_ops.conv_wgrad, autograd.conv_raw = rec_wgrad, rec_raw
        try:
            loss = gd.p_losses(state, t, noise=noise, mean=False).mean()
            loss.backward()
        finally:
            grad_ops.conv_wgrad, autograd.conv_raw = real_wgrad, real_raw
        torch.cuda.synchronize()
        seen = set()
        tot32 = tot16 = 0.0
        for g, x, k, pad, bias, e in wcalls:
            key = ("w", tuple(g.shape), tuple(x.shape), k)
            ms32 = _median_ms(lambda: real_wgrad(g, x, k, pad=pad, bias=bias))
            ms16 = _median_ms(lambda: real_wgrad(g, x, k, pad=pad, bias=bias, precision=7, exp=e))
            kn = grad_ops.conv_wgrad_kernel(g, x, k, pad=pad, precision=7)
            tot32, tot16 = tot32 + ms32, tot16 + ms16
            flop = 2.0 * g.numel() * x.shape[1] * k[0] * k[1] * k[2]
            print(f"[measured] {name} wgrad {k[0]}x{k[1]}x{k[2]} M {g.shape[1]} N {x.shape[1]} B {g.shape[0]} {tuple(g.shape[2:])}: "
                  f"fp32 {ms32 * 1e3:.1f} us | {kn} {ms16 * 1e3:.1f} us ({flop / ms16 / 1e9:.0f} TFLOP/s) -> x{ms32 / ms16:.2f}"
                  f"{' (repeat)' if key in seen else ''}", flush=True)
            seen.add(key)
        print(f"[measured] {name}: fp16-covered weight gradients of one step: fp32 {tot32:.2f} ms, fp16 {tot16:.2f} ms", flush=True)
        tot32 = tot16 = 0.0
        for x, wp, cout, k, pad, e in dcalls:
            key = ("d", tuple(x.shape), cout, k)
            d32 = _median_ms(lambda: real_raw(x, wp, None, cout, k, pad=pad, prec=7))      # the unscaled (sampler) instance
            n4 = int(grad_ops._lib.get_lib().sdc_pack_conv_weight_floats(cout, x.shape[1], *k, 4))
            wp4 = wp[:n4]
            d4 = _median_ms(lambda: real_raw(x, wp4, None, cout, k, pad=pad))
            d16 = _median_ms(lambda: real_raw(x, wp, None, cout, k, pad=pad, prec=7, gexp=e))
            tot32, tot16 = tot32 + d4, tot16 + d16
            print(f"[measured] {name} dgrad {k[0]}x{k[1]}x{k[2]} Cin {x.shape[1]} Cout {cout} B {x.shape[0]} {tuple(x.shape[2:])}: "
                  f"precision 4 {d4 * 1e3:.1f} us | fp16 scaled {d16 * 1e3:.1f} us (unscaled {d32 * 1e3:.1f}) -> x{d4 / d16:.2f}"
                  f"{' (repeat)' if key in seen else ''}", flush=True)
            seen.add(key)
        print(f"[measured] {name}: fp16-covered data gradients of one step: precision 4 {tot32:.2f} ms, fp16 {tot16:.2f} ms", flush=True)
        del net, gd, wcalls, dcalls
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c4,c2,c3")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--arm", type=int, default=6, choices=(6, 7))
    ap.add_argument("--shapes", action="store_true")
    ap.add_argument("--one", type=int, default=None, choices=(0, 6, 7), help="replay one arm only (0 = default)")
    a = ap.parse_args()
    torch.cuda.set_device(DEV)
    names = a.workloads.split(",")
    if a.shapes:
        shapes(names)
    elif a.one is not None:
        for n in names:
            one(n, a.one, a.steps)
    else:
        step_ab(names, a.steps, a.warmup, a.rounds, a.arm)


if __name__ == "__main__":
    main()
