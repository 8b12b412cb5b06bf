#!/usr/bin/env python3
"""time the streaming softmax attention core (csrc/sdc_attn_long.hip) at the smoke net's mid site and the net around it:
    python tools/attn_long_time.py [--reps N] [--warmup N] [--no-net] [--no-sdpa]

Core: per-launch device-event time (median, min - max over --reps launches after --warmup) of sdc_attn and sdc_attn_bwd at
inner = 32 frames, heads = 4, outer = B in (1, 4), ntok in (400, 1024, 4096), and the share of the 157.3 TFLOP/s fp32-MFMA
peak it stands for.  FLOPs counted: forward 4 ntok^2 32 per head and sequence (q k^T and p v); backward 2.5 x that (the five
products of the gradient) -- the backward EXECUTES 4.5 x (it recomputes the forward for the row statistics and q k^T in both
passes), which the share does not credit.  For context, PyTorch-ROCm's fp32 scaled_dot_product_attention on the same values.
Net: one net(x, t) and one forward_train + backward of Unet3D_with_Conv3D(dim=64, (1, 2, 4)) at 128 x 128 x 32 frames, B = 1:
time, peak allocated memory, and the mid attention core's share (its per-launch time above over the net's time).

The shader clock and the socket power are sampled over the core part and over the net part (bench.GpuSensors).

SDC_LIB_PATH=<another build> replaces the library the package itself loads."""
import _libsel  # noqa: F401,E402  (SDC_LIB_PATH -> safediffcon_amd._lib.use_library, tools only)
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (GpuSensors: the shader clock and socket power beside the times)
import safediffcon_amd as sdc  # noqa: E402
from safediffcon_amd import grad_ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--no-net", action="store_true")
ap.add_argument("--no-sdpa", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
PEAK = 157.3e12
HEADS, INNER = 4, 32


def event_ms(fn):
    """per-call device time of fn: warm-up, then one event pair per call"""
    for _ in range(args.warmup):
        fn()
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def line(tag, ms, flops=None):
    med = statistics.median(ms)
    share = f"; {flops / (med * 1e-3) / 1e12:6.1f} TFLOP/s = {100 * flops / (med * 1e-3) / PEAK:4.1f} % of the fp32-MFMA peak" if flops else ""
    print(f"{tag}: median {med:8.3f} ms, min {min(ms):8.3f} - max {max(ms):8.3f} ms over {len(ms)} launches{share}", flush=True)
    return med


def sensors(tag, sens):
    ck = sens.stop() or {}
    print(f"{tag}: sclk median {ck.get('sclk_mhz_median')} MHz (min {ck.get('sclk_mhz_min')}, max {ck.get('sclk_mhz_max')}), "
          f"power mean {ck.get('power_w_mean')} W over {ck.get('samples')} samples", flush=True)


print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; warm-up {args.warmup}, {args.reps} timed launches each", flush=True)
core_ms = {}
sens = bench.GpuSensors(0)
sens.start()
for ntok in (400, 1024, 4096):
    for B in (1, 4):
        g = torch.Generator().manual_seed(ntok + B)
        qkv = (torch.randn(B, 384, INNER, ntok, generator=g) * 1.2).to(dev)
        gout = torch.randn(B, 128, INNER, ntok, generator=g).to(dev)
        out = torch.empty(B, 128, INNER, ntok, device=dev)
        qs, os_ = (384 * INNER * ntok, INNER * ntok, ntok, 1), (128 * INNER * ntok, INNER * ntok, ntok, 1)
        flops = 4.0 * ntok * ntok * 32 * HEADS * INNER * B
        tag = f"B={B} inner={INNER} heads={HEADS} ntok={ntok}"
        f_ms = line(f"sdc_attn      {tag}", event_ms(lambda: grad_ops.attn_core(qkv, out, HEADS, B, INNER, ntok, qs, os_)), flops)
        b_ms = line(f"sdc_attn_bwd  {tag}", event_ms(lambda: grad_ops.attn_core_bwd(qkv, gout, HEADS, B, INNER, ntok, qs, os_)), 2.5 * flops)
        core_ms[(B, ntok)] = (f_ms, b_ms)
        if not args.no_sdpa:
            try:
                q, k, v = (t.reshape(B, HEADS, 32, INNER, ntok).permute(0, 3, 1, 4, 2).contiguous().requires_grad_() for t in qkv.chunk(3, dim=1))
                go = gout.reshape(B, HEADS, 32, INNER, ntok).permute(0, 3, 1, 4, 2).contiguous()
                with torch.no_grad():
                    line(f"torch SDPA fp32 forward             {tag}", event_ms(lambda: F.scaled_dot_product_attention(q, k, v)), flops)

                def fb():
                    q.grad = k.grad = v.grad = None
                    F.scaled_dot_product_attention(q, k, v).backward(go)
                line(f"torch SDPA fp32 forward + backward  {tag}", event_ms(fb), 3.5 * flops)
                del q, k, v, go
            except Exception as e:  # noqa: BLE001  (context only: an out-of-memory math backend is a result, not a failure of this tool)
                print(f"torch SDPA fp32 {tag}: failed: {type(e).__name__}: {str(e).splitlines()[0]}", flush=True)
        del qkv, gout, out
        torch.cuda.empty_cache()

sensors("core part", sens)

if not args.no_net:
    S, FR = 128, 32
    sens = bench.GpuSensors(0)
    sens.start()
    net = sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7).to(dev)
    g = torch.Generator().manual_seed(5)
    x, t = torch.randn(1, FR, 7, S, S, generator=g).to(dev), torch.tensor([500], device=dev)
    tag = f"Unet3D_with_Conv3D(dim=64, (1,2,4)) {S} x {S} x {FR} frames B=1"
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        ms = event_ms(lambda: net(x, t))
    f_net = line(f"net(x, t)                 {tag}", ms)
    print(f"    peak allocated {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB; the mid attention core (sdc_attn, ntok = {(S // 4) ** 2}) is "
          f"{100 * core_ms[(1, (S // 4) ** 2)][0] / f_net:.1f} % of it", flush=True)
    net.train()
    tgt = torch.randn(1, FR, 7, S, S, generator=g).to(dev)

    def step():
        net.zero_grad(set_to_none=True)
        ((net.forward_train(x, t) - tgt) ** 2).mean().backward()
    torch.cuda.reset_peak_memory_stats()
    b_net = line(f"forward_train + backward  {tag}", event_ms(step))
    fm, bm = core_ms[(1, (S // 4) ** 2)]
    print(f"    peak allocated {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB; the mid attention core (sdc_attn + sdc_attn_bwd) is "
          f"{100 * (fm + bm) / b_net:.1f} % of it", flush=True)
    sensors("net part", sens)
