#!/usr/bin/env python3
"""time the temporal attention core at 64 / 128 frames (csrc/sdc_tattn_frames.hip) against another build of the library, and the
smoke net around it at 64 frames:
    python tools/tattn_frames_time.py [--reps N] [--warmup N] [--no-net] [--tag NAME]       one run of one library
    python tools/tattn_frames_time.py --collect LOG [LOG ...]                                ranges over several runs

One run loads ONE library (SDC_LIB_PATH=<another build> replaces the in-tree one: the parent's, for the A/B) and prints, per shape,
the per-launch device-event time (median, min - max over --reps launches after --warmup) and a machine-readable `RESULT` line.
An A/B is >= 5 runs of each library, interleaved on one box (parent, new, parent, new, ...), each into its own log; --collect then
prints, per shape and library, the RANGE of the runs' medians -- a shape counts as faster only where the new range lies wholly
below the parent's.

Core, as the net calls it (rot + bias, heads = 4, frame-strided dense tensors):
    forward          outer = 2, 64 frames and outer = 1, 128 frames, inner in (4096, 1024, 256)
    backward         bias given, dbias null (the parent serves this with its generic kernel; it refuses dbias past 32 frames)
    backward+dbias   the new library only
and the share of the 157.3 TFLOP/s fp32-MFMA peak: FLOPs counted are 4 ntok^2 32 per head and sequence forward (q k^T, p v) and
2.5 x that backward (the five products of the gradient; the kernels execute more -- both orientations recompute the scores).
Net: Unet3D_with_Conv3D(dim=64, (1, 2, 4)) at 64 x 64 x 64 frames, B = 1: net(x, t); forward_train + backward with peak allocated
memory where the library can run it.

The shader clock and the socket power are sampled over each part (bench.GpuSensors)."""
import argparse
import os
import re
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--no-net", action="store_true")
ap.add_argument("--tag", default=None)
ap.add_argument("--collect", nargs="+", default=None)
args = ap.parse_args()

if args.collect:
    rows = {}
    for path in args.collect:
        with open(path) as fh:
            for ln in fh:
                m = re.match(r"RESULT\t(\S+)\t(.+)\t([0-9.eE+-]+)\t([0-9.eE+-]+)\t([0-9.eE+-]+)\t(\S*)$", ln.rstrip("\n"))
                if m:
                    rows.setdefault(m.group(2), {}).setdefault(m.group(1), []).append((float(m.group(3)), m.group(6)))
    for shape, libs in rows.items():
        parts = []
        for lib, vals in libs.items():
            med = [v for v, _ in vals]
            extra = f" ({vals[0][1]})" if vals[0][1] else ""
            parts.append(f"{lib}: {min(med):8.3f} - {max(med):8.3f} ms over {len(med)} runs{extra}")
        verdict = ""
        if len(libs) == 2 and "new" in libs and "parent" in libs:
            new_hi, par_lo = max(v for v, _ in libs["new"]), min(v for v, _ in libs["parent"])
            verdict = "  -> new wholly below parent" if new_hi < par_lo else "  -> ranges overlap or new slower"
        print(f"{shape}: " + " | ".join(parts) + verdict)
    sys.exit(0)

import ctypes  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_p = os.environ.get("SDC_LIB_PATH")
if _p:
    # another build may lack entry points this tree has added: bind what it exports
    from safediffcon_amd import _lib as _l
    probe = ctypes.CDLL(os.path.abspath(_p))
    for name in [n for n in _l.SIGNATURES if not hasattr(probe, n)]:
        print(f"[tools] {_p} does not export {name}", file=sys.stderr)
        del _l.SIGNATURES[name]
import _libsel  # noqa: F401,E402  (SDC_LIB_PATH -> safediffcon_amd._lib.use_library, tools only)
import torch  # noqa: E402

import bench  # noqa: E402  (GpuSensors: the shader clock and socket power beside the times)
import safediffcon_amd as sdc  # noqa: E402
from safediffcon_amd import _lib, grad_ops  # noqa: E402

dev = torch.device("cuda:0")
PEAK = 157.3e12
HEADS = 4
TAG = args.tag or ("parent" if _p else "new")


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


def line(what, ms, flops=None, extra=""):
    med = statistics.median(ms)
    share = f"{flops / (med * 1e-3) / 1e12:.1f} TFLOP/s = {100 * flops / (med * 1e-3) / PEAK:.1f} % of the fp32-MFMA peak" if flops else extra
    print(f"{what}: median {med:8.3f} ms, min {min(ms):8.3f} - max {max(ms):8.3f} ms over {len(ms)} launches; {share}", flush=True)
    print(f"RESULT\t{TAG}\t{what}\t{med:.4f}\t{min(ms):.4f}\t{max(ms):.4f}\t{share.replace(' ', '_')}", flush=True)
    return med


def sensors(tag, sens):
    ck = sens.stop() or {}
    print(f"{tag}: sclk median {ck.get('sclk_mhz_median')} MHz (min {ck.get('sclk_mhz_min')}, max {ck.get('sclk_mhz_max')}), "
          f"power mean {ck.get('power_w_mean')} W over {ck.get('samples')} samples", flush=True)


print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; library {TAG}; warm-up {args.warmup}, {args.reps} timed launches each",
      flush=True)
lib = _lib.get_lib()
sens = bench.GpuSensors(0)
sens.start()
for ntok, outer in ((64, 2), (128, 1)):
    fr = 1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))
    ang = torch.arange(ntok, dtype=torch.float32)[:, None] * fr[None, :]
    rot = torch.stack((ang.cos(), ang.sin()), dim=-1).reshape(-1).to(dev)
    for inner in (4096, 1024, 256):
        g = torch.Generator().manual_seed(ntok + inner)
        qkv = torch.randn(outer, 384, ntok, inner, generator=g).to(dev)
        gout = torch.randn(outer, 128, ntok, inner, generator=g).to(dev)
        bias = (0.5 * torch.randn(HEADS, ntok, ntok, generator=g)).to(dev)
        out, dqkv, dbias = torch.empty_like(gout), torch.empty_like(qkv), torch.empty_like(bias)
        qs, os_ = (384 * ntok * inner, ntok * inner, 1, inner), (128 * ntok * inner, ntok * inner, 1, inner)
        flops = 4.0 * ntok * ntok * 32 * HEADS * inner * outer
        shape = f"outer={outer} inner={inner} heads={HEADS} frames={ntok}"
        stream = torch.cuda.current_stream(dev).cuda_stream
        line(f"sdc_attn {shape}", event_ms(lambda: grad_ops.attn_core(qkv, out, HEADS, outer, inner, ntok, qs, os_, rot, bias)), flops)

        def bwd(db, wk):
            rc = lib.sdc_attn_bwd(qkv.data_ptr(), gout.data_ptr(), rot.data_ptr(), bias.data_ptr(), dqkv.data_ptr(), db, wk, outer, inner,
                                  HEADS, ntok, *qs, *os_, stream)
            if rc != 0:
                raise _lib.SdcError(_lib.last_error())
        line(f"sdc_attn_bwd dbias=null {shape}", event_ms(lambda: bwd(0, 0)), 2.5 * flops)
        work = torch.empty(int(lib.sdc_attn_bwd_bytes(outer, inner, HEADS, ntok)) // 4, device=dev)
        try:
            line(f"sdc_attn_bwd dbias {shape}", event_ms(lambda: bwd(dbias.data_ptr(), work.data_ptr())), 2.5 * flops)
        except _lib.SdcError as e:
            print(f"sdc_attn_bwd dbias {shape}: refused: {e}", flush=True)
        del qkv, gout, out, dqkv, work
        torch.cuda.empty_cache()
sensors("core part", sens)

if not args.no_net:
    S, FR = 64, 64
    sens = bench.GpuSensors(0)
    sens.start()
    net = sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7).to(dev)
    g = torch.Generator().manual_seed(5)
    x, t = torch.randn(1, FR, 7, S, S, generator=g).to(dev), torch.tensor([500], device=dev)
    shape = f"Unet3D_with_Conv3D(dim=64, (1,2,4)) {S} x {S} x {FR} frames B=1"
    with torch.no_grad():
        line(f"net(x, t) {shape}", event_ms(lambda: net(x, t)))
    net.train()
    tgt = torch.randn(1, FR, 7, S, S, generator=g).to(dev)

    def step():
        net.zero_grad(set_to_none=True)
        ((net.forward_train(x, t) - tgt) ** 2).mean().backward()
    torch.cuda.reset_peak_memory_stats()
    try:
        ms = event_ms(step)
        line(f"forward_train + backward {shape}", ms, extra=f"peak allocated {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    except _lib.SdcError as e:
        print(f"forward_train + backward {shape}: refused: {str(e).splitlines()[0]}", flush=True)
    sensors("net part", sens)
