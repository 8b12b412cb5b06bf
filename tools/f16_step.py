#!/usr/bin/env python3
"""Same-box A/B of conv precision 4 (fp32 Winograd) against 6 (fp16 operands on the 3-tap convs, csrc/sdc_conv_f16.hip).

  python tools/f16_step.py [--workloads c4,c2,c3] [--steps 20] [--warmup 5] [--rounds 2] [--arm 6|7]
      sampler step of bench.workload(..., precision=4 / arm) (bench.py itself unchanged), the two arms interleaved round by round;
      ms/step with the shader clock and socket power sampled over each timed region (bench.GpuSensors)
  python tools/f16_step.py --shapes [--workloads ...]
      every conv of the nets' forward plans that the fp16 kernel covers (precision 7: no dispatch table): sdc_conv / sdc_conv_gn
      at precision 4 against 7 on the same buffers, median of 20 launches each -- the data of precision 6's dispatch table
      (csrc/sdc_conv_f16.hip f16_faster)
  python tools/f16_step.py --drift [T] [--stem]
      T-step (default 1000) guided smoke trajectories at production width, B = 2, identical Philox noise, precisions 6 and 7
      against 4; with --stem: precision 4 + net.stem_f16 and 6 + net.stem_f16 against 4 instead
  python tools/f16_step.py --stem [--workloads c4,c2] [--steps 20] [--warmup 5] [--rounds 2] [--no-step]
      net.stem_f16 (csrc/sdc_conv_stem_f16.hip): the stem conv of the C4 / C2 plans, today's kernel (sdc_conv at precision 4) against
      sdc_conv_stem_f16 on the same buffers, median of 20 launches each; then the C4 sampler step, precision 4 against 4 + stem_f16
      and 6 against 6 + stem_f16, the four arms interleaved round by round
  python tools/f16_step.py --split [--workloads c4,c2] [--steps 20] [--warmup 5] [--rounds 3] [--no-step]
      net.stem_split (csrc/sdc_conv_stem_x3.hip, default on): the same stem launches, today's fp32 kernel against sdc_conv_stem_x3 (the
      medians of three interleaved repeats, so that their spread shows); then the C4 sampler step with the switch off against on
  python tools/f16_step.py --gemm [--workloads c4,c2,c3] [--steps 20] [--warmup 5] [--rounds 3] [--no-step]
      net.gemm_split (csrc/sdc_conv_gemm_x3.hip, default on): every conv of the nets' forward plans that conv_gemm_x3_kernel covers
      (strided (1,4,4), sub-pixel (1,2,2), 1x1x1; routed or not), sdc_conv at precision 4 against sdc_conv_gemm_x3 on the same buffers, the
      medians of 20 launches in three interleaved repeats -- the data of the routing table (sdc_conv_gemm_x3_ok, DESIGN section 15: a
      shape qualifies when every repeat beats every repeat of the fp32 kernel); then the C4 sampler step with the switch off against on
  python tools/f16_step.py --pw-split [--workloads c4,c2,c3] [--no-step]
      conv_pw_x3_kernel (csrc/sdc_conv_pw_x3.hip): every 1x1 conv of the nets' forward plans that sdc_conv_pw_x3 accepts
      (listed or not), sdc_conv at precision 3 (a 1x1 descriptor at 2 or 3 keeps the fp32 kernel the parent runs) against sdc_conv_pw_x3 on the same buffers,
      the medians of 20 launches in three interleaved repeats at the bench batch and at B = 2 -- the data of the routing table
      (sdc_conv_pw_x3_ok: a shape qualifies when every repeat beats every repeat of the fp32 kernel at the bench batch); then the C4 and
      C2 steps of this build (sdc_conv carries no switch: the step's A/B is by commit, SDC_LIB_PATH naming the parent's library)
  python tools/f16_step.py --wino [--steps 20] [--warmup 5] [--rounds 3] [--no-step]
      net.wino_split (csrc/sdc_conv_wino_x3.hip): every 3x3x3 conv of the C4 switch-off plan that conv_wg3_x3_kernel covers (routed or
      not), sdc_conv / sdc_conv_gn at precision 4 against sdc_conv_wino3_x3 on the same buffers (GroupNorm sums in both where the plan
      has them), the medians of 20 launches in three interleaved repeats -- the data of the routing table (sdc_conv_wino3_x3_ok, DESIGN
      section 18: a shape qualifies when every repeat beats every repeat of the fp32 kernel); then the C4 sampler step with the switch
      off against on
  python tools/f16_step.py --attn [--steps 20] [--warmup 5] [--rounds 3] [--no-step]
      net.attn_f16 (csrc/sdc_tablock_f16.hip): the fused temporal-attention block at the C4 site shape (64, 64, 32, 64, 64) and at B = 2,
      sdc_tattn_block against sdc_tattn_block_f16 on the same buffers, the medians of 20 launches in three interleaved repeats (the rule of
      DESIGN section 15: faster only if every repeat beats every repeat of the fp32 kernel); then the C4 sampler step, precision 4
      against 4 + attn_f16 and 6 + stem_f16 against 6 + stem_f16 + attn_f16, the four arms interleaved round by round
  python tools/f16_step.py --drift [T] --attn
      the T-step guided smoke trajectories with precision 4 + net.attn_f16 against 4
  python tools/f16_step.py --linattn [--workloads c4,c2] [--steps 20] [--warmup 5] [--rounds 3] [--no-step]
      net.linattn_f16 (csrc/sdc_lablock_f16.hip): the fused LinearAttention block at the C4 sites (B = 64: C 64, n 4096, 32 frames, the
      plain and the GroupNorm-on-load form; C 128, n 1024), the C2 sites (B = 256: C 64, n 2048; C 128, n 512) and at B = 2,
      sdc_linattn_block / _gn against sdc_linattn_block_f16 / _gn_f16 on the same buffers, the medians of 20 launches in three interleaved
      repeats (the rule of DESIGN section 15); then the C4 sampler step, precision 4 against 4 + linattn_f16 and 6 + stem_f16 + attn_f16
      against the same + linattn_f16, the four arms interleaved round by round, and the C2 step, 4 against 4 + linattn_f16
  python tools/f16_step.py --linattn-split [--no-step]
      the fused LinearAttention block with its q / k projections as exact bf16 splits (csrc/sdc_lablock_x3.hip):
      sdc_linattn_block_sel / _gn_sel with impl 0 against impl 1 on the same buffers at the sites of --linattn, the medians of 20
      launches in three interleaved repeats; a size qualifies for sdc_linattn_block_x3_ok when every repeat beats every repeat
  python tools/f16_step.py --drift [T] --linattn
      the T-step guided smoke trajectories with precision 4 + net.linattn_f16 against 4
  python tools/f16_step.py --attn-split [--steps 20] [--warmup 5] [--rounds 3] [--no-step]
      net.attn_split (csrc/sdc_tablock_x3.hip): the fused temporal-attention block at the sites of the dim-64 smoke net -- 64 x 64 pixels
      per sample at B = 64 (the C4 site) and B = 2, 32 x 32 and 16 x 16 at B = 64 --, sdc_tattn_block against sdc_tattn_block_x3 on the same
      buffers, the medians of 20 launches in three interleaved repeats -- the data of the routing table (sdc_tattn_block_x3_ok, DESIGN
      section 19: a shape qualifies when every repeat beats every repeat of the fp32 kernel); then the C4 sampler step with the switch
      off against on
  python tools/f16_step.py --attn-skew [--no-step]
      the skewed form of that block (ta_block_x3s_kernel): sdc_tattn_block_x3_sel with impl 0 against impl 1 on the
      same buffers at 64 x 64 (B = 64 and B = 2) and 32 x 32 (B = 64), the medians of 20 launches in three interleaved repeats; a size
      qualifies for sdc_tattn_block_x3_impl when every repeat of impl 1 beats every repeat of impl 0 at the bench batch
"""
import _libsel  # noqa: F401  (SDC_LIB_PATH -> safediffcon_amd._lib.use_library, tools only)
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import safediffcon_amd as sdc  # noqa: E402
from safediffcon_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")


def step_ab(names, steps, warmup, rounds, arm=6, arms=None):
    """arms: the precisions timed, interleaved; a string 'P+stem' is precision P with net.stem_f16, 'P+attn' with net.attn_f16 (both:
    'P+stem+attn'), 'P+la' with net.linattn_f16, 'P-nosplit' precision P with net.stem_split off, 'P-nogemm' precision P with net.gemm_split off, 'P-nowino' / 'P+wino' precision P
    with net.wino_split off / on, 'P-noasplit' / 'P+asplit' with net.attn_split off / on (default: 4 against `arm`)"""
    torch.cuda.set_device(DEV)
    side = torch.cuda.Stream(device=DEV)
    arms = list(arms or (4, arm))
    for name in names:
        B = bench.DEFAULT_B[name]
        loops = {}
        with torch.cuda.stream(side), torch.no_grad():
            for prec in arms:
                tag = str(prec)
                W = bench.workload(name, None, B, DEV, 0, 1, precision=int(tag.split("+")[0].split("-")[0]), cal_steps=0)
                W["gd"].model.stem_f16 = "+stem" in tag                 # (read when prep() builds the sampler's plan)
                W["gd"].model.attn_f16 = "+attn" in tag
                W["gd"].model.linattn_f16 = "+la" in tag
                W["gd"].model.stem_split = not tag.endswith("-nosplit")
                W["gd"].model.gemm_split = not tag.endswith("-nogemm")
                if tag.endswith("-noasplit") or "+asplit" in tag:
                    W["gd"].model.attn_split = "+asplit" in tag
                if tag.endswith("-nowino") or "+wino" in tag:
                    W["gd"].model.wino_split = "+wino" in tag
                torch.manual_seed(2)
                S = W["prep"]()
                S.init()
                loops[prec] = S
            res = {p: [] for p in arms}
            for r in range(rounds):
                for prec in (arms if r % 2 == 0 else arms[::-1]):
                    S = loops[prec]

                    def run(n):
                        for _ in range(n):
                            if S.t_host < (0 if S.impose_last else 1):
                                S.init()
                            S.step()
                    run(warmup)
                    torch.cuda.synchronize()
                    sens = bench.GpuSensors(0)
                    sens.start()
                    t0 = time.perf_counter()
                    run(steps)
                    torch.cuda.synchronize()
                    ms = (time.perf_counter() - t0) * 1e3 / steps
                    ck = sens.stop() or {}
                    res[prec].append(ms)
                    print(f"[measured] {name} B={B} precision {prec} round {r}: {ms:.2f} ms/step  sclk median "
                          f"{ck.get('sclk_mhz_median')} MHz (min {ck.get('sclk_mhz_min')})  power mean {ck.get('power_w_mean')} W "
                          f"(max {ck.get('power_w_max')})", flush=True)
            for base, other in zip(arms[0::2], arms[1::2]):
                m4, mx = statistics.median(res[base]), statistics.median(res[other])
                print(f"[measured] {name}: precision {other} / {base} = {mx:.2f} / {m4:.2f} ms/step = {mx / m4:.3f}", flush=True)
            for S in loops.values():
                S.close()
        del loops
        torch.cuda.empty_cache()


def _time_call(fn, args, stream, n=20):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for _ in range(3):
        _lib.check(fn(*args, stream), fn.__name__)
    ts = []
    for a, b in evs:
        a.record()
        _lib.check(fn(*args, stream), fn.__name__)
        b.record()
    torch.cuda.synchronize()
    for a, b in evs:
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def shapes(names):
    lib = _lib.get_lib()
    stream = torch.cuda.current_stream().cuda_stream
    nets = {
        "c4": (lambda: sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7), (64, 32, 7, 64, 64)),
        "c2": (lambda: sdc.Unet2D(dim=64, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1), (256, 3, 16, 128)),
        "c3": (lambda: sdc.Unet1D(dim=256, dim_mults=(1, 2, 4, 8), channels=12, resnet_block_groups=1), (128, 12, 128)),
    }
    name_buf = C.create_string_buffer(96)
    share = C.c_double(0.0)
    for wl in names:
        make, shape = nets[wl]
        torch.manual_seed(0)
        net = make().to(DEV)
        net.precision = 7
        x = torch.randn(shape, device=DEV) * 0.5
        t = torch.full((shape[0],), 500, device=DEV, dtype=torch.long)
        with torch.no_grad():
            net(x, t)
            plan = net.entry(tuple(shape), shape[0])["plan"]
        seen, tot4, tot7 = set(), 0.0, 0.0
        for fn, args in plan.calls:
            if fn.__name__ not in ("sdc_conv", "sdc_conv_gn"):
                continue
            d6 = args[0]._obj
            lib.sdc_conv_describe(C.byref(d6), name_buf, 96, C.byref(share))
            kname = name_buf.value.decode()
            if "f16" not in kname:
                continue
            key = (d6.kD, d6.kH, d6.kW, d6.Cin0, d6.Cin1, d6.Cout, d6.B, d6.oD, d6.oH, d6.oW, d6.rs[1] != 0, fn.__name__)
            d4 = type(d6).from_buffer_copy(d6)
            d4.precision = 4
            lib.sdc_conv_describe(C.byref(d4), name_buf, 96, C.byref(share))
            k4name = name_buf.value.decode()
            ms = {}
            for prec, d in ((4, d4), (7, d6)):
                if fn.__name__ == "sdc_conv_gn":
                    G = args[8]
                    nparts = int(lib.sdc_conv_gnparts(C.byref(d), G))
                    if nparts > 0:
                        parts = torch.empty(d.B * G * nparts * 2, dtype=torch.float64, device=DEV)
                        ms[prec] = _time_call(lib.sdc_conv_gn, (C.byref(d), *args[1:7], parts.data_ptr(), G), stream)
                        continue
                ms[prec] = _time_call(lib.sdc_conv, (C.byref(d), *args[1:7]), stream)
            flop = 2.0 * d6.B * d6.oD * d6.oH * d6.oW * d6.Cout * (d6.Cin0 + d6.Cin1) * d6.kD * d6.kH * d6.kW
            tot4 += ms[4]
            tot7 += ms[7]
            tag = "" if key not in seen else " (repeat)"
            seen.add(key)
            print(f"[measured] {wl} {d6.kD}x{d6.kH}x{d6.kW} Cin {d6.Cin0}+{d6.Cin1} Cout {d6.Cout} B {d6.B} {d6.oD}x{d6.oH}x{d6.oW} "
                  f"res {int(d6.rs[1] != 0)} {fn.__name__}: p4 {k4name} {ms[4] * 1e3:.1f} us | p7 {kname} {ms[7] * 1e3:.1f} us "
                  f"({flop / ms[7] / 1e9:.0f} TFLOP/s direct-form) -> x{ms[4] / ms[7]:.2f}{tag}", flush=True)
        print(f"[measured] {wl}: the fp16-covered convs of one forward: p4 {tot4:.2f} ms, p7 {tot7:.2f} ms", flush=True)
        del net, plan
        torch.cuda.empty_cache()


def stem_shapes(names, split=False):
    """the stem conv of the C4 / C2 sampler plans: sdc_conv at precision 4 (today's kernel) against sdc_conv_stem_f16 -- split: against
    sdc_conv_stem_x3 --, same buffers"""
    from safediffcon_amd.engine import as5, conv_desc, pack_conv_weight, pack_stem_f16, pack_stem_x3
    lib = _lib.get_lib()
    stream = torch.cuda.current_stream().cuda_stream
    forms = {   # the state as the net hands it to init_conv, weight shape
        "c4": (lambda: (torch.randn(64, 32, 7, 64, 64, device=DEV) * 0.5).permute(0, 2, 1, 3, 4), (64, 7, 7, 7, 7)),
        "c2": (lambda: as5(torch.randn(256, 3, 16, 128, device=DEV) * 0.5), (64, 3, 1, 7, 7)),
    }
    name_buf = C.create_string_buffer(96)
    share = C.c_double(0.0)
    for wl in names:
        if wl not in forms:
            print(f"{wl}: no 7-tap stem that the fp16 kernel covers (c4, c2)", flush=True)
            continue
        torch.manual_seed(0)
        x = forms[wl][0]()
        co, ci, *k = forms[wl][1]
        w = torch.randn(co, ci, *k, device=DEV) / (ci * k[0] * k[1] * k[2]) ** 0.5
        bias = torch.randn(co, device=DEV) * 0.1
        y4 = torch.empty(x.shape[0], co, *x.shape[2:], device=DEV)
        yh = torch.empty_like(y4)
        d = conv_desc(x, None, y4, None, co, tuple(k), (1, 1, 1), tuple(kk // 2 for kk in k), (1, 1, 1), 0, 4)
        if not lib.sdc_conv_stem_f16_ok(C.byref(d)):
            print(f"{wl}: stem not covered", flush=True)
            continue
        wp, wh = pack_conv_weight(w, precision=4), pack_stem_f16(w)
        lib.sdc_conv_describe(C.byref(d), name_buf, 96, C.byref(share))
        npos = d.B * d.oD * d.oH * d.oW
        flop = 2.0 * npos * co * ci * k[0] * k[1] * k[2]
        if split:
            wb = pack_stem_x3(w)
            m4, mx = [], []
            for _ in range(3):      # interleaved repeats of the median of 20: their spread is what a gain has to beat
                m4.append(_time_call(lib.sdc_conv, (C.byref(d), x.data_ptr(), 0, wp.data_ptr(), bias.data_ptr(), 0, y4.data_ptr()), stream))
                mx.append(_time_call(lib.sdc_conv_stem_x3, (C.byref(d), x.data_ptr(), wb.data_ptr(), bias.data_ptr(), yh.data_ptr()), stream))
            ref = torch.nn.functional.conv3d(x[:1].double(), w.double(), bias.double(), padding=tuple(kk // 2 for kk in k))
            rms = ref.pow(2).mean().sqrt().item()
            e4, ex = ((y[:1].double() - ref).pow(2).mean().sqrt().item() / rms for y in (y4, yh))
            a4, ax = statistics.median(m4), statistics.median(mx)
            print(f"[measured] {wl} stem {k[0]}x{k[1]}x{k[2]} Cin {ci} Cout {co} B {d.B} {d.oD}x{d.oH}x{d.oW}: today {name_buf.value.decode()} "
                  f"{' / '.join(f'{v * 1e3:.1f}' for v in m4)} us ({flop / a4 / 1e9:.0f} TFLOP/s) | conv_stem_x3_kernel "
                  f"{' / '.join(f'{v * 1e3:.1f}' for v in mx)} us ({flop / ax / 1e9:.0f} TFLOP/s direct-form) -> x{a4 / ax:.2f}; rms error "
                  f"against fp64 on sample 0, of the output rms: today {e4:.2e}, split {ex:.2e}", flush=True)
            del x, y4, yh, ref
            torch.cuda.empty_cache()
            continue
        ms4 = _time_call(lib.sdc_conv, (C.byref(d), x.data_ptr(), 0, wp.data_ptr(), bias.data_ptr(), 0, y4.data_ptr()), stream)
        msh = _time_call(lib.sdc_conv_stem_f16, (C.byref(d), x.data_ptr(), wh.data_ptr(), bias.data_ptr(), yh.data_ptr()), stream)
        issued = 2.0 * npos * co * k[0] * ((k[1] * 7 + 1) // 2) * 16
        err = (yh - y4).pow(2).mean().sqrt().item() / y4.pow(2).mean().sqrt().item()
        print(f"[measured] {wl} stem {k[0]}x{k[1]}x{k[2]} Cin {ci} Cout {co} B {d.B} {d.oD}x{d.oH}x{d.oW}: today {name_buf.value.decode()} "
              f"{ms4 * 1e3:.1f} us ({flop / ms4 / 1e9:.0f} TFLOP/s) | conv_stem_f16_kernel {msh * 1e3:.1f} us ({flop / msh / 1e9:.0f} TFLOP/s "
              f"direct-form, {issued / msh / 1e9:.0f} issued) -> x{ms4 / msh:.2f}; rms difference {err:.2e} of the output rms", flush=True)
        del x, y4, yh
        torch.cuda.empty_cache()


def gemm_shapes(names):
    """every conv of the switch-off forward plans that sdc_conv_gemm_x3 accepts: today's kernel against it, same buffers"""
    from safediffcon_amd.engine import pack_gemm_x3
    lib = _lib.get_lib()
    stream = torch.cuda.current_stream().cuda_stream
    nets = {
        "c4": (lambda: sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7), (64, 32, 7, 64, 64)),
        "c2": (lambda: sdc.Unet2D(dim=64, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1), (256, 3, 16, 128)),
        "c3": (lambda: sdc.Unet1D(dim=256, dim_mults=(1, 2, 4, 8), channels=12, resnet_block_groups=1), (128, 12, 128)),
    }
    name_buf = C.create_string_buffer(96)
    share = C.c_double(0.0)
    for wl in names:
        make, shape = nets[wl]
        torch.manual_seed(0)
        net = make().to(DEV)
        net.gemm_split = False
        x = torch.randn(shape, device=DEV) * 0.5
        t = torch.full((shape[0],), 500, device=DEV, dtype=torch.long)
        with torch.no_grad():
            net(x, t)
            plan = net.entry(tuple(shape), shape[0])["plan"]
        by_ptr = {k.data_ptr(): k for k in plan.keep if isinstance(k, torch.Tensor)}
        seen, tot4, totx, totq = {}, 0.0, 0.0, 0.0
        for fn, args in plan.calls:
            if fn.__name__ != "sdc_conv":
                continue
            d = args[0]._obj
            if (d.kH, d.kW) not in ((4, 4), (2, 2), (1, 1)) or d.Cin1 or d.rs[1] or d.Cout % 64:
                continue
            key = (d.kH, d.kW, d.sH, d.pH, d.pW, d.Cin0, d.Cout, d.oD, d.oH, d.oW)
            ncb = {4: 1, 2: 2, 1: 4}[d.kH]
            if d.Cin0 % (16 * ncb) or int(lib.sdc_pack_gemm_x3_bytes(d.Cout, d.Cin0, d.kH, d.kW)) == 0:
                continue
            wp = by_ptr[args[3]]
            wb = pack_gemm_x3(wp[:d.kH * d.kW * d.Cin0 * d.Cout].reshape(-1, d.Cout), d.Cout, d.Cin0, (d.kH, d.kW)).to(DEV)
            y4 = torch.empty(d.B * d.Cout * d.oD * d.oH * d.oW * 4 + 64, device=DEV)        # (a parity view spans 4x its elements)
            rc = lib.sdc_conv_gemm_x3(C.byref(d), args[1], wb.data_ptr(), args[4], y4.data_ptr(), stream)
            if rc != 0:
                print(f"{wl} {d.kH}x{d.kW} Cin {d.Cin0} Cout {d.Cout} {d.oD}x{d.oH}x{d.oW}: not covered ({_lib.last_error()})", flush=True)
                continue
            lib.sdc_conv_describe(C.byref(d), name_buf, 96, C.byref(share))
            m4, mx = [], []
            for _ in range(3):      # interleaved repeats of the median of 20: their spread is what a gain has to beat
                m4.append(_time_call(lib.sdc_conv, (C.byref(d), args[1], 0, args[3], args[4], 0, y4.data_ptr()), stream))
                mx.append(_time_call(lib.sdc_conv_gemm_x3, (C.byref(d), args[1], wb.data_ptr(), args[4], y4.data_ptr()), stream))
            flop = 2.0 * d.B * d.oD * d.oH * d.oW * d.Cout * d.Cin0 * d.kH * d.kW
            a4, ax = statistics.median(m4), statistics.median(mx)
            q = max(mx) < min(m4)
            tot4 += a4
            totx += ax
            totq += ax if q else a4
            seen[key] = seen.get(key, 0) + 1
            print(f"[measured] {wl} {d.kD}x{d.kH}x{d.kW} stride {d.sH} pad {d.pH},{d.pW} Cin {d.Cin0} Cout {d.Cout} B {d.B} {d.oD}x{d.oH}x{d.oW}: "
                  f"today {name_buf.value.decode()} {' / '.join(f'{v * 1e3:.1f}' for v in m4)} us ({flop / a4 / 1e9:.0f} TFLOP/s) | "
                  f"conv_gemm_x3_kernel {' / '.join(f'{v * 1e3:.1f}' for v in mx)} us ({flop / ax / 1e9:.0f} TFLOP/s direct-form) -> x{a4 / ax:.2f} "
                  f"{'QUALIFIES' if q else 'stays'}; table says {int(lib.sdc_conv_gemm_x3_ok(C.byref(d)))}"
                  f"{' (repeat)' if seen[key] > 1 else ''}", flush=True)
            del y4, wb
        print(f"[measured] {wl}: the covered convs of one forward: fp32 kernels {tot4:.2f} ms, split {totx:.2f} ms, "
              f"qualifying ones routed {totq:.2f} ms", flush=True)
        del net, plan, by_ptr
        torch.cuda.empty_cache()


def pw_shapes(names):
    """every 1x1 conv of the forward plans that sdc_conv_pw_x3 accepts: the fp32 kernel (sdc_conv at precision 3) against it, same buffers"""
    lib = _lib.get_lib()
    stream = torch.cuda.current_stream().cuda_stream
    nets = {
        "c4": (lambda: sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7), (64, 32, 7, 64, 64)),
        "c2": (lambda: sdc.Unet2D(dim=64, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1), (256, 3, 16, 128)),
        "c3": (lambda: sdc.Unet1D(dim=256, dim_mults=(1, 2, 4, 8), channels=12, resnet_block_groups=1), (128, 12, 128)),
    }
    name_buf = C.create_string_buffer(96)
    share = C.c_double(0.0)
    for wl in names:
        make, shape = nets[wl]
        torch.manual_seed(0)
        net = make().to(DEV)
        x = torch.randn(shape, device=DEV) * 0.5
        t = torch.full((shape[0],), 500, device=DEV, dtype=torch.long)
        with torch.no_grad():
            net(x, t)
            plan = net.entry(tuple(shape), shape[0])["plan"]
        seen, tot0, totx, totq = {}, 0.0, 0.0, 0.0
        for fn, args in plan.calls:
            if fn.__name__ != "sdc_conv":
                continue
            d = args[0]._obj
            if d.kD * d.kH * d.kW != 1:
                continue
            key = (d.Cin0, d.Cin1, d.Cout, d.oD, d.oH, d.oW, int(bool(args[5])))
            desc = f"{wl} 1x1x1 Cin {d.Cin0}+{d.Cin1} Cout {d.Cout} {d.oD}x{d.oH}x{d.oW} res {key[-1]}"
            rows = []
            for B in (d.B, 2):
                d0, dx = type(d).from_buffer_copy(d), type(d).from_buffer_copy(d)          # (the first B samples of the same buffers)
                d0.B = dx.B = B
                d0.precision = 3                                # (never routed to the split kernel: the name is printed)
                rest = tuple(args[1:7])
                rc = lib.sdc_conv_pw_x3(C.byref(dx), *rest, stream)
                if rc != 0:
                    print(f"{desc}: not covered ({_lib.last_error()})", flush=True)
                    rows = None
                    break
                lib.sdc_conv_describe(C.byref(d0), name_buf, 96, C.byref(share))
                m0, mx = [], []
                for _ in range(3):      # interleaved repeats of the median of 20: their spread is what a gain has to beat
                    m0.append(_time_call(lib.sdc_conv, (C.byref(d0), *rest), stream))
                    mx.append(_time_call(lib.sdc_conv_pw_x3, (C.byref(dx), *rest), stream))
                rows.append((B, name_buf.value.decode(), m0, mx))
            if rows is None:
                continue
            (B, kname, m0, mx), (_, kname2, n0, nx) = rows
            flop = 2.0 * B * d.oD * d.oH * d.oW * d.Cout * (d.Cin0 + d.Cin1)
            a0, ax = statistics.median(m0), statistics.median(mx)
            q = max(mx) < min(m0)
            tot0 += a0
            totx += ax
            totq += ax if q else a0
            seen[key] = seen.get(key, 0) + 1
            print(f"[measured] {desc} B {B}: fp32 {kname} {' / '.join(f'{v * 1e3:.1f}' for v in m0)} us ({flop / a0 / 1e9:.0f} TFLOP/s) | "
                  f"conv_pw_x3_kernel {' / '.join(f'{v * 1e3:.1f}' for v in mx)} us ({flop / ax / 1e9:.0f} TFLOP/s direct-form) -> x{a0 / ax:.2f} "
                  f"{'QUALIFIES' if q else 'stays'}; B 2: {kname2} {' / '.join(f'{v * 1e3:.1f}' for v in n0)} | "
                  f"{' / '.join(f'{v * 1e3:.1f}' for v in nx)} us -> x{statistics.median(n0) / statistics.median(nx):.2f}; "
                  f"table says {int(lib.sdc_conv_pw_x3_ok(C.byref(d)))}{' (repeat)' if seen[key] > 1 else ''}", flush=True)
        print(f"[measured] {wl}: the covered 1x1 convs of one forward: fp32 kernels {tot0:.2f} ms, split {totx:.2f} ms, "
              f"qualifying ones routed {totq:.2f} ms", flush=True)
        del net, plan
        torch.cuda.empty_cache()


def wino_shapes():
    """every 3x3x3 conv of the C4 switch-off forward plan that sdc_conv_wino3_x3 accepts: today's kernel against it, same buffers"""
    from safediffcon_amd.engine import pack_wino3_x3
    lib = _lib.get_lib()
    stream = torch.cuda.current_stream().cuda_stream
    shape = (64, 32, 7, 64, 64)
    name_buf = C.create_string_buffer(96)
    share = C.c_double(0.0)
    torch.manual_seed(0)
    net = sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7).to(DEV)
    net.wino_split = False
    x = torch.randn(shape, device=DEV) * 0.5
    t = torch.full((shape[0],), 500, device=DEV, dtype=torch.long)
    with torch.no_grad():
        net(x, t)
        plan = net.entry(tuple(shape), shape[0])["plan"]
    by_ptr = {k.data_ptr(): k for k in plan.keep if isinstance(k, torch.Tensor)}
    seen, tot4, totx, totq = {}, 0.0, 0.0, 0.0
    for fn, args in plan.calls:
        if fn.__name__ not in ("sdc_conv", "sdc_conv_gn"):
            continue
        d = args[0]._obj
        if (d.kD, d.kH, d.kW) != (3, 3, 3) or args[5] or int(lib.sdc_pack_wino3_x3_bytes(d.Cout, d.Cin0 + d.Cin1)) == 0:
            continue
        key = (d.Cin0, d.Cin1, d.Cout, d.oD, d.oH, d.oW, fn.__name__)
        cin = d.Cin0 + d.Cin1
        G = args[8] if fn.__name__ == "sdc_conv_gn" else 0
        nparts = int(lib.sdc_conv_gnparts(C.byref(d), G)) if G else 0
        parts = torch.empty(max(1, d.B * G * nparts * 2), dtype=torch.float64, device=DEV)
        y4 = torch.empty(d.B, d.Cout, d.oD, d.oH, d.oW, device=DEV)
        yx = torch.empty_like(y4)
        wb = pack_wino3_x3(by_ptr[args[3]].cpu(), d.Cout, cin).to(DEV)
        ax_args = (C.byref(d), args[1], args[2], wb.data_ptr(), args[4], yx.data_ptr(), parts.data_ptr() if nparts else 0, G if nparts else 0)
        rc = lib.sdc_conv_wino3_x3(*ax_args, stream)
        if rc != 0:
            print(f"c4 3x3x3 Cin {d.Cin0}+{d.Cin1} Cout {d.Cout} {d.oD}x{d.oH}x{d.oW}: not covered ({_lib.last_error()})", flush=True)
            continue
        a4_fn = lib.sdc_conv_gn if nparts else lib.sdc_conv
        a4_args = (C.byref(d), args[1], args[2], args[3], args[4], 0, y4.data_ptr()) + ((parts.data_ptr(), G) if nparts else ())
        lib.sdc_conv_describe(C.byref(d), name_buf, 96, C.byref(share))
        m4, mx = [], []
        for _ in range(3):      # interleaved repeats of the median of 20: their spread is what a gain has to beat
            m4.append(_time_call(a4_fn, a4_args, stream))
            mx.append(_time_call(lib.sdc_conv_wino3_x3, ax_args, stream))
        err = (yx - y4).double().pow(2).mean().sqrt().item() / y4.double().pow(2).mean().sqrt().item()
        flop = 2.0 * d.B * d.oD * d.oH * d.oW * d.Cout * cin * 27
        a4, ax = statistics.median(m4), statistics.median(mx)
        q = max(mx) < min(m4)
        tot4 += a4
        totx += ax
        totq += ax if q else a4
        seen[key] = seen.get(key, 0) + 1
        print(f"[measured] c4 3x3x3 Cin {d.Cin0}+{d.Cin1} Cout {d.Cout} B {d.B} {d.oD}x{d.oH}x{d.oW} {fn.__name__}: today {name_buf.value.decode()} "
              f"{' / '.join(f'{v * 1e3:.1f}' for v in m4)} us ({flop / a4 / 1e9:.0f} TFLOP/s direct-form) | conv_wg3_x3_kernel "
              f"{' / '.join(f'{v * 1e3:.1f}' for v in mx)} us ({flop / ax / 1e9:.0f} TFLOP/s direct-form, {flop * 8 / 27 * 6 / ax / 1e9:.0f} issued on the "
              f"bf16 pipe) -> x{a4 / ax:.2f} {'QUALIFIES' if q else 'stays'}; table says {int(lib.sdc_conv_wino3_x3_ok(C.byref(d)))}; "
              f"rms difference {err:.2e} of the output rms{' (repeat)' if seen[key] > 1 else ''}", flush=True)
        del y4, yx, wb, parts
    print(f"[measured] c4: the covered 3x3x3 convs of one forward: fp32 kernels {tot4:.2f} ms, split {totx:.2f} ms, "
          f"qualifying ones routed {totq:.2f} ms", flush=True)
    del net, plan, by_ptr
    torch.cuda.empty_cache()


def attn_shapes():
    """the fused temporal-attention block at the C4 site shape and at B = 2: sdc_tattn_block against sdc_tattn_block_f16, same buffers"""
    from safediffcon_amd.engine import pack_conv_weight, pack_tattn_f16
    lib = _lib.get_lib()
    stream = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    wqkv, wo = torch.randn(384, 64, device=DEV) * 0.2, torch.randn(64, 128, device=DEV) * 0.1
    g = torch.rand(64, device=DEV) + 0.5
    ang = torch.arange(32, dtype=torch.float32)[:, None] * (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)))[None, :]
    rot = torch.stack((ang.cos(), ang.sin()), dim=-1).reshape(-1).to(DEV)
    bias = torch.randn(4 * 32 * 32, device=DEV) * 0.3
    wq4, wo4, wpk = pack_conv_weight(wqkv.view(384, 64, 1)), pack_conv_weight(wo.view(64, 128, 1)), pack_tattn_f16(wqkv, wo)
    for B in (64, 2):
        x = torch.randn(B, 64, 32, 64, 64, device=DEV) * 0.5
        y4, yh = torch.empty_like(x), torch.empty_like(x)
        tail = (B, 64 * 64, 64, 32, 64 * 32 * 64 * 64, 32 * 64 * 64, 64 * 64, 1e-5)
        a4 = (x.data_ptr(), g.data_ptr(), wq4.data_ptr(), wo4.data_ptr(), rot.data_ptr(), bias.data_ptr(), y4.data_ptr(), *tail)
        ah = (x.data_ptr(), g.data_ptr(), wpk.data_ptr(), rot.data_ptr(), bias.data_ptr(), yh.data_ptr(), *tail)
        m4, mh = [], []
        for _ in range(3):          # interleaved repeats of the median of 20: their spread is what a gain has to beat
            m4.append(_time_call(lib.sdc_tattn_block, a4, stream))
            mh.append(_time_call(lib.sdc_tattn_block_f16, ah, stream))
        br = (y4[:1] - x[:1]).double()
        err = ((yh[:1] - x[:1]).double() - br).pow(2).mean().sqrt().item() / br.pow(2).mean().sqrt().item()
        med4, medh = statistics.median(m4), statistics.median(mh)
        gb = 3.0 * x.numel() * 4 / 1e9
        print(f"[measured] tattn block B {B} 64 ch 32 frames 64x64: ta_block_kernel {' / '.join(f'{v * 1e3:.1f}' for v in m4)} us | "
              f"ta_block_f16_kernel {' / '.join(f'{v * 1e3:.1f}' for v in mh)} us ({gb / medh:.2f} TB/s of x read twice + y written) -> "
              f"x{med4 / medh:.2f} {'FASTER (every repeat beats every repeat)' if max(mh) < min(m4) else 'NOT faster by the rule'}; "
              f"rms difference of the attention branch on sample 0: {err:.2e}", flush=True)
        del x, y4, yh
        torch.cuda.empty_cache()


def linattn_shapes():
    """the fused LinearAttention block at the C4 and C2 sites and at B = 2: sdc_linattn_block / _gn against sdc_linattn_block_f16 / _gn_f16
    on the same buffers; the medians of 20 launches, three interleaved repeats; FASTER when every repeat beats every repeat"""
    from safediffcon_amd.engine import pack_conv_weight, pack_linattn_f16
    lib = _lib.get_lib()
    stream = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    # (outer, inner, C, n, GroupNorm-on-load, norm modes): smoke SpatialLinearAttention (LayerNorm in, none out), Burgers LayerNorm in and out
    sites = [(64, 32, 64, 4096, True, 0, -1), (64, 32, 64, 4096, False, 0, -1), (64, 32, 128, 1024, True, 0, -1),
             (256, 1, 64, 2048, False, 0, 0), (256, 1, 128, 512, False, 0, 0),
             (2, 32, 64, 4096, True, 0, -1), (2, 32, 128, 1024, True, 0, -1), (2, 1, 64, 2048, False, 0, 0), (2, 1, 128, 512, False, 0, 0)]
    for outer, inner, Cc, n, gn, pre, post in sites:
        wqkv, wo = torch.randn(384, Cc, device=DEV) * 0.2, torch.randn(Cc, 128, device=DEV) * 0.1
        g1, g2, bo = torch.rand(Cc, device=DEV) + 0.5, torch.rand(Cc, device=DEV) + 0.5, torch.randn(Cc, device=DEV) * 0.1
        wq4, wo4, wpk = pack_conv_weight(wqkv.view(384, Cc, 1)), pack_conv_weight(wo.view(Cc, 128, 1)), pack_linattn_f16(wqkv, wo).to(DEV)
        x = torch.randn(outer, Cc, inner, n, device=DEV) * 0.5
        y4, yh = torch.empty_like(x), torch.empty_like(x)
        w4 = torch.empty(int(lib.sdc_linattn_block_bytes(outer, inner, Cc, n)) // 4, device=DEV)
        wh = torch.empty((int(lib.sdc_linattn_block_f16_bytes(outer, inner, Cc, n)) + 3) // 4, device=DEV)
        tail = (outer, inner, Cc, n, Cc * inner * n, inner * n, n, pre, post, 1e-5)
        gp = g2.data_ptr() if post >= 0 else None
        head = (x.data_ptr(),)
        if gn:
            st = torch.stack((torch.randn(outer * 8, device=DEV) * 0.1, torch.rand(outer * 8, device=DEV) + 0.5), -1).reshape(-1).contiguous()
            gam, bet, res = torch.rand(Cc, device=DEV) + 0.5, torch.randn(Cc, device=DEV) * 0.1, torch.randn_like(x) * 0.5
            head = (x.data_ptr(), st.data_ptr(), gam.data_ptr(), bet.data_ptr(), 8, res.data_ptr())
        a4 = (*head, g1.data_ptr(), wq4.data_ptr(), wo4.data_ptr(), bo.data_ptr(), gp, w4.data_ptr(), y4.data_ptr(), *tail)
        ah = (*head, g1.data_ptr(), wq4.data_ptr(), wo4.data_ptr(), wpk.data_ptr(), bo.data_ptr(), gp, wh.data_ptr(), yh.data_ptr(), *tail)
        f4, fh = ((lib.sdc_linattn_block_gn, lib.sdc_linattn_block_gn_f16) if gn else (lib.sdc_linattn_block, lib.sdc_linattn_block_f16))
        m4, mh = [], []
        for _ in range(3):          # interleaved repeats of the median of 20: their spread is what a gain has to beat
            m4.append(_time_call(f4, a4, stream))
            mh.append(_time_call(fh, ah, stream))
        # the branch y - h on sequence block 0 (the plain form: h = x)
        br = y4[:1].double()
        err = (yh[:1].double() - br).pow(2).mean().sqrt().item() / (br - (0 if gn else x[:1].double())).pow(2).mean().sqrt().item()
        med4, medh = statistics.median(m4), statistics.median(mh)
        # tensor passes over HBM: x read by pass 1 and by pass 2, y written; GroupNorm-on-load: raw x and the residual read, h written,
        # h read back, y written
        gb = (5.0 if gn else 3.0) * x.numel() * 4 / 1e9
        print(f"[measured] linattn block {'gn ' if gn else ''}outer {outer} inner {inner} C {Cc} n {n}: la_blk {' / '.join(f'{v * 1e3:.1f}' for v in m4)} us"
              f" | la16 {' / '.join(f'{v * 1e3:.1f}' for v in mh)} us ({gb / medh:.2f} TB/s of its HBM traffic) -> x{med4 / medh:.2f} "
              f"{'FASTER (every repeat beats every repeat)' if max(mh) < min(m4) else 'NOT faster by the rule'}; "
              f"rms difference on sample 0 of y{'' if gn else ', of the attention branch'}: {err:.2e}", flush=True)
        del x, y4, yh, w4, wh
        torch.cuda.empty_cache()


def linattn_split_shapes():
    """the fused LinearAttention block with its q / k projections as bf16 splits (csrc/sdc_lablock_x3.hip): sdc_linattn_block_sel /
    sdc_linattn_block_gn_sel with impl 0 against impl 1 on the same buffers, at the sites of linattn_shapes(); the medians of 20 launches,
    three interleaved repeats; a size QUALIFIES for sdc_linattn_block_x3_ok when every repeat of impl 1 beats every repeat of impl 0"""
    from safediffcon_amd.engine import pack_conv_weight
    lib = _lib.get_lib()
    stream = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    # (the C4 up path has a width-64 block at 32 x 32 and a width-128 block at 16 x 16 besides the sites of linattn_shapes())
    sites = [(64, 32, 64, 4096, True, 0, -1), (64, 32, 64, 4096, False, 0, -1), (64, 32, 128, 1024, True, 0, -1),
             (64, 32, 64, 1024, True, 0, -1), (64, 32, 128, 256, True, 0, -1),
             (256, 1, 64, 2048, False, 0, 0), (256, 1, 128, 512, False, 0, 0),
             (2, 32, 64, 4096, True, 0, -1), (2, 32, 128, 1024, True, 0, -1), (2, 32, 64, 1024, True, 0, -1), (2, 32, 128, 256, True, 0, -1),
             (2, 1, 64, 2048, False, 0, 0), (2, 1, 128, 512, False, 0, 0)]
    for outer, inner, Cc, n, gn, pre, post in sites:
        wqkv, wo = torch.randn(384, Cc, device=DEV) * 0.2, torch.randn(Cc, 128, device=DEV) * 0.1
        g1, g2, bo = torch.rand(Cc, device=DEV) + 0.5, torch.rand(Cc, device=DEV) + 0.5, torch.randn(Cc, device=DEV) * 0.1
        wq4, wo4 = pack_conv_weight(wqkv.view(384, Cc, 1)), pack_conv_weight(wo.view(Cc, 128, 1))
        x = torch.randn(outer, Cc, inner, n, device=DEV) * 0.5
        y0, y1 = torch.empty_like(x), torch.empty_like(x)
        work = torch.empty(int(lib.sdc_linattn_block_bytes(outer, inner, Cc, n)) // 4, device=DEV)
        gp = g2.data_ptr() if post >= 0 else None
        head = (x.data_ptr(),)
        if gn:
            st = torch.stack((torch.randn(outer * 8, device=DEV) * 0.1, torch.rand(outer * 8, device=DEV) + 0.5), -1).reshape(-1).contiguous()
            gam, bet, res = torch.rand(Cc, device=DEV) + 0.5, torch.randn(Cc, device=DEV) * 0.1, torch.randn_like(x) * 0.5
            head = (x.data_ptr(), st.data_ptr(), gam.data_ptr(), bet.data_ptr(), 8, res.data_ptr())
        tail = (outer, inner, Cc, n, Cc * inner * n, inner * n, n, pre, post, 1e-5)
        f = lib.sdc_linattn_block_gn_sel if gn else lib.sdc_linattn_block_sel
        a0 = (*head, g1.data_ptr(), wq4.data_ptr(), wo4.data_ptr(), bo.data_ptr(), gp, work.data_ptr(), y0.data_ptr(), *tail, 0)
        a1 = (*head, g1.data_ptr(), wq4.data_ptr(), wo4.data_ptr(), bo.data_ptr(), gp, work.data_ptr(), y1.data_ptr(), *tail, 1)
        m0, m1 = [], []
        for _ in range(3):          # interleaved repeats of the median of 20: their spread is what a gain has to beat
            m0.append(_time_call(f, a0, stream))
            m1.append(_time_call(f, a1, stream))
        # the branch y - h on sequence block 0 (the plain form: h = x)
        br = y0[:1].double()
        err = (y1[:1].double() - br).pow(2).mean().sqrt().item() / (br - (0 if gn else x[:1].double())).pow(2).mean().sqrt().item()
        med0, med1 = statistics.median(m0), statistics.median(m1)
        listed = bool(lib.sdc_linattn_block_x3_ok(Cc, n))
        print(f"[measured] linattn block {'gn ' if gn else ''}outer {outer} inner {inner} C {Cc} n {n} ({'listed' if listed else 'not listed'}): "
              f"impl 0 (fp32) {' / '.join(f'{v * 1e3:.1f}' for v in m0)} us | impl 1 (bf16-split q / k) {' / '.join(f'{v * 1e3:.1f}' for v in m1)} us"
              f" -> x{med0 / med1:.2f} {'QUALIFIES (every repeat beats every repeat)' if max(m1) < min(m0) else 'does NOT qualify'}; "
              f"rms difference on sample 0 of y{'' if gn else ', of the attention branch'}: {err:.2e}", flush=True)
        del x, y0, y1, work
        torch.cuda.empty_cache()


def attn_split_shapes():
    """net.attn_split: sdc_tattn_block against sdc_tattn_block_x3 on the same buffers at the sites of the dim-64 smoke net -- 64 x 64 (the
    C4 site, B = 64 and B = 2), 32 x 32 and 16 x 16 (B = 64); the medians of 20 launches, three interleaved repeats; a shape QUALIFIES
    for the routing table when every repeat of the split kernel beats every repeat of the fp32 kernel"""
    from safediffcon_amd.engine import pack_conv_weight, pack_tattn_x3
    lib = _lib.get_lib()
    stream = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    wqkv, wo = torch.randn(384, 64, device=DEV) * 0.2, torch.randn(64, 128, device=DEV) * 0.1
    g = torch.rand(64, device=DEV) + 0.5
    ang = torch.arange(32, dtype=torch.float32)[:, None] * (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)))[None, :]
    rot = torch.stack((ang.cos(), ang.sin()), dim=-1).reshape(-1).to(DEV)
    bias = torch.randn(4 * 32 * 32, device=DEV) * 0.3
    wq4, wo4, wpk = pack_conv_weight(wqkv.view(384, 64, 1)), pack_conv_weight(wo.view(64, 128, 1)), pack_tattn_x3(wqkv, wo)
    for B, hw in ((64, 64), (2, 64), (64, 32), (64, 16)):
        x = torch.randn(B, 64, 32, hw, hw, device=DEV) * 0.5
        y4, ys = torch.empty_like(x), torch.empty_like(x)
        tail = (B, hw * hw, 64, 32, 64 * 32 * hw * hw, 32 * hw * hw, hw * hw, 1e-5)
        a4 = (x.data_ptr(), g.data_ptr(), wq4.data_ptr(), wo4.data_ptr(), rot.data_ptr(), bias.data_ptr(), y4.data_ptr(), *tail)
        as_ = (x.data_ptr(), g.data_ptr(), wpk.data_ptr(), rot.data_ptr(), bias.data_ptr(), ys.data_ptr(), *tail)
        m4, ms = [], []
        for _ in range(3):          # interleaved repeats of the median of 20: their spread is what a gain has to beat
            m4.append(_time_call(lib.sdc_tattn_block, a4, stream))
            ms.append(_time_call(lib.sdc_tattn_block_x3, as_, stream))
        br = (y4[:1] - x[:1]).double()
        err = ((ys[:1] - x[:1]).double() - br).pow(2).mean().sqrt().item() / br.pow(2).mean().sqrt().item()
        med4, meds = statistics.median(m4), statistics.median(ms)
        routed = bool(lib.sdc_tattn_block_x3_ok(64, 32, hw * hw))
        print(f"[measured] tattn block B {B} 64 ch 32 frames {hw}x{hw} (inner {hw * hw}, {'routed' if routed else 'not routed'}): "
              f"ta_block_kernel {' / '.join(f'{v * 1e3:.1f}' for v in m4)} us | ta_block_x3_kernel "
              f"{' / '.join(f'{v * 1e3:.1f}' for v in ms)} us -> x{med4 / meds:.2f} "
              f"{'QUALIFIES (every repeat beats every repeat)' if max(ms) < min(m4) else 'does NOT qualify'}; "
              f"rms difference of the attention branch on sample 0: {err:.2e}", flush=True)
        del x, y4, ys
        torch.cuda.empty_cache()


def attn_skew_shapes():
    """the skewed form of the bf16-split temporal-attention block (ta_block_x3s_kernel): sdc_tattn_block_x3_sel with impl 0 against impl
    1 on the same buffers at 64 x 64 (the C4 site, B = 64 and B = 2) and 32 x 32 (B = 64); the medians of 20 launches, three
    interleaved repeats; a size QUALIFIES for sdc_tattn_block_x3_impl when every repeat of impl 1 beats every repeat of impl 0 at the
    bench batch"""
    from safediffcon_amd.engine import pack_tattn_x3
    lib = _lib.get_lib()
    stream = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    wqkv, wo = torch.randn(384, 64, device=DEV) * 0.2, torch.randn(64, 128, device=DEV) * 0.1
    g = torch.rand(64, device=DEV) + 0.5
    ang = torch.arange(32, dtype=torch.float32)[:, None] * (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)))[None, :]
    rot = torch.stack((ang.cos(), ang.sin()), dim=-1).reshape(-1).to(DEV)
    bias = torch.randn(4 * 32 * 32, device=DEV) * 0.3
    wpk = pack_tattn_x3(wqkv, wo)
    for B, hw in ((64, 64), (2, 64), (64, 32)):
        x = torch.randn(B, 64, 32, hw, hw, device=DEV) * 0.5
        y0, y1 = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        tail = (B, hw * hw, 64, 32, 64 * 32 * hw * hw, 32 * hw * hw, hw * hw, 1e-5)
        a0 = (x.data_ptr(), g.data_ptr(), wpk.data_ptr(), rot.data_ptr(), bias.data_ptr(), y0.data_ptr(), *tail, 0)
        a1 = (x.data_ptr(), g.data_ptr(), wpk.data_ptr(), rot.data_ptr(), bias.data_ptr(), y1.data_ptr(), *tail, 1)
        m0, m1 = [], []
        for _ in range(3):          # interleaved repeats of the median of 20: their spread is what a gain has to beat
            m0.append(_time_call(lib.sdc_tattn_block_x3_sel, a0, stream))
            m1.append(_time_call(lib.sdc_tattn_block_x3_sel, a1, stream))
        med0, med1 = statistics.median(m0), statistics.median(m1)
        listed = bool(lib.sdc_tattn_block_x3_impl(64, 32, hw * hw))
        print(f"[measured] tattn x3 block B {B} 64 ch 32 frames {hw}x{hw} (inner {hw * hw}, {'listed' if listed else 'not listed'}): "
              f"impl 0 (ta_block_x3_kernel) {' / '.join(f'{v * 1e3:.1f}' for v in m0)} us | impl 1 (ta_block_x3s_kernel) "
              f"{' / '.join(f'{v * 1e3:.1f}' for v in m1)} us -> x{med0 / med1:.3f} "
              f"{'QUALIFIES (every repeat beats every repeat)' if max(m1) < min(m0) else 'does NOT qualify'}; "
              f"bit-identical: {bool(torch.equal(y0, y1))}", flush=True)
        del x, y0, y1
        torch.cuda.empty_cache()


def attn_phase():
    """one line of the phase account of ta_block_x3_kernel: the C4 site at B = 64, the median of 20 launches of impl
    0, under an experiments build (python -m safediffcon_amd.build --experiments, SDC_LIB_PATH) with SDC_TAX3_DBG naming the part that
    is switched off (1 LayerNorm, 2 y exit, 4 splits, 8 weight fetch and park, 16 fragment reads, 32 per-head barrier, 64 rotary and
    softmax, 127 MFMAs only; 0 the whole kernel).  One process per value: the library reads the variable once.  WRONG RESULTS."""
    from safediffcon_amd.engine import pack_tattn_x3
    lib = _lib.get_lib()
    stream = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    wpk = pack_tattn_x3(torch.randn(384, 64, device=DEV) * 0.2, torch.randn(64, 128, device=DEV) * 0.1)
    g = torch.rand(64, device=DEV) + 0.5
    rot, bias = torch.rand(32 * 16 * 2, device=DEV), torch.randn(4 * 32 * 32, device=DEV) * 0.3
    B, hw = 64, 64
    x = torch.randn(B, 64, 32, hw, hw, device=DEV) * 0.5
    y = torch.empty_like(x)
    args = (x.data_ptr(), g.data_ptr(), wpk.data_ptr(), rot.data_ptr(), bias.data_ptr(), y.data_ptr(), B, hw * hw, 64, 32,
            64 * 32 * hw * hw, 32 * hw * hw, hw * hw, 1e-5, 0)
    ms = [_time_call(lib.sdc_tattn_block_x3_sel, args, stream) for _ in range(2)]
    print(f"[measured] ta_block_x3_kernel B 64 64x64 SDC_TAX3_DBG={os.environ.get('SDC_TAX3_DBG', '0')} library "
          f"{os.path.basename(os.environ.get('SDC_LIB_PATH', 'libsdc_hip.so'))}: {' / '.join(f'{v * 1e3:.1f}' for v in ms)} us", flush=True)


def drift(T, stem=False, attn=False, linattn=False):
    torch.manual_seed(0)
    net = sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7).to(DEV)
    init = (torch.rand(2, 64, 64) * 0.2).to(DEV)
    control = (torch.randn(2, 32, 2, 64, 64) * 0.3).to(DEV)
    outs = {}
    arms = (4, "4+la") if linattn else (4, "4+attn") if attn else (4, "4+stem", "6+stem") if stem else (4, 6, 7)
    for prec in arms:
        net.precision = int(prec.split("+")[0]) if isinstance(prec, str) else prec
        net.stem_f16 = "+stem" in str(prec)
        net.attn_f16 = "+attn" in str(prec)
        net.linattn_f16 = "+la" in str(prec)
        gs = sdc.GaussianDiffusionSmoke(net, image_size=64, frames=32, timesteps=T, standard_fixed_ratio=100.0).to(DEV)
        torch.manual_seed(7)
        t0 = time.perf_counter()
        outs[prec] = gs.sample(batch_size=2, design_fn=sdc.SmokeGuidance(0.01, 0.9, 0.1), init=init, control=control).cpu()
        print(f"precision {prec}: {time.perf_counter() - t0:.1f} s, finite {bool(torch.isfinite(outs[prec]).all())}, "
              f"|x|max {outs[prec].abs().max():.3f}", flush=True)
    for p in arms[1:]:
        d = (outs[p] - outs[4]).abs()
        print(f"[measured] {T}-step guided smoke trajectories, precision {p} vs 4: max|diff| {d.max():.3e}  mean|diff| {d.mean():.3e}  "
              f"MSE {(d ** 2).mean():.3e}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c4,c2,c3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--arm", type=int, default=6, choices=(6, 7), help="the precision timed against 4")
    ap.add_argument("--shapes", action="store_true")
    ap.add_argument("--drift", type=int, nargs="?", const=1000, default=None)
    ap.add_argument("--stem", action="store_true", help="net.stem_f16: the stem launch and the C4 step (with --drift: the stem arms)")
    ap.add_argument("--split", action="store_true", help="net.stem_split: the stem launch and the C4 step with the switch off / on")
    ap.add_argument("--gemm", action="store_true", help="net.gemm_split: the covered convs, launch by launch, and the C4 step with the switch off / on")
    ap.add_argument("--pw-split", action="store_true", help="conv_pw_x3_kernel: the covered 1x1 convs, launch by launch, against the fp32 kernel; then the C4 and C2 steps of this build (the A/B is by commit: SDC_LIB_PATH)")
    ap.add_argument("--wino", action="store_true", help="net.wino_split: the covered 3x3x3 convs, launch by launch, and the C4 step with the switch off / on")
    ap.add_argument("--attn", action="store_true", help="net.attn_f16: the block launch and the C4 step (with --drift: 4 + attn_f16 against 4)")
    ap.add_argument("--linattn", action="store_true", help="net.linattn_f16: the block launch at the C4 / C2 sites, the C4 and C2 steps (with --drift: 4 + linattn_f16 against 4)")
    ap.add_argument("--linattn-split", action="store_true", help="the fused LinearAttention block, impl 0 (fp32) against impl 1 (bf16-split q / k projections) launch by launch; then the C4 and C2 steps of this build (the A/B is by commit: SDC_LIB_PATH)")
    ap.add_argument("--attn-split", action="store_true", help="net.attn_split: the block launch at the sites of the dim-64 smoke net and the C4 step with the switch off / on")
    ap.add_argument("--attn-skew", action="store_true", help="the bf16-split temporal-attention block, impl 0 against impl 1 (waves 4 - 7 half a head behind) launch by launch; then the C4 step of this build (the A/B is by commit: SDC_LIB_PATH)")
    ap.add_argument("--attn-phase", action="store_true", help="one line of ta_block_x3_kernel's phase account: the C4 site under an experiments build with SDC_TAX3_DBG set")
    ap.add_argument("--no-step", action="store_true", help="--stem / --split / --gemm / --pw-split / --wino / --attn / --attn-split: the per-shape part only")
    a = ap.parse_args()
    wls = [w for w in a.workloads.split(",") if w]
    if a.drift:
        drift(a.drift, a.stem, a.attn, a.linattn)
    elif a.linattn_split:
        linattn_split_shapes()
        if not a.no_step:
            # the entry points carry no switch: the step's A/B is by commit (bench.py of the two checkouts, or SDC_LIB_PATH naming the
            # parent's library for a second run of this command)
            step_ab([w for w in wls if w in ("c4", "c2")], a.steps, a.warmup, a.rounds, arms=[4])
    elif a.pw_split:
        pw_shapes(wls)
        if not a.no_step:
            step_ab([w for w in wls if w in ("c4", "c2")], a.steps, a.warmup, a.rounds, arms=[4])
    elif a.linattn:
        linattn_shapes()
        if not a.no_step:
            if "c4" in wls:
                step_ab(["c4"], a.steps, a.warmup, a.rounds, arms=[4, "4+la", "6+stem+attn", "6+stem+attn+la"])
            if "c2" in wls:
                step_ab(["c2"], a.steps, a.warmup, a.rounds, arms=[4, "4+la"])
    elif a.attn_phase:
        attn_phase()
    elif a.attn_skew:
        attn_skew_shapes()
        if not a.no_step:
            # the entry point carries no switch: the step's A/B is by commit (bench.py of the two checkouts, or SDC_LIB_PATH)
            step_ab(["c4"], a.steps, a.warmup, a.rounds, arms=[4])
    elif a.attn_split:
        attn_split_shapes()
        if not a.no_step:
            step_ab(["c4"], a.steps, a.warmup, a.rounds, arms=["4-noasplit", "4+asplit"])
    elif a.attn:
        attn_shapes()
        if not a.no_step:
            step_ab(["c4"], a.steps, a.warmup, a.rounds, arms=[4, "4+attn", "6+stem", "6+stem+attn"])
    elif a.wino:
        wino_shapes()
        if not a.no_step:
            step_ab(["c4"], a.steps, a.warmup, a.rounds, arms=["4-nowino", "4+wino"])
    elif a.gemm:
        gemm_shapes(wls)
        if not a.no_step:
            step_ab(["c4"], a.steps, a.warmup, a.rounds, arms=["4-nogemm", 4])
    elif a.split:
        stem_shapes([w for w in wls if w != "c3"], split=True)
        if not a.no_step:
            step_ab(["c4"], a.steps, a.warmup, a.rounds, arms=["4-nosplit", 4])
    elif a.stem:
        stem_shapes([w for w in wls if w != "c3"])
        if not a.no_step:
            step_ab(["c4"], a.steps, a.warmup, a.rounds, arms=[4, "4+stem", 6, "6+stem"])
    elif a.shapes:
        shapes(wls)
    else:
        step_ab(wls, a.steps, a.warmup, a.rounds, a.arm)
