"""-m gpu: the backward (VJP) kernels of the fine-tuning path on the launch branches that production sizes take and the small
shapes of tests/test_gpu_grad.py never reach, against torch autograd in fp64 of the plain formula (same helpers, same gates):
  * sdc_attn_bwd past its cap of 1024 workgroup slots (a workgroup walks its group loop twice): both kernels, all three launch
    branches, with run-to-run and sequence-alone bit identity;
  * the softmax / linear attention cores, forward and backward, at peaked (near one-hot) attention: qkv scaled by 2 and 4;
  * sdc_chan_norm_bwd through the C ABI with a NaN-filled workspace: fewer batch slabs than samples (uneven split, the kernel's
    own zero-fill of the columns of the slabs that do not exist, a second call into the dirty workspace), ragged tiles, the
    forward's edge shapes;
  * sdc_gn_silu_bwd past the apply pass's 64-piece cap and the flat apply kernel's 8192-block cap, and its scalar fallback for
    operands that are not 16-byte aligned; sdc_act_bwd and sdc_sumpool2 past their 8192-block grids.
Every shape is the smallest that reaches its path; the arithmetic stands next to it."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from oracle.detweights import det_tensor
from safediffcon_amd import _lib, grad_ops
from test_gpu_grad import DEV, _ref_attention, _rel, _rot_table

pytestmark = pytest.mark.gpu


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


# ------------------------------------------------------------------ references of the attention cores, in fp64 or fp32
def _temporal_ref(qkv, bias, gout, heads, dtype):
    """'b c f h w -> b (h w) f c' attention with rotary + relative-position bias on (B, 3 heads 32, F, H, W): (out, dqkv, dbias)"""
    B, _, Fr, H, W = qkv.shape
    hw = H * W
    _, ang = _rot_table(Fr)
    qd, bd = qkv.to(dtype).requires_grad_(), bias.to(dtype).requires_grad_()
    q, k, v = (t.reshape(B, heads, 32, Fr, hw).permute(0, 4, 1, 3, 2) for t in qd.chunk(3, dim=1))       # (B, hw, heads, F, 32)
    o = _ref_attention(q, k, v, ang.to(dtype), bd)
    out = o.permute(0, 2, 4, 3, 1).reshape(B, heads * 32, Fr, H, W)
    out.backward(gout.to(dtype))
    return out.detach(), qd.grad, bd.grad


def _full_ref(qkv, gout, heads, dtype):
    """token-contiguous softmax attention on (B, 3 heads 32, inner, n): (out, dqkv)"""
    B, _, inner, n = qkv.shape
    qd = qkv.to(dtype).requires_grad_()
    q, k, v = (t.reshape(B, heads, 32, inner, n).permute(0, 3, 1, 4, 2) for t in qd.chunk(3, dim=1))     # (B, inner, heads, n, 32)
    out = _ref_attention(q, k, v).permute(0, 2, 4, 1, 3).reshape(B, heads * 32, inner, n)
    out.backward(gout.to(dtype))
    return out.detach(), qd.grad


def _linattn_ref(qkv, gout, heads, dtype):
    """LinearAttention core on (B, 3 heads 32, inner, n): softmax over d of q, over n of k, context, output: (out, dqkv)"""
    B, _, inner, n = qkv.shape
    qd = qkv.to(dtype).requires_grad_()
    q, k, v = (t.reshape(B, heads, 32, inner, n).permute(0, 3, 1, 2, 4) for t in qd.chunk(3, dim=1))     # (B, inner, heads, 32, n)
    qq = q.softmax(dim=-2) * 32 ** -0.5
    kk = k.softmax(dim=-1)
    ctx = torch.einsum("...dn,...en->...de", kk, v)
    out = torch.einsum("...de,...dn->...en", ctx, qq).permute(0, 2, 3, 1, 4).reshape(B, heads * 32, inner, n)
    out.backward(gout.to(dtype))
    return out.detach(), qd.grad


def _strides(ch, inner, ntok, tok_contig):
    """(so, sc, si, st) of a contiguous (outer, ch, ntok, inner) (frame-strided) or (outer, ch, inner, ntok) tensor"""
    return (ch * inner * ntok, inner * ntok, ntok, 1) if tok_contig else (ch * inner * ntok, inner * ntok, 1, inner)


def _run_attn(qkv, gout, heads, outer, inner, ntok, tok_contig, rot, bias):
    """sdc_attn + sdc_attn_bwd on device tensors -> (out, dqkv, dbias | None)"""
    qs, os_ = _strides(3 * heads * 32, inner, ntok, tok_contig), _strides(heads * 32, inner, ntok, tok_contig)
    out = torch.empty_like(gout)
    grad_ops.attn_core(qkv, out, heads, outer, inner, ntok, qs, os_, rot, bias)
    dqkv, dbias = grad_ops.attn_core_bwd(qkv, gout, heads, outer, inner, ntok, qs, os_, rot, bias)
    return out, dqkv, dbias


# ------------------------------------------------------------------ 1. sdc_attn_bwd past the slot cap
# The host caps the grid at `cap` slots per head and every workgroup walks `for (grp = slot; grp < ngrp; grp += nslots)`:
# with ngrp > cap the workgroups of slots 0 .. ngrp - cap - 1 run the loop body twice -- LDS staged again over the first
# group's images, the bias-gradient accumulator carried on -- and sum_rows_kernel adds `cap` partial tables.  heads = 1 keeps
# the tensors small.  nseq = sequences per group (what the host resolves for the shape), ngrp = outer * inner / nseq.
SLOT_CAP_CASES = [
    # MFMA kernel (frame-strided, 32 frames, inner % 8 == 0): groups of 8 pixels, 96 * 96 = 9216 pixels -> 1152 groups:
    # slots 0 .. 127 run two groups, the rest one
    pytest.param(dict(outer=1, inner=96 * 96, ntok=32, tok_contig=False, rot_bias=True, nseq=8, sp=(96, 96)), id="mfma"),
    # generic kernel, frame-strided: 256 / 8 = 32 sequences per group, 4 with the bias gradient (room for its LDS table);
    # 2 * 48 * 48 = 4608 sequences -> 1152 groups
    pytest.param(dict(outer=2, inner=48 * 48, ntok=8, tok_contig=False, rot_bias=True, nseq=4, sp=(48, 48)), id="generic-strided"),
    # generic kernel, token-contiguous: 256 / 200 = 1 sequence per group, 1030 sequences -> 1030 groups: slots 0 .. 5 run two
    pytest.param(dict(outer=1, inner=1030, ntok=200, tok_contig=True, rot_bias=False, nseq=1, sp=None), id="generic-contig"),
]


@pytest.mark.parametrize("case", SLOT_CAP_CASES)
def test_attention_backward_past_the_slot_cap(case):
    outer, inner, ntok, tc, nseq = case["outer"], case["inner"], case["ntok"], case["tok_contig"], case["nseq"]
    heads = 1
    lib = _lib.get_lib()
    cap = int(lib.sdc_attn_bwd_bytes(outer, inner, heads, ntok)) // (4 * heads * ntok * ntok)
    ngrp = outer * inner // nseq
    assert inner % nseq == 0 and ngrp > cap, (ngrp, cap)          # some workgroup runs its group loop twice
    if tc:
        qkv, gout = det_tensor((outer, 96, inner, ntok), 150), det_tensor((outer, 32, inner, ntok), 151)
        rot = bias = None
        out_ref, dq_ref = _full_ref(qkv, gout, heads, torch.float64)
        db_ref = None
    else:
        qkv, gout = det_tensor((outer, 96, ntok, *case["sp"]), 140), det_tensor((outer, 32, ntok, *case["sp"]), 142)
        bias = 0.5 * det_tensor((heads, ntok, ntok), 141)
        rot = _rot_table(ntok)[0]
        out_ref, dq_ref, db_ref = _temporal_ref(qkv, bias, gout, heads, torch.float64)
        rot, bias = rot.to(DEV), bias.to(DEV)
    qg, gg = qkv.to(DEV), gout.to(DEV)
    out, dqkv, dbias = _run_attn(qg, gg, heads, outer, inner, ntok, tc, rot, bias)
    errs = dict(out=_rel(out, out_ref), dqkv=_rel(dqkv, dq_ref))
    if db_ref is not None:
        errs["dbias"] = _rel(dbias, db_ref)
    print(f"[measured] attention backward past the slot cap {case}: ngrp {ngrp} cap {cap} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["out"] < 1e-5
    assert errs["dqkv"] < 2e-5 and errs.get("dbias", 0.0) < 2e-5
    # the partial tables are summed in a fixed order, every other element has one owner: two runs give the same bits
    _, dqkv2, dbias2 = _run_attn(qg, gg, heads, outer, inner, ntok, tc, rot, bias)
    assert torch.equal(dqkv, dqkv2)
    assert dbias is None or torch.equal(dbias, dbias2)
    # sequences are independent: the groups cap .. ngrp - 1, every one of them some workgroup's SECOND iteration, copied out
    # and run alone (the same groups of nseq sequences, one iteration each, the same kernel and LDS layout) give the same bits
    nsec = (ngrp - cap) * nseq
    o, i0 = (cap * nseq) // inner, (cap * nseq) % inner
    assert i0 + nsec == inner and o == outer - 1                   # the tail of the last `outer` block
    if tc:
        cut = lambda t: t[o:o + 1, :, i0:, :].contiguous()
    else:
        cut = lambda t: t.reshape(outer, t.shape[1], ntok, inner)[o:o + 1, :, :, i0:].contiguous()
    _, dq_alone, _ = _run_attn(cut(qg), cut(gg), heads, 1, nsec, ntok, tc, rot, bias)
    assert torch.equal(dq_alone, cut(dqkv))


# ------------------------------------------------------------------ 2. peaked softmax through the cores
# det_tensor inputs at scale 1 give logits of O(1) and nearly uniform softmaxes.  qkv scaled by 4 gives logits with a standard
# deviation around 16: near one-hot rows, where the row-maximum subtraction, softmax_exp = __expf, the cancellation in
# P (dP - D) and the row statistics shared between the two orientations of the backward carry the result.  The gate is the
# file's, unless the same torch formula evaluated in fp32 on the same inputs is itself further than a quarter of it from fp64
# (e_fp32): then 4 e_fp32, the factor 4 for another summation order and for __expf.
def _gate(file_gate, e_fp32):
    return max(file_gate, 4.0 * e_fp32)


def _finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts if t is not None)


@pytest.mark.parametrize("scale", [2.0, 4.0])
@pytest.mark.parametrize("Fr,H,W,B", [(32, 4, 8, 2), (32, 3, 5, 2)])           # the MFMA kernels, the generic ones (15 pixels)
def test_temporal_attention_core_peaked(Fr, H, W, B, scale):
    hw = H * W
    qkv = det_tensor((B, 384, Fr, H, W), 140, scale)
    bias = 0.5 * det_tensor((4, Fr, Fr), 141)
    gout = det_tensor((B, 128, Fr, H, W), 142)
    ref = _temporal_ref(qkv, bias, gout, 4, torch.float64)
    e32 = [_rel(a, b) for a, b in zip(_temporal_ref(qkv, bias, gout, 4, torch.float32), ref)]
    got = _run_attn(qkv.to(DEV), gout.to(DEV), 4, B, hw, Fr, False, _rot_table(Fr)[0].to(DEV), bias.to(DEV))
    err = [_rel(a, b) for a, b in zip(got, ref)]
    print(f"[measured] temporal attention core, qkv x {scale:g}, F={Fr} {H}x{W} B={B}: kernel out {err[0]:.2e} dqkv {err[1]:.2e} "
          f"dbias {err[2]:.2e} | fp32 torch out {e32[0]:.2e} dqkv {e32[1]:.2e} dbias {e32[2]:.2e}")
    assert _finite(*got)
    assert err[0] < _gate(1e-5, e32[0])
    assert err[1] < _gate(2e-5, e32[1]) and err[2] < _gate(2e-5, e32[2])


@pytest.mark.parametrize("scale", [2.0, 4.0])
def test_full_attention_core_peaked(scale):
    B, inner, n = 2, 4, 256
    qkv = det_tensor((B, 384, inner, n), 150, scale)
    gout = det_tensor((B, 128, inner, n), 151)
    ref = _full_ref(qkv, gout, 4, torch.float64)
    e32 = [_rel(a, b) for a, b in zip(_full_ref(qkv, gout, 4, torch.float32), ref)]
    got = _run_attn(qkv.to(DEV), gout.to(DEV), 4, B, inner, n, True, None, None)[:2]
    err = [_rel(a, b) for a, b in zip(got, ref)]
    print(f"[measured] softmax attention core, qkv x {scale:g}, B={B} inner={inner} n={n}: kernel out {err[0]:.2e} dqkv {err[1]:.2e} "
          f"| fp32 torch out {e32[0]:.2e} dqkv {e32[1]:.2e}")
    assert _finite(*got)
    assert err[0] < _gate(1e-5, e32[0]) and err[1] < _gate(2e-5, e32[1])


@pytest.mark.parametrize("scale", [2.0, 4.0])
@pytest.mark.parametrize("B,inner,n", [(2, 1, 2048), (2, 1, 77)])
def test_linear_attention_core_peaked(B, inner, n, scale):
    qkv = det_tensor((B, 384, inner, n), 160, scale)
    gout = det_tensor((B, 128, inner, n), 161)
    ref = _linattn_ref(qkv, gout, 4, torch.float64)
    e32 = [_rel(a, b) for a, b in zip(_linattn_ref(qkv, gout, 4, torch.float32), ref)]
    qs, os_ = (384 * inner * n, inner * n, n), (128 * inner * n, inner * n, n)
    qg, gg = qkv.to(DEV), gout.to(DEV)
    out = grad_ops.linattn_core(qg, torch.empty_like(gg), 4, B, inner, n, qs, os_)
    dqkv = grad_ops.linattn_core_bwd(qg, gg, 4, B, inner, n, qs, os_)
    err = [_rel(out, ref[0]), _rel(dqkv, ref[1])]
    print(f"[measured] linear attention core, qkv x {scale:g}, B={B} inner={inner} n={n}: kernel out {err[0]:.2e} dqkv {err[1]:.2e} "
          f"| fp32 torch out {e32[0]:.2e} dqkv {e32[1]:.2e}")
    assert _finite(out, dqkv)
    assert err[0] < _gate(1e-5, e32[0]) and err[1] < _gate(2e-5, e32[1])


# ------------------------------------------------------------------ 3. sdc_chan_norm_bwd: slabs, ragged tiles, the forward's shapes
# The gain-gradient kernel runs ns = min(B, smallest power of two with C ns >= 1024) batch slabs per channel, slab s summing
# the samples B s / ns .. B (s + 1) / ns - 1 into column s of the [C][B] partial table; slab 0's workgroup zero-fills the
# columns ns .. B - 1 (the caller sums all B).  (B, C, S, ns):
CHAN_NORM_SHAPES = [
    (8, 256, 40, 4),        # 256 * 4 = 1024: 4 even slabs of 2 samples, 4 zero-filled columns
    (5, 300, 19, 4),        # 300 * 4 >= 1024: slabs of 1, 1, 1, 2 samples, 1 zero-filled column; C and S off every tile size
    (2, 2048, 16, 1),       # the tokamak's deepest level: one slab of both samples
    (1, 5, 3, 1),
    (1, 20, 1089, 1),       # S >= 1024: the 64-position kernel, 1089 = 17 * 64 + 1: a one-position last tile
    (67, 6, 16, 67),        # one slab per sample, 67 of them
]


def _chan_norm_ref(x, g, gy, mode):
    xd, gd = x.double().requires_grad_(), g.double().requires_grad_()
    gb = gd.reshape(1, -1, 1)
    if mode == 0:
        var = xd.var(dim=1, unbiased=False, keepdim=True)
        y = (xd - xd.mean(dim=1, keepdim=True)) * (var + 1e-5).rsqrt() * gb
    else:
        y = F.normalize(xd, dim=1) * gb * (x.shape[1] ** 0.5)
    y.backward(gy.double())
    return xd.grad, gd.grad


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,Cc,S,ns", CHAN_NORM_SHAPES)
def test_chan_norm_backward_slabs_and_dirty_workspace(B, Cc, S, ns, mode):
    """the C ABI itself, workspace and gx NaN-filled: nothing the kernels leave unwritten can pass for a zero"""
    lib = _lib.get_lib()
    x, g, gy = det_tensor((B, Cc, S), 120), 1 + 0.1 * det_tensor((Cc,), 121), det_tensor((B, Cc, S), 122)
    gx_ref, dg_ref = _chan_norm_ref(x, g, gy, mode)
    xg, gg, gyg = x.to(DEV), g.to(DEV), gy.to(DEV)
    work = torch.full((int(lib.sdc_chan_norm_bwd_bytes(B, Cc, S)) // 4,), float("nan"), dtype=torch.float32, device=DEV)
    gx = torch.full_like(xg, float("nan"))
    assert int(lib.sdc_chan_norm_bwd_parts(B, S)) == B
    table = work[:Cc * B].view(Cc, B)

    def run():
        _lib.check(lib.sdc_chan_norm_bwd(xg.data_ptr(), gyg.data_ptr(), gg.data_ptr(), gx.data_ptr(), work.data_ptr(), B, Cc, S, mode,
                                         C.c_float(1e-5), _stream()), "sdc_chan_norm_bwd")
        return gx.clone(), table.clone()

    gx1, t1 = run()
    assert _finite(gx1, t1)
    e1, e2 = _rel(gx1, gx_ref), _rel(t1.sum(1), dg_ref)
    print(f"[measured] chan_norm_bwd (C ABI, NaN workspace) mode {mode} {(B, Cc, S)}: gx {e1:.2e} dgain {e2:.2e}")
    assert e1 < 2e-5 and e2 < 2e-5
    if ns < B:
        # the slab path was reached (every one of the ns columns is in use) and its contract holds (the rest is exactly 0.0) ...
        assert bool((t1[:, :ns] != 0).any(0).all())
        assert bool((t1[:, ns:] == 0).all())
    if (B, Cc, S) in ((8, 256, 40), (5, 300, 19)):
        assert ns < B
        # ... also when the call runs again into its own, now dirty, workspace (a replayed fine-tuning step)
        table[:, ns:] = float("nan")
        gx2, t2 = run()
        assert torch.equal(t2, t1) and torch.equal(gx2, gx1)


# ------------------------------------------------------------------ 4. gn_silu_bwd, act_bwd, sumpool2 past their caps
def _gn_ref(h, gamma, beta, ss, gy, G):
    B, Cc = h.shape[0], h.shape[1]
    hd, gd, bd = h.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    sd = None if ss is None else ss.double().requires_grad_()
    u = F.group_norm(hd, G, gd, bd, eps=1e-5)
    if ss is not None:
        bshape = (B, Cc) + (1,) * (h.dim() - 2)
        u = u * (sd[:, :Cc].reshape(bshape) + 1) + sd[:, Cc:].reshape(bshape)
    y = F.silu(u)
    y.backward(gy.double())
    return y.detach(), dict(gh=hd.grad, dgamma=gd.grad, dbeta=bd.grad, **({} if ss is None else dict(dss=sd.grad)))


def _gn_inputs(shape, cond, res):
    B, Cc = shape[0], shape[1]
    h = det_tensor(shape, 110)
    gamma, beta = 1 + 0.1 * det_tensor((Cc,), 111), 0.1 * det_tensor((Cc,), 112)
    ss = 0.2 * det_tensor((B, 2 * Cc), 113) if cond else None
    r = det_tensor(shape, 114) if res else None
    return h, gamma, beta, ss, r, det_tensor(shape, 115)


def _gn_errs(got, ref):
    return {k: _rel(v, ref[k]) for k, v in zip(("gh", "dgamma", "dbeta", "dss"), got) if v is not None}


@pytest.mark.parametrize("shape,G,cond,res", [
    # apply pass: grid.y = ceil(S / 2048) pieces per row, at most 64.  S = 33 * 64 * 64 = 135168 > 64 * 2048: 66 -> 64, every
    # thread walks its row more than 8 times and the last stride is ragged (the rows pass cuts the row into 33 fp64 pieces)
    ((1, 8, 33, 64, 64), 2, True, False),
    # flat apply kernel (S < 1024): ceil(40 * 256 * 256 / 256) = 10240 blocks -> 8192, a ragged second grid stride
    ((40, 256, 1, 1, 256), 1, True, True),
])
def test_gn_silu_backward_past_the_grid_caps(shape, G, cond, res):
    h, gamma, beta, ss, r, gy = _gn_inputs(shape, cond, res)
    y_ref, ref = _gn_ref(h, gamma, beta, ss, gy, G)
    hg, gag, beg, ssg = h.to(DEV), gamma.to(DEV), beta.to(DEV), None if ss is None else ss.to(DEV)
    st = grad_ops.gn_stats(hg, G)
    y_hip = grad_ops.gn_apply(hg, st, gag, beg, G, ssg, None if r is None else r.to(DEV))
    assert _rel(y_hip, y_ref + (r.double() if res else 0)) < 1e-5
    errs = _gn_errs(grad_ops.gn_silu_bwd(hg, gy.to(DEV), st, gag, beg, G, ssg), ref)
    print(f"[measured] gn_silu_bwd past the grid caps {shape} G={G}: {errs}")
    assert max(errs.values()) < 5e-5


def test_gn_silu_backward_unaligned_scalar_fallback():
    """h and gy one float into their buffers (4-byte, not 16-byte aligned) at a shape whose rows pass would cut the row into
    fp64 pieces with 16-byte loads: 32 rows of 16384 elements -> gn_bwd_ysplit = min(1024 / 32, 16384 / 4096, 64) = 4 > 1, so the
    rows pass must take gn_bwd_rows_kernel<1> instead.  Against fp64, and against the aligned call (same formula, other order of
    summation: the same gate, not the same bits)"""
    shape, G = (2, 16, 16, 32, 32), 4
    B, Cc, S = shape[0], shape[1], shape[2] * shape[3] * shape[4]
    lib = _lib.get_lib()
    base = ((B * Cc + B * G) * 2 + 1) // 2 * 2
    ysplit = (int(lib.sdc_gn_silu_bwd_floats(B, Cc, G, S)) - base) // (B * Cc * 4)         # the pieces' fp64 pairs, in floats
    assert ysplit > 1, ysplit
    h, gamma, beta, ss, _, gy = _gn_inputs(shape, True, False)
    _, ref = _gn_ref(h, gamma, beta, ss, gy, G)
    hg, gyg, gag, beg, ssg = h.to(DEV), gy.to(DEV), gamma.to(DEV), beta.to(DEV), ss.to(DEV)
    st = grad_ops.gn_stats(hg, G)

    def off1(t):
        v = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    aligned = grad_ops.gn_silu_bwd(hg, gyg, st, gag, beg, G, ssg)
    shifted = grad_ops.gn_silu_bwd(off1(hg), off1(gyg), st, gag, beg, G, ssg)
    errs, errs_al = _gn_errs(shifted, ref), _gn_errs(aligned, ref)
    diff = {k: _rel(a, b) for k, a, b in zip(("gh", "dgamma", "dbeta", "dss"), shifted, aligned)}
    print(f"[measured] gn_silu_bwd unaligned {shape} G={G} (ysplit {ysplit}): vs fp64 {errs} | aligned vs fp64 {errs_al} | vs aligned {diff}")
    assert max(errs.values()) < 5e-5 and max(errs_al.values()) < 5e-5
    assert max(diff.values()) < 5e-5


def test_act_backward_and_sumpool_past_the_grid_cap():
    """both kernels walk a grid-stride loop of at most 8192 blocks of 256 threads"""
    n = 8192 * 256 + 333                                   # one full grid stride and a ragged second one
    x, gy = det_tensor((n,), 130, 2.0), det_tensor((n,), 131)
    errs = {}
    for kind, fn in ((0, F.silu), (1, F.gelu)):
        xd = x.double().requires_grad_()
        fn(xd).backward(gy.double())
        errs[fn.__name__] = _rel(grad_ops.act_bwd(x.to(DEV), gy.to(DEV), kind), xd.grad)
    # 9 * 500 * 500 = 2 250 000 outputs > 8192 * 256 = 2 097 152
    g = det_tensor((9, 1, 1000, 1000), 132)
    xd = torch.zeros((9, 1, 500, 500), dtype=torch.float64).requires_grad_()
    assert xd.numel() > 8192 * 256
    F.interpolate(xd, scale_factor=2, mode="nearest").backward(g.double())
    errs["sumpool2"] = _rel(grad_ops.sumpool2(g.to(DEV), 2, 2), xd.grad)
    print(f"[measured] act_bwd n={n}, sumpool2 (9, 1, 1000, 1000) -> (9, 1, 500, 500): {errs}")
    assert errs["silu"] < 2e-6 and errs["gelu"] < 2e-6
    assert errs["sumpool2"] < 1e-6
