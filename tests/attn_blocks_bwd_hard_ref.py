"""Inputs and references shared by tests/test_host_attn_blocks_bwd_hard.py and tests/test_gpu_attn_blocks_bwd_hard.py: the three backward
entries of the fused attention blocks -- sdc_linattn_block_bwd and sdc_linattn_block_post_bwd (csrc/sdc_lablock_bwd.hip),
sdc_tattn_block_bwd (csrc/sdc_tablock_bwd.hip) -- on the hard inputs of tests/attn_blocks_hard_ref.py (DESIGN.md sections 29, 30).
The inputs are that file's la_inputs / ta_inputs plus the dy of the training-block files (det_tensor seeds 405 / 305); the references
are the _block_ref functions of the three training-block files, run once in fp64 and once in fp32.  All of it is imported, not copied.

A `flat` input has tokens whose norm backward multiplies by rstd = eps^-1/2 (LayerNorm at var = 0) or by sqrt(C) / 1e-12 (RMSNorm under
its clamp), so their dx is 1e2 - 1e14 times any other token's and they own max |dx|.  These degenerate tokens are listed per case
(Case.deg); dx is then measured over the rest of the tensor and on each of them alone (rel_rest, rel_token).  Everything here is CPU
torch, computed once per case and never modified."""
import collections
import functools

import torch

import attn_blocks_hard_ref as R
import test_gpu_linattn_post_train as LP
import test_gpu_linattn_train as LT
import test_gpu_tattn_train as TT
from oracle import nets as onets
from oracle.detweights import det_tensor
from test_gpu_grad import _rot_table

rel = R.rel
Fr = R.Fr

# one case: inp as the training-block file's _run_abi takes it; ref the fp64 outputs behind y (dx first; None where the entry has no
# such output); e32 the fp32 restatement against fp64 per output, rel; deg the degenerate tokens as index tuples into dx; e32_rest /
# e32_tok the fp32 restatement of dx over the rest of the tensor / on each degenerate token; deg_ratio the largest max |dx| of a
# degenerate token over the median token's; finite: every fp64 and fp32 output is; e_fwd (temporal): rel of the reference's forward
# branch against attn_blocks_hard_ref's exact branch
Case = collections.namedtuple("Case", "inp ref e32 deg e32_rest e32_tok deg_ratio finite e_fwd")


def rel_rest(a, b, deg):
    """rel over the tensor with the degenerate tokens removed from both the error and the scale"""
    err, ref = (a.double().cpu() - b.double()).abs(), b.double().abs().clone()
    for idx in deg:
        err[idx] = 0.0
        ref[idx] = 0.0
    return (err.max() / ref.max().clamp_min(1e-30)).item()


def rel_token(a, b, idx):
    """rel of one token's channels: max |err| over max |ref| of that token"""
    return rel(a[idx], b[idx])


def _finish(inp, ref, f32, deg, e_fwd=None):
    e32 = [None if b is None else rel(a, b) for a, b in zip(f32[1:], ref[1:])]
    dx, dx32 = ref[1], f32[1]
    ratio = None
    if deg:
        per_token = dx.abs().amax(1)
        ratio = (max(dx[idx].abs().max() for idx in deg) / per_token.median()).item()
    finite = all(bool(torch.isfinite(t).all()) for t in ref + f32 if t is not None)
    return Case(inp, ref[1:], e32, deg, rel_rest(dx32, dx, deg) if deg else e32[0], [rel_token(dx32, dx, idx) for idx in deg], ratio, finite,
                e_fwd)


# ------------------------------------------------------------------ LinearAttention block: the inputs
TINY_SEED, TINY_SCALE = 999, 1e-14


def la_tiny_token(shape):
    """(outer, inner, token) of the `tiny` token: away from the flat token (0, 0, 5) and the zero token (outer - 1, inner - 1, n - 24)"""
    return (0, 0, shape[3] // 2 + 7)


def la_inputs(shape, tag, pre, post):
    """R.la_inputs, plus the family `tiny`: `flat` and one more token with 0 < ||x|| <= 1e-12 (8.8e-14 at C = 64), the only kind of
    token at which mode 1's `live` flag decides anything -- at ||x|| = 0 the term it drops is 0 anyway"""
    if tag != "tiny":
        return R.la_inputs(shape, tag, pre, post)
    x, *rest = R.la_inputs(shape, "flat", pre, post)
    o, i, t = la_tiny_token(shape)
    x[o, :, i, t] = TINY_SCALE * det_tensor((shape[2],), TINY_SEED)
    return (x, *rest)


def la_degenerate(shape, tag):
    """(outer, inner, token) of the degenerate tokens of a case: at most 3"""
    if tag == "flat":
        return list(R.la_flat_tokens(shape))
    if tag == "tiny":
        return list(R.la_flat_tokens(shape)) + [la_tiny_token(shape)]
    return []


def la_dy(shape):
    outer, inner, Cc, n = shape
    return det_tensor((outer, Cc, inner, n), 405)


# ------------------------------------------------------------------ sdc_linattn_block_bwd: modes (0, -1)
LA_BWD_CASES = [c for c in R.LA_CASES if (c[2], c[3]) == (0, -1)]


def la_bwd_inputs(shape, tag):
    """the inputs as test_gpu_linattn_train._run_abi takes them: (outer, C, inner, n) becomes (B, C, F, H, W) = (outer, C, inner, 1, n)"""
    outer, inner, Cc, n = shape
    x, g1, _, wqkv, wo, bo = la_inputs(shape, tag, 0, -1)
    return x.reshape(outer, Cc, inner, 1, n), g1, wqkv, wo, bo, la_dy(shape).reshape(outer, Cc, inner, 1, n)


@functools.lru_cache(maxsize=None)
def la_bwd_case(shape, tag, pre=0, post=-1):
    assert (pre, post) == (0, -1)
    inp = la_bwd_inputs(shape, tag)
    deg = [(o, slice(None), i, 0, t) for o, i, t in la_degenerate(shape, tag)]
    return _finish(inp, LT._block_ref(*inp, torch.float64), LT._block_ref(*inp, torch.float32), deg)


# ------------------------------------------------------------------ sdc_linattn_block_post_bwd
_S = R.LA_SHAPES
LA_POST_CASES = ([(s, t, m, m) for s in (_S[0], _S[3]) for m in (0, 1) for t in ("peak4", "desc", "asc", "small", "offset", "flat", "post")] +
                 [(_S[0], "peak4", 0, 1), (_S[0], "peak4", 1, 0), (_S[1], "peak4", 0, 0), (_S[1], "peak4", 1, 1), (_S[2], "desc", 1, 1),
                  (_S[4], "desc8", 1, 1), (_S[4], "asc8", 1, 1)] +
                 [(s, "tiny", 1, p) for s in (_S[0], _S[3]) for p in (1, 0)])


def la_post_inputs(shape, tag, pre, post):
    """the inputs as test_gpu_linattn_post_train._run_abi takes them"""
    x, g1, g2, wqkv, wo, bo = la_inputs(shape, tag, pre, post)
    return x, g1, wqkv, wo, bo, g2, la_dy(shape)


@functools.lru_cache(maxsize=None)
def la_post_case(shape, tag, pre, post):
    inp = la_post_inputs(shape, tag, pre, post)
    deg = [(o, slice(None), i, t) for o, i, t in la_degenerate(shape, tag)]
    return _finish(inp, LP._block_ref(*inp, (pre, post), torch.float64), LP._block_ref(*inp, (pre, post), torch.float32), deg)


# ------------------------------------------------------------------ sdc_tattn_block_bwd
TA_CASES = R.TA_CASES


def ta_inputs(shape, tag, tables):
    """the inputs as test_gpu_tattn_train._run_abi takes them, and the angles of the reference: the rotary table of
    test_gpu_grad._rot_table and bias = rel_pos_bias(relw) with the case's relw (x 8 on bias8), or no tables at all"""
    x, g, wqkv, wo, freqs, relw = R.ta_inputs(shape, tag)
    rot, ang = _rot_table(Fr)
    bias = onets.rel_pos_bias(relw, Fr).float().contiguous()
    if not tables:
        rot = ang = bias = None
    return (x, g, wqkv, wo, rot, bias, det_tensor(x.shape, 305)), ang


def ta_degenerate(shape, tag):
    """the flat token and the 32 frames of the zero pixel: 33 index tuples into dx"""
    if tag != "flat":
        return []
    (b0, f0, h0, w0), (b1, h1, w1) = R.ta_flat_pixels(shape)
    return [(b0, slice(None), f0, h0, w0)] + [(b1, slice(None), f, h1, w1) for f in range(Fr)]


@functools.lru_cache(maxsize=None)
def ta_case(shape, tag, tables):
    inp, ang = ta_inputs(shape, tag, tables)
    x, g, wqkv, wo, _, bias, dy = inp
    ref = TT._block_ref(x, g, wqkv, wo, ang, bias, dy, torch.float64)
    f32 = TT._block_ref(x, g, wqkv, wo, ang, bias, dy, torch.float32)
    e_fwd = rel(ref[0] - x.double(), R.ta_case(shape, tag, tables).exact)
    return _finish(inp, ref, f32, ta_degenerate(shape, tag), e_fwd)
