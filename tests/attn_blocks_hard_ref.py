"""Inputs and references shared by tests/test_host_attn_blocks_hard.py and tests/test_gpu_attn_blocks_hard.py: the forward of the fused
LinearAttention block (csrc/sdc_lablock.hip, sdc_lablock_x3.hip, sdc_lablock_f16.hip) and of the width-64 temporal-attention block
(csrc/sdc_tablock.hip, sdc_tablock_x3.hip, sdc_tablock_f16.hip) on inputs that trained attention produces and det_tensor at scale
0.3 - 0.4 does not: rows close to one-hot, a running maximum that settles at once or moves in every tile, splits dominated by another
split, eps-dominated norms, a large common offset, flat and all-zero tokens.  The base inputs and the fp64 formulas
are those of the four block test files, imported, not copied.  Everything here is CPU torch, computed once per case and never modified."""
import collections
import functools

import torch

import test_gpu_attn_f16 as TF
import test_gpu_attn_x3 as TX
import test_gpu_linattn_f16 as LF
import test_gpu_linattn_x3 as LX
from oracle import nets as onets

TT = 64               # tokens per tile of the LinearAttention kernels
Fr = TX.Fr

# one case: the inputs (fp32, as uploaded), the exact fp64 branch y - x, its fp32 torch restatement (as fp64), the fp64 emulation of the
# fp16 entry (None where there is none), e32 = rel(f32, exact), e_in = rms(emu - exact) / rms(exact), r_out = what the rounding of the
# output y = x + branch to fp32 alone costs (out_rounding below) and e_in_max = rel(emu, exact), e_in in the max measure
Case = collections.namedtuple("Case", "inp exact f32 emu e32 e_in r_out e_in_max")


def rel(a, b):
    """_rel of tests/test_gpu_grad.py"""
    return ((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def rms_rel(a, b):
    """rms of a - b over the rms of b: the measure of tests/test_gpu_linattn_f16.py and tests/test_gpu_attn_f16.py"""
    return ((a.double() - b.double()).pow(2).mean().sqrt() / b.double().pow(2).mean().sqrt()).item()


def out_rounding(x, exact):
    """what no entry can avoid: y = x + branch is stored as fp32, and the tests take y - x in fp64.  rel of the exact branch pushed through
    that one rounding: half an ulp of |x + branch| over the branch scale.  Below 3e-7 on every family but `large` (x * 1e3), where it is
    1.3e-5 - 2.4e-5 of the LinearAttention branch's scale -- above the 1e-5 floor of the gate.  e32 stays what the formula costs in fp32;
    the GPU gate is max(1e-5, 4 e32) + r_out, so the unavoidable term is added once and not multiplied by 4."""
    assert x.dtype == torch.float32
    return rel((x.double() + exact).float().double() - x.double(), exact)


def _half(t):
    return t.half().double()


# ------------------------------------------------------------------ LinearAttention block
# (outer, inner, C, n)
LA_SHAPES = [
    (1, 2, 64, 1024),     # two splits; the route sdc_linattn_block takes by default (impl 1)
    (2, 1, 64, 1088),     # 17 tiles: uneven splits 9 + 8
    (1, 1, 64, 4096),     # eight splits: the fsp[8] table of la_blk_mid is full
    (1, 1, 128, 512),     # C = 128, one split; routed to impl 1
    (1, 2, 128, 1024),    # C = 128, two splits
]
# (tag, pre_mode, post_mode)
LA_EVERYWHERE = [("peak4", 0, -1), ("desc", 0, -1), ("asc", 0, -1)]
LA_ELSEWHERE = [("peak2", 0, -1), ("peak8", 0, -1), ("small", 0, -1), ("large", 0, -1), ("offset", 0, -1), ("flat", 0, -1), ("flat", 1, 1),
                ("post", 0, 0), ("post", 1, 1)]
# desc / asc on x 6 and x 8 instead of x 4 at the C = 128 two-split shape: the dominated split's maximum lies 98 - 101 / 131 - 134 below the
# row's, so la_blk_mid's exp(m_s - m) is a subnormal / exactly 0 (at x 4 it is 66 - 67 below and the factor a normal 8e-30)
LA_MERGE = [("desc6", 0, -1), ("asc6", 0, -1), ("desc8", 0, -1), ("asc8", 0, -1)]
LA_CASES = ([(s, *f) for s in LA_SHAPES for f in LA_EVERYWHERE] + [(s, *f) for s in (LA_SHAPES[0], LA_SHAPES[3]) for f in LA_ELSEWHERE] +
            [(LA_SHAPES[4], *f) for f in LA_MERGE])
_PEAK = {"peak2": 2.0, "peak8": 8.0, "desc6": 6.0, "asc6": 6.0, "desc8": 8.0, "asc8": 8.0}          # every other family sits on peak4


def la_splits(n):
    """the tile ranges [t0, t1) of pass 1's token splits: pick_nsplit of csrc/sdc_lablock_tile.h and the launch of csrc/sdc_lablock.hip"""
    ntiles = n // TT
    ns = max(1, min(8, ntiles // 8))
    tps = (ntiles + ns - 1) // ns
    return [(t0, min(t0 + tps, ntiles)) for t0 in range(0, ntiles, tps)]


def la_id(case):
    (outer, inner, Cc, n), tag, pre, post = case
    return f"{outer}x{inner}x{Cc}x{n}-{tag}-pre{pre}-post{post}"


def la_flat_tokens(shape):
    """(outer, inner, token) of the token with all channels 0.75 and of the all-zero token"""
    outer, inner, _, n = shape
    return (0, 0, 5), (outer - 1, inner - 1, n - 24)


def la_k(inp, pre):
    """the keys of a case in fp64: (outer, heads, d, inner, n)"""
    x, g1, _, wqkv, _, _ = inp
    B, Cc, inner, n = x.shape
    xn = LX._norm(x.double(), g1.double(), pre, Cc)
    return torch.einsum("oc,bcfn->bofn", wqkv.double()[128:256], xn).reshape(B, 4, 32, inner, n)


def la_inputs(shape, tag, pre, post):
    outer, inner, Cc, n = shape
    x, g1, g2, wqkv, wo, bo = LX._inputs(outer, inner, Cc, n, pre, post)
    x, wqkv = x.clone(), wqkv.clone()
    wqkv[:256] *= _PEAK.get(tag, 4.0)
    if tag.startswith(("desc", "asc")):
        # every k row of head 0 is the head's first: one token order sorts all 32 rows of the wave that owns the head.  The channel
        # norm is per token, so permuting the tokens of a sequence permutes its k rows
        wqkv[128:160] = wqkv[128].clone()
        k0 = torch.einsum("c,bcfn->bfn", wqkv[128].double(), LX._norm(x.double(), g1.double(), pre, Cc))
        order = k0.argsort(-1, descending=tag.startswith("desc"))[:, None].expand(outer, Cc, inner, n)
        x = x.gather(-1, order).contiguous()
    elif tag == "small":
        x = x * 1e-3
    elif tag == "large":
        x = x * 1e3
    elif tag == "offset":
        x = x + 50.0                 # formed in fp32: this tensor is what the kernels and every reference read
    elif tag == "flat":
        (o0, i0, t0), (o1, i1, t1) = la_flat_tokens(shape)
        x[o0, :, i0, t0] = 0.75
        x[o1, :, i1, t1] = 0.0
    elif tag == "post":
        wo, bo = wo * 1e-2, torch.zeros_like(bo)
    assert x.dtype == torch.float32
    return x, g1, g2, wqkv, wo, bo


def _la_f32(x, g1, g2, wqkv, wo, bo, pre, post):
    """LX._branch with every tensor left in fp32"""
    B, Cc, inner, n = x.shape
    xn = LX._norm(x, g1, pre, Cc)
    q = torch.einsum("oc,bcfn->bofn", wqkv[:128], xn).reshape(B, 4, 32, inner, n)
    k = torch.einsum("oc,bcfn->bofn", wqkv[128:256], xn).reshape(B, 4, 32, inner, n)
    v = torch.einsum("oc,bcfn->bofn", wqkv[256:], xn).reshape(B, 4, 32, inner, n)
    ctx = torch.einsum("bhdfn,bhefn->bhfde", k.softmax(-1), v)
    T = torch.einsum("cme,bmfde->bfcmd", wo.reshape(Cc, 4, 32), ctx)
    y = torch.einsum("bfcmd,bmdfn->bcfn", T, q.softmax(2) * 32 ** -0.5) + bo.view(1, -1, 1, 1)
    y = LX._norm(y, g2, post, Cc) if post >= 0 else y
    assert y.dtype == torch.float32
    return y


def la_refs(inp, pre, post):
    """the references of one set of inputs (x, g1, g2, wqkv, wo, bo)"""
    exact = LX._branch(*inp, pre, post)
    emu = LF._branch(*inp, pre, post, _half)
    f32 = _la_f32(*inp, pre, post).double()
    return Case(inp, exact, f32, emu, rel(f32, exact), rms_rel(emu, exact), out_rounding(inp[0], exact), rel(emu, exact))


@functools.lru_cache(maxsize=None)
def la_case(shape, tag, pre, post):
    return la_refs(la_inputs(shape, tag, pre, post), pre, post)


@functools.lru_cache(maxsize=None)
def la_base_stats(shape):
    """the median over rows of the largest key probability at scale 1 and at peak4"""
    out = []
    for inp in (LX._inputs(*shape, 0, -1), la_inputs(shape, "peak4", 0, -1)):
        out.append(la_k(inp, 0).softmax(-1).amax(-1).median().item())
    return tuple(out)


# ------------------------------------------------------------------ temporal-attention block (width 64, 32 frames)
# (B, H, W)
TA_SHAPES = [
    (2, 4, 8),            # eight pixel groups: the XCD-ordered walk
    (1, 3, 8),            # three groups: the plain walk
]
TA_TAGS = ["peak2", "peak4", "peak8", "bias8", "bias8+peak4", "small", "large", "offset", "flat"]
# (shape, tag, tables)
TA_CASES = [(s, t, True) for s in TA_SHAPES for t in TA_TAGS] + [(s, "peak4", False) for s in TA_SHAPES]


def ta_id(case):
    (B, H, W), tag, tables = case
    return f"{B}x{H}x{W}-{tag}" + ("" if tables else "-null-tables")


def ta_flat_pixels(shape):
    """(b, frame, h, w) of the token with all channels 0.75 and (b, h, w) of the pixel that is zero in every frame"""
    return (0, 3, 1, 2), (shape[0] - 1, 2, 5)


def ta_inputs(shape, tag):
    x, g, wqkv, wo, freqs, relw = TX._inputs(*shape)
    x, wqkv = x.clone(), wqkv.clone()
    if tag != "bias8":
        wqkv[:256] *= _PEAK.get(tag, 4.0)
    if tag.startswith("bias8"):
        relw = relw * 8.0
    if tag == "small":
        x = x * 1e-3
    elif tag == "large":
        x = x * 1e3
    elif tag == "offset":
        x = x + 50.0
    elif tag == "flat":
        (b0, f0, h0, w0), (b1, h1, w1) = ta_flat_pixels(shape)
        x[b0, :, f0, h0, w0] = 0.75
        x[b1, :, :, h1, w1] = 0.0
    assert x.dtype == torch.float32
    return x, g, wqkv, wo, freqs, relw


def _ta_scores(x, g, wqkv, freqs, relw, tables, eps=1e-5):
    """the scores (pixels, heads, query, key) and v of TX._branch in the dtype of x"""
    B, _, _, H, W = x.shape
    xn = (x - x.mean(1, keepdim=True)) * (x.var(1, unbiased=False, keepdim=True) + eps).rsqrt() * g.to(x.dtype).view(1, -1, 1, 1, 1)
    tok = xn.permute(0, 3, 4, 2, 1).reshape(B * H * W, Fr, 64)
    q, k, v = (tok @ wqkv.to(x.dtype).t()).chunk(3, -1)
    sp = lambda t: t.reshape(-1, Fr, 4, 32).permute(0, 2, 1, 3)      # noqa: E731
    q, k, v = sp(q), sp(k), sp(v)
    if tables:
        q, k = onets.rotary(q, freqs.to(x.dtype)), onets.rotary(k, freqs.to(x.dtype))
    s = (q @ k.transpose(-1, -2)) * 32 ** -0.5
    if tables:
        s = s + onets.rel_pos_bias(relw, Fr).to(x.dtype)[None]
    return s, v


def _ta_f32(x, g, wqkv, wo, freqs, relw, tables):
    """TX._branch with every tensor left in fp32"""
    B, _, _, H, W = x.shape
    s, v = _ta_scores(x, g, wqkv, freqs, relw, tables)
    out = (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(-1, Fr, 128) @ wo.t()
    assert out.dtype == torch.float32
    return out.reshape(B, H, W, Fr, 64).permute(0, 4, 3, 1, 2)


def ta_max_score(inp, tables):
    """the largest |score| in front of the softmax, in fp64"""
    x, g, wqkv, _, freqs, relw = inp
    return _ta_scores(x.double(), g, wqkv, freqs, relw, tables)[0].abs().max().item()


def ta_refs(inp, tables):
    exact = TX._branch(*inp, rot=tables, bias=tables)
    f32 = _ta_f32(*inp, tables).double()
    emu, e_in, e_in_max = None, None, None
    if tables:                                   # sdc_tattn_block_f16 needs its tables
        emu = TF._branch(*inp, _half)
        e_in, e_in_max = rms_rel(emu, exact), rel(emu, exact)
    return Case(inp, exact, f32, emu, rel(f32, exact), e_in, out_rounding(inp[0], exact), e_in_max)


@functools.lru_cache(maxsize=None)
def ta_case(shape, tag, tables):
    return ta_refs(ta_inputs(shape, tag), tables)
