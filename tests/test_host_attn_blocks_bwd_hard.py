"""CPU: the inputs and references of tests/test_gpu_attn_blocks_bwd_hard.py are sound without a GPU.
(a) Every fp64 and fp32 reference gradient of tests/attn_blocks_bwd_hard_ref.py is finite.
(b) e32 -- the fp32 torch restatement of the training-block files' _block_ref against its fp64 run, max |err| over max |ref|, per
    output -- stays below 1e-4 on every family but `offset` and temporal `peak8`, and below 1e-3 on those: the GPU gate max(2e-5, 4 e32)
    is set by fp32 arithmetic on these inputs, never by a loose reference, and never exceeds 4e-3.  Largest gradient e32 when this
    file was written (it moves in its last digits with the BLAS build and the thread count):
        LinearAttention, every family but `offset`   2.6e-5          temporal, every family but `peak8`, `offset`   3.9e-5
        LinearAttention `offset`                     1.1e-4          temporal `peak8`  1.6e-4      temporal `offset`   4.0e-4
(c) On `flat` / `tiny` the degenerate tokens own max |dx|: at least 100 x the median token's (370 x - 6.6e13 x).  That is why dx is
    judged over the rest of the tensor and on each of those tokens alone; both of these e32 figures obey the bounds of (b).
(d) The `tiny` token has 0 < ||x|| < 1e-12: it lies under the RMSNorm clamp and is not zero.
(e) m_s - m of the splits lab_mid1_kernel merges (the forward's pick_nsplit, R.la_splits): a normal factor at x 4, an fp32 subnormal
    at x 6, zero at x 8.
(f) The temporal reference is section 29's block: with the exact angles p * freqs its forward branch is TX._branch of the case to
    1e-12, the table it hands the kernel is those angles rounded to fp32 (at most 2^-20 away), cos and sin taken in fp32."""
import math

import pytest
import torch

import attn_blocks_bwd_hard_ref as B
import attn_blocks_hard_ref as R
import test_gpu_tattn_train as TT

LA_NAMES = ("dx", "dg_pre", "dwqkv", "dwo", "dbo", "dg_post")
TA_NAMES = ("dx", "dg", "dwqkv", "dwo", "dbias")


def _cap(block, tag):
    return 1e-3 if tag == "offset" or (block == "temporal" and tag == "peak8") else 1e-4


def _sound(block, name, tag, case, names):
    assert case.finite, name
    fmt = " ".join(f"{n} {e:.2e}" for n, e in zip(names, case.e32) if e is not None)
    extra = ""
    if case.deg:
        extra = (f" | dx without its {len(case.deg)} degenerate tokens {case.e32_rest:.2e}, on them alone <= {max(case.e32_tok):.2e}; their "
                 f"max |dx| is {case.deg_ratio:.1e} x the median token's")
    print(f"[measured] {block} {name}: e32 {fmt} (cap {_cap(block, tag):.0e}){extra}")
    worst = max([e for e in case.e32 if e is not None] + [case.e32_rest] + case.e32_tok)
    assert worst < _cap(block, tag), (name, worst)
    assert bool(case.deg) == (tag in ("flat", "tiny"))
    if case.deg:
        assert len(case.deg) <= (33 if block == "temporal" else 3)
        assert case.deg_ratio >= 100.0, (name, case.deg_ratio)


def test_the_case_lists_are_the_issues():
    assert len(B.LA_BWD_CASES) == 31 and len(set(B.LA_BWD_CASES)) == 31
    assert len(B.LA_POST_CASES) == 39 and len(set(B.LA_POST_CASES)) == 39
    assert len(B.TA_CASES) == 20
    assert {c[1] for c in B.LA_BWD_CASES} == {"peak2", "peak4", "peak8", "desc", "asc", "small", "large", "offset", "flat", "desc6", "asc6",
                                              "desc8", "asc8"}
    assert {(c[1], c[2], c[3]) for c in B.LA_POST_CASES if c[1] == "tiny"} == {("tiny", 1, 1), ("tiny", 1, 0)}


@pytest.mark.parametrize("c", B.LA_BWD_CASES, ids=R.la_id)
def test_linattn_bwd_case_is_finite_and_its_references_agree(c):
    _sound("sdc_linattn_block_bwd", R.la_id(c), c[1], B.la_bwd_case(*c), LA_NAMES)


@pytest.mark.parametrize("c", B.LA_POST_CASES, ids=R.la_id)
def test_linattn_post_bwd_case_is_finite_and_its_references_agree(c):
    _sound("sdc_linattn_block_post_bwd", R.la_id(c), c[1], B.la_post_case(*c), LA_NAMES)


@pytest.mark.parametrize("c", B.TA_CASES, ids=R.ta_id)
def test_temporal_bwd_case_is_finite_and_its_references_agree(c):
    case = B.ta_case(*c)
    _sound("temporal", R.ta_id(c), c[1], case, TA_NAMES)
    assert (case.ref[4] is None) == (not c[2])


@pytest.mark.parametrize("c", B.TA_CASES, ids=R.ta_id)
def test_temporal_reference_is_section_29s_block(c):
    """_block_ref of tests/test_gpu_tattn_train.py takes the rotary angles and the bias as tables; TX._branch of
    tests/test_gpu_attn_x3.py builds them from freqs and relw.  With the exact angles p * freqs in fp64 the two forward branches agree
    to 1e-12, so x, g, wqkv, wo and the bias (x 8 on bias8) are section 29's.  The angles the reference and the kernel's table are
    built from are those products rounded to fp32, at most half an ulp of a number below 32 away; the branch then moves by the
    figure printed (up to 1.8e-5 at peak8), which is part of neither gate: reference and kernel read the same rounded angles."""
    shape, tag, tables = c
    inp, ang = B.ta_inputs(shape, tag, tables)
    x, g, wqkv, wo, rot, bias, dy = inp
    exact = R.ta_case(shape, tag, tables).exact
    freqs = R.ta_inputs(shape, tag)[4]
    ang64 = None
    if tables:
        ang32 = torch.arange(R.Fr, dtype=torch.float32)[:, None] * freqs[None, :]
        ang64 = (torch.arange(R.Fr, dtype=torch.float64)[:, None] * freqs.double()[None, :]).repeat_interleave(2, dim=-1)
        assert torch.equal(rot, torch.stack((ang32.cos(), ang32.sin()), dim=-1).reshape(-1))            # TX._tables, before the upload
        assert torch.equal(ang, ang32.repeat_interleave(2, dim=-1).double())
        assert (ang - ang64).abs().max().item() <= 2.0 ** -20
        assert bias.shape == (4, R.Fr, R.Fr) and bias.dtype == torch.float32
    else:
        assert rot is None and ang is None and bias is None
    y = TT._block_ref(x, g, wqkv, wo, ang64, bias, dy, torch.float64)[0]
    e_exact = R.rel(y - x.double(), exact)
    print(f"[measured] temporal {R.ta_id(c)}: forward branch of the reference vs section 29's exact branch: {e_exact:.1e} with exact angles, "
          f"{B.ta_case(*c).e_fwd:.1e} with the fp32 table's")
    assert e_exact < 1e-12


@pytest.mark.parametrize("shape", [R.LA_SHAPES[0], R.LA_SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_the_tiny_token_lies_under_the_clamp_and_is_not_zero(shape):
    """0 < ||x|| < 1e-12 in fp64 and in the fp32 sum the kernel forms (x^2 ~ 1e-28 is a normal fp32 number); the flat and the zero
    token of `flat` are still there"""
    x = B.la_inputs(shape, "tiny", 1, 1)[0]
    o, i, t = B.la_tiny_token(shape)
    nrm, nrm32 = x[o, :, i, t].double().norm().item(), x[o, :, i, t].pow(2).sum().sqrt().item()
    print(f"[measured] {shape} tiny token: ||x|| {nrm:.2e} (fp32 {nrm32:.2e})")
    assert 0.0 < nrm < 1e-12 and 0.0 < nrm32 < 1e-12
    (o0, i0, t0), (o1, i1, t1) = R.la_flat_tokens(shape)
    assert len({(o, i, t), (o0, i0, t0), (o1, i1, t1)}) == 3
    assert bool((x[o0, :, i0, t0] == 0.75).all()) and bool((x[o1, :, i1, t1] == 0).all())
    assert min(abs(t - t0), abs(t - t1)) >= R.TT or (o, i) not in ((o0, i0), (o1, i1))


# ------------------------------------------------------------------ m_s - m of the splits the backward walks
_SORTED = [c for c in B.LA_BWD_CASES + B.LA_POST_CASES if c[1].startswith(("desc", "asc"))]


def _la_bid(c):
    return ("bwd-" if c[3] == -1 else "post_bwd-") + R.la_id(c)


@pytest.mark.parametrize("c", _SORTED, ids=_la_bid)
def test_split_maxima_of_the_sorted_cases(c):
    """lab_mid1_kernel merges the splits of the forward's pick_nsplit (R.la_splits) with fsp[s] = exp(m_s - m).  Head 0's 32 key rows
    are one sorted row, so every split but the one holding the maximum is dominated: by 23 - 67 at x 4 (a small NORMAL factor), by
    98 - 101 at x 6 (an fp32 subnormal, or 0 where the exponential flushes) and by more than 104 at x 8 (zero)."""
    shape, tag, pre, post = c
    n, desc = shape[3], tag.startswith("desc")
    k0 = R.la_k(B.la_inputs(shape, tag, pre, post), pre)[:, 0]                       # (outer, d, inner, n)
    assert bool((k0 == k0[:, :1]).all())
    step = k0[..., 1:] - k0[..., :-1]
    assert bool((step <= 0).all() if desc else (step >= 0).all())
    tmax = k0.reshape(*k0.shape[:-1], n // R.TT, R.TT).amax(-1)
    smax = torch.stack([tmax[..., t0:t1].amax(-1) for t0, t1 in R.la_splits(n)], -1)
    gap = smax - smax.amax(-1, keepdim=True)
    dominated = gap[gap < 0]
    if len(R.la_splits(n)) == 1:
        assert dominated.numel() == 0
        print(f"[measured] {_la_bid(c)}: one split, max |k| {k0.abs().max().item():.1f}")
        return
    hi, lo = dominated.max().item(), dominated.min().item()
    print(f"[measured] {_la_bid(c)}: dominated splits' m_s - m {hi:.1f} .. {lo:.1f}, max |k| {k0.abs().max().item():.1f}")
    assert dominated.numel() == gap.numel() - gap[..., 0].numel()
    scale = R._PEAK.get(tag, 4.0)
    if scale == 4.0:
        assert hi < -16.0 and lo > math.log(2.0 ** -126)
    elif scale == 6.0:
        assert hi < math.log(2.0 ** -126) and lo > math.log(2.0 ** -149)
    else:
        assert hi < math.log(2.0 ** -150)
