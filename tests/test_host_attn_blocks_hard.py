"""CPU: the hard inputs of tests/test_gpu_attn_blocks_hard.py are hard, and its references are sound without a GPU.
(a) Every exact fp64 branch, every fp32 restatement and every fp16 emulation of tests/attn_blocks_hard_ref.py is finite.
(b) peak4 makes the key softmax of the LinearAttention block close to one-hot; desc / asc put head 0's row maxima into the first /
    the last tile; the maxima of the splits la_blk_mid merges lie far below the row's -- a normal factor at x 4, a subnormal at x 6
    and 0 at x 8 on (1, 2, 128, 1024); the flat and zero tokens normalise to 0.
(c) e32 -- the fp32 torch restatement against fp64, max |err| over max |ref| -- stays below 1e-4 (1e-3 for `offset`): the GPU gate
    max(1e-5, 4 e32) is then set by fp32 arithmetic on these inputs and never by a loose reference.
(d) e_in -- the fp16 emulation against the exact block, rms -- lies within [0.7, 1.5] x the value recorded below."""
import math

import pytest
import torch

import attn_blocks_hard_ref as R
import test_gpu_attn_f16 as TF
import test_gpu_linattn_x3 as LX

# (e32, e_in) per case as measured on the CPU when this file was written.  e32 moves in its last digits with the BLAS build and the
# thread count (the order of fp32 sums); e_in does not.  LinearAttention: e_in grows with the peak scale (8.0e-4 at scale 1 ->
# 1.1e-3 -> 1.5e-3 -> 2.2e-3 at C = 64 / n = 1024).  e32 is of the formula alone; what the rounding of the output y = x + branch costs
# is Case.r_out (2.4e-5 / 1.3e-5 of the branch on LinearAttention `large`, below 3e-7 on every family but `large`).
LA_TABLE = {
    "1x2x64x1024-peak4-pre0-post-1": (2.78e-06, 1.51e-03),
    "1x2x64x1024-desc-pre0-post-1": (2.95e-06, 1.34e-03),
    "1x2x64x1024-asc-pre0-post-1": (2.93e-06, 1.34e-03),
    "2x1x64x1088-peak4-pre0-post-1": (2.56e-06, 1.46e-03),
    "2x1x64x1088-desc-pre0-post-1": (1.73e-06, 1.24e-03),
    "2x1x64x1088-asc-pre0-post-1": (1.74e-06, 1.24e-03),
    "1x1x64x4096-peak4-pre0-post-1": (2.46e-06, 1.67e-03),
    "1x1x64x4096-desc-pre0-post-1": (2.83e-06, 1.69e-03),
    "1x1x64x4096-asc-pre0-post-1": (2.77e-06, 1.69e-03),
    "1x1x128x512-peak4-pre0-post-1": (5.47e-06, 1.64e-03),
    "1x1x128x512-desc-pre0-post-1": (6.02e-06, 1.43e-03),
    "1x1x128x512-asc-pre0-post-1": (6.04e-06, 1.43e-03),
    "1x2x128x1024-peak4-pre0-post-1": (4.66e-06, 1.94e-03),
    "1x2x128x1024-desc-pre0-post-1": (4.47e-06, 1.67e-03),
    "1x2x128x1024-asc-pre0-post-1": (4.47e-06, 1.67e-03),
    "1x2x64x1024-peak2-pre0-post-1": (1.62e-06, 1.10e-03),
    "1x2x64x1024-peak8-pre0-post-1": (4.84e-06, 2.16e-03),
    "1x2x64x1024-small-pre0-post-1": (8.38e-07, 8.15e-04),
    "1x2x64x1024-large-pre0-post-1": (2.81e-06, 1.51e-03),
    "1x2x64x1024-offset-pre0-post-1": (2.63e-05, 1.51e-03),
    "1x2x64x1024-flat-pre0-post-1": (2.69e-06, 1.51e-03),
    "1x2x64x1024-flat-pre1-post1": (5.86e-06, 1.55e-03),
    "1x2x64x1024-post-pre0-post0": (3.10e-06, 1.57e-03),
    "1x2x64x1024-post-pre1-post1": (5.59e-06, 1.56e-03),
    "1x1x128x512-peak2-pre0-post-1": (3.58e-06, 1.20e-03),
    "1x1x128x512-peak8-pre0-post-1": (7.69e-06, 2.15e-03),
    "1x1x128x512-small-pre0-post-1": (1.44e-06, 9.35e-04),
    "1x1x128x512-large-pre0-post-1": (6.23e-06, 1.62e-03),
    "1x1x128x512-offset-pre0-post-1": (3.32e-05, 1.65e-03),
    "1x1x128x512-flat-pre0-post-1": (5.52e-06, 1.64e-03),
    "1x1x128x512-flat-pre1-post1": (6.94e-06, 1.61e-03),
    "1x1x128x512-post-pre0-post0": (8.06e-06, 1.70e-03),
    "1x1x128x512-post-pre1-post1": (6.88e-06, 1.62e-03),
    "1x2x128x1024-desc6-pre0-post-1": (5.92e-06, 2.20e-03),
    "1x2x128x1024-asc6-pre0-post-1": (5.97e-06, 2.20e-03),
    "1x2x128x1024-desc8-pre0-post-1": (6.20e-06, 2.54e-03),
    "1x2x128x1024-asc8-pre0-post-1": (6.22e-06, 2.54e-03),
}
# temporal: e_in 1.2e-3 at scale 1 -> 2.1e-3 -> 4.0e-3 -> 7.7e-3 (q and k are rounded to fp16 in front of a score that the scale
# multiplies); e32 grows with the scores the same way, and `offset` costs the LayerNorm's centring (x + 50 in fp32: 2.5e-4)
TA_TABLE = {
    "2x4x8-peak2": (4.24e-06, 2.11e-03),
    "2x4x8-peak4": (1.98e-05, 3.99e-03),
    "2x4x8-peak8": (4.22e-05, 7.71e-03),
    "2x4x8-bias8": (1.37e-06, 1.11e-03),
    "2x4x8-bias8+peak4": (1.47e-05, 3.93e-03),
    "2x4x8-small": (1.83e-06, 1.38e-03),
    "2x4x8-large": (1.55e-05, 4.09e-03),
    "2x4x8-offset": (2.47e-04, 3.94e-03),
    "2x4x8-flat": (1.98e-05, 4.02e-03),
    "1x3x8-peak2": (3.96e-06, 2.13e-03),
    "1x3x8-peak4": (1.61e-05, 3.95e-03),
    "1x3x8-peak8": (5.00e-05, 6.94e-03),
    "1x3x8-bias8": (2.17e-06, 1.09e-03),
    "1x3x8-bias8+peak4": (1.15e-05, 3.99e-03),
    "1x3x8-small": (1.45e-06, 1.33e-03),
    "1x3x8-large": (1.58e-05, 3.92e-03),
    "1x3x8-offset": (2.12e-04, 3.84e-03),
    "1x3x8-flat": (1.61e-05, 4.00e-03),
    "2x4x8-peak4-null-tables": (2.15e-05, None),
    "1x3x8-peak4-null-tables": (1.48e-05, None),
}


def _sound(name, tag, case, table):
    assert all(bool(torch.isfinite(t).all()) for t in (case.exact, case.f32) + case.inp)
    e32_was, e_in_was = table[name]
    print(f"[measured] {name}: e32 {case.e32:.2e} (recorded {e32_was:.2e})" +
          ("" if case.emu is None else f" | e_in {case.e_in:.2e} (recorded {e_in_was:.2e})"))
    assert case.e32 < (1e-3 if tag == "offset" else 1e-4), case.e32
    assert (case.emu is None) == (e_in_was is None)
    if case.emu is not None:
        assert torch.isfinite(case.emu).all()
        assert 0.7 * e_in_was <= case.e_in <= 1.5 * e_in_was, (case.e_in, e_in_was)


def test_the_tables_list_the_cases():
    assert sorted(LA_TABLE) == sorted(map(R.la_id, R.LA_CASES)) and sorted(TA_TABLE) == sorted(map(R.ta_id, R.TA_CASES))


@pytest.mark.parametrize("case", R.LA_CASES, ids=R.la_id)
def test_linattn_case_is_finite_and_its_references_agree(case):
    _sound(R.la_id(case), case[1], R.la_case(*case), LA_TABLE)


@pytest.mark.parametrize("case", R.TA_CASES, ids=R.ta_id)
def test_temporal_case_is_finite_and_its_references_agree(case):
    _sound(R.ta_id(case), case[1], R.ta_case(*case), TA_TABLE)


def test_the_two_temporal_files_state_one_exact_block():
    """the exact branch comes from tests/test_gpu_attn_x3.py, the emulation from tests/test_gpu_attn_f16.py: with the identity as the
    rounding the second is the first"""
    case = R.ta_case((1, 3, 8), "bias8+peak4", True)
    assert R.rel(TF._branch(*case.inp, lambda t: t), case.exact) < 1e-13


@pytest.mark.parametrize("shape", [R.LA_SHAPES[0], R.LA_SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_peak4_keys_are_close_to_one_hot(shape):
    """the median over the (head, d, sequence) rows of the largest key probability: 0.26 / 0.48 on the existing tests' inputs at
    C = 64 / 128, 0.886 / 0.968 with the q and k rows of wqkv x 4"""
    base, peaked = R.la_base_stats(shape)
    print(f"[measured] {shape}: median row maximum of the key softmax {base:.3f} at scale 1, {peaked:.3f} at peak4")
    assert peaked >= 0.85 and base < 0.5


def _sorted_case(shape, tag):
    """head 0's key row of a desc / asc case, checked to be one sorted row; -> (per-tile maxima, per-split maxima) with the splits
    la_blk_ctx walks (contiguous tile ranges: 8 tiles each, 9 + 8 at 17 tiles)"""
    n = shape[3]
    desc = tag.startswith("desc")
    k0 = R.la_k(R.la_inputs(shape, tag, 0, -1), 0)[:, 0]                       # (outer, d, inner, n)
    assert bool((k0 == k0[:, :1]).all())                                       # head 0's 32 rows are one row
    step = k0[..., 1:] - k0[..., :-1]
    assert bool((step <= 0).all() if desc else (step >= 0).all())
    assert bool((k0.argmax(-1) // R.TT == (0 if desc else n // R.TT - 1)).all())
    tmax = k0.reshape(*k0.shape[:-1], n // R.TT, R.TT).amax(-1)
    # every tile lowers (desc) / raises (asc) the maximum
    assert bool(((tmax[..., 1:] - tmax[..., :-1]) < 0).all() if desc else ((tmax[..., 1:] - tmax[..., :-1]) > 0).all())
    smax = torch.stack([tmax[..., t0:t1].amax(-1) for t0, t1 in R.la_splits(n)], -1)
    return tmax, smax


def test_the_split_layout_is_the_kernels():
    assert R.la_splits(1024) == [(0, 8), (8, 16)] and R.la_splits(1088) == [(0, 9), (9, 17)] and R.la_splits(512) == [(0, 8)]
    assert R.la_splits(4096) == [(8 * i, 8 * i + 8) for i in range(8)]


@pytest.mark.parametrize("shape", R.LA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_desc_and_asc_put_head_0s_maxima_in_the_first_and_the_last_tile(shape):
    """desc: every row of head 0 has its maximum in tile 0 and descends, so the running maximum of la_blk_ctx is final after the first
    tile; every later tile lies below it, and the far tile by more than 16 (exp < 2^-23: its probabilities vanish against the first
    tile's inside la_blk_ctx).  asc is the mirror image: the maximum moves in every tile and sits in the last tile of the last split.
    What la_blk_mid sees is another quantity: m_s, the maximum of a whole split, which for a dominated split is the largest key of
    its tile range.  It lies 23 - 50 (C = 64) and 66 - 67 (C = 128) below the row's at x 4: exp(m_s - m) is small and NORMAL on these
    ten cases (the smallest 8e-30); the subnormal and the zero factor are the cases of the next test."""
    for tag in ("desc", "asc"):
        tmax, smax = _sorted_case(shape, tag)
        far = tmax[..., -1] if tag == "desc" else tmax[..., 0]
        far_gap = (far - tmax.amax(-1)).max().item()
        assert far_gap < -16.0
        gap = smax - smax.amax(-1, keepdim=True)
        dominated = gap[gap < 0]
        if len(R.la_splits(shape[3])) == 1:
            assert dominated.numel() == 0
            print(f"[measured] {shape} {tag}: far tile {far_gap:.1f} below the row maximum; one split")
            continue
        print(f"[measured] {shape} {tag}: far tile {far_gap:.1f} below the row maximum; dominated splits' m_s - m "
              f"{dominated.max().item():.1f} .. {dominated.min().item():.1f}")
        # every split but the one holding the maximum is dominated by more than one fp32 ulp, and its factor is a normal number
        assert dominated.numel() == gap.numel() - gap[..., 0].numel()
        assert dominated.max().item() < -16.0 and dominated.min().item() > math.log(2.0 ** -126)


@pytest.mark.parametrize("tag,lo,hi", [("desc6", 2.0 ** -149, 2.0 ** -126), ("asc6", 2.0 ** -149, 2.0 ** -126), ("desc8", None, 2.0 ** -150),
                                       ("asc8", None, 2.0 ** -150)])
def test_the_merge_cases_reach_a_subnormal_and_a_zero_split_factor(tag, lo, hi):
    """(1, 2, 128, 1024) with the q / k rows x 6 and x 8: for every row of head 0 the dominated split's exp(m_s - m) lies in the fp32
    subnormal range (x 6: m_s - m = -98.4 .. -100.6) or below half the smallest subnormal, i.e. it is 0 (x 8: -131 .. -134).  A kernel
    whose exponential flushes subnormals sees 0 in both."""
    shape = R.LA_SHAPES[4]
    _, smax = _sorted_case(shape, tag)
    gap = smax - smax.amax(-1, keepdim=True)
    dominated = gap[gap < 0]
    assert dominated.numel() == gap[..., 0].numel()
    print(f"[measured] {shape} {tag}: dominated split's m_s - m {dominated.max().item():.1f} .. {dominated.min().item():.1f}")
    assert dominated.max().item() < math.log(hi)
    if lo is not None:
        assert dominated.min().item() > math.log(lo)


@pytest.mark.parametrize("pre,post", [(0, -1), (1, 1)])
@pytest.mark.parametrize("shape", [R.LA_SHAPES[0], R.LA_SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_flat_and_zero_tokens_normalise_to_zero(shape, pre, post):
    """LayerNorm sends a flat token to 0 (x - mean = 0, var = 0: rstd = eps^-1/2) and both norms send the all-zero token to 0
    (RMSNorm: 0 / max(0, 1e-12)).  Its q = Wq xn = 0, so the softmax over d is uniform, 1 / 32 -- not zero: the token's branch is
    post(T 1 * 32^-1.5 + bo), the row sums of T, and not post(bo).  The GPU test holds these tokens to the fp64 branch."""
    case = R.la_case(shape, "flat", pre, post)
    x, g1 = case.inp[0], case.inp[1]
    (o0, i0, t0), (o1, i1, t1) = R.la_flat_tokens(shape)
    assert bool((x[o0, :, i0, t0] == 0.75).all()) and bool((x[o1, :, i1, t1] == 0).all())
    xn = LX._norm(x.double(), g1.double(), pre, shape[2])
    assert bool((xn[o1, :, i1, t1] == 0).all())
    if pre == 0:
        assert bool((xn[o0, :, i0, t0] == 0).all())
    assert torch.isfinite(case.exact[o0, :, i0, t0]).all() and torch.isfinite(case.exact[o1, :, i1, t1]).all()


@pytest.mark.parametrize("shape", R.TA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_temporal_zero_pixel_has_no_branch(shape):
    """a pixel that is zero in every frame: xn = 0, so q = k = v = 0, the softmax is that of the bias alone and y - x = 0 exactly"""
    case = R.ta_case(shape, "flat", True)
    _, (b1, h1, w1) = R.ta_flat_pixels(shape)
    assert bool((case.inp[0][b1, :, :, h1, w1] == 0).all())
    assert bool((case.exact[b1, :, :, h1, w1] == 0).all()) and bool((case.emu[b1, :, :, h1, w1] == 0).all())
