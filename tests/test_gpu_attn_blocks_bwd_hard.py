"""-m gpu: the three backward entries of the fused attention blocks on hard inputs (tests/attn_blocks_bwd_hard_ref.py, DESIGN.md section
30): sdc_linattn_block_bwd, sdc_linattn_block_post_bwd (csrc/sdc_lablock_bwd.hip) and sdc_tattn_block_bwd (csrc/sdc_tablock_bwd.hip).
Each recomputes both softmaxes and the norms from x in code of its own; the forward of the node (sdc_linattn_block_sel impl 0,
sdc_tattn_block) is held by tests/test_gpu_attn_blocks_hard.py and is not run here.  Every call goes through the C ABI with the
_run_abi(..., want_y=False) of the three training-block files.

Every output is finite and held to the fp64 autograd reference by the rule of tests/test_gpu_grad_paths.py: max |err| / max |ref| <
max(2e-5, 4 e32), per output with that output's own e32 -- the same figure of the fp32 torch restatement of the reference, never of a
kernel.  On `flat` / `tiny` (and temporal `flat`) a few degenerate tokens own max |dx| by a factor 4e2 - 7e13, so dx is judged twice by
the same rule: over the tensor with those tokens removed from both the error and the scale, and on each of those tokens alone, each
time against the e32 of that very set.  The parameter gradients are sums over tokens and are judged whole.
tests/test_host_attn_blocks_bwd_hard.py shows on the CPU what the inputs are and that every e32 is below 1e-4 (1e-3 for `offset` and
temporal `peak8`)."""
import pytest
import torch

import attn_blocks_bwd_hard_ref as B
import attn_blocks_hard_ref as R
import test_gpu_linattn_post_train as LP
import test_gpu_linattn_train as LT
import test_gpu_tattn_train as TT
from safediffcon_amd import _lib
from test_gpu_grad import DEV, _rel
from test_gpu_grad_paths import _finite, _gate

pytestmark = pytest.mark.gpu
G_GATE = 2e-5          # the three training-block files
LA_NAMES = ("dx", "dg_pre", "dwqkv", "dwo", "dbo", "dg_post")
TA_NAMES = ("dx", "dg", "dwqkv", "dwo", "dbias")


def _hold(entry, name, names, got, case, note=""):
    """got: the outputs behind y.  Finite; one [measured] line; then every gate"""
    assert _finite(*got), (entry, name)
    assert [g is None for g in got] == [r is None for r in case.ref], (entry, name)
    checks = []                                                          # (what, err, e32)
    dx = got[0].cpu()
    if case.deg:
        checks.append((f"dx without its {len(case.deg)} degenerate tokens", B.rel_rest(dx, case.ref[0], case.deg), case.e32_rest))
        for j, idx in enumerate(case.deg):
            checks.append((f"dx of degenerate token {j}", B.rel_token(dx, case.ref[0], idx), case.e32_tok[j]))
    else:
        checks.append(("dx", _rel(dx, case.ref[0]), case.e32[0]))
    for n, g, r, e in zip(names[1:], got[1:], case.ref[1:], case.e32[1:]):
        if r is not None:
            checks.append((n, _rel(g, r), e))
    tok = [c for c in checks if c[0].startswith("dx of degenerate")]
    shown = [c for c in checks if not c[0].startswith("dx of degenerate")]
    line = " ".join(f"{w} {err:.2e} (e32 {e:.2e})" for w, err, e in shown)
    if tok:
        worst = max(tok, key=lambda c: c[1] / _gate(G_GATE, c[2]))
        line += f" | the {len(tok)} degenerate tokens alone: worst {worst[1]:.2e} (e32 {worst[2]:.2e})"
    close = max(checks, key=lambda c: c[1] / _gate(G_GATE, c[2]))
    print(f"[measured] {entry} {name}: {line} | closest to its gate: {close[0]} at {close[1] / _gate(G_GATE, close[2]):.2f} of it{note}")
    for what, err, e in checks:
        assert err < _gate(G_GATE, e), (entry, name, what, err, e)


def _la_note(c):
    shape, tag, pre, post = c
    return f" | max |k| {R.la_k(B.la_inputs(shape, tag, pre, post), pre).abs().max().item():.1f}"


# ------------------------------------------------------------------ sdc_linattn_block_bwd
@pytest.mark.parametrize("c", B.LA_BWD_CASES, ids=R.la_id)
def test_linattn_block_bwd_on_hard_inputs(c):
    """lab_mid1_kernel's merge of the splits (a normal, a subnormal and a zero factor), lab_dx's recomputed token softmax at |k| up to
    190 with dK = p (dp - delta) on near one-hot rows, softmax_d and dQ at peaked q, ln_tile at var = 0, at x + 50 and eps-dominated"""
    case = B.la_bwd_case(*c)
    _hold("sdc_linattn_block_bwd", R.la_id(c), LA_NAMES, LT._run_abi(case.inp, want_y=False)[1:], case, _la_note(c))


def test_linattn_block_bwd_desc_repeats_and_is_batch_independent():
    """desc at (2, 1, 64, 1088), uneven splits with the second one dominated: two runs into one NaN-filled workspace give the same
    bits, and sample 0 alone gives its bits inside the batch"""
    shape = R.LA_SHAPES[1]
    inp = B.la_bwd_inputs(shape, "desc")
    lib = _lib.get_lib()
    work = torch.full((int(lib.sdc_linattn_block_bwd_bytes(shape[0], shape[1], shape[2], shape[3])) // 4,), float("nan"), device=DEV)
    first = LT._run_abi(inp, work, want_y=False)[1:]
    second = LT._run_abi(inp, work, want_y=False)[1:]
    assert _finite(*first) and all(torch.equal(a, b) for a, b in zip(first, second))
    alone = tuple(t[:1].contiguous() if i in (0, 5) else t for i, t in enumerate(inp))
    work1 = torch.full((int(lib.sdc_linattn_block_bwd_bytes(1, shape[1], shape[2], shape[3])) // 4,), float("nan"), device=DEV)
    assert torch.equal(LT._run_abi(alone, work1, want_y=False)[1], first[0][:1])


# ------------------------------------------------------------------ sdc_linattn_block_post_bwd
@pytest.mark.parametrize("c", B.LA_POST_CASES, ids=R.la_id)
def test_linattn_block_post_bwd_on_hard_inputs(c):
    """the same kernels in their post-norm form plus post_bwd_tile (a small z over more than one split, z's LayerNorm and RMSNorm at a
    large rstd) and mode 1 of ln_tile: its clamp at ||x|| = 0 and, on `tiny`, its `live` flag at 0 < ||x|| <= 1e-12.  dx holds NaN
    before the call"""
    shape, tag, pre, post = c
    case = B.la_post_case(*c)
    _hold("sdc_linattn_block_post_bwd", R.la_id(c), LA_NAMES, LP._run_abi(case.inp, (pre, post), want_y=False, dirty=True)[1:], case,
          _la_note(c))


def test_linattn_block_post_bwd_desc_repeats_and_is_batch_independent():
    """desc at (2, 1, 64, 1088) under (1, 1): two runs into a NaN-filled workspace and a NaN-filled dx give the same bits, and sample 0
    alone gives its bits inside the batch"""
    shape, modes = R.LA_SHAPES[1], (1, 1)
    inp = B.la_post_inputs(shape, "desc", *modes)
    lib = _lib.get_lib()
    work = torch.full((int(lib.sdc_linattn_block_post_bwd_bytes(shape[0], shape[1], shape[2], shape[3])) // 4,), float("nan"), device=DEV)
    first = LP._run_abi(inp, modes, work, want_y=False, dirty=True)[1:]
    work.fill_(float("nan"))
    second = LP._run_abi(inp, modes, work, want_y=False, dirty=True)[1:]
    assert _finite(*first) and all(torch.equal(a, b) for a, b in zip(first, second))
    alone = tuple(t[:1].contiguous() if i in (0, 6) else t for i, t in enumerate(inp))
    work1 = torch.full((int(lib.sdc_linattn_block_post_bwd_bytes(1, shape[1], shape[2], shape[3])) // 4,), float("nan"), device=DEV)
    assert torch.equal(LP._run_abi(alone, modes, work1, want_y=False, dirty=True)[1], first[0][:1])


# ------------------------------------------------------------------ sdc_tattn_block_bwd
@pytest.mark.parametrize("c", B.TA_CASES, ids=R.ta_id)
def test_temporal_block_bwd_on_hard_inputs(c):
    """ta_block_bwd_kernel's two orientations of P with the row statistics handed over through LDS, at scores of 500 - 2100 and with
    a large bias; D = rowsum(P dP) and dbias += dS on near one-hot rows; the LayerNorm backward at var = 0, x + 50 and eps-dominated"""
    case = B.ta_case(*c)
    note = f" | max |score| {R.ta_max_score(R.ta_inputs(c[0], c[1]), c[2]):.1f}"
    _hold("sdc_tattn_block_bwd", R.ta_id(c), TA_NAMES, TT._run_abi(case.inp, want_y=False)[1:], case, note)


def test_temporal_block_bwd_peak8_repeats_and_is_batch_independent():
    """peak8 at (2, 4, 8): two runs into one NaN-filled workspace give the same bits, and sample 0 alone gives its bits inside the batch"""
    shape = R.TA_SHAPES[0]
    inp, _ = B.ta_inputs(shape, "peak8", True)
    lib = _lib.get_lib()
    hw = shape[1] * shape[2]
    work = torch.full((int(lib.sdc_tattn_block_bwd_bytes(shape[0], hw)) // 4,), float("nan"), device=DEV)
    first = TT._run_abi(inp, work, want_y=False)[1:]
    second = TT._run_abi(inp, work, want_y=False)[1:]
    assert _finite(*first) and all(torch.equal(a, b) for a, b in zip(first, second))
    alone = tuple(t[:1].contiguous() if i in (0, 6) else t for i, t in enumerate(inp))
    work1 = torch.full((int(lib.sdc_tattn_block_bwd_bytes(1, hw)) // 4,), float("nan"), device=DEV)
    assert torch.equal(TT._run_abi(alone, work1, want_y=False)[1], first[0][:1])
