"""-m gpu: the forward of the eight fused attention-block entries on hard inputs (tests/attn_blocks_hard_ref.py):
sdc_linattn_block_sel impl 0 / 1, sdc_linattn_block_f16, their GroupNorm-on-load forms, sdc_tattn_block, sdc_tattn_block_x3_sel impl
0 / 1 and sdc_tattn_block_f16.  Every call goes through the C ABI onto a NaN-filled y (and a NaN-filled scratch for LinearAttention),
with the _run helpers of the four block test files.

The fp32-pipe and bf16-split entries are held to the exact fp64 branch y - x by the rule of tests/test_gpu_grad_paths.py with the
training-block files' Y_GATE: max |err| / max |ref| < max(1e-5, 4 e32) + r_out, e32 being the same figure of an fp32 torch restatement
of the formula -- never another kernel -- and r_out what storing y = x + branch as fp32 costs on its own (R.out_rounding: half an ulp
of |y| over the branch scale, below 3e-7 everywhere but on `large`, where it is up to 2.4e-5 and no fp32 output can avoid it; it is
added once, not multiplied).  The fp16 entries are held to the two relative rules of tests/test_gpu_linattn_f16.py with the case's
own e_in (the fp64 emulation of the documented rounding points against the exact block, rms): kernel against emulation <= e_in / 3,
kernel against exact <= 2 e_in.  tests/test_host_attn_blocks_hard.py shows on the CPU that e32 and e_in are what the inputs cost."""
import pytest
import torch

import attn_blocks_hard_ref as R
import test_gpu_attn_f16 as TF
import test_gpu_attn_x3 as TX
import test_gpu_attn_x3_skew as TS
import test_gpu_linattn_f16 as LF
import test_gpu_linattn_x3 as LX
from safediffcon_amd import _lib
from safediffcon_amd.engine import Plan, pack_conv_weight
from oracle.detweights import det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Y_GATE = 1e-5         # tests/test_gpu_linattn_train.py, tests/test_gpu_tattn_train.py


def _gate(case):
    """_gate of tests/test_gpu_grad_paths.py on the formula's e32, plus the rounding of the fp32 output itself"""
    return max(Y_GATE, 4.0 * case.e32) + case.r_out


def _branch(y, x):
    return y.cpu().double() - x.double()


def _rms(t):
    return t.double().pow(2).mean().sqrt().item()


def _hold32(tag, what, y, x, case, note=""):
    """finite, and the gate against the exact fp64 branch; one [measured] line"""
    assert torch.isfinite(y).all(), (tag, what)
    err = R.rel(_branch(y, x), case.exact)
    print(f"[measured] {tag} {what}: err {err:.2e} | e32 {case.e32:.2e} | r_out {case.r_out:.2e} | gate {_gate(case):.2e}{note}")
    assert err < _gate(case), (tag, what, err, case.e32, case.r_out)
    return err


def _hold16(tag, what, y, x, case, note=""):
    assert torch.isfinite(y).all(), (tag, what)
    got = _branch(y, x)
    e_emu, e_x = _rms(got - case.emu) / _rms(case.exact), _rms(got - case.exact) / _rms(case.exact)          # as the fp16 files take them
    print(f"[measured] {tag} {what}: rms err vs fp64 emulation {e_emu:.2e} (gate e_in / 3 = {case.e_in / 3:.2e}), vs exact fp64 {e_x:.2e} "
          f"(gate 2 e_in) | e_in {case.e_in:.2e} | max |err| / max |ref| vs exact {R.rel(got, case.exact):.2e}{note}")
    assert e_emu <= case.e_in / 3, (tag, what, e_emu, case.e_in)
    assert e_x <= 2 * case.e_in, (tag, what, e_x, case.e_in)


def _hold16_token(tag, name, got, emu, exact, case):
    """one token (or pixel) of an fp16 entry on its own, where the rms over the tensor would dilute it: the two rules of _hold16 in
    the max measure of the branch scale.  The emulation's own distance from the exact block in that measure is e_in_max =
    max |emu - exact| / max |exact| over the tensor; the token's max |kernel - emu| stays within a third of it and its
    max |kernel - exact| within twice it."""
    assert torch.isfinite(got).all(), (tag, name)
    scale = case.exact.abs().max().item()
    e_emu, e_x = (got - emu).abs().max().item() / scale, (got - exact).abs().max().item() / scale
    print(f"[measured] {tag} f16 {name}: max |err| of the branch scale vs emulation {e_emu:.2e} (gate e_in_max / 3 = {case.e_in_max / 3:.2e}), "
          f"vs exact {e_x:.2e} (gate 2 e_in_max)")
    assert e_emu <= case.e_in_max / 3, (tag, name, e_emu, case.e_in_max)
    assert e_x <= 2 * case.e_in_max, (tag, name, e_x, case.e_in_max)


# ------------------------------------------------------------------ LinearAttention block
def _la_dev(case):
    x, g1, g2, wqkv, wo, bo = case.inp
    return x.to(DEV), LX._dev(g1, g2, wqkv, wo, bo, x.shape[1])


def _la_f16(case, pre, post):
    x, g1, g2, wqkv, wo, bo = case.inp
    pq, po, wpk = LF._dev_weights(wqkv, wo, x.shape[1])
    dev = [t.to(DEV) for t in (g1, bo, g2)]
    return lambda xd: LF._run(xd, dev[0], pq, po, wpk, dev[1], dev[2], pre, post)


def _la_note(c, case):
    return f" | max |k| {R.la_k(case.inp, c[2]).abs().max().item():.1f}"


def _la_tokens(c, y, x, case, what):
    """the flat and the zero token of a `flat` case on their own: finite, and inside the gate"""
    for name, (o, i, t) in zip(("flat token", "zero token"), R.la_flat_tokens(c[0])):
        got = _branch(y, x)[o, :, i, t]
        assert torch.isfinite(got).all()
        err = ((got - case.exact[o, :, i, t]).abs().max() / case.exact.abs().max()).item()
        print(f"[measured] {R.la_id(c)} {what} {name}: err {err:.2e} of the branch scale (the token's own |y - x| max "
              f"{case.exact[o, :, i, t].abs().max().item():.3f})")
        assert err < _gate(case), (name, err)


@pytest.mark.parametrize("c", R.LA_CASES, ids=R.la_id)
def test_linattn_block_fp32_and_split_on_hard_inputs(c):
    """sdc_linattn_block_sel impl 0 (la_blk_ctx / la_blk_mid / la_blk_out) and impl 1 (the bf16-split twins) against the exact fp64 block.
    On `flat` the flat token (LayerNorm: xn = 0 at rstd = eps^-1/2) and the zero token (both norms: xn = 0, q uniform over d) are held
    to the fp64 branch on their own as well; under pre_mode 1 that branch is post(T 1 * 32^-1.5 + bo) and the fp64 reference is the
    only statement of it."""
    shape, tag, pre, post = c
    case = R.la_case(*c)
    x_dev, d = _la_dev(case)
    for impl in (0, 1):
        y = LX._run(impl, x_dev, d, pre, post)
        _hold32(R.la_id(c), f"impl {impl}", y, case.inp[0], case, _la_note(c, case))
        if tag == "flat":
            _la_tokens(c, y, case.inp[0], case, f"impl {impl}")


@pytest.mark.parametrize("c", R.LA_CASES, ids=R.la_id)
def test_linattn_block_f16_on_hard_inputs(c):
    """sdc_linattn_block_f16: the integer exponent ceil(m log2e), p rounded to fp16, the exact power-of-two merge of the splits.  The
    absolute cap of tests/test_gpu_linattn_f16.py (3.6e-4) was measured on soft inputs and is not carried over: e_in / 3 gates."""
    shape, tag, pre, post = c
    case = R.la_case(*c)
    x_dev, _ = _la_dev(case)
    y = _la_f16(case, pre, post)(x_dev)
    _hold16(R.la_id(c), "f16", y, case.inp[0], case)
    if tag == "flat":
        got = _branch(y, case.inp[0])
        for name, (o, i, t) in zip(("flat token", "zero token"), R.la_flat_tokens(shape)):
            _hold16_token(R.la_id(c), name, got[o, :, i, t], case.emu[o, :, i, t], case.exact[o, :, i, t], case)


@pytest.mark.parametrize("shape", [R.LA_SHAPES[0], R.LA_SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_linattn_block_default_route_is_the_tested_one(shape):
    """sdc_linattn_block gives the bits of sdc_linattn_block_sel(impl = sdc_linattn_block_x3_ok(C, n)) -- impl 1 at both sizes -- on
    peak4: what the tests above hold is what the samplers run"""
    case = R.la_case(shape, "peak4", 0, -1)
    x_dev, d = _la_dev(case)
    impl = int(_lib.get_lib().sdc_linattn_block_x3_ok(shape[2], shape[3]))
    assert impl == 1
    y = LX._run_entry(x_dev, d, 0, -1)
    assert torch.isfinite(y).all()
    assert torch.equal(y, LX._run(impl, x_dev, d, 0, -1))
    assert not torch.equal(y, LX._run(0, x_dev, d, 0, -1))


def test_linattn_block_desc_repeats_and_is_batch_independent():
    """desc at (2, 1, 64, 1088) -- uneven splits, the second one dominated, the rescale skipped by head 0's wave from tile 1 on: two runs
    give the same bits, and sample 0 alone gives its bits inside the batch, for impl 0, impl 1 and the fp16 entry"""
    c = (R.LA_SHAPES[1], "desc", 0, -1)
    case = R.la_case(*c)
    x_dev, d = _la_dev(case)
    f16 = _la_f16(case, 0, -1)
    runs = {"impl 0": lambda xd: LX._run(0, xd, d, 0, -1), "impl 1": lambda xd: LX._run(1, xd, d, 0, -1), "f16": f16}
    for what, run in runs.items():
        y = run(x_dev)
        assert torch.isfinite(y).all(), what
        assert torch.equal(run(x_dev), y), what
        assert torch.equal(run(x_dev[:1].contiguous())[0], y[0]), what


@pytest.mark.parametrize("which", ["impl 0", "impl 1", "f16"])
def test_linattn_block_with_groupnorm_on_load_on_peak4(which):
    """peak4 weights at (C, F, (H, W)) = (64, 3, (16, 16)): sdc_linattn_block_gn_sel impl 0 / 1 and sdc_linattn_block_gn_f16 ==
    sdc_gn_stats + sdc_gn_apply followed by the plain entry, bit for bit (the pattern of test_linattn_x3_block_with_groupnorm_on_load),
    and the result meets the gate of the plain entry with h = SiLU(GN(x)) + r, as the unfused chain left it in fp32, as the block's
    input"""
    B, G, Cc, F_, H, W = 2, 8, 64, 3, 16, 16
    n = H * W
    _, g1, g2, wqkv, wo, bo = R.la_inputs((B, F_, Cc, n), "peak4", 0, -1)
    x = det_tensor((B, Cc, F_, H, W), 501).to(DEV)
    r = det_tensor((B, Cc, F_, H, W), 502).to(DEV)
    gam, bet = (1 + 0.2 * det_tensor((Cc,), 503)).to(DEV), (0.1 * det_tensor((Cc,), 504)).to(DEV)
    uq, uo = wqkv.view(384, Cc, 1, 1).to(DEV), wo.view(Cc, 128, 1, 1).to(DEV)
    g_pre, bo_dev = g1.to(DEV), bo.to(DEV)
    f16 = which == "f16"
    outs, h = [], None
    for fused in (True, False):
        plan = Plan(DEV, linattn_f16=True) if f16 else Plan(DEV)
        pq, po = plan.conv_weight(uq), plan.conv_weight(uo)
        xx = x.clone()
        strides = (Cc * F_ * n, F_ * n, n)
        kw = dict(w16=(uq, uo)) if f16 else {}
        if fused:
            st = plan.gn_stats_deferred(xx, G)
            y = plan.linattn_block(xx, g_pre, pq, po, bo_dev, None, B, F_, n, strides, 0, -1, gn=(st, gam, bet, G, r), **kw)
        else:
            hh = plan.gn_silu(xx, gam, bet, G, residual=r)
            y = plan.linattn_block(hh, g_pre, pq, po, bo_dev, None, B, F_, n, strides, 0, -1, **kw)
        name = ("sdc_linattn_block_gn" if fused else "sdc_linattn_block") + ("_f16" if f16 else "")
        assert [fn.__name__ for fn, _ in plan.calls][-1] == name
        if not f16:
            assert LX._forced(plan, int(which[-1])) == 1
        y.fill_(float("nan"))
        plan.run(LX._stream())
        torch.cuda.synchronize()
        assert torch.isfinite(y).all()
        outs.append(y.clone())
        if not fused:
            h = hh.clone()
    assert torch.equal(outs[0], outs[1])
    h_cpu = h.cpu().reshape(B, Cc, F_, n)
    case = R.la_refs((h_cpu, g1, g2, wqkv, wo, bo), 0, -1)
    y = outs[0].reshape(B, Cc, F_, n)
    tag = f"GroupNorm-on-load {B}x{F_}x{Cc}x{n}-peak4"
    if f16:
        _hold16(tag, which, y, h_cpu, case)
    else:
        _hold32(tag, which, y, h_cpu, case, f" | max |k| {R.la_k(case.inp, 0).abs().max().item():.1f}")


# ------------------------------------------------------------------ temporal-attention block
def _ta_dev(case, tables):
    x, g, wqkv, wo, freqs, relw = case.inp
    rot, bias = TX._tables(freqs, relw) if tables else (None, None)
    return x.to(DEV), g.to(DEV), rot, bias


def _ta_fp32_weights(case):
    wqkv, wo = case.inp[2], case.inp[3]
    return pack_conv_weight(wqkv.view(384, 64, 1)).to(DEV), pack_conv_weight(wo.view(64, 128, 1)).to(DEV)


def _ta_note(case, tables):
    return f" | max |score| {R.ta_max_score(case.inp, tables):.1f}"


def _ta_pixels(c, y, x, case, what):
    (b0, f0, h0, w0), (b1, h1, w1) = R.ta_flat_pixels(c[0])
    got = _branch(y, x)
    for name, g, e in (("flat token", got[b0, :, f0, h0, w0], case.exact[b0, :, f0, h0, w0]),
                       ("zero pixel", got[b1, :, :, h1, w1], case.exact[b1, :, :, h1, w1])):
        assert torch.isfinite(g).all()
        err = ((g - e).abs().max() / case.exact.abs().max()).item()
        print(f"[measured] {R.ta_id(c)} {what} {name}: err {err:.2e} of the branch scale")
        assert err < _gate(case), (name, err)


@pytest.mark.parametrize("c", R.TA_CASES, ids=R.ta_id)
def test_temporal_block_fp32_and_split_on_hard_inputs(c):
    """sdc_tattn_block and sdc_tattn_block_x3_sel impl 0 against the exact fp64 block: each has its own LayerNorm, scale in the exponent
    and bias add"""
    shape, tag, tables = c
    case = R.ta_case(*c)
    x_dev, g_dev, rot, bias = _ta_dev(case, tables)
    wq4, wo4 = _ta_fp32_weights(case)
    wpk = TX._pack_dev(case.inp[2], case.inp[3])
    note = _ta_note(case, tables)
    for what, y in (("fp32", TX._run_fp32(x_dev, g_dev, wq4, wo4, rot, bias)), ("split impl 0", TS._run(0, x_dev, g_dev, wpk, rot, bias))):
        _hold32(R.ta_id(c), what, y, case.inp[0], case, note)
        if tag == "flat":
            _ta_pixels(c, y, case.inp[0], case, what)


@pytest.mark.parametrize("c", [c for c in R.TA_CASES if c[2]], ids=R.ta_id)
def test_temporal_block_f16_on_hard_inputs(c):
    """sdc_tattn_block_f16 with the case's own e_in; the absolute cap of tests/test_gpu_attn_f16.py (3e-4) was measured on soft inputs
    and is not carried over"""
    shape, tag, tables = c
    case = R.ta_case(*c)
    x_dev, g_dev, rot, bias = _ta_dev(case, True)
    y = TF._run(x_dev, g_dev, TF._pack_dev(case.inp[2], case.inp[3]), rot, bias)
    _hold16(R.ta_id(c), "f16", y, case.inp[0], case)
    if tag == "flat":
        (b0, f0, h0, w0), (b1, h1, w1) = R.ta_flat_pixels(shape)
        got = _branch(y, case.inp[0])
        _hold16_token(R.ta_id(c), "flat token", got[b0, :, f0, h0, w0], case.emu[b0, :, f0, h0, w0], case.exact[b0, :, f0, h0, w0], case)
        _hold16_token(R.ta_id(c), "zero pixel", got[b1, :, :, h1, w1], case.emu[b1, :, :, h1, w1], case.exact[b1, :, :, h1, w1], case)


@pytest.mark.parametrize("tag", ["peak4", "bias8+peak4", "flat"])
@pytest.mark.parametrize("shape", R.TA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_temporal_block_skewed_form_gives_the_unskewed_bits(shape, tag):
    """sdc_tattn_block_x3_sel impl 1 == impl 0, bit for bit"""
    case = R.ta_case(shape, tag, True)
    x_dev, g_dev, rot, bias = _ta_dev(case, True)
    wpk = TX._pack_dev(case.inp[2], case.inp[3])
    y0, y1 = TS._run(0, x_dev, g_dev, wpk, rot, bias), TS._run(1, x_dev, g_dev, wpk, rot, bias)
    assert torch.isfinite(y0).all() and torch.equal(y1, y0)


@pytest.mark.parametrize("shape", R.TA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_temporal_block_default_route_is_the_tested_one(shape):
    """sdc_tattn_block_x3 gives the bits of sdc_tattn_block_x3_sel(impl = sdc_tattn_block_x3_impl(C, frames, pixels)) on peak4: the
    entry computes what the tests above hold.  It cannot tell WHICH impl the entry took -- impl 0 and impl 1 give the same bits by
    construction (the test above), so unlike the LinearAttention route test there is no `not torch.equal` counterpart; the table
    itself is read through sdc_tattn_block_x3_impl."""
    case = R.ta_case(shape, "peak4", True)
    x_dev, g_dev, rot, bias = _ta_dev(case, True)
    wpk = TX._pack_dev(case.inp[2], case.inp[3])
    impl = int(_lib.get_lib().sdc_tattn_block_x3_impl(TX.Cc, TX.Fr, shape[1] * shape[2]))
    assert impl in (0, 1)
    y = TX._run(x_dev, g_dev, wpk, rot, bias)
    assert torch.isfinite(y).all() and torch.equal(y, TS._run(impl, x_dev, g_dev, wpk, rot, bias))


def test_temporal_block_peak8_repeats_and_is_batch_independent():
    """peak8 at (2, 4, 8): two runs give the same bits and sample 0 alone gives its bits inside the batch, for every entry"""
    case = R.ta_case(R.TA_SHAPES[0], "peak8", True)
    x_dev, g_dev, rot, bias = _ta_dev(case, True)
    wq4, wo4 = _ta_fp32_weights(case)
    wpk, wpk16 = TX._pack_dev(case.inp[2], case.inp[3]), TF._pack_dev(case.inp[2], case.inp[3])
    runs = {"fp32": lambda xd: TX._run_fp32(xd, g_dev, wq4, wo4, rot, bias), "split impl 0": lambda xd: TS._run(0, xd, g_dev, wpk, rot, bias),
            "split impl 1": lambda xd: TS._run(1, xd, g_dev, wpk, rot, bias), "f16": lambda xd: TF._run(xd, g_dev, wpk16, rot, bias)}
    for what, run in runs.items():
        y = run(x_dev)
        assert torch.isfinite(y).all(), what
        assert torch.equal(run(x_dev), y), what
        assert torch.equal(run(x_dev[:1].contiguous())[0], y[0]), what
