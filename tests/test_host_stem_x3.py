"""CPU-side checks of net.stem_split (include/sdc.h, sdc_conv_stem_x3): the three bf16 planes Wb[piece][kd][s][co][8 h + ci] of the
7-tap stem conv weights sum to the fp32 weight bit for bit; the three-way split x = bf16 h + m + l is exact over the fp32 range the
nets see; the six-term product stays within 2^-24 |a b| of the exact one; the coverage predicate is sdc_conv_stem_f16_ok's; the plan's
switch."""
import ctypes as C

import pytest
import torch

from safediffcon_amd import _lib
from safediffcon_amd.engine import Plan, conv_desc, pack_conv_weight, pack_stem_f16, pack_stem_x3, split3_bf16

SDC_EINVAL, SDC_ENULL = -1, -4


def _wide_range(n, seed, lo=-100, hi=100):
    """n fp32 values with random signs and significands and exponents uniform in [lo, hi)"""
    g = torch.Generator().manual_seed(seed)
    m = 1.0 + torch.rand(n, generator=g, dtype=torch.float64)
    e = torch.randint(lo, hi, (n,), generator=g).double()
    s = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return (s * m * torch.pow(torch.tensor(2.0, dtype=torch.float64), e)).float()


@pytest.mark.parametrize("shape", [(64, 7, 7, 7, 7), (64, 3, 1, 7, 7), (128, 8, 1, 1, 7), (64, 1, 7, 7, 7)])
def test_pack_stem_x3_planes_sum_to_the_weight_bit_for_bit(shape):
    g = torch.Generator().manual_seed(sum(shape))
    w = torch.randn(*shape, generator=g) * 3.0
    co, ci, kD, kH, kW = shape
    ns = (kH * 7 + 1) // 2
    got = pack_stem_x3(w).view(torch.bfloat16)
    assert got.numel() * 2 == _lib.get_lib().sdc_pack_stem_x3_bytes(co, ci, kD, kH, kW) == 3 * _lib.get_lib().sdc_pack_stem_f16_bytes(co, ci, kD, kH, kW)
    planes = got.reshape(3, kD, ns, co, 2, 8)
    # each plane has the layout of pack_stem_f16: compared with the fp32 weight laid out the same way
    total = planes[0].double() + planes[1].double() + planes[2].double()            # (exact in fp64: 3 x 8 bits)
    lay = torch.zeros(kD, ns, co, 2, 8, dtype=torch.float64)
    for kd in range(kD):
        for t in range(kH * 7):
            lay[kd, t // 2, :, t % 2, :ci] = w[:, :, kd, t // 7, t % 7].double()
    assert torch.equal(total, lay)
    assert torch.equal(total.float().view(torch.int32), lay.float().view(torch.int32))
    # the zero pad channels and the tap past the end: exact zeros in all three planes (bit pattern 0, not -0)
    bits = planes.view(torch.int16)
    assert (bits[..., ci:] == 0).all()
    assert (bits[:, :, -1, :, 1, :] == 0).all()
    # the first plane is the bf16 rounding (RNE) of the weight, where pack_stem_f16 holds the fp16 one
    assert torch.equal(planes[0].float(), lay.float().bfloat16().float())
    assert planes[0].numel() == pack_stem_f16(w).view(torch.float16).numel()
    if kD == 1:
        w_low = w.reshape(co, ci, kW) if kH == 1 else w.reshape(co, ci, kH, kW)
        assert torch.equal(pack_stem_x3(w_low).view(torch.int32), pack_stem_x3(w).view(torch.int32))
    # the plan packs the same buffer
    assert torch.equal(Plan("cpu", precision=4, stem_split=True).stem_weight(w, pack_stem_x3).view(torch.int32), pack_stem_x3(w).view(torch.int32))


def test_pack_stem_x3_rejects_other_weights():
    lib = _lib.get_lib()
    for shape in ((64, 12, 1, 1, 7), (64, 7, 3, 3, 3), (64, 7, 7, 1, 7), (64, 7, 1, 7, 5)):
        with pytest.raises(ValueError):
            pack_stem_x3(torch.zeros(*shape))
        assert lib.sdc_pack_stem_x3_bytes(*shape) == 0
        assert lib.sdc_pack_stem_x3(256, 256, *shape, None) == SDC_EINVAL      # (the pointers are never dereferenced)
    assert lib.sdc_pack_stem_x3(None, 256, 64, 7, 7, 7, 7, None) == SDC_ENULL
    assert lib.sdc_pack_stem_x3(256, None, 64, 7, 7, 7, 7, None) == SDC_ENULL


def test_three_way_split_is_exact_from_2e_minus_100_to_2e100():
    x = torch.cat([_wide_range(1 << 20, 1), torch.randn(1 << 18, generator=torch.Generator().manual_seed(2)),
                   torch.tensor([0.0, -0.0, 2.0 ** -100, -(2.0 ** 100), 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -8 + 2.0 ** -16])])
    h, m, l = split3_bf16(x)
    s = h.double() + m.double() + l.double()
    assert torch.equal(s, x.double())
    # the pieces shrink by at least 2^-8 each (RNE to 8 significant bits: half an ulp of the piece before)
    assert (m.double().abs() <= h.double().abs() * 2.0 ** -8).all() and (l.double().abs() <= h.double().abs() * 2.0 ** -16).all()


def test_six_term_product_is_within_half_an_ulp_of_the_exact_one():
    a, b = _wide_range(1 << 20, 3, -40, 40), _wide_range(1 << 20, 4, -40, 40)
    (a1, a2, a3), (b1, b2, b3) = ([p.double() for p in split3_bf16(v)] for v in (a, b))
    # every bf16 x bf16 product is exact in fp32 (16 significant bits); summed here in fp64, smallest first, as the kernel's order
    six = a3 * b1 + a2 * b2 + a1 * b3 + a2 * b1 + a1 * b2 + a1 * b1
    exact = a.double() * b.double()
    rel = ((six - exact).abs() / exact.abs()).max().item()
    print(f"[measured] six-term product: max dropped part {rel:.3e} of |a b| (2^-24 = {2.0 ** -24:.3e})")
    assert rel <= 2.0 ** -24
    for p in (a3 * b1, a2 * b2, a1 * b3, a2 * b1, a1 * b2, a1 * b1):
        assert torch.equal(p.float().double(), p)


def _desc(B=2, cin=7, cin1=0, cout=64, size=(4, 8, 32), k=(7, 7, 7), stride=(1, 1, 1), pad=None, up=(1, 1, 1)):
    pad = tuple(kk // 2 for kk in k) if pad is None else pad
    x = torch.empty(B, cin, *size)
    x1 = torch.empty(B, cin1, *size) if cin1 else None
    o = tuple(((i * u + 2 * p - kk) // s + 1) for i, u, kk, s, p in zip(size, up, k, stride, pad))
    return conv_desc(x, x1, torch.empty(B, cout, *o), None, cout, k, stride, pad, up, 0, 0)


CASES = [dict(k=(7, 7, 7), size=(4, 8, 32)), dict(k=(1, 7, 7), size=(1, 16, 128), cin=3), dict(k=(1, 1, 7), size=(1, 1, 64), cin=1),
         dict(k=(7, 7, 7), size=(32, 32, 32)), dict(k=(7, 7, 7), size=(3, 1, 16), cin=2), dict(k=(1, 7, 7), size=(1, 5, 128), cin=2),
         dict(cin=12), dict(cout=8), dict(stride=(1, 1, 2), size=(4, 8, 64)), dict(pad=(3, 3, 2), size=(4, 8, 34)), dict(cin=4, cin1=3),
         dict(up=(1, 1, 2), size=(4, 8, 16)), dict(size=(4, 8, 24)), dict(k=(3, 3, 3)), dict(k=(7, 1, 7)), dict(cout=96), dict(cin=8),
         dict(cin=9), dict(size=(4, 8, 256))]


def test_stem_x3_ok_is_stem_f16_ok_less_the_kd1_stems():
    # (the kD = 1 stems left coverage: the C2 stem measured no faster than today's kernel)
    lib = _lib.get_lib()
    assert lib.sdc_conv_stem_x3_ok(None) == 0
    seen = set()
    for B in (1, 64):
        for kw in CASES:
            d = _desc(B=B, **kw)
            ok = lib.sdc_conv_stem_x3_ok(C.byref(d))
            assert ok == (lib.sdc_conv_stem_f16_ok(C.byref(d)) and d.kD == 7), kw
            seen.add((ok, d.kD))
    assert seen == {(0, 1), (0, 7), (1, 7), (0, 3)}
    # precision is unread; a strided (frame-major) input is covered, rows that are not dense are not
    d = _desc()
    for prec in (0, 4, 6, 99):
        d.precision = prec
        assert lib.sdc_conv_stem_x3_ok(C.byref(d)) == 1
    x = torch.empty(2, 4, 7, 8, 32).permute(0, 2, 1, 3, 4)
    d = conv_desc(x, None, torch.empty(2, 64, 4, 8, 32), None, 64, (7, 7, 7), (1, 1, 1), (3, 3, 3), (1, 1, 1), 0, 0)
    assert lib.sdc_conv_stem_x3_ok(C.byref(d)) == 1
    d.x0s[4] = 2
    assert lib.sdc_conv_stem_x3_ok(C.byref(d)) == 0
    d.x0s[4], d.ys[4] = 1, 2
    assert lib.sdc_conv_stem_x3_ok(C.byref(d)) == 0


def test_stem_x3_entry_rejects_before_any_launch():
    lib = _lib.get_lib()
    d = _desc()
    assert lib.sdc_conv_stem_x3(None, 256, 256, 0, 256, None) == SDC_ENULL
    assert lib.sdc_conv_stem_x3(C.byref(d), 0, 256, 0, 256, None) == SDC_ENULL
    assert lib.sdc_conv_stem_x3(C.byref(d), 256, 0, 0, 256, None) == SDC_ENULL
    assert lib.sdc_conv_stem_x3(C.byref(d), 256, 256, 0, 0, None) == SDC_ENULL
    assert "null" in _lib.last_error()
    for kw in (dict(cin=12), dict(cout=8), dict(k=(3, 3, 3)), dict(size=(4, 8, 24))):
        assert lib.sdc_conv_stem_x3(C.byref(_desc(**kw)), 256, 256, 0, 256, None) == SDC_EINVAL, kw
        assert "not covered" in _lib.last_error()
    # the kernel entry accepts the kD = 1 stems that sdc_conv_stem_x3_ok no longer routes (here: past the coverage check, to the alignment one)
    d = _desc(k=(1, 7, 7), size=(1, 16, 128), cin=3)
    assert lib.sdc_conv_stem_x3_ok(C.byref(d)) == 0 and lib.sdc_conv_stem_x3(C.byref(d), 256, 8, 0, 256, None) == -2


def test_plan_switch_needs_precision_4_and_yields_to_stem_f16():
    assert Plan("cpu").stem_split is False and Plan("cpu", precision=4).stem_split is False      # a Plan built directly: today's routes
    for prec, on in ((0, False), (2, False), (3, False), (4, True), (5, True), (6, True), (7, True)):
        assert Plan("cpu", precision=prec, stem_split=True).stem_split is on
    both = Plan("cpu", precision=4, stem_f16=True, stem_split=True)
    assert both.stem_f16 is True and both.stem_split is False
    # every existing weight layout is untouched by the switch
    g = torch.Generator().manual_seed(3)
    on, off = Plan("cpu", precision=4, stem_split=True), Plan("cpu", precision=4)
    for shape in ((64, 12, 7), (8, 7, 7, 7, 7), (64, 7, 7, 7, 7), (40, 24, 3, 3), (16, 8, 3, 3, 3), (16, 8, 1)):
        w = torch.randn(*shape, generator=g)
        assert torch.equal(on.conv_weight(w), off.conv_weight(w))
        assert torch.equal(on.conv_weight(w), pack_conv_weight(w, precision=4))
