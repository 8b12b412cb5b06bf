"""CPU-side checks of net.stem_f16 (include/sdc.h, sdc_conv_stem_f16): the fp16 buffer of the 7-tap stem convs
Wh[kd][s][co][8 h + ci] = w[co][ci][kd][tap = kh * 7 + kw = 2 s + h] (RNE, Cin zero-padded to 8, NS = ceil(7 kH / 2) steps), the
descriptor-only coverage predicate, the argument errors of the entry points and the plan's switch."""
import ctypes as C

import pytest
import torch

from safediffcon_amd import _lib
from safediffcon_amd.engine import Plan, conv_desc, pack_conv_weight, pack_stem_f16

SDC_EINVAL, SDC_ENULL = -1, -4


def _layout_ref(w):
    """the documented layout written out with explicit loops over (kd, s, h, ci)"""
    co, ci, kD, kH, kW = w.shape
    ns = (kH * 7 + 1) // 2
    out = torch.zeros(kD, ns, co, 16, dtype=torch.float16)
    for kd in range(kD):
        for s in range(ns):
            for h in range(2):
                t = 2 * s + h
                if t >= kH * 7:
                    continue
                for c in range(ci):
                    out[kd, s, :, 8 * h + c] = w[:, c, kd, t // 7, t % 7].half()
    return out


@pytest.mark.parametrize("shape", [(64, 7, 7, 7, 7), (64, 3, 1, 7, 7), (128, 8, 1, 1, 7), (64, 1, 7, 7, 7)])
def test_pack_stem_f16_is_the_documented_layout(shape):
    g = torch.Generator().manual_seed(sum(shape))
    w = torch.randn(*shape, generator=g) * 3.0
    co, ci, kD, kH, kW = shape
    ref = _layout_ref(w)
    got = pack_stem_f16(w).view(torch.float16)
    assert got.numel() * 2 == _lib.get_lib().sdc_pack_stem_f16_bytes(co, ci, kD, kH, kW)
    assert torch.equal(got, ref.reshape(-1))
    got = got.reshape(ref.shape)
    # padded channels and the tap past the end: exact zeros (bit pattern 0, not -0)
    bits = got.view(torch.int16).reshape(kD, -1, co, 2, 8)
    assert (bits[:, :, :, :, ci:] == 0).all()
    assert (bits[:, -1, :, 1, :] == 0).all()
    assert got.abs().sum() > 0
    # the lower-rank weights of Conv1d / Conv2d pack as their 5-D form
    if kD == 1:
        w_low = w.reshape(co, ci, kW) if kH == 1 else w.reshape(co, ci, kH, kW)
        assert torch.equal(pack_stem_f16(w_low), pack_stem_f16(w))
    # the plan packs the same buffer
    assert torch.equal(Plan("cpu", precision=4, stem_f16=True).stem_weight(w).view(torch.float16), ref.reshape(-1))


def test_pack_stem_f16_rejects_other_weights():
    lib = _lib.get_lib()
    for shape in ((64, 12, 1, 1, 7), (64, 7, 3, 3, 3), (64, 7, 7, 1, 7), (64, 7, 1, 7, 5)):
        with pytest.raises(ValueError):
            pack_stem_f16(torch.zeros(*shape))
        assert lib.sdc_pack_stem_f16_bytes(*shape) == 0
        assert lib.sdc_pack_stem_f16(256, 256, *shape, None) == SDC_EINVAL      # (the pointers are never dereferenced)
    assert lib.sdc_pack_stem_f16(None, 256, 64, 7, 7, 7, 7, None) == SDC_ENULL
    assert lib.sdc_pack_stem_f16(256, None, 64, 7, 7, 7, 7, None) == SDC_ENULL


def test_stem_f16_rounding_is_nearest_even():
    # halfway cases between two fp16 neighbours round to the even one (RNE); round-toward-zero would truncate them all
    one = 1.0 + 2.0 ** -11                           # halfway between 1 and 1 + 2^-10: even -> 1
    three = 1.0 + 3 * 2.0 ** -11                     # halfway between 1 + 2^-10 and 1 + 2^-9: even -> 1 + 2^-9
    w = torch.tensor([one, three, -three], dtype=torch.float32).reshape(1, 3, 1).repeat(64, 1, 7)
    h = pack_stem_f16(w).view(torch.float16).float().reshape(4, 64, 16)
    assert h[0, 0, 0].item() == 1.0 and h[0, 0, 1].item() == 1.0 + 2.0 ** -9 and h[0, 0, 2].item() == -(1.0 + 2.0 ** -9)
    assert h[2, 5, 8].item() == 1.0 and h[2, 5, 9].item() == 1.0 + 2.0 ** -9 and h[2, 5, 10].item() == -(1.0 + 2.0 ** -9)


def _desc(B=2, cin=7, cin1=0, cout=64, size=(4, 8, 32), k=(7, 7, 7), stride=(1, 1, 1), pad=None, up=(1, 1, 1), out_size=None):
    pad = tuple(kk // 2 for kk in k) if pad is None else pad
    x = torch.empty(B, cin, *size)
    x1 = torch.empty(B, cin1, *size) if cin1 else None
    o = out_size or tuple(((i * u + 2 * p - kk) // s + 1) for i, u, kk, s, p in zip(size, up, k, stride, pad))
    y = torch.empty(B, cout, *o)
    return conv_desc(x, x1, y, None, cout, k, stride, pad, up, 0, 0)


COVERED = [dict(k=(7, 7, 7), size=(4, 8, 32)), dict(k=(1, 7, 7), size=(1, 16, 128), cin=3), dict(k=(1, 1, 7), size=(1, 1, 64), cin=1)]
UNCOVERED = {
    "cin12": dict(cin=12), "cout8": dict(cout=8), "stride2": dict(stride=(1, 1, 2), size=(4, 8, 64)), "pad2": dict(pad=(3, 3, 2), size=(4, 8, 34)),
    "cin1": dict(cin=4, cin1=3), "upsample": dict(up=(1, 1, 2), size=(4, 8, 16)), "rows24": dict(size=(4, 8, 24)),
    "taps3": dict(k=(3, 3, 3)), "taps_7x1x7": dict(k=(7, 1, 7)), "cout96": dict(cout=96),
}


def test_stem_f16_ok_is_descriptor_only_and_batch_free():
    lib = _lib.get_lib()
    assert lib.sdc_conv_stem_f16_ok(None) == 0
    for B in (1, 64):
        for kw in COVERED:
            assert lib.sdc_conv_stem_f16_ok(C.byref(_desc(B=B, **kw))) == 1, kw
        for name, kw in UNCOVERED.items():
            d = _desc(B=B, **kw)
            assert lib.sdc_conv_stem_f16_ok(C.byref(d)) == 0, name
    # the uncovered descriptors above differ from a covered one in the named field only: rows of 32 / 64 where they need one
    assert _desc(**UNCOVERED["stride2"]).oW == 32 and _desc(**UNCOVERED["upsample"]).oW == 32 and _desc(**UNCOVERED["pad2"]).oW == 32
    # precision is unread; a strided (frame-major) input is covered, rows that are not dense are not
    d = _desc()
    for prec in (0, 4, 6, 99):
        d.precision = prec
        assert lib.sdc_conv_stem_f16_ok(C.byref(d)) == 1
    x = torch.empty(2, 4, 7, 8, 32).permute(0, 2, 1, 3, 4)
    d = conv_desc(x, None, torch.empty(2, 64, 4, 8, 32), None, 64, (7, 7, 7), (1, 1, 1), (3, 3, 3), (1, 1, 1), 0, 0)
    assert lib.sdc_conv_stem_f16_ok(C.byref(d)) == 1
    d.x0s[4] = 2
    assert lib.sdc_conv_stem_f16_ok(C.byref(d)) == 0
    d.x0s[4] = 1
    d.ys[4] = 2
    assert lib.sdc_conv_stem_f16_ok(C.byref(d)) == 0


def test_stem_f16_entry_rejects_before_any_launch():
    lib = _lib.get_lib()
    d = _desc()
    assert lib.sdc_conv_stem_f16(None, 256, 256, 0, 256, None) == SDC_ENULL
    assert lib.sdc_conv_stem_f16(C.byref(d), 0, 256, 0, 256, None) == SDC_ENULL
    assert lib.sdc_conv_stem_f16(C.byref(d), 256, 0, 0, 256, None) == SDC_ENULL
    assert lib.sdc_conv_stem_f16(C.byref(d), 256, 256, 0, 0, None) == SDC_ENULL
    assert "null" in _lib.last_error()
    for name, kw in UNCOVERED.items():
        assert lib.sdc_conv_stem_f16(C.byref(_desc(**kw)), 256, 256, 0, 256, None) == SDC_EINVAL, name
        assert "not covered" in _lib.last_error()


def test_plan_switch_leaves_the_other_layouts_alone():
    plan = Plan("cpu", precision=4, stem_f16=True)
    assert plan.stem_f16 is True and Plan("cpu", precision=4).stem_f16 is False and Plan("cpu").stem_f16 is False
    with pytest.raises(ValueError):
        Plan("cpu", precision=8, stem_f16=True)
    g = torch.Generator().manual_seed(3)
    for prec in (4, 6):
        on, off = Plan("cpu", precision=prec, stem_f16=True), Plan("cpu", precision=prec)
        # uncovered weights (and, through conv_weight, every weight): the unchanged precision-4 / precision-6 buffers
        for shape in ((64, 12, 7), (8, 7, 7, 7, 7), (64, 7, 7, 7, 7), (40, 24, 3, 3), (16, 8, 3, 3, 3), (16, 8, 1)):
            w = torch.randn(*shape, generator=g)
            assert torch.equal(on.conv_weight(w), off.conv_weight(w))
            assert torch.equal(on.conv_weight(w), pack_conv_weight(w, precision=prec))
    # a 7x7 weight packed at precision 6 is still precision 4's buffer
    w = torch.randn(16, 8, 7, 7, generator=g)
    assert torch.equal(Plan("cpu", precision=6, stem_f16=True).conv_weight(w), pack_conv_weight(w, precision=4))
