"""CPU-side checks of the precision-6 weight layout (include/sdc.h, SdcConvDesc.precision 6): precision 4's buffer, zero-padded to
16 bytes, followed by the fp16 tail Wh[tap][ci // KC][co][ci % KC] (RNE, Cin zero-padded to whole KC chunks)."""
import pytest
import torch

from safediffcon_amd import _lib
from safediffcon_amd.engine import Plan, pack_conv_weight


def _tail_ref(w, kc):
    """the documented layout written out with explicit loops over (tap, chunk, co, k)"""
    co, ci = w.shape[:2]
    w5 = w.reshape(co, ci, 1, 1, -1) if w.dim() == 3 else (w.reshape(co, ci, 1, *w.shape[2:]) if w.dim() == 4 else w)
    taps = w5.reshape(co, ci, -1)
    nch = (ci + kc - 1) // kc
    out = torch.zeros(taps.shape[2], nch, co, kc, dtype=torch.float16)
    for t in range(taps.shape[2]):
        for c in range(ci):
            out[t, c // kc, :, c % kc] = taps[:, c, t].half()
    return out.reshape(-1)


@pytest.mark.parametrize("shape,kc", [((40, 20, 3), 32), ((24, 64, 3), 32), ((40, 24, 3, 3), 32), ((8, 8, 3, 3, 3), 32),
                                      ((64, 48, 3, 3, 3), 32)])
def test_precision6_buffer_is_precision4_then_fp16_tail(shape, kc):
    g = torch.Generator().manual_seed(sum(shape))
    w = torch.randn(*shape, generator=g) * 3.0
    p4 = pack_conv_weight(w, precision=4)
    p6 = pack_conv_weight(w, precision=6)
    gap = -p4.numel() % 4
    assert torch.equal(p6[:p4.numel()], p4)
    assert torch.equal(p6[p4.numel():p4.numel() + gap], torch.zeros(gap))
    tail = p6[p4.numel() + gap:].contiguous().view(torch.float16)
    assert torch.equal(tail, _tail_ref(w, kc))
    ks = (1, 1) + tuple(shape[2:]) if len(shape) == 3 else ((1,) + tuple(shape[2:]) if len(shape) == 4 else tuple(shape[2:]))
    assert p6.numel() == _lib.get_lib().sdc_pack_conv_weight_floats(shape[0], shape[1], *ks, 6)
    # the plan packs the same buffer
    assert torch.equal(Plan("cpu", precision=6).conv_weight(w), p6)


def test_precision6_other_taps_keep_precision4_layout():
    lib = _lib.get_lib()
    for shape in ((16, 8, 1), (16, 8, 7, 7), (16, 8, 1, 2, 2), (16, 8, 3, 3, 1)):
        w = torch.randn(*shape)
        assert torch.equal(pack_conv_weight(w, precision=6), pack_conv_weight(w, precision=4))
        ks = tuple(shape[2:])
        ks = (1,) * (3 - len(ks)) + ks
        assert lib.sdc_pack_conv_weight_floats(16, 8, *ks, 6) == lib.sdc_pack_conv_weight_floats(16, 8, *ks, 4)
    for kind in ("convT", ("convT_sub", 0, 1), ("up2_sub", 1, 0)):
        w = torch.randn(8, 8, 1, 4, 4) if kind != ("up2_sub", 1, 0) else torch.randn(8, 8, 3, 3)
        assert torch.equal(pack_conv_weight(w, kind, precision=6), pack_conv_weight(w, kind, precision=4))


def test_precision6_rounding_is_nearest_even():
    # halfway cases between two fp16 neighbours round to the even one (RNE); round-toward-zero would truncate them all
    one = 1.0 + 2.0 ** -11                           # halfway between 1 and 1 + 2^-10: even -> 1
    three = 1.0 + 3 * 2.0 ** -11                     # halfway between 1 + 2^-10 and 1 + 2^-9: even -> 1 + 2^-9
    w = torch.tensor([one, three, -three], dtype=torch.float32).reshape(1, 3, 1).repeat(1, 1, 3)
    p6 = pack_conv_weight(w, precision=6)
    tail = p6[(pack_conv_weight(w, precision=4).numel() + 3) // 4 * 4:].view(torch.float16).float()
    assert tail[0].item() == 1.0 and tail[1].item() == 1.0 + 2.0 ** -9 and tail[2].item() == -(1.0 + 2.0 ** -9)


def test_precision6_switch_and_batch_plan():
    Plan("cpu", precision=6)
    Plan("cpu", precision=7)
    with pytest.raises(ValueError):
        Plan("cpu", precision=8)
    lib = _lib.get_lib()
    it = (_lib.SdcPackItem * 1)()
    it[0].w, it[0].out = 256, 256
    it[0].Cout, it[0].Cin, it[0].kD, it[0].kH, it[0].kW, it[0].precision, it[0].flip = 16, 16, 1, 1, 3, 6, 0
    import ctypes as C
    nb, lds = C.c_int(0), C.c_int(0)
    assert lib.sdc_pack_batch_plan(it, 1, C.byref(nb), C.byref(lds)) != 0      # training never asks for precision 6
