"""CPU-side checks of fine-tuning with fp16 operands (net.train_precision, include/sdc.h "Fine-tuning with fp16 operands"): the switch,
the precision-8 fp16 tail of the data-gradient weight, and the batched pack plan."""
import ctypes as C

import pytest
import torch

import safediffcon_amd as sdc
from safediffcon_amd import _lib
from safediffcon_amd.autograd import check_train_precision, f16_train_form
from safediffcon_amd.engine import Plan, f16_tail


def test_train_precision_switch():
    net = sdc.Unet1D(dim=8, dim_mults=(1, 2), channels=4, resnet_block_groups=1)
    assert net.train_precision is None
    for v in (6, 7, None):
        net.train_precision = v
        assert net.train_precision == v
    for bad in (0, 4, 5, 8, True, 6.0, "6"):
        with pytest.raises(ValueError):
            net.train_precision = bad
        with pytest.raises(ValueError):
            check_train_precision(bad)
    assert net.train_precision is None                      # a rejected value leaves the switch as it was
    # the forms the switch routes to the fp16 kernels
    assert f16_train_form((1, 1, 3), (1, 1, 1), (0, 0, 1), (1, 1, 1))
    assert f16_train_form((1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 1, 1))
    assert f16_train_form((3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1))
    assert not f16_train_form((1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1))        # 1x1
    assert not f16_train_form((1, 1, 3), (1, 1, 2), (0, 0, 1), (1, 1, 1))        # strided
    assert not f16_train_form((1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 2, 2))        # upsampling folded into the read
    assert not f16_train_form((1, 7, 7), (1, 1, 1), (0, 3, 3), (1, 1, 1))        # stem


def _flip_tail_ref(w, kc=32):
    """the flipped layout written out with explicit loops: Wh[tap][ci' // KC][co'][ci' % KC] = fp16(w[ci'][co'][T - 1 - tap]),
    co' = input channel of w, ci' = output channel of w"""
    co, ci = w.shape[:2]
    taps = w.reshape(co, ci, -1)
    T = taps.shape[2]
    nch = (co + kc - 1) // kc
    out = torch.zeros(T, nch, ci, kc, dtype=torch.float16)
    for t in range(T):
        for c in range(co):                                   # ci' = c
            out[t, c // kc, :, c % kc] = taps[c, :, T - 1 - t].half()
    return out.reshape(-1)


@pytest.mark.parametrize("shape", [(40, 20, 3), (24, 72, 3), (40, 24, 3, 3), (8, 8, 3, 3, 3), (33, 48, 3, 3, 3)])
def test_precision8_flip_tail_is_rne_of_the_flipped_transposed_taps(shape):
    g = torch.Generator().manual_seed(7 + sum(shape))
    w = torch.randn(*shape, generator=g) * 3.0
    assert torch.equal(f16_tail(w, flip=True).view(torch.float16), _flip_tail_ref(w))
    # without flip it is precision 6's tail
    assert torch.equal(f16_tail(w, flip=False), f16_tail(w))
    lib = _lib.get_lib()
    ks = ((1, 1) + tuple(shape[2:])) if len(shape) == 3 else (((1,) + tuple(shape[2:])) if len(shape) == 4 else tuple(shape[2:]))
    # precision 8 buffers are sized like precision 6's (the data-gradient weight: channel counts swapped)
    for co, ci in ((shape[0], shape[1]), (shape[1], shape[0])):
        assert lib.sdc_pack_conv_weight_floats(co, ci, *ks, 8) == lib.sdc_pack_conv_weight_floats(co, ci, *ks, 6)


def _plan(precision, flip=0, k=(1, 1, 3)):
    lib = _lib.get_lib()
    it = (_lib.SdcPackItem * 1)()
    it[0].w, it[0].out = 256, 256
    it[0].Cout, it[0].Cin = 16, 24
    it[0].kD, it[0].kH, it[0].kW = k
    it[0].precision, it[0].flip = precision, flip
    nb, lds = C.c_int(0), C.c_int(0)
    return lib.sdc_pack_batch_plan(it, 1, C.byref(nb), C.byref(lds)), nb.value


def test_batch_plan_takes_the_training_layout_and_still_rejects_precision6():
    for k in ((1, 1, 3), (1, 3, 3), (3, 3, 3), (1, 1, 1)):
        for flip in (0, 1):
            rc, nb = _plan(8, flip, k)
            assert rc == 0 and nb > 0, (k, flip)
    assert _plan(6)[0] != 0 and _plan(7)[0] != 0
    with pytest.raises(ValueError):
        Plan("cpu", precision=8)
