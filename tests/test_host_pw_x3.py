"""CPU-side checks of conv_pw_x3_kernel's routing table and coverage (include/sdc.h, sdc_conv_pw_x3_ok / sdc_conv_pw_x3): the table is
keyed on per-sample sizes only, never on B, and what the kernel does not cover is refused before any launch."""
import ctypes as C

import torch

from safediffcon_amd import _lib
from safediffcon_amd.engine import conv_desc

SDC_ENULL, SDC_EINVAL = -4, -1


def _desc(B, c0, c1, cout, sp, k=(1, 1, 1), stride=(1, 1, 1), pad=(0, 0, 0), res=False, precision=4, osp=None):
    """descriptor of dense tensors of these sizes (meta tensors: only shapes and strides are read)"""
    x0 = torch.empty(B, c0, *sp, device="meta")
    x1 = torch.empty(B, c1, *sp, device="meta") if c1 else None
    y = torch.empty(B, cout, *(osp or sp), device="meta")
    return conv_desc(x0, x1, y, y if res else None, cout, k, stride, pad, (1, 1, 1), 0, precision)


# (Cin0, Cin1, Cout, per-sample volume): the 1x1 convs of the C4 plan the kernel covers
C4_SHAPES = [(128, 0, 384, (32, 32, 32)), (256, 0, 384, (32, 16, 16)), (128, 0, 256, (32, 16, 16)), (64, 64, 64, (32, 64, 64)),
             (128, 0, 128, (32, 32, 32)), (128, 128, 64, (32, 32, 32)), (128, 0, 384, (32, 16, 16)), (64, 0, 128, (32, 32, 32)),
             (128, 0, 128, (32, 16, 16))]


def test_pw_x3_table_does_not_look_at_the_batch():
    lib = _lib.get_lib()
    listed = 0
    for c0, c1, cout, sp in C4_SHAPES + [(64, 0, 64, (4, 96, 96)), (256, 256, 128, (32, 16, 16)), (128, 0, 128, (2, 8, 32))]:
        for res in (False, True):
            want = lib.sdc_conv_pw_x3_ok(C.byref(_desc(1, c0, c1, cout, sp, res=res)))
            for B in (2, 64):
                assert lib.sdc_conv_pw_x3_ok(C.byref(_desc(B, c0, c1, cout, sp, res=res))) == want, (c0, c1, cout, sp, B)
            listed += want
    assert listed > 0                                                            # the table routes something
    assert lib.sdc_conv_pw_x3_ok(C.byref(_desc(2, 256, 256, 128, (32, 16, 16)))) == 0       # K = 512: no weight block fits the LDS
    assert lib.sdc_conv_pw_x3_ok(C.byref(_desc(2, 64, 0, 64, (4, 96, 96)))) == 0            # covered, not a measured shape
    assert lib.sdc_conv_pw_x3_ok(None) == 0


def test_pw_x3_refuses_what_the_kernel_does_not_cover():
    lib = _lib.get_lib()
    assert lib.sdc_conv_pw_x3(None, 256, 0, 256, 0, 0, 256, None) == SDC_ENULL
    ok = _desc(2, 128, 0, 256, (32, 16, 16))
    for args in ((0, 0, 256, 0, 0, 256), (256, 0, 0, 0, 0, 256), (256, 0, 256, 0, 0, 0)):
        assert lib.sdc_conv_pw_x3(C.byref(ok), *args, None) == SDC_ENULL
    bad = [
        _desc(2, 128, 0, 256, (32, 16, 16), stride=(1, 2, 2), osp=(32, 8, 8)),             # stride 2
        _desc(2, 128, 0, 256, (32, 16, 16), k=(1, 1, 3), pad=(0, 0, 1)),                    # 3 taps
        _desc(2, 128, 0, 80, (32, 16, 16)),                                                 # Cout not a whole number of blocks
        _desc(2, 48, 0, 128, (32, 16, 16)),                                                 # K below 64
        _desc(2, 80, 0, 128, (32, 16, 16)),                                                 # K not a multiple of 32
        _desc(2, 512, 0, 64, (32, 16, 16)),                                                 # the weight block does not fit
        _desc(2, 128, 0, 256, (1, 5, 6)),                                                   # 30 positions: not a multiple of 4
    ]
    strided = _desc(2, 128, 0, 256, (32, 16, 16))
    strided.x0s[4] = 2                                                                      # x not dense
    misaligned = _desc(2, 128, 0, 256, (32, 16, 16))
    misaligned.ys[1] += 2                                                                   # rows of y not 16-byte aligned
    for d in bad + [strided, misaligned]:
        assert lib.sdc_conv_pw_x3_ok(C.byref(d)) == 0
        assert lib.sdc_conv_pw_x3(C.byref(d), 256, 0, 256, 0, 0, 256, None) == SDC_EINVAL   # (before any launch: no GPU is touched)
    assert lib.sdc_conv_pw_x3(C.byref(ok), 256, 0, 256, 0, 0, 264, None) == SDC_EINVAL       # y itself not 16-byte aligned
    # precision is not part of the table (route() asks for precision >= 4 itself)
    assert lib.sdc_conv_pw_x3_ok(C.byref(_desc(2, 128, 0, 256, (32, 16, 16), precision=0))) == lib.sdc_conv_pw_x3_ok(C.byref(ok))
