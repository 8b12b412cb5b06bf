"""CPU-side checks of net.gemm_split (include/sdc.h, sdc_conv_gemm_x3): the three bf16 planes
Wb[piece][co // 64][stage][block * taps + tap][co % 64][ci % 16] of the strided (1,4,4), sub-pixel (1,2,2) and 1x1x1 conv weights sum to
the fp32 weight bit for bit; the size function; the sub-pixel pack comes from the merged sub-filters of conv_weight(w, ("convT_sub", ph,
pw)); the coverage predicate; the plan's switch."""
import ctypes as C

import pytest
import torch

from safediffcon_amd import _lib
from safediffcon_amd.engine import Plan, conv_desc, pack_conv_weight, pack_gemm_x3

SDC_EINVAL, SDC_ENULL = -1, -4
NCB = {(4, 4): 1, (2, 2): 2, (1, 1): 4}


def _unpack(buf, cout, cin, k):
    """the three planes of a pack_gemm_x3 buffer as fp64 [piece][tap][ci][co]"""
    taps, ncb = k[0] * k[1], NCB[k]
    p = buf.view(torch.bfloat16).reshape(3, cout // 64, cin // (16 * ncb), ncb, taps, 64, 16).double()
    return p.permute(0, 4, 2, 3, 6, 1, 5).reshape(3, taps, cin, cout)        # [piece][tap][(stage, block, c16)][(m tile, co)]


@pytest.mark.parametrize("cout,cin,k", [(64, 64, (4, 4)), (128, 48, (4, 4)), (128, 128, (2, 2)), (64, 32, (2, 2)), (384, 256, (1, 1)),
                                        (64, 64, (1, 1)), (128, 512, (1, 1))])
def test_pack_gemm_x3_planes_sum_to_the_weight_bit_for_bit(cout, cin, k):
    g = torch.Generator().manual_seed(cout + cin + k[0])
    taps = k[0] * k[1]
    wp = torch.randn(taps * cin, cout, generator=g) * 3.0
    wp[0, 0], wp[1, 1] = 0.0, -0.0
    got = pack_gemm_x3(wp, cout, cin, (1, *k))
    assert got.numel() * 4 == _lib.get_lib().sdc_pack_gemm_x3_bytes(cout, cin, *k) == 3 * taps * cin * cout * 2
    planes = _unpack(got, cout, cin, k)
    total = planes[0] + planes[1] + planes[2]                                 # (exact in fp64: 3 x 8 bits)
    want = wp.double().reshape(taps, cin, cout)
    assert torch.equal(total, want)
    # the first plane is the bf16 rounding (RNE) of the weight; zeros stay zeros in the lower planes
    assert torch.equal(planes[0].float(), want.float().bfloat16().float())
    assert (planes[1:, 0, 0, 0] == 0).all() and (planes[1:, 0, 1, 1] == 0).all()
    # the 2-D tap tuple packs the same buffer; so does the plan
    assert torch.equal(pack_gemm_x3(wp, cout, cin, k).view(torch.int32), got.view(torch.int32))
    assert torch.equal(Plan("cpu", precision=4, gemm_split=True).packed(lambda: pack_gemm_x3(wp, cout, cin, k)).view(torch.int32),
                       got.view(torch.int32))


def test_pack_gemm_x3_layout_one_element():
    # w[tap 5][ci 37][co 70] of a 4x4 conv, Cin 48, Cout 128: m tile 1, stage 2 (NCB 1), step 5, row 6, column 5
    wp = torch.zeros(16 * 48, 128)
    wp[5 * 48 + 37, 70] = 1.0
    p = pack_gemm_x3(wp, 128, 48, (4, 4)).view(torch.bfloat16).reshape(3, 2, 3, 16, 64, 16)
    assert p[0, 1, 2, 5, 6, 5] == 1.0 and p.float().abs().sum() == 1.0
    # 1x1, Cin 128: ci 37 + 64 = stage 1, block 2, c16 5
    wp = torch.zeros(128, 64)
    wp[101, 3] = 1.0
    p = pack_gemm_x3(wp, 64, 128, (1, 1)).view(torch.bfloat16).reshape(3, 1, 2, 4, 64, 16)
    assert p[0, 0, 1, 2, 3, 5] == 1.0 and p.float().abs().sum() == 1.0


def test_pack_gemm_x3_sub_pixel_comes_from_the_merged_sub_filters():
    g = torch.Generator().manual_seed(5)
    w = torch.randn(64, 128, 1, 4, 4, generator=g)                            # nn.ConvTranspose3d weight (Cin, Cout, 1, 4, 4)
    plan = Plan("cpu", precision=4, gemm_split=True)
    for ph in (0, 1):
        for pw in (0, 1):
            sub = plan.conv_weight(w, ("convT_sub", ph, pw))                  # [4 * Cin][Cout], what the fp32 kernel reads
            assert tuple(sub.shape) == (4 * 64, 128)
            assert torch.equal(sub, pack_conv_weight(w, ("convT_sub", ph, pw), 0))
            planes = _unpack(pack_gemm_x3(sub, 128, 64, (2, 2)), 128, 64, (2, 2))
            assert torch.equal(planes.sum(0), sub.double().reshape(4, 64, 128))
            # tap (th, tw) of parity (ph, pw) is kernel element (3 - 2 th - ph, 3 - 2 tw - pw) of the transposed conv
            for th in (0, 1):
                for tw in (0, 1):
                    assert torch.equal(planes.sum(0)[2 * th + tw], w[:, :, 0, 3 - 2 * th - ph, 3 - 2 * tw - pw].double())


def test_pack_gemm_x3_rejects_other_weights():
    lib = _lib.get_lib()
    for cout, cin, k in ((64, 64, (3, 3)), (32, 64, (1, 1)), (64, 32, (1, 1)), (64, 16, (2, 2)), (64, 8, (4, 4)), (64, 64, (1, 3))):
        with pytest.raises(ValueError):
            pack_gemm_x3(torch.zeros(k[0] * k[1] * cin, cout), cout, cin, k)
        assert lib.sdc_pack_gemm_x3_bytes(cout, cin, *k) == 0
    with pytest.raises(ValueError):
        pack_gemm_x3(torch.zeros(64, 64 * 16), 64, 64, (4, 4))               # not Wp [taps * Cin][Cout]


def _desc(form, cin=64, cout=64, hw=(8, 32), **kw):
    H, W = hw
    x = torch.empty(2, cin, 2, H, W)
    if form == "a":
        y = torch.empty(2, cout, 2, H // 2, W // 2)
        args = ((1, 4, 4), (1, 2, 2), (0, 1, 1))
    elif form == "b":
        y = torch.empty(2, cout, 2, 2 * H, 2 * W)[:, :, :, 0::2, 1::2]
        args = ((1, 2, 2), (1, 1, 1), (0, 1, 0))
    else:
        y = torch.empty(2, cout, 2, H, W)
        args = ((1, 1, 1), (1, 1, 1), (0, 0, 0))
    return conv_desc(x, kw.get("x1"), y, kw.get("residual"), cout, *args, (1, 1, 1), 0, 0), x, y


def test_gemm_x3_entry_rejects_what_the_kernel_has_no_form_for():
    """host only: the checks run before any launch"""
    lib = _lib.get_lib()
    for form in "abc":
        d, x, y = _desc(form)
        assert lib.sdc_conv_gemm_x3(None, 1, 1, 0, 1, None) == SDC_ENULL
        assert lib.sdc_conv_gemm_x3(C.byref(d), 0, 1, 0, 1, None) == SDC_ENULL
        # a second input, a residual, channel counts outside whole blocks, upsampling, depth taps
        d1, _, _ = _desc(form, x1=torch.empty_like(x))
        d2, _, _ = _desc(form, residual=torch.empty(y.shape))
        d3, _, _ = _desc(form, cin=24)
        d4, _, _ = _desc(form, cout=32)
        d5, _, _ = _desc(form)
        d5.uH = d5.uW = 2
        d6, _, _ = _desc(form, hw=(8, 24))                                    # rows of 12 / 24 / 24 columns
        for bad in (d1, d2, d3, d4, d5, d6):
            assert lib.sdc_conv_gemm_x3_ok(C.byref(bad)) == 0
            assert lib.sdc_conv_gemm_x3(C.byref(bad), 1, 1, 0, 1, None) == SDC_EINVAL
    assert lib.sdc_conv_gemm_x3_ok(None) == 0


def test_gemm_x3_predicate_does_not_look_at_the_batch():
    lib = _lib.get_lib()
    for form in "abc":
        for cin, cout, hw in ((64, 64, (64, 64)), (128, 128, (32, 32)), (256, 384, (16, 16)), (64, 64, (8, 32))):
            d, _, _ = _desc(form, cin=cin, cout=cout, hw=hw)
            want = lib.sdc_conv_gemm_x3_ok(C.byref(d))
            for B in (1, 3, 64, 1000):
                d.B = B
                assert lib.sdc_conv_gemm_x3_ok(C.byref(d)) == want


def test_plan_switch():
    assert Plan("cpu").gemm_split is False and Plan("cpu", precision=4).gemm_split is False         # a Plan built directly: today's routes
    for prec, on in ((0, False), (2, False), (3, False), (4, True), (5, True), (6, True), (7, True)):
        assert Plan("cpu", precision=prec, gemm_split=True).gemm_split is on
    import safediffcon_amd as sdc
    net = sdc.Unet1D(dim=8, dim_mults=(1, 2, 4, 8), channels=12, resnet_block_groups=1)
    assert net.gemm_split is True and net.stem_split is True and net.precision == 4
