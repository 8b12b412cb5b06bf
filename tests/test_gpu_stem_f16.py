"""-m gpu: net.stem_f16 (opt-in, samplers only) -- the 7-tap stem convs on the fp16 matrix pipe (csrc/sdc_conv_stem_f16.hip): fp16
operands (RNE), fp32 accumulation.  Conv level, through the C ABI: against an fp64 conv of the ROUNDED operands (only the fp32
accumulation order may differ) and of the exact ones, determinism, batch invariance, the device packer.  Net level: the eps-MSE
contract gate against the reference fixtures at precision 4 and 6, graph replay, batch invariance; and nothing else moves (switch off,
fine-tuning, uncovered stems keep their bits); a `.data` write to the stem weight is seen by the next call."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import safediffcon_amd as sdc
from safediffcon_amd import _lib
from safediffcon_amd.engine import conv_desc, pack_stem_f16
from oracle.detweights import det_params, det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


# (B, Cin, Cout, (D, H, W), (kD, kH, kW), frame_major): the smallest shapes at which the kernel can still go wrong
FORMS = {
    "depth_shorter_than_taps": (2, 7, 64, (4, 8, 32), (7, 7, 7), False),        # every kd clips
    "interior_depth_short_planes": (1, 7, 64, (9, 4, 64), (7, 7, 7), False),    # fewer rows than the kh halo
    "rows16_many_planes_ragged": (3, 7, 64, (3, 4, 16), (7, 7, 7), False),      # a tile spans 4 planes; 576 positions: ragged last tile
    "two_m_tiles": (1, 7, 128, (2, 8, 32), (7, 7, 7), False),
    "burgers_stem": (3, 3, 64, (1, 16, 128), (1, 7, 7), False),
    "cin8_h2": (2, 8, 64, (1, 2, 32), (1, 7, 7), False),                        # no pad channel
    "cin1_1d": (2, 1, 64, (1, 1, 64), (1, 1, 7), False),
    "frame_major": (2, 7, 64, (4, 8, 32), (7, 7, 7), True),                     # strided input view
    # tiles whose rows cross (sample, depth) planes at no multiple of the plane height, and planes of one row: the kernel instance
    # with up to 2048 staged positions (the forms above run the 512- and 1024-position ones)
    "unaligned_planes_rows64": (2, 5, 64, (2, 6, 64), (7, 7, 7), False),
    "unaligned_planes_rows128": (1, 2, 64, (1, 5, 128), (1, 7, 7), False),
    "planes_of_one_row_rows16": (1, 2, 64, (3, 1, 16), (7, 7, 7), False),
}
_CASE = {}


def _case(form):
    """inputs, fp64 references (computed once per form, never modified) and the CPU-side check of the inputs"""
    if form not in _CASE:
        B, ci, co, (D, H, W), k, fm = FORMS[form]
        g = torch.Generator().manual_seed(11)
        if fm:
            x = (torch.randn(B, D, ci, H, W, generator=g) * 2.0).permute(0, 2, 1, 3, 4)      # (B, C, F, H, W) view of (B, F, C, H, W)
        else:
            x = torch.randn(B, ci, D, H, W, generator=g) * 2.0
        w = torch.randn(co, ci, *k, generator=g) / (3.0 * (ci * k[0] * k[1] * k[2]) ** 0.5)
        bias = 0.1 * torch.randn(co, generator=g)
        pad = tuple(kk // 2 for kk in k)
        extra = bias.double().view(1, -1, 1, 1, 1)
        ref_r = F.conv3d(x.half().double(), w.half().double(), padding=pad) + extra
        ref_x = F.conv3d(x.double(), w.double(), padding=pad) + extra
        rms = ref_r.pow(2).mean().sqrt().item()
        # the rounded-operand reference alone sits near 3e-4 of the exact one on these inputs (two operands, each with a relative
        # rounding error of ~2e-4 rms): the exact-operand gate below then tests the kernel and not the inputs
        e_in = (ref_r - ref_x).pow(2).mean().sqrt().item() / rms
        assert 1.5e-4 <= e_in <= 6e-4, e_in
        _CASE[form] = (x, w, bias, pad, ref_r, ref_x, rms, e_in)
    return _CASE[form]


def _run(x_dev, wh, bias, co, k, pad):
    """one sdc_conv_stem_f16 call on a NaN-filled output"""
    lib = _lib.get_lib()
    y = torch.full((x_dev.shape[0], co, *x_dev.shape[2:]), float("nan"), device=DEV)
    d = conv_desc(x_dev, None, y, None, co, k, (1, 1, 1), pad, (1, 1, 1), 0, 0)
    assert lib.sdc_conv_stem_f16_ok(C.byref(d)) == 1
    _lib.check(lib.sdc_conv_stem_f16(C.byref(d), x_dev.data_ptr(), wh.data_ptr(), bias.data_ptr(), y.data_ptr(), _stream()), "sdc_conv_stem_f16")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("form", list(FORMS))
def test_stem_f16_conv_is_rne_operands_with_fp32_accumulation(form):
    B, ci, co, (D, H, W), k, fm = FORMS[form]
    x, w, bias, pad, ref_r, ref_x, rms, e_in = _case(form)
    lib = _lib.get_lib()
    # device packer == host packer, bit for bit
    nbytes = int(lib.sdc_pack_stem_f16_bytes(co, ci, *k))
    wh = torch.full((nbytes // 4,), float("nan"), device=DEV)
    w_dev = w.to(DEV)
    _lib.check(lib.sdc_pack_stem_f16(w_dev.data_ptr(), wh.data_ptr(), co, ci, *k, _stream()), "sdc_pack_stem_f16")
    torch.cuda.synchronize()
    assert torch.equal(wh.cpu().view(torch.int16), pack_stem_f16(w).view(torch.int16))

    if fm:
        x_dev = x.permute(0, 2, 1, 3, 4).contiguous().to(DEV).permute(0, 2, 1, 3, 4)
        assert not x_dev.is_contiguous()
    else:
        x_dev = x.to(DEV)
    b_dev = bias.to(DEV)
    y = _run(x_dev, wh, b_dev, co, k, pad)
    out = y.double().cpu()
    assert torch.isfinite(out).all()
    e_r = (out - ref_r).pow(2).mean().sqrt().item() / rms
    e_x = (out - ref_x).pow(2).mean().sqrt().item() / rms
    print(f"[measured] {form}: rms err vs rounded-operand fp64 {e_r:.2e}, vs exact fp64 {e_x:.2e} (of the output rms; "
          f"the rounded reference itself: {e_in:.2e})")
    assert e_r <= 1e-5, e_r
    assert e_x <= 1e-3, e_x
    # two runs bit-identical; sample 0 of the batch == the same sample alone
    assert torch.equal(_run(x_dev, wh, b_dev, co, k, pad), y)
    if B > 1:
        assert torch.equal(_run(x_dev[:1], wh, b_dev, co, k, pad)[0], y[0])
    # without a bias
    d = conv_desc(x_dev, None, y, None, co, k, (1, 1, 1), pad, (1, 1, 1), 0, 0)
    y0 = torch.full_like(y, float("nan"))
    _lib.check(lib.sdc_conv_stem_f16(C.byref(d), x_dev.data_ptr(), wh.data_ptr(), 0, y0.data_ptr(), _stream()), "sdc_conv_stem_f16")
    torch.cuda.synchronize()
    assert torch.equal(y0 + b_dev.view(1, -1, 1, 1, 1), y)


# ------------------------------------------------------------------ net level
_NETS = {
    "smoke": (lambda d: sdc.Unet3D_with_Conv3D(dim=d, dim_mults=(1, 2, 4), channels=7), 64, (1, 32, 7, 32, 32), 300),
    "burgers": (lambda d: sdc.Unet2D(dim=d, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1), 64, (2, 3, 16, 128), 100),
    "tokamak": (lambda d: sdc.Unet1D(dim=d, dim_mults=(1, 2, 4, 8), channels=12, resnet_block_groups=1), 256, (2, 12, 128), 200),
}
_WIDE = {}


def _wide(golden, tree):
    """the production-width net of a tree with its fixture's weights, input and reference eps (built once)"""
    if tree not in _WIDE:
        make, dim, shape, _ = _NETS[tree]
        g = golden(f"{tree}_unet_wide")
        net = make(dim)
        net.load_state_dict(det_params(g.spec(), int(g.scalar("weight_seed"))))
        net.to(DEV)
        _WIDE[tree] = (net, det_tensor(shape, int(g.scalar("x_seed"))).to(DEV), g["t"].to(DEV), g["eps"])
    return _WIDE[tree]


def _calls(net, x):
    return [fn.__name__ for fn, _ in net.entry(tuple(x.shape), x.shape[0])["plan"].calls]


@pytest.mark.parametrize("tree", ["smoke", "burgers"])
def test_stem_f16_nets_against_reference_fixtures(golden, tree):
    net, x, t, ref = _wide(golden, tree)
    try:
        for prec in (4, 6):
            net.precision, net.stem_f16, net.forward_graph = prec, True, True
            eps = net(x, t).cpu()
            mse = ((eps - ref) ** 2).mean().item()
            print(f"[measured] {tree}_unet_wide precision {prec} + stem_f16: eps-MSE {mse:.3e}  max|err| {(eps - ref).abs().max().item():.3e}")
            assert torch.isfinite(eps).all()
            assert mse <= 1e-5
            assert _calls(net, x).count("sdc_conv_stem_f16") == 1
            # graph replay == eager call list, two runs bit-identical
            net.forward_graph = False
            eager = net(x, t).cpu()
            net.forward_graph = True
            assert torch.equal(eager, eps) and torch.equal(net(x, t).cpu(), eps)
            # a sample's eps does not depend on the batch it rides in
            x2, t2 = torch.cat([x, x.flip(-1)]), torch.cat([t, t])
            assert torch.equal(net(x2, t2).cpu()[:x.shape[0]], eps)
            assert torch.equal(net(x[:1], t[:1]).cpu()[0], eps[0])
    finally:
        net.precision, net.stem_f16 = 4, False


def test_stem_f16_off_on_off_and_fine_tuning_untouched(golden):
    net, x, t, _ = _wide(golden, "burgers")
    try:
        net.precision, net.stem_f16 = 4, False
        e0 = net(x, t).clone()
        assert "sdc_conv_stem_f16" not in _calls(net, x)
        net.stem_f16 = True
        e1 = net(x, t).clone()
        net.stem_f16 = False
        assert torch.equal(net(x, t), e0) and not torch.equal(e1, e0)
        # forward_train: loss and every gradient bit-identical with the switch on and off
        res = {}
        for on in (False, True):
            net.stem_f16 = on
            net.zero_grad(set_to_none=True)
            loss = (net.forward_train(x, t) ** 2).mean()
            loss.backward()
            res[on] = (loss.detach().cpu(), [None if p.grad is None else p.grad.detach().cpu().clone() for p in net.parameters()])
        assert any(a is not None for a in res[False][1])
        assert torch.equal(res[False][0], res[True][0])
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(res[False][1], res[True][1]))
    finally:
        net.stem_f16 = False
        net.zero_grad(set_to_none=True)


def test_stem_f16_uncovered_stems_keep_their_bits(golden):
    # the tokamak stem (Cin 12) and a dim-8 net (Cout 8): switch on == switch off, bit for bit, and no stem call in the plan
    net, x, t, _ = _wide(golden, "tokamak")
    g = golden("smoke_unet")
    small = _NETS["smoke"][0](8)
    small.load_state_dict(det_params(g.spec(), 300))
    small.to(DEV)
    for n, xx, tt in ((net, x, t), (small, g["x"].to(DEV), g["t"].to(DEV))):
        try:
            n.stem_f16 = False
            e0 = n(xx, tt).clone()
            n.stem_f16 = True
            assert torch.equal(n(xx, tt), e0)
            assert "sdc_conv_stem_f16" not in _calls(n, xx)
        finally:
            n.stem_f16 = False


def test_stem_f16_sees_data_writes_to_the_stem_weight(golden):
    net, x, t, _ = _wide(golden, "burgers")
    make, dim, _, _ = _NETS["burgers"]
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    try:
        net.precision, net.stem_f16 = 4, True
        e0 = net(x, t).clone()
        net.init_conv.weight.data.mul_(1.5)
        e1 = net(x, t).clone()
        fresh = make(dim)
        fresh.load_state_dict(net.state_dict())
        fresh.to(DEV)
        fresh.stem_f16 = True
        assert torch.equal(fresh(x, t), e1) and not torch.equal(e1, e0)
    finally:
        net.load_state_dict(sd)
        net.stem_f16 = False
