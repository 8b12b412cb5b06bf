"""-m gpu: net.stem_split (default on at precision >= 4, samplers only) -- the 7-tap stem convs as exact three-way bf16 operand splits
on the bf16 matrix pipe (csrc/sdc_conv_stem_x3.hip): fp32 in, fp32 accumulation, fp32 out.  Conv level, through the C ABI: the error
against an exact-operand fp64 conv next to that of today's fp32 kernel (sdc_conv at precision 4) on the same inputs, determinism,
batch invariance, bias, power-of-two scaling invariance, the device packer.  Net level: the eps-MSE contract gate against the reference
fixtures with the default switch, graph replay, and nothing else moves (switch off, precision 0 / 3, fine-tuning, uncovered stems keep
their bits); a `.data` write to the stem weight is seen by the next call."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import safediffcon_amd as sdc
from safediffcon_amd import _lib
from safediffcon_amd.engine import conv_desc, pack_conv_weight, pack_stem_x3
from oracle.detweights import det_params, det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


# (B, Cin, Cout, (D, H, W), (kD, kH, kW), frame_major): the small forms that pin the fp16 stem kernel, whose walk this kernel keeps
FORMS = {
    "depth_shorter_than_taps": (2, 7, 64, (4, 8, 32), (7, 7, 7), False),        # every kd clips
    "interior_depth_short_planes": (1, 7, 64, (9, 4, 64), (7, 7, 7), False),    # fewer rows than the kh halo
    "rows16_many_planes_ragged": (3, 7, 64, (3, 4, 16), (7, 7, 7), False),      # a tile spans 4 planes; 576 positions: ragged last tile
    "two_m_tiles": (1, 7, 128, (2, 8, 32), (7, 7, 7), False),
    "burgers_stem": (3, 3, 64, (1, 16, 128), (1, 7, 7), False),
    "cin8_h2": (2, 8, 64, (1, 2, 32), (1, 7, 7), False),                        # no pad channel
    "cin1_1d": (2, 1, 64, (1, 1, 64), (1, 1, 7), False),                        # K = 7: one final rounding dominates
    "frame_major": (2, 7, 64, (4, 8, 32), (7, 7, 7), True),                     # strided input view
    # tiles whose rows cross (sample, depth) planes at no multiple of the plane height, and planes of one row: the kernel instance
    # with up to 2048 staged positions (the forms above run the 512- and 1024-position ones)
    "unaligned_planes_rows64": (2, 5, 64, (2, 6, 64), (7, 7, 7), False),
    "unaligned_planes_rows128": (1, 2, 64, (1, 5, 128), (1, 7, 7), False),
    "planes_of_one_row_rows16": (1, 2, 64, (3, 1, 16), (7, 7, 7), False),
}
_CASE = {}


def _case(form):
    """inputs and the exact-operand fp64 reference (computed once per form, never modified)"""
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
        ref = F.conv3d(x.double(), w.double(), padding=pad) + bias.double().view(1, -1, 1, 1, 1)
        _CASE[form] = (x, w, bias, pad, ref, ref.pow(2).mean().sqrt().item())
    return _CASE[form]


def _run(x_dev, wb, bias, co, k, pad):
    """one sdc_conv_stem_x3 call on a NaN-filled output (bias: a tensor or None)"""
    lib = _lib.get_lib()
    y = torch.full((x_dev.shape[0], co, *x_dev.shape[2:]), float("nan"), device=DEV)
    d = conv_desc(x_dev, None, y, None, co, k, (1, 1, 1), pad, (1, 1, 1), 0, 0)
    assert lib.sdc_conv_stem_x3_ok(C.byref(d)) == (1 if k[0] == 7 else 0)      # (the kD = 1 stems are run, not routed)
    _lib.check(lib.sdc_conv_stem_x3(C.byref(d), x_dev.data_ptr(), wb.data_ptr(), bias.data_ptr() if bias is not None else 0, y.data_ptr(),
                                    _stream()), "sdc_conv_stem_x3")
    torch.cuda.synchronize()
    return y


def _run_fp32(x_dev, w, bias, co, k, pad):
    """today's kernel: sdc_conv at precision 4 on the same inputs"""
    lib = _lib.get_lib()
    wp = pack_conv_weight(w, precision=4).to(DEV)
    y = torch.full((x_dev.shape[0], co, *x_dev.shape[2:]), float("nan"), device=DEV)
    d = conv_desc(x_dev, None, y, None, co, k, (1, 1, 1), pad, (1, 1, 1), 0, 4)
    _lib.check(lib.sdc_conv(C.byref(d), x_dev.data_ptr(), 0, wp.data_ptr(), bias.data_ptr(), 0, y.data_ptr(), _stream()), "sdc_conv")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("form", list(FORMS))
def test_stem_x3_conv_is_fp32_grade(form):
    B, ci, co, (D, H, W), k, fm = FORMS[form]
    x, w, bias, pad, ref, rms = _case(form)
    lib = _lib.get_lib()
    # device packer == host packer, bit for bit
    nbytes = int(lib.sdc_pack_stem_x3_bytes(co, ci, *k))
    wb = torch.full((nbytes // 4,), float("nan"), device=DEV)
    w_dev = w.to(DEV)
    _lib.check(lib.sdc_pack_stem_x3(w_dev.data_ptr(), wb.data_ptr(), co, ci, *k, _stream()), "sdc_pack_stem_x3")
    torch.cuda.synchronize()
    assert torch.equal(wb.cpu().view(torch.int16), pack_stem_x3(w).view(torch.int16))

    if fm:
        x_dev = x.permute(0, 2, 1, 3, 4).contiguous().to(DEV).permute(0, 2, 1, 3, 4)
        assert not x_dev.is_contiguous()
    else:
        x_dev = x.to(DEV)
    b_dev = bias.to(DEV)
    y = _run(x_dev, wb, b_dev, co, k, pad)
    out = y.double().cpu()
    assert torch.isfinite(out).all()
    # error against the exact-operand fp64 conv, rms over the whole output relative to the output rms, next to today's fp32 kernel's
    e_new = (out - ref).pow(2).mean().sqrt().item() / rms
    e_old = (_run_fp32(x_dev, w, b_dev, co, k, pad).double().cpu() - ref).pow(2).mean().sqrt().item() / rms
    print(f"[measured] {form}: rms err vs exact fp64 (of the output rms): split {e_new:.3e} | fp32 kernel {e_old:.3e}")
    assert e_new <= max(1.25 * e_old, 2.0 ** -23), (e_new, e_old)
    # two runs bit-identical; sample 0 of the batch == the same sample alone
    assert torch.equal(_run(x_dev, wb, b_dev, co, k, pad), y)
    if B > 1:
        assert torch.equal(_run(x_dev[:1], wb, b_dev, co, k, pad)[0], y[0])
    # without a bias
    y0 = _run(x_dev, wb, None, co, k, pad)
    assert torch.equal(y0 + b_dev.view(1, -1, 1, 1, 1), y)
    # power-of-two scaling of x scales the output bit for bit (a lost or flushed third piece would not)
    for e in (40, -40):
        ys = _run(x_dev * 2.0 ** e, wb, None, co, k, pad)
        assert torch.equal(ys, y0 * 2.0 ** e), e


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
def test_stem_split_nets_against_reference_fixtures(golden, tree):
    net, x, t, ref = _wide(golden, tree)
    assert net.precision == 4 and net.stem_split is True and net.stem_f16 is False          # the defaults
    net.forward_graph = True
    eps = net(x, t).cpu()
    mse = ((eps - ref) ** 2).mean().item()
    print(f"[measured] {tree}_unet_wide precision 4, default stem_split: eps-MSE {mse:.3e}  max|err| {(eps - ref).abs().max().item():.3e}")
    assert torch.isfinite(eps).all()
    assert mse <= 1e-5
    # the smoke stem (7x7x7) is routed to the split kernel; the Burgers stem (1x7x7) measured no faster and keeps the fp32 kernel
    assert _calls(net, x).count("sdc_conv_stem_x3") == (1 if tree == "smoke" else 0)
    # graph replay == eager call list, two runs bit-identical
    try:
        net.forward_graph = False
        eager = net(x, t).cpu()
    finally:
        net.forward_graph = True
    assert torch.equal(eager, eps) and torch.equal(net(x, t).cpu(), eps)
    # a sample's eps does not depend on the batch it rides in
    x2, t2 = torch.cat([x, x.flip(-1)]), torch.cat([t, t])
    assert torch.equal(net(x2, t2).cpu()[:x.shape[0]], eps)


def test_stem_split_off_on_off_precisions_and_fine_tuning(golden):
    net, x, t, _ = _wide(golden, "smoke")
    try:
        net.stem_split = False
        e0 = net(x, t).clone()
        assert "sdc_conv_stem_x3" not in _calls(net, x)
        net.stem_split = True
        e1 = net(x, t).clone()
        assert "sdc_conv_stem_x3" in _calls(net, x)
        net.stem_split = False
        assert torch.equal(net(x, t), e0) and not torch.equal(e1, e0)
        # the fp16 switch wins when both are set
        net.stem_split, net.stem_f16 = True, True
        names = _calls(net, x)
        assert "sdc_conv_stem_f16" in names and "sdc_conv_stem_x3" not in names
        net.stem_f16 = False
        # precision 0 and 3: the literal fp32 pipe, whatever the switch says
        for prec in (0, 3):
            net.precision = prec
            res = {}
            for on in (False, True):
                net.stem_split = on
                res[on] = (net(x, t).clone(), _calls(net, x))
            assert torch.equal(res[False][0], res[True][0]) and res[False][1] == res[True][1]
            assert "sdc_conv_stem_x3" not in res[True][1]
        net.precision = 4
        # forward_train: loss and every gradient bit-identical with the switch on and off
        res = {}
        for on in (False, True):
            net.stem_split = on
            net.zero_grad(set_to_none=True)
            loss = (net.forward_train(x, t) ** 2).mean()
            loss.backward()
            res[on] = (loss.detach().cpu(), [None if p.grad is None else p.grad.detach().cpu().clone() for p in net.parameters()])
        assert any(a is not None for a in res[False][1])
        assert torch.equal(res[False][0], res[True][0])
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(res[False][1], res[True][1]))
    finally:
        net.precision, net.stem_split, net.stem_f16 = 4, True, False
        net.zero_grad(set_to_none=True)


def test_stem_split_uncovered_stems_keep_their_bits(golden):
    # the tokamak stem (Cin 12), a dim-8 net (Cout 8) and the Burgers stem (kD = 1, left coverage): switch on == switch off, bit for
    # bit, and no new call in the plan
    net, x, t, _ = _wide(golden, "tokamak")
    bnet, bx, bt, _ = _wide(golden, "burgers")
    g = golden("smoke_unet")
    small = _NETS["smoke"][0](8)
    small.load_state_dict(det_params(g.spec(), 300))
    small.to(DEV)
    for n, xx, tt in ((net, x, t), (small, g["x"].to(DEV), g["t"].to(DEV)), (bnet, bx, bt)):
        try:
            n.stem_split = False
            e0, c0 = n(xx, tt).clone(), _calls(n, xx)
            n.stem_split = True
            assert torch.equal(n(xx, tt), e0)
            assert _calls(n, xx) == c0 and "sdc_conv_stem_x3" not in c0
        finally:
            n.stem_split = True


def test_stem_split_sees_data_writes_to_the_stem_weight(golden):
    net, x, t, _ = _wide(golden, "smoke")
    make, dim, _, _ = _NETS["smoke"]
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    try:
        assert net.stem_split is True and "sdc_conv_stem_x3" in _calls(net, x)
        e0 = net(x, t).clone()
        net.init_conv.weight.data.mul_(1.5)
        e1 = net(x, t).clone()
        fresh = make(dim)
        fresh.load_state_dict(net.state_dict())
        fresh.to(DEV)
        assert torch.equal(fresh(x, t), e1) and not torch.equal(e1, e0)
    finally:
        net.load_state_dict(sd)
