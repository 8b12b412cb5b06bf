"""-m gpu: net.gemm_split (default on at precision >= 4, samplers only) -- the strided (1,4,4)/(1,2,2) convs, the 1x2x2 sub-pixel convs of the
transposed convs and the 1x1x1 convs as exact three-way bf16 operand splits on the bf16 matrix pipe (csrc/sdc_conv_gemm_x3.hip): fp32
in, fp32 accumulation, fp32 out.  Conv level, through the C ABI: the error against an exact-operand fp64 conv next to that of today's
fp32 kernel (sdc_conv at precision 4) on the same inputs, determinism, batch invariance, bias, power-of-two scaling invariance, the
device packer, the descriptors the kernel has no form for.  Net level: the eps-MSE contract gate against the reference fixture with the
default switches, the call list against the routing table, graph replay, and nothing else moves (switch off, precision 0 / 3,
fine-tuning, nets the table does not cover); a `.data` write to a routed conv's weight is seen by the next call."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import safediffcon_amd as sdc
from safediffcon_amd import _lib
from safediffcon_amd.engine import Plan, WeightSrc, conv_desc, pack_conv_weight, pack_gemm_x3
from oracle.detweights import det_params, det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SDC_EINVAL = -1


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


# form: (kind, B, Cin, Cout, D, (input H, W))
FORMS = {
    "strided_one_tile": ("a", 2, 64, 64, 2, (8, 32)),              # -> 4 x 16: exactly one 256-position tile
    "strided_ragged_odd_height": ("a", 3, 128, 128, 1, (6, 32)),   # -> 3 x 16: ragged last tile, odd plane height
    "strided_rows32_two_m_tiles": ("a", 1, 64, 128, 2, (4, 64)),   # -> 2 x 32
    "subpixel_128": ("b", 2, 128, 128, 2, (4, 16)),                # -> 8 x 32, all four parities
    "subpixel_64_odd_height": ("b", 1, 64, 64, 3, (3, 32)),        # -> 6 x 64
    "pw_256_384": ("c", 2, 256, 384, 2, (4, 16)),
    "pw_512_128_ragged": ("c", 1, 512, 128, 1, (5, 16)),           # ragged, longest K
    "pw_64_64_shortest_k": ("c", 2, 64, 64, 1, (2, 64)),           # K = 64: one final rounding dominates
}
_CASE = {}


def _launches(kind, w):
    """(Wp [taps * Cin][Cout], taps, stride, pad, output view of the full output) per launch of a form"""
    if kind == "a":
        return [(pack_conv_weight(w, "conv", 0), (1, 4, 4), (1, 2, 2), (0, 1, 1), lambda y: y)]
    if kind == "c":
        return [(pack_conv_weight(w, "conv", 0), (1, 1, 1), (1, 1, 1), (0, 0, 0), lambda y: y)]
    return [(pack_conv_weight(w, ("convT_sub", ph, pw), 0), (1, 2, 2), (1, 1, 1), (0, 1 - ph, 1 - pw),
             lambda y, ph=ph, pw=pw: y[:, :, :, ph::2, pw::2]) for ph in (0, 1) for pw in (0, 1)]


def _case(form):
    """inputs and the exact-operand fp64 reference (computed once per form, never modified)"""
    if form not in _CASE:
        kind, B, ci, co, D, (H, W) = FORMS[form]
        g = torch.Generator().manual_seed(13)
        x = torch.randn(B, ci, D, H, W, generator=g) * 2.0
        bias = 0.1 * torch.randn(co, generator=g)
        if kind == "a":
            w = torch.randn(co, ci, 1, 4, 4, generator=g) / (3.0 * (16 * ci) ** 0.5)
            ref = F.conv3d(x.double(), w.double(), stride=(1, 2, 2), padding=(0, 1, 1))
        elif kind == "b":
            w = torch.randn(ci, co, 1, 4, 4, generator=g) / (3.0 * (4 * ci) ** 0.5)      # nn.ConvTranspose3d weight
            ref = F.conv_transpose3d(x.double(), w.double(), stride=(1, 2, 2), padding=(0, 1, 1))
        else:
            w = torch.randn(co, ci, 1, 1, 1, generator=g) / (3.0 * ci ** 0.5)
            ref = F.conv3d(x.double(), w.double())
        ref = ref + bias.double().view(1, -1, 1, 1, 1)
        _CASE[form] = (x, w, bias, ref, ref.pow(2).mean().sqrt().item())
    return _CASE[form]


def _run(form, x_dev, wbs, bias, oshape):
    """the form's sdc_conv_gemm_x3 launches into a NaN-filled full output (bias: a tensor or None)"""
    lib = _lib.get_lib()
    kind, _, ci, co = FORMS[form][:4]
    y = torch.full((x_dev.shape[0], *oshape[1:]), float("nan"), device=DEV)
    for (wp, k, stride, pad, view), wb in zip(_launches(kind, _case(form)[1]), wbs):
        yv = view(y)
        d = conv_desc(x_dev, None, yv, None, co, k, stride, pad, (1, 1, 1), 0, 0)
        _lib.check(lib.sdc_conv_gemm_x3(C.byref(d), x_dev.data_ptr(), wb.data_ptr(), bias.data_ptr() if bias is not None else 0,
                                        yv.data_ptr(), _stream()), "sdc_conv_gemm_x3")
    torch.cuda.synchronize()
    return y


def _run_fp32(form, x_dev, bias, oshape):
    """today's kernel: sdc_conv at precision 4 on the same inputs and views"""
    lib = _lib.get_lib()
    kind, _, ci, co = FORMS[form][:4]
    y = torch.full(tuple(oshape), float("nan"), device=DEV)
    keep = []
    for wp, k, stride, pad, view in _launches(kind, _case(form)[1]):
        yv, wp = view(y), wp.to(DEV)
        keep.append(wp)
        d = conv_desc(x_dev, None, yv, None, co, k, stride, pad, (1, 1, 1), 0, 4)
        _lib.check(lib.sdc_conv(C.byref(d), x_dev.data_ptr(), 0, wp.data_ptr(), bias.data_ptr(), 0, yv.data_ptr(), _stream()), "sdc_conv")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("form", list(FORMS))
def test_gemm_x3_conv_is_fp32_grade(form):
    kind, B, ci, co, D, (H, W) = FORMS[form]
    x, w, bias, ref, rms = _case(form)
    lib = _lib.get_lib()
    # device packer == host packer, bit for bit, for every launch of the form
    wbs = []
    for wp, k, _, _, _ in _launches(kind, w):
        nbytes = int(lib.sdc_pack_gemm_x3_bytes(co, ci, k[1], k[2]))
        assert nbytes == 3 * k[1] * k[2] * ci * co * 2
        wb = torch.full((nbytes // 4,), float("nan"), device=DEV)
        wp_dev = wp.to(DEV)
        _lib.check(lib.sdc_pack_gemm_x3(wp_dev.data_ptr(), wb.data_ptr(), co, ci, k[1], k[2], _stream()), "sdc_pack_gemm_x3")
        torch.cuda.synchronize()
        assert torch.equal(wb.cpu().view(torch.int16), pack_gemm_x3(wp, co, ci, k).view(torch.int16))
        wbs.append(wb)

    x_dev, b_dev = x.to(DEV), bias.to(DEV)
    y = _run(form, x_dev, wbs, b_dev, ref.shape)
    out = y.double().cpu()
    assert torch.isfinite(out).all()              # (form b: the four parities together leave no NaN -- every element is written)
    # error against the exact-operand fp64 conv, rms over the whole output relative to the output rms, next to today's fp32 kernel's
    e_new = (out - ref).pow(2).mean().sqrt().item() / rms
    e_old = (_run_fp32(form, x_dev, b_dev, ref.shape).double().cpu() - ref).pow(2).mean().sqrt().item() / rms
    print(f"[measured] {form}: rms err vs exact fp64 (of the output rms): split {e_new:.3e} | fp32 kernel {e_old:.3e}")
    assert e_new <= max(1.25 * e_old, 2.0 ** -23), (e_new, e_old)
    if kind == "b":
        # each parity equals the transposed conv at that parity (to the same bound, the parity's own rms)
        for ph in (0, 1):
            for pw in (0, 1):
                o, r = out[:, :, :, ph::2, pw::2], ref[:, :, :, ph::2, pw::2]
                e_p = (o - r).pow(2).mean().sqrt().item() / r.pow(2).mean().sqrt().item()
                assert e_p <= 4.0 * max(1.25 * e_old, 2.0 ** -23), (ph, pw, e_p)        # (a wrong tap or parity gives e_p ~ 1)
    # two runs bit-identical; sample 0 of the batch == the same sample alone
    assert torch.equal(_run(form, x_dev, wbs, b_dev, ref.shape), y)
    if B > 1:
        assert torch.equal(_run(form, x_dev[:1], wbs, b_dev, ref.shape)[0], y[0])
    # without a bias
    y0 = _run(form, x_dev, wbs, None, ref.shape)
    assert torch.equal(y0 + b_dev.view(1, -1, 1, 1, 1), y)
    # power-of-two scaling of x scales the output bit for bit (a lost or flushed third piece would not)
    for e in (40, -40):
        ys = _run(form, x_dev * 2.0 ** e, wbs, None, ref.shape)
        assert torch.equal(ys, y0 * 2.0 ** e), e


def test_gemm_x3_uncovered_descriptors():
    lib = _lib.get_lib()
    x = torch.zeros(1, 64, 1, 4, 16, device=DEV)
    y = torch.full((1, 64, 1, 4, 16), float("nan"), device=DEV)
    wb = pack_gemm_x3(torch.zeros(64, 64), 64, 64, (1, 1)).to(DEV)
    ok = conv_desc(x, None, y, None, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), 0, 0)
    with_x1 = conv_desc(x, x, y, None, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), 0, 0)
    with_res = conv_desc(x, None, y, y, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), 0, 0)
    for d in (with_x1, with_res):
        assert lib.sdc_conv_gemm_x3_ok(C.byref(d)) == 0
        assert lib.sdc_conv_gemm_x3(C.byref(d), x.data_ptr(), wb.data_ptr(), 0, y.data_ptr(), _stream()) == SDC_EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(y).all()                   # nothing was launched
    # a conv whose GroupNorm sums the epilogue could carry keeps the fp32 kernels: the plan records no split call for it
    plan = Plan(DEV, precision=4, gemm_split=True)
    plan.conv(x, WeightSrc(torch.zeros(64, 64, 1, 1, 1, device=DEV)), None, 64, (1, 1, 1), gn_groups=8)
    assert [fn.__name__ for fn, _ in plan.calls if "conv" in fn.__name__][0] in ("sdc_conv", "sdc_conv_gn")
    # (the covered descriptor runs)
    _lib.check(lib.sdc_conv_gemm_x3(C.byref(ok), x.data_ptr(), wb.data_ptr(), 0, y.data_ptr(), _stream()), "sdc_conv_gemm_x3")
    torch.cuda.synchronize()
    assert (y == 0).all()


# ------------------------------------------------------------------ net level
_NETS = {
    "smoke": (lambda d: sdc.Unet3D_with_Conv3D(dim=d, dim_mults=(1, 2, 4), channels=7), 64, (1, 32, 7, 32, 32), 300),
    "burgers": (lambda d: sdc.Unet2D(dim=d, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1), 64, (2, 3, 16, 128), 100),
    "tokamak": (lambda d: sdc.Unet1D(dim=d, dim_mults=(1, 2, 4, 8), channels=12, resnet_block_groups=1), 256, (2, 12, 128), 200),
}
_WIDE = {}
NEW = "sdc_conv_gemm_x3"


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


def _prod(golden):
    """the same smoke net on one sample at the production plane size (64 x 64, the sizes the routing table was measured at)"""
    net, _, t, _ = _wide(golden, "smoke")
    return net, det_tensor((1, 32, 7, 64, 64), 41).to(DEV), t


def _plan(net, x):
    return net.entry(tuple(x.shape), x.shape[0])["plan"]


def _calls(net, x):
    return [fn.__name__ for fn, _ in _plan(net, x).calls]


def _table_count(net, x):
    """how many convs of the switch-off plan the routing table lists: plain sdc_conv calls (no GroupNorm sums, no split-K) whose
    descriptor sdc_conv_gemm_x3_ok accepts (it refuses a second input and a residual by itself)"""
    lib = _lib.get_lib()
    on = net.gemm_split
    try:
        net.gemm_split = False
        return sum(1 for fn, a in _plan(net, x).calls if fn.__name__ == "sdc_conv" and lib.sdc_conv_gemm_x3_ok(a[0]))
    finally:
        net.gemm_split = on


def test_gemm_split_smoke_net_against_reference_fixture(golden):
    net, x, t, ref = _wide(golden, "smoke")
    assert net.precision == 4 and net.gemm_split is True and net.stem_split is True          # the defaults
    net.forward_graph = True
    eps = net(x, t).cpu()
    mse = ((eps - ref) ** 2).mean().item()
    n_new, n_table = _calls(net, x).count(NEW), _table_count(net, x)
    print(f"[measured] smoke_unet_wide precision 4, default gemm_split: eps-MSE {mse:.3e}  max|err| {(eps - ref).abs().max().item():.3e}; "
          f"{n_new} split calls, the table lists {n_table}")
    assert torch.isfinite(eps).all()
    assert mse <= 1e-5
    assert n_new == n_table
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


def test_gemm_split_off_on_off_precisions_and_fine_tuning(golden):
    net, x, t = _prod(golden)
    try:
        net.gemm_split = False
        e0 = net(x, t).clone()
        assert NEW not in _calls(net, x)
        net.gemm_split = True
        e1 = net(x, t).clone()
        routed = _calls(net, x).count(NEW)
        assert routed == _table_count(net, x)
        net.gemm_split = False
        assert torch.equal(net(x, t), e0) and NEW not in _calls(net, x)
        assert torch.equal(e1, e0) == (routed == 0)
        # precision 0 and 3: the literal fp32 pipe, whatever the switch says
        for prec in (0, 3):
            net.precision = prec
            res = {}
            for on in (False, True):
                net.gemm_split = on
                res[on] = (net(x, t).clone(), _calls(net, x))
            assert torch.equal(res[False][0], res[True][0]) and res[False][1] == res[True][1]
            assert NEW not in res[True][1]
        net.precision = 4
        # forward_train: loss and every gradient bit-identical with the switch on and off
        res = {}
        for on in (False, True):
            net.gemm_split = on
            net.zero_grad(set_to_none=True)
            loss = (net.forward_train(x, t) ** 2).mean()
            loss.backward()
            res[on] = (loss.detach().cpu(), [None if p.grad is None else p.grad.detach().cpu().clone() for p in net.parameters()])
        assert any(a is not None for a in res[False][1])
        assert torch.equal(res[False][0], res[True][0])
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(res[False][1], res[True][1]))
    finally:
        net.precision, net.gemm_split = 4, True
        net.zero_grad(set_to_none=True)


def test_gemm_split_uncovered_nets_keep_their_bits(golden):
    # the tokamak net, a dim-8 smoke net (Cout 8 .. 32) and, where the table routes none of its convs, the Burgers net: switch on ==
    # switch off, bit for bit, and no new call in the plan
    net, x, t, _ = _wide(golden, "tokamak")
    g = golden("smoke_unet")
    small = _NETS["smoke"][0](8)
    small.load_state_dict(det_params(g.spec(), 300))
    small.to(DEV)
    nets = [(net, x, t), (small, g["x"].to(DEV), g["t"].to(DEV))]
    bnet, bx, bt, _ = _wide(golden, "burgers")
    if _table_count(bnet, bx) == 0:
        nets.append((bnet, bx, bt))
    for n, xx, tt in nets:
        assert _table_count(n, xx) == 0
        try:
            n.gemm_split = False
            e0, c0 = n(xx, tt).clone(), _calls(n, xx)
            n.gemm_split = True
            assert torch.equal(n(xx, tt), e0)
            assert _calls(n, xx) == c0 and NEW not in c0
        finally:
            n.gemm_split = True


def test_gemm_split_sees_data_writes_to_a_routed_weight(golden):
    net, x, t = _prod(golden)
    make, dim, _, _ = _NETS["smoke"]
    plan = _plan(net, x)
    routed = [a for fn, a in plan.calls if fn.__name__ == NEW]
    assert routed
    # the parameter behind the first routed conv: the one whose host pack is that call's buffer
    buf = next(w for w, _ in plan.repackers if w.data_ptr() == routed[0][2]).cpu().view(torch.int32)
    name = None
    for n, p in net.named_parameters():
        w = p.detach().cpu()
        if w.dim() != 5 or w.shape[2] != 1 or tuple(w.shape[3:]) not in ((4, 4), (1, 1)):
            continue
        cands = [("conv", w.shape[0], w.shape[1], tuple(w.shape[3:]))]
        if tuple(w.shape[3:]) == (4, 4):
            cands += [(("convT_sub", ph, pw), w.shape[1], w.shape[0], (2, 2)) for ph in (0, 1) for pw in (0, 1)]
        for kind, co, ci, k in cands:
            if 3 * k[0] * k[1] * ci * co // 2 == buf.numel() and co % 64 == 0 and ci % 64 == 0 and \
                    torch.equal(pack_gemm_x3(pack_conv_weight(w, kind, 0), co, ci, k).view(torch.int32), buf):
                name = n
    assert name is not None
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    try:
        e0 = net(x, t).clone()
        dict(net.named_parameters())[name].data.mul_(1.5)
        e1 = net(x, t).clone()
        fresh = make(dim)
        fresh.load_state_dict(net.state_dict())
        fresh.to(DEV)
        assert torch.equal(fresh(x, t), e1) and not torch.equal(e1, e0)
    finally:
        net.load_state_dict(sd)
