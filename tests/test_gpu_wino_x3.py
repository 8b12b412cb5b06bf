"""-m gpu: net.wino_split -- the 3x3x3 convs over rows of 16 as Winograd F(2x2x2,3x3x3) with exact three-way bf16 splits of the transformed
operands on the bf16 matrix pipe (csrc/sdc_conv_wino_x3.hip): fp32 in, fp32 accumulation, fp32 out.  Conv level, through the C ABI (so
small shapes outside the routing table are pinned): the error against an exact-operand fp64 conv next to that of today's fp32 kernel
(sdc_conv at precision 4) on the same inputs, the GroupNorm epilogue through gn_silu, the second input, depth clipping, determinism, batch
invariance, power-of-two scaling invariance, the device packer, the descriptors the kernel has no form for.  Every launch is replayed: y is
scratch while the kernel runs (the fold parks m1 in plane 1).  Net level: the eps-MSE contract gate against the reference fixture at the
default switches, the call list against the routing table, graph replay, off -> on -> off, a `.data` write to a routed weight."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import safediffcon_amd as sdc
from safediffcon_amd import _lib
from safediffcon_amd.engine import Plan, WeightSrc, conv_desc, pack_conv_weight, pack_wino3_x3
from oracle.detweights import det_params, det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SDC_EINVAL = -1
NEW = "sdc_conv_wino3_x3"


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


# form: (B, Cin0, Cin1, Cout, (D, H, W), GroupNorm groups)
FORMS = {
    "one_workgroup_two_stages": (1, 32, 0, 64, (2, 16, 16), 0),
    "odd_stages_batch_and_depth_walk": (2, 48, 0, 64, (4, 16, 16), 0),
    "two_channel_tiles_gn": (1, 32, 0, 128, (2, 16, 16), 8),
    "two_inputs_gn": (2, 16, 16, 64, (2, 16, 16), 8),
    "depth_clips_both_ends": (1, 16, 0, 64, (2, 16, 16), 0),
}
_CASE = {}


def _case(form):
    """inputs and the exact-operand fp64 reference (computed once per form, never modified)"""
    if form not in _CASE:
        B, c0, c1, co, sp, G = FORMS[form]
        g = torch.Generator().manual_seed(29)
        x = torch.randn(B, c0 + c1, *sp, generator=g) * 2.0
        w = torch.randn(co, c0 + c1, 3, 3, 3, generator=g) / (3.0 * (27 * (c0 + c1)) ** 0.5)
        bias = 0.1 * torch.randn(co, generator=g)
        ref = F.conv3d(x.double(), w.double(), padding=1) + bias.double().view(1, -1, 1, 1, 1)
        _CASE[form] = (x, w, bias, ref)
    return _CASE[form]


def _inputs(form, x):
    """the one or two (channel-concatenated) device inputs of a form, each contiguous"""
    c0, c1 = FORMS[form][1:3]
    x0 = x[:, :c0].contiguous().to(DEV)
    return x0, (x[:, c0:].contiguous().to(DEV) if c1 else None)


def _pack_dev(wp4_dev, co, ci):
    lib = _lib.get_lib()
    nbytes = int(lib.sdc_pack_wino3_x3_bytes(co, ci))
    assert nbytes == 3 * 64 * ci * co * 2
    wb = torch.full((nbytes // 4,), float("nan"), device=DEV)
    _lib.check(lib.sdc_pack_wino3_x3(wp4_dev.data_ptr(), wb.data_ptr(), co, ci, _stream()), "sdc_pack_wino3_x3")
    torch.cuda.synchronize()
    return wb


def _run(x0, x1, wb, bias, co, parts=None, G=0, replays=2):
    """sdc_conv_wino3_x3 into a NaN-filled output, replayed: a replay starts from y holding the previous result"""
    lib = _lib.get_lib()
    y = torch.full((x0.shape[0], co, *x0.shape[2:]), float("nan"), device=DEV)
    d = conv_desc(x0, x1, y, None, co, (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, 4)
    for _ in range(replays):
        _lib.check(lib.sdc_conv_wino3_x3(C.byref(d), x0.data_ptr(), x1.data_ptr() if x1 is not None else 0, wb.data_ptr(),
                                         bias.data_ptr() if bias is not None else 0, y.data_ptr(),
                                         parts.data_ptr() if parts is not None else 0, G, _stream()), NEW)
    torch.cuda.synchronize()
    return y


def _run_fp32(x0, x1, wp4, bias, co):
    """today's kernel: sdc_conv at precision 4 on the same inputs"""
    lib = _lib.get_lib()
    y = torch.full((x0.shape[0], co, *x0.shape[2:]), float("nan"), device=DEV)
    d = conv_desc(x0, x1, y, None, co, (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, 4)
    name = C.create_string_buffer(128)
    _lib.check(lib.sdc_conv_describe(C.byref(d), name, 128, None), "sdc_conv_describe")
    assert name.value.decode().startswith("conv_wg3")
    for _ in range(2):
        _lib.check(lib.sdc_conv(C.byref(d), x0.data_ptr(), x1.data_ptr() if x1 is not None else 0, wp4.data_ptr(), bias.data_ptr(), 0,
                                y.data_ptr(), _stream()), "sdc_conv")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("form", list(FORMS))
def test_wino_x3_conv_is_fp32_grade(form):
    B, c0, c1, co, sp, G = FORMS[form]
    ci = c0 + c1
    x, w, bias, ref = _case(form)
    lib = _lib.get_lib()
    wp4 = pack_conv_weight(w, "conv", 4)
    wp4_dev = wp4.to(DEV)
    # device packer == host packer, bit for bit
    wb = _pack_dev(wp4_dev, co, ci)
    assert torch.equal(wb.cpu().view(torch.int16), pack_wino3_x3(wp4, co, ci).view(torch.int16))

    x0, x1 = _inputs(form, x)
    b_dev = bias.to(DEV)
    y = _run(x0, x1, wb, b_dev, co)
    out = y.double().cpu()
    assert torch.isfinite(out).all()
    rms, scale = ref.pow(2).mean().sqrt().item(), ref.abs().max().item()
    e_new = (out - ref).pow(2).mean().sqrt().item() / rms
    e_old = (_run_fp32(x0, x1, wp4_dev, b_dev, co).double().cpu() - ref).pow(2).mean().sqrt().item() / rms
    e_max = (out - ref).abs().max().item() / scale
    print(f"[measured] {form}: rms err vs exact fp64 (of the output rms): split {e_new:.3e} | fp32 kernel {e_old:.3e}; "
          f"max |err| of the output scale {e_max:.3e}")
    assert e_new <= max(1.25 * e_old, 2.0 ** -23), (e_new, e_old)
    assert e_max < 1e-5, e_max
    # two runs bit-identical (one launch == two launches: nothing of the previous result survives)
    assert torch.equal(_run(x0, x1, wb, b_dev, co, replays=1), y)
    # a sample alone == the same sample as batch mate of three others
    xs = torch.cat([x[:1], x[:1].flip(-1), x[:1] * 0.5, x[:1].flip(-2)])
    q0, q1 = _inputs(form, xs)
    assert torch.equal(_run(q0, q1, wb, b_dev, co)[0], _run(x0[:1], None if x1 is None else x1[:1], wb, b_dev, co)[0])
    # power-of-two scaling of x and the bias scales the output bit for bit (a lost or flushed third piece would not)
    for e in (40, -40):
        s = 2.0 ** e
        ys = _run(x0 * s, None if x1 is None else x1 * s, wb, b_dev * s, co)
        assert torch.equal(ys, y * s), e
    # without a bias: the start value of component (1, 1) is zero
    y0 = _run(x0, x1, wb, None, co).double().cpu()
    assert ((y0 + bias.double().view(1, -1, 1, 1, 1) - ref).abs().max().item() / scale) < 1e-5
    if G:
        # the GroupNorm sums of the epilogue, finished by gn_silu (which then skips its statistics pass), against torch in fp64
        nparts = int(lib.sdc_conv_gnparts(C.byref(conv_desc(x0, x1, y, None, co, (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, 4)), G))
        assert nparts > 0
        parts = torch.full((B * G * nparts * 2,), float("nan"), dtype=torch.float64, device=DEV)
        yg = _run(x0, x1, wb, b_dev, co, parts=parts, G=G)
        assert torch.equal(yg, y) and torch.isfinite(parts).all()
        gam, bet = det_tensor((co,), 296, 0.3) + 1.0, det_tensor((co,), 297, 0.2)
        plan = Plan(DEV, precision=4)
        plan._gn_parts[yg.data_ptr()] = (parts, nparts, G)
        z = plan.gn_silu(yg, gam.to(DEV), bet.to(DEV), G, out=torch.empty_like(yg))
        assert [fn.__name__ for fn, _ in plan.calls] == ["sdc_gn_finalize", "sdc_gn_apply"]
        plan.run(_stream())
        torch.cuda.synchronize()
        refn = F.silu(F.group_norm(ref, G, gam.double(), bet.double(), 1e-5))
        torch.testing.assert_close(z.cpu().double(), refn, rtol=1e-4, atol=2e-5)


def test_wino_x3_uncovered_descriptors():
    lib = _lib.get_lib()
    wb = torch.zeros(3 * 64 * 32 * 128 // 2, device=DEV)

    def desc(ci, co, D, res=False):
        x = torch.zeros(1, ci, D, 16, 16, device=DEV)
        y = torch.full((1, co, D, 16, 16), float("nan"), device=DEV)
        return x, y, conv_desc(x, None, y, y if res else None, co, (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, 4)

    for ci, co, D, res in ((24, 64, 2, False), (32, 64, 3, False), (32, 96, 2, False), (32, 64, 2, True)):
        x, y, d = desc(ci, co, D, res)
        assert lib.sdc_conv_wino3_x3_ok(C.byref(d)) == 0
        assert lib.sdc_conv_wino3_x3(C.byref(d), x.data_ptr(), 0, wb.data_ptr(), 0, y.data_ptr(), 0, 0, _stream()) == SDC_EINVAL
        torch.cuda.synchronize()
        assert torch.isnan(y).all()               # nothing was launched
    # (the covered descriptor runs: zero weights, no bias)
    x, y, d = desc(32, 64, 2)
    _lib.check(lib.sdc_conv_wino3_x3(C.byref(d), x.data_ptr(), 0, wb.data_ptr(), 0, y.data_ptr(), 0, 0, _stream()), NEW)
    torch.cuda.synchronize()
    assert (y == 0).all()


# ------------------------------------------------------------------ net level
_WIDE = {}


def _wide(golden):
    """the production-width smoke net with its fixture's weights, input and reference eps (built once)"""
    if not _WIDE:
        g = golden("smoke_unet_wide")
        net = sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7)
        net.load_state_dict(det_params(g.spec(), int(g.scalar("weight_seed"))))
        net.to(DEV)
        _WIDE["smoke"] = (net, det_tensor((1, 32, 7, 32, 32), int(g.scalar("x_seed"))).to(DEV), g["t"].to(DEV), g["eps"])
    return _WIDE["smoke"]


def _prod(golden):
    """the same net on one sample at the production plane size (64 x 64: the sizes the routing table was measured at)"""
    net, _, t, _ = _wide(golden)
    return net, det_tensor((1, 32, 7, 64, 64), 41).to(DEV), t


def _plan(net, x):
    return net.entry(tuple(x.shape), x.shape[0])["plan"]


def _calls(net, x):
    return [fn.__name__ for fn, _ in _plan(net, x).calls]


def _table_count(net, x):
    """how many convs of the switch-off plan the routing table lists: sdc_conv / sdc_conv_gn calls without a residual whose descriptor
    sdc_conv_wino3_x3_ok accepts"""
    lib = _lib.get_lib()
    on = net.wino_split
    try:
        net.wino_split = False
        return sum(1 for fn, a in _plan(net, x).calls
                   if fn.__name__ in ("sdc_conv", "sdc_conv_gn") and a[5] == 0 and lib.sdc_conv_wino3_x3_ok(a[0]))
    finally:
        net.wino_split = on


def test_wino_split_smoke_net_against_reference_fixture(golden):
    net, x, t, ref = _wide(golden)
    assert net.precision == 4
    net.forward_graph = True
    eps = net(x, t).cpu()
    mse = ((eps - ref) ** 2).mean().item()
    n_new, n_table = _calls(net, x).count(NEW), _table_count(net, x)
    print(f"[measured] smoke_unet_wide precision 4, default switches (wino_split {net.wino_split}): eps-MSE {mse:.3e}  "
          f"max|err| {(eps - ref).abs().max().item():.3e}; {n_new} wino split calls, the table lists {n_table}")
    assert torch.isfinite(eps).all()
    assert mse <= 1e-5
    assert n_new == (n_table if net.wino_split else 0)
    # one 16 x 16-level conv of a 64 x 64 sample (256 -> 256 at 32 x 16 x 16) through a Plan with the switch on: the plan holds the new
    # call exactly where the table lists the shape, and the result is that of the fp32 kernel to fp32 grade
    lib = _lib.get_lib()
    w = det_tensor((256, 256, 3, 3, 3), 61, 1.0 / (27 * 256) ** 0.5)
    xx = det_tensor((1, 256, 32, 16, 16), 62).to(DEV)
    outs = {}
    for on in (False, True):
        plan = Plan(DEV, precision=4, wino_split=on)
        y = plan.conv(xx, WeightSrc(w), None, 256, (3, 3, 3), pad=(1, 1, 1), gn_groups=8)
        z = plan.gn_silu(y, torch.ones(256, device=DEV), torch.zeros(256, device=DEV), 8, out=torch.empty_like(y))
        names = [fn.__name__ for fn, _ in plan.calls]
        listed = bool(lib.sdc_conv_wino3_x3_ok(plan.calls[0][1][0]))
        assert names == ([NEW] if on and listed else ["sdc_conv_gn"]) + ["sdc_gn_finalize", "sdc_gn_apply"], names
        for _ in range(2):
            plan.run(_stream())
        torch.cuda.synchronize()
        outs[on] = (y.clone(), z.clone())
    assert Plan(DEV, precision=4).wino_split is False and Plan(DEV, precision=3, wino_split=True).wino_split is False
    scale = outs[False][0].abs().max().item()
    assert (outs[True][0] - outs[False][0]).abs().max().item() < 2e-5 * scale
    torch.testing.assert_close(outs[True][1], outs[False][1], rtol=2e-4, atol=4e-5)


def test_wino_split_graph_replay_and_off_on_off(golden):
    net, x, t = _prod(golden)
    was = net.wino_split
    try:
        net.wino_split = False
        e0 = net(x, t).clone()
        c0 = _calls(net, x)
        assert NEW not in c0
        net.wino_split = True
        net.forward_graph = True
        e1 = net(x, t).clone()
        routed = _calls(net, x).count(NEW)
        assert routed == _table_count(net, x)
        print(f"[measured] smoke net, one 64 x 64 sample: {routed} wino split calls; max |eps on - eps off| {(e1 - e0).abs().max().item():.3e}")
        # graph replay == eager call list, two runs bit-identical
        try:
            net.forward_graph = False
            eager = net(x, t).clone()
        finally:
            net.forward_graph = True
        assert torch.equal(eager, e1) and torch.equal(net(x, t), e1)
        net.wino_split = False
        assert torch.equal(net(x, t), e0) and _calls(net, x) == c0
        assert torch.equal(e1, e0) == (routed == 0)
        # precision 0, 3 and 6: today's calls, whatever the switch says
        for prec in (0, 3, 6):
            net.precision = prec
            res = {}
            for on in (False, True):
                net.wino_split = on
                res[on] = (net(x, t).clone(), _calls(net, x))
            assert torch.equal(res[False][0], res[True][0]) and res[False][1] == res[True][1]
            assert NEW not in res[True][1]
    finally:
        net.precision, net.wino_split = 4, was


def test_wino_split_sees_data_writes_to_a_routed_weight(golden):
    net, x, t = _prod(golden)
    was = net.wino_split
    try:
        net.wino_split = True
        plan = _plan(net, x)
        routed = [a for fn, a in plan.calls if fn.__name__ == NEW]
        assert len(routed) == _table_count(net, x)
        if not routed:
            return                                # (an empty table: the switch routes nothing, there is no routed weight to write to)
        # the parameter behind the first routed conv: the one whose host pack is that call's buffer
        buf = next(w for w, _ in plan.repackers if w.data_ptr() == routed[0][3]).cpu().view(torch.int32)
        name = None
        for n, p in net.named_parameters():
            w = p.detach().cpu()
            if w.dim() == 5 and tuple(w.shape[2:]) == (3, 3, 3) and w.shape[0] % 64 == 0 and w.shape[1] % 16 == 0 and \
                    3 * 64 * w.shape[0] * w.shape[1] // 2 == buf.numel() and \
                    torch.equal(pack_wino3_x3(pack_conv_weight(w, "conv", 4), w.shape[0], w.shape[1]).view(torch.int32), buf):
                name = n
        assert name is not None
        sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
        try:
            e0 = net(x, t).clone()
            dict(net.named_parameters())[name].data.mul_(1.5)
            e1 = net(x, t).clone()
            fresh = sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7)
            fresh.load_state_dict(net.state_dict())
            fresh.to(DEV)
            fresh.wino_split = True
            assert torch.equal(fresh(x, t), e1) and not torch.equal(e1, e0)
        finally:
            net.load_state_dict(sd)
    finally:
        net.wino_split = was
