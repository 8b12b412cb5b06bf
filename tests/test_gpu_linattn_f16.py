"""-m gpu: net.linattn_f16 (opt-in, samplers only) -- the fused LinearAttention block at width 64 / 128 on the fp16 matrix pipe
(csrc/sdc_lablock_f16.hip): fp16 operands (RNE), fp32 accumulation.  Block level, through the C ABI, on the inputs of
test_linear_attention_block_fused: against an fp64 emulation that rounds at exactly the kernel's five rounding points and against the
exact fp64 block, NaN pre-fill, determinism, batch invariance, the device packer, the GroupNorm-on-load form.  Net level: the eps-MSE
contract gate against the reference fixtures, the call list, graph replay, batch invariance; and nothing else moves (switch off,
fine-tuning, a net without a fused site, the unfused chain keep their bits); a `.data` write to a to_qkv weight is seen by the next
call."""
import pytest
import torch

import safediffcon_amd as sdc
from safediffcon_amd import _lib
from safediffcon_amd.engine import Plan, pack_conv_weight, pack_linattn_f16
from oracle.detweights import det_params, det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG2E = 1.4426950408889634

# (outer, inner, C, n, pre_mode, post_mode, tokens permuted)
SHAPES = [
    (2, 1, 64, 64, 0, 0, False),        # one tile
    (2, 3, 64, 256, 0, -1, False),      # inner stride
    (2, 1, 64, 128, 1, 1, False),       # RMSNorm
    (5, 1, 128, 128, 0, 0, False),      # C = 128
    (2, 2, 64, 1088, 0, -1, False),     # 17 tiles: uneven splits 9 + 8
    (1, 2, 128, 1024, 0, -1, False),    # C = 128, two splits
    (1, 1, 64, 4096, 0, -1, False),     # 8 splits
    (2, 2, 64, 1088, 0, -1, True),      # row d = 0 of head 0's k ascends along the sequence: the running maximum moves in every tile
]
# kernel vs emulation, rms over the tensor relative to the rms of the branch y - x: 5 x the worst value measured on the MI355X over
# SHAPES (7.2e-5 at (1, 2, 128, 1024); 2.7e-5 - 5.9e-5 on the others: the fp32 accumulation and the fp32 exponent now and then flip
# an fp16 rounding of the fp64 emulation), and never above a third of the shape's e_in (emulation vs exact, 7.8e-4 - 1.04e-3): a
# dropped rounding point or a wrong fragment does not pass.  Every measured value is below e_in / 5.
GATE_EMU = 3.6e-4
_CASE = {}


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _norm(t, g, mode, Cc, eps=1e-5):          # over the channel axis (dim 1)
    if mode == 0:
        return (t - t.mean(1, keepdim=True)) * (t.var(1, unbiased=False, keepdim=True) + eps).rsqrt() * g.view(1, -1, 1, 1)
    return torch.nn.functional.normalize(t, dim=1) * g.view(1, -1, 1, 1) * Cc ** 0.5


def _inputs(outer, inner, Cc, n, pre, post, permuted):
    x = det_tensor((outer, Cc, inner, n), 111)
    g1, g2 = det_tensor((Cc,), 112, 0.3) + 1.0, det_tensor((Cc,), 113, 0.3) + 1.0
    wqkv, wo, bo = det_tensor((384, Cc), 114, 0.4), det_tensor((Cc, 128), 115, 0.3), det_tensor((Cc,), 116, 0.1)
    if permuted:
        # the channel norm is per token: permuting the tokens of a sequence permutes its k rows
        k0 = torch.einsum("c,bcfn->bfn", wqkv[128].double(), _norm(x.double(), g1.double(), pre, Cc))
        order = k0.argsort(-1)[:, None].expand(outer, Cc, inner, n)
        x = x.gather(-1, order).contiguous()
    return x, g1, g2, wqkv, wo, bo


def _branch(x, g1, g2, wqkv, wo, bo, pre, post, r):
    """the attention branch y - x = post(Wo LA(pre(x)) + bo) in fp64 (1D/model/unet.py:182-222, conv3d.py:232-258); r rounds an operand
    of a matrix product: the identity for the exact block, .half().double() for the emulation of sdc_linattn_block_f16 -- xn, Wq and Wk,
    the un-normalised probabilities p = exp2(k log2e - ceil(max k log2e)) (the row sum is of the unrounded p), T = Wo ctx, q after its
    softmax and scale"""
    B, Cc, Fr, n = x.shape
    xn = r(_norm(x.double(), g1.double(), pre, Cc))
    w = wqkv.double()
    q = torch.einsum("oc,bcfn->bofn", r(w[:128]), xn).reshape(B, 4, 32, Fr, n)
    k = torch.einsum("oc,bcfn->bofn", r(w[128:256]), xn).reshape(B, 4, 32, Fr, n)
    v = torch.einsum("oc,bcfn->bofn", w[256:], xn).reshape(B, 4, 32, Fr, n)
    p = torch.exp2(k * LOG2E - (k.amax(-1, keepdim=True) * LOG2E).ceil())
    ctx = torch.einsum("bhdfn,bhefn->bhfde", r(p), v) / p.sum(-1).permute(0, 1, 3, 2)[..., None]
    T = r(torch.einsum("cme,bmfde->bfcmd", wo.double().reshape(Cc, 4, 32), ctx))          # T[co][head, d] per sequence
    q = r(q.softmax(2) * 32 ** -0.5)
    y = torch.einsum("bfcmd,bmdfn->bcfn", T, q) + bo.double().view(1, -1, 1, 1)
    return _norm(y, g2.double(), post, Cc) if post >= 0 else y


def _case(shape):
    """inputs and the two fp64 references of a shape (computed once, never modified), with the CPU-side check of the inputs"""
    if shape not in _CASE:
        inp = _inputs(*shape)
        pre, post = shape[4], shape[5]
        exact = _branch(*inp, pre, post, lambda t: t)
        emu = _branch(*inp, pre, post, lambda t: t.half().double())
        rms = exact.pow(2).mean().sqrt().item()
        assert torch.isfinite(emu).all()
        # the emulation alone sits at 7.7e-4 - 1.0e-3 of the branch rms from the exact block on these inputs: the gates below then test
        # the kernel and not the inputs
        e_in = (emu - exact).pow(2).mean().sqrt().item() / rms
        assert 6.0e-4 <= e_in <= 1.3e-3, e_in
        _CASE[shape] = (inp, exact, emu, rms, e_in)
    return _CASE[shape]


def _dev_weights(wqkv, wo, Cc):
    """the fp32 packed weights of sdc_linattn_block and the fp16 buffer, written by the device packer onto NaN"""
    lib = _lib.get_lib()
    pq = pack_conv_weight(wqkv.view(384, Cc, 1)).to(DEV)
    po = pack_conv_weight(wo.view(Cc, 128, 1)).to(DEV)
    wpk = torch.full((int(lib.sdc_pack_linattn_f16_bytes(Cc)) // 4,), float("nan"), device=DEV)
    wq_d, wo_d = wqkv.to(DEV), wo.to(DEV)
    _lib.check(lib.sdc_pack_linattn_f16(wq_d.data_ptr(), wo_d.data_ptr(), Cc, wpk.data_ptr(), _stream()), "sdc_pack_linattn_f16")
    torch.cuda.synchronize()
    return pq, po, wpk


def _run(x_dev, g1, pq, po, wpk, bo, g2, pre, post):
    """one sdc_linattn_block_f16 call on a NaN-filled output: x (outer, C, inner, n)"""
    lib = _lib.get_lib()
    outer, Cc, inner, n = x_dev.shape
    y = torch.full_like(x_dev, float("nan"))
    work = torch.full(((int(lib.sdc_linattn_block_f16_bytes(outer, inner, Cc, n)) + 3) // 4,), float("nan"), device=DEV)
    _lib.check(lib.sdc_linattn_block_f16(x_dev.data_ptr(), g1.data_ptr(), pq.data_ptr(), po.data_ptr(), wpk.data_ptr(), bo.data_ptr(),
                                         g2.data_ptr() if post >= 0 else None, work.data_ptr(), y.data_ptr(), outer, inner, Cc, n,
                                         Cc * inner * n, inner * n, n, pre, post, 1e-5, _stream()), "sdc_linattn_block_f16")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:6])) + ("-ascending" if s[6] else ""))
def test_linattn_f16_block_rounds_where_documented(shape):
    (x, g1, g2, wqkv, wo, bo), exact, emu, rms, e_in = _case(shape)
    outer, inner, Cc, n, pre, post, _ = shape
    pq, po, wpk = _dev_weights(wqkv, wo, Cc)
    # device packer == host packer, bit for bit
    assert torch.equal(wpk.cpu().view(torch.int16), pack_linattn_f16(wqkv, wo).view(torch.int16))
    dev = [t.to(DEV) for t in (g1, bo, g2)]
    x_dev = x.to(DEV)
    y = _run(x_dev, dev[0], pq, po, wpk, dev[1], dev[2], pre, post)
    assert torch.isfinite(y).all()
    got = y.cpu().double() - x.double()
    e_emu = (got - emu).pow(2).mean().sqrt().item() / rms
    e_x = (got - exact).pow(2).mean().sqrt().item() / rms
    print(f"[measured] {shape}: rms err vs fp64 emulation {e_emu:.2e}, vs exact fp64 {e_x:.2e} (of the rms of the attention branch; "
          f"the emulation itself: {e_in:.2e})")
    assert e_x <= 2 * e_in, (e_x, e_in)
    assert e_emu <= min(GATE_EMU, e_in / 3), (e_emu, e_in)
    # two runs bit-identical
    assert torch.equal(_run(x_dev, dev[0], pq, po, wpk, dev[1], dev[2], pre, post), y)


@pytest.mark.parametrize("shape", [(3, 2, 64, 1088, 0, -1), (3, 1, 128, 128, 0, 0)], ids=lambda s: "x".join(map(str, s)))
def test_linattn_f16_block_is_batch_invariant(shape):
    """a sample's output is bit-identical alone (outer = 1) and inside outer = 3"""
    outer, inner, Cc, n, pre, post = shape
    x, g1, g2, wqkv, wo, bo = _inputs(*shape, False)
    pq, po, wpk = _dev_weights(wqkv, wo, Cc)
    dev = [t.to(DEV) for t in (g1, bo, g2)]
    x_dev = x.to(DEV)
    y = _run(x_dev, dev[0], pq, po, wpk, dev[1], dev[2], pre, post)
    assert torch.isfinite(y).all()
    for b in range(outer):
        assert torch.equal(_run(x_dev[b:b + 1].contiguous(), dev[0], pq, po, wpk, dev[1], dev[2], pre, post)[0], y[b]), b


@pytest.mark.parametrize("Cc,F_,hw,res", [(64, 3, (16, 16), True), (128, 2, (8, 16), True), (64, 1, (8, 8), False)])
def test_linattn_f16_block_with_groupnorm_on_load(Cc, F_, hw, res):
    """sdc_linattn_block_gn_f16 == sdc_gn_stats + sdc_gn_apply followed by sdc_linattn_block_f16, bit for bit (the shapes and inputs of
    test_linattn_block_with_groupnorm_on_load)"""
    B, G = 2, 8
    H, W = hw
    x = det_tensor((B, Cc, F_, H, W), 501).to(DEV)
    r = det_tensor((B, Cc, F_, H, W), 502).to(DEV) if res else None
    gam, bet = (1 + 0.2 * det_tensor((Cc,), 503)).to(DEV), (0.1 * det_tensor((Cc,), 504)).to(DEV)
    g_pre = (1 + 0.1 * det_tensor((Cc,), 505)).to(DEV)
    uq, uo = det_tensor((384, Cc, 1, 1), 506, 0.1).to(DEV), det_tensor((Cc, 128, 1, 1), 507, 0.1).to(DEV)
    outs = []
    for fused in (True, False):
        plan = Plan(DEV, linattn_f16=True)
        wqkv, wo = plan.conv_weight(uq), plan.conv_weight(uo)
        bo = (0.1 * det_tensor((Cc,), 508)).to(DEV)
        xx = x.clone()
        n = H * W
        strides = (Cc * F_ * n, F_ * n, n)
        if fused:
            st = plan.gn_stats_deferred(xx, G)
            y = plan.linattn_block(xx, g_pre, wqkv, wo, bo, None, B, F_, n, strides, 0, -1, gn=(st, gam, bet, G, r), w16=(uq, uo))
        else:
            h = plan.gn_silu(xx, gam, bet, G, residual=r)
            y = plan.linattn_block(h, g_pre, wqkv, wo, bo, None, B, F_, n, strides, 0, -1, w16=(uq, uo))
        assert [fn.__name__ for fn, _ in plan.calls][-1] == ("sdc_linattn_block_gn_f16" if fused else "sdc_linattn_block_f16")
        y.fill_(float("nan"))
        plan.run(_stream())
        torch.cuda.synchronize()
        outs.append(y.clone())
        assert torch.isfinite(y).all()
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------ net level
_NETS = {
    "smoke": (lambda d: sdc.Unet3D_with_Conv3D(dim=d, dim_mults=(1, 2, 4), channels=7), 64, (1, 32, 7, 32, 32), 300),
    "burgers": (lambda d: sdc.Unet2D(dim=d, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1), 64, (2, 3, 16, 128), 100),
    "tokamak": (lambda d: sdc.Unet1D(dim=d, dim_mults=(1, 2, 4, 8), channels=12, resnet_block_groups=1), 256, (2, 12, 128), 200),
}
_WIDE = {}
_F32 = ("sdc_linattn_block", "sdc_linattn_block_gn")
_F16 = ("sdc_linattn_block_f16", "sdc_linattn_block_gn_f16")


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


def _small(golden):
    g = golden("smoke_unet")
    small = _NETS["smoke"][0](8)
    small.load_state_dict(det_params(g.spec(), 300))
    small.to(DEV)
    return small, g["x"].to(DEV), g["t"].to(DEV)


def _calls(net, x):
    return [fn.__name__ for fn, _ in net.entry(tuple(x.shape), x.shape[0])["plan"].calls]


def _count(calls, names):
    return [calls.count(nm) for nm in names]


def _routed_sites(net, x):
    """[plain, GroupNorm-on-load] fused sites of the switch-off plan that sdc_linattn_block_f16_ok lists, and those it does not"""
    ok = _lib.get_lib().sdc_linattn_block_f16_ok
    on, off = [0, 0], [0, 0]
    for fn, args in net.entry(tuple(x.shape), x.shape[0])["plan"].calls:
        if fn.__name__ in _F32:
            form = _F32.index(fn.__name__)
            Cc, n = args[(10, 15)[form]], args[(11, 16)[form]]          # (..., outer, inner, C, n, strides ...)
            (on if ok(Cc, n) else off)[form] += 1
    return on, off


@pytest.mark.parametrize("tree,prec,fast", [("smoke", 4, False), ("smoke", 6, True), ("burgers", 4, False), ("tokamak", 4, False)])
def test_linattn_f16_net_against_reference_fixture(golden, tree, prec, fast):
    net, x, t, ref = _wide(golden, tree)
    try:
        net.precision, net.stem_f16, net.attn_f16, net.linattn_f16, net.forward_graph = prec, fast, fast, False, True
        net(x, t)
        sites, kept = _routed_sites(net, x)
        if sum(sites) + sum(kept) == 0:
            # no fused site in this net (the narrowest LinearAttention layer is wider than 128): the switch changes nothing
            e0 = net(x, t).clone()
            net.linattn_f16 = True
            assert torch.equal(net(x, t), e0) and _count(_calls(net, x), _F16) == [0, 0]
            return
        net.linattn_f16 = True
        eps = net(x, t).cpu()
        mse = ((eps - ref) ** 2).mean().item()
        print(f"[measured] {tree}_unet_wide precision {prec}{' + stem_f16 + attn_f16' if fast else ''} + linattn_f16: eps-MSE {mse:.3e}  "
              f"max|err| {(eps - ref).abs().max().item():.3e}  ({sites[0]} plain + {sites[1]} GroupNorm-on-load sites)")
        assert torch.isfinite(eps).all()
        assert mse <= 1e-5
        # the f16 entries at exactly the fused sites, form by form
        calls = _calls(net, x)
        assert sum(sites) > 0 and _count(calls, _F16) == sites and _count(calls, _F32) == kept
        # graph replay == eager call list, two runs bit-identical
        net.forward_graph = False
        eager = net(x, t).cpu()
        net.forward_graph = True
        assert torch.equal(eager, eps) and torch.equal(net(x, t).cpu(), eps)
        # a sample's eps does not depend on the batch it rides in
        assert torch.equal(net(x[:1], t[:1]).cpu()[0], eps[0])
    finally:
        net.precision, net.stem_f16, net.attn_f16, net.linattn_f16 = 4, False, False, False


def _train(net, x, t, grads):
    net.zero_grad(set_to_none=True)
    loss = (net.forward_train(x, t) ** 2).mean()
    if not grads:
        return loss.detach().cpu(), []
    loss.backward()
    return loss.detach().cpu(), [None if p.grad is None else p.grad.detach().cpu().clone() for p in net.parameters()]


def test_linattn_f16_off_on_off_and_fine_tuning_untouched(golden):
    net, x, t, _ = _wide(golden, "burgers")
    small, xs, ts = _small(golden)
    try:
        net.precision, net.linattn_f16 = 4, False
        e0 = net(x, t).clone()
        assert _count(_calls(net, x), _F16) == [0, 0] and sum(_count(_calls(net, x), _F32)) > 0
        net.linattn_f16 = True
        e1 = net(x, t).clone()
        net.linattn_f16 = False
        assert torch.equal(net(x, t), e0) and not torch.equal(e1, e0)
        # forward_train: the loss and every gradient bit-identical with the switch on and off (gradients on the dim-8 net, B = 1)
        res = {}
        for on in (False, True):
            net.linattn_f16 = small.linattn_f16 = on
            res[on] = (_train(net, x, t, True), _train(small, xs[:1], ts[:1], True))
        for i in (0, 1):
            assert torch.equal(res[False][i][0], res[True][i][0])
            assert any(a is not None for a in res[False][i][1])
            assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(res[False][i][1], res[True][i][1]))
    finally:
        net.linattn_f16 = small.linattn_f16 = False
        net.zero_grad(set_to_none=True)
        small.zero_grad(set_to_none=True)


def test_linattn_f16_net_without_a_fused_site_keeps_its_bits(golden):
    # the dim-8 smoke net has no LinearAttention layer of width 64 / 128: switch on == switch off, bit for bit, no f16 block in the plan
    n, xx, tt = _small(golden)
    try:
        n.linattn_f16 = False
        e0 = n(xx, tt).clone()
        assert sum(_count(_calls(n, xx), _F32)) == 0
        n.linattn_f16 = True
        assert torch.equal(n(xx, tt), e0)
        assert _count(_calls(n, xx), _F16) == [0, 0]
    finally:
        n.linattn_f16 = False


def test_linattn_f16_unfused_chain_keeps_its_bits(golden):
    net, x, t, _ = _wide(golden, "burgers")
    try:
        net.fuse_linattn, net.linattn_f16 = False, False
        e0 = net(x, t).clone()
        assert sum(_count(_calls(net, x), _F32)) == 0
        net.linattn_f16 = True
        assert torch.equal(net(x, t), e0)
        calls = _calls(net, x)
        assert _count(calls, _F16) == [0, 0] and _count(calls, _F32) == [0, 0]
    finally:
        net.fuse_linattn, net.linattn_f16 = True, False


def test_linattn_f16_sees_data_writes_to_a_qkv_weight(golden):
    net, x, t, _ = _wide(golden, "burgers")
    make, dim, _, _ = _NETS["burgers"]
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    name = next(k for k in sd if k.endswith("fn.fn.to_qkv.weight") and sd[k].shape[1] in (64, 128))
    try:
        net.precision, net.linattn_f16 = 4, True
        e0 = net(x, t).clone()
        dict(net.named_parameters())[name].data.mul_(1.5)
        e1 = net(x, t).clone()
        fresh = make(dim)
        fresh.load_state_dict(net.state_dict())
        fresh.to(DEV)
        fresh.linattn_f16 = True
        assert torch.equal(fresh(x, t), e1) and not torch.equal(e1, e0)
    finally:
        net.load_state_dict(sd)
        net.linattn_f16 = False
