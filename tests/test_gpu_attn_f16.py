"""-m gpu: net.attn_f16 (opt-in, samplers only) -- the fused temporal-attention block at width 64 on the fp16 matrix pipe
(csrc/sdc_tablock_f16.hip): fp16 operands (RNE), fp32 accumulation.  Block level, through the C ABI, on the inputs of
test_temporal_attention_block_fused: against an fp64 emulation that rounds at exactly the kernel's rounding points and against the exact
fp64 block, NaN pre-fill, determinism, batch invariance, the device packer, the LayerNorm scale invariance.  Net level: the eps-MSE
contract gate against the reference fixture at precision 4 and 6, the call list, graph replay, batch invariance; and nothing else moves
(switch off, fine-tuning, nets without a width-64 site, the unfused chain keep their bits); a `.data` write to a to_qkv weight is seen
by the next call."""
import pytest
import torch

import safediffcon_amd as sdc
from safediffcon_amd import _lib
from safediffcon_amd.engine import pack_tattn_f16
from oracle.detweights import det_params, det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Cc, Fr = 64, 32

# (B, H, W).  The kernel keeps ta_block_kernel's walk -- one persistent workgroup per CU (256), 8 pixels per group, the XCD-ordered
# walk where the group count and the grid are multiples of 8 -- so the shapes are the ones that reach every walk of the workgroups:
SHAPES = [
    (1, 1, 8),        # one pixel group
    (3, 2, 4),        # three groups: fewer than the CU count, not a multiple of 8, outer stride > 0
    (2, 4, 8),        # eight groups: the XCD-ordered walk with one group per XCD
    (3, 24, 32),      # 288 groups: more than one round of a 256-workgroup grid, a multiple of 8 (XCD-ordered walk, second tiles)
    (1, 17, 136),     # 289 groups: more than one round, not a multiple of 8 (plain walk, second tile)
]
_CASE = {}


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _inputs(B, H, W):
    x = det_tensor((B, Cc, Fr, H, W), 121)
    g = det_tensor((Cc,), 122, 0.3) + 1.0
    wqkv, wo = det_tensor((384, Cc), 123, 0.3), det_tensor((Cc, 128), 124, 0.3)
    freqs = (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)))
    relw = det_tensor((32, 4), 125, 0.5)                       # (num_buckets, heads) embedding
    return x, g, wqkv, wo, freqs, relw


def _branch(x, g, wqkv, wo, freqs, relw, r, eps=1e-5):
    """the attention branch y - x in fp64 (conv3d.py:165-184, 277-353); r rounds an operand of a matrix product: the identity for the
    exact block, .half().double() for the emulation of sdc_tattn_block_f16 -- xn, the weights, q and k after the rotary (unscaled: the
    scale rides on the softmax exponent), v, the un-normalised probabilities, O after the division by the (unrounded) row sum"""
    from oracle import nets as onets
    B, _, _, H, W = x.shape
    bias = onets.rel_pos_bias(relw, Fr).double()               # (heads, query, key)
    xd = x.double()
    xn = (xd - xd.mean(1, keepdim=True)) * (xd.var(1, unbiased=False, keepdim=True) + eps).rsqrt() * g.double().view(1, -1, 1, 1, 1)
    tok = r(xn).permute(0, 3, 4, 2, 1).reshape(B * H * W, Fr, Cc)                   # b (h w) f c
    q, k, v = (tok @ r(wqkv.double()).t()).chunk(3, -1)
    sp = lambda t: t.reshape(-1, Fr, 4, 32).permute(0, 2, 1, 3)                     # n heads f d
    q, k, v = r(onets.rotary(sp(q), freqs.double())), r(onets.rotary(sp(k), freqs.double())), r(sp(v))
    s = (q @ k.transpose(-1, -2)) * 32 ** -0.5 + bias[None]
    p = (s - s.amax(-1, keepdim=True)).exp()
    o = r((r(p) @ v) / p.sum(-1, keepdim=True))
    out = o.permute(0, 2, 1, 3).reshape(-1, Fr, 128) @ r(wo.double()).t()
    return out.reshape(B, H, W, Fr, Cc).permute(0, 4, 3, 1, 2)


def _case(shape):
    """inputs and the two fp64 references of a shape (computed once, never modified), with the CPU-side check of the inputs"""
    if shape not in _CASE:
        inp = _inputs(*shape)
        exact = _branch(*inp, lambda t: t)
        emu = _branch(*inp, lambda t: t.half().double())
        rms = exact.pow(2).mean().sqrt().item()
        # the emulation alone sits at 1.17-1.20e-3 of the branch rms from the exact block on these inputs (|q|, |v| up to ~12): the
        # gates below then test the kernel and not the inputs
        e_in = (emu - exact).pow(2).mean().sqrt().item() / rms
        assert 1.0e-3 <= e_in <= 1.5e-3, e_in
        _CASE[shape] = (inp, exact, emu, rms, e_in)
    return _CASE[shape]


def _tables(freqs, relw):
    from oracle import nets as onets
    ang = torch.arange(Fr, dtype=torch.float32)[:, None] * freqs[None, :]
    rot = torch.stack((ang.cos(), ang.sin()), dim=-1).reshape(-1).to(DEV)
    return rot, onets.rel_pos_bias(relw, Fr).float().reshape(-1).to(DEV)


def _pack_dev(wqkv, wo):
    lib = _lib.get_lib()
    wpk = torch.full((int(lib.sdc_pack_tattn_f16_bytes()) // 4,), float("nan"), device=DEV)
    wq_d, wo_d = wqkv.to(DEV), wo.to(DEV)
    _lib.check(lib.sdc_pack_tattn_f16(wq_d.data_ptr(), wo_d.data_ptr(), wpk.data_ptr(), _stream()), "sdc_pack_tattn_f16")
    torch.cuda.synchronize()
    return wpk


def _run(x_dev, g_dev, wpk, rot, bias, eps=1e-5):
    """one sdc_tattn_block_f16 call on a NaN-filled output"""
    lib = _lib.get_lib()
    B, _, _, H, W = x_dev.shape
    y = torch.full_like(x_dev, float("nan"))
    _lib.check(lib.sdc_tattn_block_f16(x_dev.data_ptr(), g_dev.data_ptr(), wpk.data_ptr(), rot.data_ptr(), bias.data_ptr(), y.data_ptr(),
                                       B, H * W, Cc, Fr, Cc * Fr * H * W, Fr * H * W, H * W, eps, _stream()), "sdc_tattn_block_f16")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attn_f16_block_rounds_where_documented(shape):
    (x, g, wqkv, wo, freqs, relw), exact, emu, rms, e_in = _case(shape)
    B = shape[0]
    wpk = _pack_dev(wqkv, wo)
    # device packer == host packer, bit for bit
    assert torch.equal(wpk.cpu().view(torch.int16), pack_tattn_f16(wqkv, wo).view(torch.int16))
    rot, bias = _tables(freqs, relw)
    x_dev, g_dev = x.to(DEV), g.to(DEV)
    y = _run(x_dev, g_dev, wpk, rot, bias)
    assert torch.isfinite(y).all()
    got = y.cpu().double() - x.double()
    e_emu = (got - emu).pow(2).mean().sqrt().item() / rms
    e_x = (got - exact).pow(2).mean().sqrt().item() / rms
    print(f"[measured] {shape}: rms err vs fp64 emulation {e_emu:.2e}, vs exact fp64 {e_x:.2e} (of the rms of the attention branch; "
          f"the emulation itself: {e_in:.2e})")
    assert e_emu <= 3e-4, e_emu
    assert e_x <= 2 * e_in, (e_x, e_in)
    # two runs bit-identical; sample 0 of the batch == the same sample alone
    assert torch.equal(_run(x_dev, g_dev, wpk, rot, bias), y)
    if B > 1:
        assert torch.equal(_run(x_dev[:1].contiguous(), g_dev, wpk, rot, bias)[0], y[0])


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_attn_f16_block_does_not_see_the_scale_of_x(shape):
    """LayerNorm makes the branch invariant to the scale of x, and the fp16 operands sit behind it.  The invariance is exact only with
    LayerNorm's eps scaled along (var + eps): x * 100 with eps * 100^2 must give the branch of x to within the emulation gate.  With eps
    left at 1e-5 the normalised values move by eps / (2 var) ~ 1e-5 (var ~ 0.5 here), which flips fp16 roundings: on the CPU the fp64
    emulation at x * 100 sits 4.1-4.4e-4 of the branch rms from the emulation at x (the exact block: 9.6e-6), so that run is held to the
    same gate against the emulation evaluated at x * 100.  (The residual add rounds y to fp32 at 100 |x|: ~2e-6 of the branch.)"""
    (x, g, wqkv, wo, freqs, relw), exact, emu, rms, e_in = _case(shape)
    rot, bias = _tables(freqs, relw)
    x100 = x * 100.0
    emu100 = _branch(x100, g, wqkv, wo, freqs, relw, lambda t: t.half().double())
    x_dev, g_dev, wpk = x100.to(DEV), g.to(DEV), _pack_dev(wqkv, wo)
    for eps, ref, what in ((1e-5 * 100.0 ** 2, emu, "eps * 1e4, vs the emulation at x"), (1e-5, emu100, "eps 1e-5, vs the emulation at x * 100")):
        y = _run(x_dev, g_dev, wpk, rot, bias, eps)
        assert torch.isfinite(y).all()
        got = y.cpu().double() - x100.double()
        e_emu = (got - ref).pow(2).mean().sqrt().item() / rms
        e_x = (got - exact).pow(2).mean().sqrt().item() / rms
        print(f"[measured] {shape} x * 100, {what}: rms err {e_emu:.2e}, vs exact fp64 at x {e_x:.2e} (of the rms of the attention branch)")
        assert e_emu <= 3e-4, e_emu
        assert e_x <= 2 * e_in, (e_x, e_in)


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


def _small(golden):
    g = golden("smoke_unet")
    small = _NETS["smoke"][0](8)
    small.load_state_dict(det_params(g.spec(), 300))
    small.to(DEV)
    return small, g["x"].to(DEV), g["t"].to(DEV)


def _calls(net, x):
    return [fn.__name__ for fn, _ in net.entry(tuple(x.shape), x.shape[0])["plan"].calls]


@pytest.mark.parametrize("prec,stem", [(4, False), (6, True)])
def test_attn_f16_net_against_reference_fixture(golden, prec, stem):
    net, x, t, ref = _wide(golden, "smoke")
    try:
        net.precision, net.stem_f16, net.attn_f16, net.forward_graph = prec, stem, False, True
        net(x, t)
        n_sites = _calls(net, x).count("sdc_tattn_block")
        assert n_sites > 0
        net.attn_f16 = True
        eps = net(x, t).cpu()
        mse = ((eps - ref) ** 2).mean().item()
        print(f"[measured] smoke_unet_wide precision {prec}{' + stem_f16' if stem else ''} + attn_f16: eps-MSE {mse:.3e}  "
              f"max|err| {(eps - ref).abs().max().item():.3e}")
        assert torch.isfinite(eps).all()
        assert mse <= 1e-5
        calls = _calls(net, x)
        assert calls.count("sdc_tattn_block_f16") == n_sites and calls.count("sdc_tattn_block") == 0
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
        net.precision, net.stem_f16, net.attn_f16 = 4, False, False


def _train(net, x, t, grads):
    net.zero_grad(set_to_none=True)
    loss = (net.forward_train(x, t) ** 2).mean()
    if not grads:
        return loss.detach().cpu(), []
    loss.backward()
    return loss.detach().cpu(), [None if p.grad is None else p.grad.detach().cpu().clone() for p in net.parameters()]


def test_attn_f16_off_on_off_and_fine_tuning_untouched(golden):
    net, x, t, _ = _wide(golden, "smoke")
    small, xs, ts = _small(golden)
    try:
        net.precision, net.attn_f16 = 4, False
        e0 = net(x, t).clone()
        assert "sdc_tattn_block_f16" not in _calls(net, x)
        net.attn_f16 = True
        e1 = net(x, t).clone()
        net.attn_f16 = False
        assert torch.equal(net(x, t), e0) and not torch.equal(e1, e0)
        # forward_train: the loss and every gradient bit-identical with the switch on and off (gradients on the dim-8 net, B = 1)
        res = {}
        for on in (False, True):
            net.attn_f16 = small.attn_f16 = on
            res[on] = (_train(net, x, t, False), _train(small, xs[:1], ts[:1], True))
        assert torch.equal(res[False][0][0], res[True][0][0])
        assert torch.equal(res[False][1][0], res[True][1][0])
        assert any(a is not None for a in res[False][1][1])
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(res[False][1][1], res[True][1][1]))
    finally:
        net.attn_f16 = small.attn_f16 = False
        net.zero_grad(set_to_none=True)


def test_attn_f16_nets_without_a_width_64_site_keep_their_bits(golden):
    # the dim-8 smoke net and the Burgers / tokamak nets have no fused temporal-attention site: switch on == switch off, bit for bit,
    # and no f16 block in the plan
    cases = [_small(golden)] + [_wide(golden, tree)[:3] for tree in ("burgers", "tokamak")]
    for n, xx, tt in cases:
        try:
            n.attn_f16 = False
            e0 = n(xx, tt).clone()
            n.attn_f16 = True
            assert torch.equal(n(xx, tt), e0)
            assert "sdc_tattn_block_f16" not in _calls(n, xx)
        finally:
            n.attn_f16 = False


def test_attn_f16_unfused_chain_keeps_its_bits(golden):
    net, x, t, _ = _wide(golden, "smoke")
    try:
        net.fuse_linattn, net.attn_f16 = False, False
        e0 = net(x, t).clone()
        assert "sdc_tattn_block" not in _calls(net, x)
        net.attn_f16 = True
        assert torch.equal(net(x, t), e0)
        calls = _calls(net, x)
        assert "sdc_tattn_block_f16" not in calls and "sdc_tattn_block" not in calls
    finally:
        net.fuse_linattn, net.attn_f16 = True, False


def test_attn_f16_sees_data_writes_to_a_qkv_weight(golden):
    net, x, t, _ = _wide(golden, "smoke")
    make, dim, _, _ = _NETS["smoke"]
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    try:
        net.precision, net.attn_f16 = 4, True
        e0 = net(x, t).clone()
        net.init_temporal_attn.fn.fn.fn.to_qkv.weight.data.mul_(1.5)
        e1 = net(x, t).clone()
        fresh = make(dim)
        fresh.load_state_dict(net.state_dict())
        fresh.to(DEV)
        fresh.attn_f16 = True
        assert torch.equal(fresh(x, t), e1) and not torch.equal(e1, e0)
    finally:
        net.load_state_dict(sd)
        net.attn_f16 = False
