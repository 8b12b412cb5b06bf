"""-m gpu: net.attn_split -- the fused temporal-attention block at width 64 with its weight products (q / k / v projections, out-
projection) on the bf16 matrix pipe as exact three-way operand splits (csrc/sdc_tablock_x3.hip); the score and O = V P products,
LayerNorm, rotary, softmax and the residual on the fp32 block's instructions.  Block level, through the C ABI, on the shapes and inputs
of tests/test_gpu_attn_f16.py against the exact fp64 block, gated on the fp32 block's own error on the same inputs (the split-kernel
gate of tests/test_gpu_wino_x3.py); NaN pre-fill, determinism, batch invariance, the device packer, null tables, non-finite input.  Net
level, on the dim-64 smoke net at (1, 32, 7, 64, 64) -- the smallest input with a routed site: the call lists, off -> on -> off, attn_f16's
precedence, graph replay, forward_train, and the distance to the switch-off result against that result's own distance from the eager
oracle."""
import pytest
import torch

import safediffcon_amd as sdc
from safediffcon_amd import _lib
from safediffcon_amd.engine import pack_conv_weight, pack_tattn_x3
from oracle import nets as onets
from oracle.detweights import det_params, det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Cc, Fr = 64, 32

# (B, H, W): the shapes of tests/test_gpu_attn_f16.py -- the kernel keeps that walk (one persistent workgroup per CU, 8 pixels per group)
SHAPES = [
    (1, 1, 8),        # one pixel group
    (3, 2, 4),        # three groups: fewer than the CU count, not a multiple of 8, outer stride > 0
    (2, 4, 8),        # eight groups: the XCD-ordered walk with one group per XCD
    (3, 24, 32),      # 288 groups: the persistent walk takes a second tile on some workgroups only (XCD-ordered)
    (1, 17, 136),     # 289 groups, not a multiple of 8: the plain walk, second tile
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


def _branch(x, g, wqkv, wo, freqs, relw, eps=1e-5, rot=True, bias=True):
    """the attention branch y - x in fp64 with exact operands (conv3d.py:165-184, 277-353): the exact block of test_gpu_attn_f16.py;
    rot / bias False: without the rotary / the relative-position bias (null tables)"""
    B, _, _, H, W = x.shape
    xd = x.double()
    xn = (xd - xd.mean(1, keepdim=True)) * (xd.var(1, unbiased=False, keepdim=True) + eps).rsqrt() * g.double().view(1, -1, 1, 1, 1)
    tok = xn.permute(0, 3, 4, 2, 1).reshape(B * H * W, Fr, Cc)                      # b (h w) f c
    q, k, v = (tok @ wqkv.double().t()).chunk(3, -1)
    sp = lambda t: t.reshape(-1, Fr, 4, 32).permute(0, 2, 1, 3)                     # n heads f d
    q, k, v = sp(q), sp(k), sp(v)
    if rot:
        q, k = onets.rotary(q, freqs.double()), onets.rotary(k, freqs.double())
    s = (q @ k.transpose(-1, -2)) * 32 ** -0.5
    if bias:
        s = s + onets.rel_pos_bias(relw, Fr).double()[None]                         # (heads, query, key)
    p = (s - s.amax(-1, keepdim=True)).exp()
    o = (p @ v) / p.sum(-1, keepdim=True)
    out = o.permute(0, 2, 1, 3).reshape(-1, Fr, 128) @ wo.double().t()
    return out.reshape(B, H, W, Fr, Cc).permute(0, 4, 3, 1, 2)


def _case(shape):
    """inputs and the exact fp64 branch of a shape (computed once, never modified)"""
    if shape not in _CASE:
        inp = _inputs(*shape)
        exact = _branch(*inp)
        _CASE[shape] = (inp, exact, exact.pow(2).mean().sqrt().item(), exact.abs().max().item())
    return _CASE[shape]


def _tables(freqs, relw):
    ang = torch.arange(Fr, dtype=torch.float32)[:, None] * freqs[None, :]
    rot = torch.stack((ang.cos(), ang.sin()), dim=-1).reshape(-1).to(DEV)
    return rot, onets.rel_pos_bias(relw, Fr).float().reshape(-1).to(DEV)


def _pack_dev(wqkv, wo):
    lib = _lib.get_lib()
    wpk = torch.full((int(lib.sdc_pack_tattn_x3_bytes()) // 4,), float("nan"), device=DEV)
    wq_d, wo_d = wqkv.to(DEV), wo.to(DEV)
    _lib.check(lib.sdc_pack_tattn_x3(wq_d.data_ptr(), wo_d.data_ptr(), wpk.data_ptr(), _stream()), "sdc_pack_tattn_x3")
    torch.cuda.synchronize()
    return wpk


def _ptr(t):
    return None if t is None else t.data_ptr()


def _run(x_dev, g_dev, wpk, rot, bias, eps=1e-5):
    """one sdc_tattn_block_x3 call on a NaN-filled output"""
    lib = _lib.get_lib()
    B, _, _, H, W = x_dev.shape
    y = torch.full_like(x_dev, float("nan"))
    _lib.check(lib.sdc_tattn_block_x3(x_dev.data_ptr(), g_dev.data_ptr(), wpk.data_ptr(), _ptr(rot), _ptr(bias), y.data_ptr(),
                                      B, H * W, Cc, Fr, Cc * Fr * H * W, Fr * H * W, H * W, eps, _stream()), "sdc_tattn_block_x3")
    torch.cuda.synchronize()
    return y


def _run_fp32(x_dev, g_dev, wq4, wo4, rot, bias, eps=1e-5):
    """the fp32 block, sdc_tattn_block, on the same inputs"""
    lib = _lib.get_lib()
    B, _, _, H, W = x_dev.shape
    y = torch.full_like(x_dev, float("nan"))
    _lib.check(lib.sdc_tattn_block(x_dev.data_ptr(), g_dev.data_ptr(), wq4.data_ptr(), wo4.data_ptr(), _ptr(rot), _ptr(bias), y.data_ptr(),
                                   B, H * W, Cc, Fr, Cc * Fr * H * W, Fr * H * W, H * W, eps, _stream()), "sdc_tattn_block")
    torch.cuda.synchronize()
    return y


def _gate(tag, y, y32, x, exact, rms, scale):
    """the split-kernel gate: rms error of the branch y - x against the exact fp64 block, relative to the branch's rms, at most 1.25 x
    the fp32 block's on the same inputs (or 2^-23); max |err| below 1e-5 of the branch scale"""
    assert torch.isfinite(y).all() and torch.isfinite(y32).all()
    got, old = y.cpu().double() - x.double(), y32.cpu().double() - x.double()
    e_x3 = (got - exact).pow(2).mean().sqrt().item() / rms
    e_fp32 = (old - exact).pow(2).mean().sqrt().item() / rms
    e_max = (got - exact).abs().max().item() / scale
    print(f"[measured] {tag}: rms err vs exact fp64 (of the rms of the attention branch): split {e_x3:.3e} | fp32 block {e_fp32:.3e}; "
          f"max |err| of the branch scale {e_max:.3e}")
    assert e_x3 <= max(1.25 * e_fp32, 2.0 ** -23), (e_x3, e_fp32)
    assert e_max < 1e-5, e_max


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attn_x3_block_against_exact_fp64(shape):
    (x, g, wqkv, wo, freqs, relw), exact, rms, scale = _case(shape)
    B = shape[0]
    wpk = _pack_dev(wqkv, wo)
    # device packer == host twin, bit for bit
    assert torch.equal(wpk.cpu().view(torch.int16), pack_tattn_x3(wqkv, wo).view(torch.int16))
    rot, bias = _tables(freqs, relw)
    x_dev, g_dev = x.to(DEV), g.to(DEV)
    wq4, wo4 = pack_conv_weight(wqkv.view(384, 64, 1)).to(DEV), pack_conv_weight(wo.view(64, 128, 1)).to(DEV)
    y = _run(x_dev, g_dev, wpk, rot, bias)                    # (NaN-prefilled: every element is overwritten)
    _gate(str(shape), y, _run_fp32(x_dev, g_dev, wq4, wo4, rot, bias), x, exact, rms, scale)
    # two runs bit-identical; sample 0 of the batch == the same sample alone
    assert torch.equal(_run(x_dev, g_dev, wpk, rot, bias), y)
    if B > 1:
        assert torch.equal(_run(x_dev[:1].contiguous(), g_dev, wpk, rot, bias)[0], y[0])


def test_attn_x3_block_without_tables():
    shape = SHAPES[1]
    (x, g, wqkv, wo, freqs, relw), _, _, _ = _case(shape)
    exact = _branch(x, g, wqkv, wo, freqs, relw, rot=False, bias=False)
    rms, scale = exact.pow(2).mean().sqrt().item(), exact.abs().max().item()
    x_dev, g_dev, wpk = x.to(DEV), g.to(DEV), _pack_dev(wqkv, wo)
    wq4, wo4 = pack_conv_weight(wqkv.view(384, 64, 1)).to(DEV), pack_conv_weight(wo.view(64, 128, 1)).to(DEV)
    _gate(f"{shape} rot and bias null", _run(x_dev, g_dev, wpk, None, None), _run_fp32(x_dev, g_dev, wq4, wo4, None, None),
          x, exact, rms, scale)


def test_attn_x3_block_non_finite_input():
    """a non-finite x gives a non-finite y in every frame and channel of its pixel (LayerNorm ties the channels of the token, attention
    the frames of the pixel) and nowhere else: NaN -- the residual of the split is inf - inf -- where the fp32 block may give an
    infinity"""
    shape = SHAPES[2]
    (x, g, wqkv, wo, freqs, relw), _, _, _ = _case(shape)
    rot, bias = _tables(freqs, relw)
    g_dev, wpk = g.to(DEV), _pack_dev(wqkv, wo)
    clean = _run(x.to(DEV), g_dev, wpk, rot, bias)
    for bad in (float("nan"), float("inf"), -float("inf")):
        xb = x.clone()
        xb[1, 5, 9, 2, 3] = bad
        y = _run(xb.to(DEV), g_dev, wpk, rot, bias)
        hit = torch.zeros_like(y, dtype=torch.bool)
        hit[1, :, :, 2, 3] = True
        assert not torch.isfinite(y[hit]).any(), bad
        assert torch.equal(y[~hit], clean[~hit]), bad
        print(f"[measured] x = {bad} at one element: {int(torch.isnan(y[hit]).sum())} NaN, {int(torch.isinf(y[hit]).sum())} infinite of {int(hit.sum())}")


# ------------------------------------------------------------------ net level
_NET = {}


def _net():
    """the dim-64 smoke net with det_params weights and one sample at the production plane size (built once)"""
    if not _NET:
        net = sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7)
        spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        P = det_params(spec, 31)
        net.load_state_dict(P)
        net.to(DEV)
        x = det_tensor((1, 32, 7, 64, 64), 41).to(DEV)
        t = torch.tensor([417], device=DEV)
        _NET["v"] = (net, P, x, t)
    return _NET["v"]


def _plan_calls(net, x):
    return net.entry(tuple(x.shape), x.shape[0])["plan"].calls


def _calls(net, x):
    return [fn.__name__ for fn, _ in _plan_calls(net, x)]


def test_attn_split_net_routes_and_restores():
    """The dim-64 smoke net has four width-64 temporal sites: init_temporal_attn, downs.0.3 and ups.2.3 at the input's plane (64 x 64
    here: inner 4096, the routed size) and ups.1.3 at half of it (32 x 32: inner 1024, which the routing table does not list -- the
    existing plans at (1, 32, 7, 32, 32) must keep sdc_tattn_block).  So with the switch on every width-64 temporal site at inner 4096
    records sdc_tattn_block_x3, none of them records sdc_tattn_block, and the one site at inner 1024 records the parent's call."""
    net, P, x, t = _net()
    was = net.attn_split
    try:
        assert net.precision == 4
        net.attn_split, net.forward_graph = False, True
        e0 = net(x, t).clone()
        off = _calls(net, x)
        inner_off = [a[8] for fn, a in _plan_calls(net, x) if fn.__name__ == "sdc_tattn_block"]
        assert sorted(inner_off) == [1024, 4096, 4096, 4096] and "sdc_tattn_block_x3" not in off
        net.attn_split = True
        e1 = net(x, t).clone()
        on = _calls(net, x)
        assert [a[7] for fn, a in _plan_calls(net, x) if fn.__name__ == "sdc_tattn_block_x3"] == [4096, 4096, 4096]
        assert [a[8] for fn, a in _plan_calls(net, x) if fn.__name__ == "sdc_tattn_block"] == [1024]
        # nothing else moves: the same calls at the same places
        same = {"sdc_tattn_block_x3": "sdc_tattn_block"}
        assert [same.get(c, c) for c in on] == off
        assert torch.isfinite(e1).all() and not torch.equal(e1, e0)
        # graph replay == eager, two runs bit-identical
        net.forward_graph = False
        assert torch.equal(net(x, t), e1)
        net.forward_graph = True
        assert torch.equal(net(x, t), e1)
        # attn_f16 wins over attn_split
        net.attn_f16 = True
        both = _calls(net, x)
        assert both.count("sdc_tattn_block_f16") == 4 and "sdc_tattn_block_x3" not in both and "sdc_tattn_block" not in both
        net.attn_f16 = False
        # other precisions never route
        net.precision = 3
        assert "sdc_tattn_block_x3" not in _calls(net, x)
        net.precision = 4
        # off -> on -> off restores the bits
        net.attn_split = False
        assert _calls(net, x) == off and torch.equal(net(x, t), e0)
        # the change is smaller than the fp32 path's own distance from the eager oracle on the device
        with torch.no_grad():
            ref = onets.unet_smoke({k: v.to(DEV) for k, v in P.items()}, x, t, dim=64, dim_mults=(1, 2, 4))
        d_on_off = ((e1 - e0) ** 2).mean().item()
        d_off_ref = ((e0 - ref) ** 2).mean().item()
        d_on_ref = ((e1 - ref) ** 2).mean().item()
        print(f"[measured] dim-64 smoke net (1, 32, 7, 64, 64): mse(on, off) {d_on_off:.3e} | mse(off, eager oracle) {d_off_ref:.3e} | "
              f"mse(on, eager oracle) {d_on_ref:.3e}")
        assert d_on_off <= d_off_ref, (d_on_off, d_off_ref)
    finally:
        net.attn_split, net.attn_f16, net.precision = was, False, 4


def test_attn_split_forward_train_keeps_its_bits():
    net, _, x, t = _net()
    was = net.attn_split
    try:
        loss = {}
        for on in (False, True):
            net.attn_split = on
            net.zero_grad(set_to_none=True)
            loss[on] = (net.forward_train(x, t) ** 2).mean().detach().cpu()
        assert torch.isfinite(loss[False]) and torch.equal(loss[False], loss[True])
    finally:
        net.attn_split = was
