"""net.train_fuse_attn: the fused temporal-attention block as one fine-tuning node -- sdc_tattn_block forward, sdc_tattn_block_bwd
backward (csrc/sdc_tablock_bwd.hip).

The fp64 reference of the block is a literal restatement under torch autograd: channel LayerNorm (biased variance, eps 1e-5, gain;
conv3d.py:165-174), the bias-free qkv / out Linear layers, _ref_attention with rotary and relative-position bias, the residual.
Gates are those of test_gpu_grad.py / test_gpu_grad_paths.py / test_gpu_finetune.py: y < 1e-5, every gradient < 2e-5 (_rel: max
error over max reference), loss 1e-5 and parameter gradients 2e-4 relative L2 for the whole net.
"""
import functools

import pytest
import torch

import safediffcon_amd as sdc
from oracle.detweights import det_params, det_tensor
from safediffcon_amd import _lib, autograd
from test_gpu_grad import DEV, _ref_attention, _rel, _rot_table
from test_gpu_grad_paths import _finite, _gate

pytestmark = pytest.mark.gpu

Y_GATE, G_GATE = 1e-5, 2e-5
NAMES = ("y", "dx", "dg", "dwqkv", "dwo", "dbias")


def _inputs(B, H, W, wscale=1.0):
    x = det_tensor((B, 64, 32, H, W), 300)
    g = 1.0 + 0.1 * det_tensor((64,), 301)
    wqkv = det_tensor((384, 64), 302, wscale * 64 ** -0.5)          # nn.Linear layouts
    wo = det_tensor((64, 128), 303, 128 ** -0.5)
    bias = 0.5 * det_tensor((4, 32, 32), 304)
    dy = det_tensor((B, 64, 32, H, W), 305)
    return x, g, wqkv, wo, bias, dy


def _block_ref(x, g, wqkv, wo, ang, bias, dy, dtype):
    """-> (y, dx, dg, dwqkv (384, 64), dwo (64, 128), dbias | None) in dtype on the CPU"""
    x, g, wqkv, wo, dy = (t.to(dtype).clone().requires_grad_() for t in (x, g, wqkv, wo, dy))
    bias = None if bias is None else bias.to(dtype).clone().requires_grad_()
    B, Cc, Fr, H, W = x.shape
    mean = x.mean(dim=1, keepdim=True)
    var = x.var(dim=1, unbiased=False, keepdim=True)
    xn = (x - mean) / (var + 1e-5).sqrt() * g.reshape(1, -1, 1, 1, 1)
    tok = xn.permute(0, 3, 4, 2, 1).reshape(B, H * W, Fr, Cc)                                    # b (h w) f c
    q, k, v = ((tok @ wqkv.t()).reshape(B, H * W, Fr, 3, 4, 32).permute(3, 0, 1, 4, 2, 5))       # (B, hw, heads, F, 32) each
    o = _ref_attention(q, k, v, None if ang is None else ang.to(dtype), bias)
    o = o.permute(0, 1, 3, 2, 4).reshape(B, H * W, Fr, 128) @ wo.t()
    y = o.reshape(B, H, W, Fr, Cc).permute(0, 4, 3, 1, 2) + x
    y.backward(dy.detach())
    return (y.detach(), x.grad, g.grad, wqkv.grad, wo.grad, None if bias is None else bias.grad)


@functools.lru_cache(maxsize=None)
def _case(B, H, W, tables=True, wscale=1.0):
    """inputs and the fp64 reference of one shape, computed once"""
    x, g, wqkv, wo, bias, dy = _inputs(B, H, W, wscale)
    rot, ang = _rot_table(32)
    if not tables:
        rot = ang = bias = None
    ref = _block_ref(x, g, wqkv, wo, ang, bias, dy, torch.float64)
    return (x, g, wqkv, wo, rot, bias, dy), ref


def _run_abi(inp, work=None, want_y=True):
    """sdc_tattn_block then sdc_tattn_block_bwd through the C ABI -> (y, dx, dg, dwqkv (384, 64), dwo (64, 128), dbias | None)"""
    x, g, wqkv, wo, rot, bias, dy = (None if t is None else t.to(DEV).contiguous() for t in inp)
    wqkv_p, wo_p = wqkv.t().contiguous(), wo.t().contiguous()
    lib = _lib.get_lib()
    B, Cc, Fr, H, W = x.shape
    hw = H * W
    geom = (B, hw, Cc, Fr, Cc * Fr * hw, Fr * hw, hw)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: 0 if t is None else t.data_ptr()      # noqa: E731
    y = torch.empty_like(x)
    if want_y:
        _lib.check(lib.sdc_tattn_block(p(x), p(g), p(wqkv_p), p(wo_p), p(rot), p(bias), p(y), *geom, 1e-5, st), "sdc_tattn_block")
    if work is None:
        work = torch.empty(int(lib.sdc_tattn_block_bwd_bytes(B, hw)) // 4, device=DEV)
    dx, dg, dwqkv, dwo = torch.empty_like(x), torch.empty_like(g), torch.empty_like(wqkv_p), torch.empty_like(wo_p)
    dbias = None if bias is None else torch.empty_like(bias)
    _lib.check(lib.sdc_tattn_block_bwd(p(x), p(g), p(wqkv_p), p(wo_p), p(rot), p(bias), p(dy), p(dx), p(dg), p(dwqkv), p(dwo), p(dbias),
                                       p(work), *geom, 1e-5, st), "sdc_tattn_block_bwd")
    torch.cuda.synchronize()
    return y, dx, dg, dwqkv.t(), dwo.t(), dbias


def _errs(got, ref):
    return [None if b is None else _rel(a, b) for a, b in zip(got, ref)]


def _fmt(errs):
    return " ".join(f"{n} {e:.2e}" for n, e in zip(NAMES, errs) if e is not None)


# ------------------------------------------------------------------ 1. the kernel against fp64, through the C ABI
# (1, 1x8): one pixel group, one workgroup; (2, 3x8): six groups, the plain walk, a sample boundary between tiles; (3, 32x32): 384
# groups, a multiple of 8 above the 256 CUs: the XCD-aware walk with an uneven share, every partial table live
@pytest.mark.parametrize("B,H,W,tables", [(1, 1, 8, True), (2, 3, 8, True), (3, 32, 32, True), (2, 3, 8, False)])
def test_block_backward_against_fp64(B, H, W, tables):
    inp, ref = _case(B, H, W, tables)
    got = _run_abi(inp)
    errs = _errs(got, ref)
    print(f"[measured] fused temporal block fwd + bwd B={B} {H}x{W} tables={tables}: {_fmt(errs)}")
    assert _finite(*got)
    assert errs[0] < Y_GATE
    assert all(e < G_GATE for e in errs[1:] if e is not None)
    assert (errs[5] is None) == (not tables)


# ------------------------------------------------------------------ 2. determinism, a dirty workspace
@pytest.mark.parametrize("B,H,W", [(2, 3, 8), (3, 32, 32)])
def test_block_backward_deterministic_on_dirty_workspace(B, H, W):
    inp, ref = _case(B, H, W)
    nwork = int(_lib.get_lib().sdc_tattn_block_bwd_bytes(B, H * W)) // 4
    work = torch.full((nwork,), float("nan"), device=DEV)
    first = _run_abi(inp, work, want_y=False)[1:]
    second = _run_abi(inp, work, want_y=False)[1:]
    assert _finite(*first) and _finite(*second)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert all(e < G_GATE for e in _errs(first, ref[1:]))


# ------------------------------------------------------------------ 3. sequences are independent
def test_block_backward_sample_independent_of_its_batch():
    inp, _ = _case(3, 32, 32)
    dx3 = _run_abi(inp, want_y=False)[1]
    alone = tuple(t[2:3].contiguous() if i in (0, 6) else t for i, t in enumerate(inp))
    dx1 = _run_abi(alone, want_y=False)[1]
    assert torch.equal(dx3[2:3], dx1)


# ------------------------------------------------------------------ 4. peaked softmax
@pytest.mark.parametrize("scale", [2.0, 4.0])
def test_block_backward_peaked(scale):
    inp, ref = _case(2, 4, 8, True, scale)
    x, g, wqkv, wo, rot, bias, dy = inp
    e32 = _errs(_block_ref(x, g, wqkv, wo, _rot_table(32)[1], bias, dy, torch.float32), ref)
    got = _run_abi(inp)
    errs = _errs(got, ref)
    print(f"[measured] fused temporal block, wqkv x {scale:g}, B=2 4x8: kernel {_fmt(errs)} | fp32 torch {_fmt(e32)}")
    assert _finite(*got)
    assert errs[0] < _gate(Y_GATE, e32[0])
    assert all(e < _gate(G_GATE, r) for e, r in zip(errs[1:], e32[1:]))


# ------------------------------------------------------------------ 5. the fused node against today's chain
class _Site:
    """the smallest thing Trainer.temporal needs of a net: the parameters of one site and the two switches"""
    precision, train_precision, fuse_linattn = 4, None, True

    def __init__(self, params, fuse):
        self.p, self.train_fuse_attn = params, fuse

    def P(self, key):
        return self.p[key]


def _site(B, H, W, fuse):
    x, g, wqkv, wo, _, dy = _inputs(B, H, W)
    emb = 0.5 * det_tensor((32, 4), 306)                             # time_rel_pos_bias.relative_attention_bias.weight (buckets, heads)
    leaf = lambda t: t.to(DEV).requires_grad_()                     # noqa: E731
    params = {"s.fn.norm.gamma": leaf(g.reshape(1, 64, 1, 1, 1)), "s.fn.fn.fn.to_qkv.weight": leaf(wqkv), "s.fn.fn.fn.to_out.weight": leaf(wo),
              "time_rel_pos_bias.relative_attention_bias.weight": leaf(emb),
              "init_temporal_attn.fn.fn.fn.rotary_emb.freqs": 1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)).to(DEV)}
    T = autograd.Trainer(_Site(params, fuse))
    xg = leaf(x)
    with T.step(torch.device(DEV)):
        y = T.temporal("s", xg, T._temporal_tables(32, torch.device(DEV)))
    return params, xg, y, dy


def _site_run(B, H, W, fuse):
    params, xg, y, dy = _site(B, H, W, fuse)
    (y * dy.to(DEV)).sum().backward()                                # a scalar loss whose gradient with respect to y is dy
    keys = ("s.fn.norm.gamma", "s.fn.fn.fn.to_qkv.weight", "s.fn.fn.fn.to_out.weight", "time_rel_pos_bias.relative_attention_bias.weight")
    return [y.detach(), xg.grad] + [params[k].grad for k in keys]


def test_fused_node_against_chain():
    B, H, W = 2, 4, 8
    x, g, wqkv, wo, _, dy = _inputs(B, H, W)
    emb = (0.5 * det_tensor((32, 4), 306)).double().requires_grad_()
    bias = emb[autograd._relpos_buckets(32, "cpu")].permute(2, 0, 1)
    r = _block_ref(x, g, wqkv, wo, _rot_table(32)[1], bias.detach(), dy, torch.float64)
    bias.backward(r[5])
    ref = [r[0], r[1], r[2].reshape(1, 64, 1, 1, 1), r[3], r[4], emb.grad]
    chain, fused = _site_run(B, H, W, False), _site_run(B, H, W, True)
    names = ("y", "dx", "dgamma", "dto_qkv", "dto_out", "drelpos")
    ec, ef = [_rel(a, b) for a, b in zip(chain, ref)], [_rel(a, b) for a, b in zip(fused, ref)]
    print("[measured] Trainer.temporal B=2 4x8 vs fp64: fused " + " ".join(f"{n} {e:.2e}" for n, e in zip(names, ef))
          + " | chain " + " ".join(f"{n} {e:.2e}" for n, e in zip(names, ec)))
    for n, a, b in zip(names, fused, chain):
        assert a.shape == b.shape, n
    for i, (f_, c_) in enumerate(zip(ef, ec)):
        gate = Y_GATE if i == 0 else G_GATE
        assert f_ < gate and c_ < gate, names[i]
        assert f_ <= (2 * c_ if c_ >= gate / 4 else gate), names[i]


# ------------------------------------------------------------------ 6. the whole net at production width
def _nodes(loss, name="TemporalBlockFn"):
    seen, todo, n = set(), [loss.grad_fn], 0
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        n += type(fn).__name__.startswith(name)
        todo += [f for f, _ in fn.next_functions]
    return n


# The net has FOUR temporal-attention sites of width 64, not three: init_temporal_attn, downs.0.3 and ups.2.3 at full resolution and
# ups.1.3 at half resolution (64 channels, 8 x 8 pixels here: covered by the same rule, and one of the four sites the sampler plans
# fuse).  The width-128 / 256 sites (downs.1.3, downs.2.3, ups.0.3, mid_temporal_attn) and the mid spatial attention stay
# AttnCoreFn chains: five of the nine softmax-attention cores.
FUSED_SITES, CORES = 4, 9


def _c4_net(B):
    net = sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7)
    net.load_state_dict(det_params([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 77))
    net.to(DEV).train()
    shape = (32, 7, 16, 16)
    x, t = det_tensor((B, *shape), 78).to(DEV), torch.tensor([3, 400, 777, 999][:B], device=DEV)
    tgt, w = det_tensor((B, *shape), 79).to(DEV), (det_tensor((B,), 80).abs() + 0.5).to(DEV)
    return net, x, t, tgt, w


def test_whole_net_with_fused_temporal_blocks():
    from oracle import nets as onets
    net, x, t, tgt, w = _c4_net(2)
    off =(w * ((net.forward_train(x, t) - tgt) ** 2).flatten(1).mean(1)).mean()
    assert _nodes(off) == 0 and _nodes(off, "AttnCoreFn") == CORES
    del off
    net.train_fuse_attn = True
    loss = (w * ((net.forward_train(x, t) - tgt) ** 2).flatten(1).mean(1)).mean()
    assert _nodes(loss) == FUSED_SITES and _nodes(loss, "AttnCoreFn") == CORES - FUSED_SITES      # the wider levels stay on the chain
    loss.backward()
    P = {k: v.detach().clone().requires_grad_() for k, v in net.state_dict().items()}
    ref = (w * ((onets.unet_smoke(P, x, t, dim=64, dim_mults=(1, 2, 4)) - tgt) ** 2).flatten(1).mean(1)).mean()
    ref.backward()
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
    gmax = max(v.grad.norm().item() for v in P.values() if v.grad is not None)
    worst, checked = 0.0, 0
    for k, p in net.named_parameters():
        if not p.requires_grad:
            continue
        gr, gref = p.grad, P[k].grad
        assert gr is not None and gref is not None, k
        n_ref = gref.norm().item()
        if n_ref < 1e-4 * gmax:
            assert gr.norm().item() < 2e-4 * gmax, k
            continue
        err = ((gr - gref).norm() / n_ref).item()
        worst, checked = max(worst, err), checked + 1
        assert err < 2e-4, (k, err)
    print(f"[measured] smoke dim 64, 32 frames of 16x16, B=2, train_fuse_attn: loss {loss.item():.6f} vs {ref.item():.6f}; "
          f"{checked} parameter gradients, worst relative L2 error {worst:.2e}")


# ------------------------------------------------------------------ 7. graph replay
def test_graphed_step_with_fused_temporal_blocks():
    net, _, _, _, _ = _c4_net(1)
    net.train_fuse_attn = True
    gd = sdc.GaussianDiffusionSmoke(net, image_size=16, frames=32, timesteps=50, loss_type="l2").to(DEV)
    shape = (32, 7, 16, 16)
    state, noise = det_tensor((1, *shape), 42, 0.3).to(DEV), det_tensor((1, *shape), 45).to(DEV)
    w, t = torch.tensor([1.25], device=DEV), torch.tensor([17], device=DEV)
    params = [p for p in net.parameters() if p.requires_grad]

    def eager():
        for p in params:
            p.grad = None
        loss = (w * gd.p_losses(state, t, noise=noise, mean=False)).mean()
        assert _nodes(loss) == FUSED_SITES
        loss.backward()
        return loss.detach().clone(), [p.grad.detach().clone() for p in params]
    l0, g0 = eager()
    step = sdc.GraphedLossStep(gd, state, weight=w, t=t, noise=noise)
    l1 = step(state, w, t, noise).clone()
    g1 = [g.clone() for g in step.grads]
    assert torch.equal(l0, l1) and all(torch.equal(a, b) for a, b in zip(g0, g1))
    for p in params:
        p.grad = None
    for p, g in zip(params, g1):
        p.grad = g.clone()
    torch.optim.SGD(params, lr=1e-4).step()
    l2 = step(state, None, t, None).clone()
    g2 = [g.clone() for g in step.grads]
    le, ge = eager()
    assert not torch.equal(l2, l1) and torch.equal(l2, le) and all(torch.equal(a, b) for a, b in zip(g2, ge))


# ------------------------------------------------------------------ 8. memory
def test_fused_node_saves_memory():
    B, H, W = 2, 32, 32

    def peak(fuse):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        params, xg, y, dy = _site(B, H, W, fuse)
        (y * dy.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base
    xbytes = B * 64 * 32 * H * W * 4
    chain, fused = peak(False), peak(True)
    print(f"[measured] one temporal site B=2 32x32 (x = {xbytes / 2**20:.1f} MiB), forward + backward peak allocated: chain "
          f"{chain / 2**20:.1f} MiB, fused {fused / 2**20:.1f} MiB")
    assert fused <= chain - 4 * xbytes
    lib = _lib.get_lib()
    assert lib.sdc_tattn_block_bwd_bytes(4, 1024) == lib.sdc_tattn_block_bwd_bytes(8, 1024)
