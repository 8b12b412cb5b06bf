"""net.train_fuse_linattn: the fused SpatialLinearAttention block as one fine-tuning node -- sdc_linattn_block_sel (impl 0) forward,
sdc_linattn_block_bwd backward (csrc/sdc_lablock_bwd.hip).

The fp64 reference of the block is a literal restatement under torch autograd: channel LayerNorm (biased variance, eps 1e-5, gain;
conv3d.py:165-174), the bias-free to_qkv and the biased to_out 1x1 convs, SpatialLinearAttention (conv3d.py:232-258: softmax over d
of q, times dim_head^-0.5, softmax over tokens of k, context = k v^T, out = context^T q), the residual.  Gates are those of
test_gpu_tattn_train.py: y < 1e-5, every gradient < 2e-5 (_rel: max error over max reference), loss 1e-5 and parameter gradients
2e-4 relative L2 for the whole net.
"""
import functools

import pytest
import torch

import safediffcon_amd as sdc
from oracle.detweights import det_params, det_tensor
from safediffcon_amd import _lib, autograd
from test_gpu_grad import DEV, _rel
from test_gpu_grad_paths import _finite, _gate

pytestmark = pytest.mark.gpu

Y_GATE, G_GATE = 1e-5, 2e-5
NAMES = ("y", "dx", "dg", "dwqkv", "dwo", "dbo")


def _inputs(Cc, B, Fr, H, W, wscale=1.0):
    x = det_tensor((B, Cc, Fr, H, W), 400)
    g = 1.0 + 0.1 * det_tensor((Cc,), 401)
    wqkv = det_tensor((384, Cc), 402, wscale * Cc ** -0.5)           # nn.Conv2d (1 x 1) layouts, the unit axes dropped
    wo = det_tensor((Cc, 128), 403, 128 ** -0.5)
    bo = 0.1 * det_tensor((Cc,), 404)
    dy = det_tensor((B, Cc, Fr, H, W), 405)
    return x, g, wqkv, wo, bo, dy


def _block_ref(x, g, wqkv, wo, bo, dy, dtype):
    """-> (y, dx, dg, dwqkv (384, C), dwo (C, 128), dbo | None) in dtype on the CPU"""
    x, g, wqkv, wo = (t.to(dtype).clone().requires_grad_() for t in (x, g, wqkv, wo))
    bo = None if bo is None else bo.to(dtype).clone().requires_grad_()
    B, Cc, Fr, H, W = x.shape
    n = H * W
    mean = x.mean(dim=1, keepdim=True)
    var = x.var(dim=1, unbiased=False, keepdim=True)
    xn = (x - mean) / (var + 1e-5).sqrt() * g.reshape(1, -1, 1, 1, 1)
    t = xn.permute(0, 2, 1, 3, 4).reshape(B * Fr, Cc, n)                                          # (b f) c (h w)
    q, k, v = torch.einsum("oc,bcn->bon", wqkv, t).reshape(B * Fr, 3, 4, 32, n).unbind(1)        # b h d n each
    q = q.softmax(dim=-2) * 32 ** -0.5
    k = k.softmax(dim=-1)
    ctx = torch.einsum("bhdn,bhen->bhde", k, v)
    out = torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(B * Fr, 128, n)
    z = torch.einsum("oc,bcn->bon", wo, out)
    if bo is not None:
        z = z + bo.reshape(1, -1, 1)
    y = z.reshape(B, Fr, Cc, H, W).permute(0, 2, 1, 3, 4) + x
    y.backward(dy.to(dtype))
    return (y.detach(), x.grad, g.grad, wqkv.grad, wo.grad, None if bo is None else bo.grad)


@functools.lru_cache(maxsize=None)
def _case(Cc, B, Fr, H, W, bias=True, wscale=1.0):
    """inputs and the fp64 reference of one shape, computed once"""
    x, g, wqkv, wo, bo, dy = _inputs(Cc, B, Fr, H, W, wscale)
    if not bias:
        bo = None
    return (x, g, wqkv, wo, bo, dy), _block_ref(x, g, wqkv, wo, bo, dy, torch.float64)


def _run_abi(inp, work=None, want_y=True):
    """sdc_linattn_block_sel (impl 0) then sdc_linattn_block_bwd through the C ABI -> (y, dx, dg, dwqkv (384, C), dwo (C, 128), dbo)"""
    x, g, wqkv, wo, bo, dy = (None if t is None else t.to(DEV).contiguous() for t in inp)
    wqkv_p, wo_p = wqkv.t().contiguous(), wo.t().contiguous()
    lib = _lib.get_lib()
    B, Cc, Fr, H, W = x.shape
    hw = H * W
    geom = (B, Fr, Cc, hw, Cc * Fr * hw, Fr * hw, hw)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: 0 if t is None else t.data_ptr()      # noqa: E731
    y = torch.empty_like(x)
    if want_y:
        fw = torch.empty(int(lib.sdc_linattn_block_bytes(B, Fr, Cc, hw)) // 4, device=DEV)
        _lib.check(lib.sdc_linattn_block_sel(p(x), p(g), p(wqkv_p), p(wo_p), p(bo), 0, p(fw), p(y), *geom, 0, -1, 1e-5, 0, st),
                   "sdc_linattn_block_sel")
    if work is None:
        work = torch.empty(int(lib.sdc_linattn_block_bwd_bytes(B, Fr, Cc, hw)) // 4, device=DEV)
    dx, dg, dwqkv, dwo = torch.empty_like(x), torch.empty_like(g), torch.empty_like(wqkv_p), torch.empty_like(wo_p)
    SENTINEL = 12345.0
    dbo = torch.full((Cc,), SENTINEL, device=DEV)
    _lib.check(lib.sdc_linattn_block_bwd(p(x), p(g), p(wqkv_p), p(wo_p), p(bo), p(dy), p(dx), p(dg), p(dwqkv), p(dwo),
                                         p(dbo) if bo is not None else 0, p(work), *geom, 0, -1, 1e-5, st), "sdc_linattn_block_bwd")
    torch.cuda.synchronize()
    return y, dx, dg, dwqkv.t(), dwo.t(), (dbo if bo is not None else None)


def _errs(got, ref):
    return [None if b is None else _rel(a, b) for a, b in zip(got, ref)]


def _fmt(errs):
    return " ".join(f"{n} {e:.2e}" for n, e in zip(NAMES, errs) if e is not None)


# ------------------------------------------------------------------ 1. the kernel against fp64, through the C ABI
# one tile | two tiles, one split, sample and frame boundaries | width 128 | 16 tiles, two splits | width 128, two splits | 17 tiles:
# uneven splits (9 + 8) | no output bias | 160 sequences: two chunks of whole samples (128 + 32), the second adds to the first's sums |
# 130 frames: more than the 128 sequence slots inside one sample (chunks of 128 + 2 frames)
SHAPES = [(64, 1, 1, 8, 8, True), (64, 2, 3, 8, 16, True), (128, 1, 2, 8, 8, True), (64, 1, 2, 32, 32, True), (128, 1, 1, 32, 32, True),
          (64, 1, 1, 8, 136, True), (64, 2, 3, 8, 16, False), (64, 5, 32, 8, 8, True), (64, 1, 130, 8, 8, True)]


@pytest.mark.parametrize("Cc,B,Fr,H,W,bias", SHAPES)
def test_block_backward_against_fp64(Cc, B, Fr, H, W, bias):
    inp, ref = _case(Cc, B, Fr, H, W, bias)
    got = _run_abi(inp)
    errs = _errs(got, ref)
    print(f"[measured] fused LinearAttention block fwd + bwd C={Cc} B={B} F={Fr} {H}x{W} bias={bias}: {_fmt(errs)}")
    assert _finite(*got)
    assert errs[0] < Y_GATE
    assert all(e < G_GATE for e in errs[1:] if e is not None)
    assert (errs[5] is None) == (not bias)


def test_block_backward_without_bias_leaves_dbo_alone():
    """bo null: dbo is neither required (a null dbo is accepted) nor written (a given one keeps its content)"""
    inp, _ = _case(64, 2, 3, 8, 16, False)
    x, g, wqkv, wo, _, dy = (None if t is None else t.to(DEV).contiguous() for t in inp)
    wqkv_p, wo_p = wqkv.t().contiguous(), wo.t().contiguous()
    lib = _lib.get_lib()
    B, Cc, Fr, H, W = x.shape
    hw = H * W
    work = torch.empty(int(lib.sdc_linattn_block_bwd_bytes(B, Fr, Cc, hw)) // 4, device=DEV)
    dx, dg, dwqkv, dwo = torch.empty_like(x), torch.empty_like(g), torch.empty_like(wqkv_p), torch.empty_like(wo_p)
    dbo = torch.full((Cc,), 7.0, device=DEV)
    _lib.check(lib.sdc_linattn_block_bwd(x.data_ptr(), g.data_ptr(), wqkv_p.data_ptr(), wo_p.data_ptr(), 0, dy.data_ptr(), dx.data_ptr(),
                                         dg.data_ptr(), dwqkv.data_ptr(), dwo.data_ptr(), dbo.data_ptr(), work.data_ptr(), B, Fr, Cc, hw,
                                         Cc * Fr * hw, Fr * hw, hw, 0, -1, 1e-5, torch.cuda.current_stream().cuda_stream),
               "sdc_linattn_block_bwd")
    torch.cuda.synchronize()
    assert bool((dbo == 7.0).all())


# ------------------------------------------------------------------ 2. determinism, a dirty workspace
@pytest.mark.parametrize("Cc,B,Fr,H,W", [(64, 2, 3, 8, 16), (64, 1, 2, 32, 32)])
def test_block_backward_deterministic_on_dirty_workspace(Cc, B, Fr, H, W):
    inp, ref = _case(Cc, B, Fr, H, W)
    nwork = int(_lib.get_lib().sdc_linattn_block_bwd_bytes(B, Fr, Cc, H * W)) // 4
    work = torch.full((nwork,), float("nan"), device=DEV)
    first = _run_abi(inp, work, want_y=False)[1:]
    second = _run_abi(inp, work, want_y=False)[1:]
    assert _finite(*first) and _finite(*second)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert all(e < G_GATE for e in _errs(first, ref[1:]))


# ------------------------------------------------------------------ 3. sequences are independent
def test_block_backward_sample_independent_of_its_batch():
    inp = _inputs(64, 3, 2, 32, 32)
    dx3 = _run_abi(inp, want_y=False)[1]
    alone = tuple(t[2:3].contiguous() if i in (0, 5) else t for i, t in enumerate(inp))
    dx1 = _run_abi(alone, want_y=False)[1]
    assert torch.equal(dx3[2:3], dx1)


# ------------------------------------------------------------------ 4. peaked softmaxes
@pytest.mark.parametrize("scale", [2.0, 4.0])
def test_block_backward_peaked(scale):
    inp, ref = _case(64, 2, 1, 8, 16, True, scale)
    e32 = _errs(_block_ref(*inp, torch.float32), ref)
    got = _run_abi(inp)
    errs = _errs(got, ref)
    print(f"[measured] fused LinearAttention block, wqkv x {scale:g}, C=64 B=2 F=1 8x16: kernel {_fmt(errs)} | fp32 torch {_fmt(e32)}")
    assert _finite(*got)
    assert errs[0] < _gate(Y_GATE, e32[0])
    assert all(e < _gate(G_GATE, r) for e, r in zip(errs[1:], e32[1:]))


# ------------------------------------------------------------------ 5. the fused node against today's chain
class _Site:
    """the smallest thing Trainer.spatial_linear needs of a net: the parameters of one site and the switches"""
    precision, train_precision, fuse_linattn, train_fuse_attn = 4, None, True, False

    def __init__(self, params, fuse):
        self.p, self.train_fuse_linattn = params, fuse

    def P(self, key):
        return self.p[key]


KEYS = ("s.fn.norm.gamma", "s.fn.fn.to_qkv.weight", "s.fn.fn.to_out.weight", "s.fn.fn.to_out.bias")


def _site(Cc, B, Fr, H, W, fuse):
    x, g, wqkv, wo, bo, dy = _inputs(Cc, B, Fr, H, W)
    leaf = lambda t: t.to(DEV).requires_grad_()                     # noqa: E731
    params = dict(zip(KEYS, (leaf(g.reshape(1, Cc, 1, 1, 1)), leaf(wqkv.reshape(384, Cc, 1, 1)), leaf(wo.reshape(Cc, 128, 1, 1)), leaf(bo))))
    T = autograd.Trainer(_Site(params, fuse))
    xg = leaf(x)
    with T.step(torch.device(DEV)):
        y = T.spatial_linear("s", xg)
    return params, xg, y, dy


def _site_run(Cc, B, Fr, H, W, fuse):
    params, xg, y, dy = _site(Cc, B, Fr, H, W, fuse)
    assert (type(y.grad_fn).__name__.startswith("LinAttnBlockFn")) == fuse
    (y * dy.to(DEV)).sum().backward()                                # a scalar loss whose gradient with respect to y is dy
    return [y.detach(), xg.grad] + [params[k].grad for k in KEYS]


@pytest.mark.parametrize("Cc", [64, 128])
def test_fused_node_against_chain(Cc):
    B, Fr, H, W = 2, 3, 8, 16
    _, r = _case(Cc, B, Fr, H, W)
    ref = [r[0], r[1], r[2].reshape(1, Cc, 1, 1, 1), r[3].reshape(384, Cc, 1, 1), r[4].reshape(Cc, 128, 1, 1), r[5]]
    chain, fused = _site_run(Cc, B, Fr, H, W, False), _site_run(Cc, B, Fr, H, W, True)
    names = ("y", "dx", "dgamma", "dto_qkv", "dto_out", "dbias")
    ec, ef = [_rel(a, b) for a, b in zip(chain, ref)], [_rel(a, b) for a, b in zip(fused, ref)]
    print(f"[measured] Trainer.spatial_linear C={Cc} B=2 F=3 8x16 vs fp64: fused " + " ".join(f"{n} {e:.2e}" for n, e in zip(names, ef))
          + " | chain " + " ".join(f"{n} {e:.2e}" for n, e in zip(names, ec)))
    for n, a, b in zip(names, fused, chain):
        assert a.shape == b.shape, n
    for i, (f_, c_) in enumerate(zip(ef, ec)):
        gate = Y_GATE if i == 0 else G_GATE
        assert f_ < gate and c_ < gate, names[i]


# ------------------------------------------------------------------ 6. the whole net at production width
def _nodes(loss, name):
    seen, todo, n = set(), [loss.grad_fn], 0
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        n += type(fn).__name__.startswith(name)
        todo += [f for f, _ in fn.next_functions]
    return n


def _c4_net(B):
    net = sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7)
    net.load_state_dict(det_params([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 77))
    net.to(DEV).train()
    shape = (32, 7, 16, 16)
    x, t = det_tensor((B, *shape), 78).to(DEV), torch.tensor([3, 400, 777, 999][:B], device=DEV)
    tgt, w = det_tensor((B, *shape), 79).to(DEV), (det_tensor((B,), 80).abs() + 0.5).to(DEV)
    return net, x, t, tgt, w


def _loss(net, x, t, tgt, w):
    return (w * ((net.forward_train(x, t) - tgt) ** 2).flatten(1).mean(1)).mean()


@functools.lru_cache(maxsize=None)
def _c4_reference():
    """loss and parameter gradients of oracle.nets.unet_smoke on the inputs of _c4_net(2), computed once"""
    from oracle import nets as onets
    net, x, t, tgt, w = _c4_net(2)
    P = {k: v.detach().clone().requires_grad_() for k, v in net.state_dict().items()}
    ref = (w * ((onets.unet_smoke(P, x, t, dim=64, dim_mults=(1, 2, 4)) - tgt) ** 2).flatten(1).mean(1)).mean()
    ref.backward()
    return ref.item(), {k: (None if v.grad is None else v.grad.detach()) for k, v in P.items()}


@pytest.mark.parametrize("also_temporal", [False, True])
def test_whole_net_with_fused_linattn_blocks(also_temporal, monkeypatch):
    net, x, t, tgt, w = _c4_net(2)
    shapes = []
    orig = autograd.Trainer.spatial_linear
    monkeypatch.setattr(autograd.Trainer, "spatial_linear", lambda self, p, h: (shapes.append(tuple(h.shape)), orig(self, p, h))[1])
    net.train_fuse_attn = also_temporal
    off = _loss(net, x, t, tgt, w)
    sites = sum(bool(net._la_fusable(s)) for s in shapes)
    cores = _nodes(off, "LinAttnCoreFn")
    # downs.0.2 (64 wide, 16 x 16), downs.1.2 (128, 8 x 8), ups.1.2 (64, 8 x 8) and ups.2.2 (64, 16 x 16) are covered; downs.2.2 (256
    # wide) and ups.0.2 (4 x 4 = 16 tokens) stay on the chain
    assert sites == 4 and cores == len(shapes) == 6
    assert _nodes(off, "LinAttnBlockFn") == 0
    del off
    net.train_fuse_linattn = True
    loss = _loss(net, x, t, tgt, w)
    assert _nodes(loss, "LinAttnBlockFn") == sites and _nodes(loss, "LinAttnCoreFn") == cores - sites
    assert _nodes(loss, "TemporalBlockFn") == (4 if also_temporal else 0)
    loss.backward()
    lref, G = _c4_reference()
    assert abs(loss.item() - lref) < 1e-5 * abs(lref)
    gmax = max(v.norm().item() for v in G.values() if v is not None)
    worst, checked = 0.0, 0
    for k, p in net.named_parameters():
        if not p.requires_grad:
            continue
        gr, gref = p.grad, G[k]
        assert gr is not None and gref is not None, k
        n_ref = gref.norm().item()
        if n_ref < 1e-4 * gmax:
            assert gr.norm().item() < 2e-4 * gmax, k
            continue
        err = ((gr - gref).norm() / n_ref).item()
        worst, checked = max(worst, err), checked + 1
        assert err < 2e-4, (k, err)
    print(f"[measured] smoke dim 64, 32 frames of 16x16, B=2, train_fuse_linattn (train_fuse_attn={also_temporal}): loss {loss.item():.6f} "
          f"vs {lref:.6f}; {checked} parameter gradients, worst relative L2 error {worst:.2e}")


# ------------------------------------------------------------------ 7. graph replay
def test_graphed_step_with_fused_linattn_blocks():
    net, _, _, _, _ = _c4_net(1)
    net.train_fuse_linattn = True
    gd = sdc.GaussianDiffusionSmoke(net, image_size=16, frames=32, timesteps=50, loss_type="l2").to(DEV)
    shape = (32, 7, 16, 16)
    state, noise = det_tensor((1, *shape), 42, 0.3).to(DEV), det_tensor((1, *shape), 45).to(DEV)
    w, t = torch.tensor([1.25], device=DEV), torch.tensor([17], device=DEV)
    params = [p for p in net.parameters() if p.requires_grad]

    def eager():
        for p in params:
            p.grad = None
        loss = (w * gd.p_losses(state, t, noise=noise, mean=False)).mean()
        assert _nodes(loss, "LinAttnBlockFn") == 4
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
    Cc, B, Fr, H, W = 64, 2, 4, 32, 32

    def peak(fuse):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        params, xg, y, dy = _site(Cc, B, Fr, H, W, fuse)
        (y * dy.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base
    xbytes = B * Cc * Fr * H * W * 4
    chain, fused = peak(False), peak(True)
    print(f"[measured] one SpatialLinearAttention site C=64 B=2 F=4 32x32 (x = {xbytes / 2**20:.1f} MiB), forward + backward peak "
          f"allocated: chain {chain / 2**20:.1f} MiB, fused {fused / 2**20:.1f} MiB")
    assert fused <= chain - 4 * xbytes
