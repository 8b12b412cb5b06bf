"""net.train_fuse_linattn on the 1-D nets: the fused post-norm LinearAttention block as one fine-tuning node -- sdc_linattn_block_sel
(impl 0) forward, sdc_linattn_block_post_bwd backward (csrc/sdc_lablock_bwd.hip).

The fp64 reference is _block_ref of test_gpu_linattn_train.py with the norm behind to_out added and both norm modes, restated
literally under torch autograd on the CPU: mode 0 channel LayerNorm (biased variance, eps 1e-5, gain; 1D/model/unet.py:53-63), mode 1
RMSNorm (F.normalize over channels, gain, sqrt(C); tokamak/model/unet.py:45-51); LinearAttention (1D/model/unet.py:182-222: softmax
over d of q times dim_head^-0.5, softmax over tokens of k, context = k v^T, out = context^T q, to_out = 1x1 conv + norm); the
residual.  Inputs are that file's (det_tensor seeds 400 - 405) plus g_post = 1 + 0.1 det_tensor((C,), 406).  Gates are the project's:
y < 1e-5, every gradient < 2e-5 (_rel: max error over max reference); loss 1e-5 and parameter gradients 2e-4 relative L2 for the
whole nets.  The fp32 CPU restatement against fp64 gives <= 1.1e-6 on all seven outputs in both modes on (C, B, n) = (64, 3, 128),
(128, 2, 64), (64, 1, 1088) and (64, 64, 2048), and the per-token std of z is about 0.1 >> sqrt(eps): the gates leave about 9x over
plain fp32 on well-conditioned inputs.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import safediffcon_amd as sdc
from oracle.detweights import det_params, det_tensor
from safediffcon_amd import _lib, autograd
from test_gpu_grad import DEV, _rel
from test_gpu_grad_paths import _finite, _gate

pytestmark = pytest.mark.gpu

Y_GATE, G_GATE = 1e-5, 2e-5
NAMES = ("y", "dx", "dg_pre", "dwqkv", "dwo", "dbo", "dg_post")


def _inputs(Cc, O, I, n, wscale=1.0, woscale=1.0, zero_bias=False):
    """x, dy (outer, C, inner, n): every (outer, inner) index is one sequence of n tokens"""
    x = det_tensor((O, Cc, I, n), 400)
    g = 1.0 + 0.1 * det_tensor((Cc,), 401)
    wqkv = det_tensor((384, Cc), 402, wscale * Cc ** -0.5)           # the 1x1 conv layouts, the unit axes dropped
    wo = det_tensor((Cc, 128), 403, woscale * 128 ** -0.5)
    bo = 0.1 * det_tensor((Cc,), 404)
    if zero_bias:
        bo = torch.zeros_like(bo)
    dy = det_tensor((O, Cc, I, n), 405)
    gp = 1.0 + 0.1 * det_tensor((Cc,), 406)
    return x, g, wqkv, wo, bo, gp, dy


def _norm(v, g, mode):
    """channel norm over axis 1 of v"""
    shape = [1, -1] + [1] * (v.dim() - 2)
    if mode == 0:
        mean = v.mean(dim=1, keepdim=True)
        var = v.var(dim=1, unbiased=False, keepdim=True)
        return (v - mean) / (var + 1e-5).sqrt() * g.reshape(shape)
    return F.normalize(v, dim=1) * g.reshape(shape) * v.shape[1] ** 0.5


def _block_ref(x, g, wqkv, wo, bo, gp, dy, modes, dtype):
    """-> (y, dx, dg_pre, dwqkv (384, C), dwo (C, 128), dbo | None, dg_post) in dtype on the CPU"""
    x, g, wqkv, wo, gp = (t.to(dtype).clone().requires_grad_() for t in (x, g, wqkv, wo, gp))
    bo = None if bo is None else bo.to(dtype).clone().requires_grad_()
    O, Cc, I, n = x.shape
    xn = _norm(x, g, modes[0])
    t = xn.permute(0, 2, 1, 3).reshape(O * I, Cc, n)
    q, k, v = torch.einsum("oc,bcn->bon", wqkv, t).reshape(O * I, 3, 4, 32, n).unbind(1)          # b h d n each
    q = q.softmax(dim=-2) * 32 ** -0.5
    k = k.softmax(dim=-1)
    ctx = torch.einsum("bhdn,bhen->bhde", k, v)
    out = torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(O * I, 128, n)
    z = torch.einsum("oc,bcn->bon", wo, out)
    if bo is not None:
        z = z + bo.reshape(1, -1, 1)
    u = _norm(z, gp, modes[1])
    y = u.reshape(O, I, Cc, n).permute(0, 2, 1, 3) + x
    y.backward(dy.to(dtype))
    return (y.detach(), x.grad, g.grad, wqkv.grad, wo.grad, None if bo is None else bo.grad, gp.grad)


@functools.lru_cache(maxsize=None)
def _case(Cc, O, I, n, bias=True, modes=(0, 0), wscale=1.0, woscale=1.0, zero_bias=False):
    """inputs and the fp64 reference of one case, computed once"""
    x, g, wqkv, wo, bo, gp, dy = _inputs(Cc, O, I, n, wscale, woscale, zero_bias)
    if not bias:
        bo = None
    return (x, g, wqkv, wo, bo, gp, dy), _block_ref(x, g, wqkv, wo, bo, gp, dy, modes, torch.float64)


def _run_abi(inp, modes, work=None, want_y=True, dirty=False, dbo_arg="auto"):
    """sdc_linattn_block_sel (impl 0) then sdc_linattn_block_post_bwd through the C ABI, strides (C inner n, inner n, n)
    -> (y, dx, dg_pre, dwqkv (384, C), dwo (C, 128), dbo, dg_post)"""
    x, g, wqkv, wo, bo, gp, dy = (None if t is None else t.to(DEV).contiguous() for t in inp)
    wqkv_p, wo_p = wqkv.t().contiguous(), wo.t().contiguous()
    lib = _lib.get_lib()
    O, Cc, I, n = x.shape
    geom = (O, I, Cc, n, Cc * I * n, I * n, n)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: 0 if t is None else t.data_ptr()      # noqa: E731
    y = torch.empty_like(x)
    if want_y:
        fw = torch.empty(int(lib.sdc_linattn_block_bytes(O, I, Cc, n)) // 4, device=DEV)
        _lib.check(lib.sdc_linattn_block_sel(p(x), p(g), p(wqkv_p), p(wo_p), p(bo), p(gp), p(fw), p(y), *geom, modes[0], modes[1], 1e-5,
                                             0, st), "sdc_linattn_block_sel")
    if work is None:
        work = torch.empty(int(lib.sdc_linattn_block_post_bwd_bytes(O, I, Cc, n)) // 4, device=DEV)
    dx = torch.full_like(x, float("nan")) if dirty else torch.empty_like(x)
    dg, dwqkv, dwo, dgp = torch.empty_like(g), torch.empty_like(wqkv_p), torch.empty_like(wo_p), torch.empty_like(gp)
    dbo = torch.full((Cc,), 12345.0, device=DEV)
    dbo_ptr = (p(dbo) if bo is not None else 0) if dbo_arg == "auto" else dbo_arg
    _lib.check(lib.sdc_linattn_block_post_bwd(p(x), p(g), p(wqkv_p), p(wo_p), p(bo), p(gp), p(dy), p(dx), p(dg), p(dwqkv), p(dwo),
                                              dbo_ptr, p(dgp), p(work), *geom, modes[0], modes[1], 1e-5, st),
               "sdc_linattn_block_post_bwd")
    torch.cuda.synchronize()
    return y, dx, dg, dwqkv.t(), dwo.t(), (dbo if bo is not None else None), dgp


def _errs(got, ref):
    return [None if b is None else _rel(a, b) for a, b in zip(got, ref)]


def _fmt(errs):
    return " ".join(f"{n} {e:.2e}" for n, e in zip(NAMES, errs) if e is not None)


# ------------------------------------------------------------------ 1. the kernel against fp64, through the C ABI
# (C, outer, inner, n, bias): one tile | two tiles, sequence boundaries | width 128 | 16 tiles, two token splits | width 128, two
# splits | 17 tiles: uneven splits (9 + 8) | no output bias | 160 sequences: two chunks of sequence slots (128 + 32), the second adds
# to the first's sums | inner > 1 with the smoke-style strides
SHAPES = [(64, 1, 1, 64, True), (64, 3, 1, 128, True), (128, 2, 1, 64, True), (64, 1, 1, 1024, True), (128, 1, 1, 1024, True),
          (64, 1, 1, 1088, True), (64, 3, 1, 128, False), (64, 160, 1, 64, True), (64, 2, 3, 128, True)]
CASES = [(*s, m) for m in ((0, 0), (1, 1)) for s in SHAPES] + [(64, 3, 1, 128, True, (0, 1)), (64, 3, 1, 128, True, (1, 0))]


@pytest.mark.parametrize("Cc,O,I,n,bias,modes", CASES)
def test_post_block_backward_against_fp64(Cc, O, I, n, bias, modes):
    inp, ref = _case(Cc, O, I, n, bias, modes)
    got = _run_abi(inp, modes)
    errs = _errs(got, ref)
    print(f"[measured] fused post-norm LinearAttention block fwd + bwd C={Cc} outer={O} inner={I} n={n} bias={bias} modes={modes}: "
          f"{_fmt(errs)}")
    assert _finite(*got)
    assert errs[0] < Y_GATE
    assert all(e < G_GATE for e in errs[1:] if e is not None)
    assert (errs[5] is None) == (not bias)


# ------------------------------------------------------------------ 2. no output bias
def test_post_block_backward_without_bias_leaves_dbo_alone():
    """bo null: dbo is neither required (a null dbo is accepted) nor written (a given one keeps its content)"""
    inp, ref = _case(64, 3, 1, 128, False, (0, 0))
    with_null = _run_abi(inp, (0, 0), want_y=False, dbo_arg=0)
    keep = torch.full((64,), 7.0, device=DEV)
    with_buf = _run_abi(inp, (0, 0), want_y=False, dbo_arg=keep.data_ptr())
    assert bool((keep == 7.0).all())
    for a, b in zip(with_null[1:], with_buf[1:]):
        assert (a is None and b is None) or torch.equal(a, b)
    assert all(e < G_GATE for e in _errs(with_null, ref)[1:] if e is not None)


# ------------------------------------------------------------------ 3. determinism, dirty buffers
@pytest.mark.parametrize("Cc,O,I,n", [(64, 3, 1, 128), (64, 1, 1, 1024)])
def test_post_block_backward_deterministic_on_dirty_buffers(Cc, O, I, n):
    """the workspace and dx (which the first sweep uses to hand dz to the second) hold NaN before the call"""
    inp, ref = _case(Cc, O, I, n, True, (0, 0))
    nwork = int(_lib.get_lib().sdc_linattn_block_post_bwd_bytes(O, I, Cc, n)) // 4
    work = torch.full((nwork,), float("nan"), device=DEV)
    first = _run_abi(inp, (0, 0), work, want_y=False, dirty=True)[1:]
    work.fill_(float("nan"))
    second = _run_abi(inp, (0, 0), work, want_y=False, dirty=True)[1:]
    assert _finite(*first) and _finite(*second)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert all(e < G_GATE for e in _errs(first, ref[1:]))


# ------------------------------------------------------------------ 4. sequences are independent
def test_post_block_backward_sample_independent_of_its_batch():
    inp = _inputs(64, 3, 1, 1024)
    dx3 = _run_abi(inp, (1, 1), want_y=False)[1]
    alone = tuple(t[0:1].contiguous() if i in (0, 6) else t for i, t in enumerate(inp))
    dx1 = _run_abi(alone, (1, 1), want_y=False)[1]
    assert torch.equal(dx3[0:1], dx1)


# ------------------------------------------------------------------ 5. hard inputs
# peaked softmaxes (wqkv x 2, x 4); a small z (wo x 1e-2, bo = 0): mode 0's rstd is large, eps no longer negligible
@pytest.mark.parametrize("modes", [(0, 0), (1, 1)])
@pytest.mark.parametrize("wscale,woscale,zero_bias", [(2.0, 1.0, False), (4.0, 1.0, False), (1.0, 1e-2, True)])
def test_post_block_backward_hard_inputs(wscale, woscale, zero_bias, modes):
    inp, ref = _case(64, 2, 1, 128, True, modes, wscale, woscale, zero_bias)
    e32 = _errs(_block_ref(*inp, modes, torch.float32), ref)
    got = _run_abi(inp, modes)
    errs = _errs(got, ref)
    print(f"[measured] fused post-norm LinearAttention block, wqkv x {wscale:g}, wo x {woscale:g}, zero bias {zero_bias}, modes={modes}, "
          f"C=64 outer=2 n=128: kernel {_fmt(errs)} | fp32 torch {_fmt(e32)}")
    assert _finite(*got)
    assert errs[0] < _gate(Y_GATE, e32[0])
    assert all(e < _gate(G_GATE, r) for e, r in zip(errs[1:], e32[1:]))


# ------------------------------------------------------------------ 6. the fused node against today's chain
class _Site:
    """the smallest thing Trainer.linattn_lucid needs of a net: the parameters of one site and the switches"""
    precision, train_precision, fuse_linattn, train_fuse_attn = 4, None, True, False

    def __init__(self, params, fuse):
        self.p, self.train_fuse_linattn = params, fuse

    def P(self, key):
        return self.p[key]


KEYS = ("s.fn.norm.g", "s.fn.fn.to_qkv.weight", "s.fn.fn.to_out.0.weight", "s.fn.fn.to_out.0.bias", "s.fn.fn.to_out.1.g")


def _site(Cc, B, n, fuse, mode):
    x, g, wqkv, wo, bo, gp, dy = _inputs(Cc, B, 1, n)
    leaf = lambda t: t.to(DEV).requires_grad_()                     # noqa: E731
    params = dict(zip(KEYS, (leaf(g.reshape(1, Cc, 1)), leaf(wqkv.reshape(384, Cc, 1)), leaf(wo.reshape(Cc, 128, 1)), leaf(bo),
                             leaf(gp.reshape(1, Cc, 1)))))
    T = autograd.Trainer(_Site(params, fuse))
    xg = leaf(x.reshape(B, Cc, 1, 1, n))
    with T.step(torch.device(DEV)):
        y = T.linattn_lucid("s", xg, mode)
    return params, xg, y, dy.reshape(B, Cc, 1, 1, n)


def _site_run(Cc, B, n, fuse, mode):
    params, xg, y, dy = _site(Cc, B, n, fuse, mode)
    assert (type(y.grad_fn).__name__.startswith("LinAttnPostBlockFn")) == fuse
    (y * dy.to(DEV)).sum().backward()                                # a scalar loss whose gradient with respect to y is dy
    return [y.detach(), xg.grad] + [params[k].grad for k in KEYS]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("Cc", [64, 128])
def test_fused_node_against_chain(Cc, mode):
    B, n = 2, 128
    _, r = _case(Cc, B, 1, n, True, (mode, mode))
    ref = [r[0].reshape(B, Cc, 1, 1, n), r[1].reshape(B, Cc, 1, 1, n), r[2].reshape(1, Cc, 1), r[3].reshape(384, Cc, 1),
           r[4].reshape(Cc, 128, 1), r[5], r[6].reshape(1, Cc, 1)]
    chain, fused = _site_run(Cc, B, n, False, mode), _site_run(Cc, B, n, True, mode)
    names = ("y", "dx", "dg_pre", "dto_qkv", "dto_out", "dbias", "dg_post")
    ec, ef = [_rel(a, b) for a, b in zip(chain, ref)], [_rel(a, b) for a, b in zip(fused, ref)]
    print(f"[measured] Trainer.linattn_lucid C={Cc} mode={mode} B=2 n=128 vs fp64: fused " + " ".join(f"{n_} {e:.2e}" for n_, e in zip(names, ef))
          + " | chain " + " ".join(f"{n_} {e:.2e}" for n_, e in zip(names, ec)))
    for n_, a, b, k in zip(names[2:], fused[2:], chain[2:], KEYS):
        assert a.shape == b.shape, n_
    for a, b in zip(fused[:2], chain[:2]):
        assert a.shape == b.shape
    for i, (f_, c_) in enumerate(zip(ef, ec)):
        gate = Y_GATE if i == 0 else G_GATE
        assert f_ < gate and c_ < gate, names[i]


# ------------------------------------------------------------------ 7. whole nets
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


def _small_net(tree, B=2):
    if tree == "burgers":
        net, shape = sdc.Unet2D(dim=64, dim_mults=(1, 2), channels=3, resnet_block_groups=1), (3, 16, 16)
    else:
        net, shape = sdc.Unet1D(dim=64, dim_mults=(1, 2), channels=12, resnet_block_groups=1), (12, 128)
    net.load_state_dict(det_params([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 77))
    net.to(DEV).train()
    x, t = det_tensor((B, *shape), 78).to(DEV), torch.tensor([3, 400, 777, 999][:B], device=DEV)
    tgt, w = det_tensor((B, *shape), 79).to(DEV), (det_tensor((B,), 80).abs() + 0.5).to(DEV)
    return net, x, t, tgt, w


def _loss(net, x, t, tgt, w):
    return (w * ((net.forward_train(x, t) - tgt) ** 2).flatten(1).mean(1)).mean()


@functools.lru_cache(maxsize=None)
def _net_reference(tree):
    """loss and parameter gradients of the oracle's functional net under torch autograd on the inputs of _small_net, computed once"""
    from oracle import nets as onets
    net, x, t, tgt, w = _small_net(tree)
    fwd = onets.unet_burgers if tree == "burgers" else onets.unet_tokamak
    P = {k: v.detach().clone().requires_grad_() for k, v in net.state_dict().items()}
    ref = (w * ((fwd(P, x, t, dim=64, dim_mults=(1, 2)) - tgt) ** 2).flatten(1).mean(1)).mean()
    ref.backward()
    return ref.item(), {k: (None if v.grad is None else v.grad.detach()) for k, v in P.items()}


@pytest.mark.parametrize("tree", ["burgers", "tokamak"])
def test_whole_net_with_fused_post_blocks(tree, monkeypatch):
    net, x, t, tgt, w = _small_net(tree)
    shapes = []
    orig = autograd.Trainer.linattn_lucid
    monkeypatch.setattr(autograd.Trainer, "linattn_lucid", lambda self, p, h, mode: (shapes.append((p, tuple(h.shape))), orig(self, p, h, mode))[1])
    off = _loss(net, x, t, tgt, w)
    covered = [p for p, s in shapes if s[1] in (64, 128) and (s[2] * s[3] * s[4]) % 64 == 0 and s[0] < 65536]
    cores = _nodes(off, "LinAttnCoreFn")
    print(f"[measured] {tree} dim 64, dim_mults (1, 2): LinearAttention sites {shapes}")
    # burgers (16 x 16): downs.0.2 (64 wide, 256 tokens), downs.1.2 (64, 64), ups.0.2 (128, 64), ups.1.2 (64, 256);
    # tokamak (128): downs.0.2 (64 wide, 128 tokens), downs.1.2 (64, 64), ups.0.2 (128, 64), ups.1.2 (64, 128): all four covered
    assert sorted(covered) == ["downs.0.2", "downs.1.2", "ups.0.2", "ups.1.2"] and cores == len(shapes) == 4
    assert _nodes(off, "LinAttnPostBlockFn") == 0
    del off
    net.train_fuse_linattn = True
    loss = _loss(net, x, t, tgt, w)
    assert _nodes(loss, "LinAttnPostBlockFn") == len(covered) and _nodes(loss, "LinAttnCoreFn") == cores - len(covered)
    loss.backward()
    lref, G = _net_reference(tree)
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
    print(f"[measured] {tree} dim 64, dim_mults (1, 2), B=2, train_fuse_linattn: loss {loss.item():.6f} vs {lref:.6f}; {checked} parameter "
          f"gradients, worst relative L2 error {worst:.2e}")


# ------------------------------------------------------------------ 8. a no-op where nothing is covered
@pytest.mark.parametrize("tree", ["burgers", "tokamak"])
def test_switch_is_a_noop_on_the_dim8_nets(golden, tree):
    from test_gpu_finetune import _build
    g = golden(tree + "_grad")
    res = []
    for fuse in (False, True):
        net, gd, x0, noise = _build(tree, golden(tree + "_unet").spec())
        net.train()
        net.train_fuse_linattn = fuse
        loss_b = gd.p_losses(x0.to(DEV), g["t"].to(DEV), noise=noise.to(DEV), mean=False)
        total = (g["weight"].to(DEV) * loss_b).mean()
        assert _nodes(total, "LinAttnPostBlockFn") == 0
        total.backward()
        res.append((total.detach().clone(), [None if p.grad is None else p.grad.clone() for p in net.parameters()]))
    assert torch.equal(res[0][0], res[1][0])
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))


# ------------------------------------------------------------------ 9. graph replay
def test_graphed_step_with_fused_post_blocks():
    net, _, _, _, _ = _small_net("burgers")
    net.train_fuse_linattn = True
    gd = sdc.GaussianDiffusionBurgers(net, seq_length=(16, 16), timesteps=50, temporal=True, use_conv2d=True, is_condition_u0=True,
                                      is_condition_uT=True, condition_idx=10, train_on_padded_locations=False).to(DEV)
    shape = (3, 16, 16)
    state, noise = det_tensor((2, *shape), 42, 0.3).to(DEV), det_tensor((2, *shape), 45).to(DEV)
    w, t = torch.tensor([1.25, 0.75], device=DEV), torch.tensor([17, 33], device=DEV)
    params = [p for p in net.parameters() if p.requires_grad]

    def eager():
        for p in params:
            p.grad = None
        loss = (w * gd.p_losses(state, t, noise=noise, mean=False)).mean()
        assert _nodes(loss, "LinAttnPostBlockFn") == 4
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


# ------------------------------------------------------------------ 10. memory
def test_fused_post_node_saves_memory():
    Cc, B, n = 64, 8, 2048

    def peak(fuse):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        params, xg, y, dy = _site(Cc, B, n, fuse, 0)
        (y * dy.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base
    xbytes = B * Cc * n * 4
    chain, fused = peak(False), peak(True)
    print(f"[measured] one LinearAttention site C=64 B=8 n=2048 (x = {xbytes / 2**20:.1f} MiB), forward + backward peak allocated: "
          f"chain {chain / 2**20:.1f} MiB, fused {fused / 2**20:.1f} MiB")
    assert fused <= chain - 4 * xbytes
