"""-m gpu: softmax attention past 256 tokens (csrc/sdc_attn_long.hip: streaming forward, row statistics + dq + dk/dv
backward) through plan.attn and grad_ops.attn_core / attn_core_bwd, against float64 torch on the CPU.  Error measure and
gates are the core's own (tests/test_gpu_grad.py): _rel, forward < 1e-5, gradients < 2e-5.  The inputs are those of
tests/attn_long_ref.py; tests/test_host_attn_long.py shows on the CPU that they meet the forward gate in the reference
arithmetic.  Every case with more than 256 tokens was an SDC_EINVAL ("ntok=..., max 256") before the streaming kernels."""
import functools

import pytest
import torch

import attn_long_ref as R
import safediffcon_amd as sdc
from oracle import nets as onets
from oracle.detweights import det_params, det_tensor
from safediffcon_amd import _lib, grad_ops
from safediffcon_amd.engine import Plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_GATE, GRAD_GATE = 1e-5, 2e-5
EPS_TOL = dict(rtol=5e-4, atol=5e-5)          # the dim-8 forward tests of tests/test_gpu_models.py
SDC_EINVAL = -1


@functools.lru_cache(maxsize=None)
def _core_ref(shape):
    return R.reference(*R.core_inputs(*shape))


def _plan_attn(qkv, outer, inner, n, qs, os_):
    plan = Plan(DEV)
    out = torch.zeros(outer, 128, inner, n, device=DEV)
    plan.attn(qkv, out, R.HEADS, outer, inner, n, qs, os_)
    plan.run(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    torch.cuda.synchronize()
    return out


def _both(qkv, gout, outer, inner, n, qs=None, os_=None):
    """-> out through plan.attn (checked bit for bit against grad_ops.attn_core), dqkv through grad_ops.attn_core_bwd"""
    dq, do = R.strides(outer, inner, n)
    qs, os_ = qs or dq, os_ or do
    qg, gg = qkv.to(DEV), gout.to(DEV)
    out = _plan_attn(qg, outer, inner, n, qs, os_)
    out2 = grad_ops.attn_core(qg, torch.zeros_like(out), R.HEADS, outer, inner, n, qs, os_)
    assert torch.equal(out, out2)
    dqkv, dbias = grad_ops.attn_core_bwd(qg, gg, R.HEADS, outer, inner, n, qs, os_)
    assert dbias is None
    return out, dqkv


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_core_forward_and_backward(shape):
    outer, inner, n = shape
    out_ref, dq_ref = _core_ref(shape)
    out, dqkv = _both(*R.core_inputs(*shape), outer, inner, n)
    ef, eg = R.rel(out, out_ref), R.rel(dqkv, dq_ref)
    print(f"[measured] long attention core {shape}: out {ef:.2e} dqkv {eg:.2e}")
    assert ef < FWD_GATE and eg < GRAD_GATE


def test_core_in_the_1d_nets_layout():
    """mid_attn of the 1-D nets (unet.py _full_attn): inner = 1 with an `inner` stride of 0"""
    B, n = 2, 260
    qkv, gout = R.core_inputs(B, 1, n)
    out_ref, dq_ref = _core_ref((B, 1, n))
    out, dqkv = _both(qkv, gout, B, 1, n, (384 * n, n, 0, 1), (128 * n, n, 0, 1))
    ef, eg = R.rel(out, out_ref), R.rel(dqkv, dq_ref)
    print(f"[measured] long attention core, 1-D layout n={n}: out {ef:.2e} dqkv {eg:.2e}")
    assert ef < FWD_GATE and eg < GRAD_GATE


def test_peaked_rows_with_the_maximum_in_the_first_and_in_the_last_block():
    qkv, gout = R.peaked_inputs()
    out_ref, dq_ref = R.reference(qkv, gout)
    out, dqkv = _both(qkv, gout, 1, 2, 320)
    ef, eg = R.rel(out, out_ref), R.rel(dqkv, dq_ref)
    print(f"[measured] long attention core, q x 8 (rows close to one-hot) n=320: out {ef:.2e} dqkv {eg:.2e}")
    assert ef < FWD_GATE and eg < GRAD_GATE


def test_zero_queries_give_uniform_rows():
    """q = 0: every row of P is 1/n, so out is the mean of v over the tokens and dk = sum_i dS_ij q_i vanishes.  (dq does not
    vanish here -- it is scale * dO_i^T Cov_j(v_j, k_j), a sample covariance of order n^-1/2 -- so dq is held to the float64
    reference with the rest of dqkv, and the exact zero is asserted on dk, relative to dv's scale.)"""
    qkv, gout = R.zero_q_inputs()
    out_ref, dq_ref = R.reference(qkv, gout)
    out, dqkv = _both(qkv, gout, 1, 2, 320)
    mean_v = qkv[:, 256:].mean(-1, keepdim=True).expand(-1, -1, -1, 320)
    em, ef, eg = R.rel(out, mean_v), R.rel(out, out_ref), R.rel(dqkv, dq_ref)
    dv_scale = dq_ref[:, 256:].abs().max().item()
    ek = dqkv[:, 128:256].abs().max().item() / dv_scale
    print(f"[measured] long attention core, q = 0 n=320: out vs mean(v) {em:.2e}, vs float64 {ef:.2e}; dqkv {eg:.2e}; |dk| / |dv| {ek:.2e}")
    assert em < FWD_GATE and ef < FWD_GATE and eg < GRAD_GATE and ek < GRAD_GATE


def test_a_sample_does_not_depend_on_the_batch_it_rides_in():
    n, inner = 320, 2
    qkv, gout = (det_tensor((3, 384, inner, n), 63) * 1.2).to(DEV), det_tensor((3, 128, inner, n), 153).to(DEV)
    qs3, os3 = R.strides(3, inner, n)
    out3 = grad_ops.attn_core(qkv, torch.zeros(3, 128, inner, n, device=DEV), R.HEADS, 3, inner, n, qs3, os3)
    d3, _ = grad_ops.attn_core_bwd(qkv, gout, R.HEADS, 3, inner, n, qs3, os3)
    q1, g1 = qkv[:1].contiguous(), gout[:1].contiguous()
    qs1, os1 = R.strides(1, inner, n)
    out1 = grad_ops.attn_core(q1, torch.zeros(1, 128, inner, n, device=DEV), R.HEADS, 1, inner, n, qs1, os1)
    d1, _ = grad_ops.attn_core_bwd(q1, g1, R.HEADS, 1, inner, n, qs1, os1)
    assert torch.equal(out3[:1], out1) and torch.equal(d3[:1], d1)


def test_two_runs_give_the_same_bits():
    shape = (2, 3, 257)
    qkv, gout = R.core_inputs(*shape)
    a, b = _both(qkv, gout, *shape), _both(qkv, gout, *shape)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _refusal_cases():
    n = 300
    qs, os_ = R.strides(1, 2, n)
    rot, bias = torch.zeros(n * 32, device=DEV), torch.zeros(R.HEADS, n, n, device=DEV)
    big = R.CAP + 1
    return [("rot", n, qs, os_, rot, None), ("bias", n, qs, os_, None, bias),
            ("strided tokens", n, (384 * 2 * n, 2 * n, 1, 2), (128 * 2 * n, 2 * n, 1, 2), None, None),
            ("cap + 1", big, *R.strides(1, 2, big), None, None)]


@pytest.mark.parametrize("idx", range(4), ids=["rot", "bias", "strided", "cap+1"])
def test_outside_the_domain_is_refused_before_any_launch(idx):
    tag, n, qs, os_, rot, bias = _refusal_cases()[idx]
    lib = _lib.get_lib()
    qkv = torch.ones(1, 384, 2, n, device=DEV)
    out, dqkv = torch.full((1, 128, 2, n), 7.5, device=DEV), torch.full((1, 384, 2, n), 7.5, device=DEV)
    dout, work = torch.ones(1, 128, 2, n, device=DEV), torch.empty(1 << 16, device=DEV)
    dbias = None if bias is None else torch.full_like(bias, 7.5)
    p = lambda t: 0 if t is None else t.data_ptr()
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    rc = lib.sdc_attn(p(qkv), p(out), p(rot), p(bias), 1, 2, R.HEADS, n, *qs, *os_, stream)
    msg = _lib.last_error()
    assert rc == SDC_EINVAL and "256" in msg and str(R.CAP) in msg and "contiguous" in msg, (tag, rc, msg)
    rc = lib.sdc_attn_bwd(p(qkv), p(dout), p(rot), p(bias), p(dqkv), p(dbias), p(work), 1, 2, R.HEADS, n, *qs, *os_, stream)
    msg = _lib.last_error()
    assert rc == SDC_EINVAL and "256" in msg and str(R.CAP) in msg and "contiguous" in msg, (tag, rc, msg)
    torch.cuda.synchronize()
    assert (out == 7.5).all() and (dqkv == 7.5).all() and (dbias is None or (dbias == 7.5).all())


@pytest.mark.parametrize("shape", [(2, 2, 256), (3, 1, 32)], ids=str)
def test_the_old_domain_still_meets_the_gates(shape):
    outer, inner, n = shape
    out_ref, dq_ref = _core_ref(shape)
    out, dqkv = _both(*R.core_inputs(*shape), outer, inner, n)
    ef, eg = R.rel(out, out_ref), R.rel(dqkv, dq_ref)
    print(f"[measured] attention core up to 256 tokens {shape}: out {ef:.2e} dqkv {eg:.2e}")
    assert ef < FWD_GATE and eg < GRAD_GATE


# ------------------------------------------------------------------------------------------------ the nets
def _net(cls, seed, **kw):
    net = cls(**kw)
    P = det_params([(k, tuple(v.shape)) for k, v in net.state_dict().items()], seed)
    net.load_state_dict(P)
    return net.to(DEV), P


@functools.lru_cache(maxsize=None)
def _smoke80():
    net, P = _net(sdc.Unet3D_with_Conv3D, 310, dim=8, dim_mults=(1, 2, 4), channels=7)
    return net, P, det_tensor((2, 4, 7, 80, 80), 311), torch.tensor([3, 700])


def test_smoke_net_forward_at_80x80():
    """400 mid tokens: net(x, t) (the sampler plan) against the CPU oracle, under the gate of test_unet_smoke_golden"""
    net, P, x, t = _smoke80()
    eps = net(x.to(DEV), t.to(DEV)).cpu()
    ref = onets.unet_smoke(P, x, t, dim=8, dim_mults=(1, 2, 4))
    mse = ((eps - ref) ** 2).mean().item()
    print(f"[measured] smoke U-Net dim 8 at 80 x 80 x 4 frames, B = 2: eps-MSE {mse:.2e}, max|err| {(eps - ref).abs().max().item():.2e}")
    assert mse <= 1e-5
    torch.testing.assert_close(eps, ref, **EPS_TOL)


def test_smoke_net_training_step_at_80x80():
    """forward_train + backward against torch autograd over the oracle's functional net (CPU), gates of
    test_finetune_gradients_at_production_width: loss 1e-5 relative, every parameter gradient 2e-4 in relative L2"""
    net, P, x, t = _smoke80()
    net.train()
    net.zero_grad(set_to_none=True)
    tgt, w = det_tensor(tuple(x.shape), 312), det_tensor((2,), 313).abs() + 0.5
    loss = (w.to(DEV) * ((net.forward_train(x.to(DEV), t.to(DEV)) - tgt.to(DEV)) ** 2).flatten(1).mean(1)).mean()
    loss.backward()
    Pr = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in P.items()}
    ref = (w * ((onets.unet_smoke(Pr, x, t, dim=8, dim_mults=(1, 2, 4)) - tgt) ** 2).flatten(1).mean(1)).mean()
    ref.backward()
    el = abs(loss.item() - ref.item()) / abs(ref.item())
    gmax = max(v.grad.norm().item() for v in Pr.values() if v.grad is not None)
    worst, checked = 0.0, 0
    for k, p in net.named_parameters():
        if not p.requires_grad:
            continue
        gr, gref = p.grad, Pr[k].grad
        assert gr is not None and gref is not None, k
        n_ref = gref.norm().item()
        if n_ref < 1e-4 * gmax:              # zero in exact arithmetic: rounding noise on both sides
            assert gr.norm().item() < 2e-4 * gmax, k
            continue
        err = ((gr.cpu() - gref).norm() / n_ref).item()
        worst, checked = max(worst, err), checked + 1
        assert err < 2e-4, (k, err)
    print(f"[measured] smoke U-Net dim 8 at 80 x 80 training step: loss rel err {el:.2e}; {checked} parameter gradients, "
          f"worst relative L2 error {worst:.2e}")
    assert el < 1e-5 and checked > 0


def test_burgers_net_forward_on_a_1040_wide_grid():
    """260 mid tokens: net(x, t) against the CPU oracle, under the gate of test_unet_burgers_golden"""
    net, P = _net(sdc.Unet2D, 320, dim=8, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1)
    x, t = det_tensor((1, 3, 16, 1040), 321), torch.tensor([500])
    eps = net(x.to(DEV), t.to(DEV)).cpu()
    ref = onets.unet_burgers(P, x, t, dim=8)
    mse = ((eps - ref) ** 2).mean().item()
    print(f"[measured] Burgers U-Net dim 8 on a (16, 1040) grid, B = 1: eps-MSE {mse:.2e}, max|err| {(eps - ref).abs().max().item():.2e}")
    assert mse <= 1e-5
    torch.testing.assert_close(eps, ref, **EPS_TOL)
