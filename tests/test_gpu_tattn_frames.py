"""-m gpu: temporal attention at 64 / 96 / 128 frames on the matrix cores, both directions (csrc/sdc_tattn_frames.hip), through
grad_ops.attn_core / attn_core_bwd and Plan.attn, and the smoke nets around it at 64 frames.  Inputs and fp64 references come
from tests/tattn_frames_ref.py; tests/test_host_tattn_frames.py shows on the CPU that the references leave the gates a factor
of four and that the routing predicate sends every shape here to the frames kernels.  Gates: out 1e-5, dqkv / dbias 2e-5 by
_rel (tests/test_gpu_grad.py); max(gate, 4 e_fp32) for the qkv x 2 / x 4 cases (tests/test_gpu_grad_paths.py).  Pixels per
workgroup: 8 / 4 / 4 forward and 4 / 2 / 2 backward at 64 / 96 / 128 frames, so the shapes hold full groups, ragged tails (15
and 3 pixels) and more than one workgroup per head."""
import numpy as np
import pytest
import torch

import safediffcon_amd as sdc
import tattn_frames_ref as R
from oracle import nets as onets
from oracle import samplers as osam
from oracle import schedules as osched
from oracle.detweights import det_noise, det_params, det_tensor
from safediffcon_amd import _lib, grad_ops
from safediffcon_amd.engine import Plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SDC_EINVAL = -1
EPS_TOL = dict(rtol=5e-4, atol=5e-5)         # tests/test_gpu_models.py
TRAJ_GATE = 4e-4                             # its dim-8 smoke trajectory gate
BWD_PIXELS = {64: 4, 96: 2, 128: 2}          # pixels per workgroup of the backward kernels


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _run(qkv, bias, gout, rot=True, heads=None):
    """sdc_attn + sdc_attn_bwd on dense (B, 3 heads 32, F, H, W) inputs -> (out, dqkv, dbias | None) on the device"""
    B, C, Fr, H, W = qkv.shape
    heads = heads or C // 96
    qs, os_ = R.strides(heads, Fr, H * W)
    rt = R.rot_table(Fr)[0].to(DEV) if rot else None
    bg = bias.to(DEV) if bias is not None else None
    qg, gg = qkv.to(DEV), gout.to(DEV)
    out = torch.empty_like(gg)
    grad_ops.attn_core(qg, out, heads, B, H * W, Fr, qs, os_, rt, bg)
    dqkv, dbias = grad_ops.attn_core_bwd(qg, gg, heads, B, H * W, Fr, qs, os_, rt, bg)
    return out, dqkv, dbias


def _finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts if t is not None)


# ------------------------------------------------------------------ against fp64
@pytest.mark.parametrize("shape", R.SHAPES)
def test_core_against_fp64(shape):
    got = _run(*R.inputs(*shape))
    err = [R.rel(a, b) for a, b in zip(got, R.ref64("plain", *shape))]
    print(f"[measured] temporal attention core {shape}: out {err[0]:.2e} dqkv {err[1]:.2e} dbias {err[2]:.2e}")
    assert _finite(*got)
    assert err[0] < R.GATE_OUT and err[1] < R.GATE_GRAD and err[2] < R.GATE_GRAD


@pytest.mark.parametrize("use_rot,use_bias", [(False, True), (True, False), (False, False)])
def test_core_without_rot_or_bias(use_rot, use_bias):
    """rot null, bias null, both null at 64 frames (15 pixels); where bias is null dbias is None and the backward runs with
    work == null through the C ABI"""
    shape = (64, 3, 5, 1)
    qkv, bias, gout = R.inputs(*shape)
    bias = bias if use_bias else None
    ref = R.reference(qkv, bias, gout, use_rot=use_rot)
    got = _run(qkv, bias, gout, rot=use_rot)
    assert (got[2] is None) == (not use_bias)
    err = [R.rel(a, b) for a, b in zip(got, ref) if a is not None]
    print(f"[measured] temporal attention core {shape} rot {use_rot} bias {use_bias}: " + " ".join(f"{e:.2e}" for e in err))
    assert err[0] < R.GATE_OUT and all(e < R.GATE_GRAD for e in err[1:])
    # dbias == null and work == null through the C ABI: the same dqkv bits
    Fr, H, W, B = shape
    qs, os_ = R.strides(R.HEADS, Fr, H * W)
    qg, gg = qkv.to(DEV), gout.to(DEV)
    rt = R.rot_table(Fr)[0].to(DEV) if use_rot else None
    bg = bias.to(DEV) if use_bias else None
    dq = torch.full_like(qg, float("nan"))
    rc = _lib.get_lib().sdc_attn_bwd(qg.data_ptr(), gg.data_ptr(), 0 if rt is None else rt.data_ptr(), 0 if bg is None else bg.data_ptr(),
                                     dq.data_ptr(), 0, 0, B, H * W, R.HEADS, Fr, *qs, *os_, _stream())
    assert rc == 0, _lib.last_error()
    assert torch.equal(dq, got[1])


# ------------------------------------------------------------------ peaked inputs
@pytest.mark.parametrize("scale", [2.0, 4.0])
@pytest.mark.parametrize("shape", R.PEAKED)
def test_core_peaked(shape, scale):
    e32 = R.err32("plain", *shape, scale)
    got = _run(*R.inputs(*shape, scale))
    err = [R.rel(a, b) for a, b in zip(got, R.ref64("plain", *shape, scale))]
    print(f"[measured] temporal attention core, qkv x {scale:g}, {shape}: kernel out {err[0]:.2e} dqkv {err[1]:.2e} dbias {err[2]:.2e} "
          f"| fp32 torch out {e32[0]:.2e} dqkv {e32[1]:.2e} dbias {e32[2]:.2e}")
    assert _finite(*got)
    assert err[0] < R.gate(R.GATE_OUT, e32[0])
    assert err[1] < R.gate(R.GATE_GRAD, e32[1]) and err[2] < R.gate(R.GATE_GRAD, e32[2])


@pytest.mark.parametrize("shape", R.FAR)
def test_core_far_peak(shape):
    got = _run(*R.far_peak(*shape))
    err = [R.rel(a, b) for a, b in zip(got, R.ref64("far", *shape))]
    print(f"[measured] temporal attention core, far peak {shape}: out {err[0]:.2e} dqkv {err[1]:.2e} dbias {err[2]:.2e}")
    assert _finite(*got)
    assert err[0] < R.GATE_OUT and err[1] < R.GATE_GRAD and err[2] < R.GATE_GRAD


# ------------------------------------------------------------------ bit identity
@pytest.mark.parametrize("shape", [(64, 3, 5, 1), (128, 2, 4, 1)])
def test_plan_and_reruns_give_the_same_bits(shape):
    Fr, H, W, B = shape
    qkv, bias, gout = R.inputs(*shape)
    a, b = _run(qkv, bias, gout), _run(qkv, bias, gout)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    qs, os_ = R.strides(R.HEADS, Fr, H * W)
    plan = Plan(DEV)
    out = torch.zeros_like(a[0])
    plan.attn(qkv.to(DEV), out, R.HEADS, B, H * W, Fr, qs, os_, R.rot_table(Fr)[0].to(DEV), bias.to(DEV))
    plan.run(_stream())
    assert torch.equal(out, a[0])
    print(f"[measured] temporal attention core {shape}: Plan.attn == attn_core, two runs equal bits in out / dqkv / dbias")


def test_sample_alone_equals_sample_in_batch():
    Fr, H, W, B = 64, 3, 5, 3
    qkv, bias, gout = R.inputs(Fr, H, W, B)
    out, dqkv, _ = _run(qkv, bias, gout)
    out1, dqkv1, _ = _run(qkv[:1].contiguous(), bias, gout[:1].contiguous())
    assert torch.equal(out[:1], out1) and torch.equal(dqkv[:1], dqkv1)
    print("[measured] temporal attention core F=64 3x5: sample 0 of B = 3 equals the sample alone, out and dqkv")


# ------------------------------------------------------------------ past the slot cap
def test_backward_past_the_slot_cap():
    """heads = 1, 64 frames: the smallest `inner` with more pixel groups than workgroup slots, so the workgroup of slot 0 walks
    its group loop twice (its second group is ragged: one pixel)"""
    heads, Fr, np_ = 1, 64, BWD_PIXELS[64]
    cap = int(_lib.get_lib().sdc_attn_bwd_bytes(1, 4096, heads, Fr)) // (4 * heads * Fr * Fr)
    inner = cap * np_ + 1
    ngrp = -(-inner // np_)
    assert ngrp == cap + 1
    qkv, gout = det_tensor((1, 96, Fr, 1, inner), 140), det_tensor((1, 32, Fr, 1, inner), 142)
    bias = 0.5 * det_tensor((heads, Fr, Fr), 141)
    ref = R.reference(qkv, bias, gout)
    got = _run(qkv, bias, gout, heads=heads)
    err = [R.rel(a, b) for a, b in zip(got, ref)]
    print(f"[measured] temporal attention backward past the slot cap: inner {inner} ngrp {ngrp} cap {cap} out {err[0]:.2e} dqkv {err[1]:.2e} dbias {err[2]:.2e}")
    assert err[0] < R.GATE_OUT and err[1] < R.GATE_GRAD and err[2] < R.GATE_GRAD
    again = _run(qkv, bias, gout, heads=heads)
    assert all(torch.equal(x, y) for x, y in zip(got, again))
    # the groups cap .. ngrp - 1, each some workgroup's second iteration, cut out and run alone: the same dqkv bits
    # (one pixel copied out densely would have frame stride 1, which is the token-contiguous form and not this kernel's: the cut
    # keeps the tensors' strides and hands over the pointers of pixel i0 with inner = the pixels that are left)
    i0 = cap * np_
    qs, os_ = R.strides(heads, Fr, inner)
    qg, gg, bg, rt = qkv.to(DEV), gout.to(DEV), bias.to(DEV), R.rot_table(Fr)[0].to(DEV)
    lib = _lib.get_lib()
    dq_alone, db_alone = torch.zeros_like(qg), torch.empty_like(bg)
    work = torch.empty(int(lib.sdc_attn_bwd_bytes(1, inner - i0, heads, Fr)) // 4, device=DEV)
    rc = lib.sdc_attn_bwd(qg[..., i0:].data_ptr(), gg[..., i0:].data_ptr(), rt.data_ptr(), bg.data_ptr(), dq_alone[..., i0:].data_ptr(),
                          db_alone.data_ptr(), work.data_ptr(), 1, inner - i0, heads, Fr, *qs, *os_, _stream())
    assert rc == 0, _lib.last_error()
    assert torch.equal(dq_alone[..., i0:], got[1][..., i0:]) and not bool(dq_alone[..., :i0].any())


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("case", ["160 frames", "pixels two apart"])
def test_refused_bias_gradient_launches_nothing(case):
    heads, hw = 1, 8
    if case == "160 frames":
        Fr, q_si = 160, 1
    else:
        Fr, q_si = 64, 2
    qkv = det_tensor((1, 96, Fr, hw * q_si), 140).to(DEV)
    gout = det_tensor((1, 32, Fr, hw * q_si), 142).to(DEV)
    bias, rot = (0.5 * det_tensor((heads, Fr, Fr), 141)).to(DEV), R.rot_table(Fr)[0].to(DEV)
    qs, os_ = (96 * Fr * hw * q_si, Fr * hw * q_si, q_si, hw * q_si), (32 * Fr * hw * q_si, Fr * hw * q_si, q_si, hw * q_si)
    lib = _lib.get_lib()
    out, dqkv, dbias = torch.full_like(gout, 7.0), torch.full_like(qkv, 7.0), torch.full_like(bias, 7.0)
    work = torch.empty(int(lib.sdc_attn_bwd_bytes(1, hw, heads, Fr)) // 4, device=DEV)
    rc = lib.sdc_attn_bwd(qkv.data_ptr(), gout.data_ptr(), rot.data_ptr(), bias.data_ptr(), dqkv.data_ptr(), dbias.data_ptr(),
                          work.data_ptr(), 1, hw, heads, Fr, *qs, *os_, _stream())
    msg = _lib.last_error()
    torch.cuda.synchronize()
    assert rc == SDC_EINVAL and "64, 96 or 128 frames with contiguous pixels" in msg, (rc, msg)
    assert bool((out == 7.0).all()) and bool((dqkv == 7.0).all()) and bool((dbias == 7.0).all())
    print(f"[measured] refused bias gradient ({case}): SDC_EINVAL, '{msg}', outputs untouched")


# ------------------------------------------------------------------ the nets against the fixture of the real reference
def _fixture_net(g):
    net = sdc.Unet3D_with_Conv3D(dim=int(g.scalar("dim")), dim_mults=(1, 2, 4), channels=7)
    net.load_state_dict(det_params(g.spec(), int(g.scalar("weight_seed"))))
    Fr, S = int(g.scalar("frames")), int(g.scalar("image_size"))
    return net.to(DEV), det_tensor((1, Fr, 7, S, S), int(g.scalar("x_seed"))), (1, Fr, 7, S, S)


def test_net_forward_at_64_frames_vs_reference(golden):
    g = golden("smoke_unet_f64")
    net, x, _ = _fixture_net(g)
    eps = net(x.to(DEV), g["t"].to(DEV)).cpu()
    mse = ((eps - g["eps"]) ** 2).mean().item()
    print(f"[measured] smoke U-Net dim 8 at 64 frames vs the reference: eps MSE {mse:.2e} max|err| {(eps - g['eps']).abs().max().item():.2e}")
    assert mse <= 1e-5
    torch.testing.assert_close(eps, g["eps"], **EPS_TOL)


def test_net_training_step_at_64_frames_vs_reference(golden):
    """forward_train + backward of the stored loss: loss and the gradient of every parameter, the relative-position bias
    embedding among them, under the per-parameter gates of tests/test_gpu_finetune.py's fixture test"""
    g = golden("smoke_unet_f64")
    net, x, shape = _fixture_net(g)
    net.train()
    eps = net.forward_train(x.to(DEV), g["t"].to(DEV))
    target = det_tensor(shape, int(g.scalar("target_seed"))).to(DEV)
    loss = (g["w"].to(DEV) * ((eps - target) ** 2).flatten(1).mean(1)).mean()
    loss.backward()
    el = abs(loss.item() - g.scalar("loss")) / abs(g.scalar("loss"))
    assert el < 2e-5, (loss.item(), g.scalar("loss"))
    keys = [str(k) for k in g["grad_keys"]]
    params = dict(net.named_parameters())
    seed, gmax = int(g.scalar("dot_seed")), float(np.max(g.z["grad_norms"]))
    worst_n = worst_d = worst_f = 0.0
    checked = []
    for i, k in enumerate(keys):
        n_ref, d_ref = float(g.z["grad_norms"][i]), float(g.z["grad_dots"][i])
        if not params[k].requires_grad:                   # rotary freqs: not learnable, in the reference neither
            assert n_ref == 0.0 and k.endswith("rotary_emb.freqs"), k
            continue
        gr = params[k].grad
        assert gr is not None, f"no gradient for {k}"
        gr = gr.detach().double().cpu()
        if n_ref < 1e-4 * gmax:                           # zero in exact arithmetic: as small here as in the reference
            assert gr.norm().item() < 2e-4 * gmax, (k, gr.norm().item(), n_ref, gmax)
            continue
        en = abs(gr.norm().item() - n_ref) / n_ref
        proj = det_tensor(tuple(gr.shape), seed + i).double()
        ed = abs((gr * proj).sum().item() - d_ref) / (n_ref * proj.norm().item())
        worst_n, worst_d = max(worst_n, en), max(worst_d, ed)
        assert en < 5e-5 and ed < 5e-5, (k, en, ed, n_ref)
        if "grad:" + k in g.keys():
            full = g["grad:" + k].double()
            ef = ((gr - full).abs().max() / full.abs().max()).item()
            worst_f = max(worst_f, ef)
            assert ef < 1e-4, (k, ef)
        checked.append(k)
    assert "time_rel_pos_bias.relative_attention_bias.weight" in checked
    assert set(keys) == set(params)
    print(f"[measured] smoke fine-tune step at 64 frames vs the reference: loss rel err {el:.2e}; {len(checked)} gradients: worst norm err "
          f"{worst_n:.2e}, worst projection err {worst_d:.2e}, worst element err (stored tensors) {worst_f:.2e}")


# ------------------------------------------------------------------ samplers
def test_two_step_guided_sampler_at_64_frames(golden):
    g = golden("smoke_unet_f64")
    net, _, _ = _fixture_net(g)
    P = det_params(g.spec(), int(g.scalar("weight_seed")))
    T, B, Fr, S = 2, 1, 64, 8
    gs = sdc.GaussianDiffusionSmoke(net, image_size=S, frames=Fr, timesteps=T, standard_fixed_ratio=100.0).to(DEV)
    init = det_tensor((B, S, S), 43, 0.2).abs()
    noise = det_noise((B, Fr, 7, S, S), 7400)
    out = gs.sample(batch_size=B, design_fn=sdc.SmokeGuidance(0.01, 0.9, -5.0), init=init.to(DEV), noise=noise).cpu()
    ref = osam.sample_smoke(lambda a, b: onets.unet_smoke(P, a, b, dim=8, dim_mults=(1, 2, 4)), osched.make_tables("sigmoid", T), B, noise,
                            init=init, design_fn=osam.smoke_guidance(0.01, 0.9, -5.0), ratio=100.0, shape=(Fr, 7, S, S))
    err = (out - ref).abs().max().item()
    print(f"[measured] two-step guided smoke trajectory at 64 frames vs the oracle: max|err| {err:.3e} (gate {TRAJ_GATE:.1e})")
    assert _finite(out) and err < TRAJ_GATE
    # Philox noise: the graph replay and the eager call list give the same bits
    outs = []
    for use_graph in (True, False):
        gs.use_graph = use_graph
        torch.manual_seed(1234)
        outs.append(gs.sample(batch_size=B, design_fn=sdc.SmokeGuidance(0.01, 0.9, -5.0), init=init.to(DEV)))
    assert torch.equal(outs[0], outs[1])
