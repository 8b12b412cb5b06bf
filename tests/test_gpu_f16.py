"""-m gpu: precisions 6 / 7 (opt-in, samplers only) -- the stride-1 pad-1 3-tap convs on the fp16 matrix pipe (csrc/sdc_conv_f16.hip):
fp16 operands (RNE), fp32 accumulation.  The kernel itself is tested through precision 7, the test and measurement hook that runs it on
every covered conv; precision 6 runs it where its measured dispatch table has it ahead of precision 4's kernels.  Conv level: against an fp64 conv of the ROUNDED operands (only the fp32 accumulation order
may differ) and of the exact ones; net level: the eps-MSE contract gate against the reference fixtures, determinism, graph replay,
batch invariance; and nothing else moves (fine-tuning keeps precision 4's bits)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import safediffcon_amd as sdc
from safediffcon_amd import _lib
from safediffcon_amd.engine import Plan, as5
from oracle.detweights import det_noise, det_params, det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# max |x_0 - reference| over the 8-step guided trajectories at precision 7 (every covered conv in fp16), per tree: twice the error measured
# on MI355X (printed by test_f16_guided_trajectories, `pytest -s`).  (Precision 4's gate is 4e-4: the clipped 8-step DDPM loop carries
# an eps error into x_0 amplified by 1 / sqrt(alpha_bar) at its noisiest steps.)
TRAJ7_GATE = {"burgers": 6e-2, "tokamak": 4e-2, "smoke": 7.5e-2}      # measured 2.8e-2 / 2.0e-2 / 3.7e-2


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _describe(d):
    name = C.create_string_buffer(96)
    share = C.c_double(0.0)
    _lib.check(_lib.get_lib().sdc_conv_describe(C.byref(d), name, 96, C.byref(share)), "describe")
    return name.value.decode(), share.value


def _plan_kernels(plan):
    """kernel names sdc_conv_describe gives for every sdc_conv / sdc_conv_gn call of a plan"""
    out = []
    for fn, args in plan.calls:
        if fn.__name__ in ("sdc_conv", "sdc_conv_gn"):
            out.append(_describe(args[0]._obj)[0])
    return out


# (B, Cin0, Cin1, Cout, (D, H, W), (kD, kH, kW), residual, frame_major)
FORMS = {
    "conv1d_L128_cin256": (4, 256, 0, 256, (1, 1, 128), (1, 1, 3), False, False),
    "conv1d_L16_cin2048": (8, 2048, 0, 256, (1, 1, 16), (1, 1, 3), False, False),
    "conv2d_rows128": (2, 64, 0, 128, (1, 16, 128), (1, 3, 3), False, False),
    "conv2d_rows16": (4, 512, 0, 512, (1, 2, 16), (1, 3, 3), False, False),
    "conv3d_rows64": (1, 64, 0, 128, (4, 8, 64), (3, 3, 3), False, False),
    "conv3d_rows16_concat512": (1, 256, 256, 256, (2, 16, 16), (3, 3, 3), False, False),
    "concat_residual": (2, 24, 40, 96, (1, 8, 32), (1, 3, 3), True, False),
    "ragged_cin_cout_1d": (3, 20, 0, 40, (1, 1, 64), (1, 1, 3), True, False),
    "frame_major_3d": (2, 32, 0, 64, (4, 16, 16), (3, 3, 3), False, True),
    "dim8_3d": (2, 8, 8, 8, (4, 16, 16), (3, 3, 3), False, False),
}


def _input(B, C_, D, H, W, seed, frame_major):
    g = torch.Generator().manual_seed(seed)
    if frame_major:
        x = (torch.randn(B, D, C_, H, W, generator=g) * 2.0).to(DEV).permute(0, 2, 1, 3, 4)     # (B, C, F, H, W) view of (B, F, C, H, W)
    else:
        x = (torch.randn(B, C_, D, H, W, generator=g) * 2.0).to(DEV)
    return x


@pytest.mark.parametrize("form", list(FORMS))
def test_f16_conv_is_rne_operands_with_fp32_accumulation(form):
    B, c0, c1, co, (D, H, W), k, res, fm = FORMS[form]
    g = torch.Generator().manual_seed(11)
    x0 = _input(B, c0, D, H, W, 1, fm)
    x1 = _input(B, c1, D, H, W, 2, fm) if c1 else None
    w = torch.randn(co, c0 + c1, *k, generator=g) / (3.0 * ((c0 + c1) * k[0] * k[1] * k[2]) ** 0.5)
    bias = (0.1 * torch.randn(co, generator=g)).to(DEV)
    r = (torch.randn(B, co, D, H, W, generator=g)).to(DEV) if res else None
    plan = Plan(DEV, precision=7)
    wp = plan.conv_weight(w.to(DEV))
    pad = (k[0] // 2, k[1] // 2, 1)
    out = plan.conv(x0, wp, bias, co, k, x1=x1, pad=pad, residual=r)
    plan.run(_stream())
    torch.cuda.synchronize()
    names = _plan_kernels(plan)
    assert names and all("f16" in n for n in names), names
    assert _describe(plan.calls[-1][1][0]._obj)[1] == 1.0

    xc = torch.cat([x0, x1], 1) if x1 is not None else x0
    xc, out = xc.double().cpu(), out.double().cpu()
    extra = bias.double().cpu().view(1, -1, 1, 1, 1) + (r.double().cpu() if res else 0.0)
    ref_r = F.conv3d(xc.half().double(), w.half().double(), padding=pad) + extra
    ref_x = F.conv3d(xc, w.double(), padding=pad) + extra
    rms = ref_r.pow(2).mean().sqrt().item()
    e_r = (out - ref_r).pow(2).mean().sqrt().item() / rms
    e_x = (out - ref_x).pow(2).mean().sqrt().item() / rms
    print(f"[measured] {form}: rms err vs rounded-operand fp64 {e_r:.2e}, vs exact fp64 {e_x:.2e} (of the output rms)")
    assert e_r <= 1e-5, e_r
    assert e_x <= 1e-3, e_x


@pytest.mark.parametrize("shape,G", [((2, 64, 128, (1, 16, 128), (1, 3, 3)), 1), ((2, 256, 256, (1, 1, 128), (1, 1, 3)), 32),
                                     ((1, 64, 128, (4, 16, 16), (3, 3, 3)), 8)])
def test_f16_conv_gn_partial_sums_match_gn_stats(shape, G):
    B, ci, co, (D, H, W), k = shape
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B, ci, D, H, W, generator=g)).to(DEV)
    w = (torch.randn(co, ci, *k, generator=g) / (ci * k[0] * k[1] * k[2]) ** 0.5).to(DEV)
    bias = (0.3 + 0.1 * torch.randn(co, generator=g)).to(DEV)
    plan = Plan(DEV, precision=7)
    out = plan.conv(x, plan.conv_weight(w), bias, co, k, pad=(k[0] // 2, k[1] // 2, 1), gn_groups=G)
    assert plan.calls[-1][0].__name__ == "sdc_conv_gn" and "f16" in _plan_kernels(plan)[-1]
    parts, nparts, _ = plan._gn_parts[out.data_ptr()]
    plan.run(_stream())
    lib = _lib.get_lib()
    S = D * H * W
    nb = (int(lib.sdc_gn_stats_bytes(B, G)) + 3) // 4
    st1 = torch.zeros(nb, device=DEV)
    st2 = torch.zeros(nb, device=DEV)
    _lib.check(lib.sdc_gn_finalize(parts.data_ptr(), st1.data_ptr(), B, G, nparts, (co // G) * S, 1e-5, _stream()), "finalize")
    _lib.check(lib.sdc_gn_stats(out.data_ptr(), st2.data_ptr(), B, co, G, S, 1e-5, _stream()), "stats")
    torch.cuda.synchronize()
    a, b = st1[:2 * B * G].view(B * G, 2).double().cpu(), st2[:2 * B * G].view(B * G, 2).double().cpu()
    sd = 1.0 / b[:, 1]
    assert ((a[:, 0] - b[:, 0]).abs() / sd).max().item() <= 1e-6
    assert ((a[:, 1] - b[:, 1]).abs() / b[:, 1]).max().item() <= 1e-6


# ------------------------------------------------------------------ net level
def _nets():
    return {
        "burgers": (lambda d: sdc.Unet2D(dim=d, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1), (2, 3, 16, 128)),
        "tokamak": (lambda d: sdc.Unet1D(dim=d, dim_mults=(1, 2, 4, 8), channels=12, resnet_block_groups=1), (2, 12, 128)),
        "smoke": (lambda d: sdc.Unet3D_with_Conv3D(dim=d, dim_mults=(1, 2, 4), channels=7), None),
    }


@pytest.mark.parametrize("tree", ["burgers", "tokamak", "smoke"])
def test_f16_nets_against_reference_fixtures(golden, tree):
    """precision 7 (every covered conv in fp16) and 6 (the dispatch table's convs): the contract gate, graph replay == eager, two runs
    bit-identical, a sample's eps independent of its batch; precision 6 runs the fp16 kernel on every tree at one of the two widths"""
    make, shape = _nets()[tree]
    wide_dim = {"burgers": 64, "tokamak": 256, "smoke": 64}[tree]
    seed8 = {"burgers": 100, "tokamak": 200, "smoke": 300}[tree]
    n_f16 = {6: 0, 7: 0}
    for fx, dim in ((f"{tree}_unet", 8), (f"{tree}_unet_wide", wide_dim)):
        g = golden(fx)
        net = make(dim)
        net.load_state_dict(det_params(g.spec(), seed8 if dim == 8 else int(g.scalar("weight_seed"))))
        net.to(DEV)
        if dim == 8:
            x = g["x"]
        else:
            x = det_tensor((1, 32, 7, 32, 32) if tree == "smoke" else shape, int(g.scalar("x_seed")))
        x, t = x.to(DEV), g["t"].to(DEV)
        for prec in (7, 6):
            net.precision = prec
            net.forward_graph = True
            eps = net(x, t).cpu()
            mse = ((eps - g["eps"]) ** 2).mean().item()
            print(f"[measured] {fx} precision {prec}: eps-MSE {mse:.3e}  max|err| {(eps - g['eps']).abs().max().item():.3e}")
            assert torch.isfinite(eps).all()
            assert mse <= 1e-5
            n_f16[prec] += sum("f16" in n for n in _plan_kernels(net.entry(tuple(x.shape), x.shape[0])["plan"]))
            # graph replay == eager call list, and two runs bit-identical
            net.forward_graph = False
            eager = net(x, t).cpu()
            net.forward_graph = True
            assert torch.equal(eager, eps) and torch.equal(net(x, t).cpu(), eps)
            # a sample's eps does not depend on the batch it rides in
            one = net(x[:1], t[:1]).cpu()
            assert torch.equal(one[0], eps[0])
    assert n_f16[7] > 0 and n_f16[6] > 0, n_f16


def _traj(out, ref, tag, errs):
    err = (out - ref).abs().max().item()
    print(f"[measured] trajectory {tag} precision 7: max|err| {err:.3e}  (gate {TRAJ7_GATE[tag]:.1e})")
    assert torch.isfinite(out).all()
    errs[tag] = err


def test_f16_guided_trajectories(golden):
    errs = {}
    spec = golden("burgers_unet").spec()
    g = golden("burgers_traj_guided")
    net = sdc.Unet2D(dim=8, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1)
    net.load_state_dict(det_params(spec, 100))
    net.to(DEV).precision = 7
    gd = sdc.GaussianDiffusionBurgers(net, seq_length=(16, 128), timesteps=8, temporal=True, use_conv2d=True,
                                      is_condition_u0=True, is_condition_uT=True, condition_idx=10,
                                      train_on_padded_locations=False).to(DEV)
    noise = det_noise((2, 3, 16, 128), int(g.scalar("noise_seed")))
    guid = sdc.BurgersGuidance(g.scalar("Q"), g.scalar("w_score"), g.scalar("u_bound"))
    out = gd.sample(batch_size=2, clip_denoised=True, u_init=g["u0"], u_final=g["uT"], guidance_u0=True, nablaJ=guid,
                    J_scheduler=lambda t: 1.0, w_scheduler=None, enable_grad=False, noise=noise).cpu()
    _traj(out, g["out"], "burgers", errs)

    spec = golden("tokamak_unet").spec()
    g = golden("tokamak_traj_guided")
    net = sdc.Unet1D(dim=8, dim_mults=(1, 2, 4, 8), channels=12, resnet_block_groups=1)
    net.load_state_dict(det_params(spec, 200))
    net.to(DEV).precision = 7
    gd = sdc.GaussianDiffusionTokamak(net, seq_length=128, nt=122, timesteps=8, guidance_u0=True).to(DEV)
    noise = det_noise((2, 12, 128), int(g.scalar("noise_seed")))
    guid = sdc.TokamakGuidance(g["target"], 122, g.scalar("w_obj"), g.scalar("w_safe"), g.scalar("scaler"), g.scalar("Q"),
                               g.scalar("thr"))
    out = gd.sample(batch_size=2, clip_denoised=True, guidance_u0=True, u_init=g["u0"], u_final=g["uT"], nablaJ=guid,
                    J_scheduler=lambda t: 1.0, w_scheduler=None, enable_grad=False, noise=noise).cpu()
    _traj(out, g["out"], "tokamak", errs)

    spec = golden("smoke_unet").spec()
    g = golden("smoke_traj_guided")
    net = sdc.Unet3D_with_Conv3D(dim=8, dim_mults=(1, 2, 4), channels=7)
    net.load_state_dict(det_params(spec, 300))
    net.to(DEV).precision = 7
    gd = sdc.GaussianDiffusionSmoke(net, image_size=16, frames=8, timesteps=8, loss_type="l2",
                                    standard_fixed_ratio=g.scalar("ratio")).to(DEV)
    noise = det_noise((2, 8, 7, 16, 16), int(g.scalar("noise_seed")))
    guid = sdc.SmokeGuidance(g.scalar("Q"), g.scalar("w_safe"), g.scalar("safe_bound"))
    out = gd.sample(batch_size=2, design_fn=guid, enable_grad=False, init=g["init"], noise=noise).cpu()
    _traj(out, g["out"], "smoke", errs)
    assert all(errs[k] < TRAJ7_GATE[k] for k in errs), errs


def test_f16_leaves_fine_tuning_and_precision4_untouched(golden):
    spec = golden("burgers_unet").spec()
    P = det_params(spec, 100)
    x = det_tensor((2, 3, 16, 128), 3).to(DEV)
    t = torch.tensor([3, 700], device=DEV)
    res = {}
    for prec in (4, 6, 7):
        net = sdc.Unet2D(dim=8, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1)
        net.load_state_dict(P)
        net.to(DEV).precision = prec
        loss = (net.forward_train(x, t) ** 2).mean()
        loss.backward()
        res[prec] = (loss.detach().cpu(), [None if p.grad is None else p.grad.detach().cpu().clone() for p in net.parameters()])
    assert any(a is not None for a in res[4][1])
    for prec in (6, 7):
        assert torch.equal(res[4][0], res[prec][0])
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(res[4][1], res[prec][1]))
    # a net switched 4 -> 7 -> 4 reproduces precision 4's eps bits
    net = sdc.Unet2D(dim=8, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1)
    net.load_state_dict(P)
    net.to(DEV)
    e4 = net(x, t).clone()
    net.precision = 7
    e7 = net(x, t).clone()
    net.precision = 4
    assert torch.equal(net(x, t), e4) and not torch.equal(e7, e4)


def test_f16_device_packing_equals_host_packing():
    lib = _lib.get_lib()
    for shape in ((40, 20, 1, 1, 3), (64, 48, 1, 3, 3), (24, 40, 3, 3, 3)):
        w = torch.randn(*shape, device=DEV)
        n = int(lib.sdc_pack_conv_weight_floats(*shape, 6))
        assert n == int(lib.sdc_pack_conv_weight_floats(*shape, 7))
        out = torch.full((n,), float("nan"), device=DEV)
        _lib.check(lib.sdc_pack_conv_weight(w.data_ptr(), out.data_ptr(), *shape, 6, 0, _stream()), "pack")
        torch.cuda.synchronize()
        from safediffcon_amd.engine import pack_conv_weight
        host = pack_conv_weight(w, precision=6)
        n4 = (int(lib.sdc_pack_conv_weight_floats(*shape, 4)) + 3) // 4 * 4
        assert out.numel() == host.numel()
        assert torch.equal(out[n4:].view(torch.float16), host[n4:].view(torch.float16))      # the fp16 tail bit for bit
        torch.testing.assert_close(out[:n4], host[:n4], rtol=1e-6, atol=1e-7)              # (the fp32 Winograd taps: fp64 sum order)
