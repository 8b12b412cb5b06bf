"""-m gpu: fine-tuning with fp16 operands (net.train_precision 6 / 7; include/sdc.h "Fine-tuning with fp16 operands").

Conv level: wgrad_f16_kernel and the scaled data-gradient form of conv_f16_kernel against fp64 convs of the ROUNDED operands
(G 2^e -> fp16 RNE, X / W -> fp16 RNE) and of the exact ones; the device gradient scale.  Net level (dim 8): the three trees against
the reference gradient fixtures, determinism, graph replay, training curves."""
import math

import numpy as np
import pytest
import torch

import safediffcon_amd as sdc
from safediffcon_amd import autograd, grad_ops
from safediffcon_amd.engine import f16_tail
from oracle.detweights import det_params, det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rms(t):
    return t.double().pow(2).mean().sqrt().item()


def _host_exp(g):
    m = g.abs().max().item()
    if m == 0.0 or not math.isfinite(m):
        return 0
    _, E = math.frexp(m)                  # m = f 2^E, f in [0.5, 1)
    return max(-126, min(126, 15 - E))


def _wgrad_ref(g, x, k):
    """fp64 weight gradient of a stride-1 'same' conv: g (B, M, D, H, W), x (B, N, D, H, W) -> (M, N, *k)"""
    pad = tuple(kk // 2 for kk in k)
    return torch.nn.grad.conv3d_weight(x.double(), (g.shape[1], x.shape[1], *k), g.double(), padding=pad)


def _dgrad_ref(g, w, xshape):
    pad = tuple(kk // 2 for kk in w.shape[2:])
    return torch.nn.grad.conv3d_input(xshape, w.double(), g.double(), padding=pad)


# (name, k, B, N (Cin), M (Cout), D, H, W)
WG_SHAPES = [
    ("1d_rows16", (1, 1, 3), 3, 40, 24, 1, 1, 16),
    ("1d_rows128", (1, 1, 3), 2, 64, 72, 1, 1, 128),
    ("3x3_rows16", (1, 3, 3), 2, 32, 48, 1, 8, 16),
    ("3x3_rows64", (1, 3, 3), 3, 24, 64, 1, 4, 64),
    ("3x3_rows128", (1, 3, 3), 2, 16, 20, 1, 16, 128),
    ("3x3x3_rows16", (3, 3, 3), 2, 16, 40, 4, 16, 16),
    ("3x3x3_rows64", (3, 3, 3), 1, 24, 16, 3, 2, 64),
]


def _operands(k, B, N, M, D, H, W, seed, frame_major=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, D, H, W, generator=g)
    gy = torch.randn(B, M, D, H, W, generator=g) * 3e-7            # the size of a mean loss's per-element gradient
    if frame_major:                                                  # the smoke net's (B, F, C, H, W) storage, read as (B, C, F, H, W)
        x = x.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)
        gy = gy.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)
    return x, gy


def _check_wgrad(x, gy, k, label):
    xd, gd = x.to(DEV), gy.to(DEV)
    assert grad_ops.conv_wgrad_kernel(gd, xd, k, pad=tuple(kk // 2 for kk in k), precision=7).startswith("wgrad_f16_kernel"), label
    e = grad_ops.f16_grad_exponent(gd)
    ev = int(e[0].item())
    assert ev == _host_exp(gy), (ev, _host_exp(gy))
    pad = tuple(kk // 2 for kk in k)
    dw, db = grad_ops.conv_wgrad(gd, xd, k, pad=pad, bias=True, precision=7, exp=e)
    dw32, db32 = grad_ops.conv_wgrad(gd, xd, k, pad=pad, bias=True)
    dw, db = dw.cpu().double(), db.cpu()
    ref_r = _wgrad_ref((gy * 2.0 ** ev).half(), x.half(), k) * 2.0 ** -ev
    ref_x = _wgrad_ref(gy, x, k)
    er, ex = _rms(dw - ref_r) / _rms(ref_r), _rms(dw - ref_x) / _rms(ref_x)
    e32 = _rms(dw32.cpu().double() - ref_r) / _rms(ref_r)
    print(f"[measured] wgrad {label}: rms err vs rounded operands {er:.2e}, vs exact {ex:.2e} (fp32 kernel vs rounded {e32:.2e})")
    assert er <= 1e-5 and ex <= 1e-3, (label, er, ex)
    assert e32 > 10 * er                                            # the fp16 kernel ran: the fp32 one is far from the rounded reference
    # the bias gradient: an fp32 sum of the unscaled G, as the fp32 path's (to fp32 summation order: measured against sum |G|)
    gabs = gy.double().abs().sum((0, 2, 3, 4))
    assert ((db.double() - db32.cpu().double()).abs() <= 1e-6 * gabs).all()
    assert ((db.double() - gy.double().sum((0, 2, 3, 4))).abs() <= 1e-6 * gabs).all()
    return dw


@pytest.mark.parametrize("shape", WG_SHAPES, ids=[s[0] for s in WG_SHAPES])
def test_wgrad_f16_against_rounded_operands(shape):
    name, k, B, N, M, D, H, W = shape
    x, gy = _operands(k, B, N, M, D, H, W, seed=B * 1000 + N + M)
    _check_wgrad(x, gy, k, name)


def test_wgrad_f16_frame_major_view_and_concat_input():
    # the smoke net's frame-major layout: strided (b, c, f) views
    x, gy = _operands((3, 3, 3), 2, 24, 40, 8, 16, 16, seed=11, frame_major=True)
    assert not x.is_contiguous()
    _check_wgrad(x, gy, (3, 3, 3), "3x3x3 frame-major")
    # a concat conv: ConvFn.backward takes the weight gradient per input; every column is its own sum, so the halves are bit-equal
    # to the gradient over the concatenated input
    x, gy = _operands((1, 3, 3), 2, 40, 24, 1, 8, 64, seed=12)
    xd, gd = x.to(DEV), gy.to(DEV)
    e = grad_ops.f16_grad_exponent(gd)
    full, _ = grad_ops.conv_wgrad(gd, xd, (1, 3, 3), pad=(0, 1, 1), bias=False, precision=7, exp=e)
    a, _ = grad_ops.conv_wgrad(gd, xd[:, :24], (1, 3, 3), pad=(0, 1, 1), bias=False, precision=7, exp=e)
    b, _ = grad_ops.conv_wgrad(gd, xd[:, 24:], (1, 3, 3), pad=(0, 1, 1), bias=False, precision=7, exp=e)
    assert torch.equal(torch.cat((a, b), 1), full)
    _check_wgrad(x[:, 24:], gy, (1, 3, 3), "3x3 concat input (ragged 16 channels)")


def _dgrad(gd, w, e, prec=7):
    """dx of a stride-1 'same' conv with weight w through the scaled fp16 data-gradient conv (precision-8 flipped buffer)"""
    w5 = w.to(DEV)
    k = tuple(w5.shape[2:])
    wp = grad_ops.pack_conv_weight(w5, 8, flip=True)
    return autograd.conv_raw(gd, wp, None, w5.shape[1], k, pad=tuple(kk - 1 - kk // 2 for kk in k), prec=prec, gexp=e)


DG_SHAPES = [("1d_rows128", (1, 1, 3), 2, 48, 64, 1, 1, 128), ("3x3_rows64", (1, 3, 3), 2, 32, 40, 1, 4, 64),
             ("3x3x3_rows16", (3, 3, 3), 2, 16, 24, 4, 16, 16)]


@pytest.mark.parametrize("shape", DG_SHAPES, ids=[s[0] for s in DG_SHAPES])
def test_dgrad_f16_against_rounded_operands(shape):
    name, k, B, N, M, D, H, W = shape
    x, gy = _operands(k, B, N, M, D, H, W, seed=77 + N)
    w = torch.randn(M, N, *k, generator=torch.Generator().manual_seed(5)) * 0.1
    # the device packing of the flipped fp16 tail equals its torch restatement
    wp = grad_ops.pack_conv_weight(w.to(DEV), 8, flip=True).cpu()
    tail = f16_tail(w, flip=True)
    assert torch.equal(wp[wp.numel() - tail.numel():], tail)
    gd = gy.to(DEV)
    e = grad_ops.f16_grad_exponent(gd)
    ev = int(e[0].item())
    dx = _dgrad(gd, w, e).cpu().double()
    ref_r = _dgrad_ref((gy * 2.0 ** ev).half(), w.half(), x.shape) * 2.0 ** -ev
    ref_x = _dgrad_ref(gy, w, x.shape)
    er, ex = _rms(dx - ref_r) / _rms(ref_r), _rms(dx - ref_x) / _rms(ref_x)
    print(f"[measured] dgrad {name}: rms err vs rounded operands {er:.2e}, vs exact {ex:.2e}")
    assert er <= 1e-5 and ex <= 1e-3, (name, er, ex)


def test_gradient_scale_is_exact_and_propagates_nonfinite():
    k = (1, 3, 3)
    x, gy = _operands(k, 2, 32, 32, 1, 8, 64, seed=3)
    gy = gy / 3e-7                                                  # O(1) gradients: 2^-30 of them is below fp16's subnormals
    w = torch.randn(32, 32, *k, generator=torch.Generator().manual_seed(9)) * 0.1
    xd = x.to(DEV)

    def both(g):
        gd = g.to(DEV)
        e = grad_ops.f16_grad_exponent(gd)
        dw, _ = grad_ops.conv_wgrad(gd, xd, k, pad=(0, 1, 1), bias=False, precision=7, exp=e)
        return dw, _dgrad(gd, w, e), int(e[0].item())

    dw, dx, e0 = both(gy)
    dw2, dx2, e1 = both(gy * 2.0 ** -30)
    assert e1 == e0 + 30
    assert torch.equal(dw2, dw * 2.0 ** -30) and torch.equal(dx2, dx * 2.0 ** -30)
    # unscaled fp16 operands (e = 0) flush these gradients to zero
    gd = (gy * 2.0 ** -30).to(DEV)
    z = torch.zeros(grad_ops.F16_EXP_INTS, dtype=torch.int32, device=DEV)
    dwz, _ = grad_ops.conv_wgrad(gd, xd, k, pad=(0, 1, 1), bias=False, precision=7, exp=z)
    assert dwz.abs().max().item() == 0.0 and dw2.abs().max().item() > 0.0
    # inf / NaN in G: e = 0 and non-finite dw / dx (a GradScaler sees them)
    for bad in (float("nan"), float("inf")):
        g = gy.clone()
        g[1, 3, 0, 2, 17] = bad
        dwb, dxb, eb = both(g)
        assert eb == 0 and not torch.isfinite(dwb).all().item() and not torch.isfinite(dxb).all().item()
    assert int(grad_ops.f16_grad_exponent(torch.zeros(2, 4, 1, 1, 16, device=DEV))[0].item()) == 0


# ------------------------------------------------------------------------------------------------ net level
def _build(tree, spec):
    if tree == "burgers":
        net = sdc.Unet2D(dim=8, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1)
        net.load_state_dict(det_params(spec, 100))
        gd = sdc.GaussianDiffusionBurgers(net.to(DEV), seq_length=(16, 128), timesteps=1000, temporal=True, use_conv2d=True,
                                          is_condition_u0=True, is_condition_uT=True, condition_idx=10,
                                          train_on_padded_locations=False).to(DEV)
        x0, noise = det_tensor((3, 3, 16, 128), 5000, 0.3), det_tensor((3, 3, 16, 128), 5001)
    elif tree == "tokamak":
        net = sdc.Unet1D(dim=8, dim_mults=(1, 2, 4, 8), channels=12, resnet_block_groups=1)
        net.load_state_dict(det_params(spec, 200))
        gd = sdc.GaussianDiffusionTokamak(net.to(DEV), seq_length=128, nt=122, timesteps=1000, guidance_u0=True).to(DEV)
        x0, noise = det_tensor((3, 12, 128), 5010, 0.3), det_tensor((3, 12, 128), 5011)
    else:
        net = sdc.Unet3D_with_Conv3D(dim=8, dim_mults=(1, 2, 4), channels=7)
        net.load_state_dict(det_params(spec, 300))
        gd = sdc.GaussianDiffusionSmoke(net.to(DEV), image_size=16, frames=8, timesteps=1000, loss_type="l2",
                                        standard_fixed_ratio=100.0).to(DEV)
        x0, noise = det_tensor((3, 8, 7, 16, 16), 5020, 0.3), det_tensor((3, 8, 7, 16, 16), 5021)
    return net, gd, x0.to(DEV), noise.to(DEV)


def _step(net, gd, x0, t, noise, weight=None):
    net.zero_grad(set_to_none=True)
    loss_b = gd.p_losses(x0, t, noise=noise, mean=False)
    total = (loss_b if weight is None else weight * loss_b).mean()
    total.backward()
    return loss_b.detach(), total.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


# measured worst relative errors against the reference fixtures --- the gates are about twice these, at most 1e-2
# (gradients) / 1e-3 (loss)
GATES = {("burgers", 7): (1e-4, 4.8e-3), ("burgers", 6): (2.7e-4, 2e-3), ("tokamak", 7): (6.6e-4, 1.4e-3),
         ("tokamak", 6): (1e-5, 1e-5), ("smoke", 7): (2.4e-5, 2e-3), ("smoke", 6): (2.4e-5, 2e-3)}


@pytest.mark.parametrize("tp", [7, 6])
@pytest.mark.parametrize("tree", ["burgers", "tokamak", "smoke"])
def test_f16_finetune_vs_reference(golden, tree, tp):
    g = golden(tree + "_grad")
    net, gd, x0, noise = _build(tree, golden(tree + "_unet").spec())
    t, wgt = g["t"].to(DEV), g["weight"].to(DEV)
    x_probe, t_probe = x0[:2].clone(), torch.tensor([3, 700], device=DEV)
    with torch.no_grad():
        eps_before = net(x_probe, t_probe).clone()
    _, _, g4 = _step(net, gd, x0, t, noise, wgt)
    net.train_precision = tp
    loss_b, total, gr = _step(net, gd, x0, t, noise, wgt)
    loss_b2, _, gr2 = _step(net, gd, x0, t, noise, wgt)
    assert torch.equal(loss_b, loss_b2) and all(torch.equal(gr[k], gr2[k]) for k in gr)        # two eager steps: same bits
    with torch.no_grad():
        assert torch.equal(net(x_probe, t_probe), eps_before)                                       # the sampler call is untouched
    differs = any(not torch.equal(gr[k], g4[k]) for k in gr)
    el = ((loss_b.cpu() - g["loss_b"]).abs() / g["loss_b"].abs()).max().item()
    keys = [str(k) for k in g["grad_keys"]]
    params = dict(net.named_parameters())
    seed = int(g.scalar("dot_seed"))
    gmax = float(np.max(g.z["grad_norms"]))
    worst = 0.0
    for i, k in enumerate(keys):
        n_ref, d_ref = float(g.z["grad_norms"][i]), float(g.z["grad_dots"][i])
        if not params[k].requires_grad or n_ref < 1e-4 * gmax:
            continue
        x = gr[k].double().cpu()
        proj = det_tensor(tuple(x.shape), seed + i).double()
        en = abs(x.norm().item() - n_ref) / n_ref
        ed = abs((x * proj).sum().item() - d_ref) / (n_ref * proj.norm().item())
        worst = max(worst, en, ed)
    gl, gg = GATES[(tree, tp)]
    print(f"[measured] {tree} train_precision {tp}: loss rel err {el:.2e}, worst gradient rel err {worst:.2e}, "
          f"differs from precision 4: {differs}")
    assert el <= gl and worst <= gg, (el, worst)
    if tp == 7 or tree != "tokamak":      # (tokamak at 6: every 1-D conv of the dim-8 net is below the tables' thresholds)
        assert differs


def test_graphed_step_at_train_precision6_matches_eager(golden):
    from safediffcon_amd.train_graph import GraphedLossStep
    net, gd, x0, noise = _build("burgers", golden("burgers_unet").spec())
    net.train_precision = 6
    t = torch.tensor([5, 400, 900], device=DEV)
    step = GraphedLossStep(gd, x0, t=t, noise=noise)
    arena = net._trainer().arena
    assert arena.launch is not None and any(key[2] == 8 for key in arena.meta)       # fp16 layouts ride in the one pack launch
    params = step.params
    opt = torch.optim.Adam(params, lr=1e-3)

    def eager():
        for p in params:
            p.grad = None
        per = gd.p_losses(x0, t, noise=noise, mean=False)
        loss = (torch.ones(3, device=DEV) * per).mean()
        loss.backward()
        return loss.detach().clone(), [p.grad.clone() for p in params]

    for _ in range(2):
        lg = step().clone()
        gg = [g_.clone() for g_ in step.grads]
        le, ge = eager()
        assert torch.equal(lg, le) and all(torch.equal(a, b) for a, b in zip(gg, ge))
        for p, g_ in zip(params, gg):
            p.grad = g_
        opt.step()
    step.close()


def test_f16_training_curve_follows_precision4(golden):
    spec = golden("burgers_unet").spec()
    curves = {}
    for tp in (None, 6):
        net, gd, x0, noise = _build("burgers", spec)
        net.train_precision = tp
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        t = torch.tensor([50, 400, 800], device=DEV)
        losses = []
        for _ in range(20):
            opt.zero_grad(set_to_none=True)
            loss = gd.p_losses(x0, t, noise=noise, mean=False).mean()
            loss.backward()
            opt.step()
            losses.append(loss.item())
        curves[tp] = np.array(losses)
    rel = np.abs(curves[6] - curves[None]) / np.abs(curves[None])
    print(f"[measured] 20 Adam steps, burgers dim 8: loss {curves[None][0]:.4e} -> {curves[None][-1]:.4e} (precision 4) / "
          f"{curves[6][-1]:.4e} (train_precision 6), worst relative gap {rel.max():.2e}")
    assert rel.max() <= 1e-2
