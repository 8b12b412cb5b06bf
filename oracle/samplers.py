"""Oracle: DDPM reverse loops, guidance gradients and conformal reductions.

Restates (file:line relative to /root/reference)
  burgers  p_sample_loop 1D/model/diffusion.py:368-449, p_sample :299-306,
           model_predictions :226-286, q_posterior :217-224,
           set_condition :336-358, set_pad_condition :360-366
  tokamak  p_sample_loop tokamak/model/diffusion.py:310-372, set_condition :295-308
  smoke    p_sample_loop 2d/ddpm/diffusion_2d.py:288-322, p_sample :275-285,
           model_predictions :242-261
  guidance 1D/utils/guidance.py:58-85, tokamak/utils/guidance.py:32-73,
           2d/inference_2d.py:173-195
  conformal 1D/inference/conformal.py:68-117, 1D/inference/guidance.py:39-66,
           tokamak/inference/conformal.py:103-145, tokamak/utils/guidance.py:98-148,
           2d/inference_2d.py:83-165

RNG protocol: every sampler takes ``noise(i)`` -> tensor; i = 0 is the x_T draw
and i >= 1 are the per-step draws in the order the reference makes them (after
the U-Net forward, none at t == 0; the burgers/tokamak calibration branch makes
two draws per step and discards the first, 1D/model/diffusion.py:421-423).

TEST INFRASTRUCTURE -- see oracle/__init__.py.
"""
import math

import numpy as np
import torch

BURGERS_SCALER = 10.0                                                    # 1D/utils/common.py:17
TOKAMAK_SCALER = torch.tensor([2, 7, 2, 1, 2, 2, 2, 2, 1, 1, 2, 3.0]).reshape(12, 1)   # tokamak/utils/common.py:16
SMOKE_RESCALER = torch.tensor([2, 19, 20, 17, 20, 1, 1.0]).reshape(1, 1, 7, 1, 1)      # 2d/ddpm/data_2d.py:38


class _Draws:
    def __init__(self, noise):
        self.noise, self.i = noise, 0

    def __call__(self):
        z = self.noise(self.i)
        self.i += 1
        return z


def ddpm_row(tabs, t, k=1.0):
    """Coefficient row of DDPM timestep t: {a, b, c1, c2, sigma, k} (sigma = exp(0.5 * posterior_log_variance_clipped))."""
    return dict(a=tabs["sqrt_recip_alphas_cumprod"][t], b=tabs["sqrt_recipm1_alphas_cumprod"][t],
                c1=tabs["posterior_mean_coef1"][t], c2=tabs["posterior_mean_coef2"][t],
                sigma=(0.5 * tabs["posterior_log_variance_clipped"][t]).exp(), k=k)


def ddim_row(tabs, time, time_next, eta, k=1.0):
    """Coefficient row of one DDIM step: {a, b, c1 = sqrt(alpha_next), c2 = c, sigma, k, last} (1D/model/diffusion.py:500-504)."""
    row = dict(a=tabs["sqrt_recip_alphas_cumprod"][time], b=tabs["sqrt_recipm1_alphas_cumprod"][time], k=k,
               last=time_next < 0)
    if time_next >= 0:
        alpha, alpha_next = tabs["alphas_cumprod"][time], tabs["alphas_cumprod"][time_next]
        sigma = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
        row.update(c1=alpha_next.sqrt(), c2=(1 - alpha_next - sigma ** 2).sqrt(), sigma=sigma)
    return row


def _posterior_row(row, x, eps, g, clip, z):
    """eps -> x0 -> eps' = eps + k*g -> x0' -> clamp -> posterior mean -> + sigma z."""
    if g is not None:
        eps = eps + g * row["k"]
    x0 = row["a"] * x - row["b"] * eps
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    mean = row["c1"] * x0 + row["c2"] * x
    if z is None:
        return mean, x0
    return mean + row["sigma"] * z, x0


def _x0_row(row, x, eps):
    return row["a"] * x - row["b"] * eps


def _posterior_step(tabs, x, t, eps, g, k, clip, z):
    """_posterior_row at DDPM timestep t of the tables (bench.py's CPU baseline steps with it)."""
    return _posterior_row(ddpm_row(tabs, t, k), x, eps, g, clip, z)


def _x0_from_eps(tabs, x, t, eps):
    return _x0_row(ddpm_row(tabs, t), x, eps)


# ----------------------------------------------------------------------------
# one reverse step (the bodies of the loops below; any float dtype: the row may hold 0-d tensors or Python floats)
#   x, eps   state and predicted noise
#   row      ddpm_row / ddim_row (or the same keys filled by the caller)
#   z        the step's normal draw, None where the loop makes none (t == 0)
#   guide    x0 -> dJ/dx0 (autograd of the restated J) or None
#   impose   closure writing the conditions into its argument in place, or None
# each returns (x_next, x0): x0 is the guided, clipped x_start the update was formed from
# ----------------------------------------------------------------------------

def ddpm_step(x, eps, row, z, guide, impose, *, clip=True):
    """p_sample with guidance on x0 (guidance_u0): 1D/model/diffusion.py:226-306, 2d/ddpm/diffusion_2d.py:242-285."""
    g = guide(_x0_row(row, x, eps)) if guide is not None else None
    out, x0 = _posterior_row(row, x, eps, g, clip, z)
    if impose is not None:
        impose(out)
    return out, x0


def ddpm_calib_step(x, eps, row, z, guide, impose, *, clip=True):
    """The calibration branch (guidance_u0 False, 1D/model/diffusion.py:421-447): p_sample twice, the first result only
    feeds nabla_J(img_curr).  z = (discarded draw, used draw) or None."""
    z0, z1 = z if z is not None else (None, None)
    cur, _ = _posterior_row(row, x, eps, None, clip, z0)
    eps2 = eps + (guide(cur) * row["k"] if guide is not None else 0)
    out, x0 = _posterior_row(row, x, eps2, None, clip, z1)
    if impose is not None:
        impose(out)
    return out, x0


def ddim_step(x, eps, row, z, guide, impose):
    """One ddim_sample step with model_predictions(clip_x_start=True, rederive_pred_noise=True): x0 clipped, guidance
    evaluated on the clipped x0, eps re-derived from the clipped guided x0; the last step returns x0 itself."""
    a, b = row["a"], row["b"]
    x0 = (a * x - b * eps).clamp(-1.0, 1.0)
    if guide is not None:
        eps = eps + guide(x0) * row["k"]
    x0 = (a * x - b * eps).clamp(-1.0, 1.0)
    eps = (a * x - x0) / b
    if row["last"]:
        out = x0.clone()
    else:
        out = x0 * row["c1"] + row["c2"] * eps
        if z is not None:
            out = out + row["sigma"] * z
    if impose is not None:
        impose(out)
    return out, x0


# ----------------------------------------------------------------------------
# guidance (autograd of the restated J, like the reference does it)
# ----------------------------------------------------------------------------

def burgers_J(state, Q, w_score, u_bound, use_max_safety=True):
    """calculate_guidance, 1D/utils/guidance.py:58-77 (mean when use_max_safety!)."""
    s = (state * BURGERS_SCALER)[:, 2, :11, :]
    s = s.mean(dim=(-1, -2)) if use_max_safety else s.amax(dim=(-1, -2))
    return torch.maximum(s + Q - u_bound ** 2, torch.zeros_like(s)) * w_score


def burgers_guidance(Q, w_score, u_bound, use_max_safety=True):
    def nablaJ(x):
        with torch.enable_grad():
            x = x.detach().requires_grad_()
            return torch.autograd.grad(burgers_J(x, Q, w_score, u_bound, use_max_safety).sum(), x)[0]
    return nablaJ


def tokamak_J(x, target, nt, Q, thr, w_obj, w_safe):
    """GradientGuidance.calculate_loss, tokamak/utils/guidance.py:32-56."""
    st = (x * TOKAMAK_SCALER.to(x.device))[:, :3, :nt]
    obj = (st[:, 0] - target[:, 0]).square().mean(-1) + (st[:, 2] - target[:, 2]).square().mean(-1)
    s = st[:, 1].amin(dim=-1)                                            # utils/metrics.py:144-151
    safe = torch.maximum(thr - s + Q, torch.zeros_like(s))
    return w_obj * obj + w_safe * safe


def tokamak_guidance(target, nt, Q, thr, w_obj, w_safe, scaler):
    def nablaJ(x):
        with torch.enable_grad():
            x = x.detach().requires_grad_()
            loss = tokamak_J(x, target, nt, Q, thr, w_obj, w_safe) * scaler
            return torch.autograd.grad(loss, x, grad_outputs=torch.ones_like(loss))[0]
    return nablaJ


def smoke_J(x, Q, w_safe, safe_bound):
    """InferencePipeline.guidance, 2d/inference_2d.py:173-186."""
    st = x * SMOKE_RESCALER.to(x.device)
    succ = st[:, :, 5].mean((-1, -2, -3))
    safe = torch.maximum(st[:, -1, 6].mean((-1, -2)) + Q - safe_bound, torch.zeros_like(st[:, -1, 6, 0, 0]))
    return -(1 - w_safe) * succ + w_safe * safe


def smoke_guidance(Q, w_safe, safe_bound):
    def design_fn(x):
        with torch.enable_grad():
            x = x.detach().requires_grad_()
            return torch.autograd.grad(smoke_J(x, Q, w_safe, safe_bound).sum(), x)[0]
    return design_fn


# ----------------------------------------------------------------------------
# reverse loops
# ----------------------------------------------------------------------------

def burgers_impose(u_init, u_final, w_groundtruth=None, condition_idx=10, train_on_padded_locations=False):
    """set_condition / set_pad_condition, 1D/model/diffusion.py:336-366,380-394 (in place)."""
    def impose(img):
        img[:, 0, 0, :] = u_init
        img[:, 0, condition_idx, :] = u_final
        if w_groundtruth is not None:
            img[:, 1, :, :] = w_groundtruth
        if not train_on_padded_locations:
            img[:, 0, condition_idx + 1:, :] = 0
            img[:, 1, condition_idx:, :] = 0
            img[:, 2, condition_idx:, :] = 0
    return impose


def tokamak_impose(u_init, u_final, nt=122, train_on_padded_locations=True, w_groundtruth=None):
    """tokamak/model/diffusion.py:295-308,330-336; w_groundtruth as the DDIM path writes it (:411,:453)."""
    def impose(img):
        img[:, :3, 0] = u_init
        img[:, [0, 2], :nt] = u_final
        if not train_on_padded_locations:
            img[:, :3, nt:] = 0
            img[:, 3:, nt - 1:] = 0
        if w_groundtruth is not None:
            img[:, 3:, :] = w_groundtruth
    return impose


def smoke_impose(init, control=None, control_only=False):
    """2d/ddpm/diffusion_2d.py:297-301,310-312; control_only: what follows the DDIM loop (:400-401)."""
    def impose(x):
        if not control_only:
            x[:, 0, 0] = init
        if control is not None:
            x[:, :, 3:5] = control
    return impose


def _lucid_loop(eps_fn, tabs, shape, noise, impose, *, nablaJ, J_scheduler, guidance_u0,
                clip_denoised, enable_grad, T):
    """Common body of the burgers / tokamak p_sample_loop."""
    draw = _Draws(noise)
    img = draw().clone()
    impose(img)
    for t in reversed(range(T)):
        eps = eps_fn(img, torch.full((shape[0],), t, dtype=torch.long))
        row = ddpm_row(tabs, t, J_scheduler(t) if J_scheduler is not None else 1.0)
        nxt_impose = impose if t > 0 else None                           # the loop imposes before every forward only
        if guidance_u0:
            img, _ = ddpm_step(img, eps, row, draw() if t > 0 else None, nablaJ, nxt_impose, clip=clip_denoised)
        else:
            z = (draw(), draw()) if t > 0 else None
            _ = eps_fn(img, torch.full((shape[0],), t, dtype=torch.long))   # discarded forward (:423)
            keep = t == 0 and enable_grad                                # reference keeps img there (:445-447)
            nxt, _ = ddpm_calib_step(img, eps, row, z, nablaJ, None if keep else nxt_impose, clip=clip_denoised)
            if not keep:
                img = nxt
    return img


def sample_burgers(eps_fn, tabs, batch, noise, *, u_init, u_final, nablaJ=None, J_scheduler=None,
                   guidance_u0=True, w_groundtruth=None, clip_denoised=True, enable_grad=True,
                   condition_idx=10, train_on_padded_locations=False, shape=(3, 16, 128), T=None):
    T = T or tabs["betas"].shape[0]

    impose = burgers_impose(u_init, u_final, w_groundtruth, condition_idx, train_on_padded_locations)
    return _lucid_loop(eps_fn, tabs, (batch, *shape), noise, impose, nablaJ=nablaJ, J_scheduler=J_scheduler,
                       guidance_u0=guidance_u0, clip_denoised=clip_denoised, enable_grad=enable_grad, T=T)


def sample_tokamak(eps_fn, tabs, batch, noise, *, u_init, u_final, nablaJ=None, J_scheduler=None,
                   guidance_u0=True, w_groundtruth=None, clip_denoised=True, enable_grad=True,
                   nt=122, train_on_padded_locations=True, shape=(12, 128), T=None):
    T = T or tabs["betas"].shape[0]
    if w_groundtruth is not None:
        # reference bug: ``img[:,1,:,:] = w_groundtruth`` on a 3-D tensor
        raise IndexError("too many indices for tensor of dimension 3")

    impose = tokamak_impose(u_init, u_final, nt, train_on_padded_locations)
    return _lucid_loop(eps_fn, tabs, (batch, *shape), noise, impose, nablaJ=nablaJ, J_scheduler=J_scheduler,
                       guidance_u0=guidance_u0, clip_denoised=clip_denoised, enable_grad=enable_grad, T=T)


def sample_smoke(eps_fn, tabs, batch, noise, *, init, control=None, design_fn=None, ratio=1.0,
                 shape=(32, 7, 64, 64), T=None):
    T = T or tabs["betas"].shape[0]
    draw = _Draws(noise)
    x = draw().clone()

    impose = smoke_impose(init, control)
    impose(x)
    for t in reversed(range(T)):
        eps = eps_fn(x, torch.full((batch,), t, dtype=torch.long))
        x, _ = ddpm_step(x, eps, ddpm_row(tabs, t, ratio), draw() if t > 0 else None, design_fn, impose, clip=True)
    return x


# ----------------------------------------------------------------------------
# conformal
# ----------------------------------------------------------------------------

def normalize_weights(w, smoke=False):
    w = w.clone()
    inf = torch.isinf(w)
    if inf.any():
        w[inf] = w[~inf].max()
    if w.sum() == 0:
        out = torch.ones_like(w)
    else:
        out = w.shape[0] * w / w.sum()
    if smoke:                                                            # 2d/inference_2d.py:110
        bad = torch.isinf(out)
        out[bad] = w.shape[0] / bad.sum()
    return out


def burgers_weight(state, Q, w_score, u_bound, use_max_safety=True):
    return torch.exp(-burgers_J(state, Q, w_score, u_bound, use_max_safety))


def burgers_score(pred, state, use_max_safety=True):
    f = (lambda s: s.mean(dim=(-1, -2))) if use_max_safety else (lambda s: s.amax(dim=(-1, -2)))
    return (f((pred * BURGERS_SCALER)[:, 2, :11, :]) - f((state * BURGERS_SCALER)[:, 2, :11, :])).abs()


def tokamak_weight(state, target, nt, Q, thr, w_obj, w_safe, scaler):
    return torch.exp(-tokamak_J(state, target, nt, Q, thr, w_obj, w_safe) * scaler)


def tokamak_score(pred, state, nt):
    f = lambda s: (s * TOKAMAK_SCALER)[:, 1, :nt].amin(dim=-1)
    return (f(pred) - f(state)).abs()


def smoke_weight(state, Q, w_safe, safe_bound, ratio):
    return torch.exp(-ratio * smoke_J(state, Q, w_safe, safe_bound))


def smoke_score(pred, state):
    p, s = pred * SMOKE_RESCALER.to(pred.device), state * SMOKE_RESCALER.to(state.device)
    return (p[:, -1, -1].mean((-1, -2)) - s[:, -1, -1, 0, 0]).abs()


def quantile_lucid(scores, alpha):
    """1D/inference/conformal.py:95-117 == tokamak/inference/conformal.py:121-145."""
    n = scores.shape[0]
    _, idx = torch.sort(scores)
    rank = min(int(np.ceil(alpha * (n + 1))), n) - 1
    return scores[idx[rank]]


def quantile_smoke(scores, alpha):
    """2d/inference_2d.py:150-165."""
    n = scores.shape[0]
    _, idx = torch.sort(scores)
    q = int(min(np.ceil((n + 1) * (1 - alpha)), n - 1))
    return scores[idx[q - 1]]


# ----------------------------------------------------------------------------
# DDIM: what the reference's shipped scripts actually run
# ----------------------------------------------------------------------------

def ddim_pairs(T, S):
    """[(time, time_next)] of ddim_sample: 1D/model/diffusion.py:460-462 (== tokamak, 2d)."""
    times = torch.linspace(-1, T - 1, steps=S + 1)
    times = list(reversed(times.int().tolist()))
    return list(zip(times[:-1], times[1:]))


def _ddim_loop(eps_fn, tabs, shape, noise, impose, finish, *, S, eta, guide, k_of_t):
    """ddim_sample: 1D/model/diffusion.py:451-555, tokamak/...:374-496, 2d/ddpm/diffusion_2d.py:324-404.
    model_predictions(clip_x_start=True, rederive_pred_noise=True): x0 clipped, guidance evaluated on the clipped x0,
    eps re-derived from the clipped guided x0."""
    T = tabs["betas"].shape[0]
    draw = _Draws(noise)
    img = draw().clone()
    impose(img)
    for time, time_next in ddim_pairs(T, S):
        eps = eps_fn(img, torch.full((shape[0],), time, dtype=torch.long))
        row = ddim_row(tabs, time, time_next, eta, k_of_t(time))
        last = time_next < 0
        img, _ = ddim_step(img, eps, row, None if last else draw(), guide, None if last else impose)
    finish(img)
    return img


def ddim_burgers(eps_fn, tabs, batch, noise, *, S, eta, u_init, u_final, nablaJ=None, J_scheduler=None, guidance_u0=True,
                 w_groundtruth=None, condition_idx=10, train_on_padded_locations=False, shape=(3, 16, 128)):
    impose = burgers_impose(u_init, u_final, w_groundtruth, condition_idx, train_on_padded_locations)
    k = (lambda t: J_scheduler(t)) if J_scheduler is not None else (lambda t: 1.0)
    return _ddim_loop(eps_fn, tabs, (batch, *shape), noise, impose, lambda img: None, S=S, eta=eta,
                      guide=nablaJ if guidance_u0 else None, k_of_t=k)


def ddim_tokamak(eps_fn, tabs, batch, noise, *, S, eta, u_init, u_final, nablaJ=None, J_scheduler=None, guidance_u0=True,
                 w_groundtruth=None, nt=122, train_on_padded_locations=True, shape=(12, 128)):
    impose = tokamak_impose(u_init, u_final, nt, train_on_padded_locations, w_groundtruth)   # the DDIM path indexes correctly
    k = (lambda t: J_scheduler(t)) if J_scheduler is not None else (lambda t: 1.0)
    return _ddim_loop(eps_fn, tabs, (batch, *shape), noise, impose, lambda img: None, S=S, eta=eta,
                      guide=nablaJ if guidance_u0 else None, k_of_t=k)


def ddim_smoke(eps_fn, tabs, batch, noise, *, S, eta, init, control=None, design_fn=None, ratio=1.0, shape=(32, 7, 64, 64)):
    impose, finish = smoke_impose(init, control), smoke_impose(init, control, control_only=True)
    return _ddim_loop(eps_fn, tabs, (batch, *shape), noise, impose, finish, S=S, eta=eta, guide=design_fn,
                      k_of_t=lambda t: ratio)
