"""CPU-side checks of what the fused reverse-step GPU tests (test_gpu_step_kernels.py) lean on:

* the one-step functions of oracle/samplers.py, chained, are the oracle loops (which test_oracle_golden.py pins to
  fixtures from the real reference) -- bit for bit;
* the NumPy Philox4x32-10 of oracle/philox.py gives the Random123 known answers;
* sdc_step_update and sdc_impose refuse bad arguments before any launch (no GPU is touched: every call returns
  from the host-side checks).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import philox, samplers as osam, schedules
from oracle.detweights import det_noise, det_tensor
from safediffcon_amd import _lib
from safediffcon_amd._lib import SdcStepDesc

SDC_EINVAL, SDC_EALIGN, SDC_ENULL = -1, -2, -4


# ------------------------------------------------------------------ one-step functions == the loops
def _eps_fn(x, t):
    """cheap closed form with the U-Net's signature: depends on the state, the position and the timestep"""
    pos = torch.arange(x[0].numel(), dtype=torch.float32).reshape(x.shape[1:])
    return 0.4 * x + 0.3 * torch.sin(0.37 * pos + t.reshape(-1, *[1] * (x.dim() - 1)).float())


class _Draw:
    def __init__(self, noise):
        self.noise, self.i = noise, 0

    def __call__(self):
        self.i += 1
        return self.noise(self.i - 1)


def _chain_ddpm(tabs, T, noise, impose, guide, k_of_t, *, clip, guided, impose_last, keep_last=False):
    draw = _Draw(noise)
    x = draw().clone()
    impose(x)
    B = x.shape[0]
    for t in reversed(range(T)):
        eps = _eps_fn(x, torch.full((B,), t, dtype=torch.long))
        row = osam.ddpm_row(tabs, t, k_of_t(t))
        imp = impose if (t > 0 or impose_last) else None
        if guided:
            x, x0 = osam.ddpm_step(x, eps, row, draw() if t > 0 else None, guide, imp, clip=clip)
        else:
            z = (draw(), draw()) if t > 0 else None
            if t == 0 and keep_last:
                break
            x, x0 = osam.ddpm_calib_step(x, eps, row, z, guide, imp, clip=clip)
        assert x0.shape == x.shape
    return x, draw.i


def _chain_ddim(tabs, S, eta, noise, impose, finish, guide, k_of_t):
    draw = _Draw(noise)
    x = draw().clone()
    impose(x)
    B = x.shape[0]
    for time, nxt in osam.ddim_pairs(tabs["betas"].shape[0], S):
        eps = _eps_fn(x, torch.full((B,), time, dtype=torch.long))
        row = osam.ddim_row(tabs, time, nxt, eta, k_of_t(time))
        last = nxt < 0
        x, x0 = osam.ddim_step(x, eps, row, None if last else draw(), guide, None if last else impose)
        assert x0.abs().max() <= 1.0
    finish(x)
    return x, draw.i


def _burgers_impose(u0, uT, wgt, ci, pad_zero):
    return osam.burgers_impose(u0, uT, wgt, ci, not pad_zero)


def _tokamak_impose(u0, uT, nt, pad_zero, wgt=None):
    return osam.tokamak_impose(u0, uT, nt, not pad_zero, wgt)


def _smoke_impose(init, control):
    return osam.smoke_impose(init, control)


T, B = 6, 2
K = lambda t: 0.5 + 0.25 * t   # noqa: E731


@pytest.mark.parametrize("ums", [True, False])
@pytest.mark.parametrize("clip", [True, False])
def test_burgers_ddpm_chain_equals_loop(ums, clip):
    tabs = schedules.make_tables("cosine", T)
    shape = (3, 16, 20)
    noise = det_noise((B, *shape), 40)
    u0, uT = det_tensor((B, 20), 1, 0.1), det_tensor((B, 20), 2, 0.1)
    nablaJ = osam.burgers_guidance(0.05, 3.0, 0.3, ums)
    want = osam.sample_burgers(_eps_fn, tabs, B, noise, u_init=u0, u_final=uT, nablaJ=nablaJ, J_scheduler=K,
                               clip_denoised=clip, enable_grad=False, shape=shape, condition_idx=10)
    got, draws = _chain_ddpm(tabs, T, noise, _burgers_impose(u0, uT, None, 10, True), nablaJ, K, clip=clip, guided=True,
                             impose_last=False)
    assert draws == T and torch.equal(got, want)
    unguided = osam.sample_burgers(_eps_fn, tabs, B, noise, u_init=u0, u_final=uT, clip_denoised=clip, enable_grad=False,
                                   shape=shape)
    assert not torch.equal(unguided, want)          # the guidance mattered


@pytest.mark.parametrize("enable_grad", [False, True])
@pytest.mark.parametrize("with_guide", [False, True])
def test_burgers_calibration_chain_equals_loop(enable_grad, with_guide):
    tabs = schedules.make_tables("cosine", T)
    shape = (3, 12, 8)
    noise = det_noise((B, *shape), 50)
    u0, uT, wgt = det_tensor((B, 8), 1, 0.1), det_tensor((B, 8), 2, 0.1), det_tensor((B, 12, 8), 3, 0.2)
    nablaJ = osam.burgers_guidance(0.05, 3.0, 0.3) if with_guide else None
    want = osam.sample_burgers(_eps_fn, tabs, B, noise, u_init=u0, u_final=uT, nablaJ=nablaJ, J_scheduler=K, guidance_u0=False,
                               w_groundtruth=wgt, enable_grad=enable_grad, shape=shape, condition_idx=11,
                               train_on_padded_locations=True)
    got, draws = _chain_ddpm(tabs, T, noise, _burgers_impose(u0, uT, wgt, 11, False), nablaJ, K, clip=True, guided=False,
                             impose_last=False, keep_last=enable_grad)
    assert draws == 1 + 2 * (T - 1) and torch.equal(got, want)


@pytest.mark.parametrize("guided", [True, False])
def test_tokamak_ddpm_chain_equals_loop(guided):
    tabs = schedules.make_tables("cosine", T)
    shape, nt = (12, 24), 19
    noise = det_noise((B, *shape), 60)
    u0, uT = det_tensor((B, 3), 1, 0.1), det_tensor((B, 2, nt), 2, 0.1)
    nablaJ = osam.tokamak_guidance(det_tensor((B, 3, nt), 3), nt, 0.02, 0.4, 0.5, 2.0, 0.25)
    want = osam.sample_tokamak(_eps_fn, tabs, B, noise, u_init=u0, u_final=uT, nablaJ=nablaJ, J_scheduler=K,
                               guidance_u0=guided, enable_grad=False, nt=nt, train_on_padded_locations=False, shape=shape)
    got, _ = _chain_ddpm(tabs, T, noise, _tokamak_impose(u0, uT, nt, True), nablaJ, K, clip=True, guided=guided,
                         impose_last=False)
    assert torch.equal(got, want)


@pytest.mark.parametrize("control", [False, True])
def test_smoke_ddpm_chain_equals_loop(control):
    tabs = schedules.make_tables("sigmoid", T)
    shape = (4, 7, 4, 8)
    noise = det_noise((B, *shape), 70)
    init = det_tensor((B, 4, 8), 1, 0.1)
    ctl = det_tensor((B, 4, 2, 4, 8), 2, 0.2) if control else None
    design = osam.smoke_guidance(0.01, 0.7, 0.02)
    want = osam.sample_smoke(_eps_fn, tabs, B, noise, init=init, control=ctl, design_fn=design, ratio=0.75, shape=shape)
    got, draws = _chain_ddpm(tabs, T, noise, _smoke_impose(init, ctl), design, lambda t: 0.75, clip=True, guided=True,
                             impose_last=True)
    assert draws == T and torch.equal(got, want)


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_ddim_chain_equals_loop(eta):
    Tl, S = 12, 4
    tabs = schedules.make_tables("cosine", Tl)
    # burgers
    shape = (3, 16, 20)
    noise = det_noise((B, *shape), 80)
    u0, uT, wgt = det_tensor((B, 20), 1, 0.1), det_tensor((B, 20), 2, 0.1), det_tensor((B, 16, 20), 3, 0.2)
    nablaJ = osam.burgers_guidance(0.05, 3.0, 0.3, False)
    want = osam.ddim_burgers(_eps_fn, tabs, B, noise, S=S, eta=eta, u_init=u0, u_final=uT, nablaJ=nablaJ, J_scheduler=K,
                             w_groundtruth=wgt, shape=shape)
    got, draws = _chain_ddim(tabs, S, eta, noise, _burgers_impose(u0, uT, wgt, 10, True), lambda x: None, nablaJ, K)
    assert draws == S and torch.equal(got, want)
    # tokamak
    shape, nt = (12, 24), 19
    noise = det_noise((B, *shape), 81)
    u0, uT, wgt = det_tensor((B, 3), 1, 0.1), det_tensor((B, 2, nt), 2, 0.1), det_tensor((B, 9, 24), 3, 0.2)
    nablaJ = osam.tokamak_guidance(det_tensor((B, 3, nt), 3), nt, 0.02, 0.4, 0.5, 2.0, 0.25)
    want = osam.ddim_tokamak(_eps_fn, tabs, B, noise, S=S, eta=eta, u_init=u0, u_final=uT, nablaJ=nablaJ, J_scheduler=K,
                             w_groundtruth=wgt, nt=nt, train_on_padded_locations=False, shape=shape)
    got, _ = _chain_ddim(tabs, S, eta, noise, _tokamak_impose(u0, uT, nt, True, wgt), lambda x: None, nablaJ, K)
    assert torch.equal(got, want)
    # smoke (the control channels are written once more after the loop)
    shape = (4, 7, 4, 8)
    noise = det_noise((B, *shape), 82)
    init, ctl = det_tensor((B, 4, 8), 1, 0.1), det_tensor((B, 4, 2, 4, 8), 2, 0.2)
    design = osam.smoke_guidance(0.01, 0.7, 0.02)

    finish = osam.smoke_impose(init, ctl, control_only=True)
    want = osam.ddim_smoke(_eps_fn, tabs, B, noise, S=S, eta=eta, init=init, control=ctl, design_fn=design, ratio=0.75, shape=shape)
    got, _ = _chain_ddim(tabs, S, eta, noise, _smoke_impose(init, ctl), finish, design, lambda t: 0.75)
    assert torch.equal(got, want)


def test_one_step_functions_run_in_fp64():
    """the GPU tests evaluate them in fp64 with Python-float rows: same functions, tighter arithmetic"""
    tabs = schedules.make_tables("cosine", 8)
    x, eps, z = (det_tensor((2, 3, 11, 4), s) for s in (1, 2, 3))
    row32 = osam.ddpm_row(tabs, 5, 0.5)
    row64 = {k: float(v) for k, v in row32.items()}
    guide = osam.burgers_guidance(0.05, 3.0, 0.3)
    o32, _ = osam.ddpm_step(x, eps, row32, z, guide, None)
    o64, x064 = osam.ddpm_step(x.double(), eps.double(), row64, z.double(), guide, None)
    assert o64.dtype == torch.float64 and x064.dtype == torch.float64
    torch.testing.assert_close(o32.double(), o64, rtol=1e-5, atol=1e-5)
    assert (o32.double() - o64).abs().max() > 0
    drow = {k: (float(v) if k != "last" else v) for k, v in osam.ddim_row(tabs, 5, 2, 1.0, 0.5).items()}
    o64, _ = osam.ddim_step(x.double(), eps.double(), drow, z.double(), guide, None)
    assert o64.dtype == torch.float64


# ------------------------------------------------------------------ Philox4x32-10 known answers
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = philox.philox4x32_10(counter, key)
    assert " ".join("%08x" % int(v) for v in got) == want


def test_philox_stream_layout():
    """counter = {idx_lo, idx_hi, draw, 0x5DC}, key = (seed_lo, seed_hi): words() is the raw function at those words"""
    seed, draw = (7 << 32) | 9, 3
    w = philox.words(seed, draw, 6)
    assert w.shape == (6, 4) and w.dtype == np.uint32
    for i in (0, 5):
        want = philox.philox4x32_10((i, 0, draw, 0x5DC), (9, 7))
        assert [int(v) for v in w[i]] == [int(v) for v in want]
    u = philox.uniforms(np.array([[0, 1, 0x80000000, 0xffffffff]], dtype=np.uint32))
    assert u.dtype == np.float32
    assert u[0, 0] == np.float32(2.0 ** -33) and u[0, 2] == np.float32(0.5) and u[0, 3] == np.float32(1.0)
    z = philox.normals(1234, 1, 1 << 16)
    assert z.dtype == np.float64 and abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02


# ------------------------------------------------------------------ refusals (host-side checks only; nothing launches)
P = 1 << 12          # a 16-byte-aligned, non-null stand-in for pointers the checks only test, never follow


def _desc(model, B=2, dims=None, **kw):
    d = SdcStepDesc()
    d.model, d.B = model, B
    d.d0, d.d1, d.d2, d.d3 = dims or {0: (3, 16, 128, 1), 1: (12, 128, 1, 1), 2: (8, 7, 16, 16)}[model]
    d.cond_idx = {0: 10, 1: 122, 2: 0}[model]
    d.clip = 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _update(d, x=P, eps=P, gext=0, coef=P, t_dev=P, draw_dev=P, noise=P, gpar=0, gscal=0, target=0, c0=P, c1=P, c2=P,
            xout=P, x0out=0):
    return _refusal_lib().sdc_step_update(C.byref(d), x, eps, gext, coef, t_dev, draw_dev, noise, 0, gpar, gscal, target,
                                          c0, c1, c2, xout, x0out, 0)


def _refusal_lib():
    """The library, for a call that must be refused.  These calls hand it stand-in pointers; a library that wrongly accepted
    one would launch on it, so every such call goes through here and runs only where no GPU is visible (a launch then
    fails in the runtime and harms nothing)."""
    if torch.cuda.is_available():
        pytest.skip("refusals are checked on CPU-only machines")
    return _lib.get_lib()


def _impose(d, x=P, c0=P, c1=P, c2=P):
    return _refusal_lib().sdc_impose(C.byref(d), x, c0, c1, c2, 0)


def _refused(rc, code, word):
    assert rc == code, (rc, _lib.last_error())
    assert word in _lib.last_error()


@pytest.mark.parametrize("model", [_lib.SDC_MODEL_BURGERS, _lib.SDC_MODEL_TOKAMAK])
def test_impose_refuses_null_c1(model):
    _refused(_impose(_desc(model, impose=1), c1=0), SDC_ENULL, "c1")


@pytest.mark.parametrize("model", [0, 1, 2])
def test_impose_refuses_has_wgt_without_tensor(model):
    c1, c2 = (0, P) if model == _lib.SDC_MODEL_SMOKE else (P, 0)
    _refused(_impose(_desc(model, impose=1, has_wgt=1), c1=c1, c2=c2), SDC_ENULL, "has_wgt")


@pytest.mark.parametrize("model", [_lib.SDC_MODEL_BURGERS, _lib.SDC_MODEL_TOKAMAK])
def test_impose_refuses_control_only_mode_off_smoke(model):
    _refused(_impose(_desc(model, impose=2)), SDC_EINVAL, "smoke-only")


def test_impose_refuses_null_x_c0_and_bad_desc():
    _refused(_impose(_desc(2, impose=1), x=0), SDC_ENULL, "null")
    _refused(_impose(_desc(2, impose=1), c0=0), SDC_ENULL, "null")
    _refused(_impose(_desc(0, impose=1, dims=(3, 16, 126, 1))), SDC_EINVAL, "multiple of 4")


@pytest.mark.parametrize("model,dims", [(0, (3, 16, 126, 1)), (1, (12, 126, 1, 1)), (2, (8, 7, 16, 18))])
def test_update_refuses_innermost_not_multiple_of_4(model, dims):
    _refused(_update(_desc(model, dims=dims, cond_idx=10)), SDC_EINVAL, "multiple of 4")


def test_update_refuses_bad_shapes():
    _refused(_update(_desc(0, dims=(3, 10, 128, 1), cond_idx=5)), SDC_EINVAL, "burgers expects")       # H < 11
    _refused(_update(_desc(0, cond_idx=16)), SDC_EINVAL, "burgers expects")                           # cond_idx == H
    _refused(_update(_desc(0, cond_idx=-1)), SDC_EINVAL, "burgers expects")
    _refused(_update(_desc(1, cond_idx=129)), SDC_EINVAL, "tokamak expects")                          # nt > L
    _refused(_update(_desc(1, cond_idx=0)), SDC_EINVAL, "tokamak expects")
    _refused(_update(_desc(2, dims=(8, 6, 16, 16))), SDC_EINVAL, "smoke expects")


@pytest.mark.parametrize("which", ["x", "eps", "xout", "noise"])
def test_update_refuses_misaligned(which):
    _refused(_update(_desc(0), **{which: P + 4}), SDC_EALIGN, "aligned")


def test_update_refuses_missing_guidance_inputs():
    _refused(_update(_desc(0, guide=1), gpar=0, gscal=P), SDC_ENULL, "gpar")
    _refused(_update(_desc(0, guide=1), gpar=P, gscal=0), SDC_ENULL, "gscal")
    _refused(_update(_desc(1, guide=1), gpar=P, gscal=P, target=0), SDC_ENULL, "target")
    _refused(_update(_desc(0, guide=2), gext=0), SDC_ENULL, "gext")
    _refused(_update(_desc(0, guide=3), x0out=0), SDC_ENULL, "output")
    _refused(_update(_desc(0, guide=0), xout=0), SDC_ENULL, "output")
    _refused(_update(_desc(0, guide=4)), SDC_EINVAL, "guide")


def test_update_refuses_missing_conditions():
    _refused(_update(_desc(0, impose=1), c0=0), SDC_ENULL, "c0")
    _refused(_update(_desc(0, impose=1), c1=0), SDC_ENULL, "c1")
    _refused(_update(_desc(1, impose=1), c1=0), SDC_ENULL, "c1")
    _refused(_update(_desc(0, impose=1, has_wgt=1), c2=0), SDC_ENULL, "has_wgt")
    _refused(_update(_desc(2, impose=1, has_wgt=1), c1=0), SDC_ENULL, "has_wgt")
    _refused(_update(_desc(1, impose=2)), SDC_EINVAL, "smoke-only")
    _refused(_update(_desc(0), x=0), SDC_ENULL, "null")
    _refused(_update(_desc(0), t_dev=0), SDC_ENULL, "null")


# ------------------------------------------------------------------ the GPU sweep's coverage (pure bookkeeping, no device)
def test_gpu_sweep_covers_the_flag_space():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_step_kernels.py")
    spec = importlib.util.spec_from_file_location("_gpu_step_kernels_for_coverage", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert len(mod.SWEEP) >= 200
    mod.test_sweep_covers_the_flag_space()
