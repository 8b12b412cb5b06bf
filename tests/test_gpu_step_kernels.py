"""The fused reverse-step entry points of csrc/sdc_step.hip, called through the C ABI with the test's own coefficient
table, t_dev, draw_dev, gpar and conditions, against the one-step functions of oracle/samplers.py evaluated in fp64 on
the same fp32 inputs (widened).  tests/test_host_step_reference.py ties those functions to the golden-pinned loops.

Tolerance.  u = 2^-24 is the fp32 unit roundoff; every fp32 operation contributes at most u times the magnitude of its
result, and a result is at most the sum of the magnitudes of its terms.  With
    gs    = |g|                      (and, where g depends on the element's own x0 -- the tokamak objective channels --
                                      gs = scaler w_obj 2 S / nt * (S (|a x| + |b eps|) + |target|))
    E     = |eps| + |k| gs           the terms of eps' = eps + k g
    X0S   = |a x| + |b| E            the terms of x0' = a x - b eps'
the roundings on the way to x0' are
    guide 0 / 3:  a*x, b*eps, the subtraction                                            -> Kx = 3
    guide 2    :  + g*k, eps + g*k                                                        -> Kx = 5
    guide 1    :  + the closed-form g: at most 6 operations on its own terms (tokamak objective: S*x0, - target,
                  gp2*gp0, * (...), * S, / nt; the other forms need 3 to 5) + the 3 roundings of the x0 it is evaluated
                  on, = 9 u gs, + g*k, eps + g*k, then the 3 of x0'                        -> Kx = 9 + 2 + 3 = 14
so |x0' - ref| <= Kx u X0S (clamping is 1-Lipschitz).  The update adds
    DDPM:  c1*x0', c2*x, their sum, sigma*z, the last sum: 5 roundings of at most u scale each,
           scale = |c1| X0S + |c2 x| + |sigma z|                                          -> K = Kx + 5
    DDIM:  eps_r = (a x - x0') / b: the subtraction and the division (a*x is the same product), with
           R = (X0S + |a x| + |x0'|) / |b| >= |eps_r| this is |eps_r - ref| <= (Kx + 1) u R; then x0'*c1, c2*eps_r, sum,
           sigma*z, sum, scale = |c1| X0S + |c2| R + |sigma z|                            -> K = Kx + 6
    DDIM last row: the output is x0' itself, scale = X0S                                  -> K = Kx
The bound asserted per element is K u scale (1 + 2^-10); the last factor covers the second-order terms.  Contraction of
a*x - b*eps into a fused multiply-add only removes roundings.  scale is computed from the fp64 reference.  Every
comparison prints its maximum error in units of u scale ([measured] lines); imposed elements and elements the kernel
must leave alone are compared bit for bit.
"""
import ctypes as C
import math
import random
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import philox, samplers as osam
from safediffcon_amd import _lib
from safediffcon_amd._lib import SdcStepDesc, check
from safediffcon_amd.diffusion import schedule_tables

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
SENT = -12345.5                    # fills buffers the kernel must leave alone
BURGERS, TOKAMAK, SMOKE = 0, 1, 2
NAME = {BURGERS: "burgers", TOKAMAK: "tokamak", SMOKE: "smoke"}
GRID_CAP = 4096 * 256 * 4          # elements one grid-stride pass of step_update_kernel covers
KX = {0: 3, 3: 3, 2: 5, 1: 14}
T, S_DDIM = 1000, 10
TOK_S = (2.0, 7.0, 2.0)
# fixed guidance constants (dyadic, u_bound^2 an exact square); Q is placed per case
BURGERS_W, BURGERS_UB2 = 2.0, 0.5625
TOK_WOBJ, TOK_WSAFE, TOK_SCALER, TOK_THR = 0.5, 2.0, 0.25, 0.5
SMOKE_WSAFE, SMOKE_BOUND, SMOKE_RATIO = 0.75, 0.5, 0.75


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


# ------------------------------------------------------------------ coefficient tables (rows all differ)
_TABLES = {}


def tables():
    if not _TABLES:
        tabs = schedule_tables("cosine", T)
        c = torch.zeros(T, 8, dtype=torch.float32)
        c[:, 0], c[:, 1] = tabs["sqrt_recip_alphas_cumprod"], tabs["sqrt_recipm1_alphas_cumprod"]
        c[:, 2], c[:, 3] = tabs["posterior_mean_coef1"], tabs["posterior_mean_coef2"]
        c[:, 4] = (0.5 * tabs["posterior_log_variance_clipped"]).exp()
        c[0, 4] = 0.0                                                    # 'no noise if t == 0'
        c[:, 5] = 0.5 + (torch.arange(T) % 7) / 8.0
        pairs = osam.ddim_pairs(T, S_DDIM)
        m = torch.zeros(len(pairs), 8, dtype=torch.float32)
        for i, (time, nxt) in enumerate(pairs):
            r = osam.ddim_row(tabs, time, nxt, 1.0, 0.5 + (i % 7) / 8.0)
            m[i, 0], m[i, 1], m[i, 5], m[i, 6] = r["a"], r["b"], r["k"], float(r["last"])
            if not r["last"]:
                m[i, 2], m[i, 3], m[i, 4] = r["c1"], r["c2"], r["sigma"]
        assert len({tuple(r.tolist()) for r in c}) == T and len({tuple(r.tolist()) for r in m}) == len(pairs)
        _TABLES.update(ddpm=c, ddim=m)
    return _TABLES


def row64(table, row, ddim):
    v = [float(t) for t in table[row]]
    r = dict(a=v[0], b=v[1], c1=v[2], c2=v[3], sigma=v[4], k=v[5])
    if ddim:
        r["last"] = v[6] != 0.0
    return r


# ------------------------------------------------------------------ cases
def dims_of(model, shape):
    return {BURGERS: (*shape, 1), TOKAMAK: (*shape, 1, 1), SMOKE: tuple(shape)}[model]


def region(model, t, cond_idx):
    """view of the elements the safety functional reads"""
    if model == BURGERS:
        return t[:, 2, :11, :]
    if model == TOKAMAK:
        return t[:, 1, :cond_idx]
    return t[:, -1, 6]


def new_case(model, B, shape, cond_idx=0, *, guide=0, ddim=0, row=0, clip=1, impose=0, pad_zero=0, use_max=0, has_wgt=0,
             skip=0, inplace=True, want_x0=False, seed=0):
    return NS(model=model, B=B, shape=tuple(shape), cond_idx=cond_idx, guide=guide, ddim=ddim, row=row, clip=clip,
              impose=impose, pad_zero=pad_zero, use_max=use_max, has_wgt=has_wgt, skip=skip, inplace=inplace,
              want_x0=want_x0, seed=seed)


def case_id(c):
    return (f"{NAME[c.model]}-B{c.B}-{'x'.join(map(str, c.shape))}-ci{c.cond_idx}-g{c.guide}-{'ddim' if c.ddim else 'ddpm'}"
            f"-row{c.row}-clip{c.clip}-imp{c.impose}-pad{c.pad_zero}-max{c.use_max}-wgt{c.has_wgt}-skip{c.skip}"
            f"-{'in' if c.inplace else 'out'}-x0{int(c.want_x0)}")


def extremum_mode(c):
    return c.model == TOKAMAK or (c.model == BURGERS and c.use_max)


def make_conds(c, rn):
    B = c.B
    if c.model == BURGERS:
        _, H, W = c.shape
        return 0.1 * rn(B, W), 0.1 * rn(B, W), (0.2 * rn(B, H, W) if c.has_wgt else None)
    if c.model == TOKAMAK:
        L = c.shape[1]
        return 0.1 * rn(B, 3), 0.1 * rn(B, 2, c.cond_idx), (0.2 * rn(B, 9, L) if c.has_wgt else None)
    F, _, H, W = c.shape
    return 0.1 * rn(B, H, W), (0.2 * rn(B, F, 2, H, W) if c.has_wgt else None), None


def impose_closure(c, I, dtype=torch.float64):
    if not c.impose:
        return None
    w = lambda t: None if t is None else t.to(dtype)   # noqa: E731
    if c.model == BURGERS:
        return osam.burgers_impose(w(I.c0), w(I.c1), w(I.c2), c.cond_idx, not c.pad_zero)
    if c.model == TOKAMAK:
        return osam.tokamak_impose(w(I.c0), w(I.c1), c.cond_idx, not c.pad_zero, w(I.c2))
    return osam.smoke_impose(w(I.c0), w(I.c1), control_only=c.impose == 2)


def functional(c, x0):
    """the safety functional f per sample (fp64), as burgers_J / tokamak_J / smoke_J form it"""
    r = region(c.model, x0, c.cond_idx)
    if c.model == BURGERS:
        return 10.0 * (r.amax((-1, -2)) if c.use_max else r.mean((-1, -2)))
    if c.model == TOKAMAK:
        return 7.0 * r.amin(-1)
    return r.mean((-1, -2))                                               # SMOKE_RESCALER[6] == 1


def hinge_args(c, gpar, f):
    g = [float(v) for v in gpar]
    if c.model == TOKAMAK:
        return g[3] - f + g[4]
    return f + g[2] - g[1]


def gpar_for(c, thr):
    """guidance constants with the hinge's zero crossing at f == thr"""
    g = torch.zeros(8, dtype=torch.float32)
    if c.model == BURGERS:
        g[:4] = torch.tensor([BURGERS_W, BURGERS_UB2, BURGERS_UB2 - thr, 10.0])
    elif c.model == TOKAMAK:
        g[:5] = torch.tensor([TOK_WOBJ, TOK_WSAFE, TOK_SCALER, TOK_THR, thr - TOK_THR])
    else:
        g[:4] = torch.tensor([SMOKE_WSAFE, SMOKE_BOUND, SMOKE_BOUND - thr, SMOKE_RATIO])
    return g


def guide_callable(c, I):
    if c.guide == 2:
        return lambda x0: I.gext.double()
    if c.guide != 1:
        return None
    g = [float(v) for v in I.gpar]
    if c.model == BURGERS:
        ub = math.sqrt(g[1])
        assert ub * ub == g[1]
        return osam.burgers_guidance(g[2], g[0], ub, use_max_safety=not c.use_max)
    if c.model == TOKAMAK:
        return osam.tokamak_guidance(I.target.double(), c.cond_idx, g[4], g[3], g[0], g[1], g[2])
    return osam.smoke_guidance(g[2], g[0], g[1])


def make_inputs(c):
    g = torch.Generator().manual_seed(c.seed)
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    I = NS()
    I.table = tables()["ddim" if c.ddim else "ddpm"]
    a, b = I.table[c.row, 0], I.table[c.row, 1]
    B = c.B
    x0t = 0.7 * rn(B, *c.shape)
    reg = region(c.model, x0t, c.cond_idx)
    if extremum_mode(c):
        # keep the extremum region inside (-1, 1) (a clipped extremum is a tie: those are constructed separately) and
        # give every sample a clear leader
        sgn = -1.0 if c.model == TOKAMAK else 1.0
        r = 0.7 * torch.tanh(rn(*reg.shape))
        flat = r.reshape(B, -1)
        idx = (sgn * flat).argmax(1)
        flat[torch.arange(B), idx] += sgn * 0.05
        reg.copy_(flat.reshape(reg.shape))
    shift = 0.15 * (1.0 - 2.0 * (torch.arange(B) % 2)).reshape(B, *[1] * (reg.dim() - 1))
    reg += shift                                                          # samples on both sides of the hinge
    I.eps = rn(B, *c.shape)
    I.x = (x0t + b * I.eps) / a
    I.noise = rn(3, I.x.numel())
    I.gext = 0.5 * rn(B, *c.shape) if c.guide == 2 else None
    I.target = rn(B, 3, c.cond_idx) if c.model == TOKAMAK else None
    I.c0, I.c1, I.c2 = make_conds(c, rn)
    I.gpar = None
    if c.guide == 1:
        r = row64(I.table, c.row, c.ddim)
        x0 = r["a"] * I.x.double() - r["b"] * I.eps.double()
        if c.ddim:
            x0 = x0.clamp(-1.0, 1.0)
        f = functional(c, x0)
        fs = f.sort().values
        if B > 1:
            i = (fs[1:] - fs[:-1]).argmax()
            thr = 0.5 * (fs[i] + fs[i + 1]).item()
        else:
            thr = fs[0].item() + (0.3 if c.seed % 2 else -0.3)
        I.gpar = gpar_for(c, float(np.float32(thr)))
    return I


def assert_honest(c, I, x0g):
    """conditions on the CPU reference that keep the comparison honest: a clear extremum, a hinge away from zero"""
    r = region(c.model, x0g, c.cond_idx).reshape(c.B, -1)
    if extremum_mode(c) and r.shape[1] > 1:
        sgn = -1.0 if c.model == TOKAMAK else 1.0
        top = (sgn * r).topk(2, dim=1).values
        lead = (top[:, 0] - top[:, 1]) / r.abs().amax(1)
        assert lead.min() >= 1e-4, f"extremum leads the runner-up by only {lead.min():.2e}: pick another seed"
    h = hinge_args(c, I.gpar, functional(c, x0g))
    assert h.abs().min() >= 1e-3, f"hinge argument {h.abs().min():.2e} from zero: pick another seed"
    if c.B > 1:
        assert (h > 0).any() and (h < 0).any()


def reference(c, I, honest=True):
    """fp64 one-step reference -> NS(out, x0, scale_out, scale_x0, K_out, K_x0, imposed)"""
    r = row64(I.table, c.row, c.ddim)
    x, eps = I.x.double(), I.eps.double()
    a, b = r["a"], r["b"]
    R = NS(imposed=None)
    ax, be = (a * x).abs(), (b * eps).abs()
    if c.guide == 3:
        x0 = a * x - b * eps
        R.out, R.x0 = None, (x0.clamp(-1.0, 1.0) if c.ddim else x0)
        R.scale_x0, R.K_x0 = ax + be, KX[3]
        return R
    rec = {}
    base = guide_callable(c, I)

    def guide(x0):
        rec["x0"] = x0.detach()
        rec["g"] = base(x0)
        return rec["g"]
    draw = 1 + c.skip                                                     # draw_dev = 1 in every step test
    nz = I.noise.double().reshape(3, *x.shape) if I.noise is not None else None
    z = nz[draw] if (r["sigma"] != 0.0 and nz is not None) else None
    imp = impose_closure(c, I)
    gfn = guide if base is not None else None
    if c.ddim:
        R.out, R.x0 = osam.ddim_step(x, eps, r, z, gfn, imp)
    elif c.skip and c.guide == 0:
        zz = (nz[draw - 1], nz[draw]) if z is not None else None          # the calibration branch as the samplers run it
        R.out, R.x0 = osam.ddpm_calib_step(x, eps, r, zz, None, imp, clip=bool(c.clip))
    else:
        R.out, R.x0 = osam.ddpm_step(x, eps, r, z, gfn, imp, clip=bool(c.clip))
    if c.guide == 1 and honest:
        assert_honest(c, I, rec["x0"])
    gs = rec["g"].abs() if "g" in rec else torch.zeros_like(x)
    if c.guide == 1 and c.model == TOKAMAK:
        nt = c.cond_idx
        gp = [float(v) for v in I.gpar]
        for ch in (0, 2):
            S = TOK_S[ch]
            gs[:, ch, :nt] = gp[2] * gp[0] * 2.0 * S / nt * (S * (ax + be)[:, ch, :nt] + I.target.double()[:, ch].abs())
    X0S = ax + abs(b) * (eps.abs() + abs(r["k"]) * gs)
    sz = abs(r["sigma"]) * z.abs() if z is not None else 0.0
    kx = KX[c.guide]
    if not c.ddim:
        R.scale_out, R.K_out = abs(r["c1"]) * X0S + (r["c2"] * x).abs() + sz, kx + 5
    elif r["last"]:
        R.scale_out, R.K_out = X0S, kx
    else:
        Rr = (X0S + ax + R.x0.abs()) / abs(b)
        R.scale_out, R.K_out = abs(r["c1"]) * X0S + abs(r["c2"]) * Rr + sz, kx + 6
    R.scale_x0, R.K_x0 = X0S, kx
    if imp is not None:
        probe = torch.full_like(x, float("nan"))
        imp(probe)
        R.imposed = ~probe.isnan()
    return R


def make_desc(c):
    d = SdcStepDesc()
    d.model, d.B = c.model, c.B
    d.d0, d.d1, d.d2, d.d3 = dims_of(c.model, c.shape)
    d.guide, d.clip, d.impose, d.cond_idx, d.pad_zero, d.use_max = c.guide, c.clip, c.impose, c.cond_idx, c.pad_zero, c.use_max
    d.has_wgt, d.skip_draws, d.ddim, d.seed = c.has_wgt, c.skip, c.ddim, getattr(c, "philox_seed", 0)
    return d


def run_step(c, I, *, noise="explicit", draw=1):
    """sdc_guide_reduce (guide 1) + sdc_step_update on the GPU -> NS(out, x0, gscal, x_after)"""
    lib = _lib.get_lib()
    d = make_desc(c)
    x, eps, coef = _dev(I.x), _dev(I.eps), _dev(I.table)
    numel = x.numel()
    assert I.x.dtype == torch.float32 and I.x.shape == (c.B, *c.shape) and I.eps.shape == I.x.shape
    assert 0 <= c.row < coef.shape[0] and coef.shape[1] == 8
    nz, stride = None, 0
    if isinstance(noise, str):
        nz, stride = _dev(I.noise), numel
        assert nz.numel() >= (draw + c.skip + 1) * numel                  # the row the kernel reads exists
    elif noise is not None:
        nz = noise
        assert nz.numel() == numel
    gext, gpar, target = _dev(I.gext), _dev(I.gpar), _dev(I.target)
    c0, c1, c2 = _dev(I.c0), _dev(I.c1), _dev(I.c2)
    if c.guide == 2:
        assert gext.numel() == numel
    if c.impose or c.guide == 1:
        _check_cond_sizes(c, c0, c1, c2, target)
    t_dev = torch.tensor([c.row], dtype=torch.int32, device=DEV)
    draw_dev = torch.tensor([draw], dtype=torch.int32, device=DEV)
    xout = x if c.inplace else torch.full_like(x, SENT)
    x0out = torch.full_like(x, SENT) if (c.want_x0 or c.guide == 3) else None
    gscal = torch.zeros(4 * c.B, dtype=torch.float32, device=DEV) if c.guide == 1 else None
    s = _stream()
    if c.guide == 1:
        assert gpar.numel() == 8
        check(lib.sdc_guide_reduce(C.byref(d), _p(x), _p(eps), _p(coef), _p(t_dev), _p(gpar), _p(gscal), s), "sdc_guide_reduce")
    check(lib.sdc_step_update(C.byref(d), _p(x), _p(eps), _p(gext), _p(coef), _p(t_dev), _p(draw_dev), _p(nz), stride,
                              _p(gpar), _p(gscal), _p(target), _p(c0), _p(c1), _p(c2), _p(xout), _p(x0out), s), "sdc_step_update")
    torch.cuda.synchronize()
    return NS(out=xout.cpu(), x0=None if x0out is None else x0out.cpu(), gscal=None if gscal is None else gscal.cpu(),
              x_after=x.cpu())


def _check_cond_sizes(c, c0, c1, c2, target):
    B = c.B
    if c.model == BURGERS:
        _, H, W = c.shape
        want = (B * W, B * W, B * H * W if c.has_wgt else None)
    elif c.model == TOKAMAK:
        want = (B * 3, B * 2 * c.cond_idx, B * 9 * c.shape[1] if c.has_wgt else None)
        if c.guide == 1:
            assert target.numel() == B * 3 * c.cond_idx
    else:
        F, _, H, W = c.shape
        want = (B * H * W, B * F * 2 * H * W if c.has_wgt else None, None)
    if c.impose:
        for t, n in zip((c0, c1, c2), want):
            assert n is None or (t is not None and t.numel() == n)


MEASURED = {}


def close(tag, got, ref, scale, K, exact=None):
    """|got - ref| <= K u scale per element (bit-exact where `exact`); records the maximum in units of u scale"""
    gd = got.double()
    err = (gd - ref).abs()
    assert torch.isfinite(gd).all(), f"{tag}: non-finite output"
    if exact is not None:
        assert torch.equal(gd[exact], ref[exact]), f"{tag}: imposed elements differ"
        err = err.masked_fill(exact, 0.0)
    unit = U * scale
    ratio = (err / unit.clamp_min(1e-300)).max().item()
    MEASURED[tag] = max(MEASURED.get(tag, 0.0), ratio)
    bad = err > K * SLACK * unit
    if bad.any():
        i = (err / unit.clamp_min(1e-300)).argmax()
        idx = np.unravel_index(int(i), err.shape)
        raise AssertionError(f"{tag}: {int(bad.sum())} elements over {K} u scale; worst {ratio:.1f} u scale at {idx}: "
                             f"got {gd[idx].item():.9g} want {ref[idx].item():.9g} scale {scale[idx].item():.3g}")
    return ratio


def check_case(c, I, tag=None, honest=True, **kw):
    R = reference(c, I, honest)
    G = run_step(c, I, **kw)
    tag = tag or f"{NAME[c.model]} {'ddim' if c.ddim else 'ddpm'} guide {c.guide}"
    xin = I.x
    if c.guide == 3:
        r0 = close(tag + " x0out", G.x0, R.x0, R.scale_x0, R.K_x0)
        # guide = 3 writes x0out alone
        assert torch.equal(G.out, xin if c.inplace else torch.full_like(xin, SENT)), "guide=3 touched xout"
        print(f"[measured] {case_id(c)}: x0out {r0:.2f} u scale (bound {R.K_x0})")
        return R, G
    r1 = close(tag + " xout", G.out, R.out, R.scale_out, R.K_out, R.imposed)
    msg = f"[measured] {case_id(c)}: xout {r1:.2f} u scale (bound {R.K_out})"
    if c.want_x0:
        r0 = close(tag + " x0out", G.x0, R.x0, R.scale_x0, R.K_x0)
        msg += f", x0out {r0:.2f} (bound {R.K_x0})"
    if not c.inplace:
        assert torch.equal(G.x_after, xin), "out-of-place update wrote its input"
    print(msg)
    return R, G


# ------------------------------------------------------------------ the sweep
B_CHOICES = (1, 3, 64)
BURGERS_HW = [(H, W) for H in (11, 12, 16) for W in (4, 20, 128, 132)]
TOKAMAK_LNT = [(128, 122), (128, 128), (12, 1), (124, 123), (512, 300)]
SMOKE_FHW = [(F, H, W) for F in (1, 8, 32) for (H, W) in ((4, 4), (16, 16), (12, 20), (64, 64))]
MAX_SWEEP_ELEMS = 4_000_000
FLAGS = dict(guide=(0, 1, 2, 3), clip=(0, 1), impose=(0, 1), pad_zero=(0, 1), has_wgt=(0, 1), use_max=(0, 1), skip=(0, 1),
             inplace=(False, True), want_x0=(False, True))


def _sweep():
    rnd = random.Random(20240607)
    cases = []
    for model in (BURGERS, TOKAMAK, SMOKE):
        n = 0
        for ddim in (0, 1):
            rows = (0, S_DDIM // 2, S_DDIM - 1) if ddim else (T - 1, T // 2, 1, 0)
            for guide in (0, 1, 2, 3):
                for row in rows:
                    for _ in range(3):
                        if model == BURGERS:
                            H, W = BURGERS_HW[n % len(BURGERS_HW)]
                            shape, ci = (3, H, W), (0, 10, H - 1)[(n // len(BURGERS_HW)) % 3]
                        elif model == TOKAMAK:
                            L, nt = TOKAMAK_LNT[n % len(TOKAMAK_LNT)]
                            shape, ci = (12, L), nt
                        else:
                            F, H, W = SMOKE_FHW[n % len(SMOKE_FHW)]
                            shape, ci = (F, 7, H, W), 0
                        per = math.prod(shape)
                        B = B_CHOICES[(n // 5) % 3]
                        while B * per > MAX_SWEEP_ELEMS:
                            B = B_CHOICES[B_CHOICES.index(B) - 1]
                        f = {k: rnd.choice(v) for k, v in FLAGS.items() if k != "guide"}
                        if ddim:
                            f["clip"] = 1                                 # DDIM always clips; the flag is DDPM's
                        if model == SMOKE:
                            f["impose"] = rnd.choice((0, 1, 2))
                            f["pad_zero"] = f["use_max"] = 0              # burgers / tokamak flags
                        cases.append(new_case(model, B, shape, ci, guide=guide, ddim=ddim, row=row, seed=1000 * model + n, **f))
                        n += 1
    return cases


SWEEP = _sweep()


def test_sweep_covers_the_flag_space():
    """every flag value with every model, every (flag, ddim) pair, every listed shape value, every B with every model,
    first / middle / last rows"""
    for model in (BURGERS, TOKAMAK, SMOKE):
        cs = [c for c in SWEEP if c.model == model]
        for k, vals in FLAGS.items():
            if model == SMOKE and k in ("pad_zero", "use_max"):
                continue
            vals = (0, 1, 2) if (model == SMOKE and k == "impose") else vals
            for v in vals:
                assert any(getattr(c, k) == v for c in cs), (NAME[model], k, v)
                for ddim in (0, 1):
                    if k == "clip" and ddim:
                        continue
                    assert any(getattr(c, k) == v and c.ddim == ddim for c in cs), (NAME[model], k, v, ddim)
        assert {c.B for c in cs} == set(B_CHOICES), NAME[model]
        assert {c.row for c in cs if not c.ddim} == {T - 1, T // 2, 1, 0}
        assert {c.row for c in cs if c.ddim} == {0, S_DDIM // 2, S_DDIM - 1}
    b = [c for c in SWEEP if c.model == BURGERS]
    assert {c.shape[1:] for c in b} == set(BURGERS_HW)
    assert {("0" if c.cond_idx == 0 else "10" if c.cond_idx == 10 else "H-1") for c in b if c.cond_idx in (0, 10)} == {"0", "10"}
    assert any(c.cond_idx == c.shape[1] - 1 for c in b)
    assert {(c.shape[1], c.cond_idx) for c in SWEEP if c.model == TOKAMAK} == set(TOKAMAK_LNT)
    assert {(c.shape[0], c.shape[2], c.shape[3]) for c in SWEEP if c.model == SMOKE} == set(SMOKE_FHW)
    # the flags where they act: has_wgt / pad_zero only with impose, use_max only under the built-in guidance
    for model in (BURGERS, TOKAMAK, SMOKE):
        cs = [c for c in SWEEP if c.model == model and c.guide != 3]
        for ddim in (0, 1):
            assert any(c.impose >= 1 and c.has_wgt and c.ddim == ddim for c in cs), (NAME[model], "has_wgt imposed", ddim)
            assert any(c.impose >= 1 and not c.has_wgt and c.ddim == ddim for c in cs), (NAME[model], "no wgt imposed", ddim)
            if model != SMOKE:
                for pad in (0, 1):
                    assert any(c.impose == 1 and c.pad_zero == pad and not c.has_wgt and c.ddim == ddim for c in cs), \
                        (NAME[model], "pad_zero imposed", pad, ddim)
            else:
                assert any(c.impose == 2 and c.has_wgt and c.ddim == ddim for c in cs), ("smoke control only", ddim)
            if model == BURGERS:
                for um in (0, 1):
                    assert any(c.guide == 1 and c.use_max == um and c.ddim == ddim for c in cs), ("burgers use_max guided", um, ddim)
            for skip in (0, 1):
                noisy = [c for c in cs if c.ddim == ddim and c.row != (S_DDIM - 1 if ddim else 0)]     # sigma != 0 rows
                assert any(c.skip == skip for c in noisy), (NAME[model], "skip_draws on a row that draws", skip, ddim)
    # reduction lengths below, above and at multiples of the 256-thread block
    lens = [11 * W for _, W in BURGERS_HW] + [nt for _, nt in TOKAMAK_LNT] + [H * W for _, H, W in SMOKE_FHW]
    assert any(v < 256 for v in lens) and any(v > 256 and v % 256 for v in lens) and any(v % 256 == 0 for v in lens)


@pytest.mark.parametrize("c", SWEEP, ids=case_id)
def test_step_sweep(c):
    check_case(c, make_inputs(c))


@pytest.mark.parametrize("model,B,shape,ci", [(BURGERS, 700, (3, 16, 128), 10), (TOKAMAK, 2800, (12, 128), 122),
                                              (SMOKE, 5, (32, 7, 64, 64), 0)], ids=["burgers", "tokamak", "smoke"])
def test_step_past_the_grid_cap(model, B, shape, ci):
    """more elements than one pass of the capped grid covers: the grid-stride loop's second trip, compared in full
    (the last sample included)"""
    assert B * math.prod(shape) > GRID_CAP
    c = new_case(model, B, shape, ci, guide=1, row=T // 2, impose=1, has_wgt=1, pad_zero=int(model != SMOKE), want_x0=True,
                 seed=77 + model)
    I = make_inputs(c)
    check_case(c, I, tag=f"{NAME[model]} past the grid cap")          # every element, so the last sample in full
    c3 = new_case(model, B, shape, ci, guide=3, ddim=1, row=S_DDIM // 2, inplace=False, seed=78 + model)
    check_case(c3, make_inputs(c3), tag=f"{NAME[model]} past the grid cap")


# ------------------------------------------------------------------ constructed edges (dyadic rows and values: exact in fp32 and fp64)
def dyadic_inputs(c, x0, eps, *, row=(2.0, 0.5, 0.5, 0.125, 0.5, 0.5, 0.0), seed=5):
    """inputs whose x0 = a x - b eps is exactly `x0` (all values dyadic with few bits).  c2 / b != c1, or the DDIM
    update x0' c1 + c2 (a x - x0') / b would not depend on x0' at all."""
    g = torch.Generator().manual_seed(seed)
    I = NS()
    I.table = torch.tensor([list(row) + [0.0]], dtype=torch.float32)
    a, b = row[0], row[1]
    I.eps = eps.float()
    I.x = ((x0 + b * eps) / a).float()
    assert torch.equal(a * I.x.double() - b * I.eps.double(), x0.double())
    I.noise = (torch.randint(-8, 9, (3, I.x.numel()), generator=g) / 8.0).float()
    I.gext, I.gpar = None, None
    rn = lambda *s: (torch.randint(-8, 9, s, generator=g) / 16.0).float()   # noqa: E731
    I.target = rn(c.B, 3, c.cond_idx) if c.model == TOKAMAK else None
    I.c0, I.c1, I.c2 = make_conds(c, rn)
    return I


def _dy(shape, g, lo=-8, hi=9, q=16.0):
    return torch.randint(lo, hi, shape, generator=g) / q


def _grad_support(c, I, x0g):
    """elements on which the reference's own safety gradient is non-zero (autograd of the restated J, objective off)"""
    g = [float(v) for v in I.gpar]
    if c.model == BURGERS:
        fn = osam.burgers_guidance(g[2], g[0], math.sqrt(g[1]), use_max_safety=not c.use_max)
    else:
        fn = osam.tokamak_guidance(I.target.double(), c.cond_idx, g[4], g[3], 0.0, g[1], g[2])
    return fn(x0g.double())


@pytest.mark.parametrize("model", [BURGERS, TOKAMAK], ids=["burgers", "tokamak"])
def test_ties_by_clipping_ddim(model):
    """DDIM clips x0 before the guidance: four region elements pushed past the bound tie at exactly +-1, in different
    waves, different float4s and on both trips of the block's loop; the same value outside the region (wrong channel,
    h >= 11, t >= nt) gets nothing and is not counted.  Each tied element gets 1/4 of the gradient."""
    g = torch.Generator().manual_seed(11)
    B = 3
    if model == BURGERS:
        c = new_case(model, B, (3, 16, 128), 10, guide=1, ddim=1, use_max=1, want_x0=True)
        x0 = _dy((B, 3, 16, 128), g, -8, 9, 16.0)                          # |x0| <= 0.5
        sgn = 1.0
        spots = (3, 70, 200, 300 + 256)                                   # waves 0, 1, 3 and the loop's third trip
        for b in range(B):
            x0[b, 2].view(-1)[[s + b for s in spots]] = torch.tensor([1.5, 2.0, 1.25, 1.0])
        x0[:, 2, 11:, 5] = 1.5                                            # h >= 11
        x0[:, 0, 2, 9] = 2.0                                              # wrong channel
        x0[:, 1, 12, 9] = 1.0
        thr = 5.0
    else:
        c = new_case(model, B, (12, 512), 300, guide=1, ddim=1, want_x0=True)
        x0 = _dy((B, 12, 512), g, -8, 9, 16.0)
        sgn, reg = -1.0, x0[:, 1]
        spots = (5, 70, 130, 299)
        for b in range(B):
            reg[b, [s - b for s in spots]] = torch.tensor([-1.5, -2.0, -1.25, -1.0])
        x0[:, 1, 300:310] = -1.5                                          # t >= nt
        x0[:, 4, 17] = -2.0                                               # wrong channel
        x0[:, 0, 400] = -1.0
        thr = -3.0
    I = dyadic_inputs(c, x0, _dy(x0.shape, g, -8, 9, 4.0))
    I.gpar = gpar_for(c, thr)                                             # hinge active: f = +-10 / -7 at the clipped extremum
    R, G = check_case(c, I, tag=f"{NAME[model]} ties by clipping", honest=False)     # ties on purpose
    gs = G.gscal.reshape(B, 4)
    assert torch.equal(gs[:, 0], torch.ones(B)) and torch.equal(gs[:, 2], torch.full((B,), sgn))
    assert torch.equal(gs[:, 3], torch.full((B,), 0.25)), f"1/ties = {gs[:, 3].tolist()}"
    grad = _grad_support(c, I, x0.clamp(-1, 1))
    assert int((grad != 0).sum()) == 4 * B                                # the reference shares between the four alone
    if model == BURGERS:
        # dyadic throughout (the tokamak objective divides by nt): the guided output is exact, the share shows bit for bit
        assert torch.equal(G.out.double(), R.out), (G.out.double() - R.out).abs().max()
        R0 = reference(new_case(**{**vars(c), "guide": 0}), I)
        assert torch.equal(R.out != R0.out, grad != 0)                    # the update moved the four tied elements alone


@pytest.mark.parametrize("model", [BURGERS, TOKAMAK], ids=["burgers", "tokamak"])
@pytest.mark.parametrize("row", [T // 2, 3])
def test_ties_without_clipping_ddpm(model, row):
    """DDPM guidance sees the unclipped x0: the (x, eps) pair of the extremal element copied to two more region
    positions ties three values that the reduce kernel and the update kernel each recompute from a real schedule row;
    a fourth copy outside the region gets nothing.  The value comparison `x0 == extremum` of the tie path holds only
    because both kernels form x0 through the one x0_of() of sdc_step.hip; with the expression left to the compiler in
    each kernel this case loses tied elements' shares (profiles/step_kernels_sensitivity.md)."""
    B = 3
    if model == BURGERS:
        c = new_case(model, B, (3, 16, 132), 10, guide=1, row=row, use_max=1, clip=0, seed=31)
    else:
        c = new_case(model, B, (12, 512), 300, guide=1, row=row, clip=0, seed=32)
    I = make_inputs(c)
    r = row64(I.table, row, 0)
    x0 = r["a"] * I.x.double() - r["b"] * I.eps.double()
    sgn = -1.0 if model == TOKAMAK else 1.0
    per = math.prod(c.shape)
    xf, ef = I.x.reshape(B, per), I.eps.reshape(B, per)
    for b in range(B):
        if model == BURGERS:
            base, n = 2 * 16 * 132, 11 * 132
            outside = (2 * 16 + 12) * 132 + 7                             # h = 12
        else:
            base, n = 512, 300
            outside = 512 + 400                                           # t = 400 >= nt
        arg = base + int((sgn * x0.reshape(B, per)[b, base:base + n]).argmax())
        for dst in (base + (arg - base + 67) % n, base + (arg - base + 517) % n, outside):
            xf[b, dst], ef[b, dst] = xf[b, arg], ef[b, arg]
    x0 = r["a"] * I.x.double() - r["b"] * I.eps.double()
    f = functional(c, x0)
    I.gpar = gpar_for(c, float(np.float32(f.min() - 1.0 if model == BURGERS else f.max() + 1.0)))     # active everywhere
    grad = _grad_support(c, I, x0)
    assert int((grad != 0).sum()) == 3 * B
    # the honesty conditions are for unconstructed extrema: this case ties on purpose
    R, G = check_case(c, I, tag=f"{NAME[model]} ties without clipping", honest=False)
    gs = G.gscal.reshape(B, 4)
    assert torch.equal(gs[:, 3], torch.full((B,), float(np.float32(1.0) / np.float32(3.0)))), f"1/ties = {gs[:, 3].tolist()}"


def _hinge_case(kind):
    g = torch.Generator().manual_seed(21)
    B = 2
    if kind == "smoke":
        c = new_case(SMOKE, B, (8, 7, 16, 16), 0, guide=1, want_x0=True)
        x0 = _dy((B, 8, 7, 16, 16), g)
        x0[:, -1, 6] = 0.25                                               # f = 0.25
        gpar = torch.tensor([0.75, 0.5, 0.25, 0.75, 0, 0, 0, 0])          # 0.25 + 0.25 - 0.5 == 0
        qi = 2
    elif kind in ("burgers-mean", "burgers-amax"):
        c = new_case(BURGERS, B, (3, 16, 4), 10, guide=1, use_max=int(kind == "burgers-amax"), want_x0=True)
        x0 = _dy((B, 3, 16, 4), g)
        if c.use_max:
            x0[:, 2, :11] = _dy((B, 11, 4), g, -8, 2, 16.0)               # <= 1/16
            x0[:, 2, 4, 1] = 0.125                                        # the one amax
        else:
            x0[:, 2, :11] = 0.125                                         # f = 10 * 0.125 = 1.25
        gpar = torch.tensor([2.0, 2.25, 1.0, 10.0, 0, 0, 0, 0])           # 1.25 + 1 - 1.5^2 == 0
        qi = 2
    else:
        c = new_case(TOKAMAK, B, (12, 128), 122, guide=1, want_x0=True)
        x0 = _dy((B, 12, 128), g)
        x0[:, 1, :122] = _dy((B, 122), g, -3, 9, 16.0)                    # >= -3/16
        x0[:, 1, 77] = -0.25                                              # the one amin: s = -1.75
        gpar = torch.tensor([0.5, 2.0, 0.25, -2.0, 0.25, 0, 0, 0])        # -2 + 1.75 + 0.25 == 0
        qi = 4
    I = dyadic_inputs(c, x0, _dy(x0.shape, g, -8, 9, 4.0))
    return c, I, gpar, qi


@pytest.mark.parametrize("kind", ["burgers-mean", "burgers-amax", "tokamak", "smoke"])
@pytest.mark.parametrize("side", [0, 1, -1], ids=["at-zero", "above", "below"])
def test_hinge_at_and_around_zero(kind, side):
    """hinge argument exactly 0: torch.maximum(s, 0) passes half the gradient there, so gscal[4b] must be 0.5 and the
    update must carry half the active safety gradient; 2^-10 either side it is all or nothing."""
    c, I, gpar, qi = _hinge_case(kind)
    gpar = gpar.clone()
    gpar[qi] += side * 2.0 ** -10
    I.gpar = gpar
    R, G = check_case(c, I, tag=f"hinge {kind}", honest=False)              # the hinge sits at zero on purpose
    want = {0: 0.5, 1: 1.0, -1: 0.0}[side]
    h = hinge_args(c, gpar, functional(c, I.table[0, 0].item() * I.x.double() - I.table[0, 1].item() * I.eps.double()))
    assert torch.equal(h, torch.full_like(h, side * 2.0 ** -10))
    active = G.gscal.reshape(c.B, 4)[:, 0]
    print(f"[measured] hinge {kind} argument {side:+d} * 2^-10: gscal active = {active.tolist()} (reference derivative {want})")
    assert torch.equal(active, torch.full((c.B,), want)), f"active = {active.tolist()}, torch.maximum's backward gives {want}"


@pytest.mark.parametrize("model", [BURGERS, TOKAMAK, SMOKE], ids=["burgers", "tokamak", "smoke"])
@pytest.mark.parametrize("ddim", [0, 1], ids=["ddpm", "ddim"])
def test_sigma_zero_never_reads_the_noise(model, ddim):
    """sigma == 0 (DDPM t = 0; DDIM eta = 0): z is never read, so a noise tensor full of NaN changes nothing"""
    shape, ci = {BURGERS: ((3, 12, 20), 11), TOKAMAK: ((12, 124), 123), SMOKE: ((8, 7, 12, 20), 0)}[model]
    c = new_case(model, 3, shape, ci, guide=2, ddim=ddim, row=0, impose=1, seed=41 + model)
    I = make_inputs(c)
    if ddim:
        I.table = I.table[S_DDIM // 2:S_DDIM // 2 + 1].clone()
        I.table[0, 3] = (I.table[0, 3] ** 2 + I.table[0, 4] ** 2).sqrt()   # eta = 0: c = sqrt(1 - alpha_next)
        I.table[0, 4] = 0.0
    assert I.table[c.row, 4] == 0.0
    I.noise = torch.full_like(I.noise, float("nan"))
    check_case(c, I, tag=f"{NAME[model]} sigma 0")


# ------------------------------------------------------------------ sdc_impose
@pytest.mark.parametrize("model", [BURGERS, TOKAMAK, SMOKE], ids=["burgers", "tokamak", "smoke"])
def test_impose_alone(model):
    """conditioning writes only: imposed elements carry the condition values, every other element keeps its bits.
    impose_kernel's grid covers 4096 * 256 elements a trip, so the larger shapes take its loop round again."""
    shapes = {BURGERS: [((3, H, W), ci) for H, W in BURGERS_HW for ci in (0, 10, H - 1)],
              TOKAMAK: [((12, L), nt) for L, nt in TOKAMAK_LNT],
              SMOKE: [((F, 7, H, W), 0) for F, H, W in SMOKE_FHW]}[model]
    lib = _lib.get_lib()
    seen = set()
    for i, (shape, ci) in enumerate(shapes):
        B = B_CHOICES[i % 3]
        while B * math.prod(shape) > MAX_SWEEP_ELEMS:
            B = B_CHOICES[B_CHOICES.index(B) - 1]
        if i == 0:
            B = 4096 * 256 // math.prod(shape) + 3                        # past the grid cap at the smallest shape too
        modes = (1, 2) if model == SMOKE else (1,)
        c = new_case(model, B, shape, ci, impose=modes[i % len(modes)], pad_zero=i % 2 if model != SMOKE else 0,
                     has_wgt=(i // 2) % 2, seed=i)
        seen.add((c.impose, c.pad_zero, c.has_wgt))
        g = torch.Generator().manual_seed(900 + i)
        rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
        I = NS(x=rn(B, *shape))
        I.c0, I.c1, I.c2 = make_conds(c, rn)
        want = I.x.clone()
        impose_closure(c, I, torch.float32)(want)
        assert not torch.equal(want, I.x) or (c.impose == 2 and not c.has_wgt)
        x = _dev(I.x)
        c0, c1, c2 = _dev(I.c0), _dev(I.c1), _dev(I.c2)
        _check_cond_sizes(c, c0, c1, c2, None)
        d = make_desc(c)
        check(lib.sdc_impose(C.byref(d), _p(x), _p(c0), _p(c1), _p(c2), _stream()), "sdc_impose")
        torch.cuda.synchronize()
        assert torch.equal(x.cpu(), want), case_id(c)
    assert len(seen) == 4


# ------------------------------------------------------------------ noise
@pytest.mark.parametrize("model", [BURGERS, TOKAMAK, SMOKE], ids=["burgers", "tokamak", "smoke"])
@pytest.mark.parametrize("ddim", [0, 1], ids=["ddpm", "ddim"])
def test_in_kernel_noise_is_sdc_randn(model, ddim):
    """noise == nullptr draws Philox normals in the update kernel: bit-identical to the update fed the tensor sdc_randn
    writes for (seed, draw_dev + skip_draws)"""
    lib = _lib.get_lib()
    shape, ci = {BURGERS: ((3, 16, 128), 10), TOKAMAK: ((12, 128), 122), SMOKE: ((8, 7, 16, 16), 0)}[model]
    n = 0
    for seed in (0x1234, (0xABCD << 32) | 77):
        for draw in (0, 7):
            skip = n % 2
            n += 1
            c = new_case(model, 3, shape, ci, guide=0, ddim=ddim, row=(S_DDIM // 2 if ddim else T // 2), skip=skip,
                         inplace=bool(n % 2), seed=60 + n)
            c.philox_seed = seed
            I = make_inputs(c)
            assert I.table[c.row, 4] != 0.0
            own = run_step(c, I, noise=None, draw=draw)
            z = torch.full((I.x.numel(),), SENT, dtype=torch.float32, device=DEV)
            dd = torch.tensor([draw + skip], dtype=torch.int32, device=DEV)
            check(lib.sdc_randn(_p(z), z.numel(), seed, _p(dd), _stream()), "sdc_randn")
            torch.cuda.synchronize()
            assert 0.9 < z.std().item() < 1.1 and abs(z.mean().item()) < 0.05
            fed = run_step(c, I, noise=z, draw=draw)                      # stride 0: the one tensor, whatever the draw
            assert torch.equal(own.out, fed.out), f"seed {seed:#x} draw {draw} skip {skip}"
            other = torch.tensor([draw + skip + 1], dtype=torch.int32, device=DEV)
            z2 = torch.empty_like(z)
            check(lib.sdc_randn(_p(z2), z2.numel(), seed, _p(other), _stream()), "sdc_randn")
            check(lib.sdc_randn(_p(z), z.numel(), seed ^ (1 << 40), _p(dd), _stream()), "sdc_randn")
            torch.cuda.synchronize()
            assert not torch.equal(run_step(c, I, noise=z2, draw=draw).out, own.out)      # the draw word matters
            assert not torch.equal(run_step(c, I, noise=z, draw=draw).out, own.out)       # so does the key's high word


# max |sdc_randn - fp64 Box-Muller of the same fp32 uniforms| over the 9 (seed, draw) pairs below, 2^20 normals each, as
# measured on an MI355X (profiles/step_kernels_measured.log).  The kernel's __logf / __sincosf have no derivable bound;
# 4x covers intrinsic differences between compilers, and anything below 1e-3 still rejects a wrong counter, key or draw
# word (unrelated O(1) normals).
RANDN_MEASURED = 2.04e-6
RANDN_CEILING = 1e-3


@pytest.mark.parametrize("seed", [0, 1234, 2 ** 40 + 5])
@pytest.mark.parametrize("draw", [0, 1, 7])
def test_randn_against_numpy_philox(seed, draw):
    lib = _lib.get_lib()
    n = 1 << 20
    z = torch.full((n,), SENT, dtype=torch.float32, device=DEV)
    dd = torch.tensor([draw], dtype=torch.int32, device=DEV)
    check(lib.sdc_randn(_p(z), n, seed, 0 if (draw == 0 and seed == 0) else _p(dd), _stream()), "sdc_randn")   # null = draw 0
    torch.cuda.synchronize()
    got = z.cpu().numpy().astype(np.float64)
    want = philox.normals(seed, draw, n)
    err = np.abs(got - want)
    i = int(err.argmax())
    print(f"[measured] sdc_randn seed {seed} draw {draw}: max|err| {err.max():.3e} at element {i} (want {want[i]:.6f}), "
          f"mean|err| {err.mean():.3e}")
    assert 4 * RANDN_MEASURED < RANDN_CEILING
    assert err.max() <= 4 * RANDN_MEASURED


def test_advance_counters():
    lib = _lib.get_lib()
    s = _stream()
    t_dev = torch.tensor([10], dtype=torch.int32, device=DEV)
    draw_dev = torch.tensor([1], dtype=torch.int32, device=DEV)
    for skip in (0, 1, 1):                                                # the samplers advance by 1 + skip_draws draws
        check(lib.sdc_advance(_p(t_dev), -1, _p(draw_dev), 1 + skip, s), "sdc_advance")
    check(lib.sdc_advance(0, -1, _p(draw_dev), 1, s), "sdc_advance")      # either counter may be absent
    check(lib.sdc_advance(_p(t_dev), -2, 0, 1, s), "sdc_advance")
    torch.cuda.synchronize()
    assert t_dev.item() == 10 - 3 - 2 and draw_dev.item() == 1 + 1 + 2 + 2 + 1
    ttab = torch.tensor([900, 600, 300, 42], dtype=torch.int32, device=DEV)   # S = 3 steps + the final entry
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    t_dev.fill_(900)
    draw_dev.fill_(1)
    seen = []
    for _ in range(3):
        check(lib.sdc_advance_table(_p(idx), _p(t_dev), _p(ttab), _p(draw_dev), 1, s), "sdc_advance_table")
        torch.cuda.synchronize()
        seen.append((idx.item(), t_dev.item(), draw_dev.item()))
    assert seen == [(1, 600, 2), (2, 300, 3), (3, 42, 4)]                 # the table's final entry is read
    idx.zero_()
    check(lib.sdc_advance_table(_p(idx), _p(t_dev), _p(ttab), 0, 1, s), "sdc_advance_table")
    torch.cuda.synchronize()
    assert (idx.item(), t_dev.item(), draw_dev.item()) == (1, 600, 4)


# ------------------------------------------------------------------ sdc_conformal_score
def _conformal_shapes(model):
    if model == BURGERS:
        return [((3, H, W), 10) for H, W in BURGERS_HW]
    if model == TOKAMAK:
        return [((12, L), nt) for L, nt in TOKAMAK_LNT]
    return [((F, 7, H, W), 0) for F, H, W in SMOKE_FHW]


@pytest.mark.parametrize("model,use_max", [(BURGERS, 0), (BURGERS, 1), (TOKAMAK, 0), (SMOKE, 0)],
                         ids=["burgers-mean", "burgers-amax", "tokamak", "smoke"])
def test_conformal_score(model, use_max):
    """score |f(pred) - f(truth)| and weight exp(-J(truth)) against osam.*_score / *_weight in fp64.

    Bound: a block sum of n terms is a chain of at most D = ceil(n / 256) + 10 additions (the thread's serial part, six
    shuffle steps, four wave partials), so it is off by at most D u sum|v|; scaling and dividing add 2.  f therefore
    carries (D + 2) u fs with fs = S mean|v| (one rounding, u |f|, for an amax / amin).  The score adds its subtraction:
    (D + 3) u (fs(pred) + fs(truth)).  J adds, on its own terms Js (|w| (fs + |Q| + |bound|), the tokamak objective
    mean((|S x| + |target|)^2) with 5 roundings a term, the smoke mean of channel 5), at most 8 more operations, and
    expf at most 2 ulp and the store 1, so |weight - ref| <= weight (D + 10) u (Js + 1).  D is taken for the longest sum."""
    lib = _lib.get_lib()
    worst_s = worst_w = 0.0
    for i, (shape, ci) in enumerate(_conformal_shapes(model)):
        B = 3
        c = new_case(model, B, shape, ci, use_max=use_max)
        g = torch.Generator().manual_seed(300 + 10 * model + i)
        pred, truth = 0.5 * torch.randn(B, *shape, generator=g), 0.5 * torch.randn(B, *shape, generator=g)
        target = torch.randn(B, 3, ci, generator=g) if model == TOKAMAK else None
        p64, t64 = pred.double(), truth.double()
        absf = lambda v: functional(c, v) if extremum_mode(c) else functional(c, v.abs())   # noqa: E731
        if model == BURGERS:
            gpar = torch.tensor([0.5, 0.5625, 0.25, 10.0, 0, 0, 0, 0])
            gp = [float(v) for v in gpar]
            ws, wt = osam.burgers_score(p64, t64, not use_max), osam.burgers_weight(t64, gp[2], gp[0], 0.75, not use_max)
            n = 11 * shape[2]
            Js = gp[0] * (absf(t64).abs() + gp[2] + gp[1])
        elif model == TOKAMAK:
            gpar = torch.tensor([0.5, 2.0, 0.25, 0.5, 0.125, 0, 0, 0])
            gp = [float(v) for v in gpar]
            ws = osam.tokamak_score(p64, t64, ci)
            wt = osam.tokamak_weight(t64, target.double(), ci, gp[4], gp[3], gp[0], gp[1], gp[2])
            n = 2 * ci
            obj = sum(((TOK_S[ch] * t64[:, ch, :ci]).abs() + target.double()[:, ch].abs()).square().mean(-1) for ch in (0, 2))
            Js = gp[2] * (gp[0] * obj + gp[1] * (gp[3] + absf(t64).abs() + gp[4]))
        else:
            gpar = torch.tensor([0.75, 0.5, 0.125, 0.75, 0, 0, 0, 0])
            gp = [float(v) for v in gpar]
            ws, wt = osam.smoke_score(p64, t64), osam.smoke_weight(t64, gp[2], gp[0], gp[1], gp[3])
            n = shape[0] * shape[2] * shape[3]
            Js = gp[3] * ((1 - gp[0]) * t64[:, :, 5].abs().mean((-1, -2, -3)) + gp[0] * (absf(t64).abs() + gp[2] + gp[1]))
        D = -(-n // 256) + 10
        fs = absf(p64).abs() + (absf(t64).abs() if model != SMOKE else t64[:, -1, 6, 0, 0].abs())
        d = make_desc(c)
        score = torch.full((B,), SENT, device=DEV)
        weight = torch.full((B,), SENT, device=DEV)
        pd, td, tg, gd = _dev(pred), _dev(truth), _dev(target), _dev(gpar)
        check(lib.sdc_conformal_score(C.byref(d), _p(pd), _p(td), _p(tg), _p(gd), _p(score), _p(weight), _stream()),
              "sdc_conformal_score")
        torch.cuda.synchronize()
        es = (score.cpu().double() - ws).abs() / (U * fs)
        ew = (weight.cpu().double() - wt).abs() / (U * wt * (Js + 1.0))
        worst_s, worst_w = max(worst_s, es.max().item() / (D + 3)), max(worst_w, ew.max().item() / (D + 10))
        assert (es <= (D + 3) * SLACK).all(), (case_id(c), es.tolist(), D + 3)
        assert (ew <= (D + 10) * SLACK).all(), (case_id(c), ew.tolist(), D + 10)
    print(f"[measured] sdc_conformal_score {NAME[model]} use_max {use_max}: worst score error {worst_s:.3f} of its bound, "
          f"worst weight error {worst_w:.3f} of its bound")


def test_zz_report_measured():
    """the maxima the comparisons above recorded, in units of u scale (runs last in this file)"""
    for tag in sorted(MEASURED):
        print(f"[measured] max over cases, {tag}: {MEASURED[tag]:.2f} u scale")
