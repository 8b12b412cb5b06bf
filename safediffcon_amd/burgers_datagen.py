"""Burgers data generator: what 1D/data/generate_burgers.py does to make the 1-D Burgers task's training trajectories.

  make_data_varying_f / make_data            generate_burgers.py:302-418   -> draw_parameters + the field synthesis
  burgers_numeric_solve (uniform / const)    generate_burgers.py:113-205   -> burgers_numeric_solve
  burgers_numeric_solve_free                 generate_burgers.py:207-299   -> burgers_numeric_solve_free_wave
  generate_data_burgers_equation / log_info  generate_burgers.py:421-583   -> BurgersDataGenerator.generate / .save

The reference draws a few dozen numbers per sample and then materialises sums of eight space x time Gaussians in float64 on
the host.  Here the draws stay on the host (`draw_parameters`, the reference's `np.random` order), the fields are evaluated by
`sdc_burgers_synth` (force="device": float64 in the reference's operation order, rounded once to fp32; the device's `exp` is not
numpy's, so a value may land on the neighbouring fp32) or by numpy exactly as the reference does (force="host": the reference's
bits, slow), and the rollouts run in `sdc_burgers_rollout_wave` (csrc/sdc_burgers_gen.hip: one wave per trajectory, state in
registers, bit for bit the fp32 CPU run).  `uniform` and `const` mode index the forces in the kernel; nothing is expanded.
HDF5 is not written: `.save` writes .npz files with the reference's dataset and attribute names (INTEGRATION.md has the h5py
lines that convert them).  No CPU fallback.
"""
import math
import os
import random

import numpy as np
import torch

from . import _lib, solvers
from ._lib import check

WAVE_MAX_S = 512                        # a wave holds 64 lanes x 8 cells
N_TERMS = 8


# ------------------------------------------------------------------------------------------------ parameters and fields
def draw_parameters(rs, Nu0, Nf, varying=True):
    """The reference's draws, in its order, from `rs` (a np.random.RandomState, or None for the global np.random):
    -> upar (Nu0, 6) float64 {loc1, amp1, sig1, loc2, amp2, sig2}, fpar (Nf, 8, 5) float64 {amp, xloc, xsig, tloc, tsig}.
    Term 0 has a plain amplitude, terms 1 .. 7 a randint(2) factor drawn before it.  varying (make_data_varying_f): amp, xloc,
    xsig, tloc, tsig; otherwise (make_data): loc, amp, sig, and tloc = 0, tsig = 1 unused.  The sigmas carry their 0.5."""
    rs = np.random if rs is None else rs
    upar = np.empty((Nu0, 6))
    for k, (lo, hi) in enumerate(((0.2, 0.4), (0, 2), (0.05, 0.15), (0.6, 0.8), (-2, 0), (0.05, 0.15))):
        upar[:, k] = rs.uniform(lo, hi, (Nu0, 1))[:, 0]
    fpar = np.zeros((Nf, N_TERMS, 5))
    fpar[:, :, 4] = 1.0

    def amp(k):
        if k == 0:
            return rs.uniform(-1.5, 1.5, (Nf, 1))[:, 0]
        gate = rs.randint(2, size=(Nf, 1))
        return (gate * rs.uniform(-1.5, 1.5, (Nf, 1)))[:, 0]
    for k in range(N_TERMS):
        if varying:
            fpar[:, k, 0] = amp(k)
            fpar[:, k, 1] = rs.uniform(0, 1, (Nf, 1))[:, 0]
            fpar[:, k, 2] = (rs.uniform(0.1, 0.4, (Nf, 1)) * 0.5)[:, 0]
            fpar[:, k, 3] = rs.uniform(0, 1, (Nf, 1))[:, 0]
            fpar[:, k, 4] = (rs.uniform(0.1, 0.4, (Nf, 1)) * 0.5)[:, 0]
        else:
            fpar[:, k, 1] = rs.uniform(0, 1, (Nf, 1))[:, 0]
            fpar[:, k, 0] = amp(k)
            fpar[:, k, 2] = (rs.uniform(0.1, 0.4, (Nf, 1)) * 0.5)[:, 0]
    return upar, fpar


def space_grid(s):
    """the reference's fp32 grid of the s interior points"""
    dx = 1.0 / (s + 1)
    return torch.linspace(0.0 + dx, 1.0 - dx, s)


def time_grid(t, tmax=1.0):
    dt = (tmax - 0.0) / (t + 1)
    return torch.linspace(0.0 + dt, tmax - dt, t)


def control_mask(partial_control, s):
    """-> (mask (s) float32 or None, factor on amp_compensate)"""
    if partial_control is None:
        return None, 1
    if partial_control == "front_rear_quarter":
        mask = np.zeros(s, np.float32)
        mask[np.hstack((np.arange(0, s // 4), np.arange(3 * s // 4, s)))] = 1.0
        return mask, 2
    raise ValueError("invalid partial control mode")


def _gauss(d, sig):
    return np.exp(-0.5 * d ** 2 / sig ** 2)


def synth_u0_host(upar, x):
    """(Nu0, s) float64, numpy in the reference's operation order"""
    xv = x.numpy()[None, :]
    p = [upar[:, k:k + 1] for k in range(6)]
    return p[1] * _gauss(xv - p[0], p[2]) + p[4] * _gauss(xv - p[3], p[5])


def synth_f_host(fpar, x, ts, mask, comp, alpha=1.0):
    """(Nf, Nt, s) float32 tensor (ts given) or (Nf, s) float64 array (ts None: make_data's form), the reference's order"""
    if ts is None:
        xv = x.numpy()[None, :]
        f = None
        for k in range(N_TERMS):
            term = fpar[:, k, 0:1] * _gauss(xv - fpar[:, k, 1:2], fpar[:, k, 2:3])
            f = term if f is None else f + term
        return f
    xv, tv = x.numpy()[None, None, :], ts.numpy()[None, :, None]
    f = None
    for k in range(N_TERMS):
        p = [fpar[:, k, j].reshape(-1, 1, 1) for j in range(5)]
        es = _gauss(xv - p[1], p[2])
        es = es * (np.ones(x.numel(), np.float32) if mask is None else mask)[None, None, :]
        et = comp * _gauss(tv - p[3], p[4])
        term = (p[0] * es) * et
        f = term if f is None else f + term
    f = torch.from_numpy(f).to(torch.float32)
    if alpha != 1.:
        f = (f * alpha).clamp(-10., 10.)
    return f


def _synth_device(upar, fpar, x, ts, mask, comp, alpha, device):
    """sdc_burgers_synth -> u0 (Nu0, s), f (Nf, Nt, s) fp32 on `device`"""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("safediffcon_amd.burgers_datagen runs on MI355X only (no CPU fallback)")
    s = x.numel()
    Nu0, Nf, Nt = len(upar), len(fpar), (1 if ts is None else ts.numel())
    d_x = x.to(device=device, dtype=torch.float32).contiguous()
    d_ts = None if ts is None else ts.to(device=device, dtype=torch.float32).contiguous()
    d_mask = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.float32)).to(device)
    d_up = torch.from_numpy(np.ascontiguousarray(upar, np.float64)).to(device)
    d_fp = torch.from_numpy(np.ascontiguousarray(fpar, np.float64)).to(device)
    u0 = torch.empty(Nu0, s, dtype=torch.float32, device=device)
    f = torch.empty(Nf, Nt, s, dtype=torch.float32, device=device)

    def ptr(t):
        return 0 if t is None else t.data_ptr()
    check(_lib.get_lib().sdc_burgers_synth(ptr(d_up), ptr(d_fp), ptr(d_x), ptr(d_ts), ptr(d_mask), float(comp), float(np.float32(alpha)),
                                           ptr(u0), ptr(f), Nu0, Nf, s, Nt, torch.cuda.current_stream(device).cuda_stream),
          "sdc_burgers_synth")
    return u0, f


def _check_force(force):
    if force not in ("host", "device"):
        raise ValueError('force: "host" or "device"')


def make_data_varying_f(Nu0, Nf, s, t, amp_compensate=2, partial_control=None, alpha=1., tmax=1., rs=None, force="device",
                        device="cuda"):
    """The reference's function plus `rs` (a RandomState; None: the global np.random, as there) and `force`.
    force="host": (u0 (Nu0, s) float64 array, f (Nf, t, s) float32 CPU tensor), the reference's bits;
    force="device": both as fp32 tensors on `device`, within one fp32 rounding of them."""
    _check_force(force)
    if not math.isfinite(tmax):
        raise ValueError("tmax is not finite: the time grid, and with it every force value, would be NaN "
                         "(the reference's --stretching_f False passes torch.nan here)")
    mask, factor = control_mask(partial_control, s)
    comp = amp_compensate * factor
    upar, fpar = draw_parameters(rs, Nu0, Nf, varying=True)
    x, ts = space_grid(s), time_grid(t, tmax)
    if force == "host":
        return synth_u0_host(upar, x), synth_f_host(fpar, x, ts, mask, comp, alpha)
    return _synth_device(upar, fpar, x, ts, mask, comp, alpha, device)


def make_data(Nu0, Nf, s, rs=None, force="device", device="cuda"):
    """The reference's function plus `rs` and `force`: -> u0 (Nu0, s), f (Nf, s); float64 arrays (host) or fp32 device tensors."""
    _check_force(force)
    upar, fpar = draw_parameters(rs, Nu0, Nf, varying=False)
    x = space_grid(s)
    if force == "host":
        return synth_u0_host(upar, x), synth_f_host(fpar, x, None, None, 1)
    u0, f = _synth_device(upar, fpar, x, None, None, 1, 1., device)
    return u0, f[:, 0]


# ------------------------------------------------------------------------------------------------ rollouts
def _schedule(s, Nt, visc, T, dt):
    """step count, steps per interval and the fp32 coefficients, with the reference loop's failures raised up front
    (as solvers.burgers_numeric_solve_free does)"""
    delta_x = 1.0 / (s + 1)
    steps = math.ceil(T / dt)
    rec = math.floor(steps / Nt)
    if 0 < steps < Nt:
        raise ZeroDivisionError("integer modulo by zero")                    # j % record_time, record_time = 0
    if steps > 0 and steps % Nt != 0:
        raise IndexError(f"index {Nt} is out of bounds for dimension 1 with size {Nt}")   # f[:, f_idx, :] at step Nt * record_time
    ct = float(np.float32(1.0 / (2 * delta_x)))
    d = (visc * np.array([1.0, -2.0, 1.0]) / delta_x ** 2).astype(np.float32)
    return rec, (float(np.float32(dt)), ct, float(d[0]), float(d[1]), float(d[2]))


def _force_view(f):
    """fp32 with unit stride along space; any strides over samples and intervals go to the kernel as they are"""
    f = f.detach().to(torch.float32)
    if f.stride(-1) != 1 or any(st < 0 for st in f.stride()):
        f = f.contiguous()
    return f


def _launch_wave(u0c, fc, f_sn, f_st, N, Nu0, Nf, s, Nt, rec, coef, pair_mode, waves_per_block=0):
    traj = torch.empty(N, Nt + 1, s, dtype=torch.float32, device=u0c.device)
    stream = torch.cuda.current_stream(u0c.device).cuda_stream
    check(_lib.get_lib().sdc_burgers_rollout_wave(u0c.data_ptr(), fc.data_ptr(), traj.data_ptr(), N, Nu0, Nf, s, Nt, rec, f_sn, f_st,
                                                  pair_mode, *coef, waves_per_block, stream), "sdc_burgers_rollout_wave")
    return traj


def burgers_numeric_solve_free_wave(u0, f, visc, T, dt=1e-4, num_t=10, mode=None, waves_per_block=0):
    """solvers.burgers_numeric_solve_free (same signature, semantics, exceptions and bits) on the one-wave-per-trajectory kernel;
    s > 512 goes to that function."""
    if mode == "const":
        raise ValueError
    assert f.size(1) == num_t, "check number of time interval"
    if not u0.is_cuda:
        raise RuntimeError("safediffcon_amd.burgers_datagen runs on MI355X only (no CPU fallback)")
    N, s, Nt = u0.shape[0], u0.size(-1), f.size(1)
    assert f.shape[0] == N
    if s > WAVE_MAX_S:
        return solvers.burgers_numeric_solve_free(u0, f, visc, T, dt=dt, num_t=num_t, mode=mode)
    rec, coef = _schedule(s, Nt, visc, T, dt)
    u0c = u0.detach().reshape(N, s).to(torch.float32).contiguous()
    fc = _force_view(f if f.dim() == 3 else f.reshape(N, Nt, s))
    return _launch_wave(u0c, fc, fc.stride(0), fc.stride(1), N, N, N, s, Nt, rec, coef, 0, waves_per_block)


def burgers_numeric_solve(u0, f, visc, T, dt=1e-4, num_t=10, mode=None):
    """The reference's function: every u0 (Nu0, s) against every f (Nf, Nt, s) -- mode='const': f (Nf, s), the same row in every
    interval -- on the HIP device -> (Nu0, Nf, Nt + 1, s).  The pairs are indexed inside the kernel; s > 512 expands them for
    solvers.burgers_numeric_solve_free."""
    if mode != "const":
        assert f.size(1) == num_t, "check number of time interval"
    if not u0.is_cuda:
        raise RuntimeError("safediffcon_amd.burgers_datagen runs on MI355X only (no CPU fallback)")
    Nu0, s, Nf = u0.size(0), u0.size(-1), f.size(0)
    Nt = num_t if mode == "const" else f.size(1)
    rec, coef = _schedule(s, Nt, visc, T, dt)
    u0c = u0.detach().reshape(Nu0, s).to(torch.float32).contiguous()
    if s > WAVE_MAX_S:
        fe = f.unsqueeze(1).repeat(1, Nt, 1) if mode == "const" else f.reshape(Nf, Nt, s)
        traj = solvers.burgers_numeric_solve_free(u0c.repeat_interleave(Nf, dim=0), fe.repeat(Nu0, 1, 1), visc, T, dt=dt, num_t=Nt)
        return traj.reshape(Nu0, Nf, Nt + 1, s)
    fc = _force_view(f)
    f_sn, f_st = (fc.stride(0), 0) if mode == "const" else (fc.stride(0), fc.stride(1))
    return _launch_wave(u0c, fc, f_sn, f_st, Nu0 * Nf, Nu0, Nf, s, Nt, rec, coef, 1).reshape(Nu0, Nf, Nt + 1, s)


# ------------------------------------------------------------------------------------------------ the script
def shuffled_indices(n, seed=0):
    """what `random.seed(seed); random.sample(range(n), n)` gives"""
    return random.Random(seed).sample(range(n), n)


class BurgersDataGenerator:
    """`generate` = generate_data_burgers_equation for one (nt, nx) resolution; the defaults are the script's."""

    def __init__(self, device="cuda", nt=11, nx=128, save_nt=11, end_time=1., varying_f=True, uniform=False, num_u0=100,
                 num_f=1000, partial_control=None, alpha=1.):
        if torch.device(device).type != "cuda":
            raise RuntimeError("safediffcon_amd.burgers_datagen runs on MI355X only (no CPU fallback)")
        if not 2 <= save_nt <= nt:
            raise ValueError(f"save_nt = {save_nt} outside 2 .. nt = {nt}")
        control_mask(partial_control, nx)                  # the reference's ValueError, before any work
        self.device = torch.device(device)
        self.nt, self.nx, self.save_nt, self.end_time = int(nt), int(nx), int(save_nt), end_time
        self.varying_f, self.uniform, self.num_u0, self.num_f = bool(varying_f), bool(uniform), int(num_u0), int(num_f)
        self.partial_control, self.alpha = partial_control, alpha
        self.key = f"pde_{self.save_nt}-{self.nx}"

    def attributes(self):
        """what log_info stores next to each dataset, from the `burgers` class's fields"""
        dx = 1 / (self.nx + 1)
        return {"dt": self.end_time / (self.nt - 1), "dx": dx, "nt": self.nt, "nx": self.nx, "tmin": 0.0, "tmax": self.end_time,
                "x": torch.linspace(dx, 1 - dx, self.nx)}

    def _solve_free(self, u0, f):
        return burgers_numeric_solve_free_wave(u0, f, visc=0.01, T=self.end_time, dt=1e-4, num_t=self.nt - 1)

    def _free(self, n, rs, force, chunk, timing):
        s, t, dev = self.nx, self.nt - 1, self.device
        if not math.isfinite(self.end_time):
            raise ValueError("end_time is not finite: every force value would be NaN")
        mask, factor = control_mask(self.partial_control, s)
        comp = 2 * factor
        upar, fpar = draw_parameters(rs, n, n, varying=True)
        x, ts = space_grid(s), time_grid(t, self.end_time)
        u = torch.empty(n, self.save_nt, s, dtype=torch.float32, device=dev)
        fo = torch.empty(n, self.save_nt - 1, s, dtype=torch.float32, device=dev)
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            with _timed(timing, "synthesis_s", dev):
                if force == "host":
                    u0 = torch.from_numpy(synth_u0_host(upar[lo:hi], x)).to(torch.float32).to(dev)
                    f = synth_f_host(fpar[lo:hi], x, ts, mask, comp, self.alpha).to(dev)
                else:
                    u0, f = _synth_device(upar[lo:hi], fpar[lo:hi], x, ts, mask, comp, self.alpha, dev)
            with _timed(timing, "rollout_s", dev):
                traj = self._solve_free(u0, f)
            u[lo:hi] = traj[:, -self.save_nt:]
            fo[lo:hi] = f[:, -(self.save_nt - 1):]
        return u, fo

    def _uniform(self, rs, force, chunk, timing):
        s, t, dev = self.nx, self.nt - 1, self.device
        with _timed(timing, "synthesis_s", dev):
            if self.varying_f:
                u0, f = make_data_varying_f(self.num_u0, self.num_f, s, t, rs=rs, force=force, device=dev)
            else:
                u0, f = make_data(self.num_u0, self.num_f, s, rs=rs, force=force, device=dev)
            if force == "host":
                u0, f = torch.from_numpy(u0).to(torch.float32).to(dev), torch.as_tensor(f).to(torch.float32).to(dev)
        n, mode = self.num_u0 * self.num_f, None if self.varying_f else "const"
        u = torch.empty(self.num_u0, self.num_f, self.save_nt, s, dtype=torch.float32, device=dev)
        rows = max(1, chunk // self.num_f)
        for lo in range(0, self.num_u0, rows):
            with _timed(timing, "rollout_s", dev):
                traj = burgers_numeric_solve(u0[lo:lo + rows], f, visc=0.01, T=self.end_time, dt=1e-4, num_t=t, mode=mode)
            u[lo:lo + rows] = traj[:, :, -self.save_nt:]
        frows = (f if self.varying_f else f.unsqueeze(1).expand(-1, t, -1))[:, -(self.save_nt - 1):]
        fo = frows.unsqueeze(0).expand(self.num_u0, -1, -1, -1).reshape(n, self.save_nt - 1, s)
        return u.reshape(n, self.save_nt, s), fo

    def generate(self, num_train, num_test, seed=0, force="device", chunk=8192, timing=None):
        """-> {"train": {...}, "test": {...}}, each {"pde_<save_nt>-<nx>": (n, save_nt, nx), "pde_<save_nt>-<nx>_f": (n, save_nt - 1, nx)
        float64 device tensors, "attrs": {dt, dx, nt, nx, tmin, tmax, x}}.  The parameters come from RandomState(seed), the shuffle
        from random.Random(seed); fields and rollouts are made `chunk` trajectories at a time.  timing: a dict that receives
        synthesis_s / rollout_s / shuffle_s (each part synchronised; leave None otherwise)."""
        _check_force(force)
        n = num_train + num_test
        if self.uniform:
            assert self.num_u0 * self.num_f == n, "number of all samples should == Nu0 * Nf"
            assert not self.partial_control, "only varying_f settings are supported for partial control"
            assert self.alpha == 1.
        else:
            assert self.varying_f, "Only supports varying_f when every f is paired with a different u0"
        if num_train < 0 or num_test <= 0 or chunk <= 0:
            raise ValueError("num_train >= 0, num_test > 0 and chunk > 0 expected")      # [-0:] would take every row
        rs = np.random.RandomState(seed)
        u, f = self._uniform(rs, force, chunk, timing) if self.uniform else self._free(n, rs, force, chunk, timing)
        with _timed(timing, "shuffle_s", self.device):
            order = torch.tensor(shuffled_indices(n, seed), dtype=torch.long, device=self.device)
            out = {}
            for split, idx in (("train", order[:num_train]), ("test", order[n - num_test:])):
                out[split] = {self.key: u.index_select(0, idx).double(), self.key + "_f": f.index_select(0, idx).double(),
                              "attrs": self.attributes()}
        return out

    def save(self, directory, record):
        """<directory>/burgers_train.npz and burgers_test.npz: the two datasets under the reference's names, float64, and every
        attribute as "<dataset>/<attr>".  -> the two paths"""
        os.makedirs(directory, exist_ok=True)
        paths = []
        for split in ("train", "test"):
            arrs = {}
            for name, v in record[split].items():
                if name == "attrs":
                    continue
                arrs[name] = v.detach().cpu().numpy().astype(np.float64)
                if name.endswith("_f"):
                    continue                               # log_info puts the attributes on the trajectories' dataset only
                for a, av in record[split]["attrs"].items():
                    arrs[f"{name}/{a}"] = av.cpu().numpy() if torch.is_tensor(av) else np.asarray(av)
            path = os.path.join(directory, f"burgers_{split}.npz")
            np.savez(path, **arrs)
            paths.append(path)
        return paths


class _timed:
    """adds the synchronised wall time of a block to timing[key]; does nothing (no synchronisation) without a timing dict"""

    def __init__(self, timing, key, device):
        self.timing, self.key, self.device = timing, key, device

    def __enter__(self):
        if self.timing is not None:
            import time
            torch.cuda.synchronize(self.device)
            self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        if self.timing is not None:
            import time
            torch.cuda.synchronize(self.device)
            self.timing[self.key] = self.timing.get(self.key, 0.0) + time.perf_counter() - self.t0
        return False
