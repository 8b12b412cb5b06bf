"""Oracle: Burgers' finite-difference rollout, restating burgers_numeric_solve_free
(1D/data/generate_burgers.py:207-299): same fp32 operation order, plain torch on the CPU.

TEST INFRASTRUCTURE -- see oracle/__init__.py."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def burgers_rollout(u0, f, visc=0.01, T=1.0, dt=1e-4):
    N, s = u0.shape
    Nt = f.shape[1]
    dx = 1.0 / (s + 1)
    steps = math.ceil(T / dt)
    rec = math.floor(steps / Nt)
    ct = torch.tensor(np.array([-1.0, 1.0]) / (2 * dx), dtype=torch.float32)
    dc = torch.tensor(visc * np.array([1.0, -2.0, 1.0]) / dx ** 2, dtype=torch.float32)
    u = F.pad(u0.reshape(N, s), (1, 1))
    fp = F.pad(f.reshape(N, Nt, s), (1, 1))
    sol = torch.zeros(N, Nt, s)
    c, fidx = 0, -1
    for j in range(steps):
        u = F.pad(u[:, 1:-1], (1, 1))
        us = u ** 2
        tr = torch.zeros_like(u)
        tr[:, 1:-1] = us[:, :-2] * ct[0] + us[:, 2:] * ct[1]
        df = torch.zeros_like(u)
        df[:, 1:-1] = (u[:, :-2] * dc[0] + u[:, 1:-1] * dc[1]) + u[:, 2:] * dc[2]
        if j % rec == 0:
            fidx += 1
        u = u + dt * (-(1 / 2) * tr + df + fp[:, fidx, :])
        if (j + 1) % rec == 0:
            sol[:, c] = u[:, 1:-1]
            c += 1
    return torch.cat((u0.reshape(N, 1, s), sol), dim=1)


def burgers_rollout_np(u0, f, visc=0.01, T=1.0, dt=1e-4, guards=True):
    """The same rollout in NumPy float32, one Euler step per loop iteration, sharing no code with burgers_rollout above or with
    csrc/sdc_solver.hip: every product and sum is a separate float32 operation (NumPy never contracts to FMA), the transport
    sum is u^2_{i-1} * (-ct) + u^2_{i+1} * ct, the diffusion sum (u_{i-1} d0 + u_i d1) + u_{i+1} d2, and ct, d0..d2, dt are
    rounded to float32 from float64 the way safediffcon_amd/solvers.py rounds them.  u0 (N,s), f (N,Nt,s), arrays or CPU
    tensors of any float type -> float32 array (N, Nt+1, s).

    guards=True is the C entry's defined behaviour for a step count Nt does not divide: zero force once the force row index
    reaches Nt, no snapshot once Nt have been taken.  guards=False indexes like the reference and so raises where it raises:
    IndexError for steps % Nt != 0 (f[:, Nt]), ZeroDivisionError for 0 < steps < Nt (j % 0)."""
    u0 = np.ascontiguousarray(np.asarray(u0), dtype=np.float32)
    f = np.ascontiguousarray(np.asarray(f), dtype=np.float32)
    N, s = u0.shape
    Nt = f.shape[1]
    assert f.shape == (N, Nt, s)
    dx = 1.0 / (s + 1)
    steps = math.ceil(T / dt)
    rec = math.floor(steps / Nt)
    if guards and rec == 0:
        raise ValueError("burgers_rollout_np: fewer steps than force intervals (the C entry returns SDC_EINVAL)")
    ct = np.float32(1.0 / (2 * dx))
    nct = np.float32(-ct)
    d0, d1, d2 = (visc * np.array([1.0, -2.0, 1.0]) / dx ** 2).astype(np.float32)
    dt32, mhalf = np.float32(dt), np.float32(-0.5)
    zero_force = np.zeros((N, s), np.float32)
    u = np.zeros((N, s + 2), np.float32)
    u[:, 1:-1] = u0
    traj = np.zeros((N, Nt + 1, s), np.float32)
    traj[:, 0] = u0
    c, fidx = 0, -1
    with np.errstate(all="ignore"):
        for j in range(steps):
            if j % rec == 0:
                fidx += 1
            um, uc, up = u[:, :-2], u[:, 1:-1], u[:, 2:]
            fv = zero_force if (guards and fidx >= Nt) else f[:, fidx]
            tr = (um * um) * nct + (up * up) * ct
            df = (um * d0 + uc * d1) + up * d2
            un = uc + dt32 * ((mhalf * tr + df) + fv)
            assert un.dtype == np.float32
            u = np.zeros_like(u)
            u[:, 1:-1] = un
            if (j + 1) % rec == 0 and not (guards and c >= Nt):
                traj[:, c + 1] = un
                c += 1
    return traj
