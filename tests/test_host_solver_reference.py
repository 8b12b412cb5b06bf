"""-m "not gpu": proves the reference tests/test_gpu_solver.py holds the Burgers rollout kernel to.  oracle.solvers.burgers_rollout_np
(NumPy float32, one step per iteration, the kernel's operation order and its guards) equals the torch oracle -- itself equal to the
reference solver's fixture -- bit for bit, over sizes on both sides of a wave and of the 1024-thread group, a single cell, and a
viscosity away from 0.01; and with guards=False it raises where the reference solver raises."""
import numpy as np
import pytest
import torch

from oracle import solvers as osolv
from oracle.detweights import det_tensor


# (N, s, Nt, visc, T), dt = 1e-4, inputs 0.3 * randn
SETTINGS = [(2, 37, 3, 0.01, 0.03), (2, 130, 10, 0.01, 0.1), (1, 1500, 2, 1e-4, 0.02), (3, 1, 5, 0.01, 0.05)]


@pytest.mark.parametrize("N,s,Nt,visc,T", SETTINGS)
def test_numpy_reference_equals_the_oracle(N, s, Nt, visc, T):
    u0 = det_tensor((N, s), 300 + s, 0.3)
    f = det_tensor((N, Nt, s), 301 + s, 0.3)
    want = osolv.burgers_rollout(u0, f, visc=visc, T=T, dt=1e-4).numpy()
    got = osolv.burgers_rollout_np(u0, f, visc=visc, T=T, dt=1e-4)
    assert got.dtype == np.float32 and got.shape == (N, Nt + 1, s)
    assert np.isfinite(want).all() and np.count_nonzero(want[:, -1]) > 0
    assert np.array_equal(got, want)
    # steps % Nt == 0 here, so the guards never act
    assert np.array_equal(osolv.burgers_rollout_np(u0, f, visc=visc, T=T, dt=1e-4, guards=False), want)


def test_numpy_reference_equals_the_reference_fixture(golden):
    """10 000 steps at s = 128 against what the reference's burgers_numeric_solve_free wrote: equal, not close."""
    g = golden("burgers_rollout")
    got = osolv.burgers_rollout_np(g["u0"], g["f"], visc=0.01, T=1.0, dt=1e-4)
    assert np.array_equal(got, g["traj"].numpy())


def test_numpy_reference_takes_views_and_fp64_without_touching_them():
    big = det_tensor((2, 3, 8, 37), 310, 0.3).double()
    keep = big.clone()
    u0, f = big[:, 0, 0, :], big[:, 1, :3, :]
    assert not f.is_contiguous()
    got = osolv.burgers_rollout_np(u0, f, T=0.03)
    want = osolv.burgers_rollout_np(u0.float().contiguous().numpy(), f.float().contiguous().numpy(), T=0.03)
    assert np.array_equal(got, want) and torch.equal(big, keep)


def test_guards_follow_the_c_entry_and_unguarded_raises_like_the_reference():
    u0 = det_tensor((2, 37), 320, 0.3)
    f3 = det_tensor((2, 3, 37), 321, 0.3)
    # 1000 steps, Nt = 3: rec = 333, step 999 has force row index 3
    with pytest.raises(IndexError):
        osolv.burgers_rollout_np(u0, f3, T=0.1, guards=False)
    with pytest.raises(IndexError):
        osolv.burgers_rollout(u0, f3, T=0.1)
    got = osolv.burgers_rollout_np(u0, f3, T=0.1)
    # the guarded run is the 999-step run: the 1000th step (zero force) is never recorded
    f_pad = torch.cat((f3, torch.zeros(2, 1, 37)), dim=1)
    u = u0
    for k in range(3):
        u = torch.from_numpy(osolv.burgers_rollout_np(u, f_pad[:, k:k + 1], T=0.0333))[:, 1]
        assert np.array_equal(got[:, k + 1], u.numpy())
    # 5 steps, Nt = 10: rec = 0
    f10 = det_tensor((2, 10, 37), 322, 0.3)
    with pytest.raises(ZeroDivisionError):
        osolv.burgers_rollout_np(u0, f10, T=5e-4, guards=False)
    with pytest.raises(ZeroDivisionError):
        osolv.burgers_rollout(u0, f10, T=5e-4)
    with pytest.raises(ValueError):
        osolv.burgers_rollout_np(u0, f10, T=5e-4)


def test_step_counts_that_float_rounding_moves():
    """ceil(T / dt) in float64, as the reference computes it.  The double nearest 1e-4 lies above 1e-4, so a quotient that is
    not exact falls below its integer (0.3/1e-4 = 2999.9999999999995, 0.7/1e-4 = 6999.999999999999, 0.09/1e-4 = 899.9999999999999)
    and ceil brings it back: no multiple of 1e-4 up to 1.2 gains a step, and floor(T / dt) would lose one."""
    import math
    assert 0.3 / 1e-4 < 3000 and 0.7 / 1e-4 < 7000 and 0.09 / 1e-4 < 900
    assert [math.ceil(T / 1e-4) for T in (0.3, 0.7, 1.1, 0.03, 0.07, 0.09)] == [3000, 7000, 11000, 300, 700, 900]
    assert all(math.ceil(float("%g" % (k / 10000)) / 1e-4) == k for k in range(1, 12001))
