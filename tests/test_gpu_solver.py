"""-m gpu: Burgers' finite-difference evaluation rollout (sdc_burgers_rollout, csrc/sdc_solver.hip: all Euler steps in one kernel).

The first two tests compare with the reference solver's fixture and with the torch oracle on fresh inputs, and pin the domain's
size-independent properties.  Every test after them holds the kernel to its header's promise -- "results match the fp32 CPU run bit
for bit" -- with torch.equal against oracle.solvers.burgers_rollout_np (NumPy float32, proven equal to the torch oracle and to the
reference's fixture by tests/test_host_solver_reference.py), one launch of at most 1000 steps each bar the full T = 1 case, across
the launch envelope of the C entry:

  thread count    s = 1, a ragged last wave (37, 65, 130), 1023 (1024 threads, one idle), 1025 / 1500 (strided loop: a thread owns
                  several cells of both LDS rows across the one barrier per step), 8190 (the last size whose rows fit 64 KiB of LDS)
  step schedule   Nt = 1, T / dt quotients that are exact (0.03, 0.07) and that float division leaves below the integer (0.09),
                  steps % Nt != 0 (the C entry's zero-force / stop-recording guards, through ctypes), steps < Nt and s = 8191 refused
                  with the output untouched
  wrapper         fp32 rounding of ct, d0..d2, dt away from visc = 0.01; non-contiguous views and fp64 inputs; a side stream; the
                  reference's exceptions (ValueError, AssertionError, IndexError, ZeroDivisionError)
  values          products that are subnormal in fp32, a NaN / an Inf sample next to finite ones, 300 workgroups in one launch
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import solvers as osolv
from oracle.detweights import det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SDC_EINVAL = -1


def test_rollout_matches_reference_fixture(golden):
    from safediffcon_amd import solvers
    g = golden("burgers_rollout")
    traj = solvers.burgers_numeric_solve_free(g["u0"].to(DEV), g["f"].to(DEV), visc=0.01, T=1.0, dt=1e-4, num_t=10).cpu()
    assert torch.equal(traj, g["traj"])                  # was rtol 1e-5 / atol 1e-6 while the kernel's sums were contracted to FMAs
    assert torch.equal(traj[:, 0], g["u0"])


def test_rollout_properties_and_control_trajectories():
    from safediffcon_amd import solvers
    B = 64
    diffused = det_tensor((B, 3, 16, 128), 5, 0.3)
    out = solvers.control_trajectories(diffused.to(DEV), 11).cpu()
    assert out.shape == (B, 11, 128) and torch.isfinite(out).all()
    ref = osolv.burgers_rollout(diffused[:4, 0, 0, :], diffused[:4, 1, :10, :])
    assert torch.equal(out[:4], ref)
    # zero state + zero force stays zero; the rollout of sample i does not depend on its batch neighbours
    z = solvers.burgers_numeric_solve_free(torch.zeros(2, 128, device=DEV), torch.zeros(2, 10, 128, device=DEV), 0.01, 1.0)
    assert torch.count_nonzero(z) == 0
    sub = solvers.control_trajectories(diffused[10:12].to(DEV), 11).cpu()
    assert torch.equal(sub, out[10:12])


# ------------------------------------------------------------------ bit for bit against the NumPy float32 reference

def _ref(u0, f, visc, T, guards=True):
    return torch.from_numpy(osolv.burgers_rollout_np(u0, f, visc=visc, T=T, dt=1e-4, guards=guards))


def _hip(u0, f, visc, T):
    from safediffcon_amd import solvers
    return solvers.burgers_numeric_solve_free(u0.to(DEV), f.to(DEV), visc=visc, T=T, dt=1e-4, num_t=f.shape[1]).cpu()


def _inputs(N, s, Nt, scale=0.3):
    return det_tensor((N, s), 400 + s, scale), det_tensor((N, Nt, s), 401 + s + Nt, scale)


def _c_entry(u0, f, traj, steps, rec, visc):
    """sdc_burgers_rollout itself, coefficients rounded as solvers.py rounds them; returns the status code after a device sync"""
    from safediffcon_amd import _lib
    N, s = u0.shape
    dx = 1.0 / (s + 1)
    d = (visc * np.array([1.0, -2.0, 1.0]) / dx ** 2).astype(np.float32)
    rc = _lib.get_lib().sdc_burgers_rollout(u0.data_ptr(), f.data_ptr(), traj.data_ptr(), N, s, f.shape[1], steps, rec,
                                            ctypes.c_float(1e-4), ctypes.c_float(1.0 / (2 * dx)), ctypes.c_float(d[0]),
                                            ctypes.c_float(d[1]), ctypes.c_float(d[2]),
                                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


# (s, N, Nt, visc, T).  visc * dt / dx^2 <= 0.11 everywhere: the explicit diffusion step is stable and the references stay finite.
SIZES = [
    (1, 3, 5, 0.01, 0.05),        # one cell, both neighbours ghosts, 63 idle lanes: `threads` rounding, the `i < s` cell loop
    (37, 2, 3, 0.01, 0.03),       # ragged single wave; T / dt = 300.0
    (65, 2, 1, 0.01, 0.07),       # second wave holds one cell; one force interval: rec = steps = 700 in `j % rec`, `record`
    (130, 2, 10, 0.01, 0.09),     # third wave holds two cells; 0.09 / 1e-4 = 899.9999999999999 -> 900 steps (solvers.py ceil)
    (1023, 2, 4, 1e-3, 0.1),      # 1024 threads, the last one idle
    (1025, 2, 4, 1e-3, 0.1),      # the `threads > 1024` cap: first strided size, thread 0 owns cells 0 and 1024
    (1500, 2, 2, 1e-4, 0.1),      # strided cell loop, 476 threads own two cells of cur / nxt across the one __syncthreads per step
    (37, 2, 5, 0.003, 0.1),       # d0..d2 = fp32(0.003 * [1,-2,1] * 38^2): the wrapper's coefficient rounding
    (65, 2, 5, 0.1, 0.1),         # d0..d2 = fp32(0.1 * [1,-2,1] * 66^2)
]


@pytest.mark.parametrize("s,N,Nt,visc,T", SIZES)
def test_bit_exact_across_thread_counts_and_schedules(s, N, Nt, visc, T):
    u0, f = _inputs(N, s, Nt)
    want = _ref(u0, f, visc, T, guards=False)            # steps % Nt == 0: the reference itself runs these
    assert torch.isfinite(want).all() and torch.count_nonzero(want[:, -1]) > 0
    got = _hip(u0, f, visc, T)
    assert got.shape == (N, Nt + 1, s)
    assert torch.equal(got, want)


def test_bit_exact_at_the_lds_limit_and_refused_past_it():
    """s = 8190: two rows of s + 2 floats are exactly 64 KiB, each thread owns 8 cells (the entry's LDS
    bound and the launch's dynamic LDS size).  Smooth small inputs:
    at visc = 1e-6 white noise overflows within 100 steps.  s = 8191 is SDC_EINVAL before any launch."""
    s = 8190
    x = torch.arange(1, s + 1, dtype=torch.float64) / (s + 1)
    k = torch.tensor([[1.0], [3.0]], dtype=torch.float64)
    u0 = (0.01 * torch.sin(2 * np.pi * k * x)).float()
    f = (0.01 * torch.sin(2 * np.pi * (k + 1) * x + 0.5)).float().reshape(2, 1, s)
    want = _ref(u0, f, 1e-6, 0.02, guards=False)         # 200 steps
    assert torch.isfinite(want).all() and not torch.equal(want[:, 1], want[:, 0])
    assert torch.equal(_hip(u0, f, 1e-6, 0.02), want)
    s = 8191
    traj = torch.full((1, 2, s), float("nan"), device=DEV)
    rc = _c_entry(torch.zeros(1, s, device=DEV), torch.zeros(1, 1, s, device=DEV), traj, 200, 200, 1e-6)
    assert rc == SDC_EINVAL and torch.isnan(traj).all()
    from safediffcon_amd import _lib, solvers
    with pytest.raises(_lib.SdcError):
        solvers.burgers_numeric_solve_free(torch.zeros(1, s, device=DEV), torch.zeros(1, 1, s, device=DEV), 1e-6, 0.02, num_t=1)


def test_uneven_intervals_through_the_c_entry():
    """1000 steps, Nt = 3: rec = 333, so step 999 has force row index 3 (the kernel's `fidx < Nt` zero force) and a fourth snapshot
    would be due at step 1332 (its `c < Nt` in `record`).  The reference raises here; the C entry's guards are its documented behaviour (sdc.h)."""
    u0, f = _inputs(2, 130, 3)
    want = _ref(u0, f, 0.01, 0.1, guards=True)
    traj = torch.full((2, 4, 130), float("nan"), device=DEV)
    assert _c_entry(u0.to(DEV), f.to(DEV), traj, 1000, 333, 0.01) == 0
    assert torch.equal(traj.cpu(), want)
    # 1400 steps: snapshots fall due at 333, 666, 999 and again at 1332; the fourth must not be written past the sample's rows
    # (a spare sample's worth of NaN behind the two that run shows it)
    spare = torch.full((3, 4, 130), float("nan"), device=DEV)
    assert _c_entry(u0.to(DEV), f.to(DEV), spare, 1400, 333, 0.01) == 0
    assert torch.equal(spare[:2].cpu(), want) and torch.isnan(spare[2]).all()
    # steps < Nt: record_every = 0 is refused with the output untouched
    traj.fill_(float("nan"))
    assert _c_entry(u0.to(DEV), f.to(DEV), traj, 2, 0, 0.01) == SDC_EINVAL and torch.isnan(traj).all()


def test_reference_exceptions_before_any_launch():
    """1D/data/generate_burgers.py:223-226 (mode, num_t), :284-286 (j % record_time with record_time = 0; f[:, f_idx] with f_idx = Nt)"""
    from safediffcon_amd import solvers
    u0, f = _inputs(2, 37, 3)
    u0, f = u0.to(DEV), f.to(DEV)
    with pytest.raises(ValueError):
        solvers.burgers_numeric_solve_free(u0, f, 0.01, 0.03, num_t=3, mode="const")
    with pytest.raises(AssertionError):
        solvers.burgers_numeric_solve_free(u0, f, 0.01, 0.03, num_t=10)
    with pytest.raises(AssertionError):
        solvers.burgers_numeric_solve_free(u0[:1], f, 0.01, 0.03, num_t=3)
    with pytest.raises(IndexError):                      # 1000 % 3 != 0
        solvers.burgers_numeric_solve_free(u0, f, 0.01, 0.1, num_t=3)
    with pytest.raises(IndexError):
        _ref(u0.cpu(), f.cpu(), 0.01, 0.1, guards=False)
    with pytest.raises(ZeroDivisionError):               # 2 steps, 3 intervals
        solvers.burgers_numeric_solve_free(u0, f, 0.01, 2e-4, num_t=3)
    with pytest.raises(ZeroDivisionError):
        _ref(u0.cpu(), f.cpu(), 0.01, 2e-4, guards=False)
    with pytest.raises(RuntimeError):                    # no CPU fallback
        solvers.burgers_numeric_solve_free(u0.cpu(), f.cpu(), 0.01, 0.03, num_t=3)


def test_subnormal_products_are_not_flushed():
    """Inputs of amplitude 3e-21: u * u ~ 1e-41 is subnormal in fp32 and (u * u) * ct still is; a kernel that flushed denormals would
    lose the whole transport term and differ from the CPU in the last bit of the update."""
    u0, f = _inputs(2, 130, 5, scale=0.3e-20)
    sq = (u0 * u0).abs()
    assert ((sq > 0) & (sq < torch.finfo(torch.float32).tiny)).any()
    want = _ref(u0, f, 0.01, 0.05)
    assert torch.isfinite(want).all() and torch.count_nonzero(want[:, -1]) > 0
    assert torch.equal(_hip(u0, f, 0.01, 0.05), want)
    # and states that are subnormal themselves
    u0, f = _inputs(2, 37, 5, scale=1e-39)
    want = _ref(u0, f, 0.01, 0.05)
    assert torch.count_nonzero(want[:, -1]) > 0 and (want.abs().max() < torch.finfo(torch.float32).tiny)
    assert torch.equal(_hip(u0, f, 0.01, 0.05), want)


def test_non_finite_samples_stay_in_their_rows():
    u0, f = _inputs(5, 130, 5)
    f[2, 1, 40] = float("nan")
    u0[3, 77] = float("inf")
    want = _ref(u0, f, 0.01, 0.05).numpy()
    assert np.isfinite(want[[0, 1, 4]]).all() and np.isfinite(want[2, :2]).all() and np.isnan(want[2, 2:]).any()
    assert not np.isfinite(want[3, 1:]).all()
    got = _hip(u0, f, 0.01, 0.05)
    assert np.array_equal(got.numpy(), want, equal_nan=True)
    keep = [0, 1, 4]
    assert torch.equal(_hip(u0[keep], f[keep], 0.01, 0.05), got[keep])


def test_large_batch_rows_equal_their_single_runs():
    """N = 300 workgroups on 256 CUs: the per-sample offsets of u0, fn, tn and nothing shared between workgroups"""
    u0, f = _inputs(300, 128, 10)
    want = _ref(u0, f, 0.01, 0.1)
    got = _hip(u0, f, 0.01, 0.1)
    assert torch.equal(got, want)
    for n in (0, 255, 256, 299):
        assert torch.equal(_hip(u0[n:n + 1], f[n:n + 1], 0.01, 0.1)[0], got[n])


def test_views_fp64_and_side_stream():
    """the control_trajectories layout: u0 and f are strided slices of the sampler's (B, C, padded_time, space) output"""
    from safediffcon_amd import solvers
    diffused = det_tensor((3, 3, 16, 130), 430, 0.3)
    want = _ref(diffused[:, 0, 0, :], diffused[:, 1, :10, :], 0.01, 0.1)
    for src in (diffused.to(DEV), diffused.double().to(DEV)):
        keep = src.clone()
        u0, f = src[:, 0, 0, :], src[:, 1, :10, :]
        assert not f.is_contiguous()
        got = solvers.burgers_numeric_solve_free(u0, f, visc=0.01, T=0.1, dt=1e-4, num_t=10)
        assert got.dtype == torch.float32 and torch.equal(got.cpu(), want)
        assert torch.equal(src, keep)
    src = diffused.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = solvers.burgers_numeric_solve_free(src[:, 0, 0, :], src[:, 1, :10, :], visc=0.01, T=0.1, dt=1e-4, num_t=10)
    side.synchronize()
    assert torch.equal(got.cpu(), want)


def test_full_rollout_through_control_trajectories():
    """the one full T = 1 case: 10 000 steps at a ragged s, through the caller the score check uses"""
    from safediffcon_amd import solvers
    diffused = det_tensor((2, 3, 16, 130), 440, 0.3)
    want = _ref(diffused[:, 0, 0, :], diffused[:, 1, :10, :], 0.01, 1.0, guards=False)
    assert torch.isfinite(want).all()
    assert torch.equal(solvers.control_trajectories(diffused.to(DEV), 11).cpu(), want)
