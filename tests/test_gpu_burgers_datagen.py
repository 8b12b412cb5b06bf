"""-m gpu: the Burgers data generator's kernels (csrc/sdc_burgers_gen.hip) and the generator on top of them.

Rollouts: sdc_burgers_rollout_wave keeps a trajectory in one wave's registers, lane l owning the K = ceil(s / 64) cells [l K, l K + K).
Every comparison is torch.equal against oracle.solvers.burgers_rollout_np (NumPy float32, proven equal to the reference by
tests/test_host_solver_reference.py) or against the reference generator's own fixtures:

  lane map      every K in {1, 2, 4, 8} at its full size, one past the previous one and a ragged one: a single live lane (s = 1), lane
                63's right ghost (64), a dead cell inside the last live lane (65, 129, 257), dead lanes behind it
  launch        a block that is not full (N = 3, 5 at four waves per block), 1030 trajectories, waves_per_block 1, 2, 3, 4, 8, 16
  indexing      cross pairs (ui = n / Nf, fi = n % Nf), one force row for every interval (f_st = 0), a strided f view, fp64, a side stream
  values        subnormal products, a NaN / an Inf trajectory next to finite ones
  s = 513       the wrapper's fallback to the LDS kernel, SDC_EINVAL with the output untouched through the C entry

Synthesis: sdc_burgers_synth against the numpy float64 evaluation that reproduces the reference bit for bit (test_host_burgers_datagen.py).
Both are the same float64 expressions in the same order bar exp itself: two correctly-working exps differ by an ulp or so of a value
<= 1, each of the eight terms is at most |amp| comp <= 6 in size, so the float64 sums differ by about 1e-14 at most and their fp32
roundings are equal or adjacent.  Gate: |delta| <= max(spacing(|host| as fp32), 1e-13), element-wise."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import solvers as osolv
from oracle.detweights import det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SDC_EINVAL = -1


def _ref(u0, f, visc, T):
    return torch.from_numpy(osolv.burgers_rollout_np(u0, f, visc=visc, T=T, dt=1e-4, guards=False))


def _wave(u0, f, visc, T, **kw):
    from safediffcon_amd import burgers_datagen as bd
    return bd.burgers_numeric_solve_free_wave(u0.to(DEV), f.to(DEV), visc=visc, T=T, dt=1e-4, num_t=f.shape[1], **kw).cpu()


def _inputs(N, s, Nt, scale=0.3):
    return det_tensor((N, s), 700 + s, scale), det_tensor((N, Nt, s), 701 + s + Nt, scale)


# (s, N, Nt, visc, T); visc dt / dx^2 <= 0.03 throughout: the explicit diffusion step is stable
LANE_MAP = [
    (1, 3, 5, 0.01, 0.05),        # K = 1, a single live lane
    (63, 2, 3, 0.01, 0.03),
    (64, 4, 1, 0.01, 0.07),       # K = 1 full: lane 63's right ghost; one interval
    (65, 5, 10, 0.01, 0.09),      # K = 2, a dead cell inside lane 32; 900 steps; N = 5 leaves three waves of the second block idle
    (127, 2, 4, 0.01, 0.1),
    (128, 3, 10, 0.01, 0.1),      # the production K = 2, full wave
    (129, 2, 4, 0.01, 0.1),       # K = 4
    (256, 2, 4, 1e-3, 0.1),
    (257, 2, 2, 1e-3, 0.1),       # K = 8
    (511, 2, 4, 1e-3, 0.1),
    (512, 3, 4, 1e-3, 0.1),       # K = 8 full
]


@pytest.mark.parametrize("s,N,Nt,visc,T", LANE_MAP)
def test_lane_map_bit_exact(s, N, Nt, visc, T):
    u0, f = _inputs(N, s, Nt)
    want = _ref(u0, f, visc, T)
    assert torch.isfinite(want).all() and torch.count_nonzero(want[:, -1]) > 0
    got = _wave(u0, f, visc, T)
    assert got.shape == (N, Nt + 1, s) and got.dtype == torch.float32
    assert torch.equal(got, want)


def test_old_kernel_and_new_kernel_agree_and_waves_per_block_changes_nothing():
    from safediffcon_amd import solvers
    u0, f = _inputs(7, 128, 5)
    old = solvers.burgers_numeric_solve_free(u0.to(DEV), f.to(DEV), visc=0.01, T=0.05, dt=1e-4, num_t=5).cpu()
    assert torch.equal(old, _ref(u0, f, 0.01, 0.05))
    for wpb in (0, 1, 2, 3, 4, 8, 16):
        assert torch.equal(_wave(u0, f, 0.01, 0.05, waves_per_block=wpb), old), wpb


def test_past_512_cells_the_wrapper_falls_back_and_the_c_entry_refuses():
    from safediffcon_amd import _lib
    s = 513
    u0, f = _inputs(2, s, 2)
    want = _ref(u0, f, 1e-3, 0.02)
    assert torch.isfinite(want).all()
    assert torch.equal(_wave(u0, f, 1e-3, 0.02), want)
    traj = torch.full((2, 3, s), float("nan"), device=DEV)
    c = ctypes.c_float
    rc = _lib.get_lib().sdc_burgers_rollout_wave(u0.to(DEV).data_ptr(), f.to(DEV).data_ptr(), traj.data_ptr(), 2, 2, 2, s, 2, 100, 2 * s, s, 0,
                                                 c(1e-4), c(257.), c(264.), c(-528.), c(264.), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == SDC_EINVAL and torch.isnan(traj).all()


def test_large_batch_rows_equal_their_single_runs():
    """1030 waves: 258 blocks of four, the last one half empty; a row depends on nothing but its own u0 and f"""
    u0, f = _inputs(1030, 128, 2)
    got = _wave(u0, f, 0.01, 0.01)
    rows = [0, 255, 256, 1023, 1029]
    want = _ref(u0[rows], f[rows], 0.01, 0.01)
    for i, n in enumerate(rows):
        assert torch.equal(got[n], want[i]), n
        assert torch.equal(_wave(u0[n:n + 1], f[n:n + 1], 0.01, 0.01)[0], got[n]), n


def test_cross_and_const_modes_index_inside_the_kernel():
    from safediffcon_amd import burgers_datagen as bd
    u0 = det_tensor((2, 128), 710, 0.3)
    f = det_tensor((3, 5, 128), 711, 0.3)
    got = bd.burgers_numeric_solve(u0.to(DEV), f.to(DEV), 0.01, 0.05, dt=1e-4, num_t=5).cpu()
    assert got.shape == (2, 3, 6, 128)
    pairs_u, pairs_f = u0.repeat_interleave(3, dim=0), f.repeat(2, 1, 1)
    assert torch.equal(got.reshape(6, 6, 128), _wave(pairs_u, pairs_f, 0.01, 0.05))
    assert torch.equal(got.reshape(6, 6, 128), _ref(pairs_u, pairs_f, 0.01, 0.05))
    # const: one row per force for every interval
    fc = f[:, 0]
    got = bd.burgers_numeric_solve(u0.to(DEV), fc.to(DEV), 0.01, 0.05, dt=1e-4, num_t=5, mode="const").cpu()
    rep = fc.unsqueeze(1).repeat(1, 5, 1)
    assert torch.equal(got.reshape(6, 6, 128), _ref(pairs_u, rep.repeat(2, 1, 1), 0.01, 0.05))
    # s > 512 expands the pairs for the LDS kernel
    u0, f = det_tensor((2, 513), 712, 0.3), det_tensor((3, 2, 513), 713, 0.3)
    got = bd.burgers_numeric_solve(u0.to(DEV), f.to(DEV), 1e-3, 0.02, dt=1e-4, num_t=2).cpu()
    assert torch.equal(got.reshape(6, 3, 513), _ref(u0.repeat_interleave(3, dim=0), f.repeat(2, 1, 1), 1e-3, 0.02))


def test_reference_exceptions_before_any_launch():
    from safediffcon_amd import burgers_datagen as bd
    u0, f = det_tensor((2, 37), 720, 0.3).to(DEV), det_tensor((3, 3, 37), 721, 0.3).to(DEV)
    for solve, ff in ((bd.burgers_numeric_solve, f), (bd.burgers_numeric_solve_free_wave, f[:2])):
        with pytest.raises(AssertionError):
            solve(u0, ff, 0.01, 0.03, num_t=10)
        with pytest.raises(IndexError):                      # 1000 % 3 != 0
            solve(u0, ff, 0.01, 0.1, num_t=3)
        with pytest.raises(ZeroDivisionError):               # 2 steps, 3 intervals
            solve(u0, ff, 0.01, 2e-4, num_t=3)
    with pytest.raises(AssertionError):
        bd.burgers_numeric_solve_free_wave(u0, f, 0.01, 0.03, num_t=3)      # Nu0 != Nf


def test_views_fp64_and_side_stream():
    from safediffcon_amd import burgers_datagen as bd
    diffused = det_tensor((3, 3, 16, 128), 730, 0.3)
    want = _ref(diffused[:, 0, 0, :], diffused[:, 1, :10, :], 0.01, 0.1)
    for src in (diffused.to(DEV), diffused.double().to(DEV)):
        keep = src.clone()
        u0, f = src[:, 0, 0, :], src[:, 1, :10, :]
        assert not f.is_contiguous()
        got = bd.burgers_numeric_solve_free_wave(u0, f, visc=0.01, T=0.1, dt=1e-4, num_t=10)
        assert got.dtype == torch.float32 and torch.equal(got.cpu(), want)
        assert torch.equal(src, keep)
    src = diffused.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = bd.burgers_numeric_solve_free_wave(src[:, 0, 0, :], src[:, 1, :10, :], visc=0.01, T=0.1, dt=1e-4, num_t=10)
    side.synchronize()
    assert torch.equal(got.cpu(), want)


def test_subnormal_products_are_not_flushed():
    u0, f = _inputs(2, 128, 5, scale=0.3e-20)
    sq = (u0 * u0).abs()
    assert ((sq > 0) & (sq < torch.finfo(torch.float32).tiny)).any()
    want = _ref(u0, f, 0.01, 0.05)
    assert torch.isfinite(want).all() and torch.count_nonzero(want[:, -1]) > 0
    assert torch.equal(_wave(u0, f, 0.01, 0.05), want)


def test_non_finite_samples_stay_in_their_rows():
    u0, f = _inputs(5, 128, 5)
    f[2, 1, 40] = float("nan")
    u0[3, 77] = float("inf")
    want = _ref(u0, f, 0.01, 0.05).numpy()
    assert np.isfinite(want[[0, 1, 4]]).all() and np.isfinite(want[2, :2]).all() and np.isnan(want[2, 2:]).any()
    assert not np.isfinite(want[3, 1:]).all()
    got = _wave(u0, f, 0.01, 0.05)
    assert np.array_equal(got.numpy(), want, equal_nan=True)
    # a NaN next to the ghosts of a ragged wave: the cells past s stay +0.0f and feed nothing back
    u0, f = _inputs(2, 65, 2)
    u0[1, 64] = float("nan")
    want = _ref(u0, f, 0.01, 0.02).numpy()
    assert np.array_equal(_wave(u0, f, 0.01, 0.02).numpy(), want, equal_nan=True) and np.isfinite(want[0]).all()


# ------------------------------------------------------------------------------------------------ fixtures of the real generator
@pytest.mark.parametrize("case", ["free", "partial", "uniform", "const"])
def test_reference_fixture_trajectories(golden, case):
    """full T = 1 (10 000 steps) from the fixture's own u0 and f, through the drop-in the reference script would call"""
    from safediffcon_amd import burgers_datagen as bd
    g = golden("burgers_datagen_" + case)
    u0, f = g["u0"].to(DEV), g["f"].to(DEV)              # float64 u0 (and float64 f for make_data): rounded as FloatTensor(...) does
    if case in ("free", "partial"):
        got = bd.burgers_numeric_solve_free_wave(u0, f, visc=0.01, T=1.0, dt=1e-4, num_t=10)
    else:
        got = bd.burgers_numeric_solve(u0, f, visc=0.01, T=1.0, dt=1e-4, num_t=10, mode="const" if case == "const" else None)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), g["traj"])


# ------------------------------------------------------------------------------------------------ synthesis
def _gate(dev, host, what):
    dev, host = np.asarray(dev, np.float64), np.asarray(host, np.float64)
    assert dev.shape == host.shape
    tol = np.maximum(np.spacing(np.abs(host).astype(np.float32)).astype(np.float64), 1e-13)
    delta = np.abs(dev - host)
    print(f"{what}: {np.count_nonzero(delta) / delta.size:.3%} of {delta.size} elements differ, max |delta| / gate = {(delta / tol).max():.3g}")
    assert (delta <= tol).all()


@pytest.mark.parametrize("case", ["free", "partial"])
def test_device_synthesis_within_one_rounding_of_the_host(golden, case):
    from safediffcon_amd import burgers_datagen as bd
    g = golden("burgers_datagen_" + case)
    kw = dict(partial_control=str(g["partial_control"]), alpha=g.scalar("alpha")) if case == "partial" else {}
    N, seed = g.scalar("Nu0"), g.scalar("seed")
    u0, f = bd.make_data_varying_f(N, N, 128, 10, rs=np.random.RandomState(seed), force="device", device=DEV, **kw)
    assert u0.dtype == f.dtype == torch.float32 and u0.is_cuda and f.shape == (N, 10, 128)
    f = f.cpu().numpy()
    _gate(u0.cpu().numpy(), g["u0"].numpy().astype(np.float32), case + " u0")      # the reference's u0 goes through FloatTensor(...)
    _gate(f, g["f"].numpy(), case + " f")
    if case == "partial":
        assert np.count_nonzero(f[:, :, 32:96]) == 0 and not np.signbit(f[:, :, 32:96]).any()
        assert np.abs(f).max() <= 10 and np.abs(f).max() > 8


def test_device_synthesis_const_form_and_clamp(golden):
    from safediffcon_amd import burgers_datagen as bd
    g = golden("burgers_datagen_const")
    u0, f = bd.make_data(2, 3, 128, rs=np.random.RandomState(g.scalar("seed")), force="device", device=DEV)
    assert f.shape == (3, 128) and f.dtype == torch.float32
    _gate(u0.cpu().numpy(), g["u0"].numpy().astype(np.float32), "const u0")
    _gate(f.cpu().numpy(), g["f"].numpy().astype(np.float32), "const f")
    # alpha = 8 drives the clamp: device and host saturate at the same elements
    host = bd.make_data_varying_f(3, 3, 65, 4, alpha=8., rs=np.random.RandomState(4), force="host")[1].numpy()
    dev = bd.make_data_varying_f(3, 3, 65, 4, alpha=8., rs=np.random.RandomState(4), force="device", device=DEV)[1].cpu().numpy()
    assert (np.abs(host) == 10).any() and np.abs(dev).max() == 10
    tol = np.maximum(8 * np.spacing(np.abs(host / 8).astype(np.float32)), 1e-13)       # one rounding before the fp32 multiply by 8
    assert (np.abs(dev.astype(np.float64) - host) <= tol).all()


# ------------------------------------------------------------------------------------------------ generator
def test_generator_host_force_equals_the_reference_dataset(golden):
    from safediffcon_amd import burgers_datagen as bd
    g = golden("burgers_datagen_free")
    out = bd.BurgersDataGenerator(device=DEV).generate(4, 2, seed=0, force="host")
    order = g["shuffle"].tolist()
    for split, idx in (("train", order[:4]), ("test", order[-2:])):
        u, f = out[split]["pde_11-128"], out[split]["pde_11-128_f"]
        assert u.dtype == f.dtype == torch.float64 and u.is_cuda
        assert torch.equal(u.cpu(), g["traj"][idx].double()) and torch.equal(f.cpu(), g["f"][idx].double())


def test_generator_device_force_is_closed_and_chunk_independent():
    """no tolerance: the forces the generator returns, rolled out by the oracle, give the trajectories it returns"""
    from safediffcon_amd import burgers_datagen as bd
    gen = bd.BurgersDataGenerator(device=DEV, nt=6, nx=65, save_nt=6, end_time=0.05)
    a = gen.generate(5, 2, seed=7, force="device", chunk=3)
    b = gen.generate(5, 2, seed=7, force="device", chunk=8192)
    for split in ("train", "test"):
        u, f = a[split]["pde_6-65"], a[split]["pde_6-65_f"]
        assert torch.equal(u, b[split]["pde_6-65"]) and torch.equal(f, b[split]["pde_6-65_f"])
        want = _ref(u[:, 0].cpu().float(), f.cpu().float(), 0.01, 0.05)
        assert torch.equal(u.cpu(), want.double())
        assert torch.count_nonzero(u[:, -1]) > 0
    # uniform mode: every u0 against every f, rows ordered u0-major, the forces repeated per u0
    gen = bd.BurgersDataGenerator(device=DEV, nt=6, nx=65, save_nt=4, end_time=0.05, uniform=True, num_u0=2, num_f=3)
    c = gen.generate(4, 2, seed=7, force="device", chunk=3)
    d = gen.generate(4, 2, seed=7, force="device")
    for split in ("train", "test"):
        assert all(torch.equal(c[split][k], d[split][k]) for k in ("pde_4-65", "pde_4-65_f"))
        assert c[split]["pde_4-65"].shape[1:] == (4, 65) and c[split]["pde_4-65_f"].shape[1:] == (3, 65)
    u0, f = bd.make_data_varying_f(2, 3, 65, 5, rs=np.random.RandomState(7), force="device", device=DEV)
    full = _ref(u0.cpu().repeat_interleave(3, dim=0), f.cpu().repeat(2, 1, 1), 0.01, 0.05)
    order = bd.shuffled_indices(6, 7)
    assert torch.equal(c["train"]["pde_4-65"].cpu(), full[order[:4]][:, -4:].double())
    assert torch.equal(c["test"]["pde_4-65_f"].cpu(), f.cpu().repeat(2, 1, 1)[order[-2:]][:, -3:].double())


def test_generator_uniform_const_force_on_the_host_path():
    """--uniform_u_f True --varying_f False: make_data's fields (host synthesis), one force row for all intervals, u0-major rows"""
    from safediffcon_amd import burgers_datagen as bd
    gen = bd.BurgersDataGenerator(device=DEV, nt=6, nx=65, save_nt=6, end_time=0.05, uniform=True, varying_f=False, num_u0=2, num_f=3)
    out = gen.generate(4, 2, seed=7, force="host", chunk=3)
    u0, f = bd.make_data(2, 3, 65, rs=np.random.RandomState(7), force="host")
    u0, f = torch.from_numpy(u0).float(), torch.from_numpy(f).float()
    forces = f.unsqueeze(1).repeat(2, 5, 1)
    full = _ref(u0.repeat_interleave(3, dim=0), forces, 0.01, 0.05)
    order = bd.shuffled_indices(6, 7)
    for split, idx in (("train", order[:4]), ("test", order[-2:])):
        assert torch.equal(out[split]["pde_6-65"].cpu(), full[idx].double())
        assert torch.equal(out[split]["pde_6-65_f"].cpu(), forces[idx].double())
