"""No GPU: the host half of the Burgers data generator (safediffcon_amd/burgers_datagen.py) against fixtures of the real
reference generator (tools/make_burgers_datagen_fixture.py): the draw order and the float64 field synthesis bit for bit, the
shuffle and the split, the attributes and the .npz layout, the reference's assertions, and the argument checks of the two C
entries, which come before any launch and so need no device."""
import ctypes
import random

import numpy as np
import pytest
import torch

from safediffcon_amd import _lib
from safediffcon_amd import burgers_datagen as bd

SDC_EINVAL, SDC_ENULL = -1, -4
CASES = ("free", "partial", "uniform", "const")


def _host_fields(g):
    """draw_parameters + the host synthesis for a fixture's seed and sizes -> u0 float64 array, f as the reference returns it"""
    rs = np.random.RandomState(g.scalar("seed"))
    Nu0, Nf, s, t = (g.scalar(k) for k in ("Nu0", "Nf", "s", "t"))
    if "traj" in g.keys() and g["f"].dim() == 2:
        return bd.make_data(Nu0, Nf, s, rs=rs, force="host")
    kw = {}
    if "partial_control" in g.keys():
        kw = dict(partial_control=str(g["partial_control"]), alpha=g.scalar("alpha"))
    return bd.make_data_varying_f(Nu0, Nf, s, t, rs=rs, force="host", **kw)


@pytest.mark.parametrize("case", CASES)
def test_host_synthesis_equals_the_reference_bit_for_bit(golden, case):
    g = golden("burgers_datagen_" + case)
    u0, f = _host_fields(g)
    assert u0.dtype == np.float64 and np.array_equal(u0, g["u0"].numpy())
    f = np.asarray(f)
    assert f.dtype == g["f"].numpy().dtype and np.array_equal(f, g["f"].numpy())


def test_partial_control_fixture_properties(golden):
    g = golden("burgers_datagen_partial")
    f = g["f"].numpy()
    assert np.count_nonzero(f[:, :, 32:96]) == 0 and np.count_nonzero(f[:, :, :32]) > 0
    assert abs(np.abs(f).max() - 8.45) < 0.01 and np.abs(f).max() <= 10


def test_draw_parameters_layout_and_global_stream():
    """rs=None draws from the global np.random like the reference; term 0 never has the randint gate, the sigmas carry 0.5"""
    np.random.seed(5)
    up_a, fp_a = bd.draw_parameters(None, 3, 4)
    up_b, fp_b = bd.draw_parameters(np.random.RandomState(5), 3, 4)
    assert np.array_equal(up_a, up_b) and np.array_equal(fp_a, fp_b)
    assert up_a.shape == (3, 6) and fp_a.shape == (4, 8, 5)
    up, fp = bd.draw_parameters(np.random.RandomState(1), 50, 200)
    for k, (lo, hi) in enumerate(((.2, .4), (0, 2), (.05, .15), (.6, .8), (-2, 0), (.05, .15))):
        assert (up[:, k] >= lo).all() and (up[:, k] <= hi).all()
    assert np.count_nonzero(fp[:, 0, 0]) == 200 and 40 < np.count_nonzero(fp[:, 1:, 0] == 0) / 7 < 160
    assert (fp[:, :, [2, 4]] >= 0.05).all() and (fp[:, :, [2, 4]] <= 0.2).all()
    # make_data's order differs: loc before amp, no time draws
    _, fp_c = bd.draw_parameters(np.random.RandomState(1), 50, 200, varying=False)
    assert not np.array_equal(fp_c[:, 0, 0], fp[:, 0, 0]) and (fp_c[:, :, 3] == 0).all() and (fp_c[:, :, 4] == 1).all()


def test_shuffle_and_split_equal_the_reference(golden):
    g = golden("burgers_datagen_free")
    order = bd.shuffled_indices(6, 0)
    assert order == g["shuffle"].tolist()
    random.seed(0)
    assert order == random.sample(range(6), 6)
    assert sorted(order) == list(range(6))


def test_generator_assertions_and_value_errors():
    G = bd.BurgersDataGenerator
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G(device="cpu")
    with pytest.raises(ValueError, match="invalid partial control mode"):
        G(partial_control="middle")
    with pytest.raises(ValueError):
        G(nt=11, save_nt=12)
    with pytest.raises(AssertionError, match="Nu0 \\* Nf"):
        G(uniform=True, num_u0=2, num_f=3).generate(4, 1)
    with pytest.raises(AssertionError, match="partial control"):
        G(uniform=True, num_u0=2, num_f=3, partial_control="front_rear_quarter").generate(4, 2)
    with pytest.raises(AssertionError, match="varying_f"):
        G(uniform=False, varying_f=False).generate(4, 2)
    with pytest.raises(ValueError, match="force"):
        G().generate(4, 2, force="numpy")
    with pytest.raises(ValueError, match="not finite"):
        bd.make_data_varying_f(2, 2, 128, 10, tmax=float("nan"), force="host")
    with pytest.raises(ValueError, match="invalid partial control mode"):
        bd.make_data_varying_f(2, 2, 128, 10, partial_control="x", force="host")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bd.burgers_numeric_solve(torch.zeros(2, 8), torch.zeros(3, 10, 8), 0.01, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bd.burgers_numeric_solve_free_wave(torch.zeros(2, 8), torch.zeros(2, 10, 8), 0.01, 1.0)
    with pytest.raises(AssertionError):
        bd.burgers_numeric_solve(torch.zeros(2, 8), torch.zeros(3, 4, 8), 0.01, 1.0)
    with pytest.raises(ValueError):
        bd.burgers_numeric_solve_free_wave(torch.zeros(2, 8), torch.zeros(2, 10, 8), 0.01, 1.0, mode="const")


def test_attributes_and_save_round_trip(tmp_path):
    gen = bd.BurgersDataGenerator(nt=11, nx=128, save_nt=8, end_time=1.)
    assert gen.key == "pde_8-128"
    a = gen.attributes()
    assert a["dt"] == 1. / 10 and a["dx"] == 1 / 129 and a["nt"] == 11 and a["nx"] == 128 and a["tmin"] == 0.0 and a["tmax"] == 1.
    assert torch.equal(a["x"], torch.linspace(1 / 129, 1 - 1 / 129, 128)) and a["x"].dtype == torch.float32
    rng = np.random.RandomState(0)
    record = {split: {"pde_8-128": torch.from_numpy(rng.rand(n, 8, 128)), "pde_8-128_f": torch.from_numpy(rng.rand(n, 7, 128)),
                      "attrs": gen.attributes()} for split, n in (("train", 4), ("test", 2))}
    paths = gen.save(str(tmp_path), record)
    assert [p.split("/")[-1] for p in paths] == ["burgers_train.npz", "burgers_test.npz"]
    for path, split in zip(paths, ("train", "test")):
        z = np.load(path, allow_pickle=False)
        assert sorted(z.keys()) == sorted(["pde_8-128", "pde_8-128_f"] + [f"pde_8-128/{k}" for k in a])
        for k in ("pde_8-128", "pde_8-128_f"):
            assert z[k].dtype == np.float64 and np.array_equal(z[k], record[split][k].numpy())
        assert z["pde_8-128/dt"] == 0.1 and z["pde_8-128/nt"] == 11 and z["pde_8-128/dx"] == 1 / 129
        assert np.array_equal(z["pde_8-128/x"], a["x"].numpy())


def test_save_nt_keeps_the_last_rows(monkeypatch):
    """generate with the rollout and the device stubbed out: rows -save_nt.. of u and -(save_nt - 1).. of f, shuffled and split"""
    gen = bd.BurgersDataGenerator(nt=11, nx=16, save_nt=4)
    gen.device = torch.device("cpu")
    seen = {}

    def fake_solve(u0, f):
        seen["f"] = f.clone()
        return torch.arange(11, dtype=torch.float32).reshape(1, 11, 1) + 100 * u0[:, :1].reshape(-1, 1, 1) + torch.zeros(len(u0), 11, 16)
    monkeypatch.setattr(gen, "_solve_free", fake_solve)
    out = gen.generate(4, 2, seed=0, force="host", chunk=6)
    order = bd.shuffled_indices(6, 0)
    rs = np.random.RandomState(0)
    u0, f = bd.make_data_varying_f(6, 6, 16, 10, rs=rs, force="host")
    u0 = torch.from_numpy(u0).float()
    assert torch.equal(seen["f"], f)
    for split, idx in (("train", order[:4]), ("test", order[-2:])):
        u = out[split]["pde_4-16"]
        assert u.dtype == torch.float64 and u.shape == (len(idx), 4, 16)
        want = torch.arange(7, 11, dtype=torch.float32).reshape(1, 4, 1) + 100 * u0[idx, :1].reshape(-1, 1, 1) + torch.zeros(len(idx), 4, 16)
        assert torch.equal(u, want.double())
        assert torch.equal(out[split]["pde_4-16_f"], f[idx][:, -3:].double())
        assert out[split]["attrs"]["nt"] == 11


def _wave(lib, u0=1, f=1, traj=1, N=2, Nu0=2, Nf=2, s=128, Nt=10, rec=1000, f_sn=1280, f_st=128, pair=0, wpb=0):
    c = ctypes.c_float
    return lib.sdc_burgers_rollout_wave(u0, f, traj, N, Nu0, Nf, s, Nt, rec, f_sn, f_st, pair, c(1e-4), c(64.5), c(166.), c(-332.), c(166.),
                                        wpb, None)


def test_c_entries_refuse_bad_arguments_without_a_device():
    """every check precedes the launch: the non-null pointers below (address 1) are never dereferenced"""
    lib = _lib.get_lib()
    for kw in (dict(u0=0), dict(f=0), dict(traj=0)):
        assert _wave(lib, **kw) == SDC_ENULL and "null" in _lib.last_error()
    for kw in (dict(s=513), dict(rec=0), dict(rec=-3), dict(N=0), dict(Nt=0), dict(s=0), dict(pair=2), dict(pair=-1),
               dict(pair=1, N=5, Nu0=2, Nf=3), dict(pair=0, N=6, Nu0=2, Nf=6), dict(pair=0, N=6, Nu0=6, Nf=3), dict(f_sn=-1),
               dict(f_st=-128), dict(wpb=17), dict(wpb=-1)):
        assert _wave(lib, **kw) == SDC_EINVAL, kw
    assert "512" in (_wave(lib, s=513), _lib.last_error())[1]
    with pytest.raises(_lib.SdcError):
        _lib.check(_wave(lib, rec=0), "sdc_burgers_rollout_wave")

    def synth(upar=1, fpar=1, x=1, ts=1, mask=0, u0=1, f=1, Nu0=2, Nf=2, s=128, Nt=10):
        return lib.sdc_burgers_synth(upar, fpar, x, ts, mask, 2.0, ctypes.c_float(1.0), u0, f, Nu0, Nf, s, Nt, None)
    for kw in (dict(x=0), dict(u0=0, f=0), dict(upar=0), dict(fpar=0)):
        assert synth(**kw) == SDC_ENULL, kw
    for kw in (dict(s=0), dict(Nu0=0), dict(Nf=0), dict(Nt=0), dict(ts=0, Nt=10)):
        assert synth(**kw) == SDC_EINVAL, kw
