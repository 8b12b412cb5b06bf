"""Host side of the closed-loop KSTAR rollout (sdc_kstar_closed_loop / safediffcon_amd.kstar): the library's surface, the
controller's loader, the reference's target schedule and the argument checks that come before any launch.  No GPU needed."""
import ctypes as C
import io
import json
import os
import re
import shutil
import subprocess
import zipfile

import numpy as np
import pytest
import torch

import safediffcon_amd
from oracle import kstar as okstar
from safediffcon_amd import _lib, kstar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
POLICY = os.path.join(GOLD, "kstar_rl_policy.npz")


def _fixture():
    return dict(np.load(POLICY))


# ------------------------------------------------------------------------------------------------ library
def test_the_library_exports_the_entry_point_and_the_header_declares_it():
    lib = _lib.get_lib()
    assert hasattr(lib, "sdc_kstar_closed_loop") and "sdc_kstar_closed_loop" in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "sdc.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint\s+sdc_kstar_closed_loop\s*\(", header) and "} SdcKstarPolicy;" in header
    for name in ("KSTARDataGenerator", "load_rl_policy", "random_targets", "save_record"):
        assert getattr(safediffcon_amd, name) is getattr(kstar, name)


def test_the_entry_point_refuses_a_misshapen_policy_before_it_launches():
    """SDC_EINVAL with a message for a wrong observation / action width, more than 4 hidden layers, a width past 256.  The
    pointers are dummies: a call that got as far as reading them, let alone launching, would not return these codes"""
    lib = _lib.get_lib()
    dummy = C.c_void_p(4096)

    def call(nlayers, widths, B=1, nsteps=121):
        p = _lib.SdcKstarPolicy()
        p.nlayers = nlayers
        for i, w in enumerate(widths):
            p.width[i] = w
        p.params = 4096
        return lib.sdc_kstar_closed_loop(C.byref(_lib.SdcKstarModel()), C.byref(p), dummy, dummy, dummy, dummy, dummy, B, nsteps, None)

    for nlayers, widths, word in ((2, [38, 64, 64, 9], "38 -> 9"), (2, [39, 64, 64, 8], "39 -> 8"), (5, [39, 8, 8, 8, 8, 8], "5 hidden"),
                                  (2, [39, 257, 64, 9], "257 wide"), (2, [39, 64, 0, 9], "0 wide"), (-1, [39, 9], "-1 hidden")):
        assert call(nlayers, widths) == -1                   # SDC_EINVAL
        assert "sdc_kstar_closed_loop" in _lib.last_error() and word in _lib.last_error()
    assert call(2, [39, 64, 64, 9], B=0) == -1 and call(2, [39, 64, 64, 9], nsteps=0) == -1
    assert call(2, [39, 64, 64, 9]) == -1 and "LSTM parameters missing" in _lib.last_error()      # a good policy, an empty model
    assert lib.sdc_kstar_closed_loop(C.byref(_lib.SdcKstarModel()), None, dummy, dummy, dummy, dummy, dummy, 1, 121, None) == -4


def test_the_ctypes_struct_has_the_headers_size(tmp_path):
    """sizeof(SdcKstarPolicy) as the host compiler lays the header's struct out == ctypes.sizeof of the mirror in _lib.py"""
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdc.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(SdcKstarPolicy), offsetof(SdcKstarPolicy, params),'
                   ' offsetof(SdcKstarPolicy, low_state), offsetof(SdcKstarPolicy, hist0)); return 0; }\n')
    exe = tmp_path / "size"
    cc = next((shutil.which(c) for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    assert cc is not None, "no C compiler to lay the header's struct out with"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_params, o_low, o_hist = (int(v) for v in subprocess.check_output([str(exe)]).split())
    P = _lib.SdcKstarPolicy
    assert (size, o_params, o_low, o_hist) == (C.sizeof(P), P.params.offset, P.low_state.offset, P.hist0.offset)
    assert size == 4 * 7 + 4 + 8 + 8 * (39 + 39 + 12)               # 7 ints, padding to the pointer, the pointer, 90 doubles


# ------------------------------------------------------------------------------------------------ load_rl_policy
def test_load_rl_policy_reads_the_fixture():
    fix = _fixture()
    for src in (POLICY, fix):
        pol = kstar.load_rl_policy(src)
        assert list(pol["layers"]) == [64, 64]
        assert sorted(pol) == sorted(fix)
        for k in fix:
            if k != "layers":
                assert pol[k].dtype == np.float32 and np.array_equal(pol[k], fix[k])
    assert pol["fc0_kernel"].shape == (39, 64) and pol["dense_kernel"].shape == (64, 9)


def _reference_zip(path, fix, with_layers=True):
    """a zip laid out like the reference's best_model.zip: ``data`` (json) + ``parameters`` (an npz of model/pi/... arrays)"""
    params = {}
    for k, v in fix.items():
        if k == "layers":
            continue
        layer, part = k.rsplit("_", 1)
        params[f"model/pi/{layer}/{part}:0"] = v
    params["model/vf/fc0/kernel:0"] = np.zeros((39, 64), np.float32)          # the critic's arrays are in the file too; not read
    params["model/pi/logstd:0"] = np.zeros((1, 9), np.float32)
    buf = io.BytesIO()
    np.savez(buf, **params)
    with zipfile.ZipFile(path, "w") as zf:
        zf.writestr("data", json.dumps({"policy_kwargs": {"layers": [int(v) for v in fix["layers"]]} if with_layers else {}, "gamma": 0.99}))
        zf.writestr("parameter_list", json.dumps(sorted(params)))
        zf.writestr("parameters", buf.getvalue())


def test_load_rl_policy_reads_the_references_zip_layout(tmp_path):
    fix = _fixture()
    for with_layers in (True, False):                        # the reference's default when policy_kwargs has no "layers": [64, 64]
        path = tmp_path / f"best_model_{with_layers}.zip"
        _reference_zip(path, fix, with_layers)
        pol = kstar.load_rl_policy(str(path))
        assert sorted(pol) == sorted(fix) and list(pol["layers"]) == [64, 64]
        for k in fix:
            assert np.array_equal(pol[k], fix[k])


def test_load_rl_policy_refuses_wrong_widths():
    fix = _fixture()
    bad_obs = dict(fix, fc0_kernel=fix["fc0_kernel"][:38])
    bad_act = dict(fix, dense_kernel=fix["dense_kernel"][:, :8], dense_bias=fix["dense_bias"][:8])
    too_wide = dict(fix, fc0_kernel=np.zeros((39, 257), np.float32), fc0_bias=np.zeros(257, np.float32),
                    fc1_kernel=np.zeros((257, 64), np.float32), layers=np.array([257, 64]))
    too_deep = {f"fc{i}_kernel": np.zeros((39 if i == 0 else 8, 8), np.float32) for i in range(5)}
    too_deep.update({f"fc{i}_bias": np.zeros(8, np.float32) for i in range(5)})
    too_deep.update(dense_kernel=np.zeros((8, 9), np.float32), dense_bias=np.zeros(9, np.float32), layers=np.array([8] * 5))
    for bad in (bad_obs, bad_act, too_wide, too_deep, {k: v for k, v in fix.items() if k != "fc1_bias"}):
        with pytest.raises(ValueError):
            kstar.load_rl_policy(bad)


# ------------------------------------------------------------------------------------------------ random_targets
def test_random_targets_follow_the_references_schedule_and_stream():
    seeds = [0, 1, 7, 12345]
    np.random.seed(99)
    before = np.random.get_state()
    t = kstar.random_targets(seeds)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]      # global state untouched
    assert t.shape == (4, 121, 3) and t.dtype == np.float64
    assert np.array_equal(t, kstar.random_targets(seeds)) and np.array_equal(t[2:3], kstar.random_targets([7]))
    assert not np.array_equal(t[0], t[1])
    lo, hi = np.array(okstar.RAND_TARGET_MINS), np.array(okstar.RAND_TARGET_MAXS)
    assert (t >= lo).all() and (t <= hi).all()
    assert np.array_equal(t, np.round(t * 1000) / 1000)                                     # on the 1e-3 grid
    for n, seed in enumerate(seeds):
        # windows of 31 / 30 / 30 / 30 control steps
        change = np.flatnonzero((t[n, 1:] != t[n, :-1]).any(axis=1)) + 1
        assert list(change) == [31, 61, 91]
        # the reference's stream: np.random.seed(seed) then uniform(low, high) per channel in the order beta_p, q95, l_i
        rs = np.random.RandomState(seed)
        for w in range(4):
            want = [okstar.i2f(okstar.f2i(rs.uniform(a, b))) for a, b in zip(okstar.RAND_TARGET_MINS, okstar.RAND_TARGET_MAXS)]
            assert list(t[n, 0 if w == 0 else 1 + 30 * w]) == want
    assert kstar.random_targets([3], n_steps=40).shape == (1, 40, 3)
    assert np.array_equal(kstar.random_targets([3], n_steps=40)[0], kstar.random_targets([3])[0, :40])


def test_the_modules_constants_are_the_oracles():
    for name in ("LOW_TARGET", "HIGH_TARGET", "TARGET_INIT", "RAND_TARGET_MINS", "RAND_TARGET_MAXS", "LOOKBACK", "LOW_ACTION", "HIGH_ACTION"):
        assert getattr(kstar, name) == getattr(okstar, name)


# ------------------------------------------------------------------------------------------------ refusals before any launch
def _bare_model(device):
    """a KSTARModel without its device buffers: enough for the checks closed_loop makes before it touches the device"""
    m = kstar.KSTARModel.__new__(kstar.KSTARModel)
    m.device = torch.device(device)
    return m


def test_the_cpu_is_refused():
    w = kstar.unflatten_weights(dict(np.load(os.path.join(GOLD, "kstar_weights.npz"))))
    with pytest.raises(RuntimeError):
        kstar.KSTARModel(w, "cpu")
    with pytest.raises(RuntimeError):
        _bare_model("cpu").closed_loop(kstar.random_targets([0]), _fixture())
    with pytest.raises(RuntimeError):
        kstar.KSTARDataGenerator(weights=w, policy=_fixture(), device="cpu")


@pytest.mark.parametrize("device", ["cpu", "cuda"])
def test_targets_are_validated_before_any_launch(device):
    """the bare model has nothing to launch with: reaching the device would raise AttributeError, not these"""
    m = _bare_model(device)
    good = kstar.random_targets([0, 1])
    for bad in (good[:, :120], good[:, :, :2], good[0], np.zeros((2, 122, 3)), good.reshape(2, 121, 3, 1)):
        with pytest.raises(IndexError):
            m.closed_loop(bad, _fixture())
    with pytest.raises(IndexError):
        m.closed_loop(good, _fixture(), n_steps=100)
    for poison in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[1, 77, 2] = poison
        with pytest.raises(ValueError):
            m.closed_loop(bad, _fixture())
        with pytest.raises(ValueError):
            m.closed_loop(torch.from_numpy(bad).float(), _fixture())
    with pytest.raises(TypeError):
        m.closed_loop(np.zeros((2, 121, 3), np.int64), _fixture())


def test_save_record_writes_the_references_file_layout(tmp_path):
    rec = {"inputs": np.arange(122 * 15.).reshape(122, 15), "outputs": np.ones((122, 8)), "targets": np.zeros((122, 3)),
           "actions": np.full((121, 9), 0.5)}
    path = tmp_path / "0.npz"
    kstar.save_record(str(path), rec)
    with np.load(str(path), allow_pickle=True) as z:
        assert z.files == ["data"] and z["data"].shape == () and z["data"].dtype == object
        back = z["data"].item()
    assert sorted(back) == sorted(rec) and all(np.array_equal(back[k], rec[k]) for k in rec)
