"""Closed-loop KSTAR rollouts on the GPU: sdc_kstar_closed_loop / KSTARModel.closed_loop / KSTARDataGenerator on the reference's
real surrogate weights and its real controller (tests/golden/kstar_weights.npz, kstar_rl_policy.npz).

What carries the parity (the surrogate itself stays UNPINNED):
  G1  the loop is the open-loop simulator under feedback: its quantised actuator values replayed through sdc_kstar_rollout give
      its rows bit for bit;
  G2  the policy is the reference's arithmetic: oracle.kstar.rl_policy on the observations rebuilt from the device's own records
      gives the device's raw actions to 1e-12 of the actuator range (fp64 on both sides, only the summation order differs).
A direct comparison of rows with oracle.kstar.closed_loop is printed, not gated (G4): the loop amplifies last-bit differences of
the fp32 networks through the 1e-3 quantisation of the actuators; a 1e-6 relative perturbation of the oracle's own weights already
moves its rows by 0.8-2.5 % of a column's magnitude."""
import os

import numpy as np
import pytest
import torch

from oracle import kstar as okstar
from safediffcon_amd import kstar

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
COLS = np.array([2.3, 1.8, 2.2, 1.8, 5.0, 1.9, 0.9, 3.0e5])       # typical magnitude of each output column (tests/test_gpu_kstar.py)
LOW, HIGH = np.array(okstar.LOW_ACTION), np.array(okstar.HIGH_ACTION)
SEEDS = (0, 1, 2, 3, 4, 5)
_CACHE = {}


def _weights():
    if "w" not in _CACHE:
        _CACHE["w"] = kstar.unflatten_weights(dict(np.load(os.path.join(GOLD, "kstar_weights.npz"))))
    return _CACHE["w"]


def _policy():
    if "p" not in _CACHE:
        _CACHE["p"] = kstar.load_rl_policy(os.path.join(GOLD, "kstar_rl_policy.npz"))
    return _CACHE["p"]


def _model(nbox=1):
    if ("m", nbox) not in _CACHE:
        _CACHE["m", nbox] = kstar.KSTARModel(_weights(), DEV, n_model_box=nbox)
    return _CACHE["m", nbox]


def _oracle():
    """oracle.kstar.closed_loop for SEEDS, computed once: (actions, rows, targets) stacked; the targets are what the device is fed"""
    if "oracle" not in _CACHE:
        runs = [okstar.closed_loop(_weights(), dict(np.load(os.path.join(GOLD, "kstar_rl_policy.npz"))), seed=s) for s in SEEDS]
        _CACHE["oracle"] = tuple(np.stack([r[i] for r in runs]) for i in range(3))
        for a in _CACHE["oracle"]:
            a.setflags(write=False)
    return _CACHE["oracle"]


def _device(nbox=1):
    """the device's loop on the oracle's targets for SEEDS, once per ensemble size: numpy (rows, actions, inputs)"""
    if ("dev", nbox) not in _CACHE:
        out = _model(nbox).closed_loop(_oracle()[2], _policy())
        assert all(isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float64 for x in out)
        _CACHE["dev", nbox] = tuple(x.cpu().numpy() for x in out)
    return _CACHE["dev", nbox]


@pytest.mark.parametrize("nbox", [1, 2])
def test_g1_the_loop_is_the_open_loop_simulator_under_feedback(nbox):
    """every actuator range is positive and f2i truncates toward zero, so value + 4e-4 as float32 stays in the loop's 1e-3 cell:
    sdc_kstar_rollout on those actions must retrace the loop's rows exactly -- both entry points run the same device code"""
    rows, actions, inputs = _device(nbox)
    assert rows.shape == (6, 122, 8) and actions.shape == (6, 121, 9) and inputs.shape == (6, 122, 15)
    replay = (inputs[:, 1:, okstar.ACTION_TO_INPUT] + 4e-4).astype(np.float32)
    assert (np.trunc(replay.astype(np.float64) * okstar.SCALE) == np.trunc(np.clip(actions, LOW, HIGH) * okstar.SCALE)).all()      # same cells
    got = _model(nbox).rollout(torch.from_numpy(replay).to(DEV)).cpu().numpy()
    differ = int((got != rows).sum())
    print(f"[measured] n_model_box={nbox}: {differ} of {rows.size} row entries differ between the loop and its open-loop replay")
    assert (got == rows).all()
    if nbox == 2:
        assert not (rows == _device(1)[0]).all()             # the second network takes part


def test_g2_the_policy_is_the_references_arithmetic():
    rows, actions, _ = _device()
    targets = _oracle()[2]
    policy = dict(np.load(os.path.join(GOLD, "kstar_rl_policy.npz")))
    start = list(okstar.LOW_ACTION) + list(okstar.TARGET_INIT)
    worst = 0.0
    for b in range(len(SEEDS)):
        hist = [start] * okstar.LOOKBACK
        for t in range(121):
            want = okstar.rl_policy(policy, np.array(sum(hist, []) + list(targets[b, t])))
            worst = max(worst, float(np.max(np.abs(actions[b, t] - want) / (HIGH - LOW))))
            hist = hist[1:] + [list(actions[b, t]) + list(rows[b, t + 1][[1, 4, 6]])]
    print(f"[measured] raw actions vs oracle.kstar.rl_policy on the device's own observations: {worst:.2e} of the actuator range")
    assert worst < 1e-12
    assert (actions >= LOW - 1e-12).all() and (actions <= HIGH + 1e-12).all()
    assert np.ptp(actions, axis=(0, 1)).min() > 0           # every actuator is driven


def test_g3_the_controller_tracks_its_targets():
    """tests/test_kstar_host.py's behavioural gate on the device: mean |controlled - target| / nominal over the last 10 steps of
    every 30-step window below 3 % in (beta_p, q95, l_i).  Seeds 0, 1, 3, 4 read at most 1.8 % on the CPU oracle (and stay there
    with every weight perturbed by 1e-5 relative); seeds 5-7 read 2.6-2.9 % there, too close to the gate to be asked of another summation order"""
    rows = _device()[0]
    targets = _oracle()[2]
    settled = np.arange(121) % 30 >= 20
    for b, seed in enumerate(SEEDS):
        if seed not in (0, 1, 3, 4):
            continue
        err = np.mean(np.abs(rows[b][1:][:, [1, 4, 6]] - targets[b])[settled] / np.array(okstar.TARGET_INIT), axis=0)
        print(f"[measured] device closed loop seed {seed}: mean tracking error (beta_p, q95, l_i) = {np.round(err * 100, 2)} %")
        assert (err < 0.03).all()


def test_g4_rows_beside_the_oracles_loop_printed_not_gated():
    rows, actions, _ = _device()
    o_actions, o_rows, _ = _oracle()
    rel = np.max(np.abs(rows - o_rows) / COLS, axis=(1, 2))
    first = [int(np.argmax((np.trunc(np.clip(actions[b], LOW, HIGH) * 1000) != np.trunc(np.clip(o_actions[b], LOW, HIGH) * 1000)).any(axis=1)))
             for b in range(len(SEEDS))]
    print(f"[measured] device loop vs oracle.kstar.closed_loop, largest column-relative row difference per seed: {np.round(rel, 5)}; "
          f"first step whose quantised actuators differ (0 = none or the first): {first}")
    assert np.isfinite(rows).all() and np.isfinite(actions).all()


def test_g5_a_trajectory_does_not_depend_on_the_batch_it_rides_in():
    """B <= 256 one trajectory per workgroup, B <= 512 two, beyond four (three in the last workgroup of 515): the same
    trajectories bit for bit alone, in a batch of 300 and in the batch of 515; mirrors test_all_kernel_shapes_and_ragged_batches_agree"""
    model, policy = _model(), _policy()
    targets = kstar.random_targets(range(515))
    big = model.closed_loop(targets, policy)
    low = model.closed_loop(targets[:300], policy)                        # 0, 255, 256 at their own index
    high = model.closed_loop(targets[215:], policy)                       # 256, 511, 512, 514 at index - 215
    assert big[0].shape == (515, 122, 8) and low[0].shape == (300, 122, 8) and high[0].shape == (300, 122, 8)
    for n in (0, 255, 256, 511, 512, 514):
        alone = model.closed_loop(targets[n:n + 1], policy)
        for k, name in enumerate(("rows", "actions", "inputs")):
            assert torch.equal(big[k][n], alone[k][0]), (n, name, "515 vs 1")
            if n < 300:
                assert torch.equal(big[k][n], low[k][n]), (n, name, "515 vs 300")
            if n >= 215:
                assert torch.equal(big[k][n], high[k][n - 215]), (n, name, "515 vs 300")
    assert not torch.equal(big[0][0], big[0][514])
    assert bool(torch.isfinite(big[0]).all())


def test_g6_row_zero_the_inputs_and_the_generators_records(tmp_path):
    rows, actions, inputs = _device()
    open_rows = _model().rollout(torch.from_numpy(np.tile(LOW.astype(np.float32), (2, 121, 1))).to(DEV)).cpu().numpy()
    assert (rows[:, 0] == open_rows[0, 0]).all()                          # the steady-state network's row, every sample
    inputs0 = np.array([okstar.i2f(okstar.f2i(v)) for v in okstar.INPUT_INIT])
    assert (inputs[:, 0] == inputs0).all()
    # control(): the actuators' columns hold i2f(f2i(clip(raw action))), every other column keeps its initial value
    want = np.tile(inputs0, (len(SEEDS), 121, 1))
    want[:, :, okstar.ACTION_TO_INPUT] = np.trunc(np.clip(actions, LOW, HIGH) * okstar.SCALE) / okstar.SCALE
    assert (inputs[:, 1:] == want).all()

    gen = kstar.KSTARDataGenerator(weights=_model(), policy=_policy(), device=DEV)
    recs = gen.generate([0, 1])
    targets = kstar.random_targets([0, 1])
    direct = [x.cpu().numpy() for x in _model().closed_loop(targets, _policy())]
    assert len(recs) == 2
    for n, rec in enumerate(recs):
        assert sorted(rec) == ["actions", "inputs", "outputs", "targets"]
        assert {k: (v.shape, v.dtype) for k, v in rec.items()} == {"inputs": ((122, 15), np.float64), "outputs": ((122, 8), np.float64),
                                                                   "targets": ((122, 3), np.float64), "actions": ((121, 9), np.float64)}
        assert (rec["targets"][0] == rec["targets"][1]).all() and (rec["targets"][1:] == targets[n]).all()      # the first target twice
        assert (rec["outputs"] == direct[0][n]).all() and (rec["actions"] == direct[1][n]).all() and (rec["inputs"] == direct[2][n]).all()
        assert (rec["inputs"][0] == inputs0).all() and (rec["outputs"][0] == open_rows[0, 0]).all()
    one = gen.random_target_simulation(random_seed=1)
    assert all((one[k] == recs[1][k]).all() for k in one)
    path = str(tmp_path / "1.npz")
    kstar.save_record(path, one)
    back = np.load(path, allow_pickle=True)["data"].item()
    assert sorted(back) == sorted(one) and all((back[k] == one[k]).all() and back[k].dtype == np.float64 for k in one)


def test_targets_may_be_float32_or_device_tensors_and_bad_ones_raise_like_the_python():
    model, policy = _model(), _policy()
    t64 = kstar.random_targets([3, 4])
    t32 = t64.astype(np.float32)
    a = model.closed_loop(t32, policy)
    b = model.closed_loop(torch.from_numpy(t32).to(DEV), policy)
    c = model.closed_loop(t32.astype(np.float64), policy)
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))
    short = model.closed_loop(t64[:, :40], policy, n_steps=40)
    full = model.closed_loop(t64, policy)
    assert short[0].shape == (2, 41, 8) and torch.equal(short[0], full[0][:, :41]) and torch.equal(short[1], full[1][:, :40])
    assert model.closed_loop(t64[:0], policy)[0].shape == (0, 122, 8)
    bad = torch.from_numpy(t64).to(DEV)
    bad[1, 100, 0] = float("nan")
    with pytest.raises(ValueError):
        model.closed_loop(bad, policy)
    with pytest.raises(IndexError):
        model.closed_loop(t64[:, :120], policy)
    with pytest.raises(ValueError):
        model.closed_loop(t64, dict(policy, fc0_kernel=policy["fc0_kernel"][:38]))
