#!/usr/bin/env python3
"""Generate tests/golden/smoke_datagen_*.npz by running the REAL reference data generator
(2d/dataset/apps/a_gen_dataset_128.py with its vendored PhiFlow 1.x) on seeded `np.random` streams.  The fixtures are
data only: parameters, seed, the scene values, the arrays the reference recorded and its acceptance decision.  The noise
is not stored; tests regenerate it from the seed in the reference's draw order.

    python tools/make_smoke_datagen_fixture.py --reference <checkout>/2d/dataset/apps [case ...]      # all cases: ~7 min

The reference module is imported through oracle/phi_compat.py (unchanged): `install()` handles `phi.*` and
`evaluate_solver`; `a_gen_dataset_128` itself loads through the ordinary path finder once its directory is on sys.path.

Cases (one pass straight after get_per_vel unless stated; seeds are the issue's -- the reference met every stated
condition at them, so no seed had to be moved on):
  short_rs4_a  T 32 / 8 frames / 64 cells, safe masks, seed 13    turn frames 2-4 skip book-keeping; two areas take smoke
  short_rs4_b  same shapes, safe masks, seed 3                     the hazard area takes most of the smoke
  short_rs1    T 16 / 16 frames / 128 cells, safe masks, seed 3   rs = 1, ss = 1: record-then-book, 127-in-128 density frame
  full_acc     T 256 / 32 / 64, normal masks, seed 2              the production shape; accepted with and without filter
  full_rej     T 256 / 32 / 64, normal masks, seed 3              rejected (density total too small)
  pair_acc     T 32 / 8 / 64, seed 18, both passes in main's order: pass 1 (normal masks) accepted, pass 2 (safe masks)
               on the continuing stream
  pair_rej     T 32 / 8 / 64, seed 0, pass 1 only: rejected, so main runs no pass 2
  scenes       seeds 0 .. 31 at T = 256 (rs 8) and T = 32 (rs 4): xs, ys, vxs, vys, intervals only

What is stored.  The smoke records (n, nb + 1) always whole, in float64.  Fields (density, set-zero density, velocity,
control) only at the recorded frames listed in `frames64` (float64) and, for the full-length cases, every fourth recorded
frame in float32 (`frames32`); the control's interior is exactly zero in the reference, the density fields are mostly
zero, so the files compress well below the 1 MiB a committed file may have.  A closed loop carries every earlier ring
value into every later velocity, so a late frame in float64 pins all the frames before it.
`accepted` / `accepted_filter` are what loop_write decided with filter off / on (a second run of the same pass; the two
runs' records are asserted equal).
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.environ.get("SDC_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

SHIPPED = dict(min_scale=2, max_scale=5, y_scale=5, initial_vy=0.2, min_sum_rate=0.85, max_sum_rate=1.15)

CASES = {
    "short_rs4_a": dict(T=32, time_length=8, space_length=64, masks="safe", seed=13, frames64=tuple(range(9))),
    "short_rs4_b": dict(T=32, time_length=8, space_length=64, masks="safe", seed=3, frames64=tuple(range(9))),
    "short_rs1": dict(T=16, time_length=16, space_length=128, masks="safe", seed=3, frames64=None),   # second turn frame + last, below
    "full_acc": dict(T=256, time_length=32, space_length=64, masks="normal", seed=2, frames64=(1, 16, 32), frames32=tuple(range(0, 33, 4))),
    "full_rej": dict(T=256, time_length=32, space_length=64, masks="normal", seed=3, frames64=(1, 16, 32), frames32=tuple(range(0, 33, 4))),
    "pair_acc": dict(T=32, time_length=8, space_length=64, masks="pair", seed=18, frames64=tuple(range(9))),
    "pair_rej": dict(T=32, time_length=8, space_length=64, masks="pair", seed=0, frames64=tuple(range(9))),
}

PASS1_FRAMES = (4, 8)          # pair_*: pass 1's fields at two frames only (main keeps nothing but its smoke record)


def _set_masks(g, kind):
    g.cal_smoke_list, g.cal_smoke_concat, g.set_zero_matrix = g.get_bucket_mask() if kind == "normal" else g.get_bucket_mask_safe()
    return len(g.cal_smoke_list)


def _scene(g, c):
    """main()'s draws up to the first loop_write, on the global stream seeded by the caller"""
    rs = int(c["T"] / c["time_length"])
    g.scenelength, g.dt = c["T"], 1
    xs, ys = g.exp2_target_128()
    vxs, vys, intervals = g.get_per_vel(y_scale=SHIPPED["y_scale"], min_scale=SHIPPED["min_scale"], max_scale=SHIPPED["max_scale"],
                                        xs=xs, ys=ys, record_scale=rs)
    return xs, ys, vxs, vys, intervals


def _pass(g, sim, c, scene, kind, filt):
    """get_initial_state + loop_write as main() calls them -> the write arrays (mutated in place) and the decision"""
    xs, ys, vxs, vys, intervals = scene
    rs, ss = int(c["T"] / c["time_length"]), int(128 / c["space_length"])
    nb = _set_masks(g, kind)
    n, L = c["time_length"] + 1, int(128 / ss)
    dw, dzw = np.zeros((L, L, 1, n)), np.zeros((L, L, 1, n))
    vw, cw = np.zeros((L, L, 2, n)), np.zeros((L, L, 2, n))
    sm = np.zeros((n, nb + 1))
    dens, vel, dw, dzw, vw, cw = g.get_initial_state(xs=xs, ys=ys, sim=sim, vxs=vxs, vys=vys, density_write=dw,
                                                    density_set_zero_write=dzw, velocity_write=vw, control_write=cw,
                                                    record_scale=rs, space_scale=ss, initial_vy=SHIPPED["initial_vy"])
    flag = g.loop_write(sim=sim, loop_advected_density=dens, loop_velocity=vel, smoke_outs_128=sm, save_sim_path=None, vxs=vxs,
                        vys=vys, intervals=intervals, xs=xs, ys=ys, density_write=dw, density_set_zero_write=dzw,
                        velocity_write=vw, control_write=cw, record_scale=rs, space_scale=ss, filter=filt,
                        min_sum_rate=SHIPPED["min_sum_rate"], max_sum_rate=SHIPPED["max_sum_rate"])
    return dict(density=dw, density_zero=dzw, velocity=vw, control=cw, smoke=sm), (flag is not False)


def _fields(rec, frames, dtype):
    return {k: np.ascontiguousarray(np.moveaxis(rec[k][..., list(frames)], -1, 0)).astype(dtype)
            for k in ("density", "density_zero", "velocity", "control")}


def _one_pass_twice(g, sim, c, kind, seed):
    """the same pass with filter off and on: same stream, same records, the two decisions"""
    out = []
    for filt in (False, True):
        np.random.seed(seed)
        scene = _scene(g, c)
        rec, ok = _pass(g, sim, c, scene, kind, filt)
        out.append((scene, rec, ok))
    (scene, rec, ok), (_, rec2, ok_f) = out
    assert all(np.array_equal(rec[k], rec2[k]) for k in rec)
    return scene, rec, ok, ok_f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SDC_REFERENCE_APPS"), help="the reference's 2d/dataset/apps directory")
    ap.add_argument("cases", nargs="*")
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference (or SDC_REFERENCE_APPS) is needed")
    from oracle import phi_compat
    phi_compat.install(args.reference)
    sys.path.append(args.reference)
    import matplotlib
    matplotlib.use("Agg")
    import a_gen_dataset_128 as g                      # the reference module

    os.makedirs(OUT, exist_ok=True)
    which = args.cases

    def save(name, **arrs):
        path = os.path.join(OUT, f"smoke_datagen_{name}.npz")
        np.savez_compressed(path, **arrs)
        print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)", flush=True)

    if not which or "scenes" in which:
        arrs = {}
        for T, tl in ((256, 32), (32, 8)):
            c = dict(T=T, time_length=tl)
            rows = []
            for seed in range(32):
                np.random.seed(seed)
                rows.append(_scene(g, c))
            for k, name in enumerate(("xs", "ys", "vxs", "vys", "intervals")):
                arrs[f"T{T}_{name}"] = np.array([r[k] for r in rows])
            arrs[f"T{T}_time_length"] = np.int64(tl)
        save("scenes", seeds=np.arange(32), **{k: np.float64(v) for k, v in SHIPPED.items()}, **arrs)

    sim = g.initialize_field_128()
    for name, c in CASES.items():
        if which and name not in which:
            continue
        common = dict(T=np.int64(c["T"]), time_length=np.int64(c["time_length"]), space_length=np.int64(c["space_length"]),
                      seed=np.int64(c["seed"]), **{k: np.float64(v) for k, v in SHIPPED.items()})
        if c["masks"] == "pair":
            # main()'s order: scene, pass 1 with the normal masks, then -- if accepted -- pass 2 with the safe masks on the
            # continuing stream.  filter does not touch the stream: pass 1 runs with it off and on, pass 2 follows the run without
            scene, rec1, ok, ok_f = _one_pass_twice(g, sim, c, "normal", c["seed"])
            np.random.seed(c["seed"])
            scene = _scene(g, c)
            rec1b, ok_b = _pass(g, sim, c, scene, "normal", False)
            assert ok_b == ok and np.array_equal(rec1b["smoke"], rec1["smoke"])
            arrs = dict(common, masks="pair", xs=scene[0], ys=scene[1], vxs=scene[2], vys=scene[3], intervals=scene[4],
                        smoke=rec1["smoke"], accepted=np.bool_(ok), accepted_filter=np.bool_(ok_f), frames64=np.array(c["frames64"]))
            arrs["pass1_frames64"] = np.array(PASS1_FRAMES)
            arrs.update({f"pass1_{k}": v for k, v in _fields(rec1, PASS1_FRAMES, np.float64).items()})
            if ok:
                rec2, ok2 = _pass(g, sim, c, scene, "safe", False)
                assert ok2
                arrs["smoke_safe"] = rec2["smoke"]
                arrs.update(_fields(rec2, c["frames64"], np.float64))
            print(name, "pass 1 last row", rec1["smoke"][-1], "accepted", ok, ok_f, flush=True)
            save(name, **arrs)
            continue
        scene, rec, ok, ok_f = _one_pass_twice(g, sim, c, c["masks"], c["seed"])
        frames64 = c["frames64"]
        if frames64 is None:
            iv = scene[4]
            frames64 = (iv[0], c["T"])                 # a record-then-book turn frame and the last one: 128 x 128 frames are large
        arrs = dict(common, masks=c["masks"], xs=scene[0], ys=scene[1], vxs=scene[2], vys=scene[3], intervals=scene[4],
                    smoke=rec["smoke"], accepted=np.bool_(ok), accepted_filter=np.bool_(ok_f), frames64=np.array(frames64))
        arrs.update(_fields(rec, frames64, np.float64))
        if "frames32" in c:
            arrs["frames32"] = np.array(c["frames32"])
            arrs.update({f"{k}_f32": v for k, v in _fields(rec, c["frames32"], np.float32).items()})
        print(name, "last row", rec["smoke"][-1], "accepted", ok, ok_f, flush=True)
        save(name, **arrs)


if __name__ == "__main__":
    main()
