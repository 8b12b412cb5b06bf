#!/usr/bin/env python3
"""Generate tests/golden/burgers_datagen_*.npz by running the REAL reference data generator (1D/data/generate_burgers.py) on
the CPU with seeded `np.random` / `random` streams.  The fixtures are data only: the seed, the sizes, the fields the reference
built, the trajectories it solved and its shuffle.

    python tools/make_burgers_datagen_fixture.py --reference <checkout>/1D/data [case ...]      # about 2 s per case

The reference module imports h5py and IPython at its top and uses neither in the functions called here; where they are not
installed, empty stand-in modules are placed in sys.modules first.  Nothing of the reference is copied.

Cases (s = 128, t = 10, visc = 0.01, T = 1, dt = 1e-4 throughout):
  free     seed 0, make_data_varying_f(6, 6) -> burgers_numeric_solve_free; the shuffle of 6 with random.seed(0), 4 train + 2 test
  partial  seed 2, make_data_varying_f(4, 4, partial_control='front_rear_quarter', alpha=1.5) -> burgers_numeric_solve_free
  uniform  seed 3, make_data_varying_f(2, 3) -> burgers_numeric_solve (every u0 against every f)
  const    seed 1, make_data(2, 3) -> burgers_numeric_solve(mode='const')
Stored: u0 in float64 as the reference returns it, f in the dtype it returns (float32; float64 for make_data), traj float32.
"""
import argparse
import importlib
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.environ.get("SDC_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")

S, NT = 128, 10
SOLVE = dict(visc=0.01, T=1.0, dt=1e-4, num_t=NT)
CASES = {
    "free": dict(seed=0, Nu0=6, Nf=6, num_train=4, num_test=2),
    "partial": dict(seed=2, Nu0=4, Nf=4, partial_control="front_rear_quarter", alpha=1.5),
    "uniform": dict(seed=3, Nu0=2, Nf=3),
    "const": dict(seed=1, Nu0=2, Nf=3),
}


def _import_reference(path):
    for name in ("h5py", "IPython"):
        try:
            importlib.import_module(name)
        except ImportError:
            mod = types.ModuleType(name)
            mod.embed = None
            sys.modules[name] = mod
    sys.path.append(path)
    return importlib.import_module("generate_burgers")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SDC_REFERENCE_1D_DATA"), help="the reference's 1D/data directory")
    ap.add_argument("cases", nargs="*")
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference (or SDC_REFERENCE_1D_DATA) is needed")
    g = _import_reference(args.reference)
    os.makedirs(OUT, exist_ok=True)
    for name, c in CASES.items():
        if args.cases and name not in args.cases:
            continue
        np.random.seed(c["seed"])
        random.seed(c["seed"])
        extra = {}
        if name == "const":
            u0, f = g.make_data(c["Nu0"], c["Nf"], S)
            traj = g.burgers_numeric_solve(torch.FloatTensor(u0), torch.FloatTensor(f), mode="const", **SOLVE)
        else:
            kw = {k: c[k] for k in ("partial_control", "alpha") if k in c}
            u0, f = g.make_data_varying_f(c["Nu0"], c["Nf"], S, NT, **kw)
            solve = g.burgers_numeric_solve if name == "uniform" else g.burgers_numeric_solve_free
            traj = solve(torch.FloatTensor(u0), torch.FloatTensor(f), **SOLVE)
            extra = {k: np.asarray(v) for k, v in kw.items()}
        if "num_train" in c:
            n = traj.shape[0]
            extra["shuffle"] = np.array(random.sample(range(n), n), np.int64)
            extra["num_train"], extra["num_test"] = np.int64(c["num_train"]), np.int64(c["num_test"])
        traj = traj.numpy()
        assert np.isfinite(traj).all() and traj.dtype == np.float32
        path = os.path.join(OUT, f"burgers_datagen_{name}.npz")
        np.savez_compressed(path, seed=np.int64(c["seed"]), Nu0=np.int64(c["Nu0"]), Nf=np.int64(c["Nf"]), s=np.int64(S), t=np.int64(NT),
                            u0=np.asarray(u0), f=np.asarray(f), traj=traj, **extra)
        print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)  max|f| = {np.abs(np.asarray(f)).max():.4g}", flush=True)


if __name__ == "__main__":
    main()
