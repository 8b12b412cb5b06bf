#!/usr/bin/env python3
"""time the KSTAR rollout (sdc_kstar_rollout) for a batch of control sequences: python tools/kstar_time.py [B ...]

--closed-loop            also time sdc_kstar_closed_loop (the RL controller inside the kernel) on random_targets(range(B))
--rounds N               N timed rounds per arm (default 5); the arms of one B alternate inside a round, median and min are printed
--other-lib PATH         a second build of libsdc_hip.so (a previous commit's, say) loaded beside the first: both builds'
                         sdc_kstar_rollout become arms of every round, called directly on the same device buffers, and their
                         rows are compared bit for bit

SDC_LIB_PATH=<another build> replaces the library the package itself loads (a build without sdc_kstar_closed_loop is fine as long
as --closed-loop is not asked for)."""
import _libsel  # noqa: F401,E402  (SDC_LIB_PATH -> safediffcon_amd._lib.use_library, tools only)
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safediffcon_amd import _lib, kstar  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="*", type=int)
ap.add_argument("--closed-loop", action="store_true")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--other-lib")
args = ap.parse_args()
if not args.closed_loop:
    _lib.SIGNATURES.pop("sdc_kstar_closed_loop", None)       # an older build has no such symbol; nothing here calls it

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
w = kstar.unflatten_weights(dict(np.load(os.path.join(GOLD, "kstar_weights.npz"))))
model = kstar.KSTARModel(w, "cuda:0")
policy = kstar.load_rl_policy(os.path.join(GOLD, "kstar_rl_policy.npz")) if args.closed_loop else None
other = None
if args.other_lib:
    other = C.CDLL(os.path.abspath(args.other_lib)).sdc_kstar_rollout
    other.restype, other.argtypes = _lib.SIGNATURES["sdc_kstar_rollout"]


def entry(fn, a):
    """one library's sdc_kstar_rollout on the model's own descriptor and device buffers, without the wrapper's argument checks"""
    out = torch.empty((a.shape[0], 122, 8), dtype=torch.float64, device=a.device)
    rc = fn(C.byref(model.desc), a.data_ptr(), a.stride(0), a.stride(1), a.stride(2), out.data_ptr(), model._work.data_ptr(), a.shape[0], 121,
            torch.cuda.current_stream(a.device).cuda_stream)
    assert rc == 0, f"sdc_kstar_rollout returned {rc}"
    return out


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


for B in args.B or [128, 512, 2048]:
    lo, hi = torch.tensor(kstar.LOW_ACTION), torch.tensor(kstar.HIGH_ACTION)
    acts = (lo + (hi - lo) * torch.rand(B, 121, 9, generator=torch.Generator().manual_seed(B))).float().cuda()
    arms = {"rollout": lambda: model.rollout(acts)}
    if args.closed_loop:
        targets = torch.from_numpy(kstar.random_targets(range(B))).cuda()
        arms["closed_loop"] = lambda: model.closed_loop(targets, policy)
    if other is not None:
        arms["sdc_kstar_rollout (this lib)"] = lambda: entry(model.lib.sdc_kstar_rollout, acts)
        arms["sdc_kstar_rollout (other lib)"] = lambda: entry(other, acts)
        same = torch.equal(entry(model.lib.sdc_kstar_rollout, acts), entry(other, acts))
        print(f"B={B}: rows of the two libraries' sdc_kstar_rollout are {'bit-identical' if same else 'DIFFERENT'}", flush=True)
    for fn in arms.values():
        fn()                                                 # warm-up
    ms = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    for k, v in ms.items():
        med = statistics.median(v)
        print(f"B={B} {k}: median {med:.2f} ms, min {min(v):.2f} ms over {len(v)} rounds, 122 rows "
              f"({B / med * 1e3:.0f} trajectories/s)", flush=True)
