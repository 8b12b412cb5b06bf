"""-m gpu: the fused LinearAttention block's bf16-split build (sdc_linattn_block_sel, impl 1; csrc/sdc_lablock_x3.hip) and its fp16 build
(sdc_linattn_block_f16; csrc/sdc_lablock_f16.hip) keep the bits they had before their pass bodies and shared steps moved into
csrc/sdc_lablock_tile.h / sdc_lablock_pass.h.  The fp32 build (impl 0) is pinned the same way by
test_gpu_linattn_x3.py::test_linattn_x3_impl0_has_the_parent_commits_bits; the GroupNorm-on-load forms are held to these, bit for bit, by
the *_with_groupnorm_on_load tests."""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

import test_gpu_linattn_f16 as F16
import test_gpu_linattn_x3 as X3

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_BITS = os.path.join(ROOT, "tests", "golden", "linattn_block_parent_sha256.json")

# the cases of test_gpu_linattn_f16.py, and RMSNorm at width 128: the post norm over two column tiles per wave and four row tiles
SHAPES = F16.SHAPES + [(2, 1, 128, 128, 1, 1, False)]
_ID = lambda s: "x".join(map(str, s[:6])) + ("-ascending" if s[6] else "")      # noqa: E731


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def block_bits():
    """sha256 of the output bytes of both builds on SHAPES (NaN-filled outputs and scratch), from whichever library is loaded"""
    out = {"x3": {}, "f16": {}}
    for shape in SHAPES:
        outer, inner, Cc, n, pre, post, _ = shape
        x, g1, g2, wqkv, wo, bo = F16._inputs(*shape)
        x_dev = x.to(DEV)
        pq, po, wpk = F16._dev_weights(wqkv, wo, Cc)
        d = dict(g1=g1.to(DEV), g2=g2.to(DEV), bo=bo.to(DEV), pq=pq, po=po)
        out["x3"][_ID(shape)] = _sha(X3._run(1, x_dev, d, pre, post))
        out["f16"][_ID(shape)] = _sha(F16._run(x_dev, d["g1"], pq, po, wpk, d["bo"], d["g2"], pre, post))
    return out


_PARENT_CHILD = """
import json, sys
sys.path.insert(0, {root!r})
from safediffcon_amd import _lib
_lib.use_library({lib!r})
sys.path.insert(0, {tests!r})
import test_gpu_linattn_parent_bits as T
print("PARENT_BITS " + json.dumps(T.block_bits()))
"""


def parent_bits(parent_lib):
    """block_bits() of another build of the library (the commit before this change), loaded in a child process through _lib.use_library"""
    src = _PARENT_CHILD.format(root=ROOT, lib=os.path.abspath(parent_lib), tests=os.path.join(ROOT, "tests"))
    res = subprocess.run([sys.executable, "-c", src], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    line = next(ln for ln in res.stdout.splitlines() if ln.startswith("PARENT_BITS "))
    return json.loads(line[len("PARENT_BITS "):])


def test_linattn_block_builds_have_the_parent_commits_bits():
    """impl 1 and the fp16 build == the outputs of the commit before the shared pass bodies, bit for bit: the sha256 of each output on
    SHAPES, recorded from a library built from that commit (tests/golden/linattn_block_parent_sha256.json -- a clean checkout has no
    parent library to build).  With SDC_PARENT_LIB naming such a library a child process runs it again and must reproduce the record.
    A mismatch is a changed contraction or summation order in a shared step, not a tolerance."""
    with open(PARENT_BITS) as fh:
        want = json.load(fh)["sha256"]
    lib_path = os.environ.get("SDC_PARENT_LIB")
    if lib_path:
        assert parent_bits(lib_path) == want
    assert sorted(want) == ["f16", "x3"] and all(sorted(want[b]) == sorted(map(_ID, SHAPES)) for b in want)
    got = block_bits()
    for build in ("x3", "f16"):
        for shape in SHAPES:
            assert got[build][_ID(shape)] == want[build][_ID(shape)], (build, _ID(shape))
