"""No GPU: the library-side dispatch of the fused LinearAttention block's bf16-split projections (csrc/sdc_lablock_x3.hip, DESIGN.md
section 22) -- the routing table sdc_linattn_block_x3_ok, the argument checks of sdc_linattn_block_sel / sdc_linattn_block_gn_sel (every
refusal comes before any launch: none of these calls needs a device) and the unchanged scratch size."""
import ctypes
import os
import re

import pytest

from safediffcon_amd import _lib

# the (C, tokens per sequence) the table lists: the measured fused sites of the default C4 and C2 plans that qualified per launch with
# a margin (profiles/linattn_x3_shapes.log)
LISTED = {(64, 4096), (64, 1024), (128, 1024), (64, 2048), (128, 512)}


def _codes():
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdc.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (SDC_E\w+) \((-?\d+)\)", txt)}


def test_x3_ok_table():
    ok = _lib.get_lib().sdc_linattn_block_x3_ok
    for Cc in (0, 32, 64, 128, 256):
        for n in (0, -64, 1, 63, 64, 100, 128, 256, 512, 1000, 1024, 1088, 2048, 4096, 4100, 8192, 1 << 20, (1 << 32) + 4096):
            assert ok(Cc, n) == (1 if (Cc, n) in LISTED else 0), (Cc, n)
    # never a width the kernels do not have, never a ragged or empty sequence
    for Cc, n in LISTED:
        assert Cc in (64, 128) and n > 0 and n % 64 == 0


def _fake(n):
    """distinct non-null, 16-byte aligned addresses: the checks under test return before any of them is read"""
    return [ctypes.cast(0x10000 * (i + 1), ctypes.POINTER(ctypes.c_float)) for i in range(n)]


def _sel(impl, outer=2, inner=1, Cc=64, n=128, pre=0, post=0):
    lib = _lib.get_lib()
    x, g, wq, wo, bo, gp, work, y = _fake(8)
    return lib.sdc_linattn_block_sel(x, g, wq, wo, bo, gp, work, y, outer, inner, Cc, n, Cc * inner * n, inner * n, n, pre, post, 1e-5,
                                     impl, None)


def _gn_sel(impl, outer=2, inner=1, Cc=64, n=128, G=8):
    lib = _lib.get_lib()
    x, st, ga, be, res, g, wq, wo, bo, gp, work, y = _fake(12)
    return lib.sdc_linattn_block_gn_sel(x, st, ga, be, G, res, g, wq, wo, bo, gp, work, y, outer, inner, Cc, n, Cc * inner * n, inner * n,
                                        n, 0, 0, 1e-5, impl, None)


@pytest.mark.parametrize("impl", [-1, 2, 3, 1 << 20])
def test_sel_refuses_a_bad_impl(impl):
    einval = _codes()["SDC_EINVAL"]
    assert _sel(impl) == einval and "impl" in _lib.last_error()
    assert _gn_sel(impl) == einval and "impl" in _lib.last_error()


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("kw", [dict(Cc=256), dict(Cc=32), dict(n=100), dict(n=0), dict(outer=0), dict(inner=0), dict(pre=2), dict(post=2),
                                dict(outer=65536)])
def test_sel_refuses_a_bad_shape(impl, kw):
    assert _sel(impl, **kw) == _codes()["SDC_EINVAL"]


@pytest.mark.parametrize("impl", [0, 1])
def test_gn_sel_refuses_bad_groups_and_null(impl):
    codes = _codes()
    assert _gn_sel(impl, G=0) == codes["SDC_EINVAL"]
    assert _gn_sel(impl, G=7) == codes["SDC_EINVAL"]
    assert _gn_sel(impl, Cc=256) == codes["SDC_EINVAL"]
    lib = _lib.get_lib()
    x, st, ga, be, res, g, wq, wo, bo, gp, work, y = _fake(12)
    assert lib.sdc_linattn_block_gn_sel(x, None, ga, be, 8, res, g, wq, wo, bo, gp, work, y, 2, 1, 64, 128, 64 * 128, 128, 128, 0, 0, 1e-5,
                                        impl, None) == codes["SDC_ENULL"]
    assert lib.sdc_linattn_block_sel(None, g, wq, wo, bo, gp, work, y, 2, 1, 64, 128, 64 * 128, 128, 128, 0, 0, 1e-5, impl,
                                     None) == codes["SDC_ENULL"]


def test_block_bytes_unchanged():
    """the split kernels use la_blk's scratch: partials [nseq][nsplit][4][32 (C + 2)] then T [nseq][128][C], fp32"""
    b = _lib.get_lib().sdc_linattn_block_bytes
    for outer, inner, Cc, n in [(2, 1, 64, 64), (2, 3, 64, 256), (5, 1, 128, 128), (2, 2, 64, 1088), (1, 2, 128, 1024), (64, 32, 64, 4096),
                                (64, 32, 128, 1024), (256, 1, 64, 2048), (1, 1, 64, 1 << 16)]:
        nseq, ntiles = outer * inner, n // 64
        ns = max(1, min(8, ntiles // 8))
        assert b(outer, inner, Cc, n) == 4 * (nseq * ns * 4 * 32 * (Cc + 2) + nseq * 128 * Cc), (outer, inner, Cc, n)
    assert b(2, 1, 256, 64) == 0 and b(0, 1, 64, 64) == 0 and b(2, 1, 64, 0) == 0
