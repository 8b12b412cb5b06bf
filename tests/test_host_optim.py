"""The optimizer step's host side (include/sdc.h, sdc_optim_*): exported symbols, the chunk plan against a Python restatement,
and the argument errors -- all returned before any launch, so none of this needs a GPU."""
import ctypes as C

import pytest

from safediffcon_amd import _lib
from safediffcon_amd._lib import SdcOptItem, SdcOptState

LENGTHS = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 65537]
CHUNK, GRID_CAP = 4096, 2048            # documented in include/sdc.h


def _table(lengths, v=True, base=0x10000000):
    """a table of made-up (never dereferenced) device addresses"""
    items = (SdcOptItem * len(lengths))()
    for i, (it, n) in enumerate(zip(items, lengths)):
        a = base + i * 0x1000000
        it.p, it.g, it.m, it.v, it.ema, it.n = a, a + 0x100000, a + 0x200000, (a + 0x300000) if v else None, None, n
    return items


def _plan(items, kind=1):
    chunk, total, grid = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = _lib.get_lib().sdc_optim_plan(items, len(items), kind, C.byref(chunk), C.byref(total), C.byref(grid))
    return rc, chunk.value, total.value, grid.value


def test_symbols_exported_with_signatures():
    lib = _lib.get_lib()
    for name in ("sdc_optim_plan", "sdc_optim_bytes", "sdc_optim_step"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert C.sizeof(SdcOptItem) == 56 and C.sizeof(SdcOptState) == 24
    assert lib.sdc_optim_bytes(0) == 0 and lib.sdc_optim_bytes(1000) == 8000


@pytest.mark.parametrize("lengths", [LENGTHS, LENGTHS + [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7], [7], [GRID_CAP * CHUNK],
                                     [GRID_CAP * CHUNK + 1, 3], [5, (GRID_CAP + 3) * CHUNK + 5, 1]])
def test_plan_matches_restatement(lengths):
    items = _table(lengths)
    rc, chunk, total, grid = _plan(items)
    assert rc == 0, _lib.last_error()
    assert chunk == CHUNK
    prefix, acc = [], 0
    for n in lengths:
        prefix.append(acc)
        acc += -(-n // chunk)
    assert [it.chunk0 for it in items] == prefix
    assert total == acc and grid == min(acc, GRID_CAP)
    assert [it.n for it in items] == lengths                      # the caller's fields are left alone
    assert _lib.get_lib().sdc_optim_bytes(total) == 8 * total


def test_plan_kinds():
    for kind in (0, 1, 2):
        assert _plan(_table([5, 9]), kind)[0] == 0
    assert _plan(_table([5, 9], v=False), 0)[0] == 0              # SGD keeps no second moment


def test_plan_errors_before_any_launch():
    lib = _lib.get_lib()
    for field in ("p", "g", "m", "v"):
        items = _table([8, 8])
        setattr(items[1], field, None)
        assert _plan(items, 1)[0] == -4, field
        assert "null" in _lib.last_error() and "item 1" in _lib.last_error()
    items = _table([8, 8])
    items[0].v = None
    assert _plan(items, 2)[0] == -4 and _plan(items, 0)[0] == 0
    for field in ("p", "g", "m", "v", "ema"):
        items = _table([8, 8])
        setattr(items[0], field, 0x20000002)
        assert _plan(items, 1)[0] == -2, field
        assert "aligned" in _lib.last_error()
    items = _table([8, 8])
    items[0].ema = 0x20000004                                     # 4-byte aligned is enough
    assert _plan(items, 1)[0] == 0
    for n in (0, -3):
        assert _plan(_table([8, n]), 1)[0] == -1
    for kind in (-1, 3):
        assert _plan(_table([8]), kind)[0] == -1
        assert "kind" in _lib.last_error()
    chunk, total, grid = C.c_int(), C.c_int(), C.c_int()
    assert lib.sdc_optim_plan(_table([8]), 0, 1, C.byref(chunk), C.byref(total), C.byref(grid)) == -1
    assert lib.sdc_optim_plan(None, 1, 1, C.byref(chunk), C.byref(total), C.byref(grid)) == -4
    with pytest.raises(_lib.SdcError):
        _lib.check(-4, "sdc_optim_plan")


def test_step_errors_before_any_launch():
    lib = _lib.get_lib()
    tab, hp, st, work = 0x10000000, 0x20000000, 0x30000000, 0x40000000
    good = dict(kind=1, items=tab, n=2, chunk=CHUNK, total=5, grid=5, hp=hp, st=st, work=work, flags=3)

    def call(**kw):
        a = dict(good, **kw)
        return lib.sdc_optim_step(a["kind"], a["items"], a["n"], a["chunk"], a["total"], a["grid"], a["hp"], a["st"], a["work"], a["flags"], 0)
    for kind in (-1, 3, 99):
        assert call(kind=kind) == -1
        assert "kind" in _lib.last_error()
    for k in ("items", "hp", "st", "work"):
        assert call(**{k: 0}) == -4, k
    assert call(hp=hp + 4) == -2 and call(st=st + 4) == -2 and call(work=work + 4) == -2
    assert call(n=0) == -1 and call(chunk=CHUNK // 2) == -1 and call(total=1) == -1 and call(grid=0) == -1
    assert call(grid=6) == -1 and call(grid=GRID_CAP + 1, total=GRID_CAP + 1) == -1 and call(flags=4) == -1
