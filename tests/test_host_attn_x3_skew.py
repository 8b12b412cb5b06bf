"""CPU-side checks of the skewed form of the bf16-split temporal-attention block (include/sdc.h: sdc_tattn_block_x3_sel,
sdc_tattn_block_x3_impl; DESIGN.md section 19, "The skewed form"): `impl` is checked before any launch, under the entry's name; the
measured table answers 0 for every size it does not list and is never keyed on the batch."""
import pytest

from safediffcon_amd import _lib

SDC_EINVAL, SDC_ENULL = -1, -4
P = 256                                              # a non-null, 16-byte aligned address that is never dereferenced


def _sel(impl, **kw):
    a = dict(x=P, g=P, w=P, rot=P, bias=P, y=P, outer=2, inner=16, C=64, ntok=32, so=64 * 32 * 16, sc=32 * 16, st=16)
    a.update(kw)
    return _lib.get_lib().sdc_tattn_block_x3_sel(a["x"], a["g"], a["w"], a["rot"], a["bias"], a["y"], a["outer"], a["inner"], a["C"],
                                                 a["ntok"], a["so"], a["sc"], a["st"], 1e-5, impl, None)


@pytest.mark.parametrize("impl", [2, -1])
def test_sel_refuses_a_bad_impl(impl):
    assert _sel(impl) == SDC_EINVAL
    err = _lib.last_error()
    assert err.startswith("sdc_tattn_block_x3_sel: ") and "impl" in err, err


@pytest.mark.parametrize("impl", [0, 1])
def test_sel_keeps_the_entry_checks_under_its_own_name(impl):
    for kw in (dict(C=32), dict(ntok=16), dict(inner=12), dict(sc=-1)):
        assert _sel(impl, **kw) == SDC_EINVAL, kw
        assert _lib.last_error().startswith("sdc_tattn_block_x3_sel: "), (kw, _lib.last_error())
    assert _sel(impl, w=None) == SDC_ENULL and _sel(impl, x=None) == SDC_ENULL


def test_impl_table_answers_zero_where_it_lists_nothing():
    lib = _lib.get_lib()
    for c, fr, inner in ((64, 32, 1024), (128, 32, 4096), (0, 0, 0), (64, 32, 256), (64, 16, 4096), (64, 32, 4095), (64, 32, 8)):
        assert lib.sdc_tattn_block_x3_impl(c, fr, inner) == 0, (c, fr, inner)
    assert lib.sdc_tattn_block_x3_impl(64, 32, 4096) in (0, 1)      # the one measured site: listed only if it qualified
