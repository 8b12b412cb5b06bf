"""net.train_fuse_linattn and the sdc_linattn_block_bwd entry, the parts that need no GPU: the switch, the declared symbols, the
argument checks that run before any launch or device query, the workspace bound."""
import ctypes as C

import pytest

import safediffcon_amd as sdc
from safediffcon_amd import _lib

SDC_EINVAL, SDC_ENULL = -1, -4


def test_train_fuse_linattn_switch():
    net = sdc.Unet3D_with_Conv3D(dim=8, dim_mults=(1, 2), channels=7)
    assert net.train_fuse_linattn is False
    net.train_fuse_linattn = True
    assert net.train_fuse_linattn is True
    for bad in (1, 0, None, "on", 1.5):
        with pytest.raises(ValueError):
            net.train_fuse_linattn = bad
        assert net.train_fuse_linattn is True        # a rejected value leaves the switch unchanged
    assert net.train_fuse_attn is False              # independent of its temporal sibling
    net.train_fuse_linattn = False
    assert net.train_fuse_linattn is False
    assert sdc.Unet1D(dim=32, dim_mults=(1, 2), channels=12, resnet_block_groups=1).train_fuse_linattn is False
    # not a plan switch: the sampler plans and their cache key never see it
    from safediffcon_amd import engine
    assert "train_fuse_linattn" not in getattr(engine, "PLAN_SWITCHES", ())


def test_symbols_declared_and_exported():
    lib = _lib.get_lib()
    for name in ("sdc_linattn_block_bwd_bytes", "sdc_linattn_block_bwd"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert _lib.SIGNATURES["sdc_linattn_block_bwd_bytes"][0] is C.c_size_t
    assert len(_lib.SIGNATURES["sdc_linattn_block_bwd"][1]) == 23


ORDER = ("x", "g", "wqkv", "wo", "bo", "dy", "dx", "dg", "dwqkv", "dwo", "dbo", "work", "outer", "inner", "C", "n", "so", "sc", "si",
         "pre_mode", "post_mode")


def _call(**kw):
    P = 256                                          # a non-null, 16-byte aligned address that is never dereferenced
    ok = dict(x=P, g=P, wqkv=P, wo=P, bo=P, dy=P + 4096, dx=P + 8192, dg=P, dwqkv=P, dwo=P, dbo=P, work=P,
              outer=2, inner=3, C=64, n=128, so=64 * 3 * 128, sc=3 * 128, si=128, pre_mode=0, post_mode=-1)
    a = dict(ok, **kw)
    return _lib.get_lib().sdc_linattn_block_bwd(*(a[k] for k in ORDER), 1e-5, None)


def test_backward_entry_rejects_before_any_launch():
    for name in ("x", "g", "wqkv", "wo", "dy", "dx", "dg", "dwqkv", "dwo", "work"):
        assert _call(**{name: None}) == SDC_ENULL, name
        assert f"null {'g_pre' if name == 'g' else name}" in _lib.last_error()      # the message names the pointer
    assert _call(dbo=None) == SDC_ENULL and "dbo" in _lib.last_error()      # required exactly when bo is given
    assert _call(pre_mode=1) == SDC_EINVAL and "pre norm mode 1" in _lib.last_error()
    assert _call(post_mode=0) == SDC_EINVAL and "post norm mode 0" in _lib.last_error()
    assert _call(post_mode=1) == SDC_EINVAL and "post norm mode 1" in _lib.last_error()
    for bad in (32, 96, 256):
        assert _call(C=bad) == SDC_EINVAL and "dim must be 64 or 128" in _lib.last_error()
    assert _call(n=96) == SDC_EINVAL and "multiple of 64" in _lib.last_error()
    assert _call(outer=0) == SDC_EINVAL
    assert _call(outer=256, inner=256) == SDC_EINVAL and "65536" in _lib.last_error()
    assert _call(sc=1 << 27) == SDC_EINVAL and "2^27" in _lib.last_error()
    assert _call(wqkv=256 + 4) == SDC_EINVAL and "aligned" in _lib.last_error()
    assert _call(wo=256 + 8) == SDC_EINVAL and "aligned" in _lib.last_error()
    assert _call(dx=256) == SDC_EINVAL and "alias" in _lib.last_error()
    assert _call(dx=256 + 4096) == SDC_EINVAL and "alias" in _lib.last_error()


def test_workspace_size():
    by = _lib.get_lib().sdc_linattn_block_bwd_bytes
    assert by(0, 1, 64, 64) == 0 and by(1, 1, 96, 64) == 0 and by(1, 1, 64, 96) == 0
    for Cc in (64, 128):
        assert by(1, 1, Cc, 64) > 0
        assert by(1, 2, Cc, 64) > by(1, 1, Cc, 64)
        # 64 tokens: one split, 128 sequence slots; 4096 tokens: eight splits, 32 slots.  Beyond the cap the workspace stops growing
        assert by(2, 32, Cc, 64) < by(4, 32, Cc, 64) == by(8, 32, Cc, 64) == by(1, 65535, Cc, 64)
        assert by(1, 32, Cc, 4096) == by(13, 32, Cc, 4096) == by(2047, 32, Cc, 4096)
        assert by(1, 16, Cc, 4096) < by(1, 32, Cc, 4096)
        # the stated bound (include/sdc.h), in floats
        bound = 256 * (514 * Cc + 256) + 128 * (768 * Cc + 4480) + 256 * Cc
        for n in (64, 512, 1024, 2048, 4096, 1 << 16):
            assert by(64, 64, Cc, n) <= 4 * bound
