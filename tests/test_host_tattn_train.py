"""net.train_fuse_attn and the sdc_tattn_block_bwd entry, the parts that need no GPU: the switch, the declared symbols, the argument
checks that run before any launch or device query."""
import ctypes as C

import pytest

import safediffcon_amd as sdc
from safediffcon_amd import _lib

SDC_EINVAL, SDC_ENULL = -1, -4


def test_train_fuse_attn_switch():
    net = sdc.Unet3D_with_Conv3D(dim=8, dim_mults=(1, 2), channels=7)
    assert net.train_fuse_attn is False
    net.train_fuse_attn = True
    assert net.train_fuse_attn is True
    for bad in (1.5, "on", None, 1, 0):
        with pytest.raises(ValueError):
            net.train_fuse_attn = bad
        assert net.train_fuse_attn is True           # a rejected value leaves the switch unchanged
    net.train_fuse_attn = False
    assert net.train_fuse_attn is False
    assert sdc.Unet1D(dim=32, dim_mults=(1, 2), channels=12, resnet_block_groups=1).train_fuse_attn is False
    # not a plan switch: the sampler plans and their cache key never see it
    from safediffcon_amd import engine
    assert "train_fuse_attn" not in getattr(engine, "PLAN_SWITCHES", ())


def test_symbols_declared_and_exported():
    lib = _lib.get_lib()
    for name in ("sdc_tattn_block_bwd_bytes", "sdc_tattn_block_bwd"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert _lib.SIGNATURES["sdc_tattn_block_bwd_bytes"][0] is C.c_size_t
    assert len(_lib.SIGNATURES["sdc_tattn_block_bwd"][1]) == 22


def test_backward_entry_rejects_before_any_launch():
    lib = _lib.get_lib()
    P = 256                                          # a non-null, 16-byte aligned address that is never dereferenced
    ok = dict(x=P, g=P, wqkv=P, wo=P, rot=P, bias=P, dy=P, dx=P, dg=P, dwqkv=P, dwo=P, dbias=P, work=P,
              outer=2, inner=16, C=64, ntok=32, so=64 * 32 * 16, sc=32 * 16, st=16)
    order = ("x", "g", "wqkv", "wo", "rot", "bias", "dy", "dx", "dg", "dwqkv", "dwo", "dbias", "work", "outer", "inner", "C", "ntok", "so", "sc", "st")

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sdc_tattn_block_bwd(*(a[k] for k in order), 1e-5, None)

    for name in ("x", "g", "wqkv", "wo", "dy", "dx", "dg", "dwqkv", "dwo", "work"):
        assert call(**{name: None}) == SDC_ENULL, name
        assert "null" in _lib.last_error()
    assert call(dbias=None) == SDC_ENULL             # required exactly when bias is given
    assert call(C=128) == SDC_EINVAL and "dim 64" in _lib.last_error()
    assert call(ntok=16) == SDC_EINVAL and "32 frames" in _lib.last_error()
    assert call(inner=12) == SDC_EINVAL and "multiple of 8" in _lib.last_error()
    assert call(outer=0) == SDC_EINVAL
    assert call(st=1 << 28) == SDC_EINVAL and "4 GB" in _lib.last_error()
    assert call(wqkv=P + 4) == SDC_EINVAL and call(wo=P + 8) == SDC_EINVAL and call(rot=P + 4) == SDC_EINVAL


def test_workspace_size():
    lib = _lib.get_lib()
    assert lib.sdc_tattn_block_bwd_bytes(1, 8) > 0
    assert lib.sdc_tattn_block_bwd_bytes(1, 16) == 2 * lib.sdc_tattn_block_bwd_bytes(1, 8)
    # once every workgroup has a pixel group the workspace stops growing
    assert lib.sdc_tattn_block_bwd_bytes(4, 1024) == lib.sdc_tattn_block_bwd_bytes(8, 1024)
