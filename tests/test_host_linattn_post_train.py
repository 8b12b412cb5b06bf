"""net.train_fuse_linattn on the 1-D nets and the sdc_linattn_block_post_bwd entry (the post-norm LinearAttention block's backward;
DESIGN.md section 26), the parts that need no GPU: the switch, the declared symbols, the argument checks that run before any launch
or device query, the workspace bound, and the unchanged domain of the older sdc_linattn_block_bwd."""
import ctypes as C
import os
import re

import pytest

import safediffcon_amd as sdc
from safediffcon_amd import _lib

SDC_EINVAL, SDC_ENULL = -1, -4
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "sdc.h")


def test_symbols_declared_and_exported():
    lib = _lib.get_lib()
    with open(HEADER) as fh:
        header = fh.read()
    for name in ("sdc_linattn_block_post_bwd_bytes", "sdc_linattn_block_post_bwd"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert re.search(r"\b%s\(" % name, header), name
    assert _lib.SIGNATURES["sdc_linattn_block_post_bwd_bytes"][0] is C.c_size_t
    assert len(_lib.SIGNATURES["sdc_linattn_block_post_bwd"][1]) == 25
    from safediffcon_amd import autograd, grad_ops
    assert callable(grad_ops.linattn_post_block) and callable(grad_ops.linattn_post_block_bwd)
    assert issubclass(autograd.LinAttnPostBlockFn, autograd.Function)


ORDER = ("x", "g_pre", "wqkv", "wo", "bo", "g_post", "dy", "dx", "dg_pre", "dwqkv", "dwo", "dbo", "dg_post", "work", "outer", "inner", "C",
         "n", "so", "sc", "si", "pre_mode", "post_mode")


def _call(**kw):
    P = 256                                          # a non-null, 16-byte aligned address that is never dereferenced
    ok = dict(x=P, g_pre=P, wqkv=P, wo=P, bo=P, g_post=P, dy=P + 4096, dx=P + 8192, dg_pre=P, dwqkv=P, dwo=P, dbo=P, dg_post=P, work=P,
              outer=2, inner=3, C=64, n=128, so=64 * 3 * 128, sc=3 * 128, si=128, pre_mode=0, post_mode=0)
    a = dict(ok, **kw)
    return _lib.get_lib().sdc_linattn_block_post_bwd(*(a[k] for k in ORDER), 1e-5, None)


def test_post_backward_entry_rejects_before_any_launch():
    for name in ("x", "g_pre", "wqkv", "wo", "g_post", "dy", "dx", "dg_pre", "dwqkv", "dwo", "dg_post", "work"):
        assert _call(**{name: None}) == SDC_ENULL, name
        assert _lib.last_error().endswith(f"null {name}")                       # the message names the pointer
    assert _call(dbo=None) == SDC_ENULL and "null dbo" in _lib.last_error()     # required exactly when bo is given
    for modes in ((0, 0), (0, 1), (1, 0), (1, 1)):                              # (the four supported pairs get past the mode checks)
        assert _call(pre_mode=modes[0], post_mode=modes[1], C=96) == SDC_EINVAL and "dim must be 64 or 128" in _lib.last_error()
    for bad in (-1, 2):
        assert _call(pre_mode=bad) == SDC_EINVAL and f"pre norm mode {bad}" in _lib.last_error()
    assert _call(post_mode=-1) == SDC_EINVAL
    assert "post norm mode -1" in _lib.last_error() and "sdc_linattn_block_bwd" in _lib.last_error()
    for bad in (-2, 2):
        assert _call(post_mode=bad) == SDC_EINVAL and f"post norm mode {bad}" in _lib.last_error()
    for bad in (32, 96, 256):
        assert _call(C=bad) == SDC_EINVAL and "dim must be 64 or 128" in _lib.last_error()
    assert _call(n=96) == SDC_EINVAL and "multiple of 64" in _lib.last_error()
    assert _call(n=0) == SDC_EINVAL and _call(outer=0) == SDC_EINVAL and _call(inner=0) == SDC_EINVAL
    assert _call(outer=256, inner=256) == SDC_EINVAL and "65536" in _lib.last_error()
    assert _call(sc=1 << 27) == SDC_EINVAL and "2^27" in _lib.last_error()
    assert _call(sc=0) == SDC_EINVAL and "2^27" in _lib.last_error()
    assert _call(wqkv=256 + 4) == SDC_EINVAL and "wqkv must be 16-byte aligned" in _lib.last_error()
    assert _call(wo=256 + 8) == SDC_EINVAL and "wo must be 16-byte aligned" in _lib.last_error()
    assert _call(dx=256) == SDC_EINVAL and "alias x" in _lib.last_error()
    assert _call(dx=256 + 4096) == SDC_EINVAL and "alias dy" in _lib.last_error()


def test_post_workspace_size():
    by = _lib.get_lib().sdc_linattn_block_post_bwd_bytes
    old = _lib.get_lib().sdc_linattn_block_bwd_bytes
    assert by(0, 1, 64, 64) == 0 and by(1, 0, 64, 64) == 0 and by(1, 1, 96, 64) == 0 and by(1, 1, 64, 96) == 0 and by(1, 1, 64, 0) == 0
    for Cc in (64, 128):
        assert by(1, 1, Cc, 64) > 0
        # monotone in outer * inner up to the cap (64 tokens: one split, 128 sequence slots), constant beyond it
        sizes = [by(k, 1, Cc, 64) for k in range(1, 129)]
        assert all(a < b for a, b in zip(sizes, sizes[1:]))
        assert by(128, 1, Cc, 64) == by(129, 1, Cc, 64) == by(8, 32, Cc, 64) == by(1, 65535, Cc, 64)
        # 4096 tokens: eight splits, 32 slots
        assert by(1, 16, Cc, 4096) < by(1, 32, Cc, 4096) == by(13, 32, Cc, 4096) == by(2047, 32, Cc, 4096)
        # the tables the post norm adds: T with its channel axis contiguous and the dg_post partials
        assert by(3, 1, Cc, 128) == old(3, 1, Cc, 128) + 4 * 3 * (128 * Cc + Cc)
        # the stated bound (include/sdc.h), in floats
        bound = 256 * (515 * Cc + 256) + 128 * (896 * Cc + 4480) + 256 * Cc
        for n in (64, 512, 1024, 2048, 4096, 1 << 16):
            assert by(64, 64, Cc, n) <= 4 * bound
    with open(HEADER) as fh:
        assert "256 (515 C + 256) + 128 (896 C + 4480) + 256 C floats" in fh.read()


def test_older_entry_keeps_its_domain():
    """sdc_linattn_block_bwd still is the form without a post norm only, with its own messages"""
    P = 256
    call = lambda pre, post: _lib.get_lib().sdc_linattn_block_bwd(P, P, P, P, P, P + 4096, P + 8192, P, P, P, P, P, 2, 3, 64, 128,     # noqa: E731
                                                                  64 * 3 * 128, 3 * 128, 128, pre, post, 1e-5, None)
    assert call(1, -1) == SDC_EINVAL
    assert _lib.last_error() == "sdc_linattn_block_bwd: pre norm mode 1 is not supported (0, channel LayerNorm, only)"
    assert call(0, 0) == SDC_EINVAL
    assert _lib.last_error() == "sdc_linattn_block_bwd: post norm mode 0 is not supported (-1, no post norm, only)"
    assert len(_lib.SIGNATURES["sdc_linattn_block_bwd"][1]) == 23


def test_routing_predicate():
    """the kernel's domain less the one site whose fused forward + backward measured slower than the chain"""
    from safediffcon_amd.autograd import la_post_fusable
    for B, Cc, n in ((64, 64, 2048), (64, 64, 512), (64, 128, 128), (64, 128, 64), (1, 64, 64), (65535, 128, 1024)):
        assert la_post_fusable(B, Cc, n), (B, Cc, n)
    for B, Cc, n in ((64, 128, 512), (64, 256, 64), (64, 32, 64), (64, 64, 96), (64, 64, 32), (65536, 64, 64)):
        assert not la_post_fusable(B, Cc, n), (B, Cc, n)


@pytest.mark.parametrize("make",[lambda: sdc.Unet2D(dim=8, dim_mults=(1, 2), channels=3, resnet_block_groups=1),
                                  lambda: sdc.Unet1D(dim=8, dim_mults=(1, 2), channels=12, resnet_block_groups=1)], ids=["Unet2D", "Unet1D"])
def test_switch_on_the_1d_nets(make):
    net = make()
    assert net.train_fuse_linattn is False
    net.train_fuse_linattn = True
    assert net.train_fuse_linattn is True
    for bad in (1, 0, None, "on", 1.5):
        with pytest.raises(ValueError):
            net.train_fuse_linattn = bad
        assert net.train_fuse_linattn is True        # a rejected value leaves the switch unchanged
    net.train_fuse_linattn = False
    assert net.train_fuse_linattn is False
    from safediffcon_amd import engine
    assert "train_fuse_linattn" not in getattr(engine, "PLAN_SWITCHES", ())
