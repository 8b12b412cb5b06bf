"""-m gpu: ta_block_x3s_kernel, the width-64 fused temporal-attention block with bf16-split projections in which waves 4 - 7 -- the
second wave of every SIMD -- run half a head behind waves 0 - 3 (csrc/sdc_tablock_x3.hip, DESIGN.md section 19, "The skewed form").
The skew moves when a wave issues its instructions, never which: impl 1 of sdc_tattn_block_x3_sel must give impl 0's bits.  Block
level, through the C ABI with `impl` forced, on the inputs of tests/test_gpu_attn_x3.py (which holds impl 0 against the exact fp64
block): equality on a NaN-prefilled output with and without the tables, run-to-run and batch invariance, non-finite input."""
import pytest
import torch

from safediffcon_amd import _lib
from test_gpu_attn_x3 import DEV, Cc, Fr, SHAPES as X3_SHAPES, _inputs, _pack_dev, _ptr, _stream, _tables

pytestmark = pytest.mark.gpu

# (B, H, W): the five shapes of tests/test_gpu_attn_x3.py, and one with 768 pixel groups: at least three tiles on every workgroup (one
# per CU, at most 256), so every tile-to-tile handoff of the weights (head 0's q / k / v behind head 3, its Wo in the exit) and of the
# lagging waves (the drain, then head 0 without a tail) runs on every workgroup
BIG = (2, 48, 64)
SHAPES = list(X3_SHAPES) + [BIG]
_DEVICE = {}


def _dev_case(shape):
    """the inputs of a shape on the device (uploaded once, never modified)"""
    if shape not in _DEVICE:
        x, g, wqkv, wo, freqs, relw = _inputs(*shape)
        _DEVICE[shape] = (x, x.to(DEV), g.to(DEV), _pack_dev(wqkv, wo), _tables(freqs, relw))
    return _DEVICE[shape]


def _run(impl, x_dev, g_dev, wpk, rot, bias, eps=1e-5):
    """one sdc_tattn_block_x3_sel call on a NaN-filled output"""
    lib = _lib.get_lib()
    B, _, _, H, W = x_dev.shape
    y = torch.full_like(x_dev, float("nan"))
    _lib.check(lib.sdc_tattn_block_x3_sel(x_dev.data_ptr(), g_dev.data_ptr(), wpk.data_ptr(), _ptr(rot), _ptr(bias), y.data_ptr(),
                                          B, H * W, Cc, Fr, Cc * Fr * H * W, Fr * H * W, H * W, eps, impl, _stream()),
               "sdc_tattn_block_x3_sel")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("tables", [True, False], ids=["tables", "null-tables"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_skewed_block_gives_the_unskewed_bits(shape, tables):
    _, x_dev, g_dev, wpk, (rot, bias) = _dev_case(shape)
    if not tables:
        rot = bias = None
    y0 = _run(0, x_dev, g_dev, wpk, rot, bias)
    y1 = _run(1, x_dev, g_dev, wpk, rot, bias)                # (NaN-prefilled: every element is overwritten)
    assert torch.isfinite(y0).all() and torch.isfinite(y1).all()
    assert torch.equal(y1, y0)


def test_skewed_block_is_deterministic_and_batch_invariant():
    _, x_dev, g_dev, wpk, (rot, bias) = _dev_case(BIG)
    y = _run(1, x_dev, g_dev, wpk, rot, bias)
    for _ in range(3):                                        # four runs in all
        assert torch.equal(_run(1, x_dev, g_dev, wpk, rot, bias), y)
    assert torch.equal(_run(1, x_dev[:1].contiguous(), g_dev, wpk, rot, bias)[0], y[0])


def test_skewed_block_non_finite_input():
    """a non-finite x makes every frame and channel of its own pixel non-finite and nothing else, as
    test_attn_x3_block_non_finite_input holds for impl 0"""
    shape = X3_SHAPES[2]
    x, x_dev, g_dev, wpk, (rot, bias) = _dev_case(shape)
    clean = _run(1, x_dev, g_dev, wpk, rot, bias)
    for bad in (float("nan"), float("inf"), -float("inf")):
        xb = x.clone()
        xb[1, 5, 9, 2, 3] = bad
        y = _run(1, xb.to(DEV), g_dev, wpk, rot, bias)
        hit = torch.zeros_like(y, dtype=torch.bool)
        hit[1, :, :, 2, 3] = True
        assert not torch.isfinite(y[hit]).any(), bad
        assert torch.equal(y[~hit], clean[~hit]), bad
