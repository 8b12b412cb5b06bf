"""CPU: the streaming softmax attention past 256 tokens (csrc/sdc_attn_long.hip) without a GPU.
(a) The kernel's algorithm -- keys in blocks of 64, running maximum, rescale, ragged last block masked -- restated in float32
    torch stays inside the forward gate of tests/test_gpu_attn_long.py (1e-5, _rel) against float64 softmax attention on every
    input set that file uses, so the gate is met by the reference arithmetic alone and the inputs are fair.
(b) sdc_attn_bwd_bytes: unchanged up to 256 tokens, O(rows) beyond."""
import pytest
import torch

import attn_long_ref as R
from safediffcon_amd import _lib

INPUTS = [(f"core {s}", lambda s=s: R.core_inputs(*s)[0]) for s in R.SHAPES]
INPUTS += [("1-D layout 260", lambda: R.core_inputs(2, 1, 260)[0]), ("peaked 320", lambda: R.peaked_inputs()[0]),
           ("q = 0, 320", lambda: R.zero_q_inputs()[0])]


@pytest.mark.parametrize("tag,make", INPUTS, ids=[t for t, _ in INPUTS])
def test_blocked_online_softmax_meets_the_forward_gate(tag, make):
    qkv = make()
    ref = R.reference(qkv)
    err = R.rel(R.blocked_forward(qkv), ref)
    print(f"[measured] blocked online softmax (float32, blocks of {R.BLOCK}) vs float64, {tag}: {err:.2e}")
    assert err < 1e-5


def test_the_peaked_input_raises_the_running_maximum_early_and_late():
    """rows whose maximum sits in the first block and rows whose maximum sits in the last one, and rows close to one-hot"""
    q, k, _ = R.split_heads(R.peaked_inputs()[0].double())
    sim = torch.einsum("...id,...jd->...ij", q * 32 ** -0.5, k)
    blk = sim.argmax(-1) // R.BLOCK
    assert (blk == 0).any() and (blk == (320 - 1) // R.BLOCK).any()
    assert (blk[..., 0::4] == 0).all() and (blk[..., 1::4] == 4).all()
    assert sim.softmax(-1).amax(-1).median().item() > 0.9


# 1024 partial tables of heads * ntok * ntok floats: the values of the build before the streaming kernels
@pytest.mark.parametrize("shape,want", [((2, 4, 4, 32), 16777216), ((1, 1, 4, 256), 1073741824), ((3, 2, 8, 100), 327680000)])
def test_bwd_bytes_up_to_256_tokens_are_unchanged(shape, want):
    assert _lib.get_lib().sdc_attn_bwd_bytes(*shape) == want


def test_bwd_bytes_past_256_tokens_grow_with_the_rows():
    f = _lib.get_lib().sdc_attn_bwd_bytes
    b1, b4 = f(1, 32, 4, 1024), f(1, 32, 4, 4096)
    assert b1 > 0 and b4 == 4 * b1                                  # linear in ntok, not quadratic
    assert f(4, 32, 4, 1024) == 4 * b1 and f(1, 64, 4, 1024) == 2 * b1 and f(1, 32, 8, 1024) == 2 * b1
    assert b1 <= 16 * 1 * 32 * 4 * 1024                             # a few floats per row
    assert f(1, 1, 4, 257) < f(1, 1, 4, 256)                        # the first long size needs less than the last short one
