"""Inputs and references shared by tests/test_host_attn_long.py and tests/test_gpu_attn_long.py: the token-contiguous,
rot-free, bias-free softmax attention core past 256 tokens (csrc/sdc_attn_long.hip).  Everything here is CPU torch."""
import functools

import torch

from oracle.detweights import det_tensor

HEADS = 4
BLOCK = 64            # keys per streamed block of the kernel
CAP = 4096            # sdc::ATTN_LONG_MAX
# (outer, inner, ntok) of the core cases
SHAPES = [(2, 3, 257), (1, 2, 320), (2, 1, 400), (1, 2, 1024), (1, 1, 4096)]


def rel(a, b):
    """_rel of tests/test_gpu_grad.py"""
    return ((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def strides(outer, inner, n):
    """(q strides, out strides) of a dense (outer, C, inner, n) tensor"""
    return (384 * inner * n, inner * n, n, 1), (128 * inner * n, inner * n, n, 1)


@functools.lru_cache(maxsize=None)
def core_inputs(outer, inner, ntok):
    """qkv as in test_softmax_attention_core, dout as in test_full_attention_core_backward"""
    return det_tensor((outer, 384, inner, ntok), 60) * 1.2, det_tensor((outer, 128, inner, ntok), 151)


@functools.lru_cache(maxsize=None)
def peaked_inputs():
    """ntok = 320, q scaled by 8: rows close to one-hot.  Rows 0 mod 4 point at key 3 (first block), rows 1 mod 4 at key 317
    (last block), the others wherever their random scores peak: the running maximum is raised late for some rows and never
    after the first block for others."""
    n = 320
    qkv, gout = det_tensor((1, 384, 2, n), 61) * 1.2, det_tensor((1, 128, 2, n), 152)
    qkv = qkv.clone()
    q, k = qkv[:, :128], qkv[:, 128:256]
    q[..., 0::4] = q[..., 0:1] + 0.1 * q[..., 0::4]
    q[..., 1::4] = q[..., 1:2] + 0.1 * q[..., 1::4]
    k[..., 3] = q[..., 0]
    k[..., 317] = q[..., 1]
    q *= 8.0
    return qkv, gout


@functools.lru_cache(maxsize=None)
def zero_q_inputs():
    qkv, gout = core_inputs(1, 2, 320)
    qkv = qkv.clone()
    qkv[:, :128] = 0.0
    return qkv, gout


def split_heads(qkv):
    """(outer, 384, inner, n) -> q, k, v of shape (outer, inner, heads, n, 32)"""
    B, _, inner, n = qkv.shape
    return tuple(t.reshape(B, HEADS, 32, inner, n).permute(0, 3, 1, 4, 2) for t in qkv.chunk(3, dim=1))


def merge_heads(o):
    """(outer, inner, heads, n, 32) -> (outer, 128, inner, n)"""
    B, inner, _, n, _ = o.shape
    return o.permute(0, 2, 4, 1, 3).reshape(B, 128, inner, n)


def reference(qkv, gout=None):
    """float64 softmax attention, one head at a time (an ntok x ntok matrix of one head only is alive at any moment);
    -> out, and dqkv by autograd when gout is given"""
    qd = qkv.double().requires_grad_(gout is not None)
    q, k, v = split_heads(qd)
    outs = []
    for h in range(HEADS):
        sim = torch.einsum("...id,...jd->...ij", q[:, :, h] * 32 ** -0.5, k[:, :, h])
        oh = torch.einsum("...ij,...jd->...id", sim.softmax(-1), v[:, :, h])
        if gout is not None:
            gh = merge_heads_grad(gout.double(), h)
            (oh * gh).sum().backward()
            oh = oh.detach()
        outs.append(oh)
    out = merge_heads(torch.stack(outs, dim=2))
    return (out, qd.grad) if gout is not None else out


def merge_heads_grad(gout, h):
    """the (outer, inner, n, 32) slice of dout that belongs to head h"""
    B, _, inner, n = gout.shape
    return gout.reshape(B, HEADS, 32, inner, n)[:, h].permute(0, 2, 3, 1)


def blocked_forward(qkv, block=BLOCK):
    """float32 restatement of the kernel's forward: keys in blocks of `block` in ascending order, running maximum, rescale
    of the running sum and of the accumulator, the ragged last block masked to -inf"""
    q, k, v = split_heads(qkv.float())
    q = q * torch.tensor(0.17677669529663687, dtype=torch.float32)
    n = q.shape[-2]
    m = torch.full(q.shape[:-1], float("-inf"))
    l = torch.zeros(q.shape[:-1])
    o = torch.zeros(q.shape)
    for j0 in range(0, n, block):
        kb = torch.zeros(*k.shape[:-2], block, 32)
        vb = torch.zeros(*v.shape[:-2], block, 32)
        w = min(block, n - j0)
        kb[..., :w, :] = k[..., j0:j0 + w, :]
        vb[..., :w, :] = v[..., j0:j0 + w, :]
        s = q @ kb.transpose(-1, -2)
        s[..., w:] = float("-inf")
        mn = torch.maximum(m, s.amax(-1))
        alpha = torch.exp(m - mn)
        p = torch.exp(s - mn[..., None])
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + p @ vb
        m = mn
    return merge_heads(o / l[..., None])
