"""Inputs and references shared by tests/test_host_tattn_frames.py and tests/test_gpu_tattn_frames.py: the temporal attention
core ('b c f h w -> b (h w) f c', rotary + relative-position bias) at 64 / 96 / 128 frames (csrc/sdc_tattn_frames.hip).
Everything here is CPU torch; the helpers restate those of tests/test_gpu_grad.py / test_gpu_grad_paths.py."""
import functools

import torch

from oracle.detweights import det_tensor

HEADS = 4
# (F, H, W, B): two full groups per sample | 15 pixels: ragged tail | 96 frames | 128 frames | 128 frames, one ragged group
SHAPES = [(64, 4, 4, 2), (64, 3, 5, 1), (96, 2, 4, 1), (128, 2, 4, 1), (128, 1, 3, 1)]
PEAKED = [(64, 4, 4, 2), (128, 2, 4, 1)]            # the shapes of the scale 2 / 4 cases
FAR = [(64, 2, 4, 1), (96, 2, 4, 1), (128, 2, 4, 1)]
GATE_OUT, GATE_GRAD = 1e-5, 2e-5                    # the gates of tests/test_gpu_grad.py


def rel(a, b):
    """_rel of tests/test_gpu_grad.py"""
    return ((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def gate(file_gate, e_fp32):
    """the project's rule for peaked inputs (tests/test_gpu_grad_paths.py): the file gate, unless the same torch formula in
    fp32 is itself further than a quarter of it from fp64 -- then 4 e_fp32"""
    return max(file_gate, 4.0 * e_fp32)


def rot_table(F_):
    """[F][16][2] cos / sin table of the kernels, and the fp64 angles (F, 32) of the reference"""
    fr = 1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))
    ang = torch.arange(F_, dtype=torch.float32)[:, None] * fr[None, :]
    return torch.stack((ang.cos(), ang.sin()), dim=-1).reshape(-1), ang.repeat_interleave(2, dim=-1).double()


def strides(heads, F_, hw):
    """(q strides, out strides) (so, sc, si, st) of dense (B, 3 heads 32, F, H, W) / (B, heads 32, F, H, W) tensors"""
    return (3 * heads * 32 * F_ * hw, F_ * hw, 1, hw), (heads * 32 * F_ * hw, F_ * hw, 1, hw)


@functools.lru_cache(maxsize=None)
def inputs(F_, H, W, B, scale=1.0, heads=HEADS):
    """(qkv, bias, gout) as tests/test_gpu_grad.py builds them"""
    qkv = det_tensor((B, 3 * heads * 32, F_, H, W), 140, scale)
    bias = 0.5 * det_tensor((heads, F_, F_), 141)
    gout = det_tensor((B, heads * 32, F_, H, W), 142)
    return qkv, bias, gout


@functools.lru_cache(maxsize=None)
def far_peak(F_, H, W, B):
    """the plain inputs with bias[:, i, (i + F/2) % F] += 8: each row's maximum sits in another 32-key block than its diagonal,
    rows near one-hot"""
    qkv, bias, gout = inputs(F_, H, W, B)
    bias = bias.clone()
    i = torch.arange(F_)
    bias[:, i, (i + F_ // 2) % F_] += 8.0
    return qkv, bias, gout


def _attention(q, k, v, ang=None, bias=None):
    """q, k, v (..., heads, n, 32)"""
    q = q * 32 ** -0.5
    if ang is not None:
        def rot(x):
            x2 = x.reshape(*x.shape[:-1], 16, 2)
            half = torch.stack((-x2[..., 1], x2[..., 0]), dim=-1).reshape(x.shape)
            return x * ang.cos() + half * ang.sin()
        q, k = rot(q), rot(k)
    sim = torch.einsum("...id,...jd->...ij", q, k)
    if bias is not None:
        sim = sim + bias
    return torch.einsum("...ij,...jd->...id", sim.softmax(-1), v)


def reference(qkv, bias, gout, dtype=torch.float64, use_rot=True):
    """autograd reference in `dtype` -> (out, dqkv, dbias | None)"""
    B, C, Fr, H, W = qkv.shape
    heads, hw = C // 96, H * W
    ang = rot_table(Fr)[1].to(dtype) if use_rot else None
    qd = qkv.detach().to(dtype).clone().requires_grad_()
    bd = bias.detach().to(dtype).clone().requires_grad_() if bias is not None else None
    q, k, v = (t.reshape(B, heads, 32, Fr, hw).permute(0, 4, 1, 3, 2) for t in qd.chunk(3, dim=1))       # (B, hw, heads, F, 32)
    o = _attention(q, k, v, ang, bd)
    out = o.permute(0, 2, 4, 3, 1).reshape(B, heads * 32, Fr, H, W)
    out.backward(gout.to(dtype))
    return out.detach(), qd.grad, (bd.grad if bd is not None else None)


@functools.lru_cache(maxsize=None)
def ref64(kind, F_, H, W, B, scale=1.0):
    """fp64 reference of inputs(...) (kind 'plain') or far_peak(...) ('far'), computed once and shared; do not modify"""
    return reference(*(inputs(F_, H, W, B, scale) if kind == "plain" else far_peak(F_, H, W, B)))


@functools.lru_cache(maxsize=None)
def err32(kind, F_, H, W, B, scale=1.0):
    """_rel of the same formula in fp32 against fp64: (out, dqkv, dbias)"""
    ins = inputs(F_, H, W, B, scale) if kind == "plain" else far_peak(F_, H, W, B)
    return tuple(rel(a, b) for a, b in zip(reference(*ins, dtype=torch.float32), ref64(kind, F_, H, W, B, scale)))
