"""Oracle: the in-kernel noise generator of the fused reverse step, restated in NumPy.

Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants) with
  counter = {idx_lo, idx_hi, draw, 0x5DC}     idx = index of the float4 (element // 4), draw = the draw number
  key     = (seed_lo, seed_hi)
Each counter gives four words -> four uniforms ((float)c + 0.5f) * 2^-32, formed in fp32 like the kernel forms them ->
two Box-Muller pairs {r0 cos, r0 sin, r1 cos, r1 sin} with r0 from word 0, its angle from word 1, r1 from word 2,
its angle from word 3.  Box-Muller itself runs in fp64 here: the kernel's fast log / sincos are what gets measured
against it.

TEST INFRASTRUCTURE -- see oracle/__init__.py.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl key increments
TAG = 0x5DC                              # fourth counter word


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape; key: two.  Returns the four output word arrays (uint32)."""
    c = [np.asarray(v, dtype=np.uint64) & 0xFFFFFFFF for v in counter]
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    for _ in range(10):
        p0 = M0 * c[0]                   # < 2^64: both factors < 2^32
        p1 = M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def words(seed, draw, nvec):
    """The (nvec, 4) uint32 words of float4 0 .. nvec-1 of draw `draw` under `seed` (a 64-bit integer)."""
    idx = np.arange(nvec, dtype=np.uint64)
    shape = idx.shape
    out = philox4x32_10([idx & 0xFFFFFFFF, idx >> 32, np.full(shape, draw & 0xFFFFFFFF, np.uint64), np.full(shape, TAG, np.uint64)],
                        (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return np.stack(out, axis=1)


def uniforms(w):
    """((float)c + 0.5f) * 2^-32 in fp32, from 2^-33 to 1.0 inclusive.  (The kernel's clamp of the radius uniforms to
    [1e-12, 1], which normals() repeats, is a no-op on every such value.)"""
    u = (w.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)
    assert u.dtype == np.float32
    return u


def normals(seed, draw, n):
    """fp64 Box-Muller of the fp32 uniforms: n (a multiple of 4) normals in the kernel's element order."""
    assert n % 4 == 0
    u = uniforms(words(seed, draw, n // 4))
    ur = np.minimum(np.maximum(u, np.float32(1e-12)), np.float32(1.0)).astype(np.float64)
    r0, r1 = np.sqrt(-2.0 * np.log(ur[:, 0])), np.sqrt(-2.0 * np.log(ur[:, 2]))
    # the kernel forms the angle 2*pi*u in fp32 before the sincos; the rounding of that product is part of what the
    # comparison measures, so the reference angle is the exact product
    t0, t1 = 2.0 * np.pi * u[:, 1].astype(np.float64), 2.0 * np.pi * u[:, 3].astype(np.float64)
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=1).reshape(-1)
