"""Stage-level execution engine: turns a U-Net description into a flat list of
libsdc_hip.so calls with every pointer, stride and size bound ahead of time.

PyTorch is plumbing here (device memory, streams): tensors are allocated once per
plan from a reuse pool, handed to the kernels as raw pointers, and the recorded
call list is either replayed from Python or captured into one hipGraph.
Nothing in this file computes on the CPU or through torch ops on the hot path.
"""
import collections
import ctypes as C
import functools
import os
import math

import torch

from . import _lib
from ._lib import SdcConvDesc, check


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _val(x):
    """x, or x() where a weight is handed over as a callable that reads the live parameter"""
    return x() if callable(x) else x


def _s5(t):
    assert t.dim() == 5, t.shape
    return tuple(int(s) for s in t.stride())


def as5(t):
    """(B,C,L) / (B,C,H,W) / (B,C,D,H,W) -> 5-D view (B,C,D,H,W)."""
    while t.dim() < 5:
        t = t.unsqueeze(2)
    return t


@functools.lru_cache(maxsize=16)
def _up2_merge(parity, device):
    """tap-merging matrix of the sub-pixel form of nearest-x2 upsampling + 3-tap conv, kept per device (no host-to-device copy per call)"""
    return torch.tensor([[1, 0, 0], [0, 1, 1]] if parity == 0 else [[1, 1, 0], [0, 0, 1]], dtype=torch.float64, device=device)


def pack_conv_weight(t, kind="conv", precision=0):
    """Kernel layout of a conv weight (include/sdc.h, SdcConvDesc.precision):
    nn.Conv{1,2,3}d weight (Cout,Cin,*k) -> Wp [taps*Cin][Cout], followed for precision >= 2 by the Winograd taps;
    kind 'convT': nn.ConvTranspose3d weight (Cin,Cout,*k) -> flipped-tap conv weight;
    kind 'unshuffle': 1x1 conv after 'b c (h p1) (w p2) -> b (c p1 p2) h w' -> 2x2 stride-2 conv;
    kind ('convT_sub', ph, pw) / ('up2_sub', ph, pw): the sub-pixel forms below."""
    def base():
        if kind == "convT":
            t5 = as5(t)                                   # (Cin, Cout, kD, kH, kW)
            t5 = t5.flip(2, 3, 4).permute(2, 3, 4, 0, 1)  # (kD,kH,kW,Cin,Cout)
            return t5.reshape(-1, t5.shape[-1]).contiguous()
        if isinstance(kind, tuple) and kind[0] == "convT_sub":
            # sub-pixel form of ConvTranspose (1,4,4)/(1,2,2)/(0,1,1): output parity (ph, pw) is a 2x2 conv of the
            # input with taps kh in (3,1) [ph=0] / (2,0) [ph=1] (same along W): out[2j+ph] = sum_t x[j+t-(1-ph)] W[kh_t]
            _, ph, pw = kind
            t5 = as5(t)                                   # (Cin, Cout, 1, 4, 4)
            kh = (3, 1) if ph == 0 else (2, 0)
            kw = (3, 1) if pw == 0 else (2, 0)
            # (taps (3, 1) = the odd taps reversed, (2, 0) = the even ones reversed -- as slices: indexing with a Python list
            # builds an index tensor on the host and copies it over, which drains the stream every call and cannot be recorded by a
            # stream capture (safediffcon_amd/train_graph.py))
            sub = t5[:, :, 0][:, :, (1 - ph)::2][:, :, :, (1 - pw)::2].flip(2, 3)          # (Cin, Cout, 2, 2)
            assert kh == ((3, 1) if ph == 0 else (2, 0)) and kw == ((3, 1) if pw == 0 else (2, 0))
            return sub.permute(2, 3, 0, 1).reshape(-1, sub.shape[1]).contiguous()
        if isinstance(kind, tuple) and kind[0] == "up2_sub":
            # nearest x2 upsampling + 3x3 conv (pad 1), output parity (ph, pw): rows 2i+ph of the upsampled image see
            # x[i-1], x[i], x[i] (ph = 0) or x[i], x[i], x[i+1] (ph = 1) -> a 2-tap kernel with merged weights
            # (W0, W1+W2) on rows (i-1, i)  /  (W0+W1, W2) on rows (i, i+1); same along W.  9 taps -> 4.
            _, ph, pw = kind
            t5 = as5(t).to(torch.float64)                 # (Cout, Cin, 1, 3, 3)
            mh, mw = _up2_merge(ph, t5.device), _up2_merge(pw, t5.device)
            sub = torch.einsum("ah,bw,oihw->oiab", mh, mw, t5[:, :, 0])                 # (Cout, Cin, 2, 2)
            return sub.permute(2, 3, 1, 0).reshape(-1, sub.shape[0]).to(torch.float32).contiguous()
        if kind == "unshuffle":
            co, c4 = t.shape[0], t.shape[1]
            t4 = t.reshape(co, c4 // 4, 2, 2)             # (Cout, C, p1, p2)
            return t4.permute(2, 3, 1, 0).reshape(-1, co).contiguous()
        t5 = as5(t)                                       # (Cout, Cin, kD, kH, kW)
        return t5.permute(2, 3, 4, 1, 0).reshape(-1, t5.shape[0]).contiguous()
    if precision in (6, 7):
        # precision 4's buffer, zero-padded to 16 bytes, then the fp16 tail of the 3-tap convs (f16_tail_layout)
        p4 = pack_conv_weight(t, kind, 4)
        k = tuple(as5(t).shape[2:])
        if kind != "conv" or f16_kc(k) == 0:
            return p4
        return torch.cat([p4, p4.new_zeros(-p4.numel() % 4), f16_tail(t)])
    wp = base().to(torch.float32)
    if precision not in (2, 3, 4, 5) or kind != "conv" or t.shape[-1] != 3:
        return wp
    # fp32 Wp followed by the Winograd F(2,3) taps along W, [(kd*kH + kh)*4 + xi][Cin][Cout]:
    # G g with G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]], formed in fp64 and rounded once;
    # precision 3 appends, for 3x3 (kH = kW = 3) taps, the F(2x2,3x3) taps G g G^T over (H, W): [kd][Cin][Cout][j*4 + xi]
    t5 = as5(t).to(torch.float64)                 # (Cout, Cin, kD, kH, 3)
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64, device=t5.device)
    u = torch.einsum("xk,oidhk->dhxio", G, t5)    # (kD, kH, 4, Cin, Cout)
    parts = [wp.reshape(-1), u.reshape(-1).to(torch.float32)]
    if precision == 5 and t5.shape[2] == 1 and t5.shape[3] == 1:
        # precision 5, 1-D convs: the F(4,3) taps G43 g, [xi][Cin][Cout] with xi < 6, after everything else (csrc/sdc_conv.hip conv_wg_kernel NX = 6)
        G43 = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
                            [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=torch.float64, device=t5.device)
        u43 = torch.einsum("xk,oik->xio", G43, t5[:, :, 0, 0])
        return torch.cat(parts + [u43.reshape(-1).to(torch.float32)])
    if precision >= 3 and t5.shape[3] == 3:
        u2 = torch.einsum("jh,xk,oidhk->diojx", G, G, t5)   # (kD, Cin, Cout, 4, 4): 16 components contiguous
        parts.append(u2.reshape(-1).to(torch.float32))
        if precision >= 4 and t5.shape[2] == 3:
            # F(2x2x2,3x3x3) taps, G along the depth as well: [jd][Cin][Cout][j*4 + xi]
            u3 = torch.einsum("zd,jh,xk,oidhk->ziojx", G, G, G, t5)
            parts.append(u3.reshape(-1).to(torch.float32))
    return torch.cat(parts)


def f16_kc(k):
    """channel chunk KC of the precision-6 fp16 weight tail for taps k = (kD, kH, kW); 0: that tap shape has no tail"""
    k = tuple(k)
    return 32 if tuple(k) in ((1, 1, 3), (1, 3, 3), (3, 3, 3)) else 0


def f16_tail(t, flip=False):
    """fp16 tail of a precision-6 conv weight (Cout, Cin, *k) (include/sdc.h): Wh[tap][ci // KC][co][ci % KC] = w[co][ci][tap] rounded to
    fp16 (RNE), Cin zero-padded to whole KC chunks, returned as the float32 words that hold it.  flip: the tail of the data-gradient
    weight of a precision-8 buffer (flip = 1): channels transposed, taps flipped, then rounded"""
    t5 = as5(t).to(torch.float32)
    if flip:
        t5 = t5.transpose(0, 1).flip((2, 3, 4))
    co, ci = t5.shape[0], t5.shape[1]
    kc = f16_kc(t5.shape[2:])
    nch = (ci + kc - 1) // kc
    w = t5.permute(2, 3, 4, 1, 0).reshape(-1, ci, co)                     # [tap][ci][co]
    w = torch.cat([w, w.new_zeros(w.shape[0], nch * kc - ci, co)], 1)      # Cin padded
    w = w.reshape(w.shape[0], nch, kc, co).permute(0, 1, 3, 2).contiguous()  # [tap][chunk][co][KC]
    return w.half().reshape(-1).view(torch.float32)


def pack_stem_f16(w):
    """fp16 buffer of a 7-tap stem conv weight (Cout, Cin <= 8, *k) with k = 1x1x7, 1x7x7 or 7x7x7 for sdc_conv_stem_f16 (include/sdc.h;
    host twin of sdc_pack_stem_f16, bit for bit): Wh[kd][s][co][8 h + ci] = w[co][ci][kd][tap = kh * 7 + kw = 2 s + h] rounded to fp16
    (RNE), NS = ceil(7 kH / 2) steps s, zero for ci >= Cin and for the one tap past the end; returned as the float32 words that hold it"""
    t5 = as5(w).to(torch.float32)
    co, ci, kD, kH, kW = t5.shape
    if not (kW == 7 and (kD, kH) in ((1, 1), (1, 7), (7, 7)) and 1 <= ci <= 8):
        raise ValueError(f"pack_stem_f16: taps 1x1x7, 1x7x7 or 7x7x7 and Cin <= 8 (got {tuple(t5.shape)})")
    taps, ns = kH * 7, (kH * 7 + 1) // 2
    z = t5.new_zeros(co, 8, kD, 2 * ns)
    z[:, :ci, :, :taps] = t5.reshape(co, ci, kD, taps)
    z = z.reshape(co, 8, kD, ns, 2).permute(2, 3, 0, 4, 1).contiguous()       # [kd][s][co][h][ci]
    return z.half().reshape(-1).view(torch.float32)


def pack_stem_x3(w):
    """bf16 buffer of a 7-tap stem conv weight for sdc_conv_stem_x3 (include/sdc.h; host twin of sdc_pack_stem_x3, bit for bit): three
    planes Wb[piece][kd][s][co][8 h + ci], each with the layout of pack_stem_f16, holding the exact three-way split of the fp32 weight
    -- h = bf16(w), m = bf16(w - h), l = bf16(w - h - m), all RNE, h + m + l == w -- zero for ci >= Cin and for the one tap past the
    end; returned as the float32 words that hold it"""
    t5 = as5(w).to(torch.float32)
    co, ci, kD, kH, kW = t5.shape
    if not (kW == 7 and (kD, kH) in ((1, 1), (1, 7), (7, 7)) and 1 <= ci <= 8):
        raise ValueError(f"pack_stem_x3: taps 1x1x7, 1x7x7 or 7x7x7 and Cin <= 8 (got {tuple(t5.shape)})")
    taps, ns = kH * 7, (kH * 7 + 1) // 2
    z = t5.new_zeros(co, 8, kD, 2 * ns)
    z[:, :ci, :, :taps] = t5.reshape(co, ci, kD, taps)
    z = z.reshape(co, 8, kD, ns, 2).permute(2, 3, 0, 4, 1).contiguous()       # [kd][s][co][h][ci]
    return torch.stack(split3_bf16(z)).reshape(-1).view(torch.float32)


def pack_tattn_f16(wqkv, wo):
    """fp16 buffer of the temporal-attention weights for sdc_tattn_block_f16 (include/sdc.h; host twin of sdc_pack_tattn_f16, bit for
    bit) from the nn.Linear weights to_qkv (384, 64) and to_out (64, 128), rounded to fp16 (RNE): every operand fetch of a lane (l31 =
    lane & 31, lh = lane >> 5) is 8 contiguous values j -- Wh[head][mat][s][lane][j] = Wqkv[mat * 128 + head * 32 + l31][16 s + 8 lh + j]
    (s < 4), then Wh'[head][i][s][lane][j] = Wo[32 i + l31][head * 32 + row(8 s + j, lh)] (i < 2, s < 2) with row(r, lh) = (r & 3) +
    8 (r >> 2) + 4 lh, the accumulator-row order of a 32x32 MFMA result; returned as the float32 words that hold it"""
    wqkv, wo = wqkv.to(torch.float32), wo.to(torch.float32)
    if tuple(wqkv.shape) != (384, 64) or tuple(wo.shape) != (64, 128):
        raise ValueError(f"pack_tattn_f16: to_qkv (384, 64) and to_out (64, 128) (got {tuple(wqkv.shape)}, {tuple(wo.shape)})")
    a = wqkv.reshape(3, 4, 32, 4, 2, 8).permute(1, 0, 3, 4, 2, 5)                   # [mat][head][d][s][lh][j] -> [head][mat][s][lh][d][j]
    # row(8 s + 4 jh + jl, lh) = 16 s + 8 jh + 4 lh + jl: the permutation is a transposition of index digits (no index tensor)
    b = wo.reshape(2, 32, 4, 2, 2, 2, 4).permute(2, 0, 3, 5, 1, 4, 6)               # [i][l31][head][s][jh][lh][jl] -> [head][i][s][lh][l31][jh][jl]
    return torch.cat([a.reshape(-1), b.reshape(-1)]).half().view(torch.float32)


def pack_linattn_f16(wqkv, wo):
    """fp16 buffer of the LinearAttention weights for sdc_linattn_block_f16 / sdc_linattn_block_gn_f16 (include/sdc.h; host twin of
    sdc_pack_linattn_f16, bit for bit) from the unpacked 1x1 weights to_qkv (384, C) and to_out (C, 128), C in {64, 128} (trailing
    unit axes of a conv weight are dropped), rounded to fp16 (RNE): every operand fetch of a lane (l31 = lane & 31, lh = lane >> 5) is
    8 contiguous values j -- Wh[mat][head][s][lane][j] = Wqkv[mat * 128 + head * 32 + l31][16 s + 8 lh + j], mat = 0 q, 1 k, s < C / 16.
    to_out is checked and not read (T = Wo ctx is formed in fp32 and rounded per sequence); returned as the float32 words that hold it"""
    wqkv, wo = wqkv.to(torch.float32), wo.to(torch.float32)
    wqkv, wo = wqkv.reshape(wqkv.shape[0], -1), wo.reshape(wo.shape[0], -1)
    Cc = wqkv.shape[1]
    if Cc not in (64, 128) or tuple(wqkv.shape) != (384, Cc) or tuple(wo.shape) != (Cc, 128):
        raise ValueError(f"pack_linattn_f16: to_qkv (384, C) and to_out (C, 128), C 64 or 128 (got {tuple(wqkv.shape)}, {tuple(wo.shape)})")
    a = wqkv[:256].reshape(2, 4, 32, Cc // 16, 2, 8).permute(0, 1, 3, 4, 2, 5)         # [mat][head][d][s][lh][j] -> [mat][head][s][lh][d][j]
    return a.reshape(-1).half().view(torch.float32)


def pack_tattn_x3(wqkv, wo):
    """bf16 buffer of the temporal-attention weights for sdc_tattn_block_x3 (include/sdc.h; host twin of sdc_pack_tattn_x3, bit for bit)
    from the nn.Linear weights to_qkv (384, 64) and to_out (64, 128): Wb[head][piece][e], e < 8192 -- position e of a head in
    pack_tattn_f16's fragment order (its 6144 q / k / v values [mat][s][lane][j], then its 2048 to_out values [i][s][lane][j]), the
    three planes holding the exact three-way split of the fp32 weight (h + m + l == w); returned as the float32 words that hold it"""
    wqkv, wo = wqkv.to(torch.float32), wo.to(torch.float32)
    if tuple(wqkv.shape) != (384, 64) or tuple(wo.shape) != (64, 128):
        raise ValueError(f"pack_tattn_x3: to_qkv (384, 64) and to_out (64, 128) (got {tuple(wqkv.shape)}, {tuple(wo.shape)})")
    a = wqkv.reshape(3, 4, 32, 4, 2, 8).permute(1, 0, 3, 4, 2, 5)                   # [mat][head][d][s][lh][j] -> [head][mat][s][lh][d][j]
    b = wo.reshape(2, 32, 4, 2, 2, 2, 4).permute(2, 0, 3, 5, 1, 4, 6)               # (pack_tattn_f16) -> [head][i][s][lh][l31][jh][jl]
    z = torch.cat([a.reshape(4, -1), b.reshape(4, -1)], 1)                         # [head][e]
    return torch.stack(split3_bf16(z), 1).reshape(-1).view(torch.float32)


def pack_gemm_x3(wp, cout, cin, k):
    """bf16 buffer of a strided (1,4,4), sub-pixel (1,2,2) or 1x1x1 conv weight for sdc_conv_gemm_x3 (include/sdc.h; host twin of
    sdc_pack_gemm_x3, bit for bit) from the conv's Wp [taps * Cin][Cout] (pack_conv_weight at precision 0; for a sub-pixel conv the merged
    sub-filter of its parity): three planes Wb[piece][co // 64][stage][block * taps + tap][co % 64][ci % 16], ci = (stage * NCB + block) *
    16 + ci % 16 with NCB = 1 / 2 / 4 channel blocks per stage for 4x4 / 2x2 / 1x1 taps, holding the exact three-way split of the fp32
    weight (h + m + l == w); returned as the float32 words that hold it"""
    k = tuple(k)[-2:]
    ncb = {(4, 4): 1, (2, 2): 2, (1, 1): 4}.get(k, 0)
    taps = k[0] * k[1]
    if ncb == 0 or cout <= 0 or cout % 64 or cin <= 0 or cin % (16 * ncb) or tuple(wp.shape) != (taps * cin, cout):
        raise ValueError(f"pack_gemm_x3: taps 4x4, 2x2 or 1x1, Cout % 64 == 0, Cin % {16 * max(ncb, 1)} == 0, Wp [taps * Cin][Cout] "
                         f"(got taps {k}, Cin {cin}, Cout {cout}, Wp {tuple(wp.shape)})")
    z = wp.to(torch.float32).reshape(taps, cin // (16 * ncb), ncb, 16, cout // 64, 64)      # [tap][stage][block][c16][m tile][co]
    z = z.permute(4, 1, 2, 0, 5, 3).contiguous()                                             # [m tile][stage][block][tap][co][c16]
    return torch.stack(split3_bf16(z)).reshape(-1).view(torch.float32)


def pack_wino3_x3(wp4, cout, cin):
    """bf16 buffer of a 3x3x3 conv weight for sdc_conv_wino3_x3 (include/sdc.h; host twin of sdc_pack_wino3_x3, bit for bit) from the conv's
    precision-4 buffer wp4 (pack_conv_weight at precision 4; cin = Cin0 + Cin1), whose last part is U3[jd][ci][co][j * 4 + xi]: three planes
    Wb[piece][co // 64][jd][ci // 16][j][xi][co % 64][(ci % 16) ^ 8 * ((co >> 3) & 1)] -- the two channel octets of a row swap places in
    rows 8-15 of every 16 (conflict-free fragment reads) -- holding the exact three-way split of the fp32 Winograd taps (h + m + l == u);
    returned as the float32 words that hold it"""
    n = 64 * cin * cout
    if cout <= 0 or cout % 64 or cin <= 0 or cin % 16 or wp4.dim() != 1 or wp4.numel() != (27 + 36 + 48 + 64) * cin * cout:
        raise ValueError(f"pack_wino3_x3: Cout % 64 == 0, Cin % 16 == 0, the flat precision-4 buffer of a 3x3x3 conv "
                         f"(got Cin {cin}, Cout {cout}, {tuple(wp4.shape)})")
    u3 = wp4[-n:].to(torch.float32).reshape(4, cin // 16, 16, cout // 64, 64, 4, 4)         # [jd][stage][c16][m tile][co][j][xi]
    # [m tile][jd][stage][j][xi][co / 16][(co / 8) % 2][co % 8][octet][c8]; rows 8-15 of every 16: the octets swapped
    z = u3.permute(3, 0, 1, 5, 6, 4, 2).reshape(cout // 64, 4, cin // 16, 4, 4, 4, 2, 8, 2, 8)
    z = torch.stack((z[:, :, :, :, :, :, 0], z[:, :, :, :, :, :, 1].flip(-2)), 6).contiguous()
    return torch.stack(split3_bf16(z)).reshape(-1).view(torch.float32)


def split3_bf16(x):
    """the exact three-way bf16 split of a finite fp32 tensor: (h, m, l) bfloat16 with h + m + l == x (RNE conversions, exact residuals)"""
    h = x.bfloat16()
    r = x - h.float()
    m = r.bfloat16()
    return h, m, (r - m.float()).bfloat16()


def conv_precision(n, k, cin, cout, f16=None, train=False):
    """SdcConvDesc.precision for a packed conv weight of n floats (sizes: sdc_pack_conv_weight_floats): the lowest fp32 layout code
    0, 2, 3, 4, 5 whose size matches -- a 1x1x3 buffer packed at 2, 3 or 4 reads as 2, a 3x3 one packed at 3 or 4 as 3 (the same
    buffer).  f16 = 6 / 7: a sampler plan at that precision claims the buffers that carry precision 6's fp16 tail; with train, the
    fine-tuning step's precision-8 buffer (grad_ops.pack_conv_weight), every one of which reads at f16."""
    floats = functools.partial(_lib.get_lib().sdc_pack_conv_weight_floats, cout, cin, *k)
    if train:
        assert f16 in (6, 7) and n == floats(8), (f16, n, k, cin, cout)
        return f16
    if f16 in (6, 7) and f16_kc(k) > 0 and n == floats(6):
        return f16
    code = next((p for p in (0, 2, 3, 4, 5) if n == floats(p)), None)
    assert code is not None, (n, k, cin, cout)
    return code


def conv_desc(x, x1, out, residual, cout, k, stride, pad, up, up_mode, precision):
    """SdcConvDesc of a conv of the 5-D views x (and x1, channel-concatenated) into out (include/sdc.h), strides from the views"""
    d = SdcConvDesc()
    d.B, d.Cin0, d.iD, d.iH, d.iW = x.shape
    d.Cin1, d.Cout = (0 if x1 is None else x1.shape[1]), cout
    d.oD, d.oH, d.oW = out.shape[2:]
    d.kD, d.kH, d.kW = k
    d.sD, d.sH, d.sW = stride
    d.pD, d.pH, d.pW = pad
    d.uD, d.uH, d.uW = up
    d.up_mode, d.precision = up_mode, precision
    d.x0s[:] = _s5(x)
    d.x1s[:] = _s5(x1) if x1 is not None else (0,) * 5
    d.ys[:] = _s5(out)
    d.rs[:] = _s5(residual) if residual is not None else (0,) * 5
    return d


# The switches of a sampler plan that send calls to an alternate kernel: keyword arguments of Plan (documented there), attributes of
# the nets with the same names (unet.py), part of the nets' plan cache key in this order.
PLAN_SWITCHES = ("stem_f16", "stem_split", "gemm_split", "attn_f16", "wino_split", "attn_split", "linattn_f16")

# An unpacked conv weight for Plan.conv: w = the nn weight tensor or a callable returning it, kind as for pack_conv_weight.
WeightSrc = collections.namedtuple("WeightSrc", "w kind", defaults=("conv",))

ConvRoute = collections.namedtuple("ConvRoute", "switch ok fn taps precision x1 gn splitk pack")
# The alternate conv kernels of Plan.conv, in priority order.  A conv with a residual never takes one.  To add a route: one entry here,
# one name in PLAN_SWITCHES (with its Plan keyword and net attribute), the prototypes of its entry points in _lib.py.
#   switch     Plan attribute that enables it, after the constructor's gating
#   ok, fn     coverage query and launch entry points of the library
#   taps       kind -> tap pre-filter; a kind not named never takes the route
#   precision  SdcConvDesc.precision of its descriptor
#   x1         takes a second, channel-concatenated input (its entry point then has the x1 argument)
#   gn         with gn_groups: "ignore" routes and registers no partial sums | "decline" does not route | "sums" routes and registers
#              its epilogue sums like sdc_conv_gn (its entry point then has the partial-sum and group-count arguments)
#   splitk     yields to sdc_conv_splitk under split_small_grids
#   pack       its buffer from the unpacked weight
CONV_ROUTES = (
    # the 7-tap stem convs: the stem kernels sum no GroupNorm statistics (gn_silu takes its own pass) and do not split K
    ConvRoute(switch="stem_f16", ok="sdc_conv_stem_f16_ok", fn="sdc_conv_stem_f16", taps={"conv": lambda k: k[2] == 7}, precision=0,
              x1=False, gn="ignore", splitk=False, pack=lambda w, kind, cout, cin, k: pack_stem_f16(w)),
    ConvRoute(switch="stem_split", ok="sdc_conv_stem_x3_ok", fn="sdc_conv_stem_x3", taps={"conv": lambda k: k[2] == 7}, precision=0,
              x1=False, gn="ignore", splitk=False, pack=lambda w, kind, cout, cin, k: pack_stem_x3(w)),
    # the strided (1,4,4) and 1x1x1 convs and the sub-pixel parities of conv_transpose_422; never "unshuffle", "convT" or "up2_sub", whose
    # 2x2 / merged-tap descriptors the coverage query alone would not keep out.  A conv whose GroupNorm sums the fp32 epilogue can
    # carry keeps the fp32 kernels
    ConvRoute(switch="gemm_split", ok="sdc_conv_gemm_x3_ok", fn="sdc_conv_gemm_x3",
              taps={"conv": lambda k: k in ((1, 4, 4), (1, 1, 1)), "convT_sub": lambda k: k == (1, 2, 2)}, precision=0,
              x1=False, gn="decline", splitk=True,
              pack=lambda w, kind, cout, cin, k: pack_gemm_x3(pack_conv_weight(w, kind, 0), cout, cin, k)),
    # the 3x3x3 convs in precision 4's F(2x2x2,3x3x3) form, GroupNorm sums in the epilogue included
    ConvRoute(switch="wino_split", ok="sdc_conv_wino3_x3_ok", fn="sdc_conv_wino3_x3", taps={"conv": lambda k: k == (3, 3, 3)}, precision=4,
              x1=True, gn="sums", splitk=True,
              pack=lambda w, kind, cout, cin, k: pack_wino3_x3(pack_conv_weight(w, "conv", 4), cout, cin)),
)
assert all(r.switch in PLAN_SWITCHES for r in CONV_ROUTES)


class Pool:
    """Size-keyed free list so that activation buffers are reused along the plan."""

    def __init__(self, device):
        self.device = device
        self.free = {}
        self.all = []
        self.bytes = 0

    def get(self, shape):
        n = int(math.prod(shape))
        lst = self.free.get(n)
        if lst:
            return lst.pop().view(shape)
        t = torch.empty(n, dtype=torch.float32, device=self.device)
        self.all.append(t)
        self.bytes += n * 4
        return t.view(shape)

    def put(self, t):
        self.free.setdefault(t.numel(), []).append(t.reshape(-1))


class Plan:
    """Recorded kernel calls; `run(stream)` replays them (the samplers capture that replay into a hipGraph)."""

    def __init__(self, device, precision=0, stem_f16=False, stem_split=False, gemm_split=False, attn_f16=False, wino_split=False,
                 attn_split=False, linattn_f16=False):
        self.device = torch.device(device)
        self.lib = _lib.get_lib()
        # conv algorithm (include/sdc.h): 0 direct fp32 MFMA | 2 fp32 Winograd F(2,3) along W | 3 F(2x2,3x3) over (H, W) where
        # covered, else as 2 | 4 (default of the nets) F(2x2x2,3x3x3) over (D, H, W) where covered, else as 3 | 5 (opt-in) as 4,
        # with F(4,3) along W for the (1,1,3) convs (Conv1d k3: half the direct MFMA work at 3x the rounding error) | 6 (opt-in,
        # samplers only) as 4, with fp16 operands and fp32 accumulation for the stride-1 pad-1 3-tap convs (csrc/sdc_conv_f16.hip) where
        # the measured dispatch table has the fp16 kernel ahead | 7 (tests, measurement) as 6 on every covered 3-tap conv
        self.precision = int(precision)
        if self.precision not in (0, 2, 3, 4, 5, 6, 7):
            raise ValueError(f"precision must be 0, 2, 3, 4, 5, 6 or 7 (got {precision})")
        # net.stem_f16 (opt-in, samplers only, at any precision): the 7-tap stem convs that sdc_conv_stem_f16_ok covers run
        # conv_stem_f16_kernel (fp16 operands, fp32 accumulation; csrc/sdc_conv_stem_f16.hip) on a buffer of their own
        # (pack_stem_f16); every other conv, and every conv with the switch off, is recorded exactly as without it
        self.stem_f16 = bool(stem_f16)
        # net.stem_split (the nets' default at precision >= 4, samplers only; off for a Plan built directly): the same stems run
        # conv_stem_x3_kernel -- fp32 products formed on the bf16 matrix pipe from exact three-way operand splits, fp32 accumulation
        # (csrc/sdc_conv_stem_x3.hip) -- on their pack_stem_x3 buffer.  Precision 0, 2 and 3 keep the literal fp32 pipe; stem_f16 wins
        self.stem_split = bool(stem_split) and self.precision >= 4 and not self.stem_f16
        # net.gemm_split (the nets' default at precision >= 4, samplers only; off for a Plan built directly): the strided (1,4,4), the
        # sub-pixel (1,2,2) convs of conv_transpose_422 and the 1x1x1 convs that sdc_conv_gemm_x3_ok lists -- covered by
        # conv_gemm_x3_kernel (csrc/sdc_conv_gemm_x3.hip: the stem_split arithmetic) and measured faster than the fp32 kernel -- run it on
        # their pack_gemm_x3 buffer.  Precision 0, 2 and 3 keep the literal fp32 pipe
        self.gemm_split = bool(gemm_split) and self.precision >= 4
        # net.wino_split (the nets' switch at precision >= 4, samplers only; off for a Plan built directly): the 3x3x3 convs that
        # sdc_conv_wino3_x3_ok lists -- covered by conv_wg3_x3_kernel (csrc/sdc_conv_wino_x3.hip: precision 4's Winograd F(2x2x2,3x3x3)
        # with the stem_split arithmetic) and measured faster than the fp32 kernel -- run it on their pack_wino3_x3 buffer, GroupNorm
        # sums in the epilogue included.  Precision 0, 2 and 3 keep the literal fp32 pipe, 6 and 7 their fp16 kernels and today's calls
        self.wino_split = bool(wino_split) and self.precision in (4, 5)
        # net.attn_f16 (opt-in, samplers only, at any precision): the fused temporal-attention block (Plan.tattn_block) runs
        # ta_block_f16_kernel (fp16 operands, fp32 accumulation; csrc/sdc_tablock_f16.hip) on a buffer of its own (pack_tattn_f16);
        # everything else, and every call with the switch off, is recorded exactly as without it
        self.attn_f16 = bool(attn_f16)
        # net.attn_split (the nets' switch at precision 4 and 5, samplers only; off for a Plan built directly): the fused temporal-
        # attention sites that sdc_tattn_block_x3_ok lists -- measured faster than the fp32 block -- run ta_block_x3_kernel
        # (csrc/sdc_tablock_x3.hip: the weight products with the stem_split arithmetic, the rest with the fp32 block's instructions) on
        # their pack_tattn_x3 buffer.  Every other precision keeps today's calls; attn_f16 wins
        self.attn_split = bool(attn_split) and self.precision in (4, 5) and not self.attn_f16
        # net.linattn_f16 (opt-in, samplers only, at any precision): the fused LinearAttention block (Plan.linattn_block) runs the
        # la16_* kernels (fp16 operands, fp32 accumulation; csrc/sdc_lablock_f16.hip) on a buffer of its own (pack_linattn_f16) where
        # sdc_linattn_block_f16_ok lists the site; everything else, and every call with the switch off, is recorded exactly as without it
        self.linattn_f16 = bool(linattn_f16)
        self.calls = []          # (fn, args, keepalive)
        self.pool = Pool(self.device)
        self.keep = []           # descriptors / tensors that must outlive the plan
        self.repackers = []      # (dst tensor, fn() -> src tensor) to refresh repacked weights
        self._stats = None
        self._ctx = None
        self._gn_parts = {}      # out.data_ptr() -> (partial-sum buffer, parts per (sample, group), groups) left by sdc_conv_gn
        self.fuse_gn_stats = True    # False: separate statistics pass after every conv (A/B checks)
        self.fuse_gn_small = True    # False: small groups take the three-launch path (partial, finalize, apply)
        self.split_small_grids = False   # True: sdc_conv_splitk where a conv's grid leaves most CUs idle (net.split_small_grids)

    # ------------------------------------------------------------------ execution
    def run(self, stream):
        for fn, args in self.calls:
            rc = fn(*args, stream)
            if rc:
                check(rc, fn.__name__)

    def refresh_weights(self):
        """Re-run every weight repack (after an optimiser step / load_state_dict)."""
        with torch.no_grad():
            for dst, fn in self.repackers:
                dst.copy_(fn())

    # ------------------------------------------------------------------ scratch
    def _stats_buf(self, B, G):
        need = int(self.lib.sdc_gn_stats_bytes(B, G))
        if self._stats is None or self._stats.numel() * 4 < need:
            self._stats = torch.empty((need + 3) // 4, dtype=torch.float32, device=self.device)
            self.keep.append(self._stats)
        return self._stats

    def _ctx_buf(self, n):
        if self._ctx is None or self._ctx.numel() < n:
            self._ctx = torch.empty(n, dtype=torch.float32, device=self.device)
            self.keep.append(self._ctx)
        return self._ctx

    def _emit(self, fn, *args):
        self.calls.append((fn, args))

    # ------------------------------------------------------------------ weights
    def packed(self, src_fn):
        """Register a repacked weight: src_fn() -> tensor in kernel layout; refreshed by refresh_weights()."""
        with torch.no_grad():
            w = src_fn().detach().to(self.device, torch.float32).contiguous().clone()
        self.repackers.append((w, lambda: src_fn().detach().to(self.device, torch.float32)))
        self.keep.append(w)
        return w

    def conv_weight(self, w, kind="conv"):
        """Register the kernel layout of a conv weight (pack_conv_weight), refreshed by refresh_weights()."""
        return self.packed(lambda: pack_conv_weight(_val(w), kind, self.precision))

    def stem_weight(self, w, pack=pack_stem_f16):
        """Register the 16-bit buffer of a covered stem conv weight (pack_stem_f16 / pack_stem_x3), refreshed by refresh_weights()."""
        return self.packed(lambda: pack(_val(w)))

    def vec(self, p):
        return self.packed(lambda: _val(p).reshape(-1))

    # ------------------------------------------------------------------ stages
    def _gn_partials(self, d, out, gn_groups):
        """Partial-sum buffer for a conv whose epilogue sums the statistics of the GroupNorm over `out` that follows (sdc_conv_gn,
        sdc_conv_wino3_x3), registered for the gn_silu call on `out`; None where the kernel of descriptor d cannot sum them."""
        nparts = int(self.lib.sdc_conv_gnparts(C.byref(d), gn_groups)) if (gn_groups and self.fuse_gn_stats) else 0
        if nparts <= 0:
            return None
        parts = torch.empty(d.B * gn_groups * nparts * 2, dtype=torch.float64, device=self.device)
        self.keep.append(parts)
        self._gn_parts[out.data_ptr()] = (parts, nparts, gn_groups)
        return parts

    def conv(self, x, w, bias, cout, k, *, x1=None, stride=(1, 1, 1), pad=(0, 0, 0), up=(1, 1, 1), up_mode=0,
             residual=None, out=None, gn_groups=0):
        """x (and optional x1, channel-concatenated) are 5-D views; returns out (B,cout,oD,oH,oW).
        w: the conv's packed buffer (conv_weight), or a WeightSrc -- the unpacked weight and its kind.  Only a WeightSrc can take one of
        CONV_ROUTES: the first route whose switch is on and whose fields and `_ok` entry point accept the conv records its kernel on
        its own buffer, and the fp32 buffer (pack_conv_weight at the plan's precision) is packed only when no route takes the conv.
        gn_groups > 0: a GroupNorm over `out` follows -- where the conv epilogue can sum its statistics (sdc_conv_gn, sdc_conv_wino3_x3)
        the partial sums are kept for the gn_silu call on `out`, which then skips its own pass over the tensor."""
        B, c0, iD, iH, iW = x.shape
        c1 = 0 if x1 is None else x1.shape[1]

        def osz(i, u, kk, s, p):
            v = (i - 1) * u + 1 if up_mode else i * u
            return (v + 2 * p - kk) // s + 1

        o = tuple(osz(i, u, kk, s, p) for i, u, kk, s, p in zip((iD, iH, iW), up, k, stride, pad))
        if out is None:
            out = self.pool.get((B, cout, *o))
        else:
            # a caller-sized output may differ from the symmetric-padding size by a one-sided margin (include/sdc.h); the
            # library validates it
            assert tuple(out.shape[:2]) == (B, cout) and out.dim() == 5, (out.shape, (B, cout, *o))
            o = tuple(out.shape[2:])
        if isinstance(w, WeightSrc):
            src = w
            kname = src.kind[0] if isinstance(src.kind, tuple) else src.kind
            for r in CONV_ROUTES:
                if not (getattr(self, r.switch) and residual is None and (x1 is None or r.x1) and not (gn_groups and r.gn == "decline")
                        and kname in r.taps and r.taps[kname](tuple(k))):
                    continue
                d = conv_desc(x, x1, out, None, cout, k, stride, pad, up, up_mode, r.precision)
                if not getattr(self.lib, r.ok)(C.byref(d)) or (r.splitk and self.split_small_grids and
                                                                self.lib.sdc_conv_splitk_bytes(C.byref(d))):
                    continue
                wb = self.packed(lambda: r.pack(_val(src.w), src.kind, cout, c0 + c1, k))
                self.keep += [d, x, x1, wb, bias, out]
                parts = self._gn_partials(d, out, gn_groups) if r.gn == "sums" else None
                self._emit(getattr(self.lib, r.fn), C.byref(d), _ptr(x), *([_ptr(x1)] if r.x1 else []), _ptr(wb), _ptr(bias), _ptr(out),
                           *([_ptr(parts), gn_groups if parts is not None else 0] if r.gn == "sums" else []))
                return out
            w = self.conv_weight(src.w, src.kind)
        prec = conv_precision(w.numel(), k, c0 + c1, cout, f16=self.precision)
        d = conv_desc(x, x1, out, residual, cout, k, stride, pad, up, up_mode, prec)
        if residual is not None:
            assert tuple(residual.shape) == tuple(out.shape)
        self.keep += [d, x, x1, w, bias, residual, out]     # the call list holds raw pointers only
        if self.split_small_grids and residual is None:
            # a grid that leaves most of the chip idle (small batch, deep level): Cin split over several workgroups per tile.  The
            # statistics of a following GroupNorm then come from its own kernel (these tensors are small: sdc_gn_fused)
            nsplit = int(self.lib.sdc_conv_splitk_bytes(C.byref(d)))
            if nsplit:
                work = torch.empty(nsplit // 4, dtype=torch.float32, device=self.device)
                self.keep.append(work)
                self._emit(self.lib.sdc_conv_splitk, C.byref(d), _ptr(x), _ptr(x1), _ptr(w), _ptr(bias), _ptr(out), _ptr(work), nsplit)
                return out
        parts = self._gn_partials(d, out, gn_groups)
        if parts is not None:
            self._emit(self.lib.sdc_conv_gn, C.byref(d), _ptr(x), _ptr(x1), _ptr(w), _ptr(bias), _ptr(residual), _ptr(out),
                       _ptr(parts), gn_groups)
            return out
        self._emit(self.lib.sdc_conv, C.byref(d), _ptr(x), _ptr(x1), _ptr(w), _ptr(bias), _ptr(residual), _ptr(out))
        return out

    def conv_transpose_422(self, x, w, bias, cout):
        """nn.ConvTranspose3d(C, cout, (1,4,4), (1,2,2), (0,1,1)) as four 2x2 stride-1 convs, one per output parity,
        each writing its quarter of the output through strides (conv3d.py:159-160).  The zero-stuffed form spends
        3/4 of its MFMA work on inserted zeros."""
        B, c0, iD, iH, iW = x.shape
        out = self.pool.get((B, cout, iD, 2 * iH, 2 * iW))
        for ph in (0, 1):
            for pw in (0, 1):
                self.conv(x, WeightSrc(w, ("convT_sub", ph, pw)), bias, cout, (1, 2, 2), pad=(0, 1 - ph, 1 - pw),
                          out=out[:, :, :, ph::2, pw::2])
        return out

    def upsample2_conv3(self, x, w, bias, cout):
        """nn.Upsample(scale_factor=2, mode='nearest') + Conv2d(3x3, pad 1) (1D/model/unet.py:33-37) as four 2x2 convs of the
        low-resolution input, one per output parity, with the taps that land on the same source pixel merged."""
        B, c0, iD, iH, iW = x.shape
        out = self.pool.get((B, cout, iD, 2 * iH, 2 * iW))
        for ph in (0, 1):
            for pw in (0, 1):
                self.conv(x, WeightSrc(w, ("up2_sub", ph, pw)), bias, cout, (1, 2, 2), pad=(0, 1 - ph, 1 - pw),
                          out=out[:, :, :, ph::2, pw::2])
        return out

    def gn_silu(self, x, gamma, beta, groups, *, ss=None, t_dev=None, ss_t_stride=0, ss_b_stride=0, ss_off=0,
                residual=None, out=None, eps=1e-5):
        """GroupNorm -> (scale+1, shift) -> SiLU (+ residual); x contiguous 5-D; in place by default."""
        assert x.is_contiguous()
        B, Cc = x.shape[0], x.shape[1]
        S = x.numel() // (B * Cc)
        st = self._stats_buf(B, groups)
        out = x if out is None else out
        self.keep += [x, gamma, beta, ss, t_dev, residual, out]
        fused = self._gn_parts.pop(x.data_ptr(), None)
        if fused is not None and fused[2] == groups:
            self._emit(self.lib.sdc_gn_finalize, _ptr(fused[0]), _ptr(st), B, groups, fused[1], (Cc // groups) * S, eps)
        elif self.fuse_gn_small and self.lib.sdc_gn_fused_ok(B, Cc, groups, S):
            # small groups without conv-epilogue sums (the deep levels of the 1-D nets): statistics + apply in one launch
            # (argument positions 3.. match sdc_gn_apply's 4..: bind_cond patches either form)
            self._emit(self.lib.sdc_gn_fused, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(ss), _ptr(t_dev), ss_t_stride, ss_b_stride,
                       ss_off, _ptr(residual), _ptr(out), B, Cc, groups, S, eps)
            return out
        else:
            self._emit(self.lib.sdc_gn_stats, _ptr(x), _ptr(st), B, Cc, groups, S, eps)
        self._emit(self.lib.sdc_gn_apply, _ptr(x), _ptr(st), _ptr(gamma), _ptr(beta), _ptr(ss), _ptr(t_dev),
                   ss_t_stride, ss_b_stride, ss_off, _ptr(residual), _ptr(out), B, Cc, groups, S)
        return out

    def chan_norm(self, x, g, mode, *, residual=None, out=None, eps=1e-5):
        assert x.is_contiguous()
        B, Cc = x.shape[0], x.shape[1]
        S = x.numel() // (B * Cc)
        if out is None:
            out = self.pool.get(tuple(x.shape))
        self.keep += [x, g, residual, out]
        self._emit(self.lib.sdc_chan_norm, _ptr(x), _ptr(g), _ptr(residual), _ptr(out), B, Cc, S, mode, eps)
        return out

    def act(self, x, kind, out=None):
        out = x if out is None else out
        self.keep += [x, out]
        self._emit(self.lib.sdc_act, _ptr(x), _ptr(out), x.numel(), kind)
        return out

    def linattn(self, qkv, heads, outer, inner, n, q_strides, out, o_strides):
        ctx = self._ctx_buf(outer * inner * heads * 32 * 32)
        self.keep += [qkv, out]
        self._emit(self.lib.sdc_linattn, _ptr(qkv), _ptr(ctx), _ptr(out), outer, inner, heads, n, *q_strides, *o_strides)
        return out

    def gn_stats_deferred(self, x, groups, eps=1e-5):
        """GroupNorm statistics of x -- (mean, rstd) per (sample, group) -- WITHOUT the apply pass: the consumer
        (linattn_block(..., gn=...)) normalises, activates and adds the residual while it loads its tiles."""
        assert x.is_contiguous()
        B, Cc = x.shape[0], x.shape[1]
        S = x.numel() // (B * Cc)
        # its own buffer (read two launches later), sized like _stats_buf: sdc_gn_stats keeps its fp64 partials behind the (mean, rstd) pairs
        st = torch.empty((int(self.lib.sdc_gn_stats_bytes(B, groups)) + 3) // 4, dtype=torch.float32, device=self.device)
        self.keep += [x, st]
        fused = self._gn_parts.pop(x.data_ptr(), None)
        if fused is not None and fused[2] == groups:
            self._emit(self.lib.sdc_gn_finalize, _ptr(fused[0]), _ptr(st), B, groups, fused[1], (Cc // groups) * S, eps)
        else:
            self._emit(self.lib.sdc_gn_stats, _ptr(x), _ptr(st), B, Cc, groups, S, eps)
        return st

    def gn_apply_deferred(self, x, gn):
        """the apply pass of a GroupNorm whose statistics gn_stats_deferred took: x <- SiLU(GN(x)) (+ residual), in place"""
        st, gamma, beta, groups, res = gn
        B, Cc = x.shape[0], x.shape[1]
        S = x.numel() // (B * Cc)
        self.keep += [x, st, gamma, beta, res]
        self._emit(self.lib.sdc_gn_apply, _ptr(x), _ptr(st), _ptr(gamma), _ptr(beta), 0, 0, 0, 0, 0, _ptr(res), _ptr(x), B, Cc, groups, S)
        return x

    def gn_pointwise_out(self, x, gn, w, bias, out):
        """final_conv on the RAW conv output x of the last ResnetBlock: gn = (stats, gamma, beta, groups, residual) as handed out by
        resnet(defer_gn=True); GroupNorm apply + SiLU + residual happen on the kernel's loads (sdc_gn_pointwise_out).  w = the conv
        weight (Cout, C) flat, out a 5-D view whose (H, W) planes are dense.  None when the shape is outside the kernel's contract."""
        st, gamma, beta, groups, res = gn
        B, Cc = x.shape[0], x.shape[1]
        S = x.numel() // (B * Cc)
        cout = out.shape[1]
        plane = out.shape[3] * out.shape[4]
        ys = _s5(out)
        # (a thread walks all C channels of its four positions: worth it where a sample has >= 1024 positions -- the tokamak net's 128
        # positions per sample leave one 32-lane block per sample on a 256-channel walk: 150 us against ~30 for the two small kernels)
        ok = (x.is_contiguous() and (res is None or res.is_contiguous()) and cout <= 16 and Cc % 4 == 0 and Cc <= 2048 and S >= 1024 and plane % 4 == 0 and ys[4] == 1 and
              ys[3] == out.shape[4] and all(v % 4 == 0 for v in ys[:3]) and out.data_ptr() % 16 == 0 and
              tuple(out.shape[2:]) == tuple(x.shape[2:]))
        if not ok:
            return None
        self.keep += [x, st, gamma, beta, res, w, bias, out]
        self._emit(self.lib.sdc_gn_pointwise_out, _ptr(x), _ptr(st), _ptr(gamma), _ptr(beta), _ptr(res), _ptr(w), _ptr(bias), _ptr(out),
                   B, Cc, groups, cout, S, plane, ys[0], ys[1], ys[2])
        return out

    def linattn_f16_routes(self, Cc, n):
        """True where net.linattn_f16 sends a fused LinearAttention site of width Cc and n tokens per sequence to
        sdc_linattn_block_f16 / _gn_f16: the switch is on and the library lists the site (never the batch)"""
        return self.linattn_f16 and bool(self.lib.sdc_linattn_block_f16_ok(int(Cc), int(n)))

    def linattn_block(self, x, g_pre, wqkv, wo, bo, g_post, outer, inner, n, strides, pre_mode, post_mode, eps=1e-5, gn=None, w16=None):
        """Residual(PreNorm(LinearAttention)) in one call (dim 64 / 128, n % 64 == 0); returns y shaped like x.
        gn = (stats, gamma, beta, groups, residual): x is the RAW conv output of the producing ResnetBlock, whose GroupNorm +
        SiLU + residual add is applied on load (sdc_linattn_block_gn); `outer` must then be the batch axis.
        w16 = the UNPACKED weights (to_qkv (384, C), to_out (C, 128)) or callables returning them: where linattn_f16_routes() lists
        the site the call recorded is sdc_linattn_block_f16 / sdc_linattn_block_gn_f16 on their pack_linattn_f16 buffer (wqkv and wo,
        the fp32 packed weights, still serve its fp32 middle launch)."""
        Cc = x.shape[1]
        y = self.pool.get(tuple(x.shape))
        f16 = w16 is not None and self.linattn_f16_routes(Cc, n)
        if f16:
            wpk = self.packed(lambda: pack_linattn_f16(_val(w16[0]), _val(w16[1])))
            nwork = (int(self.lib.sdc_linattn_block_f16_bytes(outer, inner, Cc, n)) + 3) // 4
        else:
            wpk, nwork = None, int(self.lib.sdc_linattn_block_bytes(outer, inner, Cc, n)) // 4
        work = torch.empty(nwork, dtype=torch.float32, device=self.device)
        self.keep += [x, g_pre, wqkv, wo, wpk, bo, g_post, work, y]
        head = [_ptr(x)]
        if gn is not None:
            st, gamma, beta, groups, res = gn
            assert outer == x.shape[0] and (res is None or (tuple(res.shape) == tuple(x.shape) and res.stride() == x.stride()))
            self.keep += [st, gamma, beta, res]
            head += [_ptr(st), _ptr(gamma), _ptr(beta), groups, _ptr(res)]
        fn = ((self.lib.sdc_linattn_block, self.lib.sdc_linattn_block_f16),
              (self.lib.sdc_linattn_block_gn, self.lib.sdc_linattn_block_gn_f16))[gn is not None][f16]
        self._emit(fn, *head, _ptr(g_pre), _ptr(wqkv), _ptr(wo), *([_ptr(wpk)] if f16 else []), _ptr(bo), _ptr(g_post), _ptr(work), _ptr(y),
                   outer, inner, Cc, n, *strides, pre_mode, post_mode, eps)
        return y

    def tattn_weight(self, wqkv, wo, split=False):
        """Register the fp16 buffer of the temporal-attention weights (pack_tattn_f16; split: the three bf16 planes of pack_tattn_x3)
        from the unpacked nn.Linear weights to_qkv / to_out (tensors or callables returning them), refreshed by refresh_weights()."""
        pack = pack_tattn_x3 if split else pack_tattn_f16
        return self.packed(lambda: pack(_val(wqkv), _val(wo)))

    def tattn_split_routes(self, Cc, Fr, hw):
        """True where net.attn_split sends a fused temporal-attention site of width Cc, Fr frames and hw pixels per sample to
        sdc_tattn_block_x3: the switch is on and the library's measured routing table lists the site (never the batch)"""
        return self.attn_split and bool(self.lib.sdc_tattn_block_x3_ok(int(Cc), int(Fr), int(hw)))

    def tattn_block(self, x, g_pre, wqkv, wo, rot, bias, eps=1e-5):
        """Residual(PreNorm(temporal Attention)) of the smoke net in one launch: x (B, 64, 32, H, W) contiguous.  wqkv, wo: the packed
        [64][384] / [128][64] weights (conv_weight); with Plan.attn_f16 the UNPACKED nn.Linear weights to_qkv (384, 64) / to_out (64, 128)
        (or callables returning them): the call recorded is then sdc_tattn_block_f16 on their pack_tattn_f16 buffer.  The same holds
        for a site that tattn_split_routes() lists: unpacked weights, sdc_tattn_block_x3 on their pack_tattn_x3 buffer."""
        B, Cc, Fr, H, W = x.shape
        assert x.is_contiguous()
        y = self.pool.get(tuple(x.shape))
        if self.tattn_split_routes(Cc, Fr, H * W):
            fn, w = self.lib.sdc_tattn_block_x3, [self.tattn_weight(wqkv, wo, split=True)]
        elif self.attn_f16:
            fn, w = self.lib.sdc_tattn_block_f16, [self.tattn_weight(wqkv, wo)]
        else:
            fn, w = self.lib.sdc_tattn_block, [wqkv, wo]
        self.keep += [x, g_pre, *w, rot, bias, y]
        self._emit(fn, _ptr(x), _ptr(g_pre), *map(_ptr, w), _ptr(rot), _ptr(bias), _ptr(y),
                   B, H * W, Cc, Fr, Cc * Fr * H * W, Fr * H * W, H * W, eps)
        return y

    def attn(self, qkv, out, heads, outer, inner, ntok, q_strides, o_strides, rot=None, bias=None):
        self.keep += [qkv, out, rot, bias]
        self._emit(self.lib.sdc_attn, _ptr(qkv), _ptr(out), _ptr(rot), _ptr(bias), outer, inner, heads, ntok,
                   *q_strides, *o_strides)
        return out
