"""-m gpu: the FORWARD kernels on the launch branches that production sizes take and the small shapes of tests/test_gpu_kernels.py
never reach (the forward twin of tests/test_gpu_grad_paths.py).  Through the C ABI on NaN-filled outputs, inputs drawn on the device
from a seeded generator, against the plain formula in fp64 torch on the device.  Launcher, branch -> test:
  * sdc_chan_norm (eight kernel forms chosen by S and C)
      chan_norm_vec_kernel<32>  (S >= 1024, S % 4 == 0, 128 < C <= 256)     -> test_chan_norm_forms[vec32-*]
      chan_norm_vec_kernel<16>  (..., 256 < C <= 512)                       -> test_chan_norm_forms[vec16-*]
      chan_norm_vec_kernel<64>  (..., C <= 128) with > 1 channel per slice  -> test_chan_norm_forms[vec64-*]
      chan_norm_kernel<64,true> (S >= 1024, S % 4 != 0, C <= 128)           -> test_chan_norm_forms[k64cache-*]
      chan_norm_kernel<64,false> (S >= 1024, S % 4 != 0, C > 128)           -> test_chan_norm_forms[k64loop-*]
      vec<64> and kernel<64,true> give the same bits per position           -> test_chan_norm_vec64_has_the_scalar_forms_bits
      (chan_norm_kernel<16,true>, chan_norm_lds_kernel<16>, chan_norm_kernel<16,false>: test_gpu_kernels.py::test_channel_norms)
  * sdc_gn_apply
      gn_apply_kernel<true,true> (STREAM: B C S 4 >= 512 MiB)               -> test_gn_apply_stream_form
      gn_apply_kernel<true>, grid.y capped at 64, the loop runs 3 times     -> test_gn_apply_stream_form (the single-sample calls)
      gn_apply_flat_kernel past its 4096-block cap (second grid stride)     -> test_gn_apply_flat_form_past_its_grid_cap
      gn_apply_kernel<false> past gx = 64 (second grid stride)              -> test_gn_apply_scalar_form_past_its_grid_cap
  * sdc_act past its 2048-block cap                                         -> test_act_past_its_grid_cap
  * sdc_attn, temporal MFMA kernels
      tattn_kernel<16>, tiles_per_wg = 4 (and 1: every sample alone)        -> test_temporal_attention_tiles_per_workgroup[ns16-tpw4]
      tattn_kernel<8>, tiles_per_wg = 2 (and 1: every sample alone)         -> test_temporal_attention_tiles_per_workgroup[ns8-tpw2]
      (tattn_kernel<16> with 2 tiles: test_gpu_grad.py / test_gpu_kernels.py at (B = 2, inner = 4096))
  * sdc_linattn_block_sel impl 0 / impl 1, sdc_linattn_block_f16: pass 2 with tiles_per_blk = 8 (last workgroup 5 tiles), 3 (last
    workgroup 1 tile) and 2 (every sample alone)                            -> test_linattn_block_pass2_walks_several_tiles
    sdc_linattn_block_gn_sel impl 0, tiles_per_blk = 3                      -> test_linattn_block_gn_pass2_walks_several_tiles
  * sdc_linattn refuses outer inner heads >= 65536 before its first launch  -> test_linattn_core_refuses_before_any_launch
Every shape is the smallest the host code allows for its branch; the arithmetic stands next to it.  _rel is test_gpu_grad._rel's
measure (max |err| over max |ref|) evaluated on the device; the gate is 1e-5 through test_gpu_grad_paths._gate."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import test_gpu_linattn_f16 as LA16
import test_gpu_linattn_x3 as LAX3
from safediffcon_amd import _lib, grad_ops
from test_gpu_grad import DEV, _ref_attention, _rot_table
from test_gpu_grad_paths import _gate

pytestmark = pytest.mark.gpu
NAN = float("nan")
NT = 256            # threads per workgroup of the normalising / activation kernels


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, g, scale=1.0):
    return scale * torch.randn(shape, generator=g, device=DEV, dtype=torch.float32)


def _rel(a, b):
    b = b.double()
    return ((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------ 1. sdc_chan_norm: the forms of long rows
def _chan_norm_form(Cc, S):
    """the dispatch of sdc_chan_norm for rows of S >= 1024 positions"""
    assert S >= 1024
    if S % 4 == 0 and Cc <= 512:
        return "vec64" if Cc <= 128 else ("vec32" if Cc <= 256 else "vec16")
    return "k64cache" if Cc <= 128 else "k64loop"


def _chan_norm_formula(x, g, res, mode):
    gb = g.reshape(1, -1, 1)
    if mode == 0:
        y = (x - x.mean(1, keepdim=True)) * (x.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt() * gb
    else:
        y = F.normalize(x, dim=1) * gb * x.shape[1] ** 0.5
    return y if res is None else y + res


def _chan_norm(x, g, res, mode):
    B, Cc, S = x.shape
    y = torch.full_like(x, NAN)
    _lib.check(_lib.get_lib().sdc_chan_norm(x.data_ptr(), g.data_ptr(), _ptr(res), y.data_ptr(), B, Cc, S, mode, C.c_float(1e-5), _stream()),
               "sdc_chan_norm")
    return y


# a thread of the vec / cached forms holds the channels slice + i NSL, i < 32, NSL = 256 / lanes: lanes x 4 positions per workgroup
CHAN_NORM_FORMS = [
    # (form, B, C, S)
    ("vec32", 2, 256, 1036),        # 8 slices x 32 channels = 256: all registers in use; S / 4 = 259 = 8 * 32 + 3: a last block of 3 lanes
    ("vec32", 2, 192, 1036),        # 24 of the 32 register slots: the `c < C` guards
    ("vec16", 2, 512, 1028),        # 16 slices x 32 channels; S / 4 = 257 = 16 * 16 + 1: a last block of one lane
    ("vec16", 2, 320, 1028),        # 20 of 32 slots
    ("vec64", 2, 128, 1028),        # 4 slices x 32 channels (the C4 case); 257 = 4 * 64 + 1
    ("vec64", 2, 96, 1028),         # 24 of 32 slots
    ("k64cache", 2, 128, 1027),     # S % 4 != 0: 64 scalar position lanes, 1027 = 16 * 64 + 3
    ("k64cache", 2, 72, 1027),      # 18 of 32 slots
    ("k64loop", 2, 160, 1027),      # C > 128: the looping form, 40 channels per slice
]


@pytest.mark.parametrize("with_res", [False, True], ids=["bare", "res"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("form,B,Cc,S", CHAN_NORM_FORMS, ids=[f"{f}-C{c}" for f, _, c, _ in CHAN_NORM_FORMS])
def test_chan_norm_forms(form, B, Cc, S, mode, with_res):
    assert _chan_norm_form(Cc, S) == form
    g = _gen(300 + Cc)
    x, gain = _randn((B, Cc, S), g, 2.0) + 0.7, 1 + _randn((Cc,), g, 0.3)
    res = _randn((B, Cc, S), g) if with_res else None
    ref = _chan_norm_formula(x.double(), gain.double(), None if res is None else res.double(), mode)
    e32 = _rel(_chan_norm_formula(x, gain, res, mode), ref)
    y = _chan_norm(x, gain, res, mode)
    e = _rel(y, ref)
    print(f"[measured] chan_norm {form} mode {mode} {(B, Cc, S)}{' + res' if with_res else ''}: kernel {e:.2e} | fp32 torch {e32:.2e}")
    assert bool(torch.isfinite(y).all())
    assert e < _gate(1e-5, e32)


@pytest.mark.parametrize("Cc", [128, 96, 72])
def test_chan_norm_vec64_has_the_scalar_forms_bits(Cc):
    """chan_norm_vec_kernel<64> (S = 1028) and chan_norm_kernel<64, true> (S = 1027) on the same per-position channel values: both keep
    the channels slice + 4 i of a position in one thread, sum them in the order of i and the four slices in the order of the slice, so
    the first 1027 positions of every row carry the same bits"""
    B = 2
    assert _chan_norm_form(Cc, 1028) == "vec64" and _chan_norm_form(Cc, 1027) == "k64cache"
    g = _gen(340 + Cc)
    x, gain, res = _randn((B, Cc, 1028), g, 2.0) + 0.7, 1 + _randn((Cc,), g, 0.3), _randn((B, Cc, 1028), g)
    cut = lambda t: t[:, :, :1027].contiguous()       # noqa: E731
    for mode in (0, 1):
        for r in (None, res):
            yv = _chan_norm(x, gain, r, mode)
            ys = _chan_norm(cut(x), gain, None if r is None else cut(r), mode)
            assert bool(torch.isfinite(yv).all()) and bool(torch.isfinite(ys).all())
            assert torch.equal(cut(yv), ys), (mode, r is not None)


# ------------------------------------------------------------------ 2. sdc_gn_apply: the STREAM form and the two grid caps
def _gn_stats64(x, G):
    """(B G, 2) float (mean, rstd) pairs from fp64 sums, rounded once: only the apply pass is under test"""
    B = x.shape[0]
    out = torch.empty((B * G, 2), dtype=torch.float32, device=DEV)
    for b in range(B):
        xd = x[b].reshape(G, -1).double()
        out[b * G:(b + 1) * G, 0] = xd.mean(1).float()
        out[b * G:(b + 1) * G, 1] = (xd.var(1, unbiased=False) + 1e-5).rsqrt().float()
    return out


def _gn_row_constants(B, Cc, G, stats, gamma, beta, ss_rows):
    """the constants of every (b, c) row as (B C, 1) columns: mean, rstd, gamma, beta, scale, shift (ss_rows (B, 2 C) or None)"""
    st = stats.view(B, G, 2).repeat_interleave(Cc // G, dim=1)
    cols = [st[..., 0], st[..., 1], gamma.expand(B, Cc), beta.expand(B, Cc)]
    cols += [None, None] if ss_rows is None else [ss_rows[:, :Cc], ss_rows[:, Cc:]]
    return [None if c is None else c.reshape(-1, 1) for c in cols]


def _gn_apply_formula(x2, consts, res2, rows, dtype):
    """y = SiLU(((x - mean) rstd gamma + beta) (scale + 1) + shift) + res on the given rows of the (B C, S) view"""
    mean, rstd, gamma, beta, sc, sh = (None if c is None else c[rows].to(dtype) for c in consts)
    u = (x2[rows].to(dtype) - mean) * rstd * gamma + beta
    if sc is not None:
        u = u * (sc + 1) + sh
    y = F.silu(u)
    return y if res2 is None else y + res2[rows].to(dtype)


def _gn_apply(x, stats, gamma, beta, G, ss=None, t_dev=None, ss_t=0, ss_b=0, ss_off=0, res=None):
    B, Cc = x.shape[0], x.shape[1]
    S = x.numel() // (B * Cc)
    y = torch.full_like(x, NAN)
    _lib.check(_lib.get_lib().sdc_gn_apply(x.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(ss), _ptr(t_dev), ss_t, ss_b,
                                           ss_off, _ptr(res), y.data_ptr(), B, Cc, G, S, _stream()), "sdc_gn_apply")
    return y


def _gn_case(B, Cc, G, S, cond, with_res, seed, t_lut=False):
    """inputs of one sdc_gn_apply case: ss rows of 2 C + 5 floats read from offset 5, through a 3-entry time table when t_lut"""
    g = _gen(seed)
    x = _randn((B, Cc, S), g, 3.0) + 1.5
    gamma, beta = 1 + _randn((Cc,), g, 0.2), _randn((Cc,), g, 0.2)
    res = _randn((B, Cc, S), g) if with_res else None
    kw, ss_rows = {}, None
    if cond:
        W = 2 * Cc + 5
        ss = _randn((3, B, W) if t_lut else (B, W), g, 0.3)
        kw = dict(ss=ss, ss_b=W, ss_off=5)
        ss_rows = ss[:, 5:]
        if t_lut:
            kw.update(t_dev=torch.tensor([2], dtype=torch.int32, device=DEV), ss_t=B * W)
            ss_rows = ss[2, :, 5:]
    stats = _gn_stats64(x, G)
    return x, stats, gamma, beta, res, kw, _gn_row_constants(B, Cc, G, stats, gamma, beta, ss_rows)


@pytest.mark.parametrize("full", [True, False], ids=["ss-t_dev-res", "bare"])
def test_gn_apply_stream_form(full):
    """gn_apply_kernel<true, true>: one 16-byte vector per thread, no loop, nontemporal loads and stores, grid.y from S.  Taken when
    B C S 4 >= 512 MiB: 1024 rows x 131220 floats = 537 477 120 bytes >= 536 870 912 (no smaller tensor reaches it).  S / 4 = 32805
    = 128 * 256 + 37: the last of the 129 blocks of a row has 37 live threads (`si < nv`).  fp64 on eight whole rows (first, last, the
    rows on either side of a sample and of a group boundary); every other row through the single-sample calls: B = 1 is 67 MB, the
    looping form with grid.y = min(129, 64) = 64 -- the form is chosen by the batch, so the bits must not depend on it."""
    B, Cc, G, S = 8, 128, 8, 131220
    assert S % 4 == 0 and S >= 1024 and B * Cc * S * 4 >= 512 << 20 and _cdiv(S // 4, NT) < 65536      # batched: STREAM
    assert (B - 1) * Cc * S * 4 < 512 << 20 and (S // 4) % NT != 0                                      # (B = 7 would not reach it)
    assert Cc * S * 4 < 512 << 20 and _cdiv(S // 4, NT) > 2 * 64                                        # alone: the loop, 3 strides
    x, stats, gamma, beta, res, kw, consts = _gn_case(B, Cc, G, S, full, full, 400, t_lut=True)
    y = _gn_apply(x, stats, gamma, beta, G, res=res, **kw)
    assert bool(torch.isfinite(y).all())
    rows = torch.tensor([0, 1, 127, 128, 511, 640, 1022, 1023], device=DEV)
    x2, r2 = x.view(B * Cc, S), None if res is None else res.view(B * Cc, S)
    ref = _gn_apply_formula(x2, consts, r2, rows, torch.float64)
    e32 = _rel(_gn_apply_formula(x2, consts, r2, rows, torch.float32), ref)
    e = _rel(y.view(B * Cc, S)[rows], ref)
    print(f"[measured] gn_apply STREAM form {(B, Cc, S)} G={G} {'ss + t_dev + res' if full else 'bare'}: kernel {e:.2e} | fp32 torch {e32:.2e}")
    assert e < _gate(1e-5, e32)
    for b in range(B):
        kb = dict(kw)
        if full:
            kb["ss_off"] = kw["ss_off"] + b * kw["ss_b"]
        yb = _gn_apply(x[b:b + 1], stats[b * G:(b + 1) * G], gamma, beta, G, res=None if res is None else res[b:b + 1], **kb)
        assert torch.equal(yb[0], y[b]), b


def test_gn_apply_flat_form_past_its_grid_cap():
    """gn_apply_flat_kernel (S < 1024, 16-byte vectors): 128 * 256 rows x 33 vectors = 1 081 344 > 4096 blocks x 256 threads =
    1 048 576: the first 32768 threads walk a second grid stride (C3 at B = 128); 33 vectors per row put a row boundary inside
    almost every wave"""
    B, Cc, G, S = 128, 256, 8, 132
    assert S % 4 == 0 and S < 1024 and 4096 * NT < B * Cc * (S // 4) < 2 * 4096 * NT
    x, stats, gamma, beta, res, kw, consts = _gn_case(B, Cc, G, S, True, True, 410)
    y = _gn_apply(x, stats, gamma, beta, G, res=res, **kw)
    rows = torch.arange(B * Cc, device=DEV)
    x2, r2 = x.view(B * Cc, S), res.view(B * Cc, S)
    ref = _gn_apply_formula(x2, consts, r2, rows, torch.float64)
    e32 = _rel(_gn_apply_formula(x2, consts, r2, rows, torch.float32), ref)
    e = _rel(y.view(B * Cc, S), ref)
    print(f"[measured] gn_apply flat form past 4096 blocks {(B, Cc, S)} G={G}: kernel {e:.2e} | fp32 torch {e32:.2e}")
    assert bool(torch.isfinite(y).all())
    assert e < _gate(1e-5, e32)


def test_gn_apply_scalar_form_past_its_grid_cap():
    """gn_apply_kernel<false> (S % 4 != 0): grid.y = ceil(16387 / 256) = 65 -> 64, so the threads of block 0 walk a second stride of
    3 elements (4 rows)"""
    B, Cc, G, S = 2, 2, 1, 16387
    assert S % 4 != 0 and 64 < _cdiv(S, NT) and S - 64 * NT == 3
    x, stats, gamma, beta, res, kw, consts = _gn_case(B, Cc, G, S, True, True, 420)
    y = _gn_apply(x, stats, gamma, beta, G, res=res, **kw)
    rows = torch.arange(B * Cc, device=DEV)
    x2, r2 = x.view(B * Cc, S), res.view(B * Cc, S)
    ref = _gn_apply_formula(x2, consts, r2, rows, torch.float64)
    e32 = _rel(_gn_apply_formula(x2, consts, r2, rows, torch.float32), ref)
    e = _rel(y.view(B * Cc, S), ref)
    print(f"[measured] gn_apply scalar form past gx = 64 {(B, Cc, S)} G={G}: kernel {e:.2e} | fp32 torch {e32:.2e}")
    assert bool(torch.isfinite(y).all())
    assert e < _gate(1e-5, e32)


# ------------------------------------------------------------------ 3. sdc_act past its grid cap
@pytest.mark.parametrize("kind", [0, 1], ids=["silu", "gelu"])
def test_act_past_its_grid_cap(kind):
    """2048 blocks x 256 threads = 524 288 < n = 525 065: the first 777 threads walk a second grid stride; values over +-20 (both
    tails of the sigmoid and of erf)"""
    n = 2048 * NT + 777
    assert _cdiv(n, NT) > 2048
    x = torch.rand((n,), generator=_gen(430), device=DEV, dtype=torch.float32) * 40 - 20
    act = F.silu if kind == 0 else F.gelu
    ref = act(x.double())
    e32 = _rel(act(x), ref)
    y = torch.full_like(x, NAN)
    _lib.check(_lib.get_lib().sdc_act(x.data_ptr(), y.data_ptr(), n, kind, _stream()), "sdc_act")
    e = _rel(y, ref)
    print(f"[measured] act kind {kind} n={n}: kernel {e:.2e} | fp32 torch {e32:.2e}")
    assert bool(torch.isfinite(y).all())
    assert e < _gate(1e-5, e32)


# ------------------------------------------------------------------ 4. sdc_attn: the temporal MFMA kernels, several tiles per workgroup
def _tattn_launch(outer, inner, heads):
    """(pixels per tile, tiles, tiles per workgroup) of sdc_attn's MFMA branch (32 frames, frame-strided)"""
    ns = 16 if inner % 16 == 0 else 8
    assert inner % 8 == 0
    nblk = outer * inner // ns * heads
    for t in (4, 2):
        if nblk % (t * 8 * heads) == 0 and nblk // t >= 1024:
            return ns, nblk, t
    return ns, nblk, 1


def _tattn_ref(qkv, bias, heads, dtype):
    """'b c f h w -> b (h w) f c' attention with rotary + relative-position bias on (B, 3 heads 32, F, H, W), the formula of
    test_gpu_grad.py"""
    B, _, Fr, H, W = qkv.shape
    hw = H * W
    ang = _rot_table(Fr)[1].to(DEV).to(dtype)
    q, k, v = (t.reshape(B, heads, 32, Fr, hw).permute(0, 4, 1, 3, 2) for t in qkv.to(dtype).chunk(3, dim=1))     # (B, hw, heads, F, 32)
    o = _ref_attention(q, k, v, ang, bias.to(dtype))
    return o.permute(0, 2, 4, 3, 1).reshape(B, heads * 32, Fr, H, W)


def _tattn(qkv, out, rot, bias, heads):
    outer, ch, Fr = qkv.shape[0], qkv.shape[1], qkv.shape[2]
    inner = qkv.shape[3] * qkv.shape[4]
    _lib.check(_lib.get_lib().sdc_attn(qkv.data_ptr(), out.data_ptr(), rot.data_ptr(), bias.data_ptr(), outer, inner, heads, Fr,
                                       ch * Fr * inner, Fr * inner, 1, inner, heads * 32 * Fr * inner, Fr * inner, 1, inner, _stream()),
               "sdc_attn")
    return out


@pytest.mark.parametrize("heads,outer,sp,want,alone", [
    # the default fine-tuning chain at 64 x 64 and B = 4: nblk = 4 * 4096 / 16 * 4 = 4096, 4096 % (4 * 8 * 4) == 0 and 4096 / 4 >= 1024.
    # tiles_per_wg = 4 needs nblk >= 4096 tiles of 16 sequences: 65 536 head-sequences whatever the split into heads, outer and inner
    # (0.8 GB of qkv).  A sample alone: nblk = 1024, 1024 / 2 < 1024 -> one tile per workgroup, nothing prefetched.
    pytest.param(4, 4, (64, 64), (16, 4096, 4), (16, 1024, 1), id="ns16-tpw4"),
    # inner = 8 (not a multiple of 16): tattn_kernel<8>, nblk = 2048 * 8 / 8 = 2048; 2048 / 4 < 1024; 2048 % (2 * 8) == 0 and
    # 2048 / 2 >= 1024 -> 2.  A sample alone is one tile.
    pytest.param(1, 2048, (2, 4), (8, 2048, 2), (8, 1, 1), id="ns8-tpw2"),
])
def test_temporal_attention_tiles_per_workgroup(heads, outer, sp, want, alone):
    """a workgroup of tattn_kernel walks tiles_per_wg tiles and holds tile t + 1's Q and K in registers while tile t is on the
    matrix cores: against fp64, two runs bit-identical, and every `outer` sample alone (one tile per workgroup: no prefetch) equal
    to its slice of the batched run bit for bit"""
    Fr, inner = 32, sp[0] * sp[1]
    assert _tattn_launch(outer, inner, heads) == want and _tattn_launch(1, inner, heads) == alone
    g = _gen(440 + heads)
    qkv = _randn((outer, 3 * heads * 32, Fr, *sp), g)
    bias = _randn((heads, Fr, Fr), g, 0.5)
    rot = _rot_table(Fr)[0].to(DEV)
    out = _tattn(qkv, torch.full((outer, heads * 32, Fr, *sp), NAN, device=DEV), rot, bias, heads)
    assert bool(torch.isfinite(out).all())
    step = max(1, outer // 4)                      # the references in four pieces: below 2 GB of fp64 temporaries
    ref = torch.cat([_tattn_ref(qkv[o:o + step], bias, heads, torch.float64) for o in range(0, outer, step)])
    e32 = _rel(torch.cat([_tattn_ref(qkv[o:o + step], bias, heads, torch.float32) for o in range(0, outer, step)]), ref)
    e = _rel(out, ref)
    print(f"[measured] temporal attention heads={heads} outer={outer} inner={inner}: (ns, nblk, tiles_per_wg) = {want}: kernel {e:.2e} | "
          f"fp32 torch {e32:.2e}")
    assert e < _gate(1e-5, e32)
    del ref
    assert torch.equal(_tattn(qkv, torch.full_like(out, NAN), rot, bias, heads), out)
    single = torch.full_like(out, NAN)
    for o in range(outer):
        _tattn(qkv[o:o + 1], single[o:o + 1], rot, bias, heads)
    assert torch.equal(single, out)


# ------------------------------------------------------------------ 5. the fused LinearAttention block: pass 2, several tiles per workgroup
# Pass 2 (la_blk_out / its bf16-split and fp16 siblings) walks tiles_per_blk = clamp(ceil(nseq ntiles / 1024), 1, 8) tiles of 64 tokens
# per workgroup and rewrites its LDS images (xs, qs, and with a post norm `red`) for every tile.  n = 3904 = 61 tiles.
# (outer, inner, C, n, pre_mode, post_mode) -> tiles_per_blk:
LA_CASES = [
    # 4 * 30 * 61 = 7320 -> ceil(7320 / 1024) = 8 (anything above 7168 does; 117 MB): 8 workgroups per sequence, the last one 5
    # tiles.  A sample alone: 1830 -> 2.  LayerNorm behind the block: `red` is in use
    pytest.param((4, 30, 64, 3904, 0, 0), 8, id="tpb8"),
    # 40 * 61 = 2440 -> 3: 21 workgroups per sequence, the last one a single tile.  RMSNorm in front and behind
    pytest.param((1, 40, 64, 3904, 1, 1), 3, id="tpb3"),
]
_LA = {}


def _la_tpb(outer, inner, n):
    return min(max(_cdiv(outer * inner * (n // 64), 1024), 1), 8)


def _la_inputs(shape, seed):
    outer, inner, Cc, n = shape[:4]
    g = _gen(seed)
    x = _randn((outer, Cc, inner, n), g)
    g1, g2 = 1 + _randn((Cc,), g, 0.3), 1 + _randn((Cc,), g, 0.3)
    return x, g1, g2, _randn((384, Cc), g, 0.4), _randn((Cc, 128), g, 0.3), _randn((Cc,), g, 0.1)


def _la_case(shape):
    """inputs, packed weights and the fp64 references of a shape (computed once, never modified): the exact block of
    test_gpu_linattn_x3.py, the exact block and the fp16-operand emulation of test_gpu_linattn_f16.py"""
    if shape not in _LA:
        x, g1, g2, wqkv, wo, bo = inp = _la_inputs(shape, 450)
        pre, post = shape[4], shape[5]
        exact = LAX3._branch(*inp, pre, post)
        exact16 = LA16._branch(*inp, pre, post, lambda t: t)
        emu = LA16._branch(*inp, pre, post, lambda t: t.half().double())
        rms16 = exact16.pow(2).mean().sqrt().item()
        e_in = (emu - exact16).pow(2).mean().sqrt().item() / rms16
        del exact16
        d = LAX3._dev(g1, g2, wqkv, wo, bo, shape[2])
        _, _, d["wpk"] = LA16._dev_weights(wqkv, wo, shape[2])
        _LA[shape] = dict(x=x, d=d, exact=exact, emu=emu, rms=exact.pow(2).mean().sqrt().item(), scale=exact.abs().max().item(), e_in=e_in)
    return _LA[shape]


def _la_run(entry, x, d, pre, post):
    if entry == "f16":
        return LA16._run(x, d["g1"], d["pq"], d["po"], d["wpk"], d["bo"], d["g2"], pre, post)
    return LAX3._run(dict(impl0=0, impl1=1)[entry], x, d, pre, post)


@pytest.mark.parametrize("entry", ["impl0", "impl1", "f16"])
@pytest.mark.parametrize("shape,tpb", LA_CASES)
def test_linattn_block_pass2_walks_several_tiles(shape, tpb, entry):
    """sdc_linattn_block_sel (impl 0: fp32 pipe, impl 1: bf16 splits) and sdc_linattn_block_f16 against the exact fp64 block under
    each entry's own gate (impl 0: max |err| below 1e-5 of the branch scale, never widened -- the imported fp64 helpers have no fp32
    form, the yardstick printed beside the split kernel is the fp32 block as in test_gpu_linattn_x3.py; impl 1: that file's; f16:
    test_gpu_linattn_f16.py's, emulation and exact); two runs bit-identical; every `outer` sample alone -- another tiles_per_blk --
    equal to its slice of the batch bit for bit.  (At tpb8 -- 120 sequences, every CU busy -- sdc_linattn_block_f16 differed from run
    to run until la16_ctx's first maximum became a plain fmaxf: DESIGN.md section 8.)"""
    outer, inner, Cc, n, pre, post = shape
    assert _la_tpb(outer, inner, n) == tpb and (n // 64) % tpb != 0            # a short last workgroup
    c = _la_case(shape)
    x, d, exact, rms = c["x"], c["d"], c["exact"], c["rms"]
    y = _la_run(entry, x, d, pre, post)
    assert bool(torch.isfinite(y).all())
    err = lambda t, ref: ((t.double() - x.double()) - ref).pow(2).mean().sqrt().item() / rms         # noqa: E731
    e_x, e_max = err(y, exact), ((y.double() - x.double()) - exact).abs().max().item() / c["scale"]
    if entry == "f16":
        e_emu, e_in = err(y, c["emu"]), c["e_in"]
        print(f"[measured] linattn block f16 {shape} tiles_per_blk {tpb}: rms err vs fp64 emulation {e_emu:.2e}, vs exact fp64 {e_x:.2e} "
              f"(the emulation itself: {e_in:.2e})")
        assert 6.0e-4 <= e_in <= 1.3e-3, e_in
        assert e_x <= 2 * e_in, (e_x, e_in)
        assert e_emu <= min(LA16.GATE_EMU, e_in / 3), (e_emu, e_in)
    else:
        e_fp32 = e_x if entry == "impl0" else err(_la_run("impl0", x, d, pre, post), exact)
        print(f"[measured] linattn block {entry} {shape} tiles_per_blk {tpb}: rms err vs exact fp64 {e_x:.3e} | fp32 block {e_fp32:.3e}; "
              f"max |err| of the branch scale {e_max:.3e}")
        assert e_max < 1e-5, e_max
        if entry == "impl1":
            assert e_x <= max(1.25 * e_fp32, 2.0 ** -23), (e_x, e_fp32)
    assert torch.equal(_la_run(entry, x, d, pre, post), y)
    if outer > 1:
        assert _la_tpb(1, inner, n) == 2
        for b in range(outer):
            assert torch.equal(_la_run(entry, x[b:b + 1], d, pre, post)[0], y[b]), b


def test_linattn_block_gn_pass2_walks_several_tiles():
    """sdc_linattn_block_gn_sel, impl 0 (GroupNorm + SiLU + residual applied while pass 1 loads; pass 2 reads the h pass 1 left in y
    and overwrites it tile by tile) with tiles_per_blk = 3: the bits of sdc_gn_apply followed by sdc_linattn_block_sel, and against
    the exact fp64 block on that h"""
    shape = (1, 40, 64, 3904, 0, -1)
    outer, inner, Cc, n, pre, post = shape
    G = 8
    assert _la_tpb(outer, inner, n) == 3
    lib = _lib.get_lib()
    x, g1, g2, wqkv, wo, bo = inp = _la_inputs(shape, 460)
    g = _gen(461)
    gam, bet, r = 1 + _randn((Cc,), g, 0.2), _randn((Cc,), g, 0.1), _randn(tuple(x.shape), g)
    d = LAX3._dev(g1, g2, wqkv, wo, bo, Cc)
    st = grad_ops.gn_stats(x, G)
    y = torch.full_like(x, NAN)
    work = torch.full((int(lib.sdc_linattn_block_bytes(outer, inner, Cc, n)) // 4,), NAN, device=DEV)
    _lib.check(lib.sdc_linattn_block_gn_sel(x.data_ptr(), st.data_ptr(), gam.data_ptr(), bet.data_ptr(), G, r.data_ptr(), d["g1"].data_ptr(),
                                            d["pq"].data_ptr(), d["po"].data_ptr(), d["bo"].data_ptr(), None, work.data_ptr(), y.data_ptr(),
                                            outer, inner, Cc, n, Cc * inner * n, inner * n, n, pre, post, 1e-5, 0, _stream()),
               "sdc_linattn_block_gn_sel")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
    h = _gn_apply(x, st, gam, bet, G, res=r)
    assert torch.equal(LAX3._run(0, h, d, pre, post), y)
    exact = LAX3._branch(h, *inp[1:], pre, post)
    e_max = ((y.double() - h.double()) - exact).abs().max().item() / exact.abs().max().item()
    print(f"[measured] linattn block gn impl 0 {shape} tiles_per_blk 3: max |err| of the branch scale vs exact fp64 {e_max:.3e}")
    assert e_max < 1e-5, e_max


# ------------------------------------------------------------------ 6. sdc_linattn refuses before it launches
def test_linattn_core_refuses_before_any_launch():
    """heads = 4, outer inner = 16 384: 65 536 sequences do not fit la_out_kernel's grid.y.  SDC_EINVAL, and -- as for every other
    entry -- nothing was launched: the NaN-filled context and output are untouched"""
    heads, outer, inner, n = 4, 1, 16384, 2
    assert outer * inner * heads == 65536
    qkv = _randn((outer, 3 * heads * 32, inner, n), _gen(470))
    ctx = torch.full((outer * inner * heads * 32 * 32,), NAN, device=DEV)
    out = torch.full((outer, heads * 32, inner, n), NAN, device=DEV)
    rc = _lib.get_lib().sdc_linattn(qkv.data_ptr(), ctx.data_ptr(), out.data_ptr(), outer, inner, heads, n, 3 * heads * 32 * inner * n,
                                    inner * n, n, heads * 32 * inner * n, inner * n, n, _stream())
    assert rc == -1 and "65536" in _lib.last_error()              # SDC_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(ctx).all()) and bool(torch.isnan(out).all())
