"""CPU-side checks of net.attn_f16 (include/sdc.h, sdc_tattn_block_f16): the fp16 fragment buffer of the temporal-attention weights
-- Wh[head][mat][s][lane][j] = Wqkv[mat * 128 + head * 32 + l31][16 s + 8 lh + j], then Wh'[head][i][s][lane][j] = Wo[32 i + l31][head *
32 + row(8 s + j, lh)] with row(r, lh) = (r & 3) + 8 (r >> 2) + 4 lh (RNE) -- the argument errors of the entry points and the plan's
switch."""
import pytest
import torch

from safediffcon_amd import _lib
from safediffcon_amd.engine import Plan, pack_conv_weight, pack_tattn_f16

SDC_EINVAL, SDC_EALIGN, SDC_ENULL = -1, -2, -4


def _layout_ref(wqkv, wo):
    """the documented layout written out with explicit loops"""
    out = torch.zeros(32768, dtype=torch.float16)
    e = 0
    for head in range(4):
        for mat in range(3):
            for s in range(4):
                for lane in range(64):
                    l31, lh = lane & 31, lane >> 5
                    for j in range(8):
                        out[e] = wqkv[mat * 128 + head * 32 + l31, 16 * s + 8 * lh + j].half()
                        e += 1
    assert e == 24576
    for head in range(4):
        for i in range(2):
            for s in range(2):
                for lane in range(64):
                    l31, lh = lane & 31, lane >> 5
                    for j in range(8):
                        r = 8 * s + j
                        out[e] = wo[32 * i + l31, head * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh].half()
                        e += 1
    assert e == 32768
    return out


def _weights(seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(384, 64, generator=g) * 3.0, torch.randn(64, 128, generator=g) * 3.0


def test_pack_tattn_f16_is_the_documented_layout():
    wqkv, wo = _weights()
    ref = _layout_ref(wqkv, wo)
    got = pack_tattn_f16(wqkv, wo).view(torch.float16)
    assert got.numel() * 2 == _lib.get_lib().sdc_pack_tattn_f16_bytes() == 65536
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    # every weight appears exactly once: the buffer is a permutation of the rounded weights
    both = torch.cat([wqkv.half().reshape(-1), wo.half().reshape(-1)])
    assert torch.equal(got.float().sort().values, both.float().sort().values)
    # the plan packs the same buffer, from tensors and from callables
    plan = Plan("cpu", attn_f16=True)
    assert torch.equal(plan.tattn_weight(wqkv, wo).view(torch.int16), ref.view(torch.int16))
    assert torch.equal(plan.tattn_weight(lambda: wqkv, lambda: wo).view(torch.int16), ref.view(torch.int16))
    for bad in ((wqkv.t(), wo), (wqkv, wo.t()), (wqkv[:256], wo)):
        with pytest.raises(ValueError):
            pack_tattn_f16(*bad)


def test_attn_f16_rounding_is_nearest_even():
    # halfway cases between two fp16 neighbours round to the even one (RNE); round-toward-zero would truncate them all
    one = 1.0 + 2.0 ** -11                           # halfway between 1 and 1 + 2^-10: even -> 1
    three = 1.0 + 3 * 2.0 ** -11                     # halfway between 1 + 2^-10 and 1 + 2^-9: even -> 1 + 2^-9
    pat = torch.tensor([one, three, -three, 1.0], dtype=torch.float32)
    wqkv, wo = pat.repeat(384, 16), pat.repeat(64, 32)
    h = pack_tattn_f16(wqkv, wo).view(torch.float16).float()
    # q / k / v fragments: j runs over consecutive channels
    a = h[:24576].reshape(-1, 8)
    assert torch.equal(a, torch.tensor([1.0, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -9), 1.0]).repeat(2).expand_as(a))
    # Wo fragments: j = 4 jh + jl covers columns 8 jh + jl (+ 16 s + 4 lh): the pattern again
    b = h[24576:].reshape(-1, 8)
    assert torch.equal(b, torch.tensor([1.0, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -9), 1.0]).repeat(2).expand_as(b))


def test_attn_f16_entries_reject_before_any_launch():
    lib = _lib.get_lib()
    P = 256                                          # a non-null, 16-byte aligned address that is never dereferenced
    ok = dict(x=P, g=P, w=P, rot=P, bias=P, y=P, outer=2, inner=16, C=64, ntok=32, so=64 * 32 * 16, sc=32 * 16, st=16)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sdc_tattn_block_f16(a["x"], a["g"], a["w"], a["rot"], a["bias"], a["y"], a["outer"], a["inner"], a["C"], a["ntok"],
                                       a["so"], a["sc"], a["st"], 1e-5, None)

    for name in ("x", "g", "w", "y"):
        assert call(**{name: None}) == SDC_ENULL, name
        assert "null" in _lib.last_error()
    assert call(C=128) == SDC_EINVAL and "dim 64" in _lib.last_error()
    assert call(C=32) == SDC_EINVAL
    assert call(ntok=16) == SDC_EINVAL and "32 frames" in _lib.last_error()
    assert call(ntok=64) == SDC_EINVAL
    assert call(inner=12) == SDC_EINVAL and "multiple of 8" in _lib.last_error()
    assert call(inner=0) == SDC_EINVAL and call(outer=0) == SDC_EINVAL
    assert call(st=1 << 28) == SDC_EINVAL and "4 GB" in _lib.last_error()
    for w in (P + 2, P + 4, P + 8):
        assert call(w=w) == SDC_EALIGN, w
        assert "16-byte aligned" in _lib.last_error()
    assert call(rot=P + 4) == SDC_EINVAL and "rot" in _lib.last_error()
    # the packer
    assert lib.sdc_pack_tattn_f16(None, P, P, None) == SDC_ENULL
    assert lib.sdc_pack_tattn_f16(P, None, P, None) == SDC_ENULL
    assert lib.sdc_pack_tattn_f16(P, P, None, None) == SDC_ENULL
    assert lib.sdc_pack_tattn_f16(P, P, P + 8, None) == SDC_EALIGN


def test_plan_switch_records_the_f16_block_and_leaves_the_other_layouts_alone():
    assert Plan("cpu", attn_f16=True).attn_f16 is True and Plan("cpu").attn_f16 is False and Plan("cpu", precision=6).attn_f16 is False
    wqkv, wo = _weights(7)
    wqkv, wo = wqkv / 10, wo / 10
    x = torch.zeros(1, 64, 32, 2, 4)
    g, rot, bias = torch.ones(64), torch.zeros(1024), torch.zeros(4096)
    for prec in (0, 4, 6):
        on, off = Plan("cpu", precision=prec, attn_f16=True), Plan("cpu", precision=prec)
        y = on.tattn_block(x, g, lambda: wqkv, lambda: wo, rot, bias)
        assert tuple(y.shape) == tuple(x.shape)
        assert [fn.__name__ for fn, _ in on.calls] == ["sdc_tattn_block_f16"]
        # the buffer is on the repacker list: refresh_weights() sees a write to the weights
        dst, fn = on.repackers[-1]
        assert torch.equal(dst, pack_tattn_f16(wqkv, wo))
        wqkv.mul_(2.0)
        on.refresh_weights()
        assert torch.equal(dst, pack_tattn_f16(wqkv, wo))
        wqkv.mul_(0.5)
        off.tattn_block(x, g, off.conv_weight(wqkv.view(384, 64, 1)), off.conv_weight(wo.view(64, 128, 1)), rot, bias)
        assert [fn.__name__ for fn, _ in off.calls] == ["sdc_tattn_block"]
        # the same sizes, strides and eps behind the pointers
        assert on.calls[0][1][6:] == off.calls[0][1][7:] and len(on.calls[0][1]) + 1 == len(off.calls[0][1])
        # conv_weight buffers are unchanged by the switch
        gen = torch.Generator().manual_seed(3)
        for shape in ((384, 64), (64, 128), (384, 64, 1), (64, 12, 7), (64, 7, 7, 7, 7), (40, 24, 3, 3), (16, 8, 3, 3, 3)):
            w = torch.randn(*shape, generator=gen)
            assert torch.equal(on.conv_weight(w), off.conv_weight(w))
            assert torch.equal(on.conv_weight(w), pack_conv_weight(w, precision=prec))
