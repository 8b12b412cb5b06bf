"""CPU-side checks of net.linattn_f16 (include/sdc.h, sdc_linattn_block_f16 / sdc_linattn_block_gn_f16): the fp16 fragment buffer of the
LinearAttention weights -- Wh[mat][head][s][lane][j] = Wqkv[mat * 128 + head * 32 + l31][16 s + 8 lh + j], mat = 0 q, 1 k, s < C / 16
(RNE) -- the argument errors of the entry points and the plan's switch."""
import pytest
import torch

from safediffcon_amd import _lib
from safediffcon_amd.engine import Plan, pack_conv_weight, pack_linattn_f16

SDC_EINVAL, SDC_EALIGN, SDC_ENULL = -1, -2, -4


def _layout_ref(wqkv, Cc):
    """the documented layout written out with explicit loops"""
    out = torch.zeros(256 * Cc, dtype=torch.float16)
    e = 0
    for mat in range(2):
        for head in range(4):
            for s in range(Cc // 16):
                for lane in range(64):
                    l31, lh = lane & 31, lane >> 5
                    for j in range(8):
                        out[e] = wqkv[mat * 128 + head * 32 + l31, 16 * s + 8 * lh + j].half()
                        e += 1
    assert e == 256 * Cc
    return out


def _weights(Cc, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(384, Cc, generator=g) * 3.0, torch.randn(Cc, 128, generator=g) * 3.0


@pytest.mark.parametrize("Cc", [64, 128])
def test_pack_linattn_f16_is_the_documented_layout(Cc):
    wqkv, wo = _weights(Cc)
    ref = _layout_ref(wqkv, Cc)
    got = pack_linattn_f16(wqkv, wo).view(torch.float16)
    assert got.numel() * 2 == _lib.get_lib().sdc_pack_linattn_f16_bytes(Cc) == 512 * Cc
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    # every q and k weight appears exactly once: the buffer is a permutation of the rounded rows 0 .. 255
    assert torch.equal(got.float().sort().values, wqkv[:256].half().float().reshape(-1).sort().values)
    # conv-shaped weights (trailing unit axes) pack the same buffer
    assert torch.equal(pack_linattn_f16(wqkv.view(384, Cc, 1), wo.view(Cc, 128, 1, 1)).view(torch.int16), got.view(torch.int16))
    for bad in ((wqkv.t(), wo), (wqkv, wo[:, :64]), (wqkv, wo[:32]), (wqkv[:256], wo), (wqkv[:, :32], wo[:32])):
        with pytest.raises(ValueError):
            pack_linattn_f16(*bad)
    assert _lib.get_lib().sdc_pack_linattn_f16_bytes(32) == 0 and _lib.get_lib().sdc_pack_linattn_f16_bytes(256) == 0


def test_linattn_f16_rounding_is_nearest_even():
    # halfway cases between two fp16 neighbours round to the even one (RNE); round-toward-zero would truncate them all
    one = 1.0 + 2.0 ** -11                           # halfway between 1 and 1 + 2^-10: even -> 1
    three = 1.0 + 3 * 2.0 ** -11                     # halfway between 1 + 2^-10 and 1 + 2^-9: even -> 1 + 2^-9
    pat = torch.tensor([one, three, -three, 1.0], dtype=torch.float32)
    for Cc in (64, 128):
        h = pack_linattn_f16(pat.repeat(384, Cc // 4), torch.zeros(Cc, 128)).view(torch.float16).float().reshape(-1, 8)
        # j runs over consecutive channels
        assert torch.equal(h, torch.tensor([1.0, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -9), 1.0]).repeat(2).expand_as(h))


def test_linattn_f16_entries_reject_before_any_launch():
    lib = _lib.get_lib()
    P = 256                                          # a non-null, 16-byte aligned address that is never dereferenced
    ok = dict(x=P, g=P, wqkv=P, wo=P, wpk=P, bo=P, gp=P, work=P, y=P, outer=2, inner=3, C=64, n=128, so=64 * 3 * 128, sc=3 * 128, si=128,
              pre=0, post=0, st=P, gam=P, bet=P, G=8, res=P)

    def plain(a):
        return lib.sdc_linattn_block_f16(a["x"], a["g"], a["wqkv"], a["wo"], a["wpk"], a["bo"], a["gp"], a["work"], a["y"], a["outer"],
                                         a["inner"], a["C"], a["n"], a["so"], a["sc"], a["si"], a["pre"], a["post"], 1e-5, None)

    def gn(a):
        return lib.sdc_linattn_block_gn_f16(a["x"], a["st"], a["gam"], a["bet"], a["G"], a["res"], a["g"], a["wqkv"], a["wo"], a["wpk"],
                                            a["bo"], a["gp"], a["work"], a["y"], a["outer"], a["inner"], a["C"], a["n"], a["so"], a["sc"],
                                            a["si"], a["pre"], a["post"], 1e-5, None)

    for entry in (plain, gn):
        call = lambda **kw: entry(dict(ok, **kw))
        for name in ("x", "g", "wqkv", "wo", "wpk", "work", "y"):
            assert call(**{name: None}) == SDC_ENULL, name
            assert "null" in _lib.last_error()
        assert call(gp=None) == SDC_ENULL and "gain" in _lib.last_error()          # a post norm needs its gain ...
        for bad in (dict(C=32), dict(C=96), dict(C=256)):
            assert call(**bad) == SDC_EINVAL, bad
        assert "64 or 128" in _lib.last_error() or "groups" in _lib.last_error()
        for bad in (dict(n=100), dict(n=0), dict(n=-64), dict(outer=0), dict(inner=0), dict(outer=300, inner=300)):
            assert call(**bad) == SDC_EINVAL, bad
        for bad in (dict(pre=2), dict(pre=-1), dict(post=2), dict(post=-2)):
            assert call(**bad) == SDC_EINVAL and "norm mode" in _lib.last_error(), bad
        assert call(sc=0) == SDC_EINVAL and call(sc=1 << 27) == SDC_EINVAL
        for w in (P + 2, P + 4, P + 8):
            assert call(wpk=w) == SDC_EALIGN and "16-byte aligned" in _lib.last_error(), w
            assert call(work=w) == SDC_EALIGN and "16-byte aligned" in _lib.last_error(), w
    call = lambda **kw: gn(dict(ok, **kw))
    for name in ("st", "gam", "bet"):
        assert call(**{name: None}) == SDC_ENULL, name
    assert call(G=0) == SDC_EINVAL and call(G=7) == SDC_EINVAL
    # the packer
    assert lib.sdc_pack_linattn_f16(None, P, 64, P, None) == SDC_ENULL
    assert lib.sdc_pack_linattn_f16(P, None, 64, P, None) == SDC_ENULL
    assert lib.sdc_pack_linattn_f16(P, P, 64, None, None) == SDC_ENULL
    assert lib.sdc_pack_linattn_f16(P, P, 96, P, None) == SDC_EINVAL
    assert lib.sdc_pack_linattn_f16(P, P, 128, P + 8, None) == SDC_EALIGN
    # the routing predicate and the scratch size: the covered (C, n), the fp32 partials plus the fp16 T fragments
    assert lib.sdc_linattn_block_f16_ok(64, 4096) == 1 and lib.sdc_linattn_block_f16_ok(128, 64) == 1
    assert lib.sdc_linattn_block_f16_ok(64, 100) == 0 and lib.sdc_linattn_block_f16_ok(256, 128) == 0 and lib.sdc_linattn_block_f16_ok(64, 0) == 0
    for outer, inner, Cc, n in ((2, 3, 64, 128), (1, 2, 128, 1024), (1, 1, 64, 4096)):
        f32 = lib.sdc_linattn_block_bytes(outer, inner, Cc, n)
        assert lib.sdc_linattn_block_f16_bytes(outer, inner, Cc, n) == f32 - outer * inner * 128 * Cc * 2
    assert lib.sdc_linattn_block_f16_bytes(1, 1, 96, 128) == 0


def test_plan_switch_records_the_f16_block_and_leaves_the_other_layouts_alone():
    assert Plan("cpu", linattn_f16=True).linattn_f16 is True and Plan("cpu").linattn_f16 is False
    assert Plan("cpu", precision=6).linattn_f16 is False and Plan("cpu", attn_f16=True).linattn_f16 is False
    for Cc in (64, 128):
        wqkv, wo = _weights(Cc, 7)
        wqkv, wo = wqkv / 10, wo / 10
        x = torch.zeros(2, Cc, 3, 128)
        g, bo = torch.ones(Cc), torch.zeros(Cc)
        geom = (2, 3, 128, (Cc * 3 * 128, 3 * 128, 128), 0, -1)
        for prec in (0, 4, 6):
            on, off = Plan("cpu", precision=prec, linattn_f16=True), Plan("cpu", precision=prec)
            pq, po = on.conv_weight(wqkv.view(384, Cc, 1)), on.conv_weight(wo.view(Cc, 128, 1))
            y = on.linattn_block(x, g, pq, po, bo, None, *geom, w16=(lambda: wqkv, lambda: wo))
            assert tuple(y.shape) == tuple(x.shape)
            assert [fn.__name__ for fn, _ in on.calls] == ["sdc_linattn_block_f16"]
            # the buffer is on the repacker list: refresh_weights() sees a write to the weights
            dst, fn = on.repackers[-1]
            assert torch.equal(dst, pack_linattn_f16(wqkv, wo))
            wqkv.mul_(2.0)
            on.refresh_weights()
            assert torch.equal(dst, pack_linattn_f16(wqkv, wo))
            wqkv.mul_(0.5)
            # tensors instead of callables; the GroupNorm-on-load form
            on.linattn_block(x, g, pq, po, bo, None, *geom, w16=(wqkv, wo), gn=(torch.zeros(64), g, bo, 8, None))
            assert [fn.__name__ for fn, _ in on.calls][1:] == ["sdc_linattn_block_gn_f16"]
            # without the unpacked weights, or with the switch off, today's calls -- the same sizes, strides, modes and eps behind the pointers
            on.linattn_block(x, g, pq, po, bo, None, *geom)
            off.linattn_block(x, g, off.conv_weight(wqkv.view(384, Cc, 1)), off.conv_weight(wo.view(Cc, 128, 1)), bo, None, *geom,
                              w16=(wqkv, wo))
            assert on.calls[2][0].__name__ == "sdc_linattn_block" and [fn.__name__ for fn, _ in off.calls] == ["sdc_linattn_block"]
            assert on.calls[0][1][9:] == off.calls[0][1][8:] and len(on.calls[0][1]) == len(off.calls[0][1]) + 1
            assert on.calls[2][1][8:] == off.calls[0][1][8:]
            # conv_weight buffers are unchanged by the switch
            gen = torch.Generator().manual_seed(3)
            for shape in ((384, 64), (64, 128), (384, 128, 1), (64, 12, 7), (64, 7, 7, 7, 7), (40, 24, 3, 3), (16, 8, 3, 3, 3)):
                w = torch.randn(*shape, generator=gen)
                assert torch.equal(on.conv_weight(w), off.conv_weight(w))
                assert torch.equal(on.conv_weight(w), pack_conv_weight(w, precision=prec))
    # a width the kernels do not cover keeps today's call whatever the switch says
    on = Plan("cpu", linattn_f16=True)
    assert not on.linattn_f16_routes(256, 128) and not on.linattn_f16_routes(64, 100) and on.linattn_f16_routes(128, 64)
    assert not Plan("cpu").linattn_f16_routes(64, 128)
