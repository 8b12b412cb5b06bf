"""CPU-side checks of net.attn_split (include/sdc.h, sdc_tattn_block_x3): the three-plane bf16 buffer of the temporal-attention weights
-- Wb[head][piece][e], e < 8192: e = ((mat * 4 + s) * 64 + lane) * 8 + j <- Wqkv[mat * 128 + head * 32 + l31][16 s + 8 lh + j], then
e = 6144 + ((i * 2 + s) * 64 + lane) * 8 + j <- Wo[32 i + l31][head * 32 + row(8 s + j, lh)] with row(r, lh) = (r & 3) + 8 (r >> 2) +
4 lh, the pieces h = bf16(w), m = bf16(w - h), l = bf16(w - h - m) (RNE) -- the argument errors of the entry points, the routing table
and the plan's switch."""
import inspect

import pytest
import torch

import safediffcon_amd as sdc
from safediffcon_amd import _lib
from safediffcon_amd.engine import Plan, pack_conv_weight, pack_tattn_f16, pack_tattn_x3

SDC_EINVAL, SDC_EALIGN, SDC_ENULL = -1, -2, -4


def _layout_ref(wqkv, wo):
    """the documented positions written out with explicit loops: the fp32 weight that belongs at [head][e]"""
    out = torch.zeros(4, 8192)
    for head in range(4):
        e = 0
        for mat in range(3):
            for s in range(4):
                for lane in range(64):
                    l31, lh = lane & 31, lane >> 5
                    for j in range(8):
                        out[head, e] = wqkv[mat * 128 + head * 32 + l31, 16 * s + 8 * lh + j]
                        e += 1
        assert e == 6144
        for i in range(2):
            for s in range(2):
                for lane in range(64):
                    l31, lh = lane & 31, lane >> 5
                    for j in range(8):
                        r = 8 * s + j
                        out[head, e] = wo[32 * i + l31, head * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh]
                        e += 1
        assert e == 8192
    return out


def _weights(seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(384, 64, generator=g) * 3.0, torch.randn(64, 128, generator=g) * 3.0


def test_pack_tattn_x3_is_the_documented_layout_and_sums_back_exactly():
    wqkv, wo = _weights()
    ref = _layout_ref(wqkv, wo)
    got = pack_tattn_x3(wqkv, wo).view(torch.bfloat16)
    assert got.numel() * 2 == _lib.get_lib().sdc_pack_tattn_x3_bytes() == 196608
    p = got.reshape(4, 3, 8192)
    # the pieces are the RNE split, piece by piece, and sum back to the fp32 weight exactly (fp32 sums, largest last to smallest: each
    # partial sum is representable because it is a residual of the split)
    h = ref.bfloat16()
    m = (ref - h.float()).bfloat16()
    low = (ref - h.float() - m.float()).bfloat16()
    assert torch.equal(p[:, 0].view(torch.int16), h.view(torch.int16))
    assert torch.equal(p[:, 1].view(torch.int16), m.view(torch.int16))
    assert torch.equal(p[:, 2].view(torch.int16), low.view(torch.int16))
    assert torch.equal((p[:, 2].float() + p[:, 1].float()) + p[:, 0].float(), ref)
    assert torch.equal(p.double().sum(1), ref.double())
    # the main plane is pack_tattn_f16's order, head by head: the same permutation of the weights
    f16 = pack_tattn_f16(wqkv, wo).view(torch.float16)
    a, b = f16[:24576].reshape(4, 6144), f16[24576:].reshape(4, 2048)
    assert torch.equal(torch.cat([a, b], 1), ref.half())
    # every weight appears exactly once per plane
    both = torch.cat([wqkv.reshape(-1), wo.reshape(-1)])
    assert torch.equal(ref.reshape(-1).sort().values, both.sort().values)
    # the plan packs the same buffer, from tensors and from callables
    plan = Plan("cpu", precision=4, attn_split=True)
    assert torch.equal(plan.tattn_weight(wqkv, wo, split=True).view(torch.int16), got.view(torch.int16))
    assert torch.equal(plan.tattn_weight(lambda: wqkv, lambda: wo, split=True).view(torch.int16), got.view(torch.int16))
    for bad in ((wqkv.t(), wo), (wqkv, wo.t()), (wqkv[:256], wo)):
        with pytest.raises(ValueError):
            pack_tattn_x3(*bad)


def test_attn_x3_entries_reject_before_any_launch():
    lib = _lib.get_lib()
    P = 256                                          # a non-null, 16-byte aligned address that is never dereferenced
    ok = dict(x=P, g=P, w=P, rot=P, bias=P, y=P, outer=2, inner=16, C=64, ntok=32, so=64 * 32 * 16, sc=32 * 16, st=16)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sdc_tattn_block_x3(a["x"], a["g"], a["w"], a["rot"], a["bias"], a["y"], a["outer"], a["inner"], a["C"], a["ntok"],
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
    assert call(sc=-1) == SDC_EINVAL
    for w in (P + 2, P + 4, P + 8):
        assert call(w=w) == SDC_EALIGN, w
        assert "16-byte aligned" in _lib.last_error()
    assert call(rot=P + 4) == SDC_EINVAL and "rot" in _lib.last_error()
    # the packer
    assert lib.sdc_pack_tattn_x3(None, P, P, None) == SDC_ENULL
    assert lib.sdc_pack_tattn_x3(P, None, P, None) == SDC_ENULL
    assert lib.sdc_pack_tattn_x3(P, P, None, None) == SDC_ENULL
    assert lib.sdc_pack_tattn_x3(P, P, P + 8, None) == SDC_EALIGN


def test_the_three_block_entries_report_shared_checks_under_their_own_name():
    """the argument checks the three entries share (sdc_tablock_tile.h) name the entry that was called"""
    lib = _lib.get_lib()
    P = 256
    ok = dict(outer=2, inner=16, C=64, so=64 * 32 * 16, sc=32 * 16, st=16)
    entries = {
        "sdc_tattn_block": lambda a: lib.sdc_tattn_block(P, P, P, P, P, P, P, a["outer"], a["inner"], a["C"], 32, a["so"], a["sc"], a["st"],
                                                         1e-5, None),
        "sdc_tattn_block_f16": lambda a: lib.sdc_tattn_block_f16(P, P, P, P, P, P, a["outer"], a["inner"], a["C"], 32, a["so"], a["sc"],
                                                                 a["st"], 1e-5, None),
        "sdc_tattn_block_x3": lambda a: lib.sdc_tattn_block_x3(P, P, P, P, P, P, a["outer"], a["inner"], a["C"], 32, a["so"], a["sc"],
                                                               a["st"], 1e-5, None),
    }
    # Cc = 32; an inner that is no multiple of 8; one outer index spanning 4 GB (31 st + inner + 63 sc = 2^30 elements) and more
    rejected = (dict(C=32), dict(inner=12), dict(st=(2 ** 30 - 16 - 63 * 512) // 31 + 1), dict(sc=1 << 26))
    for name, call in entries.items():
        for kw in rejected:
            assert call(dict(ok, **kw)) == SDC_EINVAL, (name, kw)
            assert _lib.last_error().startswith(name + ": "), (name, kw, _lib.last_error())


def test_routing_table_lists_per_sample_sizes_only():
    lib = _lib.get_lib()
    assert lib.sdc_tattn_block_x3_ok(64, 32, 64 * 64) == 1                # the measured site
    # the smaller volumes of the dim-64 net stay on the fp32 block; other widths and frame counts are not covered at all
    for c, fr, inner in ((64, 32, 32 * 32), (64, 32, 16 * 16), (64, 32, 8), (128, 32, 4096), (64, 16, 4096), (64, 32, 4095), (0, 0, 0)):
        assert lib.sdc_tattn_block_x3_ok(c, fr, inner) == 0, (c, fr, inner)


def test_plan_switch_records_the_split_block_only_where_the_table_routes():
    assert inspect.signature(Plan.__init__).parameters["attn_split"].default is False
    assert Plan("cpu", precision=4).attn_split is False                   # off for a Plan built directly
    assert Plan("cpu", precision=4, attn_split=True).attn_split is True and Plan("cpu", precision=5, attn_split=True).attn_split is True
    for prec in (0, 2, 3, 6, 7):
        assert Plan("cpu", precision=prec, attn_split=True).attn_split is False
    assert Plan("cpu", precision=4, attn_split=True, attn_f16=True).attn_split is False       # attn_f16 wins
    wqkv, wo = _weights(7)
    wqkv, wo = wqkv / 10, wo / 10
    g, rot, bias = torch.ones(64), torch.zeros(1024), torch.zeros(4096)
    routed, small = torch.zeros(1, 64, 32, 64, 64), torch.zeros(1, 64, 32, 32, 32)

    def fp32_call(plan, x):
        plan.tattn_block(x, g, plan.conv_weight(wqkv.view(384, 64, 1)), plan.conv_weight(wo.view(64, 128, 1)), rot, bias)
        return plan.calls[-1]

    for prec in (4, 5):
        on, off = Plan("cpu", precision=prec, attn_split=True), Plan("cpu", precision=prec)
        assert on.tattn_split_routes(64, 32, 4096) and not on.tattn_split_routes(64, 32, 1024) and not off.tattn_split_routes(64, 32, 4096)
        y = on.tattn_block(routed, g, lambda: wqkv, lambda: wo, rot, bias)
        assert tuple(y.shape) == tuple(routed.shape)
        assert [fn.__name__ for fn, _ in on.calls] == ["sdc_tattn_block_x3"]
        # the buffer is on the repacker list: refresh_weights() sees a write to the weights
        dst, fn = on.repackers[-1]
        assert torch.equal(dst, pack_tattn_x3(wqkv, wo))
        wqkv.mul_(2.0)
        on.refresh_weights()
        assert torch.equal(dst, pack_tattn_x3(wqkv, wo))
        wqkv.mul_(0.5)
        ref = fp32_call(off, routed)
        assert ref[0].__name__ == "sdc_tattn_block"
        # the same sizes, strides and eps behind the pointers
        assert on.calls[0][1][6:] == ref[1][7:] and len(on.calls[0][1]) + 1 == len(ref[1])
        # a site the table does not list: the parent's call, with the switch on
        assert fp32_call(on, small)[0].__name__ == "sdc_tattn_block"
        assert fp32_call(on, small)[1][7:] == fp32_call(off, small)[1][7:]
    # attn_f16 wins at a routed site; the other precisions never route
    both = Plan("cpu", precision=4, attn_split=True, attn_f16=True)
    both.tattn_block(routed, g, lambda: wqkv, lambda: wo, rot, bias)
    assert [fn.__name__ for fn, _ in both.calls] == ["sdc_tattn_block_f16"]
    for prec in (0, 3, 6):
        p = Plan("cpu", precision=prec, attn_split=True)
        assert fp32_call(p, routed)[0].__name__ == "sdc_tattn_block"
        # conv_weight buffers are unchanged by the switch
        w = torch.randn(384, 64, generator=torch.Generator().manual_seed(3))
        assert torch.equal(p.conv_weight(w), pack_conv_weight(w, precision=prec))


def test_net_switch_is_a_plan_cache_key_and_reaches_the_plan(monkeypatch):
    """entry() on a CPU box, up to the point where it builds the Plan: the cache keys it looks up differ with the switch, and the Plan is
    constructed with the net's value"""
    net = sdc.Unet3D_with_Conv3D(dim=8, dim_mults=(1, 2), channels=7)
    assert isinstance(net.attn_split, bool)

    class Stop(Exception):
        pass

    class Keys(dict):
        seen = []

        def get(self, key, default=None):
            Keys.seen.append(key)
            return super().get(key, default)

    made = []

    def fake_plan(dev, **kw):
        made.append(kw)
        raise Stop

    class Dev:
        type = "cuda"

    net._plans = Keys()
    monkeypatch.setattr(sdc.unet, "Plan", fake_plan)
    monkeypatch.setattr(net, "device", lambda: Dev())
    for on in (False, True, False):
        net.attn_split = on
        with pytest.raises(Stop):
            net.entry((1, 32, 7, 8, 8), 1)
    k_off, k_on, k_off2 = Keys.seen
    assert k_off == k_off2 and k_on != k_off                  # part of the cache key
    assert sum(a != b for a, b in zip(k_on, k_off)) == 1 and len(k_on) == len(k_off)
    assert [kw["attn_split"] for kw in made] == [False, True, False]      # handed to the Plan
    # the switch changes nothing else that the Plan is built with
    assert {k: v for k, v in made[0].items() if k != "attn_split"} == {k: v for k, v in made[1].items() if k != "attn_split"}
