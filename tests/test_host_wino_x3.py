"""CPU: the host side of net.wino_split (csrc/sdc_conv_wino_x3.hip) -- the exact three-way bf16 split, the packed weight layout of
sdc_conv_wino3_x3 against a plain-loop reference, the size query, and the switch semantics of Plan and of the nets."""
import ctypes as C
import inspect

import pytest
import torch

import safediffcon_amd as sdc
from safediffcon_amd import _lib, engine
from safediffcon_amd.engine import PLAN_SWITCHES, Plan, pack_conv_weight, pack_wino3_x3, split3_bf16


def test_split_is_exact_over_the_exponent_range():
    g = torch.Generator().manual_seed(5)
    for e in range(-100, 101, 4):
        # random signs and significands at exponent e (the pieces reach down to 2^(e - 24): normal bf16 numbers over this range)
        x = (1.0 + torch.rand(4096, generator=g)) * (2.0 * torch.randint(0, 2, (4096,), generator=g) - 1.0) * 2.0 ** e
        h, m, l = split3_bf16(x)
        assert torch.equal(h.float() + m.float() + l.float(), x), e
        # (the sum is formed exactly: h + m has at most 16 significant bits, l fills the rest)
        assert torch.equal((h.double() + m.double() + l.double()).float(), x), e


def test_dropped_terms_stay_below_fp32_rounding():
    # a b - (a1 b1 + a1 b2 + a2 b1 + a1 b3 + a2 b2 + a3 b1) = a2 b3 + a3 b2 + a3 b3: at most 2^-24 |a b|
    g = torch.Generator().manual_seed(6)
    a, b = torch.randn(1 << 16, generator=g), torch.randn(1 << 16, generator=g)
    pa, pb = [p.double() for p in split3_bf16(a)], [p.double() for p in split3_bf16(b)]
    kept = pa[0] * pb[0] + pa[0] * pb[1] + pa[1] * pb[0] + pa[0] * pb[2] + pa[1] * pb[1] + pa[2] * pb[0]
    dropped = (a.double() * b.double() - kept).abs()
    assert torch.equal(a.double() * b.double() - kept, pa[1] * pb[2] + pa[2] * pb[1] + pa[2] * pb[2])
    assert (dropped <= 2.0 ** -24 * (a.double() * b.double()).abs()).all()


def test_pack_wino3_x3_layout_against_plain_loops():
    co, ci = 64, 16
    g = torch.Generator().manual_seed(7)
    w = torch.randn(co, ci, 3, 3, 3, generator=g)
    wp4 = pack_conv_weight(w, "conv", 4)
    n = 64 * ci * co
    u3 = wp4[-n:].reshape(4, ci, co, 16)                      # U3[jd][ci][co][j * 4 + xi], the last part of the precision-4 buffer
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
    assert torch.equal(u3, torch.einsum("zd,jh,xk,oidhk->ziojx", G, G, G, w.double()).reshape(4, ci, co, 16).float())
    wb = pack_wino3_x3(wp4, co, ci).view(torch.bfloat16).reshape(3, -1)
    assert wb.shape[1] == n
    pieces = [p.reshape(-1) for p in split3_bf16(u3)]
    u3f = u3.reshape(-1)
    e = 0
    for mt in range(co // 64):
        for jd in range(4):
            for st in range(ci // 16):
                for j in range(4):
                    for xi in range(4):
                        for col in range(64):
                            for c16 in range(16):
                                # (rows 8-15 of every 16: the two channel octets swapped)
                                src = ((jd * ci + st * 16 + (c16 ^ (8 * ((col >> 3) & 1)))) * co + mt * 64 + col) * 16 + j * 4 + xi
                                for p in range(3):
                                    assert wb[p, e].view(torch.int16) == pieces[p][src].view(torch.int16), (p, mt, jd, st, j, xi, col, c16)
                                assert wb[0, e].float() + wb[1, e].float() + wb[2, e].float() == u3f[src]
                                e += 1
    assert e == n
    with pytest.raises(ValueError):
        pack_wino3_x3(wp4, 64, 24)
    with pytest.raises(ValueError):
        pack_wino3_x3(wp4[:-1], co, ci)


def test_pack_bytes_agrees_with_the_host_size():
    try:
        lib = _lib.get_lib()
    except OSError:
        return                                                # (the library needs the HIP runtime to load; the GPU tests call it)
    for co, ci in ((64, 16), (128, 512), (256, 256)):
        assert int(lib.sdc_pack_wino3_x3_bytes(co, ci)) == 3 * 64 * ci * co * 2
    w = torch.zeros(64, 16, 3, 3, 3)
    assert pack_wino3_x3(pack_conv_weight(w, "conv", 4), 64, 16).numel() * 4 == int(lib.sdc_pack_wino3_x3_bytes(64, 16))
    for co, ci in ((96, 16), (64, 24), (0, 16), (64, 0)):
        assert int(lib.sdc_pack_wino3_x3_bytes(co, ci)) == 0


def _plan(**kw):
    try:
        return Plan("cpu", **kw)
    except OSError:
        return None


def test_plan_switch_semantics():
    assert inspect.signature(Plan.__init__).parameters["wino_split"].default is False
    p = _plan(precision=4)
    if p is None:
        return
    assert p.wino_split is False                              # off for a Plan built directly
    assert _plan(precision=4, wino_split=True).wino_split is True
    assert _plan(precision=5, wino_split=True).wino_split is True
    for prec in (0, 2, 3, 6, 7):                              # off below precision 4; 6 and 7 keep their fp16 kernels and today's calls
        assert _plan(precision=prec, wino_split=True).wino_split is False


@pytest.mark.parametrize("switch", PLAN_SWITCHES)
def test_net_switch_is_on_and_part_of_the_plan_cache_key(switch, monkeypatch):
    """entry() on a CPU box, up to the point where it builds the Plan: every switch of PLAN_SWITCHES is an attribute of the nets, one
    element of the cache key, and reaches the Plan with the net's value"""
    for net in (sdc.Unet3D_with_Conv3D(dim=8, dim_mults=(1, 2), channels=7),
                sdc.Unet2D(dim=8, dim_mults=(1, 2), channels=3, resnet_block_groups=1),
                sdc.Unet1D(dim=8, dim_mults=(1, 2), channels=12, resnet_block_groups=1)):
        assert net.wino_split is WINO_DEFAULT
        assert isinstance(getattr(net, switch), bool)
    assert switch in inspect.signature(Plan.__init__).parameters

    class Stop(Exception):
        pass

    seen, made = [], []

    class Keys(dict):
        def get(self, key, default=None):
            seen.append(key)
            return super().get(key, default)

    def fake_plan(dev, **kw):
        made.append(kw)
        raise Stop

    class Dev:
        type = "cuda"

    net._plans = Keys()
    monkeypatch.setattr(sdc.unet, "Plan", fake_plan)
    monkeypatch.setattr(net, "device", lambda: Dev())
    was = getattr(net, switch)
    for on in (was, not was, was):
        setattr(net, switch, on)
        with pytest.raises(Stop):
            net.entry((2, 12, 16), 2)
    k_a, k_b, k_a2 = seen
    assert k_a == k_a2 and k_a != k_b                         # part of the cache key
    assert sum(a != b for a, b in zip(k_a, k_b)) == 1 and len(k_a) == len(k_b)
    assert [kw[switch] for kw in made] == [was, not was, was]             # handed to the Plan
    # the switch changes nothing else that the Plan is built with, and the Plan is built with every switch
    assert {k: v for k, v in made[0].items() if k != switch} == {k: v for k, v in made[1].items() if k != switch}
    assert set(made[0]) == {"precision", *PLAN_SWITCHES}


def _recorded(net, shape, wino_split):
    """the call list of net's plan at precision 4 -- (name, arguments) with descriptors as bytes and device pointers blanked -- and the
    sorted sizes of its packed weight buffers"""
    plan = Plan("cpu", precision=4, wino_split=wino_split)
    x = torch.zeros(shape)
    net._build(sdc.unet._Builder(net, plan), x, torch.zeros_like(x))
    calls = [(fn.__name__, [bytes(a._obj) if ty is C.POINTER(_lib.SdcConvDesc) else None if ty is C.c_void_p else a
                            for a, ty in zip(args, fn.argtypes)]) for fn, args in plan.calls]
    return calls, sorted(dst.numel() for dst, _ in plan.repackers)


def test_c2_c3_convs_never_ask_for_the_route():
    # the 1-D and 2-D nets have no 3x3x3 conv: with the switch on their plans record the calls of a plan with the switch off -- names,
    # descriptors, scalar arguments and the sizes of the packed weight buffers -- and none of them is the split kernel
    for net, shape in ((sdc.Unet2D(dim=64, dim_mults=(1, 2), channels=3, resnet_block_groups=1), (1, 3, 16, 128)),
                       (sdc.Unet1D(dim=64, dim_mults=(1, 2), channels=12, resnet_block_groups=1), (1, 12, 128))):
        on, off = _recorded(net, shape, True), _recorded(net, shape, False)
        assert on == off and len(on[0]) > 50
        assert "sdc_conv_wino3_x3" not in [name for name, _ in on[0]]


WINO_DEFAULT = True
