"""-m gpu: conv_pw_x3_kernel (csrc/sdc_conv_pw_x3.hip) -- the 1x1x1 stride-1 convs over a dense layout as exact
three-way bf16 operand splits with LDS-resident weights: fp32 in, fp32 accumulation, fp32 out.  Conv level, through the direct entry
sdc_conv_pw_x3: the error against an exact-operand fp64 conv next to that of the fp32 kernel (sdc_conv at precision 0) on the same inputs,
determinism, batch invariance, bias, power-of-two scaling invariance, the persistent tile walk, a non-finite input, the descriptors the
kernel does not cover.  Routing: sdc_conv on a listed shape is this kernel bit for bit at precision 4 and at 0 (the code every plan
records for a 1x1x1 conv, so the field cannot tell a precision-4 plan from another), at precision 2 and 3 the fp32 kernel, whatever the
batch.  Net level: graph replay, repeatability and batch invariance of the wide smoke net at 64 x 64."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import safediffcon_amd as sdc
from safediffcon_amd import _lib
from safediffcon_amd.engine import conv_desc, pack_conv_weight
from oracle.detweights import det_params, det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SDC_EINVAL = -1
ONE = ((1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), 0)          # taps, stride, pad, upsampling, up_mode of a pointwise conv


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


# case: B, Cin0, Cin1, Cout, (D, H, W), residual with strides of its own, y a channel slice of a wider buffer
CASES = {
    "one_block_few_tiles_bias": (2, 64, 0, 128, (2, 8, 32), False, False),        # 16 wave tiles: fewer than one per workgroup
    "ragged_residual_own_strides": (3, 128, 0, 128, (1, 5, 36), True, False),     # 180 positions per sample, ragged last tile
    "three_cout_blocks": (2, 128, 0, 384, (2, 4, 16), False, False),
    "k256_narrow_block": (1, 256, 0, 384, (2, 4, 16), False, False),              # 64-wide weight blocks
    "two_inputs_64": (2, 64, 64, 64, (1, 8, 64), False, False),
    "two_inputs_128": (1, 128, 128, 64, (2, 4, 32), False, False),
    "y_channel_slice": (1, 128, 0, 256, (2, 4, 16), False, True),
}
_CASE = {}


def _case(name):
    """inputs and the exact-operand fp64 reference without the residual (computed once per case, never modified)"""
    if name not in _CASE:
        B, c0, c1, co, sp, has_res, _ = CASES[name]
        g = torch.Generator().manual_seed(17)
        x0 = torch.randn(B, c0, *sp, generator=g) * 2.0
        x1 = torch.randn(B, c1, *sp, generator=g) * 2.0 if c1 else None
        w = torch.randn(co, c0 + c1, 1, 1, 1, generator=g) / (3.0 * (c0 + c1) ** 0.5)
        bias = 0.1 * torch.randn(co, generator=g)
        res = torch.randn(B, co + 8, *sp, generator=g) if has_res else None      # the residual: channels 4 .. co + 4 of a wider tensor
        ref = F.conv3d((x0 if x1 is None else torch.cat((x0, x1), 1)).double(), w.double(), bias.double())
        _CASE[name] = (x0, x1, w, bias, res, ref)
    return _CASE[name]


def _run(name, fn, x0, x1, wp, bias, res, precision=0):
    """one launch of `fn` (sdc_conv_pw_x3 or sdc_conv) into a NaN-filled output; returns the output view"""
    lib = _lib.get_lib()
    co, slice_y = CASES[name][3], CASES[name][6]
    B, sp = x0.shape[0], x0.shape[2:]
    if slice_y:
        y = torch.full((B, co + 16, *sp), float("nan"), device=DEV)[:, 8:8 + co]
    else:
        y = torch.full((B, co, *sp), float("nan"), device=DEV)
    rv = None if res is None else res[:, 4:4 + co]
    d = conv_desc(x0, x1, y, rv, co, *ONE, precision)
    _lib.check(getattr(lib, fn)(C.byref(d), x0.data_ptr(), 0 if x1 is None else x1.data_ptr(), wp.data_ptr(),
                                0 if bias is None else bias.data_ptr(), 0 if rv is None else rv.data_ptr(), y.data_ptr(), _stream()), fn)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("name", list(CASES))
def test_pw_x3_conv_is_fp32_grade_and_repeatable(name):
    B, c0, c1, co, sp, has_res, _ = CASES[name]
    x0, x1, w, bias, res, ref = _case(name)
    x0d, x1d, bd = x0.to(DEV), (None if x1 is None else x1.to(DEV)), bias.to(DEV)
    resd = None if res is None else res.to(DEV)
    wp = pack_conv_weight(w, "conv", 0).to(DEV)
    full = ref if res is None else ref + res[:, 4:4 + co].double()
    rms, scale = full.pow(2).mean().sqrt().item(), full.abs().max().item()
    y = _run(name, "sdc_conv_pw_x3", x0d, x1d, wp, bd, resd)
    out = y.double().cpu()
    assert torch.isfinite(out).all()                                             # no element of the NaN-filled y left unwritten
    y32 = _run(name, "sdc_conv", x0d, x1d, wp, bd, resd).double().cpu()
    e_new, e_old = ((o - full).pow(2).mean().sqrt().item() / rms for o in (out, y32))
    m_new = (out - full).abs().max().item() / scale
    print(f"[measured] {name}: rms err vs exact fp64 (of the output rms): split {e_new:.3e} | fp32 kernel {e_old:.3e}; "
          f"max |err| of the output scale {m_new:.3e}")
    assert e_new <= max(1.25 * e_old, 2.0 ** -23), (e_new, e_old)
    assert m_new < 1e-5
    # two runs bit-identical; every sample of the batch == the same sample alone
    assert torch.equal(_run(name, "sdc_conv_pw_x3", x0d, x1d, wp, bd, resd), y)
    if B > 1:
        for b in range(B):
            alone = _run(name, "sdc_conv_pw_x3", x0d[b:b + 1], None if x1d is None else x1d[b:b + 1], wp, bd,
                         None if resd is None else resd[b:b + 1])
            assert torch.equal(alone[0], y[b]), b
    # without the residual: the bias path equals no-bias + bias, and a power of two on x scales the output bit for bit (a lost or
    # flushed third piece would not)
    yb = _run(name, "sdc_conv_pw_x3", x0d, x1d, wp, bd, None)
    y0 = _run(name, "sdc_conv_pw_x3", x0d, x1d, wp, None, None)
    assert torch.equal(y0 + bd.view(1, -1, 1, 1, 1), yb)
    for e in (40, -40):
        ys = _run(name, "sdc_conv_pw_x3", x0d * 2.0 ** e, None if x1d is None else x1d * 2.0 ** e, wp, None, None)
        assert torch.equal(ys, y0 * 2.0 ** e), e


def test_pw_x3_persistent_walk_is_deterministic():
    # 3 x 36864 positions = 1728 wave tiles of 64 (432 workgroup rounds of 256 positions): several tiles per wave on 256 CUs, every
    # tile boundary of the continuous load stream crossed many times
    lib = _lib.get_lib()
    g = torch.Generator().manual_seed(23)
    x = (torch.randn(3, 64, 4, 96, 96, generator=g) * 2.0).to(DEV)
    w = torch.randn(64, 64, 1, 1, 1, generator=g) / 24.0
    wp = pack_conv_weight(w, "conv", 0).to(DEV)

    def run(xx):
        y = torch.full((xx.shape[0], 64, 4, 96, 96), float("nan"), device=DEV)
        d = conv_desc(xx, None, y, None, 64, *ONE, 0)
        _lib.check(lib.sdc_conv_pw_x3(C.byref(d), xx.data_ptr(), 0, wp.data_ptr(), 0, 0, y.data_ptr(), _stream()), "sdc_conv_pw_x3")
        torch.cuda.synchronize()
        return y
    y = run(x)
    assert torch.isfinite(y).all()
    ref = F.conv3d(x[1:2, :, :1].double(), w.to(DEV).double())
    assert (y[1:2, :, :1].double() - ref).abs().max().item() < 1e-5 * ref.abs().max().item()
    for _ in range(3):
        assert torch.equal(run(x), y)
    for b in range(3):
        assert torch.equal(run(x[b:b + 1])[0], y[b]), b


def test_pw_x3_non_finite_input_stays_in_its_position():
    lib = _lib.get_lib()
    g = torch.Generator().manual_seed(29)
    x = torch.randn(2, 128, 2, 8, 32, generator=g).to(DEV)
    wp = pack_conv_weight(torch.randn(128, 128, 1, 1, 1, generator=g) / 11.0, "conv", 0).to(DEV)

    def run(xx):
        y = torch.full((2, 128, 2, 8, 32), float("nan"), device=DEV)
        d = conv_desc(xx, None, y, None, 128, *ONE, 0)
        _lib.check(lib.sdc_conv_pw_x3(C.byref(d), xx.data_ptr(), 0, wp.data_ptr(), 0, 0, y.data_ptr(), _stream()), "sdc_conv_pw_x3")
        torch.cuda.synchronize()
        return y
    clean = run(x)
    xi = x.clone()
    xi[1, 77, 1, 3, 21] = float("inf")
    dirty = run(xi)
    hit = torch.zeros_like(clean, dtype=torch.bool)
    hit[1, :, 1, 3, 21] = True
    assert not torch.isfinite(dirty[hit]).any()                                   # every Cout of that position is NaN or Inf
    assert torch.equal(dirty[~hit], clean[~hit])                                  # and no other position moved


def test_pw_x3_uncovered_descriptors():
    lib = _lib.get_lib()
    x = torch.zeros(1, 64, 2, 8, 32, device=DEV)
    wp = torch.zeros(3 * 512 * 128, device=DEV)

    def refused(xx, x1, y, cout, k=(1, 1, 1), stride=(1, 1, 1), pad=(0, 0, 0)):
        d = conv_desc(xx, x1, y, None, cout, k, stride, pad, (1, 1, 1), 0, 4)
        assert lib.sdc_conv_pw_x3_ok(C.byref(d)) == 0
        assert lib.sdc_conv_pw_x3(C.byref(d), xx.data_ptr(), 0 if x1 is None else x1.data_ptr(), wp.data_ptr(), 0, 0, y.data_ptr(),
                                  _stream()) == SDC_EINVAL
        torch.cuda.synchronize()
        assert torch.isnan(y).all()                                               # nothing was launched

    def nan(*shape):
        return torch.full(shape, float("nan"), device=DEV)
    refused(x, None, nan(1, 64, 2, 4, 16), 64, stride=(1, 2, 2))                  # stride 2
    refused(x, None, nan(1, 64, 2, 8, 32), 64, k=(1, 1, 3), pad=(0, 0, 1))        # a 3-tap conv
    refused(x, None, nan(1, 80, 2, 8, 32), 80)                                    # Cout not a whole number of blocks
    refused(torch.zeros(1, 64, 2, 8, 64, device=DEV)[..., ::2], None, nan(1, 64, 2, 8, 32), 64)      # x not dense
    big = torch.zeros(1, 512, 2, 8, 32, device=DEV)
    refused(big, None, nan(1, 64, 2, 8, 32), 64)                                  # K = 512: no weight block fits the LDS
    refused(big[:, :256], big[:, 256:], nan(1, 128, 2, 8, 32), 128)               # the same K from two inputs
    # (the covered descriptor runs)
    y = nan(1, 64, 2, 8, 32)
    d = conv_desc(x, None, y, None, 64, *ONE, 4)
    _lib.check(lib.sdc_conv_pw_x3(C.byref(d), x.data_ptr(), 0, wp.data_ptr(), 0, 0, y.data_ptr(), _stream()), "sdc_conv_pw_x3")
    torch.cuda.synchronize()
    assert (y == 0).all()


def _describe(d):
    name, share = C.create_string_buffer(96), C.c_double(-1.0)
    _lib.check(_lib.get_lib().sdc_conv_describe(C.byref(d), name, 96, C.byref(share)), "sdc_conv_describe")
    return name.value.decode(), share.value


def test_pw_x3_routing_by_precision_not_by_batch():
    lib = _lib.get_lib()
    g = torch.Generator().manual_seed(31)
    x = (torch.randn(3, 128, 32, 16, 16, generator=g) * 2.0).to(DEV)             # 128 -> 256 over 32 x 16 x 16: a listed per-sample shape
    w = torch.randn(256, 128, 1, 1, 1, generator=g) / 34.0
    bias = (0.1 * torch.randn(256, generator=g)).to(DEV)

    def run(fn, xx, prec):
        wp = pack_conv_weight(w, "conv", prec).to(DEV)
        y = torch.full((xx.shape[0], 256, 32, 16, 16), float("nan"), device=DEV)
        d = conv_desc(xx, None, y, None, 256, *ONE, prec)
        _lib.check(getattr(lib, fn)(C.byref(d), xx.data_ptr(), 0, wp.data_ptr(), bias.data_ptr(), 0, y.data_ptr(), _stream()), fn)
        torch.cuda.synchronize()
        return y, d
    direct, d4 = run("sdc_conv_pw_x3", x[:1], 4)
    routed, _ = run("sdc_conv", x[:1], 4)
    assert lib.sdc_conv_pw_x3_ok(C.byref(d4)) == 1
    assert torch.equal(routed, direct)
    assert _describe(d4) == ("conv_pw_x3_kernel<4,2>", 0.0)
    # precision 0 is what every plan writes into a 1x1x1 descriptor, whatever its own precision (engine.conv_precision: the lowest
    # layout code; pinned by tests/test_host_plan_record.py): it routes like 4.  2 and 3 keep the fp32 kernel's name and bits
    y0, d0 = run("sdc_conv", x[:1], 0)
    assert torch.equal(y0, direct) and _describe(d0) == ("conv_pw_x3_kernel<4,2>", 0.0)
    y2, d2 = run("sdc_conv", x[:1], 2)
    y3, d3 = run("sdc_conv", x[:1], 3)
    for d in (d2, d3):
        name, share = _describe(d)
        assert name.startswith("conv_pw") and "x3" not in name and share == 1.0
    assert torch.equal(y2, y3) and not torch.equal(y3, direct)
    ref = F.conv3d(x[:1].double(), w.to(DEV).double(), bias.double())
    e3, e4 = ((y.double() - ref).pow(2).mean().sqrt().item() for y in (y3, direct))
    print(f"[measured] 128->256 at 32x16x16: rms err vs exact fp64: fp32 kernel {e3:.3e} | split {e4:.3e}")
    assert e4 <= max(1.25 * e3, 2.0 ** -23 * ref.pow(2).mean().sqrt().item())
    # B = 3: the same route, and every sample's bits are those of the sample alone
    routed3, d43 = run("sdc_conv", x, 4)
    assert lib.sdc_conv_pw_x3_ok(C.byref(d43)) == 1 and _describe(d43)[0] == "conv_pw_x3_kernel<4,2>"
    assert torch.equal(routed3[:1], direct)
    assert torch.equal(run("sdc_conv_pw_x3", x, 4)[0], routed3)


def test_pw_x3_wide_smoke_net_replay_and_batch_invariance(golden):
    g = golden("smoke_unet_wide")
    net = sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7)
    net.load_state_dict(det_params(g.spec(), int(g.scalar("weight_seed"))))
    net.to(DEV)
    x, t = det_tensor((1, 32, 7, 64, 64), 41).to(DEV), g["t"].to(DEV)[:1]
    lib = _lib.get_lib()
    plan = net.entry(tuple(x.shape), 1)["plan"]
    assert sum(1 for fn, a in plan.calls if fn.__name__ == "sdc_conv" and lib.sdc_conv_pw_x3_ok(a[0])) > 0      # the table is in play
    net.forward_graph = True
    eps = net(x, t).clone()
    assert torch.isfinite(eps).all()
    assert torch.equal(net(x, t), eps)
    net.forward_graph = False
    assert torch.equal(net(x, t), eps)                                            # graph replay == eager
    net.forward_graph = True
    x2, t2 = torch.cat([x, x.flip(-1)]), torch.cat([t, t])
    assert torch.equal(net(x2, t2)[:1], eps)                                      # the sample inside a batch of two == alone
