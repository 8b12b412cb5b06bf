"""CPU: the recorded call list of the sampler plans, pinned to tests/golden/plan_calls.json.

Plan("cpu", ...) with _Builder(net, plan) and net._build(b, x, eps) records a whole net's call list without a GPU: the library loads, the
routing tables are host code.  A record holds, per configuration, every call -- the function name, every SdcConvDesc's bytes, every
non-pointer argument's value and every pointer as a token -- the sizes of all packed weight buffers and the conditioning sites.  The
fixture keeps the function names (so a failure reads as a diff) and one sha256 over the whole record.  A host-side change that moves a
conv to another kernel, packs a buffer it did not pack before, or changes an argument, a stride or the aliasing of the activations, shows.

Weights are small dyadic numbers (integers in [-8, 8] divided by 8): the tap merges, the Winograd G transforms and the fp16 / bf16
roundings of the packers are then exact in any summation order, so the packed bytes do not depend on the machine.  Precision 5's F(4,3)
matrix has thirds in it: there the buffers are identified by their sizes.  The rotary frequencies are zero (cos 1, sin 0, exact).

`python tests/test_host_plan_record.py` rewrites the fixture from the checked-out code."""
import bisect
import ctypes as C
import functools
import hashlib
import inspect
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import safediffcon_amd as sdc  # noqa: E402
from safediffcon_amd._lib import SdcConvDesc  # noqa: E402
from safediffcon_amd import _lib  # noqa: E402
from safediffcon_amd.engine import Plan, WeightSrc, pack_gemm_x3, pack_conv_weight, pack_stem_x3, pack_wino3_x3  # noqa: E402
from safediffcon_amd.unet import _Builder  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_calls.json")

# the production nets whose shapes the routing tables key on; C3 at a quarter of its width (its 225 M parameters take a minute to pack)
NETS = {
    "c4": (lambda: sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7), (32, 7, 64, 64)),
    "c2": (lambda: sdc.Unet2D(dim=64, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1), (3, 16, 128)),
    "c3": (lambda: sdc.Unet1D(dim=64, dim_mults=(1, 2, 4, 8), channels=12, resnet_block_groups=1), (12, 128)),
}
# the switches a Plan is constructed with (everything after device and precision), read from the net like entry() does
SWITCHES = tuple(n for n in inspect.signature(Plan.__init__).parameters if n not in ("self", "device", "precision"))
F16 = tuple(n for n in SWITCHES if n.endswith("_f16"))
OFF = dict.fromkeys(SWITCHES, False)
# name -> (net, batch, net attributes set on top of the net's defaults)
CONFIGS = {
    "c4_default": ("c4", 1, {}),
    "c2_default": ("c2", 1, {}),
    "c3_default": ("c3", 1, {}),
    "c4_all_off": ("c4", 1, OFF),
    "c4_p0_splits_on": ("c4", 1, dict(precision=0)),
    "c4_p3_splits_on": ("c4", 1, dict(precision=3)),
    "c4_p5_splits_on": ("c4", 1, dict(precision=5)),
    "c4_p6_splits_on": ("c4", 1, dict(precision=6)),
    "c3_p5_splits_on": ("c3", 1, dict(precision=5)),
    "c4_f16_alone": ("c4", 1, dict(OFF, **dict.fromkeys(F16, True))),
    "c4_f16_wins_over_splits": ("c4", 1, dict.fromkeys(SWITCHES, True)),
    "c2_f16_wins_over_splits": ("c2", 1, dict.fromkeys(SWITCHES, True)),
    "c4_unfused_linattn": ("c4", 1, dict(fuse_linattn=False)),
    "c3_split_small_grids_b16": ("c3", 16, dict(split_small_grids=True)),
}
# every alternate kernel of the plans is recorded by at least one configuration: a route that nothing exercises is not pinned
EXERCISED = ("sdc_conv_stem_f16", "sdc_conv_stem_x3", "sdc_conv_gemm_x3", "sdc_conv_wino3_x3", "sdc_tattn_block_f16",
             "sdc_tattn_block_x3", "sdc_linattn_block_f16", "sdc_linattn_block_gn_f16", "sdc_conv_splitk")


@functools.lru_cache(maxsize=None)
def _net(kind):
    net = NETS[kind][0]()
    with torch.no_grad():
        for i, (name, p) in enumerate(net.named_parameters()):
            if name.endswith("rotary_emb.freqs"):
                p.zero_()
                continue
            j = torch.arange(p.numel(), dtype=torch.int64)
            p.copy_((((j * j * 31 + j * 7 + i * 13) % 17 - 8).to(torch.float32) / 8).reshape(p.shape))
    net._defaults = {k: v for k, v in vars(net).items() if isinstance(v, (bool, int)) and not k.startswith("_")}
    return net


def record(name):
    """(function names, sha256 of the full record) of configuration `name`"""
    kind, batch, attrs = CONFIGS[name]
    net = _net(kind)
    for k, v in dict(net._defaults, **attrs).items():
        setattr(net, k, v)
    # the plan as entry() constructs it
    plan = Plan("cpu", precision=net.precision, **{n: bool(getattr(net, n)) for n in SWITCHES})
    plan.split_small_grids = bool(net.split_small_grids)
    x = torch.zeros((batch, *NETS[kind][1]), dtype=torch.float32)
    eps = torch.zeros_like(x)
    b = _Builder(net, plan)
    net._build(b, x, eps)

    # a pointer into a packed weight buffer: the buffer's contents (at precision 5: its size) and the offset; any other pointer: its
    # first-seen index in the call list, which pins the aliasing pattern of the activations without pinning addresses
    bufs = sorted((dst.data_ptr(), dst) for dst, _ in plan.repackers)
    starts = [s for s, _ in bufs]
    digests, seen = {}, {}

    def token(p):
        if not p:
            return 0
        i = bisect.bisect_right(starts, p) - 1
        if i >= 0 and p < starts[i] + bufs[i][1].numel() * 4:
            if i not in digests:
                t = bufs[i][1]
                digests[i] = t.numel() if plan.precision == 5 else hashlib.sha256(t.numpy()).hexdigest()
            return ["w", digests[i], p - starts[i]]
        return ["p", seen.setdefault(p, len(seen))]

    calls = []
    for fn, args in plan.calls:
        assert len(args) + 1 == len(fn.argtypes), fn.__name__          # (the stream is passed at replay)
        enc = []
        for a, ty in zip(args, fn.argtypes):
            if ty is C.POINTER(SdcConvDesc):
                enc.append(bytes(a._obj).hex())
            elif ty is C.c_void_p:
                enc.append(token(a))
            else:
                enc.append(a)
        calls.append([fn.__name__, enc])
    full = dict(calls=calls, buffers=sorted(dst.numel() for dst, _ in plan.repackers), cond_sites=[list(s) for s in b.cond_sites])
    return [c[0] for c in calls], hashlib.sha256(json.dumps(full, sort_keys=True).encode()).hexdigest()


@functools.lru_cache(maxsize=None)
def _recorded(name):
    return record(name)


@pytest.fixture(scope="module")
def plan_calls():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_lists_exactly_these_configurations(plan_calls):
    assert sorted(plan_calls) == sorted(CONFIGS)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_plan_records_the_pinned_call_list(name, plan_calls):
    names, digest = _recorded(name)
    assert names == plan_calls[name]["calls"]
    assert digest == plan_calls[name]["sha256"]


def test_every_alternate_kernel_is_recorded_somewhere():
    union = set().union(*(_recorded(name)[0] for name in CONFIGS))
    assert not [fn for fn in EXERCISED if fn not in union]


# ------------------------------------------------------------------ the fields of engine.CONV_ROUTES that no net exercises
# Direct Plan.conv calls on descriptors that the routing tables list, so that only the table's field keeps (or lets) the conv off (or on)
# the route; every test first asserts that premise.  Not pinned, because no listed descriptor has the property: the Winograd row's
# yield to split-K (its table lists one output volume, which split-K never takes), the stem rows' splitk=False (split-K takes no 7-tap
# conv), and "unshuffle" / "convT" on the gemm row (sdc_conv_gemm_x3_ok lists neither form today).
def _conv(x, w, kind, cout, k, split_small_grids=False, **kw):
    """(plan, name of the recorded conv call, its descriptor by reference) of one Plan.conv call with every split switch on"""
    plan = Plan("cpu", precision=4, stem_split=True, gemm_split=True, wino_split=True)
    plan.split_small_grids = split_small_grids
    plan.conv(x, WeightSrc(w, kind), None, cout, k, **kw)
    (fn, args), = plan.calls
    return plan, fn.__name__, args[0]


def _sizes(plan):
    return sorted(dst.numel() for dst, _ in plan.repackers)


def test_gemm_route_declines_groupnorm_sums_and_residual_and_yields_to_split_k():
    lib = _lib.get_lib()
    x, w = torch.zeros(1, 128, 1, 32, 32), torch.zeros(128, 128, 1, 4, 4)              # (1,4,4) stride 2 -> 16 x 16: a listed shape
    geom = dict(stride=(1, 2, 2), pad=(0, 1, 1))
    plan, name, d = _conv(x, w, "conv", 128, (1, 4, 4), **geom)
    assert lib.sdc_conv_gemm_x3_ok(d) == 1 and lib.sdc_conv_splitk_bytes(d) > 0        # listed, and split-K would take it
    assert name == "sdc_conv_gemm_x3"
    assert _sizes(plan) == [pack_gemm_x3(pack_conv_weight(w, "conv", 0), 128, 128, (1, 4, 4)).numel()]     # and no fp32 buffer
    fp32 = [pack_conv_weight(w, "conv", 4).numel()]
    plan, name, d = _conv(x, w, "conv", 128, (1, 4, 4), gn_groups=8, **geom)
    assert lib.sdc_conv_gemm_x3_ok(d) == 1 and name in ("sdc_conv", "sdc_conv_gn") and _sizes(plan) == fp32
    plan, name, d = _conv(x, w, "conv", 128, (1, 4, 4), residual=torch.zeros(1, 128, 1, 16, 16), **geom)
    assert name == "sdc_conv" and _sizes(plan) == fp32
    plan, name, d = _conv(x, w, "conv", 128, (1, 4, 4), split_small_grids=True, **geom)
    assert lib.sdc_conv_gemm_x3_ok(d) == 1 and name == "sdc_conv_splitk" and _sizes(plan) == fp32


def test_gemm_route_takes_the_transposed_convs_parities_and_never_the_upsampling_ones():
    lib = _lib.get_lib()
    x, out = torch.zeros(1, 64, 1, 32, 32), torch.zeros(1, 64, 1, 64, 64)
    geom = dict(pad=(0, 1, 1), out=out[:, :, :, 0::2, 0::2])
    plan, name, d = _conv(x, torch.zeros(64, 64, 1, 4, 4), ("convT_sub", 0, 0), 64, (1, 2, 2), **geom)
    assert lib.sdc_conv_gemm_x3_ok(d) == 1 and name == "sdc_conv_gemm_x3"
    # the same 2x2 stride-1 descriptor from nearest-x2 upsampling + 3x3 conv: the library would list it, the table keeps it out
    w = torch.zeros(64, 64, 3, 3)
    plan, name, d = _conv(x, w, ("up2_sub", 0, 0), 64, (1, 2, 2), **geom)
    assert lib.sdc_conv_gemm_x3_ok(d) == 1 and name == "sdc_conv"
    assert _sizes(plan) == [pack_conv_weight(w, ("up2_sub", 0, 0), 4).numel()]


def test_stem_route_ignores_groupnorm_and_winograd_route_sums_it():
    lib = _lib.get_lib()
    g, b = torch.ones(64), torch.zeros(64)
    # stem: routes with gn_groups set and registers nothing -- the GroupNorm that follows takes its own statistics
    x, w = torch.zeros(1, 7, 2, 16, 16), torch.zeros(64, 7, 7, 7, 7)
    plan, name, d = _conv(x, w, "conv", 64, (7, 7, 7), pad=(3, 3, 3), gn_groups=8)
    assert name == "sdc_conv_stem_x3" and _sizes(plan) == [pack_stem_x3(w).numel()] and not plan._gn_parts
    plan.gn_silu(torch.zeros(1, 64, 2, 16, 16), g, b, 8)
    assert "sdc_gn_finalize" not in [fn.__name__ for fn, _ in plan.calls]
    # Winograd: routes with gn_groups set, its epilogue sums feed sdc_gn_finalize; with a residual it does not route
    x, w = torch.zeros(1, 128, 32, 16, 16), torch.zeros(256, 128, 3, 3, 3)
    plan, name, d = _conv(x, w, "conv", 256, (3, 3, 3), pad=(1, 1, 1), gn_groups=8)
    assert lib.sdc_conv_wino3_x3_ok(d) == 1 and name == "sdc_conv_wino3_x3"
    assert _sizes(plan) == [pack_wino3_x3(pack_conv_weight(w, "conv", 4), 256, 128).numel()]
    (fn, args), = plan.calls
    assert args[-2] != 0 and args[-1] == 8                    # the partial-sum buffer and the group count
    y = torch.zeros(1, 256, 32, 16, 16)
    plan._gn_parts[y.data_ptr()] = plan._gn_parts.pop(next(iter(plan._gn_parts)))         # (the pool's output, stood in for by y)
    plan.gn_silu(y, torch.ones(256), torch.zeros(256), 8)
    assert [fn.__name__ for fn, _ in plan.calls][1:] == ["sdc_gn_finalize", "sdc_gn_apply"]
    plan, name, d = _conv(x, w, "conv", 256, (3, 3, 3), pad=(1, 1, 1), residual=torch.zeros(1, 256, 32, 16, 16))
    assert name == "sdc_conv"


if __name__ == "__main__":
    rows = []
    for cfg in CONFIGS:
        fns, sha = record(cfg)
        rows.append(f' "{cfg}": {{"sha256": "{sha}", "calls": {json.dumps(fns)}}}')
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(rows) + "\n}\n")
    print(f"wrote {FIXTURE}: {len(rows)} configurations")
