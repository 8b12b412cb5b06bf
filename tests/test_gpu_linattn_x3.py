"""-m gpu: the fused LinearAttention block with its q / k projections as exact three-way bf16 splits (csrc/sdc_lablock_x3.hip, DESIGN.md
section 22).  Block level, through the C ABI with `impl` forced (sdc_linattn_block_sel / sdc_linattn_block_gn_sel) so that the routing
table cannot hide a kernel, on NaN-filled outputs: against the exact fp64 block next to the literal fp32 kernels on the same inputs, the
GroupNorm-on-load form, batch independence, repeatability, impl 0 against the bits of the commit before this change, a non-finite input."""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

from safediffcon_amd import _lib
from safediffcon_amd.engine import Plan, pack_conv_weight
from oracle.detweights import det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_BITS = os.path.join(ROOT, "tests", "golden", "linattn_x3_parent_sha256.json")

# (outer, inner, C, n, pre_mode, post_mode, tokens permuted): the cases of tests/test_gpu_linattn_f16.py
SHAPES = [
    (2, 1, 64, 64, 0, 0, False),        # one tile
    (2, 3, 64, 256, 0, -1, False),      # inner stride
    (2, 1, 64, 128, 1, 1, False),       # RMSNorm
    (5, 1, 128, 128, 0, 0, False),      # C = 128
    (2, 2, 64, 1088, 0, -1, False),     # 17 tiles: uneven splits 9 + 8
    (1, 2, 128, 1024, 0, -1, False),    # C = 128, two splits
    (2, 2, 64, 1088, 0, -1, True),      # row d = 0 of head 0's k ascends along the sequence: the running maximum moves in every tile
]
_ID = lambda s: "x".join(map(str, s[:6])) + ("-ascending" if len(s) > 6 and s[6] else "")      # noqa: E731
_CASE = {}


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _norm(t, g, mode, Cc, eps=1e-5):          # over the channel axis (dim 1)
    if mode == 0:
        return (t - t.mean(1, keepdim=True)) * (t.var(1, unbiased=False, keepdim=True) + eps).rsqrt() * g.view(1, -1, 1, 1)
    return torch.nn.functional.normalize(t, dim=1) * g.view(1, -1, 1, 1) * Cc ** 0.5


def _inputs(outer, inner, Cc, n, pre, post, permuted=False):
    x = det_tensor((outer, Cc, inner, n), 111)
    g1, g2 = det_tensor((Cc,), 112, 0.3) + 1.0, det_tensor((Cc,), 113, 0.3) + 1.0
    wqkv, wo, bo = det_tensor((384, Cc), 114, 0.4), det_tensor((Cc, 128), 115, 0.3), det_tensor((Cc,), 116, 0.1)
    if permuted:
        # the channel norm is per token: permuting the tokens of a sequence permutes its k rows
        k0 = torch.einsum("c,bcfn->bfn", wqkv[128].double(), _norm(x.double(), g1.double(), pre, Cc))
        order = k0.argsort(-1)[:, None].expand(outer, Cc, inner, n)
        x = x.gather(-1, order).contiguous()
    return x, g1, g2, wqkv, wo, bo


def _branch(x, g1, g2, wqkv, wo, bo, pre, post):
    """the attention branch y - x = post(Wo LA(pre(x)) + bo) in fp64 with exact operands (1D/model/unet.py:182-222, conv3d.py:232-258)"""
    B, Cc, Fr, n = x.shape
    xn = _norm(x.double(), g1.double(), pre, Cc)
    w = wqkv.double()
    q = torch.einsum("oc,bcfn->bofn", w[:128], xn).reshape(B, 4, 32, Fr, n)
    k = torch.einsum("oc,bcfn->bofn", w[128:256], xn).reshape(B, 4, 32, Fr, n)
    v = torch.einsum("oc,bcfn->bofn", w[256:], xn).reshape(B, 4, 32, Fr, n)
    ctx = torch.einsum("bhdfn,bhefn->bhfde", k.softmax(-1), v)
    T = torch.einsum("cme,bmfde->bfcmd", wo.double().reshape(Cc, 4, 32), ctx)          # T[co][head, d] per sequence
    y = torch.einsum("bfcmd,bmdfn->bcfn", T, q.softmax(2) * 32 ** -0.5) + bo.double().view(1, -1, 1, 1)
    return _norm(y, g2.double(), post, Cc) if post >= 0 else y


def _case(shape):
    """inputs and the exact fp64 branch of a shape (computed once, never modified)"""
    if shape not in _CASE:
        inp = _inputs(*shape)
        exact = _branch(*inp, shape[4], shape[5])
        _CASE[shape] = (inp, exact, exact.pow(2).mean().sqrt().item(), exact.abs().max().item())
    return _CASE[shape]


def _dev(g1, g2, wqkv, wo, bo, Cc):
    return dict(g1=g1.to(DEV), g2=g2.to(DEV), bo=bo.to(DEV), pq=pack_conv_weight(wqkv.view(384, Cc, 1)).to(DEV),
                po=pack_conv_weight(wo.view(Cc, 128, 1)).to(DEV))


def _run(impl, x_dev, d, pre, post):
    """one sdc_linattn_block_sel call on a NaN-filled output and scratch: x (outer, C, inner, n)"""
    lib = _lib.get_lib()
    outer, Cc, inner, n = x_dev.shape
    y = torch.full_like(x_dev, float("nan"))
    work = torch.full((int(lib.sdc_linattn_block_bytes(outer, inner, Cc, n)) // 4,), float("nan"), device=DEV)
    _lib.check(lib.sdc_linattn_block_sel(x_dev.data_ptr(), d["g1"].data_ptr(), d["pq"].data_ptr(), d["po"].data_ptr(), d["bo"].data_ptr(),
                                         d["g2"].data_ptr() if post >= 0 else None, work.data_ptr(), y.data_ptr(), outer, inner, Cc, n,
                                         Cc * inner * n, inner * n, n, pre, post, 1e-5, impl, _stream()), "sdc_linattn_block_sel")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
def test_linattn_x3_block_against_exact_fp64(shape):
    """the project's gate for the split kernels (DESIGN.md sections 18 and 19): the rms error of the branch y - x against the exact fp64
    block, relative to the branch's rms, at most 1.25 x the literal fp32 kernels' on the same inputs (or 2^-23); max |err| below 1e-5
    of the branch scale; two runs bit-identical"""
    (x, g1, g2, wqkv, wo, bo), exact, rms, scale = _case(shape)
    outer, inner, Cc, n, pre, post, _ = shape
    d = _dev(g1, g2, wqkv, wo, bo, Cc)
    x_dev = x.to(DEV)
    y, y32 = _run(1, x_dev, d, pre, post), _run(0, x_dev, d, pre, post)
    assert torch.isfinite(y).all() and torch.isfinite(y32).all()
    got, old = y.cpu().double() - x.double(), y32.cpu().double() - x.double()
    e_x3 = (got - exact).pow(2).mean().sqrt().item() / rms
    e_fp32 = (old - exact).pow(2).mean().sqrt().item() / rms
    e_max = (got - exact).abs().max().item() / scale
    print(f"[measured] {_ID(shape)}: rms err vs exact fp64 (of the rms of the attention branch): split {e_x3:.3e} | fp32 block {e_fp32:.3e}; "
          f"max |err| of the branch scale {e_max:.3e}")
    assert e_x3 <= max(1.25 * e_fp32, 2.0 ** -23), (e_x3, e_fp32)
    assert e_max < 1e-5, e_max
    assert torch.equal(_run(1, x_dev, d, pre, post), y)


@pytest.mark.parametrize("shape", [(3, 2, 64, 1088, 0, -1), (3, 1, 128, 128, 0, 0)], ids=_ID)
def test_linattn_x3_block_is_batch_independent(shape):
    """a sequence block's output is bit-identical alone (outer = 1) and inside outer = 3"""
    outer, inner, Cc, n, pre, post = shape
    x, g1, g2, wqkv, wo, bo = _inputs(*shape)
    d = _dev(g1, g2, wqkv, wo, bo, Cc)
    x_dev = x.to(DEV)
    y = _run(1, x_dev, d, pre, post)
    assert torch.isfinite(y).all()
    for b in range(outer):
        assert torch.equal(_run(1, x_dev[b:b + 1].contiguous(), d, pre, post)[0], y[b]), b


@pytest.mark.parametrize("shape", [(48, 4, 64, 1024, 0, -1), (48, 2, 128, 512, 0, 0)], ids=_ID)
def test_linattn_x3_block_repeats_with_every_cu_busy(shape):
    """two runs bit-identical, and sequence block 0 alone == inside the batch, at a size that puts two workgroups on every CU and several
    tiles into each workgroup of pass 2 (192 / 96 sequences of 16 / 8 tiles).  The small cases above cannot see a read of a matrix-core
    result that is only sometimes late: an inline-asm maximum straight behind the bf16 MFMAs passed them and differed from run to run
    in the last bits at this size."""
    outer, inner, Cc, n, pre, post = shape
    x, g1, g2, wqkv, wo, bo = _inputs(*shape)
    d = _dev(g1, g2, wqkv, wo, bo, Cc)
    x_dev = x.to(DEV)
    y = _run(1, x_dev, d, pre, post)
    assert torch.isfinite(y).all()
    for _ in range(3):
        assert torch.equal(_run(1, x_dev, d, pre, post), y)
    assert torch.equal(_run(1, x_dev[:1].contiguous(), d, pre, post)[0], y[0])


def _forced(plan, impl):
    """the plan's sdc_linattn_block / sdc_linattn_block_gn calls re-pointed at the _sel entries with `impl` (in front of the stream)"""
    lib = _lib.get_lib()
    sel = {"sdc_linattn_block": lib.sdc_linattn_block_sel, "sdc_linattn_block_gn": lib.sdc_linattn_block_gn_sel}
    hit = 0
    for i, (fn, args) in enumerate(plan.calls):
        if fn.__name__ in sel:
            f = sel[fn.__name__]
            call = lambda *a, f=f: f(*a[:-1], impl, a[-1])      # noqa: E731
            call.__name__ = f.__name__
            plan.calls[i] = (call, args)
            hit += 1
    return hit


@pytest.mark.parametrize("Cc,F_,hw,res", [(64, 3, (16, 16), True), (128, 2, (8, 16), True), (64, 1, (8, 8), False)])
def test_linattn_x3_block_with_groupnorm_on_load(Cc, F_, hw, res):
    """sdc_linattn_block_gn_sel(impl 1) == sdc_gn_stats + sdc_gn_apply followed by sdc_linattn_block_sel(impl 1), bit for bit (the shapes
    and inputs of test_linattn_block_with_groupnorm_on_load)"""
    B, G = 2, 8
    H, W = hw
    x = det_tensor((B, Cc, F_, H, W), 501).to(DEV)
    r = det_tensor((B, Cc, F_, H, W), 502).to(DEV) if res else None
    gam, bet = (1 + 0.2 * det_tensor((Cc,), 503)).to(DEV), (0.1 * det_tensor((Cc,), 504)).to(DEV)
    g_pre = (1 + 0.1 * det_tensor((Cc,), 505)).to(DEV)
    outs = []
    for fused in (True, False):
        plan = Plan(DEV)
        wqkv = plan.conv_weight(det_tensor((384, Cc, 1, 1), 506, 0.1).to(DEV))
        wo = plan.conv_weight(det_tensor((Cc, 128, 1, 1), 507, 0.1).to(DEV))
        bo = (0.1 * det_tensor((Cc,), 508)).to(DEV)
        xx = x.clone()
        n = H * W
        strides = (Cc * F_ * n, F_ * n, n)
        if fused:
            st = plan.gn_stats_deferred(xx, G)
            y = plan.linattn_block(xx, g_pre, wqkv, wo, bo, None, B, F_, n, strides, 0, -1, gn=(st, gam, bet, G, r))
        else:
            h = plan.gn_silu(xx, gam, bet, G, residual=r)
            y = plan.linattn_block(h, g_pre, wqkv, wo, bo, None, B, F_, n, strides, 0, -1)
        assert [fn.__name__ for fn, _ in plan.calls][-1] == ("sdc_linattn_block_gn" if fused else "sdc_linattn_block")
        assert _forced(plan, 1) == 1
        y.fill_(float("nan"))
        plan.run(_stream())
        torch.cuda.synchronize()
        outs.append(y.clone())
        assert torch.isfinite(y).all()
    assert torch.equal(outs[0], outs[1])


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


_PARENT_CHILD = """
import hashlib, json, sys
sys.path.insert(0, {root!r})
from safediffcon_amd import _lib
_lib.use_library({lib!r})
for name in ("sdc_linattn_block_sel", "sdc_linattn_block_gn_sel", "sdc_linattn_block_x3_ok"):      # entries that commit does not have
    _lib.SIGNATURES.pop(name)
import torch
sys.path.insert(0, {tests!r})
import test_gpu_linattn_x3 as T
out = {{}}
for shape in T.SHAPES[:6]:
    x, g1, g2, wqkv, wo, bo = T._inputs(*shape)
    d = T._dev(g1, g2, wqkv, wo, bo, shape[2])
    out[T._ID(shape)] = T._sha(T._run_entry(x.to(T.DEV), d, shape[4], shape[5]))
print("PARENT_BITS " + json.dumps(out))
"""


def _run_entry(x_dev, d, pre, post):
    """sdc_linattn_block itself (the entry a library of the commit before this change has) on a NaN-filled output"""
    lib = _lib.get_lib()
    outer, Cc, inner, n = x_dev.shape
    y = torch.full_like(x_dev, float("nan"))
    work = torch.full((int(lib.sdc_linattn_block_bytes(outer, inner, Cc, n)) // 4,), float("nan"), device=DEV)
    _lib.check(lib.sdc_linattn_block(x_dev.data_ptr(), d["g1"].data_ptr(), d["pq"].data_ptr(), d["po"].data_ptr(), d["bo"].data_ptr(),
                                     d["g2"].data_ptr() if post >= 0 else None, work.data_ptr(), y.data_ptr(), outer, inner, Cc, n,
                                     Cc * inner * n, inner * n, n, pre, post, 1e-5, _stream()), "sdc_linattn_block")
    torch.cuda.synchronize()
    return y


def parent_bits(parent_lib):
    """sha256 of sdc_linattn_block's output on the first six SHAPES from another build of the library (the commit before this change),
    loaded in a child process through _lib.use_library"""
    src = _PARENT_CHILD.format(root=ROOT, lib=os.path.abspath(parent_lib), tests=os.path.join(ROOT, "tests"))
    res = subprocess.run([sys.executable, "-c", src], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    line = next(ln for ln in res.stdout.splitlines() if ln.startswith("PARENT_BITS "))
    return json.loads(line[len("PARENT_BITS "):])


def test_linattn_x3_impl0_has_the_parent_commits_bits():
    """impl 0 == the output of the commit before this change, bit for bit.  The parent's bits are the sha256 of its sdc_linattn_block
    outputs on the first six SHAPES, recorded from a library built from that commit and loaded in a child process through
    _lib.use_library (parent_bits above; tests/golden/linattn_x3_parent_sha256.json -- a clean checkout has no parent library to
    build).  With SDC_PARENT_LIB naming such a library the child process runs again and must reproduce the record."""
    with open(PARENT_BITS) as fh:
        want = json.load(fh)["sha256"]
    lib_path = os.environ.get("SDC_PARENT_LIB")
    if lib_path:
        assert parent_bits(lib_path) == want
    assert len(want) == 6
    for shape in SHAPES[:6]:
        x, g1, g2, wqkv, wo, bo = _inputs(*shape)
        d = _dev(g1, g2, wqkv, wo, bo, shape[2])
        assert _sha(_run(0, x.to(DEV), d, shape[4], shape[5])) == want[_ID(shape)], _ID(shape)


def test_linattn_x3_block_non_finite_input():
    """one non-finite x value makes its own sequence non-finite (the softmax over tokens ties a sequence's tokens) and leaves every other
    sequence's bits as they are.  NaN -- the residual of the split is inf - inf -- where the fp32 block may give an infinity."""
    shape = (2, 2, 64, 256, 0, -1)
    outer, inner, Cc, n, pre, post = shape
    x, g1, g2, wqkv, wo, bo = _inputs(*shape)
    d = _dev(g1, g2, wqkv, wo, bo, Cc)
    y0 = _run(1, x.to(DEV), d, pre, post)
    assert torch.isfinite(y0).all()
    for bad in (float("inf"), float("nan")):
        xb = x.clone()
        xb[1, 5, 0, 77] = bad
        y = _run(1, xb.to(DEV), d, pre, post)
        hit = torch.zeros(outer, inner, dtype=torch.bool)
        hit[1, 0] = True
        for o in range(outer):
            for i in range(inner):
                if hit[o, i]:
                    # its token in every channel (the channel norm), and through the context every token of the sequence
                    assert not torch.isfinite(y[o, :, i]).any()
                    assert torch.isnan(y[o, :, i, 77]).all()
                else:
                    assert torch.equal(y[o, :, i], y0[o, :, i]), (o, i)
