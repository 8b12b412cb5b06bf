"""-m gpu: sdc.FusedOptimizer (sdc_optim_step: gradient norm + clip + SGD / Adam / AdamW + EMA twin in three launches) against
torch's own CPU optimizers in float64 with clip_grad_norm_ in float64 -- an independent implementation.

Oracle: a ONE-step fp64 replay started from the kernel's own fp32 state before that step.  Tolerance, per array (each of p, m, v,
ema of each item): max|err| / max|x| at most 4 x the same metric of torch's fp32 CPU optimizer against the fp64 one from the
same state (the reference's own error, measured here), floor 2^-23; the factor 4 covers the kernel's different operation order.
Every test prints what it measured (`pytest -s`)."""
import copy
import ctypes as C

import pytest
import torch

import safediffcon_amd as sdc
from safediffcon_amd import _lib
from safediffcon_amd._lib import SdcOptItem
from oracle.detweights import det_params, det_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2.0 ** -23
LRS = [1e-3, 7e-4, 1.3e-3, 5e-4, 9e-4]
EMA = dict(beta=0.995, update_every=2, update_after_step=2)
KINDS = {
    "sgd": ("sgd", dict(momentum=0.9), torch.optim.SGD, dict(momentum=0.9)),
    "adam999": ("adam", dict(betas=(0.9, 0.999)), torch.optim.Adam, dict(betas=(0.9, 0.999))),
    "adam99": ("adam", dict(betas=(0.9, 0.99)), torch.optim.Adam, dict(betas=(0.9, 0.99))),
    "adamw": ("adamw", dict(weight_decay=0.01), torch.optim.AdamW, dict(weight_decay=0.01)),
}


def _plan_numbers():
    items = (SdcOptItem * 1)()
    items[0].p, items[0].g, items[0].m, items[0].v, items[0].n = 256, 512, 768, 1024, 1
    chunk, total, grid = C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.get_lib().sdc_optim_plan(items, 1, 1, C.byref(chunk), C.byref(total), C.byref(grid)), "sdc_optim_plan")
    return chunk.value


def _lengths():
    c = _plan_numbers()
    return [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 65537, c - 1, c, c + 1, 2 * c + 7]


OFFSET_ITEM = 9           # this item (1025 floats) is a view offset by one float: 4-byte aligned only


@pytest.fixture(scope="module")
def data():
    """CPU fp32 inputs, computed once and never modified: parameters ~0.05, an EMA twin, gradients of magnitude 10^((i mod 5) - 3)
    per item for five steps (total norm > 1: clipping is active)"""
    gen = torch.Generator().manual_seed(1234)
    lengths = _lengths()
    p0 = [0.05 * torch.randn(n, generator=gen) for n in lengths]
    e0 = [0.05 * torch.randn(n, generator=gen) for n in lengths]
    grads = [[10.0 ** ((i % 5) - 3) * torch.randn(n, generator=gen) for i, n in enumerate(lengths)] for _ in LRS]
    assert min(torch.sqrt(sum((g.double() ** 2).sum() for g in gs)).item() for gs in grads) > 1.0
    return dict(lengths=lengths, p0=p0, e0=e0, grads=grads)


def _dev(t, offset=False):
    """a device copy; offset: a contiguous view one float into a 16-byte aligned buffer"""
    if not offset:
        return t.to(DEV)
    buf = torch.zeros(t.numel() + 1, device=DEV)
    buf[1:].copy_(t)
    v = buf[1:]
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _setup(data, kind, ema=True, **kw):
    """params on the device (item OFFSET_ITEM misaligned), one extra parameter that never gets a gradient, an EMA twin"""
    ps = [_dev(p, i == OFFSET_ITEM) for i, p in enumerate(data["p0"])]
    extra = torch.full((37,), 0.25, device=DEV)
    name, okw = KINDS[kind][0], KINDS[kind][1]
    opt = sdc.FusedOptimizer(ps + [extra], kind=name, lr=LRS[0], **okw, **kw)
    es = None
    if ema:
        es = [_dev(e, i == OFFSET_ITEM) for i, e in enumerate(data["e0"])] + [torch.full((37,), -1.0, device=DEV)]
        opt.attach_ema(es, **(ema if isinstance(ema, dict) else EMA))
    return ps, extra, es, opt


def _set_grads(ps, gs):
    for i, (p, g) in enumerate(zip(ps, gs)):
        p.grad = _dev(g, i == OFFSET_ITEM)


def _moments(opt, ps, kind):
    adam = KINDS[kind][0] != "sgd"
    m = [opt.state[p]["exp_avg" if adam else "momentum_buffer"] if p in opt.state else torch.zeros_like(p) for p in ps]
    v = [opt.state[p]["exp_avg_sq"] if p in opt.state else torch.zeros_like(p) for p in ps] if adam else None
    return m, v


def _cpu(ts):
    return None if ts is None else [t.detach().cpu().clone() for t in ts]


def _torch_step(kind, dtype, p, m, v, e, g, t, lr, clip, ema_cfg, fp64_norm=False):
    """one step of torch's CPU optimizer in `dtype` from the given state (step count t - 1): (p, m, v, ema, norm).
    fp64_norm: the fp32 run clips with the fp64 norm's coefficient (rounded to fp32) instead of clip_grad_norm_'s own fp32 norm,
    whose error over millions of elements (2.5e-4 measured at 8.4 M) would otherwise set the limit."""
    cls, kw = KINDS[kind][2], KINDS[kind][3]
    P = [x.to(dtype).clone() for x in p]
    for a, b in zip(P, g):
        a.grad = b.to(dtype).clone()
    if clip and fp64_norm and dtype != torch.float64:
        norm = torch.sqrt(sum((b.double() ** 2).sum() for b in g))
        coef = torch.clamp(clip / (norm + 1e-6), max=1.0).to(dtype)
        for a in P:
            a.grad.mul_(coef)
    else:
        norm = torch.nn.utils.clip_grad_norm_(P, clip) if clip else None
    opt = cls(P, lr=lr, foreach=False, **kw)
    for i, a in enumerate(P):
        if v is None:
            opt.state[a] = dict(momentum_buffer=m[i].to(dtype).clone())
        else:
            opt.state[a] = dict(step=torch.tensor(float(t - 1)), exp_avg=m[i].to(dtype).clone(), exp_avg_sq=v[i].to(dtype).clone())
    opt.step()
    M = [opt.state[a]["momentum_buffer" if v is None else "exp_avg"] for a in P]
    V = None if v is None else [opt.state[a]["exp_avg_sq"] for a in P]
    E = None
    if e is not None:
        E = [x.to(dtype).clone() for x in e]
        if t % ema_cfg["update_every"] == 0:
            for x, a in zip(E, P):
                if t <= ema_cfg["update_after_step"]:
                    x.copy_(a.detach())
                else:
                    x.lerp_(a.detach(), 1.0 - ema_cfg["beta"])
    return [a.detach() for a in P], M, V, E, norm


class _Worst:
    """collects, per array name, the largest kernel error, the reference's own error there and the largest error / limit"""

    def __init__(self, tag):
        self.tag, self.rows = tag, {}

    def check(self, name, item, got, ref32, ref64):
        scale = ref64.abs().max().item()
        if scale == 0.0:
            assert not got.any(), (self.tag, name, item)
            return
        ek = (got.double() - ref64).abs().max().item() / scale
        er = (ref32.double() - ref64).abs().max().item() / scale
        limit = max(4.0 * er, FLOOR)
        row = self.rows.setdefault(name, [0.0, 0.0, 0.0])
        if ek / limit > row[2]:
            row[:] = [ek, er, ek / limit]
        assert ek <= limit, f"{self.tag} {name} item {item} (n = {got.numel()}): kernel {ek:.3e}, torch fp32 {er:.3e}, limit {limit:.3e}"

    def report(self):
        for name, (ek, er, ratio) in self.rows.items():
            print(f"[measured] {self.tag} {name}: worst error/limit {ratio:.2f} (kernel {ek:.2e}, torch fp32 CPU {er:.2e}, both vs fp64, "
                  f"relative to max|x|)")


def _check_step(worst, kind, before, after, g, t, lr, clip, ema_cfg, fp64_norm=False):
    p0, m0, v0, e0 = before
    p1, m1, v1, e1 = after
    r64 = _torch_step(kind, torch.float64, p0, m0, v0, e0, g, t, lr, clip, ema_cfg)
    r32 = _torch_step(kind, torch.float32, p0, m0, v0, e0, g, t, lr, clip, ema_cfg, fp64_norm)
    for name, got, a32, a64 in (("p", p1, r32[0], r64[0]), ("m", m1, r32[1], r64[1]), ("v", v1, r32[2], r64[2]), ("ema", e1, r32[3], r64[3])):
        if got is None:
            continue
        for i, (x, y32, y64) in enumerate(zip(got, a32, a64)):
            if name == "ema" and t % ema_cfg["update_every"] != 0:
                assert torch.equal(x, e0[i]), (name, i, t)              # not touched on other steps
            else:
                worst.check(name, i, x, y32, y64)
    return r64[4]


@pytest.mark.parametrize("kind", list(KINDS))
def test_five_steps_against_fp64_torch(data, kind):
    ps, extra, es, opt = _setup(data, kind, max_grad_norm=1.0)
    worst = _Worst(kind)
    n = len(ps)
    for t, lr in enumerate(LRS, start=1):
        opt.param_groups[0]["lr"] = lr
        _set_grads(ps, data["grads"][t - 1])
        m, v = _moments(opt, ps, kind)
        before = (_cpu(ps), _cpu(m), _cpu(v), _cpu(es[:n]))
        opt.step()
        m, v = _moments(opt, ps, kind)
        after = (_cpu(ps), _cpu(m), _cpu(v), _cpu(es[:n]))
        norm64 = _check_step(worst, kind, before, after, data["grads"][t - 1], t, lr, 1.0, EMA).item()
        coef64 = min(1.0, 1.0 / (norm64 + 1e-6))
        assert coef64 < 1.0                                               # clipping is active
        assert abs(opt.grad_norm.item() - norm64) <= 1e-6 * norm64 and abs(opt.clip_coef.item() - coef64) <= 1e-6 * coef64
        assert opt.step_count.item() == t
        for i, p in enumerate(ps):                                        # .grad is not rewritten by clipping
            assert torch.equal(p.grad.cpu(), data["grads"][t - 1][i]), i
    assert torch.all(extra == 0.25) and torch.all(es[n] == -1.0) and extra not in opt.state     # no gradient: untouched
    worst.report()


def test_grid_cap_more_chunks_than_workgroups(data):
    """one item with more chunks than the plan's grid cap (the chunks are grid-strided), one small item behind it"""
    c = _plan_numbers()
    gen = torch.Generator().manual_seed(77)
    big = 2051 * c + 5
    p0 = [0.05 * torch.randn(big, generator=gen), 0.05 * torch.randn(6, generator=gen)]
    g0 = [1e-3 * torch.randn(big, generator=gen), 1e-1 * torch.randn(6, generator=gen)]
    e0 = [x * 0.5 for x in p0]
    ps, es = [x.to(DEV) for x in p0], [x.to(DEV) for x in e0]
    cfg = dict(beta=0.995, update_every=1, update_after_step=0)
    opt = sdc.FusedOptimizer(ps, kind="adam", lr=1e-3, betas=(0.9, 0.99), max_grad_norm=1.0)
    opt.attach_ema(es, **cfg)
    for p, g in zip(ps, g0):
        p.grad = g.to(DEV)
    opt.step()
    assert opt._plan[2] > opt._plan[3] == 2048
    zeros = [torch.zeros_like(x) for x in p0]
    m, v = _moments(opt, ps, "adam99")
    worst = _Worst("grid cap, adam99")
    norm64 = _check_step(worst, "adam99", (p0, zeros, zeros, e0), (_cpu(ps), _cpu(m), _cpu(v), _cpu(es)), g0, 1, 1e-3, 1.0, cfg,
                          fp64_norm=True).item()
    assert norm64 > 1.0 and abs(opt.grad_norm.item() - norm64) <= 1e-6 * norm64
    worst.report()


def test_bit_identical_runs_and_clip_off(data):
    def run(**kw):
        ps, _, es, opt = _setup(data, "adam999", **kw)
        for t in (1, 2):
            _set_grads(ps, data["grads"][t - 1])
            opt.step()
        m, v = _moments(opt, ps, "adam999")
        return _cpu(ps), _cpu(m), _cpu(v), _cpu(es), opt.grad_norm.item(), opt.clip_coef.item(), opt
    a, b = run(max_grad_norm=1.0), run(max_grad_norm=1.0)
    assert a[4] == b[4] and a[5] == b[5]
    for x, y in zip(a[:4], b[:4]):
        assert all(torch.equal(s, t) for s, t in zip(x, y))
    off = run()                                                           # clipping off: coef exactly 1, other numbers
    assert off[5] == 1.0 and not all(torch.equal(s, t) for s, t in zip(off[0], a[0]))
    # clip_grad_norm_() arms ONE step of an optimizer built without clipping; the tensor it returns holds the norm afterwards
    ps, _, _, opt = _setup(data, "adam999")
    _set_grads(ps, data["grads"][0])
    norm = opt.clip_grad_norm_(1.0)
    opt.step()
    want = torch.sqrt(sum((g.double() ** 2).sum() for g in data["grads"][0])).item()
    assert abs(norm.item() - want) <= 1e-6 * want and opt.clip_coef.item() < 1.0
    opt.step()
    assert opt.clip_coef.item() == 1.0
    print(f"[measured] two runs bit-identical; norm {a[4]:.6f}, coef {a[5]:.6f}; armed clip norm {norm.item():.6f} (fp64 {want:.6f})")


def test_skip_nonfinite(data):
    cfg = dict(beta=0.995, update_every=1, update_after_step=0)
    bad = [g.clone() for g in data["grads"][0]]
    bad[7][11] = float("inf")
    ps, extra, es, opt = _setup(data, "adam999", ema=cfg, max_grad_norm=1.0, skip_nonfinite=True)
    n = len(ps)
    _set_grads(ps, bad)
    opt.step()
    m, v = _moments(opt, ps, "adam999")
    assert opt.step_count.item() == 0 and not torch.isfinite(opt.grad_norm).item()
    assert all(torch.equal(p.cpu(), q) for p, q in zip(ps, data["p0"])) and all(torch.equal(e.cpu(), q) for e, q in zip(es[:n], data["e0"]))
    assert all(not x.any() for x in m) and all(not x.any() for x in v)
    # the next clean step is the optimizer's first
    _set_grads(ps, data["grads"][0])
    opt.step()
    assert opt.step_count.item() == 1
    zeros = [torch.zeros_like(x) for x in data["p0"]]
    m, v = _moments(opt, ps, "adam999")
    worst = _Worst("after a skipped step, adam999")
    _check_step(worst, "adam999", (data["p0"], zeros, zeros, data["e0"]), (_cpu(ps), _cpu(m), _cpu(v), _cpu(es[:n])), data["grads"][0], 1,
                LRS[0], 1.0, cfg)
    worst.report()
    # without the flag the Inf propagates exactly as in torch: coef 0, NaN where the Inf was
    ps, extra, es, opt = _setup(data, "adam999", ema=cfg, max_grad_norm=1.0)
    _set_grads(ps, bad)
    opt.step()
    ref = _torch_step("adam999", torch.float64, data["p0"], zeros, zeros, data["e0"], bad, 1, LRS[0], 1.0, cfg)
    assert opt.step_count.item() == 1 and sum(int(torch.isnan(r).sum()) for r in ref[0]) >= 1
    for i, (p, r) in enumerate(zip(ps, ref[0])):
        p = p.cpu()
        assert torch.equal(torch.isnan(p), torch.isnan(r)), i
        ok = ~torch.isnan(r)
        assert (p[ok].double() - r[ok]).abs().max().item() <= FLOOR * r[ok].abs().max().item() if ok.any() else True


@pytest.mark.parametrize("kind", ["adam999", "sgd"])
def test_state_dict_round_trip_with_torch(data, kind):
    """FusedOptimizer -> torch.optim -> one step each on the same gradients, and the reverse: moments and step count carry over.
    Limit: the per-array tolerance of this file, from the fp64 replay of the same step."""
    cls, kw = KINDS[kind][2], KINDS[kind][3]
    adam = kind != "sgd"
    g1, g2, g3 = data["grads"][0], data["grads"][1], data["grads"][2]

    def agree(tag, got, want, state, t):
        r64 = _torch_step(kind, torch.float64, *state, None, g3, t, LRS[0], 0.0, EMA)
        r32 = _torch_step(kind, torch.float32, *state, None, g3, t, LRS[0], 0.0, EMA)
        worst = _Worst(tag)
        for i, (a, b) in enumerate(zip(got, want)):
            scale = r64[0][i].abs().max().item()
            limit = max(4.0 * (r32[0][i].double() - r64[0][i]).abs().max().item() / scale, FLOOR)
            d = (a.double() - b.double()).abs().max().item() / scale
            assert d <= limit, (tag, i, d, limit)
            worst.check("p", i, a, r32[0][i], r64[0][i])
        worst.report()

    # forward: two fused steps, then the state moves into torch's class
    ps, _, _, opt = _setup(data, kind, ema=False)
    for g in (g1, g2):
        _set_grads(ps, g)
        opt.step()
    m, v = _moments(opt, ps, kind)
    state = (_cpu(ps), _cpu(m), _cpu(v))
    qs = [p.detach().clone() for p in ps]
    topt = cls(qs + [torch.full((37,), 0.25, device=DEV)], lr=LRS[0], **kw)
    topt.load_state_dict(copy.deepcopy(opt.state_dict()))
    if adam:
        assert all(float(st["step"]) == 2.0 for st in topt.state.values())
    _set_grads(ps, g3)
    _set_grads(qs, g3)
    opt.step()
    topt.step()
    agree(f"{kind} fused -> torch", _cpu(ps), _cpu(qs), state, 3)

    # reverse: two torch steps, then the state moves into FusedOptimizer
    qs = [_dev(p) for p in data["p0"]]
    topt = cls(qs, lr=LRS[0], **kw)
    for g in (g1, g2):
        _set_grads(qs, g)
        topt.step()
    ps = [q.detach().clone() for q in qs]
    opt = sdc.FusedOptimizer(ps, kind=KINDS[kind][0], lr=LRS[0], **KINDS[kind][1])
    opt.load_state_dict(copy.deepcopy(topt.state_dict()))
    assert opt.step_count.item() == (2 if adam else 0)
    m, v = _moments(opt, ps, kind)
    state = (_cpu(ps), _cpu(m), _cpu(v))
    _set_grads(ps, g3)
    _set_grads(qs, g3)
    opt.step()
    topt.step()
    agree(f"{kind} torch -> fused", _cpu(ps), _cpu(qs), state, 3)


def test_rejects_what_it_does_not_run():
    with pytest.raises(RuntimeError):
        sdc.FusedOptimizer([torch.zeros(4)], lr=1e-3)                                     # CPU
    with pytest.raises(RuntimeError):
        sdc.FusedOptimizer([torch.zeros(4, device=DEV, dtype=torch.float64)], lr=1e-3)    # not fp32
    with pytest.raises(RuntimeError):
        sdc.FusedOptimizer([torch.zeros(4, 4, device=DEV).t()], lr=1e-3)                  # not contiguous
    with pytest.raises(RuntimeError):
        sdc.FusedOptimizer([dict(params=[torch.zeros(4, device=DEV)]), dict(params=[torch.zeros(4, device=DEV)])], lr=1e-3)
    opt = sdc.FusedOptimizer([torch.zeros(4, device=DEV)], lr=1e-3)
    with pytest.raises(RuntimeError):
        opt.attach_ema([torch.zeros(5, device=DEV)])


def test_graphed_loss_step_with_fused_optimizer_is_bit_identical_to_eager():
    """GraphedLossStep(optimizer=FusedOptimizer(adam, max_grad_norm=1) + EMA twin): three replays with the learning rate changed
    between them through param_groups, against three eager backward + step iterations of a twin net: the same kernels with the
    hyper-parameters and the step counter read from device memory, so parameters, moments and EMA are bit-identical; the first
    replay is the optimizer's step 1 (the warm-up step is undone, EMA twin included); the next sampler call sees the new weights."""
    def make():
        net = sdc.Unet2D(dim=8, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1)
        net.load_state_dict(det_params([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 100))
        gd = sdc.GaussianDiffusionBurgers(net.to(DEV), seq_length=(16, 128), timesteps=1000, temporal=True, use_conv2d=True,
                                          is_condition_u0=True, is_condition_uT=True, condition_idx=10,
                                          train_on_padded_locations=False).to(DEV)
        params = [p for p in net.parameters() if p.requires_grad]
        ema = [(0.5 * p.detach()).clone() for p in params]
        opt = sdc.FusedOptimizer(params, kind="adam", lr=1e-4, betas=(0.9, 0.99), max_grad_norm=1.0)
        opt.attach_ema(ema, beta=0.995, update_every=1, update_after_step=0)          # every step: the warm-up step touches it too
        return net, gd, params, ema, opt
    (net_a, gd_a, pa, ea, opt_a), (net_b, gd_b, pb, eb, opt_b) = make(), make()
    B = 3
    state, noise = det_tensor((B, 3, 16, 128), 5000, 0.3).to(DEV), det_tensor((B, 3, 16, 128), 5001).to(DEV)
    w = (det_tensor((B,), 5002, 0.2) + 1.0).to(DEV)
    t = torch.tensor([3, 500, 900], device=DEV)
    x, tt = det_tensor((2, 3, 16, 128), 5003).to(DEV), torch.tensor([7, 600], device=DEV)
    with torch.no_grad():
        out0 = net_a(x, tt).clone()
    step = sdc.GraphedLossStep(gd_a, state, weight=w, t=t, noise=noise, optimizer=opt_a)
    assert opt_a.step_count.item() == 0
    assert all(torch.equal(a, b) for a, b in zip(pa, pb)) and all(torch.equal(a, b) for a, b in zip(ea, eb))
    losses = []
    for i, lr in enumerate((1e-4, 3e-4, 5e-5), start=1):
        opt_a.param_groups[0]["lr"] = lr
        opt_b.param_groups[0]["lr"] = lr
        losses.append(step(state, w, t, noise).item())
        for p in pb:
            p.grad = None
        (w * gd_b.p_losses(state, t, noise=noise, mean=False)).mean().backward()
        opt_b.step()
        assert opt_a.step_count.item() == i == opt_b.step_count.item()
        assert torch.equal(opt_a.grad_norm, opt_b.grad_norm) and torch.equal(opt_a.clip_coef, opt_b.clip_coef)
        for a, b in zip(pa, pb):
            assert torch.equal(a, b)
            assert torch.equal(opt_a.state[a]["exp_avg"], opt_b.state[b]["exp_avg"])
            assert torch.equal(opt_a.state[a]["exp_avg_sq"], opt_b.state[b]["exp_avg_sq"])
        assert all(torch.equal(a, b) for a, b in zip(ea, eb))
    with torch.no_grad():
        out_a, out_b = net_a(x, tt), net_b(x, tt)
    assert torch.equal(out_a, out_b) and not torch.equal(out_a, out0)
    print(f"[measured] captured FusedOptimizer vs eager, 3 steps bit-identical: losses {losses}, grad norm {opt_a.grad_norm.item():.4f}, "
          f"clip coef {opt_a.clip_coef.item():.4f}, max|eps change| {(out_a - out0).abs().max().item():.2e}")
    step.close()
