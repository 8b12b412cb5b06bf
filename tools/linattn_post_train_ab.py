#!/usr/bin/env python3
"""A/B of net.train_fuse_linattn on the 1-D nets: python tools/linattn_post_train_ab.py [workload: c2 | tok128] [batch] [reps]
  c2     : Unet2D(dim=64) at the Burgers state (3, 16, 128), the C2 fine-tuning step
  tok128 : Unet1D(dim=128) at the tokamak state (12, 128)

Switch off and on interleaved, `reps` repetitions each, min - max printed:
  * the fine-tuning step (loss = mean(w_b p_losses_b); loss.backward()), eager and as sdc.GraphedLossStep replay (two nets with the
    same weights, one per setting: a captured step keeps its mode)
  * forward + backward of Trainer.linattn_lucid alone at every covered site (found by one forward)
  * peak allocated memory of the eager step
The switch-off arm is the parent's chain, bit for bit.  The log kept in profiles/linattn_post_train_ab.log is this script's output,
one workload after the other."""
import _libsel  # noqa: F401,E402  (SDC_LIB_PATH -> safediffcon_amd._lib.use_library, tools only)
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import safediffcon_amd as sdc  # noqa: E402
from oracle.detweights import det_params, det_tensor  # noqa: E402
from safediffcon_amd import autograd  # noqa: E402

WORK = sys.argv[1] if len(sys.argv) > 1 else "c2"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda:0")
shape = {"c2": (3, 16, 128), "tok128": (12, 128)}[WORK]


def make(fuse):
    if WORK == "c2":
        net = sdc.Unet2D(dim=64, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=1)
    else:
        net = sdc.Unet1D(dim=128, dim_mults=(1, 2, 4, 8), channels=12, resnet_block_groups=1)
    net.load_state_dict(det_params([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 77))
    net.to(dev).train()
    net.train_fuse_linattn = fuse
    if WORK == "c2":
        gd = sdc.GaussianDiffusionBurgers(net, seq_length=(16, 128), timesteps=1000, temporal=True, use_conv2d=True, is_condition_u0=True,
                                          is_condition_uT=True, condition_idx=10, train_on_padded_locations=False)
    else:
        gd = sdc.GaussianDiffusionTokamak(net, seq_length=128, nt=122, timesteps=1000, guidance_u0=True)
    return net, gd.to(dev)


state, noise = det_tensor((B, *shape), 9, 0.3).to(dev), det_tensor((B, *shape), 10).to(dev)
w = torch.ones(B, device=dev)
t = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(3)).to(dev)
nets = {False: make(False), True: make(True)}


def eager_step(fuse):
    net, gd = nets[fuse]
    net.zero_grad(set_to_none=True)
    loss = (w * gd.p_losses(state, t, noise=noise, mean=False)).mean()
    loss.backward()
    return loss


def wall(fn, n=3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def ab(label, fns, n=3):
    for f in fns.values():
        f()                                            # warm-up
    ms = {k: [] for k in fns}
    for _ in range(REPS):
        for k, f in fns.items():                       # interleaved
            ms[k].append(wall(f, n))
    for k, v in ms.items():
        print(f"{label:38s} train_fuse_linattn={k!s:5s} ms/iter min {min(v):8.3f} max {max(v):8.3f}   ({REPS} repetitions of {n})")
    sys.stdout.flush()


print(f"# {WORK}: {type(nets[True][0]).__name__}(dim={nets[True][0].dim}) on {shape}, B = {B}; {torch.cuda.get_device_name(0)}")
sites = []
orig = autograd.Trainer.linattn_lucid
autograd.Trainer.linattn_lucid = lambda self, p, x, mode: (sites.append((p, tuple(x.shape), mode)), orig(self, p, x, mode))[1]
l_off = eager_step(False).item()
autograd.Trainer.linattn_lucid = orig
l_on = eager_step(True).item()
print(f"loss off {l_off:.7f} on {l_on:.7f}")
ab("eager step", {False: lambda: eager_step(False), True: lambda: eager_step(True)})

for fuse in (False, True):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    eager_step(fuse)
    torch.cuda.synchronize()
    print(f"eager step peak allocated above the resident state, train_fuse_linattn={fuse!s:5s}: "
          f"{(torch.cuda.max_memory_allocated() - base) / 2**20:9.1f} MiB")
for net, _ in nets.values():
    net.zero_grad(set_to_none=True)

# one covered site alone
for site, shp, mode in sites:
    n = shp[2] * shp[3] * shp[4]
    if not (shp[1] in (64, 128) and n % 64 == 0 and shp[0] < 65536):
        print(f"site {site} {shp}: outside the kernel's domain, the chain in both arms")
        continue
    routed = autograd.la_post_fusable(shp[0], shp[1], n)
    x, dy = det_tensor(shp, 20).to(dev), det_tensor(shp, 21).to(dev)

    def run(fuse, site=site, x=x, dy=dy, mode=mode):
        # the on arm applies the node itself, so that a site the routing predicate leaves to the chain is still measured
        net, _ = nets[fuse]
        T = net._trainer()
        xg = x.detach().requires_grad_()
        with T.step(dev):
            if fuse:
                y = autograd.LinAttnPostBlockFn.apply(xg, T.P(f"{site}.fn.norm.g"), T.P(f"{site}.fn.fn.to_qkv.weight"),
                                                      T.P(f"{site}.fn.fn.to_out.0.weight"), T.P(f"{site}.fn.fn.to_out.0.bias"),
                                                      T.P(f"{site}.fn.fn.to_out.1.g"), mode)
            else:
                y = T.linattn_lucid(site, xg, mode)
        y.backward(dy)
    ab(f"site {site} C={shp[1]} n={n} fwd+bwd{'' if routed else ' (not routed)'}", {False: lambda: run(False), True: lambda: run(True)}, n=5)
    del x, dy
for net, _ in nets.values():
    net.zero_grad(set_to_none=True)

steps = {k: sdc.GraphedLossStep(gd, state, weight=w, t=t, noise=noise) for k, (_, gd) in nets.items()}
ab("GraphedLossStep replay", {k: (lambda s=s: s()) for k, s in steps.items()})
