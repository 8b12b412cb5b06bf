#!/usr/bin/env python3
"""A/B of net.train_fuse_linattn on the C4-width smoke net (dim 64, 32 frames of 64 x 64):
python tools/linattn_train_ab.py [batch] [reps] [train_fuse_attn: 0 | 1]

Switch off and on interleaved, `reps` repetitions each, min - max printed (train_fuse_attn as the third argument says, in both arms):
  * the fine-tuning step of bench_extras.finetune_step (loss = mean(w_b p_losses_b); loss.backward()), eager and as
    sdc.GraphedLossStep replay (two nets with the same weights, one per setting: a captured step keeps its mode)
  * forward + backward of Trainer.spatial_linear alone at every covered site (the sites _la_fusable admits, found by one forward)
  * peak allocated memory of the eager step
The switch-off arm is the parent's chain, bit for bit.  The log kept in profiles/linattn_train_ab.log is this script's output."""
import _libsel  # noqa: F401,E402  (SDC_LIB_PATH -> safediffcon_amd._lib.use_library, tools only)
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import safediffcon_amd as sdc  # noqa: E402
from oracle.detweights import det_params, det_tensor  # noqa: E402
from safediffcon_amd import autograd  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
TATTN = bool(int(sys.argv[3])) if len(sys.argv) > 3 else False
dev = torch.device("cuda:0")
shape = (32, 7, 64, 64)


def make(fuse):
    net = sdc.Unet3D_with_Conv3D(dim=64, dim_mults=(1, 2, 4), channels=7)
    net.load_state_dict(det_params([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 77))
    net.to(dev).train()
    net.train_fuse_linattn = fuse
    net.train_fuse_attn = TATTN
    return net, sdc.GaussianDiffusionSmoke(net, image_size=64, frames=32, timesteps=1000, loss_type="l2").to(dev)


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
        print(f"{label:34s} train_fuse_linattn={k!s:5s} ms/iter min {min(v):8.3f} max {max(v):8.3f}   ({REPS} repetitions of {n})")
    sys.stdout.flush()


print(f"# C4-width smoke net, dim 64, 32 frames of 64x64, B = {B}, train_fuse_attn = {TATTN}; {torch.cuda.get_device_name(0)}")
sites = []
orig = autograd.Trainer.spatial_linear
autograd.Trainer.spatial_linear = lambda self, p, x: (sites.append((p, tuple(x.shape))), orig(self, p, x))[1]
l_off = eager_step(False).item()
autograd.Trainer.spatial_linear = orig
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
for site, shp in sites:
    if not nets[True][0]._la_fusable(shp):
        print(f"site {site} {shp}: not covered, the chain in both arms")
        continue
    x, dy = det_tensor(shp, 20).to(dev), det_tensor(shp, 21).to(dev)

    def run(fuse, site=site, x=x, dy=dy):
        net, _ = nets[fuse]
        T = net._trainer()
        xg = x.detach().requires_grad_()
        with T.step(dev):
            y = T.spatial_linear(site, xg)
        y.backward(dy)
    ab(f"site {site} C={shp[1]} {shp[3]}x{shp[4]} fwd+bwd", {False: lambda: run(False), True: lambda: run(True)}, n=5)
    del x, dy
for net, _ in nets.values():
    net.zero_grad(set_to_none=True)

steps = {k: sdc.GraphedLossStep(gd, state, weight=w, t=t, noise=noise) for k, (_, gd) in nets.items()}
ab("GraphedLossStep replay", {k: (lambda s=s: s()) for k, s in steps.items()})
