#!/usr/bin/env python3
"""Generate tests/golden/smoke_unet_f64.npz by running the REAL reference U-Net (2d/video_diffusion_pytorch:
Unet3D_with_Conv3D) at 64 frames on the CPU: forward, one weighted l2 loss and the gradient of every parameter.  The
fixture is data only: seeds, the time step, eps, the loss, the gradients and the parameter spec as gen_smoke stores it.
Every parameter's gradient is stored as its L2 norm and one fixed projection (on det_tensor(shape, DOT_SEED + i), as gen_grad
does); the tensors themselves for every parameter of at most FULL_MAX elements and for the stem -- all 490 727 gradient
elements in fp32 are 1.9 MB, which no committed file may have.

    python tools/make_smoke_frames_fixture.py [--reference <checkout>]          # under a second of compute

The reference is imported the way oracle/make_goldens.py:gen_smoke does it (its shims directory and the checkout's `2d`
on sys.path); that module's helpers are imported, nothing under oracle/ changes.  Never run on a GPU machine.

Net    Unet3D_with_Conv3D(dim=8, dim_mults=(1, 2, 4), channels=7), weights load_det(net, 300)
Input  x = det_tensor((1, 64, 7, 8, 8), 301), t = [700]: 8 x 8 pixels give the three levels 64, 16 and 4 pixels per frame --
       full pixel groups, the minimum, and a single ragged group for the 64-frame attention kernels
Loss   (w * ((eps - target) ** 2).flatten(1).mean(1)).mean(), target = det_tensor(x.shape, 302), w = 1 + 0.5 det_tensor((1,), 303)
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.environ.get("SDC_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

WEIGHT_SEED, X_SEED, TARGET_SEED, W_SEED, DOT_SEED = 300, 301, 302, 303, 7300
FULL_MAX = 4096
FULL_ALSO = ("init_conv.weight",)
SHAPE = (1, 64, 7, 8, 8)        # (B, frames, channels, H, W), the reference's input order
T = 700


def main():
    from oracle import make_goldens as G
    from oracle.detweights import det_tensor
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SDC_REFERENCE") or G.REF, help="the reference checkout")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(G.__file__)), "_shims"))
    sys.path.insert(0, os.path.join(args.reference, "2d"))
    from video_diffusion_pytorch.video_diffusion_pytorch_conv3d import Unet3D_with_Conv3D

    net = Unet3D_with_Conv3D(dim=8, dim_mults=(1, 2, 4), channels=7)
    spec = G.load_det(net, seed=WEIGHT_SEED)
    x, t = det_tensor(SHAPE, X_SEED), torch.tensor([T])
    target, w = det_tensor(SHAPE, TARGET_SEED), 1.0 + 0.5 * det_tensor((1,), W_SEED)
    t0 = time.time()
    eps = net(x, t)
    loss = (w * ((eps - target) ** 2).flatten(1).mean(1)).mean()
    loss.backward()
    dt = time.time() - t0
    named = list(net.named_parameters())
    grads = [(k, (p.grad if p.grad is not None else torch.zeros_like(p)).detach()) for k, p in named]
    norms = [float(g.double().norm()) for _, g in grads]
    dots = [float((g.double() * det_tensor(tuple(g.shape), DOT_SEED + i).double()).sum()) for i, (_, g) in enumerate(grads)]
    full = {"grad:" + k: g.numpy() for k, g in grads if g.numel() <= FULL_MAX or k in FULL_ALSO}
    arrs = dict(dim=np.int64(8), frames=np.int64(SHAPE[1]), image_size=np.int64(SHAPE[-1]), t=t.numpy(), weight_seed=np.int64(WEIGHT_SEED),
                x_seed=np.int64(X_SEED), target_seed=np.int64(TARGET_SEED), w=w.numpy(), eps=eps.detach().numpy(),
                loss=np.float64(loss.item()), dot_seed=np.int64(DOT_SEED), grad_keys=np.array([k for k, _ in grads]),
                grad_norms=np.array(norms), grad_dots=np.array(dots), **G.spec_arrays(spec), **full)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "smoke_unet_f64.npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB); forward + backward {dt:.2f} s; loss {loss.item():.9g}; "
          f"{len(grads)} gradients ({len(full)} stored whole), largest norm {max(norms):.3e}")


if __name__ == "__main__":
    main()
