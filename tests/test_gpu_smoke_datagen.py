"""sdc_smoke_datagen through safediffcon_amd.smoke_datagen (the smoke task's data generator with its closed loop inside the
kernel, csrc/sdc_smoke.hip) against
 * records of the REAL reference generator (2d/dataset/apps/a_gen_dataset_128.py + vendored PhiFlow;
   tools/make_smoke_datagen_fixture.py): 16- and 32-step passes, the two full 256-step passes as one batch of two, and main()'s
   pass 1 / decision / pass 2 on a continuing stream -- the noise regenerated from the fixture's seed in the reference's order;
 * the numpy restatement of the loop (tests/smoke_datagen_loop.py, itself held to those records by
   tests/test_host_smoke_datagen.py) on fresh inputs.
Gates: velocity, control, both float64 densities and the smoke rows within 1e-9 of their scale (the velocity gate of
tests/test_gpu_smoke_solver.py); acceptance flags equal.  What differs from the reference is the association of the CG's dot
products and of the bucket sums; regrouping the dot products on the CPU moved these outputs by 2.7e-13 of scale at most.
Measured on MI355X (max over the cases of a group, as a fraction of the array's scale):
  short passes (16 / 32 steps)   velocity 2.0e-14   control 2.5e-15   density 1.6e-13   set-zero density 1.6e-13   smoke 9.0e-15
  full passes (256 steps)        velocity 8.1e-16   control 1.3e-15   density 5.3e-15   set-zero density 5.3e-15   smoke 7.1e-16
  main()'s two passes            velocity 1.8e-15   control 1.7e-15   density 3.2e-14   set-zero density 1.6e-14   smoke 4.3e-15
  fresh inputs vs restatement    velocity 1.0e-14   control 4.1e-15   density 1.9e-14   set-zero density 1.4e-14   smoke 5.9e-16
The float32 frames of the full passes round to the reference's float32 values exactly."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import smoke_datagen_loop as sl

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
GATE = 1e-9                              # of the array's scale: velocity, control, densities, smoke rows
F32_ULP = 2.0 ** -23                     # a float64 value within GATE of the reference rounds to float32 within one more ulp
DEV = "cuda:0"
FIELDS = ("velocity", "control", "density", "density_zero")


def _fix(name):
    return np.load(os.path.join(G, f"smoke_datagen_{name}.npz"))


@functools.lru_cache(maxsize=None)
def _gen(T, time_length, space_length):
    from safediffcon_amd import smoke_datagen as sd
    return sd.SmokeDataGenerator(device=DEV, original_timelength=T, time_length=time_length, space_length=space_length)


def _gen_of(z):
    return _gen(int(z["T"]), int(z["time_length"]), int(z["space_length"]))


def _err(got, want, what, gate=GATE, extra=0.0):
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max())
    print(f"{what}: max|err| {err:.3e} on scale {scale:.3e} = {err / scale:.2e} of scale")
    assert err <= (gate + extra) * scale, f"{what}: max|err| {err:.3e} on scale {scale:.3e}"
    return err / scale


def _check_fields(out, b, z, name, prefix=""):
    frames = list(z[prefix + "frames64"])
    for k in FIELDS:
        if prefix + k not in z.files:
            continue
        want = z[prefix + k]
        want = want[..., 0] if k.startswith("density") else want
        got = out[k][b].cpu().numpy()
        assert got.dtype == np.float64 and got[frames].shape == want.shape, (name, k)
        _err(got[frames], want, f"{name} {prefix}{k}")
    if "frames32" in z.files and not prefix:
        frames = list(z["frames32"])
        for k in FIELDS:
            want = z[k + "_f32"]
            want = want[..., 0] if k.startswith("density") else want
            got = out[k][b].cpu().numpy()[frames]
            _err(got.astype(np.float32).astype(np.float64), want.astype(np.float64), f"{name} {k} (float32 frames)", extra=F32_ULP)


# ------------------------------------------------------------------------------------------------ the reference's records
@pytest.mark.parametrize("name", ["short_rs4_a", "short_rs4_b", "short_rs1"])
def test_short_passes_vs_reference_fixtures(name):
    """rs = 4 with turn frames off the recording grid (no book-keeping there), rs = 1 / ss = 1 with record-then-book turn
    frames and the 127-in-128 density frame; the safe masks' eight areas"""
    z = _fix(name)
    gen = _gen_of(z)
    scenes, states = gen.scenes([int(z["seed"])], return_states=True)
    assert all(np.array_equal(scenes[k][0], z[k]) for k in ("xs", "ys", "vxs", "vys", "intervals"))
    out = gen.rollout(scenes, str(z["masks"]), noise=states)
    n, L = int(z["time_length"]) + 1, int(z["space_length"])
    assert out["velocity"].shape == (1, n, L, L, 2) and out["density"].shape == (1, n, L, L) and out["smoke"].shape == (1, n, 9)
    _check_fields(out, 0, z, name)
    _err(out["smoke"][0].cpu().numpy(), z["smoke"], f"{name} smoke")
    assert out["accepted"].tolist() == [True]                                # a pass with the safe masks always is
    assert (out["control"][0, -1] == 0).all()                                # the never-recorded last control frame
    if L == 128:
        assert (out["density"][0, :, 127] == 0).all() and (out["density"][0, :, :, 127] == 0).all()


def test_the_two_full_length_passes_as_one_batch():
    """the production shape, 256 steps x 500 CG iterations, two scenes with different schedules in one launch; one accepted,
    one rejected, with the filter and without"""
    from safediffcon_amd import smoke_datagen as sd
    za, zr = _fix("full_acc"), _fix("full_rej")
    gen = _gen_of(za)
    scenes, states = gen.scenes([int(za["seed"]), int(zr["seed"])], return_states=True)
    assert not np.array_equal(scenes["schedule"][0], scenes["schedule"][1])
    out = gen.rollout(scenes, "normal", noise=states)
    for b, (name, z) in enumerate((("full_acc", za), ("full_rej", zr))):
        assert all(np.array_equal(scenes[k][b], z[k]) for k in ("xs", "ys", "vxs", "vys", "intervals"))
        _check_fields(out, b, z, name)
        row = out["smoke"][b].cpu().numpy()
        _err(row, z["smoke"], f"{name} smoke")
        assert bool(out["accepted"][b]) == bool(z["accepted"]) and sd.accept(row[-1], True) == bool(z["accepted_filter"])
    assert out["accepted"].tolist() == [True, False]


def test_generate_reproduces_mains_two_passes():
    """seeds (18, 0): pass 1 of both, seed 18 accepted and run again with the safe masks on its continuing stream, seed 0
    rejected and left without pass-2 arrays"""
    za, zr = _fix("pair_acc"), _fix("pair_rej")
    gen = _gen_of(za)
    res = gen.generate([int(za["seed"]), int(zr["seed"])], noise="reference")
    assert res["accepted"].tolist() == [True, False] == [bool(za["accepted"]), bool(zr["accepted"])]
    assert res["records"][1] is None
    _err(res["smoke"][0], za["smoke"], "pair_acc pass 1 smoke")
    _err(res["smoke"][1], zr["smoke"], "pair_rej pass 1 smoke")
    rec = res["records"][0]
    assert rec["seed"] == 18 and np.array_equal(rec["smoke"], res["smoke"][0]) and rec["domain"].shape == (1, 127, 127, 1)
    frames = list(za["frames64"])
    for k in ("velocity", "control", "density"):
        want = za[k][..., 0] if k == "density" else za[k]
        _err(rec[k][frames], want, f"pair_acc pass 2 {k}")
    _err(rec["smoke_safe"], za["smoke_safe"], "pair_acc pass 2 smoke_safe")
    # pass 1's own fields (main keeps only its smoke record): one more rollout on fresh states
    scenes, states = gen.scenes([18, 0], return_states=True)
    p1 = gen.rollout(scenes, "normal", noise=states)
    _check_fields(p1, 0, za, "pair_acc", "pass1_")
    _check_fields(p1, 1, zr, "pair_rej", "pass1_")


# ------------------------------------------------------------------------------------------------ batch independence
def test_a_scene_alone_and_as_sample_2_of_3_gives_equal_outputs():
    from safediffcon_amd import smoke_datagen as sd
    gen = _gen(32, 8, 64)
    scenes, states = gen.scenes([13, 3, 18], return_states=True)
    ring = torch.stack([torch.from_numpy(sd.reference_noise(states[b], scenes["vxs"][b], scenes["vys"][b], scenes["intervals"][b], 32))
                        for b in range(3)]).to(DEV)
    three = gen.rollout(scenes, ["normal", "safe", "normal"], noise=ring)
    alone = gen.rollout({k: v[1:2] for k, v in scenes.items()}, "safe", noise=ring[1:2])
    for k in FIELDS + ("smoke",):
        assert torch.equal(three[k][1], alone[k][0]), k
    assert (three["smoke"][0, :, 8] == 0).all() and (three["smoke"][2, :, 8] == 0).all()     # a normal row's ninth column
    assert not torch.equal(three["velocity"][0], three["velocity"][1])


# ------------------------------------------------------------------------------------------------ device noise
def test_device_noise_is_reproducible_and_has_the_references_distributions():
    gen = _gen(32, 8, 64)
    scenes = gen.scenes([13, 3])
    outs = []
    for _ in range(2):
        g = torch.Generator(device=DEV)
        g.manual_seed(5)
        outs.append(gen.rollout(scenes, "safe", noise=g))
    for k in FIELDS + ("smoke",):
        assert torch.equal(outs[0][k], outs[1][k]), k
    ctrl = outs[0]["control"]
    assert (ctrl[:, :, 8:56, 8:56] == 0).all()                              # interior cells of every control frame
    ring_mask = torch.ones(64, 64, dtype=torch.bool, device=DEV)
    ring_mask[8:56, 8:56] = False
    cells = int(ring_mask.sum())
    for b in range(2):
        for c, v in ((0, scenes["vxs"][b, 0]), (1, scenes["vys"][b, 0])):
            mean = float(ctrl[b, 0, :, :, c][ring_mask].mean())
            print(f"scene {b} component {c}: mean {mean:.5f} vs {v:.5f}, bound {5 * abs(v) / 10 / np.sqrt(cells):.5f} ({cells} cells)")
            assert abs(mean - v) <= 5 * abs(v) / 10 / np.sqrt(cells)
    # generate's device mode, both passes
    a = gen.generate([18, 0], noise="device", generator=torch.Generator(device=DEV).manual_seed(9))
    b = gen.generate([18, 0], noise="device", generator=torch.Generator(device=DEV).manual_seed(9))
    assert np.array_equal(a["smoke"], b["smoke"]) and a["accepted"].tolist() == b["accepted"].tolist()
    for ra, rb in zip(a["records"], b["records"]):
        assert (ra is None) == (rb is None) and (ra is None or all(np.array_equal(ra[k], rb[k]) for k in ("velocity", "control", "density", "smoke_safe")))


# ------------------------------------------------------------------------------------------------ fresh inputs
def test_fresh_inputs_vs_the_restated_loop():
    """T = 8 recorded every frame at ss = 2, two samples in one launch -- the normal masks with the smoke starting inside a
    side area, the safe masks with it starting inside the hazard area -- on ring fields that are no draw of the reference's"""
    from safediffcon_amd import smoke_datagen as sd
    gen = _gen(8, 8, 64)
    rng = np.random.default_rng(21)
    ring = rng.standard_normal((2, 8, 128, 128, 2)) * np.array([0.3, 2.0])[:, None, None, None, None]
    intervals = np.array([[3, 2, 2], [2, 3, 2]])
    scenes = {"xs": np.array([[10, 0, 0, 0, 0], [50, 0, 0, 0, 0]]), "ys": np.array([[24, 0, 0, 0, 0], [42, 0, 0, 0, 0]]),
              "vxs": np.zeros((2, 4)), "vys": np.zeros((2, 4)), "intervals": intervals,
              "schedule": np.stack([sd.schedule_bytes(iv, 8, 1) for iv in intervals])}
    kinds = ["normal", "safe"]
    out = gen.rollout(scenes, kinds, noise=torch.from_numpy(ring).to(DEV))
    for b in range(2):
        want = sl.loop(ring[b], int(scenes["ys"][b, 0]), int(scenes["xs"][b, 0]), intervals[b], 8, 1, 2, kinds[b])
        for k in FIELDS:
            _err(out[k][b].cpu().numpy(), want[k], f"fresh sample {b} {k}")
        nb = want["smoke"].shape[1] - 1
        assert want["smoke"][-1, :nb].sum() > 1                              # the book-keeping took smoke
        _err(out["smoke"][b, :, :nb + 1].cpu().numpy(), want["smoke"], f"fresh sample {b} smoke")
        assert (out["smoke"][b, :, nb + 1:] == 0).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_c_abi_refusals_return_their_codes_and_leave_the_outputs_untouched():
    from safediffcon_amd import _lib
    lib = _lib.get_lib()
    gen = _gen(8, 8, 64)
    B, T, n, L = 1, 8, 9, 64
    ring = torch.zeros(B, T, 128, 128, 2, dtype=torch.float64, device=DEV)
    start = torch.tensor([[24, 40]], dtype=torch.int32, device=DEV)
    sched = torch.full((B, T), 2, dtype=torch.uint8, device=DEV)
    mi = torch.zeros(B, dtype=torch.int32, device=DEV)
    maps, nbs = gen._label_maps()
    fluid = gen.sim.fluid_mask_device(torch.device(DEV))
    outs = [torch.full(s, -7.0, dtype=torch.float64, device=DEV) for s in ((B, n, L, L), (B, n, L, L), (B, n, L, L, 2), (B, n, L, L, 2), (B, n, 9))]
    wbytes = lib.sdc_smoke_datagen_workspace_bytes(B)
    work = torch.zeros(wbytes + 16, dtype=torch.uint8, device=DEV)
    nb_arr = (C.c_int32 * 2)(*nbs)

    def call(ring_p=ring.data_ptr(), T_=T, rs=1, ss=2, nbv=nb_arr, wb=wbytes, wp=work.data_ptr(), cols=9, dens=outs[0].data_ptr()):
        return lib.sdc_smoke_datagen(ring_p, ring.stride(0), ring.stride(1), start.data_ptr(), sched.data_ptr(), mi.data_ptr(),
                                     maps.data_ptr(), nbv, 2, fluid.data_ptr(), 0.2, dens, outs[1].data_ptr(), outs[2].data_ptr(),
                                     outs[3].data_ptr(), outs[4].data_ptr(), cols, wp, wb, B, T_, rs, ss, 1e-8, 500,
                                     torch.cuda.current_stream().cuda_stream)

    assert call(ring_p=None) == -4 and call(dens=None) == -4                 # SDC_ENULL
    assert call(rs=3) == -1 and "multiple of rs" in _lib.last_error()        # SDC_EINVAL
    assert call(ss=3) == -1 and "divide 128" in _lib.last_error()
    assert call(nbv=(C.c_int32 * 2)(7, 9)) == -1 and call(nbv=(C.c_int32 * 2)(1, 8)) == -1
    assert call(wb=wbytes - 1) == -1 and "workspace" in _lib.last_error()
    assert call(cols=8) == -1
    assert call(wp=work.data_ptr() + 8) == -2 and call(ring_p=ring.data_ptr() + 8) == -2      # SDC_EALIGN
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs)
    assert call() == 0                                                       # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert not any(bool((o == -7.0).any()) for o in outs)                    # every element of every output is written
