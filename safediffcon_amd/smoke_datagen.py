"""Smoke data generator: what 2d/dataset/apps/a_gen_dataset_128.py (run through data_128.sh / data_128_filter.sh) does to make
the 2-D smoke task's training trajectories, with the 256 fluid steps of a pass inside one launch of `sdc_smoke_datagen`
(csrc/sdc_smoke.hip) -- one workgroup per trajectory, any number of trajectories per launch.

  closest_multiple / exp2_target_128 / get_per_vel / get_real_vel    a_gen_dataset_128.py:37-47,110-210   -> random_scenes
  get_initial_state / get_envolve / write_vel_density / loop_write   a_gen_dataset_128.py:246-341,442-741 -> the kernel + the schedule bytes
  main                                                               a_gen_dataset_128.py:744-888         -> SmokeDataGenerator.generate

The generator's loop is closed: on every frame the velocity outside [16:112, 16:112] is the previous frame's projected velocity
plus fresh Gaussian noise (an absolute draw around a target velocity on the four turn frames), so the kernel carries the
velocity from step to step and only the noise fields come from outside.  The kernel does not care where those came from:
`noise="reference"` continues each seed's `np.random.RandomState` in the reference's draw order on the host and uploads the
fields (the reference's own numbers, 67 MB per full-length pass), `noise="device"` draws them with `torch.randn` on the device
(same distributions, no stream parity).  The reference's pid / clock seeding and its process pool are not reproduced: a
trajectory is named by its seed.  No CPU fallback.
"""
import os

import numpy as np
import torch

from . import _lib, smoke_solver
from ._lib import check

S = 128
RING_LO, RING_HI = 16, 112              # controls act outside [16:112, 16:112] (a_gen_dataset_128.py:267-270)
SCHED_ABSOLUTE = 1                      # bit 0: the ring field is the value, not an increment
SCHED_BOOK_THEN_RECORD = 1 << 1         # bits 1-2: 0 = no book-keeping on this frame
SCHED_RECORD_THEN_BOOK = 2 << 1


def closest_multiple(num, scale):
    """the multiple of `scale` nearest to num, the upper one on a tie"""
    lower = (num // scale) * scale
    upper = lower + scale
    return lower if abs(num - lower) < abs(num - upper) else upper


def _turn_points(rs):
    """five turn points of the smoke's intended path, drawn in the reference's order: start (even coordinates), two targets on
    the start's side of the middle bar, one near the gap, the end above the target bucket"""
    m = 4
    x0 = closest_multiple(rs.randint(16 + 2 + m, 112 - 10 - m), 2)
    y0 = closest_multiple(rs.randint(16 + 2 + m, 40 - 10 - m), 2)
    left = x0 < 64 - 8
    x1 = rs.randint(16 + m, 64 - 8) if left else rs.randint(64, 112 - 8 - m)
    x2 = rs.randint(16 + m, 64 - 8) if left else rs.randint(64, 112 - 8 - m)
    x3 = rs.randint(50, 80 - 1 - 8)
    x4 = rs.randint(64 - 8, 64 + 8 - 8)
    return [int(x0), int(x1), int(x2), int(x3), int(x4)], [int(y0), 40, 50, 64, 112]


def _leg_velocities(rs, xs, ys, T, record_scale, y_scale, min_scale, max_scale):
    """one uniform scale, then the four x velocities, then the four y velocities, each normal(v, |v| / 4); the first three legs'
    frame counts rounded to the recording grid"""
    d = [((xs[k + 1] - xs[k]) ** 2 + (ys[k + 1] - ys[k]) ** 2) ** 0.5 for k in range(4)]
    dist = d[0] + d[1] + d[2] + d[3]
    v = dist / float(T)
    vx = [v * (xs[k + 1] - xs[k]) / d[k] for k in range(4)]
    vy = [v * (ys[k + 1] - ys[k]) / d[k] for k in range(4)]
    scale = rs.uniform(min_scale, max_scale)

    def real(vel):
        return rs.normal(vel, abs(vel / 4))
    vxs = [real(scale * a) for a in vx]
    vys = [real(y_scale * a) for a in vy]
    iv = [closest_multiple(int(T * d[k] / dist), record_scale) for k in range(3)]
    return vxs, vys, [iv[0] + 1, iv[1], iv[2]]


def turn_frames(intervals):
    """frames (1-based) whose ring is an absolute draw: 1, iv0, iv0 + iv1, iv0 + iv1 + iv2"""
    iv = [int(v) for v in intervals]
    return [1, iv[0], iv[0] + iv[1], iv[0] + iv[1] + iv[2]]


def schedule_bytes(intervals, T, record_scale):
    """(T,) uint8, entry f - 1 for frame f = 1 .. T.  Ordinary frames and frame 1 book, then record; the three later turn
    frames record first and book after when they fall on the recording grid, and skip the book-keeping altogether when they
    do not (loop_write, a_gen_dataset_128.py:600-694)."""
    tf = turn_frames(intervals)
    if not (tf[0] < tf[1] < tf[2] < tf[3] <= T):
        raise ValueError(f"turn frames {tf} are not increasing within 1 .. {T}: the reference's loop would repeat or skip a frame")
    out = np.full(T, SCHED_BOOK_THEN_RECORD, np.uint8)
    out[0] |= SCHED_ABSOLUTE
    for f in tf[1:]:
        out[f - 1] = SCHED_ABSOLUTE | (SCHED_RECORD_THEN_BOOK if f % record_scale == 0 else 0)
    return out


def _draw_scene(rs, T, time_length, y_scale, min_scale, max_scale):
    record_scale = T // time_length
    xs, ys = _turn_points(rs)
    vxs, vys, iv = _leg_velocities(rs, xs, ys, T, record_scale, y_scale, min_scale, max_scale)
    return xs, ys, vxs, vys, iv, schedule_bytes(iv, T, record_scale)


def _stack(rows):
    return {"xs": np.array([r[0] for r in rows], np.int64), "ys": np.array([r[1] for r in rows], np.int64),
            "vxs": np.array([r[2] for r in rows], np.float64), "vys": np.array([r[3] for r in rows], np.float64),
            "intervals": np.array([r[4] for r in rows], np.int64), "schedule": np.stack([r[5] for r in rows])}


def random_scenes(seeds, original_timelength=256, time_length=32, y_scale=5, min_scale=2, max_scale=5, return_states=False):
    """One scene per seed from `np.random.RandomState(seed)` in the reference's draw order (`np.random.seed(seed)`, then
    exp2_target_128, then get_per_vel) -> {"xs", "ys" (B, 5) int64, "vxs", "vys" (B, 4) float64, "intervals" (B, 3) int64,
    "schedule" (B, T) uint8}.  The global numpy stream is not touched.  return_states: also the RandomStates, positioned where
    the reference's first noise draw comes next."""
    if original_timelength % time_length:
        raise ValueError(f"time_length = {time_length} does not divide original_timelength = {original_timelength}")
    states = [np.random.RandomState(int(s)) for s in seeds]
    scenes = _stack([_draw_scene(rs, original_timelength, time_length, y_scale, min_scale, max_scale) for rs in states])
    return (scenes, states) if return_states else scenes


def reference_noise(rs, vxs, vys, intervals, T, out=None):
    """the ring fields of one pass, (T, 128, 128, 2) float64, drawn from `rs` in get_envolve's order: on a turn frame the whole
    x field normal(vx, |vx| / 10), then the whole y field; on every other frame one interleaved normal(0, 0.1) draw"""
    out = np.empty((T, S, S, 2)) if out is None else out
    tf = turn_frames(intervals)
    for f in range(1, T + 1):
        if f in tf:
            q = tf.index(f)
            out[f - 1, :, :, 0] = rs.normal(vxs[q], abs(vxs[q] / 10), (1, S, S))[0]
            out[f - 1, :, :, 1] = rs.normal(vys[q], abs(vys[q] / 10), (1, S, S))[0]
        else:
            out[f - 1] = rs.normal(0, 0.1, (1, S, S, 2))[0]
    return out


def accept(last_row, filter=False, min_sum_rate=0.85, max_sum_rate=1.15):
    """loop_write's decision from a pass's last smoke row (a_gen_dataset_128.py:730-741): the density total inside
    (100 min_sum_rate, 100 max_sum_rate) and, with `filter`, more than 0.8 of it in the target bucket (area 1).  A row of the
    eight safe areas is always accepted."""
    row = np.asarray(last_row, np.float64)
    if len(row) - 1 != 7:
        return True
    total = np.sum(row[:-1]) + row[-1]
    with np.errstate(all="ignore"):
        target = (not filter) or bool(row[1] / total > 0.8)
    return bool(target and 10 * 10 * min_sum_rate < total < 10 * 10 * max_sum_rate)


def save_record(directory, record, index):
    """<directory>/sim_%06d/{Density,Velocity,Control,Smoke,Smoke_safe,domain}.npy + smoke_out.csv + smoke_out_safe.csv in the
    reference's layouts: fields (L, L, C, n) float64, smoke records (n, nb + 1).  -> the trajectory's directory"""
    path = os.path.join(directory, "sim_%06d" % index)
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "Density.npy"), np.ascontiguousarray(np.moveaxis(np.asarray(record["density"], np.float64)[..., None], 0, -1)))
    for name, key in (("Velocity", "velocity"), ("Control", "control")):
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(np.moveaxis(np.asarray(record[key], np.float64), 0, -1)))
    for name, key, csv in (("Smoke", "smoke", "smoke_out.csv"), ("Smoke_safe", "smoke_safe", "smoke_out_safe.csv")):
        rows = np.asarray(record[key], np.float64)
        np.save(os.path.join(path, name + ".npy"), rows)
        np.savetxt(os.path.join(path, csv), rows, delimiter=",")
    np.save(os.path.join(path, "domain.npy"), np.asarray(record["domain"]))
    return path


class SmokeDataGenerator:
    """`generate(seeds)` = main() of a_gen_dataset_128.py for one trajectory per seed; `rollout` = one loop_write pass.
    The defaults are the parameters data_128.sh ships; data_128_filter.sh adds filter=True."""

    def __init__(self, device="cuda", original_timelength=256, time_length=32, original_space_length=128, space_length=64,
                 min_scale=2, max_scale=5, y_scale=5, initial_vy=0.2, min_sum_rate=0.85, max_sum_rate=1.15, filter=False, sim=None,
                 dt=1, accuracy=1e-8, max_iterations=500):
        if dt != 1:
            raise NotImplementedError("the reference generates with dt = 1 only (a_gen_dataset_128.py:787)")
        if original_space_length != S:
            raise ValueError("the rollout kernel is built for the reference's 128-sample staggered grid")
        if original_timelength % time_length:
            raise ValueError(f"time_length = {time_length} does not divide original_timelength = {original_timelength}")
        if S % space_length:
            raise ValueError(f"space_length = {space_length} does not divide {S}")
        if torch.device(device).type != "cuda":
            raise RuntimeError("safediffcon_amd.smoke_datagen runs on MI355X only (no CPU fallback)")
        self.device = torch.device(device)
        self.T, self.time_length, self.space_length = int(original_timelength), int(time_length), int(space_length)
        self.rs, self.ss = self.T // self.time_length, S // self.space_length
        self.min_scale, self.max_scale, self.y_scale, self.initial_vy = min_scale, max_scale, y_scale, float(initial_vy)
        self.min_sum_rate, self.max_sum_rate, self.filter = min_sum_rate, max_sum_rate, bool(filter)
        self.accuracy, self.max_iterations = float(accuracy), int(max_iterations)
        self.sim = sim or smoke_solver.init_sim_128()
        self._maps = None

    # ------------------------------------------------------------------------------------------------ scenes and noise
    def scenes(self, seeds, return_states=False):
        return random_scenes(seeds, self.T, self.time_length, self.y_scale, self.min_scale, self.max_scale, return_states)

    def _label_maps(self):
        if self._maps is None:
            n, s = smoke_solver.get_bucket_mask()[0], smoke_solver.get_bucket_mask_safe()[0]
            maps = np.stack([smoke_solver._labels(n), smoke_solver._labels(s)])
            self._maps = (torch.from_numpy(maps).to(self.device), (len(n), len(s)))
        return self._maps

    def _device_noise(self, scenes, lo, hi, generator):
        """float64 randn on the device, scaled like the reference's draws: N(v, |v| / 10) per component on the turn frames,
        N(0, 0.1) elsewhere"""
        B = hi - lo
        loc = np.zeros((B, self.T, 1, 1, 2))
        scale = np.full((B, self.T, 1, 1, 2), 0.1)
        for n in range(B):
            for q, f in enumerate(turn_frames(scenes["intervals"][lo + n])):
                loc[n, f - 1, 0, 0] = (scenes["vxs"][lo + n, q], scenes["vys"][lo + n, q])
                scale[n, f - 1, 0, 0] = np.abs(loc[n, f - 1, 0, 0] / 10)
        ring = torch.randn(B, self.T, S, S, 2, dtype=torch.float64, device=self.device, generator=generator)
        return ring.mul_(torch.from_numpy(scale).to(self.device)).add_(torch.from_numpy(loc).to(self.device))

    def _host_noise(self, scenes, lo, hi, states, timing):
        """each sample's RandomState continued in the reference's order; one 67 MB field per full-length sample goes up at a time"""
        import time
        ring = torch.empty(hi - lo, self.T, S, S, 2, dtype=torch.float64, device=self.device)
        buf = np.empty((self.T, S, S, 2))
        for n in range(lo, hi):
            t0 = time.perf_counter()
            reference_noise(states[n], scenes["vxs"][n], scenes["vys"][n], scenes["intervals"][n], self.T, out=buf)
            t1 = time.perf_counter()
            ring[n - lo].copy_(torch.from_numpy(buf))
            if timing is not None:
                torch.cuda.synchronize(self.device)
                timing["host_draw_s"] = timing.get("host_draw_s", 0.0) + (t1 - t0)
                timing["upload_s"] = timing.get("upload_s", 0.0) + (time.perf_counter() - t1)
        return ring

    # ------------------------------------------------------------------------------------------------ one pass
    def _launch(self, scenes, lo, hi, map_index, ring):
        dev, B = self.device, hi - lo
        if not (torch.is_tensor(ring) and ring.is_cuda):
            raise RuntimeError("safediffcon_amd.smoke_datagen runs on MI355X only (no CPU fallback)")
        if ring.dtype != torch.float64 or tuple(ring.shape) != (B, self.T, S, S, 2):
            raise ValueError(f"ring fields: float64 {(B, self.T, S, S, 2)} expected, got {ring.dtype} {tuple(ring.shape)}")
        if ring.stride()[2:] != (S * 2, 2, 1):
            ring = ring.contiguous()
        sched = np.ascontiguousarray(scenes["schedule"][lo:hi], np.uint8)
        if sched.shape != (B, self.T):
            raise ValueError(f"schedule {sched.shape} vs {(B, self.T)}")
        start = np.stack([scenes["ys"][lo:hi, 0], scenes["xs"][lo:hi, 0]], axis=1).astype(np.int32)
        maps, nbs = self._label_maps()
        n, L, cols = self.time_length + 1, self.space_length, max(nbs) + 1
        out = {"density": torch.empty(B, n, L, L, dtype=torch.float64, device=dev),
               "density_zero": torch.empty(B, n, L, L, dtype=torch.float64, device=dev),
               "velocity": torch.empty(B, n, L, L, 2, dtype=torch.float64, device=dev),
               "control": torch.empty(B, n, L, L, 2, dtype=torch.float64, device=dev),
               "smoke": torch.empty(B, n, cols, dtype=torch.float64, device=dev)}
        lib = _lib.get_lib()
        wbytes = lib.sdc_smoke_datagen_workspace_bytes(B)
        work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
        d_start, d_sched = torch.from_numpy(start).to(dev), torch.from_numpy(sched).to(dev)
        d_map = torch.from_numpy(np.ascontiguousarray(map_index, np.int32)).to(dev)
        fluid = self.sim.fluid_mask_device(dev)
        import ctypes as C
        nb_arr = (C.c_int32 * len(nbs))(*nbs)
        check(lib.sdc_smoke_datagen(ring.data_ptr(), ring.stride(0), ring.stride(1), d_start.data_ptr(), d_sched.data_ptr(),
                                    d_map.data_ptr(), maps.data_ptr(), nb_arr, len(nbs), fluid.data_ptr(), self.initial_vy,
                                    out["density"].data_ptr(), out["density_zero"].data_ptr(), out["velocity"].data_ptr(),
                                    out["control"].data_ptr(), out["smoke"].data_ptr(), cols, work.data_ptr(), wbytes, B, self.T,
                                    self.rs, self.ss, self.accuracy, self.max_iterations,
                                    torch.cuda.current_stream(dev).cuda_stream), "sdc_smoke_datagen")
        return out

    def rollout(self, scenes, masks="normal", noise=None, chunk=64, timing=None):
        """One loop_write pass over every scene.  masks: "normal" (seven areas) / "safe" (eight), or one of the two per scene.
        noise: a float64 CUDA tensor (B, T, 128, 128, 2) of ring fields used as they are; a list of B `np.random.RandomState`
        continued in the reference's draw order on the host; or a CUDA `torch.Generator` for device draws.
        -> {"density", "density_zero" (B, n, L, L), "velocity", "control" (B, n, L, L, 2), "smoke" (B, n, nb + 1)} float64 device
        tensors (with mixed masks "smoke" has nine columns, a normal row's last one zero) and "accepted" (B,) numpy bool."""
        B = len(scenes["xs"])
        kinds = [masks] * B if isinstance(masks, str) else list(masks)
        if len(kinds) != B or any(k not in ("normal", "safe") for k in kinds):
            raise ValueError('masks: "normal" or "safe", or one of them per scene')
        map_index = np.array([0 if k == "normal" else 1 for k in kinds], np.int32)
        if torch.is_tensor(noise):
            if not noise.is_cuda:
                raise RuntimeError("safediffcon_amd.smoke_datagen runs on MI355X only (no CPU fallback)")
            chunk = B
        elif not isinstance(noise, torch.Generator) and not (isinstance(noise, (list, tuple)) and len(noise) == B):
            raise TypeError("noise: a CUDA tensor of ring fields, a list of RandomStates (one per scene) or a torch.Generator")
        parts = []
        for lo in range(0, B, chunk):
            hi = min(B, lo + chunk)
            if torch.is_tensor(noise):
                ring = noise
            elif isinstance(noise, torch.Generator):
                ring = self._device_noise(scenes, lo, hi, noise)
            else:
                ring = self._host_noise(scenes, lo, hi, noise, timing)
            parts.append(self._launch(scenes, lo, hi, map_index[lo:hi], ring))
            del ring
        out = {k: torch.cat([p[k] for p in parts]) if len(parts) > 1 else parts[0][k] for k in parts[0]}
        nbs = self._label_maps()[1]
        if len(set(kinds)) == 1:
            out["smoke"] = out["smoke"][:, :, :nbs[map_index[0]] + 1]
        last = out["smoke"][:, -1].cpu().numpy()
        out["accepted"] = np.array([accept(last[n, :nbs[map_index[n]] + 1], self.filter, self.min_sum_rate, self.max_sum_rate)
                                    for n in range(B)], bool)
        return out

    # ------------------------------------------------------------------------------------------------ both passes
    def generate(self, seeds, noise="reference", chunk=64, generator=None, timing=None):
        """main() for one trajectory per seed: pass 1 with the normal masks decides acceptance from its last smoke row; the
        accepted ones restart from the same scene for pass 2 with the safe masks and fresh noise.
        -> {"accepted": (B,) bool, "smoke": (B, n, 8) pass 1's rows, "records": a list with, per seed, None (rejected: the
        caller carries on with further seeds) or {"density" (n, L, L), "velocity", "control" (n, L, L, 2), "smoke" (n, 8),
        "smoke_safe" (n, 9), "domain", "seed"} as numpy float64 -- what `save_record` writes.
        noise="reference": every seed's own stream, continued through pass 1's and then pass 2's draws as the reference does;
        noise="device": `torch.randn` from `generator` (a CUDA torch.Generator; default one seeded with the first seed)."""
        if noise not in ("reference", "device"):
            raise ValueError('noise: "reference" or "device"')
        seeds = [int(s) for s in seeds]
        scenes, states = self.scenes(seeds, return_states=True)
        if noise == "device":
            if generator is None:
                generator = torch.Generator(device=self.device)
                generator.manual_seed(seeds[0] if seeds else 0)
            src1 = src2 = generator
        p1 = self.rollout(scenes, "normal", states if noise == "reference" else src1, chunk, timing)
        ok = p1["accepted"]
        smoke1 = p1["smoke"].cpu().numpy()
        del p1
        records = [None] * len(seeds)
        idx = np.flatnonzero(ok)
        if len(idx):
            sub = {k: v[idx] for k, v in scenes.items()}
            p2 = self.rollout(sub, "safe", [states[i] for i in idx] if noise == "reference" else src2, chunk, timing)
            host = {k: p2[k].cpu().numpy() for k in ("density", "velocity", "control", "smoke")}
            for m, i in enumerate(idx):
                records[i] = {"density": host["density"][m], "velocity": host["velocity"][m], "control": host["control"][m],
                              "smoke": smoke1[i], "smoke_safe": host["smoke"][m], "domain": self.sim._active_mask.copy(),
                              "seed": seeds[i]}
        return {"accepted": ok, "smoke": smoke1, "records": records}

    save_record = staticmethod(save_record)
