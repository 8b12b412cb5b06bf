"""Test-side numpy restatement of the smoke data generator's loop (2d/dataset/apps/a_gen_dataset_128.py `loop_write` with
`get_envolve`, `get_initial_state`, `write_vel_density`), built from oracle.smoke_solver's primitives (`domain`, `evolve`,
`advect`, the bucket masks).  Independent of safediffcon_amd.smoke_datagen: it knows turn frames and the book-keeping order
from the reference's loop structure, not from the library's schedule bytes.  Used by tests/test_host_smoke_datagen.py against
the reference's recorded fixtures and by tests/test_gpu_smoke_datagen.py as the reference for fresh inputs.  Not a test module."""
import numpy as np

from oracle import smoke_solver as oss

S, N = oss.S, oss.N


def draw_noise(rs, vxs, vys, intervals, T):
    """(T, 128, 128, 2) ring fields from the RandomState `rs` in get_envolve's draw order"""
    tf = turn_frames(intervals)
    out = np.empty((T, S, S, 2))
    for f in range(1, T + 1):
        if f in tf:
            q = tf.index(f)
            out[f - 1, ..., 0] = rs.normal(loc=vxs[q], scale=abs(vxs[q] / 10), size=(1, S, S))[0]
            out[f - 1, ..., 1] = rs.normal(loc=vys[q], scale=abs(vys[q] / 10), size=(1, S, S))[0]
        else:
            out[f - 1] = rs.normal(loc=0, scale=0.1, size=(1, S, S, 2))[0]
    return out


def turn_frames(intervals):
    a, b, c = (int(v) for v in intervals)
    return [1, a, a + b, a + b + c]


def _pad128(d):
    a = np.zeros((S, S))
    a[:-1, :-1] = d
    return a


def loop(ring, y0, x0, intervals, T, rs, ss, masks, initial_vy=0.2, dom=None):
    """one pass -> {"density", "density_zero" (n, L, L), "velocity", "control" (n, L, L, 2), "smoke" (n, nb + 1)} float64"""
    dom = dom or oss.domain()
    each, concat, keep = oss.bucket_masks() if masks == "normal" else oss.bucket_masks_safe()
    n, L = T // rs + 1, S // ss
    rec = {"density": np.zeros((n, L, L)), "density_zero": np.zeros((n, L, L)), "velocity": np.zeros((n, L, L, 2)),
           "control": np.zeros((n, L, L, 2)), "smoke": np.zeros((n, len(each) + 1))}
    dens = np.zeros((N, N))
    dens[y0:y0 + 10, x0:x0 + 10] = 1
    dz = dens.copy()
    vel = np.zeros((S, S, 2))
    vel[..., 1] = initial_vy
    outs = np.zeros(len(each))
    state = {"dz": dz}

    def book():
        az = _pad128(state["dz"])
        if np.sum(az * concat) > 0:
            for i in range(len(each)):
                outs[i] += np.sum(az * each[i])
            state["dz"] = state["dz"] * keep[:-1, :-1]

    def fields(r):
        rec["density"][r] = _pad128(dens)[::ss, ::ss]
        rec["density_zero"][r] = _pad128(state["dz"])[::ss, ::ss]
        rec["velocity"][r] = vel[::ss, ::ss]

    def row(r):
        rec["smoke"][r, :-1] = outs
        rec["smoke"][r, -1] = np.sum(state["dz"])

    fields(0)
    book()
    row(0)
    tf = turn_frames(intervals)
    for f in range(1, T + 1):
        cf = f - 1
        c = ring[cf].copy() if f in tf else vel + ring[cf]
        c[16:112, 16:112, :] = 0
        if cf % rs == 0:
            rec["control"][cf // rs] = c[::ss, ::ss]
        vel, _ = oss.evolve(dom, vel, c[..., 0], c[..., 1])
        dens, state["dz"] = oss.advect(vel, [dens, state["dz"]])
        if f in tf[1:]:
            if f % rs == 0:                 # write_vel_density: fields first, then the book-keeping, then the smoke row
                fields(f // rs)
                book()
                row(f // rs)
        else:
            book()
            if f % rs == 0:
                fields(f // rs)
                row(f // rs)
    return rec


def accept(last_row, filter, min_sum_rate=0.85, max_sum_rate=1.15):
    """the reference's decision after the last frame, from the last smoke row of a normal-mask pass"""
    buckets, field = np.asarray(last_row[:-1]), last_row[-1]
    density_sum = np.sum(buckets) + field
    target_rule = (not filter) or (buckets[1] / density_sum > 0.8)
    return bool(target_rule and (density_sum > 100 * min_sum_rate) and (density_sum < 100 * max_sum_rate))
