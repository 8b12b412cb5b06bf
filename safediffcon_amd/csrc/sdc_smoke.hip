// Smoke score check: the fluid rollout the reference runs on every sampled control
// sequence of the 2-D smoke task --
//   solver               2d/dataset/apps/evaluate_solver.py:209-350   (one Python process per sample, 2d/inference_2d.py:389-447)
//   get_envolve          2d/dataset/apps/evaluate_solver.py:82-111     control ring + last interior velocity -> projection
//   divergence_free      phi/flow.py:317-326 ; StaggeredGrid.divergence / .gradient  phi/math/nd.py:333-344,581-592
//   sparse_pressure_matrix + conjugate_gradient   phi/solver/sparse.py:27-77, phi/solver/base.py:63-103
//   StaggeredGrid.advect phi/math/nd.py:407-428 ; SciPyBackend.resample (scipy interpn, linear)  phi/math/scipy_backend.py:55-75
//   bucket book-keeping  2d/dataset/apps/evaluate_solver.py:114-178,262-336
// (phi = the PhiFlow 1.x copy vendored beside evaluate_solver.py.)
//
// One workgroup of 512 threads carries one sample through all per_timelength - 1 steps: the 127 x 127 pressure problem lives
// on chip for the whole rollout.  The reference's CG runs in float64 (numpy), stops on |r|_max < 1e-8 or after 500 iterations
// -- on this domain it always takes the 500 -- so a step is 500 x {5-point mat-vec, three dot products, three vector
// updates} on 16 129 unknowns: thread t owns column t & 127 of the 32 rows (t >> 7) * 32 ...; x, r and A p sit in its
// registers (3 x 32 doubles = 192 VGPRs; four vectors would fill the CU's whole 512 KB register file), the search direction p
// in LDS (129 rows x 128 doubles = 129 KB of the 160 KB; rows -1 and 127 and column 127 stay zero, and column 127 of one
// row is column -1 of the next, so the open border needs no halo columns) where the neighbours read it.  CG scalars never
// leave the device: wave partials by DPP lane moves, every thread then forms alpha and beta from the same eight LDS
// partials in a fixed order (a sample's result does not depend on the batch it rides in).  Element-wise arithmetic keeps
// the reference's operation order without FMA contraction (scipy's CSC mat-vec adds a row's terms in ascending column
// order; numpy multiplies, then adds); only the dot products and the bucket sums associate differently from numpy's
// pairwise sums.  The CG's first direction update reads the NEW residual on both sides, as the reference's aliased
// in-place update does.
// Velocity (128 x 128 x 2 doubles) and the three float32 density fields (ping-pong) sit in a per-sample global workspace
// that stays in L2; they are touched once per step, the CG 500 times.
// Cost (MI355X, tools/smoke_solver_probe.py): 4.6 us per CG iteration = 0.59 s per 256-step rollout, the same for 1 or 256
// samples in the batch (one CU each).  Per iteration a thread issues ~820 VALU instructions (two waves per SIMD: ~2.7 us
// if nothing else stalled) and moves 162 doubles through LDS; the two block-wide reductions cost 0.8 us of it.  A variant
// that let A p and p share registers (p re-read from LDS under the residual update) needs ~20 VGPRs more than the 256 a
// thread has at this occupancy and ran slower on its scratch spills (6.5 us).
//
// The same kernel, instantiated with GEN, is the smoke task's data generator (sdc_smoke_datagen; 2d/dataset/apps/
// a_gen_dataset_128.py): see GenArgs below.  The score check's instantiation keeps the instruction stream it had as a plain
// kernel; a change here is checked against that ("Data generator").
#include "sdc_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SN = 127;            // cells per side
constexpr int SS = 128;            // staggered samples per side
constexpr int NTHR = 512;
constexpr int RPT = 32;            // rows per thread
constexpr int LP = 128;            // LDS pitch of p (doubles): column 127 is always zero and doubles as column -1 of the next row
constexpr int NWAVE = NTHR / 64;
constexpr int GR = 4;              // rows per prefetch group of the mat-vec
constexpr int MAXB = 8;            // buckets per label map
constexpr size_t VEL_BYTES = (size_t)SS * SS * 2 * sizeof(double);
constexpr size_t DEN_FLOATS = (size_t)SN * SS;      // pitch 128
constexpr size_t WORK_BYTES = VEL_BYTES + 6 * DEN_FLOATS * sizeof(float);

struct SmokeArgs {
    const float* c1; const float* c2; int64_t c_sb, c_sf;       // controls (B, nt, nx, nx): batch / frame strides, rows dense
    const float* dens0; int64_t d_sb;                           // (B, nx, nx)
    const float* vel0; int64_t v_sb;                            // (128, 128, 2) staggered initial velocity, stride 0 = shared
    const unsigned char* fluid;                                 // (127, 127): 1 fluid, 0 obstacle
    const unsigned char* label_n; const unsigned char* label_s; // (128, 128): 0 = none, k = bucket k - 1
    double* out;                                                // (B, nt, 7, nx, nx)
    double* out_zero;                                           // (B, nt, nx, nx) or null
    char* work; int nt, nx, T, ti, si, lo, hi, max_iter, nb_n, nb_s;
    double accuracy;
};

// Data generator (2d/dataset/apps/a_gen_dataset_128.py: get_envolve :246-312, loop_write :491-741): the same fluid step in a
// loop the kernel closes itself -- the ring of step t is the projected velocity of step t - 1 plus a noise field (or an absolute
// draw on the four turn frames), so the velocity never leaves the workspace between steps.  Two float64 density fields.
constexpr int MAXMAPS = 4;         // label maps one launch can mix (normal and safe passes ride together)
constexpr size_t DEN_DOUBLES = DEN_FLOATS;    // the same 127 x 128 cells per field
constexpr size_t GEN_WORK_BYTES = VEL_BYTES + 4 * DEN_DOUBLES * sizeof(double);

struct GenArgs {
    const double* ring; int64_t r_sb, r_sf;                     // (B, T, 128, 128, 2): batch / frame strides, frames dense
    const int32_t* start;                                       // (B, 2): y0, x0 of the 10 x 10 square of ones
    const unsigned char* sched;                                 // (B, T): frame f = 1 .. T at [f - 1]
    const int32_t* map_index;                                   // (B): which label map
    const unsigned char* fluid;                                 // (127, 127)
    const unsigned char* labels;                                // (n_maps, 128, 128): 0 = none, k = area k - 1
    double* dens; double* densz; double* vel; double* ctrl; double* smoke;
    char* work; int T, rs, ss, max_iter, n_maps, smoke_cols; int nb[MAXMAPS];
    double accuracy, initial_vy;
};

// wave64 reductions on DPP lane moves (no LDS crossbar round trips): xor 1, xor 2, half-row mirror, row mirror leave
// the sum of each row of 16 in all its lanes; the four rows are combined through v_readlane in a fixed order.
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_get(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double wsum(double v) {
    v += dpp_mov<0xB1>(v);          // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);          // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v);         // row_half_mirror
    v += dpp_mov<0x140>(v);         // row_mirror
    return ((lane_get(v, 0) + lane_get(v, 16)) + lane_get(v, 32)) + lane_get(v, 48);
}
__device__ __forceinline__ double wmax(double v) {
    v = fmax(v, dpp_mov<0xB1>(v));
    v = fmax(v, dpp_mov<0x4E>(v));
    v = fmax(v, dpp_mov<0x141>(v));
    v = fmax(v, dpp_mov<0x140>(v));
    return fmax(fmax(lane_get(v, 0), lane_get(v, 16)), fmax(lane_get(v, 32), lane_get(v, 48)));
}

// numpy's np.sum over n <= 8 doubles: n < 8 a plain loop, n == 8 the unrolled pairwise block
__device__ __forceinline__ double np_sum8(const double (&v)[MAXB], int n) {
    const double pw = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < MAXB; ++q) s = (q < n) ? s + v[q] : s;
    return n == 8 ? pw : s;
}

__device__ __forceinline__ const SmokeArgs& score_args(const SmokeArgs& A) { return A; }
__device__ __forceinline__ SmokeArgs score_args(const GenArgs&) { return SmokeArgs{}; }

// GEN = false: sdc_smoke_rollout, Args = SmokeArgs -- the controls are read.  GEN = true: sdc_smoke_datagen, Args = GenArgs --
// the ring follows from the previous step's velocity.  The two share the domain set-up and the pressure projection; everything
// under `if constexpr (GEN)` is absent from the score check's kernel.
template <bool GEN, class Args>
__global__ __launch_bounds__(NTHR) void smoke_rollout_kernel(Args A) {
    extern __shared__ double P[];                    // (SS + 1) x LP: rows -1 .. 127 (rows -1 and 127, column 127 stay zero)
    __shared__ double redA[NWAVE * 2];
    __shared__ double redB[NWAVE * 2];
    __shared__ double redK[NWAVE * 2 * (MAXB + 1)];
    __shared__ double outs[2 * MAXB];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int j = t & 127, i0 = (t >> 7) * RPT;
    const int b = blockIdx.x;
    constexpr size_t WB = GEN ? GEN_WORK_BYTES : WORK_BYTES;
    double* V = reinterpret_cast<double*>(A.work + (size_t)b * WB);
    // score check: three float32 density fields, the controls, the seven-channel output (S: an empty set in the generator)
    const auto& S = score_args(A);
    float* D = reinterpret_cast<float*>(A.work + (size_t)b * WORK_BYTES + VEL_BYTES);
    const float* c1 = S.c1 + (int64_t)b * S.c_sb;
    const float* c2 = S.c2 + (int64_t)b * S.c_sb;
    const int nx = S.nx, si = S.si, ti = S.ti;
    double* outb = S.out + (int64_t)b * S.nt * 7 * nx * nx;
    double* outz = S.out_zero ? S.out_zero + (int64_t)b * S.nt * nx * nx : nullptr;
    // generator: two float64 density fields (no-set, set-zero), this sample's schedule, label map and records
    double* G = nullptr;
    const double* ring = nullptr;
    const unsigned char* sched = nullptr;
    const unsigned char* lab = nullptr;
    int nb = 0, L = 0, nrec = 0;
    double *o_dens = nullptr, *o_densz = nullptr, *o_vel = nullptr, *o_ctrl = nullptr, *o_smoke = nullptr;
    if constexpr (GEN) {
        G = reinterpret_cast<double*>(A.work + (size_t)b * GEN_WORK_BYTES + VEL_BYTES);
        ring = A.ring + (int64_t)b * A.r_sb;
        sched = A.sched + (int64_t)b * A.T;
        const int mi = min(max(A.map_index[b], 0), A.n_maps - 1);
        lab = A.labels + (size_t)mi * SS * SS;
        nb = mi == 0 ? A.nb[0] : mi == 1 ? A.nb[1] : mi == 2 ? A.nb[2] : A.nb[3];
        L = SS / A.ss; nrec = A.T / A.rs + 1;
        o_dens = A.dens + (int64_t)b * nrec * L * L;
        o_densz = A.densz ? A.densz + (int64_t)b * nrec * L * L : nullptr;
        o_vel = A.vel + (int64_t)b * nrec * L * L * 2;
        o_ctrl = A.ctrl + (int64_t)b * nrec * L * L * 2;
        o_smoke = A.smoke + (int64_t)b * nrec * A.smoke_cols;
    }
    double* Pc = P + (i0 + 1) * LP + j;              // this thread's first cell

    // ---- domain coefficients of this thread's 32 slots (phi/solver/sparse.py:27-77, phi/flow.py:455-474)
    auto fl = [&](int i, int jj) -> int {            // fluid mask padded with ones (open border: pad_fluid)
        return (i < 0 || i >= SN || jj < 0 || jj >= SN) ? 1 : (int)A.fluid[i * SN + jj];
    };
    unsigned actm = 0, vmxm = 0, vmym = 0;
    unsigned nd4[4] = {0, 0, 0, 0};                  // 4 bits per cell: -diag (1 .. 4)
    for (int k = 0; k < RPT; ++k) {
        const int i = i0 + k;
        const int in = (i < SN && j < SN);
        const int f = fl(i, j);
        if (in && f) actm |= 1u << k;
        int nd = fl(i + 1, j) + fl(i - 1, j) + fl(i, j + 1) + fl(i, j - 1);
        if (nd < 1) nd = 1;                          // minimum(centre, -1)
        nd4[k >> 3] |= (unsigned)nd << (4 * (k & 7));
        if (min(f, fl(i, j - 1))) vmxm |= 1u << k;
        if (min(f, fl(i - 1, j))) vmym |= 1u << k;
    }
    for (int q = t; q < (SS + 1) * LP; q += NTHR) P[q] = 0.0;

    // ---- initial fields
    if constexpr (GEN) {
        // get_initial_state (a_gen_dataset_128.py:315-340): vx = 0, vy = initial_vy everywhere, a 10 x 10 square of ones
        const int y0 = A.start[2 * b], x0 = A.start[2 * b + 1];
#pragma unroll 4
        for (int k = 0; k < RPT; ++k) {
            const int i = i0 + k;
            reinterpret_cast<double2*>(V)[i * SS + j] = make_double2(0.0, A.initial_vy);
            if (i < SN) {
                const double d = (j < SN && i >= y0 && i < y0 + 10 && j >= x0 && j < x0 + 10) ? 1.0 : 0.0;
                G[0 * DEN_DOUBLES + i * SS + j] = d;
                G[2 * DEN_DOUBLES + i * SS + j] = d;
            }
            // the last control frame is never recorded (its step would be frame T + 1): it stays zero, as in the reference
            if (i % A.ss == 0 && j % A.ss == 0)
                reinterpret_cast<double2*>(o_ctrl)[((int64_t)(nrec - 1) * L + i / A.ss) * L + j / A.ss] = make_double2(0.0, 0.0);
        }
    } else {
        const float* v0 = A.vel0 + (int64_t)b * A.v_sb;
#pragma unroll 4
        for (int k = 0; k < RPT; ++k) {
            const int i = i0 + k;
            const float2 v = reinterpret_cast<const float2*>(v0)[i * SS + j];
            reinterpret_cast<double2*>(V)[i * SS + j] = make_double2((double)v.x, (double)v.y);
            if (i < SN) {
                const float d = (j < SN) ? A.dens0[(int64_t)b * A.d_sb + (i / si) * nx + (j / si)] : 0.f;
                D[0 * DEN_FLOATS + i * SS + j] = d;
                D[2 * DEN_FLOATS + i * SS + j] = d;
                D[4 * DEN_FLOATS + i * SS + j] = d;
            }
        }
    }
    if (t < 2 * MAXB) outs[t] = 0.0;                 // smoke_outs / smoke_outs_safe: uniform state, kept out of the VGPRs
    int cur = 0;                                     // density ping-pong: field f at D[(2 f + cur) * DEN_FLOATS]
    __syncthreads();

    // book-keeping of the two absorbing density copies + frame output (evaluate_solver.py:262-336); the fields at `cur`
    auto book_and_record = [&](int step) {
        if constexpr (!GEN) {
            float* dzp = D + (2 + cur) * DEN_FLOATS;
            float* dsp = D + (4 + cur) * DEN_FLOATS;
            double sn[MAXB + 1], ss[MAXB + 1];
#pragma unroll
            for (int q = 0; q <= MAXB; ++q) { sn[q] = 0.0; ss[q] = 0.0; }
            if (j < SN) {
                for (int k = 0; k < RPT; ++k) {
                    const int i = i0 + k;
                    if (i >= SN) break;
                    const int ln = A.label_n[i * SS + j], ls = A.label_s[i * SS + j];
                    const double vz = (double)dzp[i * SS + j], vs = (double)dsp[i * SS + j];
#pragma unroll
                    for (int q = 0; q <= MAXB; ++q) {
                        sn[q] += (ln == q) ? vz : 0.0;
                        ss[q] += (ls == q) ? vs : 0.0;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q <= MAXB; ++q) {
                const double a = wsum(sn[q]), c = wsum(ss[q]);
                if (lane == 0) { redK[(wave * 2 + 0) * (MAXB + 1) + q] = a; redK[(wave * 2 + 1) * (MAXB + 1) + q] = c; }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q <= MAXB; ++q) {
                double a = 0.0, c = 0.0;
                for (int w = 0; w < NWAVE; ++w) { a += redK[(w * 2 + 0) * (MAXB + 1) + q]; c += redK[(w * 2 + 1) * (MAXB + 1) + q]; }
                sn[q] = a; ss[q] = c;
            }
            double cat_n = 0.0, cat_s = 0.0;
#pragma unroll
            for (int q = 1; q <= MAXB; ++q) {
                cat_n += (q <= A.nb_n) ? sn[q] : 0.0;
                cat_s += (q <= A.nb_s) ? ss[q] : 0.0;
            }
            const bool hit_n = cat_n > 0.0, hit_s = cat_s > 0.0;
            if (t == 0) {
#pragma unroll
                for (int q = 0; q < MAXB; ++q) {
                    outs[q] += (hit_n && q < A.nb_n) ? sn[q + 1] : 0.0;
                    outs[MAXB + q] += (hit_s && q < A.nb_s) ? ss[q + 1] : 0.0;
                }
            }
            if ((hit_n || hit_s) && j < SN) {
                for (int k = 0; k < RPT; ++k) {
                    const int i = i0 + k;
                    if (i >= SN) break;
                    if (hit_n && A.label_n[i * SS + j]) dzp[i * SS + j] = 0.f;
                    if (hit_s && A.label_s[i * SS + j]) dsp[i * SS + j] = 0.f;
                }
            }
            const double tot_n = hit_n ? sn[0] : sn[0] + cat_n;
            const double tot_s = hit_s ? ss[0] : ss[0] + cat_s;
            __syncthreads();                             // zeroed cells and outs visible; redK free again
            if (step % ti == 0) {
                double outs_n[MAXB], outs_s[MAXB];
#pragma unroll
                for (int q = 0; q < MAXB; ++q) { outs_n[q] = outs[q]; outs_s[q] = outs[MAXB + q]; }
                const double rec_n = outs_n[1] / (np_sum8(outs_n, A.nb_n) + tot_n);
                const double rec_s = outs_s[0] / (np_sum8(outs_s, A.nb_s) + tot_s);
                const int f = step / ti;
                double* of = outb + (int64_t)f * 7 * nx * nx;
                const float* dp = D + (0 + cur) * DEN_FLOATS;
                if (j % si == 0) {
                    for (int k = 0; k < RPT; ++k) {
                        const int i = i0 + k;
                        if (i % si) continue;
                        const int o = (i / si) * nx + (j / si);
                        const bool in = (i < SN && j < SN);
                        of[0 * nx * nx + o] = in ? (double)dp[i * SS + j] : 0.0;
                        const double2 v = reinterpret_cast<const double2*>(V)[i * SS + j];
                        of[1 * nx * nx + o] = v.x;
                        of[2 * nx * nx + o] = v.y;
                        of[3 * nx * nx + o] = (double)c1[(int64_t)f * A.c_sf + o];
                        of[4 * nx * nx + o] = (double)c2[(int64_t)f * A.c_sf + o];
                        of[5 * nx * nx + o] = rec_n;
                        of[6 * nx * nx + o] = rec_s;
                        if (outz) outz[(int64_t)f * nx * nx + o] = in ? (double)dzp[i * SS + j] : 0.0;
                    }
                }
            }
        }
    };

    // generator: book-keeping of the set-zero copy against this sample's label map (a_gen_dataset_128.py:526-536); returns
    // the field's sum after the zeroing, the last entry of a smoke row
    auto gen_book = [&](bool apply) -> double {
        double tot = 0.0;
        if constexpr (GEN) {
            double* dzp = G + (2 + cur) * DEN_DOUBLES;
            double sn[MAXB + 1];
#pragma unroll
            for (int q = 0; q <= MAXB; ++q) sn[q] = 0.0;
            if (j < SN) {
                for (int k = 0; k < RPT; ++k) {
                    const int i = i0 + k;
                    if (i >= SN) break;
                    const int ln = lab[i * SS + j];
                    const double vz = dzp[i * SS + j];
#pragma unroll
                    for (int q = 0; q <= MAXB; ++q) sn[q] += (ln == q) ? vz : 0.0;
                }
            }
#pragma unroll
            for (int q = 0; q <= MAXB; ++q) {
                const double a = wsum(sn[q]);
                if (lane == 0) redK[wave * (MAXB + 1) + q] = a;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q <= MAXB; ++q) {
                double a = 0.0;
                for (int w = 0; w < NWAVE; ++w) a += redK[w * (MAXB + 1) + q];
                sn[q] = a;
            }
            double cat = 0.0;
#pragma unroll
            for (int q = 1; q <= MAXB; ++q) cat += (q <= nb) ? sn[q] : 0.0;
            const bool hit = apply && cat > 0.0;     // !apply: the sums only (a schedule that skips a recorded frame's book)
            if (t == 0) {
#pragma unroll
                for (int q = 0; q < MAXB; ++q) outs[q] += (hit && q < nb) ? sn[q + 1] : 0.0;
            }
            if (hit && j < SN) {
                for (int k = 0; k < RPT; ++k) {
                    const int i = i0 + k;
                    if (i >= SN) break;
                    const int ln = lab[i * SS + j];
                    if (ln && ln <= nb) dzp[i * SS + j] = 0.0;
                }
            }
            tot = hit ? sn[0] : sn[0] + cat;
            __syncthreads();                         // zeroed cells and outs visible; redK free again
        }
        return tot;
    };
    // generator: recorded frame `rec` of the two densities and the velocity, sub-sampled [::ss] (write_vel_density :460-467)
    auto gen_record = [&](int rec) {
        if constexpr (GEN) {
            const int ss = A.ss;
            const double* dp = G + (0 + cur) * DEN_DOUBLES;
            const double* dzp = G + (2 + cur) * DEN_DOUBLES;
            if (j % ss == 0) {
                for (int k = 0; k < RPT; ++k) {
                    const int i = i0 + k;
                    if (i % ss) continue;
                    const int64_t o = ((int64_t)rec * L + i / ss) * L + j / ss;
                    const bool in = (i < SN && j < SN);          // ss = 1: the 127 x 127 field inside a zero 128 x 128 frame
                    o_dens[o] = in ? dp[i * SS + j] : 0.0;
                    if (o_densz) o_densz[o] = in ? dzp[i * SS + j] : 0.0;
                    reinterpret_cast<double2*>(o_vel)[o] = reinterpret_cast<const double2*>(V)[i * SS + j];
                }
            }
        }
    };
    // generator: smoke row `rec` = the cumulative per-bucket amounts, the set-zero field's sum, zeros up to smoke_cols
    auto gen_smoke_row = [&](int rec, double tot) {
        if constexpr (GEN) {
            if (t < A.smoke_cols) o_smoke[(int64_t)rec * A.smoke_cols + t] = t < nb ? outs[min(t, MAXB - 1)] : t == nb ? tot : 0.0;
        }
    };

    if constexpr (GEN) {
        gen_record(0);                               // frame 0 is written before any book-keeping (get_initial_state)
        gen_smoke_row(0, gen_book(true));
    } else {
        book_and_record(0);
    }

    double x[RPT], r[RPT], Ap[RPT];
    for (int step = 0; step < (GEN ? A.T : A.T - 1); ++step) {
        // ---- get_envolve: control ring + last interior velocity, masked (evaluate_solver.py:92-106, phi/flow.py:300-304)
        [[maybe_unused]] int sbyte = 0;
        if constexpr (GEN) {
            // a_gen_dataset_128.py:246-312: outside [16:112, 16:112] the ring field is the value (turn frames) or is added to
            // the previous velocity; the value BEFORE the velocity mask, zero inside, is control frame step / rs
            sbyte = sched[step];
            const bool absolute = sbyte & 1;
            const bool rec = (step % A.rs == 0);
            const int ss = A.ss;
            const double* rf = ring + (int64_t)step * A.r_sf;
            const bool jin = (j >= 16 && j < 112);
#pragma unroll 4
            for (int k = 0; k < RPT; ++k) {
                const int i = i0 + k;
                double2 v = reinterpret_cast<double2*>(V)[i * SS + j];
                const bool inner = jin && i >= 16 && i < 112;
                if (!inner) {
                    const double2 n = reinterpret_cast<const double2*>(rf)[i * SS + j];
                    v.x = absolute ? n.x : v.x + n.x;
                    v.y = absolute ? n.y : v.y + n.y;
                }
                if (rec && i % ss == 0 && j % ss == 0) {
                    const int64_t o = ((int64_t)(step / A.rs) * L + i / ss) * L + j / ss;
                    reinterpret_cast<double2*>(o_ctrl)[o] = inner ? make_double2(0.0, 0.0) : v;
                }
                v.x = ((vmxm >> k) & 1) ? v.x : 0.0;
                v.y = ((vmym >> k) & 1) ? v.y : 0.0;
                reinterpret_cast<double2*>(V)[i * SS + j] = v;
            }
        } else {
            const int fr = step / ti;
            const float* c1f = c1 + (int64_t)fr * A.c_sf;
            const float* c2f = c2 + (int64_t)fr * A.c_sf;
            const bool jin = (j >= A.lo && j < A.hi);
#pragma unroll 4
            for (int k = 0; k < RPT; ++k) {
                const int i = i0 + k;
                double2 v = reinterpret_cast<double2*>(V)[i * SS + j];
                if (!(jin && i >= A.lo && i < A.hi)) {
                    const int o = (i / si) * nx + (j / si);
                    v.x = (double)c1f[o];
                    v.y = (double)c2f[o];
                }
                v.x = ((vmxm >> k) & 1) ? v.x : 0.0;
                v.y = ((vmym >> k) & 1) ? v.y : 0.0;
                reinterpret_cast<double2*>(V)[i * SS + j] = v;
            }
        }
        __syncthreads();
        // ---- divergence -> k ; CG start: x = 0, p = r = k
        double rmax;
        {
            double m = 0.0;
#pragma unroll
            for (int k = 0; k < RPT; ++k) {
                const int i = i0 + k;
                double d = 0.0;
                if (i < SN && j < SN) {
                    const double2 vc = reinterpret_cast<const double2*>(V)[i * SS + j];
                    const double vyn = V[((i + 1) * SS + j) * 2 + 1];
                    const double vxn = V[(i * SS + j + 1) * 2 + 0];
                    d = (vyn - vc.y) + (vxn - vc.x);
                }
                r[k] = d;
                x[k] = 0.0;
                Pc[k * LP] = d;
                m = fmax(m, fabs(d));
            }
            m = wmax(m);
            if (lane == 0) redB[wave] = m;
            __syncthreads();
            rmax = redB[0];
            for (int w = 1; w < NWAVE; ++w) rmax = fmax(rmax, redB[w]);
        }
        // ---- conjugate_gradient (phi/solver/base.py:63-103)
        for (int it = 0; rmax >= A.accuracy && it < A.max_iter; ++it) {
            __syncthreads();                         // p (and the previous partials' readers) settled
            asm volatile("" : "+v"(nd4[0]), "+v"(nd4[1]), "+v"(nd4[2]), "+v"(nd4[3]), "+v"(actm));   // keep the per-cell
                                                     // coefficients packed: no hoisted float64 copies in VGPRs
            double s1 = 0.0, s2 = 0.0;
            {
                // mat-vec in groups of four rows, the next group's neighbours in flight while this one is computed
                const double* Pl = Pc - 1;
                const double* Pr = Pc + 1;
                double L[2][GR], R[2][GR], Dn[2][GR];
#pragma unroll
                for (int q = 0; q < GR; ++q) { L[0][q] = Pl[q * LP]; R[0][q] = Pr[q * LP]; Dn[0][q] = Pc[(q + 1) * LP]; }
                double up = Pc[-LP], c = Pc[0];
#pragma unroll
                for (int g = 0; g < RPT / GR; ++g) {
                    if (g + 1 < RPT / GR) {
#pragma unroll
                        for (int q = 0; q < GR; ++q) {
                            const int k = (g + 1) * GR + q;
                            L[(g + 1) & 1][q] = Pl[k * LP];
                            R[(g + 1) & 1][q] = Pr[k * LP];
                            Dn[(g + 1) & 1][q] = Pc[(k + 1) * LP];
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int q = 0; q < GR; ++q) {
                        const int k = g * GR + q;
                        const double dn = Dn[g & 1][q];
                        const double dk = (double)((nd4[k >> 3] >> (4 * (k & 7))) & 15u);
                        double y = up + L[g & 1][q];   // a row's terms in ascending column index: (i-1,j), (i,j-1), (i,j), (i,j+1), (i+1,j)
                        y = y - c * dk;
                        y = y + R[g & 1][q];
                        y = y + dn;
                        const int m = ((int)(actm << (31 - k))) >> 31;
                        y = __hiloint2double(__double2hiint(y) & m, __double2loint(y) & m);
                        Ap[k] = y;
                        s1 = __builtin_fma(c, y, s1);
                        s2 = __builtin_fma(c, r[k], s2);
                        up = c;
                        c = dn;
                    }
                }
            }
            s1 = wsum(s1);
            s2 = wsum(s2);
            if (lane == 0) { redA[wave * 2] = s1; redA[wave * 2 + 1] = s2; }
            __syncthreads();
            double tmp = 0.0, pr = 0.0;
#pragma unroll
            for (int w = 0; w < NWAVE; ++w) { tmp += redA[w * 2]; pr += redA[w * 2 + 1]; }
            const double a = pr / tmp;
            double s3 = 0.0, m = 0.0;
#pragma unroll
            for (int k = 0; k < RPT; ++k) {
                const double rn = r[k] - a * Ap[k];
                r[k] = rn;
                s3 = __builtin_fma(rn, Ap[k], s3);
                m = fmax(m, fabs(rn));
            }
            s3 = wsum(s3);
            m = wmax(m);
            if (lane == 0) { redB[wave * 2] = s3; redB[wave * 2 + 1] = m; }
            __syncthreads();
            double rAp = 0.0;
            rmax = 0.0;
#pragma unroll
            for (int w = 0; w < NWAVE; ++w) { rAp += redB[w * 2]; rmax = fmax(rmax, redB[w * 2 + 1]); }
            const double bb = -rAp / tmp;
            if (it == 0) {                           // the reference's first update reads the new residual as momentum
#pragma unroll
                for (int k = 0; k < RPT; ++k) {
                    x[k] = x[k] + a * Pc[k * LP];
                    Pc[k * LP] = r[k] + bb * r[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < RPT; ++k) {
                    const double po = Pc[k * LP];
                    x[k] = x[k] + a * po;
                    Pc[k * LP] = r[k] + bb * po;
                }
            }
        }
        // ---- velocity -= mask * gradient(pressure), masked again (phi/flow.py:317-326, evaluate_solver.py:109)
        __syncthreads();
#pragma unroll
        for (int k = 0; k < RPT; ++k) Pc[k * LP] = x[k];
        __syncthreads();
        {
            const int cj = min(j, SN - 1), cjm = min(max(j - 1, 0), SN - 1);
#pragma unroll 4
            for (int k = 0; k < RPT; ++k) {
                const int i = i0 + k;
                const int ci = min(i, SN - 1), cim = min(max(i - 1, 0), SN - 1);
                const double pc = P[(ci + 1) * LP + cj];
                const double gx = pc - P[(ci + 1) * LP + cjm];
                const double gy = pc - P[(cim + 1) * LP + cj];
                double2 v = reinterpret_cast<double2*>(V)[i * SS + j];
                v.x = ((vmxm >> k) & 1) ? v.x - gx : 0.0;
                v.y = ((vmym >> k) & 1) ? v.y - gy : 0.0;
                reinterpret_cast<double2*>(V)[i * SS + j] = v;
            }
        }
        __syncthreads();
        // ---- three semi-Lagrangian advections through the new velocity (phi/math/nd.py:407-428, scipy interpn linear)
        // (generator: its two float64 fields through the same arithmetic, nothing rounded to float32)
        using F = std::conditional_t<GEN, double, float>;
        F* const FB = [&] { if constexpr (GEN) return G; else return D; }();
        if (j < SN) {
            const F* s0 = FB + (0 + cur) * DEN_FLOATS; F* d0 = FB + (0 + (cur ^ 1)) * DEN_FLOATS;
            const F* s1p = FB + (2 + cur) * DEN_FLOATS; F* d1 = FB + (2 + (cur ^ 1)) * DEN_FLOATS;
            [[maybe_unused]] const F* s2p = FB + (4 + cur) * DEN_FLOATS; [[maybe_unused]] F* d2 = FB + (4 + (cur ^ 1)) * DEN_FLOATS;
#pragma unroll 2
            for (int k = 0; k < RPT; ++k) {
                const int i = i0 + k;
                if (i >= SN) break;
                const double2 vc = reinterpret_cast<const double2*>(V)[i * SS + j];
                const double cy = (V[((i + 1) * SS + j) * 2 + 1] + vc.y) / 2;
                const double cx = (V[(i * SS + j + 1) * 2 + 0] + vc.x) / 2;
                double yy = (double)i - cy, xx = (double)j - cx;
                yy = fmax(0.0, fmin((double)SN, yy));
                xx = fmax(0.0, fmin((double)SN, xx));
                const bool oob = (yy > (double)(SN - 1)) || (xx > (double)(SN - 1));
                int iy = (int)floor(yy), ix = (int)floor(xx);
                iy = min(max(iy, 0), SN - 2);
                ix = min(max(ix, 0), SN - 2);
                const double ty = yy - (double)iy, tx = xx - (double)ix;
                const double sy = 1.0 - ty, sx = 1.0 - tx;
                const double w00 = sy * sx, w01 = sy * tx, w10 = ty * sx, w11 = ty * tx;
                const int o = iy * SS + ix;
                auto samp = [&](const F* s) -> F {
                    double v = (double)s[o] * w00;
                    v = v + (double)s[o + 1] * w01;
                    v = v + (double)s[o + SS] * w10;
                    v = v + (double)s[o + SS + 1] * w11;
                    return oob ? (F)0 : (F)v;
                };
                d0[i * SS + j] = samp(s0);
                d1[i * SS + j] = samp(s1p);
                if constexpr (!GEN) d2[i * SS + j] = samp(s2p);
            }
        }
        cur ^= 1;
        __syncthreads();
        if constexpr (GEN) {
            // loop_write's order (a_gen_dataset_128.py:568-728): ordinary frames book, then record every rs-th; the later turn
            // frames record first (write_vel_density) and skip the book-keeping when they are not recorded.  A recorded frame
            // always gets its fields and its smoke row, whatever the schedule says: every output element is written.
            const int f = step + 1, mode = (sbyte >> 1) & 3;
            const bool due = (f % A.rs == 0);
            if (due && mode == 2) gen_record(f / A.rs);
            double tot = 0.0;
            if (mode != 0 || due) tot = gen_book(mode != 0);
            if (due && mode != 2) gen_record(f / A.rs);
            if (due) gen_smoke_row(f / A.rs, tot);
        } else {
            book_and_record(step + 1);
        }
    }
}



std::atomic<uint64_t> g_smoke_lds{0};
std::atomic<uint64_t> g_datagen_lds{0};

}  // namespace

extern "C" size_t sdc_smoke_rollout_workspace_bytes(int B) { return (size_t)(B > 0 ? B : 0) * WORK_BYTES; }

extern "C" int sdc_smoke_rollout(const float* c1, const float* c2, int64_t ctrl_b_stride, int64_t ctrl_f_stride,
                                 const float* init_density, int64_t dens_b_stride, const float* init_velocity,
                                 int64_t vel_b_stride, const unsigned char* fluid_mask, const unsigned char* bucket_labels,
                                 const unsigned char* safe_labels, int n_buckets, int n_safe, double* out, double* out_zero,
                                 void* work, size_t work_bytes, int B, int nt, int nx, int per_timelength, int ring_lo,
                                 int ring_hi, double accuracy, int max_iterations, void* stream) {
    SDC_REQUIRE(c1 && c2 && init_density && init_velocity && fluid_mask && bucket_labels && safe_labels && out && work,
                SDC_ENULL, "sdc_smoke_rollout: null pointer");
    SDC_REQUIRE(B > 0 && nt > 0 && nx > 0 && per_timelength > 0, SDC_EINVAL, "sdc_smoke_rollout: bad sizes");
    SDC_REQUIRE(SS % nx == 0, SDC_EINVAL, "sdc_smoke_rollout: nx = %d does not divide 128 (evaluate_solver.py:228)", nx);
    SDC_REQUIRE(per_timelength % nt == 0, SDC_EINVAL, "sdc_smoke_rollout: per_timelength = %d is not a multiple of nt = %d",
                per_timelength, nt);
    SDC_REQUIRE(n_buckets >= 2 && n_buckets <= MAXB && n_safe >= 1 && n_safe <= MAXB, SDC_EINVAL,
                "sdc_smoke_rollout: bucket counts %d / %d outside [2, %d] / [1, %d]", n_buckets, n_safe, MAXB, MAXB);
    SDC_REQUIRE(ring_lo >= 0 && ring_lo <= ring_hi && ring_hi <= SS, SDC_EINVAL, "sdc_smoke_rollout: bad control ring");
    SDC_REQUIRE(max_iterations >= 0, SDC_EINVAL, "sdc_smoke_rollout: max_iterations < 0");
    SDC_REQUIRE(work_bytes >= (size_t)B * WORK_BYTES, SDC_EINVAL, "sdc_smoke_rollout: workspace %zu < %zu bytes", work_bytes,
                (size_t)B * WORK_BYTES);
    SDC_REQUIRE((reinterpret_cast<uintptr_t>(work) & 15) == 0 && (reinterpret_cast<uintptr_t>(init_velocity) & 7) == 0 &&
                    (vel_b_stride & 1) == 0,
                SDC_EALIGN, "sdc_smoke_rollout: workspace must be 16-byte, init_velocity 8-byte aligned");
    const int lds = (SS + 1) * LP * (int)sizeof(double);
    SDC_LDS_OPTIN(g_smoke_lds, (smoke_rollout_kernel<false, SmokeArgs>), lds, "sdc_smoke_rollout");
    SmokeArgs a;
    a.c1 = c1; a.c2 = c2; a.c_sb = ctrl_b_stride; a.c_sf = ctrl_f_stride;
    a.dens0 = init_density; a.d_sb = dens_b_stride;
    a.vel0 = init_velocity; a.v_sb = vel_b_stride;
    a.fluid = fluid_mask; a.label_n = bucket_labels; a.label_s = safe_labels;
    a.out = out; a.out_zero = out_zero; a.work = static_cast<char*>(work);
    a.nt = nt; a.nx = nx; a.T = per_timelength; a.ti = per_timelength / nt; a.si = SS / nx;
    a.lo = ring_lo; a.hi = ring_hi; a.max_iter = max_iterations; a.nb_n = n_buckets; a.nb_s = n_safe;
    a.accuracy = accuracy;
    hipLaunchKernelGGL((smoke_rollout_kernel<false, SmokeArgs>), dim3(B), dim3(NTHR), lds, sdc::as_stream(stream), a);
    return sdc::check_launch("sdc_smoke_rollout");
}

extern "C" size_t sdc_smoke_datagen_workspace_bytes(int B) { return (size_t)(B > 0 ? B : 0) * GEN_WORK_BYTES; }

extern "C" int sdc_smoke_datagen(const double* ring, int64_t ring_b_stride, int64_t ring_f_stride, const int32_t* start_yx,
                                 const unsigned char* schedule, const int32_t* map_index, const unsigned char* label_maps,
                                 const int32_t* map_buckets, int n_maps, const unsigned char* fluid_mask, double initial_vy,
                                 double* density, double* density_zero, double* velocity, double* control, double* smoke,
                                 int smoke_cols, void* work, size_t work_bytes, int B, int T, int rs, int ss, double accuracy,
                                 int max_iterations, void* stream) {
    SDC_REQUIRE(ring && start_yx && schedule && map_index && label_maps && map_buckets && fluid_mask && density && velocity &&
                    control && smoke && work,
                SDC_ENULL, "sdc_smoke_datagen: null pointer");
    SDC_REQUIRE(B > 0 && T > 0 && rs > 0 && ss > 0, SDC_EINVAL, "sdc_smoke_datagen: bad sizes");
    SDC_REQUIRE(T % rs == 0, SDC_EINVAL, "sdc_smoke_datagen: T = %d is not a multiple of rs = %d", T, rs);
    SDC_REQUIRE(SS % ss == 0, SDC_EINVAL, "sdc_smoke_datagen: ss = %d does not divide 128", ss);
    SDC_REQUIRE(n_maps >= 1 && n_maps <= MAXMAPS, SDC_EINVAL, "sdc_smoke_datagen: %d label maps outside [1, %d]", n_maps, MAXMAPS);
    int nb_max = 0;
    for (int m = 0; m < n_maps; ++m) {
        SDC_REQUIRE(map_buckets[m] >= 2 && map_buckets[m] <= MAXB, SDC_EINVAL,
                    "sdc_smoke_datagen: bucket count %d of label map %d outside [2, %d]", map_buckets[m], m, MAXB);
        nb_max = map_buckets[m] > nb_max ? map_buckets[m] : nb_max;
    }
    SDC_REQUIRE(smoke_cols >= nb_max + 1 && smoke_cols <= 2 * MAXB, SDC_EINVAL,
                "sdc_smoke_datagen: smoke_cols = %d outside [%d, %d]", smoke_cols, nb_max + 1, 2 * MAXB);
    SDC_REQUIRE(max_iterations >= 0, SDC_EINVAL, "sdc_smoke_datagen: max_iterations < 0");
    SDC_REQUIRE(work_bytes >= (size_t)B * GEN_WORK_BYTES, SDC_EINVAL, "sdc_smoke_datagen: workspace %zu < %zu bytes", work_bytes,
                (size_t)B * GEN_WORK_BYTES);
    SDC_REQUIRE((reinterpret_cast<uintptr_t>(work) & 15) == 0 && (reinterpret_cast<uintptr_t>(ring) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(velocity) & 15) == 0 && (reinterpret_cast<uintptr_t>(control) & 15) == 0 &&
                    (ring_b_stride & 1) == 0 && (ring_f_stride & 1) == 0,
                SDC_EALIGN, "sdc_smoke_datagen: workspace, ring, velocity and control must be 16-byte aligned, ring strides even");
    SDC_REQUIRE(((reinterpret_cast<uintptr_t>(density) | reinterpret_cast<uintptr_t>(density_zero) |
                  reinterpret_cast<uintptr_t>(smoke)) & 7) == 0 && ((reinterpret_cast<uintptr_t>(start_yx) |
                  reinterpret_cast<uintptr_t>(map_index)) & 3) == 0,
                SDC_EALIGN, "sdc_smoke_datagen: density / smoke must be 8-byte, start_yx / map_index 4-byte aligned");
    const int lds = (SS + 1) * LP * (int)sizeof(double);
    SDC_LDS_OPTIN(g_datagen_lds, (smoke_rollout_kernel<true, GenArgs>), lds, "sdc_smoke_datagen");
    GenArgs a;
    a.ring = ring; a.r_sb = ring_b_stride; a.r_sf = ring_f_stride;
    a.start = start_yx; a.sched = schedule; a.map_index = map_index; a.fluid = fluid_mask; a.labels = label_maps;
    a.dens = density; a.densz = density_zero; a.vel = velocity; a.ctrl = control; a.smoke = smoke;
    a.work = static_cast<char*>(work);
    a.T = T; a.rs = rs; a.ss = ss; a.max_iter = max_iterations; a.n_maps = n_maps; a.smoke_cols = smoke_cols;
    for (int m = 0; m < MAXMAPS; ++m) a.nb[m] = m < n_maps ? map_buckets[m] : 0;
    a.accuracy = accuracy; a.initial_vy = initial_vy;
    hipLaunchKernelGGL((smoke_rollout_kernel<true, GenArgs>), dim3(B), dim3(NTHR), lds, sdc::as_stream(stream), a);
    return sdc::check_launch("sdc_smoke_datagen");
}
