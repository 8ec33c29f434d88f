// Eval-step pose metrics on the device: the per-sample values of the reference's Metrics.compute_metrics
// (src/lightning/utils/metrics/metric_utils.py): R / t / in-plane errors (query_pose_error, :162-211), proj2D
// (process_single_bs_2d, :255-306), ADD and ADD-S (process_single_bs_add, :331-424).
//
// Two launches per call:
//   1. adds_pairs_kernel  -- the exact nearest-neighbour search of ADD-S.  ||R_p x_j + t_p - y_i|| = ||x_j - R_p^T (y_i - t_p)||,
//      so with y_i = R_g x_i + t_g the query is q_i = A x_i + c (A = R_p^T R_g, c = R_p^T (t_g - t_p), fp64, rounded to fp32
//      once) and the candidates are the RAW model points.  A block takes 1024 queries (4 per lane, in registers) against one
//      candidate chunk, staged through LDS as float4 (every lane reads the same address: a broadcast).  Direct differences on
//      the fp32 VALU, no |x|^2 + |y|^2 - 2 x.y form (cancellation near d = 0, exactly where ADD-S matters).  The minimum squared
//      distance of every (query, chunk) goes to the workspace; a min is exact, so the chunk split cannot change a result.
//   2. finalise_kernel    -- one block per pose: min over the chunks, sqrt, ADD and proj2D per point in fp64, fixed-order fp64
//      sums (thread-strided, then one LDS tree) and the per-pose R / t / in-plane errors in fp64.  No atomics anywhere: a pose's
//      six values depend on its own inputs only, not on the batch around it, the chunk count or the stream.
#include "bd_common.h"

namespace {

constexpr int PM_THREADS = 256;
constexpr int PM_Q = 4;                             // queries per lane
constexpr int PM_QTILE = PM_THREADS * PM_Q;         // queries per block
constexpr int PM_CTILE = 512;                       // candidates per LDS stage (8 KiB of float4)
constexpr int PM_MAX_POINTS = 1 << 26;
constexpr int PM_MAX_SPLIT = 64;
constexpr int PM_TARGET_BLOCKS = 2048;              // ~8 blocks (32 waves) per CU on 256 CUs

// candidate chunks per pose: enough blocks to fill the chip, chunks of at least 256 candidates
int pm_split(int n_poses, int max_points) {
    const long long tiles = (max_points + PM_QTILE - 1) / PM_QTILE;
    long long s = (PM_TARGET_BLOCKS + n_poses * tiles - 1) / (n_poses * tiles);
    const long long cap = max_points / 256 > 1 ? max_points / 256 : 1;
    if (s > cap) s = cap;
    if (s > PM_MAX_SPLIT) s = PM_MAX_SPLIT;
    return s < 1 ? 1 : (int)s;
}

struct PosePair {
    double Rp[9], tp[3], Rg[9], tg[3];
};

// the reference's composition (:480-483, :282-283): pred[:3, 3] *= scale, then pred @ coordinate_transform; gt = original_poses[:3]
__device__ PosePair load_poses(int b, const float* pred, const float* gt, const float* scale, const float* ct) {
    PosePair p;
    const float* P = pred + b * 16;
    const float* G = gt + b * 16;
    const float* C = ct + b * 16;
    const float* s = scale + b * 3;
    for (int i = 0; i < 3; ++i) {
        double row[4] = {(double)P[i * 4 + 0], (double)P[i * 4 + 1], (double)P[i * 4 + 2], (double)P[i * 4 + 3] * (double)s[i]};
        for (int j = 0; j < 4; ++j) {
            double v = 0.0;
            for (int k = 0; k < 4; ++k) v += row[k] * (double)C[k * 4 + j];
            if (j < 3) p.Rp[i * 3 + j] = v; else p.tp[i] = v;
        }
        for (int j = 0; j < 3; ++j) p.Rg[i * 3 + j] = (double)G[i * 4 + j];
        p.tg[i] = (double)G[i * 4 + 3];
    }
    return p;
}

__global__ __launch_bounds__(PM_THREADS) void adds_pairs_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                 const float* __restrict__ scale, const float* __restrict__ ct,
                                                                 const float* __restrict__ pts, const int64_t* __restrict__ pt_offset,
                                                                 const int32_t* __restrict__ pt_count, int max_points, int split,
                                                                 float* __restrict__ minsq) {
    __shared__ float4 cand[PM_CTILE];
    const int b = blockIdx.y, tile = blockIdx.x / split, s = blockIdx.x % split, tid = threadIdx.x;
    const int n = pt_count[b];
    if (n <= 0 || n > max_points) return;                      // finalise_kernel reports NaN for such a pose
    const int q0 = tile * PM_QTILE;
    if (q0 >= n) return;
    const float* x = pts + pt_offset[b] * 3;
    const PosePair p = load_poses(b, pred, gt, scale, ct);
    double A[9], c[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) A[i * 3 + j] = p.Rp[0 * 3 + i] * p.Rg[0 * 3 + j] + p.Rp[1 * 3 + i] * p.Rg[1 * 3 + j] + p.Rp[2 * 3 + i] * p.Rg[2 * 3 + j];
        c[i] = p.Rp[0 * 3 + i] * (p.tg[0] - p.tp[0]) + p.Rp[1 * 3 + i] * (p.tg[1] - p.tp[1]) + p.Rp[2 * 3 + i] * (p.tg[2] - p.tp[2]);
    }
    float qx[PM_Q], qy[PM_Q], qz[PM_Q], m[PM_Q];
#pragma unroll
    for (int k = 0; k < PM_Q; ++k) {
        const int i = q0 + k * PM_THREADS + tid;
        const int ii = i < n ? i : n - 1;
        const double x0 = x[ii * 3 + 0], x1 = x[ii * 3 + 1], x2 = x[ii * 3 + 2];
        qx[k] = (float)(A[0] * x0 + A[1] * x1 + A[2] * x2 + c[0]);
        qy[k] = (float)(A[3] * x0 + A[4] * x1 + A[5] * x2 + c[1]);
        qz[k] = (float)(A[6] * x0 + A[7] * x1 + A[8] * x2 + c[2]);
        m[k] = INFINITY;
    }
    const int chunk = (n + split - 1) / split;
    const int c0 = s * chunk, c1 = min(n, c0 + chunk);
    for (int base = c0; base < c1; base += PM_CTILE) {
        const int cnt = min(PM_CTILE, c1 - base);
        __syncthreads();                                       // the previous stage has been read
        for (int j = tid; j < cnt; j += PM_THREADS) {
            const float* v = x + (int64_t)(base + j) * 3;
            cand[j] = make_float4(v[0], v[1], v[2], 0.f);
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const float4 v = cand[j];
#pragma unroll
            for (int k = 0; k < PM_Q; ++k) {
                const float dx = v.x - qx[k], dy = v.y - qy[k], dz = v.z - qz[k];
                m[k] = fminf(m[k], fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
            }
        }
    }
    float* out = minsq + ((int64_t)b * split + s) * max_points;
#pragma unroll
    for (int k = 0; k < PM_Q; ++k) {
        const int i = q0 + k * PM_THREADS + tid;
        if (i < n) out[i] = m[k];
    }
}

__device__ __forceinline__ double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ bool is_finite(double v) { return !isnan(v) && !isinf(v); }

__global__ __launch_bounds__(PM_THREADS) void finalise_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                               const float* __restrict__ scale, const float* __restrict__ ct,
                                                               const float* __restrict__ Kmat, const float* __restrict__ pts,
                                                               const int64_t* __restrict__ pt_offset, const int32_t* __restrict__ pt_count,
                                                               int max_points, int split, int t_scale, const float* __restrict__ minsq,
                                                               double* __restrict__ out) {
    __shared__ double red[3][PM_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = pt_count[b];
    const PosePair p = load_poses(b, pred, gt, scale, ct);
    double K[9];
    for (int i = 0; i < 9; ++i) K[i] = (double)Kmat[b * 9 + i];
    double s_proj = 0.0, s_add = 0.0, s_adds = 0.0;
    const bool ok = n > 0 && n <= max_points;
    if (ok) {
        const float* x = pts + pt_offset[b] * 3;
        const float* ms = minsq + (int64_t)b * split * max_points;
        for (int i = tid; i < n; i += PM_THREADS) {
            const double x0 = x[(int64_t)i * 3 + 0], x1 = x[(int64_t)i * 3 + 1], x2 = x[(int64_t)i * 3 + 2];
            double yp[3], yg[3];
            for (int r = 0; r < 3; ++r) {
                yp[r] = p.Rp[r * 3 + 0] * x0 + p.Rp[r * 3 + 1] * x1 + p.Rp[r * 3 + 2] * x2 + p.tp[r];
                yg[r] = p.Rg[r * 3 + 0] * x0 + p.Rg[r * 3 + 1] * x1 + p.Rg[r * 3 + 2] * x2 + p.tg[r];
            }
            const double e0 = yp[0] - yg[0], e1 = yp[1] - yg[1], e2 = yp[2] - yg[2];
            s_add += sqrt(e0 * e0 + e1 * e1 + e2 * e2);
            // project_optimized (:224-239): K (R x + t), then xy / z -- unclamped, so z == 0 gives numpy's inf / NaN
            double up[3], ug[3];
            for (int r = 0; r < 3; ++r) {
                up[r] = K[r * 3 + 0] * yp[0] + K[r * 3 + 1] * yp[1] + K[r * 3 + 2] * yp[2];
                ug[r] = K[r * 3 + 0] * yg[0] + K[r * 3 + 1] * yg[1] + K[r * 3 + 2] * yg[2];
            }
            const double d0 = up[0] / up[2] - ug[0] / ug[2], d1 = up[1] / up[2] - ug[1] / ug[2];
            s_proj += sqrt(d0 * d0 + d1 * d1);
            float m = ms[i];
            for (int s = 1; s < split; ++s) m = fminf(m, ms[(int64_t)s * max_points + i]);
            s_adds += sqrt((double)m);
        }
    }
    red[0][tid] = s_proj; red[1][tid] = s_add; red[2][tid] = s_adds;
    for (int w = PM_THREADS / 2; w > 0; w >>= 1) {
        __syncthreads();
        if (tid < w) for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + w];
    }
    if (tid != 0) return;
    double* o = out + (int64_t)b * 6;
    // query_pose_error (:162-211) on the composed pose
    double D[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) D[i * 3 + j] = p.Rp[i * 3 + 0] * p.Rg[j * 3 + 0] + p.Rp[i * 3 + 1] * p.Rg[j * 3 + 1] + p.Rp[i * 3 + 2] * p.Rg[j * 3 + 2];
    const double rad2deg = 180.0 / M_PI;
    const double tr = clampd(D[0] + D[4] + D[8], -1.0, 3.0);
    const double r_err = acos(clampd((tr - 1.0) / 2.0, -1.0, 1.0)) * rad2deg;
    const double t0 = p.tp[0] - p.tg[0], t1 = p.tp[1] - p.tg[1], t2 = p.tp[2] - p.tg[2];
    double t_err = sqrt(t0 * t0 + t1 * t1 + t2 * t2);
    if (t_scale == 1) t_err *= 100.0;
    else if (t_scale == 2) t_err /= 10.0;
    o[0] = is_finite(r_err) ? r_err : 0.0;                       // NaN / inf -> 0, as the reference
    o[1] = is_finite(t_err) ? t_err : 0.0;
    o[2] = fabs(atan2(D[3], D[0]) * rad2deg);
    o[3] = ok ? red[0][0] / (double)n : (double)NAN;
    o[4] = ok ? red[1][0] / (double)n : (double)NAN;
    o[5] = ok ? red[2][0] / (double)n : (double)NAN;
}

}  // namespace

extern "C" size_t bd_pose_metrics_workspace_bytes(int n_poses, int max_points) {
    if (n_poses <= 0 || n_poses > 65535 || max_points <= 0 || max_points > PM_MAX_POINTS) return 0;
    return (size_t)n_poses * (size_t)pm_split(n_poses, max_points) * (size_t)max_points * sizeof(float);
}

extern "C" int bd_pose_metrics(const float* pred_poses, const float* original_poses, const float* scale, const float* coordinate_transform,
                               const float* original_intrinsics, const float* points, const int64_t* pt_offset, const int32_t* pt_count,
                               int n_poses, int max_points, int t_scale, void* workspace, size_t workspace_bytes, double* out,
                               void* stream) {
    if (!pred_poses || !original_poses || !scale || !coordinate_transform || !original_intrinsics || !points || !pt_offset || !pt_count ||
        !workspace || !out)
        return BD_ERR_NULL;
    if (n_poses <= 0 || n_poses > 65535 || max_points <= 0 || max_points > PM_MAX_POINTS || t_scale < 0 || t_scale > 2) return BD_ERR_SHAPE;
    if (workspace_bytes < bd_pose_metrics_workspace_bytes(n_poses, max_points)) return BD_ERR_WORKSPACE;
    const int split = pm_split(n_poses, max_points);
    const int tiles = (max_points + PM_QTILE - 1) / PM_QTILE;
    hipStream_t s = (hipStream_t)stream;
    float* minsq = (float*)workspace;
    hipLaunchKernelGGL(adds_pairs_kernel, dim3(tiles * split, n_poses), dim3(PM_THREADS), 0, s, pred_poses, original_poses, scale,
                       coordinate_transform, points, pt_offset, pt_count, max_points, split, minsq);
    hipLaunchKernelGGL(finalise_kernel, dim3(n_poses), dim3(PM_THREADS), 0, s, pred_poses, original_poses, scale, coordinate_transform,
                       original_intrinsics, points, pt_offset, pt_count, max_points, split, t_scale, minsq, out);
    BD_CHECK_LAUNCH();
    return BD_OK;
}
