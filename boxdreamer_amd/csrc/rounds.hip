// Dense multi-round decode over a reference bank (dense.py: process_multi_round's banked form).  Two small latency-bound kernels that
// keep the facade from waiting for the device between the selection the device made (bd_match_select_rows) and the decoder:
//
//   bd_round_sources     the source table of the (B * R, sub + 1) multi-round batch, R = ceil(k / sub): sub consecutive kept
//                        references per round, the last round padded with the bank's all-zero view, the query last
//   bd_pose_select_rows  the fine level's choice (dense.fetch_neighbors_by_pose_similarity) among the kept references, from the
//                        poses the bank keeps: distance, the fk nearest in position order, their source table
//
// Both follow bd_match_select_rows' conventions (match.hip): one workgroup per sample, no atomics, every sum in index order (a
// sample's bits do not depend on the batch), arguments checked before any launch, inconsistent device data reads and writes nothing
// out of bounds.
#include "bd_common.h"

namespace {

constexpr int MAXK = 1024;
constexpr int32_t NO_VIEW = 0x7fffffff;  // a `src` entry bd_gather_view_rows / bd_assemble_entry_tokens skip (match.hip)

// The bank row of candidate position c of one sample: rows[cand[c]], NO_VIEW when the slot or the row is out of range.
__device__ __forceinline__ int32_t candidate_row(const int32_t* __restrict__ row, const int32_t* __restrict__ cand, int c, int N_max, int R) {
    const int slot = cand[c];
    if (slot < 0 || slot >= N_max) return NO_VIEW;
    const int r = row[slot];
    return r >= 0 && r < R ? r : NO_VIEW;
}

// one workgroup (4 waves) per sample; the sample's k resolved rows go through LDS once, every round reads them from there
__global__ __launch_bounds__(256) void round_sources_kernel(const int32_t* __restrict__ rows, const int32_t* __restrict__ cand, int R,
                                                             int N_max, int k, int sub, int32_t zero_row, int per_round_query,
                                                             int32_t* __restrict__ src, int32_t* __restrict__ view) {
    __shared__ int32_t tab[MAXK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int32_t* row = rows + (int64_t)b * N_max;
    const int32_t* cd = cand + (int64_t)b * k;
    for (int c = tid; c < k; c += 256) tab[c] = candidate_row(row, cd, c, N_max, R);
    __syncthreads();
    const int rounds = (k + sub - 1) / sub, w = sub + 1, n = rounds * w;
    int32_t* out_src = src + (int64_t)b * n;
    int32_t* out_view = view + (int64_t)b * n;
    for (int e = tid; e < n; e += 256) {
        const int r = e / w, j = e - r * w;
        int32_t s, v;
        if (j == sub) {
            s = -((per_round_query ? b * rounds + r : b) + 1);
            v = k;
        } else {
            const int c = r * sub + j;
            s = c < k ? tab[c] : zero_row;
            v = c < k ? c : -1;
        }
        out_src[e] = s;
        out_view[e] = v;
    }
}

// The order bd_pose_select_rows ranks by, on the stored fp32 distance: numbers before NaNs, smaller before larger (+inf an ordinary
// value), equal ones -- and NaNs among themselves -- by position.
__device__ __forceinline__ bool ranks_before(float va, int pa, float vb, int pb) {
    const bool na = va != va, nb = vb != vb;
    if (na != nb) return nb;
    if (na || va == vb) return pa < pb;
    return va < vb;
}

// The distance in fp64 from the fp32 inputs, every product and sum rounded on its own in the order the header states (the nine
// products of the trace are exact in fp64; the squares of the translation are not, so nothing here may be contracted).
__device__ __forceinline__ double pose_distance(const float* __restrict__ p, const float* __restrict__ g) {
#pragma clang fp contract(off)
    double tr = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) tr = tr + (double)p[i * 4 + j] * (double)g[i * 4 + j];
    double x = (tr - 1.0) / 2.0;
    x = x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x);          // (comparisons, not fmin / fmax: a NaN stays a NaN, as in torch.clamp)
    double ss = 0.0;
    for (int i = 0; i < 3; ++i) {
        const double d = (double)p[i * 4 + 3] - (double)g[i * 4 + 3];
        ss = ss + d * d;
    }
    return acos(x) + sqrt(ss);
}

// one workgroup (4 waves) per sample.  A candidate's rank is the number of valid candidates that rank before it: k reads of the LDS
// table per candidate (every lane reads the same word: a broadcast), no reduction and no barrier inside a loop; at k = 1024 that is
// 4096 compares per thread, at the k of a real database (20 .. 64) a few dozen.
__global__ __launch_bounds__(256) void pose_select_rows_kernel(const float* __restrict__ bank_poses, int R, const float* __restrict__ pred,
                                                                const int32_t* __restrict__ rows, const int32_t* __restrict__ cand,
                                                                int N_max, int k, int fk, float* __restrict__ dist,
                                                                int32_t* __restrict__ fine_pos, int32_t* __restrict__ src) {
    __shared__ float val[MAXK];
    __shared__ int32_t tab[MAXK];          // the candidate's bank row, NO_VIEW: not a candidate
    __shared__ unsigned char chosen[MAXK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int32_t* row = rows + (int64_t)b * N_max;
    const int32_t* cd = cand + (int64_t)b * k;
    const float* p = pred + (int64_t)b * 16;
    for (int c = tid; c < k; c += 256) {
        const int32_t r = candidate_row(row, cd, c, N_max, R);
        const float d = r == NO_VIEW ? INFINITY : (float)pose_distance(p, bank_poses + (int64_t)r * 16);
        tab[c] = r;
        val[c] = d;
        dist[(int64_t)b * k + c] = d;
    }
    __syncthreads();
    for (int c = tid; c < k; c += 256) {
        int rank = 0;
        const float v = val[c];
        for (int m = 0; m < k; ++m) rank += tab[m] != NO_VIEW && ranks_before(val[m], m, v, c);
        chosen[c] = tab[c] != NO_VIEW && rank < fk;
    }
    __syncthreads();
    // output j is the j-th chosen position in ascending order: each output finds its own (no two threads write one word)
    int32_t* out_pos = fine_pos + (int64_t)b * fk;
    int32_t* out_src = src + (int64_t)b * (fk + 1);
    for (int j = tid; j < fk; j += 256) {
        int seen = 0, at = -1;
        for (int c = 0; c < k && at < 0; ++c) {
            if (chosen[c]) { if (seen == j) at = c; ++seen; }
        }
        out_pos[j] = at;
        out_src[j] = at >= 0 ? tab[at] : NO_VIEW;
    }
    if (tid == 0) out_src[fk] = -(b + 1);
}

}  // namespace

extern "C" int bd_round_sources(const int32_t* rows, const int32_t* cand, int R, int B, int N_max, int k, int sub, int zero_row,
                                int per_round_query, int32_t* src, int32_t* view, void* stream) {
    if (!rows || !cand || !src || !view) return BD_ERR_NULL;
    if (B <= 0 || R < 0 || N_max <= 0 || k <= 0 || k > MAXK || sub <= 0) return BD_ERR_SHAPE;
    if (k % sub != 0 && (zero_row < 0 || zero_row >= R)) return BD_ERR_SHAPE;       // a padded last round needs the bank's zero view
    const int64_t n = (int64_t)B * ((k + sub - 1) / sub) * ((int64_t)sub + 1);
    if (n > 0x7fffffff) return BD_ERR_SHAPE;
    hipLaunchKernelGGL(round_sources_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, rows, cand, R, N_max, k, sub, (int32_t)zero_row,
                       per_round_query, src, view);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_pose_select_rows(const float* bank_poses, int R, const float* pred, const int32_t* rows, const int32_t* cand, int B,
                                   int N_max, int k, int fk, float* dist, int32_t* fine_pos, int32_t* src, void* stream) {
    if (!bank_poses || !pred || !rows || !cand || !dist || !fine_pos || !src) return BD_ERR_NULL;
    if (B <= 0 || R < 0 || N_max <= 0 || k <= 0 || k > MAXK || fk <= 0 || fk > k) return BD_ERR_SHAPE;
    hipLaunchKernelGGL(pose_select_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, bank_poses, R, pred, rows, cand, N_max, k, fk,
                       dist, fine_pos, src);
    BD_CHECK_LAUNCH();
    return BD_OK;
}
