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
#include "select_common.h"

namespace {

constexpr int MAXK = SEL_MAXN;

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

// one workgroup (4 waves) per sample: distances, rank by counting, compaction (select_common.h: candidate_distance, choose_nearest,
// compact_chosen)
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
        const float d = candidate_distance(p, bank_poses, r);
        tab[c] = r;
        val[c] = d;
        dist[(int64_t)b * k + c] = d;
    }
    __syncthreads();
    choose_nearest(val, tab, k, fk, chosen);
    __syncthreads();
    compact_chosen(chosen, tab, k, fk, b, fine_pos + (int64_t)b * fk, src + (int64_t)b * (fk + 1));
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
