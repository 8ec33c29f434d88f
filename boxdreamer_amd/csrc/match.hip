// Dense-reference mode: DINO-feature reference selection.
//
// The reference (src/models/utils/matching.py:64-174) scores every (query, reference) pair with the mean over all
// L x L patch pairs of the cosine similarity of the foreground patches, pairs without two foreground patches counting
// -1e4 (its later "== -1e9" filter never fires).  That mean needs no L x L product:
//
//     mean = ( s_q . s_r  -  1e4 * (L^2 - c_q c_r) ) / L^2
//     s_v  = sum over foreground patches of f_v[l] / max(|f_v[l]|, 1e-12),   c_v = number of foreground patches
//
// so the work is ONE pass over the encoder's patch features per view (HBM-bound: L*D*4 bytes per view, read twice, the
// second time from L2) plus a dot product per pair, instead of B*N bmm's of (L x D) x (D x L).
// Foreground = luminance(0.299 R + 0.587 G + 0.114 B) > threshold at the nearest-resized pixel of the patch grid
// (F.interpolate(mode="nearest"): source index floor(i * H / g)).
#include "select_common.h"

namespace {

constexpr int MAXL = SEL_MAXN;
constexpr float BACKGROUND = -1.0f;      // inv[] entry of a background patch (a foreground patch's inverse norm lies in [0, 1e12])

// Every product and sum rounded on its own, as the reference's fp32 tensor expression rounds them.  Contracted into v_fmac_f32
// (hipcc's default; __fmul_rn / __fadd_rn do not stop it) the luminance of a pixel near the threshold lands on the other side of it,
// and one flipped patch moves a score by 1e4 * c_other / L^2.
__device__ __forceinline__ float luminance(float r, float g, float b) {
#pragma clang fp contract(off)
    return 0.299f * r + 0.587f * g + 0.114f * b;
}

// one workgroup (4 waves) per view
__global__ __launch_bounds__(256) void match_sums_kernel(const float* __restrict__ feats, const void* __restrict__ images,
                                                          int img_dtype, int L, int D, int H, int W, float thr,
                                                          float* __restrict__ sums, float* __restrict__ counts) {
    __shared__ float inv[MAXL];
    __shared__ int cnt;
    const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid == 0) cnt = 0;
    __syncthreads();
    const float* f = feats + (int64_t)v * L * D;
    int g = 1;
    while ((g + 1) * (g + 1) <= L) ++g;                 // patch grid side
    const size_t plane = (size_t)H * W;
    for (int l = wid; l < L; l += 4) {
        float ss = 0.f;
        for (int d = lane; d < D; d += 64) { const float x = f[(int64_t)l * D + d]; ss += x * x; }
        ss = wave_sum(ss);
        if (lane == 0) {
            const int py = (int)floorf((float)(l / g) * ((float)H / (float)g)), px = (int)floorf((float)(l % g) * ((float)W / (float)g));
            const size_t o = (size_t)v * 3 * plane + (size_t)(py < H ? py : H - 1) * W + (px < W ? px : W - 1);
            const float lum = luminance(load_any(images, o, img_dtype), load_any(images, o + plane, img_dtype),
                                        load_any(images, o + 2 * plane, img_dtype));
            const bool fg = lum > thr;
            inv[l] = fg ? 1.0f / fmaxf(sqrtf(ss), 1e-12f) : BACKGROUND;
            if (fg) atomicAdd(&cnt, 1);
        }
    }
    __syncthreads();
    for (int d = tid; d < D; d += 256) {
        float s = 0.f;
        for (int l = 0; l < L; ++l) {
            // a background patch contributes 0 whatever it holds: the reference fills its pairs with -1e4, and NaN * 0 / Inf * 0 would
            // turn the view's scores into 0.  A select, not a branch (a branch here costs the loop its unrolled loads: +50 % time);
            // finite features give the same sum as x * 0 + s.
            const float w = inv[l];
            const float x = f[(int64_t)l * D + d];
            s = fmaf(w == BACKGROUND ? 0.f : x, w, s);
        }
        sums[(int64_t)v * D + d] = s;
    }
    if (tid == 0) counts[v] = (float)cnt;
}

// one wave per (sample, reference): references are the views != query_view[b], in view order
__global__ __launch_bounds__(64) void match_scores_kernel(const float* __restrict__ sums, const float* __restrict__ counts,
                                                           const int32_t* __restrict__ query_view, int T, int L, int D,
                                                           float* __restrict__ scores) {
    const int b = blockIdx.x / (T - 1), n = blockIdx.x % (T - 1), lane = threadIdx.x;
    const int q = query_view[b];
    const int r = n < q ? n : n + 1;
    const float dot = pair_dot(sums + ((int64_t)b * T + q) * D, sums + ((int64_t)b * T + r) * D, D, lane);
    if (lane == 0) scores[b * (T - 1) + n] = pair_score(dot, counts[b * T + q], counts[b * T + r], L);
}

// top-k mask per row (N <= 1024): k rounds of (largest value, then lowest index), one workgroup per row.  A round picks the best
// entry strictly AFTER the previous pick (pv, pi) in that order, so a picked entry is excluded by its place, not by its value:
// -inf scores are ordinary values here (a row with fewer than k finite scores takes its lowest-index -inf entries next).
// NaN scores are not ordered and never picked; the product path removes them (match_scores_kernel: nan_to_num).
__global__ __launch_bounds__(256) void topk_mask_kernel(const float* __restrict__ scores, int N, int k,
                                                         unsigned char* __restrict__ mask) {
    __shared__ float val[MAXL];
    __shared__ float wv[4];
    __shared__ int wi[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < N; i += 256) { val[i] = scores[(int64_t)b * N + i]; mask[(int64_t)b * N + i] = 0; }
    __syncthreads();
    float pv = INFINITY;
    int pi = -1;
    for (int round = 0; round < k; ++round) {
        float bv; int bi;
        topk_round(val, N, pv, pi, wv, wi, bv, bi);
        if (tid == 0 && bi < N) mask[(int64_t)b * N + bi] = 1;
        pv = bv; pi = bi;
        __syncthreads();                    // wv / wi are rewritten in the next round
    }
}

// Dense-reference mode over a bank of view summaries: score, select and compact in ONE launch, one workgroup (4 waves) per sample.
// Sample b's references are the bank rows rows[b][0 .. n_refs[b]); its query is fresh view b (q_sums / q_counts).
//   score    one wave per slot, match_scores_kernel's arithmetic (pair_dot, pair_score); a slot past n_refs[b] or a row outside
//            [0, R) scores -inf, and `rows` is not read past n_refs[b]
//   top-k    topk_mask_kernel's rounds over the slots [0, n_refs[b])
//   compact  the picked slots in ascending order -> sel[b], their bank rows followed by -(b + 1) (fresh view b) -> src
// Inconsistent device data cannot read or write out of bounds: n_refs[b] is clamped into [0, N_max]; when it is below k the
// remaining entries of sel[b] are -1 and those of src NO_VIEW, as is the src entry of a picked slot whose row is outside the bank.
__global__ __launch_bounds__(256) void match_select_rows_kernel(const float* __restrict__ bank_sums, const float* __restrict__ bank_counts,
                                                                 int R, const float* __restrict__ q_sums, const float* __restrict__ q_counts,
                                                                 const int32_t* __restrict__ rows, const int32_t* __restrict__ n_refs,
                                                                 int N_max, int L, int D, int k, float* __restrict__ scores,
                                                                 int32_t* __restrict__ sel, int32_t* __restrict__ src) {
    __shared__ float val[MAXL];
    __shared__ int pick[MAXL];
    __shared__ float wv[4];
    __shared__ int wi[4];
    const int b = blockIdx.x;
    int N = n_refs[b];
    N = N < 0 ? 0 : (N > N_max ? N_max : N);
    const int32_t* row = rows + (int64_t)b * N_max;
    score_slots(bank_sums, bank_counts, R, q_sums + (int64_t)b * D, q_counts[b], row, N, N_max, L, D, val, scores + (int64_t)b * N_max);
    __syncthreads();
    const int n_picked = topk_picks(val, N, k, pick, wv, wi);
    compact_picks(pick, n_picked, k, row, R, b, sel + (int64_t)b * k, src + (int64_t)b * (k + 1));
}

}  // namespace

extern "C" int bd_dino_match_scores(const float* feats, const void* images, int img_dtype, const int32_t* query_view, int B,
                                    int T, int L, int D, int H, int W, float lum_threshold, float* sums, float* counts,
                                    float* scores, void* stream) {
    if (!feats || !images || !query_view || !sums || !counts || !scores) return BD_ERR_NULL;
    if (B <= 0 || T < 2 || L <= 0 || L > MAXL || D <= 0 || H <= 0 || W <= 0) return BD_ERR_SHAPE;
    if (img_dtype != BD_DTYPE_F32 && img_dtype != BD_DTYPE_BF16 && img_dtype != BD_DTYPE_F16) return BD_ERR_DTYPE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(match_sums_kernel, dim3(B * T), dim3(256), 0, s, feats, images, img_dtype, L, D, H, W, lum_threshold,
                       sums, counts);
    hipLaunchKernelGGL(match_scores_kernel, dim3(B * (T - 1)), dim3(64), 0, s, sums, counts, query_view, T, L, D, scores);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_topk_mask(const float* scores, int B, int N, int k, unsigned char* mask, void* stream) {
    if (!scores || !mask) return BD_ERR_NULL;
    if (B <= 0 || N <= 0 || N > MAXL || k <= 0 || k > N) return BD_ERR_SHAPE;
    hipLaunchKernelGGL(topk_mask_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, scores, N, k, mask);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_match_view_sums(const float* feats, const void* images, int img_dtype, int V, int L, int D, int H, int W,
                                  float lum_threshold, float* sums, float* counts, void* stream) {
    if (!feats || !images || !sums || !counts) return BD_ERR_NULL;
    if (V < 0 || L <= 0 || L > MAXL || D <= 0 || H <= 0 || W <= 0) return BD_ERR_SHAPE;
    if (img_dtype != BD_DTYPE_F32 && img_dtype != BD_DTYPE_BF16 && img_dtype != BD_DTYPE_F16) return BD_ERR_DTYPE;
    if (V == 0) return BD_OK;
    hipLaunchKernelGGL(match_sums_kernel, dim3(V), dim3(256), 0, (hipStream_t)stream, feats, images, img_dtype, L, D, H, W,
                       lum_threshold, sums, counts);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_match_select_rows(const float* bank_sums, const float* bank_counts, int R, const float* q_sums, const float* q_counts,
                                    const int32_t* rows, const int32_t* n_refs, int B, int N_max, int L, int D, int k,
                                    float* scores, int32_t* sel, int32_t* src, void* stream) {
    if (!bank_sums || !bank_counts || !q_sums || !q_counts || !rows || !n_refs || !scores || !sel || !src) return BD_ERR_NULL;
    if (B <= 0 || R < 0 || N_max <= 0 || N_max > MAXL || k <= 0 || k > N_max || L <= 0 || D <= 0) return BD_ERR_SHAPE;
    hipLaunchKernelGGL(match_select_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, bank_sums, bank_counts, R, q_sums,
                       q_counts, rows, n_refs, N_max, L, D, k, scores, sel, src);
    BD_CHECK_LAUNCH();
    return BD_OK;
}
