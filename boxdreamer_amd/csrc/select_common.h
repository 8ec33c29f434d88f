// Reference selection over a bank, written once: the arithmetic and the block-level steps that bd_match_select_rows (match.hip),
// bd_pose_select_rows (rounds.hip) and bd_stream_select_rows (stream.hip) share, so that a pair's score, a pose distance and a
// ranking have the same bits whichever entry produced them.  Every block-level step here is called by a whole workgroup of 256
// threads (4 waves) with block-uniform arguments; the caller places the barriers the comments name.
#pragma once
#include "bd_common.h"

namespace {

constexpr int SEL_MAXN = 1024;           // slots / candidates one workgroup ranks (its LDS tables)
constexpr int32_t NO_VIEW = 0x7fffffff;  // a `src` entry bd_gather_view_rows / bd_assemble_entry_tokens skip (outside every bank): its view keeps its bytes

// ---- appearance rule (the DINO filter): score of a pair, top-k by rounds
// The score of one (query, reference) pair from the two views' summaries, by ONE wave; every kernel that scores a pair calls these two,
// so a pair's score has the same bits whichever entry produced it (bd_dino_match_scores, bd_match_select_rows, bd_stream_select_rows).
__device__ __forceinline__ float pair_dot(const float* __restrict__ sq, const float* __restrict__ sr, int D, int lane) {
    float dot = 0.f;
    for (int d = lane; d < D; d += 64) dot = fmaf(sq[d], sr[d], dot);
    return wave_sum(dot);
}

__device__ __forceinline__ float pair_score(float dot, float cq, float cr, int L) {
    const float ll = (float)L * (float)L;
    const float pairs = cq * cr;
    // a view without foreground: the reference fills EVERY pair with -1e4, so non-finite features of the other view (NaN * 0
    // in the dot product) do not reach the score
    if (pairs == 0.f) dot = 0.f;
    const float invalid = ll - pairs;
    float m = (dot - 1e4f * invalid) / ll;
    if (!(m == m) || fabsf(m) == INFINITY) m = 0.f;            // nan_to_num(0, 0, 0)
    return m;
}

// The scores of one sample's slots against its query, one wave per slot: val[i] (LDS) and scores[i] for i < N_max.  A slot past N or a
// row outside [0, R) scores -inf, and `row` is not read past N.  A barrier follows before val is read.
__device__ __forceinline__ void score_slots(const float* __restrict__ bank_sums, const float* __restrict__ bank_counts, int R,
                                            const float* __restrict__ sq, float cq, const int32_t* __restrict__ row, int N, int N_max,
                                            int L, int D, float* val, float* __restrict__ scores) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int i = wid; i < N_max; i += 4) {
        float m = -INFINITY;
        const int r = i < N ? row[i] : -1;                  // (wave-uniform)
        if (r >= 0 && r < R) m = pair_score(pair_dot(sq, bank_sums + (int64_t)r * D, D, lane), cq, bank_counts[r], L);
        if (lane == 0) { val[i] = m; scores[i] = m; }
    }
}

// One top-k round over val[0 .. N): the best entry (largest value, then lowest index) strictly AFTER the previous pick (pv, pi) in
// that order, so a picked entry is excluded by its place, not by its value: -inf scores are ordinary values.  NaN is not ordered and
// never picked.  Every thread returns the same (bv, bi); bi == 0x7fffffff: nothing is left.  Holds one barrier; the caller places one
// more before the next round (wv / wi are rewritten there).
__device__ __forceinline__ void topk_round(const float* val, int N, float pv, int pi, float* wv, int* wi, float& bv, int& bi) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    bv = -INFINITY; bi = 0x7fffffff;
    for (int i = tid; i < N; i += 256) {
        const float v = val[i];
        const bool after = v < pv || (v == pv && i > pi);
        if (after && (v > bv || (v == bv && i < bi))) { bv = v; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o); const int oi = __shfl_xor(bi, o);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { wv[wid] = bv; wi[wid] = bi; }
    __syncthreads();
    bv = wv[0]; bi = wi[0];
    for (int w = 1; w < 4; ++w) if (wv[w] > bv || (wv[w] == bv && wi[w] < bi)) { bv = wv[w]; bi = wi[w]; }
}

// k rounds over the slots [0, N) -> pick[0 .. n_picked) (LDS), the picked slots in rank order; returns n_picked (block-uniform),
// below k when fewer than k slots exist.  Ends with a barrier: pick is readable.
__device__ __forceinline__ int topk_picks(const float* val, int N, int k, int* pick, float* wv, int* wi) {
    float pv = INFINITY;
    int pi = -1, n_picked = 0;
    for (int round = 0; round < k; ++round) {
        float bv; int bi;
        topk_round(val, N, pv, pi, wv, wi, bv, bi);
        if (bi >= N) break;                                 // (block-uniform) fewer than k slots: nothing is left to pick
        if (threadIdx.x == 0) pick[round] = bi;
        n_picked = round + 1;
        pv = bv; pi = bi;
        __syncthreads();                    // wv / wi are rewritten in the next round
    }
    __syncthreads();
    return n_picked;
}

// The picks in ascending slot order -> out_sel[0 .. k), their bank rows -> out_src[0 .. k) and -(b + 1), fresh view b, -> out_src[k].
// The picks are distinct slots: a pick's place in ascending order is the number of smaller picks.  Entries past n_picked are -1 /
// NO_VIEW, as is the src entry of a picked slot whose row is outside the bank.
__device__ __forceinline__ void compact_picks(const int* pick, int n_picked, int k, const int32_t* __restrict__ row, int R, int b,
                                              int32_t* __restrict__ out_sel, int32_t* __restrict__ out_src) {
    const int tid = threadIdx.x;
    for (int j = tid; j < k; j += 256) {
        if (j < n_picked) {
            const int p = pick[j];
            int rank = 0;
            for (int m = 0; m < n_picked; ++m) rank += pick[m] < p;
            const int r = row[p];
            out_sel[rank] = p;
            out_src[rank] = r >= 0 && r < R ? r : NO_VIEW;
        } else {
            out_sel[j] = -1;
            out_src[j] = NO_VIEW;
        }
    }
    if (tid == 0) out_src[k] = -(b + 1);
}

// ---- pose rule (the fine level): distance to a pose, rank by counting
// The bank row of slot `slot` of one sample: row[slot], NO_VIEW when the slot or the row is out of range (`row` is not read then).
__device__ __forceinline__ int32_t slot_row(const int32_t* __restrict__ row, int slot, int N_max, int R) {
    if (slot < 0 || slot >= N_max) return NO_VIEW;
    const int r = row[slot];
    return r >= 0 && r < R ? r : NO_VIEW;
}

// The bank row of candidate position c of one sample: rows[cand[c]], NO_VIEW when the slot or the row is out of range.
__device__ __forceinline__ int32_t candidate_row(const int32_t* __restrict__ row, const int32_t* __restrict__ cand, int c, int N_max, int R) {
    return slot_row(row, cand[c], N_max, R);
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

// The stored distance of a candidate whose bank row is r: +inf for NO_VIEW, else pose_distance rounded ONCE to fp32.
__device__ __forceinline__ float candidate_distance(const float* __restrict__ p, const float* __restrict__ bank_poses, int32_t r) {
    return r == NO_VIEW ? INFINITY : (float)pose_distance(p, bank_poses + (int64_t)r * 16);
}

// chosen[c] for c < k: candidate c is valid and fewer than fk valid candidates rank before it.  A candidate's rank is the number of
// valid candidates that rank before it: k reads of the LDS table per candidate (every lane reads the same word: a broadcast), no
// reduction and no barrier inside a loop; at k = 1024 that is 4096 compares per thread, at the k of a real database (20 .. 64) a few
// dozen.  val / tab (LDS) are complete before the call (a barrier), a barrier follows before chosen is read.
__device__ __forceinline__ void choose_nearest(const float* val, const int32_t* tab, int k, int fk, unsigned char* chosen) {
    for (int c = threadIdx.x; c < k; c += 256) {
        int rank = 0;
        const float v = val[c];
        for (int m = 0; m < k; ++m) rank += tab[m] != NO_VIEW && ranks_before(val[m], m, v, c);
        chosen[c] = tab[c] != NO_VIEW && rank < fk;
    }
}

// Output j is the j-th chosen position in ascending order: each output finds its own (no two threads write one word).  out_pos
// [0 .. fk): the positions, -1 where fewer than fk were chosen; out_src: their bank rows (NO_VIEW there), then -(b + 1).
__device__ __forceinline__ void compact_chosen(const unsigned char* chosen, const int32_t* tab, int k, int fk, int b,
                                               int32_t* __restrict__ out_pos, int32_t* __restrict__ out_src) {
    const int tid = threadIdx.x;
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
