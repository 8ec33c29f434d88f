// Fused multi-head self-attention  softmax(scale * Q K^T) V  on packed qkv, gfx950.
//
// Replaces flash_attn_func / F.scaled_dot_product_attention (BETR, head_dim 96, seq T*256) and
// xformers memory_efficient_attention / the naive softmax path (DINOv2, head_dim 64, seq 261).
//
// Layout trick (all three MFMAs keep "query = lane & 31"):
//   S^T = K . Q^T      A = K tile rows from LDS (key = lane&31, 8 d per lane), B = Q^T from registers.
//                      Lane (q, h) ends up holding scores of ITS query for 16 keys per 32-key tile:
//                      key = (r&3) + 8*(r>>2) + 4*h.  Row max / sum are therefore in-lane reductions
//                      plus ONE exchange with lane^32.
//   O^T = V^T . P^T    B = P^T: the lane's own probabilities, regs 8t..8t+7, used directly as the 8
//                      k-slots of 16-key group t -- no cross-lane movement at all, because the V^T
//                      image in LDS is written with the same key permutation (quads 1 and 2 of every
//                      16-key group swapped).  A = V^T rows (d = lane&31) read with one ds_read_b128.
//                      The O^T accumulator again has query = lane&31, so the online-softmax rescale
//                      and the final 1/l are per-lane scalars.
// K tile rows are padded by 16 B and the V^T image is XOR-swizzled so that each ds_read_b128 lane
// group hits 16 distinct bank slots.  K/V tiles of 64 keys are register-prefetched one tile ahead.
// The split-bf16 hd-64 instances stage differently (DMA below): K and V tiles go row-major into LDS by LDS-DMA, with no
// staging registers, and the V^T fragments come from the transposing read ds_read_b64_tr_b16.
// NS = 2 is the split-bf16 strict mode: Q, K, V, P each carry (hi, lo) and every product issues
// hi*hi + hi*lo + lo*hi.
#include "bd_common.h"
#include <algorithm>
#include <type_traits>

#ifdef BD_ATTN_PROBE
// Measurement build only (tools/attn_phase_probe.py): per-wave shader-clock stamps of the ping-pong kernel's segments.
__device__ unsigned* bd_attn_probe_buf = nullptr;
extern "C" int bd_attn_probe_set(void* buf) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(bd_attn_probe_buf), &buf, sizeof(buf)); }
#define AP(idx) { const unsigned long long t__ = __builtin_amdgcn_s_memtime(); if ((idx) < 64) probe_ts = (lane == (idx)) ? (unsigned)t__ : probe_ts; }
#else
#define AP(idx) {}
#endif

namespace {

struct AttnArgs {
    const void* qkv; int64_t qkv_plane;
    void* out; int64_t out_plane;
    int batch, seq, heads;
    float scale_log2e;
    const int32_t* q_view;   // optional: queries are rows [q_view[b]*q_len, +q_len) of every sequence, output compact
    int q_len;               // number of query rows per sequence (== seq when q_view is NULL)
    int q_off;               // (q_view == NULL) first query row inside every sequence: queries are rows [q_off, q_off + q_len)
    int out_rows;            // rows per sample in `out` (q_len: compact; seq with q_off: the result lands in rows [q_off, q_off + q_len))
    // Ragged batches (bd_attention_varlen, the VL kernel instances): sample b owns the views [view_start[b], view_start[b + 1]) of `tpv` token
    // rows each, packed back to back; `seq`, the sample's base row and (without q_view) `q_len` then come from the offsets, per sample.
    const int32_t* view_start;   // device int32 [batch + 1], or NULL (uniform batch: every sample has `seq` rows)
    int tpv, n_views, max_views; // token rows per view; host-known total (sizes the grid) and largest per-sample view count (bounds the descriptor)
};

// (VL) which sample owns work item `wg` when sample i owns the items [view_start[i] * ipv, view_start[i + 1] * ipv): the number of interior
// offsets at or below wg -- the offsets ascend, so one ballot per 64 samples counts them (zero-view samples own nothing and are skipped).
__device__ __forceinline__ int vl_sample_of(const int32_t* view_start, int batch, int ipv, int wg, int lane) {
    int b = 0;
    for (int i0 = 0; i0 < batch; i0 += 64) {
        const int i = i0 + lane;
        const bool below = i < batch && (int64_t)view_start[i + 1] * ipv <= (int64_t)wg;
        b += __popcll(__ballot(below));
    }
    return __builtin_amdgcn_readfirstlane(b);
}

constexpr int KT = 64;   // keys per tile

// 16-byte chunk swizzle of V^T row d (128-byte rows: every row aliases the same 32 banks).
//  * ds_read_b128 (O^T A operand): a 16-lane group reads 16 consecutive rows, same logical chunk -> the 8 rows of
//    equal parity must land on 8 distinct chunks: (d >> 1) & 7 does that, and XOR-ing in (d >> 4), constant over an
//    aligned 16-row group, keeps it a bijection;
//  * ds_write_b64 (transposing stage): the lanes of a group hold d = 8*dc + const for 12 consecutive dc -> with
//    (d >> 1) alone only 2 of 8 chunks are used (6-way conflict: 43 % of LDS cycles in profiles/r1_attn_pmc.md);
//    the (d >> 4) term spreads them over all 8 (<= 2-way).
__device__ __forceinline__ int vswz(int d) { return ((d >> 1) ^ (d >> 4)) & 7; }

// low / high 16-bit halves of two dwords as one dword (the 4 x 4 register transposition of the V staging): one v_perm_b32 each
// (written as and / shift / or hipcc emits two VALU instructions per pair: 32 instead of 16 per staged micro-tile)
__device__ __forceinline__ unsigned pack_lo16(unsigned a, unsigned b) { return __builtin_amdgcn_perm(b, a, 0x05040100u); }   // (a & 0xffff) | (b << 16)
__device__ __forceinline__ unsigned pack_hi16(unsigned a, unsigned b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }   // (a >> 16) | (b & 0xffff0000)

// LDS-DMA and the transposing LDS read, as device functions: the kernel template is also instantiated for the host, which has
// neither builtin.
typedef __attribute__((__vector_size__(4 * sizeof(short)))) short s16x4;
// 16 bytes per lane, global -> LDS with no register in between: lane l's piece lands at lds_dst + 16 l (lds_dst wave-uniform); a lane
// whose voff is out of the descriptor's range fetches nothing.
// The BUILTIN, where the GEMMs issue their DMA from inline asm (gemm_common.h: glds16): there a slab's DMA flies under the MFMAs of
// the one before, and hipcc, which sees an LDS write it cannot place, would drain it with vmcnt(0) in front of the first fragment
// read.  Here nothing is in flight while fragments are read -- the tile is issued after the barrier that ends the reads and waited
// for in full before the next one -- so that conservative wait is the wait this kernel wants, and the key loop keeps its counted
// lgkmcnt waits (checked in the ISA: lgkmcnt(6 / 4 / 2) over the K fragments).
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t rsrc, unsigned char* lds_dst, int voff, int soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds_dst, 16, voff, soff, 0, 0);
}
// ds_read_b64_tr_b16: lane 4 q + p of a 16-lane group addresses row q, 16-bit columns 4 p .. 4 p + 3 of a 4 x 16 block; lane i of the
// group gets column i, row q in element q.  EXEC must be all ones.
__device__ __forceinline__ s16x4 lds_read_tr16(const unsigned char* a) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a);
}

// OUTSPLIT: single-pass f16 attention whose result is written as split-bf16 (hi, lo) planes -- the strict mode's
// attention (its GEMMs stay split-bf16 x3): q/k are RMS-normalised and P is in [0, 1], so one f16 pass costs ~1e-4 on
// the logits while the x3 attention kernel is register-bound at one wave per SIMD.
template <class T, int NS, int HD, int NW, int OUTMODE = 0, bool VL = false>
__global__ __launch_bounds__(NW * 64, HD == 64 ? 3 : 2) void attn_kernel(const AttnArgs p) {      // (HIP: 2nd argument = min waves per SIMD)
    bd_saturating_conversions();      // fp8 / f16 results saturate (bd_common.h: RANGE)
    typedef typename Op16<T>::vec8 vec8;
    // DMA: the split-bf16 hd-64 instances (DINOv2's strict attention).  With K / V register-prefetched they need 211 VGPRs = two waves per
    // SIMD, 56 of them the next tile in flight.  Here both tiles go global -> LDS by LDS-DMA (no staging registers, no ds_write pass, no
    // register transposition of V), which fits three waves per SIMD = four 3-wave workgroups per CU: the latency of a tile's loads is
    // hidden by the other workgroups, not by a prefetch.  LDS images (128-byte rows, one row per key, 16-byte chunks XOR-swizzled on the
    // GLOBAL side, because an LDS-DMA piece lands lane-linear: 1 KiB = 8 rows):
    //   K: chunk c of row r at chunk c ^ ((r >> 1) & 7) -- the 16 rows of a ds_read_b128 lane group are 8 pairs (2 j, 2 j + 1) with
    //      distinct (j & 7), and a pair shares one 256-byte bank row: 16 distinct bank slots (profiles/attn_dino_lds_dma.md);
    //   V: chunk c of row r at chunk c ^ ((r & 2) << 1) -- a 32-lane half of ds_read_b64_tr_b16 reads 64 bytes of each of 4 consecutive
    //      rows; rows r and r + 2 share the bank-row half, and the swizzle sends them to opposite 64-byte quarters of it.
    constexpr bool DMA = NS == 2 && HD == 64;
    constexpr int NT = NW * 64;
    constexpr int DCH = HD / 8;                  // 16-byte chunks per K/V row
    constexpr int KSTRIDE = DMA ? HD * 2 : HD * 2 + 16;      // K row (bytes): padded where it is written by ds_write
    constexpr int K_BYTES = KT * KSTRIDE;
    constexpr int V_BYTES = HD * 128;            // V^T image: HD rows x 64 keys x 2 B
    constexpr int PLANE_BYTES = K_BYTES + V_BYTES;
    constexpr int KCH = KT * DCH;                // K chunks per tile
    constexpr int KCPT = (KCH + NT - 1) / NT;
    constexpr int VMT = (KT / 4) * DCH;          // V micro-tiles (4 keys x 8 d)
    static_assert(VMT <= NT, "one V micro-tile per thread");
    constexpr int QB = NW * 32;
    constexpr int DM = HD / 32;                  // O^T M-tiles
    constexpr int KS = HD / 16;                  // k-steps of S^T
    constexpr int BUF_BYTES = NS * PLANE_BYTES;
    constexpr int NBUF = NS == 1 ? 2 : 1;      // strict mode keeps one buffer (two planes already fill the LDS budget)
    __shared__ __attribute__((aligned(16))) unsigned char lds[NBUF * BUF_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
#ifdef BD_ATTN_PROBE
    unsigned probe_ts = 0;
    AP(60)
#endif
    const int lq = lane & 31, lh = lane >> 5;
    int seq = p.seq;
    const int heads = p.heads;
    int q_len = p.q_len;
    int nqb = (q_len + QB - 1) / QB;

    // XCD-aware remap: consecutive work items (same batch*head, consecutive q-blocks) share K/V and
    // are kept on one XCD's L2.
    int wg;
    {
        const int nwg = gridDim.x, bid = blockIdx.x, xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    int qb = wg % nqb;
    int bh = wg / nqb;
    int head = bh % heads, b = bh / heads;
    int64_t row0 = (int64_t)b * seq;                       // the sample's first token row
    int vl_views = 0;
    if constexpr (VL) {
        // the work list is implicit: (sample, head, q-block) in that order, every sample with its own number of q-blocks (whole ones:
        // tpv % QB == 0).  Offsets are device data: anything inconsistent with the host's n_views / max_views ends the workgroup.
        if (!p.q_view) {
            const int ipv = (p.tpv / QB) * heads;          // work items per view
            b = vl_sample_of(p.view_start, p.batch, ipv, wg, lane);
            if (b >= p.batch) return;
        }
        const int s0 = __builtin_amdgcn_readfirstlane(p.view_start[b]), s1 = __builtin_amdgcn_readfirstlane(p.view_start[b + 1]);
        vl_views = s1 - s0;
        if (s0 < 0 || vl_views <= 0 || vl_views > p.max_views || s1 > p.n_views) return;
        seq = vl_views * p.tpv;
        row0 = (int64_t)s0 * p.tpv;
        if (!p.q_view) {
            q_len = seq;
            nqb = vl_views * (p.tpv / QB);
            const int local = wg - s0 * (p.tpv / QB) * heads;
            qb = local % nqb;
            head = local / nqb;
        }
    }

    const int ld = 3 * heads * HD;                         // elements per token row (32-bit offsets inside a sample)
    const T* base = (const T*)p.qkv + row0 * ld + head * HD;
    const T* qbase = base;
    const T* kbase = base + heads * HD;
    const T* vbase = base + 2 * heads * HD;
    const int64_t plane = p.qkv_plane;

    // ---- Q fragments (B operand of S^T): lane (q, h) holds Q[q][ks*16 + h*8 .. +7]
    const int q0 = qb * QB + (NS == 2 && HD == 64 ? __builtin_amdgcn_readfirstlane(wid) : wid) * 32;      // local query index (within the query range)
    int qbase_row = p.q_view ? p.q_view[b] * q_len : p.q_off;
    if constexpr (VL) { if (p.q_view) { const int qv = p.q_view[b]; qbase_row = (qv < 0 ? 0 : (qv < vl_views ? qv : vl_views - 1)) * q_len; } }
    int qrow = q0 + lq; qrow = (qrow < q_len ? qrow : q_len - 1) + qbase_row;
    // first row of this sample in `out`: its packed rows (ragged, every row a query), else its out_rows-row slot
    auto out_row0 = [&]() -> int64_t {
        if constexpr (VL) { if (!p.q_view) return row0; }
        return (int64_t)b * p.out_rows + (p.out_rows == q_len ? 0 : p.q_off);
    };
    vec8 qf[NS][KS];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            qf[s][ks] = as_vec8<T>(*(const u128*)(qbase + s * plane + (unsigned)(qrow * ld + ks * 16 + lh * 8)));

    // ---- loader coordinates
    int kc_row[KCPT], kc_col[KCPT];
    unsigned kc_off[KCPT];                                  // element offset of the chunk in tile 0
#pragma unroll
    for (int i = 0; i < KCPT; ++i) {
        const int c = tid + NT * i;
        kc_row[i] = c / DCH;
        kc_col[i] = c % DCH;
        kc_off[i] = (unsigned)(kc_row[i] * ld + kc_col[i] * 8);
    }
    const int vm_kq = tid / DCH, vm_dc = tid % DCH;     // key quad (0..15), d chunk
    const bool vm_active = tid < VMT;
    const unsigned vm_off = (unsigned)(vm_kq * 4 * ld + vm_dc * 8);
    const bool ragged = (seq % KT) != 0;
    // destination of the micro-tile in the V^T image: 16-key group g, permuted quad
    int vdst;
    {
        const int g = vm_kq >> 2, qi = vm_kq & 3;
        const int qp = (qi == 1) ? 2 : (qi == 2 ? 1 : qi);
        vdst = ((g * 2 + (qp >> 1)) << 4) | ((qp & 1) << 3);   // chunk<<4 | 8-byte half  (pre-swizzle)
    }

    u128 rk[NS][KCPT], rv[NS][4];
    // K / V tiles by BUFFER loads (round 5, as attn_kernel_pp): one wave-uniform descriptor per plane over this (sample, head)'s seq rows, the
    // tile / row origin in the scalar offset, loop-invariant 32-bit per-lane offsets.  Rows past a ragged sequence's end are OUT OF RANGE of the
    // descriptor and read as ZERO (hardware bounds check) -- no per-lane row clamp; their scores are masked to -inf and their P is exactly 0,
    // so every valid output keeps its bits (the clamped form read row seq - 1 there, equally without effect).
    __amdgpu_buffer_rsrc_t rsrc[NS];
    {
        const int bytes = __builtin_amdgcn_readfirstlane(seq * ld * (int)sizeof(T));
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const uintptr_t a = (uintptr_t)(base + s * plane);
            const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
            rsrc[s] = __builtin_amdgcn_make_buffer_rsrc((void*)(((uintptr_t)hi << 32) | lo), 0, bytes, 0x00020000);
        }
    }
    const int row_bytes = __builtin_amdgcn_readfirstlane(ld * (int)sizeof(T));
    // (DMA) one tile = 16 pieces of 1 KiB per plane (K then V, 8 rows each), piece i at byte i * 1024 of the plane, dealt round-robin to
    // the waves.  Lane l of a piece fills physical chunk l & 7 of the piece's row l >> 3.  That row and the swizzled chunk are the per-lane
    // offset; the piece's first row and the K / V column origin are the scalar offset.  Only pieces whose first row is a row of the
    // sample are issued, so the scalar offset stays inside the descriptor; the rows of such a piece past the sequence end are out of
    // range and their lanes fetch nothing.
    const int wid_s = __builtin_amdgcn_readfirstlane(wid);
    auto stage_dma = [&](const int kt) {
        // the per-lane offsets are re-derived here, from an opaque lane id: hoisted out of the key loop they are six registers that
        // the loop does not have (three waves per SIMD: 168)
        int ln;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
        const int dma_row = ln >> 3, dma_c = ln & 7, dma_row_off = dma_row * row_bytes;
        // even K pieces; odd ones: ^ 64 (row bit 3 -> chunk bit 2).  The XOR reaches the chunk alone because the row part of the sum is
        // a multiple of 128: row_bytes = 3 * heads * HD * sizeof(T) with HD == 64 here (the token row is the kernel's own ld, never an argument)
        static_assert(!DMA || (HD * sizeof(T)) % 128 == 0, "the ^ 64 of odd K pieces needs 128-byte-multiple token rows");
        const int dma_k_voff = dma_row_off + ((dma_c ^ (dma_row >> 1)) << 4);
        const int dma_v_voff = dma_row_off + ((dma_c ^ ((dma_row & 2) << 1)) << 4);
        const int tile_off = kt * KT * row_bytes + heads * HD * (int)sizeof(T), rows_left = seq - kt * KT;
#pragma unroll
        for (int j = 0; j < (16 + NW - 1) / NW; ++j) {
            const int i = wid_s + NW * j, pc = i & 7;      // piece of the plane: 0..7 K, 8..15 V
            if ((16 % NW == 0 || i < 16) && pc * 8 < rows_left) {
                const bool is_v = i >> 3;
                const int voff = is_v ? dma_v_voff : (pc & 1) ? (dma_k_voff ^ 64) : dma_k_voff;
                const int soff = tile_off + pc * 8 * row_bytes + (is_v ? heads * HD * (int)sizeof(T) : 0);
#pragma unroll
                for (int s = 0; s < NS; ++s)
                    lds_dma16(rsrc[s], lds + s * PLANE_BYTES + i * 1024, voff, soff);
            }
        }
        // V rows past a ragged end: their P is exactly 0, but 0 * (whatever LDS held) must be 0 too.  Whole rows, so no swizzle.
        const int valid = seq - kt * KT;
        if (valid < KT) {
            for (int c = valid * DCH + tid; c < KT * DCH; c += NT)
#pragma unroll
                for (int s = 0; s < NS; ++s) *(u128*)(lds + s * PLANE_BYTES + K_BYTES + c * 16) = (u128){0u, 0u, 0u, 0u};
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces have landed; the barrier that follows covers the others'
    };
    // (DMA) fragment addresses inside a plane.  K: row lq (+ 32 km), chunk (2 ks + lh) swizzled.  V^T by the transposing read: lane
    // 4 q + p of a 16-lane group addresses row q of a 4-key block, columns 4 p .. 4 p + 3 of the group's 16 d, and receives column
    // (lane & 15) of the 4 rows -- V[key0 + 0..3][d = 32 dm + lq], half of the A fragment of O^T.  dm flips chunk bit 2: address ^ 64.
    const int tr_q = (lane >> 2) & 3, tr_p = lane & 3;
    const unsigned kfrag_dma = (unsigned)(lq * 128 + ((lh ^ ((lq >> 1) & 7)) << 4));                      // ^ (ks << 5), + km * 4096
    const unsigned vfrag_dma = (unsigned)(K_BYTES + (4 * lh + tr_q) * 128 + (((((lane >> 4) & 1) * 2 + (tr_p >> 1)) ^ ((tr_q & 2) << 1)) << 4) + (tr_p & 1) * 8);
    int k_voff[KCPT];
#pragma unroll
    for (int i = 0; i < KCPT; ++i) k_voff[i] = ((int)kc_off[i] + heads * HD) * (int)sizeof(T);
    const int v_voff = ((int)vm_off + 2 * heads * HD) * (int)sizeof(T);
#define LOAD_TILE(kt)                                                                         \
    _Pragma("unroll") for (int s = 0; s < NS; ++s) {                                          \
        _Pragma("unroll") for (int i = 0; i < KCPT; ++i) {                                    \
            if (KCH % NT == 0 || tid + NT * i < KCH)                                          \
                rk[s][i] = __builtin_bit_cast(u128, __builtin_amdgcn_raw_buffer_load_b128(rsrc[s], k_voff[i], (kt) * KT * row_bytes, 0)); \
        }                                                                                     \
        if (vm_active) {                                                                      \
            _Pragma("unroll") for (int j = 0; j < 4; ++j)                                     \
                rv[s][j] = __builtin_bit_cast(u128, __builtin_amdgcn_raw_buffer_load_b128(rsrc[s], v_voff, ((kt) * KT + j) * row_bytes, 0)); \
        }                                                                                     \
    }
#define STORE_TILE(buf)                                                                        \
    _Pragma("unroll") for (int s = 0; s < NS; ++s) {                                          \
        unsigned char* kl = lds + (buf) * BUF_BYTES + s * PLANE_BYTES;                        \
        unsigned char* vl = kl + K_BYTES;                                                     \
        _Pragma("unroll") for (int i = 0; i < KCPT; ++i)                                      \
            if (KCH % NT == 0 || tid + NT * i < KCH)                                          \
                *(u128*)(kl + kc_row[i] * KSTRIDE + kc_col[i] * 16) = rk[s][i];               \
        if (vm_active) {                                                                      \
            _Pragma("unroll") for (int w = 0; w < 4; ++w) {                                   \
                const unsigned a0 = rv[s][0][w], a1 = rv[s][1][w], a2 = rv[s][2][w], a3 = rv[s][3][w]; \
                const int d = vm_dc * 8 + 2 * w;                                              \
                uint2 lo, hi;                                                                 \
                lo.x = pack_lo16(a0, a1); lo.y = pack_lo16(a2, a3);       \
                hi.x = pack_hi16(a0, a1); hi.y = pack_hi16(a2, a3); \
                *(uint2*)(vl + d * 128 + (vdst ^ (vswz(d) << 4))) = lo;                \
                *(uint2*)(vl + (d + 1) * 128 + (vdst ^ (vswz(d + 1) << 4))) = hi;    \
            }                                                                                 \
        }                                                                                     \
    }

    f32x16 oacc[DM];
#pragma unroll
    for (int i = 0; i < DM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const float sc = p.scale_log2e;

    const int nt = (seq + KT - 1) / KT;
    if constexpr (DMA) {
        stage_dma(0);
    } else {
        LOAD_TILE(0)
        STORE_TILE(0)
    }
    __syncthreads();
    AP(61)
    // One key tile.  Two instances: TAIL 0 = any tile (a ragged last one masks its scores), TAIL 2 = a ragged last tile of <= 16 keys
    // (DINOv2: 261 = 4 x 64 + 5), which skips the second 32-key M-tile of S^T and the three 16-key P.V groups that lie wholly past
    // the sequence -- their scores would be masked to -inf and their P exactly 0, so the result is bit-identical and the tile costs
    // 6 instead of 16 MFMAs per plane product.  The tail is PEELED: the same skip as wave-uniform branches inside one loop body
    // costs the main loop its schedule (seq 261: 121 -> 182 us), and so does skipping the staging of the tail's unused rows
    // (profiles/r3_attention_tail.md).  hd 64 only: the hd-96 split-plane instances have no registers for a second tile instance.
    const bool small_tail = HD == 64 && nt > 1 && seq % KT != 0 && seq % KT <= 16;
    auto tile = [&](const int kt, auto tail_c) {
        constexpr int TAIL = decltype(tail_c)::value;
        constexpr int KMN = TAIL == 2 ? 1 : 2, GN = TAIL == 2 ? 1 : 4;
        if constexpr (!DMA) { if (kt + 1 < nt) { LOAD_TILE(kt + 1) } }
        const unsigned char* cur = lds + (NBUF == 2 ? (kt & 1) : 0) * BUF_BYTES;
        if (kt < 7) AP(kt * 8)

        // ---- S^T = K . Q^T  (two 32-key M-tiles)
        f32x16 sacc[KMN];
#pragma unroll
        for (int km = 0; km < KMN; ++km) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[km][r] = 0.f;
            // (DMA) all eight fragments of the M-tile are requested before its first MFMA: left to itself hipcc, at the 168-register cap,
            // waits for every fragment right in front of the MFMAs that use it
            vec8 kfa[DMA ? KS : 1][NS];
            if constexpr (DMA) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                    for (int s = 0; s < NS; ++s)
                        kfa[ks][s] = as_vec8<T>(*(const u128*)(cur + s * PLANE_BYTES + km * 32 * KSTRIDE + (kfrag_dma ^ (unsigned)(ks << 5))));
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                vec8 kf[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if constexpr (DMA) kf[s] = kfa[ks][s];
                    else kf[s] = as_vec8<T>(*(const u128*)(cur + s * PLANE_BYTES + (km * 32 + lq) * KSTRIDE + (ks * 2 + lh) * 16));
                }
                if (NS == 2) {
                    sacc[km] = Op16<T>::mfma(kf[NS - 1], qf[0][ks], sacc[km]);
                    sacc[km] = Op16<T>::mfma(kf[0], qf[NS - 1][ks], sacc[km]);
                }
                sacc[km] = Op16<T>::mfma(kf[0], qf[0][ks], sacc[km]);
            }
        }
        // ---- online softmax (base-2), per query = per lane pair (l, l^32).  Scores stay raw; the softmax scale
        // (times log2 e) is folded into the exponent:  p = exp2(s*sc - m*sc)  = one FMA + v_exp_f32 per score.
        if (kt < 7) AP(kt * 8 + 1)
        float tmax = -INFINITY;
        if (TAIL == 2 || (kt + 1) * KT > seq) {
#pragma unroll
            for (int km = 0; km < KMN; ++km)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if constexpr (DMA) {
                        // the same test against ONE register: written per key, hipcc keeps the 22 key indices of the generic tile in
                        // registers across the loop
                        const int live = seq - kt * KT - 4 * lh;      // keys of this tile left for the lane's half
                        if (km * 32 + (r & 3) + 8 * (r >> 2) >= live) sacc[km][r] = -INFINITY;
                    } else {
                        const int key = kt * KT + km * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        if (key >= seq) sacc[km][r] = -INFINITY;
                    }
                }
        }
#pragma unroll
        for (int km = 0; km < KMN; ++km)
#pragma unroll
            for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, sacc[km][r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float m_new = fmaxf(m_run, tmax);                     // raw-score units (sc > 0)
        if (!__all(m_new == m_run)) {                               // some row's max moved: rescale O and l
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * sc);
            l_run *= alpha;
#pragma unroll
            for (int i = 0; i < DM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
            m_run = m_new;
        }
        const float mneg = -m_run * sc;
        float psum = 0.f;
#pragma unroll
        for (int km = 0; km < KMN; ++km)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(fmaf(sacc[km][r], sc, mneg));
                sacc[km][r] = pv;
                psum += pv;
            }
        l_run += psum;
        if (kt < 7) AP(kt * 8 + 2)

        // ---- O^T += V^T . P^T   (four 16-key groups)
#pragma unroll
        for (int g = 0; g < GN; ++g) {
            vec8 pf[NS];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float pv = sacc[g >> 1][(g & 1) * 8 + j];
                const T hi = from_f32<T>(pv);
                pf[0][j] = hi;
                if (NS == 2) pf[NS - 1][j] = from_f32<T>(pv - to_f32<T>(hi));
            }
#pragma unroll
            for (int dm = 0; dm < DM; ++dm) {
                const int d = dm * 32 + lq;
                vec8 vf[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if constexpr (DMA) {
                        const unsigned char* a = cur + s * PLANE_BYTES + g * 16 * 128 + (vfrag_dma ^ (unsigned)(dm << 6));
                        const s16x4 k03 = lds_read_tr16(a);                 // keys 16 g + 4 lh + 0..3
                        const s16x4 k8b = lds_read_tr16(a + 8 * 128);       // keys 16 g + 8 + 4 lh + 0..3
                        vf[s] = __builtin_bit_cast(vec8, __builtin_shufflevector(k03, k8b, 0, 1, 2, 3, 4, 5, 6, 7));
                    } else {
                        vf[s] = as_vec8<T>(*(const u128*)(cur + s * PLANE_BYTES + K_BYTES + d * 128 + (((g * 2 + lh) ^ vswz(d)) << 4)));
                    }
                }
                if (NS == 2) {
                    oacc[dm] = Op16<T>::mfma(vf[NS - 1], pf[0], oacc[dm]);
                    oacc[dm] = Op16<T>::mfma(vf[0], pf[NS - 1], oacc[dm]);
                }
                oacc[dm] = Op16<T>::mfma(vf[0], pf[0], oacc[dm]);
            }
        }
        // the other buffer was last read in iteration kt-1, which every wave left through the barrier below
        if (kt < 7) AP(kt * 8 + 3)
        if (NBUF == 1) __syncthreads();                      // single buffer: everyone must be done reading first
        if (kt < 7) AP(kt * 8 + 4)
        if constexpr (DMA) { if (kt + 1 < nt) stage_dma(kt + 1); }
        else if (kt + 1 < nt) { STORE_TILE(NBUF == 2 ? ((kt + 1) & 1) : 0) }
        if (kt < 7) AP(kt * 8 + 5)
        __syncthreads();
        if (kt < 7) AP(kt * 8 + 6)
    };
    for (int kt = 0; kt < nt - (small_tail ? 1 : 0); ++kt) tile(kt, std::integral_constant<int, 0>{});
    if (small_tail) tile(nt - 1, std::integral_constant<int, 2>{});
#undef LOAD_TILE
#undef STORE_TILE

    // ---- finalise: O[q][d] = O^T / l ; lane (q, h) owns d = dm*32 + 8*(r>>2) + 4*h + (r&3)
    AP(62)
    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv = 1.0f / l_tot;
    // (DMA) the lane's query and key half are re-derived from an opaque lane id: kept alive from the prologue they are three registers
    // spilled around the key loop
    int elq = lq, elh = lh;
    if constexpr (DMA) {
        int ln;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
        elq = ln & 31;
        elh = ln >> 5;
    }
    const int q = q0 + elq;
    if (q < q_len) {
        if (OUTMODE == 2) {
            fp8e4* orow = (fp8e4*)p.out + (out_row0() + q) * (heads * HD) + head * HD;
#pragma unroll
            for (int dm = 0; dm < DM; ++dm)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    float v4[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) v4[j] = oacc[dm][rq * 4 + j] * inv;
                    store_cvt<fp8e4, 4>(orow + dm * 32 + 8 * rq + 4 * elh, v4);
                }
        } else if (OUTMODE == 3) {
            // F16C8 operand (the proj GEMM's A in the round-2 strict mode): f16 hi plane + k-permuted lo8 plane
            const int64_t e0 = (out_row0() + q) * (heads * HD) + head * HD;
#pragma unroll
            for (int dm = 0; dm < DM; ++dm)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    float v4[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) v4[j] = oacc[dm][rq * 4 + j] * inv;
                    f16c8_store4((f16c8*)p.out, p.out_plane, e0 + dm * 32 + 8 * rq + 4 * elh, v4);
                }
        } else if (OUTMODE == 1 || OUTMODE == 4) {
            // (hi, lo) planes of ANOTHER 16-bit type than the kernel's operands: 1 = split-bf16, 4 = split-f16 (BD_PREC_F16X3)
            typedef typename std::conditional<OUTMODE == 1, __bf16, _Float16>::type OT;
            OT* orow = (OT*)p.out + (out_row0() + q) * (heads * HD) + head * HD;
#pragma unroll
            for (int dm = 0; dm < DM; ++dm)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    const int d0 = dm * 32 + 8 * rq + 4 * elh;
                    typedef __attribute__((__vector_size__(4 * sizeof(OT)))) OT ovec4;
                    ovec4 hi, lo;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float h, l;
                        split_hi_lo<OT>(oacc[dm][rq * 4 + j] * inv, h, l);
                        hi[j] = from_f32<OT>(h);
                        lo[j] = from_f32<OT>(l);
                    }
                    *(ovec4*)(orow + d0) = hi;
                    *(ovec4*)(orow + p.out_plane + d0) = lo;
                }
        } else {
            T* orow = (T*)p.out + (out_row0() + q) * (heads * HD) + head * HD;
#pragma unroll
            for (int dm = 0; dm < DM; ++dm)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    const int d0 = dm * 32 + 8 * rq + 4 * elh;
                    typedef __attribute__((__vector_size__(4 * sizeof(T)))) T vec4;
                    vec4 hi, lo;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (NS == 2) {
                            float h, l;
                            split_hi_lo<T>(oacc[dm][rq * 4 + j] * inv, h, l);
                            hi[j] = from_f32<T>(h);
                            lo[j] = from_f32<T>(l);
                        } else {
                            hi[j] = from_f32<T>(oacc[dm][rq * 4 + j] * inv);
                        }
                    }
                    *(vec4*)(orow + d0) = hi;
                    if (NS == 2) *(vec4*)(orow + p.out_plane + d0) = lo;
                }
        }
    }
#ifdef BD_ATTN_PROBE
    AP(63)
    if (bd_attn_probe_buf && blockIdx.x < 512) bd_attn_probe_buf[((size_t)blockIdx.x * 8 + wid) * 64 + lane] = probe_ts;
#endif
}

// ------------------------------------------------------------------------------------------------
// Software-pipelined form (round 2) for the single-plane operand classes: 8 waves, 256 queries per workgroup, one per CU.
//
// Why (tools/attn_phase_probe.py, profiles/r2_attention.md): attn_kernel runs S(t), softmax(t), PV(t) one after the other in
// every wave; with two independent 4-wave workgroups per CU the two waves of a SIMD fell into the same phase (VALU 55 % + MFMA
// 29 % busy adding up instead of overlapping).  A first round-2 attempt put the two waves of a SIMD into ONE workgroup, a
// barrier-enforced segment apart (one in its MFMA segment while the other does its softmax): measured 1376-1759 cycles for a
// 768-cycle MFMA segment and 504 vs 1419 cycles for the same softmax depending on which wave wins the issue arbitration --
// a dense VALU stream and an MFMA stream of two different waves do not share a SIMD's issue port gracefully.  What does work
// is interleaving them inside ONE instruction stream: an MFMA occupies the issue port for 4 of its 32 cycles, and the same
// wave's next 6-7 VALU instructions ride in the rest.  So each wave here runs, per key tile t,
//     24 MFMA slots = PV(t-1) (12) + S(t+1) (12),   with the VALU work of softmax(t) spread over the slots,
// i.e. the softmax of a tile executes under the matrix work of its two neighbours (two S accumulator sets, two P fragment
// sets; order pinned with sched_barrier).  Operand fragments are read three slots ahead into a ring of four registers.
// Staging: all 512 threads fetch tile t+2 (global -> registers) at the top of iteration t and store it (K as is, V transposed,
// attn_kernel's LDS images) at its end; K ring 2 tiles, V^T ring 4 tiles, ONE barrier per tile.
template <class T, int HD, int OUTMODE, bool VL = false>
__global__ __launch_bounds__(512, 1) void attn_kernel_pp(const AttnArgs p) {
    bd_saturating_conversions();      // fp8 / f16 results saturate (bd_common.h: RANGE)
    typedef typename Op16<T>::vec8 vec8;
    constexpr int NT = 512;
    constexpr int DCH = HD / 8;
    constexpr int KSTRIDE = HD * 2 + 16;
    constexpr int K_BYTES = KT * KSTRIDE;
    constexpr int V_BYTES = HD * 128;
    constexpr int KBUF = 2, VBUF = 4;
    constexpr int VMT = (KT / 4) * DCH;
    static_assert(VMT <= NT, "one V micro-tile per thread");
    constexpr int QB = 256;
    constexpr int DM = HD / 32;
    constexpr int KS = HD / 16;
    constexpr int NPV = 4 * DM, NS_ = 2 * KS, NSLOT = NPV + NS_;
    static_assert(NSLOT >= 22, "softmax schedule below needs 22 slots");
    // output staging (plain 16-bit and F16C8 results): one row image per query, [hi plane | lo8 plane], 16 bytes of padding
    constexpr bool OUT_VIA_LDS = (OUTMODE == 0 || OUTMODE == 3);
    constexpr int OROW = (OUTMODE == 3) ? HD * 3 : HD * 2;
    constexpr int OSTRIDE = OROW + 16;
    constexpr int RING_BYTES = KBUF * K_BYTES + VBUF * V_BYTES;
    constexpr int LDS_BYTES = (OUT_VIA_LDS && 8 * 32 * OSTRIDE > RING_BYTES) ? 8 * 32 * OSTRIDE : RING_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    unsigned char* const vring = lds;
    unsigned char* const kring = lds + VBUF * V_BYTES;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lq = lane & 31, lh = lane >> 5;
    int seq = p.seq;
    const int heads = p.heads;
    int q_len = p.q_len;
    int nqb = (q_len + QB - 1) / QB;

    int wg;
    {
        const int nwg = gridDim.x, bid = blockIdx.x, xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    int qb = wg % nqb;
    int bh = wg / nqb;
    int head = bh % heads, b = bh / heads;
    int64_t row0 = (int64_t)b * seq;
    int vl_views = 0;
    if constexpr (VL) {      // as attn_kernel: the implicit (sample, head, q-block) work list of a ragged batch
        if (!p.q_view) {
            const int ipv = (p.tpv / QB) * heads;
            b = vl_sample_of(p.view_start, p.batch, ipv, wg, lane);
            if (b >= p.batch) return;
        }
        const int s0 = __builtin_amdgcn_readfirstlane(p.view_start[b]), s1 = __builtin_amdgcn_readfirstlane(p.view_start[b + 1]);
        vl_views = s1 - s0;
        if (s0 < 0 || vl_views <= 0 || vl_views > p.max_views || s1 > p.n_views) return;
        seq = vl_views * p.tpv;
        row0 = (int64_t)s0 * p.tpv;
        if (!p.q_view) {
            q_len = seq;
            nqb = vl_views * (p.tpv / QB);
            const int local = wg - s0 * (p.tpv / QB) * heads;
            qb = local % nqb;
            head = local / nqb;
        }
    }

    const int ld = 3 * heads * HD;
    const T* base = (const T*)p.qkv + row0 * ld + head * HD;
    const T* kbase = base + heads * HD;
    const T* vbase = base + 2 * heads * HD;

    const int q0 = qb * QB + wid * 32;
    int qbase_row = p.q_view ? p.q_view[b] * q_len : p.q_off;
    if constexpr (VL) { if (p.q_view) { const int qv = p.q_view[b]; qbase_row = (qv < 0 ? 0 : (qv < vl_views ? qv : vl_views - 1)) * q_len; } }
    int qrow = q0 + lq; qrow = (qrow < q_len ? qrow : q_len - 1) + qbase_row;
    auto out_row0 = [&]() -> int64_t {
        if constexpr (VL) { if (!p.q_view) return row0; }
        return (int64_t)b * p.out_rows + (p.out_rows == q_len ? 0 : p.q_off);
    };
    vec8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = as_vec8<T>(*(const u128*)(base + (unsigned)(qrow * ld + ks * 16 + lh * 8)));

    // ---- staging coordinates
    // K tile: 8 threads per key row; thread (row, j) moves 16-byte pieces j and j + 8 (< DCH) of the row, so that the second piece's
    // global and LDS addresses are the first one's plus an immediate (no second set of address registers: the loop's budget is full)
    static_assert(KT * 8 == NT && DCH > 8 && DCH <= 16, "K staging: 8 threads per key row, two pieces each");
    const int kc_row = tid >> 3, kc_col = tid & 7;
    const bool kc_two = kc_col < DCH - 8;
    const int vm_kq = tid / DCH, vm_dc = tid % DCH;
    const bool vm_active = tid < VMT;
    // The host launches this kernel for whole key tiles only (dispatch: q_len % 256 == 0 and seq % 64 == 0).  K / V tiles are fetched with
    // BUFFER loads: one wave-uniform descriptor over this (sample, head)'s rows, the tile / row origin in the SCALAR offset, and ONE
    // loop-invariant 32-bit byte offset per lane for K and one for V -- no vector address arithmetic per tile (round 5: the flat form
    // cost five 64-bit multiply-adds + shifts per tile and wave in a loop whose VALU is the bound; MI355X guide T8 / T20).
    int vdst;
    {
        const int g = vm_kq >> 2, qi = vm_kq & 3;
        const int qp = (qi == 1) ? 2 : (qi == 2 ? 1 : qi);
        vdst = ((g * 2 + (qp >> 1)) << 4) | ((qp & 1) << 3);
    }
    u128 rk[2], rv[4];
    __amdgpu_buffer_rsrc_t rsrc;
    {
        const uintptr_t a = (uintptr_t)base;
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
        rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(((uintptr_t)hi << 32) | lo), 0, __builtin_amdgcn_readfirstlane(seq * ld * (int)sizeof(T)), 0x00020000);
    }
    const int k_voff = (kc_row * ld + kc_col * 8 + heads * HD) * (int)sizeof(T);
    const int v_voff = (vm_kq * 4 * ld + vm_dc * 8 + 2 * heads * HD) * (int)sizeof(T);
    const int row_bytes = __builtin_amdgcn_readfirstlane(ld * (int)sizeof(T));
    auto load_tile = [&](int kt) {
        const int t_off = kt * KT * row_bytes;                        // scalar
        rk[0] = __builtin_bit_cast(u128, __builtin_amdgcn_raw_buffer_load_b128(rsrc, k_voff, t_off, 0));
        if (kc_two) rk[1] = __builtin_bit_cast(u128, __builtin_amdgcn_raw_buffer_load_b128(rsrc, k_voff + 128, t_off, 0));
        if (vm_active) {
#pragma unroll
            for (int j = 0; j < 4; ++j) rv[j] = __builtin_bit_cast(u128, __builtin_amdgcn_raw_buffer_load_b128(rsrc, v_voff, t_off + j * row_bytes, 0));
        }
    };
    auto store_tile = [&](int kt, int kbi, int vbi) {
        (void)kt;
        unsigned char* kl = kring + kbi * K_BYTES;
        unsigned char* vl = vring + vbi * V_BYTES;
        *(u128*)(kl + kc_row * KSTRIDE + kc_col * 16) = rk[0];
        if (kc_two) *(u128*)(kl + kc_row * KSTRIDE + kc_col * 16 + 128) = rk[1];
        if (vm_active) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const unsigned a0 = rv[0][w], a1 = rv[1][w], a2 = rv[2][w], a3 = rv[3][w];
                const int d = vm_dc * 8 + 2 * w;
                uint2 lo, hi;
                lo.x = pack_lo16(a0, a1); lo.y = pack_lo16(a2, a3);
                hi.x = pack_hi16(a0, a1); hi.y = pack_hi16(a2, a3);
                *(uint2*)(vl + d * 128 + (vdst ^ (vswz(d) << 4))) = lo;
                *(uint2*)(vl + (d + 1) * 128 + (vdst ^ (vswz(d + 1) << 4))) = hi;
            }
        }
    };

    f32x16 oacc[DM];
#pragma unroll
    for (int i = 0; i < DM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const float sc = p.scale_log2e;
    const int nt = (seq + KT - 1) / KT;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    // ---- prologue: tiles 0 and 1 staged; the V^T buffer of "tile -1" zeroed (iteration 0 runs PV(-1) = 0 . 0 through it)
    load_tile(0);
    store_tile(0, 0, 0);
    if (nt > 1) { load_tile(1); store_tile(1, 1, 1); }
    for (int i = tid * 16; i < V_BYTES; i += NT * 16) *(u128*)(vring + (VBUF - 1) * V_BYTES + i) = (u128){0u, 0u, 0u, 0u};
    __syncthreads();

    // S[t & 1] = scores of tile t, P[t & 1] = probability fragments of tile t.  The loop is unrolled over the ring period (4)
    // so that every LDS address is a loop-invariant per-lane register plus an immediate and no register set is ever copied.
    // The P fragments are ONE set, rewritten in place: PV(t-1) reads group g in slots 3 g .. 3 g + 2 and softmax(t) writes group g in
    // slots 5 + 4 g .. 8 + 4 g, always later.
    f32x16 S[2][2];
    vec8 P[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int j = 0; j < 8; ++j) P[g][j] = from_f32<T>(0.f);                    // "P(-1)"
    const unsigned kfrag = (unsigned)(lq * KSTRIDE + lh * 16);                      // K fragment: + km*32*KSTRIDE + ks*32 (immediates)
    unsigned vfrag[DM];               // V^T fragment of (dm, 16-key group g) = vfrag[dm] ^ (g << 5): chunk (2 g + lh) ^ vswz(d)
#pragma unroll
    for (int dm = 0; dm < DM; ++dm) {
        const int d = dm * 32 + lq;
        vfrag[dm] = (unsigned)(d * 128 + ((lh ^ vswz(d)) << 4));
    }
    {   // S(0)
#pragma unroll
        for (int km = 0; km < 2; ++km)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const vec8 kf = as_vec8<T>(*(const u128*)(kring + kfrag + km * 32 * KSTRIDE + ks * 32));
                S[0][km] = Op16<T>::mfma(kf, qf[ks], ks == 0 ? zero16 : S[0][km]);
            }
    }
#ifdef BD_ATTN_PROBE
    unsigned probe_ts = 0;
#endif
    // one key tile; TI = t % 4 at compile time
#define PP_LOADF(dst, n)                                                                                         \
    {                                                                                                             \
        if ((n) < NPV) {                                                                                          \
            dst = as_vec8<T>(*(const u128*)(vring + ((TI + 3) % VBUF) * V_BYTES + (vfrag[(n) % DM] ^ (unsigned)(((n) / DM) << 5)))); \
        } else {                                                                                                  \
            const int ks_ = ((n) - NPV) / 2, km_ = ((n) - NPV) % 2;    /* alternate the two S accumulators */      \
            dst = as_vec8<T>(*(const u128*)(kring + ((TI + 1) % KBUF) * K_BYTES + kfrag + km_ * 32 * KSTRIDE + ks_ * 32)); \
        }                                                                                                         \
    }
#define PP_MFMA(n, f)                                                                                            \
    {                                                                                                             \
        if ((n) < NPV) {                                                                                          \
            oacc[(n) % DM] = Op16<T>::mfma(f, P[(n) / DM], oacc[(n) % DM]);                                       \
        } else {                                                                                                  \
            const int ks_ = ((n) - NPV) / 2, km_ = ((n) - NPV) % 2;                                               \
            S[(TI + 1) & 1][km_] = Op16<T>::mfma(f, qf[ks_], ks_ == 0 ? zero16 : S[(TI + 1) & 1][km_]);          \
        }                                                                                                         \
    }
#define PP_ITER(TI_)                                                                                             \
    {                                                                                                             \
        constexpr int TI = (TI_);                                                                                 \
        if (t >= 4 && t < 16) AP((t - 4) * 5)                                                                     \
        const bool stage = t + 2 < nt;                                                                            \
        if (stage) load_tile(t + 2);                                                                              \
        vec8 fr[4];                                                                                               \
        float tmax = -INFINITY, psum = 0.f, mneg = 0.f, alpha = 1.f;                                              \
        bool moved = false;                                                                                       \
        _Pragma("unroll") for (int n = 0; n < 3; ++n) PP_LOADF(fr[n & 3], n)                                      \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        _Pragma("unroll") for (int n = 0; n < NSLOT; ++n) {                                                       \
            PP_MFMA(n, fr[n & 3])                                                                                 \
            if (n + 3 < NSLOT) PP_LOADF(fr[(n + 3) & 3], n + 3)                                                   \
            if (n < 4) {                        /* row max, 8 scores per slot */                                  \
                _Pragma("unroll") for (int e = n * 8; e < n * 8 + 8; ++e) tmax = fmaxf(tmax, S[TI & 1][e >> 4][e & 15]); \
                asm volatile("" : "+v"(tmax));   /* pin: IR passes sink side-effect-free code past sched_barrier */  \
            } else if (n == 4) {                /* the other half of the query's keys lives in lane ^ 32 */       \
                float other;      /* two DISTINCT registers: the builtin given one value twice swaps nothing */    \
                asm volatile("v_mov_b32 %1, %0\n\ts_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(tmax), "=&v"(other)); \
                tmax = fmaxf(tmax, other);                                                                        \
                const float m_new = fmaxf(m_run, tmax);                                                           \
                moved = !__all(m_new == m_run);                                                                   \
                alpha = __builtin_amdgcn_exp2f((m_run - m_new) * sc);   /* 1 where the max did not move */        \
                m_run = m_new;                                                                                    \
                mneg = -m_new * sc;                                                                               \
            } else if (n < 21) {                /* 2 probabilities per slot: exp2, row sum, conversion */         \
                _Pragma("unroll") for (int e = (n - 5) * 2; e < (n - 5) * 2 + 2; ++e) {                           \
                    float pv = __builtin_amdgcn_exp2f(fmaf(S[TI & 1][e >> 4][e & 15], sc, mneg));                \
                    asm volatile("" : "+v"(pv));                                                                  \
                    psum += pv;                                                                                   \
                    P[e >> 3][e & 7] = from_f32<T>(pv);                                                           \
                }                                                                                                 \
            }                                                                                                     \
            __builtin_amdgcn_sched_barrier(0);                                                                    \
        }                                                                                                         \
        if (moved) {                    /* O and l follow the new max (PV(t-1) was added under the old one) */    \
            _Pragma("unroll") for (int i = 0; i < DM; ++i)                                                        \
                _Pragma("unroll") for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;                               \
            l_run *= alpha;                                                                                       \
        }                                                                                                         \
        l_run += psum;                                                                                            \
        if (t >= 4 && t < 16) AP((t - 4) * 5 + 1)                                                                 \
        if (stage) store_tile(t + 2, (TI + 2) % KBUF, (TI + 2) % VBUF);                                           \
        if (t >= 4 && t < 16) AP((t - 4) * 5 + 2)                                                                 \
        __syncthreads();                                                                                          \
        if (t >= 4 && t < 16) AP((t - 4) * 5 + 3)                                                                 \
        ++t;                                                                                                      \
    }
    int t = 0;
    while (t + 4 <= nt) { PP_ITER(0) PP_ITER(1) PP_ITER(2) PP_ITER(3) }
    const int rem = nt - t;                 // t % 4 == 0 here
    if (rem > 0) PP_ITER(0)
    if (rem > 1) PP_ITER(1)
    if (rem > 2) PP_ITER(2)
#undef PP_ITER
#undef PP_LOADF
#undef PP_MFMA
#ifdef BD_ATTN_PROBE
    if (bd_attn_probe_buf && blockIdx.x < 512) bd_attn_probe_buf[((size_t)blockIdx.x * 8 + wid) * 64 + lane] = probe_ts;
#endif
    {   // PV(nt-1): V^T buffer (nt-1) % 4 -- a run-time index here, once per kernel
        const unsigned char* vcur = vring + ((nt - 1) % VBUF) * V_BYTES;
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int dm = 0; dm < DM; ++dm) {
                const vec8 vf = as_vec8<T>(*(const u128*)(vcur + (vfrag[dm] ^ (unsigned)(g << 5))));
                oacc[dm] = Op16<T>::mfma(vf, P[g], oacc[dm]);
            }
    }

    // ---- finalise: O[q][d] = O^T / l ; lane (q, h) owns d = dm*32 + 8*(r>>2) + 4*h + (r&3)
    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv = 1.0f / l_tot;
    if constexpr (OUT_VIA_LDS) {
        // The lanes hold O^T (a query per lane, 4 consecutive d per register quad): written out directly that is 32 rows x 16
        // bytes per store instruction, ~10k cycles of a workgroup's ~100k (profiles/r2_attention.md).  Instead every wave lays its
        // 32 query rows out in LDS (the rings are dead after the barrier) and stores whole 16-byte pieces of full rows.
        __syncthreads();
        // the lane id is re-derived HERE from an opaque instruction: nothing of this block's addressing can then be hoisted above
        // the key loop, whose register budget is full (hoisted, it put a spill reload = a vector-memory load into every iteration)
        int ln;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
        const int lq2 = ln & 31, lh2 = ln >> 5;
        unsigned char* const wl = lds + wid * (32 * OSTRIDE);
        unsigned char* const rowp = wl + lq2 * OSTRIDE;
#pragma unroll
        for (int dm = 0; dm < DM; ++dm)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                float v4[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v4[j] = oacc[dm][rq * 4 + j] * inv;
                const int d = dm * 32 + 8 * rq + 4 * lh2;
                if constexpr (OUTMODE == 3) f16c8_store4((f16c8*)rowp, HD, d, v4);
                else store_cvt<T, 4>((T*)rowp + d, v4);
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        constexpr int CPR = OROW / 16, HIC = HD / 8;           // 16-byte pieces per row image / of its hi plane
        static_assert((32 * CPR) % 64 == 0, "pieces per wave");
        const int64_t orow0 = out_row0() + q0;
        unsigned char* const out_hi = (unsigned char*)p.out;
        unsigned char* const out_lo = out_hi + 2 * p.out_plane;
#pragma unroll
        for (int k = 0; k < 32 * CPR / 64; ++k) {
            const int c = ln + 64 * k, r = c / CPR, col = c % CPR;
            if (q0 + r >= q_len) continue;
            const u128 piece = *(const u128*)(wl + r * OSTRIDE + col * 16);
            const int64_t e = (orow0 + r) * (heads * HD) + head * HD;
            if (OUTMODE == 3 && col >= HIC) *(u128*)(out_lo + e + (col - HIC) * 16) = piece;
            else *(u128*)(out_hi + 2 * e + col * 16) = piece;
        }
        return;
    }
    const int q = q0 + lq;
    if (q < q_len) {
        const int64_t e0 = (out_row0() + q) * (heads * HD) + head * HD;
#pragma unroll
        for (int dm = 0; dm < DM; ++dm)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                float v4[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v4[j] = oacc[dm][rq * 4 + j] * inv;
                const int64_t e = e0 + dm * 32 + 8 * rq + 4 * lh;
                if constexpr (OUTMODE == 2) {
                    store_cvt<fp8e4, 4>((fp8e4*)p.out + e, v4);
                } else if constexpr (OUTMODE == 3) {
                    f16c8_store4((f16c8*)p.out, p.out_plane, e, v4);
                } else if constexpr (OUTMODE == 1 || OUTMODE == 4) {
                    typedef typename std::conditional<OUTMODE == 1, __bf16, _Float16>::type OT;
                    float hi4[4], lo4[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) split_hi_lo<OT>(v4[j], hi4[j], lo4[j]);
                    store_cvt<OT, 4>((OT*)p.out + e, hi4);
                    store_cvt<OT, 4>((OT*)p.out + p.out_plane + e, lo4);
                } else {
                    store_cvt<T, 4>((T*)p.out + e, v4);
                }
            }
    }
}

// ---- Host side: validate -> plan -> launch (include/boxdreamer_hip.h: bd_attention_plan).  plan_attention decides everything about a call
// on the host (no HIP call, no global state, nothing dereferenced) and names the kernel by its template arguments; one table per kernel
// lists every instantiated kernel next to that key; launching is a lookup.  A key without a row is a plan error.
typedef bd_attn_call AttnCall;
struct attn_row { int key[BD_ATTN_KEY_LEN]; void (*fn)(const AttnArgs); };
struct attn_table { int family; const attn_row* rows; int n; };

// The operand classes, once: ONE(prec, TC, OUTMODE) is a single-plane class (NS = 1, both kernels), SPLIT(...) a split-bf16 one (NS = 2,
// the tiled kernel only: it is register-bound at one wave per SIMD).  TC is the element type's code in a key: 0 __bf16, 1 _Float16.
#define BD_ATTN_CLASSES(ONE, SPLIT)                                                                                    \
    ONE(BD_PREC_BF16, 0, 0) ONE(BD_PREC_F16, 1, 0) SPLIT(BD_PREC_BF16X3, 0, 0)                                         \
    ONE(BD_PREC_F16_OUT_BF16X3, 1, 1) ONE(BD_PREC_BF16_OUT_FP8, 0, 2)                                                  \
    ONE(BD_PREC_F16_OUT_F16C8, 1, 3) SPLIT(BD_PREC_BF16X3_OUT_F16C8, 0, 3)                                             \
    ONE(BD_PREC_F16_OUT_F16X3, 1, 4) SPLIT(BD_PREC_BF16X3_OUT_F16X3, 0, 4)
template <int TC> using elem_of = typename std::conditional<TC == 0, __bf16, _Float16>::type;

struct attn_class { int prec, tc, ns, om; };
const attn_class* class_of(int prec) {
#define BD_CLASS_ONE(PREC, TC, OM) {PREC, TC, 1, OM},
#define BD_CLASS_SPLIT(PREC, TC, OM) {PREC, TC, 2, OM},
    static const attn_class classes[] = {BD_ATTN_CLASSES(BD_CLASS_ONE, BD_CLASS_SPLIT)};
#undef BD_CLASS_ONE
#undef BD_CLASS_SPLIT
    for (const attn_class& c : classes)
        if (c.prec == prec) return &c;
    return nullptr;
}

// Every instantiated kernel: one argument list gives a row's key and its kernel, so a key cannot name another instance.
// attn_kernel, per class: head_dim 96 and 64 on 4 and on 3 waves, and the ragged (VL) instance -- head_dim 96, 4 waves
#define BD_TILED_ROW(TC, NS, HD, NW, OM, VL) {{TC, NS, HD, NW, OM, VL}, attn_kernel<elem_of<TC>, NS, HD, NW, OM, VL>},
#define BD_TILED_CLASS(TC, NS, OM)                                                                                     \
    BD_TILED_ROW(TC, NS, 96, 4, OM, false) BD_TILED_ROW(TC, NS, 96, 3, OM, false) BD_TILED_ROW(TC, NS, 64, 4, OM, false) \
    BD_TILED_ROW(TC, NS, 64, 3, OM, false) BD_TILED_ROW(TC, NS, 96, 4, OM, true)
#define BD_TILED_ONE(PREC, TC, OM) BD_TILED_CLASS(TC, 1, OM)
#define BD_TILED_SPLIT(PREC, TC, OM) BD_TILED_CLASS(TC, 2, OM)
attn_table tiled_table() {
    static const attn_row rows[] = {BD_ATTN_CLASSES(BD_TILED_ONE, BD_TILED_SPLIT)};
    return {BD_ATTN_FAMILY_TILED, rows, (int)(sizeof(rows) / sizeof(rows[0]))};
}
// attn_kernel_pp, per single-plane class: head_dim 96, uniform and ragged
#define BD_PP_ROW(TC, OM, VL) {{TC, 96, OM, VL}, attn_kernel_pp<elem_of<TC>, 96, OM, VL>},
#define BD_PP_ONE(PREC, TC, OM) BD_PP_ROW(TC, OM, false) BD_PP_ROW(TC, OM, true)
#define BD_PP_SPLIT(PREC, TC, OM)
attn_table pp_table() {
    static const attn_row rows[] = {BD_ATTN_CLASSES(BD_PP_ONE, BD_PP_SPLIT)};
    return {BD_ATTN_FAMILY_PP, rows, (int)(sizeof(rows) / sizeof(rows[0]))};
}
#undef BD_TILED_ROW
#undef BD_TILED_CLASS
#undef BD_TILED_ONE
#undef BD_TILED_SPLIT
#undef BD_PP_ROW
#undef BD_PP_ONE
#undef BD_PP_SPLIT

// The launch of the table row with this key; BD_ERR_SHAPE when no instance has it: never a neighbouring instance
int plan_row(const attn_table& t, const int (&key)[BD_ATTN_KEY_LEN], int grid, int block, bd_attn_launch* l) {
    for (int r = 0; r < t.n; ++r) {
        if (!std::equal(key, key + BD_ATTN_KEY_LEN, t.rows[r].key)) continue;
        l->family = t.family;
        l->row = r;
        std::copy(key, key + BD_ATTN_KEY_LEN, l->key);
        l->grid = grid;
        l->block = block;
        return BD_OK;
    }
    return BD_ERR_SHAPE;
}

// the K / V buffer descriptors span ONE sample's rows with a 32-bit byte count (and 32-bit per-lane offsets inside it)
inline bool sample_bytes_out_of_range(int seq, int heads, int head_dim) {
    return head_dim <= 0 || (int64_t)seq * 3 * heads * head_dim * 2 >= ((int64_t)1 << 31);
}

// The shape rules of a call: what its entry point refuses before it looks at the pointers' alignment
int call_shape(const AttnCall& c) {
    const int64_t lim = (int64_t)1 << 31;
    if (c.entry < BD_ATTN_ENTRY_PLAIN || c.entry > BD_ATTN_ENTRY_VARLEN) return BD_ERR_SHAPE;
    if (c.entry == BD_ATTN_ENTRY_VARLEN) {
        const int tpv = c.tokens_per_view;
        if (c.batch <= 0 || c.heads <= 0 || c.n_views < c.batch || c.max_views <= 0 || c.max_views > c.n_views - (c.batch - 1)) return BD_ERR_SHAPE;
        if (tpv <= 0 || tpv % 128) return BD_ERR_SHAPE;      // whole q-blocks and key tiles per view: no tail masks
        if (c.head_dim != 96) return BD_ERR_SHAPE;            // (DINOv2's head_dim 64 sequences are per image, never ragged)
        if ((int64_t)c.max_views * tpv >= lim || sample_bytes_out_of_range(c.max_views * tpv, c.heads, c.head_dim)) return BD_ERR_SHAPE;
        return (int64_t)c.n_views * (tpv / 128) * c.heads >= lim ? BD_ERR_SHAPE : BD_OK;
    }
    if (c.batch <= 0 || c.seq <= 0 || c.heads <= 0) return BD_ERR_SHAPE;
    if (c.entry == BD_ATTN_ENTRY_PREFIX && (c.n_prefix <= 0 || c.n_prefix >= c.seq)) return BD_ERR_SHAPE;
    if (c.entry == BD_ATTN_ENTRY_Q && (c.has_q_view ? (c.q_len <= 0 || c.q_len > c.seq || c.seq % c.q_len) : (c.q_len != c.seq))) return BD_ERR_SHAPE;
    return sample_bytes_out_of_range(c.seq, c.heads, c.head_dim) ? BD_ERR_SHAPE : BD_OK;
}

// The one launch of a call, or the code its entry point refuses it with (pointers apart: plan_checked)
int plan_attention(const AttnCall& c, bd_attn_launch* l) {
    if (const int rc = call_shape(c)) return rc;
    const attn_class* k = class_of(c.prec);
    if (!k) return BD_ERR_DTYPE;
    if (c.entry == BD_ATTN_ENTRY_VARLEN) {
        // Ragged batches, the VL instances.  Whole q-blocks per view (tpv % 256 == 0 for the ping-pong kernel, % 128 for the 4-wave one), so
        // the grid is EXACTLY the batch's q-blocks -- n_views * (tpv / QB) * heads with every row a query, batch * (tpv / QB) * heads with
        // q_view -- and nothing is sized by the longest sample.
        const int tpv = c.tokens_per_view, units = c.has_q_view ? c.batch : c.n_views;
        l->q_len = l->out_rows = tpv;
        l->q_off = 0;
        if (k->ns == 1 && tpv % 256 == 0) return plan_row(pp_table(), {k->tc, 96, k->om, true}, units * (tpv / 256) * c.heads, 512, l);
        return plan_row(tiled_table(), {k->tc, k->ns, 96, 4, k->om, true}, units * (tpv / 128) * c.heads, 256, l);
    }
    // With the prefix queries wanted, one launch over all seq queries IS the fastest form measured (profiles/r4_attention.md: a separate
    // launch for the prefix rows re-reads the pair's K / V -- 154 MB per DINOv2 launch -- and costs more than the ninth query wave it
    // saves); without them, the patch queries alone tile exactly: the seq - n_prefix queries behind the prefix, all keys; result rows
    // [n_prefix, seq) of every sample, the others untouched
    const bool skip_prefix = c.entry == BD_ATTN_ENTRY_PREFIX && !c.prefix_queries;
    const int q_len = skip_prefix ? c.seq - c.n_prefix : c.entry == BD_ATTN_ENTRY_Q ? c.q_len : c.seq;
    l->q_len = q_len;
    l->q_off = skip_prefix ? c.n_prefix : 0;
    l->out_rows = skip_prefix ? c.seq : q_len;
    if (c.head_dim != 96 && c.head_dim != 64) return BD_ERR_SHAPE;
    // ping-pong kernel where its 256-query blocks tile the query range without waste (BETR: 1536 = 6 x 256; last block: 256)
    // (latency forms, round 6: one pose at a time the 256-query blocks are 48 workgroups on 256 CUs, 36 us; the 128-query kernel's 96
    // take 31 us -- and lose from two poses on: profiles/r6_attn_b1_probe.txt)
    const bool few = c.latency_forms && 4 * ((q_len + 255) / 256) * c.heads * c.batch <= 256;      // (a quarter of MI355X's 256 CUs)
    if (k->ns == 1 && c.head_dim == 96 && q_len % 256 == 0 && c.seq % KT == 0 && !few)               // (whole key tiles only: the kernel has no tail mask)
        return plan_row(pp_table(), {k->tc, 96, k->om, false}, (q_len / 256) * c.heads * c.batch, 512, l);
    // 3 waves (96-query blocks) when that tiles the sequence with less waste (DINOv2: 261 -> 3 x 96)
    const int waste4 = ((q_len + 127) / 128) * 128 - q_len, waste3 = ((q_len + 95) / 96) * 96 - q_len;
    const int nw = waste3 < waste4 ? 3 : 4;
    return plan_row(tiled_table(), {k->tc, k->ns, c.head_dim, nw, k->om, false}, ((q_len + nw * 32 - 1) / (nw * 32)) * c.heads * c.batch, nw * 64, l);
}

// validate -> plan, for the entry points and bd_attention_plan alike.  Refusals win in the entry points' order: a null pointer, the
// call's shape, a misaligned pointer, then the class and head_dim.
int plan_checked(const AttnCall& c, const void* qkv, const void* out, const void* view_start, bd_attn_launch* l) {
    if (!qkv || !out || (c.entry == BD_ATTN_ENTRY_VARLEN && !view_start)) return BD_ERR_NULL;
    if (const int rc = call_shape(c)) return rc;
    if (((uintptr_t)qkv & 15) || ((uintptr_t)out & 7)) return BD_ERR_ALIGN;
    return plan_attention(c, l);
}

// The one launcher.  Launch trace: one kind-1 record over the sample's (ragged: the longest sample's) key rows.
int run(const AttnCall& c, const void* qkv, int64_t qkv_plane, void* out, int64_t out_plane, float scale, const int32_t* q_view,
        const int32_t* view_start, void* stream) {
    bd_attn_launch l;
    if (const int rc = plan_checked(c, qkv, out, view_start, &l)) return rc;
    const AttnArgs a{qkv, qkv_plane, out, out_plane, c.batch, c.seq, c.heads, scale * 1.4426950408889634f, q_view, l.q_len, l.q_off, l.out_rows,
                     view_start, c.tokens_per_view, c.n_views, c.max_views};
    const attn_table t = l.family == BD_ATTN_FAMILY_PP ? pp_table() : tiled_table();
    hipStream_t s = (hipStream_t)stream;
    const int slot = bd_trace_open(s, 1, c.batch * c.heads, view_start ? c.max_views * c.tokens_per_view : c.seq, c.head_dim);
    hipLaunchKernelGGL(t.rows[l.row].fn, dim3(l.grid), dim3(l.block), 0, s, a);
    bd_trace_close(s, slot);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

}  // namespace

int bd_attention_q_forms(const void* qkv, int64_t qkv_plane, void* out, int64_t out_plane, int batch, int seq, int heads, int head_dim,
                         float scale, const int32_t* q_view, int q_len, int prec, int latency_forms, void* stream) {
    return run({BD_ATTN_ENTRY_Q, batch, seq, heads, head_dim, q_view != nullptr, q_len, 0, 0, 0, 0, 0, prec, latency_forms != 0}, qkv, qkv_plane,
               out, out_plane, scale, q_view, nullptr, stream);
}

extern "C" int bd_attention_q(const void* qkv, int64_t qkv_plane, void* out, int64_t out_plane, int batch, int seq,
                              int heads, int head_dim, float scale, const int32_t* q_view, int q_len, int prec,
                              void* stream) {
    return bd_attention_q_forms(qkv, qkv_plane, out, out_plane, batch, seq, heads, head_dim, scale, q_view, q_len, prec, 0, stream);
}

extern "C" int bd_attention_prefix(const void* qkv, int64_t qkv_plane, void* out, int64_t out_plane, int batch, int seq, int heads,
                                   int head_dim, float scale, int n_prefix, int prefix_queries, int prec, void* stream) {
    return run({BD_ATTN_ENTRY_PREFIX, batch, seq, heads, head_dim, 0, 0, n_prefix, prefix_queries, 0, 0, 0, prec, 0}, qkv, qkv_plane, out,
               out_plane, scale, nullptr, nullptr, stream);
}

extern "C" int bd_attention(const void* qkv, int64_t qkv_plane, void* out, int64_t out_plane, int batch,
                            int seq, int heads, int head_dim, float scale, int prec, void* stream) {
    return run({BD_ATTN_ENTRY_PLAIN, batch, seq, heads, head_dim, 0, 0, 0, 0, 0, 0, 0, prec, 0}, qkv, qkv_plane, out, out_plane, scale, nullptr,
               nullptr, stream);
}

extern "C" int bd_attention_varlen(const void* qkv, int64_t qkv_plane, void* out, int64_t out_plane, const int32_t* view_start, int batch,
                                   int n_views, int max_views, int tokens_per_view, int heads, int head_dim, float scale,
                                   const int32_t* q_view, int prec, void* stream) {
    return run({BD_ATTN_ENTRY_VARLEN, batch, 0, heads, head_dim, q_view != nullptr, 0, 0, 0, n_views, max_views, tokens_per_view, prec, 0}, qkv,
               qkv_plane, out, out_plane, scale, q_view, view_start, stream);
}

extern "C" int bd_attention_plan(const bd_attn_call* call, const void* qkv, const void* out, const void* view_start, bd_attn_plan_t* plan) {
    if (!plan) return BD_ERR_NULL;
    const int rc = call ? plan_checked(*call, qkv, out, view_start, &plan->launch[0]) : BD_ERR_NULL;
    plan->n_launches = rc == BD_OK;
    return rc;
}

extern "C" int bd_attention_instance(int family, int index, int* key) {
    const attn_table t = family == BD_ATTN_FAMILY_TILED ? tiled_table() : family == BD_ATTN_FAMILY_PP ? pp_table() : attn_table{0, nullptr, 0};
    if (!key || index < 0 || index >= t.n) return 0;
    std::copy(t.rows[index].key, t.rows[index].key + BD_ATTN_KEY_LEN, key);
    return 1;
}
