// Data-movement kernels either side of the GEMMs (HBM-bound): image normalise + im2col,
// heatmap patchify, token-row bookkeeping, unpatchify + sigmoid.
#include "bd_common.h"

namespace {

// one thread per 8-wide chunk of an output row [n*grid*grid, kpad]; k = c*p*p + py*p + px
template <class T, int NS>
__global__ __launch_bounds__(256) void im2col_kernel(const void* __restrict__ img, int dtype, void* __restrict__ out_,
                                                     int64_t plane, int n_images, int size, int patch, int kpad) {
    bd_saturating_conversions();      // fp8 / f16 results saturate (bd_common.h: RANGE)
    T* out = (T*)out_;
    const int grid = size / patch, pp = patch * patch, kreal = 3 * pp, cpr = kpad / 8;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)n_images * grid * grid * cpr;
    if (t >= total) return;
    const int kc = (int)(t % cpr);
    const int64_t row = t / cpr;
    const int gx = (int)(row % grid), gy = (int)((row / grid) % grid);
    const int64_t n = row / (grid * grid);
    const float mean[3] = {0.485f, 0.456f, 0.406f};
    const float stdv[3] = {0.229f, 0.224f, 0.225f};
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = kc * 8 + j;
        float y = 0.f;
        if (k < kreal) {
            const int c = k / pp, rem = k % pp, py = rem / patch, px = rem % patch;
            const int64_t src = ((n * 3 + c) * size + gy * patch + py) * size + gx * patch + px;
            y = (load_any(img, src, dtype) - mean[c]) / stdv[c];   // encoder/dinov2.py:45-46
        }
        v[j] = y;
    }
    store_operand8<T, NS>(out, plane, row * kpad + kc * 8, v);
}

// BETR.patchify: chunk j of a row holds the `channels` (= 8) values of pixel (py, px), j = py*p + px
template <class T, int NS>
__global__ __launch_bounds__(256) void patchify_kernel(const void* __restrict__ heat, int dtype, void* __restrict__ out_,
                                                       int64_t plane, int n_images, int size, int patch, int kpad) {
    bd_saturating_conversions();      // fp8 / f16 results saturate (bd_common.h: RANGE)
    T* out = (T*)out_;
    const int grid = size / patch, pp = patch * patch, cpr = kpad / 8;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)n_images * grid * grid * cpr;
    if (t >= total) return;
    const int j = (int)(t % cpr);
    const int64_t row = t / cpr;
    const int gx = (int)(row % grid), gy = (int)((row / grid) % grid);
    const int64_t n = row / (grid * grid);
    float v[8];
    if (j < pp) {
        const int py = j / patch, px = j % patch;
        const int64_t pix = (int64_t)(gy * patch + py) * size + gx * patch + px;
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = load_any(heat, (n * 8 + c) * (int64_t)size * size + pix, dtype);
    } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = 0.f;
    }
    store_operand8<T, NS>(out, plane, row * kpad + j * 8, v);
}

// ---------------------------------------------------------------- row-strip forms of im2col / patchify (patch 14: the path's geometry)
// The one-thread-per-chunk kernels above gather 2-byte elements (14-pixel runs per plane and patch row: 1.4 / 2.2 TB/s on the
// path's shapes).  im2col: one workgroup takes a horizontal strip of <= 8 patches of one patch row: every (plane, pixel row) of the
// strip is one contiguous run of <= 112 pixels, loaded in 4-byte pieces into an LDS image [patch][plane][14 x 14] of fp32 values,
// and the operand rows leave as whole 16-byte chunks.  patchify: see patchify_pair_kernel.  Same arithmetic per element as the
// kernels above (same bits: tools/layout_hash.py).
constexpr int STRIP = 8, P14 = 14, PP14 = P14 * P14;

__device__ __forceinline__ void load_pair_f32(const void* src, int64_t e, int dtype, float& a, float& b) {       // elements e, e + 1 (e even)
    if (dtype == BD_DTYPE_F32) {
        const float2 v = *(const float2*)((const float*)src + e);
        a = v.x; b = v.y;
    } else {
        const unsigned u = *(const unsigned*)((const unsigned short*)src + e);
        if (dtype == BD_DTYPE_BF16) {
            a = __builtin_bit_cast(float, u << 16); b = __builtin_bit_cast(float, u & 0xffff0000u);
        } else {
            a = (float)__builtin_bit_cast(_Float16, (unsigned short)(u & 0xffffu)); b = (float)__builtin_bit_cast(_Float16, (unsigned short)(u >> 16));
        }
    }
}

// planes: 3 (images, normalised) or 8 (heatmaps).  Fills tile[p][c][py * 14 + px] for the strip's np patches.
template <int NC, bool NORMALISE>
__device__ __forceinline__ void strip_load(const void* src, int dtype, int64_t n, int size, int gy, int x0, int np, float* tile) {
    const float mean[3] = {0.485f, 0.456f, 0.406f};
    const float stdv[3] = {0.229f, 0.224f, 0.225f};
    // lane = 4-byte piece of the run (<= 56 of 64 lanes), wave = (plane, pixel row) mod 4: no per-element index division
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane >= np * (P14 / 2)) return;
    const int x = 2 * lane, p = x / P14, px = x % P14;  // (14 is even: both pixels of a piece lie in the same patch)
    float* dcol = tile + p * NC * PP14 + px;
    const int64_t base = ((n * NC) * size + gy * P14) * (int64_t)size + x0 + x;
#pragma unroll 4
    for (int cy = wid; cy < NC * P14; cy += 4) {
        const int c = cy / P14, py = cy - c * P14;
        float a, b;
        load_pair_f32(src, base + ((int64_t)c * size + py) * size, dtype, a, b);
        if constexpr (NORMALISE) { a = (a - mean[c < 3 ? c : 0]) / stdv[c < 3 ? c : 0]; b = (b - mean[c < 3 ? c : 0]) / stdv[c < 3 ? c : 0]; }   // encoder/dinov2.py:45-46
        float* d = dcol + c * PP14 + py * P14;
        d[0] = a; d[1] = b;
    }
}

template <class T, int NS>
__global__ __launch_bounds__(256) void im2col_strip_kernel(const void* __restrict__ img, int dtype, void* __restrict__ out_,
                                                           int64_t plane, int n_images, int size, int kpad) {
    bd_saturating_conversions();
    __shared__ __attribute__((aligned(16))) float tile[STRIP * 3 * PP14];
    const int grid = size / P14, nsb = (grid + STRIP - 1) / STRIP, cpr = kpad / 8, kreal = 3 * PP14;
    const int sb = blockIdx.x % nsb, gy = (blockIdx.x / nsb) % grid;
    const int64_t n = blockIdx.x / (nsb * grid);
    const int gx0 = sb * STRIP, np = grid - gx0 < STRIP ? grid - gx0 : STRIP;
    strip_load<3, true>(img, dtype, n, size, gy, gx0 * P14, np, tile);
    __syncthreads();
    T* out = (T*)out_;
    for (int i = threadIdx.x; i < np * cpr; i += 256) {
        const int p = i / cpr, kc = i % cpr;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { const int k = kc * 8 + j; v[j] = k < kreal ? tile[p * kreal + k] : 0.f; }     // k = c*196 + py*14 + px
        const int64_t row = (n * grid + gy) * grid + gx0 + p;
        store_operand8<T, NS>(out, plane, row * kpad + kc * 8, v);
    }
}

// patchify without the LDS: a thread takes the two pixels (y, x), (y, x + 1) of ALL 8 channel planes (eight 4-byte loads, 256
// contiguous bytes per wave instruction) -- exactly the two adjacent 8-channel chunks (py, px), (py, px + 1) of one operand row.
// (The strip form with an LDS image measured slower than the gather it replaces: 161 against 114 us.)
template <class T, int NS>
__global__ __launch_bounds__(256) void patchify_pair_kernel(const void* __restrict__ heat, int dtype, void* __restrict__ out_,
                                                            int64_t plane, int n_images, int size, int kpad) {
    bd_saturating_conversions();
    const int half = size / 2, grid = size / P14, cpr = kpad / 8;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n_images * size * half) return;
    const int xp = (int)(t % half), y = (int)((t / half) % size);
    const int64_t n = t / ((int64_t)half * size);
    const int x = 2 * xp, gx = x / P14, px = x % P14, gy = y / P14, py = y % P14;
    float a[8], b[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) load_pair_f32(heat, ((n * 8 + c) * size + y) * (int64_t)size + x, dtype, a[c], b[c]);
    T* out = (T*)out_;
    const int64_t row = (n * grid + gy) * grid + gx;
    const int j = py * P14 + px;
    store_operand8<T, NS>(out, plane, row * kpad + j * 8, a);
    store_operand8<T, NS>(out, plane, row * kpad + (j + 1) * 8, b);
    if (py == 0) {                                       // the row's zero padding chunks [196, kpad / 8): by the patch's first pixel row
        const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int jj = PP14 + px / 2; jj < cpr; jj += P14 / 2) store_operand8<T, NS>(out, plane, row * kpad + jj * 8, z);
    }
}

__global__ __launch_bounds__(256) void prefix_kernel(float* __restrict__ x, const float* __restrict__ prefix,
                                                     int n_images, int tpi, int n_prefix, int dim) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)n_images * n_prefix * dim;
    if (t >= total) return;
    const int d = (int)(t % dim), pfx = (int)((t / dim) % n_prefix);
    const int64_t n = t / ((int64_t)dim * n_prefix);
    x[(n * tpi + pfx) * dim + d] = prefix[pfx * dim + d];
}

// The query view of sample b as a view index of the whole batch.  Uniform batch (vstart == NULL): b * T + qidx[b].  Ragged batch:
// sample b owns the views [vstart[b], vstart[b + 1]) and qidx[b] counts inside them (clamped to the sample: the offsets are device data;
// q < 0 takes the sample's view 0, q >= n its view n - 1).  An EMPTY sample (n <= 0) has no view to clamp to: it resolves to view
// vstart[b], which belongs to the next sample -- or, for the last sample, lies past the buffer.  The C entries cannot see the offsets
// (device data), so the callers that build them refuse an empty sample on the host (_lib.view_starts, _lib.check_view_counts).
__device__ __forceinline__ int64_t query_view_of(const int32_t* __restrict__ vstart, const int32_t* __restrict__ qidx, int b, int T) {
    if (!vstart) return (int64_t)b * T + (qidx ? qidx[b] : 0);
    const int v0 = vstart[b], n = vstart[b + 1] - v0, q = qidx ? qidx[b] : 0;
    return (int64_t)v0 + (q < 0 || n <= 0 ? 0 : (q < n ? q : n - 1));
}

__global__ __launch_bounds__(256) void query_sub_kernel(float* __restrict__ x, const float* __restrict__ rgb,
                                                        const float* __restrict__ pos, const float* __restrict__ qtok,
                                                        const int32_t* __restrict__ qidx, const int32_t* __restrict__ vstart,
                                                        int B, int T, int P, int dim) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)B * P * dim;
    if (t >= total) return;
    const int d = (int)(t % dim), tok = (int)((t / dim) % P);
    const int b = (int)(t / ((int64_t)dim * P));
    const int64_t row = query_view_of(vstart, qidx, b, T) * P + tok;
    // betr.py:288-290 + :367,399:  (query + rgb) + pos  -- same association order as the reference
    x[row * dim + d] = (qtok[d] + rgb[row * dim + d]) + pos[tok * dim + d];
}

template <class T, int NS>
__global__ __launch_bounds__(256) void gather_query_kernel(const float* __restrict__ x, const int32_t* __restrict__ qidx,
                                                           const int32_t* __restrict__ vstart, void* __restrict__ out_, int64_t plane,
                                                           int B, int T_, int P, int dim) {
    bd_saturating_conversions();      // fp8 / f16 results saturate (bd_common.h: RANGE)
    T* out = (T*)out_;
    const int cpr = dim / 8;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)B * P * cpr;
    if (t >= total) return;
    const int c = (int)(t % cpr), tok = (int)((t / cpr) % P);
    const int b = (int)(t / ((int64_t)cpr * P));
    const float* src = x + (query_view_of(vstart, qidx, b, T_) * P + tok) * dim + c * 8;
    const float4 a = *(const float4*)src, bb = *(const float4*)(src + 4);
    const float v[8] = {a.x, a.y, a.z, a.w, bb.x, bb.y, bb.z, bb.w};
    store_operand8<T, NS>(out, plane, ((int64_t)b * P + tok) * dim + c * 8, v);
}

__global__ __launch_bounds__(256) void gather_rows_f32_kernel(const float* __restrict__ x, const int32_t* __restrict__ qidx,
                                                              const int32_t* __restrict__ vstart, float* __restrict__ out, int B, int T_,
                                                              int P, int dim) {
    const int cpr = dim / 4;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)B * P * cpr;
    if (t >= total) return;
    const int c = (int)(t % cpr), tok = (int)((t / cpr) % P);
    const int b = (int)(t / ((int64_t)cpr * P));
    *(float4*)(out + ((int64_t)b * P + tok) * dim + c * 4) =
        *(const float4*)(x + (query_view_of(vstart, qidx, b, T_) * P + tok) * dim + c * 4);
}

// one thread per output pixel (b, y, x): reads the pixel's 8 consecutive channel features, writes 8 planes
__global__ __launch_bounds__(256) void unpatchify_kernel(const float* __restrict__ proj, float* __restrict__ logits,
                                                         float* __restrict__ heat, int B, int size, int patch) {
    const int grid = size / patch, F = patch * patch * 8;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)B * size * size;
    if (t >= total) return;
    const int x = (int)(t % size), y = (int)((t / size) % size);
    const int64_t b = t / ((int64_t)size * size);
    const int gx = x / patch, px = x % patch, gy = y / patch, py = y % patch;
    const float* src = proj + (b * grid * grid + gy * grid + gx) * F + (py * patch + px) * 8;
    const float4 a = *(const float4*)src, c = *(const float4*)(src + 4);
    const float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) {
        const int64_t o = ((b * 8 + ch) * size + y) * size + x;
        if (logits) logits[o] = v[ch];
        if (heat) heat[o] = 2.0f * (1.0f / (1.0f + expf(-v[ch]))) - 1.0f;   // betr.py:432-435
    }
}


// Corner heatmap rendering -- the dataset-side producer of `bbox_feat` ("next" row f2):
// make_bbox_features(type='heatmap'), src/datasets/utils/base/bbox_utils.py:263-303.
// corners [groups*group, 8, 2] pixel (x, y) -> out [groups*group, 8, H, W] in [-1, 1].
// v = exp(-dist / (dist_to_centroid/10)^2); divided by the max over the whole call-group for that corner index
// (the reference's bbox_map[..., i].max() spans all views of the sample); then 2v - 1.  The max is the value at the
// pixel nearest to the corner (exp(-d/s) is monotone in d), so it is evaluated analytically with the SAME arithmetic
// instead of a reduction over H*W pixels.
__device__ __forceinline__ float corner_value(float bx, float by, float px, float py, float scale) {
    const float dx = bx - px, dy = by - py;
    const float d = sqrtf(dx * dx + dy * dy);
    return expf(-d / scale);
}

__global__ __launch_bounds__(256) void render_heat_kernel(const float* __restrict__ corners, int group, int H, int W,
                                                          void* __restrict__ out, int out_dtype) {
    __shared__ float s_max;
    const int map = blockIdx.y;                       // (view, corner)
    const int view = map >> 3, ci = map & 7;
    const int g0 = (view / group) * group;            // first view of this call-group
    if (threadIdx.x == 0) {
        float gmax = -INFINITY;
        for (int v = g0; v < g0 + group; ++v) {
            const float* c = corners + (int64_t)v * 16;
            float cx = 0.f, cy = 0.f;
            for (int k = 0; k < 8; ++k) { cx += c[2 * k]; cy += c[2 * k + 1]; }
            cx /= 8.0f; cy /= 8.0f;                   // bbox.mean(dim=1)
            const float bx = c[2 * ci], by = c[2 * ci + 1];
            const float ex = cx - bx, ey = cy - by;
            const float dis = sqrtf(ex * ex + ey * ey);
            const float sc = (dis / 10.0f) * (dis / 10.0f);
            const float nx = fminf(fmaxf(rintf(bx), 0.f), (float)(W - 1));
            const float ny = fminf(fmaxf(rintf(by), 0.f), (float)(H - 1));
            float best = corner_value(bx, by, nx, ny, sc);
            // rint ties / clamping: also probe the 4 neighbours so the true arg-min pixel is always covered
            const float ox[4] = {-1.f, 1.f, 0.f, 0.f}, oy[4] = {0.f, 0.f, -1.f, 1.f};
            for (int k = 0; k < 4; ++k) {
                const float qx = nx + ox[k], qy = ny + oy[k];
                if (qx >= 0.f && qx <= (float)(W - 1) && qy >= 0.f && qy <= (float)(H - 1))
                    best = fmaxf(best, corner_value(bx, by, qx, qy, sc));
            }
            gmax = fmaxf(gmax, best);
        }
        s_max = gmax;
    }
    __syncthreads();
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * W) return;
    const float* c = corners + (int64_t)view * 16;
    float cx = 0.f, cy = 0.f;
    for (int k = 0; k < 8; ++k) { cx += c[2 * k]; cy += c[2 * k + 1]; }
    cx /= 8.0f; cy /= 8.0f;
    const float bx = c[2 * ci], by = c[2 * ci + 1];
    const float ex = cx - bx, ey = cy - by;
    const float dis = sqrtf(ex * ex + ey * ey);
    const float sc = (dis / 10.0f) * (dis / 10.0f);
    const float v = corner_value(bx, by, (float)(pix % W), (float)(pix / W), sc) / s_max * 2.0f - 1.0f;
    const int64_t o = (int64_t)map * H * W + pix;
    if (out_dtype == BD_DTYPE_F32) ((float*)out)[o] = v;
    else if (out_dtype == BD_DTYPE_BF16) ((__bf16*)out)[o] = (__bf16)v;
    else ((_Float16*)out)[o] = (_Float16)v;
}

// ---------------------------------------------------------------- segmented copy of whole views between operand tensors (bd_gather_view_rows)
// A view is up to three contiguous byte runs ("segments"): plane 0, plane 1 (the split classes' second 16-bit plane, or F16C8's one-byte
// lo8 plane, packed view after view at the head of plane-1 storage) and the optional fp32 copy.  Each run is a whole number of 16-byte
// chunks (the host checks P * dim % 16 == 0 and the alignment of every base), so the kernel moves nothing but 16-byte vectors and never
// looks at an element: NaN payloads and e4m3 bytes pass through as they are.  The grid is (view, block of GATHER_PER_WG chunks of the
// view's concatenated runs); src[view] is uniform over the workgroup (one scalar load), an entry outside its table ends the workgroup
// before it touches memory.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int GATHER_UNROLL = 4, GATHER_PER_WG = 256 * GATHER_UNROLL;

struct GatherSeg {
    const char* bank;      // view v of the segment starts at base + v * view_bytes, in all three tensors
    const char* fresh;
    char* out;
    int64_t view_bytes;    // 0: segment absent
};
struct GatherViewArgs {
    GatherSeg seg[3];
    const int32_t* src;
    int bank_views, n_fresh;
    unsigned blocks_per_view;
};

__global__ __launch_bounds__(256) void gather_view_rows_kernel(const GatherViewArgs a) {
    const unsigned view = blockIdx.x / a.blocks_per_view, blk = blockIdx.x - view * a.blocks_per_view;
    const int s = a.src[view];
    const bool fresh = s < 0;
    const int64_t sv = fresh ? -(int64_t)s - 1 : (int64_t)s;
    if (sv >= (int64_t)(fresh ? a.n_fresh : a.bank_views)) return;       // inconsistent entry: the view's output stays untouched
    u32x4 v[GATHER_UNROLL];
    char* dst[GATHER_UNROLL];
#pragma unroll
    for (int i = 0; i < GATHER_UNROLL; ++i) {
        int64_t off = ((int64_t)blk * GATHER_PER_WG + i * 256 + threadIdx.x) * 16;
        dst[i] = nullptr;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int64_t vb = a.seg[k].view_bytes;
            if (!dst[i] && off >= 0) {
                if (off < vb) {
                    v[i] = *(const u32x4*)((fresh ? a.seg[k].fresh : a.seg[k].bank) + sv * vb + off);
                    dst[i] = a.seg[k].out + (int64_t)view * vb + off;
                }
                off -= vb;        // (negative from here on: the chunk belonged to segment k)
            }
        }
    }
#pragma unroll
    for (int i = 0; i < GATHER_UNROLL; ++i)
        if (dst[i]) *(u32x4*)dst[i] = v[i];
}

// ---------------------------------------------------------------- decoder-entry token rows of a batch from a bank (bd_assemble_entry_tokens)
// gather_view_rows_kernel's shape on ONE fp32 run per view: the grid is (view, block of GATHER_PER_WG 16-byte chunks), src[view] is
// uniform over the workgroup, an entry outside its table ends the workgroup before it touches memory.  A banked view is moved as bits;
// a fresh view is the query view: (query_token + rgb) + pos, query_sub_kernel's association order (no product: nothing to contract).
struct AssembleArgs {
    const float* bank;       // [bank_views, view_elems]
    const float* rgb;        // [n_fresh, view_elems]
    const float* pos;        // [view_elems]
    const float* qtok;       // [dim]
    const int32_t* src;
    float* out;              // [n_views, view_elems]
    int64_t view_elems;      // P * dim, a multiple of 4
    int dim, bank_views, n_fresh;
    int fresh_first;         // rgb holds the fresh views [fresh_first, fresh_first + n_fresh) of the table's numbering (a sub-batch lane's own)
    unsigned blocks_per_view;
};

__global__ __launch_bounds__(256) void assemble_entry_tokens_kernel(const AssembleArgs a) {
    const unsigned view = blockIdx.x / a.blocks_per_view, blk = blockIdx.x - view * a.blocks_per_view;
    const int s = a.src[view];
    const bool fresh = s < 0;
    const int64_t sv = fresh ? -(int64_t)s - 1 - a.fresh_first : (int64_t)s;
    if (sv < 0 || sv >= (int64_t)(fresh ? a.n_fresh : a.bank_views)) return;       // inconsistent entry: the view's output stays untouched
    const float* from = (fresh ? a.rgb : a.bank) + sv * a.view_elems;
    float* to = a.out + (int64_t)view * a.view_elems;
    u32x4 v[GATHER_UNROLL];
    int64_t e[GATHER_UNROLL];
#pragma unroll
    for (int i = 0; i < GATHER_UNROLL; ++i) {
        e[i] = ((int64_t)blk * GATHER_PER_WG + i * 256 + threadIdx.x) * 4;
        if (e[i] < a.view_elems) v[i] = *(const u32x4*)(from + e[i]);
    }
#pragma unroll
    for (int i = 0; i < GATHER_UNROLL; ++i) {
        if (e[i] >= a.view_elems) continue;
        if (fresh) {
            const float4 p = *(const float4*)(a.pos + e[i]);
            const float rr[4] = {__uint_as_float(v[i].x), __uint_as_float(v[i].y), __uint_as_float(v[i].z), __uint_as_float(v[i].w)};
            const float pp[4] = {p.x, p.y, p.z, p.w};
            float o[4];
            int d = (int)(e[i] % a.dim);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = (a.qtok[d] + rr[j]) + pp[j];
                if (++d == a.dim) d = 0;
            }
            *(float4*)(to + e[i]) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
            *(u32x4*)(to + e[i]) = v[i];
        }
    }
}

inline unsigned nblk(int64_t total) { return (unsigned)((total + 255) / 256); }

}  // namespace

#define BD_PREC_SWITCH(FN, ...)                                                        \
    switch (prec) {                                                                    \
        case BD_PREC_BF16: hipLaunchKernelGGL((FN<__bf16, 1>), __VA_ARGS__); break;    \
        case BD_PREC_F16: hipLaunchKernelGGL((FN<_Float16, 1>), __VA_ARGS__); break;   \
        case BD_PREC_BF16X3: hipLaunchKernelGGL((FN<__bf16, 2>), __VA_ARGS__); break;  \
        case BD_PREC_F16X3: hipLaunchKernelGGL((FN<_Float16, 2>), __VA_ARGS__); break; \
        case BD_PREC_FP8: hipLaunchKernelGGL((FN<fp8e4, 1>), __VA_ARGS__); break;      \
        case BD_PREC_F16C8: hipLaunchKernelGGL((FN<f16c8, 2>), __VA_ARGS__); break;    \
        default: return BD_ERR_DTYPE;                                                  \
    }

extern "C" int bd_im2col_images(const void* images, int img_dtype, void* out16, int64_t out_plane, int n_images,
                                int size, int patch, int kpad, int prec, void* stream) {
    if (!images || !out16) return BD_ERR_NULL;
    if (n_images <= 0 || size % patch || kpad % 8 || kpad < 3 * patch * patch) return BD_ERR_SHAPE;
    if (img_dtype < 0 || img_dtype > 2) return BD_ERR_DTYPE;
    const int grid = size / patch;
    const int64_t total = (int64_t)n_images * grid * grid * (kpad / 8);
    hipStream_t s = (hipStream_t)stream;
    // (4-byte input pieces: even image width and an aligned base)
    if (patch == P14 && size % 2 == 0 && ((uintptr_t)images & 7) == 0) {
        const int nsb = (grid + STRIP - 1) / STRIP;
        BD_PREC_SWITCH(im2col_strip_kernel, dim3((unsigned)((int64_t)n_images * grid * nsb)), dim3(256), 0, s, images, img_dtype, out16,
                       out_plane, n_images, size, kpad)
    } else {
        BD_PREC_SWITCH(im2col_kernel, dim3(nblk(total)), dim3(256), 0, s, images, img_dtype, out16, out_plane,
                       n_images, size, patch, kpad)
    }
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_patchify_heatmaps(const void* heat, int in_dtype, void* out16, int64_t out_plane, int n_images,
                                    int channels, int size, int patch, int kpad, int prec, void* stream) {
    if (!heat || !out16) return BD_ERR_NULL;
    if (channels != 8 || n_images <= 0 || size % patch || kpad % 8 || kpad < patch * patch * 8) return BD_ERR_SHAPE;
    if (in_dtype < 0 || in_dtype > 2) return BD_ERR_DTYPE;
    const int grid = size / patch;
    const int64_t total = (int64_t)n_images * grid * grid * (kpad / 8);
    hipStream_t s = (hipStream_t)stream;
    if (patch == P14 && size % 2 == 0 && ((uintptr_t)heat & 7) == 0) {
        BD_PREC_SWITCH(patchify_pair_kernel, dim3(nblk((int64_t)n_images * size * (size / 2))), dim3(256), 0, s, heat, in_dtype, out16,
                       out_plane, n_images, size, kpad)
    } else {
        BD_PREC_SWITCH(patchify_kernel, dim3(nblk(total)), dim3(256), 0, s, heat, in_dtype, out16, out_plane,
                       n_images, size, patch, kpad)
    }
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_write_prefix_tokens(float* x, const float* prefix, int n_images, int tokens_per_image,
                                      int n_prefix, int dim, void* stream) {
    if (!x || !prefix) return BD_ERR_NULL;
    if (n_images <= 0 || n_prefix <= 0 || n_prefix > tokens_per_image || dim <= 0) return BD_ERR_SHAPE;
    const int64_t total = (int64_t)n_images * n_prefix * dim;
    hipLaunchKernelGGL(prefix_kernel, dim3(nblk(total)), dim3(256), 0, (hipStream_t)stream, x, prefix, n_images,
                       tokens_per_image, n_prefix, dim);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_query_substitute(float* x, const float* rgb, const float* pos, const float* query_token,
                                   const int32_t* query_idx, int B, int T, int P, int dim, void* stream) {
    if (!x || !rgb || !pos || !query_token || !query_idx) return BD_ERR_NULL;
    if (B <= 0 || T <= 0 || P <= 0 || dim <= 0) return BD_ERR_SHAPE;
    const int64_t total = (int64_t)B * P * dim;
    hipLaunchKernelGGL(query_sub_kernel, dim3(nblk(total)), dim3(256), 0, (hipStream_t)stream, x, rgb, pos,
                       query_token, query_idx, (const int32_t*)nullptr, B, T, P, dim);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_query_substitute_varlen(float* x, const float* rgb, const float* pos, const float* query_token,
                                          const int32_t* view_start, const int32_t* query_view, int B, int P, int dim, void* stream) {
    if (!x || !rgb || !pos || !query_token || !view_start || !query_view) return BD_ERR_NULL;
    if (B <= 0 || P <= 0 || dim <= 0) return BD_ERR_SHAPE;
    const int64_t total = (int64_t)B * P * dim;
    hipLaunchKernelGGL(query_sub_kernel, dim3(nblk(total)), dim3(256), 0, (hipStream_t)stream, x, rgb, pos,
                       query_token, query_view, view_start, B, 0, P, dim);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_gather_query_rows_f32(const float* x, const int32_t* query_idx, float* out, int B, int T, int P,
                                        int dim, void* stream) {
    if (!x || !query_idx || !out) return BD_ERR_NULL;
    if (B <= 0 || T <= 0 || P <= 0 || dim % 4) return BD_ERR_SHAPE;
    const int64_t total = (int64_t)B * P * (dim / 4);
    hipLaunchKernelGGL(gather_rows_f32_kernel, dim3(nblk(total)), dim3(256), 0, (hipStream_t)stream, x, query_idx,
                       (const int32_t*)nullptr, out, B, T, P, dim);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_gather_query_rows_f32_varlen(const float* x, const int32_t* view_start, const int32_t* query_view, float* out, int B,
                                               int P, int dim, void* stream) {
    if (!x || !view_start || !query_view || !out) return BD_ERR_NULL;
    if (B <= 0 || P <= 0 || dim <= 0 || dim % 4) return BD_ERR_SHAPE;
    const int64_t total = (int64_t)B * P * (dim / 4);
    hipLaunchKernelGGL(gather_rows_f32_kernel, dim3(nblk(total)), dim3(256), 0, (hipStream_t)stream, x, query_view, view_start, out,
                       B, 0, P, dim);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_gather_query_tokens(const float* x, const int32_t* query_idx, void* out16, int64_t out_plane,
                                      int B, int T, int P, int dim, int prec, void* stream) {
    if (!x || !out16) return BD_ERR_NULL;                   /* query_idx == NULL: view 0 (x already compact) */
    if (B <= 0 || T <= 0 || P <= 0 || dim % 8) return BD_ERR_SHAPE;
    const int64_t total = (int64_t)B * P * (dim / 8);
    hipStream_t s = (hipStream_t)stream;
    BD_PREC_SWITCH(gather_query_kernel, dim3(nblk(total)), dim3(256), 0, s, x, query_idx, (const int32_t*)nullptr, out16, out_plane, B, T, P, dim)
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_gather_query_tokens_varlen(const float* x, const int32_t* view_start, const int32_t* query_view, void* out16,
                                             int64_t out_plane, int B, int P, int dim, int prec, void* stream) {
    if (!x || !view_start || !query_view || !out16) return BD_ERR_NULL;
    if (B <= 0 || P <= 0 || dim <= 0 || dim % 8) return BD_ERR_SHAPE;
    const int64_t total = (int64_t)B * P * (dim / 8);
    hipStream_t s = (hipStream_t)stream;
    BD_PREC_SWITCH(gather_query_kernel, dim3(nblk(total)), dim3(256), 0, s, x, query_view, view_start, out16, out_plane, B, 0, P, dim)
    BD_CHECK_LAUNCH();
    return BD_OK;
}

// Assembles the decoder's feature operand of one batch from cached views (a device-resident bank) and the views encoded in this
// forward -- what replaces running the references through the encoder again for every query (the reference model does:
// BoxDreamerModel.py:274-285).  See include/boxdreamer_hip.h.
extern "C" int bd_gather_view_rows(const void* bank16, int64_t bank_plane, int bank_views, const void* fresh16, int64_t fresh_plane,
                                   int n_fresh, const int32_t* src, void* out16, int64_t out_plane, int n_views, int P, int dim,
                                   int prec, const float* bank32, const float* fresh32, float* out32, void* stream) {
    if (!src || !out16 || (bank_views > 0 && !bank16) || (n_fresh > 0 && !fresh16)) return BD_ERR_NULL;
    if (out32 && ((bank_views > 0 && !bank32) || (n_fresh > 0 && !fresh32))) return BD_ERR_NULL;
    if (bank_views < 0 || n_fresh < 0 || n_views < 0 || P <= 0 || dim <= 0) return BD_ERR_SHAPE;
    int esz, plane1;          // bytes per element of plane 0; of plane 1 (0: one plane)
    switch (prec) {
        case BD_PREC_BF16: case BD_PREC_F16: esz = 2; plane1 = 0; break;
        case BD_PREC_FP8: esz = 1; plane1 = 0; break;
        case BD_PREC_BF16X3: case BD_PREC_F16X3: esz = 2; plane1 = 2; break;
        case BD_PREC_F16C8: esz = 2; plane1 = 1; break;
        default: return BD_ERR_DTYPE;
    }
    const int64_t elems = (int64_t)P * dim;
    if (elems % 16) return BD_ERR_ALIGN;
    const auto misaligned = [](const void* p) { return ((uintptr_t)p & 15) != 0; };
    if (misaligned(bank16) || misaligned(fresh16) || misaligned(out16) || ((uintptr_t)src & 3)) return BD_ERR_ALIGN;
    if (out32 && (misaligned(bank32) || misaligned(fresh32) || misaligned(out32))) return BD_ERR_ALIGN;
    if (plane1) {             // plane offsets count 16-bit elements: 16-byte aligned planes, and no overlap with plane 0
        if (bank_plane % 8 || fresh_plane % 8 || out_plane % 8) return BD_ERR_ALIGN;
        if ((bank_views > 0 && bank_plane < elems * bank_views) || (n_fresh > 0 && fresh_plane < elems * n_fresh) || out_plane < elems * n_views)
            return BD_ERR_SHAPE;
    }
    // out must not overlap a source: a view copied early would be read back as another view's source.  Byte extents over all planes
    const auto extent = [&](int64_t plane, int views) { return plane1 ? plane * 2 + elems * plane1 * views : elems * esz * views; };
    const auto overlap = [](const void* p, int64_t np, const void* q, int64_t nq) {
        return np > 0 && nq > 0 && (uintptr_t)p < (uintptr_t)q + (uintptr_t)nq && (uintptr_t)q < (uintptr_t)p + (uintptr_t)np;
    };
    const int64_t out_bytes = extent(out_plane, n_views);
    if (overlap(out16, out_bytes, bank16, extent(bank_plane, bank_views)) || overlap(out16, out_bytes, fresh16, extent(fresh_plane, n_fresh)))
        return BD_ERR_SHAPE;
    if (out32 && (overlap(out32, elems * 4 * n_views, bank32, elems * 4 * bank_views) || overlap(out32, elems * 4 * n_views, fresh32, elems * 4 * n_fresh)))
        return BD_ERR_SHAPE;
    if (n_views == 0) return BD_OK;
    GatherViewArgs a{};
    a.seg[0] = {(const char*)bank16, (const char*)fresh16, (char*)out16, elems * esz};
    if (plane1)
        a.seg[1] = {(const char*)bank16 + bank_plane * 2, (const char*)fresh16 + fresh_plane * 2, (char*)out16 + out_plane * 2, elems * plane1};
    if (out32) a.seg[2] = {(const char*)bank32, (const char*)fresh32, (char*)out32, elems * 4};
    a.src = src;
    a.bank_views = bank_views;
    a.n_fresh = n_fresh;
    const int64_t view_chunks = (a.seg[0].view_bytes + a.seg[1].view_bytes + a.seg[2].view_bytes) / 16;
    const int64_t bpv = (view_chunks + GATHER_PER_WG - 1) / GATHER_PER_WG;
    if (bpv * n_views > 0x7fffffffLL) return BD_ERR_SHAPE;
    a.blocks_per_view = (unsigned)bpv;
    hipLaunchKernelGGL(gather_view_rows_kernel, dim3((unsigned)(bpv * n_views)), dim3(256), 0, (hipStream_t)stream, a);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

// The decoder's entry token rows of one batch from banked reference rows and the query views' adapter output -- what replaces
// patchifying and embedding every reference's heat maps again for every query (betr.py:313-329, :367-399).  See include/boxdreamer_hip.h.
int bd_assemble_entry_tokens_from(const float* bank_x, int bank_views, const float* rgb_fresh, int fresh_first, int n_fresh, const float* pos,
                                  const float* query_token, const int32_t* src, float* x_out, int n_views, int P, int dim, void* stream) {
    if (!src || !x_out || !pos || !query_token || (bank_views > 0 && !bank_x) || (n_fresh > 0 && !rgb_fresh)) return BD_ERR_NULL;
    if (bank_views < 0 || fresh_first < 0 || n_fresh < 0 || n_views < 0 || P <= 0 || dim <= 0) return BD_ERR_SHAPE;
    const int64_t elems = (int64_t)P * dim;
    if (elems % 4) return BD_ERR_ALIGN;
    const auto misaligned = [](const void* p) { return ((uintptr_t)p & 15) != 0; };
    if (misaligned(bank_x) || misaligned(rgb_fresh) || misaligned(pos) || misaligned(query_token) || misaligned(x_out) || ((uintptr_t)src & 3))
        return BD_ERR_ALIGN;
    // x_out must not overlap an input: a view written early would be read back as another view's source
    const auto overlap = [&](const void* q, int64_t nq) {
        const int64_t np = elems * 4 * n_views;
        return np > 0 && nq > 0 && (uintptr_t)x_out < (uintptr_t)q + (uintptr_t)nq && (uintptr_t)q < (uintptr_t)x_out + (uintptr_t)np;
    };
    if (overlap(bank_x, elems * 4 * bank_views) || overlap(rgb_fresh, elems * 4 * n_fresh) || overlap(pos, elems * 4) ||
        overlap(query_token, (int64_t)dim * 4) || overlap(src, (int64_t)n_views * 4))
        return BD_ERR_SHAPE;
    if (n_views == 0) return BD_OK;
    const int64_t bpv = (elems / 4 + GATHER_PER_WG - 1) / GATHER_PER_WG;
    if (bpv * n_views > 0x7fffffffLL) return BD_ERR_SHAPE;
    AssembleArgs a{};
    a.bank = bank_x; a.rgb = rgb_fresh; a.pos = pos; a.qtok = query_token; a.src = src; a.out = x_out;
    a.view_elems = elems; a.dim = dim; a.bank_views = bank_views; a.n_fresh = n_fresh; a.fresh_first = fresh_first;
    a.blocks_per_view = (unsigned)bpv;
    hipLaunchKernelGGL(assemble_entry_tokens_kernel, dim3((unsigned)(bpv * n_views)), dim3(256), 0, (hipStream_t)stream, a);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_assemble_entry_tokens(const float* bank_x, int bank_views, const float* rgb_fresh, int n_fresh, const float* pos,
                                        const float* query_token, const int32_t* src, float* x_out, int n_views, int P, int dim,
                                        void* stream) {
    return bd_assemble_entry_tokens_from(bank_x, bank_views, rgb_fresh, 0, n_fresh, pos, query_token, src, x_out, n_views, P, dim, stream);
}

extern "C" int bd_unpatchify_sigmoid(const float* proj, float* logits, float* heat, int B, int channels, int size,
                                     int patch, void* stream) {
    if (!proj || (!logits && !heat)) return BD_ERR_NULL;
    if (channels != 8 || B <= 0 || size % patch) return BD_ERR_SHAPE;
    const int64_t total = (int64_t)B * size * size;
    hipLaunchKernelGGL(unpatchify_kernel, dim3(nblk(total)), dim3(256), 0, (hipStream_t)stream, proj, logits, heat,
                       B, size, patch);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_render_corner_heatmaps(const float* corners, int n_groups, int group, int height, int width,
                                         void* out, int out_dtype, void* stream) {
    if (!corners || !out) return BD_ERR_NULL;
    if (n_groups <= 0 || group <= 0 || height <= 0 || width <= 0) return BD_ERR_SHAPE;
    if (out_dtype < 0 || out_dtype > 2) return BD_ERR_DTYPE;
    const dim3 grid((unsigned)((height * width + 255) / 256), (unsigned)(n_groups * group * 8));
    hipLaunchKernelGGL(render_heat_kernel, grid, dim3(256), 0, (hipStream_t)stream, corners, group, height, width, out,
                       out_dtype);
    BD_CHECK_LAUNCH();
    return BD_OK;
}
