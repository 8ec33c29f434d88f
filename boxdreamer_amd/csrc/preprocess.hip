// Crop + ToTensor + antialiased bilinear resize of raw uint8 HWC frames on the device: what the reference's dataset does per view on
// the host (src/datasets/utils/preprocess.py:123-199 pad_and_resize_image, :202-274 _crop_image; called from
// src/datasets/base.py:541-566), written where the encoder reads it.
//
// The filter is ATen's _upsample_bilinear2d_aa (align_corners = false) on the zero-padded integer crop: separable triangle filter,
// scale = s / S, support = max(scale, 1), centre c_i = scale (i + 0.5), taps [max(0, int(c_i - support + 0.5)), min(s, int(c_i + support
// + 0.5))), weight max(0, 1 - |j - c_i + 0.5| / support), normalised per output sample.  The tap geometry and the weights are evaluated
// in fp64 from the integer box (the reference's fp32 centres drift by ~3e-5 px at the far edge); the weights are rounded to fp32 once,
// the sums are sequential fp32 in ascending tap order.  `value / 255` is applied once per output sample (sum of w * byte, then one
// correctly rounded division): for a single tap of weight 1 that is bit-identical to ToTensor, otherwise within an fp32 rounding of it.
//
// One workgroup (256 threads) owns a band of R output rows of one crop (R follows out_size only: boxes are device data, so nothing on
// the host may depend on a crop's scale).  It walks the source rows the band needs in chunks:
//   1. stage   -- the chunk's source rows, clipped to the valid rectangle (crop ^ frame ^ keep box), are read as ALIGNED dwords (4 pixels
//                 = 3 dwords per lane, the unaligned head handled with v_alignbyte, the tail by not loading dwords without a valid byte)
//                 and written to LDS as one dword per pixel, R | G << 8 | B << 16.  This step alone knows the source format (FMT,
//                 pixel_format.h): BGR swaps two bytes of that dword, RGBA / BGRA are one aligned dword per pixel, NV12 is four luma
//                 pixels per aligned dword plus the chroma row y >> 1, converted here -- so a crop of any format is, bit for bit, the
//                 RGB instance's crop of the converted frame, and only pixels under a crop are converted;
//   2. horizontal -- one lane per (source row, output column): one LDS dword per tap feeds the three channels (v_cvt_f32_ubyteN), the
//                 weight comes from a per-block LDS table [tap][column] (conflict-free across lanes) shared by every row and channel;
//                 the fp32 row lands in LDS [row][channel][column];
//   3. vertical -- every lane owns up to PP_MAXI groups of 4 contiguous output columns of one (row, channel) in registers and adds the
//                 chunk's rows with the per-chunk weight table [band row][chunk row].
// Whatever lies outside the valid rectangle contributes zero and is never read or visited, so a box far larger than its frame costs
// what the frame costs.  Two forms are switched per crop (uniform per workgroup, same arithmetic, same order):
//   * weights on the fly in fp64 instead of the table when out_size x (2 support + 2) exceeds PP_WTAB floats (support > ~10 at 224);
//   * source bytes straight from global memory instead of the LDS stage when one clipped row exceeds PP_RAW pixels (4096).
// Both are far outside the crops a 224 x 224 pose pipeline sees; they exist so that no box produces a wrong answer.
// Deterministic: fixed summation order, no atomics, a crop's bits depend on its own box and frame only.
#include "bd_common.h"
#include "pixel_format.h"

namespace {

constexpr int PP_THREADS = 256;
constexpr int PP_MAX_OUT = 512;                   // out_size limit: per-column tables and one hbuf row must fit
constexpr int PP_MAXI = 6;                        // groups of 4 outputs a lane may own
constexpr int PP_MAX_BAND = 8;                    // output rows per workgroup, at most
constexpr int PP_WTAB = 5120;                     // horizontal weight table, floats (20 KiB)
constexpr int PP_RAW = 4096;                      // staged pixels per chunk (16 KiB)
constexpr int PP_HBUF = 4608;                     // horizontally filtered rows, floats (18 KiB): 6 rows at out_size 224
constexpr int PP_MAX_CH = 8;                      // source rows per chunk, at most
constexpr long long PP_MAX_SIDE = 1 << 20;        // a box side above this counts as degenerate (zeros)

int pp_band(int S) {
    const int sp = (S + 3) & ~3;
    int r = PP_MAXI * PP_THREADS * 4 / (3 * sp);
    return r > PP_MAX_BAND ? PP_MAX_BAND : r;
}

struct Taps {
    long long lo, hi;     // [lo, hi) in crop pixels
    double c;             // centre
};

__device__ __forceinline__ Taps tap_range(int i, double scale, double support, long long s) {
    Taps t;
    t.c = scale * ((double)i + 0.5);
    long long lo = (long long)(t.c - support + 0.5), hi = (long long)(t.c + support + 0.5);
    t.lo = lo < 0 ? 0 : lo;
    t.hi = hi > s ? s : hi;
    return t;
}

__device__ __forceinline__ double tap_weight(long long j, double c, double support) {
    const double w = 1.0 - fabs((double)j - c + 0.5) / support;
    return w > 0.0 ? w : 0.0;
}

__device__ __forceinline__ double tap_sum(const Taps& t, double support) {
    double sum = 0.0;
    for (long long j = t.lo; j < t.hi; ++j) sum += tap_weight(j, t.c, support);
    return sum;
}

template <class T> __device__ __forceinline__ void store4(T* dst, const float (&v)[4]) { store_cvt<T, 4>(dst, v); }
template <> __device__ __forceinline__ void store4<float>(float* dst, const float (&v)[4]) {
    f32x4 o = {v[0], v[1], v[2], v[3]};
    *(f32x4*)dst = o;
}
template <class T> __device__ __forceinline__ void store1(T* dst, float v) {
    asm("" : "+v"(v));                     // fp32 first, then ONE rounding to T (bd_common.h: store_cvt)
    *dst = (T)v;
}

template <class T, int FMT>
__global__ __launch_bounds__(PP_THREADS) void crop_resize_kernel(const uint8_t* __restrict__ frames, int n_frames, int H, int W,
                                                                  int64_t row_stride, int64_t frame_stride,
                                                                  const int32_t* __restrict__ boxes, const int32_t* __restrict__ frame_idx,
                                                                  const int32_t* __restrict__ keep_boxes, int S, int R, int vec_ok,
                                                                  T* __restrict__ out, int64_t chroma_off, YuvCoef coef) {
    __shared__ __attribute__((aligned(16))) float hbuf[PP_HBUF];
    __shared__ __attribute__((aligned(16))) uint32_t raw[PP_RAW];
    __shared__ float wtab[PP_WTAB];
    __shared__ double xsum[PP_MAX_OUT];
    __shared__ int xlo[PP_MAX_OUT], xcnt[PP_MAX_OUT];
    __shared__ double ysum[PP_MAX_BAND], yc[PP_MAX_BAND];
    __shared__ long long ylo[PP_MAX_BAND], yhi[PP_MAX_BAND];
    __shared__ float wyt[PP_MAX_BAND * PP_MAX_CH];

    const int tid = threadIdx.x, crop = blockIdx.y, r0 = blockIdx.x * R;
    const int Sp = (S + 3) & ~3, S4 = Sp >> 2;
    const int nR = min(R, S - r0);
    const int32_t* bx = boxes + (int64_t)crop * 4;
    const long long x0 = bx[0], y0 = bx[1], x1 = bx[2], y1 = bx[3];
    const long long s = x1 - x0;
    const long long f = frame_idx ? (long long)frame_idx[crop] : (long long)crop;
    bool ok = s >= 1 && s <= PP_MAX_SIDE && (y1 - y0) == s && f >= 0 && f < n_frames;
    // valid rectangle: crop ^ frame ^ keep box (ImageDraw.rectangle: both edges inclusive)
    long long vx0 = max(x0, 0LL), vx1 = min(x1, (long long)W), vy0 = max(y0, 0LL), vy1 = min(y1, (long long)H);
    if (keep_boxes) {
        const int32_t* kb = keep_boxes + (int64_t)crop * 4;
        vx0 = max(vx0, (long long)kb[0]); vy0 = max(vy0, (long long)kb[1]);
        vx1 = min(vx1, (long long)kb[2] + 1); vy1 = min(vy1, (long long)kb[3] + 1);
    }
    ok = ok && vx1 > vx0 && vy1 > vy0;

    // what this lane owns of the band: group g = tid + it * 256 -> (band row, channel, 4 columns)
    float acc[PP_MAXI][4];
    int it_r[PP_MAXI], it_off[PP_MAXI];
    const int n_groups = nR * 3 * S4;
#pragma unroll
    for (int it = 0; it < PP_MAXI; ++it) {
        const int g = tid + it * PP_THREADS;
        const int r = g / (3 * S4), rem = g - r * (3 * S4), ch = rem / S4, c4 = rem - ch * S4;
        it_r[it] = g < n_groups ? r : -1;
        it_off[it] = ch * Sp + c4 * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[it][q] = 0.f;
    }

    if (ok) {
        const double scale = (double)s / (double)S, support = scale > 1.0 ? scale : 1.0;
        const int nt_bound = (int)(2.0 * support) + 2;
        const bool use_tab = (long long)S * nt_bound <= PP_WTAB;
        const int nvx = (int)(vx1 - vx0);                       // <= W
        const int units = (nvx + 3) >> 2, rawpitch = units * 4;
        const bool direct = rawpitch > PP_RAW;
        int CH = min(PP_MAX_CH, PP_HBUF / (3 * Sp));
        if (!direct) CH = min(CH, PP_RAW / rawpitch);
        const uint8_t* fbase = frames + f * frame_stride;

        // per-column taps (shared by every source row and channel) and per-band-row taps
        for (int i = tid; i < S; i += PP_THREADS) {
            const Taps t = tap_range(i, scale, support, s);
            const double sum = tap_sum(t, support);
            xlo[i] = (int)t.lo;
            xcnt[i] = (int)(t.hi - t.lo);
            xsum[i] = sum;
            if (use_tab)
                for (long long j = t.lo; j < t.hi; ++j) wtab[(int)(j - t.lo) * S + i] = (float)(tap_weight(j, t.c, support) / sum);
        }
        if (tid < nR) {
            const Taps t = tap_range(r0 + tid, scale, support, s);
            ylo[tid] = t.lo; yhi[tid] = t.hi; yc[tid] = t.c;
            ysum[tid] = tap_sum(t, support);
        }
        __syncthreads();
        const long long j_begin = max(ylo[0], vy0 - y0), j_end = min(yhi[nR - 1], vy1 - y0);
        const long long xoff = x0 - vx0;                        // crop pixel j sits at staged pixel j + xoff

        for (long long jc = j_begin; jc < j_end; jc += CH) {
            const int nrows = (int)min((long long)CH, j_end - jc);
            // 1. stage: aligned dwords, 4 pixels per lane and step; the one place where the source format shows
            if (!direct) {
                for (int e = tid; e < nrows * units; e += PP_THREADS) {
                    const int k = e / units, u = e - k * units;
                    const long long yrow = y0 + jc + k;
                    u128 px;
                    if constexpr (FMT == PF_RGB || FMT == PF_BGR) {
                        const uint8_t* rp = fbase + yrow * row_stride + vx0 * 3;
                        const unsigned a = (unsigned)((uintptr_t)rp & 3);
                        const uint32_t* ap = (const uint32_t*)(rp - a);
                        const int ndw = (int)((a + (unsigned)nvx * 3u + 3u) >> 2);      // dwords that hold at least one valid byte
                        uint32_t d[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) d[q] = (3 * u + q < ndw) ? ap[3 * u + q] : 0u;
                        const uint32_t b0 = __builtin_amdgcn_alignbyte(d[1], d[0], a), b1 = __builtin_amdgcn_alignbyte(d[2], d[1], a),
                                       b2 = __builtin_amdgcn_alignbyte(d[3], d[2], a);
                        px = u128{b0 & 0xffffffu, (b0 >> 24) | ((b1 & 0xffffu) << 8), (b1 >> 16) | ((b2 & 0xffu) << 16), b2 >> 8};
                        if constexpr (FMT == PF_BGR) {
#pragma unroll
                            for (int q = 0; q < 4; ++q) px[q] = pf_swap_rb(px[q]);
                        }
                    } else if constexpr (FMT == PF_RGBA || FMT == PF_BGRA) {
                        // one dword per pixel; a base or stride off dword alignment makes it two halves of neighbouring dwords
                        const uint8_t* rp = fbase + yrow * row_stride + vx0 * 4;
                        const unsigned a = (unsigned)((uintptr_t)rp & 3);
                        const uint32_t* ap = (const uint32_t*)(rp - a);
                        const int ndw = (int)((a + (unsigned)nvx * 4u + 3u) >> 2);
                        uint32_t d[5];
#pragma unroll
                        for (int q = 0; q < 5; ++q) d[q] = (4 * u + q < ndw) ? ap[4 * u + q] : 0u;
#pragma unroll
                        for (int q = 0; q < 4; ++q) px[q] = pf_packed_px<FMT>(__builtin_amdgcn_alignbyte(d[q + 1], d[q], a));
                    } else {
                        // NV12: four luma bytes are one dword; their chroma is bytes [4 u, 4 u + 4) of row yrow >> 1 counted from the
                        // pair of the first valid pixel -- two more when that pixel is the second of its pair (vx0 odd)
                        const uint8_t* rp = fbase + yrow * row_stride + vx0;
                        const unsigned a = (unsigned)((uintptr_t)rp & 3);
                        const uint32_t* ap = (const uint32_t*)(rp - a);
                        const int ndw = (int)((a + (unsigned)nvx + 3u) >> 2);
                        const uint32_t l0 = u < ndw ? ap[u] : 0u, l1 = u + 1 < ndw ? ap[u + 1] : 0u;
                        const uint32_t yy = __builtin_amdgcn_alignbyte(l1, l0, a);
                        const unsigned odd = (unsigned)(vx0 & 1);
                        const uint8_t* cp = fbase + chroma_off + (yrow >> 1) * row_stride + (vx0 & ~1LL);
                        const unsigned ca = (unsigned)((uintptr_t)cp & 3);
                        const uint32_t* cap = (const uint32_t*)(cp - ca);
                        const unsigned ncb = (unsigned)((((vx1 - 1) & ~1LL) + 2) - (vx0 & ~1LL));    // chroma bytes under the valid row
                        const int ncdw = (int)((ca + ncb + 3u) >> 2);
                        const uint32_t e0 = u < ncdw ? cap[u] : 0u, e1 = u + 1 < ncdw ? cap[u + 1] : 0u,
                                       e2 = (u + 2 < ncdw && ca + 4u + 2u * odd > 8u) ? cap[u + 2] : 0u;
                        const uint64_t c = (uint64_t)__builtin_amdgcn_alignbyte(e1, e0, ca) |
                                           ((uint64_t)__builtin_amdgcn_alignbyte(e2, e1, ca) << 32);
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const uint32_t uv = (uint32_t)(c >> (16u * ((odd + (unsigned)q) >> 1)));
                            px[q] = pf_yuv_px((int)((yy >> (8 * q)) & 0xffu), (int)(uv & 0xffu), (int)((uv >> 8) & 0xffu), coef);
                        }
                    }
                    *(u128*)&raw[k * rawpitch + u * 4] = px;
                }
            }
            if (tid < nR * CH) {
                const int r = tid / CH, k = tid - r * CH;
                const long long j = jc + k;
                float w = 0.f;
                if (k < nrows && j >= ylo[r] && j < yhi[r]) w = (float)(tap_weight(j, yc[r], support) / ysum[r]);
                wyt[r * PP_MAX_CH + k] = w;
            }
            __syncthreads();
            // 2. horizontal: (chunk row, output column) per lane, three channels from one dword per tap
            for (int e = tid; e < nrows * S; e += PP_THREADS) {
                const int k = e / S, i = e - k * S;
                const int lo = xlo[i];
                const int t0 = (int)max(0LL, -xoff - lo), t1 = (int)min((long long)xcnt[i], (long long)nvx - xoff - lo);
                float cr = 0.f, cg = 0.f, cb = 0.f;
                if (!direct) {
                    const uint32_t* rowp = raw + k * rawpitch + (lo + xoff);
                    if (use_tab) {
                        for (int t = t0; t < t1; ++t) {
                            const float w = wtab[t * S + i];
                            const uint32_t px = rowp[t];
                            cr = fmaf(w, (float)(px & 0xffu), cr);
                            cg = fmaf(w, (float)((px >> 8) & 0xffu), cg);
                            cb = fmaf(w, (float)((px >> 16) & 0xffu), cb);
                        }
                    } else {
                        const double c = scale * ((double)i + 0.5), sum = xsum[i];
                        for (int t = t0; t < t1; ++t) {
                            const float w = (float)(tap_weight(lo + t, c, support) / sum);
                            const uint32_t px = rowp[t];
                            cr = fmaf(w, (float)(px & 0xffu), cr);
                            cg = fmaf(w, (float)((px >> 8) & 0xffu), cg);
                            cb = fmaf(w, (float)((px >> 16) & 0xffu), cb);
                        }
                    }
                } else {
                    const double c = scale * ((double)i + 0.5), sum = xsum[i];
                    for (int t = t0; t < t1; ++t) {
                        const float w = use_tab ? wtab[t * S + i] : (float)(tap_weight(lo + t, c, support) / sum);
                        const uint32_t px = pf_load_px<FMT>(fbase, row_stride, chroma_off, x0 + lo + t, y0 + jc + k, coef);
                        cr = fmaf(w, (float)(px & 0xffu), cr);
                        cg = fmaf(w, (float)((px >> 8) & 0xffu), cg);
                        cb = fmaf(w, (float)((px >> 16) & 0xffu), cb);
                    }
                }
                float* h = hbuf + k * 3 * Sp + i;
                h[0] = cr; h[Sp] = cg; h[2 * Sp] = cb;
            }
            __syncthreads();
            // 3. vertical: ascending source rows into the lane's registers
#pragma unroll
            for (int it = 0; it < PP_MAXI; ++it) {
                if (it_r[it] < 0) continue;
                for (int k = 0; k < nrows; ++k) {
                    const float w = wyt[it_r[it] * PP_MAX_CH + k];
                    if (w == 0.f) continue;
                    const f32x4 v = *(const f32x4*)&hbuf[k * 3 * Sp + it_off[it]];
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[it][q] = fmaf(w, v[q], acc[it][q]);
                }
            }
            __syncthreads();                                    // the chunk has been read: the next one may overwrite it
        }
    }

    // ToTensor's / 255 (once per sample), clamp, one rounding to T, CHW store: 4 contiguous columns of one plane per lane
#pragma unroll
    for (int it = 0; it < PP_MAXI; ++it) {
        if (it_r[it] < 0) continue;
        const int ch = it_off[it] / Sp, col = it_off[it] - ch * Sp;
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = fminf(fmaxf(acc[it][q] / 255.f, 0.f), 1.f);
        T* dst = out + (((int64_t)crop * 3 + ch) * S + (r0 + it_r[it])) * S + col;
        if (vec_ok) {
            store4<T>(dst, v);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (col + q < S) store1<T>(dst + q, v[q]);
        }
    }
}

struct Frames {
    const uint8_t* base;
    int n, H, W;
    int64_t row_stride, frame_stride, chroma_off;
    YuvCoef coef;
};

template <class T, int FMT>
void launch(const Frames& fr, const int32_t* boxes, const int32_t* frame_idx, const int32_t* keep_boxes, int n_crops, int S, void* out,
            hipStream_t s) {
    const int R = pp_band(S);
    const int vec_ok = (S % 4 == 0) && ((uintptr_t)out % 16 == 0);
    hipLaunchKernelGGL((crop_resize_kernel<T, FMT>), dim3((S + R - 1) / R, n_crops), dim3(PP_THREADS), 0, s, fr.base, fr.n, fr.H, fr.W,
                       fr.row_stride, fr.frame_stride, boxes, frame_idx, keep_boxes, S, R, vec_ok, (T*)out, fr.chroma_off, fr.coef);
}

template <int FMT>
void launch_dtype(const Frames& fr, const int32_t* boxes, const int32_t* frame_idx, const int32_t* keep_boxes, int n_crops, int S,
                  void* out, int out_dtype, hipStream_t s) {
    if (out_dtype == BD_DTYPE_F32)
        launch<float, FMT>(fr, boxes, frame_idx, keep_boxes, n_crops, S, out, s);
    else if (out_dtype == BD_DTYPE_F16)
        launch<_Float16, FMT>(fr, boxes, frame_idx, keep_boxes, n_crops, S, out, s);
    else
        launch<__bf16, FMT>(fr, boxes, frame_idx, keep_boxes, n_crops, S, out, s);
}

// what can be refused about a frame layout on the host: BD_OK, or the code both entries below and the host converter return
int check_frames(const Frames& fr, int format) {
    if (!fr.base) return BD_ERR_NULL;
    if (format < PF_RGB || format > PF_NV12) return BD_ERR_DTYPE;
    if (fr.n <= 0 || fr.H <= 0 || fr.W <= 0) return BD_ERR_SHAPE;
    if (fr.row_stride < (int64_t)pf_bytes_per_pixel(format) * fr.W || fr.frame_stride < 0) return BD_ERR_SHAPE;
    if (format == PF_NV12) {
        if ((fr.H & 1) || (fr.W & 1) || fr.chroma_off < (int64_t)fr.H * fr.row_stride) return BD_ERR_SHAPE;
        const int c[5] = {fr.coef.cy, fr.coef.crv, fr.coef.cgu, fr.coef.cgv, fr.coef.cbu};
        for (int v : c)
            if (v < 0 || v > PF_MAX_COEF) return BD_ERR_SHAPE;                  // (int32 holds every intermediate)
        if (fr.coef.y_off < 0 || fr.coef.y_off > 255) return BD_ERR_SHAPE;
    }
    return BD_OK;
}

template <int FMT>
void to_rgb_host(const Frames& fr, uint8_t* out) {
    for (int n = 0; n < fr.n; ++n)
        for (int y = 0; y < fr.H; ++y)
            for (int x = 0; x < fr.W; ++x) {
                const uint32_t px = pf_load_px<FMT>(fr.base + n * fr.frame_stride, fr.row_stride, fr.chroma_off, x, y, fr.coef);
                uint8_t* o = out + (((int64_t)n * fr.H + y) * fr.W + x) * 3;
                o[0] = (uint8_t)(px & 0xffu); o[1] = (uint8_t)((px >> 8) & 0xffu); o[2] = (uint8_t)((px >> 16) & 0xffu);
            }
}

}  // namespace

extern "C" int bd_crop_resize_frames_fmt(const uint8_t* frames, int n_frames, int H, int W, int64_t row_stride, int64_t frame_stride,
                                         const int32_t* boxes, const int32_t* frame_idx, const int32_t* keep_boxes, int n_crops,
                                         int out_size, void* out, int out_dtype, int format, int64_t chroma_offset, int cy, int crv,
                                         int cgu, int cgv, int cbu, int y_off, void* stream) {
    if (!frames || !boxes || !out) return BD_ERR_NULL;
    if (n_crops <= 0 || n_crops > 65535 || out_size <= 0 || out_size > PP_MAX_OUT) return BD_ERR_SHAPE;
    const Frames fr = {frames, n_frames, H, W, row_stride, frame_stride, chroma_offset, {cy, crv, cgu, cgv, cbu, y_off}};
    if (const int rc = check_frames(fr, format)) return rc;
    if (!frame_idx && n_crops > n_frames) return BD_ERR_SHAPE;                  // crop i reads frame i
    if (out_dtype != BD_DTYPE_F32 && out_dtype != BD_DTYPE_F16 && out_dtype != BD_DTYPE_BF16) return BD_ERR_DTYPE;
    hipStream_t s = (hipStream_t)stream;
    switch (format) {
        case PF_RGB: launch_dtype<PF_RGB>(fr, boxes, frame_idx, keep_boxes, n_crops, out_size, out, out_dtype, s); break;
        case PF_BGR: launch_dtype<PF_BGR>(fr, boxes, frame_idx, keep_boxes, n_crops, out_size, out, out_dtype, s); break;
        case PF_RGBA: launch_dtype<PF_RGBA>(fr, boxes, frame_idx, keep_boxes, n_crops, out_size, out, out_dtype, s); break;
        case PF_BGRA: launch_dtype<PF_BGRA>(fr, boxes, frame_idx, keep_boxes, n_crops, out_size, out, out_dtype, s); break;
        default: launch_dtype<PF_NV12>(fr, boxes, frame_idx, keep_boxes, n_crops, out_size, out, out_dtype, s); break;
    }
    BD_CHECK_LAUNCH();
    return BD_OK;
}

// the "rgb" case of the entry above: the same checks in the same order, the same kernel instance, the same launch
extern "C" int bd_crop_resize_frames(const uint8_t* frames, int n_frames, int H, int W, int64_t row_stride, int64_t frame_stride,
                                     const int32_t* boxes, const int32_t* frame_idx, const int32_t* keep_boxes, int n_crops,
                                     int out_size, void* out, int out_dtype, void* stream) {
    return bd_crop_resize_frames_fmt(frames, n_frames, H, W, row_stride, frame_stride, boxes, frame_idx, keep_boxes, n_crops, out_size, out,
                                     out_dtype, PF_RGB, 0, 0, 0, 0, 0, 0, 0, stream);
}

extern "C" int bd_frames_to_rgb_host(const uint8_t* frames, int n_frames, int H, int W, int64_t row_stride, int64_t frame_stride,
                                     int format, int64_t chroma_offset, int cy, int crv, int cgu, int cgv, int cbu, int y_off,
                                     uint8_t* out) {
    if (!frames || !out) return BD_ERR_NULL;
    const Frames fr = {frames, n_frames, H, W, row_stride, frame_stride, chroma_offset, {cy, crv, cgu, cgv, cbu, y_off}};
    if (const int rc = check_frames(fr, format)) return rc;
    switch (format) {
        case PF_RGB: to_rgb_host<PF_RGB>(fr, out); break;
        case PF_BGR: to_rgb_host<PF_BGR>(fr, out); break;
        case PF_RGBA: to_rgb_host<PF_RGBA>(fr, out); break;
        case PF_BGRA: to_rgb_host<PF_BGRA>(fr, out); break;
        default: to_rgb_host<PF_NV12>(fr, out); break;
    }
    return BD_OK;
}

