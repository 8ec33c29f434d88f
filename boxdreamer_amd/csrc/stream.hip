// The two ends of a streaming pose step (boxdreamer_amd/stream.py: PoseStream), as one launch each, so that the step's captured graph
// holds two nodes where the façade enqueues a few dozen tiny torch kernels per frame:
//   * bd_stream_windows: detector boxes -> the integer crop windows and the intrinsics of the resized crops.  The torch form of
//     preprocess.square_bbox followed by preprocess.crop_intrinsics (the reference's square_bbox / _crop_image / adjust_intrinsic_matrix,
//     src/datasets/utils/preprocess.py:22-45, :253-259, :277-300), bit for bit: fp64 from the fp32 inputs, in those functions' order.
//   * bd_stream_results: what the demo loop reads per frame (src/demo/demo.py:1500-1564) in one row of BD_STREAM_ROW_FLOATS floats
//     per sample: the pose through nan_to_num, its reprojection RMS, a validity flag, the decoded corners in crop and in full-frame
//     pixels, and the 3-D box projected into the full frame with the solved pose.
// One sample per lane, one wavefront per 64 samples, plain vector loads and stores; both are bound by launch latency.  The
// arithmetic is written once (__host__ __device__) and runs on the host as bd_stream_*_host, the twin the tests compare the
// kernels against.  Floating-point contraction is OFF in it: hipcc -O3 would turn a * b - c * d into an FMA, which rounds once
// where torch's separate fp64 kernels round twice.
//   * bd_stream_track_windows: a second form of the step's first node (PoseStream(track_boxes=True)): each object's box is the 3-D
//     box projected with its own last pose (the last step's result row) while that pose is trusted, a detector box when one is
//     offered and it is not, the last box otherwise; then the same window arithmetic.  Same layout, same twin (_host).
//   * bd_stream_select_rows: between the encoder and the decoder of a step whose session owns a reference DATABASE per object
//     (PoseStream(select_k=...)): which k views the decoder reads this frame, decided on the device and written as the decoder's
//     source table, so the captured graph replays unchanged while the references change.  One workgroup per object; the arithmetic
//     and the rankings are bd_match_select_rows' and bd_pose_select_rows' own (select_common.h).
#include "select_common.h"
#include <cmath>

namespace {

constexpr int SW_LANES = 64;
constexpr int SW_MAX_N = 65535;

__host__ __device__ inline bool sw_finite(double v) { return v - v == 0.0; }

// one sample: box [4] x0 y0 x1 y1, K [9] -> win [4], Kc [9]
__host__ __device__ inline void stream_window(const float* box, const float* K, double padding, int out_size, int32_t* win, float* Kc) {
#pragma clang fp contract(off)
    const double b0 = box[0], b1 = box[1], b2 = box[2], b3 = box[3];
    // square_bbox: centre +- the larger half-extent x (1 + padding)
    const double cx = (b0 + b2) / 2.0, cy = (b1 + b3) / 2.0;
    const double ex = (b2 - b0) / 2.0, ey = (b3 - b1) / 2.0;
    const double size = (ex > ey ? ex : ey) * (1.0 + padding);
    const double lx = cx - size, ly = cy - size, hx = cx + size, hy = cy + size;
    // integer_box: left = int(x0), width = int(x1 - x0), every int() towards zero
    const double ltx = trunc(lx), lty = trunc(ly);
    const double whx = trunc(hx - lx), why = trunc(hy - ly);
    const double w0 = ltx, w1 = lty, w2 = ltx + whx, w3 = lty + why;
    const double lim = 2147483648.0;
    const bool ok = sw_finite(b0) && sw_finite(b1) && sw_finite(b2) && sw_finite(b3) && sw_finite(w0) && sw_finite(w1) && sw_finite(w2) &&
                    sw_finite(w3) && w0 >= -lim && w0 < lim && w1 >= -lim && w1 < lim && w2 >= -lim && w2 < lim && w3 >= -lim && w3 < lim;
    const int32_t x0 = ok ? (int32_t)w0 : 0, y0 = ok ? (int32_t)w1 : 0, x1 = ok ? (int32_t)w2 : 0, y1 = ok ? (int32_t)w3 : 0;
    win[0] = x0; win[1] = y0; win[2] = x1; win[3] = y1;
    // crop_intrinsics: scale = out_size / side, offset = (x0, y0).  torch evaluates `float / tensor` as reciprocal(tensor) * float
    // (Tensor.__rtruediv__): two roundings, and those are the bits to reproduce
    const double dx0 = (double)x0, dy0 = (double)y0;
    const double rx = 1.0 / ((double)x1 - dx0), ry = 1.0 / ((double)y1 - dy0);
    const double sx = rx * (double)out_size, sy = ry * (double)out_size;
    const double k00 = (double)K[0] * sx, k11 = (double)K[4] * sy;
    const double px = (double)K[2] * sx, ox = dx0 * sx, py = (double)K[5] * sy, oy = dy0 * sy;
    const double k02 = px - ox, k12 = py - oy;
    Kc[0] = (float)k00; Kc[1] = K[1]; Kc[2] = (float)k02;
    Kc[3] = K[3]; Kc[4] = (float)k11; Kc[5] = (float)k12;
    Kc[6] = K[6]; Kc[7] = K[7]; Kc[8] = K[8];
}

// one corner of the 3-D box (X [3]) through the pose p [16] and the full-frame intrinsics: Xc = ((r0 x + r1 y) + r2 z) + t, u = ((k00 xc +
// k01 yc) + k02 zc) / zc, v = (k11 yc + k12 zc) / zc in fp64, rounded once; zc <= 0 gives NaN for both.  bd_stream_results' box slots
// and bd_stream_track_windows' tracked box are this one function.
__host__ __device__ inline void stream_project(const float* p, const float* X, double k00, double k01, double k02, double k11, double k12,
                                               float* u, float* v) {
#pragma clang fp contract(off)
    const double x = X[0], y = X[1], z = X[2];
    double c[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double a = (double)p[4 * r] * x, b = (double)p[4 * r + 1] * y, d = (double)p[4 * r + 2] * z;
        const double ab = a + b;
        const double abd = ab + d;
        c[r] = abd + (double)p[4 * r + 3];
    }
    const double xc = c[0], yc = c[1], zc = c[2];
    if (zc <= 0.0) {
        *u = *v = __builtin_nanf("");
    } else {
        const double a = k00 * xc, b = k01 * yc, d = k02 * zc;
        const double ab = a + b;
        const double nu = ab + d;
        const double e = k11 * yc, g = k12 * zc;
        const double nv = e + g;
        *u = (float)(nu / zc);
        *v = (float)(nv / zc);
    }
}

// one sample: pose [16], rms, kp [16], win [4], K [9] full frame, box [24] -> row [BD_STREAM_ROW_FLOATS]
__host__ __device__ inline void stream_result(const float* pose, float rms, const float* kp, const int32_t* win, const float* K,
                                              const float* box, int out_size, float* row) {
#pragma clang fp contract(off)
    float p[16];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        p[i] = pose[i];
        const bool f = p[i] - p[i] == 0.0f;
        finite = finite && f;
        row[i] = f ? p[i] : 0.0f;                           // nan_to_num(nan = 0, posinf = 0, neginf = 0)
    }
    const bool ok = finite && p[15] == 1.0f;                // (a failed solve leaves an all-zero matrix)
    row[16] = rms;
    row[17] = ok ? 1.0f : 0.0f;
    // corners: crop pixels, then full-frame pixels (the inverse of crop_intrinsics: no half-pixel term)
    const double x0 = (double)win[0], y0 = (double)win[1];
    const double sx = (double)win[2] - x0, sy = (double)win[3] - y0;
    const double S = (double)out_size;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float kx = kp[2 * j], ky = kp[2 * j + 1];
        row[18 + 2 * j] = kx;
        row[19 + 2 * j] = ky;
        const double mx = (double)kx * sx, my = (double)ky * sy;
        const double qx = mx / S, qy = my / S;
        row[34 + 2 * j] = (float)(x0 + qx);
        row[35 + 2 * j] = (float)(y0 + qy);
    }
    // the 3-D box through the solved pose into the full frame
    const double k00 = K[0], k01 = K[1], k02 = K[2], k11 = K[4], k12 = K[5];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float u = 0.0f, v = 0.0f;
        if (ok) stream_project(p, box + 3 * j, k00, k01, k02, k11, k12, &u, &v);
        row[50 + 2 * j] = u;
        row[51 + 2 * j] = v;
    }
}

// one object: whose box this step crops.  prev [BD_STREAM_ROW_FLOATS] the last step's row, box3 [24], K [9] full frame, det [4],
// state [4] the box used last step -> out [4]; returns the source (BD_STREAM_BOX_*).  The tracked box is onepose's rule on the
// projected corners (min / max of the fp32 values); it is taken while the last pose is trusted and the box is usable.
__host__ __device__ inline int stream_track_box(const float* prev, const float* box3, const float* K, const float* det, int det_valid,
                                                int force, const float* state, int frame_h, int frame_w, float max_rms_px,
                                                double min_side_px, double max_side_px, float* out) {
#pragma clang fp contract(off)
    const double k00 = K[0], k01 = K[1], k02 = K[2], k11 = K[4], k12 = K[5];
    float u0 = 0.0f, v0 = 0.0f, u1 = 0.0f, v1 = 0.0f;
    bool finite = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float u, v;
        stream_project(prev, box3 + 3 * j, k00, k01, k02, k11, k12, &u, &v);
        finite = finite && u - u == 0.0f && v - v == 0.0f;
        u0 = j == 0 || u < u0 ? u : u0;
        u1 = j == 0 || u > u1 ? u : u1;
        v0 = j == 0 || v < v0 ? v : v0;
        v1 = j == 0 || v > v1 ? v : v1;
    }
    // usable: enough of it inside the frame, and not absurdly large (a pose that puts the object on the camera)
    const double x0 = u0, y0 = v0, x1 = u1, y1 = v1, fw = (double)frame_w, fh = (double)frame_h;
    const double cx0 = x0 > 0.0 ? x0 : 0.0, cy0 = y0 > 0.0 ? y0 : 0.0;
    const double cx1 = x1 < fw ? x1 : fw, cy1 = y1 < fh ? y1 : fh;
    const double vis_x = cx1 - cx0, vis_y = cy1 - cy0, ext_x = x1 - x0, ext_y = y1 - y0;
    const bool valid = finite && vis_x >= min_side_px && vis_y >= min_side_px && ext_x <= max_side_px && ext_y <= max_side_px;
    const bool trusted = prev[17] == 1.0f && prev[16] <= max_rms_px && force == 0 && valid;
    if (trusted) {
        out[0] = u0; out[1] = v0; out[2] = u1; out[3] = v1;
        return BD_STREAM_BOX_TRACKED;
    }
    const bool from_det = det_valid != 0;
    const float* src = from_det ? det : state;
    const float b0 = src[0], b1 = src[1], b2 = src[2], b3 = src[3];         // (read before `out` is written: out may be state)
    out[0] = b0; out[1] = b1; out[2] = b2; out[3] = b3;
    return from_det ? BD_STREAM_BOX_DETECTOR : BD_STREAM_BOX_HELD;
}

// one object of bd_stream_track_windows: the box, its window and crop intrinsics, and what is reported about it
__host__ __device__ inline void stream_track_window(const float* prev, const float* box3, const float* K, const float* det, int det_valid,
                                                    int force, float* state, double padding, int out_size, int frame_h, int frame_w,
                                                    float max_rms_px, double min_side_px, double max_side_px, int32_t* win, float* Kc,
                                                    int32_t* box_src, int32_t* keep, float* track) {
#pragma clang fp contract(off)
    float box[4];
    const int src = stream_track_box(prev, box3, K, det, det_valid, force, state, frame_h, frame_w, max_rms_px, min_side_px, max_side_px, box);
    stream_window(box, K, padding, out_size, win, Kc);
    state[0] = box[0]; state[1] = box[1]; state[2] = box[2]; state[3] = box[3];
    *box_src = src;
    if (keep) {                                             // the object's own box, every int() towards zero; not squared
        const double t0 = trunc((double)box[0]), t1 = trunc((double)box[1]), t2 = trunc((double)box[2]), t3 = trunc((double)box[3]);
        const double lim = 2147483648.0;
        const bool ok = sw_finite(t0) && sw_finite(t1) && sw_finite(t2) && sw_finite(t3) && t0 >= -lim && t0 < lim && t1 >= -lim && t1 < lim &&
                        t2 >= -lim && t2 < lim && t3 >= -lim && t3 < lim;
        keep[0] = ok ? (int32_t)t0 : 0; keep[1] = ok ? (int32_t)t1 : 0; keep[2] = ok ? (int32_t)t2 : 0; keep[3] = ok ? (int32_t)t3 : 0;
    }
    if (track) {
        track[0] = box[0]; track[1] = box[1]; track[2] = box[2]; track[3] = box[3];
        track[4] = (float)src;
    }
}

__global__ __launch_bounds__(SW_LANES) void stream_track_windows_kernel(const float* __restrict__ prev_rows, const float* __restrict__ bbox_3d,
                                                                        const float* __restrict__ K, const float* __restrict__ det_boxes,
                                                                        const int32_t* __restrict__ det_valid, const int32_t* __restrict__ force,
                                                                        float* state_box, double padding, int out_size, int frame_h,
                                                                        int frame_w, float max_rms_px, double min_side_px, double max_side_px,
                                                                        int32_t* __restrict__ windows, float* __restrict__ K_crop,
                                                                        int32_t* __restrict__ box_src, int32_t* keep_boxes, float* track, int n) {
    const int i = blockIdx.x * SW_LANES + threadIdx.x;
    if (i >= n) return;
    stream_track_window(prev_rows + (int64_t)i * BD_STREAM_ROW_FLOATS, bbox_3d + (int64_t)i * 24, K + (int64_t)i * 9, det_boxes + (int64_t)i * 4,
                        det_valid[i], force[i], state_box + (int64_t)i * 4, padding, out_size, frame_h, frame_w, max_rms_px, min_side_px,
                        max_side_px, windows + (int64_t)i * 4, K_crop + (int64_t)i * 9, box_src + i,
                        keep_boxes ? keep_boxes + (int64_t)i * 4 : nullptr, track ? track + (int64_t)i * 5 : nullptr);
}

__global__ __launch_bounds__(SW_LANES) void stream_windows_kernel(const float* __restrict__ det_boxes, const float* __restrict__ K,
                                                                  double padding, int out_size, int32_t* __restrict__ windows,
                                                                  float* __restrict__ K_crop, int n) {
    const int i = blockIdx.x * SW_LANES + threadIdx.x;
    if (i >= n) return;
    stream_window(det_boxes + (int64_t)i * 4, K + (int64_t)i * 9, padding, out_size, windows + (int64_t)i * 4, K_crop + (int64_t)i * 9);
}

__global__ __launch_bounds__(SW_LANES) void stream_results_kernel(const float* __restrict__ poses, const float* __restrict__ rms_px,
                                                                  const float* __restrict__ kp_px, const int32_t* __restrict__ windows,
                                                                  const float* __restrict__ K, const float* __restrict__ bbox_3d,
                                                                  int out_size, float* __restrict__ rows, int n) {
    const int i = blockIdx.x * SW_LANES + threadIdx.x;
    if (i >= n) return;
    stream_result(poses + (int64_t)i * 16, rms_px[i], kp_px + (int64_t)i * 16, windows + (int64_t)i * 4, K + (int64_t)i * 9,
                  bbox_3d + (int64_t)i * 24, out_size, rows + (int64_t)i * BD_STREAM_ROW_FLOATS);
}

// One workgroup (4 waves) per tracked object: both value arrays, the rule, then the ranking of the rule that applies.
//   scores   bd_match_select_rows' (score_slots): the appearance of every database slot against this frame's query
//   dist     bd_pose_select_rows' with cand = the identity over [0, n_refs[b]): the distance of every slot's pose to the last pose
//   rule     pose when rule == TRACK, force[b] == 0, the last row's ok == 1 and its rms <= max_rms_px (a comparison: a NaN rms
//            fails it); appearance otherwise.  Every thread reads the same four words: the decision is block-uniform.
//   ranking  topk_picks + compact_picks (appearance) or choose_nearest + compact_chosen with k = N_max, fk = k (pose)
// n_refs[b] is clamped into [0, N_max] and `rows` is not read past it; a row outside [0, R) is no view under either rule.
__global__ __launch_bounds__(256) void stream_select_rows_kernel(const float* __restrict__ sums, const float* __restrict__ counts,
                                                                  const float* __restrict__ poses, int R, const float* __restrict__ q_sums,
                                                                  const float* __restrict__ q_counts, const float* __restrict__ prev_rows,
                                                                  const int32_t* __restrict__ rows, const int32_t* __restrict__ n_refs,
                                                                  const int32_t* __restrict__ force, int N_max, int L, int D, int k, int rule,
                                                                  float max_rms_px, float* __restrict__ scores, float* __restrict__ dist,
                                                                  int32_t* __restrict__ used, int32_t* __restrict__ sel,
                                                                  int32_t* __restrict__ src) {
    __shared__ float val[SEL_MAXN];             // scores
    __shared__ float dval[SEL_MAXN];            // distances
    __shared__ int32_t tab[SEL_MAXN];           // the slot's private row, NO_VIEW: no view
    __shared__ int pick[SEL_MAXN];
    __shared__ unsigned char chosen[SEL_MAXN];
    __shared__ float wv[4];
    __shared__ int wi[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int N = n_refs[b];
    N = N < 0 ? 0 : (N > N_max ? N_max : N);
    const int32_t* row = rows + (int64_t)b * N_max;
    const float* prev = prev_rows + (int64_t)b * BD_STREAM_ROW_FLOATS;
    const bool by_pose = rule == BD_STREAM_SELECT_TRACK && force[b] == 0 && prev[17] == 1.0f && prev[16] <= max_rms_px;
    score_slots(sums, counts, R, q_sums + (int64_t)b * D, q_counts[b], row, N, N_max, L, D, val, scores + (int64_t)b * N_max);
    if (poses) {
        for (int c = tid; c < N_max; c += 256) {
            const int32_t r = c < N ? slot_row(row, c, N_max, R) : NO_VIEW;
            const float d = candidate_distance(prev, poses, r);
            tab[c] = r;
            dval[c] = d;
            dist[(int64_t)b * N_max + c] = d;
        }
    }
    if (tid == 0) used[b] = by_pose ? 1 : 0;
    __syncthreads();
    int32_t* out_sel = sel + (int64_t)b * k;
    int32_t* out_src = src + (int64_t)b * (k + 1);
    if (by_pose) {                                          // (block-uniform; poses != NULL: checked before the launch)
        choose_nearest(dval, tab, N_max, k, chosen);
        __syncthreads();
        compact_chosen(chosen, tab, N_max, k, b, out_sel, out_src);
    } else {
        const int n_picked = topk_picks(val, N, k, pick, wv, wi);
        compact_picks(pick, n_picked, k, row, R, b, out_sel, out_src);
    }
}

int windows_args(const void* a, const void* b, const void* c, const void* d, int out_size, int n) {
    if (!a || !b || !c || !d) return BD_ERR_NULL;
    if (n < 0 || n > SW_MAX_N || out_size < 1) return BD_ERR_SHAPE;
    return BD_OK;
}

int results_args(const void* a, const void* b, const void* c, const void* d, const void* e, const void* f, const void* g, int out_size, int n) {
    if (!a || !b || !c || !d || !e || !f || !g) return BD_ERR_NULL;
    if (n < 0 || n > SW_MAX_N || out_size < 1) return BD_ERR_SHAPE;
    return BD_OK;
}

int track_windows_args(const void* prev_rows, const void* bbox_3d, const void* K, const void* det_boxes, const void* det_valid,
                       const void* force, const void* state_box, const void* windows, const void* K_crop, const void* box_src, int out_size,
                       int frame_h, int frame_w, double min_side_px, double max_side_px, int n) {
    if (!prev_rows || !bbox_3d || !K || !det_boxes || !det_valid || !force || !state_box || !windows || !K_crop || !box_src) return BD_ERR_NULL;
    if (n < 0 || n > SW_MAX_N || out_size < 1 || frame_h < 1 || frame_w < 1) return BD_ERR_SHAPE;
    if (!(min_side_px > 0.0) || !(max_side_px > 0.0)) return BD_ERR_SHAPE;       // (a NaN fails both comparisons)
    return BD_OK;
}

}  // namespace

extern "C" int bd_stream_track_windows(const float* prev_rows, const float* bbox_3d, const float* K, const float* det_boxes,
                                       const int32_t* det_valid, const int32_t* force, float* state_box, double padding, int out_size,
                                       int frame_h, int frame_w, float max_rms_px, double min_side_px, double max_side_px, int32_t* windows,
                                       float* K_crop, int32_t* box_src, int32_t* keep_boxes, float* track, int n, void* stream) {
    const int rc = track_windows_args(prev_rows, bbox_3d, K, det_boxes, det_valid, force, state_box, windows, K_crop, box_src, out_size, frame_h,
                                      frame_w, min_side_px, max_side_px, n);
    if (rc != BD_OK || n == 0) return rc;
    hipLaunchKernelGGL(stream_track_windows_kernel, dim3((n + SW_LANES - 1) / SW_LANES), dim3(SW_LANES), 0, (hipStream_t)stream, prev_rows,
                       bbox_3d, K, det_boxes, det_valid, force, state_box, padding, out_size, frame_h, frame_w, max_rms_px, min_side_px,
                       max_side_px, windows, K_crop, box_src, keep_boxes, track, n);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_stream_track_windows_host(const float* prev_rows, const float* bbox_3d, const float* K, const float* det_boxes,
                                            const int32_t* det_valid, const int32_t* force, float* state_box, double padding, int out_size,
                                            int frame_h, int frame_w, float max_rms_px, double min_side_px, double max_side_px,
                                            int32_t* windows, float* K_crop, int32_t* box_src, int32_t* keep_boxes, float* track, int n) {
    const int rc = track_windows_args(prev_rows, bbox_3d, K, det_boxes, det_valid, force, state_box, windows, K_crop, box_src, out_size, frame_h,
                                      frame_w, min_side_px, max_side_px, n);
    if (rc != BD_OK) return rc;
    for (int i = 0; i < n; ++i)
        stream_track_window(prev_rows + (int64_t)i * BD_STREAM_ROW_FLOATS, bbox_3d + (int64_t)i * 24, K + (int64_t)i * 9,
                            det_boxes + (int64_t)i * 4, det_valid[i], force[i], state_box + (int64_t)i * 4, padding, out_size, frame_h, frame_w,
                            max_rms_px, min_side_px, max_side_px, windows + (int64_t)i * 4, K_crop + (int64_t)i * 9, box_src + i,
                            keep_boxes ? keep_boxes + (int64_t)i * 4 : nullptr, track ? track + (int64_t)i * 5 : nullptr);
    return BD_OK;
}

extern "C" int bd_stream_windows(const float* det_boxes, const float* K, double padding, int out_size, int32_t* windows, float* K_crop,
                                 int n, void* stream) {
    const int rc = windows_args(det_boxes, K, windows, K_crop, out_size, n);
    if (rc != BD_OK || n == 0) return rc;
    hipLaunchKernelGGL(stream_windows_kernel, dim3((n + SW_LANES - 1) / SW_LANES), dim3(SW_LANES), 0, (hipStream_t)stream, det_boxes, K,
                       padding, out_size, windows, K_crop, n);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_stream_windows_host(const float* det_boxes, const float* K, double padding, int out_size, int32_t* windows,
                                      float* K_crop, int n) {
    const int rc = windows_args(det_boxes, K, windows, K_crop, out_size, n);
    if (rc != BD_OK) return rc;
    for (int i = 0; i < n; ++i)
        stream_window(det_boxes + (int64_t)i * 4, K + (int64_t)i * 9, padding, out_size, windows + (int64_t)i * 4, K_crop + (int64_t)i * 9);
    return BD_OK;
}

extern "C" int bd_stream_results(const float* poses, const float* rms_px, const float* kp_px, const int32_t* windows, const float* K,
                                 const float* bbox_3d, int out_size, float* rows, int n, void* stream) {
    const int rc = results_args(poses, rms_px, kp_px, windows, K, bbox_3d, rows, out_size, n);
    if (rc != BD_OK || n == 0) return rc;
    hipLaunchKernelGGL(stream_results_kernel, dim3((n + SW_LANES - 1) / SW_LANES), dim3(SW_LANES), 0, (hipStream_t)stream, poses, rms_px,
                       kp_px, windows, K, bbox_3d, out_size, rows, n);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

extern "C" int bd_stream_results_host(const float* poses, const float* rms_px, const float* kp_px, const int32_t* windows, const float* K,
                                      const float* bbox_3d, int out_size, float* rows, int n) {
    const int rc = results_args(poses, rms_px, kp_px, windows, K, bbox_3d, rows, out_size, n);
    if (rc != BD_OK) return rc;
    for (int i = 0; i < n; ++i)
        stream_result(poses + (int64_t)i * 16, rms_px[i], kp_px + (int64_t)i * 16, windows + (int64_t)i * 4, K + (int64_t)i * 9,
                      bbox_3d + (int64_t)i * 24, out_size, rows + (int64_t)i * BD_STREAM_ROW_FLOATS);
    return BD_OK;
}

extern "C" int bd_stream_select_rows(const float* sums, const float* counts, const float* poses, int R, const float* q_sums,
                                     const float* q_counts, const float* prev_rows, const int32_t* rows, const int32_t* n_refs,
                                     const int32_t* force, int B, int N_max, int L, int D, int k, int rule, float max_rms_px,
                                     float* scores, float* dist, int32_t* used, int32_t* sel, int32_t* src, void* stream) {
    if (!sums || !counts || !q_sums || !q_counts || !prev_rows || !rows || !n_refs || !force || !scores || !used || !sel || !src) return BD_ERR_NULL;
    if (rule != BD_STREAM_SELECT_DINO && rule != BD_STREAM_SELECT_TRACK) return BD_ERR_SHAPE;
    if (!poses && rule != BD_STREAM_SELECT_DINO) return BD_ERR_NULL;
    if (poses && !dist) return BD_ERR_NULL;
    if (B <= 0 || R < 0 || N_max <= 0 || N_max > SEL_MAXN || k <= 0 || k > N_max || L <= 0 || D <= 0) return BD_ERR_SHAPE;
    hipLaunchKernelGGL(stream_select_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, sums, counts, poses, R, q_sums, q_counts,
                       prev_rows, rows, n_refs, force, N_max, L, D, k, rule, max_rms_px, scores, dist, used, sel, src);
    BD_CHECK_LAUNCH();
    return BD_OK;
}
