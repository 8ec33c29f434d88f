// Source pixel formats of the crop kernel, written once: how the bytes of a frame become the pixel the filter sees,
// R | G << 8 | B << 16 in one dword.  The stage loop of crop_resize_kernel (preprocess.hip), its direct form and the host entry
// bd_frames_to_rgb_host run this text, so a pixel has the same bits wherever it was converted (boxdreamer_amd/preprocess.py
// frames_to_rgb is the Python mirror the three are tested against).
//
// NV12 -> RGB is integer arithmetic in int32, 16 fractional bits, rounded to nearest, >> arithmetic (floor):
//   y = Y - y_off, u = U - 128, v = V - 128
//   R = clamp((cy y         + crv v + 32768) >> 16, 0, 255)
//   G = clamp((cy y - cgu u - cgv v + 32768) >> 16, 0, 255)
//   B = clamp((cy y + cbu u         + 32768) >> 16, 0, 255)
// The coefficients are the caller's (include/boxdreamer_hip.h has the four tables); each is at most 2^20, so the largest
// intermediate stays below 2^30.  Chroma is sampled nearest: pixel (x, y) uses the pair (x >> 1, y >> 1).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace {

constexpr int PF_RGB = 0, PF_BGR = 1, PF_RGBA = 2, PF_BGRA = 3, PF_NV12 = 4;      // BD_PIXEL_*
constexpr int PF_MAX_COEF = 1 << 20;

struct YuvCoef {
    int cy, crv, cgu, cgv, cbu, y_off;
};

__host__ __device__ inline int pf_bytes_per_pixel(int fmt) { return fmt == PF_NV12 ? 1 : (fmt == PF_RGBA || fmt == PF_BGRA ? 4 : 3); }

__host__ __device__ inline int pf_clamp_byte(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// bytes 0 and 2 change places, byte 3 is dropped: B G R [A] -> R | G << 8 | B << 16
__host__ __device__ inline uint32_t pf_swap_rb(uint32_t px) { return ((px & 0xffu) << 16) | (px & 0xff00u) | ((px >> 16) & 0xffu); }

// the three (or four) bytes of a packed pixel, read as a little-endian dword, to the staged dword
template <int FMT>
__host__ __device__ inline uint32_t pf_packed_px(uint32_t bytes) {
    return (FMT == PF_BGR || FMT == PF_BGRA) ? pf_swap_rb(bytes) : (bytes & 0xffffffu);
}

__host__ __device__ inline uint32_t pf_yuv_px(int Y, int U, int V, const YuvCoef& c) {
    const int y = c.cy * (Y - c.y_off) + 32768, u = U - 128, v = V - 128;
    const int r = pf_clamp_byte((y + c.crv * v) >> 16);
    const int g = pf_clamp_byte((y - c.cgu * u - c.cgv * v) >> 16);
    const int b = pf_clamp_byte((y + c.cbu * u) >> 16);
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
}

// One pixel straight from a frame in memory (the kernel's direct form, and every pixel of the host entry): frame = the frame's
// first byte, chroma_offset = where its interleaved U V plane starts (NV12 only).
template <int FMT>
__host__ __device__ inline uint32_t pf_load_px(const uint8_t* frame, int64_t row_stride, int64_t chroma_offset, long long x, long long y,
                                               const YuvCoef& c) {
    if (FMT == PF_NV12) {
        const uint8_t* uv = frame + chroma_offset + (y >> 1) * row_stride + (x & ~1LL);
        return pf_yuv_px(frame[y * row_stride + x], uv[0], uv[1], c);
    }
    const uint8_t* p = frame + y * row_stride + x * ((FMT == PF_RGBA || FMT == PF_BGRA) ? 4 : 3);
    return pf_packed_px<FMT>((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16));
}

}  // namespace
