// Which way of making F16C8's lo8 byte e4m3((x - hi) 2^11) survives a residual that overflows fp32 when scaled by 2^11?  Under MODE.FP16_OVFL,
// side by side: fp32 multiply + v_cvt_pk_fp8_f32 (the form the kernels had), v_cvt_scalef32_pk_fp8_f32 with scale 2^-11 (the form they have:
// csrc/bd_common.h f16c8_lo8_pk), multiply + v_med3_f32 + v_cvt_pk_fp8_f32.  Prints the bytes for fp32's largest values, the lo8 ties and
// subnormals of tests/test_operand_host.py's table, and counts the differences over 1M random values of 30 binades.  Measured on one MI355X:
// the first form gives the NaN byte 0x7f / 0xff from |x| = 1.7e35 on, the other two 0x7e / 0xfe; no difference on the random values.
// (measurement tool: hipcc --offload-arch=gfx950 -o lo8_scaled_cvt_probe lo8_scaled_cvt_probe.hip)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <vector>
typedef short s2 __attribute__((ext_vector_type(2)));
__global__ void k(const float* in, unsigned char* a, unsigned char* b, unsigned char* c, int n) {
    __builtin_amdgcn_s_setreg(1 | (23 << 6) | (0 << 11), 1);
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) * 2;
    if (i >= n) return;
    float x0 = in[i], x1 = in[i + 1];
    asm("" : "+v"(x0)); asm("" : "+v"(x1));
    const _Float16 h0 = (_Float16)x0, h1 = (_Float16)x1;
    const float r0 = x0 - (float)h0, r1 = x1 - (float)h1;
    int p = 0;
    p = __builtin_amdgcn_cvt_pk_fp8_f32(r0 * 2048.f, r1 * 2048.f, p, false);
    a[i] = p & 0xff; a[i + 1] = (p >> 8) & 0xff;
    s2 o = {0, 0};
    o = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(o, r0, r1, 1.0f / 2048.f, false);
    const unsigned u = __builtin_bit_cast(unsigned, o);
    b[i] = u & 0xff; b[i + 1] = (u >> 8) & 0xff;
    int q = 0;
    q = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_fmed3f(r0 * 2048.f, -448.f, 448.f), __builtin_amdgcn_fmed3f(r1 * 2048.f, -448.f, 448.f), q, false);
    c[i] = q & 0xff; c[i + 1] = (q >> 8) & 0xff;
}
int main() {
    std::vector<float> v = {3.4028234663852886e38f, -3.4028234663852886e38f, 1e36f, -1e36f, 1.6e35f, 1.7e35f, 3e9f, 1e5f, 7e4f, 65520.f, 512.24f, 1024.49f, 40015.f,
                            1 + 17 * ldexpf(1, -16), 1 + 19 * ldexpf(1, -16), 100 + 34 * ldexpf(1, -11), 100 + 38 * ldexpf(1, -11), 1 + ldexpf(1, -20), 1 + ldexpf(1, -21), 0.f};
    const int special = (int)v.size();
    unsigned s = 12345;
    for (int i = 0; i < 1 << 20; ++i) {              // random values over many binades (both signs)
        s = s * 1664525u + 1013904223u;
        const float m = 1.0f + (float)(s >> 9) / 8388608.0f;
        s = s * 1664525u + 1013904223u;
        const int e = (int)(s >> 24) % 30 - 14;
        v.push_back(((s >> 8) & 1 ? -1.f : 1.f) * ldexpf(m, e));
    }
    const int n = (int)v.size();
    float* d; unsigned char *a, *b, *c;
    if (hipMalloc(&d, n * 4) != hipSuccess || hipMalloc(&a, n) != hipSuccess || hipMalloc(&b, n) != hipSuccess || hipMalloc(&c, n) != hipSuccess) return 1;
    if (hipMemcpy(d, v.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) return 1;
    k<<<(n / 2 + 255) / 256, 256>>>(d, a, b, c, n);
    std::vector<unsigned char> ha(n), hb(n), hc(n);
    if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
    if (hipMemcpy(ha.data(), a, n, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hb.data(), b, n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(hc.data(), c, n, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    for (int i = 0; i < special; ++i) printf("x = %-14g  mul+cvt %02x   scaled cvt %02x   mul+med3+cvt %02x\n", v[i], ha[i], hb[i], hc[i]);
    long dab = 0, dac = 0;
    for (int i = special; i < n; ++i) { dab += ha[i] != hb[i]; dac += ha[i] != hc[i]; }
    printf("random values: %d, mul+cvt vs scaled cvt differ in %ld, mul+cvt vs med3 differ in %ld\n", n - special, dab, dac);
    return 0;
}
