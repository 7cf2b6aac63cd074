// micro-benchmark (development aid): rate of v_mfma_f32_16x16x4_f32 with 1, 2 and 4 waves per SIMD -- 4 chains per wave, 16
// different A registers, no memory access in the loop (operands zero, or random with any argument); 256 workgroups (one per CU), then 512 / 1024 whose dynamic LDS size (64 KB /
// 40 KB) lets at most 2 / 4 of them share a CU
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k(const float* in, float* out, int n) {
    extern __shared__ float pad[];
    if (n < 0) pad[threadIdx.x] = 0.f;
    float a[16], b[4];
    for (int i = 0; i < 16; ++i) a[i] = in[threadIdx.x + 256 * i];
    for (int i = 0; i < 4; ++i) b[i] = in[threadIdx.x + 256 * (16 + i)];
    f32x4 c0 = {0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0;
    for (int i = 0; i < n; ++i) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * s + 0], b[s], c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * s + 1], b[s], c1, 0, 0, 0);
            c2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * s + 2], b[s], c2, 0, 0, 0);
            c3 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * s + 3], b[s], c3, 0, 0, 0);
        }
    }
    out[blockIdx.x * 256 + threadIdx.x] = c0[0] + c1[1] + c2[2] + c3[3];
}
int main(int argc, char** argv) {
    float *in, *out;
    hipMalloc(&in, 256 * 20 * 4); hipMemset(in, 0, 256 * 20 * 4); hipMalloc(&out, 4096 * 256 * 4);
    if (argc > 1) {                                         // any argument: operands uniform in [-1, 1) instead of zeros (the clock under real data)
        static float h[256 * 20];
        unsigned x = 12345u;
        for (float& v : h) { x = x * 1664525u + 1013904223u; v = (float)(x >> 8) / 8388608.f - 1.f; }
        hipMemcpy(in, h, sizeof h, hipMemcpyHostToDevice);
        printf("operands: uniform [-1, 1)\n");
    }
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    // first pass: the same trips per wave (more waves: more work, longer runs); second pass, equal work: trips = 16000 / waves
    // per SIMD, so every configuration issues the same MFMAs per SIMD and runs about as long -- a clock that falls with the
    // length of a run cannot tell them apart then; the order 4, 2, 1, 4, 2, 1 keeps a warm-up trend from siding with one of them
    for (int equal = 0; equal < 2; ++equal)
        for (int round = 0; round < (equal ? 2 : 1); ++round)
            for (int wg = equal ? 4 : 1; wg >= 1 && wg <= 4; wg = equal ? wg / 2 : wg * 2) {
                const int n = equal ? 16000 / wg : 4000;    // 16 MFMAs per trip
                for (int rep = 0; rep < 3; ++rep) {
                    hipEventRecord(e0);
                    k<<<256 * wg, 256, wg == 1 ? 0 : wg == 2 ? 65536 : 40960>>>(in, out, n);
                    hipEventRecord(e1); hipEventSynchronize(e1);
                    float ms; hipEventElapsedTime(&ms, e0, e1);
                    const double mf = 16.0 * n * wg;        // MFMAs per SIMD
                    if (rep) printf("%s%d wave(s) per SIMD: %.3f ms, %.2f ns per MFMA per SIMD, chip %.1f TFLOP/s\n", equal ? "equal work, " : "", wg, ms, ms * 1e6 / mf, 2048.0 * mf * 1024 / (ms * 1e-3) / 1e12);
                }
            }
    return hipGetLastError() != hipSuccess;
}
