// Microbenchmark: issue cost of VALU instruction kinds on gfx950 as a function of waves per SIMD.
// Build: hipcc --offload-arch=gfx950 -O3 -fno-slp-vectorize -o valu_rate tools/valu_rate.hip
// (without -fno-slp-vectorize the compiler packs the independent plain f32 rows into v_pk_*_f32 itself, and they measure
// the packed instructions under the plain names; the packed rows are written with two-lane vector types)
// Every kind runs as 16 (packed: 8) independent instructions per loop turn and, DEP, as one dependent chain of as many.
// The packed f32 kinds count one instruction for the two operations each holds: "per instr" is per v_pk_* instruction,
// to be set against TWO of the plain kind.  v_pk_fma_f32 bcast is the form the sweep step's geometry compiles to when the
// compiler packs it: one operand a register pair of which both halves read the low register (op_sel_hi:[1,0,1]).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
typedef float float2_t __attribute__((ext_vector_type(2)));

template <int KIND, bool DEP>
__global__ __launch_bounds__(64) void k(float* out, unsigned long long* cyc, int iters, float b, float c)
{
    float a[16]; float2_t p[8]; unsigned u[16];
    for (int i = 0; i < 16; ++i) { a[i] = threadIdx.x * 0.001f + i; u[i] = threadIdx.x * 977u + i; }
    for (int i = 0; i < 8; ++i) { p[i].x = a[2*i]; p[i].y = a[2*i+1]; }
    float2_t pb = {b, b}, pc = {c, c};
    float2_t pl = {b, c};                         // bcast: only .x is read
    unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
        if (KIND == 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) a[DEP ? 0 : i] = __builtin_fmaf(a[DEP ? 0 : i], b, c);
        } else if (KIND == 1) {
#pragma unroll
            for (int i = 0; i < 8; ++i) p[DEP ? 0 : i] = __builtin_elementwise_fma(p[DEP ? 0 : i], pb, pc);
        } else if (KIND == 2) {
#pragma unroll
            for (int i = 0; i < 16; ++i) u[DEP ? 0 : i] = u[DEP ? 0 : i] * 0x85EBCA6Bu + 1u;
        } else if (KIND == 3) {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                a[DEP ? 0 : i] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a[DEP ? 0 : i]), 0x130, 0xf, 0xf, true)) + c;
        } else if (KIND == 4) {
#pragma unroll
            for (int i = 0; i < 16; ++i) a[DEP ? 0 : i] = a[DEP ? 0 : i] + c;
        } else if (KIND == 5) {
#pragma unroll
            for (int i = 0; i < 8; ++i) p[DEP ? 0 : i] = p[DEP ? 0 : i] + pc;
        } else if (KIND == 6) {
#pragma unroll
            for (int i = 0; i < 8; ++i) p[DEP ? 0 : i] = p[DEP ? 0 : i] * pb;
        } else if (KIND == 7) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(p[DEP ? 0 : i]) : "v"(p[DEP ? 0 : i]), "v"(pl), "v"(pc));
        } else if (KIND == 8) {
#pragma unroll
            for (int i = 0; i < 16; ++i) a[DEP ? 0 : i] = a[DEP ? 0 : i] * b;
        }
    }
    unsigned long long t1 = __builtin_amdgcn_s_memtime();
    float s = 0; for (int i = 0; i < 16; ++i) s += a[i] + (float)u[i]; for (int i = 0; i < 8; ++i) s += p[i].x + p[i].y;
    out[blockIdx.x * 64 + threadIdx.x] = s;
    if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
}

template <int KIND, bool DEP = false> void run(const char* name, int per_instr_ops)
{
    const int iters = 20000;
    float* out; unsigned long long* cyc;
    hipMalloc(&out, 256 * 4 * 8 * 64 * 4); hipMalloc(&cyc, 256 * 4 * 8 * 8);
    for (int wps : {1, 2, 4, 8}) {
        int blocks = 256 * 4 * wps;
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        hipLaunchKernelGGL((k<KIND, DEP>), dim3(blocks), dim3(64), 0, 0, out, cyc, 100, 1.0001f, 0.5f);
        hipEventRecord(e0);
        hipLaunchKernelGGL((k<KIND, DEP>), dim3(blocks), dim3(64), 0, 0, out, cyc, iters, 1.0001f, 0.5f);
        hipEventRecord(e1); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        std::vector<unsigned long long> h(blocks); hipMemcpy(h.data(), cyc, blocks * 8, hipMemcpyDeviceToHost);
        double avg = 0; for (auto v : h) avg += v; avg /= blocks;
        double instr_per_wave = (double)iters * per_instr_ops;
        // s_memtime ticks at 100 MHz? report both wall-derived and tick-derived
        printf("%-18s %-5s waves/SIMD=%d  wall=%.3f ms  ticks/wave=%.0f  wall ns per instr per SIMD=%.3f (x2.4GHz = %.2f cyc)\n",
               name, DEP ? "chain" : "indep", wps, ms, avg, ms * 1e6 / (instr_per_wave * wps), ms * 1e6 / (instr_per_wave * wps) * 2.4);
        hipEventDestroy(e0); hipEventDestroy(e1);
    }
    hipFree(out); hipFree(cyc);
}
int main() {
    run<0>("v_fma_f32", 16); run<1>("v_pk_fma_f32", 8); run<2>("v_mul_lo+add", 16); run<3>("v_add_dpp", 16); run<4>("v_add_f32", 16);
    run<8>("v_mul_f32", 16); run<5>("v_pk_add_f32", 8); run<6>("v_pk_mul_f32", 8); run<7>("v_pk_fma_f32 bcast", 8);
    run<0, true>("v_fma_f32", 16); run<4, true>("v_add_f32", 16); run<8, true>("v_mul_f32", 16);
    run<1, true>("v_pk_fma_f32", 8); run<5, true>("v_pk_add_f32", 8); run<6, true>("v_pk_mul_f32", 8); run<7, true>("v_pk_fma_f32 bcast", 8);
    return 0;
}
