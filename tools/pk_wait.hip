// pk_wait.hip -- microbenchmark: what do the software wait states of the packed butterflies cost?  ("wait states")
// One middle forward pass of K1 on registers -- dft32s<-1> + tw_apply, no LDS, no memory -- in a loop, at one and at two waves
// per SIMD, on random data.  Built twice from the same source:
//     hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -DCRSDR_PK_GROUPS=0 -o tools/pk_wait_single tools/pk_wait.hip
//     hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -DCRSDR_PK_GROUPS=1 -o tools/pk_wait_grouped tools/pk_wait.hip
// (0: every product's second half right behind its first, a wait state each; 1: cpk.hpp's grouped forms.  In isolation the
// compiler has registers to spare and interleaves most of the single forms itself, so the two loops differ by few wait states;
// -DPK_WAIT_PAD=64 adds 64 s_nop 0 per transform to either, which prices a wait state directly at each occupancy.)  The static count of
// wait states in each loop:  add --cuda-device-only -S -o pk_wait.s to the line above, then
//     python3 tools/k1_isa_count.py --asm pk_wait.s --pattern k_loop --loops
// Prints ns per transform (per wave) of five launches and their median for each occupancy.  One workgroup per CU (its LDS request
// keeps a second one out): 256 threads = one wave per SIMD, 512 threads = two.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>
#include "../coherent-rtlsdr_amd/csrc/xcorr14p.hpp"

using namespace crsdr;
using namespace crsdr::x14p;

constexpr int kLds = 96 * 1024;      // more than half a CU's 160 KiB

__global__ __launch_bounds__(512, 1) void k_loop(const c2 *__restrict__ in, c2 *__restrict__ out, int iters)
{
    extern __shared__ unsigned char smem[];
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    c2 v[32], w[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) { v[j] = in[gid * 64 + j]; w[j] = in[gid * 64 + 32 + j]; }
    for (int it = 0; it < iters; ++it) {
        dft32s<-1>(v);
        tw_apply<-1, true, 1>(v, w);      // |w| = 1 / sqrt(32): the values keep their size from one transform to the next ...
        v[0] = v[0] * 0.17677669529663689f;      // ... output 0, which has no twiddle, by a product of its own (one v_pk_mul_f32 in every build)
#ifdef PK_WAIT_PAD      // the price of a wait state on its own: PK_WAIT_PAD more s_nop 0 per transform, one behind each value
#pragma unroll
        for (int j = 0; j < PK_WAIT_PAD; ++j) asm volatile("s_nop 0" : "+v"(v[j % 32]));
#endif
    }
#pragma unroll
    for (int j = 0; j < 32; ++j) out[gid * 32 + j] = v[j];
    if (iters < 0) smem[threadIdx.x] = 1;      // never: the LDS request is what matters
}

int main()
{
    int cus = 0;
    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
    if (cus <= 0) { printf("no device\n"); return 1; }
    const size_t nthr = (size_t)cus * 512;
    std::vector<c2> h(nthr * 64);
    uint32_t st = 777u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return (float)(st >> 8) * (1.0f / 16777216.0f); };
    for (size_t t = 0; t < nthr; ++t)
        for (int j = 0; j < 32; ++j) {
            h[t * 64 + j] = c2{std::floor(rnd() * 255.0f) - 127.0f, std::floor(rnd() * 255.0f) - 127.0f};
            const float th = 6.2831853f * rnd(), a = 0.17677669529663689f;
            h[t * 64 + 32 + j] = c2{a * std::cos(th), a * std::sin(th)};
        }
    c2 *din, *dout;
    if (hipMalloc(&din, h.size() * sizeof(c2)) != hipSuccess || hipMalloc(&dout, nthr * 32 * sizeof(c2)) != hipSuccess) return 1;
    hipMemcpy(din, h.data(), h.size() * sizeof(c2), hipMemcpyHostToDevice);
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_loop), hipFuncAttributeMaxDynamicSharedMemorySize, kLds) != hipSuccess) return 1;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    const int iters = 20000;
#ifndef PK_WAIT_PAD
#define PK_WAIT_PAD 0
#endif
    printf("pk_wait: CRSDR_PK_GROUPS=%d, PK_WAIT_PAD=%d, %d CUs, %d transforms per wave and launch\n", CRSDR_PK_GROUPS, PK_WAIT_PAD, cus, iters);
    for (int wps = 1; wps <= 2; ++wps) {
        const int threads = 256 * wps;
        k_loop<<<cus, threads, kLds>>>(din, dout, 200);
        if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
        std::vector<double> ns;
        for (int r = 0; r < 5; ++r) {
            hipEventRecord(e0);
            k_loop<<<cus, threads, kLds>>>(din, dout, iters);
            hipEventRecord(e1);
            if (hipEventSynchronize(e1) != hipSuccess) { printf("launch failed\n"); return 1; }
            float ms = 0.f;
            hipEventElapsedTime(&ms, e0, e1);
            ns.push_back((double)ms * 1e6 / iters);
        }
        printf("waves/SIMD=%d  ns per transform:", wps);
        for (double x : ns) printf(" %.1f", x);
        std::sort(ns.begin(), ns.end());
        printf("  median %.1f  (per SIMD: %.1f ns per transform)\n", ns[2], ns[2] / wps);
    }
    c2 chk[32];
    hipMemcpy(chk, dout, sizeof(chk), hipMemcpyDeviceToHost);
    printf("sample output %.6g %.6g\n", chk[0].x, chk[5].y);
    return 0;
}
