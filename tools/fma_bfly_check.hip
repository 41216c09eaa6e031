// fma_bfly_check.hip -- checks of the FMA-form network of coherent-rtlsdr_amd/csrc/cpk.hpp (fnet) and xcorr14p.hpp on the GPU.
//   1. bitwise: fma_j<K>(a, b, r), the one-instruction a + i^K r b every butterfly and twiddle bracket of the network is made of,
//      against the scalar fmaf formula it claims, for K = 0..3, for b = a (a bracket) and b != a, with r from an SGPR and r = 1
//      (the v_pk_add_f32 form);
//   2. accuracy: the FMA-form transforms K0 / K1 use (dft16s, dft32s, the pruned first pass, the fused inverse head) against a
//      double-precision DFT on the host, next to the product-form transforms they replace on the same inputs.  Each must be exact
//      to fp32 rounding: the worst error over the inputs, relative to the output's norm, below 1e-6 and at most twice the
//      product form's.
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -o tools/fma_bfly_check tools/fma_bfly_check.hip
// Prints "mismatches 0" and "accuracy ok" and exits 0 when every check passes.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
#include "../coherent-rtlsdr_amd/csrc/xcorr14p.hpp"

using namespace crsdr;

// ---- 1. the primitive, bit for bit -------------------------------------------------------------------------------------
template <int K>
__device__ void check_one(c2 a, c2 b, float r, int *bad)
{
    const c2 d = fma_j<K>(a, b, r);
    float ex, ey;
    if constexpr (K == 0) { ex = fmaf(r, b.x, a.x); ey = fmaf(r, b.y, a.y); }
    else if constexpr (K == 1) { ex = fmaf(-r, b.y, a.x); ey = fmaf(r, b.x, a.y); }
    else if constexpr (K == 2) { ex = fmaf(-r, b.x, a.x); ey = fmaf(-r, b.y, a.y); }
    else { ex = fmaf(r, b.y, a.x); ey = fmaf(-r, b.x, a.y); }
    if (__float_as_uint(d.x) != __float_as_uint(ex) || __float_as_uint(d.y) != __float_as_uint(ey)) atomicAdd(bad, 1);
}
__global__ void k_prim(const c2 *p, const c2 *q, float r, int *bad)
{
    const int i = threadIdx.x;
    const c2 a = p[i], b = q[i];
    check_one<0>(a, b, r, bad); check_one<1>(a, b, r, bad); check_one<2>(a, b, r, bad); check_one<3>(a, b, r, bad);
    check_one<0>(a, a, r, bad); check_one<1>(a, a, r, bad); check_one<2>(a, a, r, bad); check_one<3>(a, a, r, bad);
}

// ---- 2. the transforms against a double DFT ------------------------------------------------------------------------------
// case c of one thread: 32 inputs (16 for the pruned pass) at in[(c * 64 + lane) * 32 ...], twiddles (inverse head) in w
enum { C_DFT16F, C_DFT16I, C_DFT32F, C_DFT32I, C_PRUNED_SIG, C_PRUNED_REF, C_INVHEAD, C_INVMUL, NCASE };
template <bool FMA>
__global__ void k_net(const c2 *in, const c2 *w, c2 *out)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    const c2 *x = in + ((size_t)c * 64 + lane) * 32;
    const c2 *wl = w + (size_t)lane * 32;
    c2 v[32], ww[32], r[16];
#pragma unroll
    for (int i = 0; i < 32; ++i) { v[i] = x[i]; ww[i] = wl[i]; }
#pragma unroll
    for (int i = 0; i < 16; ++i) r[i] = ww[i];
    switch (c) {
    case C_DFT16F: if (FMA) fnet::dft16s<-1>(v); else x14p::dft16p<-1>(v); break;
    case C_DFT16I: if (FMA) fnet::dft16s<+1>(v); else x14p::dft16p<+1>(v); break;
    case C_DFT32F: if (FMA) x14p::dft32s<-1>(v); else x14p::dft32<-1>(v); break;
    case C_DFT32I: if (FMA) x14p::dft32s<+1>(v); else x14p::dft32<+1>(v); break;
    case C_PRUNED_SIG:
        if (FMA) x14p::dft32s_pruned<false>(v);
        else { x14p::dft32_stage1_pruned<0, false>(v); x14p::dft16p<-1>(v); x14p::dft16p<-1>(v + 16); }
        break;
    case C_PRUNED_REF:
        if (FMA) x14p::dft32s_pruned<true>(v);
        else { x14p::dft32_stage1_pruned<0, true>(v); x14p::dft16p<-1>(v); x14p::dft16p<-1>(v + 16); }
        break;
    case C_INVHEAD: x14p::tw_dft32_inv<FMA>(v, ww); break;
    case C_INVMUL: if (FMA) fnet::dft16s_inv_mul(v, r); else dft16_inv_mul(v, r); break;
    default: break;
    }
    c2 *o = out + ((size_t)c * 64 + lane) * 32;
#pragma unroll
    for (int i = 0; i < 32; ++i) o[i] = v[i];
}

static double frand(unsigned long long &s)
{
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)((s >> 11) & ((1ULL << 53) - 1)) / (double)(1ULL << 53) * 2.0 - 1.0;
}

int main()
{
    int bad_total = 0;
    // 1.
    {
        std::vector<c2> hp(64), hq(64);
        unsigned long long s = 12345;
        for (int i = 0; i < 64; ++i) {
            hp[i] = c2{(float)(100.0 * frand(s)), (float)(100.0 * frand(s))};
            hq[i] = c2{(float)(100.0 * frand(s)), (float)(100.0 * frand(s))};
        }
        c2 *p, *q; int *bad;
        hipMalloc(&p, 64 * sizeof(c2)); hipMalloc(&q, 64 * sizeof(c2)); hipMalloc(&bad, sizeof(int));
        hipMemcpy(p, hp.data(), 64 * sizeof(c2), hipMemcpyHostToDevice);
        hipMemcpy(q, hq.data(), 64 * sizeof(c2), hipMemcpyHostToDevice);
        hipMemset(bad, 0, sizeof(int));
        // the constants of the network: tangents, cosines, their ratios, and 1 (the v_pk_add_f32 form)
        const float rs[] = {1.0f, 0.19891236737965800691f, 0.41421356237309504880f, 0.66817863791929891999f, 0.70710678118654752440f,
                            0.92387953251128675613f, 1.0823922002923939688f, 1.4142135623730950488f, 0.5f, 3.0f};
        for (float r : rs) k_prim<<<1, 64>>>(p, q, r, bad);
        if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 2; }
        int hb = 0;
        hipMemcpy(&hb, bad, sizeof(int), hipMemcpyDeviceToHost);
        printf("mismatches %d\n", hb);
        bad_total += hb;
        hipFree(p); hipFree(q); hipFree(bad);
    }
    // 2.
    {
        const size_t n = (size_t)NCASE * 64 * 32;
        std::vector<c2> hin(n), hw(64 * 32), hnew(n), hold(n);
        unsigned long long s = 777;
        for (auto &x : hin) x = c2{(float)(127.0 * frand(s)), (float)(127.0 * frand(s))};
        for (int c : {C_PRUNED_SIG, C_PRUNED_REF})
            for (int l = 0; l < 64; ++l)
                for (int i = 16; i < 32; ++i) hin[((size_t)c * 64 + l) * 32 + i] = c2{0.f, 0.f};
        for (auto &x : hw) { const double a = M_PI * frand(s); x = c2{(float)cos(a), (float)sin(a)}; }
        c2 *din, *dw, *dout;
        hipMalloc(&din, n * sizeof(c2)); hipMalloc(&dw, hw.size() * sizeof(c2)); hipMalloc(&dout, n * sizeof(c2));
        hipMemcpy(din, hin.data(), n * sizeof(c2), hipMemcpyHostToDevice);
        hipMemcpy(dw, hw.data(), hw.size() * sizeof(c2), hipMemcpyHostToDevice);
        k_net<true><<<NCASE, 64>>>(din, dw, dout);
        hipMemcpy(hnew.data(), dout, n * sizeof(c2), hipMemcpyDeviceToHost);
        k_net<false><<<NCASE, 64>>>(din, dw, dout);
        hipMemcpy(hold.data(), dout, n * sizeof(c2), hipMemcpyDeviceToHost);
        if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 2; }
        const char *names[NCASE] = {"dft16 fwd", "dft16 inv", "dft32 fwd", "dft32 inv", "pruned sig", "pruned ref", "inv head", "inv mul"};
        bool ok = true;
        for (int c = 0; c < NCASE; ++c) {
            const int npt = (c == C_DFT16F || c == C_DFT16I || c == C_INVMUL) ? 16 : 32;
            double enew = 0, eold = 0;
            for (int l = 0; l < 64; ++l) {
                const c2 *x = &hin[((size_t)c * 64 + l) * 32];
                const c2 *wl = &hw[(size_t)l * 32];
                // the input the transform sees: the reference row's 16 values sit in the upper half; the inverse head and the
                // junction multiply by conj(w) / r first
                double xr[32], xi[32];
                for (int i = 0; i < npt; ++i) {
                    double a = x[i].x, b = x[i].y;
                    if (c == C_PRUNED_REF) { a = i >= 16 ? x[i - 16].x : 0.0; b = i >= 16 ? x[i - 16].y : 0.0; }
                    if (c == C_INVHEAD && i > 0) { const double wr = wl[i].x, wi = wl[i].y; const double t = a * wr + b * wi; b = b * wr - a * wi; a = t; }
                    if (c == C_INVMUL) { const double wr = wl[i].x, wi = wl[i].y; const double t = a * wr - b * wi; b = a * wi + b * wr; a = t; }
                    xr[i] = a; xi[i] = b;
                }
                const int dir = (c == C_DFT16F || c == C_DFT32F || c == C_PRUNED_SIG || c == C_PRUNED_REF) ? -1 : +1;
                double norm = 0, dn = 0, dol = 0;
                for (int k = 0; k < npt; ++k) {
                    double er = 0, ei = 0;
                    for (int j = 0; j < npt; ++j) {
                        const double ang = dir * 2.0 * M_PI * (double)((j * k) % npt) / npt;
                        er += xr[j] * cos(ang) - xi[j] * sin(ang);
                        ei += xr[j] * sin(ang) + xi[j] * cos(ang);
                    }
                    const int pos = npt == 16 ? k : (k & 1) * 16 + (k >> 1);      // dft16: natural order; dft32: x14::xpos
                    const c2 gn = hnew[((size_t)c * 64 + l) * 32 + pos], go = hold[((size_t)c * 64 + l) * 32 + pos];
                    norm += er * er + ei * ei;
                    dn = fmax(dn, hypot(gn.x - er, gn.y - ei));
                    dol = fmax(dol, hypot(go.x - er, go.y - ei));
                }
                norm = sqrt(norm / npt);
                enew = fmax(enew, dn / norm);
                eold = fmax(eold, dol / norm);
            }
            const bool pass = enew < 1e-6 && enew <= 2.0 * eold;
            ok = ok && pass;
            printf("%-11s worst error / rms output: FMA form %.3e   product form %.3e   %s\n", names[c], enew, eold, pass ? "ok" : "FAIL");
        }
        printf(ok ? "accuracy ok\n" : "accuracy FAIL\n");
        bad_total += ok ? 0 : 1;
        hipFree(din); hipFree(dw); hipFree(dout);
    }
    return bad_total != 0;
}
