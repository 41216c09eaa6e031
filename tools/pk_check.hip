// pk_check.hip -- bitwise check of the packed complex primitives of coherent-rtlsdr_amd/csrc/cpk.hpp against their scalar
// formulations (fft_lds.hpp), and of cpk.hpp's grouped forms (several independent values per asm statement, breadth-first)
// and the places that use them against the single forms run one after the other: random values, +-0, +-inf, NaN, denormals.
// Build: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -o tools/pk_check tools/pk_check.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../coherent-rtlsdr_amd/csrc/xcorr14q.hpp"
typedef float c2 __attribute__((ext_vector_type(2)));
namespace prim {      // the primitives written out once more, so that this part checks the instruction forms and not a header
// a * b, rounding like fma(a.x,b.x,-(a.y*b.y)), fma(a.x,b.y,a.y*b.x)
__device__ __forceinline__ c2 cmul(c2 a, c2 b)
{
    c2 t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0]" : "=v"(t) : "v"(a), "v"(b));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1] neg_lo:[0,0,1]" : "=v"(r) : "v"(a), "v"(b), "v"(t));
    return r;
}
// a * conj(b): fma(a.x,b.x,a.y*b.y), fma(a.y,b.x,-(a.x*b.y))
__device__ __forceinline__ c2 cmulc(c2 a, c2 b)
{
    c2 t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "v"(b));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1] neg_hi:[0,0,1]" : "=v"(r) : "v"(a), "v"(b), "v"(t));
    return r;
}
// a + (-i) x = (a.x + x.y, a.y - x.x);  a - (-i) x = (a.x - x.y, a.y + x.x)
__device__ __forceinline__ c2 add_mj(c2 a, c2 x) { c2 r; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(x)); return r; }
__device__ __forceinline__ c2 sub_mj(c2 a, c2 x) { c2 r; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(x)); return r; }
__global__ void k(c2 *p, const c2 *q, float *chk)
{
    int i = threadIdx.x;
    c2 a = p[i], b = q[i];
    c2 m = cmul(a, b), n = cmulc(a, b);
    c2 u = add_mj(a, b), w = sub_mj(a, b);
    p[i] = m; p[i + 64] = n; p[i + 128] = u; p[i + 192] = w;
    // scalar references
    chk[8 * i + 0] = fmaf(a.x, b.x, -(a.y * b.y)); chk[8 * i + 1] = fmaf(a.x, b.y, a.y * b.x);
    chk[8 * i + 2] = fmaf(a.x, b.x, a.y * b.y);    chk[8 * i + 3] = fmaf(a.y, b.x, -(a.x * b.y));
    chk[8 * i + 4] = a.x + b.y; chk[8 * i + 5] = a.y - b.x; chk[8 * i + 6] = a.x - b.y; chk[8 * i + 7] = a.y + b.x;
}
} // namespace prim

// ---- grouped forms against the single forms, bit for bit ---------------------------------------------------------------
namespace grp {
using namespace crsdr;
using namespace crsdr::x14p;
__device__ __forceinline__ uint32_t hash(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
__device__ __forceinline__ int differ(c2 a, c2 b) { return __float_as_uint(a.x) != __float_as_uint(b.x) || __float_as_uint(a.y) != __float_as_uint(b.y); }
template <bool CONJ> __device__ __forceinline__ c2 mul1(c2 a, c2 b) { return CONJ ? cmulc(a, b) : cmul(a, b); }
template <bool CONJ> __device__ __forceinline__ c2 mad1(c2 c, c2 a, c2 b) { return CONJ ? cmulc_add(c, a, b) : cmul_add(c, a, b); }

template <bool CONJ>
__device__ int check_products(const c2 *x)
{
    int bad = 0;
    c2 r0, r1, r2, r3;
    cmul_g2<CONJ>(r0, r1, x[0], x[1], x[2], x[3]);
    bad += differ(r0, mul1<CONJ>(x[0], x[2])) + differ(r1, mul1<CONJ>(x[1], x[3]));
    cmul_g3<CONJ>(r0, r1, r2, x[4], x[5], x[6], x[7], x[8], x[9]);
    bad += differ(r0, mul1<CONJ>(x[4], x[7])) + differ(r1, mul1<CONJ>(x[5], x[8])) + differ(r2, mul1<CONJ>(x[6], x[9]));
    cmul_g4<CONJ>(r0, r1, r2, r3, x[10], x[11], x[12], x[13], x[14], x[15], x[16], x[17]);
    bad += differ(r0, mul1<CONJ>(x[10], x[14])) + differ(r1, mul1<CONJ>(x[11], x[15])) + differ(r2, mul1<CONJ>(x[12], x[16])) + differ(r3, mul1<CONJ>(x[13], x[17]));
    c2 s0, s1, t0, t1;
    head_g2<CONJ>(s0, s1, t0, t1, x[18], x[19], x[20], x[21], x[22], x[23], x[24], x[25]);
    const c2 p0 = mul1<CONJ>(x[18], x[20]), e0 = mad1<CONJ>(p0, x[22], x[24]);
    const c2 p1 = mul1<CONJ>(x[19], x[21]), e1 = mad1<CONJ>(p1, x[23], x[25]);
    bad += differ(s0, e0) + differ(s1, e1) + differ(t0, twice_minus(p0, e0)) + differ(t1, twice_minus(p1, e1));
    return bad;
}
// tab: ntab floats, the first 16 of them the special values; one thread draws its 64 values by hash
__global__ void k_groups(const float *tab, int ntab, int *bad)
{
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    c2 x[32], w[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        x[j] = c2{tab[hash(id * 128 + 4 * j) % ntab], tab[hash(id * 128 + 4 * j + 1) % ntab]};
        w[j] = c2{tab[hash(id * 128 + 4 * j + 2) % ntab], tab[hash(id * 128 + 4 * j + 3) % ntab]};
    }
    int n = check_products<false>(x) + check_products<true>(w);
    {   // the twiddle chain: w[k] = w[k - hb] w[hb], hb the highest bit of k
        c2 a[32], e[32];
        a[1] = e[1] = w[1]; a[2] = e[2] = w[2]; a[4] = e[4] = w[4]; a[8] = e[8] = w[8]; a[16] = e[16] = w[16];
        tw_chain(a);
#pragma unroll
        for (int k = 3; k < 32; ++k) {
            const int hb = k >= 16 ? 16 : k >= 8 ? 8 : k >= 4 ? 4 : 2;
            if (k != hb) e[k] = cmul(e[k - hb], e[hb]);
        }
#pragma unroll
        for (int k = 1; k < 32; ++k) n += differ(a[k], e[k]);
    }
    {   // the output twiddles of a forward pass (both layouts and directions)
        c2 a[32], b[32], c[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) a[k] = b[k] = c[k] = x[k];
        tw_apply<-1, true, 1>(a, w);
        tw_apply<+1, false, 1>(b, w);
#pragma unroll
        for (int k = 1; k < 32; ++k) n += differ(a[xpos(k)], cmul(c[xpos(k)], w[k])) + differ(b[k], cmulc(c[k], w[k]));
        n += differ(a[0], c[0]) + differ(b[0], c[0]);
    }
    {   // the inverse pass's head
        c2 a[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) a[k] = x[k];
        tw_stage1s_inv<0>(a, w);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const c2 p = i == 0 ? x[0] : cmulc(x[i], w[i]);
            const c2 s = cmulc_add(p, x[i + 16], w[i + 16]);
            n += differ(a[i], s);
        }
        // the differences carry their stage's bracket: compare through the single forms
        n += differ(a[16], fnet::w32b<+1, 0>(twice_minus(x[0], cmulc_add(x[0], x[16], w[16]))));
#define CHK_T(I) { const c2 p = cmulc(x[I], w[I]); n += differ(a[I + 16], fnet::w32b<+1, I>(twice_minus(p, cmulc_add(p, x[I + 16], w[I + 16])))); }
        CHK_T(1) CHK_T(2) CHK_T(3) CHK_T(4) CHK_T(5) CHK_T(6) CHK_T(7) CHK_T(8) CHK_T(9) CHK_T(10) CHK_T(11) CHK_T(12) CHK_T(13) CHK_T(14) CHK_T(15)
#undef CHK_T
    }
    {   // the junction's head: products with the reference spectrum folded into the first radix-4 butterfly
        c2 a = x[0], b = x[1], c = x[2], d = x[3];
        dft4_inv_mul(a, b, c, d, w[0], w[1], w[2], w[3]);
        const c2 pa = cmul(x[0], w[0]), t0 = cmul_add(pa, x[2], w[2]), t1 = twice_minus(pa, t0);
        const c2 pb = cmul(x[1], w[1]), t2 = cmul_add(pb, x[3], w[3]), u = twice_minus(pb, t2);
        n += differ(a, t0 + t2) + differ(c, t0 - t2) + differ(b, add_j<+1>(t1, u)) + differ(d, sub_j<+1>(t1, u));
    }
    {   // the first-index search: magnitudes and the maximum drawn from the 16 special values, so that matches (and NaN) are common
        const float wm = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(tab[hash(blockIdx.x) % 16])));
        float m[4];
        int ix[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { m[j] = tab[hash(id * 8 + j) % 16]; ix[j] = (int)(hash(id * 8 + 4 + j) & 0xffff); }
        int e = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < 4; ++j) e = (m[j] == wm) ? ix[j] : e;
        n += q_first4(0x7fffffff, wm, m[0], m[1], m[2], m[3], ix[0], ix[1], ix[2], ix[3]) != e;
    }
    if (n) atomicAdd(bad, n);
}
} // namespace grp

static int run_groups()
{
    std::vector<float> tab;
    const float sp[16] = {0.0f, -0.0f, INFINITY, -INFINITY, NAN, 1e-40f, -1e-40f, 1.4e-45f, 1.17549435e-38f, -1.17549421e-38f,
                          3.4e38f, -3.4e38f, 1.0f, -1.0f, 127.0f, -128.0f};
    for (float v : sp) tab.push_back(v);
    uint32_t st = 12345u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return (float)(st >> 8) * (1.0f / 16777216.0f); };
    for (int i = 0; i < 150; ++i) tab.push_back((rnd() - 0.5f) * 256.0f);                                 // K1's range
    for (int i = 0; i < 90; ++i) tab.push_back((rnd() - 0.5f) * std::ldexp(1.0f, (int)(rnd() * 200.0f) - 100));      // any exponent
    float *dt; int *dbad, hbad = -1;
    hipMalloc(&dt, tab.size() * 4); hipMalloc(&dbad, 4);
    hipMemcpy(dt, tab.data(), tab.size() * 4, hipMemcpyHostToDevice); hipMemset(dbad, 0, 4);
    grp::k_groups<<<256, 256>>>(dt, (int)tab.size(), dbad);
    if (hipMemcpy(&hbad, dbad, 4, hipMemcpyDeviceToHost) != hipSuccess) hbad = -1;
    printf("grouped forms: %d values drawn per thread x 65536 threads, mismatches %d\n", 128, hbad);
    hipFree(dt); hipFree(dbad);
    return hbad;
}

int main()
{
    c2 *p, *q; float *c; hipMalloc(&p, 256 * 8); hipMalloc(&q, 64 * 8); hipMalloc(&c, 64 * 8 * 4);
    c2 hp[256], hq[64]; for (int i = 0; i < 64; ++i) { hp[i] = c2{1.1f * i + 0.3f, -0.7f * i + 2.f}; hq[i] = c2{0.37f * i - 5.f, 0.11f * i * i + 1.f}; }
    hipMemcpy(p, hp, 64 * 8, hipMemcpyHostToDevice); hipMemcpy(q, hq, 64 * 8, hipMemcpyHostToDevice);
    prim::k<<<1, 64>>>(p, q, c); hipMemcpy(hp, p, 256 * 8, hipMemcpyDeviceToHost);
    float hc[512]; hipMemcpy(hc, c, sizeof(hc), hipMemcpyDeviceToHost);
    int bad = 0;
    for (int i = 0; i < 64; ++i) {
        bad += hp[i].x != hc[8 * i] || hp[i].y != hc[8 * i + 1];
        bad += hp[i + 64].x != hc[8 * i + 2] || hp[i + 64].y != hc[8 * i + 3];
        bad += hp[i + 128].x != hc[8 * i + 4] || hp[i + 128].y != hc[8 * i + 5];
        bad += hp[i + 192].x != hc[8 * i + 6] || hp[i + 192].y != hc[8 * i + 7];
    }
    const int gbad = run_groups();
    bad += gbad != 0;
    printf("mismatches %d\n", bad);
    return bad != 0;
}
