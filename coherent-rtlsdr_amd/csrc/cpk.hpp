// cpk.hpp -- complex fp32 arithmetic on packed register pairs (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32).
//
// Why: a wave of K1 can issue one VALU instruction every ~5 cycles whatever the other wave of its SIMD does
// (tools/valu_rate.hip: 2.1 ns per instruction for a lone wave, scalar or packed), and K1's row time is its
// per-wave instruction stream plus its LDS phases.  A packed instruction does two flops per lane for the same
// issue slot, so the complex add is ONE instruction instead of two and the complex multiply TWO instead of four.
// The compiler's own SLP packing loses that to ~900 v_mov per row (dead end 4 in DESIGN.md); here the data
// simply lives as (re, im) pairs from the LDS / HBM load to the store, and the operand modifiers of VOP3P
// (op_sel / op_sel_hi pick the half each lane reads, neg_lo / neg_hi negate per lane) do the swaps and signs
// that a complex product or a multiplication by +-i needs -- clang folds whole-vector shuffles and negations
// into them, per-lane negations it does not, hence the few inline-asm primitives.
// Every primitive rounds exactly like its scalar counterpart in fft_lds.hpp (checked bitwise, tools/pk_check).
#pragma once
#include <hip/hip_runtime.h>

namespace crsdr {

typedef float c2 __attribute__((ext_vector_type(2)));     // (re, im) in an aligned VGPR pair

__device__ __forceinline__ c2 mk(float x, float y) { return c2{x, y}; }
__device__ __forceinline__ c2 cadd(c2 a, c2 b) { return a + b; }
__device__ __forceinline__ c2 csub(c2 a, c2 b) { return a - b; }

// a * b:  (fma(a.x, b.x, -(a.y b.y)), fma(a.x, b.y, a.y b.x))
__device__ __forceinline__ c2 cmul(c2 a, c2 b)
{
    c2 t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0]" : "=v"(t) : "v"(a), "v"(b));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1] neg_lo:[0,0,1]" : "=v"(r) : "v"(a), "v"(b), "v"(t));
    return r;
}
// a * conj(b):  (fma(a.x, b.x, a.y b.y), fma(a.y, b.x, -(a.x b.y)))
__device__ __forceinline__ c2 cmulc(c2 a, c2 b)
{
    c2 t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "v"(b));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1] neg_hi:[0,0,1]" : "=v"(r) : "v"(a), "v"(b), "v"(t));
    return r;
}
template <int DIR>
__device__ __forceinline__ c2 ctw(c2 a, c2 w) { return DIR < 0 ? cmul(a, w) : cmulc(a, w); }

// c + a * conj(b) as two fused multiply-adds:  (fma(a.y, b.y, fma(a.x, b.x, c.x)),  fma(-a.x, b.y, fma(a.y, b.x, c.y)))
__device__ __forceinline__ c2 cmulc_add(c2 c, c2 a, c2 b)
{
    c2 r1, r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(r1) : "v"(a), "v"(b), "v"(c));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_hi:[1,0,0]" : "=v"(r) : "v"(a), "v"(b), "v"(r1));
    return r;
}
// c + a * b:  (fma(-a.y, b.y, fma(a.x, b.x, c.x)),  fma(a.x, b.y, fma(a.y, b.x, c.y)))
__device__ __forceinline__ c2 cmul_add(c2 c, c2 a, c2 b)
{
    c2 r1, r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(r1) : "v"(a), "v"(b), "v"(c));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]" : "=v"(r) : "v"(a), "v"(b), "v"(r1));
    return r;
}
// 2 p - s in one instruction: the difference of a radix-2 butterfly whose sum s = p + q is already there (q = s - p)
__device__ __forceinline__ c2 twice_minus(c2 p, c2 s)
{
    c2 r;
    asm("v_pk_fma_f32 %0, %1, 2.0, %2 op_sel_hi:[1,0,1] neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(r) : "v"(p), "v"(s));
    return r;
}

// ---- grouped forms: the same instructions for 2..4 independent values, breadth-first in ONE asm statement ----------------
// On gfx950 hipcc keeps one wait state (s_nop 0, an issue slot like any VALU instruction) between a packed instruction and
// a reader right behind it, and -- because it counts an asm statement as no wait state at all -- in front of any asm
// statement that reads what ANY asm statement wrote since the last instruction of its own ("wait
// states").  The single forms above put every product's second half right behind its first: a pad per product.  Here all
// first halves come before all second halves, so inside a statement no instruction reads what the one before it wrote (the
// author owns that: nothing pads inside the string; tools/k1_isa_count.py --hazards checks it), and the compiler's pad, if
// any, is one per statement.  Outputs are early-clobber (written before the last input is read) and double as the temp of
// their own value, so a group of n pins n output pairs beside its inputs.  Bits: tools/pk_check.hip, against the single forms.
#ifndef CRSDR_PK_GROUPS
#define CRSDR_PK_GROUPS 1      // 0: every grouped call runs the single forms one after the other (tools/pk_wait.hip's base arm)
#endif
#define CPK_MUL1(r, a, b) "v_pk_mul_f32 %" #r ", %" #a ", %" #b " op_sel:[1,1] op_sel_hi:[1,0]\n\t"
#define CPK_MUL2(r, a, b) "v_pk_fma_f32 %" #r ", %" #a ", %" #b ", %" #r " op_sel_hi:[0,1,1] neg_lo:[0,0,1]\n\t"
#define CPK_MULC1(r, a, b) "v_pk_mul_f32 %" #r ", %" #a ", %" #b " op_sel:[1,1] op_sel_hi:[0,1]\n\t"
#define CPK_MULC2(r, a, b) "v_pk_fma_f32 %" #r ", %" #a ", %" #b ", %" #r " op_sel_hi:[1,0,1] neg_hi:[0,0,1]\n\t"
// r[i] = a[i] * b[i] (CONJ: a[i] * conj(b[i])), i < 2 / 3 / 4
template <bool CONJ>
__device__ __forceinline__ void cmul_g2(c2 &r0, c2 &r1, c2 a0, c2 a1, c2 b0, c2 b1)
{
#if CRSDR_PK_GROUPS
    if constexpr (CONJ)
        asm(CPK_MULC1(0, 2, 4) CPK_MULC1(1, 3, 5) CPK_MULC2(0, 2, 4) CPK_MULC2(1, 3, 5)
            : "=&v"(r0), "=&v"(r1) : "v"(a0), "v"(a1), "v"(b0), "v"(b1));
    else
        asm(CPK_MUL1(0, 2, 4) CPK_MUL1(1, 3, 5) CPK_MUL2(0, 2, 4) CPK_MUL2(1, 3, 5)
            : "=&v"(r0), "=&v"(r1) : "v"(a0), "v"(a1), "v"(b0), "v"(b1));
#else
    r0 = CONJ ? cmulc(a0, b0) : cmul(a0, b0);
    r1 = CONJ ? cmulc(a1, b1) : cmul(a1, b1);
#endif
}
template <bool CONJ>
__device__ __forceinline__ void cmul_g3(c2 &r0, c2 &r1, c2 &r2, c2 a0, c2 a1, c2 a2, c2 b0, c2 b1, c2 b2)
{
#if CRSDR_PK_GROUPS
    if constexpr (CONJ)
        asm(CPK_MULC1(0, 3, 6) CPK_MULC1(1, 4, 7) CPK_MULC1(2, 5, 8) CPK_MULC2(0, 3, 6) CPK_MULC2(1, 4, 7) CPK_MULC2(2, 5, 8)
            : "=&v"(r0), "=&v"(r1), "=&v"(r2) : "v"(a0), "v"(a1), "v"(a2), "v"(b0), "v"(b1), "v"(b2));
    else
        asm(CPK_MUL1(0, 3, 6) CPK_MUL1(1, 4, 7) CPK_MUL1(2, 5, 8) CPK_MUL2(0, 3, 6) CPK_MUL2(1, 4, 7) CPK_MUL2(2, 5, 8)
            : "=&v"(r0), "=&v"(r1), "=&v"(r2) : "v"(a0), "v"(a1), "v"(a2), "v"(b0), "v"(b1), "v"(b2));
#else
    r0 = CONJ ? cmulc(a0, b0) : cmul(a0, b0);
    r1 = CONJ ? cmulc(a1, b1) : cmul(a1, b1);
    r2 = CONJ ? cmulc(a2, b2) : cmul(a2, b2);
#endif
}
template <bool CONJ>
__device__ __forceinline__ void cmul_g4(c2 &r0, c2 &r1, c2 &r2, c2 &r3, c2 a0, c2 a1, c2 a2, c2 a3, c2 b0, c2 b1, c2 b2, c2 b3)
{
#if CRSDR_PK_GROUPS
    if constexpr (CONJ)
        asm(CPK_MULC1(0, 4, 8) CPK_MULC1(1, 5, 9) CPK_MULC1(2, 6, 10) CPK_MULC1(3, 7, 11)
            CPK_MULC2(0, 4, 8) CPK_MULC2(1, 5, 9) CPK_MULC2(2, 6, 10) CPK_MULC2(3, 7, 11)
            : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3) : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(b0), "v"(b1), "v"(b2), "v"(b3));
    else
        asm(CPK_MUL1(0, 4, 8) CPK_MUL1(1, 5, 9) CPK_MUL1(2, 6, 10) CPK_MUL1(3, 7, 11)
            CPK_MUL2(0, 4, 8) CPK_MUL2(1, 5, 9) CPK_MUL2(2, 6, 10) CPK_MUL2(3, 7, 11)
            : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3) : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(b0), "v"(b1), "v"(b2), "v"(b3));
#else
    r0 = CONJ ? cmulc(a0, b0) : cmul(a0, b0);
    r1 = CONJ ? cmulc(a1, b1) : cmul(a1, b1);
    r2 = CONJ ? cmulc(a2, b2) : cmul(a2, b2);
    r3 = CONJ ? cmulc(a3, b3) : cmul(a3, b3);
#endif
}
// v[pos(K + i)] *= w[K + i] (CONJ: its conjugate) for K <= K + i < END, four at a time
template <bool CONJ, int K, int END, class POS>
__device__ __forceinline__ void cmul_run(c2 *v, const c2 *w, POS pos)
{
    if constexpr (END - K >= 4) {
        c2 r0, r1, r2, r3;
        cmul_g4<CONJ>(r0, r1, r2, r3, v[pos(K)], v[pos(K + 1)], v[pos(K + 2)], v[pos(K + 3)], w[K], w[K + 1], w[K + 2], w[K + 3]);
        v[pos(K)] = r0; v[pos(K + 1)] = r1; v[pos(K + 2)] = r2; v[pos(K + 3)] = r3;
        cmul_run<CONJ, K + 4, END>(v, w, pos);
    } else if constexpr (END - K == 3) {
        c2 r0, r1, r2;
        cmul_g3<CONJ>(r0, r1, r2, v[pos(K)], v[pos(K + 1)], v[pos(K + 2)], w[K], w[K + 1], w[K + 2]);
        v[pos(K)] = r0; v[pos(K + 1)] = r1; v[pos(K + 2)] = r2;
    } else if constexpr (END - K == 2) {
        c2 r0, r1;
        cmul_g2<CONJ>(r0, r1, v[pos(K)], v[pos(K + 1)], w[K], w[K + 1]);
        v[pos(K)] = r0; v[pos(K + 1)] = r1;
    } else if constexpr (END - K == 1) {
        v[pos(K)] = CONJ ? cmulc(v[pos(K)], w[K]) : cmul(v[pos(K)], w[K]);
    }
}

// The head of an inverse pass for two independent values: p = a w (CONJ: a conj(w)), s = p + b x (b conj(x)) as two fused
// multiply-adds, t = 2 p - s -- cmul / cmul_add / twice_minus (cmulc / cmulc_add / twice_minus) instruction for instruction,
// five deep and two wide.  p lives in t's registers.
#define CPK_ADD1(r, a, b, c) "v_pk_fma_f32 %" #r ", %" #a ", %" #b ", %" #c " op_sel_hi:[1,0,1]\n\t"
#define CPK_ADD2(r, a, b) "v_pk_fma_f32 %" #r ", %" #a ", %" #b ", %" #r " op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]\n\t"
#define CPK_ADDC2(r, a, b) "v_pk_fma_f32 %" #r ", %" #a ", %" #b ", %" #r " op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_hi:[1,0,0]\n\t"
#define CPK_TWM(r, s) "v_pk_fma_f32 %" #r ", %" #r ", 2.0, %" #s " op_sel_hi:[1,0,1] neg_lo:[0,0,1] neg_hi:[0,0,1]\n\t"
template <bool CONJ>
__device__ __forceinline__ void head_g2(c2 &s0, c2 &s1, c2 &t0, c2 &t1, c2 a0, c2 a1, c2 w0, c2 w1, c2 b0, c2 b1, c2 x0, c2 x1)
{
#if CRSDR_PK_GROUPS
    //                 %0 %1 %2 %3        %4 %5 %6 %7 %8 %9 %10 %11
    if constexpr (CONJ)
        asm(CPK_MULC1(2, 4, 6) CPK_MULC1(3, 5, 7) CPK_MULC2(2, 4, 6) CPK_MULC2(3, 5, 7)
            CPK_ADD1(0, 8, 10, 2) CPK_ADD1(1, 9, 11, 3) CPK_ADDC2(0, 8, 10) CPK_ADDC2(1, 9, 11) CPK_TWM(2, 0) CPK_TWM(3, 1)
            : "=&v"(s0), "=&v"(s1), "=&v"(t0), "=&v"(t1)
            : "v"(a0), "v"(a1), "v"(w0), "v"(w1), "v"(b0), "v"(b1), "v"(x0), "v"(x1));
    else
        asm(CPK_MUL1(2, 4, 6) CPK_MUL1(3, 5, 7) CPK_MUL2(2, 4, 6) CPK_MUL2(3, 5, 7)
            CPK_ADD1(0, 8, 10, 2) CPK_ADD1(1, 9, 11, 3) CPK_ADD2(0, 8, 10) CPK_ADD2(1, 9, 11) CPK_TWM(2, 0) CPK_TWM(3, 1)
            : "=&v"(s0), "=&v"(s1), "=&v"(t0), "=&v"(t1)
            : "v"(a0), "v"(a1), "v"(w0), "v"(w1), "v"(b0), "v"(b1), "v"(x0), "v"(x1));
#else
    const c2 p0 = CONJ ? cmulc(a0, w0) : cmul(a0, w0);
    s0 = CONJ ? cmulc_add(p0, b0, x0) : cmul_add(p0, b0, x0);
    t0 = twice_minus(p0, s0);
    const c2 p1 = CONJ ? cmulc(a1, w1) : cmul(a1, w1);
    s1 = CONJ ? cmulc_add(p1, b1, x1) : cmul_add(p1, b1, x1);
    t1 = twice_minus(p1, s1);
#endif
}

// a + (-i) x = (a.x + x.y, a.y - x.x)      a - (-i) x = (a.x - x.y, a.y + x.x)
__device__ __forceinline__ c2 add_mi(c2 a, c2 x)
{
    c2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(x));
    return r;
}
__device__ __forceinline__ c2 sub_mi(c2 a, c2 x)
{
    c2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(x));
    return r;
}
// a +- exp(DIR i pi/2) x  (forward: -i, backward: +i)
template <int DIR> __device__ __forceinline__ c2 add_j(c2 a, c2 x) { return DIR < 0 ? add_mi(a, x) : sub_mi(a, x); }
template <int DIR> __device__ __forceinline__ c2 sub_j(c2 a, c2 x) { return DIR < 0 ? sub_mi(a, x) : add_mi(a, x); }
// exp(DIR i pi/2) x on its own: one multiplication by (+-1, -+1) with the halves swapped (exact)
template <int DIR>
__device__ __forceinline__ c2 mul_j(c2 x)
{
    c2 r;
    if constexpr (DIR < 0) asm("v_pk_mul_f32 %0, %1, 1.0 op_sel:[1,0] op_sel_hi:[0,0] neg_hi:[0,1]" : "=v"(r) : "v"(x));   // (x.y, -x.x)
    else asm("v_pk_mul_f32 %0, %1, 1.0 op_sel:[1,0] op_sel_hi:[0,0] neg_lo:[0,1]" : "=v"(r) : "v"(x));                     // (-x.y, x.x)
    return r;
}

// a * (c -+ i s): forward (DIR < 0)  (fma(a.x, c, a.y s), fma(a.y, c, -(a.x s)));  backward the conjugate
template <int DIR>
__device__ __forceinline__ c2 rot_cs(c2 a, float c, float s)
{
    const c2 cc = c2{c, c}, ss = c2{s, s};
    c2 u, r;
    if constexpr (DIR < 0) asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[0,0] neg_hi:[0,1]" : "=v"(u) : "v"(a), "s"(ss));  // (a.y s, -a.x s)
    else asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[0,0] neg_lo:[0,1]" : "=v"(u) : "v"(a), "s"(ss));                    // (-a.y s, a.x s)
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "s"(cc), "v"(u));
    return r;
}

constexpr float kPkSqrtHalf = 0.70710678118654752440f;
constexpr float kPkC1 = 0.92387953251128675613f; // cos(pi/8)
constexpr float kPkS1 = 0.38268343236508977173f; // sin(pi/8)

// multiply by W_16^K (forward: exp(-2 pi i K/16); backward: conjugate), K in {0,1,2,3,4,6,9}
template <int DIR, int K>
__device__ __forceinline__ c2 mul_w16(c2 a)
{
    if constexpr (K == 0) return a;
    else if constexpr (K == 4) return mul_j<DIR>(a);
    else if constexpr (K == 2) {
        // forward ((a.x + a.y) k, (a.y - a.x) k);  backward ((a.x - a.y) k, (a.x + a.y) k)
        const c2 t = DIR < 0 ? add_mi(a, a) : sub_mi(a, a);
        return t * kPkSqrtHalf;
    } else if constexpr (K == 6) {
        // forward ((a.y - a.x) k, -(a.x + a.y) k);  backward (-(a.x + a.y) k, (a.x - a.y) k)
        const c2 t = DIR < 0 ? sub_mi(a, a) : add_mi(a, a);
        return t * (-kPkSqrtHalf);
    } else {
        constexpr float c = (K == 1) ? kPkC1 : (K == 3) ? kPkS1 : (K == 9) ? -kPkC1 : 0.f;
        constexpr float s = (K == 1) ? kPkS1 : (K == 3) ? kPkC1 : (K == 9) ? -kPkS1 : 0.f;
        static_assert(K == 1 || K == 3 || K == 9, "unsupported W16 power");
        return rot_cs<DIR>(a, c, s);
    }
}

// natural-order 4-point DFT of (a,b,c,d) in place
template <int DIR>
__device__ __forceinline__ void dft4(c2 &a, c2 &b, c2 &c, c2 &d)
{
    const c2 t0 = a + c, t1 = a - c, t2 = b + d, u = b - d;
    a = t0 + t2;
    c = t0 - t2;
    b = add_j<DIR>(t1, u);
    d = sub_j<DIR>(t1, u);
}

template <int DIR>
__device__ __forceinline__ void dft16(c2 *v)
{
    // n = q + 4m, k = s + 4u:  X[s+4u] = sum_q W4^{qu} ( W16^{qs} sum_m v[q+4m] W4^{ms} )
    dft4<DIR>(v[0], v[4], v[8], v[12]);
    dft4<DIR>(v[1], v[5], v[9], v[13]);
    dft4<DIR>(v[2], v[6], v[10], v[14]);
    dft4<DIR>(v[3], v[7], v[11], v[15]);
    v[5] = mul_w16<DIR, 1>(v[5]);
    v[9] = mul_w16<DIR, 2>(v[9]);
    v[13] = mul_w16<DIR, 3>(v[13]);
    v[6] = mul_w16<DIR, 2>(v[6]);
    v[10] = mul_w16<DIR, 4>(v[10]);
    v[14] = mul_w16<DIR, 6>(v[14]);
    v[7] = mul_w16<DIR, 3>(v[7]);
    v[11] = mul_w16<DIR, 6>(v[11]);
    v[15] = mul_w16<DIR, 9>(v[15]);
    dft4<DIR>(v[0], v[1], v[2], v[3]);
    dft4<DIR>(v[4], v[5], v[6], v[7]);
    dft4<DIR>(v[8], v[9], v[10], v[11]);
    dft4<DIR>(v[12], v[13], v[14], v[15]);
    c2 t;
    t = v[1]; v[1] = v[4]; v[4] = t;
    t = v[2]; v[2] = v[8]; v[8] = t;
    t = v[3]; v[3] = v[12]; v[12] = t;
    t = v[6]; v[6] = v[9]; v[9] = t;
    t = v[7]; v[7] = v[13]; v[13] = t;
    t = v[11]; v[11] = v[14]; v[14] = t;
}

// Junction of the cross-correlation: u[i] * r[i] (the conjugated reference spectrum) followed by the inverse 16-point DFT,
// with the products folded into the first radix-4 stage:  t0 = a ra + c rc as p = a ra, t0 = p + c rc (two fused
// multiply-adds), t1 = a ra - c rc = 2 p - t0 -- 10 packed instructions per radix-4 butterfly head instead of 12.
__device__ __forceinline__ void dft4_inv_mul(c2 &a, c2 &b, c2 &c, c2 &d, c2 ra, c2 rb, c2 rc, c2 rd)
{
    c2 t0, t1, t2, u;      // pa = a ra, t0 = pa + c rc, t1 = 2 pa - t0;  pb = b rb, t2 = pb + d rd, u = 2 pb - t2
    head_g2<false>(t0, t2, t1, u, a, b, ra, rb, c, d, rc, rd);
    a = t0 + t2;
    c = t0 - t2;
    b = add_j<+1>(t1, u);
    d = sub_j<+1>(t1, u);
}
__device__ __forceinline__ void dft16_inv_mul(c2 *v, const c2 *r)
{
    dft4_inv_mul(v[0], v[4], v[8], v[12], r[0], r[4], r[8], r[12]);
    dft4_inv_mul(v[1], v[5], v[9], v[13], r[1], r[5], r[9], r[13]);
    dft4_inv_mul(v[2], v[6], v[10], v[14], r[2], r[6], r[10], r[14]);
    dft4_inv_mul(v[3], v[7], v[11], v[15], r[3], r[7], r[11], r[15]);
    v[5] = mul_w16<+1, 1>(v[5]);
    v[9] = mul_w16<+1, 2>(v[9]);
    v[13] = mul_w16<+1, 3>(v[13]);
    v[6] = mul_w16<+1, 2>(v[6]);
    v[10] = mul_w16<+1, 4>(v[10]);
    v[14] = mul_w16<+1, 6>(v[14]);
    v[7] = mul_w16<+1, 3>(v[7]);
    v[11] = mul_w16<+1, 6>(v[11]);
    v[15] = mul_w16<+1, 9>(v[15]);
    dft4<+1>(v[0], v[1], v[2], v[3]);
    dft4<+1>(v[4], v[5], v[6], v[7]);
    dft4<+1>(v[8], v[9], v[10], v[11]);
    dft4<+1>(v[12], v[13], v[14], v[15]);
    c2 t;
    t = v[1]; v[1] = v[4]; v[4] = t;
    t = v[2]; v[2] = v[8]; v[8] = t;
    t = v[3]; v[3] = v[12]; v[12] = t;
    t = v[6]; v[6] = v[9]; v[9] = t;
    t = v[7]; v[7] = v[13]; v[13] = t;
    t = v[11]; v[11] = v[14]; v[14] = t;
}

// ---- FMA-form network (K0 / K1 at B = 16384) -------------------------------------------------------------------------
// A non-trivial twiddle costs two packed instructions as a product (rot_cs) and the butterfly after it two more.  Factored as
//     w = c (1 + i t)            (|t| <= 1)      or      w = i s (1 - i t')      (|t'| < 1)
// the bracket is ONE v_pk_fma_f32 (x + t (i x), the swap and sign by op_sel / neg), and the real factor c (or i s) is not
// applied: the value carries it as a compile-time scale r i^k (true value = r i^k stored value), and the butterfly that
// combines two values folds the ratio of their scales into its fused multiply-adds -- a +- (sb / sa) b is one v_pk_fma_f32,
// the cost of the add it replaces.  A radix-4 butterfly leaves every output with the scale of its input a, so a 16-point
// transform (4 x 4) ends with the scale of its input 0 -- 1 in every transform below: no scale leaves a transform.
// Every constant is a compile-time value in an SGPR pair (VOP3P on gfx950 takes no literal; op_sel_hi = 0 reads the low half
// in both lanes); a ratio of exactly 1 is a plain v_pk_add_f32 and needs none.  Same data flow, same registers, rounding
// differs from the product form in the last bits (tools/fma_bfly_check.hip checks each primitive against its scalar formula).

// a + i^K r b, one instruction:  K = 0 (a.x + r b.x, a.y + r b.y)   1 (a.x - r b.y, a.y + r b.x)   2 (a.x - r b.x, a.y - r b.y)
// 3 (a.x + r b.y, a.y - r b.x), each lane one fmaf (r = 1: one v_pk_add_f32, which rounds the same)
template <int K>
__device__ __forceinline__ c2 fma_j(c2 a, c2 b, float r)
{
    constexpr int k = K & 3;
    c2 d;
    if (r == 1.0f) {
        if constexpr (k == 0) return a + b;
        else if constexpr (k == 2) return a - b;
        else if constexpr (k == 1) return sub_mi(a, b);
        else return add_mi(a, b);
    }
    const c2 rr = c2{r, r};
    if constexpr (k == 0) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(d) : "s"(rr), "v"(b), "v"(a));
    else if constexpr (k == 2) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]" : "=v"(d) : "s"(rr), "v"(b), "v"(a));
    else if constexpr (k == 1) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[0,0,1] neg_lo:[1,0,0]" : "=v"(d) : "s"(rr), "v"(b), "v"(a));
    else asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[0,0,1] neg_hi:[1,0,0]" : "=v"(d) : "s"(rr), "v"(b), "v"(a));
    return d;
}

namespace fnet {

struct Sc { double r; int k; };                                   // the scale r i^k, r > 0
constexpr Sc kOne{1.0, 0};
constexpr Sc sc_mul(Sc a, Sc b) { return Sc{a.r * b.r, (a.k + b.k) & 3}; }
constexpr Sc sc_div(Sc a, Sc b) { return Sc{a.r / b.r, (a.k - b.k) & 3}; }
constexpr bool sc_is_one(Sc a) { return a.r == 1.0 && a.k == 0; }
// cos (pi m / 16) for any integer m
constexpr double kCosPi16[9] = {1.0, 0.98078528040323044913, 0.92387953251128675613, 0.83146961230254523708, 0.70710678118654752440,
                                0.55557023301960222474, 0.38268343236508977173, 0.19509032201612826785, 0.0};
constexpr double cos16(int m)
{
    m = ((m % 32) + 32) % 32;
    return m <= 8 ? kCosPi16[m] : m <= 16 ? -kCosPi16[16 - m] : m <= 24 ? -kCosPi16[m - 16] : kCosPi16[32 - m];
}
constexpr double sin16(int m) { return cos16(m - 8); }
constexpr double dabs(double x) { return x < 0 ? -x : x; }
// exp(i pi m / 16) = scale * (1 + i^mk * mr):  the factoring with the larger of |cos|, |sin| as the scale (mr = 0: no bracket)
struct Tw { Sc scale; int mk; double mr; };
constexpr Tw tw16(int m)
{
    const double c = cos16(m), s = sin16(m);
    if (dabs(c) >= dabs(s)) return Tw{Sc{dabs(c), c < 0 ? 2 : 0}, s / c >= 0 ? 1 : 3, dabs(s / c)};
    return Tw{Sc{dabs(s), s > 0 ? 1 : 3}, c / s >= 0 ? 3 : 1, dabs(c / s)};
}
// W_32^n (forward exp(-2 pi i n / 32), DIR > 0 its conjugate) and W_16^n
template <int DIR> constexpr Tw w32(int n) { return tw16(DIR < 0 ? -n : n); }
template <int DIR> constexpr Tw w16(int n) { return tw16(DIR < 0 ? -2 * n : 2 * n); }

// x (1 + i^mk mr): the bracket of the twiddle W_32^N / W_16^N (the scale of w32 / w16), one instruction or none
template <int MK>
__device__ __forceinline__ c2 bracket(c2 x, double mr) { return mr == 0.0 ? x : fma_j<MK>(x, x, (float)mr); }
template <int DIR, int N> __device__ __forceinline__ c2 w32b(c2 x) { return bracket<w32<DIR>(N).mk>(x, w32<DIR>(N).mr); }
template <int DIR, int N> __device__ __forceinline__ c2 w16b(c2 x) { return bracket<w16<DIR>(N).mk>(x, w16<DIR>(N).mr); }

// the combination a + sign * (sb / sa) b with the fixed factor i^J: a + i^(J + kb - ka) (rb / ra) b
template <int J, class SA, class SB>
__device__ __forceinline__ c2 comb(c2 a, c2 b)
{
    constexpr Sc q = sc_div(SB::value, SA::value);
    return fma_j<J + q.k>(a, b, (float)q.r);
}
// a compile-time scale as a type (C++17: no floating-point template arguments)
template <class T, int I> struct At { static constexpr Sc value = T::at(I); };

// radix-4 butterfly on scaled inputs (a, b, c, d) at scale indices (IA, IB, IC, ID) of S; the outputs carry scale IA
template <int DIR, class S, int IA, int IB, int IC, int ID>
__device__ __forceinline__ void dft4s(c2 &a, c2 &b, c2 &c, c2 &d)
{
    using A = At<S, IA>; using B = At<S, IB>; using C = At<S, IC>; using D = At<S, ID>;
    const c2 t0 = comb<0, A, C>(a, c), t1 = comb<2, A, C>(a, c);
    const c2 t2 = comb<0, B, D>(b, d), u = comb<2, B, D>(b, d);       // scale B
    a = comb<0, A, B>(t0, t2);
    c = comb<2, A, B>(t0, t2);
    b = comb<DIR < 0 ? 3 : 1, A, B>(t1, u);                           // t1 + exp(DIR i pi/2) u
    d = comb<DIR < 0 ? 1 : 3, A, B>(t1, u);
}

// the scales after the first radix-4 layer and the twiddle brackets of a 16-point transform whose inputs have scales S
template <int DIR, class S>
struct Mid16 {
    // element 4 s + q (before the swap) is output s of group q times W16^(q s)
    static constexpr Sc at(int i) { return sc_mul(S::at(i & 3), w16<DIR>((i & 3) * (i >> 2)).scale); }
};
struct Unit { static constexpr Sc at(int) { return kOne; } };

// second layer of dft16 (mid-twiddle brackets, radix-4 on the scaled values, the output permutation); first-layer scales S
template <int DIR, class S>
__device__ __forceinline__ void dft16s_tail(c2 *v)
{
    static_assert(sc_is_one(S::at(0)), "a 16-point transform must end unscaled");
    using M = Mid16<DIR, S>;
    v[5] = w16b<DIR, 1>(v[5]);
    v[9] = w16b<DIR, 2>(v[9]);
    v[13] = w16b<DIR, 3>(v[13]);
    v[6] = w16b<DIR, 2>(v[6]);
    v[10] = w16b<DIR, 4>(v[10]);
    v[14] = w16b<DIR, 6>(v[14]);
    v[7] = w16b<DIR, 3>(v[7]);
    v[11] = w16b<DIR, 6>(v[11]);
    v[15] = w16b<DIR, 9>(v[15]);
    // v[4 s + q] now holds first-layer output s of group q (scale S::at(q) * W16^(q s)'s scale = M::at(4 s + q))
    dft4s<DIR, M, 0, 1, 2, 3>(v[0], v[1], v[2], v[3]);
    dft4s<DIR, M, 4, 5, 6, 7>(v[4], v[5], v[6], v[7]);
    dft4s<DIR, M, 8, 9, 10, 11>(v[8], v[9], v[10], v[11]);
    dft4s<DIR, M, 12, 13, 14, 15>(v[12], v[13], v[14], v[15]);
    c2 t;
    t = v[1]; v[1] = v[4]; v[4] = t;
    t = v[2]; v[2] = v[8]; v[8] = t;
    t = v[3]; v[3] = v[12]; v[12] = t;
    t = v[6]; v[6] = v[9]; v[9] = t;
    t = v[7]; v[7] = v[13]; v[13] = t;
    t = v[11]; v[11] = v[14]; v[14] = t;
}

// 16-point transform of inputs with scales S (S::at(0) = 1), unscaled outputs in dft16's order
template <int DIR, class S = Unit>
__device__ __forceinline__ void dft16s(c2 *v)
{
    dft4s<DIR, S, 0, 4, 8, 12>(v[0], v[4], v[8], v[12]);
    dft4s<DIR, S, 1, 5, 9, 13>(v[1], v[5], v[9], v[13]);
    dft4s<DIR, S, 2, 6, 10, 14>(v[2], v[6], v[10], v[14]);
    dft4s<DIR, S, 3, 7, 11, 15>(v[3], v[7], v[11], v[15]);
    dft16s_tail<DIR, S>(v);
}
// dft16_inv_mul with the FMA-form second layer: the products and the first layer as dft4_inv_mul (unscaled outputs)
__device__ __forceinline__ void dft16s_inv_mul(c2 *v, const c2 *r)
{
    dft4_inv_mul(v[0], v[4], v[8], v[12], r[0], r[4], r[8], r[12]);
    dft4_inv_mul(v[1], v[5], v[9], v[13], r[1], r[5], r[9], r[13]);
    dft4_inv_mul(v[2], v[6], v[10], v[14], r[2], r[6], r[10], r[14]);
    dft4_inv_mul(v[3], v[7], v[11], v[15], r[3], r[7], r[11], r[15]);
    dft16s_tail<+1, Unit>(v);
}

} // namespace fnet
} // namespace crsdr
