// esprit.hpp -- gridless directions (crsdr_doa_set_esprit, crsdr_esprit2d): 2-D ESPRIT on the signal subspace of a uniform rectangular
// array.  No grid, no search, no peak picking: k-by-k linear algebra per matrix, whatever ncx and ncy are.
//
// The definition (include/crsdr.h has the same words).  Per matrix: vec [M][M] fp32 (column r = v_r) and sv as published, k_e sources,
// the array SX x SY (element i = iy SX + ix), (double)d; everything in fp64:
//     E = the first k_e columns of vec;  E1x / E2x its rows with ix <= SX-2 / ix >= 1, paired (ix, iy) -> (ix+1, iy);  E1y / E2y along y
//     Gx = E1x^H E1x, Hx = E1x^H E2x, Psi_x = Gx^-1 Hx by Cholesky;  Psi_y likewise;  Psi_c = Psi_x + gamma Psi_y, gamma = (1 + j) / 2
//     Psi_c V = V diag(w);  lambda_x_i = (V^-1 Psi_x V)_ii, lambda_y_i = (V^-1 Psi_y V)_ii;  mu_i = arg lambda_x_i, nu_i = arg lambda_y_i
//     cb = nu / (2 pi d), clamped (flag bit 0);  sb = sqrt(1 - cb^2);  ca = sb > 0 ? mu / (2 pi d sb) : 0, clamped (flag bit 1, also
//     when sb == 0);  beta = acos(cb), alpha = acos(ca);  power_i = sum_r sv[r] |v_r^H a_i|^2 / M^2 with k_doa_beam_weights' a
//     slots by descending power, then ascending mu, then nu;  found = k_e, or 0: sv[0] == 0 (status 0), a Cholesky pivot <= 2^-40
//     (status bit 1), the eigenvalue iteration not finished within 40 k_e steps (status bit 0)
//     empty slots: phases (0, 0), angles (-1, -1), modulus (-1, -1), power -1, flags 0
//
// Shape.  One wave per matrix; the matrices of a batch run side by side, the kernel is a latency chain like k_doa_subspace.  Every k x k
// matrix lies in LDS as [16][16] complex fp64.
//   Gram      the 4 k^2 entries of Gx, Hx, Gy, Hy spread over the lanes, each a sum over the rows in ascending order
//   Cholesky  lanes 0..15 hold the rows of Gx, lanes 32..47 those of Gy (left-looking, a column per step); then a lane owns a column of H
//             and runs both substitutions on it without a barrier
//   Schur     Psi_c to Hessenberg form by Householder reflections (a lane per column from the left, per row from the right), then explicit
//             shifted QR steps: Wilkinson's shift, the Givens rotations from the left one after the other (a lane per column), their
//             transposes from the right with a lane per row of T (lanes 0..15) and of Q (lanes 32..47) and no barrier between them;
//             deflation from the bottom
//   V         Y = the triangular factor's eigenvectors by back substitution (a lane per eigenvector), V = Q Y is never formed:
//             lambda_i = entry i of the solution z of Y z = (Q^H Psi Q) y_i, lanes 0..15 for x and 32..47 for y
//   power     per slot: a lane per element forms a, a lane per column r its term (lanes as r, as k_doa_beam_weights), added in order of r
// Every branch around a barrier depends on values all lanes read from the same LDS words: uniform.  No atomics: the same bits wherever a
// matrix stands in a batch, and in the per-op kernel.
//   LDS: 40 KiB of matrices (E's 16 KiB are T, Q and Y afterwards; G's are the substitution vectors) + 3 KiB: three workgroups per CU.
#pragma once
#ifndef CRSDR_ESPRIT_HOST_THREADS      // tools/esprit_cpu.cc: the device function on 64 host threads, its own stand-ins for the HIP words
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

namespace crsdr {
namespace esprit {

constexpr int MAX_M = 64, MAX_K = 16, ES_WAVES = 1, ES_THREADS = 64 * ES_WAVES, LD = 16, MAT = LD * LD;
enum { STATUS_ITERATIONS = 1, STATUS_PIVOT = 2, FLAG_BETA = 1, FLAG_ALPHA = 2 };

typedef double2 cd;
__device__ __forceinline__ cd cmk(double x, double y) { return make_double2(x, y); }
__device__ __forceinline__ cd cadd(cd a, cd b) { return cmk(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ cd csub(cd a, cd b) { return cmk(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ cd cmul(cd a, cd b) { return cmk(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ cd cmulc(cd a, cd b) { return cmk(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x); }        // conj(a) b
__device__ __forceinline__ cd cconj(cd a) { return cmk(a.x, -a.y); }
__device__ __forceinline__ cd cscale(cd a, double s) { return cmk(a.x * s, a.y * s); }
__device__ __forceinline__ double cabs2(cd a) { return a.x * a.x + a.y * a.y; }
__device__ __forceinline__ double cabs1(cd a) { return sqrt(cabs2(a)); }
__device__ __forceinline__ cd cdiv(cd a, cd b) { const double q = 1.0 / cabs2(b); return cmk((a.x * b.x + a.y * b.y) * q, (a.y * b.x - a.x * b.y) * q); }
// acc += a b, acc += conj(a) b
__device__ __forceinline__ void cfma(cd &acc, cd a, cd b) { acc.x = fma(a.x, b.x, fma(-a.y, b.y, acc.x)); acc.y = fma(a.x, b.y, fma(a.y, b.x, acc.y)); }
__device__ __forceinline__ void cfmac(cd &acc, cd a, cd b) { acc.x = fma(a.x, b.x, fma(a.y, b.y, acc.x)); acc.y = fma(a.x, b.y, fma(-a.y, b.x, acc.y)); }
__device__ __forceinline__ cd csqrt_(cd z)
{
    const double m = cabs1(z);
    if (m == 0.0) return cmk(0.0, 0.0);
    const double t = sqrt(0.5 * (m + fabs(z.x)));
    return z.x >= 0.0 ? cmk(t, z.y / (2.0 * t)) : cmk(fabs(z.y) / (2.0 * t), z.y >= 0.0 ? t : -t);
}

// One matrix, by the 64 threads of a workgroup.  vec [M][M], sv [M] of this matrix; ke its source count; the outputs of this matrix:
// phases, angles, modulus [slots][2], power, flags [slots], found and status one word each.  1 <= slots <= MAX_K, M = SX SY <= MAX_M,
// ke <= min((SX-1) SY, SX (SY-1)) (the callers check); a ke outside 1 .. slots leaves found = 0.
__device__ void esprit2d_matrix(const float2 *__restrict__ vec, const float *__restrict__ sv, int M, int ke, float d, int SX, int SY, int slots,
                                int32_t *__restrict__ found, int32_t *__restrict__ status, double *__restrict__ phases, float *__restrict__ angles,
                                float *__restrict__ modulus, float *__restrict__ power, int32_t *__restrict__ flags)
{
    __shared__ cd sA[4 * MAT];                       // E [M][LD]; then T, Q, Y
    __shared__ cd sG[2 * MAT], sP[2 * MAT], sS[2 * MAT];
    __shared__ cd hv[MAX_K], rot[MAX_K], lam[2 * MAX_K], sa[MAX_M];
    __shared__ double sred[MAX_M], skey[3 * MAX_K];
    const int lane = threadIdx.x, h = lane >> 5, l = lane & 31;
    cd *E = sA, *T = sA, *Q = sA + MAT, *Y = sA + 2 * MAT, *Z = sG;
    const int k = ke, kk = k * k;
    int st = 0;
    bool ok = k >= 1 && k <= slots && k <= MAX_K && (double)sv[0] != 0.0;

    if (ok) {
        for (int idx = lane; idx < M * k; idx += ES_THREADS) {
            const int i = idx / k, c = idx - i * k;
            const float2 v = vec[(size_t)i * M + c];
            E[i * LD + c] = cmk((double)v.x, (double)v.y);
        }
        __syncthreads();
        // ---- the four Gram products ----
        for (int idx = lane; idx < 4 * kk; idx += ES_THREADS) {
            const int which = idx / kk, ab = idx - which * kk, a = ab / k, b = ab - a * k;
            const bool y = which >= 2, shifted = which & 1;
            const int nx = y ? SX : SX - 1, ny = y ? SY - 1 : SY, step = shifted ? (y ? SX : 1) : 0;
            cd acc = cmk(0.0, 0.0);
            for (int iy = 0; iy < ny; ++iy)
                for (int ix = 0; ix < nx; ++ix) {
                    const int i = iy * SX + ix;
                    cfmac(acc, E[i * LD + a], E[(i + step) * LD + b]);
                }
            (shifted ? sP : sG)[(y ? MAT : 0) + a * LD + b] = acc;
        }
        __syncthreads();
        // ---- Cholesky of Gx (lanes 0..) and Gy (lanes 32..): L in the lower triangle, in place ----
        cd *G = sG + h * MAT;
        for (int j = 0; j < k; ++j) {
            double p = G[j * LD + j].x;
            for (int q = 0; q < j; ++q) p -= cabs2(G[j * LD + q]);
            if (__any(!(p > 0x1p-40))) { st = STATUS_PIVOT; ok = false; break; }
            const double dj = sqrt(p);
            if (l > j && l < k) {
                cd acc = G[l * LD + j];
                for (int q = 0; q < j; ++q) { const cd t = cmulc(G[j * LD + q], G[l * LD + q]); acc = csub(acc, t); }
                G[l * LD + j] = cscale(acc, 1.0 / dj);
            }
            __syncthreads();                                             // (every lane has read G[j][j] before it becomes L[j][j])
            if (l == j) G[j * LD + j] = cmk(dj, 0.0);
            __syncthreads();
        }
    }
    if (ok) {
        cd *G = sG + h * MAT, *P = sP + h * MAT;
        // ---- Psi = G^-1 H: a lane per column of H, L y = h then L^H x = y ----
        if (l < k) {
            for (int i = 0; i < k; ++i) {
                cd acc = P[i * LD + l];
                for (int q = 0; q < i; ++q) { const cd t = cmul(G[i * LD + q], P[q * LD + l]); acc = csub(acc, t); }
                P[i * LD + l] = cscale(acc, 1.0 / G[i * LD + i].x);
            }
            for (int i = k - 1; i >= 0; --i) {
                cd acc = P[i * LD + l];
                for (int q = i + 1; q < k; ++q) { const cd t = cmulc(G[q * LD + i], P[q * LD + l]); acc = csub(acc, t); }
                P[i * LD + l] = cscale(acc, 1.0 / G[i * LD + i].x);
            }
        }
        __syncthreads();
        // ---- T = Psi_x + gamma Psi_y, Q = I (E is done with) ----
        for (int idx = lane; idx < kk; idx += ES_THREADS) {
            const int a = idx / k, b = idx - a * k;
            const cd px = sP[a * LD + b], py = sP[MAT + a * LD + b];
            T[a * LD + b] = cmk(px.x + 0.5 * (py.x - py.y), px.y + 0.5 * (py.x + py.y));
            Q[a * LD + b] = cmk(a == b ? 1.0 : 0.0, 0.0);
        }
        __syncthreads();
        // ---- Hessenberg form: a Householder reflection per column ----
        for (int j = 0; j + 2 < k; ++j) {
            const int len = k - j - 1;
            const cd x0 = T[(j + 1) * LD + j];
            double tail = 0.0;
            for (int r = 1; r < len; ++r) tail += cabs2(T[(j + 1 + r) * LD + j]);
            if (tail == 0.0) continue;                                   // (uniform: every lane read the same words)
            const double a0 = cabs1(x0), nx = sqrt(a0 * a0 + tail);
            const cd ph = a0 != 0.0 ? cscale(x0, 1.0 / a0) : cmk(1.0, 0.0);
            const cd v0 = cadd(x0, cscale(ph, nx));
            const double inv = 1.0 / sqrt(cabs2(v0) + tail);
            if (lane < len) hv[lane] = cscale(lane == 0 ? v0 : T[(j + 1 + lane) * LD + j], inv);
            __syncthreads();
            if (lane < k) {                                              // from the left: column `lane`
                cd w = cmk(0.0, 0.0);
                for (int r = 0; r < len; ++r) cfmac(w, hv[r], T[(j + 1 + r) * LD + lane]);
                w = cscale(w, 2.0);
                for (int r = 0; r < len; ++r) { const cd t = cmul(hv[r], w); T[(j + 1 + r) * LD + lane] = csub(T[(j + 1 + r) * LD + lane], t); }
                if (lane == j)
                    for (int r = 1; r < len; ++r) T[(j + 1 + r) * LD + j] = cmk(0.0, 0.0);
            }
            __syncthreads();
            if (l < k) {                                                 // from the right: row l of T (lanes 0..) and of Q (lanes 32..)
                cd *row = (h ? Q : T) + l * LD + j + 1;
                cd w = cmk(0.0, 0.0);
                for (int c = 0; c < len; ++c) cfma(w, row[c], hv[c]);
                w = cscale(w, 2.0);
                for (int c = 0; c < len; ++c) { const cd t = cmul(w, cconj(hv[c])); row[c] = csub(row[c], t); }
            }
            __syncthreads();
        }
        // ---- shifted QR steps, deflation from the bottom ----
        int n = k, steps = 0;
        while (n > 1) {
            const cd a = T[(n - 2) * LD + n - 2], b = T[(n - 2) * LD + n - 1], c = T[(n - 1) * LD + n - 2], dd = T[(n - 1) * LD + n - 1];
            if (cabs1(c) <= 0x1p-52 * (cabs1(a) + cabs1(dd))) { --n; continue; }      // (the entry is not read again: T's lower triangle is taken as zero)
            if (steps >= 40 * k) { st = STATUS_ITERATIONS; ok = false; break; }
            ++steps;
            // Wilkinson: the eigenvalue of the trailing 2 x 2 block nearer to its last entry
            const cd hh = cscale(csub(a, dd), 0.5), bc = cmul(b, c), root = csqrt_(cadd(cmul(hh, hh), bc));
            const cd dp = cadd(hh, root), dm = csub(hh, root), den = cabs2(dp) >= cabs2(dm) ? dp : dm;
            const cd sigma = cabs2(den) != 0.0 ? csub(dd, cdiv(bc, den)) : dd;
            __syncthreads();                                             // (a, b, c, dd are read)
            if (lane < n) T[lane * LD + lane] = csub(T[lane * LD + lane], sigma);
            __syncthreads();
            for (int i = 0; i + 1 < n; ++i) {                            // R = G_{n-2} .. G_0 (T - sigma): a lane per column
                const cd ti = T[i * LD + i], tj = T[(i + 1) * LD + i];
                const double na = cabs1(ti), nb = cabs1(tj);
                double cs = 1.0;
                cd sn = cmk(0.0, 0.0);
                if (nb != 0.0) {
                    if (na == 0.0) { cs = 0.0; sn = cscale(cconj(tj), 1.0 / nb); }
                    else {
                        const double r = sqrt(na * na + nb * nb);
                        cs = na / r;
                        sn = cscale(cmul(cscale(ti, 1.0 / na), cconj(tj)), 1.0 / r);
                    }
                }
                if (lane == 0) rot[i] = cmk(cs, 0.0);                    // kept for the pass from the right (hv: free since the reduction)
                if (lane == 1) hv[i] = sn;
                __syncthreads();                                         // (ti, tj are read)
                if (lane >= i && lane < k) {
                    const cd ri = T[i * LD + lane], rj = T[(i + 1) * LD + lane];
                    T[i * LD + lane] = cadd(cscale(ri, cs), cmul(sn, rj));
                    T[(i + 1) * LD + lane] = lane == i ? cmk(0.0, 0.0) : csub(cscale(rj, cs), cmulc(sn, ri));
                }
                __syncthreads();
            }
            // R G_0^H .. G_{n-2}^H and Q likewise: a lane per row, the rotations one after the other in the lane
            if (l < (h ? k : n)) {
                cd *row = (h ? Q : T) + l * LD;
                for (int i = h ? 0 : max(l - 1, 0); i + 1 < n; ++i) {
                    const double cs = rot[i].x;
                    const cd sn = hv[i], ci = row[i], cj = row[i + 1];
                    row[i] = cadd(cscale(ci, cs), cmulc(sn, cj));
                    row[i + 1] = csub(cscale(cj, cs), cmul(sn, ci));
                }
                if (!h) row[l] = cadd(row[l], sigma);
            }
            __syncthreads();
        }
    }
    if (ok) {
        // ---- Y: the eigenvectors of the triangular T, unit diagonal; a lane per eigenvector ----
        if (lane < k) {
            const cd tii = T[lane * LD + lane];
            for (int j = k - 1; j > lane; --j) Y[j * LD + lane] = cmk(0.0, 0.0);
            Y[lane * LD + lane] = cmk(1.0, 0.0);
            for (int j = lane - 1; j >= 0; --j) {
                cd den = csub(T[j * LD + j], tii);
                if (cabs2(den) == 0.0) den = cmk(0x1p-1022, 0.0);
                cd acc = cmk(0.0, 0.0);
                for (int p = j + 1; p <= lane; ++p) cfma(acc, T[j * LD + p], Y[p * LD + lane]);
                const cd q = cdiv(acc, den);
                Y[j * LD + lane] = cmk(-q.x, -q.y);
            }
        }
        // ---- S = Q^H Psi Q for x and y (Z = Psi Q between) ----
        for (int idx = lane; idx < 2 * kk; idx += ES_THREADS) {
            const int w = idx / kk, ab = idx - w * kk, a = ab / k, b = ab - a * k;
            cd acc = cmk(0.0, 0.0);
            for (int p = 0; p < k; ++p) cfma(acc, sP[w * MAT + a * LD + p], Q[p * LD + b]);
            Z[w * MAT + a * LD + b] = acc;
        }
        __syncthreads();
        for (int idx = lane; idx < 2 * kk; idx += ES_THREADS) {
            const int w = idx / kk, ab = idx - w * kk, a = ab / k, b = ab - a * k;
            cd acc = cmk(0.0, 0.0);
            for (int p = 0; p < k; ++p) cfmac(acc, Q[p * LD + a], Z[w * MAT + p * LD + b]);
            sS[w * MAT + a * LD + b] = acc;
        }
        __syncthreads();
        // ---- lambda_i = z_i of Y z = S y_i: lane (h, i) keeps its vector in row i of Z ----
        if (l < k) {
            const cd *S = sS + h * MAT;
            cd *z = Z + h * MAT + l * LD;
            for (int p = l; p < k; ++p) {
                cd acc = cmk(0.0, 0.0);
                for (int q = 0; q <= l; ++q) cfma(acc, S[p * LD + q], Y[q * LD + l]);
                z[p] = acc;
            }
            for (int p = k - 1; p >= l; --p) {
                cd acc = z[p];
                for (int q = p + 1; q < k; ++q) { const cd t = cmul(Y[p * LD + q], z[q]); acc = csub(acc, t); }
                z[p] = acc;
            }
            lam[h * MAX_K + l] = z[l];
        }
        __syncthreads();
    }
    if (!ok) {                                                           // (uniform)
        if (lane < slots) {
            phases[2 * lane] = 0.0; phases[2 * lane + 1] = 0.0;
            angles[2 * lane] = -1.f; angles[2 * lane + 1] = -1.f;
            modulus[2 * lane] = -1.f; modulus[2 * lane + 1] = -1.f;
            power[lane] = -1.f; flags[lane] = 0;
        }
        if (lane == 0) { *found = 0; *status = st; }
        return;
    }
    // ---- phases, angles ----
    const double pi = 3.14159265358979323846, tpd = 2.0 * pi * (double)d;
    double mu = 0.0, nu = 0.0, alpha = 0.0, beta = 0.0, mx_ = 0.0, my_ = 0.0, pw = 0.0;
    int fl = 0;
    if (lane < k) {
        const cd lx = lam[lane], ly = lam[MAX_K + lane];
        mu = atan2(lx.y, lx.x); nu = atan2(ly.y, ly.x);
        mx_ = cabs1(lx); my_ = cabs1(ly);
        double cb = nu / tpd;
        if (fabs(cb) > 1.0) { fl |= FLAG_BETA; cb = cb > 0.0 ? 1.0 : -1.0; }
        const double sb = sqrt(1.0 - cb * cb);
        double ca = sb > 0.0 ? mu / (tpd * sb) : 0.0;
        if (!(sb > 0.0) || fabs(ca) > 1.0) { fl |= FLAG_ALPHA; ca = ca > 1.0 ? 1.0 : ca < -1.0 ? -1.0 : ca; }
        beta = acos(cb); alpha = acos(ca);
        skey[MAX_K + lane] = alpha; skey[2 * MAX_K + lane] = beta;
    }
    __syncthreads();
    // ---- power: per slot, lanes as elements for a, then as columns r ----
    for (int i = 0; i < k; ++i) {
        const double al = skey[MAX_K + i], be = skey[2 * MAX_K + i];
        if (lane < M) {
            const int ix = lane % SX, iy = lane / SX;
            const double ph = 2.0 * 3.14159265358979323846 * (double)d * ((double)ix * cos(al) * sin(be) + (double)iy * cos(be));
            sa[lane] = cmk(cos(ph), sin(ph));
        }
        __syncthreads();
        double term = 0.0;
        if (lane < M) {
            double gr = 0.0, gi = 0.0;
            for (int c = 0; c < M; ++c) {
                const float2 v = vec[(size_t)c * M + lane];
                const cd ac = sa[c];
                gr += (double)v.x * ac.x + (double)v.y * ac.y;           // conj(v) a
                gi += (double)v.x * ac.y - (double)v.y * ac.x;
            }
            term = (double)sv[lane] * (gr * gr + gi * gi);
        }
        sred[lane] = term;
        __syncthreads();
        double sum = 0.0;
        for (int r = 0; r < M; ++r) sum += sred[r];
        if (lane == i) pw = sum / ((double)M * (double)M);
        __syncthreads();
    }
    // ---- order: descending power, then ascending mu, then nu (then the index: a slot per lane whatever the values) ----
    if (lane < k) { skey[lane] = pw; skey[MAX_K + lane] = mu; skey[2 * MAX_K + lane] = nu; }
    __syncthreads();
    if (lane < k) {
        int rank = 0;
        for (int j = 0; j < k; ++j) {
            if (j == lane) continue;
            const double pj = skey[j], mj = skey[MAX_K + j], nj = skey[2 * MAX_K + j];
            const bool before = pj > pw || (!(pw > pj) && (mj < mu || (!(mu < mj) && (nj < nu || (!(nu < nj) && j < lane)))));
            rank += before ? 1 : 0;
        }
        phases[2 * rank] = mu; phases[2 * rank + 1] = nu;
        angles[2 * rank] = (float)alpha; angles[2 * rank + 1] = (float)beta;
        modulus[2 * rank] = (float)mx_; modulus[2 * rank + 1] = (float)my_;
        power[rank] = (float)pw; flags[rank] = fl;
    } else if (lane < slots) {
        phases[2 * lane] = 0.0; phases[2 * lane + 1] = 0.0;
        angles[2 * lane] = -1.f; angles[2 * lane + 1] = -1.f;
        modulus[2 * lane] = -1.f; modulus[2 * lane + 1] = -1.f;
        power[lane] = -1.f; flags[lane] = 0;
    }
    if (lane == 0) { *found = k; *status = 0; }
}

// grid (nmat), 64 W threads (W = ES_WAVES = 1; a template, so that the kernel is emitted where it is first launched, behind every earlier
// kernel).  vec [nmat][M][M], sv [nmat][M]; korder [nmat] or NULL: the matrix's source count in place of k;
// found, status [nmat]; phases, angles, modulus [nmat][slots][2]; power, flags [nmat][slots]
template <int W>
__global__ __launch_bounds__(64 * W) void k_doa_esprit(const float2 *__restrict__ vec, const float *__restrict__ sv, int M, int k,
                                                            const int32_t *__restrict__ korder, float d, int SX, int SY, int slots,
                                                            int32_t *__restrict__ found, int32_t *__restrict__ status, double *__restrict__ phases,
                                                            float *__restrict__ angles, float *__restrict__ modulus, float *__restrict__ power,
                                                            int32_t *__restrict__ flags)
{
    const size_t e = blockIdx.x, s = e * (size_t)slots;
    esprit2d_matrix(vec + e * M * M, sv + e * M, M, korder ? korder[e] : k, d, SX, SY, slots, found + e, status + e, phases + 2 * s, angles + 2 * s, modulus + 2 * s,
                    power + s, flags + s);
}

// the per-op form: one matrix, slots = k
template <int W>
__global__ __launch_bounds__(64 * W) void k_esprit2d(const float2 *__restrict__ vec, const float *__restrict__ sv, int M, int k, float d, int SX, int SY,
                                                          int32_t *__restrict__ found, int32_t *__restrict__ status, double *__restrict__ phases,
                                                          float *__restrict__ angles, float *__restrict__ modulus, float *__restrict__ power,
                                                          int32_t *__restrict__ flags)
{
    esprit2d_matrix(vec, sv, M, k, d, SX, SY, k, found, status, phases, angles, modulus, power, flags);
}

} // namespace esprit
} // namespace crsdr
