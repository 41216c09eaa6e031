// caf_cfar_est_cpu.cc -- the estimators of csrc/caf_cfar.hpp (greatest-of, smallest-of, ordered statistic: the half an offset belongs
// to, the closed-form half counts, the half means and their choice, os_rank and the selection by the letter) as a CPU program, as
// caf_cfar_cpu.cc is for cell averaging: the functions the kernels of csrc/caf_cfar_kernels.hpp call or restate, so that the sanitizers
// can walk every index of them without a GPU (tests/test_host_caf_cfar_est.py builds this with -fsanitize=address,undefined).
//   caf_cfar_est_cpu in.bin out.bin
//   in : int32 ncases, then per case: int32 nd, R, guard, comps, gd, gr, td, tr, min_train, max_det, parts, est, axis, rank; float alpha;
//        float src[nd][R][comps]
//   out: per case: int32 count; float det[max_det][8]
// comps and parts as caf_cfar_cpu.cc has them.  The closed-form half counts are checked here against a count by trains() and half_of()
// at every cell (exit status 3), and the counting rule of k_caf_cfar_os against the sorted selection (exit status 4).
#include "../coherent-rtlsdr_amd/csrc/caf_cfar.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace crsdr::cfar;

template <typename T>
static bool get(FILE *f, T *v, size_t n) { return fread(v, sizeof(T), n, f) == n; }

// the kernel's rule: alpha x_(k) < P  <=>  #{alpha x_j < P} >= k, and x_(k) > 0  <=>  #{x_j = 0} < k
static bool os_counts_pass(const float *src, int comps, int nd, int R, int guard, const Params &q, int d, int tau, double p, int k)
{
    int under = 0, zeros = 0;
    for (int a = -(q.gd + q.td); a <= q.gd + q.td; ++a)
        for (int b = -(q.gr + q.tr); b <= q.gr + q.tr; ++b) {
            if (!trains(a, b, d, tau, nd, R, guard, q)) continue;
            const double x = crsdr::cafp::power(src, comps, wrap(d + a, nd) * R + tau + b), t = (double)q.alpha * x;
            under += t < p ? 1 : 0;
            zeros += x == 0.0 ? 1 : 0;
        }
    return under >= k && zeros < k;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t ncases = 0;
    if (!get(in, &ncases, 1) || ncases < 0) { fprintf(stderr, "bad header\n"); return 2; }
    for (int k = 0; k < ncases; ++k) {
        int32_t h[14];
        float alpha = 0.f;
        if (!get(in, h, 14) || !get(in, &alpha, 1)) { fprintf(stderr, "short case %d\n", k); return 2; }
        const int nd = h[0], R = h[1], guard = h[2], comps = h[3], parts = h[10];
        const Params q{h[4], h[5], h[6], h[7], alpha, h[8], h[9], h[11], h[12], h[13]};
        if (nd < 8 || nd > 4096 || (nd & (nd - 1)) || R < 1 || R > 1024 || guard < 0 || guard > nd / 2 || (comps != 1 && comps != 2) || parts < 1 || bad_limit(nd, q) ||
            bad_estimator(q)) {
            fprintf(stderr, "bad case %d (limit %d, estimator %d)\n", k, bad_limit(nd, q), bad_estimator(q));
            return 2;
        }
        // exactly the size the array has: an index past it is the sanitizer's to find
        std::vector<float> src((size_t)nd * R * comps);
        if (!get(in, src.data(), src.size())) { fprintf(stderr, "short case %d\n", k); return 2; }
        std::vector<std::vector<Cand>> lists((size_t)parts);
        int32_t count = 0;
        const int nfull = full_count(q);
        for (int d = 0; d < nd; ++d)
            for (int tau = 0; tau < R; ++tau) {
                Cand c;
                const double p = crsdr::cafp::power(src.data(), comps, d * R + tau);
                bool hit;
                if (q.est == EST_CA) {
                    hit = detect(src.data(), comps, nd, R, guard, q, d, tau, p, train_sum(src.data(), comps, nd, R, guard, q, d, tau), &c);
                } else if (q.est == EST_OS) {
                    int N = 0;
                    const int n = train_count(d, tau, nd, R, guard, q), kth = n >= 1 ? os_rank(q.rank, n, nfull) : 0;
                    const double xk = os_select(src.data(), comps, nd, R, guard, q, d, tau, kth, &N);
                    if (N != n || kth > n) { fprintf(stderr, "case %d cell (%d, %d): N %d, closed form %d, k %d\n", k, d, tau, N, n, kth); return 3; }
                    hit = detect_os(src.data(), comps, nd, R, guard, q, d, tau, p, xk, N, &c);
                    const bool counted = n >= 1 && n >= q.min_train && os_counts_pass(src.data(), comps, nd, R, guard, q, d, tau, p, kth);
                    if (crsdr::cafp::in_set(d, nd, guard) && counted != (n >= 1 && n >= q.min_train && xk > 0.0 && p > (double)q.alpha * xk)) {
                        fprintf(stderr, "case %d cell (%d, %d): the counting rule and the selection disagree\n", k, d, tau);
                        return 4;
                    }
                } else {
                    for (int side = -1; side <= 1; side += 2) {
                        int n = 0;
                        for (int a = -(q.gd + q.td); a <= q.gd + q.td; ++a)
                            for (int b = -(q.gr + q.tr); b <= q.gr + q.tr; ++b) n += half_of(a, b, q.axis) == side && trains(a, b, d, tau, nd, R, guard, q) ? 1 : 0;
                        if (n != half_count(d, tau, nd, R, guard, q, side)) {
                            fprintf(stderr, "case %d cell (%d, %d) side %d: %d cells, closed form %d\n", k, d, tau, side, n, half_count(d, tau, nd, R, guard, q, side));
                            return 3;
                        }
                    }
                    hit = detect_halves(src.data(), comps, nd, R, guard, q, d, tau, p, half_sum(src.data(), comps, nd, R, guard, q, d, tau, -1),
                                        half_sum(src.data(), comps, nd, R, guard, q, d, tau, 1), &c);
                }
                if (!hit) continue;
                lists[(size_t)(c.i % parts)].push_back(c);
                ++count;
            }
        for (auto &l : lists) {
            std::sort(l.begin(), l.end(), before);
            if (l.size() > (size_t)q.max_det) l.resize((size_t)q.max_det);
        }
        std::vector<size_t> head((size_t)parts, 0);
        std::vector<float> det((size_t)q.max_det * 8, 0.f);
        for (int s = 0; s < q.max_det; ++s) {
            Cand best{0.0, 0.0, -1, 0};
            int from = -1;
            for (int p = 0; p < parts; ++p)
                if (head[p] < lists[p].size() && before(lists[p][head[p]], best)) { best = lists[p][head[p]]; from = p; }
            if (from < 0) break;
            ++head[from];
            figures(src.data(), comps, nd, R, guard, best, &det[(size_t)s * 8]);
        }
        fwrite(&count, sizeof(count), 1, out);
        fwrite(det.data(), sizeof(float), det.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
