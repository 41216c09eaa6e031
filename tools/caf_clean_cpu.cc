// caf_clean_cpu.cc -- csrc/caf_clean_solve.hpp (the second cancellation stage of crsdr_caf: its limits, the walk over a detection list
// that picks the targets, the member table, where an entry of the joint normal matrix sits, its Cholesky factor with the pivot rule,
// and the solve on it) as a CPU program: the very functions the kernels of csrc/caf_clean.hpp call, so that the sanitizers can walk
// every index of them without a GPU (tests/test_host_caf_clean.py builds this with -fsanitize=address,undefined).  cl::phase alone has
// a host form of its own (cos and sin of the reduced argument where the device has sincospi): its value is checked, not its arithmetic.
//   caf_clean_cpu in.bin out.bin
//   in : int32 ncases, then per case: int32 nd, R, nrows, taps, dopp, T, wl, wq, Kdet, count; float min_snr; float det[Kdet][8];
//        double S[4 dopp + 1][taps][taps][2]; double A2[n2max][nmax][2] (row i - n1, column j <= i read); per row: double E;
//        double c[nmax][2] (the line's n first)
//   out: per case: int32 limit; if 0: int32 ntgt, picked[T], nmem, nslot, slot_lag[nslot]; per member int32 lag, slot, owner, pos and
//        double g, phi_g[nd - 1][2]; int32 status; double L[n (n + 1) / 2][2]; per row: double h[n][2]; double share
#include "../coherent-rtlsdr_amd/csrc/caf_clean_solve.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace crsdr;

template <typename T>
static bool get(FILE *f, T *v, size_t n) { return fread(v, sizeof(T), n, f) == n; }
template <typename T>
static void put(FILE *f, const T *v, size_t n) { fwrite(v, sizeof(T), n, f); }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t ncases = 0;
    if (!get(in, &ncases, 1) || ncases < 0) { fprintf(stderr, "bad header\n"); return 2; }
    for (int k = 0; k < ncases; ++k) {
        int32_t a[10];
        float min_snr = 0.f;
        if (!get(in, a, 10) || !get(in, &min_snr, 1)) { fprintf(stderr, "short case %d\n", k); return 2; }
        const int nd = a[0], R = a[1], nrows = a[2], K = a[3], P = a[4], Kdet = a[8], count = a[9];
        const cl::Params prm{a[5], min_snr, a[6], a[7]};
        if (nrows < 1 || Kdet < 1 || Kdet > 64 || cc::bad_limit(nd, R, 1, K, P)) { fprintf(stderr, "bad case %d\n", k); return 2; }
        const int32_t limit = cl::bad_limit(nd, R, 1, nrows, K, P, prm);
        put(out, &limit, 1);
        std::vector<float> det((size_t)Kdet * 8);
        if (!get(in, det.data(), det.size())) { fprintf(stderr, "short case %d\n", k); return 2; }
        if (limit) continue;                                          // (a refused descriptor ends its case here: nothing follows it)
        const int n1 = cc::basis(K, P), n2max = cl::max_target_members(prm), nmax = n1 + n2max;
        // exactly the sizes the arrays have: an index past one is the sanitizer's to find
        std::vector<int> picked((size_t)prm.max_targets, -1);
        std::vector<cc::cd> S((size_t)(4 * P + 1) * K * K), A2((size_t)n2max * nmax), c((size_t)nmax);
        if (!get(in, S.data(), S.size()) || !get(in, A2.data(), A2.size())) { fprintf(stderr, "short case %d\n", k); return 2; }
        const int32_t nt = cl::pick_walk(det.data(), count, Kdet, nd, K, P, prm, picked.data());
        cl::Table t;
        cl::build_table(det.data(), picked.data(), nt, R, prm, &t);
        put(out, &nt, 1);
        put(out, picked.data(), picked.size());
        put(out, &t.nmem, 1);
        put(out, &t.nslot, 1);
        put(out, t.slot_lag, (size_t)t.nslot);
        for (int i = 0; i < t.nmem; ++i) {
            const int32_t m[4] = {t.lag[i], t.slot[i], t.owner[i], t.pos[i]};
            put(out, m, 4);
            put(out, &t.g[i], 1);
            const cc::cd f = cl::phase(t.g[i], nd - 1, nd);
            put(out, &f, 1);
        }
        const int n = n1 + t.nmem;
        std::vector<cc::cd> Lf((size_t)n * (n + 1) / 2, cc::cd{0.0, 0.0}), y((size_t)n), h((size_t)n);
        const int32_t status = cl::joint_factor(S.data(), A2.data(), K, P, n, nmax, Lf.data());
        put(out, &status, 1);
        put(out, Lf.data(), Lf.size());
        for (int r = 0; r < nrows; ++r) {
            double E = 0.0;
            if (!get(in, &E, 1) || !get(in, c.data(), c.size())) { fprintf(stderr, "short case %d\n", k); return 2; }
            for (int j = 0; j < n; ++j) h[(size_t)j] = cc::cd{0.0, 0.0};
            if (!status) cc::chol_solve(Lf.data(), n, c.data(), y.data(), h.data());
            const double share = cc::residual_share(E, h.data(), c.data(), n);
            put(out, h.data(), h.size());
            put(out, &share, 1);
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
