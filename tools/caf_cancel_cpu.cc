// caf_cancel_cpu.cc -- csrc/caf_cancel_solve.hpp (the canceller of crsdr_caf: where an entry of the normal matrix sits, its Cholesky
// factor with the pivot rule, the solve of a row's equations and the share of the row's power that stays) as a CPU program: the very
// functions the kernels of csrc/caf_cancel.hpp call, so that the sanitizers can walk every index of them without a GPU
// (tests/test_host_caf_cancel.py builds this with -fsanitize=address,undefined).
//   caf_cancel_cpu in.bin out.bin
//   in : int32 ncases, then per case: int32 taps, dopp, nrows; double S[4 dopp + 1][taps][taps][2];
//        per row: double E; double c[n][2], n = taps (2 dopp + 1)
//   out: per case: int32 status; per row: double h[n][2]; double share
#include "../coherent-rtlsdr_amd/csrc/caf_cancel_solve.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace crsdr::cc;

template <typename T>
static bool get(FILE *f, T *v, size_t n) { return fread(v, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t ncases = 0;
    if (!get(in, &ncases, 1) || ncases < 0) { fprintf(stderr, "bad header\n"); return 2; }
    for (int k = 0; k < ncases; ++k) {
        int32_t h[3];
        if (!get(in, h, 3)) { fprintf(stderr, "short case %d\n", k); return 2; }
        const int K = h[0], P = h[1], nrows = h[2];
        if (nrows < 1 || bad_limit(8, MAX_TAPS, 1, K, P)) { fprintf(stderr, "bad case %d (limit %d)\n", k, bad_limit(8, MAX_TAPS, 1, K, P)); return 2; }
        const int n = basis(K, P);
        // exactly the sizes the arrays have: an index past one is the sanitizer's to find
        std::vector<cd> S((size_t)(4 * P + 1) * K * K), Lf((size_t)n * (n + 1) / 2), c((size_t)n), y((size_t)n), g((size_t)n);
        if (!get(in, S.data(), S.size())) { fprintf(stderr, "short case %d\n", k); return 2; }
        const bool ok = chol_factor(S.data(), K, P, Lf.data());
        const int32_t status = ok ? 0 : STATUS_SINGULAR;
        fwrite(&status, sizeof(status), 1, out);
        for (int r = 0; r < nrows; ++r) {
            double E = 0.0;
            if (!get(in, &E, 1) || !get(in, c.data(), c.size())) { fprintf(stderr, "short case %d\n", k); return 2; }
            for (int j = 0; j < n; ++j) g[(size_t)j] = cd{0.0, 0.0};
            if (ok) chol_solve(Lf.data(), n, c.data(), y.data(), g.data());
            const double share = residual_share(E, g.data(), c.data(), n);
            fwrite(g.data(), sizeof(cd), g.size(), out);
            fwrite(&share, sizeof(share), 1, out);
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
