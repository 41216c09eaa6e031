// refcancel_cpu.cc -- csrc/refcancel_solve.hpp (the canceller's Gram indexing, Cholesky factor, solve and residual) as a CPU program:
// the very functions the kernels of csrc/refcancel.hpp call, so that the sanitizers can walk every index of them without a GPU
// (tests/test_host_refcancel.py builds this with -fsanitize=address,undefined).
//   refcancel_cpu in.bin out.bin
//   in : int32 ncases, then per case: int32 taps, int32 gram[90] (the packed 9 x 9 integer Gram), double c[taps][2], double E
//   out: per case: int32 status, double g[taps][2], double residual
#include "../coherent-rtlsdr_amd/csrc/refcancel_solve.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace crsdr::rc;

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
        int32_t taps = 0;
        std::vector<int32_t> gram(GRAM_INTS);
        if (!get(in, &taps, 1) || taps < 1 || taps > MAX_TAPS || !(taps & 1) || !get(in, gram.data(), gram.size())) { fprintf(stderr, "bad case %d\n", k); return 2; }
        std::vector<cd> c((size_t)taps), g((size_t)taps);          // exactly taps entries: an index past them is the sanitizer's to find
        double E = 0.0, residual = 0.0;
        if (!get(in, c.data(), c.size()) || !get(in, &E, 1)) { fprintf(stderr, "short case %d\n", k); return 2; }
        const int32_t status = solve_row(gram.data(), taps, c.data(), E, g.data(), &residual);
        fwrite(&status, sizeof(status), 1, out);
        fwrite(g.data(), sizeof(cd), g.size(), out);
        fwrite(&residual, sizeof(residual), 1, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
