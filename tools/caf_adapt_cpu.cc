// caf_adapt_cpu.cc -- csrc/caf_adapt.hpp (the adaptive beams of crsdr_caf: the limits, the enumeration of the training cells and of
// their tiles, the order of the partial sums, the line's solve on the bearings' Cholesky pieces, the figures and the fallback) as a
// CPU program: the very functions the kernels of csrc/caf_adapt_kernels.hpp call, so that the sanitizers can walk every index of them
// without a GPU (tests/test_host_caf_adapt.py builds this with -fsanitize=address,undefined).
//   caf_adapt_cpu in.bin out.bin
//   in : int32 ncases, then per case int32 nrows, nd, R, ref_row, nbeams, d_lo, d_n, r_lo, r_n; float loading;
//        float chi[nrows][nd][R][2]; float w[nbeams][nrows - 1][2]
//   out: per case int32 status, tiles; float aw[nbeams][m][2]; float ainfo[nbeams][2]; double Qs[m (m + 1) / 2][2] (the tiles' sums added)
#include "../coherent-rtlsdr_amd/csrc/caf_adapt.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace crsdr;

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
        int32_t h[9];
        float loading;
        if (!get(in, h, 9) || !get(in, &loading, 1)) { fprintf(stderr, "short case %d\n", k); return 2; }
        const int nrows = h[0], nd = h[1], R = h[2], ref = h[3], nb = h[4], m = nrows - 1;
        const ad::Params q{h[5], h[6], h[7], h[8], loading, 0u};
        if (nd < 1 || R < 1 || ref < 0 || ref >= nrows || nb < 1 || nb > 64 || ad::bad_limit(nrows, nd, R, q)) { fprintf(stderr, "bad case %d\n", k); return 2; }
        const size_t cells = (size_t)nd * (size_t)R, pairs = (size_t)ad::pairs_of(m);
        const int N = ad::cells_of(q), tiles = ad::tiles_of(N);
        // exactly the sizes the arrays have: an index past one is the sanitizer's to find
        std::vector<float> chi((size_t)nrows * cells * 2), w((size_t)nb * m * 2), aw((size_t)nb * m * 2), ainfo((size_t)nb * 2);
        if (!get(in, chi.data(), chi.size()) || !get(in, w.data(), w.size())) { fprintf(stderr, "short case %d\n", k); return 2; }
        std::vector<double> part((size_t)tiles * pairs * 2);
        std::vector<brg::cd> P(pairs), Lf(pairs), Li(pairs), Q(pairs), x((size_t)3 * m), Qs(pairs);
        std::vector<double> t((size_t)2 * m);
        for (int tile = 0; tile < tiles; ++tile) {
            ad::tile_cov(chi.data(), m, nd, R, ref, q, tile, P.data());
            for (size_t p = 0; p < pairs; ++p) { part[2 * ((size_t)tile * pairs + p)] = P[p].re; part[2 * ((size_t)tile * pairs + p) + 1] = P[p].im; }
        }
        const int32_t status = ad::solve_line(q, m, nb, part.data(), w.data(), Lf.data(), Li.data(), Q.data(), x.data(), t.data(), aw.data(), ainfo.data());
        for (size_t p = 0; p < pairs; ++p) Qs[p] = ad::tile_sum(part.data(), tiles, (int)pairs, (int)p);
        const int32_t head[2] = {status, tiles};
        fwrite(head, sizeof(int32_t), 2, out);
        fwrite(aw.data(), sizeof(float), aw.size(), out);
        fwrite(ainfo.data(), sizeof(float), ainfo.size(), out);
        fwrite(Qs.data(), sizeof(brg::cd), Qs.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
