// caf_bearing_cpu.cc -- csrc/caf_bearing_solve.hpp (the bearings of crsdr_caf: which row is which element, the training snapshots'
// covariance over the detector's training set, its loading, the Cholesky factor and its inverse, W u, the co-array coefficients, the
// statistic T, the first maximum and the zoom search) as a CPU program: the very functions the kernels of csrc/caf_bearing.hpp call, so
// that the sanitizers can walk every index of them without a GPU (tests/test_host_caf_bearing.py builds this with
// -fsanitize=address,undefined).
//   caf_bearing_cpu in.bin out.bin
//   in : int32 ncases, then per case: int32 nrows, nd, R, ref_row, guard, gd, gr, td, tr, mx, my, ncx, ncy, mode, levels, d, tau;
//        float spacing, loading; float chi[nrows][nd][R][2]
//   out: per case: int32 N, status; double T[ncx][ncy]; float dir[8]
#include "../coherent-rtlsdr_amd/csrc/caf_bearing_solve.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace crsdr;
using brg::cd;

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
        int32_t h[17];
        float f[2];
        if (!get(in, h, 17) || !get(in, f, 2)) { fprintf(stderr, "short case %d\n", k); return 2; }
        const int nrows = h[0], nd = h[1], R = h[2], ref = h[3], guard = h[4], d = h[15], tau = h[16];
        const cfar::Params cp{h[5], h[6], h[7], h[8], 1.f, 1, 1};
        const brg::Params bp{h[9], h[10], h[11], h[12], f[0], h[13], f[1], h[14], 0u};
        if (nrows < 2 || nd < 8 || (nd & (nd - 1)) || R < 1 || ref < 0 || ref >= nrows || guard < 0 || guard > nd / 2 || d < 0 || d >= nd || tau < 0 || tau >= R ||
            cfar::bad_limit(nd, cp) || brg::bad_limit(nrows, 1, 1, bp)) {
            fprintf(stderr, "bad case %d (limits %d, %d)\n", k, cfar::bad_limit(nd, cp), brg::bad_limit(nrows, 1, 1, bp));
            return 2;
        }
        const int m = bp.mx * bp.my;
        const size_t cells = (size_t)nd * (size_t)R;
        // exactly the sizes the arrays have: an index past one is the sanitizer's to find
        std::vector<float> chi((size_t)nrows * cells * 2);
        if (!get(in, chi.data(), chi.size())) { fprintf(stderr, "short case %d\n", k); return 2; }
        std::vector<cd> u((size_t)m), Qs((size_t)m * (m + 1) / 2), Li((size_t)m * (m + 1) / 2), y((size_t)m);
        std::vector<double> rec((size_t)brg::REC), T((size_t)bp.ncx * bp.ncy);
        for (int e = 0; e < m; ++e) u[(size_t)e] = brg::snap_elem(chi.data(), cells, ref, e, d * R + tau);
        int32_t N = 0;
        if (bp.mode == brg::MODE_ADAPTIVE) N = brg::train_cov(chi.data(), m, nd, R, ref, guard, cp, d, tau, Qs.data());
        brg::solve_slot(bp, u.data(), Qs.data(), N, Li.data(), y.data(), rec.data());
        int best = 0;
        for (int g = 0; g < bp.ncx * bp.ncy; ++g) {
            T[(size_t)g] = brg::stat(rec.data(), bp.mx, bp.my, bp.d, bp.ncx, bp.ncy, (double)(g / bp.ncy), (double)(g % bp.ncy));
            if (T[(size_t)g] > T[(size_t)best]) best = g;
        }
        const int cx = best / bp.ncy, cy = best % bp.ncy;
        double x = (double)cx, yy = (double)cy, step = 0.5, fval[brg::POINTS];
        for (int l = 0; l < bp.levels; ++l) {
            for (int q = 0; q < brg::POINTS; ++q) {
                double px, py;
                brg::lattice_point(x, yy, step, q, bp.ncx, bp.ncy, &px, &py);
                fval[q] = brg::stat(rec.data(), bp.mx, bp.my, bp.d, bp.ncx, bp.ncy, px, py);
            }
            brg::zoom_pick(fval, step, bp.ncx, bp.ncy, &x, &yy);
            step *= 0.25;
        }
        float dir[8];
        brg::figures(rec.data(), cx, cy, T[(size_t)best], x, yy, bp.ncx, bp.ncy, dir);
        const int32_t status = (int32_t)rec[1];
        fwrite(&N, sizeof(N), 1, out);
        fwrite(&status, sizeof(status), 1, out);
        fwrite(T.data(), sizeof(double), T.size(), out);
        fwrite(dir, sizeof(float), 8, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
