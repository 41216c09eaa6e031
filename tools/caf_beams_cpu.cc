// caf_beams_cpu.cc -- csrc/caf_beams.hpp (the coherent beam maps of crsdr_caf: the limits, which row is which element, a beam sum in
// the kernel's order and its power, the steering weights, and the fusion of the beams' detection lists) as a CPU program: the very
// functions the kernels of csrc/caf_beams_kernels.hpp call, so that the sanitizers can walk every index of them without a GPU
// (tests/test_host_caf_beams.py builds this with -fsanitize=address,undefined).
//   caf_beams_cpu in.bin out.bin
//   in : int32 ncases, then per case int32 kind and
//        kind 0 (maps):  int32 nrows, nd, R, ref_row, nbeams; float chi[nrows][nd][R][2]; float w[nbeams][nrows - 1][2]
//        kind 1 (fuse):  int32 nbeams, K, nd, R; float bdet[nbeams][K][8]; int32 bcount[nbeams]
//        kind 2 (steer): int32 mx, my, ncx, ncy, nbeams; float d; double xy[nbeams][2]
//   out: kind 0: float bmap[nbeams][nd][R]     kind 1: int32 nfused; float fused[K][8]     kind 2: float w[nbeams][mx my][2]
#include "../coherent-rtlsdr_amd/csrc/caf_beams.hpp"

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
        int32_t kind = -1, h[5];
        if (!get(in, &kind, 1)) { fprintf(stderr, "short case %d\n", k); return 2; }
        if (kind == 0) {
            if (!get(in, h, 5)) { fprintf(stderr, "short case %d\n", k); return 2; }
            const int nrows = h[0], nd = h[1], R = h[2], ref = h[3], nb = h[4], m = nrows - 1;
            if (nrows < 2 || nd < 8 || (nd & (nd - 1)) || R < 1 || ref < 0 || ref >= nrows || nb < 1 || nb > bm::MAX_BEAMS) { fprintf(stderr, "bad case %d\n", k); return 2; }
            const size_t cells = (size_t)nd * (size_t)R;
            // exactly the sizes the arrays have: an index past one is the sanitizer's to find
            std::vector<float> chi((size_t)nrows * cells * 2), w((size_t)nb * m * 2), bmap((size_t)nb * cells);
            if (!get(in, chi.data(), chi.size()) || !get(in, w.data(), w.size())) { fprintf(stderr, "short case %d\n", k); return 2; }
            const int lim = bm::bad_limit(nrows, 1, nd, R, nb, w.data(), 0u);
            if (lim) { fprintf(stderr, "bad case %d (limit %d)\n", k, lim); return 2; }
            for (int b = 0; b < nb; ++b)
                for (size_t i = 0; i < cells; ++i) {
                    float re, im;
                    bm::beam_sum(chi.data(), cells, m, ref, w.data() + (size_t)b * m * 2, i, &re, &im);
                    bmap[(size_t)b * cells + i] = bm::power(re, im);
                }
            fwrite(bmap.data(), sizeof(float), bmap.size(), out);
        } else if (kind == 1) {
            if (!get(in, h, 4)) { fprintf(stderr, "short case %d\n", k); return 2; }
            const int nb = h[0], K = h[1], nd = h[2], R = h[3];
            if (nb < 1 || nb > bm::MAX_BEAMS || K < 1 || K > cfar::MAX_DET || nd < 8 || (nd & (nd - 1)) || R < 1) { fprintf(stderr, "bad case %d\n", k); return 2; }
            std::vector<float> bdet((size_t)nb * K * 8), fused((size_t)K * 8);
            std::vector<int32_t> bcount((size_t)nb);
            if (!get(in, bdet.data(), bdet.size()) || !get(in, bcount.data(), bcount.size())) { fprintf(stderr, "short case %d\n", k); return 2; }
            std::vector<bm::Cand> list((size_t)nb * K);
            std::vector<unsigned char> alive((size_t)nb * K);
            const int32_t nf = bm::fuse(bdet.data(), bcount.data(), nb, K, nd, R, list.data(), alive.data(), fused.data());
            fwrite(&nf, sizeof(nf), 1, out);
            fwrite(fused.data(), sizeof(float), fused.size(), out);
        } else if (kind == 2) {
            float d;
            if (!get(in, h, 5) || !get(in, &d, 1)) { fprintf(stderr, "short case %d\n", k); return 2; }
            const int mx = h[0], my = h[1], ncx = h[2], ncy = h[3], nb = h[4];
            if (mx < 1 || my < 1 || mx * my > bm::MAX_M || ncx < 2 || ncy < 2 || nb < 1 || nb > bm::MAX_BEAMS) { fprintf(stderr, "bad case %d\n", k); return 2; }
            std::vector<double> xy((size_t)nb * 2);
            if (!get(in, xy.data(), xy.size())) { fprintf(stderr, "short case %d\n", k); return 2; }
            std::vector<float> w((size_t)nb * mx * my * 2);
            for (int b = 0; b < nb; ++b) bm::steer(w.data() + (size_t)b * mx * my * 2, mx, my, d, ncx, ncy, xy[2 * (size_t)b], xy[2 * (size_t)b + 1]);
            fwrite(w.data(), sizeof(float), w.size(), out);
        } else { fprintf(stderr, "bad kind in case %d\n", k); return 2; }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
