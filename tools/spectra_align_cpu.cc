// spectra_align_cpu.cc -- csrc/spectra_align.hpp (the alignment figures of crsdr_spectra: delay, phase, gain, coherence) as a CPU
// program: the very functions the kernel of csrc/spectra.hpp calls, so that the sanitizers can walk every index of them without a GPU
// (tests/test_host_spectra.py builds this with -fsanitize=address,undefined).
//   spectra_align_cpu in.bin out.bin
//   in : int32 ncases, then per case: int32 nrows, N, lo, hi, step; float psd[nrows][N]; float cross[nrows][N][2]
//   out: per case: float align[nrows][4]
// step: the number of interleaved parts the sums are split into (1: one sum; 64: as the kernel's wave does, added in lane order).
#include "../coherent-rtlsdr_amd/csrc/spectra_align.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace crsdr::spa;

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
        int32_t h[5];
        if (!get(in, h, 5)) { fprintf(stderr, "short case %d\n", k); return 2; }
        const int nrows = h[0], N = h[1], lo = h[2], hi = h[3], step = h[4], K = hi - lo + 1;
        if (nrows < 1 || N < 2 || (N & (N - 1)) || lo < -N / 2 || hi > N / 2 - 1 || lo >= hi || step < 1) { fprintf(stderr, "bad case %d\n", k); return 2; }
        // exactly the sizes the arrays have: an index past them is the sanitizer's to find
        std::vector<float> psd((size_t)nrows * N), cross((size_t)nrows * N * 2), align((size_t)nrows * 4);
        if (!get(in, psd.data(), psd.size()) || !get(in, cross.data(), cross.size())) { fprintf(stderr, "short case %d\n", k); return 2; }
        for (int c = 0; c < nrows; ++c) {
            const float *p0 = psd.data(), *pc = psd.data() + (size_t)c * N, *sc = cross.data() + (size_t)c * N * 2;
            Lag a{0.0, 0.0};
            for (int l = 0; l < step; ++l) { const Lag p = lag_part(sc, N, lo, K, l, step); a.re += p.re; a.im += p.im; }
            const double delay = delay_of(a, N);
            Sums t{0.0, 0.0, 0.0, 0.0, 0.0};
            for (int l = 0; l < step; ++l) {
                const Sums p = sums_part(p0, pc, sc, N, lo, K, delay, l, step);
                t.zre += p.zre; t.zim += p.zim; t.p0 += p.p0; t.ss += p.ss; t.pp += p.pp;
            }
            figures(delay, t, align.data() + (size_t)c * 4);
        }
        fwrite(align.data(), sizeof(float), align.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
