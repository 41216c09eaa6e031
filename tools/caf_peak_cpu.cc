// caf_peak_cpu.cc -- csrc/caf_peak.hpp (the peak figures of crsdr_caf: lag, doppler, power, ratio and the two sub-cell offsets) as a CPU
// program: the very functions the kernel of csrc/caf.hpp calls, so that the sanitizers can walk every index of them without a GPU
// (tests/test_host_caf.py builds this with -fsanitize=address,undefined).
//   caf_peak_cpu in.bin out.bin
//   in : int32 ncases, then per case: int32 nd, R, guard, comps, step; float src[nd][R][comps]
//   out: per case: float peak[6]
// comps: 2 for a row's chi (re, im), 1 for an array map.  step: the number of interleaved parts the search is split into (1: one pass;
// 256: as the kernel's threads do, joined by the same tree).
#include "../coherent-rtlsdr_amd/csrc/caf_peak.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace crsdr::cafp;

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
        const int nd = h[0], R = h[1], guard = h[2], comps = h[3], step = h[4];
        if (nd < 8 || nd > 4096 || (nd & (nd - 1)) || R < 1 || R > 1024 || guard < 0 || guard > nd / 2 || (comps != 1 && comps != 2) || step < 1 || (step & (step - 1))) {
            fprintf(stderr, "bad case %d\n", k);
            return 2;
        }
        // exactly the size the array has: an index past it is the sanitizer's to find
        std::vector<float> src((size_t)nd * R * comps);
        if (!get(in, src.data(), src.size())) { fprintf(stderr, "short case %d\n", k); return 2; }
        std::vector<Part> parts((size_t)step);
        for (int l = 0; l < step; ++l) parts[l] = part(src.data(), comps, nd, R, guard, l, step);
        for (int h2 = step / 2; h2 >= 1; h2 >>= 1)
            for (int l = 0; l < h2; ++l) merge(parts[l], parts[l + h2]);
        float peak[6];
        figures(src.data(), comps, nd, R, guard, parts[0], peak);
        fwrite(peak, sizeof(float), 6, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
