// caf_cfar_cpu.cc -- csrc/caf_cfar.hpp (the CFAR detector of crsdr_caf: training set and count, threshold test, neighbourhood test, the
// order of the detections and the eight figures of one) as a CPU program: the very functions the kernels of csrc/caf_cfar_kernels.hpp
// call, so that the sanitizers can walk every index of them without a GPU (tests/test_host_caf_cfar.py builds this with
// -fsanitize=address,undefined).
//   caf_cfar_cpu in.bin out.bin
//   in : int32 ncases, then per case: int32 nd, R, guard, comps, gd, gr, td, tr, min_train, max_det, parts; float alpha;
//        float src[nd][R][comps]
//   out: per case: int32 count; float det[max_det][8]
// comps: 2 for a row's chi (re, im), 1 for an array map.  parts: the map's cells are dealt to `parts` lists (cell i to list i % parts),
// each list keeps its best max_det in order, and the lists are merged over their heads -- as the kernels' tiles and their merge do.
#include "../coherent-rtlsdr_amd/csrc/caf_cfar.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace crsdr::cfar;

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
        int32_t h[11];
        float alpha = 0.f;
        if (!get(in, h, 11) || !get(in, &alpha, 1)) { fprintf(stderr, "short case %d\n", k); return 2; }
        const int nd = h[0], R = h[1], guard = h[2], comps = h[3], parts = h[10];
        const Params q{h[4], h[5], h[6], h[7], alpha, h[8], h[9]};
        if (nd < 8 || nd > 4096 || (nd & (nd - 1)) || R < 1 || R > 1024 || guard < 0 || guard > nd / 2 || (comps != 1 && comps != 2) || parts < 1 || bad_limit(nd, q)) {
            fprintf(stderr, "bad case %d (limit %d)\n", k, bad_limit(nd, q));
            return 2;
        }
        // exactly the size the array has: an index past it is the sanitizer's to find
        std::vector<float> src((size_t)nd * R * comps);
        if (!get(in, src.data(), src.size())) { fprintf(stderr, "short case %d\n", k); return 2; }
        std::vector<std::vector<Cand>> lists((size_t)parts);
        int32_t count = 0;
        for (int d = 0; d < nd; ++d)
            for (int tau = 0; tau < R; ++tau) {
                Cand c;
                const double p = crsdr::cafp::power(src.data(), comps, d * R + tau), z = train_sum(src.data(), comps, nd, R, guard, q, d, tau);
                if (!detect(src.data(), comps, nd, R, guard, q, d, tau, p, z, &c)) continue;
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
