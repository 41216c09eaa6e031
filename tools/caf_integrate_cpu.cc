// caf_integrate_cpu.cc -- csrc/caf_integrate_solve.hpp (crsdr_caf's integration across lines: the limits, the offsets of the range walk,
// lambda, the clamped source cell and the three-operation update) as a CPU program: the very functions the kernel of
// csrc/caf_integrate.hpp calls, so that the sanitizers can walk every index of them without a GPU (tests/test_host_caf_integrate.py
// builds this with -fsanitize=address,undefined and -ffp-contract=off: the update is three roundings here as on the device).
//   caf_integrate_cpu in.bin out.bin
//   in : int32 ncases, then per case
//        int32 nlines, nmaps, nd, R, ncuts; int64 m0 (the lines before the first: the state starts all zero with this counter);
//        double forget, coupling; int32 cut[ncuts] (the lines of each submit, nlines in all); float maps[nlines][nmaps][nd][R]
//   out: float imap[nlines][nmaps][nd][R]; the state buffer behind the last submit (integ::state_bytes); int64 D[nlines][nd];
//        double lambda[nlines]
// Every submit loads the counter from the state buffer and stores it back, as the kernel does.
#include "../coherent-rtlsdr_amd/csrc/caf_integrate_solve.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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
        int32_t h[5];
        int64_t m0 = 0;
        double p[2];
        if (!get(in, h, 5) || !get(in, &m0, 1) || !get(in, p, 2)) { fprintf(stderr, "short case %d\n", k); return 2; }
        const int nlines = h[0], nmaps = h[1], nd = h[2], R = h[3], ncuts = h[4];
        const integ::Params q{p[0], p[1]};
        if (nlines < 1 || nmaps < 1 || nd < 1 || R < 1 || ncuts < 1 || ncuts > nlines || m0 < 0) { fprintf(stderr, "bad case %d\n", k); return 2; }
        const int lim = integ::bad_limit(nd, q);
        if (lim) { fprintf(stderr, "bad case %d (limit %d)\n", k, lim); return 2; }
        const size_t cells = (size_t)nd * (size_t)R;
        // exactly the sizes the arrays have: an index past one is the sanitizer's to find
        std::vector<int32_t> cut((size_t)ncuts);
        std::vector<float> maps((size_t)nlines * nmaps * cells), imap(maps.size());
        if (!get(in, cut.data(), cut.size()) || !get(in, maps.data(), maps.size())) { fprintf(stderr, "short case %d\n", k); return 2; }
        std::vector<unsigned char> state(integ::state_bytes(nmaps, nd, R), 0);
        memcpy(state.data(), &m0, sizeof(m0));
        std::vector<double> I((size_t)nmaps * cells), tmp((size_t)R), lam((size_t)nlines);
        std::vector<int64_t> D((size_t)nlines * nd);
        int line = 0;
        for (int c = 0; c < ncuts; ++c) {
            if (cut[c] < 1 || line + cut[c] > nlines) { fprintf(stderr, "bad cuts in case %d\n", k); return 2; }
            int64_t m;
            memcpy(&m, state.data(), sizeof(m));
            memcpy(I.data(), state.data() + integ::HEADER_BYTES, sizeof(double) * I.size());
            for (int l = 0; l < cut[c]; ++l, ++line, ++m) {
                for (int j = 0; j < nmaps; ++j)
                    integ::line(I.data() + (size_t)j * cells, tmp.data(), m, q, maps.data() + ((size_t)line * nmaps + j) * cells, nd, R,
                                imap.data() + ((size_t)line * nmaps + j) * cells);
                for (int d = 0; d < nd; ++d) D[(size_t)line * nd + d] = integ::step(m, q.coupling, cafp::signed_bin(d, nd));
                lam[(size_t)line] = integ::lambda(m, q.forget);
            }
            memcpy(state.data(), &m, sizeof(m));
            memcpy(state.data() + integ::HEADER_BYTES, I.data(), sizeof(double) * I.size());
        }
        if (line != nlines) { fprintf(stderr, "bad cuts in case %d\n", k); return 2; }
        fwrite(imap.data(), sizeof(float), imap.size(), out);
        fwrite(state.data(), 1, state.size(), out);
        fwrite(D.data(), sizeof(int64_t), D.size(), out);
        fwrite(lam.data(), sizeof(double), lam.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
