// caf_track_cpu.cc -- csrc/caf_track.hpp (the tracker of crsdr_caf: the limits, what a measurement is, the wrap, predict, the gate's
// d2, update and coast, the status rules, the strict order, lowest-free-slot initiation, the id counter and the record) as a CPU
// program: the very functions the kernel of csrc/caf_track_kernels.hpp calls, so that the sanitizers can walk every index of them
// without a GPU (tests/test_host_caf_track.py builds this with -fsanitize=address,undefined).
//   caf_track_cpu in.bin out.bin
//   in : int32 ncases, then per case
//        int32 nlines, K, nd, R, has_aux, ncuts, counter (the ids issued before the first line); int32 max_tracks, source; double sigma_r, sigma_f, gate, p0_g, q_r, q_f, q_g, coupling;
//        int32 m, n, tent_miss, conf_miss; int32 cut[ncuts] (the lines of each submit, nlines in all);
//        float det[nlines][K][8]; int32 count[nlines]; float aux[nlines][K][2] if has_aux
//   out: float trk[nlines][T][16]; int32 ntrk[nlines][4]; the state buffer behind the last submit (trk::state_bytes)
// Every submit loads the table from the state buffer and stores it back, as the kernel does.
#include "../coherent-rtlsdr_amd/csrc/caf_track.hpp"

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
        int32_t h[7], a[2], b[4];
        double d[8];
        if (!get(in, h, 7) || !get(in, a, 2) || !get(in, d, 8) || !get(in, b, 4)) { fprintf(stderr, "short case %d\n", k); return 2; }
        const int nlines = h[0], K = h[1], nd = h[2], R = h[3], has_aux = h[4], ncuts = h[5];
        const trk::Params q{a[0], a[1], d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], b[0], b[1], b[2], b[3]};
        const int lim = trk::bad_limit(q);
        if (lim) { fprintf(stderr, "bad case %d (limit %d)\n", k, lim); return 2; }
        if (nlines < 1 || K < 1 || K > trk::MAX_MEAS || nd < 8 || (nd & (nd - 1)) || R < 1 || ncuts < 1 || ncuts > nlines || h[6] < 0 || h[6] >= trk::ID_PERIOD) { fprintf(stderr, "bad case %d\n", k); return 2; }
        const size_t T = (size_t)q.max_tracks;
        // exactly the sizes the arrays have: an index past one is the sanitizer's to find
        std::vector<int32_t> cut((size_t)ncuts), count((size_t)nlines), ntrk((size_t)nlines * 4);
        std::vector<float> det((size_t)nlines * K * 8), aux(has_aux ? (size_t)nlines * K * 2 : 0), rec((size_t)nlines * T * trk::REC);
        if (!get(in, cut.data(), cut.size()) || !get(in, det.data(), det.size()) || !get(in, count.data(), count.size()) || (has_aux && !get(in, aux.data(), aux.size()))) {
            fprintf(stderr, "short case %d\n", k);
            return 2;
        }
        std::vector<unsigned char> state(trk::state_bytes(q.max_tracks), 0);
        memcpy(state.data(), &h[6], sizeof(int32_t));
        std::vector<double> d2(T * (size_t)K);
        std::vector<int> scratch(T + (size_t)K);
        int line = 0;
        for (int c = 0; c < ncuts; ++c) {
            if (cut[c] < 1 || line + cut[c] > nlines) { fprintf(stderr, "bad cuts in case %d\n", k); return 2; }
            std::vector<trk::Slot> slots(T);
            int32_t counter;
            memcpy(&counter, state.data(), sizeof(counter));
            memcpy(slots.data(), state.data() + trk::HEADER_BYTES, sizeof(trk::Slot) * T);
            for (int l = 0; l < cut[c]; ++l, ++line)
                trk::line(slots.data(), &counter, q, det.data() + (size_t)line * K * 8, count[line], has_aux ? aux.data() + (size_t)line * K * 2 : nullptr, K, nd, R, d2.data(),
                          scratch.data(), rec.data() + (size_t)line * T * trk::REC, ntrk.data() + (size_t)line * 4);
            memcpy(state.data(), &counter, sizeof(counter));
            memcpy(state.data() + trk::HEADER_BYTES, slots.data(), sizeof(trk::Slot) * T);
        }
        if (line != nlines) { fprintf(stderr, "bad cuts in case %d\n", k); return 2; }
        fwrite(rec.data(), sizeof(float), rec.size(), out);
        fwrite(ntrk.data(), sizeof(int32_t), ntrk.size(), out);
        fwrite(state.data(), 1, state.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
