// esprit_cpu.cc -- csrc/esprit.hpp's device function esprit2d_matrix on the CPU: 64 host threads in the place of the wave's lanes,
// a pthread barrier for __syncthreads, statics for __shared__.  The arithmetic is the kernel's own source, so a host build under
// AddressSanitizer / UBSan checks every LDS and global index, and one under ThreadSanitizer every barrier (a missing one is a data
// race between two "lanes"), without a GPU:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -o esprit_cpu tools/esprit_cpu.cc -lpthread
//     g++ -std=c++17 -O1 -g -fsanitize=thread -ffp-contract=off -o esprit_cpu_tsan tools/esprit_cpu.cc -lpthread
//     esprit_cpu IN OUT     IN: int32 M, k, SX, SY, slots; float d; vec [M][M][2] float; sv [M] float
//                           OUT: int32 found, status; phases [slots][2] double; angles, modulus [slots][2] float; power [slots] float;
//                                flags [slots] int32
// tests/test_esprit_cpu_threads.py runs it against the numpy model.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <pthread.h>
#include <vector>

struct double2 { double x, y; };
struct float2 { float x, y; };
static inline double2 make_double2(double x, double y) { return {x, y}; }
struct Index3 { int x, y, z; };
static thread_local Index3 threadIdx, blockIdx;
static pthread_barrier_t g_barrier;
static int g_vote;
static inline void __syncthreads() { pthread_barrier_wait(&g_barrier); }
static inline int __any(int p)
{
    __syncthreads();
    if (threadIdx.x == 0) __atomic_store_n(&g_vote, 0, __ATOMIC_RELAXED);
    __syncthreads();
    if (p) __atomic_store_n(&g_vote, 1, __ATOMIC_RELAXED);
    __syncthreads();
    return __atomic_load_n(&g_vote, __ATOMIC_RELAXED);
}
using std::max;
using std::min;
#define __shared__ static
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define CRSDR_ESPRIT_HOST_THREADS
#include "../coherent-rtlsdr_amd/csrc/esprit.hpp"

struct Args {
    const float2 *vec; const float *sv; int M, k; float d; int SX, SY, slots;
    int32_t *found, *status; double *phases; float *angles, *modulus, *power; int32_t *flags; int lane;
};

static void *lane_main(void *p)
{
    const Args *a = static_cast<const Args *>(p);
    threadIdx.x = a->lane;
    crsdr::esprit::esprit2d_matrix(a->vec, a->sv, a->M, a->k, a->d, a->SX, a->SY, a->slots, a->found, a->status, a->phases, a->angles, a->modulus, a->power, a->flags);
    return nullptr;
}

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: esprit_cpu IN OUT\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    int hdr[5];
    float d;
    if (!f || std::fread(hdr, 4, 5, f) != 5 || std::fread(&d, 4, 1, f) != 1) return 2;
    const int M = hdr[0], k = hdr[1], SX = hdr[2], SY = hdr[3], slots = hdr[4];
    if (M < 1 || M > crsdr::esprit::MAX_M || SX * SY != M || slots < 1 || slots > crsdr::esprit::MAX_K) return 2;
    std::vector<float2> vec((size_t)M * M);
    std::vector<float> sv(M);
    if (std::fread(vec.data(), 8, vec.size(), f) != vec.size() || std::fread(sv.data(), 4, sv.size(), f) != sv.size()) return 2;
    std::fclose(f);
    // exactly `slots` entries each: a write behind them is the sanitizer's to report
    int32_t found = -7, status = -7;
    std::vector<double> phases(2 * slots, 99.0);
    std::vector<float> angles(2 * slots, 99.f), modulus(2 * slots, 99.f), power(slots, 99.f);
    std::vector<int32_t> flags(slots, 99);
    pthread_barrier_init(&g_barrier, nullptr, crsdr::esprit::ES_THREADS);
    pthread_t th[crsdr::esprit::ES_THREADS];
    Args a[crsdr::esprit::ES_THREADS];
    for (int i = 0; i < crsdr::esprit::ES_THREADS; ++i) {
        a[i] = Args{vec.data(), sv.data(), M, k, d, SX, SY, slots, &found, &status, phases.data(), angles.data(), modulus.data(), power.data(), flags.data(), i};
        if (pthread_create(&th[i], nullptr, lane_main, &a[i])) return 3;
    }
    for (int i = 0; i < crsdr::esprit::ES_THREADS; ++i) pthread_join(th[i], nullptr);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(&found, 4, 1, o); std::fwrite(&status, 4, 1, o);
    std::fwrite(phases.data(), 8, phases.size(), o); std::fwrite(angles.data(), 4, angles.size(), o); std::fwrite(modulus.data(), 4, modulus.size(), o);
    std::fwrite(power.data(), 4, power.size(), o); std::fwrite(flags.data(), 4, flags.size(), o);
    std::fclose(o);
    return 0;
}
