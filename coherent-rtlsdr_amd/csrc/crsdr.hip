// crsdr.hip -- C ABI (include/crsdr.h) over the gfx950 kernels in kernels.hpp.
// Host side is plain C++: plan = device buffers + twiddle table + two HIP streams + events.
// No torch types, no CPU fallback: every compute entry point needs a HIP device.
#include "../../include/crsdr.h"
#include "kernels.hpp"
#include "doa.hpp"
#include "smooth.hpp"
#include "beams.hpp"
#include "subband.hpp"
#include "subband_beams.hpp"
#include "spectrum.hpp"
#include "refine.hpp"
#include "esprit.hpp"
#include "refcancel_solve.hpp"

#include <hip/hip_runtime.h>

#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>
#include <sched.h>

using namespace crsdr;

// ---- error plumbing ---------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail(e_ == hipErrorOutOfMemory ? CRSDR_ENOMEM                                    \
                        : (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice) ? CRSDR_ENODEV    \
                                                                                  : CRSDR_EHIP,     \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// HIP_TRY as a value: the CRSDR_* code of `expr`, for code that goes on after a failure
#define HIP_RC(expr) [&]() -> int { HIP_TRY(expr); return CRSDR_OK; }()

extern "C" int crsdr_abi_version(void) { return CRSDR_ABI_VERSION; }
extern "C" const char *crsdr_last_error(void) { return g_err; }

extern "C" int crsdr_device_count(int *count)
{
    if (!count) return fail(CRSDR_EINVAL, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(CRSDR_ENODEV, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return CRSDR_OK;
}

extern "C" int crsdr_device_info(int device, char *name, int name_cap, int *compute_units, int *clock_khz, int *memory_clock_khz,
                                 size_t *memory_bytes)
{
    int n = 0;
    int rc = crsdr_device_count(&n);
    if (rc) return rc;
    if (device < 0 || device >= n) return fail(CRSDR_ENODEV, "device_info: device %d of %d", device, n);
    hipDeviceProp_t pr;
    HIP_TRY(hipGetDeviceProperties(&pr, device));
    if (name && name_cap > 0) { snprintf(name, (size_t)name_cap, "%s (%s)", pr.name, pr.gcnArchName); }
    if (compute_units) *compute_units = pr.multiProcessorCount;
    if (clock_khz) *clock_khz = pr.clockRate;
    if (memory_clock_khz) *memory_clock_khz = pr.memoryClockRate;
    if (memory_bytes) *memory_bytes = pr.totalGlobalMem;
    return CRSDR_OK;
}

static int require_device();
// Page-locked memory should sit on the NUMA node the GPU hangs off: a transfer that crosses the socket interconnect runs at
// roughly half the PCIe rate.  The pages are placed where the allocating thread runs, so the thread is moved to that node's
// CPUs for the duration of the allocation (sysfs: /sys/bus/pci/devices/<bdf>/numa_node, /sys/devices/system/node/nodeN/cpulist).
// Best effort: any failure leaves the affinity alone.  CRSDR_HOST_NUMA=0 switches it off.
static bool near_device_cpus(cpu_set_t *set)
{
    static const bool enabled = [] { const char *e = getenv("CRSDR_HOST_NUMA"); return !e || atoi(e) != 0; }();
    if (!enabled) return false;
    int dev = 0;
    char bdf[64] = {0}, path[256], buf[4096];
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetPCIBusId(bdf, sizeof(bdf), dev) != hipSuccess) return false;
    for (char *c = bdf; *c; ++c) *c = (char)tolower(*c);
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bdf);
    FILE *f = fopen(path, "r");
    if (!f) return false;
    int node = -1;
    const int got = fscanf(f, "%d", &node);
    fclose(f);
    if (got != 1 || node < 0) return false;
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    f = fopen(path, "r");
    if (!f) return false;
    const bool ok = fgets(buf, sizeof(buf), f) != nullptr;
    fclose(f);
    if (!ok) return false;
    CPU_ZERO(set);
    int n = 0;
    for (char *tok = strtok(buf, ",\n"); tok; tok = strtok(nullptr, ",\n")) {
        int lo = 0, hi = 0;
        const int k = sscanf(tok, "%d-%d", &lo, &hi);
        if (k < 1) continue;
        if (k == 1) hi = lo;
        for (int c = lo; c <= hi && c < CPU_SETSIZE; ++c) { CPU_SET(c, set); ++n; }
    }
    return n > 0;
}

extern "C" int crsdr_host_alloc(void **ptr, size_t bytes)
{
    if (!ptr || !bytes) return fail(CRSDR_EINVAL, "host_alloc: NULL pointer or zero size");
    *ptr = nullptr;
    { int rc_ = require_device(); if (rc_) return rc_; }
    cpu_set_t old_set, near_set;
    const bool moved = sched_getaffinity(0, sizeof(old_set), &old_set) == 0 && near_device_cpus(&near_set) &&
                       sched_setaffinity(0, sizeof(near_set), &near_set) == 0;
    hipError_t e = hipHostMalloc(ptr, bytes, hipHostMallocDefault);
    if (e == hipSuccess && moved) memset(*ptr, 0, bytes);      // first touch on the near node, if the runtime left any page untouched
    if (moved) (void)sched_setaffinity(0, sizeof(old_set), &old_set);
    if (e != hipSuccess) { *ptr = nullptr; return fail(e == hipErrorOutOfMemory ? CRSDR_ENOMEM : CRSDR_EHIP, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e)); }
    return CRSDR_OK;
}
extern "C" int crsdr_host_free(void *ptr)
{
    if (!ptr) return CRSDR_OK;
    HIP_TRY(hipHostFree(ptr));
    return CRSDR_OK;
}

static int require_device()
{
    int n = 0;
    int rc = crsdr_device_count(&n);
    if (rc) return rc;
    if (n < 1) return fail(CRSDR_ENODEV, "no HIP device: libcrsdr has no CPU fallback");
    return CRSDR_OK;
}

static int ilog2_exact(int n)
{
    if (n < 1 || (n & (n - 1))) return -1;
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}

// argument checks shared by the per-op calls and the engine (doa_engine.hpp)
static bool smooth_shape_ok(int mx, int my, int sx, int sy, uint32_t flags)
{
    return mx >= 1 && my >= 1 && (long long)mx * my >= 2 && (long long)mx * my <= music::MAX_M && sx >= 1 && sx <= mx && sy >= 1 && sy <= my &&
           sx * sy >= 2 && !(flags & ~(uint32_t)CRSDR_SMOOTH_FB);
}

// Co-array augmentation (augment.hpp): sizes and mask, then c(u) of every half-plane lag.  counts [vy][2 vx - 1] (may be NULL) takes
// c(u) at [uy][ux + vx - 1], row 0's negative ux the mirrored count; *uncovered the number of half-plane lags with c(u) = 0, (*fux, *fuy)
// the first of them in the kernel's lag order (uy, then ux).  CRSDR_EINVAL for bad sizes or mask alone.
static uint64_t augment_mask(int m, uint64_t mask) { return mask ? mask : (m >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << m) - 1)); }

static int augment_lag_counts(const char *who, int mx, int my, int vx, int vy, uint64_t mask, int32_t *counts, int *uncovered, int *fux, int *fuy)
{
    if (mx < 1 || my < 1 || (long long)mx * my < 2 || (long long)mx * my > music::MAX_M)
        return fail(CRSDR_EINVAL, "%s: array of %d x %d elements (m = mx * my in [2, %d])", who, mx, my, music::MAX_M);
    if (vx < 1 || vx > mx || vy < 1 || vy > my || vx * vy < 2)
        return fail(CRSDR_EINVAL, "%s: virtual array of %d x %d in an array of %d x %d (1 <= vx <= mx, 1 <= vy <= my, vx * vy >= 2)", who, vx, vy, mx, my);
    const int m = mx * my;
    if (mask && ((m < 64 && (mask >> m)) || !(mask & (mask - 1))))
        return fail(CRSDR_EINVAL, "%s: mask = 0x%llx (0 = all %d elements; else no bit from %d on and at least two bits set)", who, (unsigned long long)mask, m, m);
    const uint64_t present = augment_mask(m, mask);
    int missing = 0;
    for (int uy = 0; uy < vy; ++uy)
        for (int ux = uy ? -(vx - 1) : 0; ux < vx; ++ux) {
            int c = 0;
            for (int p = 0; p < m; ++p) {
                const int ixq = p % mx + ux, iyq = p / mx + uy;
                if (ixq < 0 || ixq >= mx || iyq >= my) continue;
                if (((present >> p) & 1u) && ((present >> (iyq * mx + ixq)) & 1u)) ++c;
            }
            if (counts) {
                counts[uy * (2 * vx - 1) + ux + vx - 1] = c;
                if (uy == 0) counts[vx - 1 - ux] = c;
            }
            if (c == 0 && missing++ == 0) {
                if (fux) *fux = ux;
                if (fuy) *fuy = uy;
            }
        }
    if (uncovered) *uncovered = missing;
    return CRSDR_OK;
}

// what crsdr_doa_set_augment and crsdr_augment_covariance ask: the above, and every lag covered
static int augment_args_ok(const char *who, int mx, int my, int vx, int vy, uint64_t mask)
{
    int missing = 0, ux = 0, uy = 0;
    const int rc = augment_lag_counts(who, mx, my, vx, vy, mask, nullptr, &missing, &ux, &uy);
    if (rc) return rc;
    if (missing)
        return fail(CRSDR_EINVAL, "%s: no pair of present receivers at lag (ux, uy) = (%d, %d), the first of %d uncovered lags of the %d x %d virtual array", who, ux, uy,
                    missing, vx, vy);
    return CRSDR_OK;
}

extern "C" int crsdr_augment_lags(int mx, int my, int vx, int vy, uint64_t mask, int32_t *counts, int *uncovered)
{
    return augment_lag_counts("augment_lags", mx, my, vx, vy, mask, counts, uncovered, nullptr, nullptr);
}

static int subband_args_ok(const char *who, int blocksize, int nfft, int first, int nbands, int width, int window)
{
    if (nfft < (1 << subband::SB_MIN_LOG2) || nfft > (1 << subband::SB_MAX_LOG2) || (nfft & (nfft - 1)))
        return fail(CRSDR_EINVAL, "%s: nfft = %d (a power of two, %d..%d)", who, nfft, 1 << subband::SB_MIN_LOG2, 1 << subband::SB_MAX_LOG2);
    if (blocksize % (2 * nfft)) return fail(CRSDR_EINVAL, "%s: blocksize = %d is no multiple of 2 nfft = %d", who, blocksize, 2 * nfft);
    if (first < 0 || first >= nfft) return fail(CRSDR_EINVAL, "%s: first = %d (0..nfft - 1 = %d)", who, first, nfft - 1);
    if (nbands < 1 || width < 1 || (long long)nbands * width > nfft)
        return fail(CRSDR_EINVAL, "%s: %d bands of %d bins (nbands >= 1, width >= 1, nbands * width <= nfft = %d)", who, nbands, width, nfft);
    if (window != CRSDR_WINDOW_RECT && window != CRSDR_WINDOW_HANN) return fail(CRSDR_EINVAL, "%s: window = %d", who, window);
    return CRSDR_OK;
}

// kind of crsdr_doa_set_spectrum (music_ok) / crsdr_spectrum2d, and CAPON's loading
static int spectrum_args_ok(const char *who, int kind, float loading, bool music_ok)
{
    if (kind != CRSDR_SPECTRUM_BARTLETT && kind != CRSDR_SPECTRUM_CAPON && !(music_ok && kind == CRSDR_SPECTRUM_MUSIC))
        return fail(CRSDR_EINVAL, "%s: kind = %d", who, kind);
    if (kind == CRSDR_SPECTRUM_CAPON && !(loading >= 1e-6f && loading <= 1.0f)) return fail(CRSDR_EINVAL, "%s: loading = %g (1e-6..1)", who, (double)loading);
    return CRSDR_OK;
}

// forward twiddle table W_n^k = (cos, -sin)(2 pi k / n), generated in double, rounded once
static int make_twiddles(int n, float2 **d_tw)
{
    std::vector<float2> h((size_t)n);
    for (int k = 0; k < n; ++k) {
        double a = 2.0 * M_PI * (double)k / (double)n;
        h[k] = make_float2((float)std::cos(a), (float)(-std::sin(a)));
    }
    HIP_TRY(hipMalloc((void **)d_tw, sizeof(float2) * (size_t)n));
    HIP_TRY(hipMemcpy(*d_tw, h.data(), sizeof(float2) * (size_t)n, hipMemcpyHostToDevice));
    return CRSDR_OK;
}

// x14 tables: twA[j][t] = W_16384^(t 2^j), t < 512; twB[j][n] = W_512^(n 2^j), n < 16; j < 5
static int make_twiddles14(float2 **d_twA, float2 **d_twB)
{
    std::vector<float2> a(5 * 512), b(5 * 16);
    for (int j = 0; j < 5; ++j) {
        for (int t = 0; t < 512; ++t) {
            double ang = 2.0 * M_PI * (double)(t << j) / 16384.0;
            a[j * 512 + t] = make_float2((float)std::cos(ang), (float)(-std::sin(ang)));
        }
        for (int n = 0; n < 16; ++n) {
            double ang = 2.0 * M_PI * (double)(n << j) / 512.0;
            b[j * 16 + n] = make_float2((float)std::cos(ang), (float)(-std::sin(ang)));
        }
    }
    HIP_TRY(hipMalloc((void **)d_twA, sizeof(float2) * a.size()));
    HIP_TRY(hipMalloc((void **)d_twB, sizeof(float2) * b.size()));
    HIP_TRY(hipMemcpy(*d_twA, a.data(), sizeof(float2) * a.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(*d_twB, b.data(), sizeof(float2) * b.size(), hipMemcpyHostToDevice));
    return CRSDR_OK;
}

// forward table W_n^(k * step), k < count
static int make_twiddle_table(double n, size_t count, size_t step, float2 **d)
{
    std::vector<float2> h(count);
    for (size_t k = 0; k < count; ++k) {
        double a = 2.0 * M_PI * (double)(k * step) / n;
        h[k] = make_float2((float)std::cos(a), (float)(-std::sin(a)));
    }
    HIP_TRY(hipMalloc((void **)d, sizeof(float2) * count));
    HIP_TRY(hipMemcpy(*d, h.data(), sizeof(float2) * count, hipMemcpyHostToDevice));
    return CRSDR_OK;
}

constexpr int kMinLog2 = 4, kMaxLog2 = 14, kMaxLog2Plan = 22; // LDS-resident sizes; long-block plans up to 2^22 // LDS-resident transform sizes: 16 .. 16384 points

template <int LOG2N>
static constexpr size_t fft_lds_bytes() { return sizeof(float2) * ((size_t)1 << LOG2N) + 256; }

// ---- process-level switches (README, "switches"), read once ---------------------------------------------------------------
// The spin switches take "n" or "n@k": n polls from the process's (k+1)-th launch of the kernel concerned on (each launch site
// counts its own launches), the default before it, so that a test can let clean launches come first.
struct SpinSwitch {
    int value, dflt;
    long from;
    int at(long launch) const { return launch >= from ? value : dflt; }
};
static SpinSwitch spin_switch(const char *e, int dflt)
{
    const char *at = e ? strchr(e, '@') : nullptr;
    return {e ? atoi(e) : dflt, dflt, at ? atol(at + 1) : 0L};
}
struct Switches {
    // CRSDR_K1_VARIANT: 'a' (auto, default) = the two-row kernel (q, xcorr14q.hpp) for launches with enough rows per CU, the packed
    // one-row kernel (p, xcorr14p.hpp) otherwise; "packed" / "q" / "r" force one of them.  Same arithmetic, identical bits.
    // 'r' is the two-row kernel with the column twiddle chains carried from row to row (k_xcorr_lag14r): whatever holds for q
    // (launch shape, work counter, snapshot, q_disabled, CRSDR_K1_QSPIN, wait flags) holds for r -- two_row() is the one test.
    // (Measured-slower experiments live in tools/: xcorr14h.hpp, half-row LDS images -- dead end (8) of DESIGN.md --, xcorr14w.hpp,
    // 1024 threads per row -- dead end (11) --, and xcorr14_scalar.hpp, the scalar-fp32 twin of r01.)
    char k1_variant;
    SpinSwitch qspin;      // CRSDR_K1_QSPIN: polls per bounded wait of the two-row K1 and the two-line stage B (tests force 0)
    SpinSwitch refspin;    // CRSDR_K1_REFSPIN (tests only): polls of a folded launch's rows for their block's reference spectrum;
                           // -1: every row workgroup reports the wait as run out without polling
    int k2_spin;           // CRSDR_K2_SPIN: look-back polls of the fused phase kernel (one value for every launch)
    bool long_q;           // CRSDR_LONG_Q: long blocks may run stage B on the two-line kernel
};
static const Switches &sw()
{
    static const Switches s = [] {
        const char *v = getenv("CRSDR_K1_VARIANT"), *lq = getenv("CRSDR_LONG_Q");
        const char c = v ? v[0] : 'a';
        return Switches{(c == 'p' || c == 'q' || c == 'r') ? c : 'a', spin_switch(getenv("CRSDR_K1_QSPIN"), x14p::kQSpinLimit),
                        spin_switch(getenv("CRSDR_K1_REFSPIN"), kRefWaitBudget), spin_switch(getenv("CRSDR_K2_SPIN"), kFusedSpinLimit).value,
                        !lq || atoi(lq) != 0};
    }();
    return s;
}

static int device_cus()
{
    static const int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
        return n;
    }();
    return cus;
}
static bool two_row(char variant) { return variant == 'q' || variant == 'r'; }
// which B = 16384 cross-correlation kernel a launch of rows_all rows takes: 'q' / 'r' (two rows per CU) or 'p' (one)
static char k1_pick(int rows_all, bool allow_q)
{
    char variant = sw().k1_variant;
    // measured (r01, T = 64): q is 3-7 % faster at 1024 / 256 / 128 / 96 / 48 rows per block (256 ... 12 rows per CU and launch),
    // 1.4 % at 64, level with p at 32 and 21 rows (8 and 5 per CU; r03: level at 10 as well)
    if (variant == 'a') variant = rows_all >= 12 * device_cus() ? 'r' : 'p';
    if (two_row(variant) && !allow_q) variant = 'p';   // a plan whose two-row kernel once ran out of a bounded wait stays on the packed kernel
    return variant;
}

// ---- kernel launchers, dispatched on log2(B) ------------------------------------------------------
// every launch: the kernel's dynamic LDS limit (set each time), the launch, the launch's error
template <typename Kernel, typename... Args>
static hipError_t launch_lds(Kernel kern, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args &...args)
{
    const hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, block, lds, s, args...);
    return hipGetLastError();
}

template <int LOG2N>
static hipError_t launch_ref_spectrum(hipStream_t s, int nblocks, const int8_t *rows, size_t block_stride, const float2 *tw,
                                      float2 *refspec, uint32_t xor80)
{
    return launch_lds(k_ref_spectrum<LOG2N>, dim3(nblocks), dim3(FftGeom<LOG2N>::THREADS), fft_lds_bytes<LOG2N>(), s, rows, block_stride, tw,
                      refspec, xor80);
}

template <int LOG2N>
static hipError_t launch_xcorr_lag(hipStream_t s, const XcorrArgs &a, int row_count, const float2 *tw)
{
    return launch_lds(k_xcorr_lag<LOG2N>, dim3(row_count, a.nblocks), dim3(FftGeom<LOG2N>::THREADS), fft_lds_bytes<LOG2N>(), s, a, tw);
}

static hipError_t launch_ref_spectrum14(hipStream_t s, int nblocks, const int8_t *rows, size_t block_stride, const float2 *twA,
                                        const float2 *twB, float2 *refspec, uint32_t xor80)
{
    return launch_lds(x14p::k_ref_spectrum14p, dim3(nblocks), dim3(x14::THREADS), x14::LDS_BYTES, s, rows, block_stride,
                      reinterpret_cast<const c2 *>(twA), reinterpret_cast<const c2 *>(twB), (float4 *)refspec, xor80);
}

// B = 16384 cross-correlation on the kernel the caller picked (k1_pick; 'p' for a folded launch)
static hipError_t launch_xcorr_lag14(hipStream_t s, char variant, const XcorrArgs &a, int row_count, const float2 *twA, const float2 *twB,
                                     int *waitflag, unsigned int *work, unsigned int *work_base)
{
    const int items = row_count * a.nblocks + (a.fold ? a.nblocks : 0);
    if (!two_row(variant))
        return launch_lds(x14p::k_xcorr_lag14p, dim3((unsigned)items), dim3(x14::THREADS), x14::LDS_BYTES, s, a, twA, twB, row_count);
    // two rows per CU in opposite phases (xcorr14q.hpp), one persistent workgroup per CU
    static long launches = 0;
    const int qspin = sw().qspin.at(launches++);
    const hipError_t e = launch_lds(variant == 'r' ? x14p::k_xcorr_lag14r : x14p::k_xcorr_lag14q, dim3((unsigned)std::max(1, std::min(device_cus(), (items + 1) / 2))), dim3(2 * x14p::QG),
                                    x14p::LDSQ14_BYTES, s, a, twA, twB, row_count, waitflag, work, *work_base, qspin);
    if (e == hipSuccess) *work_base += (unsigned)items;      // a launch that ran advances the device counter by exactly its item count (xcorr14q.hpp)
    return e;
}

template <int LOG2N, int DIR>
static hipError_t launch_op_fft(hipStream_t s, int howmany, float2 *out, const float2 *in, const float2 *tw)
{
    return launch_lds(k_op_fft<LOG2N, DIR>, dim3(howmany), dim3(FftGeom<LOG2N>::THREADS), fft_lds_bytes<LOG2N>(), s, out, in, tw);
}

// ---- long-block path (B = N1 x 16384) ----------------------------------------------------------------
#define CRSDR_DISPATCH_N1(l2, CALL)                                                     \
    [&]() -> hipError_t {                                                               \
        switch (l2) {                                                                   \
        case 1: { constexpr int LG = 1; return CALL; }                                  \
        case 2: { constexpr int LG = 2; return CALL; }                                  \
        case 3: { constexpr int LG = 3; return CALL; }                                  \
        case 4: { constexpr int LG = 4; return CALL; }                                  \
        case 5: { constexpr int LG = 5; return CALL; }                                  \
        case 6: { constexpr int LG = 6; return CALL; }                                  \
        case 7: { constexpr int LG = 7; return CALL; }                                  \
        case 8: { constexpr int LG = 8; return CALL; }                                  \
        default: return hipErrorInvalidValue;                                           \
        }                                                                               \
    }()

// column passes of the long-block path: persistent workgroups, two per CU (64 KiB tiles), each walking its share of the
// (row, tile) work items with the next item's loads in flight (longblock.hpp); CRSDR_LONG_PERSIST=0: one workgroup per item
static int lb_grid(int nwork, bool stage_c = false)
{
    // stage A: persistent, two workgroups per CU (what the 64 KiB tiles allow); stage C (reads only) is better off with one
    // workgroup per item: measured r02, cfg5, per launch of 10.5 rows: 55 us against 61 us persistent (its reads alone run at
    // 4.1 TB/s either way: 43 us); stage A (mostly stores) gains: 61 -> 52 us
    const int per_cu = stage_c ? 0 : 2;
#ifdef CRSDR_LB_EXPERIMENT
    static const int dbg_set = [] { const char *e = getenv("CRSDR_LB_DBG"); int v = e ? atoi(e) : 0; (void)hipMemcpyToSymbol(HIP_SYMBOL(lb::lb_dbg), &v, sizeof(v)); return v; }();
    (void)dbg_set;
#endif
    return per_cu > 0 ? std::max(1, std::min(nwork, per_cu * device_cus())) : nwork;
}
template <int LOG2N1, bool IS_REF>
static hipError_t launch_long_fwd_cols(hipStream_t s, int nrows_launch, const int8_t *rows, int row_begin, uint32_t xor80,
                                       const lb::LongTw &tw, float2 *Y)
{
    const int nwork = lb::ntiles(LOG2N1) * nrows_launch;
    return launch_lds(lb::k_long_fwd_cols<LOG2N1, IS_REF>, dim3((unsigned)lb_grid(nwork)), dim3(lb::THREADS), lb::LDS_BYTES, s, rows, row_begin,
                      xor80, tw, Y, nwork);
}
// stage B with two lines per CU in opposite phases (k_rows14_cf32q): a line's HBM phases run beside the other line's transforms
static hipError_t launch_long_rows_q(hipStream_t s, int n1, int nrows_launch, float2 *Y, const float2 *twA, const float2 *twB, float2 *refspec,
                                     int *waitflag, const x14p::RampArgs *ramp = nullptr, float2 *Yout = nullptr)
{
    const int items = n1 * nrows_launch;
    // (r03: dealing the lines to just as many workgroups as make every round full -- cfg5: 2688 lines = 6 rounds x 448 groups on 224
    // CUs instead of 5 full rounds and a sixth with 128 lines -- measured level: 2 473 / 2 544 against 2 500 / 2 549 blocks/s)
    const int grid = std::max(1, std::min(device_cus(), (items + 1) / 2));
    // one queue per XCD (k_rows14_cf32q); static order: the work counter is not used.  (The apply pass's per-row spectra are
    // 2.7 MB for cfg5 and stay in every L2: lines in memory order there.)
    const int nq = (!ramp && n1 % 8 == 0 && grid % 8 == 0) ? 8 : 1;
    static long launches = 0;
    const int qspin = sw().qspin.at(launches++);
    return launch_lds(ramp ? x14p::k_rows14_cf32q<true> : x14p::k_rows14_cf32q<false>, dim3((unsigned)grid), dim3(2 * x14p::QG), x14p::LDSQ_BYTES, s,
                      reinterpret_cast<c2 *>(Y), reinterpret_cast<const c2 *>(twA), reinterpret_cast<const c2 *>(twB), (const float4 *)refspec, n1,
                      nrows_launch, nq, waitflag, qspin, ramp ? *ramp : x14p::RampArgs{}, reinterpret_cast<c2 *>(Yout));
}
// stage B: the 16384-point row transforms run on the 32x32x16 structure of xcorr14.hpp
template <bool IS_REF>
static hipError_t launch_long_rows(hipStream_t s, int n1, int nrows_launch, float2 *Y, const float2 *twA, const float2 *twB, float2 *refspec)
{
    return launch_lds(x14p::k_rows14_cf32p<IS_REF, false>, dim3(n1, nrows_launch), dim3(x14::THREADS), x14::LDS_BYTES, s, reinterpret_cast<c2 *>(Y),
                      reinterpret_cast<const c2 *>(twA), reinterpret_cast<const c2 *>(twB), (float4 *)refspec, x14p::RampArgs{});
}
// apply pass of crsdr_plan_set_frac_apply: row transforms with the row's fractional-delay response, then column transforms to int8
static hipError_t launch_long_rows_ramp(hipStream_t s, int n1, int nrows_launch, float2 *Y, const float2 *twA, const float2 *twB, const x14p::RampArgs &ra)
{
    return launch_lds(x14p::k_rows14_cf32p<false, true>, dim3(n1, nrows_launch), dim3(x14::THREADS), x14::LDS_BYTES, s, reinterpret_cast<c2 *>(Y),
                      reinterpret_cast<const c2 *>(twA), reinterpret_cast<const c2 *>(twB), (float4 *)nullptr, ra);
}
static hipError_t launch_long_rows_ref1(hipStream_t s, float2 *Y, const float2 *twA, const float2 *twB, float2 *refspec)
{
    return launch_long_rows<true>(s, 1, 1, Y, twA, twB, refspec);
}
// inverse column passes: stage C of the correlation pass (argmax partials into part) or, OUT, the apply pass's int8 rows into out
template <int LOG2N1, bool OUT = false>
static hipError_t launch_long_inv_cols(hipStream_t s, int nrows_launch, const float2 *Z, const lb::LongTw &tw, lb::LongPartial *part, int8_t *out)
{
    const int nwork = lb::ntiles(LOG2N1) * nrows_launch;
    return launch_lds(lb::k_long_inv_cols<LOG2N1, OUT>, dim3((unsigned)lb_grid(nwork, !OUT)), dim3(lb::THREADS), lb::LDS_BYTES, s, Z, tw, part, out, nwork);
}

template <int LOG2N>
static hipError_t launch_frac_apply(hipStream_t s, int row_count, int nblocks, const FracArgs &fa, const float2 *tw, const float2 *twA, const float2 *twB,
                                    const uint32_t *k2tab)
{
    if constexpr (LOG2N == 14) {
        if (k2tab && twA && twB) {             // the pass on K1's 32 x 32 x 16 network (xcorr14p.hpp)
            x14p::FracRowArgs ra{fa.rows, fa.block_stride, fa.packet, fa.packet_stride, fa.slab, fa.slab_stride, fa.nrows, fa.row_begin, fa.xor80, fa.lag, fa.frac,
                                 fa.frac_override, fa.gain, fa.phasor, k2tab, tw};
            constexpr int lds14 = x14::LDS_BYTES + 2048;          // the image + the row's two response tables
            return launch_lds(x14p::k_frac_apply14, dim3(row_count, nblocks), dim3(x14::THREADS), lds14, s, ra, twA, twB);
        }
    }
    return launch_lds(k_frac_apply<LOG2N>, dim3(row_count, nblocks), dim3(FftGeom<LOG2N>::THREADS), fft_lds_bytes<LOG2N>(), s, fa, tw);
}

#define CRSDR_DISPATCH_LOG2(l2, CALL)                                                   \
    [&]() -> hipError_t {                                                               \
        switch (l2) {                                                                   \
        case 4: { constexpr int LG = 4; return CALL; }                                  \
        case 5: { constexpr int LG = 5; return CALL; }                                  \
        case 6: { constexpr int LG = 6; return CALL; }                                  \
        case 7: { constexpr int LG = 7; return CALL; }                                  \
        case 8: { constexpr int LG = 8; return CALL; }                                  \
        case 9: { constexpr int LG = 9; return CALL; }                                  \
        case 10: { constexpr int LG = 10; return CALL; }                                \
        case 11: { constexpr int LG = 11; return CALL; }                                \
        case 12: { constexpr int LG = 12; return CALL; }                                \
        case 13: { constexpr int LG = 13; return CALL; }                                \
        case 14: { constexpr int LG = 14; return CALL; }                                \
        default: return hipErrorInvalidValue;                                           \
        }                                                                               \
    }()

// ================================================================================================
// (i) per-op entry points (class cdsp).  Host pointers; staged through grow-only device buffers.
// ================================================================================================
namespace {
struct OpCtx {
    std::mutex mu;
    void *buf[9] = {};                                        // [3]: the tiled covariance's partial sums; [4], [5]: crsdr_refine2d's further arguments; .. [8]: crsdr_esprit2d's
    size_t cap[9] = {};
    float2 *tw[kMaxLog2 + 1] = {};
    int tw_dev[kMaxLog2 + 1] = {};
    int dev = -1;
};
OpCtx g_op;

int op_reserve(int slot, size_t bytes)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (g_op.dev != dev) {
        for (int i = 0; i < 9; ++i) { if (g_op.buf[i]) (void)hipFree(g_op.buf[i]); g_op.buf[i] = nullptr; g_op.cap[i] = 0; }
        for (int i = 0; i <= kMaxLog2; ++i) { if (g_op.tw[i]) (void)hipFree(g_op.tw[i]); g_op.tw[i] = nullptr; }
        g_op.dev = dev;
    }
    if (g_op.cap[slot] >= bytes) return CRSDR_OK;
    if (g_op.buf[slot]) (void)hipFree(g_op.buf[slot]);
    g_op.buf[slot] = nullptr; g_op.cap[slot] = 0;
    size_t want = bytes < 4096 ? 4096 : bytes;
    HIP_TRY(hipMalloc(&g_op.buf[slot], want));
    g_op.cap[slot] = want;
    return CRSDR_OK;
}

inline dim3 grid1d(size_t n, int bs = 256) { return dim3((unsigned)((n + bs - 1) / bs)); }
} // namespace

#define OP_PROLOGUE(cond, msg)                                \
    if (!(cond)) return fail(CRSDR_EINVAL, msg);              \
    { int rc_ = require_device(); if (rc_) return rc_; }      \
    std::lock_guard<std::mutex> lock_(g_op.mu)

// the same for the downstream calls, which take host or device pointers: behind their own argument checks
#define OP_PROLOGUE_MEM(who, mem_kind)                                                                                              \
    if (mem_kind != CRSDR_MEM_HOST && mem_kind != CRSDR_MEM_DEVICE) return fail(CRSDR_EINVAL, who ": mem_kind = %d", mem_kind);   \
    { int rc_ = require_device(); if (rc_) return rc_; }                                                                            \
    std::lock_guard<std::mutex> lock_(g_op.mu)

#define OP_RESERVE(slot, bytes) { int rc_ = op_reserve(slot, bytes); if (rc_) return rc_; }

// The mem_kind pattern of the downstream per-op calls (under g_op.mu).  CRSDR_MEM_HOST: inputs are copied into staging slots, the
// kernels write into slots, back() copies out.  CRSDR_MEM_DEVICE: the caller's pointers as they are (misaligned: one of them missed
// the alignment its call asks for), finish() waits for the device.  rc: the first failure; the calls behind it do nothing.
struct OpStage {
    const bool host;
    bool misaligned = false;
    int rc = CRSDR_OK;
    explicit OpStage(int mem_kind) : host(mem_kind == CRSDR_MEM_HOST) {}
    const void *in(int slot, const void *p, size_t bytes, size_t align = 1)
    {
        void *d = out(slot, const_cast<void *>(p), bytes, align);
        if (host && !rc) rc = HIP_RC(hipMemcpy(d, p, bytes, hipMemcpyHostToDevice));
        return d;
    }
    void *out(int slot, void *p, size_t bytes, size_t align = 1)
    {
        if (!host) { misaligned |= (uintptr_t)p % align != 0; return p; }
        if (!rc) rc = op_reserve(slot, bytes);
        return g_op.buf[slot];
    }
    // device memory and an output not asked for (d = NULL behind out()): the kernels write it all the same, into the slot.  Returns rc.
    template <typename T>
    int spare(int slot, T *&d, size_t bytes)
    {
        if (!d && !rc && !(rc = op_reserve(slot, bytes))) d = (T *)g_op.buf[slot];
        return rc;
    }
    void back(void *p, const void *d, size_t bytes) { if (host && p && !rc) rc = HIP_RC(hipMemcpy(p, d, bytes, hipMemcpyDeviceToHost)); }
    int finish() { return rc || host ? rc : HIP_RC(hipDeviceSynchronize()); }
};

extern "C" int crsdr_convtosigned(const uint8_t *in, uint8_t *out, int n)
{
    OP_PROLOGUE(in && out && n > 0 && (n % 8) == 0, "convtosigned: need in, out, n > 0, n % 8 == 0");
    OP_RESERVE(0, n); OP_RESERVE(1, n);
    HIP_TRY(hipMemcpy(g_op.buf[0], in, n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_op_convtosigned, grid1d(n / 4), dim3(256), 0, 0, (const uint32_t *)g_op.buf[0], (uint32_t *)g_op.buf[1], n / 4);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, g_op.buf[1], n, hipMemcpyDeviceToHost));
    return CRSDR_OK;
}

extern "C" int crsdr_convtofloat(float *out, const int8_t *s8bit, int n)
{
    OP_PROLOGUE(out && s8bit && n > 0, "convtofloat: need out, s8bit, n > 0");
    OP_RESERVE(0, n); OP_RESERVE(1, sizeof(float) * (size_t)n);
    HIP_TRY(hipMemcpy(g_op.buf[0], s8bit, n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_op_convtofloat, grid1d(n), dim3(256), 0, 0, (float *)g_op.buf[1], (const int8_t *)g_op.buf[0], n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, g_op.buf[1], sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    return CRSDR_OK;
}

extern "C" int crsdr_scalarmul(float *out, const float *in, float sre, float sim, int n)
{
    OP_PROLOGUE(out && in && n > 0, "scalarmul: need out, in, n > 0");
    const size_t bytes = sizeof(float2) * (size_t)n;
    OP_RESERVE(0, bytes); OP_RESERVE(1, bytes);
    HIP_TRY(hipMemcpy(g_op.buf[0], in, bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_op_scalarmul, grid1d(n), dim3(256), 0, 0, (float2 *)g_op.buf[1], (const float2 *)g_op.buf[0], make_float2(sre, sim), n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, g_op.buf[1], bytes, hipMemcpyDeviceToHost));
    return CRSDR_OK;
}

extern "C" int crsdr_convto8bit(int8_t *out, const float *in, int n)
{
    OP_PROLOGUE(out && in && n > 0, "convto8bit: need out, in, n > 0");
    const size_t nf = 2 * (size_t)n; // the reference doubles n internally (src/cdsp.cc:52)
    OP_RESERVE(0, sizeof(float) * nf); OP_RESERVE(1, nf);
    HIP_TRY(hipMemcpy(g_op.buf[0], in, sizeof(float) * nf, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_op_convto8bit, grid1d(nf), dim3(256), 0, 0, (int8_t *)g_op.buf[1], (const float *)g_op.buf[0], (int)nf);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, g_op.buf[1], nf, hipMemcpyDeviceToHost));
    return CRSDR_OK;
}

extern "C" int crsdr_conj_dotproduct(float *res, const float *a, const float *b, int n)
{
    OP_PROLOGUE(res && a && b && n > 0, "conj_dotproduct: need res, a, b, n > 0");
    const size_t bytes = sizeof(float2) * (size_t)n;
    OP_RESERVE(0, bytes); OP_RESERVE(1, bytes); OP_RESERVE(2, 16);
    HIP_TRY(hipMemcpy(g_op.buf[0], a, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g_op.buf[1], b, bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_op_conj_dot, dim3(1), dim3(1024), 0, 0, (float *)g_op.buf[2], (const float2 *)g_op.buf[0], (const float2 *)g_op.buf[1], n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(res, g_op.buf[2], 2 * sizeof(float), hipMemcpyDeviceToHost));
    return CRSDR_OK;
}

extern "C" int crsdr_magsquared(float *out, const float *in, int n)
{
    OP_PROLOGUE(out && in && n > 0, "magsquared: need out, in, n > 0");
    OP_RESERVE(0, sizeof(float2) * (size_t)n); OP_RESERVE(1, sizeof(float) * (size_t)n);
    HIP_TRY(hipMemcpy(g_op.buf[0], in, sizeof(float2) * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_op_magsquared, grid1d(n), dim3(256), 0, 0, (float *)g_op.buf[1], (const float2 *)g_op.buf[0], n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, g_op.buf[1], sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    return CRSDR_OK;
}

extern "C" int crsdr_conjugatemul(float *out, const float *in1, const float *in2, int n)
{
    OP_PROLOGUE(out && in1 && in2 && n > 0, "conjugatemul: need out, in1, in2, n > 0");
    const size_t bytes = sizeof(float2) * (size_t)n;
    OP_RESERVE(0, bytes); OP_RESERVE(1, bytes); OP_RESERVE(2, bytes);
    HIP_TRY(hipMemcpy(g_op.buf[0], in1, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g_op.buf[1], in2, bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_op_conjugatemul, grid1d(n), dim3(256), 0, 0, (float2 *)g_op.buf[2], (const float2 *)g_op.buf[0], (const float2 *)g_op.buf[1], n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, g_op.buf[2], bytes, hipMemcpyDeviceToHost));
    return CRSDR_OK;
}

extern "C" int crsdr_indexofmax(uint32_t *index, const float *in, int n)
{
    OP_PROLOGUE(index && in && n > 0, "indexofmax: need index, in, n > 0");
    OP_RESERVE(0, sizeof(float) * (size_t)n); OP_RESERVE(2, 16);
    HIP_TRY(hipMemcpy(g_op.buf[0], in, sizeof(float) * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_op_indexofmax, dim3(1), dim3(1024), 0, 0, (uint32_t *)g_op.buf[2], (const float *)g_op.buf[0], n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(index, g_op.buf[2], sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CRSDR_OK;
}

extern "C" int crsdr_fft(float *out, const float *in, int n, int sign, int howmany)
{
    OP_PROLOGUE(out && in && howmany > 0 && (sign == 1 || sign == -1), "fft: need out, in, howmany > 0, sign = +-1");
    const int l2 = ilog2_exact(n);
    if (l2 < kMinLog2 || l2 > kMaxLog2)
        return fail(CRSDR_EINVAL, "fft: n = %d unsupported (power of two in [16, 16384])", n);
    const size_t bytes = sizeof(float2) * (size_t)n * (size_t)howmany;
    OP_RESERVE(0, bytes); OP_RESERVE(1, bytes);
    if (!g_op.tw[l2]) { int rc = make_twiddles(n, &g_op.tw[l2]); if (rc) return rc; }
    HIP_TRY(hipMemcpy(g_op.buf[0], in, bytes, hipMemcpyHostToDevice));
    const float2 *tw = g_op.tw[l2];
    hipError_t e = (sign < 0)
        ? CRSDR_DISPATCH_LOG2(l2, (launch_op_fft<LG, -1>(0, howmany, (float2 *)g_op.buf[1], (const float2 *)g_op.buf[0], tw)))
        : CRSDR_DISPATCH_LOG2(l2, (launch_op_fft<LG, +1>(0, howmany, (float2 *)g_op.buf[1], (const float2 *)g_op.buf[0], tw)));
    HIP_TRY(e);
    HIP_TRY(hipMemcpy(out, g_op.buf[1], bytes, hipMemcpyDeviceToHost));
    return CRSDR_OK;
}

// ---- (iii) downstream helper: sample covariance of the aligned matrix on the matrix cores ----
// K split of the tiled kernel: the split that minimises rounds-of-workgroups x a tile's time / S + the partial sums' write and read
// time x S.  A tile's time is what its CU takes to pull the 2 x 128 rows in (measured ~50 GB/s per CU from L2 under the MFMAs; the
// matrix cores' share, 2 MFMAs per operand pair at 9.8e12 int8 MACs/s per CU, is shorter); the partials move at ~5 TB/s.
static int cov_pick_split(int ntri, int npairs, int blocksize, int cus)
{
    const double mfma_us = 2.0 * cov::CT * cov::CT * (double)blocksize / 9.8e6, ingest_us = 2.0 * cov::CT * (double)blocksize / 5e4;
    const double tile_us = std::max(mfma_us, ingest_us), part_us = (double)ntri * 2 * cov::CT * cov::CT * 4 * 2 / 5e6;
    // a workgroup's int32 partial sums are exact while its K range is <= 65536 bytes (|sum| <= 32768 samples x 2 x 128^2 = 2^30)
    const int s_min = std::max(1, (blocksize + 65535) / 65536);
    int best = s_min;
    double best_cost = 1e30;
    for (int s = s_min; s <= std::max(s_min, std::min(npairs, 32)); ++s) {
        const double cost = (double)((ntri * s + cus - 1) / cus) / s * tile_us + s * part_us;
        if (cost < best_cost) { best_cost = cost; best = s; }
    }
    return best;
}

extern "C" int crsdr_covariance(float *rxx, const int8_t *matrix, int nrows, int blocksize, int mem_kind)
{
    if (!rxx || !matrix || nrows < 2 || blocksize < 32 || (blocksize % 32)) return fail(CRSDR_EINVAL, "covariance: need rxx, matrix, nrows >= 2, blocksize % 32 == 0");
    OP_PROLOGUE_MEM("covariance", mem_kind);
    const size_t mb = (size_t)nrows * (size_t)blocksize, nsig = (size_t)nrows - 1, rb = sizeof(float2) * nsig * nsig;
    OpStage st(mem_kind);
    const int8_t *d_m = (const int8_t *)st.in(0, matrix, mb);
    float2 *d_r = (float2 *)st.out(1, rxx, rb);
    if (st.rc) return st.rc;
    // (the one-tile-per-wave kernel keeps a whole row's sums in int32: exact up to 65536 bytes per row; longer rows take the tiled path,
    // whose K split keeps every partial inside that bound, whatever the channel count)
    if (blocksize > 65536 && (blocksize % (2 * cov::KC) || (uintptr_t)d_m % 4))
        return fail(CRSDR_EINVAL, "covariance: blocksize above 65536 must be a multiple of %d (and the matrix 4-byte aligned)", 2 * cov::KC);
    if (blocksize % (2 * cov::KC) == 0 && (uintptr_t)d_m % 4 == 0 && (nsig >= 64 || blocksize > 65536)) {
        // LDS-tiled form: 128 x 128 tiles on / above the diagonal, the K range split (in pairs of chunks) over the grid
        const int nt = (int)((nsig + cov::CT - 1) / cov::CT), ntri = nt * (nt + 1) / 2, npairs = blocksize / (2 * cov::KC);
        const int S = cov_pick_split(ntri, npairs, blocksize, device_cus());
        const unsigned grid = 8u * (unsigned)((ntri * S + 7) / 8);
        OP_RESERVE(2, sizeof(int2) * (size_t)nt * cov::CT * (size_t)S);
        OP_RESERVE(3, sizeof(int) * 2 * cov::CT * cov::CT * (size_t)ntri * (size_t)S);
        HIP_TRY(hipFuncSetAttribute((const void *)cov::k_covariance_tiled, hipFuncAttributeMaxDynamicSharedMemorySize, cov::COV_LDS_BYTES));
        hipLaunchKernelGGL(cov::k_covariance_tiled, dim3(grid), dim3(cov::COV_THREADS), cov::COV_LDS_BYTES, 0, d_m, nrows, blocksize, nt, ntri, S, (int *)g_op.buf[3],
                           (int2 *)g_op.buf[2]);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(cov::k_cov_reduce, dim3((unsigned)ntri, cov::CT / cov::CR), dim3(256), 0, 0, (const int *)g_op.buf[3], (const int2 *)g_op.buf[2], S, ntri, nt,
                           nrows, blocksize, d_r);
        HIP_TRY(hipGetLastError());
    } else {
        const unsigned tiles = (unsigned)((nsig + 63) / 64);
        OP_RESERVE(2, sizeof(int2) * (size_t)nrows);
        hipLaunchKernelGGL(cov::k_row_sums, dim3(nrows), dim3(256), 0, 0, d_m, blocksize, (int2 *)g_op.buf[2]);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(cov::k_covariance, dim3(tiles, tiles), dim3(256), 0, 0, d_m, nrows, blocksize, (const int2 *)g_op.buf[2], d_r);
        HIP_TRY(hipGetLastError());
    }
    st.back(rxx, d_r, rb);
    return st.finish();
}

extern "C" int crsdr_noisesubspace(float *vec, float *sv, const float *rxx, int m, int mem_kind)
{
    if (!vec || !rxx || m < 2 || m > music::MAX_M) return fail(CRSDR_EINVAL, "noisesubspace: need vec, rxx, 2 <= m <= %d", music::MAX_M);
    OP_PROLOGUE_MEM("noisesubspace", mem_kind);
    const size_t mm = sizeof(float2) * (size_t)m * m;
    OP_RESERVE(2, music::MAX_M * sizeof(float) + 2 * sizeof(int));
    float *d_sv = (float *)g_op.buf[2];
    int *d_info = (int *)((char *)g_op.buf[2] + music::MAX_M * sizeof(float));
    const float2 *d_r = (const float2 *)rxx;
    float2 *d_v = (float2 *)vec;
    if (mem_kind == CRSDR_MEM_HOST) {
        OP_RESERVE(0, mm); OP_RESERVE(1, mm);
        HIP_TRY(hipMemcpy(g_op.buf[0], rxx, mm, hipMemcpyHostToDevice));
        d_r = (const float2 *)g_op.buf[0];
        d_v = (float2 *)g_op.buf[1];
    }
    const size_t lds = 2 * sizeof(double2) * (size_t)m * m;
    HIP_TRY(hipFuncSetAttribute((const void *)music::k_herm_subspace, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(music::k_herm_subspace, dim3(1), dim3(music::JT), lds, 0, d_r, m, d_sv, d_v, d_info);
    HIP_TRY(hipGetLastError());
    int info[2] = {0, 0};
    HIP_TRY(hipMemcpy(info, d_info, sizeof(info), hipMemcpyDeviceToHost));
    if (mem_kind == CRSDR_MEM_HOST) {
        HIP_TRY(hipMemcpy(vec, d_v, mm, hipMemcpyDeviceToHost));
        if (sv) HIP_TRY(hipMemcpy(sv, d_sv, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost));
    } else if (sv) {
        HIP_TRY(hipMemcpy(sv, d_sv, sizeof(float) * (size_t)m, hipMemcpyDeviceToDevice));
    }
    if (!info[1]) return fail(CRSDR_ESTATE, "noisesubspace: Jacobi iteration not converged after %d sweeps", info[0]);
    return CRSDR_OK;
}

extern "C" int crsdr_pmusic2d(float *pm, const float *vec, int m, int k, float d, int mx, int my, int ncx, int ncy, int mem_kind)
{
    if (!pm || !vec || m < 2 || m > music::MAX_M || mx < 1 || my < 1 || mx * my != m || k < 1 || k >= m || ncx < 1 || ncy < 1 ||
        (long long)ncx * ncy > (1 << 24))
        return fail(CRSDR_EINVAL, "pmusic2d: need pm, vec, m = mx*my in [2, %d], 1 <= k < m, grid <= 2^24 points", music::MAX_M);
    OP_PROLOGUE_MEM("pmusic2d", mem_kind);
    const size_t mm = sizeof(float2) * (size_t)m * m, pb = sizeof(float) * (size_t)ncx * ncy;
    OpStage st(mem_kind);
    const float2 *d_v = (const float2 *)st.in(0, vec, mm);
    float *d_p = (float *)st.out(1, pm, pb);
    if (st.rc) return st.rc;
    const int nn = m - k;
    const size_t lds = sizeof(float2) * ((size_t)m * nn + (size_t)m * music::PT);
    HIP_TRY(hipFuncSetAttribute((const void *)music::k_pmusic2d, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned blocks = (unsigned)(((size_t)ncx * ncy + music::PT - 1) / music::PT);
    hipLaunchKernelGGL(music::k_pmusic2d, dim3(blocks), dim3(music::PT), lds, 0, d_v, m, m, k, nn, d, mx, my, ncx, ncy, d_p);
    HIP_TRY(hipGetLastError());
    st.back(pm, d_p, pb);
    return st.finish();
}

extern "C" int crsdr_smooth_covariance(float *rs, const float *rxx, int mx, int my, int sx, int sy, uint32_t flags, int mem_kind)
{
    if (!rs || !rxx || !smooth_shape_ok(mx, my, sx, sy, flags))
        return fail(CRSDR_EINVAL, "smooth_covariance: need rs, rxx, m = mx*my in [2, %d], 1 <= sx <= mx, 1 <= sy <= my, sx*sy >= 2, flags = 0 or CRSDR_SMOOTH_FB",
                    music::MAX_M);
    OP_PROLOGUE_MEM("smooth_covariance", mem_kind);
    const size_t m = (size_t)mx * my, ms = (size_t)sx * sy, mm = sizeof(float2) * m * m, sb = sizeof(float2) * ms * ms;
    OpStage st(mem_kind);
    const float2 *d_r = (const float2 *)st.in(0, rxx, mm);
    float2 *d_s = (float2 *)st.out(1, rs, sb);
    if (st.rc) return st.rc;
    hipLaunchKernelGGL(smooth::k_smooth_covariance, dim3(1), dim3(smooth::SM_THREADS), 0, 0, d_r, mx, my, sx, sy, flags, d_s);
    HIP_TRY(hipGetLastError());
    st.back(rs, d_s, sb);
    return st.finish();
}

extern "C" int crsdr_source_order(int32_t *k, float *criterion_values, const float *sv, int m, int64_t nsnap, int criterion, int kmin, int kmax, int mem_kind)
{
    if (!k || !sv || m < 2 || m > music::MAX_M || nsnap < 1 || (criterion != CRSDR_ORDER_MDL && criterion != CRSDR_ORDER_AIC) || kmin < 1 || kmin > kmax ||
        kmax >= m)
        return fail(CRSDR_EINVAL, "source_order: need k, sv, 2 <= m <= %d, nsnap >= 1, criterion MDL or AIC, 1 <= kmin <= kmax < m", music::MAX_M);
    OP_PROLOGUE_MEM("source_order", mem_kind);
    const size_t nc = (size_t)(kmax - kmin + 1);
    // one staging buffer: sv [MAX_M] float, crit [MAX_M] float, k
    OP_RESERVE(2, (2 * music::MAX_M) * sizeof(float) + sizeof(int32_t));
    float *s_sv = (float *)g_op.buf[2], *s_crit = s_sv + music::MAX_M;
    int32_t *s_k = (int32_t *)(s_crit + music::MAX_M);
    const bool host = mem_kind == CRSDR_MEM_HOST;
    if (host) HIP_TRY(hipMemcpy(s_sv, sv, sizeof(float) * (size_t)m, hipMemcpyHostToDevice));
    float *d_crit = host || !criterion_values ? s_crit : criterion_values;
    hipLaunchKernelGGL(smooth::k_doa_order, dim3(1), dim3(64), 0, 0, host ? (const float *)s_sv : sv, m, (double)nsnap, criterion, kmin, kmax, host ? s_k : k,
                       d_crit);
    HIP_TRY(hipGetLastError());
    if (host) {
        HIP_TRY(hipMemcpy(k, s_k, sizeof(int32_t), hipMemcpyDeviceToHost));
        if (criterion_values) HIP_TRY(hipMemcpy(criterion_values, s_crit, sizeof(float) * nc, hipMemcpyDeviceToHost));
    } else
        HIP_TRY(hipDeviceSynchronize());
    return CRSDR_OK;
}

// ================================================================================================
// (ii) batched plan
// ================================================================================================
constexpr int kStageSlots = 4;
// launches whose bounded waits report into d_sync[2] (crsdr_plan::k1_waits)
constexpr unsigned kWaitTwoRow = 1u, kWaitTwoLine = 2u, kWaitFoldRef = 4u;
constexpr int kMaxBatch = 64;

struct crsdr_plan {
    int nrows = 0, B = 0, L = 0, log2n = 0, mode = 0, device = 0, row_begin = 1, row_count = 0, max_batch = 1;
    size_t packet_bytes = 0, matrix_off = 0, packet_stride = 0, own_packet_stride = 0;
    hipStream_t own_stream = nullptr, stream = nullptr, aux = nullptr;
    hipEvent_t ev_fork = nullptr, ev_ref[2] = {nullptr, nullptr}, ev_k1done[2] = {nullptr, nullptr};
    // per-batch {lag, mag, frac} are double-buffered (obuf: a pipelined fetch of batch b reads its buffer while batch b + 1 writes the
    // other), ev_k2done[i] = the last kernel of the batch that wrote buffer i has finished
    hipStream_t cs = nullptr;                       // copy stream of crsdr_plan_fetch_batch_async
    hipEvent_t ev_copydone[4] = {nullptr, nullptr, nullptr, nullptr};   // one per outstanding asynchronous fetch (ring)
    unsigned long copy_head = 0, copy_tail = 0;      // fetches waited for / issued
    int *h_k1flag = nullptr;                         // page-locked [4]: the two-row K1's error word as copied by each asynchronous fetch
    bool copy_pending = false;                       // the next submit's kernels wait for the newest of them
    hipEvent_t ev_k2done[2] = {nullptr, nullptr};
    int obuf = 0;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    bool k1done_valid[2] = {false, false};
    // the last user of d_refspec[slot] was a folded K1 launch (written and read on the main stream, no ev_k1done record): the next
    // unfolded batch on that slot records ev_k1done[slot] on the main stream before its K0 on the aux stream may overwrite the slot
    bool fold_last[2] = {false, false};
    int slot = 0;
    float2 *d_tw = nullptr, *d_twA = nullptr, *d_twB = nullptr, *d_refspec[2] = {nullptr, nullptr}; // [T][B] each
    int8_t *d_rows = nullptr;          // staging for host input [T][nrows][B]
    uint8_t *d_packet_alloc = nullptr; // own packet allocation (front padding for alignment)
    int8_t *d_packet_own = nullptr, *d_packet = nullptr;
    int8_t *d_slab = nullptr;          // slab output mode (crsdr_plan_bind_slab), caller-owned
    size_t slab_stride = 0, tail_offset = 0;   // tail_offset: crsdr_plan_bind_slab_ex -- per-row scalars after the rows of every slot
    int hdr_first = 0, hdr_count = 0;
    uint32_t *d_readcnt = nullptr;     // [T][nrows]
    uint8_t *d_mask = nullptr;
    int32_t *d_lag = nullptr, *d_lag_state = nullptr;         // [T][nrows], [nrows]
    float *d_mag = nullptr, *d_frac = nullptr, *d_mag_state = nullptr, *d_frac_state = nullptr;
    float2 *d_phasor = nullptr, *d_phase_state[2] = {nullptr, nullptr}; // [T][nrows], 2 x [nrows]
    long long *d_corr = nullptr;       // [T][nrows][2]: integer sums (three-kernel path) or the fused kernel's two hand-over slots
    int chain_slot = 0;                // fused path: slot [chain_slot] of every entry carries this batch's unit phasors,
    int chain_armed[2] = {0, 0};       // the kernel re-arms the other one; leading blocks of each slot known to be all-ones
    unsigned int *d_sync = nullptr;    // fused K2: [0] ticket counter, [1] status; [2] bounded waits that ran out (two-row K1, two-line stage B, folded K1)
    unsigned int q_work_base = 0;      // value of the two-row K1's work counter (d_sync[3]) when the next launch starts
    bool k1_used = false;              // a launch with bounded waits is (or was) in flight: check [2] at the next sync
    unsigned k1_waits = 0;             // ... which kinds since the last status check (kWait*): what the error message names
    // carried state {lag, mag, frac}_state + phase_state[0..1] lives in ONE allocation (d_state) so that the first two-row
    // launch after a clean status check can snapshot it with one stream-ordered copy; a wait that ran out rolls the
    // plan back to that snapshot (check_fused_status) and keeps later launches on the packed kernel
    uint8_t *d_state = nullptr, *d_state_snap = nullptr;   // d_state_snap: kSnaps copies (the ring below)
    size_t state_bytes = 0;
    bool q_disabled = false;
    // Ring of stream-ordered snapshots of the carried state, one per batch that used a two-row / two-line kernel (entry = the
    // state BEFORE that batch).  A status word read clean behind batch k retires every snapshot older than the state before
    // batch k + 1; a wait that ran out rolls back to the OLDEST unretired one.  When the ring is full no new snapshot is
    // taken (the rollback then simply reaches further back).
    static constexpr int kSnaps = 8;
    struct Snap { unsigned long idx; int phase_cur; } snaps[kSnaps] = {};
    int snap_head = 0, snap_cnt = 0;
    unsigned long submit_idx = 0;          // batches submitted since create / reset / rollback
    unsigned long copy_idx[4] = {0, 0, 0, 0};   // submit index of the batch each outstanding asynchronous fetch belongs to
    bool fused_k2 = true;                      // CRSDR_K2_FUSED=0: the three-kernel phase path
    // B = 16384: the blocks' reference spectra as the first work items of the cross-correlation launch itself (CRSDR_K1_FOLD=0: from
    // k_ref_spectrum14p on the aux stream, two cross-stream dependencies and an event record per batch more)
    bool fold = true;
    unsigned int *d_refflag = nullptr, refgen = 0;     // [max_batch] words: the launch generation whose spectrum of block t is in place
    int phase_cur = 0;
    int last_nblocks = 0;
    // long-block path (B > 16384): B = N1 x 16384
    bool longblock = false;
    int log2n1 = 0;
    float2 *d_wc = nullptr, *d_wf = nullptr, *d_tw1 = nullptr, *d_Y = nullptr, *d_Yref = nullptr;
    lb::LongPartial *d_part = nullptr;
    int long_chunk = 1 << 30; // rows per pass of the long-block stages
    // fractional-delay correction (crsdr_plan_set_frac_apply; long blocks, digital mode)
    bool frac_apply = false, frac_override_on = false;
    float frac_gain = 1.0f;
    float *d_frac_override = nullptr;   // [nrows]
    uint32_t *d_k2tab = nullptr;        // [8192] frequency index k2 of every junction register pair of the row transforms
    bool frac_generic = false;          // CRSDR_FRAC_GENERIC=1: B = 16384 takes the generic fractional-delay kernel too (A/B, tests)
    float2 *d_Z = nullptr;              // second work area (set_frac_apply): the correlation pass's stage B writes here, so that the apply pass finds stage A's output still in d_Y
    float4 *d_rowspec = nullptr;        // [row_count][8192] the rows' responses G(k2) in the junction's order (k_ramp_rowspec); allocated by set_frac_apply
    // reference-noise canceller (crsdr_plan_set_refcancel; LDS-resident blocks, digital mode): everything below is allocated by the setter
    int cancel_taps = 0;                // 0: off
    float2 *d_cancel_coef = nullptr;    // [max_batch][nrows][9] g_j of the last batch, j ascending
    float *d_cancel_res = nullptr;      // [max_batch][nrows]
    int32_t *d_cancel_status = nullptr; // [max_batch][nrows]
    int32_t *d_cancel_gram = nullptr;   // [max_batch][90] the blocks' integer Gram sums
    rc::cd *d_cancel_chol = nullptr;    // [max_batch][45] their Cholesky factors
    int32_t *d_cancel_bstat = nullptr;  // [max_batch] 0 or STATUS_SINGULAR per block
    int cancel_idle = 0;                // leading blocks whose outputs hold the "pass did not run" values (status 2)
    // pinned staging ring for the small per-batch host arrays
    uint32_t *h_readcnt = nullptr;
    uint8_t *h_mask = nullptr;
    hipEvent_t ev_stage[kStageSlots] = {};
    bool stage_valid[kStageSlots] = {};
    int stage_slot = 0;
    bool submitted = false;
    // optional per-kernel event pairs (crsdr_plan_enable_profiling)
    int prof_slots = 0;
    uint32_t prof_mask = 0;              // bit k: kernel k gets an event pair; bit 31: whole-submit start/stop
    long prof_count = 0;                 // submits recorded since enable
    std::vector<hipEvent_t> prof_ev;     // [slot][kernel][begin,end]
    std::vector<unsigned char> prof_has; // [slot][kernel]
};

constexpr int kProfKernels = 4;

static hipEvent_t *prof_pair(crsdr_plan *p, int which)
{
    if (!p->prof_slots || !(p->prof_mask & (1u << which))) return nullptr;
    const int slot = (int)(p->prof_count % p->prof_slots);
    p->prof_has[(size_t)slot * kProfKernels + which] = 1;
    return &p->prof_ev[((size_t)slot * kProfKernels + which) * 2];
}

static int plan_init_state(crsdr_plan *p)
{
    const size_t n = (size_t)p->nrows, T = (size_t)p->max_batch;
    std::vector<float2> ph(n, make_float2(1.0f, 0.0f)); // src/csdrdevice.cc:39-40
    ph[0] = make_float2(0.0f, 0.0f);                     // pcorrection[0] is never written
    for (int i = 0; i < 2; ++i) HIP_TRY(hipMemcpy(p->d_phase_state[i], ph.data(), sizeof(float2) * n, hipMemcpyHostToDevice));
    for (size_t t = 0; t < T; ++t) HIP_TRY(hipMemcpy(p->d_phasor + t * n, ph.data(), sizeof(float2) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(p->d_lag, 0, sizeof(int32_t) * n * T * 2));
    HIP_TRY(hipMemset(p->d_mag, 0, sizeof(float) * n * T * 2));
    HIP_TRY(hipMemset(p->d_frac, 0, sizeof(float) * n * T * 2));
    HIP_TRY(hipMemset(p->d_lag_state, 0, sizeof(int32_t) * n));
    HIP_TRY(hipMemset(p->d_mag_state, 0, sizeof(float) * n));
    HIP_TRY(hipMemset(p->d_frac_state, 0, sizeof(float) * n));
    HIP_TRY(hipMemset(p->d_corr, 0xFF, sizeof(long long) * 4 * n * T));
    p->chain_armed[0] = p->chain_armed[1] = (int)T;
    p->phase_cur = 0;
    p->last_nblocks = 0;
    p->snap_cnt = 0; p->snap_head = 0;
    return CRSDR_OK;
}

// Which frequency k2 of the 16384-point row transform sits in which junction register?  Transform a one-hot line
// x[n] = delta[n - 1] with the reference-row form of the kernel (forward, conj, refspec layout): slot q then holds
// exp(+2 pi i k2 / 16384) twice over, and k2 is read off the angle.  Done once per long-block plan; the table must be a
// permutation of 0 .. 16383 or the plan is refused.
static int make_k2tab(crsdr_plan *p)
{
    const size_t N2 = lb::N2;
    float2 *line = p->d_Yref;              // long blocks have a line of their own; a 16384-point plan borrows one for this call
    if (!line) HIP_TRY(hipMalloc((void **)&line, sizeof(float2) * N2));
    const auto give_back = [&]() { if (line != p->d_Yref) (void)hipFree(line); };
    hipError_t e0 = hipMemset(line, 0, sizeof(float2) * N2);
    const float2 one = make_float2(1.0f, 0.0f);
    if (e0 == hipSuccess) e0 = hipMemcpy(line + 1, &one, sizeof(one), hipMemcpyHostToDevice);
    if (e0 == hipSuccess) e0 = hipDeviceSynchronize();       // the plan's streams are non-blocking: no implicit order with the null stream
    if (e0 == hipSuccess) e0 = launch_long_rows_ref1(p->own_stream, line, p->d_twA, p->d_twB, p->d_refspec[0]);
    if (e0 == hipSuccess) e0 = hipStreamSynchronize(p->own_stream);
    give_back();
    HIP_TRY(e0);
    std::vector<float2> h(N2);
    HIP_TRY(hipMemcpy(h.data(), p->d_refspec[0], sizeof(float2) * N2, hipMemcpyDeviceToHost));
    std::vector<uint32_t> tab(N2 / 2);
    std::vector<unsigned char> seen(N2, 0);
    for (size_t i = 0; i < N2; ++i) {
        const double rev = std::atan2((double)h[i].y, (double)h[i].x) / (2.0 * M_PI);      // conj(W^k2) = exp(+2 pi i k2 / N2)
        const long k2 = ((long)std::llround(rev * (double)N2) % (long)N2 + (long)N2) % (long)N2;
        const double mag = std::hypot((double)h[i].x, (double)h[i].y);
        if (std::fabs(mag - 1.0) > 1e-3 || seen[(size_t)k2]) return fail(CRSDR_EHIP, "plan_create: frequency map of the row transform is not a permutation (entry %zu)", i);
        seen[(size_t)k2] = 1;
        if (i & 1) tab[i >> 1] |= (uint32_t)k2 << 16; else tab[i >> 1] = (uint32_t)k2;
    }
    HIP_TRY(hipMalloc((void **)&p->d_k2tab, sizeof(uint32_t) * tab.size()));
    HIP_TRY(hipMemcpy(p->d_k2tab, tab.data(), sizeof(uint32_t) * tab.size(), hipMemcpyHostToDevice));
    return CRSDR_OK;
}

static int plan_alloc(crsdr_plan *p)
{
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&p->aux, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&p->cs, hipStreamNonBlocking));
    for (auto &e : p->ev_copydone) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(hipHostMalloc((void **)&p->h_k1flag, 4 * sizeof(int), hipHostMallocDefault));
    memset(p->h_k1flag, 0, 4 * sizeof(int));
    p->stream = p->own_stream;
    hipEvent_t *evs[] = {&p->ev_fork, &p->ev_ref[0], &p->ev_ref[1], &p->ev_k1done[0], &p->ev_k1done[1], &p->ev_k2done[0], &p->ev_k2done[1]};
    for (auto e : evs) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    for (int i = 0; i < kStageSlots; ++i) HIP_TRY(hipEventCreateWithFlags(&p->ev_stage[i], hipEventDisableTiming));
    HIP_TRY(hipEventCreate(&p->ev_start));
    HIP_TRY(hipEventCreate(&p->ev_stop));
    { int rc = make_twiddles(p->longblock ? lb::N2 : p->B, &p->d_tw); if (rc) return rc; }
    if (p->log2n == 14 || p->longblock) { int rc = make_twiddles14(&p->d_twA, &p->d_twB); if (rc) return rc; }
    if (p->longblock) {
        const size_t Bz = (size_t)p->B, n1 = Bz >> lb::LOG2N2;
        int rc;
        if ((rc = make_twiddle_table((double)Bz, Bz >> lb::FBITS, (size_t)1 << lb::FBITS, &p->d_wc))) return rc;
        if ((rc = make_twiddle_table((double)Bz, (size_t)1 << lb::FBITS, 1, &p->d_wf))) return rc;
        if ((rc = make_twiddle_table((double)n1, n1, 1, &p->d_tw1))) return rc;
        HIP_TRY(hipMalloc((void **)&p->d_Y, sizeof(float2) * Bz * (size_t)p->row_count));
        HIP_TRY(hipMalloc((void **)&p->d_Yref, sizeof(float2) * Bz));
        {
            const char *e = getenv("CRSDR_LONG_CHUNK_MB");
            // r01, cfg5 (21 x 2^21, 352 MB): 64 MB -4 %, 128 MB +1.5 %, 200 MB +4.7 % against unchunked.  With the r02 column stages
            // (register-first passes, persistent stage A) the launch boundaries weigh more than the cache residency of the work
            // area: 64 MB 1 952, 100 MB 2 061, 136 MB 2 197, 170 MB 2 257, 200 MB 2 370, 240 MB 2 326, one chunk 2 460 blocks/s.
            const long mb = e ? atol(e) : 400;
            if (mb > 0) p->long_chunk = (int)std::max<size_t>(1, ((size_t)mb << 20) / (sizeof(float2) * Bz));
        }
        HIP_TRY(hipMalloc((void **)&p->d_part, sizeof(lb::LongPartial) * (size_t)lb::ntiles(p->log2n1) * (size_t)p->row_count));
    }
    const size_t n = (size_t)p->nrows, T = (size_t)p->max_batch;
    const size_t rowbytes = n * (size_t)p->B;
    for (int i = 0; i < 2; ++i) HIP_TRY(hipMalloc((void **)&p->d_refspec[i], sizeof(float2) * (size_t)p->B * T));
    HIP_TRY(hipMalloc((void **)&p->d_rows, rowbytes * T));
    // own packets: pad the front so that the matrix (at +16+4N) starts 256-byte aligned; the
    // stride between the packets of a batch keeps that alignment
    const size_t pad = (256 - (p->matrix_off % 256)) % 256;
    p->own_packet_stride = (p->packet_bytes + 255) / 256 * 256;
    p->packet_stride = p->own_packet_stride;
    HIP_TRY(hipMalloc((void **)&p->d_packet_alloc, pad + p->own_packet_stride * T + 256));
    HIP_TRY(hipMemset(p->d_packet_alloc, 0, pad + p->own_packet_stride * T + 256));
    p->d_packet_own = reinterpret_cast<int8_t *>(p->d_packet_alloc + pad);
    p->d_packet = p->d_packet_own;
    HIP_TRY(hipMalloc((void **)&p->d_readcnt, sizeof(uint32_t) * n * T));
    HIP_TRY(hipMalloc((void **)&p->d_mask, n));
    HIP_TRY(hipMalloc((void **)&p->d_lag, sizeof(int32_t) * n * T * 2));   // two batches: K1 of batch b+1 runs beside the phase kernel of batch b
    HIP_TRY(hipMalloc((void **)&p->d_mag, sizeof(float) * n * T * 2));
    HIP_TRY(hipMalloc((void **)&p->d_frac, sizeof(float) * n * T * 2));
    HIP_TRY(hipMalloc((void **)&p->d_phasor, sizeof(float2) * n * T));
    HIP_TRY(hipMalloc((void **)&p->d_corr, sizeof(long long) * 4 * n * T));   // unit words, then chain values (k_align_fused)
    HIP_TRY(hipMalloc((void **)&p->d_sync, 64));
    HIP_TRY(hipMemset(p->d_sync, 0, 64));
    HIP_TRY(hipMalloc((void **)&p->d_refflag, sizeof(unsigned int) * T));
    HIP_TRY(hipMemset(p->d_refflag, 0, sizeof(unsigned int) * T));
    { const char *e = getenv("CRSDR_K1_FOLD"); if (e) p->fold = atoi(e) != 0; }
    { const char *e = getenv("CRSDR_K2_FUSED"); if (e) p->fused_k2 = atoi(e) != 0; }
    { const char *e = getenv("CRSDR_FRAC_GENERIC"); if (e) p->frac_generic = atoi(e) != 0; }
    {
        const size_t n8 = (n + 1) / 2 * 2;                   // keeps the float2 arrays 8-byte aligned
        p->state_bytes = n8 * (3 * 4 + 2 * 8);
        HIP_TRY(hipMalloc((void **)&p->d_state, p->state_bytes));
        HIP_TRY(hipMalloc((void **)&p->d_state_snap, p->state_bytes * crsdr_plan::kSnaps));
        p->d_phase_state[0] = reinterpret_cast<float2 *>(p->d_state);
        p->d_phase_state[1] = p->d_phase_state[0] + n8;
        p->d_lag_state = reinterpret_cast<int32_t *>(p->d_phase_state[1] + n8);
        p->d_mag_state = reinterpret_cast<float *>(p->d_lag_state + n8);
        p->d_frac_state = p->d_mag_state + n8;
    }
    HIP_TRY(hipHostMalloc((void **)&p->h_readcnt, sizeof(uint32_t) * n * T * kStageSlots, hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void **)&p->h_mask, n * kStageSlots, hipHostMallocDefault));
    if (p->longblock || p->log2n == 14) { int rc = make_k2tab(p); if (rc) return rc; }      // (short blocks: the fractional-delay pass on K1's network)
    HIP_TRY(hipMalloc((void **)&p->d_frac_override, sizeof(float) * (size_t)p->nrows));
    HIP_TRY(hipMemset(p->d_frac_override, 0, sizeof(float) * (size_t)p->nrows));
    return plan_init_state(p);
}

static void plan_free(crsdr_plan *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->own_stream) (void)hipStreamSynchronize(p->own_stream);
    if (p->aux) (void)hipStreamSynchronize(p->aux);
    if (p->cs) { (void)hipStreamSynchronize(p->cs); (void)hipStreamDestroy(p->cs); }
    for (auto e : p->ev_copydone) if (e) (void)hipEventDestroy(e);
    void *bufs[] = {p->d_cancel_coef, p->d_cancel_res, p->d_cancel_status, p->d_cancel_gram, p->d_cancel_chol, p->d_cancel_bstat, p->d_Z, p->d_rowspec, p->d_frac_override, p->d_k2tab, p->d_wc, p->d_wf, p->d_tw1, p->d_Y, p->d_Yref, p->d_part, p->d_tw, p->d_twA, p->d_twB, p->d_refspec[0], p->d_refspec[1], p->d_rows, p->d_packet_alloc, p->d_readcnt,
                    p->d_mask, p->d_lag, p->d_mag, p->d_frac, p->d_phasor, p->d_corr, p->d_sync, p->d_state, p->d_state_snap, p->d_refflag};
    for (void *b : bufs) if (b) (void)hipFree(b);
    if (p->h_k1flag) (void)hipHostFree(p->h_k1flag);
    if (p->h_readcnt) (void)hipHostFree(p->h_readcnt);
    if (p->h_mask) (void)hipHostFree(p->h_mask);
    hipEvent_t evs[] = {p->ev_fork, p->ev_ref[0], p->ev_ref[1], p->ev_k1done[0], p->ev_k1done[1], p->ev_k2done[0], p->ev_k2done[1], p->ev_start, p->ev_stop};
    for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < kStageSlots; ++i) if (p->ev_stage[i]) (void)hipEventDestroy(p->ev_stage[i]);
    for (hipEvent_t e : p->prof_ev) if (e) (void)hipEventDestroy(e);
    if (p->own_stream) (void)hipStreamDestroy(p->own_stream);
    if (p->aux) (void)hipStreamDestroy(p->aux);
    delete p;
}

extern "C" int crsdr_plan_create(crsdr_plan **plan, const crsdr_plan_desc *desc)
{
    if (!plan || !desc) return fail(CRSDR_EINVAL, "plan_create: NULL argument");
    *plan = nullptr;
    const int l2 = ilog2_exact(desc->blocksize);
    if (desc->nrows < 2) return fail(CRSDR_EINVAL, "plan_create: nrows = %d (need the ref row and >= 1 signal row)", desc->nrows);
    if (l2 < kMinLog2 || l2 > kMaxLog2Plan)
        return fail(CRSDR_EINVAL, "plan_create: blocksize = %d unsupported (power of two in [16, 4194304])", desc->blocksize);
    if (desc->mode != CRSDR_MODE_FAITHFUL && desc->mode != CRSDR_MODE_DIGITAL)
        return fail(CRSDR_EINVAL, "plan_create: mode = %d", desc->mode);
    const int rb = desc->row_begin ? desc->row_begin : 1;
    const int rc_rows = desc->row_count ? desc->row_count : desc->nrows - rb;
    if (rb < 1 || rc_rows < 1 || rb + rc_rows > desc->nrows)
        return fail(CRSDR_EINVAL, "plan_create: slab [%d,%d) outside signal rows [1,%d)", rb, rb + rc_rows, desc->nrows);
    const int mb = desc->max_batch ? desc->max_batch : 1;
    if (mb < 1 || mb > kMaxBatch) return fail(CRSDR_EINVAL, "plan_create: max_batch = %d (1..%d)", mb, kMaxBatch);
    if (l2 > kMaxLog2 && mb != 1) return fail(CRSDR_EINVAL, "plan_create: long blocks (blocksize > 16384) take max_batch = 1");
    { int rc = require_device(); if (rc) return rc; }
    int ndev = 0;
    (void)crsdr_device_count(&ndev);
    if (desc->device < 0 || desc->device >= ndev) return fail(CRSDR_ENODEV, "plan_create: device %d of %d", desc->device, ndev);

    crsdr_plan *p = new (std::nothrow) crsdr_plan();
    if (!p) return fail(CRSDR_ENOMEM, "plan_create: out of host memory");
    p->nrows = desc->nrows; p->B = desc->blocksize; p->L = p->B / 2; p->log2n = l2; p->mode = desc->mode;
    p->device = desc->device; p->row_begin = rb; p->row_count = rc_rows; p->max_batch = mb;
    p->longblock = l2 > kMaxLog2; p->log2n1 = p->longblock ? l2 - lb::LOG2N2 : 0;
    p->matrix_off = 16 + 4 * (size_t)p->nrows;
    p->packet_bytes = p->matrix_off + (size_t)p->nrows * (size_t)p->B;
    int rc = plan_alloc(p);
    if (rc) { plan_free(p); return rc; }
    *plan = p;
    return CRSDR_OK;
}

extern "C" int crsdr_plan_destroy(crsdr_plan *plan)
{
    if (!plan) return fail(CRSDR_EINVAL, "plan_destroy: NULL plan");
    plan_free(plan);
    return CRSDR_OK;
}

static int check_fused_status(crsdr_plan *p);
extern "C" int crsdr_plan_sync(crsdr_plan *p)
{
    if (!p) return fail(CRSDR_EINVAL, "plan_sync: NULL plan");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    HIP_TRY(hipStreamSynchronize(p->aux));
    HIP_TRY(hipStreamSynchronize(p->cs));
    p->copy_pending = false;
    p->copy_head = p->copy_tail;
    return check_fused_status(p);
}

extern "C" int crsdr_plan_reset(crsdr_plan *p)
{
    if (!p) return fail(CRSDR_EINVAL, "plan_reset: NULL plan");
    int rc = crsdr_plan_sync(p);
    if (rc) return rc;
    p->submitted = false;
    return plan_init_state(p);
}

extern "C" int crsdr_plan_set_stream(crsdr_plan *p, void *hip_stream)
{
    if (!p) return fail(CRSDR_EINVAL, "plan_set_stream: NULL plan");
    int rc = crsdr_plan_sync(p);
    if (rc) return rc;
    p->stream = hip_stream ? (hipStream_t)hip_stream : p->own_stream;
    return CRSDR_OK;
}

extern "C" size_t crsdr_plan_packet_bytes(const crsdr_plan *p) { return p ? p->packet_bytes : 0; }
extern "C" size_t crsdr_plan_matrix_offset(const crsdr_plan *p) { return p ? p->matrix_off : 0; }
extern "C" int crsdr_plan_bind_slab(crsdr_plan *p, void *device_slab, size_t slab_stride, int hdr_first, int hdr_count)
{
    if (!p) return fail(CRSDR_EINVAL, "plan_bind_slab: NULL plan");
    p->tail_offset = 0;
    if (!device_slab) { p->d_slab = nullptr; p->slab_stride = 0; p->hdr_first = p->hdr_count = 0; return CRSDR_OK; }
    if ((uintptr_t)device_slab % 4 || slab_stride % 4 || slab_stride < (size_t)p->row_count * (size_t)p->B || hdr_first < 0 || hdr_count < 0 ||
        hdr_first + hdr_count > p->max_batch)
        return fail(CRSDR_EINVAL, "plan_bind_slab: slab and stride 4-byte aligned, stride >= row_count*blocksize, header range inside the batch");
    p->d_slab = (int8_t *)device_slab; p->slab_stride = slab_stride; p->hdr_first = hdr_first; p->hdr_count = hdr_count;
    return CRSDR_OK;
}

extern "C" int crsdr_assemble_slabs(void *device_packets, size_t packet_stride, int nrows, int blocksize, const void *device_recv, int nsrc,
                                    int nblocks, void *hip_stream)
{
    if (!device_packets || !device_recv || nrows < 2 || blocksize < 16 || nsrc < 1 || nblocks < 1 || (nrows - 1) % nsrc)
        return fail(CRSDR_EINVAL, "assemble_slabs: need packets, recv, nsrc dividing the signal rows, nblocks >= 1");
    const size_t body_off = 16 + 4 * (size_t)nrows + (size_t)blocksize;          // row 1 of the matrix
    const size_t slab_bytes = (size_t)((nrows - 1) / nsrc) * (size_t)blocksize;
    if (((uintptr_t)device_packets + body_off) % 4 || packet_stride % 4 || (uintptr_t)device_recv % 4 ||
        (nblocks > 1 && packet_stride < body_off + (size_t)(nrows - 1) * blocksize) || nblocks > 65535 || nsrc > 65535)
        return fail(CRSDR_EINVAL, "assemble_slabs: 4-byte alignment of the matrix rows, stride >= packet bytes");
    { int rc_ = require_device(); if (rc_) return rc_; }
    hipStream_t s = (hipStream_t)hip_stream;
    const bool v16 = (((uintptr_t)device_packets + body_off) % 16 == 0) && (packet_stride % 16 == 0) && ((uintptr_t)device_recv % 16 == 0) && (slab_bytes % 16 == 0);
    const size_t words = slab_bytes / (v16 ? 16 : 4);
    const unsigned chunks = (unsigned)std::min<size_t>(std::max<size_t>(1, words / 1024), 64);
    if (v16) hipLaunchKernelGGL(k_assemble_slabs<uint4>, dim3(chunks, nblocks, nsrc), dim3(256), 0, s, (int8_t *)device_packets, packet_stride, body_off, (const uint4 *)device_recv, nblocks, words);
    else hipLaunchKernelGGL(k_assemble_slabs<uint32_t>, dim3(chunks, nblocks, nsrc), dim3(256), 0, s, (int8_t *)device_packets, packet_stride, body_off, (const uint32_t *)device_recv, nblocks, words);
    HIP_TRY(hipGetLastError());
    return CRSDR_OK;
}

extern "C" size_t crsdr_plan_packet_stride(const crsdr_plan *p) { return p ? p->packet_stride : 0; }

extern "C" int crsdr_plan_device_buffers(crsdr_plan *p, void **packet, void **lag, void **mag, void **frac, void **phasor)
{
    if (!p) return fail(CRSDR_EINVAL, "plan_device_buffers: NULL plan");
    if (packet) *packet = p->d_packet;
    const size_t ob = (size_t)p->obuf * (size_t)p->nrows * (size_t)p->max_batch;   // the buffers of the last submit
    if (lag) *lag = p->d_lag + ob;
    if (mag) *mag = p->d_mag + ob;
    if (frac) *frac = p->d_frac + ob;
    if (phasor) *phasor = p->d_phasor;
    return CRSDR_OK;
}

extern "C" int crsdr_plan_bind_packet(crsdr_plan *p, void *device_packet, size_t packet_stride)
{
    if (!p) return fail(CRSDR_EINVAL, "plan_bind_packet: NULL plan");
    if (device_packet && (((uintptr_t)device_packet + p->matrix_off) % 4 || packet_stride % 4 ||
                          (packet_stride < p->packet_bytes && p->max_batch > 1)))
        return fail(CRSDR_EINVAL, "plan_bind_packet: matrix start and stride must be 4-byte aligned, stride >= packet bytes");
    p->d_packet = device_packet ? (int8_t *)device_packet : p->d_packet_own;
    p->packet_stride = device_packet ? packet_stride : p->own_packet_stride;
    return CRSDR_OK;
}

extern "C" int crsdr_plan_set_frac_apply(crsdr_plan *p, int enable, float gain, const float *frac_override)
{
    if (!p) return fail(CRSDR_EINVAL, "plan_set_frac_apply: NULL plan");
    if (enable < 0 || enable > 2) return fail(CRSDR_EINVAL, "plan_set_frac_apply: enable = %d (0 off, 1 on, 2 on without the second work area)", enable);
    if (!enable) {
        // off: the two buffers this call allocated go back (a second cf32 work area is 8 * blocksize bytes per owned row)
        if (p->d_Z || p->d_rowspec) {
            int rc = crsdr_plan_sync(p);
            if (rc) return rc;
            if (p->d_Z) (void)hipFree(p->d_Z);
            if (p->d_rowspec) (void)hipFree(p->d_rowspec);
            p->d_Z = nullptr; p->d_rowspec = nullptr;
        }
        p->frac_apply = false;
        return CRSDR_OK;
    }
    if (p->mode != CRSDR_MODE_DIGITAL)
        return fail(CRSDR_EINVAL, "plan_set_frac_apply: needs a plan in CRSDR_MODE_DIGITAL (the faithful mode never shifts samples)");
    if (p->cancel_taps)
        return fail(CRSDR_ESTATE, "plan_set_frac_apply: the reference-noise canceller is on (crsdr_plan_set_refcancel): the correction re-reads the raw row, the two do not compose");
    // |D| is bounded: the response's phase k_s D / B is formed in fp32 (cis2pi), whose argument loses 6e-8 of its size per ulp --
    // at |D| <= 64 samples the phase stays within 1e-5 rad.  A proper peak's parabolic estimate is |frac| <= 1/2, so D = gain * frac
    // needs |gain| <= 128; caller-supplied delays beyond the bound belong in the integer lag (the resampler servo's business).
    if (!(gain == gain) || std::fabs(gain) > 128.0f) return fail(CRSDR_EINVAL, "plan_set_frac_apply: gain must be finite, |gain| <= 128");
    if (frac_override)
        for (int r = 1; r < p->nrows; ++r)
            if (!(std::fabs(frac_override[r]) <= 64.0f))
                return fail(CRSDR_EINVAL, "plan_set_frac_apply: frac_override[%d] = %g (need |D| <= 64 samples; larger delays belong in the integer lag)", r, (double)frac_override[r]);
    HIP_TRY(hipSetDevice(p->device));
    if (frac_override) {
        int rc = crsdr_plan_sync(p);
        if (rc) return rc;
        HIP_TRY(hipMemcpy(p->d_frac_override, frac_override, sizeof(float) * (size_t)p->nrows, hipMemcpyHostToDevice));
    }
    if (!p->longblock) {                   // LDS-resident blocks: one kernel behind the phase kernels, nothing to allocate
        p->frac_apply = true; p->frac_gain = gain; p->frac_override_on = frac_override != nullptr;
        return CRSDR_OK;
    }
    if (!p->d_rowspec) HIP_TRY(hipMalloc((void **)&p->d_rowspec, sizeof(float4) * 8192 * (size_t)p->row_count));
    if (enable == 2 && p->d_Z) {           // memory-lean form asked for: give the second work area back
        int rc = crsdr_plan_sync(p);
        if (rc) return rc;
        (void)hipFree(p->d_Z);
        p->d_Z = nullptr;
    }
    if (enable == 1 && !p->d_Z && hipMalloc((void **)&p->d_Z, sizeof(float2) * (size_t)p->B * (size_t)p->row_count) != hipSuccess) {
        p->d_Z = nullptr;                  // no room for a second work area: the apply pass repeats stage A instead (what enable = 2 asks for)
        (void)hipGetLastError();
    }
    p->frac_apply = true; p->frac_gain = gain; p->frac_override_on = frac_override != nullptr;
    return CRSDR_OK;
}

// Snapshot of the carried state before the batch now being submitted (at most one per batch; stream-ordered behind the previous
// batch's kernels).  The entry only counts once the copy has been accepted by the runtime.
static hipError_t take_snapshot(crsdr_plan *p, hipStream_t s)
{
    if (p->snap_cnt == crsdr_plan::kSnaps) return hipSuccess;                                   // full: the oldest stays the rollback point
    if (p->snap_cnt && p->snaps[(p->snap_head + p->snap_cnt - 1) % crsdr_plan::kSnaps].idx == p->submit_idx) return hipSuccess;
    const int pos = (p->snap_head + p->snap_cnt) % crsdr_plan::kSnaps;
    const hipError_t e = hipMemcpyAsync(p->d_state_snap + (size_t)pos * p->state_bytes, p->d_state, p->state_bytes, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
    p->snaps[pos].idx = p->submit_idx;
    p->snaps[pos].phase_cur = p->phase_cur;
    p->snap_cnt++;
    return hipSuccess;
}
// The status word was read clean behind batch k: every batch <= k is good, so a snapshot is obsolete as soon as a newer one
// that is still a state before some batch <= k + 1 exists; the last one goes too if nothing was submitted after batch k.
static void retire_snapshots(crsdr_plan *p, unsigned long k)
{
    while (p->snap_cnt >= 2 && p->snaps[(p->snap_head + 1) % crsdr_plan::kSnaps].idx <= k + 1) { p->snap_head = (p->snap_head + 1) % crsdr_plan::kSnaps; p->snap_cnt--; }
    if (p->snap_cnt == 1 && p->snaps[p->snap_head].idx <= k && p->submit_idx == k + 1) p->snap_cnt = 0;
}

// What one submit carries from stage to stage (crsdr_plan_submit_batch).
struct Batch {
    int nblocks;
    const int8_t *d_in;                // the batch's rows on the device: the caller's, or the plan's staging copy
    size_t d_stride;
    bool input_ready;                  // CRSDR_INPUT_READY on device rows: K0 need not wait for the main stream
    uint32_t xor80;
    const uint32_t *d_readcnt;
    const uint8_t *d_mask;
    bool any_lag;                      // the cross-correlation runs
    int32_t *o_lag;                    // this batch's {lag, mag, frac}
    float *o_mag, *o_frac;
    AlignArgs aa;                      // the phase kernels' arguments
    bool vec16;                        // 16-byte accesses
    int chunks;                        // long rows: 16 KiB of the row per workgroup
    bool fused;                        // the fused phase path
    bool cancel;                       // the reference-noise canceller writes this batch's rows (cancel_pass)
    bool kept_fwd;                     // long blocks: stage A's output survived the correlation pass (in d_Y; stage B wrote d_Z)
    bool corr_zeroed;                  // k_long_finalize zeroed the three-kernel path's integer sums
};

// Inputs: host rows to the plan's staging area, the small per-batch host arrays through the pinned ring, then the wait for a
// pipelined fetch and the profiling start.
static int stage_inputs(crsdr_plan *p, Batch &b, const void *rows, int mem_kind, size_t block_stride, const uint32_t *readcnt,
                        const uint8_t *lag_mask, uint32_t flags)
{
    hipStream_t S = p->stream;
    const size_t B = (size_t)p->B, n = (size_t)p->nrows, T = (size_t)b.nblocks;
    b.d_in = (const int8_t *)rows;
    b.d_stride = block_stride;
    b.input_ready = (flags & CRSDR_INPUT_READY) && mem_kind == CRSDR_MEM_DEVICE;
    b.xor80 = (flags & CRSDR_OFFSET_BINARY) ? 0x80808080u : 0u;
    if (mem_kind == CRSDR_MEM_HOST) {
        // reference row + this plan's slab only (cbuffer hand-off, src/crtlsdr.cc:173-203)
        for (size_t t = 0; t < T; ++t) {
            const int8_t *src = (const int8_t *)rows + t * block_stride;
            int8_t *dst = p->d_rows + t * n * B;
            HIP_TRY(hipMemcpyAsync(dst, src, B, hipMemcpyHostToDevice, S));
            HIP_TRY(hipMemcpyAsync(dst + B * (size_t)p->row_begin, src + B * (size_t)p->row_begin, B * (size_t)p->row_count,
                                   hipMemcpyHostToDevice, S));
        }
        b.d_in = p->d_rows;
        b.d_stride = n * B;
    }
    b.any_lag = !(flags & CRSDR_NO_LAG);
    if (readcnt || lag_mask) {
        const int ss = p->stage_slot;
        p->stage_slot = (ss + 1) % kStageSlots;
        if (p->stage_valid[ss]) HIP_TRY(hipEventSynchronize(p->ev_stage[ss]));
        if (readcnt) {
            uint32_t *h = p->h_readcnt + (size_t)ss * n * (size_t)p->max_batch;
            memcpy(h, readcnt, sizeof(uint32_t) * n * T);
            HIP_TRY(hipMemcpyAsync(p->d_readcnt, h, sizeof(uint32_t) * n * T, hipMemcpyHostToDevice, S));
            b.d_readcnt = p->d_readcnt;
        }
        if (lag_mask) {
            uint8_t *h = p->h_mask + (size_t)ss * n;
            memcpy(h, lag_mask, n);
            bool any = false;
            for (int r = p->row_begin; r < p->row_begin + p->row_count; ++r) any |= (h[r] != 0);
            b.any_lag = b.any_lag && any;
            HIP_TRY(hipMemcpyAsync(p->d_mask, h, n, hipMemcpyHostToDevice, S));
            b.d_mask = p->d_mask;
        }
        HIP_TRY(hipEventRecord(p->ev_stage[ss], S));
        p->stage_valid[ss] = true;
    }
    if (p->copy_pending) {
        // a pipelined fetch of the previous batch is (or was) in flight: this batch's kernels overwrite what it reads.  The
        // input copies above stay ahead of this wait, so they share the link with the device-to-host copies
        hipEvent_t newest = p->ev_copydone[(p->copy_tail - 1) % 4];
        HIP_TRY(hipStreamWaitEvent(S, newest, 0));
        p->copy_pending = false;
    }
    if (p->prof_slots) {
        const int ps = (int)(p->prof_count % p->prof_slots);
        for (int k = 0; k < kProfKernels; ++k) p->prof_has[(size_t)ps * kProfKernels + k] = 0;
        if (p->prof_mask & (1u << 31)) HIP_TRY(hipEventRecord(p->ev_start, S));
    }
    return CRSDR_OK;
}

// Outputs: this batch's {lag, mag, frac} buffer, the phase kernels' arguments and which phase path runs.
static void setup_outputs(crsdr_plan *p, Batch &b, uint32_t seq, uint32_t flags)
{
    const size_t n = (size_t)p->nrows;
    const int pin = p->phase_cur;
    const size_t ooff = (size_t)(p->obuf ^= 1) * n * (size_t)p->max_batch;      // this batch's {lag, mag, frac} buffer
    b.o_lag = p->d_lag + ooff;
    b.o_mag = p->d_mag + ooff;
    b.o_frac = p->d_frac + ooff;
    AlignArgs &aa = b.aa;
    aa.rows = b.d_in; aa.block_stride = b.d_stride; aa.packet = p->d_packet; aa.packet_stride = p->packet_stride;
    aa.readcnt = b.d_readcnt; aa.lag_mask = b.d_mask; aa.lag = b.o_lag; aa.lag_state = p->d_lag_state; aa.corr = p->d_corr;
    aa.phase_in = p->d_phase_state[pin]; aa.phase_out = p->d_phase_state[pin ^ 1]; aa.phasor = p->d_phasor;
    aa.nrows = p->nrows; aa.B = p->B; aa.row_begin = p->row_begin; aa.nblocks = b.nblocks;
    aa.digital = (p->mode == CRSDR_MODE_DIGITAL); aa.refnoise = (flags & CRSDR_REFNOISE_ENABLED) ? 1 : 0;
    aa.xcorr_ran = b.any_lag ? 1 : 0;
    aa.inline_chain = 0;
    // rows in and packet rows out are touched once: non-temporal (measured in the locked cadence, A/B in one call: stores +2.3 %, loads neutral)
    aa.nt = 3;
    aa.seq = seq; aa.xor80 = b.xor80;
    aa.slab = p->d_slab; aa.slab_stride = p->slab_stride; aa.hdr_first = p->hdr_first; aa.hdr_count = p->hdr_count;
    aa.lag_out = b.o_lag; aa.mag_out = b.o_mag; aa.frac_out = b.o_frac; aa.mag_state = p->d_mag_state; aa.frac_state = p->d_frac_state;
    // 16-byte accesses need 16-byte aligned rows and matrix rows (always true for the plan's own
    // buffers; a caller-bound packet or device input may only be 4-byte aligned -> word kernels)
    b.vec16 = ((uintptr_t)b.d_in % 16 == 0) && (b.d_stride % 16 == 0) && (((uintptr_t)p->d_packet + p->matrix_off) % 16 == 0) &&
              (p->packet_stride % 16 == 0 || b.nblocks == 1) &&
              (!p->d_slab || ((uintptr_t)p->d_slab % 16 == 0 && p->slab_stride % 16 == 0));
    b.chunks = p->B > 16384 ? p->B / 16384 : 1;
    b.cancel = p->cancel_taps && aa.refnoise && aa.digital;
    // (the canceller writes the owned rows itself, behind the three-kernel path's estimate)
    b.fused = p->fused_k2 && b.vec16 && b.chunks == 1 && !b.cancel;
}

// K0 on the aux stream into reference-spectrum slot `slot`, then the main stream's wait for it.  K0 goes behind the main
// stream's input copies (unless the caller's rows were complete before the submit) and behind the last K1 that read the slot.
template <typename LaunchK0>
static int run_k0(crsdr_plan *p, const Batch &b, int slot, LaunchK0 &&launch)
{
    hipStream_t S = p->stream, A = p->aux;
    if (!b.input_ready || b.d_readcnt || b.d_mask) {
        HIP_TRY(hipEventRecord(p->ev_fork, S)); // input copies, mask copy / the caller's producer work
        if (!b.input_ready) HIP_TRY(hipStreamWaitEvent(A, p->ev_fork, 0));
    }
    if (p->fold_last[slot]) {
        // a folded launch wrote and read refspec[slot] on the main stream after the last ev_k1done[slot] record (it records
        // none: see k1_short): the event goes behind it now, once per folded -> unfolded change of the slot
        HIP_TRY(hipEventRecord(p->ev_k1done[slot], S));
        p->k1done_valid[slot] = true;
        p->fold_last[slot] = false;
    }
    if (p->k1done_valid[slot]) HIP_TRY(hipStreamWaitEvent(A, p->ev_k1done[slot], 0)); // refspec[slot] free again
    hipEvent_t *pe0 = prof_pair(p, CRSDR_KERNEL_REF_SPECTRUM);
    if (pe0) HIP_TRY(hipEventRecord(pe0[0], A));
    { int rc = launch(A); if (rc) return rc; }
    if (pe0) HIP_TRY(hipEventRecord(pe0[1], A));
    HIP_TRY(hipEventRecord(p->ev_ref[slot], A));
    HIP_TRY(hipStreamWaitEvent(S, p->ev_ref[slot], 0));
    return CRSDR_OK;
}

// K1's arguments: this batch's rows against the reference spectra in refspec[slot], into this batch's {lag, mag, frac}
static XcorrArgs xcorr_args(const crsdr_plan *p, const Batch &b, int slot)
{
    XcorrArgs xa;
    xa.rows = b.d_in; xa.block_stride = b.d_stride; xa.refspec = p->d_refspec[slot]; xa.lag_mask = b.d_mask;
    xa.row_begin = p->row_begin; xa.nrows = p->nrows; xa.nblocks = b.nblocks; xa.xor80 = b.xor80;
    xa.stagger = 0;       // (x 512 cycles of head start for half the waves: measured r01, 0 is best for the packed kernels)
    xa.lag = b.o_lag; xa.mag = b.o_mag; xa.frac = b.o_frac;
    xa.lag_state = p->d_lag_state; xa.mag_state = p->d_mag_state; xa.frac_state = p->d_frac_state;
    return xa;
}

// Long blocks, stage B of `cnt` rows: two lines per CU (k_rows14_cf32q) once a launch has enough lines per CU; the packed one-line
// kernel otherwise (and always under CRSDR_LONG_Q=0 or CRSDR_K1_VARIANT=packed, or after a bounded wait of the two-line kernels ran out)
static bool two_line(const crsdr_plan *p, int cnt)
{
    const char kv = sw().k1_variant;
    return sw().long_q && (kv == 'a' || two_row(kv)) && !p->q_disabled && ((long)1 << p->log2n1) * cnt >= 1024;
}

// K1 of long blocks (B = N1 x 16384): column FFTs -> row FFTs (x conj ref, inverse) -> inverse column FFTs + argmax -> finalize
static int k1_long(crsdr_plan *p, Batch &b)
{
    hipStream_t S = p->stream;
    const lb::LongTw tw{p->d_wc, p->d_wf, p->d_tw1, p->d_tw, (uint32_t)(p->B - 1)};
    const int n1 = 1 << p->log2n1, l1 = p->log2n1;
    // The reference row's two stages (one row: 256 tiles, 128 lines -- they cannot fill the device) run on the aux stream
    // into the other spectrum slot, like K0 of the short blocks: with resident input they sit under the previous block's
    // stage C and phase kernels instead of in front of this block's stage A (21 us of 521 per cfg5 block).  The work line
    // d_Yref is only touched on the aux stream; a slot is rewritten after the last stage B that read it (ev_k1done).
    const int slot = (p->slot ^= 1);
    int rc = run_k0(p, b, slot, [&](hipStream_t A) -> int {
        HIP_TRY(CRSDR_DISPATCH_N1(l1, (launch_long_fwd_cols<LG, true>(A, 1, b.d_in, 0, b.xor80, tw, p->d_Yref))));
        HIP_TRY(launch_long_rows<true>(A, n1, 1, p->d_Yref, p->d_twA, p->d_twB, p->d_refspec[slot]));
        return CRSDR_OK;
    });
    if (rc) return rc;
    hipEvent_t *pe1 = prof_pair(p, CRSDR_KERNEL_XCORR_LAG);
    if (pe1) HIP_TRY(hipEventRecord(pe1[0], S));
    // with the fractional-delay pass to follow, stage B writes into the second work area: stage A's output stays in d_Y and
    // the apply pass does not repeat it (73 us of a 770 us cfg5 block) -- for the whole block or not at all (two-line kernel only)
    b.kept_fwd = p->d_Z && p->frac_apply && b.aa.digital;
    for (int r0 = 0; r0 < p->row_count; r0 += p->long_chunk) b.kept_fwd = b.kept_fwd && two_line(p, std::min(p->long_chunk, p->row_count - r0));
    // rows go through the three stages in chunks whose cf32 work area fits the 256 MB memory-side cache
    for (int r0 = 0; r0 < p->row_count; r0 += p->long_chunk) {
        const int cnt = std::min(p->long_chunk, p->row_count - r0);
        float2 *Yc = p->d_Y + (size_t)r0 * (size_t)p->B;
        float2 *Zc = b.kept_fwd ? p->d_Z + (size_t)r0 * (size_t)p->B : Yc;
        HIP_TRY(CRSDR_DISPATCH_N1(l1, (launch_long_fwd_cols<LG, false>(S, cnt, b.d_in, p->row_begin + r0, b.xor80, tw, Yc))));
        if (two_line(p, cnt)) {
            HIP_TRY(take_snapshot(p, S));              // same rollback protocol as the two-row K1 (check_fused_status)
            HIP_TRY(launch_long_rows_q(S, n1, cnt, Yc, p->d_twA, p->d_twB, p->d_refspec[slot], reinterpret_cast<int *>(p->d_sync + 2), nullptr,
                                       Zc != Yc ? Zc : nullptr));
            p->k1_used = true;
            p->k1_waits |= kWaitTwoLine;
        } else
            HIP_TRY(launch_long_rows<false>(S, n1, cnt, Yc, p->d_twA, p->d_twB, p->d_refspec[slot]));
        HIP_TRY(CRSDR_DISPATCH_N1(l1, (launch_long_inv_cols<LG>(S, cnt, Zc, tw, p->d_part + (size_t)r0 * lb::ntiles(l1), nullptr))));
    }
    HIP_TRY(hipEventRecord(p->ev_k1done[slot], S));       // the last reader of this block's reference spectrum has been enqueued
    p->k1done_valid[slot] = true;
    b.corr_zeroed = b.aa.refnoise && !b.fused && b.chunks > 1 && b.nblocks == 1;      // (the three-kernel path's integer sums: phase_three)
    hipLaunchKernelGGL(lb::k_long_finalize, dim3(p->row_count), dim3(256), 0, S, b.kept_fwd ? p->d_Z : p->d_Y, p->d_part, tw, n1, lb::ntiles(l1),
                       xcorr_args(p, b, slot), b.corr_zeroed ? p->d_corr : nullptr);
    HIP_TRY(hipGetLastError());
    if (pe1) HIP_TRY(hipEventRecord(pe1[1], S));
    return CRSDR_OK;
}

// K1 of LDS-resident blocks (B <= 16384)
static int k1_short(crsdr_plan *p, Batch &b)
{
    hipStream_t S = p->stream;
    const int slot = (p->slot ^= 1);
    const char variant = p->log2n == 14 ? k1_pick(p->row_count * b.nblocks, !p->q_disabled) : 0;
    // B = 16384: the reference spectra are the first work items of the cross-correlation launch itself (fold) -- one launch, no
    // second stream, no event between the launches of a batch.  r03, per-rank shape of the 8-GPU run (128 rows x 20 blocks,
    // 0.16 ms per batch): the kernel on the aux stream could only start when the previous batch's K1 let go of its CUs, and the
    // cross-stream wait + the event record between K1 and the phase kernel left 11 + 11 us of gaps around 138 us of kernels.
    // Folded where the launch is small (the packed kernel's launches: a GPU's share of an 8-GPU run, 0.16 ms per batch): K1 itself
    // grows by the reference items and its first rows' wait for them (0.118 -> 0.129 ms per 2560-row launch), the gaps around it
    // shrink by more (fenced 110 k -> 117 k blocks/s, back to back 122.9 k -> 124.6 k) and the host issues a batch in 10 us
    // instead of 26 - 40.  The two-row kernel's large launches keep the aux-stream kernel: there it hides completely, and the
    // folded form measured 0.910 -> 0.932 ms per 20-block launch of 1024 rows (every group's first row waits for block 0's item).
    const bool fold = p->fold && p->log2n == 14 && !p->q_disabled && variant == 'p';
    if (!fold) {
        // K0 on the aux stream: with resident input it overlaps the previous batch's K1 / K2.  (Putting it on the main stream
        // when both streams are idle -- a cold batch -- was measured in r02: exposed K0 0.0526 -> 0.0516 ms per cold batch and
        // no difference beyond the spread in a 20-block timed region; not kept.)
        int rc = run_k0(p, b, slot, [&](hipStream_t A) -> int {
            if (p->log2n == 14) HIP_TRY(launch_ref_spectrum14(A, b.nblocks, b.d_in, b.d_stride, p->d_twA, p->d_twB, p->d_refspec[slot], b.xor80));
            else HIP_TRY(CRSDR_DISPATCH_LOG2(p->log2n, (launch_ref_spectrum<LG>(A, b.nblocks, b.d_in, b.d_stride, p->d_tw, p->d_refspec[slot], b.xor80))));
            return CRSDR_OK;
        });
        if (rc) return rc;
    }
    XcorrArgs xa = xcorr_args(p, b, slot);
    if (fold) {
        static long folded = 0;                          // launches counted for CRSDR_K1_REFSPIN's "@k"
        xa.fold = 1; xa.refspec_w = p->d_refspec[slot]; xa.refflag = p->d_refflag; xa.refgen = ++p->refgen;
        xa.errflag = reinterpret_cast<int *>(p->d_sync + 2);
        xa.refspin = sw().refspin.at(folded++);
    }
    hipEvent_t *pe1 = prof_pair(p, CRSDR_KERNEL_XCORR_LAG);
    if (pe1) HIP_TRY(hipEventRecord(pe1[0], S));
    if (p->log2n == 14) {
        const bool q = two_row(variant);
        // every launch with bounded waits (the two-row kernel's, a folded launch's wait for its reference spectra) snapshots the
        // carried state first (one 28 B/row copy, ordered after the previous batch's kernels on this stream) while the ring has
        // room: what a wait that ran out is rolled back to
        if (q || fold) HIP_TRY(take_snapshot(p, S));
        HIP_TRY(launch_xcorr_lag14(S, variant, xa, p->row_count, p->d_twA, p->d_twB, reinterpret_cast<int *>(p->d_sync + 2), p->d_sync + 3, &p->q_work_base));
        p->k1_used |= q || fold;
        p->k1_waits |= (q ? kWaitTwoRow : 0u) | (fold ? kWaitFoldRef : 0u);
    } else
        HIP_TRY(CRSDR_DISPATCH_LOG2(p->log2n, (launch_xcorr_lag<LG>(S, xa, p->row_count, p->d_tw))));
    if (pe1) HIP_TRY(hipEventRecord(pe1[1], S));
    if (!fold) {                                     // (a folded launch's spectra are written and read on this stream only)
        HIP_TRY(hipEventRecord(p->ev_k1done[slot], S));
        p->k1done_valid[slot] = true;
    } else
        p->fold_last[slot] = true;                   // ... until an unfolded batch's K0 on the aux stream takes the slot over
    return CRSDR_OK;
}

// Both phase paths end with the fractional-delay pass (frac_pass, below).  The definitions from here on are in the order in which
// they first name their kernels (fused phase kernel, fractional-delay kernels, three-kernel path, long-block apply pass): that order
// is the order of the kernels in the code object.
static int frac_pass(crsdr_plan *p, const Batch &b);
static int cancel_pass(crsdr_plan *p, const Batch &b);      // the reference-noise canceller: section (v) at the end of this file

// Fused phase path: every row is read once (k_align_fused); timed under CRSDR_KERNEL_ALIGN_QUANT
static int phase_fused(crsdr_plan *p, const Batch &b)
{
    hipStream_t S = p->stream;
    const size_t n = (size_t)p->nrows;
    const int nblocks = b.nblocks;
    // hand-over words: two slots per (row, block).  A batch publishes into one and its workgroups re-arm the other
    // (all-ones) for the next batch, so the steady state needs no memset between launches; the host only tracks how
    // many leading blocks of each slot are armed and falls back to a memset when a batch needs more than that
    const int cs = p->chain_slot;
    unsigned long long *chain = reinterpret_cast<unsigned long long *>(p->d_corr);
    unsigned long long *chainv = chain + 2 * n * (size_t)p->max_batch;      // second half of d_corr: the chain values, same two slots
    const bool rn = b.aa.refnoise;
    FusedSync fs{p->d_sync, p->d_sync + 1, chain + cs, rn ? chain + (cs ^ 1) : nullptr, chainv + cs, rn ? chainv + (cs ^ 1) : nullptr,
                 p->row_count, sw().k2_spin};
    hipEvent_t *pe = prof_pair(p, CRSDR_KERNEL_ALIGN_QUANT);
    if (pe) HIP_TRY(hipEventRecord(pe[0], S));
    if (rn) {
        if (nblocks > 1 && p->chain_armed[cs] < nblocks) {
            HIP_TRY(hipMemsetAsync(p->d_corr, 0xFF, sizeof(long long) * 4 * n * (size_t)nblocks, S));
            p->chain_armed[0] = p->chain_armed[1] = nblocks;
        }
        p->chain_armed[cs] = 0;                                             // published into
        p->chain_armed[cs ^ 1] = std::max(p->chain_armed[cs ^ 1], nblocks); // re-armed by this launch
        p->chain_slot = cs ^ 1;
    }
    // (two rows per workgroup sharing the reference row's registers: built and measured in r03, 4.05 against 4.85 TB/s -- tools/k2_pair.hpp;
    //  persistent workgroups with the next item's row loads in flight: 3.1 - 3.6 against 4.76 TB/s -- tools/k2_persist.hpp)
    const dim3 grid((unsigned)((1 + p->row_count) * nblocks));
    if (p->B == 16384 && !b.xor80) hipLaunchKernelGGL((k_align_fused<true, false>), grid, dim3(kAlignThreads), 0, S, b.aa, fs);
    else if (p->B == 16384) hipLaunchKernelGGL((k_align_fused<true, true>), grid, dim3(kAlignThreads), 0, S, b.aa, fs);
    else hipLaunchKernelGGL((k_align_fused<false, true>), grid, dim3(kAlignThreads), 0, S, b.aa, fs);
    HIP_TRY(hipGetLastError());
    { int rc = frac_pass(p, b); if (rc) return rc; }
    { int rc = cancel_pass(p, b); if (rc) return rc; }
    if (pe) HIP_TRY(hipEventRecord(pe[1], S));
    return CRSDR_OK;
}

// fractional-delay correction of LDS-resident blocks: the owned rows once more, through the frequency domain
static int frac_short(crsdr_plan *p, const Batch &b)
{
    FracArgs fa{b.d_in, b.d_stride, p->d_packet, p->packet_stride, p->d_slab, p->slab_stride, p->nrows, p->row_begin, b.xor80, b.o_lag, b.o_frac,
                p->frac_override_on ? p->d_frac_override : nullptr, p->frac_gain, p->d_phasor};
    HIP_TRY(CRSDR_DISPATCH_LOG2(p->log2n, (launch_frac_apply<LG>(p->stream, p->row_count, b.nblocks, fa, p->d_tw, p->d_twA, p->d_twB,
                                                                 p->frac_generic ? nullptr : p->d_k2tab))));
    return CRSDR_OK;
}

// Three-kernel phase path (CRSDR_K2_FUSED=0, word-aligned rows, long rows): exact integer sums (k_phase_dot), the phasor chain
// (k_phase_chain), rotation and quantisation (k_align_quant)
static int phase_three(crsdr_plan *p, Batch &b)
{
    hipStream_t S = p->stream;
    const int nblocks = b.nblocks, chunks = b.chunks;
    AlignArgs &aa = b.aa;
    if (aa.refnoise) {
        hipEvent_t *pe = prof_pair(p, CRSDR_KERNEL_PHASE_DOT);
        if (pe) HIP_TRY(hipEventRecord(pe[0], S));
        p->chain_armed[0] = p->chain_armed[1] = 0;   // this path keeps its integer sums in d_corr
        if (chunks > 1 && !b.corr_zeroed)            // atomically accumulated (k_long_finalize has zeroed a tracked block's)
            HIP_TRY(hipMemsetAsync(p->d_corr, 0, sizeof(long long) * 2 * (size_t)p->nrows * (size_t)nblocks, S));
        // long rows: 32 KiB per workgroup with all 16 loads of a thread in flight at once (cfg5: 34 -> 30 us per block by the plan's events)
        if (b.vec16 && chunks >= 2) hipLaunchKernelGGL((k_phase_dot<true, 8>), dim3(p->row_count, nblocks, chunks / 2), dim3(kAlignThreads), 0, S, aa);
        else if (b.vec16) hipLaunchKernelGGL((k_phase_dot<true, 4>), dim3(p->row_count, nblocks, chunks), dim3(kAlignThreads), 0, S, aa);
        else hipLaunchKernelGGL((k_phase_dot<false, 4>), dim3(p->row_count, nblocks, chunks), dim3(kAlignThreads), 0, S, aa);
        HIP_TRY(hipGetLastError());
        if (pe) HIP_TRY(hipEventRecord(pe[1], S));
    }
    const bool apply = p->frac_apply && p->longblock && aa.digital;
    // long rows, one block per submit, rows rotated by k_align_quant itself: the single chain step is folded there
    aa.inline_chain = (chunks > 1 && nblocks == 1 && !apply) ? 1 : 0;
    if (!aa.inline_chain) {
        hipLaunchKernelGGL(k_phase_chain, dim3((p->row_count + 63) / 64), dim3(64), 0, S, aa, p->row_count);
        HIP_TRY(hipGetLastError());
    }
    hipEvent_t *pe = prof_pair(p, CRSDR_KERNEL_ALIGN_QUANT);
    if (pe) HIP_TRY(hipEventRecord(pe[0], S));
    // with the fractional-delay correction on, the rows come from the apply pass (frac_pass), with the reference-noise canceller from
    // cancel_pass: here only header + readcnt + row 0
    const unsigned gx = (apply || b.cancel) ? 1u : 1u + (unsigned)p->row_count;
    if (b.vec16) hipLaunchKernelGGL(k_align_quant<true>, dim3(gx, nblocks, chunks), dim3(kAlignThreads), 0, S, aa);
    else hipLaunchKernelGGL(k_align_quant<false>, dim3(gx, nblocks, chunks), dim3(kAlignThreads), 0, S, aa);
    HIP_TRY(hipGetLastError());
    { int rc = frac_pass(p, b); if (rc) return rc; }
    { int rc = cancel_pass(p, b); if (rc) return rc; }
    if (pe) HIP_TRY(hipEventRecord(pe[1], S));
    return CRSDR_OK;
}

// Fractional-delay correction (crsdr_plan_set_frac_apply, digital mode), behind the phase kernels and inside their
// CRSDR_KERNEL_ALIGN_QUANT event pair: frac_short for LDS-resident blocks; for long blocks the apply pass, int8 -> column FFTs
// -> row FFTs x H_row -> inverse -> inverse column FFTs -> int8.
static int frac_pass(crsdr_plan *p, const Batch &b)
{
    if (!p->frac_apply || !b.aa.digital) return CRSDR_OK;
    if (!p->longblock) return frac_short(p, b);
    hipStream_t S = p->stream;
    const float *frac_override = p->frac_override_on ? p->d_frac_override : nullptr;
    const lb::LongTw tw{p->d_wc, p->d_wf, p->d_tw1, p->d_tw, (uint32_t)(p->B - 1)};
    const int n1 = 1 << p->log2n1, l1 = p->log2n1;
    int8_t *obase = p->d_slab ? p->d_slab : p->d_packet + p->matrix_off + (size_t)p->row_begin * (size_t)p->B;
    for (int r0 = 0; r0 < p->row_count; r0 += p->long_chunk) {
        const int cnt = std::min(p->long_chunk, p->row_count - r0);
        float2 *Yc = p->d_Y + (size_t)r0 * (size_t)p->B;
        x14p::RampArgs ra{b.o_lag, b.o_frac, frac_override, p->d_phasor, p->d_k2tab, p->d_wc, p->d_wf, lb::FBITS, p->frac_gain, p->row_begin + r0, l1};
        if (!b.kept_fwd) HIP_TRY(CRSDR_DISPATCH_N1(l1, (launch_long_fwd_cols<LG, false>(S, cnt, b.d_in, p->row_begin + r0, b.xor80, tw, Yc))));
        // stage B'': the two-line kernel with the rows' responses as per-row spectra (k_ramp_rowspec + k_rows14_cf32q<true>), or
        // the one-line kernel that forms the response per bin
        if (two_line(p, cnt)) {
            hipLaunchKernelGGL(x14p::k_ramp_rowspec, dim3(8192 / 256, cnt), dim3(256), 0, S, p->d_rowspec + (size_t)r0 * 8192, ra);
            HIP_TRY(hipGetLastError());
            HIP_TRY(take_snapshot(p, S));          // (the same rollback protocol as the correlation pass)
            HIP_TRY(launch_long_rows_q(S, n1, cnt, Yc, p->d_twA, p->d_twB, reinterpret_cast<float2 *>(p->d_rowspec + (size_t)r0 * 8192),
                                       reinterpret_cast<int *>(p->d_sync + 2), &ra));
            p->k1_used = true;
            p->k1_waits |= kWaitTwoLine;
        } else
            HIP_TRY(launch_long_rows_ramp(S, n1, cnt, Yc, p->d_twA, p->d_twB, ra));
        HIP_TRY(CRSDR_DISPATCH_N1(l1, (launch_long_inv_cols<LG, true>(S, cnt, Yc, tw, nullptr, obase + (size_t)r0 * (size_t)p->B))));
    }
    return CRSDR_OK;
}

// End of a batch: the tails, the event a fetch waits for, the plan's bookkeeping
static int finish_batch(crsdr_plan *p, const Batch &b, uint32_t seq)
{
    hipStream_t S = p->stream;
    if (p->d_slab && p->tail_offset) {
        // slab mode with tails (crsdr_plan_bind_slab_ex): {lag, mag, frac, phasor} of the owned rows behind the rows of every slot
        hipLaunchKernelGGL(k_pack_tails, dim3((unsigned)((p->row_count + 255) / 256), (unsigned)b.nblocks), dim3(256), 0, S, p->d_slab, p->slab_stride,
                           p->tail_offset, p->row_begin, p->row_count, p->nrows, b.o_lag, b.o_mag, b.o_frac, p->d_phasor, b.d_readcnt, seq);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(p->ev_k2done[p->obuf], S));            // (p->obuf: this batch's buffer)
    p->phase_cur ^= 1;
    p->last_nblocks = b.nblocks;
    if (p->prof_slots) { if (p->prof_mask & (1u << 31)) HIP_TRY(hipEventRecord(p->ev_stop, S)); p->prof_count++; }
    p->submitted = true;
    p->submit_idx++;
    return CRSDR_OK;
}

extern "C" int crsdr_plan_submit_batch(crsdr_plan *p, const void *rows, int mem_kind, int nblocks, size_t block_stride,
                                       const uint32_t *readcnt, const uint8_t *lag_mask, uint32_t seq, uint32_t flags)
{
    if (!p || !rows) return fail(CRSDR_EINVAL, "plan_submit: NULL plan or rows");
    if (mem_kind != CRSDR_MEM_HOST && mem_kind != CRSDR_MEM_DEVICE) return fail(CRSDR_EINVAL, "plan_submit: mem_kind = %d", mem_kind);
    if (nblocks < 1 || nblocks > p->max_batch) return fail(CRSDR_EINVAL, "plan_submit: nblocks = %d (plan max_batch = %d)", nblocks, p->max_batch);
    const size_t block_bytes = (size_t)p->nrows * (size_t)p->B;
    if (block_stride == 0) block_stride = block_bytes;
    if (block_stride < block_bytes) return fail(CRSDR_EINVAL, "plan_submit: block_stride smaller than one block");
    if (mem_kind == CRSDR_MEM_DEVICE && ((uintptr_t)rows % 4 || block_stride % 4))
        return fail(CRSDR_EINVAL, "plan_submit: device rows and block_stride must be 4-byte aligned (16-byte for the vector kernels)");
    HIP_TRY(hipSetDevice(p->device));
    Batch b{};
    b.nblocks = nblocks;
    int rc = stage_inputs(p, b, rows, mem_kind, block_stride, readcnt, lag_mask, flags);
    if (rc) return rc;
    setup_outputs(p, b, seq, flags);
    // (K1 of batch b + 1 on its own stream beside the phase kernel of batch b was built and measured in r01 / r02 -- dead ends 5 and 10
    // of DESIGN.md: the kernels do overlap, and K1 stretches by exactly what the phase kernel costs alone -- and removed in r03.)
    if (b.any_lag && (rc = p->longblock ? k1_long(p, b) : k1_short(p, b))) return rc;
    if ((rc = b.fused ? phase_fused(p, b) : phase_three(p, b))) return rc;
    return finish_batch(p, b, seq);
}

extern "C" int crsdr_plan_submit(crsdr_plan *p, const void *rows, int mem_kind, const uint32_t *readcnt,
                                 const uint8_t *lag_mask, uint32_t seq, uint32_t flags)
{
    return crsdr_plan_submit_batch(p, rows, mem_kind, 1, 0, readcnt, lag_mask, seq, flags);
}

// (the fused phase kernel counts look-back waits it gave up on and computed locally -- d_sync[1] -- : nothing to report, results
// are exact either way)
static int check_fused_status(crsdr_plan *p)
{
    // the two-row K1 (xcorr14q.hpp) bounds its waits for the LDS image and its group barriers, the two-line stage B of long blocks
    // likewise, and the rows of a folded launch their wait for the block's reference spectrum (xcorr14p.hpp); one that runs out
    // means a scheduling assumption failed and the rows of that launch are not to be trusted: an error, never silent
    if (p->k1_used) {
        int w = 0;
        HIP_TRY(hipMemcpy(&w, p->d_sync + 2, sizeof(w), hipMemcpyDeviceToHost));
        if (w) {
            // Roll back: every batch submitted since the last clean check may have folded garbage lags into the carried
            // lag / mag / frac and EMA phase state.  Restore the snapshot taken before the first of them, re-arm the
            // phase kernel's hand-over words, and keep this plan on the packed kernel from here on -- the caller
            // resubmits those batches and gets what an undisturbed run would have given.
            (void)hipStreamSynchronize(p->stream); (void)hipStreamSynchronize(p->aux); (void)hipStreamSynchronize(p->cs);
            (void)hipMemset(p->d_sync, 0, 64);                    // flags and the work counter (its count is off after a failed launch)
            p->q_work_base = 0;
            unsigned long lost = 0;
            if (p->snap_cnt) {
                const crsdr_plan::Snap &sn = p->snaps[p->snap_head];      // the OLDEST unretired snapshot: the state before batch sn.idx
                (void)hipMemcpy(p->d_state, p->d_state_snap + (size_t)p->snap_head * p->state_bytes, p->state_bytes, hipMemcpyDeviceToDevice);
                p->phase_cur = sn.phase_cur;
                lost = p->submit_idx - sn.idx;
                p->submit_idx = sn.idx;
            }
            (void)hipMemset(p->d_corr, 0xFF, sizeof(long long) * 4 * (size_t)p->nrows * (size_t)p->max_batch);
            p->chain_armed[0] = p->chain_armed[1] = p->max_batch;
            p->snap_cnt = 0; p->snap_head = 0; p->k1_used = false; p->q_disabled = true; p->submitted = false;
            p->copy_pending = false; p->copy_head = p->copy_tail;       // outstanding asynchronous fetches delivered untrusted data: dropped
            // the status word is shared: name every kind of wait that was in flight since the last clean read
            const unsigned kinds = p->k1_waits;
            p->k1_waits = 0;
            const char *names[3] = {(kinds & kWaitTwoRow) ? "the two-row kernel's" : nullptr, (kinds & kWaitTwoLine) ? "the two-line stage B's" : nullptr,
                                    (kinds & kWaitFoldRef) ? "a folded launch's wait for its reference spectrum" : nullptr};
            std::string what;
            for (const char *nm : names)
                if (nm) what += (what.empty() ? "" : " or ") + std::string(nm);
            return fail(CRSDR_EHIP, "xcorr: %d workgroup(s) ran out of a bounded wait (%s); the last %lu submitted batch(es) -- everything "
                                    "since the last batch whose status was read clean -- were rolled back (carried lag and phase state restored): resubmit "
                                    "them; this plan now keeps to the one-row / one-line kernels, unfolded (CRSDR_K1_VARIANT=packed CRSDR_K1_FOLD=0 from the start)", w, what.empty() ? "unknown" : what.c_str(), lost);
        }
        p->snap_cnt = 0; p->snap_head = 0; p->k1_used = false; p->k1_waits = 0;  // clean and the streams are drained: the next bounded launch takes a fresh snapshot
    }
    return CRSDR_OK;
}

extern "C" int crsdr_plan_fetch_block(crsdr_plan *p, int block, int32_t *lag, float *mag, float *frac, float *phasor,
                                      int8_t *packet)
{
    if (!p) return fail(CRSDR_EINVAL, "plan_fetch: NULL plan");
    if (!p->submitted) return fail(CRSDR_ESTATE, "plan_fetch: nothing submitted");
    if (block < 0) block = p->last_nblocks - 1;
    if (block >= p->last_nblocks) return fail(CRSDR_EINVAL, "plan_fetch: block %d of a batch of %d", block, p->last_nblocks);
    if (packet && p->d_slab) return fail(CRSDR_ESTATE, "plan_fetch: slab output is bound, packets are assembled by the caller (crsdr_assemble_slabs)");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    { int rc_ = check_fused_status(p); if (rc_) return rc_; }
    const size_t n = (size_t)p->nrows, o = (size_t)block * n;
    const size_t ob = (size_t)p->obuf * n * (size_t)p->max_batch + o;
    if (lag) HIP_TRY(hipMemcpy(lag, p->d_lag + ob, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    if (mag) HIP_TRY(hipMemcpy(mag, p->d_mag + ob, sizeof(float) * n, hipMemcpyDeviceToHost));
    if (frac) HIP_TRY(hipMemcpy(frac, p->d_frac + ob, sizeof(float) * n, hipMemcpyDeviceToHost));
    if (phasor) HIP_TRY(hipMemcpy(phasor, p->d_phasor + o, sizeof(float2) * n, hipMemcpyDeviceToHost));
    if (packet) HIP_TRY(hipMemcpy(packet, p->d_packet + (size_t)block * p->packet_stride, p->packet_bytes, hipMemcpyDeviceToHost));
    return CRSDR_OK;
}

extern "C" int crsdr_plan_fetch_batch_async(crsdr_plan *p, int32_t *lag, float *mag, float *frac, float *phasor, int8_t *packets,
                                            size_t host_packet_stride)
{
    if (!p) return fail(CRSDR_EINVAL, "plan_fetch_batch_async: NULL plan");
    if (!p->submitted) return fail(CRSDR_ESTATE, "plan_fetch_batch_async: nothing submitted");
    if (packets && p->d_slab) return fail(CRSDR_ESTATE, "plan_fetch_batch_async: slab output is bound, packets are assembled by the caller");
    if (packets && host_packet_stride < p->packet_bytes) return fail(CRSDR_EINVAL, "plan_fetch_batch_async: host_packet_stride smaller than a packet");
    if (p->copy_tail - p->copy_head >= 4) return fail(CRSDR_ESTATE, "plan_fetch_batch_async: four fetches outstanding, call crsdr_plan_fetch_wait first");
    HIP_TRY(hipSetDevice(p->device));
    const size_t n = (size_t)p->nrows, T = (size_t)p->last_nblocks;
    const size_t ob = (size_t)p->obuf * n * (size_t)p->max_batch;
    HIP_TRY(hipStreamWaitEvent(p->cs, p->ev_k2done[p->obuf], 0));          // the batch's last kernel
    if (lag) HIP_TRY(hipMemcpyAsync(lag, p->d_lag + ob, sizeof(int32_t) * n * T, hipMemcpyDeviceToHost, p->cs));
    if (mag) HIP_TRY(hipMemcpyAsync(mag, p->d_mag + ob, sizeof(float) * n * T, hipMemcpyDeviceToHost, p->cs));
    if (frac) HIP_TRY(hipMemcpyAsync(frac, p->d_frac + ob, sizeof(float) * n * T, hipMemcpyDeviceToHost, p->cs));
    if (phasor) HIP_TRY(hipMemcpyAsync(phasor, p->d_phasor, sizeof(float2) * n * T, hipMemcpyDeviceToHost, p->cs));
    if (packets) {
        if (host_packet_stride == p->packet_stride)
            HIP_TRY(hipMemcpyAsync(packets, p->d_packet, p->packet_stride * (T - 1) + p->packet_bytes, hipMemcpyDeviceToHost, p->cs));
        else
            for (size_t t = 0; t < T; ++t)
                HIP_TRY(hipMemcpyAsync(packets + t * host_packet_stride, p->d_packet + t * p->packet_stride, p->packet_bytes, hipMemcpyDeviceToHost, p->cs));
    }
    // the two-row K1's error word rides along (a synchronous read in crsdr_plan_fetch_wait would wait for the whole device --
    // the next batch's upload included -- and serialise the two directions of the link: measured 25 + 25 instead of 45 GB/s)
    HIP_TRY(hipMemcpyAsync(&p->h_k1flag[p->copy_tail % 4], p->d_sync + 2, sizeof(int), hipMemcpyDeviceToHost, p->cs));
    HIP_TRY(hipEventRecord(p->ev_copydone[p->copy_tail % 4], p->cs));
    p->copy_idx[p->copy_tail % 4] = p->submit_idx - 1;                     // the batch these copies (and this status word) sit behind
    p->copy_tail++;
    p->copy_pending = true;
    return CRSDR_OK;
}

extern "C" int crsdr_plan_fetch_wait(crsdr_plan *p)
{
    if (!p) return fail(CRSDR_EINVAL, "plan_fetch_wait: NULL plan");
    HIP_TRY(hipSetDevice(p->device));
    if (p->copy_head == p->copy_tail) return fail(CRSDR_ESTATE, "plan_fetch_wait: no asynchronous fetch outstanding");
    HIP_TRY(hipEventSynchronize(p->ev_copydone[p->copy_head % 4]));      // the OLDEST outstanding fetch: later ones keep flying
    const int w = p->h_k1flag[p->copy_head % 4];                          // copied behind that batch's kernels: final for it
    const unsigned long k = p->copy_idx[p->copy_head % 4];
    p->copy_head++;
    if (w) return crsdr_plan_sync(p);                                      // drains everything, rolls back to the oldest unretired snapshot, reports
    retire_snapshots(p, k);                                                // batches <= k are good: the rollback point moves up behind them
    return CRSDR_OK;
}

extern "C" int crsdr_plan_fetch(crsdr_plan *p, int32_t *lag, float *mag, float *frac, float *phasor, int8_t *packet)
{
    return crsdr_plan_fetch_block(p, -1, lag, mag, frac, phasor, packet);
}

extern "C" int crsdr_plan_last_elapsed_ms(crsdr_plan *p, float *ms)
{
    if (!p || !ms) return fail(CRSDR_EINVAL, "plan_last_elapsed_ms: NULL argument");
    if (!p->submitted || !p->prof_slots || !(p->prof_mask & (1u << 31)))
        return fail(CRSDR_ESTATE, "plan_last_elapsed_ms: enable profiling with CRSDR_PROFILE_SUBMIT and submit first");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipEventSynchronize(p->ev_stop));
    HIP_TRY(hipEventElapsedTime(ms, p->ev_start, p->ev_stop));
    return CRSDR_OK;
}

extern "C" int crsdr_plan_enable_profiling(crsdr_plan *p, int slots, uint32_t kernel_mask)
{
    if (!p || slots < 0 || slots > 4096) return fail(CRSDR_EINVAL, "plan_enable_profiling: bad argument");
    int rc = crsdr_plan_sync(p);
    if (rc) return rc;
    for (hipEvent_t e : p->prof_ev) if (e) (void)hipEventDestroy(e);
    p->prof_ev.clear(); p->prof_has.clear();
    p->prof_slots = 0; p->prof_count = 0; p->prof_mask = kernel_mask;
    if (slots == 0) return CRSDR_OK;
    p->prof_ev.assign((size_t)slots * kProfKernels * 2, nullptr);
    p->prof_has.assign((size_t)slots * kProfKernels, 0);
    for (auto &e : p->prof_ev) HIP_TRY(hipEventCreate(&e));
    p->prof_slots = slots;
    return CRSDR_OK;
}

extern "C" int crsdr_plan_kernel_times(crsdr_plan *p, int which, float *ms, int capacity, int *count)
{
    if (!p || !ms || !count || which < 0 || which >= kProfKernels || capacity < 0) return fail(CRSDR_EINVAL, "plan_kernel_times: bad argument");
    *count = 0;
    if (!p->prof_slots) return fail(CRSDR_ESTATE, "plan_kernel_times: profiling not enabled");
    int rc = crsdr_plan_sync(p);
    if (rc) return rc;
    const long nrec = p->prof_count < p->prof_slots ? p->prof_count : p->prof_slots;
    const long first = p->prof_count - nrec;
    for (long i = first; i < p->prof_count && *count < capacity; ++i) {
        const int slot = (int)(i % p->prof_slots);
        if (!p->prof_has[(size_t)slot * kProfKernels + which]) continue;
        hipEvent_t *pe = &p->prof_ev[((size_t)slot * kProfKernels + which) * 2];
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, pe[0], pe[1]));
        ms[(*count)++] = t;
    }
    return CRSDR_OK;
}

// ================================================================================================
// (iv) batched direction-of-arrival engine (crsdr_doa)
// ================================================================================================
#include "doa_engine.hpp"

// ---- (iii) continued: the per-op calls on the engine's kernels (BEAMS_DISPATCH, SUBBAND_DISPATCH: doa_engine.hpp) ----
extern "C" int crsdr_subband_covariance(float *rbands, float *power, const int8_t *matrix, int nrows, int blocksize, int nfft, int first, int nbands, int width,
                                        int window, int mem_kind)
{
    if (!rbands || !matrix || nrows < 2 || nrows - 1 > subband::SB_MAX_ROWS || blocksize < 16)
        return fail(CRSDR_EINVAL, "subband_covariance: need rbands, matrix, 2 <= nrows <= %d, blocksize >= 16", subband::SB_MAX_ROWS + 1);
    { const int rc_ = subband_args_ok("subband_covariance", blocksize, nfft, first, nbands, width, window); if (rc_) return rc_; }
    OP_PROLOGUE_MEM("subband_covariance", mem_kind);
    const int m = nrows - 1, spb = subband::subband_spb(blocksize, nfft), lg = ilog2_exact(nfft);
    const size_t mb = (size_t)nrows * (size_t)blocksize, rb = sizeof(float2) * (size_t)nbands * m * m, pb = sizeof(float) * (size_t)nbands;
    OpStage st(mem_kind);
    const int8_t *d_m = (const int8_t *)st.in(0, matrix, mb, 4);
    float2 *d_r = (float2 *)st.out(1, rbands, rb, 8);
    float *d_p = (float *)st.out(2, power, pb, 4);
    if (st.rc) return st.rc;
    if (st.misaligned) return fail(CRSDR_EINVAL, "subband_covariance: device matrix and power 4-byte, rbands 8-byte aligned");
    if (st.spare(2, d_p, pb)) return st.rc;                           // (device memory and no power asked for: the reducer writes it all the same)
    OP_RESERVE(3, sizeof(float2) * (size_t)spb * subband::subband_partial(m, nfft));
    const dim3 grid((unsigned)spb, (unsigned)subband::subband_groups(m, nfft), 1);
    SUBBAND_DISPATCH(lg, hipLaunchKernelGGL(subband::k_doa_subband_cov<LG>, grid, dim3(subband::SB_THREADS), 0, 0, d_m, (size_t)0, (size_t)0, nrows, blocksize, 1, spb,
                                            window, (float2 *)g_op.buf[3]));
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(subband::k_doa_subband_reduce, dim3((unsigned)nbands, 1), dim3(256), 0, 0, (const float2 *)g_op.buf[3], spb, nrows, blocksize, 1, lg, first, width,
                       window, d_r, d_p);
    HIP_TRY(hipGetLastError());
    st.back(rbands, d_r, rb);
    st.back(power, d_p, pb);
    return st.finish();
}

// every instantiation the per-op call can launch may need more than 64 KiB of dynamic LDS
template <typename K>
static int sbb_lds_limit(K kern, const char *who)
{
    if (hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(sizeof(float2) * sbbeams::sbb_seg_stride(sbbeams::SBB_MAX_ROWS, 1 << subband::SB_MAX_LOG2))) != hipSuccess)
        return fail(CRSDR_EHIP, "%s: dynamic LDS limit of the band beam kernel", who);
    return CRSDR_OK;
}

extern "C" int crsdr_subband_beamform(float *out, const int8_t *matrix, int nrows, int blocksize, int nfft, int first, int nbands, int width, int window,
                                      const float *weights, int nbeams, int mem_kind)
{
    if (!out || !matrix || !weights || nrows < 2 || nrows - 1 > sbbeams::SBB_MAX_ROWS || blocksize < 16 || nbeams < 1 || nbeams > sbbeams::SBB_MAX_BEAMS)
        return fail(CRSDR_EINVAL, "subband_beamform: need out, matrix, weights, 2 <= nrows <= %d, blocksize >= 16, 1 <= nbeams <= %d", sbbeams::SBB_MAX_ROWS + 1,
                    sbbeams::SBB_MAX_BEAMS);
    { const int rc_ = subband_args_ok("subband_beamform", blocksize, nfft, first, nbands, width, window); if (rc_) return rc_; }
    OP_PROLOGUE_MEM("subband_beamform", mem_kind);
    const int m = nrows - 1, lg = ilog2_exact(nfft), J = blocksize / (2 * nfft), points = sbbeams::sbb_lds_points(m, blocksize, nfft);
    const size_t mb = (size_t)nrows * (size_t)blocksize, wb = sizeof(float2) * (size_t)nbands * nbeams * m;
    const size_t ob = sizeof(float2) * (size_t)nbands * nbeams * J * width;
    OpStage st(mem_kind);
    const int8_t *d_m = (const int8_t *)st.in(0, matrix, mb, 4);
    float2 *d_o = (float2 *)st.out(1, out, ob, 8);
    const float2 *d_w = (const float2 *)st.in(2, weights, wb, 8);
    if (st.rc) return st.rc;
    if (st.misaligned) return fail(CRSDR_EINVAL, "subband_beamform: device matrix 4-byte, weights and out 8-byte aligned");
    int rc = CRSDR_OK;
    SUBBAND_DISPATCH(lg, rc = sbb_lds_limit(sbbeams::k_subband_beamform<LG>, "subband_beamform"));
    if (rc) return rc;
    const dim3 grid((unsigned)sbbeams::sbb_spb(blocksize, nfft));
    SUBBAND_DISPATCH(lg, hipLaunchKernelGGL(sbbeams::k_subband_beamform<LG>, grid, dim3(sbbeams::SBB_THREADS), sizeof(float2) * (size_t)points, 0, d_m, nrows, blocksize,
                                            first, nbands, width, window, d_w, nbeams, points, d_o));
    HIP_TRY(hipGetLastError());
    st.back(out, d_o, ob);
    return st.finish();
}

extern "C" int crsdr_spectrum2d(float *pm, const float *vec, const float *sv, int m, int kind, float loading, float d, int mx, int my, int ncx, int ncy,
                                int mem_kind)
{
    if (!pm || !vec || !sv || m < 2 || m > music::MAX_M || mx < 1 || my < 1 || (long long)mx * my != m || ncx < 1 || ncy < 1 || (long long)ncx * ncy > (1 << 24))
        return fail(CRSDR_EINVAL, "spectrum2d: need pm, vec, sv, m = mx*my in [2, %d], grid <= 2^24 points", music::MAX_M);
    { const int rc_ = spectrum_args_ok("spectrum2d", kind, loading, false); if (rc_) return rc_; }
    OP_PROLOGUE_MEM("spectrum2d", mem_kind);
    const size_t mm = sizeof(float2) * (size_t)m * m, pb = sizeof(float) * (size_t)ncx * ncy;
    OpStage st(mem_kind);
    const float2 *d_v = (const float2 *)st.in(0, vec, mm, 8);
    float *d_p = (float *)st.out(1, pm, pb, 4);
    const float *d_s = (const float *)st.in(2, sv, sizeof(float) * (size_t)m, 4);
    if (st.rc) return st.rc;
    if (st.misaligned) return fail(CRSDR_EINVAL, "spectrum2d: device vec 8-byte, sv and pm 4-byte aligned");
    const size_t lds = spectrum::lds_bytes(m);           // 65 792 bytes at m = 64: above the default limit
    HIP_TRY(hipFuncSetAttribute((const void *)spectrum::k_spectrum2d, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned blocks = (unsigned)(((size_t)ncx * ncy + spectrum::PT - 1) / spectrum::PT);
    hipLaunchKernelGGL(spectrum::k_spectrum2d, dim3(blocks), dim3(spectrum::PT), lds, 0, d_v, d_s, m, kind, loading, d, mx, my, ncx, ncy, d_p);
    HIP_TRY(hipGetLastError());
    st.back(pm, d_p, pb);
    return st.finish();
}

extern "C" int crsdr_beamform(float *out, const int8_t *matrix, int nrows, int blocksize, const float *weights, int nbeams, int mem_kind)
{
    if (!out || !matrix || !weights || nrows < 2 || nrows - 1 > beams::MAX_M || blocksize < 32 || (blocksize % 32) || nbeams < 1 || nbeams > beams::MAX_BEAMS)
        return fail(CRSDR_EINVAL, "beamform: need out, matrix, weights, 2 <= nrows <= %d, blocksize %% 32 == 0, 1 <= nbeams <= %d", beams::MAX_M + 1,
                    beams::MAX_BEAMS);
    OP_PROLOGUE_MEM("beamform", mem_kind);
    const size_t mb = (size_t)nrows * (size_t)blocksize, wb = sizeof(float2) * (size_t)nbeams * (size_t)(nrows - 1);
    const size_t ob = sizeof(float2) * (size_t)nbeams * (size_t)(blocksize / 2);
    OpStage st(mem_kind);
    const int8_t *d_m = (const int8_t *)st.in(0, matrix, mb, 4);
    float2 *d_o = (float2 *)st.out(1, out, ob, 16);
    const float2 *d_w = (const float2 *)st.in(2, weights, wb, 8);
    if (st.rc) return st.rc;
    if (st.misaligned) return fail(CRSDR_EINVAL, "beamform: device matrix 4-byte, weights 8-byte, out 16-byte aligned");
    const dim3 grid((unsigned)((blocksize / 4 + beams::AP_THREADS - 1) / beams::AP_THREADS));
    BEAMS_DISPATCH(nbeams, hipLaunchKernelGGL(beams::k_beamform<NB>, grid, dim3(beams::AP_THREADS), 0, 0, d_m, nrows, blocksize, d_w, nbeams, d_o));
    HIP_TRY(hipGetLastError());
    st.back(out, d_o, ob);
    return st.finish();
}

#include "exchange_impl.hpp"

// ================================================================================================
// (iv) continued: the directions off the scan grid (refine.hpp).  The kernel's first use is here, behind every other kernel's: the
// code object's other kernels stay in the order they had (doa_engine.hpp)
// ================================================================================================
static const void *doa_refine_kernel() { return (const void *)refine::k_doa_refine<refine::RF_WAVES>; }

static void doa_refine_enqueue(dim3 grid, hipStream_t S, const float2 *vec, const float *sv, int M, int kind, int k, const int32_t *korder, float loading, float d, int Mx,
                               int Cx, int Cy, const int32_t *dirs, const int32_t *found, int levels, float *offsets, float *angles, float *values)
{
    hipLaunchKernelGGL(refine::k_doa_refine<refine::RF_WAVES>, grid, dim3(refine::RF_THREADS), refine::lds_bytes(M), S, vec, sv, M, kind, k, korder, loading, d, Mx, Cx, Cy,
                       dirs, found, levels, offsets, angles, values);
}

extern "C" int crsdr_refine2d(float *offsets, float *angles, float *values, const float *vec, const float *sv, int m, int kind, int k, float loading, float d, int mx,
                              int my, int ncx, int ncy, const int32_t *peaks, int npeaks, int levels, int mem_kind)
{
    if (!offsets || !angles || !values || !vec || !sv || !peaks || m < 2 || m > refine::MAX_M || mx < 1 || my < 1 || (long long)mx * my != m || ncx < 1 || ncy < 1 ||
        (long long)ncx * ncy > (1 << 24))
        return fail(CRSDR_EINVAL, "refine2d: need offsets, angles, values, vec, sv, peaks, m = mx*my in [2, %d], grid <= 2^24 points", refine::MAX_M);
    { const int rc_ = spectrum_args_ok("refine2d", kind, loading, true); if (rc_) return rc_; }
    if (kind == CRSDR_SPECTRUM_MUSIC && (k < 1 || k >= m)) return fail(CRSDR_EINVAL, "refine2d: k = %d sources (1 <= k < %d)", k, m);
    if (npeaks < 1 || npeaks > doa::MAX_PEAKS) return fail(CRSDR_EINVAL, "refine2d: npeaks = %d (1..%d)", npeaks, doa::MAX_PEAKS);
    if (levels < 1 || levels > refine::MAX_LEVELS) return fail(CRSDR_EINVAL, "refine2d: levels = %d (1..%d)", levels, refine::MAX_LEVELS);
    OP_PROLOGUE_MEM("refine2d", mem_kind);
    const size_t mm = sizeof(float2) * (size_t)m * m, n2 = sizeof(float) * 2 * (size_t)npeaks;
    OpStage st(mem_kind);
    const float2 *d_v = (const float2 *)st.in(0, vec, mm, 8);
    float *d_o = (float *)st.out(1, offsets, n2, 4);
    const float *d_s = (const float *)st.in(2, sv, sizeof(float) * (size_t)m, 4);
    float *d_a = (float *)st.out(3, angles, n2, 4);
    float *d_f = (float *)st.out(4, values, n2 / 2, 4);
    const int32_t *d_p = (const int32_t *)st.in(5, peaks, sizeof(int32_t) * 2 * (size_t)npeaks, 4);
    if (st.rc) return st.rc;
    if (st.misaligned) return fail(CRSDR_EINVAL, "refine2d: device vec 8-byte, every other pointer 4-byte aligned");
    // the engine's kernel: the limit doa_lds_limits() gives it, so that this call cannot lower it under a live object
    HIP_TRY(hipFuncSetAttribute(doa_refine_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)refine::lds_bytes(refine::MAX_M)));
    doa_refine_enqueue(dim3((unsigned)npeaks, 1), 0, d_v, d_s, m, kind, k, nullptr, kind == CRSDR_SPECTRUM_CAPON ? loading : 0.f, d, mx, ncx, ncy, d_p, nullptr, levels, d_o,
                       d_a, d_f);
    HIP_TRY(hipGetLastError());
    st.back(offsets, d_o, n2);
    st.back(angles, d_a, n2);
    st.back(values, d_f, n2 / 2);
    return st.finish();
}

// ================================================================================================
// (iv) continued: the gridless directions (esprit.hpp).  As above: the kernels' first use is here, behind every other kernel's
// ================================================================================================
static void doa_esprit_enqueue(unsigned nmat, hipStream_t S, const float2 *vec, const float *sv, int M, int k, const int32_t *korder, float d, int SX, int SY, int slots,
                               int32_t *found, int32_t *status, double *phases, float *angles, float *modulus, float *power, int32_t *flags)
{
    hipLaunchKernelGGL(esprit::k_doa_esprit<esprit::ES_WAVES>, dim3(nmat), dim3(esprit::ES_THREADS), 0, S, vec, sv, M, k, korder, d, SX, SY, slots, found, status, phases, angles, modulus,
                       power, flags);
}

extern "C" int crsdr_esprit2d(int32_t *found, int32_t *status, double *phases, float *angles, float *modulus, float *power, int32_t *flags, const float *vec,
                              const float *sv, int m, int k, float d, int mx, int my, int mem_kind)
{
    if (!found || !status || !phases || !angles || !modulus || !power || !flags || !vec || !sv)
        return fail(CRSDR_EINVAL, "esprit2d: need found, status, phases, angles, modulus, power, flags, vec, sv");
    if (mx < 2 || my < 2 || m > esprit::MAX_M || (long long)mx * my != m)
        return fail(CRSDR_EINVAL, "esprit2d: m = %d must be mx * my (%d x %d, each at least 2) and at most %d", m, mx, my, esprit::MAX_M);
    if (k < 1 || k > esprit_rank_limit(mx, my))
        return fail(CRSDR_EINVAL, "esprit2d: k = %d sources (1..%d: at most %d, and the rows a %d x %d array keeps when it drops a column or a row)", k,
                    esprit_rank_limit(mx, my), esprit::MAX_K, mx, my);
    OP_PROLOGUE_MEM("esprit2d", mem_kind);
    const size_t mm = sizeof(float2) * (size_t)m * m, n = (size_t)k;
    OpStage st(mem_kind);
    const float2 *d_v = (const float2 *)st.in(0, vec, mm, 8);
    const float *d_s = (const float *)st.in(1, sv, sizeof(float) * (size_t)m, 4);
    double *d_ph = (double *)st.out(2, phases, sizeof(double) * 2 * n, 8);
    float *d_an = (float *)st.out(3, angles, sizeof(float) * 2 * n, 4);
    float *d_mo = (float *)st.out(4, modulus, sizeof(float) * 2 * n, 4);
    float *d_pw = (float *)st.out(5, power, sizeof(float) * n, 4);
    int32_t *d_fl = (int32_t *)st.out(6, flags, sizeof(int32_t) * n, 4);
    int32_t *d_fo = (int32_t *)st.out(7, found, sizeof(int32_t), 4);
    int32_t *d_st = (int32_t *)st.out(8, status, sizeof(int32_t), 4);
    if (st.rc) return st.rc;
    if (st.misaligned) return fail(CRSDR_EINVAL, "esprit2d: device vec and phases 8-byte, every other pointer 4-byte aligned");
    hipLaunchKernelGGL(esprit::k_esprit2d<esprit::ES_WAVES>, dim3(1), dim3(esprit::ES_THREADS), 0, 0, d_v, d_s, m, k, d, mx, my, d_fo, d_st, d_ph, d_an, d_mo, d_pw, d_fl);
    HIP_TRY(hipGetLastError());
    st.back(phases, d_ph, sizeof(double) * 2 * n);
    st.back(angles, d_an, sizeof(float) * 2 * n);
    st.back(modulus, d_mo, sizeof(float) * 2 * n);
    st.back(power, d_pw, sizeof(float) * n);
    st.back(flags, d_fl, sizeof(int32_t) * n);
    st.back(found, d_fo, sizeof(int32_t));
    st.back(status, d_st, sizeof(int32_t));
    return st.finish();
}

// ================================================================================================
// (iv) continued: co-array augmentation (augment.hpp).  As above: the kernels are defined and first used here, behind every other
// kernel, so that the code object's other kernels stay where they were
// ================================================================================================
#include "augment.hpp"

static void doa_augment_enqueue(unsigned nmat, hipStream_t S, const float2 *rxx, int mx, int my, int vx, int vy, uint64_t mask, float2 *ra)
{
    hipLaunchKernelGGL(augment::k_doa_augment<augment::AG_THREADS>, dim3(nmat), dim3(augment::AG_THREADS), 0, S, rxx, mx, my, vx, vy, augment_mask(mx * my, mask), ra);
}

extern "C" int crsdr_augment_covariance(float *ra, const float *rxx, int mx, int my, int vx, int vy, uint64_t mask, int mem_kind)
{
    if (!ra || !rxx) return fail(CRSDR_EINVAL, "augment_covariance: need ra, rxx");
    { const int rc_ = augment_args_ok("augment_covariance", mx, my, vx, vy, mask); if (rc_) return rc_; }
    OP_PROLOGUE_MEM("augment_covariance", mem_kind);
    const size_t m = (size_t)mx * my, mv = (size_t)vx * vy, mm = sizeof(float2) * m * m, vb = sizeof(float2) * mv * mv;
    OpStage st(mem_kind);
    const float2 *d_r = (const float2 *)st.in(0, rxx, mm, 8);
    float2 *d_a = (float2 *)st.out(1, ra, vb, 8);
    if (st.rc) return st.rc;
    if (st.misaligned) return fail(CRSDR_EINVAL, "augment_covariance: device rxx and ra 8-byte aligned");
    hipLaunchKernelGGL(augment::k_augment_covariance<augment::AG_THREADS>, dim3(1), dim3(augment::AG_THREADS), 0, 0, d_r, mx, my, vx, vy, augment_mask((int)m, mask), d_a);
    HIP_TRY(hipGetLastError());
    st.back(ra, d_a, vb);
    return st.finish();
}

// ================================================================================================
// (v) reference-noise canceller (crsdr_plan_set_refcancel, crsdr_refcancel)
// ================================================================================================
// Its kernels are named here for the first time, behind everything else: the existing kernels keep their places in the code object.
#include "refcancel.hpp"

// Reference-noise canceller (crsdr_plan_set_refcancel), behind the three-kernel phase path and inside its CRSDR_KERNEL_ALIGN_QUANT
// event pair: the blocks' Gram sums and factors, the rows' sums and coefficients, the rows themselves (refcancel.hpp).  A batch
// submitted without CRSDR_REFNOISE_ENABLED keeps its phase path; its blocks' outputs are marked "did not run" once.
static rc::CancelArgs cancel_args(const crsdr_plan *p, const Batch &b)
{
    rc::CancelArgs ca{};
    ca.rows = b.d_in; ca.block_stride = b.d_stride;
    if (p->d_slab) { ca.orows = p->d_slab; ca.orows_stride = p->slab_stride; ca.orow_first = p->row_begin; }
    else { ca.orows = p->d_packet + p->matrix_off; ca.orows_stride = p->packet_stride; ca.orow_first = 0; }
    ca.lag = b.o_lag; ca.phasor = p->d_phasor;
    ca.coef = p->d_cancel_coef; ca.coef_pitch = rc::MAX_TAPS; ca.residual = p->d_cancel_res; ca.status = p->d_cancel_status;
    ca.gram = p->d_cancel_gram; ca.chol = p->d_cancel_chol; ca.block_status = p->d_cancel_bstat;
    ca.nrows = p->nrows; ca.B = p->B; ca.row_begin = p->row_begin; ca.taps = p->cancel_taps; ca.xor80 = b.xor80;
    return ca;
}

static int cancel_pass(crsdr_plan *p, const Batch &b)
{
    if (!p->cancel_taps) return CRSDR_OK;
    const rc::CancelArgs ca = cancel_args(p, b);
    if (!b.cancel) {
        if (p->cancel_idle >= b.nblocks) return CRSDR_OK;
        hipLaunchKernelGGL(rc::k_refcancel_idle, dim3((unsigned)((p->row_count + 255) / 256), (unsigned)b.nblocks), dim3(256), 0, p->stream, ca, p->row_count);
        HIP_TRY(hipGetLastError());
        p->cancel_idle = std::max(p->cancel_idle, b.nblocks);
        return CRSDR_OK;
    }
    p->cancel_idle = 0;
    // (the lags come from this batch's {lag, mag, frac} buffer: k_phase_chain has republished the carried ones for a batch without K1)
    HIP_TRY(rc::launch_refcancel(p->stream, ca, p->row_count, b.nblocks, b.vec16));
    return CRSDR_OK;
}

// ---- reference-noise canceller: setter, fetch, device buffers, the per-op form (kernels: refcancel.hpp; dispatch: cancel_pass) ----
static void cancel_free(crsdr_plan *p)
{
    void **bufs[] = {(void **)&p->d_cancel_coef, (void **)&p->d_cancel_res, (void **)&p->d_cancel_status, (void **)&p->d_cancel_gram, (void **)&p->d_cancel_chol,
                     (void **)&p->d_cancel_bstat};
    for (void **b : bufs) { if (*b) (void)hipFree(*b); *b = nullptr; }
    p->cancel_taps = 0; p->cancel_idle = 0;
}

static bool refcancel_taps_ok(int taps) { return taps >= 1 && taps <= rc::MAX_TAPS && (taps & 1); }

extern "C" int crsdr_plan_set_refcancel(crsdr_plan *p, int taps)
{
    if (!p) return fail(CRSDR_EINVAL, "plan_set_refcancel: NULL plan");
    if (taps != 0 && !refcancel_taps_ok(taps)) return fail(CRSDR_EINVAL, "plan_set_refcancel: taps = %d (0 off; 1, 3, 5, 7 or 9)", taps);
    if (taps == 0) {
        if (p->d_cancel_coef) {
            HIP_TRY(hipSetDevice(p->device));
            int rc = crsdr_plan_sync(p);
            if (rc) return rc;
            cancel_free(p);
        }
        p->cancel_taps = 0;
        return CRSDR_OK;
    }
    if (p->mode != CRSDR_MODE_DIGITAL)
        return fail(CRSDR_EINVAL, "plan_set_refcancel: needs a plan in CRSDR_MODE_DIGITAL (the canceller acts on the shifted row)");
    if (p->longblock) return fail(CRSDR_EINVAL, "plan_set_refcancel: blocksize = %d (the canceller takes blocks up to 16384)", p->B);
    if (p->frac_apply)
        return fail(CRSDR_ESTATE, "plan_set_refcancel: the fractional-delay correction is on (crsdr_plan_set_frac_apply): it re-reads the raw row, the two do not compose");
    HIP_TRY(hipSetDevice(p->device));
    { int rc = crsdr_plan_sync(p); if (rc) return rc; }
    const size_t n = (size_t)p->nrows, T = (size_t)p->max_batch;
    if (!p->d_cancel_coef) {
        const hipError_t e[] = {hipMalloc((void **)&p->d_cancel_coef, sizeof(float2) * rc::MAX_TAPS * n * T), hipMalloc((void **)&p->d_cancel_res, sizeof(float) * n * T),
                                hipMalloc((void **)&p->d_cancel_status, sizeof(int32_t) * n * T), hipMalloc((void **)&p->d_cancel_gram, sizeof(int32_t) * rc::GRAM_INTS * T),
                                hipMalloc((void **)&p->d_cancel_chol, sizeof(rc::cd) * rc::GRAM_PAIRS * T), hipMalloc((void **)&p->d_cancel_bstat, sizeof(int32_t) * T)};
        for (hipError_t x : e)
            if (x != hipSuccess) { cancel_free(p); (void)hipGetLastError(); return fail(CRSDR_ENOMEM, "plan_set_refcancel: %s", hipGetErrorString(x)); }
    }
    // rows outside the slab and row 0 hold zeros, and so do the coefficients beyond the tap count
    HIP_TRY(hipMemset(p->d_cancel_coef, 0, sizeof(float2) * rc::MAX_TAPS * n * T));
    HIP_TRY(hipMemset(p->d_cancel_res, 0, sizeof(float) * n * T));
    HIP_TRY(hipMemset(p->d_cancel_status, 0, sizeof(int32_t) * n * T));
    HIP_TRY(hipMemset(p->d_cancel_gram, 0, sizeof(int32_t) * rc::GRAM_INTS * T));
    HIP_TRY(hipMemset(p->d_cancel_chol, 0, sizeof(rc::cd) * rc::GRAM_PAIRS * T));
    HIP_TRY(hipMemset(p->d_cancel_bstat, 0, sizeof(int32_t) * T));
    HIP_TRY(hipDeviceSynchronize());        // the plan's streams are non-blocking: no implicit order with the null stream
    p->cancel_taps = taps; p->cancel_idle = 0;
    return CRSDR_OK;
}

static int check_fused_status(crsdr_plan *p);
extern "C" int crsdr_plan_fetch_refcancel(crsdr_plan *p, int block, float *coef, float *residual, int32_t *status)
{
    if (!p) return fail(CRSDR_EINVAL, "plan_fetch_refcancel: NULL plan");
    if (!p->cancel_taps) return fail(CRSDR_ESTATE, "plan_fetch_refcancel: the canceller is off (crsdr_plan_set_refcancel)");
    if (!p->submitted) return fail(CRSDR_ESTATE, "plan_fetch_refcancel: nothing submitted");
    if (block < 0) block = p->last_nblocks - 1;
    if (block >= p->last_nblocks) return fail(CRSDR_EINVAL, "plan_fetch_refcancel: block %d of a batch of %d", block, p->last_nblocks);
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    { int rc_ = check_fused_status(p); if (rc_) return rc_; }
    const size_t n = (size_t)p->nrows, o = (size_t)block * n;
    if (coef) {
        std::vector<float2> all(n * rc::MAX_TAPS);
        HIP_TRY(hipMemcpy(all.data(), p->d_cancel_coef + o * rc::MAX_TAPS, sizeof(float2) * all.size(), hipMemcpyDeviceToHost));
        for (size_t r = 0; r < n; ++r) memcpy(coef + 2 * r * (size_t)p->cancel_taps, &all[r * rc::MAX_TAPS], sizeof(float2) * (size_t)p->cancel_taps);
    }
    if (residual) HIP_TRY(hipMemcpy(residual, p->d_cancel_res + o, sizeof(float) * n, hipMemcpyDeviceToHost));
    if (status) HIP_TRY(hipMemcpy(status, p->d_cancel_status + o, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    return CRSDR_OK;
}

extern "C" int crsdr_plan_refcancel_buffers(crsdr_plan *p, void **coef, void **residual, void **status, int *taps)
{
    if (!p) return fail(CRSDR_EINVAL, "plan_refcancel_buffers: NULL plan");
    if (!p->cancel_taps) return fail(CRSDR_ESTATE, "plan_refcancel_buffers: the canceller is off (crsdr_plan_set_refcancel)");
    if (coef) *coef = p->d_cancel_coef;
    if (residual) *residual = p->d_cancel_res;
    if (status) *status = p->d_cancel_status;
    if (taps) *taps = p->cancel_taps;
    return CRSDR_OK;
}

extern "C" int crsdr_refcancel(int8_t *out, float *coef, float *residual, int32_t *status, const int8_t *rows, int nrows, int blocksize, const int32_t *lag,
                               const float *phasor, int taps, uint32_t flags, int mem_kind)
{
    if (!out || !coef || !residual || !status || !rows || !lag || !phasor || (const int8_t *)out == rows)
        return fail(CRSDR_EINVAL, "refcancel: need out, coef, residual, status, rows, lag and phasor (out apart from rows)");
    const int l2 = ilog2_exact(blocksize);
    if (nrows < 2 || l2 < kMinLog2 || l2 > kMaxLog2) return fail(CRSDR_EINVAL, "refcancel: nrows = %d, blocksize = %d (nrows >= 2, a power of two in [16, 16384])", nrows, blocksize);
    if (!refcancel_taps_ok(taps)) return fail(CRSDR_EINVAL, "refcancel: taps = %d (1, 3, 5, 7 or 9)", taps);
    if (flags & ~(uint32_t)CRSDR_OFFSET_BINARY) return fail(CRSDR_EINVAL, "refcancel: flags = 0x%x (CRSDR_OFFSET_BINARY or 0)", flags);
    const int L = blocksize / 2;
    if (mem_kind == CRSDR_MEM_HOST)
        for (int r = 1; r < nrows; ++r)
            if (lag[r] < -L || lag[r] > L) return fail(CRSDR_EINVAL, "refcancel: lag[%d] = %d (|lag| <= %d)", r, lag[r], L);
    if (mem_kind == CRSDR_MEM_DEVICE && ((uintptr_t)out % 4 || (uintptr_t)rows % 4 || (uintptr_t)coef % 8 || (uintptr_t)phasor % 8 || (uintptr_t)lag % 4 ||
                                         (uintptr_t)residual % 4 || (uintptr_t)status % 4))
        return fail(CRSDR_EINVAL, "refcancel: device rows and out 4-byte aligned (16-byte for the vector kernels), coef and phasor 8-byte");
    OP_PROLOGUE_MEM("refcancel", mem_kind);
    const size_t n = (size_t)nrows, mb = n * (size_t)blocksize;
    OpStage st(mem_kind);
    rc::CancelArgs ca{};
    ca.rows = (const int8_t *)st.in(0, rows, mb);
    ca.orows = (int8_t *)st.out(1, out, mb);
    ca.lag = (const int32_t *)st.in(2, lag, sizeof(int32_t) * n);
    ca.phasor = (const float2 *)st.in(3, phasor, sizeof(float2) * n);
    ca.coef = (float2 *)st.out(4, coef, sizeof(float2) * n * (size_t)taps);
    ca.residual = (float *)st.out(5, residual, sizeof(float) * n);
    ca.status = (int32_t *)st.out(6, status, sizeof(int32_t) * n);
    if (st.rc) return st.rc;
    OP_RESERVE(7, sizeof(int32_t) * rc::GRAM_INTS + sizeof(rc::cd) * rc::GRAM_PAIRS + 16);
    ca.chol = (rc::cd *)g_op.buf[7];
    ca.gram = (int32_t *)(ca.chol + rc::GRAM_PAIRS);
    ca.block_status = ca.gram + rc::GRAM_INTS;
    ca.block_stride = mb; ca.orows_stride = mb; ca.orow_first = 0; ca.coef_pitch = taps;
    ca.nrows = nrows; ca.B = blocksize; ca.row_begin = 1; ca.taps = taps; ca.xor80 = (flags & CRSDR_OFFSET_BINARY) ? 0x80808080u : 0u;
    // row 0 holds zeros in the three per-row outputs
    HIP_TRY(hipMemsetAsync(ca.coef, 0, sizeof(float2) * (size_t)taps, 0));
    HIP_TRY(hipMemsetAsync(ca.residual, 0, sizeof(float), 0));
    HIP_TRY(hipMemsetAsync(ca.status, 0, sizeof(int32_t), 0));
    hipLaunchKernelGGL(rc::k_refcancel_row0, grid1d((size_t)blocksize / 4), dim3(256), 0, 0, (uint32_t *)ca.orows, (const uint32_t *)ca.rows, blocksize / 4, ca.xor80);
    HIP_TRY(hipGetLastError());
    const bool vec = (uintptr_t)ca.rows % 16 == 0 && (uintptr_t)ca.orows % 16 == 0;
    HIP_TRY(rc::launch_refcancel(0, ca, nrows - 1, 1, vec));
    st.back(out, ca.orows, mb);
    st.back(coef, ca.coef, sizeof(float2) * n * (size_t)taps);
    st.back(residual, ca.residual, sizeof(float) * n);
    st.back(status, ca.status, sizeof(int32_t) * n);
    return st.finish();
}

// ================================================================================================
// (vi) Welch spectra and reference cross-spectra of the packets (crsdr_spectra, crsdr_welch)
// ================================================================================================
// Its kernels are named here for the first time, behind everything else: the existing kernels keep their places in the code object.
#include "spectra_engine.hpp"

// ================================================================================================
// (vii) Range-Doppler maps of the packets against a chosen row (crsdr_caf, crsdr_ambiguity)
// ================================================================================================
// Behind the spectra, for the same reason.
#include "caf_engine.hpp"
