/*
 * crsdr.h -- C ABI of the MI355X-native coherent-alignment engine (libcrsdr.so).
 *
 * Drop-in boundary for ONE path of mlaaks/coherent-rtlsdr: the ccoherent/cdsp DSP path
 * (int8 IQ -> complex float -> zero-padded FFT cross-correlation against the reference-noise
 * row -> argmax lag + magnitude -> phase estimate -> rotate (+shift) -> re-quantise into the
 * N x L receive matrix that cpacketize publishes).  Everything else of the reference (USB,
 * tuner control, console, ZMQ sockets) stays where it is.
 *
 * Two levels, mirroring the reference's own plug point (class cdsp is "wraps to volk kernels.
 * In future, these could be mapped to custom code", src/cdsp.cc:19; the RASPBERRYPI build
 * already swaps the FFT backend behind fft_scheme, include/cdsp.h:23-32):
 *   (i)  per-op entry points, one per cdsp static method   -> unit parity, drop-in for cdsp.cc
 *   (ii) a batched plan replacing ccoherent::{ctor,queuelag,computelag} plus the per-row
 *        csdrdevice::{convtofloat,est_phasecorrect,phasecorrect} and cpacketize::write chain
 *        (src/ccoherent.cc:245-294), because per-op launches would be launch-bound.
 *
 * Conventions (reference units): blocksize B = int8 values per row per block = FFT length in
 * complex points; L = B/2 complex samples per row; row 0 = reference-noise channel.
 * Complex arrays are interleaved float (re,im) -- layout-identical to std::complex<float>,
 * fftwf_complex and lv_32fc_t (src/ccoherent.cc:65).
 * Every function returns 0 on success or a negative CRSDR_E* code; nothing throws across the
 * ABI; crsdr_last_error() gives the text for the calling thread's last failure.
 * There is NO CPU fallback: without a usable HIP device every compute entry point fails with
 * CRSDR_ENODEV.
 */
#ifndef CRSDR_H
#define CRSDR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRSDR_ABI_VERSION 1

enum {
    CRSDR_OK = 0,
    CRSDR_EINVAL = -1,  /* bad argument (NULL, non power-of-two size, out of range) */
    CRSDR_ENOMEM = -2,  /* host or device allocation failed */
    CRSDR_EHIP = -3,    /* a HIP runtime call or kernel launch failed */
    CRSDR_ENODEV = -4,  /* no HIP device available */
    CRSDR_ESTATE = -5   /* call sequence error (fetch before submit, ...) */
};

int crsdr_abi_version(void);
const char *crsdr_last_error(void);
int crsdr_device_count(int *count);
/* Page-locked host memory for the rows / packet buffers handed to crsdr_plan_submit / crsdr_plan_fetch with
 * CRSDR_MEM_HOST -- the role volk_malloc / fftwf_alloc_complex play in the reference (src/ccoherent.cc:44-47,
 * 66-69: aligned allocations owned by the engine).  Pageable memory works too, at roughly half the PCIe rate
 * and with host-blocking copies. */
int crsdr_host_alloc(void **ptr, size_t bytes);
int crsdr_host_free(void *ptr);

/* Name, compute units, engine / memory clocks (kHz) and memory size of a device, for benchmark records
 * ("GPU clocks recorded").  Any output pointer may be NULL; name is NUL-terminated in name_cap bytes. */
int crsdr_device_info(int device, char *name, int name_cap, int *compute_units, int *clock_khz, int *memory_clock_khz,
                      size_t *memory_bytes);

/* ------------------------------------------------------------------------------------------
 * (i) per-op entry points == class cdsp (include/cdsp.h:36-71).  Host pointers in and out;
 *     each call stages through device memory on the current device (default stream) and
 *     returns when the result is in `out`.  Note the reference's mixed units for n.
 * ---------------------------------------------------------------------------------------- */

/* cdsp::convtosigned(const uint8_t*,const uint8_t*,int)  include/cdsp.h:40, src/cdsp.cc:21-34
 * out[i] = in[i] ^ 0x80, n bytes (n % 8 == 0 like the reference's 64-bit loop). */
int crsdr_convtosigned(const uint8_t *in, uint8_t *out, int n);

/* cdsp::convtofloat(const float*,const int8_t*,int) and the complex overload
 * include/cdsp.h:41,45, src/cdsp.cc:36-44.  n = number of int8 values (= floats written). */
int crsdr_convtofloat(float *out, const int8_t *s8bit, int n);

/* cdsp::scalarmul  include/cdsp.h:47, src/cdsp.cc:46-49.  n = complex count. */
int crsdr_scalarmul(float *out, const float *in, float scalar_re, float scalar_im, int n);

/* cdsp::convto8bit  include/cdsp.h:43, src/cdsp.cc:51-54.  n = complex count (2n bytes out). */
int crsdr_convto8bit(int8_t *out, const float *in, int n);

/* cdsp::conj_dotproduct  include/cdsp.h:49, src/cdsp.cc:61-66.  res[0..1] = sum a*conj(b). */
int crsdr_conj_dotproduct(float *res, const float *a, const float *b, int n);

/* cdsp::magsquared  include/cdsp.h:61, src/cdsp.cc:100-103.  n = complex count. */
int crsdr_magsquared(float *out, const float *in, int n);

/* cdsp::conjugatemul  include/cdsp.h:63, src/cdsp.cc:105-108.  out = in1 * conj(in2). */
int crsdr_conjugatemul(float *out, const float *in1, const float *in2, int n);

/* cdsp::indexofmax(float*,int)  include/cdsp.h:68, src/cdsp.cc:135-139: first strict maximum. */
int crsdr_indexofmax(uint32_t *index, const float *in, int n);

/* cdsp::fft(out,in,fft_scheme*)  include/cdsp.h:65, src/cdsp.cc:110-120, with the plan geometry
 * of src/ccoherent.cc:78-93 passed explicitly instead of an fftwf_plan: `howmany` contiguous
 * transforms of n complex points (dist n, stride 1), sign -1 = FFTW_FORWARD, +1 =
 * FFTW_BACKWARD, unnormalised, out of place.  n: power of two, 16 <= n <= 16384 (one
 * LDS-resident transform per workgroup; longer transforms exist only inside the plan, where the
 * four-step order never has to be undone). */
int crsdr_fft(float *out, const float *in, int n, int sign, int howmany);

/* ------------------------------------------------------------------------------------------
 * (ii) batched plan == ccoherent + per-row csdrdevice DSP members + cpacketize::write
 * ---------------------------------------------------------------------------------------- */

enum {
    CRSDR_MODE_FAITHFUL = 0, /* reference order of operations: lag reported, samples not
                                shifted (the lag feeds the resampler servo, src/ccontrol.cc:93-119),
                                phase estimated at zero offset */
    CRSDR_MODE_DIGITAL = 1   /* north_star "rotate/shift": row k is shifted by its lag, the
                                phase is estimated over the overlap, then rotate + quantise */
};

enum {
    CRSDR_MEM_HOST = 0,   /* pointer is host memory: the plan copies H2D / D2H */
    CRSDR_MEM_DEVICE = 1  /* pointer is device memory on the plan's device */
};

/* crsdr_plan_submit flags */
enum {
    CRSDR_REFNOISE_ENABLED = 1u << 0, /* crefnoise::isenabled(), gate of src/ccoherent.cc:271 */
    CRSDR_OFFSET_BINARY = 1u << 1,    /* input is librtlsdr's raw uint8: fuse cdsp::convtosigned
                                         (x ^ 0x80, include/common.h:114-122) into the loads */
    CRSDR_INPUT_READY = 1u << 2,      /* device input is already complete: the reference-spectrum
                                         kernel need not wait for earlier work on the stream */
    CRSDR_NO_LAG = 1u << 3            /* no row requests a lag this block ("locked" steady state,
                                         src/ccontrol.cc:117-120): phase path only, no FFT */
};

typedef struct crsdr_plan crsdr_plan;

typedef struct crsdr_plan_desc {
    int32_t nrows;      /* N: reference row + signal rows in the receive matrix (hdr0::N) */
    int32_t blocksize;  /* B: int8 values per row per block; power of two, 16..4194304.  B <= 16384:
                           one LDS-resident transform per row; B > 16384 (config 5: 2^21): four-step
                           B = (B/16384) x 16384 transform streamed through HBM, max_batch = 1 */
    int32_t mode;       /* CRSDR_MODE_* */
    int32_t device;     /* HIP device ordinal */
    int32_t row_begin;  /* first signal row this plan owns (>= 1); 0 = default (1) */
    int32_t row_count;  /* signal rows owned; 0 = default (all: nrows - row_begin).  Multi-GPU:
                           rank g owns a contiguous slab, the ref row is replicated */
    int32_t max_batch;  /* most consecutive blocks one crsdr_plan_submit_batch may carry (1..64);
                           0 = default (1).  Sizes every per-block device buffer. */
    uint32_t reserved;
} crsdr_plan_desc;

/* ccoherent::ccoherent (src/ccoherent.cc:32-95): allocates every device buffer, twiddle table,
 * stream and event; nothing is allocated on the per-block path afterwards. */
int crsdr_plan_create(crsdr_plan **plan, const crsdr_plan_desc *desc);
/* ccoherent::~ccoherent (src/ccoherent.cc:97-112) */
int crsdr_plan_destroy(crsdr_plan *plan);
/* back to construction state: phasecorr = phasecorrprev = 1+0j, lag = 0 (src/csdrdevice.cc:36-40) */
int crsdr_plan_reset(crsdr_plan *plan);

/* Run the plan's kernels on a caller-owned hipStream_t (e.g. the stream an RCCL gather is
 * enqueued on); NULL restores the plan's own stream. */
int crsdr_plan_set_stream(crsdr_plan *plan, void *hip_stream);

/* One ccoherent::threadf iteration (src/ccoherent.cc:245-294), asynchronous.
 *   rows      [nrows][B] int8 (uint8 with CRSDR_OFFSET_BINARY), row 0 = reference; a plan that
 *             owns a slab reads only row 0 and its own rows.
 *   mem_kind  CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE (read in place; must stay valid
 *             until the next fetch/sync).
 *   readcnt   [nrows] host array copied into the packet (cpacketize::write, src/cpacketizer.cc:
 *             142,163), or NULL: every row gets `seq`.
 *   lag_mask  [nrows] host bytes, non-zero = csdrdevice::is_lagrequested() (src/ccoherent.cc:266);
 *             NULL = every owned signal row.  Unlike the reference there is no nfft = 8 cap
 *             (src/ccoherent.cc:124): every requested row is cross-correlated in this block.
 *   seq       hdr0::globalseqn for this block (src/cpacketizer.cc:113). */
int crsdr_plan_submit(crsdr_plan *plan, const void *rows, int mem_kind, const uint32_t *readcnt,
                      const uint8_t *lag_mask, uint32_t seq, uint32_t flags);

/* nblocks consecutive ccoherent::threadf iterations in one submit: the same results as nblocks
 * crsdr_plan_submit calls in a row (the EMA phasor and the last lag are carried from block to
 * block), but every kernel is launched once over nblocks x rows workgroups -- host cost and
 * launch gaps are paid per batch, and a GPU that owns a small slab still fills its 256 CUs.
 *   rows          block t at rows + t * block_stride (bytes; 0 = nrows * B, i.e. contiguous)
 *   readcnt       [nblocks][nrows] or NULL (block t gets seq + t)
 *   lag_mask      [nrows], applies to every block of the batch
 *   seq           hdr0::globalseqn of block 0; block t gets seq + t
 * Packets land at device_packet + t * packet_stride. */
int crsdr_plan_submit_batch(crsdr_plan *plan, const void *rows, int mem_kind, int nblocks, size_t block_stride,
                            const uint32_t *readcnt, const uint8_t *lag_mask, uint32_t seq, uint32_t flags);

/* Wait for the last submitted block and copy results to host arrays (any may be NULL):
 *   lag    [nrows] int32  idx - L, what csdrdevice::set_lag receives (src/ccoherent.cc:232)
 *   mag    [nrows] float  sqrt(peak / L)                         (src/ccoherent.cc:204)
 *   frac   [nrows] float  3-point parabolic peak offset in samples (extra output; the reference
 *                         computes and discards its own variant, src/ccoherent.cc:206-219)
 *   phasor [nrows][2]     csdrdevice::get_phasecorrect() -- the port-5557 debug payload
 *                         (src/cpacketizer.cc:127,131-134); entry 0 is 0
 *   packet crsdr_plan_packet_bytes() bytes: hdr0{seq,N,L,0} + u32 readcnt[N] + int8 [N][B]
 *          (include/cpacketizer.h:32-37; parser matlabclient/zmqsdr.c:118-144).
 * Rows outside the plan's slab hold whatever the bound buffer held (zeros by default). */
int crsdr_plan_fetch(crsdr_plan *plan, int32_t *lag, float *mag, float *frac, float *phasor,
                     int8_t *packet);
/* Same for block `block` (0-based) of the last submitted batch; -1 = its last block, which is
 * what crsdr_plan_fetch returns. */
int crsdr_plan_fetch_block(crsdr_plan *plan, int block, int32_t *lag, float *mag, float *frac, float *phasor,
                           int8_t *packet);

/* Fractional-delay correction (BASELINE config 5 "long-block regime + fractional-delay phase correction"; SURVEY 8 note
 * "Fractional delay": report D and, if applied, apply it as a linear phase ramp in the frequency domain).  The reference
 * computes a 3-point estimate and discards it (src/ccoherent.cc:206-219); its authors' study of applying one
 * (matlabclient/notes.m:9-40) finds a signal-dependent gain between estimate and true delay, hence `gain` / the override.
 * CRSDR_MODE_DIGITAL only; off by default (the reference-faithful behaviour).  Every block size: long blocks (blocksize > 16384) run a
 * second four-step pass (below), LDS-resident blocks one extra kernel per batch behind the phase kernels (row -> forward transform ->
 * x the response -> inverse -> int8 over the row the phase kernel wrote), for which enable = 1 and 2 are the same and nothing is allocated.
 * With it on, row k of the matrix is the row advanced by lag_k + D_k samples -- a circular advance of the zero-padded row in
 * the frequency domain: X[f] * exp(+2 pi i f_s (lag_k + D_k) / B), f_s the signed bin index -- then rotated by the phasor
 * and quantised like cdsp::convto8bit; for D = 0 that is the digital mode's zero-filled integer shift.
 *   The advance is CIRCULAR over the 2 L samples of the zero-padded row (L = blocksize / 2 complex samples, B = 2 L bins): output
 *   sample n is the band-limited interpolation of the padded row at (n + lag_k + D_k) mod 2 L.  For |lag_k + D_k| <= L the samples
 *   that leave the row are lost into the padding; for |lag_k + D_k| > L -- a lag at the end of its range, |lag_k| >= L - 64, with
 *   a D_k of the same sign -- the advance wraps: |lag_k + D_k| - L samples re-enter from the OTHER end of the row (lag_k = -L,
 *   the all-zero row's lag, with D_k < 0 brings the row's last samples in first).  Nothing is zeroed beyond what the padding gives.
 *   D_k = frac_override[k] if given (host [nrows], copied; entry 0 ignored), else gain * frac_k (this block's estimate).
 *   Bounds: |gain| <= 128 and |frac_override[k]| <= 64 samples (CRSDR_EINVAL otherwise): the response's phase is formed in fp32 and
 *   keeps 1e-5 rad up to there; a proper peak's estimate is |frac| <= 1/2.  Larger delays belong in the integer lag.
 * lag / mag / frac / phasor outputs are unchanged (the phase is still estimated on the integer-aligned row).
 *   enable = 1: allocates (once, here -- never on the per-block path) a second cf32 work area of 8 * blocksize bytes per owned row,
 *               so that the correction pass reuses the correlation pass's first stage, and 128 KiB per owned row for the rows'
 *               response spectra; if the work area cannot be had the pass repeats its first stage instead (= enable 2);
 *   enable = 2: the memory-lean form: no second work area, the pass repeats its first stage (same results, bit for bit);
 *   enable = 0: off; both buffers are freed (after a sync). */
int crsdr_plan_set_frac_apply(crsdr_plan *plan, int enable, float gain, const float *frac_override);

/* Reference-noise canceller.  The reference switches its noise source on to calibrate and off to measure (src/ccoherent.cc:271, the
 * crefnoise gate; CRSDR_REFNOISE_ENABLED here): with the source on every signal row carries the noise far above any emitter.  With
 * the canceller on, the owned signal rows of blocks submitted with CRSDR_REFNOISE_ENABLED have the reference row projected out by a
 * short least-squares FIR before they are rotated and quantised, so that a host may calibrate and measure on the same block.
 * CRSDR_MODE_DIGITAL plans with blocksize <= 16384; taps = 2 K + 1 odd in 1 .. 9; off by default.  A batch submitted without the
 * flag does not run the pass: its packets have the bits of a plan with the canceller off, status is 2 for every owned row, the
 * coefficients are 0 (and the residual 1).  No state is carried from block to block.
 * Per owned row and block, L = blocksize / 2, all values signed int8 counts (offset-binary input is ^ 0x80 first):
 *   1. y[n] = s[n + d] for 0 <= n + d < L, zero elsewhere; d the lag the digital mode shifts the row by: the row the phase path uses.
 *   2. r_j[n] = r[n - j] for 0 <= n - j < L, zero elsewhere, j = -K .. K; r the block's reference row.
 *   3. exact integer sums  c_j = sum_n y[n] conj(r_j[n]),  G_ij = sum_n conj(r_i[n]) r_j[n]  (the full Hermitian Gram with the
 *      zero-filled edges, not its Toeplitz approximation),  E = sum_n |y[n]|^2.  c_0 is the sum the phasor is formed from: the phase
 *      estimate, the EMA chain and the outputs lag / mag / frac / phasor keep their bits.
 *   4. G g = c solved in fp64 by Cholesky (operation order not pinned).  A pivot <= 2^-40 G_00 (G_00 the centre entry sum |r|^2) is a
 *      failure -- an all-zero or rank-deficient reference row: g = 0 and status bit 0 is set.  g is published rounded once to fp32,
 *      j ascending.  residual = clamp((E - Re sum_j conj(g_j) c_j) / E, 0, 1), formed in fp64 with the unrounded g and rounded once;
 *      1 if E == 0: the share of the row's power that stays.
 *   5. z[n] = y[n] - sum_j g_j r_j[n];  w = p z, p the block's phasor as published;  out = clip(rint(w), -128, 127), ties to even,
 *      I and Q each.  The published g and p are used in fp32 arithmetic whose order is not pinned; there is no 1/127 round trip.  With
 *      g = 0 this is the plain rotation; it is not promised to match the phase path's bits on ties.  The row lands where the phase
 *      path would have put it (packet matrix, bound packet or bound slab); header, read counters and row 0 are untouched.
 * crsdr_plan_set_refcancel: taps = 0 turns it off and frees what the call allocated (after a sync); 1, 3, 5, 7, 9 turn it on and
 *   allocate everything here ([max_batch][nrows][9][2] fp32 coefficients, [max_batch][nrows] residual and status, the blocks' Grams):
 *   nothing is allocated per submit.  CRSDR_EINVAL for another count, a CRSDR_MODE_FAITHFUL plan or blocksize > 16384; CRSDR_ESTATE
 *   while crsdr_plan_set_frac_apply is on, and that call answers CRSDR_ESTATE while this is on (its pass re-reads the raw row: the two
 *   do not compose).  A batch that runs the pass takes the three-kernel phase path in front of it.
 * crsdr_plan_fetch_refcancel: waits and reports kernel-side errors as crsdr_plan_fetch_block does; block -1 = the last block.  coef
 *   [nrows][taps][2], residual [nrows], status [nrows] (any may be NULL); rows outside the slab and row 0 hold zeros.
 * crsdr_plan_refcancel_buffers: the device arrays for consumers on the plan's stream -- coef [max_batch][nrows][9][2] (a row's taps
 *   first, zeros behind), residual and status [max_batch][nrows] -- and the tap count.  CRSDR_ESTATE while off. */
int crsdr_plan_set_refcancel(crsdr_plan *plan, int taps);
int crsdr_plan_fetch_refcancel(crsdr_plan *plan, int block, float *coef /* [nrows][taps][2] */, float *residual /* [nrows] */,
                               int32_t *status /* [nrows] */);
int crsdr_plan_refcancel_buffers(crsdr_plan *plan, void **coef, void **residual, void **status, int *taps);

/* The per-op form: one block with the lags and phasors given, the same device functions, bit for bit.  rows [nrows][blocksize] (row 0
 * the reference), lag [nrows], phasor [nrows][2] (entry 0 of both ignored) -> out [nrows][blocksize] (row 0 copied, as two's
 * complement), coef [nrows][taps][2], residual [nrows], status [nrows] (row 0: zeros).  blocksize a power of two in 16 .. 16384, taps
 * as above, |lag| <= blocksize / 2 (lag = -L or L: the all-zero row), flags CRSDR_OFFSET_BINARY or 0, out apart from rows.  Every
 * argument is checked before a device is touched (a lag in device memory is clamped to the range instead).  mem_kind: CRSDR_MEM_HOST
 * (copied) or CRSDR_MEM_DEVICE (all on the device: rows and out 4-byte aligned, 16-byte for the vector kernels; coef and phasor 8-byte). */
int crsdr_refcancel(int8_t *out, float *coef, float *residual, int32_t *status, const int8_t *rows, int nrows, int blocksize,
                    const int32_t *lag, const float *phasor, int taps, uint32_t flags, int mem_kind);

/* Pipelined fetch of the LAST submitted batch into page-locked host memory (crsdr_host_alloc): the device-to-host copies
 * run on the plan's copy stream as soon as the batch's kernels have finished -- while the NEXT submit's host-to-device copies
 * use the other direction of the link; the next submit's kernels wait on the device for these copies, so the plan's output
 * buffers are never overwritten under them.  The host engine's loop (src/ccoherent.cc:245-294 run a batch at a time):
 *     submit_batch(b) ; fetch_batch_async(b) ; submit_batch(b+1) ; fetch_batch_async(b+1) ; fetch_wait() -> batch b has landed ; ...
 * Any pointer may be NULL.  lag / mag / frac: [nblocks][nrows]; phasor [nblocks][nrows][2]; packets: the batch's nblocks
 * packets, packet t at packets + t * host_packet_stride (>= crsdr_plan_packet_bytes).  Pageable destinations work but
 * serialise.  crsdr_plan_fetch_wait blocks until the OLDEST outstanding asynchronous fetch has landed (at most four may be
 * outstanding; later ones keep flying) and reports a kernel-side error like crsdr_plan_fetch does. */
int crsdr_plan_fetch_batch_async(crsdr_plan *plan, int32_t *lag, float *mag, float *frac, float *phasor, int8_t *packets,
                                 size_t host_packet_stride);
int crsdr_plan_fetch_wait(crsdr_plan *plan);

/* Block until everything submitted so far has finished (no copies). */
int crsdr_plan_sync(crsdr_plan *plan);

size_t crsdr_plan_packet_bytes(const crsdr_plan *plan);   /* 16 + 4N + N*B */
size_t crsdr_plan_matrix_offset(const crsdr_plan *plan);  /* 16 + 4N */
size_t crsdr_plan_packet_stride(const crsdr_plan *plan);  /* bytes between the packets of a batch */

/* Device-resident results for pipelines that never leave HBM (multi-GPU gather, benchmarks).
 * The packet pointer is 4-byte aligned and the matrix inside it 256-byte aligned; per-row arrays
 * are [max_batch][nrows] (block t of the last batch at + t * nrows).  lag / mag / frac alternate between two
 * such arrays from submit to submit: call this after the submit whose results are wanted; the pointers stay valid
 * (and unmodified) until the submit after the next one. */
int crsdr_plan_device_buffers(crsdr_plan *plan, void **packet, void **lag, void **mag,
                              void **frac, void **phasor);
/* Write the packets of later submits into a caller-owned device buffer instead: block t of a
 * batch at device_packet + t * packet_stride (matrix start and stride 4-byte aligned, stride >=
 * packet_bytes); NULL restores the plan's own buffer.  Does not synchronise: double-buffering
 * against a gather in flight is the caller's business. */
int crsdr_plan_bind_packet(crsdr_plan *plan, void *device_packet, size_t packet_stride);

/* Sharded plans (row_begin / row_count set): slab output for the matrix exchange between GPUs.
 * With a slab bound, the owned rows of block t of a batch are written densely at
 *   device_slab + t*slab_stride + (row - row_begin)*blocksize          (slab_stride >= row_count*blocksize)
 * instead of into the packet matrix, so one rank's batch is a contiguous [nblocks][row_count][blocksize]
 * buffer -- the send buffer of ONE all-to-all per batch (equal splits: blocks [q*nblocks/G, (q+1)*nblocks/G) go
 * to rank q).  Header + readcnt + row 0 (cpacketize::write(0, ..), src/ccoherent.cc:253) are written only for
 * blocks hdr_first <= t < hdr_first + hdr_count -- the blocks this rank assembles -- into packet
 * (t - hdr_first) of the bound packet buffer.  device_slab = NULL returns to packet output.  No sync. */
int crsdr_plan_bind_slab(crsdr_plan *plan, void *device_slab, size_t slab_stride, int hdr_first, int hdr_count);

/* On the assembling rank: recv [nsrc][nblocks][(nrows-1)/nsrc][blocksize] int8 (the all-to-all's receive
 * buffer: chunk src = that rank's slabs of the nblocks blocks assembled here) -> matrix rows 1 + src*per ..
 * of packet j at device_packets + j*packet_stride.  Replaces the per-row cpacketize::write(c, ..) calls of
 * src/ccoherent.cc:277 for rows computed on other GPUs.  Device pointers; asynchronous on hip_stream
 * (a hipStream_t, NULL = the null stream).  Independent of any plan. */
int crsdr_assemble_slabs(void *device_packets, size_t packet_stride, int nrows, int blocksize, const void *device_recv, int nsrc,
                         int nblocks, void *hip_stream);

/* ---- exchange slots: rows + per-row scalars, one message per peer -------------------------------------
 * The gather of SURVEY 8e carries the int8 rows PLUS 24 bytes per row of {lag, mag, frac, phasor, readcnt}: what
 * csdrdevice::set_lag (src/ccoherent.cc:232-233), the port-5557 debug payload (src/cpacketizer.cc:127,131-134) and the packet
 * header's per-device read counters (src/cpacketizer.cc:142,163) consume on the assembling side -- a rank need only know the
 * counters of row 0 and of the rows it owns.  crsdr_plan_bind_slab_ex is crsdr_plan_bind_slab with a TAIL per block: block t of a
 * batch goes to the slot  device_slab + t*slab_stride =
 *     [row_count][blocksize] int8 rows | at +tail_offset:  int32 lag[rc] | float mag[rc] | float frac[rc] | float phasor[rc][2] | uint32 readcnt[rc]
 * (tail_offset >= row_count*blocksize, 4-byte aligned, tail_offset + 24*row_count <= slab_stride; 0 = no tail).  A rank's
 * slots of the blocks rooted on one peer are consecutive, so they travel as ONE message whatever the block count. */
int crsdr_plan_bind_slab_ex(crsdr_plan *plan, void *device_slab, size_t slab_stride, int hdr_first, int hdr_count, size_t tail_offset);

/* Slot geometry both sides of an exchange agree on (pure arithmetic, no device needed):
 *   per = (nrows-1)/nranks rows per rank;  tail_offset = per*blocksize;  slot_stride = tail_offset + 24*per rounded up to 16;
 *   scalars_stride = 20*nrows rounded up to 16 (one assembled scalars block per packet, layout below). */
int crsdr_exchange_geometry(int nrows, int blocksize, int nranks, size_t *slot_stride, size_t *tail_offset, size_t *scalars_stride);

/* Which rank assembles block t of a batch of nblocks blocks: blocks are dealt in runs of bpr = ceil(nblocks / nranks),
 * root(t) = t / bpr -- rank q assembles blocks [q*bpr, min(nblocks, (q+1)*bpr)), a rotating root at batch granularity (a fixed
 * root would ingest (G-1)/G of every block over its own xGMI links).  first/count: rank's range (count may be 0). */
int crsdr_exchange_rooted_blocks(int nblocks, int nranks, int rank, int *first, int *count);

/* On the assembling rank: recv [nsrc][nblocks][slot_stride] (chunk src = rank src's slots of the nblocks blocks assembled here,
 * what an all-to-all of the send buffers delivers) ->  rows into matrix rows 1 + src*per .. of packet j at
 * device_packets + j*packet_stride;  tails into the scalars block j at device_scalars + j*scalars_stride =
 *     int32 lag[nrows] | float mag[nrows] | float frac[nrows] | float phasor[nrows][2]      (row 0: zeros, like crsdr_plan_fetch;
 *     the phasor part is the N x complex<float> port-5557 payload as is)
 * and, whenever the slots have tails, the read counters of rank src's rows into packet j's header (uint32 readcnt[N] at +16): the header
 * the assembling rank's own plan wrote holds ITS view of every counter, right for row 0 and its own rows.
 * self_rank >= 0 with device_self != NULL: that rank's chunk is read from device_self (its own send slots) instead of recv.
 * device_scalars may be NULL.  Asynchronous on hip_stream.  Replaces crsdr_assemble_slabs when tails travel with the rows. */
int crsdr_assemble_slots(void *device_packets, size_t packet_stride, void *device_scalars, size_t scalars_stride, int nrows, int blocksize,
                         const void *device_recv, int nsrc, int nblocks, size_t slot_stride, size_t tail_offset, int self_rank,
                         const void *device_self, void *hip_stream);

/* ---- the exchange itself under the C ABI: RCCL over xGMI, one process per GPU --------------------------------------
 * librccl is resolved at run time (dlopen "librccl.so.1"): a host that never creates an exchange does not need it.
 * The reference has no collective (its only transport is ZMQ, src/cpacketizer.cc:58-66); this is the one exchange step
 * SURVEY 8e adds.  Rendez-vous: rank 0 calls crsdr_exchange_unique_id and hands the 128 bytes to the other ranks by
 * whatever channel the host has (MPI, a socket, a file); every rank then calls crsdr_exchange_create. */
#define CRSDR_EXCHANGE_ID_BYTES 128
typedef struct crsdr_exchange crsdr_exchange;
int crsdr_exchange_unique_id(void *id /* [CRSDR_EXCHANGE_ID_BYTES] */);
int crsdr_exchange_create(crsdr_exchange **x, const void *id, int nranks, int rank, int device);
int crsdr_exchange_destroy(crsdr_exchange *x);

enum {
    CRSDR_XCHG_STAGED = 0,   /* one message per peer into device_recv, then crsdr_assemble_slots (what an all-to-all does) */
    CRSDR_XCHG_INPLACE = 1   /* rows land straight in the packet matrix (one message per block and peer, no assembly copy
                                of remote rows); only the 24 B/row tails go through a small staging buffer */
};
/* One batch of nblocks blocks (every rank calls it with the same nblocks / mode, after the submit that filled device_send on
 * hip_stream): rank q = root of blocks [q*bpr, ...) receives every rank's slots of those blocks; on return (stream order) the
 * count packets at device_packets hold all rows and device_scalars the assembled scalars blocks.
 *   device_send   this rank's slots [nblocks][slot_stride] (crsdr_plan_bind_slab_ex with the geometry above)
 *   device_recv   staging of >= nranks * bpr * slot_stride bytes (CRSDR_XCHG_STAGED; may be NULL for CRSDR_XCHG_INPLACE)
 * All RCCL calls are issued in one group on hip_stream; nothing blocks the host. */
int crsdr_exchange_batch(crsdr_exchange *x, int mode, const void *device_send, void *device_recv, int nblocks, void *device_packets,
                         size_t packet_stride, void *device_scalars, size_t scalars_stride, int nrows, int blocksize, void *hip_stream);

/* The point-to-point operations crsdr_exchange_batch issues for (nranks, rank, nblocks, mode), in issue order -- pure host
 * arithmetic, exported so that the matching of every send with its receive can be checked without GPUs (tests simulate the
 * ranks and pair each rank's sends to a peer with that peer's receives from it, first in first out, as RCCL does).
 * buffer: 0 = device_send, 1 = device_recv, 2 = device_packets, 3 = the exchange's tail staging ([nranks][bpr][24*per rounded to 16]). */
typedef struct crsdr_xop {
    int32_t peer;      /* the other rank */
    int32_t is_recv;   /* 0 = send, 1 = receive */
    int32_t buffer;    /* which buffer `offset` is relative to (above) */
    int32_t block;     /* batch-relative block index the bytes belong to (first block for multi-block messages) */
    uint64_t offset, bytes;
} crsdr_xop;
int crsdr_exchange_schedule(int nranks, int rank, int nblocks, int mode, int nrows, int blocksize, size_t packet_stride,
                            crsdr_xop *ops, int capacity, int *count);

/* ---- a sharded plan and its exchange as ONE engine: what a C++ host with one process per GPU runs (host/ccoherent.cc with
 * ranks > 1; the loop of src/ccoherent.cc:245-294 a batch at a time, rows split over the GPUs of the node).
 * crsdr_exchange_bind_plan allocates, once, everything the exchange of the plan's batches needs on the device -- two ring-buffered
 * sets of: the send slots [max_batch][slot_stride] the plan writes its rows and tails into, the receive staging, the
 * bpr = ceil(max_batch / nranks) packets this rank assembles per batch and their scalars blocks -- plus a side stream for the
 * exchange, so the host handles no device memory and no stream.  The plan must own rank's slab (row_begin = 1 + rank * per,
 * row_count = per) on the exchange's device.  Afterwards the plan is driven through the two calls below only. */
int crsdr_exchange_bind_plan(crsdr_exchange *x, crsdr_plan *plan, int mode /* CRSDR_XCHG_* */);
/* crsdr_plan_submit_batch (same arguments) into the next set, then crsdr_exchange_batch on the side stream: everything is enqueued
 * on return; the exchange of this batch runs under the compute of the next one.  At most two batches may be outstanding. */
int crsdr_exchange_submit_batch(crsdr_exchange *x, const void *rows, int mem_kind, int nblocks, size_t block_stride, const uint32_t *readcnt,
                                const uint8_t *lag_mask, uint32_t seq, uint32_t flags);
/* Waits for the OLDEST outstanding batch and copies what this rank assembled of it to host memory: blocks [*first, *first + *count)
 * of the batch (crsdr_exchange_rooted_blocks; count may be 0) -- packet j at packets + j * host_packet_stride, its scalars block
 * (int32 lag[N] | float mag[N] | float frac[N] | float phasor[N][2], 20 * nrows bytes) at scalars + j * host_scalars_stride.
 * own_tails: {lag, mag, frac, phasor} of this rank's OWN rows for every block of the batch -- block t at own_tails + t * host_tails_stride
 * as  int32 lag[per] | float mag[per] | float frac[per] | float phasor[per][2] | uint32 readcnt[per]  (24 * per bytes): what csdrdevice::set_lag needs on the
 * process that reads those dongles (src/ccoherent.cc:232-233), whichever rank assembles the block; *nblocks = blocks in the batch.
 * Any pointer may be NULL.  Reports a kernel-side error like crsdr_plan_fetch_wait does (the plan is rolled back and what else was
 * outstanding on THIS rank is dropped).  The ranks' exchange sequences stay matched -- the failing rank's sends of those batches were
 * issued -- but its peers assembled garbage rows from it: a host that wants the batches back resubmits them on every rank, in the
 * same order. */
int crsdr_exchange_fetch_rooted(crsdr_exchange *x, int8_t *packets, size_t host_packet_stride, void *scalars, size_t host_scalars_stride,
                                void *own_tails, size_t host_tails_stride, int *first, int *count, int *nblocks);

/* With profiling enabled (CRSDR_PROFILE_SUBMIT): elapsed GPU milliseconds on the plan's stream
 * between the start and the end of the most recent submit. */
int crsdr_plan_last_elapsed_ms(crsdr_plan *plan, float *ms);

/* Per-kernel timing with hipEvents recorded on the stream each kernel is launched on.
 * enable: keep event pairs for the last `slots` submits (0 disables) for the kernels in
 * `kernel_mask` (bit CRSDR_KERNEL_*; CRSDR_PROFILE_SUBMIT adds whole-submit start/stop events --
 * every recorded pair costs a few microseconds of stream time, so profile only what is read).
 * kernel_times: copy the durations (ms) of kernel `which` for the submits recorded since enable,
 * oldest first. */
enum { CRSDR_KERNEL_REF_SPECTRUM = 0, CRSDR_KERNEL_XCORR_LAG = 1, CRSDR_KERNEL_PHASE_DOT = 2, CRSDR_KERNEL_ALIGN_QUANT = 3 };
#define CRSDR_PROFILE_ALL_KERNELS 0xFu
#define CRSDR_PROFILE_SUBMIT (1u << 31)
int crsdr_plan_enable_profiling(crsdr_plan *plan, int slots, uint32_t kernel_mask);
int crsdr_plan_kernel_times(crsdr_plan *plan, int which, float *ms, int capacity, int *count);

/* ------------------------------------------------------------------------------------------
 * (iii) downstream helper: what the reference's beamformer computes first from a packet
 * ---------------------------------------------------------------------------------------- */

/* Sample covariance of the signal channels of one aligned receive matrix, as
 * beamformclient/heatmap2d2.cpp:189-199 forms it:  X(n, c) = (I + jQ)/127 of channel c >= 1 (row 0,
 * the reference channel, is dropped), per-channel mean removed,  Rxx = (1/L) X^H X.
 *   matrix [nrows][blocksize] int8 -- the data part of a packet (packet + crsdr_plan_matrix_offset)
 *   rxx    [(nrows-1)][(nrows-1)][2] float, row-major, rxx[a][b] = (1/L) sum_n conj(x_a[n]) x_b[n] - conj(mean_a) mean_b
 * Runs as an int8 GEMM on the matrix cores (v_mfma_i32_32x32x32_i8), exact integer sums (int32 per at most 65536 bytes of a row,
 * added in 64 bits: full-scale rows of any length are exact), fp64 epilogue.
 * blocksize % 32 == 0; above 65536: % 512 == 0.  mem_kind: CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE (both pointers on the device;
 * the matrix may sit where a packet holds it, 4-byte aligned). */
int crsdr_covariance(float *rxx, const int8_t *matrix, int nrows, int blocksize, int mem_kind);

/* Signal / noise subspaces of a Hermitian covariance, replacing noisesubspace(Rxx, K)
 * (beamformclient/heatmap2d2.cpp:69-79: BDCSVD of Rxx, Un = U.rightCols(M - K)).
 *   rxx [m][m][2] float row-major (the output of crsdr_covariance), 2 <= m <= 64
 *   sv  [m] singular values, descending (NULL to skip)
 *   vec [m][m][2] float row-major; column r is the singular vector of sv[r], so the noise subspace for K
 *       sources is columns K .. m-1 (a basis of it: only the projector Un Un^H is unique)
 * One workgroup, one-sided Jacobi in fp64 with the matrix resident in LDS; no host arithmetic.
 * Returns CRSDR_ESTATE if the iteration did not converge (vec / sv are still written). */
int crsdr_noisesubspace(float *vec, float *sv, const float *rxx, int m, int mem_kind);

/* 2-D MUSIC pseudo-spectrum of a uniform rectangular array, replacing pmusic2dvec(Un, d, Mx, My, Cx, Cy)
 * with s_vecd2d and pmusic (beamformclient/heatmap2d2.cpp:103-147, called at :199 with d = 1.225*1.24/3,
 * Mx = 7, My = 3, Cx = Cy = 100):
 *   a(alpha, beta)[iy*mx + ix] = exp(2 pi j ix d cos(alpha) sin(beta)) exp(2 pi j iy d cos(beta)),
 *   alpha = cx pi / ncx, beta = cy pi / ncy,   pm[cx][cy] = ( |a|^2 / |Un^H a|^2 )^2      (squared twice, :123)
 *   vec [m][m][2] as written by crsdr_noisesubspace, m = mx*my <= 64; Un = its columns k .. m-1, 1 <= k < m
 *   pm  [ncx][ncy] float row-major, not normalised (the reference divides by the maximum for plotting, :202-203) */
int crsdr_pmusic2d(float *pm, const float *vec, int m, int k, float d, int mx, int my, int ncx, int ncy, int mem_kind);

/* Beams from one aligned receive matrix: out[b][n] = sum_c weights[b][c-1] * (I_c[n] + j Q_c[n]) / 127 over the signal rows
 * c = 1 .. nrows-1 (row 0, the reference channel, is dropped as in crsdr_covariance), n < blocksize/2, fp32, no conjugate (see
 * crsdr_doa_set_beams for why).  The per-op form of the batched engine's beam kernel: the same arithmetic, bit for bit.
 *   matrix  [nrows][blocksize] int8, 2 <= nrows <= 65, blocksize % 32 == 0
 *   weights [nbeams][nrows-1][2] float, 1 <= nbeams <= 16
 *   out     [nbeams][blocksize/2][2] float
 * mem_kind: CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE (all three on the device: matrix 4-byte, weights 8-byte, out 16-byte aligned). */
int crsdr_beamform(float *out, const int8_t *matrix, int nrows, int blocksize, const float *weights, int nbeams, int mem_kind);

/* ------------------------------------------------------------------------------------------
 * (iv) batched direction-of-arrival engine: the chain above for a whole batch of packets where a plan left them
 * ---------------------------------------------------------------------------------------- */

/* crsdr_covariance -> crsdr_noisesubspace -> crsdr_pmusic2d -> index of the largest pm, for up to 64 packets per submit, one estimate
 * per `frames` consecutive packets (their samples stacked, X = [X; Xc] as measurement_script.m does: L = frames * blocksize / 2).
 * Every buffer is allocated by crsdr_doa_create (or crsdr_doa_set_peaks).  A submit is asynchronous on its stream: five kernel launches whatever the
 * number of blocks, no allocation, no process-wide lock, nothing that waits for the device.  Per estimate the numbers are those of
 * the per-op calls on the same matrix, bit for bit (exact integer sums with the same fp64 epilogue; the same instruction sequence
 * for the subspace and for every grid point). */
typedef struct crsdr_doa crsdr_doa;

enum {
    CRSDR_DOA_KEEP_SPECTRUM = 1u << 0, /* keep pm[ncx][ncy] of every estimate (otherwise only the peak leaves the scan) */
    CRSDR_DOA_KEEP_RXX = 1u << 1       /* allow crsdr_doa_fetch to return the covariances */
};

typedef struct crsdr_doa_desc {
    int32_t nrows, blocksize; /* of the packets it reads (as in crsdr_plan_desc); m = nrows - 1 = mx * my signal rows, 2 <= m <= 64;
                                 blocksize % 32 == 0 */
    int32_t device;
    int32_t max_batch;        /* blocks per submit, 1..64 (0 = 1) */
    int32_t frames;           /* F >= 1 consecutive blocks stacked into one estimate, F <= max_batch (0 = 1) */
    int32_t k;                /* number of sources, 1 <= k < m */
    int32_t mx, my, ncx, ncy; /* array and scan grid, as crsdr_pmusic2d */
    float d;
    uint32_t flags;           /* CRSDR_DOA_KEEP_* */
} crsdr_doa_desc;

int crsdr_doa_create(crsdr_doa **doa, const crsdr_doa_desc *desc);
int crsdr_doa_destroy(crsdr_doa *doa);

/* nblocks packets on the doa's device, packet t at device_packets + t * packet_stride, its matrix [nrows][blocksize] int8 at
 * + matrix_offset (4-byte aligned, like packet_stride); 1 <= nblocks <= max_batch, nblocks % frames == 0.  Asynchronous on hip_stream
 * (NULL = the object's own stream); the packets must stay valid until the work has run.  One submit at a time: the next one reuses
 * the buffers of this one, so fetch (or order the streams) in between. */
int crsdr_doa_submit(crsdr_doa *doa, const void *device_packets, size_t packet_stride, size_t matrix_offset, int nblocks,
                     void *hip_stream);

/* The plan's last submitted batch, where its packets are (own buffer or crsdr_plan_bind_packet), on the plan's stream: ordered
 * behind that batch by the stream alone, no host wait in between.  CRSDR_ESTATE for a plan with nothing submitted or with a slab
 * bound (the matrix is then not in the packet); CRSDR_EINVAL for another geometry or device, or a batch that is not a multiple of
 * `frames` or exceeds max_batch. */
int crsdr_doa_submit_plan(crsdr_doa *doa, crsdr_plan *plan);

/* Waits for the last submit and copies out what is asked for (any pointer may be NULL); nest = nblocks / frames.
 *   peak       [nest][2] int32 (cx, cy) of the largest pm; the first index in row-major order on ties (as crsdr_indexofmax).  A NaN
 *              pm counts as the largest value (numpy's argmax convention).
 *   peak_value [nest]      that pm
 *   sv         [nest][m]   singular values, descending
 *   status     [nest]      0 = converged, 1 = the Jacobi sweeps ran out (sv / peak are still written: data, not a failed call)
 *   pm         [nest][ncx][ncy]   CRSDR_EINVAL without CRSDR_DOA_KEEP_SPECTRUM
 *   rxx        [nest][m][m][2]    CRSDR_EINVAL without CRSDR_DOA_KEEP_RXX
 * CRSDR_ESTATE before the first submit. */
int crsdr_doa_fetch(crsdr_doa *doa, int32_t *peak, float *peak_value, float *sv, int32_t *status, float *pm, float *rxx);

/* Device addresses of the results ([max_batch / frames] estimates each, laid out as above; vec [nest][m][m][2] as
 * crsdr_noisesubspace writes it; pm is NULL without CRSDR_DOA_KEEP_SPECTRUM), for consumers on the same stream. */
int crsdr_doa_device_buffers(crsdr_doa *doa, void **peak, void **peak_value, void **sv, void **vec, void **pm);

/* Of the last submit: the number of estimates (what crsdr_doa_fetch will write) and the kernel launches it issued (the same for
 * every nblocks).  Either pointer may be NULL.  CRSDR_ESTATE before the first submit. */
int crsdr_doa_last_submit(crsdr_doa *doa, int *nest, int *launches);

/* Several directions per estimate: the `count` strongest local maxima of each spectrum, found on the device.  Grid point
 * g = cx * ncy + cy has the key (bits(pm) << 32) | (0xFFFFFFFF - g) (a NaN pm as 0x7FC00000, as for peak); it is a local peak if its
 * key is larger than that of every other grid point with |cx' - cx| <= radius and |cy' - cy| <= radius (the window clipped at the
 * grid's edges, no wrap-around).  The global maximum is always one, so the first direction is crsdr_doa_fetch's peak, bit for bit.
 * 1 <= count <= 16, 1 <= radius <= 16; count = 0 turns the pass off (radius is then ignored).  Any time: waits for the device if a
 * submit was made, then allocates what the pass needs (a spectrum workspace [max_batch / frames][ncx][ncy] float unless the object
 * keeps the spectrum).  A submit with peaks on is seven launches instead of five, the same for every nblocks.  CRSDR_EINVAL for a
 * bad count or radius. */
int crsdr_doa_set_peaks(crsdr_doa *doa, int count, int radius);

/* Waits for the last submit and copies out (any pointer may be NULL), nest as for crsdr_doa_fetch:
 *   found  [nest]            local peaks found, at most count
 *   peaks  [nest][count][2]  (cx, cy) in descending key order: descending pm, the lower row-major index first on ties
 *   values [nest][count]     their pm
 * Slots from found on hold (-1, -1) and -1.0f.  CRSDR_ESTATE without crsdr_doa_set_peaks or before the first submit after it. */
int crsdr_doa_fetch_directions(crsdr_doa *doa, int32_t *found, int32_t *peaks, float *values);

/* Device addresses of found, peaks and values ([max_batch / frames] estimates, laid out as above; NULL while peaks are off), for
 * consumers on the same stream.  They change with every crsdr_doa_set_peaks. */
int crsdr_doa_direction_buffers(crsdr_doa *doa, void **found, void **peaks, void **values);

/* Beams toward the directions: per estimate e and beam slot b a weight vector u (m complex entries) from the subspace the engine
 * holds, and for every block t of the estimate one IQ stream per slot, all on the device, behind the same submit.
 *   direction  nfixed = 0: slot b of the estimate's own directions -- with crsdr_doa_set_peaks on, peaks[e][b] for b < found[e] (count
 *              slots); with peaks off one slot, peak[e]; alpha = cx pi / ncx, beta = cy pi / ncy.
 *              nfixed = 1..16: the (alpha_b, beta_b) of fixed_angles [nfixed][2] (radians, host pointer, copied), for every estimate.
 *   steering   a[iy*mx + ix] = exp(2 pi j d (ix cos(alpha) sin(beta) + iy cos(beta))), crsdr_pmusic2d's vector, in fp64
 *   weights    fp64 from the published fp32 vec[e] (column r = v_r) and sv[e], rounded once to fp32:
 *              CRSDR_BEAM_CONVENTIONAL  u = a / m
 *              CRSDR_BEAM_MVDR          delta = loading * sv[0],  z = sum_r v_r (v_r^H a) / (sv[r] + delta),  u = z / Re(a^H z);
 *                                       sv[0] == 0 (an all-zero estimate): u = a / m
 *   power      conventional: sum_r sv[r] |v_r^H a|^2 / m^2 (= a^H Rxx a / m^2); MVDR: 1 / Re(a^H z), the Capon estimate of the loaded
 *              covariance (0 in the sv[0] == 0 case).  It tells a source from a side-lobe peak of the MUSIC spectrum.
 *   beams      y[t][b][n] = sum_c u[c-1] (I_c[n] + j Q_c[n]) / 127 over the signal rows c = 1 .. m, n < blocksize/2, fp32, NO
 *              conjugate: the covariance is X^H X, the conjugate of E[x x^H], so the steering vector at a MUSIC peak is conj(a_true) and
 *              w^H x with the textbook w = R^-1 a / (a^H R^-1 a) becomes u^T x; sum_c u_c conj(a_c) = 1 is the distortionless constraint.
 *              The mean is not removed from the samples.  (crsdr_caf's bearings, section (w), meet the same convention from the
 *              other side: chi_c carries a_true, so their snapshot is u = conj(chi) and the same emitter gives the same grid cell.)
 *   Slots b >= found[e]: weights 0, power -1, beam samples 0.
 * mode CRSDR_BEAM_OFF frees the buffers (the other arguments are then ignored).  loading in [1e-6, 1] (ignored for CONVENTIONAL).
 * Any time: waits for the device if a submit was made, then allocates weights, power and beams [max_batch][nbeams][blocksize/2][2].
 * A submit with beams on is two launches more (5 -> 7, 7 -> 9), the same for every nblocks, still without allocation, lock or host wait.
 * While beams follow the directions (nfixed = 0) crsdr_doa_set_peaks returns CRSDR_ESTATE: their buffers are sized by its count, turn
 * the beams off first.  CRSDR_EINVAL for a bad mode, loading outside the range in MVDR mode, nfixed outside 0..16 or NULL angles. */
enum { CRSDR_BEAM_OFF = 0, CRSDR_BEAM_CONVENTIONAL = 1, CRSDR_BEAM_MVDR = 2 };
int crsdr_doa_set_beams(crsdr_doa *doa, int mode, float loading, int nfixed, const float *fixed_angles);

/* Waits for the last submit and copies out (any pointer may be NULL): weights [nest][nbeams][m][2], power [nest][nbeams],
 * beams [nblocks][nbeams][blocksize/2][2].  CRSDR_ESTATE with beams off or before the first submit after crsdr_doa_set_beams. */
int crsdr_doa_fetch_beams(crsdr_doa *doa, float *weights, float *power, float *beams);

/* Device addresses of weights, power and beams (laid out as above for [max_batch / frames] estimates and max_batch blocks; NULL
 * while beams are off) and the slot count, for consumers on the same stream.  They change with every crsdr_doa_set_beams. */
int crsdr_doa_beam_buffers(crsdr_doa *doa, void **weights, void **power, void **beams, int *nbeams);

/* vec [nest][m][m][2] of the last submit, as crsdr_noisesubspace writes it ([nest][ms][ms][2] with crsdr_doa_set_smoothing on, [nest][mv][mv][2]
 * with crsdr_doa_set_augment).
 * CRSDR_ESTATE before the first submit. */
int crsdr_doa_fetch_subspace(crsdr_doa *doa, float *vec);

/* Spatial smoothing and forward-backward averaging of the covariance, between the covariance and the subspace: coherent arrivals (an
 * emitter and its reflections) leave Rxx with one signal eigenvalue however many paths there are; averaging it over shifted sub-arrays
 * and with its backward image restores the rank.  Sub-arrays of sx x sy elements, 1 <= sx <= mx, 1 <= sy <= my, ms = sx * sy >= 2,
 * P = (mx - sx + 1)(my - sy + 1) of them; sub-array (px, py) selects sel_p(iy * sx + ix) = (iy + py) * mx + ix + px.  For a <= b, in
 * fp64 from the fp32 rxx, p running px fastest, then py:
 *     acc[a][b] = sum_p rxx[sel_p(a)][sel_p(b)]
 *     rs[a][b]  = acc[a][b] / P                                          flags = 0
 *     rs[a][b]  = (acc[a][b] + conj(acc[ms-1-a][ms-1-b])) / (2 P)        flags = CRSDR_SMOOTH_FB
 * rounded once to fp32, rs[b][a] written as its conjugate.  (Index reversal is the centro-symmetry of a URA in this element order; it
 * holds for the conjugated steering vectors of the X^H X convention alike.)
 * (sx, sy) = (mx, my) with flags 0 is "off".  With it on, the subspace, sv, vec, the scan (an sx x sy array of ms elements, the same
 * d), peak and the directions all work on rs: crsdr_doa_fetch's sv is [nest][ms], crsdr_doa_fetch_subspace's and the device's vec
 * [nest][ms][ms][2], densely packed; rxx (CRSDR_DOA_KEEP_RXX) stays the raw [m][m] matrix.  A submit is one launch more.
 * Any time: waits for the device if a submit was made, allocates rs, and discards what the last submit left (the fetch functions return
 * CRSDR_ESTATE until the next submit).  CRSDR_EINVAL for bad sizes or flags, for desc.k >= ms, or with crsdr_doa_set_order on and its
 * kmax >= ms.  While true sub-arrays (ms < m) are on, crsdr_doa_set_beams returns CRSDR_ESTATE, and with beams on this call does: the
 * weights are m-vectors and there is then no m x m subspace.  CRSDR_SMOOTH_FB alone keeps m, and beams work from its subspace. */
enum { CRSDR_SMOOTH_FB = 1u << 0 };
int crsdr_doa_set_smoothing(crsdr_doa *doa, int sx, int sy, uint32_t flags);

/* rs [nest][ms][ms][2] of the last submit.  CRSDR_ESTATE with smoothing off or before the first submit after crsdr_doa_set_smoothing. */
int crsdr_doa_fetch_smoothed(crsdr_doa *doa, float *rs);

/* The number of sources from the singular values, between the subspace and the scan.  M = the subspace's size (m, or ms with smoothing
 * on), N = frames * blocksize / 2 snapshots (the raw count with smoothing on as well: a definition, not a claim of optimality); in fp64
 * from the published fp32 sv:
 *     lambda_i = max(sv[i], sv[0] * 2^-40)
 *     T_k      = n log((1/n) sum_{i >= k} lambda_i) - sum_{i >= k} log lambda_i,   n = M - k,   for k in [kmin, kmax]
 *     CRSDR_ORDER_MDL   N T_k + k (2M - k) log(N) / 2
 *     CRSDR_ORDER_AIC   2 N T_k + 2 k (2M - k)
 * k_e = the argmin, the smallest k on a tie; sv[0] = 0 (an all-zero estimate): k_e = kmin and every value 0.
 * 1 <= kmin <= kmax < M: "no source", k = 0, is not representable, the scan needs one signal vector.
 * With it on, the scan of estimate e projects on columns k_e .. M-1 instead of desc.k .. M-1: its pm has the bits of an engine created
 * with k = k_e.  limit_directions != 0 with crsdr_doa_set_peaks on: found[e] <= k_e, the slots from there on hold (-1, -1) and -1, and
 * beams that follow the directions see the capped found.  A submit is one launch more.
 * CRSDR_ORDER_OFF frees the buffers (the other arguments are then ignored).  Any time: waits for the device if a submit was made.
 * CRSDR_EINVAL for a bad criterion or range. */
enum { CRSDR_ORDER_OFF = 0, CRSDR_ORDER_MDL = 1, CRSDR_ORDER_AIC = 2 };
int crsdr_doa_set_order(crsdr_doa *doa, int criterion, int kmin, int kmax, int limit_directions);

/* Waits for the last submit and copies out (either pointer may be NULL): k [nest] int32, criterion_values [nest][kmax - kmin + 1]
 * (the fp64 values rounded once to fp32).  CRSDR_ESTATE with order off or before the first submit after crsdr_doa_set_order. */
int crsdr_doa_fetch_order(crsdr_doa *doa, int32_t *k, float *criterion_values);

/* Device addresses of k and the criterion values ([max_batch / frames] estimates; NULL while order is off), for consumers on the same
 * stream.  They change with every crsdr_doa_set_order. */
int crsdr_doa_order_buffers(crsdr_doa *doa, void **k, void **criterion_values);

/* The per-op forms of the two steps: the same device functions, bit for bit.
 *   rxx [mx*my][mx*my][2] -> rs [sx*sy][sx*sy][2]        (sizes and flags as crsdr_doa_set_smoothing)
 *   sv [m], nsnap = N >= 1 -> k [1], criterion_values [kmax - kmin + 1] (NULL to skip)
 * mem_kind: CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE (every pointer on the device). */
int crsdr_smooth_covariance(float *rs, const float *rxx, int mx, int my, int sx, int sy, uint32_t flags, int mem_kind);
int crsdr_source_order(int32_t *k, float *criterion_values, const float *sv, int m, int64_t nsnap, int criterion, int kmin, int kmax,
                       int mem_kind);

/* One covariance per frequency band, in place of the one time-domain covariance per estimate: "which direction is the signal at THIS
 * frequency".  Per packet a signal row c holds L = blocksize / 2 samples x_c[n] = (I + jQ) / 127.  Each row is cut into J = L / nfft
 * segments of N = nfft samples (never across packets; an estimate has J' = frames * J), and with the window w
 *     X_c[j][f] = sum_n w[n] x_c[jN + n] exp(-2 pi i f n / N)                                    (the forward transform of crsdr_fft)
 *     R_f[a][b] = 1 / (J' N sum_n w[n]^2) * sum_j conj(X_a[j][f]) X_b[j][f]                      (the X^H X convention of crsdr_covariance)
 * CRSDR_WINDOW_RECT: w = 1, and sum_f R_f is the raw second moment (1/L') sum conj(x_a) x_b (Parseval).  CRSDR_WINDOW_HANN:
 * w[n] = 0.5 - 0.5 cos(2 pi n / N), periodic.  No mean is removed: a DC offset lands in bin 0 (Hann: bins 0 and +-1), and the caller
 * leaves those bands out.  Band i, 0 <= i < nbands, is the sum of R_f over the bins (first + i * width + u) mod N, u < width: FFT
 * order, negative frequencies in the upper half, and first may wrap.  power[i] = Re trace(R_band_i) / m, the squelch before a band's
 * direction is trusted.  The sums over j are fp32 per K slice of segments (a split that depends on blocksize and nfft alone: an
 * estimate has the same bits wherever it sits in a batch), the slices, the band's bins and the scale fp64, rounded once.
 * Limits: nfft a power of two in 8 .. 256, blocksize % (2 nfft) == 0, 0 <= first < nfft, nbands, width >= 1, nbands * width <= nfft,
 * (max_batch / frames) * nbands <= 4096.  CRSDR_EINVAL outside them.
 *
 * crsdr_doa_set_subbands: from the next submit on the band covariances replace the time-domain one (the same number of launches), and
 * every later step runs over nest * nbands matrices, estimate e's band i at index e * nbands + i: crsdr_doa_fetch (peak, peak_value, sv,
 * status, pm, rxx = the band matrices), crsdr_doa_fetch_subspace, the device buffers, and crsdr_doa_last_submit's nest all count
 * nest * nbands.  Directions, smoothing and the source count work per band (the count with N = J' * width snapshots) and size their
 * buffers by (max_batch / frames) * nbands, so the order is fixed: this call, on or off (nfft = 0; the other arguments are then ignored),
 * returns CRSDR_ESTATE while any of crsdr_doa_set_peaks, _set_beams, _set_subband_beams, _set_smoothing or _set_order is on, and
 * crsdr_doa_set_beams returns CRSDR_ESTATE while subbands are on (a band's weights applied to the wideband samples mean nothing: the
 * beams of the bands are crsdr_doa_set_subband_beams).  Waits for the device if a submit was made and discards what it left: the fetch
 * functions return CRSDR_ESTATE until the next submit. */
enum { CRSDR_WINDOW_RECT = 0, CRSDR_WINDOW_HANN = 1 };
int crsdr_doa_set_subbands(crsdr_doa *doa, int nfft, int first, int nbands, int width, int window);

/* Waits for the last submit and copies out power [nest][nbands].  CRSDR_ESTATE with subbands off or before the first submit after
 * crsdr_doa_set_subbands. */
int crsdr_doa_fetch_subbands(crsdr_doa *doa, float *power);

/* Device address of power ([max_batch / frames][nbands]; NULL while subbands are off), for consumers on the same stream.  It changes
 * with every crsdr_doa_set_subbands, as the addresses of crsdr_doa_device_buffers do. */
int crsdr_doa_subband_buffers(crsdr_doa *doa, void **power);

/* The per-op form on one packet's matrix [nrows][blocksize] (frames = 1): the same device functions, bit for bit.
 * rbands [nbands][m][m][2], power [nbands] or NULL, m = nrows - 1 in 2 .. 64.  mem_kind: CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE
 * (every pointer on the device; matrix and power 4-byte, rbands 8-byte aligned). */
int crsdr_subband_covariance(float *rbands, float *power, const int8_t *matrix, int nrows, int blocksize, int nfft, int first, int nbands,
                             int width, int window, int mem_kind);

/* A beam per frequency band toward each band's directions: with subbands on every (estimate e, band i) has its own subspace, peak and
 * directions, at matrix index e * nbands + i.  Per matrix and beam slot b: direction, steering vector, weights u (m complex, fp32) and
 * power exactly as crsdr_doa_set_beams defines them, from that matrix's vec, sv and peak / peaks / found (or the fixed angles); slots
 * b >= found: weights 0, power -1.  The weighted sum is taken of the rows' band spectra instead of their samples: with X_c[t][j][f]
 * the segment spectrum of signal row c of packet t as crsdr_doa_set_subbands defines it (samples (I + jQ) / 127, window w, forward
 * transform, N = nfft) and c_w = 1 / sqrt(N sum_n w[n]^2), for every packet t of estimate e, segment j < J = blocksize / (2 N) and u < width
 *     Y[t][i][b][j][u] = c_w sum_c u_{e,i,b}[c-1] X_c[t][j][(first + i width + u) mod N]
 * fp32 throughout, NO conjugate (the X^H X convention, argued at crsdr_doa_set_beams); empty slots: zeros, written.  c_w is the
 * normalisation behind R_f: the sum over all N bins of the mean |Y|^2 is the beam's mean sample power, and for one bin
 * mean_j |Y|^2 = u^H R_f u.  One narrowband IQ stream per (packet, band, slot): the band's channeliser output, `width` bins at J
 * samples per packet.
 *   beams [nblocks][nbands][nbeams][J][width][2] float: for width = 1 a (band, slot) stream is J contiguous complex samples per packet.
 * mode, loading, nfixed, fixed_angles and their ranges as crsdr_doa_set_beams (CRSDR_BEAM_OFF frees the buffers).  Any time: waits for
 * the device if a submit was made, then allocates weights [(max_batch / frames) * nbands][nbeams][m][2], power and the beams.  A submit
 * with them on is two launches more, the same for every nblocks, without allocation, lock or host wait.  With crsdr_doa_set_order's
 * limit_directions the beams see the capped found.
 * CRSDR_ESTATE while subbands are off, and while true sub-arrays (ms < m) are on (crsdr_doa_set_smoothing with true sub-arrays returns
 * CRSDR_ESTATE while these beams are on; CRSDR_SMOOTH_FB alone is fine).  While they are on crsdr_doa_set_subbands, on or off, returns
 * CRSDR_ESTATE, and while they follow the directions (nfixed = 0) crsdr_doa_set_peaks does.  crsdr_doa_set_beams, crsdr_doa_fetch_beams
 * and crsdr_doa_beam_buffers keep to the wideband beams: these beams are not theirs.  CRSDR_EINVAL as crsdr_doa_set_beams. */
int crsdr_doa_set_subband_beams(crsdr_doa *doa, int mode, float loading, int nfixed, const float *fixed_angles);

/* Waits for the last submit and copies out (any pointer may be NULL): weights [nest * nbands][nbeams][m][2], power [nest * nbands][nbeams],
 * beams as above.  CRSDR_ESTATE with these beams off or before the first submit after crsdr_doa_set_subband_beams. */
int crsdr_doa_fetch_subband_beams(crsdr_doa *doa, float *weights, float *power, float *beams);

/* Device addresses of weights, power and beams (laid out as above for (max_batch / frames) * nbands matrices and max_batch blocks; NULL
 * while these beams are off) and the slot count, for consumers on the same stream.  They change with every crsdr_doa_set_subband_beams. */
int crsdr_doa_subband_beam_buffers(crsdr_doa *doa, void **weights, void **power, void **beams, int *nbeams);

/* The per-op form on one packet's matrix [nrows][blocksize]: the same device function as the batched kernel, bit for bit.
 *   weights [nbands][nbeams][nrows-1][2] float, 1 <= nbeams <= 16;  out [nbands][nbeams][J][width][2] float
 * nrows, blocksize, nfft, first, nbands, width, window as crsdr_subband_covariance; every argument is checked before a device is
 * touched.  mem_kind: CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE (all three on the device: matrix 4-byte, weights and out 8-byte aligned). */
int crsdr_subband_beamform(float *out, const int8_t *matrix, int nrows, int blocksize, int nfft, int first, int nbands, int width, int window,
                           const float *weights, int nbeams, int mem_kind);

/* Two power maps beside the MUSIC pseudo-spectrum, over the same grid: MUSIC needs the number of sources beforehand, has no unit and
 * cannot say how strong an arrival is; these are in power units ((I + jQ) / 127)^2 and use no source count.
 *   M       the size of the subspace: m, or ms while crsdr_doa_set_smoothing runs true sub-arrays (the array is then sx x sy)
 *   v_r     column r of the published fp32 vec, sv the published fp32 values
 *   a       the steering vector of crsdr_pmusic2d at alpha = cx pi / ncx, beta = cy pi / ncy, evaluated in fp32 with that call's
 *           expressions in their order: a grid point is the same direction in all three maps
 *   y_r     = v_r^H a = sum_i conj(vec[i][r]) a[i], for ALL r = 0 .. M-1, fp32
 *   w_r     fp64 from the fp32 sv, rounded once to fp32 (as the beams' power is formed):
 *           CRSDR_SPECTRUM_BARTLETT  w_r = sv[r] / M^2
 *           CRSDR_SPECTRUM_CAPON     delta = (double)loading * sv[0],  w_r = 1 / (sv[r] + delta)
 *   S       = sum_r w_r |y_r|^2 in fp32, r ascending
 *   pm      BARTLETT: S = a^H R a / M^2, the power a delay-and-sum beam toward the grid point receives (crsdr_doa_set_beams'
 *           conventional power); CAPON: 1 / S = 1 / a^H (R + delta I)^-1 a, the MVDR beam's power: adaptive side-lobe suppression,
 *           close sources resolved.
 * sv[0] == 0 (an all-zero estimate): pm = 0 at every grid point, for both kinds.  Otherwise w_r >= 0 with w_0 > 0: CAPON has every w_r > 0 and
 * sum_r |y_r|^2 = M, so S > 0 and 1 / S is finite; BARTLETT on a rank-deficient estimate has w_r = 0 behind the rank, and S = 0 where a is
 * orthogonal to the signal columns.  Neither kind gives a negative or NaN pm from finite input, and the keys of peak and crsdr_doa_set_peaks order it like the value.
 * loading in [1e-6, 1] for CAPON (the range of crsdr_doa_set_beams), ignored otherwise.
 *
 * crsdr_doa_set_spectrum: from the next submit on the scan computes the chosen map in place of MUSIC's, and everything behind it works
 * on that map: pm (CRSDR_DOA_KEEP_SPECTRUM), peak / peak_value, the local maxima of crsdr_doa_set_peaks and their values, the beams and
 * band beams that follow the directions, limit_directions.  Smoothing and subbands feed it as they feed MUSIC: per (estimate, band),
 * with the sub-arrays' M.  desc.k and crsdr_doa_set_order's k_e are ignored by BARTLETT and CAPON (the order is still computed, fetched
 * and applied to found under limit_directions).  The scan's kernel is replaced, not added: a submit issues the launches it issued before.
 * CRSDR_SPECTRUM_MUSIC restores the MUSIC scan, bit for bit.  Any time: waits for the device if a submit was made and discards what it
 * left (every fetch function returns CRSDR_ESTATE until the next submit); allocates nothing, and no other setter refuses or is refused
 * because of it.  CRSDR_EINVAL for a bad kind, or for loading outside the range with CAPON. */
enum { CRSDR_SPECTRUM_MUSIC = 0, CRSDR_SPECTRUM_BARTLETT = 1, CRSDR_SPECTRUM_CAPON = 2 };
int crsdr_doa_set_spectrum(crsdr_doa *doa, int kind, float loading);

/* The per-op form: the same device function as the batched scan, bit for bit.  BARTLETT and CAPON only (MUSIC is crsdr_pmusic2d).
 *   vec [m][m][2] and sv [m] as crsdr_noisesubspace writes them, 2 <= m = mx * my <= 64;  pm [ncx][ncy] float row-major
 * Every argument is checked before a device is touched.  mem_kind: CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE (all three on the
 * device: vec 8-byte, sv and pm 4-byte aligned). */
int crsdr_spectrum2d(float *pm, const float *vec, const float *sv, int m, int kind, float loading, float d, int mx, int my, int ncx, int ncy,
                     int mem_kind);

/* Directions off the scan grid.  Every direction above is a grid index (cx, cy): on a 100 x 100 grid 1.8 degrees per step, where the
 * array and the data carry far more.  The refinement is an fp64 zoom search for the maximum of the same map between the grid points:
 * no derivatives, no iteration to convergence, the same 49 points per level whatever the data.
 *   input   one matrix (vec, sv as published, of size M = sx * sy while smoothing runs sub-arrays), one of its directions (cx, cy),
 *           levels L in 1 .. 8
 *   x, y    cell coordinates (doubles), alpha = x pi / ncx, beta = y pi / ncy; the steering vector is the beam weights' fp64 expression
 *           ph_i = 2 pi (double)d (ix cos(alpha) sin(beta) + iy cos(beta)), a_i = (cos ph_i, sin ph_i)
 *   f(x, y) the map the object's scan computes, in fp64 from the fp32 vec / sv, y_r = v_r^H a:
 *           MUSIC     (M / sum_{r >= k_e} |y_r|^2)^2, k_e the object's k or, with crsdr_doa_set_order, the estimate's count
 *           BARTLETT  S,  CAPON 1 / S,  S = sum_r w_r |y_r|^2 with the w_r of crsdr_doa_set_spectrum in fp64, not rounded to fp32
 *           sv[0] == 0: f = 0
 *   x = cx, y = cy, s = 1/2
 *   repeat L times:
 *       c = f(x, y); best = c; (bx, by) = (x, y)
 *       for i in -3..3, for j in -3..3 (row-major, i major), (i, j) != (0, 0):
 *           px = min(max(x + i s, 0), ncx); py = min(max(y + j s, 0), ncy);  v = f(px, py)
 *           if v > c and v > best: best = v; (bx, by) = (px, py)
 *       (x, y) = (bx, by); s = s / 4
 * The comparison is strict: the centre keeps ties, a NaN never wins, the lowest index wins equal values.  Level l spans +-3 s_l, the
 * next +-(3/4) s_l around a point at most s_l / 2 from the maximum of a locally unimodal map: a near-tie between neighbouring lattice
 * points does not lose the maximum.  |x - cx| < 2, and every coordinate is a multiple of 2^-(2L - 1): the offsets are exact in float.
 * The definition does not pin the order of the fp64 operations inside f.
 *
 * crsdr_doa_set_refine: levels = 0 off, 1 .. 8 on.  From the next submit on, one more launch behind the directions and ahead of the beams
 * refines every direction of every matrix (estimate, or estimate and band): the `count` slots of crsdr_doa_set_peaks, or the one peak
 * while they are off.  Beams that follow the directions (nfixed = 0, wideband and band beams) then steer at the refined direction;
 * beams at fixed angles are untouched.  Works with smoothing, the source count, subbands and all three maps.  Any time: waits for the
 * device if a submit was made; allocates for the most matrices and slots there can be, so no other setter refuses or is refused because
 * of it.  With levels = 0 a submit issues the launches and computes the bits it did before the call.
 * crsdr_doa_fetch_refined (any pointer NULL = skip), per matrix and slot of the last submit (its own slot count, whatever
 * crsdr_doa_set_peaks was called with since):
 *   offsets [nest][slots][2] float  (x - cx, y - cy) in grid cells, exact
 *   angles  [nest][slots][2] float  (alpha, beta) in radians, rounded once from fp64: the convention of fixed_angles
 *   values  [nest][slots]    float  f at the refined point
 * Empty slots (from found on) hold (0, 0), (-1, -1) and -1.  CRSDR_ESTATE without crsdr_doa_set_refine, or before the first submit after it.
 * crsdr_doa_refined_buffers: the device addresses (NULL while off), and the slots per matrix a fetch would read. */
int crsdr_doa_set_refine(crsdr_doa *doa, int levels);
int crsdr_doa_fetch_refined(crsdr_doa *doa, float *offsets, float *angles, float *values);
int crsdr_doa_refined_buffers(crsdr_doa *doa, void **offsets, void **angles, void **values, int *slots);

/* The per-op form: the same kernel on one matrix, bit for bit.
 *   vec [m][m][2] and sv [m] as crsdr_noisesubspace writes them, 2 <= m = mx * my <= 64;  kind CRSDR_SPECTRUM_*; k: the sources (MUSIC:
 *   1 <= k < m, ignored otherwise); loading: CAPON's, in [1e-6, 1];  peaks [npeaks][2] int32 (cx, cy), 1 <= npeaks <= 16 (a direction
 *   outside [0, ncx] x [0, ncy] is an empty slot);  levels 1 .. 8;  offsets, angles [npeaks][2], values [npeaks]
 * Every argument is checked before a device is touched.  mem_kind: CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE (all on the device: vec
 * 8-byte, the others 4-byte aligned). */
int crsdr_refine2d(float *offsets, float *angles, float *values, const float *vec, const float *sv, int m, int kind, int k, float loading, float d, int mx,
                   int my, int ncx, int ncy, const int32_t *peaks, int npeaks, int levels, int mem_kind);

/* Gridless directions: 2-D ESPRIT.  Every direction above comes from a scan over ncx x ncy grid points.  On a uniform rectangular
 * array the k directions can be read from the shift invariance of the signal subspace instead: no grid, no search, no peak picking,
 * k-by-k linear algebra per matrix whatever the grid is, and sources that merge into one local maximum of a map stay k directions.
 * The definition, per matrix (an estimate, or an estimate and band).  Inputs: the published fp32 vec ([M][M], column r = v_r) and sv;
 * the source count k_e (desc.k, or the matrix's count from crsdr_doa_set_order); the array SX x SY, M = SX SY (the sub-array while
 * smoothing runs true sub-arrays, mx x my otherwise), element i = iy SX + ix; (double)d.  All arithmetic is fp64, its order not pinned.
 *   1. E = the first k_e columns of vec, M x k
 *   2. E1x = the rows of E with ix <= SX-2, E2x those with ix >= 1, paired (ix, iy) -> (ix+1, iy)
 *   3. E1y, E2y likewise with iy <= SY-2 and iy >= 1
 *   4. Gx = E1x^H E1x, Hx = E1x^H E2x (k x k), Psi_x = Gx^-1 Hx by Cholesky; Psi_y likewise
 *   5. Psi_c = Psi_x + gamma Psi_y, gamma = (1 + j) / 2
 *   6. Psi_c V = V diag(w), V the eigenvectors of Psi_c; lambda_x_i = (V^-1 Psi_x V)_ii, lambda_y_i = (V^-1 Psi_y V)_ii.  This pairs mu
 *      with nu, and is unique for distinct w_i whatever the order or scaling of V (the diagonal of a Schur form's Q^H Psi_x Q is not)
 *   7. mu_i = atan2(Im lambda_x_i, Re lambda_x_i), nu_i = atan2(Im lambda_y_i, Re lambda_y_i)
 *   8. the angles in the scan's convention, a_i = exp(j (ix mu + iy nu)), mu = 2 pi d cos(alpha) sin(beta), nu = 2 pi d cos(beta):
 *      cb = nu / (2 pi d), clamped to [-1, 1] with flag bit 0 if |cb| > 1;  sb = sqrt(1 - cb^2);  ca = sb > 0 ? mu / (2 pi d sb) : 0,
 *      clamped with flag bit 1 if sb == 0 or |ca| > 1;  beta = acos(cb), alpha = acos(ca).  The covariance is X^H X, so this is the
 *      direction at which MUSIC peaks for the same source (the mirrored one); nothing is conjugated.  For d > 1/2 the principal value
 *      of mu and nu is the alias nearest broadside: a source beyond it is reported at that alias.
 *   9. power_i = sum_r sv[r] |v_r^H a_i|^2 / M^2, a_i the fp64 steering vector of the beam weights at (alpha_i, beta_i): the
 *      conventional power of crsdr_doa_set_beams
 *  10. slots by descending power; equal powers by ascending mu, then nu
 *  11. found = k_e; 0 if sv[0] == 0 (status 0), if a Cholesky pivot (the diagonal entry a column starts from) is <= 2^-40 (status bit 1),
 *      or if the eigenvalue iteration did not finish within 40 k_e steps (status bit 0)
 *  12. slots from found on hold phases (0, 0), angles (-1, -1), modulus (-1, -1), power -1 and flags 0
 * Needs SX >= 2 and SY >= 2; slots = desc.k, or kmax with crsdr_doa_set_order; slots <= 16 and slots <= min((SX-1) SY, SX (SY-1)).
 * These are checked when the feature is used (by a submit: CRSDR_ESTATE before any launch), not by other setters.
 *
 * crsdr_doa_set_esprit: CRSDR_ESPRIT_OFF; CRSDR_ESPRIT_BESIDE: one launch more per submit, between the source count and the scan,
 * everything else unchanged; CRSDR_ESPRIT_ONLY: that launch, and the scan, the peak, the local peaks and the refinement are not issued.
 * After an ONLY submit crsdr_doa_fetch with a non-NULL peak, peak_value or pm answers CRSDR_ESTATE, as do crsdr_doa_fetch_directions
 * and crsdr_doa_fetch_refined; sv, status, rxx, the subspace, the smoothed matrix, the order and the band powers fetch as ever.  A
 * submit in ONLY mode with crsdr_doa_set_peaks, crsdr_doa_set_refine or beams that follow the directions (nfixed = 0, wideband or band)
 * on answers CRSDR_ESTATE before any launch; beams at fixed angles are fine (the fetched angles are in their convention).
 * Any time: waits for the device if a submit was made; allocates for the most matrices and slots there can be, so no other setter
 * refuses or is refused because of it.  CRSDR_EINVAL for another mode.  With OFF a submit issues the launches and computes the bits
 * it did before the call.
 * crsdr_doa_fetch_esprit (any pointer NULL = skip), per matrix of the last submit and its slots:
 *   found, status [nest] int32;  phases [nest][slots][2] double (mu, nu);  angles [nest][slots][2] float (alpha, beta), rounded once;
 *   modulus [nest][slots][2] float (|lambda_x|, |lambda_y|), about 1 for a plane wave: the quality figure;  power [nest][slots] float;
 *   flags [nest][slots] int32
 * CRSDR_ESTATE while off, or before the first submit after the setter.
 * crsdr_doa_esprit_buffers: the device addresses (NULL while off) and the slots per matrix a fetch would read. */
enum { CRSDR_ESPRIT_OFF = 0, CRSDR_ESPRIT_BESIDE = 1, CRSDR_ESPRIT_ONLY = 2 };
int crsdr_doa_set_esprit(crsdr_doa *doa, int mode);
int crsdr_doa_fetch_esprit(crsdr_doa *doa, int32_t *found, int32_t *status, double *phases /*[nest][slots][2] (mu, nu)*/,
                           float *angles /*[nest][slots][2] (alpha, beta), rounded once*/, float *modulus /*(|lambda_x|, |lambda_y|)*/,
                           float *power, int32_t *flags);
int crsdr_doa_esprit_buffers(crsdr_doa *doa, void **found, void **status, void **phases, void **angles, void **modulus,
                             void **power, void **flags, int *slots);

/* The per-op form: the same arithmetic on one matrix, bit for bit; slots = k.
 *   vec [m][m][2] and sv [m] as crsdr_noisesubspace writes them, m = mx * my <= 64, mx >= 2, my >= 2;  1 <= k <= 16 and
 *   k <= min((mx-1) my, mx (my-1));  found, status one int32 each;  phases [k][2] double;  angles, modulus [k][2];  power, flags [k]
 * Every argument is checked before a device is touched.  mem_kind: CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE (all on the device: vec
 * and phases 8-byte, the others 4-byte aligned). */
int crsdr_esprit2d(int32_t *found, int32_t *status, double *phases, float *angles, float *modulus, float *power, int32_t *flags,
                   const float *vec, const float *sv, int m, int k, float d, int mx, int my, int mem_kind);

/* Co-array augmentation, between the covariance and the subspace: thinned arrays and dead receivers.  Every step behind the
 * covariance assumes a filled mx x my array whose receivers all work.  From the receivers that are present, the covariance is averaged
 * per spatial lag, and the covariance of a filled virtual array is rebuilt from the averages; everything downstream runs on that.
 * With all receivers present it is the redundancy-averaged (block-Toeplitz) covariance estimate.
 *   Physical array  mx x my, element i = iy * mx + ix, m = mx * my <= 64.
 *   Mask            bit i set: element i is present.  mask == 0: all m elements.  Otherwise no bit from m on, at least two bits set.
 *   Virtual array   vx x vy, 1 <= vx <= mx, 1 <= vy <= my, mv = vx * vy >= 2, element j = jy * vx + jx.
 *   Lags            u = (ux, uy) of the half-plane: uy > 0, or uy == 0 and ux >= 0, with |ux| < vx and uy < vy.  For virtual indices
 *                   a <= b the lag pos_b - pos_a always lies in it.  P(u) = the pairs (p, q) of present physical elements with
 *                   (ix_q - ix_p, iy_q - iy_p) = u, by ascending p (q is then determined, and q >= p: only the upper triangle of rxx
 *                   is read); c(u) = |P(u)|.  Every half-plane lag needs c(u) >= 1: otherwise CRSDR_EINVAL, the text naming the first
 *                   uncovered lag.
 * In fp64 from the fp32 rxx, in that order:
 *     r(u)     = (1 / c(u)) sum_{(p, q) in P(u)} rxx[p][q]
 *     ra[a][b] = r(pos_b - pos_a)        for a <= b
 * each value rounded once to fp32, the diagonal's imaginary part exactly 0, ra[b][a] written as the conjugate.  Rows and columns of
 * absent elements are never read: they may hold anything.
 * For R = A P A^H + sigma^2 I with diagonal P (incoherent sources) the result is exactly the covariance of the filled vx x vy array,
 * whatever the mask.  Coherent sources need smoothing instead, and the two do not combine (below).  The matrix is Hermitian
 * block-Toeplitz but not guaranteed positive semidefinite: the subspace step takes singular values (in the 7 x 3 scenes of the tests
 * the most negative eigenvalue stays below 0.6 % of the last signal value).  Spatially smoothing the co-array vector would give
 * ra^2 / P, which has the same vectors: that is why this is the whole step.  (The upstream clients' DA2D orders the 2-D lags along one
 * dimension and fills a Toeplitz matrix, which is the covariance of no array: parity unpinned.)
 *
 * crsdr_doa_set_augment: vx = 0 turns it off (the other arguments are then ignored).  On: from the next submit one launch more, and
 * the subspace, sv, vec, the source count (M = mv, the raw N: a definition, as on smoothing's sub-arrays), every map, peak, the
 * directions, the refinement and ESPRIT work on ra as a vx x vy array of M = mv elements with the same d: crsdr_doa_fetch's sv is
 * [nest][mv], vec [nest][mv][mv][2]; rxx (CRSDR_DOA_KEEP_RXX) stays the raw [m][m].  With subbands on it runs per (estimate, band).
 * Any time: waits for the device if a submit was made, allocates ra, and discards what the last submit left (every fetch answers
 * CRSDR_ESTATE until the next submit).  CRSDR_EINVAL for bad sizes, a bad mask, an uncovered lag, desc.k >= mv, or with
 * crsdr_doa_set_order on and its kmax >= mv.  CRSDR_ESTATE, both ways round, with crsdr_doa_set_smoothing (a Hermitian block-Toeplitz
 * matrix is persymmetric already and all its sub-array blocks are equal: smoothing it is a no-op) and with crsdr_doa_set_beams /
 * _set_subband_beams (the subspace is the virtual array's: weights from it are not the physical rows').  crsdr_doa_set_subbands answers
 * CRSDR_ESTATE while it is on: ra is sized by the bands.
 * crsdr_doa_fetch_augmented: ra [nest][mv][mv][2] of the last submit; CRSDR_ESTATE while off or before the first submit after the setter.
 * crsdr_doa_augment_buffers: the device address of ra (NULL while off) and the virtual shape (0, 0 while off). */
int crsdr_doa_set_augment(crsdr_doa *doa, int vx, int vy, uint64_t mask);
int crsdr_doa_fetch_augmented(crsdr_doa *doa, float *ra);
int crsdr_doa_augment_buffers(crsdr_doa *doa, void **ra, int *vx, int *vy);

/* The per-op form: the same device function, bit for bit.  rxx [mx*my][mx*my][2] -> ra [vx*vy][vx*vy][2], sizes and mask as above.
 * Every argument is checked before a device is touched.  mem_kind: CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE (both on the device,
 * 8-byte aligned). */
int crsdr_augment_covariance(float *ra, const float *rxx, int mx, int my, int vx, int vy, uint64_t mask, int mem_kind);

/* The lag counts, pure host arithmetic (no device needed): to plan a thinning, or to decide whether the array survives a dead receiver.
 * counts [vy][2 vx - 1] (may be NULL) takes c(u) at [uy][ux + vx - 1]; row 0's negative ux hold the mirrored count c(-ux, 0).
 * *uncovered (may be NULL) = the number of half-plane lags with c(u) = 0: the call itself returns CRSDR_OK then, CRSDR_EINVAL only for
 * bad sizes or a bad mask.  The setter and the per-op call check with the same function. */
int crsdr_augment_lags(int mx, int my, int vx, int vy, uint64_t mask, int32_t *counts /* [vy][2vx-1], may be NULL */, int *uncovered);

/* ------------------------------------------------------------------------------------------
 * (v) Welch spectra and reference cross-spectra of the packets: a third packet consumer, beside the plan's fetches and crsdr_doa
 * ---------------------------------------------------------------------------------------- */

/* What the reference's clients do beside MUSIC (matlabclient/testchannels.m: a power spectrum per channel;
 * matlabclient/seqnum_and_correlation.m: every column against column 1), on the device and on the packets AS PUBLISHED -- behind
 * the shift, the rotation, the fractional-delay pass and the canceller.  For any number of rows; row 0, the reference channel, is a row
 * like every other here.
 *
 * Input.  A packet's matrix is [nrows][B] int8; row c holds L = B / 2 samples x_c[n] = (I + jQ) / 127, c = 0 .. nrows - 1.  N = nfft, the
 * hop is H = N (overlap 0) or H = N / 2 (overlap 1); a packet has J = (L - N) / H + 1 segments, segment j starting at sample jH:
 * segments never cross packets.  A line e is `frames` consecutive packets, J' = frames * J segments.
 * Window.  w = CRSDR_WINDOW_RECT or CRSDR_WINDOW_HANN (periodic, as in crsdr_doa_set_subbands).
 * Spectra.
 *     X_c[t][j][f] = sum_n w[n] x_c[jH + n] exp(-2 pi i f n / N)             (crsdr_fft's forward transform, FFT bin order)
 *     P_c[f] = 1 / (J' N sum w^2) * sum_{t,j} |X_c[t][j][f]|^2                  psd   [nest][nrows][N]    float
 *     S_c[f] = 1 / (J' N sum w^2) * sum_{t,j} conj(X_0[t][j][f]) X_c[t][j][f]   cross [nest][nrows][N][2] float
 * the X^H X convention and the normalisation of crsdr_doa_set_subbands (P_c[f] is the diagonal of its R_f).  No mean is removed: DC
 * lands in bin 0.  S_0[f] = (P_0[f], 0), the imaginary part written as exactly 0.
 * Alignment figures, over the band of signed bins s_i = band_lo + i, i < K = band_hi - band_lo + 1, bin f_i = s_i mod N; all in fp64
 * from the published fp32 P and S, each figure rounded once to fp32 (the order of the fp64 operations is not pinned):
 *     A         = sum_{i < K-1} S_c[f_{i+1}] conj(S_c[f_i])
 *     delay     = -atan2(Im A, Re A) * N / (2 pi)                  samples; 0 if A == 0     (row c = row 0 delayed by `delay`)
 *     z         = sum_i S_c[f_i] exp(+2 pi i s_i delay / N)
 *     phase     = atan2(Im z, Re z)                                 radians at DC with the delay taken out
 *     gain      = |z| / sum_i P_0[f_i]                              0 if the denominator is 0
 *     coherence = min(1, sum_i |S_c[f_i]|^2 / sum_i P_0[f_i] P_c[f_i])   0 if the denominator is 0; it is 1 for J' = 1 (one segment
 *                                                                   is coherent with anything): average over segments to learn something
 *     align [nest][nrows][4] float = (delay, phase, gain, coherence)
 * Row 0 is computed like every other row and gives (0, 0, 1, 1) for a non-zero reference.  An all-zero packet gives zeros everywhere,
 * never a NaN.  (Parity: unpinned by the reference, whose script only plots correlations.)
 * Bits.  The sums over a packet's segments run in fp32 chains of at most 32 terms whose split depends on (blocksize, nfft, overlap)
 * alone; the chains, the packets of a line and the scale are fp64 with one rounding.  Hence a line has the same bits wherever it
 * sits in a batch and whatever nblocks is, and crsdr_welch equals the batched engine bit for bit.
 *
 * Limits, all CRSDR_EINVAL and all checked before a device is touched: nfft a power of two in 16 .. 4096; blocksize a multiple of
 * 2 nfft (up to 2^22, as a plan's); nrows >= 2; 1 <= frames <= max_batch <= 64 (0 = 1 for both); (max_batch / frames) * nrows * nfft
 * <= 2^24; overlap 0 or 1; a valid window; -nfft/2 <= band_lo < band_hi <= nfft/2 - 1.
 *
 * Every buffer is allocated by crsdr_spectra_create.  A submit is asynchronous on its stream: three kernel launches whatever the
 * number of blocks, no allocation, no process-wide lock, nothing that waits for the device. */
typedef struct crsdr_spectra crsdr_spectra;

typedef struct crsdr_spectra_desc {
    int32_t nrows, blocksize; /* of the packets it reads (as in crsdr_plan_desc) */
    int32_t device;
    int32_t max_batch;        /* blocks per submit, 1..64 (0 = 1) */
    int32_t frames;           /* consecutive blocks per line, 1..max_batch (0 = 1) */
    int32_t nfft;
    int32_t overlap;          /* 0: hop nfft, 1: hop nfft / 2 */
    int32_t window;           /* CRSDR_WINDOW_* */
    int32_t band_lo, band_hi; /* the alignment figures' band, signed bins */
} crsdr_spectra_desc;

int crsdr_spectra_create(crsdr_spectra **spectra, const crsdr_spectra_desc *desc);
int crsdr_spectra_destroy(crsdr_spectra *spectra);

/* nblocks packets on the object's device, packet t at device_packets + t * packet_stride, its matrix [nrows][blocksize] int8 at
 * + matrix_offset (4-byte aligned, like packet_stride); 1 <= nblocks <= max_batch, nblocks % frames == 0.  Asynchronous on hip_stream
 * (NULL = the object's own stream); the packets must stay valid until the work has run.  One submit at a time: the next one reuses
 * the buffers of this one, so fetch (or order the streams) in between. */
int crsdr_spectra_submit(crsdr_spectra *spectra, const void *device_packets, size_t packet_stride, size_t matrix_offset, int nblocks,
                         void *hip_stream);

/* The plan's last submitted batch, where its packets are (own buffer or crsdr_plan_bind_packet), on the plan's stream: ordered
 * behind that batch by the stream alone, no host wait in between.  CRSDR_ESTATE for a plan with nothing submitted or with a slab
 * bound (the matrix is then not in the packet); CRSDR_EINVAL for another geometry or device, or a batch that is not a multiple of
 * `frames` or exceeds max_batch. */
int crsdr_spectra_submit_plan(crsdr_spectra *spectra, crsdr_plan *plan);

/* Waits for the last submit and copies out what is asked for (any pointer may be NULL); nest = nblocks / frames.  psd, cross and align
 * as laid out above.  CRSDR_ESTATE before the first submit. */
int crsdr_spectra_fetch(crsdr_spectra *spectra, float *psd, float *cross, float *align);

/* Device addresses of the results ([max_batch / frames] lines each, laid out as above), for consumers on the same stream. */
int crsdr_spectra_device_buffers(crsdr_spectra *spectra, void **psd, void **cross, void **align);

/* Of the last submit: the number of lines (what crsdr_spectra_fetch will write) and the kernel launches it issued (the same for
 * every nblocks).  Either pointer may be NULL.  CRSDR_ESTATE before the first submit. */
int crsdr_spectra_last_submit(crsdr_spectra *spectra, int *nest, int *launches);

/* The per-op form on one packet's matrix [nrows][blocksize] (frames = 1): the same kernels on the same arguments, bit for bit.
 * psd [nrows][nfft], cross [nrows][nfft][2], align [nrows][4]; any of the three may be NULL, not all.  nrows * nfft <= 2^24.
 * mem_kind: CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE (every pointer on the device; matrix, psd and align 4-byte, cross 8-byte
 * aligned). */
int crsdr_welch(float *psd, float *cross, float *align, const int8_t *matrix, int nrows, int blocksize, int nfft, int overlap, int window,
                int band_lo, int band_hi, int mem_kind);

/* ------------------------------------------------------------------------------------------
 * (w) Range-Doppler maps of the packets against a chosen row: a fourth packet consumer (passive radar)
 * ---------------------------------------------------------------------------------------- */

/* Sections (iii) and (v) treat the rows as stationary: a direction, a spectrum, one residual delay per row.  This one takes one row as
 * an illuminator's reference and correlates every row against it over delay AND Doppler (the cross-ambiguity function), on the device
 * and on the packets AS PUBLISHED, behind the plan by stream order alone, as (v) does.  The complex value of one cell across the rows
 * is the snapshot a per-target direction estimate needs.
 *
 * Input.  As in (v): a packet's matrix is [nrows][B] int8; row c holds L = B / 2 samples, used here as the INTEGERS X_c[n] = I + jQ.
 * Parameters.  seg = Ls, nlags = R, ref_row = r (any row; row 0 is a row like every other), frames, window, guard.
 * Segments.  A packet has J = L / Ls segments; segments never cross packets.  A line is `frames` consecutive packets; the slow-time
 * index is k = t J + j < nd = frames J.
 * Range stage, exact in int32 on the real and imaginary parts:
 *     y_c[k][tau] = sum_{n < Ls} X_c[t][j Ls + n] conj(X_r[t][j Ls + n - tau]),   tau = 0 .. R - 1,   X_r[t][m] = 0 for m < 0
 * The reference never reaches into the previous packet: only the first segment of a packet sees the zeros.  |y| <= 2^15 Ls <= 2^27,
 * so it cannot overflow, with every byte -128 included.
 * Doppler stage.  w is CRSDR_WINDOW_RECT or CRSDR_WINDOW_HANN (periodic) OVER k, as in crsdr_doa_set_subbands; the forward transform
 * is that of crsdr_fft, in FFT bin order.  The integers are converted to fp32 with one rounding, multiplied by the fp32 window and
 * transformed in fp32; the scale is applied once:
 *     chi_c[d][tau] = 1 / (127^2 Ls sum_k w[k]) * sum_k w[k] y_c[k][tau] exp(-2 pi i d k / nd)     chi [nest][nrows][nd][R][2] float, tau fastest
 * Array map.  map [nest][nd][R] float = sum_{c != r} |chi_c[d][tau]|^2, from the published fp32 chi in fp64, rounded once; the order of
 * the sum is not pinned.
 * Peaks.  peak [nest][nrows + 1][6] float.  Entry c < nrows is taken from P_c = re^2 + im^2 of the published fp32 chi, evaluated in
 * fp64; entry nrows from the published map.  s(d) = d for d < nd / 2, else d - nd.  The searched set is S = {(d, tau): |s(d)| >= guard}:
 * guard = 0 searches everything, guard = g cuts the zero-Doppler ridge of width 2 g - 1.  The six figures, each rounded once to fp32:
 *     lag, doppler = tau*, s(d*)      the first maximum in the order of the linear index d R + tau
 *     power        = P*
 *     ratio        = P* / mean of P over S                                    0 if that mean is 0
 *     dlag         = 0.5 (P- - P+) / (P- - 2 P* + P+) from the cells (d*, tau* -+ 1); 0 when tau* is 0 or R - 1, 0 when the denominator
 *                    is >= 0; clamped to [-0.5, 0.5]
 *     ddop         = the same formula from the cells (d* -+ 1 mod nd, tau*); 0 if either neighbour is outside S, 0 when the
 *                    denominator is >= 0
 * Where P* = 0 (every searched cell is zero) the position means nothing and all six figures are 0: an all-zero packet gives zeros
 * everywhere, never a NaN.  (Parity: unpinned by the reference, which has no such client.)
 * Bits.  Nothing in a line depends on the other lines or on nblocks: a line has the same bits wherever it sits in a batch, and
 * crsdr_ambiguity launches the same kernels on the same arguments and equals the engine bit for bit.
 *
 * Limits, all CRSDR_EINVAL and all checked before a device is touched, by one function for the engine and the per-op call: seg a power
 * of two in 16 .. 4096; blocksize a multiple of 2 seg (up to 2^22, as a plan's); nrows >= 2; 0 <= ref_row < nrows;
 * 1 <= nlags <= min(seg, 1024); 1 <= frames <= max_batch <= 64 (0 = 1 for both); nd a power of two in 8 .. 4096;
 * (max_batch / frames) * nrows * nd * nlags <= 2^24; a valid window; 0 <= guard <= nd / 2.
 *
 * Every buffer and table is made by crsdr_caf_create.  A submit is asynchronous on its stream: three kernel launches whatever the
 * number of blocks, no allocation, no process-wide lock, nothing that waits for the device. */
typedef struct crsdr_caf crsdr_caf;

typedef struct crsdr_caf_desc {
    int32_t nrows, blocksize; /* of the packets it reads (as in crsdr_plan_desc) */
    int32_t device;
    int32_t max_batch;        /* blocks per submit, 1..64 (0 = 1) */
    int32_t frames;           /* consecutive blocks per line, 1..max_batch (0 = 1) */
    int32_t seg;              /* samples per segment (fast time) */
    int32_t nlags;            /* lags 0 .. nlags - 1 */
    int32_t ref_row;          /* the row every row is correlated against */
    int32_t window;           /* CRSDR_WINDOW_*, over slow time */
    int32_t guard;            /* the peak search skips |Doppler| < guard */
} crsdr_caf_desc;

int crsdr_caf_create(crsdr_caf **caf, const crsdr_caf_desc *desc);
int crsdr_caf_destroy(crsdr_caf *caf);

/* nblocks packets on the object's device, packet t at device_packets + t * packet_stride, its matrix [nrows][blocksize] int8 at
 * + matrix_offset (4-byte aligned, like packet_stride); 1 <= nblocks <= max_batch, nblocks % frames == 0.  Asynchronous on hip_stream
 * (NULL = the object's own stream); the packets must stay valid until the work has run.  One submit at a time: the next one reuses
 * the buffers of this one, so fetch (or order the streams) in between. */
int crsdr_caf_submit(crsdr_caf *caf, const void *device_packets, size_t packet_stride, size_t matrix_offset, int nblocks, void *hip_stream);

/* The plan's last submitted batch, where its packets are, on the plan's stream: ordered behind that batch by the stream alone.
 * CRSDR_ESTATE for a plan with nothing submitted or with a slab bound (the matrix is then not in the packet); CRSDR_EINVAL for
 * another geometry or device, or a batch that is not a multiple of `frames` or exceeds max_batch. */
int crsdr_caf_submit_plan(crsdr_caf *caf, crsdr_plan *plan);

/* Waits for the last submit and copies out what is asked for (any pointer may be NULL); nest = nblocks / frames.  chi, map and peak
 * as laid out above.  CRSDR_ESTATE before the first submit. */
int crsdr_caf_fetch(crsdr_caf *caf, float *chi, float *map, float *peak);

/* Device addresses of the results ([max_batch / frames] lines each, laid out as above), for consumers on the same stream. */
int crsdr_caf_device_buffers(crsdr_caf *caf, void **chi, void **map, void **peak);

/* Of the last submit: the number of lines (what crsdr_caf_fetch will write) and the kernel launches it issued (the same for every
 * nblocks).  Either pointer may be NULL.  CRSDR_ESTATE before the first submit. */
int crsdr_caf_last_submit(crsdr_caf *caf, int *nest, int *launches);

/* The per-op form on one packet's matrix [nrows][blocksize] (frames = 1, so nd = blocksize / (2 seg)): the same kernels on the same
 * arguments, bit for bit.  chi [nrows][nd][nlags][2], map [nd][nlags], peak [nrows + 1][6]; any of the three may be NULL, not all.
 * mem_kind: CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE (every pointer on the device; matrix, map and peak 4-byte, chi 8-byte
 * aligned). */
int crsdr_ambiguity(float *chi, float *map, float *peak, const int8_t *matrix, int nrows, int blocksize, int seg, int nlags, int ref_row,
                    int window, int guard, int mem_kind);

/* Detections.  The peak figures name the largest cell of a map whether or not it is a target, and a map holds any number of targets or
 * none.  A cell-averaging CFAR (constant false-alarm rate) detector over every map of a line, on the device, leaves a short detection
 * list per map and, for the array map's detections, the complex snapshot across the rows: a few hundred bytes per line for the host in
 * place of chi.  It is off until crsdr_caf_set_cfar; off, a submit is the same three launches and the same bits.
 *
 * A map P [nd][R] is the published array map, or re re + im im of a row's published fp32 chi evaluated in fp64 (two products of
 * converted floats, exact in fp64, and one addition: the same bits with or without contraction).  s(d), S, guard and the linear index
 * i = d R + tau are those of the peaks above.  Hd = gd + td, Hr = gr + tr.
 * Training set of a cell (d, tau) of S: the cells (d + a mod nd, tau + b) with
 *     |a| <= Hd and |b| <= Hr;   NOT (|a| <= gd and |b| <= gr);   0 <= tau + b < R;   the Doppler bin in S.
 * Doppler wraps and lag does not; the zero-Doppler ridge that guard cuts out of the search is cut out of the training cells as well.
 * N is the size of the set, Z the fp64 sum of P over it (the order is not pinned; it is never formed by subtracting a guard block from
 * a full box, which would carry the cancelled target's rounding error).
 * A cell of S is detected if and only if
 *     N >= min_train;   Z > 0;   P > t,  noise = Z / (double)N,  t = (double)alpha * noise  (one division, one multiplication, so);
 *     it is the maximum of its 3 x 3 neighbourhood: neighbour Doppler wraps, neighbours outside 0 .. R - 1 or outside S are ignored,
 *     and against a neighbour q the test is P > P_q, or P == P_q with i < i_q.
 * One target spread over a Hann main lobe gives one detection, a plateau its first cell, an all-zero map none and no NaN.
 * Outputs per (line, entry), entries 0 .. nrows as peak has them, K = max_det:
 *     count [nest][nrows + 1] int32      the number of detected cells; may exceed K
 *     det   [nest][nrows + 1][K][8]      the K detections of largest P, ties by smaller i, in that order; unused slots zero.  A detection is
 *                                        (lag, doppler = s(d), power = P, snr = P / noise, noise, dlag, ddop, ntrain = N), each rounded once
 *                                        to fp32; dlag and ddop are the two parabolas of the peaks, with the same edge rules
 *     snap  [nest][K][nrows][2]          for the array map's detections (entry nrows) only: chi_c[d*][tau*] of every row, the reference
 *                                        row included, copied bit for bit; unused slots zero
 * Bits.  Nothing depends on the order in which workgroups run: the same input gives the same bytes, a line has the same bits wherever
 * it sits in a batch, and crsdr_cfar launches the same kernels on the same arguments.
 * Limits, all CRSDR_EINVAL and all checked before a device is touched, by one function for the engine and the per-op call:
 * gd, gr, td, tr >= 0; Hd <= 8; Hr <= 16; td + tr >= 1; 2 Hd + 1 <= nd; alpha finite and > 0; min_train >= 1; 1 <= max_det <= 64. */
typedef struct crsdr_cfar_desc {
    int32_t gd, gr;           /* guard half-widths over Doppler and lag */
    int32_t td, tr;           /* training half-widths beyond the guard */
    float alpha;              /* threshold = alpha * the training cells' mean */
    int32_t min_train;        /* a cell with fewer training cells is never detected */
    int32_t max_det;          /* K: detections kept per map, 1..64 */
} crsdr_cfar_desc;

/* Sets the detector (NULL: off).  Between submits only: it waits for the last one and allocates here, never in a submit; what a
 * fetch_cfar would have returned is gone.  With it on a submit is five launches whatever the number of blocks (crsdr_caf_last_submit). */
int crsdr_caf_set_cfar(crsdr_caf *caf, const crsdr_cfar_desc *desc);

/* Waits for the last submit and copies out what is asked for (any pointer may be NULL), laid out as above.  CRSDR_ESTATE with the
 * detector off, or before the first submit since it was set. */
int crsdr_caf_fetch_cfar(crsdr_caf *caf, float *det, int32_t *count, float *snap);

/* Device addresses of det, count and snap ([max_batch / frames] lines each), for consumers on the same stream -- a direction per
 * detection from snap, say.  They change with every crsdr_caf_set_cfar.  CRSDR_ESTATE with the detector off. */
int crsdr_caf_cfar_device_buffers(crsdr_caf *caf, void **det, void **count, void **snap);

/* The per-op form on ONE map: comps = 1 reads a map [nd][R], comps = 2 a chi [nd][R][2].  det [K][8], count [1]; either may be NULL, not
 * both.  nd a power of two in 8 .. 4096, 1 <= R <= 1024, 0 <= guard <= nd / 2.  The same two kernels on the same arguments, bit for bit.
 * mem_kind: CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE (every pointer on the device; det, count and a map 4-byte, a chi 8-byte
 * aligned). */
int crsdr_cfar(float *det, int32_t *count, const float *src, int comps, int nd, int R, int guard, const crsdr_cfar_desc *desc, int mem_kind);

/* Host only: alpha = N (pfa^(-1 / N) - 1), the cell-averaging factor that gives a false-alarm probability pfa per cell on ONE row's
 * map under exponentially distributed noise power and N = ntrain training cells.  The array map is a sum of nrows - 1 such terms
 * (a gamma variate, not an exponential one): it takes a caller's own alpha.  Cells near the lag edges, or near the guard with one
 * set, train on fewer than ntrain cells and so run at a somewhat higher rate.  CRSDR_EINVAL for pfa outside (0, 1) or ntrain < 1. */
int crsdr_cfar_alpha(double pfa, int ntrain, float *alpha);

/* Estimators.  The mean of all training cells has two known failures: a strong cell inside a weaker target's window lifts the mean
 * over it (masking), and where the floor steps the mean of the low side under-estimates the high side (clutter edges).  Three more
 * estimates of the noise can be chosen.  P, S, guard, i, the training set, N, the 3 x 3 test, the order of the detections, det[8],
 * count and snap are as above, and a detected cell still needs noise > 0 and P > t, t = (double)alpha * noise: only noise and ntrain
 * change.  Nfull = (2 Hd + 1)(2 Hr + 1) - (2 gd + 1)(2 gr + 1).
 *   CRSDR_CFAR_CA   cell averaging, as above, bit for bit.
 *   CRSDR_CFAR_GO,  greatest-of and smallest-of.  axis 0 (lag) splits the training set into the cells with b < 0 and those with b > 0,
 *   CRSDR_CFAR_SO   axis 1 (Doppler) into a < 0 and a > 0; cells on the centre line (b = 0, or a = 0) train neither half.  A half counts
 *                   if and only if its size N_h >= min_train; its mean is Z_h / (double)N_h, Z_h formed by additions only.  noise is
 *                   the larger (GO) or smaller (SO) mean over the halves that count, the lower half (b < 0, a < 0) on equal means,
 *                   and ntrain that half's N_h.  No counting half, or a chosen mean that is not above 0 (SO beside an all-zero half):
 *                   no detection.  GO holds its rate across a clutter edge; SO sees past an interferer on one side.
 *   CRSDR_CFAR_OS   ordered statistic.  1 <= rank <= Nfull.  At a cell with N >= min_train, k = max(1, ceil(rank N / Nfull)) in
 *                   integers and noise is the k-th smallest P of the training set: a value of the map, without rounding; ntrain = N.
 *                   Only cells of the set take part: a cell outside the lags or outside S is absent, not a zero, and a cell of S
 *                   whose P is 0 is present.  It survives several interferers (fewer than N - k of them).
 * The estimator belongs to the descriptor last set: every crsdr_caf_set_cfar, on or off, puts it back to cell averaging. */
enum { CRSDR_CFAR_CA = 0, CRSDR_CFAR_GO = 1, CRSDR_CFAR_SO = 2, CRSDR_CFAR_OS = 3 };
typedef struct crsdr_cfar_est_desc {
    int32_t estimator;        /* CRSDR_CFAR_* */
    int32_t axis;             /* GO, SO: 0 splits over lag, 1 over Doppler; not read otherwise */
    int32_t rank;             /* OS: 1..Nfull; not read otherwise */
} crsdr_cfar_est_desc;

/* Sets the estimator of the detector that is on (NULL: cell averaging), wherever its descriptor goes: the rows' maps, the array map
 * and the beam maps' detector; the bearings' adaptive training set is the window's geometry and does not change.  Between submits
 * only: it waits for the last one; what a fetch_cfar would have returned is gone.  It allocates nothing and a submit's launches stay
 * as many.  CRSDR_ESTATE while bearings, beams or the tracker are on (turn them off first), and with no detector set.
 * CRSDR_EINVAL, before a device is touched, for an estimator outside 0..3, an axis outside 0..1 (GO, SO) or a rank outside
 * 1..Nfull (OS). */
int crsdr_caf_set_cfar_estimator(crsdr_caf *caf, const crsdr_cfar_est_desc *est);

/* crsdr_cfar under an estimator: est NULL or CRSDR_CFAR_CA is crsdr_cfar, bit for bit; otherwise the same limits on est as above. */
int crsdr_cfar_est(float *det, int32_t *count, const float *src, int comps, int nd, int R, int guard, const crsdr_cfar_desc *desc,
                   const crsdr_cfar_est_desc *est, int mem_kind);

/* Host only: the alpha that gives a false-alarm probability pfa per cell under exponentially distributed noise power, from the exact
 * equation of the estimator by bisection in fp64, rounded once to fp32.  est NULL or CA: crsdr_cfar_alpha.
 *   GO, SO   ntrain is the cells per half n, T = alpha / n:  P_SO = 2 (2 + T)^-n sum_{i < n} C(n - 1 + i, i) (2 + T)^-i,
 *            P_GO = 2 (1 + T)^-n - P_SO
 *   OS       rank <= ntrain = N:  P_OS = prod_{i < rank} (N - i) / (N - i + alpha)
 * CRSDR_EINVAL for pfa outside (0, 1), an estimator outside 0..3, ntrain outside 1..65536 (CA: below 1), a rank outside 1..ntrain. */
int crsdr_cfar_alpha_est(double pfa, int ntrain, const crsdr_cfar_est_desc *est, float *alpha);

/* Cancellation.  A surveillance row holds the illuminator's own signal, strong and at short delays, and its ambiguity function has a
 * noise-like floor about 1 / (nd Ls) below its peak in EVERY cell, which guard does not touch: an echo 40 dB down lies under it.  The
 * canceller (the extensive cancellation algorithm, ECA) projects the reference and its first delays, optionally shifted by a few
 * Doppler bins, out of every row between the range stage and the Doppler stage -- in the lag domain, on the exact integers; no float
 * copy of the rows is made.  It is off until crsdr_caf_set_cancel; off, a submit is the same launches and the same bits.
 *
 * Parameters.  taps = K, dopp = P; the basis has n = K (2 P + 1) members.  Member (m, p), 0 <= m < K, -P <= p <= P, is in segment k
 *     phi_p[k] X_r[j Ls + n - m],   phi_p[k] = exp(2 pi i p k / nd) in fp64
 * (the phase constant within a segment, as the Doppler stage itself has it; X_r zero in front of the packet, as in y).
 * Reference sums, exact in int32 with the bound of y:
 *     G[k][m][tau] = sum_{n < Ls} X_r[j Ls + n - m] conj(X_r[j Ls + n - tau]),   m < K, tau < R;   G[k][0][tau] = y_r[k][tau]
 * Per (line, row c != r), in fp64:
 *     c_(m',p')       = sum_k conj(phi_p'[k]) y_c[k][m']
 *     A_(m',p'),(m,p) = sum_k phi_(p-p')[k] G[k][m][m']        Hermitian; one A per line, shared by its rows
 *     E               = sum |X_c|^2 over the line
 *     A h_c = c  by Cholesky.  A pivot <= 2^-40 A_(0,0),(0,0) makes the line SINGULAR (an all-zero or rank-deficient reference): then
 *     h = 0 for every row of the line, status bit 0 is set, and the line's chi has the bits the canceller-off path gives.
 * Cancellation:
 *     y'_c[k][tau] = y_c[k][tau] - sum_(m,p) h_c,(m,p) phi_p[k] G[k][m][tau]
 * evaluated in fp64 from the integers and rounded ONCE to fp32; from there the Doppler stage runs as above (w[k], the transform, the
 * scale).  Row r is left alone: its chi is bit for bit what the canceller-off path gives.  The array map, the peaks, the detector and
 * snap run unchanged on the cancelled chi.
 * Outputs per (line, row):
 *     coef  [nest][nrows][n][2] float    h, index (p + P) K + m (m fastest within p), each part rounded once; row r zero
 *     cinfo [nest][nrows][2] float       the share of the row's power that stays, clamp((E - Re sum conj(h) c) / E, 0, 1), 1 where E = 0;
 *                                        and the status (0, or 1 = singular).  Row r: (1, 0)
 * Bits.  Nothing depends on the order in which workgroups run: a line has the same bits wherever it sits in a batch, and
 * crsdr_ambiguity_cancel launches the same kernels on the same arguments.
 * Limits, all CRSDR_EINVAL and all checked before a device is touched, by one function for the engine and the per-op call:
 * 0 <= P <= 2; 1 <= K <= min(R, 32); K (2 P + 1) <= 48; 2 P + 1 <= nd; (max_batch / frames) * nd * K * R <= 2^24. */
typedef struct crsdr_caf_cancel_desc {
    int32_t taps;             /* K: delays 0 .. K - 1 of the reference */
    int32_t dopp;             /* P: Doppler shifts -P .. P bins of each */
} crsdr_caf_cancel_desc;

/* Sets the canceller (NULL: off).  Between submits only: it waits for the last one and allocates here, never in a submit; what a
 * fetch_cancel would have returned is gone.  With it on a submit is seven launches (nine with the detector) whatever the number of
 * blocks (crsdr_caf_last_submit). */
int crsdr_caf_set_cancel(crsdr_caf *caf, const crsdr_caf_cancel_desc *desc);

/* Waits for the last submit and copies out what is asked for (either pointer may be NULL), laid out as above.  CRSDR_ESTATE with the
 * canceller off, or before the first submit since it was set. */
int crsdr_caf_fetch_cancel(crsdr_caf *caf, float *coef, float *cinfo);

/* Device addresses of coef and cinfo ([max_batch / frames] lines each).  They change with every crsdr_caf_set_cancel.  CRSDR_ESTATE
 * with the canceller off. */
int crsdr_caf_cancel_device_buffers(crsdr_caf *caf, void **coef, void **cinfo);

/* crsdr_ambiguity with the canceller: its arguments, then taps, dopp and the two further outputs coef [nrows][n][2] and
 * cinfo [nrows][2] (either may be NULL; with mem_kind CRSDR_MEM_DEVICE 4-byte aligned).  The same kernels on the same arguments as the
 * engine, bit for bit. */
int crsdr_ambiguity_cancel(float *chi, float *map, float *peak, const int8_t *matrix, int nrows, int blocksize, int seg, int nlags, int ref_row,
                           int window, int guard, int mem_kind, int taps, int dopp, float *coef, float *cinfo);

/* Cleaning.  An echo has the same floor about 1 / (nd Ls) below its own peak in every cell, and the canceller removes that floor for
 * delays 0 .. K - 1 at |p| <= P alone.  A strong mover -- an aircraft close to the receiver -- lays it over the whole map, at Doppler
 * bins the canceller never touches, and every weaker target under it is lost to the detector whichever estimator it runs.  The second
 * stage takes the strong detections of the first pass, adds the reference delayed and Doppler-shifted to each of them to the
 * canceller's basis, solves jointly, and forms the maps and the lists again on the residual.  It is off until crsdr_caf_set_clean and
 * needs the canceller and the detector on.  Off, a submit is the same launches and the same bits; on, every other output -- chi, map,
 * peak, det, count, snap, coef, cinfo, and what bearings, beams, integration and tracker publish -- keeps the bits it has with it off:
 * the residual goes to buffers of its own, and nothing else reads them.
 *
 * Parameters.  max_targets = T, min_snr (the ratio a detection's snr is), wl and wq: the half-widths of a target's cluster over lag,
 * and over Doppler in HALF bins.
 * Picks, per line, from the array map's published list (entry nrows of det and count), decided in fp64 on the published fp32 figures
 * and so exact.  The first min(count, K_det) records in their order; a record has f = (double)doppler + (double)ddop and l = lag.  The
 * circular distance of two Dopplers is g = |f - f'|, or nd - g when g > nd / 2.  A record is skipped if snr < min_snr; if it touches
 * the clutter basis, l - wl <= K - 1 and the circular distance of f to 0 < P + 1 + wq / 2; or if it touches an accepted pick,
 * |l - l'| <= 2 wl and the circular distance of f to f' < wq + 1.  Otherwise it is accepted; the walk stops at T accepted.
 * Members.  The canceller's n1 = K (2 P + 1) members first, their indices unchanged.  Then per pick in pick order, q = -wq .. wq outer,
 * j = -wl .. wl inner, member (m, g) = (l + j, f + q / 2), in segment k
 *     phi_g[k] X_r[j Ls + n - m],   phi_g[k] = exp(2 pi i g k / nd), evaluated in fp64 as sincospi(2 * ((g * k) / nd))
 * A lag outside 0 .. R - 1 is left out, not wrapped.  n <= 64 members.
 * Sums.  G[k][m][tau] as above, for every distinct member lag m and all tau < R, and y_c[k][m] at those lags: exact in int32.
 * Normal equations of the line, member i = (m_i, g_i):
 *     A_ij = sum_k phi_(g_j - g_i)[k] G[k][m_j][m_i]        c_i = sum_k conj(phi_(g_i)[k]) y_c[k][m_i]
 * The canceller's block of A has the bits of the first stage's; the cross block and the target block are new.
 * Solve.  Cholesky by columns in member order with the pivot floor above, 2^-40 A_(0,0),(0,0).  The canceller's members come first,
 * so the leading block's factor is the first stage's bit for bit, and a line WITHOUT PICKS has rchi == chi, rmap == map,
 * rdet == det, rcount == count and rsnap == snap, byte for byte.
 *     Status 1: a pivot of the canceller's block at or under the floor (the first stage is singular).  h = 0; rchi has chi's bits.
 *     Status 2: a target column's pivot at or under the floor.  The target coefficients are 0, the canceller's are the first
 *               stage's, and rchi has chi's bits.
 * Residual.
 *     y''_c[k][tau] = y_c[k][tau] - sum_i h_c,i phi_(g_i)[k] G[k][m_i][tau]
 * in fp64 from the integers with ONE rounding to fp32, the canceller's members in the first stage's order and the target members
 * behind them; then the Doppler stage, the array map and the detector (under the descriptor's estimator) as they are.  Row r is left
 * alone.
 * Outputs per line:
 *     tgt    [nest][T][8]                               the picked records, copied bit for bit; unused slots zero
 *     ntgt   [nest] int32
 *     tcoef  [nest][nrows][T][(2 wq + 1)(2 wl + 1)][2]  the target members' h per row, index (q + wq)(2 wl + 1) + (j + wl), each part
 *                                                       rounded once: a target's complex amplitude across the rows.  Left-out
 *                                                       members, unused picks and row r are zero
 *     tinfo  [nest][nrows][2]                           the share of the row's power that stays under the joint solve (as cinfo has
 *                                                       it, over all members), and the status (0, 1 or 2).  Row r: (1, 0)
 *     rchi, rmap, rdet, rcount, rsnap                   laid out exactly as chi, map, det, count and snap
 * Bits.  Nothing depends on the order in which workgroups run, there are no float atomics, a line has the same bits wherever it sits
 * in a batch, and crsdr_ambiguity_clean runs the same kernels on the same arguments.
 * Limits, all CRSDR_EINVAL and all checked before a device is touched, by one function for the engine and the per-op call:
 * 1 <= T <= 8; 0 <= wl <= 2; 0 <= wq <= 2; n1 + T (2 wl + 1)(2 wq + 1) <= 64; min_snr finite and > 0;
 * (max_batch / frames) * nd * (K + T (2 wl + 1)) * R <= 2^24; 2 * (max_batch / frames) * nrows * nd * R <= 2^24 (chi and rchi).
 * State.  CRSDR_ESTATE: crsdr_caf_set_clean without the canceller or the detector, or with CRSDR_INTEGRATE_ARRAY on (the picks would
 * come from another line's energy); while it is on, crsdr_caf_set_cancel, crsdr_caf_set_cfar, crsdr_caf_set_cfar_estimator and
 * crsdr_caf_set_integrate with CRSDR_INTEGRATE_ARRAY (turn it off first).
 * Launches.  NINE more per submit (crsdr_caf_last_submit), whatever the number of blocks and however many picks a line has. */
typedef struct crsdr_caf_clean_desc {
    int32_t max_targets;      /* T: picks per line, 1..8 */
    float min_snr;            /* a record below it is not picked */
    int32_t wl;               /* lags l - wl .. l + wl of a pick */
    int32_t wq;               /* Dopplers f - wq / 2 .. f + wq / 2 of a pick, in steps of half a bin */
} crsdr_caf_clean_desc;

/* Sets the cleaning (NULL: off).  Between submits only: it waits for the last one and allocates here, never in a submit; what a
 * fetch_clean would have returned is gone. */
int crsdr_caf_set_clean(crsdr_caf *caf, const crsdr_caf_clean_desc *desc);

/* Waits for the last submit and copies out what is asked for (any pointer may be NULL), laid out as above.  CRSDR_ESTATE with the
 * cleaning off, or before the first submit since it was set. */
int crsdr_caf_fetch_clean(crsdr_caf *caf, float *tgt, int32_t *ntgt, float *tcoef, float *tinfo, float *rchi, float *rmap, float *rdet, int32_t *rcount,
                          float *rsnap);

/* Device addresses of the same ([max_batch / frames] lines each).  They change with every crsdr_caf_set_clean.  CRSDR_ESTATE with
 * the cleaning off. */
int crsdr_caf_clean_device_buffers(crsdr_caf *caf, void **tgt, void **ntgt, void **tcoef, void **tinfo, void **rchi, void **rmap, void **rdet, void **rcount,
                                   void **rsnap);

/* The per-op form on one packet's matrix (frames = 1): canceller, detector (est NULL: cell averaging) and cleaning on one line, every
 * output of the three laid out as above for nest = 1; any pointer of `out` may be NULL.  It makes a one-line engine for the call on
 * the current device and runs its submit: the same kernels on the same arguments, bit for bit.  mem_kind: CRSDR_MEM_HOST (copied) or
 * CRSDR_MEM_DEVICE (every pointer on the device, 4-byte aligned, chi and rchi 8-byte). */
typedef struct crsdr_clean_out {
    float *chi, *map, *peak, *coef, *cinfo, *det;
    int32_t *count;
    float *snap, *tgt;
    int32_t *ntgt;
    float *tcoef, *tinfo, *rchi, *rmap, *rdet;
    int32_t *rcount;
    float *rsnap;
} crsdr_clean_out;
int crsdr_ambiguity_clean(const crsdr_clean_out *out, const int8_t *matrix, int nrows, int blocksize, int seg, int nlags, int ref_row, int window, int guard,
                          int mem_kind, const crsdr_caf_cancel_desc *cancel, const crsdr_cfar_desc *cfar, const crsdr_cfar_est_desc *est,
                          const crsdr_caf_clean_desc *clean);

/* Bearings.  A detection of the array map says at which lag and Doppler a target is; snap holds its complex value across the rows.
 * This stage, behind the detector and on the device, turns every such detection into a direction: a line's result is a list of
 * (lag, Doppler, bearing) in a few hundred bytes.  It is off until crsdr_caf_set_bearing; off, a submit is the same launches and the
 * same bits.
 *
 * Array.  The rows c != ref_row in ascending order are the elements e = 0 .. m - 1 of an mx x my uniform rectangular array,
 * m = nrows - 1 = mx my, 2 <= m <= 64, in crsdr_pmusic2d's element order (e = iy mx + ix) and with crsdr_doa_set_refine's fp64
 * steering expression at the cell coordinates (x, y):
 *     alpha = x pi / ncx,  beta = y pi / ncy,  ph_e = 2 pi (double)d (ix cos(alpha) sin(beta) + iy cos(beta)),  a_e = (cos ph_e, sin ph_e)
 * Snapshot.  For slot q < min(count, K) of the array map's detections (entry nrows; K = max_det), at the detection's cell (d*, tau*):
 *     u_e = conj(chi_c[d*][tau*])      from the published fp32 chi, converted to fp64
 * The conjugate is deliberate: chi_c carries a_true, and crsdr_doa's X^H X convention (see crsdr_doa_set_beams) peaks at conj(a_true);
 * with u = conj(x) the same emitter gives the same grid cell from both engines.
 * Weighting W (m x m Hermitian, fp64).
 *     CRSDR_BEARING_CONVENTIONAL   W = I
 *     CRSDR_BEARING_ADAPTIVE       the training set of the cell is exactly the detector's set of that cell (the same gd, gr, td, tr, the
 *                                  same guard; Doppler wraps, lag does not), so N equals the ntrain the detection reports.  With u_t
 *                                  the conjugated chi across the elements at a training cell,
 *                                      Q = (1 / N) sum_train u_t u_t^H,   Q' = Q + loading (trace(Q) / m) I,   W = Q'^-1 by Cholesky.
 *                                  Q' is positive definite whenever trace(Q) > 0, also for N < m, and cond(Q') <= 1 + m / loading.
 *                                  N = 0 or trace(Q) = 0: W = I and status bit 1 is set (so, too, for a pivot that is not > 0, which only
 *                                  a non-finite chi can give).  The order of the sum is not pinned.
 * The training cells hold the direct path's ambiguity floor, whose spatial signature is the illuminator's direction in every cell and
 * which pulls a weak target's conventional bearing toward the illuminator; whitening with their covariance removes that bias.
 * Statistic.
 *     T(x, y) = |a^H W u|^2 / ((a^H W a) (u^H W u))           in [0, 1] by Cauchy-Schwarz
 * With W = I it is the share of the snapshot's power that a plane wave from (x, y) explains (the single-source maximum-likelihood
 * statistic).  The order of the fp64 operations inside T is not pinned; on this array a^H W a is a 2-D trigonometric polynomial whose
 * coefficients are the sums of W over the element pairs of equal co-array lag, and the device evaluates it so.
 * u^H u = 0: T = 0 everywhere, every figure of the slot is 0 and status bit 0 is set.  Never a NaN.
 * The adaptive T is far more selective than the conventional one, the more so the more elements there are and the stronger the
 * target's own floor in its training cells: the grid must be fine enough to sample its main lobe, or the grid peak is not the
 * target's (64 elements: a 64 x 64 grid where 32 x 32 serves the conventional mode).
 * Grid peak.  (cx, cy) is the first maximum of T over cx < ncx, cy < ncy in row-major order (index cx ncy + cy).
 * Refinement.  levels = 0 (off) or 1 .. 8: the zoom search of crsdr_doa_set_refine, word for word, on f = T -- x = cx, y = cy, s = 1/2;
 * per level the 7 x 7 lattice of spacing s around (x, y), each point clamped to [0, ncx] x [0, ncy], in row-major order (i major); a
 * point replaces the best so far if it is strictly above the centre and strictly above the best; then s = s / 4.
 * Outputs per line:
 *     dir  [nest][K][8] float           (cx, cy, T at the grid peak, x - cx, y - cy, alpha, beta, status), each figure rounded once from
 *                                       fp64; the offsets are exact.  levels = 0: offsets 0, the angles are the grid point's.  Slots from
 *                                       min(count, K) on are all zero.  status: bit 0 an all-zero snapshot, bit 1 W = I in the adaptive
 *                                       mode, bit 2 (crsdr_bearing on hand-made det only) a lag or Doppler outside the map: figures 0.
 *     spec [nest][K][ncx][ncy] float    with the flag CRSDR_BEARING_KEEP_SPECTRUM: T of every grid point; unused slots zero
 * Bits.  Nothing depends on the order in which workgroups run: a line has the same bits wherever it sits in a batch, and crsdr_bearing
 * launches the same kernels on the same arguments.
 * Limits, all CRSDR_EINVAL and all checked before a device is touched, by one function for the engine and the per-op call:
 * mx, my >= 1; m = mx my = nrows - 1 in 2 .. 64; 2 <= ncx, ncy <= 512; d finite and > 0; a valid mode; loading in [1e-6, 1] when
 * adaptive; levels in 0 .. 8; no unknown flag; with the keep flag (max_batch / frames) * K * ncx * ncy <= 2^24. */
enum { CRSDR_BEARING_CONVENTIONAL = 1, CRSDR_BEARING_ADAPTIVE = 2 };
enum { CRSDR_BEARING_KEEP_SPECTRUM = 1u << 0 };

typedef struct crsdr_caf_bearing_desc {
    int32_t mx, my;           /* the array: mx my = nrows - 1 elements */
    int32_t ncx, ncy;         /* the scan grid */
    float d;                  /* element spacing in wavelengths */
    int32_t mode;             /* CRSDR_BEARING_* */
    float loading;            /* adaptive: diagonal loading, relative to trace(Q) / m */
    int32_t levels;           /* zoom levels, 0 = the grid peak alone */
    uint32_t flags;           /* CRSDR_BEARING_KEEP_SPECTRUM */
} crsdr_caf_bearing_desc;

/* Sets the bearings (NULL: off).  Between submits only: it waits for the last one and allocates here, never in a submit; what a
 * fetch_bearing would have returned is gone.  CRSDR_ESTATE while the detector is off.  While bearings are on crsdr_caf_set_cfar returns
 * CRSDR_ESTATE: the buffers are sized by its K and the training set is its own, so turn the bearings off first.  With bearings on a
 * submit issues THREE launches more than without (eight, twelve with the canceller), whatever the number of blocks and whatever the
 * counts, which the kernels read on the device (crsdr_caf_last_submit); empty slots write their zeros and leave. */
int crsdr_caf_set_bearing(crsdr_caf *caf, const crsdr_caf_bearing_desc *desc);

/* Waits for the last submit and copies out what is asked for (either pointer may be NULL), laid out as above.  CRSDR_ESTATE with the
 * bearings off, before the first submit since they were set, or for spec without CRSDR_BEARING_KEEP_SPECTRUM. */
int crsdr_caf_fetch_bearing(crsdr_caf *caf, float *dir, float *spec);

/* Device addresses of dir and spec ([max_batch / frames] lines each; spec NULL unless kept).  They change with every
 * crsdr_caf_set_bearing.  CRSDR_ESTATE with the bearings off. */
int crsdr_caf_bearing_device_buffers(crsdr_caf *caf, void **dir, void **spec);

/* The per-op form on ONE line: chi [nrows][nd][R][2], the array map's det [K][8] and count [1] as crsdr_cfar or the engine wrote them
 * (or made by hand: only lag, Doppler and the position in the list are read), K = cfar->max_det; the detector's descriptor supplies
 * the training set.  dir [K][8], spec [K][ncx][ncy] (asked for only with the keep flag); either may be NULL, not both.  nd, R, guard as
 * crsdr_cfar has them, 0 <= ref_row < nrows, nrows nd R <= 2^24.  The same three kernels on the same arguments, bit for bit.
 * mem_kind: CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE (every pointer on the device; det, count, dir and spec 4-byte, chi 8-byte
 * aligned). */
int crsdr_bearing(float *dir, float *spec, const float *chi, int nrows, int nd, int R, int ref_row, int guard, const float *det,
                  const int32_t *count, const crsdr_cfar_desc *cfar, const crsdr_caf_bearing_desc *desc, int mem_kind);

/* Beams.  The array map sums the rows' powers: it gives away the array's coherent gain (a factor of m in power) and has no spatial
 * selectivity, so the direct path's ambiguity floor, which carries the illuminator's spatial signature in every cell, enters it at full
 * strength -- and a target it cannot detect never gets a bearing.  This stage forms a bank of coherent beams across the rows, on chi,
 * which is linear in the rows: beams formed behind the Doppler stage equal beamforming the rows first, at a fraction of the cost.  The
 * detector then runs on every beam's map and the beams' lists are fused into one per line.  It is off until crsdr_caf_set_beams; off,
 * a submit is the same launches and the same bits, in every combination of canceller, detector and bearings.
 *
 * Elements.  The rows c != ref_row in ascending order are the elements e = 0 .. m - 1, m = nrows - 1, 1 <= m <= 64: the bearings'
 * rule.  No geometry is implied: the weights w [nbeams][m][2] (re, im) are the caller's, 1 <= nbeams <= 64, every one finite.
 * Beam sums, in fp32 from the published fp32 chi:
 *     z_b[d][tau] = sum_e w_b,e chi_c(e)[d][tau]        re z = sum_e (wr cr - wi ci),   im z = sum_e (wr ci + wi cr)
 *     bmap [nest][nbeams][nd][R] float = (float)((double)re z re z + (double)im z im z)
 * The order of the sum and its fused multiply-adds are the kernel's (e ascending, per element re = fma(-wi, ci, fma(wr, cr, re)) and
 * im = fma(wr, ci, fma(wi, cr, im)): what the fp32 matrix instruction leaves) and are not pinned against the model, whose bars hold for
 * any order.  In the bearings' convention u = conj(chi) and |w^H u|^2 = |sum_e w_e chi_e|^2: with w = a(x, y) / sqrt(m)
 * (crsdr_caf_beam_steer) the bmap value is the conventional T(x, y) of crsdr_caf_set_bearing times the array map's value at that cell.
 * Non-finite inputs are the caller's; finite inputs never give a NaN.
 * Beam detections (only with the detector on).  The detector of crsdr_caf_set_cfar runs unchanged on every beam map, with the same
 * descriptor and guard: its two kernels take (line, beam) for the line of a one-map call, as crsdr_cfar has it with comps = 1.
 *     bcount [nest][nbeams] int32,   bdet [nest][nbeams][K][8]        laid out and rounded exactly as count and det; no snapshots
 * Fusion into one list per line.  The candidates are the slots q < min(bcount[b], K) of every beam, at most 64 x 64 of them (a
 * hand-made slot whose lag or Doppler lies outside the map is none).  Candidate A comes before A' iff P > P', or P == P' and b < b', or
 * both equal and i < i' with i = d R + tau (a hand-made list that names one cell twice in one beam: the earlier slot first, so that the
 * order is total on any list).  A candidate is suppressed iff some other candidate of the line comes before it and lies
 * within one cell of it -- lag difference at most 1, no wrap, and Doppler difference at most 1 modulo nd -- whether or not that other
 * candidate is itself suppressed.
 *     nfused [nest] int32         the number of survivors; may exceed K
 *     fused  [nest][K][8]         the first K survivors in that order: the bdet record bit for bit, the eighth figure (ntrain)
 *                                 replaced by the beam index as a float; unused slots zero
 * Bits.  Nothing depends on the order in which workgroups or atomics arrive: a line has the same bits wherever it sits in a batch, and
 * crsdr_beam_maps, crsdr_cfar and crsdr_beam_fuse launch the same kernels on the same arguments.
 * Limits, all CRSDR_EINVAL and all checked before a device is touched, by one function for the engine and the per-op call:
 * 1 <= m <= 64; 1 <= nbeams <= 64; weights not NULL and every one finite; no flag; (max_batch / frames) * nbeams * nd * R <= 2^24. */
typedef struct crsdr_caf_beams_desc {
    int32_t nbeams;
    const float *weights;     /* host, [nbeams][m][2]; copied by the call */
    uint32_t flags;           /* none yet: must be 0 */
} crsdr_caf_beams_desc;

/* Sets the beams (NULL: off).  Between submits only: it waits for the last one and allocates here, never in a submit; what a
 * fetch_beams would have returned is gone.  Whether the beams are detected on is the detector's state at this call, and while beams
 * are on crsdr_caf_set_cfar returns CRSDR_ESTATE: turn the beams off first.  With beams on a submit issues ONE launch more than without
 * when the detector was off, FOUR when it was on (the maps, the detector's two, the fusion), whatever the number of blocks and
 * whatever the counts (crsdr_caf_last_submit). */
int crsdr_caf_set_beams(crsdr_caf *caf, const crsdr_caf_beams_desc *desc);

/* Waits for the last submit and copies out what is asked for (any pointer may be NULL), laid out as above.  CRSDR_ESTATE with the beams
 * off, before the first submit since they were set, or for bdet, bcount, fused or nfused when the detector was off at set_beams. */
int crsdr_caf_fetch_beams(crsdr_caf *caf, float *bmap, float *bdet, int32_t *bcount, float *fused, int32_t *nfused);

/* Device addresses ([max_batch / frames] lines each; the lists NULL when the detector was off).  They change with every
 * crsdr_caf_set_beams.  CRSDR_ESTATE with the beams off. */
int crsdr_caf_beams_device_buffers(crsdr_caf *caf, void **bmap, void **bdet, void **bcount, void **fused, void **nfused);

/* The beam maps of ONE line: chi [nrows][nd][R][2] -> bmap [nbeams][nd][R].  1 <= nd <= 4096 (the maps do not depend on the shape of a
 * line, only on its nd R cells: nd need not be a power of two here), 1 <= R <= 1024, 0 <= ref_row < nrows, nrows nd R <= 2^24.  The engine's kernel on the same arguments, bit for bit.  mem_kind: CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE
 * (bmap 4-byte and chi 8-byte aligned, on the device); weights is host memory in either kind, as in the descriptor. */
int crsdr_beam_maps(float *bmap, const float *chi, int nrows, int nd, int R, int ref_row, const float *weights, int nbeams, int mem_kind);

/* The fusion of ONE line: bdet [nbeams][K][8] and bcount [nbeams] as crsdr_cfar or the engine wrote them (or made by hand: lag, Doppler,
 * power and the position are read) -> fused [K][8], nfused [1]; either may be NULL, not both.  1 <= K <= 64.  The engine's kernel on
 * the same arguments, bit for bit.  mem_kind as above, every pointer 4-byte aligned. */
int crsdr_beam_fuse(float *fused, int32_t *nfused, const float *bdet, const int32_t *bcount, int nbeams, int K, int nd, int R, int mem_kind);

/* Host only: weights [nbeams][mx my][2] = a(x, y) / sqrt(m) toward the nbeams cell coordinates xy [nbeams][2] of an ncx x ncy grid, with
 * the bearings' fp64 steering expression and element order (e = iy mx + ix), each part rounded once to fp32.  mx, my >= 1,
 * mx my <= 64, 2 <= ncx, ncy <= 512, d finite and > 0, every coordinate finite: else CRSDR_EINVAL. */
int crsdr_caf_beam_steer(float *weights, int mx, int my, float d, int ncx, int ncy, const double *xy, int nbeams);

/* Adaptive beams.  The direct path's ambiguity floor carries the illuminator's spatial signature in every cell of chi and reaches a
 * fixed beam through its sidelobes; a weak echo is then detectable only above (floor x sidelobe).  This stage replaces the caller's
 * weights, per line, by sample-matrix-inversion MVDR weights from the covariance of the line's own cells.  Off until
 * crsdr_caf_set_beam_adapt; off, a submit is the same launches and the same bits.  Everything behind bmap runs as it stands.
 * Elements e = 0 .. m - 1 are the rows c != ref_row, ascending, 1 <= m <= 64; the caller's weights v_b are those of crsdr_caf_set_beams,
 * taken as fp64.
 * Training cells of a line: Doppler bins (d_lo + a) mod nd, a = 0 .. d_n - 1 (Doppler wraps), lags r_lo + b, b = 0 .. r_n - 1 (lag does
 * not), N = d_n r_n >= 1.  The rectangle is the caller's business: to leave out the zero-Doppler guard, d_lo = guard + 1,
 * d_n = nd - 2 guard - 1.
 * Covariance: snapshot u_e = conj(chi_c(e)[cell]) from the published fp32 chi (the bearings' convention), Q = (1 / N) sum u u^H in
 * fp64, Q' = Q + loading (trace(Q) / m) I, loading in [1e-6, 1]: cond(Q') <= 1 + m / loading, and Q' is positive definite whenever
 * trace(Q) > 0, also for N < m.  The order of the sum is not pinned (every product of two fp32 values is exact in fp64, so the error of
 * Q is fp64 rounding of the sums alone), but it is fixed by the shape alone: a line has the same bits wherever it sits in a batch.
 * Weights, per beam: g = Q'^-1 v_b by Cholesky, den = v_b^H g, w_b = (v_b^H v_b / den) g: MVDR under w^H v_b = v_b^H v_b, so that the
 * beam answers its own look direction exactly as the caller's weight does.  Q proportional to I gives w = v.  A beam whose v_b is all
 * zero keeps it.
 *     aw    [nest][nbeams][m][2] float   each part rounded once from fp64
 *     ainfo [nest][nbeams][2]    float = (w_b^H Q w_b, v_b^H Q v_b), Q the unloaded one, fp64 rounded once: the training cells' mean
 *                                        power through the adaptive beam and through the caller's; both 0 on a fallback line
 *     astat [nest]               int32   0, or the fallback: bit 0 trace(Q) = 0; bit 1 a pivot not > 0 or a sum not finite (only a
 *                                        non-finite chi gives that).  On a fallback line aw is v bit for bit.  Never a NaN comes from
 *                                        finite input.
 * bmap is then the beam kernel's chain with line l's aw in place of w.
 * Limits (CRSDR_EINVAL): 0 <= d_lo < nd; 1 <= d_n <= nd; 0 <= r_lo; 1 <= r_n; r_lo + r_n <= R; loading finite and in range; flags = 0. */
typedef struct crsdr_caf_beam_adapt_desc {
    int32_t d_lo, d_n, r_lo, r_n;
    float loading;
    uint32_t flags;           /* = 0 */
} crsdr_caf_beam_adapt_desc;

/* Sets the adaptation of the beams that are on (NULL: off): the beams' counterpart of crsdr_caf_set_cfar_estimator.  It belongs to the
 * beams' descriptor: every crsdr_caf_set_beams, on or off, turns it off again.  Between submits only: it waits for the last one and
 * allocates here, never in a submit.  With adaptation on a submit issues TWO launches more, whatever the batch.  CRSDR_ESTATE with no
 * beams set, and while the tracker or the integration is on -- their state belongs to the maps this changes: the order is beams, adapt,
 * integrate, track. */
int crsdr_caf_set_beam_adapt(crsdr_caf *caf, const crsdr_caf_beam_adapt_desc *desc);

/* Waits for the last submit and copies out what is asked for (any pointer may be NULL), laid out as above.  CRSDR_ESTATE while the
 * adaptation is off, or before the first submit since it was set. */
int crsdr_caf_fetch_beam_adapt(crsdr_caf *caf, float *aw, float *ainfo, int32_t *astat);

/* Device addresses ([max_batch / frames] lines) for consumers on the same stream.  They change with every crsdr_caf_set_beam_adapt.
 * CRSDR_ESTATE while the adaptation is off. */
int crsdr_caf_beam_adapt_device_buffers(crsdr_caf *caf, void **aw, void **ainfo, void **astat);

/* The adaptive weights of ONE line: chi [nrows][nd][R][2], weights [nbeams][nrows - 1][2] on the host -> aw [nbeams][m][2],
 * ainfo [nbeams][2], astat [1] (at least one of them).  1 <= nd <= 4096, and nd need not be a power of two, as in crsdr_beam_maps.  It
 * runs the engine's kernels on the same arguments, bit for bit; the per-op chain is crsdr_beam_adapt followed by crsdr_beam_maps(aw).
 * mem_kind as above: device aw, ainfo and astat 4-byte, chi 8-byte aligned. */
int crsdr_beam_adapt(float *aw, float *ainfo, int32_t *astat, const float *chi, int nrows, int nd, int R, int ref_row,
                     const float *weights, int nbeams, const crsdr_caf_beam_adapt_desc *desc, int mem_kind);

/* Tracks.  Everything above is per line: a list of (lag, Doppler, bearing) every line, false alarms at the detector's design rate among
 * them, and which entry is last line's target is left to the host.  This stage, behind the detector and on the device, is a
 * multi-target tracker in the lag-Doppler plane -- a Kalman filter per track, gating, a deterministic global-nearest-neighbour
 * assignment, M-of-N confirmation, coasting through missed detections, Doppler wrap -- in fp64, in ONE workgroup per submit that loops
 * over the lines, with its state carried from submit to submit.  The host fetches a short table of tracks in place of the lists.  It is
 * off until crsdr_caf_set_track; off, a submit is the same launches and the same bits, in every combination of canceller, detector,
 * bearings and beams.
 *
 * Source.  The measurements of a line are the slots q < min(count, K) of ONE detection list, K the detector's max_det:
 *     CRSDR_TRACK_SRC_ARRAY   the array map's list (det entry nrows).  With bearings on the auxiliary pair of a detection is
 *                             (cx + (x - cx), cy + (y - cy)) from its dir record, the two sums in fp64; with bearings off (-1, -1).
 *     CRSDR_TRACK_SRC_FUSED   the fused list of the beams.  The auxiliary pair is (beam index, -1).
 * A measurement is z = (lag + dlag, doppler + ddop), each the sum of the two published fp32 figures in fp64; its power and snr are
 * copied from the record.  A slot whose lag or Doppler lies outside the map, or whose dlag or ddop is not finite (hand-made lists only),
 * is no measurement.
 * State.  T = max_tracks slots.  A live track has x = (r, f, g) -- lag in cells, Doppler in bins, Doppler rate in bins per line -- a
 * symmetric 3 x 3 covariance P, an id, a status (1 tentative, 2 confirmed), age, hits, consecutive misses and a 32-bit hit history;
 * everything fp64 or an integer.  With H = nd / 2, wrap(v) is the value of v in [-H, H) modulo nd; it is applied to f after every
 * prediction and update, and to every Doppler innovation.
 * Per line, in this order:
 *  1. Predict every live track.  r' = r + coupling (f + g / 2), f' = wrap(f + g), g' = g; P' = F P F^T + diag(q_r, q_f, q_g) with F
 *     that map's Jacobian.  coupling is the caller's figure in lag cells per line per Doppler bin; it may be 0 and its sign is the
 *     caller's.
 *  2. Range exit.  A track whose predicted r is < -1 or > R ends this line with status 3 and takes no further part: it is reported
 *     with its predicted state, its counts as they were, slot -1.
 *  3. Gate.  For track slot i and measurement slot j: nu = (z_r - r', wrap(z_f - f')), S = P'[0:2, 0:2] + diag(sigma_r^2, sigma_f^2),
 *     d2 = nu^T S^-1 nu by the closed 2 x 2 inverse.  The pair is a candidate iff d2 <= gate.
 *  4. Assign: greedy global nearest neighbour under a strict total order.  The candidates are sorted by (d2, i, j) ascending and walked
 *     in that order; a candidate is taken iff its track and its measurement are both still free.  That sentence is the definition; the
 *     device takes, in rounds, every candidate that is the first of its row and of its column among the free ones, which gives the
 *     same set.
 *  5. Update every assigned track: K = P' H^T S^-1, x = x' + K nu, f wrapped, P = P' - K S K^T, symmetrised by copying the upper
 *     triangle; hits + 1, misses = 0, history << 1 | 1; it remembers its measurement's slot, d2, power, snr and auxiliary pair.
 *     Coast every other live track: x = x', P = P', misses + 1, history << 1; the remembered power, snr and pair stay.
 *     age + 1 for both.
 *  6. Status.  A tentative track becomes confirmed when the popcount of the low N history bits is >= M; otherwise it ends (status 3)
 *     when misses >= tent_miss or age >= N.  A confirmed track ends when misses >= conf_miss.  A slot that ended in this line is
 *     reported once with status 3 and its last state; it is free from the next line on, never within this one.
 *  7. Initiate.  Every unassigned measurement, in slot order, starts a tentative track in the lowest slot that was free at the start
 *     of the line: x = (z_r, wrap(z_f), 0), P = diag(sigma_r^2, sigma_f^2, p0_g), age = 0, hits = 1, history 1, id = the engine's
 *     counter, which then advances; it runs 1 .. 2^24 - 1 and continues at 1.  With no slot left the measurement is dropped and counted.
 * Outputs per line:
 *     trk  [nest][T][16] float    (id, status (0 free, 1, 2, 3), r, f, g, sqrt(P00), sqrt(P11), age, hits, misses, the measurement slot of
 *                                 this line or -1, its d2 or 0, power, snr, aux0, aux1), each rounded once from fp64, the integers
 *                                 exact; free slots all zero
 *     ntrk [nest][4] int32        live tracks after the line, confirmed, initiated, dropped
 * Carry-over and bits.  The state after the last line of a submit is the state before the first line of the next; crsdr_caf_track_reset
 * empties it, and so does crsdr_caf_set_track.  A sequence of lines gives the same trk and ntrk bytes however it is cut into submits.
 * The carry-over makes consecutive submits depend on each other: they must be ordered -- on one stream (the engine's own, or a plan's
 * through crsdr_caf_submit_plan), or by the caller waiting for one before the next goes to another stream.  Two submits in flight on
 * streams that nothing orders would both read and write the table; no other stage of crsdr_caf has that dependence.
 * Nothing depends on the order in which waves or atomics arrive, and crsdr_track launches the same kernel on the same arguments.
 * Limits, all CRSDR_EINVAL and all checked before a device is touched, by one function for the engine and the per-op call:
 * 1 <= max_tracks <= 128; a valid source; sigma_r, sigma_f, gate, p0_g finite and > 0; q_r, q_f, q_g finite and >= 0; coupling finite;
 * 1 <= m <= n <= 32; tent_miss, conf_miss >= 1. */
enum { CRSDR_TRACK_SRC_ARRAY = 0, CRSDR_TRACK_SRC_FUSED = 1 };

typedef struct crsdr_caf_track_desc {
    int32_t max_tracks;       /* T: track slots, 1..128 */
    int32_t source;           /* CRSDR_TRACK_SRC_* */
    double sigma_r, sigma_f;  /* measurement deviations: lag cells, Doppler bins */
    double gate;              /* on d2 */
    double p0_g;              /* variance of the Doppler rate of a new track */
    double q_r, q_f, q_g;     /* process noise per line */
    double coupling;          /* lag cells per line per Doppler bin */
    int32_t m, n;             /* confirmation: m hits in the last n lines */
    int32_t tent_miss;        /* consecutive misses that end a tentative track */
    int32_t conf_miss;        /* ... a confirmed one */
} crsdr_caf_track_desc;

/* Sets the tracker (NULL: off) and empties its state.  Between submits only: it waits for the last one and allocates here, never in a
 * submit.  CRSDR_ESTATE while the detector is off, and for the fused source unless beams with detection are on.  While the tracker is
 * on crsdr_caf_set_cfar, crsdr_caf_set_bearing and crsdr_caf_set_beams return CRSDR_ESTATE: turn it off first.  With the tracker on a
 * submit issues ONE launch more than without, whatever the number of blocks and whatever the counts (crsdr_caf_last_submit). */
int crsdr_caf_set_track(crsdr_caf *caf, const crsdr_caf_track_desc *desc);

/* Empties the table and starts the ids again at 1 (it waits for the last submit).  CRSDR_ESTATE with the tracker off. */
int crsdr_caf_track_reset(crsdr_caf *caf);

/* Waits for the last submit and copies out what is asked for (either pointer may be NULL), laid out as above.  CRSDR_ESTATE with the
 * tracker off, or before the first submit since it was set. */
int crsdr_caf_fetch_track(crsdr_caf *caf, float *trk, int32_t *ntrk);

/* Device addresses of trk and ntrk ([max_batch / frames] lines each).  They change with every crsdr_caf_set_track.  CRSDR_ESTATE with
 * the tracker off. */
int crsdr_caf_track_device_buffers(crsdr_caf *caf, void **trk, void **ntrk);

/* *bytes = the size of the per-op call's state buffer: a 16-byte header and 128 bytes per slot.  Host only; the limits above. */
int crsdr_track_state_bytes(const crsdr_caf_track_desc *desc, size_t *bytes);

/* The per-op form on nlines lines of hand-made or fetched lists: det [nlines][K][8] and count [nlines] as crsdr_cfar, the engine or
 * crsdr_beam_fuse wrote them (only lag, Doppler, dlag, ddop, power and snr are read from a record), aux [nlines][K][2] or NULL for
 * (-1, -1).  state is an in/out buffer of crsdr_track_state_bytes bytes; zero-filled means empty.  trk [nlines][T][16], ntrk
 * [nlines][4]; either may be NULL, not both.  1 <= nlines <= 4096, 1 <= K <= 64, nd a power of two in 8 .. 4096, 1 <= R <= 1024; desc's
 * source must be valid and is not used otherwise.  The engine's kernel on the same arguments, bit for bit.  mem_kind: CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE
 * (every pointer on the device; det, count, aux, trk and ntrk 4-byte, state 8-byte aligned). */
int crsdr_track(float *trk, int32_t *ntrk, void *state, const float *det, const int32_t *count, const float *aux, int nlines, int K,
                int nd, int R, const crsdr_caf_track_desc *desc, int mem_kind);

/* Integration across lines.  Every stage ahead of the tracker treats a line on its own, so an echo that does not clear the threshold in
 * one line's map never reaches the lists.  This stage, behind the maps and ahead of the detector, is the non-coherent integration of
 * consecutive maps along the range walk: between two lines a target at Doppler bin f walks coupling * f lag cells (the tracker's
 * prediction r' = r + coupling (f + g / 2) knows the same figure), so before every update the accumulated map is shifted along the lags
 * by a whole number of cells per Doppler bin -- exact, no interpolation, no blur that grows with time -- and the detector, unchanged,
 * runs on the integrated map.  The accumulator is fp64 and is carried from submit to submit like the tracker's table.  It is off until
 * crsdr_caf_set_integrate; off, a submit is the same launches and the same bits, in every combination of the other features.
 *
 * Definition.  P_m [nd][R] is the published fp32 map of line m; m = 0, 1, ... counts the lines since the last reset, across submits.
 * s(d) is the signed bin of the peaks.  The caller sets forget = a, 0 < a <= 1, and coupling = c in lag cells per line per Doppler bin:
 * the tracker's figure with the tracker's sign, and a tracker behind this stage should be given the same one.  The state is I [nd][R]
 * in fp64 and the counter m; empty is all zero and m = 0.
 * Per line, in this order:
 *  1. Offsets.  delta(d) = c * (double)s(d), one multiplication; o(m, d) = (int64) floor((double)m * delta(d) + 0.5), one multiplication
 *     and one addition; D(d) = o(m, d) - o(m - 1, d) for m >= 1, and D = 0 at m = 0.
 *  2. Shift, per Doppler bin, in whole cells, clamped at both ends of the lags: I'[d][tau] = I[d][min(max(tau - D(d), 0), R - 1)].  No
 *     arithmetic touches the values; lag does not wrap.
 *  3. Update.  lambda = max(a, 1.0 / (double)(m + 1)): the running mean until the window is full, exponential forgetting from then on.
 *     diff = (double)P - I', t = lambda * diff, I = I' + t: three fp64 operations, each rounded on its own, never contracted into an FMA,
 *     on the device or on the host.
 *  4. Output.  imap_m = (float)I, rounded once; the counter becomes m + 1.
 * Consequences.  At m = 0 imap = map bit for bit.  A sequence of lines gives the same imap bytes and the same final state however it is
 * cut into submits.  The carry-over makes consecutive submits depend on each other: they must be ordered -- on one stream (the engine's
 * own, or a plan's through crsdr_caf_submit_plan), or by the caller waiting for one before the next goes to another stream.  Nothing
 * depends on the order in which workgroups or waves run, and crsdr_map_integrate launches the same kernel on the same arguments.
 *
 * In the engine.  CRSDR_INTEGRATE_ARRAY: one launch behind the array map; the detector is handed imap where it is handed map without,
 * so entry nrows of det and count is the integrated map's; snap is still the current line's chi at those cells; the rows' entries, map,
 * peak and chi keep their bits.  CRSDR_INTEGRATE_BEAMS: one launch behind the beam maps, every (line, beam) map integrated on its own;
 * the beams' lists and the fused list are then ibmap's.  Each is ONE launch whatever the batch.  Bearings, fusion and the tracker follow
 * the lists they are given.
 * Limits, all CRSDR_EINVAL and all checked before a device is touched, by one function for the engine and the per-op call: forget finite
 * and in (0, 1]; coupling finite and |coupling| * (nd / 2) <= 1024; what a non-empty subset of the two flags. */
enum { CRSDR_INTEGRATE_ARRAY = 1, CRSDR_INTEGRATE_BEAMS = 2 };

typedef struct crsdr_caf_integrate_desc {
    int32_t what;             /* CRSDR_INTEGRATE_* */
    int32_t reserved;         /* 0 */
    double forget;            /* a: the weight of a new line once the window is full, (0, 1] */
    double coupling;          /* c: lag cells per line per Doppler bin */
} crsdr_caf_integrate_desc;

/* Sets the integration (NULL: off) and empties its state.  Between submits only: it waits for the last one and allocates here, never in
 * a submit.  CRSDR_ESTATE while bearings or the tracker are on -- the lists this changes are their input: the order is detector / beams,
 * integration, bearings, tracker -- and for CRSDR_INTEGRATE_BEAMS with beams off.  While integration is on crsdr_caf_set_beams returns
 * CRSDR_ESTATE (turn it off first); crsdr_caf_set_cfar and crsdr_caf_set_cfar_estimator stay allowed: the detector owns no integration
 * buffer. */
int crsdr_caf_set_integrate(crsdr_caf *caf, const crsdr_caf_integrate_desc *desc);

/* Empties the state: all zero, m = 0 (it waits for the last submit).  CRSDR_ESTATE with integration off. */
int crsdr_caf_integrate_reset(crsdr_caf *caf);

/* Waits for the last submit and copies out what is asked for (either pointer may be NULL): imap [nest][nd][R], ibmap
 * [nest][nbeams][nd][R].  CRSDR_ESTATE with integration off, before the first submit since it was set, or for a map whose flag is off. */
int crsdr_caf_fetch_integrate(crsdr_caf *caf, float *imap, float *ibmap);

/* Device addresses ([max_batch / frames] lines of maps; NULL for a map whose flag is off).  state: the array map's block, then the beam
 * maps', each laid out as crsdr_map_integrate's state for its number of maps; a block whose flag is off is not there.  They change with
 * every crsdr_caf_set_integrate.  CRSDR_ESTATE with integration off. */
int crsdr_caf_integrate_device_buffers(crsdr_caf *caf, void **imap, void **ibmap, void **state);

/* *bytes = the size of the per-op call's state buffer: a 16-byte header (int64 m, int64 0) and nmaps nd R doubles.  Host only; nd a
 * power of two in 8 .. 4096, 1 <= R <= 1024, nmaps >= 1 and nmaps nd R <= 2^24. */
int crsdr_map_integrate_state_bytes(int nmaps, int nd, int R, size_t *bytes);

/* The per-op form on nlines lines of nmaps maps each: maps [nlines][nmaps][nd][R] -> imap of the same shape; every map of a line is
 * integrated on its own.  state is an in/out buffer of crsdr_map_integrate_state_bytes bytes; zero-filled means empty.  1 <= nlines <=
 * 4096, nlines nmaps nd R <= 2^26; desc's what is not read.  The engine's kernel on the same arguments, bit for bit.  mem_kind:
 * CRSDR_MEM_HOST (copied) or CRSDR_MEM_DEVICE (every pointer on the device; maps and imap 4-byte, state 8-byte aligned). */
int crsdr_map_integrate(float *imap, void *state, const float *maps, int nlines, int nmaps, int nd, int R,
                        const crsdr_caf_integrate_desc *desc, int mem_kind);

#ifdef __cplusplus
}
#endif
#endif /* CRSDR_H */
