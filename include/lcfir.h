/*
 * lcfir.h -- C ABI of the MI355X (gfx950) low-cut FIR hot path.
 *
 * This is the drop-in boundary for the reference's hot path
 * (diskerror/audio-fir-filter, "lowcut"):
 *
 *   void apply_filter_range(const VectorMath<float32_t>& channel,
 *                           const WindowedSinc<float64_t>& sinc,
 *                           VectorMath<float32_t>& temp_output,
 *                           int_fast64_t startIdx, int_fast64_t endIdx,
 *                           ThreadSafeProgress* progress);      FilterCore.h:20-27
 *
 * called by N std::threads on disjoint [start,end) chunks of one channel
 * (ProcessFile.cp:60-83), plus the per-file peak/normalize post-pass
 * (ProcessFile.cp:91-101).  Every entry point below names the reference
 * interface it replaces.  Plain C: no exceptions cross this boundary, every
 * function returns an lcfir_status, and lcfir_last_error() holds a
 * thread-local message for the last failure on the calling thread.
 *
 * Semantics of a filtered sample (zero-padded, centred linear convolution,
 * output length = input length):
 *     y[n] = (float) sum_{k=0}^{T-1} h[k] * x[n - M/2 + k],   x[i] = 0 outside [0, N)
 * with T = M + 1 odd taps (WindowedSinc kernel length, getMo2() = M/2),
 * f32 samples, f64 taps, f64 accumulation, one round-to-nearest-even to f32.
 *
 * The samples' value domain (a float source can hold any bit pattern;
 * tests/test_gpu_value_domain.py):
 *   - direct method: exact support.  y[n] depends on x[n - M/2, n + M/2]
 *     alone, so one NaN or +-Inf sample makes exactly the T outputs whose taps
 *     reach it non-finite, as the reference's fms() would (Inf times a zero
 *     tap, and Inf - Inf, are NaN); every other output keeps its bits.
 *   - FFT method: overlap-save mixes a segment's samples, so every output of
 *     a segment whose input window (lcfir_ctx_window of the segment's outputs)
 *     holds a non-finite sample becomes non-finite.  Nothing else changes:
 *     the other segments, the other channels and their peaks, the buffer a
 *     fused normalize rescales, and later calls on the same ctx keep their bits.
 *   - Finite samples whose sum passes f32's range narrow to +-Inf.
 *   - The peak is max |y| with NaN skipped and Inf taken (0 for a channel of
 *     NaN).  A peak of Inf normalizes with gain 1 / Inf = 0: finite samples
 *     become signed zeros, Inf and NaN become NaN, as `if (maxMag > 1.0f)
 *     normalize()` (ProcessFile.cp:98-101) would with a scale of 1 / maxMag.
 *   - Scale invariance: y(2^k x) = 2^k y(x) bit for bit, for every method,
 *     wherever both sides are normal f32 (power-of-two scaling is exact in
 *     f64 fma, mul and add); nothing has an absolute floor.
 *   - Subnormal samples, outputs and peaks are honoured: nothing flushes to 0.
 *   - The f32 codec formats move bits (NaN payloads survive decode and encode).
 *
 * The taps' value domain (tests/test_gpu_tap_domain.py):
 *   - Every tap must be a finite double.  lcfir_ctx_create returns LCFIR_EINVAL
 *     for a NaN or +-Inf tap and names the first such index, before any device
 *     call: the methods could not agree on one (the direct kernel multiplies a
 *     channel edge's zero padding by it, 0 * Inf = NaN, where the reference's
 *     shortened sums never reach it; the FFT's tables would be all NaN).
 *   - Any finite taps are honoured: symmetric, antisymmetric, one-sided, all
 *     zero (every output and peak 0).  Nothing assumes a low-cut's shape.
 *   - Delays are exact.  A single unit tap h[k] = 1 gives y[n] = x[n + k - M/2]
 *     bit for bit, and h[M/2 - d] = h[M/2 + d] = 0.5 gives (x[n-d] + x[n+d]) / 2
 *     correctly rounded, for every method wherever the expected output is
 *     not 0 (samples on the 16-bit grid; the FFT's f64 error, 2^-50 |h|_1 max|x|,
 *     is far below half an f32 spacing there); the direct method's zeros are
 *     exact, the FFT's within 1e-12.
 *   - Scale invariance holds in the taps too: y(2^s h) = 2^s y(h) bit for bit
 *     wherever both sides are normal f32, for every method, with the same
 *     plan; no threshold on the taps is absolute.
 *   - Taps symmetric up to an antisymmetric part of 2^-50 of their l1 norm run
 *     the FFT's zero-phase form (lcfir_ctx_fft_info); anything above runs the
 *     general table.
 */
#ifndef LCFIR_H
#define LCFIR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LCFIR_ABI_VERSION 1

typedef struct lcfir_ctx lcfir_ctx;

typedef enum lcfir_status {
    LCFIR_OK = 0,
    LCFIR_EINVAL = 1,    /* bad argument (null pointer, even tap count, bad range) */
    LCFIR_EDEVICE = 2,   /* HIP runtime / device error */
    LCFIR_ENOMEM = 3,    /* device or host allocation failed */
    LCFIR_EINTERNAL = 4
} lcfir_status;

/* How the convolution is evaluated.  All methods meet the same parity bar. */
typedef enum lcfir_method {
    LCFIR_METHOD_AUTO = 0,   /* fastest method for the tap count: direct below 64 taps, else FFT */
    LCFIR_METHOD_DIRECT = 1, /* strict-order f64 FMA chain per output (bit-exact vs the
                                oracle's ORACLE_FMA restatement) */
    LCFIR_METHOD_FFT = 2     /* f64 overlap-save FFT convolution, any T up to 2^20 taps (longer
                                than ~10 900 taps: equal partitions summed in f64) */
} lcfir_method;

/* Progress callback: `count` more samples finished.  Replaces
 * ThreadSafeProgress::report(size_t) (ProgressBar.h:69-81). */
typedef void (*lcfir_progress_fn)(void *user, uint64_t count);

/* ---- library --------------------------------------------------------- */
int lcfir_abi_version(void);
const char *lcfir_last_error(void);
/* The library's build id: 16 hex digits of the SHA-256 of the sources it was
 * built from (audio-fir-filter_amd/src_hash.sh), "unknown" for a build outside
 * the Makefile.  bench.py matches PMC sidecars (profiles/traffic_*.json) to
 * the loaded library by it. */
const char *lcfir_build_id(void);
int lcfir_device_count(int *count);

/* ---- filter context ---------------------------------------------------- */
/* Uploads the taps to `device` once.  Replaces the per-file construction of
 * WindowedSinc<float64_t> (ProcessFile.cp:47-50) as seen by the hot path:
 * taps = the kernel, ntaps = M + 1 (must be odd), half = getMo2()
 * (FilterCore.h:29). */
int lcfir_ctx_create(int device, const double *taps, int32_t ntaps, lcfir_ctx **out);
/* Waits for the streams the ctx launched on (not the whole device) and frees
 * its device memory in stream order.  The caller must not destroy a stream
 * that still has work of this ctx queued before calling it. */
int lcfir_ctx_destroy(lcfir_ctx *ctx);
int lcfir_ctx_set_method(lcfir_ctx *ctx, int method);
int lcfir_ctx_get_method(const lcfir_ctx *ctx, int *method);
int lcfir_ctx_half(const lcfir_ctx *ctx, int32_t *half); /* getMo2() */
int lcfir_ctx_ntaps(const lcfir_ctx *ctx, int32_t *ntaps);
/* Diagnostic: the FFT plan this ctx runs (built if needed): overlap-save
 * segment length in real samples, the number of tap partitions, and whether
 * the filter runs in zero-phase form (linear-phase taps).  All 0 when the tap
 * count is outside the FFT method's range. */
int lcfir_ctx_fft_info(lcfir_ctx *ctx, int32_t *seg_len, int32_t *parts, int32_t *zero_phase);
/* Diagnostic: the unit geometry of the same plan.  *outputs: outputs per
 * overlap-save segment (B = seg_len - taps per partition + 1); *kernel: which
 * kernel runs a unit (LCFIR_FFT_KERNEL_*); *nrm_floats: the most floats of a
 * previous file's normalize (lcfir_filter_window_norm_dev) one unit carries
 * inside the filter launch, 0 when that kernel never carries one.  A call
 * fuses the normalize iff d_ny is 16-byte aligned and
 * ceil(ceil(ncount / U) / blk) x blk <= *nrm_floats, where
 * U = nseg x max(1, min(nch, max_units / nseg)) units share it,
 * nseg = ceil(outputs of the call's first launch chunk / B), max_units is
 * lcfir_ctx_set_fft_tuning's (2^31 - 1 by default) and blk = 2 048 floats on
 * the register kernel (LCFIR_FFT_KERNEL_L32_REG), 1 024 on the others.  All 0
 * when the tap count is outside the FFT method's range. */
#define LCFIR_FFT_KERNEL_L16 1      /* fir_fft_f64_kernel: L = 16 384, LDS columns */
#define LCFIR_FFT_KERNEL_L32_PARK 2 /* fir_fft32_f64_kernel: L = 32 768, two halves + park slab */
#define LCFIR_FFT_KERNEL_L32_REG 3  /* fir_fft32r_kernel: L = 32 768 held in registers (zero-phase) */
int lcfir_ctx_fft_units(lcfir_ctx *ctx, int32_t *outputs, int32_t *kernel, int32_t *nrm_floats);
/* Diagnostic: how many previous-file normalizes (lcfir_filter_window_norm_dev
 * with ncount > 0) this ctx carried inside its filter launch (*fused) and how
 * many it ran as their own pass (*separate) since it was created. */
int lcfir_ctx_nrm_stats(const lcfir_ctx *ctx, int64_t *fused, int64_t *separate);
/* Explicit FFT-method choices for this ctx (the library reads no environment
 * variables).  seg_len: 0 = automatic, or 16384 / 32768.  Automatic picks the
 * length with the lower estimated time per output for the taps alone: tap
 * partitions x the measured unit cost (a 32768-sample unit costs 2.2
 * 16384-sample ones on the register kernel, 2.9 on the park-slab kernel) /
 * outputs per segment.  It never depends on a call's
 * shape, so every call on a ctx (range, window, channels, fft_info; every
 * thread, rank or device stage) runs the same plan and the same bytes,
 * whichever call comes first.  zero_phase: 1 = linear-phase filters run in zero-phase form (the
 * default), 0 = always the general pair table; chunk: outputs per launch
 * chunk (0 = 2^28, else >= 4096); max_units: segments x channels per launch
 * (0 = 2^31 - 1).  Every setting gives outputs within 1 f32 ulp of every
 * other (the tests run each); the defaults are the fast ones.  Waits for the
 * ctx's queued launches and drops its plan; not to be called concurrently
 * with launches on the same ctx. */
int lcfir_ctx_set_fft_tuning(lcfir_ctx *ctx, int32_t seg_len, int32_t zero_phase, int64_t chunk,
                             int64_t max_units);
/* Which kernel family runs the ctx's zero-phase single-partition plans:
 * DEFAULT = the transform held in registers at L = 32 768 (fir_fft32r), the
 * LDS-column kernel at L = 16 384; LDS = the LDS-column kernels
 * (fir_fft_f64_kernel, fir_fft32_f64_kernel), which every other plan runs.
 * Outputs agree within 1 f32 ulp either way (tests run each); waits for the
 * ctx's queued launches and drops its plan, as lcfir_ctx_set_fft_tuning.
 * Any other value (2 named round 5's experimental register family, now
 * outside the library) fails with LCFIR_EINVAL. */
#define LCFIR_FFT_FAMILY_DEFAULT 0
#define LCFIR_FFT_FAMILY_LDS 1
int lcfir_ctx_set_fft_family(lcfir_ctx *ctx, int family);
/* Input window [*lo, *hi) (within [0, n)) of a channel of n samples that
 * makes a call for outputs [start, end) reproduce the whole-channel call's
 * outputs bit for bit, whatever the range: the partition invariance of
 * FilterCore.h's per-thread ranges (ProcessFile.cp:60-83).  The direct
 * method needs [start - half, end + half); the FFT method needs the samples
 * of the whole segments the range touches (its segment grid is anchored at
 * output 0), a few thousand more.  A narrower window that still covers
 * [start - half, end + half) gives outputs within 1 f32 ulp of those.
 * Builds the FFT plan if needed. */
int lcfir_ctx_window(lcfir_ctx *ctx, int64_t n, int64_t start, int64_t end, int64_t *lo, int64_t *hi);

/* ---- the hot path: host-pointer range call ----------------------------- */
/* Replaces apply_filter_range(channel, sinc, temp_output, startIdx, endIdx,
 * progress) (FilterCore.h:20-79).  x: the whole channel (n samples, host);
 * y: the caller's output buffer (n samples, host); only y[start, end) is
 * written; x is read over [start - half, end + half) intersected with [0, n).
 * Re-entrant: any number of host threads may call it concurrently on the
 * same ctx with disjoint ranges (the ProcessFile.cp:71-78 pattern).
 * progress may be NULL; otherwise it receives end - start once the range is
 * done (the reference batches reports every 2048 samples, FilterCore.h:38-54). */
int lcfir_apply_range(lcfir_ctx *ctx, const float *x, int64_t n, float *y, int64_t start,
                      int64_t end, lcfir_progress_fn progress, void *user);
/* lcfir_apply_range borrows a staging slot (a HIP stream + grow-only device
 * buffers) per call from a per-device pool of at most 16 slots; callers beyond
 * that wait for a free slot, so the reference's default of floor(0.7 cores)
 * threads per channel (main.cp:75) never creates a stream per thread.
 * lcfir_staging_release frees the idle slots of `device` (-1: every device),
 * and a device's two link queues (page-locked copies) once it has no slot left;
 * lcfir_staging_count reports the slots in existence and the idle ones. */
int lcfir_staging_release(int device);
int lcfir_staging_count(int device, int *live, int *idle);
/* How lcfir_apply_range moves the caller's (pageable) buffers over PCIe.
 * PAGEABLE: the caller's pointers go to hipMemcpyAsync as they are (the
 * runtime pins the pages itself: 35-56 GB/s each way for one thread's 115 MB
 * range on MI355X, but concurrent calls' copies run one at a time).  BOUNCE:
 * a call whose input window is 2-32 MiB (a multi-thread fan-out's share of a
 * channel) is copied whole by the calling thread into its staging slot's
 * page-locked buffers (grow-only, at most 32 MiB each, kept by the slot
 * until lcfir_staging_release; a slot that cannot page-lock them takes the
 * runtime's path) and moved over the
 * device's shared link queues, both ways at once; other calls through two
 * 4 MiB pinned chunks (slower than the runtime for one thread's whole
 * channel).  AUTO (the default): BOUNCE's whole-window path where it applies,
 * PAGEABLE otherwise (config 2's 16-thread fan-out: 0.31-0.45 of the
 * pinned-H2D bound against 0.19-0.22 pageable on one box, alternating).
 * Memory allocated page-locked (hipHostMalloc,
 * lcfir_host_malloc) is copied directly in every mode, on one H2D and one D2H
 * queue per device shared by all calls (the D2H by a kernel through the
 * buffer's device mapping when both ends are 16-byte aligned), so concurrent
 * calls use the link both ways at once.  hipHostRegister'd memory goes to
 * hipMemcpyAsync as it is (the runtime DMAs it directly, on the call's own
 * stream: ROCm 7.2 does not report a registration's extent, so the library
 * cannot prove a range lies in one).  Process-wide; takes effect at the next
 * call. */
typedef enum lcfir_staging_mode {
    LCFIR_STAGING_BOUNCE = 0,
    LCFIR_STAGING_PAGEABLE = 1,
    LCFIR_STAGING_AUTO = 2 /* the default */
} lcfir_staging_mode;
int lcfir_staging_set_mode(int mode);
/* Accounting of lcfir_apply_range calls since the last reset (process-wide).
 * Always: calls, outputs, bytes each way, bounce-staged calls, the calls'
 * host wall time (summed over calls, so concurrent calls add up).  With
 * lcfir_range_profile(1) each call also records HIP events (a few
 * microseconds per call), each on the queue that runs the step -- the
 * device's shared link queues for page-locked buffers of >= 2 MiB, else the
 * call's slot stream: H2D span (first DMA to last; bounce mode: first host
 * chunk copy to last DMA), kernel (samples landed to kernel end), D2H DMA
 * span, summed over the profiled calls.  The copy spans exclude any wait
 * behind other calls' copies on a shared link queue (round 6; round 5's
 * numbers included it). */
typedef struct lcfir_range_stats {
    uint64_t calls;
    uint64_t samples;
    uint64_t h2d_bytes;
    uint64_t d2h_bytes;
    uint64_t staged_calls;
    uint64_t profiled_calls;
    double wall_ms;
    double h2d_ms;
    double kernel_ms;
    double d2h_ms;
} lcfir_range_stats;
int lcfir_range_profile(int enable);
int lcfir_range_stats_get(lcfir_range_stats *out, int reset);

/* ---- device-resident variants (async on a hipStream_t passed as void*) -- */
/* Same as lcfir_apply_range with device pointers; no host synchronisation. */
int lcfir_apply_range_dev(lcfir_ctx *ctx, const float *d_x, int64_t n, float *d_y,
                          int64_t start, int64_t end, void *stream);

/* The whole per-channel loop of ProcessFile.cp:57-87 for nch deinterleaved
 * channels of n samples: channel c at d_x + c*x_stride, output at
 * d_y + c*y_stride (d_y must not alias d_x).  If d_peak is non-NULL it must
 * hold nch floats, zeroed by the caller (or by lcfir_peak_reset_dev); each
 * receives max|y| of its channel (fused into the filter kernel). */
int lcfir_filter_channels_dev(lcfir_ctx *ctx, const float *d_x, int64_t x_stride, int32_t nch,
                              int64_t n, float *d_y, int64_t y_stride, float *d_peak,
                              void *stream);

/* General windowed form, for a file sharded across processes/GPUs by sample
 * range: the caller holds only samples [x_lo, x_hi) of channels that are n
 * samples long (channel c's window at d_xw + c*x_stride, element 0 = sample
 * x_lo) and wants outputs [start, end) (channel c's at d_yw + c*y_stride,
 * element 0 = output y_lo).  The window must cover
 * [max(0, start - half), min(n, end + half)); lcfir_ctx_window's window
 * makes the outputs bit-identical to the whole-channel call's.  d_peak (nullable): channel c's
 * max|y| is max-ed into d_peak[c * peak_stride] (peak_stride 0 folds every
 * channel into one per-file slot, ProcessFile.cp:92-96). */
int lcfir_filter_window_dev(lcfir_ctx *ctx, const float *d_xw, int64_t x_lo, int64_t x_hi,
                            int64_t x_stride, int64_t n, int32_t nch, float *d_yw, int64_t y_lo,
                            int64_t y_stride, int64_t start, int64_t end, float *d_peak,
                            int64_t peak_stride, void *stream);

/* lcfir_filter_window_dev that also carries the PREVIOUS file's normalize
 * (ProcessFile.cp:98-101, applied per file by main.cp:132-147): the ncount
 * contiguous floats at d_ny are rescaled by 1/peak iff peak = max(d_npeak[0,
 * nnpeak)) > 1 or nforce -- exactly lcfir_normalize_dev(d_ny, ncount, 1,
 * ncount, d_npeak, nnpeak, nforce), bit for bit.  The peak slots must be
 * final when the call's work starts (written by earlier work on `stream`).
 * For single-partition FFT filters the rescale rides in the filter launch
 * (the workgroups' older waves do it while waiting at a barrier), so a batch
 * of files needs one normalize pass (the last file's) instead of one per
 * file; otherwise it runs as a separate pass after the filter.  d_ny must
 * not overlap the window or the outputs; ncount = 0 is a plain
 * lcfir_filter_window_dev call (d_ny, d_npeak may then be NULL). */
int lcfir_filter_window_norm_dev(lcfir_ctx *ctx, const float *d_xw, int64_t x_lo, int64_t x_hi,
                                 int64_t x_stride, int64_t n, int32_t nch, float *d_yw, int64_t y_lo,
                                 int64_t y_stride, int64_t start, int64_t end, float *d_peak,
                                 int64_t peak_stride, float *d_ny, int64_t ncount, const float *d_npeak,
                                 int32_t nnpeak, int nforce, void *stream);

/* ---- peak + normalize post-pass (ProcessFile.cp:91-101) ----------------- */
/* max_mag() over each channel (VectorMath::max_mag); d_peak[c] = max(d_peak[c], max|y_c|). */
int lcfir_peak_reset_dev(float *d_peak, int32_t count, void *stream);
int lcfir_peak_dev(const float *d_y, int64_t stride, int32_t nch, int64_t n, float *d_peak,
                   void *stream);
/* Per-file normalize decision and rescale, device-side (no host sync):
 * peak = max over d_peak[0..npeak); if (peak > 1 || force) every sample
 * becomes (float)((double)y * (1.0 / (double)peak)).  The scale rule of
 * c_lib's AudioSamples::normalize is unpinned. */
int lcfir_normalize_dev(float *d_y, int64_t stride, int32_t nch, int64_t n,
                        const float *d_peak, int32_t npeak, int force, void *stream);
/* lcfir_normalize_dev that also zeroes d_clear[0..nclear) in the same launch
 * (a batch driver's next-step peak slots: one launch per step fewer than a
 * separate lcfir_peak_reset_dev).  d_clear must not overlap d_peak[0..npeak)
 * (LCFIR_EINVAL).  nclear 0 = lcfir_normalize_dev. */
int lcfir_normalize_clear_dev(float *d_y, int64_t stride, int32_t nch, int64_t n,
                              const float *d_peak, int32_t npeak, int force, float *d_clear,
                              int32_t nclear, void *stream);
/* Host-pointer convenience: max|y| of one channel (VectorMath::max_mag). */
int lcfir_channel_peak(int device, const float *y, int64_t n, float *peak);

/* ---- tap design (host, long double) ---------------- */
/* Replaces `WindowedSinc<float64_t> sinc(freq / fs, slope / fs); sinc.makeLowCut();`
 * (ProcessFile.cp:47-50): dspguide ch.16 Blackman windowed-sinc low-pass with
 * unity DC gain, then spectral inversion to a high-pass (README.md:50,60-62).
 * Kernel length M + 1 with M = 4 / (slope / fs) rounded to the nearest even
 * integer (c_lib's exact rounding rule is unpinned).  Writes *ntaps; if taps
 * is non-NULL and cap >= *ntaps, also writes the taps.  -s 48 at 48 kHz
 * gives 4001 taps, -s 10 at 48 kHz 19 201. */
int lcfir_design_lowcut(double freq_hz, double slope_hz, double fs, double *taps, int32_t cap,
                        int32_t *ntaps);

/* ---- sample codec either side of the path -------- */
/* Interleaved PCM frames (WAV little-endian / AIFF big-endian) <-> the
 * deinterleaved float32 AudioBuffer the hot path works on.  Replaces, on the
 * device, c_lib's AudioSamples::readAll (ProcessFile.cp:40-41) and
 * AudioSamples::writeAll(buf, true) (:115-117), whose exact conventions are
 * unpinned; ours: int b-bit v <-> v / 2^(b-1), encode rounds half-to-even in
 * f64 and clamps to [-2^(b-1), 2^(b-1) - 1]; float32 is passed through. */
typedef enum lcfir_pcm_format {
    LCFIR_PCM_S16LE = 1,
    LCFIR_PCM_S24LE = 2, /* packed 3-byte */
    LCFIR_PCM_S32LE = 3,
    LCFIR_PCM_F32LE = 4,
    LCFIR_PCM_S16BE = 5,
    LCFIR_PCM_S24BE = 6,
    LCFIR_PCM_S32BE = 7,
    LCFIR_PCM_F32BE = 8
} lcfir_pcm_format;

int lcfir_pcm_bytes(int format); /* bytes per sample, 0 for an unknown format */
/* d_in: frames * nch interleaved samples; channel c goes to d_out + c*out_stride. */
int lcfir_decode_pcm_dev(const void *d_in, int format, int32_t nch, int64_t frames,
                         float *d_out, int64_t out_stride, void *stream);
/* Channel c is read from d_in + c*in_stride.  This is lcfir_encode_pcm_dither_dev
 * (below) with LCFIR_DITHER_NONE, no peak (d_peak NULL, npeak 0, force 0), seed
 * 0 and frame0 0: the same kernel, the same argument rules. */
int lcfir_encode_pcm_dev(const float *d_in, int64_t in_stride, int32_t nch, int64_t frames,
                         int format, void *d_out, void *stream);
/* lcfir_normalize_dev + lcfir_encode_pcm_dev in one pass (ProcessFile.cp:91-101
 * then :115-117): the normalize decision is taken from d_peak[0..npeak) on the
 * device and each sample is scaled exactly as lcfir_normalize_dev would scale
 * it before encoding -- byte-identical output, d_in is left unscaled.  This is
 * lcfir_encode_pcm_dither_dev with LCFIR_DITHER_NONE, seed 0 and frame0 0. */
int lcfir_encode_pcm_scaled_dev(const float *d_in, int64_t in_stride, int32_t nch, int64_t frames,
                                int format, const float *d_peak, int32_t npeak, int force,
                                void *d_out, void *stream);

/* ---- TPDF dither for the integer encode (opt-in) ------------------------- */
/* Plain rounding to 16 or 24 bits leaves an error correlated with the signal:
 * what a low-cut leaves of room tone or a fade, a few LSB, comes out as
 * harmonic distortion or as digital silence.  Triangular noise of +-1 LSB
 * added before the rounding makes the error's mean and variance independent
 * of the signal.  The noise is a pure function of (seed, channel, absolute
 * frame index of the file), never of a generator's state, so a file's bytes
 * do not depend on how its frames were cut into calls, devices or item-set
 * rows.  All integer arithmetic is modulo 2^64:
 *
 *   s = seed ^ ((uint64)(ch + 1) * 0xD1B54A32D192ED03)
 *   z = s + (uint64)frame * 0x9E3779B97F4A7C15
 *   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *   z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *   z =  z ^ (z >> 31)
 *   d = ((double)(z >> 32) - (double)(z & 0xFFFFFFFF)) * 2^-32
 *
 * d lies in (-1, 1) LSB, triangular, and every step is exact in f64.  The
 * dithered encode of a float v for a b-bit integer format is
 *
 *   q = rint((double)v * 2^(b-1) + d)
 *
 * (the product is exact, so the add is the only rounding), then the plain
 * encode's clamp to [-2^(b-1), 2^(b-1) - 1] and its NaN -> 0.  The float32
 * formats pass their bits through, dither or not.  With a rescale folded in,
 * v is first (float)((double)v * (1.0 / (double)peak)), as in
 * lcfir_encode_pcm_scaled_dev. */
#define LCFIR_DITHER_NONE 0
#define LCFIR_DITHER_TPDF 1

/* Pure host function, no device: d[i] = the noise of (seed, ch, frame0 + i),
 * in LSB, i in [0, count).  LCFIR_EINVAL: ch, frame0 or count negative,
 * frame0 + count overflowing int64, d NULL with count > 0. */
int lcfir_dither_tpdf(uint64_t seed, int32_t ch, int64_t frame0, int64_t count, double *d);
/* lcfir_encode_pcm_scaled_dev with the dither option.  frame0 is the absolute
 * index, within its file, of the first frame the call encodes: frame i of the
 * call takes the noise of frame0 + i, so a file encoded in ranges equals the
 * file encoded whole.  d_peak may be NULL when npeak is 0 (no rescale).  With
 * LCFIR_DITHER_NONE the output is lcfir_encode_pcm_scaled_dev's, byte for
 * byte (seed and frame0 are checked and otherwise unused).  LCFIR_EINVAL: an
 * unknown dither mode, a negative frame0, frame0 + frames overflowing int64;
 * otherwise lcfir_encode_pcm_scaled_dev's argument rules.  Where d_out is
 * 4-byte aligned the samples are stored as whole dwords, four samples a lane
 * (all but the buffer's last frames * nch % 4); any d_out is accepted. */
int lcfir_encode_pcm_dither_dev(const float *d_in, int64_t in_stride, int32_t nch, int64_t frames,
                                int format, const float *d_peak, int32_t npeak, int force,
                                int dither, uint64_t seed, int64_t frame0, void *d_out, void *stream);

/* ---- item sets: a batch of files of different lengths in few launches ---- */
/* The reference's batch scenario (main.cp:132-147) filters many files one
 * after another.  Every entry point above takes channels that share one
 * length, so a library of short files costs a launch per file.  An item set
 * lays the files' channels out as rows of one arena, zero-padded, grouped by
 * the number of work units their length needs, and filters each group with
 * one ordinary multi-channel launch: a row of n samples followed by physical
 * zeros, filtered with x_hi = end = N_g >= n, gives outputs [0, n) that are
 * bit-identical to the per-file call's (x = 0 outside [0, N) above; the
 * segment grid is anchored at output 0 of every row).  Outputs [n, N_g) of a
 * shorter row hold the filter's ringing tail, so the peak, the normalize and
 * the codec have forms of their own here that stop at each file's n.
 *
 * lcfir_items_plan: the layout rule, a pure function (no device).
 *   key     k = ceil(n / unit); files with n = 0 or nch = 0 get no rows
 *           (group -1, offset 0, stride 0);
 *   order   groups in ascending k, files within a group in input order;
 *   block   a file's nch rows are contiguous at its group's stride
 *           S_g = N_g rounded up to 4 floats, N_g = the group's largest n:
 *           an (nch, S_g) block the per-file calls accept as it is;
 *   align   every group, so every row, starts a multiple of 4 floats (16 B)
 *           into the arena;
 *   cut     a group of more than 65 535 rows runs as consecutive launches
 *           of whole files (nch > 65 535 is LCFIR_EINVAL).
 * Outputs, each nullable: per file (nfiles entries) its group, its first
 * row's arena offset in floats, its stride; per group (up to nfiles entries,
 * *ngroups written) N_g, the group's first row (rows numbered in arena
 * order) and its row count; the launch, row and arena-float totals.
 * Correctness never depends on the grouping (any N_g >= n gives the same
 * bytes; it only decides how many padded units run), so a plan made before
 * lcfir_ctx_set_fft_tuning / _set_method / _set_fft_family stays valid. */
int lcfir_items_plan(int64_t unit, int32_t nfiles, const int64_t *n, const int32_t *nch,
                     int32_t *file_group, int64_t *file_offset, int64_t *file_stride,
                     int32_t *ngroups, int64_t *group_n, int64_t *group_first_row, int64_t *group_rows,
                     int32_t *nlaunches, int64_t *nrows, int64_t *arena_floats);

/* The per-unit table of an item set: one entry per (row, segment) of every
 * file with rows, rows in arena order (lcfir_items_plan's), segments ascending
 * within a row.  Entry: the row's arena offset in floats (the file's offset +
 * channel * stride), the segment (outputs [seg B, min((seg + 1) B, n)) of the
 * row) and the FILE's frame count n, not the group's N_g.  A row of n frames
 * has ceil(n / B) entries, so the total is sum nch ceil(n / B).  A pure
 * function (no device).  *nunits always receives the total; entries (nullable
 * when cap = 0) is written only if cap >= the total, else nothing is written
 * and the call returns LCFIR_EINVAL.  n[f] > 2^31 - 1 on a file with rows is
 * LCFIR_EINVAL (the entry holds n in 32 bits). */
typedef struct lcfir_item_unit {
    int64_t off;
    int32_t seg;
    int32_t n;
} lcfir_item_unit;
int lcfir_items_unit_table(int64_t B, int32_t nfiles, const int64_t *n, const int32_t *nch, int64_t *nunits,
                           lcfir_item_unit *entries, int64_t cap);
/* The file of every entry of lcfir_items_unit_table, in its order: file[u] is
 * the index (into n / nch) of the file whose row entry u belongs to.  A pure
 * function (no device) with the unit table's count, order and cap rules:
 * *nunits always receives the total, file (nullable when cap = 0) is written
 * only if cap >= the total, else nothing is written and the call returns
 * LCFIR_EINVAL; files with n = 0 or nch = 0 have no entry.  No launch reads it
 * yet: it is the slot table a per-file peak fused into the item kernels needs
 * (scripts/variants/items_peak/). */
int lcfir_items_unit_files(int64_t B, int32_t nfiles, const int64_t *n, const int32_t *nch, int64_t *nunits,
                           int32_t *file, int64_t cap);

typedef struct lcfir_items lcfir_items;
/* Plans nfiles files (n[f] frames, nch[f] channels) with unit = the outputs
 * per work unit of the ctx's method as resolved now (lcfir_ctx_fft_units'
 * *outputs for the FFT method, 4 096 for the direct form), allocates an input
 * and an output arena of the planned length on the ctx's device, zeroes the
 * input arena once and uploads the tile tables the passes below walk.  If the
 * ctx's plan is then an FFT plan on an LDS-column kernel (LCFIR_FFT_KERNEL_L16
 * or _L32_PARK), of one partition or of several, the per-unit table
 * (lcfir_items_unit_table at that plan's outputs per unit) is uploaded too and
 * its B recorded: what the fused filter launches below walk (16 bytes per
 * entry; the table alone changes nothing about which path a call takes).  The
 * ctx must outlive the item set's lcfir_items_filter_dev calls.  An item set
 * serves one stream at a time: calls on one stream run in order; the caller
 * orders a change of stream itself. */
int lcfir_items_create(lcfir_ctx *ctx, const int64_t *n, const int32_t *nch, int32_t nfiles,
                       lcfir_items **out);
/* Waits for the streams the item set launched on, then frees its memory. */
int lcfir_items_destroy(lcfir_items *items);
/* File f's block of rows in each arena: channel c at *d_x + c * *stride
 * (input) and *d_y + c * *stride (output); NULL, NULL, 0 for a file without
 * rows.  The caller writes ONLY [0, n_f) of each input row: the zeros
 * behind them are what makes a row's outputs the per-file call's.  Output
 * rows hold the result in [0, n_f) and unspecified values beyond. */
int lcfir_items_file(const lcfir_items *items, int32_t f, float **d_x, float **d_y, int64_t *stride);
int lcfir_items_info(const lcfir_items *items, int32_t *groups, int32_t *launches, int64_t *rows,
                     int64_t *arena_floats);
/* Filters every file, then, if d_peak is non-NULL, one launch that max-es
 * each file's max|y| over its channels and over [0, n_f) only into
 * d_peak[f] (nfiles floats, zeroed by the caller as for
 * lcfir_filter_channels_dev; NaN skipped, Inf taken).
 * Per-group path (the default): one ordinary multi-channel launch per group
 * launch (x_hi = end = N_g, no fused peak); outputs [n, N_g) of a shorter row
 * then hold the ringing tail.
 * Fused path (lcfir_items_set_fusion): ONE filter launch for all groups, the
 * item form of the plan's FFT kernel walking the per-unit table: every unit
 * runs with exactly the parameters the per-file call gives it (x_hi = end =
 * the file's n), so outputs [0, n) are lcfir_filter_channels_dev's bytes and
 * nothing of a row past n is written.  Taken when fusion is
 * LCFIR_ITEMS_FUSION_AUTO, the ctx's current plan is FFT with one partition on
 * an LDS-column kernel (LCFIR_FFT_KERNEL_L16 or _L32_PARK; the register kernel
 * has no item form) with the table's B, and every row is at most one launch
 * chunk long (the `chunk` tuning; 2^28 outputs by default); a max_units
 * tuning splits it into consecutive launches of that many entries.  Otherwise
 * (the direct method, a partitioned plan, a register-kernel plan, a seg_len
 * changed after create, a row longer than a chunk) the per-group path.
 * Fused partitioned path (LCFIR_ITEMS_FUSION_PARTS only): a plan of P > 1
 * partitions on an LDS-column kernel runs P launches over the same table, in
 * the order first, add ... add, last, each with the parameters the per-file
 * call gives that partition of that unit (half - part * the partition's taps;
 * one chunk, start = 0, x_hi = end = n), so the partial sums, their adds and
 * the final rounding are lcfir_filter_channels_dev's and outputs [0, n) are
 * its bytes.  The f64 partial sums live in the stream's FFT scratch, one
 * double per arena float (each row's slice at the row's own arena offset),
 * behind the park kernel's slab: the call grows that scratch to
 * 8 * arena_floats bytes (+ the slab) where the per-group path needs one
 * group's rows at a time; if that allocation fails the call returns
 * LCFIR_ENOMEM and LCFIR_ITEMS_FUSION_GROUPS is the way out.  The first
 * launch writes every output of every row's [0, n) before the later ones read
 * it, so stale scratch never reaches an output.  Taken when the plan is FFT,
 * not on the register kernel, has the table's B, and every row is at most one
 * launch chunk long (2^26 outputs for a partitioned plan, or the `chunk`
 * tuning if lower); with one partition PARTS is exactly AUTO's launch; a
 * max_units tuning splits the table as above, P launches per slice.
 * Every path gives the same bytes in [0, n) of every row.  Allocates nothing
 * beyond the stream's FFT scratch, as the filter launches do, so it captures
 * into a HIP graph under their rule (an eager call on the stream first sizes
 * the FFT scratch; a capture that would have to grow it is LCFIR_EINVAL). */
int lcfir_items_filter_dev(lcfir_items *items, float *d_peak, void *stream);
/* How lcfir_items_filter_dev picks its path: GROUPS (the default, DESIGN.md
 * s4.8) always runs the per-group launches, AUTO fuses single-partition plans
 * where the rule above allows and leaves a partitioned plan on the per-group
 * path, PARTS does what AUTO does and also fuses partitioned plans on the
 * LDS-column kernels (one launch per partition).  PARTS is 3, not 2: callers
 * and tests written against the two-mode header use 2 as "an unknown mode",
 * and it stays LCFIR_EINVAL, like every other value. */
#define LCFIR_ITEMS_FUSION_AUTO 0
#define LCFIR_ITEMS_FUSION_GROUPS 1
#define LCFIR_ITEMS_FUSION_PARTS 3
int lcfir_items_set_fusion(lcfir_items *items, int mode);
/* What the next lcfir_items_filter_dev would launch under the ctx's plan as it
 * is now: the fused path's launches (parts * ceil(entries / max_units): 1 for
 * a single-partition plan unless a max_units tuning splits the table, one per
 * partition and slice on the fused partitioned path) and the table entries
 * they run; on the per-group path
 * lcfir_items_info's launches (the plan's group launches; each still runs one
 * kernel per chunk and partition) and 0 entries.  The peak launch is not
 * counted. */
int lcfir_items_filter_launches(lcfir_items *items, int32_t *filter_launches, int64_t *fused_units);
/* One launch: file f's output rows [0, n_f) become
 * (float)((double)y * (1.0 / (double)d_peak[f])) iff (d_peak[f] > 1 or
 * force) and d_peak[f] > 0 -- lcfir_normalize_dev per file with npeak = 1
 * and the file's own slot, bit for bit. */
int lcfir_items_normalize_dev(lcfir_items *items, const float *d_peak, int force, void *stream);
/* One launch each: lcfir_decode_pcm_dev into every file's input rows /
 * lcfir_encode_pcm_scaled_dev (npeak = 1, the file's own slot; the output
 * rows stay unscaled) from every file's output rows.  d_bytes: one device
 * buffer holding every file's interleaved payload, file f's at
 * byte_offset[f] in format[f] (lcfir_pcm_format); byte_offset and format are
 * host arrays of nfiles entries, copied before the call returns (entries of
 * files without rows are ignored).  These two calls cannot be captured into a
 * HIP graph (the per-call table is uploaded from the host).
 * lcfir_items_encode_pcm_scaled_dev is lcfir_items_encode_pcm_dither_dev
 * (below) with LCFIR_DITHER_NONE and seed 0, except that it rejects a NULL
 * d_peak where any file has rows. */
int lcfir_items_decode_pcm_dev(lcfir_items *items, const void *d_bytes, const int64_t *byte_offset,
                               const int32_t *format, void *stream);
int lcfir_items_encode_pcm_scaled_dev(lcfir_items *items, const float *d_peak, int force, void *d_bytes,
                                      const int64_t *byte_offset, const int32_t *format, void *stream);
/* lcfir_items_encode_pcm_scaled_dev with the dither option, one launch: every
 * file's noise is keyed on its own channel and frame index (frame0 = 0) with
 * the one seed, so file f's bytes are those of lcfir_encode_pcm_dither_dev on
 * that file alone (npeak = 1, its own slot), whatever else is in the batch.
 * d_peak may be NULL (no file is rescaled).  LCFIR_EINVAL for an unknown
 * dither mode; like the two calls above it cannot be captured into a HIP
 * graph. */
int lcfir_items_encode_pcm_dither_dev(lcfir_items *items, const float *d_peak, int force, int dither,
                                      uint64_t seed, void *d_bytes, const int64_t *byte_offset,
                                      const int32_t *format, void *stream);
/* The way in and out for files that already sit in device memory of the
 * caller's (torch tensors, say), one launch each whatever the file count.
 * d_src / d_dst and the strides are host arrays of nfiles entries, copied
 * before the call returns: entry f is the device pointer to channel 0 of file
 * f and the floats between its channels (>= n_f when nch_f > 1, ignored for
 * one channel); pointers need 4-byte alignment only (a 16-byte aligned row
 * moves in 16-byte pieces, any other in 4-byte ones).  Entries of files
 * without rows are ignored.
 * lcfir_items_gather_dev copies [0, n_f) of every channel into the file's
 * input rows; values are moved, not computed on, so every bit pattern arrives
 * (NaN payloads, -0.0, subnormals), and the rows' zero padding is not touched.
 * lcfir_items_scatter_scaled_dev copies [0, n_f) of every output row to d_dst,
 * scaled on the way as lcfir_items_normalize_dev would scale it -- by
 * 1 / d_peak[f] iff (d_peak[f] > 1 or force) and d_peak[f] > 0, bit for bit
 * -- while the output rows stay unscaled; with d_peak NULL it is a plain copy
 * (force is ignored).  Nothing outside [0, n_f) of a destination row is
 * written.
 * LCFIR_EINVAL: a file with rows whose pointer is NULL or not 4-byte aligned,
 * whose stride is below n_f with nch_f > 1, or whose memory overlaps one of
 * the item set's arenas; a call on a capturing stream (the per-call table is
 * uploaded from the host, through page-locked slots allocated at the first of
 * these calls, as for the codec calls). */
int lcfir_items_gather_dev(lcfir_items *items, const float *const *d_src, const int64_t *src_stride, void *stream);
int lcfir_items_scatter_scaled_dev(lcfir_items *items, const float *d_peak, int force,
                                   float *const *d_dst, const int64_t *dst_stride, void *stream);

/* ---- device memory / stream helpers for hosts without a GPU runtime ----- */
int lcfir_dev_malloc(int device, size_t bytes, void **out);
int lcfir_dev_free(void *p);
int lcfir_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int lcfir_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream); /* synchronous */
/* Pinned (page-locked) host memory: H2D/D2H from it run asynchronously at PCIe rate, so a
 * multi-file driver can overlap file i+1's upload and file i-1's download with file i's
 * filtering.  lcfir_memcpy_d2h_async returns once the copy is queued;
 * the caller syncs the stream before touching dst. */
int lcfir_host_malloc(size_t bytes, void **out);
int lcfir_host_free(void *p);
int lcfir_memcpy_d2h_async(void *dst, const void *src, size_t bytes, void *stream);
int lcfir_stream_create(int device, void **stream);
int lcfir_stream_destroy(void *stream);
int lcfir_stream_sync(void *stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* LCFIR_H */
