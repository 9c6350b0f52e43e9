/*
 * sdsp_hip.h -- C ABI of the MI355X (gfx950) batched-FFT + cascaded-biquad engine.
 *
 * This is the drop-in boundary for simpledsp's FFT/IIR hot path.  The reference has no FFI
 * layer of its own: its boundary is the header-only C++ surface (include/sdsp/fft.h,
 * include/sdsp/casc_2o_iir.h).  The sdsp:: headers shipped in include/sdsp/ keep that surface
 * and call the entry points below; each entry point cites the reference interface it replaces
 * (paths relative to the reference checkout).  Plain pointers and sizes only -- no torch, no
 * C++ types.  `stream` arguments are hipStream_t passed as void* (NULL = the default stream).
 *
 * Conventions
 *   - every function returns an sdsp_hip_status (0 = ok, negative = error); a human-readable
 *     description of the calling thread's last error: sdsp_hip_last_error_string().
 *   - the caller owns all data buffers; transforms and filters run IN PLACE (fft.h:259,302;
 *     casc_2o_iir.h:37,71).  Plans own twiddles/coefficients/workspaces on their device.
 *   - complex data is interleaved (re,im), the layout of std::complex (fft.h:51-52).
 *   - there is no CPU fallback: without a usable HIP device the compute calls fail with
 *     SDSP_HIP_ERR_NO_DEVICE / SDSP_HIP_ERR_HIP.
 *   - distinct plans may be used from distinct host threads concurrently.
 */
#ifndef SDSP_HIP_H
#define SDSP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    SDSP_HIP_OK = 0,
    SDSP_HIP_ERR_INVALID_SIZE = -1, /* replaces static_assert fft.h:261,304 / casc_2o_iir.h:25 */
    SDSP_HIP_ERR_UNSUPPORTED = -2,
    SDSP_HIP_ERR_HIP = -3,
    SDSP_HIP_ERR_NO_DEVICE = -4,
    SDSP_HIP_ERR_INVALID_ARG = -5,
    SDSP_HIP_ERR_NOMEM = -6
} sdsp_hip_status;

typedef enum {
    SDSP_HIP_F32 = 0,
    SDSP_HIP_F64 = 1,
    /* IIR banks only: samples stored as float (8 bytes of HBM traffic per sample, like F32), per-channel state,
     * coefficients and the recurrence in double -- the reference computes in double (casc_2o_iir.h:11-18), and an f32
     * recurrence loses up to 1e-4 at low normalised cutoffs (f0/fs = 0.005); this mode is within float rounding of the
     * double result everywhere.  State buffers then hold doubles. */
    SDSP_HIP_F32_F64STATE = 2
} sdsp_hip_precision;
/* forward_fft / reverse_fft policy, fft.h:121-146 (reverse: conjugate twiddles and 1/N scale) */
typedef enum { SDSP_HIP_FORWARD = 1, SDSP_HIP_REVERSE = -1 } sdsp_hip_direction;
/* filter_type.h:6 -- the same integer values */
typedef enum {
    SDSP_HIP_FILTER_NONE = 0,
    SDSP_HIP_FILTER_LOW_PASS = 1,
    SDSP_HIP_FILTER_HIGH_PASS = 2,
    SDSP_HIP_FILTER_BAND_PASS = 3,
    SDSP_HIP_FILTER_BAND_STOP = 4 /* not in the reference (README.md:15 TODO); SURVEY 8(f)-4 */
} sdsp_hip_filter_type;
/* which process() body runs: casc_2o_iir::process (casc_2o_iir.h:36-80) or the
 * numerator-folded casc_2o_iir_{lp,hp,bp}::process_spec (:286-295, :344-353, :402-411) */
typedef enum {
    SDSP_HIP_IIR_GENERIC = 0,
    SDSP_HIP_IIR_LP = 1,
    SDSP_HIP_IIR_HP = 2,
    SDSP_HIP_IIR_BP = 3
} sdsp_hip_iir_kind;

#define SDSP_HIP_MAX_SECTIONS 16
#define SDSP_HIP_RADIX_AUTO 0
#define SDSP_HIP_STAGES_2_THEN_4 24 /* plan info: radix-2 stage(s) in front of radix-4 stages (mixed radix) */
#define SDSP_HIP_FIR_MAX_TAPS 4096
/* FFT-domain (overlap-save) FIR plans: f32 up to 16384 taps, f64 up to 8192 (fft_n <= 32768 / 16384 keeps the convolution one
 * fused kernel) */
#define SDSP_HIP_FIR_FFT_MAX_TAPS 16384
#define SDSP_HIP_FIR_FFT_MAX_TAPS_F64 8192
#define SDSP_HIP_FIR_DIRECT 0
#define SDSP_HIP_FIR_FFT 1

typedef struct sdsp_hip_fft_plan sdsp_hip_fft_plan;
typedef struct sdsp_hip_iir_plan sdsp_hip_iir_plan;

/* ------------------------------------------------------------------ runtime */

const char *sdsp_hip_last_error_string(void);
const char *sdsp_hip_version(void);
int sdsp_hip_device_count(int *count);
/* device memory helpers so that a C/C++ host can stay free of <hip/hip_runtime.h> */
int sdsp_hip_malloc(void **dev_ptr, size_t bytes, int device);
int sdsp_hip_free(void *dev_ptr, int device);
int sdsp_hip_memcpy_h2d(void *dev_dst, const void *host_src, size_t bytes, int device);
int sdsp_hip_memcpy_d2h(void *host_dst, const void *dev_src, size_t bytes, int device);
int sdsp_hip_device_synchronize(int device);

/* ------------------------------------------------------------------ size helpers, fft.h:12-43 */

unsigned sdsp_hip_log2(unsigned num);
unsigned sdsp_hip_log4(unsigned num);
int sdsp_hip_is_power_of_2(unsigned num);
int sdsp_hip_is_power_of_4(unsigned num);
/* digit_reverse<N,base>, fft.h:217-236 (the GPU folds this into load/store addressing) */
unsigned sdsp_hip_digit_reverse(unsigned n, unsigned base, unsigned x);
/* one row of the run-time twiddle precompute that replaces the compile-time calc_wCoeffs
 * (fft.h:197-214): out[j] = exp(-/+ 2*pi*i*j/n), j in [0,n), n interleaved complex doubles,
 * first quadrant from libm, the rest by exact mirror symmetry (fft.h:148-194). */
int sdsp_hip_calc_twiddles(unsigned n, int direction, double *out);

/* ------------------------------------------------------------------ FFT */

/*
 * Replaces sdsp::fft_radix2<T,N> (fft.h:258-299, radix = 2, n a power of 2) and
 * sdsp::fft_radix4<T,N> (fft.h:301-360, radix = 4, n a power of 4) for a BATCH of transforms.
 * radix: 2 or 4 checks the size the way the reference's function does (power of 2 / power of 4) and selects the
 * butterflies where a kernel of that stage type exists -- every n <= 16384, both precisions: a radix-4 plan runs radix-4
 * butterflies, a radix-2 plan radix-2 butterflies.  Above that the DEFAULT kernels of both radices are the multi-pass
 * kernels, whose register passes are radix-2 butterflies (the same DFT, held to the same tolerance against the radix-4
 * oracle); sdsp_hip_fft_plan_get_info reports the butterflies that actually run in `stage_radix`, and a variant >= 8 of a
 * radix-4 plan runs genuine radix-4 stages at any size (coverage kernel, fft_tile.hip).
 * radix = SDSP_HIP_RADIX_AUTO (0) asks for the fastest kernel of the size: any power of two through one entry (radix-4
 * stages where n is a power of 4 -- except n = 16384 --, radix-2 stages otherwise; `radix` in the plan info says which).
 * The mixed-radix case of SURVEY 8(f)-4, n = 8192 = 2 * 4^6 through the radix-4 machinery behind ONE radix-2 stage, is
 * variant 1 of AUTO plans of that size (kernel "sdsp_fft_mix_f32", stage_radix SDSP_HIP_STAGES_2_THEN_4); their default is
 * the registers-resident radix-2 kernel "sdsp_fft_big_kernel", which measured 1-2 points faster.
 * n must satisfy the radix (else SDSP_HIP_ERR_INVALID_SIZE -- the run-time form of the
 * reference's static_asserts).  `max_batch` sizes the plan-owned workspace that transforms too
 * large for on-chip memory need (n > 32768 in f32, n > 16384 in f64): allocated here when the plan's default kernel is
 * multi-pass (so sdsp_hip_fft_exec never allocates and can be stream-captured), on first use by an alternate variant
 * otherwise; larger batches are processed in slices of max_batch (the two-pass sizes never hold more than 256 MiB of intermediate:
 * their workspace stops growing there).  Twiddles are precomputed in double, rounded once to
 * the plan precision and kept resident in HBM.
 * One exec per plan in flight: the multi-pass kernels share the plan's workspace (and the persistent kernels their ticket
 * counters), so two sdsp_hip_fft_exec calls on the SAME plan must not overlap (different streams / host threads): use one
 * plan per stream.  Distinct plans are independent.
 */
int sdsp_hip_fft_plan_create(sdsp_hip_fft_plan **plan, uint32_t n, int radix, int direction,
                             int precision, uint64_t max_batch, int device);
int sdsp_hip_fft_plan_destroy(sdsp_hip_fft_plan *plan);

/* data: DEVICE pointer, batch x n interleaved complex of the plan precision, transformed in
 * place.  Asynchronous on `stream`.  Alignment: `data` must be aligned to ONE complex element of the plan precision (8 bytes
 * in f32, 16 in f64; real-input plans included: a pointer aligned to one real sample only is SDSP_HIP_ERR_INVALID_ARG) and
 * needs no more than that: every kernel takes such a pointer and gives the bits of an allocator-aligned one
 * (tests/test_gpu_isolation.py).  The same holds for `data` and `h` of sdsp_hip_fft_convolve. */
int sdsp_hip_fft_exec(sdsp_hip_fft_plan *plan, void *data, uint64_t batch, void *stream);
/* same with a HOST pointer: H2D, transform, D2H, synchronous (the single-call drop-in path) */
int sdsp_hip_fft_exec_host(sdsp_hip_fft_plan *plan, void *host_data, uint64_t batch);
/* contiguous batch split over `n_plans` devices (one plan per device, same n/radix/direction/
 * precision), one host thread + stream per device, no collective: SURVEY 8(e) */
int sdsp_hip_fft_exec_sharded(sdsp_hip_fft_plan *const *plans, int n_plans, void *host_data,
                              uint64_t batch);

/*
 * Fast convolution, SURVEY 8(f)-1: per transform, in place, data <- IFFT( FFT(data) .* h ), i.e. what a
 * reference user writes as fft_radix4(x); x[k] *= H[k]; fft_radix4<reverse_fft>(x); (the reverse_fft
 * policy with its 1/N scale exists for exactly this, fft.h:121-133).  `plan` must be a FORWARD plan;
 * h: DEVICE pointer to n complex values of the plan precision (frequency response, natural order).
 * f32 with n = 16 .. 16384 (radix-2 plans: .. 32768) and f64 with n = 16 .. 8192 (radix-2 plans: .. 16384) run as ONE kernel (one HBM read + one
 * write per element instead of three of each); larger n runs forward and reverse as two transforms with the multiply riding on the
 * forward transform's last pass (two-pass sizes) or as a third launch.
 */
int sdsp_hip_fft_convolve(sdsp_hip_fft_plan *plan, void *data, const void *h, uint64_t batch,
                          void *stream);

/*
 * Real-input packing, SURVEY 8(f)-3.  Every reference test feeds REAL signals through the complex
 * transform (testFFT.cpp:23-25,84-90); a plan made here moves half the bytes: n_real real samples
 * are transformed as n_real/2 complex points and split / merged on chip.
 *   direction FORWARD: data = batch x n_real floats in, batch x n_real/2 complex out, in place:
 *     out[k] = X[k] for 0 < k < n_real/2 (the spectrum of the real signal, same values the complex
 *     transform would give), out[0] = (X[0], X[n_real/2]) -- both are real; the upper half of the
 *     spectrum is the conjugate mirror.
 *   direction REVERSE: the inverse of that (packed half spectrum in, real samples out, 1/N scaled).
 * f32; radix 2: n_real = 32 .. 65536 a power of 2; radix 4: n_real/2 a power of 4, n_real <= 32768.  Use the plan
 * with sdsp_hip_fft_exec / _exec_host (batch counts transforms).
 */
int sdsp_hip_rfft_plan_create(sdsp_hip_fft_plan **plan, uint32_t n_real, int radix, int direction,
                              uint64_t max_batch, int device);
/* the same with a precision: SDSP_HIP_F64 packs n_real doubles <-> n_real/2 complex doubles (n_real = 32 .. 16384; radix 2: .. 32768); the
 * reference computes in double (fft.h:51-52). */
int sdsp_hip_rfft_plan_create_p(sdsp_hip_fft_plan **plan, uint32_t n_real, int radix, int direction, int precision,
                                uint64_t max_batch, int device);

/* Synchronises the plan's device and reports the health of its last sdsp_hip_fft_exec call.  The persistent kernels (n = 2^20
 * f32: "sdsp_fft1m_fused"; the other two-pass sizes where the plan info names "sdsp_fft2p_fused")
 * hand an intermediate from one workgroup to another inside a launch; every wait of that hand-off is bounded (2 s), and a
 * wait that gives up marks the call (a sticky word that every launch of the call can set and only the next call clears)
 * instead of hanging the GPU: this returns SDSP_HIP_ERR_HIP then, SDSP_HIP_OK otherwise (always OK for plans whose kernels
 * have no in-kernel hand-off).  The synchronous sdsp_hip_fft_exec_host checks the same word itself and returns the error;
 * ASYNCHRONOUS callers of such plans (sdsp_hip_fft_exec, sdsp_hip_fft_convolve -- whose reverse half is covered too) must call this
 * before trusting the output.  Has no reference
 * counterpart. */
int sdsp_hip_fft_plan_status(sdsp_hip_fft_plan *plan);
/* Testing hook for the error path above: the bound of the hand-off waits in 100 MHz ticks (default 200 000 000 = 2 s);
 * 0 = fault injection: every hand-off wait of the next launches gives up at once (their output is invalid by construction). */
int sdsp_hip_fft_plan_set_wait_limit(sdsp_hip_fft_plan *plan, uint64_t ticks);
/* Kernel launches that one sdsp_hip_fft_exec(plan, data, batch) issues with the plan's current variant (launch pieces and
 * workspace slices included; memsets not counted).  For profilers and bench.py: per-launch bytes = batch x
 * algorithmic_bytes / launches when hbm_passes == 1. */
int sdsp_hip_fft_plan_launches(const sdsp_hip_fft_plan *plan, uint64_t batch, uint64_t *launches);

/* Launch granularity (process-wide; has no reference counterpart).  A batch of transforms whose buffer is larger than
 * 1.5 x `bytes` is issued as consecutive launches over pieces of at most `bytes` of the buffer, in stream order (same bits,
 * same single call).  Why: workgroups are dealt to the eight XCDs round-robin and the XCDs drift apart over a long launch, so
 * the window of DRAM pages the chip works on widens.  Measured on the N = 4096 kernel: one launch over 8 GiB 72.1 % of HBM
 * peak, the same buffer in 2 GiB pieces 75.4 %, in 1 GiB pieces 76.3 %, 512 MiB 75.8 %, 256 MiB 74.4 % (DESIGN.md section
 * 5.1c).  Applies to the FFT kernels that cover a batch with one launch, N <= 8192 (many short workgroups); not to
 * N = 16384 / 32768 (one or two transforms fill a CU: pieces cost 1.6 points there), not to the multi-pass sizes (they chunk
 * by their workspace) and not to the IIR / FIR kernels (a workgroup there walks whole rows for milliseconds: pieces only add launch
 * tails -- 70.0 % in one launch, 68.7 / 66.4 / 45.2 % in 2 GiB / 1 GiB / 512 MiB pieces).  bytes = 0: never split. */
#define SDSP_HIP_DEFAULT_PIECE_BYTES (1ull << 30)
int sdsp_hip_set_launch_piece_bytes(uint64_t bytes);
int sdsp_hip_get_launch_piece_bytes(uint64_t *bytes);

typedef struct {
    uint32_t n;
    int radix;
    int direction;
    int precision;
    int device;
    int hbm_passes;              /* passes over HBM of the kernel(s) that run: 1 = one read + one write per element */
    uint64_t algorithmic_bytes;  /* per transform: n * sizeof(complex) * 2 (read + write once) */
    uint64_t workspace_bytes;
    uint64_t twiddle_bytes;
    char kernel[64];             /* name of the dominant kernel (for rocprofv3 matching) */
    int stage_radix;             /* the butterflies that kernel executes: 2, 4, or SDSP_HIP_STAGES_2_THEN_4 */
} sdsp_hip_fft_plan_info;
int sdsp_hip_fft_plan_get_info(const sdsp_hip_fft_plan *plan, sdsp_hip_fft_plan_info *info);
/* copy the plan's resident twiddle row W_n^j (plan precision, n complex) back to the host */
int sdsp_hip_fft_plan_get_twiddles(const sdsp_hip_fft_plan *plan, void *host_out);
/* choose among kernel variants of a plan (tuning/testing).  Variant 0 is the default; a plan has at most two documented
 * alternates (same transform, same tolerance; DESIGN.md section 5 lists them per size: e.g. n = 4096 radix 4: 1, 2 = other
 * store / barrier schedules of the same kernel; n = 8192 AUTO plans and n = 16384 radix-4 plans: 1 = the fft_mix.hip kernel
 * (mixed radix / leading radix-4 stage); the two-pass sizes (f32 n = 2^16 .. 2^19, 2^21, 2^22; f64 n = 2^15 .. 2^20): 1 = three
 * streaming passes, 3 = the other SCHEDULE of the same two passes -- one persistent, ticketed launch ("sdsp_fft2p_fused") against two
 * launches per chunk ("sdsp_fft2p_cols+sdsp_fft2p_rows"), bit-identical results; the default is the persistent launch (level or faster at
 * every size, 1 - 5 points of HBM peak), and plans whose workspace (max_batch) is smaller than the
 * persistent launch's 256 MiB ring of intermediates run the two launches under either number; n = 2^20 f32: 1 = two launches per chunk, 2 = the persistent launch through
 * fft_2pass.hip's generic kernel instead of the dedicated one (42.3 against 42.7 % of HBM peak); n = 16 .. 2048 f32 (the register-pass family, fft_reg.hip): 1 = the
 * same kernel with the default cache policy, 2 = the one-wave kernel (fft_wave.hip) at n = 256 / 1024 / 2048; real-input plans of
 * n_real = 1024, whose default IS the one-wave kernel: 1, 2 = the register-pass family with the default / streaming cache
 * policy (n_real = 512 / 2048: as the complex plans); the same as variant 2 of sdsp_hip_fft_convolve for the fused convolution of n = 256 .. 2048 (default: the one-wave kernel); f64 n = 1024: 1 = the one-wave kernel); any larger number selects the untuned coverage kernel
 * (fft_tile.hip), which the tests use as an independent implementation. */
int sdsp_hip_fft_plan_set_variant(sdsp_hip_fft_plan *plan, int variant);

/*
 * Column plans: batched transforms along the STRIDED axis.  Where sdsp_hip_fft_exec transforms the contiguous
 * rows of batch x n, a column plan transforms every column of `batch` compact row-major cubes of n rows x width columns -- the Doppler
 * step of a pulse-Doppler chain ([cube][pulse][range bin], one transform per range bin across the pulses) and the second axis of a 2-D
 * transform -- in one read and one write of the cube, with no transpose and no workspace.
 *   - layout.  in: batch cubes of n rows x width interleaved complex elements of the plan precision (F32 or F64); element [b][p][r] is
 *     at (b n + p) width + r, and column r of cube b is the sequence x[p] = in[b][p][r], p = 0 .. n - 1.  out has the same [b][k][r]
 *     layout and holds complex elements (COMPLEX) or real elements (POWER).  Cubes are compact: there is no row pitch.
 *   - transform.  X[k] = sum_p v[p] W_n^(p k) with the conventions of fft.h:121-146: FORWARD W = e^(-2 pi i / n); REVERSE the
 *     conjugate and a 1/n scale.  The twiddles are sdsp_hip_calc_twiddles's, rounded once to the precision.  n is a power of two,
 *     SDSP_HIP_FFT_COLS_MIN_N <= n <= SDSP_HIP_FFT_COLS_MAX_N; width >= 1 is any number; batch n width < 2^40.
 *   - window.  NULL or n host doubles, each rounded once to the precision at plan creation; v[p] = x[p] w[p], one product per component
 *     (the kernel may fuse it into the first butterfly).  Without a window v = x.  Only FORWARD plans take a window.
 *   - shift != 0 puts zero Doppler in the middle: a FORWARD plan writes X[k] to row (k + n/2) mod n, a REVERSE plan reads x[p] from row
 *     (p + n/2) mod n, so that reverse undoes forward (n is even).
 *   - POWER writes re re + im im of X[k] as a real row: the layout sdsp_hip_cfar_process takes as batch n channel-major rows of width
 *     powers.  Only FORWARD plans allow it.
 *   - in place and overlap.  COMPLEX: out == in (the same pointer) or disjoint ranges.  POWER: disjoint ranges.  Any other overlap is
 *     SDSP_HIP_ERR_INVALID_ARG.  in is never written out of place.
 *   - pointers need the alignment of one element of their own type (in: one complex element; out: one complex element, POWER one
 *     real) and no more.  exec is asynchronous on `stream`, allocates nothing and can be captured in a graph; batch == 0 does nothing.
 *   - accuracy.  Nothing at bit level is promised against the row plans; the results meet their tolerances: f64 within 4 n eps of the
 *     double transform relative to max |X| of the column, f32 within 1e-6 normwise.
 *   - independence.  The bits of a column's n outputs depend on that column's n inputs, the window and the plan (n, direction,
 *     precision, output, shift, variant) only: not on width, the column's position r, the cube index, batch, the neighbouring columns
 *     (a NaN stays in its column), in place or out of place, or the alignment of the pointers beyond one element.
 * Errors: n not a power of two or out of range, width == 0, the size limit exceeded: SDSP_HIP_ERR_INVALID_SIZE; a null pointer, an
 * unknown direction, output or precision, a window or POWER on a REVERSE plan, a window value that is not finite once rounded, a
 * misaligned pointer, a refused overlap: SDSP_HIP_ERR_INVALID_ARG; no device: SDSP_HIP_ERR_NO_DEVICE.  Arguments are checked before a
 * device is looked for.
 */
typedef struct sdsp_hip_fft_cols_plan sdsp_hip_fft_cols_plan;
#define SDSP_HIP_FFT_COLS_COMPLEX 0
#define SDSP_HIP_FFT_COLS_POWER 1
#define SDSP_HIP_FFT_COLS_MIN_N 8
#define SDSP_HIP_FFT_COLS_MAX_N 1024
int sdsp_hip_fft_cols_plan_create(sdsp_hip_fft_cols_plan **plan, uint32_t n, uint64_t width, int direction, int precision,
                                  int output, int shift, const double *window, int device);
int sdsp_hip_fft_cols_plan_destroy(sdsp_hip_fft_cols_plan *plan);
/* in, out: DEVICE pointers to batch cubes */
int sdsp_hip_fft_cols_exec(sdsp_hip_fft_cols_plan *plan, const void *in, void *out, uint64_t batch, void *stream);
/* same with HOST pointers (synchronous); host_out == host_in transforms in place */
int sdsp_hip_fft_cols_exec_host(sdsp_hip_fft_cols_plan *plan, const void *host_in, void *host_out, uint64_t batch);
/* kernel variants (same tolerances, no common bits promised): 0 = sdsp_fft_cols_kernel, whose form depends on n and the precision only
 * -- n <= 32: one lane per column, the column in registers, no LDS; n >= 64: tiles of 16 adjacent columns, n / 32 threads per column,
 * two register passes around one exchange through LDS --; 1 = sdsp_fft_cols_plain_kernel, one thread per output summing the DFT from
 * global memory in double (the cross-check; it shares no staging or butterfly code with variant 0). */
int sdsp_hip_fft_cols_plan_set_variant(sdsp_hip_fft_cols_plan *plan, int variant);
/* kernel launches of one exec of `batch` cubes: one where the grid fits, else consecutive launches over whole cubes; 0 for batch == 0 */
int sdsp_hip_fft_cols_plan_launches(const sdsp_hip_fft_cols_plan *plan, uint64_t batch, uint64_t *launches);
typedef struct {
    uint32_t n;
    uint64_t width;
    int direction, precision, output, shift, windowed, device, variant;
    uint32_t tile_columns;      /* adjacent columns that one tile of the variant's kernel transforms together */
    uint32_t threads;           /* of one workgroup */
    uint32_t lds_bytes;         /* of one workgroup */
    uint64_t algorithmic_bytes; /* per cube: n width (complex element + output element), read once plus write once */
    char kernel[64];            /* the kernel the plan's variant runs */
} sdsp_hip_fft_cols_plan_info;
int sdsp_hip_fft_cols_plan_get_info(const sdsp_hip_fft_cols_plan *plan, sdsp_hip_fft_cols_plan_info *info);

/* ------------------------------------------------------------------ cascaded biquads */

/*
 * Coefficient design (host, double) -- set_lp_coeff / set_hp_coeff / set_bp_coeff,
 * casc_2o_iir.h:168-194, :140-166, :82-138 (identical in the specialised classes :297-467).
 * sections = m_t (even).  Outputs: a[sections*3], b[sections*3], *gain (= m_gain).
 */
int sdsp_hip_iir_design_lp(uint32_t sections, double f0, double fs, double gain_in, double *a,
                           double *b, double *gain);
int sdsp_hip_iir_design_hp(uint32_t sections, double f0, double fs, double gain_in, double *a,
                           double *b, double *gain);
int sdsp_hip_iir_design_bp(uint32_t sections, double f0, double fs, double q, double gain_in,
                           double *a, double *b, double *gain);
/*
 * Band-stop design -- the reference's README.md:15 TODO, SURVEY 8(f)-4 (no reference code: parity is
 * pinned to scipy.signal.butter(btype='bandstop') instead).  Same parameters as design_bp: centre f0,
 * -3 dB width f0/q, Butterworth prototype of order `sections`.  Every section's numerator is
 * [1, -2cos(2 pi f0/fs), 1]; run it on a GENERIC plan.
 */
int sdsp_hip_iir_design_bs(uint32_t sections, double f0, double fs, double q, double gain_in,
                           double *a, double *b, double *gain);
/* preload_filter, casc_2o_iir.h:197-214: mem[(sections+1)*3] for a steady input `value` */
int sdsp_hip_iir_preload(uint32_t sections, int filter_type, const double *a, const double *b,
                         double gain, double value, double *mem);

/*
 * A bank of identical cascades (shared coefficients, per-channel state) -- the batched form of
 * sdsp::casc_2o_iir<m_t> (kind GENERIC) and sdsp::casc_2o_iir_{lp,hp,bp}<m_t>.
 * a: sections*3, b: sections*3 (may be NULL for the specialised kinds), gain: m_gain.
 */
int sdsp_hip_iir_plan_create(sdsp_hip_iir_plan **plan, uint32_t sections, int kind,
                             const double *a, const double *b, double gain, int precision,
                             int device);
int sdsp_hip_iir_plan_destroy(sdsp_hip_iir_plan *plan);

/*
 * process(): casc_2o_iir.h:36-80 / :228-263 for `channels` independent streams.
 * data: DEVICE pointer; channel c's samples are data[c*stride + 0 .. samples) (channel-major,
 * each channel is what one reference process() call sees), filtered in place.
 * state: DEVICE pointer or NULL.  NULL = every channel starts from a zero-initialised filter
 *   and the final state is dropped.  Otherwise state[(3*(sections+1)) * channels] of the plan
 *   precision, laid out state[(3*j + age) * channels + c] = y_j[n-1-age] of channel c
 *   (j = 0 is the gain-scaled input history, j = sections the output history, age 0..2):
 *   the reference's m_mem ring (casc_2o_iir.h:15) rotated so that m_pos is implicit.  Read at
 *   entry, written at exit, so consecutive calls continue the stream bit-identically
 *   (testIIR.cpp:61-75).
 */
int sdsp_hip_iir_process(sdsp_hip_iir_plan *plan, void *data, uint64_t channels,
                         uint64_t samples, uint64_t stride, void *state, void *stream);
/*
 * The same filter bank on the interleaved ("wire") layout: sample s of channel c is
 * data[s*stride + c] (stride >= channels elements between consecutive sample rows), i.e. what an
 * ADC / network frame delivers.  No transpose is needed, so this is the fastest entry; results are
 * bit-identical to sdsp_hip_iir_process on the transposed data.  Fast path: rows 8-byte aligned and
 * an even channel count for f32 (any 4-byte aligned f32 shape still works).  SURVEY 8(f)-2.
 */
int sdsp_hip_iir_process_interleaved(sdsp_hip_iir_plan *plan, void *data, uint64_t channels,
                                     uint64_t samples, uint64_t stride, void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_iir_process_host(sdsp_hip_iir_plan *plan, void *host_data, uint64_t channels,
                              uint64_t samples, uint64_t stride, void *host_state);
/* contiguous channel range split over devices, no collective */
int sdsp_hip_iir_process_sharded(sdsp_hip_iir_plan *const *plans, int n_plans, void *host_data,
                                 uint64_t channels, uint64_t samples);
/* bytes of a state buffer for `channels` channels */
int sdsp_hip_iir_state_bytes(const sdsp_hip_iir_plan *plan, uint64_t channels, uint64_t *bytes);
/* kernel variants of sdsp_hip_iir_process (tuning / testing; identical arithmetic, bit-identical results): 0 = default -- the
 * landing-slot kernel (LDS-DMA fill one tile ahead of the recurrence) for f32 banks of up to 4 sections on whole [64
 * channels x 512 bytes] tiles, the super-tile kernel for everything else; 1 = wide super-tile; 2 = direct (any alignment);
 * 3 = super-tile.  DESIGN.md section 5.4. */
int sdsp_hip_iir_plan_set_variant(sdsp_hip_iir_plan *plan, int variant);
/* name of the kernel sdsp_hip_iir_process would launch for this buffer shape with the plan's variant (for matching
 * rocprofv3 rows); the same selection function as the launcher's.  Has no reference counterpart. */
int sdsp_hip_iir_plan_kernel(const sdsp_hip_iir_plan *plan, const void *data, uint64_t channels, uint64_t samples,
                             uint64_t stride, char *name, size_t name_bytes);

/* ------------------------------------------------------------------ FIR filter bank */

/*
 * The reference lists "FIR filter" as a TODO (README.md:16) and has no code for it -- SURVEY 8(f)-4.
 * These entries follow the conventions of the IIR bank above (what sdsp::casc_2o_iir does for one
 * stream, casc_2o_iir.h:36-80: in place, stateful across calls); parity is pinned to
 * scipy.signal.firwin / lfilter, not to the reference.
 *
 * Design: Hamming-windowed sinc, `taps` coefficients h[0..taps), unit gain (times gain_in) in the
 * pass band.  filter_type: LOW_PASS / HIGH_PASS (cutoff f0; q ignored), BAND_PASS / BAND_STOP (centre
 * f0, edges f0 -+ f0/(2q)).  Filters that pass fs/2 (HIGH_PASS, BAND_STOP) need an odd tap count.
 */
int sdsp_hip_fir_design(uint32_t taps, int filter_type, double f0, double fs, double q,
                        double gain_in, double *h);

typedef struct sdsp_hip_fir_plan sdsp_hip_fir_plan;
/* h: taps doubles (host), rounded to the plan precision and kept resident on the device */
int sdsp_hip_fir_plan_create(sdsp_hip_fir_plan **plan, uint32_t taps, const double *h,
                             int precision, int device);
int sdsp_hip_fir_plan_destroy(sdsp_hip_fir_plan *plan);
/*
 * y[n] = sum_{k<taps} h[k] x[n-k] for `channels` independent streams, in place.  data: DEVICE pointer,
 * channel-major like sdsp_hip_iir_process (channel c = data[c*stride .. +samples)).
 * state: DEVICE pointer or NULL (zero history, final history dropped); otherwise
 * state[c*(taps-1) + j] = x_c[n-1-j] (j = 0 is the newest input), plan precision, read at entry and
 * written at exit so block-by-block calls equal one long call bit for bit.  Accumulation order:
 * ascending k, one multiply and one add per tap in f64 (bit-identical to the CPU oracle), FMA in f32.
 */
int sdsp_hip_fir_process(sdsp_hip_fir_plan *plan, void *data, uint64_t channels, uint64_t samples,
                         uint64_t stride, void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_fir_process_host(sdsp_hip_fir_plan *plan, void *host_data, uint64_t channels,
                              uint64_t samples, uint64_t stride, void *host_state);
int sdsp_hip_fir_state_bytes(const sdsp_hip_fir_plan *plan, uint64_t channels, uint64_t *bytes);
/* direct plans: kernel variants of sdsp_fir_kernel (same values); FFT plans: the variant of the inner convolution
 * (sdsp_hip_fft_convolve's numbering on a forward radix-2 plan of size fft_n: 0 = the fused kernel, 1 = the three-launch
 * composition -- an independent cross-check, within the same tolerance).  Whatever the variant needs is allocated here. */
int sdsp_hip_fir_plan_set_variant(sdsp_hip_fir_plan *plan, int variant);

/*
 * FFT-domain FIR plans (overlap-save) for long filters: the same filter as a direct plan of the same h,
 * computed per frame of N = fft_n inputs as IFFT(FFT(frame) .* H) with H = FFT(h zero-padded to N), computed in double at
 * creation and rounded once to the plan precision.  Hop L = N - taps + 1 outputs per frame; N >= 2 (taps - 1).  Two frames
 * of one channel share one complex transform (real / imaginary part): a NaN or Inf input reaches every output of the frame
 * pairs (frames 2p and 2p + 1) whose frames read it, not only the `taps` outputs that depend on it, and no other channel.
 * Rounding differs from the direct form (the error is
 * normwise per frame pair, ~1e-7 in f32, ~1e-15 in f64), so block-by-block calls match one long call within that
 * tolerance, not bit for bit.
 * sdsp_hip_fir_process / _process_host / _state_bytes / _plan_set_variant / _plan_destroy take these plans with the same
 * arguments, stride and state layout as direct plans: a stream may move between a direct and an FFT plan of the same h from one
 * block to the next.  A process call runs in slices of the plan's workspace (frame gather -> convolution -> scatter in place,
 * then the new history); it allocates nothing and can be stream-captured.  One process call per plan in flight: the slices
 * share the plan's workspace, so two calls on the SAME plan must not overlap (use one plan per stream).
 */
/* auto FFT size for `taps` (power of two, N >= 2(taps-1), within the fused-convolution range of the precision) */
int sdsp_hip_fir_fft_size(uint32_t taps, int precision, uint32_t *fft_n);
/* fft_n = 0: auto; workspace_bytes = 0: default budget (rounded down to whole transforms, at least one).
 * Errors: taps == 0 or above the precision's maximum, fft_n not a power of two or below 2 (taps - 1):
 * SDSP_HIP_ERR_INVALID_SIZE; fft_n outside the fused convolution (f32 16 .. 32768, f64 16 .. 16384): SDSP_HIP_ERR_UNSUPPORTED;
 * a bad precision or a null pointer: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_fir_fft_plan_create(sdsp_hip_fir_plan **plan, uint32_t taps, const double *h, int precision,
                                 uint32_t fft_n, uint64_t workspace_bytes, int device);
typedef struct {
    uint32_t taps;
    int precision;
    int device;
    int method;               /* SDSP_HIP_FIR_DIRECT / SDSP_HIP_FIR_FFT */
    uint32_t fft_n, hop;      /* 0 for direct plans */
    uint64_t workspace_bytes; /* FFT plans: frame pairs + staged history + carry */
    char kernel[64];          /* dominant kernel: "sdsp_fir_kernel" or the convolution's */
} sdsp_hip_fir_plan_info;
int sdsp_hip_fir_plan_get_info(const sdsp_hip_fir_plan *plan, sdsp_hip_fir_plan_info *info);
/* kernel launches one sdsp_hip_fir_process(plan, ., channels, samples, ...) with a state buffer issues (memsets not counted) */
int sdsp_hip_fir_plan_launches(const sdsp_hip_fir_plan *plan, uint64_t channels, uint64_t samples, uint64_t *launches);

/* ------------------------------------------------------------------ polyphase FIR resampler banks */

/*
 * Rate change by U / D (up factor U, down factor D, g = gcd(U, D), q = D / g) with a T-tap filter h, for `channels` independent
 * streams, out of place.  Output m of a call, x = the history followed by the block:
 *     y[m] = sum over k < T with (m D - k) = 0 (mod U) of h[k] x[(m D - k) / U],   m in [0, S U / D)
 * -- the causal part of scipy.signal.upfirdn(h, x, U, D); outputs of a phase without taps (T < U) are 0.  No reference counterpart:
 * pinned to scipy, like the FIR bank.
 *   - samples S must be a multiple of q; every call yields exactly S U / D outputs and starts at phase 0, so block-by-block calls
 *     equal one long call bit for bit.
 *   - history: H = floor((T - 1) / U) inputs per channel, state[c H + j] = x_c[n-1-j] (j = 0 the newest), plan precision; read at
 *     entry, written at exit; NULL = zero history, final history dropped.  With U = 1 this is the direct FIR plan's layout.
 *   - each output sums exactly its own taps in ascending k: a plain multiply, then one multiply and one add per tap in f64, one
 *     fmaf in f32 -- the values of zero-stuff -> sdsp_hip_fir_process of the same precision -> every D-th sample (signed zeros
 *     aside).  No phase is padded with zero taps.
 * Limits: 1 <= T <= SDSP_HIP_FIR_MAX_TAPS, 1 <= U, D <= SDSP_HIP_RESAMPLE_MAX_FACTOR.
 */
#define SDSP_HIP_RESAMPLE_MAX_FACTOR 1024
typedef struct sdsp_hip_resample_plan sdsp_hip_resample_plan;
/* anti-aliasing / anti-imaging low-pass for the ratio: Hamming-windowed sinc, cutoff 1 / (2 max(U, D)) of the intermediate rate
 * (U times the input rate), pass-band gain U (what interpolation by U loses) -- sdsp_hip_fir_design(taps, LOW_PASS, 1 / max(U, D),
 * 2, 0, U) == U * scipy.signal.firwin(taps, 1 / max(U, D)).  U = D = 1 (no rate change): SDSP_HIP_ERR_INVALID_ARG; taps or a factor
 * out of range: SDSP_HIP_ERR_INVALID_SIZE. */
int sdsp_hip_resample_design(uint32_t taps, uint32_t up, uint32_t down, double *h);
/* outputs one call of `samples` inputs per channel yields (S U / D); host only, no device needed.  samples not a multiple of q, or a
 * factor out of range: SDSP_HIP_ERR_INVALID_SIZE; out NULL: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_resample_out_samples(uint32_t up, uint32_t down, uint64_t samples, uint64_t *out);
/* h: taps doubles (host), rounded to the plan precision and kept on the device.  Errors: taps, up or down out of range:
 * SDSP_HIP_ERR_INVALID_SIZE; a null pointer or a precision other than F32 / F64: SDSP_HIP_ERR_INVALID_ARG; no device:
 * SDSP_HIP_ERR_NO_DEVICE. */
int sdsp_hip_resample_plan_create(sdsp_hip_resample_plan **plan, uint32_t taps, const double *h, uint32_t up, uint32_t down,
                                  int precision, int device);
int sdsp_hip_resample_plan_destroy(sdsp_hip_resample_plan *plan);
/*
 * in: DEVICE pointer, channel c = in[c in_stride .. + samples), never written.  out: DEVICE pointer, channel c = out[c out_stride
 * .. + S U / D); nothing past those rows is touched.  state: DEVICE pointer or NULL (layout above).  Asynchronous on `stream`,
 * allocates nothing (stream-capturable); one call per plan in flight.
 * Errors: samples % q != 0: SDSP_HIP_ERR_INVALID_SIZE; null in / out, in_stride < samples or out_stride < S U / D with more
 * than one channel, overlapping in and out ranges: SDSP_HIP_ERR_INVALID_ARG.  channels == 0 or samples == 0: nothing to do.
 * Measured (1 MI355X, 1M channels x 4032 samples f32, 64 taps, D = 4): DESIGN.md section 5.10.
 */
int sdsp_hip_resample_process(sdsp_hip_resample_plan *plan, const void *in, uint64_t in_stride, void *out, uint64_t out_stride,
                              uint64_t channels, uint64_t samples, void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_resample_process_host(sdsp_hip_resample_plan *plan, const void *host_in, uint64_t in_stride, void *host_out,
                                   uint64_t out_stride, uint64_t channels, uint64_t samples, void *host_state);
/* bytes of a state buffer for `channels` channels: H channels element size (0 when H = 0) */
int sdsp_hip_resample_state_bytes(const sdsp_hip_resample_plan *plan, uint64_t channels, uint64_t *bytes);
/* kernel variants (identical values, bit for bit): 0 = default (sdsp_resample_dec_kernel for U = 1 and D in {1, 2, 4, 8, 16},
 * sdsp_resample_poly_kernel otherwise); 1 = sdsp_resample_plain_kernel, one output per thread from global memory (the
 * cross-check); 2 = sdsp_resample_poly_kernel for every ratio. */
int sdsp_hip_resample_plan_set_variant(sdsp_hip_resample_plan *plan, int variant);
typedef struct {
    uint32_t taps, up, down;
    uint32_t hist;   /* H = floor((taps - 1) / up) */
    int precision;
    int device;
    char kernel[64]; /* the kernel the plan's variant runs on a long contiguous row */
} sdsp_hip_resample_plan_info;
int sdsp_hip_resample_plan_get_info(const sdsp_hip_resample_plan *plan, sdsp_hip_resample_plan_info *info);

/* ------------------------------------------------------------------ STFT banks */

/*
 * Short-time Fourier transform of `channels` independent real streams.  N = n_fft (a power of two in the
 * radix-2 real-input range: f32 32 .. 65536, f64 32 .. 32768), 1 <= hop <= N, hist = N - hop, bins = N / 2 + 1.  A call takes
 * S samples per channel, S a multiple of hop, and writes exactly F = S / hop frames.  With x = the channel's history followed by
 * the block (the block starts at index hist), frame j of the call is
 *     out[c out_stride + j bins + k] = sum over n < N of fl(x[j hop + n] w[n]) e^(-2 pi i k n / N),   0 <= k <= N / 2
 * -- the np.fft.rfft sign, no scaling; torch.stft(concat(history, block), N, hop, window = w, center = False) in frame-major order.
 * A fresh stream (NULL or zeroed state) is the stream with hist zeros in front of it.
 *   - history: state[c hist + j] = x_c[-1 - j] (newest first), plan precision; read at entry, written at exit; NULL = zero history,
 *     final history dropped (the FIR and resampler layout).  hop = N: hist = 0, no state.
 *   - block-by-block calls equal one long call bit for bit, for any split into multiples of hop (blocks shorter than hist included).
 *   - the window: N host doubles, rounded once to the plan precision at creation; every windowed sample is one rounding of x w.
 *   - output kinds: COMPLEX = interleaved complex of the plan precision; POWER = re re + im im in the plan precision (two products
 *     and a sum, no FMA contraction); MAGNITUDE = sqrt of the power.  Bins 0 and N / 2 have zero imaginary parts.
 *   - strides count elements (a complex bin is one element).  `in` is never written; nothing past each channel's F bins outputs is.
 * A call runs in slices of the plan's workspace: windowed frames -> the library's forward real-input transform (unchanged) -> the
 * output rows, then one launch for the new history.
 */
#define SDSP_HIP_STFT_COMPLEX 0
#define SDSP_HIP_STFT_POWER 1
#define SDSP_HIP_STFT_MAGNITUDE 2
#define SDSP_HIP_WINDOW_RECT 0
#define SDSP_HIP_WINDOW_HANN 1
#define SDSP_HIP_WINDOW_HAMMING 2
#define SDSP_HIP_WINDOW_BLACKMAN 3
typedef struct sdsp_hip_stft_plan sdsp_hip_stft_plan;
/* periodic window of n points (scipy.signal.get_window(name, n), fftbins = True), host only: RECT 1; HANN 0.5 - 0.5 cos(2 pi k / n);
 * HAMMING 0.54 - 0.46 cos(2 pi k / n); BLACKMAN 0.42 - 0.5 cos(2 pi k / n) + 0.08 cos(4 pi k / n).  Unknown kind or w NULL:
 * SDSP_HIP_ERR_INVALID_ARG; n = 0: SDSP_HIP_ERR_INVALID_SIZE. */
int sdsp_hip_stft_window(int kind, uint32_t n, double *w);
/* frames one call of `samples` per channel writes (samples / hop); host only.  hop = 0 or samples % hop != 0:
 * SDSP_HIP_ERR_INVALID_SIZE; frames NULL: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_stft_frames(uint32_t hop, uint64_t samples, uint64_t *frames);
/* window: n_fft host doubles.  workspace_bytes: the slice budget (0 = the default); a slice holds at least
 * one frame.  Errors: n_fft not a power of two, hop = 0 or hop > n_fft: SDSP_HIP_ERR_INVALID_SIZE; n_fft outside the real-input
 * range of the precision: SDSP_HIP_ERR_UNSUPPORTED; a null pointer, a precision other than F32 / F64 or an unknown output kind:
 * SDSP_HIP_ERR_INVALID_ARG; no device: SDSP_HIP_ERR_NO_DEVICE. */
int sdsp_hip_stft_plan_create(sdsp_hip_stft_plan **plan, uint32_t n_fft, uint32_t hop, const double *window, int output,
                              int precision, uint64_t workspace_bytes, int device);
int sdsp_hip_stft_plan_destroy(sdsp_hip_stft_plan *plan);
/*
 * in: DEVICE pointer, channel c = in[c in_stride .. + samples).  out: DEVICE pointer, channel c = out[c out_stride .. + F bins)
 * elements.  state: DEVICE pointer or NULL.  Asynchronous on `stream`, allocates nothing (stream-capturable); one call per plan
 * in flight.  Errors: samples % hop != 0: SDSP_HIP_ERR_INVALID_SIZE; null in / out, in_stride < samples or out_stride < F bins
 * with more than one channel, overlapping in and out ranges: SDSP_HIP_ERR_INVALID_ARG.  channels == 0 or samples == 0: nothing
 * to do.  Measured (1 MI355X, 1024 channels x 2^18 samples f32, N = 1024, hop = 256): power 4.25 ms against 8.60 ms for
 * unfold x window -> rfft -> unpack -> |X|^2 (2.02x) and 10.6 ms for torch.stft (2.50x); complex 4.64 ms (1.16x / 1.62x).
 * DESIGN.md section 5.11.
 */
int sdsp_hip_stft_process(sdsp_hip_stft_plan *plan, const void *in, uint64_t in_stride, void *out, uint64_t out_stride,
                          uint64_t channels, uint64_t samples, void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_stft_process_host(sdsp_hip_stft_plan *plan, const void *host_in, uint64_t in_stride, void *host_out, uint64_t out_stride,
                               uint64_t channels, uint64_t samples, void *host_state);
/* bytes of a state buffer for `channels` channels: hist channels element size (0 when hop = n_fft) */
int sdsp_hip_stft_state_bytes(const sdsp_hip_stft_plan *plan, uint64_t channels, uint64_t *bytes);
/* the kernel variant of the inner real-input plan (sdsp_hip_fft_plan_set_variant of an rfft plan of n_real = n_fft, radix 2);
 * SDSP_HIP_ERR_UNSUPPORTED where that plan has no such variant */
int sdsp_hip_stft_plan_set_variant(sdsp_hip_stft_plan *plan, int variant);
/* kernel launches of one process call of `samples` per channel with a state buffer (frame, transform and emit launches per slice,
 * plus the state launch when hist > 0) */
int sdsp_hip_stft_plan_launches(const sdsp_hip_stft_plan *plan, uint64_t channels, uint64_t samples, uint64_t *launches);
typedef struct {
    uint32_t n_fft, hop, bins, hist;
    int output, precision, device;
    uint64_t workspace_bytes;
    char kernel[64]; /* the inner transform's kernel */
} sdsp_hip_stft_plan_info;
int sdsp_hip_stft_plan_get_info(const sdsp_hip_stft_plan *plan, sdsp_hip_stft_plan_info *info);

/* ------------------------------------------------------------------ inverse STFT banks */

/*
 * Overlap-add synthesis of `channels` independent real streams from frames of N / 2 + 1 complex bins (the STFT bank's COMPLEX
 * layout).  N = n_fft (a power of two in the radix-2 real-input range: f32 32 .. 65536, f64 32 .. 32768),
 * 1 <= hop <= N, hist = N - hop, bins = N / 2 + 1.  A call takes F frames per channel and writes F hop samples per channel.
 *   - synthesis window g (computed in double on the host, rounded once to the plan precision): NORMALIZED g[n] = w[n] / env[n mod hop]
 *     with env[r] = sum over k of w[r + k hop]^2 (the window-square normalisation of torch.istft / scipy.signal.istft); RAW g = w.
 *     A NORMALIZED plan whose min env <= 1e-10 max env breaks the NOLA condition and is refused (SDSP_HIP_ERR_INVALID_ARG).
 *   - z_j = the library's reverse real-input transform of frame j (1 / N scaled; the imaginary parts of bins 0 and N / 2 are
 *     ignored, as in irfft).  P = the pending sums, hist values per channel in time order: state[c hist + i] belongs to output
 *     sample i of this call.  a[t] = P[t] (t < hist), then fl(g[t - j hop] z_j[t - j hop]) added one at a time in ascending j --
 *     the only additions, no FMA contraction.  out[c out_stride + t] = a[t] for t < F hop; the new state is a[F hop + i].
 *     NULL state = zero pending sums, the new tail dropped.  hop = N: hist = 0, no state.
 *   - block-by-block calls equal one long call bit for bit, for any split into frame counts (F hop < hist and empty blocks
 *     included).  istft(stft(x)) with NORMALIZED, both fresh, is x delayed by hist samples; on [hist, F hop) a fresh call equals
 *     torch.istft(X, N, hop, window = w, center = False).
 *   - strides count elements: complex bins for `in`, reals for `out`.  `in` is never written; nothing past each channel's F hop
 *     outputs is.
 * A call runs in slices of the plan's workspace: one launch that consumes the old pending sums, then per slice pack -> the library's
 * reverse real-input transform (unchanged) -> overlap-add (one owner per output position, no atomics).
 */
#define SDSP_HIP_ISTFT_NORMALIZED 0
#define SDSP_HIP_ISTFT_RAW 1
typedef struct sdsp_hip_istft_plan sdsp_hip_istft_plan;
/* the synthesis window g (n_fft doubles) of a plan made with these arguments; host only.  Errors as sdsp_hip_istft_plan_create
 * (n_fft is not range-checked against a precision here); a NORMALIZED window that breaks NOLA: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_istft_synthesis_window(uint32_t n_fft, uint32_t hop, const double *window, int norm, double *g);
/* window: n_fft host doubles.  norm: SDSP_HIP_ISTFT_NORMALIZED / _RAW.  workspace_bytes: the slice budget (0 = the default, DESIGN.md
 * section 5.12); a slice holds at least one frame.  Errors: n_fft not a power of two, hop = 0 or hop > n_fft: SDSP_HIP_ERR_INVALID_SIZE;
 * n_fft outside the real-input range of the precision: SDSP_HIP_ERR_UNSUPPORTED; a null pointer, a precision other than F32 / F64, an
 * unknown norm or a window that breaks NOLA: SDSP_HIP_ERR_INVALID_ARG; no device: SDSP_HIP_ERR_NO_DEVICE. */
int sdsp_hip_istft_plan_create(sdsp_hip_istft_plan **plan, uint32_t n_fft, uint32_t hop, const double *window, int norm, int precision,
                               uint64_t workspace_bytes, int device);
int sdsp_hip_istft_plan_destroy(sdsp_hip_istft_plan *plan);
/*
 * in: DEVICE pointer, channel c = in[c in_stride .. + F bins) complex elements of the plan precision.  out: DEVICE pointer, channel
 * c = out[c out_stride .. + F hop) reals.  state: DEVICE pointer or NULL.  Asynchronous on `stream`, allocates nothing
 * (stream-capturable); one call per plan in flight.  Errors: null in / out, in_stride < F bins or out_stride < F hop with more than
 * one channel, overlapping in and out ranges, misaligned pointers: SDSP_HIP_ERR_INVALID_ARG.  channels == 0 or frames == 0:
 * nothing to do.  Measured (1 MI355X, 1024 channels x 2^18 output samples f32, N = 1024, hop = 256, Hann): 3.65 ms against 7.14 ms
 * for pack -> rfft reverse -> x g -> overlap-add (1.96x) and 12.9 ms for torch.istft (3.53x); pack / transform / overlap-add
 * 1.33 / 1.48 / 0.90 ms.  DESIGN.md section 5.12.
 */
int sdsp_hip_istft_process(sdsp_hip_istft_plan *plan, const void *in, uint64_t in_stride, void *out, uint64_t out_stride,
                           uint64_t channels, uint64_t frames, void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_istft_process_host(sdsp_hip_istft_plan *plan, const void *host_in, uint64_t in_stride, void *host_out, uint64_t out_stride,
                                uint64_t channels, uint64_t frames, void *host_state);
/* bytes of a state buffer for `channels` channels: hist channels element size (0 when hop = n_fft) */
int sdsp_hip_istft_state_bytes(const sdsp_hip_istft_plan *plan, uint64_t channels, uint64_t *bytes);
/* the kernel variant of the inner reverse real-input plan (n_real = n_fft, radix 2); SDSP_HIP_ERR_UNSUPPORTED where it has none */
int sdsp_hip_istft_plan_set_variant(sdsp_hip_istft_plan *plan, int variant);
/* kernel launches of one process call of `frames` per channel with a state buffer (the seed launch when hist > 0, then pack,
 * transform and overlap-add launches per slice) */
int sdsp_hip_istft_plan_launches(const sdsp_hip_istft_plan *plan, uint64_t channels, uint64_t frames, uint64_t *launches);
typedef struct {
    uint32_t n_fft, hop, bins, hist;
    int norm, precision, device;
    uint64_t workspace_bytes;
    char kernel[64];         /* the inner transform's kernel */
    double env_min, env_max; /* of env[r] = sum over k of w[r + k hop]^2, r < hop */
} sdsp_hip_istft_plan_info;
int sdsp_hip_istft_plan_get_info(const sdsp_hip_istft_plan *plan, sdsp_hip_istft_plan_info *info);

/* ------------------------------------------------------------------ zero-phase forward-backward filtering of biquad cascades */

/*
 * scipy.signal.sosfiltfilt for `channels` independent rows of a cascaded-biquad bank, in place.  The cascade
 * is the one sdsp_hip_iir_plan_create takes (sections M even, 2 .. 16; kind GENERIC / LP / HP / BP; a, b, gain; F32, F64 or
 * F32_F64STATE), S the sample type and R the recurrence type of the precision.  For each row x of L samples:
 *   1. steady state: s_0 = gain, s_{j+1} = s_j (1 + b1_j + b2_j) / (1 + a1_j + a2_j) in double (the folded numerators 1+2+1, 1-2+1,
 *      1+0-1 for LP / HP / BP): with every age of level j at s_j v the cascade outputs s_M v for a constant input v -- the DF-I
 *      form of scipy.signal.sosfilt_zi.  A section with 1 + a1 + a2 == 0 is refused at plan creation.
 *   2. pad length P: by default scipy's 3 (2M + 1 - min(#{b2_j == 0}, #{a2_j == 0})); any P >= 0 on request; PAD_NONE: P = 0.
 *   3. extension e of L + 2P samples, computed in S: ODD e[i] = 2 x[0] - x[P - i], e[P + L + i] = 2 x[L - 1] - x[L - 2 - i];
 *      EVEN x[P - i] and x[L - 2 - i]; CONSTANT x[0] and x[L - 1].
 *   4. forward: sdsp_hip_iir_process's recurrence over e (the same arithmetic per precision), every age of level j starting at
 *      R(s_j) R(e[0]) rounded in R; outputs u rounded to S.
 *   5. backward: the same over u reversed, from R(s_j) R(u[L + 2P - 1]); outputs rounded to S, reversed, and the middle L written
 *      back.  Row positions [L, stride) are never touched.
 * The result equals pad -> sdsp_hip_iir_process with that state -> flip -> sdsp_hip_iir_process -> flip -> slice bit for bit, and
 * scipy.signal.sosfiltfilt(sos, x, padtype, padlen) in exact arithmetic (sos rows [1, b1, b2, 1, a1, a2], gain in the first row):
 * f64 within ~1e-13 of max |y|, F32_F64STATE within float rounding (1e-6), F32 within the f32 recurrence's accuracy (as for
 * sdsp_hip_iir_process: up to 1e-4 at low normalised cutoffs, f0/fs = 0.005).
 */
#define SDSP_HIP_PAD_NONE 0
#define SDSP_HIP_PAD_ODD 1
#define SDSP_HIP_PAD_EVEN 2
#define SDSP_HIP_PAD_CONSTANT 3
typedef struct sdsp_hip_filtfilt_plan sdsp_hip_filtfilt_plan;
/* s[0 .. sections] of step 1; host only, no device needed.  Errors: sections odd or 0: SDSP_HIP_ERR_INVALID_SIZE; sections > 16:
 * SDSP_HIP_ERR_UNSUPPORTED; an unknown kind, a null pointer (b may be NULL for LP / HP / BP) or a section with 1 + a1 + a2 == 0:
 * SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_iir_steady_state(uint32_t sections, int kind, const double *a, const double *b, double gain, double *s);
/* the default P of step 2; host only.  Errors as sdsp_hip_iir_steady_state (no check of 1 + a1 + a2). */
int sdsp_hip_filtfilt_default_padlen(uint32_t sections, int kind, const double *a, const double *b, uint32_t *padlen);
/* padtype: SDSP_HIP_PAD_*.  padlen < 0: the default; ignored for PAD_NONE.  workspace_bytes: the slice budget, 0 = the default
 * (256 MiB, raised toward 2^17 channels per slice for long edges, at most 1 GiB); a slice holds P samples
 * of each of a multiple of 64 channels, at least 64.  A plan with P = 0 allocates no workspace.  Errors: as sdsp_hip_iir_steady_state, plus an unknown padtype or precision: SDSP_HIP_ERR_INVALID_ARG;
 * padlen >= 2^31: SDSP_HIP_ERR_INVALID_SIZE; no device: SDSP_HIP_ERR_NO_DEVICE. */
int sdsp_hip_filtfilt_plan_create(sdsp_hip_filtfilt_plan **plan, uint32_t sections, int kind, const double *a, const double *b,
                                  double gain, int precision, int padtype, int64_t padlen, uint64_t workspace_bytes, int device);
int sdsp_hip_filtfilt_plan_destroy(sdsp_hip_filtfilt_plan *plan);
/*
 * data: DEVICE pointer, row c = data[c stride .. + samples), filtered in place.  Asynchronous on `stream`, allocates nothing
 * (stream-capturable).  One call per plan in flight: the calls walk the channels in slices of the plan's workspace, so two calls
 * on the SAME plan must not overlap (use one plan per stream).  Errors: samples <= P: SDSP_HIP_ERR_INVALID_SIZE (scipy's
 * ValueError); a null plan or data, stride < samples with more than one channel, data not aligned to its element size:
 * SDSP_HIP_ERR_INVALID_ARG.  channels == 0: nothing to do.  Measured (1 MI355X, 262144 channels x 4096 samples f32, 4 sections,
 * default odd edge): 3.35 ms (65 % of 8 TB/s on 16 B per sample) against 70.0 ms for pad -> process -> flip -> process -> flip ->
 * slice (20.9x; 12.2 ms and 3.64x when the padded rows are 16-byte aligned).  DESIGN.md section 5.13.
 */
int sdsp_hip_filtfilt_process(sdsp_hip_filtfilt_plan *plan, void *data, uint64_t channels, uint64_t samples, uint64_t stride,
                              void *stream);
/* same with a HOST pointer (synchronous) */
int sdsp_hip_filtfilt_process_host(sdsp_hip_filtfilt_plan *plan, void *host_data, uint64_t channels, uint64_t samples,
                                   uint64_t stride);
/* kernel variants (bit-identical): 0 = default -- "sdsp_filtfilt_fused_kernel" (one wave per 64 channels, super-tile transport)
 * for up to 8 sections on 16-byte aligned rows (data pointer and stride), "sdsp_filtfilt_direct_kernel" otherwise; 1 = the direct
 * kernel (one lane per channel, plain accesses: the cross-check) */
int sdsp_hip_filtfilt_plan_set_variant(sdsp_hip_filtfilt_plan *plan, int variant);
/* name of the kernel sdsp_hip_filtfilt_process would launch for this buffer shape with the plan's variant (its first slice; for
 * matching rocprofv3 rows and for tests); the same selection function as the launcher's */
int sdsp_hip_filtfilt_plan_kernel(const sdsp_hip_filtfilt_plan *plan, const void *data, uint64_t channels, uint64_t samples,
                                  uint64_t stride, char *name, size_t name_bytes);
/* kernel launches of one process call: one per workspace slice (0 when channels == 0; samples <= P: SDSP_HIP_ERR_INVALID_SIZE) */
int sdsp_hip_filtfilt_plan_launches(const sdsp_hip_filtfilt_plan *plan, uint64_t channels, uint64_t samples, uint64_t *launches);
typedef struct {
    uint32_t sections, padlen;
    int kind, padtype, precision, device, variant;
    uint64_t workspace_bytes;
    uint64_t slice_channels; /* channels per launch */
    char kernel[64];         /* the kernel the plan's variant runs on aligned rows */
} sdsp_hip_filtfilt_plan_info;
int sdsp_hip_filtfilt_plan_get_info(const sdsp_hip_filtfilt_plan *plan, sdsp_hip_filtfilt_plan_info *info);

/* ------------------------------------------------------------------ Welch power spectral density banks */

/*
 * Welch power spectral density of `channels` independent real streams, accumulated across calls:
 * scipy.signal.welch(x, fs, window, nperseg = N, noverlap = N - hop, detrend, scaling, return_onesided = True, average = "mean").
 * N = n_fft (a power of two in the radix-2 real-input range: f32 32 .. 65536, f64 32 .. 32768), 1 <= hop <= N, bins = N / 2 + 1,
 * hist = N - 1.
 *   - segments are scipy's: segment m >= 0 covers stream samples [m hop, m hop + N).  A call receives `position` (samples of the
 *     stream processed since reset, the same for every channel) and S samples per channel, any S >= 0, and counts exactly the
 *     segments that end inside it: position < m hop + N <= position + S (sdsp_hip_welch_frames).  No segment reaches before sample 0.
 *   - history: state[c hist + j] = x_c[position - 1 - j] (newest first), plan precision; read at entry, written at exit.  NULL is
 *     allowed only with position == 0, and then the final history is dropped.
 *   - detrend, per segment x_0 .. x_{N-1} of plan-precision samples: mu = sum x_n / N and, for LINEAR, beta = sum (n - (N-1)/2) x_n /
 *     (N (N^2 - 1) / 12), in double; trend t_n = mu + beta (n - (N-1)/2) (beta = 0 for CONSTANT); d_n = round_p(x_n - t_n) with the
 *     difference taken in double; windowed sample round_p(d_n w_n).  NONE: round_p(x_n w_n), the STFT bank's frame value.  Sum
 *     order: every lane sums its samples in order, the lanes of a segment then add in an xor butterfly, the waves in ascending order.
 *   - transform: the library's forward real-input plan of n_real = N, radix 2 (unchanged).  p_k = re re + im im in double from the
 *     plan-precision re and im, no FMA contraction; bins 0 and N / 2 from the packed slot 0.
 *   - acc[c acc_stride + k], k < bins: doubles owned by the caller, beside the history.  A call adds its segments' p_k: runs of up to
 *     R segments of one channel are summed in ascending order, then each channel's runs in ascending order, then one addition into
 *     acc (R: DESIGN.md section 5.14).  No atomics: identical calls give identical bits, and a call that counts one segment leaves
 *     acc + p_k with a single rounding.  Block-by-block calls agree with one long call to rounding.
 *   - finalize: out[c out_stride + k] = round_p(acc c_k), c_k = m_k scale / frames_total in double on the host, m_k = 2 for
 *     0 < k < N / 2 and 1 otherwise; scale = 1 / (fs sum w^2) for DENSITY, 1 / (sum w)^2 for SPECTRUM, summed in double over the
 *     plan's rounded window.
 *   - strides count elements.  `in` is never written; nothing past each row's bins of acc or out is.
 * A call runs in slices of the plan's workspace: detrended, windowed segments -> the forward real-input transform -> run sums ->
 * per-channel combine into acc, then one launch for the new history (the STFT bank's state launch with hist = N - 1).
 */
#define SDSP_HIP_DETREND_NONE 0
#define SDSP_HIP_DETREND_CONSTANT 1
#define SDSP_HIP_DETREND_LINEAR 2
#define SDSP_HIP_SCALING_DENSITY 0
#define SDSP_HIP_SCALING_SPECTRUM 1
typedef struct sdsp_hip_welch_plan sdsp_hip_welch_plan;
/* segments one call of `samples` per channel at `position` counts; host only.  n_fft = 0 or hop = 0: SDSP_HIP_ERR_INVALID_SIZE;
 * frames NULL: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_welch_frames(uint32_t n_fft, uint32_t hop, uint64_t position, uint64_t samples, uint64_t *frames);
/* window: n_fft host doubles (sdsp_hip_stft_window gives scipy's periodic windows).  detrend: SDSP_HIP_DETREND_*; scaling:
 * SDSP_HIP_SCALING_*; fs > 0.  workspace_bytes: the slice budget (0 = the default, 256 MiB); a slice of u segments takes
 * u (N size(precision) + (N / 2 + 1) 8) bytes, at least one segment.  Errors: n_fft not a power of two, hop = 0 or hop > n_fft:
 * SDSP_HIP_ERR_INVALID_SIZE; n_fft outside the real-input range of the precision: SDSP_HIP_ERR_UNSUPPORTED; a null pointer, a
 * precision other than F32 / F64, an unknown detrend or scaling, fs <= 0 or not finite: SDSP_HIP_ERR_INVALID_ARG; no device:
 * SDSP_HIP_ERR_NO_DEVICE. */
int sdsp_hip_welch_plan_create(sdsp_hip_welch_plan **plan, uint32_t n_fft, uint32_t hop, const double *window, int detrend, int scaling,
                               double fs, int precision, uint64_t workspace_bytes, int device);
int sdsp_hip_welch_plan_destroy(sdsp_hip_welch_plan *plan);
/*
 * in: DEVICE pointer, channel c = in[c in_stride .. + samples).  state: DEVICE pointer (or NULL at position 0).  acc: DEVICE pointer,
 * doubles, channel c = acc[c acc_stride .. + bins).  Asynchronous on `stream`, allocates nothing (stream-capturable); one call per
 * plan in flight.  Errors: a null plan, in or acc, state NULL with position > 0, in_stride < samples or acc_stride < bins with more
 * than one channel, `in` overlapping state or acc, misaligned pointers: SDSP_HIP_ERR_INVALID_ARG.  channels == 0 or samples == 0:
 * nothing to do.  DESIGN.md section 5.14.
 */
int sdsp_hip_welch_process(sdsp_hip_welch_plan *plan, const void *in, uint64_t in_stride, uint64_t channels, uint64_t samples,
                           uint64_t position, void *state, double *acc, uint64_t acc_stride, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_welch_process_host(sdsp_hip_welch_plan *plan, const void *host_in, uint64_t in_stride, uint64_t channels, uint64_t samples,
                                uint64_t position, void *host_state, double *host_acc, uint64_t acc_stride);
/* out: DEVICE pointer, plan precision, channel c = out[c out_stride .. + bins).  frames_total: the segments acc holds.  Asynchronous,
 * one launch.  Errors: frames_total == 0: SDSP_HIP_ERR_INVALID_SIZE; a null plan, acc or out, acc_stride or out_stride < bins with
 * more than one channel, overlapping acc and out, misaligned pointers: SDSP_HIP_ERR_INVALID_ARG.  channels == 0: nothing to do. */
int sdsp_hip_welch_finalize(sdsp_hip_welch_plan *plan, const double *acc, uint64_t acc_stride, uint64_t frames_total, void *out,
                            uint64_t out_stride, uint64_t channels, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_welch_finalize_host(sdsp_hip_welch_plan *plan, const double *host_acc, uint64_t acc_stride, uint64_t frames_total,
                                 void *host_out, uint64_t out_stride, uint64_t channels);
/* bytes of a state buffer for `channels` channels: (n_fft - 1) channels element size */
int sdsp_hip_welch_state_bytes(const sdsp_hip_welch_plan *plan, uint64_t channels, uint64_t *bytes);
/* kernel launches of one process call of `samples` per channel at `position` with a state buffer (frame, transform, run and combine
 * launches per slice, plus the state launch when samples > 0); finalize is one more */
int sdsp_hip_welch_plan_launches(const sdsp_hip_welch_plan *plan, uint64_t channels, uint64_t samples, uint64_t position,
                                 uint64_t *launches);
typedef struct {
    uint32_t n_fft, hop, bins, hist;
    int detrend, scaling;
    double fs;
    int precision, device;
    uint64_t workspace_bytes;
    char kernel[64]; /* the inner transform's kernel */
} sdsp_hip_welch_plan_info;
int sdsp_hip_welch_plan_get_info(const sdsp_hip_welch_plan *plan, sdsp_hip_welch_plan_info *info);

/* ------------------------------------------------------------------ cross-spectral density and coherence banks */

/*
 * Welch cross-spectral density and magnitude-squared coherence of pairs of `channels` real streams, accumulated across calls
 * (DESIGN.md section 5.18): scipy.signal.csd(x_a, x_b, fs, window, nperseg = N, noverlap = N - hop, detrend, scaling) and
 * scipy.signal.coherence(x_a, x_b, ...) for a list of `npairs` channel pairs (a_i, b_i) fixed at plan creation.  a_i == b_i is
 * allowed and a pair may appear more than once.  N, hop, bins = N / 2 + 1 and hist = N - 1 are the Welch bank's, and so are
 *   - the segments and `position` (sdsp_hip_welch_frames counts the segments of a call), the history (state[c hist + j] =
 *     x_c[position - 1 - j], plan precision, NULL only at position 0), the detrended, windowed segment value round_p(d_n w_n) with its
 *     sum order, and the transform (the library's forward real-input plan of n_real = N, radix 2, unchanged).
 *   - cross power: with X_a = (ar, ai) and Y_b = (br, bi) the plan-precision spectra of one segment at bin k, widened to double,
 *     re = ar br + ai bi and im = ar bi - ai br (scipy's conj(X) Y), every product and sum rounded on its own, no FMA contraction.
 *     Bins 0 and N / 2 come from the packed slot 0: bin 0 has re = ar br, bin N / 2 has re = ai bi, both with im = +0.0.
 *   - accumulators, doubles owned by the caller: acc_xy[i acc_xy_stride + 2 k + {0, 1}] = re, im of pair i, k < bins; acc_auto[c
 *     acc_auto_stride + k] = the sum of re re + im im of channel c (the Welch bank's acc), optional: NULL skips the auto spectra, and
 *     coherence then cannot be finalized.
 *   - slices and sum order: a call runs in slices, each a range [ja, jb) of the call's segments of ALL channels; a slice of u segment
 *     columns takes u column_bytes of the workspace, column_bytes = channels N size(precision) + (2 npairs + channels) (N / 2 + 1) 8
 *     (segments, then one partial row per pair and per channel), so jb - ja <= workspace_bytes / column_bytes.  Per (pair or channel,
 *     bin) and slice: runs of R consecutive segments are summed in ascending order, then the runs in ascending order, then one
 *     addition into the accumulator; R is the Welch bank's run length for jb - ja segments.  Every
 *     accumulator element has one owner per launch: no atomics.
 *   Consequences: identical calls give identical bits; a call that counts one segment adds one product with a single rounding, so
 *   acc_auto and the real part of a pair (c, c) then equal the Welch bank's acc bit for bit; pair (b, a) is the exact complex
 *   conjugate of pair (a, b) for any slicing; pair (c, c) has im == 0 exactly and its real part has the bits of acc_auto[c];
 *   block-by-block calls agree with one long call to rounding.
 *   - finalize, one launch.  SDSP_HIP_CSD_CROSS: out[i out_stride + 2 k + {0, 1}] = round_p(re c_k), round_p(im c_k), c_k the Welch
 *     bank's host double m_k scale / frames_total.  SDSP_HIP_CSD_COHERENCE: out[i out_stride + k] = round_p((re re + im im) /
 *     (A_a A_b)) with A from acc_auto, a plain IEEE division in double: scale and frame count cancel and are not applied, 0 / 0 is NaN
 *     as in scipy, nothing is clamped.
 *   - strides count real elements (doubles for the accumulators, plan precision for in and out).  `in` is never written; nothing
 *     past each row's 2 bins (acc_xy, CROSS out) or bins (acc_auto, COHERENCE out) elements is.
 */
#define SDSP_HIP_CSD_CROSS 0
#define SDSP_HIP_CSD_COHERENCE 1
typedef struct sdsp_hip_csd_plan sdsp_hip_csd_plan;
/* n_fft, hop, window, detrend, scaling, fs, precision: as sdsp_hip_welch_plan_create.  channels: fixed per plan, since a slice holds
 * the same segments of every channel.  pairs: npairs x 2 host channel indices (a_i, b_i).  workspace_bytes: the slice budget (0 = the
 * default, 256 MiB), used in whole columns.  Errors: those of sdsp_hip_welch_plan_create; channels == 0 or npairs == 0:
 * SDSP_HIP_ERR_INVALID_SIZE; pairs NULL or an index >= channels: SDSP_HIP_ERR_INVALID_ARG; a budget below one column, or sizes whose
 * column does not fit 64 bits: SDSP_HIP_ERR_UNSUPPORTED. */
int sdsp_hip_csd_plan_create(sdsp_hip_csd_plan **plan, uint32_t n_fft, uint32_t hop, const double *window, int detrend, int scaling,
                             double fs, int precision, uint64_t channels, uint64_t npairs, const uint32_t *pairs,
                             uint64_t workspace_bytes, int device);
int sdsp_hip_csd_plan_destroy(sdsp_hip_csd_plan *plan);
/*
 * in: DEVICE pointer, channel c = in[c in_stride .. + samples), the plan's `channels` rows.  state: DEVICE pointer (or NULL at
 * position 0).  acc_xy: DEVICE doubles, pair i = acc_xy[i acc_xy_stride .. + 2 bins).  acc_auto: DEVICE doubles, channel c =
 * acc_auto[c acc_auto_stride .. + bins), or NULL.  Asynchronous on `stream`, allocates nothing (stream-capturable as a linear chain of
 * launches); one call per plan in flight.  Errors: a null plan, in or acc_xy, state NULL with position > 0, in_stride < samples with
 * more than one channel, acc_xy_stride < 2 bins with more than one pair, acc_auto_stride < bins with more than one channel, `in`
 * overlapping state or an accumulator, the accumulators overlapping each other, misaligned pointers: SDSP_HIP_ERR_INVALID_ARG; more
 * than 2^32 - 1 samples between the first and the last segment of one call: SDSP_HIP_ERR_UNSUPPORTED.  samples == 0: nothing to do.
 */
int sdsp_hip_csd_process(sdsp_hip_csd_plan *plan, const void *in, uint64_t in_stride, uint64_t samples, uint64_t position, void *state,
                         double *acc_xy, uint64_t acc_xy_stride, double *acc_auto, uint64_t acc_auto_stride, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_csd_process_host(sdsp_hip_csd_plan *plan, const void *host_in, uint64_t in_stride, uint64_t samples, uint64_t position,
                              void *host_state, double *host_acc_xy, uint64_t acc_xy_stride, double *host_acc_auto,
                              uint64_t acc_auto_stride);
/* mode: SDSP_HIP_CSD_CROSS (out: npairs rows of 2 bins plan-precision values) or SDSP_HIP_CSD_COHERENCE (npairs rows of bins values);
 * out: DEVICE pointer.  frames_total: the segments the accumulators hold.  Asynchronous, one launch.  Errors: frames_total == 0:
 * SDSP_HIP_ERR_INVALID_SIZE; a null plan, acc_xy or out, an unknown mode, COHERENCE with acc_auto NULL, strides below the row with more
 * than one row, out overlapping an accumulator, misaligned pointers: SDSP_HIP_ERR_INVALID_ARG.  acc_auto is not read in CROSS mode. */
int sdsp_hip_csd_finalize(sdsp_hip_csd_plan *plan, int mode, const double *acc_xy, uint64_t acc_xy_stride, const double *acc_auto,
                          uint64_t acc_auto_stride, uint64_t frames_total, void *out, uint64_t out_stride, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_csd_finalize_host(sdsp_hip_csd_plan *plan, int mode, const double *host_acc_xy, uint64_t acc_xy_stride,
                               const double *host_acc_auto, uint64_t acc_auto_stride, uint64_t frames_total, void *host_out,
                               uint64_t out_stride);
/* bytes of the plan's state buffer: (n_fft - 1) channels element size */
int sdsp_hip_csd_state_bytes(const sdsp_hip_csd_plan *plan, uint64_t *bytes);
/* kernel launches of one process call of `samples` per channel at `position` with a state buffer (frame, transform, run and combine
 * launches per slice, plus the state launch when samples > 0); finalize is one more */
int sdsp_hip_csd_plan_launches(const sdsp_hip_csd_plan *plan, uint64_t samples, uint64_t position, uint64_t *launches);
typedef struct {
    uint32_t n_fft, hop, bins, hist;
    int detrend, scaling;
    double fs;
    int precision, device;
    uint64_t channels, npairs;
    uint64_t column_bytes;    /* workspace bytes of one segment column (the formula above) */
    uint64_t slice_columns;   /* segment columns per slice: workspace_bytes / column_bytes */
    uint64_t workspace_bytes; /* slice_columns column_bytes */
    char kernel[64];          /* the inner transform's kernel */
} sdsp_hip_csd_plan_info;
int sdsp_hip_csd_plan_get_info(const sdsp_hip_csd_plan *plan, sdsp_hip_csd_plan_info *info);

/* ------------------------------------------------------------------ polyphase filter-bank channelizer banks */

/*
 * Polyphase filter bank (PFB) of `channels` independent streams: every stream is split into M equally spaced
 * sub-bands with a prototype low-pass of L = P M taps h[0 .. L), one M-point transform per frame.  M = channels_m (a power of two),
 * P = taps_per_channel (1 .. SDSP_HIP_PFB_MAX_TAPS_PER_CHANNEL), L <= 2^20, D = hop (1 <= D <= M; D = M critically sampled, D = M / 2
 * oversampled by 2), hist = L - D.  A call takes S samples per channel, S a multiple of D, and writes exactly F = S / D frames.  With
 * x = the channel's history followed by the block (the block starts at index hist), frame j of the call is
 *     u_j[r] = sum over p < P of fl(x[j D + p M + r] h[p M + r]),  0 <= r < M     (ascending p; every product and sum rounded on its own)
 *     Y_j[k] = sum over r < M of v_j[r] e^(-2 pi i k r / M)                       (the library's forward transform, unchanged)
 *   - phase FRAME: v_j = u_j.  Y_j[k] is bin k P of the L-point STFT with window h:
 *     torch.stft(concat(history, block), n_fft = L, hop = D, window = h, center = False)[k P].
 *   - phase TIME: v_j[(r + s_j) mod M] = u_j[r] with s_j = (position + j D - hist) mod M, a circular shift by the absolute index of the
 *     frame's first sample: Y_j[k] = sum over n of x[n0 + n] h[n] e^(-2 pi i k (n0 + n) / M), n0 that absolute index -- every sub-band
 *     is a down-converted baseband signal whose phase is continuous from frame to frame for any D.  `position` is the number of samples
 *     of the stream that earlier calls consumed.  For D = M and position a multiple of M both references coincide.
 *   - h multiplies x in window (correlation) order, as the STFT window does: a caller who thinks in convolution order (y = x * g)
 *     passes the reversed taps h[n] = g[L - 1 - n].  A symmetric prototype is the same either way.
 *   - input kinds: REAL = samples of the plan precision, M / 2 + 1 bins per frame through the real-input plans (M in their radix-2
 *     range: f32 32 .. 65536, f64 32 .. 32768; bins 0 and M / 2 with zero imaginary parts -- the STFT bank's COMPLEX layout);
 *     COMPLEX = interleaved complex samples (real and imaginary parts folded separately with the real tap), M bins per frame in
 *     natural order through the complex plans (SDSP_HIP_RADIX_AUTO; M = 16 .. 65536 in f32, 16 .. 32768 in f64).
 *   - history: state[c hist + j] = x_c[-1 - j] (newest first), elements of the input kind; read at entry, written at exit; NULL = zero
 *     history, final history dropped.  A fresh stream (NULL or zeroed state) is the stream with hist zeros in front of it.
 *   - block-by-block calls equal one long call bit for bit for any split into multiples of D (blocks shorter than hist included).
 *   - the taps: L host doubles, rounded once to the plan precision at creation.
 *   - strides count elements (a complex sample or bin is one element).  `in` is never written; nothing past each channel's F bins
 *     outputs is.  Output is complex: out[c out_stride + j bins + k].
 * A call runs in slices of the workspace budget: fold -> transform (-> unpack to the output rows, REAL), then one launch for the new
 * history.  REAL folds into the plan's workspace; COMPLEX folds straight into the output rows and transforms them in place (no
 * workspace is allocated; the budget only sets the slice).
 */
#define SDSP_HIP_PFB_REAL 0
#define SDSP_HIP_PFB_COMPLEX 1
#define SDSP_HIP_PFB_PHASE_FRAME 0
#define SDSP_HIP_PFB_PHASE_TIME 1
#define SDSP_HIP_PFB_MAX_TAPS_PER_CHANNEL 64
#define SDSP_HIP_PFB_MAX_TAPS (1u << 20)
typedef struct sdsp_hip_pfb_plan sdsp_hip_pfb_plan;
/* the windowed-sinc prototype of p m taps with cutoff at half the sub-band spacing and unit DC gain, host only:
 * scipy.signal.firwin(p m, 1.0 / m, window = name) for the four SDSP_HIP_WINDOW_* kinds (firwin's SYMMETRIC window, not the periodic
 * one sdsp_hip_stft_window returns).  m < 2, p = 0, p > SDSP_HIP_PFB_MAX_TAPS_PER_CHANNEL or p m > SDSP_HIP_PFB_MAX_TAPS:
 * SDSP_HIP_ERR_INVALID_SIZE; unknown kind or h NULL: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_pfb_prototype(int window_kind, uint32_t m, uint32_t p, double *h);
/* frames one call of `samples` per channel writes (samples / hop); host only.  Errors as sdsp_hip_stft_frames. */
int sdsp_hip_pfb_frames(uint32_t hop, uint64_t samples, uint64_t *frames);
/* taps: p m host doubles.  workspace_bytes: the slice budget (0 = the default, 256 MiB); a slice holds at least one frame.  Errors:
 * channels_m not a power of two, taps_per_channel = 0 or above the maximum, p m > SDSP_HIP_PFB_MAX_TAPS, hop = 0 or hop > channels_m:
 * SDSP_HIP_ERR_INVALID_SIZE; channels_m outside the transform range of the kind and precision: SDSP_HIP_ERR_UNSUPPORTED; a null
 * pointer, a precision other than F32 / F64, an unknown input kind or phase: SDSP_HIP_ERR_INVALID_ARG; no device:
 * SDSP_HIP_ERR_NO_DEVICE. */
int sdsp_hip_pfb_plan_create(sdsp_hip_pfb_plan **plan, uint32_t channels_m, uint32_t taps_per_channel, uint32_t hop, const double *taps,
                             int input_kind, int phase, int precision, uint64_t workspace_bytes, int device);
int sdsp_hip_pfb_plan_destroy(sdsp_hip_pfb_plan *plan);
/*
 * in: DEVICE pointer, channel c = in[c in_stride .. + samples) elements.  out: DEVICE pointer, channel c = out[c out_stride .. + F bins)
 * complex elements.  state: DEVICE pointer or NULL.  position: samples of the stream consumed before this call (phase TIME; ignored for
 * FRAME).  Asynchronous on `stream`, allocates nothing (stream-capturable); one call per plan in flight.  Errors: samples % hop != 0:
 * SDSP_HIP_ERR_INVALID_SIZE; null plan, in or out, in_stride < samples or out_stride < F bins with more than one channel, overlapping
 * in and out ranges, misaligned pointers: SDSP_HIP_ERR_INVALID_ARG.  channels == 0 or samples == 0: nothing to do.
 */
int sdsp_hip_pfb_process(sdsp_hip_pfb_plan *plan, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t channels,
                         uint64_t samples, uint64_t position, void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_pfb_process_host(sdsp_hip_pfb_plan *plan, const void *host_in, uint64_t in_stride, void *host_out, uint64_t out_stride,
                              uint64_t channels, uint64_t samples, uint64_t position, void *host_state);
/* bytes of a state buffer for `channels` channels: hist channels element size (0 when p = 1 and hop = channels_m) */
int sdsp_hip_pfb_state_bytes(const sdsp_hip_pfb_plan *plan, uint64_t channels, uint64_t *bytes);
/* the kernel variant of the inner transform plan (sdsp_hip_fft_plan_set_variant); SDSP_HIP_ERR_UNSUPPORTED where it has no such variant */
int sdsp_hip_pfb_plan_set_variant(sdsp_hip_pfb_plan *plan, int variant);
/* measurement and cross-check hook: 0 = the fold form the sizes select (sliding where hop divides channels_m, else plain), 1 = the
 * plain per-frame form for every hop.  Both forms give the same bits. */
int sdsp_hip_pfb_plan_set_fold_form(sdsp_hip_pfb_plan *plan, int form);
/* kernel launches of one process call of `samples` per channel with a state buffer and out_stride = F bins */
int sdsp_hip_pfb_plan_launches(const sdsp_hip_pfb_plan *plan, uint64_t channels, uint64_t samples, uint64_t *launches);
typedef struct {
    uint32_t channels_m, taps_per_channel, hop, bins, hist;
    int input_kind, phase, precision, device;
    uint64_t workspace_bytes; /* allocated (REAL) or the slice budget in use (COMPLEX) */
    char kernel[64];          /* the inner transform's kernel */
    char fold[16];            /* "sliding" or "plain" */
} sdsp_hip_pfb_plan_info;
int sdsp_hip_pfb_plan_get_info(const sdsp_hip_pfb_plan *plan, sdsp_hip_pfb_plan_info *info);

/* ------------------------------------------------------------------ polyphase synthesis filter banks (inverse channelizer) */

/*
 * The synthesis half of the polyphase filter bank: `channels` independent streams are rebuilt from frames of
 * M sub-bands in sdsp_hip_pfb_process's output layout.  M, P, L = P M, D, hist = L - D as above; g[0 .. L) is the synthesis prototype.
 * A call takes F frames of `bins` complex values per channel and writes exactly F D samples per channel.  For frame j of the call:
 *     v_j = the library's reverse M-point transform of the frame, 1 / M scaled (COMPLEX: the complex SDSP_HIP_RADIX_AUTO plan over M
 *           bins; REAL: the real-input plan over M / 2 + 1 bins, the imaginary parts of bins 0 and M / 2 ignored, as the inverse STFT)
 *     u_j = v_j (phase FRAME), or u_j[r] = v_j[(r + s_j) mod M] with s_j = (position + j D - hist) mod M (phase TIME: the analysis
 *           bank's s_j; `position` is the number of samples per channel that earlier calls produced)
 * Output position t of the call starts from the pending sum at t where one exists (t < hist and a state was given), else from 0, and
 * receives fl(g[t - j D] u_j[(t - j D) mod M]) for every frame j with 0 <= t - j D < L, added in ascending j, every product and sum
 * rounded on its own (COMPLEX: real and imaginary parts multiplied separately by the real tap).  Positions t < F D go to out,
 * positions F D <= t < F D + hist are the new pending sums.
 *   - state: hist elements of the output kind per channel, in time order; read at entry, written at exit; none when P = 1 and D = M.
 *     NULL = start from zero and drop the tail.
 *   - block-by-block calls equal one long call bit for bit for any split into frame counts (F D < hist included).
 *   - with g a dual of the analysis prototype (sdsp_hip_pfb_dual_prototype), synthesis(analysis(x)), both fresh, is x delayed by hist
 *     samples, for both kinds and both phases.
 *   - the two limits: P = 1, FRAME, REAL is the inverse STFT bank with SDSP_HIP_ISTFT_RAW and window g; P = 1, D = M is the plain
 *     reverse transform times g.
 *   - strides count elements.  `in` is never written; in and out may not overlap; nothing outside each channel's F D output elements
 *     and its state row is written.  The taps: L host doubles, rounded once to the plan precision at creation.
 * A call runs as one launch that moves the old pending sums to their places, then slices of the workspace budget: spectra into the
 * workspace (REAL: packed) -> reverse transform in place -> unfold (one owner per output position, no atomics).
 */
typedef struct sdsp_hip_pfb_synth_plan sdsp_hip_pfb_synth_plan;
/* the minimum-norm synthesis prototype g (p m doubles) that reconstructs through the analysis prototype h (p m doubles) at this hop,
 * host only: for every t0 in [0, hop) and every k in (-p, p), sum over i of g[t0 + i hop] h[t0 + i hop + k m] = (k == 0), over the i
 * whose two indices lie in [0, p m).  Solved per t0 in double by a singular value decomposition (no normal equations).  Where the
 * largest residual exceeds 1e-9 no dual of this support exists: SDSP_HIP_ERR_INVALID_ARG (hops above m / 2 with p > 1, typically).
 * Size errors as sdsp_hip_pfb_prototype, and hop = 0 or hop > m: SDSP_HIP_ERR_INVALID_SIZE; h or g NULL: SDSP_HIP_ERR_INVALID_ARG.
 * Cost: O(p^2 L) flops per Jacobi sweep over all residues together, a handful of sweeps -- milliseconds
 * for the usual shapes, seconds at L = 2^20 with p = 8, and minutes at the extreme p = 64, L = 2^20 (one thread, no progress report). */
int sdsp_hip_pfb_dual_prototype(uint32_t m, uint32_t p, uint32_t hop, const double *h, double *g);
/* taps: the synthesis prototype, p m host doubles.  output_kind: SDSP_HIP_PFB_REAL or SDSP_HIP_PFB_COMPLEX; phase: SDSP_HIP_PFB_PHASE_*.
 * workspace_bytes: the slice budget (0 = the default, 256 MiB); a slice holds at least one frame.  Errors and size ranges are those of
 * sdsp_hip_pfb_plan_create. */
int sdsp_hip_pfb_synth_plan_create(sdsp_hip_pfb_synth_plan **plan, uint32_t channels_m, uint32_t taps_per_channel, uint32_t hop,
                                   const double *taps, int output_kind, int phase, int precision, uint64_t workspace_bytes, int device);
int sdsp_hip_pfb_synth_plan_destroy(sdsp_hip_pfb_synth_plan *plan);
/*
 * in: DEVICE pointer, channel c = in[c in_stride .. + frames bins) complex elements.  out: DEVICE pointer, channel c = out[c out_stride ..
 * + frames hop) elements of the output kind.  state: DEVICE pointer or NULL.  position: samples per channel produced before this call
 * (phase TIME; ignored for FRAME).  Asynchronous on `stream`, allocates nothing (stream-capturable); one call per plan in flight.
 * Errors: null plan, in or out, in_stride < frames bins or out_stride < frames hop with more than one channel, overlapping in and out
 * ranges, misaligned pointers: SDSP_HIP_ERR_INVALID_ARG.  channels == 0 or frames == 0: nothing to do.
 */
int sdsp_hip_pfb_synth_process(sdsp_hip_pfb_synth_plan *plan, const void *in, uint64_t in_stride, void *out, uint64_t out_stride,
                               uint64_t channels, uint64_t frames, uint64_t position, void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_pfb_synth_process_host(sdsp_hip_pfb_synth_plan *plan, const void *host_in, uint64_t in_stride, void *host_out,
                                    uint64_t out_stride, uint64_t channels, uint64_t frames, uint64_t position, void *host_state);
/* bytes of a state buffer for `channels` channels: hist channels element size (0 when p = 1 and hop = channels_m) */
int sdsp_hip_pfb_synth_state_bytes(const sdsp_hip_pfb_synth_plan *plan, uint64_t channels, uint64_t *bytes);
/* the kernel variant of the inner reverse plan (sdsp_hip_fft_plan_set_variant); SDSP_HIP_ERR_UNSUPPORTED where it has no such variant */
int sdsp_hip_pfb_synth_plan_set_variant(sdsp_hip_pfb_synth_plan *plan, int variant);
/* measurement and cross-check hook: 0 = the unfold form the sizes select (sliding where hop = channels_m, else plain), 1 = the plain
 * per-position form for every hop.  Both forms give the same bits. */
int sdsp_hip_pfb_synth_plan_set_unfold_form(sdsp_hip_pfb_synth_plan *plan, int form);
/* kernel launches of one process call of `frames` per channel with a state buffer */
int sdsp_hip_pfb_synth_plan_launches(const sdsp_hip_pfb_synth_plan *plan, uint64_t channels, uint64_t frames, uint64_t *launches);
typedef struct {
    uint32_t channels_m, taps_per_channel, hop, bins, hist;
    int output_kind, phase, precision, device;
    uint64_t workspace_bytes;
    char kernel[64];          /* the inner reverse transform's kernel */
    char unfold[16];          /* "sliding" or "plain" */
} sdsp_hip_pfb_synth_plan_info;
int sdsp_hip_pfb_synth_plan_get_info(const sdsp_hip_pfb_synth_plan *plan, sdsp_hip_pfb_synth_plan_info *info);

/* ------------------------------------------------------------------ digital down-converter banks */

/*
 * Digital down-converter (DDC) bank: from `channels` independent input streams, `nb` bands at arbitrary centre
 * frequencies are shifted to baseband, low-pass filtered with one real T-tap filter h and decimated by D, with the oscillator phase
 * continuous across calls.  A band is (src, fcw, phase0): the input channel and two 32-bit phase words, frequency = fcw / 2^32 cycles
 * per sample (fcw >= 2^31 is a negative frequency), phase0 / 2^32 cycles.  A call takes S samples per channel, S a multiple of D, and
 * writes exactly S / D interleaved complex outputs per BAND: out[i out_stride + m].  `position` is the number of samples of the stream
 * that earlier calls consumed.  With x = history followed by the block and n = position + m D, output m of band i is, mathematically,
 *     y_i[m] = sum over k < T of h[k] x_src[n - k] e^(-2 pi i (phase0_i + fcw_i (n - k)) / 2^32)
 * (mix, FIR, keep every D-th sample).  It is computed in the factored form, which is the bit-level definition:
 *   - band taps, host, at plan creation: g_i[k] = h[k] e^(+2 pi i (k fcw_i mod 2^32) / 2^32) -- the integer reduction is exact, cos and
 *     sin are taken in double, the two products (sdsp_hip_ddc_band_taps) are rounded once to the plan precision.
 *   - oscillator tables, host, double, rounded once to the plan precision (sdsp_hip_ddc_oscillator):
 *     C[a] = e^(-2 pi i a / 65536), F[b] = e^(-2 pi i b / 2^32), a, b < 65536.
 *   - phase index of an output: j = (phase0_i + fcw_i n) mod 2^32 in unsigned integers, exact at any stream position.
 *   - oscillator value w = C[j >> 16] (x) F[j & 0xffff], where (a (x) b).re = a.re b.re - a.im b.im and (a (x) b).im = a.re b.im + a.im b.re:
 *     two products and one sum or difference, each rounded on its own, never contracted.
 *   - filter sum z = sum over k of g_i[k] x[n - k] in ascending k, accumulators starting at +0.  REAL: per tap zr += gr x, zi += gi x.
 *     COMPLEX: per tap, in this order, zr += gr xr, zr -= gi xi, zi += gr xi, zi += gi xr.  Every step is one fmaf in f32 and a multiply
 *     then an add, each rounded, in f64 (the resampler's rule).
 *   - output y = z (x) w.
 *   - history: H = T - 1 elements of the input kind per INPUT CHANNEL (not per band), state[c H + j] = x_c[-1 - j] (newest first); read at
 *     entry, written at exit; NULL = zero history, final history dropped.
 *   - block-by-block calls equal one long call bit for bit for any split into multiples of D when the caller advances `position`
 *     (blocks shorter than H and blocks of 0 samples included); position and position + 2^32 give the same bits.
 *   - input kinds: REAL = samples of the plan precision; COMPLEX = interleaved I/Q (one complex sample is one element, as in the PFB bank).
 *   - strides count elements.  `in` is never written; nothing past each band's S / D outputs is.
 * Limits: 1 <= T <= SDSP_HIP_FIR_MAX_TAPS, 1 <= D <= SDSP_HIP_RESAMPLE_MAX_FACTOR, 1 <= nb <= 65536, channels >= 1.  The bands, the taps
 * and D are fixed at plan creation.  sdsp_hip_resample_design(T, 1, D, h) is the matching anti-aliasing low-pass for D >= 2.
 */
#define SDSP_HIP_DDC_REAL 0
#define SDSP_HIP_DDC_COMPLEX 1
#define SDSP_HIP_DDC_MAX_BANDS 65536
typedef struct sdsp_hip_ddc_plan sdsp_hip_ddc_plan;
typedef struct {
    uint32_t src;    /* input channel */
    uint32_t fcw;    /* frequency, cycles per sample in units of 2^-32 */
    uint32_t phase0; /* phase at stream position 0, cycles in units of 2^-32 */
} sdsp_hip_ddc_band;
/* round(f 2^32) mod 2^32 for f in [-0.5, 0.5] (ties to the even word), host only; anything else (NaN included) or fcw NULL:
 * SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_ddc_phase_word(double cycles_per_sample, uint32_t *fcw);
/* the band taps before rounding to a plan precision, host only: g[2 k], g[2 k + 1] = h[k] cos, h[k] sin of 2 pi (k fcw mod 2^32) / 2^32.
 * taps out of range: SDSP_HIP_ERR_INVALID_SIZE; a null pointer: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_ddc_band_taps(uint32_t taps, const double *h, uint32_t fcw, double *g);
/* the oscillator tables before rounding, host only: 2 x 65536 doubles each (interleaved re, im).  The values on the axes are exact
 * (C[32768] = (-1, +0)). */
int sdsp_hip_ddc_oscillator(double *coarse, double *fine);
/* outputs per band of one call of `samples` per channel (S / D), host only.  down out of range or samples % down != 0:
 * SDSP_HIP_ERR_INVALID_SIZE; out NULL: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_ddc_out_samples(uint32_t down, uint64_t samples, uint64_t *out);
/* h: taps host doubles; bands: nb entries.  The plan rounds the products of sdsp_hip_ddc_band_taps and sdsp_hip_ddc_oscillator to its
 * precision.  Errors: taps, down, channels = 0, nb = 0 or nb > SDSP_HIP_DDC_MAX_BANDS: SDSP_HIP_ERR_INVALID_SIZE; a null pointer, a
 * band with src >= channels, an unknown input kind, a precision other than F32 / F64: SDSP_HIP_ERR_INVALID_ARG; no device:
 * SDSP_HIP_ERR_NO_DEVICE. */
int sdsp_hip_ddc_plan_create(sdsp_hip_ddc_plan **plan, uint32_t taps, const double *h, uint32_t down, uint32_t channels, uint32_t nb,
                             const sdsp_hip_ddc_band *bands, int input_kind, int precision, int device);
int sdsp_hip_ddc_plan_destroy(sdsp_hip_ddc_plan *plan);
/*
 * in: DEVICE pointer, channel c = in[c in_stride .. + samples) elements of the input kind.  out: DEVICE pointer, band i = out[i out_stride
 * .. + S / D) complex elements.  state: DEVICE pointer or NULL.  Asynchronous on `stream`, allocates nothing (stream-capturable); one
 * call per plan in flight.  Errors: samples % down != 0: SDSP_HIP_ERR_INVALID_SIZE; null plan, in or out, in_stride < samples with more
 * than one channel, out_stride < S / D with more than one band, overlapping in and out ranges, misaligned pointers:
 * SDSP_HIP_ERR_INVALID_ARG; a grid that does not fit one launch: SDSP_HIP_ERR_UNSUPPORTED.  samples == 0: nothing to do.
 */
int sdsp_hip_ddc_process(sdsp_hip_ddc_plan *plan, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t samples,
                         uint64_t position, void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_ddc_process_host(sdsp_hip_ddc_plan *plan, const void *host_in, uint64_t in_stride, void *host_out, uint64_t out_stride,
                              uint64_t samples, uint64_t position, void *host_state);
/* bytes of the plan's state buffer: H channels element size (0 when T = 1) */
int sdsp_hip_ddc_state_bytes(const sdsp_hip_ddc_plan *plan, uint64_t *bytes);
/* kernel variants (identical values, bit for bit): 0 = sdsp_ddc_kernel, the fused form (each channel's block staged in LDS once for all
 * of its bands); 1 = sdsp_ddc_plain_kernel, one output per thread from global memory (the cross-check). */
int sdsp_hip_ddc_plan_set_variant(sdsp_hip_ddc_plan *plan, int variant);
/* kernel launches of one process call of `samples` per channel with a state buffer: the band kernel, and one for the new history
 * when T > 1; 0 for samples == 0 */
int sdsp_hip_ddc_plan_launches(const sdsp_hip_ddc_plan *plan, uint64_t samples, uint64_t *launches);
typedef struct {
    uint32_t taps, down, channels, bands;
    uint32_t hist;      /* H = taps - 1 */
    uint32_t block_out; /* outputs per band one workgroup of sdsp_ddc_kernel produces from one LDS block (block_out down inputs) */
    int input_kind, precision, device;
    char kernel[64];    /* the kernel the plan's variant runs */
} sdsp_hip_ddc_plan_info;
int sdsp_hip_ddc_plan_get_info(const sdsp_hip_ddc_plan *plan, sdsp_hip_ddc_plan_info *info);

/* ------------------------------------------------------------------ digital up-converter banks */

/*
 * Digital up-converter (DUC) bank, the mirror of the DDC bank: `nb` baseband complex band streams, all at the
 * same low rate, are interpolated by U through one real T-tap low-pass h in polyphase form, shifted up to their centre frequencies
 * and summed into `channels` output streams, with the oscillator phase continuous across calls.  A band is (dst, fcw, phase0): the
 * output channel and the DDC's two 32-bit phase words (sdsp_hip_ddc_phase_word).  A call takes S input samples per BAND (any S >= 0, no
 * multiple required) and writes exactly S U outputs per CHANNEL: out[c out_stride + r].  `position` is the number of input samples
 * per band that earlier calls consumed.  With x = a band's history followed by its block, output r of the call has m = r div U,
 * p = r mod U and the stream index n = position U + r; mathematically
 *     out_c[r] = sum over the bands i with dst_i = c of e^(+2 pi i (phase0_i + fcw_i n) / 2^32) sum over q of h[q U + p] x_i[m - q].
 * The bit-level definition:
 *   - filter sum, per band: z = sum of h[q U + p] x[m - q] over the q >= 0 with q U + p < T, in ascending q, accumulators starting at
 *     +0; per tap zr += h xr, then zi += h xi; every step is one fmaf in f32 and a multiply then an add, each rounded, in f64 (the
 *     resampler's rule).  A phase without taps (T <= p) has z = (+0, +0); no phase is padded with zero taps.
 *   - oscillator: j = (phase0 + fcw n) mod 2^32 in unsigned integers, w = conj(C[j >> 16] (x) F[j & 0xffff]) with C, F and (x) exactly
 *     the DDC's: the tables of sdsp_hip_ddc_oscillator rounded once to the plan precision; two products and one sum or difference,
 *     each rounded on its own, never contracted.  The conjugate is the sign flip of the imaginary part, which is exact: a DUC and a
 *     DDC with the same words turn by exactly conjugate values.
 *   - band value y = z (x) w.
 *   - sum: for each output element the channel's bands are taken in ascending band index; COMPLEX: acc_r += y.re and acc_i += y.im
 *     from +0, one rounded add each; REAL: only y.re = zr wr - zi wi is formed and summed.  A channel that no band names is written
 *     as +0 over all S U outputs.
 *   - history: H = floor((T - 1) / U) complex elements per BAND, state[i H + j] = x_i[-1 - j] (newest first); read at entry, written
 *     at exit; NULL = zero history, final history dropped.
 *   - block-by-block calls equal one long call bit for bit for any split into blocks when the caller advances `position` (blocks of 0
 *     samples and blocks shorter than H included); position and position + 2^32 give the same bits.
 *   - output kinds: COMPLEX = interleaved I/Q; REAL = the real part only.  The input is always interleaved complex of the plan
 *     precision (one complex sample is one element, as in the PFB and DDC banks).
 *   - strides count elements.  `in` is never written; nothing past each channel's S U outputs is.
 * Limits: 1 <= T <= SDSP_HIP_FIR_MAX_TAPS, 1 <= U <= SDSP_HIP_RESAMPLE_MAX_FACTOR, 1 <= nb <= 65536, channels >= 1, any number of
 * bands per channel.  The bands, the taps and U are fixed at plan creation.  sdsp_hip_resample_design(T, U, 1, h) is the matching
 * anti-imaging low-pass (gain U) for U >= 2.
 */
#define SDSP_HIP_DUC_REAL 0
#define SDSP_HIP_DUC_COMPLEX 1
#define SDSP_HIP_DUC_MAX_BANDS 65536
typedef struct sdsp_hip_duc_plan sdsp_hip_duc_plan;
typedef struct {
    uint32_t dst;    /* output channel */
    uint32_t fcw;    /* frequency, cycles per OUTPUT sample in units of 2^-32 */
    uint32_t phase0; /* phase at output stream index 0, cycles in units of 2^-32 */
} sdsp_hip_duc_band;
/* outputs per channel of one call of `samples` per band (S U), host only.  up out of range, or S U >= 2^62: SDSP_HIP_ERR_INVALID_SIZE;
 * out NULL: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_duc_out_samples(uint32_t up, uint64_t samples, uint64_t *out);
/* h: taps host doubles; bands: nb entries.  The plan rounds h and the tables of sdsp_hip_ddc_oscillator to its precision.  Errors:
 * taps, up, channels = 0, nb = 0 or nb > SDSP_HIP_DUC_MAX_BANDS: SDSP_HIP_ERR_INVALID_SIZE; a null pointer, a band with dst >=
 * channels, an unknown output kind, a precision other than F32 / F64: SDSP_HIP_ERR_INVALID_ARG; no device: SDSP_HIP_ERR_NO_DEVICE. */
int sdsp_hip_duc_plan_create(sdsp_hip_duc_plan **plan, uint32_t taps, const double *h, uint32_t up, uint32_t channels, uint32_t nb,
                             const sdsp_hip_duc_band *bands, int output_kind, int precision, int device);
int sdsp_hip_duc_plan_destroy(sdsp_hip_duc_plan *plan);
/*
 * in: DEVICE pointer, band i = in[i in_stride .. + samples) complex elements.  out: DEVICE pointer, channel c = out[c out_stride ..
 * + S U) elements of the output kind.  state: DEVICE pointer or NULL.  Asynchronous on `stream`, allocates nothing
 * (stream-capturable); one call per plan in flight.  Errors: null plan, in or out, in_stride < samples with more than one band,
 * out_stride < S U with more than one channel, overlapping in and out ranges, misaligned pointers: SDSP_HIP_ERR_INVALID_ARG; a grid
 * that does not fit one launch: SDSP_HIP_ERR_UNSUPPORTED.  samples == 0: nothing to do.
 */
int sdsp_hip_duc_process(sdsp_hip_duc_plan *plan, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t samples,
                         uint64_t position, void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_duc_process_host(sdsp_hip_duc_plan *plan, const void *host_in, uint64_t in_stride, void *host_out, uint64_t out_stride,
                              uint64_t samples, uint64_t position, void *host_state);
/* bytes of the plan's state buffer: H nb complex elements (0 when T <= U) */
int sdsp_hip_duc_state_bytes(const sdsp_hip_duc_plan *plan, uint64_t *bytes);
/* kernel variants (identical values, bit for bit): 0 = sdsp_duc_kernel, the fused form (h and each band's block staged in LDS, the
 * sums over all of a channel's bands kept in registers, every output written once); 1 = sdsp_duc_plain_kernel, one output per
 * thread from global memory (the cross-check). */
int sdsp_hip_duc_plan_set_variant(sdsp_hip_duc_plan *plan, int variant);
/* kernel launches of one process call of `samples` per band with a state buffer: the band kernel, and one for the new history
 * when H > 0; 0 for samples == 0 */
int sdsp_hip_duc_plan_launches(const sdsp_hip_duc_plan *plan, uint64_t samples, uint64_t *launches);
typedef struct {
    uint32_t taps, up, channels, bands;
    uint32_t hist;     /* H = floor((taps - 1) / up) */
    uint32_t block_in; /* input positions per band one workgroup of sdsp_duc_kernel turns into block_in up outputs of its channel */
    int output_kind, precision, device;
    char kernel[64];   /* the kernel the plan's variant runs */
} sdsp_hip_duc_plan_info;
int sdsp_hip_duc_plan_get_info(const sdsp_hip_duc_plan *plan, sdsp_hip_duc_plan_info *info);

/* ------------------------------------------------------------------ arbitrary-ratio polyphase resampler banks */

/*
 * Arbitrary-ratio polyphase resampler bank: every channel is resampled by any ratio in [1 / 1024, 1024],
 * which may change from call to call, through a prototype low-pass h of L T taps split into L phases of T taps (L a power of two,
 * phase p, tap k = h[k L + p]: the upfirdn layout), taking the nearest phase or interpolating linearly between two.  The channel
 * count is given per call, as in sdsp_hip_resample_process.
 * Time is unsigned Q32.32 in units of input samples.  `step` is input samples per output sample, 2^22 <= step <= max_step <= 2^42;
 * `time` is the instant of the call's first output relative to the call's first input sample, any value < 2^63.  A call takes
 * S < 2^31 samples per channel.  Output m of the call sits at t = time + m step, i = t >> 32, f = t & 0xffffffff, and the call
 * produces every m with i < S: n_out = 0 if time >= S 2^32, else ceil((S 2^32 - time) / step); the next call's time is
 * time + n_out step - S 2^32 (sdsp_hip_arb_out_samples).  All of it is exact integer arithmetic, so any split of a stream into
 * calls gives the same samples bit for bit (empty calls, calls shorter than the history and calls without an output included).
 * Value, the bit-level definition: lb = log2 L, p = f >> (32 - lb) (0 for L = 1), r = f & (2^(32 - lb) - 1),
 *   - mu = fl(r) 2^-(32 - lb), fl the unsigned-to-float conversion of the plan precision, round to nearest even (exact in f64).
 *   - tables, host, double, rounded once to the plan precision (sdsp_hip_arb_tables): H[p][k] = h[k L + p],
 *     Dt[p][k] = hext[k L + p + 1] - h[k L + p] with hext = h followed by zeros (the row after phase L - 1 is phase 0 one tap later).
 *   - with x = the history followed by the block: a = H[p][0] x[i], a plain multiply; then for k = 1 .. T - 1
 *     a = fmaf(H[p][k], x[i - k], a) in f32, a multiply then an add, each rounded, in f64 (the resampler's rule).  b: the same over Dt.
 *   - NEAREST: y = a.  LINEAR: y = fmaf(mu, b, a) in f32, a + mu b with two roundings in f64.
 *   - COMPLEX input (interleaved I/Q, one pair is one element, real taps): the two planes independently by the same steps.
 *   - history: H = T - 1 elements of the input kind per channel, state[c H + j] = x_c[-1 - j] (newest first); read at entry, written
 *     at exit (also when n_out = 0); NULL = zero history, final history dropped.
 *   - strides count elements.  `in` is never written; nothing past each row's n_out outputs is.
 */
#define SDSP_HIP_ARB_REAL 0
#define SDSP_HIP_ARB_COMPLEX 1
#define SDSP_HIP_ARB_NEAREST 0
#define SDSP_HIP_ARB_LINEAR 1
#define SDSP_HIP_ARB_MAX_PHASES 1024
#define SDSP_HIP_ARB_MIN_STEP (1ull << 22)
#define SDSP_HIP_ARB_MAX_STEP (1ull << 42)
typedef struct sdsp_hip_arb_plan sdsp_hip_arb_plan;
/* round(in_per_out 2^32), ties to even, for in_per_out in [1 / 1024, 1024], host only; anything else (NaN included) or step NULL:
 * SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_arb_step(double in_per_out, uint64_t *step);
/* n_out and the next call's time of one call, host only (next_time may be NULL).  step outside [2^22, 2^42], time >= 2^63,
 * samples >= 2^31 or n_out >= 2^31: SDSP_HIP_ERR_INVALID_SIZE; n_out NULL: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_arb_out_samples(uint64_t step, uint64_t time, uint64_t samples, uint64_t *n_out, uint64_t *next_time);
/* the matching prototype, host only: a Hamming-windowed sinc of phases * taps taps with cutoff min(1, 1 / max_in_per_out) / phases
 * of the L-times rate's Nyquist and gain phases, which is phases * scipy.signal.firwin(phases * taps, cutoff).  phases = 1 with a
 * ratio <= 1 has no band to protect: SDSP_HIP_ERR_INVALID_ARG; sizes out of range: SDSP_HIP_ERR_INVALID_SIZE. */
int sdsp_hip_arb_design(uint32_t phases, uint32_t taps, double max_in_per_out, double *h);
/* the two tables before rounding, host only: table_h[p taps + k] = H[p][k], table_d[p taps + k] = Dt[p][k] */
int sdsp_hip_arb_tables(uint32_t phases, uint32_t taps, const double *h, double *table_h, double *table_d);
/* h: phases * taps host doubles.  Errors: phases not a power of two in [1, SDSP_HIP_ARB_MAX_PHASES], taps = 0, phases * taps >
 * SDSP_HIP_FIR_MAX_TAPS, max_step outside [2^22, 2^42]: SDSP_HIP_ERR_INVALID_SIZE; a null pointer, an unknown input kind or
 * interpolation mode, a precision other than F32 / F64: SDSP_HIP_ERR_INVALID_ARG; no device: SDSP_HIP_ERR_NO_DEVICE. */
int sdsp_hip_arb_plan_create(sdsp_hip_arb_plan **plan, uint32_t phases, uint32_t taps, const double *h, uint64_t max_step,
                             int input_kind, int interp, int precision, int device);
int sdsp_hip_arb_plan_destroy(sdsp_hip_arb_plan *plan);
/*
 * in: DEVICE pointer, channel c = in[c in_stride .. + samples) elements of the input kind.  out: DEVICE pointer, channel c =
 * out[c out_stride .. + n_out) elements of the same kind.  state: DEVICE pointer or NULL.  Asynchronous on `stream`, allocates nothing
 * (stream-capturable); one call per plan in flight.  Errors: step outside [2^22, max_step], time >= 2^63, samples >= 2^31, n_out >=
 * 2^31: SDSP_HIP_ERR_INVALID_SIZE; null plan, in or out, in_stride < samples or out_stride < n_out with more than one channel,
 * overlapping in and out ranges, misaligned pointers: SDSP_HIP_ERR_INVALID_ARG; a grid that does not fit one launch:
 * SDSP_HIP_ERR_UNSUPPORTED.  channels == 0 or samples == 0: nothing to do.
 */
int sdsp_hip_arb_process(sdsp_hip_arb_plan *plan, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t channels,
                         uint64_t samples, uint64_t step, uint64_t time, void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_arb_process_host(sdsp_hip_arb_plan *plan, const void *host_in, uint64_t in_stride, void *host_out, uint64_t out_stride,
                              uint64_t channels, uint64_t samples, uint64_t step, uint64_t time, void *host_state);
/* bytes of a state buffer for `channels` channels: H channels element size (0 when T = 1) */
int sdsp_hip_arb_state_bytes(const sdsp_hip_arb_plan *plan, uint64_t channels, uint64_t *bytes);
/* kernel variants (identical values, bit for bit): 0 = sdsp_arb_kernel, the fused form (the tap tables and each block's input span
 * staged in LDS); 1 = sdsp_arb_plain_kernel, one output per thread from global memory (the cross-check). */
int sdsp_hip_arb_plan_set_variant(sdsp_hip_arb_plan *plan, int variant);
/* kernel launches of one process call with a state buffer: the resampling kernel when n_out > 0, and one for the new history when
 * T > 1; 0 for samples == 0 */
int sdsp_hip_arb_plan_launches(const sdsp_hip_arb_plan *plan, uint64_t step, uint64_t time, uint64_t samples, uint64_t *launches);
typedef struct {
    uint32_t phases, taps; /* L, T */
    uint32_t hist;         /* H = taps - 1 */
    uint32_t block_out;    /* outputs one workgroup of sdsp_arb_kernel produces from one staged input span */
    uint64_t max_step;
    int input_kind, interp, precision, device;
    char kernel[64];       /* the kernel the plan's variant runs */
} sdsp_hip_arb_plan_info;
int sdsp_hip_arb_plan_get_info(const sdsp_hip_arb_plan *plan, sdsp_hip_arb_plan_info *info);

/* ------------------------------------------------------------------ CIC decimator banks for integer sample streams */

/*
 * Cascaded integrator-comb (Hogenauer) decimator bank: every channel, a stream of 16- or 32-bit integer
 * samples, real or interleaved I/Q, goes through N integrators at the input rate, keeps every R-th sample, and through N combs of
 * differential delay M at the output rate.  No multiplies, no coefficients, exact in modular integer arithmetic: the contract is
 * bit-exact for every input.  The channel count is given per call, as in sdsp_hip_arb_process.
 * Parameters: order 1 <= N <= 8, decimation 2 <= R <= 16384, delay M in {1, 2}, hist = N M R <= SDSP_HIP_CIC_MAX_HISTORY.
 * in_bits is the number of significant bits of a sample, 2 .. 16 for I16 and 2 .. 32 for I32; growth = bit_length((R M)^N - 1) in
 * exact integers (sdsp_hip_cic_growth).  The register width is W = 32 if in_bits + growth <= 32, else 64; in_bits + growth > 64 is
 * SDSP_HIP_ERR_UNSUPPORTED.
 * `position` is the number of samples earlier calls consumed.  A call takes any S < 2^31 samples per channel, not only multiples
 * of R, and writes n_out = floor((position + S) / R) - floor(position / R) outputs per channel (sdsp_hip_cic_out_samples): one at
 * each stream index n with n mod R == R - 1.
 * Value, the bit-level definition: all registers are W-bit two's complement and wrap, and are zero at the start of the stream.
 *   - for each input sample (sign-extended to W bits), in cascade order, integrator s adds the value in front of it to its register
 *     and passes the sum on.
 *   - at a due index, comb s outputs (its input - its input M outputs earlier), each difference wrapped.
 *   - the last comb's value, sign-extended, is y.  This holds for any input values, also ones wider than in_bits: the definition
 *     is modular.  It equals the FIR form, boxcar(R M) convolved N times (sdsp_hip_cic_taps) applied mod 2^W, so an output depends
 *     on the N (R M - 1) + 1 <= hist newest inputs only.
 *   - OUT_INT writes y as int32 when W = 32 and as int64 when W = 64.  OUT_F32 writes (float)((double)y * scale), each conversion
 *     and the product rounded to nearest even; `scale` is the plan's, and 1 / (double)(R M)^N (sdsp_hip_cic_unity_scale) gives
 *     unity gain at DC.
 *   - COMPLEX input (interleaved I/Q, one pair is one element): the two planes independently by the same steps; the outputs are
 *     interleaved pairs likewise.
 *   - history: hist elements of the input kind and type per channel, state[c hist + j] = x_c[-1 - j] (newest first); read at
 *     entry, written at exit (also when n_out = 0); NULL = zero history, final history dropped.
 *   - any split of a stream into calls gives the same bits when the caller advances `position` (empty calls, calls shorter than
 *     hist and calls without an output included); `position` and `position + k R` give the same bits.
 *   - strides count elements.  `in` is never written; nothing past each row's n_out outputs is.  Pointers need only element
 *     alignment (2 bytes for I16 real).
 */
#define SDSP_HIP_CIC_REAL 0
#define SDSP_HIP_CIC_COMPLEX 1
#define SDSP_HIP_CIC_I16 0
#define SDSP_HIP_CIC_I32 1
#define SDSP_HIP_CIC_OUT_INT 0
#define SDSP_HIP_CIC_OUT_F32 1
#define SDSP_HIP_CIC_MAX_ORDER 8
#define SDSP_HIP_CIC_MAX_DOWN 16384
#define SDSP_HIP_CIC_MAX_HISTORY 65536
typedef struct sdsp_hip_cic_plan sdsp_hip_cic_plan;
/* The four helpers below are host only and need no device.  order outside [1, 8], down outside [2, 16384], delay outside {1, 2} or
 * order * delay * down > SDSP_HIP_CIC_MAX_HISTORY: SDSP_HIP_ERR_INVALID_SIZE; a null output pointer: SDSP_HIP_ERR_INVALID_ARG. */
/* bits = bit_length((down * delay)^order - 1), up to 104 */
int sdsp_hip_cic_growth(uint32_t order, uint32_t down, uint32_t delay, uint32_t *bits);
/* n_out of one call; position may be any 64-bit value.  down outside [2, 16384] or samples >= 2^31: SDSP_HIP_ERR_INVALID_SIZE */
int sdsp_hip_cic_out_samples(uint32_t down, uint64_t position, uint64_t samples, uint64_t *n_out);
/* scale = 1.0 / (double)(down * delay)^order, the integer converted with one rounding */
int sdsp_hip_cic_unity_scale(uint32_t order, uint32_t down, uint32_t delay, double *scale);
/* h: the order * (down * delay - 1) + 1 coefficients of boxcar(down * delay) convolved `order` times, each reduced mod 2^64 */
int sdsp_hip_cic_taps(uint32_t order, uint32_t down, uint32_t delay, uint64_t *h);
/* Errors: the sizes above: SDSP_HIP_ERR_INVALID_SIZE; in_bits outside 2 .. 16 (I16) or 2 .. 32 (I32): SDSP_HIP_ERR_INVALID_SIZE; a
 * null pointer, an unknown input type, input kind or output kind, a scale that is not finite: SDSP_HIP_ERR_INVALID_ARG; in_bits +
 * growth > 64: SDSP_HIP_ERR_UNSUPPORTED, the message names in_bits, growth and their sum; no device: SDSP_HIP_ERR_NO_DEVICE.
 * `scale` is used by OUT_F32 only. */
int sdsp_hip_cic_plan_create(sdsp_hip_cic_plan **plan, uint32_t order, uint32_t down, uint32_t delay, int in_type, uint32_t in_bits,
                             int input_kind, int out_kind, double scale, int device);
int sdsp_hip_cic_plan_destroy(sdsp_hip_cic_plan *plan);
/*
 * in: DEVICE pointer, channel c = in[c in_stride .. + samples) elements of the input kind and type.  out: DEVICE pointer, channel
 * c = out[c out_stride .. + n_out) elements of the output kind (real or pairs of int32 / int64 / float).  state: DEVICE pointer
 * or NULL.  Asynchronous on `stream`, allocates nothing (stream-capturable); one call per plan in flight.  Errors: samples >= 2^31:
 * SDSP_HIP_ERR_INVALID_SIZE; null plan, in or out, in_stride < samples or out_stride < n_out with more than one channel,
 * overlapping in and out ranges, misaligned pointers: SDSP_HIP_ERR_INVALID_ARG; a grid that does not fit one launch:
 * SDSP_HIP_ERR_UNSUPPORTED.  channels == 0 or samples == 0: nothing to do.
 */
int sdsp_hip_cic_process(sdsp_hip_cic_plan *plan, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t channels,
                         uint64_t samples, uint64_t position, void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_cic_process_host(sdsp_hip_cic_plan *plan, const void *host_in, uint64_t in_stride, void *host_out, uint64_t out_stride,
                              uint64_t channels, uint64_t samples, uint64_t position, void *host_state);
/* bytes of a state buffer for `channels` channels: hist * channels * the input element size */
int sdsp_hip_cic_state_bytes(const sdsp_hip_cic_plan *plan, uint64_t channels, uint64_t *bytes);
/* kernel variants (identical values, bit for bit): 0 = sdsp_cic_kernel, the fused form (integrators as workgroup scans chunk by
 * chunk, combs in LDS); 1 = sdsp_cic_plain_kernel, one output per thread as the direct sum of h[k] x[n - k] mod 2^W over global
 * memory (the cross-check; it shares no logic with the scan). */
int sdsp_hip_cic_plan_set_variant(sdsp_hip_cic_plan *plan, int variant);
/* chunks of input per workgroup of the fused kernel: 0 = automatic, else exactly `chunks` (< 2^20).  The
 * bits do not depend on it. */
int sdsp_hip_cic_plan_set_segment(sdsp_hip_cic_plan *plan, uint32_t chunks);
/* kernel launches of one process call with a state buffer: the decimating kernel when n_out > 0, and one for the new history;
 * 0 for samples == 0 */
int sdsp_hip_cic_plan_launches(const sdsp_hip_cic_plan *plan, uint64_t position, uint64_t samples, uint64_t *launches);
typedef struct {
    uint32_t order, down, delay; /* N, R, M */
    uint32_t hist;               /* N M R */
    uint32_t in_bits, growth;    /* growth = bit_length((R M)^N - 1) */
    uint32_t reg_bits;           /* W: 32 or 64 */
    uint32_t chunk;              /* input elements one workgroup of sdsp_cic_kernel scans per pass */
    uint32_t segment;            /* sdsp_hip_cic_plan_set_segment's value, 0 = automatic */
    int in_type, input_kind, out_kind, device;
    double scale;
    char kernel[64];             /* the kernel the plan's variant runs */
} sdsp_hip_cic_plan_info;
int sdsp_hip_cic_plan_get_info(const sdsp_hip_cic_plan *plan, sdsp_hip_cic_plan_info *info);

/* ------------------------------------------------------------------ CIC interpolator banks for integer sample streams */

/*
 * Cascaded integrator-comb (Hogenauer) interpolator bank, the transmit-side mirror of the decimator above:
 * every channel, a stream of 16- or 32-bit integer samples, real or interleaved I/Q, goes through N combs of differential delay M
 * at the input rate, is zero-stuffed by R, and goes through N integrators at the output rate.  No multiplies, no coefficients,
 * exact in modular integer arithmetic: the contract is bit-exact for every input.  Kinds, types and output kinds are the
 * decimator's SDSP_HIP_CIC_* constants; the channel count is given per call.
 * Parameters: order 1 <= N <= 8, up-sampling 2 <= R <= 16384, delay M in {1, 2}, N M R <= SDSP_HIP_CIC_MAX_HISTORY.
 * in_bits is the number of significant bits of a sample, 2 .. 16 for I16 and 2 .. 32 for I32; growth = bit_length(R^(N-1) M^N - 1)
 * in exact integers (sdsp_hip_cic_interp_growth).  The register width is W = 32 if in_bits + growth <= 32, else 64; in_bits +
 * growth > 64 is SDSP_HIP_ERR_UNSUPPORTED.
 * A call takes S samples per channel and writes exactly R S outputs per channel, R S < 2^31.  There is no stream position: the
 * filter is time-invariant at the input rate, and every call starts on an input boundary.
 * Value, the bit-level definition: all registers are W-bit two's complement and wrap, and are zero at the start of the stream.
 *   - combs at the input rate: c_0 = x (sign-extended to W bits), c_k[m] = c_{k-1}[m] - c_{k-1}[m - M], k = 1 .. N.
 *   - zero-stuffing: u[m R] = c_N[m], u[n] = 0 otherwise.
 *   - integrators at the output rate: I_0 = u, I_k[n] = I_k[n - 1] + I_{k-1}[n] (inclusive), k = 1 .. N; y = I_N, sign-extended.
 *     This holds for any input values, also ones wider than in_bits: the definition is modular.  It equals the polyphase FIR form
 *     y[m R + p] = sum_j h[p + j R] x[m - j] mod 2^W with h = boxcar(R M) convolved N times (sdsp_hip_cic_taps), so an output
 *     depends on the N M newest inputs only.  Every branch p sums to R^(N-1) M^N, the gain at DC.
 *   - OUT_INT writes y as int32 when W = 32 and as int64 when W = 64.  OUT_F32 writes (float)((double)y * scale), each conversion
 *     and the product rounded to nearest even; `scale` is the plan's, and sdsp_hip_cic_interp_unity_scale gives unity gain at DC.
 *   - COMPLEX input (interleaved I/Q, one pair is one element): the two planes independently by the same steps; the outputs are
 *     interleaved pairs likewise.
 *   - history: N M elements of the input kind and type per channel, state[c N M + j] = x_c[-1 - j] (newest first); read at entry,
 *     written at exit (also by calls shorter than N M); NULL = zero history, final history dropped.
 *   - any split of a stream into calls gives the same bits (empty and one-sample calls included).
 *   - strides count elements.  `in` is never written; nothing past each row's R S outputs is.  Pointers need only element
 *     alignment (2 bytes for I16 real).
 */
typedef struct sdsp_hip_cic_interp_plan sdsp_hip_cic_interp_plan;
/* The two helpers below are host only and need no device.  order outside [1, 8], up outside [2, 16384], delay outside {1, 2} or
 * order * delay * up > SDSP_HIP_CIC_MAX_HISTORY: SDSP_HIP_ERR_INVALID_SIZE; a null output pointer: SDSP_HIP_ERR_INVALID_ARG. */
/* bits = bit_length(up^(order-1) * delay^order - 1), up to 92 */
int sdsp_hip_cic_interp_growth(uint32_t order, uint32_t up, uint32_t delay, uint32_t *bits);
/* scale = 1.0 / (double)(up^(order-1) * delay^order), the integer converted with one rounding */
int sdsp_hip_cic_interp_unity_scale(uint32_t order, uint32_t up, uint32_t delay, double *scale);
/* Errors: as sdsp_hip_cic_plan_create, with `up` in the place of `down` and the interpolator's growth. */
int sdsp_hip_cic_interp_plan_create(sdsp_hip_cic_interp_plan **plan, uint32_t order, uint32_t up, uint32_t delay, int in_type,
                                    uint32_t in_bits, int input_kind, int out_kind, double scale, int device);
int sdsp_hip_cic_interp_plan_destroy(sdsp_hip_cic_interp_plan *plan);
/*
 * in: DEVICE pointer, channel c = in[c in_stride .. + samples) elements of the input kind and type.  out: DEVICE pointer, channel
 * c = out[c out_stride .. + up * samples) elements of the output kind (real or pairs of int32 / int64 / float).  state: DEVICE
 * pointer or NULL.  Asynchronous on `stream`, allocates nothing (stream-capturable); one call per plan in flight.  Errors:
 * up * samples >= 2^31: SDSP_HIP_ERR_INVALID_SIZE; null plan, in or out, in_stride < samples or out_stride < up * samples with more
 * than one channel, overlapping in and out ranges, misaligned pointers: SDSP_HIP_ERR_INVALID_ARG; a grid that does not fit one
 * launch: SDSP_HIP_ERR_UNSUPPORTED.  channels == 0 or samples == 0: nothing to do.
 */
int sdsp_hip_cic_interp_process(sdsp_hip_cic_interp_plan *plan, const void *in, uint64_t in_stride, void *out, uint64_t out_stride,
                                uint64_t channels, uint64_t samples, void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_cic_interp_process_host(sdsp_hip_cic_interp_plan *plan, const void *host_in, uint64_t in_stride, void *host_out,
                                     uint64_t out_stride, uint64_t channels, uint64_t samples, void *host_state);
/* bytes of a state buffer for `channels` channels: order * delay * channels * the input element size */
int sdsp_hip_cic_interp_state_bytes(const sdsp_hip_cic_interp_plan *plan, uint64_t channels, uint64_t *bytes);
/* kernel variants (identical values, bit for bit): 0 = sdsp_cic_interp_kernel, the time-parallel form (the first integrator as a
 * hold of comb sums, the others as workgroup scans chunk by chunk); 1 = sdsp_cic_interp_plain_kernel, one output per thread as the
 * direct polyphase sum of h[p + j R] x[m - j] mod 2^W over global memory (the cross-check; it shares no logic with the scan). */
int sdsp_hip_cic_interp_plan_set_variant(sdsp_hip_cic_interp_plan *plan, int variant);
/* chunks of output per workgroup of the scan kernel: 0 = automatic, else exactly `chunks` (< 2^20).  The
 * bits do not depend on it. */
int sdsp_hip_cic_interp_plan_set_segment(sdsp_hip_cic_interp_plan *plan, uint32_t chunks);
/* kernel launches of one process call with a state buffer: the interpolating kernel and one for the new history; 0 for
 * samples == 0.  up * samples >= 2^31: SDSP_HIP_ERR_INVALID_SIZE */
int sdsp_hip_cic_interp_plan_launches(const sdsp_hip_cic_interp_plan *plan, uint64_t samples, uint64_t *launches);
typedef struct {
    uint32_t order, up, delay;   /* N, R, M */
    uint32_t hist;               /* N M */
    uint32_t in_bits, growth;    /* growth = bit_length(R^(N-1) M^N - 1) */
    uint32_t reg_bits;           /* W: 32 or 64 */
    uint32_t chunk;              /* output elements one workgroup of sdsp_cic_interp_kernel scans per pass */
    uint32_t segment;            /* sdsp_hip_cic_interp_plan_set_segment's value, 0 = automatic */
    int in_type, input_kind, out_kind, device;
    double scale;
    char kernel[64];             /* the kernel the plan's variant runs */
} sdsp_hip_cic_interp_plan_info;
int sdsp_hip_cic_interp_plan_get_info(const sdsp_hip_cic_interp_plan *plan, sdsp_hip_cic_interp_plan_info *info);

/* ------------------------------------------------------------------ time-delay beamformer banks */

/*
 * Time-delay (filter-and-sum) beamformer bank: the streams of a sensor array are delayed, weighted and summed
 * into beams.  There are `groups` arrays of `sensors` = C input rows and `beams` = B output rows each: input row g C + c, output row
 * g B + b, channel-major, strides in elements.  All groups share the plan's entries.  An entry is {beam, sensor, delay} with its own T
 * taps g[0..T): the beam gets the sensor's stream delayed by `delay` whole samples and filtered with g (a fractional-delay filter, a
 * weight, or both; sdsp_hip_beam_delay_taps designs one).  A call takes S >= 0 samples per input row and writes S outputs per beam.
 * The bit-level definition, with x_c = the sensor's history followed by the call's block:
 *   - output n of beam b has one accumulator, starting at +0.  It runs over the beam's entries in the order given, and within an entry
 *     over ascending t:  acc = g[t] x_c[n - delay - t] + acc.  REAL: one fmaf per step in f32, a multiply then an add, each rounded, in
 *     f64.  COMPLEX (accumulators zr, zi): per step, in this order, zr += gr xr, zr -= gi xi, zi += gr xi, zi += gi xr, each of the four
 *     one fmaf in f32 and a multiply then an add (or subtraction) in f64 -- the DDC bank's filter step.  Nothing else is contracted.
 *   - taps: host doubles (interleaved re, im pairs for COMPLEX), [entry][t], rounded once to the plan precision.
 *   - entries are sorted by beam (beam numbers never decrease), and within a beam the sensor numbers strictly ascend: at most one entry
 *     per sensor and beam.  A beam may have no entry: its outputs are +0.  A sensor may be used by no beam: it is never read, but its
 *     history is still carried.
 *   - history: H = (max delay over all entries) + T - 1 elements of the input kind per INPUT ROW, state[(g C + c) H + j] = x[-1 - j]
 *     (newest first); read at entry, written at exit (a call of S = 0 leaves it as it is); NULL = zero history, final history
 *     dropped.  There is no stream position: the operation is time-invariant.
 *   - any split of a stream into calls (blocks shorter than H and empty blocks included) gives the same bits and the same final state.
 *   - kinds: REAL = real rows, real taps, real beams; COMPLEX = interleaved I/Q rows, complex taps, complex beams (one complex sample is
 *     one element); with T = 1 this is the narrowband phase-shift beamformer behind a DDC bank.
 *   - `in` is never written; nothing past each beam's S outputs is.
 * Limits: 1 <= T <= SDSP_HIP_BEAM_MAX_TAPS, 0 <= delay <= SDSP_HIP_BEAM_MAX_DELAY, 1 <= C, B <= SDSP_HIP_BEAM_MAX_ROWS,
 * 0 <= n_entries <= SDSP_HIP_BEAM_MAX_ENTRIES, groups >= 1 with groups C and groups B below 2^31.  Entries and taps are fixed at plan
 * creation.
 */
#define SDSP_HIP_BEAM_REAL 0
#define SDSP_HIP_BEAM_COMPLEX 1
#define SDSP_HIP_BEAM_MAX_TAPS 256
#define SDSP_HIP_BEAM_MAX_DELAY 65535
#define SDSP_HIP_BEAM_MAX_ROWS 4096
#define SDSP_HIP_BEAM_MAX_ENTRIES (1u << 20)
typedef struct sdsp_hip_beam_plan sdsp_hip_beam_plan;
typedef struct {
    uint32_t beam;   /* output row within a group */
    uint32_t sensor; /* input row within a group */
    uint32_t delay;  /* whole samples */
} sdsp_hip_beam_entry;
/* fractional-delay taps for one entry, host only, in double: a Kaiser-windowed sinc.  T >= 2: d = floor(tau), mu = tau - d,
 * c0 = (T - 1) div 2, u_t = t - c0 - mu, g[t] proportional to sinc(u_t) I0(beta sqrt(max(0, 1 - (u_t / ((T + 1) / 2))^2))) / I0(beta)
 * (sinc(u) = sin(pi u) / (pi u)), scaled so that sum g = weight; *delay = d.  An entry with these taps delays by tau + c0 samples: c0 is
 * the latency every entry of the plan shares.  T = 1: *delay = floor(tau + 1/2), g[0] = weight.  Errors: taps out of range:
 * SDSP_HIP_ERR_INVALID_SIZE; tau < 0, tau >= SDSP_HIP_BEAM_MAX_DELAY, beta < 0, a non-finite argument, a null pointer:
 * SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_beam_delay_taps(double tau, double weight, uint32_t taps, double beta, uint32_t *delay, double *g);
/* entries: n_entries entries in the contract's order; g: n_entries x taps host doubles (x 2 for COMPLEX).  Errors: sensors, beams,
 * groups, taps, n_entries or a delay out of range: SDSP_HIP_ERR_INVALID_SIZE; a null pointer, an entry naming a beam or sensor the plan
 * does not have, entries out of order or a (beam, sensor) pair given twice, an unknown kind, a precision other than F32 / F64:
 * SDSP_HIP_ERR_INVALID_ARG; no device: SDSP_HIP_ERR_NO_DEVICE. */
int sdsp_hip_beam_plan_create(sdsp_hip_beam_plan **plan, uint32_t sensors, uint32_t beams, uint32_t groups, uint32_t taps,
                              uint32_t n_entries, const sdsp_hip_beam_entry *entries, const double *g, int kind, int precision,
                              int device);
int sdsp_hip_beam_plan_destroy(sdsp_hip_beam_plan *plan);
/*
 * in: DEVICE pointer, input row r = in[r in_stride .. + samples) elements of the kind.  out: DEVICE pointer, output row r = out[r
 * out_stride .. + samples).  state: DEVICE pointer or NULL.  Asynchronous on `stream`, allocates nothing (stream-capturable); one call
 * per plan in flight.  Errors: null plan, in or out, a stride < samples with more than one row, overlapping in and out ranges,
 * misaligned pointers: SDSP_HIP_ERR_INVALID_ARG; samples >= 2^31: SDSP_HIP_ERR_INVALID_SIZE; a grid that does not fit one launch:
 * SDSP_HIP_ERR_UNSUPPORTED.  samples == 0: nothing to do.
 */
int sdsp_hip_beam_process(sdsp_hip_beam_plan *plan, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t samples,
                          void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_beam_process_host(sdsp_hip_beam_plan *plan, const void *host_in, uint64_t in_stride, void *host_out, uint64_t out_stride,
                               uint64_t samples, void *host_state);
/* bytes of the plan's state buffer: H groups C element size (0 when H = 0) */
int sdsp_hip_beam_state_bytes(const sdsp_hip_beam_plan *plan, uint64_t *bytes);
/* kernel variants (identical values, bit for bit): 0 = sdsp_beam_kernel, the fused form (a workgroup stages each sensor's window in LDS
 * once for a chunk of beams, a lane slides a register window over the taps for four consecutive outputs); 1 =
 * sdsp_beam_plain_kernel, one output per thread from global memory (the cross-check; it shares no staging logic with the fused form). */
int sdsp_hip_beam_plan_set_variant(sdsp_hip_beam_plan *plan, int variant);
/* kernel launches of one process call with a state buffer: the beam kernel, and one for the new history when H > 0; 0 for
 * samples == 0 */
int sdsp_hip_beam_plan_launches(const sdsp_hip_beam_plan *plan, uint64_t samples, uint64_t *launches);
typedef struct {
    uint32_t sensors, beams, groups, taps, entries;
    uint32_t max_delay;      /* over all entries */
    uint32_t hist;           /* H = max_delay + taps - 1 */
    uint32_t block_out;      /* outputs per beam one workgroup of sdsp_beam_kernel produces */
    uint32_t chunks;         /* chunks of consecutive beams that share staged sensor windows (the beam chunk table) */
    uint32_t max_spread;     /* the widest delay spread (max - min over a chunk's beams on one sensor) a chunk may have */
    uint32_t lds_line_bytes; /* one of the two LDS lines of sdsp_beam_kernel: the plan's widest sensor window, padded */
    int kind, precision, device, variant;
    char kernel[64];         /* the kernel the plan's variant runs */
} sdsp_hip_beam_plan_info;
int sdsp_hip_beam_plan_get_info(const sdsp_hip_beam_plan *plan, sdsp_hip_beam_plan_info *info);

/* ------------------------------------------------------------------ LMS / NLMS adaptive filter banks */

/*
 * LMS / NLMS adaptive filter bank: `channels` independent adaptive FIR filters of T taps each, whose weights
 * move with every sample.  A call takes S >= 0 samples per channel of two input rows, the reference input x and the desired signal d
 * (channel-major: row c = ptr[c stride .. + S) elements of the kind, strides in elements), and writes up to two output rows, the
 * filter output y and the error e.  The step size mu is an argument of the call.  The bit-level definition, with x_c = the channel's
 * history followed by the call's block and w = the channel's T weights, for n = 0 .. S - 1 in this order:
 *   1. y = +0, then for t = 0 .. T - 1 ascending  y = w[t] x_c[n - t] + y.  REAL: one fmaf per step in f32; a multiply then an add, each
 *      rounded, in f64.  COMPLEX (no conjugate: with mu = 0 the plan is a complex FIR filter): per tap, in this order,
 *      yr += wr xr, yr -= wi xi, yi += wr xi, yi += wi xr, each one fmaf in f32 (the subtraction: fmaf(-wi, xi, yr)) and a multiply then an
 *      add (or subtraction) in f64 -- the DDC bank's filter step.
 *   2. e = d[n] - y, one subtraction (per component).
 *   3. LMS: g = mu e, one rounded product (per component).
 *   4. NLMS: p = +0, then for t ascending  p = x_c[n - t] x_c[n - t] + p  with the rule of step 1 (COMPLEX: xr xr, then xi xi, per
 *      tap); then g = (mu e) / (eps + p): a rounded product, a rounded sum and a correctly rounded division (both components of a
 *      complex e divide by the same eps + p).  The energy is recomputed from the window for every sample, never carried.
 *   5. for t ascending  w[t] = g x_c[n - t] + w[t]  with the rule of step 1.  COMPLEX (w += g conj(x)): wr = gr xr + wr, wr = gi xi + wr,
 *      wi = gi xr + wi, wi = -(gr xi) + wi (f32: fmaf(-gr, xi, wi); f64: wi - gr xi), in this order.
 *   6. y[n] and e[n] are the values of steps 1 and 2: the a-priori output and error.
 * Nothing else is contracted.  mu and eps are host doubles, each rounded once to the plan precision (eps at plan creation).  mu = 0
 * filters with frozen weights (w[t] = (+-0) x + w[t] still runs: a weight of -0 becomes +0, a non-finite x reaches the weights).
 *   - state: one caller-owned device buffer of sdsp_hip_lms_state_bytes bytes.  First channels x T weights, state[c T + t] = w_c[t];
 *     then channels x (T - 1) elements of x history, newest first: state[channels T + c (T - 1) + j] = x_c[-1 - j].  Read at entry,
 *     written at exit.  A zero-filled buffer is a fresh stream with zero weights.  NULL = zero weights and zero history, nothing kept.
 *   - there is no stream position; any split of a stream into calls (empty calls included) gives the same bits and the same final
 *     state.  A call with S = 0 returns at once and leaves the state alone.
 *   - y or e or both may be NULL and are then not written.  Outputs may not overlap inputs or each other.  x and d are never
 *     written; nothing past each row's S outputs is.
 *   - kinds: REAL = real rows and weights; COMPLEX = interleaved I/Q rows and weights (one complex sample is one element).
 * Limits: 1 <= T <= SDSP_HIP_LMS_MAX_TAPS (SDSP_HIP_LMS_MAX_TAPS_F64_COMPLEX for F64 COMPLEX), 1 <= channels < 2^31, S < 2^31.
 */
#define SDSP_HIP_LMS_REAL 0
#define SDSP_HIP_LMS_COMPLEX 1
#define SDSP_HIP_LMS_LMS 0
#define SDSP_HIP_LMS_NLMS 1
#define SDSP_HIP_LMS_MAX_TAPS 64
#define SDSP_HIP_LMS_MAX_TAPS_F64_COMPLEX 32
typedef struct sdsp_hip_lms_plan sdsp_hip_lms_plan;
/* eps is used by NLMS only.  Errors: channels or taps out of range: SDSP_HIP_ERR_INVALID_SIZE; a null pointer, an unknown kind or mode,
 * a precision other than F32 / F64, for NLMS an eps that is not finite and > 0 once rounded to the precision:
 * SDSP_HIP_ERR_INVALID_ARG; no device: SDSP_HIP_ERR_NO_DEVICE. */
int sdsp_hip_lms_plan_create(sdsp_hip_lms_plan **plan, uint64_t channels, uint32_t taps, int kind, int precision, int mode, double eps,
                             int device);
int sdsp_hip_lms_plan_destroy(sdsp_hip_lms_plan *plan);
/*
 * x, d: DEVICE pointers; y, e: DEVICE pointers or NULL; state: DEVICE pointer or NULL.  Asynchronous on `stream`, allocates nothing
 * (stream-capturable); one call per plan in flight.  Errors: null plan, x or d, a stride < samples with more than one channel,
 * overlapping ranges, misaligned pointers, a mu that is not finite in the precision: SDSP_HIP_ERR_INVALID_ARG; samples >= 2^31:
 * SDSP_HIP_ERR_INVALID_SIZE; a grid that does not fit one launch: SDSP_HIP_ERR_UNSUPPORTED.  samples == 0: nothing to do.
 */
int sdsp_hip_lms_process(sdsp_hip_lms_plan *plan, const void *x, uint64_t x_stride, const void *d, uint64_t d_stride, void *y,
                         uint64_t y_stride, void *e, uint64_t e_stride, uint64_t samples, double mu, void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_lms_process_host(sdsp_hip_lms_plan *plan, const void *host_x, uint64_t x_stride, const void *host_d, uint64_t d_stride,
                              void *host_y, uint64_t y_stride, void *host_e, uint64_t e_stride, uint64_t samples, double mu,
                              void *host_state);
/* bytes of the plan's state buffer: channels (2 T - 1) element size */
int sdsp_hip_lms_state_bytes(const sdsp_hip_lms_plan *plan, uint64_t *bytes);
/* kernel variants (identical values, bit for bit): 0 = sdsp_lms_kernel (a lane per channel, the weights in registers for the whole call,
 * rows transposed through LDS, the update of one sample fused into the filtering of the next); 1 = sdsp_lms_plain_kernel, one thread
 * per channel from global memory with the weights read-modify-written in `state` (the cross-check; it shares no staging logic with
 * variant 0).  Selecting variant 1 allocates channels x T elements of plan-owned scratch once, for calls without a state buffer. */
int sdsp_hip_lms_plan_set_variant(sdsp_hip_lms_plan *plan, int variant);
/* kernel launches of one process call with a state buffer: the filter kernel, and one for the new history when T > 1; 0 for
 * samples == 0 */
int sdsp_hip_lms_plan_launches(const sdsp_hip_lms_plan *plan, uint64_t samples, uint64_t *launches);
typedef struct {
    uint64_t channels;
    uint32_t taps;
    uint32_t block;     /* samples per time block of sdsp_lms_kernel for this kind, precision and tap count */
    uint32_t lds_bytes; /* LDS of one workgroup (one wave, 64 channels) of sdsp_lms_kernel: (T + 2 block) rows of 65 elements */
    double eps;         /* as rounded to the precision; 0 for LMS */
    int kind, precision, mode, device, variant;
    char kernel[64];    /* the kernel the plan's variant runs */
} sdsp_hip_lms_plan_info;
int sdsp_hip_lms_plan_get_info(const sdsp_hip_lms_plan *plan, sdsp_hip_lms_plan_info *info);

/* ------------------------------------------------------------------ rank-order filter banks (running median, minimum, maximum) */

/*
 * Rank-order filter bank: `channels` independent real rows, F32 or F64 (channel-major: row c =
 * ptr[c stride .. + S) elements, strides in elements).  A plan fixes the window W and the rank r, 0 <= r < W.  A call takes S >= 0
 * samples per row, out of place.  With x_c = the row's history followed by the call's block,
 *     y[n] = the element of rank r, counted from 0 and ascending, of the W values x_c[n - W + 1 .. n]:
 * r = 0 is the running minimum, r = W - 1 the running maximum, r = (W - 1) / 2 with odd W the running median.
 *   - order: IEEE 754 totalOrder, defined through a key.  Take the value's bits as an unsigned integer u; the key is ~u if the sign
 *     bit is set, else u | signbit; keys compare as unsigned integers.  So -0 < +0, NaNs with the sign bit set sort below -inf, NaNs
 *     with it clear sort above +inf, ordered by payload.  Nothing is quieted or canonicalised: the output is bit for bit one of the
 *     W inputs.  Equal keys are identical bit patterns, so which copy is returned cannot matter.  No floating-point arithmetic
 *     happens anywhere.
 *   - state: one caller-owned device buffer of sdsp_hip_rank_state_bytes bytes: channels x (W - 1) elements of x history, newest
 *     first: state[c (W - 1) + j] = x_c[-1 - j].  Read at entry, written at exit.  A zero-filled buffer is a fresh stream preceded
 *     by zeros (+0).  NULL = zero history, nothing kept.
 *   - there is no stream position; any split of a stream into calls (empty calls and calls shorter than W - 1 included) gives the
 *     same bits and the same final state.  A call with S = 0 returns at once and leaves the state alone.
 *   - y may not overlap x.  x is never written; nothing past each row's S outputs is.
 * Limits: 1 <= W <= SDSP_HIP_RANK_MAX_WINDOW (SDSP_HIP_RANK_MAX_WINDOW_F64 for F64; W = 1 is a copy), 1 <= channels < 2^31,
 * S < 2^31.
 */
#define SDSP_HIP_RANK_MAX_WINDOW 255
#define SDSP_HIP_RANK_MAX_WINDOW_F64 127
#define SDSP_HIP_RANK_DEPART_TILE 0 /* the departing sample x[n - W] comes from a second staged tile of the input */
typedef struct sdsp_hip_rank_plan sdsp_hip_rank_plan;
/* Errors: channels or window out of range: SDSP_HIP_ERR_INVALID_SIZE; a null pointer, a rank >= window, a precision other than
 * F32 / F64: SDSP_HIP_ERR_INVALID_ARG; no device: SDSP_HIP_ERR_NO_DEVICE. */
int sdsp_hip_rank_plan_create(sdsp_hip_rank_plan **plan, uint64_t channels, uint32_t window, uint32_t rank, int precision, int device);
int sdsp_hip_rank_plan_destroy(sdsp_hip_rank_plan *plan);
/*
 * x, y: DEVICE pointers; state: DEVICE pointer or NULL.  Asynchronous on `stream`, allocates nothing (stream-capturable); one call
 * per plan in flight.  Errors: null plan, x or y, a stride < samples with more than one channel, overlapping ranges, misaligned
 * pointers: SDSP_HIP_ERR_INVALID_ARG; samples >= 2^31: SDSP_HIP_ERR_INVALID_SIZE; a grid that does not fit one launch:
 * SDSP_HIP_ERR_UNSUPPORTED.  samples == 0: nothing to do.
 */
int sdsp_hip_rank_process(sdsp_hip_rank_plan *plan, const void *x, uint64_t x_stride, void *y, uint64_t y_stride, uint64_t samples,
                          void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_rank_process_host(sdsp_hip_rank_plan *plan, const void *host_x, uint64_t x_stride, void *host_y, uint64_t y_stride,
                               uint64_t samples, void *host_state);
/* bytes of the plan's state buffer: channels (W - 1) element size */
int sdsp_hip_rank_state_bytes(const sdsp_hip_rank_plan *plan, uint64_t *bytes);
/* kernel variants (identical bits): 0 = sdsp_rank_kernel (a lane per run of consecutive outputs, the window as a sorted array of keys
 * in registers, one delete-and-insert pass per output, rows transposed through LDS); 1 = sdsp_rank_plain_kernel, one thread per output
 * from global memory, selection by counting in O(W^2) (the cross-check; it shares no logic with variant 0). */
int sdsp_hip_rank_plan_set_variant(sdsp_hip_rank_plan *plan, int variant);
/* outputs per lane of sdsp_rank_kernel.  0 (the default) = chosen per call from channels, S and W: enough lanes to fill the device at
 * the kernel's occupancy, runs of at least 4 W, a multiple of 16.  Any other value is taken as it is (capped at S).  The bits do not
 * depend on it; the override exists for tests and benchmarks.  run >= 2^31: SDSP_HIP_ERR_INVALID_SIZE. */
int sdsp_hip_rank_plan_set_run(sdsp_hip_rank_plan *plan, uint64_t run);
/* kernel launches of one process call with a state buffer: the filter kernel, and one for the new history when W > 1; 0 for
 * samples == 0 */
int sdsp_hip_rank_plan_launches(const sdsp_hip_rank_plan *plan, uint64_t samples, uint64_t *launches);
typedef struct {
    uint64_t channels;
    uint32_t window, rank;
    uint32_t padded;    /* WP: the compile-time size of the sorted array (8, 16 .. 256), W keys and WP - W sentinels above them */
    uint32_t out_index; /* the array index the output is read from (the rank: no sentinels lie below the window) */
    uint32_t run;       /* set_run's value; 0 = automatic */
    uint32_t last_run;  /* the run the latest call of variant 0 took; 0 before the first */
    uint32_t block;     /* samples per staging block of sdsp_rank_kernel */
    uint32_t lds_bytes; /* LDS of one workgroup (one wave, 64 runs) of sdsp_rank_kernel; it does not depend on W */
    int departing;      /* where x[n - W] comes from: SDSP_HIP_RANK_DEPART_TILE for every window */
    int precision, device, variant;
    char kernel[64];    /* the kernel the plan's variant runs */
} sdsp_hip_rank_plan_info;
int sdsp_hip_rank_plan_get_info(const sdsp_hip_rank_plan *plan, sdsp_hip_rank_plan_info *info);

/* ------------------------------------------------------------------ CFAR detector banks (CA, GO, SO and OS thresholds) */

/*
 * Constant-false-alarm-rate detector bank: `channels` independent rows, F32 or F64 (channel-major: row c =
 * ptr[c stride .. + S) elements, strides in elements of the row's kind).  A plan fixes train = L (training cells per side), guard = G
 * (guard cells per side), a mode, the OS rank k, the input kind and the factor alpha.  Let half = L + G, W = 2 half + 1 and p_c = the
 * powers of the row's history followed by those of the call's block.  For every input sample n the cell under test is p[n - half]: the
 * bank is causal with a delay of half samples.
 *   - input kinds.  POWER: real rows, used as they are; no value is rejected (negative values, NaN and inf go through the arithmetic
 *     below).  IQ: interleaved I/Q rows (one complex sample is one element), p = fl(fl(re re) + fl(im im)): two products and a sum,
 *     never an FMA -- the bits of the STFT bank's power output.
 *   - training cells: lag (older) = p[n - W + 1 .. n - W + L], lead (newer) = p[n - L + 1 .. n].
 *   - modes; c is a host double rounded once to the precision.
 *       CA: lag = (((+0 + p[n - W + 1]) + p[n - W + 2]) + ..) in ascending index, lead likewise;
 *           thr = fl(fl(lag + lead) c), c = alpha / (2 L).
 *       GO: v = (lag > lead) ? lag : lead, thr = fl(v c), c = alpha / L.     SO: v = (lag < lead) ? lag : lead, the same c.
 *       OS: v = the element of rank k (from 0, ascending, IEEE 754 totalOrder through the rank bank's key) of the 2 L training cells;
 *           thr = fl(v alpha).
 *   - a threshold that is a NaN is written as the canonical quiet NaN (0x7FC00000, F64: 0x7FF8000000000000): IEEE 754 leaves the
 *     sign and payload of a NaN result to the implementation, so this is what makes "the same bits" below hold for such rows too,
 *     across kernel variants, runs and splits.  Every other threshold, infinities and signed zeros included, is the arithmetic's.
 *   - detection: det[n] = (p[n - half] > thr[n]) ? 1 : 0, one byte.  A NaN on either side gives 0.
 *   - outputs: thr (a row of the precision) and det (a row of uint8_t, stride in bytes).  Either may be NULL and is then not written;
 *     both NULL is an error.  Outputs may not overlap x or each other; x is never written; nothing past each row's S outputs is.
 *   - state: one caller-owned device buffer of sdsp_hip_cfar_state_bytes bytes: channels x (W - 1) elements of the input's kind,
 *     newest first: state[c (W - 1) + j] = x_c[-1 - j].  Read at entry, written at exit.  A zero-filled buffer is a fresh stream
 *     preceded by zeros.  NULL = zero history, nothing kept.
 *   - there is no stream position; any split of a stream into calls (empty calls included) gives the same bits and the same final
 *     state.  A call with S = 0 returns at once and leaves the state alone.
 * Limits: 1 <= L <= SDSP_HIP_CFAR_MAX_TRAIN; in OS mode 2 L <= SDSP_HIP_RANK_MAX_WINDOW (SDSP_HIP_RANK_MAX_WINDOW_F64 for F64), the rank
 * bank's register limits; 0 <= G <= SDSP_HIP_CFAR_MAX_GUARD; 0 <= k < 2 L; 1 <= channels < 2^31; S < 2^31.
 */
#define SDSP_HIP_CFAR_CA 0
#define SDSP_HIP_CFAR_GO 1
#define SDSP_HIP_CFAR_SO 2
#define SDSP_HIP_CFAR_OS 3
#define SDSP_HIP_CFAR_POWER 0
#define SDSP_HIP_CFAR_IQ 1
#define SDSP_HIP_CFAR_MAX_TRAIN 128
#define SDSP_HIP_CFAR_MAX_GUARD 255
typedef struct sdsp_hip_cfar_plan sdsp_hip_cfar_plan;
typedef struct {
    uint32_t train, guard;
    int mode;      /* SDSP_HIP_CFAR_CA / GO / SO / OS */
    uint32_t rank; /* OS only (ignored otherwise) */
    int input;     /* SDSP_HIP_CFAR_POWER / IQ */
    double alpha;
} sdsp_hip_cfar_desc;
/* Errors: channels, train or guard out of range: SDSP_HIP_ERR_INVALID_SIZE; a null pointer, an unknown mode or input kind, in OS mode
 * a rank >= 2 train, a precision other than F32 / F64: SDSP_HIP_ERR_INVALID_ARG; no device: SDSP_HIP_ERR_NO_DEVICE. */
int sdsp_hip_cfar_plan_create(sdsp_hip_cfar_plan **plan, uint64_t channels, const sdsp_hip_cfar_desc *desc, int precision, int device);
int sdsp_hip_cfar_plan_destroy(sdsp_hip_cfar_plan *plan);
/*
 * x: DEVICE pointer; thr, det, state: DEVICE pointers or NULL.  Asynchronous on `stream`, allocates nothing (stream-capturable); one
 * call per plan in flight.  Errors: null plan or x, thr and det both null, a stride < samples with more than one channel, overlapping
 * ranges, pointers not aligned to their element size: SDSP_HIP_ERR_INVALID_ARG; samples >= 2^31: SDSP_HIP_ERR_INVALID_SIZE; a grid
 * that does not fit one launch: SDSP_HIP_ERR_UNSUPPORTED.  samples == 0: nothing to do.
 */
int sdsp_hip_cfar_process(sdsp_hip_cfar_plan *plan, const void *x, uint64_t x_stride, void *thr, uint64_t thr_stride, uint8_t *det,
                          uint64_t det_stride, uint64_t samples, void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_cfar_process_host(sdsp_hip_cfar_plan *plan, const void *host_x, uint64_t x_stride, void *host_thr, uint64_t thr_stride,
                               uint8_t *host_det, uint64_t det_stride, uint64_t samples, void *host_state);
/* bytes of the plan's state buffer: channels (W - 1) element size of the input's kind */
int sdsp_hip_cfar_state_bytes(const sdsp_hip_cfar_plan *plan, uint64_t *bytes);
/* alpha for later calls; the state is left alone */
int sdsp_hip_cfar_plan_set_alpha(sdsp_hip_cfar_plan *plan, double alpha);
/* kernel variants (identical bits): 0 = sdsp_cfar_sum_kernel for CA, GO and SO (a workgroup per row segment, powers and one boxcar per
 * position in LDS, eight consecutive boxcars per thread in registers: L additions per output) and sdsp_cfar_os_kernel for OS (the rank
 * bank's lane per run with the 2 L training keys as a sorted array in registers, two delete-and-insert passes per output);
 * 1 = sdsp_cfar_plain_kernel, one thread per output from global memory, plain loops and selection by counting (the cross-check; it
 * shares no logic with variant 0). */
int sdsp_hip_cfar_plan_set_variant(sdsp_hip_cfar_plan *plan, int variant);
/* outputs per workgroup (sum modes, capped at info.block) or per lane (OS) of variant 0.  0 (the default) = chosen per call from
 * channels, S and W.  The bits do not depend on it; the override exists for tests and benchmarks.  run >= 2^31:
 * SDSP_HIP_ERR_INVALID_SIZE. */
int sdsp_hip_cfar_plan_set_run(sdsp_hip_cfar_plan *plan, uint64_t run);
/* kernel launches of one process call with a state buffer: the detector kernel and one for the new history; 0 for samples == 0 */
int sdsp_hip_cfar_plan_launches(const sdsp_hip_cfar_plan *plan, uint64_t samples, uint64_t *launches);
typedef struct {
    uint64_t channels;
    uint32_t train, guard, half, window; /* half = L + G, window = W = 2 half + 1 */
    uint32_t lag_shift;                  /* D = L + 2 G + 1: the lag sum at n is the lead sum at n - D */
    uint32_t rank;                       /* OS only */
    uint32_t padded;                     /* OS: WP, the compile-time size of the sorted array (8, 16 .. 256); else 0 */
    uint32_t run;                        /* set_run's value; 0 = automatic */
    uint32_t last_run;                   /* the run the latest call of variant 0 took; 0 before the first */
    uint32_t block;                      /* sum modes: the largest segment of a workgroup; OS: samples per staging block */
    uint32_t lds_bytes;                  /* LDS of one workgroup of the variant-0 kernel */
    double alpha, scale;                 /* alpha as given; c (OS: alpha) as rounded to the precision */
    int mode, input, precision, device, variant;
    char kernel[64];                     /* the kernel the plan's variant runs */
} sdsp_hip_cfar_plan_info;
int sdsp_hip_cfar_plan_get_info(const sdsp_hip_cfar_plan *plan, sdsp_hip_cfar_plan_info *info);

/* ------------------------------------------------------------------ 2-D CFAR plans on range-Doppler maps */

/*
 * 2-D cell-averaging CFAR: a detector over `maps` compact maps of D rows (Doppler, the circular axis) by R
 * columns (range, with edges), with an ordered list of detections per map.  Stateless: a map is complete in itself.
 *   - layout.  Rows are real, F32 or F64; element [m][d][r] is at (m D + d) R + r: exactly the POWER output of a column plan with
 *     n = D, width = R.  Maps are compact: there is no row pitch and no row-distance parameter (as for the column plans), so every
 *     size is a uint32_t (D, R) or the uint64_t count of maps.
 *   - window.  A plan fixes train_d = Ld, guard_d = Gd, train_r = Lr, guard_r = Gr (Hd = Ld + Gd, Hr = Lr + Gr), an edge mode, a peak
 *     flag, and alpha or a scale table.  The training set of cell (d, r) is every ((d + i) mod D, r + j) with |i| <= Hd and |j| <= Hr
 *     except the guard box |i| <= Gd and |j| <= Gr.  Cells with r + j outside [0, R) count as +0 in the sums and are left out of the
 *     cell count n(r) = (2 Hd + 1) wf(r) - (2 Gd + 1) wg(r), where wf(r) is the number of in-map columns in r - Hr .. r + Hr and wg(r)
 *     that in r - Gr .. r + Gr.
 *   - sums.  Every sum starts from +0 and adds in ascending index, one rounding per addition, never an FMA.  Per row:
 *         lag(d, r)  = sum_{j = -Hr .. -Gr - 1} p[d][r + j]      mid(d, r) = sum_{j = -Gr .. Gr} p[d][r + j]
 *         lead(d, r) = sum_{j = Gr + 1 .. Hr} p[d][r + j]        side = fl(lag + lead)      full = fl(fl(lag + mid) + lead)
 *     and across rows, with d + i taken mod D:
 *         top = sum_{i = -Hd .. -Gd - 1} full(d + i, r)    band = sum_{i = -Gd .. Gd} side(d + i, r)
 *         bottom = sum_{i = Gd + 1 .. Hd} full(d + i, r)   T = fl(fl(top + band) + bottom).
 *     There is no subtraction, hence no cancellation; an empty sum is +0.
 *   - threshold.  thr = fl(T c(r)); c(r) is a host double rounded once to the precision: alpha / n(r), or entry r of the caller's
 *     table of R doubles when one is given (each finite once rounded).  A NaN threshold is written as the canonical quiet NaN (sign 0,
 *     the top mantissa bit alone), as sdsp_hip_cfar_process does.
 *   - edges.  SDSP_HIP_CFAR2D_EDGE_MARK: the cells with r < Hr or r >= R - Hr get thr = +inf, det = 0 and no hit (what
 *     simpledsp_amd.cfar does).  SDSP_HIP_CFAR2D_EDGE_CLIP: those cells are tested against their clipped training set with c(r) as above.
 *   - detection.  det = (p > thr) ? 1 : 0: a NaN on either side gives 0.  With peak != 0 a hit must also be the local maximum of its
 *     eight neighbours (d + i mod D, r + j), |i|, |j| <= 1; out-of-map columns are ignored; D = 1 or 2 compares with the wrapped cells
 *     as they fall (for D = 1 that includes the cell itself, which it never exceeds).  The comparison is p > q for the neighbours that
 *     precede the cell in (i, j) lexicographic order and p >= q for those that follow: a plateau yields exactly one hit, and a NaN
 *     neighbour suppresses the hit.  det then carries the peak condition too.
 *   - outputs.  Each may be NULL; all NULL is SDSP_HIP_ERR_INVALID_ARG.  thr: a map of the precision.  det: a uint8_t map.  The hit
 *     list: hits[m][0 .. cap) records and counts[m], which go together.  counts[m] is the total number of hits of map m, even when it
 *     exceeds cap (a total above 2^32 - 1 is written as 2^32 - 1); records k < min(counts[m], cap) are the hits in ascending
 *     (doppler, range); nothing at or past that index is written.
 *   - outputs may not overlap the input or each other; the input is never written.  Pointers need the alignment of one element of
 *     their type (hits: 4 bytes in F32, 8 in F64; counts: 4) and no more.
 *   - independence.  The bits of cell (m, d, r) depend only on its own window and the plan: not on maps, m, which outputs were asked
 *     for, the variant, or pointer alignment.
 *   - limits.  Lr, Gr <= SDSP_HIP_CFAR2D_MAX_R; Ld <= SDSP_HIP_CFAR2D_MAX_TRAIN_D, Gd <= SDSP_HIP_CFAR2D_MAX_GUARD_D; Ld + Lr >= 1;
 *     2 Hd + 1 <= D <= 2^20; 1 <= R < 2^31; maps D R < 2^40; cap < 2^31.
 *   - process is asynchronous on `stream`, allocates nothing and can be captured in a graph: the list's workspace (12 bytes per row and
 *     strip of 64 columns) is allocated at plan creation from max_maps.  maps > max_maps is SDSP_HIP_ERR_INVALID_SIZE; maps == 0 does
 *     nothing.
 * Errors: a window, D, R, max_maps, maps or cap outside the limits: SDSP_HIP_ERR_INVALID_SIZE; a null plan, descriptor or input, all
 * outputs null, hits without counts or counts without hits, an unknown edge mode or precision, a table value that is not
 * finite once rounded (alpha / n(r) is not checked), a misaligned pointer, an overlap: SDSP_HIP_ERR_INVALID_ARG; set_alpha on a plan made with a
 * table: SDSP_HIP_ERR_INVALID_ARG; a map that needs more than 2^31 - 1 workgroups: SDSP_HIP_ERR_UNSUPPORTED; no device:
 * SDSP_HIP_ERR_NO_DEVICE.  Arguments are checked before a device is looked for.
 */
typedef struct sdsp_hip_cfar2d_plan sdsp_hip_cfar2d_plan;
#define SDSP_HIP_CFAR2D_EDGE_MARK 0
#define SDSP_HIP_CFAR2D_EDGE_CLIP 1
#define SDSP_HIP_CFAR2D_MAX_R 64       /* train_r and guard_r, each */
#define SDSP_HIP_CFAR2D_MAX_TRAIN_D 32
#define SDSP_HIP_CFAR2D_MAX_GUARD_D 16
#define SDSP_HIP_CFAR2D_MAX_D (1u << 20)
typedef struct {
    uint32_t train_d, guard_d, train_r, guard_r;
    int edge;     /* SDSP_HIP_CFAR2D_EDGE_MARK or _CLIP */
    int peak;     /* != 0: the 3 x 3 peak rule */
    double alpha; /* c(r) = alpha / n(r); unused with a scale table */
} sdsp_hip_cfar2d_desc;
typedef struct {
    uint32_t doppler, range;
    float power, thr;
} sdsp_hip_cfar2d_hit_f32; /* 16 bytes */
typedef struct {
    uint32_t doppler, range;
    double power, thr;
} sdsp_hip_cfar2d_hit_f64; /* 24 bytes */
/* scale_or_null: R host doubles c(r) that replace alpha / n(r) */
int sdsp_hip_cfar2d_plan_create(sdsp_hip_cfar2d_plan **plan, uint32_t D, uint32_t R, uint64_t max_maps, const sdsp_hip_cfar2d_desc *desc,
                                const double *scale_or_null, int precision, int device);
int sdsp_hip_cfar2d_plan_destroy(sdsp_hip_cfar2d_plan *plan);
/* DEVICE pointers; hits: maps x cap records of the precision, counts: maps totals */
int sdsp_hip_cfar2d_process(sdsp_hip_cfar2d_plan *plan, const void *p, void *thr, uint8_t *det, void *hits, uint32_t *counts, uint64_t cap,
                            uint64_t maps, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_cfar2d_process_host(sdsp_hip_cfar2d_plan *plan, const void *host_p, void *host_thr, uint8_t *host_det, void *host_hits,
                                 uint32_t *host_counts, uint64_t cap, uint64_t maps);
/* a new alpha: c(r) = alpha / n(r) again (synchronous: it uploads the table; not for plans made with a scale table) */
int sdsp_hip_cfar2d_plan_set_alpha(sdsp_hip_cfar2d_plan *plan, double alpha);
/* kernel variants (the same bits): 0 = sdsp_cfar2d_kernel, tiles of tile_rows x 64 cells through LDS, the list by a scan of the
 * per-(row, strip) counts and a placement launch; 1 = sdsp_cfar2d_plain_kernel, one thread per cell from global memory with plain
 * loops in the contract's order, the list by a count, a sequential scan and a placement with one thread per row (the cross-check) */
int sdsp_hip_cfar2d_plan_set_variant(sdsp_hip_cfar2d_plan *plan, int variant);
/* kernel launches of one process of maps >= 1 maps: variant 0: 1, with a list 3; variant 1: 1 for thr / det plus 3 for a list */
int sdsp_hip_cfar2d_plan_launches(const sdsp_hip_cfar2d_plan *plan, int with_thr_or_det, int with_hits, uint64_t *launches);
typedef struct {
    uint32_t D, R;
    uint64_t max_maps;
    uint32_t train_d, guard_d, train_r, guard_r;
    uint32_t cells;             /* n(r) of an interior column: (2 Hd + 1)(2 Hr + 1) - (2 Gd + 1)(2 Gr + 1) */
    int edge, peak, tabled, precision, device, variant;
    double alpha;
    uint32_t tile_rows, tile_cols; /* the cells one workgroup of the variant's kernel computes */
    uint32_t threads;              /* of one workgroup */
    uint32_t lds_bytes;            /* of one workgroup */
    uint64_t workspace_bytes;      /* the list's workspace, allocated at creation */
    char kernel[64];               /* the kernel the plan's variant runs */
} sdsp_hip_cfar2d_plan_info;
int sdsp_hip_cfar2d_plan_get_info(const sdsp_hip_cfar2d_plan *plan, sdsp_hip_cfar2d_plan_info *info);
/* host designer: the constant-false-alarm table c(r) = pfa^(-1 / n(r)) - 1, r < R (the CA formula alpha_n / n for n independent
 * exponential cells), for the clipped counts n(r); a column with n(r) = 0 gets +inf.  0 < pfa < 1, else SDSP_HIP_ERR_INVALID_ARG */
int sdsp_hip_cfar2d_scale(uint32_t D, uint32_t R, const sdsp_hip_cfar2d_desc *desc, double pfa, double *scale);

/* ------------------------------------------------------------------ carrier-recovery PLL / Costas loop banks */

/*
 * Carrier-recovery bank: `channels` independent second-order phase-locked loops on interleaved I/Q rows, F32
 * or F64 (channel-major: row c = ptr[c stride .. + S) elements, strides in elements of the row's kind: one complex sample is one
 * element of x and y, one real is one element of err and freq).  Each loop has a numerically controlled oscillator with a 32-bit
 * phase accumulator theta, a phase detector fixed by the plan, and a proportional-plus-integral loop filter whose gains alpha and beta
 * are arguments of the call (acquire wide, then track narrow; a zero gain freezes that path).  R is the plan precision.
 * Notation: ma(a, b, c) = a b + c as one fmaf in F32 and as a multiply then an add, each rounded, in F64.  u (x) v = (ur vr - ui vi,
 * ur vi + ui vr): four products, one difference and one sum, each rounded.  Per channel, for n = 0 .. S - 1, in this order:
 *   1. oscillator: j = theta.  w = C[j >> 21] (x) F[(j >> 10) & 0x7ff] with C[a] = e^(-2 pi i a / 2^11) and F[a] = e^(-2 pi i a / 2^22),
 *      2048 entries each, the doubles of sdsp_hip_pll_oscillator rounded once to R.  The accumulator keeps all 32 bits (a frequency
 *      resolution of 2^-32 cycles per sample); the oscillator sees the top 22 (a phase granularity of 2^-22 cycle, about 1.5 urad).
 *   2. mix: y = x[n] (x) w.
 *   3. detector.  CROSS: e = yi (a tone or pilot).  BPSK: e = yr yi, one rounded product.  QPSK: e = a - b, a = yi with its sign bit
 *      flipped when the sign bit of yr is set, b = yr with its sign bit flipped when the sign bit of yi is set: bit operations, -0
 *      counts as negative.
 *   4. loop filter: integ = ma(beta, e, integ); then integ = integ < -max_dev ? -max_dev : (integ > max_dev ? max_dev : integ) (a NaN
 *      stays a NaN); v = ma(alpha, e, integ).
 *   5. advance: t = v 2^32 (a power-of-two scaling); t = t < lo ? lo : (t > hi ? hi : t) with lo = -2^31 and hi = 2^31 - 128 in F32,
 *      2^31 - 1 in F64; a NaN becomes 0; k = t rounded to the nearest integer, ties to even, as int32;
 *      theta = theta + fcw0 + k mod 2^32.
 *   6. outputs: y[n], err[n] = e, freq[n] = integ after its clamp: the tracked frequency offset in cycles per sample.
 * With this sign convention a carrier at fcw0 / 2^32 + df cycles per sample drives freq to +df.  alpha, beta and max_dev are host
 * doubles, each rounded once to R (max_dev at plan creation).  Outputs are bit-exact for finite data.  A NaN in x poisons its own
 * channel and no other: y[n] and err[n] of that sample and integ, hence freq, from that sample on are NaN, while theta goes on at
 * fcw0, so the later y and err are those of the open loop (the payload of such a NaN is not contracted).
 *   - state: one caller-owned device buffer of sdsp_hip_pll_state_bytes = channels (sizeof(R) + 4) bytes: channels elements of R
 *     (integ), then channels uint32_t (theta).  Read at entry, written at exit.  A zero-filled buffer is a fresh loop at phase 0.
 *     NULL = zero state, nothing kept.
 *   - there is no history and no stream position: any split of a stream into calls (empty calls included) gives the same bits and the
 *     same final state.  A call with S = 0 returns at once and leaves the state alone.
 *   - y, err and freq may each be NULL and are then not written.  y may be x itself (the same pointer and stride); any other overlap
 *     between an output and x or another output, or between the state buffer and x or an output, is an error.  Nothing past each
 *     row's S outputs is written.
 * Limits: 1 <= channels < 2^31, S < 2^31, 0 < max_dev <= 0.5.
 */
#define SDSP_HIP_PLL_CROSS 0
#define SDSP_HIP_PLL_BPSK 1
#define SDSP_HIP_PLL_QPSK 2
typedef struct sdsp_hip_pll_plan sdsp_hip_pll_plan;
/* host helper: coarse[2 a], coarse[2 a + 1] = re, im of e^(-2 pi i a / 2^11) and fine[..] of e^(-2 pi i a / 2^22), a < 2048, in double;
 * the axis values are exact */
int sdsp_hip_pll_oscillator(double *coarse, double *fine);
/* host helper: the gains of a loop of noise bandwidth bn (cycles per sample, > 0) and damping zeta (> 0) for a signal of the given
 * amplitude (> 0).  theta = bn / (zeta + 1 / (4 zeta)), d = 1 + 2 zeta theta + theta^2, alpha = 4 zeta theta / (d Kd 2 pi),
 * beta = 4 theta^2 / (d Kd 2 pi); the detector gain per radian Kd is A (CROSS), A^2 (BPSK), A sqrt(2) (QPSK); the factor 2 pi is there
 * because the loop works in cycles.  Errors: a null pointer, an unknown mode, an argument that is not finite and > 0:
 * SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_pll_gains(double bn, double zeta, double amplitude, int mode, double *alpha, double *beta);
/* fcw0: n_fcw0 = channels centre-frequency words (sdsp_hip_ddc_phase_word), or n_fcw0 = 1 for one word shared by every channel (HOST
 * pointer).  Errors: channels out of range: SDSP_HIP_ERR_INVALID_SIZE; a null pointer, n_fcw0 other than 1 or channels, an unknown
 * mode, a precision other than F32 / F64, a max_dev that is not in (0, 0.5] once rounded to the precision: SDSP_HIP_ERR_INVALID_ARG; no
 * device: SDSP_HIP_ERR_NO_DEVICE. */
int sdsp_hip_pll_plan_create(sdsp_hip_pll_plan **plan, uint64_t channels, int precision, int mode, const uint32_t *fcw0, uint64_t n_fcw0,
                             double max_dev, int device);
int sdsp_hip_pll_plan_destroy(sdsp_hip_pll_plan *plan);
/*
 * x: DEVICE pointer; y, err, freq, state: DEVICE pointers or NULL.  Asynchronous on `stream`, one launch, allocates nothing
 * (stream-capturable); one call per plan in flight.  Errors: null plan, null x with samples > 0, a stride < samples with more than one
 * channel, overlapping ranges other than y == x, misaligned pointers, an alpha or beta that is not finite in the precision:
 * SDSP_HIP_ERR_INVALID_ARG; samples >= 2^31: SDSP_HIP_ERR_INVALID_SIZE; a grid that does not fit one launch: SDSP_HIP_ERR_UNSUPPORTED.
 * samples == 0: nothing to do.
 */
int sdsp_hip_pll_process(sdsp_hip_pll_plan *plan, const void *x, uint64_t x_stride, void *y, uint64_t y_stride, void *err,
                         uint64_t err_stride, void *freq, uint64_t freq_stride, uint64_t samples, double alpha, double beta, void *state,
                         void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_pll_process_host(sdsp_hip_pll_plan *plan, const void *host_x, uint64_t x_stride, void *host_y, uint64_t y_stride,
                              void *host_err, uint64_t err_stride, void *host_freq, uint64_t freq_stride, uint64_t samples, double alpha,
                              double beta, void *host_state);
/* bytes of the plan's state buffer: channels (sizeof(R) + 4) */
int sdsp_hip_pll_state_bytes(const sdsp_hip_pll_plan *plan, uint64_t *bytes);
/* kernel variants (identical bits): 0 = sdsp_pll_kernel (a lane per channel with theta and integ in registers for the whole call, both
 * tables in LDS, rows transposed through LDS); 1 = sdsp_pll_plain_kernel, one thread per channel from global memory, the tables read
 * from global memory and the state read-modify-written (the cross-check; it shares no staging logic with variant 0).  Selecting
 * variant 1 allocates one plan-owned state buffer once, for calls without a state buffer. */
int sdsp_hip_pll_plan_set_variant(sdsp_hip_pll_plan *plan, int variant);
/* kernel launches of one process call: 1; 0 for samples == 0 */
int sdsp_hip_pll_plan_launches(const sdsp_hip_pll_plan *plan, uint64_t samples, uint64_t *launches);
typedef struct {
    uint64_t channels;
    uint32_t block;     /* samples per time block of sdsp_pll_kernel */
    uint32_t waves;     /* waves (of 64 channels each) per workgroup of sdsp_pll_kernel */
    uint32_t lds_bytes; /* LDS of one workgroup of sdsp_pll_kernel: both tables and `waves` tiles of 4 x block rows of 65 reals */
    double max_dev;     /* as rounded to the precision */
    int precision, mode, device, variant;
    char kernel[64];    /* the kernel the plan's variant runs */
} sdsp_hip_pll_plan_info;
int sdsp_hip_pll_plan_get_info(const sdsp_hip_pll_plan *plan, sdsp_hip_pll_plan_info *info);

/* ------------------------------------------------------------------ symbol-timing recovery banks (Gardner, zero-crossing) */

/*
 * Symbol-timing recovery bank: `channels` independent second-order timing loops on interleaved I/Q rows, F32
 * or F64 (channel-major: row c = ptr[c stride ..), strides in elements of the row's kind: one complex sample is one element of x and
 * y, one real is one element of err and period).  Each loop interpolates its row with the nearest-phase polyphase interpolator of the
 * arbitrary-ratio resampler (L phases of T taps, H[p][k] = h[k L + p] rounded once to R, exactly as sdsp_hip_arb_tables lays it out)
 * at two strobes per symbol, measures the timing error on the symbol strobes with the plan's detector, and steers its step through a
 * proportional-plus-integral loop filter whose gains alpha and beta are arguments of the call.  The number of symbols a channel
 * yields depends on its data and differs from channel to channel.  R is the plan precision.
 * Notation: ma(a, b, c) = a b + c as one fmaf in F32 and as a multiply then an add, each rounded, in F64.  s(v) = +1 or -1 by the sign
 * bit of v (-0 counts as negative; s of a NaN is a NaN).  step0 is the nominal half-symbol period as a Q32.32 word, 2^32 <= step0 <= 2^38 (2 to 128 samples
 * per symbol, not necessarily an integer; sdsp_hip_timing_step).  Per channel the state is: the integrator integ (R), the stream time
 * t (uint64, Q32.32: the integer part counts from the first sample of the call, the fraction is the sub-sample position), the advance
 * word w (int32), parity (0: the next strobe is a mid-symbol strobe, 1: a symbol strobe), the previous symbol strobe ps and the last
 * mid-symbol strobe ym (complex R), and the T - 1 input samples in front of the call, newest first.
 * Per channel, while (t >> 32) < S, in this order:
 *   1. interpolate: i = t >> 32, f = t & 0xffffffff, p = f >> (32 - log2 L) (0 when L = 1).  Per real plane z = H[p][0] x[i], a plain
 *      product, then z = ma(H[p][k], x[i - k], z) for k = 1 .. T - 1 in ascending order; x at negative indices is the history.
 *   2. parity == 0 (mid-symbol strobe): ym = z; parity = 1.
 *   3. otherwise (symbol strobe):
 *        detector.  GARDNER: dr = ps.r - z.r, di = ps.i - z.i, e = ma(di, ym.i, dr ym.r) (dr ym.r is one rounded product).
 *                   ZC_QPSK: the same with dr = s(ps.r) - s(z.r) and di = s(ps.i) - s(z.i).
 *                   ZC_BPSK: e = (s(ps.r) - s(z.r)) ym.r, one rounded product.
 *        loop filter.  integ = ma(beta, e, integ); integ = integ < -max_dev ? -max_dev : (integ > max_dev ? max_dev : integ) (a NaN
 *                   stays a NaN); v = ma(alpha, e, integ); q = v 2^32 (a power-of-two scaling); q = q < lo ? lo : (q > hi ? hi : q)
 *                   with lo = -2^31 and hi = 2^31 - 128 in F32, 2^31 - 1 in F64; a NaN becomes 0; w = q rounded to the nearest integer,
 *                   ties to even, as int32.
 *        outputs.   With m the channel's count of this call so far: y[m] = z, err[m] = e, period[m] = integ (after its clamp: the
 *                   tracked offset of the half-symbol period from step0, in samples); then the count goes up by one.
 *        ps = z; parity = 0.
 *   4. t = t + step0 + w.  The word set at a symbol strobe serves both half steps up to the next one.  step0 >= 2^32 and |w| <= 2^31:
 *      the advance is always positive, and at most two strobes fall on one input sample.
 * At the end of the call t = t - (S << 32) and the history becomes the last T - 1 inputs.  Sign convention: e < 0 means the strobes
 * are late and the period shrinks.  alpha, beta and max_dev are host doubles, each rounded once to R (max_dev at plan creation); zero
 * gains free-run at step0.  Outputs are bit-exact for finite data.  A NaN in x poisons its own channel and no other: the strobes
 * whose windows hold it, and integ (hence period) from the first such symbol on, are NaN, while the time goes on at step0, so the
 * channel's count and its later y are those of the open loop (the payload of such a NaN is not contracted).  ZC_BPSK reads real
 * parts only in its detector: a NaN in an imaginary part alone reaches y and nothing else.
 *   - outputs: y is required; err and period may each be NULL and are then not written.  counts, a required DEVICE array of `channels`
 *     uint32_t, receives each channel's number of symbols of this call.  Elements of a row at or past its count are not written.  A row
 *     needs room for sdsp_hip_timing_max_out(plan, S) elements, the most any loop yields from S inputs: with n = ceil(S 2^32 / (step0 -
 *     2^31)) strobes at most, (n + 1) / 2 of them symbol strobes.  y, err, period and counts must not overlap x, one another or the state.
 *   - state: one caller-owned DEVICE buffer of sdsp_hip_timing_state_bytes, 8-byte aligned: one array per field, each starting at
 *     the next multiple of 8 bytes, in this order: t (channels uint64_t), ps (channels complex R), ym (channels complex R), integ
 *     (channels R), w (channels int32_t), parity (channels uint32_t), then the history (channels rows of T - 1 complex R, newest first).
 *     Read at entry, written at exit.  A zero-filled buffer is a fresh loop at t = 0 preceded by zeros.  NULL = zero state, nothing kept.
 *   - any split of a stream into calls (empty calls included) gives the same concatenated per-channel outputs and the same final
 *     state, bit for bit.  A call with S = 0 zeroes counts and leaves the state alone.
 * Limits: 1 <= channels < 2^31, S < 2^31, L a power of two <= 128, 1 <= T <= 64, L T <= 4096, 0 < max_dev <= 0.5.
 */
#define SDSP_HIP_TIMING_GARDNER 0
#define SDSP_HIP_TIMING_ZC_QPSK 1
#define SDSP_HIP_TIMING_ZC_BPSK 2
#define SDSP_HIP_TIMING_MAX_PHASES 128
#define SDSP_HIP_TIMING_MAX_TAPS 64
#define SDSP_HIP_TIMING_MAX_TABLE 4096
#define SDSP_HIP_TIMING_MIN_STEP (1ull << 32)
#define SDSP_HIP_TIMING_MAX_STEP (1ull << 38)
typedef struct sdsp_hip_timing_plan sdsp_hip_timing_plan;
/* host helper: the half-symbol step word of sps samples per symbol, round(sps / 2 2^32) with ties to even.  Errors: a null pointer, sps
 * outside [2, 128] (NaN included): SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_timing_step(double sps, uint64_t *step0);
/* host helper: the capacity a row needs for `samples` inputs at step word step0 (see above).  Errors: a null pointer:
 * SDSP_HIP_ERR_INVALID_ARG; step0 outside [2^32, 2^38] or samples >= 2^31: SDSP_HIP_ERR_INVALID_SIZE. */
int sdsp_hip_timing_max_out_for(uint64_t step0, uint64_t samples, uint64_t *n);
/* host helper: the gains of a loop of noise bandwidth bn (cycles per symbol, > 0) and damping zeta (> 0) for a detector of slope kd
 * (units of e per symbol of timing offset, > 0; it depends on the pulse and the amplitude: INTEGRATION.md says how to read it off the
 * open loop) at sps samples per symbol.  theta = bn / (zeta + 1 / (4 zeta)), d = 1 + 2 zeta theta + theta^2,
 * alpha = 4 zeta theta / (d kd) sps / 2, beta = 4 theta^2 / (d kd) sps / 2: v is in samples per half symbol.  Errors: a null pointer, an
 * argument that is not finite and > 0: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_timing_gains(double bn, double zeta, double kd, double sps, double *alpha, double *beta);
/* host helper: the root-raised-cosine matched prototype of `phases` x `taps` values for sps samples per symbol (> 0) and a roll-off in
 * (0, 1]: sampled at sps phases per symbol, centred at (phases taps - 1) / 2, scaled so that the values sum to `phases` (the
 * sdsp_hip_arb_design convention: every phase has about unit gain at DC).  The two removable singularities (the centre and
 * |tau| = 1 / (4 rolloff)) take their limits.  Errors: the shape limits above: SDSP_HIP_ERR_INVALID_SIZE; a null pointer, sps or rolloff
 * out of range: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_timing_design(uint32_t phases, uint32_t taps, double sps, double rolloff, double *h);
/* h: phases x taps HOST doubles.  Errors: channels, phases, taps or step0 out of range: SDSP_HIP_ERR_INVALID_SIZE; a null pointer, an
 * unknown mode, a precision other than F32 / F64, a max_dev that is not in (0, 0.5] once rounded to the precision, a tap that is not
 * finite in the precision: SDSP_HIP_ERR_INVALID_ARG; no device: SDSP_HIP_ERR_NO_DEVICE. */
int sdsp_hip_timing_plan_create(sdsp_hip_timing_plan **plan, uint64_t channels, int precision, int mode, uint32_t phases, uint32_t taps,
                                const double *h, uint64_t step0, double max_dev, int device);
int sdsp_hip_timing_plan_destroy(sdsp_hip_timing_plan *plan);
/*
 * x, y, counts: DEVICE pointers; err, period, state: DEVICE pointers or NULL.  Asynchronous on `stream`, one launch, allocates
 * nothing (stream-capturable); one call per plan in flight.  Errors: null plan, null x, y or counts with samples > 0, x_stride <
 * samples or an output stride < sdsp_hip_timing_max_out with more than one channel, overlapping ranges, misaligned pointers, an alpha
 * or beta that is not finite in the precision: SDSP_HIP_ERR_INVALID_ARG; samples >= 2^31: SDSP_HIP_ERR_INVALID_SIZE; a grid that does
 * not fit one launch: SDSP_HIP_ERR_UNSUPPORTED.  samples == 0: counts is zeroed (when given), nothing else is touched.
 */
int sdsp_hip_timing_process(sdsp_hip_timing_plan *plan, const void *x, uint64_t x_stride, void *y, uint64_t y_stride, void *err,
                            uint64_t err_stride, void *period, uint64_t period_stride, uint32_t *counts, uint64_t samples, double alpha,
                            double beta, void *state, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_timing_process_host(sdsp_hip_timing_plan *plan, const void *host_x, uint64_t x_stride, void *host_y, uint64_t y_stride,
                                 void *host_err, uint64_t err_stride, void *host_period, uint64_t period_stride, uint32_t *host_counts,
                                 uint64_t samples, double alpha, double beta, void *host_state);
/* bytes of the plan's state buffer (the layout above) */
int sdsp_hip_timing_state_bytes(const sdsp_hip_timing_plan *plan, uint64_t *bytes);
/* the capacity a row needs for `samples` inputs: sdsp_hip_timing_max_out_for at the plan's step0 */
int sdsp_hip_timing_max_out(const sdsp_hip_timing_plan *plan, uint64_t samples, uint64_t *n);
/* kernel variants (identical bits): 0 = sdsp_timing_kernel (a lane per channel with the loop in registers for the whole call, the
 * table in LDS, rows transposed through a per-wave LDS ring); 1 = sdsp_timing_plain_kernel, one thread per channel from global memory,
 * the table read from global memory and the state read-modify-written (the cross-check; it shares no staging logic with variant 0).
 * Selecting variant 1 allocates one plan-owned state buffer once, for calls without a state buffer. */
int sdsp_hip_timing_plan_set_variant(sdsp_hip_timing_plan *plan, int variant);
/* kernel launches of one process call: 1; 0 for samples == 0 */
int sdsp_hip_timing_plan_launches(const sdsp_hip_timing_plan *plan, uint64_t samples, uint64_t *launches);
typedef struct {
    uint64_t channels;
    uint64_t step0;
    uint32_t phases, taps;
    uint32_t block;     /* input samples per time block of sdsp_timing_kernel */
    uint32_t waves;     /* waves (of 64 channels each) per workgroup of sdsp_timing_kernel, sized from the plan against 160 KiB */
    uint32_t lds_bytes; /* LDS of one workgroup of sdsp_timing_kernel: the table at its odd row pitch and `waves` rings of
                           block + taps - 1 rows of 65 complex values */
    double max_dev;     /* as rounded to the precision */
    int precision, mode, device, variant;
    char kernel[64];    /* the kernel the plan's variant runs */
} sdsp_hip_timing_plan_info;
int sdsp_hip_timing_plan_get_info(const sdsp_hip_timing_plan *plan, sdsp_hip_timing_plan_info *info);

/*
 * ---- streaming Viterbi decoder banks for convolutional codes (viterbi.hip) ----
 *
 * A bank of soft-decision Viterbi decoders for one rate-1/n convolutional code: `channels` compact rows of steps n soft values in,
 * `steps` decoded bits per row out, the decoder state carried from call to call.  Every operation is on integers: both kernel
 * variants and tests/viterbi_ref.py give the same bits and the same state, with no tolerance.
 * Code: constraint length K = 3 .. 9, n = 2 or 3 generators, each a K-bit integer in the usual octal convention: the most significant
 * bit multiplies the newest input bit (K = 7: 0171, 0133).  The state s holds the last K - 1 input bits, the newest in bit 0: input b
 * takes s to s' = ((s << 1) | b) mod S with S = 2^(K-1), and the predecessors of s' are p0 = s' >> 1 and p1 = p0 + S / 2.
 * Input: row c starts at in + c steps n elements (no stride: the row length is the row distance); the n values of a step are
 * adjacent.  I8: int8, positive favours coded bit 0, -128 is read as -127, 0 is an erasure (a punctured position).  F32: quantised on
 * the way in as q = clamp(rint(fl32(x scale)), -127, 127) with the plan's float `scale`, ties to even, NaN becomes 0.
 * Metrics: path metrics are 32-bit integers that wrap.  The branch from p to s' with coded bits c_j has the metric
 * sum_j (c_j ? -q_j : +q_j); a0 = m[p0] + bm0, a1 = m[p1] + bm1, d = 1 iff (int32)(a1 - a0) > 0 (a tie takes p0), m'[s'] = d ? a1 : a0.
 * Nothing is ever normalised: the spread stays at or below (K - 1) n 254, so the comparison modulo 2^32 is exact.  The best state of a
 * step is the lowest s with the largest (int32)(m[s] - m[0]).  A fresh stream has every metric 0, or with a known start state s0
 * m[s0] = 0 and every other metric -2^20.
 * Traceback: the plan fixes a block B (a multiple of 32, 32 .. 1024) and a depth D (K - 1 .. 4096); Dr = B ceil(D / B).  Every call
 * takes a multiple of B steps, so blocks are aligned to the start of the stream whatever its split into calls.  Block m covers steps
 * [m B, (m + 1) B) and is decided when step e = (m + 1) B - 1 + D has been processed: from the best state of step e walk back D steps
 * and drop them, then walk back B steps and emit them, with s_{t-1} = (s_t >> 1) + d_t[s_t] S / 2 and the bit of step t = bit 0 of
 * s_t.  A call writes `steps` outputs per row: out[t] is the bit of stream step (start of the call + t - Dr); the first Dr outputs of
 * a stream are 0.
 * Output: BYTES: one 0 / 1 byte per bit, row c at out + c steps.  PACKED: uint32 words, least significant bit first, steps / 32 words
 * per row.
 * State: one plan-owned device buffer of sdsp_hip_viterbi_plan_state_bytes, for max_channels channels, in this order: the metrics
 * (max_channels x S int32), the count of steps held (max_channels uint32, at most Dr: outputs in front of it are the zeros of the
 * stream's start), padding to 8 bytes, the decisions (max_channels x Dr x W uint64 with W = max(1, S / 64), oldest step first; bit
 * s % 64 of word s / 64 is d[s]).  Both kernels read it at entry and write it at exit, so a stream may change variant between calls;
 * any split of a stream into calls gives the same bits and the same final state.  process touches the first `channels` channels only.
 * Limits: 1 <= max_channels < 2^31, steps < 2^31.
 */
#define SDSP_HIP_VITERBI_I8 0
#define SDSP_HIP_VITERBI_F32 1
#define SDSP_HIP_VITERBI_BYTES 0
#define SDSP_HIP_VITERBI_PACKED 1
#define SDSP_HIP_VITERBI_MIN_K 3
#define SDSP_HIP_VITERBI_MAX_K 9
#define SDSP_HIP_VITERBI_MAX_BLOCK 1024
#define SDSP_HIP_VITERBI_MAX_DEPTH 4096
#define SDSP_HIP_VITERBI_START_METRIC (-(1 << 20))
typedef struct sdsp_hip_viterbi_plan sdsp_hip_viterbi_plan;
/* host helper: Dr = block ceil(depth / block), the delay in steps between a row's input and its output.  Errors: a null pointer:
 * SDSP_HIP_ERR_INVALID_ARG; block not a multiple of 32 in [32, 1024] or depth outside [1, 4096]: SDSP_HIP_ERR_INVALID_SIZE. */
int sdsp_hip_viterbi_delay(uint32_t block, uint32_t depth, uint32_t *delay);
/* host helper: the encoder of the code above from state 0.  bits: nbits bytes (non-zero counts as 1); with `terminate` K - 1 zero bits
 * follow them; out receives n coded bits (0 / 1 bytes) per input bit, generator 0 first.  Errors: k or n out of range:
 * SDSP_HIP_ERR_INVALID_SIZE; a null pointer (bits may be null with nbits == 0), a generator of 0 or >= 2^k: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_conv_encode(uint32_t k, uint32_t n, const uint32_t *generators, const uint8_t *bits, uint64_t nbits, int terminate, uint8_t *out);
/* generators: n HOST values.  scale is read by F32 plans only and must then be finite and > 0.  The plan starts as after
 * sdsp_hip_viterbi_plan_reset(plan, -1), in variant 0 where K = 7 and in variant 1 elsewhere.  Errors: k, n, block, depth or
 * max_channels out of range: SDSP_HIP_ERR_INVALID_SIZE; a null pointer, an unknown kind, a generator of 0 or >= 2^k, a bad scale:
 * SDSP_HIP_ERR_INVALID_ARG; no device: SDSP_HIP_ERR_NO_DEVICE; no memory for the state: SDSP_HIP_ERR_NOMEM. */
int sdsp_hip_viterbi_plan_create(sdsp_hip_viterbi_plan **plan, uint32_t k, uint32_t n, const uint32_t *generators, uint32_t block,
                                 uint32_t depth, int in_kind, int out_kind, float scale, uint64_t max_channels, int device);
int sdsp_hip_viterbi_plan_destroy(sdsp_hip_viterbi_plan *plan);
/*
 * in, out: DEVICE pointers, aligned to their element (F32: 4 bytes, PACKED: 4 bytes; I8 and BYTES: any byte).  Asynchronous on
 * `stream`, one plain launch, allocates nothing (stream-capturable); one call per plan in flight.  Errors: steps not a multiple of the
 * block, steps >= 2^31, channels above max_channels: SDSP_HIP_ERR_INVALID_SIZE; null plan, null in or out with work to do, a
 * misaligned pointer, in overlapping out, in or out overlapping the state: SDSP_HIP_ERR_INVALID_ARG.  channels == 0 or steps == 0:
 * nothing to do, nothing is touched.
 */
int sdsp_hip_viterbi_process(sdsp_hip_viterbi_plan *plan, const void *in, void *out, uint64_t channels, uint64_t steps, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_viterbi_process_host(sdsp_hip_viterbi_plan *plan, const void *host_in, void *host_out, uint64_t channels, uint64_t steps);
/* a fresh stream in every channel: no steps held, and every metric 0 (start_state == -1) or the known start state 0 <= start_state < S.
 * Synchronous.  Errors: any other start_state: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_viterbi_plan_reset(sdsp_hip_viterbi_plan *plan, int start_state);
/* the metrics of the first `channels` channels, channels x S int32, to or from HOST memory; synchronous.  set_metrics leaves the
 * decisions held alone.  Errors: null pointers: SDSP_HIP_ERR_INVALID_ARG; channels above max_channels: SDSP_HIP_ERR_INVALID_SIZE. */
int sdsp_hip_viterbi_plan_get_metrics(sdsp_hip_viterbi_plan *plan, int32_t *host_metrics, uint64_t channels);
int sdsp_hip_viterbi_plan_set_metrics(sdsp_hip_viterbi_plan *plan, const int32_t *host_metrics, uint64_t channels);
/* bytes of the plan's state buffer (the layout above) */
int sdsp_hip_viterbi_plan_state_bytes(const sdsp_hip_viterbi_plan *plan, uint64_t *bytes);
/* kernel variants (identical bits, one state layout): 0 = sdsp_viterbi_wave_kernel, K = 7 only (a wave per channel, lane = state, the
 * metrics exchanged by ds_bpermute, a step's decisions one ballot word in an LDS ring, the tracebacks of a chunk side by side on the
 * lanes); 1 = sdsp_viterbi_plain_kernel, every K (a workgroup of S threads per channel, the metrics in LDS with a barrier per step).
 * Errors: variant 0 where K != 7: SDSP_HIP_ERR_UNSUPPORTED; any other value: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_viterbi_plan_set_variant(sdsp_hip_viterbi_plan *plan, int variant);
/* kernel launches of one process call: 1; 0 for channels == 0 or steps == 0 */
int sdsp_hip_viterbi_plan_launches(const sdsp_hip_viterbi_plan *plan, uint64_t channels, uint64_t steps, uint64_t *launches);
typedef struct {
    uint32_t k, n, generators[3];
    uint32_t states;      /* S = 2^(k-1) */
    uint32_t block, depth;
    uint32_t delay;       /* Dr */
    uint32_t chunk;       /* steps between two rounds of tracebacks in the variant's kernel: a multiple of block */
    uint32_t threads;     /* per workgroup */
    uint32_t waves;       /* variant 0: channels per workgroup */
    uint32_t lds_bytes;   /* dynamic LDS of one workgroup */
    uint32_t ring_in_lds; /* 0: the plain kernel's decision ring lies in a plan-owned buffer in global memory */
    uint64_t max_channels;
    uint64_t state_bytes;
    float scale;
    int in_kind, out_kind, device, variant;
    char kernel[64];      /* the kernel the plan's variant runs */
} sdsp_hip_viterbi_plan_info;
int sdsp_hip_viterbi_plan_get_info(const sdsp_hip_viterbi_plan *plan, sdsp_hip_viterbi_plan_info *info);

/*
 * ---- Reed-Solomon decoder banks over GF(256) for concatenated codes (rs.hip) ----
 *
 * The outer code behind a Viterbi decoder: errors-and-erasures decoding of many interleaved frames at once.  Everything is integer
 * arithmetic: both kernel variants and tests/rs_ref.py give the same bytes and the same counts, with no tolerance.
 * Field: GF(2^8) is defined by `field_poly`, a 9-bit integer with bit 8 set (0x11D, 0x187, ..), and alpha = 0x02.  Creation refuses a
 * polynomial under which alpha does not have order 255 (0x11B: order 51).
 * Code: the generator is g(x) = prod_{j=0}^{nroots-1} (x - alpha^(prim (fcr + j))) with 0 <= fcr < 255, gcd(prim, 255) = 1
 * (1 <= prim < 255), 2 <= nroots <= 64, nroots < n <= 255 and k = n - nroots.  n < 255 is the shortened code, whose leading 255 - n
 * symbols are zero and absent.  In memory order, symbol i of a codeword is the coefficient of x^(n-1-i).  The code is systematic: k
 * data symbols, then nroots parity symbols.  CCSDS is (0x187, 112, 11, 32 or 16, 255) in the conventional basis, DVB is
 * (0x11D, 0, 1, 16, 204).
 * Frames: a frame is `interleave` = I codewords (1 <= I <= 16), symbol-interleaved: byte s I + j of the frame is symbol s of codeword
 * j.  A call takes `frames` compact frames of I n bytes: the frame length is the frame distance.
 * Erasures: an optional second input of the same layout; a non-zero byte marks that symbol as erased.
 * Result: the result of codeword r with erased set E is defined mathematically, not by algorithm.  If |E| > nroots, the codeword is
 * a failure.  Otherwise, look for a codeword c with 2 |{i not in E : c_i != r_i}| + |E| <= nroots; the minimum distance is
 * nroots + 1, so at most one exists.  If one exists, the output is c, and `corrected` is the number of positions where c differs
 * from r.  If none exists, the codeword is a failure.  A failure leaves the codeword's symbols exactly as received and writes
 * `corrected` = -1.  A received word beyond the bound may decode to another codeword: that is part of the contract and is
 * deterministic.
 * Outputs: `out` is FULL (I n bytes per frame; out == in is allowed and is the in-place form) or DATA (the first I k bytes of each
 * frame, which are exactly the data symbols in the same interleaved order).  Any other overlap of in, out, erasures and corrected is
 * refused.  `corrected` is optional: int32, one per codeword, at [frame I + j].
 * Limits: frames < 2^31.  frames == 0 touches nothing.
 * Errors: sizes out of range: SDSP_HIP_ERR_INVALID_SIZE; a null pointer, an unknown kind, a non-primitive polynomial,
 * gcd(prim, 255) != 1, a misaligned `corrected`, or an overlap: SDSP_HIP_ERR_INVALID_ARG.  A refusal writes nothing.
 */
#define SDSP_HIP_RS_FULL 0
#define SDSP_HIP_RS_DATA 1
#define SDSP_HIP_RS_MAX_NROOTS 64
#define SDSP_HIP_RS_MAX_INTERLEAVE 16
typedef struct sdsp_hip_rs_plan sdsp_hip_rs_plan;
/* host helper: the nroots + 1 coefficients of g, the highest (1) first, into HOST memory */
int sdsp_hip_rs_generator(uint32_t field_poly, uint32_t fcr, uint32_t prim, uint32_t nroots, uint8_t *g);
/* host helper: the systematic encoder.  data: `frames` frames of I k HOST bytes; out: `frames` frames of I n HOST bytes, the data
 * symbols followed by the parity symbols, interleaved as above.  data and out must not overlap. */
int sdsp_hip_rs_encode(uint32_t field_poly, uint32_t fcr, uint32_t prim, uint32_t nroots, uint32_t n, uint32_t interleave,
                       const uint8_t *data, uint64_t frames, uint8_t *out);
/* the argument checks come before the device is touched; the plan starts in variant 0.  Errors as above; no device:
 * SDSP_HIP_ERR_NO_DEVICE; no memory for the field's table: SDSP_HIP_ERR_NOMEM. */
int sdsp_hip_rs_plan_create(sdsp_hip_rs_plan **plan, uint32_t field_poly, uint32_t fcr, uint32_t prim, uint32_t nroots, uint32_t n,
                            uint32_t interleave, int out_kind, int device);
int sdsp_hip_rs_plan_destroy(sdsp_hip_rs_plan *plan);
/* in, erasures (nullable), out: DEVICE bytes at any address; corrected (nullable): DEVICE int32, 4-byte aligned.  Asynchronous on
 * `stream`, one plain launch, allocates nothing (stream-capturable). */
int sdsp_hip_rs_process(sdsp_hip_rs_plan *plan, const void *in, const void *erasures, void *out, int32_t *corrected, uint64_t frames,
                        void *stream);
/* same with HOST pointers (synchronous); host_out == host_in is the in-place form */
int sdsp_hip_rs_process_host(sdsp_hip_rs_plan *plan, const void *host_in, const void *host_erasures, void *host_out,
                             int32_t *host_corrected, uint64_t frames);
/* kernel variants (identical bytes): 0 = sdsp_rs_wave_kernel (a wave per frame: the frame staged and de-interleaved through LDS, lane
 * = symbol position for the syndromes and the root search, lane = coefficient for the key equation); 1 = sdsp_rs_plain_kernel (a
 * thread per codeword, serial loops).  Errors: any other value: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_rs_plan_set_variant(sdsp_hip_rs_plan *plan, int variant);
/* kernel launches of one process call: 1; 0 for frames == 0 */
int sdsp_hip_rs_plan_launches(const sdsp_hip_rs_plan *plan, uint64_t frames, uint64_t *launches);
typedef struct {
    uint32_t field_poly, fcr, prim, nroots, n, interleave;
    uint32_t k;         /* n - nroots */
    uint32_t t;         /* nroots / 2 */
    uint32_t threads;   /* per workgroup */
    uint32_t waves;     /* per workgroup; variant 0: frames a workgroup holds at a time */
    uint32_t lds_bytes; /* LDS of one workgroup */
    int out_kind, device, variant;
    char kernel[64];    /* the kernel the plan's variant runs */
} sdsp_hip_rs_plan_info;
int sdsp_hip_rs_plan_get_info(const sdsp_hip_rs_plan *plan, sdsp_hip_rs_plan_info *info);

/*
 * ---- streaming frame synchroniser banks between the Viterbi and the Reed-Solomon decoders (fsync.hip) ----
 *
 * A bank finds the attached sync marker in `channels` compact rows of bits, at any bit offset and in either polarity, follows it with
 * a SEARCH / VERIFY / LOCK machine per channel, and writes the payloads behind accepted markers as compact frames of bytes, the
 * inversion and a pseudo-random sequence removed: what sdsp_hip_rs_process takes as it lies.  Every operation is on integers: both
 * kernel variants and tests/fsync_ref.py give the same frames, records and state for any split of a stream into calls.
 * Frame: a marker of M bits (8 .. 64, a uint64_t whose bit M - 1 is the first bit on the line; bits at and above M must be 0), then P
 * payload bytes (1 .. 8192); the period is L = M + 8 P bits.  tol: 0 .. min(15, M / 2 - 1); verify V and flywheel F: 0 .. 255;
 * polarity NORMAL or EITHER; pn: nullable HOST array of P bytes that is XORed onto every payload.
 * Input: BYTES: one byte per bit, non-zero counts as 1, row c at in + c nbits, any nbits; PACKED: uint32 words, the oldest bit lowest
 * (sdsp_hip_viterbi_process's PACKED output), nbits / 32 words per row, nbits a multiple of 32.  No strides: rows are compact.
 * Positions count the bits of a channel's stream from 0 at the last reset, as uint64_t; nothing exists in front of position 0.
 * d(p) = popcount(bits[p .. p + M - 1] XOR marker); a normal hit is d <= tol, an inverted hit M - d <= tol (EITHER only; tol < M / 2,
 * so never both).  A position is examined once bit p + M - 1 exists.
 * Machine, per channel (mode, next position p, polarity, count, misses), run while p + M <= bits seen:
 *   SEARCH at p: a hit takes its polarity, count = misses = 0; with V == 0 it goes to LOCK and accepts the frame at p, otherwise to
 *     VERIFY; p += L either way.  No hit: p += 1.
 *   VERIFY at p (the held polarity only): a hit: count += 1, and when count reaches V, LOCK and the frame at this p is accepted;
 *     p += L.  A miss: SEARCH at p - L + 1, so that a false candidate does not shadow a true marker behind it.
 *   LOCK at p: a hit: misses = 0, the frame is accepted, p += L.  A miss: misses += 1; above F: SEARCH at the same p (either polarity
 *     again, nothing accepted); otherwise the frame is accepted with the flywheel flag, p += L.
 * A frame accepted at p is emitted by the call that brings bit p + L - 1, so a call emits at most max_frames(nbits) = ceil(nbits / L)
 * frames per row (sdsp_hip_fsync_max_frames), in stream order, and at most one accepted frame is pending at the end of a call.
 * Outputs, rows compact: out (nullable) uint8 channels x max_frames x P: the payload bits p + M .. p + L - 1, the first bit the most
 * significant of byte 0, XOR 0xFF where the polarity is inverted, XOR pn; counts uint32 per row; pos (nullable) uint64 channels x
 * max_frames: the marker's first bit; info (nullable) uint32: bits 0-7 the polarity-corrected marker distance, bit 8 inverted, bit 9
 * flywheel.  Slots at and beyond counts[c] are not written.
 * State: one plan-owned device buffer of sdsp_hip_fsync_plan_state_bytes: max_channels records of 16 uint32 (0 mode: 0 SEARCH, 1
 * VERIFY, 2 LOCK; 1 polarity; 2 count; 3 misses; 4 pending; 5 the pending frame's info; 6-7 next position; 8-9 bits seen; 10-11 the
 * pending frame's position; 12-15 zero; 64-bit values low word first), then max_channels rings of HW = ceil((L + M) / 32) + 1 uint32:
 * the stream's word W (bits 32 W .. 32 W + 31, the oldest lowest) lies in slot W mod HW, bits at and beyond `bits seen` are 0.  The
 * ring always holds the last L + M bits: the oldest a later decision can need is L + M - 2 back (a VERIFY miss examined one bit
 * behind a call's end).  Both variants read and write it, so a stream may change variant between calls.
 * Limits: 1 <= max_channels < 2^31, 1 <= max_bits < 2^31.
 */
#define SDSP_HIP_FSYNC_BYTES 0
#define SDSP_HIP_FSYNC_PACKED 1
#define SDSP_HIP_FSYNC_NORMAL 0
#define SDSP_HIP_FSYNC_EITHER 1
#define SDSP_HIP_FSYNC_SEARCH 0
#define SDSP_HIP_FSYNC_VERIFY 1
#define SDSP_HIP_FSYNC_LOCK 2
#define SDSP_HIP_FSYNC_MAX_PAYLOAD 8192
#define SDSP_HIP_FSYNC_CCSDS_ASM 0x1ACFFC1Du
typedef struct sdsp_hip_fsync_plan sdsp_hip_fsync_plan;
/* host helper: n bytes of the CCSDS pseudo-randomiser, a[i + 8] = a[i] ^ a[i + 3] ^ a[i + 5] ^ a[i + 7] from eight ones, the first bit
 * the most significant (FF 48 0E C0 9A 0D 70 BC ..; the period is 255 bits).  Errors: out null with n > 0: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_fsync_ccsds_pn(uint8_t *out, uint64_t n);
/* host helper, the transmit side: nframes x P payload bytes -> nframes L bits (0 / 1 bytes): the marker, then the payload XOR pn
 * (nullable), all of it inverted where `invert` is non-zero.  Errors: marker_bits or payload_bytes out of range:
 * SDSP_HIP_ERR_INVALID_SIZE; a null pointer with nframes > 0, marker bits at or above marker_bits: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_fsync_attach(uint64_t marker, uint32_t marker_bits, uint32_t payload_bytes, const uint8_t *pn, const uint8_t *frames,
                          uint64_t nframes, int invert, uint8_t *bits);
/* host helper: ceil(nbits / L).  Errors: sizes out of range: SDSP_HIP_ERR_INVALID_SIZE; null: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_fsync_max_frames(uint32_t marker_bits, uint32_t payload_bytes, uint64_t nbits, uint64_t *frames);
/* max_bits: the most bits per row one call may bring; it sizes the plan-owned workspace of variant 0 (three words per 32 bits and
 * row, and the frame records), so that process allocates nothing.  The plan starts reset, in variant 0.  Errors: marker_bits,
 * payload_bytes, verify, flywheel, max_channels or max_bits out of range: SDSP_HIP_ERR_INVALID_SIZE; a null plan pointer, tol out of
 * range, marker bits at or above marker_bits, an unknown polarity or kind: SDSP_HIP_ERR_INVALID_ARG; no device:
 * SDSP_HIP_ERR_NO_DEVICE; no memory: SDSP_HIP_ERR_NOMEM. */
int sdsp_hip_fsync_plan_create(sdsp_hip_fsync_plan **plan, uint64_t marker, uint32_t marker_bits, uint32_t payload_bytes, uint32_t tol,
                               uint32_t verify, uint32_t flywheel, int polarity, const uint8_t *pn, int in_kind, uint64_t max_channels,
                               uint64_t max_bits, int device);
int sdsp_hip_fsync_plan_destroy(sdsp_hip_fsync_plan *plan);
/*
 * in, out, counts, pos, info: DEVICE pointers, aligned to their element (in: 1 byte for BYTES, 4 for PACKED; out: 1; counts, info: 4;
 * pos: 8).  Asynchronous on `stream`, plain launches only (sdsp_hip_fsync_plan_launches of them), allocates nothing
 * (stream-capturable); one call per plan in flight.  Errors: channels above max_channels, nbits above max_bits, nbits not a multiple
 * of 32 for PACKED: SDSP_HIP_ERR_INVALID_SIZE; null plan, null in or counts with work to do, a misaligned pointer, two of the ranges
 * overlapping, or one overlapping the state: SDSP_HIP_ERR_INVALID_ARG.  channels == 0: nothing is touched.  nbits == 0: counts is
 * zeroed and nothing else is touched.
 */
int sdsp_hip_fsync_process(sdsp_hip_fsync_plan *plan, const void *in, uint8_t *out, uint32_t *counts, uint64_t *pos, uint32_t *info,
                           uint64_t channels, uint64_t nbits, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_fsync_process_host(sdsp_hip_fsync_plan *plan, const void *host_in, uint8_t *host_out, uint32_t *host_counts,
                                uint64_t *host_pos, uint32_t *host_info, uint64_t channels, uint64_t nbits);
/* a fresh stream in every channel: SEARCH at position 0, nothing seen, nothing pending.  Synchronous. */
int sdsp_hip_fsync_plan_reset(sdsp_hip_fsync_plan *plan);
/* the machine of the first `channels` channels to HOST arrays of `channels` values each (every one nullable): mode, next position,
 * polarity, count, misses, pending (0 / 1), bits seen.  Synchronous.  Errors: a null plan: SDSP_HIP_ERR_INVALID_ARG; channels above
 * max_channels: SDSP_HIP_ERR_INVALID_SIZE. */
int sdsp_hip_fsync_plan_get_state(sdsp_hip_fsync_plan *plan, uint32_t *mode, uint64_t *next, uint32_t *polarity, uint32_t *count,
                                  uint32_t *misses, uint32_t *pending, uint64_t *seen, uint64_t channels);
/* bytes of the plan's state buffer (the layout above) */
int sdsp_hip_fsync_plan_state_bytes(const sdsp_hip_fsync_plan *plan, uint64_t *bytes);
/* kernel variants (identical bits, one state layout): 0 = five launches over a packed working row in the plan's workspace (pack by
 * ballot, correlate by v_alignbit and popcount into a hit word per polarity, sdsp_fsync_walk_kernel: a wave per channel with a
 * find-first over 64 hit words per round, extract four bytes per thread, carry); 1 = sdsp_fsync_plain_kernel (a thread per channel,
 * bit by bit).  Errors: any other value: SDSP_HIP_ERR_INVALID_ARG. */
int sdsp_hip_fsync_plan_set_variant(sdsp_hip_fsync_plan *plan, int variant);
/* kernel launches of one process call: variant 0: 5 (4 without out), variant 1: 1; 0 for channels == 0 or nbits == 0 */
int sdsp_hip_fsync_plan_launches(const sdsp_hip_fsync_plan *plan, uint64_t channels, uint64_t nbits, uint64_t *launches);
typedef struct {
    uint64_t marker;
    uint32_t marker_bits, payload_bytes;
    uint32_t period;       /* L */
    uint32_t tol, verify, flywheel;
    uint32_t ring_words;   /* HW */
    uint32_t row_words;    /* words per row and array of variant 0's workspace */
    uint32_t has_pn;
    uint64_t max_channels, max_bits;
    uint64_t max_frames;   /* of a call of max_bits */
    uint64_t state_bytes, workspace_bytes;
    int polarity, in_kind, device, variant;
    char kernel[64];       /* the kernel that runs the machine in the plan's variant */
} sdsp_hip_fsync_plan_info;
int sdsp_hip_fsync_plan_get_info(const sdsp_hip_fsync_plan *plan, sdsp_hip_fsync_plan_info *info);

/*
 * ---- LDPC decoder banks for quasi-cyclic codes, layered min-sum (ldpc.hip) ----
 *
 * A block decoder for many independent codewords of one quasi-cyclic LDPC code: nothing is carried between calls.  Every operation
 * but the F32 quantiser is on integers: both kernel variants and tests/ldpc_ref.py give the same bits, posteriors and status, with no
 * tolerance.
 * Code: a base matrix `base` of mb block rows x nb block columns of int16, row-major, and a lifting size Z.  Entry -1 is the zero
 * block; entry s in [0, Z) is the Z x Z circulant with a one at (i, (i + s) mod Z), so check row r Z + i contains variable
 * c Z + (i + s) mod Z.  n = nb Z variables, m = mb Z checks, one circulant per entry.
 * Limits: 2 <= Z <= 512, 1 <= mb <= 64, mb < nb <= 128, n <= 16384, every row has 2 to 32 entries (a row's sign bits fit one word),
 * every column has at least one entry.  Posteriors then fit int16: |L| <= 127 (1 + 64) = 8255.
 * Soft values: positive favours bit 0, as in the Viterbi banks; 0 is an erasure, which is how punctured columns are fed.  I8: int8,
 * -128 is read as -127.  F32: quantised on the way in as q = clamp(rint(fl32(x scale)), -127, 127) with the plan's float `scale`,
 * ties to even, NaN becomes 0: the one floating-point operation.  One codeword is n compact values: the row length is the row
 * distance.
 * Decoding, each codeword on its own:
 *  1. L[v] = q[v] as integers; all check-to-variable messages R start at 0.
 *  2. One iteration visits the layers r = 0 .. mb - 1 in order; the Z checks of a layer touch different variables, so their order
 *     cannot matter.
 *  3. For a check, number the entries of row r as j = 0 .. d - 1 in ascending block column, v_j the variable of entry j:
 *     T_j = L[v_j] - R_j, a_j = min(|T_j|, 127), sigma_j = (T_j < 0) (zero counts as positive), S = sigma_0 xor .. xor sigma_(d-1),
 *     m1 = the smallest a_j, m2 = the smallest of the others, f(x) = max(((x norm + 8) >> 4) - beta, 0).  The new R_j has magnitude
 *     f(m2) if a_j is the minimum and f(m1) otherwise (with a tie f(m1) = f(m2), so which j "is" the minimum does not matter) and
 *     the sign S xor sigma_j, negative if set; L[v_j] = T_j + R_j(new).  There is no clamp anywhere but the 127 on a_j.
 *  4. norm is 1 .. 16 (sixteenths: 12 is the usual 0.75, 16 is plain min-sum), beta is 0 .. 31; both are plan parameters.
 *  5. The hard decision is h[v] = (L[v] < 0).
 *  6. The syndrome test is "every check has even parity of h", made on the input before the first iteration and after the last
 *     layer of every iteration.
 *  7. With early_stop (a plan parameter) a codeword stops at the first test that passes, and its status is the number of iterations
 *     run: 0 if the input already passes, otherwise 1 .. max_iter.  Without it max_iter iterations always run, and a codeword whose
 *     final test passes has the status max_iter.
 *  8. A codeword whose final test fails gets the status -1; its outputs are still written.
 *  9. A codeword that passes may be another codeword than the one sent: that is deterministic and part of the contract.
 * 10. max_iter is an argument of each call, 0 .. 255; 0 gives the hard decisions of the input and its syndrome.
 * Outputs, each optional, at least one required.  bits: the first out_bits hard decisions of each codeword (1 <= out_bits <= n, a plan
 * parameter: typically n, or (nb - mb) Z for the systematic part), as BYTES (0 / 1, out_bits per codeword) or PACKED (uint32 words,
 * bit v in bit v mod 32 of word v / 32, ceil(out_bits / 32) words per codeword, the unused top bits zero).  post: the int16
 * posteriors L, n per codeword.  status: int32, one per codeword.
 * Buffers: bits, post and status must not overlap the input or each other; F32 input, int16, int32 and word outputs must be aligned
 * to their element; the byte and int8 buffers may lie at any address.  codewords < 2^31; codewords == 0 touches nothing.
 * Errors: mb, nb, Z, n, norm, beta, out_bits, max_iter or codewords out of range: SDSP_HIP_ERR_INVALID_SIZE; a null pointer, an
 * unknown kind, a shift outside [-1, Z), a bad row or column degree, a scale that is not finite and positive (F32), no output at all,
 * misalignment or overlap: SDSP_HIP_ERR_INVALID_ARG.  A refusal writes nothing.
 */
#define SDSP_HIP_LDPC_I8 0
#define SDSP_HIP_LDPC_F32 1
#define SDSP_HIP_LDPC_BYTES 0
#define SDSP_HIP_LDPC_PACKED 1
#define SDSP_HIP_LDPC_MAX_Z 512
#define SDSP_HIP_LDPC_MAX_MB 64
#define SDSP_HIP_LDPC_MAX_NB 128
#define SDSP_HIP_LDPC_MAX_N 16384
#define SDSP_HIP_LDPC_MAX_ROW_DEGREE 32
#define SDSP_HIP_LDPC_MAX_ITER 255
typedef struct sdsp_hip_ldpc_plan sdsp_hip_ldpc_plan;
/* host helper for codewords [data | parity] with k = n - m: the m x ceil(k / 32) HOST words of P with parity = P data over GF(2), bit
 * j of row i in bit j mod 32 of word j / 32, by Gaussian elimination on bit words.  Errors: the code's as above; a null pointer:
 * SDSP_HIP_ERR_INVALID_ARG; the last m columns of H singular: SDSP_HIP_ERR_UNSUPPORTED.  A refusal writes nothing. */
int sdsp_hip_ldpc_parity_matrix(const int16_t *base, uint32_t mb, uint32_t nb, uint32_t z, uint32_t *P);
/* host helper: the systematic encoder of the same codes.  data: `codewords` rows of k HOST bytes (non-zero counts as 1); out:
 * `codewords` rows of n HOST 0 / 1 bytes, the data then the parity.  data and out must not overlap; codewords < 2^31. */
int sdsp_hip_ldpc_encode(const int16_t *base, uint32_t mb, uint32_t nb, uint32_t z, const uint8_t *data, uint64_t codewords, uint8_t *out);
/* base: mb x nb HOST values.  scale is read by F32 plans only.  The argument checks come before the device is touched; the plan
 * starts in variant 0.  Errors as above; no device: SDSP_HIP_ERR_NO_DEVICE; no memory for the table: SDSP_HIP_ERR_NOMEM. */
int sdsp_hip_ldpc_plan_create(sdsp_hip_ldpc_plan **plan, const int16_t *base, uint32_t mb, uint32_t nb, uint32_t z, uint32_t norm,
                              uint32_t beta, int early_stop, int in_kind, float scale, int out_kind, uint32_t out_bits, int device);
int sdsp_hip_ldpc_plan_destroy(sdsp_hip_ldpc_plan *plan);
/* llr, bits (nullable), post (nullable), status (nullable): DEVICE pointers.  Asynchronous on `stream`, plain launches only
 * (sdsp_hip_ldpc_plan_launches of them), allocates nothing (stream-capturable); one call per plan in flight in variant 1, whose
 * workspace belongs to the plan. */
int sdsp_hip_ldpc_process(sdsp_hip_ldpc_plan *plan, const void *llr, void *bits, int16_t *post, int32_t *status, uint64_t codewords,
                          uint32_t max_iter, void *stream);
/* same with HOST pointers (synchronous) */
int sdsp_hip_ldpc_process_host(sdsp_hip_ldpc_plan *plan, const void *host_llr, void *host_bits, int16_t *host_post, int32_t *host_status,
                               uint64_t codewords, uint32_t max_iter);
/* kernel variants (identical bits, posteriors and status): 0 = sdsp_ldpc_wave_kernel (lanes are the checks of a layer; a wave holds
 * floor(64 / Z) codewords side by side where Z <= 32, one where Z <= 64, and walks a layer in ceil(Z / 64) pieces above that; L as
 * int16 and a record of 8 bytes per check in LDS, no barrier); 1 = sdsp_ldpc_plain_kernel (a thread per codeword, L and one int8
 * message per edge in a plan-owned global workspace of at most 256 MiB, which set_variant(1) allocates; a call goes out in pieces
 * of the codewords that fit it).  Errors: any other value: SDSP_HIP_ERR_INVALID_ARG; no memory: SDSP_HIP_ERR_NOMEM. */
int sdsp_hip_ldpc_plan_set_variant(sdsp_hip_ldpc_plan *plan, int variant);
/* kernel launches of one process call: variant 0: 1; variant 1: ceil(codewords / piece); 0 for codewords == 0 */
int sdsp_hip_ldpc_plan_launches(const sdsp_hip_ldpc_plan *plan, uint64_t codewords, uint64_t *launches);
typedef struct {
    uint32_t mb, nb, z;
    uint32_t n, m;            /* nb z, mb z */
    uint32_t edges;           /* per codeword: entries x z */
    uint32_t max_row_degree;
    uint32_t norm, beta, out_bits;
    uint32_t group;           /* variant 0: codewords per wave; variant 1: 1 (per thread) */
    uint32_t threads;         /* per workgroup */
    uint32_t lds_bytes;       /* LDS of one workgroup */
    uint32_t codewords_per_cu; /* variant 0: codewords a compute unit holds at a time by its LDS and wave slots; variant 1: 0 */
    uint64_t piece;           /* variant 1: codewords per launch */
    uint64_t workspace_bytes; /* variant 1 */
    float scale;
    int early_stop, in_kind, out_kind, device, variant;
    char kernel[64];          /* the kernel the plan's variant runs */
} sdsp_hip_ldpc_plan_info;
int sdsp_hip_ldpc_plan_get_info(const sdsp_hip_ldpc_plan *plan, sdsp_hip_ldpc_plan_info *info);

#ifdef __cplusplus
}
#endif
#endif /* SDSP_HIP_H */
