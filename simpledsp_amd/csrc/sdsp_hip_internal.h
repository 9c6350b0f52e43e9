// sdsp_hip_internal.h -- shared declarations of the libsdsp_hip implementation (not installed).
#pragma once

#include "sdsp_hip.h"

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

namespace sdsp_hip
{
extern thread_local std::string g_last_error;
int fail(int code, const std::string &msg);

// Raise a kernel's dynamic-LDS limit (needed above 64 KiB).  The attribute belongs to the function object of the
// CURRENT device, so it is set once per (kernel, device): `done` is the caller's per-kernel mask, bit = device index.
// Safe from concurrent host threads (sharded entry points run one thread per device).  Defined in capi.hip.
int ensure_dynamic_lds(const void *kernel, size_t bytes, std::atomic<uint64_t> &done);

// host_math.cpp
void make_twiddles(uint32_t n, int direction, std::vector<double> &out);
void make_twiddles_rounded(uint32_t n, int direction, std::vector<double> &out); // the same row, every entry correctly rounded
int design_lp(uint32_t m, double f0, double fs, double gain_in, double *a, double *b, double *gain);
int design_hp(uint32_t m, double f0, double fs, double gain_in, double *a, double *b, double *gain);
int design_bp(uint32_t m, double f0, double fs, double q, double gain_in, double *a, double *b, double *gain);
int design_bs(uint32_t m, double f0, double fs, double q, double gain_in, double *a, double *b, double *gain);
int design_fir(uint32_t taps, int filter_type, double f0, double fs, double q, double gain_in, double *h);
int preload(uint32_t m, int filter_type, const double *a, const double *b, double gain, double value,
            double *mem);
// s[0..m]: s_0 = gain, s_{j+1} = s_j (1 + b1_j + b2_j) / (1 + a1_j + a2_j), the folded numerators for LP / HP / BP
int iir_steady_state(uint32_t m, int kind, const double *a, const double *b, double gain, double *s);
// scipy.signal.sosfiltfilt's default edge: 3 (2 m + 1 - min(#{b2_j == 0}, #{a2_j == 0}))
int filtfilt_default_padlen(uint32_t m, int kind, const double *a, const double *b, uint32_t *padlen);

// ------------------------------------------------------------------------------------------
// FFT: one "tile" launch = every workgroup transforms `cols` independent length-n sequences held
// in LDS.  The same kernel serves contiguous batches (cols transforms per workgroup) and the two
// HBM passes of the four-step decomposition for transforms larger than LDS.
struct fft_tile_args {
    const void *in;
    void *out;
    const void *tw;     // W_n^j, j in [0,n): direction already folded in (conjugated for reverse)
    const void *tw_big; // four-step pass 1: W_N^j, j in [0,N) of the whole transform; else null
    uint32_t n;         // sub-transform length held in LDS
    uint32_t log2n;
    uint32_t cols;      // sequences per workgroup
    uint32_t pitch;     // LDS row pitch in complex elements (cols + padding)
    uint64_t total_cols;       // sequences in the whole launch (ragged last tile is masked)
    uint32_t tiles_per_group;  // tiles that make up one big transform (1 for contiguous batches)
    uint64_t group_stride;     // elements between big transforms
    uint64_t in_tile_step, out_tile_step;   // element offset between consecutive tiles of a group
    uint64_t in_si, in_sc;     // input strides: sequence index i, column c
    uint64_t out_sk, out_sc;   // output strides: frequency index k, column c
    uint32_t in_c_fast, out_c_fast; // which index runs fastest over the lanes (coalescing)
    uint32_t reverse;          // direction of the +-i rotation (twiddles are pre-conjugated)
    uint32_t apply_scale;      // multiply by `scale` on store (reverse_fft::ScaleValues)
    float scale;               // 1/N
    double scale_d;
};

int launch_fft_tile(int precision, int radix, const fft_tile_args &a, uint64_t n_tiles, void *stream);
size_t fft_tile_lds_bytes(int precision, uint32_t n, uint32_t pitch);
size_t fft_tile_max_lds_bytes();

// fast path: batched n = 4096, radix 4, f32 (BASELINE config 2 / 5)
struct fft4096_args {
    void *data;
    const void *tw; // the plan's thread-twiddle table (make_thread_twiddles_4096), f32 complex
    uint64_t batch;
    float scale;
    int reverse;
};
int launch_fft4096_r4_f32(const fft4096_args &a, int variant, void *stream);
int fft4096_num_variants();
int launch_fft4096_r2_f32(const fft4096_args &a, void *stream); // tuned radix-2 sibling
// fused y = IFFT(FFT(x) .* h), n = 4096, f32; tw = FORWARD thread-twiddle table
int launch_fft4096_conv_f32(void *data, const void *tw, const void *h, uint64_t batch, void *stream);
// data[b][i] *= h[i] (generic three-launch convolution path)
int launch_pointwise_mul(int precision, void *data, const void *h, uint32_t n, uint64_t batch, void *stream);

// fast path for every other batched f32 size 16 .. 4096, radix 2 or 4 (register-pass family)
struct fft_reg_args {
    void *data;
    const void *tw; // fft_reg.hip (f32): the plan's thread-twiddle table; fft_reg64 / fft_big: the row W_n^j
    uint32_t n;
    int radix;
    uint64_t batch;
    float scale;
    double scale_d = 1.0;      // f64 kernels
    int reverse;
    int nontemporal;
    int real_mode = 0;         // 0 complex; 1 real forward (split); 2 real inverse (merge): SURVEY 8(f)-3
    const void *tw2 = nullptr; // real modes: W_{2n}^k
};
bool fft_reg_supports(uint32_t n, int radix);
int launch_fft_reg_f32(const fft_reg_args &a, void *stream);
bool fft_reg64_supports(uint32_t n, int radix); // f64 family: 16 .. 8192
int launch_fft_reg_f64(const fft_reg_args &a, void *stream);
// N = 8192 / 16384 / 32768, radix 2, f32: transform held in registers, LDS only for the exchanges (fft_big.hip)
// N = 1024 f32, one transform per wave (fft_wave.hip); a.tw = the register-pass thread-twiddle table
bool fft_wave_supports(uint32_t n, int radix);
int launch_fft_wave_f32(const fft_reg_args &a, void *stream);
int launch_fft_wave_f64(const fft_reg_args &a, void *stream); // scale_d
// N = 256 / 512 / 2048 f32, radix-2 stages: 1024 points (or one transform of 2048) per wave; a.tw = twt_wave
bool fft_wave2_supports(uint32_t n, int radix);
int launch_fft_wave2_f32(const fft_reg_args &a, void *stream);
bool fft_big_supports(uint32_t n, int radix);
bool fft_big_real_supports(uint32_t n, int radix); // real-input plans, n = n_real / 2
bool fft_big_conv_supports(uint32_t n, int radix); // fused convolution
int launch_fft_big_f32(const fft_reg_args &a, void *stream);
// the same design in double: N = 4096 / 8192 / 16384, radix-2 stages (fft_big64.hip); a.tw = the [pass][stage][thread] table in double
bool fft_big64_supports(uint32_t n, int radix);
bool fft_big64_real_supports(uint32_t n, int radix); // the real-input form (real_mode = 1 / 2, W_2N in tw2)
bool fft_big64_conv_supports(uint32_t n, int radix); // the fused convolution form (launch_fft_big_f64 with real_mode = 3, h in tw2)
int launch_fft_big_f64(const fft_reg_args &a, void *stream);

// N = 8192 / 16384, f32: one leading radix-2 / radix-4 stage + the tuned N = 4096 radix-4 machinery (fft_mix.hip)
struct fft_mix_args {
    void *data;
    const void *tw;      // sub-transform thread-twiddle table (layout of the N = 4096 radix-4 kernel's)
    const void *tw_lead; // [q - 1][t] = W_N^(q t), q < R, t < 256
    uint32_t n;
    uint64_t batch;
    float scale;
    int reverse;
};
bool fft_mix_supports(uint32_t n);
int launch_fft_mix_f32(const fft_mix_args &a, void *stream);

// N = 2^16 .. 2^19, f32: two passes over HBM, N = N1 x N2 with N1, N2 in {256, 512, 1024} (fft_2pass.hip)
struct fft_2pass_args {
    void *data;          // count x n complex, in place
    void *workspace;     // count x n complex
    const void *tw_1024; // W_1024^j, direction-folded
    uint32_t n;
    uint64_t count;
    float scale;
    int reverse;
    double scale_d = 1.0; // f64
    const void *hmul = nullptr; // forward only: every output X[k] leaves multiplied by hmul[k] (the fused convolution's forward half)
};
bool fft_2pass_supports(uint32_t n, int precision);
int launch_fft_2pass(int precision, const fft_2pass_args &a, void *stream);

// N = 2^16 .. 2^19, f32 (variant 1) and larger / f64: the two streaming passes around 16 x batch row transforms (fft_mid.hip)
int launch_fft_mid_cols(int precision, const void *in, void *out, const void *tw, uint32_t n2, uint64_t batch, int reverse,
                        void *stream);
int launch_fft_mid_untwist(int precision, const void *in, void *out, uint32_t n2, uint64_t batch, void *stream);

// fast path: batched n = 2^20, radix 2, f32 (BASELINE config 3), one chunk of transforms
struct fft1m_args {
    void *data;          // count x 2^20 complex, in place
    void *workspace;     // count x 2^20 complex
    const void *tw_n;    // W_N^j, j < 1024 used
    const void *tw_1024; // W_1024^j
    uint64_t count;
    float scale;
    int reverse;
};
int launch_fft1m_pass(const fft1m_args &a, int which, void *stream); // which = 1 columns pass, 2 rows pass (variant 1)
// the default schedule: ONE persistent launch over `count` transforms (fft1m_kernels.h)
struct fft1m_fused_args {
    void *data;          // count x 2^20 complex, in place
    void *workspace;     // ring x 2^20 complex
    const void *tw_1024; // W_1024^j
    void *sync;          // fft1m_sync_bytes(count) bytes of device memory (zeroed by the launcher)
    void *sticky = nullptr;  // one word outside that block, or null: set to 1 by a launch that gave up, never cleared by the launcher
    uint64_t spin_limit = 200000000ull; // wall_clock64 ticks (100 MHz) a hand-off poll may take: 2 s
    uint64_t count;
    uint32_t ring, lag;  // intermediate ring slots per queue; steps pass 2 trails pass 1 (lag < ring)
    uint32_t queues;     // independent ticket queues (workspace holds queues x ring transforms)
    float scale;
    int reverse;
};
size_t fft1m_sync_bytes(uint64_t count, uint32_t queues);
int launch_fft1m_fused(const fft1m_fused_args &a, void *stream);

// the two-pass sizes of fft_2pass.hip in ONE persistent, ticketed launch (the schedule of launch_fft1m_fused; handoff.h)
struct fft_2pass_fused_args {
    void *data;          // count x n complex, in place
    void *workspace;     // queues x ring x unit transforms
    const void *tw_1024; // W_1024^j
    void *sync;          // fft_2pass_sync_bytes(units, queues) bytes of device memory (zeroed by the launcher)
    void *sticky = nullptr;  // one word outside that block, or null: set to 1 by a launch that gave up
    uint64_t spin_limit = 200000000ull; // wall_clock64 ticks (100 MHz) a hand-off poll may take: 2 s; 0 = fault injection
    uint64_t count;
    uint32_t n;
    uint32_t unit;       // transforms per ticket step
    uint32_t ring, lag;  // ring slots (units) per queue; steps pass 2 trails pass 1 (lag < ring)
    uint32_t queues;
    float scale;
    double scale_d;
    int reverse;
    const void *hmul = nullptr; // forward only: every output X[k] leaves multiplied by hmul[k]
};
size_t fft_2pass_sync_bytes(uint64_t units, uint32_t queues);
void fft_2pass_fused_shape(uint32_t n, int precision, uint32_t *unit, uint32_t *queues, uint32_t *ring, uint32_t *lag);
int launch_fft_2pass_fused(int precision, const fft_2pass_fused_args &a, void *stream);

// ------------------------------------------------------------------------------------------
// IIR bank
struct iir_args {
    void *data;
    void *state; // nullable
    uint64_t channels, samples, stride;
    uint32_t sections;
    int kind;
    // coefficients in double; kernels round to their precision
    double gain;
    double a1[SDSP_HIP_MAX_SECTIONS], a2[SDSP_HIP_MAX_SECTIONS];
    double b1[SDSP_HIP_MAX_SECTIONS], b2[SDSP_HIP_MAX_SECTIONS];
};
int launch_iir(int precision, const iir_args &a, int variant, void *stream);
// the kernel launch_iir would run for this shape and variant (iir.hip: iir_select -- the same function the launcher uses)
const char *iir_kernel_for(int precision, const iir_args &a, int variant);
int launch_iir_interleaved(int precision, const iir_args &a, int variant, void *stream);
// zero-phase forward-backward filtering (iir_filtfilt.hip): one launch per workspace slice
struct filtfilt_args {
    void *data; // the slice's first row
    void *ws;   // ceil(channels / 64) * 64 * padlen samples; null when padlen = 0
    uint64_t channels, samples, stride;
    uint32_t sections, padlen;
    int kind, padtype;
    double gain;
    double a1[SDSP_HIP_MAX_SECTIONS], a2[SDSP_HIP_MAX_SECTIONS];
    double b1[SDSP_HIP_MAX_SECTIONS], b2[SDSP_HIP_MAX_SECTIONS];
    double ss[SDSP_HIP_MAX_SECTIONS + 1]; // steady state per level (host_math.cpp: iir_steady_state)
};
int launch_filtfilt(int precision, const filtfilt_args &a, int variant, void *stream);
// the kernel launch_filtfilt runs for this shape and variant (the same selection function)
const char *filtfilt_kernel_for(int precision, const filtfilt_args &a, int variant);

// FIR bank
struct fir_args {
    void *data;
    void *state;   // nullable; channels x (taps-1), newest first
    const void *h; // device, plan precision, `taps` values
    uint64_t channels, samples, stride;
    uint32_t taps;
};
int launch_fir(int precision, const fir_args &a, int variant, void *stream);

// FFT-domain FIR plans (overlap-save, fir_fft.hip): the launches of one slice around the convolution
enum { FIR_OS_FRAME = 0, FIR_OS_SCATTER = 1, FIR_OS_STATE = 2 };
struct fir_os_args {
    void *data;
    void *state;          // nullable; channels x (taps-1), newest first
    void *ws;             // units x n complex (frame pairs)
    void *tails;          // staged new history: (taps-1) per channel whose last unit is in the slice; null without state
    const void *carry_in; // the previous slice's carry (the straddling channel's taps-1 inputs), ...
    void *carry_out;      // ... and this slice's
    uint64_t stride, samples, frames, pairs, g0, units;
    uint32_t n, hop, taps_m1;
};
int launch_fir_os(int precision, const fir_os_args &a, int step, void *stream);

// polyphase FIR resampler banks (fir_resample.hip): up by `up`, filter, down by `down`, out of place
struct resample_args {
    const void *in;
    void *out;
    void *state;   // nullable; channels x floor((taps-1)/up), newest first
    const void *h; // device, plan precision, `taps` values
    uint64_t channels, samples, in_stride, out_stride; // samples: a multiple of down / gcd(up, down)
    uint32_t taps, up, down;
};
int launch_resample(int precision, const resample_args &a, int variant, void *stream);
// the kernel launch_resample runs for this shape and variant (the same selection function)
const char *resample_kernel_for(int precision, const resample_args &a, int variant);
// carried state of the streaming banks (stream_carry.hip).  elem_bytes: one real or one interleaved complex
// value of `precision`; `family` labels the error messages ("<family> state too large for one launch", "<family> launch: ...").
// Both return at once for hist = 0, a null state or no channels.
// after a call's last frame launch: state (channels x hist, newest first) = the last hist elements of old history + in[.., :samples]
int carry_history(int precision, uint32_t elem_bytes, const void *in, uint64_t in_stride, void *state, uint64_t channels,
                  uint64_t samples, uint32_t hist, void *stream, const char *family);
// before a call's first slice: the pending sums (channels x hist, time order) of the call's first min(hist, samples) positions go to
// out, the rest move to the front of their row
int carry_seed(int precision, uint32_t elem_bytes, void *out, uint64_t out_stride, void *state, uint64_t channels, uint64_t samples,
               uint32_t hist, void *stream, const char *family);
// digital down-converter banks (ddc.hip): the one launch of a call, in front of carry_history
struct ddc_args {
    const void *in;
    void *out;
    const void *state;     // nullable; channels x (taps - 1) elements of the input kind, newest first
    const void *g;         // device, plan precision: [band in table order][tap] interleaved complex band taps
    const void *coarse;    // device, plan precision: C[a], F[b], 65536 interleaved complex values each
    const void *fine;
    const uint32_t *csr;   // device: channels + 1 offsets into the table (the bands sorted by src)
    const uint32_t *bands; // device: 4 words per band in table order: output row, src, fcw, phase0
    uint64_t samples, in_stride, out_stride, position;
    uint32_t taps, down, channels, nb;
    int complex_in;
};
int launch_ddc(int precision, const ddc_args &a, int variant, void *stream);
const char *ddc_kernel_for(int variant);
// once per device and instantiation, at plan creation: the fused kernel's dynamic-LDS limit, large enough for every plan
int ddc_prepare(int precision, int complex_in);
// outputs per band and LDS block of sdsp_ddc_kernel for these sizes
uint32_t ddc_block_out(int precision, int complex_in, uint32_t taps, uint32_t down);
// digital up-converter banks (duc.hip): the one launch of a call, in front of carry_history
struct duc_args {
    const void *in;        // nb rows of interleaved complex elements
    void *out;             // channels rows: interleaved complex, or reals when real_out
    const void *state;     // nullable; nb x floor((taps - 1) / up) complex elements, newest first
    const void *h;         // device, plan precision, `taps` values
    const void *coarse;    // device, plan precision: the DDC's C[a], F[b], 65536 interleaved complex values each
    const void *fine;
    const uint32_t *csr;   // device: channels + 1 offsets into the table (the bands sorted by dst)
    const uint32_t *bands; // device: 4 words per band in table order: input row, dst, fcw, phase0
    uint64_t samples, in_stride, out_stride, position;
    uint32_t taps, up, channels, nb;
    int real_out;
};
int launch_duc(int precision, const duc_args &a, int variant, void *stream);
const char *duc_kernel_for(int variant);
// once per device and instantiation, at plan creation: the fused kernel's dynamic-LDS limit, large enough for every plan
int duc_prepare(int precision, int real_out);
// input positions per workgroup of sdsp_duc_kernel for these sizes
uint32_t duc_block_in(int precision, uint32_t taps, uint32_t up);
// arbitrary-ratio resampler banks (arb_resample.hip): the one launch of a call with n_out > 0, in front of
// carry_history
struct arb_args {
    const void *in;
    void *out;
    const void *state;  // nullable; channels x (taps - 1) elements of the input kind, newest first
    const void *table;  // device, plan precision: [phase][tap] values H (nearest) or pairs (H, Dt) (linear)
    uint64_t channels, samples, in_stride, out_stride;
    uint64_t step, time, n_out; // n_out in [1, 2^31): sdsp_hip_arb_out_samples of step, time, samples
    uint32_t phases, taps;
    uint32_t block_out; // the plan's: arb_block_out at its max_step
    int complex_in, linear;
};
int launch_arb(int precision, const arb_args &a, int variant, void *stream);
const char *arb_kernel_for(int variant);
// once per device and instantiation, at plan creation: the fused kernel's dynamic-LDS limit, large enough for every plan
int arb_prepare(int precision, int complex_in, int linear);
// outputs per workgroup and staged span of sdsp_arb_kernel for these sizes, computed once per plan; 0: the line of one output does
// not fit (no plan within the documented limits)
uint32_t arb_block_out(int precision, int complex_in, int linear, uint32_t phases, uint32_t taps, uint64_t max_step);
// CIC decimator banks (cic.hip): the one launch of a call with n_out > 0, in front of carry_history
struct cic_args {
    const void *in;
    void *out;
    const void *state; // nullable; channels x hist elements of the input kind and type, newest first
    const void *taps;  // device, order * (down * delay - 1) + 1 values of 64 bits (variant 1 only)
    uint64_t channels, samples, in_stride, out_stride;
    uint64_t position, n_out; // n_out in [1, 2^31): sdsp_hip_cic_out_samples of down, position, samples
    uint32_t order, down, delay;
    uint32_t segment;  // chunks per workgroup of the fused kernel, 0 = automatic
    int in32, complex_in, reg64, out_f32;
    double scale;
};
int launch_cic(const cic_args &a, int variant, void *stream);
const char *cic_kernel_for(int variant);
// input elements one workgroup of sdsp_cic_kernel scans per pass
uint32_t cic_chunk();
// CIC interpolator banks (cic_interp.hip): the one launch of a call, in front of carry_history
struct cic_interp_args {
    const void *in;
    void *out;
    const void *state; // nullable; channels x order * delay elements of the input kind and type, newest first
    const void *taps;  // device, order * (up * delay - 1) + 1 values of 64 bits (variant 1 only)
    uint64_t channels, samples, in_stride, out_stride; // samples * up in [1, 2^31)
    uint32_t order, up, delay;
    uint32_t segment;  // chunks of output per workgroup of the scan kernel, 0 = automatic
    int in32, complex_in, reg64, out_f32;
    double scale;
};
int launch_cic_interp(const cic_interp_args &a, int variant, void *stream);
const char *cic_interp_kernel_for(int variant);
// outputs one workgroup of sdsp_cic_interp_kernel scans per pass
uint32_t cic_interp_chunk();
// time-delay beamformer banks (beam.hip): the one launch of a call, in front of carry_history
struct beam_layout {
    uint32_t chunks = 0;         // chunks of consecutive beams
    uint32_t max_spread = 0;     // the widest delay spread on one sensor a chunk may have
    uint32_t line_elems = 0;     // elements of the plan's widest staged sensor window (before the pad)
    uint32_t lds_line_bytes = 0; // ... as one padded LDS line
    uint32_t off_beams = 0, off_chunks = 0, off_recs = 0; // word offsets into the table
};
struct beam_args {
    const void *in;
    void *out;
    const void *state;     // nullable; groups x sensors x hist elements of the kind, newest first
    const void *g;         // device, plan precision: [entry][tap] taps (interleaved pairs for complex)
    const uint32_t *table; // device: the plan's table (beam_build_table)
    beam_layout lay;
    uint64_t samples, in_stride, out_stride;
    uint32_t taps, hist, sensors, beams, groups;
    int complex_in;
};
// the plan's device table from its checked entries: 3 words per entry (beam, sensor, delay); beams + 1 offsets of each beam's entries;
// 4 words per chunk (first beam, beams, first record, records); 8 words per record = one sensor a chunk uses (sensor, smallest and
// largest delay of the chunk's beams on it, 0, then per beam of the chunk its entry or 0xffffffff)
void beam_build_table(int precision, int complex_in, uint32_t taps, uint32_t beams, uint32_t n_entries, const sdsp_hip_beam_entry *entries,
                      std::vector<uint32_t> &table, beam_layout &lay);
int launch_beam(int precision, const beam_args &a, int variant, void *stream);
const char *beam_kernel_for(int variant);
// once per device and instantiation, at plan creation: the fused kernel's dynamic-LDS limit, large enough for every plan
int beam_prepare(int precision, int complex_in);
// outputs per beam one workgroup of sdsp_beam_kernel produces
uint32_t beam_block_out();
// LMS / NLMS adaptive filter banks (lms.hip): the one launch of a call, in front of carry_history
struct lms_args {
    const void *x, *d;
    void *y, *e;      // nullable: not written
    void *w;          // nullable for variant 0 (zero weights, nothing kept); channels x taps elements of the kind, [channel][tap]
    const void *hist; // nullable; channels x (taps - 1) elements of x, newest first
    uint64_t channels, samples, x_stride, d_stride, y_stride, e_stride;
    uint32_t taps;
    int complex_in, nlms;
    double mu, eps; // already rounded to the plan precision
};
int launch_lms(int precision, const lms_args &a, int variant, void *stream);
const char *lms_kernel_for(int variant);
// samples per time block of sdsp_lms_kernel and its LDS bytes per workgroup (one wave), for this kind, precision and tap count
uint32_t lms_block(int precision, int complex_in, uint32_t taps);
uint32_t lms_lds_bytes(int precision, int complex_in, uint32_t taps);
// rank-order filter banks (rank_filter.hip): the one launch of a call, in front of carry_history
struct rank_args {
    const void *x;
    void *y;
    const void *hist; // nullable; channels x (window - 1) elements of x, newest first
    uint64_t channels, samples, x_stride, y_stride;
    uint32_t window, rank;
    uint32_t run; // outputs per lane of sdsp_rank_kernel, 1 .. samples (unused by the plain kernel)
};
int launch_rank(int precision, const rank_args &a, int variant, void *stream);
const char *rank_kernel_for(int variant);
// the sorted array's compile-time size for a window, the samples per staging block and the LDS bytes per workgroup (one wave) of
// sdsp_rank_kernel, and the run it takes by default for a call's shape
uint32_t rank_padded(uint32_t window);
uint32_t rank_block(int precision);
uint32_t rank_lds_bytes(int precision);
uint32_t rank_auto_run(int precision, uint64_t channels, uint64_t samples, uint32_t window);
// CFAR detector banks (cfar.hip): the one launch of a call, in front of carry_history
struct cfar_args {
    const void *x;
    void *thr, *det;  // nullable: not written (det: bytes)
    const void *hist; // nullable; channels x 2 (train + guard) elements of the input's kind, newest first
    uint64_t channels, samples, x_stride, thr_stride, det_stride;
    uint32_t train, guard, rank;
    int mode, iq;
    double scale; // c of the mode (OS: alpha), rounded to the precision
    uint32_t run; // outputs per workgroup (sum modes) or per lane (OS) of variant 0, 1 .. samples (unused by the plain kernel)
};
int launch_cfar(int precision, const cfar_args &a, int variant, void *stream);
const char *cfar_kernel_for(int variant, int mode);
// the sorted array's compile-time size for 2 L training cells, the block (sum modes: the largest segment; OS: samples per staging
// block) and the LDS bytes per workgroup of the variant-0 kernel, and the run it takes by default for a call's shape
uint32_t cfar_padded(uint32_t cells);
uint32_t cfar_block(int precision, int mode);
uint32_t cfar_lds_bytes(int precision, int mode);
uint32_t cfar_auto_run(int precision, int mode, uint64_t channels, uint64_t samples, uint32_t train, uint32_t guard);
// Carrier-recovery PLL / Costas loop banks (pll.hip): the one launch of a call
struct pll_args {
    const void *x;
    void *y, *err, *freq; // nullable: not written; y may be x
    void *integ;          // channels reals; nullable for variant 0 (zero state, nothing kept)
    uint32_t *theta;      // channels phase words; null with integ
    const uint32_t *fcw0; // channels centre-frequency words
    const void *osc;      // the two oscillator tables of the precision, C then F
    uint64_t channels, samples, x_stride, y_stride, err_stride, freq_stride;
    int mode;
    double alpha, beta, max_dev; // already rounded to the plan precision
};
int launch_pll(int precision, const pll_args &a, int variant, void *stream);
const char *pll_kernel_for(int variant);
// samples per time block, waves per workgroup and LDS bytes per workgroup of sdsp_pll_kernel
uint32_t pll_block(int precision);
uint32_t pll_waves(int precision);
uint32_t pll_lds_bytes(int precision);
// Symbol-timing recovery banks (timing.hip): the one launch of a call
struct timing_args {
    const void *x;
    void *y, *err, *period; // err and period nullable: not written
    uint32_t *counts;       // channels words: each channel's symbols of this call
    // the arrays of the state buffer, all null for variant 0 without state (zero state, nothing kept)
    uint64_t *time;         // channels Q32.32 stream times
    void *ps, *ym;          // channels complex values each
    void *integ;            // channels reals
    int32_t *w;             // channels advance words
    uint32_t *parity;       // channels words, 0 or 1
    void *hist;             // channels x (taps - 1) complex values, newest first
    const void *table;      // [phase][tap] reals of the precision
    uint64_t channels, samples, x_stride, y_stride, err_stride, period_stride, step0;
    uint64_t cap;           // sdsp_hip_timing_max_out of samples: no row is written at or past it
    uint32_t phases, taps;
    int mode;
    double alpha, beta, max_dev; // already rounded to the plan precision
};
int launch_timing(int precision, const timing_args &a, int variant, void *stream);
const char *timing_kernel_for(int variant);
// samples per input block, waves per workgroup and LDS bytes per workgroup of sdsp_timing_kernel
uint32_t timing_block(int precision);
uint32_t timing_waves(int precision, uint32_t phases, uint32_t taps);
uint32_t timing_lds_bytes(int precision, uint32_t phases, uint32_t taps);
// Column FFT plans (fft_cols.hip): the launches of one call over compact cubes [batch][n][width]
struct fft_cols_args {
    const void *in;     // null: launch nothing, only prepare the kernel (its dynamic-LDS limit) on the current device
    void *out;          // complex elements, or reals for `power`; may equal `in` for complex output
    const void *tw;     // W_n^j, j < n, direction-folded, plan precision
    const void *window; // nullable; n reals of the plan precision (forward only)
    uint64_t width, batch;
    uint32_t n;
    int reverse, power, shift;
};
int launch_fft_cols(int precision, const fft_cols_args &a, int variant, void *stream);
struct fft_cols_shape {
    uint32_t tile_columns; // columns of one tile
    uint32_t columns;      // columns of one workgroup (tiles side by side)
    uint32_t threads, lds_bytes;
};
fft_cols_shape fft_cols_shape_for(int precision, uint32_t n, int variant);
uint64_t fft_cols_launches(int precision, uint32_t n, uint64_t width, uint64_t batch, int variant);
const char *fft_cols_kernel_for(int variant);
// 2-D CFAR plans (cfar2d.hip): the launches of one call over compact maps [maps][D][R]
struct cfar2d_args {
    const void *p;       // null: launch nothing, only prepare the kernel (its dynamic-LDS limit) on the current device
    void *thr;           // nullable
    uint8_t *det;        // nullable
    void *hits;          // nullable: maps x cap records of the precision
    uint32_t *counts;    // with hits: maps totals
    const void *scale;   // device: R values c(r) of the plan precision
    void *ws_mask;       // the plan's workspace (cfar2d_workspace)
    uint32_t *ws_cnt;
    uint64_t maps, cap;
    uint32_t D, R, Ld, Gd, Lr, Gr;
    int clip, peak;
};
int launch_cfar2d(int precision, const cfar2d_args &a, int variant, void *stream);
struct cfar2d_shape {
    uint32_t tile_rows, tile_cols, threads, lds_bytes;
};
cfar2d_shape cfar2d_shape_for(int precision, uint32_t D, uint32_t Ld, uint32_t Gd, uint32_t Lr, uint32_t Gr, int variant);
void cfar2d_workspace(uint32_t D, uint32_t R, uint64_t max_maps, uint64_t *mask_bytes, uint64_t *cnt_bytes);
uint64_t cfar2d_launches(int variant, bool maps_out, bool list);
const char *cfar2d_kernel_for(int variant);
// Viterbi decoder banks (viterbi.hip): the one launch of a call over compact rows
struct viterbi_args {
    const void *in; // null: launch nothing, only prepare the kernels (their dynamic-LDS limit) on the current device
    void *out;
    uint32_t *metrics; // the plan's state: max_channels x S path metrics,
    uint32_t *filled;  // max_channels counts of the steps held, at most Dr,
    uint64_t *hist;    // max_channels x Dr x max(1, S / 64) decision words, oldest step first
    uint64_t *ring_ws; // nullable: the plain kernel's ring where it does not fit LDS (viterbi_shape::ring_in_lds == 0)
    uint64_t channels, steps;
    uint32_t k, n, generators[3], block, depth, dr;
    int in_kind, out_kind;
    float scale;
};
int launch_viterbi(const viterbi_args &a, int variant, void *stream);
struct viterbi_shape {
    uint32_t threads, waves, chunk, ring_steps, lds_bytes, ring_in_lds;
    uint32_t wave_bytes, q_off, outw_off; // the LDS of one wave of the wave kernel and its parts
};
viterbi_shape viterbi_shape_for(uint32_t k, uint32_t n, uint32_t block, uint32_t dr, int variant);
const char *viterbi_kernel_for(int variant);
// Reed-Solomon decoder banks (rs.hip): the one launch of a call over compact frames
struct rs_args {
    const void *in;
    void *out;            // == in: in place
    const void *erasures; // nullable
    int32_t *corrected;   // nullable
    const void *table;    // device: exp[512] (alpha^i, twice round), log[256]
    uint64_t frames;
    uint32_t n, nroots, interleave, fcr, prim;
    bool data_only;
};
int launch_rs(const rs_args &a, int variant, void *stream);
struct rs_shape {
    uint32_t threads, waves, lds_bytes;
    uint32_t image; // wave kernel: LDS bytes of one staged frame
};
rs_shape rs_shape_for(uint32_t n, uint32_t interleave, int variant);
const char *rs_kernel_for(int variant);
// LDPC decoder banks (ldpc.hip): the launches of one call over compact codewords
struct ldpc_args {
    const void *llr;
    void *bits;        // nullable
    int16_t *post;     // nullable
    int32_t *status;   // nullable
    const void *table; // device uint32: rowptr[0 .. mb], padding to an even count, then per entry (first variable of the column, shift)
    uint32_t table_entries_at; // where the entries start, in uint32
    void *workspace;   // variant 1: L (int16) and R (int8) of one piece, codeword-minor
    uint64_t codewords;
    uint32_t mb, nb, z, edges; // edges per codeword
    uint32_t norm, beta, max_iter, out_bits;
    bool early_stop, packed, f32;
    float scale;
};
int launch_ldpc(const ldpc_args &a, int variant, void *stream);
struct ldpc_shape {
    uint32_t threads, waves, lds_bytes;
    uint32_t group;      // wave kernel: codewords per wave
    uint32_t wave_bytes; // wave kernel: LDS of one wave
    uint32_t per_cu;     // wave kernel: codewords a CU holds at a time
    uint64_t piece;      // codewords of one launch
    uint64_t workspace_bytes; // variant 1
};
ldpc_shape ldpc_shape_for(uint32_t mb, uint32_t nb, uint32_t z, uint32_t edges, int variant);
int ldpc_prepare(int in_kind, uint32_t lds_bytes);
const char *ldpc_kernel_for(int variant);
// frame synchroniser banks (fsync.hip): the launches of one call over compact rows; the kernels take it as it is
struct fsync_args {
    const void *in; // BYTES: channels x nbits bytes; PACKED: channels x nbits / 32 words
    uint8_t *out;   // nullable: channels x maxf x P
    uint32_t *counts;
    uint64_t *pos;  // nullable
    uint32_t *info; // nullable
    uint32_t *state; // the plan's state: max_channels records of 16 words,
    uint32_t *ring;  // then max_channels x HW words of the stream's last bits
    uint32_t *work, *hitn, *hiti; // variant 0's workspace: channels x RW words each: the working row and a hit word per polarity,
    uint64_t *ws_seen;            // the bits seen in front of the call,
    uint64_t *rec_pos;            // and the call's frame records, channels x maxf
    uint32_t *rec_info, *rec_cnt;
    const uint32_t *pnw; // nullable: the pn sequence as ceil(P / 4) words, zero behind byte P
    uint64_t channels, nbits, maxf;
    uint32_t M, P, L, tol, V, F, either, packed, HW, RW;
    uint32_t mrev_lo, mrev_hi; // the marker with its first bit lowest
};
int launch_fsync(const fsync_args &a, int variant, void *stream);
uint32_t fsync_ring_words(uint32_t M, uint32_t P);                  // HW = ceil((L + M) / 32) + 1
uint64_t fsync_row_words(uint32_t M, uint32_t P, uint64_t nbits);   // RW: ring, the call's words, two zero words; even
uint64_t fsync_launches(int variant);
const char *fsync_kernel_for(int variant);
// STFT banks (stft.hip): the launches of one slice around the plan's real-input transform
enum { STFT_FRAME = 0, STFT_EMIT = 1 };
struct stft_args {
    const void *in;
    void *out;
    const void *state;  // nullable; channels x hist, newest first
    const void *window; // device, plan precision, n values
    void *ws;           // units x n reals (windowed frames, then their packed half spectra)
    uint64_t in_stride, out_stride;
    uint64_t g0;        // the slice: units [g0, g0 + units) of the channel-major (channel, frame) numbering
    uint32_t units, frames, n, hop, hist;
    int output;         // SDSP_HIP_STFT_*
};
int launch_stft(int precision, const stft_args &a, int step, void *stream);
// inverse STFT banks (istft.hip): the launches of one slice around the plan's reverse real-input transform
enum { ISTFT_PACK = 0, ISTFT_OLA = 1 };
struct istft_args {
    const void *in;     // complex bins, plan precision
    void *out;
    void *state;        // nullable; channels x hist, time order
    const void *g;      // device, plan precision, n values: the synthesis window
    void *ws;           // units x n reals (packed half spectra, then their frames)
    uint64_t in_stride, out_stride;
    uint64_t g0;        // the slice: units [g0, g0 + units) of the channel-major (channel, frame) numbering
    uint32_t units, frames, n, hop, hist;
};
int launch_istft(int precision, const istft_args &a, int step, void *stream);
// host_math.cpp: the synthesis window (n doubles) and the range of env[r] = sum_k w[r + k hop]^2; NOLA is checked for NORMALIZED
int istft_synthesis(uint32_t n, uint32_t hop, const double *w, int norm, double *g, double *env_min, double *env_max);
// Welch PSD banks (welch.hip): the launches of one slice around the plan's real-input transform, and finalize
enum { WELCH_FRAME = 0, WELCH_RUN = 1, WELCH_COMBINE = 2, WELCH_FINALIZE = 3 };
struct welch_args {
    const void *in;
    const void *state;  // channels x (n - 1), newest first; null only when no segment reaches into the history
    const void *window; // device, plan precision, n values
    void *ws;           // units x n reals (detrended, windowed segments, then their packed half spectra)
    double *part;       // the slice's run partials: runs x (n / 2 + 1) doubles
    double *acc;        // acc[c acc_stride + k]
    void *out;          // finalize: out[c out_stride + k], plan precision
    uint64_t in_stride, acc_stride, out_stride, channels;
    uint64_t g0;        // the slice: units [g0, g0 + units) of the channel-major (channel, segment) numbering
    uint32_t units, frames, n, hop;
    uint32_t off0;      // x offset of the call's first segment (x = history followed by the block)
    uint32_t run;       // R: segments per run
    int detrend;        // SDSP_HIP_DETREND_*
    double c_edge, c_mid; // finalize: c_k for k = 0, N / 2 and for the bins between
};
int launch_welch(int precision, const welch_args &a, int step, void *stream);
// cross-spectral density banks (csd.hip): the run and combine launches of one slice [ja, jb) of every channel's
// segments, behind the Welch bank's frame launch (WELCH_FRAME with frames = jb - ja, g0 = 0) and the plan's transform; and finalize
enum { CSD_RUN = 0, CSD_COMBINE = 1, CSD_FINALIZE = 2 };
struct csd_args {
    const void *ws;        // [channel][segment of the slice] packed half spectra, n reals each
    const uint32_t *table; // device.  run: `nentries` triples (a, b, dst) in launch order, dst < npairs a pair's index, else npairs +
                           // the channel of an auto entry; finalize: the plan's `npairs` pairs (a, b) in the caller's order
    double *part_xy;       // the slice's run partials of the pairs: [pair][run][n / 2 + 1] complex doubles
    double *part_auto;     // ... and of the auto spectra: [channel][run][n / 2 + 1] doubles
    double *acc_xy;        // acc_xy[i acc_xy_stride + 2 k + {0, 1}]
    double *acc_auto;      // acc_auto[c acc_auto_stride + k]; null without auto spectra (then nentries == npairs)
    void *out;             // finalize: plan precision
    uint64_t acc_xy_stride, acc_auto_stride, out_stride;
    uint32_t nentries, npairs;
    uint32_t frames;       // segments per channel in the slice (jb - ja)
    uint32_t run;          // R: segments per run
    uint32_t n;
    int mode;              // finalize: SDSP_HIP_CSD_*
    double c_edge, c_mid;  // finalize, CROSS: c_k for k = 0, N / 2 and for the bins between
};
int launch_csd(int precision, const csd_args &a, int step, void *stream);
// polyphase filter-bank channelizers (pfb.hip): the fold launch of one rectangle of (channel, frame) units in
// front of the plan's transform
struct pfb_args {
    const void *in;
    const void *state;  // nullable; channels x hist elements, newest first
    const void *taps;   // device, plan precision, p x m reals
    void *dst;          // frame j of channel c at dst + (c dst_cstride + j m - dst_sub) elements
    uint64_t in_stride;
    uint64_t dst_cstride, dst_sub;
    uint64_t c0, nc;    // channels [c0, c0 + nc)
    uint32_t j0, nj;    // frames [j0, j0 + nj) of each
    uint32_t m, p, hop, hist;
    uint32_t shift0;    // TIME: frame j is rotated by (shift0 + j hop) mod m; FRAME: rotate = 0
    int complex_in, rotate;
    int form;           // 0: chosen from hop and m; 1: the plain per-frame form (measurement and cross-checks)
};
int launch_pfb(int precision, const pfb_args &a, void *stream);
// the fold form a plan of these sizes runs: "sliding" where hop divides m, else "plain"
const char *pfb_form_for(uint32_t m, uint32_t hop);
// host_math.cpp: symmetric-window sinc low-pass of `taps` points with cutoff `cutoff` (fraction of Nyquist) and unit DC gain
int windowed_sinc_lowpass(uint64_t taps, double cutoff, int window_kind, double *h);
// polyphase synthesis banks (pfb_synth.hip): the copy of one slice's complex spectra into the workspace (real
// banks pack with ISTFT_PACK), and the unfold launch of one rectangle of (stream, frame) units behind the plan's reverse transform
enum { PFB_SYNTH_COPY = 0, PFB_SYNTH_UNFOLD = 1 };
struct pfb_synth_args {
    const void *in;     // complex bins, plan precision
    void *out;
    void *state;        // nullable; channels x hist elements of the output kind, time order
    const void *taps;   // device, plan precision, p x m reals
    void *ws;           // the slice's rows of m elements: spectra in, v_j after the transform
    uint64_t in_stride, out_stride;
    uint64_t g0;        // the slice: units [g0, g0 + units) of the channel-major (channel, frame) numbering
    uint64_t units;
    uint64_t c0, nc;    // unfold: the rectangle's channels ...
    uint32_t j0, nj;    // ... and frames
    uint32_t frames, m, p, hop, hist;
    uint32_t shift0;    // TIME: (position - hist) mod m
    int complex_out, rotate;
    int form;           // 0: chosen from hop and m; 1: the plain per-position form (measurement and cross-checks)
};
int launch_pfb_synth(int precision, const pfb_synth_args &a, int step, void *stream);
// the unfold form a plan of these sizes runs: "sliding" where hop = m, else "plain"
const char *pfb_synth_form_for(uint32_t m, uint32_t hop);
// host_math.cpp: the minimum-norm dual of the analysis prototype h at hop `hop` (g: p m doubles); INVALID_ARG where none exists
int pfb_dual_prototype(uint32_t m, uint32_t p, uint32_t hop, const double *h, double *g);
} // namespace sdsp_hip
