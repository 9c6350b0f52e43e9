// capi.hip -- the extern "C" boundary declared in include/sdsp_hip.h: plans, launches, host and
// multi-device convenience paths.  Everything that computes goes to the HIP kernels of the other translation units -- the
// transforms (fft_tile, fft4096, fft1m, fft_reg, fft_reg64, fft_big, fft_big64, fft_mix, fft_wave, fft_mid, fft_2pass, fft_cols), the filters
// (iir, iir_filtfilt, fir, fir_fft, fir_resample, arb_resample, cic, cic_interp, ddc, duc, beam, lms, rank_filter, cfar, cfar2d, pll, timing, viterbi, rs, fsync) and the framed banks (stft, istft, welch, pfb, pfb_synth); there is no CPU implementation
// behind these entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <new>
#include <thread>
#include <vector>

#include "sdsp_hip_internal.h"

using namespace sdsp_hip;

int sdsp_hip::ensure_dynamic_lds(const void *kernel, size_t bytes, std::atomic<uint64_t> &done)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess)
        return fail(SDSP_HIP_ERR_HIP, std::string("hipGetDevice: ") + hipGetErrorString(e));
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit)
        return SDSP_HIP_OK;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess)
        return fail(SDSP_HIP_ERR_HIP, std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e));
    done.fetch_or(bit, std::memory_order_release);
    return SDSP_HIP_OK;
}

namespace
{
int hip_fail(hipError_t e, const char *what)
{
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice)
        return fail(SDSP_HIP_ERR_NO_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return fail(SDSP_HIP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr)                          \
    do {                                       \
        hipError_t _e = (expr);                \
        if (_e != hipSuccess)                  \
            return hip_fail(_e, #expr);        \
    } while (0)

int use_device(int device)
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(SDSP_HIP_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= count)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    return SDSP_HIP_OK;
}

size_t esize(int precision) { return precision == SDSP_HIP_F64 ? 16 : 8; }    // one complex element
size_t real_size(int precision) { return precision == SDSP_HIP_F64 ? 8 : 4; } // one real sample (the mixed mode stores floats)

bool ranges_overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a && b && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

bool misaligned(const void *ptr, uint64_t element_bytes) { return reinterpret_cast<uintptr_t>(ptr) % element_bytes != 0; }

// what the out-of-place framed banks ask of their device pointers: in and out apart, and in, out and state (null passes) aligned
// to their element size
int check_out_of_place(const void *in, uint64_t in_bytes, uint64_t in_esize, const void *out, uint64_t out_bytes, uint64_t out_esize,
                       const void *state, uint64_t state_esize, const char *overlap_msg)
{
    if (ranges_overlap(in, in_bytes, out, out_bytes))
        return fail(SDSP_HIP_ERR_INVALID_ARG, overlap_msg);
    if (misaligned(in, in_esize) || misaligned(out, out_esize) || misaligned(state, state_esize))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in, out and state must be aligned to their element size");
    return SDSP_HIP_OK;
}

// The device side of every *_process_host / *_finalize_host call.  Each host buffer gets a device buffer of its size, filled from
// it before the run -- outputs too, so that what lies between and behind their rows keeps what the caller had there -- and the ones
// flagged `copy_back` return after a run that succeeded.  An item whose host pointer is null is absent: its device pointer stays
// null.  Everything is freed when the stage goes out of scope.
struct host_stage {
    struct item {
        const void *host;
        size_t bytes;
        bool copy_back; // `host` is writable where this is set
    };
    const char *family;
    item items[6] = {};
    void *dev[6] = {};
    size_t n = 0;

    host_stage(const char *family_, std::initializer_list<item> list) : family(family_)
    {
        for (const item &it : list)
            items[n++] = it;
    }
    host_stage(const host_stage &) = delete;
    host_stage &operator=(const host_stage &) = delete;
    ~host_stage()
    {
        for (void *d : dev)
            (void)hipFree(d);
    }
    // every allocation, then every copy to the device
    int in()
    {
        hipError_t e = hipSuccess;
        for (size_t i = 0; i < n && e == hipSuccess; i++)
            if (items[i].host)
                e = hipMalloc(&dev[i], items[i].bytes);
        for (size_t i = 0; i < n && e == hipSuccess; i++)
            if (items[i].host)
                e = hipMemcpy(dev[i], items[i].host, items[i].bytes, hipMemcpyHostToDevice);
        return e == hipSuccess ? SDSP_HIP_OK : hip_fail(e, (std::string(family) + " host staging").c_str());
    }
    // the call's result: `rc` of a run that failed (nothing is copied back), else that of the copies back
    int out(int rc)
    {
        hipError_t e = hipSuccess;
        for (size_t i = 0; i < n && !rc && e == hipSuccess; i++)
            if (items[i].host && items[i].copy_back)
                e = hipMemcpy(const_cast<void *>(items[i].host), dev[i], items[i].bytes, hipMemcpyDeviceToHost);
        return e == hipSuccess ? rc : hip_fail(e, (std::string(family) + " host read-back").c_str());
    }
};

// units per workspace slice of a framed plan: what the budget holds, at least one; the kernels count a slice's units in 32 bits
uint64_t slice_units(uint64_t budget, uint64_t unit_bytes)
{
    return std::min<uint64_t>(std::max<uint64_t>(1, budget / unit_bytes), 1ull << 30);
}

// launch granularity, sdsp_hip.h: sdsp_hip_set_launch_piece_bytes
std::atomic<uint64_t> g_piece_bytes{ SDSP_HIP_DEFAULT_PIECE_BYTES };

// units (transforms, channels) per launch for a batch of `units` x `unit_bytes`; a multiple of `multiple`, so that a piece
// boundary never cuts a workgroup's tile
uint64_t piece_units(uint64_t units, uint64_t unit_bytes, uint64_t multiple)
{
    const uint64_t pb = g_piece_bytes.load(std::memory_order_relaxed);
    if (pb == 0 || unit_bytes == 0 || units * unit_bytes <= pb + pb / 2) // a tail under half a piece rides along
        return units;
    const uint64_t u = pb / unit_bytes / multiple * multiple;
    return u ? u : multiple;
}

// round a double table to the plan precision and park it in HBM
int upload_twiddles(const std::vector<double> &w, int precision, void **dev)
{
    const size_t n = w.size() / 2;
    if (precision == SDSP_HIP_F64) {
        HIP_TRY(hipMalloc(dev, n * 16));
        HIP_TRY(hipMemcpy(*dev, w.data(), n * 16, hipMemcpyHostToDevice));
    } else {
        std::vector<float> wf(w.size());
        for (size_t i = 0; i < w.size(); i++)
            wf[i] = (float)w[i];
        HIP_TRY(hipMalloc(dev, n * 8));
        HIP_TRY(hipMemcpy(*dev, wf.data(), n * 8, hipMemcpyHostToDevice));
    }
    return SDSP_HIP_OK;
}

// its sibling for the real tables (windows, taps): n values rounded once, by conversion, to the plan precision.  The HIP error comes
// back as it is, since what a failed creation reports differs by family; *dev is the caller's to free either way.
hipError_t upload_reals(const double *src, size_t n, int precision, void **dev)
{
    const hipError_t e = hipMalloc(dev, n * real_size(precision));
    if (e != hipSuccess)
        return e;
    if (precision == SDSP_HIP_F64)
        return hipMemcpy(*dev, src, n * sizeof(double), hipMemcpyHostToDevice);
    const std::vector<float> f(src, src + n);
    return hipMemcpy(*dev, f.data(), n * sizeof(float), hipMemcpyHostToDevice);
}

// a HIP error of plan creation, as the families with plan-owned workspaces report it: out of memory has a code of its own
int plan_fail(hipError_t e, const char *family)
{
    const std::string what = std::string(family) + " plan";
    return e == hipErrorOutOfMemory ? fail(SDSP_HIP_ERR_NOMEM, what + ": out of device memory") : hip_fail(e, what.c_str());
}

// Thread-twiddle table of the tuned N = 4096 f32 kernels (fft4096.hip): the stage twiddles each thread needs,
// taken from the row W_4096^j (same rounded values) and laid out [value][thread] so the kernel reads them
// with coalesced loads.  radix 4: W^(r t), W^(4 r t) (r = 1..3, t < 256), then W^(16 r rr), W^(64 r rr)
// (rr < 16); radix 2: W^(t << j) (j < 4), then W^((16 rr) << j).
int upload_thread_twiddles_4096(const std::vector<double> &w, int radix, void **dev)
{
    std::vector<float> tab;
    auto put = [&](uint32_t idx) {
        tab.push_back((float)w[2 * idx]);
        tab.push_back((float)w[2 * idx + 1]);
    };
    if (radix == 4) {
        for (uint32_t mult : { 1u, 4u })
            for (uint32_t r = 1; r < 4; r++)
                for (uint32_t t = 0; t < 256; t++)
                    put(mult * r * t);
        for (uint32_t mult : { 16u, 64u })
            for (uint32_t r = 1; r < 4; r++)
                for (uint32_t rr = 0; rr < 16; rr++)
                    put(mult * r * rr);
    } else {
        for (uint32_t j = 0; j < 4; j++)
            for (uint32_t t = 0; t < 256; t++)
                put(t << j);
        for (uint32_t j = 0; j < 4; j++)
            for (uint32_t rr = 0; rr < 16; rr++)
                put((16 * rr) << j);
    }
    HIP_TRY(hipMalloc(dev, tab.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(*dev, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    return SDSP_HIP_OK;
}

// Thread-twiddle table of the register-pass families (fft_reg.hip, fft_reg64.hip): for every pass I that has thread
// twiddles (point stride S = N >> 4(I+1) > 1) and every thread t < N/16 of a transform (r = t mod S,
// unit = r * 16^I): six slots -- radix 2: W^(unit << v), v < 4; radix 4: W^(unit q), W^(4 unit q), q = 1..3.
int upload_thread_twiddles_reg(const std::vector<double> &w, uint32_t n, int radix, int precision, void **dev)
{
    const uint32_t log2n = sdsp_hip_log2(n), T = n / 16, P = (log2n + 3) / 4;
    std::vector<double> tab((size_t)6 * P * T * 2, 0.0);
    for (uint32_t I = 0; I + 1 < P; I++) {
        const uint32_t S = n >> (4 * (I + 1));
        for (uint32_t t = 0; t < T; t++) {
            const uint32_t unit = (t % S) << (4 * I);
            for (uint32_t v = 0; v < 6; v++) {
                uint32_t idx;
                if (radix == 2)
                    idx = v < 4 ? unit << v : 0;
                else
                    idx = v < 3 ? unit * (v + 1) : 4 * unit * (v - 2);
                const size_t o = ((size_t)(6 * I + v) * T + t) * 2;
                tab[o] = w[2 * (size_t)idx];
                tab[o + 1] = w[2 * (size_t)idx + 1];
            }
        }
    }
    return upload_twiddles(tab, precision, dev); // rounds to the plan precision exactly like the row itself
}

// Thread-twiddle table of fft_wave.hip's N = 256 / 512 / 2048 kernels.  Radix 2: [global stage g][lane t] = W^((t mod s_i) << g) for
// the stages of pass i < last (P = n / 64 points per lane, log2 P stages per pass, s_i = n >> (log2 P (i + 1))); the last
// pass has no thread twiddles.
int upload_thread_twiddles_wave(const std::vector<double> &w, uint32_t n, int radix, void **dev)
{
    if (radix == 4) { // N = 256: [pass i < 3][q = 1 .. 3][lane] = W^(q (t mod s_i) 4^i), s_i = 64 >> 2 i
        std::vector<double> tab((size_t)3 * 3 * 64 * 2, 0.0);
        for (uint32_t i = 0; i < 3; i++)
            for (uint32_t q = 1; q < 4; q++)
                for (uint32_t t = 0; t < 64; t++) {
                    const size_t idx = (size_t)q * (t % (64u >> (2 * i))) << (2 * i);
                    const size_t o = ((size_t)(i * 3 + q - 1) * 64 + t) * 2;
                    tab[o] = w[2 * idx];
                    tab[o + 1] = w[2 * idx + 1];
                }
        return upload_twiddles(tab, SDSP_HIP_F32, dev);
    }
    const uint32_t L = sdsp_hip_log2(n), LP = L - 6, NP = (L + LP - 1) / LP;
    std::vector<double> tab((size_t)(NP - 1) * LP * 64 * 2, 0.0);
    for (uint32_t i = 0; i + 1 < NP; i++) {
        const uint32_t sg = n >> (LP * (i + 1));
        for (uint32_t s = 0; s < LP; s++)
            for (uint32_t t = 0; t < 64; t++) {
                const size_t idx = (size_t)(t % sg) << (i * LP + s);
                const size_t o = ((size_t)(i * LP + s) * 64 + t) * 2;
                tab[o] = w[2 * idx];
                tab[o + 1] = w[2 * idx + 1];
            }
    }
    return upload_twiddles(tab, SDSP_HIP_F32, dev);
}

// Thread-twiddle table of fft_big.hip: [pass (A, B)][stage s < 5][thread t < N/32] = W^(t << s) for pass A,
// W^((32 v) << s), v = t mod (N/1024), for pass B.
int upload_thread_twiddles_big(const std::vector<double> &w, uint32_t n, int precision, void **dev)
{
    const uint32_t T = n / 32, vmask = n / 1024 - 1;
    std::vector<double> tab((size_t)10 * T * 2);
    for (uint32_t pass = 0; pass < 2; pass++)
        for (uint32_t s = 0; s < 5; s++)
            for (uint32_t t = 0; t < T; t++) {
                const uint32_t idx = (pass == 0 ? t : 32 * (t & vmask)) << s;
                const size_t o = ((size_t)(pass * 5 + s) * T + t) * 2;
                tab[o] = w[2 * (size_t)idx];
                tab[o + 1] = w[2 * (size_t)idx + 1];
            }
    return upload_twiddles(tab, precision, dev); // rounds to the plan precision exactly like the row itself
}

// Thread-twiddle table of fft_big.hip's radix-4 form (N = 16384 = 4^7 and N = 4096 = 4^6, fft32_r4.h): [slot < 14][thread t < N/32].
// For N = 16384: slots 0-2: W_N^(q t); 3-5: W_4096^(q t); 6, 7: stage 2's pair for the thread's block parity -- (1, W_1024^(2v)) for an
// even block, (W_1024^v, W_1024^(3v)) for an odd one; 8-10: W_256^(q v); 11-13: W_64^(q v); q = 1, 2, 3, v = t mod 16, block = t / 16.
// `w` is the row W_N^j, direction-folded.  tools/model_fft_big_r4.py is the index arithmetic's model.
int upload_thread_twiddles_big_r4(const std::vector<double> &w, uint32_t n, int precision, void **dev)
{
    const uint32_t T = n / 32, R = sdsp_hip_log2(n) - 10; // R = 4 (N = 16384) or 2 (N = 4096); v = t mod 2^R, block = t >> R
    std::vector<double> tab((size_t)14 * T * 2);
    auto put = [&](uint32_t slot, uint32_t t, uint64_t idx) {
        idx %= n;
        tab[((size_t)slot * T + t) * 2] = w[2 * idx];
        tab[((size_t)slot * T + t) * 2 + 1] = w[2 * idx + 1];
    };
    for (uint32_t t = 0; t < T; t++) {
        const uint32_t v = t & ((1u << R) - 1), odd = (t >> R) & 1;
        for (uint32_t q = 1; q <= 3; q++) {
            put(q - 1, t, (uint64_t)q * t);        // W_N^(q t)
            put(2 + q, t, (uint64_t)4 * q * t);    // W_(N/4)^(q t) = W_N^(4 q t)
            put(7 + q, t, (uint64_t)64 * q * v);   // W_(2^(R+4))^(q v) = W_N^(64 q v)    (N = 16384: W_256^(q v))
            put(10 + q, t, (uint64_t)256 * q * v); // W_(2^(R+2))^(q v) = W_N^(256 q v)   (N = 16384: W_64^(q v))
        }
        put(6, t, odd ? (uint64_t)16 * v : 0);             // stage 2 (G = N/16), j < 16: q = 1 (odd block) / none
        put(7, t, (uint64_t)16 * (odd ? 3 : 2) * v);       // j >= 16: q = 3 (odd) / 2 (even)
    }
    return upload_twiddles(tab, precision, dev); // rounds to the plan precision exactly like the row itself
}

// N = 16384 radix-4 plans: fft_big.hip's radix-4 form is variant 0 and the fft_mix.hip kernel variant 1
inline bool big_r4_form(uint32_t n, int radix) { return radix == 4 && (n == 16384 || n == 4096); } // table of the radix-4 form (4096: real-input plans)
// (N = 8192, AUTO plans: fft_big.hip's radix-2 stages measured 76.9-77.9 % against 74.1-76.2 % for the mixed-radix kernel in one
// run once their thread twiddles were fetched ahead of the passes, so they are variant 0 there too and fft_mix.hip variant 1)
inline bool big_is_default(uint32_t n, int radix) { return big_r4_form(n, radix) || n == 8192; }
// f64 radix-2 plans the double-precision registers-resident kernel serves: the variant number that selects it
inline int big64_variant(uint32_t) { return 0; } // 4096: 73.2-73.6 % against 66.5-68.6 % (fft_reg64.hip), one call, round 3

constexpr uint64_t kFft1mQueues = 8, kFft1mRing = 3; // persistent N = 2^20 kernel: ticket queues x intermediates per queue
constexpr uint64_t kFused2pUnitsPerLaunch = 1024; // units (8 - 32 MiB each) one persistent launch covers (sizes the counter block)
constexpr uint64_t kFft1mPerLaunch = 4096; // transforms one persistent launch covers (sizes the counter block)
// Tables of fft_mix.hip (N = R x 4096, R = 2 / 4): the N = 4096 radix-4 thread-twiddle table built from W_4096^j = W_N^(R j),
// and the leading stage's thread twiddles [q - 1][t] = W_N^(q t), q < R, t < 256 (R = 2) / 512 (R = 4).
int upload_thread_twiddles_mix(const std::vector<double> &w, uint32_t n, void **sub, void **lead)
{
    const uint32_t R = n / 4096;
    std::vector<double> w4096(2 * 4096);
    for (uint32_t j = 0; j < 4096; j++) {
        w4096[2 * j] = w[2 * (size_t)(R * j)];
        w4096[2 * j + 1] = w[2 * (size_t)(R * j) + 1];
    }
    if (int rc = upload_thread_twiddles_4096(w4096, 4, sub))
        return rc;
    std::vector<float> tab;
    const uint32_t threads = R == 4 ? 512 : 256; // the N = 16384 kernel runs 512 threads per transform
    for (uint32_t q = 1; q < R; q++)
        for (uint32_t t = 0; t < threads; t++) {
            tab.push_back((float)w[2 * (size_t)(q * t)]);
            tab.push_back((float)w[2 * (size_t)(q * t) + 1]);
        }
    HIP_TRY(hipMalloc(lead, tab.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(*lead, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    return SDSP_HIP_OK;
}

enum fft_path { PATH_NOOP = 0, PATH_TILE = 1, PATH_FFT4096 = 2, PATH_FOUR_STEP = 3, PATH_FFT1M = 4, PATH_REG = 5 };
} // namespace

struct sdsp_hip_fft_plan {
    uint32_t n = 0;
    int radix = 0, direction = 0, precision = 0, device = 0;
    uint64_t max_batch = 0;
    int path = PATH_NOOP;
    int variant = 0;
    void *tw = nullptr;            // W_n (single pass) or W_N (four-step inter-pass twiddle)
    void *tw1 = nullptr;           // four-step: W_n1
    void *tw2 = nullptr;           // four-step: W_n2
    void *twt = nullptr;           // tuned N = 4096 f32 kernels: thread-twiddle table
    void *twt_reg = nullptr;       // register-pass family (f32): thread-twiddle table
    void *twt_big = nullptr;       // fft_big.hip: thread-twiddle table
    void *twt_wave = nullptr;      // fft_wave.hip, N = 256 / 512 / 2048 radix 2: [stage][lane] table
    void *twt_mix = nullptr;       // fft_mix.hip (N = 8192 / 16384): the sub-transforms' thread-twiddle table ...
    void *tw_lead = nullptr;       // ... and the leading stage's thread twiddles W_N^(q t)
    uint32_t n1 = 0, n2 = 0;       // four-step split
    uint32_t cols = 1, pitch = 1;  // tile shape (single pass)
    uint32_t cols1 = 1, pitch1 = 1, cols2 = 1, pitch2 = 1;
    void *workspace = nullptr;
    uint64_t workspace_bytes = 0;
    uint64_t ws_batch = 0;         // transforms the workspace holds (multi-pass paths run in slices)
    uint64_t twiddle_bytes = 0;
    void *host_stage = nullptr;    // device staging buffer of the *_host path
    uint64_t host_stage_bytes = 0;
    void *sync = nullptr;          // persistent two-pass kernels: ticket / arrival counters
    uint64_t sync_count = 0;       // ... units (N = 2^20 f32: transforms) one launch covers
    uint64_t sticky_off = 0;       // ... byte offset of the sticky abort word behind the per-launch block
    uint32_t f2_unit = 0, f2_queues = 0, f2_ring = 0, f2_lag = 0; // fft_2pass.hip's persistent schedule (0 = workspace too small)
    uint64_t wait_limit = 200000000ull; // ... and what a hand-off poll may take (100 MHz ticks: 2 s) before the launch gives up
    sdsp_hip_fft_plan *partner = nullptr; // reverse plan of the generic convolution path (lazy)
    sdsp_hip_fft_plan *mid_rows = nullptr; // N = 2^16 .. 2^19 f32: plan of the 16 row transforms (fft_mid.hip)
    void *tw1024 = nullptr;                // ... and W_1024^j, the coarse factor of its inter-pass twiddle
    int real_mode = 0;                    // 0 complex; 1 real forward; 2 real inverse (n = n_real / 2)
    bool allow_mix = false;               // radix-4 stages behind one leading radix-2 / radix-4 stage may serve this plan
};

struct sdsp_hip_iir_plan {
    uint32_t sections = 0;
    int kind = 0, precision = 0, device = 0, variant = 0;
    double gain = 1.0;
    double a[3 * SDSP_HIP_MAX_SECTIONS] = {};
    double b[3 * SDSP_HIP_MAX_SECTIONS] = {};
};

struct sdsp_hip_fir_plan {
    uint32_t taps = 0;
    int precision = 0, device = 0, variant = 0;
    void *h_dev = nullptr;
    // FFT-domain plans (sdsp_hip_fir_fft_plan_create, fir_fft.hip)
    int method = SDSP_HIP_FIR_DIRECT;
    uint32_t fft_n = 0, hop = 0;
    sdsp_hip_fft_plan *conv = nullptr; // forward radix-2 plan of size fft_n; its variant is the plan's
    void *H = nullptr;                 // FFT(h zero-padded to fft_n), plan precision, fft_n complex
    void *ws = nullptr;                // ws_units x fft_n complex (frame pairs), then ws_units x (taps-1) staged history
    void *carry = nullptr;             // 2 x (taps-1): the straddling channel's inputs, ping-pong between slices
    uint64_t ws_units = 0, workspace_bytes = 0;
};

struct sdsp_hip_resample_plan {
    uint32_t taps = 0, up = 1, down = 1, q = 1, hist = 0; // q = down / gcd(up, down), hist = floor((taps - 1) / up)
    int precision = 0, device = 0, variant = 0;
    void *h_dev = nullptr;
};

struct sdsp_hip_stft_plan {
    uint32_t n = 0, hop = 0, hist = 0, bins = 0; // hist = n - hop, bins = n / 2 + 1
    int output = 0, precision = 0, device = 0;
    sdsp_hip_fft_plan *inner = nullptr; // forward real-input plan of n_real = n, radix 2; its variant is the plan's
    void *window = nullptr;             // n values, plan precision
    void *ws = nullptr;                 // ws_units x n reals: the slice's frames, transformed in place
    uint64_t ws_units = 0, workspace_bytes = 0;
};

struct sdsp_hip_istft_plan {
    uint32_t n = 0, hop = 0, hist = 0, bins = 0; // hist = n - hop, bins = n / 2 + 1
    int norm = 0, precision = 0, device = 0;
    sdsp_hip_fft_plan *inner = nullptr; // reverse real-input plan of n_real = n, radix 2; its variant is the plan's
    void *g = nullptr;                  // the synthesis window: n values, plan precision
    void *ws = nullptr;                 // ws_units x n reals: the slice's packed spectra, transformed in place
    uint64_t ws_units = 0, workspace_bytes = 0;
    double env_min = 0, env_max = 0;
};

struct sdsp_hip_welch_plan {
    uint32_t n = 0, hop = 0, hist = 0, bins = 0; // hist = n - 1, bins = n / 2 + 1
    int detrend = 0, scaling = 0, precision = 0, device = 0;
    double fs = 1.0, scale = 1.0;       // scale: 1 / (fs sum w^2) or 1 / (sum w)^2 over the rounded window
    sdsp_hip_fft_plan *inner = nullptr; // forward real-input plan of n_real = n, radix 2
    void *window = nullptr;             // n values, plan precision
    void *ws = nullptr;                 // ws_units x n reals (the slice's segments, transformed in place), then the run partials
    double *part = nullptr;             // inside ws: up to ws_units x bins doubles
    uint64_t ws_units = 0, workspace_bytes = 0;
};

struct sdsp_hip_csd_plan {
    uint32_t n = 0, hop = 0, hist = 0, bins = 0; // hist = n - 1, bins = n / 2 + 1
    int detrend = 0, scaling = 0, precision = 0, device = 0;
    double fs = 1.0, scale = 1.0;       // scale: as the Welch plan's
    uint64_t channels = 0, npairs = 0;
    sdsp_hip_fft_plan *inner = nullptr; // forward real-input plan of n_real = n, radix 2
    void *window = nullptr;             // n values, plan precision
    void *ws = nullptr;                 // channels x ws_cols x n reals (the slice's segments, transformed in place), then the partials
    double *part_xy = nullptr;          // inside ws: npairs x ws_cols x bins complex doubles
    double *part_auto = nullptr;        // inside ws: channels x ws_cols x bins doubles
    uint32_t *tables = nullptr;         // device: the pairs (2 npairs), the run order with auto entries (3 (npairs + channels)), without
    uint64_t ws_cols = 0, column_bytes = 0, workspace_bytes = 0;
};

struct sdsp_hip_pfb_plan {
    uint32_t m = 0, p = 0, hop = 0, hist = 0, bins = 0; // hist = p m - hop; bins = m / 2 + 1 (REAL) or m (COMPLEX)
    int kind = 0, phase = 0, precision = 0, device = 0, form = 0;
    sdsp_hip_fft_plan *inner = nullptr; // REAL: forward real-input plan of n_real = m, radix 2; COMPLEX: forward complex plan of m, RADIX_AUTO
    void *taps = nullptr;               // p m values, plan precision
    void *ws = nullptr;                 // REAL: ws_units x m reals (the slice's folded frames, transformed in place); COMPLEX: none
    uint64_t ws_units = 0, workspace_bytes = 0;
};

struct sdsp_hip_pfb_synth_plan {
    uint32_t m = 0, p = 0, hop = 0, hist = 0, bins = 0; // hist = p m - hop; bins = m / 2 + 1 (REAL) or m (COMPLEX)
    int kind = 0, phase = 0, precision = 0, device = 0, form = 0;
    sdsp_hip_fft_plan *inner = nullptr; // REAL: reverse real-input plan of n_real = m, radix 2; COMPLEX: reverse complex plan of m, RADIX_AUTO
    void *taps = nullptr;               // the synthesis prototype: p m values, plan precision
    void *ws = nullptr;                 // ws_units x m elements: the slice's spectra, transformed in place
    uint64_t ws_units = 0, workspace_bytes = 0;
};

struct sdsp_hip_ddc_plan {
    uint32_t taps = 0, down = 1, hist = 0, channels = 0, nb = 0; // hist = taps - 1
    int kind = 0, precision = 0, device = 0, variant = 0;
    void *g = nullptr;        // [band in table order][tap] interleaved complex band taps, plan precision
    void *osc = nullptr;      // C then F: 2 x 65536 interleaved complex values, plan precision
    uint32_t *table = nullptr; // channels + 1 offsets (the bands sorted by src), then 4 words per band: output row, src, fcw, phase0
};

struct sdsp_hip_duc_plan {
    uint32_t taps = 0, up = 1, hist = 0, channels = 0, nb = 0; // hist = floor((taps - 1) / up)
    int kind = 0, precision = 0, device = 0, variant = 0;
    void *h = nullptr;         // the taps, plan precision
    void *osc = nullptr;       // the DDC's C then F: 2 x 65536 interleaved complex values, plan precision
    uint32_t *table = nullptr; // channels + 1 offsets (the bands sorted by dst), then 4 words per band: input row, dst, fcw, phase0
};

struct sdsp_hip_beam_plan {
    uint32_t sensors = 0, beams = 0, groups = 1, taps = 0, entries = 0, max_delay = 0, hist = 0; // hist = max_delay + taps - 1
    int kind = 0, precision = 0, device = 0, variant = 0;
    void *g = nullptr;         // [entry][tap] taps (interleaved pairs for complex), plan precision
    uint32_t *table = nullptr; // beam_build_table's: the entries, each beam's run of them, the beam chunks and their sensor records
    beam_layout lay;
};

struct sdsp_hip_lms_plan {
    uint64_t channels = 0;
    uint32_t taps = 0;
    int kind = 0, precision = 0, mode = 0, device = 0, variant = 0;
    double eps = 0.0;          // rounded to the plan precision
    void *scratch_w = nullptr; // channels x taps weights for the plain kernel of a call without state; made by set_variant(1)
};

struct sdsp_hip_rank_plan {
    uint64_t channels = 0;
    uint32_t window = 0, rank = 0;
    uint32_t run = 0;      // set_run's override; 0 = chosen per call
    uint32_t last_run = 0; // what the latest call of variant 0 took
    int precision = 0, device = 0, variant = 0;
};

struct sdsp_hip_cfar_plan {
    uint64_t channels = 0;
    uint32_t train = 0, guard = 0, rank = 0;
    uint32_t run = 0;      // set_run's override; 0 = chosen per call
    uint32_t last_run = 0; // what the latest call of variant 0 took
    int mode = 0, input = 0, precision = 0, device = 0, variant = 0;
    double alpha = 0.0, scale = 0.0; // scale: c of the mode, rounded to the precision
};

struct sdsp_hip_pll_plan {
    uint64_t channels = 0;
    int precision = 0, mode = 0, device = 0, variant = 0;
    double max_dev = 0.0;      // rounded to the plan precision
    uint32_t *fcw0 = nullptr;  // device: channels centre-frequency words
    void *osc = nullptr;       // device: the tables C then F, 2 x 2048 complex values of the precision
    void *scratch = nullptr;   // a state buffer for the plain kernel of a call without state; made by set_variant(1)
};

struct sdsp_hip_viterbi_plan {
    uint32_t k = 0, n = 0, generators[3] = {}, block = 0, depth = 0, dr = 0;
    int in_kind = 0, out_kind = 0, device = 0, variant = 0;
    float scale = 1.0f;
    uint64_t max_channels = 0, state_bytes = 0;
    void *state = nullptr;   // device: metrics, counts, decisions (the layout of sdsp_hip.h)
    void *ring_ws = nullptr; // device: the plain kernel's ring where it does not fit LDS
    uint64_t ring_bytes = 0;
};

struct sdsp_hip_fsync_plan {
    uint64_t marker = 0, max_channels = 0, max_bits = 0, max_frames = 0, state_bytes = 0, ws_bytes = 0;
    uint32_t M = 0, P = 0, L = 0, tol = 0, V = 0, F = 0, HW = 0, RW = 0;
    int polarity = 0, in_kind = 0, device = 0, variant = 0;
    void *state = nullptr; // device: the records, then the rings (the layout of sdsp_hip.h)
    void *ws = nullptr;    // device: variant 0's working rows, hit words and frame records
    void *pn = nullptr;    // device: the pn sequence as words, or null
};

struct sdsp_hip_rs_plan {
    uint32_t field_poly = 0, fcr = 0, prim = 0, nroots = 0, n = 0, interleave = 0;
    int out_kind = 0, device = 0, variant = 0;
    void *table = nullptr; // device: exp[512], log[256]
};

struct sdsp_hip_ldpc_plan {
    uint32_t mb = 0, nb = 0, z = 0, n = 0, m = 0, entries = 0, entries_at = 0, max_degree = 0;
    uint32_t norm = 0, beta = 0, out_bits = 0;
    float scale = 1.0f;
    int early_stop = 0, in_kind = 0, out_kind = 0, device = 0, variant = 0;
    void *table = nullptr; // device uint32: rowptr[0 .. mb], padding to an even count, entries x (first variable of the column, shift)
    void *ws = nullptr;    // device: variant 1's L and R of one piece; made by set_variant(1)
};

struct sdsp_hip_timing_plan {
    uint64_t channels = 0, step0 = 0;
    uint32_t phases = 1, taps = 0;
    int precision = 0, mode = 0, device = 0, variant = 0;
    double max_dev = 0.0;    // rounded to the plan precision
    void *table = nullptr;   // device: H[p][k] = h[k L + p], phases x taps reals of the precision
    void *scratch = nullptr; // a state buffer for the plain kernel of a call without state; made by set_variant(1)
};

struct sdsp_hip_fft_cols_plan {
    uint32_t n = 0;
    uint64_t width = 0;
    int direction = 0, precision = 0, output = 0, shift = 0, device = 0, variant = 0;
    void *tw = nullptr;     // device: W_n^j, j < n, direction-folded, plan precision
    void *window = nullptr; // device: n reals of the plan precision, or null
};

struct sdsp_hip_cfar2d_plan {
    uint32_t D = 0, R = 0;
    uint64_t max_maps = 0;
    sdsp_hip_cfar2d_desc desc{};
    int tabled = 0, precision = 0, device = 0, variant = 0;
    void *scale = nullptr;   // device: c(r), R reals of the plan precision
    void *ws_mask = nullptr; // device: the list's workspace (cfar2d_workspace)
    void *ws_cnt = nullptr;
    uint64_t ws_bytes = 0;
};

struct sdsp_hip_arb_plan {
    uint32_t phases = 1, taps = 0, hist = 0; // hist = taps - 1
    uint32_t block_out = 0;                  // outputs per block of sdsp_arb_kernel, fixed here from max_step
    uint64_t max_step = 0;
    int kind = 0, interp = 0, precision = 0, device = 0, variant = 0;
    void *table = nullptr; // [phase][tap] values H (nearest) or interleaved pairs (H, Dt) (linear), plan precision
};

struct sdsp_hip_cic_plan {
    uint32_t order = 0, down = 0, delay = 0, hist = 0; // hist = order * delay * down
    uint32_t in_bits = 0, growth = 0, reg_bits = 0;
    uint32_t segment = 0;                              // chunks per workgroup of sdsp_cic_kernel, 0 = automatic
    int in_type = 0, kind = 0, out_kind = 0, device = 0, variant = 0;
    double scale = 0.0;
    uint64_t *taps = nullptr; // boxcar(down * delay)^order mod 2^64, for the plain variant
};

struct sdsp_hip_cic_interp_plan {
    uint32_t order = 0, up = 0, delay = 0, hist = 0; // hist = order * delay
    uint32_t in_bits = 0, growth = 0, reg_bits = 0;
    uint32_t segment = 0;                            // chunks per workgroup of sdsp_cic_interp_kernel, 0 = automatic
    int in_type = 0, kind = 0, out_kind = 0, device = 0, variant = 0;
    double scale = 0.0;
    uint64_t *taps = nullptr; // boxcar(up * delay)^order mod 2^64, for the plain variant
};

struct sdsp_hip_filtfilt_plan {
    uint32_t sections = 0, padlen = 0;
    int kind = 0, precision = 0, device = 0, padtype = 0, variant = 0;
    double gain = 1.0;
    double a1[SDSP_HIP_MAX_SECTIONS] = {}, a2[SDSP_HIP_MAX_SECTIONS] = {};
    double b1[SDSP_HIP_MAX_SECTIONS] = {}, b2[SDSP_HIP_MAX_SECTIONS] = {};
    double ss[SDSP_HIP_MAX_SECTIONS + 1] = {}; // steady state per level
    void *ws = nullptr;                        // slice_channels x padlen samples (null when padlen = 0)
    uint64_t slice_channels = 0, workspace_bytes = 0;
};

namespace
{
// largest power-of-two column count whose padded tile fits the LDS budget
void pick_tile(int precision, uint32_t n, uint32_t want_cols, uint32_t *cols, uint32_t *pitch)
{
    uint32_t c = want_cols;
    while (c > 1 && fft_tile_lds_bytes(precision, n, c + 1) > fft_tile_max_lds_bytes())
        c >>= 1;
    *cols = c;
    *pitch = c > 1 ? c + 1 : 1; // odd pitch: both access orders spread over the banks
}

// the multi-pass paths' plan-owned workspace, allocated on the first exec that needs it (single-pass default kernels
// such as fft_big at N = 32768 never do)
int ensure_workspace(sdsp_hip_fft_plan *p)
{
    if (p->workspace || p->workspace_bytes == 0)
        return SDSP_HIP_OK;
    hipError_t e = hipMalloc(&p->workspace, p->workspace_bytes);
    if (e != hipSuccess) {
        p->workspace = nullptr;
        return fail(SDSP_HIP_ERR_NOMEM, std::string("workspace hipMalloc: ") + hipGetErrorString(e));
    }
    return SDSP_HIP_OK;
}

// the persistent kernels' sticky abort word: set by any launch whose bounded hand-off wait gave up, cleared by
// sdsp_hip_fft_exec at the start of a call (the per-launch abort flag beside the tickets is re-zeroed for every launch)
void *fft1m_sticky(const sdsp_hip_fft_plan *p) { return reinterpret_cast<char *>(p->sync) + p->sticky_off; }

// ------------------------------------------------------------------------------------------------------------------
// The optional thread-twiddle tables.  Each predicate reads the plan's shape only (n, radix, precision, real_mode, allow_mix):
// plan creation uploads a table where its predicate holds, and select_kernel / select_conv test the same predicate where a kernel
// reads the table, so a plan holds a table iff some variant of its exec or convolve can run a kernel that reads it.
// tuned N = 4096 kernels of fft4096.hip, either radix, and their fused convolution
bool uses_twt4096(const sdsp_hip_fft_plan *p) { return p->precision == SDSP_HIP_F32 && !p->real_mode && p->n == 4096; }
// register-pass families (fft_reg.hip, fft_reg64.hip) and fft_wave.hip's N = 1024 kernels; not the f32 N = 4096 radix-4 complex plan
// (fft4096.hip's kernels, or the coverage kernel)
bool uses_twt_reg(const sdsp_hip_fft_plan *p)
{
    if (p->precision == SDSP_HIP_F64)
        return fft_reg64_supports(p->n, p->radix);
    return fft_reg_supports(p->n, p->radix) && !(uses_twt4096(p) && p->radix == 4);
}
// registers-resident kernels (fft_big.hip, fft_big64.hip): the transform, its fused convolution, the REAL forms
bool uses_twt_big(const sdsp_hip_fft_plan *p)
{
    if (p->precision == SDSP_HIP_F64)
        return p->real_mode ? fft_big64_real_supports(p->n, p->radix) : fft_big64_supports(p->n, p->radix);
    return p->real_mode ? fft_big_real_supports(p->n, p->radix) : fft_big_conv_supports(p->n, p->radix);
}
// fft_wave.hip's N = 256 / 512 / 2048 kernels (real-input plans: n <= 512)
bool uses_twt_wave(const sdsp_hip_fft_plan *p)
{
    return p->precision == SDSP_HIP_F32 && fft_wave2_supports(p->n, p->radix) && (!p->real_mode || p->n <= 512);
}
// fft_mix.hip: the sub-transforms' table and the leading stage's twiddles
bool uses_mix(const sdsp_hip_fft_plan *p) { return p->precision == SDSP_HIP_F32 && !p->real_mode && p->allow_mix && fft_mix_supports(p->n); }

// ------------------------------------------------------------------------------------------------------------------
// The ONE dispatch table: which kernel serves (plan, variant), with which launcher and which table.  sdsp_hip_fft_exec,
// sdsp_hip_fft_plan_get_info and sdsp_hip_fft_plan_launches go through select_kernel(), sdsp_hip_fft_convolve through
// select_conv() beside it, so what the plan reports is what runs, by construction.
enum fft_kernel_id {
    K_NOOP = 0,
    K_FFT4096_R4,    // fft4096.hip: the headline kernel (cfg 2 / 5)
    K_FFT4096_R2,    // fft4096.hip: its radix-2 sibling
    K_MIX,           // fft_mix.hip: one leading radix-2 / radix-4 stage + the N = 4096 radix-4 machinery
    K_BIG,           // fft_big.hip: transform in registers, N = 8192 .. 32768
    K_BIG_REAL,      // fft_big.hip, REAL form (real-input plans, n = n_real / 2 = 2048 .. 32768)
    K_BIG64,         // fft_big64.hip: the same design in double, N = 4096 .. 16384
    K_BIG64_REAL,    // fft_big64.hip, REAL form (real-input plans in double, n = n_real / 2 = 4096 .. 16384)
    K_REG64,         // fft_reg64.hip: register-pass family in double
    K_WAVE64,        // fft_wave.hip: N = 1024 in double, one transform per two waves
    K_WAVE1024,      // fft_wave.hip: N = 1024 f32, one transform per wave
    K_WAVE2,         // fft_wave.hip: N = 256 / 512 / 2048 f32
    K_REG32,         // fft_reg.hip: register-pass family, f32
    K_TILE,          // fft_tile.hip: coverage kernel, one pass
    K_FFT1M_CHUNKED, // fft1m.hip: two launches per chunk of <= 32 transforms
    K_FFT1M_FUSED,   // fft1m.hip: one persistent launch (cfg 3)
    K_2PASS,         // fft_2pass.hip: N = N1 x N2, two passes
    K_2PASS_FUSED,   // fft_2pass.hip: the same tiles in one persistent, ticketed launch
    K_MID,           // fft_mid.hip: 16-point column step + row plan + untwist
    K_FOUR_STEP,     // fft_tile.hip twice: the general four-step
    K_UNSUPPORTED,   // no kernel serves this (plan, variant)
};

using reg_launcher = int (*)(const fft_reg_args &, void *);
using plan_table = void *sdsp_hip_fft_plan::*;

struct fft_kernel_sel {
    fft_kernel_id id;
    const char *name;  // as rocprofv3 prints the dominant kernel(s)
    int hbm_passes;    // passes over HBM of one transform
    int stage_radix;   // butterflies that run: 2, 4, or SDSP_HIP_STAGES_2_THEN_4
    bool workspace;    // needs the plan-owned workspace
    bool pieces;       // one launch per batch, issued in launch pieces (sdsp_hip_set_launch_piece_bytes)
    reg_launcher launch = nullptr; // kernels launched with fft_reg_args (launch_reg)
    plan_table table = nullptr;    // the optional table the kernel reads (its `tw`)
    bool nontemporal = true;       // fft_reg_args.nontemporal
    bool conv = false;             // select_conv: one launch computes the whole convolution ...
    int variant = 0;               // ... or else the variant of the three-launch composition's forward transform
};

fft_kernel_sel select_kernel(const sdsp_hip_fft_plan *p, int variant)
{
    using P = sdsp_hip_fft_plan;
    const bool f32 = p->precision == SDSP_HIP_F32;
    // launch pieces: kernels with many short workgroups (N <= 8192); see fft_exec_pieces
    const bool pc = (p->path == PATH_FFT4096 || p->path == PATH_REG || p->path == PATH_TILE) && p->n <= 8192;
    if (p->path == PATH_NOOP)
        return { K_NOOP, "none", 0, p->radix, false, false };
    if (p->path == PATH_FFT4096 && variant < fft4096_num_variants())
        return { K_FFT4096_R4, "sdsp_fft4096_r4_f32", 1, 4, false, pc, nullptr, &P::twt };
    if (p->path == PATH_REG && f32 && variant == 0 && p->n == 4096 && p->radix == 2 && !p->real_mode)
        return { K_FFT4096_R2, "sdsp_fft4096_r2_f32", 1, 2, false, pc, nullptr, &P::twt };
    // N = 8192 / 16384 f32, either stage type: one leading radix-2 / radix-4 stage + the tuned N = 4096 radix-4 machinery
    const bool mix_size = p->path == PATH_REG && uses_mix(p);
    const int mix_variant = big_is_default(p->n, p->radix) ? 1 : 0;
    if (mix_size && variant == mix_variant)
        return { K_MIX, "sdsp_fft_mix_f32", 1, p->n == 8192 ? SDSP_HIP_STAGES_2_THEN_4 : 4, false, pc, nullptr, &P::twt_mix };
    // N = 32768 (variant 0) and N = 8192 / 16384 (variant 0 or 1, see big_is_default), f32: registers-resident kernel
    if ((p->path == PATH_REG || p->path == PATH_FOUR_STEP) && f32 && variant == (mix_size ? 1 - mix_variant : 0) && !p->real_mode &&
        fft_big_supports(p->n, p->radix))
        return { K_BIG, "sdsp_fft_big_kernel", 1, big_r4_form(p->n, p->radix) ? 4 : 2, false, pc, launch_fft_big_f32, &P::twt_big };
    // real-input plans of n_real = 4096 .. 65536: split / merge inside the registers-resident kernel; variants 1 / 2 keep
    // the register-pass family's MODE 1 / 2
    if (p->path == PATH_REG && f32 && variant == 0 && p->real_mode && uses_twt_big(p))
        return { K_BIG_REAL, "sdsp_fft_big_kernel", 1, big_r4_form(p->n, p->radix) ? 4 : 2, false, pc, launch_fft_big_f32, &P::twt_big };
    // double precision, N = 4096 / 8192 / 16384: the registers-resident kernel in double (fft_big64.hip) -- radix-2 stages, or, for
    // radix-4 plans of N = 4096 / 16384, genuine radix-4 stages (its R4 form).
    // The default of all three sizes: 73.4 / 74.5 / 59.5 % of HBM peak against 67.5 % (N = 4096, fft_reg64.hip), 51.4 % (N = 8192:
    // the whole tile in LDS) and 24.2 % (N = 16384: three streaming passes) in one call (tools/sweep_sizes64.py, round 3);
    // what served a size before is its variant 1
    const bool big64 = !f32 && !p->real_mode && uses_twt_big(p);
    if (big64 && variant == big64_variant(p->n))
        return { K_BIG64, "sdsp_fft_big_f64_kernel", 1, p->radix == 4 ? 4 : 2, false, pc && p->n <= 4096, launch_fft_big_f64, &P::twt_big };
    // real-input plans in double of n_real = 8192 / 16384 / 32768 (radix 2): split / merge around the same transform (its REAL form);
    // variant 1 keeps the register-pass family's MODE 1 / 2 (n_real <= 16384)
    const bool big64_real = !f32 && p->real_mode && uses_twt_big(p);
    if (big64_real && variant == 0)
        return { K_BIG64_REAL, "sdsp_fft_big_f64_real_kernel", 1, 2, false, pc && p->n <= 4096, launch_fft_big_f64, &P::twt_big };
    if (p->path == PATH_REG && !f32 && fft_reg64_supports(p->n, p->radix)) {
        if ((big64 && big64_variant(p->n) == 0) || big64_real) // the kernel that was the default becomes variant 1
            variant = variant == 1 ? 0 : variant;
        const bool wave64 = !p->real_mode && fft_wave_supports(p->n, p->radix);
        if (variant == 1 && wave64) // N = 1024 alternate: same bits; measured 71.4-72.1 % against 71.7-72.6 %: no gain in double
            return { K_WAVE64, "sdsp_fft1024_wave", 1, p->radix, false, pc, launch_fft_wave_f64, &P::twt_reg };
        if (variant == 0)
            return { K_REG64, "sdsp_fft_reg_f64_kernel", 1, p->radix, false, pc, launch_fft_reg_f64, &P::twt_reg };
    }
    if (p->path == PATH_REG && f32 && variant < 3) {
        // Complex plans: the register-pass family (fft_reg.hip) at every N <= 2048 since its tiles are 2048 points (eight 128-thread
        // workgroups per CU instead of four of 256; round 3): 75.8-78.9 % of HBM peak at N = 16 .. 2048, either radix, in one call,
        // where it measured 68-74 % with 4096-point tiles and the one-wave kernels (fft_wave.hip) 72.5 / 74.7 / 74.2 % at N = 256 /
        // 1024 / 2048 -- those are variant 2 of their sizes now (variant 1: the family with the default cache policy).
        // Real-input plans (the one-wave kernels split / merge by ds_bpermute, the family in LDS): with the 2048-point tiles the family
        // leads at n_real = 512 (74.7 against 71.8 %; radix 4: 75.5 / 71.0) and 2048 (70.5 / 67.2), the one-wave kernel keeps n_real = 1024
        // (70.8 / 69.8) -- tools/rfft_probe.py, one call each; n_real = 4096 .. 65536 radix 2 were taken by K_BIG_REAL above
        const int wave_variant = (p->real_mode && p->n == 512) ? 0 : 2;
        const bool nt = variant != 1 || uses_mix(p); // variant 1: default cache policy (N < 8192)
        if (variant == wave_variant && fft_wave_supports(p->n, p->radix) && (!p->real_mode || p->radix == 2))
            return { K_WAVE1024, "sdsp_fft1024_wave", 1, p->radix, false, pc, launch_fft_wave_f32, &P::twt_reg, nt };
        if (variant == wave_variant && uses_twt_wave(p) && (p->real_mode || p->n != 512))
            return { K_WAVE2, "sdsp_fft_wave_f32", 1, p->radix, false, pc, launch_fft_wave2_f32, &P::twt_wave, nt };
        return { K_REG32, "sdsp_fft_reg_kernel", 1, p->radix, false, pc, launch_fft_reg_f32, &P::twt_reg, nt };
    }
    if (p->real_mode)
        return { K_UNSUPPORTED, "none", 0, p->radix, false, false };
    if (p->path == PATH_TILE || p->path == PATH_FFT4096 || p->path == PATH_REG)
        return { K_TILE, "sdsp_fft_tile_kernel", 1, p->radix, false, pc };
    // ---- everything below is multi-pass and uses the plan's workspace
    if (p->path == PATH_FFT1M && variant < 2) {
        if (variant == 1 || p->ws_batch < kFft1mQueues * kFft1mRing)
            return { K_FFT1M_CHUNKED, "sdsp_fft1m_cols+sdsp_fft1m_rows", 2, 2, true, false };
        return { K_FFT1M_FUSED, "sdsp_fft1m_fused", 2, 2, true, false };
    }
    // variant 2: the same schedule through fft_2pass.hip's generic persistent kernel (its tile functions at 1024 x 1024) -- the A/B that
    // says what the dedicated kernel of fft1m_kernels.h is worth
    if (p->path == PATH_FFT1M && variant == 2 && p->ws_batch >= 4 * kFft1mQueues)
        return { K_2PASS_FUSED, "sdsp_fft2p_fused", 2, 2, true, false };
    const bool two_pass_size = fft_2pass_supports(p->n, p->precision);
    // two schedules over the same tiles (bit-identical results): ONE persistent, ticketed launch (the workspace is a ring of
    // intermediates inside the Infinity Cache; needs a plan whose workspace holds that ring) -- variant 0, level or ahead at every size in
    // one-call A/Bs (fft_2pass.hip, profiles/r03_fft2p_fused_lab.txt) -- and two launches per chunk of 256 MiB, variant 3
    if (p->path == PATH_FOUR_STEP && two_pass_size && (variant == 0 || variant == 3)) {
        if (p->f2_unit && variant == 0)
            return { K_2PASS_FUSED, "sdsp_fft2p_fused", 2, 2, true, false };
        return { K_2PASS, "sdsp_fft2p_cols+sdsp_fft2p_rows", 2, 2, true, false };
    }
    // three streaming passes, N = 16 x N2 with the rows on a tuned single-pass kernel (or, nested, on another plan)
    if (p->path == PATH_FOUR_STEP && p->mid_rows && variant == ((two_pass_size || (big64 && big64_variant(p->n) == 0)) ? 1 : 0)) {
        const fft_kernel_sel rows = select_kernel(p->mid_rows, p->mid_rows->variant);
        // the column step is four radix-2 stages (fft_mid.hip), whatever runs in the rows
        return { K_MID, "sdsp_fft_col16_kernel+rows+sdsp_fft_untwist16", 2 + rows.hbm_passes,
                 rows.stage_radix == 2 ? 2 : SDSP_HIP_STAGES_2_THEN_4, true, false };
    }
    return { K_FOUR_STEP, "sdsp_fft_tile_kernel", 2, p->radix, true, false };
}

// The convolution y = IFFT(FFT(x) .* h) of a forward complex plan (sdsp_hip_fft_convolve) with kernel variant `variant`: ONE fused
// launch (`conv`: both transforms and the multiply; launch_reg passes real_mode 3 and h in tw2), or else the three-launch composition --
// the forward transform of `variant` (the result's), the multiply (riding on its pass 2 where that is K_2PASS / K_2PASS_FUSED: four
// passes over HBM instead of five), the partner plan's reverse transform.  Either form runs in launch pieces where the plan is a
// single-pass one of N <= 8192.
fft_kernel_sel select_conv(const sdsp_hip_fft_plan *p, int variant)
{
    using P = sdsp_hip_fft_plan;
    const bool f32 = p->precision == SDSP_HIP_F32, reg = p->path == PATH_REG, big = reg || p->path == PATH_FOUR_STEP;
    const bool pc = (p->path == PATH_FFT4096 || reg || p->path == PATH_TILE) && p->n <= 8192;
    auto fused = [&](fft_kernel_id id, const char *name, reg_launcher launch, plan_table table) {
        return fft_kernel_sel{ id, name, 1, p->radix, false, pc, launch, table, true, true };
    };
    if (p->path == PATH_FFT4096 && variant == 0)
        return fused(K_FFT4096_R4, "sdsp_fft4096_conv_f32", nullptr, &P::twt);
    // N = 2048 .. 32768 radix-2 stages, N = 16384 radix-4 stages: both transforms and the multiply in the registers-resident kernel
    // (fft_big.hip)
    if (big && f32 && variant == 0 && uses_twt_big(p))
        return fused(K_BIG, "sdsp_fft_big_kernel", launch_fft_big_f32, &P::twt_big);
    // variant 0: the fused kernel of the size; variant 2: the register-pass family's fused MODE 3 where a one-wave kernel is the
    // default (A/B and cross-check); any other variant: three launches
    if (reg && f32 && variant == 0 && fft_wave_supports(p->n, p->radix)) // N = 1024: both transforms in one wave's registers
        return fused(K_WAVE1024, "sdsp_fft1024_wave", launch_fft_wave_f32, &P::twt_reg);
    // N = 256 / 512 radix 2 (N = 2048 radix 2 was taken by the fft_big.hip form above: 65-69 % against 52 %)
    if (reg && f32 && variant == 0 && uses_twt_wave(p))
        return fused(K_WAVE2, "sdsp_fft_wave_f32", launch_fft_wave2_f32, &P::twt_wave);
    if (reg && f32 && (variant == 0 || variant == 2))
        return fused(K_REG32, "sdsp_fft_reg_kernel", launch_fft_reg_f32, &P::twt_reg);
    // double, N = 4096 / 8192 / 16384 radix-2 plans: fft_big64.hip's convolution form; variant 2: what served N <= 8192 before (the
    // register-pass family's fused MODE 3)
    if (big && !f32 && variant == 0 && uses_twt_big(p) && fft_big64_conv_supports(p->n, p->radix))
        return fused(K_BIG64, "sdsp_fft_big_f64_kernel", launch_fft_big_f64, &P::twt_big);
    if (reg && !f32 && (variant == 0 || variant == 2)) // f64, N = 16 .. 8192
        return fused(K_REG64, "sdsp_fft_reg_f64_kernel", launch_fft_reg_f64, &P::twt_reg);
    // PATH_FFT4096 with variant != 0 selects the three launches for cross-checking: its transforms run variant 0.  N = 2^20 f32 takes
    // the generic persistent kernel (its variant 2) for the forward half, which can carry the multiply
    int v = p->path == PATH_FFT4096 ? 0 : variant;
    if (p->path == PATH_FFT1M && v == 0 && select_kernel(p, 2).id == K_2PASS_FUSED)
        v = 2;
    fft_kernel_sel s = select_kernel(p, v);
    s.pieces = pc;
    s.variant = v;
    return s;
}

// a kernel is never handed a null table: a predicate that disagrees with what plan creation uploaded is a host error
int check_table(const sdsp_hip_fft_plan *p, const fft_kernel_sel &sel)
{
    if (sel.table && !(p->*sel.table))
        return fail(SDSP_HIP_ERR_UNSUPPORTED, std::string(sel.name) + ": the plan holds no table for this kernel");
    return SDSP_HIP_OK;
}

// every kernel launched with fft_reg_args: the transforms, and with `h` the fused convolutions (real_mode 3, h in tw2)
int launch_reg(const sdsp_hip_fft_plan *p, const fft_kernel_sel &sel, void *data, uint64_t batch, hipStream_t stream,
               const void *h = nullptr)
{
    const bool f64 = p->precision == SDSP_HIP_F64;
    fft_reg_args a;
    a.data = data;
    a.tw = p->*sel.table;
    a.n = p->n;
    a.radix = p->radix;
    a.batch = batch;
    a.scale = f64 ? 1.0f : (float)(1.0 / p->n); // the f64 kernels scale by scale_d
    a.scale_d = f64 ? 1.0 / p->n : 1.0;
    a.reverse = p->direction == SDSP_HIP_REVERSE;
    a.nontemporal = sel.nontemporal;
    a.real_mode = h ? 3 : p->real_mode;
    a.tw2 = h ? h : p->real_mode ? p->tw2 : nullptr; // real-input plans: W_2n (a complex four-step plan's tw2 is W_n2)
    return sel.launch(a, stream);
}

// transforms one step of a multi-pass schedule covers -- a chunk of two launches, one persistent launch, one workspace slice
// (shared by exec and the launch count)
uint64_t fft_step_units(const sdsp_hip_fft_plan *p, fft_kernel_id id)
{
    switch (id) {
    case K_FFT1M_CHUNKED: return std::max<uint64_t>(1, std::min<uint64_t>(32, p->ws_batch));
    case K_FFT1M_FUSED: return p->sync_count;
    case K_2PASS: { // an intermediate of at most 256 MiB per chunk
        const uint64_t cap = 1ull << 28; // the Infinity Cache: 37 % at 256 MiB, 35 % at 128 / 192, 33 - 34 % at 288 MiB and beyond (profiles/r03_fft2p_chunk_lab.txt)
        return std::max<uint64_t>(1, std::min<uint64_t>(p->ws_batch, cap / ((uint64_t)p->n * esize(p->precision))));
    }
    case K_2PASS_FUSED: return p->path == PATH_FFT1M ? p->sync_count : p->sync_count * p->f2_unit; // N = 2^20: unit = one transform
    default: return p->ws_batch; // K_MID, K_FOUR_STEP
    }
}

int fft_exec_device(sdsp_hip_fft_plan *p, void *data, uint64_t batch, hipStream_t stream, int variant, const void *hmul = nullptr);

// one step of the multi-pass kernel `id` over `nb` transforms at `d`
int fft_exec_step(sdsp_hip_fft_plan *p, fft_kernel_id id, char *d, uint64_t nb, hipStream_t stream, const void *hmul)
{
    const int rev = p->direction == SDSP_HIP_REVERSE;
    const float scale = (float)(1.0 / p->n);
    switch (id) {
    case K_FFT1M_CHUNKED: { // two launches per chunk of <= 32 transforms (round 1's schedule; also what plans with a small workspace run)
        fft1m_args a;
        a.data = d;
        a.workspace = p->workspace;
        a.tw_n = p->tw;
        a.tw_1024 = p->tw1;
        a.count = nb;
        a.scale = scale;
        a.reverse = rev;
        if (int rc = launch_fft1m_pass(a, 1, stream))
            return rc;
        return launch_fft1m_pass(a, 2, stream);
    }
    case K_FFT1M_FUSED: { // ONE persistent launch (fft1m_kernels.h): eight ticket queues, per queue a ring of three intermediates,
                          // pass 2 of a queue's transform one ticket step behind its pass 1
        fft1m_fused_args a;
        a.data = d;
        a.workspace = p->workspace;
        a.tw_1024 = p->tw1;
        a.sync = p->sync;
        a.sticky = fft1m_sticky(p);
        a.spin_limit = p->wait_limit;
        a.count = nb;
        // a ring of 4 with pass 2 two steps behind measured 42.0-42.2 %, 3 / one step 41.4-41.6 % (profiles/r02_fft1m_lab.md)
        a.ring = p->ws_batch >= 4 * kFft1mQueues ? 4 : (uint32_t)kFft1mRing;
        a.lag = a.ring - 2;
        a.queues = (uint32_t)kFft1mQueues;
        a.scale = scale;
        a.reverse = rev;
        return launch_fft1m_fused(a, stream);
    }
    case K_2PASS_FUSED: { // the two-pass sizes in one persistent launch per kFused2pUnitsPerLaunch units
        const bool m1 = p->path == PATH_FFT1M; // unit = one transform, the counters of the dedicated kernel
        fft_2pass_fused_args a;
        a.data = d;
        a.workspace = p->workspace;
        a.tw_1024 = m1 ? p->tw1 : p->tw1024; // N = 2^20: n1 = 1024, so W_n1 is that table
        a.sync = p->sync;
        a.sticky = fft1m_sticky(p);
        a.spin_limit = p->wait_limit;
        a.count = nb;
        a.n = p->n;
        a.unit = m1 ? 1 : p->f2_unit;
        a.ring = m1 ? 4 : p->f2_ring;
        a.lag = m1 ? 2 : p->f2_lag;
        a.queues = m1 ? (uint32_t)kFft1mQueues : p->f2_queues;
        a.scale = scale;
        a.scale_d = 1.0 / p->n;
        a.reverse = rev;
        a.hmul = hmul;
        return launch_fft_2pass_fused(p->precision, a, stream);
    }
    case K_2PASS: { // N = 2^16 .. 2^19, f32: two passes over HBM (fft_2pass.hip), in chunks whose intermediate is at most 256 MiB
        fft_2pass_args a;
        a.data = d;
        a.workspace = p->workspace;
        a.tw_1024 = p->tw1024;
        a.n = p->n;
        a.count = nb;
        a.scale = scale;
        a.scale_d = 1.0 / p->n;
        a.reverse = rev;
        a.hmul = hmul;
        return launch_fft_2pass(p->precision, a, stream);
    }
    case K_MID: { // three streaming passes, N = 16 x N2 with the rows on a tuned single-pass kernel: f32 N = 2^21 .. 2^23, f64
                  // N = 2^14 .. 2^21, and variant 1 of the f32 sizes above
        const uint32_t n2 = p->n / 16;
        if (int rc = launch_fft_mid_cols(p->precision, d, p->workspace, p->tw1024, n2, nb, rev, stream))
            return rc;
        if (int rc = fft_exec_device(p->mid_rows, p->workspace, nb * 16, stream, p->mid_rows->variant))
            return rc;
        return launch_fft_mid_untwist(p->precision, p->workspace, d, n2, nb, stream);
    }
    default: break; // K_FOUR_STEP
    }
    // four-step: N = n1 x n2 viewed as a row-major [n1][n2] matrix (index n = n2_count*i1 + i2).
    //   pass 1: length-n1 transforms down the columns, times W_N^(i2*k1), data -> workspace
    //   pass 2: length-n2 transforms along the rows, written transposed, workspace -> data
    const uint64_t N = (uint64_t)p->n1 * p->n2;
    fft_tile_args a{};
    a.in = d;
    a.out = p->workspace;
    a.tw = p->tw1;
    a.tw_big = p->tw;
    a.n = p->n1;
    a.log2n = sdsp_hip_log2(p->n1);
    a.cols = p->cols1;
    a.pitch = p->pitch1;
    a.tiles_per_group = p->n2 / p->cols1;
    a.total_cols = nb * p->n2;
    a.group_stride = N;
    a.in_tile_step = a.out_tile_step = p->cols1;
    a.in_si = a.out_sk = p->n2;
    a.in_sc = a.out_sc = 1;
    a.in_c_fast = a.out_c_fast = 1;
    a.reverse = rev;
    a.apply_scale = 0;
    a.scale = 1.0f;
    a.scale_d = 1.0;
    if (int rc = launch_fft_tile(p->precision, p->radix, a, nb * a.tiles_per_group, stream))
        return rc;

    fft_tile_args c{};
    c.in = p->workspace;
    c.out = d;
    c.tw = p->tw2;
    c.tw_big = nullptr;
    c.n = p->n2;
    c.log2n = sdsp_hip_log2(p->n2);
    c.cols = p->cols2;
    c.pitch = p->pitch2;
    c.tiles_per_group = p->n1 / p->cols2;
    c.total_cols = nb * p->n1;
    c.group_stride = N;
    c.in_tile_step = (uint64_t)p->cols2 * p->n2;
    c.out_tile_step = p->cols2;
    c.in_si = 1;
    c.in_sc = p->n2;
    c.in_c_fast = 0;
    c.out_sk = p->n1;
    c.out_sc = 1;
    c.out_c_fast = 1;
    c.reverse = rev;
    c.apply_scale = rev;
    c.scale = (float)(1.0 / (double)N);
    c.scale_d = 1.0 / (double)N;
    return launch_fft_tile(p->precision, p->radix, c, nb * c.tiles_per_group, stream);
}

// `variant`: the kernel variant to run (normally the plan's; the convolution path overrides it without touching the plan)
// hmul (the two-pass kernels, forward plans): every output leaves multiplied by hmul[k] -- the fused convolution's forward half
int fft_exec_device(sdsp_hip_fft_plan *p, void *data, uint64_t batch, hipStream_t stream, int variant, const void *hmul)
{
    if (batch == 0 || p->path == PATH_NOOP)
        return SDSP_HIP_OK;
    const bool rev = p->direction == SDSP_HIP_REVERSE;
    const fft_kernel_sel sel = select_kernel(p, variant);
    if (sel.id == K_UNSUPPORTED)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "real-input plans have no alternative kernel variant");
    if (int rc = check_table(p, sel))
        return rc;
    if (sel.launch)
        return launch_reg(p, sel, data, batch, stream);
    switch (sel.id) {
    case K_FFT4096_R4:
    case K_FFT4096_R2: {
        fft4096_args a;
        a.data = data;
        a.tw = p->twt;
        a.batch = batch;
        a.scale = 1.0f / 4096.0f;
        a.reverse = rev;
        return sel.id == K_FFT4096_R4 ? launch_fft4096_r4_f32(a, variant, stream) : launch_fft4096_r2_f32(a, stream);
    }
    case K_MIX: {
        fft_mix_args a;
        a.data = data;
        a.tw = p->twt_mix;
        a.tw_lead = p->tw_lead;
        a.n = p->n;
        a.batch = batch;
        a.scale = (float)(1.0 / p->n);
        a.reverse = rev;
        return launch_fft_mix_f32(a, stream);
    }
    case K_TILE: {
        fft_tile_args a{};
        a.in = data;
        a.out = data;
        a.tw = p->tw;
        a.tw_big = nullptr;
        a.n = p->n;
        a.log2n = sdsp_hip_log2(p->n);
        a.cols = p->cols;
        a.pitch = p->pitch;
        a.total_cols = batch;
        a.tiles_per_group = 1;
        a.group_stride = (uint64_t)p->cols * p->n;
        a.in_tile_step = a.out_tile_step = 0;
        a.in_si = a.out_sk = 1;
        a.in_sc = a.out_sc = p->n;
        a.in_c_fast = a.out_c_fast = 0;
        a.reverse = rev;
        a.apply_scale = rev;
        a.scale = (float)(1.0 / p->n);
        a.scale_d = 1.0 / p->n;
        const uint64_t tiles = (batch + p->cols - 1) / p->cols;
        return launch_fft_tile(p->precision, p->radix, a, tiles, stream);
    }
    default:
        break; // the multi-pass kernels follow
    }
    if (int rc = ensure_workspace(p))
        return rc;
    const uint64_t step = fft_step_units(p, sel.id), row_bytes = (uint64_t)p->n * esize(p->precision);
    for (uint64_t done = 0; done < batch; done += step)
        if (int rc = fft_exec_step(p, sel.id, static_cast<char *>(data) + done * row_bytes, std::min(step, batch - done), stream, hmul))
            return rc;
    return SDSP_HIP_OK;
}

// single-launch paths in pieces (sdsp_hip_set_launch_piece_bytes); the multi-pass paths chunk by their workspace already
// N <= 8192: kernels with many short workgroups, where pieces measured +1 .. +3 points (N = 64: 66.6 -> 69.8 %, 1024:
// 68.7 -> 71.4 %, 4096: 72.1 -> 76.3 %, 8192: 75.4 -> 76.4 %, 4 GiB buffers).  The N = 16384 / 32768 kernels keep one
// or two transforms per CU for tens of microseconds: 62.9 -> 61.3 % and 44.9 -> 43.3 % in pieces, so they stay whole.
uint64_t fft_piece(const sdsp_hip_fft_plan *p, const fft_kernel_sel &sel, uint64_t batch)
{
    if (!sel.pieces)
        return batch;
    const uint64_t row_bytes = (uint64_t)p->n * esize(p->precision); // real-input plans: n = n_real / 2 complex elements
    return piece_units(batch, row_bytes, p->n < 16 ? 4096 : 256);    // a multiple of what one workgroup owns
}

int fft_exec_pieces(sdsp_hip_fft_plan *p, void *data, uint64_t batch, hipStream_t stream, int variant)
{
    const fft_kernel_sel sel = select_kernel(p, variant);
    const uint64_t row_bytes = (uint64_t)p->n * esize(p->precision);
    const uint64_t piece = fft_piece(p, sel, batch);
    for (uint64_t done = 0; done < batch; done += piece) {
        const uint64_t nb = std::min(piece, batch - done);
        if (int rc = fft_exec_device(p, static_cast<char *>(data) + done * row_bytes, nb, stream, variant))
            return rc;
    }
    return SDSP_HIP_OK;
}

// kernel launches one sdsp_hip_fft_exec(plan, data, batch) issues with kernel variant `variant` (memsets not counted)
uint64_t fft_launch_count(const sdsp_hip_fft_plan *p, uint64_t batch, int variant, bool in_pieces = true)
{
    if (batch == 0)
        return 0;
    const fft_kernel_sel sel = select_kernel(p, variant);
    auto ceil_div = [](uint64_t a, uint64_t b) { return (a + b - 1) / b; };
    switch (sel.id) {
    case K_NOOP:
    case K_UNSUPPORTED: return 0;
    case K_FFT1M_FUSED:
    case K_2PASS_FUSED: return ceil_div(batch, fft_step_units(p, sel.id));
    case K_FFT1M_CHUNKED:
    case K_2PASS:
    case K_FOUR_STEP: return 2 * ceil_div(batch, fft_step_units(p, sel.id));
    case K_MID: {
        const uint64_t step = fft_step_units(p, K_MID);
        uint64_t n = 0;
        for (uint64_t done = 0; done < batch; done += step)
            n += 2 + fft_launch_count(p->mid_rows, std::min(step, batch - done) * 16, p->mid_rows->variant, false);
        return n;
    }
    default: return in_pieces ? ceil_div(batch, fft_piece(p, sel, batch)) : 1;
    }
}

int fft1m_check_sticky(sdsp_hip_fft_plan *p)
{
    if (!p->sync)
        return SDSP_HIP_OK;
    unsigned flag = 0;
    HIP_TRY(hipMemcpy(&flag, fft1m_sticky(p), sizeof(flag), hipMemcpyDeviceToHost));
    if (flag)
        return fail(SDSP_HIP_ERR_HIP, "a persistent two-pass launch gave up on a bounded wait between its passes: the output of the last call is invalid");
    return SDSP_HIP_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// What the framed banks (STFT, inverse STFT, Welch, filter bank) share around their inner FFT plan.

// The kernel variant of a bank's inner plan.  Rejected here rather than at the next process call: a variant without a kernel, or whose
// kernel needs a table this size's plan does not upload.  `with_workspace`: a multi-pass alternate of a single-pass default gets
// its workspace here, not on the launch path.
int set_inner_variant(sdsp_hip_fft_plan *inner, int variant, const char *unsupported_msg, bool with_workspace = false)
{
    const fft_kernel_sel sel = select_kernel(inner, variant);
    if (sel.id == K_UNSUPPORTED)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, unsupported_msg);
    if (int rc = check_table(inner, sel))
        return rc;
    if (with_workspace && sel.workspace) {
        if (int rc = use_device(inner->device))
            return rc;
        if (int rc = ensure_workspace(inner))
            return rc;
    }
    inner->variant = variant;
    return SDSP_HIP_OK;
}

// kernel launches of a bank's slice loop over `total` units: per slice, `own` launches of the bank and the inner transform's
uint64_t slice_launch_count(const sdsp_hip_fft_plan *inner, uint64_t total, uint64_t ws_units, uint64_t own)
{
    uint64_t n = 0;
    for (uint64_t g0 = 0; g0 < total; g0 += ws_units)
        n += own + fft_launch_count(inner, std::min(ws_units, total - g0), inner->variant);
    return n;
}

// the device side of a bank's plan_destroy: its workspace, its table (window or taps) and its inner plan
void free_bank(int device, void *ws, void *table, sdsp_hip_fft_plan *inner)
{
    if (use_device(device) == SDSP_HIP_OK) {
        (void)hipFree(ws);
        (void)hipFree(table);
    }
    if (inner)
        sdsp_hip_fft_plan_destroy(inner);
}

} // namespace

extern "C" {

// ------------------------------------------------------------------ runtime

int sdsp_hip_device_count(int *count)
{
    if (!count)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "count is null");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *count = e == hipSuccess ? c : 0;
    return SDSP_HIP_OK;
}

int sdsp_hip_malloc(void **dev_ptr, size_t bytes, int device)
{
    if (!dev_ptr)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "dev_ptr is null");
    if (int rc = use_device(device))
        return rc;
    HIP_TRY(hipMalloc(dev_ptr, bytes ? bytes : 1));
    return SDSP_HIP_OK;
}

int sdsp_hip_free(void *dev_ptr, int device)
{
    if (!dev_ptr)
        return SDSP_HIP_OK;
    if (int rc = use_device(device))
        return rc;
    HIP_TRY(hipFree(dev_ptr));
    return SDSP_HIP_OK;
}

int sdsp_hip_memcpy_h2d(void *dev_dst, const void *host_src, size_t bytes, int device)
{
    if (int rc = use_device(device))
        return rc;
    HIP_TRY(hipMemcpy(dev_dst, host_src, bytes, hipMemcpyHostToDevice));
    return SDSP_HIP_OK;
}

int sdsp_hip_memcpy_d2h(void *host_dst, const void *dev_src, size_t bytes, int device)
{
    if (int rc = use_device(device))
        return rc;
    HIP_TRY(hipMemcpy(host_dst, dev_src, bytes, hipMemcpyDeviceToHost));
    return SDSP_HIP_OK;
}

int sdsp_hip_device_synchronize(int device)
{
    if (int rc = use_device(device))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    return SDSP_HIP_OK;
}

// ------------------------------------------------------------------ FFT plans

// real_mode 0: a complex plan; 1 / 2: the real-input plan of n_real = 2 n (forward / inverse), decided here as the plan it is
static int fft_plan_create(sdsp_hip_fft_plan **out, uint32_t n, int radix, int direction, int precision, uint64_t max_batch,
                           int device, int real_mode)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    // radix 0 (SDSP_HIP_RADIX_AUTO): radix-4 stages where n is a power of 4, radix-2 stages otherwise -- the
    // "mixed" entry of SURVEY 8(f)-4: any power of two without the caller choosing the function
    const bool radix_auto = radix == SDSP_HIP_RADIX_AUTO;
    if (radix_auto) {
        if (!sdsp_hip_is_power_of_2(n))
            return fail(SDSP_HIP_ERR_INVALID_SIZE, "FFT size must be a power of 2!");
        // the stage type of the fastest kernel of the size: radix 4 where n is a power of 4 -- except n = 16384, where
        // fft_big.hip's radix-2 stages measure 69-70 % of HBM peak and its seven radix-4 stages 67-69 %
        radix = (sdsp_hip_is_power_of_4(n) && n != 16384) ? 4 : 2;
    }
    // the reference's static_asserts (fft.h:261, :304) as run-time checks
    if (radix == 2) {
        if (!sdsp_hip_is_power_of_2(n))
            return fail(SDSP_HIP_ERR_INVALID_SIZE, "FFT size must be a power of 2!");
    } else if (radix == 4) {
        if (!sdsp_hip_is_power_of_4(n))
            return fail(SDSP_HIP_ERR_INVALID_SIZE, "FFT radix 4 size must be a power of 4!");
    } else {
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "radix must be 2 or 4");
    }
    if (direction != SDSP_HIP_FORWARD && direction != SDSP_HIP_REVERSE)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "direction must be SDSP_HIP_FORWARD or SDSP_HIP_REVERSE");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (n > (1u << 24))
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "FFT sizes above 2^24 are not supported");
    if (int rc = use_device(device))
        return rc;

    auto *p = new sdsp_hip_fft_plan();
    p->n = n;
    p->radix = radix;
    p->direction = direction;
    p->precision = precision;
    p->device = device;
    p->max_batch = max_batch ? max_batch : 1;
    p->real_mode = real_mode;
    // An explicit radix is the stage type that runs (radix 2: radix-2 butterflies only; radix 4: radix-4 only).  AUTO asks
    // for the fastest kernel: at N = 8192 = 2 * 4^6 that is the radix-4 machinery behind ONE radix-2 stage.
    p->allow_mix = (radix_auto && n == 8192) || radix == 4;

    int rc = SDSP_HIP_OK;
    std::vector<double> w;
    const uint32_t lds_cap_n = (uint32_t)(fft_tile_max_lds_bytes() / esize(precision));
    // double-precision plans build every table but the reported row from the correctly rounded row (host_math.cpp): the reference's
    // recipe leaves entries up to 1.85 units of 2^-53 off, which the thread-twiddle kernels multiply in once or twice per stage
    auto table_row = [&](uint32_t len) {
        if (precision == SDSP_HIP_F64)
            make_twiddles_rounded(len, direction, w);
        else
            make_twiddles(len, direction, w);
    };
    if (n > 1) {
        make_twiddles(n, direction, w);
        rc = upload_twiddles(w, precision, &p->tw);
        p->twiddle_bytes = (uint64_t)n * esize(precision);
        table_row(n);
    }
    // the optional thread-twiddle tables: where some variant of this plan's exec or convolve runs a kernel that reads them
    if (!rc && uses_twt4096(p))
        rc = upload_thread_twiddles_4096(w, radix, &p->twt);
    if (!rc && uses_twt_reg(p))
        rc = upload_thread_twiddles_reg(w, n, radix, precision, &p->twt_reg);
    if (!rc && uses_twt_big(p))
        rc = radix == 4 ? upload_thread_twiddles_big_r4(w, n, precision, &p->twt_big) : upload_thread_twiddles_big(w, n, precision, &p->twt_big);
    if (!rc && uses_twt_wave(p))
        rc = upload_thread_twiddles_wave(w, n, radix, &p->twt_wave);
    if (!rc && uses_mix(p))
        rc = upload_thread_twiddles_mix(w, n, &p->twt_mix, &p->tw_lead);
    if (n == 1) {
        p->path = PATH_NOOP;
    } else if (real_mode) { // every size on the split / merge kernels (n = 4096 f32 too: the tuned complex kernels have no split stage)
        p->path = PATH_REG;
        table_row(2 * n);
        if (!rc)
            rc = upload_twiddles(w, precision, &p->tw2); // W_2n
        p->twiddle_bytes += 2ull * n * esize(precision);
    } else if (n <= lds_cap_n) {
        if (n == 4096 && radix == 4 && precision == SDSP_HIP_F32)
            p->path = PATH_FFT4096;
        else if (precision == SDSP_HIP_F32 && fft_reg_supports(n, radix))
            p->path = PATH_REG;
        else if (precision == SDSP_HIP_F64 && fft_reg64_supports(n, radix))
            p->path = PATH_REG;
        else
            p->path = PATH_TILE;
        pick_tile(precision, n, std::max<uint32_t>(1, 1024 / n), &p->cols, &p->pitch);
        if (p->cols > 16)
            pick_tile(precision, n, 16, &p->cols, &p->pitch);
    } else {
        // N = 2^20 f32 runs the tuned two-pass kernels for either radix: a radix-4 DIF stage (fft.h:311-349) is two fused
        // radix-2 stages, so the 10 + 10 radix-2 stages of fft1m.hip are the same dataflow as ten radix-4 stages (as for
        // N = 16384 in fft_big.hip); variants >= 8 of such a plan still run genuine radix-4 stages (coverage kernel)
        p->path = (n == (1u << 20) && precision == SDSP_HIP_F32) ? PATH_FFT1M : PATH_FOUR_STEP;
        const uint32_t k = sdsp_hip_log2(n);
        if (radix == 2) {
            p->n1 = 1u << ((k + 1) / 2);
        } else {
            const uint32_t d = k / 2;
            p->n1 = 1u << (2 * ((d + 1) / 2));
        }
        p->n2 = n / p->n1;
        if (!rc) {
            table_row(p->n1);
            rc = upload_twiddles(w, precision, &p->tw1);
        }
        if (!rc) {
            table_row(p->n2);
            rc = upload_twiddles(w, precision, &p->tw2);
        }
        p->twiddle_bytes += ((uint64_t)p->n1 + p->n2) * esize(precision);
        pick_tile(precision, p->n1, 16, &p->cols1, &p->pitch1);
        pick_tile(precision, p->n2, 16, &p->cols2, &p->pitch2);
        // the tuned 2^20 path keeps 24 intermediates for the persistent kernel (8 queues x 3) / 32 for variant 1's chunks
        p->ws_batch = p->path == PATH_FFT1M ? std::min<uint64_t>(p->max_batch, 32) : p->max_batch;
        // the two-pass sizes never touch more than 256 MiB of intermediate at a time (a chunk of the two launches, the persistent
        // launch's ring): their workspace stops there instead of growing with max_batch (the alternates run in slices of it)
        if (p->path == PATH_FOUR_STEP && fft_2pass_supports(n, precision))
            p->ws_batch = std::min<uint64_t>(p->max_batch, std::max<uint64_t>(1, (1ull << 28) / ((uint64_t)n * esize(precision))));
        p->workspace_bytes = p->ws_batch * n * esize(precision); // allocated by the first exec that needs it
        if (!rc && p->path == PATH_FFT1M) {
            p->sync_count = std::min<uint64_t>(p->max_batch, kFft1mPerLaunch);
            // + one line behind the per-launch block for the sticky abort word (never touched by the per-launch memset)
            p->sticky_off = fft1m_sync_bytes(p->sync_count, (uint32_t)kFft1mQueues);
            const size_t sync_bytes = p->sticky_off + 64;
            hipError_t e = hipMalloc(&p->sync, sync_bytes);
            if (e == hipSuccess) // the abort words must read 0 before the first persistent launch (sdsp_hip_fft_plan_status)
                e = hipMemset(p->sync, 0, sync_bytes);
            if (e != hipSuccess)
                rc = fail(SDSP_HIP_ERR_NOMEM, std::string("fft1m counters hipMalloc: ") + hipGetErrorString(e));
        }
    }
    // three-pass schedule (fft_mid.hip): f32 N = 2^16 .. 2^23 (2^20 is PATH_FFT1M); f64 N = 2^14 .. 2^21 -- the rows
    // then land on the f64 register-pass family (N <= 8192) or, nested, on another three-pass plan
    if (!rc && p->path == PATH_FOUR_STEP &&
        ((precision == SDSP_HIP_F32 && n >= (1u << 16) && n <= (1u << 23)) ||
         (precision == SDSP_HIP_F64 && n >= (1u << 14) && n <= (1u << 21)))) {
        const uint32_t n2 = n / 16;
        const int sub_radix = (radix == 4 && sdsp_hip_is_power_of_4(n2)) ? 4 : 2;
        rc = sdsp_hip_fft_plan_create(&p->mid_rows, n2, sub_radix, direction, precision, p->ws_batch * 16, device);
        if (!rc) {
            table_row(1024);
            rc = upload_twiddles(w, precision, &p->tw1024);
        }
    }
    // the two-pass sizes of fft_2pass.hip: counters of the persistent schedule, where the workspace holds its ring of intermediates
    if (!rc && p->path == PATH_FOUR_STEP && fft_2pass_supports(n, precision)) {
        uint32_t unit, queues, ring, lag;
        fft_2pass_fused_shape(n, precision, &unit, &queues, &ring, &lag);
        if (unit && p->ws_batch >= (uint64_t)unit * queues * ring) {
            p->sync_count = std::min<uint64_t>((p->max_batch + unit - 1) / unit, kFused2pUnitsPerLaunch);
            p->sticky_off = fft_2pass_sync_bytes(p->sync_count, queues);
            hipError_t e = hipMalloc(&p->sync, p->sticky_off + 64);
            if (e == hipSuccess)
                e = hipMemset(p->sync, 0, p->sticky_off + 64);
            if (e != hipSuccess)
                rc = fail(SDSP_HIP_ERR_NOMEM, std::string("fft_2pass counters hipMalloc: ") + hipGetErrorString(e));
            else {
                p->f2_unit = unit;
                p->f2_queues = queues;
                p->f2_ring = ring;
                p->f2_lag = lag;
            }
        }
    }
    // plans whose DEFAULT kernel is multi-pass own their workspace from here on (no allocation on the launch path: stream
    // capture works, out-of-memory is a create-time error); single-pass defaults with multi-pass alternates stay lazy
    if (!rc && select_kernel(p, 0).workspace)
        rc = ensure_workspace(p);
    if (rc) {
        sdsp_hip_fft_plan_destroy(p);
        return rc;
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_fft_plan_create(sdsp_hip_fft_plan **out, uint32_t n, int radix, int direction, int precision,
                             uint64_t max_batch, int device)
{
    return fft_plan_create(out, n, radix, direction, precision, max_batch, device, 0);
}

int sdsp_hip_rfft_plan_create_p(sdsp_hip_fft_plan **out, uint32_t n_real, int radix, int direction, int precision,
                                uint64_t max_batch, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (!sdsp_hip_is_power_of_2(n_real) || n_real < 32)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "FFT size must be a power of 2! (real-input plans: >= 32)");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    const uint32_t n = n_real / 2;
    if (radix == 4 && !sdsp_hip_is_power_of_4(n))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "FFT radix 4 size must be a power of 4! (n_real / 2)");
    if (radix != 2 && radix != 4)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "radix must be 2 or 4");
    const bool big_real = (precision == SDSP_HIP_F32 && fft_big_real_supports(n, radix)) ||   // fft_big.hip, REAL
                          (precision == SDSP_HIP_F64 && fft_big64_real_supports(n, radix));    // fft_big64.hip, REAL
    if (!big_real && (precision == SDSP_HIP_F32 ? !fft_reg_supports(n, radix) : !fft_reg64_supports(n, radix)))
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "real-input plans cover n_real = 32 .. 32768 (f32; radix 2: .. 65536) / 32 .. 16384 (f64; radix 2: .. 32768)");
    return fft_plan_create(out, n, radix, direction, precision, max_batch, device, direction == SDSP_HIP_FORWARD ? 1 : 2);
}

int sdsp_hip_rfft_plan_create(sdsp_hip_fft_plan **out, uint32_t n_real, int radix, int direction, uint64_t max_batch,
                              int device)
{
    return sdsp_hip_rfft_plan_create_p(out, n_real, radix, direction, SDSP_HIP_F32, max_batch, device);
}

int sdsp_hip_fft_plan_destroy(sdsp_hip_fft_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (hipSetDevice(p->device) == hipSuccess) {
        (void)hipFree(p->tw);
        (void)hipFree(p->tw1);
        (void)hipFree(p->tw2);
        (void)hipFree(p->twt);
        (void)hipFree(p->twt_reg);
        (void)hipFree(p->twt_big);
        (void)hipFree(p->twt_wave);
        (void)hipFree(p->twt_mix);
        (void)hipFree(p->tw_lead);
        (void)hipFree(p->tw1024);
        (void)hipFree(p->workspace);
        (void)hipFree(p->host_stage);
        if (p->partner)
            sdsp_hip_fft_plan_destroy(p->partner);
        p->partner = nullptr;
        if (p->mid_rows)
            sdsp_hip_fft_plan_destroy(p->mid_rows);
        p->mid_rows = nullptr;
        (void)hipSetDevice(p->device);
        (void)hipFree(p->sync);
    }
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_fft_exec(sdsp_hip_fft_plan *p, void *data, uint64_t batch, void *stream)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (batch == 0)
        return SDSP_HIP_OK;
    if (!data)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "data is null");
    if ((uintptr_t)data % esize(p->precision) != 0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "data must be aligned to one complex element");
    if (int rc = use_device(p->device))
        return rc;
    if (p->sync) // this call's launches report into a clean sticky abort word
        HIP_TRY(hipMemsetAsync(fft1m_sticky(p), 0, sizeof(unsigned), reinterpret_cast<hipStream_t>(stream)));
    return fft_exec_pieces(p, data, batch, reinterpret_cast<hipStream_t>(stream), p->variant);
}

int sdsp_hip_fft_exec_host(sdsp_hip_fft_plan *p, void *host_data, uint64_t batch)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (batch == 0)
        return SDSP_HIP_OK;
    if (!host_data)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "data is null");
    if (int rc = use_device(p->device))
        return rc;
    const uint64_t bytes = batch * p->n * esize(p->precision);
    if (bytes > p->host_stage_bytes) {
        (void)hipFree(p->host_stage);
        p->host_stage = nullptr;
        p->host_stage_bytes = 0;
        hipError_t e = hipMalloc(&p->host_stage, bytes);
        if (e != hipSuccess)
            return fail(SDSP_HIP_ERR_NOMEM, std::string("staging hipMalloc: ") + hipGetErrorString(e));
        p->host_stage_bytes = bytes;
    }
    HIP_TRY(hipMemcpy(p->host_stage, host_data, bytes, hipMemcpyHostToDevice));
    if (p->sync)
        HIP_TRY(hipMemsetAsync(fft1m_sticky(p), 0, sizeof(unsigned), nullptr));
    if (int rc = fft_exec_device(p, p->host_stage, batch, nullptr, p->variant))
        return rc;
    HIP_TRY(hipMemcpy(host_data, p->host_stage, bytes, hipMemcpyDeviceToHost));
    return fft1m_check_sticky(p); // synchronous path: a launch that gave up is reported here, not only by _plan_status
}

int sdsp_hip_fft_exec_sharded(sdsp_hip_fft_plan *const *plans, int n_plans, void *host_data, uint64_t batch)
{
    if (!plans || n_plans <= 0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "no plans");
    for (int i = 0; i < n_plans; i++) {
        if (!plans[i])
            return fail(SDSP_HIP_ERR_INVALID_ARG, "null plan in shard list");
        if (plans[i]->n != plans[0]->n || plans[i]->radix != plans[0]->radix ||
            plans[i]->direction != plans[0]->direction || plans[i]->precision != plans[0]->precision)
            return fail(SDSP_HIP_ERR_INVALID_ARG, "shard plans must describe the same transform");
    }
    if (batch == 0)
        return SDSP_HIP_OK;
    if (!host_data)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "data is null");
    // contiguous ranges [g*B/G, (g+1)*B/G): independent transforms, no exchange step
    const size_t per = (size_t)plans[0]->n * esize(plans[0]->precision);
    std::vector<int> rcs(n_plans, 0);
    std::vector<std::string> errs(n_plans);
    std::vector<std::thread> th;
    for (int g = 0; g < n_plans; g++) {
        const uint64_t lo = batch * g / n_plans, hi = batch * (g + 1) / n_plans;
        th.emplace_back([=, &rcs, &errs] {
            rcs[g] = sdsp_hip_fft_exec_host(plans[g], reinterpret_cast<char *>(host_data) + lo * per, hi - lo);
            if (rcs[g])
                errs[g] = g_last_error;
        });
    }
    for (auto &t : th)
        t.join();
    for (int g = 0; g < n_plans; g++)
        if (rcs[g])
            return fail(rcs[g], errs[g]);
    return SDSP_HIP_OK;
}

int sdsp_hip_fft_convolve(sdsp_hip_fft_plan *p, void *data, const void *h, uint64_t batch, void *stream)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (p->direction != SDSP_HIP_FORWARD)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "convolve needs a forward plan");
    if (batch == 0)
        return SDSP_HIP_OK;
    if (!data || !h)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null pointer");
    if (p->real_mode) // a real-input plan's transform is not the complex DFT the product is defined on
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "convolve needs a complex plan (real-input plans are not supported)");
    if (int rc = use_device(p->device))
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // this call's launches report into clean sticky abort words (the persistent two-pass kernels; forward and reverse half)
    if (p->sync)
        HIP_TRY(hipMemsetAsync(fft1m_sticky(p), 0, sizeof(unsigned), s));
    if (p->partner && p->partner->sync)
        HIP_TRY(hipMemsetAsync(fft1m_sticky(p->partner), 0, sizeof(unsigned), s));
    const fft_kernel_sel sel = select_conv(p, p->variant);
    if (sel.conv) {
        if (int rc = check_table(p, sel))
            return rc;
    } else if (!p->partner) { // the reverse half of the three launches
        if (int rc = sdsp_hip_fft_plan_create(&p->partner, p->n, p->radix, SDSP_HIP_REVERSE, p->precision, p->max_batch, p->device))
            return rc;
        p->partner->wait_limit = p->wait_limit;
    }
    const bool fused_mul = sel.id == K_2PASS || sel.id == K_2PASS_FUSED; // the forward transform's pass 2 multiplies by h
    const uint64_t row_bytes = (uint64_t)p->n * esize(p->precision);
    const uint64_t piece = fft_piece(p, sel, batch);
    for (uint64_t done = 0; done < batch; done += piece) {
        char *d = static_cast<char *>(data) + done * row_bytes;
        const uint64_t nb = std::min(piece, batch - done);
        int rc;
        if (sel.conv) {
            rc = sel.launch ? launch_reg(p, sel, d, nb, s, h) : launch_fft4096_conv_f32(d, p->twt, h, nb, stream);
        } else {
            rc = fft_exec_device(p, d, nb, s, sel.variant, fused_mul ? h : nullptr);
            if (!rc && !fused_mul)
                rc = launch_pointwise_mul(p->precision, d, h, p->n, nb, stream);
            if (!rc)
                rc = fft_exec_device(p->partner, d, nb, s, p->partner->variant);
        }
        if (rc)
            return rc;
    }
    return SDSP_HIP_OK;
}

int sdsp_hip_fft_plan_get_info(const sdsp_hip_fft_plan *p, sdsp_hip_fft_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->n = p->n;
    info->radix = p->radix;
    info->direction = p->direction;
    info->precision = p->precision;
    info->device = p->device;
    const fft_kernel_sel sel = select_kernel(p, p->variant); // the same table sdsp_hip_fft_exec dispatches on
    info->hbm_passes = sel.hbm_passes;
    info->stage_radix = sel.stage_radix;
    info->algorithmic_bytes = 2ull * p->n * esize(p->precision); // real plans: n complex = n_real floats, same bytes
    info->workspace_bytes = p->workspace_bytes;
    info->twiddle_bytes = p->twiddle_bytes;
    const char *name = sel.name;
    std::strncpy(info->kernel, name, sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_fft_plan_status(sdsp_hip_fft_plan *p)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (int rc = use_device(p->device))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = fft1m_check_sticky(p))
        return rc;
    // sdsp_hip_fft_convolve runs its reverse half on the plan's partner: a hand-off lost there belongs to this plan's last call too
    return p->partner ? fft1m_check_sticky(p->partner) : SDSP_HIP_OK;
}

int sdsp_hip_fft_plan_set_wait_limit(sdsp_hip_fft_plan *p, uint64_t ticks)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    p->wait_limit = ticks;
    if (p->partner)
        p->partner->wait_limit = ticks;
    return SDSP_HIP_OK;
}

int sdsp_hip_fft_plan_launches(const sdsp_hip_fft_plan *p, uint64_t batch, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = fft_launch_count(p, batch, p->variant);
    return SDSP_HIP_OK;
}

int sdsp_hip_set_launch_piece_bytes(uint64_t bytes)
{
    g_piece_bytes.store(bytes, std::memory_order_relaxed);
    return SDSP_HIP_OK;
}

int sdsp_hip_get_launch_piece_bytes(uint64_t *bytes)
{
    if (!bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "bytes is null");
    *bytes = g_piece_bytes.load(std::memory_order_relaxed);
    return SDSP_HIP_OK;
}

int sdsp_hip_fft_plan_get_twiddles(const sdsp_hip_fft_plan *p, void *host_out)
{
    if (!p || !host_out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    if (!p->tw)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "plan has no twiddle table");
    if (int rc = use_device(p->device))
        return rc;
    HIP_TRY(hipMemcpy(host_out, p->tw, (size_t)p->n * esize(p->precision), hipMemcpyDeviceToHost));
    return SDSP_HIP_OK;
}

int sdsp_hip_fft_plan_set_variant(sdsp_hip_fft_plan *p, int variant)
{
    if (!p || variant < 0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "bad argument");
    p->variant = variant;
    return SDSP_HIP_OK;
}

// ------------------------------------------------------------------ IIR banks

int sdsp_hip_iir_plan_create(sdsp_hip_iir_plan **out, uint32_t sections, int kind, const double *a,
                             const double *b, double gain, int precision, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (sections == 0 || sections % 2 != 0) // static_assert casc_2o_iir.h:25
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "M must be even!");
    if (sections > SDSP_HIP_MAX_SECTIONS) // 2 .. 8: the tuned kernels; 10 .. 16: the direct kernel
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "at most SDSP_HIP_MAX_SECTIONS (16) sections are compiled in");
    if (kind < SDSP_HIP_IIR_GENERIC || kind > SDSP_HIP_IIR_BP)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "unknown IIR kind");
    if (!a || (kind == SDSP_HIP_IIR_GENERIC && !b))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "coefficient pointer is null");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64 && precision != SDSP_HIP_F32_F64STATE)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32, SDSP_HIP_F64 or SDSP_HIP_F32_F64STATE");
    if (int rc = use_device(device))
        return rc;
    auto *p = new sdsp_hip_iir_plan();
    p->sections = sections;
    p->kind = kind;
    p->precision = precision;
    p->device = device;
    p->gain = gain;
    std::memcpy(p->a, a, sizeof(double) * 3 * sections);
    if (b)
        std::memcpy(p->b, b, sizeof(double) * 3 * sections);
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_iir_plan_destroy(sdsp_hip_iir_plan *p)
{
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_iir_state_bytes(const sdsp_hip_iir_plan *p, uint64_t channels, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = 3ull * (p->sections + 1) * channels * (p->precision == SDSP_HIP_F32 ? 4 : 8);
    return SDSP_HIP_OK;
}

int sdsp_hip_iir_plan_set_variant(sdsp_hip_iir_plan *p, int variant)
{
    if (!p || variant < 0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "bad argument");
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_iir_process(sdsp_hip_iir_plan *p, void *data, uint64_t channels, uint64_t samples, uint64_t stride,
                         void *state, void *stream)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (!data)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "data is null");
    if (stride < samples && channels > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "stride must be >= samples");
    if (int rc = use_device(p->device))
        return rc;
    iir_args a{};
    a.data = data;
    a.state = state;
    a.channels = channels;
    a.samples = samples;
    a.stride = stride;
    a.sections = p->sections;
    a.kind = p->kind;
    a.gain = p->gain;
    for (uint32_t j = 0; j < p->sections; j++) {
        a.a1[j] = p->a[3 * j + 1];
        a.a2[j] = p->a[3 * j + 2];
        a.b1[j] = p->b[3 * j + 1];
        a.b2[j] = p->b[3 * j + 2];
    }
    return launch_iir(p->precision, a, p->variant, stream);
}

int sdsp_hip_iir_plan_kernel(const sdsp_hip_iir_plan *p, const void *data, uint64_t channels, uint64_t samples, uint64_t stride,
                             char *name, size_t name_bytes)
{
    if (!p || !name || name_bytes == 0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    iir_args a{};
    a.data = const_cast<void *>(data);
    a.channels = channels;
    a.samples = samples;
    a.stride = stride;
    a.sections = p->sections;
    a.kind = p->kind;
    std::strncpy(name, iir_kernel_for(p->precision, a, p->variant), name_bytes - 1);
    name[name_bytes - 1] = 0;
    return SDSP_HIP_OK;
}

int sdsp_hip_iir_process_interleaved(sdsp_hip_iir_plan *p, void *data, uint64_t channels, uint64_t samples,
                                     uint64_t stride, void *state, void *stream)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (!data)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "data is null");
    if (stride < channels && samples > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "stride must be >= channels");
    if (int rc = use_device(p->device))
        return rc;
    iir_args a{};
    a.data = data;
    a.state = state;
    a.channels = channels;
    a.samples = samples;
    a.stride = stride;
    a.sections = p->sections;
    a.kind = p->kind;
    a.gain = p->gain;
    for (uint32_t j = 0; j < p->sections; j++) {
        a.a1[j] = p->a[3 * j + 1];
        a.a2[j] = p->a[3 * j + 2];
        a.b1[j] = p->b[3 * j + 1];
        a.b2[j] = p->b[3 * j + 2];
    }
    return launch_iir_interleaved(p->precision, a, p->variant, stream);
}

int sdsp_hip_iir_process_host(sdsp_hip_iir_plan *p, void *host_data, uint64_t channels, uint64_t samples,
                              uint64_t stride, void *host_state)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (!host_data)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "data is null");
    if (int rc = use_device(p->device))
        return rc;
    const size_t rs = real_size(p->precision); // sample size (the mixed mode stores floats)
    const size_t data_bytes = ((channels - 1) * stride + samples) * rs;
    uint64_t state_bytes = 0;
    sdsp_hip_iir_state_bytes(p, channels, &state_bytes);
    host_stage st("iir", { { host_data, data_bytes, true }, { host_state, state_bytes, true } });
    int rc = st.in();
    if (!rc)
        rc = sdsp_hip_iir_process(p, st.dev[0], channels, samples, stride, st.dev[1], nullptr);
    return st.out(rc);
}

int sdsp_hip_iir_process_sharded(sdsp_hip_iir_plan *const *plans, int n_plans, void *host_data, uint64_t channels,
                                 uint64_t samples)
{
    if (!plans || n_plans <= 0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "no plans");
    for (int i = 0; i < n_plans; i++)
        if (!plans[i] || plans[i]->precision != plans[0]->precision || plans[i]->sections != plans[0]->sections)
            return fail(SDSP_HIP_ERR_INVALID_ARG, "shard plans must describe the same filter bank");
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (!host_data)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "data is null");
    const size_t row = samples * real_size(plans[0]->precision);
    std::vector<int> rcs(n_plans, 0);
    std::vector<std::string> errs(n_plans);
    std::vector<std::thread> th;
    for (int g = 0; g < n_plans; g++) {
        const uint64_t lo = channels * g / n_plans, hi = channels * (g + 1) / n_plans;
        th.emplace_back([=, &rcs, &errs] {
            rcs[g] = sdsp_hip_iir_process_host(plans[g], reinterpret_cast<char *>(host_data) + lo * row, hi - lo,
                                               samples, samples, nullptr);
            if (rcs[g])
                errs[g] = g_last_error;
        });
    }
    for (auto &t : th)
        t.join();
    for (int g = 0; g < n_plans; g++)
        if (rcs[g])
            return fail(rcs[g], errs[g]);
    return SDSP_HIP_OK;
}
// ------------------------------------------------------------------ FIR banks

int sdsp_hip_fir_plan_create(sdsp_hip_fir_plan **out, uint32_t taps, const double *h, int precision, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (taps == 0 || taps > SDSP_HIP_FIR_MAX_TAPS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps must be in [1, SDSP_HIP_FIR_MAX_TAPS]");
    if (!h)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "coefficient pointer is null");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (int rc = use_device(device))
        return rc;
    auto *p = new sdsp_hip_fir_plan();
    p->taps = taps;
    p->precision = precision;
    p->device = device;
    const hipError_t e = upload_reals(h, taps, precision, &p->h_dev);
    if (e != hipSuccess) {
        (void)hipFree(p->h_dev);
        delete p;
        return hip_fail(e, "fir coefficients");
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_fir_plan_destroy(sdsp_hip_fir_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK) {
        (void)hipFree(p->h_dev);
        (void)hipFree(p->H);
        (void)hipFree(p->ws);
        (void)hipFree(p->carry);
    }
    if (p->conv)
        sdsp_hip_fft_plan_destroy(p->conv);
    delete p;
    return SDSP_HIP_OK;
}

// ------------------------------------------------------------------ FFT-domain FIR plans (overlap-save)

namespace
{
// frame pairs + staged history of one slice.  Measured (tools/bench_fir_fft.py): 16 / 32 / 64 / 128 / 256 /
// 512 MiB, f32 1024 taps 98.8 / 74.5 / 56.6 / 49.9 / 47.9 / 49.0 ms, f64 1024 taps 109 / 70.1 / 49.1 / 44.9 / 41.8 / 41.4 ms: fewer,
// longer slices win; keeping a slice inside the Infinity Cache (<= 128 MiB) does not
constexpr uint64_t kFirFftDefaultBudget = 256ull << 20;
// auto fft_n: the smallest power of two >= 4 taps, but not above 4096 unless 2 (taps - 1) needs it.  Measured on 4096-sample rows
// (DESIGN.md section 5.9): 1024 taps N = 2048 / 4096 / 8192 / 16384: 53.0 / 49.9 / 85.1 / 189 ms; 4096 taps N = 8192 / 16384 / 32768:
// 93.7 / 200 / 445 ms -- the fused convolution slows down above N = 4096 and short rows pay for the padding of a large frame
constexpr uint32_t kFirFftAutoRatio = 4, kFirFftAutoCap = 4096;

uint32_t fir_fft_max_taps(int precision) { return precision == SDSP_HIP_F64 ? SDSP_HIP_FIR_FFT_MAX_TAPS_F64 : SDSP_HIP_FIR_FFT_MAX_TAPS; }
// the fused convolution's range on radix-2 plans (sdsp_hip_fft_convolve)
uint32_t fir_fft_max_n(int precision) { return precision == SDSP_HIP_F64 ? 16384u : 32768u; }
constexpr uint32_t kFirFftMinN = 16;

// what the plan's inner convolution needs for its current variant, allocated now so that process never allocates: the
// three-launch composition's reverse partner and the multi-pass workspaces
int fir_fft_prepare_conv(sdsp_hip_fir_plan *p)
{
    sdsp_hip_fft_plan *c = p->conv;
    const fft_kernel_sel sel = select_conv(c, c->variant);
    if (sel.conv)
        return SDSP_HIP_OK;
    if (!c->partner) {
        if (int rc = sdsp_hip_fft_plan_create(&c->partner, c->n, c->radix, SDSP_HIP_REVERSE, c->precision, c->max_batch, c->device))
            return rc;
        c->partner->wait_limit = c->wait_limit;
    }
    if (select_kernel(c, sel.variant).workspace)
        if (int rc = ensure_workspace(c))
            return rc;
    if (select_kernel(c->partner, c->partner->variant).workspace)
        if (int rc = ensure_workspace(c->partner))
            return rc;
    return SDSP_HIP_OK;
}

// kernel launches of sdsp_hip_fft_convolve(c, ., ., batch) -- the same loop
uint64_t conv_launch_count(const sdsp_hip_fft_plan *c, uint64_t batch)
{
    const fft_kernel_sel sel = select_conv(c, c->variant);
    const bool fused_mul = sel.id == K_2PASS || sel.id == K_2PASS_FUSED;
    const uint64_t piece = fft_piece(c, sel, batch);
    uint64_t n = 0;
    for (uint64_t done = 0; done < batch; done += piece) {
        const uint64_t nb = std::min(piece, batch - done);
        if (sel.conv)
            n += 1;
        else
            n += fft_launch_count(c, nb, sel.variant, false) + (fused_mul ? 0 : 1) +
                 (c->partner ? fft_launch_count(c->partner, nb, c->partner->variant, false) : 0);
    }
    return n;
}

// the stream's frame grid: F frames, P pairs per channel
void fir_fft_grid(const sdsp_hip_fir_plan *p, uint64_t samples, uint64_t *frames, uint64_t *pairs)
{
    *frames = (samples + p->hop - 1) / p->hop;
    *pairs = (*frames + 1) / 2;
}

// H = FFT(h zero-padded to n) in double (iterative radix 2 on the library's own twiddle row), natural order
std::vector<double> fir_fft_response(const double *h, uint32_t taps, uint32_t n)
{
    std::vector<double> x(2 * static_cast<size_t>(n), 0.0), w(2 * static_cast<size_t>(n));
    for (uint32_t i = 0; i < taps; i++)
        x[2 * i] = h[i];
    sdsp_hip_calc_twiddles(n, SDSP_HIP_FORWARD, w.data());
    const uint32_t lg = sdsp_hip_log2(n);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t r = 0;
        for (uint32_t b = 0; b < lg; b++)
            r |= ((i >> b) & 1u) << (lg - 1 - b);
        if (r > i) {
            std::swap(x[2 * i], x[2 * r]);
            std::swap(x[2 * i + 1], x[2 * r + 1]);
        }
    }
    for (uint32_t len = 2; len <= n; len <<= 1) {
        const uint32_t half = len / 2, step = n / len;
        for (uint32_t s0 = 0; s0 < n; s0 += len)
            for (uint32_t j = 0; j < half; j++) {
                const double wr = w[2 * (j * step)], wi = w[2 * (j * step) + 1];
                double *a = &x[2 * (s0 + j)], *b = &x[2 * (s0 + j + half)];
                const double tr = b[0] * wr - b[1] * wi, ti = b[0] * wi + b[1] * wr;
                b[0] = a[0] - tr;
                b[1] = a[1] - ti;
                a[0] += tr;
                a[1] += ti;
            }
    }
    return x;
}

int fir_fft_process(sdsp_hip_fir_plan *p, void *data, uint64_t channels, uint64_t samples, uint64_t stride, void *state, void *stream)
{
    const size_t rs = real_size(p->precision);
    const uint32_t t1 = p->taps - 1;
    uint64_t frames = 0, pairs = 0;
    fir_fft_grid(p, samples, &frames, &pairs);
    if (channels > ~0ull / pairs)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many frames for one call");
    const uint64_t total = channels * pairs;
    char *tails = static_cast<char *>(p->ws) + p->ws_units * p->fft_n * 2 * rs;
    fir_os_args a{};
    a.data = data;
    a.state = t1 ? state : nullptr;
    a.ws = p->ws;
    a.tails = a.state ? tails : nullptr;
    a.stride = stride;
    a.samples = samples;
    a.frames = frames;
    a.pairs = pairs;
    a.n = p->fft_n;
    a.hop = p->hop;
    a.taps_m1 = t1;
    uint64_t k = 0;
    for (uint64_t g0 = 0; g0 < total; g0 += p->ws_units, k++) {
        a.g0 = g0;
        a.units = std::min(p->ws_units, total - g0);
        a.carry_in = static_cast<char *>(p->carry) + ((k + 1) & 1) * t1 * rs;
        a.carry_out = static_cast<char *>(p->carry) + (k & 1) * t1 * rs;
        if (int rc = launch_fir_os(p->precision, a, FIR_OS_FRAME, stream))
            return rc;
        if (int rc = sdsp_hip_fft_convolve(p->conv, p->ws, p->H, a.units, stream))
            return rc;
        if (int rc = launch_fir_os(p->precision, a, FIR_OS_SCATTER, stream))
            return rc;
        if (a.state)
            if (int rc = launch_fir_os(p->precision, a, FIR_OS_STATE, stream))
                return rc;
    }
    return SDSP_HIP_OK;
}
} // namespace

int sdsp_hip_fir_fft_size(uint32_t taps, int precision, uint32_t *fft_n)
{
    if (!fft_n)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "fft_n is null");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (taps == 0 || taps > fir_fft_max_taps(precision))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps must be in [1, SDSP_HIP_FIR_FFT_MAX_TAPS] (f64: SDSP_HIP_FIR_FFT_MAX_TAPS_F64)");
    const uint64_t want = std::max<uint64_t>(2ull * (taps - 1), std::min<uint64_t>(static_cast<uint64_t>(kFirFftAutoRatio) * taps, kFirFftAutoCap));
    uint32_t n = kFirFftMinN;
    while (n < want && n < fir_fft_max_n(precision))
        n <<= 1;
    *fft_n = n; // >= 2 (taps - 1): the clamp only binds where 2 x max taps = max n
    return SDSP_HIP_OK;
}

int sdsp_hip_fir_fft_plan_create(sdsp_hip_fir_plan **out, uint32_t taps, const double *h, int precision, uint32_t fft_n,
                                 uint64_t workspace_bytes, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (!h)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "coefficient pointer is null");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (taps == 0 || taps > fir_fft_max_taps(precision))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps must be in [1, SDSP_HIP_FIR_FFT_MAX_TAPS] (f64: SDSP_HIP_FIR_FFT_MAX_TAPS_F64)");
    if (fft_n == 0) {
        if (int rc = sdsp_hip_fir_fft_size(taps, precision, &fft_n))
            return rc;
    } else {
        if (!sdsp_hip_is_power_of_2(fft_n) || fft_n < 2ull * (taps - 1))
            return fail(SDSP_HIP_ERR_INVALID_SIZE, "fft_n must be a power of 2 and >= 2 (taps - 1)");
        if (fft_n < kFirFftMinN || fft_n > fir_fft_max_n(precision))
            return fail(SDSP_HIP_ERR_UNSUPPORTED, "fft_n must be in the fused convolution's range (f32 16 .. 32768, f64 16 .. 16384)");
    }
    if (int rc = use_device(device))
        return rc;
    const size_t rs = real_size(precision);
    const uint64_t unit_bytes = 2ull * fft_n * rs + static_cast<uint64_t>(taps - 1) * rs; // one frame pair + its staged history
    const uint64_t budget = workspace_bytes ? workspace_bytes : kFirFftDefaultBudget;
    auto *p = new sdsp_hip_fir_plan();
    p->taps = taps;
    p->precision = precision;
    p->device = device;
    p->method = SDSP_HIP_FIR_FFT;
    p->fft_n = fft_n;
    p->hop = fft_n - taps + 1;
    p->ws_units = std::max<uint64_t>(1, budget / unit_bytes);
    p->workspace_bytes = p->ws_units * unit_bytes + 2ull * (taps - 1) * rs;
    int rc = sdsp_hip_fft_plan_create(&p->conv, fft_n, 2, SDSP_HIP_FORWARD, precision, p->ws_units, device);
    if (!rc && !select_conv(p->conv, 0).conv)
        rc = fail(SDSP_HIP_ERR_UNSUPPORTED, "no fused convolution for this fft_n");
    if (!rc) {
        hipError_t e = hipMalloc(&p->ws, p->ws_units * unit_bytes);
        if (e == hipSuccess)
            e = hipMalloc(&p->carry, std::max<size_t>(1, 2ull * (taps - 1) * rs));
        // coefficients and response rounded once to the plan precision (the twiddle-table convention)
        if (e == hipSuccess)
            e = upload_reals(h, taps, precision, &p->h_dev);
        if (e == hipSuccess) {
            const std::vector<double> resp = fir_fft_response(h, taps, fft_n); // fft_n complex values, re and im interleaved
            e = upload_reals(resp.data(), resp.size(), precision, &p->H);
        }
        if (e != hipSuccess)
            rc = plan_fail(e, "fir fft");
    }
    if (rc) {
        sdsp_hip_fir_plan_destroy(p);
        return rc;
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_fir_plan_get_info(const sdsp_hip_fir_plan *p, sdsp_hip_fir_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->taps = p->taps;
    info->precision = p->precision;
    info->device = p->device;
    info->method = p->method;
    info->fft_n = p->fft_n;
    info->hop = p->hop;
    info->workspace_bytes = p->workspace_bytes;
    const char *name = p->method == SDSP_HIP_FIR_FFT ? select_conv(p->conv, p->conv->variant).name : "sdsp_fir_kernel";
    std::strncpy(info->kernel, name, sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_fir_plan_launches(const sdsp_hip_fir_plan *p, uint64_t channels, uint64_t samples, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = 0;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (p->method != SDSP_HIP_FIR_FFT) {
        *launches = 1;
        return SDSP_HIP_OK;
    }
    uint64_t frames = 0, pairs = 0;
    fir_fft_grid(p, samples, &frames, &pairs);
    const uint64_t total = channels * pairs;
    uint64_t n = 0;
    for (uint64_t g0 = 0; g0 < total; g0 += p->ws_units) {
        const uint64_t g1 = std::min(total, g0 + p->ws_units);
        n += 2 + conv_launch_count(p->conv, g1 - g0);
        if (p->taps > 1 && g1 / pairs > g0 / pairs) // a channel ends in this slice: the state launch
            n += 1;
    }
    *launches = n;
    return SDSP_HIP_OK;
}

int sdsp_hip_fir_state_bytes(const sdsp_hip_fir_plan *p, uint64_t channels, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = static_cast<uint64_t>(p->taps - 1) * channels * real_size(p->precision);
    return SDSP_HIP_OK;
}

int sdsp_hip_fir_plan_set_variant(sdsp_hip_fir_plan *p, int variant)
{
    if (!p || variant < 0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "bad argument");
    p->variant = variant;
    if (p->method != SDSP_HIP_FIR_FFT)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    p->conv->variant = variant;
    return fir_fft_prepare_conv(p);
}

int sdsp_hip_fir_process(sdsp_hip_fir_plan *p, void *data, uint64_t channels, uint64_t samples, uint64_t stride,
                         void *state, void *stream)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (!data)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "data is null");
    if (stride < samples && channels > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "stride must be >= samples");
    if (int rc = use_device(p->device))
        return rc;
    if (p->method == SDSP_HIP_FIR_FFT)
        return fir_fft_process(p, data, channels, samples, stride, state, stream);
    fir_args a{};
    a.data = data;
    a.state = p->taps > 1 ? state : nullptr;
    a.h = p->h_dev;
    a.channels = channels;
    a.samples = samples;
    a.stride = stride;
    a.taps = p->taps;
    return launch_fir(p->precision, a, p->variant, stream);
}

int sdsp_hip_fir_process_host(sdsp_hip_fir_plan *p, void *host_data, uint64_t channels, uint64_t samples,
                              uint64_t stride, void *host_state)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (!host_data)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "data is null");
    if (int rc = use_device(p->device))
        return rc;
    const size_t data_bytes = ((channels - 1) * stride + samples) * real_size(p->precision);
    uint64_t state_bytes = 0;
    sdsp_hip_fir_state_bytes(p, channels, &state_bytes);
    const bool with_state = host_state && state_bytes;
    host_stage st("fir", { { host_data, data_bytes, true }, { with_state ? host_state : nullptr, state_bytes, true } });
    int rc = st.in();
    if (!rc)
        rc = sdsp_hip_fir_process(p, st.dev[0], channels, samples, stride, st.dev[1], nullptr);
    return st.out(rc);
}

// ------------------------------------------------------------------ polyphase FIR resampler banks (fir_resample.hip)

int sdsp_hip_resample_plan_create(sdsp_hip_resample_plan **out, uint32_t taps, const double *h, uint32_t up, uint32_t down,
                                  int precision, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (taps == 0 || taps > SDSP_HIP_FIR_MAX_TAPS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps must be in [1, SDSP_HIP_FIR_MAX_TAPS]");
    if (up == 0 || down == 0 || up > SDSP_HIP_RESAMPLE_MAX_FACTOR || down > SDSP_HIP_RESAMPLE_MAX_FACTOR)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "up and down must be in [1, SDSP_HIP_RESAMPLE_MAX_FACTOR]");
    if (!h)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "coefficient pointer is null");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (int rc = use_device(device))
        return rc;
    auto *p = new sdsp_hip_resample_plan();
    uint32_t g = up, b = down;
    while (b) {
        const uint32_t t = g % b;
        g = b;
        b = t;
    }
    p->taps = taps;
    p->up = up;
    p->down = down;
    p->q = down / g;
    p->hist = (taps - 1) / up;
    p->precision = precision;
    p->device = device;
    const hipError_t e = upload_reals(h, taps, precision, &p->h_dev);
    if (e != hipSuccess) {
        (void)hipFree(p->h_dev);
        delete p;
        return hip_fail(e, "resample coefficients");
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_resample_plan_destroy(sdsp_hip_resample_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK)
        (void)hipFree(p->h_dev);
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_resample_state_bytes(const sdsp_hip_resample_plan *p, uint64_t channels, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = static_cast<uint64_t>(p->hist) * channels * real_size(p->precision);
    return SDSP_HIP_OK;
}

int sdsp_hip_resample_plan_set_variant(sdsp_hip_resample_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 2)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0, 1 or 2");
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_resample_plan_get_info(const sdsp_hip_resample_plan *p, sdsp_hip_resample_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->taps = p->taps;
    info->up = p->up;
    info->down = p->down;
    info->hist = p->hist;
    info->precision = p->precision;
    info->device = p->device;
    resample_args a{};
    a.taps = p->taps;
    a.up = p->up;
    a.down = p->down;
    a.channels = 1;
    a.samples = 4096ull * p->q;
    std::strncpy(info->kernel, resample_kernel_for(p->precision, a, p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_resample_process(sdsp_hip_resample_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride,
                              uint64_t channels, uint64_t samples, void *state, void *stream)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    uint64_t outs = 0;
    if (int rc = sdsp_hip_resample_out_samples(p->up, p->down, samples, &outs))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (!in || !out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in or out is null");
    if (channels > 1 && (in_stride < samples || out_stride < outs))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_stride must be >= samples and out_stride >= samples * up / down");
    const uint64_t rs = real_size(p->precision);
    if (ranges_overlap(in, ((channels - 1) * in_stride + samples) * rs, out, ((channels - 1) * out_stride + outs) * rs))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in and out ranges overlap (the resampler runs out of place)");
    if (int rc = use_device(p->device))
        return rc;
    resample_args a{};
    a.in = in;
    a.out = out;
    a.state = p->hist ? state : nullptr;
    a.h = p->h_dev;
    a.channels = channels;
    a.samples = samples;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.taps = p->taps;
    a.up = p->up;
    a.down = p->down;
    return launch_resample(p->precision, a, p->variant, stream);
}

int sdsp_hip_resample_process_host(sdsp_hip_resample_plan *p, const void *host_in, uint64_t in_stride, void *host_out,
                                   uint64_t out_stride, uint64_t channels, uint64_t samples, void *host_state)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    uint64_t outs = 0;
    if (int rc = sdsp_hip_resample_out_samples(p->up, p->down, samples, &outs))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (!host_in || !host_out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in or out is null");
    if (channels > 1 && (in_stride < samples || out_stride < outs))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_stride must be >= samples and out_stride >= samples * up / down");
    if (int rc = use_device(p->device))
        return rc;
    const size_t rs = real_size(p->precision);
    const size_t in_bytes = ((channels - 1) * in_stride + samples) * rs;
    const size_t out_bytes = ((channels - 1) * out_stride + outs) * rs;
    uint64_t state_bytes = 0;
    sdsp_hip_resample_state_bytes(p, channels, &state_bytes);
    const bool with_state = host_state && state_bytes;
    host_stage st("resample", { { host_in, in_bytes, false }, { host_out, out_bytes, true },
                            { with_state ? host_state : nullptr, state_bytes, true } });
    int rc = st.in();
    if (!rc)
        rc = sdsp_hip_resample_process(p, st.dev[0], in_stride, st.dev[1], out_stride, channels, samples, st.dev[2], nullptr);
    return st.out(rc);
}

// ------------------------------------------------------------------ STFT banks (stft.hip)

namespace
{
// windowed frames of one slice (transformed in place).  Measured (tools/bench_stft.py), f32 N = 1024,
// hop = 256, complex, 1 GiB in: 16 / 64 / 128 / 256 / 512 / 1024 MiB 7.73 / 4.87 / 4.73 / 4.64 / 4.62 / 4.64 ms -- flat from 256 MiB on
constexpr uint64_t kStftDefaultBudget = 256ull << 20;

uint32_t stft_max_n(int precision) { return precision == SDSP_HIP_F64 ? 32768u : 65536u; }

// create-time checks the STFT, inverse STFT and Welch banks share; each runs its own between the two
int check_frame_shape(uint32_t n_fft, uint32_t hop, const double *window, int precision)
{
    if (!sdsp_hip_is_power_of_2(n_fft))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "n_fft must be a power of 2");
    if (hop == 0 || hop > n_fft)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "hop must be in [1, n_fft]");
    if (!window)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "window pointer is null");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    return SDSP_HIP_OK;
}
int check_real_input_range(uint32_t n_fft, int precision)
{
    if (n_fft < 32 || n_fft > stft_max_n(precision))
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "n_fft must be in the radix-2 real-input range (f32 32 .. 65536, f64 32 .. 32768)");
    return SDSP_HIP_OK;
}

int stft_run(sdsp_hip_stft_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t channels,
             uint64_t samples, void *state, hipStream_t stream)
{
    const uint64_t frames = samples / p->hop;
    if (frames >= (1ull << 31))
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many frames per channel for one call");
    if (channels > ~0ull / frames)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many frames for one call");
    const uint64_t total = channels * frames;
    stft_args a{};
    a.in = in;
    a.out = out;
    a.state = p->hist ? state : nullptr;
    a.window = p->window;
    a.ws = p->ws;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.frames = static_cast<uint32_t>(frames);
    a.n = p->n;
    a.hop = p->hop;
    a.hist = p->hist;
    a.output = p->output;
    for (uint64_t g0 = 0; g0 < total; g0 += p->ws_units) {
        a.g0 = g0;
        a.units = static_cast<uint32_t>(std::min(p->ws_units, total - g0));
        if (int rc = launch_stft(p->precision, a, STFT_FRAME, stream))
            return rc;
        if (int rc = fft_exec_pieces(p->inner, p->ws, a.units, stream, p->inner->variant))
            return rc;
        if (int rc = launch_stft(p->precision, a, STFT_EMIT, stream))
            return rc;
    }
    // after every frame launch: they may read the old history
    return carry_history(p->precision, real_size(p->precision), in, in_stride, state, channels, samples, p->hist, stream, "stft");
}

// argument checks shared by process and process_host (device pointers or not)
int stft_check(const sdsp_hip_stft_plan *p, const void *in, uint64_t in_stride, const void *out, uint64_t out_stride,
               uint64_t channels, uint64_t samples, uint64_t *frames)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (int rc = sdsp_hip_stft_frames(p->hop, samples, frames))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (!in || !out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in or out is null");
    if (channels > 1 && (in_stride < samples || out_stride < *frames * p->bins))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_stride must be >= samples and out_stride >= frames * bins");
    return SDSP_HIP_OK;
}

uint64_t stft_out_esize(const sdsp_hip_stft_plan *p)
{
    return p->output == SDSP_HIP_STFT_COMPLEX ? esize(p->precision) : real_size(p->precision);
}
} // namespace

int sdsp_hip_stft_plan_create(sdsp_hip_stft_plan **out, uint32_t n_fft, uint32_t hop, const double *window, int output,
                              int precision, uint64_t workspace_bytes, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (int rc = check_frame_shape(n_fft, hop, window, precision))
        return rc;
    if (output != SDSP_HIP_STFT_COMPLEX && output != SDSP_HIP_STFT_POWER && output != SDSP_HIP_STFT_MAGNITUDE)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "output must be SDSP_HIP_STFT_COMPLEX, _POWER or _MAGNITUDE");
    if (int rc = check_real_input_range(n_fft, precision))
        return rc;
    if (int rc = use_device(device))
        return rc;
    const uint64_t unit_bytes = static_cast<uint64_t>(n_fft) * real_size(precision);
    const uint64_t budget = workspace_bytes ? workspace_bytes : kStftDefaultBudget;
    auto *p = new sdsp_hip_stft_plan();
    p->n = n_fft;
    p->hop = hop;
    p->hist = n_fft - hop;
    p->bins = n_fft / 2 + 1;
    p->output = output;
    p->precision = precision;
    p->device = device;
    p->ws_units = slice_units(budget, unit_bytes);
    p->workspace_bytes = p->ws_units * unit_bytes;
    int rc = fft_plan_create(&p->inner, n_fft / 2, 2, SDSP_HIP_FORWARD, precision, p->ws_units, device, 1);
    if (!rc) {
        hipError_t e = hipMalloc(&p->ws, p->workspace_bytes);
        if (e == hipSuccess)
            e = upload_reals(window, n_fft, precision, &p->window);
        if (e != hipSuccess)
            rc = plan_fail(e, "stft");
    }
    if (rc) {
        sdsp_hip_stft_plan_destroy(p);
        return rc;
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_stft_plan_destroy(sdsp_hip_stft_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    free_bank(p->device, p->ws, p->window, p->inner);
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_stft_state_bytes(const sdsp_hip_stft_plan *p, uint64_t channels, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = static_cast<uint64_t>(p->hist) * channels * real_size(p->precision);
    return SDSP_HIP_OK;
}

int sdsp_hip_stft_plan_set_variant(sdsp_hip_stft_plan *p, int variant)
{
    if (!p || variant < 0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "bad argument");
    return set_inner_variant(p->inner, variant, "the inner real-input plan has no such kernel variant");
}

int sdsp_hip_stft_plan_get_info(const sdsp_hip_stft_plan *p, sdsp_hip_stft_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->n_fft = p->n;
    info->hop = p->hop;
    info->bins = p->bins;
    info->hist = p->hist;
    info->output = p->output;
    info->precision = p->precision;
    info->device = p->device;
    info->workspace_bytes = p->workspace_bytes;
    std::strncpy(info->kernel, select_kernel(p->inner, p->inner->variant).name, sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_stft_plan_launches(const sdsp_hip_stft_plan *p, uint64_t channels, uint64_t samples, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = 0;
    uint64_t frames = 0;
    if (int rc = sdsp_hip_stft_frames(p->hop, samples, &frames))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    *launches = slice_launch_count(p->inner, channels * frames, p->ws_units, 2) + (p->hist ? 1 : 0);
    return SDSP_HIP_OK;
}

int sdsp_hip_stft_process(sdsp_hip_stft_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t channels,
                          uint64_t samples, void *state, void *stream)
{
    uint64_t frames = 0;
    if (int rc = stft_check(p, in, in_stride, out, out_stride, channels, samples, &frames))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    const uint64_t rs = real_size(p->precision), oes = stft_out_esize(p);
    if (int rc = check_out_of_place(in, ((channels - 1) * in_stride + samples) * rs, rs, out,
                                    ((channels - 1) * out_stride + frames * p->bins) * oes, oes, state, rs,
                                    "in and out ranges overlap (the STFT runs out of place)"))
        return rc;
    if (int rc = use_device(p->device))
        return rc;
    return stft_run(p, in, in_stride, out, out_stride, channels, samples, state, reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_stft_process_host(sdsp_hip_stft_plan *p, const void *host_in, uint64_t in_stride, void *host_out, uint64_t out_stride,
                               uint64_t channels, uint64_t samples, void *host_state)
{
    uint64_t frames = 0;
    if (int rc = stft_check(p, host_in, in_stride, host_out, out_stride, channels, samples, &frames))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const size_t in_bytes = ((channels - 1) * in_stride + samples) * real_size(p->precision);
    const size_t out_bytes = ((channels - 1) * out_stride + frames * p->bins) * stft_out_esize(p);
    uint64_t state_bytes = 0;
    sdsp_hip_stft_state_bytes(p, channels, &state_bytes);
    const bool with_state = host_state && state_bytes;
    host_stage st("stft", { { host_in, in_bytes, false }, { host_out, out_bytes, true },
                        { with_state ? host_state : nullptr, state_bytes, true } });
    int rc = st.in();
    if (!rc)
        rc = stft_run(p, st.dev[0], in_stride, st.dev[1], out_stride, channels, samples, st.dev[2], nullptr);
    return st.out(rc);
}

// ------------------------------------------------------------------ inverse STFT banks (istft.hip)

namespace
{
// packed spectra of one slice (transformed in place): the STFT bank's budget, whose workspace round trip per frame is the same
// 4 N rs (DESIGN.md section 5.12 has the sweep)
constexpr uint64_t kIstftDefaultBudget = 256ull << 20;

int istft_run(sdsp_hip_istft_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t channels,
              uint64_t frames, void *state, hipStream_t stream)
{
    if (frames >= (1ull << 31))
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many frames per channel for one call");
    if (channels > ~0ull / frames)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many frames for one call");
    const uint64_t total = channels * frames;
    istft_args a{};
    a.in = in;
    a.out = out;
    a.state = p->hist ? state : nullptr;
    a.g = p->g;
    a.ws = p->ws;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.frames = static_cast<uint32_t>(frames);
    a.n = p->n;
    a.hop = p->hop;
    a.hist = p->hist;
    // before every overlap-add launch: those write the new pending sums where the old ones were
    if (int rc = carry_seed(p->precision, real_size(p->precision), out, out_stride, state, channels, frames * p->hop, p->hist, stream,
                            "istft"))
        return rc;
    for (uint64_t g0 = 0; g0 < total; g0 += p->ws_units) {
        a.g0 = g0;
        a.units = static_cast<uint32_t>(std::min(p->ws_units, total - g0));
        if (int rc = launch_istft(p->precision, a, ISTFT_PACK, stream))
            return rc;
        if (int rc = fft_exec_pieces(p->inner, p->ws, a.units, stream, p->inner->variant))
            return rc;
        if (int rc = launch_istft(p->precision, a, ISTFT_OLA, stream))
            return rc;
    }
    return SDSP_HIP_OK;
}

// argument checks shared by process and process_host (device pointers or not)
int istft_check(const sdsp_hip_istft_plan *p, const void *in, uint64_t in_stride, const void *out, uint64_t out_stride,
                uint64_t channels, uint64_t frames)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (channels == 0 || frames == 0)
        return SDSP_HIP_OK;
    if (!in || !out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in or out is null");
    if (frames > ~0ull / p->n)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many frames for one call");
    if (channels > 1 && (in_stride < frames * p->bins || out_stride < frames * p->hop))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_stride must be >= frames * bins and out_stride >= frames * hop");
    return SDSP_HIP_OK;
}
} // namespace

int sdsp_hip_istft_plan_create(sdsp_hip_istft_plan **out, uint32_t n_fft, uint32_t hop, const double *window, int norm, int precision,
                               uint64_t workspace_bytes, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (int rc = check_frame_shape(n_fft, hop, window, precision))
        return rc;
    if (int rc = check_real_input_range(n_fft, precision))
        return rc;
    std::vector<double> g(n_fft);
    double env_min = 0, env_max = 0;
    if (int rc = istft_synthesis(n_fft, hop, window, norm, g.data(), &env_min, &env_max))
        return rc;
    if (int rc = use_device(device))
        return rc;
    const uint64_t unit_bytes = static_cast<uint64_t>(n_fft) * real_size(precision);
    const uint64_t budget = workspace_bytes ? workspace_bytes : kIstftDefaultBudget;
    auto *p = new sdsp_hip_istft_plan();
    p->n = n_fft;
    p->hop = hop;
    p->hist = n_fft - hop;
    p->bins = n_fft / 2 + 1;
    p->norm = norm;
    p->precision = precision;
    p->device = device;
    p->env_min = env_min;
    p->env_max = env_max;
    p->ws_units = slice_units(budget, unit_bytes);
    p->workspace_bytes = p->ws_units * unit_bytes;
    int rc = fft_plan_create(&p->inner, n_fft / 2, 2, SDSP_HIP_REVERSE, precision, p->ws_units, device, 2);
    if (!rc) {
        hipError_t e = hipMalloc(&p->ws, p->workspace_bytes);
        if (e == hipSuccess)
            e = upload_reals(g.data(), n_fft, precision, &p->g);
        if (e != hipSuccess)
            rc = plan_fail(e, "istft");
    }
    if (rc) {
        sdsp_hip_istft_plan_destroy(p);
        return rc;
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_istft_plan_destroy(sdsp_hip_istft_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    free_bank(p->device, p->ws, p->g, p->inner);
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_istft_state_bytes(const sdsp_hip_istft_plan *p, uint64_t channels, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = static_cast<uint64_t>(p->hist) * channels * real_size(p->precision);
    return SDSP_HIP_OK;
}

int sdsp_hip_istft_plan_set_variant(sdsp_hip_istft_plan *p, int variant)
{
    if (!p || variant < 0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "bad argument");
    return set_inner_variant(p->inner, variant, "the inner real-input plan has no such kernel variant");
}

int sdsp_hip_istft_plan_get_info(const sdsp_hip_istft_plan *p, sdsp_hip_istft_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->n_fft = p->n;
    info->hop = p->hop;
    info->bins = p->bins;
    info->hist = p->hist;
    info->norm = p->norm;
    info->precision = p->precision;
    info->device = p->device;
    info->workspace_bytes = p->workspace_bytes;
    std::strncpy(info->kernel, select_kernel(p->inner, p->inner->variant).name, sizeof(info->kernel) - 1);
    info->env_min = p->env_min;
    info->env_max = p->env_max;
    return SDSP_HIP_OK;
}

int sdsp_hip_istft_plan_launches(const sdsp_hip_istft_plan *p, uint64_t channels, uint64_t frames, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = 0;
    if (channels == 0 || frames == 0)
        return SDSP_HIP_OK;
    if (channels > ~0ull / frames)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many frames for one call");
    *launches = (p->hist ? 1 : 0) + slice_launch_count(p->inner, channels * frames, p->ws_units, 2);
    return SDSP_HIP_OK;
}

int sdsp_hip_istft_process(sdsp_hip_istft_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t channels,
                           uint64_t frames, void *state, void *stream)
{
    if (int rc = istft_check(p, in, in_stride, out, out_stride, channels, frames))
        return rc;
    if (channels == 0 || frames == 0)
        return SDSP_HIP_OK;
    const uint64_t rs = real_size(p->precision);
    if (int rc = check_out_of_place(in, ((channels - 1) * in_stride + frames * p->bins) * 2 * rs, 2 * rs, out,
                                    ((channels - 1) * out_stride + frames * p->hop) * rs, rs, state, rs,
                                    "in and out ranges overlap (the inverse STFT runs out of place)"))
        return rc;
    if (int rc = use_device(p->device))
        return rc;
    return istft_run(p, in, in_stride, out, out_stride, channels, frames, state, reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_istft_process_host(sdsp_hip_istft_plan *p, const void *host_in, uint64_t in_stride, void *host_out, uint64_t out_stride,
                                uint64_t channels, uint64_t frames, void *host_state)
{
    if (int rc = istft_check(p, host_in, in_stride, host_out, out_stride, channels, frames))
        return rc;
    if (channels == 0 || frames == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const size_t rs = real_size(p->precision);
    const size_t in_bytes = ((channels - 1) * in_stride + frames * p->bins) * 2 * rs;
    const size_t out_bytes = ((channels - 1) * out_stride + frames * p->hop) * rs;
    uint64_t state_bytes = 0;
    sdsp_hip_istft_state_bytes(p, channels, &state_bytes);
    const bool with_state = host_state && state_bytes;
    host_stage st("istft", { { host_in, in_bytes, false }, { host_out, out_bytes, true },
                         { with_state ? host_state : nullptr, state_bytes, true } });
    int rc = st.in();
    if (!rc)
        rc = istft_run(p, st.dev[0], in_stride, st.dev[1], out_stride, channels, frames, st.dev[2], nullptr);
    return st.out(rc);
}

// ------------------------------------------------------------------ forward-backward filtering (iir_filtfilt.hip)

namespace
{
// the default slice budget: 256 MiB of right-edge samples, raised for long edges toward the 2^17 channels per slice that fill the
// chip (256 CUs x 8 resident waves x 64 channels), but never above 1 GiB whatever the edge (DESIGN.md section 5.13 has the sweep)
constexpr uint64_t kFiltfiltDefaultBudget = 256ull << 20;
constexpr uint64_t kFiltfiltMaxDefaultBudget = 1ull << 30;
constexpr uint64_t kFiltfiltFillSlice = 1ull << 17;

filtfilt_args filtfilt_make_args(const sdsp_hip_filtfilt_plan *p, void *data, uint64_t channels, uint64_t samples, uint64_t stride)
{
    filtfilt_args a{};
    a.data = data;
    a.ws = p->ws;
    a.channels = channels;
    a.samples = samples;
    a.stride = stride;
    a.sections = p->sections;
    a.padlen = p->padlen;
    a.kind = p->kind;
    a.padtype = p->padtype;
    a.gain = p->gain;
    for (uint32_t j = 0; j < p->sections; j++) {
        a.a1[j] = p->a1[j];
        a.a2[j] = p->a2[j];
        a.b1[j] = p->b1[j];
        a.b2[j] = p->b2[j];
    }
    for (uint32_t j = 0; j <= p->sections; j++)
        a.ss[j] = p->ss[j];
    return a;
}

int filtfilt_run(sdsp_hip_filtfilt_plan *p, void *data, uint64_t channels, uint64_t samples, uint64_t stride, hipStream_t stream)
{
    const size_t rs = real_size(p->precision);
    for (uint64_t c0 = 0; c0 < channels; c0 += p->slice_channels) {
        const uint64_t n = std::min(p->slice_channels, channels - c0);
        const filtfilt_args a = filtfilt_make_args(p, static_cast<char *>(data) + c0 * stride * rs, n, samples, stride);
        if (int rc = launch_filtfilt(p->precision, a, p->variant, stream))
            return rc;
    }
    return SDSP_HIP_OK;
}

// argument checks shared by process and process_host (device pointers or not)
int filtfilt_check(const sdsp_hip_filtfilt_plan *p, const void *data, uint64_t channels, uint64_t samples, uint64_t stride)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (samples <= p->padlen)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "samples must be larger than padlen (the edge extension mirrors padlen samples)");
    if (channels == 0)
        return SDSP_HIP_OK;
    if (!data)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "data is null");
    if (stride < samples && channels > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "stride must be >= samples");
    return SDSP_HIP_OK;
}
} // namespace

int sdsp_hip_filtfilt_plan_create(sdsp_hip_filtfilt_plan **out, uint32_t sections, int kind, const double *a, const double *b,
                                  double gain, int precision, int padtype, int64_t padlen, uint64_t workspace_bytes, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    double ss[SDSP_HIP_MAX_SECTIONS + 1];
    if (int rc = iir_steady_state(sections, kind, a, b, gain, ss))
        return rc;
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64 && precision != SDSP_HIP_F32_F64STATE)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32, SDSP_HIP_F64 or SDSP_HIP_F32_F64STATE");
    if (padtype < SDSP_HIP_PAD_NONE || padtype > SDSP_HIP_PAD_CONSTANT)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "padtype must be SDSP_HIP_PAD_NONE / ODD / EVEN / CONSTANT");
    uint32_t pad = 0;
    if (padtype != SDSP_HIP_PAD_NONE) {
        if (padlen >= (1ll << 31))
            return fail(SDSP_HIP_ERR_INVALID_SIZE, "padlen must be below 2^31");
        if (padlen < 0) {
            if (int rc = filtfilt_default_padlen(sections, kind, a, b, &pad))
                return rc;
        } else {
            pad = static_cast<uint32_t>(padlen);
        }
    }
    if (int rc = use_device(device))
        return rc;
    const uint64_t rs = real_size(precision);
    auto *p = new sdsp_hip_filtfilt_plan();
    p->sections = sections;
    p->padlen = pad;
    p->kind = kind;
    p->precision = precision;
    p->device = device;
    p->padtype = padtype;
    p->gain = gain;
    for (uint32_t j = 0; j < sections; j++) {
        p->a1[j] = a[3 * j + 1];
        p->a2[j] = a[3 * j + 2];
        if (b) {
            p->b1[j] = b[3 * j + 1];
            p->b2[j] = b[3 * j + 2];
        }
    }
    std::memcpy(p->ss, ss, sizeof(double) * (sections + 1));
    if (pad == 0) { // nothing to keep between the passes: one launch covers every channel
        p->slice_channels = 1ull << 40;
    } else {
        const uint64_t per_channel = pad * rs;
        const uint64_t fill = kFiltfiltFillSlice * per_channel;
        const uint64_t budget =
            workspace_bytes ? workspace_bytes : std::min(std::max(kFiltfiltDefaultBudget, fill), kFiltfiltMaxDefaultBudget);
        p->slice_channels = std::min<uint64_t>(std::max<uint64_t>(64, budget / per_channel / 64 * 64), 1ull << 36);
        p->workspace_bytes = p->slice_channels * per_channel;
        hipError_t e = hipMalloc(&p->ws, p->workspace_bytes);
        if (e != hipSuccess) {
            p->ws = nullptr;
            const int rc = plan_fail(e, "filtfilt");
            sdsp_hip_filtfilt_plan_destroy(p);
            return rc;
        }
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_filtfilt_plan_destroy(sdsp_hip_filtfilt_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (p->ws && use_device(p->device) == SDSP_HIP_OK)
        (void)hipFree(p->ws);
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_filtfilt_plan_set_variant(sdsp_hip_filtfilt_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 (fused) or 1 (direct)");
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_filtfilt_plan_launches(const sdsp_hip_filtfilt_plan *p, uint64_t channels, uint64_t samples, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = 0;
    if (samples <= p->padlen)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "samples must be larger than padlen");
    *launches = (channels + p->slice_channels - 1) / p->slice_channels;
    return SDSP_HIP_OK;
}

int sdsp_hip_filtfilt_plan_kernel(const sdsp_hip_filtfilt_plan *p, const void *data, uint64_t channels, uint64_t samples,
                                  uint64_t stride, char *name, size_t name_bytes)
{
    if (!p || !name || name_bytes == 0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    // the first slice's shape: the one the launcher selects for first (later slices start stride * slice_channels further on)
    const filtfilt_args a = filtfilt_make_args(p, const_cast<void *>(data), std::min(channels, p->slice_channels), samples, stride);
    std::strncpy(name, filtfilt_kernel_for(p->precision, a, p->variant), name_bytes - 1);
    name[name_bytes - 1] = 0;
    return SDSP_HIP_OK;
}

int sdsp_hip_filtfilt_plan_get_info(const sdsp_hip_filtfilt_plan *p, sdsp_hip_filtfilt_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->sections = p->sections;
    info->padlen = p->padlen;
    info->kind = p->kind;
    info->padtype = p->padtype;
    info->precision = p->precision;
    info->device = p->device;
    info->variant = p->variant;
    info->workspace_bytes = p->workspace_bytes;
    info->slice_channels = p->slice_channels;
    // the kernel of a long run of 16-byte aligned rows (address 0 stands for any aligned pointer)
    const filtfilt_args a = filtfilt_make_args(p, nullptr, 2, p->padlen + 1, 64);
    std::strncpy(info->kernel, filtfilt_kernel_for(p->precision, a, p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_filtfilt_process(sdsp_hip_filtfilt_plan *p, void *data, uint64_t channels, uint64_t samples, uint64_t stride, void *stream)
{
    if (int rc = filtfilt_check(p, data, channels, samples, stride))
        return rc;
    if (channels == 0)
        return SDSP_HIP_OK;
    if (misaligned(data, real_size(p->precision)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "data must be aligned to its element size");
    if (int rc = use_device(p->device))
        return rc;
    return filtfilt_run(p, data, channels, samples, stride, reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_filtfilt_process_host(sdsp_hip_filtfilt_plan *p, void *host_data, uint64_t channels, uint64_t samples, uint64_t stride)
{
    if (int rc = filtfilt_check(p, host_data, channels, samples, stride))
        return rc;
    if (channels == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    host_stage st("filtfilt", { { host_data, ((channels - 1) * stride + samples) * real_size(p->precision), true } });
    int rc = st.in();
    if (!rc)
        rc = filtfilt_run(p, st.dev[0], channels, samples, stride, nullptr);
    return st.out(rc);
}

// ------------------------------------------------------------------ Welch PSD banks (welch.hip)

namespace
{
// the STFT bank's measured slice budget, now split between segments and run partials
constexpr uint64_t kWelchDefaultBudget = 256ull << 20;

uint64_t welch_unit_bytes(uint32_t n, int precision)
{
    return static_cast<uint64_t>(n) * real_size(precision) + (static_cast<uint64_t>(n) / 2 + 1) * 8;
}

// segments per run: one run per channel up to 16 segments, else the smallest power of two R with R^2 >= the segments one channel
// has in a slice, so that the run stage and the combine stage both loop about sqrt of them
uint32_t welch_run_length(uint64_t frames, uint64_t ws_units)
{
    const uint64_t f = std::min(frames, ws_units);
    if (f <= 16)
        return static_cast<uint32_t>(std::max<uint64_t>(f, 1));
    uint32_t r = 1;
    while (static_cast<uint64_t>(r) * r < f)
        r <<= 1;
    return r;
}

int welch_run(sdsp_hip_welch_plan *p, const void *in, uint64_t in_stride, uint64_t channels, uint64_t samples, uint64_t position,
              void *state, double *acc, uint64_t acc_stride, hipStream_t stream)
{
    uint64_t frames = 0;
    if (int rc = sdsp_hip_welch_frames(p->n, p->hop, position, samples, &frames))
        return rc;
    if (frames >= (1ull << 31))
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many segments per channel for one call");
    if (frames && channels > ~0ull / frames)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many segments for one call");
    const uint64_t total = channels * frames;
    const uint64_t first = position < p->n ? 0 : (position - p->n) / p->hop + 1; // the call's first segment
    welch_args a{};
    a.in = in;
    a.state = state;
    a.window = p->window;
    a.ws = p->ws;
    a.part = p->part;
    a.acc = acc;
    a.in_stride = in_stride;
    a.acc_stride = acc_stride;
    a.channels = channels;
    a.frames = static_cast<uint32_t>(frames);
    a.n = p->n;
    a.hop = p->hop;
    a.off0 = static_cast<uint32_t>(first * p->hop + p->hist - position); // in [0, max(N - 1, hop - 1)]
    a.run = welch_run_length(frames, p->ws_units);
    a.detrend = p->detrend;
    for (uint64_t g0 = 0; g0 < total; g0 += p->ws_units) {
        a.g0 = g0;
        a.units = static_cast<uint32_t>(std::min(p->ws_units, total - g0));
        if (int rc = launch_welch(p->precision, a, WELCH_FRAME, stream))
            return rc;
        if (int rc = fft_exec_pieces(p->inner, p->ws, a.units, stream, p->inner->variant))
            return rc;
        if (int rc = launch_welch(p->precision, a, WELCH_RUN, stream))
            return rc;
        if (int rc = launch_welch(p->precision, a, WELCH_COMBINE, stream))
            return rc;
    }
    if (samples == 0)
        return SDSP_HIP_OK;
    // after every frame launch: they may read the old history (the label keeps the message texts of the STFT bank's launch)
    return carry_history(p->precision, real_size(p->precision), in, in_stride, state, channels, samples, p->hist, stream, "stft");
}

// argument checks shared by process and process_host (device pointers or not)
int welch_check(const sdsp_hip_welch_plan *p, const void *in, uint64_t in_stride, uint64_t channels, uint64_t samples,
                uint64_t position, const void *state, const double *acc, uint64_t acc_stride)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    uint64_t frames = 0;
    if (int rc = sdsp_hip_welch_frames(p->n, p->hop, position, samples, &frames))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (!in || !acc)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in or acc is null");
    if (!state && position > 0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "state may be null only at position 0");
    if (channels > 1 && (in_stride < samples || acc_stride < p->bins))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_stride must be >= samples and acc_stride >= bins");
    return SDSP_HIP_OK;
}

int welch_finalize_check(const sdsp_hip_welch_plan *p, const double *acc, uint64_t acc_stride, uint64_t frames_total, const void *out,
                         uint64_t out_stride, uint64_t channels)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (frames_total == 0)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "frames_total must be >= 1");
    if (channels == 0)
        return SDSP_HIP_OK;
    if (!acc || !out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "acc or out is null");
    if (channels > 1 && (acc_stride < p->bins || out_stride < p->bins))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "acc_stride and out_stride must be >= bins");
    return SDSP_HIP_OK;
}

int welch_finalize_run(const sdsp_hip_welch_plan *p, const double *acc, uint64_t acc_stride, uint64_t frames_total, void *out,
                       uint64_t out_stride, uint64_t channels, hipStream_t stream)
{
    welch_args a{};
    a.acc = const_cast<double *>(acc);
    a.acc_stride = acc_stride;
    a.out = out;
    a.out_stride = out_stride;
    a.channels = channels;
    a.n = p->n;
    a.c_edge = p->scale / static_cast<double>(frames_total);
    a.c_mid = 2.0 * p->scale / static_cast<double>(frames_total);
    return launch_welch(p->precision, a, WELCH_FINALIZE, stream);
}
} // namespace

int sdsp_hip_welch_plan_create(sdsp_hip_welch_plan **out, uint32_t n_fft, uint32_t hop, const double *window, int detrend, int scaling,
                               double fs, int precision, uint64_t workspace_bytes, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (int rc = check_frame_shape(n_fft, hop, window, precision))
        return rc;
    if (detrend != SDSP_HIP_DETREND_NONE && detrend != SDSP_HIP_DETREND_CONSTANT && detrend != SDSP_HIP_DETREND_LINEAR)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "detrend must be SDSP_HIP_DETREND_NONE, _CONSTANT or _LINEAR");
    if (scaling != SDSP_HIP_SCALING_DENSITY && scaling != SDSP_HIP_SCALING_SPECTRUM)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "scaling must be SDSP_HIP_SCALING_DENSITY or _SPECTRUM");
    if (!(fs > 0.0) || !std::isfinite(fs))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "fs must be finite and > 0");
    if (int rc = check_real_input_range(n_fft, precision))
        return rc;
    // the window rounded once to the plan precision; the scale sums run over those values
    std::vector<double> wr(window, window + n_fft);
    if (precision == SDSP_HIP_F32)
        for (double &v : wr)
            v = static_cast<double>(static_cast<float>(v));
    double sw = 0.0, sw2 = 0.0;
    for (double v : wr) {
        sw += v;
        sw2 += v * v;
    }
    if (int rc = use_device(device))
        return rc;
    const uint64_t unit_bytes = welch_unit_bytes(n_fft, precision);
    const uint64_t budget = workspace_bytes ? workspace_bytes : kWelchDefaultBudget;
    auto *p = new sdsp_hip_welch_plan();
    p->n = n_fft;
    p->hop = hop;
    p->hist = n_fft - 1;
    p->bins = n_fft / 2 + 1;
    p->detrend = detrend;
    p->scaling = scaling;
    p->fs = fs;
    p->scale = scaling == SDSP_HIP_SCALING_DENSITY ? 1.0 / (fs * sw2) : 1.0 / (sw * sw);
    p->precision = precision;
    p->device = device;
    p->ws_units = slice_units(budget, unit_bytes);
    p->workspace_bytes = p->ws_units * unit_bytes;
    int rc = fft_plan_create(&p->inner, n_fft / 2, 2, SDSP_HIP_FORWARD, precision, p->ws_units, device, 1);
    if (!rc) {
        hipError_t e = hipMalloc(&p->ws, p->workspace_bytes);
        if (e == hipSuccess) {
            p->part = reinterpret_cast<double *>(static_cast<char *>(p->ws) + p->ws_units * n_fft * real_size(precision));
            e = upload_reals(wr.data(), n_fft, precision, &p->window); // wr holds the rounded values: converting them again is exact
        }
        if (e != hipSuccess)
            rc = plan_fail(e, "welch");
    }
    if (rc) {
        sdsp_hip_welch_plan_destroy(p);
        return rc;
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_welch_plan_destroy(sdsp_hip_welch_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    free_bank(p->device, p->ws, p->window, p->inner);
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_welch_state_bytes(const sdsp_hip_welch_plan *p, uint64_t channels, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = static_cast<uint64_t>(p->hist) * channels * real_size(p->precision);
    return SDSP_HIP_OK;
}

int sdsp_hip_welch_plan_get_info(const sdsp_hip_welch_plan *p, sdsp_hip_welch_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->n_fft = p->n;
    info->hop = p->hop;
    info->bins = p->bins;
    info->hist = p->hist;
    info->detrend = p->detrend;
    info->scaling = p->scaling;
    info->fs = p->fs;
    info->precision = p->precision;
    info->device = p->device;
    info->workspace_bytes = p->workspace_bytes;
    std::strncpy(info->kernel, select_kernel(p->inner, p->inner->variant).name, sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_welch_plan_launches(const sdsp_hip_welch_plan *p, uint64_t channels, uint64_t samples, uint64_t position,
                                 uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = 0;
    uint64_t frames = 0;
    if (int rc = sdsp_hip_welch_frames(p->n, p->hop, position, samples, &frames))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    *launches = slice_launch_count(p->inner, channels * frames, p->ws_units, 3) + 1;
    return SDSP_HIP_OK;
}

int sdsp_hip_welch_process(sdsp_hip_welch_plan *p, const void *in, uint64_t in_stride, uint64_t channels, uint64_t samples,
                           uint64_t position, void *state, double *acc, uint64_t acc_stride, void *stream)
{
    if (int rc = welch_check(p, in, in_stride, channels, samples, position, state, acc, acc_stride))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    const uint64_t rs = real_size(p->precision);
    const uint64_t in_bytes = ((channels - 1) * in_stride + samples) * rs;
    if (ranges_overlap(in, in_bytes, state, channels * p->hist * rs) ||
        ranges_overlap(in, in_bytes, acc, ((channels - 1) * acc_stride + p->bins) * 8))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in overlaps state or acc");
    if (misaligned(in, rs) || misaligned(state, rs) || misaligned(acc, 8))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in, state and acc must be aligned to their element size");
    if (int rc = use_device(p->device))
        return rc;
    return welch_run(p, in, in_stride, channels, samples, position, state, acc, acc_stride, reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_welch_process_host(sdsp_hip_welch_plan *p, const void *host_in, uint64_t in_stride, uint64_t channels, uint64_t samples,
                                uint64_t position, void *host_state, double *host_acc, uint64_t acc_stride)
{
    if (int rc = welch_check(p, host_in, in_stride, channels, samples, position, host_state, host_acc, acc_stride))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const size_t rs = real_size(p->precision);
    const size_t in_bytes = ((channels - 1) * in_stride + samples) * rs;
    const size_t acc_bytes = ((channels - 1) * acc_stride + p->bins) * 8;
    const size_t state_bytes = channels * p->hist * rs;
    host_stage st("welch", { { host_in, in_bytes, false }, { host_acc, acc_bytes, true }, { host_state, state_bytes, true } });
    int rc = st.in();
    if (!rc)
        rc = welch_run(p, st.dev[0], in_stride, channels, samples, position, st.dev[2], static_cast<double *>(st.dev[1]), acc_stride,
                       nullptr);
    return st.out(rc);
}

int sdsp_hip_welch_finalize(sdsp_hip_welch_plan *p, const double *acc, uint64_t acc_stride, uint64_t frames_total, void *out,
                            uint64_t out_stride, uint64_t channels, void *stream)
{
    if (int rc = welch_finalize_check(p, acc, acc_stride, frames_total, out, out_stride, channels))
        return rc;
    if (channels == 0)
        return SDSP_HIP_OK;
    const uint64_t rs = real_size(p->precision);
    if (ranges_overlap(acc, ((channels - 1) * acc_stride + p->bins) * 8, out, ((channels - 1) * out_stride + p->bins) * rs))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "acc and out overlap");
    if (misaligned(acc, 8) || misaligned(out, rs))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "acc and out must be aligned to their element size");
    if (int rc = use_device(p->device))
        return rc;
    return welch_finalize_run(p, acc, acc_stride, frames_total, out, out_stride, channels, reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_welch_finalize_host(sdsp_hip_welch_plan *p, const double *host_acc, uint64_t acc_stride, uint64_t frames_total,
                                 void *host_out, uint64_t out_stride, uint64_t channels)
{
    if (int rc = welch_finalize_check(p, host_acc, acc_stride, frames_total, host_out, out_stride, channels))
        return rc;
    if (channels == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const size_t acc_bytes = ((channels - 1) * acc_stride + p->bins) * 8;
    const size_t out_bytes = ((channels - 1) * out_stride + p->bins) * real_size(p->precision);
    host_stage st("welch", { { host_acc, acc_bytes, false }, { host_out, out_bytes, true } });
    int rc = st.in();
    if (!rc)
        rc = welch_finalize_run(p, static_cast<const double *>(st.dev[0]), acc_stride, frames_total, st.dev[1], out_stride, channels,
                                nullptr);
    return st.out(rc);
}

// ------------------------------------------------------------------ cross-spectral density banks (csd.hip)

namespace
{
// the bytes of the first element through the last of `rows` rows of `row` elements `stride` apart
uint64_t rows_bytes(uint64_t rows, uint64_t stride, uint64_t row, uint64_t element_bytes)
{
    return rows ? ((rows - 1) * stride + row) * element_bytes : 0;
}

int csd_run(sdsp_hip_csd_plan *p, const void *in, uint64_t in_stride, uint64_t samples, uint64_t position, void *state, double *acc_xy,
            uint64_t acc_xy_stride, double *acc_auto, uint64_t acc_auto_stride, hipStream_t stream)
{
    uint64_t frames = 0;
    if (int rc = sdsp_hip_welch_frames(p->n, p->hop, position, samples, &frames))
        return rc;
    const uint64_t first = position < p->n ? 0 : (position - p->n) / p->hop + 1; // the call's first segment
    const uint64_t off0 = first * p->hop + p->hist - position;                  // in [0, max(N - 1, hop - 1)]
    if (frames && off0 + (frames - 1) * p->hop > 0xffffffffull)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many samples for one call");
    welch_args w{};
    w.in = in;
    w.state = state;
    w.window = p->window;
    w.ws = p->ws;
    w.in_stride = in_stride;
    w.channels = p->channels;
    w.n = p->n;
    w.hop = p->hop;
    w.detrend = p->detrend;
    w.g0 = 0;
    csd_args a{};
    a.ws = p->ws;
    a.part_xy = p->part_xy;
    a.part_auto = p->part_auto;
    a.acc_xy = acc_xy;
    a.acc_auto = acc_auto;
    a.acc_xy_stride = acc_xy_stride;
    a.acc_auto_stride = acc_auto_stride;
    a.npairs = static_cast<uint32_t>(p->npairs);
    a.nentries = static_cast<uint32_t>(acc_auto ? p->npairs + p->channels : p->npairs);
    a.table = p->tables + 2 * p->npairs + (acc_auto ? 0 : 3 * (p->npairs + p->channels));
    a.n = p->n;
    for (uint64_t ja = 0; ja < frames; ja += p->ws_cols) {
        const uint64_t cols = std::min(p->ws_cols, frames - ja);
        // the Welch bank's frame stage on the rectangle of every channel's segments [ja, ja + cols): units in channel-major order
        w.frames = static_cast<uint32_t>(cols);
        w.units = static_cast<uint32_t>(p->channels * cols);
        w.off0 = static_cast<uint32_t>(off0 + ja * p->hop);
        if (int rc = launch_welch(p->precision, w, WELCH_FRAME, stream))
            return rc;
        if (int rc = fft_exec_pieces(p->inner, p->ws, w.units, stream, p->inner->variant))
            return rc;
        a.frames = w.frames;
        a.run = welch_run_length(cols, cols);
        if (int rc = launch_csd(p->precision, a, CSD_RUN, stream))
            return rc;
        if (int rc = launch_csd(p->precision, a, CSD_COMBINE, stream))
            return rc;
    }
    if (samples == 0)
        return SDSP_HIP_OK;
    // after every frame launch: they may read the old history (the label keeps the message texts of the STFT bank's launch)
    return carry_history(p->precision, real_size(p->precision), in, in_stride, state, p->channels, samples, p->hist, stream, "stft");
}

// argument checks shared by process and process_host (device pointers or not)
int csd_check(const sdsp_hip_csd_plan *p, const void *in, uint64_t in_stride, uint64_t samples, uint64_t position, const void *state,
              const double *acc_xy, uint64_t acc_xy_stride, const double *acc_auto, uint64_t acc_auto_stride)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    uint64_t frames = 0;
    if (int rc = sdsp_hip_welch_frames(p->n, p->hop, position, samples, &frames))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    if (!in || !acc_xy)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in or acc_xy is null");
    if (!state && position > 0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "state may be null only at position 0");
    if (p->channels > 1 && (in_stride < samples || (acc_auto && acc_auto_stride < p->bins)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_stride must be >= samples and acc_auto_stride >= bins");
    if (p->npairs > 1 && acc_xy_stride < 2ull * p->bins)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "acc_xy_stride must be >= 2 bins");
    return SDSP_HIP_OK;
}

int csd_finalize_check(const sdsp_hip_csd_plan *p, int mode, const double *acc_xy, uint64_t acc_xy_stride, const double *acc_auto,
                       uint64_t acc_auto_stride, uint64_t frames_total, const void *out, uint64_t out_stride)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (mode != SDSP_HIP_CSD_CROSS && mode != SDSP_HIP_CSD_COHERENCE)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "mode must be SDSP_HIP_CSD_CROSS or _COHERENCE");
    if (frames_total == 0)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "frames_total must be >= 1");
    if (!acc_xy || !out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "acc_xy or out is null");
    if (mode == SDSP_HIP_CSD_COHERENCE && !acc_auto)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "coherence needs acc_auto");
    const uint64_t row = mode == SDSP_HIP_CSD_CROSS ? 2ull * p->bins : p->bins;
    if (p->npairs > 1 && (acc_xy_stride < 2ull * p->bins || out_stride < row))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "acc_xy_stride must be >= 2 bins and out_stride >= the output row");
    if (mode == SDSP_HIP_CSD_COHERENCE && p->channels > 1 && acc_auto_stride < p->bins)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "acc_auto_stride must be >= bins");
    return SDSP_HIP_OK;
}

uint64_t csd_out_row(const sdsp_hip_csd_plan *p, int mode) { return mode == SDSP_HIP_CSD_CROSS ? 2ull * p->bins : p->bins; }

int csd_finalize_run(const sdsp_hip_csd_plan *p, int mode, const double *acc_xy, uint64_t acc_xy_stride, const double *acc_auto,
                     uint64_t acc_auto_stride, uint64_t frames_total, void *out, uint64_t out_stride, hipStream_t stream)
{
    csd_args a{};
    a.table = p->tables;
    a.acc_xy = const_cast<double *>(acc_xy);
    a.acc_auto = const_cast<double *>(acc_auto);
    a.acc_xy_stride = acc_xy_stride;
    a.acc_auto_stride = acc_auto_stride;
    a.out = out;
    a.out_stride = out_stride;
    a.npairs = static_cast<uint32_t>(p->npairs);
    a.n = p->n;
    a.mode = mode;
    a.c_edge = p->scale / static_cast<double>(frames_total);
    a.c_mid = 2.0 * p->scale / static_cast<double>(frames_total);
    return launch_csd(p->precision, a, CSD_FINALIZE, stream);
}
} // namespace

int sdsp_hip_csd_plan_create(sdsp_hip_csd_plan **out, uint32_t n_fft, uint32_t hop, const double *window, int detrend, int scaling,
                             double fs, int precision, uint64_t channels, uint64_t npairs, const uint32_t *pairs,
                             uint64_t workspace_bytes, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (int rc = check_frame_shape(n_fft, hop, window, precision))
        return rc;
    if (detrend != SDSP_HIP_DETREND_NONE && detrend != SDSP_HIP_DETREND_CONSTANT && detrend != SDSP_HIP_DETREND_LINEAR)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "detrend must be SDSP_HIP_DETREND_NONE, _CONSTANT or _LINEAR");
    if (scaling != SDSP_HIP_SCALING_DENSITY && scaling != SDSP_HIP_SCALING_SPECTRUM)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "scaling must be SDSP_HIP_SCALING_DENSITY or _SPECTRUM");
    if (!(fs > 0.0) || !std::isfinite(fs))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "fs must be finite and > 0");
    if (int rc = check_real_input_range(n_fft, precision))
        return rc;
    if (channels == 0 || npairs == 0)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "channels and npairs must be >= 1");
    if (!pairs)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "pairs is null");
    if (channels >= (1ull << 30) || npairs >= (1ull << 30))
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many channels or pairs");
    for (uint64_t i = 0; i < 2 * npairs; i++)
        if (pairs[i] >= channels)
            return fail(SDSP_HIP_ERR_INVALID_ARG, "pair " + std::to_string(i / 2) + " names channel " + std::to_string(pairs[i]) +
                                                      " of " + std::to_string(channels));
    // one column: every channel's segment, and one partial row per pair (complex) and per channel
    const uint64_t bins = n_fft / 2 + 1;
    const uint64_t column_bytes = channels * n_fft * real_size(precision) + (2 * npairs + channels) * bins * 8;
    const uint64_t budget = workspace_bytes ? workspace_bytes : kWelchDefaultBudget;
    if (budget < column_bytes)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "workspace_bytes holds no segment column: one takes " + std::to_string(column_bytes) +
                                                  " bytes");
    // the window rounded once to the plan precision; the scale sums run over those values
    std::vector<double> wr(window, window + n_fft);
    if (precision == SDSP_HIP_F32)
        for (double &v : wr)
            v = static_cast<double>(static_cast<float>(v));
    double sw = 0.0, sw2 = 0.0;
    for (double v : wr) {
        sw += v;
        sw2 += v * v;
    }
    // the tables: the pairs as given; the run stage's order (sorted by a, then b, channel c's auto entry behind the pairs with a = c)
    // with and without the auto entries
    std::vector<std::array<uint32_t, 3>> order;
    for (uint64_t i = 0; i < npairs; i++)
        order.push_back({ pairs[2 * i], pairs[2 * i + 1], static_cast<uint32_t>(i) });
    std::stable_sort(order.begin(), order.end(), [](const auto &x, const auto &y) { return x[0] != y[0] ? x[0] < y[0] : x[1] < y[1]; });
    std::vector<uint32_t> tab(pairs, pairs + 2 * npairs);
    size_t at = 0;
    for (uint64_t c = 0; c < channels; c++) {
        for (; at < order.size() && order[at][0] == c; at++)
            tab.insert(tab.end(), order[at].begin(), order[at].end());
        tab.insert(tab.end(), { static_cast<uint32_t>(c), static_cast<uint32_t>(c), static_cast<uint32_t>(npairs + c) });
    }
    for (const auto &e : order)
        tab.insert(tab.end(), e.begin(), e.end());
    if (int rc = use_device(device))
        return rc;
    auto *p = new sdsp_hip_csd_plan();
    p->n = n_fft;
    p->hop = hop;
    p->hist = n_fft - 1;
    p->bins = n_fft / 2 + 1;
    p->detrend = detrend;
    p->scaling = scaling;
    p->fs = fs;
    p->scale = scaling == SDSP_HIP_SCALING_DENSITY ? 1.0 / (fs * sw2) : 1.0 / (sw * sw);
    p->precision = precision;
    p->device = device;
    p->channels = channels;
    p->npairs = npairs;
    p->column_bytes = column_bytes;
    p->ws_cols = std::min<uint64_t>(budget / column_bytes, (1ull << 30) / channels); // a slice's units are counted in 32 bits
    p->workspace_bytes = p->ws_cols * column_bytes;
    int rc = fft_plan_create(&p->inner, n_fft / 2, 2, SDSP_HIP_FORWARD, precision, channels * p->ws_cols, device, 1);
    if (!rc) {
        hipError_t e = hipMalloc(&p->ws, p->workspace_bytes);
        if (e == hipSuccess) {
            p->part_xy = reinterpret_cast<double *>(static_cast<char *>(p->ws) + channels * p->ws_cols * n_fft * real_size(precision));
            p->part_auto = p->part_xy + 2 * npairs * p->ws_cols * bins;
            e = upload_reals(wr.data(), n_fft, precision, &p->window); // wr holds the rounded values: converting them again is exact
        }
        if (e == hipSuccess)
            e = hipMalloc(reinterpret_cast<void **>(&p->tables), tab.size() * sizeof(uint32_t));
        if (e == hipSuccess)
            e = hipMemcpy(p->tables, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess)
            rc = plan_fail(e, "csd");
    }
    if (rc) {
        sdsp_hip_csd_plan_destroy(p);
        return rc;
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_csd_plan_destroy(sdsp_hip_csd_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK)
        (void)hipFree(p->tables);
    free_bank(p->device, p->ws, p->window, p->inner);
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_csd_state_bytes(const sdsp_hip_csd_plan *p, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = static_cast<uint64_t>(p->hist) * p->channels * real_size(p->precision);
    return SDSP_HIP_OK;
}

int sdsp_hip_csd_plan_get_info(const sdsp_hip_csd_plan *p, sdsp_hip_csd_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->n_fft = p->n;
    info->hop = p->hop;
    info->bins = p->bins;
    info->hist = p->hist;
    info->detrend = p->detrend;
    info->scaling = p->scaling;
    info->fs = p->fs;
    info->precision = p->precision;
    info->device = p->device;
    info->channels = p->channels;
    info->npairs = p->npairs;
    info->column_bytes = p->column_bytes;
    info->slice_columns = p->ws_cols;
    info->workspace_bytes = p->workspace_bytes;
    std::strncpy(info->kernel, select_kernel(p->inner, p->inner->variant).name, sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_csd_plan_launches(const sdsp_hip_csd_plan *p, uint64_t samples, uint64_t position, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = 0;
    uint64_t frames = 0;
    if (int rc = sdsp_hip_welch_frames(p->n, p->hop, position, samples, &frames))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    // a slice of `cols` columns is channels cols units of the transform
    *launches = slice_launch_count(p->inner, p->channels * frames, p->channels * p->ws_cols, 3) + 1;
    return SDSP_HIP_OK;
}

int sdsp_hip_csd_process(sdsp_hip_csd_plan *p, const void *in, uint64_t in_stride, uint64_t samples, uint64_t position, void *state,
                         double *acc_xy, uint64_t acc_xy_stride, double *acc_auto, uint64_t acc_auto_stride, void *stream)
{
    if (int rc = csd_check(p, in, in_stride, samples, position, state, acc_xy, acc_xy_stride, acc_auto, acc_auto_stride))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    const uint64_t rs = real_size(p->precision);
    const uint64_t in_bytes = rows_bytes(p->channels, in_stride, samples, rs);
    const uint64_t xy_bytes = rows_bytes(p->npairs, acc_xy_stride, 2ull * p->bins, 8);
    const uint64_t auto_bytes = rows_bytes(p->channels, acc_auto_stride, p->bins, 8);
    if (ranges_overlap(in, in_bytes, state, p->channels * p->hist * rs) || ranges_overlap(in, in_bytes, acc_xy, xy_bytes) ||
        ranges_overlap(in, in_bytes, acc_auto, auto_bytes))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in overlaps state or an accumulator");
    if (ranges_overlap(acc_xy, xy_bytes, acc_auto, auto_bytes))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "acc_xy and acc_auto overlap");
    if (misaligned(in, rs) || misaligned(state, rs) || misaligned(acc_xy, 8) || misaligned(acc_auto, 8))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in, state and the accumulators must be aligned to their element size");
    if (int rc = use_device(p->device))
        return rc;
    return csd_run(p, in, in_stride, samples, position, state, acc_xy, acc_xy_stride, acc_auto, acc_auto_stride,
                   reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_csd_process_host(sdsp_hip_csd_plan *p, const void *host_in, uint64_t in_stride, uint64_t samples, uint64_t position,
                              void *host_state, double *host_acc_xy, uint64_t acc_xy_stride, double *host_acc_auto,
                              uint64_t acc_auto_stride)
{
    if (int rc = csd_check(p, host_in, in_stride, samples, position, host_state, host_acc_xy, acc_xy_stride, host_acc_auto,
                           acc_auto_stride))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const size_t rs = real_size(p->precision);
    host_stage st("csd", { { host_in, rows_bytes(p->channels, in_stride, samples, rs), false },
                           { host_acc_xy, rows_bytes(p->npairs, acc_xy_stride, 2ull * p->bins, 8), true },
                           { host_state, p->channels * p->hist * rs, true },
                           { host_acc_auto, rows_bytes(p->channels, acc_auto_stride, p->bins, 8), true } });
    int rc = st.in();
    if (!rc)
        rc = csd_run(p, st.dev[0], in_stride, samples, position, st.dev[2], static_cast<double *>(st.dev[1]), acc_xy_stride,
                     static_cast<double *>(st.dev[3]), acc_auto_stride, nullptr);
    return st.out(rc);
}

int sdsp_hip_csd_finalize(sdsp_hip_csd_plan *p, int mode, const double *acc_xy, uint64_t acc_xy_stride, const double *acc_auto,
                          uint64_t acc_auto_stride, uint64_t frames_total, void *out, uint64_t out_stride, void *stream)
{
    if (int rc = csd_finalize_check(p, mode, acc_xy, acc_xy_stride, acc_auto, acc_auto_stride, frames_total, out, out_stride))
        return rc;
    const uint64_t rs = real_size(p->precision);
    const uint64_t out_bytes = rows_bytes(p->npairs, out_stride, csd_out_row(p, mode), rs);
    if (ranges_overlap(acc_xy, rows_bytes(p->npairs, acc_xy_stride, 2ull * p->bins, 8), out, out_bytes) ||
        (mode == SDSP_HIP_CSD_COHERENCE && ranges_overlap(acc_auto, rows_bytes(p->channels, acc_auto_stride, p->bins, 8), out, out_bytes)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "an accumulator and out overlap");
    if (misaligned(acc_xy, 8) || misaligned(out, rs) || (mode == SDSP_HIP_CSD_COHERENCE && misaligned(acc_auto, 8)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "the accumulators and out must be aligned to their element size");
    if (int rc = use_device(p->device))
        return rc;
    return csd_finalize_run(p, mode, acc_xy, acc_xy_stride, acc_auto, acc_auto_stride, frames_total, out, out_stride,
                            reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_csd_finalize_host(sdsp_hip_csd_plan *p, int mode, const double *host_acc_xy, uint64_t acc_xy_stride,
                               const double *host_acc_auto, uint64_t acc_auto_stride, uint64_t frames_total, void *host_out,
                               uint64_t out_stride)
{
    if (int rc = csd_finalize_check(p, mode, host_acc_xy, acc_xy_stride, host_acc_auto, acc_auto_stride, frames_total, host_out,
                                    out_stride))
        return rc;
    if (int rc = use_device(p->device))
        return rc;
    const bool coh = mode == SDSP_HIP_CSD_COHERENCE;
    host_stage st("csd", { { host_acc_xy, rows_bytes(p->npairs, acc_xy_stride, 2ull * p->bins, 8), false },
                           { host_out, rows_bytes(p->npairs, out_stride, csd_out_row(p, mode), real_size(p->precision)), true },
                           { coh ? host_acc_auto : nullptr, rows_bytes(p->channels, acc_auto_stride, p->bins, 8), false } });
    int rc = st.in();
    if (!rc)
        rc = csd_finalize_run(p, mode, static_cast<const double *>(st.dev[0]), acc_xy_stride, static_cast<const double *>(st.dev[2]),
                              acc_auto_stride, frames_total, st.dev[1], out_stride, nullptr);
    return st.out(rc);
}

// ------------------------------------------------------------------ polyphase filter-bank channelizer banks (pfb.hip)

namespace
{
constexpr uint64_t kPfbDefaultBudget = 256ull << 20; // the STFT bank's

uint64_t pfb_in_esize(const sdsp_hip_pfb_plan *p)
{
    return p->kind == SDSP_HIP_PFB_COMPLEX ? esize(p->precision) : real_size(p->precision);
}
uint64_t pfb_out_esize(const sdsp_hip_pfb_plan *p) { return esize(p->precision); }

// the slice [g0, g0 + units) of the channel-major (channel, frame) numbering as rectangles: a partial first channel, whole channels, a
// partial last channel.  f(c0, nc, j0, nj) is called for each; a non-zero return stops the walk.
extern "C++" template <typename F> int pfb_rects(uint64_t g0, uint64_t units, uint64_t frames, F f)
{
    uint64_t g = g0;
    const uint64_t end = g0 + units;
    while (g < end) {
        const uint64_t c = g / frames, j = g - c * frames;
        uint64_t nc = 1, nj;
        if (j == 0 && end - g >= frames) {
            nc = (end - g) / frames;
            nj = frames;
        } else {
            nj = std::min(frames - j, end - g);
        }
        if (int rc = f(c, nc, static_cast<uint32_t>(j), static_cast<uint32_t>(nj)))
            return rc;
        g += nc * nj;
    }
    return SDSP_HIP_OK;
}

int pfb_run(sdsp_hip_pfb_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t channels, uint64_t samples,
            uint64_t position, void *state, hipStream_t stream)
{
    const uint64_t frames = samples / p->hop;
    if (frames >= (1ull << 31))
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many frames per channel for one call");
    if (channels > ~0ull / frames)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many frames for one call");
    const uint64_t total = channels * frames;
    const bool cplx = p->kind == SDSP_HIP_PFB_COMPLEX;
    const bool whole = cplx && (channels == 1 || out_stride == frames * p->m); // the output rows are one contiguous run of frames
    if (p->inner->sync) // this call's launches report into a clean sticky abort word (as sdsp_hip_fft_exec)
        HIP_TRY(hipMemsetAsync(fft1m_sticky(p->inner), 0, sizeof(unsigned), stream));
    pfb_args a{};
    a.in = in;
    a.state = p->hist ? state : nullptr;
    a.taps = p->taps;
    a.in_stride = in_stride;
    a.m = p->m;
    a.p = p->p;
    a.hop = p->hop;
    a.hist = p->hist;
    a.complex_in = cplx;
    a.rotate = p->phase == SDSP_HIP_PFB_PHASE_TIME;
    a.shift0 = static_cast<uint32_t>((position % p->m + p->hop) % p->m); // (position - hist) mod m: hist = p m - hop
    a.form = p->form;
    stft_args e{}; // REAL: the STFT bank's emit launch
    e.out = out;
    e.ws = p->ws;
    e.out_stride = out_stride;
    e.frames = static_cast<uint32_t>(frames);
    e.n = p->m;
    e.output = SDSP_HIP_STFT_COMPLEX;
    char *const ob = static_cast<char *>(out);
    const uint64_t oes = pfb_out_esize(p);
    for (uint64_t g0 = 0; g0 < total; g0 += p->ws_units) {
        const uint64_t units = std::min(p->ws_units, total - g0);
        a.dst = cplx ? out : p->ws;
        a.dst_cstride = cplx ? out_stride : frames * p->m;
        a.dst_sub = cplx ? 0 : g0 * p->m;
        if (int rc = pfb_rects(g0, units, frames, [&](uint64_t c0, uint64_t nc, uint32_t j0, uint32_t nj) {
                a.c0 = c0;
                a.nc = nc;
                a.j0 = j0;
                a.nj = nj;
                return launch_pfb(p->precision, a, stream);
            }))
            return rc;
        if (!cplx) {
            e.g0 = g0;
            e.units = static_cast<uint32_t>(units);
            if (int rc = fft_exec_pieces(p->inner, p->ws, units, stream, p->inner->variant))
                return rc;
            if (int rc = launch_stft(p->precision, e, STFT_EMIT, stream))
                return rc;
        } else if (whole) {
            if (int rc = fft_exec_pieces(p->inner, ob + g0 * p->m * oes, units, stream, p->inner->variant))
                return rc;
        } else { // padded rows: every channel's run of frames on its own
            if (int rc = pfb_rects(g0, units, frames, [&](uint64_t c0, uint64_t nc, uint32_t j0, uint32_t nj) {
                    for (uint64_t c = c0; c < c0 + nc; c++)
                        if (int rc2 = fft_exec_pieces(p->inner, ob + (c * out_stride + static_cast<uint64_t>(j0) * p->m) * oes, nj, stream,
                                                      p->inner->variant))
                            return rc2;
                    return static_cast<int>(SDSP_HIP_OK);
                }))
                return rc;
        }
    }
    // after every fold launch: they may read the old history (the labels keep each kind's message texts)
    return carry_history(p->precision, cplx ? esize(p->precision) : real_size(p->precision), in, in_stride, state, channels, samples,
                         p->hist, stream, cplx ? "pfb" : "stft");
}

// argument checks shared by process and process_host (device pointers or not)
int pfb_check(const sdsp_hip_pfb_plan *p, const void *in, uint64_t in_stride, const void *out, uint64_t out_stride, uint64_t channels,
              uint64_t samples, uint64_t *frames)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (int rc = sdsp_hip_pfb_frames(p->hop, samples, frames))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (!in || !out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in or out is null");
    if (channels > 1 && (in_stride < samples || out_stride < *frames * p->bins))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_stride must be >= samples and out_stride >= frames * bins");
    return SDSP_HIP_OK;
}
} // namespace

int sdsp_hip_pfb_plan_create(sdsp_hip_pfb_plan **out, uint32_t channels_m, uint32_t taps_per_channel, uint32_t hop, const double *taps,
                             int input_kind, int phase, int precision, uint64_t workspace_bytes, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    const uint32_t m = channels_m;
    if (!sdsp_hip_is_power_of_2(m))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "channels_m must be a power of 2");
    if (taps_per_channel == 0 || taps_per_channel > SDSP_HIP_PFB_MAX_TAPS_PER_CHANNEL)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps_per_channel must be in [1, SDSP_HIP_PFB_MAX_TAPS_PER_CHANNEL]");
    if (static_cast<uint64_t>(m) * taps_per_channel > SDSP_HIP_PFB_MAX_TAPS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "the prototype may have at most SDSP_HIP_PFB_MAX_TAPS taps");
    if (hop == 0 || hop > m)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "hop must be in [1, channels_m]");
    if (!taps)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "taps pointer is null");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (input_kind != SDSP_HIP_PFB_REAL && input_kind != SDSP_HIP_PFB_COMPLEX)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "input_kind must be SDSP_HIP_PFB_REAL or SDSP_HIP_PFB_COMPLEX");
    if (phase != SDSP_HIP_PFB_PHASE_FRAME && phase != SDSP_HIP_PFB_PHASE_TIME)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "phase must be SDSP_HIP_PFB_PHASE_FRAME or SDSP_HIP_PFB_PHASE_TIME");
    const bool cplx = input_kind == SDSP_HIP_PFB_COMPLEX;
    if (m < (cplx ? 16u : 32u) || m > stft_max_n(precision))
        return fail(SDSP_HIP_ERR_UNSUPPORTED,
                    "channels_m must be in the transform range (f32 .. 65536, f64 .. 32768; from 32 for real input, 16 for complex)");
    if (int rc = use_device(device))
        return rc;
    const uint64_t taps_n = static_cast<uint64_t>(m) * taps_per_channel;
    const uint64_t unit_bytes = static_cast<uint64_t>(m) * real_size(precision) * (cplx ? 2 : 1);
    const uint64_t budget = workspace_bytes ? workspace_bytes : kPfbDefaultBudget;
    auto *p = new sdsp_hip_pfb_plan();
    p->m = m;
    p->p = taps_per_channel;
    p->hop = hop;
    p->hist = static_cast<uint32_t>(taps_n - hop);
    p->bins = cplx ? m : m / 2 + 1;
    p->kind = input_kind;
    p->phase = phase;
    p->precision = precision;
    p->device = device;
    p->ws_units = slice_units(budget, unit_bytes);
    p->workspace_bytes = p->ws_units * unit_bytes;
    int rc = cplx ? fft_plan_create(&p->inner, m, SDSP_HIP_RADIX_AUTO, SDSP_HIP_FORWARD, precision, p->ws_units, device, 0)
                  : fft_plan_create(&p->inner, m / 2, 2, SDSP_HIP_FORWARD, precision, p->ws_units, device, 1);
    if (!rc) {
        hipError_t e = cplx ? hipSuccess : hipMalloc(&p->ws, p->workspace_bytes);
        if (e == hipSuccess)
            e = upload_reals(taps, taps_n, precision, &p->taps);
        if (e != hipSuccess)
            rc = plan_fail(e, "pfb");
    }
    if (rc) {
        sdsp_hip_pfb_plan_destroy(p);
        return rc;
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_pfb_plan_destroy(sdsp_hip_pfb_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    free_bank(p->device, p->ws, p->taps, p->inner);
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_pfb_state_bytes(const sdsp_hip_pfb_plan *p, uint64_t channels, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = static_cast<uint64_t>(p->hist) * channels * pfb_in_esize(p);
    return SDSP_HIP_OK;
}

int sdsp_hip_pfb_plan_set_variant(sdsp_hip_pfb_plan *p, int variant)
{
    if (!p || variant < 0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "bad argument");
    return set_inner_variant(p->inner, variant, "the inner plan has no such kernel variant", true);
}

int sdsp_hip_pfb_plan_set_fold_form(sdsp_hip_pfb_plan *p, int form)
{
    if (!p || (form != 0 && form != 1))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "form must be 0 (chosen from the sizes) or 1 (plain)");
    p->form = form;
    return SDSP_HIP_OK;
}

int sdsp_hip_pfb_plan_get_info(const sdsp_hip_pfb_plan *p, sdsp_hip_pfb_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->channels_m = p->m;
    info->taps_per_channel = p->p;
    info->hop = p->hop;
    info->bins = p->bins;
    info->hist = p->hist;
    info->input_kind = p->kind;
    info->phase = p->phase;
    info->precision = p->precision;
    info->device = p->device;
    info->workspace_bytes = p->workspace_bytes;
    std::strncpy(info->kernel, select_kernel(p->inner, p->inner->variant).name, sizeof(info->kernel) - 1);
    std::strncpy(info->fold, p->form ? "plain" : pfb_form_for(p->m, p->hop), sizeof(info->fold) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_pfb_plan_launches(const sdsp_hip_pfb_plan *p, uint64_t channels, uint64_t samples, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = 0;
    uint64_t frames = 0;
    if (int rc = sdsp_hip_pfb_frames(p->hop, samples, &frames))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    const uint64_t total = channels * frames;
    uint64_t n = 0;
    for (uint64_t g0 = 0; g0 < total; g0 += p->ws_units) {
        const uint64_t units = std::min(p->ws_units, total - g0);
        pfb_rects(g0, units, frames, [&](uint64_t, uint64_t, uint32_t, uint32_t) {
            n++;
            return 0;
        });
        n += fft_launch_count(p->inner, units, p->inner->variant) + (p->kind == SDSP_HIP_PFB_REAL ? 1 : 0);
    }
    *launches = n + (p->hist ? 1 : 0);
    return SDSP_HIP_OK;
}

int sdsp_hip_pfb_process(sdsp_hip_pfb_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t channels,
                         uint64_t samples, uint64_t position, void *state, void *stream)
{
    uint64_t frames = 0;
    if (int rc = pfb_check(p, in, in_stride, out, out_stride, channels, samples, &frames))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    const uint64_t ies = pfb_in_esize(p), oes = pfb_out_esize(p);
    if (int rc = check_out_of_place(in, ((channels - 1) * in_stride + samples) * ies, ies, out,
                                    ((channels - 1) * out_stride + frames * p->bins) * oes, oes, state, ies,
                                    "in and out ranges overlap (the filter bank runs out of place)"))
        return rc;
    if (int rc = use_device(p->device))
        return rc;
    return pfb_run(p, in, in_stride, out, out_stride, channels, samples, position, state, reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_pfb_process_host(sdsp_hip_pfb_plan *p, const void *host_in, uint64_t in_stride, void *host_out, uint64_t out_stride,
                              uint64_t channels, uint64_t samples, uint64_t position, void *host_state)
{
    uint64_t frames = 0;
    if (int rc = pfb_check(p, host_in, in_stride, host_out, out_stride, channels, samples, &frames))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const size_t in_bytes = ((channels - 1) * in_stride + samples) * pfb_in_esize(p);
    const size_t out_bytes = ((channels - 1) * out_stride + frames * p->bins) * pfb_out_esize(p);
    uint64_t state_bytes = 0;
    sdsp_hip_pfb_state_bytes(p, channels, &state_bytes);
    const bool with_state = host_state && state_bytes;
    host_stage st("pfb", { { host_in, in_bytes, false }, { host_out, out_bytes, true },
                       { with_state ? host_state : nullptr, state_bytes, true } });
    int rc = st.in();
    if (!rc)
        rc = pfb_run(p, st.dev[0], in_stride, st.dev[1], out_stride, channels, samples, position, st.dev[2], nullptr);
    return st.out(rc);
}

// ------------------------------------------------------------------ polyphase synthesis banks (pfb_synth.hip)

namespace
{
uint64_t pfb_synth_out_esize(const sdsp_hip_pfb_synth_plan *p)
{
    return p->kind == SDSP_HIP_PFB_COMPLEX ? esize(p->precision) : real_size(p->precision);
}

int pfb_synth_run(sdsp_hip_pfb_synth_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t channels,
                  uint64_t frames, uint64_t position, void *state, hipStream_t stream)
{
    if (frames >= (1ull << 31))
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many frames per channel for one call");
    if (channels > ~0ull / frames)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many frames for one call");
    const uint64_t total = channels * frames;
    const bool cplx = p->kind == SDSP_HIP_PFB_COMPLEX;
    if (p->inner->sync) // this call's launches report into a clean sticky abort word (as sdsp_hip_fft_exec)
        HIP_TRY(hipMemsetAsync(fft1m_sticky(p->inner), 0, sizeof(unsigned), stream));
    pfb_synth_args a{};
    a.in = in;
    a.out = out;
    a.state = p->hist ? state : nullptr;
    a.taps = p->taps;
    a.ws = p->ws;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.frames = static_cast<uint32_t>(frames);
    a.m = p->m;
    a.p = p->p;
    a.hop = p->hop;
    a.hist = p->hist;
    a.complex_out = cplx;
    a.rotate = p->phase == SDSP_HIP_PFB_PHASE_TIME;
    a.shift0 = static_cast<uint32_t>((position % p->m + p->hop) % p->m); // (position - hist) mod m: hist = p m - hop
    a.form = p->form;
    istft_args r{}; // REAL: the inverse STFT bank's pack launch
    r.in = in;
    r.ws = p->ws;
    r.in_stride = in_stride;
    r.frames = a.frames;
    r.n = p->m;
    // before every unfold launch: those write the new pending sums where the old ones were (the labels keep each kind's message texts)
    if (int rc = carry_seed(p->precision, pfb_synth_out_esize(p), out, out_stride, a.state, channels, frames * p->hop, p->hist, stream,
                            cplx ? "pfb synthesis" : "istft"))
        return rc;
    for (uint64_t g0 = 0; g0 < total; g0 += p->ws_units) {
        const uint64_t units = std::min(p->ws_units, total - g0);
        a.g0 = r.g0 = g0;
        a.units = units;
        r.units = static_cast<uint32_t>(units);
        if (int rc = cplx ? launch_pfb_synth(p->precision, a, PFB_SYNTH_COPY, stream) : launch_istft(p->precision, r, ISTFT_PACK, stream))
            return rc;
        if (int rc = fft_exec_pieces(p->inner, p->ws, units, stream, p->inner->variant))
            return rc;
        if (int rc = pfb_rects(g0, units, frames, [&](uint64_t c0, uint64_t nc, uint32_t j0, uint32_t nj) {
                a.c0 = c0;
                a.nc = nc;
                a.j0 = j0;
                a.nj = nj;
                return launch_pfb_synth(p->precision, a, PFB_SYNTH_UNFOLD, stream);
            }))
            return rc;
    }
    return SDSP_HIP_OK;
}

// argument checks shared by process and process_host (device pointers or not)
int pfb_synth_check(const sdsp_hip_pfb_synth_plan *p, const void *in, uint64_t in_stride, const void *out, uint64_t out_stride,
                    uint64_t channels, uint64_t frames)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (channels == 0 || frames == 0)
        return SDSP_HIP_OK;
    if (!in || !out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in or out is null");
    if (frames > ~0ull / p->m)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many frames for one call");
    if (channels > 1 && (in_stride < frames * p->bins || out_stride < frames * p->hop))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_stride must be >= frames * bins and out_stride >= frames * hop");
    return SDSP_HIP_OK;
}
} // namespace

int sdsp_hip_pfb_synth_plan_create(sdsp_hip_pfb_synth_plan **out, uint32_t channels_m, uint32_t taps_per_channel, uint32_t hop,
                                   const double *taps, int output_kind, int phase, int precision, uint64_t workspace_bytes, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    const uint32_t m = channels_m;
    if (!sdsp_hip_is_power_of_2(m))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "channels_m must be a power of 2");
    if (taps_per_channel == 0 || taps_per_channel > SDSP_HIP_PFB_MAX_TAPS_PER_CHANNEL)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps_per_channel must be in [1, SDSP_HIP_PFB_MAX_TAPS_PER_CHANNEL]");
    if (static_cast<uint64_t>(m) * taps_per_channel > SDSP_HIP_PFB_MAX_TAPS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "the prototype may have at most SDSP_HIP_PFB_MAX_TAPS taps");
    if (hop == 0 || hop > m)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "hop must be in [1, channels_m]");
    if (!taps)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "taps pointer is null");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (output_kind != SDSP_HIP_PFB_REAL && output_kind != SDSP_HIP_PFB_COMPLEX)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "output_kind must be SDSP_HIP_PFB_REAL or SDSP_HIP_PFB_COMPLEX");
    if (phase != SDSP_HIP_PFB_PHASE_FRAME && phase != SDSP_HIP_PFB_PHASE_TIME)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "phase must be SDSP_HIP_PFB_PHASE_FRAME or SDSP_HIP_PFB_PHASE_TIME");
    const bool cplx = output_kind == SDSP_HIP_PFB_COMPLEX;
    if (m < (cplx ? 16u : 32u) || m > stft_max_n(precision))
        return fail(SDSP_HIP_ERR_UNSUPPORTED,
                    "channels_m must be in the transform range (f32 .. 65536, f64 .. 32768; from 32 for real output, 16 for complex)");
    if (int rc = use_device(device))
        return rc;
    const uint64_t taps_n = static_cast<uint64_t>(m) * taps_per_channel;
    const uint64_t unit_bytes = static_cast<uint64_t>(m) * real_size(precision) * (cplx ? 2 : 1);
    const uint64_t budget = workspace_bytes ? workspace_bytes : kPfbDefaultBudget;
    auto *p = new sdsp_hip_pfb_synth_plan();
    p->m = m;
    p->p = taps_per_channel;
    p->hop = hop;
    p->hist = static_cast<uint32_t>(taps_n - hop);
    p->bins = cplx ? m : m / 2 + 1;
    p->kind = output_kind;
    p->phase = phase;
    p->precision = precision;
    p->device = device;
    p->ws_units = slice_units(budget, unit_bytes);
    p->workspace_bytes = p->ws_units * unit_bytes;
    int rc = cplx ? fft_plan_create(&p->inner, m, SDSP_HIP_RADIX_AUTO, SDSP_HIP_REVERSE, precision, p->ws_units, device, 0)
                  : fft_plan_create(&p->inner, m / 2, 2, SDSP_HIP_REVERSE, precision, p->ws_units, device, 2);
    if (!rc) {
        hipError_t e = hipMalloc(&p->ws, p->workspace_bytes);
        if (e == hipSuccess)
            e = upload_reals(taps, taps_n, precision, &p->taps);
        if (e != hipSuccess)
            rc = plan_fail(e, "pfb synthesis");
    }
    if (rc) {
        sdsp_hip_pfb_synth_plan_destroy(p);
        return rc;
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_pfb_synth_plan_destroy(sdsp_hip_pfb_synth_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    free_bank(p->device, p->ws, p->taps, p->inner);
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_pfb_synth_state_bytes(const sdsp_hip_pfb_synth_plan *p, uint64_t channels, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = static_cast<uint64_t>(p->hist) * channels * pfb_synth_out_esize(p);
    return SDSP_HIP_OK;
}

int sdsp_hip_pfb_synth_plan_set_variant(sdsp_hip_pfb_synth_plan *p, int variant)
{
    if (!p || variant < 0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "bad argument");
    return set_inner_variant(p->inner, variant, "the inner plan has no such kernel variant", true);
}

int sdsp_hip_pfb_synth_plan_set_unfold_form(sdsp_hip_pfb_synth_plan *p, int form)
{
    if (!p || (form != 0 && form != 1))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "form must be 0 (chosen from the sizes) or 1 (plain)");
    p->form = form;
    return SDSP_HIP_OK;
}

int sdsp_hip_pfb_synth_plan_get_info(const sdsp_hip_pfb_synth_plan *p, sdsp_hip_pfb_synth_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->channels_m = p->m;
    info->taps_per_channel = p->p;
    info->hop = p->hop;
    info->bins = p->bins;
    info->hist = p->hist;
    info->output_kind = p->kind;
    info->phase = p->phase;
    info->precision = p->precision;
    info->device = p->device;
    info->workspace_bytes = p->workspace_bytes;
    std::strncpy(info->kernel, select_kernel(p->inner, p->inner->variant).name, sizeof(info->kernel) - 1);
    std::strncpy(info->unfold, p->form ? "plain" : pfb_synth_form_for(p->m, p->hop), sizeof(info->unfold) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_pfb_synth_plan_launches(const sdsp_hip_pfb_synth_plan *p, uint64_t channels, uint64_t frames, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = 0;
    if (channels == 0 || frames == 0)
        return SDSP_HIP_OK;
    if (channels > ~0ull / frames)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many frames for one call");
    const uint64_t total = channels * frames;
    uint64_t n = slice_launch_count(p->inner, total, p->ws_units, 1); // per slice: the copy / pack launch and the transform's
    for (uint64_t g0 = 0; g0 < total; g0 += p->ws_units)
        pfb_rects(g0, std::min(p->ws_units, total - g0), frames, [&](uint64_t, uint64_t, uint32_t, uint32_t) {
            n++;
            return 0;
        });
    *launches = n + (p->hist ? 1 : 0);
    return SDSP_HIP_OK;
}

int sdsp_hip_pfb_synth_process(sdsp_hip_pfb_synth_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride,
                               uint64_t channels, uint64_t frames, uint64_t position, void *state, void *stream)
{
    if (int rc = pfb_synth_check(p, in, in_stride, out, out_stride, channels, frames))
        return rc;
    if (channels == 0 || frames == 0)
        return SDSP_HIP_OK;
    const uint64_t ies = esize(p->precision), oes = pfb_synth_out_esize(p);
    if (int rc = check_out_of_place(in, ((channels - 1) * in_stride + frames * p->bins) * ies, ies, out,
                                    ((channels - 1) * out_stride + frames * p->hop) * oes, oes, state, oes,
                                    "in and out ranges overlap (the synthesis bank runs out of place)"))
        return rc;
    if (int rc = use_device(p->device))
        return rc;
    return pfb_synth_run(p, in, in_stride, out, out_stride, channels, frames, position, state, reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_pfb_synth_process_host(sdsp_hip_pfb_synth_plan *p, const void *host_in, uint64_t in_stride, void *host_out,
                                    uint64_t out_stride, uint64_t channels, uint64_t frames, uint64_t position, void *host_state)
{
    if (int rc = pfb_synth_check(p, host_in, in_stride, host_out, out_stride, channels, frames))
        return rc;
    if (channels == 0 || frames == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const size_t in_bytes = ((channels - 1) * in_stride + frames * p->bins) * esize(p->precision);
    const size_t out_bytes = ((channels - 1) * out_stride + frames * p->hop) * pfb_synth_out_esize(p);
    uint64_t state_bytes = 0;
    sdsp_hip_pfb_synth_state_bytes(p, channels, &state_bytes);
    const bool with_state = host_state && state_bytes;
    host_stage st("pfb synthesis", { { host_in, in_bytes, false }, { host_out, out_bytes, true },
                                 { with_state ? host_state : nullptr, state_bytes, true } });
    int rc = st.in();
    if (!rc)
        rc = pfb_synth_run(p, st.dev[0], in_stride, st.dev[1], out_stride, channels, frames, position, st.dev[2], nullptr);
    return st.out(rc);
}

// ------------------------------------------------------------------ digital down-converter banks (ddc.hip)

namespace
{
uint64_t ddc_in_esize(const sdsp_hip_ddc_plan *p)
{
    return p->kind == SDSP_HIP_DDC_COMPLEX ? esize(p->precision) : real_size(p->precision);
}

// argument checks shared by process and process_host (device pointers or not)
int ddc_check(const sdsp_hip_ddc_plan *p, const void *in, uint64_t in_stride, const void *out, uint64_t out_stride, uint64_t samples,
              uint64_t *outs)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (int rc = sdsp_hip_ddc_out_samples(p->down, samples, outs))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    if (!in || !out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in or out is null");
    if ((p->channels > 1 && in_stride < samples) || (p->nb > 1 && out_stride < *outs))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_stride must be >= samples and out_stride >= samples / down");
    return SDSP_HIP_OK;
}

int ddc_run(sdsp_hip_ddc_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t samples, uint64_t position,
            void *state, hipStream_t stream)
{
    ddc_args a{};
    a.in = in;
    a.out = out;
    a.state = p->hist ? state : nullptr;
    a.g = p->g;
    a.coarse = p->osc;
    a.fine = static_cast<char *>(p->osc) + 65536 * esize(p->precision);
    a.csr = p->table;
    a.bands = p->table + p->channels + 1;
    a.samples = samples;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.position = position;
    a.taps = p->taps;
    a.down = p->down;
    a.channels = p->channels;
    a.nb = p->nb;
    a.complex_in = p->kind == SDSP_HIP_DDC_COMPLEX;
    if (int rc = launch_ddc(p->precision, a, p->variant, stream))
        return rc;
    // behind the band kernel: it reads the old history
    return carry_history(p->precision, static_cast<uint32_t>(ddc_in_esize(p)), in, in_stride, state, p->channels, samples, p->hist, stream,
                         "ddc");
}
} // namespace

int sdsp_hip_ddc_plan_create(sdsp_hip_ddc_plan **out, uint32_t taps, const double *h, uint32_t down, uint32_t channels, uint32_t nb,
                             const sdsp_hip_ddc_band *bands, int input_kind, int precision, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (taps == 0 || taps > SDSP_HIP_FIR_MAX_TAPS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps must be in [1, SDSP_HIP_FIR_MAX_TAPS]");
    if (down == 0 || down > SDSP_HIP_RESAMPLE_MAX_FACTOR)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "down must be in [1, SDSP_HIP_RESAMPLE_MAX_FACTOR]");
    if (channels == 0 || channels > 0x7fffffffu)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "channels must be in [1, 2^31)");
    if (nb == 0 || nb > SDSP_HIP_DDC_MAX_BANDS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "the band count must be in [1, SDSP_HIP_DDC_MAX_BANDS]");
    if (!h || !bands)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "coefficient or band pointer is null");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (input_kind != SDSP_HIP_DDC_REAL && input_kind != SDSP_HIP_DDC_COMPLEX)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "input_kind must be SDSP_HIP_DDC_REAL or SDSP_HIP_DDC_COMPLEX");
    for (uint32_t i = 0; i < nb; i++)
        if (bands[i].src >= channels)
            return fail(SDSP_HIP_ERR_INVALID_ARG, "a band names an input channel the plan does not have");
    if (int rc = use_device(device))
        return rc;
    if (int rc = ddc_prepare(precision, input_kind == SDSP_HIP_DDC_COMPLEX))
        return rc;
    // the bands sorted by source channel (stable: equal sources keep the caller's order), and where each channel's run starts.  The
    // host tables grow with channels and nb T: running out of host memory for them is an error code, not an exception
    std::vector<uint32_t> order, table;
    std::vector<double> g, osc;
    try {
        order.resize(nb);
        table.assign(static_cast<size_t>(channels) + 1 + 4 * static_cast<size_t>(nb), 0);
        g.resize(static_cast<size_t>(nb) * taps * 2);
        osc.resize(4 * 65536);
    } catch (const std::bad_alloc &) {
        return fail(SDSP_HIP_ERR_NOMEM, "ddc plan: out of host memory for the band tables");
    }
    for (uint32_t i = 0; i < nb; i++)
        order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return bands[a].src < bands[b].src; });
    for (uint32_t s = 0; s < nb; s++) {
        const sdsp_hip_ddc_band &b = bands[order[s]];
        table[b.src + 1]++;
        uint32_t *e = &table[static_cast<size_t>(channels) + 1 + 4 * static_cast<size_t>(s)];
        e[0] = order[s];
        e[1] = b.src;
        e[2] = b.fcw;
        e[3] = b.phase0;
        sdsp_hip_ddc_band_taps(taps, h, b.fcw, &g[static_cast<size_t>(s) * taps * 2]);
    }
    for (uint32_t c = 0; c < channels; c++)
        table[c + 1] += table[c];
    sdsp_hip_ddc_oscillator(osc.data(), osc.data() + 2 * 65536);
    auto *p = new sdsp_hip_ddc_plan();
    p->taps = taps;
    p->down = down;
    p->hist = taps - 1;
    p->channels = channels;
    p->nb = nb;
    p->kind = input_kind;
    p->precision = precision;
    p->device = device;
    hipError_t e = upload_reals(g.data(), g.size(), precision, &p->g);
    if (e == hipSuccess)
        e = upload_reals(osc.data(), osc.size(), precision, &p->osc);
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void **>(&p->table), table.size() * sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipMemcpy(p->table, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        sdsp_hip_ddc_plan_destroy(p);
        return plan_fail(e, "ddc");
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_ddc_plan_destroy(sdsp_hip_ddc_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK) {
        (void)hipFree(p->g);
        (void)hipFree(p->osc);
        (void)hipFree(p->table);
    }
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_ddc_state_bytes(const sdsp_hip_ddc_plan *p, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = static_cast<uint64_t>(p->hist) * p->channels * ddc_in_esize(p);
    return SDSP_HIP_OK;
}

int sdsp_hip_ddc_plan_set_variant(sdsp_hip_ddc_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_ddc_plan_launches(const sdsp_hip_ddc_plan *p, uint64_t samples, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = 0;
    uint64_t outs = 0;
    if (int rc = sdsp_hip_ddc_out_samples(p->down, samples, &outs))
        return rc;
    if (samples)
        *launches = 1 + (p->hist ? 1 : 0);
    return SDSP_HIP_OK;
}

int sdsp_hip_ddc_plan_get_info(const sdsp_hip_ddc_plan *p, sdsp_hip_ddc_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->taps = p->taps;
    info->down = p->down;
    info->channels = p->channels;
    info->bands = p->nb;
    info->hist = p->hist;
    info->block_out = ddc_block_out(p->precision, p->kind == SDSP_HIP_DDC_COMPLEX, p->taps, p->down);
    info->input_kind = p->kind;
    info->precision = p->precision;
    info->device = p->device;
    std::strncpy(info->kernel, ddc_kernel_for(p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_ddc_process(sdsp_hip_ddc_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t samples,
                         uint64_t position, void *state, void *stream)
{
    uint64_t outs = 0;
    if (int rc = ddc_check(p, in, in_stride, out, out_stride, samples, &outs))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    const uint64_t ies = ddc_in_esize(p), oes = esize(p->precision);
    if (int rc = check_out_of_place(in, ((p->channels - 1) * in_stride + samples) * ies, ies, out, ((p->nb - 1) * out_stride + outs) * oes,
                                    oes, state, ies, "in and out ranges overlap (the down-converter runs out of place)"))
        return rc;
    if (int rc = use_device(p->device))
        return rc;
    return ddc_run(p, in, in_stride, out, out_stride, samples, position, state, reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_ddc_process_host(sdsp_hip_ddc_plan *p, const void *host_in, uint64_t in_stride, void *host_out, uint64_t out_stride,
                              uint64_t samples, uint64_t position, void *host_state)
{
    uint64_t outs = 0;
    if (int rc = ddc_check(p, host_in, in_stride, host_out, out_stride, samples, &outs))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const size_t in_bytes = ((p->channels - 1) * in_stride + samples) * ddc_in_esize(p);
    const size_t out_bytes = ((p->nb - 1) * out_stride + outs) * esize(p->precision);
    uint64_t state_bytes = 0;
    sdsp_hip_ddc_state_bytes(p, &state_bytes);
    const bool with_state = host_state && state_bytes;
    host_stage st("ddc", { { host_in, in_bytes, false }, { host_out, out_bytes, true },
                       { with_state ? host_state : nullptr, state_bytes, true } });
    int rc = st.in();
    if (!rc)
        rc = ddc_run(p, st.dev[0], in_stride, st.dev[1], out_stride, samples, position, st.dev[2], nullptr);
    return st.out(rc);
}
// ------------------------------------------------------------------ digital up-converter banks (duc.hip)

namespace
{
uint64_t duc_out_esize(const sdsp_hip_duc_plan *p)
{
    return p->kind == SDSP_HIP_DUC_COMPLEX ? esize(p->precision) : real_size(p->precision);
}

// argument checks shared by process and process_host (device pointers or not)
int duc_check(const sdsp_hip_duc_plan *p, const void *in, uint64_t in_stride, const void *out, uint64_t out_stride, uint64_t samples,
              uint64_t *outs)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (int rc = sdsp_hip_duc_out_samples(p->up, samples, outs))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    if (!in || !out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in or out is null");
    if ((p->nb > 1 && in_stride < samples) || (p->channels > 1 && out_stride < *outs))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_stride must be >= samples and out_stride >= samples * up");
    return SDSP_HIP_OK;
}

int duc_run(sdsp_hip_duc_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t samples, uint64_t position,
            void *state, hipStream_t stream)
{
    duc_args a{};
    a.in = in;
    a.out = out;
    a.state = p->hist ? state : nullptr;
    a.h = p->h;
    a.coarse = p->osc;
    a.fine = static_cast<char *>(p->osc) + 65536 * esize(p->precision);
    a.csr = p->table;
    a.bands = p->table + p->channels + 1;
    a.samples = samples;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.position = position;
    a.taps = p->taps;
    a.up = p->up;
    a.channels = p->channels;
    a.nb = p->nb;
    a.real_out = p->kind == SDSP_HIP_DUC_REAL;
    if (int rc = launch_duc(p->precision, a, p->variant, stream))
        return rc;
    // behind the band kernel: it reads the old history
    return carry_history(p->precision, static_cast<uint32_t>(esize(p->precision)), in, in_stride, state, p->nb, samples, p->hist, stream,
                         "duc");
}
} // namespace

int sdsp_hip_duc_plan_create(sdsp_hip_duc_plan **out, uint32_t taps, const double *h, uint32_t up, uint32_t channels, uint32_t nb,
                             const sdsp_hip_duc_band *bands, int output_kind, int precision, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (taps == 0 || taps > SDSP_HIP_FIR_MAX_TAPS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps must be in [1, SDSP_HIP_FIR_MAX_TAPS]");
    if (up == 0 || up > SDSP_HIP_RESAMPLE_MAX_FACTOR)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "up must be in [1, SDSP_HIP_RESAMPLE_MAX_FACTOR]");
    if (channels == 0 || channels > 0x7fffffffu)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "channels must be in [1, 2^31)");
    if (nb == 0 || nb > SDSP_HIP_DUC_MAX_BANDS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "the band count must be in [1, SDSP_HIP_DUC_MAX_BANDS]");
    if (!h || !bands)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "coefficient or band pointer is null");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (output_kind != SDSP_HIP_DUC_REAL && output_kind != SDSP_HIP_DUC_COMPLEX)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "output_kind must be SDSP_HIP_DUC_REAL or SDSP_HIP_DUC_COMPLEX");
    for (uint32_t i = 0; i < nb; i++)
        if (bands[i].dst >= channels)
            return fail(SDSP_HIP_ERR_INVALID_ARG, "a band names an output channel the plan does not have");
    if (int rc = use_device(device))
        return rc;
    if (int rc = duc_prepare(precision, output_kind == SDSP_HIP_DUC_REAL))
        return rc;
    // the bands sorted by output channel (stable: equal channels keep the caller's order, which is the order of the sum), and where
    // each channel's run starts.  Running out of host memory for the tables is an error code, not an exception
    std::vector<uint32_t> order, table;
    std::vector<double> osc;
    try {
        order.resize(nb);
        table.assign(static_cast<size_t>(channels) + 1 + 4 * static_cast<size_t>(nb), 0);
        osc.resize(4 * 65536);
    } catch (const std::bad_alloc &) {
        return fail(SDSP_HIP_ERR_NOMEM, "duc plan: out of host memory for the band tables");
    }
    for (uint32_t i = 0; i < nb; i++)
        order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return bands[a].dst < bands[b].dst; });
    for (uint32_t s = 0; s < nb; s++) {
        const sdsp_hip_duc_band &b = bands[order[s]];
        table[b.dst + 1]++;
        uint32_t *e = &table[static_cast<size_t>(channels) + 1 + 4 * static_cast<size_t>(s)];
        e[0] = order[s];
        e[1] = b.dst;
        e[2] = b.fcw;
        e[3] = b.phase0;
    }
    for (uint32_t c = 0; c < channels; c++)
        table[c + 1] += table[c];
    sdsp_hip_ddc_oscillator(osc.data(), osc.data() + 2 * 65536);
    auto *p = new sdsp_hip_duc_plan();
    p->taps = taps;
    p->up = up;
    p->hist = (taps - 1) / up;
    p->channels = channels;
    p->nb = nb;
    p->kind = output_kind;
    p->precision = precision;
    p->device = device;
    hipError_t e = upload_reals(h, taps, precision, &p->h);
    if (e == hipSuccess)
        e = upload_reals(osc.data(), osc.size(), precision, &p->osc);
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void **>(&p->table), table.size() * sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipMemcpy(p->table, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        sdsp_hip_duc_plan_destroy(p);
        return plan_fail(e, "duc");
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_duc_plan_destroy(sdsp_hip_duc_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK) {
        (void)hipFree(p->h);
        (void)hipFree(p->osc);
        (void)hipFree(p->table);
    }
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_duc_state_bytes(const sdsp_hip_duc_plan *p, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = static_cast<uint64_t>(p->hist) * p->nb * esize(p->precision);
    return SDSP_HIP_OK;
}

int sdsp_hip_duc_plan_set_variant(sdsp_hip_duc_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_duc_plan_launches(const sdsp_hip_duc_plan *p, uint64_t samples, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = 0;
    uint64_t outs = 0;
    if (int rc = sdsp_hip_duc_out_samples(p->up, samples, &outs))
        return rc;
    if (samples)
        *launches = 1 + (p->hist ? 1 : 0);
    return SDSP_HIP_OK;
}

int sdsp_hip_duc_plan_get_info(const sdsp_hip_duc_plan *p, sdsp_hip_duc_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->taps = p->taps;
    info->up = p->up;
    info->channels = p->channels;
    info->bands = p->nb;
    info->hist = p->hist;
    info->block_in = duc_block_in(p->precision, p->taps, p->up);
    info->output_kind = p->kind;
    info->precision = p->precision;
    info->device = p->device;
    std::strncpy(info->kernel, duc_kernel_for(p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_duc_process(sdsp_hip_duc_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t samples,
                         uint64_t position, void *state, void *stream)
{
    uint64_t outs = 0;
    if (int rc = duc_check(p, in, in_stride, out, out_stride, samples, &outs))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    const uint64_t ies = esize(p->precision), oes = duc_out_esize(p);
    if (int rc = check_out_of_place(in, ((p->nb - 1) * in_stride + samples) * ies, ies, out, ((p->channels - 1) * out_stride + outs) * oes,
                                    oes, state, ies, "in and out ranges overlap (the up-converter runs out of place)"))
        return rc;
    if (int rc = use_device(p->device))
        return rc;
    return duc_run(p, in, in_stride, out, out_stride, samples, position, state, reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_duc_process_host(sdsp_hip_duc_plan *p, const void *host_in, uint64_t in_stride, void *host_out, uint64_t out_stride,
                              uint64_t samples, uint64_t position, void *host_state)
{
    uint64_t outs = 0;
    if (int rc = duc_check(p, host_in, in_stride, host_out, out_stride, samples, &outs))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const size_t in_bytes = ((p->nb - 1) * in_stride + samples) * esize(p->precision);
    const size_t out_bytes = ((p->channels - 1) * out_stride + outs) * duc_out_esize(p);
    uint64_t state_bytes = 0;
    sdsp_hip_duc_state_bytes(p, &state_bytes);
    const bool with_state = host_state && state_bytes;
    host_stage st("duc", { { host_in, in_bytes, false }, { host_out, out_bytes, true },
                       { with_state ? host_state : nullptr, state_bytes, true } });
    int rc = st.in();
    if (!rc)
        rc = duc_run(p, st.dev[0], in_stride, st.dev[1], out_stride, samples, position, st.dev[2], nullptr);
    return st.out(rc);
}

// ------------------------------------------------------------------ arbitrary-ratio resampler banks (arb_resample.hip)

namespace
{
uint64_t arb_esize(const sdsp_hip_arb_plan *p) { return p->kind == SDSP_HIP_ARB_COMPLEX ? esize(p->precision) : real_size(p->precision); }

// argument checks shared by process and process_host (device pointers or not)
int arb_check(const sdsp_hip_arb_plan *p, const void *in, uint64_t in_stride, const void *out, uint64_t out_stride, uint64_t channels,
              uint64_t samples, uint64_t step, uint64_t time, uint64_t *outs)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (step > p->max_step)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "step must be in [2^22, the plan's max_step]");
    if (int rc = sdsp_hip_arb_out_samples(step, time, samples, outs, nullptr))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (!in || (*outs && !out))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in or out is null");
    if (channels > 1 && (in_stride < samples || out_stride < *outs))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_stride must be >= samples and out_stride >= the call's outputs per channel");
    return SDSP_HIP_OK;
}

int arb_run(sdsp_hip_arb_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t channels, uint64_t samples,
            uint64_t step, uint64_t time, uint64_t outs, void *state, hipStream_t stream)
{
    if (outs) {
        arb_args a{};
        a.in = in;
        a.out = out;
        a.state = p->hist ? state : nullptr;
        a.table = p->table;
        a.channels = channels;
        a.samples = samples;
        a.in_stride = in_stride;
        a.out_stride = out_stride;
        a.step = step;
        a.time = time;
        a.n_out = outs;
        a.block_out = p->block_out;
        a.phases = p->phases;
        a.taps = p->taps;
        a.complex_in = p->kind == SDSP_HIP_ARB_COMPLEX;
        a.linear = p->interp == SDSP_HIP_ARB_LINEAR;
        if (int rc = launch_arb(p->precision, a, p->variant, stream))
            return rc;
    }
    // behind the resampling kernel: it reads the old history.  Also when the call made no output
    return carry_history(p->precision, static_cast<uint32_t>(arb_esize(p)), in, in_stride, state, channels, samples, p->hist, stream, "arb");
}
} // namespace

int sdsp_hip_arb_plan_create(sdsp_hip_arb_plan **out, uint32_t phases, uint32_t taps, const double *h, uint64_t max_step, int input_kind,
                             int interp, int precision, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (phases == 0 || phases > SDSP_HIP_ARB_MAX_PHASES || (phases & (phases - 1)))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "phases must be a power of 2 in [1, SDSP_HIP_ARB_MAX_PHASES]");
    if (taps == 0 || static_cast<uint64_t>(phases) * taps > SDSP_HIP_FIR_MAX_TAPS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps per phase must be >= 1 and phases * taps <= SDSP_HIP_FIR_MAX_TAPS");
    if (max_step < SDSP_HIP_ARB_MIN_STEP || max_step > SDSP_HIP_ARB_MAX_STEP)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "max_step must be in [2^22, 2^42]");
    if (!h)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "coefficient pointer is null");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (input_kind != SDSP_HIP_ARB_REAL && input_kind != SDSP_HIP_ARB_COMPLEX)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "input_kind must be SDSP_HIP_ARB_REAL or SDSP_HIP_ARB_COMPLEX");
    if (interp != SDSP_HIP_ARB_NEAREST && interp != SDSP_HIP_ARB_LINEAR)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "interp must be SDSP_HIP_ARB_NEAREST or SDSP_HIP_ARB_LINEAR");
    if (int rc = use_device(device))
        return rc;
    if (int rc = arb_prepare(precision, input_kind == SDSP_HIP_ARB_COMPLEX, interp == SDSP_HIP_ARB_LINEAR))
        return rc;
    const uint32_t block_out = arb_block_out(precision, input_kind == SDSP_HIP_ARB_COMPLEX, interp == SDSP_HIP_ARB_LINEAR, phases, taps, max_step);
    if (block_out == 0)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "arb plan: the line of one output does not fit the LDS next to the table");
    const size_t n = static_cast<size_t>(phases) * taps;
    std::vector<double> th(n), td(n), tab;
    sdsp_hip_arb_tables(phases, taps, h, th.data(), td.data());
    if (interp == SDSP_HIP_ARB_LINEAR) {
        tab.resize(2 * n);
        for (size_t i = 0; i < n; i++) {
            tab[2 * i] = th[i];
            tab[2 * i + 1] = td[i];
        }
    } else {
        tab = th;
    }
    auto *p = new sdsp_hip_arb_plan();
    p->phases = phases;
    p->taps = taps;
    p->hist = taps - 1;
    p->max_step = max_step;
    p->block_out = block_out;
    p->kind = input_kind;
    p->interp = interp;
    p->precision = precision;
    p->device = device;
    const hipError_t e = upload_reals(tab.data(), tab.size(), precision, &p->table);
    if (e != hipSuccess) {
        sdsp_hip_arb_plan_destroy(p);
        return plan_fail(e, "arb");
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_arb_plan_destroy(sdsp_hip_arb_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK)
        (void)hipFree(p->table);
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_arb_state_bytes(const sdsp_hip_arb_plan *p, uint64_t channels, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = static_cast<uint64_t>(p->hist) * channels * arb_esize(p);
    return SDSP_HIP_OK;
}

int sdsp_hip_arb_plan_set_variant(sdsp_hip_arb_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_arb_plan_launches(const sdsp_hip_arb_plan *p, uint64_t step, uint64_t time, uint64_t samples, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = 0;
    if (step > p->max_step)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "step must be in [2^22, the plan's max_step]");
    uint64_t outs = 0;
    if (int rc = sdsp_hip_arb_out_samples(step, time, samples, &outs, nullptr))
        return rc;
    if (samples)
        *launches = (outs ? 1 : 0) + (p->hist ? 1 : 0);
    return SDSP_HIP_OK;
}

int sdsp_hip_arb_plan_get_info(const sdsp_hip_arb_plan *p, sdsp_hip_arb_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->phases = p->phases;
    info->taps = p->taps;
    info->hist = p->hist;
    info->block_out = p->block_out;
    info->max_step = p->max_step;
    info->input_kind = p->kind;
    info->interp = p->interp;
    info->precision = p->precision;
    info->device = p->device;
    std::strncpy(info->kernel, arb_kernel_for(p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_arb_process(sdsp_hip_arb_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t channels,
                         uint64_t samples, uint64_t step, uint64_t time, void *state, void *stream)
{
    uint64_t outs = 0;
    if (int rc = arb_check(p, in, in_stride, out, out_stride, channels, samples, step, time, &outs))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    const uint64_t es = arb_esize(p);
    if (int rc = check_out_of_place(in, ((channels - 1) * in_stride + samples) * es, es, outs ? out : nullptr,
                                    ((channels - 1) * out_stride + outs) * es, es, state, es,
                                    "in and out ranges overlap (the resampler runs out of place)"))
        return rc;
    if (int rc = use_device(p->device))
        return rc;
    return arb_run(p, in, in_stride, out, out_stride, channels, samples, step, time, outs, state, reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_arb_process_host(sdsp_hip_arb_plan *p, const void *host_in, uint64_t in_stride, void *host_out, uint64_t out_stride,
                              uint64_t channels, uint64_t samples, uint64_t step, uint64_t time, void *host_state)
{
    uint64_t outs = 0;
    if (int rc = arb_check(p, host_in, in_stride, host_out, out_stride, channels, samples, step, time, &outs))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const size_t in_bytes = ((channels - 1) * in_stride + samples) * arb_esize(p);
    const size_t out_bytes = ((channels - 1) * out_stride + outs) * arb_esize(p);
    uint64_t state_bytes = 0;
    sdsp_hip_arb_state_bytes(p, channels, &state_bytes);
    const bool with_state = host_state && state_bytes;
    host_stage st("arb", { { host_in, in_bytes, false }, { outs ? host_out : nullptr, out_bytes, true },
                       { with_state ? host_state : nullptr, state_bytes, true } });
    int rc = st.in();
    if (!rc)
        rc = arb_run(p, st.dev[0], in_stride, st.dev[1], out_stride, channels, samples, step, time, outs, st.dev[2], nullptr);
    return st.out(rc);
}

// ------------------------------------------------------------------ CIC decimator banks (cic.hip)

namespace
{
uint64_t cic_in_esize(const sdsp_hip_cic_plan *p)
{
    return (p->in_type == SDSP_HIP_CIC_I32 ? 4u : 2u) * (p->kind == SDSP_HIP_CIC_COMPLEX ? 2u : 1u);
}
uint64_t cic_out_esize(const sdsp_hip_cic_plan *p)
{
    return (p->out_kind == SDSP_HIP_CIC_OUT_INT && p->reg_bits == 64 ? 8u : 4u) * (p->kind == SDSP_HIP_CIC_COMPLEX ? 2u : 1u);
}

// argument checks shared by process and process_host (device pointers or not)
int cic_check(const sdsp_hip_cic_plan *p, const void *in, uint64_t in_stride, const void *out, uint64_t out_stride, uint64_t channels,
              uint64_t samples, uint64_t position, uint64_t *outs)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (int rc = sdsp_hip_cic_out_samples(p->down, position, samples, outs))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (!in || (*outs && !out))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in or out is null");
    if (channels > 1 && (in_stride < samples || out_stride < *outs))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_stride must be >= samples and out_stride >= the call's outputs per channel");
    return SDSP_HIP_OK;
}

int cic_run(sdsp_hip_cic_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t channels, uint64_t samples,
            uint64_t position, uint64_t outs, void *state, hipStream_t stream)
{
    if (outs) {
        cic_args a{};
        a.in = in;
        a.out = out;
        a.state = state;
        a.taps = p->taps;
        a.channels = channels;
        a.samples = samples;
        a.in_stride = in_stride;
        a.out_stride = out_stride;
        a.position = position;
        a.n_out = outs;
        a.order = p->order;
        a.down = p->down;
        a.delay = p->delay;
        a.segment = p->segment;
        a.in32 = p->in_type == SDSP_HIP_CIC_I32;
        a.complex_in = p->kind == SDSP_HIP_CIC_COMPLEX;
        a.reg64 = p->reg_bits == 64;
        a.out_f32 = p->out_kind == SDSP_HIP_CIC_OUT_F32;
        a.scale = p->scale;
        if (int rc = launch_cic(a, p->variant, stream))
            return rc;
    }
    // behind the decimating kernel: it reads the old history.  Also when the call made no output.  Integer elements of 4 and 8
    // bytes move as the f32 ones do
    return carry_history(SDSP_HIP_F32, static_cast<uint32_t>(cic_in_esize(p)), in, in_stride, state, channels, samples, p->hist, stream,
                         "cic");
}
} // namespace

int sdsp_hip_cic_plan_create(sdsp_hip_cic_plan **out, uint32_t order, uint32_t down, uint32_t delay, int in_type, uint32_t in_bits,
                             int input_kind, int out_kind, double scale, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    uint32_t growth = 0;
    if (int rc = sdsp_hip_cic_growth(order, down, delay, &growth)) // the size checks
        return rc;
    if (in_type != SDSP_HIP_CIC_I16 && in_type != SDSP_HIP_CIC_I32)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_type must be SDSP_HIP_CIC_I16 or SDSP_HIP_CIC_I32");
    if (input_kind != SDSP_HIP_CIC_REAL && input_kind != SDSP_HIP_CIC_COMPLEX)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "input_kind must be SDSP_HIP_CIC_REAL or SDSP_HIP_CIC_COMPLEX");
    if (out_kind != SDSP_HIP_CIC_OUT_INT && out_kind != SDSP_HIP_CIC_OUT_F32)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "out_kind must be SDSP_HIP_CIC_OUT_INT or SDSP_HIP_CIC_OUT_F32");
    if (in_bits < 2 || in_bits > (in_type == SDSP_HIP_CIC_I32 ? 32u : 16u))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "in_bits must be in [2, 16] for I16 and [2, 32] for I32");
    if (!std::isfinite(scale))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "scale must be finite");
    if (in_bits + growth > 64)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "cic plan: in_bits " + std::to_string(in_bits) + " + growth " + std::to_string(growth) + " = " +
                                                  std::to_string(in_bits + growth) + " bits exceed the 64-bit registers");
    if (int rc = use_device(device))
        return rc;
    auto *p = new sdsp_hip_cic_plan();
    p->order = order;
    p->down = down;
    p->delay = delay;
    p->hist = order * delay * down;
    p->in_bits = in_bits;
    p->growth = growth;
    p->reg_bits = in_bits + growth <= 32 ? 32 : 64;
    p->in_type = in_type;
    p->kind = input_kind;
    p->out_kind = out_kind;
    p->scale = scale;
    p->device = device;
    std::vector<uint64_t> h(static_cast<size_t>(order) * (down * delay - 1) + 1);
    sdsp_hip_cic_taps(order, down, delay, h.data());
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&p->taps), h.size() * sizeof(uint64_t));
    if (e == hipSuccess)
        e = hipMemcpy(p->taps, h.data(), h.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        sdsp_hip_cic_plan_destroy(p);
        return plan_fail(e, "cic");
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_cic_plan_destroy(sdsp_hip_cic_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK)
        (void)hipFree(p->taps);
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_cic_state_bytes(const sdsp_hip_cic_plan *p, uint64_t channels, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = static_cast<uint64_t>(p->hist) * channels * cic_in_esize(p);
    return SDSP_HIP_OK;
}

int sdsp_hip_cic_plan_set_variant(sdsp_hip_cic_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_cic_plan_set_segment(sdsp_hip_cic_plan *p, uint32_t chunks)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (chunks >= (1u << 20))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "chunks per segment must be below 2^20");
    p->segment = chunks;
    return SDSP_HIP_OK;
}

int sdsp_hip_cic_plan_launches(const sdsp_hip_cic_plan *p, uint64_t position, uint64_t samples, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = 0;
    uint64_t outs = 0;
    if (int rc = sdsp_hip_cic_out_samples(p->down, position, samples, &outs))
        return rc;
    if (samples)
        *launches = (outs ? 1 : 0) + 1;
    return SDSP_HIP_OK;
}

int sdsp_hip_cic_plan_get_info(const sdsp_hip_cic_plan *p, sdsp_hip_cic_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->order = p->order;
    info->down = p->down;
    info->delay = p->delay;
    info->hist = p->hist;
    info->in_bits = p->in_bits;
    info->growth = p->growth;
    info->reg_bits = p->reg_bits;
    info->chunk = cic_chunk();
    info->segment = p->segment;
    info->in_type = p->in_type;
    info->input_kind = p->kind;
    info->out_kind = p->out_kind;
    info->device = p->device;
    info->scale = p->scale;
    std::strncpy(info->kernel, cic_kernel_for(p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_cic_process(sdsp_hip_cic_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t channels,
                         uint64_t samples, uint64_t position, void *state, void *stream)
{
    uint64_t outs = 0;
    if (int rc = cic_check(p, in, in_stride, out, out_stride, channels, samples, position, &outs))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    const uint64_t ies = cic_in_esize(p), oes = cic_out_esize(p);
    if (int rc = check_out_of_place(in, ((channels - 1) * in_stride + samples) * ies, ies, outs ? out : nullptr,
                                    ((channels - 1) * out_stride + outs) * oes, oes, state, ies,
                                    "in and out ranges overlap (the decimator runs out of place)"))
        return rc;
    if (int rc = use_device(p->device))
        return rc;
    return cic_run(p, in, in_stride, out, out_stride, channels, samples, position, outs, state, reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_cic_process_host(sdsp_hip_cic_plan *p, const void *host_in, uint64_t in_stride, void *host_out, uint64_t out_stride,
                              uint64_t channels, uint64_t samples, uint64_t position, void *host_state)
{
    uint64_t outs = 0;
    if (int rc = cic_check(p, host_in, in_stride, host_out, out_stride, channels, samples, position, &outs))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const size_t in_bytes = ((channels - 1) * in_stride + samples) * cic_in_esize(p);
    const size_t out_bytes = ((channels - 1) * out_stride + outs) * cic_out_esize(p);
    uint64_t state_bytes = 0;
    sdsp_hip_cic_state_bytes(p, channels, &state_bytes);
    host_stage st("cic", { { host_in, in_bytes, false }, { outs ? host_out : nullptr, out_bytes, true },
                       { host_state, state_bytes, true } });
    int rc = st.in();
    if (!rc)
        rc = cic_run(p, st.dev[0], in_stride, st.dev[1], out_stride, channels, samples, position, outs, st.dev[2], nullptr);
    return st.out(rc);
}

// ------------------------------------------------------------------ CIC interpolator banks (cic_interp.hip)

namespace
{
uint64_t cic_interp_in_esize(const sdsp_hip_cic_interp_plan *p)
{
    return (p->in_type == SDSP_HIP_CIC_I32 ? 4u : 2u) * (p->kind == SDSP_HIP_CIC_COMPLEX ? 2u : 1u);
}
uint64_t cic_interp_out_esize(const sdsp_hip_cic_interp_plan *p)
{
    return (p->out_kind == SDSP_HIP_CIC_OUT_INT && p->reg_bits == 64 ? 8u : 4u) * (p->kind == SDSP_HIP_CIC_COMPLEX ? 2u : 1u);
}

// outputs per channel of a call: up * samples, below 2^31
int cic_interp_outs(const sdsp_hip_cic_interp_plan *p, uint64_t samples, uint64_t *outs)
{
    *outs = 0;
    if (samples >= (1ull << 31) || samples * p->up >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "up * samples must be below 2^31");
    *outs = samples * p->up;
    return SDSP_HIP_OK;
}

// argument checks shared by process and process_host (device pointers or not)
int cic_interp_check(const sdsp_hip_cic_interp_plan *p, const void *in, uint64_t in_stride, const void *out, uint64_t out_stride,
                     uint64_t channels, uint64_t samples, uint64_t *outs)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (int rc = cic_interp_outs(p, samples, outs))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (!in || !out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in or out is null");
    if (channels > 1 && (in_stride < samples || out_stride < *outs))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_stride must be >= samples and out_stride >= the call's outputs per channel");
    return SDSP_HIP_OK;
}

int cic_interp_run(sdsp_hip_cic_interp_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t channels,
                   uint64_t samples, void *state, hipStream_t stream)
{
    cic_interp_args a{};
    a.in = in;
    a.out = out;
    a.state = state;
    a.taps = p->taps;
    a.channels = channels;
    a.samples = samples;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.order = p->order;
    a.up = p->up;
    a.delay = p->delay;
    a.segment = p->segment;
    a.in32 = p->in_type == SDSP_HIP_CIC_I32;
    a.complex_in = p->kind == SDSP_HIP_CIC_COMPLEX;
    a.reg64 = p->reg_bits == 64;
    a.out_f32 = p->out_kind == SDSP_HIP_CIC_OUT_F32;
    a.scale = p->scale;
    if (int rc = launch_cic_interp(a, p->variant, stream))
        return rc;
    // behind the interpolating kernel: it reads the old history.  Also for calls shorter than the history.  Integer elements of 4
    // and 8 bytes move as the f32 ones do
    return carry_history(SDSP_HIP_F32, static_cast<uint32_t>(cic_interp_in_esize(p)), in, in_stride, state, channels, samples, p->hist,
                         stream, "cic_interp");
}
} // namespace

int sdsp_hip_cic_interp_plan_create(sdsp_hip_cic_interp_plan **out, uint32_t order, uint32_t up, uint32_t delay, int in_type,
                                    uint32_t in_bits, int input_kind, int out_kind, double scale, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    uint32_t growth = 0;
    if (int rc = sdsp_hip_cic_interp_growth(order, up, delay, &growth)) // the size checks
        return rc;
    if (in_type != SDSP_HIP_CIC_I16 && in_type != SDSP_HIP_CIC_I32)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_type must be SDSP_HIP_CIC_I16 or SDSP_HIP_CIC_I32");
    if (input_kind != SDSP_HIP_CIC_REAL && input_kind != SDSP_HIP_CIC_COMPLEX)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "input_kind must be SDSP_HIP_CIC_REAL or SDSP_HIP_CIC_COMPLEX");
    if (out_kind != SDSP_HIP_CIC_OUT_INT && out_kind != SDSP_HIP_CIC_OUT_F32)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "out_kind must be SDSP_HIP_CIC_OUT_INT or SDSP_HIP_CIC_OUT_F32");
    if (in_bits < 2 || in_bits > (in_type == SDSP_HIP_CIC_I32 ? 32u : 16u))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "in_bits must be in [2, 16] for I16 and [2, 32] for I32");
    if (!std::isfinite(scale))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "scale must be finite");
    if (in_bits + growth > 64)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "cic_interp plan: in_bits " + std::to_string(in_bits) + " + growth " + std::to_string(growth) +
                                                  " = " + std::to_string(in_bits + growth) + " bits exceed the 64-bit registers");
    if (int rc = use_device(device))
        return rc;
    auto *p = new sdsp_hip_cic_interp_plan();
    p->order = order;
    p->up = up;
    p->delay = delay;
    p->hist = order * delay;
    p->in_bits = in_bits;
    p->growth = growth;
    p->reg_bits = in_bits + growth <= 32 ? 32 : 64;
    p->in_type = in_type;
    p->kind = input_kind;
    p->out_kind = out_kind;
    p->scale = scale;
    p->device = device;
    std::vector<uint64_t> h(static_cast<size_t>(order) * (up * delay - 1) + 1);
    sdsp_hip_cic_taps(order, up, delay, h.data());
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&p->taps), h.size() * sizeof(uint64_t));
    if (e == hipSuccess)
        e = hipMemcpy(p->taps, h.data(), h.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        sdsp_hip_cic_interp_plan_destroy(p);
        return plan_fail(e, "cic_interp");
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_cic_interp_plan_destroy(sdsp_hip_cic_interp_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK)
        (void)hipFree(p->taps);
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_cic_interp_state_bytes(const sdsp_hip_cic_interp_plan *p, uint64_t channels, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = static_cast<uint64_t>(p->hist) * channels * cic_interp_in_esize(p);
    return SDSP_HIP_OK;
}

int sdsp_hip_cic_interp_plan_set_variant(sdsp_hip_cic_interp_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_cic_interp_plan_set_segment(sdsp_hip_cic_interp_plan *p, uint32_t chunks)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (chunks >= (1u << 20))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "chunks per segment must be below 2^20");
    p->segment = chunks;
    return SDSP_HIP_OK;
}

int sdsp_hip_cic_interp_plan_launches(const sdsp_hip_cic_interp_plan *p, uint64_t samples, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = 0;
    uint64_t outs = 0;
    if (int rc = cic_interp_outs(p, samples, &outs))
        return rc;
    if (samples)
        *launches = 2;
    return SDSP_HIP_OK;
}

int sdsp_hip_cic_interp_plan_get_info(const sdsp_hip_cic_interp_plan *p, sdsp_hip_cic_interp_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->order = p->order;
    info->up = p->up;
    info->delay = p->delay;
    info->hist = p->hist;
    info->in_bits = p->in_bits;
    info->growth = p->growth;
    info->reg_bits = p->reg_bits;
    info->chunk = cic_interp_chunk();
    info->segment = p->segment;
    info->in_type = p->in_type;
    info->input_kind = p->kind;
    info->out_kind = p->out_kind;
    info->device = p->device;
    info->scale = p->scale;
    std::strncpy(info->kernel, cic_interp_kernel_for(p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_cic_interp_process(sdsp_hip_cic_interp_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride,
                                uint64_t channels, uint64_t samples, void *state, void *stream)
{
    uint64_t outs = 0;
    if (int rc = cic_interp_check(p, in, in_stride, out, out_stride, channels, samples, &outs))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    const uint64_t ies = cic_interp_in_esize(p), oes = cic_interp_out_esize(p);
    if (int rc = check_out_of_place(in, ((channels - 1) * in_stride + samples) * ies, ies, out, ((channels - 1) * out_stride + outs) * oes,
                                    oes, state, ies, "in and out ranges overlap (the interpolator runs out of place)"))
        return rc;
    if (int rc = use_device(p->device))
        return rc;
    return cic_interp_run(p, in, in_stride, out, out_stride, channels, samples, state, reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_cic_interp_process_host(sdsp_hip_cic_interp_plan *p, const void *host_in, uint64_t in_stride, void *host_out,
                                     uint64_t out_stride, uint64_t channels, uint64_t samples, void *host_state)
{
    uint64_t outs = 0;
    if (int rc = cic_interp_check(p, host_in, in_stride, host_out, out_stride, channels, samples, &outs))
        return rc;
    if (channels == 0 || samples == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const size_t in_bytes = ((channels - 1) * in_stride + samples) * cic_interp_in_esize(p);
    const size_t out_bytes = ((channels - 1) * out_stride + outs) * cic_interp_out_esize(p);
    uint64_t state_bytes = 0;
    sdsp_hip_cic_interp_state_bytes(p, channels, &state_bytes);
    host_stage st("cic_interp", { { host_in, in_bytes, false }, { host_out, out_bytes, true }, { host_state, state_bytes, true } });
    int rc = st.in();
    if (!rc)
        rc = cic_interp_run(p, st.dev[0], in_stride, st.dev[1], out_stride, channels, samples, st.dev[2], nullptr);
    return st.out(rc);
}
// ------------------------------------------------------------------ time-delay beamformer banks (beam.hip)

namespace
{
uint64_t beam_esize(const sdsp_hip_beam_plan *p)
{
    return p->kind == SDSP_HIP_BEAM_COMPLEX ? esize(p->precision) : real_size(p->precision);
}

// argument checks shared by process and process_host (device pointers or not)
int beam_check(const sdsp_hip_beam_plan *p, const void *in, uint64_t in_stride, const void *out, uint64_t out_stride, uint64_t samples)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (samples >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "samples must be below 2^31");
    if (samples == 0)
        return SDSP_HIP_OK;
    if (!in || !out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in or out is null");
    if ((static_cast<uint64_t>(p->groups) * p->sensors > 1 && in_stride < samples) ||
        (static_cast<uint64_t>(p->groups) * p->beams > 1 && out_stride < samples))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_stride and out_stride must be >= samples");
    return SDSP_HIP_OK;
}

int beam_run(sdsp_hip_beam_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t samples, void *state,
             hipStream_t stream)
{
    beam_args a{};
    a.in = in;
    a.out = out;
    a.state = p->hist ? state : nullptr;
    a.g = p->g;
    a.table = p->table;
    a.lay = p->lay;
    a.samples = samples;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.taps = p->taps;
    a.hist = p->hist;
    a.sensors = p->sensors;
    a.beams = p->beams;
    a.groups = p->groups;
    a.complex_in = p->kind == SDSP_HIP_BEAM_COMPLEX;
    if (int rc = launch_beam(p->precision, a, p->variant, stream))
        return rc;
    // behind the beam kernel: it reads the old history
    return carry_history(p->precision, static_cast<uint32_t>(beam_esize(p)), in, in_stride, state,
                         static_cast<uint64_t>(p->groups) * p->sensors, samples, p->hist, stream, "beam");
}
} // namespace

int sdsp_hip_beam_plan_create(sdsp_hip_beam_plan **out, uint32_t sensors, uint32_t beams, uint32_t groups, uint32_t taps,
                              uint32_t n_entries, const sdsp_hip_beam_entry *entries, const double *g, int kind, int precision,
                              int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (sensors == 0 || sensors > SDSP_HIP_BEAM_MAX_ROWS || beams == 0 || beams > SDSP_HIP_BEAM_MAX_ROWS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "sensors and beams must be in [1, SDSP_HIP_BEAM_MAX_ROWS]");
    if (groups == 0 || static_cast<uint64_t>(groups) * sensors > 0x7fffffffull || static_cast<uint64_t>(groups) * beams > 0x7fffffffull)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "groups must be >= 1 with groups * sensors and groups * beams below 2^31");
    if (taps == 0 || taps > SDSP_HIP_BEAM_MAX_TAPS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps must be in [1, SDSP_HIP_BEAM_MAX_TAPS]");
    if (n_entries > SDSP_HIP_BEAM_MAX_ENTRIES)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "the entry count must be in [0, SDSP_HIP_BEAM_MAX_ENTRIES]");
    if (n_entries && (!entries || !g))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "entry or tap pointer is null");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (kind != SDSP_HIP_BEAM_REAL && kind != SDSP_HIP_BEAM_COMPLEX)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "kind must be SDSP_HIP_BEAM_REAL or SDSP_HIP_BEAM_COMPLEX");
    uint32_t max_delay = 0;
    for (uint32_t i = 0; i < n_entries; i++) {
        const sdsp_hip_beam_entry &e = entries[i];
        if (e.beam >= beams || e.sensor >= sensors)
            return fail(SDSP_HIP_ERR_INVALID_ARG, "an entry names a beam or a sensor the plan does not have");
        if (e.delay > SDSP_HIP_BEAM_MAX_DELAY)
            return fail(SDSP_HIP_ERR_INVALID_SIZE, "a delay must be in [0, SDSP_HIP_BEAM_MAX_DELAY]");
        if (i && (e.beam < entries[i - 1].beam || (e.beam == entries[i - 1].beam && e.sensor <= entries[i - 1].sensor)))
            return fail(SDSP_HIP_ERR_INVALID_ARG, "entries must be sorted by beam, and by strictly ascending sensor within a beam");
        max_delay = e.delay > max_delay ? e.delay : max_delay;
    }
    if (int rc = use_device(device))
        return rc;
    const bool cplx = kind == SDSP_HIP_BEAM_COMPLEX;
    if (int rc = beam_prepare(precision, cplx))
        return rc;
    // the host tables grow with the beams and the entries: running out of host memory for them is an error code, not an exception
    std::vector<uint32_t> table;
    beam_layout lay;
    try {
        beam_build_table(precision, cplx, taps, beams, n_entries, entries, table, lay);
    } catch (const std::bad_alloc &) {
        return fail(SDSP_HIP_ERR_NOMEM, "beam plan: out of host memory for the entry tables");
    }
    auto *p = new sdsp_hip_beam_plan();
    p->sensors = sensors;
    p->beams = beams;
    p->groups = groups;
    p->taps = taps;
    p->entries = n_entries;
    p->max_delay = max_delay;
    p->hist = max_delay + taps - 1;
    p->kind = kind;
    p->precision = precision;
    p->device = device;
    p->lay = lay;
    const size_t ng = static_cast<size_t>(n_entries) * taps * (cplx ? 2 : 1);
    const double none = 0.0; // a plan without entries still owns a (one-value) tap table
    hipError_t e = upload_reals(ng ? g : &none, ng ? ng : 1, precision, &p->g);
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void **>(&p->table), table.size() * sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipMemcpy(p->table, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        sdsp_hip_beam_plan_destroy(p);
        return plan_fail(e, "beam");
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_beam_plan_destroy(sdsp_hip_beam_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK) {
        (void)hipFree(p->g);
        (void)hipFree(p->table);
    }
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_beam_state_bytes(const sdsp_hip_beam_plan *p, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = static_cast<uint64_t>(p->hist) * p->groups * p->sensors * beam_esize(p);
    return SDSP_HIP_OK;
}

int sdsp_hip_beam_plan_set_variant(sdsp_hip_beam_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_beam_plan_launches(const sdsp_hip_beam_plan *p, uint64_t samples, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = samples ? 1 + (p->hist ? 1 : 0) : 0;
    return SDSP_HIP_OK;
}

int sdsp_hip_beam_plan_get_info(const sdsp_hip_beam_plan *p, sdsp_hip_beam_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->sensors = p->sensors;
    info->beams = p->beams;
    info->groups = p->groups;
    info->taps = p->taps;
    info->entries = p->entries;
    info->max_delay = p->max_delay;
    info->hist = p->hist;
    info->block_out = beam_block_out();
    info->chunks = p->lay.chunks;
    info->max_spread = p->lay.max_spread;
    info->lds_line_bytes = p->lay.lds_line_bytes;
    info->kind = p->kind;
    info->precision = p->precision;
    info->device = p->device;
    info->variant = p->variant;
    std::strncpy(info->kernel, beam_kernel_for(p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_beam_process(sdsp_hip_beam_plan *p, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t samples,
                          void *state, void *stream)
{
    if (int rc = beam_check(p, in, in_stride, out, out_stride, samples))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    const uint64_t es = beam_esize(p), rows_in = static_cast<uint64_t>(p->groups) * p->sensors,
                   rows_out = static_cast<uint64_t>(p->groups) * p->beams;
    if (int rc = check_out_of_place(in, ((rows_in - 1) * in_stride + samples) * es, es, out, ((rows_out - 1) * out_stride + samples) * es, es,
                                    state, es, "in and out ranges overlap (the beamformer runs out of place)"))
        return rc;
    if (int rc = use_device(p->device))
        return rc;
    return beam_run(p, in, in_stride, out, out_stride, samples, state, reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_beam_process_host(sdsp_hip_beam_plan *p, const void *host_in, uint64_t in_stride, void *host_out, uint64_t out_stride,
                               uint64_t samples, void *host_state)
{
    if (int rc = beam_check(p, host_in, in_stride, host_out, out_stride, samples))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const uint64_t es = beam_esize(p);
    const size_t in_bytes = ((static_cast<uint64_t>(p->groups) * p->sensors - 1) * in_stride + samples) * es;
    const size_t out_bytes = ((static_cast<uint64_t>(p->groups) * p->beams - 1) * out_stride + samples) * es;
    uint64_t state_bytes = 0;
    sdsp_hip_beam_state_bytes(p, &state_bytes);
    const bool with_state = host_state && state_bytes;
    host_stage st("beam", { { host_in, in_bytes, false }, { host_out, out_bytes, true },
                        { with_state ? host_state : nullptr, state_bytes, true } });
    int rc = st.in();
    if (!rc)
        rc = beam_run(p, st.dev[0], in_stride, st.dev[1], out_stride, samples, st.dev[2], nullptr);
    return st.out(rc);
}
// ------------------------------------------------------------------ LMS / NLMS adaptive filter banks (lms.hip)

namespace
{
uint64_t lms_esize(const sdsp_hip_lms_plan *p) { return p->kind == SDSP_HIP_LMS_COMPLEX ? esize(p->precision) : real_size(p->precision); }

double lms_round(const sdsp_hip_lms_plan *p, double v) { return p->precision == SDSP_HIP_F64 ? v : static_cast<double>(static_cast<float>(v)); }

// argument checks shared by process and process_host (device pointers or not)
int lms_check(const sdsp_hip_lms_plan *p, const void *x, uint64_t x_stride, const void *d, uint64_t d_stride, const void *y,
              uint64_t y_stride, const void *e, uint64_t e_stride, uint64_t samples, double mu)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (samples >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "samples must be below 2^31");
    if (!std::isfinite(mu) || !std::isfinite(lms_round(p, mu)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "mu must be finite in the plan precision");
    if (samples == 0)
        return SDSP_HIP_OK;
    if (!x || !d)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "x or d is null");
    if (p->channels > 1 && (x_stride < samples || d_stride < samples || (y && y_stride < samples) || (e && e_stride < samples)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "every stride must be >= samples");
    return SDSP_HIP_OK;
}

int lms_run(sdsp_hip_lms_plan *p, const void *x, uint64_t x_stride, const void *d, uint64_t d_stride, void *y, uint64_t y_stride, void *e,
            uint64_t e_stride, uint64_t samples, double mu, void *state, hipStream_t stream)
{
    const uint64_t es = lms_esize(p);
    lms_args a{};
    a.x = x;
    a.d = d;
    a.y = y;
    a.e = e;
    a.w = state;
    a.hist = state && p->taps > 1 ? static_cast<unsigned char *>(state) + p->channels * p->taps * es : nullptr;
    a.channels = p->channels;
    a.samples = samples;
    a.x_stride = x_stride;
    a.d_stride = d_stride;
    a.y_stride = y_stride;
    a.e_stride = e_stride;
    a.taps = p->taps;
    a.complex_in = p->kind == SDSP_HIP_LMS_COMPLEX;
    a.nlms = p->mode == SDSP_HIP_LMS_NLMS;
    a.mu = lms_round(p, mu);
    a.eps = p->eps;
    if (p->variant == 1 && !state) { // the plain kernel keeps its weights in memory: zero rows of the plan's
        if (!p->scratch_w)
            return fail(SDSP_HIP_ERR_INVALID_ARG, "lms: variant 1 without its scratch rows");
        HIP_TRY(hipMemsetAsync(p->scratch_w, 0, p->channels * p->taps * es, stream));
        a.w = p->scratch_w;
    }
    if (int rc = launch_lms(p->precision, a, p->variant, stream))
        return rc;
    // behind the kernel: it reads the old history
    return carry_history(p->precision, static_cast<uint32_t>(es), x, x_stride, const_cast<void *>(a.hist), p->channels, samples,
                         p->taps - 1, stream, "lms");
}
} // namespace

int sdsp_hip_lms_plan_create(sdsp_hip_lms_plan **out, uint64_t channels, uint32_t taps, int kind, int precision, int mode, double eps,
                             int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (channels == 0 || channels > 0x7fffffffull)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "channels must be in [1, 2^31)");
    if (taps == 0 || taps > SDSP_HIP_LMS_MAX_TAPS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps must be in [1, SDSP_HIP_LMS_MAX_TAPS]");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (kind != SDSP_HIP_LMS_REAL && kind != SDSP_HIP_LMS_COMPLEX)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "kind must be SDSP_HIP_LMS_REAL or SDSP_HIP_LMS_COMPLEX");
    if (mode != SDSP_HIP_LMS_LMS && mode != SDSP_HIP_LMS_NLMS)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "mode must be SDSP_HIP_LMS_LMS or SDSP_HIP_LMS_NLMS");
    if (precision == SDSP_HIP_F64 && kind == SDSP_HIP_LMS_COMPLEX && taps > SDSP_HIP_LMS_MAX_TAPS_F64_COMPLEX)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps must be in [1, SDSP_HIP_LMS_MAX_TAPS_F64_COMPLEX] for F64 COMPLEX");
    const double eps_r = precision == SDSP_HIP_F64 ? eps : static_cast<double>(static_cast<float>(eps));
    if (mode == SDSP_HIP_LMS_NLMS && !(std::isfinite(eps_r) && eps_r > 0.0))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "eps must be finite and > 0 in the plan precision for NLMS");
    if (int rc = use_device(device))
        return rc;
    auto *p = new sdsp_hip_lms_plan();
    p->channels = channels;
    p->taps = taps;
    p->kind = kind;
    p->precision = precision;
    p->mode = mode;
    p->device = device;
    p->eps = mode == SDSP_HIP_LMS_NLMS ? eps_r : 0.0;
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_lms_plan_destroy(sdsp_hip_lms_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (p->scratch_w && use_device(p->device) == SDSP_HIP_OK)
        (void)hipFree(p->scratch_w);
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_lms_state_bytes(const sdsp_hip_lms_plan *p, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = p->channels * (2ull * p->taps - 1) * lms_esize(p);
    return SDSP_HIP_OK;
}

int sdsp_hip_lms_plan_set_variant(sdsp_hip_lms_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    if (variant == 1 && !p->scratch_w) {
        if (int rc = use_device(p->device))
            return rc;
        const hipError_t e = hipMalloc(&p->scratch_w, p->channels * p->taps * lms_esize(p));
        if (e != hipSuccess) {
            p->scratch_w = nullptr;
            return plan_fail(e, "lms");
        }
    }
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_lms_plan_launches(const sdsp_hip_lms_plan *p, uint64_t samples, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = samples ? 1 + (p->taps > 1 ? 1 : 0) : 0;
    return SDSP_HIP_OK;
}

int sdsp_hip_lms_plan_get_info(const sdsp_hip_lms_plan *p, sdsp_hip_lms_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    const int cplx = p->kind == SDSP_HIP_LMS_COMPLEX;
    info->channels = p->channels;
    info->taps = p->taps;
    info->block = lms_block(p->precision, cplx, p->taps);
    info->lds_bytes = lms_lds_bytes(p->precision, cplx, p->taps);
    info->eps = p->eps;
    info->kind = p->kind;
    info->precision = p->precision;
    info->mode = p->mode;
    info->device = p->device;
    info->variant = p->variant;
    std::strncpy(info->kernel, lms_kernel_for(p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_lms_process(sdsp_hip_lms_plan *p, const void *x, uint64_t x_stride, const void *d, uint64_t d_stride, void *y,
                         uint64_t y_stride, void *e, uint64_t e_stride, uint64_t samples, double mu, void *state, void *stream)
{
    if (int rc = lms_check(p, x, x_stride, d, d_stride, y, y_stride, e, e_stride, samples, mu))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    const uint64_t es = lms_esize(p);
    auto span = [&](uint64_t stride) { return ((p->channels - 1) * stride + samples) * es; };
    const void *ins[2] = { x, d };
    const uint64_t in_bytes[2] = { span(x_stride), span(d_stride) };
    for (int i = 0; i < 2; i++)
        if (ranges_overlap(ins[i], in_bytes[i], y, span(y_stride)) || ranges_overlap(ins[i], in_bytes[i], e, span(e_stride)))
            return fail(SDSP_HIP_ERR_INVALID_ARG, "an output range overlaps an input range (the adaptive filter runs out of place)");
    if (ranges_overlap(y, span(y_stride), e, span(e_stride)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "the y and e ranges overlap");
    if (misaligned(x, es) || misaligned(d, es) || misaligned(y, es) || misaligned(e, es) || misaligned(state, es))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "x, d, y, e and state must be aligned to their element size");
    if (int rc = use_device(p->device))
        return rc;
    return lms_run(p, x, x_stride, d, d_stride, y, y_stride, e, e_stride, samples, mu, state, reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_lms_process_host(sdsp_hip_lms_plan *p, const void *host_x, uint64_t x_stride, const void *host_d, uint64_t d_stride,
                              void *host_y, uint64_t y_stride, void *host_e, uint64_t e_stride, uint64_t samples, double mu,
                              void *host_state)
{
    if (int rc = lms_check(p, host_x, x_stride, host_d, d_stride, host_y, y_stride, host_e, e_stride, samples, mu))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const uint64_t es = lms_esize(p);
    auto span = [&](uint64_t stride) { return static_cast<size_t>(((p->channels - 1) * stride + samples) * es); };
    uint64_t state_bytes = 0;
    sdsp_hip_lms_state_bytes(p, &state_bytes);
    host_stage st("lms", { { host_x, span(x_stride), false }, { host_d, span(d_stride), false }, { host_y, span(y_stride), true },
                       { host_e, span(e_stride), true }, { host_state, static_cast<size_t>(state_bytes), true } });
    int rc = st.in();
    if (!rc)
        rc = lms_run(p, st.dev[0], x_stride, st.dev[1], d_stride, st.dev[2], y_stride, st.dev[3], e_stride, samples, mu, st.dev[4],
                     nullptr);
    return st.out(rc);
}
// ------------------------------------------------------------------ rank-order filter banks (rank_filter.hip)

namespace
{
// argument checks shared by process and process_host (device pointers or not)
int rank_check(const sdsp_hip_rank_plan *p, const void *x, uint64_t x_stride, const void *y, uint64_t y_stride, uint64_t samples)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (samples >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "samples must be below 2^31");
    if (samples == 0)
        return SDSP_HIP_OK;
    if (!x || !y)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "x or y is null");
    if (p->channels > 1 && (x_stride < samples || y_stride < samples))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "every stride must be >= samples");
    return SDSP_HIP_OK;
}

uint32_t rank_run_for(const sdsp_hip_rank_plan *p, uint64_t samples)
{
    if (p->run)
        return static_cast<uint32_t>(p->run < samples ? p->run : samples);
    return rank_auto_run(p->precision, p->channels, samples, p->window);
}

int rank_run(sdsp_hip_rank_plan *p, const void *x, uint64_t x_stride, void *y, uint64_t y_stride, uint64_t samples, void *state,
             hipStream_t stream)
{
    rank_args a{};
    a.x = x;
    a.y = y;
    a.hist = p->window > 1 ? state : nullptr;
    a.channels = p->channels;
    a.samples = samples;
    a.x_stride = x_stride;
    a.y_stride = y_stride;
    a.window = p->window;
    a.rank = p->rank;
    a.run = rank_run_for(p, samples);
    if (p->variant == 0)
        p->last_run = a.run;
    if (int rc = launch_rank(p->precision, a, p->variant, stream))
        return rc;
    // behind the kernel: it reads the old history
    return carry_history(p->precision, static_cast<uint32_t>(real_size(p->precision)), x, x_stride, const_cast<void *>(a.hist), p->channels,
                         samples, p->window - 1, stream, "rank");
}
} // namespace

int sdsp_hip_rank_plan_create(sdsp_hip_rank_plan **out, uint64_t channels, uint32_t window, uint32_t rank, int precision, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (channels == 0 || channels > 0x7fffffffull)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "channels must be in [1, 2^31)");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (window == 0 || window > (precision == SDSP_HIP_F64 ? SDSP_HIP_RANK_MAX_WINDOW_F64 : SDSP_HIP_RANK_MAX_WINDOW))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "window must be in [1, SDSP_HIP_RANK_MAX_WINDOW] (SDSP_HIP_RANK_MAX_WINDOW_F64 for F64)");
    if (rank >= window)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "rank must be below the window");
    if (int rc = use_device(device))
        return rc;
    auto *p = new sdsp_hip_rank_plan();
    p->channels = channels;
    p->window = window;
    p->rank = rank;
    p->precision = precision;
    p->device = device;
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_rank_plan_destroy(sdsp_hip_rank_plan *p)
{
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_rank_state_bytes(const sdsp_hip_rank_plan *p, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = p->channels * (p->window - 1ull) * real_size(p->precision);
    return SDSP_HIP_OK;
}

int sdsp_hip_rank_plan_set_variant(sdsp_hip_rank_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_rank_plan_set_run(sdsp_hip_rank_plan *p, uint64_t run)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (run >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "run must be below 2^31");
    p->run = static_cast<uint32_t>(run);
    return SDSP_HIP_OK;
}

int sdsp_hip_rank_plan_launches(const sdsp_hip_rank_plan *p, uint64_t samples, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = samples ? 1 + (p->window > 1 ? 1 : 0) : 0;
    return SDSP_HIP_OK;
}

int sdsp_hip_rank_plan_get_info(const sdsp_hip_rank_plan *p, sdsp_hip_rank_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->channels = p->channels;
    info->window = p->window;
    info->rank = p->rank;
    info->padded = rank_padded(p->window);
    info->out_index = p->rank;
    info->run = p->run;
    info->last_run = p->last_run;
    info->block = rank_block(p->precision);
    info->lds_bytes = rank_lds_bytes(p->precision);
    info->departing = SDSP_HIP_RANK_DEPART_TILE;
    info->precision = p->precision;
    info->device = p->device;
    info->variant = p->variant;
    std::strncpy(info->kernel, rank_kernel_for(p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_rank_process(sdsp_hip_rank_plan *p, const void *x, uint64_t x_stride, void *y, uint64_t y_stride, uint64_t samples,
                          void *state, void *stream)
{
    if (int rc = rank_check(p, x, x_stride, y, y_stride, samples))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    const uint64_t es = real_size(p->precision);
    auto span = [&](uint64_t stride) { return ((p->channels - 1) * stride + samples) * es; };
    if (ranges_overlap(x, span(x_stride), y, span(y_stride)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "the y range overlaps the x range (the rank filter runs out of place)");
    if (misaligned(x, es) || misaligned(y, es) || misaligned(state, es))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "x, y and state must be aligned to their element size");
    if (int rc = use_device(p->device))
        return rc;
    return rank_run(p, x, x_stride, y, y_stride, samples, state, reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_rank_process_host(sdsp_hip_rank_plan *p, const void *host_x, uint64_t x_stride, void *host_y, uint64_t y_stride,
                               uint64_t samples, void *host_state)
{
    if (int rc = rank_check(p, host_x, x_stride, host_y, y_stride, samples))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const uint64_t es = real_size(p->precision);
    auto span = [&](uint64_t stride) { return static_cast<size_t>(((p->channels - 1) * stride + samples) * es); };
    uint64_t state_bytes = 0;
    sdsp_hip_rank_state_bytes(p, &state_bytes);
    host_stage st("rank", { { host_x, span(x_stride), false }, { host_y, span(y_stride), true },
                        { host_state, static_cast<size_t>(state_bytes), true } });
    int rc = st.in();
    if (!rc)
        rc = rank_run(p, st.dev[0], x_stride, st.dev[1], y_stride, samples, st.dev[2], nullptr);
    return st.out(rc);
}
// ------------------------------------------------------------------ CFAR detector banks (cfar.hip)

namespace
{
uint32_t cfar_hist(const sdsp_hip_cfar_plan *p) { return 2 * (p->train + p->guard); }
uint64_t cfar_in_esize(const sdsp_hip_cfar_plan *p) { return real_size(p->precision) * (p->input == SDSP_HIP_CFAR_IQ ? 2u : 1u); }

// c of the mode from alpha: a host double rounded once to the precision
double cfar_scale(int mode, uint32_t train, double alpha, int precision)
{
    const double c = mode == SDSP_HIP_CFAR_CA ? alpha / (2.0 * train) : mode == SDSP_HIP_CFAR_OS ? alpha : alpha / train;
    return precision == SDSP_HIP_F64 ? c : static_cast<double>(static_cast<float>(c));
}

// argument checks shared by process and process_host (device pointers or not)
int cfar_check(const sdsp_hip_cfar_plan *p, const void *x, uint64_t x_stride, const void *thr, uint64_t thr_stride, const void *det,
               uint64_t det_stride, uint64_t samples)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (samples >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "samples must be below 2^31");
    if (samples == 0)
        return SDSP_HIP_OK;
    if (!thr && !det)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "thr and det are both null: nothing to write");
    if (!x)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "x is null");
    if (p->channels > 1 && (x_stride < samples || (thr && thr_stride < samples) || (det && det_stride < samples)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "every stride must be >= samples");
    return SDSP_HIP_OK;
}

uint32_t cfar_run_for(const sdsp_hip_cfar_plan *p, uint64_t samples)
{
    uint64_t run = p->run ? p->run : cfar_auto_run(p->precision, p->mode, p->channels, samples, p->train, p->guard);
    if (p->mode != SDSP_HIP_CFAR_OS && run > cfar_block(p->precision, p->mode))
        run = cfar_block(p->precision, p->mode);
    return static_cast<uint32_t>(run < samples ? run : samples);
}

int cfar_run(sdsp_hip_cfar_plan *p, const void *x, uint64_t x_stride, void *thr, uint64_t thr_stride, void *det, uint64_t det_stride,
             uint64_t samples, void *state, hipStream_t stream)
{
    cfar_args a{};
    a.x = x;
    a.thr = thr;
    a.det = det;
    a.hist = state;
    a.channels = p->channels;
    a.samples = samples;
    a.x_stride = x_stride;
    a.thr_stride = thr_stride;
    a.det_stride = det_stride;
    a.train = p->train;
    a.guard = p->guard;
    a.rank = p->rank;
    a.mode = p->mode;
    a.iq = p->input == SDSP_HIP_CFAR_IQ;
    a.scale = p->scale;
    a.run = cfar_run_for(p, samples);
    if (p->variant == 0)
        p->last_run = a.run;
    if (int rc = launch_cfar(p->precision, a, p->variant, stream))
        return rc;
    // behind the kernel: it reads the old history
    return carry_history(p->precision, static_cast<uint32_t>(cfar_in_esize(p)), x, x_stride, state, p->channels, samples, cfar_hist(p),
                         stream, "cfar");
}
} // namespace

int sdsp_hip_cfar_plan_create(sdsp_hip_cfar_plan **out, uint64_t channels, const sdsp_hip_cfar_desc *d, int precision, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (!d)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "descriptor is null");
    if (channels == 0 || channels > 0x7fffffffull)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "channels must be in [1, 2^31)");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (d->mode < SDSP_HIP_CFAR_CA || d->mode > SDSP_HIP_CFAR_OS)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "mode must be SDSP_HIP_CFAR_CA, GO, SO or OS");
    if (d->input != SDSP_HIP_CFAR_POWER && d->input != SDSP_HIP_CFAR_IQ)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "input must be SDSP_HIP_CFAR_POWER or SDSP_HIP_CFAR_IQ");
    if (d->train == 0 || d->train > SDSP_HIP_CFAR_MAX_TRAIN)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "train must be in [1, SDSP_HIP_CFAR_MAX_TRAIN]");
    if (d->guard > SDSP_HIP_CFAR_MAX_GUARD)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "guard must be in [0, SDSP_HIP_CFAR_MAX_GUARD]");
    if (d->mode == SDSP_HIP_CFAR_OS) {
        if (2 * d->train > (precision == SDSP_HIP_F64 ? SDSP_HIP_RANK_MAX_WINDOW_F64 : SDSP_HIP_RANK_MAX_WINDOW))
            return fail(SDSP_HIP_ERR_INVALID_SIZE,
                        "OS: 2 train must be at most SDSP_HIP_RANK_MAX_WINDOW (SDSP_HIP_RANK_MAX_WINDOW_F64 for F64)");
        if (d->rank >= 2 * d->train)
            return fail(SDSP_HIP_ERR_INVALID_ARG, "rank must be below 2 train");
    }
    if (int rc = use_device(device))
        return rc;
    auto *p = new sdsp_hip_cfar_plan();
    p->channels = channels;
    p->train = d->train;
    p->guard = d->guard;
    p->mode = d->mode;
    p->rank = d->mode == SDSP_HIP_CFAR_OS ? d->rank : 0;
    p->input = d->input;
    p->alpha = d->alpha;
    p->scale = cfar_scale(d->mode, d->train, d->alpha, precision);
    p->precision = precision;
    p->device = device;
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_cfar_plan_destroy(sdsp_hip_cfar_plan *p)
{
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_cfar_state_bytes(const sdsp_hip_cfar_plan *p, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = p->channels * cfar_hist(p) * cfar_in_esize(p);
    return SDSP_HIP_OK;
}

int sdsp_hip_cfar_plan_set_alpha(sdsp_hip_cfar_plan *p, double alpha)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    p->alpha = alpha;
    p->scale = cfar_scale(p->mode, p->train, alpha, p->precision);
    return SDSP_HIP_OK;
}

int sdsp_hip_cfar_plan_set_variant(sdsp_hip_cfar_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_cfar_plan_set_run(sdsp_hip_cfar_plan *p, uint64_t run)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (run >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "run must be below 2^31");
    p->run = static_cast<uint32_t>(run);
    return SDSP_HIP_OK;
}

int sdsp_hip_cfar_plan_launches(const sdsp_hip_cfar_plan *p, uint64_t samples, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = samples ? 2 : 0; // W - 1 >= 2: there is always a history to carry
    return SDSP_HIP_OK;
}

int sdsp_hip_cfar_plan_get_info(const sdsp_hip_cfar_plan *p, sdsp_hip_cfar_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->channels = p->channels;
    info->train = p->train;
    info->guard = p->guard;
    info->half = p->train + p->guard;
    info->window = 2 * info->half + 1;
    info->lag_shift = p->train + 2 * p->guard + 1;
    info->rank = p->rank;
    info->padded = p->mode == SDSP_HIP_CFAR_OS ? cfar_padded(2 * p->train) : 0;
    info->run = p->run;
    info->last_run = p->last_run;
    info->block = cfar_block(p->precision, p->mode);
    info->lds_bytes = cfar_lds_bytes(p->precision, p->mode);
    info->alpha = p->alpha;
    info->scale = p->scale;
    info->mode = p->mode;
    info->input = p->input;
    info->precision = p->precision;
    info->device = p->device;
    info->variant = p->variant;
    std::strncpy(info->kernel, cfar_kernel_for(p->variant, p->mode), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_cfar_process(sdsp_hip_cfar_plan *p, const void *x, uint64_t x_stride, void *thr, uint64_t thr_stride, uint8_t *det,
                          uint64_t det_stride, uint64_t samples, void *state, void *stream)
{
    if (int rc = cfar_check(p, x, x_stride, thr, thr_stride, det, det_stride, samples))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    const uint64_t es = real_size(p->precision), xs = cfar_in_esize(p);
    auto span = [&](uint64_t stride, uint64_t bytes) { return ((p->channels - 1) * stride + samples) * bytes; };
    if (ranges_overlap(x, span(x_stride, xs), thr, span(thr_stride, es)) || ranges_overlap(x, span(x_stride, xs), det, span(det_stride, 1)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "an output range overlaps the x range (the detector runs out of place)");
    if (ranges_overlap(thr, span(thr_stride, es), det, span(det_stride, 1)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "the thr and det ranges overlap");
    if (misaligned(x, xs) || misaligned(thr, es) || misaligned(state, xs))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "x, thr and state must be aligned to their element size");
    if (int rc = use_device(p->device))
        return rc;
    return cfar_run(p, x, x_stride, thr, thr_stride, det, det_stride, samples, state, reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_cfar_process_host(sdsp_hip_cfar_plan *p, const void *host_x, uint64_t x_stride, void *host_thr, uint64_t thr_stride,
                               uint8_t *host_det, uint64_t det_stride, uint64_t samples, void *host_state)
{
    if (int rc = cfar_check(p, host_x, x_stride, host_thr, thr_stride, host_det, det_stride, samples))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const uint64_t es = real_size(p->precision), xs = cfar_in_esize(p);
    auto span = [&](uint64_t stride, uint64_t bytes) { return static_cast<size_t>(((p->channels - 1) * stride + samples) * bytes); };
    uint64_t state_bytes = 0;
    sdsp_hip_cfar_state_bytes(p, &state_bytes);
    host_stage st("cfar", { { host_x, span(x_stride, xs), false }, { host_thr, span(thr_stride, es), true },
                        { host_det, span(det_stride, 1), true }, { host_state, static_cast<size_t>(state_bytes), true } });
    int rc = st.in();
    if (!rc)
        rc = cfar_run(p, st.dev[0], x_stride, st.dev[1], thr_stride, st.dev[2], det_stride, samples, st.dev[3], nullptr);
    return st.out(rc);
}
// ------------------------------------------------------------------ carrier-recovery PLL / Costas loop banks (pll.hip)

namespace
{
double pll_round(const sdsp_hip_pll_plan *p, double v) { return p->precision == SDSP_HIP_F64 ? v : static_cast<double>(static_cast<float>(v)); }

uint64_t pll_state_size(const sdsp_hip_pll_plan *p) { return p->channels * (real_size(p->precision) + sizeof(uint32_t)); }

// argument checks shared by process and process_host (device pointers or not)
int pll_check(const sdsp_hip_pll_plan *p, const void *x, uint64_t x_stride, const void *y, uint64_t y_stride, const void *err,
              uint64_t err_stride, const void *freq, uint64_t freq_stride, uint64_t samples, double alpha, double beta)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (samples >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "samples must be below 2^31");
    if (!std::isfinite(alpha) || !std::isfinite(beta) || !std::isfinite(pll_round(p, alpha)) || !std::isfinite(pll_round(p, beta)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "alpha and beta must be finite in the plan precision");
    if (samples == 0)
        return SDSP_HIP_OK;
    if (!x)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "x is null");
    if (p->channels > 1 &&
        (x_stride < samples || (y && y_stride < samples) || (err && err_stride < samples) || (freq && freq_stride < samples)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "every stride must be >= samples");
    return SDSP_HIP_OK;
}

int pll_run(sdsp_hip_pll_plan *p, const void *x, uint64_t x_stride, void *y, uint64_t y_stride, void *err, uint64_t err_stride, void *freq,
            uint64_t freq_stride, uint64_t samples, double alpha, double beta, void *state, hipStream_t stream)
{
    if (p->variant == 1 && !state) { // the plain kernel keeps its state in memory: a zeroed buffer of the plan's
        if (!p->scratch)
            return fail(SDSP_HIP_ERR_INVALID_ARG, "pll: variant 1 without its scratch state");
        HIP_TRY(hipMemsetAsync(p->scratch, 0, pll_state_size(p), stream));
        state = p->scratch;
    }
    pll_args a{};
    a.x = x;
    a.y = y;
    a.err = err;
    a.freq = freq;
    a.integ = state;
    a.theta = state ? reinterpret_cast<uint32_t *>(static_cast<unsigned char *>(state) + p->channels * real_size(p->precision)) : nullptr;
    a.fcw0 = p->fcw0;
    a.osc = p->osc;
    a.channels = p->channels;
    a.samples = samples;
    a.x_stride = x_stride;
    a.y_stride = y_stride;
    a.err_stride = err_stride;
    a.freq_stride = freq_stride;
    a.mode = p->mode;
    a.alpha = pll_round(p, alpha);
    a.beta = pll_round(p, beta);
    a.max_dev = p->max_dev;
    return launch_pll(p->precision, a, p->variant, stream);
}
} // namespace

int sdsp_hip_pll_plan_create(sdsp_hip_pll_plan **out, uint64_t channels, int precision, int mode, const uint32_t *fcw0, uint64_t n_fcw0,
                             double max_dev, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (channels == 0 || channels > 0x7fffffffull)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "channels must be in [1, 2^31)");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (mode != SDSP_HIP_PLL_CROSS && mode != SDSP_HIP_PLL_BPSK && mode != SDSP_HIP_PLL_QPSK)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "mode must be SDSP_HIP_PLL_CROSS, SDSP_HIP_PLL_BPSK or SDSP_HIP_PLL_QPSK");
    if (!fcw0 || (n_fcw0 != 1 && n_fcw0 != channels))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "fcw0 must hold one word or one word per channel");
    const double dev_r = precision == SDSP_HIP_F64 ? max_dev : static_cast<double>(static_cast<float>(max_dev));
    if (!(dev_r > 0.0 && dev_r <= 0.5)) // NaN included
        return fail(SDSP_HIP_ERR_INVALID_ARG, "max_dev must be in (0, 0.5] in the plan precision");
    if (int rc = use_device(device))
        return rc;
    std::vector<uint32_t> words;
    std::vector<double> osc;
    try {
        words.resize(static_cast<size_t>(channels));
        osc.resize(4 * 2048);
    } catch (const std::bad_alloc &) {
        return fail(SDSP_HIP_ERR_NOMEM, "pll plan: out of host memory for the frequency words");
    }
    for (uint64_t c = 0; c < channels; c++)
        words[static_cast<size_t>(c)] = fcw0[n_fcw0 == 1 ? 0 : c];
    sdsp_hip_pll_oscillator(osc.data(), osc.data() + 2 * 2048);
    auto *p = new sdsp_hip_pll_plan();
    p->channels = channels;
    p->precision = precision;
    p->mode = mode;
    p->device = device;
    p->max_dev = dev_r;
    hipError_t e = upload_reals(osc.data(), osc.size(), precision, &p->osc);
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void **>(&p->fcw0), words.size() * sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipMemcpy(p->fcw0, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        sdsp_hip_pll_plan_destroy(p);
        return plan_fail(e, "pll");
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_pll_plan_destroy(sdsp_hip_pll_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK) {
        (void)hipFree(p->osc);
        (void)hipFree(p->fcw0);
        (void)hipFree(p->scratch);
    }
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_pll_state_bytes(const sdsp_hip_pll_plan *p, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = pll_state_size(p);
    return SDSP_HIP_OK;
}

int sdsp_hip_pll_plan_set_variant(sdsp_hip_pll_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    if (variant == 1 && !p->scratch) {
        if (int rc = use_device(p->device))
            return rc;
        const hipError_t e = hipMalloc(&p->scratch, pll_state_size(p));
        if (e != hipSuccess) {
            p->scratch = nullptr;
            return plan_fail(e, "pll");
        }
    }
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_pll_plan_launches(const sdsp_hip_pll_plan *p, uint64_t samples, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = samples ? 1 : 0;
    return SDSP_HIP_OK;
}

int sdsp_hip_pll_plan_get_info(const sdsp_hip_pll_plan *p, sdsp_hip_pll_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->channels = p->channels;
    info->block = pll_block(p->precision);
    info->waves = pll_waves(p->precision);
    info->lds_bytes = pll_lds_bytes(p->precision);
    info->max_dev = p->max_dev;
    info->precision = p->precision;
    info->mode = p->mode;
    info->device = p->device;
    info->variant = p->variant;
    std::strncpy(info->kernel, pll_kernel_for(p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_pll_process(sdsp_hip_pll_plan *p, const void *x, uint64_t x_stride, void *y, uint64_t y_stride, void *err,
                         uint64_t err_stride, void *freq, uint64_t freq_stride, uint64_t samples, double alpha, double beta, void *state,
                         void *stream)
{
    if (int rc = pll_check(p, x, x_stride, y, y_stride, err, err_stride, freq, freq_stride, samples, alpha, beta))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    const uint64_t es = esize(p->precision), rs = real_size(p->precision);
    auto span = [&](uint64_t stride, uint64_t bytes) { return ((p->channels - 1) * stride + samples) * bytes; };
    const bool in_place = y == x && y_stride == x_stride;
    if (!in_place && ranges_overlap(x, span(x_stride, es), y, span(y_stride, es)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "y overlaps x without being x itself (the same pointer and stride)");
    const void *reals[2] = { err, freq };
    const uint64_t real_bytes[2] = { span(err_stride, rs), span(freq_stride, rs) };
    for (int i = 0; i < 2; i++)
        if (ranges_overlap(reals[i], real_bytes[i], x, span(x_stride, es)) || ranges_overlap(reals[i], real_bytes[i], y, span(y_stride, es)))
            return fail(SDSP_HIP_ERR_INVALID_ARG, "err or freq overlaps x or y");
    if (ranges_overlap(err, real_bytes[0], freq, real_bytes[1]))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "the err and freq ranges overlap");
    const uint64_t state_bytes = pll_state_size(p);
    if (ranges_overlap(state, state_bytes, x, span(x_stride, es)) || ranges_overlap(state, state_bytes, y, span(y_stride, es)) ||
        ranges_overlap(state, state_bytes, err, real_bytes[0]) || ranges_overlap(state, state_bytes, freq, real_bytes[1]))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "the state buffer overlaps x or an output");
    if (misaligned(x, es) || misaligned(y, es) || misaligned(err, rs) || misaligned(freq, rs) || misaligned(state, rs))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "x, y, err, freq and state must be aligned to their element size");
    if (int rc = use_device(p->device))
        return rc;
    return pll_run(p, x, x_stride, y, y_stride, err, err_stride, freq, freq_stride, samples, alpha, beta, state,
                   reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_pll_process_host(sdsp_hip_pll_plan *p, const void *host_x, uint64_t x_stride, void *host_y, uint64_t y_stride,
                              void *host_err, uint64_t err_stride, void *host_freq, uint64_t freq_stride, uint64_t samples, double alpha,
                              double beta, void *host_state)
{
    if (int rc = pll_check(p, host_x, x_stride, host_y, y_stride, host_err, err_stride, host_freq, freq_stride, samples, alpha, beta))
        return rc;
    if (samples == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const uint64_t es = esize(p->precision), rs = real_size(p->precision);
    auto span = [&](uint64_t stride, uint64_t bytes) { return static_cast<size_t>(((p->channels - 1) * stride + samples) * bytes); };
    host_stage st("pll", { { host_x, span(x_stride, es), false }, { host_y, span(y_stride, es), true }, { host_err, span(err_stride, rs), true },
                       { host_freq, span(freq_stride, rs), true }, { host_state, static_cast<size_t>(pll_state_size(p)), true } });
    int rc = st.in();
    if (!rc)
        rc = pll_run(p, st.dev[0], x_stride, st.dev[1], y_stride, st.dev[2], err_stride, st.dev[3], freq_stride, samples, alpha, beta,
                     st.dev[4], nullptr);
    return st.out(rc);
}
// ------------------------------------------------------------------ symbol-timing recovery banks (timing.hip)

namespace
{
double timing_round(const sdsp_hip_timing_plan *p, double v) { return p->precision == SDSP_HIP_F64 ? v : static_cast<double>(static_cast<float>(v)); }

// byte offsets of the state's arrays: one per field, each at the next multiple of 8 bytes, the history last
struct timing_layout {
    uint64_t time, ps, ym, integ, w, parity, hist, bytes;
};
timing_layout timing_state_layout(const sdsp_hip_timing_plan *p)
{
    const uint64_t ch = p->channels, rs = real_size(p->precision);
    auto up8 = [](uint64_t v) { return (v + 7) / 8 * 8; };
    timing_layout l{};
    uint64_t o = 0;
    l.time = o;
    o = up8(o + ch * 8);
    l.ps = o;
    o = up8(o + ch * 2 * rs);
    l.ym = o;
    o = up8(o + ch * 2 * rs);
    l.integ = o;
    o = up8(o + ch * rs);
    l.w = o;
    o = up8(o + ch * 4);
    l.parity = o;
    o = up8(o + ch * 4);
    l.hist = o;
    o = up8(o + ch * (p->taps - 1) * 2 * rs);
    l.bytes = o;
    return l;
}

uint64_t timing_cap(const sdsp_hip_timing_plan *p, uint64_t samples)
{
    uint64_t n = 0;
    (void)sdsp_hip_timing_max_out_for(p->step0, samples, &n); // both in range: checked at plan creation and by timing_check
    return n;
}

// argument checks shared by process and process_host (device pointers or not)
int timing_check(const sdsp_hip_timing_plan *p, const void *x, uint64_t x_stride, const void *y, uint64_t y_stride, const void *err,
                 uint64_t err_stride, const void *period, uint64_t period_stride, const void *counts, uint64_t samples, double alpha,
                 double beta)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (samples >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "samples must be below 2^31");
    if (!std::isfinite(alpha) || !std::isfinite(beta) || !std::isfinite(timing_round(p, alpha)) || !std::isfinite(timing_round(p, beta)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "alpha and beta must be finite in the plan precision");
    if (samples == 0)
        return SDSP_HIP_OK;
    if (!x || !y || !counts)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "x, y and counts must not be null");
    const uint64_t cap = timing_cap(p, samples);
    if (p->channels > 1 && (x_stride < samples || y_stride < cap || (err && err_stride < cap) || (period && period_stride < cap)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "x_stride must be >= samples and every output stride >= sdsp_hip_timing_max_out of samples");
    return SDSP_HIP_OK;
}

int timing_run(sdsp_hip_timing_plan *p, const void *x, uint64_t x_stride, void *y, uint64_t y_stride, void *err, uint64_t err_stride,
               void *period, uint64_t period_stride, uint32_t *counts, uint64_t samples, double alpha, double beta, void *state,
               hipStream_t stream)
{
    const timing_layout l = timing_state_layout(p);
    if (p->variant == 1 && !state) { // the plain kernel keeps its state in memory: a zeroed buffer of the plan's
        if (!p->scratch)
            return fail(SDSP_HIP_ERR_INVALID_ARG, "timing: variant 1 without its scratch state");
        HIP_TRY(hipMemsetAsync(p->scratch, 0, l.bytes, stream));
        state = p->scratch;
    }
    unsigned char *s = static_cast<unsigned char *>(state);
    timing_args a{};
    a.x = x;
    a.y = y;
    a.err = err;
    a.period = period;
    a.counts = counts;
    if (s) {
        a.time = reinterpret_cast<uint64_t *>(s + l.time);
        a.ps = s + l.ps;
        a.ym = s + l.ym;
        a.integ = s + l.integ;
        a.w = reinterpret_cast<int32_t *>(s + l.w);
        a.parity = reinterpret_cast<uint32_t *>(s + l.parity);
        a.hist = s + l.hist;
    }
    a.table = p->table;
    a.channels = p->channels;
    a.samples = samples;
    a.x_stride = x_stride;
    a.y_stride = y_stride;
    a.err_stride = err_stride;
    a.period_stride = period_stride;
    a.step0 = p->step0;
    a.cap = timing_cap(p, samples);
    a.phases = p->phases;
    a.taps = p->taps;
    a.mode = p->mode;
    a.alpha = timing_round(p, alpha);
    a.beta = timing_round(p, beta);
    a.max_dev = p->max_dev;
    return launch_timing(p->precision, a, p->variant, stream);
}
} // namespace

int sdsp_hip_timing_plan_create(sdsp_hip_timing_plan **out, uint64_t channels, int precision, int mode, uint32_t phases, uint32_t taps,
                                const double *h, uint64_t step0, double max_dev, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (channels == 0 || channels > 0x7fffffffull)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "channels must be in [1, 2^31)");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (mode != SDSP_HIP_TIMING_GARDNER && mode != SDSP_HIP_TIMING_ZC_QPSK && mode != SDSP_HIP_TIMING_ZC_BPSK)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "mode must be SDSP_HIP_TIMING_GARDNER, SDSP_HIP_TIMING_ZC_QPSK or SDSP_HIP_TIMING_ZC_BPSK");
    if (phases == 0 || phases > SDSP_HIP_TIMING_MAX_PHASES || (phases & (phases - 1)))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "phases must be a power of 2 in [1, SDSP_HIP_TIMING_MAX_PHASES]");
    if (taps == 0 || taps > SDSP_HIP_TIMING_MAX_TAPS || static_cast<uint64_t>(phases) * taps > SDSP_HIP_TIMING_MAX_TABLE)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps per phase must be in [1, SDSP_HIP_TIMING_MAX_TAPS] and phases * taps <= SDSP_HIP_TIMING_MAX_TABLE");
    if (step0 < SDSP_HIP_TIMING_MIN_STEP || step0 > SDSP_HIP_TIMING_MAX_STEP)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "step0 must be in [2^32, 2^38]");
    if (!h)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "h is null");
    const double dev_r = precision == SDSP_HIP_F64 ? max_dev : static_cast<double>(static_cast<float>(max_dev));
    if (!(dev_r > 0.0 && dev_r <= 0.5)) // NaN included
        return fail(SDSP_HIP_ERR_INVALID_ARG, "max_dev must be in (0, 0.5] in the plan precision");
    const size_t n = static_cast<size_t>(phases) * taps;
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(precision == SDSP_HIP_F64 ? h[i] : static_cast<double>(static_cast<float>(h[i]))))
            return fail(SDSP_HIP_ERR_INVALID_ARG, "every tap must be finite in the plan precision");
    if (int rc = use_device(device))
        return rc;
    std::vector<double> tab(n); // H[p][k] = h[k L + p], as sdsp_hip_arb_tables lays it out
    for (uint32_t p = 0; p < phases; p++)
        for (uint32_t k = 0; k < taps; k++)
            tab[static_cast<size_t>(p) * taps + k] = h[static_cast<size_t>(k) * phases + p];
    auto *p = new sdsp_hip_timing_plan();
    p->channels = channels;
    p->step0 = step0;
    p->phases = phases;
    p->taps = taps;
    p->precision = precision;
    p->mode = mode;
    p->device = device;
    p->max_dev = dev_r;
    const hipError_t e = upload_reals(tab.data(), tab.size(), precision, &p->table);
    if (e != hipSuccess) {
        sdsp_hip_timing_plan_destroy(p);
        return plan_fail(e, "timing");
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_timing_plan_destroy(sdsp_hip_timing_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK) {
        (void)hipFree(p->table);
        (void)hipFree(p->scratch);
    }
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_timing_state_bytes(const sdsp_hip_timing_plan *p, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = timing_state_layout(p).bytes;
    return SDSP_HIP_OK;
}

int sdsp_hip_timing_max_out(const sdsp_hip_timing_plan *p, uint64_t samples, uint64_t *n)
{
    if (!p || !n)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    return sdsp_hip_timing_max_out_for(p->step0, samples, n);
}

int sdsp_hip_timing_plan_set_variant(sdsp_hip_timing_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    if (variant == 1 && !p->scratch) {
        if (int rc = use_device(p->device))
            return rc;
        const hipError_t e = hipMalloc(&p->scratch, timing_state_layout(p).bytes);
        if (e != hipSuccess) {
            p->scratch = nullptr;
            return plan_fail(e, "timing");
        }
    }
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_timing_plan_launches(const sdsp_hip_timing_plan *p, uint64_t samples, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = samples ? 1 : 0;
    return SDSP_HIP_OK;
}

int sdsp_hip_timing_plan_get_info(const sdsp_hip_timing_plan *p, sdsp_hip_timing_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->channels = p->channels;
    info->step0 = p->step0;
    info->phases = p->phases;
    info->taps = p->taps;
    info->block = timing_block(p->precision);
    info->waves = timing_waves(p->precision, p->phases, p->taps);
    info->lds_bytes = timing_lds_bytes(p->precision, p->phases, p->taps);
    info->max_dev = p->max_dev;
    info->precision = p->precision;
    info->mode = p->mode;
    info->device = p->device;
    info->variant = p->variant;
    std::strncpy(info->kernel, timing_kernel_for(p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}

int sdsp_hip_timing_process(sdsp_hip_timing_plan *p, const void *x, uint64_t x_stride, void *y, uint64_t y_stride, void *err,
                            uint64_t err_stride, void *period, uint64_t period_stride, uint32_t *counts, uint64_t samples, double alpha,
                            double beta, void *state, void *stream)
{
    if (int rc = timing_check(p, x, x_stride, y, y_stride, err, err_stride, period, period_stride, counts, samples, alpha, beta))
        return rc;
    if (misaligned(counts, sizeof(uint32_t)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "counts must be aligned to 4 bytes");
    if (samples == 0) {
        if (!counts)
            return SDSP_HIP_OK;
        if (int rc = use_device(p->device))
            return rc;
        HIP_TRY(hipMemsetAsync(counts, 0, p->channels * sizeof(uint32_t), reinterpret_cast<hipStream_t>(stream)));
        return SDSP_HIP_OK;
    }
    const uint64_t es = esize(p->precision), rs = real_size(p->precision), cap = timing_cap(p, samples);
    auto span = [&](uint64_t stride, uint64_t n, uint64_t bytes) { return ((p->channels - 1) * stride + n) * bytes; };
    const void *ptr[6] = { x, y, err, period, counts, state };
    const uint64_t bytes[6] = { span(x_stride, samples, es), span(y_stride, cap, es),   span(err_stride, cap, rs),
                                span(period_stride, cap, rs), p->channels * sizeof(uint32_t), timing_state_layout(p).bytes };
    for (int i = 0; i < 6; i++)
        for (int j = i + 1; j < 6; j++)
            if (ranges_overlap(ptr[i], bytes[i], ptr[j], bytes[j]))
                return fail(SDSP_HIP_ERR_INVALID_ARG, "x, y, err, period, counts and the state buffer must not overlap one another");
    if (misaligned(x, es) || misaligned(y, es) || misaligned(err, rs) || misaligned(period, rs) || misaligned(state, 8))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "x, y, err and period must be aligned to their element size and state to 8 bytes");
    if (int rc = use_device(p->device))
        return rc;
    return timing_run(p, x, x_stride, y, y_stride, err, err_stride, period, period_stride, counts, samples, alpha, beta, state,
                      reinterpret_cast<hipStream_t>(stream));
}

int sdsp_hip_timing_process_host(sdsp_hip_timing_plan *p, const void *host_x, uint64_t x_stride, void *host_y, uint64_t y_stride,
                                 void *host_err, uint64_t err_stride, void *host_period, uint64_t period_stride, uint32_t *host_counts,
                                 uint64_t samples, double alpha, double beta, void *host_state)
{
    if (int rc = timing_check(p, host_x, x_stride, host_y, y_stride, host_err, err_stride, host_period, period_stride, host_counts, samples,
                              alpha, beta))
        return rc;
    if (samples == 0) {
        if (host_counts)
            std::memset(host_counts, 0, static_cast<size_t>(p->channels) * sizeof(uint32_t));
        return SDSP_HIP_OK;
    }
    if (int rc = use_device(p->device))
        return rc;
    const uint64_t es = esize(p->precision), rs = real_size(p->precision), cap = timing_cap(p, samples);
    auto span = [&](uint64_t stride, uint64_t n, uint64_t bytes) { return static_cast<size_t>(((p->channels - 1) * stride + n) * bytes); };
    host_stage st("timing", { { host_x, span(x_stride, samples, es), false },
                              { host_y, span(y_stride, cap, es), true },
                              { host_err, span(err_stride, cap, rs), true },
                              { host_period, span(period_stride, cap, rs), true },
                              { host_counts, static_cast<size_t>(p->channels) * sizeof(uint32_t), true },
                              { host_state, static_cast<size_t>(timing_state_layout(p).bytes), true } });
    int rc = st.in();
    if (!rc)
        rc = timing_run(p, st.dev[0], x_stride, st.dev[1], y_stride, st.dev[2], err_stride, st.dev[3], period_stride,
                        static_cast<uint32_t *>(st.dev[4]), samples, alpha, beta, st.dev[5], nullptr);
    return st.out(rc);
}
// ------------------------------------------------------------------ column FFT plans (fft_cols.hip)

namespace
{
constexpr uint64_t kFftColsMaxElements = 1ull << 40;

uint64_t fft_cols_out_esize(const sdsp_hip_fft_cols_plan *p)
{
    return p->output == SDSP_HIP_FFT_COLS_POWER ? real_size(p->precision) : esize(p->precision);
}

// argument checks shared by exec and exec_host (device pointers or not): in == out is in place (complex output only), any other
// overlap is refused
int fft_cols_check(const sdsp_hip_fft_cols_plan *p, const void *in, const void *out, uint64_t batch)
{
    if (!p || !in || !out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    const uint64_t cube = static_cast<uint64_t>(p->n) * p->width; // < 2^40
    if (batch >= kFftColsMaxElements || batch * cube >= kFftColsMaxElements)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "batch n width must be below 2^40");
    if (batch == 0)
        return SDSP_HIP_OK;
    const uint64_t es = esize(p->precision), oes = fft_cols_out_esize(p);
    if (misaligned(in, es) || misaligned(out, oes))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in and out must be aligned to their element size");
    if (in == out) {
        if (p->output == SDSP_HIP_FFT_COLS_POWER)
            return fail(SDSP_HIP_ERR_INVALID_ARG, "POWER output runs out of place: in and out ranges overlap");
    } else if (ranges_overlap(in, batch * cube * es, out, batch * cube * oes)) {
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in and out ranges overlap (out must equal in or lie apart from it)");
    }
    return SDSP_HIP_OK;
}

fft_cols_args fft_cols_args_of(const sdsp_hip_fft_cols_plan *p, const void *in, void *out, uint64_t batch)
{
    fft_cols_args a{};
    a.in = in;
    a.out = out;
    a.tw = p->tw;
    a.window = p->window;
    a.width = p->width;
    a.batch = batch;
    a.n = p->n;
    a.reverse = p->direction == SDSP_HIP_REVERSE;
    a.power = p->output == SDSP_HIP_FFT_COLS_POWER;
    a.shift = p->shift;
    return a;
}
} // namespace

int sdsp_hip_fft_cols_plan_create(sdsp_hip_fft_cols_plan **out, uint32_t n, uint64_t width, int direction, int precision, int output,
                                  int shift, const double *window, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (!sdsp_hip_is_power_of_2(n) || n < SDSP_HIP_FFT_COLS_MIN_N || n > SDSP_HIP_FFT_COLS_MAX_N)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "n must be a power of 2 in [SDSP_HIP_FFT_COLS_MIN_N, SDSP_HIP_FFT_COLS_MAX_N]");
    if (width == 0 || width >= kFftColsMaxElements / n)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "width must be at least 1 with n width below 2^40");
    if (direction != SDSP_HIP_FORWARD && direction != SDSP_HIP_REVERSE)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "direction must be SDSP_HIP_FORWARD or SDSP_HIP_REVERSE");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (output != SDSP_HIP_FFT_COLS_COMPLEX && output != SDSP_HIP_FFT_COLS_POWER)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "output must be SDSP_HIP_FFT_COLS_COMPLEX or SDSP_HIP_FFT_COLS_POWER");
    if (direction == SDSP_HIP_REVERSE && (window || output == SDSP_HIP_FFT_COLS_POWER))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "only FORWARD plans take a window or POWER output");
    if (window)
        for (uint32_t i = 0; i < n; i++) {
            const double w = precision == SDSP_HIP_F64 ? window[i] : static_cast<double>(static_cast<float>(window[i]));
            if (!std::isfinite(w))
                return fail(SDSP_HIP_ERR_INVALID_ARG, "window values must be finite once rounded to the precision");
        }
    if (int rc = use_device(device))
        return rc;
    auto *p = new sdsp_hip_fft_cols_plan();
    p->n = n;
    p->width = width;
    p->direction = direction;
    p->precision = precision;
    p->output = output;
    p->shift = shift != 0;
    p->device = device;
    std::vector<double> w;
    make_twiddles(n, direction, w);
    int rc = upload_twiddles(w, precision, &p->tw);
    if (!rc && window) {
        const hipError_t e = upload_reals(window, n, precision, &p->window);
        if (e != hipSuccess)
            rc = plan_fail(e, "fft_cols");
    }
    if (!rc) // the kernel's dynamic-LDS limit, so that exec sets no attribute (it may be captured)
        rc = launch_fft_cols(precision, fft_cols_args_of(p, nullptr, nullptr, 0), 0, nullptr);
    if (rc) {
        sdsp_hip_fft_cols_plan_destroy(p);
        return rc;
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_fft_cols_plan_destroy(sdsp_hip_fft_cols_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK) {
        (void)hipFree(p->tw);
        (void)hipFree(p->window);
    }
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_fft_cols_exec(sdsp_hip_fft_cols_plan *p, const void *in, void *out, uint64_t batch, void *stream)
{
    if (int rc = fft_cols_check(p, in, out, batch))
        return rc;
    if (batch == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    return launch_fft_cols(p->precision, fft_cols_args_of(p, in, out, batch), p->variant, stream);
}

int sdsp_hip_fft_cols_exec_host(sdsp_hip_fft_cols_plan *p, const void *host_in, void *host_out, uint64_t batch)
{
    if (int rc = fft_cols_check(p, host_in, host_out, batch))
        return rc;
    if (batch == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const uint64_t elements = batch * p->n * p->width;
    const size_t in_bytes = static_cast<size_t>(elements * esize(p->precision));
    const size_t out_bytes = static_cast<size_t>(elements * fft_cols_out_esize(p));
    const bool in_place = host_in == host_out;
    // in place: one device buffer, read back; else the input and an output buffer
    host_stage st("fft_cols", { { host_in, in_bytes, in_place }, { in_place ? nullptr : host_out, out_bytes, true } });
    int rc = st.in();
    if (!rc)
        rc = launch_fft_cols(p->precision, fft_cols_args_of(p, st.dev[0], in_place ? st.dev[0] : st.dev[1], batch), p->variant, nullptr);
    if (!rc) {
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess)
            rc = hip_fail(e, "fft_cols exec_host");
    }
    return st.out(rc);
}

int sdsp_hip_fft_cols_plan_set_variant(sdsp_hip_fft_cols_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_fft_cols_plan_launches(const sdsp_hip_fft_cols_plan *p, uint64_t batch, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = fft_cols_launches(p->precision, p->n, p->width, batch, p->variant);
    return SDSP_HIP_OK;
}

int sdsp_hip_fft_cols_plan_get_info(const sdsp_hip_fft_cols_plan *p, sdsp_hip_fft_cols_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    const fft_cols_shape s = fft_cols_shape_for(p->precision, p->n, p->variant);
    info->n = p->n;
    info->width = p->width;
    info->direction = p->direction;
    info->precision = p->precision;
    info->output = p->output;
    info->shift = p->shift;
    info->windowed = p->window != nullptr;
    info->device = p->device;
    info->variant = p->variant;
    info->tile_columns = s.tile_columns;
    info->threads = s.threads;
    info->lds_bytes = s.lds_bytes;
    info->algorithmic_bytes = static_cast<uint64_t>(p->n) * p->width * (esize(p->precision) + fft_cols_out_esize(p));
    std::strncpy(info->kernel, fft_cols_kernel_for(p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}
// ------------------------------------------------------------------ 2-D CFAR plans (cfar2d.hip)

namespace
{
constexpr uint64_t kCfar2dMaxCells = 1ull << 40;

// the window and the map sizes of a descriptor, without a device
int cfar2d_check_shape(uint32_t D, uint32_t R, const sdsp_hip_cfar2d_desc *d)
{
    if (!d)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "descriptor is null");
    if (d->train_r > SDSP_HIP_CFAR2D_MAX_R || d->guard_r > SDSP_HIP_CFAR2D_MAX_R)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "train_r and guard_r must be at most SDSP_HIP_CFAR2D_MAX_R");
    if (d->train_d > SDSP_HIP_CFAR2D_MAX_TRAIN_D || d->guard_d > SDSP_HIP_CFAR2D_MAX_GUARD_D)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "train_d must be at most SDSP_HIP_CFAR2D_MAX_TRAIN_D, guard_d at most SDSP_HIP_CFAR2D_MAX_GUARD_D");
    if (d->train_d + d->train_r == 0)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "train_d + train_r must be at least 1");
    if (D < 2 * (d->train_d + d->guard_d) + 1 || D > SDSP_HIP_CFAR2D_MAX_D)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "D must be in [2 (train_d + guard_d) + 1, SDSP_HIP_CFAR2D_MAX_D]");
    if (R == 0 || R >= (1u << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "R must be in [1, 2^31)");
    if (d->edge != SDSP_HIP_CFAR2D_EDGE_MARK && d->edge != SDSP_HIP_CFAR2D_EDGE_CLIP)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "edge must be SDSP_HIP_CFAR2D_EDGE_MARK or SDSP_HIP_CFAR2D_EDGE_CLIP");
    return SDSP_HIP_OK;
}

// n(r): the training cells of column r that lie inside the map
uint64_t cfar2d_cells(uint32_t R, const sdsp_hip_cfar2d_desc *d, uint32_t r)
{
    auto inside = [&](int64_t half) { return std::min<int64_t>(r + half, static_cast<int64_t>(R) - 1) - std::max<int64_t>(r - half, 0) + 1; };
    const int64_t Hd = d->train_d + d->guard_d, Hr = d->train_r + d->guard_r;
    return static_cast<uint64_t>((2 * Hd + 1) * inside(Hr) - (2 * int64_t(d->guard_d) + 1) * inside(d->guard_r));
}

int cfar2d_upload_alpha(sdsp_hip_cfar2d_plan *p, double alpha)
{
    std::vector<double> c(p->R);
    for (uint32_t r = 0; r < p->R; r++)
        c[r] = alpha / static_cast<double>(cfar2d_cells(p->R, &p->desc, r));
    if (!p->scale)
        return upload_reals(c.data(), c.size(), p->precision, &p->scale) == hipSuccess ? SDSP_HIP_OK : fail(SDSP_HIP_ERR_NOMEM, "cfar2d plan: the scale table");
    if (p->precision == SDSP_HIP_F64) {
        HIP_TRY(hipMemcpy(p->scale, c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice));
    } else {
        const std::vector<float> f(c.begin(), c.end());
        HIP_TRY(hipMemcpy(p->scale, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return SDSP_HIP_OK;
}

size_t cfar2d_record(int precision) { return precision == SDSP_HIP_F64 ? sizeof(sdsp_hip_cfar2d_hit_f64) : sizeof(sdsp_hip_cfar2d_hit_f32); }

// argument checks shared by process and process_host (device pointers or not)
int cfar2d_check(const sdsp_hip_cfar2d_plan *p, const void *in, const void *thr, const void *det, const void *hits, const void *counts,
                 uint64_t cap, uint64_t maps)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (maps > p->max_maps)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "maps must be at most the plan's max_maps");
    if (cap >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "cap must be below 2^31");
    if (maps == 0)
        return SDSP_HIP_OK;
    if (!in)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "p is null");
    if (!thr && !det && !hits && !counts)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "every output is null");
    if (!hits != !counts)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "hits and counts go together");
    const uint64_t rs = real_size(p->precision), cells = maps * p->D * p->R;
    if (misaligned(in, rs) || misaligned(thr, rs) || misaligned(hits, rs) || misaligned(counts, 4))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "p, thr, hits and counts must be aligned to their element size");
    const void *ptr[5] = { in, thr, det, hits, counts };
    const uint64_t bytes[5] = { cells * rs, cells * rs, cells, maps * cap * cfar2d_record(p->precision), maps * 4 };
    for (int i = 0; i < 5; i++)
        for (int j = i + 1; j < 5; j++)
            if (ranges_overlap(ptr[i], bytes[i], ptr[j], bytes[j]))
                return fail(SDSP_HIP_ERR_INVALID_ARG, "the input and the outputs must not overlap one another");
    return SDSP_HIP_OK;
}

cfar2d_args cfar2d_args_of(const sdsp_hip_cfar2d_plan *p, const void *in, void *thr, uint8_t *det, void *hits, uint32_t *counts, uint64_t cap,
                           uint64_t maps)
{
    cfar2d_args a{};
    a.p = in;
    a.thr = thr;
    a.det = det;
    a.hits = hits;
    a.counts = counts;
    a.scale = p->scale;
    a.ws_mask = p->ws_mask;
    a.ws_cnt = static_cast<uint32_t *>(p->ws_cnt);
    a.maps = maps;
    a.cap = cap;
    a.D = p->D;
    a.R = p->R;
    a.Ld = p->desc.train_d;
    a.Gd = p->desc.guard_d;
    a.Lr = p->desc.train_r;
    a.Gr = p->desc.guard_r;
    a.clip = p->desc.edge == SDSP_HIP_CFAR2D_EDGE_CLIP;
    a.peak = p->desc.peak != 0;
    return a;
}
} // namespace

int sdsp_hip_cfar2d_scale(uint32_t D, uint32_t R, const sdsp_hip_cfar2d_desc *d, double pfa, double *scale)
{
    if (int rc = cfar2d_check_shape(D, R, d))
        return rc;
    if (!scale || !(pfa > 0.0 && pfa < 1.0))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "scale must not be null and pfa must lie in (0, 1)");
    for (uint32_t r = 0; r < R; r++) {
        const uint64_t n = cfar2d_cells(R, d, r);
        scale[r] = n ? std::pow(pfa, -1.0 / static_cast<double>(n)) - 1.0 : HUGE_VAL;
    }
    return SDSP_HIP_OK;
}

int sdsp_hip_cfar2d_plan_create(sdsp_hip_cfar2d_plan **out, uint32_t D, uint32_t R, uint64_t max_maps, const sdsp_hip_cfar2d_desc *d,
                                const double *scale, int precision, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (int rc = cfar2d_check_shape(D, R, d))
        return rc;
    if (max_maps == 0 || max_maps >= kCfar2dMaxCells || max_maps * D >= kCfar2dMaxCells || max_maps * D * R >= kCfar2dMaxCells)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "max_maps must be at least 1 with max_maps D R below 2^40");
    if (precision != SDSP_HIP_F32 && precision != SDSP_HIP_F64)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "precision must be SDSP_HIP_F32 or SDSP_HIP_F64");
    if (scale)
        for (uint32_t r = 0; r < R; r++) {
            const double c = precision == SDSP_HIP_F64 ? scale[r] : static_cast<double>(static_cast<float>(scale[r]));
            if (!std::isfinite(c))
                return fail(SDSP_HIP_ERR_INVALID_ARG, "scale values must be finite once rounded to the precision");
        }
    if (int rc = use_device(device))
        return rc;
    auto *p = new sdsp_hip_cfar2d_plan();
    p->D = D;
    p->R = R;
    p->max_maps = max_maps;
    p->desc = *d;
    p->desc.peak = d->peak != 0;
    p->tabled = scale != nullptr;
    p->precision = precision;
    p->device = device;
    int rc = SDSP_HIP_OK;
    if (scale) {
        const hipError_t e = upload_reals(scale, R, precision, &p->scale);
        if (e != hipSuccess)
            rc = plan_fail(e, "cfar2d");
    } else {
        rc = cfar2d_upload_alpha(p, d->alpha);
    }
    if (!rc) {
        uint64_t mask_bytes = 0, cnt_bytes = 0;
        cfar2d_workspace(D, R, max_maps, &mask_bytes, &cnt_bytes);
        p->ws_bytes = mask_bytes + cnt_bytes;
        hipError_t e = hipMalloc(&p->ws_mask, mask_bytes);
        if (e == hipSuccess)
            e = hipMalloc(&p->ws_cnt, cnt_bytes);
        if (e != hipSuccess)
            rc = plan_fail(e, "cfar2d");
    }
    if (!rc) // the kernel's dynamic-LDS limit, so that process sets no attribute (it may be captured)
        rc = launch_cfar2d(precision, cfar2d_args{}, 0, nullptr);
    if (rc) {
        sdsp_hip_cfar2d_plan_destroy(p);
        return rc;
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_cfar2d_plan_destroy(sdsp_hip_cfar2d_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK) {
        (void)hipFree(p->scale);
        (void)hipFree(p->ws_mask);
        (void)hipFree(p->ws_cnt);
    }
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_cfar2d_process(sdsp_hip_cfar2d_plan *p, const void *in, void *thr, uint8_t *det, void *hits, uint32_t *counts, uint64_t cap,
                            uint64_t maps, void *stream)
{
    if (int rc = cfar2d_check(p, in, thr, det, hits, counts, cap, maps))
        return rc;
    if (maps == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    return launch_cfar2d(p->precision, cfar2d_args_of(p, in, thr, det, hits, counts, cap, maps), p->variant, stream);
}

int sdsp_hip_cfar2d_process_host(sdsp_hip_cfar2d_plan *p, const void *host_p, void *host_thr, uint8_t *host_det, void *host_hits,
                                 uint32_t *host_counts, uint64_t cap, uint64_t maps)
{
    if (int rc = cfar2d_check(p, host_p, host_thr, host_det, host_hits, host_counts, cap, maps))
        return rc;
    if (maps == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const size_t rs = real_size(p->precision), cells = static_cast<size_t>(maps * p->D * p->R);
    const size_t list_bytes = static_cast<size_t>(maps * cap) * cfar2d_record(p->precision);
    // a list of cap == 0 has no bytes to stage: the kernels still need a pointer that says "with a list", and write nothing through it
    host_stage st("cfar2d", { { host_p, cells * rs, false }, { host_thr, cells * rs, true }, { host_det, cells, true },
                          { list_bytes ? host_hits : nullptr, list_bytes, true }, { host_counts, static_cast<size_t>(maps) * 4, true } });
    int rc = st.in();
    if (!rc) {
        void *hits = host_hits && !list_bytes ? p->ws_mask : st.dev[3];
        rc = launch_cfar2d(p->precision,
                           cfar2d_args_of(p, st.dev[0], st.dev[1], static_cast<uint8_t *>(st.dev[2]), hits, static_cast<uint32_t *>(st.dev[4]), cap, maps),
                           p->variant, nullptr);
    }
    if (!rc) {
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess)
            rc = hip_fail(e, "cfar2d process_host");
    }
    return st.out(rc);
}

int sdsp_hip_cfar2d_plan_set_alpha(sdsp_hip_cfar2d_plan *p, double alpha)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (p->tabled)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "the plan was made with a scale table");
    if (int rc = use_device(p->device))
        return rc;
    if (int rc = cfar2d_upload_alpha(p, alpha))
        return rc;
    p->desc.alpha = alpha;
    return SDSP_HIP_OK;
}

int sdsp_hip_cfar2d_plan_set_variant(sdsp_hip_cfar2d_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_cfar2d_plan_launches(const sdsp_hip_cfar2d_plan *p, int with_thr_or_det, int with_hits, uint64_t *launches)
{
    if (!p || !launches || (!with_thr_or_det && !with_hits))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument, or no output");
    *launches = cfar2d_launches(p->variant, with_thr_or_det != 0, with_hits != 0);
    return SDSP_HIP_OK;
}

int sdsp_hip_cfar2d_plan_get_info(const sdsp_hip_cfar2d_plan *p, sdsp_hip_cfar2d_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    const sdsp_hip_cfar2d_desc &d = p->desc;
    const cfar2d_shape s = cfar2d_shape_for(p->precision, p->D, d.train_d, d.guard_d, d.train_r, d.guard_r, p->variant);
    info->D = p->D;
    info->R = p->R;
    info->max_maps = p->max_maps;
    info->train_d = d.train_d;
    info->guard_d = d.guard_d;
    info->train_r = d.train_r;
    info->guard_r = d.guard_r;
    info->cells = (2 * (d.train_d + d.guard_d) + 1) * (2 * (d.train_r + d.guard_r) + 1) - (2 * d.guard_d + 1) * (2 * d.guard_r + 1);
    info->edge = d.edge;
    info->peak = d.peak;
    info->tabled = p->tabled;
    info->precision = p->precision;
    info->device = p->device;
    info->variant = p->variant;
    info->alpha = d.alpha;
    info->tile_rows = s.tile_rows;
    info->tile_cols = s.tile_cols;
    info->threads = s.threads;
    info->lds_bytes = s.lds_bytes;
    info->workspace_bytes = p->ws_bytes;
    std::strncpy(info->kernel, cfar2d_kernel_for(p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}
// ------------------------------------------------------------------ Viterbi decoder banks (viterbi.hip)

namespace
{
// the code of a plan or of the encoder, without a device
int viterbi_check_code(uint32_t k, uint32_t n, const uint32_t *generators)
{
    if (k < SDSP_HIP_VITERBI_MIN_K || k > SDSP_HIP_VITERBI_MAX_K)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "k must be in [3, 9]");
    if (n < 2 || n > 3)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "n must be 2 or 3");
    if (!generators)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "generators is null");
    for (uint32_t j = 0; j < n; j++)
        if (generators[j] == 0 || generators[j] >= (1u << k))
            return fail(SDSP_HIP_ERR_INVALID_ARG, "every generator must be in [1, 2^k)");
    return SDSP_HIP_OK;
}

int viterbi_check_traceback(uint32_t block, uint32_t depth, uint32_t min_depth)
{
    if (block < 32 || block > SDSP_HIP_VITERBI_MAX_BLOCK || block % 32 != 0)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "block must be a multiple of 32 in [32, 1024]");
    if (depth < min_depth || depth > SDSP_HIP_VITERBI_MAX_DEPTH)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "depth must be in [k - 1, 4096]");
    return SDSP_HIP_OK;
}

struct viterbi_layout {
    uint64_t filled_off, hist_off, bytes;
};
viterbi_layout viterbi_layout_of(uint32_t k, uint32_t dr, uint64_t max_channels)
{
    const uint64_t S = 1ull << (k - 1), W = S > 64 ? S / 64 : 1;
    viterbi_layout l{};
    l.filled_off = max_channels * S * 4;
    l.hist_off = (l.filled_off + max_channels * 4 + 7) / 8 * 8;
    l.bytes = l.hist_off + max_channels * dr * W * 8;
    return l;
}

size_t viterbi_in_size(const sdsp_hip_viterbi_plan *p) { return p->in_kind == SDSP_HIP_VITERBI_F32 ? 4 : 1; }
// bytes of a row of `steps` outputs
uint64_t viterbi_out_row(const sdsp_hip_viterbi_plan *p, uint64_t steps) { return p->out_kind == SDSP_HIP_VITERBI_PACKED ? steps / 8 : steps; }

// argument checks shared by process and process_host (device pointers or not)
int viterbi_check(const sdsp_hip_viterbi_plan *p, const void *in, const void *out, uint64_t channels, uint64_t steps, bool device_ptrs)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (channels > p->max_channels)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "channels must be at most the plan's max_channels");
    if (steps >= (1ull << 31) || steps % p->block != 0)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "steps must be a multiple of the plan's block, below 2^31");
    if (channels == 0 || steps == 0)
        return SDSP_HIP_OK;
    if (!in || !out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in and out must not be null");
    if (misaligned(in, viterbi_in_size(p)) || misaligned(out, p->out_kind == SDSP_HIP_VITERBI_PACKED ? 4 : 1))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in and out must be aligned to their element size");
    const uint64_t in_bytes = channels * steps * p->n * viterbi_in_size(p), out_bytes = channels * viterbi_out_row(p, steps);
    if (ranges_overlap(in, in_bytes, out, out_bytes))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in and out must not overlap");
    if (device_ptrs && (ranges_overlap(in, in_bytes, p->state, p->state_bytes) || ranges_overlap(out, out_bytes, p->state, p->state_bytes)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in and out must not overlap the plan's state");
    return SDSP_HIP_OK;
}

viterbi_args viterbi_args_of(const sdsp_hip_viterbi_plan *p, const void *in, void *out, uint64_t channels, uint64_t steps)
{
    const viterbi_layout l = viterbi_layout_of(p->k, p->dr, p->max_channels);
    char *s = static_cast<char *>(p->state);
    viterbi_args a{};
    a.in = in;
    a.out = out;
    a.metrics = reinterpret_cast<uint32_t *>(s);
    a.filled = reinterpret_cast<uint32_t *>(s + l.filled_off);
    a.hist = reinterpret_cast<uint64_t *>(s + l.hist_off);
    a.ring_ws = static_cast<uint64_t *>(p->ring_ws);
    a.channels = channels;
    a.steps = steps;
    a.k = p->k;
    a.n = p->n;
    for (uint32_t j = 0; j < p->n; j++)
        a.generators[j] = p->generators[j];
    a.block = p->block;
    a.depth = p->depth;
    a.dr = p->dr;
    a.in_kind = p->in_kind;
    a.out_kind = p->out_kind;
    a.scale = p->scale;
    return a;
}
} // namespace

int sdsp_hip_viterbi_delay(uint32_t block, uint32_t depth, uint32_t *delay)
{
    if (!delay)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "delay is null");
    if (int rc = viterbi_check_traceback(block, depth, 1))
        return rc;
    *delay = (depth + block - 1) / block * block;
    return SDSP_HIP_OK;
}

int sdsp_hip_conv_encode(uint32_t k, uint32_t n, const uint32_t *generators, const uint8_t *bits, uint64_t nbits, int terminate, uint8_t *out)
{
    if (int rc = viterbi_check_code(k, n, generators))
        return rc;
    const uint64_t total = nbits + (terminate ? k - 1 : 0);
    if ((!bits && nbits) || (!out && total))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "bits and out must not be null");
    uint32_t grev[3] = {};
    for (uint32_t j = 0; j < n; j++)
        for (uint32_t b = 0; b < k; b++)
            grev[j] |= ((generators[j] >> b) & 1u) << (k - 1 - b);
    uint32_t reg = 0; // the input of i steps ago in bit i
    for (uint64_t t = 0; t < total; t++) {
        reg = ((reg << 1) | (t < nbits && bits[t] ? 1u : 0u)) & ((1u << k) - 1);
        for (uint32_t j = 0; j < n; j++)
            out[t * n + j] = static_cast<uint8_t>(__builtin_popcount(grev[j] & reg) & 1);
    }
    return SDSP_HIP_OK;
}

int sdsp_hip_viterbi_plan_create(sdsp_hip_viterbi_plan **out, uint32_t k, uint32_t n, const uint32_t *generators, uint32_t block,
                                 uint32_t depth, int in_kind, int out_kind, float scale, uint64_t max_channels, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (int rc = viterbi_check_code(k, n, generators))
        return rc;
    if (int rc = viterbi_check_traceback(block, depth, k - 1))
        return rc;
    if (max_channels == 0 || max_channels >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "max_channels must be in [1, 2^31)");
    if (in_kind != SDSP_HIP_VITERBI_I8 && in_kind != SDSP_HIP_VITERBI_F32)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_kind must be SDSP_HIP_VITERBI_I8 or SDSP_HIP_VITERBI_F32");
    if (out_kind != SDSP_HIP_VITERBI_BYTES && out_kind != SDSP_HIP_VITERBI_PACKED)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "out_kind must be SDSP_HIP_VITERBI_BYTES or SDSP_HIP_VITERBI_PACKED");
    if (in_kind == SDSP_HIP_VITERBI_F32 && !(std::isfinite(scale) && scale > 0.0f))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "scale must be finite and above 0");
    if (int rc = use_device(device))
        return rc;
    auto *p = new sdsp_hip_viterbi_plan();
    p->k = k;
    p->n = n;
    for (uint32_t j = 0; j < n; j++)
        p->generators[j] = generators[j];
    p->block = block;
    p->depth = depth;
    p->dr = (depth + block - 1) / block * block;
    p->in_kind = in_kind;
    p->out_kind = out_kind;
    p->scale = in_kind == SDSP_HIP_VITERBI_F32 ? scale : 1.0f;
    p->max_channels = max_channels;
    p->device = device;
    p->variant = k == 7 ? 0 : 1;
    p->state_bytes = viterbi_layout_of(k, p->dr, max_channels).bytes;
    int rc = SDSP_HIP_OK;
    hipError_t e = hipMalloc(&p->state, p->state_bytes);
    const viterbi_shape plain = viterbi_shape_for(k, n, block, p->dr, 1);
    if (e == hipSuccess && !plain.ring_in_lds) {
        p->ring_bytes = max_channels * plain.ring_steps * ((1ull << (k - 1)) / 64) * 8;
        e = hipMalloc(&p->ring_ws, p->ring_bytes);
    }
    if (e != hipSuccess)
        rc = plan_fail(e, "viterbi");
    if (!rc)
        rc = sdsp_hip_viterbi_plan_reset(p, -1);
    if (!rc) // the kernels' dynamic-LDS limit, so that process sets no attribute (it may be captured)
        rc = launch_viterbi(viterbi_args{}, 0, nullptr);
    if (rc) {
        sdsp_hip_viterbi_plan_destroy(p);
        return rc;
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_viterbi_plan_destroy(sdsp_hip_viterbi_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK) {
        (void)hipFree(p->state);
        (void)hipFree(p->ring_ws);
    }
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_viterbi_process(sdsp_hip_viterbi_plan *p, const void *in, void *out, uint64_t channels, uint64_t steps, void *stream)
{
    if (int rc = viterbi_check(p, in, out, channels, steps, true))
        return rc;
    if (channels == 0 || steps == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    return launch_viterbi(viterbi_args_of(p, in, out, channels, steps), p->variant, stream);
}

int sdsp_hip_viterbi_process_host(sdsp_hip_viterbi_plan *p, const void *host_in, void *host_out, uint64_t channels, uint64_t steps)
{
    if (int rc = viterbi_check(p, host_in, host_out, channels, steps, false))
        return rc;
    if (channels == 0 || steps == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    host_stage st("viterbi", { { host_in, static_cast<size_t>(channels * steps * p->n) * viterbi_in_size(p), false },
                           { host_out, static_cast<size_t>(channels * viterbi_out_row(p, steps)), true } });
    int rc = st.in();
    if (!rc)
        rc = launch_viterbi(viterbi_args_of(p, st.dev[0], st.dev[1], channels, steps), p->variant, nullptr);
    if (!rc) {
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess)
            rc = hip_fail(e, "viterbi process_host");
    }
    return st.out(rc);
}

int sdsp_hip_viterbi_plan_reset(sdsp_hip_viterbi_plan *p, int start_state)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    const uint32_t S = 1u << (p->k - 1);
    if (start_state < -1 || start_state >= static_cast<int>(S))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "start_state must be -1 or a state of the code");
    if (int rc = use_device(p->device))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(p->state, 0, p->state_bytes));
    if (start_state >= 0) {
        std::vector<int32_t> row(S, SDSP_HIP_VITERBI_START_METRIC);
        row[static_cast<size_t>(start_state)] = 0;
        // one row, then doubling copies on the device
        HIP_TRY(hipMemcpy(p->state, row.data(), S * 4, hipMemcpyHostToDevice));
        for (uint64_t have = 1; have < p->max_channels; have *= 2) {
            const uint64_t more = std::min<uint64_t>(have, p->max_channels - have);
            HIP_TRY(hipMemcpy(static_cast<char *>(p->state) + have * S * 4, p->state, more * S * 4, hipMemcpyDeviceToDevice));
        }
    }
    HIP_TRY(hipDeviceSynchronize());
    return SDSP_HIP_OK;
}

int sdsp_hip_viterbi_plan_get_metrics(sdsp_hip_viterbi_plan *p, int32_t *host_metrics, uint64_t channels)
{
    if (!p || !host_metrics)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    if (channels > p->max_channels)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "channels must be at most the plan's max_channels");
    if (int rc = use_device(p->device))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (channels)
        HIP_TRY(hipMemcpy(host_metrics, p->state, channels * (4ull << (p->k - 1)), hipMemcpyDeviceToHost));
    return SDSP_HIP_OK;
}

int sdsp_hip_viterbi_plan_set_metrics(sdsp_hip_viterbi_plan *p, const int32_t *host_metrics, uint64_t channels)
{
    if (!p || !host_metrics)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    if (channels > p->max_channels)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "channels must be at most the plan's max_channels");
    if (int rc = use_device(p->device))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (channels)
        HIP_TRY(hipMemcpy(p->state, host_metrics, channels * (4ull << (p->k - 1)), hipMemcpyHostToDevice));
    return SDSP_HIP_OK;
}

int sdsp_hip_viterbi_plan_state_bytes(const sdsp_hip_viterbi_plan *p, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = p->state_bytes;
    return SDSP_HIP_OK;
}

int sdsp_hip_viterbi_plan_set_variant(sdsp_hip_viterbi_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    if (variant == 0 && p->k != 7)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "the wave kernel serves K = 7 only");
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_viterbi_plan_launches(const sdsp_hip_viterbi_plan *p, uint64_t channels, uint64_t steps, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = channels && steps ? 1 : 0;
    return SDSP_HIP_OK;
}

int sdsp_hip_viterbi_plan_get_info(const sdsp_hip_viterbi_plan *p, sdsp_hip_viterbi_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    const viterbi_shape s = viterbi_shape_for(p->k, p->n, p->block, p->dr, p->variant);
    info->k = p->k;
    info->n = p->n;
    for (uint32_t j = 0; j < p->n; j++)
        info->generators[j] = p->generators[j];
    info->states = 1u << (p->k - 1);
    info->block = p->block;
    info->depth = p->depth;
    info->delay = p->dr;
    info->chunk = s.chunk;
    info->threads = s.threads;
    info->waves = s.waves;
    info->lds_bytes = s.lds_bytes;
    info->ring_in_lds = s.ring_in_lds;
    info->max_channels = p->max_channels;
    info->state_bytes = p->state_bytes;
    info->scale = p->scale;
    info->in_kind = p->in_kind;
    info->out_kind = p->out_kind;
    info->device = p->device;
    info->variant = p->variant;
    std::strncpy(info->kernel, viterbi_kernel_for(p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}
// ------------------------------------------------------------------ Reed-Solomon decoder banks (rs.hip)

namespace
{
// exp[0 .. 512): alpha^i twice round (the last two entries stay 0), then log[0 .. 256); false where alpha = 2 has not order 255
bool rs_field_table(uint32_t field_poly, uint8_t *t)
{
    std::memset(t, 0, 768);
    uint32_t x = 1;
    for (uint32_t i = 0; i < 255; i++) {
        if (i && x == 1)
            return false;
        t[i] = t[i + 255] = static_cast<uint8_t>(x);
        t[512 + x] = static_cast<uint8_t>(i);
        x <<= 1;
        if (x & 0x100)
            x ^= field_poly;
    }
    return x == 1;
}

uint32_t rs_gcd(uint32_t a, uint32_t b)
{
    while (b) {
        const uint32_t r = a % b;
        a = b;
        b = r;
    }
    return a;
}

// the field and the roots of a code, without a device; t receives the field's table
int rs_check_code(uint32_t field_poly, uint32_t fcr, uint32_t prim, uint32_t nroots, uint8_t *t)
{
    if (field_poly < 0x100 || field_poly >= 0x200)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "field_poly must be a 9-bit polynomial with bit 8 set");
    if (fcr >= 255 || prim >= 255)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "fcr and prim must be below 255");
    if (nroots < 2 || nroots > SDSP_HIP_RS_MAX_NROOTS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "nroots must be in [2, 64]");
    if (rs_gcd(prim, 255) != 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "gcd(prim, 255) must be 1");
    if (!rs_field_table(field_poly, t))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "alpha = 2 must have order 255 under field_poly");
    return SDSP_HIP_OK;
}

int rs_check_frame(uint32_t nroots, uint32_t n, uint32_t interleave)
{
    if (n <= nroots || n > 255)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "n must be in (nroots, 255]");
    if (interleave < 1 || interleave > SDSP_HIP_RS_MAX_INTERLEAVE)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "interleave must be in [1, 16]");
    return SDSP_HIP_OK;
}

uint8_t rs_mul(const uint8_t *t, uint32_t a, uint32_t b) { return a && b ? t[t[512 + a] + t[512 + b]] : 0; }

// g[0 .. nroots]: the highest coefficient first
void rs_generator_of(const uint8_t *t, uint32_t fcr, uint32_t prim, uint32_t nroots, uint8_t *g)
{
    std::memset(g, 0, nroots + 1);
    g[0] = 1; // of degree 0 so far, kept at the front
    for (uint32_t j = 0; j < nroots; j++) {
        const uint32_t root = t[(prim * (fcr + j)) % 255];
        for (uint32_t c = j + 1; c >= 1; c--)
            g[c] = static_cast<uint8_t>(g[c] ^ rs_mul(t, g[c - 1], root));
    }
}

// argument checks shared by process and process_host
int rs_check(const sdsp_hip_rs_plan *p, const void *in, const void *erasures, const void *out, const int32_t *corrected, uint64_t frames)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (frames >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "frames must be below 2^31");
    if (frames == 0)
        return SDSP_HIP_OK;
    if (!in || !out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in and out must not be null");
    if (corrected && misaligned(corrected, 4))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "corrected must be aligned to 4 bytes");
    const bool data = p->out_kind == SDSP_HIP_RS_DATA;
    const uint64_t in_bytes = frames * p->interleave * p->n, out_bytes = frames * p->interleave * (data ? p->n - p->nroots : p->n);
    const uint64_t cor_bytes = frames * p->interleave * 4;
    if (!(in == out && !data) && ranges_overlap(in, in_bytes, out, out_bytes))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in and out must be the same (FULL) or apart");
    if (ranges_overlap(erasures, in_bytes, in, in_bytes) || ranges_overlap(erasures, in_bytes, out, out_bytes) ||
        ranges_overlap(corrected, cor_bytes, in, in_bytes) || ranges_overlap(corrected, cor_bytes, out, out_bytes) ||
        ranges_overlap(corrected, cor_bytes, erasures, in_bytes))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in, out, erasures and corrected must not overlap");
    return SDSP_HIP_OK;
}

rs_args rs_args_of(const sdsp_hip_rs_plan *p, const void *in, const void *erasures, void *out, int32_t *corrected, uint64_t frames)
{
    rs_args a{};
    a.in = in;
    a.out = out;
    a.erasures = erasures;
    a.corrected = corrected;
    a.table = p->table;
    a.frames = frames;
    a.n = p->n;
    a.nroots = p->nroots;
    a.interleave = p->interleave;
    a.fcr = p->fcr;
    a.prim = p->prim;
    a.data_only = p->out_kind == SDSP_HIP_RS_DATA;
    return a;
}
} // namespace

int sdsp_hip_rs_generator(uint32_t field_poly, uint32_t fcr, uint32_t prim, uint32_t nroots, uint8_t *g)
{
    uint8_t t[768];
    if (int rc = rs_check_code(field_poly, fcr, prim, nroots, t))
        return rc;
    if (!g)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "g is null");
    rs_generator_of(t, fcr, prim, nroots, g);
    return SDSP_HIP_OK;
}

int sdsp_hip_rs_encode(uint32_t field_poly, uint32_t fcr, uint32_t prim, uint32_t nroots, uint32_t n, uint32_t interleave,
                       const uint8_t *data, uint64_t frames, uint8_t *out)
{
    uint8_t t[768], g[SDSP_HIP_RS_MAX_NROOTS + 1], par[SDSP_HIP_RS_MAX_NROOTS];
    if (int rc = rs_check_code(field_poly, fcr, prim, nroots, t))
        return rc;
    if (int rc = rs_check_frame(nroots, n, interleave))
        return rc;
    if (frames >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "frames must be below 2^31");
    if (frames == 0)
        return SDSP_HIP_OK;
    if (!data || !out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "data and out must not be null");
    const uint64_t k = n - nroots, I = interleave;
    if (ranges_overlap(data, frames * I * k, out, frames * I * n))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "data and out must not overlap");
    rs_generator_of(t, fcr, prim, nroots, g);
    for (uint64_t f = 0; f < frames; f++) {
        const uint8_t *d = data + f * I * k;
        uint8_t *o = out + f * I * n;
        std::memcpy(o, d, I * k);
        for (uint64_t j = 0; j < I; j++) {
            // the remainder of data(x) x^nroots by g, in a shift register
            std::memset(par, 0, sizeof(par));
            for (uint64_t s = 0; s < k; s++) {
                const uint32_t fb = d[s * I + j] ^ par[0];
                for (uint32_t c = 0; c + 1 < nroots; c++)
                    par[c] = static_cast<uint8_t>(par[c + 1] ^ rs_mul(t, fb, g[c + 1]));
                par[nroots - 1] = rs_mul(t, fb, g[nroots]);
            }
            for (uint32_t c = 0; c < nroots; c++)
                o[(k + c) * I + j] = par[c];
        }
    }
    return SDSP_HIP_OK;
}

int sdsp_hip_rs_plan_create(sdsp_hip_rs_plan **out, uint32_t field_poly, uint32_t fcr, uint32_t prim, uint32_t nroots, uint32_t n,
                            uint32_t interleave, int out_kind, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    uint8_t t[768];
    if (int rc = rs_check_code(field_poly, fcr, prim, nroots, t))
        return rc;
    if (int rc = rs_check_frame(nroots, n, interleave))
        return rc;
    if (out_kind != SDSP_HIP_RS_FULL && out_kind != SDSP_HIP_RS_DATA)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "out_kind must be SDSP_HIP_RS_FULL or SDSP_HIP_RS_DATA");
    if (int rc = use_device(device))
        return rc;
    auto *p = new sdsp_hip_rs_plan();
    p->field_poly = field_poly;
    p->fcr = fcr;
    p->prim = prim;
    p->nroots = nroots;
    p->n = n;
    p->interleave = interleave;
    p->out_kind = out_kind;
    p->device = device;
    p->variant = 0;
    hipError_t e = hipMalloc(&p->table, sizeof(t));
    if (e == hipSuccess)
        e = hipMemcpy(p->table, t, sizeof(t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        const int rc = plan_fail(e, "rs");
        sdsp_hip_rs_plan_destroy(p);
        return rc;
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_rs_plan_destroy(sdsp_hip_rs_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK)
        (void)hipFree(p->table);
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_rs_process(sdsp_hip_rs_plan *p, const void *in, const void *erasures, void *out, int32_t *corrected, uint64_t frames,
                        void *stream)
{
    if (int rc = rs_check(p, in, erasures, out, corrected, frames))
        return rc;
    if (frames == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    return launch_rs(rs_args_of(p, in, erasures, out, corrected, frames), p->variant, stream);
}

int sdsp_hip_rs_process_host(sdsp_hip_rs_plan *p, const void *host_in, const void *host_erasures, void *host_out, int32_t *host_corrected,
                             uint64_t frames)
{
    if (int rc = rs_check(p, host_in, host_erasures, host_out, host_corrected, frames))
        return rc;
    if (frames == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const bool inplace = host_in == host_out;
    const size_t cw = static_cast<size_t>(frames) * p->interleave;
    const size_t in_bytes = cw * p->n, out_bytes = cw * (p->out_kind == SDSP_HIP_RS_DATA ? p->n - p->nroots : p->n);
    host_stage st("rs", { { host_in, in_bytes, inplace },
                          { host_erasures, in_bytes, false },
                          { inplace ? nullptr : host_out, out_bytes, true },
                          { host_corrected, cw * 4, true } });
    int rc = st.in();
    if (!rc)
        rc = launch_rs(rs_args_of(p, st.dev[0], st.dev[1], inplace ? st.dev[0] : st.dev[2], static_cast<int32_t *>(st.dev[3]), frames),
                       p->variant, nullptr);
    if (!rc) {
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess)
            rc = hip_fail(e, "rs process_host");
    }
    return st.out(rc);
}

int sdsp_hip_rs_plan_set_variant(sdsp_hip_rs_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_rs_plan_launches(const sdsp_hip_rs_plan *p, uint64_t frames, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = frames ? 1 : 0;
    return SDSP_HIP_OK;
}

int sdsp_hip_rs_plan_get_info(const sdsp_hip_rs_plan *p, sdsp_hip_rs_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    const rs_shape s = rs_shape_for(p->n, p->interleave, p->variant);
    info->field_poly = p->field_poly;
    info->fcr = p->fcr;
    info->prim = p->prim;
    info->nroots = p->nroots;
    info->n = p->n;
    info->interleave = p->interleave;
    info->k = p->n - p->nroots;
    info->t = p->nroots / 2;
    info->threads = s.threads;
    info->waves = s.waves;
    info->lds_bytes = s.lds_bytes;
    info->out_kind = p->out_kind;
    info->device = p->device;
    info->variant = p->variant;
    std::strncpy(info->kernel, rs_kernel_for(p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}
// ------------------------------------------------------------------ frame synchroniser banks (fsync.hip)

namespace
{
constexpr uint32_t kFsyncRecWords = 16; // a channel's record in the state, in uint32

// the frame of a plan or of a host helper, without a device
int fsync_check_frame(uint64_t marker, uint32_t M, uint32_t P)
{
    if (M < 8 || M > 64)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "marker_bits must be in [8, 64]");
    if (P < 1 || P > SDSP_HIP_FSYNC_MAX_PAYLOAD)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "payload_bytes must be in [1, 8192]");
    if (M < 64 && (marker >> M) != 0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "the marker has bits at or above marker_bits");
    return SDSP_HIP_OK;
}

struct fsync_ws_layout {
    uint64_t rec_pos, work, hitn, hiti, rec_info, rec_cnt, bytes; // ws_seen lies at 0
};
fsync_ws_layout fsync_ws_layout_of(const sdsp_hip_fsync_plan *p)
{
    fsync_ws_layout l{};
    const uint64_t mc = p->max_channels, row = mc * p->RW * 4;
    l.rec_pos = mc * 8;
    l.work = l.rec_pos + mc * p->max_frames * 8;
    l.hitn = l.work + row;
    l.hiti = l.hitn + row;
    l.rec_info = l.hiti + row;
    l.rec_cnt = l.rec_info + mc * p->max_frames * 4;
    l.bytes = l.rec_cnt + mc * 4;
    return l;
}

uint64_t fsync_in_row(const sdsp_hip_fsync_plan *p, uint64_t nbits) { return p->in_kind == SDSP_HIP_FSYNC_PACKED ? nbits / 8 : nbits; }
uint64_t fsync_frames_of(const sdsp_hip_fsync_plan *p, uint64_t nbits) { return (nbits + p->L - 1) / p->L; }

// argument checks shared by process and process_host (device pointers or not)
int fsync_check(const sdsp_hip_fsync_plan *p, const void *in, const uint8_t *out, const uint32_t *counts, const uint64_t *pos,
                const uint32_t *info, uint64_t channels, uint64_t nbits, bool device_ptrs)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (channels > p->max_channels)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "channels must be at most the plan's max_channels");
    if (nbits > p->max_bits)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "nbits must be at most the plan's max_bits");
    if (p->in_kind == SDSP_HIP_FSYNC_PACKED && nbits % 32 != 0)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "nbits must be a multiple of 32 for packed input");
    if (channels == 0)
        return SDSP_HIP_OK;
    if (!counts || (!in && nbits))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in and counts must not be null");
    if (misaligned(counts, 4) || misaligned(info, 4) || misaligned(pos, 8) || (p->in_kind == SDSP_HIP_FSYNC_PACKED && misaligned(in, 4)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in, counts, pos and info must be aligned to their element size");
    const uint64_t mf = fsync_frames_of(p, nbits);
    const void *ptr[7] = { in, out, counts, pos, info, device_ptrs ? p->state : nullptr, device_ptrs ? p->ws : nullptr };
    const uint64_t bytes[7] = { channels * fsync_in_row(p, nbits), channels * mf * p->P, channels * 4, channels * mf * 8, channels * mf * 4,
                                p->state_bytes, p->ws_bytes };
    for (int i = 0; i < 5; i++)
        for (int j = i + 1; j < 7; j++)
            if (bytes[i] && bytes[j] && ranges_overlap(ptr[i], bytes[i], ptr[j], bytes[j]))
                return fail(SDSP_HIP_ERR_INVALID_ARG, "in, out, counts, pos, info and the plan's buffers must not overlap");
    return SDSP_HIP_OK;
}

sdsp_hip::fsync_args fsync_args_of(const sdsp_hip_fsync_plan *p, const void *in, uint8_t *out, uint32_t *counts, uint64_t *pos,
                                   uint32_t *info, uint64_t channels, uint64_t nbits)
{
    const fsync_ws_layout l = fsync_ws_layout_of(p);
    char *ws = static_cast<char *>(p->ws);
    sdsp_hip::fsync_args a{};
    a.in = in;
    a.out = out;
    a.counts = counts;
    a.pos = pos;
    a.info = info;
    a.state = static_cast<uint32_t *>(p->state);
    a.ring = a.state + p->max_channels * kFsyncRecWords;
    a.ws_seen = reinterpret_cast<uint64_t *>(ws);
    a.rec_pos = reinterpret_cast<uint64_t *>(ws + l.rec_pos);
    a.work = reinterpret_cast<uint32_t *>(ws + l.work);
    a.hitn = reinterpret_cast<uint32_t *>(ws + l.hitn);
    a.hiti = reinterpret_cast<uint32_t *>(ws + l.hiti);
    a.rec_info = reinterpret_cast<uint32_t *>(ws + l.rec_info);
    a.rec_cnt = reinterpret_cast<uint32_t *>(ws + l.rec_cnt);
    a.pnw = static_cast<const uint32_t *>(p->pn);
    a.channels = channels;
    a.nbits = nbits;
    a.maxf = fsync_frames_of(p, nbits);
    a.M = p->M;
    a.P = p->P;
    a.L = p->L;
    a.tol = p->tol;
    a.V = p->V;
    a.F = p->F;
    a.either = p->polarity == SDSP_HIP_FSYNC_EITHER ? 1 : 0;
    a.packed = p->in_kind == SDSP_HIP_FSYNC_PACKED ? 1 : 0;
    a.HW = p->HW;
    a.RW = p->RW;
    uint64_t rev = 0; // the marker with its first bit lowest
    for (uint32_t i = 0; i < p->M; i++)
        rev |= ((p->marker >> (p->M - 1 - i)) & 1ull) << i;
    a.mrev_lo = static_cast<uint32_t>(rev);
    a.mrev_hi = static_cast<uint32_t>(rev >> 32);
    return a;
}

// the work of one call on device pointers: counts alone for an empty call
int fsync_run(const sdsp_hip_fsync_plan *p, const void *in, uint8_t *out, uint32_t *counts, uint64_t *pos, uint32_t *info,
              uint64_t channels, uint64_t nbits, hipStream_t stream)
{
    if (nbits == 0) {
        const hipError_t e = hipMemsetAsync(counts, 0, channels * 4, stream);
        return e == hipSuccess ? SDSP_HIP_OK : hip_fail(e, "fsync process");
    }
    return sdsp_hip::launch_fsync(fsync_args_of(p, in, out, counts, pos, info, channels, nbits), p->variant, stream);
}
} // namespace

int sdsp_hip_fsync_ccsds_pn(uint8_t *out, uint64_t n)
{
    if (!out && n)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "out is null");
    uint32_t reg = 0xff; // a[i] in bit 7 .. a[i + 7] in bit 0
    for (uint64_t i = 0; i < n; i++) {
        uint32_t byte = 0;
        for (int b = 0; b < 8; b++) {
            byte = (byte << 1) | ((reg >> 7) & 1u);
            const uint32_t next = ((reg >> 7) ^ (reg >> 4) ^ (reg >> 2) ^ reg) & 1u;
            reg = ((reg << 1) | next) & 0xff;
        }
        out[i] = static_cast<uint8_t>(byte);
    }
    return SDSP_HIP_OK;
}

int sdsp_hip_fsync_attach(uint64_t marker, uint32_t M, uint32_t P, const uint8_t *pn, const uint8_t *frames, uint64_t nframes, int invert,
                          uint8_t *bits)
{
    if (int rc = fsync_check_frame(marker, M, P))
        return rc;
    if (nframes && (!frames || !bits))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "frames and bits must not be null");
    const uint8_t flip = invert ? 1 : 0;
    for (uint64_t f = 0; f < nframes; f++) {
        uint8_t *o = bits + f * (M + 8ull * P);
        for (uint32_t i = 0; i < M; i++)
            o[i] = static_cast<uint8_t>(((marker >> (M - 1 - i)) & 1ull) ^ flip);
        for (uint32_t i = 0; i < P; i++) {
            const uint32_t v = frames[f * P + i] ^ (pn ? pn[i] : 0);
            for (uint32_t b = 0; b < 8; b++)
                o[M + 8 * i + b] = static_cast<uint8_t>(((v >> (7 - b)) & 1u) ^ flip);
        }
    }
    return SDSP_HIP_OK;
}

int sdsp_hip_fsync_max_frames(uint32_t M, uint32_t P, uint64_t nbits, uint64_t *frames)
{
    if (!frames)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "frames is null");
    if (int rc = fsync_check_frame(0, M, P))
        return rc;
    const uint64_t L = M + 8ull * P;
    *frames = nbits / L + (nbits % L ? 1 : 0);
    return SDSP_HIP_OK;
}

int sdsp_hip_fsync_plan_create(sdsp_hip_fsync_plan **out, uint64_t marker, uint32_t M, uint32_t P, uint32_t tol, uint32_t verify,
                               uint32_t flywheel, int polarity, const uint8_t *pn, int in_kind, uint64_t max_channels, uint64_t max_bits,
                               int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    if (int rc = fsync_check_frame(marker, M, P))
        return rc;
    if (tol > 15 || tol + 1 > M / 2)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "tol must be in [0, min(15, marker_bits / 2 - 1)]");
    if (verify > 255 || flywheel > 255)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "verify and flywheel must be in [0, 255]");
    if (max_channels == 0 || max_channels >= (1ull << 31) || max_bits == 0 || max_bits >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "max_channels and max_bits must be in [1, 2^31)");
    if (polarity != SDSP_HIP_FSYNC_NORMAL && polarity != SDSP_HIP_FSYNC_EITHER)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "polarity must be SDSP_HIP_FSYNC_NORMAL or SDSP_HIP_FSYNC_EITHER");
    if (in_kind != SDSP_HIP_FSYNC_BYTES && in_kind != SDSP_HIP_FSYNC_PACKED)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_kind must be SDSP_HIP_FSYNC_BYTES or SDSP_HIP_FSYNC_PACKED");
    if (int rc = use_device(device))
        return rc;
    auto *p = new sdsp_hip_fsync_plan();
    p->marker = marker;
    p->M = M;
    p->P = P;
    p->L = M + 8 * P;
    p->tol = tol;
    p->V = verify;
    p->F = flywheel;
    p->polarity = polarity;
    p->in_kind = in_kind;
    p->max_channels = max_channels;
    p->max_bits = max_bits;
    p->max_frames = fsync_frames_of(p, max_bits);
    p->device = device;
    p->variant = 0;
    p->HW = sdsp_hip::fsync_ring_words(M, P);
    p->RW = static_cast<uint32_t>(sdsp_hip::fsync_row_words(M, P, max_bits));
    p->state_bytes = max_channels * (kFsyncRecWords + p->HW) * 4;
    p->ws_bytes = fsync_ws_layout_of(p).bytes;
    int rc = SDSP_HIP_OK;
    hipError_t e = hipMalloc(&p->state, p->state_bytes);
    if (e == hipSuccess)
        e = hipMalloc(&p->ws, p->ws_bytes);
    if (e == hipSuccess && pn) {
        std::vector<uint8_t> words((P + 3) / 4 * 4, 0);
        std::copy(pn, pn + P, words.begin());
        e = hipMalloc(&p->pn, words.size());
        if (e == hipSuccess)
            e = hipMemcpy(p->pn, words.data(), words.size(), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess)
        rc = plan_fail(e, "fsync");
    if (!rc)
        rc = sdsp_hip_fsync_plan_reset(p);
    if (rc) {
        sdsp_hip_fsync_plan_destroy(p);
        return rc;
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_fsync_plan_destroy(sdsp_hip_fsync_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK) {
        (void)hipFree(p->state);
        (void)hipFree(p->ws);
        (void)hipFree(p->pn);
    }
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_fsync_process(sdsp_hip_fsync_plan *p, const void *in, uint8_t *out, uint32_t *counts, uint64_t *pos, uint32_t *info,
                           uint64_t channels, uint64_t nbits, void *stream)
{
    if (int rc = fsync_check(p, in, out, counts, pos, info, channels, nbits, true))
        return rc;
    if (channels == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    return fsync_run(p, in, out, counts, pos, info, channels, nbits, static_cast<hipStream_t>(stream));
}

int sdsp_hip_fsync_process_host(sdsp_hip_fsync_plan *p, const void *host_in, uint8_t *host_out, uint32_t *host_counts, uint64_t *host_pos,
                                uint32_t *host_info, uint64_t channels, uint64_t nbits)
{
    if (int rc = fsync_check(p, host_in, host_out, host_counts, host_pos, host_info, channels, nbits, false))
        return rc;
    if (channels == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const size_t mf = static_cast<size_t>(fsync_frames_of(p, nbits)), ch = static_cast<size_t>(channels);
    host_stage st("fsync", { { nbits ? host_in : nullptr, ch * static_cast<size_t>(fsync_in_row(p, nbits)), false },
                             { mf ? host_out : nullptr, ch * mf * p->P, true },
                             { host_counts, ch * 4, true },
                             { mf ? host_pos : nullptr, ch * mf * 8, true },
                             { mf ? host_info : nullptr, ch * mf * 4, true } });
    int rc = st.in();
    if (!rc)
        rc = fsync_run(p, st.dev[0], static_cast<uint8_t *>(st.dev[1]), static_cast<uint32_t *>(st.dev[2]), static_cast<uint64_t *>(st.dev[3]),
                       static_cast<uint32_t *>(st.dev[4]), channels, nbits, nullptr);
    if (!rc) {
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess)
            rc = hip_fail(e, "fsync process_host");
    }
    return st.out(rc);
}

int sdsp_hip_fsync_plan_reset(sdsp_hip_fsync_plan *p)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (int rc = use_device(p->device))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(p->state, 0, p->state_bytes));
    HIP_TRY(hipDeviceSynchronize());
    return SDSP_HIP_OK;
}

int sdsp_hip_fsync_plan_get_state(sdsp_hip_fsync_plan *p, uint32_t *mode, uint64_t *next, uint32_t *polarity, uint32_t *count,
                                  uint32_t *misses, uint32_t *pending, uint64_t *seen, uint64_t channels)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (channels > p->max_channels)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "channels must be at most the plan's max_channels");
    if (channels == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint32_t> rec(static_cast<size_t>(channels) * kFsyncRecWords);
    HIP_TRY(hipMemcpy(rec.data(), p->state, rec.size() * 4, hipMemcpyDeviceToHost));
    for (uint64_t c = 0; c < channels; c++) {
        const uint32_t *r = rec.data() + c * kFsyncRecWords;
        if (mode)
            mode[c] = r[0];
        if (polarity)
            polarity[c] = r[1];
        if (count)
            count[c] = r[2];
        if (misses)
            misses[c] = r[3];
        if (pending)
            pending[c] = r[4];
        if (next)
            next[c] = r[6] | (static_cast<uint64_t>(r[7]) << 32);
        if (seen)
            seen[c] = r[8] | (static_cast<uint64_t>(r[9]) << 32);
    }
    return SDSP_HIP_OK;
}

int sdsp_hip_fsync_plan_state_bytes(const sdsp_hip_fsync_plan *p, uint64_t *bytes)
{
    if (!p || !bytes)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *bytes = p->state_bytes;
    return SDSP_HIP_OK;
}

int sdsp_hip_fsync_plan_set_variant(sdsp_hip_fsync_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_fsync_plan_launches(const sdsp_hip_fsync_plan *p, uint64_t channels, uint64_t nbits, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    *launches = channels && nbits ? sdsp_hip::fsync_launches(p->variant) : 0;
    return SDSP_HIP_OK;
}

int sdsp_hip_fsync_plan_get_info(const sdsp_hip_fsync_plan *p, sdsp_hip_fsync_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->marker = p->marker;
    info->marker_bits = p->M;
    info->payload_bytes = p->P;
    info->period = p->L;
    info->tol = p->tol;
    info->verify = p->V;
    info->flywheel = p->F;
    info->ring_words = p->HW;
    info->row_words = p->RW;
    info->has_pn = p->pn ? 1 : 0;
    info->max_channels = p->max_channels;
    info->max_bits = p->max_bits;
    info->max_frames = p->max_frames;
    info->state_bytes = p->state_bytes;
    info->workspace_bytes = p->ws_bytes;
    info->polarity = p->polarity;
    info->in_kind = p->in_kind;
    info->device = p->device;
    info->variant = p->variant;
    std::strncpy(info->kernel, sdsp_hip::fsync_kernel_for(p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}
// ------------------------------------------------------------------ LDPC decoder banks (ldpc.hip)

namespace
{
// the code of a plan or of a host helper, without a device; counts (nullable): the entries of H's base and the largest row degree
int ldpc_check_code(const int16_t *base, uint32_t mb, uint32_t nb, uint32_t z, uint32_t *entries, uint32_t *max_degree)
{
    if (z < 2 || z > SDSP_HIP_LDPC_MAX_Z)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "z must be in [2, 512]");
    if (mb < 1 || mb > SDSP_HIP_LDPC_MAX_MB)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "mb must be in [1, 64]");
    if (nb <= mb || nb > SDSP_HIP_LDPC_MAX_NB)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "nb must be in (mb, 128]");
    if (nb * z > SDSP_HIP_LDPC_MAX_N)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "n = nb z must be at most 16384");
    if (!base)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "base is null");
    uint32_t in_column[SDSP_HIP_LDPC_MAX_NB] = {}, total = 0, deepest = 0;
    for (uint32_t r = 0; r < mb; r++) {
        uint32_t d = 0;
        for (uint32_t c = 0; c < nb; c++) {
            const int s = base[r * nb + c];
            if (s < -1 || s >= static_cast<int>(z))
                return fail(SDSP_HIP_ERR_INVALID_ARG, "a shift must be -1 or in [0, z)");
            if (s >= 0) {
                d++;
                in_column[c]++;
            }
        }
        if (d < 2 || d > SDSP_HIP_LDPC_MAX_ROW_DEGREE)
            return fail(SDSP_HIP_ERR_INVALID_ARG, "every row must have 2 to 32 entries");
        total += d;
        deepest = std::max(deepest, d);
    }
    for (uint32_t c = 0; c < nb; c++)
        if (!in_column[c])
            return fail(SDSP_HIP_ERR_INVALID_ARG, "every column must have at least one entry");
    if (entries)
        *entries = total;
    if (max_degree)
        *max_degree = deepest;
    return SDSP_HIP_OK;
}

// P of a checked code: m rows of ceil(k / 32) words.  The rows of H as [parity part | data part] bit words, the parity part reduced
// to the identity by Gauss-Jordan elimination: what is left of the data part is P.
int ldpc_parity_rows(const int16_t *base, uint32_t mb, uint32_t nb, uint32_t z, std::vector<uint32_t> &P)
{
    const uint32_t n = nb * z, m = mb * z, k = n - m, wp = (m + 31) / 32, wk = (k + 31) / 32, W = wp + wk;
    std::vector<uint32_t> rows(static_cast<size_t>(m) * W, 0);
    for (uint32_t r = 0; r < mb; r++)
        for (uint32_t c = 0; c < nb; c++) {
            const int s = base[r * nb + c];
            if (s < 0)
                continue;
            for (uint32_t i = 0; i < z; i++) {
                const uint32_t v = c * z + (i + static_cast<uint32_t>(s)) % z;
                uint32_t *row = rows.data() + static_cast<size_t>(r * z + i) * W;
                if (v >= k)
                    row[(v - k) / 32] ^= 1u << ((v - k) % 32);
                else
                    row[wp + v / 32] ^= 1u << (v % 32);
            }
        }
    for (uint32_t q = 0; q < m; q++) {
        const uint32_t w = q / 32, bit = 1u << (q % 32);
        uint32_t piv = q;
        while (piv < m && !(rows[static_cast<size_t>(piv) * W + w] & bit))
            piv++;
        if (piv == m)
            return fail(SDSP_HIP_ERR_UNSUPPORTED, "the last m columns of H are singular: the code has no [data | parity] encoder");
        uint32_t *pr = rows.data() + static_cast<size_t>(q) * W;
        if (piv != q)
            std::swap_ranges(pr, pr + W, rows.data() + static_cast<size_t>(piv) * W);
        for (uint32_t i = 0; i < m; i++) {
            uint32_t *row = rows.data() + static_cast<size_t>(i) * W;
            if (i != q && (row[w] & bit))
                for (uint32_t x = w; x < W; x++) // the pivot row is zero in front of word w
                    row[x] ^= pr[x];
        }
    }
    P.assign(static_cast<size_t>(m) * wk, 0);
    for (uint32_t i = 0; i < m; i++)
        std::memcpy(P.data() + static_cast<size_t>(i) * wk, rows.data() + static_cast<size_t>(i) * W + wp, wk * 4);
    return SDSP_HIP_OK;
}

uint64_t ldpc_bits_row(const sdsp_hip_ldpc_plan *p) { return p->out_kind == SDSP_HIP_LDPC_PACKED ? (p->out_bits + 31) / 32 * 4ull : p->out_bits; }
uint64_t ldpc_in_row(const sdsp_hip_ldpc_plan *p) { return static_cast<uint64_t>(p->n) * (p->in_kind == SDSP_HIP_LDPC_F32 ? 4 : 1); }

// argument checks shared by process and process_host
int ldpc_check(const sdsp_hip_ldpc_plan *p, const void *llr, const void *bits, const int16_t *post, const int32_t *status, uint64_t codewords,
               uint32_t max_iter)
{
    if (!p)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan is null");
    if (codewords >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "codewords must be below 2^31");
    if (max_iter > SDSP_HIP_LDPC_MAX_ITER)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "max_iter must be in [0, 255]");
    if (codewords == 0)
        return SDSP_HIP_OK;
    if (!llr)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "llr must not be null");
    if (!bits && !post && !status)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "at least one of bits, post and status is required");
    if ((p->in_kind == SDSP_HIP_LDPC_F32 && misaligned(llr, 4)) || (p->out_kind == SDSP_HIP_LDPC_PACKED && misaligned(bits, 4)) ||
        misaligned(post, 2) || misaligned(status, 4))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "llr, bits, post and status must be aligned to their element size");
    const uint64_t nl = codewords * ldpc_in_row(p), nb = codewords * ldpc_bits_row(p), np = codewords * p->n * 2, ns = codewords * 4;
    if (ranges_overlap(llr, nl, bits, nb) || ranges_overlap(llr, nl, post, np) || ranges_overlap(llr, nl, status, ns) ||
        ranges_overlap(bits, nb, post, np) || ranges_overlap(bits, nb, status, ns) || ranges_overlap(post, np, status, ns))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "llr, bits, post and status must not overlap");
    return SDSP_HIP_OK;
}

ldpc_args ldpc_args_of(const sdsp_hip_ldpc_plan *p, const void *llr, void *bits, int16_t *post, int32_t *status, uint64_t codewords,
                       uint32_t max_iter)
{
    ldpc_args a{};
    a.llr = llr;
    a.bits = bits;
    a.post = post;
    a.status = status;
    a.table = p->table;
    a.table_entries_at = p->entries_at;
    a.workspace = p->ws;
    a.codewords = codewords;
    a.mb = p->mb;
    a.nb = p->nb;
    a.z = p->z;
    a.edges = p->entries * p->z;
    a.norm = p->norm;
    a.beta = p->beta;
    a.max_iter = max_iter;
    a.out_bits = p->out_bits;
    a.early_stop = p->early_stop != 0;
    a.packed = p->out_kind == SDSP_HIP_LDPC_PACKED;
    a.f32 = p->in_kind == SDSP_HIP_LDPC_F32;
    a.scale = p->scale;
    return a;
}

ldpc_shape ldpc_shape_of(const sdsp_hip_ldpc_plan *p, int variant) { return ldpc_shape_for(p->mb, p->nb, p->z, p->entries * p->z, variant); }
} // namespace

int sdsp_hip_ldpc_parity_matrix(const int16_t *base, uint32_t mb, uint32_t nb, uint32_t z, uint32_t *P)
{
    if (int rc = ldpc_check_code(base, mb, nb, z, nullptr, nullptr))
        return rc;
    if (!P)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "P is null");
    std::vector<uint32_t> rows;
    if (int rc = ldpc_parity_rows(base, mb, nb, z, rows))
        return rc;
    std::memcpy(P, rows.data(), rows.size() * 4);
    return SDSP_HIP_OK;
}

int sdsp_hip_ldpc_encode(const int16_t *base, uint32_t mb, uint32_t nb, uint32_t z, const uint8_t *data, uint64_t codewords, uint8_t *out)
{
    if (int rc = ldpc_check_code(base, mb, nb, z, nullptr, nullptr))
        return rc;
    if (codewords >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "codewords must be below 2^31");
    if (codewords == 0)
        return SDSP_HIP_OK;
    if (!data || !out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "data and out must not be null");
    const uint32_t n = nb * z, m = mb * z, k = n - m, wk = (k + 31) / 32;
    if (ranges_overlap(data, codewords * k, out, codewords * n))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "data and out must not overlap");
    std::vector<uint32_t> P;
    if (int rc = ldpc_parity_rows(base, mb, nb, z, P))
        return rc;
    std::vector<uint32_t> word(wk);
    for (uint64_t f = 0; f < codewords; f++) {
        const uint8_t *d = data + f * k;
        uint8_t *o = out + f * n;
        std::fill(word.begin(), word.end(), 0u);
        for (uint32_t j = 0; j < k; j++) {
            o[j] = d[j] != 0;
            word[j / 32] |= static_cast<uint32_t>(d[j] != 0) << (j % 32);
        }
        for (uint32_t i = 0; i < m; i++) {
            uint32_t acc = 0;
            for (uint32_t w = 0; w < wk; w++)
                acc ^= P[static_cast<size_t>(i) * wk + w] & word[w];
            o[k + i] = static_cast<uint8_t>(__builtin_popcount(acc) & 1);
        }
    }
    return SDSP_HIP_OK;
}

int sdsp_hip_ldpc_plan_create(sdsp_hip_ldpc_plan **out, const int16_t *base, uint32_t mb, uint32_t nb, uint32_t z, uint32_t norm,
                              uint32_t beta, int early_stop, int in_kind, float scale, int out_kind, uint32_t out_bits, int device)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "plan out-pointer is null");
    *out = nullptr;
    uint32_t entries = 0, max_degree = 0;
    if (int rc = ldpc_check_code(base, mb, nb, z, &entries, &max_degree))
        return rc;
    if (norm < 1 || norm > 16)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "norm must be in [1, 16]");
    if (beta > 31)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "beta must be in [0, 31]");
    if (out_bits < 1 || out_bits > nb * z)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "out_bits must be in [1, n]");
    if (in_kind != SDSP_HIP_LDPC_I8 && in_kind != SDSP_HIP_LDPC_F32)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "in_kind must be SDSP_HIP_LDPC_I8 or SDSP_HIP_LDPC_F32");
    if (out_kind != SDSP_HIP_LDPC_BYTES && out_kind != SDSP_HIP_LDPC_PACKED)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "out_kind must be SDSP_HIP_LDPC_BYTES or SDSP_HIP_LDPC_PACKED");
    if (in_kind == SDSP_HIP_LDPC_F32 && !(std::isfinite(scale) && scale > 0.0f))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "scale must be finite and positive");
    if (int rc = use_device(device))
        return rc;
    auto *p = new sdsp_hip_ldpc_plan();
    p->mb = mb;
    p->nb = nb;
    p->z = z;
    p->n = nb * z;
    p->m = mb * z;
    p->entries = entries;
    p->entries_at = (mb + 2) & ~1u;
    p->max_degree = max_degree;
    p->norm = norm;
    p->beta = beta;
    p->out_bits = out_bits;
    p->scale = in_kind == SDSP_HIP_LDPC_F32 ? scale : 1.0f;
    p->early_stop = early_stop ? 1 : 0;
    p->in_kind = in_kind;
    p->out_kind = out_kind;
    p->device = device;
    p->variant = 0;
    std::vector<uint32_t> t(p->entries_at + 2 * static_cast<size_t>(entries), 0);
    uint32_t e = 0;
    for (uint32_t r = 0; r < mb; r++) {
        t[r] = e;
        for (uint32_t c = 0; c < nb; c++)
            if (base[r * nb + c] >= 0) {
                t[p->entries_at + 2 * e] = c * z;
                t[p->entries_at + 2 * e + 1] = static_cast<uint32_t>(base[r * nb + c]);
                e++;
            }
    }
    t[mb] = e;
    hipError_t err = hipMalloc(&p->table, t.size() * 4);
    if (err == hipSuccess)
        err = hipMemcpy(p->table, t.data(), t.size() * 4, hipMemcpyHostToDevice);
    int rc = err == hipSuccess ? SDSP_HIP_OK : plan_fail(err, "ldpc");
    if (!rc)
        rc = ldpc_prepare(in_kind, ldpc_shape_of(p, 0).lds_bytes);
    if (rc) {
        sdsp_hip_ldpc_plan_destroy(p);
        return rc;
    }
    *out = p;
    return SDSP_HIP_OK;
}

int sdsp_hip_ldpc_plan_destroy(sdsp_hip_ldpc_plan *p)
{
    if (!p)
        return SDSP_HIP_OK;
    if (use_device(p->device) == SDSP_HIP_OK) {
        (void)hipFree(p->table);
        (void)hipFree(p->ws);
    }
    delete p;
    return SDSP_HIP_OK;
}

int sdsp_hip_ldpc_process(sdsp_hip_ldpc_plan *p, const void *llr, void *bits, int16_t *post, int32_t *status, uint64_t codewords,
                          uint32_t max_iter, void *stream)
{
    if (int rc = ldpc_check(p, llr, bits, post, status, codewords, max_iter))
        return rc;
    if (codewords == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    return launch_ldpc(ldpc_args_of(p, llr, bits, post, status, codewords, max_iter), p->variant, stream);
}

int sdsp_hip_ldpc_process_host(sdsp_hip_ldpc_plan *p, const void *host_llr, void *host_bits, int16_t *host_post, int32_t *host_status,
                               uint64_t codewords, uint32_t max_iter)
{
    if (int rc = ldpc_check(p, host_llr, host_bits, host_post, host_status, codewords, max_iter))
        return rc;
    if (codewords == 0)
        return SDSP_HIP_OK;
    if (int rc = use_device(p->device))
        return rc;
    const size_t cw = static_cast<size_t>(codewords);
    host_stage st("ldpc", { { host_llr, cw * ldpc_in_row(p), false },
                            { host_bits, cw * ldpc_bits_row(p), true },
                            { host_post, cw * p->n * 2, true },
                            { host_status, cw * 4, true } });
    int rc = st.in();
    if (!rc)
        rc = launch_ldpc(ldpc_args_of(p, st.dev[0], st.dev[1], static_cast<int16_t *>(st.dev[2]), static_cast<int32_t *>(st.dev[3]), codewords,
                                      max_iter),
                         p->variant, nullptr);
    if (!rc) {
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess)
            rc = hip_fail(e, "ldpc process_host");
    }
    return st.out(rc);
}

int sdsp_hip_ldpc_plan_set_variant(sdsp_hip_ldpc_plan *p, int variant)
{
    if (!p || variant < 0 || variant > 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "variant must be 0 or 1");
    if (variant == 1 && !p->ws) {
        if (int rc = use_device(p->device))
            return rc;
        const hipError_t e = hipMalloc(&p->ws, ldpc_shape_of(p, 1).workspace_bytes);
        if (e != hipSuccess) {
            p->ws = nullptr;
            return plan_fail(e, "ldpc");
        }
    }
    p->variant = variant;
    return SDSP_HIP_OK;
}

int sdsp_hip_ldpc_plan_launches(const sdsp_hip_ldpc_plan *p, uint64_t codewords, uint64_t *launches)
{
    if (!p || !launches)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    const uint64_t piece = ldpc_shape_of(p, p->variant).piece;
    *launches = (codewords + piece - 1) / piece;
    return SDSP_HIP_OK;
}

int sdsp_hip_ldpc_plan_get_info(const sdsp_hip_ldpc_plan *p, sdsp_hip_ldpc_plan_info *info)
{
    if (!p || !info)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    const ldpc_shape s = ldpc_shape_of(p, p->variant);
    info->mb = p->mb;
    info->nb = p->nb;
    info->z = p->z;
    info->n = p->n;
    info->m = p->m;
    info->edges = p->entries * p->z;
    info->max_row_degree = p->max_degree;
    info->norm = p->norm;
    info->beta = p->beta;
    info->out_bits = p->out_bits;
    info->group = s.group;
    info->threads = s.threads;
    info->lds_bytes = s.lds_bytes;
    info->codewords_per_cu = s.per_cu;
    info->piece = p->variant == 1 ? s.piece : 0;
    info->workspace_bytes = s.workspace_bytes;
    info->scale = p->scale;
    info->early_stop = p->early_stop;
    info->in_kind = p->in_kind;
    info->out_kind = p->out_kind;
    info->device = p->device;
    info->variant = p->variant;
    std::strncpy(info->kernel, ldpc_kernel_for(p->variant), sizeof(info->kernel) - 1);
    return SDSP_HIP_OK;
}
}
