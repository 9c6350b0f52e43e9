// pll.hip -- carrier-recovery PLL / Costas loop banks for MI355X (gfx950): many independent second-order loops on interleaved I/Q rows,
// each a 32-bit numerically controlled oscillator, a phase detector and a proportional-plus-integral loop filter.
//
// Sample n of a channel (theta: the uint32 phase, integ: the integrator), in this order:
//     w = C[theta >> 21] (x) F[(theta >> 10) & 0x7ff]                       the oscillator, from two tables of 2048 unit vectors
//     y = x[n] (x) w                                                        (x): four products, a difference and a sum, each rounded
//     e = yi | yr yi | flip(yi, yr) - flip(yr, yi)                          CROSS | BPSK | QPSK (flip(v, s): v's sign bit xor s's)
//     integ = ma(beta, e, integ), clamped to +-max_dev;  v = ma(alpha, e, integ)     ma: one fmaf in f32, a multiply then an add in f64
//     theta += fcw0 + rint(clamp(v 2^32))                                   mod 2^32; a NaN advances by fcw0 alone
// Built with -ffp-contract=off and without fast-math, so nothing here contracts.  DESIGN.md section 5.28.
//
// Two kernels:
//   sdsp_pll_kernel        variant 0.  A workgroup of WAVES waves; each wave owns 64 channels, one lane per channel, and walks the whole
//                          call in blocks of B samples with theta and integ in registers from the first sample to the last.  Both
//                          oscillator tables are staged into LDS once per workgroup and shared by its waves: the two gathers of a
//                          sample are LDS reads, independent of each other.  The rows are channel-major, so a block of x goes through
//                          the wave's own LDS tile on its way in ([time][lane], a pitch of 65 elements) and y, err and freq on their way
//                          out: 16-byte nontemporal accesses where a row is 16-byte aligned, neighbouring lanes on one row; element by
//                          element otherwise.  y[n] takes x[n]'s place in the tile, so y may be x itself.  The next block's global loads
//                          are in flight while the current one computes.
//   sdsp_pll_plain_kernel  variant 1: one thread per channel straight from global memory, the tables read from global memory, the
//                          state read-modify-written once per sample.  The independent cross-check.
#include "stream_dev.h"

#include <atomic>
#include <type_traits>

namespace sdsp_hip
{
namespace
{
constexpr int kLanes = 64;         // one lane per channel
constexpr int kPitch = kLanes + 1; // elements between two rows of a tile: the transposing accesses spread over the banks
constexpr int kTable = 2048;       // entries of each oscillator table

template <typename R> __device__ __forceinline__ R ma(R a, R b, R c);
template <> __device__ __forceinline__ float ma<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
template <> __device__ __forceinline__ double ma<double>(double a, double b, double c) { return a * b + c; }

// a (x) b: four products, one difference and one sum, each rounded (the file is built without contraction)
template <typename E> __device__ __forceinline__ E cmul(E a, E b)
{
    E r;
    r.x = a.x * b.x - a.y * b.y;
    r.y = a.x * b.y + a.y * b.x;
    return r;
}

// v with its sign bit flipped where the sign bit of s is set
__device__ __forceinline__ float flip_sign(float v, float s)
{
    return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, v) ^ (__builtin_bit_cast(uint32_t, s) & 0x80000000u));
}
__device__ __forceinline__ double flip_sign(double v, double s)
{
    return __builtin_bit_cast(double, __builtin_bit_cast(uint64_t, v) ^ (__builtin_bit_cast(uint64_t, s) & 0x8000000000000000ull));
}

template <typename R> struct advance_limits;
template <> struct advance_limits<float> {
    static constexpr float lo = -2147483648.0f, hi = 2147483520.0f; // 2^31 - 128: the largest float below 2^31
};
template <> struct advance_limits<double> {
    static constexpr double lo = -2147483648.0, hi = 2147483647.0;
};
__device__ __forceinline__ float round_even(float t) { return __builtin_rintf(t); }
__device__ __forceinline__ double round_even(double t) { return __builtin_rint(t); }

// steps 2 to 5 of the contract for one sample: x and the oscillator value in, y and e out, integ and theta moved on
template <typename R, int MODE>
__device__ __forceinline__ void loop_step(typename cplx_pair<R>::type x, typename cplx_pair<R>::type w, R alpha, R beta, R max_dev,
                                          uint32_t fcw, typename cplx_pair<R>::type &y, R &e, R &integ, uint32_t &theta)
{
    y = cmul(x, w);
    if constexpr (MODE == SDSP_HIP_PLL_CROSS)
        e = y.y;
    else if constexpr (MODE == SDSP_HIP_PLL_BPSK)
        e = y.x * y.y;
    else
        e = flip_sign(y.y, y.x) - flip_sign(y.x, y.y);
    integ = ma<R>(beta, e, integ);
    integ = integ < -max_dev ? -max_dev : (integ > max_dev ? max_dev : integ); // a NaN stays
    const R v = ma<R>(alpha, e, integ);
    R t = v * R(4294967296.0);
    t = t < advance_limits<R>::lo ? advance_limits<R>::lo : (t > advance_limits<R>::hi ? advance_limits<R>::hi : t);
    t = t == t ? t : R(0); // a NaN advances by fcw alone
    theta += fcw + static_cast<uint32_t>(static_cast<int32_t>(round_even(t)));
}

struct pll_kargs {
    const void *x;
    void *y, *err, *freq;  // nullable
    void *integ;           // channels reals, nullable for variant 0 (zero state, nothing kept)
    uint32_t *theta;       // channels words, null with integ
    const uint32_t *fcw0;  // channels words
    const void *osc;       // C then F: 2 x 2048 complex values of the precision
    uint64_t channels, samples, x_stride, y_stride, err_stride, freq_stride;
    double alpha, beta, max_dev; // exactly representable in the plan precision
};

// the 16-byte chunks of a [64 channels][B samples] tile of elements E (NR reals each): chunk q = i * 64 + lane covers channel q / CPR,
// elements (q % CPR) * EL ..; in LDS sample i of the block is row i
template <typename R, typename E, int B> struct tile {
    using V = typename vec16<R>::type;
    static constexpr int NR = sizeof(E) / sizeof(R); // reals per element
    static constexpr int EL = 16 / sizeof(E);        // elements per chunk
    static constexpr int CPR = B / EL;               // chunks per channel and block = chunks per lane
    static_assert(B % EL == 0 && CPR >= 1, "a block is a whole number of 16-byte chunks");

    static __device__ __forceinline__ E get(const V &v, int e)
    {
        if constexpr (NR == 2) {
            E s;
            s.x = v[2 * e];
            s.y = v[2 * e + 1];
            return s;
        } else {
            return v[e];
        }
    }
    static __device__ __forceinline__ void put(V &v, int e, E s)
    {
        if constexpr (NR == 2) {
            v[2 * e] = s.x;
            v[2 * e + 1] = s.y;
        } else {
            v[e] = s;
        }
    }

    // block [n0, n0 + B) of the rows at `base` into registers; what lies past the row's samples or the bank's channels is zero
    static __device__ __forceinline__ void load(const E *base, uint64_t stride, uint64_t c0, uint64_t channels, uint64_t n0,
                                                uint64_t samples, uint32_t lane, V (&v)[CPR])
    {
#pragma unroll
        for (int i = 0; i < CPR; i++) {
            const uint32_t q = static_cast<uint32_t>(i) * kLanes + lane, ch = q / CPR, k = q % CPR;
            const uint64_t c = c0 + ch, n = n0 + static_cast<uint64_t>(k) * EL;
            V r;
#pragma unroll
            for (int j = 0; j < vec16<R>::lanes; j++)
                r[j] = R(0);
            if (c < channels && n < samples) {
                const E *p = base + c * stride + n;
                if (n + EL <= samples && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
                    r = __builtin_nontemporal_load(reinterpret_cast<const V *>(p));
                } else {
#pragma unroll
                    for (int e = 0; e < EL; e++)
                        if (n + e < samples)
                            put(r, e, p[e]);
                }
            }
            v[i] = r;
        }
    }

    // registers -> LDS
    static __device__ __forceinline__ void to_lds(E *rows, uint32_t lane, const V (&v)[CPR])
    {
#pragma unroll
        for (int i = 0; i < CPR; i++) {
            const uint32_t q = static_cast<uint32_t>(i) * kLanes + lane, ch = q / CPR, k = q % CPR;
#pragma unroll
            for (int e = 0; e < EL; e++)
                rows[(k * EL + e) * kPitch + ch] = get(v[i], e);
        }
    }

    // LDS rows -> the first `len` samples of block n0 of the rows at `base`
    static __device__ __forceinline__ void store(const E *rows, E *base, uint64_t stride, uint64_t c0, uint64_t channels, uint64_t n0,
                                                 uint32_t len, uint32_t lane)
    {
#pragma unroll
        for (int i = 0; i < CPR; i++) {
            const uint32_t q = static_cast<uint32_t>(i) * kLanes + lane, ch = q / CPR, k = q % CPR;
            const uint64_t c = c0 + ch;
            if (c >= channels || k * EL >= len)
                continue;
            E *p = base + c * stride + n0 + static_cast<uint64_t>(k) * EL;
            if (k * EL + EL <= len && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
                V r;
#pragma unroll
                for (int e = 0; e < EL; e++)
                    put(r, e, rows[(k * EL + e) * kPitch + ch]);
                __builtin_nontemporal_store(r, reinterpret_cast<V *>(p));
            } else {
#pragma unroll
                for (int e = 0; e < EL; e++)
                    if (k * EL + e < len)
                        __builtin_nontemporal_store(rows[(k * EL + e) * kPitch + ch], p + e);
            }
        }
    }
};

// What was chosen and why.  The block length sets the piece in which a row is read and written: B samples
// of y are 8 (f32) or 16 (f64) bytes each, B reals of err and freq half that.  Measured in f32 with 4 waves per workgroup: blocks
// of 16 samples (128-byte pieces of y, 64-byte pieces of err and freq; 32 KiB of tables + 4 x 16640 B = 99328 B, one workgroup and
// one wave per SIMD on a CU) take 0.61 to 0.75 of the time of blocks of 8 with y only and 0.36 to 0.39 with all outputs, although
// blocks of 8 let two workgroups share a CU: whole cache lines matter more here than resident waves.  4 waves keep 65536 channels
// at one workgroup for each of the 256 CUs.  f64: one workgroup fits beside 64 KiB of tables either way, and 4 waves with blocks of
// 8 samples (128-byte pieces of y; 64 KiB + 4 x 16640 B = 132096 B) take 0.69 to 0.77 of the time of 8 waves with blocks of 4 with y
// only and 0.38 to 0.45 with all outputs.  The overrides are for block-length experiments at build time.
#ifndef SDSP_PLL_BLOCK_F32
#define SDSP_PLL_BLOCK_F32 16
#endif
#ifndef SDSP_PLL_BLOCK_F64
#define SDSP_PLL_BLOCK_F64 8
#endif
#ifndef SDSP_PLL_WAVES_F64
#define SDSP_PLL_WAVES_F64 4
#endif
template <typename R> struct shape_of;
template <> struct shape_of<float> {
    static constexpr int waves = 4, block = SDSP_PLL_BLOCK_F32;
};
template <> struct shape_of<double> {
    static constexpr int waves = SDSP_PLL_WAVES_F64, block = SDSP_PLL_BLOCK_F64;
};
template <typename R> constexpr size_t wave_tile_bytes() { return static_cast<size_t>(shape_of<R>::block) * kPitch * 4 * sizeof(R); }
template <typename R> constexpr size_t lds_bytes_of()
{
    return 2 * kTable * 2 * sizeof(R) + shape_of<R>::waves * wave_tile_bytes<R>();
}

template <typename R, int MODE> __global__ __launch_bounds__(shape_of<R>::waves *kLanes) void sdsp_pll_kernel(pll_kargs a)
{
    using E = typename cplx_pair<R>::type;
    constexpr int B = shape_of<R>::block, WAVES = shape_of<R>::waves;
    using TC = tile<R, E, B>;
    using TR = tile<R, R, B>;
    using V = typename vec16<R>::type;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const uint32_t lane = threadIdx.x % kLanes, wave = threadIdx.x / kLanes;
    // the tables: C then F, as they lie in a.osc
    E *const tab = reinterpret_cast<E *>(lds_raw);
    {
        constexpr int NV = 2 * kTable * static_cast<int>(sizeof(E)) / 16;
        const V *src = static_cast<const V *>(a.osc);
        V *dst = reinterpret_cast<V *>(lds_raw);
        for (int i = threadIdx.x; i < NV; i += WAVES * kLanes)
            dst[i] = src[i];
    }
    const E *const ctab = tab, *const ftab = tab + kTable;
    // the wave's own tile: B rows of x (y takes their place), then B rows of err, then B rows of freq
    unsigned char *const mine = lds_raw + 2 * kTable * sizeof(E) + wave * wave_tile_bytes<R>();
    E *const xw = reinterpret_cast<E *>(mine);
    R *const ew = reinterpret_cast<R *>(xw + B * kPitch);
    R *const fw = ew + B * kPitch;
    const uint64_t c0 = (static_cast<uint64_t>(blockIdx.x) * WAVES + wave) * kLanes, c = c0 + lane;
    const bool have = c < a.channels;
    const R alpha = static_cast<R>(a.alpha), beta = static_cast<R>(a.beta), max_dev = static_cast<R>(a.max_dev);
    const E *xg = static_cast<const E *>(a.x);

    V xv[TC::CPR];
    TC::load(xg, a.x_stride, c0, a.channels, 0, a.samples, lane, xv);
    R integ = have && a.integ ? static_cast<const R *>(a.integ)[c] : R(0);
    uint32_t theta = have && a.integ ? a.theta[c] : 0u;
    const uint32_t fcw = have ? a.fcw0[c] : 0u;

    const uint64_t nblk = (a.samples + B - 1) / B;
    for (uint64_t blk = 0; blk < nblk; blk++) {
        const uint64_t n0 = blk * B;
        const uint32_t len = a.samples - n0 < static_cast<uint64_t>(B) ? static_cast<uint32_t>(a.samples - n0) : B;
        TC::to_lds(xw, lane, xv);
        __syncthreads(); // the tile is whole (and, the first time, the tables)
        if (blk + 1 < nblk)
            TC::load(xg, a.x_stride, c0, a.channels, n0 + B, a.samples, lane, xv);
        // the lane's own column from here to the barrier
        for (uint32_t n = 0; n < len; n++) {
            const E cw = ctab[theta >> 21], fv = ftab[(theta >> 10) & 0x7ffu];
            E y;
            R e;
            loop_step<R, MODE>(xw[n * kPitch + lane], cmul(cw, fv), alpha, beta, max_dev, fcw, y, e, integ, theta);
            xw[n * kPitch + lane] = y;
            if (a.err)
                ew[n * kPitch + lane] = e;
            if (a.freq)
                fw[n * kPitch + lane] = integ;
        }
        __syncthreads();
        if (a.y)
            TC::store(xw, static_cast<E *>(a.y), a.y_stride, c0, a.channels, n0, len, lane);
        if (a.err)
            TR::store(ew, static_cast<R *>(a.err), a.err_stride, c0, a.channels, n0, len, lane);
        if (a.freq)
            TR::store(fw, static_cast<R *>(a.freq), a.freq_stride, c0, a.channels, n0, len, lane);
        __syncthreads(); // the tile is free again
    }
    if (have && a.integ) {
        static_cast<R *>(a.integ)[c] = integ;
        a.theta[c] = theta;
    }
}

// ---- variant 1: one thread per channel from global memory, the state read-modify-written ---------------------------------------------
template <typename R, int MODE> __global__ __launch_bounds__(kThreads) void sdsp_pll_plain_kernel(pll_kargs a)
{
    using E = typename cplx_pair<R>::type;
    const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (c >= a.channels)
        return;
    const R alpha = static_cast<R>(a.alpha), beta = static_cast<R>(a.beta), max_dev = static_cast<R>(a.max_dev);
    const E *osc = static_cast<const E *>(a.osc);
    const E *x = static_cast<const E *>(a.x) + c * a.x_stride;
    E *y = a.y ? static_cast<E *>(a.y) + c * a.y_stride : nullptr;
    R *err = a.err ? static_cast<R *>(a.err) + c * a.err_stride : nullptr;
    R *freq = a.freq ? static_cast<R *>(a.freq) + c * a.freq_stride : nullptr;
    volatile R *integ_p = static_cast<R *>(a.integ) + c; // volatile: every sample goes through memory
    volatile uint32_t *theta_p = a.theta + c;
    const uint32_t fcw = a.fcw0[c];
    for (uint64_t n = 0; n < a.samples; n++) {
        R integ = *integ_p, e;
        uint32_t theta = *theta_p;
        E yv;
        const E w = cmul(osc[theta >> 21], osc[kTable + ((theta >> 10) & 0x7ffu)]);
        loop_step<R, MODE>(x[n], w, alpha, beta, max_dev, fcw, yv, e, integ, theta);
        *integ_p = integ;
        *theta_p = theta;
        if (y)
            y[n] = yv;
        if (err)
            err[n] = e;
        if (freq)
            freq[n] = integ;
    }
}

// f(R(), mode constant)
template <typename F> int with_kernel(int precision, int mode, F f)
{
    auto by_mode = [&](auto r) {
        switch (mode) {
        case SDSP_HIP_PLL_CROSS:
            return f(r, std::integral_constant<int, SDSP_HIP_PLL_CROSS>());
        case SDSP_HIP_PLL_BPSK:
            return f(r, std::integral_constant<int, SDSP_HIP_PLL_BPSK>());
        default:
            return f(r, std::integral_constant<int, SDSP_HIP_PLL_QPSK>());
        }
    };
    return precision == SDSP_HIP_F64 ? by_mode(double()) : by_mode(float());
}
} // namespace

uint32_t pll_block(int precision) { return precision == SDSP_HIP_F64 ? shape_of<double>::block : shape_of<float>::block; }

uint32_t pll_waves(int precision) { return precision == SDSP_HIP_F64 ? shape_of<double>::waves : shape_of<float>::waves; }

uint32_t pll_lds_bytes(int precision)
{
    return static_cast<uint32_t>(precision == SDSP_HIP_F64 ? lds_bytes_of<double>() : lds_bytes_of<float>());
}

const char *pll_kernel_for(int variant) { return variant == 1 ? "sdsp_pll_plain_kernel" : "sdsp_pll_kernel"; }

int launch_pll(int precision, const pll_args &pa, int variant, void *stream_v)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    pll_kargs k{};
    k.x = pa.x;
    k.y = pa.y;
    k.err = pa.err;
    k.freq = pa.freq;
    k.integ = pa.integ;
    k.theta = pa.theta;
    k.fcw0 = pa.fcw0;
    k.osc = pa.osc;
    k.channels = pa.channels;
    k.samples = pa.samples;
    k.x_stride = pa.x_stride;
    k.y_stride = pa.y_stride;
    k.err_stride = pa.err_stride;
    k.freq_stride = pa.freq_stride;
    k.alpha = pa.alpha;
    k.beta = pa.beta;
    k.max_dev = pa.max_dev;
    dim3 grid;
    if (variant == 1) {
        if (!k.integ || !k.theta)
            return fail(SDSP_HIP_ERR_INVALID_ARG, "pll: the plain kernel needs a state buffer");
        if (int rc = grid_for(pa.channels, "pll", &grid))
            return rc;
        with_kernel(precision, pa.mode, [&](auto r, auto mode) {
            hipLaunchKernelGGL((sdsp_pll_plain_kernel<decltype(r), decltype(mode)::value>), grid, dim3(kThreads), 0, stream, k);
            return static_cast<int>(SDSP_HIP_OK);
        });
        return launch_status("pll");
    }
    const uint64_t per_group = static_cast<uint64_t>(pll_waves(precision)) * kLanes;
    if (int rc = grid_of_blocks((pa.channels + per_group - 1) / per_group, "pll", &grid))
        return rc;
    if (int rc = with_kernel(precision, pa.mode, [&](auto r, auto mode) {
            using R = decltype(r);
            constexpr size_t lds = lds_bytes_of<R>();
            auto kern = sdsp_pll_kernel<R, decltype(mode)::value>;
            static std::atomic<uint64_t> attr_done{ 0 }; // one per instantiation of this lambda, that is per kernel
            if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), lds, attr_done))
                return rc;
            hipLaunchKernelGGL(kern, grid, dim3(shape_of<R>::waves * kLanes), lds, stream, k);
            return static_cast<int>(SDSP_HIP_OK);
        }))
        return rc;
    return launch_status("pll");
}
} // namespace sdsp_hip
