// timing.hip -- symbol-timing recovery banks for MI355X (gfx950): many independent second-order timing loops on interleaved I/Q rows,
// each a polyphase interpolator stepped in Q32.32 stream time at two strobes per symbol, a timing-error detector on the symbol strobes
// and a proportional-plus-integral loop filter that steers the step.
//
// One strobe of a channel (t: the uint64 stream time, w: the int32 advance word, parity: 0 = mid-symbol, 1 = symbol), in this order:
//     i = t >> 32, f = t & 0xffffffff, p = f >> (32 - log2 L)
//     z = H[p][0] x[i], then z = ma(H[p][k], x[i - k], z) for k = 1 .. T - 1, both planes alike     ma: one fmaf in f32, a multiply
//                                                                                                    then an add in f64
//     mid-symbol:  ym = z
//     symbol:      d = ps - z | s(ps) - s(z) | s(ps.r) - s(z.r)                 GARDNER | ZC_QPSK | ZC_BPSK (s: +-1 by the sign bit, NaN of a NaN)
//                  e = ma(d.i, ym.i, d.r ym.r)   (ZC_BPSK: e = d ym.r)
//                  integ = ma(beta, e, integ), clamped to +-max_dev;  v = ma(alpha, e, integ);  w = rint(clamp(v 2^32)), a NaN gives 0
//                  y[m] = z, err[m] = e, period[m] = integ;  ps = z
//     t += step0 + w
// Built with -ffp-contract=off and without fast-math, so nothing here contracts.  DESIGN.md section 5.29.
//
// Two kernels:
//   sdsp_timing_kernel        variant 0.  A workgroup of `waves` waves; each wave owns 64 channels, one lane per channel, and walks the
//                             whole call in blocks of B input samples with t, w, integ, ps, ym and parity in registers from the first
//                             sample to the last.  The tap table is staged into LDS once per workgroup, its rows at an odd pitch: the
//                             lanes of a wave sit on different phases.  A block of x goes through the wave's own LDS ring of
//                             B + T - 1 rows ([time][lane], a pitch of 65 elements; the row of sample n is (n + T - 1) mod (B + T - 1)),
//                             so the T - 1 samples in front of a block are still there when it arrives.  Per block every lane runs the
//                             strobes whose i lies inside the block, whatever its own clock; the next block's global loads are in
//                             flight meanwhile.  Outputs leave by per-lane stores at the lane's own running count.
//   sdsp_timing_plain_kernel  variant 1: one thread per channel straight from global memory, the table read from global memory and the
//                             state read-modify-written once per strobe.  The independent cross-check.
#include "stream_dev.h"

#include <atomic>
#include <type_traits>

namespace sdsp_hip
{
namespace
{
constexpr int kLanes = 64;              // one lane per channel
constexpr int kPitch = kLanes + 1;      // elements between two rows of a ring: the transposing accesses spread over the banks
constexpr int kMaxWaves = 4;            // waves per workgroup, at most
constexpr size_t kLdsLimit = 160 * 1024; // the LDS of a CU

template <typename R> __device__ __forceinline__ R ma(R a, R b, R c);
template <> __device__ __forceinline__ float ma<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
template <> __device__ __forceinline__ double ma<double>(double a, double b, double c) { return a * b + c; }

// +-1 by the sign bit of v: -0 counts as negative; a NaN stays a NaN, so a poisoned strobe poisons e whatever its sign bit
__device__ __forceinline__ float sign_of(float v)
{
    const float s = __builtin_bit_cast(float, 0x3f800000u | (__builtin_bit_cast(uint32_t, v) & 0x80000000u));
    return v == v ? s : v;
}
__device__ __forceinline__ double sign_of(double v)
{
    const double s = __builtin_bit_cast(double, 0x3ff0000000000000ull | (__builtin_bit_cast(uint64_t, v) & 0x8000000000000000ull));
    return v == v ? s : v;
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

// what a loop carries from strobe to strobe
template <typename R> struct loop_state {
    typename cplx_pair<R>::type ps, ym;
    R integ;
    uint64_t t;
    int32_t w;
    uint32_t parity;
};

// steps 2 to 4 of the contract for one strobe with the interpolated value z.  True on a symbol strobe: e and s.integ are then this
// symbol's err and period
template <typename R, int MODE>
__device__ __forceinline__ bool strobe(typename cplx_pair<R>::type z, R alpha, R beta, R max_dev, uint64_t step0, loop_state<R> &s, R &e)
{
    const bool symbol = s.parity != 0;
    if (!symbol) {
        s.ym = z;
        s.parity = 1;
    } else {
        if constexpr (MODE == SDSP_HIP_TIMING_GARDNER) {
            const R dr = s.ps.x - z.x, di = s.ps.y - z.y;
            e = ma<R>(di, s.ym.y, dr * s.ym.x);
        } else if constexpr (MODE == SDSP_HIP_TIMING_ZC_QPSK) {
            const R dr = sign_of(s.ps.x) - sign_of(z.x), di = sign_of(s.ps.y) - sign_of(z.y);
            e = ma<R>(di, s.ym.y, dr * s.ym.x);
        } else {
            e = (sign_of(s.ps.x) - sign_of(z.x)) * s.ym.x;
        }
        R integ = ma<R>(beta, e, s.integ);
        integ = integ < -max_dev ? -max_dev : (integ > max_dev ? max_dev : integ); // a NaN stays
        s.integ = integ;
        const R v = ma<R>(alpha, e, integ);
        R q = v * R(4294967296.0);
        q = q < advance_limits<R>::lo ? advance_limits<R>::lo : (q > advance_limits<R>::hi ? advance_limits<R>::hi : q);
        q = q == q ? q : R(0); // a NaN advances by step0 alone
        s.w = static_cast<int32_t>(round_even(q));
        s.ps = z;
        s.parity = 0;
    }
    s.t += step0 + static_cast<uint64_t>(static_cast<int64_t>(s.w)); // step0 >= 2^32 > |w|: always forward
    return symbol;
}

struct timing_kargs {
    const void *x;
    void *y, *err, *period; // err and period nullable
    uint32_t *counts;
    // the state's arrays; all null for variant 0 without state (zero state, nothing kept); hist null when T = 1
    uint64_t *time;
    void *ps, *ym, *integ;
    int32_t *w;
    uint32_t *parity;
    void *hist;
    const void *table; // [phase][tap] reals, unpadded
    uint64_t channels, samples, x_stride, y_stride, err_stride, period_stride, step0, cap;
    double alpha, beta, max_dev; // exactly representable in the plan precision
    uint32_t taps, phases;
    uint32_t pshift;      // 32 - log2 L
    uint32_t tpitch;      // LDS table: reals per phase row
    uint32_t ring_rows;   // B + T - 1
    uint32_t table_bytes; // LDS bytes in front of the first ring (a multiple of 16)
    uint32_t ring_bytes;  // LDS bytes of one wave's ring (a multiple of 16)
};

template <typename R> __device__ __forceinline__ void state_load(const timing_kargs &a, uint64_t c, loop_state<R> &s)
{
    const R *ps = static_cast<const R *>(a.ps), *ym = static_cast<const R *>(a.ym);
    s.ps.x = ps[2 * c];
    s.ps.y = ps[2 * c + 1];
    s.ym.x = ym[2 * c];
    s.ym.y = ym[2 * c + 1];
    s.integ = static_cast<const R *>(a.integ)[c];
    s.t = a.time[c];
    s.w = a.w[c];
    s.parity = a.parity[c] & 1u;
}
template <typename R> __device__ __forceinline__ void state_store(const timing_kargs &a, uint64_t c, const loop_state<R> &s)
{
    R *ps = static_cast<R *>(a.ps), *ym = static_cast<R *>(a.ym);
    ps[2 * c] = s.ps.x;
    ps[2 * c + 1] = s.ps.y;
    ym[2 * c] = s.ym.x;
    ym[2 * c + 1] = s.ym.y;
    static_cast<R *>(a.integ)[c] = s.integ;
    a.time[c] = s.t;
    a.w[c] = s.w;
    a.parity[c] = s.parity;
}

template <typename R> struct block_of;
template <> struct block_of<float> {
    static constexpr int value = 16; // 128-byte pieces of x
};
template <> struct block_of<double> {
    static constexpr int value = 8;
};

// the 16-byte chunks of a [64 channels][B samples] block of x: chunk q = i * 64 + lane covers channel q / CPR, samples (q % CPR) * EL ..
template <typename R, int B> struct xtile {
    using E = typename cplx_pair<R>::type;
    using V = typename vec16<R>::type;
    static constexpr int EL = 16 / sizeof(E); // samples per chunk
    static constexpr int CPR = B / EL;        // chunks per channel and block = chunks per lane
    static_assert(B % EL == 0 && CPR >= 1, "a block is a whole number of 16-byte chunks");

    // block [n0, n0 + B) into registers; what lies past the row's samples or the bank's channels is zero
    static __device__ __forceinline__ void load(const E *base, uint64_t stride, uint64_t c0, uint64_t channels, uint64_t n0, uint64_t samples,
                                                uint32_t lane, V (&v)[CPR])
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
                const R *p = reinterpret_cast<const R *>(base + c * stride + n);
                if (n + EL <= samples && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
                    r = __builtin_nontemporal_load(reinterpret_cast<const V *>(p));
                } else {
#pragma unroll
                    for (int e = 0; e < EL; e++)
                        if (n + e < samples) {
                            r[2 * e] = p[2 * e];
                            r[2 * e + 1] = p[2 * e + 1];
                        }
                }
            }
            v[i] = r;
        }
    }

    // registers -> the ring's rows first, first + 1 .. (mod rows)
    static __device__ __forceinline__ void to_ring(E *ring, uint32_t first, uint32_t rows, uint32_t lane, const V (&v)[CPR])
    {
#pragma unroll
        for (int i = 0; i < CPR; i++) {
            const uint32_t q = static_cast<uint32_t>(i) * kLanes + lane, ch = q / CPR, k = q % CPR;
#pragma unroll
            for (int e = 0; e < EL; e++) {
                uint32_t r = first + k * EL + e; // below 2 rows
                r = r >= rows ? r - rows : r;
                E s;
                s.x = v[i][2 * e];
                s.y = v[i][2 * e + 1];
                ring[r * kPitch + ch] = s;
            }
        }
    }
};

template <typename R, int MODE> __global__ __launch_bounds__(kMaxWaves *kLanes) void sdsp_timing_kernel(timing_kargs a)
{
    using E = typename cplx_pair<R>::type;
    constexpr int B = block_of<R>::value;
    using TX = xtile<R, B>;
    using V = typename vec16<R>::type;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const uint32_t lane = threadIdx.x % kLanes, wave = threadIdx.x / kLanes, waves = blockDim.x / kLanes;
    const uint32_t T = a.taps, RB = a.ring_rows;
    R *const tab = reinterpret_cast<R *>(lds_raw);
    {
        const R *g = static_cast<const R *>(a.table);
        const uint32_t entries = a.phases * T;
        for (uint32_t e = threadIdx.x; e < entries; e += blockDim.x) {
            const uint32_t p = e / T, k = e - p * T;
            tab[p * a.tpitch + k] = g[e];
        }
    }
    E *const ring = reinterpret_cast<E *>(lds_raw + a.table_bytes + static_cast<size_t>(wave) * a.ring_bytes);
    const uint64_t c0 = (static_cast<uint64_t>(blockIdx.x) * waves + wave) * kLanes, c = c0 + lane;
    const bool have = c < a.channels;
    const R alpha = static_cast<R>(a.alpha), beta = static_cast<R>(a.beta), max_dev = static_cast<R>(a.max_dev);
    const E *xg = static_cast<const E *>(a.x);

    V xv[TX::CPR];
    TX::load(xg, a.x_stride, c0, a.channels, 0, a.samples, lane, xv);
    loop_state<R> s{};
    if (have && a.time)
        state_load<R>(a, c, s);
    if (!have)
        s.t = ~0ull; // never below the call's end: no strobe
    // the T - 1 samples in front of the call: sample -1 - j lies in row T - 2 - j
    {
        const R *hist = have && a.hist ? static_cast<const R *>(a.hist) + c * (T - 1) * 2 : nullptr;
        for (uint32_t j = 0; j + 1 < T; j++) {
            E h;
            h.x = hist ? hist[2 * j] : R(0);
            h.y = hist ? hist[2 * j + 1] : R(0);
            ring[(T - 2 - j) * kPitch + lane] = h;
        }
    }
    E *const yg = static_cast<E *>(a.y) + c * a.y_stride;
    R *const eg = a.err ? static_cast<R *>(a.err) + c * a.err_stride : nullptr;
    R *const pg = a.period ? static_cast<R *>(a.period) + c * a.period_stride : nullptr;
    uint64_t m = 0; // this call's symbols of the channel so far

    const uint32_t S = static_cast<uint32_t>(a.samples); // below 2^31
    const uint32_t nblk = (S + B - 1) / B;
    uint32_t r0 = T - 1; // the row of the block's first sample
    const E *const col = ring + lane;
    const uint32_t top = (RB - 1) * kPitch;
    for (uint32_t blk = 0; blk < nblk; blk++) {
        const uint32_t n0 = blk * B;
        const uint32_t end = S - n0 < static_cast<uint32_t>(B) ? S : n0 + B;
        TX::to_ring(ring, r0, RB, lane, xv);
        __syncthreads(); // the block is whole (and, the first time, the table and the history)
        if (blk + 1 < nblk)
            TX::load(xg, a.x_stride, c0, a.channels, static_cast<uint64_t>(n0) + B, a.samples, lane, xv);
        // the lane's own column from here to the barrier: every strobe that falls on a sample of this block
        while (static_cast<uint32_t>(s.t >> 32) < end) { // t >> 32 >= n0: the blocks before took everything below; idle lanes: 2^32 - 1
            const uint32_t i = static_cast<uint32_t>(s.t >> 32), f = static_cast<uint32_t>(s.t);
            const R *hp = tab + static_cast<uint32_t>(static_cast<uint64_t>(f) >> a.pshift) * a.tpitch;
            uint32_t r = r0 + (i - n0); // below 2 RB
            r = r >= RB ? r - RB : r;
            uint32_t ro = r * kPitch; // the row's offset in the lane's column; one row back per tap, from row 0 to the last one
            E xs = col[ro];
            R g = hp[0];
            E z;
            z.x = g * xs.x;
            z.y = g * xs.y;
#pragma unroll 4 // the reads of four taps go out before the first sum needs one: a wave has no neighbour on its SIMD to hide them
            for (uint32_t k = 1; k < T; k++) {
                ro = ro ? ro - kPitch : top;
                xs = col[ro];
                g = hp[k];
                z.x = ma<R>(g, xs.x, z.x);
                z.y = ma<R>(g, xs.y, z.y);
            }
            R e = R(0);
            if (strobe<R, MODE>(z, alpha, beta, max_dev, a.step0, s, e)) {
                if (m < a.cap) { // always: cap bounds the count of any loop (sdsp_hip_timing_max_out)
                    yg[m] = z;
                    if (eg)
                        eg[m] = e;
                    if (pg)
                        pg[m] = s.integ;
                }
                m++;
            }
        }
        __syncthreads(); // the rows in front of the block are free for the next one
        r0 += B;
        r0 = r0 >= RB ? r0 - RB : r0;
    }
    if (have) {
        a.counts[c] = static_cast<uint32_t>(m);
        if (a.time) {
            s.t -= static_cast<uint64_t>(S) << 32;
            state_store<R>(a, c, s);
            if (a.hist) {
                // the last T - 1 inputs, newest first: sample S - 1 lies in row (S - 1 + T - 1) mod RB
                R *hist = static_cast<R *>(a.hist) + c * (T - 1) * 2;
                uint32_t r = (S + T - 2) % RB;
                for (uint32_t j = 0; j + 1 < T; j++) {
                    const E h = ring[r * kPitch + lane];
                    hist[2 * j] = h.x;
                    hist[2 * j + 1] = h.y;
                    r = r ? r - 1 : RB - 1;
                }
            }
        }
    }
}

// ---- variant 1: one thread per channel from global memory, the state read-modify-written once per strobe ---------------------------
template <typename R, int MODE> __global__ __launch_bounds__(kThreads) void sdsp_timing_plain_kernel(timing_kargs a)
{
    using E = typename cplx_pair<R>::type;
    const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (c >= a.channels)
        return;
    const R alpha = static_cast<R>(a.alpha), beta = static_cast<R>(a.beta), max_dev = static_cast<R>(a.max_dev);
    const uint32_t T = a.taps;
    const R *tab = static_cast<const R *>(a.table);
    const R *x = static_cast<const R *>(a.x) + c * a.x_stride * 2;
    R *y = static_cast<R *>(a.y) + c * a.y_stride * 2;
    R *err = a.err ? static_cast<R *>(a.err) + c * a.err_stride : nullptr;
    R *period = a.period ? static_cast<R *>(a.period) + c * a.period_stride : nullptr;
    R *hist = a.hist ? static_cast<R *>(a.hist) + c * (T - 1) * 2 : nullptr;
    volatile uint64_t *time_p = a.time + c; // volatile: every strobe goes through memory
    volatile R *ps_p = static_cast<R *>(a.ps) + 2 * c, *ym_p = static_cast<R *>(a.ym) + 2 * c, *integ_p = static_cast<R *>(a.integ) + c;
    volatile int32_t *w_p = a.w + c;
    volatile uint32_t *parity_p = a.parity + c;
    const int64_t S = static_cast<int64_t>(a.samples);
    uint64_t m = 0;
    for (;;) {
        loop_state<R> s;
        s.t = *time_p;
        const int64_t i = static_cast<int64_t>(s.t >> 32);
        if (i >= S)
            break;
        s.ps.x = ps_p[0];
        s.ps.y = ps_p[1];
        s.ym.x = ym_p[0];
        s.ym.y = ym_p[1];
        s.integ = *integ_p;
        s.w = *w_p;
        s.parity = *parity_p & 1u;
        const uint32_t f = static_cast<uint32_t>(s.t);
        const R *hp = tab + static_cast<size_t>(static_cast<uint64_t>(f) >> a.pshift) * T;
        E z;
        for (uint32_t k = 0; k < T; k++) {
            const int64_t xi = i - static_cast<int64_t>(k);
            const R *src = xi >= 0 ? x + 2 * xi : hist + 2 * (-1 - xi); // -1 - xi < T - 1: k <= T - 1
            const R xr = src[0], xm = src[1], g = hp[k];
            if (k == 0) {
                z.x = g * xr;
                z.y = g * xm;
            } else {
                z.x = ma<R>(g, xr, z.x);
                z.y = ma<R>(g, xm, z.y);
            }
        }
        R e = R(0);
        if (strobe<R, MODE>(z, alpha, beta, max_dev, a.step0, s, e)) {
            if (m < a.cap) {
                y[2 * m] = z.x;
                y[2 * m + 1] = z.y;
                if (err)
                    err[m] = e;
                if (period)
                    period[m] = s.integ;
            }
            m++;
        }
        ps_p[0] = s.ps.x;
        ps_p[1] = s.ps.y;
        ym_p[0] = s.ym.x;
        ym_p[1] = s.ym.y;
        *integ_p = s.integ;
        *w_p = s.w;
        *parity_p = s.parity;
        *time_p = s.t;
    }
    a.counts[c] = static_cast<uint32_t>(m);
    *time_p = *time_p - (static_cast<uint64_t>(S) << 32);
    // the last T - 1 inputs, newest first; from the oldest up, so that what moves back inside the history is read before it is replaced
    for (int64_t j = static_cast<int64_t>(T) - 2; j >= 0; j--) {
        const int64_t xi = S - 1 - j;
        const R *src = xi >= 0 ? x + 2 * xi : hist + 2 * (j - S);
        const R hr = src[0], hi = src[1];
        hist[2 * j] = hr;
        hist[2 * j + 1] = hi;
    }
}

size_t real_bytes(int precision) { return precision == SDSP_HIP_F64 ? 8 : 4; }
uint32_t block_for(int precision) { return precision == SDSP_HIP_F64 ? block_of<double>::value : block_of<float>::value; }
uint32_t tpitch_for(uint32_t phases, uint32_t taps) { return phases > 1 ? (taps | 1u) : taps; }
size_t round16(size_t b) { return (b + 15) / 16 * 16; }
size_t table_bytes_for(int precision, uint32_t phases, uint32_t taps)
{
    return round16(static_cast<size_t>(phases) * tpitch_for(phases, taps) * real_bytes(precision));
}
size_t ring_bytes_for(int precision, uint32_t taps)
{
    return round16(static_cast<size_t>(block_for(precision) + taps - 1) * kPitch * 2 * real_bytes(precision));
}

// f(R(), mode constant)
template <typename F> int with_kernel(int precision, int mode, F f)
{
    auto by_mode = [&](auto r) {
        switch (mode) {
        case SDSP_HIP_TIMING_GARDNER:
            return f(r, std::integral_constant<int, SDSP_HIP_TIMING_GARDNER>());
        case SDSP_HIP_TIMING_ZC_QPSK:
            return f(r, std::integral_constant<int, SDSP_HIP_TIMING_ZC_QPSK>());
        default:
            return f(r, std::integral_constant<int, SDSP_HIP_TIMING_ZC_BPSK>());
        }
    };
    return precision == SDSP_HIP_F64 ? by_mode(double()) : by_mode(float());
}
} // namespace

uint32_t timing_block(int precision) { return block_for(precision); }

// as many waves as fit beside the table in the LDS of a CU, at most kMaxWaves; at least one fits within the plan limits (a table of
// at most 33792 B and a ring of at most 73840 B)
uint32_t timing_waves(int precision, uint32_t phases, uint32_t taps)
{
    const size_t w = (kLdsLimit - table_bytes_for(precision, phases, taps)) / ring_bytes_for(precision, taps);
    return static_cast<uint32_t>(w < static_cast<size_t>(kMaxWaves) ? w : kMaxWaves);
}

uint32_t timing_lds_bytes(int precision, uint32_t phases, uint32_t taps)
{
    return static_cast<uint32_t>(table_bytes_for(precision, phases, taps) + timing_waves(precision, phases, taps) * ring_bytes_for(precision, taps));
}

const char *timing_kernel_for(int variant) { return variant == 1 ? "sdsp_timing_plain_kernel" : "sdsp_timing_kernel"; }

int launch_timing(int precision, const timing_args &ta, int variant, void *stream_v)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    uint32_t lb = 0;
    while ((1u << lb) < ta.phases)
        lb++;
    timing_kargs k{};
    k.x = ta.x;
    k.y = ta.y;
    k.err = ta.err;
    k.period = ta.period;
    k.counts = ta.counts;
    k.time = ta.time;
    k.ps = ta.ps;
    k.ym = ta.ym;
    k.integ = ta.integ;
    k.w = ta.w;
    k.parity = ta.parity;
    k.hist = ta.taps > 1 ? ta.hist : nullptr;
    k.table = ta.table;
    k.channels = ta.channels;
    k.samples = ta.samples;
    k.x_stride = ta.x_stride;
    k.y_stride = ta.y_stride;
    k.err_stride = ta.err_stride;
    k.period_stride = ta.period_stride;
    k.step0 = ta.step0;
    k.cap = ta.cap;
    k.alpha = ta.alpha;
    k.beta = ta.beta;
    k.max_dev = ta.max_dev;
    k.taps = ta.taps;
    k.phases = ta.phases;
    k.pshift = 32 - lb;
    k.tpitch = tpitch_for(ta.phases, ta.taps);
    k.ring_rows = block_for(precision) + ta.taps - 1;
    k.table_bytes = static_cast<uint32_t>(table_bytes_for(precision, ta.phases, ta.taps));
    k.ring_bytes = static_cast<uint32_t>(ring_bytes_for(precision, ta.taps));
    dim3 grid;
    if (variant == 1) {
        if (!k.time)
            return fail(SDSP_HIP_ERR_INVALID_ARG, "timing: the plain kernel needs a state buffer");
        if (int rc = grid_for(ta.channels, "timing", &grid))
            return rc;
        with_kernel(precision, ta.mode, [&](auto r, auto mode) {
            hipLaunchKernelGGL((sdsp_timing_plain_kernel<decltype(r), decltype(mode)::value>), grid, dim3(kThreads), 0, stream, k);
            return static_cast<int>(SDSP_HIP_OK);
        });
        return launch_status("timing");
    }
    const uint32_t waves = timing_waves(precision, ta.phases, ta.taps);
    if (waves == 0)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "timing: the table and one ring exceed the LDS of a CU"); // no plan within the limits
    const uint64_t per_group = static_cast<uint64_t>(waves) * kLanes;
    if (int rc = grid_of_blocks((ta.channels + per_group - 1) / per_group, "timing", &grid))
        return rc;
    const size_t lds = k.table_bytes + static_cast<size_t>(waves) * k.ring_bytes;
    if (int rc = with_kernel(precision, ta.mode, [&](auto r, auto mode) {
            using R = decltype(r);
            auto kern = sdsp_timing_kernel<R, decltype(mode)::value>;
            static std::atomic<uint64_t> attr_done{ 0 }; // one per instantiation of this lambda, that is per kernel
            if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), kLdsLimit, attr_done))
                return rc;
            hipLaunchKernelGGL(kern, grid, dim3(waves * kLanes), lds, stream, k);
            return static_cast<int>(SDSP_HIP_OK);
        }))
        return rc;
    return launch_status("timing");
}
} // namespace sdsp_hip
