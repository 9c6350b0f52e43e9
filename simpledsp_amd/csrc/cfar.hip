// cfar.hip -- streaming constant-false-alarm-rate detector banks (CA, GO, SO and OS thresholds) for MI355X (gfx950): many independent
// rows of power (or of interleaved I/Q that becomes power on the way in), each output a threshold and a one-byte decision.
//
// With L = train, G = guard, half = L + G, W = 2 half + 1, D = L + 2 G + 1 and p_c = the row's history followed by the block, input
// sample n tests the cell p[n - half] against a threshold made from the 2 L training cells
//     lag  = p[n - W + 1 .. n - W + L]      lead = p[n - L + 1 .. n].
// CA, GO and SO sum each side in ascending index from +0 and combine the two sums; OS takes the element of rank k (IEEE 754 totalOrder
// through the rank bank's key) of all 2 L cells.  One product with the plan's scale, one comparison.  DESIGN.md section 5.27.  Built
// with -ffp-contract=off: the I/Q power is two products and a sum, the threshold a sum and a product, never an FMA.
//
// Three kernels:
//   sdsp_cfar_sum_kernel    variant 0 of CA, GO and SO.  A workgroup takes `run` consecutive outputs of one row.  It stages the powers
//                           of the segment and of the W - 1 cells in front of it in LDS, then computes the boxcar
//                           B[j] = (((+0 + p[j - L + 1]) + ..) + p[j]) once per position for the segment and the D positions in front
//                           of it: a thread keeps eight consecutive boxcars in registers and reads every power once for up to eight
//                           additions.  The sums run in ascending index, so lag(n) is B[n - D] bit for bit and lead(n) is B[n]: L
//                           additions per output, not 2 L.  Thresholds leave as 16-byte vectors and decisions as 4-byte words where
//                           the row's alignment allows.
//   sdsp_cfar_os_kernel     variant 0 of OS: the rank bank's form.  One wave per workgroup, one lane per run of consecutive outputs;
//                           the 2 L training keys are a sorted array of WP keys (8 .. 256) in registers.  One output is two
//                           delete-and-insert passes -- lead: p[n] arrives, p[n - L] departs; lag: p[n - D] arrives, p[n - W]
//                           departs -- and one read through the wave-uniform switch.  A run starts from 2 L keys of value 0 and a
//                           stream that holds key 0 in front of the W - 1 cells before the run, so the bits cannot depend on `run`.
//                           The five streams (four for the passes, the cell under test) go through LDS transposed, [time][lane].
//   sdsp_cfar_plain_kernel  variant 1, every mode: one thread per output straight from global memory, plain loops, selection by
//                           counting.  The independent cross-check.
// to_key / from_key / sorted_step / element_at are copies of rank_filter.hip's: that file and its register profile stay as they are.
// The new history is carry_history's (stream_carry.hip), launched by the caller behind either kernel.
#include "stream_dev.h"

#include <type_traits>

namespace sdsp_hip
{
namespace
{
constexpr int kLanes = 64;         // sdsp_cfar_os_kernel: one wave per workgroup, one lane per run
constexpr int kPitch = kLanes + 1; // elements between two LDS rows of its tiles
constexpr int kWin = 8;            // sdsp_cfar_sum_kernel: consecutive boxcars per thread
constexpr int kMaxLead = 2 * (128 + 255);   // W - 1 at the limits
constexpr int kMaxLag = 128 + 2 * 255 + 1;  // D at the limits

template <typename R> struct key_of;
template <> struct key_of<float> {
    typedef uint32_t type;
};
template <> struct key_of<double> {
    typedef uint64_t type;
};

template <typename K> __host__ __device__ __forceinline__ K to_key(K u)
{
    constexpr K sign = K(1) << (sizeof(K) * 8 - 1);
    return (u & sign) ? ~u : (u | sign);
}
template <typename K> __host__ __device__ __forceinline__ K from_key(K k)
{
    constexpr K sign = K(1) << (sizeof(K) * 8 - 1);
    return (k & sign) ? (k ^ sign) : ~k;
}
template <typename R> __device__ __forceinline__ typename key_of<R>::type bits_of(R v)
{
    typename key_of<R>::type u;
    __builtin_memcpy(&u, &v, sizeof(u));
    return u;
}
template <typename R> __device__ __forceinline__ R value_of(typename key_of<R>::type u)
{
    R v;
    __builtin_memcpy(&v, &u, sizeof(v));
    return v;
}

struct cfar_kargs {
    const void *x;
    void *thr;        // nullable
    uint8_t *det;     // nullable
    const void *hist; // nullable: channels x (W - 1) elements of the input's kind, newest first
    uint64_t channels, x_stride, thr_stride, det_stride;
    double scale; // already rounded to the precision
    uint32_t samples, train, guard, mode, rank, iq, run, runs_per_row;
};

// the power at position pos of row c, -(W - 1) <= pos < samples; positions below 0 are the history
template <typename R> __device__ __forceinline__ R power_at(const cfar_kargs &a, uint64_t c, int64_t pos)
{
    const uint64_t H = 2ull * (a.train + a.guard);
    if (!a.iq) {
        if (pos >= 0)
            return static_cast<const R *>(a.x)[c * a.x_stride + static_cast<uint64_t>(pos)];
        return a.hist ? static_cast<const R *>(a.hist)[c * H + static_cast<uint64_t>(-1 - pos)] : R(0);
    }
    using Z = typename cplx_pair<R>::type;
    Z z;
    z[0] = R(0);
    z[1] = R(0);
    if (pos >= 0)
        z = static_cast<const Z *>(a.x)[c * a.x_stride + static_cast<uint64_t>(pos)];
    else if (a.hist)
        z = static_cast<const Z *>(a.hist)[c * H + static_cast<uint64_t>(-1 - pos)];
    const R rr = z[0] * z[0], ii = z[1] * z[1];
    return rr + ii;
}

// A threshold that is a NaN leaves as the canonical quiet NaN (sign 0, the top mantissa bit alone): IEEE 754 leaves the sign and
// payload of a NaN result to the implementation, and with them which operand's payload a sum of two NaNs keeps, so without this the
// bits could depend on the kernel variant and on the order the compiler gives the operands of an addition.
template <typename R> __device__ __forceinline__ R canonical(R th)
{
    using K = typename key_of<R>::type;
    constexpr K quiet = sizeof(K) == 4 ? K(0x7FC00000u) : K(0x7FF8000000000000ull);
    return th != th ? value_of<R>(quiet) : th;
}

// thr of the sum modes from the two side sums
template <typename R> __device__ __forceinline__ R combine(uint32_t mode, R lag, R lead, R c)
{
    R v;
    if (mode == SDSP_HIP_CFAR_CA)
        v = lag + lead;
    else if (mode == SDSP_HIP_CFAR_GO)
        v = (lag > lead) ? lag : lead;
    else
        v = (lag < lead) ? lag : lead;
    return canonical<R>(v * c);
}

// ---- variant 0, sum modes ---------------------------------------------------------------------------------------------------------------
template <typename R> constexpr int seg_max() { return sizeof(R) == 4 ? 2048 : 1024; }

// LDS index of element i: one pad element after every eight, so that threads eight elements apart fall on different banks
__device__ __forceinline__ uint32_t padded(uint32_t i) { return i + (i >> 3); }
constexpr int padded_size(int n) { return n + n / 8 + 1; }

template <typename R> __global__ __launch_bounds__(kThreads) void sdsp_cfar_sum_kernel(cfar_kargs a)
{
    using V = typename vec16<R>::type;
    constexpr int EL = 16 / sizeof(R);
    __shared__ R pw[padded_size(seg_max<R>() + kMaxLead + kWin)]; // index i: position n0 - (W - 1) + i
    __shared__ R bx[padded_size(seg_max<R>() + kMaxLag + kWin)];  // index m: the boxcar that ends at position n0 - D + m
    const uint32_t L = a.train, G = a.guard, half = L + G, W = 2 * half + 1, D = L + 2 * G + 1;
    const uint32_t tid = threadIdx.x;
    const uint64_t c = udiv(blockIdx.x, a.runs_per_row);
    const uint32_t seg = blockIdx.x - static_cast<uint32_t>(c) * a.runs_per_row;
    const uint32_t n0 = seg * a.run; // < samples
    const uint32_t T = a.samples - n0 < a.run ? a.samples - n0 : a.run;
    const uint32_t np = T + W - 1, nb = T + D;
    for (uint32_t i = tid; i < np; i += kThreads)
        pw[padded(i)] = power_at<R>(a, c, static_cast<int64_t>(n0) - (W - 1) + i);
    if (tid < kWin) { // the spare elements behind both ranges: read by the last threads' windows and output groups, never used
        pw[padded(np + tid)] = R(0);
        bx[padded(nb + tid)] = R(0);
    }
    __syncthreads();
    // boxcar m is pw[m] + .. + pw[m + L - 1] in that order (W - 1 - D = L - 1).  Step t of a thread reads pw[m0 + t] once; boxcar r
    // of the thread's eight takes it when 0 <= t - r < L.  Boxcars at m >= nb read up to kWin - 1 elements past np and are dropped.
    for (uint32_t m0 = tid * kWin; m0 < nb; m0 += kThreads * kWin) {
        R acc[kWin];
#pragma unroll
        for (int r = 0; r < kWin; r++)
            acc[r] = R(0);
#pragma unroll
        for (int t = 0; t < kWin - 1; t++) { // the window fills: boxcars 0 .. t
            const R v = pw[padded(m0 + t)];
#pragma unroll
            for (int r = 0; r <= t; r++)
                if (static_cast<uint32_t>(t - r) < L)
                    acc[r] += v;
        }
        for (uint32_t t = kWin - 1; t < L; t++) { // every boxcar takes every power
            const R v = pw[padded(m0 + t)];
#pragma unroll
            for (int r = 0; r < kWin; r++)
                acc[r] += v;
        }
        for (uint32_t t = L > kWin - 1 ? L : kWin - 1; t < L + kWin - 1; t++) { // the window drains
            const R v = pw[padded(m0 + t)];
#pragma unroll
            for (int r = 0; r < kWin; r++)
                if (t - static_cast<uint32_t>(r) < L) // t >= r here
                    acc[r] += v;
        }
#pragma unroll
        for (int r = 0; r < kWin; r++)
            if (m0 + r < nb)
                bx[padded(m0 + r)] = acc[r];
    }
    __syncthreads();
    // output i of the segment: lead = bx[i + D], lag = bx[i], the cell under test = pw[i + half]
    const R scale = static_cast<R>(a.scale);
    R *thr_row = a.thr ? static_cast<R *>(a.thr) + c * a.thr_stride + n0 : nullptr;
    uint8_t *det_row = a.det ? a.det + c * a.det_stride + n0 : nullptr;
    const bool thr_vec = (reinterpret_cast<uintptr_t>(thr_row) & 15u) == 0, det_vec = (reinterpret_cast<uintptr_t>(det_row) & 3u) == 0;
    for (uint32_t i0 = tid * 4; i0 < T; i0 += kThreads * 4) {
        R th[4];
        uint32_t d = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t i = i0 + e; // below T + 3: inside the staged ranges (D, half >= 1 .. and the kWin spare elements)
            th[e] = combine<R>(a.mode, bx[padded(i)], bx[padded(i + D)], scale);
            d |= (pw[padded(i + half)] > th[e] ? 1u : 0u) << (8 * e);
        }
        const bool whole = i0 + 4 <= T;
        if (thr_row) {
            if (whole && thr_vec) {
#pragma unroll
                for (int q = 0; q < 4 / EL; q++) {
                    V v;
#pragma unroll
                    for (int e = 0; e < EL; e++)
                        v[e] = th[q * EL + e];
                    *reinterpret_cast<V *>(thr_row + i0 + q * EL) = v;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (i0 + e < T)
                        thr_row[i0 + e] = th[e];
            }
        }
        if (det_row) {
            if (whole && det_vec) {
                *reinterpret_cast<uint32_t *>(det_row + i0) = d;
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (i0 + e < T)
                        det_row[i0 + e] = static_cast<uint8_t>((d >> (8 * e)) & 1u);
            }
        }
    }
}

// ---- variant 0, OS mode -----------------------------------------------------------------------------------------------------------------
// the middle one of a <= b and v: v clamped to [a, b]
__device__ __forceinline__ uint32_t clamp_between(uint32_t a, uint32_t b, uint32_t v)
{
    uint32_t r; // one instruction; the compiler does not form it from min and max of three variables
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(v));
    return r;
}
__device__ __forceinline__ uint64_t clamp_between(uint64_t a, uint64_t b, uint64_t v)
{
    const uint64_t lo = v < a ? a : v;
    return b < lo ? b : lo;
}

// The sorted array loses one copy of `old` and gains `v` (rank_filter.hip): with t = the array without that copy, the new element i
// is v clamped to [t[i - 1], t[i]].
template <typename K, int WP> __device__ __forceinline__ void sorted_step(K (&s)[WP], K old, K v)
{
    K tp = K(0);
#pragma unroll
    for (int i = 0; i < WP; i++) {
        const K nx = i + 1 < WP ? s[i + 1] : static_cast<K>(~K(0));
        const K t = s[i] < old ? s[i] : nx;
        s[i] = clamp_between(tp, t, v);
        tp = t;
    }
}

// s[idx] for a wave-uniform idx < WP through compile-time indices only
#define SDSP_CFAR_CASE1(i)                                                                                                             \
    case (i):                                                                                                                          \
        if constexpr ((i) < WP)                                                                                                        \
            out = s[(i) < WP ? (i) : 0];                                                                                               \
        break;
#define SDSP_CFAR_CASE4(i) SDSP_CFAR_CASE1(i) SDSP_CFAR_CASE1((i) + 1) SDSP_CFAR_CASE1((i) + 2) SDSP_CFAR_CASE1((i) + 3)
#define SDSP_CFAR_CASE16(i) SDSP_CFAR_CASE4(i) SDSP_CFAR_CASE4((i) + 4) SDSP_CFAR_CASE4((i) + 8) SDSP_CFAR_CASE4((i) + 12)
#define SDSP_CFAR_CASE64(i) SDSP_CFAR_CASE16(i) SDSP_CFAR_CASE16((i) + 16) SDSP_CFAR_CASE16((i) + 32) SDSP_CFAR_CASE16((i) + 48)
template <typename K, int WP> __device__ __forceinline__ K element_at(const K (&s)[WP], uint32_t idx)
{
    K out = s[0];
    switch (idx) {
        SDSP_CFAR_CASE64(0)
        SDSP_CFAR_CASE64(64)
        SDSP_CFAR_CASE64(128)
        SDSP_CFAR_CASE64(192)
    default:
        break;
    }
    return out;
}
#undef SDSP_CFAR_CASE64
#undef SDSP_CFAR_CASE16
#undef SDSP_CFAR_CASE4
#undef SDSP_CFAR_CASE1

// samples per staging block
template <typename R> constexpr int os_block() { return static_cast<int>(32 / sizeof(R)); }

// A lane's stream: index j is position start - (W - 1) + j of its row; indices below 0 hold key 0, the array's filling, and positions
// past the row +0 (they reach no output).  Tile t of a block holds the stream shifted by offs[t]: the lead pass's arriving (0) and
// departing (L) keys, the lag pass's (D, W), and the cell under test (half).
template <typename R, int WP> __global__ __launch_bounds__(kLanes) void sdsp_cfar_os_kernel(cfar_kargs a)
{
    using K = typename key_of<R>::type;
    constexpr int B = os_block<R>();
    __shared__ K tile[5][B * kPitch];
    __shared__ uint32_t row_of[kLanes], start_of[kLanes];
    const uint32_t lane = threadIdx.x, L = a.train, G = a.guard, half = L + G, W = 2 * half + 1, D = L + 2 * G + 1;
    {
        const uint64_t g = static_cast<uint64_t>(blockIdx.x) * kLanes + lane;
        const uint64_t c = udiv(g, a.runs_per_row), k = g - c * a.runs_per_row;
        const bool have = c < a.channels;
        row_of[lane] = have ? static_cast<uint32_t>(c) : 0u;
        start_of[lane] = have ? static_cast<uint32_t>(k * a.run) : 0xffffffffu; // k run < samples
    }
    K s[WP];
#pragma unroll
    for (int i = 0; i < WP; i++)
        s[i] = static_cast<uint32_t>(i) < 2 * L ? K(0) : static_cast<K>(~K(0));
    __syncthreads();
    const uint32_t offs[5] = { 0u, L, D, W, half };
    const R scale = static_cast<R>(a.scale);
    const int64_t total = static_cast<int64_t>(W - 1) + a.run; // steps of every lane of the grid
    for (int64_t j0 = 0; j0 < total; j0 += B) {
        const int len = total - j0 < B ? static_cast<int>(total - j0) : B;
#pragma unroll
        for (int t = 0; t < 5; t++) {
#pragma unroll 4
            for (int i = 0; i < B; i++) { // element q = i 64 + lane of the tile: step q % B of lane q / B
                const uint32_t q = static_cast<uint32_t>(i) * kLanes + lane, o = q / B, kk = q % B;
                const int64_t sidx = j0 + kk - static_cast<int64_t>(offs[t]);
                const uint32_t st = start_of[o];
                K key = K(0);
                if (sidx >= 0 && st < a.samples) {
                    const int64_t pos = static_cast<int64_t>(st) - (W - 1) + sidx; // >= -(W - 1)
                    const R p = pos < static_cast<int64_t>(a.samples) ? power_at<R>(a, row_of[o], pos) : R(0);
                    key = to_key<K>(bits_of<R>(p));
                }
                tile[t][kk * kPitch + o] = key;
            }
        }
        __syncthreads();
        // the lane's own column from here to the barrier; the threshold and the decision take the places of tiles 0 and 4
        for (int i = 0; i < len; i++) {
            const int at = i * kPitch + lane;
            sorted_step<K, WP>(s, tile[1][at], tile[0][at]);
            sorted_step<K, WP>(s, tile[3][at], tile[2][at]);
            const R v = value_of<R>(from_key<K>(element_at<K, WP>(s, a.rank)));
            const R th = canonical<R>(v * scale);
            const R cut = value_of<R>(from_key<K>(tile[4][at]));
            tile[0][at] = bits_of<R>(th);
            tile[4][at] = cut > th ? K(1) : K(0);
        }
        __syncthreads();
        // outputs: step j >= W - 1 of a lane is output start + j - (W - 1) of its row, inside its run and the row
#pragma unroll 4
        for (int i = 0; i < B; i++) {
            const uint32_t q = static_cast<uint32_t>(i) * kLanes + lane, o = q / B, kk = q % B;
            const int64_t j = j0 + kk;
            const uint32_t st = start_of[o];
            if (static_cast<int>(kk) >= len || j < static_cast<int64_t>(W - 1) || st >= a.samples)
                continue;
            const uint64_t n = static_cast<uint64_t>(st) + static_cast<uint64_t>(j - (W - 1)); // < st + run
            if (n >= a.samples)
                continue;
            if (a.thr)
                static_cast<K *>(a.thr)[static_cast<uint64_t>(row_of[o]) * a.thr_stride + n] = tile[0][kk * kPitch + o];
            if (a.det)
                a.det[static_cast<uint64_t>(row_of[o]) * a.det_stride + n] = static_cast<uint8_t>(tile[4][kk * kPitch + o]);
        }
        __syncthreads();
    }
}

// ---- variant 1: one thread per output from global memory --------------------------------------------------------------------------------
template <typename R> __global__ __launch_bounds__(kThreads) void sdsp_cfar_plain_kernel(cfar_kargs a)
{
    using K = typename key_of<R>::type;
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= a.channels * a.samples)
        return;
    const uint64_t c = udiv(i, a.samples), n = i - c * a.samples;
    const uint32_t L = a.train, half = L + a.guard, W = 2 * half + 1;
    auto cell = [&](uint32_t back) -> R { // p_c[n - back], back <= W - 1
        const bool in_row = n >= back;
        const uint64_t at = in_row ? c * a.x_stride + (n - back) : c * (W - 1ull) + (back - n - 1);
        const void *base = in_row ? a.x : a.hist;
        if (!base)
            return R(0);
        if (!a.iq)
            return static_cast<const R *>(base)[at];
        const R re = static_cast<const R *>(base)[2 * at], im = static_cast<const R *>(base)[2 * at + 1];
        const R rr = re * re, ii = im * im;
        return rr + ii;
    };
    // training cell q of 2 L in ascending position: the lag side first
    auto train_back = [&](uint32_t q) -> uint32_t { return q < L ? W - 1 - q : 2 * L - 1 - q; };
    const R scale = static_cast<R>(a.scale);
    R th;
    if (a.mode == SDSP_HIP_CFAR_OS) {
        K found = K(0);
        for (uint32_t t = 0; t < 2 * L; t++) {
            const R pv = cell(train_back(t));
            K cand;
            __builtin_memcpy(&cand, &pv, sizeof(cand));
            cand = (cand >> (sizeof(K) * 8 - 1)) ? ~cand : (cand | (K(1) << (sizeof(K) * 8 - 1)));
            uint32_t below = 0;
            for (uint32_t q = 0; q < 2 * L; q++) {
                const R ov = cell(train_back(q));
                K other;
                __builtin_memcpy(&other, &ov, sizeof(other));
                other = (other >> (sizeof(K) * 8 - 1)) ? ~other : (other | (K(1) << (sizeof(K) * 8 - 1)));
                below += (other < cand || (other == cand && q < t)) ? 1u : 0u;
            }
            if (below == a.rank)
                found = cand;
        }
        found = (found >> (sizeof(K) * 8 - 1)) ? (found ^ (K(1) << (sizeof(K) * 8 - 1))) : ~found;
        R v;
        __builtin_memcpy(&v, &found, sizeof(v));
        th = v * scale;
    } else {
        R lag = R(0), lead = R(0);
        for (uint32_t q = 0; q < L; q++)
            lag = lag + cell(W - 1 - q);
        for (uint32_t q = 0; q < L; q++)
            lead = lead + cell(L - 1 - q);
        if (a.mode == SDSP_HIP_CFAR_CA) {
            const R both = lag + lead;
            th = both * scale;
        } else if (a.mode == SDSP_HIP_CFAR_GO) {
            th = ((lag > lead) ? lag : lead) * scale;
        } else {
            th = ((lag < lead) ? lag : lead) * scale;
        }
    }
    if (th != th) { // a NaN threshold is the canonical quiet NaN
        const K quiet = sizeof(K) == 4 ? K(0x7FC00000u) : K(0x7FF8000000000000ull);
        __builtin_memcpy(&th, &quiet, sizeof(th));
    }
    if (a.thr)
        static_cast<R *>(a.thr)[c * a.thr_stride + n] = th;
    if (a.det)
        a.det[c * a.det_stride + n] = cell(half) > th ? 1 : 0;
}

int padded_for(uint32_t cells) { return cells <= 8 ? 8 : cells <= 16 ? 16 : cells <= 32 ? 32 : cells <= 64 ? 64 : cells <= 128 ? 128 : 256; }

// waves per SIMD of sdsp_cfar_os_kernel by its registers (profiles/cfar_kernel_regs.txt)
uint32_t occupancy_for(int precision, int wp)
{
    if (precision == SDSP_HIP_F64)
        return wp <= 32 ? 4u : wp <= 64 ? 2u : 1u;
    return wp <= 32 ? 4u : wp <= 128 ? 3u : 1u;
}

// f(R(), WP)
template <typename F> int with_os_kernel(int precision, uint32_t cells, F f)
{
    auto by_wp = [&](auto r) {
        switch (padded_for(cells)) {
        case 8:
            return f(r, std::integral_constant<int, 8>());
        case 16:
            return f(r, std::integral_constant<int, 16>());
        case 32:
            return f(r, std::integral_constant<int, 32>());
        case 64:
            return f(r, std::integral_constant<int, 64>());
        case 128:
            return f(r, std::integral_constant<int, 128>());
        default:
            if constexpr (sizeof(r) == 8)
                return static_cast<int>(fail(SDSP_HIP_ERR_INVALID_SIZE, "cfar: more than 127 training cells for OS in F64"));
            else
                return f(r, std::integral_constant<int, 256>());
        }
    };
    return precision == SDSP_HIP_F64 ? by_wp(double()) : by_wp(float());
}
} // namespace

uint32_t cfar_padded(uint32_t cells) { return static_cast<uint32_t>(padded_for(cells)); }

uint32_t cfar_block(int precision, int mode)
{
    if (mode == SDSP_HIP_CFAR_OS)
        return static_cast<uint32_t>(precision == SDSP_HIP_F64 ? os_block<double>() : os_block<float>());
    return static_cast<uint32_t>(precision == SDSP_HIP_F64 ? seg_max<double>() : seg_max<float>());
}

uint32_t cfar_lds_bytes(int precision, int mode)
{
    const uint32_t es = precision == SDSP_HIP_F64 ? 8u : 4u, b = cfar_block(precision, mode);
    if (mode == SDSP_HIP_CFAR_OS)
        return 5 * b * kPitch * es + 2 * kLanes * 4;
    return static_cast<uint32_t>(padded_size(static_cast<int>(b) + kMaxLead + kWin) + padded_size(static_cast<int>(b) + kMaxLag + kWin)) * es;
}

const char *cfar_kernel_for(int variant, int mode)
{
    return variant == 1 ? "sdsp_cfar_plain_kernel" : mode == SDSP_HIP_CFAR_OS ? "sdsp_cfar_os_kernel" : "sdsp_cfar_sum_kernel";
}

// The run of a call.  OS: the rank bank's rule -- enough lanes for 1024 SIMDs at the kernel's occupancy, runs of at least four windows
// (the W - 1 cells in front of a run are then a fifth of its work at the most), a multiple of 16.  Sum modes: the largest segment the
// LDS arrays hold, shortened (to four windows or 256 outputs at the least, a multiple of 16) while the call has fewer than 2048
// workgroups.
uint32_t cfar_auto_run(int precision, int mode, uint64_t channels, uint64_t samples, uint32_t train, uint32_t guard)
{
    if (samples == 0)
        return 0;
    const uint64_t window = 2ull * (train + guard) + 1;
    uint64_t run;
    if (mode == SDSP_HIP_CFAR_OS) {
        const uint64_t lanes = 1024ull * kLanes * occupancy_for(precision, padded_for(2 * train));
        const uint64_t per_row = (lanes + channels - 1) / channels;
        run = (samples + per_row - 1) / per_row;
        if (run < 4 * window)
            run = 4 * window;
        run = (run + 15) / 16 * 16;
    } else {
        const uint64_t top = cfar_block(precision, mode);
        const uint64_t per_row = (2048 + channels - 1) / channels;
        run = (samples + per_row - 1) / per_row;
        const uint64_t low = 4 * window < 256 ? 256 : 4 * window;
        if (run < low)
            run = low;
        run = (run + 15) / 16 * 16;
        if (run > top)
            run = top;
    }
    return static_cast<uint32_t>(run < samples ? run : samples);
}

int launch_cfar(int precision, const cfar_args &ca, int variant, void *stream_v)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const bool os = ca.mode == SDSP_HIP_CFAR_OS, f64 = precision == SDSP_HIP_F64;
    cfar_kargs k{};
    k.x = ca.x;
    k.thr = ca.thr;
    k.det = static_cast<uint8_t *>(ca.det);
    k.hist = ca.hist;
    k.channels = ca.channels;
    k.x_stride = ca.x_stride;
    k.thr_stride = ca.thr_stride;
    k.det_stride = ca.det_stride;
    k.scale = ca.scale;
    k.samples = static_cast<uint32_t>(ca.samples);
    k.train = ca.train;
    k.guard = ca.guard;
    k.mode = static_cast<uint32_t>(ca.mode);
    k.rank = ca.rank;
    k.iq = ca.iq ? 1u : 0u;
    k.run = ca.run;
    dim3 grid;
    if (variant == 1) {
        k.runs_per_row = 1;
        if (int rc = grid_for(ca.channels * ca.samples, "cfar", &grid))
            return rc;
        if (f64)
            hipLaunchKernelGGL(sdsp_cfar_plain_kernel<double>, grid, dim3(kThreads), 0, stream, k);
        else
            hipLaunchKernelGGL(sdsp_cfar_plain_kernel<float>, grid, dim3(kThreads), 0, stream, k);
        return launch_status("cfar");
    }
    if (!os && k.run > cfar_block(precision, ca.mode)) // the LDS arrays of sdsp_cfar_sum_kernel hold no more
        k.run = cfar_block(precision, ca.mode);
    if (k.run == 0 || ca.train == 0 || ca.train > 128 || ca.guard > 255)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "cfar: run, train or guard out of range");
    k.runs_per_row = static_cast<uint32_t>((ca.samples + k.run - 1) / k.run);
    if (os) {
        if (int rc = grid_of_blocks((ca.channels * k.runs_per_row + kLanes - 1) / kLanes, "cfar", &grid))
            return rc;
        if (int rc = with_os_kernel(precision, 2 * ca.train, [&](auto r, auto wp) {
                hipLaunchKernelGGL((sdsp_cfar_os_kernel<decltype(r), decltype(wp)::value>), grid, dim3(kLanes), 0, stream, k);
                return static_cast<int>(SDSP_HIP_OK);
            }))
            return rc;
        return launch_status("cfar");
    }
    if (int rc = grid_of_blocks(ca.channels * k.runs_per_row, "cfar", &grid))
        return rc;
    if (f64)
        hipLaunchKernelGGL(sdsp_cfar_sum_kernel<double>, grid, dim3(kThreads), 0, stream, k);
    else
        hipLaunchKernelGGL(sdsp_cfar_sum_kernel<float>, grid, dim3(kThreads), 0, stream, k);
    return launch_status("cfar");
}
} // namespace sdsp_hip
