// rank_filter.hip -- streaming rank-order filter banks (running median, minimum, maximum, any rank) for MI355X (gfx950): many
// independent real rows, each output the element of rank r of the last W inputs.
//
// Output n of a row (x_c = the row's history, then the block):  y[n] = the element of rank r, counted from 0 and ascending, of the W
// values x_c[n - W + 1 .. n].  The order is IEEE 754 totalOrder, through the key of a value's bits u:  key = ~u if the sign bit is
// set, else u | signbit; keys compare as unsigned integers.  Nothing is computed: every output is one of the inputs, bit for bit.
// DESIGN.md section 5.26.
//
// Two kernels:
//   sdsp_rank_kernel        variant 0.  One wave per workgroup, one lane per *run*: `run` consecutive outputs of one row.  A lane keeps
//                           its window as a sorted array of WP keys (8, 16 .. 256; WP >= W) in registers: the W keys of the window and,
//                           above them, WP - W sentinels of key all-ones.  One output is one fully unrolled pass with static indices:
//                           delete one copy of the departing key, insert the arriving one (sorted_step).  The output is the element at
//                           index r, read through a wave-uniform switch over compile-time indices, so the array never leaves the
//                           registers.  A run starts from W keys of value 0 and inserts the W - 1 samples in front of it (the row's
//                           history or x itself) with 0 as the departing key: the bits cannot depend on `run`.
//                           Rows go through LDS transposed ([time][lane], pitch 65) in blocks of B samples: the arriving keys in one
//                           tile, the departing keys (the same input, W samples earlier) in a second one, so LDS does not grow with W.
//                           Both are read with 16-byte loads where a chunk is whole and aligned; the outputs take the place of the
//                           arriving keys and leave the same way.  Values become keys on the way into LDS and values again on the way
//                           out of the pass.  Small arrays (PREFETCH, FAST) keep the next block's loads in flight during the passes and
//                           address the blocks inside a run's interior from bases fixed before the loop.
//   sdsp_rank_plain_kernel  variant 1: one thread per output straight from global memory, selection by counting (for every candidate
//                           the keys that are smaller plus the equal keys at an earlier position; the candidate whose count is r).
//                           O(W^2) per output: the independent cross-check.
// The new history is carry_history's (stream_carry.hip), launched by the caller behind either kernel.
#include "stream_dev.h"

#include <type_traits>

namespace sdsp_hip
{
namespace
{
constexpr int kLanes = 64;         // one wave per workgroup, one lane per run
constexpr int kPitch = kLanes + 1; // elements between two LDS rows: the transposing accesses spread over the banks

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

struct rank_kargs {
    const void *x;
    void *y;
    const void *hist; // nullable: channels x (W - 1) elements, newest first
    uint64_t channels, x_stride, y_stride;
    uint32_t samples, window, rank, run, runs_per_row;
};

// samples per block: four 16-byte chunks of a row
template <typename R> constexpr int block_for() { return 4 * static_cast<int>(16 / sizeof(R)); }

// the middle one of a <= b and v: v clamped to [a, b]
__device__ __forceinline__ uint32_t clamp_between(uint32_t a, uint32_t b, uint32_t v)
{
    uint32_t r; // one instruction; the compiler has no builtin for it and does not form it from min and max of three variables
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(v));
    return r;
}
__device__ __forceinline__ uint64_t clamp_between(uint64_t a, uint64_t b, uint64_t v)
{
    const uint64_t lo = v < a ? a : v;
    return b < lo ? b : lo;
}

// One output: the sorted array loses one copy of `old` and gains `v`.  With t = the array without that copy (t[i] = s[i] where
// s[i] < old, else s[i + 1]; s[WP] counts as all-ones), the new element i is v clamped to [t[i - 1], t[i]] (t[-1] counts as 0): t[i]
// where t[i] <= v, v where t[i - 1] <= v < t[i], t[i - 1] where v < t[i - 1].  Every new element is one of s[i - 1], s[i], s[i + 1], v.
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
#define SDSP_RANK_CASE1(i)                                                                                                             \
    case (i):                                                                                                                          \
        if constexpr ((i) < WP)                                                                                                        \
            out = s[(i) < WP ? (i) : 0];                                                                                               \
        break;
#define SDSP_RANK_CASE4(i) SDSP_RANK_CASE1(i) SDSP_RANK_CASE1((i) + 1) SDSP_RANK_CASE1((i) + 2) SDSP_RANK_CASE1((i) + 3)
#define SDSP_RANK_CASE16(i) SDSP_RANK_CASE4(i) SDSP_RANK_CASE4((i) + 4) SDSP_RANK_CASE4((i) + 8) SDSP_RANK_CASE4((i) + 12)
#define SDSP_RANK_CASE64(i) SDSP_RANK_CASE16(i) SDSP_RANK_CASE16((i) + 16) SDSP_RANK_CASE16((i) + 32) SDSP_RANK_CASE16((i) + 48)
template <typename K, int WP> __device__ __forceinline__ K element_at(const K (&s)[WP], uint32_t idx)
{
    K out = s[0];
    switch (idx) {
        SDSP_RANK_CASE64(0)
        SDSP_RANK_CASE64(64)
        SDSP_RANK_CASE64(128)
        SDSP_RANK_CASE64(192)
    default:
        break;
    }
    return out;
}
#undef SDSP_RANK_CASE64
#undef SDSP_RANK_CASE16
#undef SDSP_RANK_CASE4
#undef SDSP_RANK_CASE1

// A lane's stream: index j counts from the first of `lead` idle steps (they make the 16-byte chunks of a block start on multiples of
// what 16 bytes hold when the run length is such a multiple), then the W - 1 samples in front of the run, then the run.  Index j is
// position p0 + j of the row (p0 = start - (W - 1) - lead); positions below 0 are the history.  An idle step has key 0 arriving and
// departing, which leaves the array as it is.
template <typename R> struct lane_stream {
    using K = typename key_of<R>::type;
    using V = typename vec16<K>::type;
    static constexpr int EL = 16 / sizeof(R);

    // the bits of indices j .. j + EL of the lane that owns (row c, first output `start`), all-ones (the value of key 0) for an idle
    // index; `start` >= samples: a lane without a run.  The caller turns them into keys when it needs them, so that a load issued
    // here can stay in flight.
    static __device__ __forceinline__ V values(const rank_kargs &a, uint32_t c, uint32_t start, int64_t j, int lead)
    {
        V r;
#pragma unroll
        for (int e = 0; e < EL; e++)
            r[e] = static_cast<K>(~K(0));
        if (start >= a.samples || j + EL <= lead)
            return r;
        const K *row = static_cast<const K *>(a.x) + static_cast<uint64_t>(c) * a.x_stride;
        const int64_t p = static_cast<int64_t>(start) - (a.window - 1) - lead + j;
        if (j >= lead && p >= 0 && p + EL <= static_cast<int64_t>(a.samples) && (reinterpret_cast<uintptr_t>(row + p) & 15u) == 0)
            return *reinterpret_cast<const V *>(row + p);
        const K *h = a.hist ? static_cast<const K *>(a.hist) + static_cast<uint64_t>(c) * (a.window - 1) : nullptr;
#pragma unroll
        for (int e = 0; e < EL; e++) {
            const int64_t pe = p + e;
            if (j + e < lead)
                continue; // idle
            K u = K(0);   // +0 in front of a stream without history; past the row: never part of an output
            if (pe >= static_cast<int64_t>(a.samples))
                u = K(0);
            else if (pe >= 0)
                u = row[pe];
            else if (h)
                u = h[-1 - pe]; // pe >= -(W - 1) because j + e >= lead
            r[e] = u;
        }
        return r;
    }
};

template <typename R, int WP> __global__ __launch_bounds__(kLanes) void sdsp_rank_kernel(rank_kargs a)
{
    using K = typename key_of<R>::type;
    using LS = lane_stream<R>;
    using V = typename LS::V;
    constexpr int EL = LS::EL, B = block_for<R>(), CPR = B / EL;
    // small arrays, where the staging costs as much as the passes and registers are free: the next block's loads in flight during the
    // passes, and one access per chunk at a fixed base inside a run's interior
    constexpr bool PREFETCH = WP * sizeof(K) <= 32 * 4, FAST = PREFETCH;
    __shared__ K arrive[B * kPitch];         // [time][lane]; the outputs take the arriving keys' places
    __shared__ K depart[(B + EL) * kPitch];  // the same stream W + dshift indices earlier
    __shared__ uint32_t row_of[kLanes], start_of[kLanes];
    const uint32_t lane = threadIdx.x, W = a.window;
    const int lead = static_cast<int>((EL - (W - 1) % EL) % EL), dshift = static_cast<int>((EL - W % EL) % EL);
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
        s[i] = static_cast<uint32_t>(i) < W ? K(0) : static_cast<K>(~K(0));
    __syncthreads();
    const int64_t total = static_cast<int64_t>(lead) + (W - 1) + a.run; // steps of every lane of the grid
    // The blocks j0 in [jlo, jhi] (wave-uniform; none when jlo > jhi) are the interior of every run of this wave: all their chunks,
    // arriving, departing and leaving, lie inside the run's row, are whole and 16-byte aligned, so each is one access at a base fixed
    // here plus j0.  A lane's own bounds first, then the wave's through LDS (the tiles are not in use yet).
    uint32_t jlo = 1, jhi = 0;
    {
        const uint32_t st = start_of[lane];
        if (st < a.samples) {
            const int64_t p0 = static_cast<int64_t>(st) - (W - 1) - lead;
            const uint64_t end = static_cast<uint64_t>(st) + a.run < a.samples ? static_cast<uint64_t>(st) + a.run : a.samples;
            const intptr_t xr = reinterpret_cast<intptr_t>(static_cast<const K *>(a.x) + static_cast<uint64_t>(row_of[lane]) * a.x_stride);
            const intptr_t yr = reinterpret_cast<intptr_t>(static_cast<K *>(a.y) + static_cast<uint64_t>(row_of[lane]) * a.y_stride);
            const int64_t es = static_cast<int64_t>(sizeof(K));
            // arriving: j0 >= lead; departing: j0 - W - dshift >= lead and p0 + j0 - W - dshift >= 0; leaving: p0 + j0 >= st; all:
            // p0 + j0 + B <= end
            int64_t l = static_cast<int64_t>(lead) + W + dshift;
            l = l < static_cast<int64_t>(W) + dshift - p0 ? static_cast<int64_t>(W) + dshift - p0 : l;
            const int64_t h = static_cast<int64_t>(end) - B - p0;
            if (((xr + p0 * es) & 15) == 0 && ((yr + p0 * es) & 15) == 0 && h >= l) {
                jlo = static_cast<uint32_t>(l);
                jhi = static_cast<uint32_t>(h); // < 2^31 + W + 16
            }
        }
        uint32_t *bounds = reinterpret_cast<uint32_t *>(depart);
        bounds[lane] = jlo;
        bounds[kLanes + lane] = jhi;
        __syncthreads();
        for (int o = 0; o < kLanes; o++) {
            jlo = bounds[o] > jlo ? bounds[o] : jlo;
            jhi = bounds[kLanes + o] < jhi ? bounds[kLanes + o] : jhi;
        }
        __syncthreads();
        jlo = __builtin_amdgcn_readfirstlane(jlo);
        jhi = __builtin_amdgcn_readfirstlane(jhi);
    }
    auto interior = [&](int64_t j0) { return FAST && j0 >= static_cast<int64_t>(jlo) && j0 <= static_cast<int64_t>(jhi); };
    // chunk q = i 64 + lane of a tile is chunk q % n of lane q / n (n = the tile's chunks per lane).  Arriving: indices j0 ..; departing:
    // row i + dshift holds index j0 + i - W, and in front of the stream (and of its idle steps) key 0, the array's filling.  The bases
    // are where index 0 of the chunk would lie; they are only used inside the interior.
    const K *abase[CPR], *dbase[CPR + 1];
    K *ybase[CPR];
#pragma unroll
    for (int i = 0; i < CPR; i++) {
        const uint32_t q = static_cast<uint32_t>(i) * kLanes + lane, o = q / CPR, k = q % CPR;
        const int64_t off = static_cast<int64_t>(start_of[o]) - (W - 1) - lead + k * EL;
        abase[i] = static_cast<const K *>(a.x) + (static_cast<int64_t>(static_cast<uint64_t>(row_of[o]) * a.x_stride) + off);
        ybase[i] = static_cast<K *>(a.y) + (static_cast<int64_t>(static_cast<uint64_t>(row_of[o]) * a.y_stride) + off);
    }
#pragma unroll
    for (int i = 0; i < CPR + 1; i++) {
        const uint32_t q = static_cast<uint32_t>(i) * kLanes + lane, o = q / (CPR + 1), k = q % (CPR + 1);
        const int64_t off = static_cast<int64_t>(start_of[o]) - (W - 1) - lead - static_cast<int64_t>(W) - dshift + k * EL;
        dbase[i] = static_cast<const K *>(a.x) + (static_cast<int64_t>(static_cast<uint64_t>(row_of[o]) * a.x_stride) + off);
    }
    V av[CPR], dv[CPR + 1];
    auto fetch = [&](int64_t j0) {
        if (interior(j0)) {
#pragma unroll
            for (int i = 0; i < CPR; i++)
                av[i] = *reinterpret_cast<const V *>(abase[i] + j0);
#pragma unroll
            for (int i = 0; i < CPR + 1; i++)
                dv[i] = *reinterpret_cast<const V *>(dbase[i] + j0);
            return;
        }
#pragma unroll
        for (int i = 0; i < CPR; i++) {
            const uint32_t q = static_cast<uint32_t>(i) * kLanes + lane, o = q / CPR, k = q % CPR;
            av[i] = LS::values(a, row_of[o], start_of[o], j0 + k * EL, lead);
        }
#pragma unroll
        for (int i = 0; i < CPR + 1; i++) {
            const uint32_t q = static_cast<uint32_t>(i) * kLanes + lane, o = q / (CPR + 1), k = q % (CPR + 1);
            dv[i] = LS::values(a, row_of[o], start_of[o], j0 - static_cast<int64_t>(W) - dshift + k * EL, lead);
        }
    };
    if constexpr (PREFETCH)
        fetch(0);
    for (int64_t j0 = 0; j0 < total; j0 += B) {
        const int len = total - j0 < B ? static_cast<int>(total - j0) : B;
        if constexpr (!PREFETCH)
            fetch(j0);
#pragma unroll
        for (int i = 0; i < CPR; i++) {
            const uint32_t q = static_cast<uint32_t>(i) * kLanes + lane, o = q / CPR, k = q % CPR;
#pragma unroll
            for (int e = 0; e < EL; e++)
                arrive[(k * EL + e) * kPitch + o] = to_key<K>(av[i][e]);
        }
#pragma unroll
        for (int i = 0; i < CPR + 1; i++) {
            const uint32_t q = static_cast<uint32_t>(i) * kLanes + lane, o = q / (CPR + 1), k = q % (CPR + 1);
#pragma unroll
            for (int e = 0; e < EL; e++)
                depart[(k * EL + e) * kPitch + o] = to_key<K>(dv[i][e]);
        }
        __syncthreads();
        if constexpr (PREFETCH) // the next block's loads are in flight while this one computes
            if (j0 + B < total)
                fetch(j0 + B);
        // the lane's own column from here to the barrier
        for (int i = 0; i < len; i++) {
            sorted_step<K, WP>(s, depart[(i + dshift) * kPitch + lane], arrive[i * kPitch + lane]);
            arrive[i * kPitch + lane] = from_key<K>(element_at<K, WP>(s, a.rank));
        }
        __syncthreads();
        // outputs: index j is output p0 + j of the row, for the positions of the lane's run
#pragma unroll
        for (int i = 0; i < CPR; i++) {
            const uint32_t q = static_cast<uint32_t>(i) * kLanes + lane, o = q / CPR, k = q % CPR;
            if (interior(j0)) {
                V v;
#pragma unroll
                for (int e = 0; e < EL; e++)
                    v[e] = arrive[(k * EL + e) * kPitch + o];
                __builtin_nontemporal_store(v, reinterpret_cast<V *>(ybase[i] + j0));
                continue;
            }
            const uint32_t start = start_of[o];
            if (start >= a.samples)
                continue;
            const uint64_t end = static_cast<uint64_t>(start) + a.run < a.samples ? static_cast<uint64_t>(start) + a.run : a.samples;
            const int64_t p = static_cast<int64_t>(start) - (W - 1) - lead + j0 + k * EL;
            if (p + EL <= static_cast<int64_t>(start) || p >= static_cast<int64_t>(end))
                continue;
            K *out = static_cast<K *>(a.y) + static_cast<uint64_t>(row_of[o]) * a.y_stride;
            if (p >= static_cast<int64_t>(start) && p + EL <= static_cast<int64_t>(end) && (reinterpret_cast<uintptr_t>(out + p) & 15u) == 0) {
                V v;
#pragma unroll
                for (int e = 0; e < EL; e++)
                    v[e] = arrive[(k * EL + e) * kPitch + o];
                __builtin_nontemporal_store(v, reinterpret_cast<V *>(out + p));
            } else {
#pragma unroll
                for (int e = 0; e < EL; e++)
                    if (p + e >= static_cast<int64_t>(start) && p + e < static_cast<int64_t>(end))
                        __builtin_nontemporal_store(arrive[(k * EL + e) * kPitch + o], out + p + e);
            }
        }
        __syncthreads();
    }
}

// ---- variant 1: one thread per output from global memory, selection by counting ---------------------------------------------------------
template <typename R> __global__ __launch_bounds__(kThreads) void sdsp_rank_plain_kernel(rank_kargs a)
{
    using K = typename key_of<R>::type;
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= a.channels * a.samples)
        return;
    const uint64_t c = udiv(i, a.samples), n = i - c * a.samples;
    const uint32_t W = a.window;
    const K *row = static_cast<const K *>(a.x) + c * a.x_stride;
    const K *h = a.hist ? static_cast<const K *>(a.hist) + c * (W - 1) : nullptr;
    auto key_at = [&](uint32_t t) -> K { // x_c[n - t]; t - n - 1 <= W - 2
        return to_key<K>(n >= t ? row[n - t] : (h ? h[t - n - 1] : K(0)));
    };
    K found = K(0);
    for (uint32_t t = 0; t < W; t++) {
        const K cand = key_at(t);
        uint32_t below = 0;
        for (uint32_t q = 0; q < W; q++) { // q > t lies earlier in time
            const K other = key_at(q);
            below += (other < cand || (other == cand && q > t)) ? 1u : 0u;
        }
        if (below == a.rank)
            found = cand;
    }
    static_cast<K *>(a.y)[c * a.y_stride + n] = from_key<K>(found);
}

int padded_for(uint32_t window) { return window <= 8 ? 8 : window <= 16 ? 16 : window <= 32 ? 32 : window <= 64 ? 64 : window <= 128 ? 128 : 256; }

// waves per SIMD of sdsp_rank_kernel by its registers (profiles/rank_filter_kernel_regs.txt)
uint32_t occupancy_for(int precision, int wp)
{
    if (precision == SDSP_HIP_F64)
        return wp <= 32 ? 3u : wp <= 64 ? 2u : 1u;
    return wp <= 8 ? 4u : wp <= 64 ? 3u : wp <= 128 ? 2u : 1u;
}

// f(R(), WP)
template <typename F> int with_kernel(int precision, uint32_t window, F f)
{
    auto by_wp = [&](auto r) {
        switch (padded_for(window)) {
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
                return static_cast<int>(fail(SDSP_HIP_ERR_INVALID_SIZE, "rank: a window above 127 for F64"));
            else
                return f(r, std::integral_constant<int, 256>());
        }
    };
    return precision == SDSP_HIP_F64 ? by_wp(double()) : by_wp(float());
}
} // namespace

uint32_t rank_padded(uint32_t window) { return static_cast<uint32_t>(padded_for(window)); }

uint32_t rank_block(int precision) { return static_cast<uint32_t>(precision == SDSP_HIP_F64 ? block_for<double>() : block_for<float>()); }

uint32_t rank_lds_bytes(int precision)
{
    const uint32_t es = precision == SDSP_HIP_F64 ? 8u : 4u, b = rank_block(precision);
    return (2 * b + 16 / es) * kPitch * es + 2 * kLanes * 4;
}

const char *rank_kernel_for(int variant) { return variant == 1 ? "sdsp_rank_plain_kernel" : "sdsp_rank_kernel"; }

// The run of a call: enough lanes for 1024 SIMDs at the kernel's occupancy, runs of at least four windows (the W - 1 samples in front
// of a run are then a fifth of its work at the most), a multiple of 16 samples so that every run starts where a 16-byte chunk does.
uint32_t rank_auto_run(int precision, uint64_t channels, uint64_t samples, uint32_t window)
{
    if (samples == 0)
        return 0;
    const uint64_t lanes = 1024ull * kLanes * occupancy_for(precision, padded_for(window));
    const uint64_t per_row = (lanes + channels - 1) / channels;
    uint64_t run = (samples + per_row - 1) / per_row;
    if (run < 4ull * window)
        run = 4ull * window;
    run = (run + 15) / 16 * 16;
    return static_cast<uint32_t>(run < samples ? run : samples);
}

int launch_rank(int precision, const rank_args &ra, int variant, void *stream_v)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    rank_kargs k{};
    k.x = ra.x;
    k.y = ra.y;
    k.hist = ra.window > 1 ? ra.hist : nullptr;
    k.channels = ra.channels;
    k.x_stride = ra.x_stride;
    k.y_stride = ra.y_stride;
    k.samples = static_cast<uint32_t>(ra.samples);
    k.window = ra.window;
    k.rank = ra.rank;
    k.run = ra.run;
    k.runs_per_row = static_cast<uint32_t>((ra.samples + ra.run - 1) / ra.run);
    dim3 grid;
    if (variant == 1) {
        if (int rc = grid_for(ra.channels * ra.samples, "rank", &grid))
            return rc;
        if (precision == SDSP_HIP_F64)
            hipLaunchKernelGGL(sdsp_rank_plain_kernel<double>, grid, dim3(kThreads), 0, stream, k);
        else
            hipLaunchKernelGGL(sdsp_rank_plain_kernel<float>, grid, dim3(kThreads), 0, stream, k);
        return launch_status("rank");
    }
    if (int rc = grid_of_blocks((ra.channels * k.runs_per_row + kLanes - 1) / kLanes, "rank", &grid))
        return rc;
    if (int rc = with_kernel(precision, ra.window, [&](auto r, auto wp) {
            hipLaunchKernelGGL((sdsp_rank_kernel<decltype(r), decltype(wp)::value>), grid, dim3(kLanes), 0, stream, k);
            return static_cast<int>(SDSP_HIP_OK);
        }))
        return rc;
    return launch_status("rank");
}
} // namespace sdsp_hip
