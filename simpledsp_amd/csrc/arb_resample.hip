// arb_resample.hip -- arbitrary-ratio polyphase resampler banks for MI355X (gfx950): L phases of T taps, nearest phase or linear
// interpolation between two, any step in Q32.32 input samples per output.
//
// Output m of a call (x = the channel's history, then the block; t = time + m step in unsigned 64-bit integers):
//     i = t >> 32, f = t & 0xffffffff, p = f >> (32 - log2 L), r = f & (2^(32 - log2 L) - 1), mu = fl(r) 2^-(32 - log2 L)
//     a = H[p][0] x[i], then a = fmaf(H[p][k], x[i - k], a) for k = 1 .. T - 1 (f64: a multiply then an add); b the same over Dt
//     y = a (nearest) or fmaf(mu, b, a) (linear; f64: a + mu b with two roundings); complex input: both planes alike
// H and Dt come rounded from the plan (capi.hip); built with -ffp-contract=off, so nothing here contracts.  DESIGN.md section 5.21.
//
// Two kernels:
//   sdsp_arb_kernel        variant 0.  A workgroup copies the tap table into LDS once -- for linear plans as interleaved (H, Dt)
//                          pairs, so one 8- or 16-byte read serves both sums, rows padded to an odd number of entries so that lanes
//                          on different phases of one tap spread over the banks -- and then walks a run of consecutive blocks of
//                          block_out outputs of one channel.  Per block the 64-bit times of the first and the last output give the
//                          input span, which is staged in LDS (16-byte nontemporal loads where the row allows, the part in front
//                          of the row from `state`); a lane computes t, i, p and mu once per output, runs the T-tap loop from LDS
//                          and stores; consecutive lanes own consecutive outputs.
//   sdsp_arb_plain_kernel  variant 1: one output per thread straight from global memory, the independent cross-check.
// The new history is carry_history's (stream_carry.hip), launched by the caller behind either kernel.
#include "stream_dev.h"

#include <type_traits>

namespace sdsp_hip
{
namespace
{
constexpr uint32_t kMaxBlockOut = 1024;      // outputs per block: four per lane
constexpr size_t kLdsSmall = 32 * 1024;      // table + line target for tables up to 8 KiB (five workgroups per CU)
constexpr size_t kLdsMid = 64 * 1024;        // ... up to 32 KiB (two workgroups per CU)
constexpr size_t kLdsLarge = 144 * 1024;     // ... above: one workgroup per CU; a 64 KiB table and a line of T + 1 = 4097 f64 pairs fit
constexpr size_t kLdsLimit = kLdsLarge;      // every instantiation's dynamic-LDS limit, set once per device (arb_prepare)
constexpr uint64_t kTableShare = 16;         // a run streams at least this many times the table's bytes
constexpr uint64_t kMinGroups = 1024;        // ... unless that leaves fewer workgroups than this

typedef cplx_pair<float>::type f2;
typedef cplx_pair<double>::type d2;

// one input element: a real, or an interleaved complex pair; one table entry: H, or the pair (H, Dt)
template <typename R, bool PAIR> struct maybe_pair {
    typedef R type;
};
template <typename R> struct maybe_pair<R, true> {
    typedef typename cplx_pair<R>::type type;
};

// the contract's steps on one element (both planes of a pair alike)
__device__ __forceinline__ float mul(float g, float x) { return g * x; }
__device__ __forceinline__ double mul(double g, double x) { return g * x; }
__device__ __forceinline__ f2 mul(float g, f2 x)
{
    f2 r;
    r.x = g * x.x;
    r.y = g * x.y;
    return r;
}
__device__ __forceinline__ d2 mul(double g, d2 x)
{
    d2 r;
    r.x = g * x.x;
    r.y = g * x.y;
    return r;
}
__device__ __forceinline__ float madd(float g, float x, float a) { return __builtin_fmaf(g, x, a); }
__device__ __forceinline__ double madd(double g, double x, double a) { return a + g * x; }
__device__ __forceinline__ f2 madd(float g, f2 x, f2 a)
{
    f2 r;
    r.x = __builtin_fmaf(g, x.x, a.x);
    r.y = __builtin_fmaf(g, x.y, a.y);
    return r;
}
__device__ __forceinline__ d2 madd(double g, d2 x, d2 a)
{
    d2 r;
    r.x = a.x + g * x.x;
    r.y = a.y + g * x.y;
    return r;
}
// y = a + mu b, by the same rule
__device__ __forceinline__ float lerp(float mu, float b, float a) { return __builtin_fmaf(mu, b, a); }
__device__ __forceinline__ double lerp(double mu, double b, double a) { return a + mu * b; }
__device__ __forceinline__ f2 lerp(float mu, f2 b, f2 a)
{
    f2 r;
    r.x = __builtin_fmaf(mu, b.x, a.x);
    r.y = __builtin_fmaf(mu, b.y, a.y);
    return r;
}
__device__ __forceinline__ d2 lerp(double mu, d2 b, d2 a)
{
    d2 r;
    r.x = a.x + mu * b.x;
    r.y = a.y + mu * b.y;
    return r;
}

struct arb_kargs {
    const void *in;
    void *out;
    const void *state;
    const void *table; // [phase][tap] entries, unpadded
    uint64_t in_stride, out_stride, step, time;
    double mu_scale;     // 2^-(32 - lb)
    uint32_t n_out, channels;
    uint32_t taps, hist, phases;
    uint32_t pshift;     // 32 - lb
    uint32_t rmask;      // 2^(32 - lb) - 1
    uint32_t blk_out;    // outputs per block
    uint32_t nblk;       // blocks per channel
    uint32_t run, nrun;  // blocks per workgroup, workgroups per channel
    uint32_t row_stride; // LDS table: entries per phase row
    uint32_t line_off;   // bytes from the start of LDS to the line (a multiple of 16)
    uint32_t vec_in;     // rows 16-byte aligned
};

// phase and fraction of a time's low word
__device__ __forceinline__ uint32_t phase_of(const arb_kargs &a, uint32_t f) { return static_cast<uint32_t>(static_cast<uint64_t>(f) >> a.pshift); }
template <typename R> __device__ __forceinline__ R mu_of(const arb_kargs &a, uint32_t f)
{
    return static_cast<R>(f & a.rmask) * static_cast<R>(a.mu_scale); // the conversion rounds to nearest even; the scaling is exact
}

template <typename R, bool CPLX, bool LINEAR> __global__ __launch_bounds__(kThreads) void sdsp_arb_kernel(arb_kargs a)
{
    using E = typename maybe_pair<R, CPLX>::type;
    using W = typename maybe_pair<R, LINEAR>::type;
    using V = typename vec16<R>::type;
    constexpr uint32_t EL = 16 / sizeof(E); // elements per 16-byte load
    extern __shared__ __align__(16) unsigned char lds_raw[];
    W *tab = reinterpret_cast<W *>(lds_raw);
    E *line = reinterpret_cast<E *>(lds_raw + a.line_off); // x[g0 ..] of the current block

    const uint32_t wg = xcd_block(blockIdx.x, gridDim.x); // neighbouring runs of a channel behind one L2: their spans overlap by T - 1
    const uint32_t c = wg / a.nrun, rn = wg - c * a.nrun;
    const uint32_t t = threadIdx.x, T = a.taps, H = a.hist;
    const E *row = static_cast<const E *>(a.in) + static_cast<uint64_t>(c) * a.in_stride;
    const E *st = a.state ? static_cast<const E *>(a.state) + static_cast<uint64_t>(c) * H : nullptr;
    E *dst = static_cast<E *>(a.out) + static_cast<uint64_t>(c) * a.out_stride;

    {
        const W *g = static_cast<const W *>(a.table);
        const uint32_t entries = a.phases * T;
        for (uint32_t e = t; e < entries; e += kThreads) {
            const uint32_t p = e / T, k = e - p * T;
            tab[p * a.row_stride + k] = g[e];
        }
    }

    const uint32_t b0 = rn * a.run, b1 = min(b0 + a.run, a.nblk); // both below 2^31
    for (uint32_t blk = b0; blk < b1; blk++) {
        const uint32_t m0 = blk * a.blk_out;
        const uint32_t no = min(a.blk_out, a.n_out - m0);
        const uint64_t t0 = a.time + static_cast<uint64_t>(m0) * a.step;        // valid outputs: below samples 2^32 < 2^63
        const uint64_t t1 = t0 + static_cast<uint64_t>(no - 1) * a.step;
        const uint32_t i0 = static_cast<uint32_t>(t0 >> 32), i1 = static_cast<uint32_t>(t1 >> 32); // i0 <= i1 < samples < 2^31
        const int64_t g0 = static_cast<int64_t>(i0) - H;                                           // line[e] = x[g0 + e]
        const uint32_t before = g0 < 0 ? static_cast<uint32_t>(-g0) : 0;                           // elements in front of the row
        const uint32_t jlo = g0 < 0 ? 0 : static_cast<uint32_t>(g0), jhi = i1 + 1;                 // the row's part: [jlo, jhi)

        __syncthreads(); // the block before this one has been read
        for (uint32_t e = t; e < before; e += kThreads)
            line[e] = st ? st[before - 1 - e] : E(0); // x[g0 + e] = state[-1 - (g0 + e)]
        E *ln = line + (static_cast<int64_t>(before) - jlo); // ln[j] = x[j] for j in [jlo, jhi)
        if (a.vec_in) {
            uint32_t v0 = (jlo + EL - 1) / EL * EL; // the 16-byte aligned middle [v0, v1)
            if (v0 > jhi)
                v0 = jhi;
            const uint32_t nv = (jhi - v0) / EL, v1 = v0 + nv * EL;
            const V *src = reinterpret_cast<const V *>(row + v0);
            for (uint32_t i = t; i < nv; i += kThreads) {
                const V v = __builtin_nontemporal_load(src + i);
#pragma unroll
                for (uint32_t e = 0; e < EL; e++) {
                    E x;
                    if constexpr (CPLX) {
                        x.x = v[2 * e];
                        x.y = v[2 * e + 1];
                    } else {
                        x = v[e];
                    }
                    ln[v0 + i * EL + e] = x;
                }
            }
            if (t < v0 - jlo) // fewer than EL each
                ln[jlo + t] = row[jlo + t];
            if (t < jhi - v1)
                ln[v1 + t] = row[v1 + t];
        } else {
            for (uint32_t j = jlo + t; j < jhi; j += kThreads)
                ln[j] = row[j];
        }
        __syncthreads();

        for (uint32_t o = t; o < no; o += kThreads) { // lanes past the block compute nothing
            const uint64_t tt = t0 + static_cast<uint64_t>(o) * a.step;
            const uint32_t i = static_cast<uint32_t>(tt >> 32), f = static_cast<uint32_t>(tt);
            const W *w = tab + phase_of(a, f) * a.row_stride;
            const E *x = line + (i - i0) + H; // x[0] = x_c[i]; x[-k] reaches back to line[i - i0 + H - (T - 1)] >= line[0]
            E y;
            if constexpr (LINEAR) {
                W g = w[0];
                E xa = x[0];
                E s = mul(g.x, xa), d = mul(g.y, xa);
#pragma unroll 4
                for (uint32_t k = 1; k < T; k++) {
                    g = w[k];
                    xa = *(x - k);
                    s = madd(g.x, xa, s);
                    d = madd(g.y, xa, d);
                }
                y = lerp(mu_of<R>(a, f), d, s);
            } else {
                E s = mul(w[0], x[0]);
#pragma unroll 4
                for (uint32_t k = 1; k < T; k++)
                    s = madd(w[k], *(x - k), s);
                y = s;
            }
            __builtin_nontemporal_store(y, dst + m0 + o);
        }
    }
}

// ---- variant 1: one output per thread from global memory ----------------------------------------------------------------------
template <typename R, bool CPLX, bool LINEAR> __global__ __launch_bounds__(kThreads) void sdsp_arb_plain_kernel(arb_kargs a)
{
    using E = typename maybe_pair<R, CPLX>::type;
    using W = typename maybe_pair<R, LINEAR>::type;
    const uint64_t total = static_cast<uint64_t>(a.channels) * a.n_out;
    const uint32_t T = a.taps, H = a.hist;
    for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; idx < total;
         idx += static_cast<uint64_t>(gridDim.x) * kThreads) {
        const uint64_t c = udiv(idx, a.n_out), m = idx - c * a.n_out;
        const uint64_t tt = a.time + m * a.step;
        const int64_t i = static_cast<int64_t>(tt >> 32);
        const uint32_t f = static_cast<uint32_t>(tt);
        const E *inp = static_cast<const E *>(a.in) + c * a.in_stride;
        const E *st = a.state ? static_cast<const E *>(a.state) + c * H : nullptr;
        const W *w = static_cast<const W *>(a.table) + static_cast<size_t>(phase_of(a, f)) * T;
        auto x_at = [&](uint32_t k) {
            const int64_t xi = i - static_cast<int64_t>(k);
            return xi >= 0 ? inp[xi] : (st ? st[-1 - xi] : E(0)); // -1 - xi < H: k <= T - 1
        };
        E y;
        if constexpr (LINEAR) {
            W g = w[0];
            E xa = x_at(0);
            E s = mul(g.x, xa), d = mul(g.y, xa);
            for (uint32_t k = 1; k < T; k++) {
                g = w[k];
                xa = x_at(k);
                s = madd(g.x, xa, s);
                d = madd(g.y, xa, d);
            }
            y = lerp(mu_of<R>(a, f), d, s);
        } else {
            E s = mul(w[0], x_at(0));
            for (uint32_t k = 1; k < T; k++)
                s = madd(w[k], x_at(k), s);
            y = s;
        }
        static_cast<E *>(a.out)[c * a.out_stride + m] = y;
    }
}

size_t real_bytes(int precision) { return precision == SDSP_HIP_F64 ? 8 : 4; }

// LDS table: entries per phase row.  An odd count puts the lanes of an access group, which sit on scattered phases of one tap, on
// different banks (the entry is 1, 2 or 4 dwords wide); a single row needs none
uint32_t row_stride_for(uint32_t phases, uint32_t taps) { return phases > 1 ? (taps | 1u) : taps; }

size_t table_bytes_for(int precision, int linear, uint32_t phases, uint32_t taps)
{
    const size_t b = static_cast<size_t>(phases) * row_stride_for(phases, taps) * real_bytes(precision) * (linear ? 2 : 1);
    return (b + 15) / 16 * 16;
}

// elements of the staged span of `outs` consecutive outputs at `step`, at most
uint64_t span_for(uint32_t outs, uint64_t step, uint32_t taps) { return ((static_cast<uint64_t>(outs - 1) * step) >> 32) + taps + 1; }

template <typename F> int with_kernel(int precision, int complex_in, int linear, F f)
{
    auto pick = [&](auto r) {
        if (complex_in)
            return linear ? f(r, std::true_type(), std::true_type()) : f(r, std::true_type(), std::false_type());
        return linear ? f(r, std::false_type(), std::true_type()) : f(r, std::false_type(), std::false_type());
    };
    return precision == SDSP_HIP_F64 ? pick(double()) : pick(float());
}
} // namespace

uint32_t arb_block_out(int precision, int complex_in, int linear, uint32_t phases, uint32_t taps, uint64_t max_step)
{
    const size_t es = real_bytes(precision) * (complex_in ? 2 : 1);
    const size_t tb = table_bytes_for(precision, linear, phases, taps);
    // the smallest target that holds the table and the line of ONE output, taps + 1 elements: a long single row (L = 1, T in the
    // thousands) has a small table and still needs the next target for its line
    const size_t least = tb + static_cast<size_t>(taps + 1) * es;
    const size_t target = (tb <= 8 * 1024 && least <= kLdsSmall) ? kLdsSmall : ((tb <= 32 * 1024 && least <= kLdsMid) ? kLdsMid : kLdsLarge);
    if (least > target)
        return 0; // no plan within the documented limits: the largest is 64 KiB of table and 4097 f64 pairs, 128 KiB and 16 bytes
    const uint64_t q = (target - tb) / es - (taps + 1); // the largest ((b - 1) max_step) >> 32
    const uint64_t b = 1 + (((q + 1) << 32) - 1) / max_step;
    return static_cast<uint32_t>(b < kMaxBlockOut ? b : kMaxBlockOut);
}

int arb_prepare(int precision, int complex_in, int linear)
{
    static std::atomic<uint64_t> done[8];
    return with_kernel(precision, complex_in, linear, [&](auto r, auto cplx, auto lin) {
        constexpr bool c = decltype(cplx)::value, l = decltype(lin)::value;
        return ensure_dynamic_lds(reinterpret_cast<const void *>(sdsp_arb_kernel<decltype(r), c, l>), kLdsLimit,
                                  done[(sizeof(r) == 8 ? 4 : 0) + (c ? 2 : 0) + (l ? 1 : 0)]);
    });
}

const char *arb_kernel_for(int variant) { return variant == 1 ? "sdsp_arb_plain_kernel" : "sdsp_arb_kernel"; }

int launch_arb(int precision, const arb_args &aa, int variant, void *stream_v)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const size_t es = real_bytes(precision) * (aa.complex_in ? 2 : 1);
    uint32_t lb = 0;
    while ((1u << lb) < aa.phases)
        lb++;
    arb_kargs k{};
    k.in = aa.in;
    k.out = aa.out;
    k.table = aa.table;
    k.in_stride = aa.in_stride;
    k.out_stride = aa.out_stride;
    k.step = aa.step;
    k.time = aa.time;
    k.mu_scale = 1.0 / static_cast<double>(1ull << (32 - lb));
    k.n_out = static_cast<uint32_t>(aa.n_out);
    k.channels = static_cast<uint32_t>(aa.channels);
    k.taps = aa.taps;
    k.hist = aa.taps - 1;
    k.state = k.hist ? aa.state : nullptr;
    k.phases = aa.phases;
    k.pshift = 32 - lb;
    k.rmask = static_cast<uint32_t>((1ull << (32 - lb)) - 1);
    k.vec_in = (reinterpret_cast<uintptr_t>(aa.in) % 16 == 0 && (aa.in_stride * es) % 16 == 0) ? 1 : 0;
    if (aa.channels > 0x7fffffffull)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "arb too large for one launch");
    dim3 grid;
    if (variant == 1) {
        const uint64_t total = aa.channels * aa.n_out;
        if (int rc = grid_for(total < (65536ull * kThreads) ? total : 65536ull * kThreads, "arb", &grid)) // grid-stride beyond
            return rc;
        if (int rc = with_kernel(precision, aa.complex_in, aa.linear, [&](auto r, auto cplx, auto lin) {
                hipLaunchKernelGGL((sdsp_arb_plain_kernel<decltype(r), decltype(cplx)::value, decltype(lin)::value>), grid, dim3(kThreads),
                                   0, stream, k);
                return static_cast<int>(SDSP_HIP_OK);
            }))
            return rc;
        return launch_status("arb");
    }
    k.blk_out = aa.block_out; // the plan's, fixed at its creation from max_step
    k.nblk = (k.n_out + k.blk_out - 1) / k.blk_out;
    k.row_stride = row_stride_for(aa.phases, aa.taps);
    const size_t tb = table_bytes_for(precision, aa.linear, aa.phases, aa.taps);
    k.line_off = static_cast<uint32_t>(tb);
    // blocks per workgroup: enough stream bytes behind one copy of the table, while the grid stays wide
    uint64_t run = (kTableShare * tb + static_cast<uint64_t>(k.blk_out) * es - 1) / (static_cast<uint64_t>(k.blk_out) * es);
    if (run > k.nblk)
        run = k.nblk;
    while (run > 1 && aa.channels * ((k.nblk + run - 1) / run) < kMinGroups)
        run = (run + 1) / 2;
    k.run = static_cast<uint32_t>(run);
    k.nrun = (k.nblk + k.run - 1) / k.run;
    if (int rc = grid_of_blocks(aa.channels * k.nrun, "arb", &grid))
        return rc;
    const size_t lds = tb + span_for(k.blk_out, aa.step, aa.taps) * es; // step <= max_step: inside the target block_out was sized for
    if (k.blk_out == 0 || lds > kLdsLimit)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "arb line exceeds the LDS limit"); // a plan is refused at creation before it gets here
    if (int rc = with_kernel(precision, aa.complex_in, aa.linear, [&](auto r, auto cplx, auto lin) {
            hipLaunchKernelGGL((sdsp_arb_kernel<decltype(r), decltype(cplx)::value, decltype(lin)::value>), grid, dim3(kThreads), lds,
                               stream, k);
            return static_cast<int>(SDSP_HIP_OK);
        }))
        return rc;
    return launch_status("arb");
}
} // namespace sdsp_hip
