// lms.hip -- LMS / NLMS adaptive filter banks for MI355X (gfx950): many independent channels, each with its own T weights that move
// with every sample.
//
// Sample n of a channel (x_c = the channel's history, then the block; w = its T weights), in this order:
//     y = +0;  for t ascending: y = w[t] x_c[n - t] + y          one fmaf in f32, a multiply then an add in f64
//     e = d[n] - y
//     LMS:  g = mu e        NLMS:  p = +0;  for t ascending: p = x_c[n - t] x_c[n - t] + p;   g = (mu e) / (eps + p)
//     for t ascending: w[t] = g x_c[n - t] + w[t]
// complex rows: y and the update take the four steps written out in filter_tap and update_tap below.  Built with -ffp-contract=off and
// without fast-math, so nothing here contracts and `/` is the correctly rounded division.  DESIGN.md section 5.25.
//
// Two kernels:
//   sdsp_lms_kernel        variant 0.  One wave per workgroup owns 64 channels, one lane per channel, and walks the whole call in blocks
//                          of B = block_for() samples.  A lane's weights stay in registers from the first sample to the last: the tap loop is
//                          unrolled over the compile-time bound TP (8, 16, 32, 64) and taps t >= T are kept out by wave-uniform tests per group of four (selects inside the last group);
//                          T = TP has an instantiation of its own without tests.
//                          The rows are channel-major, so a block of x and d goes through LDS on its way in and y and e on their way
//                          out: 16-byte nontemporal accesses where a row is 16-byte aligned, neighbouring lanes on one row; element by
//                          element otherwise.  In LDS everything is [time][lane] with a pitch of 65 elements, so a tap's read is
//                          conflict-free and its address is the sample's plus an immediate.  The x window holds T rows in front of the
//                          block, newest row first; y[n] takes the place of the row that sample n needs last, e[n] that of d[n].  The update of sample
//                          n - 1 is fused into the filtering of sample n (one LDS read per tap serves both); the first sample of a
//                          call has nothing pending and the last update is flushed before the weights are stored.  The next block's
//                          global loads are in flight while the current one computes.
//   sdsp_lms_plain_kernel  variant 1: one thread per channel straight from global memory, runtime T, the weights read-modify-written
//                          in `state` (or in the plan's scratch rows when there is no state).  The independent cross-check.
// The new history is carry_history's (stream_carry.hip), launched by the caller behind either kernel.
#include "stream_dev.h"

#include <type_traits>

namespace sdsp_hip
{
namespace
{
constexpr int kLanes = 64;                     // one wave per workgroup, one lane per channel
constexpr int kPitch = kLanes + 1;             // elements between two LDS rows: the transposing accesses spread over the banks
constexpr size_t kLdsPerWave = 160 * 1024 / 4; // four waves per CU at least

template <typename R> __device__ __forceinline__ R mul_add(R g, R x, R acc);
template <> __device__ __forceinline__ float mul_add<float>(float g, float x, float acc) { return __builtin_fmaf(g, x, acc); }
template <> __device__ __forceinline__ double mul_add<double>(double g, double x, double acc) { return acc + g * x; }
template <typename R> __device__ __forceinline__ R mul_sub(R g, R x, R acc);
template <> __device__ __forceinline__ float mul_sub<float>(float g, float x, float acc) { return __builtin_fmaf(-g, x, acc); }
template <> __device__ __forceinline__ double mul_sub<double>(double g, double x, double acc) { return acc - g * x; }

// one element of a row: a real, or an interleaved complex pair
template <typename R, bool CPLX> struct elem {
    typedef R type;
};
template <typename R> struct elem<R, true> {
    typedef typename cplx_pair<R>::type type;
};

template <typename R> __device__ __forceinline__ R re(R x) { return x; }
template <typename R> __device__ __forceinline__ R im(R) { return R(0); }
__device__ __forceinline__ float re(cplx_pair<float>::type x) { return x.x; }
__device__ __forceinline__ float im(cplx_pair<float>::type x) { return x.y; }
__device__ __forceinline__ double re(cplx_pair<double>::type x) { return x.x; }
__device__ __forceinline__ double im(cplx_pair<double>::type x) { return x.y; }

template <typename R, bool CPLX> __device__ __forceinline__ typename elem<R, CPLX>::type make(R r, R i)
{
    typename elem<R, CPLX>::type v;
    if constexpr (CPLX) {
        v.x = r;
        v.y = i;
    } else {
        v = r;
    }
    return v;
}

// y += w x in the contract's order
template <typename R, bool CPLX> __device__ __forceinline__ void filter_tap(R wr, R wi, typename elem<R, CPLX>::type x, R &yr, R &yi)
{
    if constexpr (CPLX) {
        yr = mul_add<R>(wr, x.x, yr);
        yr = mul_sub<R>(wi, x.y, yr);
        yi = mul_add<R>(wr, x.y, yi);
        yi = mul_add<R>(wi, x.x, yi);
    } else {
        yr = mul_add<R>(wr, x, yr);
    }
}
// p += |x|^2
template <typename R, bool CPLX> __device__ __forceinline__ void energy_tap(typename elem<R, CPLX>::type x, R &p)
{
    if constexpr (CPLX) {
        p = mul_add<R>(x.x, x.x, p);
        p = mul_add<R>(x.y, x.y, p);
    } else {
        p = mul_add<R>(x, x, p);
    }
}
// w += g conj(x)
template <typename R, bool CPLX> __device__ __forceinline__ void update_tap(R gr, R gi, typename elem<R, CPLX>::type x, R &wr, R &wi)
{
    if constexpr (CPLX) {
        wr = mul_add<R>(gr, x.x, wr);
        wr = mul_add<R>(gi, x.y, wr);
        wi = mul_add<R>(gi, x.x, wi);
        wi = mul_sub<R>(gr, x.y, wi);
    } else {
        wr = mul_add<R>(gr, x, wr);
    }
}
// steps 2 to 4: e = d - y and the step g of the update
template <typename R, bool CPLX, bool NLMS>
__device__ __forceinline__ void error_and_step(typename elem<R, CPLX>::type d, R yr, R yi, R p, R mu, R eps, R &er, R &ei, R &gr, R &gi)
{
    er = re(d) - yr;
    ei = CPLX ? im(d) - yi : R(0);
    gr = mu * er;
    gi = CPLX ? mu * ei : R(0);
    if constexpr (NLMS) {
        const R q = eps + p;
        gr = gr / q;
        if constexpr (CPLX)
            gi = gi / q;
    }
}

struct lms_kargs {
    const void *x, *d;
    void *y, *e;     // nullable
    void *w;         // channels x T weights (never null for the plain kernel; null = zero weights, nothing kept, for variant 0)
    const void *hist; // nullable: channels x (T - 1) elements of x, newest first
    uint64_t channels, samples, x_stride, d_stride, y_stride, e_stride;
    uint32_t taps;
    double mu, eps; // exactly representable in the plan precision
};

// samples per block of sdsp_lms_kernel: T + 2 B rows of kPitch elements within kLdsPerWave, a multiple of what 16 bytes hold, and
// at most eight 16-byte chunks per row (a lane keeps that many of x and of d for the next block in registers)
constexpr int block_for(size_t es, int tp)
{
    const int rows = static_cast<int>(kLdsPerWave / (kPitch * es)), el = es >= 16 ? 1 : static_cast<int>(16 / es);
    const int b = (rows - tp) / 2 / el * el;
    return b > 8 * el ? 8 * el : b;
}

// the 16-byte chunks of a [64 channels][B samples] tile: chunk q = i * 64 + lane covers channel q / CPR, elements (q % CPR) * EL ..
template <typename R, bool CPLX, int B> struct tile {
    using E = typename elem<R, CPLX>::type;
    using V = typename vec16<R>::type;
    static constexpr int EL = 16 / sizeof(E);   // elements per chunk
    static constexpr int CPR = B / EL;          // chunks per channel and block = chunks per lane
    static constexpr int VL = vec16<R>::lanes;  // reals per chunk

    // block [n0, n0 + B) of the rows at `base` into registers; what lies past the row's samples or the bank's channels is zero
    static __device__ __forceinline__ void load(const E *base, uint64_t stride, uint64_t c0, uint64_t channels, uint64_t n0,
                                                uint64_t samples, V (&v)[CPR])
    {
#pragma unroll
        for (int i = 0; i < CPR; i++) {
            const uint32_t q = static_cast<uint32_t>(i) * kLanes + threadIdx.x, ch = q / CPR, k = q % CPR;
            const uint64_t c = c0 + ch, n = n0 + static_cast<uint64_t>(k) * EL;
            V r;
#pragma unroll
            for (int j = 0; j < VL; j++)
                r[j] = R(0);
            if (c < channels && n < samples) {
                const E *p = base + c * stride + n;
                if (n + EL <= samples && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
                    r = __builtin_nontemporal_load(reinterpret_cast<const V *>(p));
                } else {
#pragma unroll
                    for (int e = 0; e < EL; e++)
                        if (n + e < samples) {
                            const E s = p[e];
                            if constexpr (CPLX) {
                                r[2 * e] = s.x;
                                r[2 * e + 1] = s.y;
                            } else {
                                r[e] = s;
                            }
                        }
                }
            }
            v[i] = r;
        }
    }

    // sample i of the block lives in row i, or in row -i for REV (`rows` is then the row of sample 0, the highest)
    template <bool REV> static __device__ __forceinline__ int row_of(uint32_t i)
    {
        return REV ? -static_cast<int>(i) * kPitch : static_cast<int>(i) * kPitch;
    }

    // registers -> LDS
    template <bool REV> static __device__ __forceinline__ void to_lds(E *rows, const V (&v)[CPR])
    {
#pragma unroll
        for (int i = 0; i < CPR; i++) {
            const uint32_t q = static_cast<uint32_t>(i) * kLanes + threadIdx.x, ch = q / CPR, k = q % CPR;
#pragma unroll
            for (int e = 0; e < EL; e++)
                rows[row_of<REV>(k * EL + e) + static_cast<int>(ch)] = make<R, CPLX>(v[i][CPLX ? 2 * e : e], CPLX ? v[i][2 * e + 1] : R(0));
        }
    }

    // LDS rows -> the first `len` samples of block n0 of the rows at `base`
    template <bool REV>
    static __device__ __forceinline__ void store(const E *rows, E *base, uint64_t stride, uint64_t c0, uint64_t channels, uint64_t n0,
                                                 uint32_t len)
    {
#pragma unroll
        for (int i = 0; i < CPR; i++) {
            const uint32_t q = static_cast<uint32_t>(i) * kLanes + threadIdx.x, ch = q / CPR, k = q % CPR;
            const uint64_t c = c0 + ch;
            if (c >= channels || k * EL >= len)
                continue;
            E *p = base + c * stride + n0 + static_cast<uint64_t>(k) * EL;
            if (k * EL + EL <= len && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
                V r;
#pragma unroll
                for (int e = 0; e < EL; e++) {
                    const E s = rows[row_of<REV>(k * EL + e) + static_cast<int>(ch)];
                    if constexpr (CPLX) {
                        r[2 * e] = s.x;
                        r[2 * e + 1] = s.y;
                    } else {
                        r[e] = s;
                    }
                }
                __builtin_nontemporal_store(r, reinterpret_cast<V *>(p));
            } else {
#pragma unroll
                for (int e = 0; e < EL; e++)
                    if (k * EL + e < len)
                        __builtin_nontemporal_store(rows[row_of<REV>(k * EL + e) + static_cast<int>(ch)], p + e);
            }
        }
    }
};

// One pass over the taps for the sample whose x sits at xn[0] (xn[t kPitch] = x[n - t]: the window is stored newest row first, so
// that a tap's offset is a non-negative immediate).  UPD: the pending update of the sample before
// (w[t] = g x[n - 1 - t] + w[t]) first; FILT: y and, for NLMS, p of this sample with the weights as they then are.  Taps t >= T are
// never touched.  FULL: T = TP, known at compile time: no tests, one basic block, so the LDS reads of a pass can be issued ahead of the
// multiply-adds that use them.
template <typename R, bool CPLX, bool NLMS, int TP, bool FULL, bool UPD, bool FILT>
__device__ __forceinline__ void taps_pass(const typename elem<R, CPLX>::type *xn, uint32_t T, R gr, R gi, R (&wr)[TP], R (&wi)[CPLX ? TP : 1],
                                          R &yr, R &yi, R &p)
{
    using E = typename elem<R, CPLX>::type;
    E v = E(0), vn;
    if constexpr (FILT)
        v = xn[0];
#define SDSP_LMS_TAP(t_, live)                                                                                                            \
    {                                                                                                                                    \
        R &wit = wi[CPLX ? (t_) : 0];                                                                                                    \
        R nwr = wr[t_], nwi = wit, nyr = yr, nyi = yi, np_ = p;                                                                           \
        vn = xn[((t_) + 1) * kPitch];                                                                                                    \
        if constexpr (UPD)                                                                                                               \
            update_tap<R, CPLX>(gr, gi, vn, nwr, nwi);                                                                                   \
        if constexpr (FILT) {                                                                                                            \
            filter_tap<R, CPLX>(nwr, nwi, v, nyr, nyi);                                                                                  \
            if constexpr (NLMS)                                                                                                          \
                energy_tap<R, CPLX>(v, np_);                                                                                             \
            v = vn;                                                                                                                      \
        }                                                                                                                                \
        wr[t_] = (live) ? nwr : wr[t_];                                                                                                  \
        wit = (live) ? nwi : wit;                                                                                                        \
        yr = (live) ? nyr : yr;                                                                                                          \
        yi = (live) ? nyi : yi;                                                                                                          \
        p = (live) ? np_ : p;                                                                                                            \
    }
    // A group of four taps runs whole, or, where T ends inside it, with the results of the taps t >= T thrown away by wave-uniform
    // selects (they read rows past the window, which lie inside the LDS block, and leave w, y and p as they were, bit for bit).  Both
    // branches write the same registers: whatever the compiler merges between them, a weight's register index stays a constant, and
    // the weights stay out of scratch.  No early exit: the trip count is a constant, so the loop unrolls before the weights are
    // split into registers.
#pragma unroll
    for (int t = 0; t < TP; t += 4) {
        if (FULL || static_cast<uint32_t>(t) + 4 <= T) {
            SDSP_LMS_TAP(t, true)
            SDSP_LMS_TAP(t + 1, true)
            SDSP_LMS_TAP(t + 2, true)
            SDSP_LMS_TAP(t + 3, true)
        } else if (static_cast<uint32_t>(t) < T) {
            SDSP_LMS_TAP(t, true)
            SDSP_LMS_TAP(t + 1, static_cast<uint32_t>(t) + 1 < T)
            SDSP_LMS_TAP(t + 2, static_cast<uint32_t>(t) + 2 < T)
            SDSP_LMS_TAP(t + 3, false)
        }
    }
#undef SDSP_LMS_TAP
}

template <typename R, bool CPLX, bool NLMS, int TP, bool FULL> __global__ __launch_bounds__(kLanes) void sdsp_lms_kernel(lms_kargs a)
{
    using E = typename elem<R, CPLX>::type;
    constexpr int B = block_for(sizeof(E), TP);
    static_assert(B >= 3, "a block of at least three rows: the taps thrown away in the last group read up to three rows past the window");
    using TL = tile<R, CPLX, B>;
    using V = typename TL::V;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const uint32_t T = FULL ? TP : a.taps, lane = threadIdx.x;
    // the x window, newest first: row B - 1 - j holds x[n0 + j] for j = -T .. B - 1 (T rows of the past, of which the oldest serves only
    // the pending update); y[n] overwrites x[n0 + n - T], which sample n's pass reads last.  Behind it d, then e in d's place, in time order
    E *xw = reinterpret_cast<E *>(lds_raw);
    E *dw = xw + static_cast<size_t>(T + B) * kPitch;
    E *const x0 = xw + static_cast<size_t>(B - 1) * kPitch;     // the row of x[n0]
    E *const y0 = xw + static_cast<size_t>(B - 1 + T) * kPitch; // the row of y[n0]
    const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * kLanes, c = c0 + lane;
    const bool have = c < a.channels;
    const R mu = static_cast<R>(a.mu), eps = static_cast<R>(a.eps);
    const E *xg = static_cast<const E *>(a.x), *dg = static_cast<const E *>(a.d);

    V xv[TL::CPR], dv[TL::CPR];
    TL::load(xg, a.x_stride, c0, a.channels, 0, a.samples, xv);
    TL::load(dg, a.d_stride, c0, a.channels, 0, a.samples, dv);

    R wr[TP], wi[CPLX ? TP : 1];
    {
        const E *w = have && a.w ? static_cast<const E *>(a.w) + c * T : nullptr;
#pragma unroll
        for (int t = 0; t < TP; t++) {
            const E v = w && static_cast<uint32_t>(t) < T ? w[t] : E(0);
            wr[t] = re(v);
            if constexpr (CPLX)
                wi[t] = im(v);
        }
        if constexpr (!CPLX)
            wi[0] = R(0);
        // the history: x[-1 - j] in row B + j; x[-T] is older than any sample the first pass uses
        const E *h = have && a.hist ? static_cast<const E *>(a.hist) + c * (T - 1) : nullptr;
        for (uint32_t j = 0; j + 1 < T; j++)
            xw[(B + j) * kPitch + lane] = h ? h[j] : E(0);
        xw[(B + T - 1) * kPitch + lane] = E(0);
    }

    R gr = R(0), gi = R(0);
    bool pending = false; // wave-uniform: an update waits to be fused into the next sample's pass
    const uint64_t nblk = (a.samples + B - 1) / B;
    for (uint64_t blk = 0; blk < nblk; blk++) {
        const uint64_t n0 = blk * B;
        const uint32_t len = a.samples - n0 < static_cast<uint64_t>(B) ? static_cast<uint32_t>(a.samples - n0) : B;
        TL::template to_lds<true>(x0, xv);
        TL::template to_lds<false>(dw, dv);
        __syncthreads();
        if (blk + 1 < nblk) {
            TL::load(xg, a.x_stride, c0, a.channels, n0 + B, a.samples, xv);
            TL::load(dg, a.d_stride, c0, a.channels, n0 + B, a.samples, dv);
        }
        // the lane's own column from here to the barrier
        E *xn = x0 + lane;
        for (uint32_t n = 0; n < len; n++, xn -= kPitch) {
            R yr = R(0), yi = R(0), p = R(0), er, ei;
            if (pending)
                taps_pass<R, CPLX, NLMS, TP, FULL, true, true>(xn, T, gr, gi, wr, wi, yr, yi, p);
            else
                taps_pass<R, CPLX, NLMS, TP, FULL, false, true>(xn, T, gr, gi, wr, wi, yr, yi, p);
            pending = true;
            error_and_step<R, CPLX, NLMS>(dw[n * kPitch + lane], yr, yi, p, mu, eps, er, ei, gr, gi);
            xn[T * kPitch] = make<R, CPLX>(yr, yi);
            dw[n * kPitch + lane] = make<R, CPLX>(er, ei);
        }
        __syncthreads();
        if (a.y)
            TL::template store<true>(y0, static_cast<E *>(a.y), a.y_stride, c0, a.channels, n0, len);
        if (a.e)
            TL::template store<false>(dw, static_cast<E *>(a.e), a.e_stride, c0, a.channels, n0, len);
        __syncthreads();
        if (blk + 1 < nblk) {
            // a full block: its last T samples (rows T - 1 .. 0) become the next one's past (rows B + T - 1 .. B), in the lane's own
            // column, oldest first, so that no row is overwritten before it has moved
            for (uint32_t r = T; r-- > 0;)
                xw[(r + B) * kPitch + lane] = xw[r * kPitch + lane];
            __syncthreads();
        } else if (pending) { // the last sample's update: xn is where sample `len` would sit
            R yr, yi, p;
            taps_pass<R, CPLX, NLMS, TP, FULL, true, false>(xn, T, gr, gi, wr, wi, yr, yi, p);
        }
    }
    if (have && a.w) {
        E *w = static_cast<E *>(a.w) + c * T;
#pragma unroll
        for (int t = 0; t < TP; t++)
            if (static_cast<uint32_t>(t) < T)
                w[t] = make<R, CPLX>(wr[t], CPLX ? wi[CPLX ? t : 0] : R(0));
    }
}

// ---- variant 1: one thread per channel from global memory, the weights read-modify-written in a.w ------------------------------------
template <typename R, bool CPLX, bool NLMS> __global__ __launch_bounds__(kThreads) void sdsp_lms_plain_kernel(lms_kargs a)
{
    using E = typename elem<R, CPLX>::type;
    const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (c >= a.channels)
        return;
    const uint32_t T = a.taps;
    const R mu = static_cast<R>(a.mu), eps = static_cast<R>(a.eps);
    const E *x = static_cast<const E *>(a.x) + c * a.x_stride, *d = static_cast<const E *>(a.d) + c * a.d_stride;
    const E *h = a.hist ? static_cast<const E *>(a.hist) + c * (T - 1) : nullptr;
    E *w = static_cast<E *>(a.w) + c * T;
    E *y = a.y ? static_cast<E *>(a.y) + c * a.y_stride : nullptr, *e = a.e ? static_cast<E *>(a.e) + c * a.e_stride : nullptr;
    auto sample = [&](uint64_t n, uint32_t t) -> E { // x[n - t]; t - n - 1 <= T - 2
        return n >= t ? x[n - t] : (h ? h[t - n - 1] : E(0));
    };
    for (uint64_t n = 0; n < a.samples; n++) {
        R yr = R(0), yi = R(0), p = R(0), er, ei, gr, gi;
        for (uint32_t t = 0; t < T; t++) {
            const E wt = w[t], v = sample(n, t);
            filter_tap<R, CPLX>(re(wt), im(wt), v, yr, yi);
            if constexpr (NLMS)
                energy_tap<R, CPLX>(v, p);
        }
        error_and_step<R, CPLX, NLMS>(d[n], yr, yi, p, mu, eps, er, ei, gr, gi);
        for (uint32_t t = 0; t < T; t++) {
            const E wt = w[t];
            R wr = re(wt), wi = im(wt);
            update_tap<R, CPLX>(gr, gi, sample(n, t), wr, wi);
            w[t] = make<R, CPLX>(wr, wi);
        }
        if (y)
            y[n] = make<R, CPLX>(yr, yi);
        if (e)
            e[n] = make<R, CPLX>(er, ei);
    }
}

size_t elem_bytes(int precision, int complex_in) { return (precision == SDSP_HIP_F64 ? 8u : 4u) * (complex_in ? 2u : 1u); }

int tap_bound(uint32_t taps) { return taps <= 8 ? 8 : taps <= 16 ? 16 : taps <= 32 ? 32 : 64; }

// f(R(), complex?, nlms?, TP); F64 COMPLEX stops at 32 taps
template <typename F> int with_kernel(int precision, int complex_in, int nlms, uint32_t taps, F f)
{
    auto by_tp = [&](auto r, auto cplx, auto nl) {
        constexpr bool wide = sizeof(r) == 8 && decltype(cplx)::value;
        switch (tap_bound(taps)) {
        case 8:
            return f(r, cplx, nl, std::integral_constant<int, 8>());
        case 16:
            return f(r, cplx, nl, std::integral_constant<int, 16>());
        case 32:
            return f(r, cplx, nl, std::integral_constant<int, 32>());
        default:
            if constexpr (wide)
                return static_cast<int>(fail(SDSP_HIP_ERR_INVALID_SIZE, "lms: more than 32 taps for F64 COMPLEX"));
            else
                return f(r, cplx, nl, std::integral_constant<int, 64>());
        }
    };
    auto by_mode = [&](auto r, auto cplx) { return nlms ? by_tp(r, cplx, std::true_type()) : by_tp(r, cplx, std::false_type()); };
    if (precision == SDSP_HIP_F64)
        return complex_in ? by_mode(double(), std::true_type()) : by_mode(double(), std::false_type());
    return complex_in ? by_mode(float(), std::true_type()) : by_mode(float(), std::false_type());
}
} // namespace

uint32_t lms_block(int precision, int complex_in, uint32_t taps)
{
    return static_cast<uint32_t>(block_for(elem_bytes(precision, complex_in), tap_bound(taps)));
}

uint32_t lms_lds_bytes(int precision, int complex_in, uint32_t taps)
{
    return static_cast<uint32_t>((taps + 2 * lms_block(precision, complex_in, taps)) * kPitch * elem_bytes(precision, complex_in));
}

const char *lms_kernel_for(int variant) { return variant == 1 ? "sdsp_lms_plain_kernel" : "sdsp_lms_kernel"; }

int launch_lms(int precision, const lms_args &la, int variant, void *stream_v)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    lms_kargs k{};
    k.x = la.x;
    k.d = la.d;
    k.y = la.y;
    k.e = la.e;
    k.w = la.w;
    k.hist = la.taps > 1 ? la.hist : nullptr;
    k.channels = la.channels;
    k.samples = la.samples;
    k.x_stride = la.x_stride;
    k.d_stride = la.d_stride;
    k.y_stride = la.y_stride;
    k.e_stride = la.e_stride;
    k.taps = la.taps;
    k.mu = la.mu;
    k.eps = la.eps;
    dim3 grid;
    if (variant == 1) {
        if (!k.w)
            return fail(SDSP_HIP_ERR_INVALID_ARG, "lms: the plain kernel needs weight rows");
        if (int rc = grid_for(la.channels, "lms", &grid))
            return rc;
        if (int rc = with_kernel(precision, la.complex_in, la.nlms, la.taps, [&](auto r, auto cplx, auto nl, auto) {
                hipLaunchKernelGGL((sdsp_lms_plain_kernel<decltype(r), decltype(cplx)::value, decltype(nl)::value>), grid, dim3(kThreads), 0,
                                   stream, k);
                return static_cast<int>(SDSP_HIP_OK);
            }))
            return rc;
        return launch_status("lms");
    }
    if (int rc = grid_of_blocks((la.channels + kLanes - 1) / kLanes, "lms", &grid))
        return rc;
    const size_t lds = lms_lds_bytes(precision, la.complex_in, la.taps);
    if (int rc = with_kernel(precision, la.complex_in, la.nlms, la.taps, [&](auto r, auto cplx, auto nl, auto tp) {
            constexpr int TP = decltype(tp)::value;
            if (la.taps == static_cast<uint32_t>(TP)) // the tap count is the bound itself: the form without tests
                hipLaunchKernelGGL((sdsp_lms_kernel<decltype(r), decltype(cplx)::value, decltype(nl)::value, TP, true>), grid, dim3(kLanes),
                                   lds, stream, k);
            else
                hipLaunchKernelGGL((sdsp_lms_kernel<decltype(r), decltype(cplx)::value, decltype(nl)::value, TP, false>), grid, dim3(kLanes),
                                   lds, stream, k);
            return static_cast<int>(SDSP_HIP_OK);
        }))
        return rc;
    return launch_status("lms");
}
} // namespace sdsp_hip
