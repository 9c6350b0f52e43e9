// welch.hip -- the kernels of the Welch PSD bank (sdsp_hip_welch_*).
//
// One sdsp_hip_welch_process call runs as slices of frame -> transform -> run -> combine launches over the plan's workspace, then
// the history update (stream_carry.hip: carry_history, hist = N - 1).  The unit of work is one segment of N reals of one channel; units are
// numbered channel-major (g = c F + j, F segments per channel in the call) and a slice is a contiguous range of them.
//
//   sdsp_welch_frame    detrended, windowed segment j of channel c into the workspace (N reals per unit).  x is the channel's
//                       history followed by the block: x[p] = state[c (N-1) + N - 2 - p] for p < N - 1, else in[c in_stride + p -
//                       N + 1]; segment j starts at p = off0 + j hop.  2^lc threads per unit (at most 256, so 256 >> lc units per
//                       workgroup), each holding nq = N / (VEC 2^lc) vectors of VEC samples: vector q of thread t is samples
//                       [(q 2^lc + t) VEC, + VEC).  DETREND_NONE is one pass.  CONSTANT / LINEAR: each thread sums its samples in
//                       double in (q, lane) order, the lanes of a unit add theirs in an xor butterfly (masks 1, 2, 4 .. 32), and
//                       units wider than a wave add the waves' sums in ascending order through LDS; then the subtract-and-window
//                       pass runs from registers (nq <= 8, template K = nq) or re-reads the segment, which the first pass left in
//                       the caches (K = 0).  Workgroups are ordered so that neighbouring units, which overlap, share an XCD
//                       (stream_dev.h: xcd_block).
//   (the plan's forward real-input transform of n_real = N, radix 2, in place on the slice: unchanged kernels)
//   sdsp_welch_run      one thread per (run, packed bin k < N/2): a run is up to R consecutive segments of one channel in the slice;
//                       it sums p = re re + im im in double in ascending segment order (k = 0: re^2 for bin 0 and im^2 for N/2)
//                       and writes one partial per bin.
//   sdsp_welch_combine  one thread per (channel of the slice, bin): that channel's partials of the slice added in ascending run order,
//                       then one addition into acc.  No atomics: every acc element has one owner per slice.
//   sdsp_welch_finalize out = round_p(acc c_k), elementwise.
// This file is compiled with -ffp-contract=off: every product and sum above is rounded on its own.
#include "stream_dev.h"

namespace sdsp_hip
{
namespace
{
constexpr int kBatch = 8; // run and combine stages: loads in flight per thread

// one slice's view of the call; the slice's first unit is segment j0 of channel c0
struct wl_view {
    uint64_t in_stride;
    uint64_t c0;
    uint32_t j0, frames; // frames: segments per channel in the call (F)
    uint32_t units;      // units in the slice
    uint32_t n, hop, off0, hist; // off0: x offset of the call's first segment; hist = N - 1
    uint32_t lc;         // log2(threads per unit)
    uint32_t vec_ok;     // `in` and in_stride keep 16-B alignment of element offsets that are multiples of the vector width
    double denom;        // N (N^2 - 1) / 12
};

// the slice's runs: the first channel's [j0, first_end) in runs_first runs of R from j0; the channels after it in runs of R from
// segment 0, rpc runs each (the last one, channel last_cc of the slice, ends at jend)
struct wl_runs {
    uint64_t runs;
    uint32_t frames, j0, first_end, jend, run, rpc, runs_first, runs_last, last_cc, bins, half, lk;
};

template <typename R>
__device__ __forceinline__ R load_x(const wl_view &v, const R *in, const R *state, uint64_t c, uint64_t p)
{
    if (p < v.hist)
        return state[c * v.hist + (v.hist - 1 - p)]; // only reached with position > 0, where state is required
    return in[c * v.in_stride + (p - v.hist)];
}

template <typename R>
__device__ __forceinline__ typename vec16<R>::type load_vec(const wl_view &v, const R *in, const R *state, uint64_t c, uint64_t p0)
{
    using V = typename vec16<R>::type;
    constexpr int VEC = vec16<R>::lanes;
    V x;
    const uint64_t off = c * v.in_stride + (p0 - v.hist);
    if (v.vec_ok && p0 >= v.hist && off % VEC == 0) {
        x = *reinterpret_cast<const V *>(in + off);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; e++)
            x[e] = load_x(v, in, state, c, p0 + e);
    }
    return x;
}

template <typename R, int DT, int K>
__global__ __launch_bounds__(kThreads) void sdsp_welch_frame(wl_view v, const R *__restrict__ in, const R *__restrict__ state,
                                                             const R *__restrict__ window, R *__restrict__ ws)
{
    using V = typename vec16<R>::type;
    constexpr int VEC = vec16<R>::lanes;
    const uint32_t tpu = 1u << v.lc;
    const uint64_t u = (static_cast<uint64_t>(xcd_block(blockIdx.x, gridDim.x)) << (8 - v.lc)) + (threadIdx.x >> v.lc);
    const uint32_t t = threadIdx.x & (tpu - 1);
    const bool live = u < v.units;
    uint64_t c = 0;
    uint32_t j = 0;
    if (live) {
        const uint32_t g = v.j0 + static_cast<uint32_t>(u); // < F + units < 2^32 (checked by the launcher)
        const uint32_t dc = g / v.frames;
        c = v.c0 + dc;
        j = g - dc * v.frames;
    }
    const uint64_t p0 = v.off0 + static_cast<uint64_t>(j) * v.hop;
    const uint32_t nq = v.n / (VEC * tpu);
    R *dst = ws + u * v.n;
    if (DT == SDSP_HIP_DETREND_NONE) {
        if (!live)
            return;
        for (uint32_t q = 0; q < nq; q++) {
            const uint32_t i0 = (q * tpu + t) * VEC;
            const V x = load_vec(v, in, state, c, p0 + i0);
            const V w = *reinterpret_cast<const V *>(window + i0);
            V y;
#pragma unroll
            for (int e = 0; e < VEC; e++)
                y[e] = x[e] * w[e];
            *reinterpret_cast<V *>(dst + i0) = y;
        }
        return;
    }
    const double mid = 0.5 * static_cast<double>(v.n - 1);
    double s0 = 0.0, s1 = 0.0;
    V xr[K > 0 ? K : 1];
    auto add = [&](const V &x, uint32_t i0) {
#pragma unroll
        for (int e = 0; e < VEC; e++) {
            const double xd = static_cast<double>(x[e]);
            s0 += xd;
            if (DT == SDSP_HIP_DETREND_LINEAR)
                s1 += (static_cast<double>(i0 + e) - mid) * xd;
        }
    };
    if (live) {
        if (K > 0) {
#pragma unroll
            for (int q = 0; q < K; q++) {
                const uint32_t i0 = (q * tpu + t) * VEC;
                xr[q] = load_vec(v, in, state, c, p0 + i0);
                add(xr[q], i0);
            }
        } else {
            for (uint32_t q = 0; q < nq; q++) {
                const uint32_t i0 = (q * tpu + t) * VEC;
                add(load_vec(v, in, state, c, p0 + i0), i0);
            }
        }
    }
    // the unit's lanes (all lanes of the wave take part: the masks stay inside a unit's 2^lc lanes)
    const uint32_t wl = tpu < 64 ? tpu : 64;
    for (uint32_t m = 1; m < wl; m <<= 1) {
        s0 += __shfl_xor(s0, m);
        if (DT == SDSP_HIP_DETREND_LINEAR)
            s1 += __shfl_xor(s1, m);
    }
    if (tpu > 64) { // 128 or 256 threads per unit: the waves' sums in ascending order
        __shared__ double red[kThreads / 64][2];
        const uint32_t w = threadIdx.x >> 6, wpu = tpu >> 6, wb = w & ~(wpu - 1);
        if ((threadIdx.x & 63) == 0) {
            red[w][0] = s0;
            red[w][1] = s1;
        }
        __syncthreads();
        s0 = red[wb][0];
        s1 = red[wb][1];
        for (uint32_t i = 1; i < wpu; i++) {
            s0 += red[wb + i][0];
            s1 += red[wb + i][1];
        }
    }
    if (!live)
        return;
    const double mu = s0 / static_cast<double>(v.n);
    const double beta = DT == SDSP_HIP_DETREND_LINEAR ? s1 / v.denom : 0.0;
    auto emit = [&](const V &x, uint32_t i0) {
        const V w = *reinterpret_cast<const V *>(window + i0);
        V y;
#pragma unroll
        for (int e = 0; e < VEC; e++) {
            double tr = mu;
            if (DT == SDSP_HIP_DETREND_LINEAR)
                tr = mu + beta * (static_cast<double>(i0 + e) - mid);
            const R d = static_cast<R>(static_cast<double>(x[e]) - tr);
            y[e] = d * w[e];
        }
        *reinterpret_cast<V *>(dst + i0) = y;
    };
    if (K > 0) {
#pragma unroll
        for (int q = 0; q < K; q++)
            emit(xr[q], (q * tpu + t) * VEC);
    } else {
        for (uint32_t q = 0; q < nq; q++) {
            const uint32_t i0 = (q * tpu + t) * VEC;
            emit(load_vec(v, in, state, c, p0 + i0), i0);
        }
    }
}

template <typename R>
__global__ __launch_bounds__(kThreads) void sdsp_welch_run(wl_runs r, const R *__restrict__ ws, double *__restrict__ part)
{
    using C2 = typename cplx_pair<R>::type;
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t rid = gid >> r.lk;
    if (rid >= r.runs)
        return;
    const uint32_t k = static_cast<uint32_t>(gid & (r.half - 1));
    uint32_t cc, ja, jb;
    if (rid < r.runs_first) {
        cc = 0;
        ja = r.j0 + static_cast<uint32_t>(rid) * r.run;
        jb = min(ja + r.run, r.first_end);
    } else {
        const uint32_t q = static_cast<uint32_t>(rid - r.runs_first), d = q / r.rpc;
        cc = 1 + d;
        ja = (q - d * r.rpc) * r.run;
        jb = min(ja + r.run, cc == r.last_cc ? r.jend : r.frames);
    }
    const uint64_t u = static_cast<uint64_t>(cc) * r.frames + ja - r.j0; // the run's first unit in the slice
    const C2 *z = reinterpret_cast<const C2 *>(ws + u * (2ull * r.half)) + k;
    double *o = part + rid * r.bins;
    // loads in batches of kBatch (independent of the sums, so their latencies overlap), additions in segment order
    double s = 0.0, sn = 0.0;
    uint32_t f = ja;
    for (; f + kBatch <= jb; f += kBatch, z += kBatch * r.half) {
        double re[kBatch], im[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; i++) {
            const C2 q = z[static_cast<uint64_t>(i) * r.half];
            re[i] = static_cast<double>(q[0]);
            im[i] = static_cast<double>(q[1]);
        }
        if (k == 0) {
#pragma unroll
            for (int i = 0; i < kBatch; i++) {
                s += re[i] * re[i];
                sn += im[i] * im[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < kBatch; i++)
                s += re[i] * re[i] + im[i] * im[i];
        }
    }
    for (; f < jb; f++, z += r.half) {
        const C2 q = *z;
        const double re = static_cast<double>(q[0]), im = static_cast<double>(q[1]);
        if (k == 0) {
            s += re * re;
            sn += im * im;
        } else {
            s += re * re + im * im;
        }
    }
    o[k] = s;
    if (k == 0)
        o[r.half] = sn;
}

__global__ __launch_bounds__(kThreads) void sdsp_welch_combine(wl_runs r, uint64_t nch, uint64_t c0, const double *__restrict__ part,
                                                               double *__restrict__ acc, uint64_t acc_stride)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (gid >= nch * r.bins)
        return;
    const uint64_t cc = gid / r.bins, k = gid - cc * r.bins;
    uint64_t r0;
    uint32_t nr;
    if (cc == 0) {
        r0 = 0;
        nr = r.runs_first;
    } else {
        r0 = r.runs_first + (cc - 1) * r.rpc;
        nr = cc == r.last_cc ? r.runs_last : r.rpc;
    }
    const double *p = part + r0 * r.bins + k;
    double s = p[0];
    uint32_t i = 1;
    for (; i + kBatch <= nr; i += kBatch) { // loads in batches, additions in run order
        double q[kBatch];
#pragma unroll
        for (int e = 0; e < kBatch; e++)
            q[e] = p[static_cast<uint64_t>(i + e) * r.bins];
#pragma unroll
        for (int e = 0; e < kBatch; e++)
            s += q[e];
    }
    for (; i < nr; i++)
        s += p[static_cast<uint64_t>(i) * r.bins];
    acc[(c0 + cc) * acc_stride + k] += s;
}

template <typename R>
__global__ __launch_bounds__(kThreads) void sdsp_welch_finalize(const double *__restrict__ acc, R *__restrict__ out, uint64_t acc_stride,
                                                                uint64_t out_stride, uint64_t channels, uint32_t bins, double c_edge,
                                                                double c_mid)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (gid >= channels * bins)
        return;
    const uint64_t c = gid / bins, k = gid - c * bins;
    const double ck = (k == 0 || k == bins - 1) ? c_edge : c_mid;
    out[c * out_stride + k] = static_cast<R>(acc[c * acc_stride + k] * ck);
}

uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

template <typename R, int DT> void frame_launch(int K, dim3 grid, const wl_view &v, const R *in, const R *st, const R *w, R *ws,
                                                hipStream_t s)
{
    switch (K) {
    case 1: hipLaunchKernelGGL((sdsp_welch_frame<R, DT, 1>), grid, dim3(kThreads), 0, s, v, in, st, w, ws); break;
    case 2: hipLaunchKernelGGL((sdsp_welch_frame<R, DT, 2>), grid, dim3(kThreads), 0, s, v, in, st, w, ws); break;
    case 4: hipLaunchKernelGGL((sdsp_welch_frame<R, DT, 4>), grid, dim3(kThreads), 0, s, v, in, st, w, ws); break;
    case 8: hipLaunchKernelGGL((sdsp_welch_frame<R, DT, 8>), grid, dim3(kThreads), 0, s, v, in, st, w, ws); break;
    default: hipLaunchKernelGGL((sdsp_welch_frame<R, DT, 0>), grid, dim3(kThreads), 0, s, v, in, st, w, ws); break;
    }
}

// the runs of the slice [g0, g0 + units) (wl_runs above)
wl_runs slice_runs(const welch_args &a)
{
    wl_runs r{};
    const uint64_t F = a.frames, c0 = a.g0 / F, clast = (a.g0 + a.units - 1) / F;
    r.frames = a.frames;
    r.j0 = static_cast<uint32_t>(a.g0 - c0 * F);
    r.jend = static_cast<uint32_t>(a.g0 + a.units - clast * F);
    r.first_end = clast == c0 ? r.jend : a.frames;
    r.run = a.run;
    r.rpc = static_cast<uint32_t>(ceil_div(F, a.run));
    r.runs_first = static_cast<uint32_t>(ceil_div(r.first_end - r.j0, a.run));
    r.last_cc = static_cast<uint32_t>(clast - c0);
    r.runs_last = clast == c0 ? r.runs_first : static_cast<uint32_t>(ceil_div(r.jend, a.run));
    r.runs = clast == c0 ? r.runs_first : r.runs_first + (clast - c0 - 1) * r.rpc + r.runs_last;
    r.half = a.n / 2;
    r.bins = a.n / 2 + 1;
    r.lk = log2u(r.half);
    return r;
}

template <typename R> int launch(const welch_args &a, int step, hipStream_t stream)
{
    constexpr int VEC = vec16<R>::lanes;
    dim3 grid;
    if (step == WELCH_FINALIZE) {
        if (int rc = grid_for(a.channels * (a.n / 2 + 1), "welch finalize", &grid))
            return rc;
        hipLaunchKernelGGL(sdsp_welch_finalize<R>, grid, dim3(kThreads), 0, stream, a.acc, static_cast<R *>(a.out), a.acc_stride,
                           a.out_stride, a.channels, a.n / 2 + 1, a.c_edge, a.c_mid);
    } else if (step == WELCH_FRAME) {
        if (static_cast<uint64_t>(a.frames) + a.units >= (1ull << 32))
            return fail(SDSP_HIP_ERR_UNSUPPORTED, "welch slice: too many segments per channel");
        wl_view v{};
        v.in_stride = a.in_stride;
        v.c0 = a.g0 / a.frames;
        v.j0 = static_cast<uint32_t>(a.g0 - v.c0 * a.frames);
        v.frames = a.frames;
        v.units = a.units;
        v.n = a.n;
        v.hop = a.hop;
        v.off0 = a.off0;
        v.hist = a.n - 1;
        v.vec_ok = (reinterpret_cast<uintptr_t>(a.in) % 16 == 0 && (a.in_stride * sizeof(R)) % 16 == 0) ? 1 : 0;
        v.lc = log2u(std::min<uint32_t>(a.n / VEC, kThreads));
        v.denom = static_cast<double>(a.n) * (static_cast<double>(a.n) * a.n - 1.0) / 12.0; // exact: N (N^2 - 1) is a multiple of 12
        const uint32_t nq = a.n / (VEC << v.lc);
        const int K = nq <= 8 ? static_cast<int>(nq) : 0;
        if (int rc = grid_of_blocks(ceil_div(a.units, kThreads >> v.lc), "welch slice", &grid))
            return rc;
        const R *in = static_cast<const R *>(a.in), *st = static_cast<const R *>(a.state), *w = static_cast<const R *>(a.window);
        R *ws = static_cast<R *>(a.ws);
        if (a.detrend == SDSP_HIP_DETREND_NONE) // one pass: nothing to keep in registers
            hipLaunchKernelGGL((sdsp_welch_frame<R, SDSP_HIP_DETREND_NONE, 0>), grid, dim3(kThreads), 0, stream, v, in, st, w, ws);
        else if (a.detrend == SDSP_HIP_DETREND_CONSTANT)
            frame_launch<R, SDSP_HIP_DETREND_CONSTANT>(K, grid, v, in, st, w, ws, stream);
        else
            frame_launch<R, SDSP_HIP_DETREND_LINEAR>(K, grid, v, in, st, w, ws, stream);
    } else {
        const wl_runs r = slice_runs(a);
        if (step == WELCH_RUN) {
            if (int rc = grid_for(r.runs << r.lk, "welch slice", &grid))
                return rc;
            hipLaunchKernelGGL(sdsp_welch_run<R>, grid, dim3(kThreads), 0, stream, r, static_cast<const R *>(a.ws), a.part);
        } else {
            const uint64_t nch = r.last_cc + 1ull;
            if (int rc = grid_for(nch * r.bins, "welch slice", &grid))
                return rc;
            hipLaunchKernelGGL(sdsp_welch_combine, grid, dim3(kThreads), 0, stream, r, nch, a.g0 / a.frames,
                               static_cast<const double *>(a.part), a.acc, a.acc_stride);
        }
    }
    return launch_status("welch");
}
} // namespace

int launch_welch(int precision, const welch_args &a, int step, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    return precision == SDSP_HIP_F64 ? launch<double>(a, step, s) : launch<float>(a, step, s);
}
} // namespace sdsp_hip
