// csd.hip -- the kernels of the cross-spectral density and coherence bank (sdsp_hip_csd_*).
//
// One sdsp_hip_csd_process call runs as slices of frame -> transform -> run -> combine launches over the plan's workspace, then the
// history update (stream_carry.hip: carry_history, hist = N - 1).  A slice is a range [ja, jb) of the call's segments of EVERY channel.
// The frame stage is the Welch bank's (welch.hip: sdsp_welch_frame with frames = jb - ja, off0 advanced by ja hop, g0 = 0 and units =
// channels (jb - ja)), so after the unchanged real-input transform the workspace holds the packed half spectra as
// [channel][segment of the slice][N / 2 complex].
//
//   sdsp_csd_run       one thread per (run, entry, packed bin k < N/2).  An entry is a pair (a, b) of the plan or, when the caller
//                      keeps auto spectra, a channel c as the internal pair (c, c); a run is up to R consecutive segments of the
//                      slice.  With X = (ar, ai) the spectrum of a and Y = (br, bi) that of b widened to double, the thread sums
//                      re = ar br + ai bi and im = ar bi - ai br in ascending segment order (k = 0: re = ar br for bin 0, and ai bi
//                      for bin N/2, both with im = +0) and writes one complex double partial per bin -- an auto entry writes the
//                      real part only, which is the Welch bank's re re + im im.  Consecutive lanes take consecutive bins: both
//                      spectra are read as coalesced 8-byte (f32) or 16-byte (f64) elements, kBatch loads per operand in flight
//                      before the additions.
//                      Order of the workgroups: runs outermost, then the entries sorted by (a, b) with channel c's auto entry behind
//                      the pairs whose a = c, bins innermost; xcd_block (stream_dev.h) gives each XCD one contiguous range of that
//                      order.  So one L2 serves all entries of a few runs -- every channel's R segments of a run are fetched once per
//                      XCD and the other entries that name the channel hit them -- and inside a run the entries that share `a` are
//                      neighbours.
//   sdsp_csd_combine   one thread per (pair or channel, bin): that entry's partials of the slice added in ascending run order, then
//                      one addition into acc_xy (re and im) or acc_auto.  No atomics: every accumulator element has one owner.
//   sdsp_csd_finalize  elementwise.  CROSS: out = round_p(re c_k), round_p(im c_k).  COHERENCE: out = round_p((re re + im im) /
//                      (A_a A_b)), a plain double division (0 / 0 = NaN).
// This file is compiled with -ffp-contract=off: every product and sum above is rounded on its own.
#include "stream_dev.h"

namespace sdsp_hip
{
namespace
{
constexpr int kBatch = 8; // run and combine stages: loads in flight per thread and operand

struct cs_view {
    uint64_t runs;                    // runs of the slice: ceil(frames / run)
    uint32_t frames, run;             // segments per channel in the slice; R
    uint32_t nentries, npairs;        // entries of the run stage; dst >= npairs: the auto entry of channel dst - npairs
    uint32_t bins, half, lk;          // N / 2 + 1, N / 2, log2(N / 2)
};

template <typename R>
__global__ __launch_bounds__(kThreads) void sdsp_csd_run(cs_view v, const R *__restrict__ ws, const uint32_t *__restrict__ entries,
                                                         double *__restrict__ part_xy, double *__restrict__ part_auto)
{
    using C2 = typename cplx_pair<R>::type;
    using D2 = typename vec_n<double, 2>::type;
    const uint64_t gid = static_cast<uint64_t>(xcd_block(blockIdx.x, gridDim.x)) * kThreads + threadIdx.x;
    const uint64_t t = gid >> v.lk;
    const uint64_t rid = udiv(t, v.nentries);
    if (rid >= v.runs)
        return;
    const uint32_t e = static_cast<uint32_t>(t - rid * v.nentries);
    const uint32_t k = static_cast<uint32_t>(gid & (v.half - 1));
    const uint32_t a = entries[3 * e], b = entries[3 * e + 1], dst = entries[3 * e + 2];
    const uint32_t ja = static_cast<uint32_t>(rid) * v.run, jb = min(ja + v.run, v.frames);
    const C2 *za = reinterpret_cast<const C2 *>(ws + (static_cast<uint64_t>(a) * v.frames + ja) * (2ull * v.half)) + k;
    const C2 *zb = reinterpret_cast<const C2 *>(ws + (static_cast<uint64_t>(b) * v.frames + ja) * (2ull * v.half)) + k;
    // loads in batches of kBatch per operand (independent of the sums, so their latencies overlap), additions in segment order
    double sr = 0.0, si = 0.0, sn = 0.0;
    uint32_t f = ja;
    for (; f + kBatch <= jb; f += kBatch, za += kBatch * v.half, zb += kBatch * v.half) {
        C2 x[kBatch], y[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; i++)
            x[i] = za[static_cast<uint64_t>(i) * v.half];
#pragma unroll
        for (int i = 0; i < kBatch; i++)
            y[i] = zb[static_cast<uint64_t>(i) * v.half];
        if (k == 0) {
#pragma unroll
            for (int i = 0; i < kBatch; i++) {
                sr += static_cast<double>(x[i][0]) * static_cast<double>(y[i][0]);
                sn += static_cast<double>(x[i][1]) * static_cast<double>(y[i][1]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < kBatch; i++) {
                const double ar = static_cast<double>(x[i][0]), ai = static_cast<double>(x[i][1]);
                const double br = static_cast<double>(y[i][0]), bi = static_cast<double>(y[i][1]);
                sr += ar * br + ai * bi;
                si += ar * bi - ai * br;
            }
        }
    }
    for (; f < jb; f++, za += v.half, zb += v.half) {
        const C2 x = *za, y = *zb;
        const double ar = static_cast<double>(x[0]), ai = static_cast<double>(x[1]);
        const double br = static_cast<double>(y[0]), bi = static_cast<double>(y[1]);
        if (k == 0) {
            sr += ar * br;
            sn += ai * bi;
        } else {
            sr += ar * br + ai * bi;
            si += ar * bi - ai * br;
        }
    }
    if (dst < v.npairs) {
        D2 *o = reinterpret_cast<D2 *>(part_xy) + (static_cast<uint64_t>(dst) * v.runs + rid) * v.bins;
        D2 q;
        q[0] = sr;
        q[1] = si;
        o[k] = q;
        if (k == 0) {
            q[0] = sn;
            q[1] = 0.0;
            o[v.half] = q;
        }
    } else {
        double *o = part_auto + (static_cast<uint64_t>(dst - v.npairs) * v.runs + rid) * v.bins;
        o[k] = sr;
        if (k == 0)
            o[v.half] = sn;
    }
}

// W doubles per element: 2 for the pairs (re, im), 1 for the auto spectra
template <int W>
__device__ __forceinline__ void combine_row(const cs_view &v, uint64_t row, uint64_t k, const double *__restrict__ part,
                                            double *__restrict__ acc, uint64_t acc_stride)
{
    using DW = typename vec_n<double, W>::type;
    const DW *p = reinterpret_cast<const DW *>(part) + row * v.runs * v.bins + k;
    DW s = p[0];
    uint64_t i = 1;
    for (; i + kBatch <= v.runs; i += kBatch) { // loads in batches, additions in run order
        DW q[kBatch];
#pragma unroll
        for (int e = 0; e < kBatch; e++)
            q[e] = p[(i + e) * v.bins];
#pragma unroll
        for (int e = 0; e < kBatch; e++)
            s += q[e];
    }
    for (; i < v.runs; i++)
        s += p[i * v.bins];
    double *o = acc + row * acc_stride + W * k;
#pragma unroll
    for (int w = 0; w < W; w++)
        o[w] += s[w];
}

__global__ __launch_bounds__(kThreads) void sdsp_csd_combine(cs_view v, uint64_t nauto, const double *__restrict__ part_xy,
                                                             const double *__restrict__ part_auto, double *__restrict__ acc_xy,
                                                             uint64_t acc_xy_stride, double *__restrict__ acc_auto,
                                                             uint64_t acc_auto_stride)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (gid >= (v.npairs + nauto) * v.bins)
        return;
    const uint64_t row = udiv(gid, v.bins), k = gid - row * v.bins;
    if (row < v.npairs)
        combine_row<2>(v, row, k, part_xy, acc_xy, acc_xy_stride);
    else
        combine_row<1>(v, row - v.npairs, k, part_auto, acc_auto, acc_auto_stride);
}

template <typename R>
__global__ __launch_bounds__(kThreads) void sdsp_csd_finalize(const double *__restrict__ acc_xy, const double *__restrict__ acc_auto,
                                                              const uint32_t *__restrict__ pairs, R *__restrict__ out,
                                                              uint64_t acc_xy_stride, uint64_t acc_auto_stride, uint64_t out_stride,
                                                              uint64_t npairs, uint32_t bins, int mode, double c_edge, double c_mid)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (gid >= npairs * bins)
        return;
    const uint64_t i = udiv(gid, bins), k = gid - i * bins;
    const double re = acc_xy[i * acc_xy_stride + 2 * k], im = acc_xy[i * acc_xy_stride + 2 * k + 1];
    if (mode == SDSP_HIP_CSD_CROSS) {
        const double ck = (k == 0 || k == bins - 1) ? c_edge : c_mid;
        out[i * out_stride + 2 * k] = static_cast<R>(re * ck);
        out[i * out_stride + 2 * k + 1] = static_cast<R>(im * ck);
    } else {
        const double pa = acc_auto[pairs[2 * i] * acc_auto_stride + k], pb = acc_auto[pairs[2 * i + 1] * acc_auto_stride + k];
        out[i * out_stride + k] = static_cast<R>((re * re + im * im) / (pa * pb));
    }
}

template <typename R> int launch(const csd_args &a, int step, hipStream_t stream)
{
    dim3 grid;
    const uint32_t bins = a.n / 2 + 1;
    if (step == CSD_FINALIZE) {
        if (int rc = grid_for(static_cast<uint64_t>(a.npairs) * bins, "csd finalize", &grid))
            return rc;
        hipLaunchKernelGGL(sdsp_csd_finalize<R>, grid, dim3(kThreads), 0, stream, a.acc_xy, a.acc_auto, a.table, static_cast<R *>(a.out),
                           a.acc_xy_stride, a.acc_auto_stride, a.out_stride, static_cast<uint64_t>(a.npairs), bins, a.mode, a.c_edge,
                           a.c_mid);
        return launch_status("csd");
    }
    cs_view v{};
    v.frames = a.frames;
    v.run = a.run;
    v.runs = (static_cast<uint64_t>(a.frames) + a.run - 1) / a.run;
    v.nentries = a.nentries;
    v.npairs = a.npairs;
    v.bins = bins;
    v.half = a.n / 2;
    v.lk = log2u(v.half);
    if (step == CSD_RUN) {
        if (int rc = grid_for((v.runs * a.nentries) << v.lk, "csd slice", &grid))
            return rc;
        hipLaunchKernelGGL(sdsp_csd_run<R>, grid, dim3(kThreads), 0, stream, v, static_cast<const R *>(a.ws), a.table, a.part_xy,
                           a.part_auto);
    } else {
        const uint64_t nauto = a.nentries - a.npairs;
        if (int rc = grid_for((a.npairs + nauto) * bins, "csd slice", &grid))
            return rc;
        hipLaunchKernelGGL(sdsp_csd_combine, grid, dim3(kThreads), 0, stream, v, nauto, a.part_xy, a.part_auto, a.acc_xy,
                           a.acc_xy_stride, a.acc_auto, a.acc_auto_stride);
    }
    return launch_status("csd");
}
} // namespace

int launch_csd(int precision, const csd_args &a, int step, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    return precision == SDSP_HIP_F64 ? launch<double>(a, step, s) : launch<float>(a, step, s);
}
} // namespace sdsp_hip
