// fir_fft.hip -- the streaming layer of the FFT-domain FIR plan (overlap-save), DESIGN.md section 5.9.
//
// One sdsp_hip_fir_process call on an FFT plan runs as slices of frame -> convolve -> scatter (-> state) launches over the
// plan's workspace.  The unit of work is a frame PAIR of one channel: frames 2p and 2p+1 (N = fft_n inputs each, hop
// L = N - T + 1) go into the real and the imaginary part of one complex transform; since h is real, the fused convolution
// (sdsp_hip_fft_convolve, unchanged) returns frame 2p's circular convolution in the real and frame 2p+1's in the imaginary
// part.  Units are numbered channel-major (g = c * P + p, P pairs per channel) and a slice is a contiguous range of them.
//
//   sdsp_fir_os_frame   gathers the slice's frame pairs into the workspace (N interleaved complex values per unit); stages the
//                       new history of every channel whose last unit is in the slice (`tails`), and the T-1 inputs in front of
//                       the next slice's first frame when a channel straddles the slice boundary (`carry_out`)
//   sdsp_fir_os_scatter writes outputs [f L, f L + L) of each frame -- points T-1 .. N-1 of its circular convolution -- in place
//   sdsp_fir_os_state   copies the staged tails to `state` after the slice's frame launch (which may still read the old history)
//
// Inputs of a frame: s = f L - (T-1) + i; s < 0 reads the old history (state[c (T-1) + (-1 - s)], newest first), s >= samples
// reads 0, and the straddling channel's [s_b - (T-1), s_b) -- already overwritten by the previous slice's scatter -- reads the
// previous slice's carry.  Every global access is 16 B per lane where the element offset is a multiple of 16 B and the chunk is
// whole; the rest go element by element.
#include "stream_dev.h"

namespace sdsp_hip
{
namespace
{
// one slice's view of the stream; every quantity the kernels derive per unit comes from these
struct os_view {
    uint64_t stride, samples;
    uint64_t frames, pairs; // per channel: F = ceil(samples / L), P = ceil(F / 2)
    uint64_t g0, units;     // the slice: units [g0, g0 + units)
    uint64_t cin_c;         // channel whose [cin_lo, cin_hi) inputs come from carry_in (~0: none)
    int64_t cin_lo, cin_hi;
    uint32_t n, hop, t1;    // N, L, T - 1
    uint32_t lc;            // log2(N / lanes): threads per unit
    uint32_t vec_ok;        // data base and stride keep 16-B alignment of element offsets that are multiples of `lanes`
};

template <typename R> struct os_ptrs {
    R *data;
    const R *state;   // old history (nullable)
    R *ws;            // units x N complex
    R *tails;         // staged new history, (T-1) per channel ending in the slice (nullable: no state)
    const R *carry_in;
    R *carry_out;
};

// the input sample s of channel c as this slice sees it (see the file comment)
template <typename R> __device__ __forceinline__ R load_input(const os_view &v, const os_ptrs<R> &q, uint64_t c, int64_t s)
{
    if (s < 0)
        return q.state ? q.state[c * v.t1 + static_cast<uint64_t>(-1 - s)] : R(0);
    if (static_cast<uint64_t>(s) >= v.samples)
        return R(0);
    if (c == v.cin_c && s >= v.cin_lo && s < v.cin_hi)
        return q.carry_in[s - v.cin_lo];
    return q.data[c * v.stride + static_cast<uint64_t>(s)];
}

// VEC consecutive inputs s0 .. s0+VEC of channel c: one 16-B load when the chunk is plain data and aligned
template <typename R> __device__ __forceinline__ void load_chunk(const os_view &v, const os_ptrs<R> &q, uint64_t c, int64_t s0,
                                                                  R (&out)[vec16<R>::lanes])
{
    using V = typename vec16<R>::type;
    constexpr int VEC = vec16<R>::lanes;
    const int64_t lo = c == v.cin_c ? v.cin_hi : 0;
    const uint64_t off = c * v.stride + static_cast<uint64_t>(s0);
    if (v.vec_ok && s0 >= lo && static_cast<uint64_t>(s0) + VEC <= v.samples && off % VEC == 0) {
        const V x = *reinterpret_cast<const V *>(q.data + off);
#pragma unroll
        for (int j = 0; j < VEC; j++)
            out[j] = x[j];
    } else {
#pragma unroll
        for (int j = 0; j < VEC; j++)
            out[j] = load_input(v, q, c, s0 + j);
    }
}

template <typename R> __global__ __launch_bounds__(kThreads) void sdsp_fir_os_frame(os_view v, os_ptrs<R> q)
{
    using V = typename vec16<R>::type;
    constexpr int VEC = vec16<R>::lanes;
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t u = gid >> v.lc;
    if (u >= v.units)
        return;
    const uint32_t k = static_cast<uint32_t>(gid & ((1ull << v.lc) - 1)), tpu = 1u << v.lc;
    const uint64_t g = v.g0 + u, c = g / v.pairs, p = g - c * v.pairs;
    const uint32_t i0 = k * VEC;

    // ---- the pair: frame 2p in the real part, frame 2p+1 (zeros past the channel's last frame) in the imaginary part
    const int64_t sa = static_cast<int64_t>(2 * p * v.hop) - static_cast<int64_t>(v.t1) + i0;
    R a[VEC], b[VEC];
    load_chunk<R>(v, q, c, sa, a);
    if (2 * p + 1 < v.frames) {
        load_chunk<R>(v, q, c, sa + v.hop, b);
    } else {
#pragma unroll
        for (int j = 0; j < VEC; j++)
            b[j] = R(0);
    }
    // VEC complex values = two 16-B vectors of (re, im) pairs; 16-B aligned since i0 is a multiple of VEC
    V *dst = reinterpret_cast<V *>(q.ws + 2 * (u * v.n + i0));
#pragma unroll
    for (int m = 0; m < 2; m++) {
        V w;
#pragma unroll
        for (int e = 0; e < VEC / 2; e++) {
            w[2 * e] = a[m * VEC / 2 + e];
            w[2 * e + 1] = b[m * VEC / 2 + e];
        }
        dst[m] = w;
    }

    // ---- the channel's new history: its last T-1 inputs, older history behind them when samples < T-1
    if (q.tails && p + 1 == v.pairs) {
        R *t = q.tails + (c - v.g0 / v.pairs) * v.t1;
        for (uint32_t j = k; j < v.t1; j += tpu)
            t[j] = load_input(v, q, c, static_cast<int64_t>(v.samples) - 1 - static_cast<int64_t>(j));
    }
    // ---- the next slice starts inside this channel: the T-1 inputs in front of its first frame, before this slice's scatter
    if (u + 1 == v.units && p + 1 < v.pairs) {
        const int64_t sb = static_cast<int64_t>(2 * (p + 1) * v.hop) - static_cast<int64_t>(v.t1);
        for (uint32_t j = k; j < v.t1; j += tpu)
            q.carry_out[j] = load_input(v, q, c, sb + j);
    }
}

template <typename R> __global__ __launch_bounds__(kThreads) void sdsp_fir_os_scatter(os_view v, os_ptrs<R> q)
{
    using V = typename vec16<R>::type;
    constexpr int VEC = vec16<R>::lanes;
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t u = gid >> v.lc;
    if (u >= v.units)
        return;
    const uint32_t o0 = static_cast<uint32_t>(gid & ((1ull << v.lc) - 1)) * VEC;
    if (o0 >= v.hop)
        return;
    const uint64_t g = v.g0 + u, c = g / v.pairs, p = g - c * v.pairs;
    const bool whole = o0 + VEC <= v.hop;

    // points T-1+o of the pair's circular convolution: real part -> frame 2p, imaginary part -> frame 2p+1
    const R *src = q.ws + 2 * (u * v.n + v.t1 + o0);
    R re[VEC], im[VEC];
    if (whole && (2 * (v.t1 + o0)) % VEC == 0) {
#pragma unroll
        for (int j = 0; j < 2 * VEC; j += VEC) {
            const V w = *reinterpret_cast<const V *>(src + j);
#pragma unroll
            for (int e = 0; e < VEC; e += 2) {
                re[(j + e) / 2] = w[e];
                im[(j + e) / 2] = w[e + 1];
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < VEC; j++) {
            const bool in = o0 + j < v.hop; // never past the unit's N points
            re[j] = in ? src[2 * j] : R(0);
            im[j] = in ? src[2 * j + 1] : R(0);
        }
    }
    auto put = [&](uint64_t s0, const R(&y)[VEC]) {
        if (s0 >= v.samples)
            return;
        const uint64_t off = c * v.stride + s0;
        if (v.vec_ok && whole && s0 + VEC <= v.samples && off % VEC == 0) {
            V w;
#pragma unroll
            for (int j = 0; j < VEC; j++)
                w[j] = y[j];
            *reinterpret_cast<V *>(q.data + off) = w;
        } else {
#pragma unroll
            for (int j = 0; j < VEC; j++)
                if (o0 + j < v.hop && s0 + j < v.samples)
                    q.data[off + j] = y[j];
        }
    };
    put(2 * p * v.hop + o0, re);
    put((2 * p + 1) * v.hop + o0, im);
}

// after the slice's frame launch: the staged tails of the channels [c_lo, c_lo + count) become their history
template <typename R> __global__ __launch_bounds__(kThreads) void sdsp_fir_os_state(R *state, const R *tails, uint64_t c_lo, uint64_t count,
                                                                                  uint32_t t1)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i < count * t1)
        state[c_lo * t1 + i] = tails[i];
}

template <typename R> int launch_os(const fir_os_args &a, int step, hipStream_t stream)
{
    constexpr int VEC = vec16<R>::lanes;
    const uint64_t g1 = a.g0 + a.units;
    if (step == FIR_OS_STATE) {
        const uint64_t c_lo = a.g0 / a.pairs, count = g1 / a.pairs - c_lo;
        const uint64_t n = count * a.taps_m1;
        if (n == 0)
            return SDSP_HIP_OK;
        hipLaunchKernelGGL(sdsp_fir_os_state<R>, dim3(static_cast<uint32_t>((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                           static_cast<R *>(a.state), static_cast<const R *>(a.tails), c_lo, count, a.taps_m1);
    } else {
        os_view v{};
        v.stride = a.stride;
        v.samples = a.samples;
        v.frames = a.frames;
        v.pairs = a.pairs;
        v.g0 = a.g0;
        v.units = a.units;
        v.n = a.n;
        v.hop = a.hop;
        v.t1 = a.taps_m1;
        v.lc = log2u(a.n / VEC);
        const uint64_t p0 = a.g0 % a.pairs;
        v.cin_c = (p0 && a.taps_m1) ? a.g0 / a.pairs : ~0ull;
        v.cin_hi = static_cast<int64_t>(2 * p0 * a.hop);
        v.cin_lo = v.cin_hi - static_cast<int64_t>(a.taps_m1);
        v.vec_ok = (reinterpret_cast<uintptr_t>(a.data) % 16 == 0 && (a.stride * sizeof(R)) % 16 == 0) ? 1 : 0;
        os_ptrs<R> q{ static_cast<R *>(a.data), static_cast<const R *>(a.state), static_cast<R *>(a.ws), static_cast<R *>(a.tails),
                      static_cast<const R *>(a.carry_in), static_cast<R *>(a.carry_out) };
        dim3 grid;
        if (int rc = grid_for(a.units << v.lc, "fir slice", &grid))
            return rc;
        if (step == FIR_OS_FRAME)
            hipLaunchKernelGGL(sdsp_fir_os_frame<R>, grid, dim3(kThreads), 0, stream, v, q);
        else
            hipLaunchKernelGGL(sdsp_fir_os_scatter<R>, grid, dim3(kThreads), 0, stream, v, q);
    }
    return launch_status("fir overlap-save");
}
} // namespace

int launch_fir_os(int precision, const fir_os_args &a, int step, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    return precision == SDSP_HIP_F64 ? launch_os<double>(a, step, s) : launch_os<float>(a, step, s);
}
} // namespace sdsp_hip
