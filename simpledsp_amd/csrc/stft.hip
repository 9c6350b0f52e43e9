// stft.hip -- the streaming layer of the STFT bank (sdsp_hip_stft_*).
//
// One sdsp_hip_stft_process call runs as slices of frame -> transform -> emit launches over the plan's workspace, then the history
// update (stream_carry.hip: carry_history).  The unit of work is one frame of N reals of one channel; units are numbered channel-major (g = c F + j, F frames per
// channel) and a slice is a contiguous range of them, so a slice may start or end inside a channel.
//
//   sdsp_stft_frame  x[j hop + i] * w[i] for the slice's frames into the workspace (N reals per unit, 16 B per lane); x is the
//                    channel's history followed by the block: x[p] = state[c hist + hist - 1 - p] for p < hist, else
//                    in[c in_stride + p - hist].  Overlapping frames read the same input: consecutive workgroups of a slice are
//                    placed on one XCD (stream_dev.h: xcd_block), so those re-reads hit its L2.
//   (the plan's forward real-input transform of n_real = N, radix 2, in place on the slice: unchanged kernels)
//   sdsp_stft_emit   the packed half spectrum (Z[0] = (X[0], X[N/2]), Z[k] = X[k]) -> N/2 + 1 output bins per frame: complex,
//                    re re + im im (no contraction: this file is compiled with -ffp-contract=off) or its square root
#include "stream_dev.h"

namespace sdsp_hip
{
namespace
{
// one slice's view of the call; the slice's first unit is frame j0 of channel c0
struct st_view {
    uint64_t in_stride, out_stride;
    uint64_t c0;
    uint32_t j0, frames; // frames per channel (F)
    uint32_t units;      // units in the slice
    uint32_t n, hop, hist, bins;
    uint32_t lc;         // log2(threads per unit)
    uint32_t vec_ok;     // `in` and in_stride keep 16-B alignment of element offsets that are multiples of the vector width
};

// unit u of the slice -> (channel, frame)
__device__ __forceinline__ void unit_pos(const st_view &v, uint32_t u, uint64_t &c, uint32_t &j)
{
    const uint32_t t = v.j0 + u; // < F + units < 2^32 (checked by the launcher)
    const uint32_t dc = t / v.frames;
    c = v.c0 + dc;
    j = t - dc * v.frames;
}

template <typename R>
__device__ __forceinline__ R load_x(const st_view &v, const R *in, const R *state, uint64_t c, uint64_t p)
{
    if (p < v.hist)
        return state ? state[c * v.hist + (v.hist - 1 - p)] : R(0);
    return in[c * v.in_stride + (p - v.hist)];
}

template <typename R>
__global__ __launch_bounds__(kThreads) void sdsp_stft_frame(st_view v, const R *__restrict__ in, const R *__restrict__ state,
                                                            const R *__restrict__ window, R *__restrict__ ws)
{
    using V = typename vec16<R>::type;
    constexpr int VEC = vec16<R>::lanes;
    const uint64_t gid = static_cast<uint64_t>(xcd_block(blockIdx.x, gridDim.x)) * kThreads + threadIdx.x;
    const uint64_t u = gid >> v.lc;
    if (u >= v.units)
        return;
    const uint32_t i0 = static_cast<uint32_t>(gid & ((1ull << v.lc) - 1)) * VEC;
    uint64_t c;
    uint32_t j;
    unit_pos(v, static_cast<uint32_t>(u), c, j);
    const uint64_t p0 = static_cast<uint64_t>(j) * v.hop + i0;
    const V w = *reinterpret_cast<const V *>(window + i0);
    V x;
    const uint64_t off = c * v.in_stride + (p0 - v.hist);
    if (v.vec_ok && p0 >= v.hist && off % VEC == 0) {
        x = *reinterpret_cast<const V *>(in + off);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; e++)
            x[e] = load_x(v, in, state, c, p0 + e);
    }
    V y;
#pragma unroll
    for (int e = 0; e < VEC; e++)
        y[e] = x[e] * w[e];
    *reinterpret_cast<V *>(ws + u * v.n + i0) = y;
}

template <typename R, int KIND>
__global__ __launch_bounds__(kThreads) void sdsp_stft_emit(st_view v, const R *__restrict__ ws, R *__restrict__ out)
{
    using C2 = typename cplx_pair<R>::type;
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t u = gid >> v.lc;
    if (u >= v.units)
        return;
    const uint32_t k = static_cast<uint32_t>(gid & ((1ull << v.lc) - 1)); // 0 .. N/2 - 1: one packed bin per thread
    uint64_t c;
    uint32_t j;
    unit_pos(v, static_cast<uint32_t>(u), c, j);
    const C2 z = reinterpret_cast<const C2 *>(ws + u * v.n)[k];
    const uint64_t row = c * v.out_stride + static_cast<uint64_t>(j) * v.bins; // in output elements
    auto put = [&](uint32_t bin, R re, R im) {
        if (KIND == SDSP_HIP_STFT_COMPLEX) {
            C2 o;
            o[0] = re;
            o[1] = im;
            reinterpret_cast<C2 *>(out)[row + bin] = o;
        } else {
            const R pw = re * re + im * im;
            out[row + bin] = KIND == SDSP_HIP_STFT_POWER ? pw : sqrt(pw);
        }
    };
    if (k == 0) {
        put(0, z[0], R(0));
        put(v.n / 2, z[1], R(0));
    } else {
        put(k, z[0], z[1]);
    }
}

template <typename R> int launch(const stft_args &a, int step, hipStream_t stream)
{
    constexpr int VEC = vec16<R>::lanes;
    if (static_cast<uint64_t>(a.frames) + a.units >= (1ull << 32))
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "stft slice: too many frames per channel");
    st_view v{};
    v.in_stride = a.in_stride;
    v.out_stride = a.out_stride;
    v.c0 = a.g0 / a.frames;
    v.j0 = static_cast<uint32_t>(a.g0 - v.c0 * a.frames);
    v.frames = a.frames;
    v.units = a.units;
    v.n = a.n;
    v.hop = a.hop;
    v.hist = a.hist;
    v.bins = a.n / 2 + 1;
    v.vec_ok = (reinterpret_cast<uintptr_t>(a.in) % 16 == 0 && (a.in_stride * sizeof(R)) % 16 == 0) ? 1 : 0;
    v.lc = log2u(step == STFT_FRAME ? a.n / VEC : a.n / 2);
    dim3 grid;
    if (int rc = grid_for(static_cast<uint64_t>(a.units) << v.lc, "stft slice", &grid))
        return rc;
    R *ws = static_cast<R *>(a.ws);
    if (step == STFT_FRAME) {
        hipLaunchKernelGGL(sdsp_stft_frame<R>, grid, dim3(kThreads), 0, stream, v, static_cast<const R *>(a.in),
                           static_cast<const R *>(a.state), static_cast<const R *>(a.window), ws);
    } else {
        R *out = static_cast<R *>(a.out);
        if (a.output == SDSP_HIP_STFT_COMPLEX)
            hipLaunchKernelGGL((sdsp_stft_emit<R, SDSP_HIP_STFT_COMPLEX>), grid, dim3(kThreads), 0, stream, v, ws, out);
        else if (a.output == SDSP_HIP_STFT_POWER)
            hipLaunchKernelGGL((sdsp_stft_emit<R, SDSP_HIP_STFT_POWER>), grid, dim3(kThreads), 0, stream, v, ws, out);
        else
            hipLaunchKernelGGL((sdsp_stft_emit<R, SDSP_HIP_STFT_MAGNITUDE>), grid, dim3(kThreads), 0, stream, v, ws, out);
    }
    return launch_status("stft");
}
} // namespace

int launch_stft(int precision, const stft_args &a, int step, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    return precision == SDSP_HIP_F64 ? launch<double>(a, step, s) : launch<float>(a, step, s);
}
} // namespace sdsp_hip
