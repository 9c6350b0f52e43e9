// istft.hip -- the streaming layer of the inverse STFT bank (sdsp_hip_istft_*).
//
// One sdsp_hip_istft_process call runs as the pending-sum seed (stream_carry.hip: carry_seed), then slices of pack -> transform -> overlap-add launches over the plan's
// workspace.  The unit of work is one frame of N / 2 + 1 bins of one channel; units are numbered channel-major (g = c F + j, F frames
// per channel) and a slice is a contiguous range of them, so a slice may start or end inside a channel.  Output position t of a
// channel lives in out[c out_stride + t] for t < S = F hop and in state[c hist + t - S] above (the new pending sums).
//
//   sdsp_istft_pack  bins -> the packed half spectrum the reverse real-input transform reads: Z[0] = (Re X[0], Re X[N/2]), Z[k] = X[k];
//                    16-B stores (two f32 bins or one f64 bin per lane)
//   (the plan's reverse real-input transform of n_real = N, radix 2, 1 / N scaled, in place on the slice: unchanged kernels)
//   sdsp_istft_ola   one owner per output position, no atomics: the slice's frames of channel c are js .. je - 1 and cover
//                    t in [js hop, (je - 1) hop + N).  The owner of t starts from the sum at t's place when one exists (t < js hop + hist,
//                    and js > 0 or a state was given -- known without reading memory), else from 0, adds fl(g[t - j hop] z_j[t - j hop])
//                    for the covering frames in ascending j (no contraction: this file is compiled with -ffp-contract=off) and stores
//                    the sum back to t's place (dropped past S without a state).  Every addition of the contract happens in
//                    ascending j across slices too, so any slicing and any split into calls gives the same bits.  VEC consecutive
//                    positions per lane when hop is a multiple of VEC: frame edges then fall on vector boundaries.
#include "stream_dev.h"

namespace sdsp_hip
{
namespace
{
// one slice's view of the call; the slice's first unit is frame j0 of channel c0, its last frame j1 of channel c1
struct is_view {
    uint64_t in_stride, out_stride;
    uint64_t c0, c1;
    uint64_t g0;        // first unit of the slice
    uint64_t samples;   // S = F hop
    uint64_t len0;      // positions of channel c0 in the slice: (je0 - j0) hop + hist
    uint64_t len_full;  // positions of a channel whose every frame is in the slice: S + hist
    uint64_t positions; // positions of the slice (all channels), in lanes of VEC
    uint32_t j0, j1, frames;
    uint32_t units;
    uint32_t n, hop, hist;
    uint32_t lc;        // pack: log2(threads per unit)
    uint32_t has_state;
};

template <typename R>
__global__ __launch_bounds__(kThreads) void sdsp_istft_pack(is_view v, const R *__restrict__ in, R *__restrict__ ws)
{
    using C2 = typename cplx_pair<R>::type;
    constexpr int PB = vec16<R>::lanes / 2; // packed bins per lane (16 B)
    using V = typename vec_n<R, 2 * PB>::type;
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t u = gid >> v.lc;
    if (u >= v.units)
        return;
    const uint32_t k0 = static_cast<uint32_t>(gid & ((1ull << v.lc) - 1)) * PB;
    const uint64_t g = v.g0 + u;
    const uint64_t c = udiv(g, v.frames);
    const uint64_t j = g - c * v.frames;
    const C2 *x = reinterpret_cast<const C2 *>(in) + c * v.in_stride + j * (v.n / 2 + 1);
    V z;
#pragma unroll
    for (int e = 0; e < PB; e++) {
        const C2 b = x[k0 + e];
        z[2 * e] = b[0];
        z[2 * e + 1] = b[1];
    }
    if (k0 == 0)
        z[1] = x[v.n / 2][0];
    *reinterpret_cast<V *>(ws + u * v.n + 2 * k0) = z;
}

template <typename R, int VEC>
__global__ __launch_bounds__(kThreads) void sdsp_istft_ola(is_view v, const R *__restrict__ ws, const R *__restrict__ g, R *out, R *state)
{
    using V = typename vec_n<R, VEC>::type;
    const uint64_t p = (static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x);
    if (p >= v.positions)
        return;
    // lane -> (channel, first position t of its VEC)
    uint64_t c, t;
    const uint64_t q = p * VEC;
    if (q < v.len0) {
        c = v.c0;
        t = static_cast<uint64_t>(v.j0) * v.hop + q;
    } else {
        const uint64_t r = q - v.len0;
        const uint64_t k = udiv(r, v.len_full);
        c = v.c0 + 1 + k;
        t = r - k * v.len_full;
    }
    const uint32_t js = c == v.c0 ? v.j0 : 0;
    const uint32_t je = c == v.c1 ? v.j1 + 1 : v.frames; // exclusive
    // covering frames j: j hop <= t < j hop + N
    const uint64_t hi = udiv(t, v.hop);
    const uint64_t lo = t < v.n ? 0 : udiv(t - v.n, v.hop) + 1;
    const uint32_t jlo = static_cast<uint32_t>(lo > js ? lo : js);
    const uint32_t jhi = static_cast<uint32_t>(hi < je - 1 ? hi : je - 1);
    const bool tail = t >= v.samples;
    R *place = tail ? (state ? state + c * v.hist + (t - v.samples) : nullptr) : out + c * v.out_stride + t;
    // a sum already sits at t's place (a tail without a state has none: its partial sums were dropped, and so is this one)
    V acc = V(R(0));
    if (place && t < static_cast<uint64_t>(js) * v.hop + v.hist && (js > 0 || v.has_state))
        acc = *reinterpret_cast<const V *>(place);
    const uint64_t base = c * v.frames - v.g0; // unit of frame j = base + j
    for (uint32_t j = jlo; j <= jhi; j++) {
        const uint32_t off = static_cast<uint32_t>(t - static_cast<uint64_t>(j) * v.hop);
        const V z = *reinterpret_cast<const V *>(ws + (base + j) * v.n + off);
        const V w = *reinterpret_cast<const V *>(g + off);
        const V y = w * z;
        acc = acc + y;
    }
    if (place)
        *reinterpret_cast<V *>(place) = acc;
}

template <typename R> int launch(const istft_args &a, int step, hipStream_t stream)
{
    R *out = static_cast<R *>(a.out);
    R *state = static_cast<R *>(a.state);
    const uint64_t samples = static_cast<uint64_t>(a.frames) * a.hop;
    is_view v{};
    v.in_stride = a.in_stride;
    v.out_stride = a.out_stride;
    v.g0 = a.g0;
    v.c0 = a.g0 / a.frames;
    v.j0 = static_cast<uint32_t>(a.g0 - v.c0 * a.frames);
    const uint64_t g1 = a.g0 + a.units - 1;
    v.c1 = g1 / a.frames;
    v.j1 = static_cast<uint32_t>(g1 - v.c1 * a.frames);
    v.frames = a.frames;
    v.units = a.units;
    v.n = a.n;
    v.hop = a.hop;
    v.hist = a.hist;
    v.samples = samples;
    v.has_state = state ? 1 : 0;
    const R *ws = static_cast<const R *>(a.ws);
    dim3 grid;
    if (step == ISTFT_PACK) {
        v.lc = log2u(a.n / vec16<R>::lanes); // N / 2 packed bins, 16 B of them per lane
        if (int rc = grid_for(static_cast<uint64_t>(a.units) << v.lc, "istft slice", &grid))
            return rc;
        hipLaunchKernelGGL(sdsp_istft_pack<R>, grid, dim3(kThreads), 0, stream, v, static_cast<const R *>(a.in), static_cast<R *>(a.ws));
    } else {
        const uint32_t je0 = v.c0 == v.c1 ? v.j1 + 1 : a.frames;
        v.len0 = static_cast<uint64_t>(je0 - v.j0) * a.hop + a.hist;
        v.len_full = samples + a.hist;
        const uint64_t len1 = v.c0 == v.c1 ? 0 : static_cast<uint64_t>(v.j1 + 1) * a.hop + a.hist;
        const uint64_t middle = v.c1 > v.c0 + 1 ? (v.c1 - v.c0 - 1) * v.len_full : 0;
        const uint64_t total = v.len0 + middle + len1;
        constexpr int VEC = vec16<R>::lanes;
        // VEC positions per lane: frame edges (multiples of hop, + N) and the out / state split (S) on vector boundaries, and every
        // vector address 16-B aligned
        const bool vec = a.hop % VEC == 0 && reinterpret_cast<uintptr_t>(a.out) % 16 == 0 && a.out_stride % VEC == 0 &&
                         reinterpret_cast<uintptr_t>(a.state) % 16 == 0;
        v.positions = vec ? total / VEC : total;
        if (int rc = grid_for(v.positions, "istft slice", &grid))
            return rc;
        if (vec)
            hipLaunchKernelGGL((sdsp_istft_ola<R, VEC>), grid, dim3(kThreads), 0, stream, v, ws, static_cast<const R *>(a.g), out, state);
        else
            hipLaunchKernelGGL((sdsp_istft_ola<R, 1>), grid, dim3(kThreads), 0, stream, v, ws, static_cast<const R *>(a.g), out, state);
    }
    return launch_status("istft");
}
} // namespace

int launch_istft(int precision, const istft_args &a, int step, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    return precision == SDSP_HIP_F64 ? launch<double>(a, step, s) : launch<float>(a, step, s);
}
} // namespace sdsp_hip
