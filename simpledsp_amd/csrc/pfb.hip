// pfb.hip -- the fold kernel of the polyphase filter-bank channelizer banks (sdsp_hip_pfb_*).
//
// One sdsp_hip_pfb_process call runs as slices of fold -> transform (-> emit, real input) launches, then the history update
// (stream_carry.hip: carry_history).  The unit
// of work is one frame of M elements of one channel (an element is one real or one interleaved complex sample).
//
//   sdsp_pfb_fold   u_j[r] = sum over p < P of fl(x[j D + p M + r] h[p M + r]) in ascending p, every product and sum rounded on its own
//                   (this file is compiled with -ffp-contract=off), written at element (r + s_j) mod M of the frame's row: s_j = 0
//                   (FRAME) or (shift0 + j D) mod M (TIME).  x is the channel's history followed by the block: x[q] = state[c hist +
//                   hist - 1 - q] for q < hist, else in[c in_stride + q - hist].  A thread owns 16 bytes of the row (VEC reals = VEC / CPX
//                   elements) and J frames:
//                     sliding form (D divides M, J = 8): with q = M / D the frames a, a + q, a + 2 q .. of a channel start M samples
//                       apart, so frame i of that chain needs x[(a D + r) + (i + p) M]: one thread walks m = i + p over J frames of one
//                       chain, loads each sample once and adds its product into every frame that covers it -- P + J - 1 loads for J
//                       outputs.  The J taps in use sit in a register ring (tap p is loaded at step m = p and last used at p + J - 1).
//                     plain form (every other D, J = 1): one frame per thread, P loads per output; consecutive workgroups are placed on
//                       one XCD (stream_dev.h: xcd_block), so the re-reads of overlapping frames hit its L2.
//                   Loads and stores are 16 bytes wide where the element offset allows (history, odd strides and rotations that split a
//                   vector go element by element).
#include "stream_dev.h"

namespace sdsp_hip
{
namespace
{
constexpr int kSlide = 8; // frames per thread of the sliding form

// one fold launch: channels [c0, ..) x frames [j0, j0 + nj), as units (channel, chain a < q, chunk k < kc) with k fastest
struct pf_view {
    uint64_t in_stride, dst_cstride, dst_sub;
    uint64_t c0, units;
    uint32_t j0, nj;
    uint32_t m, p, hop, hist;
    uint32_t q, kc, cs;  // chains per channel, chunks of J frames per chain, samples between a chain's frames (sliding M, plain D)
    uint32_t lc;         // log2(threads per unit)
    uint32_t in_vec_ok, dst_vec_ok; // pointer and strides keep 16-B alignment of offsets that are multiples of the vector width
    uint32_t rotate, shift0, xcd;
};

// VEC reals = VEC / CPX elements of channel c from element position q0 of x
template <typename R, int CPX>
__device__ __forceinline__ typename vec16<R>::type load_x(const pf_view &v, const R *in, const R *state, uint64_t c, uint64_t q0)
{
    using V = typename vec16<R>::type;
    constexpr int VEC = vec16<R>::lanes, EPT = VEC / CPX;
    V x;
    const uint64_t off = (c * v.in_stride + (q0 - v.hist)) * CPX; // in reals; only used where q0 >= hist
    if (v.in_vec_ok && q0 >= v.hist && off % VEC == 0) {
        x = *reinterpret_cast<const V *>(in + off);
    } else {
#pragma unroll
        for (int el = 0; el < EPT; el++) {
            const uint64_t q = q0 + el;
#pragma unroll
            for (int k = 0; k < CPX; k++) {
                if (q < v.hist)
                    x[el * CPX + k] = state ? state[(c * v.hist + (v.hist - 1 - q)) * CPX + k] : R(0);
                else
                    x[el * CPX + k] = in[(c * v.in_stride + (q - v.hist)) * CPX + k];
            }
        }
    }
    return x;
}

// the taps of VEC reals from tap index t0 (= p M + the thread's first element): one tap per element
template <typename R, int CPX> __device__ __forceinline__ typename vec16<R>::type load_taps(const R *taps, uint64_t t0)
{
    using V = typename vec16<R>::type;
    constexpr int VEC = vec16<R>::lanes;
    if (CPX == 1)
        return *reinterpret_cast<const V *>(taps + t0); // t0 is a multiple of VEC: M is, and so is the thread's first element
    V t;
#pragma unroll
    for (int e = 0; e < VEC; e++)
        t[e] = taps[t0 + e / CPX];
    return t;
}

template <typename R, int CPX, int J>
__global__ __launch_bounds__(kThreads) void sdsp_pfb_fold(pf_view v, const R *__restrict__ in, const R *__restrict__ state,
                                                          const R *__restrict__ taps, R *__restrict__ dst)
{
    using V = typename vec16<R>::type;
    using C2 = typename cplx_pair<R>::type;
    constexpr int VEC = vec16<R>::lanes, EPT = VEC / CPX;
    const uint32_t b = v.xcd ? xcd_block(blockIdx.x, gridDim.x) : blockIdx.x;
    const uint64_t gid = static_cast<uint64_t>(b) * kThreads + threadIdx.x;
    const uint64_t u = gid >> v.lc;
    if (u >= v.units)
        return;
    const uint32_t r0 = static_cast<uint32_t>(gid & ((1ull << v.lc) - 1)) * EPT; // the thread's first element of the frame
    const uint32_t k = static_cast<uint32_t>(u % v.kc);
    const uint64_t uc = u / v.kc;
    const uint32_t a = static_cast<uint32_t>(uc % v.q);
    const uint64_t c = v.c0 + uc / v.q;
    if (a >= v.nj)
        return;
    const uint32_t chain = (v.nj - a + v.q - 1) / v.q, first = k * J; // frames of chain a in this launch; the thread's first
    if (first >= chain)
        return;
    const uint32_t jeff = min(static_cast<uint32_t>(J), chain - first);
    const uint64_t xb = static_cast<uint64_t>(v.j0 + a) * v.hop + static_cast<uint64_t>(first) * v.cs + r0;
    const uint32_t steps = v.p + jeff - 1;
    V acc[J], ring[J];
#pragma unroll
    for (int i = 0; i < J; i++)
        acc[i] = V(0);
    for (uint32_t mb = 0; mb < steps; mb += J) {
#pragma unroll
        for (int mm = 0; mm < J; mm++) {
            const uint32_t mi = mb + mm;
            // past the last step the load repeats the last one: its products reach only frames past jeff, which are not stored
            const V x = load_x<R, CPX>(v, in, state, c, xb + static_cast<uint64_t>(min(mi, steps - 1)) * v.m);
            ring[mm] = load_taps<R, CPX>(taps, static_cast<uint64_t>(min(mi, v.p - 1)) * v.m + r0);
#pragma unroll
            for (int i = 0; i < J; i++) {
                if (mi >= static_cast<uint32_t>(i) && mi - i < v.p) { // tap p = mi - i of frame i (the same in every lane)
                    const V t = ring[(mm - i + J) % J];
                    const bool lead = mi == static_cast<uint32_t>(i);
#pragma unroll
                    for (int e = 0; e < VEC; e++) {
                        const R prod = x[e] * t[e];
                        acc[i][e] = lead ? prod : acc[i][e] + prod;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < J; i++) {
        if (static_cast<uint32_t>(i) < jeff) {
            const uint64_t j = static_cast<uint64_t>(v.j0) + a + static_cast<uint64_t>(first + i) * v.q;
            const uint32_t s = v.rotate ? static_cast<uint32_t>((v.shift0 + j * v.hop) & (v.m - 1)) : 0;
            const uint64_t row = c * v.dst_cstride + j * v.m - v.dst_sub; // in elements
            if (v.dst_vec_ok && s % EPT == 0) {
                *reinterpret_cast<V *>(dst + (row + ((r0 + s) & (v.m - 1))) * CPX) = acc[i];
            } else {
#pragma unroll
                for (int el = 0; el < EPT; el++) {
                    const uint64_t at = row + ((r0 + el + s) & (v.m - 1));
                    if (CPX == 2) {
                        C2 o;
                        o[0] = acc[i][el * CPX];
                        o[1] = acc[i][el * CPX + CPX - 1];
                        reinterpret_cast<C2 *>(dst)[at] = o;
                    } else {
                        dst[at] = acc[i][el];
                    }
                }
            }
        }
    }
}

bool sliding(uint32_t m, uint32_t hop, int form) { return form == 0 && m % hop == 0; }

template <typename R, int CPX> int launch_fold(const pfb_args &a, hipStream_t stream)
{
    constexpr int VEC = vec16<R>::lanes;
    if (a.nc == 0 || a.nj == 0)
        return SDSP_HIP_OK;
    const bool slide = sliding(a.m, a.hop, a.form);
    const uint32_t J = slide ? kSlide : 1;
    pf_view v{};
    v.in_stride = a.in_stride;
    v.dst_cstride = a.dst_cstride;
    v.dst_sub = a.dst_sub;
    v.c0 = a.c0;
    v.j0 = a.j0;
    v.nj = a.nj;
    v.m = a.m;
    v.p = a.p;
    v.hop = a.hop;
    v.hist = a.hist;
    v.q = slide ? a.m / a.hop : 1;
    v.cs = slide ? a.m : a.hop;
    const uint32_t chain = (a.nj + v.q - 1) / v.q;
    v.kc = (chain + J - 1) / J;
    v.units = a.nc * v.q * v.kc;
    v.lc = log2u(static_cast<uint64_t>(a.m) * CPX / VEC);
    v.in_vec_ok = (reinterpret_cast<uintptr_t>(a.in) % 16 == 0 && (a.in_stride * CPX * sizeof(R)) % 16 == 0) ? 1 : 0;
    v.dst_vec_ok = (reinterpret_cast<uintptr_t>(a.dst) % 16 == 0 && (a.dst_cstride * CPX * sizeof(R)) % 16 == 0 &&
                    (a.dst_sub * CPX * sizeof(R)) % 16 == 0) ? 1 : 0;
    v.rotate = a.rotate ? 1 : 0;
    v.shift0 = a.shift0;
    v.xcd = slide ? 0 : 1;
    if ((v.units << v.lc) >> v.lc != v.units)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "pfb slice too large for one launch");
    dim3 grid;
    if (int rc = grid_for(v.units << v.lc, "pfb slice", &grid))
        return rc;
    const R *in = static_cast<const R *>(a.in), *st = static_cast<const R *>(a.state), *h = static_cast<const R *>(a.taps);
    R *dst = static_cast<R *>(a.dst);
    if (slide)
        hipLaunchKernelGGL((sdsp_pfb_fold<R, CPX, kSlide>), grid, dim3(kThreads), 0, stream, v, in, st, h, dst);
    else
        hipLaunchKernelGGL((sdsp_pfb_fold<R, CPX, 1>), grid, dim3(kThreads), 0, stream, v, in, st, h, dst);
    return SDSP_HIP_OK;
}

template <typename R> int launch(const pfb_args &a, hipStream_t stream)
{
    if (int rc = a.complex_in ? launch_fold<R, 2>(a, stream) : launch_fold<R, 1>(a, stream))
        return rc;
    return launch_status("pfb");
}
} // namespace

int launch_pfb(int precision, const pfb_args &a, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    return precision == SDSP_HIP_F64 ? launch<double>(a, s) : launch<float>(a, s);
}

const char *pfb_form_for(uint32_t m, uint32_t hop) { return sliding(m, hop, 0) ? "sliding" : "plain"; }
} // namespace sdsp_hip
