// pfb.hip -- the fold kernel of the polyphase filter-bank channelizer banks (sdsp_hip_pfb_*).
//
// One sdsp_hip_pfb_process call runs as slices of fold -> transform (-> emit, real input) launches, then one state launch.  The unit
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
//                       one XCD (the STFT bank's placement), so the re-reads of overlapping frames hit its L2.
//                   Loads and stores are 16 bytes wide where the element offset allows (history, odd strides and rotations that split a
//                   vector go element by element).
//   sdsp_pfb_state_flat / _shift   the STFT bank's state kernels for complex elements (real banks launch stft.hip's own).
#include "sdsp_hip_internal.h"

#include <hip/hip_runtime.h>

namespace sdsp_hip
{
namespace
{
constexpr int kThreads = 256;
constexpr int kSlide = 8; // frames per thread of the sliding form

template <typename R> struct pf_vec;
template <> struct pf_vec<float> {
    typedef float type __attribute__((ext_vector_type(4)));
    static constexpr int lanes = 4;
};
template <> struct pf_vec<double> {
    typedef double type __attribute__((ext_vector_type(2)));
    static constexpr int lanes = 2;
};

template <typename R> struct pf_cplx;
template <> struct pf_cplx<float> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct pf_cplx<double> { typedef double type __attribute__((ext_vector_type(2))); };

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

// workgroup b -> the position it works on: the blocks that share an XCD (b mod 8) get one contiguous range (the STFT bank's
// placement).  A bijection on [0, nb) for every nb.
__device__ __forceinline__ uint32_t xcd_block(uint32_t b, uint32_t nb)
{
    const uint32_t q = nb / 8, r = nb % 8, x = b % 8;
    return x * q + min(x, r) + b / 8;
}

// VEC reals = VEC / CPX elements of channel c from element position q0 of x
template <typename R, int CPX>
__device__ __forceinline__ typename pf_vec<R>::type load_x(const pf_view &v, const R *in, const R *state, uint64_t c, uint64_t q0)
{
    using V = typename pf_vec<R>::type;
    constexpr int VEC = pf_vec<R>::lanes, EPT = VEC / CPX;
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
template <typename R, int CPX> __device__ __forceinline__ typename pf_vec<R>::type load_taps(const R *taps, uint64_t t0)
{
    using V = typename pf_vec<R>::type;
    constexpr int VEC = pf_vec<R>::lanes;
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
    using V = typename pf_vec<R>::type;
    using C2 = typename pf_cplx<R>::type;
    constexpr int VEC = pf_vec<R>::lanes, EPT = VEC / CPX;
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

// S >= hist: the new history is the block's last hist elements, newest first
template <typename E>
__global__ __launch_bounds__(kThreads) void sdsp_pfb_state_flat(const E *__restrict__ in, E *__restrict__ state, uint64_t in_stride,
                                                                uint64_t samples, uint64_t channels, uint32_t hist)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= channels * hist)
        return;
    const uint64_t c = i / hist, jj = i - c * hist;
    state[i] = in[c * in_stride + (samples - 1 - jj)];
}

// S < hist: one workgroup per row, chunks from the high end down with a barrier between each chunk's reads and its writes
template <typename E>
__global__ __launch_bounds__(kThreads) void sdsp_pfb_state_shift(const E *__restrict__ in, E *state, uint64_t in_stride, uint32_t samples,
                                                                 uint32_t hist)
{
    const uint64_t c = blockIdx.x;
    E *row = state + c * hist;
    const uint32_t chunks = (hist + kThreads - 1) / kThreads;
    for (uint32_t q = chunks; q-- > 0;) {
        const uint32_t jj = q * kThreads + threadIdx.x;
        E val = E(0);
        if (jj < hist)
            val = jj < samples ? in[c * in_stride + (samples - 1 - jj)] : row[jj - samples];
        __syncthreads();
        if (jj < hist)
            row[jj] = val;
        __syncthreads();
    }
}

uint32_t log2u(uint64_t v)
{
    uint32_t l = 0;
    while ((1ull << l) < v)
        l++;
    return l;
}

bool sliding(uint32_t m, uint32_t hop, int form) { return form == 0 && m % hop == 0; }

template <typename R, int CPX> int launch_fold(const pfb_args &a, hipStream_t stream)
{
    constexpr int VEC = pf_vec<R>::lanes;
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
    const uint64_t threads = v.units << v.lc, blocks = (threads + kThreads - 1) / kThreads;
    if ((v.units << v.lc) >> v.lc != v.units || blocks > 0x7fffffffull)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "pfb slice too large for one launch");
    const dim3 grid(static_cast<uint32_t>(blocks));
    const R *in = static_cast<const R *>(a.in), *st = static_cast<const R *>(a.state), *h = static_cast<const R *>(a.taps);
    R *dst = static_cast<R *>(a.dst);
    if (slide)
        hipLaunchKernelGGL((sdsp_pfb_fold<R, CPX, kSlide>), grid, dim3(kThreads), 0, stream, v, in, st, h, dst);
    else
        hipLaunchKernelGGL((sdsp_pfb_fold<R, CPX, 1>), grid, dim3(kThreads), 0, stream, v, in, st, h, dst);
    return SDSP_HIP_OK;
}

template <typename R> int launch_state(const pfb_args &a, hipStream_t stream)
{
    using E = typename pf_cplx<R>::type;
    if (a.hist == 0 || !a.state_out || a.channels == 0)
        return SDSP_HIP_OK;
    const E *in = static_cast<const E *>(a.in);
    E *state = static_cast<E *>(a.state_out);
    if (a.samples >= a.hist) {
        const uint64_t n = a.channels * a.hist, blocks = (n + kThreads - 1) / kThreads;
        if (blocks > 0x7fffffffull)
            return fail(SDSP_HIP_ERR_UNSUPPORTED, "pfb state too large for one launch");
        hipLaunchKernelGGL(sdsp_pfb_state_flat<E>, dim3(static_cast<uint32_t>(blocks)), dim3(kThreads), 0, stream, in, state, a.in_stride,
                           a.samples, a.channels, a.hist);
    } else {
        if (a.channels > 0x7fffffffull)
            return fail(SDSP_HIP_ERR_UNSUPPORTED, "pfb state too large for one launch");
        hipLaunchKernelGGL(sdsp_pfb_state_shift<E>, dim3(static_cast<uint32_t>(a.channels)), dim3(kThreads), 0, stream, in, state,
                           a.in_stride, static_cast<uint32_t>(a.samples), a.hist);
    }
    return SDSP_HIP_OK;
}

template <typename R> int launch(const pfb_args &a, int step, hipStream_t stream)
{
    int rc;
    if (step == PFB_STATE)
        rc = launch_state<R>(a, stream);
    else
        rc = a.complex_in ? launch_fold<R, 2>(a, stream) : launch_fold<R, 1>(a, stream);
    if (rc)
        return rc;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(SDSP_HIP_ERR_HIP, std::string("pfb launch: ") + hipGetErrorString(e));
    return SDSP_HIP_OK;
}
} // namespace

int launch_pfb(int precision, const pfb_args &a, int step, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    return precision == SDSP_HIP_F64 ? launch<double>(a, step, s) : launch<float>(a, step, s);
}

const char *pfb_form_for(uint32_t m, uint32_t hop) { return sliding(m, hop, 0) ? "sliding" : "plain"; }
} // namespace sdsp_hip
