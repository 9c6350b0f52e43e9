// pfb_synth.hip -- the unfold kernel of the polyphase synthesis filter banks (sdsp_hip_pfb_synth_*).
//
// One sdsp_hip_pfb_synth_process call runs as the pending-sum seed (stream_carry.hip: carry_seed), then slices of copy / pack -> reverse transform -> unfold launches over the
// plan's workspace.  The unit of work is one frame of M elements of one channel (an element is one real or one interleaved complex
// sample); units are numbered channel-major (g = c F + j) and a slice is a contiguous range of them, unfolded as rectangles of
// (channels, frames): a partial first channel, whole channels, a partial last channel.  Output position t of a channel lives in
// out[c out_stride + t] for t < S = F D and in state[c hist + t - S] above (the new pending sums): the inverse STFT bank's place rule.
//
//   sdsp_pfb_synth_copy    COMPLEX: the slice's spectra into the workspace rows, 16 bytes per lane where the input rows allow
//   (the plan's reverse transform, 1 / M scaled, in place on the slice: unchanged kernels; v_j = row j afterwards)
//   sdsp_pfb_synth_unfold  one owner per output position, no atomics.  The rectangle's frames of channel c are js .. je - 1 and cover
//                   t in [js D, (je - 1) D + L).  The owner of t starts from the sum at t's place when one exists (t < js D + hist, and
//                   js > 0 or a state was given -- known without reading memory), else from 0, adds fl(g[t - j D] v_j[i]) for the covering
//                   frames in ascending j (this file is compiled with -ffp-contract=off) and stores the sum back to t's place (dropped past
//                   S without a state).  i = (t - j D) mod M (FRAME) or (t + shift0) mod M (TIME: the rotation by s_j = (shift0 + j D) mod M
//                   cancels the frame's offset, so the row index does not depend on j).  A thread owns 16 bytes of positions (EPT
//                   elements) where D is a multiple of EPT and the pointers allow, one element otherwise; rows are read 16 bytes wide
//                   where the rotation keeps the vector whole, element by element otherwise.
//                     sliding form (D = M, J = 8): output hop n of residue r is sum over p of g[p M + r] v_(n - p)[r]: a thread owns a
//                       residue vector and J consecutive output hops, walks the frames n0 - P + 1 .. n0 + J - 1 once, loads each
//                       frame's vector once and adds its product with tap p into the accumulator of hop j + p -- P + J - 1 loads for J
//                       outputs, every accumulator receiving its frames in ascending j.  The J taps in use sit in a register ring
//                       (tap p is loaded at step P - 1 - p and last used J - 1 steps later).
//                     plain form (every other D): the owner of t loops over its ceil(L / D) covering frames; consecutive workgroups
//                       are placed on one XCD (stream_dev.h: xcd_block), so the re-reads of the rows hit its L2.
//                   Both forms perform the same additions in the same order: the same bits.
#include "stream_dev.h"

namespace sdsp_hip
{
namespace
{
constexpr int kSlide = 8; // output hops per thread of the sliding form

// one unfold launch: channels [c0, c0 + nc) x frames [j0, j0 + nj)
struct ps_view {
    uint64_t out_stride, samples;
    uint64_t c0, nc;
    uint64_t g0, frames; // frame j of channel c is workspace row c frames + j - g0
    uint64_t len;        // positions of one channel in the launch: nj D + hist
    uint64_t threads;
    uint32_t j0, nj;
    uint32_t m, p, hop, hist, taps_n;
    uint32_t kc, lc;     // sliding: chunks of J output hops per channel, log2(threads per chunk)
    uint32_t rotate, shift0, has_state, place_vec_ok;
};

// N reals from / to an address aligned to N reals
template <typename R, int N> __device__ __forceinline__ void ld(R *x, const R *p)
{
    const typename vec_n<R, N>::type t = *reinterpret_cast<const typename vec_n<R, N>::type *>(p);
#pragma unroll
    for (int e = 0; e < N; e++)
        x[e] = t[e];
}
template <typename R, int N> __device__ __forceinline__ void st(R *p, const R *x)
{
    typename vec_n<R, N>::type t;
#pragma unroll
    for (int e = 0; e < N; e++)
        t[e] = x[e];
    *reinterpret_cast<typename vec_n<R, N>::type *>(p) = t;
}

// E elements of a workspace row from element index i (a multiple of E unless the TIME rotation says otherwise), wrapping at M
template <typename R, int CPX, int E> __device__ __forceinline__ void load_row(R *x, const R *row, uint32_t i, uint32_t m)
{
    if (i % E == 0) {
        ld<R, E * CPX>(x, row + static_cast<uint64_t>(i) * CPX);
    } else {
#pragma unroll
        for (int el = 0; el < E; el++)
            ld<R, CPX>(x + el * CPX, row + static_cast<uint64_t>((i + el) & (m - 1)) * CPX);
    }
}

// the taps of E elements from tap index t0, one tap per element; `wide`: t0 is a multiple of E
template <typename R, int CPX, int E> __device__ __forceinline__ void load_taps(R *w, const R *taps, uint64_t t0, bool wide)
{
    R t[E];
    if (wide) {
        ld<R, E>(t, taps + t0);
    } else {
#pragma unroll
        for (int el = 0; el < E; el++)
            t[el] = taps[t0 + el];
    }
#pragma unroll
    for (int e = 0; e < E * CPX; e++)
        w[e] = t[e / CPX];
}

// where position t of channel c lives (null: a tail without a state, dropped)
template <typename R, int CPX> __device__ __forceinline__ R *place_of(const ps_view &v, R *out, R *state, uint64_t c, uint64_t t)
{
    if (t >= v.samples)
        return state ? state + (c * v.hist + (t - v.samples)) * CPX : nullptr;
    return out + (c * v.out_stride + t) * CPX;
}

template <typename R, int CPX, int E> __device__ __forceinline__ void load_place(const ps_view &v, R *x, const R *place)
{
    if (E == 1 || v.place_vec_ok) {
        ld<R, E * CPX>(x, place);
    } else {
#pragma unroll
        for (int el = 0; el < E; el++)
            ld<R, CPX>(x + el * CPX, place + el * CPX);
    }
}
template <typename R, int CPX, int E> __device__ __forceinline__ void store_place(const ps_view &v, R *place, const R *x)
{
    if (E == 1 || v.place_vec_ok) {
        st<R, E * CPX>(place, x);
    } else {
#pragma unroll
        for (int el = 0; el < E; el++)
            st<R, CPX>(place + el * CPX, x + el * CPX);
    }
}

// T: 16 bytes, or one f32 complex bin where the input rows are not 16-B aligned; `row` = T per frame
template <typename T>
__global__ __launch_bounds__(kThreads) void sdsp_pfb_synth_copy(const T *__restrict__ in, T *__restrict__ ws, uint64_t in_stride,
                                                                uint64_t row, uint64_t frames, uint64_t g0, uint64_t total)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= total)
        return;
    const uint64_t u = udiv(i, row), k = i - u * row;
    const uint64_t g = g0 + u;
    const uint64_t c = udiv(g, frames), j = g - c * frames;
    ws[i] = in[c * in_stride + j * row + k];
}

template <typename R, int CPX, int E>
__global__ __launch_bounds__(kThreads) void sdsp_pfb_synth_unfold(ps_view v, const R *__restrict__ ws, const R *__restrict__ taps, R *out,
                                                                  R *state)
{
    constexpr int N = E * CPX;
    const uint64_t gid = static_cast<uint64_t>(xcd_block(blockIdx.x, gridDim.x)) * kThreads + threadIdx.x;
    if (gid >= v.threads)
        return;
    // lane -> (channel, first position t of its E)
    const uint64_t q = gid * E;
    const uint64_t k = udiv(q, v.len);
    const uint64_t c = v.c0 + k;
    const uint64_t t = static_cast<uint64_t>(v.j0) * v.hop + (q - k * v.len);
    const uint32_t js = v.j0, je = v.j0 + v.nj; // exclusive
    // covering frames j: j D <= t < j D + L
    const uint64_t hi = udiv(t, v.hop);
    const uint64_t lo = t < v.taps_n ? 0 : udiv(t - v.taps_n, v.hop) + 1;
    const uint32_t jlo = static_cast<uint32_t>(lo > js ? lo : js);
    const uint32_t jhi = static_cast<uint32_t>(hi < je - 1 ? hi : je - 1);
    R *place = place_of<R, CPX>(v, out, state, c, t);
    R acc[N];
#pragma unroll
    for (int e = 0; e < N; e++)
        acc[e] = R(0);
    // a sum already sits at t's place (a tail without a state has none: its partial sums were dropped, and so is this one)
    if (place && t < static_cast<uint64_t>(js) * v.hop + v.hist && (js > 0 || v.has_state))
        load_place<R, CPX, E>(v, acc, place);
    const uint64_t base = c * v.frames - v.g0; // row of frame j = base + j
    const uint32_t it = static_cast<uint32_t>((t + v.shift0) & (v.m - 1));
    for (uint32_t j = jlo; j <= jhi; j++) {
        const uint32_t off = static_cast<uint32_t>(t - static_cast<uint64_t>(j) * v.hop);
        R x[N], w[N];
        load_row<R, CPX, E>(x, ws + (base + j) * v.m * CPX, v.rotate ? it : (off & (v.m - 1)), v.m);
        load_taps<R, CPX, E>(w, taps, off, true); // E > 1 only where D is a multiple of E: so is off
#pragma unroll
        for (int e = 0; e < N; e++) {
            const R y = w[e] * x[e];
            acc[e] = acc[e] + y;
        }
    }
    if (place)
        store_place<R, CPX, E>(v, place, acc);
}

template <typename R, int CPX, int J>
__global__ __launch_bounds__(kThreads) void sdsp_pfb_synth_unfold_slide(ps_view v, const R *__restrict__ ws, const R *__restrict__ taps,
                                                                        R *out, R *state)
{
    constexpr int E = vec16<R>::lanes / CPX, N = E * CPX;
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (gid >= v.threads)
        return;
    const uint64_t u = gid >> v.lc;
    const uint32_t r0 = static_cast<uint32_t>(gid & ((1ull << v.lc) - 1)) * E; // the thread's first residue
    const uint64_t kq = udiv(u, v.kc);
    const uint32_t first = static_cast<uint32_t>(u - kq * v.kc) * J; // the thread's first output hop, counted from hop j0
    const uint64_t c = v.c0 + kq;
    const uint32_t nout = v.nj + v.p - 1; // output hops the rectangle's frames reach
    const uint32_t jeff = min(static_cast<uint32_t>(J), nout - first);
    const uint64_t n0 = static_cast<uint64_t>(v.j0) + first;
    const uint32_t steps = v.p + jeff - 1;
    const uint32_t ir = v.rotate ? ((r0 + v.shift0) & (v.m - 1)) : r0;
    const uint64_t base = c * v.frames - v.g0;
    R acc[J][N], ring[J][N];
#pragma unroll
    for (int i = 0; i < J; i++) {
#pragma unroll
        for (int e = 0; e < N; e++)
            acc[i][e] = R(0);
        if (static_cast<uint32_t>(i) < jeff) {
            const uint64_t t = (n0 + i) * v.m + r0;
            const R *place = place_of<R, CPX>(v, out, state, c, t);
            if (place && t < static_cast<uint64_t>(v.j0) * v.m + v.hist && (v.j0 > 0 || v.has_state))
                load_place<R, CPX, E>(v, acc[i], place);
        }
    }
    for (uint32_t mb = 0; mb < steps; mb += J) {
#pragma unroll
        for (int mm = 0; mm < J; mm++) {
            const uint32_t mi = mb + mm;
            // step mi visits frame j = n0 + mi - (P - 1); frames outside the rectangle contribute nothing and are not read
            const uint64_t jp = n0 + mi; // j + P - 1
            const bool valid = mi < steps && jp >= static_cast<uint64_t>(v.j0) + (v.p - 1) && jp < static_cast<uint64_t>(v.j0) + v.nj + (v.p - 1);
            R x[N];
#pragma unroll
            for (int e = 0; e < N; e++)
                x[e] = R(0);
            if (valid)
                load_row<R, CPX, E>(x, ws + (base + (jp - (v.p - 1))) * v.m * CPX, ir, v.m);
            load_taps<R, CPX, E>(ring[mm], taps, static_cast<uint64_t>(v.p - 1 - min(mi, v.p - 1)) * v.m + r0, true);
#pragma unroll
            for (int i = 0; i < J; i++) {
                if (valid && mi >= static_cast<uint32_t>(i) && mi - i < v.p) { // tap p = P - 1 - (mi - i) of output hop i
#pragma unroll
                    for (int e = 0; e < N; e++) {
                        const R y = ring[(mm - i + J) % J][e] * x[e];
                        acc[i][e] = acc[i][e] + y;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < J; i++) {
        if (static_cast<uint32_t>(i) < jeff) {
            R *place = place_of<R, CPX>(v, out, state, c, (n0 + i) * v.m + r0);
            if (place)
                store_place<R, CPX, E>(v, place, acc[i]);
        }
    }
}

bool sliding(uint32_t m, uint32_t hop, int form) { return form == 0 && hop == m; }

template <typename T> int launch_copy(const pfb_synth_args &a, uint64_t bin_bytes, hipStream_t stream)
{
    const uint64_t per = sizeof(T) / bin_bytes; // bins per T
    const uint64_t row = a.m / per, total = a.units * row;
    dim3 grid;
    if (int rc = grid_for(total, "pfb synthesis slice", &grid))
        return rc;
    if (total)
        hipLaunchKernelGGL(sdsp_pfb_synth_copy<T>, grid, dim3(kThreads), 0, stream, static_cast<const T *>(a.in), static_cast<T *>(a.ws),
                           a.in_stride / per, row, static_cast<uint64_t>(a.frames), a.g0, total);
    return SDSP_HIP_OK;
}

template <typename R, int CPX> int launch_unfold(const pfb_synth_args &a, hipStream_t stream)
{
    constexpr int EPT = vec16<R>::lanes / CPX;
    if (a.nc == 0 || a.nj == 0)
        return SDSP_HIP_OK;
    const uint64_t es = sizeof(R) * CPX;
    ps_view v{};
    v.out_stride = a.out_stride;
    v.samples = static_cast<uint64_t>(a.frames) * a.hop;
    v.c0 = a.c0;
    v.nc = a.nc;
    v.g0 = a.g0;
    v.frames = a.frames;
    v.j0 = a.j0;
    v.nj = a.nj;
    v.m = a.m;
    v.p = a.p;
    v.hop = a.hop;
    v.hist = a.hist;
    v.taps_n = a.m * a.p;
    v.len = static_cast<uint64_t>(a.nj) * a.hop + a.hist;
    v.rotate = a.rotate ? 1 : 0;
    v.shift0 = a.rotate ? a.shift0 : 0;
    v.has_state = a.state ? 1 : 0;
    // 16-B accesses of out and state at element offsets that are multiples of EPT (hist is one where hop is)
    v.place_vec_ok = (reinterpret_cast<uintptr_t>(a.out) % 16 == 0 && (a.out_stride * es) % 16 == 0 &&
                      reinterpret_cast<uintptr_t>(a.state) % 16 == 0) ? 1 : 0;
    const R *ws = static_cast<const R *>(a.ws), *g = static_cast<const R *>(a.taps);
    R *out = static_cast<R *>(a.out), *state = static_cast<R *>(a.state);
    const bool slide = sliding(a.m, a.hop, a.form);
    const bool wide = !slide && EPT > 1 && a.hop % EPT == 0 && v.place_vec_ok;
    if (slide) {
        const uint32_t nout = a.nj + a.p - 1;
        v.kc = (nout + kSlide - 1) / kSlide;
        v.lc = log2u(a.m / EPT);
        v.threads = (a.nc * v.kc) << v.lc;
        if (v.threads >> v.lc != a.nc * v.kc)
            return fail(SDSP_HIP_ERR_UNSUPPORTED, "pfb synthesis slice too large for one launch");
    } else {
        if (a.nc > ~0ull / v.len)
            return fail(SDSP_HIP_ERR_UNSUPPORTED, "pfb synthesis slice too large for one launch");
        v.threads = a.nc * v.len / (wide ? EPT : 1);
    }
    dim3 grid;
    if (int rc = grid_for(v.threads, "pfb synthesis slice", &grid))
        return rc;
    if (slide)
        hipLaunchKernelGGL((sdsp_pfb_synth_unfold_slide<R, CPX, kSlide>), grid, dim3(kThreads), 0, stream, v, ws, g, out, state);
    else if (wide)
        hipLaunchKernelGGL((sdsp_pfb_synth_unfold<R, CPX, EPT>), grid, dim3(kThreads), 0, stream, v, ws, g, out, state);
    else
        hipLaunchKernelGGL((sdsp_pfb_synth_unfold<R, CPX, 1>), grid, dim3(kThreads), 0, stream, v, ws, g, out, state);
    return SDSP_HIP_OK;
}

template <typename R> int launch(const pfb_synth_args &a, int step, hipStream_t stream)
{
    typedef typename cplx_pair<R>::type C2;
    typedef typename vec16<R>::type V16;
    int rc;
    if (step == PFB_SYNTH_COPY) {
        const bool wide = reinterpret_cast<uintptr_t>(a.in) % 16 == 0 && (a.in_stride * sizeof(C2)) % 16 == 0;
        rc = wide ? launch_copy<V16>(a, sizeof(C2), stream) : launch_copy<C2>(a, sizeof(C2), stream);
    } else {
        rc = a.complex_out ? launch_unfold<R, 2>(a, stream) : launch_unfold<R, 1>(a, stream);
    }
    if (rc)
        return rc;
    return launch_status("pfb synthesis");
}
} // namespace

int launch_pfb_synth(int precision, const pfb_synth_args &a, int step, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    return precision == SDSP_HIP_F64 ? launch<double>(a, step, s) : launch<float>(a, step, s);
}

const char *pfb_synth_form_for(uint32_t m, uint32_t hop) { return sliding(m, hop, 0) ? "sliding" : "plain"; }
} // namespace sdsp_hip
