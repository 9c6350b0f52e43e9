// ddc.hip -- digital down-converter banks for MI355X (gfx950): mix to baseband, filter with h[0..T), keep every D-th sample.
//
// Output m of band i of a call (x = the source channel's history, then the block; n = position + m D):
//     z = sum over k < T of g_i[k] x[n - k]      ascending k from +0; one fmaf per step in f32, a multiply then an add in f64
//     w = C[j >> 16] (x) F[j & 0xffff],          j = (phase0_i + fcw_i n) mod 2^32 in unsigned integers
//     y = z (x) w                                (a (x) b): two products and one sum or difference, each rounded on its own
// g_i (the taps turned by the band's frequency), C and F come rounded from the plan (capi.hip); built with -ffp-contract=off, so
// nothing here contracts.  DESIGN.md section 5.19.
//
// Two kernels:
//   sdsp_ddc_kernel        variant 0.  A workgroup owns one input channel and one block of outputs.  It stages the block's inputs and
//                          the T - 1 samples in front of them (from `state` or from the row) in LDS once -- 16-byte nontemporal
//                          loads, a padded line so that lanes reading at stride 2 D spread over the banks -- and then works through
//                          every band of that channel: a wave takes (up to four bands, 128 consecutive outputs) at a time, each lane
//                          two consecutive outputs, so one LDS read of x serves up to eight multiply-adds (sixteen for complex
//                          input), the band taps are wave-uniform scalar loads, and a lane's two results leave as one 16-byte store.
//                          The oscillator is one gather of C and F per output.  A channel without bands returns at once.
//   sdsp_ddc_plain_kernel  variant 1: one output per thread straight from global memory, the independent cross-check.
// The new history is carry_history's (stream_carry.hip), launched by the caller behind either kernel.
#include "stream_dev.h"

#include <type_traits>

namespace sdsp_hip
{
namespace
{
constexpr int kPerLane = 2;                   // consecutive outputs per lane
constexpr uint32_t kGroup = 64 * kPerLane;    // outputs of one wave task
constexpr uint32_t kBandChunk = 4;            // bands that share one LDS read
constexpr uint32_t kMaxBlockOut = 512;        // outputs per band and block: every lane of the workgroup busy with one band chunk
constexpr size_t kLdsTarget = 64 * 1024;      // LDS line target (two workgroups per CU); huge T + D alone may need more
// the largest line a plan can ask for: T = 4096 and D = 1024 on 16-byte elements (87 KiB).  Every instantiation of the fused kernel gets
// this one dynamic-LDS limit, set once per device when the first plan that runs it is created (ddc_prepare), never per launch
constexpr size_t kLdsLimit = 96 * 1024;

template <typename R> __device__ __forceinline__ R mul_add(R g, R x, R acc);
template <> __device__ __forceinline__ float mul_add<float>(float g, float x, float acc) { return __builtin_fmaf(g, x, acc); }
template <> __device__ __forceinline__ double mul_add<double>(double g, double x, double acc) { return acc + g * x; }
template <typename R> __device__ __forceinline__ R mul_sub(R g, R x, R acc);
template <> __device__ __forceinline__ float mul_sub<float>(float g, float x, float acc) { return __builtin_fmaf(-g, x, acc); }
template <> __device__ __forceinline__ double mul_sub<double>(double g, double x, double acc) { return acc - g * x; }

// one input element: a real, or an interleaved complex pair
template <typename R, bool CPLX> struct elem {
    typedef R type;
};
template <typename R> struct elem<R, true> {
    typedef typename cplx_pair<R>::type type;
};

// one tap of the filter sum, in the contract's order
__device__ __forceinline__ void tap(float gr, float gi, float x, float &zr, float &zi)
{
    zr = mul_add<float>(gr, x, zr);
    zi = mul_add<float>(gi, x, zi);
}
__device__ __forceinline__ void tap(double gr, double gi, double x, double &zr, double &zi)
{
    zr = mul_add<double>(gr, x, zr);
    zi = mul_add<double>(gi, x, zi);
}
template <typename R> __device__ __forceinline__ void tap_c(R gr, R gi, typename cplx_pair<R>::type x, R &zr, R &zi)
{
    zr = mul_add<R>(gr, x.x, zr);
    zr = mul_sub<R>(gi, x.y, zr);
    zi = mul_add<R>(gr, x.y, zi);
    zi = mul_add<R>(gi, x.x, zi);
}
__device__ __forceinline__ void tap(float gr, float gi, cplx_pair<float>::type x, float &zr, float &zi) { tap_c<float>(gr, gi, x, zr, zi); }
__device__ __forceinline__ void tap(double gr, double gi, cplx_pair<double>::type x, double &zr, double &zi)
{
    tap_c<double>(gr, gi, x, zr, zi);
}

// a (x) b: every product and the sum or difference rounded on its own
template <typename R> __device__ __forceinline__ typename cplx_pair<R>::type cmul(typename cplx_pair<R>::type a, typename cplx_pair<R>::type b)
{
    typename cplx_pair<R>::type r;
    r.x = a.x * b.x - a.y * b.y;
    r.y = a.x * b.y + a.y * b.x;
    return r;
}

struct ddc_kargs {
    const void *in;
    void *out;
    const void *state;
    const void *g, *coarse, *fine;
    const uint32_t *csr, *bands;
    uint64_t samples, in_stride, out_stride, position, outs;
    uint32_t taps, down, hist, nb;
    uint32_t blk_out;   // outputs per band and block
    uint32_t nblk;      // blocks per channel
    uint32_t pad_shift; // LDS line: element p lives at p + (p >> pad_shift)
    uint32_t vec_in, vec_out; // rows 16-byte aligned
};

__device__ __forceinline__ uint32_t slot(uint32_t p, uint32_t shift) { return p + (p >> shift); }

// y = z (x) w for output n of the stream (n mod 2^32 is all the phase needs)
template <typename R>
__device__ __forceinline__ typename cplx_pair<R>::type mix(const ddc_kargs &a, R zr, R zi, uint32_t fcw, uint32_t phase0, uint32_t n)
{
    using P = typename cplx_pair<R>::type;
    const uint32_t j = phase0 + fcw * n;
    const P c = static_cast<const P *>(a.coarse)[j >> 16];
    const P f = static_cast<const P *>(a.fine)[j & 0xffffu];
    P z;
    z.x = zr;
    z.y = zi;
    return cmul<R>(z, cmul<R>(c, f));
}

// NB bands [s0, s0 + NB) of the table for the lane's two outputs mo, mo + 1 of the block (no = the block's valid outputs)
template <typename R, bool CPLX, int NB>
__device__ __forceinline__ void band_chunk(const ddc_kargs &a, const typename elem<R, CPLX>::type *line, uint32_t s0, uint32_t mo, uint32_t no,
                                           uint64_t m0)
{
    using E = typename elem<R, CPLX>::type;
    using P = typename cplx_pair<R>::type;
    const uint32_t T = a.taps, D = a.down, sh = a.pad_shift;
    bool ok[kPerLane];
    uint32_t idx[kPerLane]; // line index of x[n] for tap 0; a lane past the block reads the block's last output's samples
#pragma unroll
    for (int r = 0; r < kPerLane; r++) {
        ok[r] = mo + r < no;
        idx[r] = a.hist + (ok[r] ? mo + r : no - 1) * D;
    }
    R zr[NB][kPerLane], zi[NB][kPerLane];
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
        for (int r = 0; r < kPerLane; r++)
            zr[b][r] = zi[b][r] = R(0);
    const R *g = static_cast<const R *>(a.g) + static_cast<size_t>(s0) * T * 2; // wave-uniform: scalar loads
#pragma unroll 4
    for (uint32_t k = 0; k < T; k++) {
        E x[kPerLane];
#pragma unroll
        for (int r = 0; r < kPerLane; r++)
            x[r] = line[slot(idx[r] - k, sh)]; // idx - k >= (output index) D >= 0
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const R gr = g[(static_cast<size_t>(b) * T + k) * 2], gi = g[(static_cast<size_t>(b) * T + k) * 2 + 1];
#pragma unroll
            for (int r = 0; r < kPerLane; r++)
                tap(gr, gi, x[r], zr[b][r], zi[b][r]);
        }
    }
    const uint32_t nlow = static_cast<uint32_t>(a.position + (m0 + mo) * D);
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const uint32_t *bd = a.bands + static_cast<size_t>(s0 + b) * 4;
        const uint32_t row = bd[0], fcw = bd[2], phase0 = bd[3];
        P y[kPerLane];
#pragma unroll
        for (int r = 0; r < kPerLane; r++)
            y[r] = mix<R>(a, zr[b][r], zi[b][r], fcw, phase0, nlow + r * D);
        P *dst = static_cast<P *>(a.out) + static_cast<uint64_t>(row) * a.out_stride + m0 + mo;
        if (sizeof(R) == 4 && ok[1] && a.vec_out) { // m0 + mo is even whenever a second output exists
            typename vec_n<R, 4>::type v;
            v[0] = y[0].x;
            v[1] = y[0].y;
            v[2] = y[1].x;
            v[3] = y[1].y;
            __builtin_nontemporal_store(v, reinterpret_cast<typename vec_n<R, 4>::type *>(dst));
        } else {
#pragma unroll
            for (int r = 0; r < kPerLane; r++)
                if (ok[r])
                    __builtin_nontemporal_store(y[r], dst + r);
        }
    }
}

template <typename R, bool CPLX> __global__ __launch_bounds__(kThreads) void sdsp_ddc_kernel(ddc_kargs a)
{
    using E = typename elem<R, CPLX>::type;
    using V = typename vec16<R>::type;
    constexpr uint32_t EL = 16 / sizeof(E); // elements per 16-byte load
    extern __shared__ __align__(16) unsigned char lds_raw[];
    E *line = reinterpret_cast<E *>(lds_raw); // [history | block], padded by slot()

    const uint32_t wg = xcd_block(blockIdx.x, gridDim.x); // neighbouring blocks of a channel behind one L2: they share T - 1 samples
    const uint32_t c = wg / a.nblk, blk = wg - c * a.nblk;
    const uint32_t b0 = a.csr[c], b1 = a.csr[c + 1];
    if (b0 == b1)
        return; // no band names this channel: nothing of it is read
    const uint32_t t = threadIdx.x, H = a.hist, D = a.down, sh = a.pad_shift;
    const uint64_t m0 = static_cast<uint64_t>(blk) * a.blk_out; // the block's first output ...
    const uint64_t n0 = m0 * D;                                 // ... and its sample
    const uint64_t left = a.samples - n0;
    const uint32_t span = a.blk_out * D;
    const uint32_t len = left < span ? static_cast<uint32_t>(left) : span; // a multiple of D
    const E *row = static_cast<const E *>(a.in) + static_cast<uint64_t>(c) * a.in_stride;
    const E *st = a.state ? static_cast<const E *>(a.state) + static_cast<uint64_t>(c) * H : nullptr;

    for (uint32_t j = t; j < H; j += kThreads) { // x[n0 - 1 - j]: the row where it reaches back that far, else the old history
        E v = E(0);
        if (j < n0)
            v = row[n0 - 1 - j];
        else if (st)
            v = st[j - n0];
        line[slot(H - 1 - j, sh)] = v;
    }
    const E *src = row + n0;
    if (a.vec_in && (n0 * sizeof(E)) % 16 == 0) {
        const uint32_t nv = len / EL;
        for (uint32_t i = t; i < nv; i += kThreads) {
            const V v = __builtin_nontemporal_load(reinterpret_cast<const V *>(src) + i);
#pragma unroll
            for (uint32_t e = 0; e < EL; e++) {
                E x;
                if constexpr (CPLX) {
                    x.x = v[2 * e];
                    x.y = v[2 * e + 1];
                } else {
                    x = v[e];
                }
                line[slot(H + i * EL + e, sh)] = x;
            }
        }
        for (uint32_t e = nv * EL + t; e < len; e += kThreads)
            line[slot(H + e, sh)] = src[e];
    } else {
        for (uint32_t e = t; e < len; e += kThreads)
            line[slot(H + e, sh)] = src[e];
    }
    __syncthreads();

    // task = (chunk of up to four of the channel's bands, group of 128 outputs): both wave-uniform
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const uint32_t no = len / D;
    const uint32_t groups = (no + kGroup - 1) / kGroup;
    const uint32_t chunks = (b1 - b0 + kBandChunk - 1) / kBandChunk;
    for (uint32_t task = wave; task < chunks * groups; task += kThreads / 64) {
        const uint32_t ck = task / groups, og = task - ck * groups;
        const uint32_t s0 = b0 + ck * kBandChunk, n = b1 - s0;
        const uint32_t mo = og * kGroup + lane * kPerLane;
        if (n >= 4) {
            band_chunk<R, CPLX, 4>(a, line, s0, mo, no, m0);
        } else {
            if (n >= 2)
                band_chunk<R, CPLX, 2>(a, line, s0, mo, no, m0);
            if (n & 1)
                band_chunk<R, CPLX, 1>(a, line, s0 + (n & 2), mo, no, m0);
        }
    }
}

// ---- variant 1: one output per thread from global memory ----------------------------------------------------------------------
template <typename R, bool CPLX> __global__ __launch_bounds__(kThreads) void sdsp_ddc_plain_kernel(ddc_kargs a)
{
    using E = typename elem<R, CPLX>::type;
    using P = typename cplx_pair<R>::type;
    const uint64_t total = a.nb * a.outs;
    const uint32_t H = a.hist;
    for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; idx < total;
         idx += static_cast<uint64_t>(gridDim.x) * kThreads) {
        const uint64_t s = udiv(idx, a.outs), m = idx - s * a.outs;
        const uint32_t *bd = a.bands + s * 4;
        const uint32_t row = bd[0], c = bd[1], fcw = bd[2], phase0 = bd[3];
        const int64_t n = static_cast<int64_t>(m * a.down);
        const E *inp = static_cast<const E *>(a.in) + static_cast<uint64_t>(c) * a.in_stride;
        const E *st = a.state ? static_cast<const E *>(a.state) + static_cast<uint64_t>(c) * H : nullptr;
        const R *g = static_cast<const R *>(a.g) + s * a.taps * 2;
        R zr = R(0), zi = R(0);
        for (uint32_t k = 0; k < a.taps; k++) {
            const int64_t xi = n - static_cast<int64_t>(k);
            const E x = xi >= 0 ? inp[xi] : (st ? st[-1 - xi] : E(0)); // -1 - xi < H: k <= taps - 1
            tap(g[2 * k], g[2 * k + 1], x, zr, zi);
        }
        const uint32_t nlow = static_cast<uint32_t>(a.position + m * a.down);
        static_cast<P *>(a.out)[static_cast<uint64_t>(row) * a.out_stride + m] = mix<R>(a, zr, zi, fcw, phase0, nlow);
    }
}

uint32_t ctz32(uint32_t v)
{
    uint32_t n = 0;
    while (!(v & 1u)) {
        v >>= 1;
        n++;
    }
    return n;
}

// the LDS line's pad: one element after every 2^shift.  Lanes read at a stride of kPerLane D elements; with 2^a the power of two in
// that stride, shift = max(a, log2 of the elements one LDS access cycle of the lane group spans) puts the lanes of a group on
// different banks: 32 elements for the 4- and 8-byte reads (32 lanes a cycle), 16 for the 16-byte read (16 lanes a cycle)
uint32_t pad_shift_for(size_t elem_bytes, uint32_t down)
{
    const uint32_t lo = elem_bytes == 16 ? 4 : 5, a = ctz32(kPerLane * down);
    return a > lo ? a : lo;
}

template <typename F> int with_kernel(int precision, int complex_in, F f)
{
    if (precision == SDSP_HIP_F64)
        return complex_in ? f(double(), std::true_type()) : f(double(), std::false_type());
    return complex_in ? f(float(), std::true_type()) : f(float(), std::false_type());
}
} // namespace

uint32_t ddc_block_out(int precision, int complex_in, uint32_t taps, uint32_t down)
{
    const size_t es = (precision == SDSP_HIP_F64 ? 8 : 4) * (complex_in ? 2 : 1);
    const uint64_t usable = kLdsTarget / es * 16 / 17; // the pad adds at most one element in 16
    const uint64_t H = taps - 1;
    uint64_t o = usable > H ? (usable - H) / down : 0;
    if (o > kMaxBlockOut)
        o = kMaxBlockOut;
    // a multiple of four keeps every block's first sample on a 16-byte boundary of an aligned row (and its first output even)
    return o >= 4 ? static_cast<uint32_t>(o & ~3ull) : (o >= 2 ? 2 : 1);
}

int ddc_prepare(int precision, int complex_in)
{
    static std::atomic<uint64_t> done[4];
    return with_kernel(precision, complex_in, [&](auto r, auto cplx) {
        constexpr bool c = decltype(cplx)::value;
        return ensure_dynamic_lds(reinterpret_cast<const void *>(sdsp_ddc_kernel<decltype(r), c>), kLdsLimit,
                                  done[(sizeof(r) == 8 ? 2 : 0) + (c ? 1 : 0)]);
    });
}

const char *ddc_kernel_for(int variant) { return variant == 1 ? "sdsp_ddc_plain_kernel" : "sdsp_ddc_kernel"; }

int launch_ddc(int precision, const ddc_args &da, int variant, void *stream_v)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const size_t rs = precision == SDSP_HIP_F64 ? 8 : 4;
    const size_t es = rs * (da.complex_in ? 2 : 1);
    ddc_kargs k{};
    k.in = da.in;
    k.out = da.out;
    k.g = da.g;
    k.coarse = da.coarse;
    k.fine = da.fine;
    k.csr = da.csr;
    k.bands = da.bands;
    k.samples = da.samples;
    k.in_stride = da.in_stride;
    k.out_stride = da.out_stride;
    k.position = da.position;
    k.outs = da.samples / da.down;
    k.taps = da.taps;
    k.down = da.down;
    k.hist = da.taps - 1;
    k.state = k.hist ? da.state : nullptr;
    k.nb = da.nb;
    k.blk_out = ddc_block_out(precision, da.complex_in, da.taps, da.down);
    k.pad_shift = pad_shift_for(es, da.down);
    k.vec_in = (reinterpret_cast<uintptr_t>(da.in) % 16 == 0 && (da.in_stride * es) % 16 == 0) ? 1 : 0;
    k.vec_out = (reinterpret_cast<uintptr_t>(da.out) % 16 == 0 && (da.out_stride * 2 * rs) % 16 == 0) ? 1 : 0;
    dim3 grid;
    if (variant == 1) {
        const uint64_t total = static_cast<uint64_t>(da.nb) * k.outs;
        if (int rc = grid_for(total < (65536ull * kThreads) ? total : 65536ull * kThreads, "ddc", &grid)) // grid-stride beyond
            return rc;
        if (int rc = with_kernel(precision, da.complex_in, [&](auto r, auto cplx) {
                hipLaunchKernelGGL((sdsp_ddc_plain_kernel<decltype(r), decltype(cplx)::value>), grid, dim3(kThreads), 0, stream, k);
                return static_cast<int>(SDSP_HIP_OK);
            }))
            return rc;
        return launch_status("ddc");
    }
    const uint64_t nblk = (k.outs + k.blk_out - 1) / k.blk_out;
    if (nblk > 0x7fffffffull)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "ddc too large for one launch");
    k.nblk = static_cast<uint32_t>(nblk);
    if (int rc = grid_of_blocks(nblk * da.channels, "ddc", &grid))
        return rc;
    const uint32_t line = k.hist + k.blk_out * da.down; // <= 4095 + 1024 or the LDS target: far inside 32 bits
    const size_t lds = static_cast<size_t>(line + (line >> k.pad_shift) + 1) * es;
    if (lds > kLdsLimit)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "ddc line exceeds the LDS limit"); // not reachable within the documented sizes
    if (int rc = with_kernel(precision, da.complex_in, [&](auto r, auto cplx) {
            hipLaunchKernelGGL((sdsp_ddc_kernel<decltype(r), decltype(cplx)::value>), grid, dim3(kThreads), lds, stream, k);
            return static_cast<int>(SDSP_HIP_OK);
        }))
        return rc;
    return launch_status("ddc");
}
} // namespace sdsp_hip
