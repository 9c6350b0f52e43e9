// duc.hip -- digital up-converter banks for MI355X (gfx950): interpolate every band by U through h[0..T) in polyphase form, shift it up
// to its centre frequency, sum the bands of each output channel.  The mirror of ddc.hip.
//
// Output r of a channel of a call (m = r div U, p = r mod U, n = position U + r; x = a band's history, then its block):
//     z = sum over q of h[q U + p] x[m - q]      ascending q while q U + p < T, from +0; one fmaf per step in f32, a multiply then an
//                                                add in f64; a phase without taps gives (+0, +0)
//     w = conj(C[j >> 16] (x) F[j & 0xffff]),    j = (phase0 + fcw n) mod 2^32 in unsigned integers; C, F: the DDC's tables
//     y = z (x) w                                (a (x) b): two products and one sum or difference, each rounded on its own
//     out = sum of y over the channel's bands in ascending band index, from +0, one rounded add each (REAL: of y.re only)
// h, C and F come rounded from the plan (capi.hip); built with -ffp-contract=off, so nothing here contracts.  DESIGN.md section 5.20.
//
// Two kernels:
//   sdsp_duc_kernel        variant 0.  A workgroup owns one output channel and one block of blk_in input positions (blk_in U <= 1024
//                          consecutive outputs).  It stages h in LDS once, then the channel's bands in chunks of up to four: each
//                          band's blk_in + H inputs (history from `state` or from the row) with 16-byte nontemporal loads.  Lane t owns
//                          outputs t, t + 256, t + 512, t + 768 of the block and keeps their running sums over ALL of the channel's
//                          bands in registers: per q one tap read per output (consecutive lanes read consecutive taps) serves the
//                          bands of the chunk, and the x read is one address for all lanes that share m (a broadcast).  Every output
//                          element is stored once, by its one owner, in rows of 64 consecutive elements per wave; no atomics and no
//                          read of `out`.  A channel without bands stores zeros and reads nothing.
//   sdsp_duc_plain_kernel  variant 1: one output per thread straight from global memory, looping over the channel's bands: the
//                          independent cross-check.
// The new history is carry_history's (stream_carry.hip), launched by the caller behind either kernel.
#include "stream_dev.h"

#include <type_traits>

namespace sdsp_hip
{
namespace
{
constexpr int kPerLane = 4;                          // outputs per lane, kThreads apart
constexpr uint32_t kBlockOuts = kThreads * kPerLane; // outputs per block at the most
constexpr uint32_t kBandChunk = 4;                   // bands staged together: they share the tap reads
constexpr size_t kLdsTarget = 64 * 1024;             // taps + staged lines (two workgroups per CU); long histories alone may need more
// the largest a plan can ask for: f64, T = 4096, U = 1 (32 KiB of taps and one line of 4095 + 1024 elements: 112 KiB).  Every
// instantiation of the fused kernel gets this one dynamic-LDS limit, set once per device at plan creation (duc_prepare)
constexpr size_t kLdsLimit = 128 * 1024;

template <typename R> __device__ __forceinline__ R mul_add(R g, R x, R acc);
template <> __device__ __forceinline__ float mul_add<float>(float g, float x, float acc) { return __builtin_fmaf(g, x, acc); }
template <> __device__ __forceinline__ double mul_add<double>(double g, double x, double acc) { return acc + g * x; }

// a (x) b: every product and the sum or difference rounded on its own
template <typename R> __device__ __forceinline__ typename cplx_pair<R>::type cmul(typename cplx_pair<R>::type a, typename cplx_pair<R>::type b)
{
    typename cplx_pair<R>::type r;
    r.x = a.x * b.x - a.y * b.y;
    r.y = a.x * b.y + a.y * b.x;
    return r;
}

struct duc_kargs {
    const void *in;
    void *out;
    const void *state;
    const void *h, *coarse, *fine;
    const uint32_t *csr, *bands;
    uint64_t samples, in_stride, out_stride, outs; // outs = samples U
    uint32_t pos_lo;                               // (position U) mod 2^32: all the phase needs
    uint32_t taps, up, hist, channels;
    uint32_t blk_in;    // input positions per block
    uint32_t nblk;      // blocks per channel
    uint32_t chunk;     // bands per staged chunk (1 .. kBandChunk)
    uint32_t tap_bytes; // LDS in front of the lines
    uint32_t vec_in;    // rows 16-byte aligned
};

// w = conj(C (x) F) for stream index n (mod 2^32)
template <typename R> __device__ __forceinline__ typename cplx_pair<R>::type osc(const duc_kargs &a, uint32_t fcw, uint32_t phase0, uint32_t n)
{
    using P = typename cplx_pair<R>::type;
    const uint32_t j = phase0 + fcw * n;
    const P c = static_cast<const P *>(a.coarse)[j >> 16];
    const P f = static_cast<const P *>(a.fine)[j & 0xffffu];
    P w = cmul<R>(c, f);
    w.y = -w.y;
    return w;
}

// y = z (x) w added to the running sums (REAL: the real part only)
template <typename R, bool REAL_OUT>
__device__ __forceinline__ void mix_add(typename cplx_pair<R>::type w, R zr, R zi, R &acc_r, R &acc_i)
{
    const R yr = zr * w.x - zi * w.y;
    acc_r = acc_r + yr;
    if constexpr (!REAL_OUT) {
        const R yi = zr * w.y + zi * w.x;
        acc_i = acc_i + yi;
    }
}

// NB staged bands (table entries s0 ..) for the lane's kPerLane outputs: idx = line index of x[m], k0 = p, n0 = stream index of the
// block's output 0
template <typename R, bool REAL_OUT, int NB>
__device__ __forceinline__ void band_chunk(const duc_kargs &a, const R *hs, const typename cplx_pair<R>::type *line, uint32_t pitch, uint32_t s0,
                                           const uint32_t (&idx)[kPerLane], const uint32_t (&k0)[kPerLane], uint32_t n0, R (&acc_r)[kPerLane],
                                           R (&acc_i)[kPerLane])
{
    using P = typename cplx_pair<R>::type;
    const uint32_t T = a.taps, U = a.up;
    R zr[NB][kPerLane], zi[NB][kPerLane];
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
        for (int i = 0; i < kPerLane; i++)
            zr[b][i] = zi[b][i] = R(0);
    const uint32_t Q = a.hist + 1; // ceil(T / U)
    for (uint32_t q = 0; q < Q; q++) {
        R g[kPerLane];
        bool on[kPerLane];
#pragma unroll
        for (int i = 0; i < kPerLane; i++) {
            const uint32_t k = q * U + k0[i];
            on[i] = k < T; // only the last q can run past the taps: that phase has no tap there, and none is made up
            g[i] = hs[on[i] ? k : 0];
        }
#pragma unroll
        for (int b = 0; b < NB; b++)
#pragma unroll
            for (int i = 0; i < kPerLane; i++) {
                const P x = line[b * pitch + idx[i] - q]; // idx - q >= m >= 0: q <= H
                const R nr = mul_add<R>(g[i], x.x, zr[b][i]), ni = mul_add<R>(g[i], x.y, zi[b][i]);
                zr[b][i] = on[i] ? nr : zr[b][i];
                zi[b][i] = on[i] ? ni : zi[b][i];
            }
    }
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const uint32_t *bd = a.bands + static_cast<size_t>(s0 + b) * 4;
        const uint32_t fcw = bd[2], phase0 = bd[3];
#pragma unroll
        for (int i = 0; i < kPerLane; i++)
            mix_add<R, REAL_OUT>(osc<R>(a, fcw, phase0, n0 + threadIdx.x + i * kThreads), zr[b][i], zi[b][i], acc_r[i], acc_i[i]);
    }
}

template <typename R, bool REAL_OUT> __global__ __launch_bounds__(kThreads) void sdsp_duc_kernel(duc_kargs a)
{
    using P = typename cplx_pair<R>::type;
    using V = typename vec16<R>::type;
    constexpr uint32_t EL = 16 / sizeof(P); // elements per 16-byte load
    extern __shared__ __align__(16) unsigned char lds_raw[];
    R *hs = reinterpret_cast<R *>(lds_raw);                  // h in natural order
    P *lines = reinterpret_cast<P *>(lds_raw + a.tap_bytes); // chunk x [history | block]

    const uint32_t wg = xcd_block(blockIdx.x, gridDim.x); // neighbouring blocks of a channel behind one L2: they share H inputs per band
    const uint32_t c = wg / a.nblk, blk = wg - c * a.nblk;
    const uint32_t b0 = a.csr[c], b1 = a.csr[c + 1];
    const uint32_t t = threadIdx.x, T = a.taps, U = a.up, H = a.hist;
    const uint64_t m0 = static_cast<uint64_t>(blk) * a.blk_in; // the block's first input position ...
    const uint64_t o0 = m0 * U;                                // ... and its first output
    const uint64_t left = a.samples - m0;
    const uint32_t len = left < a.blk_in ? static_cast<uint32_t>(left) : a.blk_in;
    const uint32_t nout = len * U; // <= kBlockOuts
    const uint32_t pitch = a.blk_in + H;

    bool ok[kPerLane];
    uint32_t idx[kPerLane], k0[kPerLane]; // a lane past the block's outputs works on output 0 and stores nothing
    R acc_r[kPerLane], acc_i[kPerLane];
#pragma unroll
    for (int i = 0; i < kPerLane; i++) {
        const uint32_t r = t + i * kThreads;
        ok[i] = r < nout;
        const uint32_t rr = ok[i] ? r : 0, m = rr / U;
        idx[i] = H + m;
        k0[i] = rr - m * U;
        acc_r[i] = acc_i[i] = R(0);
    }

    if (b0 != b1) { // (uniform over the workgroup)
        for (uint32_t j = t; j < T; j += kThreads)
            hs[j] = static_cast<const R *>(a.h)[j];
        const uint32_t n0 = a.pos_lo + static_cast<uint32_t>(o0);
        for (uint32_t s0 = b0; s0 < b1; s0 += a.chunk) {
            const uint32_t n = b1 - s0 < a.chunk ? b1 - s0 : a.chunk;
            if (s0 != b0)
                __syncthreads(); // the previous chunk has been read
            for (uint32_t b = 0; b < n; b++) {
                const uint32_t band = a.bands[static_cast<size_t>(s0 + b) * 4];
                const P *row = static_cast<const P *>(a.in) + static_cast<uint64_t>(band) * a.in_stride;
                const P *st = a.state ? static_cast<const P *>(a.state) + static_cast<uint64_t>(band) * H : nullptr;
                P *line = lines + b * pitch;
                for (uint32_t j = t; j < H; j += kThreads) { // x[m0 - 1 - j]: the row where it reaches back that far, else the old history
                    P v = P(0);
                    if (j < m0)
                        v = row[m0 - 1 - j];
                    else if (st)
                        v = st[j - m0];
                    line[H - 1 - j] = v;
                }
                const P *src = row + m0;
                if (a.vec_in && (m0 * sizeof(P)) % 16 == 0) {
                    const uint32_t nv = len / EL;
                    for (uint32_t i = t; i < nv; i += kThreads) {
                        const V v = __builtin_nontemporal_load(reinterpret_cast<const V *>(src) + i);
#pragma unroll
                        for (uint32_t e = 0; e < EL; e++) {
                            P x;
                            x.x = v[2 * e];
                            x.y = v[2 * e + 1];
                            line[H + i * EL + e] = x;
                        }
                    }
                    for (uint32_t e = nv * EL + t; e < len; e += kThreads)
                        line[H + e] = src[e];
                } else {
                    for (uint32_t e = t; e < len; e += kThreads)
                        line[H + e] = src[e];
                }
            }
            __syncthreads();
            if (n >= 4) {
                band_chunk<R, REAL_OUT, 4>(a, hs, lines, pitch, s0, idx, k0, n0, acc_r, acc_i);
            } else {
                if (n >= 2)
                    band_chunk<R, REAL_OUT, 2>(a, hs, lines, pitch, s0, idx, k0, n0, acc_r, acc_i);
                if (n & 1)
                    band_chunk<R, REAL_OUT, 1>(a, hs, lines + (n & 2) * pitch, pitch, s0 + (n & 2), idx, k0, n0, acc_r, acc_i);
            }
        }
    }

    // each wave stores rows of 64 consecutive elements; every element of the block has this one owner
    if constexpr (REAL_OUT) {
        R *dst = static_cast<R *>(a.out) + static_cast<uint64_t>(c) * a.out_stride + o0 + t;
#pragma unroll
        for (int i = 0; i < kPerLane; i++)
            if (ok[i])
                __builtin_nontemporal_store(acc_r[i], dst + i * kThreads);
    } else {
        P *dst = static_cast<P *>(a.out) + static_cast<uint64_t>(c) * a.out_stride + o0 + t;
#pragma unroll
        for (int i = 0; i < kPerLane; i++)
            if (ok[i]) {
                P y;
                y.x = acc_r[i];
                y.y = acc_i[i];
                __builtin_nontemporal_store(y, dst + i * kThreads);
            }
    }
}

// ---- variant 1: one output per thread from global memory ----------------------------------------------------------------------
template <typename R, bool REAL_OUT> __global__ __launch_bounds__(kThreads) void sdsp_duc_plain_kernel(duc_kargs a)
{
    using P = typename cplx_pair<R>::type;
    const uint64_t total = a.channels * a.outs;
    const uint32_t H = a.hist, T = a.taps, U = a.up;
    const R *h = static_cast<const R *>(a.h);
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < total; i += static_cast<uint64_t>(gridDim.x) * kThreads) {
        const uint64_t c = udiv(i, a.outs), r = i - c * a.outs;
        const uint64_t m = udiv(r, U);
        const uint32_t p = static_cast<uint32_t>(r - m * U);
        const uint32_t n = a.pos_lo + static_cast<uint32_t>(r);
        R acc_r = R(0), acc_i = R(0);
        for (uint32_t s = a.csr[c]; s < a.csr[c + 1]; s++) {
            const uint32_t *bd = a.bands + static_cast<size_t>(s) * 4;
            const uint32_t band = bd[0], fcw = bd[2], phase0 = bd[3];
            const P *inp = static_cast<const P *>(a.in) + static_cast<uint64_t>(band) * a.in_stride;
            const P *st = a.state ? static_cast<const P *>(a.state) + static_cast<uint64_t>(band) * H : nullptr;
            R zr = R(0), zi = R(0);
            uint32_t q = 0;
            for (uint32_t k = p; k < T; k += U, q++) {
                P x = P(0);
                if (q <= m)
                    x = inp[m - q];
                else if (st)
                    x = st[q - m - 1]; // q - m - 1 < H: q <= H
                zr = mul_add<R>(h[k], x.x, zr);
                zi = mul_add<R>(h[k], x.y, zi);
            }
            mix_add<R, REAL_OUT>(osc<R>(a, fcw, phase0, n), zr, zi, acc_r, acc_i);
        }
        if constexpr (REAL_OUT) {
            static_cast<R *>(a.out)[c * a.out_stride + r] = acc_r;
        } else {
            P y;
            y.x = acc_r;
            y.y = acc_i;
            static_cast<P *>(a.out)[c * a.out_stride + r] = y;
        }
    }
}

template <typename F> int with_kernel(int precision, int real_out, F f)
{
    if (precision == SDSP_HIP_F64)
        return real_out ? f(double(), std::true_type()) : f(double(), std::false_type());
    return real_out ? f(float(), std::true_type()) : f(float(), std::false_type());
}

// the fused kernel's block, chunk and LDS bytes for these sizes
void duc_shape(int precision, uint32_t taps, uint32_t up, uint32_t *blk_in, uint32_t *chunk, size_t *lds, uint32_t *tap_bytes)
{
    const size_t rs = precision == SDSP_HIP_F64 ? 8 : 4, es = 2 * rs;
    const uint32_t tb = static_cast<uint32_t>((taps * rs + 15) & ~static_cast<size_t>(15)); // <= 32 KiB
    const uint32_t H = (taps - 1) / up;
    uint32_t base = kBlockOuts / up; // every lane of the workgroup busy where U allows it
    if (base < 1)
        base = 1;
    if (base >= 4)
        base &= ~3u; // a multiple of four keeps every block's first input on a 16-byte boundary of an aligned row
    const uint32_t budget = static_cast<uint32_t>((kLdsTarget - tb) / es); // elements beside the taps inside the target
    uint32_t b = base, kc = 1;
    if (budget >= base + H) {
        kc = budget / (base + H);
        if (kc > kBandChunk)
            kc = kBandChunk;
    } else if (budget > H && (budget - H) * 4 >= base) { // a smaller block where it keeps the target and a quarter of the lanes busy
        b = budget - H;
        if (b >= 4)
            b &= ~3u;
    } // else: the history alone (nearly) fills the target: one full block in a line above it, within kLdsLimit
    *blk_in = b;
    *chunk = kc;
    *tap_bytes = tb;
    *lds = tb + static_cast<size_t>(kc) * (b + H) * es;
}
} // namespace

uint32_t duc_block_in(int precision, uint32_t taps, uint32_t up)
{
    uint32_t b = 0, kc = 0, tb = 0;
    size_t lds = 0;
    duc_shape(precision, taps, up, &b, &kc, &lds, &tb);
    return b;
}

int duc_prepare(int precision, int real_out)
{
    static std::atomic<uint64_t> done[4];
    return with_kernel(precision, real_out, [&](auto r, auto real) {
        constexpr bool ro = decltype(real)::value;
        return ensure_dynamic_lds(reinterpret_cast<const void *>(sdsp_duc_kernel<decltype(r), ro>), kLdsLimit,
                                  done[(sizeof(r) == 8 ? 2 : 0) + (ro ? 1 : 0)]);
    });
}

const char *duc_kernel_for(int variant) { return variant == 1 ? "sdsp_duc_plain_kernel" : "sdsp_duc_kernel"; }

int launch_duc(int precision, const duc_args &da, int variant, void *stream_v)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const size_t es = precision == SDSP_HIP_F64 ? 16 : 8;
    duc_kargs k{};
    k.in = da.in;
    k.out = da.out;
    k.h = da.h;
    k.coarse = da.coarse;
    k.fine = da.fine;
    k.csr = da.csr;
    k.bands = da.bands;
    k.samples = da.samples;
    k.in_stride = da.in_stride;
    k.out_stride = da.out_stride;
    k.outs = da.samples * da.up;
    k.pos_lo = static_cast<uint32_t>(da.position) * da.up; // mod 2^32
    k.taps = da.taps;
    k.up = da.up;
    k.hist = (da.taps - 1) / da.up;
    k.state = k.hist ? da.state : nullptr;
    k.channels = da.channels;
    size_t lds = 0;
    duc_shape(precision, da.taps, da.up, &k.blk_in, &k.chunk, &lds, &k.tap_bytes);
    k.vec_in = (reinterpret_cast<uintptr_t>(da.in) % 16 == 0 && (da.in_stride * es) % 16 == 0) ? 1 : 0;
    dim3 grid;
    if (variant == 1) {
        const uint64_t total = static_cast<uint64_t>(da.channels) * k.outs;
        if (int rc = grid_for(total < (65536ull * kThreads) ? total : 65536ull * kThreads, "duc", &grid)) // grid-stride beyond
            return rc;
        if (int rc = with_kernel(precision, da.real_out, [&](auto r, auto real) {
                hipLaunchKernelGGL((sdsp_duc_plain_kernel<decltype(r), decltype(real)::value>), grid, dim3(kThreads), 0, stream, k);
                return static_cast<int>(SDSP_HIP_OK);
            }))
            return rc;
        return launch_status("duc");
    }
    const uint64_t nblk = (da.samples + k.blk_in - 1) / k.blk_in;
    if (nblk > 0x7fffffffull)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "duc too large for one launch");
    k.nblk = static_cast<uint32_t>(nblk);
    if (int rc = grid_of_blocks(nblk * da.channels, "duc", &grid))
        return rc;
    if (lds > kLdsLimit)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "duc lines exceed the LDS limit"); // not reachable within the documented sizes
    if (int rc = with_kernel(precision, da.real_out, [&](auto r, auto real) {
            hipLaunchKernelGGL((sdsp_duc_kernel<decltype(r), decltype(real)::value>), grid, dim3(kThreads), lds, stream, k);
            return static_cast<int>(SDSP_HIP_OK);
        }))
        return rc;
    return launch_status("duc");
}
} // namespace sdsp_hip
