// cic.hip -- cascaded integrator-comb (Hogenauer) decimator banks for MI355X (gfx950): N integrators at the input rate, keep every
// R-th sample, N combs of differential delay M at the output rate, on 16- or 32-bit integer rows, real or interleaved I/Q.
//
// All arithmetic is mod 2^W (W = 32 or 64, unsigned registers that wrap), so the serial form of the contract (sdsp_hip.h), its FIR
// form and every time-parallel form give the same bits.  What the kernels rest on:
//   - an output at stream index n depends on x[n - k], k = 0 .. N (R M - 1), only: whatever a cascade is started with, zero
//     registers included, hist = N M R inputs before an output are enough for that output to be exact;
//   - N combs of delay M on the decimated sequence z are y[d] = sum_j (-1)^j C(N, j) z[d - j M], also mod 2^W.
//
// Two kernels:
//   sdsp_cic_kernel        variant 0.  A workgroup owns a segment [a, b) of one channel's row and walks it in passes of one chunk,
//                          256 lanes x 8 consecutive elements, from E0 <= a - hist on (from `state` where that reaches in front of
//                          the call, zeros for NULL and in front of the state).  Per pass each lane loads its 8 elements (16-byte
//                          nontemporal loads where they lie inside the row; E0 is placed so that they are aligned), and each of
//                          the N stages is a lane-local running sum, a wave scan of the lane totals with cross-lane moves, the
//                          wave totals through LDS, and the offset -- carry of the passes before + waves before + lanes before --
//                          added: 2 N W-bit adds per sample.  The stage carries live in LDS between passes.  The last stage's
//                          values at due indices go to an LDS ring of decimated values, and the pass's outputs are formed there by
//                          the binomial sum above, consecutive lanes on consecutive outputs.
//   sdsp_cic_plain_kernel  variant 1: one output per thread as sum_k h[k] x[n - k] mod 2^W from global memory, h = boxcar(R M)^N
//                          (sdsp_hip_cic_taps): the independent cross-check.
// The new history is carry_history's (stream_carry.hip), launched by the caller behind either kernel.
#include "cic_dev.h"

#include <type_traits>

namespace sdsp_hip
{
namespace
{
constexpr uint32_t kLane = 8;                      // consecutive elements per lane and pass
constexpr uint32_t kChunk = kThreads * kLane;      // elements per pass
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kMaxOrder = SDSP_HIP_CIC_MAX_ORDER;
constexpr uint32_t kRing = kChunk / 2 + 32;        // decimated values kept: a pass's (at most kChunk / 2 + 1) and the N M <= 16 before
constexpr uint32_t kMinSegment = 4;                // automatic segments: at least this many chunks ...
constexpr uint32_t kWarmShare = 8;                 // ... and this many times the warm-up

typedef int v4i __attribute__((ext_vector_type(4)));

struct cic_kargs {
    const void *in;
    void *out;
    const void *state;
    const uint64_t *taps;
    uint64_t in_stride, out_stride;
    double scale;
    uint32_t samples, n_out, channels;
    uint32_t order, down, delay, hist;
    uint32_t phase;              // position mod R
    uint32_t seg, nseg;          // elements per segment (a multiple of kChunk), segments per channel
    uint32_t out_f32;
    uint32_t ntaps;
    int32_t binom[kMaxOrder + 1]; // (-1)^j C(N, j)
};

// y -> out[idx]: the register as it is (int32 / int64), or (float)((double)y * scale)
template <typename ACC> __device__ __forceinline__ void put(void *out, uint64_t idx, ACC y, uint32_t out_f32, double scale)
{
    typedef typename signed_of<ACC>::type S;
    if (out_f32)
        static_cast<float *>(out)[idx] = static_cast<float>(static_cast<double>(static_cast<S>(y)) * scale);
    else
        static_cast<S *>(out)[idx] = static_cast<S>(y);
}

// the 16 / sizeof(IN) scalars of one 16-byte vector
__device__ __forceinline__ void unpack(const v4i &v, int32_t *s)
{
#pragma unroll
    for (int i = 0; i < 4; i++)
        s[i] = v[i];
}
__device__ __forceinline__ void unpack(const v4i &v, int16_t *s)
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        s[2 * i] = static_cast<int16_t>(v[i]);
        s[2 * i + 1] = static_cast<int16_t>(v[i] >> 16);
    }
}
__device__ __forceinline__ v4i pack(const int32_t *s)
{
    v4i v;
#pragma unroll
    for (int i = 0; i < 4; i++)
        v[i] = s[i];
    return v;
}
__device__ __forceinline__ v4i pack(const int16_t *s)
{
    v4i v;
#pragma unroll
    for (int i = 0; i < 4; i++)
        v[i] = static_cast<int>(static_cast<uint32_t>(static_cast<uint16_t>(s[2 * i])) |
                                (static_cast<uint32_t>(static_cast<uint16_t>(s[2 * i + 1])) << 16));
    return v;
}

template <typename IN, bool CPLX, typename ACC> __global__ __launch_bounds__(kThreads) void sdsp_cic_kernel(cic_kargs a)
{
    constexpr uint32_t P = CPLX ? 2 : 1;                    // planes
    constexpr uint32_t NS = 16 / sizeof(IN);                // scalars per 16-byte vector
    constexpr uint32_t VE = NS / P;                         // elements per vector
    constexpr uint32_t NV = kLane / VE;                     // vectors per lane and pass
    __shared__ ACC ring[P][kRing];                          // decimated values of the last stage, by d mod kRing
    __shared__ ACC wave_total[kMaxOrder][P][kWaves];
    __shared__ ACC carry[2][kMaxOrder][P];                  // stage registers at the start of a pass, by the pass's parity

    const uint32_t wg = xcd_block(blockIdx.x, gridDim.x);   // neighbouring segments of a channel behind one L2: they overlap by hist
    const uint32_t c = wg / a.nseg, sg = wg - c * a.nseg;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t N = a.order, R = a.down, M = a.delay, H = a.hist, S = a.samples;
    const IN *row = static_cast<const IN *>(a.in) + static_cast<uint64_t>(c) * a.in_stride * P;
    const IN *st = a.state ? static_cast<const IN *>(a.state) + static_cast<uint64_t>(c) * H * P : nullptr;
    const uint64_t out_row = static_cast<uint64_t>(c) * a.out_stride;

    const int64_t sa = static_cast<int64_t>(sg) * a.seg;                                    // the segment: elements [sa, sb)
    const int64_t sb = sa + a.seg < static_cast<int64_t>(S) ? sa + a.seg : static_cast<int64_t>(S);
    // E0: the first element scanned, at most sa - hist and such that a lane's vectors are 16-byte aligned in this row
    const uint32_t to_line = static_cast<uint32_t>((16 - reinterpret_cast<uintptr_t>(row) % 16) % 16 / (sizeof(IN) * P));
    int64_t E0 = sa - H;
    {
        int64_t r = (E0 - to_line) % static_cast<int64_t>(VE);
        if (r < 0)
            r += VE;
        E0 -= r;
    }
    // stream index of E0 = position + E0 = qq R + ph with 0 <= ph < R; element E0 + t is due when (t + ph) mod R == R - 1, and it is
    // decimated value d = (t + ph) / R of this segment and output m = d + qq of the call
    int64_t qq;
    uint32_t ph;
    {
        const int64_t g = static_cast<int64_t>(a.phase) + E0;
        qq = g / static_cast<int64_t>(R);
        int64_t r = g - qq * static_cast<int64_t>(R);
        if (r < 0) {
            r += R;
            qq--;
        }
        ph = static_cast<uint32_t>(r);
    }
    const uint32_t npass = static_cast<uint32_t>((sb - E0 + kChunk - 1) / kChunk);

    // x[e] of this row as stored: the row, the state in front of it, zeros in front of that, behind the row and for a null state
    auto x_at = [&](int64_t e, uint32_t p) -> IN {
        if (e >= 0)
            return e < static_cast<int64_t>(S) ? row[e * P + p] : IN(0);
        const int64_t j = -1 - e;
        return (st && j < static_cast<int64_t>(H)) ? st[j * P + p] : IN(0);
    };
    // the lane's NV vectors of pass q
    auto load = [&](uint32_t q, v4i *raw) {
        const int64_t e0 = E0 + static_cast<int64_t>(q) * kChunk + tid * kLane;
#pragma unroll
        for (uint32_t j = 0; j < NV; j++) {
            const int64_t ev = e0 + j * VE;
            if (ev >= 0 && ev + VE <= static_cast<int64_t>(S)) {
                raw[j] = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(row + ev * P));
            } else {
                IN s[NS];
#pragma unroll
                for (uint32_t i = 0; i < NS; i++)
                    s[i] = x_at(ev + i / P, i % P);
                raw[j] = pack(s);
            }
        }
    };

    if (tid < kMaxOrder * P)
        carry[0][tid / P][tid % P] = 0; // read behind the first stage barrier

    v4i raw[NV];
    load(0, raw);
    for (uint32_t q = 0; q < npass; q++) {
        ACC v[P][kLane];
#pragma unroll
        for (uint32_t j = 0; j < NV; j++) {
            IN s[NS];
            unpack(raw[j], s);
#pragma unroll
            for (uint32_t i = 0; i < NS; i++)
                v[i % P][j * VE + i / P] = widen<ACC>(s[i]);
        }
        if (q + 1 < npass)
            load(q + 1, raw);

        const uint32_t par = q & 1;
        for (uint32_t s = 0; s < N; s++) {
            ACC tot[P];
#pragma unroll
            for (uint32_t p = 0; p < P; p++) {
#pragma unroll
                for (uint32_t i = 1; i < kLane; i++)
                    v[p][i] += v[p][i - 1];
                ACC t = v[p][kLane - 1]; // inclusive scan of the lane totals over the wave
#pragma unroll
                for (uint32_t d = 1; d < 64; d *= 2) {
                    const ACC u = lane_up(t, d);
                    if (lane >= d)
                        t += u;
                }
                if (lane == 63)
                    wave_total[s][p][wave] = t;
                tot[p] = t - v[p][kLane - 1]; // the lanes before this one
            }
            __syncthreads();
#pragma unroll
            for (uint32_t p = 0; p < P; p++) {
                ACC off = carry[par][s][p], all = off;
#pragma unroll
                for (uint32_t w = 0; w < kWaves; w++) {
                    const ACC wt = wave_total[s][p][w];
                    all += wt;
                    if (w < wave)
                        off += wt;
                }
                if (tid == 0)
                    carry[par ^ 1][s][p] = all; // read in the next pass behind its stage barrier; this pass reads carry[par]
                off += tot[p];
#pragma unroll
                for (uint32_t i = 0; i < kLane; i++)
                    v[p][i] += off;
            }
        }

        // due values of the last stage -> ring.  The pass before read the ring ahead of this pass's stage barriers (N >= 1)
        const uint32_t T0 = q * kChunk; // t of the pass's first element; t + ph < 2^32: a segment and its warm-up stay below that
        {
            const uint32_t u = T0 + tid * kLane + ph;
            uint32_t d = u / R, r = u - d * R;
#pragma unroll
            for (uint32_t i = 0; i < kLane; i++) {
                if (r == R - 1) {
#pragma unroll
                    for (uint32_t p = 0; p < P; p++)
                        ring[p][d % kRing] = v[p][i];
                }
                if (++r == R) {
                    r = 0;
                    d++;
                }
            }
        }
        __syncthreads();
        // the pass's outputs: decimated indices [dlo, dhi); those of the segment's own elements are stored
        const uint32_t dlo = (T0 + ph) / R, dhi = (T0 + kChunk + ph) / R;
        for (uint32_t d = dlo + tid; d < dhi; d += kThreads) {
            const int64_t e = E0 + static_cast<int64_t>(d) * R + (R - 1 - ph);
            const int64_t m = static_cast<int64_t>(d) + qq;
            if (e < sa || e >= sb || m < 0 || m >= static_cast<int64_t>(a.n_out))
                continue; // e >= sa >= E0 + hist: d >= N M, every value read below was written by this workgroup
#pragma unroll
            for (uint32_t p = 0; p < P; p++) {
                ACC y = ring[p][d % kRing];
                for (uint32_t j = 1; j <= N; j++)
                    y += static_cast<ACC>(static_cast<typename signed_of<ACC>::type>(a.binom[j])) * ring[p][(d - j * M) % kRing];
                put<ACC>(a.out, (out_row + static_cast<uint64_t>(m)) * P + p, y, a.out_f32, a.scale);
            }
        }
    }
}

// ---- variant 1: one output per thread as the direct FIR sum from global memory ------------------------------------------------
template <typename IN, bool CPLX, typename ACC> __global__ __launch_bounds__(kThreads) void sdsp_cic_plain_kernel(cic_kargs a)
{
    constexpr uint32_t P = CPLX ? 2 : 1;
    const uint64_t total = static_cast<uint64_t>(a.channels) * a.n_out;
    for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; idx < total;
         idx += static_cast<uint64_t>(gridDim.x) * kThreads) {
        const uint64_t c = udiv(idx, a.n_out), m = idx - c * a.n_out;
        const int64_t n = static_cast<int64_t>(m) * a.down + (a.down - 1 - a.phase); // the m-th due index of the call, < samples
        const IN *inp = static_cast<const IN *>(a.in) + c * a.in_stride * P;
        const IN *st = a.state ? static_cast<const IN *>(a.state) + c * a.hist * P : nullptr;
        ACC y[P] = {};
        for (uint32_t k = 0; k < a.ntaps; k++) { // n - k > -hist: ntaps <= hist
            const int64_t xi = n - static_cast<int64_t>(k);
            const ACC h = static_cast<ACC>(a.taps[k]);
#pragma unroll
            for (uint32_t p = 0; p < P; p++) {
                const IN x = xi >= 0 ? inp[xi * P + p] : (st ? st[(-1 - xi) * P + p] : IN(0));
                y[p] += h * widen<ACC>(x);
            }
        }
#pragma unroll
        for (uint32_t p = 0; p < P; p++)
            put<ACC>(a.out, (c * a.out_stride + m) * P + p, y[p], a.out_f32, a.scale);
    }
}

template <typename F> int with_kernel(int in32, int complex_in, int reg64, F f)
{
    auto pick = [&](auto in) {
        if (complex_in)
            return reg64 ? f(in, std::true_type(), uint64_t()) : f(in, std::true_type(), uint32_t());
        return reg64 ? f(in, std::false_type(), uint64_t()) : f(in, std::false_type(), uint32_t());
    };
    return in32 ? pick(int32_t()) : pick(int16_t());
}
} // namespace

uint32_t cic_chunk() { return kChunk; }

const char *cic_kernel_for(int variant) { return variant == 1 ? "sdsp_cic_plain_kernel" : "sdsp_cic_kernel"; }

int launch_cic(const cic_args &aa, int variant, void *stream_v)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    cic_kargs k{};
    k.in = aa.in;
    k.out = aa.out;
    k.state = aa.state;
    k.taps = static_cast<const uint64_t *>(aa.taps);
    k.in_stride = aa.in_stride;
    k.out_stride = aa.out_stride;
    k.scale = aa.scale;
    k.samples = static_cast<uint32_t>(aa.samples);
    k.n_out = static_cast<uint32_t>(aa.n_out);
    k.channels = static_cast<uint32_t>(aa.channels);
    k.order = aa.order;
    k.down = aa.down;
    k.delay = aa.delay;
    k.hist = aa.order * aa.delay * aa.down;
    k.phase = static_cast<uint32_t>(aa.position % aa.down);
    k.out_f32 = aa.out_f32 ? 1 : 0;
    k.ntaps = aa.order * (aa.down * aa.delay - 1) + 1;
    int64_t b = 1;
    for (uint32_t j = 0; j <= aa.order; j++) { // (-1)^j C(N, j)
        k.binom[j] = static_cast<int32_t>((j & 1) ? -b : b);
        b = b * (aa.order - j) / (j + 1);
    }
    if (aa.channels > 0x7fffffffull)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "cic too large for one launch");
    dim3 grid;
    if (variant == 1) {
        const uint64_t total = aa.channels * aa.n_out;
        if (int rc = grid_for(total < (65536ull * kThreads) ? total : 65536ull * kThreads, "cic", &grid)) // grid-stride beyond
            return rc;
        if (int rc = with_kernel(aa.in32, aa.complex_in, aa.reg64, [&](auto in, auto cplx, auto acc) {
                hipLaunchKernelGGL((sdsp_cic_plain_kernel<decltype(in), decltype(cplx)::value, decltype(acc)>), grid, dim3(kThreads), 0,
                                   stream, k);
                return static_cast<int>(SDSP_HIP_OK);
            }))
            return rc;
        return launch_status("cic");
    }
    // chunks per workgroup.  Automatic: the warm-up of hist inputs stays a small share of a segment, and a row too short for two
    // such segments is one segment: fewer, longer segments rather than more overlap
    const uint64_t chunks = (aa.samples + kChunk - 1) / kChunk;
    uint64_t per = aa.segment;
    if (per == 0) {
        const uint64_t want = std::max<uint64_t>(kMinSegment, (static_cast<uint64_t>(kWarmShare) * k.hist + kChunk - 1) / kChunk);
        const uint64_t nseg = std::max<uint64_t>(1, chunks / want);
        per = (chunks + nseg - 1) / nseg;
    }
    k.seg = static_cast<uint32_t>(per * kChunk); // per < 2^20 + 1
    k.nseg = static_cast<uint32_t>((chunks + per - 1) / per);
    if (int rc = grid_of_blocks(aa.channels * k.nseg, "cic", &grid))
        return rc;
    if (int rc = with_kernel(aa.in32, aa.complex_in, aa.reg64, [&](auto in, auto cplx, auto acc) {
            hipLaunchKernelGGL((sdsp_cic_kernel<decltype(in), decltype(cplx)::value, decltype(acc)>), grid, dim3(kThreads), 0, stream, k);
            return static_cast<int>(SDSP_HIP_OK);
        }))
        return rc;
    return launch_status("cic");
}
} // namespace sdsp_hip
