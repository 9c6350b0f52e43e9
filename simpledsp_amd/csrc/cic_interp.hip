// cic_interp.hip -- cascaded integrator-comb (Hogenauer) interpolator banks for MI355X (gfx950): N combs of differential delay M at
// the input rate, zero-stuffing by R, N integrators at the output rate, on 16- or 32-bit integer rows, real or interleaved I/Q.
//
// All arithmetic is mod 2^W (W = 32 or 64, unsigned registers that wrap), so the serial form of the contract (sdsp_hip.h), its FIR
// form and every time-parallel form give the same bits.  What the kernels rest on:
//   - started from zero registers at input m0, the cascade computes the FIR output of the input cut off in front of m0, and an
//     output depends on at most N M inputs: every output at n >= (m0 + N M) R is exact;
//   - the first integrator over a zero-stuffed comb output is a hold: I_1[n] = g[floor(n / R)] with g[m] = sum_{i < M} c_{N-1}[m - i]
//     = sum_{k < N M} w[k] x[m - k], w = boxcar(M) (1 - z^-M)^(N - 1) (cic_interp_kargs::hold).
//
// Two kernels:
//   sdsp_cic_interp_kernel        variant 0.  A workgroup owns a segment [oa, ob) of one channel's output row and walks it in passes
//                                 of one chunk, 256 lanes x 8 consecutive outputs, from E0 <= m0 R on, m0 = floor(oa / R) - N M, with
//                                 the input taken as zero in front of m0 (and from `state` in front of the call).  Per pass a lane
//                                 forms the hold values of its 8 outputs from the row, and each of the N - 1 remaining stages is a
//                                 lane-local running sum, a wave scan of the lane totals with cross-lane moves, the wave totals
//                                 through LDS, and the offset -- carry of the passes before + waves before + lanes before -- added.
//                                 The stage carries live in LDS between passes.  The pass's outputs go through an LDS transpose
//                                 and leave as 16-byte vectors, consecutive lanes on consecutive vectors, where they lie inside
//                                 the segment; E0 is placed so that they are aligned in this row.
//   sdsp_cic_interp_plain_kernel  variant 1: one output per thread as sum_j h[p + j R] x[m - j] mod 2^W from global memory,
//                                 h = boxcar(R M)^N (sdsp_hip_cic_taps): the independent cross-check.
// The new history is carry_history's (stream_carry.hip), launched by the caller behind either kernel.
#include "cic_dev.h"

#include <type_traits>

namespace sdsp_hip
{
namespace
{
constexpr uint32_t kLane = 8;                      // consecutive outputs per lane and pass
constexpr uint32_t kChunk = kThreads * kLane;      // outputs per pass
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kMaxOrder = SDSP_HIP_CIC_MAX_ORDER;
constexpr uint32_t kMaxHold = 2 * kMaxOrder;       // N M
constexpr uint32_t kMinSegment = 16;               // automatic segments: at least this many chunks (one more pass is the warm-up's) ...
constexpr uint32_t kWarmShare = 8;                 // ... and this many times the warm-up

struct cic_interp_kargs {
    const void *in;
    void *out;
    const void *state;
    const uint64_t *taps;
    uint64_t in_stride, out_stride;
    double scale;
    uint32_t samples, n_out, channels;
    uint32_t order, up, hist;    // hist = N M inputs
    uint32_t seg, nseg;          // outputs per segment (a multiple of kChunk), segments per channel
    uint32_t out_f32;
    uint32_t ntaps;
    int32_t hold[kMaxHold];      // w[k], k < N M
};

// the register as the output type O sees it: as it is (int32 / int64), or (float)((double)y * scale)
template <typename O, typename ACC> __device__ __forceinline__ O as_out(ACC y, double scale)
{
    typedef typename signed_of<ACC>::type S;
    if constexpr (std::is_same<O, float>::value)
        return static_cast<float>(static_cast<double>(static_cast<S>(y)) * scale);
    else
        return static_cast<S>(y);
}

// the pass's outputs [np0, np0 + kChunk) of P planes, kLane consecutive ones per lane in v, to the row at `out`, those inside [lo, hi)
// only.  A lane's 16-byte vectors go to LDS in memory order and consecutive lanes store consecutive vectors, 1 KiB per wave and
// instruction: lane-strided 16-byte stores straight from the registers were measured 2 to 8 times slower.
// Whole vectors where all their elements are inside, element by element at the edges; np0 is such that the vectors are aligned.
// `reuse`: the caller has no barrier of its own between this call and the next one's LDS writes.
template <typename O, uint32_t P, typename ACC>
__device__ __forceinline__ void store_pass_lds(O *out, int64_t np0, int64_t lo, int64_t hi, const ACC (&v)[P][kLane], double scale, void *lds,
                                               uint32_t tid, bool reuse)
{
    constexpr uint32_t NS = 16 / sizeof(O);
    constexpr uint32_t VE = NS / P;
    constexpr uint32_t NV = kLane / VE;
    typedef typename vec_n<O, NS>::type vec;
    if (np0 + kChunk <= lo || np0 >= hi)
        return; // the whole workgroup
    vec *l = static_cast<vec *>(lds);
#pragma unroll
    for (uint32_t j = 0; j < NV; j++) {
        vec t;
#pragma unroll
        for (uint32_t i = 0; i < NS; i++)
            t[i] = as_out<O>(v[i % P][j * VE + i / P], scale);
        l[tid * NV + j] = t;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < NV; j++) {
        const uint32_t k = j * kThreads + tid;
        const int64_t nv = np0 + static_cast<int64_t>(k) * VE;
        if (nv + VE <= lo || nv >= hi)
            continue;
        const vec t = l[k];
        if (nv >= lo && nv + VE <= hi) {
            __builtin_nontemporal_store(t, reinterpret_cast<vec *>(out + nv * P));
        } else {
#pragma unroll
            for (uint32_t i = 0; i < NS; i++) {
                const int64_t n = nv + i / P;
                if (n >= lo && n < hi)
                    out[n * P + i % P] = t[i];
            }
        }
    }
    if (reuse)
        __syncthreads();
}

template <typename IN, bool CPLX, typename ACC> __global__ __launch_bounds__(kThreads) void sdsp_cic_interp_kernel(cic_interp_kargs a)
{
    constexpr uint32_t P = CPLX ? 2 : 1;                    // planes
    typedef typename signed_of<ACC>::type SO;
    __shared__ ACC wave_total[2][kMaxOrder][P][kWaves];     // by the pass's parity: a stage's totals are read behind its barrier, and
                                                            // with one scan stage nothing else separates that from the next pass
    __shared__ ACC carry[2][kMaxOrder][P];                  // stage registers at the start of a pass, by the pass's parity
    __shared__ __attribute__((aligned(16))) unsigned char stage[kChunk * P * sizeof(SO)]; // a pass's outputs in memory order

    const uint32_t wg = xcd_block(blockIdx.x, gridDim.x);   // neighbouring segments of a channel behind one L2: they share inputs
    const uint32_t c = wg / a.nseg, sg = wg - c * a.nseg;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t N = a.order, R = a.up, H = a.hist, S = a.samples;
    const IN *row = static_cast<const IN *>(a.in) + static_cast<uint64_t>(c) * a.in_stride * P;
    const IN *st = a.state ? static_cast<const IN *>(a.state) + static_cast<uint64_t>(c) * H * P : nullptr;
    const uint64_t osize = a.out_f32 ? sizeof(float) : sizeof(SO);
    char *orow = static_cast<char *>(a.out) + static_cast<uint64_t>(c) * a.out_stride * P * osize;

    const int64_t oa = static_cast<int64_t>(sg) * a.seg;                                    // the segment: outputs [oa, ob)
    const int64_t ob = oa + a.seg < static_cast<int64_t>(a.n_out) ? oa + a.seg : static_cast<int64_t>(a.n_out);
    // the input is taken as zero in front of m0: every output from floor(oa / R) R <= oa on is exact
    const int64_t m0 = oa / static_cast<int64_t>(R) - H;
    // E0: the first output scanned, at most m0 R and such that a lane's vectors are 16-byte aligned in this row
    const uint32_t VE = static_cast<uint32_t>(16 / (osize * P));
    const uint32_t to_line = static_cast<uint32_t>((16 - reinterpret_cast<uintptr_t>(orow) % 16) % 16 / (osize * P));
    int64_t E0 = m0 * static_cast<int64_t>(R);
    {
        int64_t r = (E0 - to_line) % static_cast<int64_t>(VE);
        if (r < 0)
            r += VE;
        E0 -= r;
    }
    // output E0 + t holds input mb + (t + tb) / R, with mb = m0 - 2 and tb = E0 - mb R in (0, 2 R]
    const int64_t mb = m0 - 2;
    const uint32_t tb = static_cast<uint32_t>(E0 - mb * static_cast<int64_t>(R));
    const uint32_t npass = static_cast<uint32_t>((ob - E0 + kChunk - 1) / kChunk);

    // x[e] of this row, widened: zero in front of m0, the state in front of the row (zeros for a null state), zero behind the row
    auto x_at = [&](int64_t e, uint32_t p) -> ACC {
        if (e < m0 || e >= static_cast<int64_t>(S))
            return 0;
        if (e >= 0)
            return widen<ACC>(row[e * P + p]);
        const int64_t j = -1 - e;
        return (st && j < static_cast<int64_t>(H)) ? widen<ACC>(st[j * P + p]) : ACC(0);
    };
    // the hold value of input m: sum_k w[k] x[m - k]
    auto hold = [&](int64_t m, ACC *g) {
#pragma unroll
        for (uint32_t p = 0; p < P; p++)
            g[p] = 0;
        for (uint32_t k = 0; k < H; k++) {
            const ACC w = static_cast<ACC>(static_cast<SO>(a.hold[k]));
#pragma unroll
            for (uint32_t p = 0; p < P; p++)
                g[p] += w * x_at(m - k, p);
        }
    };

    if (tid < kMaxOrder * P)
        carry[0][tid / P][tid % P] = 0; // read behind the first stage barrier

    for (uint32_t q = 0; q < npass; q++) {
        // t + tb < 2^32: a segment and its warm-up stay below that
        const uint32_t t0 = q * kChunk + tid * kLane;
        ACC v[P][kLane];
        {
            const uint32_t u = t0 + tb;
            const uint32_t d = u / R;
            uint32_t r = u - d * R;
            int64_t m = mb + d;
            ACC g[P];
            hold(m, g);
            if (R >= kLane) { // at most one input boundary inside the lane: both values up front, not a divergent branch per output
                const uint32_t cross = R - r;
                ACC g1[P] = {};
                if (cross < kLane)
                    hold(m + 1, g1);
#pragma unroll
                for (uint32_t i = 0; i < kLane; i++) {
#pragma unroll
                    for (uint32_t p = 0; p < P; p++)
                        v[p][i] = i < cross ? g[p] : g1[p];
                }
            } else {
#pragma unroll
                for (uint32_t i = 0; i < kLane; i++) {
#pragma unroll
                    for (uint32_t p = 0; p < P; p++)
                        v[p][i] = g[p];
                    if (++r == R && i + 1 < kLane) {
                        r = 0;
                        hold(++m, g);
                    }
                }
            }
        }

        const uint32_t par = q & 1;
        for (uint32_t s = 0; s + 1 < N; s++) {
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
                    wave_total[par][s][p][wave] = t;
                tot[p] = t - v[p][kLane - 1]; // the lanes before this one
            }
            __syncthreads();
#pragma unroll
            for (uint32_t p = 0; p < P; p++) {
                ACC off = carry[par][s][p], all = off;
#pragma unroll
                for (uint32_t w = 0; w < kWaves; w++) {
                    const ACC wt = wave_total[par][s][p][w];
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

        // with a scan stage its barrier in the next pass separates this pass's LDS reads from the next pass's writes
        const int64_t np0 = E0 + static_cast<int64_t>(q) * kChunk;
        if (a.out_f32)
            store_pass_lds<float, P>(reinterpret_cast<float *>(orow), np0, oa, ob, v, a.scale, stage, tid, N == 1);
        else
            store_pass_lds<SO, P>(reinterpret_cast<SO *>(orow), np0, oa, ob, v, a.scale, stage, tid, N == 1);
    }
}

// ---- variant 1: one output per thread as the direct polyphase FIR sum from global memory ----------------------------------------
template <typename IN, bool CPLX, typename ACC> __global__ __launch_bounds__(kThreads) void sdsp_cic_interp_plain_kernel(cic_interp_kargs a)
{
    constexpr uint32_t P = CPLX ? 2 : 1;
    typedef typename signed_of<ACC>::type SO;
    const uint64_t total = static_cast<uint64_t>(a.channels) * a.n_out;
    for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; idx < total;
         idx += static_cast<uint64_t>(gridDim.x) * kThreads) {
        const uint64_t c = udiv(idx, a.n_out), n = idx - c * a.n_out;
        const uint32_t m = static_cast<uint32_t>(n) / a.up, ph = static_cast<uint32_t>(n) - m * a.up; // m < samples
        const IN *inp = static_cast<const IN *>(a.in) + c * a.in_stride * P;
        const IN *st = a.state ? static_cast<const IN *>(a.state) + c * a.hist * P : nullptr;
        ACC y[P] = {};
        uint32_t j = 0;
        for (uint32_t k = ph; k < a.ntaps; k += a.up, j++) { // j <= hist - 1: ntaps <= hist up
            const int64_t xi = static_cast<int64_t>(m) - j;
            const ACC h = static_cast<ACC>(a.taps[k]);
#pragma unroll
            for (uint32_t p = 0; p < P; p++) {
                const IN x = xi >= 0 ? inp[xi * P + p] : (st ? st[(-1 - xi) * P + p] : IN(0));
                y[p] += h * widen<ACC>(x);
            }
        }
        const uint64_t o = (c * a.out_stride + n) * P;
#pragma unroll
        for (uint32_t p = 0; p < P; p++) {
            if (a.out_f32)
                static_cast<float *>(a.out)[o + p] = as_out<float>(y[p], a.scale);
            else
                static_cast<SO *>(a.out)[o + p] = as_out<SO>(y[p], a.scale);
        }
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

uint32_t cic_interp_chunk() { return kChunk; }

const char *cic_interp_kernel_for(int variant) { return variant == 1 ? "sdsp_cic_interp_plain_kernel" : "sdsp_cic_interp_kernel"; }

int launch_cic_interp(const cic_interp_args &aa, int variant, void *stream_v)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    cic_interp_kargs k{};
    k.in = aa.in;
    k.out = aa.out;
    k.state = aa.state;
    k.taps = static_cast<const uint64_t *>(aa.taps);
    k.in_stride = aa.in_stride;
    k.out_stride = aa.out_stride;
    k.scale = aa.scale;
    k.samples = static_cast<uint32_t>(aa.samples);
    k.n_out = static_cast<uint32_t>(aa.samples * aa.up); // < 2^31
    k.channels = static_cast<uint32_t>(aa.channels);
    k.order = aa.order;
    k.up = aa.up;
    k.hist = aa.order * aa.delay;
    k.out_f32 = aa.out_f32 ? 1 : 0;
    k.ntaps = aa.order * (aa.up * aa.delay - 1) + 1;
    {
        // w = boxcar(M) (1 - z^-M)^(N - 1): N M coefficients, the largest C(7, 3) = 35
        int64_t b = 1;
        for (uint32_t j = 0; j < aa.order; j++) { // (-1)^j C(N - 1, j) at k = j M + i, i < M
            for (uint32_t i = 0; i < aa.delay; i++)
                k.hold[j * aa.delay + i] += static_cast<int32_t>((j & 1) ? -b : b);
            b = b * (aa.order - 1 - j) / (j + 1);
        }
    }
    if (aa.channels > 0x7fffffffull)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "cic_interp too large for one launch");
    const uint64_t n_out = k.n_out;
    dim3 grid;
    if (variant == 1) {
        const uint64_t total = aa.channels * n_out;
        if (int rc = grid_for(total < (65536ull * kThreads) ? total : 65536ull * kThreads, "cic_interp", &grid)) // grid-stride beyond
            return rc;
        if (int rc = with_kernel(aa.in32, aa.complex_in, aa.reg64, [&](auto in, auto cplx, auto acc) {
                hipLaunchKernelGGL((sdsp_cic_interp_plain_kernel<decltype(in), decltype(cplx)::value, decltype(acc)>), grid,
                                   dim3(kThreads), 0, stream, k);
                return static_cast<int>(SDSP_HIP_OK);
            }))
            return rc;
        return launch_status("cic_interp");
    }
    // chunks per workgroup.  Automatic: the warm-up of hist R outputs stays a small share of a segment, and a row too short for two
    // such segments is one segment: fewer, longer segments rather than more overlap
    const uint64_t chunks = (n_out + kChunk - 1) / kChunk;
    uint64_t per = aa.segment;
    if (per == 0) {
        const uint64_t warm = static_cast<uint64_t>(k.hist) * k.up;
        const uint64_t want = std::max<uint64_t>(kMinSegment, (kWarmShare * warm + kChunk - 1) / kChunk);
        const uint64_t nseg = std::max<uint64_t>(1, chunks / want);
        per = (chunks + nseg - 1) / nseg;
    }
    k.seg = static_cast<uint32_t>(per * kChunk); // per < 2^20 + 1
    k.nseg = static_cast<uint32_t>((chunks + per - 1) / per);
    if (int rc = grid_of_blocks(aa.channels * k.nseg, "cic_interp", &grid))
        return rc;
    if (int rc = with_kernel(aa.in32, aa.complex_in, aa.reg64, [&](auto in, auto cplx, auto acc) {
            hipLaunchKernelGGL((sdsp_cic_interp_kernel<decltype(in), decltype(cplx)::value, decltype(acc)>), grid, dim3(kThreads), 0,
                               stream, k);
            return static_cast<int>(SDSP_HIP_OK);
        }))
        return rc;
    return launch_status("cic_interp");
}
} // namespace sdsp_hip
