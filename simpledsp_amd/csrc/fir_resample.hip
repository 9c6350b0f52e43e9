// fir_resample.hip -- polyphase FIR resampler banks for MI355X (gfx950): up by U, filter with h[0..T), down by D, out of place.
//
// Output m of a call (x = history, then the block; g = gcd(U, D), q = D / g; samples S a multiple of q, S U / D outputs):
//     y[m] = sum over k < T with (m D - k) = 0 (mod U) of h[k] x[(m D - k) / U]
// With n = m D, phase p = n mod U and base b = floor(n / U) this is y[m] = sum_{j < T_p} h[p + j U] x[b - j], T_p = the number of
// taps of phase p (0 when p >= T).  Every output sums exactly its own taps in ascending k: the first term is a plain multiply,
// each further one a multiply and an add in f64 (built with -ffp-contract=off) and one fmaf in f32.  Nothing is padded with zero
// taps, so a non-finite input reaches only the outputs whose taps touch it, and the result equals zero-stuff -> direct FIR ->
// every D-th sample bit for bit (signed zeros aside).  DESIGN.md section 5.10.
//
// Three kernels:
//   sdsp_resample_dec_kernel   U = 1, D in {1, 2, 4, 8, 16} (variant 0).  The machinery of sdsp_fir_kernel (fir.hip): a group of
//                              threads owns a row, 16-byte nontemporal loads into a padded LDS line with the history in front,
//                              a 16-sample block per thread and a sliding register window over 16-tap chunks; the thread keeps
//                              only the 16 / D outputs of its block that land on multiples of D, so the coefficients stay
//                              wave-uniform (SGPR) and one LDS block read serves 16 / D * 16 multiply-adds.
//   sdsp_resample_poly_kernel  every other (U, D) (variant 0) and any (U, D) as variant 2.  One workgroup per row; the input comes
//                              through an LDS line in blocks of a multiple of lcm(q, 4) samples, sized for 256 periods (q inputs
//                              each) within a 48 KiB line.  A wave takes one output phase at a time (so h[p + j U] is
//                              wave-uniform), each lane four periods of that phase, 64 apart, on four accumulators.
//   sdsp_resample_plain_kernel variant 1: one output per thread straight from global memory (+ sdsp_resample_state_kernel for the
//                              history), the independent cross-check.
#include "stream_dev.h"

namespace sdsp_hip
{
namespace
{
constexpr int kBlk = 16;       // samples per thread and LDS block (dec kernel)
constexpr int kPolyThreads = 256;
constexpr int kAcc = 4;           // poly kernel: independent output chains per lane
constexpr size_t kPolyLdsBudget = 48 * 1024; // poly kernel: LDS line target (three workgroups per CU)

template <typename R> struct rvec;
template <> struct rvec<float> {
    typedef float type __attribute__((ext_vector_type(4)));
    static constexpr int lanes = 4;
    static constexpr int pad = 4; // elements after every 16-element block: 80-B pitch, as fir.hip
};
template <> struct rvec<double> {
    typedef double type __attribute__((ext_vector_type(2)));
    static constexpr int lanes = 2;
    static constexpr int pad = 2;
};

template <typename R> __device__ __forceinline__ R mul_add(R h, R x, R acc);
template <> __device__ __forceinline__ float mul_add<float>(float h, float x, float acc) { return __builtin_fmaf(h, x, acc); }
template <> __device__ __forceinline__ double mul_add<double>(double h, double x, double acc) { return acc + h * x; }

template <typename R> __device__ __forceinline__ uint32_t slot(uint32_t p) { return p + (p >> 4) * rvec<R>::pad; }

template <typename R> __device__ __forceinline__ void read_block(const R *line, uint32_t blk, R (&dst)[kBlk])
{
    using V = typename rvec<R>::type;
    constexpr int L = rvec<R>::lanes;
    const V *src = reinterpret_cast<const V *>(line + blk * (kBlk + rvec<R>::pad));
#pragma unroll
    for (int i = 0; i < kBlk / L; i++) {
        V v = src[i];
#pragma unroll
        for (int j = 0; j < L; j++)
            dst[i * L + j] = v[j];
    }
}

struct rs_kargs {
    const void *in;
    void *out;
    void *state;
    uint64_t channels, samples, in_stride, out_stride;
    uint32_t taps, up, down, q, hist_len; // hist_len = H = floor((taps - 1) / up)
    uint32_t hist;     // LDS history region in elements (dec: 16 ceil(taps / 16); poly: H rounded up to 4)
    uint32_t blk_in;   // poly: input samples per LDS block (a multiple of lcm(q, 4))
    uint32_t tpr_log2; // dec: threads per row
    uint32_t vec_in, vec_out; // rows 16-byte aligned
};

// ---- U = 1, D | 16 ------------------------------------------------------------------------------------------------------------
// 16 taps h[k0 .. k0+16) applied to the 16 / D outputs at block positions r D.  win[0..16) = the block before, win[16..32) = the
// block the newest of these taps reads.  `count` < 16 only in the last chunk.
template <typename R, int D, bool FIRST, bool PARTIAL>
__device__ __forceinline__ void dec_taps16(const R *__restrict__ h, uint32_t k0, uint32_t count, const R (&win)[2 * kBlk],
                                           R (&acc)[kBlk / D])
{
#pragma unroll
    for (int kk = 0; kk < kBlk; kk++) {
        if (!PARTIAL || static_cast<uint32_t>(kk) < count) { // wave-uniform
            const R hk = h[k0 + kk];
#pragma unroll
            for (int r = 0; r < kBlk / D; r++) {
                if (FIRST && kk == 0)
                    acc[r] = hk * win[kBlk + r * D];
                else
                    acc[r] = mul_add<R>(hk, win[kBlk + r * D - kk], acc[r]);
            }
        }
    }
}

template <typename R, int D>
__device__ __forceinline__ void dec_block(const R *line, uint32_t mine, const R *__restrict__ h, uint32_t taps, R (&acc)[kBlk / D])
{
    const uint32_t nfull = taps / kBlk, rem = taps % kBlk;
    R win[2 * kBlk];
    {
        R cur[kBlk];
        read_block<R>(line, mine, cur);
#pragma unroll
        for (int i = 0; i < kBlk; i++)
            win[kBlk + i] = cur[i];
    }
    uint32_t kc = 0;
    if (nfull) {
        R prev[kBlk];
        read_block<R>(line, mine - 1, prev);
#pragma unroll
        for (int i = 0; i < kBlk; i++)
            win[i] = prev[i];
        dec_taps16<R, D, true, false>(h, 0, kBlk, win, acc);
        for (kc = 1; kc < nfull; kc++) {
#pragma unroll
            for (int i = 0; i < kBlk; i++)
                win[kBlk + i] = win[i];
            read_block<R>(line, mine - kc - 1, prev);
#pragma unroll
            for (int i = 0; i < kBlk; i++)
                win[i] = prev[i];
            dec_taps16<R, D, false, false>(h, kc * kBlk, kBlk, win, acc);
        }
        if (rem) {
#pragma unroll
            for (int i = 0; i < kBlk; i++)
                win[kBlk + i] = win[i];
        }
    }
    if (rem) {
        R prev[kBlk];
        read_block<R>(line, mine - kc - 1, prev);
#pragma unroll
        for (int i = 0; i < kBlk; i++)
            win[i] = prev[i];
        if (nfull)
            dec_taps16<R, D, false, true>(h, kc * kBlk, rem, win, acc);
        else
            dec_taps16<R, D, true, true>(h, 0, rem, win, acc);
    }
}

template <typename R, int D, int TH>
__global__ __launch_bounds__(TH) void sdsp_resample_dec_kernel(rs_kargs a, const R *__restrict__ h)
{
    using V = typename rvec<R>::type;
    constexpr int L = rvec<R>::lanes;
    constexpr int VPT = kBlk / L;
    constexpr int RO = kBlk / D;              // outputs per thread and block
    constexpr int W = RO < L ? RO : L;        // elements per output store
    typedef R VW __attribute__((ext_vector_type(W)));
    extern __shared__ __align__(16) unsigned char lds_raw[];

    const uint32_t tpr = 1u << a.tpr_log2;
    const uint32_t row = threadIdx.x >> a.tpr_log2;
    const uint32_t t = threadIdx.x & (tpr - 1);
    const uint32_t rows_per_wg = (uint32_t)TH >> a.tpr_log2;
    const uint64_t ch = static_cast<uint64_t>(blockIdx.x) * rows_per_wg + row;
    const bool live = ch < a.channels;
    const uint32_t block_len = tpr * kBlk;
    const uint32_t line_elems = slot<R>(a.hist + block_len);
    R *line = reinterpret_cast<R *>(lds_raw) + static_cast<size_t>(row) * line_elems;
    const uint64_t c = live ? ch : 0;
    const R *inp = static_cast<const R *>(a.in) + c * a.in_stride;
    R *outp = static_cast<R *>(a.out) + c * a.out_stride;
    const uint32_t H = a.hist_len;
    R *statep = a.state ? static_cast<R *>(a.state) + c * H : nullptr;

    for (uint32_t j = t; j < a.hist; j += tpr) {
        R v = R(0);
        if (live && statep && j < H)
            v = statep[j];
        line[slot<R>(a.hist - 1 - j)] = v;
    }

    for (uint64_t s0 = 0; s0 < a.samples; s0 += block_len) {
        const uint64_t left = a.samples - s0;
        const uint32_t len = left < block_len ? static_cast<uint32_t>(left) : block_len;
        const bool whole = len == block_len;
        const R *blk = inp + s0;

        if (live) {
            if (whole && a.vec_in) {
                V v[VPT];
#pragma unroll
                for (int i = 0; i < VPT; i++) {
                    const V *src = reinterpret_cast<const V *>(blk) + (i * tpr + t);
                    v[i] = __builtin_nontemporal_load(src);
                }
#pragma unroll
                for (int i = 0; i < VPT; i++)
                    *reinterpret_cast<V *>(line + slot<R>(a.hist + (i * tpr + t) * L)) = v[i];
            } else {
#pragma unroll
                for (int i = 0; i < VPT; i++)
#pragma unroll
                    for (int j = 0; j < L; j++) {
                        const uint32_t e = (i * tpr + t) * L + j;
                        line[slot<R>(a.hist + e)] = e < len ? blk[e] : R(0);
                    }
            }
        }
        __syncthreads();

        R acc[RO];
        dec_block<R, D>(line, (a.hist >> 4) + t, h, a.taps, acc);
        __syncthreads();

        const bool last = s0 + block_len >= a.samples;
        if (last) {
            if (live && statep)
                for (uint32_t j = t; j < H; j += tpr)
                    statep[j] = line[slot<R>(a.hist + len - 1 - j)];
        } else {
            for (uint32_t j = t; j < a.hist; j += tpr)
                line[slot<R>(j)] = line[slot<R>(block_len + j)];
        }

        // the thread's outputs are consecutive: block positions 16 t + r D, output index (s0 + 16 t) / D + r
        if (live) {
            R *dst = outp + s0 / D + static_cast<uint64_t>(t) * RO;
            if (whole && a.vec_out) {
#pragma unroll
                for (int i = 0; i < RO / W; i++) {
                    VW v;
#pragma unroll
                    for (int j = 0; j < W; j++)
                        v[j] = acc[i * W + j];
                    __builtin_nontemporal_store(v, reinterpret_cast<VW *>(dst) + i);
                }
            } else {
#pragma unroll
                for (int r = 0; r < RO; r++)
                    if (t * kBlk + r * D < len)
                        dst[r] = acc[r];
            }
        }
        __syncthreads(); // the next block's LDS writes
    }
}

// ---- any (U, D) ---------------------------------------------------------------------------------------------------------------
template <typename R>
__global__ __launch_bounds__(kPolyThreads) void sdsp_resample_poly_kernel(rs_kargs a, const R *__restrict__ h)
{
    using V = typename rvec<R>::type;
    constexpr int L = rvec<R>::lanes;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    R *line = reinterpret_cast<R *>(lds_raw); // [hist | blk_in]

    const uint64_t c = blockIdx.x;
    const uint32_t t = threadIdx.x;
    const R *inp = static_cast<const R *>(a.in) + c * a.in_stride;
    R *outp = static_cast<R *>(a.out) + c * a.out_stride;
    const uint32_t H = a.hist_len;
    R *statep = a.state ? static_cast<R *>(a.state) + c * H : nullptr;
    const uint32_t U = a.up, D = a.down, q = a.q;
    const uint32_t uq = U / (D / q); // outputs per period (U / g); a period is q inputs

    for (uint32_t j = t; j < a.hist; j += kPolyThreads)
        line[a.hist - 1 - j] = (statep && j < H) ? statep[j] : R(0);

    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t lane = t & 63;
    R *blkl = line + a.hist;
    for (uint64_t s0 = 0; s0 < a.samples; s0 += a.blk_in) {
        const uint64_t left = a.samples - s0;
        const uint32_t len = left < a.blk_in ? static_cast<uint32_t>(left) : a.blk_in;
        const R *blk = inp + s0;
        if (len == a.blk_in && a.vec_in) {
            for (uint32_t i = t; i < len / L; i += kPolyThreads) {
                const V *src = reinterpret_cast<const V *>(blk) + i;
                *reinterpret_cast<V *>(blkl + i * L) = __builtin_nontemporal_load(src);
            }
        } else {
            for (uint32_t e = t; e < len; e += kPolyThreads)
                blkl[e] = blk[e];
        }
        __syncthreads();

        // task = (phase slot r of the period, chunk of 64 kAcc periods); r is wave-uniform, so p and h[p + j U] are too.  Lane l
        // keeps kAcc independent chains, periods i0 + 64 a, that share every coefficient load
        const uint32_t periods = len / q;
        const uint32_t chunks = (periods + 64 * kAcc - 1) / (64 * kAcc);
        const uint64_t o0 = s0 / q * uq; // first output of the block
        for (uint32_t task = wave; task < uq * chunks; task += kPolyThreads / 64) {
            const uint32_t r = task / chunks, ck = task - r * chunks;
            const uint32_t i0 = ck * 64 * kAcc + lane;
            const uint32_t n = r * D;
            const uint32_t p = n % U;
            const uint32_t tp = p < a.taps ? (a.taps - 1 - p) / U + 1 : 0;
            const R *x[kAcc];
#pragma unroll
            for (int k = 0; k < kAcc; k++) {
                const uint32_t i = i0 + 64 * k < periods ? i0 + 64 * k : periods - 1; // lanes past the block read a valid period
                x[k] = blkl + (n / U + i * q);                                       // x[b - j] = x[k][-j]
            }
            R acc[kAcc];
#pragma unroll
            for (int k = 0; k < kAcc; k++)
                acc[k] = R(0);
            if (tp) {
                const R h0 = h[p];
#pragma unroll
                for (int k = 0; k < kAcc; k++)
                    acc[k] = h0 * x[k][0];
                for (uint32_t j = 1; j < tp; j++) {
                    const R hj = h[p + j * U];
#pragma unroll
                    for (int k = 0; k < kAcc; k++)
                        acc[k] = mul_add<R>(hj, *(x[k] - static_cast<int32_t>(j)), acc[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < kAcc; k++)
                if (i0 + 64 * k < periods)
                    __builtin_nontemporal_store(acc[k], outp + o0 + r + static_cast<uint64_t>(i0 + 64 * k) * uq);
        }
        __syncthreads();

        const bool last = s0 + a.blk_in >= a.samples;
        if (last) {
            if (statep)
                for (uint32_t j = t; j < H; j += kPolyThreads)
                    statep[j] = blkl[static_cast<int32_t>(len) - 1 - static_cast<int32_t>(j)];
        } else {
            for (uint32_t j = t; j < a.hist; j += kPolyThreads) // blk_in >= hist: no overlap
                line[j] = line[a.blk_in + j];
        }
        __syncthreads();
    }
}

// ---- variant 1: one output per thread from global memory ----------------------------------------------------------------------
template <typename R>
__global__ __launch_bounds__(256) void sdsp_resample_plain_kernel(rs_kargs a, const R *__restrict__ h, uint64_t outs)
{
    const uint64_t total = a.channels * outs;
    const uint32_t H = a.hist_len;
    for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total;
         idx += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t c = idx / outs, m = idx - c * outs;
        const uint64_t n = m * a.down;
        const uint32_t p = static_cast<uint32_t>(n % a.up);
        const int64_t b = static_cast<int64_t>(n / a.up);
        const R *inp = static_cast<const R *>(a.in) + c * a.in_stride;
        const R *st = a.state ? static_cast<const R *>(a.state) + c * H : nullptr;
        R acc = R(0);
        for (uint32_t k = p, j = 0; k < a.taps; k += a.up, j++) {
            const int64_t xi = b - static_cast<int64_t>(j);
            const R x = xi >= 0 ? inp[xi] : (st ? st[-1 - xi] : R(0)); // -1 - xi < H: k <= taps - 1
            acc = j == 0 ? h[k] * x : mul_add<R>(h[k], x, acc);
        }
        static_cast<R *>(a.out)[c * a.out_stride + m] = acc;
    }
}

// new history, one thread per channel, newest first; descending j reads only entries not yet overwritten
template <typename R> __global__ __launch_bounds__(256) void sdsp_resample_state_kernel(rs_kargs a)
{
    const uint64_t c = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c >= a.channels)
        return;
    const uint32_t H = a.hist_len;
    const R *inp = static_cast<const R *>(a.in) + c * a.in_stride;
    R *st = static_cast<R *>(a.state) + c * H;
    for (uint32_t j = H; j-- > 0;)
        st[j] = j < a.samples ? inp[a.samples - 1 - j] : st[j - a.samples];
}

uint32_t gcd_u32(uint32_t a, uint32_t b)
{
    while (b) {
        const uint32_t r = a % b;
        a = b;
        b = r;
    }
    return a;
}

bool dec_supported(uint32_t up, uint32_t down) { return up == 1 && down <= kBlk && (kBlk % down) == 0; }

enum { RS_PLAIN, RS_DEC, RS_POLY };
struct rs_launch {
    int kind;
    const char *name;
    uint32_t threads, tpr_log2, hist, blk_in;
    size_t lds;
    uint64_t grid;
};

// the one selection rule: launch_resample and resample_kernel_for both call it
rs_launch select_resample(int precision, const resample_args &ra, int variant)
{
    const size_t rs = precision == SDSP_HIP_F64 ? 8 : 4;
    rs_launch l{};
    const uint32_t q = ra.down / gcd_u32(ra.up, ra.down);
    const uint32_t H = (ra.taps - 1) / ra.up;
    if (variant == 1) {
        l.kind = RS_PLAIN;
        l.name = "sdsp_resample_plain_kernel";
        l.threads = 256;
        return l;
    }
    if (variant == 0 && dec_supported(ra.up, ra.down)) {
        l.kind = RS_DEC;
        l.name = "sdsp_resample_dec_kernel";
        l.hist = kBlk * ((ra.taps + kBlk - 1) / kBlk);
        // threads per row as launch_fir: enough for the row, never fewer than the history needs; 128-thread workgroups
        uint32_t lg = log2u((ra.samples + kBlk - 1) / kBlk);
        const uint32_t lmin = log2u(l.hist / kBlk);
        if (lg < lmin)
            lg = lmin;
        l.threads = lmin <= 7 ? 128 : 256;
        const uint32_t lmax = l.threads == 128 ? 7 : 8;
        if (lg > lmax)
            lg = lmax;
        l.tpr_log2 = lg;
        const uint32_t elems = l.hist + (kBlk << lg);
        const uint32_t pad = precision == SDSP_HIP_F64 ? rvec<double>::pad : rvec<float>::pad;
        l.lds = (elems + (elems >> 4) * pad) * (l.threads >> lg) * rs;
        const uint32_t rows = l.threads >> lg;
        l.grid = (ra.channels + rows - 1) / rows;
        return l;
    }
    l.kind = RS_POLY;
    l.name = "sdsp_resample_poly_kernel";
    l.threads = kPolyThreads;
    l.hist = (H + 3) & ~3u;
    const uint32_t unit = q % 4 == 0 ? q : (q % 2 == 0 ? 2 * q : 4 * q); // lcm(q, 4)
    // enough periods for every chain of a wave (64 kAcc), within the LDS budget, never fewer samples than the history
    const uint32_t fit = static_cast<uint32_t>(kPolyLdsBudget / rs) > l.hist ? static_cast<uint32_t>(kPolyLdsBudget / rs) - l.hist : 0;
    uint64_t want = 64ull * kAcc * q;
    if (want < 2048)
        want = 2048;
    if (want > fit)
        want = fit / unit * unit;
    if (want < l.hist)
        want = l.hist;
    if (want < unit)
        want = unit;
    l.blk_in = static_cast<uint32_t>(unit * ((want + unit - 1) / unit));
    l.lds = static_cast<size_t>(l.hist + l.blk_in) * rs;
    l.grid = ra.channels;
    return l;
}
} // namespace

const char *resample_kernel_for(int precision, const resample_args &a, int variant) { return select_resample(precision, a, variant).name; }

int launch_resample(int precision, const resample_args &ra, int variant, void *stream_v)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const size_t rs = precision == SDSP_HIP_F64 ? 8 : 4;
    const rs_launch l = select_resample(precision, ra, variant);
    rs_kargs k{};
    k.in = ra.in;
    k.out = ra.out;
    k.state = ra.state;
    k.channels = ra.channels;
    k.samples = ra.samples;
    k.in_stride = ra.in_stride;
    k.out_stride = ra.out_stride;
    k.taps = ra.taps;
    k.up = ra.up;
    k.down = ra.down;
    k.q = ra.down / gcd_u32(ra.up, ra.down);
    k.hist_len = (ra.taps - 1) / ra.up;
    if (k.hist_len == 0)
        k.state = nullptr;
    k.hist = l.hist;
    k.blk_in = l.blk_in;
    k.tpr_log2 = l.tpr_log2;
    k.vec_in = (reinterpret_cast<uintptr_t>(ra.in) % 16 == 0 && (ra.in_stride * rs) % 16 == 0) ? 1 : 0;
    k.vec_out = (reinterpret_cast<uintptr_t>(ra.out) % 16 == 0 && (ra.out_stride * rs) % 16 == 0) ? 1 : 0;
    auto check = [](const char *what) -> int {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return fail(SDSP_HIP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
        return SDSP_HIP_OK;
    };
    if (l.kind == RS_PLAIN) {
        const uint64_t outs = ra.samples / k.q * (ra.up / (ra.down / k.q));
        const uint64_t total = ra.channels * outs;
        uint64_t grid = (total + 255) / 256;
        if (grid > 65536)
            grid = 65536; // grid-stride
        if (precision == SDSP_HIP_F64)
            hipLaunchKernelGGL(sdsp_resample_plain_kernel<double>, dim3(static_cast<uint32_t>(grid)), dim3(256), 0, stream, k,
                               static_cast<const double *>(ra.h), outs);
        else
            hipLaunchKernelGGL(sdsp_resample_plain_kernel<float>, dim3(static_cast<uint32_t>(grid)), dim3(256), 0, stream, k,
                               static_cast<const float *>(ra.h), outs);
        if (int rc = check("resample plain launch"))
            return rc;
        if (!k.state)
            return SDSP_HIP_OK;
        const uint32_t sgrid = static_cast<uint32_t>((ra.channels + 255) / 256);
        if (precision == SDSP_HIP_F64)
            hipLaunchKernelGGL(sdsp_resample_state_kernel<double>, dim3(sgrid), dim3(256), 0, stream, k);
        else
            hipLaunchKernelGGL(sdsp_resample_state_kernel<float>, dim3(sgrid), dim3(256), 0, stream, k);
        return check("resample state launch");
    }
    if (l.grid > 0x7fffffffull)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many channels for one launch");
    auto run = [&](auto kernel, auto hp) -> int {
        if (l.lds > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               static_cast<int>(l.lds));
            if (e != hipSuccess)
                return fail(SDSP_HIP_ERR_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e));
        }
        hipLaunchKernelGGL(kernel, dim3(static_cast<uint32_t>(l.grid)), dim3(l.threads), l.lds, stream, k, hp);
        return check("resample launch");
    };
    if (l.kind == RS_POLY) {
        if (precision == SDSP_HIP_F64)
            return run(sdsp_resample_poly_kernel<double>, static_cast<const double *>(ra.h));
        return run(sdsp_resample_poly_kernel<float>, static_cast<const float *>(ra.h));
    }
    auto dec = [&](auto hp) -> int {
        using R = std::remove_const_t<std::remove_pointer_t<decltype(hp)>>;
        const bool wide = l.threads == 256;
        switch (ra.down) {
        case 1: return wide ? run(sdsp_resample_dec_kernel<R, 1, 256>, hp) : run(sdsp_resample_dec_kernel<R, 1, 128>, hp);
        case 2: return wide ? run(sdsp_resample_dec_kernel<R, 2, 256>, hp) : run(sdsp_resample_dec_kernel<R, 2, 128>, hp);
        case 4: return wide ? run(sdsp_resample_dec_kernel<R, 4, 256>, hp) : run(sdsp_resample_dec_kernel<R, 4, 128>, hp);
        case 8: return wide ? run(sdsp_resample_dec_kernel<R, 8, 256>, hp) : run(sdsp_resample_dec_kernel<R, 8, 128>, hp);
        default: return wide ? run(sdsp_resample_dec_kernel<R, 16, 256>, hp) : run(sdsp_resample_dec_kernel<R, 16, 128>, hp);
        }
    };
    if (precision == SDSP_HIP_F64)
        return dec(static_cast<const double *>(ra.h));
    return dec(static_cast<const float *>(ra.h));
}
} // namespace sdsp_hip
