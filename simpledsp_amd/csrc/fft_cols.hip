// fft_cols.hip -- batched complex FFT along the STRIDED axis of row-major cubes [cube][n rows][width columns] for gfx950
// (DESIGN.md section 5.30): every column of every cube is one transform of n = 8 .. 1024 points whose elements lie `width` elements
// apart.  One read and one write of the cube; no transpose and no workspace.
//
// Variant 0, sdsp_fft_cols_kernel.  Its form depends on n and the precision only, never on width, batch or the column's position:
//
//   n <= 32        one lane per column.  A wave reads 64 adjacent columns row by row (one element per lane: 512 contiguous bytes per
//                  instruction in f32), a lane holds its whole column in registers, runs log2 n radix-2 DIF stages with compile-time
//                  twiddles (fft32.h's W_32 constants) and stores row by row.  No LDS, no barrier.
//   n = 64 .. 1024 the tile scheme of fft_2pass.hip's cols_tile2p: a tile is 16 adjacent columns (128-byte row segments in f32, 256 in
//                  f64), T = n / 32 threads per column hold 32 points each.  Five DIF stages across the thread's points (row stride T,
//                  thread twiddles W_n^(u << s) from the plan's table), ONE exchange through an XOR-swizzled LDS plane (real plane, then
//                  imaginary) after which a thread holds 32 consecutive points, then the remaining log2 T stages on 32 / T groups of T
//                  points with constants only.  The result leaves in natural order: register k of thread u holds X[bit_reverse(32 u + k)].
//                  Where a tile has fewer than 64 threads (n = 64) two tiles run side by side in one workgroup.
//
// Fusions: the window multiplies at the load (forward plans), the shift is a row offset at the store (forward) or the load (reverse),
// POWER squares at the store, reverse plans scale by 1 / n at the store.  A lane moves one element per instruction, so an element-aligned
// pointer and an odd width need no other path.  The ragged last tile of a row runs the same code: an out-of-range column loads zeros and
// stores nothing, which leaves the arithmetic of the real columns as it is.  Every load of a tile precedes its first store (the barrier
// of the exchange; program order in the short form), and a tile writes the columns it read, so out == in is allowed.
//
// Variant 1, sdsp_fft_cols_plain_kernel: the cross-check.  One thread per (column, output row): the plain sum X[k] = sum_p v[p] W^(p k)
// from global memory, accumulated in double for both precisions.  It shares no staging or butterfly code with variant 0.
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "fft32.h"
#include "sdsp_hip_internal.h"
#include "stream_dev.h"

namespace sdsp_hip
{
namespace
{
using namespace fft32;

constexpr int kShortMax = 32;    // the largest n of the lane-per-column form
constexpr int kShortColumns = 64; // columns of its tile: one wave
constexpr int kTile = 16;        // columns of a tile of the LDS form

template <typename C> struct cols_kargs {
    using Real = typename w32<C>::real;
    const C *in;     // the launch's first cube
    void *out;       // C (COMPLEX) or Real (POWER) elements, the same [cube][row][column] layout
    const C *tw;     // W_n^j, j < n, direction-folded, plan precision
    const Real *win; // n values of the plan precision, or null
    uint64_t width;
    uint32_t tiles;  // workgroups per cube
    uint32_t shift;  // 0 or n / 2
    Real scale;      // reverse: 1 / n
};

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v / 2); }

template <int BITS> __device__ __forceinline__ uint32_t brev_bits(uint32_t v) { return BITS == 0 ? 0u : (__brev(v) >> (32 - BITS)); }

// log2 N radix-2 DIF stages on N = 8, 16 or 32 registers with compile-time twiddles: fft32_dif's butterflies (fft32.h) for a whole
// transform of N points.  Stage s pairs (k, k + h), h = N / 2 >> s; the lower output owes W_N^((k mod h) << s) = W_32^(that * 32 / N).
// x[k] leaves holding X[bit_reverse(k)].
template <int N, bool REV, typename C> __device__ __forceinline__ void dif_regs(C (&x)[N])
{
    using R = typename w32<C>::real;
#pragma unroll
    for (int s = 0; s < ilog2(N); s++) {
        const int h = (N / 2) >> s;
#pragma unroll
        for (int k = 0; k < N; k++) {
            if ((k & h) != 0)
                continue;
            const C a = x[k], b = x[k + h];
            x[k] = a + b;
            C d = a - b;
            const int e = ((k & (h - 1)) << s) * (32 / N); // W_32 exponent, 0..15
            if (e == 8) {
                d = REV ? C{ -d.y, d.x } : C{ d.y, -d.x };
            } else if (e != 0) {
                const R cr = w32<C>::c(e), ci = REV ? w32<C>::s(e) : -w32<C>::s(e);
                d = C{ d.x * cr - d.y * ci, d.x * ci + d.y * cr };
            }
            x[k + h] = d;
        }
    }
}

// one output element: X of row `row`, column already folded into dst
template <bool REV, bool POWER, typename C>
__device__ __forceinline__ void put(void *out, size_t idx, C v, typename w32<C>::real scale)
{
    using R = typename w32<C>::real;
    if constexpr (REV)
        v = C{ v.x * scale, v.y * scale };
    if constexpr (POWER)
        static_cast<R *>(out)[idx] = v.x * v.x + v.y * v.y;
    else
        nt_store(static_cast<C *>(out) + idx, v);
}

template <int N> struct cols_shape {
    static constexpr bool SHORT = N <= kShortMax;
    static constexpr int T = SHORT ? 1 : N / 32;                    // threads per column
    static constexpr int TT = SHORT ? kShortColumns : kTile * T;    // threads per tile
    static constexpr int G = TT >= 64 ? 1 : 64 / TT;                // tiles side by side in one workgroup
    static constexpr int THREADS = TT * G;
    static constexpr int COLUMNS = SHORT ? kShortColumns : kTile * G; // columns per workgroup
    static constexpr int TILE_COLUMNS = SHORT ? kShortColumns : kTile;
    template <typename Real> static constexpr size_t lds() { return SHORT ? 0 : (size_t)N * kTile * G * sizeof(Real); }
};

// f(std::integral_constant<int, n>) for the n a plan can have
template <typename F> int for_n(uint32_t n, F &&f)
{
    switch (n) {
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
    case 128: return f(std::integral_constant<int, 128>{});
    case 256: return f(std::integral_constant<int, 256>{});
    case 512: return f(std::integral_constant<int, 512>{});
    case 1024: return f(std::integral_constant<int, 1024>{});
    }
    return fail(SDSP_HIP_ERR_INVALID_SIZE, "fft_cols: n must be a power of two in [8, 1024]");
}

template <int N, typename C, bool REV, bool POWER>
__global__ __launch_bounds__(cols_shape<N>::THREADS) void sdsp_fft_cols_kernel(cols_kargs<C> a)
{
    using Real = typename w32<C>::real;
    using S = cols_shape<N>;
    constexpr int L = ilog2(N);
    const uint32_t cube = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const size_t cube0 = (size_t)cube * N * a.width;

    if constexpr (S::SHORT) {
        const uint64_t col = (uint64_t)tile * kShortColumns + threadIdx.x;
        const bool live = col < a.width;
        const C *src = a.in + cube0 + col;
        C x[N];
        if (live) {
#pragma unroll
            for (int p = 0; p < N; p++) {
                const uint32_t row = REV ? ((uint32_t)p + a.shift) & (N - 1) : (uint32_t)p;
                x[p] = nt_load(src + (size_t)row * a.width);
            }
        } else {
#pragma unroll
            for (int p = 0; p < N; p++)
                x[p] = C{ Real(0), Real(0) };
        }
        if (a.win) {
#pragma unroll
            for (int p = 0; p < N; p++) {
                const Real w = a.win[p];
                x[p] = C{ x[p].x * w, x[p].y * w };
            }
        }
        dif_regs<N, REV>(x);
        if (live) {
#pragma unroll
            for (int k = 0; k < N; k++) {
                const uint32_t kk = brev_bits<L>((uint32_t)k);
                const uint32_t row = REV ? kk : (kk + a.shift) & (N - 1);
                put<REV, POWER>(a.out, cube0 + (size_t)row * a.width + col, x[k], a.scale);
            }
        }
    } else {
        constexpr int T = S::T, TT = S::TT;
        extern __shared__ __attribute__((aligned(16))) unsigned char sdsp_fft_cols_smem[];
        const uint32_t g = threadIdx.x / TT, tt = threadIdx.x % TT;
        const uint32_t c = tt & 15, u = tt >> 4; // u < T
        Real *plane = reinterpret_cast<Real *>(sdsp_fft_cols_smem) + (size_t)g * N * kTile;
        const uint64_t col = (uint64_t)tile * S::COLUMNS + g * kTile + c;
        const bool live = col < a.width;
        const C *src = a.in + cube0 + col;

        // rows u + T k of the column
        C x[32];
        if (live) {
#pragma unroll
            for (int k = 0; k < 32; k++) {
                const uint32_t p = u + T * k;
                const uint32_t row = REV ? (p + a.shift) & (N - 1) : p;
                x[k] = nt_load(src + (size_t)row * a.width);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 32; k++)
                x[k] = C{ Real(0), Real(0) };
        }
        if (a.win) {
#pragma unroll
            for (int k = 0; k < 32; k++) {
                const Real w = a.win[u + T * k];
                x[k] = C{ x[k].x * w, x[k].y * w };
            }
        }
        fft32_dif<REV, true, 0, false, false, C>(x, a.tw, u); // W_n^(u << s)

        // exchange rows {u + T k} -> {32 u + k}; slot(row, col) = (row * 16 + col) ^ (((row >> 5) & 1) << 4), as cols_tile2p
        {
            Real *const w0 = plane + (u * 16 + c);
            Real *const w1 = plane + ((u * 16 + c) ^ 16);
            const int flip = (int)(u & 1) * 16;
            const Real *const r_even = plane + (512 * u + c) + flip;
            const Real *const r_odd = plane + (512 * u + c) - flip;
#pragma unroll
            for (int half = 0; half < 2; half++) {
#pragma unroll
                for (int k = 0; k < 32; k++) // row u + T k: bit 5 of the row = that bit of T k (no carry from u < T, T >= 2)
                    ((((k * T) >> 5) & 1) ? w1 : w0)[16 * T * k] = half ? x[k].y : x[k].x;
                __syncthreads();
#pragma unroll
                for (int k = 0; k < 32; k++) {
                    const Real f = ((k & 1) ? r_odd : r_even)[16 * k];
                    if (half)
                        x[k].y = f;
                    else
                        x[k].x = f;
                }
                if (half == 0)
                    __syncthreads();
            }
        }
        fft32_dif<REV, false, 10 - L, false, false, C>(x, a.tw, 0); // the last log2 T stages on 32 / T groups of T consecutive rows

        // row 32 u + k holds X[kk], kk = bit_reverse_L(32 u + k) = (bit_reverse5(k) << (L - 5)) | bit_reverse(u)
        if (live) {
            const uint32_t bu = brev_bits<L - 5>(u);
#pragma unroll
            for (int k = 0; k < 32; k++) {
                const uint32_t kk = ((__brev((uint32_t)k) >> 27) << (L - 5)) | bu;
                const uint32_t row = REV ? kk : (kk + a.shift) & (N - 1);
                put<REV, POWER>(a.out, cube0 + (size_t)row * a.width + col, x[k], a.scale);
            }
        }
    }
}

// ---- variant 1: the plain sum ----------------------------------------------------------------------------------------
// workgroup = cpb adjacent columns x all n output rows (cpb = blockDim.x / n); a thread sums its output in double, and the barrier
// between the sums and the stores is what lets out == in
template <typename C, bool REV, bool POWER> __global__ void sdsp_fft_cols_plain_kernel(cols_kargs<C> a, uint32_t n)
{
    using Real = typename w32<C>::real;
    const uint32_t cpb = blockDim.x / n;
    const uint32_t c = threadIdx.x % cpb, k = threadIdx.x / cpb;
    const uint32_t cube = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const uint64_t col = (uint64_t)tile * cpb + c;
    const size_t cube0 = (size_t)cube * n * a.width;
    double sr = 0.0, si = 0.0;
    if (col < a.width) {
        for (uint32_t p = 0; p < n; p++) {
            const uint32_t row = REV ? (p + a.shift) & (n - 1) : p;
            C v = a.in[cube0 + (size_t)row * a.width + col];
            if (a.win) {
                const Real w = a.win[p];
                v = C{ v.x * w, v.y * w };
            }
            const C t = a.tw[(p * k) & (n - 1)];
            const double vr = v.x, vi = v.y, tr = t.x, ti = t.y;
            sr += vr * tr - vi * ti;
            si += vr * ti + vi * tr;
        }
    }
    __syncthreads();
    if (col < a.width) {
        const uint32_t row = REV ? k : (k + a.shift) & (n - 1);
        const size_t idx = cube0 + (size_t)row * a.width + col;
        Real re = (Real)sr, im = (Real)si;
        if constexpr (REV) {
            re *= a.scale;
            im *= a.scale;
        }
        if constexpr (POWER)
            static_cast<Real *>(a.out)[idx] = re * re + im * im;
        else
            static_cast<C *>(a.out)[idx] = C{ re, im };
    }
}

constexpr uint32_t kPlainThreads = 256;
uint32_t plain_threads(uint32_t n) { return n >= kPlainThreads ? n : kPlainThreads; }

// ---- host side ------------------------------------------------------------------------------------------------------------
constexpr uint64_t kMaxGrid = 0x7fffffffull;

template <int N, typename C, bool REV, bool POWER> int launch_n(const fft_cols_args &a, hipStream_t stream)
{
    using Real = typename w32<C>::real;
    using S = cols_shape<N>;
    auto kern = sdsp_fft_cols_kernel<N, C, REV, POWER>;
    constexpr size_t lds = S::template lds<Real>();
    if constexpr (lds > 32768) {
        static std::atomic<uint64_t> lds_done{ 0 };
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), lds, lds_done))
            return rc;
    }
    if (!a.in) // plan creation: the attribute only
        return SDSP_HIP_OK;
    cols_kargs<C> k{};
    k.tw = static_cast<const C *>(a.tw);
    k.win = static_cast<const Real *>(a.window);
    k.width = a.width;
    const uint64_t tiles = (a.width + S::COLUMNS - 1) / S::COLUMNS;
    if (tiles > kMaxGrid)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "fft_cols: one cube is too wide for one launch");
    k.tiles = static_cast<uint32_t>(tiles);
    k.shift = a.shift ? N / 2 : 0;
    k.scale = Real(1) / Real(N);
    const uint64_t per_launch = std::max<uint64_t>(1, kMaxGrid / k.tiles);
    const size_t cube_in = (size_t)N * a.width, out_es = POWER ? sizeof(Real) : sizeof(C);
    for (uint64_t b0 = 0; b0 < a.batch; b0 += per_launch) {
        const uint64_t cubes = std::min(per_launch, a.batch - b0);
        k.in = static_cast<const C *>(a.in) + b0 * cube_in;
        k.out = static_cast<char *>(a.out) + b0 * cube_in * out_es;
        hipLaunchKernelGGL(kern, dim3(static_cast<uint32_t>(cubes * k.tiles)), dim3(S::THREADS), lds, stream, k);
    }
    return launch_status("fft_cols");
}

template <typename C, bool REV, bool POWER> int launch_form(const fft_cols_args &a, hipStream_t stream)
{
    return for_n(a.n, [&](auto n) { return launch_n<decltype(n)::value, C, REV, POWER>(a, stream); });
}

template <typename C, bool REV, bool POWER> int launch_plain(const fft_cols_args &a, hipStream_t stream)
{
    using Real = typename w32<C>::real;
    if (!a.in)
        return SDSP_HIP_OK;
    const uint32_t threads = plain_threads(a.n), cpb = threads / a.n;
    cols_kargs<C> k{};
    k.tw = static_cast<const C *>(a.tw);
    k.win = static_cast<const Real *>(a.window);
    k.width = a.width;
    const uint64_t tiles = (a.width + cpb - 1) / cpb;
    if (tiles > kMaxGrid)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "fft_cols: one cube is too wide for one launch");
    k.tiles = static_cast<uint32_t>(tiles);
    k.shift = a.shift ? a.n / 2 : 0;
    k.scale = Real(1) / Real(a.n);
    const uint64_t per_launch = std::max<uint64_t>(1, kMaxGrid / k.tiles);
    const size_t cube_in = (size_t)a.n * a.width, out_es = POWER ? sizeof(Real) : sizeof(C);
    for (uint64_t b0 = 0; b0 < a.batch; b0 += per_launch) {
        const uint64_t cubes = std::min(per_launch, a.batch - b0);
        k.in = static_cast<const C *>(a.in) + b0 * cube_in;
        k.out = static_cast<char *>(a.out) + b0 * cube_in * out_es;
        hipLaunchKernelGGL((sdsp_fft_cols_plain_kernel<C, REV, POWER>), dim3(static_cast<uint32_t>(cubes * k.tiles)), dim3(threads), 0,
                           stream, k, a.n);
    }
    return launch_status("fft_cols");
}

template <typename C> int launch_c(const fft_cols_args &a, int variant, hipStream_t stream)
{
    if (a.reverse)
        return variant ? launch_plain<C, true, false>(a, stream) : launch_form<C, true, false>(a, stream);
    if (a.power)
        return variant ? launch_plain<C, false, true>(a, stream) : launch_form<C, false, true>(a, stream);
    return variant ? launch_plain<C, false, false>(a, stream) : launch_form<C, false, false>(a, stream);
}
} // namespace

// with a.in == nullptr: raises the kernel's dynamic-LDS limit where it needs that and launches nothing (plan creation, so that a
// captured exec sets no attribute)
int launch_fft_cols(int precision, const fft_cols_args &a, int variant, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    return precision == SDSP_HIP_F64 ? launch_c<double2>(a, variant, s) : launch_c<float2>(a, variant, s);
}

fft_cols_shape fft_cols_shape_for(int precision, uint32_t n, int variant)
{
    fft_cols_shape s{};
    if (variant) {
        s.threads = plain_threads(n);
        s.tile_columns = s.columns = s.threads / n;
        return s;
    }
    (void)for_n(n, [&](auto nc) {
        using S = cols_shape<decltype(nc)::value>;
        s.tile_columns = S::TILE_COLUMNS;
        s.columns = S::COLUMNS;
        s.threads = S::THREADS;
        s.lds_bytes = static_cast<uint32_t>(precision == SDSP_HIP_F64 ? S::template lds<double>() : S::template lds<float>());
        return static_cast<int>(SDSP_HIP_OK);
    });
    return s;
}

uint64_t fft_cols_launches(int precision, uint32_t n, uint64_t width, uint64_t batch, int variant)
{
    if (batch == 0)
        return 0;
    const uint64_t columns = fft_cols_shape_for(precision, n, variant).columns;
    const uint64_t tiles = (width + columns - 1) / columns;
    const uint64_t per_launch = std::max<uint64_t>(1, kMaxGrid / tiles);
    return (batch + per_launch - 1) / per_launch;
}

const char *fft_cols_kernel_for(int variant) { return variant ? "sdsp_fft_cols_plain_kernel" : "sdsp_fft_cols_kernel"; }
} // namespace sdsp_hip
