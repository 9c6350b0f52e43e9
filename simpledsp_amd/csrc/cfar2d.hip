// cfar2d.hip -- two-dimensional cell-averaging CFAR over compact range-Doppler maps [map][D][R] for MI355X (gfx950), with an ordered
// hit list per map.  DESIGN.md section 5.32; the contract is the comment in front of sdsp_hip_cfar2d_plan_create (sdsp_hip.h).
//
// With Hd = Ld + Gd, Hr = Lr + Gr: per row  lag, mid, lead  are the sums of p over the columns r - Hr .. r - Gr - 1, r - Gr .. r + Gr and
// r + Gr + 1 .. r + Hr (columns outside the map count +0), side = lag + lead, full = (lag + mid) + lead; down the rows (Doppler wraps)
// top and bottom sum `full` over the Ld rows on either side, band sums `side` over the 2 Gd + 1 rows in the middle, and
// T = (top + band) + bottom.  Every sum starts at +0 and runs in ascending index.  thr = T c(r), det = p > thr, optionally the 3 x 3 peak
// rule.  Built with -ffp-contract=off: never an FMA.
//
// Kernels:
//   sdsp_cfar2d_kernel         variant 0.  A workgroup owns a strip of kCols columns and a block of TR rows (TR / 8 waves).  It stages
//                              the TR + 2 Hd wrapped rows x kCols + 2 Hr columns through LDS in chunks of rows; per chunk every thread
//                              forms lag, mid and lead of eight consecutive columns of one row from register windows (every staged power
//                              is read once for up to eight additions) and leaves side and full in LDS.  Then wave w takes rows 8 w .. 8 w + 7
//                              of the block, lane l column l, and runs the same windows down the column.  The peak rule reads its eight
//                              neighbours from global memory, for the cells above their threshold only.  With a hit list the wave leaves
//                              the ballot of each (row, strip) segment and its count in the workspace.
//   sdsp_cfar2d_scan_kernel    one workgroup per map: the exclusive prefix of the segment counts in (d, strip) order, and counts[m].
//   sdsp_cfar2d_place_kernel   a wave per 64 segments; for each segment with a hit, lane l places column l at the segment's offset plus
//                              the number of set bits below l.  The record's threshold is computed again, by direct_cell.
//   sdsp_cfar2d_plain_kernel   variant 1: one thread per cell from global memory, plain loops in the contract's order (direct_cell).
//   sdsp_cfar2d_plain_piece_kernel / sdsp_cfar2d_plain_scan_kernel   its list: one thread per piece of 64 columns of a row counts, one
//                              thread per map scans, one thread per piece places.  No staging, no wave operations.
// No workgroup waits on another and nothing on the ordering path is atomic.
#include "stream_dev.h"

#include <algorithm>

namespace sdsp_hip
{
namespace
{
constexpr uint32_t kCols = 64;             // columns of a strip: one per lane
constexpr uint32_t kWin = 8;               // consecutive sums per thread
constexpr uint32_t kPitchS = kCols + 1;    // elements between two rows of side / full
constexpr uint32_t kMaxLds = 160 * 1024;   // of one CU
constexpr uint32_t kLdsGoal = 64 * 1024;   // two workgroups per CU
constexpr uint32_t kChunkBytes = 24 * 1024; // staged powers of one chunk of rows
constexpr uint64_t kMaxGrid = 0x7fffffffull;

struct c2_kargs {
    const void *p;
    void *thr;          // nullable
    uint8_t *det;       // nullable
    void *hits;         // nullable
    uint32_t *counts;   // with hits
    const void *scale;  // R values c(r) of the precision
    uint64_t *mask;     // workspace: the ballot of every (map, d, strip) segment; null without a list
    uint32_t *cnt;      // workspace: its count, after the scan its offset
    uint64_t maps, cap;
    uint32_t D, R, Ld, Gd, Lr, Gr, clip, peak;
    uint32_t TR, strips, rblocks, chunk, pitchP;
};

template <typename R> struct bits_type;
template <> struct bits_type<float> {
    typedef uint32_t type;
};
template <> struct bits_type<double> {
    typedef uint64_t type;
};

// cfar.hip's rule: a NaN threshold leaves as the canonical quiet NaN
template <typename R> __device__ __forceinline__ R canonical(R th)
{
    using K = typename bits_type<R>::type;
    const K quiet = sizeof(K) == 4 ? K(0x7FC00000u) : K(0x7FF8000000000000ull);
    R q;
    __builtin_memcpy(&q, &quiet, sizeof(q));
    return th != th ? q : th;
}
template <typename R> __device__ __forceinline__ R infinity()
{
    using K = typename bits_type<R>::type;
    const K inf = sizeof(K) == 4 ? K(0x7F800000u) : K(0x7FF0000000000000ull);
    R q;
    __builtin_memcpy(&q, &inf, sizeof(q));
    return q;
}

// MARK: the columns whose range window leaves the map
__device__ __forceinline__ bool marked(const c2_kargs &a, uint32_t col)
{
    const uint32_t Hr = a.Lr + a.Gr;
    return !a.clip && (col < Hr || static_cast<uint64_t>(col) + Hr >= a.R);
}

// the 3 x 3 peak rule for the cell (d, col) of power pv: > for the neighbours in front of it in (i, j) order, >= behind it
template <typename R> __device__ bool is_peak(const c2_kargs &a, const R *map, uint32_t d, uint32_t col, R pv)
{
    for (int i = -1; i <= 1; i++) {
        const uint64_t row = (static_cast<uint64_t>(d) + a.D + i) % a.D;
        for (int j = -1; j <= 1; j++) {
            if (i == 0 && j == 0)
                continue;
            const int64_t c = static_cast<int64_t>(col) + j;
            if (c < 0 || c >= static_cast<int64_t>(a.R))
                continue;
            const R q = map[row * a.R + static_cast<uint64_t>(c)];
            const bool before = i < 0 || (i == 0 && j < 0);
            if (!(before ? pv > q : pv >= q))
                return false;
        }
    }
    return true;
}

// One cell from global memory in the contract's order: the plain kernels, and the thresholds of variant 0's hit records.
template <typename R> __device__ void direct_cell(const c2_kargs &a, const R *map, uint32_t d, uint32_t col, R &th, bool &hit)
{
    const int Hd = static_cast<int>(a.Ld + a.Gd), Gd = static_cast<int>(a.Gd), Hr = static_cast<int>(a.Lr + a.Gr), Gr = static_cast<int>(a.Gr);
    R top = R(0), band = R(0), bottom = R(0);
    for (int i = -Hd; i <= Hd; i++) {
        const R *row = map + ((static_cast<uint64_t>(d) + a.D + i) % a.D) * a.R;
        auto at = [&](int j) -> R {
            const int64_t c = static_cast<int64_t>(col) + j;
            return (c >= 0 && c < static_cast<int64_t>(a.R)) ? row[c] : R(0);
        };
        R lag = R(0), mid = R(0), lead = R(0);
        for (int j = -Hr; j < -Gr; j++)
            lag = lag + at(j);
        for (int j = -Gr; j <= Gr; j++)
            mid = mid + at(j);
        for (int j = Gr + 1; j <= Hr; j++)
            lead = lead + at(j);
        if (i < -Gd) {
            const R lm = lag + mid;
            top = top + (lm + lead);
        } else if (i <= Gd) {
            band = band + (lag + lead);
        } else {
            const R lm = lag + mid;
            bottom = bottom + (lm + lead);
        }
    }
    const R tb = top + band;
    const R T = tb + bottom;
    th = canonical<R>(T * static_cast<const R *>(a.scale)[col]);
    if (marked(a, col))
        th = infinity<R>();
    const R pv = map[static_cast<uint64_t>(d) * a.R + col];
    hit = pv > th;
    if (hit && a.peak)
        hit = is_peak<R>(a, map, d, col, pv);
}

template <typename R> __device__ __forceinline__ void put_record(const c2_kargs &a, uint64_t m, uint64_t pos, uint32_t d, uint32_t col, R pv, R th)
{
    constexpr size_t rec = sizeof(R) == 4 ? 16 : 24;
    unsigned char *at = static_cast<unsigned char *>(a.hits) + (m * a.cap + pos) * rec;
    reinterpret_cast<uint32_t *>(at)[0] = d;
    reinterpret_cast<uint32_t *>(at)[1] = col;
    reinterpret_cast<R *>(at + 8)[0] = pv;
    reinterpret_cast<R *>(at + 8)[1] = th;
}

__device__ __forceinline__ uint32_t saturated(uint64_t v) { return v > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(v); }

// ---- variant 0 ------------------------------------------------------------------------------------------------------------------------
// acc[r] = ((+0 + base[r stride]) + ..) + base[(r + L - 1) stride], r < 8: every element is read once into a register window that
// slides over the elements.  Reads base[0 .. (L + 6) stride], also where L is small; the callers' arrays hold them.
template <typename R> __device__ __forceinline__ void box8(const R *base, uint32_t stride, uint32_t L, R (&acc)[kWin])
{
    R w[2 * kWin - 1]; // w[i] = base[(t + i) stride]: step t gives element t + r to sum r, so no addition waits on a condition
#pragma unroll
    for (uint32_t r = 0; r < kWin; r++)
        acc[r] = R(0);
#pragma unroll
    for (uint32_t i = 0; i < kWin - 1; i++)
        w[i] = base[i * stride];
    uint32_t t = 0;
    for (; t + kWin <= L; t += kWin) { // eight steps on fifteen elements, every index a constant
#pragma unroll
        for (uint32_t i = 0; i < kWin; i++)
            w[kWin - 1 + i] = base[(t + kWin - 1 + i) * stride];
#pragma unroll
        for (uint32_t s = 0; s < kWin; s++)
#pragma unroll
            for (uint32_t r = 0; r < kWin; r++)
                acc[r] = acc[r] + w[s + r];
#pragma unroll
        for (uint32_t i = 0; i < kWin - 1; i++)
            w[i] = w[kWin + i];
    }
    for (; t < L; t++) { // one step, then the window moves by one
        w[kWin - 1] = base[(t + kWin - 1) * stride];
#pragma unroll
        for (uint32_t r = 0; r < kWin; r++)
            acc[r] = acc[r] + w[r];
#pragma unroll
        for (uint32_t i = 0; i < kWin - 1; i++)
            w[i] = w[i + 1];
    }
}

// LDS: full[NR][kPitchS], side[NR][kPitchS], centre[TR][kCols], chunk[chunk][pitchP]; NR = TR + 2 Hd.  Staged row q is map row
// (d0 - Hd + q) mod D, staged column x is map column c0 - Hr + x.
template <typename R> __global__ __launch_bounds__(256) void sdsp_cfar2d_kernel(c2_kargs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t Hd = a.Ld + a.Gd, Hr = a.Lr + a.Gr, TR = a.TR, NR = TR + 2 * Hd, W = kCols + 2 * Hr;
    R *full = reinterpret_cast<R *>(smem);
    R *side = full + NR * kPitchS;
    R *centre = side + NR * kPitchS;
    R *chunk = centre + TR * kCols;
    const uint32_t tid = threadIdx.x, threads = blockDim.x;
    const uint32_t s = blockIdx.x % a.strips, t = blockIdx.x / a.strips, rb = t % a.rblocks;
    const uint64_t m = t / a.rblocks;
    const uint32_t d0 = rb * TR, c0 = s * kCols;
    const R *map = static_cast<const R *>(a.p) + m * a.D * a.R;

    for (uint32_t q0 = 0; q0 < NR; q0 += a.chunk) {
        const uint32_t rows = NR - q0 < a.chunk ? NR - q0 : a.chunk;
        // a wave per staged row, its lanes along the row: the row's place in the map is found once per row (d0 + D - Hd + q < 2^22)
        for (uint32_t rr = tid >> 6; rr < rows; rr += threads >> 6) {
            const uint32_t q = q0 + rr, row = (d0 + a.D - Hd + q) % a.D;
            const R *src = map + static_cast<uint64_t>(row) * a.R;
            const bool mid_row = q >= Hd && q < Hd + TR;
            for (uint32_t x = tid & 63u; x < W; x += 64) {
                const int64_t col = static_cast<int64_t>(c0) - Hr + x;
                const R v = (col >= 0 && col < static_cast<int64_t>(a.R)) ? src[col] : R(0);
                chunk[rr * a.pitchP + x] = v;
                if (mid_row && x >= Hr && x < Hr + kCols)
                    centre[(q - Hd) * kCols + (x - Hr)] = v;
            }
        }
        __syncthreads();
        // a thread takes columns 8 g .. 8 g + 7 of row rr.  The 32 lanes of a half wave walk 32 rows, whose pitch is odd: no two of
        // them on one bank.  Piece j of the half waves: column group j % 8 of rows 32 (j / 8) .. + 31.
        for (uint32_t j = tid >> 5; j < (kCols / kWin) * ((rows + 31) / 32); j += threads >> 5) {
            const uint32_t g = j % (kCols / kWin), rr = (j / (kCols / kWin)) * 32 + (tid & 31u);
            if (rr >= rows)
                continue;
            const R *base = chunk + rr * a.pitchP + g * kWin; // column c0 + 8 g - Hr
            R lag[kWin], mid[kWin], lead[kWin];
            box8<R>(base, 1, a.Lr, lag);
            box8<R>(base + a.Lr, 1, 2 * a.Gr + 1, mid);
            box8<R>(base + Hr + a.Gr + 1, 1, a.Lr, lead);
            const uint32_t o = (q0 + rr) * kPitchS + g * kWin;
#pragma unroll
            for (uint32_t r = 0; r < kWin; r++) {
                const R lm = lag[r] + mid[r];
                side[o + r] = lag[r] + lead[r];
                full[o + r] = lm + lead[r];
            }
        }
        __syncthreads();
    }

    const uint32_t lane = tid & 63u, dl0 = (tid >> 6) * kWin, col = c0 + lane;
    R top[kWin], band[kWin], bottom[kWin];
    box8<R>(full + dl0 * kPitchS + lane, kPitchS, a.Ld, top);
    box8<R>(side + (dl0 + a.Ld) * kPitchS + lane, kPitchS, 2 * a.Gd + 1, band);
    box8<R>(full + (dl0 + Hd + a.Gd + 1) * kPitchS + lane, kPitchS, a.Ld, bottom);
    const bool in_map = col < a.R;
    const R c = in_map ? static_cast<const R *>(a.scale)[col] : R(0);
    const bool edge = marked(a, col);
#pragma unroll
    for (uint32_t r = 0; r < kWin; r++) {
        const uint32_t d = d0 + dl0 + r;
        if (d >= a.D) // the same for the whole wave
            break;
        const R tb = top[r] + band[r];
        const R T = tb + bottom[r];
        R th = canonical<R>(T * c);
        if (edge)
            th = infinity<R>();
        const R pv = centre[(dl0 + r) * kCols + lane];
        bool hit = in_map && pv > th;
        if (hit && a.peak)
            hit = is_peak<R>(a, map, d, col, pv);
        if (in_map) {
            const uint64_t at = (m * a.D + d) * a.R + col;
            if (a.thr)
                static_cast<R *>(a.thr)[at] = th;
            if (a.det)
                a.det[at] = hit ? 1 : 0;
        }
        if (a.mask) {
            const uint64_t b = __ballot(hit);
            if (lane == 0) {
                const uint64_t seg = (m * a.D + d) * a.strips + s;
                a.mask[seg] = b;
                a.cnt[seg] = static_cast<uint32_t>(__popcll(b));
            }
        }
    }
}

// cnt[map][segment] -> its exclusive prefix within the map; counts[map] = the total
__global__ __launch_bounds__(kThreads) void sdsp_cfar2d_scan_kernel(c2_kargs a)
{
    __shared__ uint64_t wave_sum[kThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint64_t nseg = static_cast<uint64_t>(a.D) * a.strips;
    uint32_t *cnt = a.cnt + blockIdx.x * nseg;
    uint64_t base = 0;
    for (uint64_t i0 = 0; i0 < nseg; i0 += kThreads * kWin) {
        const uint64_t at = i0 + static_cast<uint64_t>(tid) * kWin;
        uint64_t before[kWin], sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kWin; k++) {
            before[k] = sum;
            sum += at + k < nseg ? cnt[at + k] : 0u;
        }
        uint64_t x = sum; // inclusive over the wave
        for (uint32_t off = 1; off < 64; off <<= 1) {
            const uint64_t y = __shfl_up(x, off);
            if (lane >= off)
                x += y;
        }
        if (lane == 63)
            wave_sum[w] = x;
        __syncthreads();
        uint64_t in_front = 0, total = 0;
        for (uint32_t k = 0; k < kThreads / 64; k++) {
            in_front += k < w ? wave_sum[k] : 0;
            total += wave_sum[k];
        }
        const uint64_t mine = base + in_front + x - sum;
#pragma unroll
        for (uint32_t k = 0; k < kWin; k++)
            if (at + k < nseg)
                cnt[at + k] = saturated(mine + before[k]);
        base += total;
        __syncthreads();
    }
    if (tid == 0)
        a.counts[blockIdx.x] = saturated(base);
}

template <typename R> __global__ __launch_bounds__(kThreads) void sdsp_cfar2d_place_kernel(c2_kargs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nseg = static_cast<uint64_t>(a.D) * a.strips, all = a.maps * nseg;
    const uint64_t first = (static_cast<uint64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6)) * 64;
    const uint64_t mine = first + lane < all ? a.mask[first + lane] : 0;
    const uint32_t offset = first + lane < all ? a.cnt[first + lane] : 0;
    uint64_t busy = __ballot(mine != 0);
    while (busy) { // the same for the whole wave
        const int k = __ffsll(static_cast<unsigned long long>(busy)) - 1;
        busy &= busy - 1;
        const uint64_t bits = (static_cast<uint64_t>(__shfl(static_cast<uint32_t>(mine >> 32), k)) << 32) | __shfl(static_cast<uint32_t>(mine), k);
        const uint64_t pos = static_cast<uint64_t>(__shfl(offset, k)) + __popcll(bits & ((1ull << lane) - 1));
        if (!((bits >> lane) & 1) || pos >= a.cap)
            continue;
        const uint64_t seg = first + k, m = udiv(seg, nseg), rest = seg - m * nseg;
        const uint32_t d = static_cast<uint32_t>(udiv(rest, a.strips)), col = static_cast<uint32_t>(rest - static_cast<uint64_t>(d) * a.strips) * kCols + lane;
        const R *map = static_cast<const R *>(a.p) + m * a.D * a.R;
        R th;
        bool hit;
        direct_cell<R>(a, map, d, col, th, hit);
        put_record<R>(a, m, pos, d, col, map[static_cast<uint64_t>(d) * a.R + col], th);
    }
}

// ---- variant 1 ------------------------------------------------------------------------------------------------------------------------
template <typename R> __global__ __launch_bounds__(kThreads) void sdsp_cfar2d_plain_kernel(c2_kargs a)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x, cells = static_cast<uint64_t>(a.D) * a.R;
    if (i >= a.maps * cells)
        return;
    const uint64_t m = udiv(i, cells), rest = i - m * cells;
    const uint32_t d = static_cast<uint32_t>(udiv(rest, a.R)), col = static_cast<uint32_t>(rest - static_cast<uint64_t>(d) * a.R);
    R th;
    bool hit;
    direct_cell<R>(a, static_cast<const R *>(a.p) + m * cells, d, col, th, hit);
    if (a.thr)
        static_cast<R *>(a.thr)[i] = th;
    if (a.det)
        a.det[i] = hit ? 1 : 0;
}

// One thread per piece of kCols columns of a row, the pieces of a map in (d, piece) order.  PLACE = false: cnt[piece] = its hits;
// PLACE = true: its records from offset cnt[piece] on.
template <typename R, bool PLACE> __global__ __launch_bounds__(kThreads) void sdsp_cfar2d_plain_piece_kernel(c2_kargs a)
{
    const uint64_t piece = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x, per_map = static_cast<uint64_t>(a.D) * a.strips;
    if (piece >= a.maps * per_map)
        return;
    const uint64_t m = udiv(piece, per_map), rest = piece - m * per_map;
    const uint32_t d = static_cast<uint32_t>(udiv(rest, a.strips)), c0 = static_cast<uint32_t>(rest - static_cast<uint64_t>(d) * a.strips) * kCols;
    const uint32_t c1 = a.R - c0 < kCols ? a.R : c0 + kCols;
    const R *map = static_cast<const R *>(a.p) + m * a.D * a.R;
    uint64_t n = PLACE ? a.cnt[piece] : 0;
    for (uint32_t col = c0; col < c1; col++) {
        R th;
        bool hit;
        direct_cell<R>(a, map, d, col, th, hit);
        if (!hit)
            continue;
        if (PLACE && n < a.cap)
            put_record<R>(a, m, n, d, col, map[static_cast<uint64_t>(d) * a.R + col], th);
        n++;
    }
    if (!PLACE)
        a.cnt[piece] = saturated(n);
}

// one thread per map, one piece after the other
__global__ __launch_bounds__(kThreads) void sdsp_cfar2d_plain_scan_kernel(c2_kargs a)
{
    const uint64_t m = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x, per_map = static_cast<uint64_t>(a.D) * a.strips;
    if (m >= a.maps)
        return;
    uint64_t sum = 0;
    for (uint64_t i = 0; i < per_map; i++) {
        const uint32_t v = a.cnt[m * per_map + i];
        a.cnt[m * per_map + i] = saturated(sum);
        sum += v;
    }
    a.counts[m] = saturated(sum);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
uint32_t elem(int precision) { return precision == SDSP_HIP_F64 ? 8u : 4u; }

struct tile {
    uint32_t TR, chunk, pitchP, lds;
};
tile tile_for(int precision, uint32_t D, uint32_t Ld, uint32_t Gd, uint32_t Lr, uint32_t Gr)
{
    const uint32_t es = elem(precision), Hd = Ld + Gd, Hr = Lr + Gr;
    tile t{};
    t.pitchP = (kCols + 2 * Hr) | 1u;
    auto bytes = [&](uint32_t TR, uint32_t *chunk) {
        const uint32_t NR = TR + 2 * Hd;
        *chunk = std::min(NR, std::max(kWin, kChunkBytes / (t.pitchP * es)));
        return (2 * NR * kPitchS + TR * kCols + *chunk * t.pitchP) * es;
    };
    t.TR = 32; // halved while the tile misses the goal of two workgroups per CU or half of it would hold every row
    while (t.TR > 8 && (bytes(t.TR, &t.chunk) > kLdsGoal || t.TR / 2 >= D))
        t.TR /= 2;
    t.lds = bytes(t.TR, &t.chunk);
    return t;
}

template <typename R> int launch_r(const cfar2d_args &ca, int variant, hipStream_t stream)
{
    const int precision = sizeof(R) == 8 ? SDSP_HIP_F64 : SDSP_HIP_F32;
    auto kern = sdsp_cfar2d_kernel<R>;
    static std::atomic<uint64_t> lds_done{ 0 };
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), kMaxLds, lds_done))
        return rc;
    if (!ca.p) // plan creation: the attribute only
        return SDSP_HIP_OK;
    const tile t = tile_for(precision, ca.D, ca.Ld, ca.Gd, ca.Lr, ca.Gr);
    if (t.lds > kMaxLds)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "cfar2d: the window does not fit the LDS");
    c2_kargs k{};
    k.p = ca.p;
    k.thr = ca.thr;
    k.det = ca.det;
    k.hits = ca.hits;
    k.counts = ca.counts;
    k.scale = ca.scale;
    k.mask = ca.hits ? static_cast<uint64_t *>(ca.ws_mask) : nullptr;
    k.cnt = ca.ws_cnt;
    k.maps = ca.maps;
    k.cap = ca.cap;
    k.D = ca.D;
    k.R = ca.R;
    k.Ld = ca.Ld;
    k.Gd = ca.Gd;
    k.Lr = ca.Lr;
    k.Gr = ca.Gr;
    k.clip = ca.clip ? 1u : 0u;
    k.peak = ca.peak ? 1u : 0u;
    k.TR = t.TR;
    k.chunk = t.chunk;
    k.pitchP = t.pitchP;
    k.strips = (ca.R + kCols - 1) / kCols;
    k.rblocks = (ca.D + t.TR - 1) / t.TR;
    dim3 grid;
    if (variant == 1) {
        if (ca.thr || ca.det) {
            if (int rc = grid_for(ca.maps * ca.D * ca.R, "cfar2d", &grid))
                return rc;
            hipLaunchKernelGGL(sdsp_cfar2d_plain_kernel<R>, grid, dim3(kThreads), 0, stream, k);
        }
        if (ca.hits) {
            if (int rc = grid_for(ca.maps * ca.D * k.strips, "cfar2d", &grid))
                return rc;
            hipLaunchKernelGGL((sdsp_cfar2d_plain_piece_kernel<R, false>), grid, dim3(kThreads), 0, stream, k);
            dim3 per_map;
            if (int rc = grid_for(ca.maps, "cfar2d", &per_map))
                return rc;
            hipLaunchKernelGGL(sdsp_cfar2d_plain_scan_kernel, per_map, dim3(kThreads), 0, stream, k);
            hipLaunchKernelGGL((sdsp_cfar2d_plain_piece_kernel<R, true>), grid, dim3(kThreads), 0, stream, k);
        }
        return launch_status("cfar2d");
    }
    const uint64_t nseg = static_cast<uint64_t>(ca.D) * k.strips;
    if (int rc = grid_of_blocks(ca.maps * k.rblocks * k.strips, "cfar2d", &grid))
        return rc;
    hipLaunchKernelGGL(kern, grid, dim3(t.TR * kWin), t.lds, stream, k);
    if (ca.hits) {
        if (int rc = grid_of_blocks(ca.maps, "cfar2d", &grid))
            return rc;
        hipLaunchKernelGGL(sdsp_cfar2d_scan_kernel, grid, dim3(kThreads), 0, stream, k);
        if (int rc = grid_of_blocks((ca.maps * nseg + kThreads - 1) / kThreads, "cfar2d", &grid))
            return rc;
        hipLaunchKernelGGL(sdsp_cfar2d_place_kernel<R>, grid, dim3(kThreads), 0, stream, k);
    }
    return launch_status("cfar2d");
}
} // namespace

// with a.p == nullptr: raises the dynamic-LDS limit of sdsp_cfar2d_kernel and launches nothing (plan creation, so that a captured
// process sets no attribute)
int launch_cfar2d(int precision, const cfar2d_args &a, int variant, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    return precision == SDSP_HIP_F64 ? launch_r<double>(a, variant, s) : launch_r<float>(a, variant, s);
}

cfar2d_shape cfar2d_shape_for(int precision, uint32_t D, uint32_t Ld, uint32_t Gd, uint32_t Lr, uint32_t Gr, int variant)
{
    cfar2d_shape s{};
    if (variant == 1) {
        s.tile_rows = 1;
        s.tile_cols = kThreads;
        s.threads = kThreads;
        return s;
    }
    const tile t = tile_for(precision, D, Ld, Gd, Lr, Gr);
    s.tile_rows = t.TR;
    s.tile_cols = kCols;
    s.threads = t.TR * kWin;
    s.lds_bytes = t.lds;
    return s;
}

// the list's workspace of a plan for max_maps maps: a 64-bit ballot and a 32-bit count per (map, d, strip) segment
void cfar2d_workspace(uint32_t D, uint32_t R, uint64_t max_maps, uint64_t *mask_bytes, uint64_t *cnt_bytes)
{
    const uint64_t segs = max_maps * D * ((R + kCols - 1) / kCols);
    *mask_bytes = segs * 8;
    *cnt_bytes = segs * 4;
}

uint64_t cfar2d_launches(int variant, bool maps_out, bool list)
{
    if (variant == 1)
        return (maps_out ? 1 : 0) + (list ? 3 : 0);
    return 1 + (list ? 2 : 0);
}

const char *cfar2d_kernel_for(int variant) { return variant ? "sdsp_cfar2d_plain_kernel" : "sdsp_cfar2d_kernel"; }
} // namespace sdsp_hip
