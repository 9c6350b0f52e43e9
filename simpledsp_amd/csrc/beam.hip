// beam.hip -- time-delay (filter-and-sum) beamformer banks for MI355X (gfx950): every beam is a sum over sensors of the sensor's stream
// delayed by whole samples and filtered with the entry's own T taps.
//
// Output n of beam b of a call (x_c = the sensor's history, then the block): one accumulator from +0 over the beam's entries in order
// and, within an entry, over ascending t:
//     acc = g[t] x_c[n - delay - t] + acc       one fmaf in f32, a multiply then an add in f64; complex: the four steps of tap_c
// The taps come rounded from the plan (capi.hip); built with -ffp-contract=off, so nothing here contracts.  DESIGN.md section 5.24.
//
// Two kernels:
//   sdsp_beam_kernel        variant 0.  A workgroup owns one group, one block of kBlockOut outputs and one chunk of up to kBeamChunk
//                           consecutive beams.  It walks the sensors the chunk uses in ascending order; for each it stages in LDS only
//                           the window the chunk's beams need, [n0 - dmax - T + 1, n0 + block - dmin) with dmin, dmax over the chunk's
//                           entries on that sensor -- 16-byte nontemporal loads where a whole 16 bytes lie in the row, element by
//                           element from `state` or the row at the head and tail, a padded line so that lanes reading at stride 4
//                           spread over the banks.  Two lines: the next sensor's window is staged before the current one is used, one
//                           barrier per sensor.  A lane owns four consecutive outputs of every beam of the chunk, accumulators in
//                           registers across all sensors; for one entry it slides a window of four registers over the taps, the tap
//                           loop unrolled by four with the registers rotating by name, so one LDS read feeds four multiply-adds
//                           (sixteen for complex rows) and nothing is moved.  The taps are wave-uniform scalar loads; a beam without
//                           an entry on the sensor is skipped by a wave-uniform branch.  Results leave as 16-byte stores where the
//                           lane's four outputs are aligned, element stores otherwise.
//   sdsp_beam_plain_kernel  variant 1: one output per thread straight from global memory and `state`, the independent cross-check.
// The chunk table (beam_build_table) is made at plan creation: chunks are consecutive beams, shrunk until the widest sensor window
// fits one LDS line; a chunk of one beam has spread 0 and always fits.  The new history is carry_history's (stream_carry.hip),
// launched by the caller behind either kernel.
#include "stream_dev.h"

#include <type_traits>

namespace sdsp_hip
{
namespace
{
constexpr int kPerLane = 4;                        // consecutive outputs per lane: the register window
constexpr uint32_t kBlockOut = kThreads * kPerLane; // outputs per beam and workgroup
constexpr uint32_t kBeamChunk = 4;                 // beams whose accumulators a lane keeps
constexpr size_t kLineBytes = 32 * 1024;           // one LDS line at most; two lines, two workgroups per CU
constexpr size_t kLdsLimit = 2 * kLineBytes;
constexpr uint32_t kNone = 0xffffffffu;

template <typename R> __device__ __forceinline__ R mul_add(R g, R x, R acc);
template <> __device__ __forceinline__ float mul_add<float>(float g, float x, float acc) { return __builtin_fmaf(g, x, acc); }
template <> __device__ __forceinline__ double mul_add<double>(double g, double x, double acc) { return acc + g * x; }
template <typename R> __device__ __forceinline__ R mul_sub(R g, R x, R acc);
template <> __device__ __forceinline__ float mul_sub<float>(float g, float x, float acc) { return __builtin_fmaf(-g, x, acc); }
template <> __device__ __forceinline__ double mul_sub<double>(double g, double x, double acc) { return acc - g * x; }

// one element of a row: a real, or an interleaved complex pair
template <typename R, bool CPLX> struct elem {
    typedef R type;
};
template <typename R> struct elem<R, true> {
    typedef typename cplx_pair<R>::type type;
};

// one tap in the contract's order (gi is not used for real rows)
__device__ __forceinline__ void tap(float gr, float, float x, float &zr, float &) { zr = mul_add<float>(gr, x, zr); }
__device__ __forceinline__ void tap(double gr, double, double x, double &zr, double &) { zr = mul_add<double>(gr, x, zr); }
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

// the plan's taps and tables are never written by a kernel: the fused kernel reads them through the constant address space, so that
// its wave-uniform reads are scalar loads whatever barriers and stores lie between them
template <typename T> using konst = const T __attribute__((address_space(4)));
template <typename T> __device__ __forceinline__ konst<T> *as_const(const T *p) { return (konst<T> *)reinterpret_cast<uintptr_t>(p); }

struct beam_kargs {
    const void *in;
    void *out;
    const void *state;
    const void *g;
    const uint32_t *entries, *beam_off, *chunks, *recs;
    uint64_t samples, in_stride, out_stride;
    uint32_t taps, hist, sensors, beams, groups;
    uint32_t nblk;       // blocks per row
    uint32_t nchunks;    // beam chunks
    uint32_t line_slots; // elements between the two LDS lines (the padded line, a multiple of what 16 bytes hold)
    uint32_t pad_shift;  // LDS line: element p lives at p + (p >> pad_shift)
};

__device__ __forceinline__ uint32_t slot(uint32_t p, uint32_t shift) { return p + (p >> shift); }

// where a sensor's staged window starts: the first sample the chunk needs, moved down to a 16-byte boundary of the row when the row's
// elements can be loaded 16 bytes at a time (vec)
template <typename E> __device__ __forceinline__ int64_t line_start(const E *row, int64_t lo, bool &vec)
{
    constexpr uint32_t EL = 16 / sizeof(E);
    const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(row) & 15u);
    vec = mis % sizeof(E) == 0;
    if (!vec || EL == 1)
        return lo;
    return lo - ((lo + mis / static_cast<uint32_t>(sizeof(E))) & static_cast<int64_t>(EL - 1));
}

// the window [a0, hi) of one sensor into `line`; samples below lo are not needed (zeros), below 0 they come from the history
template <typename R, bool CPLX>
__device__ __forceinline__ void stage(const beam_kargs &a, typename elem<R, CPLX>::type *line, const typename elem<R, CPLX>::type *row,
                                      const typename elem<R, CPLX>::type *st, int64_t a0, int64_t lo, int64_t hi, bool vec)
{
    using E = typename elem<R, CPLX>::type;
    using V = typename vec16<R>::type;
    constexpr uint32_t EL = 16 / sizeof(E);
    const uint32_t sh = a.pad_shift;
    const uint32_t nv = (static_cast<uint32_t>(hi - a0) + EL - 1) / EL;
    for (uint32_t v = threadIdx.x; v < nv; v += kThreads) {
        const int64_t i0 = a0 + static_cast<int64_t>(v) * EL;
        if (vec && i0 >= 0 && i0 + EL <= static_cast<int64_t>(a.samples)) {
            const V x = __builtin_nontemporal_load(reinterpret_cast<const V *>(row + i0));
#pragma unroll
            for (uint32_t e = 0; e < EL; e++) {
                E y;
                if constexpr (CPLX) {
                    y.x = x[2 * e];
                    y.y = x[2 * e + 1];
                } else {
                    y = x[e];
                }
                line[slot(v * EL + e, sh)] = y;
            }
        } else {
#pragma unroll
            for (uint32_t e = 0; e < EL; e++) {
                const int64_t i = i0 + e;
                E y = E(0);
                if (i >= lo && i < hi) {
                    if (i >= 0)
                        y = row[i];
                    else if (st)
                        y = st[-1 - i]; // -1 - i <= dmax + T - 2 < hist
                }
                line[slot(v * EL + e, sh)] = y;
            }
        }
    }
}

// all T taps of one entry for the lane's four outputs; line[base + r - t] is output r's sample for tap t.  w0..w3 hold line[base + q]
// with q = 0..3 (mod 4); a step loads the one new sample into the register whose sample no output needs any more
template <typename R, bool CPLX>
__device__ __forceinline__ void entry_taps(const typename elem<R, CPLX>::type *line, uint32_t sh, uint32_t base, konst<R> *g, uint32_t T,
                                           R (&zr)[kPerLane], R (&zi)[kPerLane])
{
    using E = typename elem<R, CPLX>::type;
    constexpr uint32_t GS = CPLX ? 2 : 1;
    E w0, w1 = line[slot(base + 1, sh)], w2 = line[slot(base + 2, sh)], w3 = line[slot(base + 3, sh)];
#define SDSP_BEAM_STEP(t_, fresh, x0, x1, x2, x3)                                                                                           \
    {                                                                                                                                    \
        fresh = line[slot(base - (t_), sh)];                                                                                             \
        const R gr = g[static_cast<size_t>(t_) * GS], gi = CPLX ? g[static_cast<size_t>(t_) * GS + GS - 1] : R(0);                         \
        tap(gr, gi, x0, zr[0], zi[0]);                                                                                                   \
        tap(gr, gi, x1, zr[1], zi[1]);                                                                                                   \
        tap(gr, gi, x2, zr[2], zi[2]);                                                                                                   \
        tap(gr, gi, x3, zr[3], zi[3]);                                                                                                   \
    }
    uint32_t t = 0;
    for (; t + 4 <= T; t += 4) {
        SDSP_BEAM_STEP(t, w0, w0, w1, w2, w3)
        SDSP_BEAM_STEP(t + 1, w3, w3, w0, w1, w2)
        SDSP_BEAM_STEP(t + 2, w2, w2, w3, w0, w1)
        SDSP_BEAM_STEP(t + 3, w1, w1, w2, w3, w0)
    }
    if (t < T) {
        SDSP_BEAM_STEP(t, w0, w0, w1, w2, w3)
        if (t + 1 < T) {
            SDSP_BEAM_STEP(t + 1, w3, w3, w0, w1, w2)
            if (t + 2 < T)
                SDSP_BEAM_STEP(t + 2, w2, w2, w3, w0, w1)
        }
    }
#undef SDSP_BEAM_STEP
}

template <typename R, bool CPLX> __global__ __launch_bounds__(kThreads) void sdsp_beam_kernel(beam_kargs a)
{
    using E = typename elem<R, CPLX>::type;
    using V = typename vec16<R>::type;
    constexpr uint32_t GS = CPLX ? 2 : 1;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    E *lines = reinterpret_cast<E *>(lds_raw); // two padded lines

    // neighbouring workgroups (the chunks of one block, then the next block of the group) behind one L2: they read the same samples
    uint32_t wg = xcd_block(blockIdx.x, gridDim.x);
    const uint32_t ck = wg % a.nchunks;
    wg /= a.nchunks;
    const uint32_t blk = wg % a.nblk, grp = wg / a.nblk;
    konst<uint32_t> *ch = as_const(a.chunks) + static_cast<size_t>(ck) * 4;
    const uint32_t beam0 = ch[0], nbeams = ch[1], r0 = ch[2], nrec = ch[3];
    const uint32_t T = a.taps, H = a.hist, sh = a.pad_shift;
    const int64_t n0 = static_cast<int64_t>(blk) * kBlockOut;
    const uint64_t left = a.samples - static_cast<uint64_t>(n0);
    const uint32_t len = left < kBlockOut ? static_cast<uint32_t>(left) : kBlockOut;
    const uint32_t mine = threadIdx.x * kPerLane; // the lane's first output of the block

    R zr[kBeamChunk][kPerLane], zi[kBeamChunk][kPerLane];
#pragma unroll
    for (uint32_t b = 0; b < kBeamChunk; b++)
#pragma unroll
        for (int r = 0; r < kPerLane; r++)
            zr[b][r] = zi[b][r] = R(0);

    // the window of record k into line k & 1
    auto stage_rec = [&](uint32_t k) {
        konst<uint32_t> *rec = as_const(a.recs) + static_cast<size_t>(r0 + k) * 8;
        const uint32_t c = rec[0], dmin = rec[1], dmax = rec[2];
        const uint64_t rowi = static_cast<uint64_t>(grp) * a.sensors + c;
        const E *row = static_cast<const E *>(a.in) + rowi * a.in_stride;
        const E *st = a.state ? static_cast<const E *>(a.state) + rowi * H : nullptr;
        const int64_t lo = n0 - static_cast<int64_t>(dmax) - static_cast<int64_t>(T - 1);
        bool vec;
        const int64_t a0 = line_start<E>(row, lo, vec);
        stage<R, CPLX>(a, lines + static_cast<size_t>(k & 1) * a.line_slots, row, st, a0, lo, n0 + len - static_cast<int64_t>(dmin), vec);
    };

    if (nrec)
        stage_rec(0);
    for (uint32_t k = 0; k < nrec; k++) {
        __syncthreads(); // line k is whole, and nobody reads the other line any more
        if (k + 1 < nrec)
            stage_rec(k + 1);
        konst<uint32_t> *rec = as_const(a.recs) + static_cast<size_t>(r0 + k) * 8;
        const uint32_t c = rec[0], dmax = rec[2];
        const E *row = static_cast<const E *>(a.in) + (static_cast<uint64_t>(grp) * a.sensors + c) * a.in_stride;
        bool vec;
        const int64_t a0 = line_start<E>(row, n0 - static_cast<int64_t>(dmax) - static_cast<int64_t>(T - 1), vec);
        const E *line = lines + static_cast<size_t>(k & 1) * a.line_slots;
#pragma unroll
        for (uint32_t b = 0; b < kBeamChunk; b++) {
            const uint32_t e = rec[4 + b]; // wave-uniform
            if (e != kNone) {
                const uint32_t d = as_const(a.entries)[static_cast<size_t>(e) * 3 + 2];
                // >= T - 1 (the window starts at or below n0 - dmax - T + 1), and base + 3 lies inside the line's capacity
                const uint32_t base = static_cast<uint32_t>(n0 - a0) + mine - d;
                entry_taps<R, CPLX>(line, sh, base, as_const(static_cast<const R *>(a.g)) + static_cast<size_t>(e) * T * GS, T, zr[b], zi[b]);
            }
        }
    }

    if (mine >= len)
        return;
    const uint32_t nvalid = len - mine < kPerLane ? len - mine : kPerLane;
#pragma unroll
    for (uint32_t b = 0; b < kBeamChunk; b++) {
        if (b >= nbeams)
            break;
        E *dst = static_cast<E *>(a.out) + (static_cast<uint64_t>(grp) * a.beams + beam0 + b) * a.out_stride + static_cast<uint64_t>(n0) +
                 mine;
        if (nvalid == kPerLane && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
            constexpr int VL = vec16<R>::lanes;              // reals per 16-byte store
            constexpr int NV = kPerLane * static_cast<int>(GS) / VL; // stores
            R flat[kPerLane * GS];
#pragma unroll
            for (int r = 0; r < kPerLane; r++) {
                flat[r * GS] = zr[b][r];
                if constexpr (CPLX)
                    flat[r * GS + 1] = zi[b][r];
            }
#pragma unroll
            for (int j = 0; j < NV; j++) {
                V v;
#pragma unroll
                for (int i = 0; i < VL; i++)
                    v[i] = flat[j * VL + i];
                __builtin_nontemporal_store(v, reinterpret_cast<V *>(dst) + j);
            }
        } else {
#pragma unroll
            for (int r = 0; r < kPerLane; r++)
                if (static_cast<uint32_t>(r) < nvalid) {
                    E y;
                    if constexpr (CPLX) {
                        y.x = zr[b][r];
                        y.y = zi[b][r];
                    } else {
                        y = zr[b][r];
                    }
                    __builtin_nontemporal_store(y, dst + r);
                }
        }
    }
}

// ---- variant 1: one output per thread from global memory ----------------------------------------------------------------------
template <typename R, bool CPLX> __global__ __launch_bounds__(kThreads) void sdsp_beam_plain_kernel(beam_kargs a)
{
    using E = typename elem<R, CPLX>::type;
    constexpr uint32_t GS = CPLX ? 2 : 1;
    const uint64_t rows = static_cast<uint64_t>(a.groups) * a.beams, total = rows * a.samples;
    const uint32_t H = a.hist, T = a.taps;
    for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; idx < total;
         idx += static_cast<uint64_t>(gridDim.x) * kThreads) {
        const uint64_t orow = udiv(idx, a.samples), n = idx - orow * a.samples;
        const uint64_t grp = udiv(orow, a.beams);
        const uint32_t b = static_cast<uint32_t>(orow - grp * a.beams);
        R zr = R(0), zi = R(0);
        for (uint32_t e = a.beam_off[b]; e < a.beam_off[b + 1]; e++) {
            const uint32_t c = a.entries[static_cast<size_t>(e) * 3 + 1], d = a.entries[static_cast<size_t>(e) * 3 + 2];
            const uint64_t rowi = grp * a.sensors + c;
            const E *inp = static_cast<const E *>(a.in) + rowi * a.in_stride;
            const E *st = a.state ? static_cast<const E *>(a.state) + rowi * H : nullptr;
            const R *g = static_cast<const R *>(a.g) + static_cast<size_t>(e) * T * GS;
            for (uint32_t t = 0; t < T; t++) {
                const int64_t xi = static_cast<int64_t>(n) - static_cast<int64_t>(d) - static_cast<int64_t>(t);
                const E x = xi >= 0 ? inp[xi] : (st ? st[-1 - xi] : E(0)); // -1 - xi <= d + T - 2 < hist
                tap(g[static_cast<size_t>(t) * GS], CPLX ? g[static_cast<size_t>(t) * GS + GS - 1] : R(0), x, zr, zi);
            }
        }
        E y;
        if constexpr (CPLX) {
            y.x = zr;
            y.y = zi;
        } else {
            y = zr;
        }
        static_cast<E *>(a.out)[orow * a.out_stride + n] = y;
    }
}

size_t elem_bytes(int precision, int complex_in) { return (precision == SDSP_HIP_F64 ? 8u : 4u) * (complex_in ? 2u : 1u); }

// one element after every 2^shift: the lanes of one LDS access cycle (32 for the 4- and 8-byte reads, 16 for the 16-byte read), reading
// at a stride of kPerLane elements, land on different banks
uint32_t pad_shift_for(size_t es) { return es == 16 ? 4 : 5; }

// padded slots of a line of `elems` elements, rounded up to whole 16 bytes
uint32_t line_slots_for(uint32_t elems, size_t es)
{
    const uint32_t el = static_cast<uint32_t>(16 / es), s = elems + (elems >> pad_shift_for(es)) + 1;
    return (s + el - 1) / el * el;
}

// elements of a staged window with this delay spread: the block, the spread, T - 1 in front, and what moving its start down and its end
// up to 16-byte boundaries can add
uint32_t window_elems(uint32_t spread, uint32_t taps, size_t es)
{
    return kBlockOut + spread + (taps - 1) + 2 * static_cast<uint32_t>(16 / es);
}

template <typename F> int with_kernel(int precision, int complex_in, F f)
{
    if (precision == SDSP_HIP_F64)
        return complex_in ? f(double(), std::true_type()) : f(double(), std::false_type());
    return complex_in ? f(float(), std::true_type()) : f(float(), std::false_type());
}
} // namespace

uint32_t beam_block_out() { return kBlockOut; }

void beam_build_table(int precision, int complex_in, uint32_t taps, uint32_t beams, uint32_t n_entries, const sdsp_hip_beam_entry *entries,
                      std::vector<uint32_t> &table, beam_layout &lay)
{
    const size_t es = elem_bytes(precision, complex_in);
    // the widest spread whose window still fits one line (>= 0 for every T within the limit: a chunk of one beam always fits)
    const uint32_t cap = static_cast<uint32_t>(kLineBytes / es);
    uint32_t spread_max = cap - (cap >> pad_shift_for(es)) - window_elems(0, taps, es); // within a few elements of the bound
    while (line_slots_for(window_elems(spread_max, taps, es), es) > cap)
        spread_max--;
    if (spread_max > SDSP_HIP_BEAM_MAX_DELAY)
        spread_max = SDSP_HIP_BEAM_MAX_DELAY;
    std::vector<uint32_t> beam_off(static_cast<size_t>(beams) + 1, 0);
    for (uint32_t e = 0; e < n_entries; e++)
        beam_off[entries[e].beam + 1]++;
    for (uint32_t b = 0; b < beams; b++)
        beam_off[b + 1] += beam_off[b];

    // records of the chunk [b0, b0 + n): the sensors it uses, ascending, with the delay range and each beam's entry
    std::vector<uint32_t> chunks, recs, trial;
    auto records = [&](uint32_t b0, uint32_t n, std::vector<uint32_t> &out) {
        uint32_t widest = 0;
        uint32_t cur[kBeamChunk];
        for (uint32_t j = 0; j < n; j++)
            cur[j] = beam_off[b0 + j];
        out.clear();
        for (;;) {
            uint32_t c = kNone; // the smallest sensor not yet taken
            for (uint32_t j = 0; j < n; j++)
                if (cur[j] < beam_off[b0 + j + 1] && entries[cur[j]].sensor < c)
                    c = entries[cur[j]].sensor;
            if (c == kNone)
                break;
            uint32_t rec[8] = { c, 0xffffffffu, 0, 0, kNone, kNone, kNone, kNone };
            for (uint32_t j = 0; j < n; j++)
                if (cur[j] < beam_off[b0 + j + 1] && entries[cur[j]].sensor == c) {
                    const uint32_t d = entries[cur[j]].delay;
                    rec[1] = d < rec[1] ? d : rec[1];
                    rec[2] = d > rec[2] ? d : rec[2];
                    rec[4 + j] = cur[j]++;
                }
            widest = rec[2] - rec[1] > widest ? rec[2] - rec[1] : widest;
            out.insert(out.end(), rec, rec + 8);
        }
        return widest;
    };
    uint32_t widest_kept = 0;
    for (uint32_t b0 = 0; b0 < beams;) {
        uint32_t n = beams - b0 < kBeamChunk ? beams - b0 : kBeamChunk, widest;
        while ((widest = records(b0, n, trial)) > spread_max)
            n--; // n = 1 has spread 0
        const uint32_t hdr[4] = { b0, n, static_cast<uint32_t>(recs.size() / 8), static_cast<uint32_t>(trial.size() / 8) };
        chunks.insert(chunks.end(), hdr, hdr + 4);
        recs.insert(recs.end(), trial.begin(), trial.end());
        widest_kept = widest > widest_kept ? widest : widest_kept;
        b0 += n;
    }
    table.clear();
    for (uint32_t e = 0; e < n_entries; e++) {
        const uint32_t w[3] = { entries[e].beam, entries[e].sensor, entries[e].delay };
        table.insert(table.end(), w, w + 3);
    }
    lay.off_beams = static_cast<uint32_t>(table.size());
    table.insert(table.end(), beam_off.begin(), beam_off.end());
    lay.off_chunks = static_cast<uint32_t>(table.size());
    table.insert(table.end(), chunks.begin(), chunks.end());
    lay.off_recs = static_cast<uint32_t>(table.size());
    table.insert(table.end(), recs.begin(), recs.end());
    lay.chunks = static_cast<uint32_t>(chunks.size() / 4);
    lay.max_spread = spread_max;
    lay.line_elems = window_elems(widest_kept, taps, es);
    lay.lds_line_bytes = static_cast<uint32_t>(line_slots_for(lay.line_elems, es) * es);
}

int beam_prepare(int precision, int complex_in)
{
    static std::atomic<uint64_t> done[4];
    return with_kernel(precision, complex_in, [&](auto r, auto cplx) {
        constexpr bool c = decltype(cplx)::value;
        return ensure_dynamic_lds(reinterpret_cast<const void *>(sdsp_beam_kernel<decltype(r), c>), kLdsLimit,
                                  done[(sizeof(r) == 8 ? 2 : 0) + (c ? 1 : 0)]);
    });
}

const char *beam_kernel_for(int variant) { return variant == 1 ? "sdsp_beam_plain_kernel" : "sdsp_beam_kernel"; }

int launch_beam(int precision, const beam_args &ba, int variant, void *stream_v)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const size_t es = elem_bytes(precision, ba.complex_in);
    beam_kargs k{};
    k.in = ba.in;
    k.out = ba.out;
    k.hist = ba.hist;
    k.state = k.hist ? ba.state : nullptr;
    k.g = ba.g;
    k.entries = ba.table;
    k.beam_off = ba.table + ba.lay.off_beams;
    k.chunks = ba.table + ba.lay.off_chunks;
    k.recs = ba.table + ba.lay.off_recs;
    k.samples = ba.samples;
    k.in_stride = ba.in_stride;
    k.out_stride = ba.out_stride;
    k.taps = ba.taps;
    k.sensors = ba.sensors;
    k.beams = ba.beams;
    k.groups = ba.groups;
    k.nchunks = ba.lay.chunks;
    k.pad_shift = pad_shift_for(es);
    k.line_slots = line_slots_for(ba.lay.line_elems, es);
    dim3 grid;
    if (variant == 1) {
        const uint64_t total = static_cast<uint64_t>(ba.groups) * ba.beams * ba.samples; // < 2^31 rows x 2^31 samples
        if (int rc = grid_for(total < (65536ull * kThreads) ? total : 65536ull * kThreads, "beam", &grid)) // grid-stride beyond
            return rc;
        if (int rc = with_kernel(precision, ba.complex_in, [&](auto r, auto cplx) {
                hipLaunchKernelGGL((sdsp_beam_plain_kernel<decltype(r), decltype(cplx)::value>), grid, dim3(kThreads), 0, stream, k);
                return static_cast<int>(SDSP_HIP_OK);
            }))
            return rc;
        return launch_status("beam");
    }
    const uint64_t nblk = (ba.samples + kBlockOut - 1) / kBlockOut; // < 2^21
    k.nblk = static_cast<uint32_t>(nblk);
    if (nblk * ba.groups > 0x7fffffffull || nblk * ba.groups * k.nchunks > 0x7fffffffull)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "beam too large for one launch");
    if (int rc = grid_of_blocks(nblk * ba.groups * k.nchunks, "beam", &grid))
        return rc;
    const size_t lds = 2 * static_cast<size_t>(k.line_slots) * es;
    if (lds > kLdsLimit)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "beam line exceeds the LDS limit"); // not reachable: the chunk table keeps every line inside
    if (int rc = with_kernel(precision, ba.complex_in, [&](auto r, auto cplx) {
            hipLaunchKernelGGL((sdsp_beam_kernel<decltype(r), decltype(cplx)::value>), grid, dim3(kThreads), lds, stream, k);
            return static_cast<int>(SDSP_HIP_OK);
        }))
        return rc;
    return launch_status("beam");
}
} // namespace sdsp_hip
