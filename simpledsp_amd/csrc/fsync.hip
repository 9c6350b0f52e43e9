// fsync.hip -- streaming frame synchroniser banks (sdsp_hip_fsync_*): the attached sync marker found at any
// bit offset and in either polarity, a SEARCH / VERIFY / LOCK machine with a flywheel per channel, and the frames behind accepted
// markers cut out, packed most significant bit first, with the inversion and the pseudo-random sequence removed.  Integers only: both
// variants give the bits, records and state of the contract in include/sdsp_hip.h (tests/fsync_ref.py).
//
// Variant 0 is five plain launches over a packed working row per channel in the plan's workspace.  Word j of the row holds the stream
// bits [32 (Wb + j), 32 (Wb + j + 1)), the oldest lowest, with Wb = max(0, seen / 32 - (HW - 1)): the state's ring of the last HW
// words in front, the call's bits behind, two zero words at the end so that every funnel shift finds its neighbours.
//   pack       BYTES: a wave turns 64 bytes into two words by a ballot; PACKED: the words are copied (seen is a multiple of 32)
//   correlate  a thread per word: 32 windows by v_alignbit, XOR with the bit-reversed marker, one popcount for both polarities,
//              one hit word per polarity
//   walk       a wave per channel: SEARCH is a find-first over 64 hit words per round (ballot, then ffs), VERIFY and LOCK one bit
//              test per L; writes the records and the machine's state
//   extract    a thread per (row, frame, four bytes): v_alignbit, bit reverse, byte swap, XOR polarity and pn
//   carry      the last HW words of the row back into the ring
// Variant 1 is one thread per channel, bit by bit from the ring and the input, in one launch.
#include "stream_dev.h"

#include <algorithm>

namespace sdsp_hip
{
namespace
{
enum { kMode = 0, kPol = 1, kCount = 2, kMisses = 3, kPending = 4, kPendInfo = 5, kNext = 6, kSeen = 8, kPendPos = 10, kRecWords = 16 };
enum { kSearch = 0, kVerify = 1, kLock = 2 };

__device__ __forceinline__ uint64_t ld64(const uint32_t *p) { return static_cast<uint64_t>(p[0]) | (static_cast<uint64_t>(p[1]) << 32); }
__device__ __forceinline__ void st64(uint32_t *p, uint64_t v)
{
    p[0] = static_cast<uint32_t>(v);
    p[1] = static_cast<uint32_t>(v >> 32);
}
// first word of the working row: the ring's HW - 1 whole words in front of the one that holds bit `seen`
__device__ __forceinline__ uint64_t first_word(uint64_t seen, uint32_t HW) { return (seen >> 5) >= HW - 1 ? (seen >> 5) - (HW - 1) : 0; }

// the M-bit window at bit offset r of a working row, the first bit lowest, against the bit-reversed marker
__device__ __forceinline__ uint32_t window_distance(const uint32_t *wk, uint64_t r, const fsync_args &a)
{
    const uint32_t j = static_cast<uint32_t>(r >> 5), b = static_cast<uint32_t>(r & 31);
    const uint32_t lo = __funnelshift_r(wk[j], wk[j + 1], b);
    if (a.M <= 32)
        return __popc((lo ^ a.mrev_lo) & (0xffffffffu >> (32 - a.M)));
    const uint32_t hi = __funnelshift_r(wk[j + 1], wk[j + 2], b);
    return __popc(lo ^ a.mrev_lo) + __popc((hi ^ a.mrev_hi) & (0xffffffffu >> (64 - a.M)));
}

// ---- variant 0, stage 1a: the working row
__global__ __launch_bounds__(256) void sdsp_fsync_pack_words_kernel(fsync_args a, uint32_t words)
{
    const uint64_t id = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const uint64_t c = id / words;
    if (c >= a.channels)
        return;
    const uint32_t j = static_cast<uint32_t>(id % words);
    const uint64_t seen = ld64(a.state + c * kRecWords + kSeen), W = first_word(seen, a.HW) + j, in_words = a.nbits >> 5;
    uint32_t v = 0;
    if (W < (seen >> 5))
        v = a.ring[c * a.HW + W % a.HW];
    else if (W - (seen >> 5) < in_words)
        v = static_cast<const uint32_t *>(a.in)[c * in_words + (W - (seen >> 5))];
    a.work[c * a.RW + j] = v;
    if (j == 0)
        a.ws_seen[c] = seen;
}

__global__ __launch_bounds__(256) void sdsp_fsync_pack_bytes_kernel(fsync_args a, uint32_t pairs)
{
    const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * 4 + threadIdx.x / 64;
    const uint64_t c = wave / pairs;
    if (c >= a.channels) // the whole wave leaves together
        return;
    const uint32_t jj = static_cast<uint32_t>(wave % pairs), lane = threadIdx.x & 63;
    const uint64_t seen = ld64(a.state + c * kRecWords + kSeen);
    const uint64_t p = (first_word(seen, a.HW) + 2ull * jj) * 32 + lane;
    bool bit = false;
    if (p < seen)
        bit = (a.ring[c * a.HW + (p >> 5) % a.HW] >> (p & 31)) & 1u;
    else if (p - seen < a.nbits)
        bit = static_cast<const uint8_t *>(a.in)[c * a.nbits + (p - seen)] != 0;
    const uint64_t m = __ballot(bit);
    if (lane == 0) {
        a.work[c * a.RW + 2 * jj] = static_cast<uint32_t>(m);
        a.work[c * a.RW + 2 * jj + 1] = static_cast<uint32_t>(m >> 32);
        if (jj == 0)
            a.ws_seen[c] = seen;
    }
}

// ---- stage 1b: one hit word per polarity
__global__ __launch_bounds__(256) void sdsp_fsync_correlate_kernel(fsync_args a, uint32_t words)
{
    const uint64_t id = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const uint64_t c = id / words;
    if (c >= a.channels)
        return;
    const uint32_t j = static_cast<uint32_t>(id % words);
    const uint64_t seen = a.ws_seen[c], total = seen + a.nbits, p0 = (first_word(seen, a.HW) + j) * 32;
    const uint32_t *wk = a.work + c * a.RW;
    uint32_t hn = 0, hi = 0;
    if (p0 + a.M <= total) {
        const uint32_t w0 = wk[j], w1 = wk[j + 1], w2 = a.M > 32 ? wk[j + 2] : 0;
        const uint32_t mlo = a.M >= 32 ? 0xffffffffu : (1u << a.M) - 1, mhi = a.M > 32 ? 0xffffffffu >> (64 - a.M) : 0;
        // positions of this word that may be examined: p + M <= total
        const uint64_t room = total - a.M - p0 + 1;
        const uint32_t nb = room >= 32 ? 32 : static_cast<uint32_t>(room);
        for (uint32_t b = 0; b < nb; b++) {
            uint32_t d = __popc((__funnelshift_r(w0, w1, b) ^ a.mrev_lo) & mlo);
            if (a.M > 32)
                d += __popc((__funnelshift_r(w1, w2, b) ^ a.mrev_hi) & mhi);
            hn |= (d <= a.tol ? 1u : 0u) << b;
            hi |= (a.either && a.M - d <= a.tol ? 1u : 0u) << b;
        }
    }
    a.hitn[c * a.RW + j] = hn;
    a.hiti[c * a.RW + j] = hi;
}

// ---- stage 2: the machine, a wave per channel; every lane carries the same state, lane 0 stores
__global__ __launch_bounds__(256) void sdsp_fsync_walk_kernel(fsync_args a)
{
    const uint64_t c = static_cast<uint64_t>(blockIdx.x) * 4 + threadIdx.x / 64;
    if (c >= a.channels)
        return;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t *st = a.state + c * kRecWords;
    const uint32_t *wk = a.work + c * a.RW, *hn = a.hitn + c * a.RW, *hi = a.hiti + c * a.RW;
    const uint64_t seen = a.ws_seen[c], total = seen + a.nbits, base = first_word(seen, a.HW) * 32;
    const uint32_t M = a.M, L = a.L;
    uint32_t mode = st[kMode], pol = st[kPol], count = st[kCount], misses = st[kMisses], pending = st[kPending], pinfo = st[kPendInfo];
    uint64_t p = ld64(st + kNext), ppos = ld64(st + kPendPos);
    uint32_t k = 0;

    auto record = [&](uint64_t pos, uint32_t info) {
        if (lane == 0 && k < a.maxf) {
            a.rec_pos[c * a.maxf + k] = pos;
            a.rec_info[c * a.maxf + k] = info;
            if (a.pos)
                a.pos[c * a.maxf + k] = pos;
            if (a.info)
                a.info[c * a.maxf + k] = info;
        }
        k++;
    };
    auto accept = [&](uint64_t pos, uint32_t fly) {
        const uint32_t d = window_distance(wk, pos - base, a);
        const uint32_t info = (pol ? M - d : d) | (pol << 8) | (fly << 9);
        if (pos + L <= total)
            record(pos, info);
        else {
            pending = 1;
            ppos = pos;
            pinfo = info;
        }
    };
    auto hit = [&](const uint32_t *h, uint64_t pos) { return (h[(pos - base) >> 5] >> ((pos - base) & 31)) & 1u; };

    if (pending && ppos + L <= total) {
        record(ppos, pinfo);
        pending = 0;
    }
    while (p + M <= total) {
        if (mode == kSearch) {
            const uint64_t r = p - base, j0 = r >> 5, jlast = (total - M - base) >> 5, j = j0 + lane;
            uint32_t wn = 0, wi = 0;
            if (j <= jlast) {
                wn = hn[j];
                wi = hi[j];
            }
            if (lane == 0) {
                wn &= 0xffffffffu << (r & 31);
                wi &= 0xffffffffu << (r & 31);
            }
            const uint64_t any = __ballot((wn | wi) != 0);
            if (!any) {
                p = std::min<uint64_t>(base + (j0 + 64) * 32, total - M + 1);
                continue;
            }
            const int first = __ffsll(static_cast<unsigned long long>(any)) - 1;
            wn = __shfl(wn, first);
            wi = __shfl(wi, first);
            const uint32_t b = __ffs(wn | wi) - 1;
            p = base + (j0 + first) * 32 + b;
            pol = (wn >> b) & 1u ? 0 : 1;
            count = misses = 0;
            if (a.V == 0) {
                mode = kLock;
                accept(p, 0);
            } else
                mode = kVerify;
            p += L;
        } else if (mode == kVerify) {
            if (hit(pol ? hi : hn, p)) {
                if (++count == a.V) {
                    mode = kLock;
                    accept(p, 0);
                }
                p += L;
            } else {
                mode = kSearch;
                p = p - L + 1;
            }
        } else {
            if (hit(pol ? hi : hn, p)) {
                misses = 0;
                accept(p, 0);
                p += L;
            } else if (++misses > a.F)
                mode = kSearch;
            else {
                accept(p, 1);
                p += L;
            }
        }
    }
    if (lane == 0) {
        st[kMode] = mode;
        st[kPol] = pol;
        st[kCount] = count;
        st[kMisses] = misses;
        st[kPending] = pending;
        st[kPendInfo] = pinfo;
        st64(st + kNext, p);
        st64(st + kSeen, total);
        st64(st + kPendPos, ppos);
        a.rec_cnt[c] = k;
        a.counts[c] = k;
    }
}

// ---- stage 3: four payload bytes per thread
__global__ __launch_bounds__(256) void sdsp_fsync_extract_kernel(fsync_args a, uint32_t groups)
{
    const uint64_t id = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const uint64_t fr = id / groups; // c maxf + k
    if (fr >= a.channels * a.maxf)
        return;
    const uint32_t g = static_cast<uint32_t>(id % groups);
    const uint64_t c = fr / a.maxf, k = fr % a.maxf;
    if (k >= a.rec_cnt[c])
        return;
    const uint32_t *wk = a.work + c * a.RW;
    const uint64_t q = a.rec_pos[fr] + a.M + 32ull * g - first_word(a.ws_seen[c], a.HW) * 32;
    const uint32_t j = static_cast<uint32_t>(q >> 5), b = static_cast<uint32_t>(q & 31);
    uint32_t v = __builtin_bswap32(__brev(__funnelshift_r(wk[j], wk[j + 1], b))); // first bit -> bit 7 of byte 0
    if (a.rec_info[fr] & 0x100)
        v = ~v;
    if (a.pnw)
        v ^= a.pnw[g];
    uint8_t *dst = a.out + fr * a.P + 4ull * g;
    const uint32_t nb = std::min<uint32_t>(4, a.P - 4 * g);
    if (nb == 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0)
        *reinterpret_cast<uint32_t *>(dst) = v;
    else
        for (uint32_t i = 0; i < nb; i++)
            dst[i] = static_cast<uint8_t>(v >> (8 * i));
}

// ---- the carry: the words that hold new bits, at most the last HW, back into the ring
__global__ __launch_bounds__(256) void sdsp_fsync_carry_kernel(fsync_args a)
{
    const uint64_t id = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const uint64_t c = id / a.HW;
    if (c >= a.channels)
        return;
    const uint64_t t = id % a.HW, seen = a.ws_seen[c], end = (seen + a.nbits + 31) >> 5;
    if (t >= end)
        return;
    const uint64_t W = end - 1 - t;
    if (W >= (seen >> 5))
        a.ring[c * a.HW + W % a.HW] = a.work[c * a.RW + (W - first_word(seen, a.HW))];
}

// ---- variant 1: a thread per channel, bit by bit
__global__ __launch_bounds__(64) void sdsp_fsync_plain_kernel(fsync_args a)
{
    const uint64_t c = static_cast<uint64_t>(blockIdx.x) * 64 + threadIdx.x;
    if (c >= a.channels)
        return;
    uint32_t *st = a.state + c * kRecWords, *ring = a.ring + c * a.HW;
    const uint64_t seen = ld64(st + kSeen), total = seen + a.nbits;
    const uint32_t M = a.M, L = a.L, HW = a.HW;
    const uint64_t marker_rev = static_cast<uint64_t>(a.mrev_lo) | (static_cast<uint64_t>(a.mrev_hi) << 32);
    const uint64_t mmask = M == 64 ? ~0ull : (1ull << M) - 1;
    uint32_t mode = st[kMode], pol = st[kPol], count = st[kCount], misses = st[kMisses], pending = st[kPending], pinfo = st[kPendInfo];
    uint64_t p = ld64(st + kNext), ppos = ld64(st + kPendPos);
    uint32_t k = 0;

    auto bit = [&](uint64_t q) -> uint64_t {
        if (q < seen)
            return (ring[(q >> 5) % HW] >> (q & 31)) & 1u;
        const uint64_t i = q - seen;
        if (a.packed)
            return (static_cast<const uint32_t *>(a.in)[c * (a.nbits >> 5) + (i >> 5)] >> (i & 31)) & 1u;
        return static_cast<const uint8_t *>(a.in)[c * a.nbits + i] != 0;
    };
    auto window = [&](uint64_t q) {
        uint64_t w = 0;
        for (uint32_t i = 0; i < M; i++)
            w |= bit(q + i) << i;
        return w;
    };
    auto distance = [&](uint64_t w) { return static_cast<uint32_t>(__popcll((w ^ marker_rev) & mmask)); };
    auto emit = [&](uint64_t pos, uint32_t info) {
        if (k < a.maxf) {
            const uint64_t fr = c * a.maxf + k;
            if (a.pos)
                a.pos[fr] = pos;
            if (a.info)
                a.info[fr] = info;
            if (a.out)
                for (uint32_t i = 0; i < a.P; i++) {
                    uint32_t v = 0;
                    for (uint32_t b = 0; b < 8; b++)
                        v = (v << 1) | static_cast<uint32_t>(bit(pos + M + 8ull * i + b));
                    if (info & 0x100)
                        v ^= 0xff;
                    if (a.pnw)
                        v ^= reinterpret_cast<const uint8_t *>(a.pnw)[i];
                    a.out[fr * a.P + i] = static_cast<uint8_t>(v);
                }
        }
        k++;
    };
    auto accept = [&](uint64_t pos, uint32_t d, uint32_t fly) {
        const uint32_t info = (pol ? M - d : d) | (pol << 8) | (fly << 9);
        if (pos + L <= total)
            emit(pos, info);
        else {
            pending = 1;
            ppos = pos;
            pinfo = info;
        }
    };

    if (pending && ppos + L <= total) {
        emit(ppos, pinfo);
        pending = 0;
    }
    bool have = false; // w is the window at p (SEARCH slides it by one bit)
    uint64_t w = 0;
    while (p + M <= total) {
        if (!have)
            w = window(p);
        have = false;
        const uint32_t d = distance(w);
        if (mode == kSearch) {
            const bool n = d <= a.tol, inv = a.either && M - d <= a.tol;
            if (n || inv) {
                pol = n ? 0 : 1;
                count = misses = 0;
                if (a.V == 0) {
                    mode = kLock;
                    accept(p, d, 0);
                } else
                    mode = kVerify;
                p += L;
            } else {
                p += 1;
                if (p + M <= total) {
                    w = (w >> 1) | (bit(p + M - 1) << (M - 1));
                    have = true;
                }
            }
        } else {
            const bool h = (pol ? M - d : d) <= a.tol;
            if (mode == kVerify) {
                if (h) {
                    if (++count == a.V) {
                        mode = kLock;
                        accept(p, d, 0);
                    }
                    p += L;
                } else {
                    mode = kSearch;
                    p = p - L + 1;
                }
            } else if (h) {
                misses = 0;
                accept(p, d, 0);
                p += L;
            } else if (++misses > a.F)
                mode = kSearch;
            else {
                accept(p, d, 1);
                p += L;
            }
        }
    }
    // the ring: the words that hold new bits, at most the last HW, in ascending order (the first may hold old bits too, and is read
    // before it is written)
    const uint64_t end = (total + 31) >> 5;
    uint64_t W = seen >> 5;
    if (end > HW && end - HW > W)
        W = end - HW;
    for (; W < end; W++) {
        uint32_t v = 0;
        for (uint32_t b = 0; b < 32; b++) {
            const uint64_t q = W * 32 + b;
            if (q < total)
                v |= static_cast<uint32_t>(bit(q)) << b;
        }
        ring[W % HW] = v;
    }
    st[kMode] = mode;
    st[kPol] = pol;
    st[kCount] = count;
    st[kMisses] = misses;
    st[kPending] = pending;
    st[kPendInfo] = pinfo;
    st64(st + kNext, p);
    st64(st + kSeen, total);
    st64(st + kPendPos, ppos);
    a.counts[c] = k;
}
} // namespace

const char *fsync_kernel_for(int variant) { return variant == 1 ? "sdsp_fsync_plain_kernel" : "sdsp_fsync_walk_kernel"; }

uint32_t fsync_ring_words(uint32_t M, uint32_t P) { return (M + 8 * P + M + 31) / 32 + 1; }

uint64_t fsync_row_words(uint32_t M, uint32_t P, uint64_t nbits) { return (fsync_ring_words(M, P) + (nbits + 31) / 32 + 2 + 1) / 2 * 2; }

uint64_t fsync_launches(int variant) { return variant == 1 ? 1 : 5; }

int launch_fsync(const fsync_args &a, int variant, void *stream_v)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    dim3 grid;
    if (variant == 1) {
        if (int rc = grid_of_blocks((a.channels + 63) / 64, "fsync", &grid))
            return rc;
        hipLaunchKernelGGL(sdsp_fsync_plain_kernel, grid, dim3(64), 0, stream, a);
        return launch_status("fsync");
    }
    const uint32_t words = static_cast<uint32_t>(fsync_row_words(a.M, a.P, a.nbits)); // of this call: at most the plan's RW
    if (a.packed) {
        if (int rc = grid_for(a.channels * words, "fsync", &grid))
            return rc;
        hipLaunchKernelGGL(sdsp_fsync_pack_words_kernel, grid, dim3(kThreads), 0, stream, a, words);
    } else {
        if (int rc = grid_of_blocks((a.channels * (words / 2) + 3) / 4, "fsync", &grid))
            return rc;
        hipLaunchKernelGGL(sdsp_fsync_pack_bytes_kernel, grid, dim3(kThreads), 0, stream, a, words / 2);
    }
    if (int rc = grid_for(a.channels * (words - 2), "fsync", &grid))
        return rc;
    hipLaunchKernelGGL(sdsp_fsync_correlate_kernel, grid, dim3(kThreads), 0, stream, a, words - 2);
    if (int rc = grid_of_blocks((a.channels + 3) / 4, "fsync", &grid))
        return rc;
    hipLaunchKernelGGL(sdsp_fsync_walk_kernel, grid, dim3(kThreads), 0, stream, a);
    const uint32_t groups = (a.P + 3) / 4;
    if (a.out && a.maxf) {
        if (int rc = grid_for(a.channels * a.maxf * groups, "fsync", &grid))
            return rc;
        hipLaunchKernelGGL(sdsp_fsync_extract_kernel, grid, dim3(kThreads), 0, stream, a, groups);
    }
    if (int rc = grid_for(a.channels * a.HW, "fsync", &grid))
        return rc;
    hipLaunchKernelGGL(sdsp_fsync_carry_kernel, grid, dim3(kThreads), 0, stream, a);
    return launch_status("fsync");
}
} // namespace sdsp_hip
