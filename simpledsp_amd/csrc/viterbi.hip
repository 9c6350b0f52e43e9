// viterbi.hip -- streaming soft-decision Viterbi decoder banks for rate-1/n convolutional codes (sdsp_hip_viterbi_*, DESIGN.md
// section 5.33).  The contract is the comment in front of sdsp_hip_viterbi_plan_create in include/sdsp_hip.h: integer branch and path
// metrics that wrap, the decision d = (int32)(a1 - a0) > 0, a block-aligned traceback of depth D that emits B bits at a time, and one
// state buffer (metrics, the count of steps held, the decision words of the last Dr steps) that both kernels read and write.
//
// sdsp_viterbi_wave_kernel (variant 0, K = 7): one wave per channel, lane = state.  The two predecessor metrics of a lane come by two
// ds_bpermute, the branch metrics from the step's soft values (staged through LDS as int8, picked up one per lane for eight steps and
// read with v_readlane) times per-lane signs.  The 64 decisions of a step are one ballot word; the words of 32 steps gather in lanes
// 0 .. 31 of a register pair and go to the wave's LDS ring in one store.  After the steps of a chunk lane j walks the traceback of the
// chunk's block j, so the tracebacks run side by side; the bits go through LDS and leave in lane order.  No workgroup barrier: the
// waves of a workgroup share nothing but the launch.
// sdsp_viterbi_plain_kernel (variant 1, every K): a workgroup of S threads per channel, the metrics in two LDS arrays that swap per
// step with one barrier, the soft values read from global memory, the best state by a scan on one thread.  The ring lies in LDS, or in
// a plan-owned buffer in global memory where K = 9 with a long traceback does not fit.
#include "stream_dev.h"

#include <algorithm>

namespace sdsp_hip
{
namespace
{
constexpr uint32_t kLanes = 64;
constexpr uint32_t kMaxWaves = 4;          // waves per workgroup of the wave kernel
constexpr uint32_t kWaveBudget = 5120;     // LDS bytes per wave that keep 32 waves on a CU (160 KiB / 32)
constexpr uint32_t kLdsLimit = 160 * 1024; // one workgroup's most
constexpr uint32_t kMaxChunkBlocks = 64;   // blocks per chunk: one traceback per lane

struct vit_kargs {
    const void *in;
    void *out;
    uint32_t *metrics;
    uint32_t *filled;
    uint64_t *hist;
    uint64_t *ring_ws; // plain kernel: the ring in global memory, or null for LDS
    uint64_t channels;
    uint32_t steps, n, S, B, D, Dr, C, Rg, r; // C: steps per chunk; Rg = Dr + C ring steps; r = (D - 1) % B
    uint32_t grev[3];                         // generators with their K bits reversed: bit i multiplies the input of i steps ago
    uint32_t waves, wave_bytes, q_off, outw_off;
    float scale;
    int packed;
};

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int quant(int8_t x, float) { return x < -127 ? -127 : x; }
// the one floating-point product of the bank: fl32(x scale), to the nearest integer with ties to even, clamped; NaN is an erasure
__device__ __forceinline__ int quant(float x, float scale)
{
    const float y = rintf(x * scale);
    return y != y ? 0 : static_cast<int>(fminf(fmaxf(y, -127.0f), 127.0f));
}

// +1 where the branch (register r: input of i steps ago in bit i) sends coded bit 0 through generator g, -1 where it sends 1
__device__ __forceinline__ int branch_sign(uint32_t grev, uint32_t reg) { return (__popc(grev & reg) & 1) ? -1 : 1; }

// 16 bytes of int8 with every -128 made -127: 0x80 in exactly the bytes that are 0x80, shifted down to their bit 0
__device__ __forceinline__ uint32_t fix4(uint32_t x)
{
    const uint32_t t = x ^ 0x80808080u;
    const uint32_t z = ~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t | 0x7f7f7f7fu);
    return x | (z >> 7);
}

// `count` soft values from g into lq[a0 ..] as int8, a0 = the element's place inside its 16 global bytes, so that the aligned
// 16-byte pieces of the row land on aligned LDS addresses; the head in front of the first piece and the tail go element-wise
template <typename in_t> __device__ __forceinline__ uint32_t stage(const in_t *g, uint32_t count, int8_t *lq, uint32_t lane, float scale)
{
    constexpr uint32_t P = 16 / sizeof(in_t);
    const uint32_t a0 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(g) / sizeof(in_t)) % P;
    const uint32_t head = min(count, (P - a0) % P);
    const uint32_t pieces = (count - head) / P;
    int8_t *dst = lq + a0;
    for (uint32_t e = lane; e < head; e += kLanes)
        dst[e] = static_cast<int8_t>(quant(g[e], scale));
    for (uint32_t k = lane; k < pieces; k += kLanes) {
        const uint32_t e = head + k * P;
        if constexpr (sizeof(in_t) == 1) {
            uint4 v = *reinterpret_cast<const uint4 *>(g + e);
            v.x = fix4(v.x);
            v.y = fix4(v.y);
            v.z = fix4(v.z);
            v.w = fix4(v.w);
            *reinterpret_cast<uint4 *>(dst + e) = v;
        } else {
            const float4 v = *reinterpret_cast<const float4 *>(g + e);
            const uint32_t w = (static_cast<uint32_t>(quant(v.x, scale)) & 0xffu) | ((static_cast<uint32_t>(quant(v.y, scale)) & 0xffu) << 8)
                               | ((static_cast<uint32_t>(quant(v.z, scale)) & 0xffu) << 16) | ((static_cast<uint32_t>(quant(v.w, scale)) & 0xffu) << 24);
            *reinterpret_cast<uint32_t *>(dst + e) = w;
        }
    }
    for (uint32_t e = head + pieces * P + lane; e < count; e += kLanes)
        dst[e] = static_cast<int8_t>(quant(g[e], scale));
    return a0;
}

// One block's traceback.  idx: the ring slot of step e, s: the best state of step e.  D steps are walked and dropped, then B steps
// are walked and their bits (bit 0 of the state) packed, least significant bit = the oldest step, into outw[0 .. B / 32).
__device__ __forceinline__ void traceback(const uint64_t *ring, uint32_t Rg, uint32_t W, uint32_t idx, uint32_t s, uint32_t D, uint32_t B,
                                          uint32_t half, uint32_t *outw)
{
    auto back = [&]() {
        const uint64_t word = ring[idx * W + (s >> 6)];
        s = (s >> 1) + (static_cast<uint32_t>(word >> (s & 63)) & 1u) * half;
        idx = idx ? idx - 1 : Rg - 1;
    };
    for (uint32_t i = 0; i < D; i++)
        back();
    for (int w = static_cast<int>(B / 32) - 1; w >= 0; w--) {
        uint32_t acc = 0;
        for (int b = 31; b >= 0; b--) {
            acc |= (s & 1u) << b;
            back();
        }
        outw[w] = acc;
    }
}

// the chunk's decoded bits from outw to the row: bytes, or the words themselves
__device__ __forceinline__ void write_bits(const vit_kargs &a, uint64_t ch, uint32_t t0, uint32_t cs, const uint32_t *outw, uint32_t tid,
                                           uint32_t threads)
{
    if (a.packed) {
        uint32_t *o = static_cast<uint32_t *>(a.out) + ch * (a.steps / 32) + t0 / 32;
        for (uint32_t w = tid; w < cs / 32; w += threads)
            o[w] = outw[w];
    } else {
        uint8_t *o = static_cast<uint8_t *>(a.out) + ch * a.steps + t0;
        for (uint32_t e = tid; e < cs; e += threads)
            o[e] = static_cast<uint8_t>((outw[e >> 5] >> (e & 31)) & 1u);
    }
}

template <int N, typename in_t> __global__ __launch_bounds__(kMaxWaves *kLanes, 8) void sdsp_viterbi_wave_kernel(vit_kargs a)
{
    extern __shared__ __align__(16) unsigned char vit_lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t ch = static_cast<uint64_t>(blockIdx.x) * a.waves + wave;
    if (wave >= a.waves || ch >= a.channels)
        return;
    unsigned char *base = vit_lds + wave * a.wave_bytes;
    uint64_t *ring = reinterpret_cast<uint64_t *>(base);
    int8_t *lq = reinterpret_cast<int8_t *>(base + a.q_off);
    uint32_t *outw = reinterpret_cast<uint32_t *>(base + a.outw_off);

    // lane = new state s': predecessors p0 = s' >> 1 and p0 + 32, input bit s' & 1
    const uint32_t p0 = lane >> 1, reg0 = lane, reg1 = lane | 64u; // (p << 1) | b for p0 and p0 + 32
    const int addr0 = static_cast<int>(p0 * 4), addr1 = static_cast<int>((p0 + 32) * 4);
    int s0[N], s1[N];
#pragma unroll
    for (int j = 0; j < N; j++) {
        s0[j] = branch_sign(a.grev[j], reg0);
        s1[j] = branch_sign(a.grev[j], reg1);
    }

    uint32_t m = a.metrics[ch * 64 + lane];
    const uint32_t filled = a.filled[ch];
    for (uint32_t i = lane; i < a.Dr; i += kLanes)
        ring[i] = a.hist[ch * a.Dr + i];
    uint32_t widx = a.Dr; // the ring slot of the next step; Rg > Dr
    const in_t *row = static_cast<const in_t *>(a.in) + ch * a.steps * N;

    for (uint32_t t0 = 0; t0 < a.steps; t0 += a.C) {
        const uint32_t cs = min(a.C, a.steps - t0), nb = cs / a.B;
        const uint32_t q0 = stage(row + static_cast<uint64_t>(t0) * N, cs * N, lq, lane, a.scale);
        wave_lds_sync();
        uint32_t my_best = 0, my_idx = 0;
        const int8_t *qp = lq + q0;
        for (uint32_t blk = 0; blk < nb; blk++) {
            for (uint32_t g = 0; g < a.B; g += 32, qp += 32 * N) {
                // The decision words of the 32 steps gather in two registers, step i in lane i, and go to the ring in
                // one store: a group never wraps, since Dr, the chunk and so the ring are multiples of 32 steps.
                int wlo = 0, whi = 0;
                // eight steps unrolled at a time: all 32 would keep 64 branch metrics alive and spill
#pragma nounroll
                for (int i8 = 0; i8 < 32; i8 += 8) {
                    // the soft values of the eight steps, one per lane, then read by v_readlane at constant lanes
                    const int v = lane < 8 * N ? qp[i8 * N + static_cast<int>(lane)] : 0;
#pragma unroll
                    for (int ii = 0; ii < 8; ii++) {
                        const int i = i8 + ii;
                        int q[N];
#pragma unroll
                        for (int j = 0; j < N; j++)
                            q[j] = __builtin_amdgcn_readlane(v, ii * N + j);
                        int bm0 = __mul24(q[0], s0[0]), bm1 = __mul24(q[0], s1[0]); // |q| <= 127, the signs are +-1: 24 bits do
#pragma unroll
                        for (int j = 1; j < N; j++) {
                            bm0 += __mul24(q[j], s0[j]);
                            bm1 += __mul24(q[j], s1[j]);
                        }
                        const uint32_t c0 = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(addr0, static_cast<int>(m))) + static_cast<uint32_t>(bm0);
                        const uint32_t c1 = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(addr1, static_cast<int>(m))) + static_cast<uint32_t>(bm1);
                        const bool d = static_cast<int32_t>(c1 - c0) > 0;
                        m = d ? c1 : c0;
                        const uint64_t word = __ballot(d);
                        wlo = lane == static_cast<uint32_t>(i) ? static_cast<int>(static_cast<uint32_t>(word)) : wlo;
                        whi = lane == static_cast<uint32_t>(i) ? static_cast<int>(static_cast<uint32_t>(word >> 32)) : whi;
                        if (g + static_cast<uint32_t>(i) == a.r) { // the step that decides a block: the lowest state of the largest m[s] - m[0]
                            const int rel = static_cast<int32_t>(m - static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(m))));
                            int mx = rel;
#pragma unroll
                            for (int o = 32; o >= 1; o >>= 1)
                                mx = max(mx, __shfl_xor(mx, o));
                            const uint32_t best = static_cast<uint32_t>(__builtin_ctzll(__ballot(rel == mx)));
                            if (lane == blk) {
                                my_best = best;
                                my_idx = widx + static_cast<uint32_t>(i);
                            }
                        }
                    }
                }
                if (lane < 32)
                    ring[widx + lane] = (static_cast<uint64_t>(static_cast<uint32_t>(whi)) << 32) | static_cast<uint32_t>(wlo);
                widx = widx + 32 == a.Rg ? 0 : widx + 32;
            }
        }
        wave_lds_sync();
        if (lane < nb) {
            uint32_t *w = outw + lane * (a.B / 32);
            if (static_cast<uint64_t>(filled) + t0 + lane * a.B >= a.Dr) {
                traceback(ring, a.Rg, 1, my_idx, my_best, a.D, a.B, 32, w);
            } else { // the first Dr outputs of a stream
                for (uint32_t i = 0; i < a.B / 32; i++)
                    w[i] = 0;
            }
        }
        wave_lds_sync();
        write_bits(a, ch, t0, cs, outw, lane, kLanes);
        wave_lds_sync();
    }

    a.metrics[ch * 64 + lane] = m;
    if (lane == 0)
        a.filled[ch] = static_cast<uint32_t>(min(static_cast<uint64_t>(filled) + a.steps, static_cast<uint64_t>(a.Dr)));
    // the last Dr steps, oldest first: they end in front of widx
    uint32_t src = widx + (a.Rg - a.Dr);
    src = src >= a.Rg ? src - a.Rg : src;
    for (uint32_t i = lane; i < a.Dr; i += kLanes) {
        uint32_t k = src + i;
        k = k >= a.Rg ? k - a.Rg : k;
        a.hist[ch * a.Dr + i] = ring[k];
    }
}

template <typename in_t> __global__ __launch_bounds__(256) void sdsp_viterbi_plain_kernel(vit_kargs a)
{
    extern __shared__ __align__(16) unsigned char vit_lds[];
    const uint32_t tid = threadIdx.x, S = a.S, W = S > 64 ? S / 64 : 1, half = S / 2, n = a.n;
    const uint64_t ch = blockIdx.x;
    uint32_t *mm = reinterpret_cast<uint32_t *>(vit_lds);        // two arrays of S metrics
    uint32_t *best_s = mm + 2 * S;                               // kMaxChunkBlocks best states
    uint32_t *best_idx = best_s + kMaxChunkBlocks;               // and the ring slots of their steps
    uint32_t *outw = best_idx + kMaxChunkBlocks;                 // C / 32 words
    uint64_t *lds_ring = reinterpret_cast<uint64_t *>(vit_lds + a.q_off); // 8-byte aligned
    uint64_t *ring = a.ring_ws ? a.ring_ws + ch * a.Rg * W : lds_ring;

    const uint32_t pa = tid >> 1, pb = pa + half, rega = tid, regb = tid | S;
    int sa[3], sb[3];
    for (uint32_t j = 0; j < 3; j++) {
        sa[j] = j < n ? branch_sign(a.grev[j], rega) : 0;
        sb[j] = j < n ? branch_sign(a.grev[j], regb) : 0;
    }

    mm[tid] = a.metrics[ch * S + tid];
    const uint32_t filled = a.filled[ch];
    for (uint32_t i = tid; i < a.Dr * W; i += S)
        ring[i] = a.hist[ch * a.Dr * W + i];
    __syncthreads();
    uint32_t widx = a.Dr, cur = 0;
    const in_t *row = static_cast<const in_t *>(a.in) + ch * a.steps * n;

    for (uint32_t t0 = 0; t0 < a.steps; t0 += a.C) {
        const uint32_t cs = min(a.C, a.steps - t0), nb = cs / a.B;
        for (uint32_t blk = 0; blk < nb; blk++) {
            for (uint32_t ib = 0; ib < a.B; ib++) {
                const in_t *x = row + static_cast<uint64_t>(t0 + blk * a.B + ib) * n;
                int bma = 0, bmb = 0;
                for (uint32_t j = 0; j < n; j++) {
                    const int q = quant(x[j], a.scale);
                    bma += q * sa[j];
                    bmb += q * sb[j];
                }
                const uint32_t *from = mm + cur * S;
                uint32_t *to = mm + (cur ^ 1u) * S;
                const uint32_t ca = from[pa] + static_cast<uint32_t>(bma), cb = from[pb] + static_cast<uint32_t>(bmb);
                const bool d = static_cast<int32_t>(cb - ca) > 0;
                to[tid] = d ? cb : ca;
                const uint64_t word = __ballot(d);
                if ((tid & 63u) == 0)
                    ring[widx * W + (tid >> 6)] = word;
                __syncthreads();
                cur ^= 1u;
                if (ib == a.r && tid == 0) {
                    const uint32_t *now = mm + cur * S;
                    int mx = 0;
                    uint32_t best = 0;
                    for (uint32_t s = 1; s < S; s++) {
                        const int v = static_cast<int32_t>(now[s] - now[0]);
                        if (v > mx) {
                            mx = v;
                            best = s;
                        }
                    }
                    best_s[blk] = best;
                    best_idx[blk] = widx;
                }
                widx = widx + 1 == a.Rg ? 0 : widx + 1;
            }
        }
        __syncthreads();
        for (uint32_t j = tid; j < nb; j += S) {
            uint32_t *w = outw + j * (a.B / 32);
            if (static_cast<uint64_t>(filled) + t0 + j * a.B >= a.Dr) {
                traceback(ring, a.Rg, W, best_idx[j], best_s[j], a.D, a.B, half, w);
            } else {
                for (uint32_t i = 0; i < a.B / 32; i++)
                    w[i] = 0;
            }
        }
        __syncthreads();
        write_bits(a, ch, t0, cs, outw, tid, S);
        __syncthreads();
    }

    a.metrics[ch * S + tid] = mm[cur * S + tid];
    if (tid == 0)
        a.filled[ch] = static_cast<uint32_t>(min(static_cast<uint64_t>(filled) + a.steps, static_cast<uint64_t>(a.Dr)));
    uint32_t src = widx + (a.Rg - a.Dr);
    src = src >= a.Rg ? src - a.Rg : src;
    for (uint32_t i = tid; i < a.Dr * W; i += S) {
        uint32_t k = src + i / W;
        k = k >= a.Rg ? k - a.Rg : k;
        a.hist[ch * a.Dr * W + i] = ring[k * W + i % W];
    }
}

uint32_t align16(uint32_t v) { return (v + 15u) & ~15u; }

std::atomic<uint64_t> g_wave_lds[4], g_plain_lds[2];
} // namespace

const char *viterbi_kernel_for(int variant) { return variant == 1 ? "sdsp_viterbi_plain_kernel" : "sdsp_viterbi_wave_kernel"; }

viterbi_shape viterbi_shape_for(uint32_t k, uint32_t n, uint32_t block, uint32_t dr, int variant)
{
    viterbi_shape s{};
    const uint32_t S = 1u << (k - 1), W = S > 64 ? S / 64 : 1;
    // steps per chunk: what the per-wave budget holds beside the Dr steps in front of it, whole blocks, one at least and 64 at most.
    // Per step: W decision words, and in the wave kernel n staged soft values; one bit of output.
    auto chunk_for = [&](uint32_t per_step_x8, uint32_t fixed) {
        const uint64_t used = static_cast<uint64_t>(dr) * W * 8 + fixed;
        const uint64_t room = kWaveBudget > used ? kWaveBudget - used : 0;
        const uint32_t blocks = static_cast<uint32_t>(room * 8 / per_step_x8 / block);
        return block * std::min(kMaxChunkBlocks, std::max(1u, blocks));
    };
    if (variant == 0) {
        s.chunk = chunk_for(W * 64 + n * 8 + 1, 32);
        s.ring_steps = dr + s.chunk;
        s.q_off = align16(s.ring_steps * 8);
        s.outw_off = s.q_off + align16(s.chunk * n + 16);
        s.wave_bytes = s.outw_off + align16(s.chunk / 8);
        s.waves = std::min(kMaxWaves, kLdsLimit / s.wave_bytes);
        s.threads = s.waves * kLanes;
        s.lds_bytes = s.waves * s.wave_bytes;
        s.ring_in_lds = 1;
        return s;
    }
    const uint32_t fixed = (2 * S + 2 * kMaxChunkBlocks) * 4;
    s.chunk = chunk_for(W * 64 + 1, fixed);
    s.ring_steps = dr + s.chunk;
    s.q_off = align16(fixed + s.chunk / 8); // where the ring starts
    s.ring_in_lds = static_cast<uint64_t>(s.q_off) + static_cast<uint64_t>(s.ring_steps) * W * 8 <= kLdsLimit;
    s.lds_bytes = s.q_off + (s.ring_in_lds ? s.ring_steps * W * 8 : 0);
    s.waves = (S + 63) / 64;
    s.threads = S;
    s.wave_bytes = 0;
    s.outw_off = 0;
    return s;
}

int launch_viterbi(const viterbi_args &va, int variant, void *stream_v)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (!va.in) { // prepare: the dynamic-LDS limit of every kernel on the current device, so that process sets no attribute
        const void *wave[4] = { reinterpret_cast<const void *>(sdsp_viterbi_wave_kernel<2, int8_t>), reinterpret_cast<const void *>(sdsp_viterbi_wave_kernel<3, int8_t>),
                                reinterpret_cast<const void *>(sdsp_viterbi_wave_kernel<2, float>), reinterpret_cast<const void *>(sdsp_viterbi_wave_kernel<3, float>) };
        const void *plain[2] = { reinterpret_cast<const void *>(sdsp_viterbi_plain_kernel<int8_t>), reinterpret_cast<const void *>(sdsp_viterbi_plain_kernel<float>) };
        for (int i = 0; i < 4; i++)
            if (int rc = ensure_dynamic_lds(wave[i], kLdsLimit, g_wave_lds[i]))
                return rc;
        for (int i = 0; i < 2; i++)
            if (int rc = ensure_dynamic_lds(plain[i], kLdsLimit, g_plain_lds[i]))
                return rc;
        return SDSP_HIP_OK;
    }
    const viterbi_shape s = viterbi_shape_for(va.k, va.n, va.block, va.dr, variant);
    vit_kargs k{};
    k.in = va.in;
    k.out = va.out;
    k.metrics = va.metrics;
    k.filled = va.filled;
    k.hist = va.hist;
    k.ring_ws = variant == 1 && !s.ring_in_lds ? va.ring_ws : nullptr;
    k.channels = va.channels;
    k.steps = static_cast<uint32_t>(va.steps);
    k.n = va.n;
    k.S = 1u << (va.k - 1);
    k.B = va.block;
    k.D = va.depth;
    k.Dr = va.dr;
    k.C = s.chunk;
    k.Rg = s.ring_steps;
    k.r = (va.depth - 1) % va.block;
    for (uint32_t j = 0; j < va.n; j++) {
        uint32_t g = 0;
        for (uint32_t b = 0; b < va.k; b++)
            g |= ((va.generators[j] >> b) & 1u) << (va.k - 1 - b);
        k.grev[j] = g;
    }
    k.waves = s.waves;
    k.wave_bytes = s.wave_bytes;
    k.q_off = s.q_off;
    k.outw_off = s.outw_off;
    k.scale = va.scale;
    k.packed = va.out_kind == SDSP_HIP_VITERBI_PACKED;
    const bool f32 = va.in_kind == SDSP_HIP_VITERBI_F32;
    dim3 grid;
    if (variant == 1) {
        if (!s.ring_in_lds && !va.ring_ws)
            return fail(SDSP_HIP_ERR_UNSUPPORTED, "viterbi: the plan holds no ring for the plain kernel");
        if (int rc = grid_of_blocks(va.channels, "viterbi", &grid))
            return rc;
        if (f32)
            hipLaunchKernelGGL(sdsp_viterbi_plain_kernel<float>, grid, dim3(s.threads), s.lds_bytes, stream, k);
        else
            hipLaunchKernelGGL(sdsp_viterbi_plain_kernel<int8_t>, grid, dim3(s.threads), s.lds_bytes, stream, k);
        return launch_status("viterbi");
    }
    if (va.k != 7)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "viterbi: the wave kernel serves K = 7 only");
    if (int rc = grid_of_blocks((va.channels + s.waves - 1) / s.waves, "viterbi", &grid))
        return rc;
    if (va.n == 2) {
        if (f32)
            hipLaunchKernelGGL((sdsp_viterbi_wave_kernel<2, float>), grid, dim3(s.threads), s.lds_bytes, stream, k);
        else
            hipLaunchKernelGGL((sdsp_viterbi_wave_kernel<2, int8_t>), grid, dim3(s.threads), s.lds_bytes, stream, k);
    } else {
        if (f32)
            hipLaunchKernelGGL((sdsp_viterbi_wave_kernel<3, float>), grid, dim3(s.threads), s.lds_bytes, stream, k);
        else
            hipLaunchKernelGGL((sdsp_viterbi_wave_kernel<3, int8_t>), grid, dim3(s.threads), s.lds_bytes, stream, k);
    }
    return launch_status("viterbi");
}
} // namespace sdsp_hip
