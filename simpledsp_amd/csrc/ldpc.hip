// ldpc.hip -- LDPC decoder banks for quasi-cyclic codes, layered normalised / offset min-sum on integers (sdsp_hip_ldpc_*, DESIGN.md
// section 5.37).  The contract is the comment in front of sdsp_hip_ldpc_plan_create in include/sdsp_hip.h; every bit, posterior and
// status both kernels write is the one tests/ldpc_ref.py writes.
//
// Both kernels read the plan's table: rowptr[0 .. mb] and, per entry in ascending block column, (first variable of the block column,
// shift).  The index of the table is the same on every lane, so the loads are scalar.
// sdsp_ldpc_wave_kernel (variant 0): lanes are the checks of a layer.  A wave owns floor(64 / Z) codewords side by side where Z <= 32
// (lane = (codeword, check)), one codeword where Z <= 64, and walks a layer in ceil(Z / 64) pieces above that: the checks of a layer
// touch different variables, so nothing but wave-scope ordering of the LDS accesses between layers is needed, and waves share nothing
// (no barrier, no atomics).  The posteriors L of the wave's codewords lie in LDS as int16, staged with 16-byte loads at the offset the
// input has within 16 bytes, the float quantiser on the way; a check's messages are kept as a record of 8 bytes (the two normalised
// minima, the entry that holds the minimum, the d sign bits) in LDS.  A layer is two passes over the row's entries: the first reads L
// and rebuilds T = L - R from the old record for the minima and the signs, the second reads L again and writes L - R(old) + R(new).
// The rotated index is a compare and a subtract.  The syndrome test is the contract's: one pass over the layers on the final L.
// sdsp_ldpc_plain_kernel (variant 1): a thread per codeword, L (int16) and one int8 message per edge in the plan's global workspace,
// codeword-minor; the message of an entry is chosen by the value of its |T|, not by a stored index.
#include "stream_dev.h"

#include <algorithm>

namespace sdsp_hip
{
namespace
{
constexpr uint32_t kLanes = 64;
constexpr uint32_t kMaxWaves = 4;          // waves per workgroup of the wave kernel, where their LDS fits kSmallLds
constexpr uint32_t kSmallLds = 64 * 1024;  // LDS a workgroup takes without raising the kernel's limit
constexpr uint32_t kCuLds = 160 * 1024;
constexpr uint32_t kSlack = 16;            // int16 elements in front of a wave's image: the input's offset within 16 bytes
constexpr uint32_t kPlainThreads = 64;
constexpr uint64_t kWorkspace = 256ull << 20;
constexpr uint64_t kMaxPiece = 65536;      // codewords of one launch of the plain kernel

struct ldpc_kargs {
    const void *llr;
    void *bits;      // nullable
    int16_t *post;   // nullable
    int32_t *status; // nullable
    const uint32_t *rowptr;
    const uint2 *ent; // x: first variable of the block column, y: shift
    uint64_t codewords;
    uint32_t mb, z, n, m, norm, beta, early, max_iter, out_bits, packed;
    float scale;
    uint32_t group, waves, wave_bytes; // wave kernel: codewords per wave, waves per workgroup, LDS of one wave
    int16_t *ws_l;                     // plain kernel: L[v cap + t]
    int8_t *ws_r;                      // plain kernel: R[e cap + t]
    uint64_t cap;
};

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int quant(int8_t x, float) { return x < -127 ? -127 : x; }
// the one floating-point product of the family: fl32(x scale), to the nearest integer with ties to even, clamped; NaN is an erasure
__device__ __forceinline__ int quant(float x, float scale)
{
    const float y = rintf(x * scale);
    return y != y ? 0 : static_cast<int>(fminf(fmaxf(y, -127.0f), 127.0f));
}

// f(x) = max(((x norm + 8) >> 4) - beta, 0)
__device__ __forceinline__ int normalise(int x, uint32_t norm, uint32_t beta)
{
    return max(((x * static_cast<int>(norm) + 8) >> 4) - static_cast<int>(beta), 0);
}

__device__ __forceinline__ uint32_t rotated(uint32_t i, uint32_t shift, uint32_t z)
{
    const uint32_t s = i + shift;
    return s >= z ? s - z : s;
}

// ---------------------------------------------------------------------------------------------------------------- wave kernel

__device__ __forceinline__ uint32_t pack2(int lo, int hi) { return (static_cast<uint32_t>(lo) & 0xffffu) | (static_cast<uint32_t>(hi) << 16); }
__device__ __forceinline__ int byte_of(uint32_t w, int b) { return static_cast<int8_t>(w >> (8 * b)); }

// `total` soft values from g into the image as int16, at the offset g has within 16 bytes; returns where value 0 landed
template <typename in_t>
__device__ __forceinline__ int16_t *stage_in(int16_t *img, const in_t *g, uint32_t total, float scale, uint32_t lane)
{
    constexpr uint32_t P = 16 / sizeof(in_t); // values of a 16-byte load
    const uint32_t off = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(g) & 15) / sizeof(in_t);
    int16_t *L = img + off;
    const uint32_t head = min((P - off) % P, total);
    const uint32_t nvec = (total - head) / P, tail = head + nvec * P;
    if (lane < head)
        L[lane] = static_cast<int16_t>(quant(g[lane], scale));
    for (uint32_t k = lane; k < nvec; k += kLanes) {
        const uint32_t e = head + k * P;
        if constexpr (sizeof(in_t) == 1) {
            const uint4 x = *reinterpret_cast<const uint4 *>(g + e);
            const uint32_t w[4] = { x.x, x.y, x.z, x.w };
            uint32_t o[8];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                o[2 * q] = pack2(quant(static_cast<int8_t>(byte_of(w[q], 0)), scale), quant(static_cast<int8_t>(byte_of(w[q], 1)), scale));
                o[2 * q + 1] = pack2(quant(static_cast<int8_t>(byte_of(w[q], 2)), scale), quant(static_cast<int8_t>(byte_of(w[q], 3)), scale));
            }
            uint4 *d = reinterpret_cast<uint4 *>(L + e); // off + head is a multiple of 16 values: 32 bytes
            d[0] = make_uint4(o[0], o[1], o[2], o[3]);
            d[1] = make_uint4(o[4], o[5], o[6], o[7]);
        } else {
            const float4 x = *reinterpret_cast<const float4 *>(g + e);
            *reinterpret_cast<uint2 *>(L + e) = make_uint2(pack2(quant(x.x, scale), quant(x.y, scale)), pack2(quant(x.z, scale), quant(x.w, scale)));
        }
    }
    if (tail + lane < total)
        L[tail + lane] = static_cast<int16_t>(quant(g[tail + lane], scale));
    return L;
}

// `total` posteriors from LDS to o (aligned to 2 bytes)
__device__ __forceinline__ void stage_out(int16_t *o, const int16_t *L, uint32_t total, uint32_t lane)
{
    const uint32_t off = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(o) & 15) / 2;
    const uint32_t head = min((8 - off) % 8, total);
    const uint32_t nvec = (total - head) / 8, tail = head + nvec * 8;
    if (lane < head)
        o[lane] = L[lane];
    const bool aligned = (reinterpret_cast<uintptr_t>(L + head) & 15) == 0; // wave-uniform
    for (uint32_t k = lane; k < nvec; k += kLanes) {
        const int16_t *s = L + head + k * 8;
        uint4 x;
        if (aligned)
            x = *reinterpret_cast<const uint4 *>(s);
        else
            __builtin_memcpy(&x, s, 16);
        *reinterpret_cast<uint4 *>(o + head + k * 8) = x;
    }
    if (tail + lane < total)
        o[tail + lane] = L[tail + lane];
}

// the message an entry holds in a record: w = m1 | m2 << 8 | index of the minimum << 16, sg = the sign bits
__device__ __forceinline__ int record_message(uint32_t w, uint32_t sg, uint32_t j)
{
    const int mag = static_cast<int>(j == ((w >> 16) & 0xffu) ? (w >> 8) & 0xffu : w & 0xffu);
    return (sg >> j) & 1u ? -mag : mag;
}

// check i of a layer: L of the codeword, the check's record, the row's d entries
__device__ __forceinline__ void wave_check(int16_t *L, uint2 *rec, const uint2 *__restrict__ ent, uint32_t d, uint32_t i, const ldpc_kargs &a)
{
    const uint2 old = *rec;
    int m1 = 128, m2 = 128;
    uint32_t ix = 0, sig = 0;
    for (uint32_t j = 0; j < d; j++) {
        const uint2 e = ent[j];
        const int t = L[e.x + rotated(i, e.y, a.z)] - record_message(old.x, old.y, j);
        const int mag = min(abs(t), 127);
        sig |= static_cast<uint32_t>(t < 0) << j;
        if (mag < m1) {
            m2 = m1;
            m1 = mag;
            ix = j;
        } else if (mag < m2) {
            m2 = mag;
        }
    }
    const uint32_t mask = d == 32 ? 0xffffffffu : (1u << d) - 1;
    const uint32_t sg = ((__popc(sig) & 1) ? ~sig : sig) & mask; // the signs of the new messages: S xor sigma_j
    const uint32_t w = static_cast<uint32_t>(normalise(m1, a.norm, a.beta)) | (static_cast<uint32_t>(normalise(m2, a.norm, a.beta)) << 8) | (ix << 16);
    *rec = make_uint2(w, sg);
    for (uint32_t j = 0; j < d; j++) {
        const uint2 e = ent[j];
        int16_t *p = L + e.x + rotated(i, e.y, a.z);
        *p = static_cast<int16_t>(*p - record_message(old.x, old.y, j) + record_message(w, sg, j));
    }
}

// the parity of check i on the hard decisions
__device__ __forceinline__ uint32_t wave_parity(const int16_t *L, const uint2 *__restrict__ ent, uint32_t d, uint32_t i, uint32_t z)
{
    uint32_t par = 0;
    for (uint32_t j = 0; j < d; j++) {
        const uint2 e = ent[j];
        par ^= static_cast<uint32_t>(L[e.x + rotated(i, e.y, z)] < 0);
    }
    return par;
}

template <typename in_t> __global__ __launch_bounds__(kMaxWaves *kLanes) void sdsp_ldpc_wave_kernel(ldpc_kargs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t ldpc_lds[];
    const uint32_t lane = threadIdx.x % kLanes, wave = threadIdx.x / kLanes;
    const uint64_t first = (static_cast<uint64_t>(blockIdx.x) * a.waves + wave) * a.group;
    if (first >= a.codewords) // wave-uniform
        return;
    const uint32_t cnt = static_cast<uint32_t>(min(static_cast<uint64_t>(a.group), a.codewords - first));
    uint8_t *mine = ldpc_lds + static_cast<size_t>(wave) * a.wave_bytes;
    int16_t *img = reinterpret_cast<int16_t *>(mine);
    uint2 *recs = reinterpret_cast<uint2 *>(mine + (static_cast<size_t>(a.group) * a.n + kSlack + 7) / 8 * 16);
    const uint32_t n = a.n, m = a.m, z = a.z;
    int16_t *L0 = stage_in(img, static_cast<const in_t *>(a.llr) + first * n, cnt * n, a.scale, lane);
    for (uint32_t k = lane; k < cnt * m; k += kLanes)
        recs[k] = make_uint2(0, 0);
    // lane -> (codeword g of the wave, check i0 of the piece)
    uint32_t g = 0, i0 = lane, pieces = (z + kLanes - 1) / kLanes;
    if (a.group > 1) {
        g = lane / z;
        i0 = lane - g * z;
        pieces = 1;
    }
    const bool active = g < cnt;
    int16_t *L = L0 + (active ? g * n : 0);
    uint2 *rec = recs + (active ? g * m : 0);
    const uint64_t mine_mask = a.group > 1 && active ? ((1ull << z) - 1) << (g * z) : ~0ull;
    wave_lds_sync();

    // the syndrome test of the lane's codeword on the L of this moment
    auto passes = [&]() {
        uint32_t bad = 0;
        for (uint32_t r = 0; r < a.mb; r++) {
            const uint32_t e0 = a.rowptr[r], d = a.rowptr[r + 1] - e0;
            for (uint32_t p = 0; p < pieces; p++) {
                const uint32_t i = i0 + p * kLanes;
                if (active && i < z)
                    bad |= wave_parity(L, a.ent + e0, d, i, z);
            }
        }
        return (__ballot(bad != 0) & mine_mask) == 0;
    };

    int st = passes() ? 0 : -1;
    bool done = !active || (a.early && st == 0);
    for (uint32_t it = 1; it <= a.max_iter; it++) {
        if (__ballot(!done) == 0) // every codeword of the wave has stopped
            break;
        for (uint32_t r = 0; r < a.mb; r++) {
            const uint32_t e0 = a.rowptr[r], d = a.rowptr[r + 1] - e0;
            for (uint32_t p = 0; p < pieces; p++) {
                const uint32_t i = i0 + p * kLanes;
                if (!done && i < z)
                    wave_check(L, rec + r * z + i, a.ent + e0, d, i, a);
            }
            wave_lds_sync();
        }
        if (a.early || it == a.max_iter) {
            const bool ok = passes();
            if (!done) {
                st = ok ? static_cast<int>(it) : -1;
                done = a.early && ok;
            }
        }
    }

    if (a.status && active && i0 == 0)
        a.status[first + g] = st;
    if (a.post)
        stage_out(a.post + first * n, L0, cnt * n, lane);
    if (a.bits) {
        if (a.packed) {
            const uint32_t words = (a.out_bits + 31) / 32;
            uint32_t *o = static_cast<uint32_t *>(a.bits) + first * words;
            for (uint32_t c = 0; c < cnt; c++)
                for (uint32_t b = 0; b < a.out_bits; b += kLanes) {
                    const uint32_t v = b + lane;
                    const uint64_t hard = __ballot(v < a.out_bits && L0[c * n + v] < 0);
                    const uint32_t w = b / 32 + lane;
                    if (lane < 2 && w < words)
                        o[c * words + w] = static_cast<uint32_t>(hard >> (32 * lane));
                }
        } else {
            uint8_t *o = static_cast<uint8_t *>(a.bits) + first * a.out_bits;
            for (uint32_t c = 0; c < cnt; c++)
                for (uint32_t v = lane; v < a.out_bits; v += kLanes)
                    o[c * a.out_bits + v] = L0[c * n + v] < 0;
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- plain kernel

__device__ bool plain_passes(const int16_t *L, const ldpc_kargs &a)
{
    for (uint32_t r = 0; r < a.mb; r++)
        for (uint32_t i = 0; i < a.z; i++) {
            uint32_t par = 0;
            for (uint32_t e = a.rowptr[r]; e < a.rowptr[r + 1]; e++)
                par ^= static_cast<uint32_t>(L[(a.ent[e].x + rotated(i, a.ent[e].y, a.z)) * a.cap] < 0);
            if (par)
                return false;
        }
    return true;
}

template <typename in_t> __global__ __launch_bounds__(kPlainThreads) void sdsp_ldpc_plain_kernel(ldpc_kargs a)
{
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kPlainThreads + threadIdx.x;
    if (t >= a.codewords)
        return;
    const uint64_t cap = a.cap;
    int16_t *L = a.ws_l + t;
    int8_t *R = a.ws_r + t;
    const in_t *x = static_cast<const in_t *>(a.llr) + t * a.n;
    for (uint32_t v = 0; v < a.n; v++)
        L[v * cap] = static_cast<int16_t>(quant(x[v], a.scale));
    const uint64_t edges = static_cast<uint64_t>(a.rowptr[a.mb]) * a.z;
    for (uint64_t e = 0; e < edges; e++)
        R[e * cap] = 0;
    bool ok = plain_passes(L, a);
    int st = ok ? 0 : -1;
    for (uint32_t it = 1; it <= a.max_iter && !(a.early && ok); it++) {
        for (uint32_t r = 0; r < a.mb; r++) {
            const uint32_t e0 = a.rowptr[r], e1 = a.rowptr[r + 1];
            for (uint32_t i = 0; i < a.z; i++) {
                int m1 = 128, m2 = 128;
                uint32_t neg = 0;
                for (uint32_t e = e0; e < e1; e++) {
                    const int tv = L[(a.ent[e].x + rotated(i, a.ent[e].y, a.z)) * cap] - R[(static_cast<uint64_t>(e) * a.z + i) * cap];
                    const int mag = min(abs(tv), 127);
                    neg ^= static_cast<uint32_t>(tv < 0);
                    if (mag < m1) {
                        m2 = m1;
                        m1 = mag;
                    } else if (mag < m2) {
                        m2 = mag;
                    }
                }
                const int f1 = normalise(m1, a.norm, a.beta), f2 = normalise(m2, a.norm, a.beta);
                for (uint32_t e = e0; e < e1; e++) {
                    int16_t *pl = L + (a.ent[e].x + rotated(i, a.ent[e].y, a.z)) * cap;
                    int8_t *pr = R + (static_cast<uint64_t>(e) * a.z + i) * cap;
                    const int tv = *pl - *pr;
                    const int mag = min(abs(tv), 127) == m1 ? f2 : f1; // the minimum of the others; a tie has f1 == f2
                    const int msg = (neg ^ static_cast<uint32_t>(tv < 0)) ? -mag : mag;
                    *pr = static_cast<int8_t>(msg);
                    *pl = static_cast<int16_t>(tv + msg);
                }
            }
        }
        if (a.early || it == a.max_iter) {
            ok = plain_passes(L, a);
            st = ok ? static_cast<int>(it) : -1;
        }
    }
    if (a.status)
        a.status[t] = st;
    if (a.post)
        for (uint32_t v = 0; v < a.n; v++)
            a.post[t * a.n + v] = L[v * cap];
    if (a.bits) {
        if (a.packed) {
            const uint32_t words = (a.out_bits + 31) / 32;
            uint32_t *o = static_cast<uint32_t *>(a.bits) + t * words;
            for (uint32_t w = 0; w < words; w++) {
                uint32_t acc = 0;
                for (uint32_t b = 0; b < 32 && w * 32 + b < a.out_bits; b++)
                    acc |= static_cast<uint32_t>(L[(w * 32 + b) * cap] < 0) << b;
                o[w] = acc;
            }
        } else {
            uint8_t *o = static_cast<uint8_t *>(a.bits) + t * a.out_bits;
            for (uint32_t v = 0; v < a.out_bits; v++)
                o[v] = L[v * cap] < 0;
        }
    }
}

std::atomic<uint64_t> g_wave_lds_done[2];
} // namespace

const char *ldpc_kernel_for(int variant) { return variant == 1 ? "sdsp_ldpc_plain_kernel" : "sdsp_ldpc_wave_kernel"; }

ldpc_shape ldpc_shape_for(uint32_t mb, uint32_t nb, uint32_t z, uint32_t edges, int variant)
{
    ldpc_shape s{};
    const uint64_t n = static_cast<uint64_t>(nb) * z, m = static_cast<uint64_t>(mb) * z;
    if (variant == 1) {
        const uint64_t per_codeword = 2 * n + edges;
        s.threads = kPlainThreads;
        s.group = 1;
        s.waves = 1;
        s.piece = std::max<uint64_t>(kPlainThreads, std::min(kMaxPiece, kWorkspace / per_codeword) / kPlainThreads * kPlainThreads);
        s.workspace_bytes = s.piece * per_codeword;
        s.per_cu = 0;
        return s;
    }
    s.group = z <= 32 ? kLanes / z : 1;
    s.wave_bytes = static_cast<uint32_t>((s.group * n + kSlack + 7) / 8 * 16 + s.group * m * 8);
    s.waves = std::max<uint32_t>(1, std::min<uint32_t>(kMaxWaves, kSmallLds / s.wave_bytes));
    s.threads = s.waves * kLanes;
    s.lds_bytes = s.waves * s.wave_bytes;
    s.per_cu = std::min<uint32_t>(kCuLds / s.lds_bytes * s.waves, 32) * s.group;
    s.piece = 0x7fffffffull;
    return s;
}

// the wave kernel's LDS limit on the current device: at plan creation and set_variant, so that process sets nothing
int ldpc_prepare(int in_kind, uint32_t lds_bytes)
{
    if (lds_bytes <= kSmallLds)
        return SDSP_HIP_OK;
    const void *k = in_kind == SDSP_HIP_LDPC_F32 ? reinterpret_cast<const void *>(sdsp_ldpc_wave_kernel<float>)
                                                 : reinterpret_cast<const void *>(sdsp_ldpc_wave_kernel<int8_t>);
    return ensure_dynamic_lds(k, kCuLds, g_wave_lds_done[in_kind == SDSP_HIP_LDPC_F32 ? 1 : 0]);
}

int launch_ldpc(const ldpc_args &la, int variant, void *stream_v)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const ldpc_shape s = ldpc_shape_for(la.mb, la.nb, la.z, la.edges, variant);
    ldpc_kargs k{};
    k.rowptr = static_cast<const uint32_t *>(la.table);
    k.ent = reinterpret_cast<const uint2 *>(k.rowptr + la.table_entries_at);
    k.mb = la.mb;
    k.z = la.z;
    k.n = la.nb * la.z;
    k.m = la.mb * la.z;
    k.norm = la.norm;
    k.beta = la.beta;
    k.early = la.early_stop ? 1 : 0;
    k.max_iter = la.max_iter;
    k.out_bits = la.out_bits;
    k.packed = la.packed ? 1 : 0;
    k.scale = la.scale;
    k.group = s.group;
    k.waves = s.waves;
    k.wave_bytes = s.wave_bytes;
    const uint64_t in_row = static_cast<uint64_t>(k.n) * (la.f32 ? 4 : 1);
    const uint64_t bits_row = la.packed ? (la.out_bits + 31) / 32 * 4ull : la.out_bits;
    dim3 grid;
    if (variant == 1) {
        k.ws_l = static_cast<int16_t *>(la.workspace);
        k.ws_r = reinterpret_cast<int8_t *>(k.ws_l + s.piece * k.n);
        k.cap = s.piece;
    }
    for (uint64_t c0 = 0; c0 < la.codewords; c0 += s.piece) {
        k.codewords = std::min<uint64_t>(s.piece, la.codewords - c0);
        k.llr = static_cast<const uint8_t *>(la.llr) + c0 * in_row;
        k.bits = la.bits ? static_cast<uint8_t *>(la.bits) + c0 * bits_row : nullptr;
        k.post = la.post ? la.post + c0 * k.n : nullptr;
        k.status = la.status ? la.status + c0 : nullptr;
        if (variant == 1) {
            if (int rc = grid_of_blocks((k.codewords + kPlainThreads - 1) / kPlainThreads, "ldpc", &grid))
                return rc;
            if (la.f32)
                hipLaunchKernelGGL(sdsp_ldpc_plain_kernel<float>, grid, dim3(kPlainThreads), 0, stream, k);
            else
                hipLaunchKernelGGL(sdsp_ldpc_plain_kernel<int8_t>, grid, dim3(kPlainThreads), 0, stream, k);
        } else {
            const uint64_t per_block = static_cast<uint64_t>(s.waves) * s.group;
            if (int rc = grid_of_blocks((k.codewords + per_block - 1) / per_block, "ldpc", &grid))
                return rc;
            if (la.f32)
                hipLaunchKernelGGL(sdsp_ldpc_wave_kernel<float>, grid, dim3(s.threads), s.lds_bytes, stream, k);
            else
                hipLaunchKernelGGL(sdsp_ldpc_wave_kernel<int8_t>, grid, dim3(s.threads), s.lds_bytes, stream, k);
        }
    }
    return launch_status("ldpc");
}
} // namespace sdsp_hip
