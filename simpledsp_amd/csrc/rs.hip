// rs.hip -- Reed-Solomon decoder banks over GF(256) (sdsp_hip_rs_*).  The contract is the comment in front of
// sdsp_hip_rs_plan_create in include/sdsp_hip.h: the result of a codeword is defined by the code, not by an algorithm, so both kernels
// end with the definition itself -- the corrected word has zero syndromes and lies within 2 errors + erasures <= nroots -- and every
// byte they write is the one tests/rs_ref.py writes.
//
// Both kernels read the plan's 768-byte table (exp[0 .. 512), alpha^i twice round so that a sum of two logarithms needs no
// reduction, then log[0 .. 256)) into LDS once per workgroup.
// sdsp_rs_wave_kernel (variant 0): a wave per frame, a few frames in turn.  The frame and its erasure flags are staged into the wave's
// LDS with 16-byte loads wherever global memory is aligned (the LDS image starts at the same offset within 16 bytes, so a load and its
// store are both aligned), and a codeword's symbols are read from there I apart.  Lane l holds symbols l, l + 64, l + 128, l + 192 as
// logarithms; the exponent of a symbol's term advances by a per-lane constant from one syndrome to the next; four syndromes are the
// four bytes of a register and reduce with one XOR butterfly.  A clean codeword is done there.  Otherwise lane i holds coefficient
// i + 1 of the locator and of its companion (coefficient 0 is the constant 1, and a wave-uniform value), the discrepancy is a masked
// multiply per lane and the same butterfly, the root search and Forney's values run on the four positions a lane owns, and the
// corrected word's syndromes are taken again before anything leaves.  No barrier after the table's, no atomics.
// sdsp_rs_plain_kernel (variant 1): a thread per codeword, the textbook serial loops on private arrays, the symbols read from global
// memory I apart.
#include "stream_dev.h"

#include <algorithm>

namespace sdsp_hip
{
namespace
{
constexpr uint32_t kLanes = 64;
constexpr uint32_t kWaves = 4;        // waves per workgroup of the wave kernel
constexpr uint32_t kTable = 768;      // exp[512], log[256]
constexpr uint32_t kLog = 512;        // offset of the logarithms
constexpr uint32_t kSyn = 64;         // a wave's syndromes
constexpr uint32_t kMaxRoots = 64;
constexpr uint32_t kMaxFramesPerWave = 16;
constexpr uint32_t kMinBlocks = 2048; // frames are shared out among at least so many workgroups before a wave takes a second one

struct rs_kargs {
    const uint8_t *in;
    uint8_t *out;
    const uint8_t *eras; // nullable
    int32_t *corrected;  // nullable
    const uint8_t *table;
    uint64_t frames;
    uint32_t n, nroots, k, I, fcr, prim;
    uint32_t data_only, inplace;
    uint32_t fpw;      // wave kernel: frames per wave
    uint32_t image;    // wave kernel: bytes of one staged image (frame or flags), a multiple of 16
};

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t gf_mul(const uint8_t *tab, uint32_t a, uint32_t b)
{
    const uint32_t p = tab[tab[kLog + a] + tab[kLog + b]];
    return a && b ? p : 0;
}
__device__ __forceinline__ uint32_t gf_inv(const uint8_t *tab, uint32_t a) { return tab[255 - tab[kLog + a]]; }
// e + d mod 255 for e, d < 255
__device__ __forceinline__ uint32_t add255(uint32_t e, uint32_t d)
{
    const uint32_t s = e + d;
    return min(s, s - 255);
}
__device__ __forceinline__ uint32_t xor_reduce(uint32_t v)
{
#pragma unroll
    for (int m = 1; m < 64; m *= 2)
        v ^= static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), m));
    return v;
}
__device__ __forceinline__ uint32_t lane_value(uint32_t v, uint32_t lane)
{
    return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), static_cast<int>(lane)));
}

__device__ __forceinline__ void load_table(uint8_t *tab, const uint8_t *table)
{
    if (threadIdx.x < kTable / 4)
        reinterpret_cast<uint32_t *>(tab)[threadIdx.x] = reinterpret_cast<const uint32_t *>(table)[threadIdx.x];
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------- wave kernel

// what a lane keeps for the four positions it owns: the logarithm of the locator X_i = alpha^(prim (n-1-i)), of X_i^fcr and of 1 / X_i
struct lane_consts {
    uint32_t step[4], base[4], zl[4];
};

// `bytes` bytes from g into the image at `img`, at the offset g has within 16 bytes; returns where byte 0 landed
__device__ __forceinline__ uint8_t *stage_in(uint8_t *img, const uint8_t *g, uint32_t bytes, uint32_t lane)
{
    const uint32_t off = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(g) & 15);
    uint8_t *w = img + off;
    const uint32_t head = min((16 - off) & 15, bytes);
    const uint32_t nvec = (bytes - head) / 16, tail = head + nvec * 16;
    if (lane < head)
        w[lane] = g[lane];
    for (uint32_t v = lane; v < nvec; v += kLanes)
        *reinterpret_cast<uint4 *>(w + head + v * 16) = *reinterpret_cast<const uint4 *>(g + head + v * 16);
    if (tail + lane < bytes)
        w[tail + lane] = g[tail + lane];
    return w;
}

// `bytes` bytes from the LDS image at w to o
__device__ __forceinline__ void stage_out(uint8_t *o, const uint8_t *w, uint32_t bytes, uint32_t lane)
{
    const uint32_t off = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(o) & 15);
    const uint32_t head = min((16 - off) & 15, bytes);
    const uint32_t nvec = (bytes - head) / 16, tail = head + nvec * 16;
    if (lane < head)
        o[lane] = w[lane];
    const bool aligned = (reinterpret_cast<uintptr_t>(w + head) & 15) == 0; // wave-uniform
    for (uint32_t v = lane; v < nvec; v += kLanes) {
        const uint8_t *s = w + head + v * 16;
        uint4 x;
        if (aligned)
            x = *reinterpret_cast<const uint4 *>(s);
        else
            __builtin_memcpy(&x, s, 16);
        *reinterpret_cast<uint4 *>(o + head + v * 16) = x;
    }
    if (tail + lane < bytes)
        o[tail + lane] = w[tail + lane];
}

// the syndromes of the codeword whose symbol s is cw[s I], into syn[0 .. nroots); returns the OR of them, the same on every lane
__device__ uint32_t wave_syndromes(const uint8_t *tab, const uint8_t *cw, uint8_t *syn, const rs_kargs &a, const lane_consts &c, uint32_t lane)
{
    uint32_t e[4];
    bool nz[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t i = lane + 64 * q;
        const uint32_t v = i < a.n ? cw[i * a.I] : 0;
        nz[q] = v != 0;
        e[q] = add255(tab[kLog + v], c.base[q]);
    }
    uint32_t any = 0;
    for (uint32_t j0 = 0; j0 < a.nroots; j0 += 4) {
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            uint32_t t = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t x = tab[e[q]];
                t ^= nz[q] ? x : 0;
                e[q] = add255(e[q], c.step[q]);
            }
            word |= t << (8 * b);
        }
        word = xor_reduce(word);
        const uint32_t left = a.nroots - j0;
        if (left < 4)
            word &= (1u << (8 * left)) - 1;
        any |= word;
        if (lane < 4 && lane < left)
            syn[j0 + lane] = static_cast<uint8_t>(word >> (8 * lane));
    }
    wave_lds_sync();
    return any;
}

// a codeword with non-zero syndromes and at most nroots erasures (em: their ballots): locator, roots, values, and the contract as the
// last word.  Returns the count of symbols changed, or -1 with the codeword as it was.  gout: the codeword in global memory where the
// call is in place, else null.
__device__ int wave_correct(const uint8_t *tab, uint8_t *cw, uint8_t *syn, const rs_kargs &a, const lane_consts &c, uint32_t lane,
                            const uint64_t em[4], uint32_t ne, uint8_t *gout)
{
    const uint32_t nroots = a.nroots;
    const bool live = lane < nroots;
    // the erasure locator prod (1 + X_i x)
    uint32_t L = 0;
    for (int q = 0; q < 4; q++) {
        uint64_t m = em[q];
        while (m) {
            const uint32_t i = 64 * q + static_cast<uint32_t>(__builtin_ctzll(m));
            m &= m - 1;
            const uint32_t x = tab[(a.prim * (a.n - 1 - i)) % 255];
            uint32_t up = static_cast<uint32_t>(__shfl_up(static_cast<int>(L), 1));
            if (lane == 0)
                up = 1;
            L ^= gf_mul(tab, x, up);
            if (!live)
                L = 0;
        }
    }
    // Berlekamp-Massey on top of it
    uint32_t B = L, b0 = 1, el = ne;
    for (uint32_t r = ne + 1; r <= nroots; r++) {
        const int idx = static_cast<int>(r) - 2 - static_cast<int>(lane);
        const uint32_t s = idx >= 0 ? syn[idx] : 0;
        uint32_t d = gf_mul(tab, L, s);
        if (lane == 0)
            d ^= syn[r - 1];
        d = lane_value(xor_reduce(d), 0);
        uint32_t xb = static_cast<uint32_t>(__shfl_up(static_cast<int>(B), 1));
        if (lane == 0)
            xb = b0;
        if (d == 0) {
            B = xb;
            b0 = 0;
        } else {
            const uint32_t T = L ^ gf_mul(tab, d, xb);
            if (2 * el <= r + ne - 1) {
                el = r + ne - el;
                const uint32_t di = gf_inv(tab, d);
                B = gf_mul(tab, L, di);
                b0 = di;
            } else {
                B = xb;
                b0 = 0;
            }
            L = T;
        }
        if (!live) {
            L = 0;
            B = 0;
        }
    }
    const uint64_t nzmask = __ballot(L != 0);
    if (nzmask == 0)
        return -1;
    const uint32_t deg = 64 - static_cast<uint32_t>(__builtin_clzll(nzmask));
    // the root search on the positions a lane owns: val = lambda(z), den = z lambda'(z) (the odd terms), z = 1 / X_i
    const uint32_t logL = tab[kLog + L];
    uint32_t val[4] = { 1, 1, 1, 1 }, den[4] = { 0, 0, 0, 0 }, ex[4] = { 0, 0, 0, 0 };
    for (uint32_t k = 1; k <= deg; k++) {
        const uint32_t lc = lane_value(L, k - 1), ll = lane_value(logL, k - 1);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            ex[q] = add255(ex[q], c.zl[q]);
            const uint32_t t = lc ? tab[ll + ex[q]] : 0;
            val[q] ^= t;
            den[q] ^= (k & 1) ? t : 0;
        }
    }
    bool root[4];
    uint32_t count = 0;
    bool bad = false;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        root[q] = lane + 64 * q < a.n && val[q] == 0;
        count += static_cast<uint32_t>(__popcll(__ballot(root[q])));
        bad = bad || (root[q] && den[q] == 0);
    }
    if (count != deg || __ballot(bad) != 0)
        return -1;
    // omega = S lambda mod x^nroots: lane m holds coefficient m
    uint32_t Om = live ? syn[lane] : 0;
    for (uint32_t k = 1; k <= deg; k++) {
        const uint32_t lc = lane_value(L, k - 1), ll = lane_value(logL, k - 1);
        const int idx = static_cast<int>(lane) - static_cast<int>(k);
        const uint32_t s = live && idx >= 0 ? syn[idx] : 0;
        const uint32_t t = tab[ll + tab[kLog + s]];
        Om ^= lc && s ? t : 0;
    }
    const uint32_t logO = tab[kLog + Om];
    uint32_t num[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int q = 0; q < 4; q++)
        ex[q] = 0;
    for (uint32_t m = 0; m < nroots; m++) {
        const uint32_t om = lane_value(Om, m), lo = lane_value(logO, m);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            num[q] ^= om ? tab[lo + ex[q]] : 0;
            ex[q] = add255(ex[q], c.zl[q]);
        }
    }
    // Forney: e_i = X_i^(1 - fcr) omega(z) / lambda'(z) = X_i^(-fcr) omega(z) / (z lambda'(z))
    uint32_t orig[4], ev[4];
    uint32_t changed = 0, outside = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t i = lane + 64 * q;
        ev[q] = 0;
        orig[q] = 0;
        if (root[q]) {
            const uint32_t x = (tab[kLog + num[q]] + 255 - tab[kLog + den[q]]) % 255;
            const uint32_t v = tab[x + (a.fcr * c.zl[q]) % 255];
            ev[q] = num[q] ? v : 0;
            orig[q] = cw[i * a.I];
            if (ev[q])
                cw[i * a.I] = static_cast<uint8_t>(orig[q] ^ ev[q]);
        }
        const uint64_t ch = __ballot(ev[q] != 0);
        changed += static_cast<uint32_t>(__popcll(ch));
        outside += static_cast<uint32_t>(__popcll(ch & ~em[q]));
    }
    wave_lds_sync();
    const uint32_t any = wave_syndromes(tab, cw, syn, a, c, lane);
    if (any != 0 || 2 * outside + ne > nroots) {
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (ev[q])
                cw[(lane + 64 * q) * a.I] = static_cast<uint8_t>(orig[q]);
        wave_lds_sync();
        return -1;
    }
    if (gout) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t i = lane + 64 * q;
            if (ev[q] && (!a.data_only || i < a.k))
                gout[static_cast<uint64_t>(i) * a.I] = static_cast<uint8_t>(orig[q] ^ ev[q]);
        }
    }
    return static_cast<int>(changed);
}

__global__ __launch_bounds__(kWaves *kLanes) void sdsp_rs_wave_kernel(rs_kargs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t rs_lds[];
    uint8_t *tab = rs_lds;
    load_table(tab, a.table);
    const uint32_t lane = threadIdx.x % kLanes, wave = threadIdx.x / kLanes;
    uint8_t *syn = rs_lds + kTable + wave * (kSyn + 2 * a.image);
    uint8_t *frame_img = syn + kSyn, *flag_img = frame_img + a.image;
    lane_consts c;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t i = lane + 64 * q;
        const uint32_t p = i < a.n ? a.n - 1 - i : 0;
        c.step[q] = (a.prim * p) % 255;
        c.base[q] = (c.step[q] * a.fcr) % 255;
        c.zl[q] = (255 - c.step[q]) % 255;
    }
    const uint32_t fb = a.I * a.n, ob = a.data_only ? a.I * a.k : fb;
    const uint64_t first = (static_cast<uint64_t>(blockIdx.x) * kWaves + wave) * a.fpw;
    for (uint32_t f = 0; f < a.fpw; f++) {
        const uint64_t frame = first + f;
        if (frame >= a.frames) // wave-uniform
            break;
        uint8_t *w = stage_in(frame_img, a.in + frame * fb, fb, lane);
        const uint8_t *fl = a.eras ? stage_in(flag_img, a.eras + frame * fb, fb, lane) : nullptr;
        wave_lds_sync();
        for (uint32_t j = 0; j < a.I; j++) {
            uint8_t *cw = w + j;
            uint64_t em[4] = { 0, 0, 0, 0 };
            uint32_t ne = 0;
            if (fl) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t i = lane + 64 * q;
                    em[q] = __ballot(i < a.n && fl[i * a.I + j] != 0);
                    ne += static_cast<uint32_t>(__popcll(em[q]));
                }
            }
            int result = -1;
            if (ne <= a.nroots) {
                result = 0;
                if (wave_syndromes(tab, cw, syn, a, c, lane) != 0)
                    result = wave_correct(tab, cw, syn, a, c, lane, em, ne, a.inplace ? a.out + frame * fb + j : nullptr);
            }
            if (a.corrected && lane == 0)
                a.corrected[frame * a.I + j] = result;
        }
        wave_lds_sync();
        if (!a.inplace)
            stage_out(a.out + frame * ob, w, ob, lane);
        wave_lds_sync();
    }
}

// --------------------------------------------------------------------------------------------------------------- plain kernel

// s: the syndromes (updated to those of the corrected word); epos: the erased positions; pos, ev: the roots found and their values,
// *found of them.  Returns the count of symbols changed, or -1.
__device__ int plain_correct(const uint8_t *tab, const rs_kargs &a, const uint8_t *er, uint8_t *s, const uint8_t *epos, uint32_t ne,
                             uint8_t *pos, uint8_t *ev, uint32_t *found)
{
    const uint32_t nroots = a.nroots, n = a.n;
    uint8_t lam[kMaxRoots + 1], b[kMaxRoots + 1], t[kMaxRoots + 1], om[kMaxRoots];
    for (uint32_t k = 0; k <= nroots; k++)
        lam[k] = k == 0;
    for (uint32_t e = 0; e < ne; e++) {
        const uint32_t x = tab[(a.prim * (n - 1 - epos[e])) % 255];
        for (uint32_t k = nroots; k >= 1; k--)
            lam[k] ^= static_cast<uint8_t>(gf_mul(tab, x, lam[k - 1]));
    }
    for (uint32_t k = 0; k <= nroots; k++)
        b[k] = lam[k];
    uint32_t el = ne;
    for (uint32_t step = ne + 1; step <= nroots; step++) {
        uint32_t d = 0;
        for (uint32_t k = 0; k < step; k++)
            d ^= gf_mul(tab, lam[k], s[step - 1 - k]);
        if (d == 0) {
            for (uint32_t k = nroots; k >= 1; k--)
                b[k] = b[k - 1];
            b[0] = 0;
            continue;
        }
        t[0] = lam[0];
        for (uint32_t k = 1; k <= nroots; k++)
            t[k] = lam[k] ^ static_cast<uint8_t>(gf_mul(tab, d, b[k - 1]));
        if (2 * el <= step + ne - 1) {
            el = step + ne - el;
            const uint32_t di = gf_inv(tab, d);
            for (uint32_t k = 0; k <= nroots; k++)
                b[k] = static_cast<uint8_t>(gf_mul(tab, lam[k], di));
        } else {
            for (uint32_t k = nroots; k >= 1; k--)
                b[k] = b[k - 1];
            b[0] = 0;
        }
        for (uint32_t k = 0; k <= nroots; k++)
            lam[k] = t[k];
    }
    uint32_t deg = 0;
    for (uint32_t k = 1; k <= nroots; k++)
        if (lam[k])
            deg = k;
    if (deg == 0)
        return -1;
    for (uint32_t m = 0; m < nroots; m++) {
        uint32_t v = 0;
        for (uint32_t k = 0; k <= min(m, deg); k++)
            v ^= gf_mul(tab, lam[k], s[m - k]);
        om[m] = static_cast<uint8_t>(v);
    }
    // roots and values, position by position
    uint32_t nr = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t zl = (255 - (a.prim * (n - 1 - i)) % 255) % 255;
        uint32_t val = 0, den = 0;
        for (uint32_t k = 0; k <= deg; k++) {
            const uint32_t term = lam[k] ? tab[(tab[kLog + lam[k]] + k * zl) % 255] : 0;
            val ^= term;
            den ^= (k & 1) ? term : 0;
        }
        if (val != 0)
            continue;
        if (den == 0 || nr >= deg)
            return -1;
        uint32_t num = 0;
        for (uint32_t m = 0; m < nroots; m++)
            num ^= om[m] ? tab[(tab[kLog + om[m]] + m * zl) % 255] : 0;
        pos[nr] = static_cast<uint8_t>(i);
        ev[nr] = num ? tab[(tab[kLog + num] + 255 - tab[kLog + den] + (a.fcr * zl) % 255) % 255] : 0;
        nr++;
    }
    if (nr != deg)
        return -1;
    // the contract as the last word: the corrected word's syndromes, and the bound
    uint32_t changed = 0, outside = 0;
    for (uint32_t l = 0; l < nr; l++) {
        if (!ev[l])
            continue;
        changed++;
        if (!(er && er[static_cast<uint64_t>(pos[l]) * a.I]))
            outside++;
        const uint32_t xl = (a.prim * (n - 1 - pos[l])) % 255, le = tab[kLog + ev[l]];
        for (uint32_t j = 0; j < nroots; j++)
            s[j] ^= tab[(le + xl * (a.fcr + j)) % 255];
    }
    uint32_t any = 0;
    for (uint32_t j = 0; j < nroots; j++)
        any |= s[j];
    if (any != 0 || 2 * outside + ne > nroots)
        return -1;
    *found = nr;
    return static_cast<int>(changed);
}

__global__ __launch_bounds__(256) void sdsp_rs_plain_kernel(rs_kargs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t tab[kTable];
    load_table(tab, a.table);
    const uint64_t id = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (id >= a.frames * a.I)
        return;
    const uint64_t frame = id / a.I, j = id % a.I;
    const uint32_t n = a.n, nroots = a.nroots, I = a.I;
    const uint8_t *r = a.in + frame * I * n + j;
    const uint8_t *er = a.eras ? a.eras + frame * I * n + j : nullptr;
    const uint32_t lim = a.data_only ? a.k : n;
    uint8_t *o = a.out + frame * I * lim + j;
    uint8_t s[kMaxRoots], epos[kMaxRoots], pos[kMaxRoots], ev[kMaxRoots];
    uint32_t ne = 0;
    if (er)
        for (uint32_t i = 0; i < n; i++)
            if (er[static_cast<uint64_t>(i) * I]) {
                if (ne < nroots)
                    epos[ne] = static_cast<uint8_t>(i);
                ne++;
            }
    int result = -1;
    uint32_t found = 0;
    if (ne <= nroots) {
        // Horner in every root at once: S_j = (S_j alpha^(prim (fcr + j))) + r_i
        for (uint32_t q = 0; q < nroots; q++)
            s[q] = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t v = r[static_cast<uint64_t>(i) * I];
            for (uint32_t q = 0; q < nroots; q++)
                s[q] = static_cast<uint8_t>((s[q] ? tab[tab[kLog + s[q]] + (a.prim * (a.fcr + q)) % 255] : 0) ^ v);
        }
        uint32_t any = 0;
        for (uint32_t q = 0; q < nroots; q++)
            any |= s[q];
        result = any ? plain_correct(tab, a, er, s, epos, ne, pos, ev, &found) : 0;
    }
    if (!a.inplace)
        for (uint32_t i = 0; i < lim; i++)
            o[static_cast<uint64_t>(i) * I] = r[static_cast<uint64_t>(i) * I];
    if (result > 0)
        for (uint32_t l = 0; l < found; l++)
            if (ev[l] && pos[l] < lim)
                o[static_cast<uint64_t>(pos[l]) * I] = static_cast<uint8_t>(r[static_cast<uint64_t>(pos[l]) * I] ^ ev[l]);
    if (a.corrected)
        a.corrected[id] = result;
}
} // namespace

const char *rs_kernel_for(int variant) { return variant == 1 ? "sdsp_rs_plain_kernel" : "sdsp_rs_wave_kernel"; }

rs_shape rs_shape_for(uint32_t n, uint32_t interleave, int variant)
{
    rs_shape s{};
    if (variant == 1) {
        s.threads = 256;
        s.waves = 4;
        s.image = 0;
        s.lds_bytes = kTable;
        return s;
    }
    s.threads = kWaves * kLanes;
    s.waves = kWaves;
    s.image = (interleave * n + 15 + 15) / 16 * 16; // the frame at any offset within 16 bytes
    s.lds_bytes = kTable + kWaves * (kSyn + 2 * s.image);
    return s;
}

int launch_rs(const rs_args &ra, int variant, void *stream_v)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const rs_shape s = rs_shape_for(ra.n, ra.interleave, variant);
    rs_kargs k{};
    k.in = static_cast<const uint8_t *>(ra.in);
    k.out = static_cast<uint8_t *>(ra.out);
    k.eras = static_cast<const uint8_t *>(ra.erasures);
    k.corrected = ra.corrected;
    k.table = static_cast<const uint8_t *>(ra.table);
    k.frames = ra.frames;
    k.n = ra.n;
    k.nroots = ra.nroots;
    k.k = ra.n - ra.nroots;
    k.I = ra.interleave;
    k.fcr = ra.fcr;
    k.prim = ra.prim;
    k.data_only = ra.data_only ? 1 : 0;
    k.inplace = ra.in == ra.out ? 1 : 0;
    k.image = s.image;
    dim3 grid;
    if (variant == 1) {
        if (int rc = grid_of_blocks((ra.frames * ra.interleave + 255) / 256, "rs", &grid))
            return rc;
        hipLaunchKernelGGL(sdsp_rs_plain_kernel, grid, dim3(s.threads), 0, stream, k);
        return launch_status("rs");
    }
    k.fpw = static_cast<uint32_t>(std::min<uint64_t>(kMaxFramesPerWave, std::max<uint64_t>(1, ra.frames / (kWaves * kMinBlocks))));
    const uint64_t per_block = static_cast<uint64_t>(kWaves) * k.fpw;
    if (int rc = grid_of_blocks((ra.frames + per_block - 1) / per_block, "rs", &grid))
        return rc;
    hipLaunchKernelGGL(sdsp_rs_wave_kernel, grid, dim3(s.threads), s.lds_bytes, stream, k);
    return launch_status("rs");
}
} // namespace sdsp_hip
