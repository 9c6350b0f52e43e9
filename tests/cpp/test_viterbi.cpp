// sdsp::viterbi_bank (include/sdsp/viterbi.h) on 5 channels of 12 blocks in two calls: the K = 7 (171, 133) code in both kernel variants
// and a K = 5 rate-1/3 code, int8 and float soft values, bytes and packed words, through the host entry, against the contract written as
// direct loops here (add, compare, select on 32-bit metrics; a traceback per block).  Everything is on integers, so the comparison is on
// bits.  Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/viterbi.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <random>
#include <type_traits>
#include <vector>

namespace
{
constexpr std::uint64_t kChannels = 5;
constexpr float kScale = 8.0f;

struct code {
    std::uint32_t k;
    std::vector<std::uint32_t> gens;
};

int quantise(std::int8_t x) { return std::max<int>(x, -127); }
int quantise(float x)
{
    const float y = std::nearbyint(x * kScale); // the default rounding mode: to nearest, ties to even
    return std::isnan(y) ? 0 : static_cast<int>(std::min(std::max(y, -127.0f), 127.0f));
}

// the coded bit of generator g for the register reg (the input of i steps ago in bit i)
int coded(std::uint32_t k, std::uint32_t g, std::uint32_t reg)
{
    int c = 0;
    for (std::uint32_t i = 0; i < k; i++)
        c ^= static_cast<int>(((g >> (k - 1 - i)) & 1u) & ((reg >> i) & 1u));
    return c;
}

// one channel of the whole stream by the contract: out[t] = the bit of step t - Dr
template <typename in_t>
void by_loops(const code &c, std::uint32_t B, std::uint32_t D, const in_t *soft, std::size_t steps, std::vector<std::uint8_t> &out,
              std::vector<std::int32_t> &metrics)
{
    const std::size_t n = c.gens.size();
    const std::uint32_t S = 1u << (c.k - 1), Dr = (D + B - 1) / B * B;
    std::vector<std::uint32_t> m(S, 0), next(S);
    std::vector<std::vector<std::uint8_t>> dec(steps, std::vector<std::uint8_t>(S));
    out.assign(steps, 0);
    for (std::size_t t = 0; t < steps; t++) {
        for (std::uint32_t s = 0; s < S; s++) {
            const std::uint32_t p0 = s >> 1, p1 = p0 + S / 2;
            int bm0 = 0, bm1 = 0;
            for (std::size_t j = 0; j < n; j++) {
                const int q = quantise(soft[t * n + j]);
                bm0 += coded(c.k, c.gens[j], (p0 << 1) | (s & 1u)) ? -q : q;
                bm1 += coded(c.k, c.gens[j], (p1 << 1) | (s & 1u)) ? -q : q;
            }
            const std::uint32_t a0 = m[p0] + static_cast<std::uint32_t>(bm0), a1 = m[p1] + static_cast<std::uint32_t>(bm1);
            const bool d = static_cast<std::int32_t>(a1 - a0) > 0;
            dec[t][s] = d ? 1 : 0;
            next[s] = d ? a1 : a0;
        }
        m.swap(next);
        if (t + 1 >= static_cast<std::size_t>(B) + D && (t + 1 - D) % B == 0) { // step t decides the block that ends at t - D
            std::uint32_t s = 0;
            std::int32_t best = 0;
            for (std::uint32_t v = 1; v < S; v++)
                if (static_cast<std::int32_t>(m[v] - m[0]) > best) {
                    best = static_cast<std::int32_t>(m[v] - m[0]);
                    s = v;
                }
            const std::size_t first = t + 1 - D - B;
            for (std::size_t u = t + 1; u-- > first;) {
                if (u < first + B && u + Dr < steps)
                    out[u + Dr] = static_cast<std::uint8_t>(s & 1u);
                s = (s >> 1) + dec[u][s] * (S / 2);
            }
        }
    }
    metrics.resize(S);
    for (std::uint32_t s = 0; s < S; s++)
        metrics[s] = static_cast<std::int32_t>(m[s]);
}

template <typename in_t> int run(const code &c, std::uint32_t B, std::uint32_t D, unsigned seed)
{
    const std::size_t n = c.gens.size(), steps = 12 * static_cast<std::size_t>(B), first = 5 * static_cast<std::size_t>(B);
    std::mt19937 gen(seed);
    std::normal_distribution<double> noise(0.0, 30.0);
    std::vector<in_t> soft(kChannels * steps * n);
    for (std::uint64_t ch = 0; ch < kChannels; ch++) {
        std::vector<std::uint8_t> bits(steps);
        for (auto &b : bits)
            b = static_cast<std::uint8_t>(gen() & 1u);
        const std::vector<std::uint8_t> cb = sdsp::conv_encode(c.k, c.gens, bits);
        for (std::size_t i = 0; i < steps * n; i++) {
            const double v = std::min(127.0, std::max(-128.0, std::nearbyint((cb[i] ? -40.0 : 40.0) + noise(gen))));
            if (std::is_same<in_t, float>::value)
                soft[ch * steps * n + i] = static_cast<in_t>((v + (i % 7 == 0 ? 0.5 : 0.0)) / kScale);
            else
                soft[ch * steps * n + i] = static_cast<in_t>(v);
        }
    }
    std::vector<std::vector<std::uint8_t>> want(kChannels);
    std::vector<std::int32_t> want_m;
    for (std::uint64_t ch = 0; ch < kChannels; ch++) {
        std::vector<std::int32_t> m;
        by_loops(c, B, D, soft.data() + ch * steps * n, steps, want[ch], m);
        want_m.insert(want_m.end(), m.begin(), m.end());
    }
    int bad = 0;
    std::size_t ones = 0;
    sdsp_hip_viterbi_plan_info info{};
    for (int packed = 0; packed < 2; packed++)
        for (int variant = c.k == 7 ? 0 : 1; variant < 2; variant++) {
            sdsp::viterbi_bank<in_t> bank(c.k, c.gens, B, D, kChannels, packed ? sdsp::viterbi_output::packed : sdsp::viterbi_output::bytes, kScale);
            bank.set_variant(variant);
            info = bank.info();
            bad += bank.delay() != sdsp::viterbi_delay(B, D) || bank.launches(kChannels, steps) != 1;
            // two calls: the rows of a call are compact, so each gets its own copy of its part of every channel
            std::size_t t0 = 0;
            for (std::size_t part : { first, steps - first }) {
                std::vector<in_t> in(kChannels * part * n);
                for (std::uint64_t ch = 0; ch < kChannels; ch++)
                    std::copy_n(soft.data() + (ch * steps + t0) * n, part * n, in.data() + ch * part * n);
                std::vector<std::uint8_t> bytes(kChannels * part, 9);
                std::vector<std::uint32_t> words(kChannels * part / 32, 0xdeadbeefu);
                bank.process_host(in.data(), packed ? static_cast<void *>(words.data()) : static_cast<void *>(bytes.data()), kChannels, part);
                for (std::uint64_t ch = 0; ch < kChannels; ch++)
                    for (std::size_t t = 0; t < part; t++) {
                        const std::uint32_t got = packed ? (words[(ch * part + t) / 32] >> (t % 32)) & 1u : bytes[ch * part + t];
                        bad += got != want[ch][t0 + t];
                        ones += got;
                    }
                t0 += part;
            }
            bad += bank.metrics(kChannels) != want_m;
        }
    const bool ok = bad == 0 && ones > 0 && info.states == (1u << (c.k - 1)) && info.block == B && info.depth == D;
    std::printf("viterbi_bank<%s>: K = %u, n = %zu, (B, D) = (%u, %u), %llu x %zu steps, kernel %s, chunk %u, lds %u: %s\n",
                std::is_same<in_t, float>::value ? "float" : "int8", c.k, n, B, D, static_cast<unsigned long long>(kChannels), steps, info.kernel,
                info.chunk, info.lds_bytes, ok ? "bit for bit" : "MISMATCH");
    return ok ? 0 : 1;
}
} // namespace

int main()
{
    try {
        const code k7{ 7, { 0171, 0133 } }, k5{ 5, { 025, 033, 037 } };
        int rc = run<std::int8_t>(k7, 32, 64, 1) | run<float>(k7, 64, 100, 2);
        rc |= run<std::int8_t>(k5, 32, 35, 3) | run<float>(k5, 32, 4, 4);
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &ex) {
        std::printf("no usable device: %s\n", ex.what());
        return 3;
    }
}
