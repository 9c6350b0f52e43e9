// test_ldpc.cpp -- sdsp::ldpc_decoder (include/sdsp/ldpc.h) against a direct serial decoder written here: the contract in front of
// sdsp_hip_ldpc_plan_create read check by check, with one explicit message per edge.  A few noisy codewords of two codes, both input
// kinds, both output layouts, both kernel variants; bits, posteriors and status must agree exactly.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <random>
#include <vector>

#include "sdsp/ldpc.h"

namespace
{
// three circulants per information column and a staircase of zero shifts over the parity columns
sdsp::ldpc_code make_code(std::uint32_t mb, std::uint32_t nb, std::uint32_t z, unsigned seed)
{
    std::mt19937 rng(seed);
    sdsp::ldpc_code code{ std::vector<std::int16_t>(static_cast<std::size_t>(mb) * nb, -1), mb, nb, z };
    const std::uint32_t kb = nb - mb;
    for (std::uint32_t c = 0; c < kb; c++)
        for (std::uint32_t t = 0; t < 3; t++)
            code.base[((c + t * 5 + rng() % 2) % mb) * nb + c] = static_cast<std::int16_t>(rng() % z);
    for (std::uint32_t r = 0; r < mb; r++) {
        code.base[r * nb + kb + r] = 0;
        if (r + 1 < mb)
            code.base[(r + 1) * nb + kb + r] = 0;
    }
    code.base[0] = static_cast<std::int16_t>(rng() % z); // row 0 has an information entry beside its one parity entry
    return code;
}

struct result {
    std::vector<std::uint8_t> bits;
    std::vector<std::int16_t> post;
    std::int32_t status;
};

// one codeword, check by check
result direct_decode(const sdsp::ldpc_code &code, const std::vector<int> &q, const sdsp::ldpc_rule &rule, std::uint32_t max_iter)
{
    const std::uint32_t z = code.z, n = code.n(), m = code.m();
    std::vector<std::vector<std::uint32_t>> vars(m);
    for (std::uint32_t r = 0; r < code.mb; r++)
        for (std::uint32_t i = 0; i < z; i++)
            for (std::uint32_t c = 0; c < code.nb; c++) {
                const int s = code.base[r * code.nb + c];
                if (s >= 0)
                    vars[r * z + i].push_back(c * z + (i + static_cast<std::uint32_t>(s)) % z);
            }
    std::vector<int> L(q);
    std::vector<std::vector<int>> msg(m);
    for (std::uint32_t c = 0; c < m; c++)
        msg[c].assign(vars[c].size(), 0);
    auto passes = [&]() {
        for (std::uint32_t c = 0; c < m; c++) {
            int par = 0;
            for (std::uint32_t v : vars[c])
                par ^= L[v] < 0;
            if (par)
                return false;
        }
        return true;
    };
    std::int32_t status = passes() ? 0 : -1;
    for (std::uint32_t it = 1; it <= max_iter && !(rule.early_stop && status >= 0); it++) {
        for (std::uint32_t c = 0; c < m; c++) {
            const std::size_t d = vars[c].size();
            std::vector<int> T(d);
            int S = 0;
            for (std::size_t j = 0; j < d; j++) {
                T[j] = L[vars[c][j]] - msg[c][j];
                S ^= T[j] < 0;
            }
            for (std::size_t j = 0; j < d; j++) {
                int least = 1000;
                for (std::size_t o = 0; o < d; o++)
                    if (o != j)
                        least = std::min(least, std::min(std::abs(T[o]), 127));
                const int mag = std::max(((least * static_cast<int>(rule.norm) + 8) >> 4) - static_cast<int>(rule.beta), 0);
                msg[c][j] = (S ^ (T[j] < 0)) ? -mag : mag;
                L[vars[c][j]] = T[j] + msg[c][j];
            }
        }
        if (rule.early_stop || it == max_iter)
            status = passes() ? static_cast<std::int32_t>(it) : -1;
    }
    result res{ std::vector<std::uint8_t>(n), std::vector<std::int16_t>(n), status };
    for (std::uint32_t v = 0; v < n; v++) {
        res.bits[v] = L[v] < 0;
        res.post[v] = static_cast<std::int16_t>(L[v]);
    }
    return res;
}

int quantise(float x, float scale)
{
    const float y = std::nearbyint(x * scale);
    return y != y ? 0 : static_cast<int>(std::min(std::max(y, -127.0f), 127.0f));
}

template <typename in_t>
int run(const sdsp::ldpc_code &code, const sdsp::ldpc_rule &rule, sdsp::ldpc_output output, std::uint32_t out_bits, std::uint32_t max_iter,
        std::uint64_t codewords, unsigned seed)
{
    constexpr bool f32 = std::is_same<in_t, float>::value;
    const float scale = 8.0f;
    std::mt19937 rng(seed);
    std::normal_distribution<float> gauss(0.0f, 1.0f);
    const std::uint32_t n = code.n(), k = code.k();
    std::vector<std::uint8_t> data(codewords * k);
    for (auto &v : data)
        v = static_cast<std::uint8_t>(rng() & 1);
    const std::vector<std::uint8_t> sent = sdsp::ldpc_encode(code, data);
    int bad = 0;
    bad += !std::equal(data.begin(), data.begin() + k, sent.begin());
    bad += sdsp::ldpc_parity_matrix(code).size() != static_cast<std::size_t>(code.m()) * ((k + 31) / 32);
    std::vector<in_t> llr(codewords * n);
    std::vector<result> want;
    int clean = 0, late = 0, failed = 0;
    for (std::uint64_t c = 0; c < codewords; c++) {
        const float sigma = (c % 4 == 0) ? 0.0f : (c % 4 == 3) ? 3.0f : 0.55f; // clean, 5 dB (two of four), hopeless
        std::vector<int> q(n);
        for (std::uint32_t v = 0; v < n; v++) {
            const float y = (sent[c * n + v] ? -1.0f : 1.0f) + sigma * gauss(rng);
            if constexpr (f32) {
                llr[c * n + v] = y;
                q[v] = quantise(y, scale);
            } else {
                const int raw = std::min(std::max(static_cast<int>(std::nearbyint(y * scale)), -128), 127);
                llr[c * n + v] = static_cast<std::int8_t>(raw);
                q[v] = std::max(raw, -127);
            }
        }
        want.push_back(direct_decode(code, q, rule, max_iter));
        bad += c % 4 == 0 && !std::equal(want.back().bits.begin(), want.back().bits.end(), sent.begin() + static_cast<std::ptrdiff_t>(c * n));
        clean += c % 4 == 0 && want.back().status >= 0;
        late += c % 4 != 0 && want.back().status > 0;
        failed += want.back().status < 0;
    }
    sdsp::ldpc_decoder<in_t> dec(code, rule, output, out_bits, scale);
    const std::size_t bb = dec.bits_bytes();
    sdsp_hip_ldpc_plan_info info{};
    for (int variant : { 0, 1 }) {
        dec.set_variant(variant);
        info = dec.info();
        std::vector<std::uint8_t> bits(codewords * bb, 0x55);
        std::vector<std::int16_t> post(codewords * n, 0x5555);
        std::vector<std::int32_t> status(codewords, 77);
        dec.process_host(llr.data(), bits.data(), post.data(), status.data(), codewords, max_iter);
        for (std::uint64_t c = 0; c < codewords; c++) {
            bad += status[c] != want[c].status;
            bad += !std::equal(want[c].post.begin(), want[c].post.end(), post.begin() + static_cast<std::ptrdiff_t>(c * n));
            for (std::uint32_t v = 0; v < dec.out_bits(); v++) {
                const unsigned got = output == sdsp::ldpc_output::packed ? (bits[c * bb + v / 8] >> (v % 8)) & 1u : bits[c * bb + v];
                bad += got != want[c].bits[v];
            }
            if (output == sdsp::ldpc_output::packed)
                for (std::size_t v = dec.out_bits(); v < bb * 8; v++)
                    bad += (bits[c * bb + v / 8] >> (v % 8)) & 1u; // the unused top bits are zero
        }
        bad += dec.launches(codewords) != 1 || info.variant != variant || info.n != n || info.m != code.m();
    }
    const bool ok = bad == 0 && clean > 0 && late > 0 && failed > 0;
    std::printf("ldpc_decoder<%s>: %u x %u, z = %u, %s, %llu codewords: %d clean, %d decoded, %d undecoded, kernel %s, lds %u: %s\n",
                f32 ? "float" : "int8", code.mb, code.nb, code.z, output == sdsp::ldpc_output::packed ? "packed" : "bytes",
                static_cast<unsigned long long>(codewords), clean, late, failed, info.kernel, info.lds_bytes, ok ? "bit for bit" : "MISMATCH");
    return ok ? 0 : 1;
}
} // namespace

int main()
{
    try {
        const sdsp::ldpc_code a = make_code(6, 12, 27, 1), b = make_code(4, 10, 81, 2);
        int rc = run<std::int8_t>(a, { 12, 0, true }, sdsp::ldpc_output::bytes, 0, 15, 9, 1);
        rc |= run<float>(b, { 16, 1, false }, sdsp::ldpc_output::packed, b.k() + 3, 6, 7, 2);
        rc |= run<float>(a, { 13, 0, true }, sdsp::ldpc_output::packed, 45, 15, 5, 3);
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &ex) {
        std::printf("no usable device: %s\n", ex.what());
        return 3;
    }
}
