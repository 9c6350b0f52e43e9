// sdsp::rank_filter_bank (include/sdsp/rank_filter.h) as a de-spiker: every channel is a sine of its own frequency with isolated
// impulses of +-100 on top, streamed block by block through the host entry of a 5-point running median (empty and one-sample blocks
// included).  Every output must equal, bit for bit, a std::nth_element loop over the same five samples computed here (the data holds
// no NaN and no -0, so `<` orders it as the bank does), and no impulse may survive: |y| <= 1 everywhere.
// Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/rank_filter.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

namespace
{
constexpr std::uint32_t kWindow = 5;
constexpr std::uint64_t kChannels = 70;
constexpr std::uint64_t kBlocks[] = { 4, 0, 12, 1, 400, 83, 300 };

template <typename real_t> int run()
{
    std::uint64_t total = 0;
    for (std::uint64_t b : kBlocks)
        total += b;
    std::vector<real_t> x(kChannels * total);
    std::uint64_t impulses = 0;
    for (std::uint64_t c = 0; c < kChannels; c++)
        for (std::uint64_t n = 0; n < total; n++) {
            double v = std::sin(0.01 * static_cast<double>(c + 3) * static_cast<double>(n) + 0.5);
            if ((n + 3 * c) % 11 == 7) { // isolated: ten clean samples between two impulses
                v += (n / 11) % 2 ? -100.0 : 100.0;
                impulses++;
            }
            x[c * total + n] = static_cast<real_t>(v);
        }
    sdsp::rank_filter_bank<real_t> bank(kChannels, kWindow, sdsp::rank_filter_bank<real_t>::median_rank(kWindow));
    std::vector<real_t> y(kChannels * total);
    std::uint64_t s0 = 0;
    for (std::uint64_t blk : kBlocks) {
        std::vector<real_t> bx(kChannels * blk), by(kChannels * blk);
        for (std::uint64_t c = 0; c < kChannels; c++)
            std::copy_n(&x[c * total + s0], blk, &bx[c * blk]);
        bank.process_host(bx.data(), by.data(), blk);
        for (std::uint64_t c = 0; c < kChannels; c++)
            std::copy_n(&by[c * blk], blk, &y[c * total + s0]);
        s0 += blk;
    }
    std::uint64_t wrong = 0, survived = 0;
    for (std::uint64_t c = 0; c < kChannels; c++)
        for (std::uint64_t n = 0; n < total; n++) {
            real_t w[kWindow];
            for (std::uint32_t t = 0; t < kWindow; t++) // zeros in front of the stream
                w[t] = n >= t ? x[c * total + n - t] : real_t(0);
            std::nth_element(w, w + (kWindow - 1) / 2, w + kWindow);
            const real_t want = w[(kWindow - 1) / 2], got = y[c * total + n];
            wrong += std::memcmp(&want, &got, sizeof(real_t)) != 0 ? 1u : 0u;
            survived += std::fabs(static_cast<double>(got)) > 1.0 ? 1u : 0u;
        }
    // the carried history is the stream's last window - 1 samples, newest first
    const std::vector<real_t> h = bank.history();
    std::uint64_t stale = 0;
    for (std::uint64_t c = 0; c < kChannels; c++)
        for (std::uint32_t j = 0; j + 1 < kWindow; j++)
            stale += std::memcmp(&h[c * (kWindow - 1) + j], &x[c * total + total - 1 - j], sizeof(real_t)) != 0 ? 1u : 0u;
    const sdsp_hip_rank_plan_info info = bank.info();
    std::printf("rank_filter_bank<%s>: %llu channels, window %u, rank %u, padded %u, block %u, lds %u, kernel %s, %llu impulses, "
                "%llu outputs differ, %llu impulses survived, %llu history elements differ\n",
                sizeof(real_t) == 8 ? "double" : "float", static_cast<unsigned long long>(info.channels), info.window, info.rank,
                info.padded, info.block, info.lds_bytes, info.kernel, static_cast<unsigned long long>(impulses),
                static_cast<unsigned long long>(wrong), static_cast<unsigned long long>(survived), static_cast<unsigned long long>(stale));
    return impulses > 0 && wrong == 0 && survived == 0 && stale == 0 ? 0 : 1;
}
} // namespace

int main()
{
    try {
        const int rc = run<float>() | run<double>();
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &ex) {
        std::printf("no usable device: %s\n", ex.what());
        return 3;
    }
}
