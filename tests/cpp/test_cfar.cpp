// sdsp::cfar_bank (include/sdsp/cfar.h) as a detector: every channel is exponential noise (a fixed linear congruential generator
// through -log) with targets of 30 dB on top, streamed block by block through the host entry (empty and one-sample blocks included) of
// a CA bank on power rows, a GO bank on I/Q rows and an OS bank on power rows.  Every threshold and decision must equal, bit for bit, a
// loop over the same cells computed here in the contract's order (sums in ascending index from +0, one product; std::nth_element for
// OS: the data holds no NaN and no -0, so `<` orders it as the bank does), and every target must be found at its own cell.
// Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/cfar.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

namespace
{
constexpr std::uint32_t kTrain = 8, kGuard = 2, kHalf = kTrain + kGuard, kWindow = 2 * kHalf + 1;
constexpr std::uint64_t kChannels = 70;
constexpr std::uint64_t kBlocks[] = { 4, 0, 12, 1, 400, 83, 300 };
constexpr std::uint64_t kPeriod = 97; // one target per 97 cells and channel

struct noise {
    std::uint64_t s = 0x9E3779B97F4A7C15ull;
    double uniform() // in (0, 1)
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (static_cast<double>(s >> 11) + 0.5) / 9007199254740992.0;
    }
};

// one rounded product (never fused into a following sum)
template <typename real_t> real_t product(real_t a, real_t b)
{
    volatile real_t p = a * b;
    return p;
}

template <typename real_t> int run(sdsp::cfar_mode mode, sdsp::cfar_input input, double alpha, std::uint32_t rank, const char *name)
{
    const bool iq = input == sdsp::cfar_input::iq;
    const std::size_t per = iq ? 2 : 1;
    std::uint64_t total = 0;
    for (std::uint64_t b : kBlocks)
        total += b;
    noise gen;
    std::vector<real_t> x(kChannels * total * per), p(kChannels * total);
    std::uint64_t targets = 0;
    for (std::uint64_t c = 0; c < kChannels; c++)
        for (std::uint64_t n = 0; n < total; n++) {
            const bool target = (n + 5 * c) % kPeriod == 40 && n + kHalf < total && n >= kWindow;
            targets += target ? 1u : 0u;
            if (iq) {
                const double scale = target ? std::sqrt(1000.0) : std::sqrt(-std::log(gen.uniform()));
                const double phase = 6.283185307179586 * gen.uniform();
                const real_t re = static_cast<real_t>(scale * std::cos(phase)), im = static_cast<real_t>(scale * std::sin(phase));
                x[(c * total + n) * 2] = re;
                x[(c * total + n) * 2 + 1] = im;
                p[c * total + n] = product(re, re) + product(im, im);
            } else {
                const real_t v = static_cast<real_t>(target ? 1000.0 : -std::log(gen.uniform()));
                x[c * total + n] = v;
                p[c * total + n] = v;
            }
        }
    sdsp::cfar_bank<real_t> bank(kChannels, kTrain, kGuard, mode, alpha, rank, input);
    std::vector<real_t> thr(kChannels * total);
    std::vector<std::uint8_t> det(kChannels * total);
    std::uint64_t s0 = 0;
    for (std::uint64_t blk : kBlocks) {
        std::vector<real_t> bx(kChannels * blk * per), bt(kChannels * blk);
        std::vector<std::uint8_t> bd(kChannels * blk);
        for (std::uint64_t c = 0; c < kChannels; c++)
            std::copy_n(&x[(c * total + s0) * per], blk * per, bx.begin() + static_cast<std::ptrdiff_t>(c * blk * per));
        bank.process_host(bx.data(), bt.data(), bd.data(), blk);
        for (std::uint64_t c = 0; c < kChannels; c++) {
            std::copy_n(bt.begin() + static_cast<std::ptrdiff_t>(c * blk), blk, &thr[c * total + s0]);
            std::copy_n(bd.begin() + static_cast<std::ptrdiff_t>(c * blk), blk, &det[c * total + s0]);
        }
        s0 += blk;
    }
    const sdsp_hip_cfar_plan_info info = bank.info();
    const real_t scale = static_cast<real_t>(info.scale);
    std::uint64_t wrong_thr = 0, wrong_det = 0, found = 0, alarms = 0;
    for (std::uint64_t c = 0; c < kChannels; c++)
        for (std::uint64_t n = 0; n < total; n++) {
            auto cell = [&](std::uint64_t back) { return n >= back ? p[c * total + n - back] : real_t(0); }; // zeros in front
            real_t want;
            if (mode == sdsp::cfar_mode::os) {
                real_t w[2 * kTrain];
                for (std::uint32_t i = 0; i < kTrain; i++) {
                    w[i] = cell(kWindow - 1 - i);
                    w[kTrain + i] = cell(kTrain - 1 - i);
                }
                std::nth_element(w, w + rank, w + 2 * kTrain);
                want = product(w[rank], scale);
            } else {
                real_t lag = 0, lead = 0;
                for (std::uint32_t i = 0; i < kTrain; i++) {
                    lag = lag + cell(kWindow - 1 - i);
                    lead = lead + cell(kTrain - 1 - i);
                }
                const real_t v = mode == sdsp::cfar_mode::ca ? lag + lead : mode == sdsp::cfar_mode::go ? (lag > lead ? lag : lead)
                                                                                                        : (lag < lead ? lag : lead);
                want = product(v, scale);
            }
            const std::uint8_t want_det = cell(kHalf) > want ? 1 : 0;
            wrong_thr += std::memcmp(&want, &thr[c * total + n], sizeof(real_t)) != 0 ? 1u : 0u;
            wrong_det += want_det != det[c * total + n] ? 1u : 0u;
            if (n >= kHalf && p[c * total + n - kHalf] >= real_t(900)) // the decision about cell n - half arrives with sample n
                found += det[c * total + n];
            else
                alarms += det[c * total + n];
        }
    // the carried history is the stream's last window - 1 elements, newest first
    const std::vector<real_t> h = bank.history();
    std::uint64_t stale = 0;
    for (std::uint64_t c = 0; c < kChannels; c++)
        for (std::uint32_t j = 0; j + 1 < kWindow; j++)
            stale += std::memcmp(&h[(c * (kWindow - 1) + j) * per], &x[(c * total + total - 1 - j) * per], sizeof(real_t) * per) != 0 ? 1u : 0u;
    std::printf("cfar_bank<%s> %s: %llu channels, train %u, guard %u, window %u, rank %u, padded %u, block %u, lds %u, kernel %s, "
                "%llu of %llu targets found, %llu alarms elsewhere, %llu thresholds differ, %llu decisions differ, %llu history "
                "elements differ\n",
                sizeof(real_t) == 8 ? "double" : "float", name, static_cast<unsigned long long>(info.channels), info.train, info.guard,
                info.window, info.rank, info.padded, info.block, info.lds_bytes, info.kernel, static_cast<unsigned long long>(found),
                static_cast<unsigned long long>(targets), static_cast<unsigned long long>(alarms),
                static_cast<unsigned long long>(wrong_thr), static_cast<unsigned long long>(wrong_det),
                static_cast<unsigned long long>(stale));
    return targets > 0 && found == targets && wrong_thr == 0 && wrong_det == 0 && stale == 0 ? 0 : 1;
}

template <typename real_t> int run_all()
{
    const double n = 2.0 * kTrain;
    const double ca_alpha = n * (std::pow(1e-4, -1.0 / n) - 1.0); // the CA designer for pfa = 1e-4
    return run<real_t>(sdsp::cfar_mode::ca, sdsp::cfar_input::power, ca_alpha, 0, "ca power")
           | run<real_t>(sdsp::cfar_mode::go, sdsp::cfar_input::iq, 20.0, 0, "go iq")
           | run<real_t>(sdsp::cfar_mode::os, sdsp::cfar_input::power, 15.0, sdsp::cfar_bank<real_t>::default_rank(kTrain), "os power");
}
} // namespace

int main()
{
    try {
        const int rc = run_all<float>() | run_all<double>();
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &ex) {
        std::printf("no usable device: %s\n", ex.what());
        return 3;
    }
}
