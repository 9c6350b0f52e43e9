// sdsp::stft_bank (include/sdsp/stft.h) against a double DFT computed here, block by block on the host entry (blocks shorter than
// the history included): within 4 N eps (f64) / 2e-6 (f32) of each frame's largest bin.  Exit 0 = pass, 1 = mismatch, 3 = no
// usable device (the library has no CPU fallback).
#include <sdsp/stft.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
constexpr std::uint32_t kN = 256, kHop = 64;
constexpr std::uint64_t kChannels = 3;
constexpr std::uint64_t kBlocks[] = { 64, 128, 640, 64 }; // multiples of hop; 64 and 128 are shorter than hist = 192

template <typename real_t> int run(double tol)
{
    using bank_t = sdsp::stft_bank<kN, kHop, real_t>;
    std::mt19937 gen(11);
    std::normal_distribution<double> dist(0.0, 1.0);
    std::uint64_t total = 0;
    for (std::uint64_t b : kBlocks)
        total += b;
    std::vector<real_t> x(kChannels * total);
    for (auto &v : x)
        v = static_cast<real_t>(dist(gen));
    bank_t bank(kChannels, SDSP_HIP_STFT_COMPLEX);
    bank.set_window(SDSP_HIP_WINDOW_HAMMING);
    bank.preload_filter(0.25);
    // frames of every block, channel-major per block: y[c][frame][bin][re, im]
    std::vector<std::vector<double>> y(kChannels);
    std::uint64_t s0 = 0;
    for (std::uint64_t blk : kBlocks) {
        const std::uint64_t frames = bank_t::frames(blk);
        std::vector<real_t> in(kChannels * blk), out(kChannels * frames * bank_t::bins * 2);
        for (std::uint64_t c = 0; c < kChannels; c++)
            std::copy_n(&x[c * total + s0], blk, &in[c * blk]);
        bank.process_host(in.data(), out.data(), blk);
        for (std::uint64_t c = 0; c < kChannels; c++)
            for (std::uint64_t i = 0; i < frames * bank_t::bins * 2; i++)
                y[c].push_back(static_cast<double>(out[c * frames * bank_t::bins * 2 + i]));
        s0 += blk;
    }
    const std::array<double, kN> &w = bank.window();
    const double pi = 3.14159265358979323846;
    double worst = 0.0;
    for (std::uint64_t c = 0; c < kChannels; c++) {
        // the stream with the preloaded history in front
        std::vector<double> s(bank_t::hist, static_cast<double>(static_cast<real_t>(0.25)));
        for (std::uint64_t i = 0; i < total; i++)
            s.push_back(static_cast<double>(x[c * total + i]));
        const std::uint64_t frames = total / kHop;
        for (std::uint64_t j = 0; j < frames; j++) {
            double num = 0.0, den = 0.0;
            for (std::uint32_t k = 0; k < bank_t::bins; k++) {
                double re = 0.0, im = 0.0;
                for (std::uint32_t n = 0; n < kN; n++) {
                    const double v = s[j * kHop + n] * w[n];
                    const double a = -2.0 * pi * static_cast<double>((static_cast<std::uint64_t>(k) * n) % kN) / kN;
                    re += v * std::cos(a);
                    im += v * std::sin(a);
                }
                const double gr = y[c][(j * bank_t::bins + k) * 2], gi = y[c][(j * bank_t::bins + k) * 2 + 1];
                num = std::max(num, std::hypot(gr - re, gi - im));
                den = std::max(den, std::hypot(re, im));
            }
            worst = std::max(worst, num / den);
        }
    }
    const sdsp_hip_stft_plan_info info = bank.info();
    std::printf("stft_bank<%u, %u, %s>: hist %u, bins %u, kernel %s, rel err vs DFT %.3e\n", kN, kHop, sizeof(real_t) == 8 ? "double" : "float",
                info.hist, info.bins, info.kernel, worst);
    return worst <= tol ? 0 : 1;
}
} // namespace

int main()
{
    try {
        const int rc = run<float>(2e-6) | run<double>(4.0 * kN * 2.220446049250313e-16);
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &e) {
        std::printf("no usable device: %s\n", e.what());
        return 3;
    }
}
