// sdsp::welch_bank (include/sdsp/welch.h) against a double Welch estimate computed here (linear detrend, direct DFT), block by block
// on the host entry with blocks shorter than a segment and a hop that does not divide N: within 1e-12 (f64) / 2e-5 (f32) of each
// channel's largest bin.  Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/welch.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
constexpr std::uint32_t kN = 64, kHop = 24;
constexpr std::uint64_t kChannels = 3;
constexpr std::uint64_t kBlocks[] = { 10, 63, 1, 200, 24, 0, 77 };

template <typename real_t> int run(double tol)
{
    using bank_t = sdsp::welch_bank<kN, kHop, real_t>;
    std::mt19937 gen(5);
    std::normal_distribution<double> dist(0.0, 1.0);
    std::uint64_t total = 0;
    for (std::uint64_t b : kBlocks)
        total += b;
    std::vector<real_t> x(kChannels * total);
    for (std::uint64_t i = 0; i < x.size(); i++)
        x[i] = static_cast<real_t>(dist(gen) + 0.01 * static_cast<double>(i % total));
    const double fs = 100.0;
    bank_t bank(kChannels, SDSP_HIP_DETREND_LINEAR, SDSP_HIP_SCALING_DENSITY, fs);
    bank.set_window(SDSP_HIP_WINDOW_HAMMING);
    std::uint64_t s0 = 0;
    for (std::uint64_t blk : kBlocks) {
        std::vector<real_t> in(kChannels * blk);
        for (std::uint64_t c = 0; c < kChannels; c++)
            std::copy_n(&x[c * total + s0], blk, &in[c * blk]);
        bank.process_host(in.data(), blk);
        s0 += blk;
    }
    const std::uint64_t segs = (total - kN) / kHop + 1;
    if (bank.frames() != segs || bank.position() != total) {
        std::printf("segment count %llu, want %llu\n", static_cast<unsigned long long>(bank.frames()), static_cast<unsigned long long>(segs));
        return 1;
    }
    std::vector<real_t> out(kChannels * bank_t::bins);
    bank.psd_host(out.data());
    std::array<double, kN> w{};
    double sw2 = 0.0;
    for (std::uint32_t n = 0; n < kN; n++) {
        w[n] = static_cast<double>(static_cast<real_t>(bank.window()[n]));
        sw2 += w[n] * w[n];
    }
    const double pi = 3.14159265358979323846, mid = (kN - 1) / 2.0;
    double worst = 0.0;
    for (std::uint64_t c = 0; c < kChannels; c++) {
        std::vector<double> p(bank_t::bins, 0.0);
        for (std::uint64_t m = 0; m < segs; m++) {
            const real_t *seg = &x[c * total + m * kHop];
            double s0_ = 0.0, s1 = 0.0;
            for (std::uint32_t n = 0; n < kN; n++) {
                s0_ += static_cast<double>(seg[n]);
                s1 += (n - mid) * static_cast<double>(seg[n]);
            }
            const double mu = s0_ / kN, beta = s1 / (kN * (static_cast<double>(kN) * kN - 1) / 12);
            for (std::uint32_t k = 0; k < bank_t::bins; k++) {
                double re = 0.0, im = 0.0;
                for (std::uint32_t n = 0; n < kN; n++) {
                    const double v = (static_cast<double>(seg[n]) - mu - beta * (n - mid)) * w[n];
                    const double a = -2.0 * pi * static_cast<double>((static_cast<std::uint64_t>(k) * n) % kN) / kN;
                    re += v * std::cos(a);
                    im += v * std::sin(a);
                }
                p[k] += re * re + im * im;
            }
        }
        double num = 0.0, den = 0.0;
        for (std::uint32_t k = 0; k < bank_t::bins; k++) {
            const double want = p[k] * ((k == 0 || k == kN / 2) ? 1.0 : 2.0) / (fs * sw2) / static_cast<double>(segs);
            num = std::max(num, std::fabs(static_cast<double>(out[c * bank_t::bins + k]) - want));
            den = std::max(den, std::fabs(want));
        }
        worst = std::max(worst, num / den);
    }
    const sdsp_hip_welch_plan_info info = bank.info();
    std::printf("welch_bank<%u, %u, %s>: hist %u, bins %u, kernel %s, %llu segments, rel err vs double %.3e\n", kN, kHop,
                sizeof(real_t) == 8 ? "double" : "float", info.hist, info.bins, info.kernel, static_cast<unsigned long long>(segs), worst);
    return worst <= tol ? 0 : 1;
}
} // namespace

int main()
{
    try {
        const int rc = run<float>(2e-5) | run<double>(1e-12);
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &e) {
        std::printf("no usable device: %s\n", e.what());
        return 3;
    }
}
