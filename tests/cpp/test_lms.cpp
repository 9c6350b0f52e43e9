// sdsp::lms_bank (include/sdsp/lms.h) on a system identification: every channel's d is its own known 8-tap system applied to white x,
// streamed block by block through the host entry (empty and one-sample blocks included).  NLMS at mu = 1 for 2000 samples must end
// with max |w - h| <= 2e-6 in float (the bound of tests/test_lms_host.py; 1e-12 in double), and over the first 64 samples every e[n]
// must match a double loop computed here (the same recursion with every operation in double) within 64 u S, u the unit roundoff of
// the precision and S the largest sum |w[t]| |x[n - t]| + |d[n]| the channel has seen so far: T + 2 = 10 roundings of the chain and
// the subtraction, and the weights' own error, which an NLMS step at mu = 1 does not amplify, over a few filter lengths.
// Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/lms.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
constexpr std::uint32_t kTaps = 8;
constexpr std::uint64_t kChannels = 70;
constexpr std::uint64_t kBlocks[] = { 4, 0, 12, 1, 400, 83, 1500 };
constexpr double kMu = 1.0, kEps = 1e-6;

template <typename real_t> int run()
{
    std::mt19937 gen(17);
    std::normal_distribution<double> dist(0.0, 1.0);
    std::uint64_t total = 0;
    for (std::uint64_t b : kBlocks)
        total += b;
    std::vector<double> h(kChannels * kTaps);
    for (double &v : h)
        v = dist(gen);
    std::vector<real_t> x(kChannels * total), d(kChannels * total);
    for (real_t &v : x)
        v = static_cast<real_t>(dist(gen));
    for (std::uint64_t c = 0; c < kChannels; c++)
        for (std::uint64_t n = 0; n < total; n++) {
            double acc = 0.0;
            for (std::uint32_t t = 0; t < kTaps && t <= n; t++)
                acc += h[c * kTaps + t] * static_cast<double>(x[c * total + n - t]);
            d[c * total + n] = static_cast<real_t>(acc);
        }
    sdsp::lms_bank<real_t> bank(kChannels, kTaps, false, true, kEps);
    std::vector<real_t> e(kChannels * total);
    std::uint64_t s0 = 0;
    for (std::uint64_t blk : kBlocks) {
        std::vector<real_t> bx(kChannels * blk), bd(kChannels * blk), be(kChannels * blk);
        for (std::uint64_t c = 0; c < kChannels; c++) {
            std::copy_n(&x[c * total + s0], blk, &bx[c * blk]);
            std::copy_n(&d[c * total + s0], blk, &bd[c * blk]);
        }
        bank.process_host(bx.data(), bd.data(), nullptr, be.data(), blk, kMu); // y is left out
        for (std::uint64_t c = 0; c < kChannels; c++)
            std::copy_n(&be[c * blk], blk, &e[c * total + s0]);
        s0 += blk;
    }
    // the identified systems
    const std::vector<real_t> w = bank.weights();
    double werr = 0.0;
    for (std::size_t i = 0; i < w.size(); i++)
        werr = std::max(werr, std::fabs(static_cast<double>(w[i]) - h[i]));
    // the same recursion in double on the first samples
    const std::uint64_t head = 64;
    const double u = sizeof(real_t) == 8 ? std::ldexp(1.0, -53) : std::ldexp(1.0, -24);
    double eerr = 0.0; // error / bound
    for (std::uint64_t c = 0; c < kChannels; c++) {
        double wd[kTaps] = {}, scale = 0.0;
        for (std::uint64_t n = 0; n < head; n++) {
            double y = 0.0, p = 0.0, mag = std::fabs(static_cast<double>(d[c * total + n]));
            for (std::uint32_t t = 0; t < kTaps && t <= n; t++) {
                const double v = static_cast<double>(x[c * total + n - t]);
                y += wd[t] * v;
                p += v * v;
                mag += std::fabs(wd[t] * v);
            }
            scale = std::max(scale, mag);
            const double err = static_cast<double>(d[c * total + n]) - y;
            const double g = kMu * err / (static_cast<double>(static_cast<real_t>(kEps)) + p);
            for (std::uint32_t t = 0; t < kTaps && t <= n; t++)
                wd[t] += g * static_cast<double>(x[c * total + n - t]);
            eerr = std::max(eerr, std::fabs(static_cast<double>(e[c * total + n]) - err) / (64.0 * u * scale));
        }
    }
    const bool f64 = sizeof(real_t) == 8;
    const sdsp_hip_lms_plan_info info = bank.info();
    std::printf("lms_bank<%s>: %llu channels, %u taps, block %u, lds %u, kernel %s, max |w - h| %.3e, e: err / bound %.3f\n",
                f64 ? "double" : "float", static_cast<unsigned long long>(info.channels), info.taps, info.block, info.lds_bytes, info.kernel,
                werr, eerr);
    // set_weights round trip
    bank.set_weights(w);
    const bool same = bank.weights() == w;
    return werr <= (f64 ? 1e-12 : 2e-6) && eerr <= 1.0 && same ? 0 : 1;
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
