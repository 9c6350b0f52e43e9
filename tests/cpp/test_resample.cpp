// sdsp::fir_resampler_bank (include/sdsp/resample.h) against a double reference computed here, block by block on the host entry:
// f64 bit for bit, f32 within 1e-6 normwise per channel.  Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no
// CPU fallback).
#include <sdsp/resample.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
constexpr size_t kTaps = 65;
constexpr std::uint32_t kUp = 3, kDown = 2;
constexpr std::uint64_t kChannels = 5;
constexpr std::uint64_t kBlock = 600; // a multiple of q = 2
constexpr int kBlocks = 3;

// y[m] = sum over k with (m D - k) = 0 (mod U) of h[k] x[(m D - k) / U], ascending k, history x[-1 - j] = hist[j]
std::vector<double> reference(const std::array<double, kTaps> &h, const std::vector<double> &x, double preload)
{
    const std::uint64_t outs = x.size() * kUp / kDown;
    std::vector<double> y(outs, 0.0);
    for (std::uint64_t m = 0; m < outs; m++) {
        const std::uint64_t n = m * kDown;
        bool first = true;
        double acc = 0.0;
        for (std::uint64_t k = n % kUp; k < kTaps; k += kUp) {
            const std::int64_t xi = static_cast<std::int64_t>(n / kUp) - static_cast<std::int64_t>((k - n % kUp) / kUp);
            const double v = xi >= 0 ? x[static_cast<size_t>(xi)] : preload;
            acc = first ? h[k] * v : acc + h[k] * v;
            first = false;
        }
        y[m] = acc;
    }
    return y;
}

template <typename real_t> int run(double tol)
{
    std::mt19937 gen(7);
    std::normal_distribution<double> dist(0.0, 1.0);
    std::array<double, kTaps> h{};
    for (auto &v : h)
        v = dist(gen) / 8.0;
    std::vector<real_t> x(kChannels * kBlock * kBlocks);
    for (auto &v : x)
        v = static_cast<real_t>(dist(gen));
    using bank_t = sdsp::fir_resampler_bank<kTaps, kUp, kDown, real_t>;
    bank_t bank(kChannels);
    bank.set_coeff(h);
    bank.preload_filter(0.25);
    const std::uint64_t outs = bank_t::out_samples(kBlock);
    std::vector<real_t> y(kChannels * outs * kBlocks);
    for (int b = 0; b < kBlocks; b++) {
        std::vector<real_t> in(kChannels * kBlock), out(kChannels * outs);
        for (std::uint64_t c = 0; c < kChannels; c++)
            std::copy_n(&x[(c * kBlocks + static_cast<std::uint64_t>(b)) * kBlock], kBlock, &in[c * kBlock]);
        bank.process_host(in.data(), out.data(), kBlock);
        for (std::uint64_t c = 0; c < kChannels; c++)
            std::copy_n(&out[c * outs], outs, &y[(c * kBlocks + static_cast<std::uint64_t>(b)) * outs]);
    }
    const sdsp_hip_resample_plan_info info = bank.info();
    double worst = 0.0;
    for (std::uint64_t c = 0; c < kChannels; c++) {
        std::vector<double> xc(kBlock * kBlocks);
        for (size_t i = 0; i < xc.size(); i++)
            xc[i] = static_cast<double>(x[c * kBlock * kBlocks + i]);
        std::array<double, kTaps> hs{};
        for (size_t k = 0; k < kTaps; k++)
            hs[k] = static_cast<double>(static_cast<real_t>(h[k]));
        const std::vector<double> want = reference(hs, xc, static_cast<double>(static_cast<real_t>(0.25)));
        double num = 0.0, den = 0.0;
        for (size_t m = 0; m < want.size(); m++) {
            num = std::max(num, std::fabs(static_cast<double>(y[c * want.size() + m]) - want[m]));
            den = std::max(den, std::fabs(want[m]));
        }
        worst = std::max(worst, num / den);
    }
    std::printf("fir_resampler_bank<%zu, %u, %u, %s>: hist %u, kernel %s, rel err vs reference %.3e\n", kTaps, kUp, kDown,
                sizeof(real_t) == 8 ? "double" : "float", info.hist, info.kernel, worst);
    return worst <= tol ? 0 : 1;
}
} // namespace

int main()
{
    try {
        const int rc = run<float>(1e-6) | run<double>(0.0);
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &e) {
        std::printf("no usable device: %s\n", e.what());
        return 3;
    }
}
