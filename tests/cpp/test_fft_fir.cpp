// sdsp::fft_fir_bank against sdsp::fir_bank of the same filter (include/sdsp/fir.h): block-by-block on the host entry,
// output within 1e-5 of the direct form (normwise per channel), history equal.  Exit 0 = pass, 1 = mismatch, 3 = no usable
// device (the library has no CPU fallback).
#include <sdsp/fir.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
constexpr size_t kTaps = 2049;
constexpr std::uint64_t kChannels = 6;
constexpr std::uint64_t kSamples = 9000;

template <typename real_t> int run(double tol)
{
    std::mt19937 gen(42);
    std::normal_distribution<double> dist(0.0, 1.0);
    std::array<double, kTaps> h{};
    for (auto &v : h)
        v = dist(gen) / std::sqrt(static_cast<double>(kTaps));
    std::vector<real_t> x(kChannels * kSamples);
    for (auto &v : x)
        v = static_cast<real_t>(dist(gen));
    std::vector<real_t> a = x, b = x;

    sdsp::fir_bank<kTaps, real_t> direct(kChannels);
    sdsp::fft_fir_bank<kTaps, real_t> fft(kChannels);
    direct.set_coeff(h);
    fft.set_coeff(h);
    direct.preload_filter(0.5);
    fft.preload_filter(0.5);
    direct.process_host(a.data(), kSamples);
    fft.process_host(b.data(), kSamples);
    const sdsp_hip_fir_plan_info info = fft.info();
    if (info.method != SDSP_HIP_FIR_FFT || info.fft_n < 2 * (kTaps - 1) || info.hop != info.fft_n - kTaps + 1) {
        std::printf("bad plan info: method %d fft_n %u hop %u\n", info.method, info.fft_n, info.hop);
        return 1;
    }
    double worst = 0.0;
    for (std::uint64_t c = 0; c < kChannels; c++) {
        double num = 0.0, den = 0.0;
        for (std::uint64_t s = 0; s < kSamples; s++) {
            const double want = static_cast<double>(a[c * kSamples + s]);
            num = std::max(num, std::fabs(static_cast<double>(b[c * kSamples + s]) - want));
            den = std::max(den, std::fabs(want));
        }
        worst = std::max(worst, num / den);
    }
    std::printf("fft_fir_bank<%zu, %s>: fft_n %u, kernel %s, rel err vs fir_bank %.3e\n", kTaps, sizeof(real_t) == 8 ? "double" : "float",
                info.fft_n, info.kernel, worst);
    return worst <= tol ? 0 : 1;
}
} // namespace

int main()
{
    try {
        const int rc = run<float>(1e-5) | run<double>(1e-12);
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &e) {
        std::printf("no usable device: %s\n", e.what());
        return 3;
    }
}
