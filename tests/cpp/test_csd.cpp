// sdsp::csd_bank (include/sdsp/csd.h) against double cross spectra computed here (linear detrend, direct DFT), block by block on the
// host entry with blocks shorter than a segment and a hop that does not divide N.  The cross-spectral density is held within 1e-12
// (f64) / 2e-5 (f32) of each pair's largest bin; the coherence within 1e-12 (f64), and in f32 within the first-order bound that
// follows from 2e-5 on the three spectra: 2e-5 (2 max|Pxy| / sqrt(Pxx_k Pyy_k) + max Pxx / Pxx_k + max Pyy / Pyy_k) per bin.
// Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/csd.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
constexpr std::uint32_t kN = 64, kHop = 24;
constexpr std::uint64_t kChannels = 3;
constexpr std::uint64_t kBlocks[] = { 10, 63, 1, 200, 24, 0, 77, 300 };

template <typename real_t> int run(double tol)
{
    using bank_t = sdsp::csd_bank<kN, kHop, real_t>;
    constexpr std::uint32_t bins = bank_t::bins;
    const std::vector<std::pair<std::uint32_t, std::uint32_t>> pairs = { { 0, 1 }, { 0, 2 }, { 2, 2 }, { 1, 0 } };
    std::mt19937 gen(5);
    std::normal_distribution<double> dist(0.0, 1.0);
    std::uint64_t total = 0;
    for (std::uint64_t b : kBlocks)
        total += b;
    // channels 0 and 1 share a component; channel 2 is channel 0 through a two-tap filter plus a little noise
    std::vector<real_t> x(kChannels * total);
    for (std::uint64_t i = 0; i < total; i++) {
        const double common = dist(gen), ramp = 0.001 * static_cast<double>(i);
        const double x0 = dist(gen) + 0.8 * common + ramp;
        x[i] = static_cast<real_t>(x0);
        x[total + i] = static_cast<real_t>(dist(gen) + 0.8 * common - ramp);
        x[2 * total + i] = static_cast<real_t>(0.6 * x0 + (i ? 0.3 * static_cast<double>(x[i - 1]) : 0.0) + 0.05 * dist(gen));
    }
    const double fs = 100.0;
    bank_t bank(kChannels, pairs, SDSP_HIP_DETREND_LINEAR, SDSP_HIP_SCALING_DENSITY, fs);
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
    if (bank.frames() != segs || bank.position() != total || bank.npairs() != pairs.size()) {
        std::printf("segment count %llu, want %llu\n", static_cast<unsigned long long>(bank.frames()), static_cast<unsigned long long>(segs));
        return 1;
    }
    std::vector<real_t> out(pairs.size() * 2 * bins), coh(pairs.size() * bins);
    bank.csd_host(out.data());
    bank.coherence_host(coh.data());
    std::array<double, kN> w{};
    double sw2 = 0.0;
    for (std::uint32_t n = 0; n < kN; n++) {
        w[n] = static_cast<double>(static_cast<real_t>(bank.window()[n]));
        sw2 += w[n] * w[n];
    }
    // every segment's spectrum in double, then the sums
    const double pi = 3.14159265358979323846, mid = (kN - 1) / 2.0;
    std::vector<std::complex<double>> z(kChannels * segs * bins);
    for (std::uint64_t c = 0; c < kChannels; c++)
        for (std::uint64_t m = 0; m < segs; m++) {
            const real_t *seg = &x[c * total + m * kHop];
            double sum0 = 0.0, sum1 = 0.0;
            for (std::uint32_t n = 0; n < kN; n++) {
                sum0 += static_cast<double>(seg[n]);
                sum1 += (n - mid) * static_cast<double>(seg[n]);
            }
            const double mu = sum0 / kN, beta = sum1 / (kN * (static_cast<double>(kN) * kN - 1) / 12);
            for (std::uint32_t k = 0; k < bins; k++) {
                double re = 0.0, im = 0.0;
                for (std::uint32_t n = 0; n < kN; n++) {
                    const double v = (static_cast<double>(seg[n]) - mu - beta * (n - mid)) * w[n];
                    const double a = -2.0 * pi * static_cast<double>((static_cast<std::uint64_t>(k) * n) % kN) / kN;
                    re += v * std::cos(a);
                    im += v * std::sin(a);
                }
                z[(c * segs + m) * bins + k] = { re, im };
            }
        }
    std::vector<double> au(kChannels * bins, 0.0);
    for (std::uint64_t c = 0; c < kChannels; c++)
        for (std::uint64_t m = 0; m < segs; m++)
            for (std::uint32_t k = 0; k < bins; k++)
                au[c * bins + k] += std::norm(z[(c * segs + m) * bins + k]);
    double worst = 0.0, worst_coh = 0.0;
    bool coh_ok = true;
    for (std::size_t i = 0; i < pairs.size(); i++) {
        const std::uint64_t a = pairs[i].first, b = pairs[i].second;
        std::vector<std::complex<double>> p(bins);
        for (std::uint64_t m = 0; m < segs; m++)
            for (std::uint32_t k = 0; k < bins; k++)
                p[k] += std::conj(z[(a * segs + m) * bins + k]) * z[(b * segs + m) * bins + k];
        double num = 0.0, den = 0.0, amax = 0.0, bmax = 0.0;
        for (std::uint32_t k = 0; k < bins; k++) {
            const std::complex<double> want = p[k] * (((k == 0 || k == kN / 2) ? 1.0 : 2.0) / (fs * sw2) / static_cast<double>(segs));
            const std::complex<double> got(static_cast<double>(out[(i * bins + k) * 2]), static_cast<double>(out[(i * bins + k) * 2 + 1]));
            num = std::max(num, std::abs(got - want));
            den = std::max(den, std::abs(want));
            amax = std::max(amax, au[a * bins + k]);
            bmax = std::max(bmax, au[b * bins + k]);
        }
        worst = std::max(worst, num / den);
        double pmax = 0.0;
        for (std::uint32_t k = 0; k < bins; k++)
            pmax = std::max(pmax, std::abs(p[k]));
        for (std::uint32_t k = 0; k < bins; k++) {
            const double pa = au[a * bins + k], pb = au[b * bins + k];
            const double want = std::norm(p[k]) / (pa * pb);
            const double err = std::fabs(static_cast<double>(coh[i * bins + k]) - want);
            const double bound = sizeof(real_t) == 8 ? 1e-12 : 2e-5 * (2.0 * pmax / std::sqrt(pa * pb) + amax / pa + bmax / pb);
            worst_coh = std::max(worst_coh, err);
            coh_ok = coh_ok && err <= bound;
        }
    }
    const sdsp_hip_csd_plan_info info = bank.info();
    std::printf("csd_bank<%u, %u, %s>: hist %u, bins %u, kernel %s, %llu segments, %llu pairs, csd rel err vs double %.3e, "
                "coherence abs err %.3e\n",
                kN, kHop, sizeof(real_t) == 8 ? "double" : "float", info.hist, info.bins, info.kernel,
                static_cast<unsigned long long>(segs), static_cast<unsigned long long>(info.npairs), worst, worst_coh);
    return worst <= tol && coh_ok ? 0 : 1;
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
