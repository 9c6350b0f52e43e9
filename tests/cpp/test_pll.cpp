// sdsp::pll_bank (include/sdsp/pll.h) on carrier recovery: every channel is a unit tone at 0.1 + df cycles per sample (df uniform in
// +-0.4 bn, bn = 0.01) with a random start phase and Gaussian noise of 0.05 per component, streamed block by block through the host
// entry (empty and one-sample blocks included) with the gains of sdsp_hip_pll_gains(bn).  Over the last 1000 of 6000 samples the mean
// of freq must be within 0.01 bn of df and the angle of the mean of y within 0.02 rad (the bounds of tests/test_pll_host.py), and every
// err[n] must match a double loop computed here: the contract's recursion with every operation in double on the doubles of
// sdsp_hip_pll_oscillator.  For double that loop is the contract itself, so err must be equal; for float the tolerance kErrTolF32 is
// twice the largest deviation measured on an MI355X (it comes from the f32 tables and products, about 2^-23 per operation on values
// near 1, and from oscillator steps of 2^-22 cycle taken a sample apart once a rounded advance differs by a unit).
// Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/pll.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
constexpr std::uint64_t kChannels = 70;
constexpr std::uint64_t kBlocks[] = { 4, 0, 12, 1, 400, 83, 5500 };
constexpr std::uint64_t kTail = 1000;
constexpr double kBn = 0.01, kF0 = 0.1, kNoise = 0.05, kMaxDev = 0.5;
constexpr double kTwoPi = 6.283185307179586476925286766559;
constexpr double kErrTolF32 = 2.0 * 1.807e-6; // twice the 1.807e-6 measured on an MI355X (double: 0); DESIGN.md section 5.28

template <typename real_t> int run()
{
    std::mt19937 gen(23);
    std::normal_distribution<double> noise(0.0, kNoise);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    std::uint64_t total = 0;
    for (std::uint64_t b : kBlocks)
        total += b;
    std::uint32_t fcw = 0;
    sdsp::detail::check(sdsp_hip_ddc_phase_word(kF0, &fcw));
    const double centre = static_cast<double>(fcw) / 4294967296.0;
    double alpha = 0.0, beta = 0.0;
    sdsp::detail::check(sdsp_hip_pll_gains(kBn, std::sqrt(0.5), 1.0, SDSP_HIP_PLL_CROSS, &alpha, &beta));
    std::vector<double> df(kChannels);
    std::vector<real_t> x(kChannels * total * 2);
    for (std::uint64_t c = 0; c < kChannels; c++) {
        df[c] = (2.0 * unit(gen) - 1.0) * 0.4 * kBn;
        const double ph = kTwoPi * unit(gen);
        for (std::uint64_t n = 0; n < total; n++) {
            const double a = kTwoPi * (kF0 + df[c]) * static_cast<double>(n) + ph;
            x[2 * (c * total + n)] = static_cast<real_t>(std::cos(a) + noise(gen));
            x[2 * (c * total + n) + 1] = static_cast<real_t>(std::sin(a) + noise(gen));
        }
    }
    sdsp::pll_bank<real_t> bank(kChannels, SDSP_HIP_PLL_CROSS, fcw, kMaxDev);
    std::vector<real_t> y(kChannels * total * 2), err(kChannels * total), freq(kChannels * total);
    std::uint64_t s0 = 0;
    for (std::uint64_t blk : kBlocks) {
        std::vector<real_t> bx(kChannels * blk * 2), by(kChannels * blk * 2), be(kChannels * blk), bf(kChannels * blk);
        for (std::uint64_t c = 0; c < kChannels; c++)
            std::copy_n(&x[2 * (c * total + s0)], 2 * blk, &bx[2 * c * blk]);
        bank.process_host(bx.data(), by.data(), be.data(), bf.data(), blk, alpha, beta);
        for (std::uint64_t c = 0; c < kChannels; c++) {
            std::copy_n(&by[2 * c * blk], 2 * blk, &y[2 * (c * total + s0)]);
            std::copy_n(&be[c * blk], blk, &err[c * total + s0]);
            std::copy_n(&bf[c * blk], blk, &freq[c * total + s0]);
        }
        s0 += blk;
    }
    // lock: the tracked frequency and the residual phase over the tail
    double f_err = 0.0, angle = 0.0;
    for (std::uint64_t c = 0; c < kChannels; c++) {
        double fm = 0.0, yr = 0.0, yi = 0.0;
        for (std::uint64_t n = total - kTail; n < total; n++) {
            fm += static_cast<double>(freq[c * total + n]);
            yr += static_cast<double>(y[2 * (c * total + n)]);
            yi += static_cast<double>(y[2 * (c * total + n) + 1]);
        }
        f_err = std::max(f_err, std::fabs(fm / static_cast<double>(kTail) - (kF0 + df[c] - centre)));
        angle = std::max(angle, std::fabs(std::atan2(yi, yr)));
    }
    // the contract's recursion in double
    std::vector<double> coarse(2 * 2048), fine(2 * 2048);
    sdsp::detail::check(sdsp_hip_pll_oscillator(coarse.data(), fine.data()));
    const double a_r = static_cast<double>(static_cast<real_t>(alpha)), b_r = static_cast<double>(static_cast<real_t>(beta));
    double e_dev = 0.0;
    for (std::uint64_t c = 0; c < kChannels; c++) {
        std::uint32_t theta = 0;
        double integ = 0.0;
        for (std::uint64_t n = 0; n < total; n++) {
            const std::uint32_t ia = theta >> 21, ib = (theta >> 10) & 0x7ffu;
            const std::complex<double> cw(coarse[2 * ia], coarse[2 * ia + 1]), fw(fine[2 * ib], fine[2 * ib + 1]);
            const double wr = cw.real() * fw.real() - cw.imag() * fw.imag(), wi = cw.real() * fw.imag() + cw.imag() * fw.real();
            const double xr = static_cast<double>(x[2 * (c * total + n)]), xi = static_cast<double>(x[2 * (c * total + n) + 1]);
            const double e = xr * wi + xi * wr; // CROSS: the imaginary part of x (x) w
            integ = b_r * e + integ;
            integ = integ < -kMaxDev ? -kMaxDev : (integ > kMaxDev ? kMaxDev : integ);
            double t = (a_r * e + integ) * 4294967296.0;
            t = t < -2147483648.0 ? -2147483648.0 : (t > 2147483647.0 ? 2147483647.0 : t);
            theta += fcw + static_cast<std::uint32_t>(static_cast<std::int32_t>(std::nearbyint(t)));
            e_dev = std::max(e_dev, std::fabs(static_cast<double>(err[c * total + n]) - e));
        }
    }
    const bool f64 = sizeof(real_t) == 8;
    const sdsp_hip_pll_plan_info info = bank.info();
    std::printf("pll_bank<%s>: %llu channels, block %u, waves %u, lds %u, kernel %s, |mean(freq) - df| %.3e bn, angle %.3e rad, "
                "max |err - double loop| %.3e\n",
                f64 ? "double" : "float", static_cast<unsigned long long>(info.channels), info.block, info.waves, info.lds_bytes,
                info.kernel, f_err / kBn, angle, e_dev);
    // state round trip, then a fresh start
    const std::vector<real_t> fr = bank.freq();
    const std::vector<std::uint32_t> ph = bank.phase();
    bank.reset();
    bool same = bank.freq() == std::vector<real_t>(kChannels, real_t(0)) && bank.phase() == std::vector<std::uint32_t>(kChannels, 0u);
    bank.set_freq(fr);
    bank.set_phase(ph);
    same = same && bank.freq() == fr && bank.phase() == ph;
    const bool locked = f_err <= 0.01 * kBn && angle <= 0.02;
    const bool close = f64 ? e_dev == 0.0 : e_dev <= kErrTolF32;
    return locked && close && same ? 0 : 1;
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
