// sdsp::ddc_bank (include/sdsp/ddc.h) against a double mix -> FIR -> decimate computed here, block by block on the host entry with
// blocks shorter than the history: real and complex input, several bands on one channel and a channel without bands.  f64 is held
// within 1e-12 sum|h| max|x| of the double result, f32 within 1e-6 of each band's largest output.
// Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/ddc.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
constexpr std::uint32_t kTaps = 65, kDown = 4, kChannels = 3;
constexpr std::uint64_t kBlocks[] = { 4, 0, 12, 400, 8, 1200, 36 };

template <typename real_t> int run(bool cplx, double tol, bool absolute)
{
    const std::vector<sdsp_hip_ddc_band> bands = { { 0, sdsp::ddc_phase_word(0.123), 0 },
                                                   { 2, sdsp::ddc_phase_word(-0.31), sdsp::ddc_phase_word(0.25) },
                                                   { 0, 0x80000000u, 17 },
                                                   { 0, 0, 0 } };
    std::mt19937 gen(11);
    std::normal_distribution<double> dist(0.0, 1.0);
    std::uint64_t total = 0;
    for (std::uint64_t b : kBlocks)
        total += b;
    const std::size_t width = cplx ? 2 : 1;
    std::vector<real_t> x(kChannels * total * width);
    for (real_t &v : x)
        v = static_cast<real_t>(dist(gen));
    sdsp::ddc_bank<real_t> bank(kTaps, kDown, bands, kChannels, cplx);
    bank.set_antialias_coeff();
    const std::uint64_t pos0 = (1ull << 32) - 100 * kDown; // the phase index wraps inside the stream
    bank.set_position(pos0);
    const std::uint64_t outs = total / kDown;
    std::vector<real_t> y(bands.size() * outs * 2);
    std::uint64_t s0 = 0;
    for (std::uint64_t blk : kBlocks) {
        std::vector<real_t> in(kChannels * blk * width), out(bands.size() * (blk / kDown) * 2);
        for (std::uint64_t c = 0; c < kChannels; c++)
            std::copy_n(&x[(c * total + s0) * width], blk * width, &in[c * blk * width]);
        bank.process_host(in.data(), out.data(), blk);
        for (std::size_t i = 0; i < bands.size(); i++)
            std::copy_n(&out[i * (blk / kDown) * 2], (blk / kDown) * 2, &y[(i * outs + s0 / kDown) * 2]);
        s0 += blk;
    }
    if (bank.position() != pos0 + total)
        return 1;
    const double two_pi = 6.283185307179586476925286766559;
    double hsum = 0.0, xmax = 0.0;
    std::vector<double> h(kTaps);
    for (std::uint32_t k = 0; k < kTaps; k++) {
        h[k] = static_cast<double>(static_cast<real_t>(bank.coeff()[k]));
        hsum += std::fabs(h[k]);
    }
    for (real_t v : x)
        xmax = std::max(xmax, std::fabs(static_cast<double>(v)));
    double worst = 0.0;
    for (std::size_t i = 0; i < bands.size(); i++) {
        const sdsp_hip_ddc_band &b = bands[i];
        double err = 0.0, ymax = 0.0;
        for (std::uint64_t m = 0; m < outs; m++) {
            std::complex<double> acc = 0.0;
            for (std::uint32_t k = 0; k < kTaps && k <= m * kDown; k++) {
                const std::uint64_t n = m * kDown - k;
                const real_t *p = &x[(b.src * total + n) * width];
                const std::complex<double> xv(static_cast<double>(p[0]), cplx ? static_cast<double>(p[1]) : 0.0);
                const std::uint32_t j = b.phase0 + b.fcw * static_cast<std::uint32_t>(pos0 + n);
                acc += h[k] * xv * std::polar(1.0, -two_pi * static_cast<double>(j) / 4294967296.0);
            }
            const std::complex<double> got(static_cast<double>(y[(i * outs + m) * 2]), static_cast<double>(y[(i * outs + m) * 2 + 1]));
            err = std::max(err, std::abs(got - acc));
            ymax = std::max(ymax, std::abs(acc));
        }
        worst = std::max(worst, absolute ? err / (hsum * xmax) : err / ymax);
    }
    const sdsp_hip_ddc_plan_info info = bank.info();
    std::printf("ddc_bank<%s> %s input: %u taps, down %u, %u bands, hist %u, block %u, kernel %s, err %.3e (bound %.0e)\n",
                sizeof(real_t) == 8 ? "double" : "float", cplx ? "complex" : "real", info.taps, info.down, info.bands, info.hist,
                info.block_out, info.kernel, worst, tol);
    return worst <= tol ? 0 : 1;
}
} // namespace

int main()
{
    try {
        const int rc = run<float>(false, 1e-6, false) | run<float>(true, 1e-6, false) | run<double>(false, 1e-12, true) |
                       run<double>(true, 1e-12, true);
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &e) {
        std::printf("no usable device: %s\n", e.what());
        return 3;
    }
}
