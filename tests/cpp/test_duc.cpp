// sdsp::duc_bank (include/sdsp/duc.h) against a double interpolate -> mix -> sum computed here, block by block on the host entry with
// blocks of any length (empty and shorter than the history included): I/Q and real output, one channel with one band, one with
// six and one without.  f64 is held within 1e-12 B max_p sum_q |h[q U + p]| max|x| of the double result on every channel (B = its
// band count), f32 within 1e-6 of the largest output on the six-band channel; the channel without bands must be zero.
// Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/duc.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
constexpr std::uint32_t kTaps = 65, kUp = 4, kChannels = 3;
constexpr std::uint64_t kBlocks[] = { 1, 0, 3, 100, 2, 300, 9 };

template <typename real_t> int run(bool real_out, double tol, bool absolute)
{
    const std::vector<sdsp_hip_duc_band> bands = { { 1, sdsp::ddc_phase_word(0.123), 0 },
                                                   { 0, sdsp::ddc_phase_word(-0.31), sdsp::ddc_phase_word(0.25) },
                                                   { 1, 0x80000000u, 17 },
                                                   { 1, 0, 0 },
                                                   { 1, 0x12345678u, 0xfedcba98u },
                                                   { 1, sdsp::ddc_phase_word(0.4), 5 },
                                                   { 1, sdsp::ddc_phase_word(-0.05), 0 } };
    const std::uint32_t per_channel[kChannels] = { 1, 6, 0 };
    std::mt19937 gen(11);
    std::normal_distribution<double> dist(0.0, 1.0);
    std::uint64_t total = 0;
    for (std::uint64_t b : kBlocks)
        total += b;
    const std::size_t nb = bands.size(), width = real_out ? 1 : 2;
    std::vector<real_t> x(nb * total * 2);
    for (real_t &v : x)
        v = static_cast<real_t>(dist(gen));
    sdsp::duc_bank<real_t> bank(kTaps, kUp, bands, kChannels, real_out);
    bank.set_antiimage_coeff();
    const std::uint64_t pos0 = (1ull << 30) - 100; // position * up wraps 2^32 inside the stream
    bank.set_position(pos0);
    const std::uint64_t outs = total * kUp;
    std::vector<real_t> y(kChannels * outs * width);
    std::uint64_t s0 = 0;
    for (std::uint64_t blk : kBlocks) {
        std::vector<real_t> in(nb * blk * 2), out(kChannels * blk * kUp * width);
        for (std::size_t i = 0; i < nb; i++)
            std::copy_n(&x[(i * total + s0) * 2], blk * 2, &in[i * blk * 2]);
        bank.process_host(in.data(), out.data(), blk);
        for (std::uint64_t c = 0; c < kChannels; c++)
            std::copy_n(&out[c * blk * kUp * width], blk * kUp * width, &y[(c * outs + s0 * kUp) * width]);
        s0 += blk;
    }
    if (bank.position() != pos0 + total)
        return 1;
    const double two_pi = 6.283185307179586476925286766559;
    double xmax = 0.0, phase_sum = 0.0;
    std::vector<double> h(kTaps);
    for (std::uint32_t k = 0; k < kTaps; k++)
        h[k] = static_cast<double>(static_cast<real_t>(bank.coeff()[k]));
    for (std::uint32_t p = 0; p < kUp; p++) {
        double s = 0.0;
        for (std::uint32_t k = p; k < kTaps; k += kUp)
            s += std::fabs(h[k]);
        phase_sum = std::max(phase_sum, s);
    }
    for (real_t v : x)
        xmax = std::max(xmax, std::fabs(static_cast<double>(v)));
    double worst = 0.0;
    bool zero_ok = true;
    for (std::uint32_t c = 0; c < kChannels; c++) {
        double err = 0.0, ymax = 0.0;
        for (std::uint64_t r = 0; r < outs; r++) {
            const std::uint64_t m = r / kUp;
            const std::uint32_t p = static_cast<std::uint32_t>(r % kUp);
            const std::uint32_t n = static_cast<std::uint32_t>(pos0 * kUp + r);
            std::complex<double> acc = 0.0;
            for (std::size_t i = 0; i < nb; i++) {
                if (bands[i].dst != c)
                    continue;
                std::complex<double> z = 0.0;
                for (std::uint32_t q = 0; q * kUp + p < kTaps && q <= m; q++) {
                    const real_t *s = &x[(i * total + (m - q)) * 2];
                    z += h[q * kUp + p] * std::complex<double>(static_cast<double>(s[0]), static_cast<double>(s[1]));
                }
                const std::uint32_t j = bands[i].phase0 + bands[i].fcw * n;
                acc += z * std::polar(1.0, two_pi * static_cast<double>(j) / 4294967296.0);
            }
            const real_t *g = &y[(c * outs + r) * width];
            const std::complex<double> got(static_cast<double>(g[0]), real_out ? 0.0 : static_cast<double>(g[1]));
            const std::complex<double> want = real_out ? std::complex<double>(acc.real(), 0.0) : acc;
            err = std::max(err, std::abs(got - want));
            ymax = std::max(ymax, std::abs(want));
        }
        if (per_channel[c] == 0)
            zero_ok = zero_ok && err == 0.0;
        else if (absolute)
            worst = std::max(worst, err / (per_channel[c] * phase_sum * xmax));
        else if (per_channel[c] == 6)
            worst = std::max(worst, err / ymax);
    }
    const sdsp_hip_duc_plan_info info = bank.info();
    std::printf("duc_bank<%s> %s output: %u taps, up %u, %u bands, hist %u, block %u, kernel %s, err %.3e (bound %.0e)%s\n",
                sizeof(real_t) == 8 ? "double" : "float", real_out ? "real" : "complex", info.taps, info.up, info.bands, info.hist,
                info.block_in, info.kernel, worst, tol, zero_ok ? "" : ", the channel without bands is not zero");
    return worst <= tol && zero_ok ? 0 : 1;
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
