// sdsp::stft_bank -> sdsp::istft_bank (include/sdsp/stft.h, include/sdsp/istft.h) round trip, block by block on the host entries
// (blocks whose F hop is shorter than the pending sums included): the output is the input delayed by hist = N - hop samples, within
// 1e-5 (f32) / 8 N eps (f64) of the signal's largest sample.  Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no
// CPU fallback).
#include <sdsp/istft.h>
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
constexpr std::uint64_t kBlocks[] = { 1, 2, 10, 1, 6 }; // frames per block; 1 and 2 frames are shorter than hist = 192

template <typename real_t> int run(double tol)
{
    using stft_t = sdsp::stft_bank<kN, kHop, real_t>;
    using istft_t = sdsp::istft_bank<kN, kHop, real_t>;
    std::mt19937 gen(13);
    std::normal_distribution<double> dist(0.0, 1.0);
    std::uint64_t frames = 0;
    for (std::uint64_t b : kBlocks)
        frames += b;
    const std::uint64_t total = frames * kHop;
    std::vector<real_t> x(kChannels * total);
    for (auto &v : x)
        v = static_cast<real_t>(dist(gen));
    stft_t fwd(kChannels, SDSP_HIP_STFT_COMPLEX);
    istft_t inv(kChannels);
    fwd.set_window(SDSP_HIP_WINDOW_HAMMING);
    inv.set_window(SDSP_HIP_WINDOW_HAMMING);
    std::vector<std::vector<double>> y(kChannels);
    std::uint64_t f0 = 0;
    for (std::uint64_t blk : kBlocks) {
        const std::uint64_t s = blk * kHop;
        std::vector<real_t> in(kChannels * s), spec(kChannels * blk * stft_t::bins * 2), out(kChannels * s);
        for (std::uint64_t c = 0; c < kChannels; c++)
            std::copy_n(&x[c * total + f0 * kHop], s, &in[c * s]);
        fwd.process_host(in.data(), spec.data(), s);
        inv.process_host(spec.data(), out.data(), blk);
        for (std::uint64_t c = 0; c < kChannels; c++)
            for (std::uint64_t i = 0; i < s; i++)
                y[c].push_back(static_cast<double>(out[c * s + i]));
        f0 += blk;
    }
    double worst = 0.0, peak = 0.0;
    for (std::uint64_t c = 0; c < kChannels; c++)
        for (std::uint64_t t = 0; t < total; t++) {
            const double want = t < istft_t::hist ? 0.0 : static_cast<double>(x[c * total + t - istft_t::hist]);
            worst = std::max(worst, std::fabs(y[c][t] - want));
            peak = std::max(peak, std::fabs(want));
        }
    const sdsp_hip_istft_plan_info info = inv.info();
    std::printf("istft_bank<%u, %u, %s>: hist %u, bins %u, kernel %s, env %.4f .. %.4f, round-trip rel err %.3e\n", kN, kHop,
                sizeof(real_t) == 8 ? "double" : "float", info.hist, info.bins, info.kernel, info.env_min, info.env_max, worst / peak);
    return worst <= tol * peak ? 0 : 1;
}
} // namespace

int main()
{
    try {
        const int rc = run<float>(1e-5) | run<double>(8.0 * kN * 2.220446049250313e-16);
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &e) {
        std::printf("no usable device: %s\n", e.what());
        return 3;
    }
}
