// sdsp::pfb_bank -> sdsp::pfb_synthesis_bank (include/sdsp/pfb.h, include/sdsp/pfb_synth.h): blocks streamed through the analysis bank
// and, with the dual prototype, back through the synthesis bank on the host entries (blocks shorter than the history included) return
// the input delayed by hist samples, real and complex streams, both phase references: within 1e-10 (f64) / 1e-4 (f32) of
// max|x| max|g|.  Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/pfb.h>
#include <sdsp/pfb_synth.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
constexpr std::uint32_t kM = 64, kP = 4, kHop = 32;
constexpr std::uint64_t kStreams = 3;
constexpr std::uint64_t kBlocks[] = { 32, 96, 640, 32, 320 }; // multiples of hop; 32 and 96 are shorter than hist = 224

template <typename real_t> int run(int kind, int phase, double tol)
{
    const std::uint32_t cv = kind == SDSP_HIP_PFB_COMPLEX ? 2u : 1u;
    std::mt19937 gen(7);
    std::normal_distribution<double> dist(0.0, 1.0);
    std::uint64_t total = 0;
    for (std::uint64_t b : kBlocks)
        total += b;
    std::vector<real_t> x(kStreams * total * cv);
    for (auto &v : x)
        v = static_cast<real_t>(dist(gen));
    sdsp::pfb_bank<real_t> analysis(kM, kP, kHop, kStreams, kind, phase);
    analysis.set_prototype(SDSP_HIP_WINDOW_BLACKMAN);
    sdsp::pfb_synthesis_bank<real_t> synthesis(kM, kP, kHop, kStreams, kind, phase);
    synthesis.set_dual_of(analysis.taps());
    const std::vector<double> g = sdsp::pfb_dual_prototype(analysis.taps(), kM, kP, kHop);
    if (g != synthesis.taps() || synthesis.hist() != analysis.hist() || synthesis.bins() != analysis.bins())
        return 1;
    const std::uint32_t bins = analysis.bins(), hist = synthesis.hist();
    std::vector<std::vector<double>> y(kStreams);
    std::uint64_t s0 = 0;
    for (std::uint64_t blk : kBlocks) {
        const std::uint64_t frames = analysis.frames(blk);
        std::vector<real_t> in(kStreams * blk * cv), spec(kStreams * frames * bins * 2), out(kStreams * blk * cv);
        for (std::uint64_t c = 0; c < kStreams; c++)
            std::copy_n(&x[(c * total + s0) * cv], blk * cv, &in[c * blk * cv]);
        analysis.process_host(in.data(), spec.data(), blk);
        synthesis.process_host(spec.data(), out.data(), frames);
        for (std::uint64_t c = 0; c < kStreams; c++)
            for (std::uint64_t i = 0; i < blk * cv; i++)
                y[c].push_back(static_cast<double>(out[c * blk * cv + i]));
        s0 += blk;
    }
    if (synthesis.position() != total || analysis.position() != total)
        return 1;
    double num = 0.0, xmax = 0.0, gmax = 0.0;
    for (double t : g)
        gmax = std::max(gmax, std::fabs(t));
    for (std::uint64_t c = 0; c < kStreams; c++)
        for (std::uint64_t i = 0; i < total * cv; i++) {
            const std::uint64_t t = i / cv; // the sample; its delayed source is sample t - hist (zero before the stream)
            const double want = t < hist ? 0.0 : static_cast<double>(x[(c * total + (t - hist)) * cv + i % cv]);
            num = std::max(num, std::fabs(y[c][i] - want));
            xmax = std::max(xmax, std::fabs(static_cast<double>(x[c * total * cv + i])));
        }
    const double err = num / (xmax * gmax);
    const sdsp_hip_pfb_synth_plan_info info = synthesis.info();
    std::printf("pfb_synthesis_bank<%s> %s %s: hist %u, bins %u, unfold %s, kernel %s, round-trip err %.3e\n",
                sizeof(real_t) == 8 ? "double" : "float", kind == SDSP_HIP_PFB_COMPLEX ? "complex" : "real",
                phase == SDSP_HIP_PFB_PHASE_TIME ? "time" : "frame", info.hist, info.bins, info.unfold, info.kernel, err);
    return err <= tol ? 0 : 1;
}
} // namespace

int main()
{
    try {
        int rc = 0;
        for (int kind : { SDSP_HIP_PFB_REAL, SDSP_HIP_PFB_COMPLEX })
            for (int phase : { SDSP_HIP_PFB_PHASE_FRAME, SDSP_HIP_PFB_PHASE_TIME })
                rc |= run<float>(kind, phase, 1e-4) | run<double>(kind, phase, 1e-10);
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &e) {
        std::printf("no usable device: %s\n", e.what());
        return 3;
    }
}
