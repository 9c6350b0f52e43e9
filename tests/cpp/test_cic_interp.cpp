// sdsp::cic_interpolator_bank (include/sdsp/cic_interp.h) against the serial Hogenauer form computed here -- N wrapping combs of
// delay M per input sample, then R output samples through N wrapping integrators, the comb value at the first and zeros at the
// others, registers of W bits zero at the start of the stream -- block by block on the host entry with blocks of irregular length
// (empty and shorter than the history included): int16 I/Q rows into 64-bit registers, int32 real rows into 64-bit registers, and
// int16 real rows into 32-bit registers, bit for bit; one float bank against (float)((double)y * scale).
// Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/cic_interp.h>

#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
constexpr std::uint64_t kChannels = 3;
constexpr std::uint64_t kBlocks[] = { 1, 0, 3, 100, 2, 700, 9, 1501, 64 };

// one row through the serial form in registers of type reg_t (unsigned: they wrap)
template <typename reg_t, typename in_t>
std::vector<reg_t> serial(const std::vector<in_t> &x, std::uint32_t order, std::uint32_t up, std::uint32_t delay)
{
    using sreg_t = typename std::make_signed<reg_t>::type;
    std::vector<reg_t> integ(order, 0), dly(static_cast<std::size_t>(order) * delay, 0), y;
    for (std::size_t i = 0; i < x.size(); i++) {
        reg_t v = static_cast<reg_t>(static_cast<sreg_t>(x[i]));
        for (std::uint32_t s = 0; s < order; s++) {
            reg_t *d = &dly[static_cast<std::size_t>(s) * delay];
            const reg_t in = v;
            v = static_cast<reg_t>(v - d[0]);
            for (std::uint32_t j = 0; j + 1 < delay; j++)
                d[j] = d[j + 1];
            d[delay - 1] = in;
        }
        for (std::uint32_t p = 0; p < up; p++) {
            reg_t u = p == 0 ? v : 0;
            for (std::uint32_t s = 0; s < order; s++) {
                integ[s] = static_cast<reg_t>(integ[s] + u);
                u = integ[s];
            }
            y.push_back(u);
        }
    }
    return y;
}

template <typename in_t, typename out_t, typename reg_t>
int run(std::uint32_t order, std::uint32_t up, std::uint32_t delay, bool cplx, std::uint32_t in_bits)
{
    using sreg_t = typename std::make_signed<reg_t>::type;
    const std::size_t width = cplx ? 2 : 1;
    std::mt19937 gen(11);
    const int amp = 1 << (in_bits - 2);
    std::uniform_int_distribution<int> dist(-amp, amp - 1);
    std::uint64_t total = 0;
    for (std::uint64_t b : kBlocks)
        total += b;
    std::vector<in_t> x(kChannels * total * width);
    for (in_t &v : x)
        v = static_cast<in_t>(dist(gen) + amp); // a large offset: the integrators wrap
    sdsp::cic_interpolator_bank<in_t, out_t> bank(order, up, delay, kChannels, cplx, in_bits);
    // the whole stream's outputs, per channel and plane
    std::vector<std::vector<reg_t>> want(kChannels * width);
    for (std::uint64_t c = 0; c < kChannels; c++)
        for (std::size_t w = 0; w < width; w++) {
            std::vector<in_t> row(total);
            for (std::uint64_t i = 0; i < total; i++)
                row[i] = x[(c * total + i) * width + w];
            want[c * width + w] = serial<reg_t, in_t>(row, order, up, delay);
        }
    std::uint64_t s0 = 0, outs = 0, bad = 0;
    for (std::uint64_t blk : kBlocks) {
        const std::uint64_t n = bank.out_samples(blk);
        std::vector<in_t> in(kChannels * blk * width);
        std::vector<out_t> out(kChannels * n * width);
        for (std::uint64_t c = 0; c < kChannels; c++)
            for (std::uint64_t i = 0; i < blk * width; i++)
                in[c * blk * width + i] = x[(c * total + s0) * width + i];
        if (bank.process_host(in.data(), out.data(), blk) != n)
            return 1;
        for (std::uint64_t c = 0; c < kChannels; c++)
            for (std::uint64_t m = 0; m < n; m++)
                for (std::size_t w = 0; w < width; w++) {
                    const sreg_t y = static_cast<sreg_t>(want[c * width + w][outs + m]);
                    const out_t got = out[(c * n + m) * width + w];
                    const out_t ref = std::is_same<out_t, float>::value
                                          ? static_cast<out_t>(static_cast<float>(static_cast<double>(y) * bank.scale()))
                                          : static_cast<out_t>(y);
                    if (!(got == ref))
                        bad++;
                }
        s0 += blk;
        outs += n;
    }
    const sdsp_hip_cic_interp_plan_info info = bank.info();
    std::printf("cic_interpolator_bank<int%u, %s> %s input: N %u, R %u, M %u, hist %u, in_bits %u + growth %u -> W %u, chunk %u, "
                "kernel %s, %llu outputs, %llu wrong\n",
                static_cast<unsigned>(8 * sizeof(in_t)), std::is_same<out_t, float>::value ? "float" : (sizeof(out_t) == 8 ? "int64" : "int32"),
                cplx ? "complex" : "real", info.order, info.up, info.delay, info.hist, info.in_bits, info.growth, info.reg_bits, info.chunk,
                info.kernel, static_cast<unsigned long long>(outs), static_cast<unsigned long long>(bad));
    return bad == 0 && outs == total * up && info.reg_bits == 8 * sizeof(reg_t) ? 0 : 1;
}
} // namespace

int main()
{
    try {
        const int rc = run<std::int16_t, std::int64_t, std::uint64_t>(6, 64, 1, true, 16) |
                       run<std::int32_t, std::int64_t, std::uint64_t>(5, 7, 2, false, 32) |
                       run<std::int16_t, std::int32_t, std::uint32_t>(4, 16, 2, false, 16) |
                       run<std::int16_t, float, std::uint64_t>(8, 3, 2, true, 16);
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &e) {
        std::printf("no usable device: %s\n", e.what());
        return 3;
    }
}
