// The four host-only helpers of the CIC bank (sdsp_hip_cic_growth, _out_samples, _unity_scale, _taps; csrc/host_math.cpp) called from
// a program of its own, so that tests/test_cic_host.py can build both with -fsanitize=address,undefined: the tap buffer has exactly
// N (R M - 1) + 1 entries, so a write past it is seen.  Each result is also checked against an independent evaluation in unsigned
// __int128.  Exit 0 = pass, 1 = mismatch.
#include <sdsp_hip.h>

#include <cstdint>
#include <cstdio>
#include <vector>

namespace
{
struct shape {
    std::uint32_t n, r, m;
};
const shape kShapes[] = { { 1, 2, 1 }, { 3, 5, 1 }, { 4, 16, 2 }, { 6, 64, 1 }, { 5, 7, 2 }, { 8, 3, 2 }, { 6, 1024, 1 }, { 8, 4096, 2 }, { 2, 16384, 2 } };

int check(const shape &s)
{
    unsigned __int128 gain = 1;
    for (std::uint32_t i = 0; i < s.n; i++)
        gain *= static_cast<std::uint64_t>(s.r) * s.m;
    std::uint32_t want_bits = 0;
    for (unsigned __int128 v = gain - 1; v; v >>= 1)
        want_bits++;
    std::uint32_t bits = 0;
    if (sdsp_hip_cic_growth(s.n, s.r, s.m, &bits) != SDSP_HIP_OK || bits != want_bits)
        return 1;
    double scale = 0.0;
    if (sdsp_hip_cic_unity_scale(s.n, s.r, s.m, &scale) != SDSP_HIP_OK || scale != 1.0 / static_cast<double>(gain))
        return 1;
    const std::size_t len = static_cast<std::size_t>(s.n) * (s.r * s.m - 1) + 1;
    std::vector<std::uint64_t> h(len);
    if (sdsp_hip_cic_taps(s.n, s.r, s.m, h.data()) != SDSP_HIP_OK)
        return 1;
    unsigned __int128 sum = 0; // the taps sum to the gain; symmetric; the first is 1
    for (std::size_t k = 0; k < len; k++) {
        sum += h[k];
        if (h[k] != h[len - 1 - k])
            return 1;
    }
    if (h[0] != 1 || (gain >> 64 == 0 && sum != gain))
        return 1;
    for (std::uint64_t position : { 0ull, 1ull, ~0ull, ~0ull - s.r, 1ull << 40 })
        for (std::uint64_t samples : { 0ull, 1ull, static_cast<unsigned long long>(s.r), (1ull << 31) - 1 }) {
            std::uint64_t n = 0;
            const unsigned __int128 end = static_cast<unsigned __int128>(position) + samples;
            if (sdsp_hip_cic_out_samples(s.r, position, samples, &n) != SDSP_HIP_OK ||
                n != static_cast<std::uint64_t>(end / s.r - position / s.r))
                return 1;
        }
    return 0;
}
} // namespace

int main()
{
    int rc = 0;
    for (const shape &s : kShapes)
        rc |= check(s);
    std::uint32_t bits = 0;
    std::uint64_t n = 0;
    rc |= sdsp_hip_cic_growth(9, 2, 1, &bits) != SDSP_HIP_ERR_INVALID_SIZE;
    rc |= sdsp_hip_cic_growth(8, 8192, 2, &bits) != SDSP_HIP_ERR_INVALID_SIZE;
    rc |= sdsp_hip_cic_taps(1, 2, 1, nullptr) != SDSP_HIP_ERR_INVALID_ARG;
    rc |= sdsp_hip_cic_out_samples(2, 0, 1ull << 31, &n) != SDSP_HIP_ERR_INVALID_SIZE;
    std::printf("%s\n", rc ? "FAILED" : "ok");
    return rc;
}
