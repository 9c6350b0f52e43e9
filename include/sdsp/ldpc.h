// sdsp/ldpc.h -- LDPC decoder banks for quasi-cyclic codes for the MI355X engine (sdsp_hip_ldpc_*).
//
// Codewords of n = nb z soft values of one code (a base matrix of shifts, -1 for the zero block, and the lifting size z) in: int8
// (ldpc_decoder<std::int8_t>) or float quantised with `scale` (ldpc_decoder<float>), positive favours bit 0, 0 is an erasure.  Hard
// bits (ldpc_output::bytes or ::packed), int16 posteriors and one status per codeword out (the iterations run, -1 where the
// syndrome test still fails), each optional.  The results are the contract's in front of sdsp_hip_ldpc_plan_create, in either
// kernel variant.  Mirrors sdsp::rs_decoder's plan handling (sdsp/rs.h): an RAII plan, process() on device pointers, process_host()
// for host buffers through detail::host_stage, info().  ldpc_parity_matrix and ldpc_encode run on the host; there is no CPU decoder.
#ifndef SDSP_MI355X_LDPC_H
#define SDSP_MI355X_LDPC_H

#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
enum class ldpc_output : int { bytes = SDSP_HIP_LDPC_BYTES, packed = SDSP_HIP_LDPC_PACKED };

// what names a code: mb x nb shifts, row-major, and the lifting size
struct ldpc_code {
    std::vector<std::int16_t> base;
    std::uint32_t mb, nb, z;
    std::uint32_t n() const noexcept { return nb * z; }
    std::uint32_t m() const noexcept { return mb * z; }
    std::uint32_t k() const noexcept { return (nb - mb) * z; }
};

// normalisation in sixteenths (12 is 0.75, 16 plain min-sum), offset, and whether a codeword stops at the first syndrome test it passes
struct ldpc_rule {
    std::uint32_t norm = 12, beta = 0;
    bool early_stop = true;
};

// the m x ceil(k / 32) words of P with parity = P data over GF(2), for codewords [data | parity]
inline std::vector<std::uint32_t> ldpc_parity_matrix(const ldpc_code &code)
{
    std::vector<std::uint32_t> P(static_cast<std::size_t>(code.m()) * ((code.k() + 31) / 32));
    detail::check(sdsp_hip_ldpc_parity_matrix(code.base.data(), code.mb, code.nb, code.z, P.data()));
    return P;
}

// rows of k data bits (0 / 1 bytes) -> rows of n bits: the data, then the parity
inline std::vector<std::uint8_t> ldpc_encode(const ldpc_code &code, const std::vector<std::uint8_t> &data)
{
    const std::size_t rows = code.k() ? data.size() / code.k() : 0;
    std::vector<std::uint8_t> out(rows * code.n());
    detail::check(sdsp_hip_ldpc_encode(code.base.data(), code.mb, code.nb, code.z, data.data(), rows, out.data()));
    return out;
}

template <typename in_t> class ldpc_decoder {
    static_assert(std::is_same<in_t, std::int8_t>::value || std::is_same<in_t, float>::value, "soft values are int8 or float");

public:
    // out_bits == 0: all n hard decisions; scale is read by ldpc_decoder<float> only
    ldpc_decoder(const ldpc_code &code, const ldpc_rule &rule = ldpc_rule(), ldpc_output output = ldpc_output::bytes,
                 std::uint32_t out_bits = 0, float scale = 1.0f, int device = 0)
        : m_n(code.n()), m_out_bits(out_bits ? out_bits : code.n()), m_output(output), m_device(device)
    {
        sdsp_hip_ldpc_plan *plan = nullptr;
        detail::check(sdsp_hip_ldpc_plan_create(&plan, code.base.data(), code.mb, code.nb, code.z, rule.norm, rule.beta, rule.early_stop ? 1 : 0,
                                                std::is_same<in_t, float>::value ? SDSP_HIP_LDPC_F32 : SDSP_HIP_LDPC_I8, scale,
                                                static_cast<int>(output), m_out_bits, device));
        m_plan.reset(plan);
    }
    ldpc_decoder(const ldpc_decoder &) = delete;
    ldpc_decoder &operator=(const ldpc_decoder &) = delete;

    // device pointers: `codewords` rows of n soft values in; rows of bits_bytes() hard bits, rows of n posteriors and one status per
    // codeword out, each of the three nullable but not all of them; asynchronous on `stream`
    void process(const in_t *device_llr, void *device_bits, std::int16_t *device_post, std::int32_t *device_status, std::uint64_t codewords,
                 std::uint32_t max_iter, void *stream = nullptr)
    {
        detail::check(sdsp_hip_ldpc_process(m_plan.get(), device_llr, device_bits, device_post, device_status, codewords, max_iter, stream));
    }
    // host pointers, the same shapes
    void process_host(const in_t *host_llr, void *host_bits, std::int16_t *host_post, std::int32_t *host_status, std::uint64_t codewords,
                      std::uint32_t max_iter)
    {
        if (codewords == 0)
            return;
        const std::size_t c = static_cast<std::size_t>(codewords);
        const detail::stage_item items[] = { { host_llr, nullptr, c * m_n * sizeof(in_t) },
                                             { nullptr, host_bits, c * bits_bytes() },
                                             { nullptr, host_post, c * m_n * sizeof(std::int16_t) },
                                             { nullptr, host_status, c * sizeof(std::int32_t) } };
        detail::host_stage(m_device, items, [&](void *const *dev) {
            return sdsp_hip_ldpc_process(m_plan.get(), dev[0], dev[1], static_cast<std::int16_t *>(dev[2]), static_cast<std::int32_t *>(dev[3]),
                                         codewords, max_iter, nullptr);
        });
    }
    // 0 = lanes are the checks of a layer, 1 = the plain kernel (allocates its workspace)
    void set_variant(int variant) { detail::check(sdsp_hip_ldpc_plan_set_variant(m_plan.get(), variant)); }
    std::uint32_t n() const noexcept { return m_n; }
    std::uint32_t out_bits() const noexcept { return m_out_bits; }
    // bytes of one codeword's hard bits
    std::size_t bits_bytes() const noexcept
    {
        return m_output == ldpc_output::packed ? static_cast<std::size_t>((m_out_bits + 31) / 32) * sizeof(std::uint32_t) : m_out_bits;
    }
    std::uint64_t launches(std::uint64_t codewords) const
    {
        std::uint64_t v = 0;
        detail::check(sdsp_hip_ldpc_plan_launches(m_plan.get(), codewords, &v));
        return v;
    }
    sdsp_hip_ldpc_plan_info info() const
    {
        sdsp_hip_ldpc_plan_info i{};
        detail::check(sdsp_hip_ldpc_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    std::uint32_t m_n, m_out_bits;
    ldpc_output m_output;
    int m_device;
    detail::plan_ptr<sdsp_hip_ldpc_plan, sdsp_hip_ldpc_plan_destroy> m_plan;
};
} // namespace sdsp

#endif // SDSP_MI355X_LDPC_H
