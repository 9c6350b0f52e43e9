// sdsp/rs.h -- Reed-Solomon decoder banks over GF(256) for the MI355X engine (sdsp_hip_rs_*).
//
// Frames of `interleave` symbol-interleaved codewords of one code (field_poly, fcr, prim, nroots, n) in, optionally with erasure
// flags; the corrected frames (rs_output::full) or their data symbols (rs_output::data) and one count per codeword out, -1 where a
// codeword is beyond the code.  The bytes are the contract's in front of sdsp_hip_rs_plan_create, in either kernel variant.  Mirrors
// sdsp::viterbi_bank's plan handling (sdsp/viterbi.h): an RAII plan, process() on device pointers, process_host() for host buffers
// through detail::host_stage, info().  rs_generator and rs_encode run on the host; there is no CPU decoder.
#ifndef SDSP_MI355X_RS_H
#define SDSP_MI355X_RS_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
enum class rs_output : int { full = SDSP_HIP_RS_FULL, data = SDSP_HIP_RS_DATA };

// what names a code: GF(2^8) by field_poly with alpha = 2, and g(x) = prod_{j < nroots} (x - alpha^(prim (fcr + j))), shortened to n
struct rs_code {
    std::uint32_t field_poly, fcr, prim, nroots, n;
};

// the nroots + 1 coefficients of g, the highest first
inline std::vector<std::uint8_t> rs_generator(const rs_code &code)
{
    std::vector<std::uint8_t> g(static_cast<std::size_t>(code.nroots) + 1);
    detail::check(sdsp_hip_rs_generator(code.field_poly, code.fcr, code.prim, code.nroots, g.data()));
    return g;
}

// frames of interleave (n - nroots) data bytes -> frames of interleave n bytes: data symbols, then parity symbols
inline std::vector<std::uint8_t> rs_encode(const rs_code &code, std::uint32_t interleave, const std::vector<std::uint8_t> &data)
{
    const std::size_t row = static_cast<std::size_t>(interleave) * (code.n - code.nroots);
    const std::size_t frames = row ? data.size() / row : 0;
    std::vector<std::uint8_t> out(frames * interleave * code.n);
    detail::check(sdsp_hip_rs_encode(code.field_poly, code.fcr, code.prim, code.nroots, code.n, interleave, data.data(), frames, out.data()));
    return out;
}

class rs_decoder {
public:
    rs_decoder(const rs_code &code, std::uint32_t interleave = 1, rs_output output = rs_output::full, int device = 0)
        : m_code(code), m_interleave(interleave), m_output(output), m_device(device)
    {
        sdsp_hip_rs_plan *plan = nullptr;
        detail::check(sdsp_hip_rs_plan_create(&plan, code.field_poly, code.fcr, code.prim, code.nroots, code.n, interleave,
                                              static_cast<int>(output), device));
        m_plan.reset(plan);
    }
    rs_decoder(const rs_decoder &) = delete;
    rs_decoder &operator=(const rs_decoder &) = delete;

    // device pointers: `frames` frames of frame_bytes() in (and erasure flags, or null), frames of out_bytes() out (device_out ==
    // device_in: in place, rs_output::full only), frames interleave counts (or null); asynchronous on `stream`
    void process(const std::uint8_t *device_in, const std::uint8_t *device_erasures, std::uint8_t *device_out, std::int32_t *device_corrected,
                 std::uint64_t frames, void *stream = nullptr)
    {
        detail::check(sdsp_hip_rs_process(m_plan.get(), device_in, device_erasures, device_out, device_corrected, frames, stream));
    }
    // host pointers, the same shapes; host_out must not be host_in
    void process_host(const std::uint8_t *host_in, const std::uint8_t *host_erasures, std::uint8_t *host_out, std::int32_t *host_corrected,
                      std::uint64_t frames)
    {
        if (frames == 0)
            return;
        const std::size_t f = static_cast<std::size_t>(frames);
        const detail::stage_item items[] = { { host_in, nullptr, f * frame_bytes() },
                                             { host_erasures, nullptr, f * frame_bytes() },
                                             { nullptr, host_out, f * out_bytes() },
                                             { nullptr, host_corrected, f * m_interleave * sizeof(std::int32_t) } };
        detail::host_stage(m_device, items, [&](void *const *dev) {
            return sdsp_hip_rs_process(m_plan.get(), dev[0], dev[1], dev[2], static_cast<std::int32_t *>(dev[3]), frames, nullptr);
        });
    }
    // 0 = a wave per frame, 1 = the plain kernel
    void set_variant(int variant) { detail::check(sdsp_hip_rs_plan_set_variant(m_plan.get(), variant)); }
    std::uint32_t k() const noexcept { return m_code.n - m_code.nroots; }
    std::uint32_t t() const noexcept { return m_code.nroots / 2; }
    std::uint32_t interleave() const noexcept { return m_interleave; }
    std::size_t frame_bytes() const noexcept { return static_cast<std::size_t>(m_interleave) * m_code.n; }
    std::size_t out_bytes() const noexcept { return static_cast<std::size_t>(m_interleave) * (m_output == rs_output::data ? k() : m_code.n); }
    std::uint64_t launches(std::uint64_t frames) const
    {
        std::uint64_t v = 0;
        detail::check(sdsp_hip_rs_plan_launches(m_plan.get(), frames, &v));
        return v;
    }
    sdsp_hip_rs_plan_info info() const
    {
        sdsp_hip_rs_plan_info i{};
        detail::check(sdsp_hip_rs_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    rs_code m_code;
    std::uint32_t m_interleave;
    rs_output m_output;
    int m_device;
    detail::plan_ptr<sdsp_hip_rs_plan, sdsp_hip_rs_plan_destroy> m_plan;
};
} // namespace sdsp

#endif // SDSP_MI355X_RS_H
