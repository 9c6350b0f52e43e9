// sdsp/viterbi.h -- streaming soft-decision Viterbi decoder banks for the MI355X engine (sdsp_hip_viterbi_*).
//
// One rate-1/n convolutional code (K = 3 .. 9, n = 2 or 3) decoded in many channels at once: compact rows of steps n soft values in
// (in_t = std::int8_t, or float quantised by the plan's scale), `steps` decoded bits per row out, Dr = block ceil(depth / block) steps
// behind the input.  The bits are the contract's in front of sdsp_hip_viterbi_plan_create, in either kernel variant.  Mirrors
// sdsp::cfar2d_plan's plan handling (sdsp/cfar2d.h): an RAII plan that owns its device state, process() on device pointers,
// process_host() for host buffers through detail::host_stage, info().  There is no CPU path.
#ifndef SDSP_MI355X_VITERBI_H
#define SDSP_MI355X_VITERBI_H

#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
enum class viterbi_output : int { bytes = SDSP_HIP_VITERBI_BYTES, packed = SDSP_HIP_VITERBI_PACKED };

// Dr = block ceil(depth / block)
inline std::uint32_t viterbi_delay(std::uint32_t block, std::uint32_t depth)
{
    std::uint32_t d = 0;
    detail::check(sdsp_hip_viterbi_delay(block, depth, &d));
    return d;
}

// the coded bits (0 / 1) of `bits` from state 0, n per input bit; with `terminate`, k - 1 zero bits follow the input
inline std::vector<std::uint8_t> conv_encode(std::uint32_t k, const std::vector<std::uint32_t> &generators, const std::vector<std::uint8_t> &bits,
                                             bool terminate = false)
{
    const std::uint32_t n = static_cast<std::uint32_t>(generators.size());
    std::vector<std::uint8_t> out((bits.size() + (terminate && k ? k - 1 : 0)) * n);
    detail::check(sdsp_hip_conv_encode(k, n, generators.data(), bits.data(), bits.size(), terminate ? 1 : 0, out.data()));
    return out;
}

template <typename in_t = std::int8_t> class viterbi_bank {
    static_assert(std::is_same<in_t, std::int8_t>::value || std::is_same<in_t, float>::value, "soft values are std::int8_t or float");

public:
    static constexpr int in_kind = std::is_same<in_t, float>::value ? SDSP_HIP_VITERBI_F32 : SDSP_HIP_VITERBI_I8;

    viterbi_bank(std::uint32_t k, const std::vector<std::uint32_t> &generators, std::uint32_t block, std::uint32_t depth,
                 std::uint64_t max_channels, viterbi_output output = viterbi_output::bytes, float scale = 1.0f, int device = 0)
        : m_n(static_cast<std::uint32_t>(generators.size())), m_block(block), m_output(output), m_device(device)
    {
        sdsp_hip_viterbi_plan *plan = nullptr;
        detail::check(sdsp_hip_viterbi_plan_create(&plan, k, m_n, generators.data(), block, depth, in_kind, static_cast<int>(output), scale,
                                                   max_channels, device));
        m_plan.reset(plan);
    }
    viterbi_bank(const viterbi_bank &) = delete;
    viterbi_bank &operator=(const viterbi_bank &) = delete;

    // device pointers: channels rows of steps n soft values in, channels rows of steps bytes (or steps / 32 words) out; steps is a
    // multiple of the block; asynchronous on `stream`
    void process(const in_t *device_in, void *device_out, std::uint64_t channels, std::uint64_t steps, void *stream = nullptr)
    {
        detail::check(sdsp_hip_viterbi_process(m_plan.get(), device_in, device_out, channels, steps, stream));
    }
    // host pointers, the same shapes
    void process_host(const in_t *host_in, void *host_out, std::uint64_t channels, std::uint64_t steps)
    {
        if (channels == 0 || steps == 0)
            return;
        const std::size_t in_bytes = static_cast<std::size_t>(channels * steps * m_n) * sizeof(in_t);
        const std::size_t out_bytes = static_cast<std::size_t>(channels * (m_output == viterbi_output::packed ? steps / 8 : steps));
        const detail::stage_item items[] = { { host_in, nullptr, in_bytes }, { nullptr, host_out, out_bytes } };
        detail::host_stage(m_device, items, [&](void *const *dev) { return sdsp_hip_viterbi_process(m_plan.get(), dev[0], dev[1], channels, steps, nullptr); });
    }
    // a fresh stream in every channel; start_state >= 0 is the encoder's known start state
    void reset(int start_state = -1) { detail::check(sdsp_hip_viterbi_plan_reset(m_plan.get(), start_state)); }
    // the path metrics of the first `channels` channels, channels x states
    std::vector<std::int32_t> metrics(std::uint64_t channels) const
    {
        std::vector<std::int32_t> m(static_cast<std::size_t>(channels) * info().states);
        if (!m.empty())
            detail::check(sdsp_hip_viterbi_plan_get_metrics(m_plan.get(), m.data(), channels));
        return m;
    }
    void set_metrics(const std::vector<std::int32_t> &m)
    {
        detail::check(sdsp_hip_viterbi_plan_set_metrics(m_plan.get(), m.data(), m.size() / info().states));
    }
    // 0 = a wave per channel (K = 7 only), 1 = the plain kernel
    void set_variant(int variant) { detail::check(sdsp_hip_viterbi_plan_set_variant(m_plan.get(), variant)); }
    std::uint32_t delay() const { return info().delay; }
    std::uint32_t block() const noexcept { return m_block; }
    std::uint64_t state_bytes() const
    {
        std::uint64_t v = 0;
        detail::check(sdsp_hip_viterbi_plan_state_bytes(m_plan.get(), &v));
        return v;
    }
    std::uint64_t launches(std::uint64_t channels, std::uint64_t steps) const
    {
        std::uint64_t v = 0;
        detail::check(sdsp_hip_viterbi_plan_launches(m_plan.get(), channels, steps, &v));
        return v;
    }
    sdsp_hip_viterbi_plan_info info() const
    {
        sdsp_hip_viterbi_plan_info i{};
        detail::check(sdsp_hip_viterbi_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    std::uint32_t m_n, m_block;
    viterbi_output m_output;
    int m_device;
    detail::plan_ptr<sdsp_hip_viterbi_plan, sdsp_hip_viterbi_plan_destroy> m_plan;
};
} // namespace sdsp

#endif // SDSP_MI355X_VITERBI_H
