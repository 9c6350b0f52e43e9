// sdsp/cic.h -- CIC (Hogenauer) decimator bank for integer sample streams on the MI355X engine (sdsp_hip_cic_*, DESIGN.md
// section 5.22).
//
// Every channel, a stream of 16- or 32-bit integer samples (real, or interleaved I/Q), goes through `order` integrators, keeps every
// `down`-th sample, and through `order` combs of differential delay `delay`: no multiplies, exact in modular arithmetic, bit-exact
// for every input.  Mirrors sdsp::arb_resampler_bank (sdsp/arb_resample.h): RAII plan and device-resident per-channel history,
// process() on device pointers, process_host() for host buffers; the bank counts the stream position, so calls of any length chain
// into one stream.  in_t is std::int16_t or std::int32_t; out_t is std::int32_t (32-bit registers), std::int64_t (64-bit
// registers) or float, and the constructor checks that it matches the plan.  No reference counterpart: pinned to the serial
// Hogenauer form.  There is no CPU path.
#ifndef SDSP_MI355X_CIC_H
#define SDSP_MI355X_CIC_H

#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
// bit_length((down * delay)^order - 1): the bits the registers need above the input's
inline std::uint32_t cic_growth(std::uint32_t order, std::uint32_t down, std::uint32_t delay = 1)
{
    std::uint32_t b = 0;
    detail::check(sdsp_hip_cic_growth(order, down, delay, &b));
    return b;
}
// 1 / (double)(down * delay)^order: unity gain at DC
inline double cic_unity_scale(std::uint32_t order, std::uint32_t down, std::uint32_t delay = 1)
{
    double s = 0.0;
    detail::check(sdsp_hip_cic_unity_scale(order, down, delay, &s));
    return s;
}

template <typename in_t = std::int16_t, typename out_t = std::int64_t> class cic_decimator_bank {
    static_assert(std::is_same<in_t, std::int16_t>::value || std::is_same<in_t, std::int32_t>::value, "in_t: int16_t or int32_t");
    static_assert(std::is_same<out_t, std::int32_t>::value || std::is_same<out_t, std::int64_t>::value || std::is_same<out_t, float>::value,
                  "out_t: int32_t, int64_t or float");

public:
    // in_bits: significant bits of a sample (0: the width of in_t); complex_input: rows of interleaved I/Q pairs (one pair is one
    // sample); scale (float output only): 0 means unity gain at DC.  Throws when out_t is an integer of another width than the
    // registers in_bits + growth ask for.
    cic_decimator_bank(std::uint32_t order, std::uint32_t down, std::uint32_t delay, std::uint64_t channels, bool complex_input = false,
                       std::uint32_t in_bits = 0, double scale = 0.0, int device = 0)
        : m_order(order), m_down(down), m_delay(delay), m_in_bits(in_bits ? in_bits : static_cast<std::uint32_t>(8 * sizeof(in_t))),
          m_channels(channels), m_complex(complex_input), m_device(device)
    {
        const std::uint32_t bits = m_in_bits + cic_growth(order, down, delay);
        const bool is_float = std::is_same<out_t, float>::value;
        if (!is_float && bits <= 64 && (bits <= 32 ? 4u : 8u) != sizeof(out_t))
            throw hip_error(SDSP_HIP_ERR_INVALID_ARG, "sdsp_hip: out_t must be int32_t for 32-bit registers and int64_t for 64-bit ones");
        m_scale = is_float ? (scale != 0.0 ? scale : cic_unity_scale(order, down, delay)) : 1.0;
        m_hist = order * delay * down;
    }
    cic_decimator_bank(const cic_decimator_bank &) = delete;
    cic_decimator_bank &operator=(const cic_decimator_bank &) = delete;

    // forget the history and the stream position
    void reset()
    {
        if (m_state)
            zero_state();
        m_position = 0;
    }

    // outputs per channel of a call of `samples` at the bank's position
    std::uint64_t out_samples(std::uint64_t samples) const
    {
        std::uint64_t n = 0;
        detail::check(sdsp_hip_cic_out_samples(m_down, m_position, samples, &n));
        return n;
    }

    // device pointers (channel-major rows of samples or I/Q pairs), strides in elements, asynchronous on `stream`; continues every
    // channel's stream and returns the outputs written per channel
    std::uint64_t process(const in_t *device_in, std::uint64_t in_stride, out_t *device_out, std::uint64_t out_stride, std::uint64_t samples,
                          void *stream = nullptr)
    {
        ensure_plan();
        ensure_state();
        const std::uint64_t n = out_samples(samples);
        detail::check(sdsp_hip_cic_process(m_plan.get(), device_in, in_stride, device_out, out_stride, m_channels, samples, m_position,
                                           m_state.get(), stream));
        m_position += samples;
        return n;
    }
    // host pointers: in = channels x samples elements, out = channels x out_samples(samples) elements, both contiguous
    std::uint64_t process_host(const in_t *host_in, out_t *host_out, std::uint64_t samples)
    {
        ensure_plan();
        ensure_state();
        const std::uint64_t n = out_samples(samples);
        if (samples == 0)
            return 0;
        const std::size_t width = m_complex ? 2u : 1u;
        const std::size_t in_bytes = static_cast<std::size_t>(m_channels * samples) * width * sizeof(in_t);
        const std::size_t out_bytes = static_cast<std::size_t>(m_channels * n) * width * sizeof(out_t);
        // a call that yields no output has no output buffer and waits for the device instead of copying back
        const detail::stage_item items[] = { { host_in, nullptr, in_bytes }, { nullptr, out_bytes ? host_out : nullptr, out_bytes } };
        detail::host_stage(m_device, items, [&](void *const *dev) {
            const int rc = sdsp_hip_cic_process(m_plan.get(), dev[0], samples, dev[1], n, m_channels, samples, m_position, m_state.get(),
                                                nullptr);
            return rc || out_bytes ? rc : sdsp_hip_device_synchronize(m_device);
        });
        m_position += samples;
        return n;
    }
    std::uint64_t channels() const noexcept { return m_channels; }
    std::uint32_t history() const noexcept { return m_hist; }
    std::uint64_t position() const noexcept { return m_position; }
    void set_position(std::uint64_t position) noexcept { m_position = position; }
    double scale() const noexcept { return m_scale; }
    // 0 = the fused kernel, 1 = the plain cross-check kernel
    void set_variant(int variant)
    {
        ensure_plan();
        detail::check(sdsp_hip_cic_plan_set_variant(m_plan.get(), variant));
    }
    // chunks of input per workgroup of the fused kernel, 0 = automatic
    void set_segment(std::uint32_t chunks)
    {
        ensure_plan();
        detail::check(sdsp_hip_cic_plan_set_segment(m_plan.get(), chunks));
    }
    sdsp_hip_cic_plan_info info()
    {
        ensure_plan();
        sdsp_hip_cic_plan_info i{};
        detail::check(sdsp_hip_cic_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    void ensure_plan()
    {
        if (m_plan)
            return;
        sdsp_hip_cic_plan *plan = nullptr;
        detail::check(sdsp_hip_cic_plan_create(&plan, m_order, m_down, m_delay, sizeof(in_t) == 4 ? SDSP_HIP_CIC_I32 : SDSP_HIP_CIC_I16,
                                               m_in_bits, m_complex ? SDSP_HIP_CIC_COMPLEX : SDSP_HIP_CIC_REAL,
                                               std::is_same<out_t, float>::value ? SDSP_HIP_CIC_OUT_F32 : SDSP_HIP_CIC_OUT_INT, m_scale,
                                               m_device));
        m_plan.reset(plan);
    }
    void zero_state()
    {
        const std::size_t bytes = static_cast<std::size_t>(m_hist) * static_cast<std::size_t>(m_channels) * (m_complex ? 2u : 1u) * sizeof(in_t);
        if (!m_state)
            m_state.alloc(bytes, m_device);
        m_state.fill<unsigned char>(bytes, 0);
    }
    void ensure_state()
    {
        if (!m_state)
            zero_state();
    }

    std::uint32_t m_order, m_down, m_delay, m_in_bits;
    std::uint64_t m_channels;
    bool m_complex;
    int m_device;
    std::uint32_t m_hist{ 0 };
    double m_scale{ 1.0 };
    std::uint64_t m_position{ 0 };
    detail::plan_ptr<sdsp_hip_cic_plan, sdsp_hip_cic_plan_destroy> m_plan;
    detail::device_buffer m_state;
};
} // namespace sdsp

#endif // SDSP_MI355X_CIC_H
