// sdsp/arb_resample.h -- arbitrary-ratio polyphase resampler bank for the MI355X engine (sdsp_hip_arb_*).
//
// Every channel is resampled by any ratio in [1 / 1024, 1024] (input samples per output sample, Q32.32) through a prototype low-pass
// of phases * taps_per_phase taps, nearest phase or linear interpolation between two, out of place.  Mirrors
// sdsp::fir_resampler_bank (sdsp/resample.h) and sdsp::ddc_bank (sdsp/ddc.h): RAII plan and device-resident per-channel history,
// process() on device pointers, process_host() for host buffers; the bank keeps the step and counts the stream time, so calls of any
// length chain into one stream and the step may change between calls.  No reference counterpart: pinned to the piecewise-linear
// prototype evaluated in double.  There is no CPU path.
#ifndef SDSP_MI355X_ARB_RESAMPLE_H
#define SDSP_MI355X_ARB_RESAMPLE_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
// round(in_per_out 2^32), ties to even, for in_per_out in [1 / 1024, 1024] input samples per output sample; throws outside
inline std::uint64_t arb_step(double in_per_out)
{
    std::uint64_t s = 0;
    detail::check(sdsp_hip_arb_step(in_per_out, &s));
    return s;
}

template <typename real_t = float> class arb_resampler_bank {
public:
    // max_step: the largest Q32.32 step a call may use (arb_step(max ratio)); complex_input: rows of interleaved I/Q pairs (one pair
    // is one sample) instead of real samples; linear: interpolate between neighbouring phases instead of taking the nearest below
    arb_resampler_bank(std::uint32_t phases, std::uint32_t taps_per_phase, std::uint64_t max_step, std::uint64_t channels,
                       bool complex_input = false, bool linear = true, int device = 0)
        : m_phases(phases), m_taps(taps_per_phase), m_max_step(max_step), m_channels(channels), m_complex(complex_input), m_linear(linear),
          m_device(device), m_coeff(static_cast<std::size_t>(phases) * taps_per_phase, 0.0),
          m_step(max_step < (1ull << 32) ? max_step : (1ull << 32))
    {
    }
    arb_resampler_bank(const arb_resampler_bank &) = delete;
    arb_resampler_bank &operator=(const arb_resampler_bank &) = delete;

    // the prototype: phases * taps_per_phase values, phase p, tap k = h[k * phases + p]
    void set_coeff(const std::vector<double> &h)
    {
        if (h.size() != m_coeff.size())
            throw hip_error(SDSP_HIP_ERR_INVALID_SIZE, "sdsp_hip: coefficient count differs from phases * taps_per_phase");
        m_coeff = h;
        m_plan.reset();
    }
    // Hamming low-pass for ratios up to max_in_per_out, gain phases (sdsp_hip_arb_design)
    void set_default_coeff(double max_in_per_out)
    {
        detail::check(sdsp_hip_arb_design(m_phases, m_taps, max_in_per_out, m_coeff.data()));
        m_plan.reset();
    }
    // forget the history and the stream time
    void reset()
    {
        if (m_state)
            zero_state();
        m_time = 0;
    }

    // outputs per channel of a call of `samples` at the bank's step and time
    std::uint64_t out_samples(std::uint64_t samples) const
    {
        std::uint64_t n = 0;
        detail::check(sdsp_hip_arb_out_samples(m_step, m_time, samples, &n, nullptr));
        return n;
    }

    // device pointers (channel-major rows of reals or I/Q pairs), strides in elements, asynchronous on `stream`; continues every
    // channel's stream and returns the outputs written per channel
    std::uint64_t process(const real_t *device_in, std::uint64_t in_stride, real_t *device_out, std::uint64_t out_stride,
                          std::uint64_t samples, void *stream = nullptr)
    {
        ensure_plan();
        ensure_state();
        std::uint64_t n = 0, next = 0;
        detail::check(sdsp_hip_arb_out_samples(m_step, m_time, samples, &n, &next));
        detail::check(sdsp_hip_arb_process(m_plan.get(), device_in, in_stride, device_out, out_stride, m_channels, samples, m_step, m_time,
                                           m_state.get(), stream));
        m_time = next;
        return n;
    }
    // host pointers: in = channels x samples elements, out = channels x out_samples(samples) elements, both contiguous
    std::uint64_t process_host(const real_t *host_in, real_t *host_out, std::uint64_t samples)
    {
        ensure_plan();
        ensure_state();
        std::uint64_t n = 0, next = 0;
        detail::check(sdsp_hip_arb_out_samples(m_step, m_time, samples, &n, &next));
        if (samples == 0)
            return 0;
        const std::size_t in_bytes = static_cast<std::size_t>(m_channels * samples) * elem_bytes();
        const std::size_t out_bytes = static_cast<std::size_t>(m_channels * n) * elem_bytes();
        // a call that yields no output has no output buffer and waits for the device instead of copying back
        const detail::stage_item items[] = { { host_in, nullptr, in_bytes }, { nullptr, out_bytes ? host_out : nullptr, out_bytes } };
        detail::host_stage(m_device, items, [&](void *const *dev) {
            const int rc = sdsp_hip_arb_process(m_plan.get(), dev[0], samples, dev[1], n, m_channels, samples, m_step, m_time,
                                                m_state.get(), nullptr);
            return rc || out_bytes ? rc : sdsp_hip_device_synchronize(m_device);
        });
        m_time = next;
        return n;
    }
    std::uint64_t channels() const noexcept { return m_channels; }
    std::uint64_t step() const noexcept { return m_step; }
    // the step of the calls from here on: Q32.32 in [2^22, max_step]
    void set_step(std::uint64_t step)
    {
        if (step < SDSP_HIP_ARB_MIN_STEP || step > m_max_step)
            throw hip_error(SDSP_HIP_ERR_INVALID_SIZE, "sdsp_hip: step must be in [2^22, max_step]");
        m_step = step;
    }
    std::uint64_t time() const noexcept { return m_time; }
    void set_time(std::uint64_t time) noexcept { m_time = time; }
    const std::vector<double> &coeff() const { return m_coeff; }
    sdsp_hip_arb_plan_info info()
    {
        ensure_plan();
        sdsp_hip_arb_plan_info i{};
        detail::check(sdsp_hip_arb_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    std::size_t elem_bytes() const noexcept { return (m_complex ? 2u : 1u) * sizeof(real_t); }
    void ensure_plan()
    {
        if (m_plan)
            return;
        sdsp_hip_arb_plan *plan = nullptr;
        detail::check(sdsp_hip_arb_plan_create(&plan, m_phases, m_taps, m_coeff.data(), m_max_step,
                                               m_complex ? SDSP_HIP_ARB_COMPLEX : SDSP_HIP_ARB_REAL,
                                               m_linear ? SDSP_HIP_ARB_LINEAR : SDSP_HIP_ARB_NEAREST, detail::precision_of<real_t>::value,
                                               m_device));
        m_plan.reset(plan);
    }
    void zero_state()
    {
        const std::size_t len = m_taps > 1 ? m_taps - 1 : 1;
        const std::size_t bytes = len * static_cast<std::size_t>(m_channels) * elem_bytes();
        if (!m_state)
            m_state.alloc(bytes, m_device);
        m_state.fill<unsigned char>(bytes, 0);
    }
    void ensure_state()
    {
        if (!m_state)
            zero_state();
    }

    std::uint32_t m_phases, m_taps;
    std::uint64_t m_max_step, m_channels;
    bool m_complex, m_linear;
    int m_device;
    std::vector<double> m_coeff;
    std::uint64_t m_step;
    std::uint64_t m_time{ 0 };
    detail::plan_ptr<sdsp_hip_arb_plan, sdsp_hip_arb_plan_destroy> m_plan;
    detail::device_buffer m_state;
};
} // namespace sdsp

#endif // SDSP_MI355X_ARB_RESAMPLE_H
