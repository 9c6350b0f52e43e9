// sdsp/duc.h -- digital up-converter bank for the MI355X engine (sdsp_hip_duc_*).
//
// A list of bands (output channel, frequency word, phase word), one baseband I/Q stream per band at the same low rate, is
// interpolated by `up` through one real low-pass, shifted up to the bands' centre frequencies and summed into `channels` output
// streams, out of place, with the oscillator phase continuous across calls.  The mirror of sdsp::ddc_bank (sdsp/ddc.h): RAII plan
// and device-resident per-band history, process() on device pointers, process_host() for host buffers; the bank counts the stream
// position.  A call of S samples per band (any S) writes S * up outputs per channel: I/Q pairs, or the real part only.  Phase words
// come from sdsp::ddc_phase_word.  No reference counterpart: pinned to scipy.signal.upfirdn -> mix -> sum.  There is no CPU path.
#ifndef SDSP_MI355X_DUC_H
#define SDSP_MI355X_DUC_H

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "ddc.h"

namespace sdsp
{
template <typename real_t = float> class duc_bank {
public:
    // real_output: rows of real samples (the real part of the sum) instead of interleaved I/Q pairs
    duc_bank(std::uint32_t n_taps, std::uint32_t up, std::vector<sdsp_hip_duc_band> bands, std::uint32_t channels = 1,
             bool real_output = false, int device = 0)
        : m_taps(n_taps), m_up(up), m_channels(channels), m_real(real_output), m_device(device), m_bands(std::move(bands)),
          m_coeff(n_taps, 0.0)
    {
    }
    duc_bank(const duc_bank &) = delete;
    duc_bank &operator=(const duc_bank &) = delete;

    void set_coeff(const std::vector<double> &h)
    {
        if (h.size() != m_taps)
            throw hip_error(SDSP_HIP_ERR_INVALID_SIZE, "sdsp_hip: coefficient count differs from n_taps");
        m_coeff = h;
        m_plan.reset();
    }
    // Hamming low-pass at 1 / (2 up) of the output rate with gain up (sdsp_hip_resample_design(n_taps, up, 1)); needs up >= 2
    void set_antiimage_coeff()
    {
        detail::check(sdsp_hip_resample_design(m_taps, m_up, 1, m_coeff.data()));
        m_plan.reset();
    }
    // forget the history and the stream position
    void reset()
    {
        if (m_state)
            zero_state();
        m_position = 0;
    }

    std::uint64_t out_samples(std::uint64_t samples) const
    {
        std::uint64_t n = 0;
        detail::check(sdsp_hip_duc_out_samples(m_up, samples, &n));
        return n;
    }

    // device pointers (in: one row of I/Q pairs per band; out: channel-major rows of I/Q pairs or reals), strides in elements,
    // asynchronous on `stream`; continues every band's stream
    void process(const real_t *device_in, std::uint64_t in_stride, real_t *device_out, std::uint64_t out_stride, std::uint64_t samples,
                 void *stream = nullptr)
    {
        ensure_plan();
        ensure_state();
        detail::check(sdsp_hip_duc_process(m_plan.get(), device_in, in_stride, device_out, out_stride, samples, m_position, m_state.get(),
                                           stream));
        m_position += samples;
    }
    // host pointers: in = bands x samples I/Q pairs, out = channels x out_samples(samples) elements, both contiguous
    void process_host(const real_t *host_in, real_t *host_out, std::uint64_t samples)
    {
        ensure_plan();
        ensure_state();
        const std::uint64_t outs = out_samples(samples);
        const std::size_t in_bytes = static_cast<std::size_t>(m_bands.size() * samples) * 2 * sizeof(real_t);
        const std::size_t out_bytes = static_cast<std::size_t>(m_channels * outs) * out_elem_bytes();
        if (samples == 0)
            return;
        detail::host_stage(m_device, { { host_in, nullptr, in_bytes }, { nullptr, host_out, out_bytes } }, [&](void *const *dev) {
            return sdsp_hip_duc_process(m_plan.get(), dev[0], samples, dev[1], outs, samples, m_position, m_state.get(), nullptr);
        });
        m_position += samples;
    }
    std::uint32_t channels() const noexcept { return m_channels; }
    std::size_t bands() const noexcept { return m_bands.size(); }
    std::uint64_t position() const noexcept { return m_position; }
    void set_position(std::uint64_t position) noexcept { m_position = position; }
    void set_variant(int variant)
    {
        ensure_plan();
        detail::check(sdsp_hip_duc_plan_set_variant(m_plan.get(), variant));
    }
    const std::vector<double> &coeff() const { return m_coeff; }
    sdsp_hip_duc_plan_info info()
    {
        ensure_plan();
        sdsp_hip_duc_plan_info i{};
        detail::check(sdsp_hip_duc_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    std::size_t out_elem_bytes() const noexcept { return (m_real ? 1u : 2u) * sizeof(real_t); }
    void ensure_plan()
    {
        if (m_plan)
            return;
        sdsp_hip_duc_plan *plan = nullptr;
        detail::check(sdsp_hip_duc_plan_create(&plan, m_taps, m_coeff.data(), m_up, m_channels, static_cast<std::uint32_t>(m_bands.size()),
                                               m_bands.data(), m_real ? SDSP_HIP_DUC_REAL : SDSP_HIP_DUC_COMPLEX,
                                               detail::precision_of<real_t>::value, m_device));
        m_plan.reset(plan);
    }
    void zero_state()
    {
        const std::size_t hist = m_taps && m_up ? (m_taps - 1) / m_up : 0;
        const std::size_t bytes = (hist ? hist : 1) * m_bands.size() * 2 * sizeof(real_t);
        if (!m_state)
            m_state.alloc(bytes, m_device);
        m_state.fill<unsigned char>(bytes, 0);
    }
    void ensure_state()
    {
        if (!m_state)
            zero_state();
    }

    std::uint32_t m_taps, m_up, m_channels;
    bool m_real;
    int m_device;
    std::vector<sdsp_hip_duc_band> m_bands;
    std::vector<double> m_coeff;
    std::uint64_t m_position{ 0 };
    detail::plan_ptr<sdsp_hip_duc_plan, sdsp_hip_duc_plan_destroy> m_plan;
    detail::device_buffer m_state;
};
} // namespace sdsp

#endif // SDSP_MI355X_DUC_H
