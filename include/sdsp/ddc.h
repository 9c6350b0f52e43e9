// sdsp/ddc.h -- digital down-converter bank for the MI355X engine (sdsp_hip_ddc_*).
//
// From `channels` input streams a list of bands (source channel, frequency word, phase word) is shifted to baseband, filtered with one
// real low-pass and decimated by `down`, out of place, with the oscillator phase continuous across calls.  Mirrors
// sdsp::fir_resampler_bank (sdsp/resample.h): RAII plan and device-resident per-channel history, process() on device pointers,
// process_host() for host buffers; the bank counts the stream position.  A call of S samples per channel (S a multiple of down)
// writes S / down interleaved complex outputs per band.  No reference counterpart: pinned to mix -> scipy.signal.upfirdn.  There is
// no CPU path.
#ifndef SDSP_MI355X_DDC_H
#define SDSP_MI355X_DDC_H

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
// round(f 2^32) mod 2^32 for f in [-0.5, 0.5] cycles per sample (or cycles of phase); throws outside
inline std::uint32_t ddc_phase_word(double cycles)
{
    std::uint32_t w = 0;
    detail::check(sdsp_hip_ddc_phase_word(cycles, &w));
    return w;
}

template <typename real_t = float> class ddc_bank {
public:
    // complex_input: rows of interleaved I/Q pairs (one pair is one sample) instead of real samples
    ddc_bank(std::uint32_t n_taps, std::uint32_t down, std::vector<sdsp_hip_ddc_band> bands, std::uint32_t channels = 1,
             bool complex_input = false, int device = 0)
        : m_taps(n_taps), m_down(down), m_channels(channels), m_complex(complex_input), m_device(device), m_bands(std::move(bands)),
          m_coeff(n_taps, 0.0)
    {
    }
    ddc_bank(const ddc_bank &) = delete;
    ddc_bank &operator=(const ddc_bank &) = delete;

    void set_coeff(const std::vector<double> &h)
    {
        if (h.size() != m_taps)
            throw hip_error(SDSP_HIP_ERR_INVALID_SIZE, "sdsp_hip: coefficient count differs from n_taps");
        m_coeff = h;
        m_plan.reset();
    }
    // Hamming low-pass at 1 / (2 down) of the input rate, unit gain (sdsp_hip_resample_design(n_taps, 1, down)); needs down >= 2
    void set_antialias_coeff()
    {
        detail::check(sdsp_hip_resample_design(m_taps, 1, m_down, m_coeff.data()));
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
        detail::check(sdsp_hip_ddc_out_samples(m_down, samples, &n));
        return n;
    }

    // device pointers (in: channel-major rows of reals or I/Q pairs; out: one row of I/Q pairs per band), strides in elements,
    // asynchronous on `stream`; continues every channel's stream
    void process(const real_t *device_in, std::uint64_t in_stride, real_t *device_out, std::uint64_t out_stride, std::uint64_t samples,
                 void *stream = nullptr)
    {
        ensure_plan();
        ensure_state();
        detail::check(sdsp_hip_ddc_process(m_plan.get(), device_in, in_stride, device_out, out_stride, samples, m_position, m_state.get(),
                                           stream));
        m_position += samples;
    }
    // host pointers: in = channels x samples elements, out = bands x out_samples(samples) I/Q pairs, both contiguous
    void process_host(const real_t *host_in, real_t *host_out, std::uint64_t samples)
    {
        ensure_plan();
        ensure_state();
        const std::uint64_t outs = out_samples(samples);
        const std::size_t in_bytes = static_cast<std::size_t>(m_channels * samples) * in_elem_bytes();
        const std::size_t out_bytes = static_cast<std::size_t>(m_bands.size() * outs) * 2 * sizeof(real_t);
        if (samples == 0)
            return;
        detail::host_stage(m_device, { { host_in, nullptr, in_bytes }, { nullptr, host_out, out_bytes } }, [&](void *const *dev) {
            return sdsp_hip_ddc_process(m_plan.get(), dev[0], samples, dev[1], outs, samples, m_position, m_state.get(), nullptr);
        });
        m_position += samples;
    }
    std::uint32_t channels() const noexcept { return m_channels; }
    std::size_t bands() const noexcept { return m_bands.size(); }
    std::uint64_t position() const noexcept { return m_position; }
    void set_position(std::uint64_t position) noexcept { m_position = position; }
    const std::vector<double> &coeff() const { return m_coeff; }
    sdsp_hip_ddc_plan_info info()
    {
        ensure_plan();
        sdsp_hip_ddc_plan_info i{};
        detail::check(sdsp_hip_ddc_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    std::size_t in_elem_bytes() const noexcept { return (m_complex ? 2u : 1u) * sizeof(real_t); }
    void ensure_plan()
    {
        if (m_plan)
            return;
        sdsp_hip_ddc_plan *plan = nullptr;
        detail::check(sdsp_hip_ddc_plan_create(&plan, m_taps, m_coeff.data(), m_down, m_channels,
                                               static_cast<std::uint32_t>(m_bands.size()), m_bands.data(),
                                               m_complex ? SDSP_HIP_DDC_COMPLEX : SDSP_HIP_DDC_REAL,
                                               detail::precision_of<real_t>::value, m_device));
        m_plan.reset(plan);
    }
    void zero_state()
    {
        const std::size_t len = m_taps > 1 ? m_taps - 1 : 1;
        const std::size_t bytes = len * m_channels * in_elem_bytes();
        if (!m_state)
            m_state.alloc(bytes, m_device);
        m_state.fill<unsigned char>(bytes, 0);
    }
    void ensure_state()
    {
        if (!m_state)
            zero_state();
    }

    std::uint32_t m_taps, m_down, m_channels;
    bool m_complex;
    int m_device;
    std::vector<sdsp_hip_ddc_band> m_bands;
    std::vector<double> m_coeff;
    std::uint64_t m_position{ 0 };
    detail::plan_ptr<sdsp_hip_ddc_plan, sdsp_hip_ddc_plan_destroy> m_plan;
    detail::device_buffer m_state;
};
} // namespace sdsp

#endif // SDSP_MI355X_DDC_H
