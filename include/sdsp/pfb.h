// sdsp/pfb.h -- streaming polyphase filter-bank channelizer bank for the MI355X engine (sdsp_hip_pfb_*).
//
// Splits each of a bank of real or complex streams on the device into n_channels equally spaced sub-bands with a prototype low-pass
// of taps_per_channel * n_channels taps: per frame one fold of the polyphase branches and one n_channels-point transform of the
// library.  Mirrors sdsp::stft_bank (sdsp/stft.h): RAII plan and device-resident per-stream history, process() on device pointers,
// process_host() for host buffers; the sizes are run-time values here (a prototype may have 2^20 taps).  A call of S samples per
// stream (S a multiple of hop) writes S / hop frames of bins() interleaved complex values: n_channels / 2 + 1 for real input,
// n_channels for complex input (samples then are interleaved re, im pairs of real_t).  The taps multiply the samples in window
// (correlation) order, as the STFT window does; pass the reversed taps for a prototype meant in convolution order.  The bank counts
// the samples it has consumed: SDSP_HIP_PFB_PHASE_TIME refers every sub-band's phase to the start of the stream.  There is no CPU path.
#ifndef SDSP_MI355X_PFB_H
#define SDSP_MI355X_PFB_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
template <typename real_t = float> class pfb_bank {
public:
    pfb_bank(std::uint32_t n_channels, std::uint32_t taps_per_channel, std::uint32_t hop, std::uint64_t streams,
             int input_kind = SDSP_HIP_PFB_REAL, int phase = SDSP_HIP_PFB_PHASE_TIME, int device = 0)
        : m_m(n_channels), m_p(taps_per_channel), m_hop(hop), m_streams(streams), m_kind(input_kind), m_phase(phase), m_device(device)
    {
        set_prototype(SDSP_HIP_WINDOW_HAMMING);
    }
    pfb_bank(const pfb_bank &) = delete;
    pfb_bank &operator=(const pfb_bank &) = delete;

    // taps_per_channel * n_channels taps, window (correlation) order
    void set_taps(const std::vector<double> &h)
    {
        if (h.size() != static_cast<std::size_t>(m_m) * m_p)
            detail::check(SDSP_HIP_ERR_INVALID_SIZE);
        m_taps = h;
        m_plan.reset();
    }
    // windowed-sinc prototype, cutoff at half the sub-band spacing, unit DC gain (sdsp_hip_pfb_prototype): SDSP_HIP_WINDOW_*
    void set_prototype(int window_kind)
    {
        std::vector<double> h(static_cast<std::size_t>(m_m) * m_p + 1);
        detail::check(sdsp_hip_pfb_prototype(window_kind, m_m, m_p, h.data()));
        h.pop_back();
        m_taps = h;
        m_plan.reset();
    }
    void preload_filter(double value) { fill_state(static_cast<real_t>(value)); }
    // forget the history and the stream position
    void reset()
    {
        if (m_state)
            fill_state(real_t(0));
        m_position = 0;
    }

    std::uint32_t bins() const noexcept { return m_kind == SDSP_HIP_PFB_COMPLEX ? m_m : m_m / 2 + 1; }
    std::uint32_t hist() const noexcept { return m_m * m_p - m_hop; } // history per stream in samples, newest first
    // real_t values per input sample: 2 for complex input
    std::uint32_t sample_values() const noexcept { return m_kind == SDSP_HIP_PFB_COMPLEX ? 2u : 1u; }
    std::uint64_t position() const noexcept { return m_position; }
    std::uint64_t streams() const noexcept { return m_streams; }
    const std::vector<double> &taps() const { return m_taps; }
    // frames of a call of `samples` per stream; throws unless samples is a multiple of hop
    std::uint64_t frames(std::uint64_t samples) const
    {
        std::uint64_t n = 0;
        detail::check(sdsp_hip_pfb_frames(m_hop, samples, &n));
        return n;
    }

    // device pointers, stream-major; strides count samples and bins; asynchronous on `stream`; continues every stream
    void process(const real_t *device_in, std::uint64_t in_stride, void *device_out, std::uint64_t out_stride, std::uint64_t samples,
                 void *stream = nullptr)
    {
        ensure_plan();
        ensure_state();
        detail::check(sdsp_hip_pfb_process(m_plan.get(), device_in, in_stride, device_out, out_stride, m_streams, samples, m_position,
                                           m_state.get(), stream));
        m_position += samples;
    }
    // host pointers: in = streams x samples x sample_values(), out = streams x frames(samples) x bins() x 2, both contiguous
    void process_host(const real_t *host_in, real_t *host_out, std::uint64_t samples)
    {
        ensure_plan();
        ensure_state();
        const std::uint64_t row = frames(samples) * bins();
        const std::size_t in_bytes = static_cast<std::size_t>(m_streams * samples * sample_values()) * sizeof(real_t);
        const std::size_t out_bytes = static_cast<std::size_t>(m_streams * row * 2) * sizeof(real_t);
        if (in_bytes == 0)
            return;
        detail::host_stage(m_device, { { host_in, nullptr, in_bytes }, { nullptr, host_out, out_bytes } }, [&](void *const *dev) {
            return sdsp_hip_pfb_process(m_plan.get(), dev[0], samples, dev[1], row, m_streams, samples, m_position, m_state.get(), nullptr);
        });
        m_position += samples;
    }
    sdsp_hip_pfb_plan_info info()
    {
        ensure_plan();
        sdsp_hip_pfb_plan_info i{};
        detail::check(sdsp_hip_pfb_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    std::size_t state_values() const
    {
        const std::size_t h = hist() > 0 ? hist() : 1;
        return h * static_cast<std::size_t>(m_streams) * sample_values();
    }
    void ensure_plan()
    {
        if (m_plan)
            return;
        sdsp_hip_pfb_plan *plan = nullptr;
        detail::check(sdsp_hip_pfb_plan_create(&plan, m_m, m_p, m_hop, m_taps.data(), m_kind, m_phase, detail::precision_of<real_t>::value,
                                               0, m_device));
        m_plan.reset(plan);
    }
    void fill_state(real_t v)
    {
        if (!m_state)
            m_state.alloc(state_values() * sizeof(real_t), m_device);
        std::vector<real_t> host(state_values(), v);
        if (m_kind == SDSP_HIP_PFB_COMPLEX) // a steady real value: zero imaginary parts
            for (std::size_t i = 1; i < host.size(); i += 2)
                host[i] = real_t(0);
        m_state.upload(host.data(), host.size() * sizeof(real_t));
    }
    void ensure_state()
    {
        if (!m_state)
            fill_state(real_t(0));
    }

    std::uint32_t m_m, m_p, m_hop;
    std::uint64_t m_streams;
    int m_kind, m_phase, m_device;
    std::uint64_t m_position{ 0 };
    std::vector<double> m_taps;
    detail::plan_ptr<sdsp_hip_pfb_plan, sdsp_hip_pfb_plan_destroy> m_plan;
    detail::device_buffer m_state;
};
} // namespace sdsp

#endif // SDSP_MI355X_PFB_H
