// sdsp/pfb_synth.h -- streaming polyphase synthesis filter bank for the MI355X engine (sdsp_hip_pfb_synth_*).
//
// The inverse of sdsp::pfb_bank (sdsp/pfb.h): rebuilds each of a bank of real or complex streams on the device from frames of
// n_channels sub-bands in pfb_bank's output layout -- per frame one reverse n_channels-point transform of the library, then every
// output sample gathers the frames that cover it times the synthesis prototype.  RAII plan and device-resident per-stream pending
// sums, process() on device pointers, process_host() for host buffers.  A call of F frames per stream writes F * hop samples
// (interleaved re, im pairs of real_t for complex output).  The default prototype is the dual of pfb_bank's default (Hamming) at this
// hop, so that pfb_synthesis_bank(pfb_bank(x)) is x delayed by hist() samples; the constructor throws where that prototype has no
// dual (hops above n_channels / 2 with more than one tap per channel, typically).  There is no CPU path.
#ifndef SDSP_MI355X_PFB_SYNTH_H
#define SDSP_MI355X_PFB_SYNTH_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
// the minimum-norm synthesis prototype that reconstructs through the analysis prototype h at this hop (sdsp_hip_pfb_dual_prototype)
inline std::vector<double> pfb_dual_prototype(const std::vector<double> &h, std::uint32_t n_channels, std::uint32_t taps_per_channel,
                                              std::uint32_t hop)
{
    if (h.size() != static_cast<std::size_t>(n_channels) * taps_per_channel)
        detail::check(SDSP_HIP_ERR_INVALID_SIZE);
    std::vector<double> g(h.size() + 1);
    detail::check(sdsp_hip_pfb_dual_prototype(n_channels, taps_per_channel, hop, h.data(), g.data()));
    g.pop_back();
    return g;
}

template <typename real_t = float> class pfb_synthesis_bank {
public:
    pfb_synthesis_bank(std::uint32_t n_channels, std::uint32_t taps_per_channel, std::uint32_t hop, std::uint64_t streams,
                       int output_kind = SDSP_HIP_PFB_REAL, int phase = SDSP_HIP_PFB_PHASE_TIME, int device = 0)
        : m_m(n_channels), m_p(taps_per_channel), m_hop(hop), m_streams(streams), m_kind(output_kind), m_phase(phase), m_device(device)
    {
        set_dual_of_prototype(SDSP_HIP_WINDOW_HAMMING);
    }
    pfb_synthesis_bank(const pfb_synthesis_bank &) = delete;
    pfb_synthesis_bank &operator=(const pfb_synthesis_bank &) = delete;

    // the synthesis prototype itself: taps_per_channel * n_channels taps
    void set_taps(const std::vector<double> &g)
    {
        if (g.size() != static_cast<std::size_t>(m_m) * m_p)
            detail::check(SDSP_HIP_ERR_INVALID_SIZE);
        m_taps = g;
        m_plan.reset();
    }
    // the dual of an analysis prototype h
    void set_dual_of(const std::vector<double> &h) { set_taps(pfb_dual_prototype(h, m_m, m_p, m_hop)); }
    // the dual of the windowed-sinc prototype sdsp_hip_pfb_prototype(window_kind): SDSP_HIP_WINDOW_*
    void set_dual_of_prototype(int window_kind)
    {
        std::vector<double> h(static_cast<std::size_t>(m_m) * m_p + 1);
        detail::check(sdsp_hip_pfb_prototype(window_kind, m_m, m_p, h.data()));
        h.pop_back();
        set_dual_of(h);
    }
    // forget the pending sums and the stream position
    void reset()
    {
        if (m_state)
            zero_state();
        m_position = 0;
    }

    std::uint32_t bins() const noexcept { return m_kind == SDSP_HIP_PFB_COMPLEX ? m_m : m_m / 2 + 1; }
    std::uint32_t hist() const noexcept { return m_m * m_p - m_hop; } // pending sums per stream, time order: the round-trip delay
    // real_t values per output sample: 2 for complex output
    std::uint32_t sample_values() const noexcept { return m_kind == SDSP_HIP_PFB_COMPLEX ? 2u : 1u; }
    std::uint64_t position() const noexcept { return m_position; }
    std::uint64_t streams() const noexcept { return m_streams; }
    const std::vector<double> &taps() const { return m_taps; }

    // device pointers, stream-major; strides count bins and samples; asynchronous on `stream`; continues every stream
    void process(const void *device_in, std::uint64_t in_stride, real_t *device_out, std::uint64_t out_stride, std::uint64_t frames,
                 void *stream = nullptr)
    {
        ensure_plan();
        ensure_state();
        detail::check(sdsp_hip_pfb_synth_process(m_plan.get(), device_in, in_stride, device_out, out_stride, m_streams, frames, m_position,
                                                 m_state.get(), stream));
        m_position += frames * m_hop;
    }
    // host pointers: in = streams x frames x bins() x 2, out = streams x frames * hop x sample_values(), both contiguous
    void process_host(const real_t *host_in, real_t *host_out, std::uint64_t frames)
    {
        ensure_plan();
        ensure_state();
        const std::uint64_t in_row = frames * bins(), out_row = frames * m_hop;
        const std::size_t in_bytes = static_cast<std::size_t>(m_streams * in_row * 2) * sizeof(real_t);
        const std::size_t out_bytes = static_cast<std::size_t>(m_streams * out_row * sample_values()) * sizeof(real_t);
        if (in_bytes == 0)
            return;
        detail::host_stage(m_device, { { host_in, nullptr, in_bytes }, { nullptr, host_out, out_bytes } }, [&](void *const *dev) {
            return sdsp_hip_pfb_synth_process(m_plan.get(), dev[0], in_row, dev[1], out_row, m_streams, frames, m_position, m_state.get(),
                                              nullptr);
        });
        m_position += out_row;
    }
    sdsp_hip_pfb_synth_plan_info info()
    {
        ensure_plan();
        sdsp_hip_pfb_synth_plan_info i{};
        detail::check(sdsp_hip_pfb_synth_plan_get_info(m_plan.get(), &i));
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
        sdsp_hip_pfb_synth_plan *plan = nullptr;
        detail::check(sdsp_hip_pfb_synth_plan_create(&plan, m_m, m_p, m_hop, m_taps.data(), m_kind, m_phase,
                                                     detail::precision_of<real_t>::value, 0, m_device));
        m_plan.reset(plan);
    }
    void zero_state()
    {
        if (!m_state)
            m_state.alloc(state_values() * sizeof(real_t), m_device);
        m_state.fill(state_values(), real_t(0));
    }
    void ensure_state()
    {
        if (!m_state)
            zero_state();
    }

    std::uint32_t m_m, m_p, m_hop;
    std::uint64_t m_streams;
    int m_kind, m_phase, m_device;
    std::uint64_t m_position{ 0 };
    std::vector<double> m_taps;
    detail::plan_ptr<sdsp_hip_pfb_synth_plan, sdsp_hip_pfb_synth_plan_destroy> m_plan;
    detail::device_buffer m_state;
};
} // namespace sdsp

#endif // SDSP_MI355X_PFB_SYNTH_H
