// sdsp/beamformer.h -- time-delay (filter-and-sum) beamformer bank for the MI355X engine (sdsp_hip_beam_*).
//
// `groups` sensor arrays of `sensors` rows each are steered into `beams` rows each: a beam is the sum over its entries of the entry's
// sensor delayed by whole samples and filtered with the entry's own taps (a fractional-delay filter that carries the weight), out of
// place.  Mirrors sdsp::ddc_bank (sdsp/ddc.h): RAII plan and device-resident per-row history, process() on device pointers,
// process_host() for host buffers.  There is no stream position: the operation is time-invariant.  A call of S samples per row
// writes S outputs per beam.  No reference counterpart: pinned to a sum of scipy.signal.lfilter runs.  There is no CPU path.
#ifndef SDSP_MI355X_BEAMFORMER_H
#define SDSP_MI355X_BEAMFORMER_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
// Kaiser-windowed-sinc fractional-delay taps for a delay of tau samples (sdsp_hip_beam_delay_taps): returns the whole-sample part and
// fills g with n_taps values that sum to `weight`; an entry with them delays by tau + (n_taps - 1) / 2 samples
inline std::uint32_t beam_delay_taps(double tau, double weight, std::uint32_t n_taps, double beta, double *g)
{
    std::uint32_t delay = 0;
    detail::check(sdsp_hip_beam_delay_taps(tau, weight, n_taps, beta, &delay, g));
    return delay;
}

template <typename real_t = float> class beamformer_bank {
public:
    // complex_rows: rows of interleaved I/Q pairs (one pair is one sample) and complex taps instead of reals
    beamformer_bank(std::uint32_t sensors, std::uint32_t beams, std::uint32_t n_taps, std::uint32_t groups = 1, bool complex_rows = false,
                    int device = 0)
        : m_sensors(sensors), m_beams(beams), m_taps(n_taps), m_groups(groups), m_complex(complex_rows), m_device(device)
    {
    }
    beamformer_bank(const beamformer_bank &) = delete;
    beamformer_bank &operator=(const beamformer_bank &) = delete;

    // entries sorted by beam and, within a beam, by strictly ascending sensor; taps: entries.size() x n_taps doubles (x 2, interleaved
    // re, im, for complex rows).  Drops the plan and the history.
    void set_entries(std::vector<sdsp_hip_beam_entry> entries, std::vector<double> taps)
    {
        if (taps.size() != entries.size() * m_taps * (m_complex ? 2u : 1u))
            throw hip_error(SDSP_HIP_ERR_INVALID_SIZE, "sdsp_hip: tap count differs from entries x n_taps");
        m_entries = std::move(entries);
        m_coeff = std::move(taps);
        m_plan.reset();
        m_state.reset();
    }
    // every beam uses every sensor with a designed fractional delay: tau and weights are beams x sensors, row-major (real rows, or
    // complex rows with real weights)
    void set_steering(const std::vector<double> &tau, const std::vector<double> &weights, double beta)
    {
        const std::size_t n = static_cast<std::size_t>(m_beams) * m_sensors, width = m_complex ? 2u : 1u;
        if (tau.size() != n || weights.size() != n)
            throw hip_error(SDSP_HIP_ERR_INVALID_SIZE, "sdsp_hip: tau and weights must be beams x sensors");
        std::vector<sdsp_hip_beam_entry> entries(n);
        std::vector<double> taps(n * m_taps * width, 0.0), g(m_taps);
        for (std::uint32_t b = 0; b < m_beams; b++)
            for (std::uint32_t c = 0; c < m_sensors; c++) {
                const std::size_t i = static_cast<std::size_t>(b) * m_sensors + c;
                entries[i] = { b, c, beam_delay_taps(tau[i], weights[i], m_taps, beta, g.data()) };
                for (std::uint32_t t = 0; t < m_taps; t++)
                    taps[(i * m_taps + t) * width] = g[t];
            }
        set_entries(std::move(entries), std::move(taps));
    }
    // forget the history
    void reset()
    {
        if (m_state)
            zero_state();
    }

    // device pointers (channel-major rows of reals or I/Q pairs: groups x sensors in, groups x beams out), strides in elements,
    // asynchronous on `stream`; continues every row's stream
    void process(const real_t *device_in, std::uint64_t in_stride, real_t *device_out, std::uint64_t out_stride, std::uint64_t samples,
                 void *stream = nullptr)
    {
        ensure_plan();
        ensure_state();
        detail::check(sdsp_hip_beam_process(m_plan.get(), device_in, in_stride, device_out, out_stride, samples, m_state.get(), stream));
    }
    // host pointers: in = groups x sensors x samples elements, out = groups x beams x samples elements, both contiguous
    void process_host(const real_t *host_in, real_t *host_out, std::uint64_t samples)
    {
        ensure_plan();
        ensure_state();
        if (samples == 0)
            return;
        const std::size_t in_bytes = static_cast<std::size_t>(m_groups) * m_sensors * samples * elem_bytes();
        const std::size_t out_bytes = static_cast<std::size_t>(m_groups) * m_beams * samples * elem_bytes();
        detail::host_stage(m_device, { { host_in, nullptr, in_bytes }, { nullptr, host_out, out_bytes } }, [&](void *const *dev) {
            return sdsp_hip_beam_process(m_plan.get(), dev[0], samples, dev[1], samples, samples, m_state.get(), nullptr);
        });
    }
    std::uint32_t sensors() const noexcept { return m_sensors; }
    std::uint32_t beams() const noexcept { return m_beams; }
    std::uint32_t groups() const noexcept { return m_groups; }
    // elements of history per input row: the largest delay + n_taps - 1
    std::uint32_t hist() const noexcept
    {
        std::uint32_t d = 0;
        for (const sdsp_hip_beam_entry &e : m_entries)
            d = std::max(d, e.delay);
        return d + m_taps - 1;
    }
    const std::vector<sdsp_hip_beam_entry> &entries() const { return m_entries; }
    const std::vector<double> &coeff() const { return m_coeff; }
    void set_variant(int variant)
    {
        ensure_plan();
        detail::check(sdsp_hip_beam_plan_set_variant(m_plan.get(), variant));
    }
    sdsp_hip_beam_plan_info info()
    {
        ensure_plan();
        sdsp_hip_beam_plan_info i{};
        detail::check(sdsp_hip_beam_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    std::size_t elem_bytes() const noexcept { return (m_complex ? 2u : 1u) * sizeof(real_t); }
    void ensure_plan()
    {
        if (m_plan)
            return;
        sdsp_hip_beam_plan *plan = nullptr;
        detail::check(sdsp_hip_beam_plan_create(&plan, m_sensors, m_beams, m_groups, m_taps, static_cast<std::uint32_t>(m_entries.size()),
                                                m_entries.data(), m_coeff.data(), m_complex ? SDSP_HIP_BEAM_COMPLEX : SDSP_HIP_BEAM_REAL,
                                                detail::precision_of<real_t>::value, m_device));
        m_plan.reset(plan);
    }
    void zero_state()
    {
        const std::size_t len = std::max<std::size_t>(hist(), 1);
        const std::size_t bytes = len * m_groups * m_sensors * elem_bytes();
        if (!m_state)
            m_state.alloc(bytes, m_device);
        m_state.fill<unsigned char>(bytes, 0);
    }
    void ensure_state()
    {
        if (!m_state)
            zero_state();
    }

    std::uint32_t m_sensors, m_beams, m_taps, m_groups;
    bool m_complex;
    int m_device;
    std::vector<sdsp_hip_beam_entry> m_entries;
    std::vector<double> m_coeff;
    detail::plan_ptr<sdsp_hip_beam_plan, sdsp_hip_beam_plan_destroy> m_plan;
    detail::device_buffer m_state;
};
} // namespace sdsp

#endif // SDSP_MI355X_BEAMFORMER_H
