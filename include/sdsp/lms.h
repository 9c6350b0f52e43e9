// sdsp/lms.h -- LMS / NLMS adaptive filter bank for the MI355X engine (sdsp_hip_lms_*).
//
// `channels` independent adaptive FIR filters of n_taps weights each: process() filters the reference rows x with the current weights,
// compares with the desired rows d and moves the weights with every sample; it writes the a-priori output y and error e, either of
// which may be left out.  Mirrors sdsp::beamformer_bank (sdsp/beamformer.h): RAII plan and device-resident state, process() on device
// pointers, process_host() for host buffers.  The state holds the weights, [channel][tap], followed by the x history; weights() and
// set_weights() copy the first part.  No reference counterpart: pinned to a scalar loop and to scipy.signal.lfilter.  There is no CPU
// path.
#ifndef SDSP_MI355X_LMS_H
#define SDSP_MI355X_LMS_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
template <typename real_t = float> class lms_bank {
public:
    // complex_rows: rows and weights of interleaved I/Q pairs (one pair is one element); normalised: NLMS, the step is
    // mu / (eps + the window's energy), eps > 0
    lms_bank(std::uint64_t channels, std::uint32_t n_taps, bool complex_rows = false, bool normalised = false, double eps = 0.0,
             int device = 0)
        : m_channels(channels), m_taps(n_taps), m_complex(complex_rows), m_device(device)
    {
        sdsp_hip_lms_plan *plan = nullptr;
        detail::check(sdsp_hip_lms_plan_create(&plan, channels, n_taps, complex_rows ? SDSP_HIP_LMS_COMPLEX : SDSP_HIP_LMS_REAL,
                                               detail::precision_of<real_t>::value, normalised ? SDSP_HIP_LMS_NLMS : SDSP_HIP_LMS_LMS, eps,
                                               device));
        m_plan.reset(plan);
    }
    lms_bank(const lms_bank &) = delete;
    lms_bank &operator=(const lms_bank &) = delete;

    // zero weights, zero history
    void reset()
    {
        if (m_state)
            zero_state();
    }

    // device pointers (channel-major rows of reals or I/Q pairs, strides in elements; y and e may be null), asynchronous on `stream`;
    // continues every channel's stream
    void process(const real_t *device_x, std::uint64_t x_stride, const real_t *device_d, std::uint64_t d_stride, real_t *device_y,
                 std::uint64_t y_stride, real_t *device_e, std::uint64_t e_stride, std::uint64_t samples, double mu, void *stream = nullptr)
    {
        ensure_state();
        detail::check(sdsp_hip_lms_process(m_plan.get(), device_x, x_stride, device_d, d_stride, device_y, y_stride, device_e, e_stride,
                                           samples, mu, m_state.get(), stream));
    }
    // host pointers: contiguous channels x samples elements each; y and e may be null
    void process_host(const real_t *host_x, const real_t *host_d, real_t *host_y, real_t *host_e, std::uint64_t samples, double mu)
    {
        ensure_state();
        if (samples == 0)
            return;
        const std::size_t bytes = static_cast<std::size_t>(m_channels * samples) * elem_bytes();
        const detail::stage_item items[] = { { host_x, nullptr, bytes }, { host_d, nullptr, bytes }, { nullptr, host_y, bytes },
                                             { nullptr, host_e, bytes } };
        detail::host_stage(m_device, items, [&](void *const *dev) {
            return sdsp_hip_lms_process(m_plan.get(), dev[0], samples, dev[1], samples, dev[2], samples, dev[3], samples, samples, mu,
                                        m_state.get(), nullptr);
        });
    }
    // the weights, [channel][tap] (x 2, interleaved re, im, for complex rows), copied from the device state: the identified systems
    std::vector<real_t> weights()
    {
        ensure_state();
        std::vector<real_t> w(weight_elems() * (m_complex ? 2u : 1u));
        m_state.download(w.data(), weight_elems() * elem_bytes());
        return w;
    }
    // ... copied into it; the history stays
    void set_weights(const std::vector<real_t> &w)
    {
        if (w.size() != weight_elems() * (m_complex ? 2u : 1u))
            throw hip_error(SDSP_HIP_ERR_INVALID_SIZE, "sdsp_hip: weights must be channels x n_taps");
        ensure_state();
        m_state.upload(w.data(), weight_elems() * elem_bytes());
    }
    std::uint64_t channels() const noexcept { return m_channels; }
    std::uint32_t taps() const noexcept { return m_taps; }
    void set_variant(int variant) { detail::check(sdsp_hip_lms_plan_set_variant(m_plan.get(), variant)); }
    sdsp_hip_lms_plan_info info() const
    {
        sdsp_hip_lms_plan_info i{};
        detail::check(sdsp_hip_lms_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    std::size_t elem_bytes() const noexcept { return (m_complex ? 2u : 1u) * sizeof(real_t); }
    std::size_t weight_elems() const noexcept { return static_cast<std::size_t>(m_channels) * m_taps; }
    void zero_state()
    {
        std::uint64_t bytes = 0;
        detail::check(sdsp_hip_lms_state_bytes(m_plan.get(), &bytes));
        if (!m_state)
            m_state.alloc(static_cast<std::size_t>(bytes), m_device);
        m_state.fill<unsigned char>(static_cast<std::size_t>(bytes), 0);
    }
    void ensure_state()
    {
        if (!m_state)
            zero_state();
    }

    std::uint64_t m_channels;
    std::uint32_t m_taps;
    bool m_complex;
    int m_device;
    detail::plan_ptr<sdsp_hip_lms_plan, sdsp_hip_lms_plan_destroy> m_plan;
    detail::device_buffer m_state;
};
} // namespace sdsp

#endif // SDSP_MI355X_LMS_H
