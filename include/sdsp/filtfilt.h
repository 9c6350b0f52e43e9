// sdsp/filtfilt.h -- zero-phase forward-backward filtering of biquad cascades for the MI355X engine (sdsp_hip_filtfilt_*, DESIGN.md
// section 5.13).
//
// scipy.signal.sosfiltfilt for a bank of whole records at once: each row is extended at both ends (odd / even / constant), run forward
// through the cascade from its steady state, then backward, and its middle written back in place.  The cascade is the one
// sdsp::casc_2o_iir_bank runs (m_t sections, GENERIC / LP / HP / BP, the library's designs); real_t float or double sets the sample and
// recurrence type.  RAII plan, process() on device pointers, process_host() for host buffers, in the style of sdsp::istft_bank.  There is
// no CPU path.
#ifndef SDSP_MI355X_FILTFILT_H
#define SDSP_MI355X_FILTFILT_H

#include <array>
#include <cstddef>
#include <cstdint>

#include "detail/hip_runtime.h"

namespace sdsp
{
template <std::uint32_t m_t, typename real_t = float> class filtfilt_bank {
    static_assert(m_t >= 2 && m_t % 2 == 0 && m_t <= SDSP_HIP_MAX_SECTIONS, "m_t must be even, 2 .. 16");

public:
    using coeff_array = std::array<double, 3 * m_t>;

    // padlen < 0: scipy's default for the cascade (ignored for SDSP_HIP_PAD_NONE)
    explicit filtfilt_bank(int padtype = SDSP_HIP_PAD_ODD, std::int64_t padlen = -1, int device = 0)
        : m_padtype(padtype), m_padlen(padlen), m_device(device)
    {
    }
    filtfilt_bank(const filtfilt_bank &) = delete;
    filtfilt_bank &operator=(const filtfilt_bank &) = delete;

    // the library's Butterworth designs (sdsp_hip_iir_design_*) on the numerator-folded kinds
    void set_lp_coeff(double f0, double fs, double gain_in = 1.0)
    {
        detail::check(sdsp_hip_iir_design_lp(m_t, f0, fs, gain_in, m_a.data(), m_b.data(), &m_gain));
        designed(SDSP_HIP_IIR_LP);
    }
    void set_hp_coeff(double f0, double fs, double gain_in = 1.0)
    {
        detail::check(sdsp_hip_iir_design_hp(m_t, f0, fs, gain_in, m_a.data(), m_b.data(), &m_gain));
        designed(SDSP_HIP_IIR_HP);
    }
    void set_bp_coeff(double f0, double fs, double q, double gain_in = 1.0)
    {
        detail::check(sdsp_hip_iir_design_bp(m_t, f0, fs, q, gain_in, m_a.data(), m_b.data(), &m_gain));
        designed(SDSP_HIP_IIR_BP);
    }
    // any cascade on the GENERIC kind: a, b = [1, c1, c2] per section, gain in front of the first
    void set_coeff(const coeff_array &a, const coeff_array &b, double gain)
    {
        m_a = a;
        m_b = b;
        m_gain = gain;
        designed(SDSP_HIP_IIR_GENERIC);
    }

    // device pointer, `channels` rows of `samples` at `stride` elements; in place, asynchronous on `stream`
    void process(real_t *device_data, std::uint64_t channels, std::uint64_t samples, std::uint64_t stride, void *stream = nullptr)
    {
        ensure_plan();
        detail::check(sdsp_hip_filtfilt_process(m_plan.get(), device_data, channels, samples, stride, stream));
    }
    // host pointer, contiguous rows; synchronous
    void process_host(real_t *host_data, std::uint64_t channels, std::uint64_t samples)
    {
        ensure_plan();
        detail::check(sdsp_hip_filtfilt_process_host(m_plan.get(), host_data, channels, samples, samples));
    }
    std::array<double, m_t + 1> steady_state() const
    {
        std::array<double, m_t + 1> s{};
        detail::check(sdsp_hip_iir_steady_state(m_t, m_kind, m_a.data(), m_b.data(), m_gain, s.data()));
        return s;
    }
    sdsp_hip_filtfilt_plan_info info()
    {
        ensure_plan();
        sdsp_hip_filtfilt_plan_info i{};
        detail::check(sdsp_hip_filtfilt_plan_get_info(m_plan.get(), &i));
        return i;
    }
    int kind() const noexcept { return m_kind; }
    double gain() const noexcept { return m_gain; }
    const coeff_array &a() const noexcept { return m_a; }
    const coeff_array &b() const noexcept { return m_b; }

private:
    void designed(int kind)
    {
        m_kind = kind;
        m_plan.reset();
    }
    void ensure_plan()
    {
        if (m_plan)
            return;
        sdsp_hip_filtfilt_plan *plan = nullptr;
        detail::check(sdsp_hip_filtfilt_plan_create(&plan, m_t, m_kind, m_a.data(), m_b.data(), m_gain, detail::precision_of<real_t>::value,
                                                    m_padtype, m_padlen, 0, m_device));
        m_plan.reset(plan);
    }

    int m_padtype;
    std::int64_t m_padlen;
    int m_device;
    int m_kind{ SDSP_HIP_IIR_GENERIC };
    double m_gain{ 1.0 };
    coeff_array m_a{};
    coeff_array m_b{};
    detail::plan_ptr<sdsp_hip_filtfilt_plan, sdsp_hip_filtfilt_plan_destroy> m_plan;
};
} // namespace sdsp

#endif // SDSP_MI355X_FILTFILT_H
