// sdsp/fsync.h -- streaming frame synchroniser banks for the MI355X engine (sdsp_hip_fsync_*).
//
// The stage between sdsp::viterbi_bank and sdsp::rs_decoder: compact rows of bits in (in_t = std::uint8_t: one byte per bit;
// std::uint32_t: packed words, the oldest bit lowest), the attached sync marker found at any bit offset and in either polarity, a
// SEARCH / VERIFY / LOCK machine with a flywheel per channel, and the payloads behind accepted markers out as compact frames of bytes,
// the first bit most significant, inversion and pseudo-random sequence removed.  The frames, records and state are the contract's in
// front of sdsp_hip_fsync_plan_create, in either kernel variant and for any split of a stream into calls.  Mirrors sdsp::rs_decoder's
// plan handling (sdsp/rs.h): an RAII plan that owns its device state, process() on device pointers, process_host() for host buffers
// through detail::host_stage, info().  ccsds_pn, attach_sync and fsync_max_frames run on the host; there is no CPU synchroniser.
#ifndef SDSP_MI355X_FSYNC_H
#define SDSP_MI355X_FSYNC_H

#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
enum class sync_polarity : int { normal = SDSP_HIP_FSYNC_NORMAL, either = SDSP_HIP_FSYNC_EITHER };

constexpr std::uint64_t ccsds_asm = SDSP_HIP_FSYNC_CCSDS_ASM;

// what names a frame and its machine: a marker of marker_bits bits (bit marker_bits - 1 first on the line), payload_bytes bytes
// behind it, tol marker errors accepted, verify further markers before lock, flywheel misses ridden out in lock
struct sync_frame {
    std::uint64_t marker;
    std::uint32_t marker_bits, payload_bytes, tol, verify, flywheel;
    sync_polarity polarity;
    std::uint32_t period() const noexcept { return marker_bits + 8 * payload_bytes; }
};

// n bytes of the CCSDS pseudo-randomiser (FF 48 0E C0 ..)
inline std::vector<std::uint8_t> ccsds_pn(std::size_t n)
{
    std::vector<std::uint8_t> out(n);
    detail::check(sdsp_hip_fsync_ccsds_pn(out.data(), n));
    return out;
}

// ceil(nbits / L)
inline std::uint64_t fsync_max_frames(std::uint32_t marker_bits, std::uint32_t payload_bytes, std::uint64_t nbits)
{
    std::uint64_t v = 0;
    detail::check(sdsp_hip_fsync_max_frames(marker_bits, payload_bytes, nbits, &v));
    return v;
}

// the transmit side: frames of payload_bytes bytes -> the bit row (0 / 1 bytes): marker, payload XOR pn (empty: none), all inverted
// with `invert`
inline std::vector<std::uint8_t> attach_sync(std::uint64_t marker, std::uint32_t marker_bits, std::uint32_t payload_bytes,
                                             const std::vector<std::uint8_t> &frames, const std::vector<std::uint8_t> &pn = {},
                                             bool invert = false)
{
    const std::size_t n = payload_bytes ? frames.size() / payload_bytes : 0;
    std::vector<std::uint8_t> bits(n * (static_cast<std::size_t>(marker_bits) + 8u * payload_bytes));
    detail::check(sdsp_hip_fsync_attach(marker, marker_bits, payload_bytes, pn.empty() ? nullptr : pn.data(), frames.data(), n, invert ? 1 : 0,
                                        bits.data()));
    return bits;
}

struct sync_state {
    std::vector<std::uint32_t> mode, polarity, count, misses, pending;
    std::vector<std::uint64_t> next, seen;
};

template <typename in_t = std::uint8_t> class frame_sync_bank {
    static_assert(std::is_same<in_t, std::uint8_t>::value || std::is_same<in_t, std::uint32_t>::value,
                  "bits come as std::uint8_t (one per byte) or std::uint32_t (packed words)");

public:
    static constexpr int in_kind = std::is_same<in_t, std::uint32_t>::value ? SDSP_HIP_FSYNC_PACKED : SDSP_HIP_FSYNC_BYTES;

    // pn: empty, or payload_bytes bytes XORed onto every payload
    frame_sync_bank(const sync_frame &frame, std::uint64_t max_channels, std::uint64_t max_bits, const std::vector<std::uint8_t> &pn = {},
                    int device = 0)
        : m_frame(frame), m_device(device)
    {
        if (!pn.empty() && pn.size() != frame.payload_bytes)
            throw hip_error(SDSP_HIP_ERR_INVALID_ARG, "sdsp::frame_sync_bank: pn must hold payload_bytes bytes");
        sdsp_hip_fsync_plan *plan = nullptr;
        detail::check(sdsp_hip_fsync_plan_create(&plan, frame.marker, frame.marker_bits, frame.payload_bytes, frame.tol, frame.verify,
                                                 frame.flywheel, static_cast<int>(frame.polarity), pn.empty() ? nullptr : pn.data(), in_kind,
                                                 max_channels, max_bits, device));
        m_plan.reset(plan);
    }
    frame_sync_bank(const frame_sync_bank &) = delete;
    frame_sync_bank &operator=(const frame_sync_bank &) = delete;

    // device pointers: channels rows of nbits bits in; out (or null) channels x max_frames(nbits) x payload_bytes, counts one per
    // row, pos and info (or null) channels x max_frames(nbits); slots at and beyond counts[c] are not written; asynchronous on `stream`
    void process(const in_t *device_in, std::uint8_t *device_out, std::uint32_t *device_counts, std::uint64_t *device_pos,
                 std::uint32_t *device_info, std::uint64_t channels, std::uint64_t nbits, void *stream = nullptr)
    {
        detail::check(sdsp_hip_fsync_process(m_plan.get(), device_in, device_out, device_counts, device_pos, device_info, channels, nbits, stream));
    }
    // host pointers, the same shapes; what the outputs held at and beyond counts[c] stays
    void process_host(const in_t *host_in, std::uint8_t *host_out, std::uint32_t *host_counts, std::uint64_t *host_pos, std::uint32_t *host_info,
                      std::uint64_t channels, std::uint64_t nbits)
    {
        if (channels == 0)
            return;
        const std::size_t ch = static_cast<std::size_t>(channels), mf = static_cast<std::size_t>(max_frames(nbits));
        const std::size_t in_bytes = ch * static_cast<std::size_t>(in_kind == SDSP_HIP_FSYNC_PACKED ? nbits / 8 : nbits);
        const detail::stage_item items[] = { { in_bytes ? host_in : nullptr, nullptr, in_bytes },
                                             { mf ? host_out : nullptr, mf ? host_out : nullptr, ch * mf * m_frame.payload_bytes },
                                             { host_counts, host_counts, ch * sizeof(std::uint32_t) },
                                             { mf ? host_pos : nullptr, mf ? host_pos : nullptr, ch * mf * sizeof(std::uint64_t) },
                                             { mf ? host_info : nullptr, mf ? host_info : nullptr, ch * mf * sizeof(std::uint32_t) } };
        detail::host_stage(m_device, items, [&](void *const *dev) {
            return sdsp_hip_fsync_process(m_plan.get(), dev[0], static_cast<std::uint8_t *>(dev[1]), static_cast<std::uint32_t *>(dev[2]),
                                          static_cast<std::uint64_t *>(dev[3]), static_cast<std::uint32_t *>(dev[4]), channels, nbits, nullptr);
        });
    }
    // a fresh stream in every channel
    void reset() { detail::check(sdsp_hip_fsync_plan_reset(m_plan.get())); }
    // the machine of the first `channels` channels
    sync_state state(std::uint64_t channels) const
    {
        const std::size_t n = static_cast<std::size_t>(channels);
        sync_state s{ std::vector<std::uint32_t>(n), std::vector<std::uint32_t>(n), std::vector<std::uint32_t>(n), std::vector<std::uint32_t>(n),
                      std::vector<std::uint32_t>(n), std::vector<std::uint64_t>(n), std::vector<std::uint64_t>(n) };
        detail::check(sdsp_hip_fsync_plan_get_state(m_plan.get(), s.mode.data(), s.next.data(), s.polarity.data(), s.count.data(),
                                                    s.misses.data(), s.pending.data(), s.seen.data(), channels));
        return s;
    }
    // 0 = the staged kernels over a packed working row, 1 = the plain kernel
    void set_variant(int variant) { detail::check(sdsp_hip_fsync_plan_set_variant(m_plan.get(), variant)); }
    const sync_frame &frame() const noexcept { return m_frame; }
    std::uint64_t max_frames(std::uint64_t nbits) const noexcept { return (nbits + m_frame.period() - 1) / m_frame.period(); }
    std::uint64_t state_bytes() const
    {
        std::uint64_t v = 0;
        detail::check(sdsp_hip_fsync_plan_state_bytes(m_plan.get(), &v));
        return v;
    }
    std::uint64_t launches(std::uint64_t channels, std::uint64_t nbits) const
    {
        std::uint64_t v = 0;
        detail::check(sdsp_hip_fsync_plan_launches(m_plan.get(), channels, nbits, &v));
        return v;
    }
    sdsp_hip_fsync_plan_info info() const
    {
        sdsp_hip_fsync_plan_info i{};
        detail::check(sdsp_hip_fsync_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    sync_frame m_frame;
    int m_device;
    detail::plan_ptr<sdsp_hip_fsync_plan, sdsp_hip_fsync_plan_destroy> m_plan;
};
} // namespace sdsp

#endif // SDSP_MI355X_FSYNC_H
