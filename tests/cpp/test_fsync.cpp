// sdsp::frame_sync_bank (include/sdsp/fsync.h) on a few rows of framed bits -- junk in front, clean frames, a damaged marker, a slip of
// one bit, an inverted stretch -- in both kernel variants and both input kinds through the host entry, in one call and in three, against
// a direct synchroniser written here one bit at a time from the contract's paragraphs.  Everything is on integers, so the comparison is
// on bytes, records and the machine's state.
// Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/fsync.h>

#include <algorithm>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
using bytes = std::vector<std::uint8_t>;

struct record {
    std::uint64_t pos;
    std::uint32_t info;
    bytes body;
    bool operator==(const record &o) const { return pos == o.pos && info == o.info && body == o.body; }
};

// the whole row at once; frames whose last bit is not in the row stay pending
struct direct_sync {
    sdsp::sync_frame f;
    bytes pn;
    std::uint32_t mode = 0, pol = 0, count = 0, misses = 0, pending = 0;
    std::uint64_t p = 0;

    std::uint32_t distance(const bytes &bits, std::uint64_t at) const
    {
        std::uint32_t d = 0;
        for (std::uint32_t i = 0; i < f.marker_bits; i++)
            d += static_cast<std::uint32_t>((bits[at + i] != 0) != (((f.marker >> (f.marker_bits - 1 - i)) & 1u) != 0));
        return d;
    }
    void accept(const bytes &bits, std::uint64_t at, std::uint32_t fly, std::vector<record> &out)
    {
        const std::uint32_t M = f.marker_bits, L = f.period();
        if (at + L > bits.size()) {
            pending = 1;
            return;
        }
        const std::uint32_t d = distance(bits, at);
        record r{ at, (pol ? M - d : d) | (pol << 8) | (fly << 9), bytes(f.payload_bytes) };
        for (std::uint32_t i = 0; i < f.payload_bytes; i++) {
            std::uint32_t v = 0;
            for (std::uint32_t b = 0; b < 8; b++)
                v = 2 * v + (bits[at + M + 8 * i + b] != 0);
            if (pol)
                v ^= 0xffu;
            if (!pn.empty())
                v ^= pn[i];
            r.body[i] = static_cast<std::uint8_t>(v);
        }
        out.push_back(r);
    }
    std::vector<record> run(const bytes &bits)
    {
        const std::uint32_t M = f.marker_bits, L = f.period();
        std::vector<record> out;
        while (p + M <= bits.size()) {
            const std::uint32_t d = distance(bits, p);
            if (mode == 0) {
                const bool normal = d <= f.tol, inverted = f.polarity == sdsp::sync_polarity::either && M - d <= f.tol;
                if (!normal && !inverted) {
                    p += 1;
                    continue;
                }
                pol = normal ? 0 : 1;
                count = misses = 0;
                if (f.verify == 0) {
                    mode = 2;
                    accept(bits, p, 0, out);
                } else
                    mode = 1;
                p += L;
            } else if (mode == 1) {
                if ((pol ? M - d : d) <= f.tol) {
                    if (++count == f.verify) {
                        mode = 2;
                        accept(bits, p, 0, out);
                    }
                    p += L;
                } else {
                    mode = 0;
                    p = p - L + 1;
                }
            } else if ((pol ? M - d : d) <= f.tol) {
                misses = 0;
                accept(bits, p, 0, out);
                p += L;
            } else if (++misses > f.flywheel)
                mode = 0;
            else {
                accept(bits, p, 1, out);
                p += L;
            }
        }
        return out;
    }
};

std::vector<std::uint32_t> pack(const bytes &bits)
{
    std::vector<std::uint32_t> w(bits.size() / 32, 0);
    for (std::size_t i = 0; i < bits.size(); i++)
        w[i / 32] |= static_cast<std::uint32_t>(bits[i] != 0) << (i % 32);
    return w;
}

template <typename in_t>
int run_bank(const sdsp::sync_frame &f, const bytes &pn, const std::vector<bytes> &rows, const std::vector<std::vector<record>> &want,
             const std::vector<direct_sync> &machines, const std::vector<std::size_t> &edges, int first_variant, const char **kernel)
{
    const std::size_t ch = rows.size(), nbits = rows[0].size(), P = f.payload_bytes;
    const bool packed = std::is_same<in_t, std::uint32_t>::value;
    std::size_t longest = 0;
    for (std::size_t i = 0; i + 1 < edges.size(); i++)
        longest = std::max(longest, edges[i + 1] - edges[i]);
    sdsp::frame_sync_bank<in_t> bank(f, ch, longest, pn);
    std::vector<std::vector<record>> got(ch);
    int bad = 0;
    static sdsp_hip_fsync_plan_info info;
    for (std::size_t i = 0; i + 1 < edges.size(); i++) {
        const std::size_t a = edges[i], n = edges[i + 1] - a, mf = static_cast<std::size_t>(bank.max_frames(n));
        bank.set_variant((first_variant + static_cast<int>(i)) % 2);
        info = bank.info();
        *kernel = info.kernel;
        std::vector<in_t> in;
        for (std::size_t c = 0; c < ch; c++) {
            const bytes part(rows[c].begin() + static_cast<std::ptrdiff_t>(a), rows[c].begin() + static_cast<std::ptrdiff_t>(a + n));
            if (packed)
                for (std::uint32_t w : pack(part))
                    in.push_back(static_cast<in_t>(w));
            else
                for (std::uint8_t b : part)
                    in.push_back(static_cast<in_t>(b ? 1 + 37 * (c + 1) % 255 : 0)); // any non-zero byte is a one
        }
        bytes out(ch * mf * P, 0x55);
        std::vector<std::uint32_t> counts(ch, 77), inf(ch * mf, 0x55555555u);
        std::vector<std::uint64_t> pos(ch * mf, 0x5555555555555555ull);
        bank.process_host(in.data(), out.data(), counts.data(), pos.data(), inf.data(), ch, n);
        for (std::size_t c = 0; c < ch; c++) {
            if (counts[c] > mf) {
                bad++;
                continue;
            }
            for (std::size_t k = 0; k < mf; k++) {
                const std::size_t s = c * mf + k;
                if (k < counts[c])
                    got[c].push_back({ pos[s], inf[s], bytes(out.begin() + static_cast<std::ptrdiff_t>(s * P),
                                                             out.begin() + static_cast<std::ptrdiff_t>((s + 1) * P)) });
                else // slots at and beyond counts are not written
                    bad += pos[s] != 0x5555555555555555ull || inf[s] != 0x55555555u ||
                           !std::all_of(out.begin() + static_cast<std::ptrdiff_t>(s * P), out.begin() + static_cast<std::ptrdiff_t>((s + 1) * P),
                                        [](std::uint8_t v) { return v == 0x55; });
            }
        }
    }
    const sdsp::sync_state st = bank.state(ch);
    for (std::size_t c = 0; c < ch; c++) {
        const direct_sync &m = machines[c];
        bad += !(got[c] == want[c]);
        bad += st.mode[c] != m.mode || st.next[c] != m.p || st.polarity[c] != m.pol || st.count[c] != m.count || st.misses[c] != m.misses ||
               st.pending[c] != m.pending || st.seen[c] != nbits;
    }
    bad += bank.launches(ch, 64) != (info.variant == 1 ? 1u : 5u) || bank.launches(ch, 0) != 0;
    bad += bank.state_bytes() != ch * (16 + info.ring_words) * 4 || info.period != f.period();
    return bad;
}

int run(const sdsp::sync_frame &f, bool with_pn, unsigned seed)
{
    std::mt19937 rng(seed);
    const std::uint32_t M = f.marker_bits, P = f.payload_bytes, L = f.period();
    const bytes pn = with_pn ? sdsp::ccsds_pn(P) : bytes();
    const std::size_t ch = 3, frames = 12;
    std::vector<bytes> rows(ch);
    std::vector<std::vector<record>> want(ch);
    std::vector<direct_sync> machines;
    std::size_t emitted = 0;
    int bad = 0;
    for (std::size_t c = 0; c < ch; c++) {
        bytes payload(frames * P);
        for (auto &v : payload)
            v = static_cast<std::uint8_t>(rng());
        const bytes half(payload.begin(), payload.begin() + static_cast<std::ptrdiff_t>(8 * P));
        const bytes rest(payload.begin() + static_cast<std::ptrdiff_t>(8 * P), payload.end());
        bytes row(5 + 13 * c);
        for (auto &b : row)
            b = static_cast<std::uint8_t>(rng() & 1);
        const bytes upright = sdsp::attach_sync(f.marker, M, P, half, pn), inverted = sdsp::attach_sync(f.marker, M, P, rest, pn, true);
        row.insert(row.end(), upright.begin(), upright.end());
        row.insert(row.end(), inverted.begin(), inverted.end());
        const std::size_t start = 5 + 13 * c;
        row[start + 3 * L + 1] ^= 1; // a damaged marker
        row[start + 3 * L + 5] ^= 1;
        row.insert(row.begin() + static_cast<std::ptrdiff_t>(start + 6 * L), static_cast<std::uint8_t>(rng() & 1)); // a slip
        while (row.size() % 32 != 16)
            row.push_back(static_cast<std::uint8_t>(rng() & 1));
        row.resize(row.size() + 16, 0);
        rows[c] = row;
    }
    const std::size_t nbits = std::max({ rows[0].size(), rows[1].size(), rows[2].size() });
    for (std::size_t c = 0; c < ch; c++) {
        rows[c].resize(nbits, 0);
        direct_sync d{ f, pn };
        want[c] = d.run(rows[c]);
        machines.push_back(d);
        emitted += want[c].size();
        bad += sdsp::fsync_max_frames(M, P, nbits) < want[c].size();
    }
    const char *kernel = "";
    const std::vector<std::size_t> whole = { 0, nbits }, split = { 0, 32, 32, (nbits / 64) * 32, nbits }; // an empty call among them
    for (int variant : { 0, 1 }) {
        bad += run_bank<std::uint8_t>(f, pn, rows, want, machines, whole, variant, &kernel);
        bad += run_bank<std::uint32_t>(f, pn, rows, want, machines, whole, variant, &kernel);
        bad += run_bank<std::uint8_t>(f, pn, rows, want, machines, split, variant, &kernel);
        bad += run_bank<std::uint32_t>(f, pn, rows, want, machines, split, variant, &kernel);
    }
    const bool ok = bad == 0 && emitted >= ch * (frames - 5);
    std::printf("frame_sync_bank: marker %#llx / %u bits, %u bytes, tol %u, verify %u, flywheel %u, %zu rows of %zu bits, %zu frames, last kernel %s: %s\n",
                static_cast<unsigned long long>(f.marker), M, P, f.tol, f.verify, f.flywheel, ch, nbits, emitted, kernel,
                ok ? "bit for bit" : "MISMATCH");
    return ok ? 0 : 1;
}
} // namespace

int main()
{
    try {
        const bytes pn = sdsp::ccsds_pn(8);
        const std::uint8_t first[8] = { 0xFF, 0x48, 0x0E, 0xC0, 0x9A, 0x0D, 0x70, 0xBC };
        int rc = std::equal(pn.begin(), pn.end(), first) ? 0 : 1;
        rc |= run({ sdsp::ccsds_asm, 32, 10, 2, 1, 1, sdsp::sync_polarity::either }, true, 1);
        rc |= run({ 0xEB90, 16, 3, 0, 0, 0, sdsp::sync_polarity::either }, false, 2);
        rc |= run({ 0x034776C7272895B0ull, 64, 5, 3, 2, 2, sdsp::sync_polarity::either }, true, 3);
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &ex) {
        std::printf("no usable device: %s\n", ex.what());
        return 3;
    }
}
