// sdsp::rs_decoder (include/sdsp/rs.h) on a few frames of RS(255, 223) at I = 5 (CCSDS, full frames out, erasure flags) and of the
// shortened RS(204, 188) (DVB, data out, no flags), in both kernel variants through the host entry, against a direct serial decoder
// written here on other lines than the library's: field products by shift and reduce, the error locator from the modified syndromes by
// Gaussian elimination (Peterson-Gorenstein-Zierler), the error values from the syndrome equations by Gaussian elimination, and then the
// contract itself -- zero syndromes, 2 errors + erasures <= nroots.  Everything is on integers, so the comparison is on bytes.
// Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/rs.h>

#include <algorithm>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
using bytes = std::vector<std::uint8_t>;

struct field {
    std::uint32_t poly;
    std::uint8_t mul(std::uint8_t a, std::uint8_t b) const
    {
        std::uint32_t r = 0, x = a;
        for (int i = 0; i < 8; i++) {
            if ((b >> i) & 1)
                r ^= x;
            x <<= 1;
            if (x & 0x100)
                x ^= poly;
        }
        return static_cast<std::uint8_t>(r);
    }
    std::uint8_t pow(std::uint8_t a, std::uint32_t e) const
    {
        std::uint8_t r = 1;
        for (; e; e >>= 1, a = mul(a, a))
            if (e & 1)
                r = mul(r, a);
        return r;
    }
    std::uint8_t inv(std::uint8_t a) const { return pow(a, 254); }
};

// A x = b over the field, A square; false where A is singular
bool solve(const field &f, std::vector<bytes> a, bytes b, bytes &x)
{
    const std::size_t m = b.size();
    for (std::size_t col = 0; col < m; col++) {
        std::size_t piv = col;
        while (piv < m && a[piv][col] == 0)
            piv++;
        if (piv == m)
            return false;
        std::swap(a[piv], a[col]);
        std::swap(b[piv], b[col]);
        const std::uint8_t s = f.inv(a[col][col]);
        for (std::size_t j = 0; j < m; j++)
            a[col][j] = f.mul(a[col][j], s);
        b[col] = f.mul(b[col], s);
        for (std::size_t row = 0; row < m; row++) {
            const std::uint8_t q = a[row][col];
            if (row == col || q == 0)
                continue;
            for (std::size_t j = 0; j < m; j++)
                a[row][j] = static_cast<std::uint8_t>(a[row][j] ^ f.mul(q, a[col][j]));
            b[row] = static_cast<std::uint8_t>(b[row] ^ f.mul(q, b[col]));
        }
    }
    x = b;
    return true;
}

struct direct_decoder {
    sdsp::rs_code c;
    field f;
    explicit direct_decoder(const sdsp::rs_code &code) : c(code), f{ code.field_poly } {}

    std::uint8_t locator(std::size_t i) const { return f.pow(2, (c.prim * static_cast<std::uint32_t>(c.n - 1 - i)) % 255); } // X_i
    bytes syndromes(const bytes &r) const
    {
        bytes s(c.nroots, 0);
        for (std::uint32_t j = 0; j < c.nroots; j++)
            for (std::size_t i = 0; i < c.n; i++)
                s[j] = static_cast<std::uint8_t>(s[j] ^ f.mul(r[i], f.pow(locator(i), c.fcr + j)));
        return s;
    }
    // the word in place; returns the count of symbols changed or -1
    int decode(bytes &r, const bytes &erased) const
    {
        const std::uint32_t nroots = c.nroots;
        std::vector<std::size_t> E;
        for (std::size_t i = 0; i < c.n; i++)
            if (erased[i])
                E.push_back(i);
        const std::uint32_t ne = static_cast<std::uint32_t>(E.size());
        if (ne > nroots)
            return -1;
        const bytes s = syndromes(r);
        if (std::all_of(s.begin(), s.end(), [](std::uint8_t v) { return v == 0; }))
            return 0;
        bytes gam{ 1 }; // the erasure locator
        for (std::size_t e : E) {
            gam.push_back(0);
            for (std::size_t k = gam.size() - 1; k >= 1; k--)
                gam[k] = static_cast<std::uint8_t>(gam[k] ^ f.mul(locator(e), gam[k - 1]));
        }
        bytes t(nroots, 0); // the modified syndromes, meaningful from index ne on
        for (std::uint32_t m = ne; m < nroots; m++)
            for (std::uint32_t k = 0; k <= ne; k++)
                t[m] = static_cast<std::uint8_t>(t[m] ^ f.mul(gam[k], s[m - k]));
        bytes sigma{ 1 };
        for (std::uint32_t v = (nroots - ne) / 2; v >= 1; v--) {
            std::vector<bytes> a(v, bytes(v));
            bytes b(v), x;
            for (std::uint32_t i = 0; i < v; i++) {
                b[i] = t[ne + v + i];
                for (std::uint32_t j = 1; j <= v; j++)
                    a[i][j - 1] = t[ne + v + i - j];
            }
            if (solve(f, a, b, x)) {
                sigma.insert(sigma.end(), x.begin(), x.end());
                break;
            }
        }
        bytes psi(sigma.size() + gam.size() - 1, 0); // the whole locator
        for (std::size_t i = 0; i < sigma.size(); i++)
            for (std::size_t j = 0; j < gam.size(); j++)
                psi[i + j] = static_cast<std::uint8_t>(psi[i + j] ^ f.mul(sigma[i], gam[j]));
        while (psi.size() > 1 && psi.back() == 0)
            psi.pop_back();
        std::vector<std::size_t> P;
        for (std::size_t i = 0; i < c.n; i++) {
            const std::uint8_t z = f.inv(locator(i));
            std::uint8_t v = 0;
            for (std::size_t k = psi.size(); k-- > 0;)
                v = static_cast<std::uint8_t>(f.mul(v, z) ^ psi[k]);
            if (v == 0)
                P.push_back(i);
        }
        if (P.empty() || P.size() != psi.size() - 1 || P.size() > nroots)
            return -1;
        std::vector<bytes> a(P.size(), bytes(P.size()));
        bytes b(P.size()), y;
        for (std::size_t j = 0; j < P.size(); j++) {
            b[j] = s[j];
            for (std::size_t l = 0; l < P.size(); l++)
                a[j][l] = f.pow(locator(P[l]), c.fcr + static_cast<std::uint32_t>(j));
        }
        if (!solve(f, a, b, y))
            return -1;
        bytes out = r;
        std::uint32_t changed = 0, outside = 0;
        for (std::size_t l = 0; l < P.size(); l++) {
            out[P[l]] = static_cast<std::uint8_t>(out[P[l]] ^ y[l]);
            changed += y[l] != 0;
            outside += y[l] != 0 && !erased[P[l]];
        }
        const bytes s2 = syndromes(out);
        if (!std::all_of(s2.begin(), s2.end(), [](std::uint8_t v) { return v == 0; }) || 2 * outside + ne > nroots)
            return -1;
        r = out;
        return static_cast<int>(changed);
    }
};

int run(const sdsp::rs_code &code, std::uint32_t I, sdsp::rs_output output, bool with_flags, std::uint64_t frames, unsigned seed)
{
    std::mt19937 rng(seed);
    const std::uint32_t n = code.n, k = code.n - code.nroots, t = code.nroots / 2;
    const direct_decoder direct(code);
    bytes data(frames * I * k);
    for (auto &v : data)
        v = static_cast<std::uint8_t>(rng());
    const bytes sent = sdsp::rs_encode(code, I, data);
    int bad = 0;
    {   // the encoder's output is the data followed by parity that makes every syndrome zero
        bytes w(n);
        for (std::uint32_t s = 0; s < n; s++)
            w[s] = sent[s * I];
        const bytes s0 = direct.syndromes(w);
        bad += !std::all_of(s0.begin(), s0.end(), [](std::uint8_t v) { return v == 0; });
        bad += !std::equal(data.begin(), data.begin() + I * k, sent.begin());
        bad += sdsp::rs_generator(code).size() != code.nroots + 1 || sdsp::rs_generator(code)[0] != 1;
    }
    bytes recv = sent, flags(sent.size(), 0);
    std::vector<std::int32_t> want_cnt(frames * I);
    bytes want = sent;
    int good = 0, failed = 0;
    for (std::uint64_t fr = 0; fr < frames; fr++)
        for (std::uint32_t j = 0; j < I; j++) {
            const std::size_t base = fr * I * n + j;
            const unsigned kind = static_cast<unsigned>(fr * I + j) % 5; // clean, a few errors, t errors, t + 1 errors, errors and erasures
            const std::uint32_t few = 1 + static_cast<std::uint32_t>(rng() % 3);
            const std::uint32_t errors = kind == 0 ? 0 : kind == 1 ? few : kind == 2 ? t : kind == 3 ? t + 1 : t / 2;
            const std::uint32_t erasures = kind == 4 && with_flags ? code.nroots - 2 * (t / 2) : 0;
            std::vector<std::uint32_t> pos(n);
            for (std::uint32_t s = 0; s < n; s++)
                pos[s] = s;
            std::shuffle(pos.begin(), pos.end(), rng);
            for (std::uint32_t e = 0; e < errors + erasures; e++) {
                recv[base + pos[e] * I] = static_cast<std::uint8_t>(recv[base + pos[e] * I] ^ (1 + rng() % 255));
                if (e >= errors)
                    flags[base + pos[e] * I] = static_cast<std::uint8_t>(1 + rng() % 255);
            }
            bytes w(n), fl(n);
            for (std::uint32_t s = 0; s < n; s++) {
                w[s] = recv[base + s * I];
                fl[s] = flags[base + s * I];
            }
            const int cnt = direct.decode(w, fl);
            want_cnt[fr * I + j] = cnt;
            for (std::uint32_t s = 0; s < n; s++)
                want[base + s * I] = w[s];
            good += cnt > 0;
            failed += cnt < 0;
        }
    sdsp::rs_decoder dec(code, I, output);
    const std::size_t ob = dec.out_bytes(), fb = dec.frame_bytes();
    sdsp_hip_rs_plan_info info{};
    for (int variant : { 0, 1 }) {
        dec.set_variant(variant);
        info = dec.info();
        bytes out(frames * ob, 0x55);
        std::vector<std::int32_t> cnt(frames * I, 77);
        dec.process_host(recv.data(), with_flags ? flags.data() : nullptr, out.data(), cnt.data(), frames);
        for (std::uint64_t fr = 0; fr < frames; fr++)
            bad += !std::equal(out.begin() + static_cast<std::ptrdiff_t>(fr * ob), out.begin() + static_cast<std::ptrdiff_t>((fr + 1) * ob),
                               want.begin() + static_cast<std::ptrdiff_t>(fr * fb));
        bad += cnt != want_cnt;
        bad += dec.launches(frames) != 1 || info.variant != variant || info.k != k || info.t != t;
    }
    const bool ok = bad == 0 && good > 0 && failed > 0;
    std::printf("rs_decoder: (%#x, %u, %u, %u, %u) I = %u, %s, %llu frames, %d corrected, %d beyond the code, kernel %s, lds %u: %s\n",
                code.field_poly, code.fcr, code.prim, code.nroots, code.n, I, output == sdsp::rs_output::data ? "data" : "full",
                static_cast<unsigned long long>(frames), good, failed, info.kernel, info.lds_bytes, ok ? "byte for byte" : "MISMATCH");
    return ok ? 0 : 1;
}
} // namespace

int main()
{
    try {
        int rc = run({ 0x187, 112, 11, 32, 255 }, 5, sdsp::rs_output::full, true, 3, 1);
        rc |= run({ 0x11D, 0, 1, 16, 204 }, 1, sdsp::rs_output::data, false, 11, 2);
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &ex) {
        std::printf("no usable device: %s\n", ex.what());
        return 3;
    }
}
