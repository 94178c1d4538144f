// AddressSanitizer / UBSan build of the functions the setup kernels share with the host (csrc/h2r_setup.hpp): the header
// itself is compiled instrumented into this stand-alone program, and the window bases, the table entries, the digit walk over an exact-size
// heap table, the scalar families and the G2 multiplication run on inputs whose answers follow from the group law alone.  No device work
// and no library: host code only.
//   hipcc --cuda-host-only -x hip -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Ihalo2_rsa_amd/csrc
//         tests/cpp/test_setup_shared.cpp -o test_setup_shared
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "h2r_setup.hpp"
#include "h2r_curve_ntt.hpp"

using namespace h2r;

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

template <typename T> static std::unique_ptr<T[]> heap(size_t n) { return std::unique_ptr<T[]>(new T[n]()); }

static bool aff_eq(const PtAff &a, const PtAff &b) { return fe_eq(a.x, b.x) && fe_eq(a.y, b.y); }
// [k]P by the curve transform's 2-bit windows: a second route that shares no table with the walk
static PtAff mul_ref(const PtAff &p, const uint64_t (&k)[4], const CurveConsts &cv) { return pt_to_affine(pt_mul_window2(pt_from_affine(p, cv), k, cv), cv); }

// the order r of the group (the modulus of bn254_fr)
static const uint64_t kR[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};

static int run_g1(const CurveConsts &cv) {
    PtAff g; g.x = fe_to_mont(fe_small(1), cv.fq); g.y = fe_to_mont(fe_small(2), cv.fq);
    REQUIRE(pt_aff_on_curve(g, cv));
    PtAff off = g; off.y = fe_to_mont(fe_small(3), cv.fq);
    REQUIRE(!pt_aff_on_curve(off, cv));
    PtAff ident; ident.x = fe_zero(); ident.y = fe_zero();
    REQUIRE(pt_aff_on_curve(ident, cv));
    // the table of G on the heap, exactly FB_TABLE_BYTES / 64 entries
    auto wb = heap<PtAff>(FB_WINDOWS);
    fb_window_bases(g, wb.get(), cv);
    auto table = heap<PtAff>(FB_WINDOWS * FB_DIGITS);
    for (uint32_t w = 0; w < FB_WINDOWS; ++w)
        for (uint32_t d = 0; d < FB_DIGITS; ++d) table[w * FB_DIGITS + d] = fb_table_entry(wb[w], d, cv);
    REQUIRE(aff_eq(table[1], g) && pt_aff_is_identity(table[0]) && pt_aff_is_identity(table[5 * FB_DIGITS]));
    {   // T[w][d] = [d 256^w]G by the other route
        const uint32_t ws[4] = {0, 1, 8, 31}, ds[4] = {1, 2, 128, 255};
        for (uint32_t w : ws) for (uint32_t d : ds) {
            uint64_t k[4] = {0, 0, 0, 0};
            k[w / 8] = (uint64_t)d << (8 * (w % 8));
            REQUIRE(aff_eq(table[w * FB_DIGITS + d], mul_ref(g, k, cv)));
        }
    }
    auto entry = [&](uint32_t w, uint32_t d) { return table[w * FB_DIGITS + d]; };
    const uint64_t ks[][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {255, 0, 0, 0}, {256, 0, 0, 0}, {~0ull, ~0ull, ~0ull, ~0ull}, {kR[0] - 1, kR[1], kR[2], kR[3]},
                              {kR[0], kR[1], kR[2], kR[3]}, {kR[0] + 1, kR[1], kR[2], kR[3]}, {0xff00ff00ff00ff00ull, 0xff00ff00ff00ff00ull, 0xff00ff00ff00ff00ull, 0xff00ff00ff00ff00ull},
                              {0x0123456789abcdefull, 0xfedcba9876543210ull, 0x0f1e2d3c4b5a6978ull, 0x8000000000000001ull}};
    for (const auto &k : ks) {
        const PtAff got = pt_to_affine(fb_walk(fe_words(k), entry, cv), cv);
        REQUIRE(aff_eq(got, mul_ref(g, k, cv)));
    }
    REQUIRE(pt_aff_is_identity(pt_to_affine(fb_walk(fe_words(kR), entry, cv), cv)));
    // the identity's table: every entry (0, 0), every product the identity
    fb_window_bases(ident, wb.get(), cv);
    for (uint32_t w = 0; w < FB_WINDOWS; ++w) REQUIRE(pt_aff_is_identity(wb[w]) && pt_aff_is_identity(fb_table_entry(wb[w], 255, cv)));
    return 0;
}

static int run_scalars() {
    FieldConsts fr;
    field_consts_init(kR, &fr);
    const Fe one = fe_load_one(fr), tau = fe_to_mont(fe_small(0x1234567), fr);
    auto pw = heap<Fe>(SETUP_MAX_LOG);
    Fe b = tau;
    for (uint32_t i = 0; i < SETUP_MAX_LOG; ++i) { pw[i] = b; b = fe_mont_mul(b, b, fr); }
    Fe acc = one;
    for (uint32_t i = 0; i < 300; ++i) { REQUIRE(fe_eq(setup_chain_power(i, pw.get(), fr), acc)); acc = fe_mont_mul(acc, tau, fr); }
    REQUIRE(fe_eq(setup_chain_power((1u << 24) - 1, pw.get(), fr), fe_mont_mul(fe_mont_mul(pw[23], pw[23], fr), fe_to_mont(fe_inv(fe_from_mont(tau, fr), fr), fr), fr)));
    // n = 2, omega = -1: l_0 = (tau + 1) / 2, l_1 = (1 - tau) / 2, and they sum to one
    const Fe m1 = fe_sub(fe_zero(), one, fr.p), t2 = fe_mont_mul(tau, tau, fr);
    const Fe c = fe_mont_mul(fe_sub(t2, one, fr.p), fe_to_mont(fe_inv(fe_small(2), fr), fr), fr);
    const Fe l0 = setup_lagrange_value(one, tau, c, fr), l1 = setup_lagrange_value(m1, tau, c, fr);
    REQUIRE(fe_eq(fe_add(l0, l1, fr.p), one));
    REQUIRE(fe_eq(fe_add(l0, l0, fr.p), fe_add(tau, one, fr.p)));
    return 0;
}

static int run_g2(const CurveConsts &cv, uint32_t mont) {
    PairingConsts c;
    pairing_consts_init(cv, mont, &c);
    auto g2 = heap<uint8_t>(PR_G2_BYTES);
    auto out = heap<uint8_t>(PR_G2_BYTES);
    g2_generator(g2.get(), c);
    G2Aff q;
    REQUIRE(g2_load(g2.get(), &q, c) == 0 && !q.inf);
    const uint64_t k5[4] = {5, 0, 0, 0}, k3[4] = {3, 0, 0, 0}, k2[4] = {2, 0, 0, 0}, k0[4] = {0, 0, 0, 0};
    const uint64_t rm1[4] = {kR[0] - 1, kR[1], kR[2], kR[3]}, all[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    const G2Aff p5 = g2_mul(q, k5, c.fq), p3 = g2_mul(q, k3, c.fq), p2 = g2_mul(q, k2, c.fq);
    const G2Aff s = g2_add(p3, p2, c.fq);
    REQUIRE(!p5.inf && fq2_eq(s.x, p5.x) && fq2_eq(s.y, p5.y));
    const G2Aff d = g2_double(q, c.fq);
    REQUIRE(fq2_eq(d.x, p2.x) && fq2_eq(d.y, p2.y));
    REQUIRE(g2_mul(q, kR, c.fq).inf && g2_mul(q, k0, c.fq).inf && g2_mul(g2_identity(), k5, c.fq).inf);
    const G2Aff neg = g2_mul(q, rm1, c.fq);
    REQUIRE(fq2_eq(neg.x, q.x) && fq2_eq(neg.y, fq2_neg(q.y, c.fq)) && g2_add(neg, q, c.fq).inf);
    // every result is on the twist and round-trips through the 128 bytes
    for (const G2Aff &p : {p5, neg, g2_mul(q, all, c.fq)}) {
        g2_store(out.get(), p, c);
        G2Aff back;
        REQUIRE(g2_load(out.get(), &back, c) == 0 && !back.inf && fq2_eq(back.x, p.x) && fq2_eq(back.y, p.y));
    }
    g2_store(out.get(), g2_identity(), c);
    for (uint32_t i = 0; i < PR_G2_BYTES; ++i) REQUIRE(out[i] == 0);
    G2Aff back;
    REQUIRE(g2_load(out.get(), &back, c) == 0 && back.inf);
    // the refusals: a coordinate = q, a point off E'
    std::memcpy(out.get(), g2.get(), PR_G2_BYTES);
    std::memcpy(out.get() + 96, c.fq.p, 32);
    REQUIRE(g2_load(out.get(), &back, c) == (uint32_t)H2R_E_SHAPE);
    std::memcpy(out.get() + 96, g2.get(), 32);
    REQUIRE(g2_load(out.get(), &back, c) == (uint32_t)H2R_E_ASSERTION);
    return 0;
}

int main() {
    const CurveConsts *cv = curve_of_field(0);
    if (!cv) return 1;
    if (run_g1(*cv) || run_scalars()) return 1;
    for (uint32_t mont = 0; mont < 2; ++mont)
        if (run_g2(*cv, mont)) return 1;
    std::printf("SETUP_SHARED_OK 2 representations\n");
    return 0;
}
