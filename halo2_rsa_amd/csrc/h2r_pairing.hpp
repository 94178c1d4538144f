// The optimal ate pairing check over bn256 for the verifier's verdict: Fq2 = Fq[i] / (i^2 + 1), xi = 9 + i,
// Fq12 = Fq2[w] / (w^6 - xi) as six Fq2 coefficients, G2 on the twist E': y^2 = x^3 + 3 / xi as KEY MATERIAL (a table of 102 line
// coefficients per fixed point, made once on the host: no G2 arithmetic runs per proof), the Miller loop over 6 u + 2 and the EXACT
// final exponentiation f^((q^12 - 1) / r).  A restatement held to the Python model tests/pairing_ref.py; byte parity with halo2curves'
// Gt is not claimed.  Host and device share every formula (H2R_FD): h2r_pairing_eval runs on the host exactly what the kernel inlines.
//
// An Fq12 value is 96 dwords: a product held in one lane's registers spills.  So a circuit is served by a TEAM: `each(d, fn)` forms
// coefficient k of a value by fn(k) and stores it to slot d of the team's store.  On the host a team is a loop over k and an array
// (PrHostTeam); on the device it is PR_TEAM = 8 adjacent lanes of one wavefront -- lanes 0..5 own a coefficient, lanes 6 and 7 repeat
// the work of 0 and 1 and store nothing -- over PR_SLOTS values in LDS (PrLaneTeam: fn, barrier, store, barrier, so a destination may
// be an operand).  Coefficient k of a product is c_k = sum_{i+j=k} a_i b_j + xi sum_{i+j=k+6} a_i b_j: six Fq2 products by Karatsuba
// (a square: the unordered pairs once, four); a line y_P + (-lambda x_P) w + c w^3 has three nonzero operands.  Both walks are sequences of team operations whose order is fixed
// by compile-time constants (the bits of 6 u + 2 and of u, the program of the final exponentiation): no trip count and no branch
// around a barrier depends on the data; only fe_inv's loop does, inside one lane.
// Elements are in the Montgomery form of Fq inside; memory holds the ctx's representation, canonical representatives.
#pragma once

#include <cstring>

#include "h2r.h"
#include "h2r_curve.hpp"

namespace h2r {

#if defined(__HIP_DEVICE_COMPILE__)
#define H2R_PR_ROLLED _Pragma("unroll 1")
#else
#define H2R_PR_ROLLED
#endif

constexpr uint32_t PR_STEPS = 102, PR_STEP_BYTES = 128, PR_TABLE_BYTES = PR_STEPS * PR_STEP_BYTES, PR_MAX_PAIRS = 4;
constexpr uint32_t PR_FQ12_BYTES = 384, PR_G2_BYTES = 128, PR_G1_BYTES = 64;
constexpr uint32_t PR_SLOTS = 10;                         // Fq12 values of a team's store (the final exponentiation's program uses all)
constexpr uint32_t PR_TEAM = 8, PR_LANES = 64, PR_TEAMS = PR_LANES / PR_TEAM;   // lanes of a team; of a workgroup (ONE wavefront); circuits of a workgroup
constexpr uint32_t PR_TEAM_FQ2 = PR_SLOTS * 6 + PR_MAX_PAIRS;                     // a team's store: the slots, then the G1 operands (x, y) of its circuit
constexpr uint64_t PR_U = 4965661367192848881ull;         // bn256's u: q = 36 u^4 + 36 u^3 + 24 u^2 + 6 u + 1 (63 bits, 28 set)
constexpr uint64_t PR_LOOP_LO = 11347224129447541672ull;  // 6 u + 2 = 2^64 + this: the 64 bits below the top bit (36 set)
// the generator of G2 (EIP-197's; tests/pairing_ref.G2): x.re, x.im, y.re, y.im as canonical integers, four little-endian words each
constexpr uint64_t PR_G2_GENERATOR[4][4] = {{0x46debd5cd992f6edull, 0x674322d4f75edaddull, 0x426a00665e5c4479ull, 0x1800deef121f1e76ull},
                                            {0x97e485b7aef312c2ull, 0xf1aa493335a9e712ull, 0x7260bfb731fb5d25ull, 0x198e9393920d483aull},
                                            {0x4ce6cc0166fa7daaull, 0xe3d1e7690c43d37bull, 0x4aab71808dcb408full, 0x12c85ea5db8c6debull},
                                            {0x55acdadcd122975bull, 0xbc4b313370b38ef3ull, 0xec9e99ad690c3395ull, 0x090689d0585ff075ull}};

struct Fq2 { Fe re, im; };

H2R_FD Fq2 fq2_zero() { Fq2 r; r.re = fe_zero(); r.im = fe_zero(); return r; }
H2R_FD bool fq2_is_zero(const Fq2 &a) { return fe_is_zero(a.re) && fe_is_zero(a.im); }
H2R_FD bool fq2_eq(const Fq2 &a, const Fq2 &b) { return fe_eq(a.re, b.re) && fe_eq(a.im, b.im); }
H2R_FD Fq2 fq2_add(const Fq2 &a, const Fq2 &b, const FieldConsts &f) { Fq2 r; r.re = fe_add(a.re, b.re, f.p); r.im = fe_add(a.im, b.im, f.p); return r; }
H2R_FD Fq2 fq2_sub(const Fq2 &a, const Fq2 &b, const FieldConsts &f) { Fq2 r; r.re = fe_sub(a.re, b.re, f.p); r.im = fe_sub(a.im, b.im, f.p); return r; }
H2R_FD Fq2 fq2_neg(const Fq2 &a, const FieldConsts &f) { return fq2_sub(fq2_zero(), a, f); }
H2R_FD Fq2 fq2_conj(const Fq2 &a, const FieldConsts &f) { Fq2 r; r.re = a.re; r.im = fe_sub(fe_zero(), a.im, f.p); return r; }
// Karatsuba: three products
H2R_FD Fq2 fq2_mul(const Fq2 &a, const Fq2 &b, const FieldConsts &f) {
    const Fe t0 = fe_mont_mul(a.re, b.re, f), t1 = fe_mont_mul(a.im, b.im, f);
    const Fe t2 = fe_mont_mul(fe_add(a.re, a.im, f.p), fe_add(b.re, b.im, f.p), f);
    Fq2 r; r.re = fe_sub(t0, t1, f.p); r.im = fe_sub(fe_sub(t2, t0, f.p), t1, f.p);
    return r;
}
// (re + im)(re - im) + 2 re im i: two products
H2R_FD Fq2 fq2_square(const Fq2 &a, const FieldConsts &f) {
    const Fe t = fe_mont_mul(a.re, a.im, f);
    Fq2 r; r.re = fe_mont_mul(fe_add(a.re, a.im, f.p), fe_sub(a.re, a.im, f.p), f); r.im = fe_add(t, t, f.p);
    return r;
}
H2R_FD Fq2 fq2_mul_fe(const Fq2 &a, const Fe &s, const FieldConsts &f) { Fq2 r; r.re = fe_mont_mul(a.re, s, f); r.im = fe_mont_mul(a.im, s, f); return r; }
// (9 + i)(re + im i) = (9 re - im) + (re + 9 im) i, the 9 by doublings
H2R_FD Fq2 fq2_mul_xi(const Fq2 &a, const FieldConsts &f) {
    auto nine = [&](const Fe &x) __attribute__((always_inline)) { Fe t = fe_add(x, x, f.p); t = fe_add(t, t, f.p); t = fe_add(t, t, f.p); return fe_add(t, x, f.p); };
    Fq2 r; r.re = fe_sub(nine(a.re), a.im, f.p); r.im = fe_add(a.re, nine(a.im), f.p);
    return r;
}
// conj(a) / (re^2 + im^2): ONE fe_inv.  a = 0 has no inverse (fe_inv's garbage, no hang)
H2R_FD Fq2 fq2_inv(const Fq2 &a, const FieldConsts &f) {
    const Fe n = fe_add(fe_mont_mul(a.re, a.re, f), fe_mont_mul(a.im, a.im, f), f.p);
    const Fe ni = fe_to_mont(fe_inv(fe_from_mont(n, f), f), f);
    Fq2 r; r.re = fe_mont_mul(a.re, ni, f); r.im = fe_sub(fe_zero(), fe_mont_mul(a.im, ni, f), f.p);
    return r;
}

// the Frobenius constants gamma_k[j] = xi^(j (q^k - 1) / 6) for k = 1, 2, 3, the two curves' b, the representation: made once on the host
struct PairingConsts {
    FieldConsts fq;
    Fq2 g[3][6];
    Fq2 b2;             // 3 / xi: the twist's b
    Fe b;               // 3: the curve's b
    uint32_t mont, pad_;
};

// 32 bytes of host or device memory <-> an element in Montgomery form (device: two 16-byte accesses, as fe_load / fe_store)
H2R_FD Fe pr_ld_raw(const uint8_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return fe_load(p);
#else
    Fe r; std::memcpy(r.v, p, 32); return r;
#endif
}
H2R_FD Fe pr_ld(const uint8_t *p, const PairingConsts &c) { const Fe r = pr_ld_raw(p); return c.mont ? r : fe_to_mont(r, c.fq); }
H2R_FD void pr_st(uint8_t *p, const Fe &x, const PairingConsts &c) {
    const Fe r = c.mont ? x : fe_from_mont(x, c.fq);
#if defined(__HIP_DEVICE_COMPILE__)
    fe_store(p, r);
#else
    std::memcpy(p, r.v, 32);
#endif
}
H2R_FD Fq2 pr_ld2(const uint8_t *p, const PairingConsts &c) { Fq2 r; r.re = pr_ld(p, c); r.im = pr_ld(p + 32, c); return r; }
H2R_FD void pr_st2(uint8_t *p, const Fq2 &x, const PairingConsts &c) { pr_st(p, x.re, c); pr_st(p + 32, x.im, c); }
// n x 32 bytes hold canonical representatives
H2R_FD bool pr_in_range(const uint8_t *p, uint32_t n, const PairingConsts &c) {
    bool ok = true;
    H2R_PR_ROLLED
    for (uint32_t i = 0; i < n; ++i) { const Fe r = pr_ld_raw(p + (uint64_t)i * 32); if (ge_p(r.v, c.fq.p)) ok = false; }
    return ok;
}

// ---- Fq12, coefficient by coefficient ---------------------------------------------------------------------------------------------------
// coefficient k of a b
H2R_FD Fq2 fq12_mul_coeff(const Fq2 *a, const Fq2 *b, uint32_t k, const FieldConsts &f) {
    Fq2 lo = fq2_zero(), hi = fq2_zero();
    H2R_PR_ROLLED
    for (uint32_t i = 0; i < 6; ++i) {
        const bool wrap = i > k;
        const Fq2 p = fq2_mul(a[i], b[wrap ? k + 6 - i : k - i], f), z = fq2_zero();
        lo = fq2_add(lo, wrap ? z : p, f); hi = fq2_add(hi, wrap ? p : z, f);
    }
    return fq2_add(lo, fq2_mul_xi(hi, f), f);
}
// coefficient k of a^2: the unordered pairs {i, j} of i + j = k or k + 6 once each -- i = s, j = k - s for s <= k / 2, then i = k + 1 + t,
// j = 5 - t while i <= j -- doubled where i != j: four Fq2 products for an even k, three for an odd one (its fourth slot adds zero), not six
H2R_FD Fq2 fq12_square_coeff(const Fq2 *a, uint32_t k, const FieldConsts &f) {
    Fq2 lo = fq2_zero(), hi = fq2_zero();
    const uint32_t n_lo = k / 2 + 1;
    H2R_PR_ROLLED
    for (uint32_t s = 0; s < 4; ++s) {
        const bool wrap = s >= n_lo;
        uint32_t i = wrap ? k + 1 + (s - n_lo) : s, j = wrap ? 5 - (s - n_lo) : k - s;
        const bool valid = i <= j;
        if (!valid) { i = 0; j = 0; }
        Fq2 p = fq2_mul(a[i], a[j], f);
        const Fq2 z = fq2_zero();
        p = valid ? (i != j ? fq2_add(p, p, f) : p) : z;
        lo = fq2_add(lo, wrap ? z : p, f); hi = fq2_add(hi, wrap ? p : z, f);
    }
    return fq2_add(lo, fq2_mul_xi(hi, f), f);
}
// coefficient k of a product whose operands may be one value
H2R_FD Fq2 fq12_product_coeff(const Fq2 *a, const Fq2 *b, uint32_t k, const FieldConsts &f) { return a == b ? fq12_square_coeff(a, k, f) : fq12_mul_coeff(a, b, k, f); }
// a line l0 + l1 w + l3 w^3 with l0 in Fq, and coefficient k of a * line
struct PrLine { Fe l0; Fq2 l1, l3; };
H2R_FD Fq2 fq12_mul_line_coeff(const Fq2 *a, const PrLine &l, uint32_t k, const FieldConsts &f) {
    Fq2 r = fq2_mul_fe(a[k], l.l0, f);
    Fq2 t = fq2_mul(a[k >= 1 ? k - 1 : k + 5], l.l1, f);
    r = fq2_add(r, k >= 1 ? t : fq2_mul_xi(t, f), f);
    t = fq2_mul(a[k >= 3 ? k - 3 : k + 3], l.l3, f);
    return fq2_add(r, k >= 3 ? t : fq2_mul_xi(t, f), f);
}
// coefficient j of pi^k(a), k = 1, 2, 3: conj^k(a_j) gamma_k[j]
H2R_FD Fq2 fq12_frob_coeff(const Fq2 *a, uint32_t k, uint32_t j, const PairingConsts &c) {
    const Fq2 x = (k & 1u) ? fq2_conj(a[j], c.fq) : a[j];
    return fq2_mul(x, c.g[k - 1][j], c.fq);
}
// coefficient j of a^(q^6): w -> -w
H2R_FD Fq2 fq12_conj_coeff(const Fq2 *a, uint32_t j, const FieldConsts &f) { return (j & 1u) ? fq2_neg(a[j], f) : a[j]; }
H2R_FD Fq2 fq12_one_coeff(uint32_t j, const FieldConsts &f) { Fq2 r = fq2_zero(); if (j == 0) r.re = fe_load_one(f); return r; }

// ---- teams ----------------------------------------------------------------------------------------------------------------------------------
// the host's: slot d, coefficient j at s[d * 6 + j]; the G1 operands (x, y) at pts[j]
struct PrHostTeam {
    Fq2 *s, *pts;
    template <class F> H2R_FD void each(uint32_t d, F &&fn) {
        Fq2 r[6];
        for (uint32_t k = 0; k < 6; ++k) r[k] = fn(k);
        for (uint32_t k = 0; k < 6; ++k) s[d * 6 + k] = r[k];
    }
    template <class F> H2R_FD void each_point(F &&fn) { for (uint32_t j = 0; j < PR_MAX_PAIRS; ++j) pts[j] = fn(j); }
};
#if defined(__HIPCC__)
// the device's: lane k of the team, the store in LDS.  EVERY lane of the workgroup calls every operation (the barriers).
struct PrLaneTeam {
    Fq2 *s, *pts;
    uint32_t k;
    template <class F> __device__ __forceinline__ void each(uint32_t d, F &&fn) {
        const Fq2 r = fn(k < 6 ? k : k - 6);
        __syncthreads();
        if (k < 6) s[d * 6 + k] = r;
        __syncthreads();
    }
    template <class F> __device__ __forceinline__ void each_point(F &&fn) {
        const Fq2 r = fn(k & (PR_MAX_PAIRS - 1));
        if (k < PR_MAX_PAIRS) pts[k] = r;
        __syncthreads();
    }
};
#endif

// ---- the G1 operands ------------------------------------------------------------------------------------------------------------------------
// J points of 64 bytes: H2R_E_SHAPE for a coordinate >= q anywhere, else H2R_E_ASSERTION for a point that is neither (0, 0) nor on the curve
// (two passes, ordered as h2r_proof_decode orders them)
H2R_FD uint32_t pr_points_status(const uint8_t *p, uint32_t J, const PairingConsts &c) {
    if (!pr_in_range(p, 2 * J, c)) return (uint32_t)H2R_E_SHAPE;
    const FieldConsts &f = c.fq;
    bool off = false;
    H2R_PR_ROLLED
    for (uint32_t j = 0; j < J; ++j) {
        const Fe x = pr_ld(p + (uint64_t)j * 64, c), y = pr_ld(p + (uint64_t)j * 64 + 32, c);
        const Fe rhs = fe_add(fe_mont_mul(fe_mont_mul(x, x, f), x, f), c.b, f.p);
        if (!(fe_is_zero(x) && fe_is_zero(y)) && !fe_eq(fe_mont_mul(y, y, f), rhs)) off = true;
    }
    return off ? (uint32_t)H2R_E_ASSERTION : 0u;
}
// the team's operands: pair j's point, y negated where bit j of `mask` is set; (0, 0) for j >= J and for a circuit that is not `live`
// (flagged, or padding: its memory is not read)
template <class T> H2R_FD void pr_set_points(T &t, const uint8_t *p, uint32_t J, uint32_t mask, bool live, const PairingConsts &c) {
    t.each_point([&](uint32_t j) __attribute__((always_inline)) {
        Fq2 r = fq2_zero();
        if (live && j < J) {
            r.re = pr_ld(p + (uint64_t)j * 64, c); r.im = pr_ld(p + (uint64_t)j * 64 + 32, c);
            if ((mask >> j) & 1u) r.im = fe_sub(fe_zero(), r.im, c.fq.p);
        }
        return r;
    });
}

// ---- the Miller value -----------------------------------------------------------------------------------------------------------------------
// the line of one table step at P = (x, y); the identity (0, 0) contributes the line 1
H2R_FD PrLine pr_line(const uint8_t *step, const Fq2 &P, const PairingConsts &c) {
    const FieldConsts &f = c.fq;
    const bool ident = fq2_is_zero(P);
    const Fq2 lam = pr_ld2(step, c), cc = pr_ld2(step + 64, c), l1 = fq2_neg(fq2_mul_fe(lam, P.re, f), f), z = fq2_zero();
    PrLine l;
    l.l0 = ident ? fe_load_one(f) : P.im; l.l1 = ident ? z : l1; l.l3 = ident ? z : cc;
    return l;
}
// slot 0 = the Miller value of the team's operands against the tables at tab + j * tab_stride.  The 102 steps: a doubling step squares
// first (one squaring for all pairs), an addition step and the two Frobenius steps only multiply by the lines.
template <class T> H2R_FD void pr_miller(T &t, uint32_t J, const uint8_t *tab, uint64_t tab_stride, const PairingConsts &c) {
    const FieldConsts &f = c.fq;
    t.each(0, [&](uint32_t k) __attribute__((always_inline)) { return fq12_one_coeff(k, f); });
    int bit = 63;
    bool add_next = false;
    H2R_PR_ROLLED
    for (uint32_t step = 0; step < PR_STEPS; ++step) {
        const bool dbl = !add_next && bit >= 0;
        if (dbl) {
            t.each(0, [&](uint32_t k) __attribute__((always_inline)) { return fq12_square_coeff(t.s, k, f); });
            add_next = ((PR_LOOP_LO >> bit) & 1ull) != 0;
            --bit;
        } else add_next = false;
        H2R_PR_ROLLED
        for (uint32_t j = 0; j < J; ++j) {
            const PrLine l = pr_line(tab + (uint64_t)j * tab_stride + (uint64_t)step * PR_STEP_BYTES, t.pts[j], c);
            t.each(0, [&](uint32_t k) __attribute__((always_inline)) { return fq12_mul_line_coeff(t.s, l, k, f); });
        }
    }
}

// ---- the final exponentiation ---------------------------------------------------------------------------------------------------------------
// slot 0 <- slot 0 ^ ((q^12 - 1) / r), exactly: the easy part (q^6 - 1)(q^2 + 1) with the inverse through the norms -- N = f conj(f) in Fq6,
// t = N^(q^2) N^(q^4), n = N t in Fq2, f^-1 = conj(f) t n^-1 -- then (q^4 - q^2 + 1) / r = q^3 + (6 u^2 + 1) q^2 + (-36 u^3 - 18 u^2 - 12 u + 1) q
// + (-36 u^3 - 30 u^2 - 18 u - 2) (Devegili, Scott, Dahab): with a = m^u, b = a^u, c = b^u and t = c^36 b^18 a^12,
//     m^(q^3) (b^6 m)^(q^2) (conj(t) m)^q conj(t b^12 a^6 m^2);   a negative exponent is a conjugation, m being unitary.
// A program of team operations over the slots; PR_OP_POWU expands to a copy and 62 squarings with a product after each set bit of u.
enum : uint8_t { PR_OP_MUL, PR_OP_CONJ, PR_OP_FROB, PR_OP_SCALE_INV, PR_OP_POWU, PR_OP_COPY, PR_OP_NOP };
struct PrOp { uint8_t op, d, a, b; };   // d <- a * b | conj(a) | pi^b(a) | a / b[0] | a^u | a
constexpr uint32_t PR_PROG_LEN = 45;
H2R_FD PrOp pr_prog(uint32_t pc) {
    constexpr PrOp prog[PR_PROG_LEN] = {
        {PR_OP_CONJ, 1, 0, 0}, {PR_OP_MUL, 2, 0, 1},                         // conj f; N
        {PR_OP_FROB, 3, 2, 2}, {PR_OP_FROB, 4, 3, 2}, {PR_OP_MUL, 3, 3, 4},  // t = N^(q^2) N^(q^4)
        {PR_OP_MUL, 4, 2, 3}, {PR_OP_MUL, 3, 1, 3}, {PR_OP_SCALE_INV, 3, 3, 4},   // n; conj f t; f^-1
        {PR_OP_MUL, 1, 1, 3}, {PR_OP_FROB, 2, 1, 2}, {PR_OP_MUL, 0, 2, 1},   // g = f^(q^6 - 1); m = g^(q^2) g
        {PR_OP_POWU, 1, 0, 0}, {PR_OP_POWU, 2, 1, 0}, {PR_OP_POWU, 3, 2, 0}, // a, b, c
        {PR_OP_MUL, 4, 1, 1}, {PR_OP_MUL, 5, 4, 4}, {PR_OP_MUL, 4, 5, 4}, {PR_OP_MUL, 5, 4, 4},                          // 4 = a^6, 5 = a^12
        {PR_OP_MUL, 6, 2, 2}, {PR_OP_MUL, 7, 6, 6}, {PR_OP_MUL, 6, 7, 6}, {PR_OP_MUL, 7, 6, 6}, {PR_OP_MUL, 8, 7, 6},   // 6 = b^6, 7 = b^12, 8 = b^18
        {PR_OP_MUL, 9, 3, 3}, {PR_OP_MUL, 9, 9, 9}, {PR_OP_MUL, 9, 9, 9}, {PR_OP_MUL, 9, 9, 3}, {PR_OP_MUL, 9, 9, 9}, {PR_OP_MUL, 9, 9, 9},   // 9 = c^36
        {PR_OP_MUL, 9, 9, 8}, {PR_OP_MUL, 9, 9, 5},                          // 9 = t
        {PR_OP_MUL, 8, 9, 7}, {PR_OP_MUL, 8, 8, 4}, {PR_OP_MUL, 5, 0, 0}, {PR_OP_MUL, 8, 8, 5}, {PR_OP_CONJ, 8, 8, 0},   // 8 = conj(t b^12 a^6 m^2)
        {PR_OP_CONJ, 9, 9, 0}, {PR_OP_MUL, 9, 9, 0}, {PR_OP_FROB, 9, 9, 1},  // 9 = (conj(t) m)^q
        {PR_OP_MUL, 6, 6, 0}, {PR_OP_FROB, 6, 6, 2},                         // 6 = (b^6 m)^(q^2)
        {PR_OP_FROB, 5, 0, 3},                                                // 5 = m^(q^3)
        {PR_OP_MUL, 0, 5, 6}, {PR_OP_MUL, 0, 0, 9}, {PR_OP_MUL, 0, 0, 8}};
    return prog[pc];
}
// one team operation
template <class T> H2R_FD void pr_exec(T &t, const PrOp &o, const PairingConsts &c) {
    const FieldConsts &f = c.fq;
    const Fq2 *a = t.s + (uint32_t)o.a * 6, *b = t.s + (uint32_t)o.b * 6;
    t.each(o.d, [&](uint32_t k) __attribute__((always_inline)) {
        if (o.op == PR_OP_MUL) return fq12_product_coeff(a, b, k, f);
        if (o.op == PR_OP_FROB) return fq12_frob_coeff(a, o.b, k, c);
        if (o.op == PR_OP_CONJ) return fq12_conj_coeff(a, k, f);
        if (o.op == PR_OP_SCALE_INV) return fq2_mul(a[k], fq2_inv(b[0], f), f);
        return a[k];
    });
}
template <class T> H2R_FD void pr_final_exp(T &t, const PairingConsts &c) {
    uint32_t pc = 0;
    int sub = -1;                                             // inside a PR_OP_POWU: the next of its 124 phases
    H2R_PR_ROLLED
    while (pc < PR_PROG_LEN) {
        PrOp o = pr_prog(pc);
        if (o.op == PR_OP_POWU) {
            if (sub < 0) { o.op = PR_OP_COPY; sub = 0; }      // d = a: the top bit of u (bit 62)
            else {
                const int bit = 61 - (sub >> 1);
                const uint8_t base = o.a;
                if (!(sub & 1)) { o.op = PR_OP_MUL; o.a = o.d; o.b = o.d; }
                else { o.op = ((PR_U >> bit) & 1ull) ? PR_OP_MUL : PR_OP_NOP; o.a = o.d; o.b = base; }
                if (++sub == 124) { sub = -1; ++pc; }
            }
        } else ++pc;
        if (o.op != PR_OP_NOP) pr_exec(t, o, c);
    }
}
// the inverse alone (h2r_pairing_eval op 1): slot 0 <- 1 / slot 0, the first eight operations of the program and a copy
template <class T> H2R_FD void pr_inverse(T &t, const PairingConsts &c) {
    for (uint32_t pc = 0; pc < 8; ++pc) pr_exec(t, pr_prog(pc), c);
    PrOp o; o.op = PR_OP_COPY; o.d = 0; o.a = 3; o.b = 0;
    pr_exec(t, o, c);
}
H2R_FD bool pr_is_one(const Fq2 *a, const FieldConsts &f) {
    bool one = true;
    H2R_PR_ROLLED
    for (uint32_t j = 0; j < 6; ++j) if (!fq2_eq(a[j], fq12_one_coeff(j, f))) one = false;
    return one;
}

// ---- key material: the table of a fixed Q in G2 (host) ------------------------------------------------------------------------------------
// g2 = x.re, x.im, y.re, y.im -> PR_STEPS x (lambda, c = lambda x_T - y_T), both in the ctx's representation.  H2R_E_SHAPE for a coordinate >= q,
// H2R_E_ASSERTION for the identity (all zero) or a point off E'.  Membership of the order-r subgroup is NOT checked (key material); outside
// it a step may divide by zero (fe_inv's garbage, no hang).
inline uint32_t pr_prepare(const uint8_t *g2, uint8_t *table, const PairingConsts &c) {
    const FieldConsts &f = c.fq;
    if (!pr_in_range(g2, 4, c)) return (uint32_t)H2R_E_SHAPE;
    const Fq2 xq = pr_ld2(g2, c), yq = pr_ld2(g2 + 64, c);
    if (fq2_is_zero(xq) && fq2_is_zero(yq)) return (uint32_t)H2R_E_ASSERTION;
    if (!fq2_eq(fq2_square(yq, f), fq2_add(fq2_mul(fq2_square(xq, f), xq, f), c.b2, f))) return (uint32_t)H2R_E_ASSERTION;
    Fq2 xt = xq, yt = yq;
    uint32_t step = 0;
    auto emit = [&](const Fq2 &lam) { pr_st2(table + (uint64_t)step * PR_STEP_BYTES, lam, c); pr_st2(table + (uint64_t)step * PR_STEP_BYTES + 64, fq2_sub(fq2_mul(lam, xt, f), yt, f), c); ++step; };
    auto move = [&](const Fq2 &lam, const Fq2 &xs) {          // T <- the third point of the line of slope lam through T and (xs, .), mirrored
        const Fq2 x3 = fq2_sub(fq2_sub(fq2_square(lam, f), xt, f), xs, f);
        yt = fq2_sub(fq2_mul(lam, fq2_sub(xt, x3, f), f), yt, f); xt = x3;
    };
    auto slope_to = [&](const Fq2 &xs, const Fq2 &ys) { return fq2_mul(fq2_sub(ys, yt, f), fq2_inv(fq2_sub(xs, xt, f), f), f); };
    for (int bit = 63; bit >= 0; --bit) {
        const Fq2 x2 = fq2_square(xt, f);
        const Fq2 lam = fq2_mul(fq2_add(fq2_add(x2, x2, f), x2, f), fq2_inv(fq2_add(yt, yt, f), f), f);
        emit(lam); move(lam, xt);
        if ((PR_LOOP_LO >> bit) & 1ull) { const Fq2 l = slope_to(xq, yq); emit(l); move(l, xq); }
    }
    const Fq2 x1 = fq2_mul(fq2_conj(xq, f), c.g[0][2], f), y1 = fq2_mul(fq2_conj(yq, f), c.g[0][3], f);     // pi(Q)
    const Fq2 x2 = fq2_mul(fq2_conj(x1, f), c.g[0][2], f), y2 = fq2_mul(fq2_conj(y1, f), c.g[0][3], f);     // pi^2(Q)
    { const Fq2 l = slope_to(x1, y1); emit(l); move(l, x1); }
    emit(slope_to(x2, fq2_neg(y2, f)));
    return step == PR_STEPS ? 0u : (uint32_t)H2R_E_INTERNAL;
}

// Host: the constants over a curve's coordinate field, for one representation
inline void pairing_consts_init(const CurveConsts &cv, uint32_t mont, PairingConsts *pc) {
    const FieldConsts &f = cv.fq;
    pc->fq = f; pc->mont = mont; pc->pad_ = 0;
    const Fe one = fe_load_one(f);
    pc->b = fe_mul_small(one, cv.b3 / 3u, f.p);
    Fq2 xi; xi.re = fe_mul_small(one, 9u, f.p); xi.im = one;
    pc->b2 = fq2_mul_fe(fq2_inv(xi, f), pc->b, f);
    uint64_t e[4]; unsigned __int128 rem = 0;                 // (q - 1) / 6 (q = 1 mod 6)
    for (int k = 3; k >= 0; --k) { const unsigned __int128 cur = (rem << 64) | (f.p[k] - (k == 0 ? 1u : 0u)); e[k] = (uint64_t)(cur / 6u); rem = cur % 6u; }
    Fq2 g = fq12_one_coeff(0, f);
    for (int bit = 255; bit >= 0; --bit) { g = fq2_square(g, f); if ((e[bit >> 6] >> (bit & 63)) & 1ull) g = fq2_mul(g, xi, f); }
    for (uint32_t j = 0; j < 6; ++j) {
        pc->g[0][j] = j ? fq2_mul(pc->g[0][j - 1], g, f) : fq12_one_coeff(0, f);
        pc->g[1][j] = fq2_mul(pc->g[0][j], fq2_conj(pc->g[0][j], f), f);   // gamma_1^(q + 1)
        pc->g[2][j] = fq2_mul(pc->g[1][j], pc->g[0][j], f);               // gamma_1^(q^2 + q + 1), gamma_1^(q^2) = gamma_1
    }
}
// ... of a ctx field (H2R_FIELD_*) with a curve, or nullptr; built on first use
inline const PairingConsts *pairing_consts_of(uint32_t field, bool mont) {
    const CurveConsts *cv = curve_of_field(field);
    if (!cv || field != 0u) return nullptr;                   // bn256 is the one pairing-friendly instance
    static const struct Table {
        PairingConsts c[2];
        Table() { const CurveConsts *v = curve_of_field(0u); pairing_consts_init(*v, 0u, &c[0]); pairing_consts_init(*v, 1u, &c[1]); }
    } table;
    return &table.c[mont ? 1 : 0];
}

// ---- the kernel's argument ------------------------------------------------------------------------------------------------------------------
struct PairingArgs {
    const uint8_t *tables;                              // [num_pairs][PR_TABLE_BYTES], shared by the batch
    const uint8_t *points; uint64_t points_elem_stride; // circuit e: num_pairs x 64 bytes at points + e * stride
    uint8_t *gt;                                        // nullable [batch][384]
    uint8_t *accept;                                    // nullable [batch]
    uint8_t *status;                                    // nullable, never cleared
    uint64_t batch;
    uint32_t block0, num_pairs, negate_mask, pad_;
    PairingConsts c;
};

#ifdef H2R_TU_PAIRING

// grid (workgroups of PR_TEAMS circuits of one launch), 64 lanes = one wavefront = 8 teams of 8.  A flagged circuit, an identity operand and
// the padding teams of the last workgroup run to the end on the value 1: every lane reaches every barrier, only the stores are masked.
__global__ __launch_bounds__(PR_LANES) void pairing_kernel(PairingArgs a) {
    __shared__ Fq2 sh[PR_TEAMS * PR_TEAM_FQ2];
    const uint32_t team = threadIdx.x / PR_TEAM;
    const uint64_t e = ((uint64_t)a.block0 + blockIdx.x) * PR_TEAMS + team;
    const bool live = e < a.batch;
    const uint8_t *p = a.points + (live ? e : 0) * a.points_elem_stride;
    uint32_t st_in = 0, st = 0;
    if (live) {
        st_in = a.status ? a.status[e] : 0u;
        if (!st_in) st = pr_points_status(p, a.num_pairs, a.c);
    }
    const bool run = live && !st_in && !st;
    PrLaneTeam t{sh + team * PR_TEAM_FQ2, sh + team * PR_TEAM_FQ2 + PR_SLOTS * 6, threadIdx.x % PR_TEAM};
    pr_set_points(t, p, a.num_pairs, a.negate_mask, run, a.c);
    pr_miller(t, a.num_pairs, a.tables, PR_TABLE_BYTES, a.c);
    pr_final_exp(t, a.c);
    if (!live) return;                                        // (behind the last barrier)
    const bool one = pr_is_one(t.s, a.c.fq);
    if (run && a.gt && t.k < 6) pr_st2(a.gt + e * PR_FQ12_BYTES + t.k * 64, t.s[t.k], a.c);
    if (t.k == 0) {
        if (st && a.status) a.status[e] = (uint8_t)st;
        if (a.accept) a.accept[e] = (run && one) ? 1 : 0;
    }
}

#endif  // H2R_TU_PAIRING

}  // namespace h2r
