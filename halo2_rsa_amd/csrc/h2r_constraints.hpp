// THIS circuit's constraint expression, once: the one main gate, up to PERM_MAX_COLUMNS permutation columns in sets, the five lookup
// arguments -- not a general expression evaluator.  The prover's quotient (h2r_quotient.hpp: columns on the extended domain) and the
// verifier (h2r_verify.hpp: evaluations at x) fold the same terms in the same order, or every proof is rejected; both call constraint_fold
// below and differ only in the SOURCE they hand it.  Third-party behaviour (halo2's plonk::evaluation::evaluate_h and plonk::verifier, not
// in the reference tree), restated in DESIGN.md section 2g; the Python models (tests/quotient_ref.py, tests/opening_ref.py) restate it
// independently.  With f<t> the rotation of a column by t rows (a point set of the verifier), X the point (X_j, or x), acc starts at 0
// and every term t does acc = acc * y + t, in this order (upstream's; part of the contract):
//   gate         sum_{i<5} s_i v_i + s_mul_ab v_0 v_1 + s_mul_cd v_2 v_3 + se_next v_4<+1> + s_const
//   permutation  l0 (1 - Z_0);  l_last (Z_{S-1}^2 - Z_{S-1});  for s = 1 .. S-1: l0 (Z_s - Z_{s-1}<-(blinding_factors + 1)>);
//                for s = 0 .. S-1: l_active (Z_s<+1> prod_{c in s} (v_c + beta sigma_c + gamma) - Z_s prod_{c in s} (v_c + delta^c beta X + gamma))
//   lookup k     (ascending over the selected arguments) with A_k = theta fixed[tag_k] + fixed[enable_k] v_(advice_k),
//                S = theta fixed[table_tag] + fixed[table_value]:
//                l0 (1 - Z_k);  l_last (Z_k^2 - Z_k);  l_active (Z_k<+1> (A'_k + beta)(S'_k + gamma) - Z_k (A_k + beta)(S + gamma));
//                l0 (A'_k - S'_k);  l_active (A'_k - S'_k)(A'_k - A'_k<-1>)
// The result is acc; the division by X^n - 1 is the caller's.
// A SOURCE answers, as elements the arithmetic below takes:
//   adv(c, rot), fix(c), sigma(c)                advice column c < 5 at a rotation; fixed and sigma columns (unrotated)
//   perm_value(src)                              permutation column source src: advice src < 5, else the prover's extra column src - 5
//   perm_z(s, rot), look_z(k, rot), a_perm(k, rot), s_perm(k)
//   l(i)                                         l0, l_last, l_active for i = 0, 1, 2
//   ident(c)                                     delta^c beta X
//   theta(), beta(), gamma(), y(); one(), mul, add, sub
// so the fold names no field and no memory.  A source whose reads record themselves and whose arithmetic does nothing turns the fold into
// the list of evaluations the expression needs (h2r_api.hip: the verifier's plan check).
#pragma once

#include "h2r_kernels.hpp"

namespace h2r {

constexpr u32 QUOT_MAX_FIXED = 16;
constexpr u32 QUOT_LOOKUP_ARGS = 5;
constexpr u32 QUOT_PERM_MAX_COLUMNS = 8;
constexpr u32 QUOT_GATE_FIXED = 9;                  // sa, sb, sc, sd, se, s_mul_ab, s_mul_cd, se_next, s_const
// the rotations the expression reads: the rows 0, +1, -(blinding_factors + 1), -1.  The values are the bits of the verifier's plan masks.
constexpr u32 ROT_CUR = 0, ROT_NEXT = 1, ROT_LAST = 2, ROT_PREV = 3, ROTATIONS = 4;

struct ConstraintShape {
    u32 m, chunk_len, n_sets, lookup_mask;          // permutation columns, columns of a set (<= m), sets; bit k = lookup argument k takes part
    u8 gate_fixed[QUOT_GATE_FIXED], src[QUOT_PERM_MAX_COLUMNS];
    u8 lookup_advice[QUOT_LOOKUP_ARGS], lookup_tag[QUOT_LOOKUP_ARGS], lookup_enable[QUOT_LOOKUP_ARGS], table_tag, table_value;
    Fe dpow[QUOT_PERM_MAX_COLUMNS];                 // delta^c, Montgomery form
};

// the arithmetic of both real sources: the Montgomery domain of f
struct ConstraintField {
    const FieldConsts &f;
    H2R_FD Fe one() const { return fe_words(f.one); }
    H2R_FD Fe mul(const Fe &x, const Fe &w) const { return fe_mont_mul(x, w, f); }
    H2R_FD Fe add(const Fe &x, const Fe &w) const { return fe_add(x, w, f.p); }
    H2R_FD Fe sub(const Fe &x, const Fe &w) const { return fe_sub(x, w, f.p); }
};

#if defined(__HIP_DEVICE_COMPILE__)
#define H2R_ROLLED _Pragma("unroll 1")              // a loop of the fold stays a loop on the device
#else
#define H2R_ROLLED
#endif

template <class Src> H2R_FD Fe constraint_fold(const ConstraintShape &cs, const Src &s) {
    // ---- the gate (the first term: acc = 0 * y + gate) ----
    Fe acc = fe_zero();
    H2R_ROLLED
    for (u32 pr = 0; pr < 2; ++pr) {   // (v_0, v_1) under sa, sb, s_mul_ab, then (v_2, v_3) under sc, sd, s_mul_cd
        const Fe va = s.adv(2 * pr, ROT_CUR), vb = s.adv(2 * pr + 1, ROT_CUR);
        acc = s.add(acc, s.add(s.mul(s.fix(cs.gate_fixed[2 * pr]), va), s.mul(s.fix(cs.gate_fixed[2 * pr + 1]), vb)));
        acc = s.add(acc, s.mul(s.fix(cs.gate_fixed[5 + pr]), s.mul(va, vb)));
    }
    acc = s.add(acc, s.mul(s.fix(cs.gate_fixed[4]), s.adv(4, ROT_CUR)));
    acc = s.add(acc, s.mul(s.fix(cs.gate_fixed[7]), s.adv(4, ROT_NEXT)));
    acc = s.add(acc, s.fix(cs.gate_fixed[8]));
    auto push = [&](const Fe &t) __attribute__((always_inline)) { acc = s.add(s.mul(acc, s.y()), t); };
    const Fe one = s.one(), l0 = s.l(0), l_last = s.l(1), l_active = s.l(2);
    // ---- the permutation argument ----
    push(s.mul(l0, s.sub(one, s.perm_z(0, ROT_CUR))));
    {
        const Fe z = s.perm_z(cs.n_sets - 1, ROT_CUR);
        push(s.mul(l_last, s.sub(s.mul(z, z), z)));
    }
    H2R_ROLLED
    for (u32 i = 1; i < cs.n_sets; ++i) push(s.mul(l0, s.sub(s.perm_z(i, ROT_CUR), s.perm_z(i - 1, ROT_LAST))));
    H2R_ROLLED
    for (u32 i = 0; i < cs.n_sets; ++i) {
        const u32 c0 = i * cs.chunk_len, c1 = c0 + cs.chunk_len < cs.m ? c0 + cs.chunk_len : cs.m;
        Fe left = s.perm_z(i, ROT_NEXT), right = s.perm_z(i, ROT_CUR);
        H2R_ROLLED
        for (u32 c = c0; c < c1; ++c) {
            const Fe vg = s.add(s.perm_value(cs.src[c]), s.gamma());
            left = s.mul(left, s.add(vg, s.mul(s.beta(), s.sigma(c))));
            right = s.mul(right, s.add(vg, s.ident(c)));
        }
        push(s.mul(l_active, s.sub(left, right)));
    }
    // ---- the lookup arguments ----
    if (cs.lookup_mask) {
        const Fe sg = s.add(s.add(s.mul(s.theta(), s.fix(cs.table_tag)), s.fix(cs.table_value)), s.gamma());   // S + gamma
        H2R_ROLLED
        for (u32 k = 0; k < QUOT_LOOKUP_ARGS; ++k) {
            if (!((cs.lookup_mask >> k) & 1u)) continue;
            const Fe z = s.look_z(k, ROT_CUR);
            push(s.mul(l0, s.sub(one, z)));
            push(s.mul(l_last, s.sub(s.mul(z, z), z)));
            const Fe ap = s.a_perm(k, ROT_CUR), sp = s.s_perm(k);
            {
                const Fe ak = s.add(s.mul(s.theta(), s.fix(cs.lookup_tag[k])), s.mul(s.fix(cs.lookup_enable[k]), s.adv(cs.lookup_advice[k], ROT_CUR)));
                const Fe left = s.mul(s.mul(s.look_z(k, ROT_NEXT), s.add(ap, s.beta())), s.add(sp, s.gamma()));
                const Fe right = s.mul(s.mul(z, s.add(ak, s.beta())), sg);
                push(s.mul(l_active, s.sub(left, right)));
            }
            const Fe d = s.sub(ap, sp);
            push(s.mul(l0, d));
            push(s.mul(l_active, s.mul(d, s.sub(ap, s.a_perm(k, ROT_PREV)))));
        }
    }
    return acc;
}

}  // namespace h2r
