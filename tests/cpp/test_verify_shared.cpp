// AddressSanitizer / UBSan build of the functions the verifier's kernels share with the host (csrc/h2r_verify.hpp):
// the header itself is compiled instrumented into this stand-alone program, and the decoder, the scalars and the sum of terms run over
// exact-size heap buffers on inputs whose answers follow from the curve alone -- G = (1, 2) decodes from x = 1, [r]G is the identity,
// P + (-P) too, x a root of unity is an assertion.  No device work and no library: host code only.
//   hipcc --cuda-host-only -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Ihalo2_rsa_amd/csrc
//         tests/cpp/test_verify_shared.cpp -o test_verify_shared
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "h2r_verify.hpp"

using namespace h2r;

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

template <typename T> static std::unique_ptr<T[]> heap(size_t n) { return std::unique_ptr<T[]>(new T[n]()); }

static const u64 kR[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};   // bn256 Fr

static TrConsts consts(const CurveConsts &cv, u32 mont) {
    TrConsts c;
    std::memset(static_cast<void *>(&c), 0, sizeof c);
    field_consts_init(kR, &c.fr);
    c.fq = cv.fq; c.mont = mont;
    return c;
}

static int decoder(const CurveConsts &cv, u32 mont) {
    const TrConsts c = consts(cv, mont);
    u64 e[4], t[4], cy = 1;                                   // (q + 1) / 4
    for (int k = 0; k < 4; ++k) { t[k] = cv.fq.p[k] + cy; cy = t[k] < cy ? 1 : 0; }
    for (int k = 0; k < 4; ++k) e[k] = (t[k] >> 2) | (k < 3 ? t[k + 1] << 62 : 0);
    auto in = heap<u8>(32); auto out = heap<u8>(64);
    for (u64 sign = 0; sign < 2; ++sign) {                    // x = 1: G = (1, 2) and its negative
        Fe raw = fe_small(1);
        raw.v[3] |= sign << 63;
        std::memcpy(in.get(), raw.v, 32);
        REQUIRE(vf_item_range(VF_POINT, vf_ld(in.get()), c) == 0);
        Fe x, y;
        REQUIRE(vf_decode_point(vf_ld(in.get()), e, cv.b3, c, x, y) == 0);
        vf_st(out.get(), x); vf_st(out.get() + 32, y);
        const Fe xc = mont ? fe_from_mont(vf_ld(out.get()), cv.fq) : vf_ld(out.get()), yc = mont ? fe_from_mont(vf_ld(out.get() + 32), cv.fq) : vf_ld(out.get() + 32);
        REQUIRE(fe_eq(xc, fe_small(1)) && (yc.v[0] & 1) == sign);
        REQUIRE(sign ? fe_eq(fe_add(yc, fe_small(2), cv.fq.p), fe_zero()) : fe_eq(yc, fe_small(2)));
    }
    Fe q = fe_words(cv.fq.p), r = fe_words(kR), top;
    for (int k = 0; k < 4; ++k) top.v[k] = ~0ull;
    REQUIRE(vf_item_range(VF_POINT, q, c) == (u32)H2R_E_SHAPE && vf_item_range(VF_POINT, top, c) == (u32)H2R_E_SHAPE);
    REQUIRE(vf_item_range(VF_SCALAR, r, c) == (u32)H2R_E_SHAPE && vf_item_range(VF_SCALAR, top, c) == (u32)H2R_E_SHAPE && vf_item_range(VF_SCALAR, fe_zero(), c) == 0);
    u32 not_points = 0;                                       // about half of the small abscissae are no point's
    for (u64 xs = 2; xs < 34; ++xs) {
        Fe x, y;
        const u32 st = vf_decode_point(fe_small(xs), e, cv.b3, c, x, y);
        REQUIRE(st == 0 || st == (u32)H2R_E_ASSERTION);
        not_points += st != 0;
    }
    REQUIRE(not_points > 4 && not_points < 28);
    const Fe s = vf_decode_scalar(fe_small(5), c);
    REQUIRE(fe_eq(mont ? fe_from_mont(s, c.fr) : s, fe_small(5)));
    return 0;
}

static int terms(const CurveConsts &cv, u32 mont) {
    FieldConsts fr;
    field_consts_init(kR, &fr);
    auto put_scalar = [&](u8 *p, Fe s) { if (mont && !ge_p(s.v, fr.p)) s = fe_to_mont(s, fr); std::memcpy(p, s.v, 32); };
    auto put_point = [&](u8 *p, u64 x, Fe y) {
        Fe xx = fe_small(x);
        if (mont) { xx = fe_to_mont(xx, cv.fq); y = fe_to_mont(y, cv.fq); }
        std::memcpy(p, xx.v, 32); std::memcpy(p + 32, y.v, 32);
    };
    auto sum = [&](const u8 *rec, u32 T, u8 *out) {
        PtProj acc = pt_identity(cv);
        for (u32 t = 0; t < T; ++t) acc = pt_add(acc, vf_term(rec + t * 96, rec + t * 96 + 32, mont, fr, cv), cv);
        vf_store_sum(out, acc, mont, cv);
    };
    const Fe two = fe_small(2), minus_two = fe_sub(fe_zero(), two, cv.fq.p);
    auto rec = heap<u8>(3 * 96); auto out = heap<u8>(64); auto zero = heap<u8>(64);
    // [r] G = O (canonical ctx: the integer r itself; a Montgomery ctx reads r as r * R^-1, so it takes r - 1 and one more G)
    if (!mont) { put_scalar(rec.get(), fe_words(kR)); put_point(rec.get() + 32, 1, two); sum(rec.get(), 1, out.get()); REQUIRE(std::memcmp(out.get(), zero.get(), 64) == 0); }
    put_scalar(rec.get(), fe_sub(fe_zero(), fe_small(1), fr.p)); put_point(rec.get() + 32, 1, two);
    put_scalar(rec.get() + 96, fe_small(1)); put_point(rec.get() + 128, 1, two);
    sum(rec.get(), 2, out.get());
    REQUIRE(std::memcmp(out.get(), zero.get(), 64) == 0);
    // G + (-G) = O; 0 * G + 1 * O + 1 * G = G
    put_scalar(rec.get(), fe_small(1)); put_point(rec.get() + 32, 1, two); put_scalar(rec.get() + 96, fe_small(1)); put_point(rec.get() + 128, 1, minus_two);
    sum(rec.get(), 2, out.get());
    REQUIRE(std::memcmp(out.get(), zero.get(), 64) == 0);
    put_scalar(rec.get(), fe_zero()); std::memset(rec.get() + 128, 0, 64); put_scalar(rec.get() + 192, fe_small(1)); put_point(rec.get() + 224, 1, two);
    sum(rec.get(), 3, out.get());
    REQUIRE(std::memcmp(out.get(), rec.get() + 224, 64) == 0);
    // G + G = [2] G
    put_scalar(rec.get(), fe_small(1)); put_scalar(rec.get() + 96, fe_small(1)); put_point(rec.get() + 128, 1, two);
    auto dbl = heap<u8>(64);
    sum(rec.get(), 2, dbl.get());
    put_scalar(rec.get(), fe_small(2));
    sum(rec.get(), 1, out.get());
    REQUIRE(std::memcmp(out.get(), dbl.get(), 64) == 0 && std::memcmp(out.get(), zero.get(), 64) != 0);
    return 0;
}

// Two configurations of the constraint expression (csrc/h2r_constraints.hpp: constraint_fold, the source over evaluations).  The smallest: one
// fixed column for every selector, one permutation column, no lookups.  The full one: two fixed columns, three permutation columns in sets
// of two (a ragged last set, Z_0 read at the last rotation), the lookup arguments 1 and 4 (A' read at the previous rotation).  log_n = 3,
// one blinding factor; the plans hold exactly what the expression reads, so a read of anything else leaves the exact-size buffers.
static int scalars(u32 mont, bool full) {
    auto a = std::make_unique<VerifyScalarsArgs>();
    std::memset(static_cast<void *>(a.get()), 0, sizeof *a);
    field_consts_init(kR, &a->f);
    const FieldConsts &f = a->f;
    const u32 F = full ? 2 : 1, m = full ? 3 : 1, S = full ? 2 : 1, mask = full ? 0x12 : 0, A = vf_popc(mask);
    a->mont = mont; a->log_n = 3; a->bf = 1; a->batch = 1;
    ConstraintShape &cs = a->cs;
    cs.m = m; cs.chunk_len = full ? 2 : 1; cs.n_sets = S; cs.lookup_mask = mask;
    if (full) {
        cs.gate_fixed[8] = 1; cs.src[1] = 2; cs.src[2] = 4; cs.table_tag = 1;
        cs.lookup_advice[1] = 3; cs.lookup_tag[1] = 1; cs.lookup_advice[4] = 0; cs.lookup_enable[4] = 1;
    }
    // the base order: 5 advice, A' / S' per argument, the S permutation Z, the A lookup Z, random, 4 h, 4 W, F fixed, m sigma, G
    const u32 pz = 5 + 2 * A, lz = pz + S, rnd = lz + A, h = rnd + 1, fx = h + 8, sg = fx + F;
    u32 q = 0, no = 0, rank = 0;
    auto col = [&](u32 g, u32 i, u32 msk, u32 pos, bool open) {
        a->ev_first[g][i] = (unsigned short)q; a->ev_mask[g][i] = (u8)msk; a->base_pos[g][i] = (unsigned short)pos; q += vf_popc(msk);
        if (open) a->open[no++] = VfPlanEntry{(u8)g, (u8)i, (u8)msk, 0};
    };
    for (u32 c = 0; c < 5; ++c) col(VF_G_ADVICE, c, c == 4 ? 3 : 1, c, full || c == 4);   // (the smallest: advice 0..3 are evaluated and not opened)
    for (u32 i = 0; i < F; ++i) col(VF_G_FIXED, i, 1, fx + i, true);
    for (u32 c = 0; c < m; ++c) col(VF_G_SIGMA, c, 1, sg + c, true);
    for (u32 s = 0; s < S; ++s) col(VF_G_PERM_Z, s, s + 1 < S ? 7 : 3, pz + s, true);
    for (u32 k = 0; k < QUOT_LOOKUP_ARGS; ++k) {
        if (!((mask >> k) & 1u)) continue;
        col(VF_G_LOOKUP_Z, k, 3, lz + rank, true); col(VF_G_LOOKUP_A, k, 9, 5 + 2 * rank, true); col(VF_G_LOOKUP_S, k, 1, 6 + 2 * rank, true);
        ++rank;
    }
    a->base_pos[VF_G_RANDOM][0] = (unsigned short)rnd; a->base_pos[VF_G_H][0] = (unsigned short)h; a->w_pos = h + 4; a->g_pos = sg + m; a->num_bases = a->g_pos + 1;
    a->open[no++] = VfPlanEntry{VF_G_H, 0, 1, 0};
    a->num_open = no;
    // omega of order 8: 7^((r - 1) / 8) by square-and-multiply
    Fe e = fe_sub(fe_words(kR), fe_small(1), f.p), w = fe_words(f.one);
    for (int s = 0; s < 3; ++s) { e.v[0] = (e.v[0] >> 1) | (e.v[1] << 63); e.v[1] = (e.v[1] >> 1) | (e.v[2] << 63); e.v[2] = (e.v[2] >> 1) | (e.v[3] << 63); e.v[3] >>= 1; }
    const Fe seven = fe_to_mont(fe_small(7), f);
    for (int bit = 255; bit >= 0; --bit) { w = fe_mont_mul(w, w, f); if ((e.v[bit >> 6] >> (bit & 63)) & 1) w = fe_mont_mul(w, seven, f); }
    Fe w4 = fe_mont_mul(fe_mont_mul(w, w, f), fe_mont_mul(w, w, f), f);
    REQUIRE(fe_is_zero(fe_add(w4, fe_words(f.one), f.p)));                     // omega^4 = -1
    auto inv = [&](const Fe &x) { return fe_to_mont(fe_inv(fe_from_mont(x, f), f), f); };
    a->zmul[ROT_CUR] = fe_words(f.one); a->zmul[ROT_NEXT] = w; a->zmul[ROT_PREV] = inv(w); a->zmul[ROT_LAST] = fe_mont_mul(a->zmul[ROT_PREV], a->zmul[ROT_PREV], f);
    a->ninv = inv(fe_to_mont(fe_small(8), f));
    cs.dpow[0] = fe_words(f.one);
    for (u32 c = 1; c < m; ++c) cs.dpow[c] = fe_mont_mul(cs.dpow[c - 1], seven, f);   // (delta: any element will do)
    auto repr = [&](u64 v) { const Fe x = fe_small(v); return mont ? fe_to_mont(x, f) : x; };
    auto ch = heap<u64>(7 * 4); auto ev = heap<u8>(32 * q); auto right = heap<u8>(32 * a->num_bases); auto left = heap<u8>(128); auto tmp = heap<Fe>(VF_MAX_INV);
    for (u32 k = 0; k < 7; ++k) { const Fe c = repr(3 + 2 * k); std::memcpy(ch.get() + 4 * k, c.v, 32); a->ch[k] = ch.get() + 4 * k; }
    for (u32 i = 0; i < q; ++i) { const Fe v = repr(100 + i); std::memcpy(ev.get() + 32 * i, v.v, 32); }
    std::memset(right.get(), 0xEE, 32 * a->num_bases);
    REQUIRE(vf_scalars(*a, 0, ev.get(), right.get(), left.get(), VfStore{tmp.get(), 1}) == 0);
    // left = u^p; W_p's scalar = u^p x omega^rot; the scalars nobody queries (advice 0..3, the random polynomial) are 0
    const Fe u = fe_to_mont(fe_small(15), f), x = fe_to_mont(fe_small(11), f);
    Fe up = fe_words(f.one);
    for (u32 p = 0; p < 4; ++p) {
        const Fe l = vf_ld(left.get() + 32 * p), wp = vf_ld(right.get() + 32 * (a->w_pos + p));
        REQUIRE(fe_eq(mont ? l : fe_to_mont(l, f), up));
        REQUIRE(fe_eq(mont ? wp : fe_to_mont(wp, f), fe_mont_mul(up, fe_mont_mul(x, a->zmul[p], f), f)));
        up = fe_mont_mul(up, u, f);
    }
    if (!full) for (u32 pos : {0u, 1u, 2u, 3u}) REQUIRE(fe_is_zero(vf_ld(right.get() + 32 * pos)));
    REQUIRE(fe_is_zero(vf_ld(right.get() + 32 * rnd)));
    REQUIRE(!fe_is_zero(vf_ld(right.get() + 32 * a->g_pos)) && !fe_is_zero(vf_ld(right.get() + 32 * (h + 3))));
    // x = omega^5: an assertion, nothing written; a challenge = r: a shape
    std::memset(right.get(), 0xEE, 32 * a->num_bases);
    Fe w5 = fe_mont_mul(w4, w, f);
    if (!mont) w5 = fe_from_mont(w5, f);
    std::memcpy(ch.get() + 16, w5.v, 32);
    REQUIRE(vf_scalars(*a, 0, ev.get(), right.get(), left.get(), VfStore{tmp.get(), 1}) == (u32)H2R_E_ASSERTION);
    std::memcpy(ch.get() + 16, kR, 32);
    REQUIRE(vf_scalars(*a, 0, ev.get(), right.get(), left.get(), VfStore{tmp.get(), 1}) == (u32)H2R_E_SHAPE);
    for (u32 i = 0; i < 32 * a->num_bases; ++i) REQUIRE(right[i] == 0xEE);
    return 0;
}

int main() {
    const CurveConsts *cv = curve_of_field(0);
    if (!cv) return 1;
    for (u32 mont = 0; mont < 2; ++mont)
        if (decoder(*cv, mont) || terms(*cv, mont) || scalars(mont, false) || scalars(mont, true)) return 1;
    std::printf("VERIFY_SHARED_OK 2 representations\n");
    return 0;
}
