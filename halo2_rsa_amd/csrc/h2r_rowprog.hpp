// Advice rows of the Fresh-integer family (add, sub, add_mod, sub_mod, is_zero, the comparisons, assert_in_field):
// the ops' flat-stream values (AuxGeom regions written by aux_kernel / fresh_kernel / the step kernel's aux role) laid out
// as rows of the main gate's five advice columns, every cell the ops assign.
//
// These ops are a tree of small main-gate calls whose shape depends only on (op, limb counts), never on the data.  The
// host therefore walks the reference's control flow ONCE per (ctx, op) SYMBOLICALLY -- each value is "where it lives"
// (a byte range of the element's region, a limb of an operand, a constant) instead of a number -- and records one
// descriptor per row (RowProgBuilder, below: same walk as big_integer/chip.rs:245-373, 452-528, 754-805, 908-1006,
// 1286-1318).  The kernel is an interpreter of that table: one thread per row, 5 cells fetched, 160 bytes staged in
// LDS and written out as whole 16-byte lines.  ~1,500 rows (240 KB) per assert_in_field of RSA-2048.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "h2r.h"
#include "h2r_kernels.hpp"
#include "h2r_field.hpp"

namespace h2r {

// row kinds beyond the mul_mod image's (h2r.h H2R_ROW_*)
enum { ROWK_SELECT = 15, ROWK_NOT = 16, /* ROWK_ASSERT_ONE = 17: h2r_kernels.hpp (the mul_mod image ends with one) */ ROWK_CONST_BM1 = 18, ROWK_ASSERT_ZERO = 19,
       ROWK_CONST_EM = 20,    // + j: assign_constant of the j-th constant of the encoded-message check (em_const)
       ROWK_RANGE_U32 = 48,   // + row of RangeChip::assign(value, 4, 32): eight 4-bit sub-limbs (src/chip.rs:170-171)
       ROWK_CONST_COEFF8 = 56 }; // + j: assign_constant(2^(8j)), the byte coefficients of the hashed-message limbs (src/lib.rs:228-229)

// the constants RSAChip::verify_pkcs1v15_signature assigns (src/chip.rs:149-152, 169, 174, 179, 190)
constexpr u32 EM_CONSTS = 6;
__host__ __device__ inline u64 em_const(u32 j) {
    switch (j) {
        case 0: return 217300885422736416ull;    // prefix_64_1
        case 1: return 938447882527703397ull;    // prefix_64_2
        case 2: return 1ull << 32;               // u32_v
        case 3: return 3158320ull;               // prefix_32
        case 4: return 4294967295ull;            // ff_32
        default: return 562949953421311ull;      // last_em
    }
}

enum : u8 {
    RP_ZERO = 0, RP_ONE, RP_B /* 2^w */, RP_BM1 /* 2^w - 1 */,
    RP_STREAM,              // little-endian unsigned integer of `width` bytes at region + off
    RP_IN_A, RP_IN_B, RP_IN_N,   // limb `off` of the element's operand
    RP_DIFF01,              // cell 0 - cell 1 (field subtraction): main_gate.sub's result
    RP_DIFF34,              // operand 3 - operand 4: the value is_zero is asked about
    RP_INV34,               // its inverse, or 1 when it is zero: is_zero's witness
    RP_CONST64,             // em_const(off)
    RP_POW2,                // 2^off, off < 64
    RP_HIDDEN = 0x80        // operand only: the cell itself is unassigned (zero)
};
struct RpCell { u32 off; u8 type, width; uint16_t pad; };
struct RpRow { RpCell c[5]; u32 kind, pad; };   // 48 bytes
static_assert(sizeof(RpRow) == 48, "three 16-byte loads per row");

// ---- host: the symbolic walk ---------------------------------------------------------------------------------------
//
// Origins.  Every value the walk hands on also remembers the cell where the reference FIRST assigned it: a row of this program and a
// column, limb j of an operand (H2R_COPY_SRC_A / _B / _N, as in copy_map_record), or nothing (an unassigned zero).  A row that takes a
// value with an origin as one of its visible cells records the copy pair (this row, that column) <- origin; the cells an op assigns
// fresh -- results, bits, inverses, range sub-limbs, constants -- become origins.  Same walk, so the pairs cannot drift from the rows.
constexpr u32 RP_NO_ORIGIN = 0xFFFFFFFFu;
constexpr u32 RP_ORIGIN_SEED = 0xFFFFFF04u;    // build_em: the preamble's assign_constant(1) (the whole element's CONST1 row)
constexpr u32 RP_ORIGIN_VALID = 0xFFFFFF05u;   // build_frame: the is_valid the encoded-message check returns (its last running AND)
struct RowProgBuilder {
    const AuxGeom g;
    std::vector<RpRow> rows;
    std::vector<h2r_copy> copies;   // (row, col) <- (src_row, src_col); rows of this program
    u64 off = 0;   // section cursor inside the element's region, as fresh_sections / the kernels advance it
    struct V : RpCell { u32 orow = RP_NO_ORIGIN, ocol = 0; };   // host only: the interpreter sees the RpCell
    using Int = std::vector<V>;

    explicit RowProgBuilder(const AuxGeom &g_) : g(g_) {}
    static V mk(u8 type, u32 off = 0, u8 width = 0) { V v; v.off = off; v.type = type; v.width = width; v.pad = 0; return v; }
    static V zero() { return mk(RP_ZERO); }
    static V one() { return mk(RP_ONE); }
    V st(u64 o, u32 width) const { return mk(RP_STREAM, (u32)o, (u8)width); }
    static V hidden(V v) { v.type |= RP_HIDDEN; return v; }
    static V at(V v, u32 orow, u32 ocol) { v.orow = orow; v.ocol = ocol; return v; }   // v, first assigned at (orow, ocol)
    static Int operand(u8 type, u32 n) {
        Int r;
        for (u32 i = 0; i < n; ++i) r.push_back(at(mk(type, i), type == RP_IN_A ? H2R_COPY_SRC_A : type == RP_IN_B ? H2R_COPY_SRC_B : H2R_COPY_SRC_N, i));
        return r;
    }

    u32 row(u32 kind, V c0 = zero(), V c1 = zero(), V c2 = zero(), V c3 = zero(), V c4 = zero()) {   // returns the row's index
        const V *c[5] = {&c0, &c1, &c2, &c3, &c4};
        const u32 idx = (u32)rows.size();
        RpRow r; r.kind = kind; r.pad = 0;
        for (u32 q = 0; q < 5; ++q) {
            r.c[q] = *c[q];
            if (!(c[q]->type & RP_HIDDEN) && c[q]->orow != RP_NO_ORIGIN) copies.push_back(h2r_copy{idx, q, c[q]->orow, c[q]->ocol});
        }
        rows.push_back(r);
        return idx;
    }
    V const_row(u32 kind, V v = zero()) { const u32 r = row(kind, v); return at(v, r, 0); }   // main_gate.assign_constant: the cell later rows copy
    V range_rows(u32 kind, V src, V value) {   // RangeChip::assign: two rows; the assigned value is column e of the first
        const u32 r = row(kind + 0, src);
        row(kind + 1, src);
        return at(value, r, 4);
    }
    V range_limb(u64 ra_off) {   // RangeChip::assign(limb, w/8, w): value at ra_off, its eight sub-limb bytes behind it
        return range_rows(ROWK_RANGE_LIMB, st(ra_off, g.LB), st(ra_off, g.LB));
    }
    // main_gate.is_zero(d = x - y): assign_bit(r), [d, d', r], [r, d]; d was first assigned where `d_at` says.  Returns r.
    V is_zero_rows(V x, V y, V flag, V d_at) {
        const V f = at(flag, row(ROWK_BIT, flag, flag, flag), 0);
        const V d = at(mk(RP_DIFF34), d_at.orow, d_at.ocol);
        row(ROWK_ISZERO_INV, d, mk(RP_INV34), f, hidden(x), hidden(y));
        row(ROWK_ISZERO_RA, f, d, zero(), hidden(x), hidden(y));
        return f;
    }
    V is_equal(V x, V y, V flag) {          // main_gate.is_equal = sub + is_zero
        const u32 r = row(ROWK_SUB, x, y, mk(RP_DIFF01));
        return is_zero_rows(x, y, flag, at(zero(), r, 2));
    }

    Int add(const Int &a, const Int &b) {   // chip.rs:245-297; section layout of aux_add
        const u32 n = (u32)std::max(a.size(), b.size());
        const u64 sec = off;
        off += g.add_sz(n);
        const V zv = const_row(ROWK_CONST0);              // zero_value :254: pads the shorter operand, and is carrys[0]
        const V lmax = const_row(ROWK_CONST_B, mk(RP_B)); // limb_max_val :267
        Int out;
        V carry = zv;
        for (u32 i = 0; i < n; ++i) {
            const u64 q = sec + (u64)i * g.STEP;
            const V ai = i < a.size() ? a[i] : zv, bi = i < b.size() ? b[i] : zv;
            V a_b = st(q, g.SB), sum = st(q + g.SB, g.SB), cac = st(q + 2 * g.SB + 2 * g.RA, g.SB);
            a_b = at(a_b, row(ROWK_ADD, ai, bi, a_b), 2);            // :272
            sum = at(sum, row(ROWK_ADD, a_b, carry, sum), 2);        // :273
            const V c = range_limb(q + 2 * g.SB);                    // c :279-280
            const V cy = range_limb(q + 2 * g.SB + g.RA);            // carry :281-282
            cac = at(cac, row(ROWK_MUL_ADD, cy, lmax, c, cac), 3);   // :283
            row(ROWK_ASSERT_EQ, sum, cac);                           // :285
            out.push_back(c);
            carry = cy;
        }
        out.push_back(carry);                           // :290
        return out;
    }
    V is_equal_fresh(const Int &a, const Int &b) {   // chip.rs:780-805; (flag, running AND) byte pairs of aux_eq
        const u32 n1 = (u32)a.size(), n2 = (u32)b.size();
        const bool larger = n1 > n2;
        const u32 n = larger ? n1 : n2;
        const u64 sec = off;
        off += g.eq_sz(n);
        V eq = at(one(), row(ROWK_BIT, one(), one(), one()), 0);
        for (u32 i = 0; i < n; ++i) {
            V flag = st(sec + 2ull * i, 1), run = st(sec + 2ull * i + 1, 1);
            if (larger && i >= n2) flag = is_zero_rows(a[i], zero(), flag, a[i]);
            else if (!larger && i >= n1) flag = is_zero_rows(b[i], zero(), flag, b[i]);
            else flag = is_equal(a[i], b[i], flag);
            eq = at(run, row(ROWK_MUL, eq, flag, run), 2);   // and
        }
        return eq;
    }
    V is_zero(const Int &a) {                        // chip.rs:754-767 (the kernel writes it as aux_eq against zero)
        const u64 sec = off;
        off += g.eq_sz((u32)a.size());
        V bit = at(one(), row(ROWK_BIT, one(), one(), one()), 0);
        for (u32 i = 0; i < a.size(); ++i) {
            V flag = st(sec + 2ull * i, 1), run = st(sec + 2ull * i + 1, 1);
            flag = is_zero_rows(a[i], zero(), flag, a[i]);
            bit = at(run, row(ROWK_MUL, bit, flag, run), 2);
        }
        return bit;
    }
    Int sub_unchecked(const Int &a, const Int &b) {  // chip.rs:1286-1318; aux_subu
        const u32 n1 = (u32)a.size();
        const u64 sec = off;
        off += g.cl_sz(n1);
        Int c;
        for (u32 i = 0; i < n1; ++i) c.push_back(range_limb(sec + (u64)i * g.RA));
        const Int added = add(b, c);
        const V ok = is_equal_fresh(a, added);
        row(ROWK_ASSERT_ONE, ok);                       // assert_equal_fresh -> assert_one
        return c;
    }
    std::pair<Int, V> sub(const Int &a, const Int &b) {   // chip.rs:310-373; aux_sub
        const u32 nA = (u32)a.size(), n2 = (u32)b.size(), m = std::max(nA, n2), n1 = m + 1;
        Int max_int;
        for (u32 i = 0; i < n2; ++i) max_int.push_back(const_row(ROWK_CONST_BM1, mk(RP_BM1)));   // max_value :138-154
        const Int inflated_a = add(a, max_int);
        const Int is_ = sub_unchecked(inflated_a, b);
        V not_ov = st(off, 1), ov = st(off + 1, 1);
        off += 16;
        const V one_bit = at(one(), row(ROWK_BIT, one(), one(), one()), 0);   // one :326
        not_ov = is_equal(is_[n2], one_bit, not_ov);    // :330
        ov = at(ov, row(ROWK_NOT, not_ov, ov), 1);      // :331
        const V zv = const_row(ROWK_CONST0);            // zero_value :343
        Int sel_l, sel_r;
        const u64 sl = off, sr = off + AuxGeom::a16((u64)n1 * g.LB);
        off = sr + AuxGeom::a16((u64)m * g.LB);
        auto select = [&](V x, V y, V v) { return at(v, row(ROWK_SELECT, not_ov, x, not_ov, y, v), 4); };
        for (u32 i = 0; i < n1; ++i)                    // :345-357
            sel_l.push_back(select(is_[i], i >= n2 ? zv : b[i], st(sl + (u64)i * g.LB, g.LB)));
        for (u32 i = 0; i < m; ++i) {                   // :358-367
            const V v = st(sr + (u64)i * g.LB, g.LB);
            if (i >= nA) sel_r.push_back(select(max_int[i], zv, v));
            else if (i >= n2) sel_r.push_back(select(zv, a[i], v));
            else sel_r.push_back(select(max_int[i], a[i], v));
        }
        Int real = sub_unchecked(sel_l, sel_r);
        return {real, ov};
    }
    V is_less_than(const Int &a, const Int &b) {     // chip.rs:908-919; aux_less_than
        const V ov = sub(a, b).second;
        const V is_eq = is_equal_fresh(a, b);
        V is_not_eq = st(off, 1), lt = st(off + 1, 1);
        off += 16;
        is_not_eq = at(is_not_eq, row(ROWK_NOT, is_eq, is_not_eq), 1);   // :917
        return at(lt, row(ROWK_MUL, ov, is_not_eq, lt), 2);              // :918
    }
    void select_mod(const Int &x, const Int &y, V cond, u32 n_limbs) {   // tail of add_mod :466-478 / sub_mod :512-525
        const V zv = const_row(ROWK_CONST0);
        const u32 num = (u32)std::max(x.size(), y.size());
        Int out;
        for (u32 i = 0; i < num; ++i) {
            const V v = st(off + (u64)i * g.LB, g.LB);
            out.push_back(at(v, row(ROWK_SELECT, cond, i < x.size() ? x[i] : zv, cond, i < y.size() ? y[i] : zv, v), 4));
        }
        for (u32 i = n_limbs; i < num; ++i) row(ROWK_ASSERT_ZERO, out[i]);
    }

    V range_u32(u64 ra_off) { return range_rows(ROWK_RANGE_U32, st(ra_off, 4), st(ra_off, 4)); }
    // RSAChip::verify_pkcs1v15_signature after the modpow (src/chip.rs:138-198; 64-bit limbs): operand A = powed, B = hashed (4 limbs);
    // region = the encoded-message region the aux role wrote (flags, the two 32-bit range assigns, the recomposed limb)
    void build_em() {
        const u32 L = g.L;
        const Int A = operand(RP_IN_A, L), H = operand(RP_IN_B, 4);
        auto K = [&](u32 j) { return const_row(ROWK_CONST_EM + j, mk(RP_CONST64, j)); };
        V is_eq = at(one(), RP_ORIGIN_SEED, 0);             // the cell of the preamble's assign_constant(1), :137
        // is_eq = and(is_eq, is_equal(x, y)): the flag byte at `fo`, the running AND at `ro`
        auto eq_and = [&](V x, V y, u64 fo, u64 ro) { const V flag = is_equal(x, y, st(fo, 1)); is_eq = at(st(ro, 1), row(ROWK_MUL, is_eq, flag, st(ro, 1)), 2); };
        for (u32 i = 0; i < 4; ++i) eq_and(A[i], H[i], 2 * i, 2 * i + 1);                                            // :141-144
        const V k0 = K(0), k1 = K(1);                                                                                // :149-152
        const V f4 = is_equal(A[4], k0, st(8, 1)), f5 = is_equal(A[5], k1, st(9, 1));                                // :153-154
        is_eq = at(st(10, 1), row(ROWK_MUL, is_eq, f4, st(10, 1)), 2);                                               // :155
        is_eq = at(st(11, 1), row(ROWK_MUL, is_eq, f5, st(11, 1)), 2);                                               // :156
        const V low = range_u32(12), high = range_u32(24);                                                           // :170-171
        const V k2 = K(2);                                                                                           // :172
        const V concat = at(st(36, 8), row(ROWK_MUL_ADD, high, k2, low, st(36, 8)), 3);                              // :173
        row(ROWK_ASSERT_EQ, A[6], concat);                                                                           // :174
        const V k3 = K(3); eq_and(low, k3, 44, 45);                                                                  // :175-177
        const V k4 = K(4); eq_and(high, k4, 46, 47);                                                                 // :180-182
        const V ff = const_row(ROWK_CONST_BM1, mk(RP_BM1));                                                          // ff_64 :183-184
        for (u32 i = 7; i + 1 < L; ++i) { const u64 f = 48 + 2ull * (i - 7); eq_and(A[i], ff, f, f + 1); }           // :185-188
        const u64 f = 48 + 2ull * (L - 8);
        const V k5 = K(5); eq_and(A[L - 1], k5, f, f + 1);                                                           // :190-197
    }
    // RSASignatureVerifier::verify_pkcs1v15_signature, src/lib.rs:225-239: the four hashed-message limbs composed from the 32
    // reversed digest bytes; region = [32 byte cells][32 running limb values, 8 bytes each] (sha256_kernel, h2r_sha256.hpp)
    void build_hashed_msg() {
        for (u32 i = 0; i < 4; ++i) {
            V limb = const_row(ROWK_CONST0);                                         // limb_val = assign_constant(0) :226
            for (u32 j = 0; j < 8; ++j) {
                const V coeff = const_row(ROWK_CONST_COEFF8 + j, mk(RP_POW2, 8 * j)), nv = st(32 + 8ull * (8 * i + j), 8);   // :228-229
                limb = at(nv, row(ROWK_MUL_ADD, coeff, st(8 * i + j, 1), limb, nv), 3);   // :230-235 (the byte cells are the SHA-256 chip's)
            }
        }
    }
    void build_verify_preamble() { row(ROWK_CONST1, one()); }   // is_eq = assign_constant(1), src/chip.rs:137 (before the modpow)
    // What stands around the element in the reference's signature circuit (benches/bench.rs:145-221): assign_signature, assign_public_key
    // (Fix exponent: n only), the four hashed-message limbs -- RangeChip::assign per limb, operand A = signature, N = modulus, B = hashed --
    // and, behind the element, main_gate.assert_one(is_valid): region = the caller's is_valid byte.  The last row is the program's tail.
    void build_frame() {
        const u32 L = g.L;
        auto assign_integer = [&](u8 type, u32 n) { for (u32 j = 0; j < n; ++j) range_rows(ROWK_RANGE_LIMB, mk(type, j), mk(type, j)); };
        assign_integer(RP_IN_A, L);
        assign_integer(RP_IN_N, L);
        assign_integer(RP_IN_B, 4);
        row(ROWK_ASSERT_ONE, at(st(0, 1), RP_ORIGIN_VALID, 0));
    }

    // returns false for an unknown op
    bool build(u32 op, bool assert_one) {
        const u32 L = g.L;
        const Int A = operand(RP_IN_A, L), B = operand(RP_IN_B, L), N = operand(RP_IN_N, L);
        V bit = zero();
        bool has_bit = true;
        switch (op) {
            case FRESH_ADD: add(A, B); has_bit = false; break;
            case FRESH_SUB: sub(A, B); has_bit = false; break;
            case FRESH_ADD_MOD: { const Int added = add(A, B); auto s = sub(added, N); select_mod(added, s.first, s.second, L); has_bit = false; break; }
            case FRESH_SUB_MOD: {
                auto s1 = sub(A, B); auto s2 = sub(N, s1.first);
                row(ROWK_ASSERT_ZERO, s2.second);       // :510
                select_mod(s2.first, s1.first, s1.second, L); has_bit = false; break;
            }
            case FRESH_IS_ZERO: bit = is_zero(A); break;
            case FRESH_IS_EQUAL_FRESH: bit = is_equal_fresh(A, B); break;
            case FRESH_IS_LESS_THAN: case FRESH_IS_IN_FIELD: bit = is_less_than(A, B); break;
            case FRESH_IS_LESS_THAN_OR_EQUAL: bit = sub(A, B).second; break;
            case FRESH_IS_GREATER_THAN: { const V le = sub(A, B).second; bit = st(off, 1); bit = at(bit, row(ROWK_NOT, le, bit), 1); break; }              // :954-963
            case FRESH_IS_GREATER_THAN_OR_EQUAL: { const V lt = is_less_than(A, B); bit = st(off, 1); bit = at(bit, row(ROWK_NOT, lt, bit), 1); break; }   // :976-985
            default: return false;
        }
        if (assert_one) { if (!has_bit) return false; row(ROWK_ASSERT_ONE, bit); }
        return true;
    }
};

// ---- device: the interpreter ---------------------------------------------------------------------------------------
struct RowProgArgs {
    const RpRow *prog; u32 rows;
    const void *a, *b, *n; u64 a_stride, b_stride, n_stride;   // limbs between the elements' operands (0: one shared integer)
    const u8 *trace; u64 elem_stride, first_off;               // element e's region at trace + e * elem_stride + first_off
    const u8 *status; u64 batch;
    AdviceDst dst; const MontK *mk;     // the program's first row = row 0 of dst
    FieldConsts f;
    const u32 *inv_rows; u32 n_inv;     // the rows with an RP_INV34 cell (rowprog_inv_kernel fills those cells)
    u32 tail_rows; u64 tail_skip;       // the program's last tail_rows rows land tail_skip rows further down (the frame's assert_one behind the element)
};
// workgroups per element of a program whose rows are staged sr at a time: the head and the tail never share a stage
__host__ __device__ inline u32 rowprog_chunks(u32 rows, u32 tail_rows, u32 sr) { return (rows - tail_rows + sr - 1) / sr + (tail_rows + sr - 1) / sr; }

// the value a cell descriptor names, for element `elem` whose region starts at `reg`
template <int LW>
__device__ __forceinline__ Fe rp_fetch(const RowProgArgs &a, const u8 *reg, u32 elem, const RpCell &c) {
    using limb_t = typename LimbT<LW>::type;
    Fe v = fe_zero();
    switch (c.type & 0x7f) {
        case RP_ONE: v.v[0] = 1; break;
        case RP_B: if (LW == 64) v.v[1] = 1; else v.v[0] = 1ull << 32; break;
        case RP_BM1: v.v[0] = LW == 64 ? ~0ull : 0xffffffffull; break;
        case RP_STREAM: {
            const u8 *p = reg + c.off;
            if (c.width == 1) v.v[0] = p[0];
            else {   // 4, 8, 12 or 16 bytes on a 4-byte boundary
                const u32 *p4 = reinterpret_cast<const u32 *>(p);
                const u32 nw = c.width / 4;
                const u32 w0 = p4[0], w1 = nw > 1 ? p4[1] : 0, w2 = nw > 2 ? p4[2] : 0, w3 = nw > 3 ? p4[3] : 0;
                v.v[0] = ((u64)w1 << 32) | w0; v.v[1] = ((u64)w3 << 32) | w2;
            }
            break;
        }
        case RP_CONST64: v.v[0] = em_const(c.off); break;
        case RP_POW2: v.v[0] = 1ull << c.off; break;
        case RP_IN_A: v.v[0] = reinterpret_cast<const limb_t *>(a.a)[(u64)elem * a.a_stride + c.off]; break;
        case RP_IN_B: v.v[0] = reinterpret_cast<const limb_t *>(a.b)[(u64)elem * a.b_stride + c.off]; break;
        case RP_IN_N: v.v[0] = reinterpret_cast<const limb_t *>(a.n)[(u64)elem * a.n_stride + c.off]; break;
        default: break;
    }
    return v;
}

// SR rows per workgroup (= its threads), staged in SR x 160 bytes of LDS.  Next to a cells kernel that fills every CU's LDS a workgroup
// only starts where retiring cells workgroups have left SR x 160 bytes free: the smaller stage is the one that finds room.
template <int LW, u32 SR = 256>
__global__ __launch_bounds__(SR) void rowprog_kernel(RowProgArgs a) {
    using limb_t = typename LimbT<LW>::type;
    __shared__ uint4 stage[SR * (ADVICE_ROW_BYTES / 16)];
    const u32 tid = threadIdx.x;
    const u32 head = a.rows - a.tail_rows, hchunks = (head + SR - 1) / SR, nchunks = rowprog_chunks(a.rows, a.tail_rows, SR);
    const u32 item = xcd_contiguous_block(blockIdx.x, gridDim.x);
    const u32 elem = item / nchunks, ci = item - elem * nchunks;
    const bool tail = ci >= hchunks;
    const u32 r0 = tail ? head + (ci - hchunks) * SR : ci * SR, r_end = tail ? a.rows : head;
    if (a.status && a.status[elem]) return;
    const u8 *reg = a.trace + (u64)elem * a.elem_stride + a.first_off;
    const u32 r = r0 + tid;
    if (r < r_end) {
        const uint4 *pr = reinterpret_cast<const uint4 *>(a.prog + r);
        union { uint4 q[3]; RpRow row; } u;
        u.q[0] = pr[0]; u.q[1] = pr[1]; u.q[2] = pr[2];
        const RpRow &rw = u.row;
        auto fetch = [&](const RpCell &c) -> Fe { return rp_fetch<LW>(a, reg, elem, c); };
        Fe c[5];
        const bool u32r = rw.kind >= ROWK_RANGE_U32 && rw.kind < ROWK_RANGE_U32 + 2;
        if ((rw.kind >= ROWK_RANGE_LIMB && rw.kind < ROWK_RANGE_LIMB + 2) || u32r) {
            // main_gate.decompose of a limb (eight w/8-bit sub-limbs) or of a 32-bit half (eight 4-bit ones): four sub-limb
            // bytes per row (the last row reversed), column e = what remains
            // bytes behind the value in the stream -- or, for a limb of an operand (assign_integer), the limb's own w/8-bit digits
            u64 subs;
            if (rw.c[0].type == RP_STREAM) {
                const u8 *p = reg + rw.c[0].off;
                const u32 *ps = reinterpret_cast<const u32 *>(p + (u32r ? 4 : LW / 8));
                subs = ((u64)ps[1] << 32) | ps[0];
            } else {
                const u64 limb = fetch(rw.c[0]).v[0];
                subs = limb;
                if (LW != 64) { subs = 0; for (u32 k = 0; k < 8; ++k) subs |= ((limb >> (4 * k)) & 0xf) << (8 * k); }
            }
            const u32 sb = u32r ? 4 : LW / 8;
            u64 rem = 0;
            const u32 k0 = (rw.kind & 1) ? 4u : 0u;
#pragma unroll
            for (u32 k = 0; k < 8; ++k) if (k >= k0) rem += ((subs >> (8 * k)) & 0xff) << (k * sb);
            for (int q = 0; q < 5; ++q) c[q] = fe_zero();
#pragma unroll
            for (u32 q = 0; q < 4; ++q) c[q].v[0] = (subs >> (8 * (k0 ? 7 - q : q))) & 0xff;
            c[4].v[0] = rem;
        } else {
#pragma unroll
            for (int q = 0; q < 5; ++q) c[q] = fetch(rw.c[q]);
            bool need34 = false, need_inv = false;
#pragma unroll
            for (int q = 0; q < 3; ++q) { const u32 t = rw.c[q].type; need34 = need34 || t == RP_DIFF34 || t == RP_INV34; need_inv = need_inv || t == RP_INV34; }
            Fe d34 = fe_zero(), inv = fe_zero();
            if (need34) {
                d34 = fe_sub(c[3], c[4], a.f.p);
                if (need_inv) inv.v[0] = 1;   // d = 0: is_zero's witness is 1; d != 0: rowprog_inv_kernel overwrites the cell with 1/d
            }
            const Fe d01 = fe_sub(c[0], c[1], a.f.p);
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const u32 t = rw.c[q].type;
                if (t & RP_HIDDEN) c[q] = fe_zero();
                else if (t == RP_DIFF01) c[q] = d01;
                else if (t == RP_DIFF34) c[q] = d34;
                else if (t == RP_INV34) c[q] = inv;
            }
        }
        uint4 *sp = stage + (u64)tid * (ADVICE_ROW_BYTES / 16);
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            sp[2 * q] = make_uint4((u32)c[q].v[0], (u32)(c[q].v[0] >> 32), (u32)c[q].v[1], (u32)(c[q].v[1] >> 32));
            sp[2 * q + 1] = make_uint4((u32)c[q].v[2], (u32)(c[q].v[2] >> 32), (u32)c[q].v[3], (u32)(c[q].v[3] >> 32));
        }
    }
    __syncthreads();
    const u32 n_rows = r_end - r0 < SR ? r_end - r0 : SR;
    advice_flush<SR>(a.dst, a.mk, a.dst.elem(elem), r0 + (tail ? a.tail_skip : 0), n_rows, stage, tid);
}


// main_gate.is_zero's inverse witnesses, in their own launch: a Fermat inversion is ~380 Montgomery products (~0.5 ms for a
// wave), and inside rowprog_kernel the few rows that need one (d != 0: e.g. the 32 limb comparisons of is_equal_fresh(x, n) in an
// assert_in_field) are spread thinly over waves whose other lanes wait -- 5.1 ms for 1,024 RSA-2048 elements.  Here one thread
// looks at one (element, is_zero row); the rows with d != 0 are packed into a dense list in LDS, so the waves that invert are
// full, and every cell 1 = 1/d goes out as two 16-byte stores behind the image rowprog_kernel wrote.
template <int LW, u32 NT = 256>
__global__ __launch_bounds__(NT) void rowprog_inv_kernel(RowProgArgs a) {
    __shared__ u32 cnt;
    __shared__ u32 l_elem[NT], l_row[NT];
    __shared__ Fe l_d[NT];
    const u32 tid = threadIdx.x;
    if (tid == 0) cnt = 0;
    __syncthreads();
    const u64 g = (u64)blockIdx.x * NT + tid;
    if (g < a.batch * a.n_inv) {
        const u32 elem = (u32)(g / a.n_inv), r = a.inv_rows[g - (u64)elem * a.n_inv];
        if (!(a.status && a.status[elem])) {
            const RpRow *rw = a.prog + r;
            const u8 *reg = a.trace + (u64)elem * a.elem_stride + a.first_off;
            const Fe d = fe_sub(rp_fetch<LW>(a, reg, elem, rw->c[3]), rp_fetch<LW>(a, reg, elem, rw->c[4]), a.f.p);
            if (!fe_is_zero(d)) { const u32 slot = atomicAdd(&cnt, 1u); l_elem[slot] = elem; l_row[slot] = r; l_d[slot] = d; }
        }
    }
    __syncthreads();
    if (tid < cnt) {
        const Fe iv = fe_inv_fast(l_d[tid], a.f);
        advice_put_cell(a.dst, a.mk, a.dst.elem(l_elem[tid]), l_row[tid], 1, make_uint4((u32)iv.v[0], (u32)(iv.v[0] >> 32), (u32)iv.v[1], (u32)(iv.v[1] >> 32)),
                        make_uint4((u32)iv.v[2], (u32)(iv.v[2] >> 32), (u32)iv.v[3], (u32)(iv.v[3] >> 32)));
    }
}

}  // namespace h2r
