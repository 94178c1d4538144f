"""The word-level model of the field helpers (tests/fe_words_ref.py), its mutants and its operand sets; no GPU.

1. With no switch set the model equals Python big integers on every operand set, in all four fields.
2. The kill condition: for every mutant (one carry, borrow or equality term of csrc/h2r_field.hpp dropped) the operand set holds an input on
   which the mutant's result differs from the true one -- per field, on exactly the inputs the device routes of tests/test_fe_device_gpu.py
   send.  UNKILLED lists the mutants no input can kill, each with the bound that makes its term unreachable; the test also checks that
   those terms fire on no input of the set.  No mutant is in the class "no input found".
3. The rare terms, word by word: the equal word under a borrow and the all-ones word under a carry are killed at every word where they
   can change a result.
4. The same sets through h2r_field_eval ops 0 .. 5 on a host-only ctx: the host twin of the helpers is pinned on the set the device twin is."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fe_words_ref as FW

# Mutants that no input kills: site -> why its term never fires.  All of them are of the class "unreachable" (p < 2^255, operands < p).
_CIOS = ("after every row of the CIOS loop the accumulator t[0..4] is below 2 p < 2^256 (row i adds a * b[i] + m * p < 2^64 * 2 p to an accumulator "
         "below 2 p and divides by 2^64), so t[4] is 0 after a reduction row and at most one word before it")
UNKILLED = {
    "mul.t5": "unreachable: " + _CIOS + "; t[4] is 0 going into a product row, so t[4] + c never wraps and t[5] stays 0",
    "mul.c2": "unreachable: " + _CIOS + "; the reduced accumulator fits four words, so the reduction row's t[4] + c never wraps",
    "mul.t4": "unreachable: " + _CIOS + "; the result in front of the final subtraction is below 2^256, t[4] == 0",
    "mul.ge_eq": "unreachable: the unreduced result T is a * b * R^-1 (mod p); T == p needs p | a * b, that is a == 0 or b == 0, and then every "
                 "m is 0 and T == 0",
    "inv.half.top": "unreachable: half_mod adds p to x < p < 2^255, the sum is below 2^256 and nothing leaves the fourth word",
}
# the rare terms and the words at which they can change a result (word 0 has nothing entering it; what leaves word 3 is dropped or cannot
# be: a + b < 2^256, s >= p and T >= p keep the top word's borrow at zero, x + p keeps the top word below 2^64 - 1)
RARE = {"add.c2": (1, 2), "add.b2": (1, 2), "sub.b2": (1, 2, 3), "sub.c2": (1, 2), "mul.b2": (1, 2), "inv.sub256.b2": (1, 2), "inv.half.c2": (1, 2)}


@pytest.mark.parametrize("field", FW.FIELDS)
def test_unmutated_model_equals_big_integers(field):
    f = FW.field(field)
    P = f.P
    sets = FW.kill_sets(field)
    for op, inputs in sets.items():
        for args in inputs:
            assert FW.evaluate(op, f, args) == FW.truth(op, f, args), (field, op, args)
    for args in sets["inv"] + sets["inv_word"] + [(P - w,) for w, in sets["inv_word"]]:
        assert FW.evaluate("inv_fast", f, args) == pow(args[0], -1, P), (field, "inv_fast", args)
    # the conversions and the constants the routes rely on
    for _, v in FW.thinned_values(field):
        assert FW.value(FW.PLAIN.to_mont(FW.words(v), f)) == v * f.R % P and FW.value(FW.PLAIN.from_mont(FW.words(v), f)) == v * f.Rinv % P
    assert (f.n0inv * f.p[0] + 1) % (1 << 64) == 0


@pytest.mark.parametrize("field", FW.FIELDS)
def test_operand_sets(field):
    """Canonical, distinct, of the promised size; the sets are the same at every call (built once, deterministic)."""
    P = FW.FIELD_MODULI[field]
    thin, mult = FW.thinned_values(field), FW.multipliers(field)
    assert 100 <= len(thin) <= 400 and 2 <= len(mult) <= 64
    assert {1, FW.field(field).R} <= {y for _, y in mult}
    for named in (thin, mult, FW.inv_inputs(field)):
        vals = [v for _, v in named]
        assert all(0 <= v < P for v in vals) and len(set(vals)) == len(vals)
    assert all(v for _, v in FW.inv_inputs(field))
    assert all(0 <= a < P and 0 <= b < P for _, (a, b) in FW.addsub_pairs(field) + FW.mul_pairs(field))
    assert len(FW.mul_pairs(field)) == len(thin) * len(mult) + len(FW.searched_mul_pairs(field))
    base = {v for _, v in FW.base_values(FW.field(field))}
    assert {v for _, v in thin} <= base
    FW._CACHE.pop(("thin", field))
    assert FW.thinned_values(field) == thin
    print("%s: |W| %d, thinned %d, multipliers %d, product pairs %d (%d searched), add/sub pairs %d, inversion inputs %d (%d searched), words %d"
          % (field, len(base), len(thin), len(mult), len(FW.mul_pairs(field)), len(FW.searched_mul_pairs(field)), len(FW.addsub_pairs(field)),
             len(FW.inv_inputs(field)), len(FW.searched_inv_inputs(field)), len(FW.inv_words(field))))


@pytest.mark.parametrize("field", FW.FIELDS)
def test_kill_condition(field):
    assert set(UNKILLED) < set(FW.SITES)
    killed = []
    index = FW.fired_index(field)
    for site in FW.SITES:
        k = FW.killer(field, site)
        if site in UNKILLED:
            assert UNKILLED[site].startswith("unreachable: ")
            assert k is None and not any(inst[0] == site for idx in index.values() for inst in idx), (field, site, "listed as unreachable, yet it fires")
            continue
        assert k is not None, (field, site, FW.SITES[site])
        op, args = k
        assert FW.evaluate(op, FW.field(field), args, drop=(site,)) != FW.truth(op, FW.field(field), args)
        killed.append(site)
    assert len(killed) == len(FW.SITES) - len(UNKILLED) == 20
    print("%s: %d of %d mutants killed, %d unreachable" % (field, len(killed), len(FW.SITES), len(UNKILLED)))


@pytest.mark.parametrize("field", FW.FIELDS)
def test_rare_terms_are_killed_at_every_word(field):
    for site, ks in RARE.items():
        for k in ks:
            assert FW.killer(field, site, instance=k) is not None, (field, site, k)
    # mac inside fe_mont_mul, product by product: phase "a" is the row a * b[i], "r" the row m * p.  c1 needs t != 0 (nothing is accumulated
    # yet in row 0 of phase "a") and lo != 0 (a zero word of p: pasta's p[2]); c2 needs a carry word coming in (none at column 0).
    p = FW.field(field).p
    for ph in "ar":
        for i in range(4):
            for j in range(4):
                if not (ph == "a" and i == 0) and not (ph == "r" and p[j] == 0):
                    assert FW.killer(field, "mac.c1", instance=(ph, i, j)) is not None, (field, "mac.c1", ph, i, j)
                if j:
                    assert FW.killer(field, "mac.c2", instance=(ph, i, j)) is not None, (field, "mac.c2", ph, i, j)


@pytest.mark.parametrize("field", FW.FIELDS)
def test_searched_operands_hit_what_they_were_searched_for(field):
    f = FW.field(field)
    for _, (x, y) in FW.searched_mul_pairs(field):
        xw, t4 = FW.PLAIN.mont_mul_unreduced(FW.words(x), FW.words(y), f)
        assert t4 == 0 and FW.value(xw) >= f.P and any(s == "mul.b2" for s, _ in FW.fired_by("mul", f, (x, y)))
    hits = set()
    for _, u in FW.searched_inv_inputs(field):
        got = {i for i in FW.fired_by("inv", f, (u,)) if i[0] in ("inv.sub256.b2", "inv.half.c2")}
        assert got, (field, u)
        hits |= got
    assert {("inv.sub256.b2", 1), ("inv.sub256.b2", 2), ("inv.half.c2", 1), ("inv.half.c2", 2)} <= hits
    assert f.p[1] * (1 << 64) + f.p[0] + 2 in [u for _, u in FW.searched_inv_inputs(field)]


@pytest.mark.parametrize("field", FW.FIELDS)
def test_host_twin_on_the_same_sets(field):
    """h2r_field_eval on a host-only ctx.  Ops 0 / 1: the add / sub pairs as they are.  Op 2 is the canonical product
    fe_mont_mul(fe_to_mont(a), b): a = x * R^-1 puts the pair (x, y) itself into the second fe_mont_mul.  Ops 3 / 4 / 5: the inversion inputs
    (5 also on the one-word inputs s and p - s, which take fe_inv_word)."""
    from halo2_rsa_amd import _lib
    from halo2_rsa_amd._lib import H2RParams, lib
    f = FW.field(field)
    P = f.P
    ctx = ctypes.c_void_p()
    prm = H2RParams(64, 2048, _lib.FIELDS[field], -1)
    assert lib().h2r_ctx_create(ctypes.byref(prm), ctypes.byref(ctx)) == 0
    out = (ctypes.c_uint64 * 4)()
    fe = lambda v: (ctypes.c_uint64 * 4)(*FW.words(v))
    ev = lambda op, a, b=None: (lib().h2r_field_eval(ctx, op, fe(a), None if b is None else fe(b), out), FW.value([int(w) for w in out]))
    try:
        for name, (a, b) in FW.addsub_pairs(field):
            assert ev(0, a, b) == (0, (a + b) % P), (field, "add", name)
            assert ev(1, a, b) == (0, (a - b) % P), (field, "sub", name)
            assert ev(1, b, a) == (0, (b - a) % P), (field, "sub'", name)
        for name, (x, y) in FW.mul_pairs(field):
            assert ev(2, x * f.Rinv % P, y) == (0, x * y * f.Rinv % P), (field, "mul", name)
        for name, a in FW.inv_inputs(field):
            want = pow(a, -1, P)
            assert ev(3, a) == (0, want) and ev(4, a) == (0, want) and ev(5, a) == (0, want), (field, "inv", name)
        for s in FW.inv_words(field):
            assert ev(5, s) == (0, pow(s, -1, P)) and ev(5, P - s) == (0, pow(P - s, -1, P)), (field, "inv_word", s)
    finally:
        lib().h2r_ctx_destroy(ctx)
