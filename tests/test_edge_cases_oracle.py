"""The C oracle on the edge cases of tests/edge_cases.py (CPU only): for every shape a chain build is reached with, the oracle's status
equals the rule and its values equal Python integers -- mul_mod, pow_mod_fixed_exp (sparse and dense e), pow_mod (one and several
exponent limbs) and assert_in_field.  The GPU module tests/test_chain_edge_moduli.py compares the kernels with this oracle."""
import numpy as np
import pytest

import edge_cases as E
from oracle_lib import Oracle

VAR_E1 = ([17], 5)                          # RSAChip's one 5-bit limb
VAR_EM = ([0x1A2B3, 0x5, 0x1FFFF], 17)      # three 17-bit limbs, one nearly empty


def test_generator_classes_and_rules():
    """Every class is non-empty for every shape, the cases are deterministic, and the fit-limit pair straddles the rule."""
    for w, L in E.SHAPES:
        bits = w * L
        mods = E.moduli(w, L)
        assert mods == E.moduli(w, L)
        cls = E.by_class(mods)
        assert all(cls[c] for c in E.CLASSES), (w, L, {c: len(v) for c, v in cls.items()})
        assert all(0 < n < (1 << bits) for _c, n in mods)
        assert all(n.bit_length() < bits for n in cls["clear_top"])
        assert all(n & (n - 1) == 0 for n in cls["pow2"])
        K = E.digits(w, L)
        tops = {(n.bit_length() - 1) // 32 for n in cls["lane_edge"]}
        assert tops == set([d for d in (63, 64, 127, 128) if d < K] if K > 64 else [K // 2 - 1, K // 2]), (w, L, tops)
        mm = E.mul_mod_cases(w, L)
        assert mm == E.mul_mod_cases(w, L)
        tags = {}
        for c, tag, a, b, n in mm:
            assert 0 <= a < (1 << bits) and 0 <= b < (1 << bits)
            tags.setdefault(tag, []).append(E.mul_mod_expect(a, b, n, bits)[0])
        assert set(tags["limit"]) == {E.OK} and set(tags["limit+1"]) == {E.NOT_REDUCED}
        assert set(tags["n*1"]) == {E.OK}
        for c in E.CLASSES:
            assert any(t[0] == c and t[1] == "rand" for t in mm)
            assert any(t[0] == c for t in E.pow_cases(w, L, lean=True))
    assert E.mul_mod_expect(3, 4, 0, 64) == (E.ZERO_MODULUS, None)
    assert E.pow_fixed_expect(5, 3, 7, 64, in_field=False) == (0, pow(5, 3, 7))
    assert E.pow_fixed_expect(9, 3, 7, 64, in_field=True)[0] == E.NOT_IN_FIELD


def _lean(w, L):
    return w * L >= 3072


@pytest.mark.parametrize("w,L", E.SHAPES)
def test_oracle_mul_mod_edge_cases(w, L):
    o = Oracle(w, L)
    bits = w * L
    for c, tag, a, b, n in E.mul_mod_cases(w, L) + [("zero-n", "zero-n", 3, 4, 0)]:
        st, val = E.mul_mod_expect(a, b, n, bits)
        rc, r, _ = o.mul_mod(o.limbs(a), o.limbs(b), o.limbs(n), want_stream=False)
        assert rc == st, (w, L, c, tag, hex(n))
        if st == 0:
            assert o.to_int(r) == val, (w, L, c, tag, hex(n))


@pytest.mark.parametrize("w,L", E.SHAPES)
def test_oracle_pow_edge_cases(w, L):
    o = Oracle(w, L)
    bits = w * L
    for e, lean in ((E.E_SPARSE, _lean(w, L)), (E.E_DENSE, True)):
        for c, tag, x, n in E.pow_cases(w, L, lean=lean):
            st, val = E.pow_fixed_expect(x, e, n, bits)
            rc, out, _ = o.pow_mod_fixed_exp(o.limbs(x), o.limbs(n), e, want_stream=False)
            assert rc == st, (w, L, e, c, tag, hex(n))
            if st == 0:
                assert o.to_int(out) == val == pow(x, e, n), (w, L, e, c, tag, hex(n))
    for (limbs, eb), lean in ((VAR_E1, _lean(w, L)), (VAR_EM, True)):
        e_int = sum(v << (eb * k) for k, v in enumerate(limbs))
        for c, tag, x, n in E.pow_cases(w, L, lean=lean):
            st, val = E.pow_var_expect(x, limbs, eb, n, bits)
            rc, out, _ = o.pow_mod(o.limbs(x), np.array(limbs, dtype=o.dtype), eb, o.limbs(n), want_stream=False)
            assert rc == st, (w, L, limbs, c, tag, hex(n))
            if st == 0:
                assert o.to_int(out) == val == pow(x, e_int, n), (w, L, limbs, c, tag, hex(n))


@pytest.mark.parametrize("w,L", E.SHAPES)
def test_oracle_assert_in_field_edge_cases(w, L):
    o = Oracle(w, L)
    cases = [(x, n) for _c, _t, x, n in E.pow_cases(w, L)]
    for j in E.in_field_offsets(w, L):
        for _c, n in E.moduli(w, L):
            for x in (n + (1 << (w * j)), n - (1 << (w * j))):
                if 0 <= x < (1 << (w * L)):
                    cases.append((x, n))
    for x, n in cases:
        rc, lt, _ = o.assert_in_field(o.limbs(x), o.limbs(n))
        assert rc == E.in_field_expect(x, n) and lt == int(x < n), (w, L, hex(x), hex(n))
