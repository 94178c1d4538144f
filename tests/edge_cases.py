"""Edge-case generator shared by the oracle and GPU tests: moduli by class, operands at the quotient-fit limit, and the status
each case must get by rule.  A plain module (not a conftest): deterministic, seeded `random.Random`, Python integers only.

Shape (w, L): bits = w * L, K = ceil(bits / 32) digits -- the chain kernels work on 32-bit digits.

Modulus classes:
  full       random, top bit set (the control)
  pow2       2^(bits-1), 2^(bits-1-s) for s in {1, 31, 32, 33, 63, 64}, 2^64, 2^32, 2: mu' at its maximum, n' with all-zero low digits
  clear_top  top bit clear: a shift inside the top digit (1..31), and whole-digit shifts 32j and 32j + 31
  tiny       1, 3, 2^31 + 1, 2^32 - 1, 2^32 + 1, 2^64 - 1, 2^64 + 1: one or two digits, the shift near 32K
  lane_edge  the top non-zero digit at a 64-lane group boundary (digit 63 / 64 / 127 / 128 where it exists; for K <= 64, the
             middle digits K/2 - 1 and K/2, where the low half of a double-width product ends)
  ones       2^bits - 1, and 2^bits - 1 with one zero limb in the middle

Status rules (values of H2R_E_* / H2RO_E_*, which are equal):
  n = 0                                   ZERO_MODULUS
  a mul_mod whose quotient a*b // n does not fit `bits` bits   NOT_REDUCED (also inside a pow chain, at the first such step)
  the in-field check (modpow_public_key) with x >= n            NOT_IN_FIELD (checked before the chain)
"""
import random

OK, ZERO_MODULUS, NOT_REDUCED, NOT_IN_FIELD = 0, 2, 3, 8

CLASSES = ("full", "pow2", "clear_top", "tiny", "lane_edge", "ones")

# every (w, L) a chain build is reached with in tests/test_chain_edge_moduli.py
SHAPES = [(64, 4), (32, 8), (64, 8), (32, 16), (64, 16), (64, 12), (32, 32), (32, 24), (64, 32), (32, 64), (64, 48), (64, 40),
          (32, 96), (64, 64), (32, 128)]

E_SPARSE = 65537
E_DENSE = 0xF7D39A5CB1E40C6B          # 64 bits, popcount 35: a "dense" fixed exponent (>= 64 bits, popcount >= bits / 4)
E_LONG = (1 << 699) | (1 << 350) | (1 << 33) | 1   # 700 bits: walked as segments on a latency-bound batch


def digits(w, L):
    return (w * L + 31) // 32


def _rand_bitlen(rng, nbits):
    """A random integer of exactly `nbits` bits (odd when nbits > 1)."""
    if nbits <= 1:
        return nbits
    return rng.getrandbits(nbits - 1) | (1 << (nbits - 1)) | 1


def moduli(w, L, seed=0):
    """[(class, n)] for the shape, every class non-empty, no duplicates within a class."""
    bits = w * L
    K = digits(w, L)
    rng = random.Random(1000003 * w + 7919 * L + seed)
    out = []

    def add(cls, n):
        if 0 < n < (1 << bits) and (cls, n) not in out:
            out.append((cls, n))

    add("full", _rand_bitlen(rng, bits))
    add("full", (rng.getrandbits(bits) | (1 << (bits - 1))) & ~1)    # even
    for s in (0, 1, 31, 32, 33, 63, 64):
        if bits - 1 - s >= 1:
            add("pow2", 1 << (bits - 1 - s))
    for p in (64, 32, 1):
        add("pow2", 1 << p)
    for s in (1, 7, 31):                                          # the shift inside the top digit
        add("clear_top", _rand_bitlen(rng, bits - s))
    for j in sorted({1, 2, max(1, K // 2)}):                     # whole-digit shifts 32j and 32j + 31
        for s in (32 * j, 32 * j + 31):
            if bits - s >= 2:
                add("clear_top", _rand_bitlen(rng, bits - s))
    for n in (1, 3, (1 << 31) + 1, (1 << 32) - 1, (1 << 32) + 1, (1 << 64) - 1, (1 << 64) + 1):
        add("tiny", n)
    edges = [d for d in (63, 64, 127, 128) if d < K] if K > 64 else [K // 2 - 1, K // 2]
    for d in edges:
        add("lane_edge", _rand_bitlen(rng, 32 * d + 32))             # digit d full
        add("lane_edge", (1 << (32 * d)) | rng.getrandbits(32 * d) | 1)   # digit d == 1
    full = (1 << bits) - 1
    add("ones", full)
    add("ones", full ^ (((1 << w) - 1) << (w * (L // 2))))
    return out


def by_class(mods):
    d = {c: [] for c in CLASSES}
    for c, n in mods:
        d[c].append(n)
    return d


# ---- rules ---------------------------------------------------------------------------------------------------------------
def mul_mod_expect(a, b, n, bits):
    """(status, a*b mod n or None)."""
    if n == 0:
        return ZERO_MODULUS, None
    if (a * b) // n >> bits:
        return NOT_REDUCED, None
    return OK, (a * b) % n


def fit_limit(n, b, bits):
    """The largest a < 2^bits with a*b // n < 2^bits (None when every a < 2^bits fits)."""
    a = ((n << bits) - 1) // b
    return a if a < (1 << bits) - 1 else None


def pow_fixed_expect(x, e, n, bits, in_field=False):
    """BigIntChip::pow_mod_fixed_exp (LSB first: square, then multiply acc by the pre-square value on a set bit), each
    step under the mul_mod rule; with in_field, RSAChip::modpow_public_key's assert_in_field first."""
    if n == 0:
        return ZERO_MODULUS, None
    if in_field and x >= n:
        return NOT_IN_FIELD, None
    sq, acc = x, 1
    for i in range(int(e).bit_length()):
        cur = sq
        st, sq = mul_mod_expect(cur, cur, n, bits)
        if st:
            return st, None
        if (e >> i) & 1:
            st, acc = mul_mod_expect(acc, cur, n, bits)
            if st:
                return st, None
    return OK, acc


def pow_var_expect(x, e_limbs, exp_limb_bits, n, bits, in_field=False):
    """BigIntChip::pow_mod: per bit, acc * squared (selected on the bit), then the squaring."""
    if n == 0:
        return ZERO_MODULUS, None
    if in_field and x >= n:
        return NOT_IN_FIELD, None
    sq, acc = x, 1
    for limb in e_limbs:
        for t in range(exp_limb_bits):
            st, m = mul_mod_expect(acc, sq, n, bits)
            if st:
                return st, None
            if (limb >> t) & 1:
                acc = m
            st, sq = mul_mod_expect(sq, sq, n, bits)
            if st:
                return st, None
    return OK, acc


def in_field_expect(x, n):
    return OK if x < n else NOT_IN_FIELD


# ---- cases ---------------------------------------------------------------------------------------------------------------
def mul_mod_cases(w, L, seed=0):
    """[(class, tag, a, b, n)] for every modulus of the shape.  Tags: "zero", "one", "n-1", "n*1" (unreduced a == n), "limit"
    (the largest a whose quotient fits, for a b > n), "limit+1" (one above: NOT_REDUCED), "max" (2^bits - 1), "rand"."""
    bits = w * L
    full = (1 << bits) - 1
    rng = random.Random(31 * w + L + 17 * seed)
    out = []
    for cls, n in moduli(w, L, seed):
        out.append((cls, "zero", 0, rng.randrange(n), n))
        out.append((cls, "one", 1, n - 1, n))
        out.append((cls, "n-1", n - 1, n - 1, n))
        out.append((cls, "n*1", n, 1, n))
        out.append((cls, "max", full, 1, n))
        out.append((cls, "max", full, full, n))
        out.append((cls, "rand", rng.randrange(n), rng.randrange(n), n))
        for b in (full, rng.randrange(n + 1, full + 1) if n < full else None):
            if b is None or b <= n:
                continue
            a = fit_limit(n, b, bits)
            if a is not None:
                out.append((cls, "limit", a, b, n))
                out.append((cls, "limit+1", a + 1, b, n))
    return out


def pow_cases(w, L, seed=0, lean=False):
    """[(class, tag, x, n)].  Every modulus with x = n - 1 and a random x; the first modulus of each class also with 0, 1,
    n (unreduced) and 2^bits - 1.  lean: the first and last modulus of each class only (long chains, wide shapes)."""
    bits = w * L
    full = (1 << bits) - 1
    rng = random.Random(97 * w + L + 13 * seed)
    out = []
    for cls, ns in by_class(moduli(w, L, seed)).items():
        picked = sorted({0, len(ns) - 1}) if lean else range(len(ns))
        for k in picked:
            n = ns[k]
            out.append((cls, "n-1", n - 1, n))
            out.append((cls, "rand", rng.randrange(n), n))
            if k == 0:
                out += [(cls, "n", n, n), (cls, "max", full, n)]
                if not lean:
                    out += [(cls, "zero", 0, n), (cls, "one", 1, n)]
    return out


def filler(w, L, count, seed=0):
    """`count` random full-size (x / a, b, n) triples, all with status 0 -- the neighbours of the edge elements."""
    bits = w * L
    rng = random.Random(4099 * w + L + seed)
    out = []
    for _ in range(count):
        n = _rand_bitlen(rng, bits)
        out.append((rng.randrange(n), rng.randrange(n), n))
    return out


def in_field_offsets(w, L):
    """j with x = n +- 2^(w*j): a borrow / carry run of j limbs decides the comparison (j in 1, 63, 64, L - 1 where j < L)."""
    return sorted({j for j in (1, 63, 64, L - 1) if 0 < j < L})


def fresh_carry_cases(w, L, seed=0):
    """[(tag, a, b, n)] for the Fresh family and assert_in_field: propagate runs of the carry / borrow / compare chains."""
    bits = w * L
    full = (1 << bits) - 1
    mask = (1 << w) - 1
    rng = random.Random(7 * w + L + seed)
    n = _rand_bitlen(rng, bits)
    out = [("carry-all", full, 1, n), ("carry-all-rev", 1, full, n)]
    for j in in_field_offsets(w, L):
        out.append(("borrow-run-%d" % j, 1 << (w * j), 1, n))                 # a - b: a borrow through j limbs
        out.append(("borrow-run-rev-%d" % j, 1, 1 << (w * j), n))
    for j in sorted({0, 63, 64, L - 1} & set(range(L))):
        base = rng.getrandbits(bits)
        a = base | (1 << (w * j))
        b = a ^ (1 << (w * j))                                               # equal but for limb j: a > b decided there
        out.append(("differ-limb-%d" % j, a, b, n))
        out.append(("differ-limb-rev-%d" % j, b, a, n))
    # a + b == n with every limb sum == MASK: n = 2^bits - 1 (mod) with a's limbs arbitrary
    n_ones = full
    a = rng.getrandbits(bits) & full
    out.append(("sum-is-n-mask", a, n_ones - a, n_ones))
    # with a general n: limb sums all MASK except where n's limbs differ -- use n - a directly as well
    a = rng.randrange(n)
    out.append(("sum-is-n", a, n - a, n))
    # sub_mod with a < b and a long borrow run: every limb of a below the top one is zero
    out.append(("sub-borrow-long", 1, n - 1, n))
    top = 1 << (w * (L - 1))
    out.append(("sub-borrow-long2", top, top + 1, n))
    return out
