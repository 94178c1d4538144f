"""Word-level model of the field helpers of csrc/h2r_field.hpp (fe_add, fe_sub, mac, fe_mont_mul, ge_p, fe_inv with its half_mod / sub256 /
shr1, fe_inv_word, fe_inv_fast), its single-term mutants, and the operand sets that pin the helpers on word-boundary operands.

The model is a restatement of the header term by term on four 64-bit words (the section on the field helpers); with no switch set
it equals Python big integers: (a +- b) % p, a * b * R^-1 % p, pow(a, -1, p).  Every carry, borrow and equality term of the header is a
SITE with a name (SITES below).  A `Run` carries two things through an evaluation:
    drop    the sites that are switched off: a name drops the term wherever the (unrolled) source has it, a pair (name, index) drops one
            instance of it (index = the word, or for `mac` the (phase, row, column) of the product it belongs to)
    fired   None, or a set that collects every instance (name, index) whose term was 1 (resp. whose equality held) in this evaluation.
            A term that never fires cannot be told from its absence, so `fired` is what the thinning and the searches below work from; the
            kill condition itself (tests/test_fe_words_model.py) is always checked by evaluating the mutant.

Operand sets, per field (bn254 Fr / Fq, pasta Fp / Fq), all deterministic:
    base_values      W: small values, p - small, (p +- 1) / 2, 2^k + {-1, 0, 1}, p - 2^k + {-1, 0, 1}, one word equal to p's word (+- 1) among
                     zero / all-ones words, the 16 patterns of all-ones and zero words; and v * R, v * R^-1 of each of them
    thinned_values   W thinned greedily (see there)
    multipliers      at most 64 second operands of fe_mont_mul
    mul_pairs        thinned_values x multipliers and the searched pairs of searched_mul_pairs (the final subtraction's equal word under a borrow)
    addsub_pairs     pairs (a, b) for fe_add / fe_sub: a + b = p - 1, p, p + 1, ..., a - b = 0, -1, equal words under a borrow, all-ones
                     words under a carry
    inv_inputs       thinned_values without 0, and the inputs of searched_inv_inputs: sub256 through an equal word under a borrow in the
                     first round, half_mod through an all-ones word under a carry
    inv_words        one-word inputs of fe_inv_word
Everything here is Python integers; nothing touches the library or a GPU."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
from pyref import FIELD_MODULI

M64 = (1 << 64) - 1
R256 = 1 << 256
FIELDS = ("bn254_fr", "bn254_fq", "pasta_fp", "pasta_fq")

# name -> what the term is in the header.  The groups: fe_add, fe_sub, mac, fe_mont_mul, fe_inv (its lambdas), fe_inv_word.
SITES = {
    "add.c1": "fe_add, the sum: c1 = t < a[k], the carry of a[k] + b[k]",
    "add.c2": "fe_add, the sum: u < t, the carry of an all-ones word that a carry enters",
    "add.ge_eq": "fe_add: ge_p true on s == p",
    "add.b1": "fe_add, s - p: b1 = s[k] < p[k]",
    "add.b2": "fe_add, s - p: t < br, the borrow that enters a word with s[k] == p[k]",
    "sub.b1": "fe_sub, a - b: b1 = a[k] < b[k]",
    "sub.b2": "fe_sub, a - b: t < br, the borrow that enters a word with a[k] == b[k]",
    "sub.c1": "fe_sub, + p: c1 = t < r[k]",
    "sub.c2": "fe_sub, + p: u < t, the carry that enters a word with r[k] + p[k] == 2^64 - 1",
    "mac.c1": "mac: c1 = s1 < t, the carry of t + lo",
    "mac.c2": "mac: c2 = s2 < s1, the carry of (t + lo) + c",
    "mul.t5": "fe_mont_mul: t[5] = s < t[4], the product row's carry out of t[4]",
    "mul.c2": "fe_mont_mul: c2 = s2 < t[4], the reduction row's carry into t[4]",
    "mul.t4": "fe_mont_mul: the `t[4] ||` in front of the final subtraction",
    "mul.ge_eq": "fe_mont_mul: ge_p true on x == p",
    "mul.b1": "fe_mont_mul, x - p: b1 = x[k] < p[k]",
    "mul.b2": "fe_mont_mul, x - p: u < br, the borrow that enters a word with x[k] == p[k]",
    "inv.half.c1": "fe_inv, half_mod: c1 = t < x[k] of x + p",
    "inv.half.c2": "fe_inv, half_mod: w < t of x + p",
    "inv.half.top": "fe_inv, half_mod: the carry out of 256 bits that shr1 shifts in",
    "inv.sub256.b1": "fe_inv, sub256: b1 = x[k] < y[k]",
    "inv.sub256.b2": "fe_inv, sub256: t < br, the borrow that enters a word with x[k] == y[k]",
    "inv.shr1.x": "fe_inv, shr1: the bit that crosses from word k + 1 into word k",
    "invw.top": "fe_inv_word, the restoring division: `top ||`, the remainder's bit that left the word",
    "invw.ge_eq": "fe_inv_word, the restoring division: rc >= s true on rc == s",
}


def words(v):
    return [(v >> (64 * k)) & M64 for k in range(4)]


def value(w):
    return w[0] | w[1] << 64 | w[2] << 128 | w[3] << 192


class Field:
    """FieldConsts of the header, from big integers."""

    def __init__(self, name):
        self.name, self.P = name, FIELD_MODULI[name]
        P = self.P
        self.p = words(P)
        self.n0inv = (-pow(P, -1, 1 << 64)) & M64
        self.R = R256 % P
        self.Rinv = pow(R256, -1, P)
        self.one, self.r2 = words(self.R), words(R256 * R256 % P)


_FIELDS = {}


def field(name):
    if name not in _FIELDS:
        _FIELDS[name] = Field(name)
    return _FIELDS[name]


class Run:
    """One evaluation context of the model: which sites are dropped, and (optionally) which fired."""

    def __init__(self, drop=(), fired=None):
        self.drop, self.fired = frozenset(drop), fired

    def term(self, name, idx, cond):
        """The term `cond` of site `name`, instance `idx`: 1 when it holds and is not dropped."""
        if not cond:
            return 0
        if self.fired is not None:
            self.fired.add((name, idx))
        if name in self.drop or (name, idx) in self.drop:
            return 0
        return 1

    # ---- ge_p, fe_lt ----
    def ge_p(self, x, p, site):
        for k in (3, 2, 1, 0):
            if x[k] != p[k]:
                return x[k] > p[k]
        return bool(self.term(site, None, True))

    @staticmethod
    def lt(a, b):
        for k in (3, 2, 1, 0):
            if a[k] != b[k]:
                return a[k] < b[k]
        return False

    # ---- the two chains every helper is made of ----
    def _add4(self, a, b, c1_site, c2_site):
        """a + b over four words; (words, carry out)."""
        s, cy = [0] * 4, 0
        for k in range(4):
            t = (a[k] + b[k]) & M64
            c1 = self.term(c1_site, k, t < a[k])
            u = (t + cy) & M64
            cy = c1 | self.term(c2_site, k, u < t)
            s[k] = u
        return s, cy

    def _sub4(self, a, b, b1_site, b2_site):
        """a - b over four words; (words, borrow out)."""
        r, br = [0] * 4, 0
        for k in range(4):
            t = (a[k] - b[k]) & M64
            b1 = self.term(b1_site, k, a[k] < b[k])
            u = (t - br) & M64
            br = b1 | self.term(b2_site, k, t < br)
            r[k] = u
        return r, br

    # ---- fe_add, fe_sub ----
    def add(self, a, b, f):
        s, _ = self._add4(a, b, "add.c1", "add.c2")
        if self.ge_p(s, f.p, "add.ge_eq"):
            return self._sub4(s, f.p, "add.b1", "add.b2")[0]
        return s

    def sub(self, a, b, f):
        r, br = self._sub4(a, b, "sub.b1", "sub.b2")
        if br:
            r, _ = self._add4(r, f.p, "sub.c1", "sub.c2")
        return r

    # ---- mac, fe_mont_mul ----
    def mac(self, t, a, b, c, idx):
        """t + a * b + c: (low word, high word)."""
        prod = a * b
        lo, hi = prod & M64, prod >> 64
        s1 = (t + lo) & M64
        c1 = self.term("mac.c1", idx, s1 < t)
        s2 = (s1 + c) & M64
        c2 = self.term("mac.c2", idx, s2 < s1)
        return s2, (hi + c1 + c2) & M64

    def mont_mul_unreduced(self, a, b, f):
        """The CIOS accumulator in front of the final subtraction: (x[4], t[4])."""
        t = [0] * 6
        for i in range(4):
            c = 0
            for j in range(4):
                t[j], c = self.mac(t[j], a[j], b[i], c, ("a", i, j))
            s = (t[4] + c) & M64
            t[5] = self.term("mul.t5", i, s < t[4])
            t[4] = s
            m = (t[0] * f.n0inv) & M64
            _, c = self.mac(t[0], m, f.p[0], 0, ("r", i, 0))
            for j in range(1, 4):
                t[j], c = self.mac(t[j], m, f.p[j], c, ("r", i, j))
                t[j - 1] = t[j]
            s2 = (t[4] + c) & M64
            c2 = self.term("mul.c2", i, s2 < t[4])
            t[3], t[4], t[5] = s2, t[5] + c2, 0
        return t[:4], t[4]

    def mont_mul(self, a, b, f):
        x, t4 = self.mont_mul_unreduced(a, b, f)
        if self.term("mul.t4", None, t4 != 0) or self.ge_p(x, f.p, "mul.ge_eq"):
            return self._sub4(x, f.p, "mul.b1", "mul.b2")[0]
        return x

    def to_mont(self, a, f):
        return self.mont_mul(a, f.r2, f)

    def from_mont(self, a, f):
        return self.mont_mul(a, [1, 0, 0, 0], f)

    # ---- fe_inv ----
    def shr1(self, x, top):
        n = x[1:] + [top]
        return [(x[k] >> 1) | ((n[k] << 63) & M64 if k == 3 or self.term("inv.shr1.x", k, n[k] & 1) else 0) for k in range(4)]

    def half_mod(self, x, f):
        cy = 0
        if x[0] & 1:
            x, cy = self._add4(x, f.p, "inv.half.c1", "inv.half.c2")
            cy = self.term("inv.half.top", None, cy)
        return self.shr1(x, cy)

    def inv(self, a, f, max_rounds=1024):
        u, v, x1, x2 = list(a), list(f.p), [1, 0, 0, 0], [0, 0, 0, 0]
        one = [1, 0, 0, 0]
        rounds = 0
        while rounds < max_rounds and u != one and v != one:
            if (u[0] & 1) and (v[0] & 1):
                if self.lt(u, v):
                    v = self._sub4(v, u, "inv.sub256.b1", "inv.sub256.b2")[0]
                    x2 = self.sub(x2, x1, f)
                else:
                    u = self._sub4(u, v, "inv.sub256.b1", "inv.sub256.b2")[0]
                    x1 = self.sub(x1, x2, f)
            if not u[0] & 1:
                u = self.shr1(u, 0)
                x1 = self.half_mod(x1, f)
            else:
                v = self.shr1(v, 0)
                x2 = self.half_mod(x2, f)
            rounds += 1
        return x1 if u == one else x2

    # ---- fe_inv_word, fe_inv_fast ----
    def inv_word(self, s, f):
        tc, tp = [0, 0, 0, 0], [1, 0, 0, 0]
        rc, rp = 0, s
        for bit in range(255, -1, -1):
            top = rc >> 63
            rc = ((rc << 1) & M64) | ((f.p[bit >> 6] >> (bit & 63)) & 1)
            if self.term("invw.top", None, top) or rc > s or (rc == s and self.term("invw.ge_eq", None, True)):
                rc = (rc - s) & M64
                tc[bit >> 6] |= 1 << (bit & 63)
        neg = True
        while rc > 1:
            q, rn = rp // rc, rp % rc
            c, tn = 0, [0] * 4
            for k in range(4):
                tn[k], c = self.mac(tp[k], q, tc[k], c, ("w", k))
            tp, tc = tc, tn
            rp, rc, neg = rc, rn, not neg
        return self.sub([0, 0, 0, 0], tc, f) if neg else tc

    def inv_fast(self, a, f):
        if not (a[1] | a[2] | a[3]):
            return list(a) if a[0] == 1 else self.inv_word(a[0], f)
        na = self.sub([0, 0, 0, 0], a, f)
        if not (na[1] | na[2] | na[3]):
            return list(a) if na[0] == 1 else self.sub([0, 0, 0, 0], self.inv_word(na[0], f), f)
        return self.inv(a, f)


PLAIN = Run()

# what an operation of the kill condition is: name -> (the model's call on integers, the true result on integers)
OPS = {
    "add": (lambda run, f, a, b: value(run.add(words(a), words(b), f)), lambda f, a, b: (a + b) % f.P),
    "sub": (lambda run, f, a, b: value(run.sub(words(a), words(b), f)), lambda f, a, b: (a - b) % f.P),
    "mul": (lambda run, f, a, b: value(run.mont_mul(words(a), words(b), f)), lambda f, a, b: a * b * f.Rinv % f.P),
    "inv": (lambda run, f, a: value(run.inv(words(a), f)), lambda f, a: pow(a, -1, f.P)),
    "inv_word": (lambda run, f, a: value(run.inv_word(a, f)), lambda f, a: pow(a, -1, f.P)),
    "inv_fast": (lambda run, f, a: value(run.inv_fast(words(a), f)), lambda f, a: pow(a, -1, f.P)),
}


def evaluate(op, f, args, drop=(), fired=None):
    return OPS[op][0](Run(drop, fired), f, *args)


def truth(op, f, args):
    return OPS[op][1](f, *args)


def fired_by(op, f, args):
    s = set()
    evaluate(op, f, args, fired=s)
    return s


# ---- the base set W -------------------------------------------------------------------------------------------------------------------
def _dedupe(named):
    seen, out = set(), []
    for name, v in named:
        if v not in seen:
            seen.add(v)
            out.append((name, v))
    return out


BOUNDARY_BITS = (31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 253)   # 2^k with k next to a 32-bit or 64-bit digit boundary


def core_values(f):
    """The values every thinned set keeps: the small ones, the 16 word patterns, one word of p (+- 1) among zero / all-ones words, and
    2^k, p - 2^k (+- 1) for the k of BOUNDARY_BITS."""
    P, p = f.P, f.p
    named = [("0", 0), ("1", 1), ("2", 2), ("3", 3), ("p-1", P - 1), ("p-2", P - 2), ("(p-1)/2", (P - 1) // 2), ("(p+1)/2", (P + 1) // 2)]
    for mask in range(16):
        named.append(("ones%x" % mask, sum(M64 << (64 * k) for k in range(4) if (mask >> k) & 1) % P))
    for j in range(4):
        for d in (-1, 0, 1):
            for fill, fname in ((0, "z"), (M64, "f")):
                v = sum(fill << (64 * k) for k in range(4) if k != j) | ((p[j] + d) & M64) << (64 * j)
                named.append(("pw%d%+d%s" % (j, d, fname), v % P))
    for k in BOUNDARY_BITS:
        for d in (-1, 0, 1):
            named += [("2^%d%+d" % (k, d), (1 << k) + d), ("p-2^%d%+d" % (k, d), P - (1 << k) + d)]
    return named


def base_values(f):
    """W as [(name, value)], values distinct and below p."""
    P = f.P
    named = core_values(f)
    for k in range(256):
        for d in (-1, 0, 1):
            if 0 <= (1 << k) + d < P:
                named.append(("2^%d%+d" % (k, d), (1 << k) + d))
            if 0 <= P - (1 << k) + d < P:
                named.append(("p-2^%d%+d" % (k, d), P - (1 << k) + d))
    named = _dedupe(named)
    return _dedupe(named + [(n + "*R", v * f.R % P) for n, v in named] + [(n + "/R", v * f.Rinv % P) for n, v in named])


def _signature(f, v):
    """The instances a value fires as an operand of the cheap helpers: against itself, its complements and a few fixed partners."""
    P, s = f.P, set()
    for b in (v, P - 1 - v, (P - v) % P, (P + 1 - v) % P, 1, P - 1):
        s |= {("add",) + i for i in fired_by("add", f, (v, b))}
    for a, b in ((v, (v + 1) % P), (0, v), (v, P - 1), (1, v), (v, (v + (1 << 64)) % P), (v, (v + (1 << 128)) % P)):
        s |= {("sub",) + i for i in fired_by("sub", f, (a, b))}
    for y in (value(f.r2), 1, P - 1):
        s |= {("mul",) + i for i in fired_by("mul", f, (v, y))}
        s |= {("mul'",) + i for i in fired_by("mul", f, (y, v))}
    return s


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


THIN_COVER = 3    # witnesses kept per instance, where W has that many


def thinned_values(name):
    """W thinned, once and deterministically: core_values, then greedily the value that adds most to the cover until every instance that
    some value of W fires (_signature) is fired by THIN_COVER kept values, or by all that fire it.  [(name, value)] in W's order."""
    def make():
        f = field(name)
        W = base_values(f)
        sig = [_signature(f, v) for _, v in W]
        need = {}
        for s in sig:
            for i in s:
                need[i] = min(THIN_COVER, need.get(i, 0) + 1)
        core = {v for _, v in _dedupe(core_values(f))}
        keep = [w in core for _, w in W]
        for k, s in enumerate(sig):
            if keep[k]:
                for i in s:
                    need[i] = max(0, need[i] - 1)
        while any(need.values()):
            gain = [0 if keep[k] else sum(1 for i in s if need[i]) for k, s in enumerate(sig)]
            best = max(range(len(W)), key=lambda k: (gain[k], -k))
            assert gain[best]
            keep[best] = True
            for i in sig[best]:
                need[i] = max(0, need[i] - 1)
        return [w for k, w in enumerate(W) if keep[k]]
    return _cached(("thin", name), make)


def multipliers(name):
    """At most 64 second operands of fe_mont_mul, [(name, value)]: 1 (the product is x * R^-1: fe_from_mont), R (the product is x), R^2
    (fe_to_mont), 0, the small and the large ones, the word patterns."""
    def make():
        f = field(name)
        P = f.P
        named = [("1", 1), ("R", f.R), ("R^2", value(f.r2)), ("0", 0), ("2", 2), ("3", 3), ("p-1", P - 1), ("p-2", P - 2), ("(p-1)/2", (P - 1) // 2),
                 ("(p+1)/2", (P + 1) // 2), ("1/R", f.Rinv), ("2^64-1", M64), ("2^64", 1 << 64), ("2^64+1", (1 << 64) + 1), ("2^128-1", (1 << 128) - 1),
                 ("2^128", 1 << 128), ("2^192", 1 << 192), ("2^253", 1 << 253), ("p-2^64", P - (1 << 64)), ("p-2^128", P - (1 << 128)),
                 ("p-2^192", P - (1 << 192)), ("n0inv", f.n0inv), ("p-n0inv", P - f.n0inv)]
        named += [(n, v) for n, v in core_values(f) if n.startswith("ones") or n.endswith("+0z") or n.endswith("+0f")]
        named += [(n + "*R", v * f.R % P) for n, v in named[4:12]]
        out = _dedupe(named)[:64]
        return out
    return _cached(("mult", name), make)


def searched_mul_pairs(name):
    """Pairs (x, y) whose unreduced CIOS result T is at least p and has a word equal to p's word with a borrow entering it (the `u < br` term
    of the final subtraction).  T = x * y * R^-1 (mod p) and T < 2 p, so for a wanted T in [p, 2 p) the pair is x random (fixed seed),
    y = (T - p) * R / x; the model tells whether the accumulator came out as T or as T - p.  [(name, (x, y))], each confirmed by `fired`."""
    def make():
        f = field(name)
        P, p = f.P, f.p
        rng = random.Random("fe_words/mul/" + name)
        targets = []
        for k in (1, 2):                     # word k equal to p's; a word below it smaller (the borrow), a word above it larger (T >= p)
            for low in range(k):
                for high in range(k + 1, 4):
                    t = list(p)
                    if t[low] == 0:
                        continue
                    t[low] -= 1
                    t[high] += 1
                    T = value(t)
                    if P <= T < 2 * P:
                        targets.append(("T:w%d=p,w%d-1,w%d+1" % (k, low, high), k, T))
        out = []
        for tname, k, T in targets:
            found = 0
            for _ in range(400):
                x = rng.randrange(1, P)
                y = (T - P) * f.R % P * pow(x, -1, P) % P
                xw, t4 = PLAIN.mont_mul_unreduced(words(x), words(y), f)
                if t4 == 0 and value(xw) == T:
                    assert ("mul.b2", k) in fired_by("mul", f, (x, y))
                    out.append(("%s#%d" % (tname, found), (x, y)))
                    found += 1
                    if found == 2:
                        break
            assert found, (name, tname)
        return out
    return _cached(("mulsearch", name), make)


def mul_pairs(name):
    """Every pair the product route sends, [(name, (x, y))]: thinned_values x multipliers, then searched_mul_pairs."""
    return _cached(("mulpairs", name), lambda: [("%s x %s" % (nx, ny), (x, y)) for ny, y in multipliers(name) for nx, x in thinned_values(name)] +
                   searched_mul_pairs(name))


def addsub_pairs(name):
    """Pairs (a, b), both below p, for fe_add and fe_sub alike, [(name, (a, b))]."""
    def make():
        f = field(name)
        P, p = f.P, f.p
        firsts = [("0", 0), ("1", 1), ("2^64-1", M64), ("2^64", 1 << 64), ("2^128-1", (1 << 128) - 1), ("2^192", 1 << 192), ("(p-1)/2", (P - 1) // 2),
                  ("(p+1)/2", (P + 1) // 2), ("p-1", P - 1), ("p-2^64", P - (1 << 64)), ("p-2^128+1", P - (1 << 128) + 1), ("R", f.R), ("1/R", f.Rinv)]
        named = []
        # sums: a + b = T exactly (no reduction in between), for T around p and for T >= p with an equal word under a borrow
        sums = [("p-2", P - 2), ("p-1", P - 1), ("p", P), ("p+1", P + 1), ("p+2^64-1", P + M64), ("p+2^64", P + (1 << 64)), ("p+2^128", P + (1 << 128)),
                ("2p-2", 2 * P - 2), ("2^255-1", (1 << 255) - 1), ("2^255", 1 << 255)]
        for k in (1, 2):
            for low in range(k):
                for high in range(k + 1, 4):
                    t = list(p)
                    if t[low]:
                        t[low] -= 1
                        t[high] += 1
                        sums.append(("p:w%d-1,w%d+1" % (low, high), value(t)))
        for sn, T in sums:
            for an, a in firsts:
                if 0 <= T - a < P:
                    named.append(("%s+?=%s" % (an, sn), (a, T - a)))
        # all-ones words under a carry: a[k] + b[k] = 2^64 - 1 for k in `ones`, a carry out of word 0
        for ones in ((1,), (2,), (1, 2)):
            for x in (0, 1, 0x0123456789abcdef, M64):
                a = [M64, 0, 0, 1]
                b = [1, 0, 0, 2]
                for k in ones:
                    a[k], b[k] = x, M64 - x
                named.append(("carry into ones %s/%x" % (ones, x), (value(a), value(b))))
                a[0], b[0] = 1 << 63, 1 << 63
                named.append(("carry into ones %s/%x'" % (ones, x), (value(a), value(b))))
        # differences: 0, -1, +1; equal words under a borrow; a - b + p with an all-ones word under a carry
        for an, a in firsts:
            named.append(("%s-same" % an, (a, a)))
            if a + 1 < P:
                named.append(("%s-(same+1)" % an, (a, a + 1)))
                named.append(("(%s+1)-same" % an, (a + 1, a)))
        for eq in ((1,), (2,), (1, 2), (1, 2, 3), (3,), (2, 3)):
            for x in (0, 1, M64, p[eq[0]]):
                a = [0, 5, 6, 7]
                b = [1, 4, 3, 2]
                for k in eq:
                    a[k] = b[k] = min(x, p[3] - 1) if k == 3 else x
                if value(a) < P and value(b) < P:
                    named.append(("borrow into equal %s/%x" % (eq, x), (value(a), value(b))))
                    named.append(("borrow into equal %s/%x'" % (eq, x), (value(b), value(a))))
        for ks in ((1,), (2,), (1, 2), (3,), (1, 2, 3)):
            d = [M64, 0, 0, M64]                    # a - b (mod 2^256); word 0 + p[0] carries (p is odd)
            for k in range(1, 4):
                d[k] = (M64 - p[k]) if k in ks else M64
            diff = R256 - value(d)                  # b - a
            for an, a in firsts[:6]:
                if 0 < diff and a + diff < P:
                    named.append(("%s-?: +p carries into ones %s" % (an, ks), (a, a + diff)))
        return _dedupe_pairs(named)
    return _cached(("addsub", name), make)


def _dedupe_pairs(named):
    seen, out = set(), []
    for n, pr in named:
        if pr not in seen:
            seen.add(pr)
            out.append((n, pr))
    return out


def searched_inv_inputs(name):
    """Inputs of fe_inv that take its loop through the rare terms, [(name, value)], each confirmed by `fired`:
    sub256   an equal word under a borrow in the first round: u odd and below v = p with the words 1 .. k - 1 equal to p's and word 0 above
             p's, e.g. u = p[1] * 2^64 + p[0] + 2
    half_mod a carry into a word with x[k] + p[k] = 2^64 - 1.  The loop keeps x1 * a == u (mod p), so x1 is U / a whenever u = U: for a wanted
             odd X (word k = 2^64 - 1 - p[k], the words below it all ones) the input a = U / X makes half_mod meet X when u passes the even
             U.  u passes few values, so small U (2, 4, 6, ...) are tried and the model tells which of them it met."""
    def make():
        f = field(name)
        P, p = f.P, f.p
        named = []
        for top in (2, 3, 4):                       # words 1 .. top - 1 equal to p's, nothing above them
            for d in (2, 4, 1 << 32, (M64 - p[0]) & ~1):
                if d and p[0] + d <= M64:
                    u = value([p[0] + d] + [p[k] if k < top else 0 for k in range(1, 4)])
                    if 0 < u < P:
                        named.append(("p[:%d]+%#x" % (top, d), u))
        named = [(n, u) for n, u in _dedupe(named) if any(s == "inv.sub256.b2" for s, _ in fired_by("inv", f, (u,)))]
        assert named
        for k in (1, 2, 3):
            for hi in (0, 1):
                X = value([M64 if j < k else (M64 - p[j]) & M64 if j == k else hi for j in range(4)])
                if k == 3:
                    X = value([M64, M64, M64, (M64 - p[3]) & M64])
                if not X < P:
                    continue
                found = 0
                for U in range(2, 66, 2):
                    a = U * pow(X, -1, P) % P
                    if ("inv.half.c2", k) in fired_by("inv", f, (a,)):
                        named.append(("%d/half:ones<%d,w%d+p=ones,%d" % (U, k, k, hi), a))
                        found += 1
                        if found == 2:
                            break
        return _dedupe(named)
    return _cached(("invsearch", name), make)


def inv_inputs(name):
    """Every input the inversion route sends, [(name, value)], none zero."""
    return _cached(("inv", name), lambda: _dedupe([(n, v) for n, v in thinned_values(name) if v] + searched_inv_inputs(name)))


def inv_words(name):
    """One-word inputs of fe_inv_word (2 <= s < 2^64): the fixed words of tests/test_cabi_host.py, every 2^k and 2^k +- 1, seeded ones."""
    def make():
        P = FIELD_MODULI[name]
        rng = random.Random("fe_words/inv_word/" + name)
        ws = [2, 3, 255, 256, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 64) - 1, (1 << 64) - 2, P % (1 << 64) or 7, 0x0304020105000420, 0x0001ffffffffffff]
        ws += [(1 << k) + d for k in range(2, 64) for d in (-1, 0, 1)]
        ws += [rng.getrandbits(64) | 1 for _ in range(40)] + [rng.getrandbits(rng.randrange(2, 65)) or 5 for _ in range(40)]
        return [w for w in dict.fromkeys(ws) if 2 <= w <= M64]
    return _cached(("invw", name), make)


# ---- the kill condition ----------------------------------------------------------------------------------------------------------------
# site -> (operation, which set).  A site is killed when some input of the set gives a mutant result that differs from the true one.
def kill_sets(name):
    """op -> [args]: exactly the inputs the routes send."""
    return {
        "add": [pr for _, pr in addsub_pairs(name)],
        "sub": [pr for _, pr in addsub_pairs(name)],
        "mul": [pr for _, pr in mul_pairs(name)],
        "inv": [(v,) for _, v in inv_inputs(name)],
        "inv_word": [(w,) for w in inv_words(name)],
    }


SITE_OPS = {"add": ("add",), "sub": ("sub", "inv"), "mac": ("mul", "inv_word"), "mul": ("mul",), "inv": ("inv",), "invw": ("inv_word",)}


def fired_index(name):
    """op -> {instance: [args that fire it]} over kill_sets: one unmutated pass, shared by every mutant's search for a witness."""
    def make():
        f = field(name)
        index = {}
        for op, inputs in kill_sets(name).items():
            idx = index.setdefault(op, {})
            for args in inputs:
                for inst in fired_by(op, f, args):
                    idx.setdefault(inst, []).append(args)
        return index
    return _cached(("fired", name), make)


def killer(name, site, instance=None, tries=8):
    """(op, args) on which the mutant that drops `site` (or its one `instance`) differs from the truth, or None.  Only inputs that fire the
    site can differ, so those are the ones evaluated (at most `tries` per instance and operation)."""
    f = field(name)
    index = fired_index(name)
    drop = (site,) if instance is None else ((site, instance),)
    for op in SITE_OPS[site.split(".")[0]]:
        for inst, inputs in sorted(index[op].items(), key=repr):
            if inst[0] != site or (instance is not None and inst[1] != instance):
                continue
            for args in inputs[:tries]:
                if evaluate(op, f, args, drop=drop) != truth(op, f, args):
                    return op, args
    return None
