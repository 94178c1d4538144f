"""The case table of the adversarial lookup tests (test_lookup_cases_model.py on the CPU, test_lookup_adversarial.py on the GPU): synthetic
circuits for h2r_lookup_permuted_columns / h2r_lookup_product_columns whose challenge theta is chosen against lookup_setup_kernel's closed-form
ranking, with hand-made multiplicities.  Pure Python; no image and no chip emitter is involved.

A GROUP is one (config, field, usable_rows): one permuted_columns call and one product_columns call, its circuits are the batch elements.
A circuit is (theta, beta, gamma, five histograms): one histogram shape per lookup argument.  The plain model is advice_ref's compress /
table_column / permute_expression_pair and the Z recurrence with pow(den, -1, P), as test_lookup_product.Case.model writes it; the input
column A is the histogram's table rows plus (0, 0) padding in a seeded shuffled order.

Challenge families, per (config, field); t_j, S_j = 2^bit_len_j are the tag and the size of group j (the rows of one bit length), inverses mod P:
  zero            theta = 0: every group is 0, 1, 2, ...
  wrap(j, c)      theta = (P - c) / t_j: group j runs P - c, ..., P - 1, 0, 1, ...; j = the largest and the smallest group,
                  c in {1, S_j / 2, S_j - 1} (wraps), S_j (ends exactly at P - 1), S_j + 1 (ends at P - 2)
  overlap(i,j,d)  theta = d / (t_i - t_j): group i is group j shifted by d; j = the largest, i = the second largest group, d in {1, S_j - 1, S_j}
  word(j, k)      theta = (2^(64 k) - 3) / t_j, k = 1, 2, 3: the largest group straddles a word boundary of the 256-bit value
  one, pm1, random
Every family runs on all four fields of pyref.FIELD_MODULI."""
import os
import random
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import advice_ref as AR
import pyref

FIELDS = dict(pyref.FIELD_MODULI)
with open(os.path.join(ROOT, "halo2_rsa_amd", "csrc", "h2r_grand_product.hpp")) as _f:
    TILE = int(re.search(r"GRAND_PRODUCT_TILE = (\d+);", _f.read()).group(1))
R256 = 1 << 256

# ---- configurations ------------------------------------------------------------------------------------------------------------------
CONFIGS = {  # name -> (bit lengths, tags); "rsa" is h2r_lookup_config_default(rsa_chip = 1) of BigIntChip(64, 2048)
    "rsa": (sorted(set(b for b in AR.range_lens(64, 32, rsa=True) if b)), None),
    "max": (list(range(2, 10)), list(range(1, 9))),
    "tiny": ([1, 2], [1, 2]),
    "bigtag": ([3, 8], [0xFFFFFFFF, 0x80000001]),
}


def lookup_config(name):
    lens, tags = CONFIGS[name]
    return AR.LookupConfig(lens, tags=tags)


def groups_of(cfg):
    """[(tag, size, first table row)] of the configuration's bit lengths, ascending."""
    return [(cfg.tag_of[b], 1 << b, cfg.row_off[b]) for b in cfg.bit_lens]


def group_values(cfg, j, theta, P):
    t, S, _ = groups_of(cfg)[j]
    return [(t * theta + u) % P for u in range(S)]


# ---- challenges ----------------------------------------------------------------------------------------------------------------------
def _uniq(xs):
    out = []
    for x in xs:
        if x not in out:
            out.append(x)
    return out


def challenges(name, field):
    """[(label, theta, (family, parameters...))] of one (config, field), in a fixed order."""
    cfg, P = lookup_config(name), FIELDS[field]
    gs = groups_of(cfg)
    big, small, second = len(gs) - 1, 0, len(gs) - 2
    out = [("zero", 0, ("zero",))]
    for j in (big, small):
        t, S, _ = gs[j]
        for c in _uniq([1, S // 2, S - 1, S, S + 1]):
            out.append(("wrap(%d,%d)" % (j, c), (P - c) * pow(t, -1, P) % P, ("wrap", j, c)))
    (ti, _, _), (tj, Sj, _) = gs[second], gs[big]
    for d in _uniq([1, Sj - 1, Sj]):
        out.append(("overlap(%d,%d,%d)" % (second, big, d), d * pow(ti - tj, -1, P) % P, ("overlap", second, big, d)))
    for k in (1, 2, 3):
        out.append(("word(%d,%d)" % (big, k), ((1 << (64 * k)) - 3) * pow(tj, -1, P) % P, ("word", big, k)))
    out.append(("one", 1, ("one",)))
    out.append(("pm1", P - 1, ("pm1",)))
    out.append(("random", random.Random("theta/%s/%s" % (name, field)).randrange(P), ("random",)))
    return out


def size_challenges(name, field):
    """The three challenges every size of the full size list is crossed with: zero, one wrap (the largest group wraps in its middle), random."""
    big = len(groups_of(lookup_config(name))) - 1
    S = groups_of(lookup_config(name))[big][1]
    want = ("zero", "wrap(%d,%d)" % (big, S // 2), "random")
    got = [c for c in challenges(name, field) if c[0] in want]
    assert [c[0] for c in got] == list(want)
    return got


# ---- histograms ----------------------------------------------------------------------------------------------------------------------
SHAPES = ("empty", "once", "full", "last", "sparse", "collide")
SHAPES_FIRST = ("empty", "once", "full", "last", "sparse")      # the five arguments of a challenge's first circuit
SHAPES_SECOND = ("collide", "last", "sparse", "once", "full")   # ... and of its second one: the sixth shape, the others on other arguments


def colliding_rows(cfg, theta, P):
    """Table rows whose compressed value is also another row's."""
    vals = AR.compress(cfg.table(), theta, P)
    seen = {}
    for v in vals:
        seen[v] = seen.get(v, 0) + 1
    return [r for r, v in enumerate(vals) if seen[v] > 1]


def histogram(shape, cfg, theta, P, usable, rng):
    """(multiplicities of the table rows, the shape that was built -- "collide" falls back to "sparse" where no two rows collide)."""
    n = cfg.n_rows
    h = [0] * n
    if shape == "empty":
        pass
    elif shape == "once":                      # every table row exactly once, row 0 included
        h = [1] * n
    elif shape == "full":                      # total == usable_rows with h[0] = 0: no padding row
        chosen = rng.sample(range(1, n), max(1, (n - 1) // 2))
        for r in chosen:
            h[r] = 1
        rest = usable - len(chosen)
        for _ in range(8):
            take = rng.randrange(rest + 1)
            h[rng.choice(chosen)] += take
            rest -= take
        h[chosen[0]] += rest
    elif shape == "last":                      # all usable_rows inputs on the last table row
        h[n - 1] = usable
    elif shape == "collide":
        rows = colliding_rows(cfg, theta, P)
        if not rows:
            return histogram("sparse", cfg, theta, P, usable, rng)
        total = 0
        for r in sorted(rng.sample(rows, min(16, len(rows)))):
            m = rng.randrange(1, 4)
            if total + m > usable:
                break
            h[r] = m
            total += m
    elif shape == "sparse":
        k = min(8, n - 1)
        cap = max(1, usable // (2 * k))
        for r in rng.sample(range(n), k):
            h[r] = rng.randrange(1, cap + 1)
    else:
        raise ValueError(shape)
    assert sum(h) <= usable
    return h, shape


# ---- circuits and groups -------------------------------------------------------------------------------------------------------------
class Circuit:
    def __init__(self, key, name, field, usable, label, theta, family, shapes):
        cfg, P = lookup_config(name), FIELDS[field]
        self.key, self.label, self.theta, self.family = key, label, theta, family
        rng = random.Random(key)
        self.beta, self.gamma = rng.randrange(1, P), rng.randrange(P)
        built = [histogram(s, cfg, theta, P, usable, rng) for s in shapes]
        self.hists = [h for h, _ in built]
        self.shapes = [s for _, s in built]
        self.asked = list(shapes)

    def __repr__(self):
        return self.key


class Group:
    def __init__(self, name, field, usable, chals, second, kind):
        self.config, self.field, self.usable, self.kind, self.second = name, field, usable, kind, second
        self.id = "%s-%s-%d" % (name, field, usable)
        self.cfg, self.P = lookup_config(name), FIELDS[field]
        self.circuits = []
        for i, (label, theta, family) in enumerate(chals):
            first = SHAPES_FIRST if second else SHAPES_FIRST[i % 5:] + SHAPES_FIRST[:i % 5]   # (one circuit per challenge: rotate the shapes over the arguments)
            self.circuits.append(Circuit("%s/%s/1" % (self.id, label), name, field, usable, label, theta, family, first))
            if second:
                self.circuits.append(Circuit("%s/%s/2" % (self.id, label), name, field, usable, label, theta, family, SHAPES_SECOND))

    def model(self):
        return [circuit_model(self.cfg, self.P, c, self.usable) for c in self.circuits]

    def __repr__(self):
        return self.id


def input_pairs(cfg, hist, usable, seed):
    """The (tag, value) inputs of one argument: hist[r] copies of table row r, (0, 0) on every other usable row, in a seeded shuffled order."""
    table = cfg.table()
    pairs = [table[r] for r, m in enumerate(hist) for _ in range(m)]
    assert len(pairs) <= usable
    pairs += [(0, 0)] * (usable - len(pairs))
    random.Random(seed).shuffle(pairs)
    return pairs


def product_column(A, S, Ap, Sp, beta, gamma, P):
    """(Z, index of the first zero denominator or None): Z[0] = 1, Z[i+1] = Z[i] (A+beta)(S+gamma) / ((A'+beta)(S'+gamma)); Z stops at a zero denominator."""
    Z, inv = [1], {}
    for i in range(len(A)):
        den = (Ap[i] + beta) * (Sp[i] + gamma) % P
        if den == 0:
            return Z, i
        if den not in inv:
            inv[den] = pow(den, -1, P)
        Z.append(Z[-1] * (A[i] + beta) % P * (S[i] + gamma) % P * inv[den] % P)
    return Z, None


def circuit_model(cfg, P, c, usable, beta=None, gamma=None):
    """dict(A, S, Ap, Sp, Z, zero_den) of one circuit: five lists per column name (S: one list), canonical integers."""
    beta = c.beta if beta is None else beta
    gamma = c.gamma if gamma is None else gamma
    S = AR.table_column(cfg, c.theta, usable, P)
    out = dict(A=[], S=S, Ap=[], Sp=[], Z=[], zero_den=[])
    for k in range(5):
        A = AR.compress(input_pairs(cfg, c.hists[k], usable, "%s/A%d" % (c.key, k)), c.theta, P)
        Ap, Sp = AR.permute_expression_pair(A, S)
        Z, bad = product_column(A, S, Ap, Sp, beta, gamma, P)
        for key, v in (("A", A), ("Ap", Ap), ("Sp", Sp), ("Z", Z), ("zero_den", bad)):
            out[key].append(v)
    return out


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
FULL_SIZES = {"tiny": (7, 65), "rsa": (339, 513), "max": (1021, 1025), "bigtag": (265, 321)}   # n_rows and one ragged size: x every challenge
SIZE_LIST = {"tiny": [7, 63, 64, 65, 255, 256, 257], "rsa": [339, 340, 511, 512, 513, 1023, 1024, 1025, 8186], "max": [1021, 1024, 1025],
             "bigtag": [265, 321]}                                                              # x (zero, one wrap, random)
# rsa only.  The carry kernel gives lane l the tiles [l * per, (l + 1) * per), per = ceil(T / 64): T = 65 (per = 2, lanes 33-63 empty, one row in the
# last tile), T = 129 (per = 3, 43 lanes), and T = 64 -- every lane one tile, the one shape below 126 tiles where lane 63 holds a tile, and
# usable_rows a multiple of the tile, so Z[usable_rows] is written by the last thread of the last tile
Z_SIZES = [(64 * TILE + 1, "pasta_fp"), (128 * TILE + 5, "bn254_fr"), (64 * TILE, "bn254_fq")]
GAMMA_PM1 = "bn254_fr"   # per config, in the n_rows group of this field: one circuit with gamma = P - 1
BETA_PM1 = "pasta_fp"    # ... and one with beta = P - 1


def _pin_pm1(g, which):
    """gamma = P - 1 (beta = P - 1) on the first circuit of the group where the model says no S' + gamma (A' + beta) vanishes: S' is a permutation of
    the table column and A' of the inputs, so that is the first circuit without the value 1 in its table (inputs)."""
    for c in g.circuits:
        if which == "gamma":
            vals = set(AR.table_column(g.cfg, c.theta, g.usable, g.P))
        else:
            tv = AR.compress(g.cfg.table(), c.theta, g.P)
            vals = set(tv[r] for h in c.hists for r, m in enumerate(h) if m)
            if any(sum(h) < g.usable for h in c.hists):
                vals.add(0)
        if 1 not in vals:
            setattr(c, which, g.P - 1)
            c.pinned = which
            return c
    raise AssertionError("no circuit of %s takes %s = P - 1" % (g.id, which))


def build_groups():
    out = []
    for name in ("tiny", "rsa", "max", "bigtag"):
        for field in FIELDS:
            for usable in SIZE_LIST[name]:
                if usable in FULL_SIZES[name]:
                    # (the second circuit of every challenge, with the sixth histogram shape, at the n_rows size only: model time)
                    g = Group(name, field, usable, challenges(name, field), usable == FULL_SIZES[name][0], "challenges")
                    if usable == FULL_SIZES[name][0] and field == GAMMA_PM1:
                        _pin_pm1(g, "gamma")
                    if usable == FULL_SIZES[name][0] and field == BETA_PM1:
                        _pin_pm1(g, "beta")
                else:
                    g = Group(name, field, usable, size_challenges(name, field), False, "sizes")
                out.append(g)
    for usable, field in Z_SIZES:
        out.append(Group("rsa", field, usable, size_challenges("rsa", field), False, "tiles"))
    return out


GROUPS = build_groups()
BY_ID = {g.id: g for g in GROUPS}
N_GROUPS = len(GROUPS)
N_CIRCUITS = sum(len(g.circuits) for g in GROUPS)
MONTGOMERY_GROUPS = ["%s-pasta_fq-%d" % (name, FULL_SIZES[name][1]) for name in ("tiny", "rsa", "max", "bigtag")]
ARG_MASK_GROUP = "rsa-bn254_fq-513"


def to_bytes(vals, P, montgomery=False):
    """canonical integers -> 32-byte little-endian elements in the ctx's representation"""
    if montgomery:
        return b"".join((v * R256 % P).to_bytes(32, "little") for v in vals)
    return b"".join(v.to_bytes(32, "little") for v in vals)
