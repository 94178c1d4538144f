"""The case table of the verifier's scalar tests (test_verify_scalars_host.py on the CPU, test_verify_scalars_gpu.py on the GPU): synthetic
constraint-system shapes for h2r_verify_scalars / h2r_verify_eval -- domains from 2 to 2^24 rows, 0 to 13 blinding
factors, permutation sets that are single, full and ragged, every kind of lookup mask -- with evaluations and challenges drawn from uniform
and edge values.  Pure Python over the plain models; the library is imported by `verify_config` alone, when it is called.

A SHAPE is (k, bf, m, chunk_len, lookup_mask); num_fixed and every column index of its configuration are drawn from a generator seeded by
the shape, so a shape names one configuration.  A circuit is (evaluations in create_proof_ref.eval_plan's order, the seven challenges
theta, beta, gamma, y, x, v, u), canonical integers.  `lagrange_products` is a second opinion on create_proof_ref.lagrange_at: the product
form of the interpolation polynomials, for the small domains."""
import ctypes
import itertools
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import create_proof_ref as C
import msm_ref as M
import ntt_ref as NR
import permutation_ref as PR
import quotient_ref as QR
import transcript_ref as T

R = T.R
EDGE = (0, 1, R - 1)
MAX_PLAN, MAX_PRODUCT_K = 64, 5

# ---- the grid --------------------------------------------------------------------------------------------------------------------------
DOMAINS = [(1, 0), (2, 0), (2, 2), (3, 1), (3, 6), (4, 13), (5, 13), (5, 5), (9, 5), (24, 13)]       # (k, blinding factors)
COLUMNS = [(1, 1), (3, 2), (8, 1), (8, 3), (8, 8), (5, 9), (7, 6)]                                  # (m, chunk_len)
MASKS = [0, 1, 16, 10, 31]
NUM_FIXED = (1, 9, 16)
GRID = [(k, bf, m, chunk, mask) for (k, bf), (m, chunk), mask in itertools.product(DOMAINS, COLUMNS, MASKS)]
_DOMAIN = {}


def make(rng, k, bf, m, chunk_len, lookup_mask, num_fixed):
    """The quotient_ref.Config of one shape: halo2's omega and delta, every column index drawn below its bound."""
    if k not in _DOMAIN:
        _DOMAIN[k] = NR.omega_of(R, k + 1), PR.domain(R, k)[1], NR.cube_root_of_unity(R)
    omega_ext, delta, zeta = _DOMAIN[k]
    fixed = lambda count: [rng.randrange(num_fixed) for _ in range(count)]
    return QR.Config(k, k + 1, bf, omega_ext, zeta, delta, num_fixed, fixed(9), [rng.randrange(5) for _ in range(m)], chunk_len, lookup_mask,
                     [rng.randrange(5) for _ in range(5)], fixed(5), fixed(5), rng.randrange(num_fixed), rng.randrange(num_fixed))


def shape_id(shape):
    return "k%d-bf%d-m%d-chunk%d-mask%d" % shape


def config_of(shape):
    """The one configuration of a shape (num_fixed is part of the draw)."""
    rng = random.Random("verify_cases/" + shape_id(shape))
    return make(rng, *shape, num_fixed=rng.choice(NUM_FIXED))


def shapes(domain=None):
    """The grid's shapes, or those of one (k, bf)."""
    return [s for s in GRID if domain is None or s[:2] == tuple(domain)]


def _self_check():
    """The grid holds every edge the tests are about: pruning it cannot silently drop one."""
    assert len(GRID) == len(set(GRID)) == 350
    cfgs = [config_of(s) for s in GRID]
    for cfg in cfgs:
        assert 1 <= cfg.k <= 24 and cfg.blinding_factors <= 13 and cfg.blinding_factors + 2 <= cfg.n and cfg.num_fixed <= 16 and cfg.m <= 8
        assert max(len(C.eval_plan(cfg)), len(C.open_plan(cfg))) <= MAX_PLAN and cfg.n_extra == 0
    sets = [[len(s) for s in cfg.sets] for cfg in cfgs]
    assert any(len(s) > 1 and s[-1] < s[0] for s in sets), "no ragged last set"
    assert any(len(s) == 1 for s in sets) and any(len(s) == 8 for s in sets)
    masks = {cfg.lookup_mask for cfg in cfgs}
    assert 0 in masks and any(mk and not mk & 1 for mk in masks), "no empty mask / no mask whose lowest argument is not 0"
    assert {0, 13} <= {cfg.blinding_factors for cfg in cfgs} and {1, 24} <= {cfg.k for cfg in cfgs}
    assert {cfg.num_fixed for cfg in cfgs} == set(NUM_FIXED)
    assert max(len(C.open_plan(cfg)) for cfg in cfgs) == 54


_self_check()


# ---- l0, l_last, l_active as products ------------------------------------------------------------------------------------------------------
def lagrange_products(cfg, x):
    """l0(x), l_last(x), l_active(x) from l_i(x) = prod_{j != i} (x - omega^j) / (omega^i - omega^j): l_last = l_u, l_active the sum over
    the usable rows i < u.  n^2 factors: small domains only."""
    assert cfg.k <= MAX_PRODUCT_K
    n, u, w = cfg.n, cfg.u, cfg.omega(R)
    pts = [pow(w, i, R) for i in range(n)]

    def l(i):
        num = den = 1
        for j in range(n):
            if j != i:
                num, den = num * (x - pts[j]) % R, den * (pts[i] - pts[j]) % R
        return num * pow(den, -1, R) % R

    return [l(0), l(u), sum(l(i) for i in range(u)) % R]


# ---- circuits ------------------------------------------------------------------------------------------------------------------------------
def draw(rng, exclude=()):
    """One value: three times in four uniform, else an edge value; never one of `exclude`."""
    while True:
        v = rng.choice(EDGE) if rng.randrange(4) == 0 else rng.randrange(R)
        if v not in exclude:
            return v


def inputs(rng, cfg, count):
    """[(evaluations, challenges)] of `count` circuits.  x is never 1 -- nor R - 1 = omega^(n/2), the other edge value that is a root of
    unity of every domain: x^n = 1 is a status of its own, which the tests raise on purpose."""
    ne = len(C.queries(C.eval_plan(cfg)))
    out = []
    for _ in range(count):
        evals = [draw(rng) for _ in range(ne)]
        out.append((evals, [draw(rng, (1, R - 1) if name == "x" else ()) for name in ("theta", "beta", "gamma", "y", "x", "v", "u")]))
    return out


def verify_config(cfg, montgomery):
    """h2r_verify_scalars' configuration of a model configuration: the model's own plans, entry by entry."""
    from halo2_rsa_amd import _lib
    plans = C.eval_plan(cfg), C.open_plan(cfg)
    out = _lib.H2RVerifyScalarsConfig(struct_size=ctypes.sizeof(_lib.H2RVerifyScalarsConfig), log_n=cfg.k, blinding_factors=cfg.blinding_factors,
                                      num_fixed=cfg.num_fixed, num_columns=cfg.m, chunk_len=cfg.chunk_len, lookup_mask=cfg.lookup_mask,
                                      num_eval_plan=len(plans[0]), num_open_plan=len(plans[1]), reserved=0)
    out.omega[:] = M.words(T.to_repr(cfg.omega(R), R, montgomery))
    out.delta[:] = M.words(T.to_repr(cfg.delta, R, montgomery))
    out.gate_fixed[:] = cfg.gate_fixed
    out.column_src[:cfg.m] = cfg.column_src
    out.lookup_advice[:], out.lookup_tag[:], out.lookup_enable[:] = cfg.lookup_advice, cfg.lookup_tag, cfg.lookup_enable
    out.table_tag, out.table_value = cfg.table_tag, cfg.table_value
    for table, plan in zip((out.eval_plan, out.open_plan), plans):
        for entry, (g, i, m) in zip(table, plan):
            entry.group, entry.index, entry.mask = _lib.VERIFY_GROUPS.index(g), i, m
    return out
