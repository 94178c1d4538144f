"""CPU: the models of the prover chain fit each other and the circuits this library records (tests/prover_chain_ref.py; DESIGN.md section
2g).  An advice image restated from the oracle's stream, the fixed rows of its row kinds, the record's copy map as sigma columns, the
permutation and lookup products of the existing models: the quotient h of all of it together is a polynomial of degree < 4n -- every
coefficient of index >= 4n is zero -- and after any single fault it is not.  Nothing is compared with a model of the quotient's own; what
is checked is that the conventions agree: the order of the fixed columns, se_next as rotation +1 of column e, theta * tag + enable * advice
against AR.lookup_inputs, labels delta^c * omega^i against sigma, Z_s[0] = Z_{s-1}[u], where u and the blinding rows lie, first_row.

Sets of more than three permutation columns are not tried: with the extended domain at k + 3 the numerator may have degree 5 (n - 1), and
l_active * Z * (chunk_len factors) has degree (chunk_len + 2) (n - 1) (the same bound test_quotient_model.py states).

The extended form of a column costs two Python transforms, so the module keeps every extension it has made (`cache`): circuits that
share a key or an image transform only what differs."""
import copy
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import advice_ref as AR
import prover_chain_ref as CR
import quotient_ref as QR
from oracle_lib import Oracle
from test_maingate_image_ref import FIELDS
from test_mockprover_ref import _mul_mod, _record_copies

FIELD_INDEX = {"bn254_fr": 0, "bn254_fq": 1, "pasta_fp": 2, "pasta_fq": 3}      # h2r_params.field


def _in_field(w, L, field, seed):
    o = Oracle(w, L)
    rng = random.Random(seed)
    n = rng.getrandbits(w * L) | (1 << (w * L - 1)) | 1
    x = rng.randrange(n)
    rc, lt, st = o.assert_in_field(o.limbs(x), o.limbs(n))
    assert rc == 0 and lt == 1
    return AR.in_field_image(o.p, [int(v) for v in o.limbs(x)], [int(v) for v in o.limbs(n)], st, FIELDS[field])


# name -> (w, L, field, RSAChip's table, k, rows, table rows)
IMAGES = {
    "mul_mod-64x4-bn254": (64, 4, "bn254_fr", False, 9, 250, 267),       # the default table does not fit 2^8 - 6 rows
    "mul_mod-32x8-pasta": (32, 8, "pasta_fq", False, 10, 590, 19),
    "in_field-64x4-bn254": (64, 4, "bn254_fr", False, 9, 244, 267),
    "mul_mod-64x4-rsa-table": (64, 4, "bn254_fr", True, 9, 250, 283),    # the 4-bit range between 3 and 8: the 8-bit rows carry tag 4, not 3
}
BASE = "mul_mod-64x4-bn254"


class Chain:
    """The module's images (made once), the circuits built from them, and the extensions kept between them."""

    def __init__(self):
        self.cache, self._image, self._circuit = {}, {}, {}

    def image(self, name):
        """(rows, kinds, pairs, lcfg) of a named image."""
        if name not in self._image:
            w, L, field, rsa, _, _, _ = IMAGES[name]
            if name.startswith("in_field"):
                im, pairs = _in_field(w, L, field, 41), []                 # (the library has no copy map of this op: the permutation is the identity)
            else:
                im, pairs = _mul_mod(w, L, field, 1000 * w + L)[4], _record_copies(w, L)
            self._image[name] = (im.rows, im.kinds, pairs, AR.LookupConfig(AR.range_lens(w, L, rsa=rsa)))
        return self._image[name]

    def circuit(self, name, **kw):
        """The circuit of a named image (chunk_len 2, first_row 0, all five lookup arguments unless kw says otherwise), made once per kw."""
        key = (name, tuple(sorted((k, v) for k, v in kw.items() if k not in ("fixed_rows", "table"))), "fixed_rows" in kw)
        if key not in self._circuit:
            w, L, field, _, k, _, _ = IMAGES[name]
            rows, kinds, pairs, lcfg = self.image(name)
            P = FIELDS[field]
            rng = random.Random("chain/challenges/" + name)
            ch = tuple(rng.randrange(1, P) for _ in range(4))
            self._circuit[key] = CR.circuit_from_image(rows, kinds, pairs, w, L, P, lcfg, k, ch, random.Random("chain/tails/" + name), **kw)
        return self._circuit[key]

    def split(self, circ):
        """(the coefficients of h in [3n, 4n), those of index >= 4n)."""
        n = circ.cfg.n
        coeffs = CR.quotient_coefficients(circ, self.cache)
        assert len(coeffs) == 8 * n
        return coeffs[3 * n:4 * n], coeffs[4 * n:]


@pytest.fixture(scope="module")
def chain():
    return Chain()


@pytest.mark.parametrize("name", list(IMAGES))
def test_a_recorded_image_has_a_polynomial_quotient(chain, name):
    w, L, field, rsa, k, n_rows, table_rows = IMAGES[name]
    circ = chain.circuit(name)
    c = circ.cfg
    assert (c.k, c.log_ext, c.u, len(c.sets), c.args, circ.image_rows, circ.lcfg.n_rows) == (k, k + 3, (1 << k) - 6, 3, [0, 1, 2, 3, 4], n_rows, table_rows)
    assert n_rows > (1 << (k - 1)) - 6 or table_rows > (1 << (k - 1)) - 6              # no smaller domain holds the image and the table
    fx = circ.lag["fixed"]
    assert any(fx[7][:c.u]) and any(fx[QR.F_COMP_TAG][:c.u]) and any(fx[5][:c.u])         # se_next rows, lookup rows, multiplication rows
    if not name.startswith("in_field"):
        inside = [p for p in circ.pairs if p[2] not in CR.PR.H2R_COPY_SRC]                 # (64, 4): 288 of the record's 336 pairs
        assert len(inside) >= 288 and len(circ.pairs) - len(inside) == 3 * L * L and any(fx[QR.F_OVER_TAG][:c.u]) == (w == 64)
    if rsa:
        assert circ.lcfg.tag_of[8] == 4 and max(fx[QR.F_COMP_TAG]) == 4
    top, high = chain.split(circ)
    assert not any(high), "%d nonzero coefficients of index >= 4n" % sum(1 for v in high if v)
    assert any(top)                                                                       # ... and the bound is no looser than it has to be


@pytest.mark.parametrize("chunk_len,first_row", [(1, 0), (3, 0), (2, 7)])
def test_set_sizes_and_placement(chain, chunk_len, first_row):
    circ = chain.circuit(BASE, chunk_len=chunk_len, first_row=first_row)
    assert len(circ.cfg.sets) == {1: 5, 2: 3, 3: 2}[chunk_len]
    if first_row:
        fx = circ.lag["fixed"]
        assert not any(any(col[:first_row]) for col in fx[:9]) and fx[QR.F_TABLE_TAG][1] == 1       # the image's rows moved, the table did not
        assert all(r >= first_row for (r, _, _, _) in circ.pairs)
    top, high = chain.split(circ)
    assert not any(high) and any(top)


def _library_key(name):
    """(fixed rows of the image's kinds, table rows) from the library's host calls, under the ctx's default lookup configuration."""
    from halo2_rsa_amd import _lib
    from test_copymap_layout import _host_ctx
    w, L, field, rsa, _, _, _ = IMAGES[name]
    lib, ctx = _host_ctx(w, w * L, FIELD_INDEX[field])
    cfg = _lib.H2RLookupConfig()
    assert lib.h2r_lookup_config_default(ctx, 1 if rsa else 0, ctypes.byref(cfg)) == 0
    import numpy as np
    tag_col, val_col = np.zeros((cfg.n_rows, 4), dtype=np.uint64), np.zeros((cfg.n_rows, 4), dtype=np.uint64)
    assert lib.h2r_lookup_table_image(ctx, ctypes.byref(cfg), tag_col.ctypes.data, val_col.ctypes.data) == 0
    assert not tag_col[:, 1:].any() and not val_col[:, 1:].any()
    table = [(int(t[0]), int(v[0])) for t, v in zip(tag_col, val_col)]
    by_kind = {}

    def fixed_row(kind):
        if kind not in by_kind:
            fr = _lib.H2RFixedRow()
            assert lib.h2r_advice_fixed_row(ctx, ctypes.byref(cfg), kind, ctypes.byref(fr)) == 0, kind
            by_kind[kind] = fr.as_dict()
        return by_kind[kind]

    return lib, ctx, fixed_row, table


@pytest.mark.parametrize("name", [BASE, "mul_mod-32x8-pasta", "mul_mod-64x4-rsa-table"])
def test_the_library_key_is_the_models(chain, name):
    """h2r_advice_fixed_row of every row's kind and h2r_lookup_table_image give the fixed columns the helper builds from AR.fixed_row and
    LookupConfig.table(), and the quotient built from the library's vanishes."""
    lib, ctx, fixed_row, table = _library_key(name)
    rows, kinds, pairs, lcfg = chain.image(name)
    own = chain.circuit(name, fixed_rows=[fixed_row(int(k)) for k in kinds], table=table)
    lib.h2r_ctx_destroy(ctx)
    assert table == lcfg.table()
    model = chain.circuit(name)
    for i, (a, b) in enumerate(zip(own.lag["fixed"], model.lag["fixed"])):
        assert a == b, "fixed column %d" % i
    top, high = chain.split(own)
    assert not any(high) and any(top)


# ---- single faults on the real image ------------------------------------------------------------------------------------------------------
def _fault_gate_cell(f):
    row = next(i for i in range(f.cfg.u) if f.lag["fixed"][0][i])                            # a row whose sa is nonzero: cell a counts
    f.lag["advice"][0][row] = (f.lag["advice"][0][row] + 1) % f.P


def _fault_copy_destination(f):
    row, col, _, _ = next(p for p in f.pairs if p[2] not in CR.PR.H2R_COPY_SRC)
    f.lag["advice"][col][row] = (f.lag["advice"][col][row] + 1) % f.P


def _fault_sigma_entry(f):
    row, col, src_row, src_col = next(p for p in f.pairs if p[2] not in CR.PR.H2R_COPY_SRC)
    lab = CR.PR.labels(f.cfg.m, f.cfg.n, f.cfg.delta, f.cfg.omega(f.P), f.P)
    assert f.lag["sigma"][col][row] != lab[col][row]                                          # the cell is in a cycle ...
    f.lag["sigma"][col][row] = lab[col][row]                                                  # ... and now maps to itself


def _fault_swap_a_perm(f):
    ap = f.lag["lookup_a_perm"][0]
    i = next(i for i in range(f.cfg.u - 1) if ap[i] != ap[i + 1])
    ap[i], ap[i + 1] = ap[i + 1], ap[i]


def _fault_z0_first(f):
    f.lag["perm_z"][0][0] = 2


def _fault_selector(f):
    row = next(i for i in range(f.cfg.u) if f.lag["fixed"][5][i] and f.lag["advice"][0][i] * f.lag["advice"][1][i] % f.P)
    f.lag["fixed"][5][row] = (f.lag["fixed"][5][row] + 1) % f.P                                # s_mul_ab of a row whose a * b is nonzero


FAULTS = [_fault_gate_cell, _fault_copy_destination, _fault_sigma_entry, _fault_swap_a_perm, _fault_z0_first, _fault_selector]


@pytest.mark.parametrize("fault", FAULTS, ids=[f.__name__[7:] for f in FAULTS])
def test_a_single_fault_leaves_no_polynomial(chain, fault):
    good = chain.circuit(BASE)
    f = copy.copy(good)
    f.lag = copy.deepcopy(good.lag)
    fault(f)
    changed = [(name, i) for name, group in f.lag.items() for i, col in enumerate(group) if col != good.lag[name][i]]
    assert len(changed) == 1 and sum(1 for a, b in zip(f.lag[changed[0][0]][changed[0][1]], good.lag[changed[0][0]][changed[0][1]]) if a != b) <= 2
    _, high = chain.split(f)
    assert any(high)
