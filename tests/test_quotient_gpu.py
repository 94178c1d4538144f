"""h2r_quotient_columns / EvaluationDomain.quotient: the vanishing argument's quotient h on the extended domain (halo2 plonk::evaluation::
evaluate_h [3P, restated in DESIGN.md section 2g]) against the plain model of tests/quotient_ref.py, byte for byte.

The inputs are computed on the host with the model, so the byte-equality tests do not depend on h2r_ntt_columns.  They are random (an
unsatisfied circuit: equality matters here, not satisfaction) except where a test says otherwise.  Every output buffer is pre-filled with a
sentinel and has guard rows behind every circuit's h, which must come back unchanged; input columns have padding rows too, and the columns
of unselected lookup arguments hold bytes that are no field element.  The kernel takes QUOT_TILE points per workgroup (read from
csrc/h2r_quotient.hpp): 2^5 and 2^7 points are part of one workgroup, 2^8 one partly filled, 2^11 several, so that the rotations cross
workgroup and column ends.  One last test runs the device chain end to end: Lagrange columns of a satisfying circuit through
EvaluationDomain.ntt, quotient, the inverse coset transform, and the soundness condition on the coefficients."""
import os
import random
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ntt_ref as NR
import permutation_ref as PR
import quotient_ref as QR
from halo2_rsa_amd._lib import H2R_E_SHAPE
from pyref import FIELD_MODULI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R256 = 1 << 256
SENTINEL = 0xAB
GUARD = 3                                # sentinel rows behind every circuit's h
PAD = 2                                  # rows behind every input column
with open(os.path.join(ROOT, "halo2_rsa_amd", "csrc", "h2r_quotient.hpp")) as _f:
    _src = _f.read()
    TILE = 256 * int(re.search(r"constexpr u32 QUOT_LANE_POINTS = (\d+);", _src).group(1))
SHAPES = [(4, 5), (4, 7), (5, 8), (7, 11)]
assert (1 << 7) < TILE and (1 << 11) >= 2 * TILE and TILE % 256 == 0


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import halo2_rsa_amd as H_
    return H_


def to_bytes(vals, P, montgomery):
    if montgomery:
        vals = [v * R256 % P for v in vals]
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(len(vals), 32)


def to_ints(host, P, montgomery):
    raw = np.ascontiguousarray(host).tobytes()
    vals = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
    assert all(v < P for v in vals), "not the canonical representative"
    if montgomery:
        rinv = pow(R256, -1, P)
        vals = [v * rinv % P for v in vals]
    return vals


def make_config(P, k, log_ext, rng, column_src=(0, 1, 2, 3, 4, 5), chunk_len=2, lookup_mask=31, bf=None, scrambled=True):
    """A configuration over `num_fixed` = 16 fixed columns whose indices are scrambled: nothing depends on where a column lies."""
    idx = list(range(16))
    if scrambled:
        rng.shuffle(idx)
    n = 1 << k
    bf = min(5, n - 2) if bf is None else bf
    return QR.Config(k, log_ext, bf, NR.omega_of(P, log_ext), NR.cube_root_of_unity(P), PR.domain(P, k)[1], 16, idx[:9], column_src, chunk_len, lookup_mask,
                     [rng.randrange(5) for _ in range(5)], [rng.choice(idx) for _ in range(5)], [rng.choice(idx) for _ in range(5)], idx[9], idx[10])


class Dev:
    """A chip over `field` in one representation and what a call needs around it."""

    def __init__(self, H, field, montgomery):
        self.H, self.P, self.mont = H, FIELD_MODULI[field], montgomery
        self.chip = H.BigIntChip(64, 256, field=field, montgomery=montgomery)

    def rep(self, v):
        return v * R256 % self.P if self.mont else v

    def domain(self, cfg):
        return self.H.EvaluationDomain(self.chip, cfg.k, cfg.log_ext, self.rep(cfg.omega_ext), self.rep(cfg.zeta))

    def group(self, columns, N, col_major=False):
        """columns: [circuit][column] lists of N integers (None: a column that is never read) -> (host array, device view [B, C, N, 32])."""
        B, C = len(columns), len(columns[0])
        host = np.full((C, B, N + PAD, 32) if col_major else (B, C, N + PAD, 32), 0xEE, dtype=np.uint8)
        for b in range(B):
            for c in range(C):
                if columns[b][c] is not None:
                    (host[c, b] if col_major else host[b, c])[:N] = to_bytes(columns[b][c], self.P, self.mont)
        dev = torch.from_numpy(host).cuda()
        return host, dev, (dev.permute(1, 0, 2, 3) if col_major else dev)[:, :, :N]

    def run(self, cfg, circuits, chs, status_in=None, col_major=False, raw_challenges=None):
        """circuits: per circuit the model's column dict (the key groups are taken from the first); chs: per circuit (theta, beta, gamma, y).
        Returns (per circuit h as integers or None where the sentinel is untouched, status bytes) after checking guards and inputs."""
        B, N, P = len(circuits), cfg.N, self.P
        nl = max(cfg.args) + 1 if cfg.args else 0
        kept, views = [], {}
        for name in QR.PER_CIRCUIT:
            cols = [c[name][:nl] if name.startswith("lookup") else c[name] for c in circuits]
            if cols[0]:
                hst, dev, view = self.group(cols, N, col_major)
                kept.append((hst, dev))
                views[name] = view
        for name in QR.KEY:
            hst, dev, view = self.group([circuits[0][name]], N)
            kept.append((hst, dev))
            views[name] = view[0]
        full = torch.full((B, N + GUARD, 32), SENTINEL, dtype=torch.uint8, device="cuda")
        status = torch.tensor(status_in if status_in is not None else [0] * B, dtype=torch.uint8, device="cuda")
        words = raw_challenges or [[self.rep(v) for v in ch] for ch in chs]
        dom = self.domain(cfg)
        h, st = dom.quotient(cfg.blinding_factors, self.rep(cfg.delta), cfg.gate_fixed, cfg.column_src, cfg.chunk_len, views["advice"], views["perm_z"],
                             views["fixed"], views["sigma"], views["l"], *[[w[i] for w in words] for i in range(4)], extra=views.get("extra"),
                             lookup_mask=cfg.lookup_mask, lookup_advice=cfg.lookup_advice, lookup_tag=cfg.lookup_tag, lookup_enable=cfg.lookup_enable,
                             table_tag=cfg.table_tag, table_value=cfg.table_value, lookup_a_perm=views.get("lookup_a_perm"),
                             lookup_s_perm=views.get("lookup_s_perm"), lookup_z=views.get("lookup_z"), out=(full[:, :N], status))
        torch.cuda.synchronize()
        fh = full.cpu().numpy()
        assert (fh[:, N:] == SENTINEL).all(), "guard rows behind a circuit's h were written"
        for hst, dev in kept:
            assert np.array_equal(dev.cpu().numpy(), hst), "an input was written"
        out = []
        for b in range(B):
            if (fh[b, :N] == SENTINEL).all():
                out.append(None)
            else:
                out.append(to_ints(fh[b, :N], P, self.mont))
        return out, st.cpu().tolist()


def challenges(rng, P):
    return tuple(rng.randrange(1, P) for _ in range(4))


def check_random(d, cfg, rng, batch=1, col_major=False):
    key = QR.random_columns(rng, cfg, d.P)
    circuits = []
    for _ in range(batch):
        c = QR.random_columns(rng, cfg, d.P)
        for name in QR.KEY:
            c[name] = key[name]
        circuits.append(c)
    chs = [challenges(rng, d.P) for _ in range(batch)]
    got, st = d.run(cfg, circuits, chs, col_major=col_major)
    assert st == [0] * batch
    for b in range(batch):
        assert got[b] == QR.quotient(cfg, circuits[b], chs[b], d.P), (cfg.k, cfg.log_ext, cfg.chunk_len, cfg.lookup_mask, b)


# ---- 1. every shape, field and representation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("montgomery", [False, True], ids=["canonical", "montgomery"])
@pytest.mark.parametrize("field", NR.FIELDS_WITH_DOMAINS)
def test_shapes_against_the_model(H, field, montgomery):
    d = Dev(H, field, montgomery)
    rng = random.Random("quotient/%s/%d" % (field, montgomery))
    for (k, log_ext) in SHAPES:
        check_random(d, make_config(d.P, k, log_ext, rng), rng)


# ---- 2. permutation sets and lookup masks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("montgomery", [False, True], ids=["canonical", "montgomery"])
def test_sets_and_masks(H, montgomery):
    d = Dev(H, "bn254_fr", montgomery)
    rng = random.Random(11 + montgomery)
    for chunk_len, mask in [(1, 0), (2, 1 << 3), (3, 31), (4, 1), (9, 1 << 4)]:
        cfg = make_config(d.P, 4, 7, rng, chunk_len=chunk_len, lookup_mask=mask)
        assert len(cfg.sets) == {1: 6, 2: 3, 3: 2, 4: 2, 9: 1}[chunk_len]
        check_random(d, cfg, rng)
    for src, mask in [((3,), 0), ((5,), 0b10100), ((7, 2, 6, 0, 5, 4, 1, 3), 31)]:          # m = 1 (an advice column; an extra column), m = 8 with three extra
        check_random(d, make_config(d.P, 4, 7, rng, column_src=src, chunk_len=3, lookup_mask=mask), rng)
    check_random(d, make_config(d.P, 1, 2, rng, column_src=(0,), chunk_len=1, lookup_mask=1, bf=0), rng)   # the smallest domain there is
    check_random(d, make_config(d.P, 3, 7, rng, bf=0), rng)                                  # r = 16; no blinding rows: the last rotation is -1
    check_random(d, make_config(d.P, 5, 6, rng, bf=29), rng)                                 # u = 2: the last rotation spans nearly the whole column


# ---- 3. a batch: a skipped circuit, a refused one, both stride orders ------------------------------------------------------------------------------
@pytest.mark.parametrize("col_major", [False, True], ids=["circuit-major", "column-major"])
@pytest.mark.parametrize("montgomery", [False, True], ids=["canonical", "montgomery"])
def test_batch_of_three(H, montgomery, col_major):
    d = Dev(H, "pasta_fq", montgomery)
    P = d.P
    rng = random.Random(23 + montgomery)
    for (k, log_ext) in [(4, 7), (7, 11)]:
        cfg = make_config(P, k, log_ext, rng)
        check_random(d, cfg, rng, batch=3, col_major=col_major)
        # circuit 0 has status 7 on entry, circuit 2 a y that is no field element: both stay at the sentinel, 7 stays, 2 is told
        key = QR.random_columns(rng, cfg, P)
        circuits = [dict(QR.random_columns(rng, cfg, P), **{name: key[name] for name in QR.KEY}) for _ in range(3)]
        chs = [challenges(rng, P) for _ in range(3)]
        raw = [[d.rep(v) for v in ch] for ch in chs]
        raw[2][3] = P
        got, st = d.run(cfg, circuits, chs, status_in=[7, 0, 0], col_major=col_major, raw_challenges=raw)
        assert st == [7, 0, H2R_E_SHAPE]
        assert got[0] is None and got[2] is None
        assert got[1] == QR.quotient(cfg, circuits[1], chs[1], P)
    for bad in range(3):                                                                     # theta, beta, gamma >= p are refused alike
        raw = [[d.rep(v) for v in chs[0]]]
        raw[0][bad] = (1 << 256) - 1
        got, st = d.run(cfg, circuits[:1], chs[:1], col_major=col_major, raw_challenges=raw)
        assert st == [H2R_E_SHAPE] and got == [None]


# ---- 4. the satisfying circuit, and columns of all 0 and all p - 1 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("montgomery", [False, True], ids=["canonical", "montgomery"])
def test_satisfying_circuit_and_extreme_columns(H, montgomery):
    d = Dev(H, "bn254_fr", montgomery)
    P = d.P
    circ = QR.satisfying_circuit(random.Random("quotient/gpu"), P, 4)
    cols = circ.extended()
    want = QR.quotient(circ.cfg, cols, circ.ch, P)
    got, st = d.run(circ.cfg, [cols], [circ.ch])
    assert st == [0] and got[0] == want
    assert not any(QR.coefficients(circ.cfg, got[0], P)[4 * circ.cfg.n:])                  # ... and it is a polynomial of degree < 4n
    rng = random.Random(31 + montgomery)
    cfg = make_config(P, 5, 8, rng)
    for fill in (0, P - 1):
        for groups in (QR.PER_CIRCUIT + QR.KEY, QR.PER_CIRCUIT, QR.KEY, ("advice", "l"), ("perm_z", "lookup_z", "sigma")):
            c = QR.random_columns(rng, cfg, P)
            for name in groups:
                c[name] = [None if col is None else [fill] * cfg.N for col in c[name]]
            for ch in (challenges(rng, P), (0, 0, 0, 0), (P - 1,) * 4):
                got, st = d.run(cfg, [c], [ch])
                assert st == [0] and got[0] == QR.quotient(cfg, c, ch, P), (fill, groups, ch[0])


# ---- 5. the device chain, end to end ----------------------------------------------------------------------------------------------------------------
def test_device_chain_end_to_end(H):
    """Lagrange columns of a satisfying circuit at k = 7 -> lagrange_to_coeff -> coeff_to_extended (k + 3) -> quotient -> extended_to_coeff:
    the coefficients of index >= 4n are all zero bytes; with one advice cell changed they are not.  (This case runs h2r_ntt_columns.)"""
    d = Dev(H, "bn254_fr", True)
    P = d.P
    circ = QR.satisfying_circuit(random.Random("quotient/chain"), P, 7, n_cycles=12)
    cfg = circ.cfg
    n, N = cfg.n, cfg.N
    dom = d.domain(cfg)
    nl = max(cfg.args) + 1

    def extended(columns):
        lag = torch.from_numpy(np.stack([to_bytes(c, P, d.mont) for c in columns])).cuda()
        return dom.coeff_to_extended(dom.lagrange_to_coeff(lag))

    def high_coefficients(lag):
        ext = {name: extended(lag[name][:nl] if name.startswith("lookup") else lag[name]) for name in QR.PER_CIRCUIT + ("fixed", "sigma")}
        h, st = dom.quotient(cfg.blinding_factors, d.rep(cfg.delta), cfg.gate_fixed, cfg.column_src, cfg.chunk_len, ext["advice"][None], ext["perm_z"][None],
                             ext["fixed"], ext["sigma"], dom.vanishing_columns(cfg.blinding_factors), *[[d.rep(v)] for v in circ.ch], extra=ext["extra"][None],
                             lookup_mask=cfg.lookup_mask, lookup_advice=cfg.lookup_advice, lookup_tag=cfg.lookup_tag, lookup_enable=cfg.lookup_enable,
                             table_tag=cfg.table_tag, table_value=cfg.table_value, lookup_a_perm=ext["lookup_a_perm"][None],
                             lookup_s_perm=ext["lookup_s_perm"][None], lookup_z=ext["lookup_z"][None])
        coeffs = dom.extended_to_coeff(h)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0]
        host = coeffs.cpu().numpy()
        assert host.shape == (1, N, 32)
        return host[0, 4 * n:], host[0, :4 * n]

    high, low = high_coefficients(circ.lag)
    assert low.any()
    assert not high.any(), "%d nonzero bytes in the coefficients of index >= 4n" % int(np.count_nonzero(high))
    row = next(i for i in range(cfg.u) if circ.lag["fixed"][0][i])
    circ.lag["advice"][0][row] = (circ.lag["advice"][0][row] + 1) % P
    high, _ = high_coefficients(circ.lag)
    assert high.any()
