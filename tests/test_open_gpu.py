"""The openings on the device (EvaluationDomain.fold / open_eval / open_witness: h2r_fold_columns, h2r_open_eval_columns,
h2r_open_witness_columns) byte for byte against the plain model (tests/opening_ref.py) in both representations, over
bn254_fr and bn254_fq (nothing here needs a root of unity).  Sizes: one coefficient, less than a lane's four, a partial tile, a whole tile,
one past it, three tiles and one, and 2^17 (128 tiles: more than the carry wave's 64 lanes, so a lane holds a run of tiles).  Every output
buffer is filled with sentinel bytes and has guard rows behind each column."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import opening_ref as OR
from pyref import FIELD_MODULI
from test_lookup_product import bytes_of, in_repr

FIELDS = ("bn254_fr", "bn254_fq")
REPRS = [False, True]
SENTINEL, GUARD = 0xAB, 2
SENTINEL_WORD = int.from_bytes(bytes([SENTINEL]) * 8, "little", signed=True)
MASKS = (0b0011, 0b0001, 0b1011, 0b0001, 0b0001)     # of four points: 0 has every column, 1 two, 3 a single one, 2 none
KEY = 1                                              # the column that is the proving key's (one copy for every circuit)
MODEL = {}                                           # what the plain model made of a case, shared by the two representations


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import halo2_rsa_amd as H_
    return H_


def domain(H, field, montgomery):
    P = FIELD_MODULI[field]
    chip = H.BigIntChip(64, 256, field=field, montgomery=montgomery)
    rep = (lambda v: v * (1 << 256) % P) if montgomery else (lambda v: v)
    return H.EvaluationDomain(chip, 1, 1, rep(P - 1), rep(1))      # the openings use no root of unity: -1 serves any field


def scalars(vals, P, montgomery):
    """Integers in the ctx's representation; one that is no field element (>= p) stays what it is."""
    return [v if v >= P else in_repr([v], P, montgomery)[0] for v in vals]


def words_of(vals, P, montgomery):
    """Canonical integers (nested lists) -> the int64 [..., 4] a device array of elements holds in the ctx's representation."""
    a = np.array(vals, dtype=object)
    flat = bytes_of([int(v) for v in a.reshape(-1)], P, montgomery)
    return np.ascontiguousarray(flat).view(np.int64).reshape(a.shape + (4,))


def column_tensor(col, P, montgomery, batch=None):
    """A column (or per circuit a column) of integers -> uint8 [n, 32] / [batch, n, 32] on the device."""
    if batch is None:
        return torch.from_numpy(bytes_of(col, P, montgomery).copy()).cuda()
    return torch.from_numpy(np.stack([bytes_of(c, P, montgomery) for c in col])).cuda()


def guarded(lead, n):
    """(full, view): a sentinel-filled [*lead, n + GUARD, 32] and the view of its first n rows that a call is given."""
    full = torch.full(tuple(lead) + (n + GUARD, 32), SENTINEL, dtype=torch.uint8, device="cuda")
    return full, full[..., :n, :]


def make_case(name, P, n, batch, masks, points, key=None):
    """Random columns (the last per-circuit one holds p - 1 throughout) and the model's evaluations of them, made once per (name, field)."""
    if name in MODEL:
        return MODEL[name]
    rng = random.Random(name)
    cols = []                                            # cols[c][e] = coefficients; a key column has one copy
    for c in range(len(masks)):
        if c == key:
            cols.append([[rng.randrange(P) for _ in range(n)]])
        elif c == len(masks) - 1:
            cols.append([[P - 1] * n for _ in range(batch)])
        else:
            cols.append([[rng.randrange(P) for _ in range(n)] for _ in range(batch)])
    of = lambda c, e: cols[c][0 if c == key else e]
    qs = OR.queries(masks, len(points[0]))
    evals = [[OR.evaluate(of(c, e), points[e][p], P) for (c, p) in qs] for e in range(batch)]
    MODEL[name] = (cols, of, qs, evals)
    return MODEL[name]


def run_case(H, field, montgomery, name, n, batch, masks, points, vs, key=None, statuses=None, bad=()):
    """open_eval and open_witness of one case against the model; `bad`: circuits whose outputs must keep their sentinel bytes, statuses: the
    status bytes on entry.  Returns the status vectors after the calls."""
    P = FIELD_MODULI[field]
    dom = domain(H, field, montgomery)
    cols, of, qs, evals = make_case("%s/%s" % (name, field), P, n, batch, masks, points, key)
    num_points = len(points[0])
    tensors = [(column_tensor(cols[c][0], P, montgomery) if c == key else column_tensor(cols[c], P, montgomery, batch), m) for c, m in enumerate(masks)]
    pts = [scalars(row, P, montgomery) for row in points]
    st0 = torch.tensor(statuses or [0] * batch, dtype=torch.uint8, device="cuda")

    ev_out = torch.full((batch, len(qs), 4), SENTINEL_WORD, dtype=torch.int64, device="cuda")
    st_ev = st0.clone()
    dom.open_eval(tensors, pts, out=(ev_out, st_ev))
    full, W = guarded((batch, num_points), n)
    be = torch.full((batch, num_points, 4), SENTINEL_WORD, dtype=torch.int64, device="cuda")
    st_w = st0.clone()
    dom.open_witness(tensors, pts, scalars(vs, P, montgomery), out=(W, be, st_w))
    torch.cuda.synchronize()
    ev_host, be_host, w_host = ev_out.cpu().numpy(), be.cpu().numpy(), full.cpu().numpy()
    assert (w_host[:, :, n:] == SENTINEL).all(), "guard rows behind a W column were written"
    for e in range(batch):
        if e in bad:
            assert (ev_host[e] == SENTINEL_WORD).all() and (be_host[e] == SENTINEL_WORD).all() and (w_host[e] == SENTINEL).all(), e
            continue
        assert np.array_equal(ev_host[e], words_of(evals[e], P, montgomery)), "evaluations of circuit %d" % e
        if vs[e] >= P:                                   # v is the witness's alone
            assert (be_host[e] == SENTINEL_WORD).all() and (w_host[e] == SENTINEL).all(), e
            continue
        wit = OR.witness([of(c, e) for c in range(len(masks))], masks, points[e], vs[e], P)
        for p in range(num_points):
            if wit[p] is None:
                assert (w_host[e, p] == SENTINEL).all() and (be_host[e, p] == SENTINEL_WORD).all(), (e, p)
                continue
            Wm, rem = wit[p]
            assert np.array_equal(w_host[e, p, :n], bytes_of(Wm, P, montgomery)), "W of circuit %d, point %d" % (e, p)
            assert np.array_equal(be_host[e, p], words_of(rem, P, montgomery)), "batched evaluation of circuit %d, point %d" % (e, p)
            # the device's two routes agree without the model: the remainder is sum v^idx over the evaluations, combined here
            sel = [q for q, (c, pp) in enumerate(qs) if pp == p]
            got = [int.from_bytes(ev_host[e, q].tobytes(), "little") for q in sel]
            if montgomery:
                got = [g * pow(1 << 256, -1, P) % P for g in got]
            assert np.array_equal(be_host[e, p], words_of(sum(pow(vs[e], i, P) * g for i, g in enumerate(got)) % P, P, montgomery)), (e, p)
    return st_ev.cpu().tolist(), st_w.cpu().tolist()


@pytest.mark.parametrize("montgomery", REPRS, ids=["canonical", "montgomery"])
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", [1, 4, 1000, 1024, 1025, 3 * 1024 + 1])
def test_evaluations_and_witnesses(H, field, montgomery, n):
    P = FIELD_MODULI[field]
    rng = random.Random("open/points/%d" % n)
    points = [[rng.randrange(P) for _ in range(4)] for _ in range(3)]
    st_ev, st_w = run_case(H, field, montgomery, "open/%d" % n, n, 3, MASKS, points, [rng.randrange(P) for _ in range(3)], key=KEY)
    assert st_ev == [0, 0, 0] and st_w == [0, 0, 0]


@pytest.mark.parametrize("montgomery", REPRS, ids=["canonical", "montgomery"])
@pytest.mark.parametrize("field", FIELDS)
def test_adversarial_scalars(H, field, montgomery):
    """z in {0, 1, p - 1} at every point index in turn, v in {0, 1} (v = 0 leaves the first column of each point: 0^0 = 1)."""
    P = FIELD_MODULI[field]
    rng = random.Random("open/adversarial")
    points = [[0, 1, P - 1, rng.randrange(P)], [1, P - 1, rng.randrange(P), 0], [P - 1, 0, 1, 1], [rng.randrange(P), P - 1, 0, P - 1]]
    assert run_case(H, field, montgomery, "open/adversarial", 1025 + 7, 4, MASKS, points, [0, 1, 0, 1], key=KEY) == ([0] * 4, [0] * 4)


@pytest.mark.parametrize("montgomery", REPRS, ids=["canonical", "montgomery"])
@pytest.mark.parametrize("field", FIELDS)
def test_128_tiles(H, field, montgomery):
    """2^17 coefficients: three columns, two points (the model stays at a few seconds, and is made once per field)."""
    P = FIELD_MODULI[field]
    rng = random.Random("open/2^17")
    points = [[rng.randrange(P) for _ in range(2)] for _ in range(2)]
    assert run_case(H, field, montgomery, "open/2^17", 1 << 17, 2, (0b11, 0b01, 0b10), points, [rng.randrange(P), rng.randrange(P)]) == ([0, 0], [0, 0])


@pytest.mark.parametrize("montgomery", REPRS, ids=["canonical", "montgomery"])
def test_refused_and_skipped_circuits(H, montgomery):
    """A point >= p (circuit 1) refuses both calls for that circuit, v >= p (circuit 3) the witness alone, a status byte that is nonzero on
    entry (circuit 2) skips it and is left alone; the outputs of such circuits keep their sentinel bytes and the neighbours are computed."""
    from halo2_rsa_amd import _lib
    field = "bn254_fr"
    P = FIELD_MODULI[field]
    rng = random.Random("open/status")
    points = [[rng.randrange(P) for _ in range(4)] for _ in range(5)]
    points[1][3] = P                                       # (a point that only column 2 queries)
    vs = [rng.randrange(P) for _ in range(5)]
    vs[3] = (1 << 256) - 1
    st_ev, st_w = run_case(H, field, montgomery, "open/status", 1030, 5, MASKS, points, vs, key=KEY, statuses=[0, 0, 9, 0, 0], bad=(1, 2))
    assert st_ev == [0, _lib.H2R_E_SHAPE, 9, 0, 0]
    assert st_w == [0, _lib.H2R_E_SHAPE, 9, _lib.H2R_E_SHAPE, 0]


@pytest.mark.parametrize("montgomery", REPRS, ids=["canonical", "montgomery"])
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n,C", [(1, 1), (4, 3), (1000, 4), (1025, 2), (3 * 1024 + 1, 5)])
def test_fold(H, field, montgomery, n, C):
    """s random, 0 (the first column is left: 0^0 = 1), 1, >= p (refused) and a circuit skipped on entry; one column holds p - 1 throughout."""
    from halo2_rsa_amd import _lib
    P = FIELD_MODULI[field]
    dom = domain(H, field, montgomery)
    rng = random.Random("fold/%d/%s" % (n, field))
    B = 5
    cols = [[[P - 1] * n if c == C - 1 else [rng.randrange(P) for _ in range(n)] for c in range(C)] for _ in range(B)]
    s = [rng.randrange(P), 0, 1, P, rng.randrange(P)]
    full_in, cin = guarded((B, C), n)
    cin.copy_(torch.from_numpy(np.stack([np.stack([bytes_of(col, P, montgomery) for col in circ]) for circ in cols])).cuda())
    full, out = guarded((B,), n)
    status = torch.tensor([0, 0, 0, 0, 7], dtype=torch.uint8, device="cuda")
    dom.fold(cin, scalars(s, P, montgomery), out=(out, status))
    torch.cuda.synchronize()
    host = full.cpu().numpy()
    assert status.cpu().tolist() == [0, 0, 0, _lib.H2R_E_SHAPE, 7]
    assert (host[:, n:] == SENTINEL).all() and (host[3] == SENTINEL).all() and (host[4] == SENTINEL).all()
    for e in range(3):
        assert np.array_equal(host[e, :n], bytes_of(OR.fold(cols[e], s[e], P), P, montgomery)), e
    assert np.array_equal(host[1, :n], bytes_of(cols[1][0], P, montgomery))
