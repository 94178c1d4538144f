"""h2r_verify_scalars on the device (verify_scalars_kernel) byte for byte against the plain model (tests/
verify_proof_ref.py: scalars_of -- never the host twin, never prover.verify_proof), bn254_fr in both representations.  Full wavefronts:
batches on either side of a workgroup of 64 circuits, every circuit its own evaluations and challenges, so every column of the LDS tile
and a second and third workgroup are in use, with a fixed set of lanes that return early (a status on entry, a challenge that is not
canonical, x on the domain) or carry edge values beside lanes that run to the end.  Swept shapes: the whole grid of tests/verify_cases.py
at five distinct circuits per shape.  Every output is pre-filled with a sentinel, `right` has a padding row behind every circuit, and
`right`, `left` and `status` lie between guards."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import transcript_ref as T
import verify_cases as VC
import verify_proof_ref as V

REPRS, IDS = [False, True], ["canonical", "montgomery"]
SENTINEL, GUARD, STATUS_GUARD = 0xAB, 2, 64
R = T.R
ENTRY = 7                                         # a status on entry that no kernel raises
WAVE_SHAPES = [(9, 5, 8, 3, 31), (4, 13, 8, 3, 10)]
THETA, BETA, GAMMA, Y, X, V_, U = range(7)
CACHE = {}


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import halo2_rsa_amd as H_
    return H_


def chip_of(H, montgomery):
    if ("chip", montgomery) not in CACHE:
        CACHE[("chip", montgomery)] = H.BigIntChip(64, 256, field="bn254_fr", montgomery=montgomery)
    return CACHE[("chip", montgomery)]


def rep_bytes(vals, montgomery):
    """Integers as they lie in the ctx's memory; one that is no field element has no Montgomery form and stays what it is."""
    return b"".join((T.to_repr(v, R, montgomery) if v < R else v).to_bytes(32, "little") for v in vals)


def dev_bytes(raw, shape):
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).reshape(shape).cuda()


def device(H, montgomery, cfg, circuits, entry=None, shared_evals=False, with_status=True):
    """(right rows [batch] of 32 * num_bases bytes, left rows [batch] of 128 bytes, status list or None) of h2r_verify_scalars on `circuits`
    = [(evaluations, challenges)]; the padding rows, the guards and an untouched status are checked here."""
    from halo2_rsa_amd import _lib
    chip = chip_of(H, montgomery)
    batch = len(circuits)
    vcfg = VC.verify_config(cfg, montgomery)
    ne = ctypes.c_uint32(0)
    nb = _lib.lib().h2r_verify_bases(ctypes.byref(vcfg), ctypes.byref(ne))
    assert nb == len(V.base_index(cfg)) and all(len(ev) == ne.value for ev, _ in circuits)
    assert not shared_evals or batch == 1
    evals = dev_bytes(b"".join(rep_bytes(ev, montgomery) for ev, _ in circuits), (batch, 32 * ne.value))
    chal = dev_bytes(b"".join(rep_bytes([ch[k] for _, ch in circuits], montgomery) for k in range(7)), (7, batch, 32))
    row = 32 * (nb + 1)                                                        # a padding row behind every circuit
    right = torch.full((batch + 2 * GUARD, row), SENTINEL, dtype=torch.uint8, device="cuda")
    left = torch.full((batch + 2 * GUARD, 128), SENTINEL, dtype=torch.uint8, device="cuda")
    status = torch.full((batch + 2 * STATUS_GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    status[STATUS_GUARD:STATUS_GUARD + batch] = torch.tensor(entry if entry is not None else [0] * batch, dtype=torch.uint8, device="cuda")
    ch = _lib.H2RVerifyChallenges(*[chal[k].data_ptr() for k in range(7)])
    _lib.check(_lib.lib().h2r_verify_scalars(chip._ctx, ctypes.byref(vcfg), evals.data_ptr(), 0 if shared_evals else evals.stride(0), ctypes.byref(ch), batch,
                                             right[GUARD].data_ptr(), row, left[GUARD].data_ptr(),
                                             status[STATUS_GUARD:].data_ptr() if with_status else None, chip._stream()), "h2r_verify_scalars")
    torch.cuda.synchronize()
    rt, lf, st = right.cpu().numpy(), left.cpu().numpy(), status.cpu().numpy()
    assert (rt[:GUARD] == SENTINEL).all() and (rt[GUARD + batch:] == SENTINEL).all(), "a write outside right"
    assert (rt[GUARD:GUARD + batch, 32 * nb:] == SENTINEL).all(), "a write into a padding row of right"
    assert (lf[:GUARD] == SENTINEL).all() and (lf[GUARD + batch:] == SENTINEL).all(), "a write outside left"
    assert (st[:STATUS_GUARD] == SENTINEL).all() and (st[STATUS_GUARD + batch:] == SENTINEL).all(), "a write outside status"
    inner = st[STATUS_GUARD:STATUS_GUARD + batch].tolist()
    if not with_status:
        assert inner == (entry if entry is not None else [0] * batch), "a status that was not passed is written"
    return [bytes(r[:32 * nb]) for r in rt[GUARD:GUARD + batch]], [bytes(r) for r in lf[GUARD:GUARD + batch]], inner if with_status else None


def model(cfg, circuit):
    """(status, right, left) of the plain model; a challenge that is not canonical is H2R_E_SHAPE before anything else."""
    evals, ch = circuit
    if any(c >= R for c in ch):
        return T.E_SHAPE, None, None
    return V.scalars_of(cfg, evals, ch)


def compare(got, cfg, circuits, montgomery, what, entry=None):
    """Every circuit against the model: its status; byte-equal rows, or rows that keep the sentinel under a status.  Returns the statuses."""
    right, left, status = got
    pos = V.base_index(cfg)
    names = {at: name for name, at in pos.items()}
    want_status = []
    for e, circuit in enumerate(circuits):
        st, want_right, want_left = (entry[e], None, None) if entry is not None and entry[e] else model(cfg, circuit)
        want_status.append(st)
        if status is not None:
            assert status[e] == st, "%s: the status of circuit %d is %d, the model's %d" % (what, e, status[e], st)
        if st:
            assert right[e] == bytes([SENTINEL]) * len(right[e]) and left[e] == bytes([SENTINEL]) * 128, "%s: the flagged circuit %d is written" % (what, e)
            continue
        want = rep_bytes(want_right, montgomery)
        if right[e] != want:
            at = next(i for i in range(len(want_right)) if right[e][32 * i:32 * i + 32] != want[32 * i:32 * i + 32])
            raise AssertionError("%s: circuit %d, the scalar of base %d %r" % (what, e, at, names[at]))
        assert left[e] == rep_bytes(want_left, montgomery), "%s: circuit %d, the scalars of L" % (what, e)
    return want_status


# ---- full wavefronts -------------------------------------------------------------------------------------------------------------------
def special_lanes(batch, count):
    """`count` circuits of a batch >= 64, fixed per batch: circuit 0, lane 63, lane 64 (the second workgroup's first) and the last circuit
    where the batch has them, the rest spread over every workgroup."""
    lanes = [e for e in (63, 64, batch - 1, 0) if e < batch]
    e = 5
    while len(set(lanes)) < count:
        lanes.append(e)
        e = (e + 37) % batch
    out = []
    for e in lanes:
        if e not in out:
            out.append(e)
    return out


def wave_case(shape, batch):
    """(cfg, circuits, entry statuses, {circuit: what it carries}) of one (shape, batch), made once for both representations."""
    if (shape, batch) in CACHE:
        return CACHE[(shape, batch)]
    cfg = VC.config_of(shape)
    rng = random.Random("verify_scalars/gpu/%s/%d" % (VC.shape_id(shape), batch))
    circuits = [(list(ev), list(ch)) for ev, ch in VC.inputs(rng, cfg, batch)]
    entry, marks = [0] * batch, {}
    if batch >= 64:
        w, ne = cfg.omega(R), len(circuits[0][0])

        def challenge(k, val):
            return lambda e: circuits[e][1].__setitem__(k, val)

        def on_entry(e):
            entry[e] = ENTRY

        def zeros(e):
            for k in (THETA, BETA, GAMMA):
                circuits[e][1][k] = 0

        def all_evals(val):
            return lambda e: circuits[e][0].__setitem__(slice(None), [val] * ne)

        # lane 63 ends on the domain, lane 64 on a challenge, the last circuit runs to the end on edge values; the early returns alternate with the rest
        special = [("x = omega^u", challenge(X, pow(w, cfg.u, R))), ("theta = R + 0", challenge(THETA, R)), ("evaluations all R - 1", all_evals(R - 1)),
                   ("a status on entry", on_entry), ("x = 0", challenge(X, 0)), ("beta = R + 1", challenge(BETA, R + 1)), ("u = 0", challenge(U, 0)),
                   ("gamma = R + 2", challenge(GAMMA, R + 2)), ("theta = beta = gamma = 0", zeros), ("y = R + 3", challenge(Y, R + 3)),
                   ("evaluations all 0", all_evals(0)), ("x = R + 4", challenge(X, R + 4)), ("x = omega^0", challenge(X, 1)), ("v = R + 5", challenge(V_, R + 5)),
                   ("x = omega^(u+1)", challenge(X, pow(w, cfg.u + 1, R))), ("u = R + 6", challenge(U, R + 6)), ("x = omega^(n-1)", challenge(X, pow(w, cfg.n - 1, R))),
                   ("v = 0", challenge(V_, 0)), ("y = 0", challenge(Y, 0))]
        assert cfg.blinding_factors > 0, "omega^(u+1) is a blinding row"
        lanes = special_lanes(batch, len(special))
        assert len(lanes) == len(special) and {63, batch - 1} <= set(lanes) and (batch == 64 or 64 in lanes)
        assert batch < 128 or len({e // 64 for e in lanes}) == (batch + 63) // 64, "a workgroup without a special lane"
        for e, (name, put) in zip(lanes, special):
            put(e)
            marks[e] = name
    CACHE[(shape, batch)] = cfg, circuits, entry, marks
    return CACHE[(shape, batch)]


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
@pytest.mark.parametrize("batch", [1, 64, 65, 130])
@pytest.mark.parametrize("shape", WAVE_SHAPES, ids=[VC.shape_id(s) for s in WAVE_SHAPES])
def test_full_wavefronts(H, shape, batch, montgomery):
    assert shape in VC.GRID
    cfg, circuits, entry, marks = wave_case(shape, batch)
    assert len({tuple(ev) + tuple(ch) for ev, ch in circuits}) == batch, "every circuit has its own evaluations and challenges"
    got = device(H, montgomery, cfg, circuits, entry)
    want = compare(got, cfg, circuits, montgomery, "%s, batch %d" % (VC.shape_id(shape), batch), entry)
    if batch == 1:
        assert want == [0]
        return
    # what the marked lanes are there for, by the model; the device equals the model above
    by_name = {name: e for e, name in marks.items()}
    for name, e in by_name.items():
        st = want[e]
        if name == "a status on entry":
            assert st == ENTRY and got[2][e] == ENTRY, "an entry status is kept"
        elif " = R + " in name:
            assert st == T.E_SHAPE, name
        elif name.startswith("x = omega"):
            assert st == T.E_ASSERTION, name
        else:
            assert st == 0, name
    assert got[1][by_name["u = 0"]] == rep_bytes([1, 0, 0, 0], montgomery)
    assert sum(1 for st in want if st == 0) >= batch - 14 and sum(1 for st in want if st) == 12
    assert all(want[e] == 0 for e in range(batch) if e not in marks), "a drawn circuit has a status"


# ---- swept shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
@pytest.mark.parametrize("domain", VC.DOMAINS, ids=["k%d-bf%d" % d for d in VC.DOMAINS])
def test_the_grid(H, domain, montgomery):
    shapes = VC.shapes(domain)
    assert len(shapes) == len(VC.COLUMNS) * len(VC.MASKS)
    for shape in shapes:
        sid = VC.shape_id(shape)
        if ("grid", shape) not in CACHE:
            cfg = VC.config_of(shape)
            CACHE[("grid", shape)] = cfg, VC.inputs(random.Random("verify_scalars/gpu/grid/" + sid), cfg, 5)
        cfg, circuits = CACHE[("grid", shape)]
        assert len({tuple(ev) + tuple(ch) for ev, ch in circuits}) == 5
        want = compare(device(H, montgomery, cfg, circuits), cfg, circuits, montgomery, sid)
        assert want == [0] * 5, "%s: the model flags a drawn circuit" % sid


# ---- other cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_one_circuit_with_an_evaluation_stride_of_zero(H, montgomery):
    shape = (5, 5, 7, 6, 16)
    assert shape in VC.GRID
    cfg = VC.config_of(shape)
    circuits = VC.inputs(random.Random("verify_scalars/gpu/stride0"), cfg, 1)
    assert compare(device(H, montgomery, cfg, circuits, shared_evals=True), cfg, circuits, montgomery, "evals_stride = 0") == [0]


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_a_null_status_pointer(H, montgomery):
    shape = (3, 6, 8, 3, 10)
    assert shape in VC.GRID
    cfg = VC.config_of(shape)
    circuits = [(list(ev), list(ch)) for ev, ch in VC.inputs(random.Random("verify_scalars/gpu/nullstatus"), cfg, 4)]
    circuits[1][1][X] = pow(cfg.omega(R), cfg.u, R)                               # x on the domain: nothing to report to, nothing written
    circuits[2][1][V_] = R                                                        # a challenge that is not canonical: likewise
    got = device(H, montgomery, cfg, circuits, with_status=False)
    assert got[2] is None
    assert compare(got, cfg, circuits, montgomery, "status = NULL") == [0, T.E_ASSERTION, T.E_SHAPE, 0]
