"""The Fiat-Shamir transcript on the device (prover.Transcript: h2r_transcript_round) byte for byte against the plain
model (tests/transcript_ref.py: hashlib and Python integers) -- challenges, derived values, the proof buffer, and of every state record
the byte counter, the fill and the pending block bytes -- bn254_fr in both representations, different data in every circuit.  A script is a
list of rounds; a round's items are (kind, values, shared): values[e][k] per circuit, or values[k] for one copy the batch shares."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import transcript_ref as T

Q, R = T.Q, T.R
REPRS, IDS = [False, True], ["canonical", "montgomery"]
SENTINEL = 0xAB
SENTINEL_WORD = int.from_bytes(bytes([SENTINEL]) * 8, "little", signed=True)
OMEGA17 = pow(7, (R - 1) >> 17, R)
CACHE = {}                      # the model's results, shared by the two representations


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import halo2_rsa_amd as H_
    return H_


def chip_of(H, montgomery):
    return H.BigIntChip(64, 256, field="bn254_fr", montgomery=montgomery)


def item_tensor(kind, values, shared, montgomery):
    """int64 [batch, count, 2, 4] / [batch, count, 4] per circuit, [count, 2, 4] / [count, 4] shared: the ctx's bytes of the values."""
    rows = [values] if shared else values
    raw = b"".join(T.item_repr_bytes(kind, v, montgomery) for row in rows for v in row)
    t = torch.frombuffer(bytearray(raw), dtype=torch.int64).reshape((len(rows), len(rows[0])) + ((2, 4) if kind == "point" else (4,)))
    return (t[0] if shared else t).cuda()


def words_bytes(t):
    return t.cpu().numpy().tobytes()


def run_script(H, montgomery, name, batch, script, statuses=None):
    """Runs the rounds on one Transcript and on `batch` models; compares everything after every round.  Returns the transcript."""
    chip = chip_of(H, montgomery)
    total = 32 * sum(len(vals if shared else vals[0]) for items, _, _, common in script for _, vals, shared in items if not common)
    tr = H.Transcript(chip, batch, total + 32)
    if (name, batch) not in CACHE:   # the model's whole run, once
        models, runs = [T.Transcript() for _ in range(batch)], []
        for items, squeeze, derive, common in script:
            res = [m.round([(kind, v) for kind, vals, shared in items for v in (vals if shared else vals[e])], squeeze, derive, common)
                   for e, m in enumerate(models)]
            assert all(st == 0 for st, _, _ in res)
            runs.append([(c, d, m.proof, m.pending()) for (_, c, d), m in zip(res, models)])
        CACHE[(name, batch)] = runs
    runs = CACHE[(name, batch)]
    status = torch.zeros(batch, dtype=torch.uint8, device="cuda")
    for r, (items, squeeze, derive, common) in enumerate(script):
        tensors = [(item_tensor(kind, vals, shared, montgomery), kind) for kind, vals, shared in items]
        ch, dv = tr.round(tensors, squeeze, [(s, T.to_repr(m, R, montgomery), l) for s, m, l in derive], common, status)
        got_ch, got_dv = words_bytes(ch), words_bytes(dv)
        for e in range(batch):
            c, d, _, _ = runs[r][e]
            exp_c = b"".join(T.to_repr(v, R, montgomery).to_bytes(32, "little") for v in c)
            exp_d = b"".join(T.to_repr(v, R, montgomery).to_bytes(32, "little") for v in d)
            assert got_ch[e * squeeze * 32:(e + 1) * squeeze * 32] == exp_c, (name, r, e)
            assert got_dv[e * len(derive) * 32:(e + 1) * len(derive) * 32] == exp_d, (name, r, e)
    proof, buf, states = tr.proof().cpu().numpy(), tr.buffer.cpu().numpy(), tr.states.cpu().numpy()
    assert status.cpu().tolist() == [0] * batch and tr.offset == total
    last = runs[-1]
    for e in range(batch):
        _, _, want_proof, (done, block) = last[e]
        assert proof[e].tobytes() == want_proof and len(want_proof) == total, (name, e)
        assert not buf[e, total:].any(), "bytes behind the proof were written"
        raw = states[e].tobytes()
        assert int.from_bytes(raw[64:72], "little") == done and int.from_bytes(raw[72:80], "little") == len(block) and raw[80:80 + len(block)] == block
    return tr


def rand_point(rng):
    return (rng.randrange(Q), rng.randrange(Q))


def per_circuit(rng, batch, count, kind):
    return [[rand_point(rng) if kind == "point" else rng.randrange(R) for _ in range(count)] for _ in range(batch)]


@pytest.mark.parametrize("batch", [1, 3, 64, 65, 130])
@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_a_run_of_rounds(H, montgomery, batch):
    rng = random.Random("transcript/gpu/run/%d" % batch)
    script = [
        ([("scalar", [rng.randrange(R)], True)], 0, [], True),                                    # the init round: a common scalar of stride 0
        ([("point", per_circuit(rng, batch, 5, "point"), False), ("scalar", per_circuit(rng, batch, 1, "scalar"), False)], 1, [], False),
        ([], 2, [], False),
        ([("scalar", per_circuit(rng, batch, 46, "scalar"), False)], 1,
         [(0, OMEGA17, 0), (0, pow(OMEGA17, -1, R), 0), (0, 1, 17), (0, R - 1, 1)], False),
    ]
    run_script(H, montgomery, "run", batch, script)


def squeezes(n):
    return [([], min(8, n - k), [], False) for k in range(0, n, 8)]


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_block_boundaries(H, montgomery):
    """The host test's cases at batch 3: challenges finalised on 127, 128, 129 and on 255, 256, 257 bytes, a point that straddles a block
    boundary from offset 100, a scalar that ends exactly on one, and a squeeze as the first operation."""
    batch = 3
    rng = random.Random("transcript/gpu/boundaries")
    run_script(H, montgomery, "one-point", batch, [([("point", per_circuit(rng, batch, 1, "point"), False)], 0, [], False)] + squeezes(72))
    run_script(H, montgomery, "three-points", batch, [([("point", per_circuit(rng, batch, 3, "point"), False)], 0, [], True)] + squeezes(66))
    edge = [[0, 1, R - 1]] * batch
    run_script(H, montgomery, "straddle", batch,
               [([("scalar", edge, False)], 1, [], False),                                         # 100 bytes
                ([("point", [[(Q - 1, Q - 2)], [(1, 2)], [(0, 1)]], False)], 0, [], False)]        # bytes 100..164
               + squeezes(58) +
               [([("scalar", per_circuit(rng, batch, 1, "scalar"), False)], 0, [], False),         # ends exactly on 256
                ([], 1, [], False),
                ([("scalar", [3], True), ("point", [(2, 5)], True)], 1, [(0, 1, 1)], False)])
    run_script(H, montgomery, "empty", batch, [([], 1, [], False), ([], 2, [(1, OMEGA17, 0)], False)])


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_status(H, montgomery):
    """A nonzero status on entry leaves that circuit's state, proof bytes and outputs as they were (sentinel bytes), its neighbours go on;
    one (0, 0) point or one non-canonical scalar marks that circuit alone, and the round leaves it untouched."""
    batch = 5
    rng = random.Random("transcript/gpu/status")
    chip = chip_of(H, montgomery)
    tr = H.Transcript(chip, batch, 4 * 32)
    models = [T.Transcript() for _ in range(batch)]
    first = per_circuit(rng, batch, 1, "scalar")
    status = torch.zeros(batch, dtype=torch.uint8, device="cuda")
    tr.round([item_tensor("scalar", first, False, montgomery)], 0, (), False, status)
    for e in range(batch):
        models[e].round([("scalar", first[e][0])])
    # circuit 1 is skipped on entry; its records are filled with sentinel bytes (a skipped circuit's state is nobody's to read)
    status[1] = 7
    tr.states[1] = SENTINEL
    tr.buffer[1] = SENTINEL
    pts = per_circuit(rng, batch, 2, "point")
    pts[2][1] = (0, 0)                                                        # circuit 2: the point at infinity
    scal = per_circuit(rng, batch, 1, "scalar")
    scal[3][0] = R                                                            # circuit 3: a scalar that is not canonical
    before = tr.states.clone()
    ch = torch.full((batch, 2, 4), SENTINEL_WORD, dtype=torch.int64, device="cuda")
    dv = torch.full((batch, 1, 4), SENTINEL_WORD, dtype=torch.int64, device="cuda")
    tr.round([item_tensor("point", pts, False, montgomery), item_tensor("scalar", scal, False, montgomery)], 2,
             [(1, T.to_repr(OMEGA17, R, montgomery), 1)], False, status, out=(ch, dv))
    assert status.cpu().tolist() == [0, 7, T.E_ASSERTION, T.E_SHAPE, 0]
    states, proof, got_ch, got_dv = tr.states.cpu().numpy(), tr.buffer.cpu().numpy(), ch.cpu().numpy(), dv.cpu().numpy()
    for e in range(batch):
        if e in (1, 2, 3):
            assert states[e].tobytes() == before[e].cpu().numpy().tobytes(), e
            assert got_ch[e].tobytes() == bytes([SENTINEL]) * 64 and got_dv[e].tobytes() == bytes([SENTINEL]) * 32, e
            assert proof[e, 32:].tobytes() == (bytes([SENTINEL]) if e == 1 else bytes(1)) * 96, e
            assert (proof[e, :32] == SENTINEL).all() if e == 1 else proof[e, :32].tobytes() == models[e].proof
            continue
        st, c, d = models[e].round([("point", p) for p in pts[e]] + [("scalar", scal[e][0])], 2, [(1, OMEGA17, 1)])
        assert st == 0
        assert got_ch[e].tobytes() == b"".join(T.to_repr(v, R, montgomery).to_bytes(32, "little") for v in c), e
        assert got_dv[e].tobytes() == T.to_repr(d[0], R, montgomery).to_bytes(32, "little"), e
        assert proof[e].tobytes() == models[e].proof, e
    # the marked circuits stay skipped, the others go on
    c2, _ = tr.round([], 1, (), False, status)
    got = c2.cpu().numpy()
    for e in (0, 4):
        assert got[e].tobytes() == T.to_repr(models[e].squeeze(), R, montgomery).to_bytes(32, "little")
    assert not got[1:4].any()


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_two_transcripts_on_one_stream_are_independent(H, montgomery):
    batch = 3
    rng = random.Random("transcript/gpu/two")
    chip = chip_of(H, montgomery)
    a, b = H.Transcript(chip, batch, 64), H.Transcript(chip, batch, 64)
    ma, mb = [T.Transcript() for _ in range(batch)], [T.Transcript() for _ in range(batch)]
    xs, ys = per_circuit(rng, batch, 1, "point"), per_circuit(rng, batch, 2, "scalar")
    ca1, _ = a.write_points(item_tensor("point", xs, False, montgomery), squeeze=1)
    cb1, _ = b.write_scalars(item_tensor("scalar", ys, False, montgomery), squeeze=1)
    ca2, _ = a.common_scalars(item_tensor("scalar", ys, False, montgomery), squeeze=1)
    cb2, _ = b.common_points(item_tensor("point", xs, False, montgomery), squeeze=1)
    got = [t.cpu().numpy() for t in (ca1, cb1, ca2, cb2)]
    for e in range(batch):
        wa1 = ma[e].round([("point", xs[e][0])], 1)[1][0]
        wb1 = mb[e].round([("scalar", s) for s in ys[e]], 1)[1][0]
        wa2 = ma[e].round([("scalar", s) for s in ys[e]], 1, common=True)[1][0]
        wb2 = mb[e].round([("point", xs[e][0])], 1, common=True)[1][0]
        for g, w in zip(got, (wa1, wb1, wa2, wb2)):
            assert g[e].tobytes() == T.to_repr(w, R, montgomery).to_bytes(32, "little"), e
    pa, pb = a.proof().cpu().numpy(), b.proof().cpu().numpy()
    for e in range(batch):
        assert pa[e].tobytes() == ma[e].proof and pb[e].tobytes() == mb[e].proof and len(ma[e].proof) == 32 and len(mb[e].proof) == 64
