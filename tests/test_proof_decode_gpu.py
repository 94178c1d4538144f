"""h2r_proof_decode on the device against the plain model (tests/verify_proof_ref.py: decode_item), bn254_fr in both
representations: batches on either side of a workgroup of 64 circuits, a section list of a single item, statuses that several lanes of one
circuit raise (H2R_E_SHAPE wins over H2R_E_ASSERTION wherever the two occur), circuits flagged on entry, outputs between guards."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import create_proof_ref as C
import msm_ref as M
import transcript_ref as T
import verify_proof_ref as V

REPRS, IDS = [False, True], ["canonical", "montgomery"]
SENTINEL = 0xAB
Q, R = T.Q, T.R
LAYOUT = [("point", 3), ("scalar", 2), ("point", 1)]
CACHE = {}


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import halo2_rsa_amd as H_
    return H_


def pool():
    """Real points (both parities of y occur), an abscissa of no point."""
    if "pool" not in CACHE:
        pts = M.mul_g_batch(range(2, 26))
        assert {p[1] & 1 for p in pts} == {0, 1}
        CACHE["pool"] = pts, next(x for x in range(2, 100) if C.decompress(x.to_bytes(32, "little")) is None)
    return CACHE["pool"]


def item_of(kind, rng):
    pts, _ = pool()
    return T.proof_bytes("point", rng.choice(pts)) if kind == "point" else rng.randrange(R).to_bytes(32, "little")


def decode(H, montgomery, layout, proofs, status_in=None):
    """The device's (points, scalars, status) of `proofs` (a list of byte strings), outputs pre-filled with the sentinel."""
    from halo2_rsa_amd import _lib
    chip = H.BigIntChip(64, 256, field="bn254_fr", montgomery=montgomery)
    batch, np_, ns = len(proofs), sum(c for k, c in layout if k == "point"), sum(c for k, c in layout if k == "scalar")
    dev = torch.frombuffer(bytearray(b"".join(proofs)), dtype=torch.uint8).reshape(batch, -1).cuda()
    points = torch.full((batch, max(np_, 1), 64), SENTINEL, dtype=torch.uint8, device="cuda")
    scalars = torch.full((batch, max(ns, 1), 32), SENTINEL, dtype=torch.uint8, device="cuda")
    status = torch.tensor(status_in if status_in is not None else [0] * batch, dtype=torch.uint8, device="cuda")
    sec = (_lib.H2RProofSection * len(layout))(*[_lib.H2RProofSection(1 if k == "point" else 2, c) for k, c in layout])
    cfg = _lib.H2RProofDecodeConfig(struct_size=ctypes.sizeof(_lib.H2RProofDecodeConfig), num_sections=len(layout), reserved=0)
    _lib.check(_lib.lib().h2r_proof_decode(chip._ctx, ctypes.byref(cfg), sec, dev.data_ptr(), dev.stride(0), batch, points.data_ptr() if np_ else None,
                                           points.stride(0), scalars.data_ptr() if ns else None, scalars.stride(0), status.data_ptr(), chip._stream()), "h2r_proof_decode")
    torch.cuda.synchronize()
    return points.cpu().numpy(), scalars.cpu().numpy(), status.cpu().tolist()


def model(layout, proof, montgomery):
    """(status, the points' bytes, the scalars' bytes) as they lie in the ctx's memory."""
    status, pts, scs, off = 0, b"", b"", 0
    for kind, count in layout:
        for _ in range(count):
            st, val = V.decode_item(kind, proof[off:off + 32])
            off += 32
            status = T.E_SHAPE if T.E_SHAPE in (st, status) else max(st, status)
            if not st:
                raw = T.item_repr_bytes(kind, val, montgomery)
                pts, scs = (pts + raw, scs) if kind == "point" else (pts, scs + raw)
    return status, pts, scs


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
@pytest.mark.parametrize("batch", [1, 64, 65, 130])
def test_batches_on_either_side_of_a_workgroup(H, montgomery, batch):
    rng = random.Random("decode/%d" % batch)
    _, no_point = pool()
    items = sum(c for _, c in LAYOUT)
    proofs = [b"".join(item_of(k, rng) for k, c in LAYOUT for _ in range(c)) for _ in range(batch)]

    def put(e, item, val):
        proofs[e] = proofs[e][:32 * item] + val.to_bytes(32, "little") + proofs[e][32 * item + 32:]

    last = batch - 1
    bad = {}
    if batch > 1:
        put(last, 5, no_point | 1 << 255)                      # one lane: an assertion in the last circuit
        put(batch // 2, 0, no_point)
        put(batch // 2, 2, no_point)                           # two lanes raise the same code
        put(1, 0, no_point)
        put(1, 5, Q)                                           # an assertion and a shape: the shape wins ...
        put(2, 0, Q | 1 << 255)
        put(2, 5, no_point)                                    # ... in either item order
        put(3, 3, R)
        put(3, 4, (1 << 256) - 1)                              # two scalars out of range
        put(4, 1, 0)
        put(4, 3, 0)
        put(4, 4, R - 1)                                       # edge values that decode (x = 0 may or may not be a point: the model says)
        bad = {last, batch // 2, 1, 2, 3}
    entry = [0] * batch
    if batch > 5:
        entry[5] = 7                                           # flagged on entry: skipped
    points, scalars, status = decode(H, montgomery, LAYOUT, proofs, entry)
    for e in range(batch):
        want_st, pts, scs = model(LAYOUT, proofs[e], montgomery)
        if entry[e]:
            assert status[e] == entry[e] and (points[e] == SENTINEL).all() and (scalars[e] == SENTINEL).all(), e
            continue
        assert status[e] == want_st, (e, status[e], want_st)
        assert (want_st != 0) == (e in bad) or e == 4
        if not want_st:
            assert bytes(points[e].reshape(-1)) == pts and bytes(scalars[e].reshape(-1)) == scs, e
    assert len(set(status)) > 1 or batch == 1


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_a_section_list_of_a_single_item(H, montgomery):
    pts, no_point = pool()
    for kind, vals in (("point", [T.proof_bytes("point", pts[0]), T.proof_bytes("point", M.neg(pts[0])), (1).to_bytes(32, "little"), no_point.to_bytes(32, "little"),
                                  (Q - 1).to_bytes(32, "little"), ((1 << 255) - 1).to_bytes(32, "little")]),
                       ("scalar", [(0).to_bytes(32, "little"), (R - 1).to_bytes(32, "little"), R.to_bytes(32, "little"), b"\xff" * 32])):
        points, scalars, status = decode(H, montgomery, [(kind, 1)], vals)
        for e, raw in enumerate(vals):
            want_st, p, s = model([(kind, 1)], raw, montgomery)
            got = points[e] if kind == "point" else scalars[e]
            assert status[e] == want_st, (kind, e)
            assert bytes(got.reshape(-1)) == ((p or s) if not want_st else bytes([SENTINEL]) * got.size), (kind, e)
        assert (points == SENTINEL).all() if kind == "scalar" else (scalars == SENTINEL).all()
