"""The generator of the blinding values on the device (h2r_random_columns through prover.random_columns) byte for
byte against hashlib (tests/create_proof_ref.py): row ranges around the wavefront and the 256-row tile and the tails create_proof draws
(u..n of a k = 10 column), one and several circuits, one and seven columns whose element strides differ, a column the batch shares, a
first circuit other than 0, both representations.  Every column lies in a sentinel-filled buffer with rows before and behind the range:
the whole buffer is compared, so a row written outside the range fails the case.  The model's values are made once per (circuit, tag,
row) and shared."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import create_proof_ref as C
from transcript_ref import R, to_repr

SEED = bytes(range(7, 39))
RANGES = [(0, 1), (0, 63), (0, 64), (0, 65), (250, 257), (1018, 1024)]
SENTINEL, N = 0xAB, 1024
TAGS7 = [C.tag(C.KIND_ADVICE, 0), C.tag(C.KIND_ADVICE, 4), C.tag(C.KIND_LOOKUP_A_PERM, 2), C.tag(C.KIND_LOOKUP_S_PERM, 2), C.tag(C.KIND_PERM_Z, 1),
         C.tag(C.KIND_LOOKUP_Z, 3), C.tag(C.KIND_RANDOM_POLY)]


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import halo2_rsa_amd as H_
    return H_


@pytest.fixture(scope="module", params=[False, True], ids=["canonical", "montgomery"])
def chip(H, request):
    return H.BigIntChip(64, 256, field="bn254_fr", montgomery=request.param)


@functools.lru_cache(maxsize=None)
def element_bytes(circuit, tag, row, montgomery):
    return np.frombuffer(to_repr(C.random_element(SEED, circuit, tag, row), R, montgomery).to_bytes(32, "little"), dtype=np.uint8)


def buffers(batch, num_cols, shared=()):
    """Sentinel-filled columns: column c of a batch has N + 3 c + 2 rows per circuit (so the element strides differ), a shared one is [rows, 32]."""
    return [torch.full(((N + 3 * c + 2, 32) if c in shared else (batch, N + 3 * c + 2, 32)), SENTINEL, dtype=torch.uint8, device="cuda") for c in range(num_cols)]


def expected(buf, tags, rows, first_circuit, montgomery):
    want = []
    for t, tag in zip(buf, tags):
        w = np.full(tuple(t.shape), SENTINEL, dtype=np.uint8)
        for e in range(t.shape[0] if t.dim() == 3 else 1):
            for i in range(*rows):
                (w[e] if t.dim() == 3 else w)[i] = element_bytes(first_circuit + e, tag, i, montgomery)
        want.append(w)
    return want


def assert_equal(buf, want):
    torch.cuda.synchronize()
    for c, (t, w) in enumerate(zip(buf, want)):
        got = t.cpu().numpy()
        assert np.array_equal(got, w), "column %d: %d rows differ" % (c, int((got != w).any(axis=-1).sum()))


@pytest.mark.parametrize("rows", RANGES, ids=["%d-%d" % r for r in RANGES])
def test_the_rows_of_the_range_and_nothing_else(H, chip, rows):
    for batch in (1, 3):
        for num_cols in (1, 7):
            buf, tags = buffers(batch, num_cols), TAGS7[:num_cols]
            assert num_cols == 1 or len({t.stride(0) for t in buf}) == num_cols
            H.prover.random_columns(chip, buf, tags, rows, SEED)
            assert_equal(buf, expected(buf, tags, rows, 0, chip.montgomery))


def test_a_shared_column_and_a_first_circuit(H, chip):
    buf = buffers(3, 3, shared=(1,))
    tags = TAGS7[4:7]
    H.prover.random_columns(chip, buf, tags, (250, 257), SEED, first_circuit=5)
    want = expected(buf, tags, (250, 257), 5, chip.montgomery)
    assert_equal(buf, want)
    assert not np.array_equal(want[0][0, 250], want[0][1, 250])               # circuits 5 and 6 draw different values ...
    one = buffers(1, 1)
    H.prover.random_columns(chip, one, tags[:1], (250, 257), SEED, first_circuit=6)
    torch.cuda.synchronize()
    assert torch.equal(one[0][0], buf[0][1])                                  # ... and circuit 6 alone draws what it drew in the batch


def test_two_launches_that_split_a_range_equal_one(H, chip):
    whole, parts = buffers(3, 2), buffers(3, 2)
    H.prover.random_columns(chip, whole, TAGS7[:2], (0, 600), SEED)
    H.prover.random_columns(chip, parts, TAGS7[:2], (0, 257), SEED)
    H.prover.random_columns(chip, parts, TAGS7[:2], (257, 600), SEED)
    torch.cuda.synchronize()
    for a, b in zip(whole, parts):
        assert torch.equal(a, b) and bool((a[:, 600:] == SENTINEL).all()) and not bool((a[:, :600] == SENTINEL).all(dim=-1).any())
    # rows 0, 255, 256 and 599 of circuit 2 against the model: the tile boundary and the last row
    got = whole[1][2].cpu().numpy()
    for i in (0, 255, 256, 599):
        assert np.array_equal(got[i], element_bytes(2, TAGS7[1], i, chip.montgomery)), i


def test_an_empty_range_and_the_wrapper_refusals(H, chip):
    from halo2_rsa_amd import _lib
    buf = buffers(2, 1)
    H.prover.random_columns(chip, buf, TAGS7[:1], (9, 9), SEED)
    torch.cuda.synchronize()
    assert bool((buf[0] == SENTINEL).all())
    short = dict(rows=(0, buf[0].shape[1] + 1))                              # one row more than the column has: refused, never launched
    for kw in (dict(tags=[]), dict(seed=SEED[:31]), dict(rows=(5, 4)), dict(columns=[]), short, dict(columns=[buf[0].view(torch.int8)]),
               dict(columns=[buf[0].cpu()]), dict(columns=[buf[0][:, :, :16]])):
        args = dict(columns=buf, tags=TAGS7[:1], rows=(0, 4), seed=SEED)
        args.update(kw)
        with pytest.raises(_lib.H2RError) as err:
            H.prover.random_columns(chip, **args)
        assert err.value.code == _lib.H2R_E_SHAPE
    other = H.BigIntChip(64, 256, field="pasta_fq")
    with pytest.raises(_lib.H2RError) as err:
        H.prover.random_columns(other, buf, TAGS7[:1], (0, 4), SEED)
    assert err.value.code == _lib.H2R_E_SHAPE
    assert bool((buf[0] == SENTINEL).all())
