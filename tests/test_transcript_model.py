"""The plain model of the transcript (tests/transcript_ref.py) held to facts from outside it: what hashlib's BLAKE2b is (RFC 7693), that a
streamed hash is the hash of the whole, and that the wide reduction is the integer's remainder.  The model's parameters are then checked
against the library's own constants, so that this file fails where the transcript does not exist."""
import hashlib
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transcript_ref as T
from halo2_rsa_amd import _lib

RFC7693_ABC = ("ba80a53f981c4d0d6a2797b69f12f6e94c212f14685ac4b74b12bb6fdbffa2d1"
               "7d87c5392aab792dc252d5de4533cc9518d38aa8dbf1925ab92386edd4009923")


def test_hashlib_blake2b_is_rfc7693():
    assert hashlib.blake2b(b"abc", digest_size=64).hexdigest() == RFC7693_ABC                  # RFC 7693 appendix A
    assert T.new_hash(person=b"").copy().digest() == hashlib.blake2b(b"", digest_size=64).digest()
    h = T.new_hash(person=b"")
    h.update(b"abc")
    assert h.hexdigest() == RFC7693_ABC
    assert T.new_hash().digest() != T.new_hash(person=b"").digest() and len(T.PERSON) == 16   # the personalisation matters, and fills its field


def test_absorbing_in_pieces_equals_absorbing_at_once():
    rng = random.Random("transcript/model/pieces")
    for total in (0, 1, 64, 65, 127, 128, 129, 255, 256, 257, 1000):
        data = bytes(rng.randrange(256) for _ in range(total))
        whole = T.new_hash()
        whole.update(data)
        for _ in range(4):
            h, off = T.new_hash(), 0
            while off < total:
                n = rng.choice((1, 33, 65, 128))
                h.update(data[off:off + n])
                off += n
            assert h.digest() == whole.digest(), total
    # a squeeze finalises a copy: the running hash goes on as if nobody had looked
    t = T.Transcript()
    t.round([("scalar", 5)])
    before = t.h.copy()
    c = t.squeeze()
    before.update(b"\x00")
    assert c == T.reduce_wide(before.digest()) and t.h.digest() == before.digest() and t.absorbed == 34


def test_wide_reduction_is_the_remainder():
    rng = random.Random("transcript/model/wide")
    for d in [bytes(64), b"\xff" * 64, T.R.to_bytes(64, "little"), (T.R - 1).to_bytes(64, "little"), (T.R << 256).to_bytes(64, "little")] + \
             [bytes(rng.randrange(256) for _ in range(64)) for _ in range(16)]:
        v = int.from_bytes(d, "little")
        assert T.reduce_wide(d) == v % T.R
        d0, d1 = v & (T.R256 - 1), v >> 256                                                     # the halves the library multiplies by R^2 and R^3
        assert T.reduce_wide(d) == (d0 + d1 * T.R256) % T.R


def test_framing_and_encoding():
    assert T.absorbed_bytes("point", (1, 2)) == b"\x01" + (1).to_bytes(32, "little") + (2).to_bytes(32, "little")
    assert T.absorbed_bytes("scalar", 7) == b"\x02" + (7).to_bytes(32, "little")
    assert T.proof_bytes("point", (1, 2))[31] == 0 and T.proof_bytes("point", (1, 3))[31] == 0x80
    assert T.proof_bytes("point", (T.Q - 1, 1))[31] == ((T.Q - 1) >> 248) | 0x80               # q < 2^254: the top bit is free
    assert T.item_status("point", (0, 0)) == _lib.H2R_E_ASSERTION == T.E_ASSERTION
    assert T.item_status("scalar", T.R) == _lib.H2R_E_SHAPE == T.E_SHAPE and T.item_status("point", (T.Q, 1)) == T.E_SHAPE
    t = T.Transcript()
    assert t.pending() == (0, b"")
    t.round([("point", (1, 2))] * 2, common=True)                                               # 130 bytes: one block compressed
    assert t.pending() == (128, t.tail[128:]) and t.proof == b""
    t2 = T.Transcript()
    t2._update(bytes(128))
    assert t2.pending() == (0, bytes(128))                                                      # a full block waits
    # the library's numbers for the same things
    assert (_lib.H2R_TRANSCRIPT_POINT, _lib.H2R_TRANSCRIPT_SCALAR) == (T.PREFIX_POINT[0], T.PREFIX_SCALAR[0])
    assert _lib.lib().h2r_transcript_state_bytes() % 16 == 0
