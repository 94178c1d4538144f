"""Plain model of the Fiat-Shamir transcript (h2r_transcript_round, h2r_transcript_eval): halo2's Blake2bWrite over
bn256 G1Affine with Challenge255, as the reference's only prover configuration uses it.  The hash is Python's hashlib -- a true oracle, not
a restatement of the library's compression function -- and everything else is Python integers.  The framing (prefix bytes, x before y, the
compressed encoding) is a restatement of halo2 and halo2curves [3P], not pinned against them.  Nothing here is shared with the library.

Items are ("point", (x, y)) or ("scalar", s), canonical integers; a Montgomery ctx's bytes are made by the tests."""
import hashlib

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583       # bn256 Fq: the coordinates
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617       # bn256 Fr: scalars and challenges
R256 = 1 << 256
PERSON = b"Halo2-Transcript"
E_SHAPE, E_ASSERTION = 1, 9                      # H2R_E_SHAPE, H2R_E_ASSERTION
PREFIX_CHALLENGE, PREFIX_POINT, PREFIX_SCALAR = b"\x00", b"\x01", b"\x02"


def new_hash(person=PERSON):
    return hashlib.blake2b(digest_size=64, person=person)


def reduce_wide(digest: bytes) -> int:
    """from_bytes_wide: the 64 digest bytes as a little-endian 512-bit integer, modulo r."""
    assert len(digest) == 64
    return int.from_bytes(digest, "little") % R


def item_status(kind, v) -> int:
    """What the item does to its circuit: 0, E_SHAPE (a value >= its modulus) or E_ASSERTION (the point at infinity)."""
    if kind == "point":
        if v[0] >= Q or v[1] >= Q:
            return E_SHAPE
        return E_ASSERTION if v == (0, 0) else 0
    return E_SHAPE if v >= R else 0


def absorbed_bytes(kind, v) -> bytes:
    if kind == "point":
        return PREFIX_POINT + v[0].to_bytes(32, "little") + v[1].to_bytes(32, "little")
    return PREFIX_SCALAR + v.to_bytes(32, "little")


def proof_bytes(kind, v) -> bytes:
    """A written scalar: its 32 bytes.  A written point: x with bit 7 of byte 31 = the lowest bit of y."""
    if kind == "point":
        return (v[0] | ((v[1] & 1) << 255)).to_bytes(32, "little")
    return v.to_bytes(32, "little")


class Transcript:
    """One circuit's transcript: the running hash, the proof written so far, and how many bytes went in."""

    def __init__(self):
        self.h = new_hash()
        self.proof = b""
        self.absorbed = 0
        self.tail = b""          # every absorbed byte (the tests' inputs are small): what the pending block is cut from

    def _update(self, data: bytes):
        self.h.update(data)
        self.absorbed += len(data)
        self.tail += data

    def round(self, items, squeeze=0, derive=(), common=False):
        """(status, challenges, derived).  A status leaves the transcript as it was (the first bad item in item order decides)."""
        for kind, v in items:
            st = item_status(kind, v)
            if st:
                return st, None, None
        for kind, v in items:
            self._update(absorbed_bytes(kind, v))
            if not common:
                self.proof += proof_bytes(kind, v)
        ch = [self.squeeze() for _ in range(squeeze)]
        return 0, ch, [mult * pow(ch[src], 1 << log2_pow, R) % R for src, mult, log2_pow in derive]

    def squeeze(self) -> int:
        self._update(PREFIX_CHALLENGE)
        return reduce_wide(self.h.copy().digest())

    def pending(self):
        """(bytes compressed so far, the bytes waiting in the block): a full block waits until more input arrives."""
        done = 0 if self.absorbed == 0 else (self.absorbed - 1) // 128 * 128
        return done, self.tail[done:]


def to_repr(v: int, modulus: int, montgomery: bool) -> int:
    return v * R256 % modulus if montgomery else v


def from_repr(v: int, modulus: int, montgomery: bool) -> int:
    return v * pow(R256, -1, modulus) % modulus if montgomery else v


def item_repr_bytes(kind, v, montgomery: bool) -> bytes:
    """The item as it lies in the ctx's memory.  A value that is not canonical has no Montgomery form: it is given as it is."""
    def enc(x, m):
        return (to_repr(x, m, montgomery) if x < m else x).to_bytes(32, "little")
    return enc(v[0], Q) + enc(v[1], Q) if kind == "point" else enc(v, R)
