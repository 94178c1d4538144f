"""Plain model of this library's vk_repr, over hashlib: BLAKE2b-512 with the personalisation "H2R-VerifyKey-v1"
over a fixed little-endian serialisation of the constraint system's configuration and of the key's commitments, the digest reduced as a
little-endian integer modulo r.  Every field element goes in as its CANONICAL integer, so the value does not depend on the representation
a context works in.  The two plans of h2r_verify_scalars_config are derived from the rest and are not hashed."""
import hashlib

PERSON = b"H2R-VerifyKey-v1"
FIELDS = {"bn254_fr": 0, "bn254_fq": 1, "pasta_fp": 2, "pasta_fq": 3}


def le32(v):
    return int(v).to_bytes(4, "little")


def message(field, log_n, blinding_factors, num_fixed, column_src, chunk_len, lookup_mask, gate_fixed, lookup_advice, lookup_tag, lookup_enable,
            table_tag, table_value, omega, delta, extended_k, points) -> bytes:
    """The hashed bytes.  field: the index of FIELDS; omega, delta: canonical integers; points: num_fixed fixed commitments, then one
    sigma commitment per permutation column, then G, as (x, y) canonical integers ((0, 0): the identity)."""
    m = len(column_src)
    assert len(gate_fixed) == 9 and len(lookup_advice) == len(lookup_tag) == len(lookup_enable) == 5 and 1 <= m <= 8 and len(points) == num_fixed + m + 1
    out = le32(field) + le32(log_n) + le32(blinding_factors) + le32(num_fixed) + le32(m) + le32(chunk_len) + le32(lookup_mask)
    out += bytes(list(column_src) + [0] * (8 - m)) + bytes(gate_fixed) + bytes(lookup_advice) + bytes(lookup_tag) + bytes(lookup_enable)
    out += bytes([table_tag, table_value]) + int(omega).to_bytes(32, "little") + int(delta).to_bytes(32, "little") + le32(extended_k)
    for x, y in points:
        out += int(x).to_bytes(32, "little") + int(y).to_bytes(32, "little")
    return out


def digest(msg: bytes) -> bytes:
    return hashlib.blake2b(msg, digest_size=64, person=PERSON).digest()


def vk_repr(r, *args, **kw) -> int:
    """The canonical integer: digest(message(...)) as a little-endian 512-bit integer modulo r."""
    return int.from_bytes(digest(message(*args, **kw)), "little") % r


def config_args(field, cfg, P, points):
    """message()'s arguments from a quotient_ref.Config (prover_chain_ref.config)."""
    return (FIELDS[field], cfg.k, cfg.blinding_factors, cfg.num_fixed, cfg.column_src, cfg.chunk_len, cfg.lookup_mask, cfg.gate_fixed,
            cfg.lookup_advice, cfg.lookup_tag, cfg.lookup_enable, cfg.table_tag, cfg.table_value, cfg.omega(P), cfg.delta, cfg.log_ext, points)
