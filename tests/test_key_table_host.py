"""Keyed moduli, host side: the key table's size query on device-less contexts, the refusals of the table exports that need no
device, and the ABI version the keyed form arrived with.  No device work."""
import ctypes

from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import lib
from test_cabi_host import SHAPES, host_ctx


def chain_digits(kreal):
    """K of the chain build that serves integers of `kreal` 32-bit digits (launch_chain_shape)."""
    return next(k for k in (8, 16, 32, 64, 96, 128) if kreal <= k)


def chain_pre_words(K):
    """[shift, status, 0, 0], n'[K], mu'[K] (h2r_kernels.hpp)."""
    return 4 + 2 * K


def test_abi_version_is_5():
    assert lib().h2r_abi_version() == 5 == _lib.H2R_VERSION
    assert _lib.H2R_F_KEYED_MODULI == 2
    assert ctypes.sizeof(_lib.H2RKeyedModuli) == 32


def test_key_table_bytes_on_host_only_contexts():
    for (w, L) in SHAPES:
        c = host_ctx(w, L)
        K = chain_digits(w * L // 32)
        prev = 0
        for num_keys in (1, 2, 3, 16, 17, 255, 256, 1024, 100000):
            nb = int(lib().h2r_key_table_bytes(c, num_keys))
            assert nb > 0 and nb % 16 == 0, (w, L, num_keys, nb)
            assert nb >= prev, (w, L, num_keys)                       # monotone in num_keys
            assert nb >= num_keys * (L * (w // 8) + 4 * chain_pre_words(K)), (w, L, num_keys, nb)
            prev = nb
        assert int(lib().h2r_key_table_bytes(c, 0)) > 0               # the sentinel entry alone
        assert int(lib().h2r_key_table_bytes(c, 1 << 32)) == 0        # key indices are 32-bit
        lib().h2r_ctx_destroy(c)
    assert int(lib().h2r_key_table_bytes(None, 4)) == 0


def test_build_and_expand_refuse_a_host_only_ctx():
    c = host_ctx(64, 32)
    buf = (ctypes.c_uint64 * 1024)()
    tab = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)       # (aligned; a host-only ctx never touches it)
    idx = (ctypes.c_uint32 * 4)()
    out = (ctypes.c_uint64 * 128)()
    st = (ctypes.c_uint8 * 4)()
    assert lib().h2r_key_table_build(c, buf, 1, tab, st, None) == _lib.H2R_E_UNSUPPORTED
    assert lib().h2r_key_table_expand(c, tab, 1, idx, 4, out, None) == _lib.H2R_E_UNSUPPORTED
    lib().h2r_ctx_destroy(c)


def test_null_arguments():
    c = host_ctx(64, 32)
    buf = (ctypes.c_uint64 * 1024)()
    tab = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)
    idx = (ctypes.c_uint32 * 4)()
    out = (ctypes.c_uint64 * 128)()
    E = _lib.H2R_E_NULL
    assert lib().h2r_key_table_build(None, buf, 1, tab, None, None) == E
    assert lib().h2r_key_table_build(c, None, 1, tab, None, None) == E
    assert lib().h2r_key_table_build(c, buf, 1, None, None, None) == E
    assert lib().h2r_key_table_expand(None, tab, 1, idx, 4, out, None) == E
    assert lib().h2r_key_table_expand(c, None, 1, idx, 4, out, None) == E
    assert lib().h2r_key_table_expand(c, tab, 1, None, 4, out, None) == E
    assert lib().h2r_key_table_expand(c, tab, 1, idx, 4, None, None) == E
    # the keyed form of an export: a NULL struct, a NULL table / index inside it (checked before the ctx's device is looked at)
    st = (ctypes.c_uint8 * 4)()
    F = _lib.H2R_F_KEYED_MODULI
    assert lib().h2r_mul_mod_batch(c, out, out, None, 1, F, None, None, st, None, None) == E
    km = _lib.H2RKeyedModuli(ctypes.sizeof(_lib.H2RKeyedModuli), 0, 1, None, ctypes.addressof(idx))
    assert lib().h2r_mul_mod_batch(c, out, out, ctypes.addressof(km), 1, F, None, None, st, None, None) == E
    km = _lib.H2RKeyedModuli(ctypes.sizeof(_lib.H2RKeyedModuli), 0, 1, tab, None)
    assert lib().h2r_mul_mod_batch(c, out, out, ctypes.addressof(km), 1, F, None, None, st, None, None) == E
    # ... a struct of another size, or both flags: refused as unsupported
    km = _lib.H2RKeyedModuli(ctypes.sizeof(_lib.H2RKeyedModuli) - 8, 0, 1, tab, ctypes.addressof(idx))
    assert lib().h2r_mul_mod_batch(c, out, out, ctypes.addressof(km), 1, F, None, None, st, None, None) == _lib.H2R_E_UNSUPPORTED
    km = _lib.H2RKeyedModuli(ctypes.sizeof(_lib.H2RKeyedModuli), 0, 1, tab, ctypes.addressof(idx))
    assert lib().h2r_mul_mod_batch(c, out, out, ctypes.addressof(km), 1, F | _lib.H2R_F_SHARED_MODULUS, None, None, st, None, None) == _lib.H2R_E_UNSUPPORTED
    lib().h2r_ctx_destroy(c)
