"""Host-side checks of the lookup argument's input-column / grand-product exports (h2r_lookup_input_columns, h2r_lookup_product_columns,
h2r_lookup_product_workspace_bytes): argument checking only, no device work."""
import ctypes

from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import H2RParams, lib


def host_ctx(w=64, L=32):
    ctx = ctypes.c_void_p()
    p = H2RParams(w, w * L, 0, -1)
    assert lib().h2r_ctx_create(ctypes.byref(p), ctypes.byref(ctx)) == 0
    return ctx


def _cfg(ctx):
    cfg = _lib.H2RLookupConfig()
    assert lib().h2r_lookup_config_default(ctx, 1, ctypes.byref(cfg)) == 0
    return cfg


def _call_inputs(ctx, cfg, kinds, image, theta, out, usable=1018, rows=4, first_row=0):
    return lib().h2r_lookup_input_columns(ctx, cfg, None, kinds, rows, image, rows * 160, 1, None, theta, usable, first_row, 31, out, 5 * usable * 32, None)


def _call_product(ctx, cfg, a_in, a_perm, s_perm, theta, beta, gamma, z, ws, usable=1018):
    col = (usable + 1) * 32
    return lib().h2r_lookup_product_columns(ctx, cfg, a_in, a_perm, s_perm, 5 * usable * 32, theta, beta, gamma, 1, usable, 31, z, 5 * col, col, None, ws, None)


def test_host_only_ctx_refuses_device_work():
    """As every device export does on a ctx without a device (test_cabi_host.test_ctx_create_status_codes): H2R_E_UNSUPPORTED."""
    ctx = host_ctx()
    cfg = _cfg(ctx)
    buf = (ctypes.c_uint64 * 64)()
    assert _call_inputs(ctx, ctypes.byref(cfg), buf, buf, buf, buf) == _lib.H2R_E_UNSUPPORTED
    assert _call_product(ctx, ctypes.byref(cfg), buf, buf, buf, buf, buf, buf, buf, buf) == _lib.H2R_E_UNSUPPORTED
    lib().h2r_ctx_destroy(ctx)


def test_null_pointers():
    ctx = host_ctx()
    cfg = _cfg(ctx)
    buf = (ctypes.c_uint64 * 64)()
    c = ctypes.byref(cfg)
    assert _call_inputs(None, c, buf, buf, buf, buf) == _lib.H2R_E_NULL
    assert _call_inputs(ctx, None, buf, buf, buf, buf) == _lib.H2R_E_NULL
    for hole in range(4):      # kinds, image, theta, the output
        args = [buf] * 4
        args[hole] = None
        assert _call_inputs(ctx, c, *args) == _lib.H2R_E_NULL, hole
    assert _call_product(None, c, *([buf] * 8)) == _lib.H2R_E_NULL
    assert _call_product(ctx, None, *([buf] * 8)) == _lib.H2R_E_NULL
    for hole in range(8):      # a_in, a_perm, s_perm, theta, beta, gamma, z, workspace
        args = [buf] * 8
        args[hole] = None
        assert _call_product(ctx, c, *args) == _lib.H2R_E_NULL, hole
    lib().h2r_ctx_destroy(ctx)


def test_workspace_bytes():
    ws = lib().h2r_lookup_product_workspace_bytes
    assert ws(131066, 0) == 0 and ws(0, 0) == 0
    rows = [1, 1018, 1024, 1025, 4090, 131066, (1 << 20) - 6]
    elems = [1, 2, 3, 256, 65535]
    for u in rows:
        sizes = [ws(u, e) for e in elems]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes) and sizes[0] > 0, u
    for e in elems:
        sizes = [ws(u, e) for u in rows]
        assert sizes == sorted(sizes), e
    assert ws(131066, 256) < 16 << 20      # two products per tile of a column: a few megabytes next to 10.7 GB of columns
