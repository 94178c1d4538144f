"""The verifier's scalars on the host (h2r_verify_bases, h2r_verify_eval op 1 -- the very function verify_scalars_kernel inlines; DESIGN.md
section 2n) over the whole grid of tests/verify_cases.py, in both representations on a host-only ctx: the base and evaluation counts and
every scalar of R and L against the plain model (tests/verify_proof_ref.py: scalars_of), the model's closed-form l0 / l_last / l_active
against the product form wherever the domain is small enough, and x on the domain -- row 0, row u, the first blinding row, the last row --
which is H2R_E_ASSERTION with nothing written."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import create_proof_ref as C
import transcript_ref as T
import verify_cases as VC
import verify_proof_ref as V
from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import lib
from test_transcript_host import host_ctx

R = T.R
REPRS, IDS = [False, True], ["canonical", "montgomery"]
FILL = 0xEE


@pytest.fixture(scope="module", params=REPRS, ids=IDS)
def ctx(request):
    c = host_ctx(request.param)
    yield c, request.param
    lib().h2r_ctx_destroy(c)


def eval_scalars(c, mont, vcfg, evals, ch, num_bases):
    """(rc, the scalars of R, the scalars of L, the raw output) of the host twin; the output is pre-filled."""
    raw = b"".join(T.to_repr(v, R, mont).to_bytes(32, "little") for v in list(ch) + list(evals))
    out = (ctypes.c_uint8 * (32 * (num_bases + 4)))(*([FILL] * (32 * (num_bases + 4))))
    rc = lib().h2r_verify_eval(c, 1, ctypes.byref(vcfg), raw, len(raw), out, len(out))
    vals = [T.from_repr(int.from_bytes(bytes(out[i:i + 32]), "little"), R, mont) for i in range(0, len(out), 32)]
    return rc, vals[:num_bases], vals[num_bases:], bytes(out)


@pytest.mark.parametrize("domain", VC.DOMAINS, ids=["k%d-bf%d" % d for d in VC.DOMAINS])
def test_the_grid(ctx, domain):
    c, mont = ctx
    shapes = VC.shapes(domain)
    assert len(shapes) == len(VC.COLUMNS) * len(VC.MASKS)
    for shape in shapes:
        sid = VC.shape_id(shape)
        cfg = VC.config_of(shape)
        rng = random.Random("verify_scalars/host/" + sid)                         # (the same circuit in both representations)
        (evals, ch), = VC.inputs(rng, cfg, 1)
        pos = V.base_index(cfg)
        names = {at: name for name, at in pos.items()}
        vcfg = VC.verify_config(cfg, mont)
        ne = ctypes.c_uint32(0)
        nb = lib().h2r_verify_bases(ctypes.byref(vcfg), ctypes.byref(ne))
        assert nb == len(pos) and ne.value == len(C.queries(C.eval_plan(cfg))) == len(evals), sid
        st, right, left = V.scalars_of(cfg, evals, ch)
        assert st == 0, "%s: the model flags a drawn circuit" % sid
        rc, got_right, got_left, _ = eval_scalars(c, mont, vcfg, evals, ch, nb)
        assert rc == 0, (sid, rc)
        for at, (g, w) in enumerate(zip(got_right, right)):
            assert g == w, "%s: the scalar of base %d %r" % (sid, at, names[at])
        assert got_left == left, sid
        if cfg.k <= VC.MAX_PRODUCT_K:
            assert C.lagrange_at(cfg, ch[4]) == VC.lagrange_products(cfg, ch[4]), sid
        # x on the domain: an l_i's denominator and x^n - 1 vanish
        rows = [0, cfg.u, cfg.n - 1] + ([cfg.u + 1] if cfg.blinding_factors else [])
        for i in rows:
            bad = list(ch)
            bad[4] = pow(cfg.omega(R), i, R)
            rc, _, _, raw = eval_scalars(c, mont, vcfg, evals, bad, nb)
            assert rc == _lib.H2R_E_ASSERTION == V.scalars_of(cfg, evals, bad)[0], (sid, i, rc)
            assert raw == bytes([FILL]) * len(raw), "%s: a status writes nothing (row %d)" % (sid, i)
