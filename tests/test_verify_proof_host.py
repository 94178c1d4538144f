"""CPU-side checks of the verifier's exports on a host-only ctx: the host twin h2r_verify_eval -- the very functions
the kernels inline -- against the plain model (tests/verify_proof_ref.py) on the decoder's edge abscissae and scalars, on the scalar vector
of the k = 9 model proof in both representations, and on sums of terms with edge scalars and colliding bases; and every refusal of
h2r_proof_decode, h2r_verify_scalars and h2r_msm_terms next to a valid twin that ends in H2R_E_UNSUPPORTED (its last check)."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import create_proof_ref as C
import msm_ref as M
import transcript_ref as T
import verify_proof_ref as V
from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import lib
from test_create_proof_model import INSTANCES, TAU, case   # noqa: F401  (case: the module's fixture, the model proof made once here)
from test_transcript_host import host_ctx
from verify_cases import verify_config

Q, R = T.Q, T.R
NULL, SHAPE, UNSUP, ASSERTION = _lib.H2R_E_NULL, _lib.H2R_E_SHAPE, _lib.H2R_E_UNSUPPORTED, _lib.H2R_E_ASSERTION
BASE = 0x100000                                  # never dereferenced: the checks are host arithmetic on the addresses
REPRS, IDS = [False, True], ["canonical", "montgomery"]


@pytest.fixture(scope="module", params=REPRS, ids=IDS)
def ctx(request):
    c = host_ctx(request.param)
    yield c, request.param
    lib().h2r_ctx_destroy(c)


def copy_config(c):
    out = _lib.H2RVerifyScalarsConfig()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(c), ctypes.sizeof(c))
    return out


# ---- the decoder ------------------------------------------------------------------------------------------------------------------------------
def decode(c, kind, val):
    out = (ctypes.c_uint8 * (64 if kind == "point" else 32))(*([0xEE] * 64)[:64 if kind == "point" else 32])
    raw = bytes([1 if kind == "point" else 2]) + val.to_bytes(32, "little")
    rc = lib().h2r_verify_eval(c, 0, None, raw, len(raw), out, len(out))
    return rc, bytes(out)


def test_decode_one_item(ctx):
    c, mont = ctx
    real = M.mul_g(0xABCDEF)                                                     # a real point; its negative has the other parity
    no_point = next(x for x in range(2, 100) if C.decompress(x.to_bytes(32, "little")) is None)
    even = next(p for p in (M.mul_g(k) for k in range(2, 40)) if p[1] & 1 == 0)
    odd = next(p for p in (M.mul_g(k) for k in range(2, 40)) if p[1] & 1 == 1)
    xs = [0, 1, Q - 1, Q, (1 << 255) - 1, no_point, real[0], even[0], odd[0]]
    for x in xs:
        for sign in (0, 1):
            val = x | sign << 255
            want_st, want = V.decode_item("point", val.to_bytes(32, "little"))
            rc, got = decode(c, "point", val)
            assert rc == want_st, (x, sign, rc, want_st)
            if rc == 0:
                assert got == T.item_repr_bytes("point", want, mont), (x, sign)
                assert want[1] & 1 == sign and M.on_curve(want)
            else:
                assert got == b"\xEE" * 64, "a status writes nothing"
    assert V.decode_item("point", Q.to_bytes(32, "little"))[0] == SHAPE and V.decode_item("point", no_point.to_bytes(32, "little"))[0] == ASSERTION
    assert V.decode_item("point", real[0].to_bytes(32, "little"))[1] in (real, M.neg(real))
    for s in (0, 1, R - 1, R, (1 << 256) - 1, random.Random(1).randrange(R)):
        want_st, want = V.decode_item("scalar", s.to_bytes(32, "little"))
        rc, got = decode(c, "scalar", s)
        assert rc == want_st == (SHAPE if s >= R else 0)
        assert got == (T.to_repr(want, R, mont).to_bytes(32, "little") if rc == 0 else b"\xEE" * 32)


def test_verify_eval_refusals(ctx):
    c, _ = ctx
    out = (ctypes.c_uint8 * 64)()
    item = b"\x01" + (1).to_bytes(32, "little")
    ev = lib().h2r_verify_eval
    assert ev(None, 0, None, item, 33, out, 64) == NULL and ev(c, 0, None, None, 33, out, 64) == NULL and ev(c, 0, None, item, 33, None, 64) == NULL
    assert ev(c, 1, None, item, 33, out, 64) == NULL                              # op 1 reads a configuration
    assert ev(c, 3, None, item, 33, out, 64) == SHAPE
    assert ev(c, 0, None, item, 32, out, 64) == SHAPE and ev(c, 0, None, item, 33, out, 32) == SHAPE
    assert ev(c, 0, None, b"\x03" + item[1:], 33, out, 64) == SHAPE and ev(c, 0, None, b"\x02" + item[1:], 33, out, 64) == SHAPE
    assert ev(c, 2, None, bytes(96), 95, out, 64) == SHAPE and ev(c, 2, None, bytes(96), 0, out, 64) == SHAPE and ev(c, 2, None, bytes(96), 96, out, 32) == SHAPE
    other = host_ctx(False, "pasta_fp")
    assert ev(other, 0, None, item, 33, out, 64) == UNSUP
    lib().h2r_ctx_destroy(other)


# ---- the scalars ------------------------------------------------------------------------------------------------------------------------------
def eval_scalars(c, mont, vcfg, ch, evals, num_bases):
    raw = b"".join(T.to_repr(v, R, mont).to_bytes(32, "little") if v < R else v.to_bytes(32, "little") for v in list(ch) + list(evals))
    out = (ctypes.c_uint8 * (32 * (num_bases + 4)))(*([0xEE] * (32 * (num_bases + 4))))
    rc = lib().h2r_verify_eval(c, 1, ctypes.byref(vcfg), raw, len(raw), out, len(out))
    vals = [T.from_repr(int.from_bytes(bytes(out[i:i + 32]), "little"), R, mont) for i in range(0, len(out), 32)]
    return rc, vals[:num_bases], vals[num_bases:], bytes(out)


def test_the_scalar_vector_of_the_model_proof(ctx, case):
    c, mont = ctx
    _, key, proof = case
    cfg = key.cfg
    vk = V.VerifyingKey(key, TAU)
    _, sec = V.decode(cfg, proof)
    ch = V.challenges(vk, sec, INSTANCES)
    st, right, left = V.scalars_of(cfg, sec["evals"], ch)
    assert st == 0
    vcfg = verify_config(cfg, mont)
    ne = ctypes.c_uint32(0)
    nb = lib().h2r_verify_bases(ctypes.byref(vcfg), ctypes.byref(ne))
    assert nb == len(right) == len(V.base_index(cfg)) and ne.value == len(sec["evals"])
    rc, got_right, got_left, _ = eval_scalars(c, mont, vcfg, ch, sec["evals"], nb)
    assert rc == 0
    names = {pos: name for name, pos in V.base_index(cfg).items()}
    for pos, (g, w) in enumerate(zip(got_right, right)):
        assert g == w, "the scalar of base %d %r" % (pos, names[pos])
    assert got_left == left
    # other challenges, other evaluations: every term of the expression moves
    rng = random.Random("verify/host/scalars")
    ch2, ev2 = [rng.randrange(R) for _ in range(7)], [rng.randrange(R) for _ in sec["evals"]]
    st, right, left = V.scalars_of(cfg, ev2, ch2)
    rc, got_right, got_left, _ = eval_scalars(c, mont, vcfg, ch2, ev2, nb)
    assert rc == st == 0 and got_right == right and got_left == left
    # x a root of unity (an l_i's denominator or x^n - 1 vanishes): H2R_E_ASSERTION, nothing written
    for i in (0, 5, cfg.u, cfg.n - 1):
        bad = list(ch)
        bad[4] = pow(cfg.omega(R), i, R)
        rc, _, _, raw = eval_scalars(c, mont, vcfg, bad, sec["evals"], nb)
        assert rc == ASSERTION == V.scalars_of(cfg, sec["evals"], bad)[0] and raw == b"\xEE" * len(raw)
    for k in range(7):                                                            # a challenge that is not canonical
        bad = list(ch)
        bad[k] = R + k
        rc, _, _, raw = eval_scalars(c, mont, vcfg, bad, sec["evals"], nb)
        assert rc == SHAPE and raw == b"\xEE" * len(raw)
    # in_len / out_len
    buf = (ctypes.c_uint8 * (32 * (nb + 4)))()
    raw = bytes(32 * (7 + ne.value))
    assert lib().h2r_verify_eval(c, 1, ctypes.byref(vcfg), raw, len(raw) - 32, buf, len(buf)) == SHAPE
    assert lib().h2r_verify_eval(c, 1, ctypes.byref(vcfg), raw, len(raw), buf, len(buf) - 32) == SHAPE


def test_configuration_refusals(ctx, case):
    c, mont = ctx
    cfg = case[1].cfg
    good = verify_config(cfg, mont)
    nb = lib().h2r_verify_bases(ctypes.byref(good), None)
    assert nb == 32 + cfg.num_fixed + cfg.m + 1
    ev, op = copy_config(good).eval_plan, copy_config(good).open_plan
    find = lambda plan, n, g, i: next(j for j in range(n) if (plan[j].group, plan[j].index) == (_lib.VERIFY_GROUPS.index(g), i))
    e_adv4, e_pz0, e_sig0, o_h = find(ev, good.num_eval_plan, "advice", 4), find(ev, good.num_eval_plan, "perm_z", 0), find(ev, good.num_eval_plan, "sigma", 0), find(op, good.num_open_plan, "h", 0)

    def changed(fn):
        x = copy_config(good)
        fn(x)
        return x

    def setf(name, v):
        return lambda x: setattr(x, name, v)

    def seta(name, i, v):
        return lambda x: getattr(x, name).__setitem__(i, v)

    def plan(name, j, field, v):
        return lambda x: setattr(getattr(x, name)[j], field, v)

    bad = [setf("log_n", 0), setf("log_n", 25), setf("blinding_factors", 14), setf("num_fixed", 17), setf("num_fixed", cfg.num_fixed - 1), setf("num_columns", 0),
           setf("num_columns", 9), setf("chunk_len", 0), setf("lookup_mask", 32), setf("reserved", 1), setf("num_eval_plan", 0), setf("num_eval_plan", 65),
           setf("num_open_plan", 0), setf("num_open_plan", 65), seta("gate_fixed", 3, cfg.num_fixed), seta("column_src", 0, 5), seta("lookup_advice", 2, 5),
           seta("lookup_tag", 1, cfg.num_fixed), seta("lookup_enable", 4, cfg.num_fixed), setf("table_tag", cfg.num_fixed), setf("table_value", cfg.num_fixed),
           plan("eval_plan", 0, "group", 9), plan("eval_plan", 0, "group", 8), plan("eval_plan", 0, "index", 5), plan("eval_plan", 0, "mask", 0),
           plan("eval_plan", 0, "mask", 16), plan("eval_plan", 0, "reserved", 1), plan("eval_plan", 1, "index", 0),             # advice 0 twice
           plan("eval_plan", e_adv4, "mask", 1), plan("eval_plan", e_pz0, "mask", 3), plan("eval_plan", e_sig0, "group", 2),   # a missing evaluation
           setf("num_eval_plan", good.num_eval_plan - 1),
           plan("open_plan", 0, "mask", 3), plan("open_plan", 0, "mask", 0), plan("open_plan", 1, "index", 0), plan("open_plan", o_h, "mask", 3),
           plan("open_plan", o_h, "index", 1), plan("open_plan", 0, "reserved", 1), plan("open_plan", 0, "group", 9)]
    for k, fn in enumerate(bad):
        assert lib().h2r_verify_bases(ctypes.byref(changed(fn)), None) == 0, k
    # a lookup column of an argument that is not selected
    x = changed(setf("lookup_mask", 15))
    assert lib().h2r_verify_bases(ctypes.byref(x), None) == 0
    # what needs the field: omega, delta
    rep = lambda v: M.words(T.to_repr(v, R, mont))
    ch = _lib.H2RVerifyChallenges(*([BASE + 0x1000 * k for k in range(7)]))
    call = lambda vc: lib().h2r_verify_scalars(c, ctypes.byref(vc), BASE + 0x10000, 32 * 60, ctypes.byref(ch), 3, BASE + 0x20000, 32 * nb, BASE + 0x30000, BASE + 0x40000, None)
    assert call(good) == UNSUP                                                    # the valid twin: a host-only ctx, the last check
    for fn in (lambda x: x.omega.__setitem__(slice(0, 4), M.words(R)), lambda x: x.delta.__setitem__(slice(0, 4), M.words(R + 1)),
               lambda x: x.omega.__setitem__(slice(0, 4), rep(pow(cfg.omega(R), 2, R))), lambda x: x.omega.__setitem__(slice(0, 4), rep(1))):
        assert call(changed(fn)) == SHAPE
    assert call(changed(setf("struct_size", 8))) == UNSUP and call(changed(setf("log_n", 0))) == SHAPE


def test_verify_scalars_refusals(ctx, case):
    c, mont = ctx
    good = verify_config(case[1].cfg, mont)
    nb, ne = lib().h2r_verify_bases(ctypes.byref(good), None), 60
    EV, RT, LF, ST = BASE + 0x10000, BASE + 0x20000, BASE + 0x30000, BASE + 0x40000

    def call(cfg=good, evals=EV, es=32 * ne, ch=None, batch=3, right=RT, rs=32 * nb, left=LF, status=ST, nullch=None):
        chs = [BASE + 0x1000 * k for k in range(7)] if ch is None else ch
        if nullch is not None:
            chs[nullch] = None
        s = _lib.H2RVerifyChallenges(*chs)
        return lib().h2r_verify_scalars(c, ctypes.byref(cfg) if cfg is not None else None, evals, es, ctypes.byref(s), batch, right, rs, left, status, None)

    assert call() == UNSUP and call(status=None) == UNSUP and call(batch=0) == UNSUP and call(es=0, batch=1) == UNSUP
    assert call(cfg=None) == NULL and call(evals=None) == NULL and call(right=None) == NULL and call(left=None) == NULL
    assert lib().h2r_verify_scalars(c, ctypes.byref(good), EV, 32 * ne, None, 3, RT, 32 * nb, LF, ST, None) == NULL
    assert lib().h2r_verify_scalars(None, ctypes.byref(good), EV, 32 * ne, None, 3, RT, 32 * nb, LF, ST, None) == NULL
    for k in range(7):
        assert call(nullch=k) == NULL
        assert call(ch=[BASE + 0x1000 * j + (8 if j == k else 0) for j in range(7)]) == SHAPE         # misaligned
        assert call(ch=[RT + 32 if j == k else BASE + 0x1000 * j for j in range(7)]) == SHAPE         # inside an output
    assert call(evals=EV + 8) == SHAPE and call(es=32 * ne + 8) == SHAPE and call(right=RT + 8) == SHAPE and call(rs=32 * nb + 8) == SHAPE and call(left=LF + 8) == SHAPE
    assert call(es=32 * ne - 32) == SHAPE and call(rs=32 * nb - 32) == SHAPE and call(es=0) == SHAPE and call(rs=0) == SHAPE
    assert call(right=EV + 32) == SHAPE and call(left=EV) == SHAPE and call(status=EV + 5) == SHAPE          # an output over the evaluations
    assert call(left=RT + 64) == SHAPE and call(status=RT + 3 * 32 * nb - 1) == SHAPE and call(status=LF + 383) == SHAPE and call(status=LF + 384) == UNSUP
    other = host_ctx(False, "pasta_fp")
    s = _lib.H2RVerifyChallenges(*[BASE + 0x1000 * k for k in range(7)])
    assert lib().h2r_verify_scalars(other, ctypes.byref(good), EV, 32 * ne, ctypes.byref(s), 3, RT, 32 * nb, LF, ST, None) == UNSUP
    lib().h2r_ctx_destroy(other)


# ---- the sum of terms -------------------------------------------------------------------------------------------------------------------------
def eval_sum(c, mont, scalars, bases):
    raw = b"".join(M.scalar_bytes([s], mont) + M.point_bytes([p], mont) for s, p in zip(scalars, bases))
    out = (ctypes.c_uint8 * 64)()
    assert lib().h2r_verify_eval(c, 2, None, raw, len(raw), out, 64) == 0
    return M.points_from_bytes(bytes(out), mont)[0]


def test_sum_of_terms(ctx):
    c, mont = ctx
    rng = random.Random("verify/host/sum")
    P1, P2 = M.mul_g(rng.randrange(R)), M.mul_g(rng.randrange(R))
    edge = [0, 1, R - 1, R, (1 << 256) - 1]
    for s in edge:
        assert eval_sum(c, mont, [s], [P1]) == M.mul(s, P1), s
    assert eval_sum(c, mont, [R - 1], [P1]) == M.neg(P1) and eval_sum(c, mont, [R], [P1]) == M.IDENT
    cases = [([1, 1], [P1, P1]), ([1, 1], [P1, M.neg(P1)]), ([5, 5], [P1, P1]), ([7, R - 7], [P1, P1]), ([3, 4], [M.IDENT, P2]), ([3, 4], [P1, M.IDENT]),
             ([0, 0], [P1, P2]), ([9], [M.IDENT]), (edge, [P1, P2, P1, P2, P1]), ([rng.randrange(R) for _ in range(7)], [M.mul_g(rng.randrange(R)) for _ in range(7)])]
    for scalars, bases in cases:
        assert eval_sum(c, mont, scalars, bases) == M.naive_msm(scalars, bases), (scalars, bases)
    assert eval_sum(c, mont, [1, 1], [P1, P1]) == M.mul(2, P1) and eval_sum(c, mont, [1, 1], [P1, M.neg(P1)]) == M.IDENT


def test_msm_terms_refusals(ctx):
    c, _ = ctx
    S, B, O, ST = BASE, BASE + 0x100000, BASE + 0x200000, BASE + 0x300000

    def call(T=8, scalars=S, ss=256, bases=B, bs=512, batch=3, out=O, status=ST, size=None, reserved=0, ctx_=c, cfg=True):
        mc = _lib.H2RMsmTermsConfig(struct_size=ctypes.sizeof(_lib.H2RMsmTermsConfig) if size is None else size, num_terms=T, reserved=reserved)
        return lib().h2r_msm_terms(ctx_, ctypes.byref(mc) if cfg else None, scalars, ss, bases, bs, batch, out, status, None)

    assert call() == UNSUP and call(status=None) == UNSUP and call(ss=0, bs=0) == UNSUP and call(batch=0) == UNSUP and call(T=4096, ss=32 * 4096, bs=64 * 4096) == UNSUP
    assert call(ctx_=None) == NULL and call(cfg=False) == NULL and call(scalars=None) == NULL and call(bases=None) == NULL and call(out=None) == NULL
    assert call(size=8) == UNSUP
    assert call(T=0) == SHAPE and call(T=4097, ss=32 * 4097, bs=64 * 4097) == SHAPE and call(reserved=1) == SHAPE
    assert call(scalars=S + 8) == SHAPE and call(ss=264) == SHAPE and call(bases=B + 8) == SHAPE and call(bs=520) == SHAPE and call(out=O + 8) == SHAPE
    assert call(ss=224) == SHAPE and call(bs=496) == SHAPE
    assert call(out=S + 32) == SHAPE and call(out=B + 2 * 512) == SHAPE and call(out=S + 2 * 256 + 224) == SHAPE and call(out=S + 2 * 256 + 256) == UNSUP
    assert call(status=O + 191) == SHAPE and call(status=O + 192) == UNSUP
    other = host_ctx(False, "pasta_fp")
    assert call(ctx_=other) == UNSUP
    lib().h2r_ctx_destroy(other)


def test_proof_decode_refusals(ctx):
    c, _ = ctx
    PR, PT, SC, ST = BASE, BASE + 0x100000, BASE + 0x200000, BASE + 0x300000
    layout = [(1, 5), (2, 3), (1, 2)]                                             # 10 items: 7 points, 3 scalars

    def call(sections=layout, proof=PR, ps=320, batch=3, points=PT, pts=448, scalars=SC, scs=96, status=ST, size=None, reserved=0, ctx_=c, nsec=None, cfg=True, sec=True):
        arr = (_lib.H2RProofSection * max(len(sections), 1))(*[_lib.H2RProofSection(k, n) for k, n in sections])
        dc = _lib.H2RProofDecodeConfig(struct_size=ctypes.sizeof(_lib.H2RProofDecodeConfig) if size is None else size,
                                       num_sections=len(sections) if nsec is None else nsec, reserved=reserved)
        return lib().h2r_proof_decode(ctx_, ctypes.byref(dc) if cfg else None, arr if sec else None, proof, ps, batch, points, pts, scalars, scs, status, None)

    assert call() == UNSUP and call(status=None) == UNSUP and call(batch=0) == UNSUP and call(ps=0, batch=1) == UNSUP
    assert call(sections=[(2, 4)], points=None, scs=128) == UNSUP and call(sections=[(1, 1)], scalars=None, pts=64) == UNSUP   # a single item; no output of the other kind
    assert call(ctx_=None) == NULL and call(cfg=False) == NULL and call(sec=False) == NULL and call(proof=None) == NULL
    assert call(points=None) == NULL and call(scalars=None) == NULL
    assert call(size=8) == UNSUP
    assert call(nsec=0) == SHAPE and call(sections=[(1, 1)] * 17) == SHAPE and call(reserved=1) == SHAPE
    assert call(sections=[(3, 1)]) == SHAPE and call(sections=[(0, 1)]) == SHAPE and call(sections=[(1, 0), (2, 1)]) == SHAPE
    assert call(sections=[(1, 40000), (2, 30000)], ps=32 * 70000, pts=64 * 40000, scs=32 * 30000) == SHAPE                      # more than 65,535 items
    assert call(proof=PR + 8) == SHAPE and call(ps=328) == SHAPE and call(points=PT + 8) == SHAPE and call(pts=456) == SHAPE and call(scalars=SC + 8) == SHAPE and call(scs=104) == SHAPE
    assert call(ps=288) == SHAPE and call(ps=0) == SHAPE and call(pts=384) == SHAPE and call(scs=64) == SHAPE and call(pts=0) == SHAPE
    assert call(points=PR + 32) == SHAPE and call(scalars=PR + 2 * 320) == SHAPE and call(status=PR + 959) == SHAPE and call(status=PR + 960) == UNSUP
    assert call(scalars=PT + 2 * 448 + 432) == SHAPE and call(scalars=PT + 3 * 448) == UNSUP and call(status=SC + 287) == SHAPE and call(status=PT) == SHAPE
    other = host_ctx(False, "pasta_fp")
    assert call(ctx_=other) == UNSUP
    lib().h2r_ctx_destroy(other)
