"""Every chain build on edge moduli and quotient-boundary operands (tests/edge_cases.py), against the C oracle.

Each test is one row of the build matrix: it reaches its build by the dispatch rule quoted above it (launch_chain_shape in
h2r_tu_chain.hip; step_eligible / two_queue_shape / exp_segment_count / plain_call_overlaps in h2r_api.hip), mixes the edge elements
with random full-size neighbours in one batch, and checks for every element: the status against the rule and the oracle; for a
status-0 element the value, the WHOLE flat stream against the oracle's, and the in-place audit.  A row asserts its own coverage:
every modulus class has a status-0 element whose stream was compared, per-element and with one shared modulus
(H2R_F_SHARED_MODULUS); a row that runs mul_mod also has an element at the quotient-fit limit (status 0) and one above it.
"""
import random

import numpy as np
import pytest

import edge_cases as E
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VAR_E1 = ([17], 5)
VAR_EM = ([0x1A2B3, 0x5, 0x1FFFF], 17)
FULL_COMPARE_MAX = 2048   # above this many elements per call: every edge element and a seeded sample of the filler


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    import halo2_rsa_amd
    return halo2_rsa_amd


@pytest.fixture(scope="module")
def cus(H):
    return torch.cuda.get_device_properties(0).multi_processor_count


class Cover:
    """(form, class) cells with a status-0 element whose whole stream equalled the oracle's; mul_mod quotient-limit hits."""

    def __init__(self):
        self.cells, self.limit_ok, self.limit_over = set(), False, False

    def assert_complete(self, forms):
        for f in forms:
            missing = [c for c in E.CLASSES if (f, c) not in self.cells]
            assert not missing, (f, missing)


def _mix(edge, fill, seed):
    """Edge elements and their random neighbours interleaved in one batch (seeded)."""
    items = list(edge) + list(fill)
    random.Random(seed).shuffle(items)
    return items


def _first_mismatch(a, b):
    if len(a) != len(b):
        return "length %d != %d" % (len(a), len(b))
    return "byte %d of %d" % (int(np.nonzero(a != b)[0][0]), len(a))


def _compare_set(items, seed):
    if len(items) <= FULL_COMPARE_MAX:
        return set(range(len(items)))
    edge = {i for i, it in enumerate(items) if it[0] != "filler"}
    rest = sorted(set(range(len(items))) - edge)
    return edge | set(random.Random(seed).sample(rest, 64))


# ---- one call of each kind, checked element by element ---------------------------------------------------------------------
def run_mul_mod(H, chip, o, items, cover, form, shared_n=None, seed=0):
    """items: [(class, tag, a, b, n)]."""
    bits = chip.limb_width * chip.num_limbs
    A = [it[2] for it in items]; B = [it[3] for it in items]; N = [it[4] for it in items]
    n_dev = chip.assign_integer([shared_n] if shared_n is not None else N)
    res = chip.mul_mod(chip.assign_integer(A), chip.assign_integer(B), n_dev)
    bad, _first = res.audit()
    torch.cuda.synchronize()
    st = res.status.cpu().tolist()
    vals = res.value.to_big_uint()
    nb = bad.cpu().numpy()
    host = res.trace.buf.cpu().numpy()
    stride = res.trace.elem_stride
    cmp = _compare_set(items, seed)
    for i, (cls, tag, a, b, n) in enumerate(items):
        exp, val = E.mul_mod_expect(a, b, n, bits)
        ctx = (form, cls, tag, i, hex(n))
        assert st[i] == exp, ctx + (st[i], exp)
        rc, rr, ost = o.mul_mod(o.limbs(a), o.limbs(b), o.limbs(n), want_stream=(exp == 0 and i in cmp))
        assert rc == exp, ctx
        if tag == "limit+1":
            cover.limit_over = True
        if exp:
            continue
        assert vals[i] == val == o.to_int(rr), ctx
        assert nb[i] == 0, ctx + ("audit",)
        if i in cmp:
            got = _flatten_mul(chip, host[i * stride:(i + 1) * stride])
            assert np.array_equal(got, ost), ctx + (_first_mismatch(got, ost),)
            cover.cells.add((form, cls))
            if tag == "limit":
                cover.limit_ok = True


def _flatten_mul(chip, elem_bytes):
    from halo2_rsa_amd._lib import check, lib
    host = np.ascontiguousarray(elem_bytes)
    out = np.zeros(chip.layout.stream_bytes, dtype=np.uint8)
    check(lib().h2r_trace_flatten_ex(chip._ctx, host.ctypes.data, 0, out.ctypes.data), "h2r_trace_flatten_ex")
    return out


def _e_dev(H, chip, limbs, batch):
    a = np.array([limbs] * batch, dtype=chip.np_dtype)
    return H.AssignedInteger(torch.from_numpy(a.view(np.int64 if chip.limb_width == 64 else np.int32)).cuda().contiguous(), chip.limb_width)


def run_pow(H, chip, o, items, cover, form, e=None, var=None, in_field=False, shared_n=None, seed=0):
    """items: [(class, tag, x, n)].  e: a fixed exponent (pow_mod_fixed_exp / modpow_public_key Fix); var: (limbs, exp_limb_bits)
    (pow_mod / modpow_public_key Var).  in_field: the modpow_public_key form (assert_in_field first, its witness compared too)."""
    bits = chip.limb_width * chip.num_limbs
    X = [it[2] for it in items]; N = [it[3] for it in items]
    x_dev = chip.assign_integer(X)
    n_dev = chip.assign_integer([shared_n] if shared_n is not None else N)
    if var is None:
        res = chip.pow_mod_fixed_exp(x_dev, e, n_dev, check_in_field=in_field)
    else:
        res = chip.pow_mod(x_dev, _e_dev(H, chip, var[0], len(X)), n_dev, var[1], check_in_field=in_field)
    bad, _first = res.audit()
    torch.cuda.synchronize()
    check_pow_result(chip, o, items, res.status, res.value, res.trace, res.in_field, bad, cover, form, e, var, in_field, seed)


def check_pow_result(chip, o, items, status, value, trace, in_field_trace, bad, cover, form, e, var, in_field, seed, covers=True):
    bits = chip.limb_width * chip.num_limbs
    st = status.cpu().tolist()
    vals = value.to_big_uint()
    nb = bad.cpu().numpy() if bad is not None else None
    cmp = _compare_set(items, seed)
    for i, (cls, tag, x, n) in enumerate(items):
        if var is None:
            exp, val = E.pow_fixed_expect(x, e, n, bits, in_field)
        else:
            exp, val = E.pow_var_expect(x, var[0], var[1], n, bits, in_field)
        ctx = (form, cls, tag, i, hex(n))
        assert st[i] == exp, ctx + (st[i], exp)
        if in_field:
            rc, lt, s_if = o.assert_in_field(o.limbs(x), o.limbs(n))
            assert lt == int(x < n), ctx
            if in_field_trace is not None and i in cmp:    # (written for a failing element too: is_less_than = 0 in its stream)
                got = in_field_trace.flatten(i)
                assert np.array_equal(got, s_if), ctx + ("in-field", _first_mismatch(got, s_if))
            if exp == E.NOT_IN_FIELD:
                continue
        want = exp == 0 and i in cmp
        if var is None:
            rc, oo, ost = o.pow_mod_fixed_exp(o.limbs(x), o.limbs(n), e, want_stream=want)
        else:
            rc, oo, ost = o.pow_mod(o.limbs(x), np.array(var[0], dtype=o.dtype), var[1], o.limbs(n), want_stream=want)
        assert rc == exp, ctx
        if exp:
            continue
        assert vals[i] == val == o.to_int(oo), ctx
        if nb is not None:
            assert nb[i] == 0, ctx + ("audit",)
        if want:
            got = trace.flatten(i)
            assert np.array_equal(got, ost), ctx + (_first_mismatch(got, ost),)
            if covers:
                cover.cells.add((form, cls))


# ---- element lists ------------------------------------------------------------------------------------------------------------
def mul_items(w, L, fill, seed=0):
    edge = E.mul_mod_cases(w, L, seed)
    return _mix(edge, [("filler", "rand", a, b, n) for a, b, n in E.filler(w, L, fill, seed)], seed)


def pow_items(w, L, fill, lean=False, in_field=False, seed=0):
    edge = E.pow_cases(w, L, seed, lean=lean)
    if in_field:   # x = n +- 2^(w*j): the in-field comparison decided after a borrow / carry run of j limbs
        bits = w * L
        for cls, ns in E.by_class(E.moduli(w, L, seed)).items():
            for j in E.in_field_offsets(w, L):
                for x in (ns[0] + (1 << (w * j)), ns[0] - (1 << (w * j))):
                    if 0 <= x < (1 << bits):
                        edge.append((cls, "n%+d*2^%d" % (1 if x > ns[0] else -1, w * j), x, ns[0]))
    return _mix(edge, [("filler", "rand", x, n) for x, _b, n in E.filler(w, L, fill, seed)], seed)


def shared_items(items, n, seed):
    """The same operand tags against ONE modulus `n`, with random neighbours reduced mod n."""
    rng = random.Random(seed)
    out = []
    for it in items:
        if it[-1] == n:
            out.append(it)
    for _ in range(max(4, len(out) // 2)):
        out.append(("filler", "rand") + tuple(rng.randrange(n) for _ in range(len(items[0]) - 3)) + (n,))
    rng.shuffle(out)
    return out


def run_ops(H, w, L, ops, cover, fill=16, lean_pow=False, shared=True, max_batch=None, seed=0):
    """The ops of one row, per-element moduli and then one shared modulus per class."""
    chip = H.BigIntChip(w, w * L)
    o = Oracle(w, L)
    mods = E.by_class(E.moduli(w, L, seed))
    for op in ops:
        if op == "mul_mod":
            items = mul_items(w, L, fill, seed)
            if max_batch is not None:
                assert len(items) <= max_batch, (len(items), max_batch)
            run_mul_mod(H, chip, o, items, cover, "per-element", seed=seed)
            if shared:
                for cls in E.CLASSES:
                    run_mul_mod(H, chip, o, shared_items(items, mods[cls][0], seed), cover, "shared", shared_n=mods[cls][0], seed=seed)
            continue
        kw = dict(e=E.E_SPARSE)
        lean = lean_pow
        if op == "pow_dense":
            kw, lean = dict(e=E.E_DENSE), True
        elif op == "pow_var1":
            kw = dict(var=VAR_E1)
        elif op == "pow_varm":
            kw, lean = dict(var=VAR_EM), True
        elif op == "modpow":
            kw = dict(e=E.E_SPARSE, in_field=True)
        elif op == "modpow_dense":
            kw, lean = dict(e=E.E_DENSE, in_field=True), True
        items = pow_items(w, L, fill, lean=lean, in_field=kw.get("in_field", False), seed=seed)
        if max_batch is not None:
            assert len(items) <= max_batch, (len(items), max_batch)
        run_pow(H, chip, o, items, cover, "per-element", seed=seed, **kw)
        if shared:
            for cls in E.CLASSES:
                run_pow(H, chip, o, shared_items(items, mods[cls][0], seed), cover, "shared", shared_n=mods[cls][0], seed=seed, **kw)
    return chip, o


ALL_OPS = ["mul_mod", "pow", "pow_dense", "pow_var1", "pow_varm", "modpow"]


# ---- rows of the build matrix -------------------------------------------------------------------------------------------------
# launch_chain_shape: K = digits rounded up to 8 / 16 / 32 / 64 / 96 / 128.  K = 8 and 16: chain_kernel<K,1> for any call.  K = 32:
# chain_wave_kernel<32> (one wave per element; knobs default chain_wave = -1, chain_nw = 0), a shared modulus first through
# recip_kernel<32,4>.  K = 96: chain_kernel<96,6>; K = 128: chain_kernel<128,8>, any batch.  (No call below reaches the sub-batch
# walk: plain_call_overlaps needs > 1,536 elements at these shapes.)
@pytest.mark.parametrize("build,w,L", [
    ("chain_kernel<8,1>", 64, 4), ("chain_kernel<8,1>", 32, 8),
    ("chain_kernel<16,1>", 64, 8), ("chain_kernel<16,1>", 32, 16),
    ("chain_wave_kernel<32>", 64, 16), ("chain_wave_kernel<32>", 64, 12), ("chain_wave_kernel<32>", 32, 32), ("chain_wave_kernel<32>", 32, 24),
    ("chain_kernel<96,6>", 64, 48), ("chain_kernel<96,6>", 64, 40), ("chain_kernel<96,6>", 32, 96),
    ("chain_kernel<128,8>", 64, 64), ("chain_kernel<128,8>", 32, 128),
])
def test_edge_moduli_any_call_builds(H, build, w, L):
    cover = Cover()
    run_ops(H, w, L, ALL_OPS, cover, lean_pow=w * L >= 3072, max_batch=1536)
    cover.assert_complete(["per-element", "shared"])
    assert cover.limit_ok and cover.limit_over


# K = 64 at <= 2 * num_CUs elements: chain_kernel<64,4,DEEP> (deep = batch <= 512) for mul_mod, sparse fixed exponents and any shared
# modulus (ca.pre set: never the dual build).
@pytest.mark.parametrize("w,L", [(64, 32), (32, 64)])
def test_edge_moduli_deep_chain(H, cus, w, L):
    cover = Cover()
    run_ops(H, w, L, ["mul_mod", "pow", "modpow"], cover, max_batch=min(2 * cus, 512))
    cover.assert_complete(["per-element", "shared"])
    assert cover.limit_ok and cover.limit_over


# K = 64 at <= 2 * num_CUs elements, per-element moduli, a variable exponent or a fixed one of >= 64 bits with popcount >= bits / 4:
# chain_dual_kernel<64> (its own chain_element_dual setup).  The shared-modulus calls of the same ops take the deep build above.
@pytest.mark.parametrize("w,L", [(64, 32), (32, 64)])
def test_edge_moduli_dual_chain(H, cus, w, L):
    assert bin(E.E_DENSE).count("1") * 4 >= E.E_DENSE.bit_length() >= 64
    cover = Cover()
    run_ops(H, w, L, ["pow_dense", "pow_var1", "pow_varm", "modpow_dense"], cover, max_batch=2 * cus)
    cover.assert_complete(["per-element", "shared"])


# K = 64 at > max(512, 2 * num_CUs) elements: the throughput build chain_kernel<64,4> for every exponent.  RSA-2048 stays a single
# run_path call up to 6 * num_CUs elements (plain_call_overlaps: L in (16, 32] walks > 1.5 * 4 * num_CUs as sub-batches); 32-bit limbs
# never take that walk.
@pytest.mark.parametrize("w,L", [(64, 32), (32, 64)])
def test_edge_moduli_throughput_chain(H, cus, w, L):
    B = max(512, 2 * cus) + 64
    assert B > 512 and B > 2 * cus and (w != 64 or B <= 6 * cus)
    chip = H.BigIntChip(w, w * L)
    o = Oracle(w, L)
    cover = Cover()
    items = mul_items(w, L, 0)
    items = _mix(items, [("filler", "rand", a, b, n) for a, b, n in E.filler(w, L, B - len(items), 1)], 1)
    assert len(items) == B
    run_mul_mod(H, chip, o, items, cover, "per-element")
    for e, in_field, lean in ((E.E_SPARSE, False, False), (E.E_SPARSE, True, False), (E.E_DENSE, False, True)):
        items = pow_items(w, L, 0, lean=lean, in_field=in_field)
        items = _mix(items, [("filler", "rand", x, n) for x, _b, n in E.filler(w, L, B - len(items), 2)], 2)
        assert len(items) == B
        run_pow(H, chip, o, items, cover, "per-element", e=e, in_field=in_field)
    n0 = E.by_class(E.moduli(w, L))
    for cls in E.CLASSES:    # one shared modulus per class, the batch filled past the threshold with x < n
        n = n0[cls][0]
        edge = [it for it in pow_items(w, L, 0) if it[3] == n]
        rng = random.Random(3)
        items = _mix(edge, [("filler", "rand", rng.randrange(n), n) for _ in range(B - len(edge))], 3)
        run_pow(H, chip, o, items, cover, "shared", e=E.E_SPARSE, shared_n=n)
    cover.assert_complete(["per-element", "shared"])
    assert cover.limit_ok and cover.limit_over


def _pipeline_calls(H, chip, pipe, items_per_call, e, B):
    """Pipelined modpow_public_key calls (Fix e) on rotating buffer sets; returns per call (status, out, Trace, InFieldTrace)."""
    w, L = chip.limb_width, chip.num_limbs
    pl = chip.pow_fixed_layout(e)
    ies = chip.in_field_layout()[0]
    mk = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    outs = []
    for items in items_per_call:
        X = [it[2] for it in items]; N = [it[3] for it in items]
        s = dict(trace=mk(B * pl.elem_stride), inf=mk(B * ies), ws=mk(chip.workspace_bytes(B, pl.num_mul_mods)),
                 out=torch.zeros((B, L), dtype=chip.torch_dtype, device="cuda"), status=mk(B), x=chip.assign_integer(X), n=chip.assign_integer(N))
        pipe.modpow_public_key(s["x"], e, s["n"], s["trace"], s["ws"], s["out"], s["status"], in_field_buf=s["inf"])
        outs.append(s)
    pipe.join()
    torch.cuda.synchronize()
    res = []
    for s in outs:
        r = H.BatchResult(H.AssignedInteger(s["out"], w), H.Trace(chip, s["trace"], B, pl), s["status"],
                          H.big_integer.InFieldTrace(chip, s["inf"], B, ies, chip.in_field_layout()[1]), s["ws"],
                          ("pow_fixed", s["x"], None, s["n"], (e).to_bytes((e.bit_length() + 7) // 8, "little")), chip, pl)
        bad, _first = r.audit()
        torch.cuda.synchronize()
        res.append((r, bad))
    return res


def _pipeline_items(w, L, B, seed):
    items = pow_items(w, L, 0, in_field=True, seed=seed)
    assert len(items) < B
    return _mix(items, [("filler", "rand", x, n) for x, _b, n in E.filler(w, L, B - len(items), seed + 1)], seed + 1)


# step_kernel, chain role: pipelined calls of > 512 elements with a trace at a step shape (kStepShapes: (64,32), (64,16), ...) are
# issued as one-launch steps (step_eligible) -- a call's chains run in the same launch as the previous sub-batch's records -- unless the
# two-queue form applies (two_queue_shape: depth >= 3 with two side streams; (64,16) only from 1,280 per call).
@pytest.mark.parametrize("w,L,B,depth,side", [(64, 32, 640, 2, 1), (64, 16, 768, 3, 2)])
def test_edge_moduli_step_chain_role(H, w, L, B, depth, side):
    from halo2_rsa_amd import _lib
    assert B > 512
    chip = H.BigIntChip(w, w * L)
    o = Oracle(w, L)
    pipe = H.Pipeline(chip, depth=depth, side_streams=side)
    assert pipe.info(B).record_form == _lib.H2R_PIPE_ONE_LAUNCH_STEP
    items = _pipeline_items(w, L, B, 11)
    _lib.profile_enable(64)
    res = _pipeline_calls(H, chip, pipe, [items, items], E.E_SPARSE, B)
    n_step = len(_lib.profile_read(_lib.KERNEL_STEP))
    _lib.profile_enable(0)
    pipe.close()
    assert n_step >= 1, n_step
    cover = Cover()
    for k, (r, bad) in enumerate(res):
        check_pow_result(chip, o, items, r.status, r.value, r.trace, r.in_field, bad, cover, "per-element", E.E_SPARSE, None, True, k)
    cover.assert_complete(["per-element"])


# The two-queue form: RSA-2048 up to 2,048 per call, RSA-1024 from 1,280 per call, on Pipeline(depth=3, side_streams=2) when the three
# streams sit on three hardware queues (else the one-launch step: either form is accepted, as in test_pipeline_two_queue_rsa1024).
@pytest.mark.parametrize("w,L,B", [(64, 32, 1024), (64, 16, 1280)])
def test_edge_moduli_two_queue_form(H, w, L, B):
    from halo2_rsa_amd import _lib
    assert (L == 32 and B <= 2048) or (L == 16 and B >= 1280)
    chip = H.BigIntChip(w, w * L)
    o = Oracle(w, L)
    pipe = H.Pipeline(chip, depth=3, side_streams=2)
    info = pipe.info(B)
    assert info.three_queues in (0, 1) and (info.record_form == _lib.H2R_PIPE_TWO_QUEUE) == (info.three_queues == 1)
    items = _pipeline_items(w, L, B, 21)
    res = _pipeline_calls(H, chip, pipe, [items] * 3, E.E_SPARSE, B)
    pipe.close()
    cover = Cover()
    for k, (r, bad) in enumerate(res):
        check_pow_result(chip, o, items, r.status, r.value, r.trace, r.in_field, bad, cover, "per-element", E.E_SPARSE, None, True, k)
    cover.assert_complete(["per-element"])


# The segmented walk: an exponent of >= 512 bits on <= 2 * num_CUs elements (exp_segment_count: min(16, bits / 128) segments), the
# (squared, acc) pair crossing launches in the workspace (SEG state); a sparse exponent keeps the deep / K = 128 chain builds.
@pytest.mark.parametrize("w,L", [(64, 32), (64, 16), (32, 128)])
def test_edge_moduli_segmented_walk(H, cus, w, L):
    e = E.E_LONG
    assert e.bit_length() >= 512
    chip = H.BigIntChip(w, w * L)
    o = Oracle(w, L)
    bits = w * L
    mods = E.by_class(E.moduli(w, L))
    full = (1 << bits) - 1
    rng = random.Random(5)
    edge = []
    for cls in E.CLASSES:
        n = mods[cls][0]
        edge += [(cls, "n-1", n - 1, n), (cls, "max", full, n)]
        if bits <= 2048:
            edge += [(cls, "rand", rng.randrange(n), n), (cls, "n", n, n), (cls, "n-1", mods[cls][-1] - 1, mods[cls][-1])]
    cover = Cover()
    for in_field in (False, True):
        items = _mix(edge, [("filler", "rand", x, n) for x, _b, n in E.filler(w, L, 3, 9)], 9)
        assert len(items) <= 2 * cus
        res = chip.pow_mod_fixed_exp(chip.assign_integer([it[2] for it in items]), e, chip.assign_integer([it[3] for it in items]),
                                     check_in_field=in_field)
        assert res.trace.num_mul_mods == e.bit_length() + bin(e).count("1")
        bad, _first = res.audit()
        torch.cuda.synchronize()
        check_pow_result(chip, o, items, res.status, res.value, res.trace, res.in_field, bad, cover, "per-element", e, None, in_field, 0)
        del res
    for cls in E.CLASSES:
        n = mods[cls][0]
        items = [(cls, "n-1", n - 1, n), ("filler", "rand", rng.randrange(n), n)]
        res = chip.pow_mod_fixed_exp(chip.assign_integer([it[2] for it in items]), e, chip.assign_integer([n]))
        bad, _first = res.audit()
        torch.cuda.synchronize()
        check_pow_result(chip, o, items, res.status, res.value, res.trace, None, bad, cover, "shared", e, None, False, 0)
        del res
    cover.assert_complete(["per-element", "shared"])
