"""Keyed moduli (H2R_F_KEYED_MODULI): a key table built once, a per-element index into it.

Every row of the build matrix of tests/test_chain_edge_moduli.py runs the same elements again as a keyed call -- the keys are the
distinct moduli of the row (so every class of edge_cases.CLASSES is a key) plus one zero key and two keys nobody names -- and is checked
twice: element by element against the C oracle and the audit (the checker of the per-element rows), and against the per-element call
on `expand()`: equal `out`, equal `status`, and for the status-0 elements equal trace bytes.  Then the index patterns, both exponent
arms and the wrappers, the life of a table (two streams, a pipelined sequence whose index staging buffer is overwritten in stream
order, a device-to-device copy) and the refusals.

The feature is reached only through names that do not exist before it (`chip.key_table`, `lib().h2r_key_table_bytes`,
`_lib.H2R_F_KEYED_MODULI`): `_feature()` is the first statement of every test.
"""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import edge_cases as E
from oracle_lib import Oracle
from test_chain_edge_moduli import (ALL_OPS, VAR_E1, VAR_EM, Cover, _compare_set, _e_dev, _first_mismatch, _flatten_mul, _mix, _pipeline_items,
                                    check_pow_result, mul_items, pow_items)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

E_SHAPE = 1


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    import halo2_rsa_amd
    return halo2_rsa_amd


@pytest.fixture(scope="module")
def cus(H):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _feature(H):
    """The names the feature arrives with; on a tree without it this is an AttributeError before any device call is made."""
    from halo2_rsa_amd import _lib
    return H.BigIntChip.key_table, _lib.lib().h2r_key_table_bytes, _lib.H2R_F_KEYED_MODULI


# ---- a row's elements as a keyed call ---------------------------------------------------------------------------------------------
def make_keys(moduli, seed=0):
    """(keys, index of every modulus): the distinct moduli in a seeded order, a zero key and two keys nobody names among them."""
    distinct = list(dict.fromkeys(moduli))
    rng = random.Random(seed)
    rng.shuffle(distinct)
    h = len(distinct) // 2
    keys = [5] + distinct[:h] + [0] + distinct[h:] + [3]   # (5 is no modulus of any row; a second 3 is never the one that is named)
    pos = {}
    for k, n in enumerate(keys):
        if k not in (0, len(keys) - 1):
            pos.setdefault(n, k)
    return keys, pos


def zero_key_tail(bits, count, seed):
    """Elements of the zero key, appended behind a row's own elements: (x, 0)."""
    rng = random.Random(seed)
    return [rng.getrandbits(bits) for _ in range(count)]


def same_as_per_element(res_k, res_p, batch, oob=()):
    """out / status / (status-0) trace bytes of the keyed call equal those of the per-element call on expand()."""
    sk, sp = res_k.status.cpu().numpy(), res_p.status.cpu().numpy()
    want = sp.copy()
    for i in oob:
        want[i] = E_SHAPE
    assert np.array_equal(sk, want), np.nonzero(sk != want)[0][:8]
    good = torch.from_numpy(np.nonzero(sk == 0)[0]).to(res_k.status.device)
    assert torch.equal(res_k.value.limbs_dev[good], res_p.value.limbs_dev[good])
    # (an element that failed has no defined out or trace.  The trace bytes are compared as the flat streams the device emits for
    #  every element: the padding between the regions of an element is nobody's to write)
    if res_k.trace is not None:
        assert torch.equal(res_k.trace.emit_stream()[good], res_p.trace.emit_stream()[good])
    if res_k.in_field is not None:
        ies = res_k.in_field.elem_stride
        assert torch.equal(res_k.in_field.buf.view(batch, ies)[good], res_p.in_field.buf.view(batch, ies)[good])
    return sk


def run_keyed_mul_mod(H, chip, o, items, cover, seed=0):
    """items: [(class, tag, a, b, n)] -- run_mul_mod's checks on the keyed call, plus the comparison with the per-element call."""
    bits = chip.limb_width * chip.num_limbs
    keys, pos = make_keys([it[4] for it in items], seed)
    zk = keys.index(0)
    tail = zero_key_tail(bits, 2, seed)
    A = [it[2] for it in items] + tail
    B = [it[3] for it in items] + tail
    idx = [pos[it[4]] for it in items] + [zk] * len(tail)
    kt = chip.key_table(keys)
    km = kt.select(idx)
    a_dev, b_dev = chip.assign_integer(A), chip.assign_integer(B)
    res = chip.mul_mod(a_dev, b_dev, km)
    ref = chip.mul_mod(a_dev, b_dev, km.expand())
    bad, _first = res.audit()
    torch.cuda.synchronize()
    assert kt.status.cpu().tolist() == [E.ZERO_MODULUS if n == 0 else 0 for n in keys]
    st = same_as_per_element(res, ref, len(A)).tolist()
    assert st[len(items):] == [E.ZERO_MODULUS] * len(tail)
    vals = res.value.to_big_uint()
    nb = bad.cpu().numpy()
    host = res.trace.buf.cpu().numpy()
    stride = res.trace.elem_stride
    cmp = _compare_set(items, seed)
    for i, (cls, tag, a, b, n) in enumerate(items):
        exp, val = E.mul_mod_expect(a, b, n, bits)
        ctx = ("keyed", cls, tag, i, hex(n))
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
            cover.cells.add(("keyed", cls))
            if tag == "limit":
                cover.limit_ok = True


def run_keyed_pow(H, chip, o, items, cover, e=None, var=None, in_field=False, seed=0):
    """items: [(class, tag, x, n)] -- run_pow's call as a keyed call, through check_pow_result, plus the per-element comparison."""
    bits = chip.limb_width * chip.num_limbs
    keys, pos = make_keys([it[3] for it in items], seed)
    zk = keys.index(0)
    tail = zero_key_tail(bits, 2, seed)
    X = [it[2] for it in items] + tail
    idx = [pos[it[3]] for it in items] + [zk] * len(tail)
    kt = chip.key_table(keys)
    km = kt.select(idx)
    x_dev = chip.assign_integer(X)

    def call(n):
        if var is None:
            return chip.pow_mod_fixed_exp(x_dev, e, n, check_in_field=in_field)
        return chip.pow_mod(x_dev, _e_dev(H, chip, var[0], len(X)), n, var[1], check_in_field=in_field)
    res = call(km)
    ref = call(km.expand())
    bad, _first = res.audit()
    torch.cuda.synchronize()
    st = same_as_per_element(res, ref, len(X))
    assert st[len(items):].tolist() == [E.ZERO_MODULUS] * len(tail)
    check_pow_result(chip, o, items, res.status, res.value, res.trace, res.in_field, bad, cover, "keyed", e, var, in_field, seed)
    return res


def run_keyed_ops(H, w, L, ops, cover, fill=16, lean_pow=False, max_batch=None, seed=0):
    chip = H.BigIntChip(w, w * L)
    o = Oracle(w, L)
    for op in ops:
        if op == "mul_mod":
            items = mul_items(w, L, fill, seed)
            assert max_batch is None or len(items) + 2 <= max_batch, (len(items), max_batch)
            run_keyed_mul_mod(H, chip, o, items, cover, seed=seed)
            continue
        kw, lean = dict(e=E.E_SPARSE), lean_pow
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
        assert max_batch is None or len(items) + 2 <= max_batch, (len(items), max_batch)
        run_keyed_pow(H, chip, o, items, cover, seed=seed, **kw)


# ---- the build matrix -----------------------------------------------------------------------------------------------------------
# K = 8, 16: chain_kernel<K,1,..,KEYED>; K = 32: chain_wave_kernel<32,..,KEYED>; K = 96, 128: the six- and eight-wave builds.
@pytest.mark.parametrize("build,w,L", [
    ("chain_kernel<8,1>", 64, 4), ("chain_kernel<8,1>", 32, 8),
    ("chain_kernel<16,1>", 64, 8), ("chain_kernel<16,1>", 32, 16),
    ("chain_wave_kernel<32>", 64, 16), ("chain_wave_kernel<32>", 64, 12), ("chain_wave_kernel<32>", 32, 32), ("chain_wave_kernel<32>", 32, 24),
    ("chain_kernel<96,6>", 64, 48), ("chain_kernel<96,6>", 64, 40), ("chain_kernel<96,6>", 32, 96),
    ("chain_kernel<128,8>", 64, 64), ("chain_kernel<128,8>", 32, 128),
])
def test_keyed_any_call_builds(H, build, w, L):
    _feature(H)
    cover = Cover()
    run_keyed_ops(H, w, L, ALL_OPS, cover, lean_pow=w * L >= 3072, max_batch=1536)
    cover.assert_complete(["keyed"])
    assert cover.limit_ok and cover.limit_over


# K = 64 at <= 2 * num_CUs elements: the deep build chain_kernel<64,4,DEEP,..,KEYED>.
@pytest.mark.parametrize("w,L", [(64, 32), (32, 64)])
def test_keyed_deep_chain(H, cus, w, L):
    _feature(H)
    cover = Cover()
    run_keyed_ops(H, w, L, ["mul_mod", "pow", "modpow"], cover, max_batch=min(2 * cus, 512))
    cover.assert_complete(["keyed"])
    assert cover.limit_ok and cover.limit_over


# The range of the two-chains-per-element build (dense or variable exponents on <= 2 * num_CUs elements): a keyed call is routed past
# chain_dual_kernel to the four-wave deep build -- same values, same items, same statuses as the per-element call, which takes it.
@pytest.mark.parametrize("w,L", [(64, 32), (32, 64)])
def test_keyed_dual_range(H, cus, w, L):
    _feature(H)
    cover = Cover()
    run_keyed_ops(H, w, L, ["pow_dense", "pow_var1", "pow_varm", "modpow_dense"], cover, max_batch=2 * cus)
    cover.assert_complete(["keyed"])


# K = 64 above max(512, 2 * num_CUs) elements: the throughput build chain_kernel<64,4,false,..,KEYED>.
@pytest.mark.parametrize("w,L", [(64, 32), (32, 64)])
def test_keyed_throughput_chain(H, cus, w, L):
    _feature(H)
    B = max(512, 2 * cus) + 64
    assert B > 512 and B > 2 * cus and (w != 64 or B + 2 <= 6 * cus)
    chip = H.BigIntChip(w, w * L)
    o = Oracle(w, L)
    cover = Cover()
    items = mul_items(w, L, 0)
    items = _mix(items, [("filler", "rand", a, b, n) for a, b, n in E.filler(w, L, B - len(items), 1)], 1)
    run_keyed_mul_mod(H, chip, o, items, cover)
    for e, in_field, lean in ((E.E_SPARSE, False, False), (E.E_SPARSE, True, False), (E.E_DENSE, False, True)):
        items = pow_items(w, L, 0, lean=lean, in_field=in_field)
        items = _mix(items, [("filler", "rand", x, n) for x, _b, n in E.filler(w, L, B - len(items), 2)], 2)
        assert len(items) == B
        run_keyed_pow(H, chip, o, items, cover, e=e, in_field=in_field)
    cover.assert_complete(["keyed"])
    assert cover.limit_ok and cover.limit_over


def _keyed_pipeline_calls(H, chip, pipe, kt, calls, e, B):
    """Pipelined modpow_public_key calls (Fix e), keyed, each on its own buffer set.  calls: [(X, key index list)].  The index of every
    call goes through ONE staging buffer that is overwritten in stream order as soon as the call before has returned; the results
    keep the index each call was made with (for expand() / audit()).  Returns [(BatchResult, bad)] after the join."""
    w, L = chip.limb_width, chip.num_limbs
    pl = chip.pow_fixed_layout(e)
    ies, isb = chip.in_field_layout()
    mk = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    staging = torch.zeros(B, dtype=torch.int32, device="cuda")
    staged = kt.select(staging)
    sets = []
    for X, idx in calls:
        own = kt.select(idx)
        s = dict(trace=mk(B * pl.elem_stride), inf=mk(B * ies), ws=mk(chip.workspace_bytes(B, pl.num_mul_mods)),
                 out=torch.zeros((B, L), dtype=chip.torch_dtype, device="cuda"), status=mk(B), x=chip.assign_integer(X), n=own)
        staging.copy_(own.key_idx, non_blocking=True)   # in stream order, right behind the previous call's launches
        pipe.modpow_public_key(s["x"], e, staged, s["trace"], s["ws"], s["out"], s["status"], in_field_buf=s["inf"])
        sets.append(s)
    staging.fill_(-1)   # ... and once more behind the last call: every index out of range, had anything read it late
    pipe.join()
    torch.cuda.synchronize()
    res = []
    for s in sets:
        r = H.BatchResult(H.AssignedInteger(s["out"], w), H.Trace(chip, s["trace"], B, pl), s["status"],
                          H.big_integer.InFieldTrace(chip, s["inf"], B, ies, isb), s["ws"],
                          ("pow_fixed", s["x"], None, s["n"], (e).to_bytes((e.bit_length() + 7) // 8, "little")), chip, pl)
        bad, _first = r.audit()
        torch.cuda.synchronize()
        res.append((r, bad))
    return res


def _per_element_pipeline_call(H, chip, pipe, x_dev, n_dev, e, B):
    """The same call with per-element moduli, alone on the pipeline: what the keyed call's bytes are compared with."""
    pl = chip.pow_fixed_layout(e)
    ies, isb = chip.in_field_layout()
    mk = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    s = dict(trace=mk(B * pl.elem_stride), inf=mk(B * ies), ws=mk(chip.workspace_bytes(B, pl.num_mul_mods)),
             out=torch.zeros((B, chip.num_limbs), dtype=chip.torch_dtype, device="cuda"), status=mk(B))
    pipe.modpow_public_key(x_dev, e, n_dev, s["trace"], s["ws"], s["out"], s["status"], in_field_buf=s["inf"])
    pipe.join()
    torch.cuda.synchronize()
    return H.BatchResult(H.AssignedInteger(s["out"], chip.limb_width), H.Trace(chip, s["trace"], B, pl), s["status"],
                         H.big_integer.InFieldTrace(chip, s["inf"], B, ies, isb), s["ws"])


def _keyed_pipeline_row(H, w, L, B, depth, side, seed, n_calls, want_step):
    from halo2_rsa_amd import _lib
    chip = H.BigIntChip(w, w * L)
    o = Oracle(w, L)
    items = _pipeline_items(w, L, B - 2, seed)
    keys, pos = make_keys([it[3] for it in items], seed)
    tail = zero_key_tail(w * L, 2, seed)
    X = [it[2] for it in items] + tail
    idx = [pos[it[3]] for it in items] + [keys.index(0)] * 2
    assert len(X) == B
    kt = chip.key_table(keys)
    pipe = H.Pipeline(chip, depth=depth, side_streams=side)
    info = pipe.info(B)
    if want_step:
        assert info.record_form == _lib.H2R_PIPE_ONE_LAUNCH_STEP
    else:
        assert info.three_queues in (0, 1) and (info.record_form == _lib.H2R_PIPE_TWO_QUEUE) == (info.three_queues == 1)
    _lib.profile_enable(64)
    res = _keyed_pipeline_calls(H, chip, pipe, kt, [(X, idx)] * n_calls, E.E_SPARSE, B)
    n_step = len(_lib.profile_read(_lib.KERNEL_STEP))
    _lib.profile_enable(0)
    if want_step:
        assert n_step >= 1, n_step
    km = kt.select(idx)
    ref = _per_element_pipeline_call(H, chip, pipe, chip.assign_integer(X), km.expand(), E.E_SPARSE, B)
    pipe.close()
    cover = Cover()
    for k, (r, bad) in enumerate(res):
        st = same_as_per_element(r, ref, B)
        assert st[B - 2:].tolist() == [E.ZERO_MODULUS] * 2
        check_pow_result(chip, o, items, r.status, r.value, r.trace, r.in_field, bad, cover, "keyed", E.E_SPARSE, None, True, k)
    cover.assert_complete(["keyed"])


# step_kernel<.., KEYED>, chain role (four-wave for RSA-2048, one-wave chains for RSA-1024): the call's chains in one launch with the
# previous call's records; the in-field witness role of the same launch reads the key table's raw plane.
@pytest.mark.parametrize("w,L,B,depth,side", [(64, 32, 640, 2, 1), (64, 16, 768, 3, 2)])
def test_keyed_step_chain_role(H, w, L, B, depth, side):
    _feature(H)
    _keyed_pipeline_row(H, w, L, B, depth, side, 11, 2, want_step=True)


# The two-queue form (or, where the three streams share a hardware queue, the one-launch step: either is accepted, as in the
# per-element row).
@pytest.mark.parametrize("w,L,B", [(64, 32, 1024), (64, 16, 1280)])
def test_keyed_two_queue_form(H, w, L, B):
    _feature(H)
    _keyed_pipeline_row(H, w, L, B, 3, 2, 21, 3, want_step=False)


# The segmented walk (an exponent of >= 512 bits on <= 2 * num_CUs elements): every segment's launch takes the key's entry again.
@pytest.mark.parametrize("w,L", [(64, 32), (64, 16), (32, 128)])
def test_keyed_segmented_walk(H, cus, w, L):
    _feature(H)
    e = E.E_LONG
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
        assert len(items) + 2 <= 2 * cus
        res = run_keyed_pow(H, chip, o, items, cover, e=e, in_field=in_field)
        assert res.trace.num_mul_mods == e.bit_length() + bin(e).count("1")
        del res
    cover.assert_complete(["keyed"])


# ---- index patterns ---------------------------------------------------------------------------------------------------------------
def _check_indexed(chip, o, keys, idx, X, res, bad, e, in_field, sample):
    """Every element by rule (out of range: H2R_E_SHAPE; the zero key: H2R_E_ZERO_MODULUS; else Python's pow), the audit for every
    status-0 element, the whole flat stream against the oracle for the elements in `sample`."""
    bits = chip.limb_width * chip.num_limbs
    st = res.status.cpu().tolist()
    vals = res.value.to_big_uint()
    nb = bad.cpu().numpy()
    n_ok = 0
    for i, (k, x) in enumerate(zip(idx, X)):
        if k >= len(keys):
            assert st[i] == E_SHAPE, (i, k, st[i])
            continue
        n = keys[k]
        exp, val = E.pow_fixed_expect(x, e, n, bits, in_field)
        assert st[i] == exp, (i, k, st[i], exp)
        if exp:
            continue
        n_ok += 1
        assert vals[i] == val and nb[i] == 0, (i, k)
        if i in sample:
            rc, oo, ost = o.pow_mod_fixed_exp(o.limbs(x), o.limbs(n), e)
            assert rc == 0 and o.to_int(oo) == val
            got = res.trace.flatten(i)
            assert np.array_equal(got, ost), (i, _first_mismatch(got, ost))
            if in_field:
                _rc, _lt, s_if = o.assert_in_field(o.limbs(x), o.limbs(n))
                assert np.array_equal(res.in_field.flatten(i), s_if), (i, "in-field")
    return n_ok


@pytest.mark.parametrize("bits", [2048, 1024])
def test_keyed_index_patterns(H, bits):
    _feature(H)
    w, L, e, B = 64, bits // 64, 65537, 96
    chip = H.BigIntChip(w, bits)
    o = Oracle(w, L)
    rng = random.Random(bits)
    pool = [n for _x, _b, n in E.filler(w, L, B, 77)]
    assert len(set(pool)) == B

    def run(keys, idx, tag):
        X = [rng.randrange(keys[k]) if (k < len(keys) and keys[k]) else rng.getrandbits(bits) for k in idx]
        kt = chip.key_table(keys)
        km = kt.select(idx)
        x_dev = chip.assign_integer(X)
        res = chip.pow_mod_fixed_exp(x_dev, e, km, check_in_field=True)
        ref = chip.pow_mod_fixed_exp(x_dev, e, km.expand(), check_in_field=True)
        bad, _first = res.audit()
        torch.cuda.synchronize()
        oob = [i for i, k in enumerate(idx) if k >= len(keys)]
        same_as_per_element(res, ref, B, oob)
        sample = set(random.Random(tag).sample(range(B), 6)) | {i + d for i in oob for d in (-1, 1) if 0 <= i + d < B}
        return _check_indexed(chip, o, keys, idx, X, res, bad, e, True, sample), res.status.cpu().tolist()

    n_ok, _ = run(pool[:1], [0] * B, "one key")
    assert n_ok == B
    for nk in (3, 16):
        n_ok, _ = run(pool[:nk], [i % nk for i in range(B)], "round robin %d" % nk)
        assert n_ok == B
    n_ok, _ = run(pool[:16], [rng.randrange(16) for _ in range(B)], "random")
    assert n_ok == B
    perm = list(range(B))
    rng.shuffle(perm)
    n_ok, _ = run(pool, perm, "num_keys == batch")
    assert n_ok == B
    # two indices out of range (num_keys and 2^32 - 1) between in-range neighbours, which match the oracle (they are in the sample)
    keys = pool[:5]
    idx = [i % 5 for i in range(B)]
    idx[17], idx[40] = len(keys), 0xFFFFFFFF
    n_ok, st = run(keys, idx, "out of range")
    assert n_ok == B - 2 and st[17] == st[40] == E_SHAPE and st[16] == st[18] == st[39] == st[41] == 0
    # the zero key: its elements get H2R_E_ZERO_MODULUS, exactly as a per-element zero modulus does
    keys = pool[:2] + [0] + pool[2:4]
    idx = [i % 5 for i in range(B)]
    n_ok, st = run(keys, idx, "zero key")
    assert n_ok == B - len([k for k in idx if k == 2]) and all(st[i] == (E.ZERO_MODULUS if k == 2 else 0) for i, k in enumerate(idx))
    # no keys at all: every index is out of range
    n_ok, st = run([], [0] * B, "no keys")
    assert n_ok == 0 and st == [E_SHAPE] * B


# ---- both exponent arms and the wrappers ------------------------------------------------------------------------------------------
def _kats(golden):
    k = golden["rsa_kats"]
    return [int(v["n"]) for v in k], [int(v["sig"]) for v in k], [int(v["hashed"]) for v in k], [int(v["is_valid"]) for v in k]


def test_keyed_var_modpow_public_key(H, golden):
    """RSAPubE::Var through RSAChip.modpow_public_key: e = 65537 as four 5-bit limbs, the three KAT keys in one call."""
    _feature(H)
    ns, sigs, _hashed, _ok = _kats(golden)
    rsa = H.RSAChip(2048, 5)
    chip = rsa.bigint_chip()
    o = Oracle(64, 32)
    e_limbs = [(65537 >> (5 * i)) & 31 for i in range(4)]
    B = 24
    rng = random.Random(4)
    keys = [ns[2], 0, ns[0], ns[1]]
    idx = [(0, 2, 3)[i % 3] for i in range(B)]
    idx[5], idx[9] = 1, len(keys)
    X = [sigs[{0: 2, 2: 0, 3: 1}[k]] if k in (0, 2, 3) and i < 3 else rng.getrandbits(2040) for i, k in enumerate(idx)]
    km = chip.key_table(keys).select(idx)
    ev = H.UnassignedInteger(np.array([e_limbs] * B, dtype=np.uint64))
    x_dev = chip.assign_integer(X)
    res = rsa.modpow_public_key(x_dev, rsa.assign_public_key(H.RSAPublicKey(km, H.Var(ev))))
    ref = rsa.modpow_public_key(x_dev, rsa.assign_public_key(H.RSAPublicKey(km.expand(), H.Var(ev))))
    bad, _first = res.audit()
    torch.cuda.synchronize()
    st = same_as_per_element(res, ref, B, oob=[9]).tolist()
    assert st[5] == E.ZERO_MODULUS and st[9] == E_SHAPE
    items = [("kat", "var", x, keys[k]) for x, k in zip(X, idx) if k < len(keys) and keys[k]]
    keep = [i for i, k in enumerate(idx) if k < len(keys) and keys[k]]
    assert keep == [i for i in range(B) if i not in (5, 9)]
    # (check_pow_result walks a dense batch: the two refused elements are checked above, the rest through a gathered view)
    sel = torch.tensor(keep, device="cuda")
    es, ies = res.trace.elem_stride, res.in_field.elem_stride
    tr = H.Trace(chip, res.trace.buf.view(B, es)[sel].contiguous().view(-1), len(keep), res.trace.pow_layout)
    inf = H.big_integer.InFieldTrace(chip, res.in_field.buf.view(B, ies)[sel].contiguous().view(-1), len(keep), ies, res.in_field.stream_bytes)
    cover = Cover()
    check_pow_result(chip, o, items, res.status[sel], H.AssignedInteger(res.value.limbs_dev[sel].contiguous(), 64), tr, inf, bad[sel], cover,
                     "keyed", None, (e_limbs, 5), True, 0)


def test_keyed_verify_pkcs1v15_kats(H, golden):
    """RSAChip.verify_pkcs1v15_signature under three keys in one call: is_valid = 1, 1, 0 (src/chip.rs:703-713, 748-758, 798)."""
    _feature(H)
    ns, sigs, hashed, ok = _kats(golden)
    assert ok == [1, 1, 0]
    rsa = H.RSAChip(2048, 5)
    chip = rsa.bigint_chip()
    o = Oracle(64, 32)
    keys = [ns[1], ns[2], 7, ns[0]]
    idx = [3, 0, 1]
    km = chip.key_table(keys).select(idx)
    sg = rsa.assign_signature(H.RSASignature(H.UnassignedInteger.from_ints(sigs, 32, 64)))
    for pub_e in (H.Fix(65537), H.Var(H.UnassignedInteger(np.array([[(65537 >> (5 * i)) & 31 for i in range(4)]] * 3, dtype=np.uint64)))):
        res = rsa.verify_pkcs1v15_signature(rsa.assign_public_key(H.RSAPublicKey(km, pub_e)), hashed, sg)
        ref = rsa.verify_pkcs1v15_signature(rsa.assign_public_key(H.RSAPublicKey(km.expand(), pub_e)), hashed, sg)
        torch.cuda.synchronize()
        assert res.status.cpu().tolist() == [0, 0, 0] and res.is_valid.cpu().tolist() == [1, 1, 0]
        assert torch.equal(res.powed.limbs_dev, ref.powed.limbs_dev)
        assert all(np.array_equal(res.flatten(i), ref.flatten(i)) for i in range(3))
        assert torch.equal(res.emit_advice(), ref.emit_advice())   # (a keyed result expands for the emitter)
        if isinstance(pub_e, H.Fix):
            hl = H.hashed_msg_from_digest(hashlib.sha256(b"hello world").digest()).limbs[0]
            for i in range(3):
                _, _, s_if = o.assert_in_field(o.limbs(sigs[i]), o.limbs(ns[i]))
                _, out, s_pow = o.pow_mod_fixed_exp(o.limbs(sigs[i]), o.limbs(ns[i]), 65537)
                _, valid, s_em = o.pkcs1v15_em_check(out, hl)
                assert valid == ok[i]
                assert np.array_equal(res.flatten(i), np.concatenate([s_if, s_pow, s_em]))


def test_keyed_signature_verifier(H, golden):
    """RSASignatureVerifier from message bytes with a keyed key set, plain and pipelined; an index out of range and the zero key."""
    _feature(H)
    ns, sigs, _hashed, ok = _kats(golden)
    rsa = H.RSAChip(2048, 5)
    chip = rsa.bigint_chip()
    verifier = H.RSASignatureVerifier(rsa)
    keys = [ns[0], 0, ns[1], ns[2]]
    idx = [0, 2, 3, 1, 9, 0]
    msgs = [b"hello world"] * 3 + [b"hello world", b"hello world", b"hello world!"]
    sg = H.RSASignature(H.UnassignedInteger.from_ints(sigs + [sigs[0], sigs[0], sigs[0]], 32, 64))
    kt = chip.key_table(keys)
    km = kt.select(idx)
    res = verifier.verify_pkcs1v15_signature(H.RSAPublicKey(km, H.Fix(65537)), msgs, sg)
    ref = verifier.verify_pkcs1v15_signature(H.RSAPublicKey(km.expand(), H.Fix(65537)), msgs, sg)
    torch.cuda.synchronize()
    assert res.status.cpu().tolist() == [0, 0, 0, E.ZERO_MODULUS, E_SHAPE, 0]
    assert res.is_valid.cpu().tolist() == [1, 1, 0, 0, 0, 0]
    good = torch.tensor([0, 1, 2, 5], device="cuda")
    es = res.layout.elem_stride
    assert all(np.array_equal(res.flatten(i), ref.flatten(i)) for i in (0, 1, 2, 5)) and torch.equal(res.powed.limbs_dev[good], ref.powed.limbs_dev[good])
    assert ref.status.cpu().tolist() == [0, 0, 0, E.ZERO_MODULUS, E.ZERO_MODULUS, 0]
    # pipelined (h2r_pipeline_signature_verifier), two calls on rotating buffers
    pipe = H.Pipeline(chip, depth=2, side_streams=1)
    buf, off = H.pack_messages(msgs, "cuda")
    sig_dev = chip.assign_integer(sg.c)
    outs = []
    for _ in range(2):
        b = dict(trace=torch.zeros(6 * es, dtype=torch.uint8, device="cuda"), ws=torch.zeros(chip.workspace_bytes(6, res.layout.pow.num_mul_mods), dtype=torch.uint8, device="cuda"),
                 powed=torch.zeros((6, 32), dtype=torch.int64, device="cuda"), valid=torch.zeros(6, dtype=torch.uint8, device="cuda"),
                 status=torch.zeros(6, dtype=torch.uint8, device="cuda"), hashed=torch.zeros((6, 4), dtype=torch.int64, device="cuda"))
        pipe.signature_verifier(buf, off, 0, sig_dev, 65537, km, b["trace"], b["ws"], b["powed"], b["valid"], b["status"], b["hashed"])
        outs.append(b)
    pipe.join()
    torch.cuda.synchronize()
    pipe.close()
    for b in outs:
        assert b["status"].cpu().tolist() == [0, 0, 0, E.ZERO_MODULUS, E_SHAPE, 0] and b["valid"].cpu().tolist() == [1, 1, 0, 0, 0, 0]
        piped = H.rsa.VerifyResult(b["valid"], H.AssignedInteger(b["powed"], 64), b["status"], b["trace"], res.layout, chip)
        assert all(np.array_equal(piped.flatten(i), res.flatten(i)) for i in (0, 1, 2, 5)) and torch.equal(b["powed"][good], res.powed.limbs_dev[good])


def test_keyed_cpp_host_mirror(H):
    """include/h2r_chips.hpp: KeyTable / AssignedInteger::keyed through the verifier and square_mod (tests/cpp/test_keyed_chip.cpp)."""
    _feature(H)
    import os
    import subprocess
    from cpp_build import build_cpp
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = build_cpp("test_keyed_chip")
    out = subprocess.run([exe, os.path.join(root, "tests", "golden", "rsa_kats_limbs.txt")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "CPP_KEYED_MIRROR_OK 5" in out.stdout


# ---- the life of a table ----------------------------------------------------------------------------------------------------------
def test_one_table_two_streams_and_a_copy(H):
    """One table serves calls on two streams at once; a device-to-device copy of it gives the same results."""
    _feature(H)
    w, L, e, B = 64, 32, 65537, 192
    chip = H.BigIntChip(w, w * L)
    o = Oracle(w, L)
    rng = random.Random(8)
    keys = [n for _x, _b, n in E.filler(w, L, 7, 5)]
    kt = chip.key_table(keys)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    runs = []
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())   # (the table's build is ordered in front of both)
        idx = [rng.randrange(len(keys)) for _ in range(B)]
        X = [rng.randrange(keys[k]) for k in idx]
        with torch.cuda.stream(s):
            res = chip.pow_mod_fixed_exp(chip.assign_integer(X), e, kt.select(idx), check_in_field=True)
        runs.append((idx, X, res))
    for s in streams:
        s.synchronize()
    for idx, X, res in runs:
        bad, _first = res.audit()
        torch.cuda.synchronize()
        assert _check_indexed(chip, o, keys, idx, X, res, bad, e, True, set(range(0, B, 37))) == B
    idx, X, res = runs[0]
    kt2 = kt.copy()
    assert kt2.buf.data_ptr() != kt.buf.data_ptr()
    res2 = chip.pow_mod_fixed_exp(chip.assign_integer(X), e, kt2.select(idx), check_in_field=True)
    torch.cuda.synchronize()
    assert torch.equal(res2.status, res.status) and torch.equal(res2.value.limbs_dev, res.value.limbs_dev)
    assert torch.equal(res2.trace.emit_stream(), res.trace.emit_stream())
    assert torch.equal(res2.in_field.buf, res.in_field.buf)


@pytest.mark.parametrize("bits,B", [(2048, 1024), (1024, 2048)])
def test_one_table_pipelined_sequence_with_refilled_index(H, bits, B):
    """Depth 3, two side streams, eight calls on one table; the caller's key_idx staging buffer is overwritten in stream order right
    after each call returns (and once more behind the last).  Every call is audited after the join."""
    _feature(H)
    w, L, e, n_calls = 64, bits // 64, 65537, 8
    chip = H.BigIntChip(w, bits)
    o = Oracle(w, L)
    rng = random.Random(bits + 1)
    keys = [n for _x, _b, n in E.filler(w, L, 16, 6)] + [0]
    kt = chip.key_table(keys)
    calls = []
    for c in range(n_calls):
        idx = [rng.randrange(16) for _ in range(B)]
        idx[c], idx[B - 1 - c] = 16, len(keys) + c      # the zero key and an index out of range, elsewhere in every call
        X = [rng.randrange(keys[k]) if (k < len(keys) and keys[k]) else rng.getrandbits(bits) for k in idx]
        calls.append((X, idx))
    pipe = H.Pipeline(chip, depth=3, side_streams=2)
    res = _keyed_pipeline_calls(H, chip, pipe, kt, calls, e, B)
    pipe.close()
    for c, ((X, idx), (r, bad)) in enumerate(zip(calls, res)):
        sample = set(random.Random(c).sample(range(B), 4)) | {c + 1, B - 2 - c}
        assert _check_indexed(chip, o, keys, idx, X, r, bad, e, True, sample) == B - 2, c


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
NOT_KEYED = {   # export: (position of n, position of flags)
    "h2r_fresh_op_batch": (4, 6), "h2r_fresh_op_emit_advice": (5, 2),
    "h2r_mul_mod_emit_advice": (3, 4), "h2r_pow_trace_emit_advice": (2, 3), "h2r_modpow_public_key_emit_advice": (3, 4), "h2r_verify_emit_advice": (3, 6),
    "h2r_pipeline_modpow_public_key_advice": (2, 6), "h2r_pipeline_modpow_public_key_var_advice": (5, 7),
    "h2r_pipeline_verify_pkcs1v15_advice": (2, 7), "h2r_pipeline_verify_pkcs1v15_var_advice": (2, 8),
    "h2r_mul_mod_trace_check": (3, 4), "h2r_pow_trace_check": (3, 6), "h2r_advice_check": (13, 14),
}


def test_refusals(H):
    _feature(H)
    from halo2_rsa_amd import _lib
    L_ = _lib.lib()
    KEYED, UNSUP = _lib.H2R_F_KEYED_MODULI, _lib.H2R_E_UNSUPPORTED
    chip = H.BigIntChip(64, 2048)
    B = 4
    keys = [n for _x, _b, n in E.filler(64, 32, 3, 1)]
    kt = chip.key_table(keys)
    km = kt.select([0, 1, 2, 0])
    n_dev = km.expand()                      # a valid device buffer of per-element moduli
    x = chip.assign_integer([5, 6, 7, 8])
    out = chip._new_limbs(B)
    status = torch.zeros(B, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    # both flags together; a struct of another size (the struct is the keyed call's own, valid one)
    rc = L_.h2r_mul_mod_batch(chip._ctx, x.data_ptr(), x.data_ptr(), km.data_ptr(), B, KEYED | _lib.H2R_F_SHARED_MODULUS, None, out.data_ptr(),
                              status.data_ptr(), None, chip._stream())
    assert rc == UNSUP
    for size in (0, ctypes.sizeof(_lib.H2RKeyedModuli) - 8, ctypes.sizeof(_lib.H2RKeyedModuli) + 8):
        bad = _lib.H2RKeyedModuli(size, 0, kt.num_keys, kt.buf.data_ptr(), km.key_idx.data_ptr())
        rc = L_.h2r_pow_mod_fixed_exp_batch(chip._ctx, x.data_ptr(), ctypes.addressof(bad), b"\x03", 1, B, KEYED, None, out.data_ptr(), status.data_ptr(),
                                            None, chip._stream())
        assert rc == UNSUP, size
    # every export that takes n and flags but is not keyed answers H2R_E_UNSUPPORTED to the flag before it looks at n.  n IS a valid
    # device buffer of per-element moduli here, so an export without the guard shows as another return code, not as a fault.
    pipe = H.Pipeline(chip, depth=2, side_streams=1)
    for name, (n_pos, f_pos) in NOT_KEYED.items():
        fn = getattr(L_, name)
        args = []
        for k, t in enumerate(fn.argtypes):
            if k == 0:
                args.append(pipe._p if name.startswith("h2r_pipeline_") else chip._ctx)
            elif k == n_pos:
                args.append(n_dev.data_ptr())
            elif k == f_pos:
                args.append(KEYED)
            elif t in (ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t):
                args.append(0)
            else:
                args.append(None)
        assert fn(*args) == UNSUP, name
    pipe.close()
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * B    # nothing ran
