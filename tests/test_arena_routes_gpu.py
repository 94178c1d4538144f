"""Every route that writes records, into a trace arena's kept regions (include/h2r.h, trace arena).  run_path is the common driver of all
of them and decides in one place (on_arena_slots) whether a launch may leave the seven constant planes of its records alone; a wrong "yes"
leaves stale bytes inside an otherwise correct witness.  tests/test_arena_constants_gpu.py drives the pipelined fixed-exponent call; here:
the plain exports (with and without a caller workspace), mul_mod / square_mod, the per-element-exponent exports, the verifier (stream-ordered,
side-stream and one-launch-step forms), the plain export's walks (sub-batches of elements, segments of a long exponent), shared and keyed
moduli, calls from other contexts, and every slot of a region stitched from two physical chunks.

Every route gets the same three assertions, byte-exact:
  A. into a kept region the test has not written, next to a zero-filled plain twin: statuses and results equal, every status-0 element equal
     across the whole element stride, the first and last status-0 elements' flat streams equal the oracle's, the in-place audit clean;
  B. into a 0xA5-filled region: exact outside the constant planes, inside them every record either all 0xA5 or all the twin's bytes (all 0xA5
     except where the verifier's step launches write the records), the audit flags exactly the elements that kept 0xA5, and after
     arena.restore() the region equals the twin and the audit is clean;
  C. a twin that must not match (256 bytes into the region, or a geometry the arena was not created for) writes complete records.
Elements with a nonzero status are left out of the comparisons (their trace is unspecified): at most two per case, planted at the first and
the last slot the call uses, and the set of nonzero statuses is asserted to be exactly the planted set.  (The oracle's streams are therefore
compared for the first and the last status-0 element.)

What these tests found.  Records written into a freshly created region were lost in 3 to 7 of these 32 cases per run: complete when first
read (out of the caches), then the region read back as the zero fill or the look had left it.  The region's address range had been freed
with hipMemAddressFree by an earlier candidate or arena and reserved again, and the device kept the old translation for a while, so the
stores went to the released chunks.  A loop (create the arena, one 13-element call into region 0, checksum at once and 30 ms later, close)
lost records in 33 of 40 arenas; with the ranges retired instead of freed (h2r_api.hip, RetiredRanges) in 0 of 40, and this file passed
three times in a row.  Neither the candidate's memset nor keep_const had a part in it."""
import ctypes
import random
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle_lib import Oracle  # noqa: E402
from test_arena_constants_gpu import CONST_PLANES, Calls, const_plane_mask  # noqa: E402

E = 65537
OFF = 5          # the arenas hold OFF more elements than a call: calls at element offset OFF and 256 bytes into the region fit


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    import halo2_rsa_amd
    return halo2_rsa_amd


def _ck(rc, where):
    from halo2_rsa_amd import _lib
    _lib.check(rc, where)


def _p(t):
    return t.data_ptr() if t is not None else None


def _inputs(w, L, B, seed, planted, in_field):
    """Moduli with the top bit set and operands below them; the planted elements have x >= n: n + 1 where the call asserts x < n
    (H2R_E_NOT_IN_FIELD), 2^(wL) - 1 elsewhere -- its square over any n <= 2^(wL) - 2 does not fit L limbs (H2R_E_NOT_REDUCED)."""
    rng = random.Random(seed)
    top = (1 << (w * L)) - 1
    N = [rng.getrandbits(w * L) | (1 << (w * L - 1)) | 1 for _ in range(B)]
    assert all(n < top - 1 for n in N)
    X = [rng.randrange(n) for n in N]
    for i in planted:
        X[i] = N[i] + 1 if in_field else top
    return X, N


class Route:
    """One export bound to one set of inputs (the Calls pattern of test_arena_constants_gpu): run() makes the call once per target trace
    buffer, back to back, then joins.  elem_stride / T / off_records describe where the call puts its records."""
    pipe = None

    def __init__(self, H, chip, B, ES, T, planted):
        self.H, self.chip, self.B, self.ES, self.T, self.planted = H, chip, B, ES, T, planted
        self.o = Oracle(chip.limb_width, chip.num_limbs)
        self.cmask = const_plane_mask(chip, SimpleNamespace(elem_stride=ES, num_mul_mods=T, off_records=0))
        from halo2_rsa_amd import _lib
        per_record = 2 * chip.num_limbs * sum(chip.layout.plane_elem[_lib.PLANES.index(p)] for p in CONST_PLANES)
        assert int(self.cmask.sum()) == T * per_record

    def run(self, targets, null_ws=False):
        chip, B = self.chip, self.B
        assert len(targets) <= 3
        sets = []
        for tb in targets:
            assert tb.numel() == B * self.ES
            s = SimpleNamespace(trace=tb, ws=None if null_ws else torch.zeros(chip.workspace_bytes(B, self.T), dtype=torch.uint8, device="cuda"),
                                out=torch.zeros((B, chip.num_limbs), dtype=chip.torch_dtype, device="cuda"),
                                status=torch.zeros(B, dtype=torch.uint8, device="cuda"), valid=torch.zeros(B, dtype=torch.uint8, device="cuda"))
            self.issue(s)
            sets.append(s)
        if self.pipe is not None:
            self.pipe.join()
        torch.cuda.synchronize()
        return sets

    def rows(self, buf, first=0):
        return buf[first * self.ES:(first + self.B) * self.ES].view(self.B, self.ES)

    def audit(self, s, ws=None):
        """The in-place audit of the records in s.trace (BatchResult.audit); `ws`: the operands of an identical call, where this one
        was made without a caller workspace."""
        from halo2_rsa_amd import big_integer as BI
        tr = self.trace_of(s.trace)
        res = BI.BatchResult(self.H.AssignedInteger(s.out, self.chip.limb_width), tr, s.status, workspace=s.ws if s.ws is not None else ws,
                             inputs=self.audit_inputs())
        bad, _ = res.audit()
        torch.cuda.synchronize()
        return bad.cpu().numpy()

    def close(self):
        if self.pipe is not None:
            self.pipe.close()


class PowFixed(Route):
    """export: "pow" (h2r_pow_mod_fixed_exp_batch), "modpow" (h2r_modpow_public_key_batch) or "pipe" (h2r_pipeline_modpow_public_key).
    n: integers (one per element, or one for the whole batch: H2R_F_SHARED_MODULUS) or (keys, key_idx): H2R_F_KEYED_MODULI."""

    def __init__(self, H, chip, export, e, X, n, planted, moduli=None):
        from halo2_rsa_amd import big_integer as BI
        self.pl = chip.pow_fixed_layout(e)
        super().__init__(H, chip, len(X), self.pl.elem_stride, self.pl.num_mul_mods, planted)
        self.export, self.e, self.eb, self.X = export, e, BI._e_bytes(e), X
        self.x = chip.assign_integer(X)
        if isinstance(n, tuple):
            keys, idx = n
            self.table = chip.key_table(keys)
            self.n = self.table.select(idx)
            self.moduli = [keys[k] if k < len(keys) else None for k in idx]
        else:
            self.n = chip.assign_integer(n)
            self.moduli = list(n) * (self.B if len(n) == 1 else 1)
        self.flags = chip._flags(self.n, self.B)
        if export == "pipe":
            self.pipe = H.Pipeline(chip, depth=3, side_streams=2)

    def issue(self, s):
        c, L_ = self.chip, self.H.lib()
        if self.export == "pow":
            _ck(L_.h2r_pow_mod_fixed_exp_batch(c._ctx, self.x.data_ptr(), self.n.data_ptr(), self.eb, len(self.eb), self.B, self.flags, _p(s.trace),
                                               _p(s.out), _p(s.status), _p(s.ws), c._stream()), "h2r_pow_mod_fixed_exp_batch")
        elif self.export == "modpow":
            _ck(L_.h2r_modpow_public_key_batch(c._ctx, self.x.data_ptr(), self.n.data_ptr(), self.eb, len(self.eb), self.B, self.flags, _p(s.trace),
                                               None, _p(s.out), _p(s.status), _p(s.ws), c._stream()), "h2r_modpow_public_key_batch")
        else:
            self.pipe.modpow_public_key(self.x, self.e, self.n, s.trace, s.ws, s.out, s.status)

    def trace_of(self, buf):
        return self.H.Trace(self.chip, buf, self.B, self.pl)

    def audit_inputs(self):
        return ("pow_fixed", self.x, None, self.n, self.eb)

    def flat(self, s, i):
        return self.trace_of(s.trace).flatten(i)

    def oracle(self, s, i):
        o = self.o
        rc, out, st = o.pow_mod_fixed_exp(o.limbs(self.X[i]), o.limbs(self.moduli[i]), self.e)
        assert rc == 0 and o.to_int(out) == pow(self.X[i], self.e, self.moduli[i])
        return st


class PowVar(Route):
    """export: "pow" (h2r_pow_mod_batch), "modpow" (h2r_modpow_public_key_var_batch) or "pipe" (h2r_pipeline_modpow_public_key_var)."""

    def __init__(self, H, chip, export, e_num_limbs, exp_limb_bits, X, EXP, N, planted):
        self.pl = chip.pow_var_layout(e_num_limbs, exp_limb_bits)
        super().__init__(H, chip, len(X), self.pl.elem_stride, self.pl.num_mul_mods, planted)
        self.export, self.bits, self.X, self.EXP, self.moduli = export, exp_limb_bits, X, EXP, N
        self.x, self.n = chip.assign_integer(X), chip.assign_integer(N)
        ev = np.array(EXP, dtype=chip.np_dtype).reshape(self.B, e_num_limbs)
        self.ev = H.AssignedInteger(torch.from_numpy(ev.view(np.int64 if chip.limb_width == 64 else np.int32)).cuda().contiguous(), chip.limb_width)
        if export == "pipe":
            self.pipe = H.Pipeline(chip, depth=3, side_streams=2)

    def issue(self, s):
        c, L_, ev = self.chip, self.H.lib(), self.ev
        if self.export == "pow":
            _ck(L_.h2r_pow_mod_batch(c._ctx, self.x.data_ptr(), ev.data_ptr(), ev.num_limbs(), self.bits, self.n.data_ptr(), self.B, 0, _p(s.trace),
                                     _p(s.out), _p(s.status), _p(s.ws), c._stream()), "h2r_pow_mod_batch")
        elif self.export == "modpow":
            _ck(L_.h2r_modpow_public_key_var_batch(c._ctx, self.x.data_ptr(), ev.data_ptr(), ev.num_limbs(), self.bits, self.n.data_ptr(), self.B, 0,
                                                   _p(s.trace), None, _p(s.out), _p(s.status), _p(s.ws), c._stream()), "h2r_modpow_public_key_var_batch")
        else:
            self.pipe.modpow_public_key_var(self.x, ev, self.bits, self.n, s.trace, s.ws, s.out, s.status)

    def trace_of(self, buf):
        return self.H.Trace(self.chip, buf, self.B, self.pl)

    def audit_inputs(self):
        return ("pow_var", self.x, None, self.n, None)

    def flat(self, s, i):
        return self.trace_of(s.trace).flatten(i)

    def oracle(self, s, i):
        o = self.o
        rc, out, st = o.pow_mod(o.limbs(self.X[i]), np.atleast_1d(np.array(self.EXP[i], dtype=o.dtype)), self.bits, o.limbs(self.moduli[i]))
        e = sum(int(v) << (self.bits * k) for k, v in enumerate(np.atleast_1d(self.EXP[i])))
        assert rc == 0 and o.to_int(out) == pow(self.X[i], e, self.moduli[i])
        return st


class MulMod(Route):
    """h2r_mul_mod_batch, or h2r_square_mod_batch when Bv is None: one record per element, element stride = record stride."""

    def __init__(self, H, chip, A, Bv, N, planted):
        super().__init__(H, chip, len(A), chip.layout.record_stride, 1, planted)
        self.A, self.Bv, self.moduli = A, Bv, N
        self.a, self.n = chip.assign_integer(A), chip.assign_integer(N)
        self.b = chip.assign_integer(Bv) if Bv is not None else None

    def issue(self, s):
        c, L_ = self.chip, self.H.lib()
        if self.b is not None:
            _ck(L_.h2r_mul_mod_batch(c._ctx, self.a.data_ptr(), self.b.data_ptr(), self.n.data_ptr(), self.B, 0, _p(s.trace), _p(s.out), _p(s.status),
                                     _p(s.ws), c._stream()), "h2r_mul_mod_batch")
        else:
            _ck(L_.h2r_square_mod_batch(c._ctx, self.a.data_ptr(), self.n.data_ptr(), self.B, 0, _p(s.trace), _p(s.out), _p(s.status), _p(s.ws),
                                        c._stream()), "h2r_square_mod_batch")

    def trace_of(self, buf):
        return self.H.Trace(self.chip, buf, self.B, None)

    def audit_inputs(self):
        return ("mul_mod", self.a, self.b if self.b is not None else self.a, self.n, None)

    def flat(self, s, i):
        return self.trace_of(s.trace).flatten(i)

    def oracle(self, s, i):
        o = self.o
        b = self.Bv[i] if self.Bv is not None else self.A[i]
        rc, r, st = o.mul_mod(o.limbs(self.A[i]), o.limbs(b), o.limbs(self.moduli[i]))
        assert rc == 0 and o.to_int(r) == self.A[i] * b % self.moduli[i]
        return st


class Verify(Route):
    """h2r_verify_pkcs1v15_batch (pipe is None) or h2r_pipeline_verify_pkcs1v15: the pow element's records sit at offset 0 of a VERIFY element."""

    def __init__(self, H, chip, pipe, SIG, N, HASHED, planted):
        from halo2_rsa_amd import _lib, big_integer as BI
        self.eb = BI._e_bytes(E)
        self.vl = _lib.H2RVerifyLayout()
        _ck(H.lib().h2r_verify_layout_fixed(chip._ctx, self.eb, len(self.eb), ctypes.byref(self.vl)), "h2r_verify_layout_fixed")
        assert self.vl.pow.off_records == 0
        super().__init__(H, chip, len(SIG), self.vl.elem_stride, self.vl.pow.num_mul_mods, planted)
        self.pipe, self.X, self.moduli, self.HASHED = pipe, SIG, N, HASHED
        self.x, self.n = chip.assign_integer(SIG), chip.assign_integer(N)
        self.h = torch.from_numpy(H.UnassignedInteger.from_ints(HASHED, 4, 64).limbs.view(np.int64)).cuda()

    def issue(self, s):
        c = self.chip
        if self.pipe is None:
            _ck(self.H.lib().h2r_verify_pkcs1v15_batch(c._ctx, self.x.data_ptr(), self.n.data_ptr(), self.eb, len(self.eb), self.h.data_ptr(), self.B, 0,
                                                       _p(s.trace), _p(s.out), _p(s.valid), _p(s.status), _p(s.ws), c._stream()), "h2r_verify_pkcs1v15_batch")
        else:
            self.pipe.verify_pkcs1v15(self.x, E, self.n, self.h, s.trace, s.ws, s.out, s.valid, s.status)

    def trace_of(self, buf):
        tr = self.H.Trace(self.chip, buf, self.B, self.vl.pow)
        tr.elem_stride = self.vl.elem_stride          # (the audit walks the pow element inside every verify element)
        return tr

    def audit_inputs(self):
        return ("pow_fixed", self.x, None, self.n, self.eb)

    def flat(self, s, i):
        return self.H.rsa.VerifyResult(s.valid, self.H.AssignedInteger(s.out, 64), s.status, s.trace, self.vl, self.chip).flatten(i)

    def oracle(self, s, i):
        o = self.o
        rc_if, lt, s_if = o.assert_in_field(o.limbs(self.X[i]), o.limbs(self.moduli[i]))
        rc, out, s_pow = o.pow_mod_fixed_exp(o.limbs(self.X[i]), o.limbs(self.moduli[i]), E)
        rc_em, ok, s_em = o.pkcs1v15_em_check(out, o.limbs(self.HASHED[i], 4))
        assert rc_if == 0 and lt == 1 and rc == 0 and ok == int(s.valid[i].item())
        return np.concatenate([s_if, s_pow, s_em])


# ---- the three assertions ------------------------------------------------------------------------------------------------------------------
def same_results(R, got, ref):
    """Statuses (exactly the planted set), results of the status-0 elements and the verifier's verdicts equal the reference call's."""
    status = ref.status.cpu().numpy()
    want = np.zeros(R.B, dtype=np.uint8)
    for i, code in R.planted.items():
        want[i] = code
    assert np.array_equal(status, want), status.nonzero()
    assert torch.equal(got.status, ref.status) and torch.equal(got.valid, ref.valid)
    ok = ref.status == 0
    assert torch.equal(got.out[ok], ref.out[ok])
    return status, ok


def kept_records(R, rows_region, rows_twin):
    """Per status-0 element and record: did the record keep 0xA5 in its constant planes?  Asserts assertion B's rule on the way: the
    constant-plane bytes of a record are 0xA5 throughout or the twin's throughout, never a mixture."""
    n = rows_region.shape[0]
    c = rows_region[:, R.cmask].view(n, R.T, -1)          # (the mask's bytes in ascending order: record by record)
    t = rows_twin[:, R.cmask].view(n, R.T, -1)
    kept, same = (c == 0xA5).all(dim=2), (c == t).all(dim=2)
    assert not bool((t == 0xA5).all(dim=2).any())          # (a complete record never looks like a kept one)
    assert bool((kept | same).all()), "a record with some of its constant planes written"
    return kept


def reference(R):
    """The plain twin: the route's call into a zero-filled plain buffer, with a caller workspace.  Made once per route and left unchanged."""
    plain0 = torch.zeros(R.B * R.ES, dtype=torch.uint8, device="cuda")
    (ref,) = R.run([plain0])
    status, ok = same_results(R, ref, ref)
    assert not R.audit(ref)[status == 0].any()
    return ref


def assert_a(R, region, ref, first=0, null_ws=False):
    """A: the call into `region` (as the arena made it) at element offset `first`."""
    target = region[first * R.ES:(first + R.B) * R.ES]
    (got,) = R.run([target], null_ws)
    status, ok = same_results(R, got, ref)
    assert torch.equal(R.rows(target)[ok], R.rows(ref.trace)[ok])
    good = np.flatnonzero(status == 0)
    for i in (int(good[0]), int(good[-1])):
        want = R.oracle(got, i)
        assert np.array_equal(R.flat(got, i), want) and np.array_equal(R.flat(ref, i), want), i
    assert not R.audit(got, ref.ws)[status == 0].any()
    return got


def twin_a5(R, ref, null_ws=False):
    """The same call into a 0xA5-filled plain buffer: complete records (the flag is clear), equal to the reference wherever the call writes."""
    plain_a5 = torch.full((R.B * R.ES,), 0xA5, dtype=torch.uint8, device="cuda")
    (s,) = R.run([plain_a5], null_ws)
    status, ok = same_results(R, s, ref)
    assert not R.audit(s, ref.ws)[status == 0].any()
    assert torch.equal(R.rows(plain_a5)[ok][:, R.cmask], R.rows(ref.trace)[ok][:, R.cmask])
    return s


def assert_b(R, arena, k, ref, tw, first=0, null_ws=False, all_kept=True, fill=True):
    """B: the call into kept region k, filled with 0xA5, at element offset `first`; `tw`: twin_a5()."""
    region = arena.regions[k]
    if fill:
        region.fill_(0xA5)
    target = region[first * R.ES:(first + R.B) * R.ES]
    (got,) = R.run([target], null_ws)
    check_b(R, arena, k, got, ref, tw, all_kept)
    return got


def check_b(R, arena, k, got, ref, tw, all_kept):
    status, ok = same_results(R, got, ref)
    rows_r, rows_t = R.rows(got.trace)[ok], R.rows(tw.trace)[ok]
    assert torch.equal(rows_r[:, ~R.cmask], rows_t[:, ~R.cmask])
    kept = kept_records(R, rows_r, rows_t)
    if all_kept:
        assert bool(kept.all()), "constant planes stored into an arena region: %d of %d records" % (int((~kept).sum()), kept.numel())
    bad = R.audit(got, ref.ws)[status == 0]
    assert np.array_equal(bad != 0, kept.any(dim=1).cpu().numpy())          # the audit flags exactly the elements that kept 0xA5
    arena.restore(k)
    torch.cuda.synchronize()
    assert torch.equal(R.rows(got.trace)[ok], rows_t)
    assert not R.audit(got, ref.ws)[status == 0].any()
    return kept


def assert_c_shifted(R, region, ref, tw, null_ws=False):
    """C: the same call 256 bytes into the 0xA5-filled region is not a set of whole record slots -- complete records."""
    region.fill_(0xA5)
    target = region[256:256 + R.B * R.ES]
    (got,) = R.run([target], null_ws)
    status, ok = same_results(R, got, ref)
    assert torch.equal(R.rows(target)[ok], R.rows(tw.trace)[ok])


def assert_c_other(R2, region):
    """C: a call of another geometry (route R2) into the 0xA5-filled region writes complete records, equal to its own 0xA5-filled plain twin."""
    ref2 = reference(R2)
    tw2 = twin_a5(R2, ref2)
    region.fill_(0xA5)
    target = region[:R2.B * R2.ES]
    (got,) = R2.run([target])
    status, ok = same_results(R2, got, ref2)
    assert torch.equal(R2.rows(target)[ok], R2.rows(tw2.trace)[ok])
    assert not R2.audit(got)[status == 0].any()


def drive(R, arena, first=0, null_ws=False, other=None):
    """A into region 0, B into region 1, C into region 1 (shifted, and `other`: a route of another geometry)."""
    ref = reference(R)
    assert_a(R, arena.regions[0], ref, first, null_ws)
    tw = twin_a5(R, ref, null_ws)
    assert_b(R, arena, 1, ref, tw, first, null_ws)
    assert_c_shifted(R, arena.regions[1], ref, tw, null_ws)
    if other is not None:
        assert_c_other(other, arena.regions[1])
    arena.restore(1)          # (the contract: whoever overwrote the planes restores them)
    return ref, tw


def planted_ends(H, B, in_field, both=True):
    code = H.H2R_E_NOT_IN_FIELD if in_field else H.H2R_E_NOT_REDUCED
    return {0: code, B - 1: code} if both else {0: code}


# ---- 1. the plain exports, one launch pair -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("null_ws", [False, True], ids=["workspace", "null_workspace"])
@pytest.mark.parametrize("export", ["pow", "modpow"])
@pytest.mark.parametrize("w,L,B", [(64, 32, 13), (32, 128, 3)])
def test_plain_exports_into_arena_regions(H, w, L, B, export, null_ws):
    chip = H.BigIntChip(w, w * L)
    planted = planted_ends(H, B, export == "modpow", both=B >= 5)
    X, N = _inputs(w, L, B, 100 * L + B, planted, export == "modpow")
    R = PowFixed(H, chip, export, E, X, N, planted)
    arena = H.TraceArena.for_pow(chip, E, B + OFF, regions=2, candidates=3)
    e3 = PowFixed(H, chip, export, 3, X, N, planted)          # another exponent's geometry
    assert (e3.ES, e3.T) != (R.ES, R.T)
    drive(R, arena, first=0, null_ws=null_ws, other=e3)
    arena.close()
    torch.cuda.synchronize()


# ---- 2. mul_mod / square_mod ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, OFF])
@pytest.mark.parametrize("square", [False, True], ids=["mul_mod", "square_mod"])
@pytest.mark.parametrize("w,L,B", [(64, 16, 21), (32, 128, 3)])
def test_mul_mod_into_arena_regions(H, w, L, B, square, first):
    chip = H.BigIntChip(w, w * L)
    planted = planted_ends(H, B, False, both=B >= 5)
    A, N = _inputs(w, L, B, 200 * L + B, planted, False)
    Bv, _ = _inputs(w, L, B, 201 * L + B, planted, False)
    R = MulMod(H, chip, A, None if square else Bv, N, planted)
    arena = H.TraceArena(chip, chip.layout.record_stride, 0, 1, B + OFF, regions=2, candidates=3)
    # C, another geometry: a fixed-exponent pow element (stride and records per element differ) of fewer bytes than the region
    pw = PowFixed(H, chip, "pow", 3, A[1:2], N[1:2], {})
    assert pw.B * pw.ES <= arena.regions[1].numel() and pw.ES != R.ES
    drive(R, arena, first=first, other=pw)
    arena.close()
    torch.cuda.synchronize()


# ---- 3. per-element exponents --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("export", ["pow", "modpow", "pipe"])
def test_var_exponent_into_arena_regions(H, export):
    from halo2_rsa_amd import _lib
    w, L, B, nl, bits = 64, 16, 9, 1, 6
    chip = H.BigIntChip(w, w * L)
    planted = planted_ends(H, B, export != "pow")
    X, N = _inputs(w, L, B, 300 + len(export), planted, export != "pow")
    rng = random.Random(31)
    EXP = [rng.randrange(1 << bits) for _ in range(B)]
    EXP[1], EXP[2] = (1 << bits) - 1, 0
    R = PowVar(H, chip, export, nl, bits, X, EXP, N, planted)
    pl = R.pl
    assert pl.num_mul_mods == 12 and pl.off_records == 0
    arena = H.TraceArena(chip, pl.elem_stride, pl.off_records, pl.num_mul_mods, B + OFF, regions=2, candidates=3)
    ref, tw = drive(R, arena)
    # the selected operands, the exponent bits and the result lie outside the records and are written as ever
    r1 = arena.regions[1]
    got = assert_b(R, arena, 1, ref, tw)
    ok = ref.status == 0
    lb = chip.num_limbs * chip.layout.limb_bytes
    for lo, n in ((pl.off_selected, pl.num_exp_bits * pl.selected_stride), (pl.off_e_bits, pl.num_exp_bits), (pl.off_result, lb)):
        assert lo + n <= pl.elem_stride and not bool(R.cmask[lo:lo + n].any())
        assert torch.equal(R.rows(got.trace)[ok][:, lo:lo + n], R.rows(tw.trace)[ok][:, lo:lo + n])
    # C: a fixed-exponent call into that region
    e3 = chip.pow_fixed_layout(3)
    assert (e3.elem_stride, e3.num_mul_mods) != (pl.elem_stride, pl.num_mul_mods) and B * e3.elem_stride <= r1.numel()
    Xf, Nf = _inputs(w, L, B, 301, {}, True)
    calls = Calls(H, chip, _lib.H2R_PIPE_AUTO, Xf, Nf)
    plain3 = torch.full((B * e3.elem_stride,), 0xA5, dtype=torch.uint8, device="cuda")
    r1.fill_(0xA5)
    s_r, s_p = calls.run(3, [r1[:B * e3.elem_stride], plain3])
    assert not s_p[2].any() and torch.equal(r1[:B * e3.elem_stride], plain3)
    assert not calls.audit(3, r1[:B * e3.elem_stride], s_r).cpu().numpy().any()
    arena.restore(1)
    calls.pipe.close()
    R.close()
    del r1, got, ref, tw
    arena.close()
    torch.cuda.synchronize()


# ---- 4. the verifier -----------------------------------------------------------------------------------------------------------------------
def _verifier_inputs(H, golden, B, seed):
    """Random signatures (verdict 0) with the three golden vectors (verdicts 1, 1, 0) at elements 1..3; x >= n at the first and last slot."""
    kats = golden["rsa_kats"]
    planted = planted_ends(H, B, True)
    SIG, N = _inputs(64, 32, B, seed, {}, True)
    rng = random.Random(seed + 1)
    HASHED = [rng.getrandbits(256) for _ in range(B)]
    for j, k in enumerate(kats):
        SIG[1 + j], N[1 + j], HASHED[1 + j] = int(k["sig"]), int(k["n"]), int(k["hashed"])
    for i in planted:
        SIG[i] = N[i] + 1
    return SIG, N, HASHED, planted


def _witness_regions_equal(R, a, b, status):
    """The in-field region of every element and the encoded-message region of every status-0 element (an element that is not in the
    field gets no pow / EM trace: include/h2r.h) equal the twin's."""
    vl = R.vl
    ok = torch.from_numpy(status == 0).cuda()
    assert torch.equal(R.rows(a)[:, vl.off_in_field:vl.off_em], R.rows(b)[:, vl.off_in_field:vl.off_em])
    assert torch.equal(R.rows(a)[ok][:, vl.off_em:], R.rows(b)[ok][:, vl.off_em:])
    assert not bool(R.cmask[vl.off_in_field:].any())


@pytest.mark.parametrize("form", ["batch", "side_stream"])
def test_verifier_into_arena_regions(H, golden, form):
    from halo2_rsa_amd import _lib
    B = 13
    chip = H.RSAChip(2048, 5).bigint_chip()
    SIG, N, HASHED, planted = _verifier_inputs(H, golden, B, 400)
    pipe = None
    if form == "side_stream":
        pipe = H.Pipeline(chip, depth=2, side_streams=1)
        assert pipe.info(B).record_form == _lib.H2R_PIPE_SIDE_STREAM
    R = Verify(H, chip, pipe, SIG, N, HASHED, planted)
    vl = R.vl
    arena = H.TraceArena(chip, vl.elem_stride, 0, vl.pow.num_mul_mods, B + OFF, regions=2, candidates=3)
    ref, tw = drive(R, arena)
    assert ref.valid.cpu().tolist()[1:4] == [1, 1, 0] and int(ref.valid.sum()) == 2
    got = assert_b(R, arena, 1, ref, tw)
    _witness_regions_equal(R, got.trace, tw.trace, ref.status.cpu().numpy())
    # C: a pow-layout call, whose stride differs, into the same region
    pl = chip.pow_fixed_layout(E)
    assert pl.elem_stride != vl.elem_stride and pl.num_mul_mods == vl.pow.num_mul_mods
    pw = PowFixed(H, chip, "modpow", E, SIG, N, planted)
    assert_c_other(pw, arena.regions[1])
    arena.restore(1)
    R.close()
    del got, ref, tw
    arena.close()
    torch.cuda.synchronize()


def test_verifier_step_launches_into_arena_regions(H, golden):
    """The verifier's step builds are compiled without the flag: the records a step launch writes come out complete whatever the target,
    and only the last call's records -- which go out through the flush and the generic record kernel -- may keep 0xA5.  Three calls back to
    back and a join: the first call's records (region 0) and the second's (plain) ride on step launches, the third's (region 1) are flushed."""
    from halo2_rsa_amd import _lib
    B = 515
    chip = H.RSAChip(2048, 5).bigint_chip()
    SIG, N, HASHED, planted = _verifier_inputs(H, golden, B, 401)
    pipe = H.Pipeline(chip, depth=3, side_streams=2, form=_lib.H2R_PIPE_ONE_LAUNCH_STEP)
    assert pipe.info(B).record_form == _lib.H2R_PIPE_ONE_LAUNCH_STEP
    R = Verify(H, chip, pipe, SIG, N, HASHED, planted)
    vl, n = R.vl, B * R.ES
    arena = H.TraceArena(chip, vl.elem_stride, 0, vl.pow.num_mul_mods, B + OFF, regions=2, candidates=3)
    r0, r1 = arena.regions
    # A: both regions as created
    plain0 = torch.zeros(n, dtype=torch.uint8, device="cuda")
    s0, ref, s1 = R.run([r0[:n], plain0, r1[:n]])
    status, ok = same_results(R, ref, ref)
    assert ref.valid.cpu().tolist()[1:4] == [1, 1, 0] and int(ref.valid.sum()) == 2
    good = np.flatnonzero(status == 0)
    for s in (s0, s1):
        same_results(R, s, ref)
        assert torch.equal(R.rows(s.trace)[ok], R.rows(plain0)[ok])
        assert not R.audit(s)[status == 0].any()
        for i in (int(good[0]), int(good[-1])):
            assert np.array_equal(R.flat(s, i), R.oracle(s, i)), i
    # B: both regions filled with 0xA5
    r0.fill_(0xA5)
    r1.fill_(0xA5)
    plain_a5 = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    s0, tw, s1 = R.run([r0[:n], plain_a5, r1[:n]])
    same_results(R, tw, ref)
    assert torch.equal(R.rows(plain_a5)[ok][:, R.cmask], R.rows(plain0)[ok][:, R.cmask]) and not R.audit(tw)[status == 0].any()
    kept0 = check_b(R, arena, 0, s0, ref, tw, all_kept=False)
    assert not bool(kept0.any()), "a step launch of the verifier left constant planes out"
    kept1 = check_b(R, arena, 1, s1, ref, tw, all_kept=False)
    assert bool(kept1.any()), "the flush stored the constant planes of every record of an arena region"
    for s in (s0, s1):
        _witness_regions_equal(R, s.trace, tw.trace, status)
    # C: a pow-layout call, whose stride differs, into the same region; and the verifier's own call 256 bytes into it
    assert_c_shifted(R, r1, ref, tw)
    pw = PowFixed(H, chip, "modpow", E, SIG[:13], N[:13], {0: H.H2R_E_NOT_IN_FIELD})
    assert pw.ES != R.ES
    assert_c_other(pw, r1)
    arena.restore(1)
    R.close()
    del r0, r1, s0, s1, ref, tw
    arena.close()
    torch.cuda.synchronize()


# ---- 5. the plain export's walk through sub-batches of elements ----------------------------------------------------------------------------
def test_sub_batch_walk_into_arena_regions(H):
    """h2r_pow_mod_fixed_exp_batch above the size at which a plain call is walked as sub-batches (overlapped_pow_fixed): the second sub-batch's
    trace pointer is the region's base advanced by a whole number of elements, and must match like the first."""
    w, L, e = 64, 24, 3
    chip = H.BigIntChip(w, w * L)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_out, sizes = ctypes.c_uint32(), (ctypes.c_uint64 * 16)()
    B = 6 * cus + 1
    for B in range(6 * cus + 1, 6 * cus + 258):          # the smallest walked batch, from the product's own plan
        _ck(H.lib().h2r_pipeline_call_plan(chip._ctx, B, 0, sizes, 16, ctypes.byref(n_out), None), "h2r_pipeline_call_plan")
        if n_out.value >= 2:
            break
    assert n_out.value >= 2 and sum(sizes[:n_out.value]) == B, (B, n_out.value)
    second = int(sizes[0])
    assert 0 < second < B - 1
    planted = planted_ends(H, B, False)
    X, N = _inputs(w, L, B, 500, planted, False)
    R = PowFixed(H, chip, "pow", e, X, N, planted)
    arena = H.TraceArena.for_pow(chip, e, B + 1, regions=2, candidates=3)
    ref = reference(R)
    assert_a(R, arena.regions[0], ref)
    tw = twin_a5(R, ref)
    got = assert_b(R, arena, 1, ref, tw)          # (every record of both sub-batches kept 0xA5, and is exact after the restore)
    arena.regions[1].fill_(0xA5)
    (got,) = R.run([arena.regions[1][:B * R.ES]])
    tail = R.rows(got.trace)[second:][ref.status[second:] == 0]
    assert bool((tail[:, R.cmask] == 0xA5).all()) and torch.equal(tail[:, ~R.cmask], R.rows(tw.trace)[second:][ref.status[second:] == 0][:, ~R.cmask])
    assert_c_shifted(R, arena.regions[1], ref, tw)
    arena.restore(1)
    del got, tail, ref, tw
    arena.close()
    torch.cuda.synchronize()


# ---- 6. the plain export's walk through segments of a long exponent ------------------------------------------------------------------------
def test_segment_walk_into_arena_regions(H):
    """A 512-bit exponent on a latency-bound batch through h2r_pow_mod_fixed_exp_batch: four segments, one chain and one record launch each
    (TraceArgs::t_lo / T_ops), every one of them on the region's slots."""
    w, L, B, nbits = 64, 32, 5, 512
    chip = H.BigIntChip(w, w * L)
    rng = random.Random(nbits + 1)
    e = rng.getrandbits(nbits) | (1 << (nbits - 1)) | 1
    eb = e.to_bytes(nbits // 8, "little")
    n_seg = ctypes.c_uint32()
    assert H.lib().h2r_exp_segment_plan(chip._ctx, B, eb, len(eb), 0, None, None, 0, ctypes.byref(n_seg)) == 0 and n_seg.value == 4
    planted = planted_ends(H, B, False)
    X, N = _inputs(w, L, B, 600, planted, False)
    R = PowFixed(H, chip, "pow", e, X, N, planted)
    arena = H.TraceArena.for_pow(chip, e, B + 1, regions=2, candidates=3)
    e2 = PowFixed(H, chip, "pow", E, X, N, planted)
    drive(R, arena, other=e2)
    arena.close()
    torch.cuda.synchronize()


# ---- 7. shared and keyed moduli ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("export", ["pow", "modpow"])
@pytest.mark.parametrize("moduli", ["shared", "keyed"])
def test_moduli_flags_into_arena_regions(H, moduli, export):
    from halo2_rsa_amd import _lib
    w, L, B = 64, 32, 13
    chip = H.BigIntChip(w, w * L)
    in_field = export == "modpow"
    code = H.H2R_E_NOT_IN_FIELD if in_field else H.H2R_E_NOT_REDUCED
    rng = random.Random(700)
    keys = [rng.getrandbits(w * L) | (1 << (w * L - 1)) | 1 for _ in range(3)]
    top = (1 << (w * L)) - 1
    if moduli == "shared":
        planted = {0: code, B - 1: code}
        per_elem = [keys[0]] * B
        n = [keys[0]]
    else:
        idx = [(5 * i + 1) % 3 for i in range(B)]
        idx[0] = 7                                        # out of range: H2R_E_SHAPE for that element
        planted = {0: H.H2R_E_SHAPE, B - 1: code}
        per_elem = [keys[k % 3] for k in idx]
        n = (keys, idx)
    X = [rng.randrange(m) for m in per_elem]
    for i in planted:
        X[i] = per_elem[i] + 1 if in_field else top
    R = PowFixed(H, chip, export, E, X, n, planted)
    assert R.flags == (_lib.H2R_F_SHARED_MODULUS if moduli == "shared" else _lib.H2R_F_KEYED_MODULI)
    arena = H.TraceArena.for_pow(chip, E, B + OFF, regions=2, candidates=3)
    drive(R, arena)          # (the audit goes through the expanded moduli, as BatchResult.audit does)
    arena.close()
    torch.cuda.synchronize()


# ---- 8. who matches ------------------------------------------------------------------------------------------------------------------------
def test_another_ctx_of_the_same_shape_matches(H):
    """The match is about (device, limb width, limbs) and the slots, not about the ctx the arena was created with: a second ctx of the same
    shape but another field and Montgomery representation of its advice matches, and its bytes are right."""
    w, L, B = 64, 32, 13
    chip = H.BigIntChip(w, w * L)
    other = H.BigIntChip(w, w * L, field="pasta_fq", montgomery=True)
    arena = H.TraceArena.for_pow(chip, E, B + OFF, regions=2, candidates=3)
    planted = planted_ends(H, B, True)
    X, N = _inputs(w, L, B, 800, planted, True)
    for export in ("modpow", "pipe"):
        R = PowFixed(H, other, export, E, X, N, planted)
        ref = reference(R)
        tw = twin_a5(R, ref)
        if export == "modpow":
            assert_a(R, arena.regions[0], ref)
        assert_b(R, arena, 1, ref, tw)
        assert_c_shifted(R, arena.regions[1], ref, tw)
        arena.restore(1)
        R.close()
    del ref, tw
    arena.close()
    torch.cuda.synchronize()


def test_a_ctx_of_another_shape_writes_complete_records(H):
    """A (64, 16) ctx given a pointer inside the (64, 32) arena's region -- the region's base and an element offset of its own stride."""
    B = 13
    chip32, chip16 = H.BigIntChip(64, 64 * 32), H.BigIntChip(64, 64 * 16)
    arena = H.TraceArena.for_pow(chip32, E, B + OFF, regions=2, candidates=3)
    planted = planted_ends(H, B, True)
    X, N = _inputs(64, 16, B, 801, planted, True)
    for export in ("modpow", "pipe"):
        R = PowFixed(H, chip16, export, E, X, N, planted)
        assert R.B * R.ES + chip32.pow_fixed_layout(E).elem_stride <= arena.regions[1].numel()
        assert_c_other(R, arena.regions[1])
        assert_c_other(R, arena.regions[1][chip32.pow_fixed_layout(E).elem_stride:])
        R.close()
    arena.restore(1)
    arena.close()
    torch.cuda.synchronize()


def test_closing_one_arena_leaves_the_other_matching(H):
    w, L, B = 64, 32, 13
    chip = H.BigIntChip(w, w * L)
    planted = planted_ends(H, B, False)
    X, N = _inputs(w, L, B, 802, planted, False)
    a1 = H.TraceArena.for_pow(chip, E, B + OFF, regions=2, candidates=3)
    a2 = H.TraceArena.for_pow(chip, 3, B + OFF, regions=2, candidates=3)
    R1, R2 = PowFixed(H, chip, "pow", E, X, N, planted), PowFixed(H, chip, "pow", 3, X, N, planted)
    ref1, ref2 = reference(R1), reference(R2)
    tw1, tw2 = twin_a5(R1, ref1), twin_a5(R2, ref2)
    assert_b(R2, a2, 1, ref2, tw2)                        # both alive: each call matches its own arena ...
    assert_b(R1, a1, 1, ref1, tw1)
    assert_c_other(R2, a1.regions[1])                     # ... and not the other's
    a1.restore(1)
    a2.close()
    assert_a(R1, a1.regions[0], ref1)
    assert_b(R1, a1, 1, ref1, tw1)                        # constant planes stay 0xA5, exact after the restore
    plain = torch.full((R2.B * R2.ES,), 0xA5, dtype=torch.uint8, device="cuda")
    (s,) = R2.run([plain])                                # the closed arena's geometry is gone with it
    assert torch.equal(R2.rows(plain)[ref2.status == 0], R2.rows(tw2.trace)[ref2.status == 0])
    del ref1, ref2, tw1, tw2, s
    a1.close()
    torch.cuda.synchronize()


# ---- 9. every slot, from creation, across a chunk seam -------------------------------------------------------------------------------------
def _allocation_granularity(H, device):
    """hipMemGetAllocationGranularity(recommended) for pinned device memory, as arena_build asks -- through the HIP runtime libh2r.so links."""
    class Loc(ctypes.Structure):
        _fields_ = [("type", ctypes.c_int), ("id", ctypes.c_int)]

    class Flags(ctypes.Structure):
        _fields_ = [("compressionType", ctypes.c_ubyte), ("gpuDirectRDMACapable", ctypes.c_ubyte), ("usage", ctypes.c_ushort)]

    class Prop(ctypes.Structure):
        _fields_ = [("type", ctypes.c_int), ("requestedHandleType", ctypes.c_int), ("location", Loc), ("win32HandleMetaData", ctypes.c_void_p),
                    ("allocFlags", Flags)]
    prop = Prop(1, 0, Loc(1, device), None, Flags(0, 0, 0))          # hipMemAllocationTypePinned, hipMemLocationTypeDevice
    gran = ctypes.c_size_t(0)
    fn = H.lib().hipMemGetAllocationGranularity
    fn.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(Prop), ctypes.c_int]
    assert fn(ctypes.byref(gran), ctypes.byref(prop), 1) == 0          # hipMemAllocationGranularityRecommended
    return gran.value or (2 << 20)


def test_every_slot_from_creation_across_a_chunk_seam(H):
    """arena_build stitches a region from physical chunks of at most 256 MB; this region is just over 256 MB, so two equal chunks.  The
    constant planes of EVERY slot of EVERY kept region are valid directly after creation (no call in between) and again after 0xA5 and
    restore(), and a call on the slots that straddle the seam passes A and B.  This pins the rewrite of the constant planes at creation, which
    everything rests on since the look's own all-planes launch was seen to lose most constants on 50 GB regions; it does not reproduce 50 GB."""
    w, L, B = 64, 32, 13
    chip = H.BigIntChip(w, w * L)
    pl = chip.pow_fixed_layout(E)
    ES = pl.elem_stride
    batch = (256 << 20) // ES + 1
    planted = planted_ends(H, B, True)
    X, N = _inputs(w, L, B, 900, planted, True)
    R = PowFixed(H, chip, "modpow", E, X, N, planted)
    ref = reference(R)
    good = int(np.flatnonzero(ref.status.cpu().numpy() == 0)[0])
    consts = R.rows(ref.trace)[good][R.cmask].clone()          # the constant-plane bytes of one element of a plain call
    assert bool((consts.view(R.T, -1) == consts.view(R.T, -1)[0]).all()) and bool(consts.any())          # (the same for every record)
    arena = H.TraceArena.for_pow(chip, E, batch, regions=2, candidates=3)
    region_bytes = arena.regions[0].numel()
    assert region_bytes == batch * ES and (256 << 20) < region_bytes <= (512 << 20)
    for r in arena.regions:                                    # directly after creation
        assert bool((r.view(batch, ES)[:, R.cmask] == consts).all())
    gran = _allocation_granularity(H, chip.device)
    seam = -(-((region_bytes + 1) // 2) // gran) * gran          # each chunk: half the region, rounded up to the granularity
    first = seam // ES - B // 2
    assert 0 < seam < region_bytes and first * ES < seam < (first + B) * ES - ES and first + B <= batch
    assert_a(R, arena.regions[0], ref, first)
    r1 = arena.regions[1]
    r1.fill_(0xA5)
    arena.restore(1)
    torch.cuda.synchronize()
    assert bool((r1.view(batch, ES)[:, R.cmask] == consts).all())
    assert bool((r1.view(batch, ES)[:, ~R.cmask] == 0xA5).all())
    tw = twin_a5(R, ref)
    ok = ref.status == 0
    (got,) = R.run([r1[first * ES:(first + B) * ES]])          # onto restored slots: exact at once
    assert torch.equal(R.rows(got.trace)[ok], R.rows(tw.trace)[ok]) and not R.audit(got)[ok.cpu().numpy()].any()
    assert_b(R, arena, 1, ref, tw, first)
    assert bool((r1.view(batch, ES)[:first][:, ~R.cmask] == 0xA5).all()) and bool((r1.view(batch, ES)[first + B:][:, ~R.cmask] == 0xA5).all())
    assert_c_shifted(R, r1, ref, tw)
    arena.restore(1)
    del r1, r, got, ref, tw
    arena.close()
    torch.cuda.synchronize()
