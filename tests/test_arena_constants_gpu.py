"""A trace arena's regions keep the constant planes of their record slots (include/h2r.h, trace arena): a record launch whose
records all lie on such slots does not store ACCX_LO/HI, QACC, MODACC, NQ2_LO/HI and AMNQ2 again; every other launch writes whole
records.  Byte-exact throughout: the same pipelined modpow_public_key call into an arena region and into plain buffers, the oracle's
stream, the in-place audit, and 0xA5-filled targets that show which bytes a launch wrote."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle_lib import Oracle  # noqa: E402

CONST_PLANES = ("ACCX_LO", "ACCX_HI", "QACC", "MODACC", "NQ2_LO", "NQ2_HI", "AMNQ2")
E = 65537


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    import halo2_rsa_amd
    return halo2_rsa_amd


def const_plane_mask(chip, pl):
    """Which bytes of an element of layout `pl` are constant planes of one of its records."""
    from halo2_rsa_amd import _lib
    lo = chip.layout
    m = np.zeros(pl.elem_stride, dtype=bool)
    for t in range(pl.num_mul_mods):
        for name in CONST_PLANES:
            p = _lib.PLANES.index(name)
            start = pl.off_records + t * lo.record_stride + lo.plane_off[p]
            m[start:start + lo.plane_elem[p] * 2 * lo.num_limbs] = True     # (2L entries: the kernels write the reserved last one as zero)
    return torch.from_numpy(m).cuda()


class Calls:
    """Pipelined modpow_public_key calls of one set of inputs into the trace buffers the test names."""

    def __init__(self, H, chip, form, X, N):
        self.H, self.chip, self.B = H, chip, len(X)
        self.x, self.n = chip.assign_integer(X), chip.assign_integer(N)
        self.pipe = H.Pipeline(chip, depth=3, side_streams=2, form=form)

    def run(self, e, targets):
        """One call per target, back to back, then the join.  Returns [(ws, out, status)] per call."""
        chip, B = self.chip, self.B
        pl = chip.pow_fixed_layout(e)
        assert len(targets) <= 3
        sets = []
        for tb in targets:
            ws = torch.zeros(chip.workspace_bytes(B, pl.num_mul_mods), dtype=torch.uint8, device="cuda")
            out = torch.zeros((B, chip.num_limbs), dtype=chip.torch_dtype, device="cuda")
            status = torch.zeros(B, dtype=torch.uint8, device="cuda")
            self.pipe.modpow_public_key(self.x, e, self.n, tb, ws, out, status)
            sets.append((ws, out, status))
        self.pipe.join()
        torch.cuda.synchronize()
        return sets

    def audit(self, e, tb, s):
        from halo2_rsa_amd import big_integer as BI
        H, chip = self.H, self.chip
        ws, out, status = s
        tr = H.Trace(chip, tb, self.B, chip.pow_fixed_layout(e))
        eb = e.to_bytes((e.bit_length() + 7) // 8, "little")
        res = BI.BatchResult(H.AssignedInteger(out, chip.limb_width), tr, status, workspace=ws, inputs=("pow_fixed", self.x, None, self.n, eb))
        bad, first = res.audit()
        torch.cuda.synchronize()
        return bad


# (w, L, batch, form): ragged against the record kernel's items per workgroup; the last one is issued as step launches
CASES = [(64, 32, 13, "two_queue"), (64, 16, 21, "two_queue"), (64, 48, 7, "two_queue"), (32, 128, 3, "two_queue"),
         (64, 32, 13, "step"), (64, 16, 21, "step"), (64, 48, 7, "step"), (32, 128, 3, "step"), (64, 32, 515, "step")]


@pytest.mark.parametrize("w,L,B,form", CASES)
def test_arena_regions_keep_their_constant_planes(H, w, L, B, form):
    from halo2_rsa_amd import _lib
    chip = H.BigIntChip(w, w * L)
    o = Oracle(w, L)
    pl = chip.pow_fixed_layout(E)
    ES = pl.elem_stride
    OFF = 5                                             # the arena holds OFF more elements than a call: calls at element offset OFF fit
    rng = random.Random(1000 * L + B)
    N = [rng.getrandbits(w * L) | (1 << (w * L - 1)) | 1 for _ in range(B)]
    X = [rng.randrange(n) for n in N]
    big = B // 2
    X[big] = N[big] + 1 if N[big] + 1 < (1 << (w * L)) else N[big]      # one element with x >= n: status NOT_IN_FIELD, no records
    arena = H.TraceArena.for_pow(chip, E, B + OFF, regions=2, candidates=3)
    calls = Calls(H, chip, _lib.H2R_PIPE_TWO_QUEUE if form == "two_queue" else _lib.H2R_PIPE_ONE_LAUNCH_STEP, X, N)
    r0, r1 = arena.regions
    cmask = const_plane_mask(chip, pl)
    assert int(cmask.sum()) == pl.num_mul_mods * 2 * L * sum(chip.layout.plane_elem[_lib.PLANES.index(p)] for p in CONST_PLANES)

    def rows(buf, first=0):
        return buf[first * ES:(first + B) * ES].view(B, ES)

    # 1. the same call into an arena region and into a zero-filled plain buffer (the region's records go out first: with step
    #    launches they are the record role's, the plain buffer's the flush's)
    plain0 = torch.zeros(B * ES, dtype=torch.uint8, device="cuda")
    s_r0, s_p0 = calls.run(E, [r0[:B * ES], plain0])
    status = s_p0[2].cpu().numpy()
    assert torch.equal(s_r0[2], s_p0[2]) and torch.equal(s_r0[1], s_p0[1])
    assert status[big] == H.H2R_E_NOT_IN_FIELD and not np.delete(status, big).any()
    ok = s_p0[2] == 0
    assert torch.equal(rows(r0)[ok], rows(plain0)[ok])
    tr = H.Trace(chip, r0[:B * ES], B, pl)
    for i in (0, B - 1):
        rc, oo, ost = o.pow_mod_fixed_exp(o.limbs(X[i]), o.limbs(N[i]), E)
        assert rc == 0 and np.array_equal(ost, tr.flatten(i)), i
    assert not calls.audit(E, r0[:B * ES], s_r0).cpu().numpy()[status == 0].any()
    got = H.AssignedInteger(s_r0[1], w).to_big_uint()
    assert all(got[i] == pow(X[i], E, N[i]) for i in range(B) if i != big)

    # 2. 0xA5-filled targets: a plain buffer comes out complete (the flag is clear); a region keeps 0xA5 in its constant planes --
    #    that is how we know the stores are gone -- and is exact everywhere else
    plain_a5 = torch.full((B * ES,), 0xA5, dtype=torch.uint8, device="cuda")
    r1.fill_(0xA5)
    s_pa, s_r1 = calls.run(E, [plain_a5, r1[:B * ES]])
    assert not calls.audit(E, plain_a5, s_pa).cpu().numpy()[status == 0].any()
    assert torch.equal(rows(plain_a5)[ok][:, cmask], rows(plain0)[ok][:, cmask])
    got_r1 = rows(r1)[ok]
    assert bool((got_r1[:, cmask] == 0xA5).all())
    assert torch.equal(got_r1[:, ~cmask], rows(plain_a5)[ok][:, ~cmask])
    assert calls.audit(E, r1[:B * ES], s_r1).cpu().numpy()[status == 0].all()
    arena.restore(1)
    torch.cuda.synchronize()
    assert torch.equal(rows(r1)[ok], rows(plain_a5)[ok])
    assert bool((r1[B * ES:].view(OFF, ES)[:, ~cmask] == 0xA5).all())          # the restore touched constant planes only
    assert not calls.audit(E, r1[:B * ES], s_r1).cpu().numpy()[status == 0].any()

    # 3. a call at element offset OFF of a region matches (its constant planes stay 0xA5) and is exact after the restore
    r1.fill_(0xA5)
    (s_off,) = calls.run(E, [r1[OFF * ES:(OFF + B) * ES]])
    got_off = rows(r1, OFF)[ok]
    assert bool((got_off[:, cmask] == 0xA5).all())
    arena.restore(1)
    torch.cuda.synchronize()
    assert torch.equal(rows(r1, OFF)[ok], rows(plain_a5)[ok])
    assert not calls.audit(E, r1[OFF * ES:(OFF + B) * ES], s_off).cpu().numpy()[status == 0].any()

    # 4. a pointer that is not a whole number of elements into the region, and another exponent's geometry: complete records
    r1.fill_(0xA5)
    (s_sh,) = calls.run(E, [r1[256:256 + B * ES]])
    assert torch.equal(r1[256:256 + B * ES].view(B, ES)[ok], rows(plain_a5)[ok])
    e3 = 3
    pl3 = chip.pow_fixed_layout(e3)
    ES3 = pl3.elem_stride
    assert (ES3, pl3.num_mul_mods) != (ES, pl.num_mul_mods)
    r1.fill_(0xA5)
    plain3 = torch.full((B * ES3,), 0xA5, dtype=torch.uint8, device="cuda")
    s_r3, s_p3 = calls.run(e3, [r1[:B * ES3], plain3])
    assert torch.equal(r1[:B * ES3].view(B, ES3)[ok], plain3.view(B, ES3)[ok])
    assert not calls.audit(e3, r1[:B * ES3], s_r3).cpu().numpy()[status == 0].any()
    arena.restore(1)                                                           # (the contract: whoever overwrote the planes restores them)

    # the exports' own checks
    L_ = H.lib()
    assert L_.h2r_arena_restore_constants(arena._a, 2, None) == H.H2R_E_SHAPE
    assert L_.h2r_arena_restore_constants(None, 0, None) == _lib.H2R_E_NULL
    img = H.TraceArena.for_images(chip, 1 << 20, regions=1, candidates=1)
    assert L_.h2r_arena_restore_constants(img._a, 0, None) == _lib.H2R_E_UNSUPPORTED
    img.close()
    torch.cuda.synchronize()
    calls.pipe.close()
    del r0, r1, tr
    arena.close()

    # 5. the arena is gone: its addresses are plain memory again (a new allocation may reuse them) -- complete records
    plain_z = torch.full((B * ES,), 0xA5, dtype=torch.uint8, device="cuda")
    calls2 = Calls(H, chip, _lib.H2R_PIPE_AUTO, X, N)
    (s_z,) = calls2.run(E, [plain_z])
    assert torch.equal(plain_z.view(B, ES)[ok], rows(plain_a5)[ok])
    calls2.pipe.close()


# A long exponent: 512 bits and more on a latency-bound batch are walked as SEGMENTS of the exponent's bits (one chain and one record
# launch per segment, TraceArgs::t_lo / T_ops), 500 bits as one launch pair -- some 750 records per element either way.
@pytest.mark.parametrize("nbits,segments", [(512, 4), (500, 1)])
def test_long_exponent_into_arena_regions(H, nbits, segments):
    import ctypes
    from halo2_rsa_amd import _lib
    w, L, B = 64, 32, 5
    chip = H.BigIntChip(w, w * L)
    rng = random.Random(nbits)
    e = rng.getrandbits(nbits) | (1 << (nbits - 1)) | 1
    eb = e.to_bytes((nbits + 7) // 8, "little")
    n_seg = ctypes.c_uint32()
    assert H.lib().h2r_exp_segment_plan(chip._ctx, B, eb, len(eb), 0, None, None, 0, ctypes.byref(n_seg)) == 0 and n_seg.value == segments
    pl = chip.pow_fixed_layout(e)
    ES = pl.elem_stride
    N = [rng.getrandbits(w * L) | (1 << (w * L - 1)) | 1 for _ in range(B)]
    X = [rng.randrange(n) for n in N]
    X[2] = N[2]                                                         # x >= n: no records for this element
    arena = H.TraceArena.for_pow(chip, e, B, regions=2, candidates=3)
    calls = Calls(H, chip, _lib.H2R_PIPE_AUTO, X, N)
    r0, r1 = arena.regions
    cmask = const_plane_mask(chip, pl)
    plain0 = torch.zeros(B * ES, dtype=torch.uint8, device="cuda")
    plain_a5 = torch.full((B * ES,), 0xA5, dtype=torch.uint8, device="cuda")
    s_r0, s_p0 = calls.run(e, [r0, plain0])
    status = s_p0[2].cpu().numpy()
    assert status.tolist() == [0, 0, H.H2R_E_NOT_IN_FIELD, 0, 0]
    ok = s_p0[2] == 0
    assert torch.equal(r0.view(B, ES)[ok], plain0.view(B, ES)[ok])
    assert not calls.audit(e, r0, s_r0).cpu().numpy()[status == 0].any()
    got = H.AssignedInteger(s_r0[1], w).to_big_uint()
    assert all(got[i] == pow(X[i], e, N[i]) for i in range(B) if i != 2)
    r1.fill_(0xA5)
    s_pa, s_r1 = calls.run(e, [plain_a5, r1])
    assert not calls.audit(e, plain_a5, s_pa).cpu().numpy()[status == 0].any()
    got_r1 = r1.view(B, ES)[ok]
    assert bool((got_r1[:, cmask] == 0xA5).all())                       # every launch of the call carried the flag
    assert torch.equal(got_r1[:, ~cmask], plain_a5.view(B, ES)[ok][:, ~cmask])
    arena.restore(1)
    torch.cuda.synchronize()
    assert torch.equal(r1.view(B, ES)[ok], plain_a5.view(B, ES)[ok])
    assert not calls.audit(e, r1, s_r1).cpu().numpy()[status == 0].any()
    calls.pipe.close()
    del r0, r1
    arena.close()
