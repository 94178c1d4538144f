"""GPU: h2r_lookup_permuted_columns (A' / S') and h2r_lookup_product_columns (Z) on the case table of tests/lookup_cases.py -- challenges
theta chosen against lookup_setup_kernel's closed-form ranking (theta = 0, groups that wrap past p at their first, middle and last row or end
exactly at p - 1, groups that coincide over a stretch, groups that straddle 2^64 / 2^128 / 2^192, on all four moduli), hand-made
multiplicities (empty, every row once, no padding row, everything on the last row, sparse, colliding rows only), sizes next to every multiple
the kernels work in, and columns of 65 and 129 tiles for the carry kernel's lane partition.  test_lookup_cases_model.py (CPU) proves the table
is what it says and that the model's Z ends at 1 everywhere.

One permuted_columns call and one product_columns call per group; its circuits are the batch elements.  The input column A is the model's,
uploaded.  Every comparison is byte for byte against the plain model; outputs start as a sentinel and carry 64 guard bytes behind them."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import lookup_cases as LC

SENTINEL = 0xAB
GUARD = 64


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import halo2_rsa_amd as H_
    return H_


_chips, _args = {}, {}


def lookup_argument(H, name, field, montgomery=False):
    if (field, montgomery) not in _chips:
        _chips[field, montgomery] = H.BigIntChip(64, 2048, field=field, montgomery=montgomery)
    if (name, field, montgomery) not in _args:
        chip = _chips[field, montgomery]
        lens, tags = LC.CONFIGS[name]
        la = H.LookupArgument(chip, rsa_chip=True) if name == "rsa" else H.LookupArgument(chip, bit_lens=lens, tags=tags)
        if not montgomery:   # (table_image reports small integers)
            assert la.table_image() == LC.lookup_config(name).table()
        _args[name, field, montgomery] = la
    return _args[name, field, montgomery]


def guarded(shape):
    """(whole allocation, the tensor of `shape` at its start): sentinel-filled, GUARD bytes behind the tensor"""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    return buf, buf[:n].view(shape)


def hist_tensor(hists):
    """[circuit][5][n_rows] counts (any value below 2^32) -> the device's uint32 histogram"""
    return torch.from_numpy(np.array(hists, dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()


def in_repr(vals, P, montgomery):
    return [v * LC.R256 % P for v in vals] if montgomery else list(vals)


class Run:
    """The device's A', S', Z and both status vectors of a batch of circuits."""

    def __init__(self, la, cfg, P, circuits, models, usable, montgomery=False, arg_mask=31, hists=None, betas=None, product=True):
        B = len(circuits)
        self.B, self.usable, self.P, self.montgomery = B, usable, P, montgomery
        th = in_repr([c.theta for c in circuits], P, montgomery)
        be = in_repr([c.beta for c in circuits] if betas is None else betas, P, montgomery)
        ga = in_repr([c.gamma for c in circuits], P, montgomery)
        hist = hist_tensor([c.hists for c in circuits] if hists is None else hists)
        assert hist.shape == (B, 5, cfg.n_rows)
        self.bufs = [guarded((B, 5, usable, 32)), guarded((B, 5, usable, 32)), guarded((B, 5, usable + 1, 32))]
        (_, self.a_perm), (_, self.s_perm), (_, self.z) = self.bufs
        _, _, st = la.permuted_columns(hist, th, usable, arg_mask=arg_mask, out=(self.a_perm, self.s_perm))
        torch.cuda.synchronize()
        self.status = st.cpu().tolist()
        self.z_status = None
        if product:
            a_host = b"".join(LC.to_bytes(m["A"][k], P, montgomery) for m in models for k in range(5))
            a_in = torch.frombuffer(bytearray(a_host), dtype=torch.uint8).view(B, 5, usable, 32).cuda()
            zst = torch.zeros(B, dtype=torch.uint8, device="cuda")
            la.product_columns(a_in, self.a_perm, self.s_perm, th, be, ga, usable, arg_mask=arg_mask, out=(self.z, zst))
            torch.cuda.synchronize()
            self.z_status = zst.cpu().tolist()
        self.host = [t.cpu().numpy() for _, t in self.bufs]
        for name, (buf, t) in zip(("A'", "S'", "Z"), self.bufs):
            assert bool((buf[t.numel():] == SENTINEL).all()), "%s: the bytes behind the tensor were written" % name

    def column(self, which, b, k):
        return self.host[which][b, k].tobytes()

    def assert_model(self, b, k, m, what=("A'", "S'", "Z"), tag=""):
        for which, name, key in ((0, "A'", "Ap"), (1, "S'", "Sp"), (2, "Z", "Z")):
            if name not in what:
                continue
            got, want = self.column(which, b, k), LC.to_bytes(m[key][k], self.P, self.montgomery)
            if got != want:
                rows = [i for i in range(len(want) // 32) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]]
                raise AssertionError("%s %s argument %d: %d rows differ, first %s" % (tag, name, k, len(rows), rows[:4]))

    def assert_untouched(self, which, b, k):
        col = self.host[which][b, k]
        assert bool((col == SENTINEL).all()), (("A'", "S'", "Z")[which], b, k)


def run_group(H, g, montgomery=False, arg_mask=31):
    la = lookup_argument(H, g.config, g.field, montgomery)
    assert la.n_rows == g.cfg.n_rows
    models = g.model()
    r = Run(la, g.cfg, g.P, g.circuits, models, g.usable, montgomery=montgomery, arg_mask=arg_mask)
    assert r.status == [0] * r.B and r.z_status == [0] * r.B
    assert r.z.shape == (r.B, 5, g.usable + 1, 32)
    for b, (c, m) in enumerate(zip(g.circuits, models)):
        for k in range(5):
            if (arg_mask >> k) & 1:
                r.assert_model(b, k, m, tag="%s [%s]" % (c.key, c.shapes[k]))
            else:
                for which in range(3):
                    r.assert_untouched(which, b, k)


# ---- 1. parity: every group of the table -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid", [g.id for g in LC.GROUPS])
def test_group_against_the_plain_model(H, gid):
    run_group(H, LC.BY_ID[gid])


@pytest.mark.parametrize("gid", LC.MONTGOMERY_GROUPS)
def test_group_in_a_montgomery_ctx(H, gid):
    """theta, beta, gamma and A go in, A' / S' / Z come out as the canonical model * 2^256 mod p"""
    run_group(H, LC.BY_ID[gid], montgomery=True)


def test_arg_mask_leaves_the_other_arguments_alone(H):
    run_group(H, LC.BY_ID[LC.ARG_MASK_GROUP], arg_mask=0b10010)


# ---- 2. red cases: circuit 1 of three is damaged, the others stay byte-equal to the model ------------------------------------------------
RED_CONFIG, RED_FIELD, RED_USABLE = "rsa", "bn254_fr", 512
RED_SHAPES = ("empty", "once", "sparse", "collide", "sparse")   # circuit 1: every argument keeps padding rows, so every A' starts with the value 0


@pytest.fixture(scope="module")
def red():
    cfg, P = LC.lookup_config(RED_CONFIG), LC.FIELDS[RED_FIELD]
    chals = {lab: (lab, th, fam) for lab, th, fam in LC.challenges(RED_CONFIG, RED_FIELD)}
    big = len(LC.groups_of(cfg)) - 1
    picks = [chals["random"], chals["wrap(%d,%d)" % (big, LC.groups_of(cfg)[big][1] // 2)], chals["zero"]]
    circuits = [LC.Circuit("red/%s/%d" % (lab, i), RED_CONFIG, RED_FIELD, RED_USABLE, lab, th, fam, RED_SHAPES if i == 1 else LC.SHAPES_FIRST)
                for i, (lab, th, fam) in enumerate(picks)]
    models = [LC.circuit_model(cfg, P, c, RED_USABLE) for c in circuits]
    assert all(m["zero_den"] == [None] * 5 for m in models)
    return cfg, P, circuits, models


def _others_green(r, models, what=("A'", "S'", "Z")):
    for b in (0, 2):
        for k in range(5):
            r.assert_model(b, k, models[b], what=what, tag="circuit %d" % b)


def _damaged(circuits, k, counts):
    """the three circuits' histograms with circuit 1's argument k replaced by {row: count}"""
    hists = [[list(h) for h in c.hists] for c in circuits]
    hists[1][k] = [0] * len(hists[1][k])
    for r, m in counts.items():
        hists[1][k][r] = m
    return hists


def test_red_undamaged_batch(H, red):
    cfg, P, circuits, models = red
    r = Run(lookup_argument(H, RED_CONFIG, RED_FIELD), cfg, P, circuits, models, RED_USABLE)
    assert r.status == [0, 0, 0] and r.z_status == [0, 0, 0]
    for b in range(3):
        for k in range(5):
            r.assert_model(b, k, models[b], tag="circuit %d" % b)


@pytest.mark.parametrize("name,arg,counts", [
    ("one input too many", 2, {0: 1, 5: RED_USABLE - 2, 338: 2}),            # usable_rows + 1
    ("two counts of 2^31", 2, {7: 1 << 31, 300: 1 << 31}),                   # the 32-bit sum is 0
    ("2^32 - 1 next to 2", 0, {17: (1 << 32) - 1, 18: 2}),                   # the 32-bit sum is 1
    ("2^32 - 1 and 1 in one thread's rows", 4, {3: (1 << 32) - 1, 259: 1}),  # rows r and r + 256 are added by the same thread
])
def test_red_counts_that_do_not_fit(H, red, name, arg, counts):
    """H2R_E_SHAPE and the circuit's columns untouched; the counts are 32-bit words of the CALLER's, so a sum that wraps must not pass as small"""
    cfg, P, circuits, models = red
    assert sum(counts.values()) > RED_USABLE and all(r < cfg.n_rows and m < (1 << 32) for r, m in counts.items())
    r = Run(lookup_argument(H, RED_CONFIG, RED_FIELD), cfg, P, circuits, models, RED_USABLE, hists=_damaged(circuits, arg, counts), product=False)
    print(name, "status", r.status)
    assert r.status == [0, H.H2R_E_SHAPE, 0]
    for k in range(5):
        r.assert_untouched(0, 1, k)
        r.assert_untouched(1, 1, k)
    _others_green(r, models, what=("A'", "S'"))


def test_red_beta_zero_on_a_wrapping_challenge(H, red):
    """the sorted A' starts with the value 0 in every argument: with beta = 0 a denominator is zero -- H2R_E_ASSERTION, no Z of that circuit"""
    from halo2_rsa_amd import _lib
    cfg, P, circuits, models = red
    assert circuits[1].family[0] == "wrap" and all(models[1]["Ap"][k][0] == 0 for k in range(5))
    bad = LC.circuit_model(cfg, P, circuits[1], RED_USABLE, beta=0)
    assert bad["zero_den"] == [0] * 5                                        # the model: the first row's denominator vanishes
    r = Run(lookup_argument(H, RED_CONFIG, RED_FIELD), cfg, P, circuits, models, RED_USABLE, betas=[circuits[0].beta, 0, circuits[2].beta])
    assert r.status == [0, 0, 0] and r.z_status == [0, _lib.H2R_E_ASSERTION, 0]
    for k in range(5):
        r.assert_untouched(2, 1, k)
        r.assert_model(1, k, models[1], what=("A'", "S'"), tag="circuit 1")  # (A' / S' do not depend on beta)
    _others_green(r, models)
