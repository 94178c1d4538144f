"""CPU: the case table of tests/lookup_cases.py is what it claims to be, so that test_lookup_adversarial.py cannot pass vacuously -- every wrap
challenge really wraps its group at the stated row, every overlap has the stated number of equal rows, every word challenge has rows on both
sides of 2^(64 k); every histogram has its shape; and for EVERY circuit of every group the plain model's Z ends at 1 with no zero denominator.
No case is filtered or skipped at run time: a seeded beta / gamma that hits a zero denominator fails here and gets another seed."""
import pytest

import advice_ref as AR
import lookup_cases as LC

PINNED_GROUPS = 87
PINNED_CIRCUITS = 1077


def test_the_case_table_has_its_pinned_length():
    assert LC.N_GROUPS == PINNED_GROUPS and LC.N_CIRCUITS == PINNED_CIRCUITS
    assert len(LC.BY_ID) == LC.N_GROUPS                                     # (no two groups share an id)
    keys = [c.key for g in LC.GROUPS for c in g.circuits]
    assert len(set(keys)) == len(keys)
    kinds = {}
    for g in LC.GROUPS:
        kinds[g.kind] = kinds.get(g.kind, 0) + 1
    assert kinds == {"challenges": 32, "sizes": 52, "tiles": 3}
    assert all(i in LC.BY_ID for i in LC.MONTGOMERY_GROUPS + [LC.ARG_MASK_GROUP])
    for name in LC.CONFIGS:                                                  # one gamma = P - 1 and one beta = P - 1 circuit per config
        pins = sorted(getattr(c, "pinned", "") for g in LC.GROUPS if g.config == name for c in g.circuits if hasattr(c, "pinned"))
        assert pins == ["beta", "gamma"], name
    for g in LC.GROUPS:
        for c in g.circuits:
            if getattr(c, "pinned", None) == "gamma":
                assert c.gamma == g.P - 1
            if getattr(c, "pinned", None) == "beta":
                assert c.beta == g.P - 1


def test_configurations_and_sizes():
    rows = {name: LC.lookup_config(name).n_rows for name in LC.CONFIGS}
    assert rows == {"rsa": 339, "max": 1021, "tiny": 7, "bigtag": 265}
    assert LC.lookup_config("rsa").bit_lens == [1, 4, 6, 8] and LC.lookup_config("rsa").tags == [1, 2, 3, 4]
    assert LC.lookup_config("max").bit_lens == list(range(2, 10)) and len(LC.lookup_config("max").bit_lens) == 8
    assert LC.lookup_config("bigtag").tags == [0xFFFFFFFF, 0x80000001]
    for name, (lo, ragged) in LC.FULL_SIZES.items():
        assert lo == rows[name] and ragged % 64 and lo in LC.SIZE_LIST[name] and ragged in LC.SIZE_LIST[name]
    T = LC.TILE
    tiles = [(u + T - 1) // T for u, _ in LC.Z_SIZES]
    assert tiles == [65, 129, 64] and [(t + 63) // 64 for t in tiles] == [2, 3, 1]
    assert LC.Z_SIZES[0][0] % T == 1                                         # the last tile holds one row
    assert [-(-t // -(-t // 64)) for t in tiles] == [33, 43, 64]               # lanes of the carry kernel that hold a tile
    assert [63 * ((t + 63) // 64) < t for t in tiles] == [False, False, True]      # lane 63 holds a tile
    assert LC.Z_SIZES[2][0] % T == 0
    assert LC.Z_SIZES[1][0] == 131077                                        # the largest column


@pytest.mark.parametrize("field", list(LC.FIELDS))
@pytest.mark.parametrize("name", list(LC.CONFIGS))
def test_challenges_are_what_their_labels_say(name, field):
    cfg, P = LC.lookup_config(name), LC.FIELDS[field]
    gs = LC.groups_of(cfg)
    chals = LC.challenges(name, field)
    fams = [f[0] for _, _, f in chals]
    assert fams.count("zero") == 1 and fams.count("word") == 3 and fams.count("overlap") in (2, 3) and fams.count("wrap") >= 8
    assert fams[-3:] == ["one", "pm1", "random"]
    assert all(0 <= th < P for _, th, _ in chals)
    for label, theta, fam in chals:
        table = AR.compress(cfg.table(), theta, P)
        if fam[0] == "zero":
            assert theta == 0 and len(set(table)) == max(S for _, S, _ in gs)          # exactly max S_j distinct table values
        elif fam[0] == "wrap":
            j, c = fam[1], fam[2]
            v, S = LC.group_values(cfg, j, theta, P), gs[j][1]
            assert v[0] == P - c, label
            assert v == table[gs[j][2]:gs[j][2] + S]
            if c < S:                                                                     # crosses P behind row c - 1: row c is 0
                assert v[c - 1] == P - 1 and v[c] == 0 and v[S - 1] == S - 1 - c, label
            elif c == S:                                                                  # ends exactly at P - 1
                assert v[S - 1] == P - 1 and 0 not in v, label
            else:
                assert c == S + 1 and v[S - 1] == P - 2 and 0 not in v, label
        elif fam[0] == "overlap":
            i, j, d = fam[1], fam[2], fam[3]
            vi, vj = LC.group_values(cfg, i, theta, P), LC.group_values(cfg, j, theta, P)
            assert vi[0] == (vj[0] + d) % P, label
            want = max(0, min(d + gs[i][1], gs[j][1]) - d)                               # |[d, d + S_i) & [0, S_j)|
            assert len(set(vi) & set(vj)) == want, label
            assert want == {1: gs[i][1], gs[j][1] - 1: 1, gs[j][1]: 0}[d]
        elif fam[0] == "word":
            j, k = fam[1], fam[2]
            v = LC.group_values(cfg, j, theta, P)
            assert v[0] == (1 << (64 * k)) - 3 and v[2] == (1 << (64 * k)) - 1 and v[3] == 1 << (64 * k), label
            assert any(x < (1 << (64 * k)) for x in v) and any(x >= (1 << (64 * k)) for x in v)
    wraps = [f for _, _, f in chals if f[0] == "wrap"]
    for j in (len(gs) - 1, 0):                                                           # the largest and the smallest group: all five positions
        S = gs[j][1]
        assert sorted(set(c for _, jj, c in wraps if jj == j)) == sorted(set([1, S // 2, S - 1, S, S + 1]))


def _check_hist(g, c, k):
    h, shape, n, u = c.hists[k], c.shapes[k], g.cfg.n_rows, g.usable
    assert len(h) == n and all(m >= 0 for m in h) and sum(h) <= u
    if shape == "empty":
        assert sum(h) == 0
    elif shape == "once":
        assert h == [1] * n
    elif shape == "full":
        assert sum(h) == u and h[0] == 0
    elif shape == "last":
        assert h[n - 1] == u and sum(h) == u
    elif shape == "collide":
        rows = set(LC.colliding_rows(g.cfg, c.theta, g.P))
        assert sum(h) > 0 and all(r in rows for r, m in enumerate(h) if m)
    else:
        assert shape == "sparse" and 0 < sum(h) < u
    if c.asked[k] != shape:                                                              # the one fall-back: no two rows collide under this theta
        assert (c.asked[k], shape) == ("collide", "sparse") and not LC.colliding_rows(g.cfg, c.theta, g.P)


@pytest.mark.parametrize("gid", [g.id for g in LC.GROUPS])
def test_model_of_every_circuit(gid):
    g = LC.BY_ID[gid]
    P, u = g.P, g.usable
    assert g.cfg.n_rows <= u
    labels = [c.label for c in g.circuits]
    if g.kind == "challenges":
        assert g.second == (u == g.cfg.n_rows)
        assert labels == [lab for lab, _, _ in LC.challenges(g.config, g.field) for _ in range(2 if g.second else 1)]
        assert sorted(set(s for c in g.circuits for s in c.asked)) == sorted(LC.SHAPES if g.second else LC.SHAPES_FIRST)
    else:
        assert [lab.split("(")[0] for lab in labels] == ["zero", "wrap", "random"]
        assert sorted(set(s for c in g.circuits for s in c.asked)) == sorted(LC.SHAPES_FIRST)
    models = g.model()
    assert len(models) == len(g.circuits)
    for c, m in zip(g.circuits, models):
        assert 0 <= c.theta < P and 0 < c.beta < P and 0 <= c.gamma < P
        assert len(m["S"]) == u and sorted(m["S"]) == sorted(AR.compress(g.cfg.table(), c.theta, P) + [0] * (u - g.cfg.n_rows))
        for k in range(5):
            _check_hist(g, c, k)
            A, Ap, Sp, Z = m["A"][k], m["Ap"][k], m["Sp"][k], m["Z"][k]
            assert m["zero_den"][k] is None, (c.key, k)                                  # no denominator is zero
            assert len(A) == len(Ap) == len(Sp) == u and len(Z) == u + 1
            assert Z[0] == 1 and Z[u] == 1, (c.key, k)
            assert Ap == sorted(A) and sorted(Sp) == sorted(m["S"])
            assert sum(1 for v in A if v) <= sum(c.hists[k])
            if c.shapes[k] == "full" and 0 not in AR.compress(g.cfg.table()[1:], c.theta, P):
                assert Ap[0] != 0                                                        # no padding row: the value-0 group is empty in A'
