"""CPU: which evaluations h2r_verify_bases demands of a plan, over the whole grid of tests/verify_cases.py (host code: no device, no ctx).
The library takes that list from a walk of its one constraint expression (csrc/h2r_constraints.hpp); the second
opinion here is the model's own restatement, opening_ref.constraint_at_point, run over mappings that record every (group, index,
rotation) it touches.  A plan that lacks one evaluation of that read set is refused; a plan that lacks an evaluation outside it -- the
random polynomial's, an unused fixed column's -- is accepted, so the refusals are about the missing value and not about the editing."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import create_proof_ref as C
import opening_ref as O
import transcript_ref as T
import verify_cases as VC
from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import lib

BIT = {0: 0, 1: 1, O.LAST: 2, -1: 3}        # a rotation of the model -> the point set of a plan mask


class Reads:
    """evals[group][index][rotation] of constraint_at_point: the value is 0, the key is logged."""

    def __init__(self, log, path=()):
        self.log, self.path = log, path

    def __getitem__(self, key):
        path = self.path + (key,)
        if len(path) < 3:
            return Reads(self.log, path)
        self.log.add(path)
        return 0


def read_set(cfg):
    """{(group, index, point set)} the model's expression reads; l0 / l_last / l_active are no evaluations of the verifier's (closed form)."""
    log = set()
    O.constraint_at_point(cfg, Reads(log), (0, 0, 0, 0), 0, T.R)
    return {(g, i, BIT[rot]) for g, i, rot in log if g != "l"}


def without(vcfg, group, index, bit):
    """A copy of the configuration whose plans lack point set `bit` of one column; an entry left with no point set is taken out."""
    out = type(vcfg).from_buffer_copy(vcfg)
    gid = _lib.VERIFY_GROUPS.index(group)
    for plan, count in ((out.eval_plan, "num_eval_plan"), (out.open_plan, "num_open_plan")):
        entries = [(e.group, e.index, e.mask & ~(1 << bit) if (e.group, e.index) == (gid, index) else e.mask) for e in plan[:getattr(out, count)]]
        kept = [e for e in entries if e[2]]
        for slot, (g, i, m) in zip(plan, kept + [(0, 0, 0)] * (len(entries) - len(kept))):
            slot.group, slot.index, slot.mask = g, i, m
        setattr(out, count, len(kept))
    return out


@pytest.mark.parametrize("domain", VC.DOMAINS, ids=["k%d-bf%d" % d for d in VC.DOMAINS])
def test_a_plan_holds_what_the_expression_reads(domain):
    bases = lambda vcfg: lib().h2r_verify_bases(ctypes.byref(vcfg), None)
    spare = set()                                                                  # the groups of evaluations that a plan holds and no term reads
    for shape in VC.shapes(domain):
        sid, cfg = VC.shape_id(shape), VC.config_of(shape)
        vcfg = VC.verify_config(cfg, False)
        nb = bases(vcfg)
        assert nb != 0, sid
        reads, held = read_set(cfg), set(C.queries(C.eval_plan(cfg)))
        assert reads <= held, "%s: the model's own plan lacks %r" % (sid, sorted(reads - held))
        for g, i, bit in sorted(reads):
            assert bases(without(vcfg, g, i, bit)) == 0, "%s: accepted without %s %d at point set %d" % (sid, g, i, bit)
        for g, i, bit in sorted(held - reads):
            assert bases(without(vcfg, g, i, bit)) == nb, "%s: refused without %s %d at point set %d, which nothing reads" % (sid, g, i, bit)
            spare.add(g)
    assert spare >= {"random", "fixed"}, "the accepted half is empty or probes the random polynomial alone"

