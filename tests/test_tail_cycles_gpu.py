"""The one-workgroup tail cycles with their levels in LDS and the per-point constants in registers (kk_cc_tailcycle_lds, kk_nd_tailcycle_lds,
varden_amd/csrc/tail_plan.h) against the same levels launch by launch (VDN_MG_TAILCYCLE=0): the same bits, with graphs and without, and the oracle's solution.

Finest cells, the levels the tail cycle gets, and what they exercise:
  16^3      8^3, 4^3, 2^3 cells; 9^3, 5^3, 3^3 nodes: the tail of the benchmark's 256^3 box
  16x8x32   8 x 4 x 16, 4 x 2 x 8 cells: extents that differ, one above 8.  Nodes: 9 x 5 x 17 are 765 > 729, a level of its own, and the one level left is no
            tail cycle: form 0
  24^3      6^3, 3^3 cells; 7^3, 4^3 nodes: an odd coarsest level
Boundaries: walls on all faces (the singular system), an outlet at z-hi (a Dirichlet face: nd_is_dir nodes), an inlet at x-lo with its outlet, y periodic.
The periodic box keeps the body on global memory in the nodal solve (tail_plan refuses it) and, with the 3^3 level of 24^3, in the cell-centred one (an odd
periodic extent); 16^3 and 16x8x32 cells run the LDS body with the ghost images written by the owners.  cc-16-walls-alpha: the viscous solves' cell coefficient;
nd-16-outz-aniso: dx in ratio 1 : 1.2 : 1, the stencil's face weights; *-cg: the Krylov bottom solver, which keeps the body on global memory (form 0; its
solution is not the oracle's sweeps', so it is held to the other forms only).
The switches are read once per process: one child per launch form runs every case (tests/_tail_worker.py), once for the module.  Every case converges in the
oracle within mg_max_iter / hg_max_iter (python tests/_tail_worker.py oracle-only, on the CPU)."""
import os

import pytest

from tests.children import ROOT, run_variant, run_variants

pytestmark = pytest.mark.gpu

# the body the default form must report (vdn_last_tail_form), case by case: 1 wherever tail_plan takes the level set
FORM = {}
for _s in ("16", "16x8x32", "24"):
    for _b in ("walls", "outz", "inlet", "pery"):
        FORM["cc-%s-%s" % (_s, _b)] = 0 if (_s, _b) == ("24", "pery") else 1
        FORM["nd-%s-%s" % (_s, _b)] = 0 if (_b == "pery" or _s == "16x8x32") else 1
FORM.update({"cc-16-walls-alpha": 1, "cc-16-walls-cg": 0, "nd-16-outz-aniso": 1, "nd-16-walls-cg": 0})
FORMS = {"default": {}, "plain": {"VDN_MG_TAILCYCLE": "0"}, "nographs": {"VDN_NO_GRAPHS": "1"}}


@pytest.fixture(scope="module")
def runs(gpu):
    out = {}
    for form, extra in FORMS.items():      # (in this order: a form that fails ends the fixture, none is started after it)
        r = run_variant([os.path.join(ROOT, "tests", "_tail_worker.py")] + (["oracle"] if form == "default" else []), extra, 300)
        out[form] = {tok[1]: tok[2:] for tok in r["CASE"]}
    return out


@pytest.mark.parametrize("case", list(FORM))
def test_tail_cycle_in_lds_agrees_bit_for_bit_with_the_launches(runs, case):
    got = {form: tuple(runs[form][case][:2]) for form in FORMS}          # (hash of phi, cycles)
    print(case, got)
    assert len(set(got.values())) == 1, (case, got)
    for form in FORMS:
        want = 0 if form == "plain" else FORM[case]
        assert int(runs[form][case][2]) == want, (case, form, runs[form][case][2])


@pytest.mark.parametrize("case", [c for c in FORM if not c.endswith("-cg")])
def test_tail_cycle_in_lds_solve_matches_the_oracle(runs, case):
    verdict = runs["default"][case][3]
    print(case, verdict)
    assert verdict.startswith("ok:"), (case, verdict)


def test_whole_steps_are_bit_equal_to_the_launches(gpu):
    """the 32^3 bubble, three steps: u, s, gp and p of the default form and of VDN_MG_TAILCYCLE=0 (tests/util.state_hash: every box, ghost cells included)"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from varden_amd import driver\n"
            "from varden_amd.capi import default_params\n"
            "from tests.util import state_hash\n"
            "G = driver.Varden(32, [[15, 15]] * 3, default_params(cflfac=0.9), init_shrink=0.1, init_iter=1)\n"
            "for _ in range(3): G.step()\n"
            "print('HASH', state_hash(G, 1))\n") % ROOT
    a, b = run_variants(("-c", code), ({}, {"VDN_MG_TAILCYCLE": "0"}), 300)
    assert a["HASH"][0][1] == b["HASH"][0][1], (a, b)
