"""The coarse correction inside the first post-smoothing march of the nodal multigrid (kk_nd_march_pair<0, 4, 1>) against the two-launch form
(kk_nd_prolong_m, then the plain march; VDN_ND_PROLONG_FUSED=0): the same bits, with graphs and without, and the oracle's solution.

Shapes that are paired on the finest level and thin elsewhere:
  128 x 16 x 24 cells: 65 node pairs -- one main tile and a 3-pair remainder segment; 25 planes in four slabs;
  260 x 8 x 12 cells: 131 pairs -- two main tiles and a 7-pair remainder; the 130-cell second level is paired too (its coarse level is the first
                       replicated one), so two fused levels sit in one cycle; rows beyond the level fall in the last tile;
  128 x 16 x 28 cells: 29 planes in slabs that start at planes 0, 7, 14, 21 -- the warm-up of the coarse planes for odd and even k0 (the balanced
                       slabs of the two shapes above all start on even planes).
Each with walls on all faces and with an outlet on one x, one y and one z face in turn (the Dirichlet skip on each axis); sigma is the bubble's 1 / rho.
The switches are read once per process: one child process per launch form runs every case (tests/_nd_prolong_worker.py), once for the module."""
import os

import pytest

from tests.children import ROOT, run_variant

pytestmark = pytest.mark.gpu

SHAPES = ("128x16x24", "260x8x12", "128x16x28")
BCS = ("walls", "outx", "outy", "outz")
FORMS = {"fused": {}, "fused-nographs": {"VDN_NO_GRAPHS": "1"}, "two-launch": {"VDN_ND_PROLONG_FUSED": "0"},
         "two-launch-nographs": {"VDN_ND_PROLONG_FUSED": "0", "VDN_NO_GRAPHS": "1"}}


@pytest.fixture(scope="module")
def runs(gpu):
    out = {}
    for form, extra in FORMS.items():      # (in this order: a form that fails ends the fixture, none is started after it)
        r = run_variant([os.path.join(ROOT, "tests", "_nd_prolong_worker.py")] + (["oracle"] if form == "fused" else []), extra, 300)
        out[form] = {tok[1]: tok[2:] for tok in r["CASE"]}
    return out


@pytest.mark.parametrize("bcname", BCS)
@pytest.mark.parametrize("shape", SHAPES)
def test_prolonging_march_agrees_bit_for_bit_with_the_two_launches(runs, shape, bcname):
    case = "%s-%s" % (shape, bcname)
    got = {form: tuple(runs[form][case][:2]) for form in FORMS}          # (hash of phi, cycles)
    print(case, got)
    assert len(set(got.values())) == 1, (case, got)
    # this solve did launch the prolonging march by default (on both paired levels of the 260-cell shape) and did not under the switch
    for form in FORMS:
        want = 0 if form.startswith("two-launch") else (3 if shape == "260x8x12" else 1)
        assert int(runs[form][case][2]) == want, (case, form, runs[form][case][2])


@pytest.mark.parametrize("bcname", BCS)
@pytest.mark.parametrize("shape", SHAPES)
def test_prolonging_march_solve_matches_the_oracle(runs, shape, bcname):
    case = "%s-%s" % (shape, bcname)
    verdict = runs["fused"][case][3]
    print(case, verdict)
    assert verdict.startswith("ok:"), (case, verdict)
