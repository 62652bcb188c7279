"""The 17^3 .. 65^3 levels of the nodal multigrid as one launch down and one up (kk_nd_lds_down / kk_nd_lds_up, varden_amd/csrc/nd_lds_plan.h) against the
six launches per level they replace (VDN_MG_LDS=0): the same bits, with graphs and without, and the oracle's solution.

Finest cells and what they exercise (level l has the finest extents / 2^l; bit l of the mask is set when level l took the tiled form):
  32^3       level 1 = 17^3 nodes: 8 tiles, every one touches faces of the level and owns a last node                          0b10
  64^3       33^3 (an interior tile exists) and 17^3; also without the nested iteration (hg_fmg = 0)                           0b110
  128x32x32  level 1 = 65 x 17 x 17 nodes, 8 x 2 x 2 tiles, under the paired finest level; level 2 has 8-cell axes: plain      0b10
  48x32x80   level 1 = 24 x 16 x 40 cells: 3 x 2 x 5 tiles; level 2 (12 x 8 x 20) is refused                                   0b10
  40^3       level 1 = 20 cells: refused                                                                                       0
Each with walls on all faces and with an outlet on one x, one y and one z face in turn (the Dirichlet skip on each axis); sigma is the bubble's 1 / rho.
The switches are read once per process: one child process per launch form runs every case (tests/_nd_lds_worker.py), once for the module."""
import os

import pytest

from tests.children import ROOT, run_variant

pytestmark = pytest.mark.gpu

MASKS = {"32": 0b10, "64": 0b110, "64-nofmg": 0b110, "128x32x32": 0b10, "48x32x80": 0b10, "40": 0}
BCS = ("walls", "outx", "outy", "outz")
FORMS = {"tiled": {}, "tiled-nographs": {"VDN_NO_GRAPHS": "1"}, "plain": {"VDN_MG_LDS": "0"}, "plain-nographs": {"VDN_MG_LDS": "0", "VDN_NO_GRAPHS": "1"}}


@pytest.fixture(scope="module")
def runs(gpu):
    out = {}
    for form, extra in FORMS.items():      # (in this order: a form that fails ends the fixture, none is started after it)
        r = run_variant([os.path.join(ROOT, "tests", "_nd_lds_worker.py")] + (["oracle"] if form == "tiled" else []), extra, 300)
        out[form] = {tok[1]: tok[2:] for tok in r["CASE"]}
    return out


@pytest.mark.parametrize("bcname", BCS)
@pytest.mark.parametrize("shape", list(MASKS))
def test_tiled_levels_agree_bit_for_bit_with_the_six_launches(runs, shape, bcname):
    case = "%s-%s" % (shape, bcname)
    got = {form: tuple(runs[form][case][:2]) for form in FORMS}          # (hash of phi, cycles)
    print(case, got)
    assert len(set(got.values())) == 1, (case, got)
    # this solve did run the listed levels as down / up by default and none under the switch
    for form in FORMS:
        want = 0 if form.startswith("plain") else MASKS[shape]
        assert int(runs[form][case][2]) == want, (case, form, runs[form][case][2])


@pytest.mark.parametrize("bcname", BCS)
@pytest.mark.parametrize("shape", list(MASKS))
def test_tiled_levels_solve_matches_the_oracle(runs, shape, bcname):
    case = "%s-%s" % (shape, bcname)
    verdict = runs["tiled"][case][3]
    print(case, verdict)
    assert verdict.startswith("ok:"), (case, verdict)
