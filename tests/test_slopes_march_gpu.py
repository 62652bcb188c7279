"""The pair form of the slopes march (kk_slopes_pr, varden_amd/csrc/slopes_plan.h: two cells per lane, 16-byte accesses, the y-neighbours staged in LDS) against
the oracle's slope routine and against the two older launch forms: the same bits in every slope array of every box, ghost cells included, and the same max |u|.

Shapes (tests/_slopes_worker.py; the range of a launch is the box grown by one, 62 pairs fill a full-width segment, R rows a workgroup):
  8x8x8       narrower than any full segment: narrow segments only
  124x4x8     one full segment and one pair beside it, one row group
  126x7x12    a remainder of two pairs, rows no multiple of R
  132x(R+1)x20  a remainder segment, a second row group of few rows, several k-chunks
  61x5x9      odd width: the 16-byte accesses cannot be aligned, the box keeps the march with one cell per lane (form 1)
  inner       low corner (3, 5, 7) inside a 16^3 domain: no face has a boundary rule, the index parity differs
  two         a level of two boxes, 64 and 62 cells wide, side by side
each with the five boundary sets of test_slope and with an inlet, an outlet and a no-slip wall on every face in turn, slope_order 0, 2 and 4, three components
(max |u| rides along) and two.  The switches are read once per process: one child per launch form runs every case, once for the module; the default form's
child also holds every case against the oracle."""
import os

import pytest

from tests._slopes_worker import BCS, NCS, ORDERS, PAIR_FORM, SHAPES, case_name
from tests.children import ROOT, run_variant

pytestmark = pytest.mark.gpu

# launch form -> (switches, the form vdn_last_slopes_form must report; None: the pair form wherever the layouts take it)
FORMS = {"default": ({}, None), "one-cell": ({"VDN_SLOPES_MARCH": "1"}, 1), "per-cell": ({"VDN_SLOPES_MARCH": "0"}, 0)}


@pytest.fixture(scope="module")
def runs(gpu):
    out = {}
    for form, (extra, _) in FORMS.items():      # (in this order: a form that fails ends the fixture, none is started after it)
        r = run_variant([os.path.join(ROOT, "tests", "_slopes_worker.py")] + (["oracle"] if form == "default" else []), extra, 300)
        out[form] = {tok[1]: tok[2:] for tok in r["CASE"]}
    return out


@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pair_form_agrees_bit_for_bit_with_the_oracle_and_the_older_forms(runs, shape, order, nc):
    for bc in BCS:
        name = case_name(shape, bc, order, nc)
        got = {form: runs[form][name][0] for form in FORMS}
        assert len(set(got.values())) == 1, (name, got)
        for form, (_, want) in FORMS.items():      # a silent fallback must not pass
            assert int(runs[form][name][1]) == (PAIR_FORM[shape] if want is None else want), (name, form, runs[form][name][1])
        assert runs["default"][name][2] == "ok:", (name, runs["default"][name][2])
