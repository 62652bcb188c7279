"""The composite-grid reductions (vdn_diagnostics, vdn_profiles, vdn_pdf, vdn_pdf2; varden_amd/csrc/composite.h) give the bits recorded in
tests/golden/composite_reduction_bits.json: one SHA-256 per case of tools/reduction_bits.py over the raw bytes of every output array.  The file was written by
`python tools/reduction_bits.py --out tests/golden/composite_reduction_bits.json` with the library as it stood BEFORE the three entries were moved onto their shared
header; a change to the thread -> cell map, a tree or the slot order of a final sum gives another hash."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reductions_give_the_recorded_bits(gpu):
    import varden_amd
    from varden_amd import advance, boxlib, capi  # noqa: F401
    spec = importlib.util.spec_from_file_location("reduction_bits", os.path.join(ROOT, "tools", "reduction_bits.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "composite_reduction_bits.json")))
    got = dict(tool.figures(varden_amd))
    assert sorted(got) == sorted(want) and len(want) == 26
    differ = [name for name in want if got[name] != want[name]]
    assert not differ, differ
