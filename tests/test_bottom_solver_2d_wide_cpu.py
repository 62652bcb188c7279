"""What tests/test_bottom_solver_2d_wide_gpu.py relies on and needs no GPU: its inputs file, and where the crossover between the two Krylov forms lies."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_n202_inputs_file_parses():
    from varden_amd import inputs
    nl = dict(inputs.DEFAULTS)
    nl.update(inputs.parse_namelist(open(os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_2d_n202_cg")).read()))
    prm = inputs.namelist_params(nl)
    assert prm.dm == 2 and (nl["n_cellx"], nl["n_celly"], nl["max_levs"]) == (202, 202, 1)
    assert (prm.mg_bottom_solver, prm.hg_bottom_solver) == (2, 2) and prm.visc_coef > 0.0
    assert nl["max_grid_size"] >= 202, "one box"
    assert os.path.exists(os.path.join(ROOT, "tests", "golden", "inputs", "README.inputs_bubble_2d_n202_cg"))


def test_the_crossovers_keep_the_small_bottoms_in_one_workgroup_and_the_wide_ones_grid_wide():
    """the shared constant serves dm = 3; the dm = 2 one was measured apart (the table beside it).  Both lie above 23 x 12 nodes, the largest bottom of
    tests/test_bottom_solver_2d_gpu.py; the dm = 2 one is not above 101 x 101 cells, the bottom of the whole steps of tests/test_bottom_solver_2d_wide_gpu.py and
    the smallest of that file (BAND: 45 x 227, STRIP: 21 x 487)"""
    txt = open(os.path.join(ROOT, "varden_amd", "csrc", "krylov_grid.h")).read()
    x3 = int(re.search(r"#define\s+VDN_KRYLOV_GRID_MIN_POINTS\s+(\d+)", txt).group(1))
    x2 = int(re.search(r"#define\s+VDN_KRYLOV_GRID_MIN_POINTS_2D\s+(\d+)", txt).group(1))
    assert 23 * 12 <= x3 and 23 * 12 <= x2 <= 101 * 101 <= 45 * 227 <= 21 * 487
    src = open(os.path.join(ROOT, "varden_amd", "csrc", "dim2.hip")).read()
    assert src.count("VDN_KRYLOV_GRID_MIN_POINTS_2D);") == 2, "both dm = 2 multigrids take the dm = 2 constant"
    # both dm = 2 multigrids visit their bottom through the one host visit of krylov_grid.h, which takes the grid-wide form above the crossover
    assert src.count("mg_krylov_visit(M.kry,") == 2 and "always one workgroup" not in src
    visit = txt[txt.index("void mg_krylov_visit("):]
    assert "if (!kry.part)" in visit and "krylov_grid_visit<VDN_KRYLOV_CG>" in visit and "always one workgroup" not in txt
