"""Refinement criteria chosen at run time (vdn_tag_boxes_by / vdn_make_new_grids_by): what can be held without a GPU -- the two entries are declared, typed and
exported, capi.TagCriterion has the C struct's layout, the namelist keys tag_field / tag_comp / tag_gt / tag_lt reach tag_criteria, and the Fortran sources name them."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vdn_tag_boxes_by", "vdn_make_new_grids_by")
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs", "inputs_vortextube_3d_amr")


def _header():
    txt = open(os.path.join(ROOT, "include", "varden_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_signatures_and_both_libraries_have_the_entries():
    from varden_amd import capi
    h = _header()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert name in capi.SIGNATURES
    assert len(capi.SIGNATURES["vdn_tag_boxes_by"][1]) == 8 and len(capi.SIGNATURES["vdn_make_new_grids_by"][1]) == 17
    for lib in ("libvarden_amd.so", "libvarden_amd_testing.so"):
        L = C.CDLL(os.path.join(ROOT, "varden_amd", "csrc", lib), mode=os.RTLD_LOCAL)
        for name in ENTRIES:
            assert hasattr(L, name), "%s does not export %s" % (lib, name)


def test_tag_criterion_mirrors_the_c_struct():
    from varden_amd import capi
    h = _header()
    maxlev = int(re.search(r"#define\s+VDN_MAXLEV\s+(\d+)", h).group(1))
    assert maxlev == capi.MAXLEV
    assert int(re.search(r"#define\s+VDN_TAG_MAX_CRITERIA\s+(\d+)", h).group(1)) == capi.TAG_MAX_CRITERIA == 8
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*vdn_tag_criterion\s*;", h)
    assert m, "vdn_tag_criterion is not declared"
    order = re.findall(r"\b(?:int|double)\s+(\w+)", m.group(1))
    assert order == ["field", "comp", "gt", "lt"] == [f[0] for f in capi.TagCriterion._fields_]
    assert C.sizeof(capi.TagCriterion) == 2 * 4 + 2 * 8 * maxlev
    assert capi.TagCriterion.gt.offset == 8 and capi.TagCriterion.lt.offset == 8 + 8 * maxlev
    for name, val in capi.TAG_FIELDS.items():
        macro = {"scalar": "VDN_TAG_SCALAR", "scalar_grad": "VDN_TAG_SCALAR_GRAD", "vorticity": "VDN_TAG_VORTICITY", "magvel": "VDN_TAG_MAGVEL"}[name]
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, h).group(1)) == val


def test_namelist_keys_reach_tag_criteria():
    from varden_amd import advance as adv
    from varden_amd.inputs import DEFAULTS, namelist_tag_criteria, parse_namelist
    inf = float("inf")
    nl = dict(DEFAULTS)
    nl.update(parse_namelist("&PROBIN\n max_levs = 3\n tag_field(1) = 'vorticity'\n tag_gt(1,1) = 3.5d0\n tag_gt(1,2) = 7.0\n"
                             " tag_field(3) = 'scalar_grad'\n tag_comp(3) = 2, tag_gt(3,1) = 0.25\n tag_lt(3,1) = 0.5\n u_bc(1,1) = 1.0\n/\n"))
    assert nl["u_bc(1,1)"] == 1.0 and nl["tag_field(1)"] == "vorticity" and nl["tag_gt(1,2)"] == 7.0
    crit = namelist_tag_criteria(nl)
    assert crit == [dict(field="vorticity", comp=1, gt=[3.5, 7.0]), dict(field="scalar_grad", comp=2, gt=[0.25], lt=[0.5])]
    arr, n = adv.tag_criteria(crit)
    assert n == 2
    assert (arr[0].field, arr[0].comp, list(arr[0].gt), list(arr[0].lt)) == (2, 0, [3.5, 7.0, 7.0, 7.0], [inf] * 4)      # a short list repeats its last value; no key: open
    assert (arr[1].field, arr[1].comp, list(arr[1].gt), list(arr[1].lt)) == (1, 1, [0.25] * 4, [0.5] * 4)
    # tuples, single numbers and None sides
    arr, n = adv.tag_criteria([("scalar", 1, (1.01, 1.1, 1.5)), ("magvel", 1, None, 2.0)])
    assert list(arr[0].gt) == [1.01, 1.1, 1.5, 1.5] and list(arr[1].gt) == [-inf] * 4 and list(arr[1].lt) == [2.0] * 4
    # refusals in Python
    bad = dict(DEFAULTS)
    bad.update(parse_namelist("&PROBIN\n tag_field(1) = 'enstrophy'\n tag_gt(1,1) = 1.0\n/\n"))
    with pytest.raises(ValueError, match="enstrophy"):
        namelist_tag_criteria(bad)
    with pytest.raises(ValueError, match="enstrophy"):
        adv.tag_criteria([dict(field="enstrophy", gt=1.0)])
    with pytest.raises(ValueError):
        adv.tag_criteria([dict(field="scalar", gt=1.0)] * 9)
    with pytest.raises(ValueError):
        adv.tag_criteria([])
    orphan = dict(DEFAULTS)
    orphan.update(parse_namelist("&PROBIN\n tag_gt(2,1) = 1.0\n/\n"))
    with pytest.raises(ValueError, match="tag_field"):
        namelist_tag_criteria(orphan)
    # no keys: None, and every reference inputs file is such a namelist
    assert namelist_tag_criteria(dict(DEFAULTS)) is None
    ref = dict(DEFAULTS)
    ref.update(parse_namelist(open(os.path.join(ROOT, "tests", "golden", "inputs", "inputs_vortextube_3d")).read()))
    assert namelist_tag_criteria(ref) is None


def test_the_adaptive_vortex_tube_inputs():
    from varden_amd.inputs import DEFAULTS, namelist_tag_criteria, parse_namelist
    nl = dict(DEFAULTS)
    nl.update(parse_namelist(open(INPUTS).read()))
    assert (nl["prob_type"], nl["dim_in"], nl["max_levs"], nl["regrid_int"], nl["n_cellx"], nl["n_celly"], nl["n_cellz"]) == (4, 3, 2, 2, 32, 32, 32)
    crit = namelist_tag_criteria(nl)
    assert len(crit) == 1 and crit[0]["field"] == "vorticity" and len(crit[0]["gt"]) == 1 and "lt" not in crit[0]
    readme = open(INPUTS.replace("inputs_vortextube_3d_amr", "README.inputs_vortextube_3d_amr")).read()
    assert repr(crit[0]["gt"][0]) in readme          # the literal and how it was obtained


def test_fortran_sources_name_the_keys_and_the_entry():
    main = open(os.path.join(ROOT, "varden_amd", "fortran", "varden_main.f90")).read()
    mod = open(os.path.join(ROOT, "varden_amd", "fortran", "varden_amd_mod.f90")).read()
    nml = re.search(r"namelist /probin/(.*?)\n\s*\n", main, flags=re.S).group(1)
    for key in ("tag_field", "tag_comp", "tag_gt", "tag_lt"):
        assert re.search(r"\b%s\b" % key, nml), key
    assert len(re.findall(r"call make_new_grids_by\(", main)) == 2               # initial grids and regrid
    assert 'bind(C, name="vdn_make_new_grids_by")' in mod and 'bind(C, name="vdn_tag_boxes_by")' in mod
    assert re.search(r"subroutine make_new_grids_by\(", mod) and re.search(r"public ::.*make_new_grids_by", mod)
    m = re.search(r"type, bind\(C\), public :: vdn_tag_criterion(.*?)end type", mod, flags=re.S).group(1)
    assert re.search(r"integer\(c_int\) :: field, comp\s+real\(c_double\) :: gt\(4\), lt\(4\)", m)
