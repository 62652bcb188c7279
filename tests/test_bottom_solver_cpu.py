"""mg_bottom_solver / hg_bottom_solver / max_mg_bottom_nlevels through the layers that need no GPU: the defaults of the C-ABI, of its Python mirror and of
the reference's src/_parameters agree, the inputs reader carries the namelist keys into vdn_params, and vdn_init refuses a value outside FBoxLib's numbering."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# reference src/_parameters:55-57 (name, type, default) and mac_multigrid.f90:56 (bottom_solver_eps = 1.d-3); hg_bottom_solver_eps is this library's own
REFERENCE = dict(mg_bottom_solver=-1, hg_bottom_solver=-1, max_mg_bottom_nlevels=1000, mg_bottom_solver_eps=1.0e-3, hg_bottom_solver_eps=1.0e-3)


def test_defaults_agree_between_the_library_the_mirror_and_the_reference():
    from varden_amd import capi, inputs
    lib = capi.load()
    c = capi.Params()
    lib.vdn_params_default(C.byref(c))
    p = capi.default_params()
    names = [n for n, _ in capi.Params._fields_]
    assert names[-5:] == ["mg_bottom_solver", "hg_bottom_solver", "max_mg_bottom_nlevels", "mg_bottom_solver_eps", "hg_bottom_solver_eps"], "appended at the end of vdn_params"
    for name, want in REFERENCE.items():
        assert getattr(c, name) == want, (name, getattr(c, name))
        assert getattr(p, name) == want, (name, getattr(p, name))
    for name in ("mg_bottom_solver", "hg_bottom_solver", "max_mg_bottom_nlevels"):
        assert inputs.DEFAULTS[name] == REFERENCE[name]
    # the Fortran hosts declare the same defaults (probin_module of varden_boxlib.f90, the namelist of varden_main.f90)
    for f in ("varden_boxlib.f90", "varden_main.f90"):
        txt = open(os.path.join(ROOT, "varden_amd", "fortran", f)).read()
        for name in ("mg_bottom_solver", "hg_bottom_solver", "max_mg_bottom_nlevels"):
            m = re.search(r"\b%s\s*=\s*(-?\d+)" % name, txt)
            assert m and int(m.group(1)) == REFERENCE[name], (f, name)
    # the header documents all five
    hdr = open(os.path.join(ROOT, "include", "varden_amd.h")).read()
    for name in REFERENCE:
        assert name in hdr


def test_inputs_namelist_reaches_the_params():
    from varden_amd import inputs
    text = "&PROBIN\n dim_in = 3\n n_cellx = 40\n mg_bottom_solver = 2\n hg_bottom_solver = 1\n max_mg_bottom_nlevels = 7\n/\n"
    nl = dict(inputs.DEFAULTS)
    nl.update(inputs.parse_namelist(text))
    prm = inputs.namelist_params(nl)                       # what inputs.build hands to the driver
    assert (prm.mg_bottom_solver, prm.hg_bottom_solver, prm.max_mg_bottom_nlevels) == (2, 1, 7)
    assert (prm.mg_bottom_solver_eps, prm.hg_bottom_solver_eps) == (1.0e-3, 1.0e-3)
    nl = dict(inputs.DEFAULTS)
    nl.update(inputs.parse_namelist("&PROBIN\n dim_in = 3\n/\n"))
    prm = inputs.namelist_params(nl)
    assert (prm.mg_bottom_solver, prm.hg_bottom_solver, prm.max_mg_bottom_nlevels) == (-1, -1, 1000)
    # the project's own inputs file of tests/test_bottom_solver_fortran_gpu.py
    nl = dict(inputs.DEFAULTS)
    nl.update(inputs.parse_namelist(open(os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_3d_n40_cg")).read()))
    prm = inputs.namelist_params(nl)
    assert (prm.mg_bottom_solver, prm.hg_bottom_solver, nl["n_cellx"], nl["max_levs"]) == (2, 2, 40, 1)


@pytest.mark.parametrize("field", ["mg_bottom_solver", "hg_bottom_solver"])
def test_init_refuses_an_unknown_bottom_solver(field):
    from varden_amd import capi
    lib = capi.load()
    p = capi.default_params(**{field: 7})
    assert lib.vdn_init(C.byref(p), 0, 1, 0) != 0
    msg = lib.vdn_last_error()
    assert field.encode() in msg and b"7" in msg, msg
    p = capi.default_params(**{field: -2})
    assert lib.vdn_init(C.byref(p), 0, 1, 0) != 0 and field.encode() in lib.vdn_last_error()


def test_python_wrapper_and_signature_exist():
    from varden_amd import advance, capi
    assert "vdn_last_bottom_stats" in capi.SIGNATURES and callable(advance.last_bottom_stats)
