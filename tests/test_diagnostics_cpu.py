"""Run diagnostics on the device (vdn_diagnostics, varden_amd/csrc/diag.hip): what can be held without a GPU -- the struct and both entries are declared, typed and
exported, capi.Diag and the Fortran type mirror vdn_diag member for member, the namelist keys exist in both hosts, the slab planner (csrc/diag_plan.h) tiles every
box once in (level, box, k) order, and the call refuses to run uninitialised."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = ["cells", "cells_lev", "nonfinite", "volume", "volume_lev", "sum_s", "momentum", "kinetic", "enstrophy",
           "s_min", "s_max", "u_min", "u_max", "magvel_max", "vort_min", "vort_max"]


def _header():
    txt = open(os.path.join(ROOT, "include", "varden_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _members(body, types):
    """[(name, length)] of the declarations `type a, b[4], c(11)` in a struct body (C or Fortran)"""
    out = []
    for decl in re.findall(r"(?:%s)\s*(?:::)?\s*([^;\n]+)" % types, body):
        for item in decl.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:[\[(](\d+)[\])])?\s*", item)
            assert m, item
            out.append((m.group(1), int(m.group(2) or 1)))
    return out


def test_struct_and_signatures():
    from varden_amd import capi
    h = _header()
    assert re.search(r"\bint\s+vdn_diagnostics\s*\(", h) and re.search(r"\bsize_t\s+vdn_diag_sizeof\s*\(", h)
    assert "vdn_diagnostics" in capi.SIGNATURES and "vdn_diag_sizeof" in capi.SIGNATURES
    assert len(capi.SIGNATURES["vdn_diagnostics"][1]) == 8
    assert int(re.search(r"#define\s+VDN_DIAG_VORT\s+(\d+)", h).group(1)) == capi.DIAG_VORT
    body = re.search(r"typedef\s+struct\s+vdn_diag\s*\{([^}]*)\}\s*vdn_diag\s*;", h).group(1)
    cm = _members(body, r"long long|double")
    assert [n for n, _ in cm] == MEMBERS == [f[0] for f in capi.Diag._fields_]
    for (name, length), (_, ctype) in zip(cm, capi.Diag._fields_):
        assert C.sizeof(ctype) == 8 * length, name
    assert C.sizeof(capi.Diag) == 8 * sum(n for _, n in cm)
    for lib in ("libvarden_amd.so", "libvarden_amd_testing.so"):
        L = C.CDLL(os.path.join(ROOT, "varden_amd", "csrc", lib), mode=os.RTLD_LOCAL)
        L.vdn_diag_sizeof.restype = C.c_size_t
        assert L.vdn_diag_sizeof() == C.sizeof(capi.Diag), lib
        assert hasattr(L, "vdn_diagnostics"), lib
    # the Fortran type: the same members in the same order, 8-byte kinds
    mod = open(os.path.join(ROOT, "varden_amd", "fortran", "varden_amd_mod.f90")).read()
    ft = re.search(r"type, bind\(C\), public :: vdn_diag\n(.*?)end type vdn_diag", mod, flags=re.S).group(1)
    assert _members(ft, r"integer\(c_long_long\)|real\(c_double\)") == cm
    assert 'bind(C, name="vdn_diagnostics")' in mod and 'bind(C, name="vdn_diag_sizeof")' in mod
    assert re.search(r"subroutine diagnostics\(", mod) and re.search(r"public ::.*\bdiagnostics\b", mod)


def test_namelist_keys_in_both_hosts():
    from varden_amd import advance as adv
    from varden_amd import inputs
    assert inputs.DEFAULTS["diag_int"] == 0 and inputs.DEFAULTS["diag_file_name"] == "varden_diag.out"
    nl = inputs.parse_namelist("&PROBIN\n diag_int = 5\n diag_file_name = 'out/d.txt'\n/\n")
    assert nl == dict(diag_int=5, diag_file_name="out/d.txt")
    main = open(os.path.join(ROOT, "varden_amd", "fortran", "varden_main.f90")).read()
    nml = re.search(r"namelist /probin/(.*?)\n\s*\n", main, flags=re.S).group(1)
    for key in ("diag_int", "diag_file_name"):
        assert re.search(r"\b%s\b" % key, nml), key
    assert re.search(r"integer :: diag_int = 0\b", main) and "diag_file_name = 'varden_diag.out'" in main
    # the line: step, time, dt, cells, nonfinite, volume, then integrals and extrema in struct order; header and data line have the same width
    cols = adv.diag_columns(2, 3)
    assert cols[:3] == ["cells", "nonfinite", "volume"] and cols[3:5] == ["sum_s1", "sum_s2"] and cols[-3:] == ["magvel_max", "vort_min", "vort_max"]
    d = dict(cells=0, nonfinite=0, volume=0.0, sum_s=[0.0] * 2, momentum=[0.0] * 3, kinetic=0.0, enstrophy=0.0, s_min=[0.0] * 2, s_max=[0.0] * 2,
             u_min=[0.0] * 3, u_max=[0.0] * 3, magvel_max=0.0, vort_min=0.0, vort_max=0.0)
    line, head = inputs.diag_line(3, 0.5, 0.25, d), inputs.diag_header(2, 3)
    assert len(line) == len(head) == 1 + 8 + 2 * 27 + 2 * 16 + 27 * (len(cols) - 2)
    assert line.startswith("       3   5.00000000000000000E-001   2.50000000000000000E-001               0               0   0.00000000000000000E+000")


def test_slab_planner(tmp_path):
    exe = str(tmp_path / "diag_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "varden_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "diag_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr


def test_refuses_without_a_gpu():
    """before vdn_init (or where it failed: no GPU) the call returns non-zero with a message"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    from varden_amd import capi
    lib = capi.load()
    out = capi.Diag()
    dx = (C.c_double * 3)(1.0, 1.0, 1.0)
    rc = lib.vdn_diagnostics(1, None, None, None, dx, None, 0, C.byref(out))
    assert rc != 0 and b"vdn_init" in lib.vdn_last_error()
    with pytest.raises(capi.VardenError, match="vdn_diagnostics"):
        capi.check(rc)
