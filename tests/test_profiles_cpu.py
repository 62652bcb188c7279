"""Plane-averaged profiles on the device (vdn_profiles, varden_amd/csrc/profiles.hip): what can be held without a GPU -- the struct and the four entries are
declared, typed and exported, capi.ProfileLayout and the Fortran type mirror vdn_profile_layout member for member, vdn_profiles_layout (a pure host function) gives
the offsets of the header's table, the namelist keys exist in both hosts, the command line has its two options, the piece planner (csrc/profile_plan.h) holds under
the sanitizers, and the call refuses to run uninitialised."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = ["nrow", "volume", "s", "ss", "u", "ru", "ruu", "sua", "s_min", "s_max", "u_min", "u_max"]
ENTRIES = {"vdn_profiles_layout": 3, "vdn_profile_layout_sizeof": 0, "vdn_profiles_nbins": 3, "vdn_profiles": 9}


def _header():
    txt = open(os.path.join(ROOT, "include", "varden_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_struct_and_signatures():
    from varden_amd import capi
    h = _header()
    body = re.search(r"typedef\s+struct\s+vdn_profile_layout\s*\{([^}]*)\}\s*vdn_profile_layout\s*;", h).group(1)
    assert re.fullmatch(r"\s*int\s+([\w\s,]+);\s*", body), body
    cm = [m.strip() for m in re.fullmatch(r"\s*int\s+([\w\s,]+);\s*", body).group(1).split(",")]
    assert cm == MEMBERS == [f[0] for f in capi.ProfileLayout._fields_]
    assert all(f[1] is C.c_int for f in capi.ProfileLayout._fields_) and C.sizeof(capi.ProfileLayout) == 4 * len(MEMBERS)
    for name, nargs in ENTRIES.items():
        assert re.search(r"\b%s\s*\(" % name, h), name
        assert name in capi.SIGNATURES and len(capi.SIGNATURES[name][1]) == nargs, name
    assert re.search(r"\blong\s+vdn_profiles_nbins\s*\(", h) and capi.SIGNATURES["vdn_profiles_nbins"][0] is C.c_long
    for lib in ("libvarden_amd.so", "libvarden_amd_testing.so"):
        L = C.CDLL(os.path.join(ROOT, "varden_amd", "csrc", lib), mode=os.RTLD_LOCAL)
        L.vdn_profile_layout_sizeof.restype = C.c_size_t
        assert L.vdn_profile_layout_sizeof() == C.sizeof(capi.ProfileLayout), lib
        for name in ENTRIES:
            assert hasattr(L, name), (lib, name)
    # the Fortran type: the same members in the same order, c_int; the wrappers are public
    mod = open(os.path.join(ROOT, "varden_amd", "fortran", "varden_amd_mod.f90")).read()
    ft = re.search(r"type, bind\(C\), public :: vdn_profile_layout\n\s*integer\(c_int\) :: ([^\n]*)\n\s*end type vdn_profile_layout", mod).group(1)
    assert [m.strip() for m in ft.split(",")] == MEMBERS
    for name in ENTRIES:
        assert 'bind(C, name="%s")' % name in mod, name
    for name in ("profiles_layout", "profiles_nbins", "profiles"):
        assert re.search(r"(subroutine|function) %s\(" % name, mod) and re.search(r"public ::.*\b%s\b" % name, mod), name


@pytest.mark.parametrize("dm,nscal", [(3, 2), (3, 11), (2, 2)])
def test_layout_offsets(dm, nscal):
    """nrow and the offsets against the table of include/varden_amd.h; the row groups tile 0 .. nrow-1 without gap or overlap"""
    from varden_amd import advance as adv
    from varden_amd import capi
    lib = capi.load()
    lay = capi.ProfileLayout()
    assert lib.vdn_profiles_layout(dm, nscal, C.byref(lay)) == 0
    count = dict(volume=1, s=nscal, ss=nscal, u=dm, ru=dm, ruu=dm * (dm + 1) // 2, sua=nscal - 1, s_min=nscal, s_max=nscal, u_min=dm, u_max=dm)
    assert list(count) == MEMBERS[1:] == list(adv.PROFILE_GROUPS)
    rows = []
    for g in MEMBERS[1:]:
        assert getattr(lay, g) == len(rows), (g, getattr(lay, g), len(rows))
        rows += [g] * count[g]
    assert lay.nrow == len(rows) == 3 * nscal + 2 * dm + dm * (dm + 1) // 2 + 2 * nscal + 2 * dm
    assert lay.nrow == {(3, 2): 28, (3, 11): 73, (2, 2): 21}[dm, nscal]
    d = adv.profiles_layout(dm, nscal)
    assert d["nrow"] == lay.nrow and all(d[g] == (getattr(lay, g), count[g]) for g in count)
    cols = adv.profile_columns(nscal, dm)
    assert len(cols) == lay.nrow and len(set(cols)) == lay.nrow and cols[lay.ruu] == "ruu11" and cols[lay.sua] == "sua2" and cols[lay.u_max] == "u_max1"
    if dm == 3:
        assert cols[lay.ruu:lay.sua] == ["ruu11", "ruu12", "ruu13", "ruu22", "ruu23", "ruu33"]
    # refused: a dimension or a scalar count the library does not run, a NULL struct
    for bad in ((1, 2), (4, 2), (3, 0), (3, 12)):
        assert lib.vdn_profiles_layout(bad[0], bad[1], C.byref(lay)) != 0 and b"vdn_profiles_layout" in lib.vdn_last_error()
    assert lib.vdn_profiles_layout(3, 2, None) != 0


def test_namelist_keys_in_both_hosts():
    from varden_amd import inputs
    assert inputs.DEFAULTS["prof_int"] == 0 and inputs.DEFAULTS["prof_axis"] == -1 and inputs.DEFAULTS["prof_base_name"] == "prof"
    nl = inputs.parse_namelist("&PROBIN\n prof_int = 5\n prof_axis = 2\n prof_base_name = 'out/p'\n/\n")
    assert nl == dict(prof_int=5, prof_axis=2, prof_base_name="out/p")
    main = open(os.path.join(ROOT, "varden_amd", "fortran", "varden_main.f90")).read()
    nml = re.search(r"namelist /probin/(.*?)\n\s*\n", main, flags=re.S).group(1)
    for key in ("prof_int", "prof_axis", "prof_base_name"):
        assert re.search(r"\b%s\b" % key, nml), key
    assert re.search(r"integer :: prof_int = 0\b", main) and re.search(r"integer :: prof_axis = -1\b", main) and "prof_base_name = 'prof'" in main
    text = open(os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_3d_n32_prof")).read()
    nl = dict(inputs.DEFAULTS, **inputs.parse_namelist(text))
    assert nl["prof_int"] == 2 and nl["prof_axis"] == -1 and nl["diag_int"] == 1 and nl["max_levs"] == 2 and nl["n_cellx"] == 32


def test_profile_text():
    """the file: the tag, dm, axis (from 1), nbins, step, time, the column names, one line per bin; header and data lines have the same width"""
    import numpy as np
    from varden_amd import advance as adv
    from varden_amd import inputs
    P = adv.Profiles(2, 3, 2, (np.arange(4) + 0.5) * 0.25, np.arange(1, 28 * 4 + 1, dtype=np.float64).reshape(28, 4), np.array([7, 8, 9, 10]))
    lines = inputs.profile_text(P, 3, 0.5).split("\n")
    assert lines[:6] == ["# VDN_PROFILES 1", "# dm 3", "# axis 3", "# nbins 4", "# step 3", "# time   5.00000000000000000E-001"] and lines[-1] == ""
    assert lines[6].split() == ["#", "x", "cells"] + adv.profile_columns(2, 3) and len(lines) == 7 + 4 + 1
    assert all(len(ln) == 27 + 16 + 27 * 28 for ln in lines[6:-1])
    assert lines[8].startswith("   3.75000000000000000E-001               8   2.00000000000000000E+000   6.00000000000000000E+000")
    assert P["volume"].shape == (4,) and P["ruu"].shape == (6, 4) and P["sua"].shape == (1, 4) and P.mean("s").shape == (2, 4)
    assert np.array_equal(P.mean("ru"), P.rows[8:11] / P.rows[0]) and set(P.keys()) == set(("x", "cells") + adv.PROFILE_GROUPS)
    with pytest.raises(KeyError):
        P.mean("s_min")


def test_command_line_options():
    r = subprocess.run([sys.executable, "-m", "varden_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--prof-int" in r.stdout and "--prof-axis" in r.stdout, r.stdout + r.stderr


def test_piece_planner(tmp_path):
    exe = str(tmp_path / "profile_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "varden_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "profile_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr


def test_level_lists_are_properly_nested():
    """the hierarchy of the GPU tests (tests/_profiles_worker.py: AMR3) as vdn_layout_create wants it: every fine box starts on an even and ends on an odd index, lies
    inside the union of the boxes of the level below, and the boxes of a level are disjoint"""
    import numpy as np
    from tests._profiles_worker import AMR3
    nbase, levels = AMR3
    inbox = []
    for l, boxes in enumerate(levels):
        m = np.zeros((nbase << l,) * 3, dtype=np.int32)
        for lo, hi in boxes:
            assert all(0 <= lo[d] <= hi[d] < nbase << l for d in range(3))
            if l > 0:
                assert all(lo[d] % 2 == 0 and hi[d] % 2 == 1 for d in range(3)), (l, lo, hi)
                assert inbox[l - 1][tuple(slice(lo[d] // 2, hi[d] // 2 + 1) for d in range(3))].all(), (l, lo, hi)
            m[tuple(slice(lo[d], hi[d] + 1) for d in range(3))] += 1
        assert m.max() == 1
        inbox.append(m == 1)
    assert inbox[0].all()
    # ... and the library takes them (the layout is host data: no GPU needed)
    from varden_amd import boxlib as bl
    mla = bl.MLLayout([((0, 0, 0), ((nbase << l) - 1,) * 3) for l in range(3)], levels, rr=[(2, 2, 2)] * 2)
    assert mla.h
    mla.destroy()
    # one level-1 box is not aligned with the other and they share no face; the level-2 box lies strictly inside the first
    (a, b), (c,) = levels[1], levels[2]
    assert not any(all(a[0][e] <= b[1][e] and b[0][e] <= a[1][e] for e in range(3) if e != d) and (a[1][d] + 1 == b[0][d] or b[1][d] + 1 == a[0][d]) for d in range(3))
    assert all(a[0][d] * 2 < c[0][d] and c[1][d] < a[1][d] * 2 + 1 for d in range(3))


def test_refuses_without_a_gpu():
    """before vdn_init (or where it failed: no GPU) the call returns non-zero with the library's message"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    from varden_amd import capi
    lib = capi.load()
    out, cells = (C.c_double * 28)(), (C.c_longlong * 1)()
    dx = (C.c_double * 3)(1.0, 1.0, 1.0)
    rc = lib.vdn_profiles(1, None, None, None, dx, 0, 1, out, cells)
    assert rc != 0 and b"vdn_init" in lib.vdn_last_error() and lib.vdn_last_error().startswith(b"vdn_profiles")
    with pytest.raises(capi.VardenError, match="vdn_profiles"):
        capi.check(rc)
    assert lib.vdn_profiles_nbins(1, None, 0) == -1 and b"vdn_profiles_nbins" in lib.vdn_last_error()
