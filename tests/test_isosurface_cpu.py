"""Isosurfaces on the device (vdn_isosurface, vdn_isosurface_write, varden_amd/csrc/iso.hip): what can be held without a GPU -- the struct and the entries are declared,
typed and exported in both libraries, capi.Iso and the Fortran type mirror vdn_iso member for member, the namelist keys (in both hosts), the command-line options and the .dat header exist, the PLY writer
and reader round-trip bytes, the per-cell routine (csrc/iso_cell.h) holds under the sanitizers, and the call refuses to run uninitialised."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"vdn_iso_sizeof": 0, "vdn_isosurface": 12, "vdn_isosurface_write": 6, "vdn_isosurface_timed": 14}
KEYS = dict(iso_int=0, iso_field="scalar", iso_comp=1, iso_value=0.0, iso_base_name="iso")
CTYPES = {"long long": C.c_longlong, "double": C.c_double}


def _header():
    txt = open(os.path.join(ROOT, "include", "varden_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_struct_and_signatures():
    from varden_amd import capi
    h = _header()
    body = re.search(r"typedef\s+struct\s+vdn_iso\s*\{([^}]*)\}\s*vdn_iso\s*;", h).group(1)
    members = []
    for ctype, names in re.findall(r"(long long|double)\s+([^;]+);", body):
        for m in names.split(","):
            name, dim = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", m).groups()
            members.append((name, CTYPES[ctype] * int(dim) if dim else CTYPES[ctype]))
    assert [m[0] for m in members] == ["ntri", "ntri_lev", "cut_cells", "cut_cells_lev", "nonfinite_cells", "written", "area", "area_lev", "area_vec", "volume_above", "volume"]
    assert [(n, t._type_ if hasattr(t, "_length_") else t, getattr(t, "_length_", 0)) for n, t in capi.Iso._fields_] == \
           [(n, t._type_ if hasattr(t, "_length_") else t, getattr(t, "_length_", 0)) for n, t in members]
    assert C.sizeof(capi.Iso) == 8 * (12 + 10)
    for name, nargs in ENTRIES.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, h)
        assert decl, name
        assert name in capi.SIGNATURES and len(capi.SIGNATURES[name][1]) == nargs, name
        assert (0 if decl.group(1).strip() == "void" else decl.group(1).count(",") + 1) == nargs, (name, decl.group(1))
    sig = capi.SIGNATURES["vdn_isosurface"][1]
    assert sig[7] is C.c_double and sig[8] is C.c_longlong and sig[10] is C.POINTER(C.c_ubyte) and sig[11] is C.POINTER(capi.Iso)
    for lib in ("libvarden_amd.so", "libvarden_amd_testing.so"):
        L = C.CDLL(os.path.join(ROOT, "varden_amd", "csrc", lib), mode=os.RTLD_LOCAL)
        L.vdn_iso_sizeof.restype = C.c_size_t
        assert L.vdn_iso_sizeof() == C.sizeof(capi.Iso), lib
        for name in ENTRIES:
            assert hasattr(L, name), (lib, name)
    # the Fortran type: the same members in the same order and kinds; the wrappers are public, also under the reference's container types; varden_main has the keys
    mod = open(os.path.join(ROOT, "varden_amd", "fortran", "varden_amd_mod.f90")).read()
    ft = re.search(r"type, bind\(C\), public :: vdn_iso\n\s*integer\(c_long_long\) :: ([^\n]*)\n\s*real\(c_double\) :: ([^\n]*)\n\s*end type vdn_iso", mod)
    fm = [re.sub(r"\((\d+)\)", r"[\1]", m.strip()) for part in ft.groups() for m in part.split(",")]
    assert fm == [n + ("[%d]" % t._length_ if hasattr(t, "_length_") else "") for n, t in members], fm
    for name in ("vdn_iso_sizeof", "vdn_isosurface", "vdn_isosurface_write"):
        assert 'bind(C, name="%s")' % name in mod, name
    for name in ("isosurface", "isosurface_write"):
        assert re.search(r"subroutine %s\(" % name, mod) and re.search(r"public ::.*\b%s\b" % name, mod), name
    box = open(os.path.join(ROOT, "varden_amd", "fortran", "varden_boxlib.f90")).read()
    assert re.search(r"(?m)^module isosurface_module$", box) and re.search(r"subroutine isosurface\(mla, mf, comp, bccomp, dx, the_bc_tower, value, iso, tri, lev\)", box)
    main = open(os.path.join(ROOT, "varden_amd", "fortran", "varden_main.f90")).read()
    nml = re.search(r"namelist /probin/(.*?)\n\n", main, flags=re.S).group(1)
    for key, default in KEYS.items():
        assert re.search(r"\b%s\b" % key, nml), key
        assert re.search(r"(?m)^\s*(integer|real\(dp_t\)|character\(len=\d+\)) :: %s = %s" % (key, "'%s'" % default if isinstance(default, str) else re.escape(str(default))), main), key
    # the per-cell routine is a dependency of every object
    mk = open(os.path.join(ROOT, "varden_amd", "csrc", "Makefile")).read()
    assert re.search(r"(?m)^SRC\s*:=.*\biso\.hip\b", mk) and len(re.findall(r"(?m)^%.*\.o:.*\biso_cell\.h\b", mk)) == 2


def test_namelist_keys_and_dat_text():
    from varden_amd import advance as adv
    from varden_amd import inputs
    assert {k: inputs.DEFAULTS[k] for k in KEYS} == KEYS
    nl = inputs.parse_namelist("&PROBIN\n iso_int = 5\n iso_field = 'velocity'\n iso_comp = 3\n iso_value = -1.5d0\n iso_base_name = 'out/s'\n/\n")
    assert nl == dict(iso_int=5, iso_field="velocity", iso_comp=3, iso_value=-1.5, iso_base_name="out/s")
    text = open(os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_3d_n32_iso")).read()
    nl = dict(inputs.DEFAULTS, **inputs.parse_namelist(text))
    assert nl["iso_int"] == 2 and nl["iso_field"] == "scalar" and nl["iso_comp"] == 1 and nl["iso_value"] == 5.5 and nl["iso_base_name"] == "iso"
    assert nl["diag_int"] == 1 and nl["max_levs"] == 2 and nl["n_cellx"] == 32 and nl["pdf_int"] == 0 and nl["dim_in"] == 3 and nl["prob_type"] == 1
    assert os.path.exists(os.path.join(ROOT, "tests", "golden", "inputs", "README.inputs_bubble_3d_n32_iso"))
    # the keys with the arguments over them; with iso_int = 0 nothing is looked at
    base = dict(inputs.DEFAULTS, dim_in=3)
    assert inputs.iso_keys(base) == (0, "scalar", 1, 0.0) and inputs.iso_keys(dict(base, iso_field="nonsense", iso_value=float("nan")))[0] == 0
    assert inputs.iso_keys(base, iso_int=2, iso_field="velocity", iso_comp=3, iso_value=0.25) == (2, "velocity", 3, 0.25)
    with pytest.raises(ValueError, match="iso_field"):
        inputs.iso_keys(dict(base, iso_int=1, iso_field="vorticity"))
    with pytest.raises(ValueError, match="iso_value"):
        inputs.iso_keys(dict(base, iso_int=1, iso_value=float("inf")))
    with pytest.raises(ValueError, match="dim_in = 3"):
        inputs.iso_keys(dict(base, iso_int=1, dim_in=2))
    with pytest.raises(ValueError, match="dim_in = 3"):
        inputs.run("&PROBIN\n dim_in = 2\n iso_int = 1\n/\n", report=None)           # refused before anything is built: no GPU is touched
    # the .dat file: a header line and data lines of the same width, in the format of a diagnostics line
    head = inputs.iso_header()
    assert head.split() == ["#", "step", "time"] + list(adv.ISO_DAT_COLUMNS) and adv.ISO_DAT_COLUMNS == ("ntri", "cut_cells", "area", "volume_above")

    class S:
        ntri, cut_cells, area, volume_above = 1234, 567, 0.5, 0.125
    line = inputs.iso_line(3, 0.25, S)
    assert len(line) == len(head) and line == "       3   2.50000000000000000E-001            1234             567   5.00000000000000000E-001   1.25000000000000000E-001\n"


def test_command_line_options():
    r = subprocess.run([sys.executable, "-m", "varden_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for opt in ("--iso-int", "--iso-field", "--iso-comp", "--iso-value"):
        assert opt in r.stdout, (opt, r.stdout)


def test_ply_round_trip(tmp_path):
    """the writer is a host function: the header lines of include/varden_amd.h, then the vertices and faces; the reader gives the bits back; the same arguments give the
    same bytes; an empty surface is a valid file"""
    from varden_amd import advance as adv
    from varden_amd import capi
    rng = np.random.default_rng(3)
    tri, level = rng.uniform(0.0, 1.0, (7, 3, 3)), np.array([0, 0, 1, 1, 2, 3, 0], dtype=np.uint8)

    class S:
        pass
    S.tri, S.level, S.value = tri, level, 1.0 / 3.0
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    adv.write_iso(a, S, 0.1)
    adv.write_iso(b, S, 0.1)
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read()
    head = raw[:raw.index(b"end_header\n")].decode().split("\n")
    assert head[:-1] == ["ply", "format binary_little_endian 1.0", "comment VDN_ISO 1 iso %.17g time %.17g" % (1.0 / 3.0, 0.1), "element vertex 21", "property double x",
                         "property double y", "property double z", "element face 7", "property list uchar int vertex_indices", "property uchar level"]
    body = raw[raw.index(b"end_header\n") + 11:]
    assert len(body) == 21 * 24 + 7 * 14 and body[:21 * 24] == tri.astype("<f8").tobytes()
    assert body[21 * 24:21 * 24 + 14] == b"\x03" + np.array([0, 1, 2], dtype="<i4").tobytes() + b"\x00" and body[-1:] == b"\x00" and body[-2 * 14 + 13:-14] == b"\x03"
    P = adv.read_iso(a)
    assert P["iso"] == 1.0 / 3.0 and P["time"] == 0.1 and np.array_equal(P["tri"].view(np.uint64), tri.view(np.uint64)) and np.array_equal(P["level"], level)
    assert np.array_equal(P["indices"], np.arange(21).reshape(7, 3))
    S.tri, S.level = np.zeros((0, 3, 3)), np.zeros(0, dtype=np.uint8)
    adv.write_iso(a, S, 0.0)
    P = adv.read_iso(a)
    assert P["tri"].shape == (0, 3, 3) and P["level"].shape == (0,) and open(a, "rb").read().endswith(b"end_header\n")
    # refusals of the writer: a directory that does not exist, triangles without their arrays
    lib = capi.load()
    assert lib.vdn_isosurface_write(os.fsencode(str(tmp_path / "none" / "x.ply")), 0, None, None, 0.0, 0.0) != 0 and b"cannot open" in lib.vdn_last_error()
    assert lib.vdn_isosurface_write(os.fsencode(a), 2, None, None, 0.0, 0.0) != 0 and lib.vdn_last_error().startswith(b"vdn_isosurface_write:")
    assert lib.vdn_isosurface_write(os.fsencode(a), -1, None, None, 0.0, 0.0) != 0 and lib.vdn_isosurface_write(None, 0, None, None, 0.0, 0.0) != 0
    S.tri = None
    with pytest.raises(ValueError, match="no triangles"):
        adv.write_iso(a, S, 0.0)
    open(b, "wb").write(b"ply\nformat ascii 1.0\nend_header\n")
    with pytest.raises(ValueError, match="not an isosurface file"):
        adv.read_iso(b)


def test_cell_routine(tmp_path):
    exe = str(tmp_path / "iso_cell_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "varden_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "iso_cell_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    # the header's case table against the restatement the GPU tests use, whose turns come from the rule: every case on the unit cube with values +-1, vertex for vertex
    from tests._isosurface_worker import _corners, _tet_case, turned
    r = subprocess.run([exe, "--cases"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        got[int(w[0]), int(w[1]), int(w[2])] = np.array([float(v) for v in w[3:]]).reshape(3, 3)
    seen = 0
    for n in range(6):
        c = _corners(n)
        for m in range(1, 15):
            qv = np.array([[1.0 if (m >> v) & 1 else -1.0 for v in range(4)]])
            X = np.array([[[float((c[v] >> d) & 1) for d in range(3)] for v in range(4)]])
            tris, _ = _tet_case(n, m, qv, X, 0.0, 1.0 / 6.0)
            for k, (T, turn) in enumerate(zip(tris, turned(n, m))):
                want = T[0][[0, 2, 1]] if turn else T[0]
                assert np.array_equal(got[n, m, k], want), (n, m, k, got[n, m, k], want)
                seen += 1
    assert seen == len(got) == 6 * (8 + 6 * 2)


def test_numpy_restatement_turns_triangles_by_the_rule():
    """tests/_isosurface_worker.turned, which the GPU tests hold the kernel against: every case of every tetrahedron has a decided orientation, a case and its
    complement turn the opposite way, and the six tetrahedra alternate"""
    from tests._isosurface_worker import ORDERS, turned
    for n in range(6):
        for m in range(1, 15):
            t, c = turned(n, m), turned(n, 15 - m)
            assert len(t) == len(c) == (2 if bin(m).count("1") == 2 else 1)
        inv = sum(ORDERS[n][a] > ORDERS[n][b] for a in range(3) for b in range(a + 1, 3))
        assert turned(n, 1) == [not v for v in turned(n, 14)]
        assert turned(n, 1)[0] == (turned(0, 1)[0] ^ (inv % 2 == 1)), n


def test_refuses_uninitialised():
    """before vdn_init the call returns non-zero with the library's message; the driver refuses dm = 2 and an unknown field.  A fresh process, so that the library is
    uninitialised whatever ran before in this one"""
    code = ("import ctypes as C\nfrom varden_amd import capi\nlib = capi.load()\nout = capi.Iso()\ndx = (C.c_double * 3)(1.0, 1.0, 1.0)\n"
            "rc = lib.vdn_isosurface(1, None, None, 0, 0, dx, None, 0.5, 0, None, None, C.byref(out))\n"
            "msg = lib.vdn_last_error()\nassert rc != 0 and msg.startswith(b'vdn_isosurface:') and b'vdn_init' in msg, (rc, msg)\n"
            "try:\n    capi.check(rc)\nexcept capi.VardenError as e:\n    assert 'vdn_isosurface' in str(e)\nelse:\n    raise SystemExit('no error raised')\nprint('refused')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("refused"), r.stdout + r.stderr
    from varden_amd import driver

    class Sim:
        dm, nscal = 2, 2
    with pytest.raises(ValueError, match="dm = 2"):
        driver._state_isosurface(Sim, "scalar", 0, 1.5, True)
    with pytest.raises(ValueError, match="isosurface field"):
        driver._state_isosurface(Sim, "magvel", 0, 1.5, True)
    Sim.dm = 3
    with pytest.raises(ValueError, match="comp"):
        driver._state_isosurface(Sim, "scalar", 2, 1.5, True)
