"""Values at points and tracer particles (varden_amd/csrc/particles.hip): what can be held without a GPU -- every entry is declared in the header, typed in
capi.SIGNATURES with as many arguments, exported by both libraries and bound in the Fortran module; the box locator (csrc/particle_plan.h) agrees with a search over
all boxes on every cell; the numpy restatement's boundary rule does what DESIGN.md section 21 says; the calls refuse to run uninitialised."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["vdn_sample_points", "vdn_particles_create", "vdn_particles_destroy", "vdn_particles_count", "vdn_particles_get", "vdn_particles_advance",
           "vdn_particles_sample", "vdn_particles_write", "vdn_particles_read"]
WRAPPERS = ["sample_points", "particles_create", "particles_destroy", "particles_count", "particles_get", "particles_advance", "particles_sample", "particles_write",
            "particles_read"]


def _header():
    txt = open(os.path.join(ROOT, "include", "varden_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_entries_declared_everywhere():
    from varden_amd import capi
    h = _header()
    mod = open(os.path.join(ROOT, "varden_amd", "fortran", "varden_amd_mod.f90")).read()
    libs = [C.CDLL(os.path.join(ROOT, "varden_amd", "csrc", lib), mode=os.RTLD_LOCAL) for lib in ("libvarden_amd.so", "libvarden_amd_testing.so")]
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, h)
        assert m, name
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in capi.SIGNATURES, name
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, (name, nargs, len(args))
        for lib in libs:
            assert hasattr(lib, name), name
        f = re.search(r"integer\(c_int\) function %s\(([^)]*)\)\s*(?:&\s*)?bind\(C, name=\"%s\"\)" % (name, name), mod)
        assert f, name
        assert len([a for a in f.group(1).split(",") if a.strip()]) == nargs, name
    assert re.search(r"typedef\s+struct\s+vdn_particles\s+vdn_particles\s*;", h)
    for w in WRAPPERS:
        assert re.search(r"(subroutine|function) %s\(" % w, mod) and re.search(r"public ::.*\b%s\b" % w, mod), w


def test_locator(tmp_path):
    exe = str(tmp_path / "particle_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "varden_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "particle_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr


def test_boundary_rule_of_the_reference():
    """the numpy restatement the GPU tests compare against: wrap, mirror once and clamp, crossing of an open face"""
    from tests._particles_worker import OPEN, PER, WALL, boundary
    p = np.array([-0.25, 0.0, 0.5, 1.0, 1.25, -3.0, 3.5])
    q, c = boundary(p, 1.0, PER, PER)
    assert np.array_equal(q, [0.75, 0.0, 0.5, 0.0, 0.25, 0.0, 1.0]) and not c.any()          # (more than a domain length: wrapped once, then clamped)
    q, c = boundary(p, 1.0, WALL, WALL)
    assert np.array_equal(q, [0.25, 0.0, 0.5, 1.0, 0.75, 1.0, 0.0]) and not c.any()
    q, c = boundary(p, 1.0, OPEN, OPEN)
    assert np.array_equal(c, [True, False, False, False, True, True, True]) and np.array_equal(q, p)
    q, c = boundary(p, 1.0, OPEN, WALL)
    assert np.array_equal(c, [True, False, False, False, False, True, False]) and q[4] == 0.75


def test_namelist_keys_in_both_hosts():
    from varden_amd import inputs
    assert inputs.DEFAULTS["particle_lattice"] == (0, 0, 0) and inputs.DEFAULTS["particle_int"] == 0 and inputs.DEFAULTS["particle_base_name"] == "part"
    text = "&PROBIN\n particle_lattice(1) = 4\n particle_lattice(2) = 5\n particle_lattice(3) = 6\n particle_int = 2\n particle_base_name = 'tr'\n/\n"
    nl = dict(inputs.DEFAULTS)
    nl.update(inputs.parse_namelist(text))
    assert inputs.namelist_particle_lattice(nl, text) == (4, 5, 6) and nl["particle_int"] == 2 and nl["particle_base_name"] == "tr"
    text = "&PROBIN\n particle_lattice = 8, 8 2\n/\n"
    nl = dict(inputs.DEFAULTS)
    nl.update(inputs.parse_namelist(text))
    assert inputs.namelist_particle_lattice(nl, text) == (8, 8, 2)
    assert inputs.namelist_particle_lattice(dict(inputs.DEFAULTS), "&PROBIN\n/\n") == (0, 0, 0)
    main = open(os.path.join(ROOT, "varden_amd", "fortran", "varden_main.f90")).read()
    nml = re.search(r"namelist /probin/(.*?)\n\s*\n", main, flags=re.S).group(1)
    for key in ("particle_lattice", "particle_int", "particle_base_name"):
        assert re.search(r"\b%s\b" % key, nml), key
    assert re.search(r"integer :: particle_lattice\(3\) = 0\b", main) and re.search(r"integer :: particle_int = 0\b", main) and "particle_base_name = 'part'" in main
    golden = open(os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_3d_n32_part")).read()
    g = dict(inputs.DEFAULTS)
    g.update(inputs.parse_namelist(golden))
    assert inputs.namelist_particle_lattice(g, golden) == (4, 4, 4) and (g["n_cellx"], g["max_levs"], g["regrid_int"], g["particle_int"], g["chk_int"]) == (32, 2, 2, 2, 3)
    assert os.path.exists(os.path.join(ROOT, "tests", "golden", "inputs", "README.inputs_bubble_3d_n32_part"))


def test_lattice():
    from varden_amd import advance as adv
    x = adv.particle_lattice((4, 2, 3), (1.0, 2.0, 0.5))
    assert x.shape == (24, 3)
    assert np.array_equal(x[:4, 0], [0.125, 0.375, 0.625, 0.875]) and np.array_equal(x[:4, 1], [0.5] * 4) and x[4, 1] == 1.5 and x[8, 2] == 0.25
    x = adv.particle_lattice((2, 2), (1.0, 1.0))
    assert x.shape == (4, 3) and (x[:, 2] == 0.0).all()


def test_refuses_uninitialised():
    """before vdn_init every call returns non-zero with a message that says so (a child process: this one may have initialised the library already)"""
    code = """
import ctypes as C, sys
sys.path.insert(0, %r)
from varden_amd import capi
lib = capi.load()
x = (C.c_double * 3)(0.5, 0.5, 0.5)
h, n, t = C.c_void_p(), C.c_long(), C.c_double()
calls = [lib.vdn_sample_points(1, None, None, 0, 1, 0, x, None, 1, x, x, None), lib.vdn_particles_create(1, x, C.byref(h)), lib.vdn_particles_count(None, C.byref(n), None),
         lib.vdn_particles_get(None, x, None), lib.vdn_particles_advance(None, 1, None, None, None, x, None, 0.1),
         lib.vdn_particles_sample(None, 1, None, None, 0, 1, 0, x, None, x, None), lib.vdn_particles_write(None, b"x", 0.0, 0, None, None),
         lib.vdn_particles_read(b"x", C.byref(h), C.byref(t))]
assert all(rc != 0 for rc in calls), calls
assert b"vdn_init" in lib.vdn_last_error(), lib.vdn_last_error()
assert lib.vdn_particles_destroy(None) == 0
print("refused")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "refused" in r.stdout, r.stdout + r.stderr
