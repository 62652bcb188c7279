"""vdn_last_bottom_form (0 bottom sweeps, 1 a Krylov solver in one workgroup, 2 over the whole GPU) through the layers that need no GPU: declared in the header,
exported by both builds of the library, typed in the Python mirror, wrapped by advance.last_bottom_form and present in the Fortran interface block."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_exists_in_every_layer():
    from varden_amd import advance, capi
    hdr = open(os.path.join(ROOT, "include", "varden_amd.h")).read()
    assert re.search(r"\bint\s+vdn_last_bottom_form\s*\(\s*int\s+which", hdr)
    for name in ("libvarden_amd.so", "libvarden_amd_testing.so"):
        L = C.CDLL(os.path.join(ROOT, "varden_amd", "csrc", name), mode=os.RTLD_LOCAL)
        assert hasattr(L, "vdn_last_bottom_form"), name
    assert capi.SIGNATURES["vdn_last_bottom_form"] == (C.c_int, [C.c_int])
    assert callable(advance.last_bottom_form)
    f90 = open(os.path.join(ROOT, "varden_amd", "fortran", "varden_amd_mod.f90")).read()
    block = f90[f90.index("  interface\n"):f90.index("  end interface")]
    assert re.search(r'function vdn_last_bottom_form\(which\) bind\(C, name="vdn_last_bottom_form"\)', block)


def test_it_answers_without_a_device():
    """one of the three forms for either multigrid (0 before any solve); anything but 0 or 1 is refused with -1"""
    from varden_amd import advance, capi
    lib = capi.load()
    assert all(lib.vdn_last_bottom_form(w) in (0, 1, 2) for w in (0, 1))
    assert advance.last_bottom_form("mac") == lib.vdn_last_bottom_form(0) and advance.last_bottom_form("hg") == lib.vdn_last_bottom_form(1)
    assert lib.vdn_last_bottom_form(2) == -1 and lib.vdn_last_bottom_form(-1) == -1


def test_the_crossover_keeps_the_existing_bottoms_in_one_workgroup():
    """the compiled-in crossover lies above every bottom level tests/test_bottom_solver_gpu.py solves: 22 x 11 x 11 cells, 23 x 12 x 12 nodes"""
    txt = open(os.path.join(ROOT, "varden_amd", "csrc", "krylov_grid.h")).read()
    x = int(re.search(r"#define\s+VDN_KRYLOV_GRID_MIN_POINTS\s+(\d+)", txt).group(1))
    assert x > 23 * 12 * 12 > 22 * 11 * 11
