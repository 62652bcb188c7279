"""Tracer particles through the inputs runner and the Fortran host: tests/golden/inputs/inputs_bubble_3d_n32_part (32^3, two levels, regrid_int = 2, a 4 x 4 x 4
lattice, particle_int = 2, chk_int = 3) writes part00000 .. part00006 and a Particles file inside every checkpoint; restarted from chk00003 it ends with the same
particle bits and the same part00006 bytes; varden_main (varden_amd/fortran/varden_main.f90), started from the same checkpoint, writes part* files byte-identical to
inputs.run's (a fresh start would hand the library initial states that differ in the last bit: each host forms initdata's tanh with its own mathematical library,
tests/test_diagnostics_fortran_gpu.py); without the keys neither host writes any such file."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "varden_amd", "fortran", "varden_main")
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_3d_n32_part")


def variant(**kw):
    t = open(INPUTS).read()
    for k, v in kw.items():
        t, n = re.subn(r"(?mi)^(\s*%s\s*=\s*)[^!\n]*" % re.escape(k), lambda m: m.group(1) + str(v) + " ", t)
        if n == 0:
            t = re.sub(r"(?m)^\s*/\s*$", " %s = %s\n/" % (k, v), t, count=1)
    return t


def _main(text, cwd):
    if not os.path.exists(MAIN):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(MAIN)])
    with open(os.path.join(cwd, "inputs"), "w") as f:
        f.write(text)
    out = subprocess.run([MAIN, "inputs"], cwd=cwd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def test_inputs_file_restart_and_fortran_host(gpu, tmp_path):
    from varden_amd import advance as adv
    from varden_amd import inputs
    full, again, fo = tmp_path / "full", tmp_path / "again", tmp_path / "fo"
    for d in (full, again, fo):
        d.mkdir()
    text = open(INPUTS).read()
    nl, G = inputs.run(text, report=None, outdir=str(full))
    assert G.istep == 6 and G.particles.n == 64 and G.particles.active == 64 and G.nregrids >= 3
    x_full = G.particles.positions().view(np.uint64).copy()
    G.close()
    names = sorted(os.listdir(str(full)))
    assert names == ["chk00000", "chk00003", "chk00006", "part00000", "part00002", "part00004", "part00006"], names
    for chk in ("chk00000", "chk00003", "chk00006"):
        assert sorted(os.listdir(str(full / chk))) == sorted(["Header", "Particles", "Pressure", "State"]), os.listdir(str(full / chk))
    # the file: the lattice at the start, the columns, finite values; the particles have moved by step 6
    P0, t0, c0 = adv.Particles.read(str(full / "part00000"))
    assert t0 == 0.0 and list(c0) == ["vel1", "vel2", "vel3", "s1", "s2"]
    assert np.array_equal(P0.positions(), adv.particle_lattice((4, 4, 4), (1.0, 1.0, 1.0)))
    P6, t6, c6 = adv.Particles.read(str(full / "part00006"))
    assert t6 > 0.0 and np.array_equal(P6.positions().view(np.uint64), x_full) and all(np.isfinite(v).all() for v in c6.values())
    assert np.abs(P6.positions() - P0.positions()).max() > 0.0 and (c6["s1"] > 0.99).all() and (c6["s1"] < 10.01).all()      # (the bubble's density, 1 .. 10)
    PC, tc, cc = adv.Particles.read(str(full / "chk00006" / "Particles"))
    assert tc == t6 and cc == {} and np.array_equal(PC.positions().view(np.uint64), x_full)
    for p in (P0, P6, PC):
        p.destroy()
    # restarted from chk00003: the same particle bits, the same bytes
    for d in (again, fo):
        shutil.copytree(str(full / "chk00003"), str(d / "chk00003"))
    rtext = variant(restart=3)
    nl, G = inputs.run(rtext, report=None, outdir=str(again))
    assert G.istep == 6 and np.array_equal(G.particles.positions().view(np.uint64), x_full)
    G.close()
    assert sorted(os.listdir(str(again))) == ["chk00003", "chk00006", "part00004", "part00006"]
    for name in ("part00004", "part00006", os.path.join("chk00006", "Particles")):
        assert open(str(full / name), "rb").read() == open(str(again / name), "rb").read(), name
    # the Fortran host from the same checkpoint: the same files
    _main(rtext, str(fo))
    assert sorted(os.listdir(str(fo))) == ["chk00003", "chk00006", "inputs", "part00004", "part00006"]
    for name in ("part00004", "part00006", os.path.join("chk00006", "Particles")):
        assert open(str(full / name), "rb").read() == open(str(fo / name), "rb").read(), name
    # a checkpoint without a Particles file restarts a run without particles
    os.remove(str(again / "chk00003" / "Particles"))
    for f in ("part00004", "part00006"):
        os.remove(str(again / f))
    shutil.rmtree(str(again / "chk00006"))
    nl, G = inputs.run(rtext, report=None, outdir=str(again))
    assert G.particles is None and sorted(os.listdir(str(again))) == ["chk00003", "chk00006"]
    assert sorted(os.listdir(str(again / "chk00006"))) == ["Header", "Pressure", "State"]
    G.close()


def test_fresh_fortran_run_and_no_keys_no_files(gpu, tmp_path):
    """a fresh varden_main run writes the same set of files with the same lattice; without the keys both hosts write no particle file and the checkpoint holds
    what it held"""
    from varden_amd import advance as adv
    from varden_amd import inputs
    on, off, pyoff = tmp_path / "on", tmp_path / "off", tmp_path / "pyoff"
    for d in (on, off, pyoff):
        d.mkdir()
    out_on = _main(variant(max_step=2, chk_int=2), str(on))
    assert sorted(os.listdir(str(on))) == ["chk00000", "chk00002", "inputs", "part00000", "part00002"]
    P0, t0, c0 = adv.Particles.read(str(on / "part00000"))
    assert t0 == 0.0 and list(c0) == ["vel1", "vel2", "vel3", "s1", "s2"] and np.array_equal(P0.positions(), adv.particle_lattice((4, 4, 4), (1.0, 1.0, 1.0)))
    P0.destroy()
    none = {"particle_lattice(1)": 0, "particle_lattice(2)": 0, "particle_lattice(3)": 0}
    out_off = _main(variant(max_step=2, chk_int=2, **none), str(off))
    assert sorted(os.listdir(str(off))) == ["chk00000", "chk00002", "inputs"]
    assert sorted(os.listdir(str(off / "chk00002"))) == ["Header", "Pressure", "State"]
    assert out_on == out_off                                     # the fields of the run do not know about the particles
    nl, G = inputs.run(variant(max_step=2, chk_int=2, **none), report=None, outdir=str(pyoff))
    assert G.particles is None and sorted(os.listdir(str(pyoff))) == ["chk00000", "chk00002"]
    G.close()
    # the command line's --particles / --particle-int over the namelist
    nl, G = inputs.run(variant(max_step=2, chk_int=0, **none), report=None, outdir=str(pyoff), particles=(2, 3, 1), particle_int=1)
    assert G.particles.n == 6 and sorted(f for f in os.listdir(str(pyoff)) if f.startswith("part")) == ["part00000", "part00001", "part00002"]
    G.close()
