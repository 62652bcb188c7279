"""Run diagnostics on the device (vdn_diagnostics, varden_amd/csrc/diag.hip) against numpy over to_numpy() of the same multifabs, the composite mask built in numpy
from the box lists (tests/_diagnostics_worker.py: reference).  Sums agree to the rounding bound of adding their terms in another order, ncells * 2^-53 * sum |term|
(derived, not measured); counts, nonfinite and every extremum agree exactly, bit for bit (-0 below +0)."""
import os
import re

import numpy as np
import pytest

from tests._diagnostics_worker import CASES, FIELDS, SUMS, WALLS, Hier, all_bits, bits, reference
from tests.children import launch_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INOUT = [[11, 12], [14, 14], [15, 15]]          # inflow / outflow along x, slip and no-slip walls (tests/test_tag_criteria_gpu.py: BC3["inout"])


def _pkg():
    import varden_amd
    from varden_amd import advance, boxlib, capi  # noqa: F401
    return varden_amd


def check(got, ref, bound, what=""):
    """every figure of a diagnostics dict against the reference: sums within their bound, everything else exactly"""
    for name in FIELDS:
        g, r = got[name], ref[name]
        gl, rl = (g, r) if isinstance(g, list) else ([g], [r])
        assert len(gl) == len(rl), (what, name, g, r)
        for i, (x, y) in enumerate(zip(gl, rl)):
            if name in SUMS:
                b = bound[name][i] if isinstance(bound[name], list) else bound[name]
                print("%s %s[%d]: device %.17e numpy %.17e |diff| %.3e bound %.3e" % (what, name, i, x, y, abs(x - y), b))
                assert abs(x - y) <= b, (what, name, i, x, y, abs(x - y), b)
            elif name in ("cells", "cells_lev", "nonfinite"):
                assert x == y, (what, name, i, x, y)
            else:
                assert bits(x) == bits(y), (what, name, i, x, y)


def vorticity(H):
    """vdn_make_vorticity of every level (it fills the same-level and physical ghost cells of u, which the diagnostics then read), gathered"""
    from varden_amd import advance as adv
    W = []
    for l in range(H.nlev):
        w = H.bl.MultiFab(H.mla, l, 1, 0)
        adv.make_vorticity(w, 0, H.u[l], H.dx[l], H.bct)
        W.append(w)
    out = H.gather(W)
    for w in W:
        w.destroy()
    return out


ONE_LEVEL = {"one-box-two-slabs": ((48, 48, 40), [((0, 0, 0), (47, 47, 39))]),
             "four-boxes": ((40, 24, 28), [((20 * i, 12 * j, 0), (20 * i + 19, 12 * j + 11, 27)) for j in range(2) for i in range(2)])}


@pytest.mark.parametrize("nscal", [1, 2, 4, 11])
@pytest.mark.parametrize("grid", sorted(ONE_LEVEL))
def test_one_level(gpu, grid, nscal):
    """random fields with negative values, a -0.0 that is a minimum and a +0.0 that is a maximum; every ghost cell NaN: without the vorticity terms no ghost cell is read"""
    n, boxes = ONE_LEVEL[grid]
    H = Hier(_pkg(), n, [boxes], nscal=nscal, seed=nscal, nan_ghosts=True)
    try:
        d = H.diagnostics(vort=False)
        R, B = reference(H, H.gather(H.u), H.gather(H.s))
        assert d["nonfinite"] == 0 and all(np.isfinite(x) for name in FIELDS for x in (d[name] if isinstance(d[name], list) else [d[name]]))
        assert d["cells"] == n[0] * n[1] * n[2] and abs(d["volume"] - 1.0) <= B["volume"]
        assert bits(d["s_min"][nscal - 1]) == bits(-0.0) and bits(d["u_max"][1]) == bits(0.0)
        assert d["enstrophy"] == 0.0 and d["vort_min"] == 0.0 and d["vort_max"] == 0.0
        check(d, R, B, grid)
    finally:
        H.close()


@pytest.mark.parametrize("case", ["amr2", "amr3"])
def test_hierarchies(gpu, case):
    """two and three levels: the composite grid (a fine box on the domain wall, one on the edge between two coarse boxes), volume, cells per level, every integral and
    extremum with the vorticity terms; a NaN under a fine box changes nothing, the same NaN in an uncovered cell is counted once"""
    nbase, boxes = CASES[case]
    H = Hier(_pkg(), nbase, boxes, nscal=3, seed=3, ng_u=2, ng_s=0)
    try:
        W = vorticity(H)
        d = H.diagnostics(vort=True)
        R, B = reference(H, H.gather(H.u), H.gather(H.s), W)
        assert d["cells_lev"] == R["cells_lev"] and all(0 < c for c in d["cells_lev"]) and d["cells_lev"][0] < nbase ** 3
        assert abs(d["volume"] - 1.0) <= B["volume"]
        check(d, R, B, case)
        d0 = H.diagnostics(vort=False)
        # a NaN in the coarse cell under the first fine box's low corner; then in the level's first cell, which nothing covers
        flo = boxes[1][0][0]
        covered, free = tuple(x // 2 for x in flo), (0, 0, 0)
        for cell, expect in ((covered, 0), (free, 1)):
            for i in range(H.s[0].nfabs()):
                lo, hi = H.s[0].get_box(i)
                if all(lo[k] <= cell[k] <= hi[k] for k in range(3)):
                    a = H.s[0].to_numpy(i)
                    keep = a.copy()
                    a[cell[0] - lo[0], cell[1] - lo[1], cell[2] - lo[2], 1] = np.nan
                    H.s[0].from_numpy(a, i)
                    d1 = H.diagnostics(vort=False)
                    H.s[0].from_numpy(keep, i)
                    if expect == 0:
                        assert np.array_equal(all_bits(d1), all_bits(d0)), "a NaN in a covered cell changed the figures"
                    else:
                        assert d1["nonfinite"] == 1 and d1["cells"] == d0["cells"] and np.isnan(d1["sum_s"][1]) and d1["sum_s"][0] == d0["sum_s"][0]
                    break
            else:
                raise AssertionError("no box holds the cell")
    finally:
        H.close()


@pytest.mark.parametrize("dm,phys", [(3, WALLS), (3, INOUT), (2, [[15, 15], [15, 15]]), (2, [[11, 12], [14, 15]])])
def test_vorticity_terms(gpu, dm, phys):
    """enstrophy, vort_min and vort_max against vdn_make_vorticity's own output (held to the reference's makevort elsewhere), masked and summed in numpy: one-sided forms
    at walls and inflow faces, several boxes; dm = 2: the signed vorticity"""
    n, boxes = ((24, 20, 16), [((12 * i, 0, 8 * k), (12 * i + 11, 19, 8 * k + 7)) for k in range(2) for i in range(2)]) if dm == 3 else \
               ((40, 24), [((20 * i, 0, 0), (20 * i + 19, 23, 0)) for i in range(2)])
    H = Hier(_pkg(), n, [boxes], phys=phys, nscal=2, dm=dm, seed=5 + dm, plant_zeros=False)
    try:
        W = vorticity(H)
        d = H.diagnostics(vort=True)
        R, B = reference(H, H.gather(H.u), H.gather(H.s), W)
        assert d["enstrophy"] > 0.0 and d["vort_max"] > 0.0
        assert (d["vort_min"] < 0.0) if dm == 2 else (d["vort_min"] >= 0.0)
        assert abs(d["volume"] - (1.0 if dm == 3 else 2.0)) <= B["volume"]
        check(d, R, B, "dm=%d" % dm)
    finally:
        H.close()


def test_two_calls_give_the_same_bits(gpu):
    nbase, boxes = CASES["amr2"]
    H = Hier(_pkg(), nbase, boxes, nscal=11, seed=9)
    try:
        a, b = H.diagnostics(vort=True), H.diagnostics(vort=True)
        assert np.array_equal(all_bits(a), all_bits(b))
        assert a["nonfinite"] == 0 and a["cells"] > 0
    finally:
        H.close()


def test_ranks_give_identical_bits(gpu, tmp_path):
    """one rank against two and eight (the RCCL test double, rank threads in child processes): every rank gets the same bits, and they do not depend on the number of
    ranks -- the partials of a slab live in the slot of its GLOBAL number and are added in that order everywhere"""
    out = {}
    for nranks, per_proc in ((1, 1), (2, 1), (8, 2)):
        out[nranks] = launch_ranks("_diagnostics_worker.py", nranks, tmp_path, "diag%d" % nranks, ["amr3"], per_proc=per_proc, agree=("bits", "again", "novort"), timeout=300)
    for nranks in (1, 2, 8):
        assert np.array_equal(out[nranks]["bits"], out[nranks]["again"]), nranks
        for key in ("bits", "novort"):
            assert np.array_equal(out[nranks][key], out[1][key]), (nranks, key, out[nranks][key], out[1][key])
    assert out[1]["bits"][0] > 0


def test_mass_drift_after_real_steps(gpu):
    """the 32^3 bubble, one level, walls, three steps: the drift of the mass the library reports equals numpy's drift of the same fields within the bound of the two sums.
    (The drift itself is recorded in DESIGN.md section 20; no fixed number is asserted.)"""
    from varden_amd import driver
    from varden_amd.capi import default_params
    G = driver.Varden(32, WALLS, default_params(cflfac=0.9), prob_type=1, grav=-9.8, init_shrink=0.1, init_iter=1)
    try:
        def both():
            d = G.diagnostics()
            rho = G.sold[0].to_numpy()[3:-3, 3:-3, 3:-3, 0]
            terms = rho.ravel() * float(np.prod(G.dx[0]))
            import math
            return d, math.fsum(terms), rho.size * 2.0 ** -53 * math.fsum(np.abs(terms))
        d0, m0, b0 = both()
        for _ in range(3):
            G.step()
        d1, m1, b1 = both()
        drift, ref = d1["sum_s"][0] - d0["sum_s"][0], m1 - m0
        print("mass %.17e -> %.17e: drift %.3e (numpy %.3e), relative %.3e; bound %.3e" % (d0["sum_s"][0], d1["sum_s"][0], drift, ref, drift / d0["sum_s"][0], b0 + b1))
        assert abs(drift - ref) <= b0 + b1
        assert d1["nonfinite"] == 0 and d1["cells"] == 32 ** 3 and d1["kinetic"] > 0.0 and d1["s_min"][0] > 0.0
    finally:
        G.close()


def test_refusals(gpu):
    import ctypes as C
    from varden_amd import advance as adv
    from varden_amd import capi
    from varden_amd.boxlib import handle_array
    lib = capi.load()
    nbase, boxes = CASES["amr2"]
    H = Hier(_pkg(), nbase, boxes, nscal=2, seed=1)
    out = capi.Diag()
    dx = (C.c_double * 12)(*([1.0 / 16] * 12))

    def call(nlev, u, s, dxp, bct, what):
        rc = lib.vdn_diagnostics(nlev, H.mla.h, handle_array(u), handle_array(s), dxp, bct, what, C.byref(out))
        return rc, (lib.vdn_last_error() or b"").decode()
    try:
        other = H.bl.MLLayout([((0, 0, 0), (15, 15, 15))], [[((0, 0, 0), (15, 15, 15))]])
        s_other = H.bl.MultiFab(other, 0, 2, 0)
        u_nog = [H.bl.MultiFab(H.mla, l, 3, 0) for l in range(2)]
        four = H.u + H.u
        for args, word in (((0, H.u, H.s, dx, H.bct.h, 0), "nlev"), ((5, four + H.u[:1], four + H.s[:1], dx, H.bct.h, 0), "nlev"),
                           ((1, H.u, H.s, dx, H.bct.h, 0), "does not match"),
                           ((2, H.u, [s_other, H.s[1]], dx, H.bct.h, 0), "layouts of u and s differ"),
                           ((2, H.u, H.s, dx, None, capi.DIAG_VORT), "bct"), ((2, H.u, H.s, None, H.bct.h, capi.DIAG_VORT), "dx"),
                           ((2, u_nog, H.s, dx, H.bct.h, capi.DIAG_VORT), "ghost")):
            rc, msg = call(*args)
            assert rc != 0 and word in msg, (args[0], word, rc, msg)
        rc, msg = call(2, H.u, H.s, dx, None, 0)            # without the vorticity terms the tower is not needed
        assert rc == 0, msg
        with pytest.raises(capi.VardenError, match="bct"):
            adv.diagnostics(H.mla, H.u, H.s, H.dx, None, vort=True)
        for m in u_nog + [s_other]:
            m.destroy()
        other.destroy()
    finally:
        H.close()
    # dm = 2 runs on one level
    H2 = Hier(_pkg(), (16, 16), [[((0, 0, 0), (15, 15, 0))]], phys=[[15, 15], [15, 15]], dm=2, nscal=2)
    try:
        two = H2.bl.MLLayout([((0, 0, 0), (15, 15, 0)), ((0, 0, 0), (31, 31, 0))], [[((0, 0, 0), (15, 15, 0))], [((8, 8, 0), (23, 23, 0))]], rr=[(2, 2, 1)])
        u2 = [H2.bl.MultiFab(two, l, 2, 1) for l in range(2)]
        s2 = [H2.bl.MultiFab(two, l, 2, 1) for l in range(2)]
        rc = lib.vdn_diagnostics(2, two.h, handle_array(u2), handle_array(s2), dx, None, 0, C.byref(out))
        assert rc != 0 and b"dm = 2" in lib.vdn_last_error(), lib.vdn_last_error()
        for m in u2 + s2:
            m.destroy()
        two.destroy()
    finally:
        H2.close()


def test_diagnostics_file_of_an_adaptive_run(gpu, tmp_path):
    """inputs.run on the adaptive vortex tube (two levels, regrid every second step) with diag_int = 1, four steps: a header and five lines; the volume never changes;
    `cells` changes from one line to the next exactly when the box lists did; the last line holds the figures of a fresh G.diagnostics(), digit for digit.
    Measured on this input: the regrids of steps 1 and 3 return the grids they started from -- the tube is uniform along x and four steps move nothing across a
    blocking unit --, every line reads 90112 cells; test_cells_follow_a_regrid below shows cells changing with the grids at constant volume."""
    from varden_amd import advance as adv
    from varden_amd import inputs
    text = open(os.path.join(ROOT, "tests", "golden", "inputs", "inputs_vortextube_3d_amr")).read()
    text = re.sub(r"(?m)^\s*/\s*$", " diag_int = 1\n/", text, count=1)
    grids = []
    nl, G = inputs.run(text, nsteps=4, report=lambda g: grids.append([list(b) for b in g.boxes]), outdir=str(tmp_path))
    try:
        lines = open(str(tmp_path / "varden_diag.out")).read().splitlines()
        assert lines[0].startswith("#") and lines[0] == inputs.diag_header(2, 3).rstrip("\n") and len(lines) == 6
        rows = [ln.split() for ln in lines[1:]]
        cols = ["step", "time", "dt"] + adv.diag_columns(2, 3)
        assert all(len(r) == len(cols) for r in rows) and [int(r[0]) for r in rows] == [0, 1, 2, 3, 4]
        cells, volume = [int(r[cols.index("cells")]) for r in rows], [float(r[cols.index("volume")]) for r in rows]
        print("cells per line:", cells, "regrids:", G.nregrids)
        assert G.nregrids == 2 and len(grids) == 4
        for k in range(1, 4):                       # lines of steps k and k + 1
            assert (cells[k] != cells[k + 1]) == (grids[k - 1] != grids[k]), (k, cells, [len(b) for g in grids for b in g])
        assert all(abs(v - 1.0) <= c * 2.0 ** -53 for v, c in zip(volume, cells)), volume
        assert all(int(r[cols.index("nonfinite")]) == 0 for r in rows)
        assert lines[-1] + "\n" == inputs.diag_line(G.istep, G.time, G.dt, G.diagnostics())
    finally:
        G.close()


def test_cells_follow_a_regrid(gpu):
    """the same hierarchy regridded with a wider buffer: other boxes on level 1, so other cell counts on both levels, and the same volume"""
    from varden_amd import inputs
    text = open(os.path.join(ROOT, "tests", "golden", "inputs", "inputs_vortextube_3d_amr")).read()
    nl, G = inputs.build(text)
    try:
        before, a = [list(b) for b in G.boxes], G.diagnostics()
        G.regrid(buf_wid=G.amr_buf_width + 4)
        after, b = [list(b) for b in G.boxes], G.diagnostics()
        assert before[0] == after[0] and before[1] != after[1]
        assert b["cells_lev"][1] > a["cells_lev"][1] and b["cells_lev"][0] < a["cells_lev"][0] and b["cells"] > a["cells"]
        for d in (a, b):
            assert abs(d["volume"] - 1.0) <= d["cells"] * 2.0 ** -53 and d["nonfinite"] == 0
            assert abs(sum(d["volume_lev"]) - 1.0) <= d["cells"] * 2.0 ** -53
    finally:
        G.close()
