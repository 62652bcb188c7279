"""Isosurfaces on the device (vdn_isosurface, varden_amd/csrc/iso.hip, iso_cell.h) against the numpy float64 restatement of the definitions of include/varden_amd.h
(tests/_isosurface_worker.py: restate, which takes the orientation of a triangle from the rule, not from the library's table).  The grids are those of
tests/_profiles_worker.py; spacings differ per direction and are powers of two; the test writes every valid and ghost cell of the field itself -- the call fills nothing
--; the fields are seeded random multiples of 1/8, so nodes equal iso somewhere.  Triangle coordinates agree bit for bit in output order, the counts exactly, the sums
with sums formed in numpy.longdouble to (n + c) 2^-53 sum |term| (derived in the worker, not measured)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests._isosurface_worker import (INLET_X, NFIG, PERIODIC_Y, WALLS, WRITTEN, all_bits, check, hier, isosurface, node_values, random_field, rank_figures, restate,
                                      sum_bound, wide_sum, write_field)
from tests._profiles_worker import AMR3, ONE_LEVEL
from tests.children import launch_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_3d_n32_iso")
GRIDS = {"one-box": (ONE_LEVEL["one-box"][0], [ONE_LEVEL["one-box"][1]]), "six-boxes": (ONE_LEVEL["six-boxes"][0], [ONE_LEVEL["six-boxes"][1]]), "amr3": AMR3}
ISO = 0.125          # a multiple of 1/64: some nodes of the random fields equal it


def _pkg():
    import varden_amd
    from varden_amd import advance, boxlib, capi  # noqa: F401
    return varden_amd


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_against_numpy(gpu, grid):
    """one box none of whose extents is a multiple of the wave width, six boxes (the surface passes their boundaries), three levels (it passes coarse-fine boundaries):
    counts, every triangle bit for bit in output order, the sums; no face value anywhere (walls, a scalar's boundary component)"""
    n, boxes = GRIDS[grid]
    H = hier(_pkg(), n, boxes, seed=2)
    try:
        A = random_field(H, 11)
        write_field(H, A)
        N = node_values(A[0], [False] * 3, [False] * 3)
        assert (N == ISO).any() and (N > ISO).any() and (N < ISO).any()
        R = restate(H, A, ISO)
        I = isosurface(H, ISO)
        worst = check(I, R, grid)
        assert I.ntri > 1000 and I.nonfinite_cells == 0 and all(v > 0 for v in I.ntri_lev) and len(I.ntri_lev) == H.nlev
        D = H.pkg.advance.diagnostics(H.mla, H.u, H.s, H.dx, None, vort=False)
        assert I.volume == D["volume"], (I.volume, D["volume"])
        print("%s: %d triangles in %d cut cells; the largest |device - numpy| / bound = %.3f" % (grid, I.ntri, I.cut_cells, worst))
        # the counts alone: the same figures, no triangle
        J = isosurface(H, ISO, triangles=False)
        want = all_bits(I)[:NFIG].copy()
        want[WRITTEN] = 0
        assert J.tri is None and J.written == 0 and np.array_equal(all_bits(J), want)
    finally:
        H.close()


@pytest.mark.parametrize("case", ["inlet", "inlet-other-component", "periodic", "walls-velocity"])
def test_boundaries(gpu, case):
    """the face-value rule for the component asked for alone: an inlet at x = 0 gives scalar 0 (boundary component 3) a value ON the face and the pressure's component
    (5) none, the outlet at the other end gives the pressure's one and the scalar none; a periodic pair; no-slip walls give a velocity's component (0) a face value on
    all six faces -- on the six boxes, so the rule meets box boundaries too"""
    phys, bccomp, per = dict(inlet=(INLET_X, 3, ()), periodic=(PERIODIC_Y, 3, (1,)), walls=(WALLS, 0, ()))[case.split("-")[0]]
    if case == "inlet-other-component":
        bccomp = 5
    n, boxes = GRIDS["six-boxes"]
    H = hier(_pkg(), n, boxes, seed=3, phys=phys)
    try:
        A = random_field(H, 13, periodic=per)
        write_field(H, A)
        R = restate(H, A, ISO, bccomp=bccomp, phys=phys)
        I = isosurface(H, ISO, bccomp=bccomp)
        check(I, R, case)
        plain = restate(H, A, ISO, bccomp=5, phys=WALLS)           # no face value anywhere
        if case == "periodic":
            assert np.array_equal(R["tri"].view(np.uint64), plain["tri"].view(np.uint64))
        else:
            assert not np.array_equal(R["tri"], plain["tri"]), "the face values change the surface"
    finally:
        H.close()


def _plane_field(H):
    """q = z - (1/8 + x / 8 + y / 16) at the cell centres of every level's grown domain: exact in binary, so every node mean is the plane's value at the node"""
    A = []
    for l in range(H.nlev):
        c = [(np.arange(-1, H.n[l][d] + 1) + 0.5) * H.dx[l][d] for d in range(3)]
        X, Y, Z = np.meshgrid(*c, indexing="ij")
        A.append(Z - (0.125 + 0.125 * X + 0.0625 * Y))
    return A


def test_plane(gpu):
    """an oblique plane through the 2 x 4 x 1 domain, above every cell's floor and below its ceiling: marching tetrahedra are exact for it.  The area is the analytic section,
    the volume the analytic cut, on one level and on three, and the area of the hierarchy is that of the one level.  Bound: (n + c) 2^-53 sum |term| with c the roundings
    of a term weighted by how far a difference of coordinates magnifies them: a coordinate carries 4 roundings (quotient, product, sum, the node's own position is
    exact) of relative size 2^-53 |x| <= 2^-53 L_d, an edge is a difference of two of them over a length >= the finest dx_d -- L_d / dx_d = 64 on the finest level for
    every d --, nine coordinates per triangle, then 21 roundings of the cross product, the norm and the half: c = 9 * 4 * 64 + 21"""
    Lx, Ly, Lz = 2.0, 4.0, 1.0
    area = Lx * Ly * math.sqrt(1.0 + 0.125 ** 2 + 0.0625 ** 2)
    above = Lx * Ly * (Lz - 0.125 - 0.125 * Lx / 2 - 0.0625 * Ly / 2)
    c = 9 * 4 * 64 + 21
    got = {}
    for name, (n, boxes) in (("one-level", (16, [[((0, 0, 0), (15, 15, 15))]])), ("amr3", AMR3)):
        H = hier(_pkg(), n, boxes, seed=4)
        try:
            A = _plane_field(H)
            write_field(H, A)
            I = isosurface(H, 0.0)
            R = restate(H, A, 0.0)
            check(I, R, "plane " + name)
            # a tetrahedron's volume term: at most four factors 1 - t or t, each with the quotient's rounding and its own, and four products and sums: 12
            ba, bv = sum_bound(I.ntri, area, c), sum_bound(len(R["vol_terms"]), above, 12)
            print("plane %s: area %.17e analytic %.17e |diff| %.3e bound %.3e; above %.17e analytic %.17e |diff| %.3e bound %.3e; %d triangles" % (
                name, I.area, area, abs(I.area - area), ba, I.volume_above, above, abs(I.volume_above - above), bv, I.ntri))
            assert abs(I.area - area) <= ba and abs(I.volume_above - above) <= bv and I.volume == Lx * Ly * Lz
            # the area vector of a plane section: area * (-grad q) / |grad q|, grad q = (-1/8, -1/16, 1)
            for d, g in enumerate((-0.125, -0.0625, 1.0)):
                assert abs(I.area_vec[d] + Lx * Ly * g) <= ba, (d, I.area_vec[d])
            got[name] = (I.area, ba)
        finally:
            H.close()
    assert abs(got["amr3"][0] - got["one-level"][0]) <= got["amr3"][1] + got["one-level"][1]


def _sphere_field(n):
    x = (np.arange(-1, n + 1) + 0.5) / n
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    return 0.3 - np.sqrt((X - 0.5) ** 2 + (Y - 0.5) ** 2 + (Z - 0.5) ** 2)


def test_sphere(gpu):
    """q = 0.3 - |x - centre| in the unit cube, iso = 0: the restatement on a CPU gives 2520 triangles with relative errors -3.32e-2 (area) and -5.41e-2 (volume) at 16^3,
    10416 triangles with -8.23e-3 and -1.356e-2 at 32^3 -- second order, ratios 4.03 and 3.99.  The device reproduces the counts exactly (the assertion on ntri) and the errors to the summation
    bound: that is check() against the restatement, which forms them; the comparison with the table's own figures can only be held to the digits the table gives.  The
    surface is closed: |area_vec| <= the bound, and the divergence theorem holds -- the sum of p0 . (p1 x p2) / 6 over the triangles is volume_above --, on one
    box and on six unequal ones"""
    A0, V0 = 4.0 * math.pi * 0.09, 4.0 / 3.0 * math.pi * 0.027
    six = [((0, 0, 0), (19, 31, 7)), ((20, 0, 0), (31, 31, 7)), ((0, 0, 8), (19, 31, 19)), ((20, 0, 8), (31, 31, 19)), ((0, 0, 20), (19, 31, 31)), ((20, 0, 20), (31, 31, 31))]
    table = {16: (2520, -3.32e-2, -5.41e-2), 32: (10416, -8.23e-3, -1.356e-2)}
    err, bits = {}, {}
    for name, n, boxes in (("16", 16, [((0, 0, 0), (15, 15, 15))]), ("32", 32, [((0, 0, 0), (31, 31, 31))]), ("32 six boxes", 32, six)):
        H = hier(_pkg(), n, [boxes], dx0=(1.0 / n,) * 3, seed=5)
        try:
            A = [_sphere_field(n)]
            write_field(H, A)
            I = isosurface(H, 0.0)
            R = restate(H, A, 0.0)
            check(I, R, "sphere " + name)
            assert I.ntri == table[n][0] and I.volume == 1.0
            ea, ev = I.area / A0 - 1.0, I.volume_above / V0 - 1.0
            print("sphere %s: %d triangles, relative area error %.4e, relative volume error %.4e" % (name, I.ntri, ea, ev))
            assert abs(ea - table[n][1]) < 0.5e-4 and abs(ev - table[n][2]) < 0.5e-4          # the table's digits
            for d in range(3):
                assert abs(I.area_vec[d]) <= sum_bound(I.ntri, wide_sum(R["av_terms"][:, d])[1]), (name, d, I.area_vec[d])
            # the divergence theorem on the returned triangles; a term makes 9 + 5 + 1 roundings (cross product, dot product, the sixth)
            T = I.tri.astype(np.longdouble)
            terms = (T[:, 0] * np.cross(T[:, 1], T[:, 2])).sum(axis=1) / 6
            total, ab = terms.sum(), np.abs(terms).sum()
            bound = sum_bound(I.ntri, ab, 15) + sum_bound(len(R["vol_terms"]), I.volume_above)
            print("sphere %s: divergence theorem %.17e volume_above %.17e |diff| %.3e bound %.3e" % (name, float(total), I.volume_above, abs(float(total) - I.volume_above), bound))
            assert abs(float(total - np.longdouble(I.volume_above))) <= bound
            err[name], bits[name] = (ea, ev), I
        finally:
            H.close()
    ra, rv = err["16"][0] / err["32"][0], err["16"][1] / err["32"][1]
    print("sphere: convergence ratios %.3f (area) %.3f (volume)" % (ra, rv))
    assert 3.5 <= ra <= 4.5 and 3.5 <= rv <= 4.5
    # cutting the level into boxes changes the order of the triangles and of the sums, not the surface
    a, b = bits["32"], bits["32 six boxes"]
    assert a.ntri == b.ntri and abs(a.area - b.area) <= 2 * sum_bound(a.ntri, a.area)
    key = lambda I: np.sort(np.ascontiguousarray(I.tri).view(np.uint64).reshape(-1, 9).view([("", np.uint64)] * 9).ravel())      # noqa: E731
    assert np.array_equal(key(a), key(b))


def test_edges(gpu):
    """iso above the maximum, below the minimum, a planted NaN, a buffer one triangle too small, no buffer"""
    from varden_amd import capi
    from varden_amd.boxlib import handle_array
    H = hier(_pkg(), AMR3[0], AMR3[1], seed=6)
    try:
        A = random_field(H, 17)
        write_field(H, A)
        hi = isosurface(H, 1.5)
        assert hi.ntri == 0 and hi.cut_cells == 0 and hi.volume_above == 0.0 and hi.area == 0.0 and hi.tri.shape == (0, 3, 3) and hi.written == 0
        lo = isosurface(H, -1.5)
        ncell = 16 ** 3 + (12 * 16 * 12 + 8 * 8 * 16) * 7 // 8 + 16 * 24 * 16 * 7 // 8
        assert lo.ntri == 0 and lo.volume == 8.0 and abs(lo.volume_above - lo.volume) <= sum_bound(6 * ncell, lo.volume)
        check(lo, restate(H, A, -1.5), "below the minimum")
        first = isosurface(H, ISO)
        # a NaN in a composite cell of level 1 away from every boundary: the 27 cells around it see it, nothing else changes
        M = H.composite()
        c = (23, 11, 24)
        assert M[1][c[0] - 1:c[0] + 2, c[1] - 1:c[1] + 2, c[2] - 1:c[2] + 2].all()
        B = [a.copy() for a in A]
        B[1][c[0] + 1, c[1] + 1, c[2] + 1] = np.nan
        write_field(H, B)
        I = isosurface(H, ISO)
        R = restate(H, B, ISO)
        check(I, R, "a planted NaN")
        assert I.nonfinite_cells == 27 and I.volume == 8.0 - 27 * float(np.prod(H.dx[1])) and I.ntri_lev[0] == first.ntri_lev[0] and I.ntri_lev[2] == first.ntri_lev[2]
        clean = restate(H, A, ISO)
        sees = np.isin(clean["cell_of"], np.setdiff1d(clean["cell_of"], R["cell_of"]))          # (the cells that lost their triangles)
        assert np.array_equal(I.tri.view(np.uint64), first.tri[~sees].view(np.uint64)) and 0 < sees.sum() == first.ntri - I.ntri
        write_field(H, A)
        # max_tri = ntri - 1: nothing is written, the buffer is untouched, the sums are the same bits
        lib, out = capi.load(), capi.Iso()
        n = first.ntri
        tri, lev = np.full((n, 3, 3), -7.0), np.full(n, 9, dtype=np.uint8)
        dx = (C.c_double * 9)(*[v for l in H.dx for v in l])
        args = (3, H.mla.h, handle_array(H.s), 0, 3, dx, H.bct.h, ISO)
        pt, pl = tri.ctypes.data_as(C.POINTER(C.c_double)), lev.ctypes.data_as(C.POINTER(C.c_ubyte))
        assert lib.vdn_isosurface(*args, n - 1, pt, pl, C.byref(out)) == 0
        assert out.written == 0 and out.ntri == n and (tri == -7.0).all() and (lev == 9).all()
        assert out.area == first.area and out.volume_above == first.volume_above and list(out.area_vec) == first.area_vec
        # the exact size, without the levels
        assert lib.vdn_isosurface(*args, n, pt, None, C.byref(out)) == 0 and out.written == n and np.array_equal(tri, first.tri) and (lev == 9).all()
        # no buffer: counts and sums alone
        assert lib.vdn_isosurface(*args, 0, None, None, C.byref(out)) == 0 and out.written == 0 and out.ntri == n and out.area == first.area
    finally:
        H.close()


def test_both_forms_of_pass_two_give_the_same_bits(gpu):
    """vdn_isosurface_timed: pass 2 recomputing every cell (form 0) and pass 2 reading the counts pass 1 stored (form 1) write the triangles and figures of
    vdn_isosurface, bit for bit, on three levels with covered cells, face values and a planted NaN; the times are those of passes that ran; a form that does not exist
    and a NULL ms are refused"""
    from varden_amd import capi
    from varden_amd.boxlib import handle_array
    lib = capi.load()
    H = hier(_pkg(), AMR3[0], AMR3[1], seed=9)
    try:
        A = random_field(H, 23)
        A[1][24, 12, 25] = np.nan
        write_field(H, A)
        first = isosurface(H, ISO, bccomp=0)
        check(first, restate(H, A, ISO, bccomp=0), "forms")
        n = first.ntri
        dx = (C.c_double * 9)(*[v for l in H.dx for v in l])
        args = (3, H.mla.h, handle_array(H.s), 0, 0, dx, H.bct.h, ISO)
        for form in (0, 1):
            tri, lev, out, ms = np.full((n, 3, 3), -7.0), np.full(n, 9, dtype=np.uint8), capi.Iso(), (C.c_double * 2)(-1.0, -1.0)
            pt, pl = tri.ctypes.data_as(C.POINTER(C.c_double)), lev.ctypes.data_as(C.POINTER(C.c_ubyte))
            assert lib.vdn_isosurface_timed(*args, n, pt, pl, C.byref(out), form, ms) == 0, lib.vdn_last_error()
            assert out.written == n and np.array_equal(tri.view(np.uint64), first.tri.view(np.uint64)) and np.array_equal(lev, first.level), form
            assert out.area == first.area and out.volume_above == first.volume_above and list(out.area_vec) == first.area_vec and out.nonfinite_cells == 27, form
            assert ms[0] > 0.0 and ms[1] > 0.0, (form, ms[0], ms[1])
            # too small a buffer: pass 2 does not run, whatever pass 1 stored
            assert lib.vdn_isosurface_timed(*args, n - 1, pt, pl, C.byref(out), form, ms) == 0 and out.written == 0 and ms[0] > 0.0 and ms[1] == 0.0, form
            assert lib.vdn_isosurface_timed(*args, 0, None, None, C.byref(out), form, ms) == 0 and out.ntri == n and ms[1] == 0.0, form
        ms = (C.c_double * 2)()
        assert lib.vdn_isosurface_timed(*args, 0, None, None, C.byref(out), 2, ms) != 0 and lib.vdn_last_error().startswith(b"vdn_isosurface_timed: form")
        assert lib.vdn_isosurface_timed(*args, 0, None, None, C.byref(out), 0, None) != 0 and b"ms" in lib.vdn_last_error()
        assert np.array_equal(all_bits(isosurface(H, ISO, bccomp=0)), all_bits(first))
    finally:
        H.close()


def test_two_calls_give_the_same_bits(gpu):
    H = hier(_pkg(), AMR3[0], AMR3[1], seed=7)
    try:
        out = rank_figures(H)
        assert np.array_equal(out["iso"], out["again"]) and out["iso"].size > NFIG + 10 * 1000
    finally:
        H.close()


def test_ranks_give_identical_bits(gpu, tmp_path):
    """one rank against two and four (the RCCL test double, rank threads in child processes) on the three-level hierarchy: every rank gets the same bits in every count,
    sum and triangle, and they do not depend on the number of ranks -- a slab's partials and its triangles' places live under its GLOBAL number"""
    out = {}
    for nranks, per_proc in ((1, 1), (2, 1), (4, 2)):
        out[nranks] = launch_ranks("_isosurface_worker.py", nranks, tmp_path, "iso%d" % nranks, [], per_proc=per_proc, agree=("iso", "again", "counts"), timeout=300)
    for nranks in (1, 2, 4):
        assert np.array_equal(out[nranks]["iso"], out[nranks]["again"]), nranks
        assert np.array_equal(out[nranks]["iso"], out[1]["iso"]) and np.array_equal(out[nranks]["counts"], out[1]["counts"]), nranks
    ntri = int(out[1]["iso"][0])
    assert ntri > 1000 and out[1]["iso"].size == NFIG + 10 * ntri and int(out[1]["iso"][WRITTEN]) == ntri and int(out[1]["counts"][WRITTEN]) == 0 and out[1]["counts"].size == NFIG


def test_refusals(gpu):
    """every refusal of include/varden_amd.h, each followed by a call that succeeds and gives the bits of the first: nothing was left allocated or broken"""
    from varden_amd import capi
    from varden_amd.boxlib import handle_array
    lib = capi.load()
    H = hier(_pkg(), AMR3[0], AMR3[1], seed=8)
    out = capi.Iso()
    dx = (C.c_double * 12)(*[v for l in H.dx for v in l] + [1.0] * 3)
    bad_dx = (C.c_double * 12)(*[v for l in H.dx for v in l][:4] + [0.0] + [1.0] * 7)
    buf = np.zeros((8, 3, 3))
    pt = buf.ctypes.data_as(C.POINTER(C.c_double))

    def call(nlev, mf, comp, bccomp, dxp, bct, iso, max_tri=0, tri=None, o=C.byref(out), mla=H.mla.h):
        rc = lib.vdn_isosurface(nlev, mla, handle_array(mf) if mf is not None else None, comp, bccomp, dxp, bct, iso, max_tri, tri, None, o)
        return rc, (lib.vdn_last_error() or b"").decode()
    try:
        write_field(H, random_field(H, 19))
        first = all_bits(isosurface(H, ISO))
        other = H.bl.MLLayout([((0, 0, 0), (15, 15, 15))], [[((0, 0, 0), (15, 15, 15))]])
        s_other = H.bl.MultiFab(other, 0, 2, 1)
        bct_other = H.bl.BCTower(other, WALLS)
        s_nog = [H.bl.MultiFab(H.mla, l, 2, 0) for l in range(3)]
        nodal = [H.bl.MultiFab(H.mla, l, 2, 1, nodal=(1, 1, 1)) for l in range(3)]
        b, inf, nan = H.bct.h, float("inf"), float("nan")
        four = H.s + H.s[:1]
        cases = [((0, H.s, 0, 3, dx, b, ISO), "nlev"), ((5, four + H.s[:1], 0, 3, dx, b, ISO), "nlev"), ((2, H.s, 0, 3, dx, b, ISO), "does not match"),
                 ((3, None, 0, 3, dx, b, ISO), "null argument"), ((3, H.s, 0, 3, dx, b, ISO, 0, None, None), "null argument"),
                 ((3, H.s, 0, 3, dx, b, ISO, 0, None, C.byref(out), None), "null argument"),
                 ((3, H.s, 0, 3, None, b, ISO), "dx"), ((3, H.s, 0, 3, bad_dx, b, ISO), "dx["), ((3, H.s, 0, 3, dx, None, ISO), "bct"),
                 ((3, H.s, 0, 3, dx, bct_other.h, ISO), "another layout"), ((3, [s_other] + H.s[1:], 0, 3, dx, b, ISO), "not a multifab of level"),
                 ((3, H.s[::-1], 0, 3, dx, b, ISO), "not a multifab of level"), ((3, nodal, 0, 3, dx, b, ISO), "nodal"),
                 ((3, H.s, 2, 3, dx, b, ISO), "component"), ((3, H.s, -1, 3, dx, b, ISO), "comp"), ((3, s_nog, 0, 3, dx, b, ISO), "ghost"),
                 ((3, H.s, 0, -1, dx, b, ISO), "boundary component"), ((3, H.s, 0, 99, dx, b, ISO), "boundary component"),
                 ((3, H.s, 0, 3, dx, b, nan), "not finite"), ((3, H.s, 0, 3, dx, b, inf), "not finite"), ((3, H.s, 0, 3, dx, b, -inf), "not finite"),
                 ((3, H.s, 0, 3, dx, b, ISO, -1, pt), "max_tri"), ((3, H.s, 0, 3, dx, b, ISO, 8, None), "NULL tri_host")]
        for args, word in cases:
            rc, msg = call(*args)
            assert rc != 0 and word in msg and msg.startswith("vdn_isosurface:"), (args[0], word, rc, msg)
            assert np.array_equal(all_bits(isosurface(H, ISO)), first), word
        for m in s_nog + nodal + [s_other]:
            m.destroy()
        bct_other.destroy()
        other.destroy()
        # a refinement ratio other than 2
        four = H.bl.MLLayout([((0, 0, 0), (7, 7, 7)), ((0, 0, 0), (31, 31, 31))], [[((0, 0, 0), (7, 7, 7))], [((8, 8, 8), (23, 23, 23))]], rr=[(4, 4, 4)])
        s4 = [H.bl.MultiFab(four, l, 2, 1) for l in range(2)]
        b4 = H.bl.BCTower(four, WALLS)
        rc, msg = call(2, s4, 0, 3, dx, b4.h, ISO, mla=four.h)
        assert rc != 0 and "refinement ratio" in msg, msg
        assert np.array_equal(all_bits(isosurface(H, ISO)), first)
        for m in s4:
            m.destroy()
        b4.destroy()
        four.destroy()
    finally:
        H.close()
    # dm = 2
    from tests._diagnostics_worker import Hier
    H2 = Hier(_pkg(), (16, 16), [[((0, 0, 0), (15, 15, 0))]], phys=[[15, 15], [15, 15]], dm=2, nscal=2)
    try:
        rc = lib.vdn_isosurface(1, H2.mla.h, handle_array(H2.s), 0, 2, dx, H2.bct.h, ISO, 0, None, None, C.byref(out))
        assert rc != 0 and b"dm = 2" in lib.vdn_last_error(), lib.vdn_last_error()
        with pytest.raises(capi.VardenError, match="dm = 2"):
            H2.pkg.advance.isosurface(H2.mla, H2.s, 0, 2, H2.dx, H2.bct, ISO)
        assert H2.diagnostics(vort=False)["cells"] == 256
    finally:
        H2.close()


def _state(G):
    return [np.concatenate([mf.to_numpy(i).ravel() for i in range(mf.nfabs())]) for mfs in (G.uold, G.sold, G.gp, G.p) for mf in mfs]


def test_files_of_an_adaptive_run(gpu, tmp_path):
    """inputs.run on the 32^3 bubble with two levels, iso_int = 2 and diag_int = 1, four steps: a .ply file for step 0 and after every second step and a .dat line for each;
    every file holds the triangles of its line, the bubble's surface is closed and encloses the heavy fluid; the last file is a fresh call's bytes.  Without the key no
    file is written, and uold, sold, gp, p of the run are bit for bit those of the run with it"""
    from varden_amd import advance as adv
    from varden_amd import inputs
    text = open(INPUTS).read()
    on, off = tmp_path / "on", tmp_path / "off"
    on.mkdir(); off.mkdir()
    nl, G = inputs.run(text, report=None, outdir=str(on))
    try:
        assert int(nl["iso_int"]) == 2 and float(nl["iso_value"]) == 5.5 and int(nl["max_step"]) == 4 and G.nlev == 2
        found = sorted(f for f in os.listdir(str(on)) if f.startswith("iso"))
        assert found == ["iso.dat", "iso00000.ply", "iso00002.ply", "iso00004.ply"], found
        lines = open(str(on / "iso.dat")).read().splitlines()
        assert lines[0] == inputs.iso_header().rstrip("\n") and lines[0].split() == ["#", "step", "time", "ntri", "cut_cells", "area", "volume_above"] and len(lines) == 4
        diag = {int(ln.split()[0]): ln.split() for ln in open(str(on / "varden_diag.out")).read().splitlines()[1:]}
        assert all(len(ln) == len(lines[0]) for ln in lines)
        for ln, f in zip(lines[1:], found[1:]):
            step, time, ntri, cut, area, above = ln.split()
            P = adv.read_iso(str(on / f))
            assert int(step) == int(f[3:8]) and P["iso"] == 5.5 and P["time"] == float(time) == float(diag[int(step)][1])
            assert P["tri"].shape == (int(ntri), 3, 3) and int(ntri) > 500 and 0 < int(cut) < int(ntri) and set(P["level"]) <= {0, 1}
            assert np.array_equal(P["indices"].ravel(), np.arange(3 * int(ntri)))
            # the bubble: radius about 0.1, closed (the divergence theorem gives the volume of the line), inside the unit cube
            T = P["tri"].astype(np.longdouble)
            enclosed = float(((T[:, 0] * np.cross(T[:, 1], T[:, 2])).sum(axis=1) / 6).sum())
            assert abs(enclosed - float(above)) < 1e-12 and 0.5 < float(above) / (4 / 3 * math.pi * 1e-3) < 1.5 and 0.5 < float(area) / (4 * math.pi * 1e-2) < 1.5
            assert P["tri"].min() > 0.2 and P["tri"].max() < 0.8
        S = G.isosurface("scalar", 0, 5.5)
        adv.write_iso(str(on / "again.ply"), S, G.time)
        assert open(str(on / "again.ply"), "rb").read() == open(str(on / found[-1]), "rb").read()
        assert lines[-1] == inputs.iso_line(G.istep, G.time, S).rstrip("\n")
        R = adv.read_iso(str(on / "again.ply"))
        assert np.array_equal(R["tri"].view(np.uint64), S.tri.view(np.uint64)) and np.array_equal(R["level"], S.level)
        # the velocity through the driver; a field it does not know
        V = G.isosurface("velocity", 2, 0.0, triangles=False)
        assert V.tri is None and V.ntri > 0 and V.nonfinite_cells == 0
        with pytest.raises(ValueError, match="isosurface field"):
            G.isosurface("vorticity", 0, 1.0)
        with_key = _state(G)
    finally:
        G.close()
    nl, G = inputs.run(re.sub(r"(?m)^\s*iso_int\s*=.*$", " iso_int = 0", text), report=None, outdir=str(off))
    try:
        assert not [f for f in os.listdir(str(off)) if f.startswith("iso")]
        without = _state(G)
        assert len(with_key) == len(without) and all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(with_key, without))
    finally:
        G.close()
