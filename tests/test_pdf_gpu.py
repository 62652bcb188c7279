"""PDFs and conditional sums by value on the device (vdn_pdf, vdn_pdf2, varden_amd/csrc/pdf.hip) against numpy over to_numpy() of the same multifabs, the composite mask
built in numpy from the box lists and the slot rule of csrc/pdf_bin.h restated in float64 (tests/_pdf_worker.py: slots, reference).  The grids are those of
tests/_profiles_worker.py; the fields are seeded random values of both signs, the spacings are powers of two, every ghost cell is NaN for the three fields that read
none.  cells per level, nan_cells and the volume row agree exactly; every sum row agrees with a reference added in extended precision to (n + 8) 2^-53 sum |term| per
slot and row (derived in _pdf_worker.check, not measured)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests._diagnostics_worker import Hier
from tests._pdf_worker import (RANK_AXES, RANK_PAIR, SUM_GROUPS, all_bits, all_bits2, check, group, pdf, pdf2, rank_figures, reference2, slots, vorticity)
from tests._profiles_worker import AMR3, EPS, FLAT, ONE_LEVEL, hier
from tests.children import launch_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_3d_n32_pdf")
NBINS = (1, 7, 256)
# per field: comp, lo, hi -- widths that are no power of two, with cells below and above the range (the random fields lie in (-1, 1), their magnitude below sqrt 3)
AXES = {"scalar": (0, -0.75, 0.8), "velocity": (2, -0.5, 0.9), "magvel": (0, 0.2, 1.5)}


def _pkg():
    import varden_amd
    from varden_amd import advance, boxlib, capi  # noqa: F401
    return varden_amd


def power_of_two_dx(H):
    H.dx = [[2.0 ** -((3, 2, 4)[d] + l) for d in range(H.dm)] for l in range(H.nlev)]
    return H


def edit(H, mfs, l, fn):
    """fn(f, lo, g) changes the host copy f of every box of level l of mfs in place: f[i - lo[0] + g[0], j - lo[1] + g[1], k - lo[2] + g[2], comp] is cell (i, j, k)"""
    mf = mfs[l]
    for i in range(mf.nfabs()):
        lo, hi = mf.get_box(i)
        f = mf.to_numpy(i)
        g = [mf.ng if f.shape[d] > hi[d] - lo[d] + 1 else 0 for d in range(3)]
        fn(f, lo, hi, g)
        mf.from_numpy(f, i)


def plant(H, mfs, l, cell, comp, value):
    def fn(f, lo, hi, g):
        if all(lo[d] <= cell[d] <= hi[d] for d in range(3)):
            f[tuple(cell[d] - lo[d] + g[d] for d in range(3)) + (comp,)] = value
    edit(H, mfs, l, fn)


@pytest.mark.parametrize("nscal", [2, 5, 11])
def test_fields_without_ghost_cells(gpu, nscal):
    """scalar, velocity, magvel on one box, six boxes and three levels; nscal 2 runs the instantiation that carries four scalars, 5 and 11 the one that carries eleven;
    256 bins at nscal = 11 is the largest LDS table.  Every ghost cell is NaN: none is read"""
    for name, (n, boxes) in (("one-box", (ONE_LEVEL["one-box"][0], [ONE_LEVEL["one-box"][1]])), ("six-boxes", (ONE_LEVEL["six-boxes"][0], [ONE_LEVEL["six-boxes"][1]])),
                             ("amr3", AMR3)):
        H = hier(_pkg(), n, boxes, nscal=nscal, seed=nscal)
        try:
            for field, (comp, lo, hi) in AXES.items():
                for nbins in NBINS:
                    P = pdf(H, field, comp, lo, hi, nbins)
                    assert P.rows.shape == (P.layout["nrow"], nbins + 2) and P.layout["nrow"] == nscal + 9 and P.cells.shape == (H.nlev, nbins + 2)
                    ref, cells, nan_cells, volume, ab = check(P, H, field, comp, lo, hi, nbins, "%s nscal=%d" % (name, nscal))
                    assert nan_cells == 0 and cells[:, 0].sum() + cells[:, -1].sum() > 0 and np.isfinite(P.rows).all()
            # the host wrappers: the density integrates to 1 over the range, a conditional mean of q lies in its bin
            P = pdf(H, "scalar", 0, -0.75, 0.8, 7)
            assert abs((P.density() * P.w).sum() - 1.0) < 1e-14 and np.array_equal(P.edges[[0, -1]], [-0.75, 0.8]) and len(P.centres) == 9
            mq = P.mean("q")[1:-1]
            assert ((mq >= P.edges[:-1]) & (mq <= P.edges[1:])).all() and P.mean("s").shape == (nscal, 9)
            assert np.array_equal(group(P, "q"), group(P, "s")[:1])
        finally:
            H.close()


@pytest.mark.parametrize("dm,nscal", [(3, 2), (3, 5), (3, 11), (2, 2)])
def test_vorticity(gpu, dm, nscal):
    """q is, bit for bit, what vdn_make_vorticity stores: its magnitude on three levels with no-slip walls (one-sided forms), the signed value for dm = 2.  nscal = 5 runs
    the instantiation that carries eleven scalars with rows it does not have"""
    if dm == 3:
        H = power_of_two_dx(Hier(_pkg(), AMR3[0], AMR3[1], nscal=nscal, seed=20 + nscal))
        lo, hi = 1.0, 400.0
    else:
        H = power_of_two_dx(Hier(_pkg(), FLAT[0], [FLAT[1]], phys=[[15, 15], [15, 15]], nscal=nscal, dm=2, seed=5))
        lo, hi = -9.0, 13.0
    try:
        W = vorticity(H)                                      # fills the ghost cells the call reads
        assert dm == 3 or min(float(np.nanmin(w)) for w in W) < 0.0
        for nbins in NBINS:
            P = pdf(H, "vorticity", 0, lo, hi, nbins)
            ref, cells, nan_cells, volume, ab = check(P, H, "vorticity", 0, lo, hi, nbins, "dm=%d nscal=%d" % (dm, nscal))
            assert nan_cells == 0 and cells[:, 1:-1].sum() > 0.5 * cells.sum()
    finally:
        H.close()


def test_dim2(gpu):
    n, boxes = FLAT
    H = hier(_pkg(), n, [boxes], phys=[[15, 15], [15, 15]], nscal=2, dm=2, seed=4)
    try:
        for field, (comp, lo, hi) in (("scalar", (1, 0.1, 0.9)), ("velocity", (1, -0.9, -0.1)), ("magvel", (0, 0.2, 1.2))):
            for nbins in NBINS:
                P = pdf(H, field, comp, lo, hi, nbins)
                assert P.layout["nrow"] == 9 and P.rows.shape == (9, nbins + 2) and P["u"].shape == (2, nbins + 2)
                check(P, H, field, comp, lo, hi, nbins, "dm=2")
        a1, a2 = ("scalar", 0, -0.75, 0.8, 64), ("velocity", 1, -0.9, -0.1, 3)
        J = pdf2(H, a1, a2)
        cells, nan_cells, volume = reference2(H, a1, a2)
        assert np.array_equal(J.cells, cells) and J.nan_cells == nan_cells == 0 and np.array_equal(J.volume, volume) and J.cells.sum() == 24 * 40
    finally:
        H.close()


def test_planted_values(gpu):
    """scalar 1 is 0.3 everywhere but for eight planted cells of level 0: lo, -0.0 (lo = 0), hi, the last double below hi, +Inf, -Inf and a NaN in composite cells, a NaN
    in a COVERED cell, which must not count"""
    H = hier(_pkg(), AMR3[0], AMR3[1], nscal=2, seed=11)
    lo, hi, nbins = 0.0, 0.5, 4
    try:
        def flat(f, blo, bhi, g):
            f[tuple(slice(g[d], f.shape[d] - g[d]) for d in range(3)) + (1,)] = 0.3
        for l in range(H.nlev):
            edit(H, H.s, l, flat)
        M = H.composite()
        free = [tuple(int(v) for v in c) for c in np.argwhere(M[0])[::37][:7]]
        covered = tuple(int(v) for v in np.argwhere(~M[0])[5])
        values = [lo, -0.0, hi, np.nextafter(hi, -np.inf), np.inf, -np.inf, np.nan]
        assert list(slots(np.array(values), lo, hi, nbins)) == [1, 1, 5, 4, 5, 0, -1] and slots(np.array([0.3]), lo, hi, nbins)[0] == 3
        for c, v in zip(free, values):
            plant(H, H.s, 0, c, 1, v)
        plant(H, H.s, 0, covered, 1, np.nan)
        N = int(sum(m.sum() for m in M))
        P = pdf(H, "scalar", 1, lo, hi, nbins)
        assert P.nan_cells == 1 and list(P.cells.sum(axis=0)) == [1, 2, 0, N - 7, 1, 2], (P.nan_cells, P.cells)
        assert list(P.cells[0]) == [1, 2, 0, int(M[0].sum()) - 7, 1, 2] and list(P.cells[2]) == [0, 0, 0, int(M[2].sum()), 0, 0]
        check(P, H, "scalar", 1, lo, hi, nbins, "planted")
        dv0 = float(np.prod(H.dx[0]))
        # the rows of the slots with an infinite q: q and s1 are Inf of the right sign; the other rows are finite
        assert P["q"][5] == np.inf and P["q"][0] == -np.inf and P["s"][1][5] == np.inf and np.isfinite(P["s"][0]).all() and np.isfinite(P["ke"]).all()
        assert P["q"][1] == 0.0 and P["q"][4] == np.nextafter(hi, -np.inf) * dv0 and P["volume"][1] == 2 * dv0
        # the joint form counts the NaN cell once when either value is NaN, and never the covered one
        J = pdf2(H, ("scalar", 1, lo, hi, nbins), ("scalar", 0, -0.75, 0.8, 5))
        cells, nan_cells, volume = reference2(H, ("scalar", 1, lo, hi, nbins), ("scalar", 0, -0.75, 0.8, 5))
        assert J.nan_cells == nan_cells == 1 and np.array_equal(J.cells, cells) and np.array_equal(J.cells.sum(axis=2), P.cells)
    finally:
        H.close()


def test_smooth_field_and_worst_case(gpu):
    """the two extremes of the distinct-slot loop on a 64 x 8 x 4 box.  Smooth: q depends on k alone, every lane of a wave takes the same slot.  Worst case: q is a ramp
    along x with 64 bins over one row, every lane of a wave takes another slot.  The same bounds hold"""
    H = hier(_pkg(), (64, 8, 4), [[((0, 0, 0), (63, 7, 3))]], nscal=2, seed=13)
    try:
        def ramp(axis):
            def fn(f, lo, hi, g):
                idx = np.arange(lo[axis], hi[axis] + 1, dtype=np.float64) + 0.5
                shape = [1, 1, 1]
                shape[axis] = len(idx)
                f[tuple(slice(g[d], f.shape[d] - g[d]) for d in range(3)) + (1,)] = idx.reshape(shape)
            return fn
        edit(H, H.s, 0, ramp(2))
        P = pdf(H, "scalar", 1, 0.0, 4.0, 4)
        check(P, H, "scalar", 1, 0.0, 4.0, 4, "smooth")
        assert list(P.cells[0]) == [0] + [64 * 8] * 4 + [0]
        edit(H, H.s, 0, ramp(0))
        P = pdf(H, "scalar", 1, 0.0, 64.0, 64)
        check(P, H, "scalar", 1, 0.0, 64.0, 64, "worst case")
        assert list(P.cells[0]) == [0] + [8 * 4] * 64 + [0]
        assert np.array_equal(P["q"][1:-1], (np.arange(64) + 0.5) * 32 * float(np.prod(H.dx[0])))         # 32 equal terms: exact
    finally:
        H.close()


def test_identities(gpu):
    """summed over the slots the figures are vdn_diagnostics': cells and volume exactly, s, ru and ke within (N + 8) 2^-53 sum |term|, N the number of composite cells"""
    H = hier(_pkg(), AMR3[0], AMR3[1], nscal=3, seed=3)
    try:
        D = H.pkg.advance.diagnostics(H.mla, H.u, H.s, H.dx, None, vort=False)
        N = D["cells"]
        for field, (comp, lo, hi) in AXES.items():
            P = pdf(H, field, comp, lo, hi, 64)
            ref, cells, nan_cells, volume, ab = check(P, H, field, comp, lo, hi, 64, "identities")
            assert int(P.cells.sum()) + P.nan_cells == N and list(P.cells.sum(axis=1)) == D["cells_lev"]
            assert math.fsum(P["volume"]) == D["volume"]
            pairs = [("s", c, D["sum_s"][c]) for c in range(3)] + [("ru", d, D["momentum"][d]) for d in range(3)] + [("ke", 0, D["kinetic"])]
            for g, i, want in pairs:
                got, bound = math.fsum(group(P, g)[i]), (N + 8) * EPS * math.fsum(ab[g][i])
                print("%s %s[%d]: slots %.17e diagnostics %.17e |diff| %.3e bound %.3e" % (field, g, i, got, want, abs(got - want), bound))
                assert abs(got - want) <= bound, (field, g, i, got, want, bound)
    finally:
        H.close()


def test_pdf2(gpu):
    """the joint counts agree with numpy exactly; the marginal over axis 2 is vdn_pdf's cells per level for the same first axis; the vorticity as one of the two"""
    H = power_of_two_dx(Hier(_pkg(), AMR3[0], AMR3[1], nscal=3, seed=17))
    try:
        vorticity(H)
        for a1, a2 in ((("scalar", 0, -0.75, 0.8, 64), ("velocity", 2, -0.5, 0.9, 64)), (("magvel", 0, 0.2, 1.5, 7), ("scalar", 2, 0.1, 0.9, 1)),
                       (("scalar", 0, -0.75, 0.8, 5), ("vorticity", 0, 1.0, 60.0, 33))):
            J = pdf2(H, a1, a2)
            cells, nan_cells, volume = reference2(H, a1, a2)
            assert J.cells.shape == (3, a1[4] + 2, a2[4] + 2) and J.cells.dtype == np.int64 and np.array_equal(J.cells, cells), (a1, a2)
            assert J.nan_cells == nan_cells == 0 and np.array_equal(J.volume.view(np.uint64), volume.view(np.uint64))
            P = pdf(H, *a1)
            assert np.array_equal(J.cells.sum(axis=2), P.cells) and np.array_equal(J.cells.sum(axis=1), pdf(H, *a2).cells)
            assert len(J.edges1) == a1[4] + 1 and len(J.edges2) == a2[4] + 1 and J.edges1[-1] == a1[3]
    finally:
        H.close()


def test_two_calls_give_the_same_bits(gpu):
    H = power_of_two_dx(Hier(_pkg(), AMR3[0], AMR3[1], nscal=11, seed=9))
    try:
        out = rank_figures(H)
        for i in range(len(RANK_AXES)):
            assert np.array_equal(out["axis%d" % i], out["again%d" % i]), RANK_AXES[i]
        assert np.array_equal(out["pair"], all_bits2(pdf2(H, *RANK_PAIR)))
    finally:
        H.close()


def test_ranks_give_identical_bits(gpu, tmp_path):
    """one rank against two and four (the RCCL test double, rank threads in child processes) on the three-level hierarchy: every rank gets the same bits in every row
    and count, and they do not depend on the number of ranks -- a slab's partials live under its GLOBAL number and are added in that order everywhere"""
    keys = tuple("%s%d" % (k, a) for k in ("axis", "again") for a in range(len(RANK_AXES))) + ("pair",)
    out = {}
    for nranks, per_proc in ((1, 1), (2, 1), (4, 2)):
        out[nranks] = launch_ranks("_pdf_worker.py", nranks, tmp_path, "pdf%d" % nranks, [], per_proc=per_proc, agree=keys, timeout=300)
    for nranks in (1, 2, 4):
        for a, ax in enumerate(RANK_AXES):
            assert np.array_equal(out[nranks]["axis%d" % a], out[nranks]["again%d" % a]), (nranks, ax)
            assert np.array_equal(out[nranks]["axis%d" % a], out[1]["axis%d" % a]), (nranks, ax)
        assert np.array_equal(out[nranks]["pair"], out[1]["pair"]), nranks
    assert out[1]["axis0"].size == 66 * (3 + 9) + 3 * 66 + 1
    # the single rank's figures are not empty: every composite cell is counted
    ncells = 16 ** 3 + (12 * 16 * 12 + 8 * 8 * 16) * 7 // 8 + 16 * 24 * 16 * 7 // 8
    assert int(out[1]["axis0"][66 * 12:-1].sum()) + int(out[1]["axis0"][-1]) == ncells


def test_refusals(gpu):
    """every refusal of include/varden_amd.h, each followed by a call that succeeds and gives the bits of the first: nothing was left allocated or broken"""
    from varden_amd import capi
    from varden_amd.boxlib import handle_array
    lib = capi.load()
    H = power_of_two_dx(Hier(_pkg(), AMR3[0], AMR3[1], nscal=2, seed=1))
    nrow = H.pkg.advance.pdf_layout(3, 2)["nrow"]
    rows, cells, nan = np.zeros((nrow, 258)), np.zeros((4, 258), dtype=np.int64), C.c_longlong(0)
    cells2, vol2 = np.zeros((4, 66, 66), dtype=np.int64), np.zeros((66, 66))
    dx = (C.c_double * 12)(*[v for lev in H.dx for v in lev] + [1.0] * 3)
    po, pc = rows.ctypes.data_as(C.POINTER(C.c_double)), cells.ctypes.data_as(C.POINTER(C.c_longlong))
    pc2, pv2 = cells2.ctypes.data_as(C.POINTER(C.c_longlong)), vol2.ctypes.data_as(C.POINTER(C.c_double))
    good = (0, 0, 64, -0.75, 0.8)

    def call(nlev, u, s, dxp, bct, axis, o=po, c=pc, n=C.byref(nan), mla=H.mla.h):
        rc = lib.vdn_pdf(nlev, mla, handle_array(u) if u is not None else None, handle_array(s) if s is not None else None, dxp, bct, *axis, o, c, n)
        return rc, (lib.vdn_last_error() or b"").decode()

    def call2(nlev, u, s, dxp, bct, a1, a2, c=pc2, v=pv2, n=C.byref(nan), mla=H.mla.h):
        rc = lib.vdn_pdf2(nlev, mla, handle_array(u) if u is not None else None, handle_array(s) if s is not None else None, dxp, bct, *a1, *a2, c, v, n)
        return rc, (lib.vdn_last_error() or b"").decode()
    try:
        vorticity(H)
        first = all_bits(pdf(H, "scalar", 0, -0.75, 0.8, 64))
        first_vort = all_bits(pdf(H, "vorticity", 0, 1.0, 60.0, 64))
        other = H.bl.MLLayout([((0, 0, 0), (15, 15, 15))], [[((0, 0, 0), (15, 15, 15))]])
        s_other = H.bl.MultiFab(other, 0, 2, 0)
        u_nog = [H.bl.MultiFab(H.mla, l, 3, 0) for l in range(3)]
        four = H.u + H.u[:1]
        b = H.bct.h
        inf, nanv = float("inf"), float("nan")
        cases = [((0, H.u, H.s, dx, b, good), "nlev"), ((5, four + H.u[:1], four + H.s[:1], dx, b, good), "nlev"), ((2, H.u, H.s, dx, b, good), "does not match"),
                 ((3, H.u, [s_other] + H.s[1:], dx, b, good), "layouts of u and s differ"), ((3, H.s, H.s, dx, b, good), "components"),
                 ((3, H.u, H.s, None, b, good), "dx"), ((3, None, H.s, dx, b, good), "null argument"), ((3, H.u, None, dx, b, good), "null argument"),
                 ((3, H.u, H.s, dx, b, good, po, pc, C.byref(nan), None), "null argument"),
                 ((3, H.u, H.s, dx, b, good, None), "null output"), ((3, H.u, H.s, dx, b, good, po, None), "null output"), ((3, H.u, H.s, dx, b, good, po, pc, None), "null output"),
                 ((3, H.u, H.s, dx, b, (4, 0, 64, -0.75, 0.8)), "field"), ((3, H.u, H.s, dx, b, (-1, 0, 64, -0.75, 0.8)), "field"),
                 ((3, H.u, H.s, dx, b, (0, 2, 64, -0.75, 0.8)), "comp"), ((3, H.u, H.s, dx, b, (0, -1, 64, -0.75, 0.8)), "comp"), ((3, H.u, H.s, dx, b, (1, 3, 64, -0.75, 0.8)), "comp"),
                 ((3, H.u, H.s, dx, b, (0, 0, 0, -0.75, 0.8)), "nbins"), ((3, H.u, H.s, dx, b, (0, 0, 257, -0.75, 0.8)), "nbins"),
                 ((3, H.u, H.s, dx, b, (0, 0, 64, 0.8, 0.8)), "lo <"), ((3, H.u, H.s, dx, b, (0, 0, 64, 0.8, -0.75)), "lo <"), ((3, H.u, H.s, dx, b, (0, 0, 64, nanv, 0.8)), "finite"),
                 ((3, H.u, H.s, dx, b, (0, 0, 64, -0.75, inf)), "finite"), ((3, H.u, H.s, dx, b, (0, 0, 64, -inf, 0.8)), "finite"),
                 ((3, H.u, H.s, dx, None, (3, 0, 64, 1.0, 60.0)), "bct"), ((3, u_nog, H.s, dx, b, (3, 0, 64, 1.0, 60.0)), "ghost")]
        for args, word in cases:
            rc, msg = call(*args)
            assert rc != 0 and word in msg and msg.startswith("vdn_pdf:"), (args[0], word, rc, msg)
            rc, msg = call(3, H.u, H.s, dx, None, good)
            assert rc == 0, msg
            again = np.concatenate([rows.ravel()[:nrow * 66].view(np.uint64), cells.ravel()[:3 * 66].astype(np.uint64), np.array([nan.value], dtype=np.uint64)])
            assert np.array_equal(again, first), word
        assert np.array_equal(all_bits(pdf(H, "vorticity", 0, 1.0, 60.0, 64)), first_vort)
        # the joint form refuses the same, per axis, with its own limit of 64 bins
        j_first = all_bits2(pdf2(H, *RANK_PAIR))
        g2 = (1, 2, 5, -0.5, 0.9)
        for args, word in (((0, H.u, H.s, dx, b, good, g2), "nlev"), ((3, H.u, H.s, None, b, good, g2), "dx"), ((3, H.u, H.s, dx, b, (0, 0, 65, -0.75, 0.8), g2), "nbins"),
                           ((3, H.u, H.s, dx, b, good, (1, 2, 0, -0.5, 0.9)), "axis 2: nbins"), ((3, H.u, H.s, dx, b, good, (5, 0, 5, -0.5, 0.9)), "axis 2: field"),
                           ((3, H.u, H.s, dx, b, (0, 7, 64, -0.75, 0.8), g2), "axis 1: comp"), ((3, H.u, H.s, dx, b, good, (1, 2, 5, 0.9, 0.9)), "lo <"),
                           ((3, H.u, H.s, dx, None, good, (3, 0, 5, 1.0, 60.0)), "bct"), ((3, u_nog, H.s, dx, b, (3, 0, 5, 1.0, 60.0), g2), "ghost"),
                           ((3, H.u, H.s, dx, b, good, g2, None), "null output"), ((3, H.u, H.s, dx, b, good, g2, pc2, None), "null output"),
                           ((3, H.u, H.s, dx, b, good, g2, pc2, pv2, None), "null output"), ((5, four + H.u[:1], four + H.s[:1], dx, b, good, g2), "nlev"),
                           ((2, H.u, H.s, dx, b, good, g2), "does not match"), ((3, H.u, [s_other] + H.s[1:], dx, b, good, g2), "layouts of u and s differ"),
                           ((3, H.s, H.s, dx, b, good, g2), "components"), ((3, None, H.s, dx, b, good, g2), "null argument"), ((3, H.u, None, dx, b, good, g2), "null argument"),
                           ((3, H.u, H.s, dx, b, good, g2, pc2, pv2, C.byref(nan), None), "null argument"),
                           ((3, H.u, H.s, dx, b, (0, 0, 64, nanv, 0.8), g2), "finite"), ((3, H.u, H.s, dx, b, good, (1, 2, 5, -0.5, inf)), "finite"),
                           ((3, H.u, H.s, dx, b, good, (1, 2, 5, -inf, 0.9)), "finite"), ((3, H.u, H.s, dx, b, good, (1, 2, 5, 0.9, -0.5)), "lo <"),
                           ((3, H.u, H.s, dx, b, (-1, 0, 64, -0.75, 0.8), g2), "axis 1: field"), ((3, H.u, H.s, dx, b, good, (1, 3, 5, -0.5, 0.9)), "axis 2: comp"),
                           ((3, H.u, H.s, dx, b, good, (1, 2, 65, -0.5, 0.9)), "axis 2: nbins")):
            rc, msg = call2(*args)
            assert rc != 0 and word in msg and msg.startswith("vdn_pdf2:"), (args[0], word, rc, msg)
            assert np.array_equal(all_bits2(pdf2(H, *RANK_PAIR)), j_first), word
        with pytest.raises(ValueError, match="pdf field"):
            pdf(H, "density", 0, 0.0, 1.0, 4)
        for m in u_nog + [s_other]:
            m.destroy()
        other.destroy()
    finally:
        H.close()
    # a refinement ratio other than 2; dm = 2 runs on one level.  Each refusal of either entry is followed by the call on the process's own hierarchy, bits as before
    g2 = (1, 1, 5, -0.9, -0.1)
    pair = (("scalar", 0, -0.75, 0.8, 64), ("velocity", 1, -0.9, -0.1, 5))

    def refused_then_same(Hx, first, j_first, rc, word):
        msg = lib.vdn_last_error() or b""
        assert rc != 0 and word in msg, (word, rc, msg)
        assert np.array_equal(all_bits(pdf(Hx, "scalar", 0, -0.75, 0.8, 64)), first) and np.array_equal(all_bits2(pdf2(Hx, *pair)), j_first), word
    H4 = hier(_pkg(), 8, [[((0, 0, 0), (7, 7, 7))]], nscal=2)
    try:
        first, j_first = all_bits(pdf(H4, "scalar", 0, -0.75, 0.8, 64)), all_bits2(pdf2(H4, *pair))
        assert int(first[11 * 66:-1].sum()) == 512
        four = H4.bl.MLLayout([((0, 0, 0), (7, 7, 7)), ((0, 0, 0), (31, 31, 31))], [[((0, 0, 0), (7, 7, 7))], [((8, 8, 8), (23, 23, 23))]], rr=[(4, 4, 4)])
        u4 = [H4.bl.MultiFab(four, l, 3, 1) for l in range(2)]
        s4 = [H4.bl.MultiFab(four, l, 2, 1) for l in range(2)]
        refused_then_same(H4, first, j_first, lib.vdn_pdf(2, four.h, handle_array(u4), handle_array(s4), dx, None, *good, po, pc, C.byref(nan)), b"refinement ratio")
        refused_then_same(H4, first, j_first, lib.vdn_pdf2(2, four.h, handle_array(u4), handle_array(s4), dx, None, *good, *g2, pc2, pv2, C.byref(nan)), b"refinement ratio")
        for m in u4 + s4:
            m.destroy()
        four.destroy()
    finally:
        H4.close()
    H2 = hier(_pkg(), (16, 16), [[((0, 0, 0), (15, 15, 0))]], phys=[[15, 15], [15, 15]], dm=2, nscal=2)
    try:
        first, j_first = all_bits(pdf(H2, "scalar", 0, -0.75, 0.8, 64)), all_bits2(pdf2(H2, *pair))
        assert int(first[9 * 66:-1].sum()) == 256
        two = H2.bl.MLLayout([((0, 0, 0), (15, 15, 0)), ((0, 0, 0), (31, 31, 0))], [[((0, 0, 0), (15, 15, 0))], [((8, 8, 0), (23, 23, 0))]], rr=[(2, 2, 1)])
        u2 = [H2.bl.MultiFab(two, l, 2, 1) for l in range(2)]
        s2 = [H2.bl.MultiFab(two, l, 2, 1) for l in range(2)]
        refused_then_same(H2, first, j_first, lib.vdn_pdf(2, two.h, handle_array(u2), handle_array(s2), dx, None, *good, po, pc, C.byref(nan)), b"dm = 2")
        refused_then_same(H2, first, j_first, lib.vdn_pdf2(2, two.h, handle_array(u2), handle_array(s2), dx, None, *good, *g2, pc2, pv2, C.byref(nan)), b"dm = 2")
        hu, hs = handle_array(H2.u), handle_array(H2.s)
        refused_then_same(H2, first, j_first, lib.vdn_pdf(1, H2.mla.h, hu, hs, dx, None, 1, 2, 64, -0.75, 0.8, po, pc, C.byref(nan)), b"comp")
        refused_then_same(H2, first, j_first, lib.vdn_pdf2(1, H2.mla.h, hu, hs, dx, None, *good, 1, 2, 5, -0.9, -0.1, pc2, pv2, C.byref(nan)), b"axis 2: comp")
        for m in u2 + s2:
            m.destroy()
        two.destroy()
    finally:
        H2.close()


def _read(path):
    """a pdf file: ({header key: value}, column names, rows as strings)"""
    lines = open(path).read().splitlines()
    assert lines[0] == "# VDN_PDF 1", lines[0]
    head = {}
    for ln, key in zip(lines[1:10], ("dm", "field", "comp", "nbins", "lo", "hi", "step", "time", "nan_cells")):
        m = re.fullmatch(r"# %s\s*(\S+)" % key, ln)
        assert m, ln
        head[key] = m.group(1)
    assert lines[10].startswith("#")
    return head, lines[10][1:].split(), [ln.split() for ln in lines[11:]]


def _state(G):
    return [np.concatenate([mf.to_numpy(i).ravel() for i in range(mf.nfabs())]) for mfs in (G.uold, G.sold) for mf in mfs]


def test_pdf_files_of_an_adaptive_run(gpu, tmp_path):
    """inputs.run on the 32^3 bubble with two levels, pdf_int = 2 and diag_int = 1, four steps: a file for step 0 and after every second step, each with 40 + 2 lines; in
    every file the cells add up to the composite cells and the s1 column to the mass on the matching line of the diagnostics file, and both fluids are there.  Without
    the key no file is written, and the fields of the run are bit for bit those of the run with it"""
    from varden_amd import advance as adv
    from varden_amd import inputs
    text = open(INPUTS).read()
    on, off = tmp_path / "on", tmp_path / "off"
    on.mkdir(); off.mkdir()
    nl, G = inputs.run(text, report=None, outdir=str(on))
    try:
        assert int(nl["pdf_int"]) == 2 and int(nl["diag_int"]) == 1 and int(nl["max_step"]) == 4 and G.nlev == 2
        found = sorted(f for f in os.listdir(str(on)) if f.startswith("pdf"))
        assert found == ["pdf00000", "pdf00002", "pdf00004"], found
        cols = ["centre", "cells"] + adv.pdf_columns(2, 3)
        dcols = ["step", "time", "dt"] + adv.diag_columns(2, 3)
        diag = {int(ln.split()[0]): ln.split() for ln in open(str(on / "varden_diag.out")).read().splitlines()[1:]}
        for f in found:
            head, names, rows = _read(str(on / f))
            step = int(f[3:])
            assert names == cols and head["dm"] == "3" and head["field"] == "scalar" and head["comp"] == "1" and head["nbins"] == "40" and int(head["step"]) == step
            assert float(head["lo"]) == 0.5 and float(head["hi"]) == 10.5 and head["nan_cells"] == "0" and float(head["time"]) == float(diag[step][1])
            assert len(rows) == 42 and all(len(r) == len(cols) for r in rows)
            assert [float(r[0]) for r in rows] == [0.5 + (m + 0.5) * 0.25 for m in range(-1, 41)]
            ncell = [int(r[1]) for r in rows]
            vol = [float(r[cols.index("volume")]) for r in rows]
            dcells, dmass = int(diag[step][dcols.index("cells")]), float(diag[step][dcols.index("sum_s1")])
            assert sum(ncell) == dcells and math.fsum(vol) == 1.0 and ncell[0] == 0 and ncell[-1] == 0
            assert ncell[1 + 2] > 0.5 * dcells and sum(ncell[1 + 30:1 + 40]) > 0, ncell                # density 1 lies in bin 2 (slot 3), the bubble's 10 in the top bins
            mass = math.fsum(float(r[cols.index("s1")]) for r in rows)
            # every term is positive: sum |term| is the mass itself; q is s1
            print("%s: sum of the slots %.17e, diagnostics %.17e, |diff| %.3e, bound %.3e" % (f, mass, dmass, abs(mass - dmass), (dcells + 8) * EPS * dmass))
            assert abs(mass - dmass) <= (dcells + 8) * EPS * dmass and [r[cols.index("q")] for r in rows] == [r[cols.index("s1")] for r in rows]
        # the last file holds the figures of a fresh call, digit for digit
        assert open(str(on / found[-1])).read() == inputs.pdf_text(G.pdf("scalar", 0, 0.5, 10.5, 40), G.istep, G.time)
        # the vorticity through the driver: it fills the ghost cells itself; |curl u| >= 0
        V = G.pdf("vorticity", 0, 0.0, 50.0, 16)
        assert V.cells[:, 0].sum() == 0 and int(V.cells.sum()) + V.nan_cells == dcells and V.nan_cells == 0
        J = G.pdf2("scalar", 0, 0.5, 10.5, 40, "velocity", 2, -1.0, 1.0, 8)
        assert np.array_equal(J.cells.sum(axis=2), G.pdf("scalar", 0, 0.5, 10.5, 40).cells)
        with_key = _state(G)
    finally:
        G.close()
    nl, G = inputs.run(re.sub(r"(?m)^\s*pdf_int\s*=.*$", " pdf_int = 0", text), report=None, outdir=str(off))
    try:
        assert not [f for f in os.listdir(str(off)) if f.startswith("pdf")]
        without = _state(G)
        assert len(with_key) == len(without) and all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(with_key, without))
    finally:
        G.close()
