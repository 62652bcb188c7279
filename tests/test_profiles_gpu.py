"""Plane-averaged profiles on the device (vdn_profiles, varden_amd/csrc/profiles.hip) against numpy over to_numpy() of the same multifabs, the composite mask built in
numpy from the box lists (tests/_profiles_worker.py: reference).  The fields are seeded random values of both signs with a few exact +-0 planted, every ghost cell is
NaN (none is read), the spacings are powers of two.  cells and every extremum agree exactly, as 64-bit patterns; sums agree with a reference added in extended
precision to (n + 4) 2^-53 sum |term| per bin and row (derived in _profiles_worker.check, not measured)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests._profiles_worker import AMR3, EPS, FLAT, ONE_LEVEL, all_bits, check, group, hier, profiles
from tests.children import launch_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_3d_n32_prof")


def _pkg():
    import varden_amd
    from varden_amd import advance, boxlib, capi  # noqa: F401
    return varden_amd


def exact_volume(P, H, axis):
    """every bin's volume is (cross-section area) * h, exactly: the spacings are powers of two"""
    area = 1.0
    for d in range(H.dm):
        if d != axis:
            area *= H.n[0][d] * H.dx[0][d]
    want = area * H.dx[H.nlev - 1][axis]
    assert np.array_equal(P["volume"], np.full(len(P.x), want)), (axis, P["volume"], want)
    assert np.array_equal(P.x, (np.arange(len(P.x)) + 0.5) * H.dx[H.nlev - 1][axis])


@pytest.mark.parametrize("grid,nscal", [("one-box", 2), ("one-box", 5), ("six-boxes", 2), ("six-boxes", 5), ("six-boxes", 11)])
def test_one_level(gpu, grid, nscal):
    """nscal 2 runs the instantiation that carries four scalars, 5 and 11 the one that carries eleven; every axis has a thread map of its own"""
    n, boxes = ONE_LEVEL[grid]
    H = hier(_pkg(), n, [boxes], nscal=nscal, seed=nscal)
    try:
        for axis in range(3):
            P = profiles(H, axis)
            assert P.rows.shape == (P.layout["nrow"], n[axis]) and np.isfinite(P.rows).all()
            check(P, H, axis, "%s nscal=%d" % (grid, nscal))
            exact_volume(P, H, axis)
            assert P.cells.sum() == n[0] * n[1] * n[2]
            assert np.allclose(P.mean("s")[0], P["s"][0] / P["volume"]) and P.mean("ruu").shape == (6, n[axis])
        # the planted zeros: the last scalar's minimum is -0.0 in the bin of the first box's low corner, velocity component 1 has +0.0 there as its maximum
        P = profiles(H, 2)
        assert np.signbit(P["s_min"][nscal - 1][0]) and P["s_min"][nscal - 1][0] == 0.0
        assert P["u_max"][1][0] == 0.0 and not np.signbit(P["u_max"][1][0])
    finally:
        H.close()


def test_hierarchy(gpu):
    """three levels, every axis: bins reached by one, two and three levels, every r from 1 to 4; summed over the bins the rows are vdn_diagnostics' figures"""
    nbase, boxes = AMR3
    H = hier(_pkg(), nbase, boxes, nscal=3, seed=3)
    try:
        M = H.composite()
        depth = set()
        D = H.pkg.advance.diagnostics(H.mla, H.u, H.s, H.dx, None, vort=False)
        N = D["cells"]
        for axis in range(3):
            other = tuple(d for d in range(3) if d != axis)
            levels = sum(np.repeat(M[l].any(axis=other), 4 >> l) for l in range(3))
            depth |= set(int(v) for v in levels)
            P = profiles(H, axis)
            assert len(P.x) == 64 and P.rows.shape[0] == P.layout["nrow"]
            ref, cells, ab = check(P, H, axis, "amr3")
            exact_volume(P, H, axis)
            # identities with vdn_diagnostics: (N + 4) 2^-53 sum |term|, N the number of composite cells
            assert sum(int((M[l].sum(axis=other) * (4 >> l)).sum()) for l in range(3)) == int(P.cells.sum())
            pairs = [("volume", 0, D["volume"])] + [("s", c, D["sum_s"][c]) for c in range(3)] + [("ru", d, D["momentum"][d]) for d in range(3)]
            for g, i, want in pairs:
                got, bound = math.fsum(group(P, g)[i]), (N + 4) * EPS * math.fsum(ab[g][i])
                print("axis %d %s[%d]: bins %.17e diagnostics %.17e |diff| %.3e bound %.3e" % (axis, g, i, got, want, abs(got - want), bound))
                assert abs(got - want) <= bound, (axis, g, i, got, want, bound)
            ruu = group(P, "ruu")
            diag = [P.ruu_pairs.index((d, d)) for d in range(3)]
            got = 0.5 * math.fsum(np.concatenate([ruu[i] for i in diag]))
            bound = (N + 4) * EPS * 0.5 * math.fsum(np.concatenate([ab["ruu"][i] for i in diag]))
            print("axis %d kinetic: bins %.17e diagnostics %.17e |diff| %.3e bound %.3e" % (axis, got, D["kinetic"], abs(got - D["kinetic"]), bound))
            assert abs(got - D["kinetic"]) <= bound
            assert D["volume"] == math.fsum(P["volume"])
        assert depth == {1, 2, 3}, depth
    finally:
        H.close()


def test_dim2(gpu):
    n, boxes = FLAT
    H = hier(_pkg(), n, [boxes], phys=[[15, 15], [15, 15]], nscal=2, dm=2, seed=4)
    try:
        for axis in range(2):
            P = profiles(H, axis)
            assert P.rows.shape == (P.layout["nrow"], n[axis]) and P.layout["nrow"] == 21 and P.ruu_pairs == [(0, 0), (0, 1), (1, 1)]
            check(P, H, axis, "dm=2")
            exact_volume(P, H, axis)
    finally:
        H.close()


def test_two_calls_give_the_same_bits(gpu):
    nbase, boxes = AMR3
    H = hier(_pkg(), nbase, boxes, nscal=11, seed=9)
    try:
        for axis in range(3):
            a, b = all_bits(profiles(H, axis)), all_bits(profiles(H, axis))
            assert np.array_equal(a, b), axis
    finally:
        H.close()


def test_ranks_give_identical_bits(gpu, tmp_path):
    """one rank against two and four (the RCCL test double, rank threads in child processes) on the three-level hierarchy: every rank gets the same bits in every row,
    and they do not depend on the number of ranks -- a slot's partials live under its GLOBAL number and are added in that order everywhere"""
    keys = tuple("%s%d" % (k, a) for k in ("axis", "again") for a in range(3))
    out = {}
    for nranks, per_proc in ((1, 1), (2, 1), (4, 2)):
        out[nranks] = launch_ranks("_profiles_worker.py", nranks, tmp_path, "prof%d" % nranks, [], per_proc=per_proc, agree=keys, timeout=300)
    for nranks in (1, 2, 4):
        for a in range(3):
            assert np.array_equal(out[nranks]["axis%d" % a], out[nranks]["again%d" % a]), (nranks, a)
            assert np.array_equal(out[nranks]["axis%d" % a], out[1]["axis%d" % a]), (nranks, a)
    assert out[1]["axis2"].size == 64 * (1 + 3 + 3 + 3 + 3 + 6 + 2 + 6 + 6 + 1)


def test_refusals(gpu):
    """every refusal of include/varden_amd.h, each followed by a call that succeeds and gives the bits of the first: nothing was left allocated or broken"""
    from varden_amd import capi
    from varden_amd.boxlib import handle_array
    lib = capi.load()
    nbase, boxes = AMR3
    H = hier(_pkg(), nbase, boxes, nscal=2, seed=1)
    nrow = H.pkg.advance.profiles_layout(3, 2)["nrow"]
    rows, cells = np.zeros((nrow, 64)), np.zeros(64, dtype=np.int64)
    dx = (C.c_double * 12)(*[v for lev in H.dx for v in lev] + [1.0] * 3)
    po, pc = rows.ctypes.data_as(C.POINTER(C.c_double)), cells.ctypes.data_as(C.POINTER(C.c_longlong))

    def call(nlev, u, s, dxp, axis, nbins, o=po, c=pc, mla=None):
        rc = lib.vdn_profiles(nlev, (mla or H.mla).h, handle_array(u), handle_array(s), dxp, axis, nbins, o, c)
        return rc, (lib.vdn_last_error() or b"").decode()
    try:
        first = all_bits(profiles(H, 2))
        other = H.bl.MLLayout([((0, 0, 0), (15, 15, 15))], [[((0, 0, 0), (15, 15, 15))]])
        s_other = H.bl.MultiFab(other, 0, 2, 0)
        four = H.u + H.u[:1]
        for args, word in (((0, H.u, H.s, dx, 2, 64), "nlev"), ((5, four + H.u[:1], four + H.s[:1], dx, 2, 64), "nlev"),
                           ((2, H.u, H.s, dx, 2, 32), "does not match"),
                           ((3, H.u, [s_other] + H.s[1:], dx, 2, 64), "layouts of u and s differ"),
                           ((3, H.u, H.s, None, 2, 64), "dx"),
                           ((3, H.u, H.s, dx, 2, 64, None, pc), "null output"), ((3, H.u, H.s, dx, 2, 64, po, None), "null output"),
                           ((3, H.u, H.s, dx, 3, 64), "axis"), ((3, H.u, H.s, dx, -1, 64), "axis"),
                           ((3, H.u, H.s, dx, 2, 63), "nbins"), ((3, H.u, H.s, dx, 2, 16), "nbins")):
            rc, msg = call(*args)
            assert rc != 0 and word in msg and msg.startswith("vdn_profiles"), (args[0], word, rc, msg)
            rc, msg = call(3, H.u, H.s, dx, 2, 64)
            assert rc == 0, msg
            again = np.concatenate([rows.view(np.uint64).ravel(), cells.astype(np.uint64)])
            assert np.array_equal(again, first), word
        assert lib.vdn_profiles_nbins(3, H.mla.h, 3) == -1 and b"axis" in lib.vdn_last_error()
        assert lib.vdn_profiles_nbins(2, H.mla.h, 0) == -1 and lib.vdn_profiles_nbins(3, None, 0) == -1
        assert lib.vdn_profiles_nbins(3, H.mla.h, 1) == 64
        lay = capi.ProfileLayout()
        assert lib.vdn_profiles_layout(4, 2, C.byref(lay)) != 0 and lib.vdn_profiles_layout(3, 12, C.byref(lay)) != 0 and lib.vdn_profiles_layout(3, 2, None) != 0
        s_other.destroy()
        other.destroy()
    finally:
        H.close()
    # dm = 2 runs on one level
    H2 = hier(_pkg(), (16, 16), [[((0, 0, 0), (15, 15, 0))]], phys=[[15, 15], [15, 15]], dm=2, nscal=2)
    try:
        two = H2.bl.MLLayout([((0, 0, 0), (15, 15, 0)), ((0, 0, 0), (31, 31, 0))], [[((0, 0, 0), (15, 15, 0))], [((8, 8, 0), (23, 23, 0))]], rr=[(2, 2, 1)])
        u2 = [H2.bl.MultiFab(two, l, 2, 1) for l in range(2)]
        s2 = [H2.bl.MultiFab(two, l, 2, 1) for l in range(2)]
        rc = lib.vdn_profiles(2, two.h, handle_array(u2), handle_array(s2), dx, 0, 32, po, pc)
        assert rc != 0 and b"dm = 2" in lib.vdn_last_error(), lib.vdn_last_error()
        rc = lib.vdn_profiles(1, H2.mla.h, handle_array(H2.u), handle_array(H2.s), dx, 2, 1, po, pc)
        assert rc != 0 and b"axis" in lib.vdn_last_error(), lib.vdn_last_error()
        P = profiles(H2, 1)
        assert P.rows.shape == (21, 16) and P.cells.sum() == 256
        for m in u2 + s2:
            m.destroy()
        two.destroy()
    finally:
        H2.close()


def _read(path):
    """a profile file: ({header key: value}, column names, rows as strings)"""
    lines = open(path).read().splitlines()
    assert lines[0] == "# VDN_PROFILES 1", lines[0]
    head = {}
    for ln, key in zip(lines[1:6], ("dm", "axis", "nbins", "step", "time")):
        m = re.fullmatch(r"# %s\s*(\S+)" % key, ln)
        assert m, ln
        head[key] = m.group(1)
    assert lines[6].startswith("#")
    return head, lines[6][1:].split(), [ln.split() for ln in lines[7:]]


def test_profile_files_of_an_adaptive_run(gpu, tmp_path):
    """inputs.run on the 32^3 bubble with two levels, prof_int = 2 and diag_int = 1, four steps: a file for step 0 and after every second step, each with 32 << 1 lines
    whatever the grids of the moment; in every file the volumes add up to 1 exactly and the s1 column to the mass on the matching line of the diagnostics file"""
    from varden_amd import advance as adv
    from varden_amd import inputs
    text = open(INPUTS).read()
    nl, G = inputs.run(text, report=None, outdir=str(tmp_path))
    try:
        assert int(nl["prof_int"]) == 2 and int(nl["diag_int"]) == 1 and int(nl["max_step"]) == 4 and G.nlev == 2
        found = sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("prof"))
        assert found == ["prof00000", "prof00002", "prof00004"], found
        cols = ["x", "cells"] + adv.profile_columns(2, 3)
        dcols = ["step", "time", "dt"] + adv.diag_columns(2, 3)
        diag = {int(ln.split()[0]): ln.split() for ln in open(str(tmp_path / "varden_diag.out")).read().splitlines()[1:]}
        for f in found:
            head, names, rows = _read(str(tmp_path / f))
            assert names == cols and head["dm"] == "3" and head["axis"] == "3" and head["nbins"] == "64" and int(head["step"]) == int(f[4:])
            assert len(rows) == 64 and all(len(r) == len(cols) for r in rows)
            assert float(head["time"]) == float(diag[int(f[4:])][1])
            assert [float(r[0]) for r in rows] == [(m + 0.5) / 64 for m in range(64)]
            vol = [float(r[cols.index("volume")]) for r in rows]
            assert math.fsum(vol) == 1.0 and all(v == 1.0 / 64 for v in vol)
            ncell = sum(int(r[1]) for r in rows)
            mass = math.fsum(float(r[cols.index("s1")]) for r in rows)
            dmass, dcells = float(diag[int(f[4:])][dcols.index("sum_s1")]), int(diag[int(f[4:])][dcols.index("cells")])
            # every term is positive: sum |term| is the mass itself
            print("%s: sum of the bins %.17e, diagnostics %.17e, |diff| %.3e, bound %.3e" % (f, mass, dmass, abs(mass - dmass), (dcells + 4) * EPS * dmass))
            assert abs(mass - dmass) <= (dcells + 4) * EPS * dmass and ncell >= dcells
        # the last file holds the figures of a fresh call, digit for digit
        assert open(str(tmp_path / found[-1])).read() == inputs.profile_text(G.profiles(), G.istep, G.time)
    finally:
        G.close()


def test_without_the_key_no_file(gpu, tmp_path):
    from varden_amd import inputs
    text = re.sub(r"(?m)^\s*prof_int\s*=.*$", " prof_int = 0", open(INPUTS).read())
    nl, G = inputs.run(text, nsteps=1, report=None, outdir=str(tmp_path))
    G.close()
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("prof")]
