"""Refinement criteria chosen at run time on the device: vdn_tag_boxes_by / vdn_make_new_grids_by (varden_amd/csrc/grids.hip: kk_tag_by) through advance.tag_boxes_by,
advance.make_new_grids_by, VardenAMR(tag_criteria=...), the namelist keys of inputs.py -- every bitmap against numpy or against vdn_tag_boxes, exactly."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.children import launch_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs", "inputs_vortextube_3d_amr")
INF = float("inf")
# one boundary set from each family of the reference-kernel cases (tests/refcases.py: BC3 / BC2): inflow, no-slip, slip, outlet (with an inlet opposite), periodic
BC3 = {"inlets": [[11, 11]] * 3, "walls": [[15, 15]] * 3, "slip": [[14, 14]] * 3, "inout": [[11, 12], [14, 14], [15, 15]], "periodic": [[-1, -1]] * 3}
BC2 = {"inlets": [[11, 11]] * 2, "walls": [[15, 15]] * 2, "slip": [[14, 14]] * 2, "inout": [[11, 12], [14, 15]], "periodic": [[-1, -1]] * 2}
LO3, N3 = (8, 4, 12), (12, 16, 20)          # not at the origin; three different extents, so three different dx
N2 = (16, 12)


@pytest.fixture(autouse=True)
def _default_runtime_afterwards(gpu):
    """tests here initialise the runtime with their own parameters (dm = 2, prob_type, inflow data): the session's defaults come back afterwards"""
    yield
    from varden_amd.capi import default_params
    gpu.initialize(default_params(), 0, 1, 0)


def params_for(dm, phys, **kw):
    """inflow data on the inlet faces (the normal velocity points inwards), as tests/refcases.py: params gives its plain sets"""
    from varden_amd.capi import default_params
    p = default_params(dm=dm, **kw)
    vel = [p.u_bc, p.v_bc, p.w_bc]
    for d in range(dm):
        for s in range(2):
            if phys[d][s] == 11:
                vel[d][d][s] = 1.0 if s == 0 else -1.0
                vel[(d + 1) % dm][d][s] = 0.25
    return p


class Level:
    """one level in one or several boxes: layout, bc tower, multifabs filled from arrays over the level's domain"""

    def __init__(self, bl, dm, lo, n, phys, boxes=None, prm=None):
        self.bl, self.dm = bl, dm
        self.lo = tuple(lo) + (0,) * (3 - len(lo))
        self.n = tuple(n) + (1,) * (3 - len(n))
        self.hi = tuple(self.lo[d] + self.n[d] - 1 for d in range(3))
        self.phys = [list(phys[d]) if d < dm else [0, 0] for d in range(3)]
        bl.initialize(prm if prm is not None else params_for(dm, self.phys), 0, 1, 0)
        self.boxes = boxes or [(self.lo, self.hi)]
        self.mla = bl.MLLayout([(self.lo, self.hi)], [self.boxes], pmask=[1 if self.phys[d][0] == -1 else 0 for d in range(3)])
        self.bct = bl.BCTower(self.mla, self.phys)
        self.dx = [1.0 / self.n[d] for d in range(dm)]
        self.mfs = []

    def mf(self, nc, ng, valid=None, rng=None):
        """a multifab; valid: its valid cells from an array over the level's domain (ghost cells random when rng is given, else zero)"""
        m = self.bl.MultiFab(self.mla, 0, nc, ng)
        self.mfs.append(m)
        if valid is not None:
            for i, (blo, bhi) in enumerate(self.boxes):
                shp = m.shape(i)
                a = np.zeros(shp, order="F") if rng is None else np.asfortranarray(rng.uniform(-1.0, 1.0, shp))
                g = [ng if shp[d] > bhi[d] - blo[d] + 1 else 0 for d in range(3)]
                sl = tuple(slice(g[d], shp[d] - g[d]) for d in range(3))
                a[sl] = valid[tuple(slice(blo[d] - self.lo[d], bhi[d] - self.lo[d] + 1) for d in range(3))]
                m.from_numpy(a, i)
        return m

    def valid(self, m):
        """the valid cells of a multifab as one array over the level's domain"""
        out = np.full(self.n + (m.nc,), np.nan)
        for i, (blo, bhi) in enumerate(self.boxes):
            a = m.to_numpy(i)
            g = [m.ng if a.shape[d] > bhi[d] - blo[d] + 1 else 0 for d in range(3)]
            out[tuple(slice(blo[d] - self.lo[d], bhi[d] - self.lo[d] + 1) for d in range(3))] = a[tuple(slice(g[d], a.shape[d] - g[d]) for d in range(3))]
        return out

    def close(self):
        for m in self.mfs:
            m.destroy()
        self.bct.destroy()
        self.mla.destroy()


def threshold_field(n, seed):
    """a density that crosses every threshold of tag_boxes.f90 (1.01, 1.1, 1.5; 1.2 .. 1.8) with cells exactly ON each of them (tests/test_amr_gpu.py:651-656)"""
    rng = np.random.default_rng(seed)
    ax = [(np.arange(m) + 0.5) / m for m in n]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    v = 1.4 + 0.55 * np.sin(2.0 * np.pi * X) * np.cos(2.0 * np.pi * Y) * np.cos(np.pi * Z) + 0.01 * rng.random(X.shape)
    v[0, 0, 0], v[1, 0, 0], v[2, 0, 0], v[3, 0, 0], v[4, 0, 0], v[5, 0, 0] = 1.01, 1.1, 1.5, 1.2, 1.8, np.nextafter(1.01, 2.0)
    v[0, 1, 0], v[1, 1, 0], v[2, 1, 0] = np.nextafter(1.8, 0.0), np.nextafter(1.2, 2.0), np.nextafter(1.5, 2.0)
    return v


REFERENCE_RULE = {1: [dict(field="scalar", comp=1, gt=(1.01, 1.1, 1.5, 1.5))], 2: [dict(field="scalar", comp=1, gt=(1.01, 1.1, 1.5, 1.5))],
                  3: [dict(field="scalar", comp=1, gt=1.2, lt=1.8)]}


@pytest.mark.parametrize("dm", [3, 2])
def test_reference_rules_as_criteria_equal_tag_boxes(gpu, dm):
    """1. the rules of src/tag_boxes.f90 written as criteria give vdn_tag_boxes' bitmap byte for byte: prob_type 1 - 3, levels 1 - 3, both layouts; u = NULL"""
    from varden_amd import advance as adv
    phys = BC3["walls"] if dm == 3 else BC2["walls"]
    K = Level(gpu, dm, LO3 if dm == 3 else (0, 0), N3 if dm == 3 else N2, phys)
    v = threshold_field(K.n, 11)
    s = K.mf(2, 3, np.stack([v, 3.0 - v], axis=-1))
    for prob_type in (1, 2, 3):
        gpu.initialize(params_for(dm, K.phys, prob_type=prob_type), 0, 1, 0)
        for lev in (1, 2, 3):
            ref = adv.tag_boxes(s, lev)
            got = adv.tag_boxes_by(s, None, None, None, lev, REFERENCE_RULE[prob_type])
            print("prob_type %d lev %d: %d of %d tagged" % (prob_type, lev, ref.sum(), ref.size))
            assert 0 < ref.sum() < ref.size
            assert got.dtype == np.uint8 and np.array_equal(got, ref), (dm, prob_type, lev)
    gpu.initialize(params_for(dm, K.phys, prob_type=4), 0, 1, 0)                 # the pinned refusal stays, the criteria do not care
    with pytest.raises(Exception, match="unsupported prob_type 4"):
        adv.tag_boxes(s, 1)
    assert np.array_equal(adv.tag_boxes_by(s, None, None, None, 1, REFERENCE_RULE[1]), (v > 1.01).astype(np.uint8))
    K.close()


@pytest.mark.parametrize("bc", sorted(BC3))
@pytest.mark.parametrize("dm", [3, 2])
def test_velocity_criteria_equal_thresholds_of_the_stored_fields(gpu, dm, bc):
    """2. vorticity and magvel criteria: the bitmap is numpy's thresholding of what make_vorticity / make_magvel STORE for the same u (the same device arithmetic,
    one-sided differences next to inflow and wall faces included) -- exactly.  Thresholds: the median and the 0.9-quantile of the stored field."""
    from varden_amd import advance as adv
    phys = (BC3 if dm == 3 else BC2)[bc]
    K = Level(gpu, dm, LO3 if dm == 3 else (0, 0), N3 if dm == 3 else N2, phys)
    rng = np.random.default_rng(100 * dm + sorted(BC3).index(bc))
    u = K.mf(dm, 3, rng.uniform(-1.0, 1.0, K.n + (dm,)), rng=rng)
    s = K.mf(2, 0)
    out = K.mf(2, 0)
    adv.make_magvel(out, 0, u)
    adv.make_vorticity(out, 1, u, K.dx, K.bct)
    stored = K.valid(out)
    mag, vort = stored[..., 0], (stored[..., 1] if dm == 3 else np.abs(stored[..., 1]))
    for name, f in (("vorticity", vort), ("magvel", mag)):
        med, q9 = float(np.quantile(f, 0.5)), float(np.quantile(f, 0.9))
        for gt, lt in ((med, None), (None, med), (med, q9), (q9, None)):
            exp = np.ones(f.shape, dtype=bool)
            if gt is not None:
                exp &= f > gt
            if lt is not None:
                exp &= f < lt
            got = adv.tag_boxes_by(s, u, K.dx, K.bct, 1, [dict(field=name, gt=gt, lt=lt)])
            print("%s dm %d %s gt %r lt %r: %d of %d" % (bc, dm, name, gt, lt, exp.sum(), exp.size))
            assert 0 < exp.sum() < exp.size
            assert np.array_equal(got.astype(bool), exp), (bc, dm, name, gt, lt, int((got.astype(bool) != exp).sum()))
    # strictness: a threshold that IS a stored value does not tag its own cell
    top = float(vort.max())
    assert adv.tag_boxes_by(s, u, K.dx, K.bct, 1, [dict(field="vorticity", gt=top)]).sum() == 0
    assert adv.tag_boxes_by(s, u, K.dx, K.bct, 1, [dict(field="vorticity", gt=np.nextafter(top, 0.0))]).sum() == (vort == top).sum()
    K.close()


def numpy_grad(a, dm):
    """max over d < dm of max(|s(i+e_d) - s(i)|, |s(i) - s(i-e_d)|) on the cells that have both neighbours in `a` (one layer is shaved off the dm directions)"""
    core = tuple(slice(1, -1) if d < dm else slice(None) for d in range(3))
    c = a[core]
    out = np.zeros(c.shape)
    for d in range(dm):
        up = a[tuple(slice(2, None) if t == d else core[t] for t in range(3))]
        um = a[tuple(slice(0, -2) if t == d else core[t] for t in range(3))]
        out = np.maximum(out, np.maximum(np.abs(up - c), np.abs(c - um)))
    return out


@pytest.mark.parametrize("dm", [3, 2])
def test_gradient_criterion_against_numpy_and_across_box_faces(gpu, dm):
    """3. the undivided-gradient criterion against a numpy restatement (each term is one subtraction: exact), on a random field with physical and periodic sides;
    the same level in one box and in 8 boxes of 8^3 (dm = 2: four of 8 x 8) with filled ghost cells gives the same bitmap -- the reads across box faces."""
    from varden_amd import advance as adv
    n = (16, 16, 16) if dm == 3 else (16, 16)
    phys = [[-1, -1], [14, 15], [12, 11]][:dm] if dm == 3 else [[-1, -1], [15, 12]]
    rng = np.random.default_rng(7 + dm)
    field = rng.uniform(1.0, 2.0, tuple(n) + (1,) * (3 - dm) + (2,))
    maps = []
    for split in (False, True):
        boxes = None
        if split:
            r2 = (0, 8) if dm == 3 else (0,)
            boxes = [((i, j, k), (i + 7, j + 7, k + 7 if dm == 3 else 0)) for k in r2 for j in (0, 8) for i in (0, 8)]
        K = Level(gpu, dm, (0,) * dm, n, phys, boxes=boxes)
        s = K.mf(2, 1, field)
        s.fill_boundary()
        s.physbc(0, dm, 2, K.bct)
        if not split:
            a = s.to_numpy(0)[..., 1]                                  # comp 2, ghost layer included (dm = 2: one plane, no ghost cells along z)
            g = numpy_grad(a, dm)
            thr = float(np.median(g))
        got = adv.tag_boxes_by(s, None, None, None, 1, [dict(field="scalar_grad", comp=2, gt=thr)])
        print("gradient dm %d %s: %d of %d tagged" % (dm, "split" if split else "one box", got.sum(), got.size))
        assert np.array_equal(got.astype(bool), g > thr), int((got.astype(bool) != (g > thr)).sum())
        assert 0 < got.sum() < got.size
        maps.append(got)
        K.close()
    assert np.array_equal(maps[0], maps[1])


def test_combination_levels_open_sides_and_refusals(gpu):
    """4. criteria OR together; thresholds are per level; +-HUGE_VAL opens a side; gt = +inf switches a criterion off; a NaN tags nothing; every refusal of the
    header returns non-zero with a message; scalar rules run with u = NULL"""
    from varden_amd import advance as adv, capi
    K = Level(gpu, 3, LO3, N3, BC3["walls"])
    rng = np.random.default_rng(3)
    sv = rng.uniform(1.0, 2.0, K.n + (2,))
    sv[3, 4, 5, 0] = np.nan
    s = K.mf(2, 1, sv)
    u = K.mf(3, 1, rng.uniform(-1.0, 1.0, K.n + (3,)))
    mv = K.mf(1, 0)
    adv.make_magvel(mv, 0, u)
    mag = K.valid(mv)[..., 0]
    with np.errstate(invalid="ignore"):
        a, b = sv[..., 0] > 1.7, mag < 0.6
        two = adv.tag_boxes_by(s, u, K.dx, K.bct, 1, [dict(field="scalar", gt=1.7), dict(field="magvel", lt=0.6)]).astype(bool)
        assert np.array_equal(two, a | b) and (a & ~b).any() and (b & ~a).any()
        crit = [dict(field="scalar", comp=2, gt=[1.2, 1.6], lt=[INF, 1.9])]
        l1, l2, l4 = (adv.tag_boxes_by(s, None, None, None, lev, crit).astype(bool) for lev in (1, 2, 4))
        assert np.array_equal(l1, sv[..., 1] > 1.2) and np.array_equal(l2, (sv[..., 1] > 1.6) & (sv[..., 1] < 1.9)) and np.array_equal(l4, l2) and not np.array_equal(l1, l2)
        every = adv.tag_boxes_by(s, None, None, None, 1, [dict(field="scalar", gt=-INF, lt=INF)])
        assert every.sum() == every.size - 1 and every[3, 4, 5] == 0                          # both sides open: everything but the NaN
        assert np.array_equal(adv.tag_boxes_by(s, None, None, None, 1, [dict(field="scalar", lt=1.5)]).astype(bool), sv[..., 0] < 1.5)
    assert adv.tag_boxes_by(s, None, None, None, 1, [dict(field="scalar", gt=INF)]).sum() == 0
    assert np.array_equal(adv.tag_boxes_by(s, u, K.dx, K.bct, 1, [dict(field="scalar", gt=INF), dict(field="magvel", lt=0.6)]).astype(bool), b)
    # refusals
    lib = capi.load()
    tags = np.zeros(K.n, dtype=np.uint8, order="F")
    tp = tags.ctypes.data_as(C.POINTER(C.c_ubyte))
    dx = (C.c_double * 3)(*K.dx)
    one, _ = adv.tag_criteria([dict(field="scalar", gt=1.5)])

    def refused(rc, *words):
        msg = (lib.vdn_last_error() or b"").decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg)
    bad = capi.TagCriterion(); bad.field = 7
    refused(lib.vdn_tag_boxes_by(s.h, u.h, dx, K.bct.h, 1, 1, (capi.TagCriterion * 1)(bad), tp), "unknown field")
    for comp in (0, 3):
        with pytest.raises(capi.VardenError, match="component"):
            adv.tag_boxes_by(s, None, None, None, 1, [dict(field="scalar", comp=comp, gt=1.0)])
    for ncrit in (0, 9, -1):
        refused(lib.vdn_tag_boxes_by(s.h, None, None, None, 1, ncrit, one, tp), "criteria")
    for name in ("vorticity", "magvel"):
        with pytest.raises(capi.VardenError, match="u is null"):
            adv.tag_boxes_by(s, None, K.dx, K.bct, 1, [dict(field=name, gt=0.0)])
    s0 = K.mf(2, 0, sv)
    with pytest.raises(capi.VardenError, match="ghost"):
        adv.tag_boxes_by(s0, None, None, None, 1, [dict(field="scalar_grad", gt=0.1)])
    boxes = (capi.Box * 8)()
    nb, nt = C.c_int(), C.c_long()
    refused(lib.vdn_make_new_grids_by(s.h, None, None, None, 1, 0, one, 2, 0, 0.9, 4, 4, 32, 8, boxes, C.byref(nb), C.byref(nt)), "vdn_make_new_grids_by", "criteria")
    refused(lib.vdn_make_new_grids_by(s.h, None, None, None, 1, 1, one, 2, 0, 0.9, 4, 64, 32, 8, boxes, C.byref(nb), C.byref(nt)), "clustering")
    assert adv.tag_boxes_by(s0, None, None, None, 1, [dict(field="scalar", gt=1.5)]).sum() == (sv[..., 0] > 1.5).sum()   # still usable after the refusals
    K.close()


def _dilate(a, w, periodic):
    out = a.copy()
    for d in range(3):
        src = out.copy()
        for k in range(1, w + 1):
            for sh in (k, -k):
                r = np.roll(src, sh, axis=d)
                if not periodic[d]:
                    idx = [slice(None)] * 3
                    idx[d] = slice(0, sh) if sh > 0 else slice(sh, None)
                    r[tuple(idx)] = False
                out |= r
    return out


def _covered(boxes, n, rr=2):
    fine = np.zeros(tuple(rr * m for m in n), dtype=np.int32)
    for lo, hi in boxes:
        fine[tuple(slice(lo[d], hi[d] + 1) for d in range(3))] += 1
    return fine


def test_make_new_grids_by_equals_make_new_grids_and_keeps_its_properties(gpu):
    """5. with the reference rule vdn_make_new_grids_by returns vdn_make_new_grids' boxes, in its order, and its tag count (a 32^3 blob on level 2 of a hierarchy,
    nest = 2); with a vorticity rule every tagged cell, grown by buf_wid and clipped to the nesting region, is covered by disjoint, blocking-aligned boxes of at
    most max_grid_size cells a side"""
    from varden_amd import advance as adv
    from varden_amd.capi import default_params
    from varden_amd.driver import initdata_numpy
    bl = gpu
    bl.initialize(default_params(), 0, 1, 0)
    walls = [[15, 15]] * 3
    lo, hi = (4, 4, 4), (27, 27, 27)                                              # level 2 (index 1): one box inside the 32^3 index space, nest cells from its edge kept free
    mla = bl.MLLayout([((0, 0, 0), (15,) * 3), ((0, 0, 0), (31,) * 3)], [[((0, 0, 0), (15,) * 3)], [(lo, hi)]], rr=[(2, 2, 2)])
    bct = bl.BCTower(mla, walls)
    n = tuple(hi[d] - lo[d] + 1 for d in range(3))
    h = [1.0 / 32] * 3
    u0, s0 = initdata_numpy(n, h, 1, 3, 2, lo=lo)
    s, u = bl.MultiFab(mla, 1, 2, 3), bl.MultiFab(mla, 1, 3, 3)
    s.from_numpy(s0)
    cl = dict(buf_wid=2, nest=2, min_eff=0.9, min_width=4, blocking=4, max_grid_size=16)
    ref, nref = adv.make_new_grids(s, 2, **cl)
    got, ngot = adv.make_new_grids_by(s, None, None, None, 2, REFERENCE_RULE[1], **cl)
    print("blob: %d tagged, boxes %r" % (nref, ref))
    assert nref > 0 and len(ref) >= 1 and got == ref and ngot == nref
    # a vorticity rule: a vortex ring, strongest off the centre of the level; the ghost cells at the coarse-fine boundary are the caller's (analytic here)
    ax = [h[d] * (lo[d] - 3 + np.arange(n[d] + 6) + 0.5) - 0.5 for d in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    ua = np.zeros(X.shape + (3,), order="F")
    ring = np.exp(-((np.sqrt(X * X + Y * Y) - 0.22) ** 2 + (Z - 0.05) ** 2) / 0.004)
    ua[..., 0], ua[..., 1], ua[..., 2] = -Y * ring, X * ring, 0.3 * ring
    u.from_numpy(ua)
    rule = [dict(field="vorticity", gt=2.0)]
    cl = dict(buf_wid=2, nest=4, min_eff=0.8, min_width=4, blocking=4, max_grid_size=16)   # nest = 4: the nesting region (8 .. 23) ends on block faces
    tags = adv.tag_boxes_by(s, u, h, bct, 2, rule).astype(bool)
    boxes, nt = adv.make_new_grids_by(s, u, h, bct, 2, rule, **cl)
    assert nt == tags.sum() and 0 < nt < tags.size and not tags[:4].any() and not tags[28:].any()
    grown = _dilate(tags, cl["buf_wid"], (False,) * 3)
    inside = np.zeros((32,) * 3, dtype=bool)
    inside[8:24, 8:24, 8:24] = True
    assert (grown & ~inside).any(), "the ring's buffer does not reach the edge of the nesting region: the clip is not tested"
    want = np.repeat(np.repeat(np.repeat(grown & inside, 2, 0), 2, 1), 2, 2)
    fine = _covered(boxes, (32,) * 3)
    print("ring: %d tagged, %d grown and clipped, %d boxes covering %d fine cells" % (nt, (grown & inside).sum(), len(boxes), (fine > 0).sum()))
    assert fine.max() == 1, "boxes overlap"
    assert (fine[want] == 1).all(), "a tagged cell is not covered"
    assert not (fine > 0)[~np.repeat(np.repeat(np.repeat(inside, 2, 0), 2, 1), 2, 2)].any(), "a box leaves the nesting region"
    for blo, bhi in boxes:
        for d in range(3):
            assert blo[d] % 8 == 0 and (bhi[d] + 1) % 8 == 0 and bhi[d] - blo[d] + 1 <= 16, (blo, bhi)
    for m in (s, u):
        m.destroy()
    bct.destroy(); mla.destroy()


@pytest.fixture(scope="module")
def tube():
    """the vortex tube at 32^3: max |curl u| of the initial data by make_vorticity, the threshold (half of it), the numpy tag set and its grown form"""
    from varden_amd import advance as adv, boxlib as bl
    from varden_amd.capi import default_params
    from varden_amd.driver import initdata_numpy
    bl.initialize(default_params(prob_type=4), 0, 1, 0)
    per = [[-1, -1]] * 3
    mla = bl.MLLayout([((0, 0, 0), (31,) * 3)], [[((0, 0, 0), (31,) * 3)]], pmask=(1, 1, 1))
    bct = bl.BCTower(mla, per)
    u, w = bl.MultiFab(mla, 0, 3, 3), bl.MultiFab(mla, 0, 1, 0)
    u0, _ = initdata_numpy((32,) * 3, [1.0 / 32] * 3, 4, 3, 2)
    u.from_numpy(u0)
    adv.make_vorticity(w, 0, u, [1.0 / 32] * 3, bct)
    vort = w.to_numpy(0)[..., 0]
    for m in (u, w):
        m.destroy()
    bct.destroy(); mla.destroy()
    bl.initialize(default_params(), 0, 1, 0)
    thr = 0.5 * float(vort.max())
    return dict(max=float(vort.max()), thr=thr, tags=vort > thr)


def test_the_vortex_tube_refines_on_vorticity(gpu, tube, tmp_path):
    """6. prob_type 4, which tag_boxes.f90 refuses: tagged_grids with one vorticity criterion (half the initial maximum) returns a level 1 that covers the numpy tag
    set grown by the buffer and is not the whole domain; VardenAMR on those grids runs four steps with regrid_int = 2; inputs.run on the project's inputs file is the
    same run; without tag_criteria the set-up still raises"""
    from varden_amd import advance as adv, driver, inputs
    from varden_amd.capi import default_params
    per = [[-1, -1]] * 3
    text = open(INPUTS).read()
    nl = dict(inputs.DEFAULTS); nl.update(inputs.parse_namelist(text))
    crit = inputs.namelist_tag_criteria(nl)
    print("max |curl u| = %r, threshold %r, %d cells tagged" % (tube["max"], tube["thr"], tube["tags"].sum()))
    assert crit == [dict(field="vorticity", comp=1, gt=[tube["thr"]])], (crit, tube["thr"])          # the literal of the inputs file IS half the maximum
    rule = [dict(field="vorticity", gt=[tube["thr"]])]
    prm = lambda: default_params(cflfac=0.9, visc_coef=0.001)                    # noqa: E731
    buf = 2                                                                        # max(amr_buf_width, regrid_int, 1) of the inputs file
    levels = driver.VardenAMR.tagged_grids(32, per, prm(), prob_type=4, max_levs=2, buf_wid=buf, max_grid_size=32, tag_criteria=rule)
    assert len(levels) == 1
    grown = _dilate(tube["tags"], buf, (True,) * 3)
    blocks = grown.reshape(8, 4, 8, 4, 8, 4).any(axis=(1, 3, 5))                  # the blocks of 4^3 cells that hold a grown tag: what clustering must cover
    fine = _covered(levels[0], (32,) * 3)
    expected = int(blocks.sum()) * 64 * 8
    print("level 1: %d boxes, %d fine cells; grown tags %d cells in %d blocks = %d fine cells; domain %d" % (len(levels[0]), (fine > 0).sum(), grown.sum(), blocks.sum(), expected, fine.size))
    assert fine.max() == 1
    assert (fine[np.repeat(np.repeat(np.repeat(grown, 2, 0), 2, 1), 2, 2)] == 1).all()
    assert 0 < expected <= (fine > 0).sum() < fine.size
    # the tube lies along x: the tagged blocks fill their bounding box (checked here), so its efficiency is 1 >= cluster_min_eff, clustering accepts it whole and
    # the level is EXACTLY the grown tag set's blocks
    bb = [np.nonzero(blocks.any(axis=tuple(t for t in range(3) if t != d)))[0] for d in range(3)]
    assert blocks.sum() == np.prod([b.max() - b.min() + 1 for b in bb])
    assert (fine > 0).sum() == expected
    # the boxes hug the tagged blocks: the bounding box of the level is the bounding box of the tagged blocks (clustering starts from it and only cuts)
    for d in range(3):
        occ_b = np.nonzero(blocks.any(axis=tuple(t for t in range(3) if t != d)))[0]
        occ_f = np.nonzero((fine > 0).any(axis=tuple(t for t in range(3) if t != d)))[0]
        assert (occ_f.min(), occ_f.max() + 1) == (8 * occ_b.min(), 8 * (occ_b.max() + 1)), d
    G = driver.VardenAMR(32, levels[0], per, params=prm(), prob_type=4, grav=0.0, init_shrink=1.0, init_iter=1, do_initial_projection=1, regrid_int=2, max_levs=2,
                         max_grid_size=32, amr_buf_width=buf, stop_time=1000.0, tag_criteria=rule)
    assert G.initial_projection_stat[0] < 100 and np.isfinite(G.initial_projection_stat[2])
    rows = []
    for _ in range(4):
        G.step()
        mac, hg = adv.last_solver_stats("mac"), adv.last_solver_stats("hg")
        assert mac[0] < 100 and hg[0] < 100 and np.isfinite(mac[2]) and np.isfinite(hg[2]), (mac, hg)      # both projections converged (abort_on_max_iter would have raised)
        rows.append((G.time, G.dt, [list(b) for b in G.boxes]))
    assert G.nregrids == 2 and G.nlev == 2
    for n in range(G.nlev):
        for mfs in (G.uold, G.sold, G.gp, G.p):
            for i in range(mfs[n].nfabs()):
                assert np.isfinite(mfs[n].to_numpy(i)).all()
    G.close()
    prows = []
    nl, H = inputs.run(text, report=lambda g: prows.append((g.time, g.dt, [list(b) for b in g.boxes])), outdir=str(tmp_path))
    assert H.nregrids == 2 and len(prows) == 4
    for a, b in zip(rows, prows):
        assert abs(a[0] - b[0]) <= 1e-12 * a[0] and abs(a[1] - b[1]) <= 1e-12 * a[1] and a[2] == b[2], (a, b)
    H.close()
    # no behaviour change: without criteria prob_type 4 is refused where it always was
    with pytest.raises(Exception, match="unsupported prob_type 4"):
        driver.VardenAMR.tagged_grids(32, per, prm(), prob_type=4, max_levs=2, buf_wid=buf, max_grid_size=32)


def test_two_ranks_return_the_boxes_of_one(gpu, tmp_path):
    """7. make_new_grids_by with a vorticity rule on a 32^3 level in eight boxes: two ranks (the RCCL test double) both return the boxes one rank returns -- the
    bitmap is ORed over the ranks before anything is clustered"""
    one = launch_ranks("_tag_criteria_worker.py", 1, tmp_path, "tc1", (), agree=("boxes", "ntagged", "tags"))
    two = launch_ranks("_tag_criteria_worker.py", 2, tmp_path, "tc2", (), agree=("boxes", "ntagged", "tags"))
    print("one rank: %d tagged, %d boxes" % (one["ntagged"][0], len(one["boxes"])))
    assert one["ntagged"][0] > 0 and len(one["boxes"]) >= 1 and 0 < one["tags"].sum() < one["tags"].size
    assert np.array_equal(one["boxes"], two["boxes"]) and np.array_equal(one["ntagged"], two["ntagged"]) and np.array_equal(one["tags"], two["tags"])
