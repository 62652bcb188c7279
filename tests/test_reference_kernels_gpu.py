"""The HIP kernels, through the C-ABI, against the RECORDED results of the reference's own routines (tests/golden/reference_kernels.json, written by
tests/test_reference_kernels_cpu.py from oracle/_ref/libvref.so): the same cases, the same input bytes, the SHA-256 of the same compared region.  Needs
neither the reference tree nor oracle/_ref/.

Every routine of tests/refcases.py is held: slope, velpred, mkflux, update, mkvelforce, mkscalforce, estdt, physbc, make_at_halftime, make_vorticity,
make_magvel and tag_boxes, 2-D and 3-D.  The C-ABI calls of the two forces and of make_at_halftime include the ghost fill that the reference's drivers
apply to the result, so they are held to the `<case>#filled` hashes: the reference routine's output after that same fill.

How a case's box is laid out on the device:
  * a box with physical (or periodic) sides is its own domain, also where it does not start at the origin (lo = (8, 4, 12));
  * the box-interior box of dm = 3 (INTERIOR on all six faces) is the only box of a level whose domain is larger on every side.
    A dm = 2 level must cover its domain (dim2.hip refuses others), so the C-ABI cannot express a 2-D box with interior sides: the 18 2-D `interior` cases are
    held through the oracle only (tests/test_reference_kernels_cpu.py); they are listed in NOT_EXPRESSIBLE below and nowhere else."""
import json
import os

import numpy as np
import pytest

from tests import refcases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_kernels.json")
NOT_EXPRESSIBLE = [cid for cid, s in rc.CASES.items() if s["dm"] == 2 and s.get("bc") == "interior"]
IDS = [cid for cid in rc.CASES if cid not in NOT_EXPRESSIBLE]


class Gpu:
    """the `how` of tests.refcases: one box on the device"""

    def __init__(self, K):
        from varden_amd import advance as adv, boxlib as bl
        self.adv, self.bl, self.K = adv, bl, K
        if K.spec["routine"] == "tag_boxes":
            K.prm.prob_type = K.spec["prob_type"]
        bl.initialize(K.prm, 0, 1, 0)
        if K.bcname == "interior":
            assert min(K.lo) >= 4
            pd = ((0, 0, 0), tuple(K.hi[d] + 8 for d in range(3)))
            phys = [[15, 15]] * 3                                   # the domain's walls are nowhere near the box
        else:
            pd, phys = (K.lo, K.hi), K.phys3
        self.mla = bl.MLLayout([pd], [[(K.lo, K.hi)]], pmask=K.pmask)
        self.bct = bl.BCTower(self.mla, phys)
        for d in range(K.dm):
            for s in range(2):
                assert self.bct.phys(0, 1, d, s) == K.phys3[d][s]          # grid 0 is the domain, grid 1 the box
        self.mfs = []

    def mf(self, f):
        m = self.bl.MultiFab(self.mla, 0, f.nc, f.ng, f.nodal)
        m.from_numpy(f.a)
        self.mfs.append(m)
        return m

    def close(self):
        for m in self.mfs:
            m.destroy()
        self.bct.destroy(); self.mla.destroy()

    def slope(self, K, src, d, bccomp):
        out = self.mf(K.fab(1, src.nc))
        self.adv.slope(self.mf(src), out, d, bccomp, self.bct)
        return out.to_numpy()

    def velpred(self, K, u, um, force, dt):
        g = [self.mf(f) for f in um]
        self.adv.velpred(self.mf(u), g, self.mf(force), K.dx, dt, self.bct)
        for f, m in zip(um, g):
            f.a[...] = m.to_numpy()

    def mkflux(self, K, src, se, fl, um, force, rhs, dt, is_vel, cons):
        gse, gfl = [self.mf(f) for f in se], [self.mf(f) for f in fl]
        self.adv.mkflux(self.mf(src), gse, gfl, [self.mf(f) for f in um], self.mf(force), self.mf(rhs), K.dx, dt, self.bct, is_vel, cons)
        for f, m in zip(se + fl, gse + gfl):
            f.a[...] = m.to_numpy()

    def update(self, K, sold, um, se, fl, force, snew, dt, is_vel, cons):
        g = self.mf(snew)
        self.adv.update(self.mf(sold), [self.mf(f) for f in um], [self.mf(f) for f in se], [self.mf(f) for f in fl], self.mf(force), g, K.dx, dt, is_vel, cons, self.bct)
        snew.a[...] = g.to_numpy()

    def mkvelforce(self, K, vf, ext, gp, s, lapu, visc_fac):
        g = self.mf(vf)
        self.adv.mkvelforce(g, self.mf(ext), self.mf(s), self.mf(gp), self.mf(lapu), visc_fac, self.bct)
        vf.a[...] = g.to_numpy()

    def mkscalforce(self, K, sf, ext, laps, diff_fac):
        g = self.mf(sf)
        self.adv.mkscalforce(g, self.mf(ext), self.mf(laps), diff_fac, self.bct)
        sf.a[...] = g.to_numpy()

    def halftime(self, K, rh, s0, s1):
        g = self.mf(rh)
        self.adv.make_at_halftime(g, self.mf(s0), self.mf(s1), 0, 0, self.bct)
        rh.a[...] = g.to_numpy()

    def plot(self, K, out, u):
        g = self.mf(out)
        gu = self.mf(u)
        self.adv.make_magvel(g, 0, gu)
        self.adv.make_vorticity(g, 1, gu, K.dx, self.bct)
        out.a[...] = g.to_numpy()

    def tag(self, K, s, lev, pt, tags):
        try:
            t = self.adv.tag_boxes(self.mf(s), lev)
        except Exception:                                           # an unknown prob_type: the call is refused, as bl_error does; no cell is tagged
            return 1
        lo = [K.lo[d] - self.mla.pd[0][0][d] for d in range(3)]
        tags[...] = t[lo[0]:lo[0] + K.n[0], lo[1]:lo[1] + K.n[1], lo[2]:lo[2] + K.n[2]]
        assert t.sum() == tags.sum()
        return 0

    def physbc(self, K, u, s):
        for f, b in ((u, 0), (s, K.dm)):
            g = self.mf(f)
            g.physbc(0, b, f.nc, self.bct)
            f.a[...] = g.to_numpy()

    def estdt(self, K, u, s, gp, ext, dtold):
        return self.adv.estdt(1, self.mf(u), self.mf(s), self.mf(gp), self.mf(ext), K.dx, dtold)


def test_every_case_is_held_or_cannot_be_expressed():
    assert len(IDS) + len(NOT_EXPRESSIBLE) == len(rc.CASES) and len(NOT_EXPRESSIBLE) == sum(1 for s in rc.CASES.values() if s["dm"] == 2 and s.get("bc") == "interior")
    assert {rc.CASES[c]["routine"] for c in IDS} == set(rc.RUN)


@pytest.mark.parametrize("cid", IDS)
def test_hip_matches_recorded_reference(gpu, cid):
    with open(GOLDEN) as f:
        golden = json.load(f)
    K = rc.Ctx(rc.CASES[cid])
    G = Gpu(K)
    try:
        out = rc.RUN[K.spec["routine"]](K, G)
    finally:
        G.close()
        del rc._KEEP[:]
    assert all(np.isfinite(a).all() for _, a in out if a.dtype == np.float64)
    key = cid + "#filled" if rc.filled_only(out) else cid
    assert rc.digest(out) == golden[key], "%s: the HIP kernels' output is not the reference's recorded output" % cid
