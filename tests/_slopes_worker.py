"""child process of tests/test_slopes_march_gpu.py: the slope launch of the predictors by itself (vdn_k_slopes_march -> launch_slopes) on every case, under the
launch-form switches of this process's environment (they are read once per process).  One line per case: its name, the SHA-256 of the three slope arrays of
every box (ghost cells included) and of max |u| where the caller asks for it, the form the launch took (vdn_last_slopes_form of the testing build: 0 one thread
per cell, 1 the march with one cell per lane, 2 its pair form) and, with `oracle` as the first argument, the bit-for-bit comparison against the oracle's slope
routine, called box by box and direction by direction the way tests/test_kernels_gpu.py::test_slope calls it."""
import ctypes as C
import hashlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from oracle import voracle as vo
from tests.util import BC_SETS, params_for

# the rows of a workgroup of the pair form (varden_amd/csrc/slopes_plan.h): the cases below are cut to it
R = int(re.search(r"#define SLP_WAVES (\d+)", open(os.path.join(ROOT, "varden_amd", "csrc", "slopes_plan.h")).read()).group(1))


def one(n):
    return n, [((0, 0, 0), tuple(x - 1 for x in n))]


# name -> (cells of the domain, boxes).  The range of a box is the box grown by one: n + 2 cells, (n + 2) / 2 pairs per row, 62 pairs to a full segment.
SHAPES = {
    "8x8x8": one((8, 8, 8)),                          # narrower than any full segment: 5 pairs in 8-lane segments
    "124x4x8": one((124, 4, 8)),                      # one full segment (and one pair beside it), one row group
    "126x7x12": one((126, 7, 12)),                    # a remainder of two pairs, rows no multiple of R
    "132xR1x20": one((132, R + 1, 20)),               # a remainder segment, a second row group of few rows, more than one k-chunk
    "61x5x9": one((61, 5, 9)),                        # odd width: keeps the march with one cell per lane
    "inner": ((16, 16, 16), [((3, 5, 7), (12, 10, 14))]),          # no face on the boundary, odd low corner
    "two": ((126, 8, 8), [((0, 0, 0), (63, 7, 7)), ((64, 0, 0), (125, 7, 7))]),      # a level of two boxes, 64 and 62 wide, side by side
}
ORDERS = (0, 2, 4)
NCS = (3, 2)
# the boundary sets of test_slope, then every kind on every face in turn (the other faces slip walls)
BCS = dict(BC_SETS)
for _d in range(3):
    for _sd in range(2):
        for _k in (11, 12, 15):
            _p = [[14, 14] for _ in range(3)]
            _p[_d][_sd] = _k
            BCS["f%d%d-%d" % (_d, _sd, _k)] = _p
PAIR_FORM = {name: 1 if name == "61x5x9" else 2 for name in SHAPES}      # what the default build must report


def case_name(shape, bc, order, nc):
    return "%s/%s/o%d/c%d" % (shape, bc, order, nc)


def run(shape, bcname, order, mode):
    from varden_amd import advance as adv
    from varden_amd import boxlib as bl
    from varden_amd import capi
    n, boxes = SHAPES[shape]
    phys = BCS[bcname]
    prm = params_for(phys, slope_order=order)
    bl.initialize(prm, 0, 1, 0)
    pmask = [1 if phys[d][0] == -1 else 0 for d in range(3)]
    dom = ((0, 0, 0), tuple(x - 1 for x in n))
    mla = bl.MLLayout([dom], [boxes], pmask=pmask)
    bct = bl.BCTower(mla, phys)
    form_of = capi.load().vdn_last_slopes_form
    form_of.restype, form_of.argtypes = C.c_int, []
    rng = np.random.default_rng(sorted(SHAPES).index(shape) * 1000 + sorted(BCS).index(bcname))
    for nc in NCS:
        bccomp = 0 if nc == 3 else 3
        s = bl.MultiFab(mla, 0, nc, 3)
        src = []
        for i in range(len(boxes)):
            a = np.asfortranarray(rng.standard_normal(s.shape(i)))
            s.from_numpy(a, i)
            src.append(a)
        sl = [bl.MultiFab(mla, 0, nc, 1) for _ in range(3)]
        vmax = adv.slopes_march(s, sl, bccomp, bct, want_max=(nc == 3))
        form = form_of()
        got = [[sl[d].to_numpy(i) for i in range(len(boxes))] for d in range(3)]
        h = hashlib.sha256()
        for d in range(3):
            for g in got[d]:
                h.update(np.ascontiguousarray(g).tobytes())
        if vmax is not None:
            h.update(np.float64(vmax).tobytes())
        verdict = "-"
        if mode == "oracle":
            bad = []
            for i, (lo, hi) in enumerate(boxes):
                pb = [[phys[d][0] if lo[d] == 0 else vo.INTERIOR, phys[d][1] if hi[d] == n[d] - 1 else vo.INTERIOR] for d in range(3)]
                obc = vo.make_bc(pb, 3, prm.nscal)
                osrc = vo.Fab(lo, hi, 3, nc)
                osrc.a[...] = src[i]
                for d in range(3):
                    osl = vo.Fab(lo, hi, 1, nc)
                    vo.lib().vo_slope(osrc.ref, osl.ref, d, nc, bccomp, C.byref(obc), order)
                    if not np.array_equal(got[d][i], osl.a, equal_nan=True):
                        bad.append("box%d:dir%d:%d" % (i, d, int((got[d][i] != osl.a).sum())))
            if vmax is not None:
                want = max(float(np.abs(a[3:-3, 3:-3, 3:-3]).max()) for a in src)
                if vmax != want:
                    bad.append("vmax:%r!=%r" % (vmax, want))
            verdict = "ok:" if not bad else "FAIL:" + ",".join(bad)
        print("CASE %s %s %d %s" % (case_name(shape, bcname, order, nc), h.hexdigest(), form, verdict), flush=True)
        for m in sl + [s]:
            m.destroy()
    bct.destroy()
    mla.destroy()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "plain"
    for order in ORDERS:
        for shape in SHAPES:
            for bcname in BCS:
                run(shape, bcname, order, mode)
