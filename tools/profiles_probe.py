#!/usr/bin/env python
"""What one call of the plane-averaged profiles costs (vdn_profiles, csrc/profiles.hip), wall-clock per call (every call ends in its one read-back), for each of
the three axes, on

  one      a 256^3 level in one box
  amr3     the three-level hierarchy of tests/golden/amr_grids_256_l3.json (a 256^3 base in one box, 263 and 997 boxes above it): 1024 bins

next to the route a user has without the entry:

  (h) host copy + numpy      to_numpy() of every box of every level, a composite mask from the box lists, numpy.bincount per sum row (weights = term) over the
                             bin index of every cell and level, minima and maxima per plane.  This Python depends on the library only through to_numpy(), so
                             it runs the same on a build without the entry: --lib <the parent commit's libvarden_amd.so> --only-host

The bytes a call must read are (dm + nscal) * 8 B per composite cell; the table gives them per second and as a fraction of the 8 TB/s HBM peak the README uses.
The fields are constants set on the device: the time of neither route depends on the values.

    python tools/profiles_probe.py [--repeats 5] [--host-repeats 2] [--grids one,amr3] [--no-host] [--out profiles/profiles_probe.txt]
    python tools/profiles_probe.py --lib <libvarden_amd.so of another build> --only-host"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
ENTRIES = ("vdn_profiles_layout", "vdn_profile_layout_sizeof", "vdn_profiles_nbins", "vdn_profiles")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--grids", default="one,amr3")
    ap.add_argument("--lib", default=None, help="another build of libvarden_amd.so")
    ap.add_argument("--only-host", action="store_true", help="(h) only: a build without vdn_profiles")
    ap.add_argument("--no-host", action="store_true", help="leave (h) out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from varden_amd import capi
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    if a.only_host:
        for name in ENTRIES:
            capi.SIGNATURES.pop(name)
    from varden_amd import advance as adv, boxlib as bl
    prm = capi.default_params()
    dm, ns = prm.dm, prm.nscal
    bl.initialize(prm, 0, 1, 0)
    n = 256
    text = []
    for grid in a.grids.split(","):
        boxes = [[((0, 0, 0), (n - 1,) * 3)]]
        if grid == "amr3":
            boxes += [[(tuple(b[0]), tuple(b[1])) for b in lev] for lev in json.load(open(os.path.join(ROOT, "tests", "golden", "amr_grids_256_l3.json")))]
        NL = len(boxes)
        L = NL - 1
        mla = bl.MLLayout([((0, 0, 0), ((n << l) - 1,) * 3) for l in range(NL)], boxes, rr=[(2, 2, 2)] * L)
        dx = [[1.0 / (n << l)] * 3 for l in range(NL)]
        u, s = [bl.MultiFab(mla, l, dm, 1) for l in range(NL)], [bl.MultiFab(mla, l, ns, 1) for l in range(NL)]
        for l in range(NL):
            for c in range(dm):
                u[l].setval(0.25 * (c + 1) - 0.5, c, 1, all=True)
            for c in range(ns):
                s[l].setval(1.0 + 0.5 * c, c, 1, all=True)
        nbins = n << L

        def host(axis):
            """the sum rows, the extrema and the counts of vdn_profiles along `axis`, from host copies"""
            other = tuple(d for d in range(3) if d != axis)
            nsum = 1 + 2 * ns + 2 * dm + dm * (dm + 1) // 2 + ns - 1
            rows, cells = np.zeros((nsum, nbins)), np.zeros(nbins, dtype=np.int64)
            lo_rows, hi_rows = np.full((ns + dm, nbins), np.inf), np.full((ns + dm, nbins), -np.inf)
            for l in range(NL):
                r = 1 << (L - l)
                w = float(np.prod(dx[l])) / r
                for i in range(u[l].nfabs()):
                    lo, hi = u[l].get_box(i)
                    uv, sv = u[l].to_numpy(i)[1:-1, 1:-1, 1:-1], s[l].to_numpy(i)[1:-1, 1:-1, 1:-1]
                    mask = np.ones(uv.shape[:3], dtype=bool)
                    if l < L:
                        for flo, fhi in boxes[l + 1]:
                            a0 = [max(flo[d] // 2, lo[d]) - lo[d] for d in range(3)]
                            a1 = [min(fhi[d] // 2, hi[d]) - lo[d] for d in range(3)]
                            if all(a0[d] <= a1[d] for d in range(3)):
                                mask[a0[0]:a1[0] + 1, a0[1]:a1[1] + 1, a0[2]:a1[2] + 1] = False
                    idx = np.broadcast_to(np.arange(lo[axis], hi[axis] + 1).reshape([-1 if d == axis else 1 for d in range(3)]), mask.shape)[mask]
                    um, sm = uv[mask], sv[mask]
                    terms = [np.full(idx.shape, w)] + [sm[:, c] * w for c in range(ns)] + [(sm[:, c] * sm[:, c]) * w for c in range(ns)]
                    terms += [um[:, d] * w for d in range(dm)] + [(sm[:, 0] * um[:, d]) * w for d in range(dm)]
                    terms += [((sm[:, 0] * um[:, d]) * um[:, e]) * w for d in range(dm) for e in range(d, dm)] + [(sm[:, c] * um[:, axis]) * w for c in range(1, ns)]
                    n0 = hi[axis] - lo[axis] + 1
                    sl = slice(lo[axis] * r, (hi[axis] + 1) * r)
                    for q, t in enumerate(terms):
                        rows[q, sl] += np.repeat(np.bincount(idx - lo[axis], weights=t, minlength=n0), r)
                    cells[sl] += np.repeat(np.bincount(idx - lo[axis], minlength=n0), r)
                    both = np.concatenate([sv, uv], axis=3)
                    lo_rows[:, sl] = np.minimum(lo_rows[:, sl], np.repeat(np.where(mask[..., None], both, np.inf).min(axis=other).T, r, axis=1))
                    hi_rows[:, sl] = np.maximum(hi_rows[:, sl], np.repeat(np.where(mask[..., None], both, -np.inf).max(axis=other).T, r, axis=1))
            return rows, cells, lo_rows, hi_rows

        runs = []
        if not a.only_host:
            runs += [("profiles, axis %d (%s)" % (ax, "xyz"[ax]), (lambda ax=ax: adv.profiles(mla, u, s, dx, ax))) for ax in range(3)]
        res = {name: fn() for name, fn in runs}                                           # warm-up (and the results)
        times = {name: [] for name, _ in runs}
        for r in range(a.repeats):
            for name, fn in runs[r % max(1, len(runs)):] + runs[:r % max(1, len(runs))]:
                capi.check(capi.load().vdn_device_synchronize())
                t0 = time.perf_counter()
                fn()
                times[name].append(1e3 * (time.perf_counter() - t0))
        hname = "(h) to_numpy + mask + numpy.bincount, axis 2"
        if not a.no_host:
            times[hname] = []
            for r in range(a.host_repeats):
                capi.check(capi.load().vdn_device_synchronize())
                t0 = time.perf_counter()
                hres = host(2)
                times[hname].append(1e3 * (time.perf_counter() - t0))
            runs.append((hname, None))
        cells = sum(int(np.prod([hi[k] - lo[k] + 1 for k in range(3)])) for lev in boxes for lo, hi in lev)
        cells -= sum(int(np.prod([hi[k] - lo[k] + 1 for k in range(3)])) // 8 for lev in boxes[1:] for lo, hi in lev)
        if not a.only_host:
            for ax in range(3):
                P = res[runs[ax][0]]
                assert len(P.x) == nbins and abs(P["volume"].sum() - 1.0) < 1e-9 and (P["volume"] == 1.0 / nbins).all(), ax
            if not a.no_host:                                                             # the two routes agree
                P = res[runs[2][0]]
                assert np.array_equal(P.cells, hres[1]) and np.allclose(P.rows[:hres[0].shape[0]], hres[0], rtol=1e-12, atol=0.0)
                assert np.array_equal(P.rows[hres[0].shape[0]:], np.concatenate([hres[2][:ns], hres[3][:ns], hres[2][ns:], hres[3][ns:]]))
        nbytes = (dm + ns) * 8 * cells
        text += ["profiles_probe %s: %d level(s), boxes %s, %d composite cells, %d bins, (dm + nscal) * 8 B * cells = %.1f MB; %d timed calls each after a warm-up (host route: %d, "
                 "no warm-up); library %s (%s)" % (grid, NL, [len(b) for b in boxes], cells, nbins, nbytes / 1e6, a.repeats, a.host_repeats,
                                                  os.path.relpath(capi.LIB_PATH, ROOT), capi.load().vdn_build_flavour().decode()),
                 "%-48s %9s %9s %9s %9s %9s" % ("", "median ms", "min ms", "max ms", "GB/s", "of peak")]
        for name, _ in runs:
            t = times[name]
            gbs = nbytes / (1e-3 * statistics.median(t)) / 1e9
            text.append("%-48s %9.3f %9.3f %9.3f %9.1f %9.4f" % (name, statistics.median(t), min(t), max(t), gbs, gbs * 1e9 / HBM_PEAK))
        text.append("")
        for m in u + s:
            m.destroy()
        mla.destroy()
    print("\n".join(text))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
