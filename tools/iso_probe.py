#!/usr/bin/env python
"""What one call of the isosurface extraction costs (vdn_isosurface, csrc/iso.hip), wall-clock per call with a device synchronisation either side (every call ends in
its read-back), on

  one      the 256^3 bubble in one box after three steps
  amr3     the three-level bubble of bench.py's amr3 config (a 256^3 base in one box, refined levels tagged rho > 1.01 / rho > 1.1) after one step

for the density at the value halfway between the two fluids (5.5):

  count        the count call alone (max_tri = 0): pass 1, the slot sums, one read-back of the partials
  triangles    one call with a buffer of the known size: pass 1 as above, then pass 2 and the copy of the triangles to the host
  pass 2       the difference of the two medians: the second march, its stores and the copy home
  sized        advance.isosurface as a user calls it: the count call, then the call with triangles

and, through vdn_isosurface_timed, the device time of the launches of each pass alone (events around them, no read-back inside) for both forms of pass 2:

  form 0       every cell forms its nodes and counts again in pass 2
  form 1       pass 1 stores one byte per cell, pass 2 reads it and loads the neighbourhood of cut cells alone

next to the least any host route pays before it extracts anything:

  (h) host copy    to_numpy() of the density's multifab, every box of every level

Pass 1 reads the 3 x 3 x 3 neighbourhood of every composite cell (27 loads of 8 B, neighbours mostly in cache: 8 B per cell of new data); pass 2 reads the same and
writes 72 B per triangle.  The table gives both figures; it claims no fraction of any peak.

    python tools/iso_probe.py [--repeats 5] [--grids one,amr3] [--out profiles/iso_probe.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VALUE = 5.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grids", default="one,amr3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from varden_amd import advance as adv, capi, driver
    from varden_amd.boxlib import handle_array
    lib = capi.load()
    n, walls = 256, [[15, 15]] * 3
    prm = capi.default_params(cflfac=0.9)
    text = []
    for grid in a.grids.split(","):
        if grid == "one":
            G = driver.Varden((n,) * 3, walls, prm, prob_type=1, grav=-9.8, init_shrink=0.1, init_iter=1, swap_state=True)
            boxes, steps = [G.boxes], 3
        else:
            levels = driver.VardenAMR.tagged_grids(n, walls, prm, max_levs=3, max_grid_size=256)
            G = driver.VardenAMR(n, levels[0], walls, params=prm, finer_levels=levels[1:], init_shrink=0.1, init_iter=1, do_initial_projection=1, max_grid_size=256,
                                 swap_state=True)
            boxes, steps = G.boxes, 1
        for _ in range(steps):
            G.step()
        NL = len(boxes)
        G.fill_state_ghosts()
        first = G.isosurface("scalar", 0, VALUE)                    # warm-up (and the result)
        ntri = first.ntri
        tri, lev, out = np.zeros((max(ntri, 1), 3, 3)), np.zeros(max(ntri, 1), dtype=np.uint8), capi.Iso()
        args = (NL, G.mla.h, handle_array(G.sold), 0, G.dm, adv._dx3(G.dx), G.bct.h, VALUE)

        def count():
            capi.check(lib.vdn_isosurface(*args, 0, None, None, C.byref(out)))

        def triangles():
            capi.check(lib.vdn_isosurface(*args, ntri, tri.ctypes.data_as(C.POINTER(C.c_double)), lev.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(out)))

        def sized():
            adv.isosurface(G.mla, G.sold, 0, G.dm, G.dx, G.bct, VALUE)

        def host():
            return [G.sold[l].to_numpy(i) for l in range(NL) for i in range(G.sold[l].nfabs())]

        def timed(form):
            ms = (C.c_double * 2)()
            capi.check(lib.vdn_isosurface_timed(*args, ntri, tri.ctypes.data_as(C.POINTER(C.c_double)), lev.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(out), form, ms))
            return ms[0], ms[1]

        runs = [("count (pass 1, sums, read-back)", count), ("triangles (pass 1, pass 2, copy home)", triangles), ("sized (count call, then triangles)", sized),
                ("(h) host copy of the density's multifab", host)]
        for _, fn in runs:
            fn()
        assert out.written == ntri and np.array_equal(tri[:ntri], first.tri)
        times = {name: [] for name, _ in runs}
        for r in range(a.repeats):
            for name, fn in runs[r % len(runs):] + runs[:r % len(runs)]:
                capi.check(lib.vdn_device_synchronize())
                t0 = time.perf_counter()
                fn()
                capi.check(lib.vdn_device_synchronize())
                times[name].append(1e3 * (time.perf_counter() - t0))
        forms = {0: [], 1: []}
        for form in (0, 1):
            timed(form)
            assert out.written == ntri and np.array_equal(tri[:ntri], first.tri)
        for r in range(a.repeats):
            for form in ((0, 1) if r % 2 == 0 else (1, 0)):
                capi.check(lib.vdn_device_synchronize())
                t0 = time.perf_counter()
                p1, p2 = timed(form)
                capi.check(lib.vdn_device_synchronize())
                forms[form].append((p1, p2, 1e3 * (time.perf_counter() - t0)))
        cells = G.diagnostics(vort=False)["cells"]
        text += ["iso_probe %s: %d level(s), boxes %s, %d composite cells after %d step(s); density = %g: %d triangles in %d cut cells (per level %s), area %.6g, volume above "
                 "%.6g; %d timed calls each after a warm-up; library %s (%s)" % (grid, NL, [len(b) for b in boxes], cells, steps, VALUE, ntri, first.cut_cells, first.ntri_lev,
                                                                                   first.area, first.volume_above, a.repeats, os.path.relpath(capi.LIB_PATH, ROOT),
                                                                                   lib.vdn_build_flavour().decode()),
                 "new data read by a pass: 8 B * cells = %.1f MB (27 loads per cell: %.1f MB through the caches); written by pass 2 and copied home: 72 B * triangles = %.2f MB" % (
                     8 * cells / 1e6, 27 * 8 * cells / 1e6, 72 * ntri / 1e6),
                 "%-48s %9s %9s %9s" % ("", "median ms", "min ms", "max ms")]
        for name, _ in runs:
            t = times[name]
            text.append("%-48s %9.3f %9.3f %9.3f" % (name, statistics.median(t), min(t), max(t)))
        text.append("%-48s %9.3f" % ("pass 2 and the copy home (difference of medians)", statistics.median(times[runs[1][0]]) - statistics.median(times[runs[0][0]])))
        text.append("%-48s %9s %9s %9s" % ("device time of the launches alone, median ms", "pass 1", "pass 2", "call"))
        for form, name in ((0, "form 0: pass 2 recomputes every cell"), (1, "form 1: pass 1 stores counts, pass 2 reads them")):
            text.append("%-48s %9.3f %9.3f %9.3f" % (name, statistics.median(v[0] for v in forms[form]), statistics.median(v[1] for v in forms[form]),
                                                      statistics.median(v[2] for v in forms[form])))
        text.append("")
        G.close()
    print("\n".join(text))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
