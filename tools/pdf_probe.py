#!/usr/bin/env python
"""What one call of the PDFs by value costs (vdn_pdf, vdn_pdf2, csrc/pdf.hip), wall-clock per call with a device synchronisation either side (every call ends in its
one read-back), on

  one      the 256^3 bubble in one box after three steps
  amr3     the three-level bubble of bench.py's amr3 config (a 256^3 base in one box, refined levels tagged rho > 1.01 / rho > 1.1) after one step

for
  density      the density PDF at 64 bins over [0.5, 10.5)
  vorticity    the vorticity PDF at 256 bins over [0, the state's largest |curl u|): the rough field, many distinct slots in a wave
  rho-w        the joint distribution of the density and the vertical velocity at 64 x 64

next to the route a user has without the entries:

  (h) host copy + numpy      to_numpy() of every box of every level, a composite mask from the box lists, numpy.histogram of the density weighted by the cell
                             volume.  This Python depends on the library only through to_numpy(), so a build without the entries runs the same code.

The bytes a call must read are (dm + nscal) * 8 B per composite cell for vdn_pdf (the vorticity's neighbours are re-reads) and 2 * 8 B for this vdn_pdf2; the table
gives them per second and as a fraction of the 8 TB/s HBM peak the README uses.  For the one-box grid the mean number of DISTINCT slots among the 64 cells of a wave
trip is counted on the host from the same fields (a wave's cells are 64 consecutive cells along x): the length of the kernel's inner loop.

    python tools/pdf_probe.py [--repeats 5] [--host-repeats 2] [--grids one,amr3] [--no-host] [--out profiles/pdf_probe.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def slots(q, lo, hi, nbins):
    """the slot rule of csrc/pdf_bin.h in float64 (-1: NaN, 0: below lo, nbins + 1: at or above hi)"""
    w = (hi - lo) / nbins
    with np.errstate(all="ignore"):
        m = np.minimum(np.floor((q - lo) / w), float(nbins - 1))
    return np.where(np.isnan(q), -1, np.where(q < lo, 0, np.where(q >= hi, nbins + 1, 1 + np.nan_to_num(m)))).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--grids", default="one,amr3")
    ap.add_argument("--no-host", action="store_true", help="leave (h) out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from varden_amd import advance as adv, boxlib as bl, capi, driver
    n, walls = 256, [[15, 15]] * 3
    prm = capi.default_params(cflfac=0.9)
    dm, ns = prm.dm, prm.nscal
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
        dxs = G.dx if hasattr(G.dx[0], "__len__") else [G.dx]
        D = G.diagnostics()
        vmax = float(np.nextafter(D["vort_max"], np.inf))
        wlo, whi = float(D["u_min"][2]), float(np.nextafter(D["u_max"][2], np.inf))
        axes = {"density": ("scalar", 0, 0.5, 10.5, 64), "vorticity": ("vorticity", 0, 0.0, vmax, 256)}
        pair = (("scalar", 0, 0.5, 10.5, 64), ("velocity", 2, wlo, whi, 64))

        def valid(mf, i):
            lo, hi = mf.get_box(i)
            f = mf.to_numpy(i)
            g = [(f.shape[d] - (hi[d] - lo[d] + 1)) // 2 for d in range(3)]
            return lo, hi, f[tuple(slice(g[d], f.shape[d] - g[d]) for d in range(3))]

        def host():
            """the volume per bin of the density axis from host copies: (volume over the bins, below, above)"""
            _, _, lo_, hi_, nb = axes["density"]
            vol = np.zeros(nb + 2)
            for l in range(NL):
                dv = float(np.prod(dxs[l]))
                for i in range(G.sold[l].nfabs()):
                    lo, hi, sv = valid(G.sold[l], i)
                    _, _, uv = valid(G.uold[l], i)                                  # (the conditional sums would need it; the copy is part of the route)
                    mask = np.ones(sv.shape[:3], dtype=bool)
                    if l < NL - 1:
                        for flo, fhi in boxes[l + 1]:
                            a0 = [max(flo[d] // 2, lo[d]) - lo[d] for d in range(3)]
                            a1 = [min(fhi[d] // 2, hi[d]) - lo[d] for d in range(3)]
                            if all(a0[d] <= a1[d] for d in range(3)):
                                mask[a0[0]:a1[0] + 1, a0[1]:a1[1] + 1, a0[2]:a1[2] + 1] = False
                    rho = sv[..., 0][mask]
                    h, _ = np.histogram(rho, bins=nb, range=(lo_, hi_), weights=np.full(rho.shape, dv))
                    vol[1:-1] += h
                    vol[0] += dv * int((rho < lo_).sum())
                    vol[-1] += dv * int((rho > hi_).sum())
            return vol

        runs = [(name, (lambda ax=ax: G.pdf(ax[0], ax[1], ax[2], ax[3], ax[4]))) for name, ax in axes.items()]
        runs.append(("rho-w", lambda: G.pdf2(pair[0][0], pair[0][1], pair[0][2], pair[0][3], pair[0][4], pair[1][0], pair[1][1], pair[1][2], pair[1][3], pair[1][4])))
        res = {name: fn() for name, fn in runs}                                           # warm-up (and the results)
        times = {name: [] for name, _ in runs}
        for r in range(a.repeats):
            for name, fn in runs[r % len(runs):] + runs[:r % len(runs)]:
                capi.check(capi.load().vdn_device_synchronize())
                t0 = time.perf_counter()
                fn()
                capi.check(capi.load().vdn_device_synchronize())
                times[name].append(1e3 * (time.perf_counter() - t0))
        cells = D["cells"]
        assert int(res["density"].cells.sum()) + res["density"].nan_cells == cells and int(res["rho-w"].cells.sum()) + res["rho-w"].nan_cells == cells
        assert np.array_equal(res["rho-w"].cells.sum(axis=2), res["density"].cells) and res["vorticity"].cells[:, 0].sum() == 0 and res["vorticity"].cells[:, -1].sum() == 0
        hname = "(h) to_numpy + mask + numpy.histogram, density"
        if not a.no_host:
            times[hname] = []
            for r in range(a.host_repeats):
                capi.check(capi.load().vdn_device_synchronize())
                t0 = time.perf_counter()
                hvol = host()
                times[hname].append(1e3 * (time.perf_counter() - t0))
            runs.append((hname, None))
            assert np.allclose(hvol[1:-1], res["density"]["volume"][1:-1], rtol=1e-9, atol=1e-15), (hvol, res["density"]["volume"])       # (numpy closes the last bin at hi)
        nbytes = {"density": (dm + ns) * 8 * cells, "vorticity": (dm + ns) * 8 * cells, "rho-w": 2 * 8 * cells, hname: (dm + ns) * 8 * cells}
        text += ["pdf_probe %s: %d level(s), boxes %s, %d composite cells after %d step(s); (dm + nscal) * 8 B * cells = %.1f MB; %d timed calls each after a warm-up (host "
                 "route: %d, no warm-up); library %s (%s)" % (grid, NL, [len(b) for b in boxes], cells, steps, (dm + ns) * 8 * cells / 1e6, a.repeats, a.host_repeats,
                                                              os.path.relpath(capi.LIB_PATH, ROOT), capi.load().vdn_build_flavour().decode()),
                 "vorticity axis [0, %.6g), w axis [%.6g, %.6g)" % (vmax, wlo, whi),
                 "%-48s %9s %9s %9s %9s %9s" % ("", "median ms", "min ms", "max ms", "GB/s", "of peak")]
        for name, _ in runs:
            t = times[name]
            gbs = nbytes[name] / (1e-3 * statistics.median(t)) / 1e9
            text.append("%-48s %9.3f %9.3f %9.3f %9.1f %9.4f" % (name, statistics.median(t), min(t), max(t), gbs, gbs * 1e9 / HBM_PEAK))
        if grid == "one":                                   # the inner loop's length: distinct slots among the 64 consecutive cells (along x) of a wave trip
            G.fill_state_ghosts()
            w = bl.MultiFab(G.mla, 0, 1, 0)
            adv.make_vorticity(w, 0, G.uold[0], dxs[0], G.bct)
            fields = {"density": valid(G.sold[0], 0)[2][..., 0], "vorticity": valid(w, 0)[2][..., 0]}
            w.destroy()
            for name, q in fields.items():
                _, _, lo_, hi_, nb = axes[name]
                sl = np.sort(slots(q.ravel(order="F"), lo_, hi_, nb).reshape(-1, 64), axis=1)
                distinct = 1 + (np.diff(sl, axis=1) != 0).sum(axis=1)
                text.append("distinct slots per wave trip, %-10s mean %.2f, median %d, max %d" % (name + ":", distinct.mean(), int(np.median(distinct)), distinct.max()))
        text.append("")
        G.close()
    print("\n".join(text))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
