#!/usr/bin/env python
"""What moving tracer particles costs (vdn_particles_advance, csrc/particles.hip) next to the step it rides on, wall-clock, on

  one      the 256^3 bubble in one box (driver.Varden), after three steps
  amr3     the three-level hierarchy of tests/golden/amr_grids_256_l3.json (a 256^3 base in one box, 263 and 997 boxes above it; driver.VardenAMR on
           fixed grids), after two steps

with 2^20 and 2^24 particles on an even lattice over the domain:

  (a) step(), no particles          the step of the same run in the same session
  (b) particles.advance             one move between uold and unew (three launches; every call is followed by a device synchronisation here)
  (c) host copy                     to_numpy() of uold and unew of every level: what a host-side tracer would need before it can interpolate anything
  (d) host copy + numpy             ... and the trilinear interpolation of both fields at the particles in numpy (one box only, 2^20 particles)

    python tools/particles_probe.py [--repeats 5] [--grids one,amr3] [--counts 20,24] [--out profiles/particles_probe.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def numpy_trilinear(f, ng, dx, x):
    """cell-centred trilinear interpolation of one fab (valid box from cell 0) at x (n, 3), away from face-value weights: the arithmetic a host-side tracer does"""
    out = np.zeros((x.shape[0], f.shape[3]))
    xi = x / dx - 0.5
    i = np.floor(xi).astype(np.int64)
    w = xi - i
    i += ng
    for c in range(f.shape[3]):
        A = f[..., c]
        v = []
        for dk in (0, 1):
            for dj in (0, 1):
                a, b = A[i[:, 0], i[:, 1] + dj, i[:, 2] + dk], A[i[:, 0] + 1, i[:, 1] + dj, i[:, 2] + dk]
                v.append(a + w[:, 0] * (b - a))
        r0, r1 = v[0] + w[:, 1] * (v[1] - v[0]), v[2] + w[:, 1] * (v[3] - v[2])
        out[:, c] = r0 + w[:, 2] * (r1 - r0)
    return out


def timed(fn, repeats, sync):
    fn()                                                       # warm-up
    t = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        t.append(1e3 * (time.perf_counter() - t0))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grids", default="one,amr3")
    ap.add_argument("--counts", default="20,24", help="log2 of the particle counts")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from varden_amd import advance as adv, boxlib as bl, capi, driver
    walls = [[bl.NO_SLIP_WALL] * 2] * 3
    n = 256
    text = []

    def sync():
        capi.check(capi.load().vdn_device_synchronize())

    for grid in a.grids.split(","):
        if grid == "one":
            S = driver.Varden(n, walls, capi.default_params(), init_shrink=0.1, init_iter=1)
            nsteps = 3
        else:
            boxes = [[(tuple(b[0]), tuple(b[1])) for b in lev] for lev in json.load(open(os.path.join(ROOT, "tests", "golden", "amr_grids_256_l3.json")))]
            S = driver.VardenAMR(n, boxes[0], walls, capi.default_params(), finer_levels=boxes[1:], init_shrink=0.1)
            nsteps = 2
        for _ in range(nsteps):
            S.step()
        nlev = len(S.uold)
        rows = [("(a) step(), no particles", timed(S.step, max(2, a.repeats // 2), sync))]
        # the two fields of a move, as step() prepares them
        S.fill_state_ghosts()
        if nlev == 1:
            S.unew[0].fill_boundary()
            S.unew[0].physbc(0, 0, 3, S.bct)
        else:
            adv.ml_restrict_and_fill(S.unew, 0, 0, 3, S.bct)
        dt = S.dt
        for lg in [int(v) for v in a.counts.split(",")]:
            per = [1 << ((lg + 2 - d) // 3) for d in range(3)]
            x0 = adv.particle_lattice(per, (1.0, 1.0, 1.0))
            P = adv.Particles(x0)
            rows.append(("(b) particles.advance, 2^%d particles" % lg, timed(lambda: P.advance(S.mla, S.uold, S.unew, S.dx, S.bct, dt), a.repeats, sync)))
            assert P.active == x0.shape[0] and np.isfinite(P.positions()).all()
            P.destroy()

        def copy():
            return [[m.to_numpy(i) for i in range(m.nfabs())] for m in S.uold + S.unew]
        rows.append(("(c) host copy of uold and unew, every level", timed(copy, max(2, a.repeats // 2), sync)))
        if nlev == 1:
            x1 = adv.particle_lattice((128, 128, 64), (1.0, 1.0, 1.0))

            def host():
                f = copy()
                return [numpy_trilinear(f[0][0], 3, S.dx[0][0], x1), numpy_trilinear(f[1][0], 3, S.dx[0][0], x1)]
            rows.append(("(d) host copy + numpy at 2^20 particles", timed(host, 2, sync)))
        text += ["particles_probe %s: %d level(s), boxes %s, after %d steps; library %s" % (grid, nlev, [len(b) for b in (S.boxes if nlev > 1 else [S.boxes])], nsteps,
                                                                                            capi.load().vdn_build_flavour().decode()),
                 "%-48s %9s %9s %9s %5s" % ("", "median ms", "min ms", "max ms", "calls")]
        for name, t in rows:
            text.append("%-48s %9.3f %9.3f %9.3f %5d" % (name, statistics.median(t), min(t), max(t), len(t)))
        text.append("")
        S.close()
    print("\n".join(text))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
