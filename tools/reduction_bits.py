#!/usr/bin/env python
"""The bits of the composite-grid reductions (vdn_diagnostics, vdn_profiles, vdn_pdf, vdn_pdf2) on the small grids of the test workers: one SHA-256 per case over
the raw bytes of every output array.  The three entries promise that a result's bits depend on the box lists and the fields alone; a change to the thread -> cell
map, a shuffle tree, the (w0 + w1) + (w2 + w3) step or the slot order of a final sum shows here as another hash.  The grids have extents that are no multiple of
64, planes smaller than a workgroup, several boxes per level and partly covered boxes; nscal = 2 and 3 run the kernels that carry four scalars, 11 those that
carry eleven.  Only the Python surface is used, so the same file runs against any build that has the four entries:

    python tools/reduction_bits.py [--out tests/golden/composite_reduction_bits.json]

tests/test_composite_bits_gpu.py holds the library to the recorded file."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WALLS2 = [[15, 15], [15, 15]]


def sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def figures(pkg):
    """yields (case, sha256) in a fixed order"""
    from tests import _diagnostics_worker as dw, _pdf_worker as pw, _profiles_worker as fw
    six = (fw.ONE_LEVEL["six-boxes"][0], [fw.ONE_LEVEL["six-boxes"][1]])
    one = (fw.ONE_LEVEL["one-box"][0], [fw.ONE_LEVEL["one-box"][1]])
    flat = (fw.FLAT[0], [fw.FLAT[1]])

    def each(H, calls):
        try:
            for name, fn in calls(H):
                yield name, sha(fn())
        finally:
            H.close()

    # vdn_diagnostics with the vorticity terms (the ghost cells of u are cut out of the same seeded array as the valid cells)
    for name, (n, boxes), kw in (("amr2", dw.CASES["amr2"], dict(nscal=3)), ("amr3", dw.CASES["amr3"], dict(nscal=3)), ("six-boxes-nscal11", six, dict(nscal=11)),
                                 ("dm2", flat, dict(nscal=2, dm=2, phys=WALLS2))):
        yield from each(dw.Hier(pkg, n, boxes, seed=7, **kw), lambda H: [("diag %s" % name, lambda: dw.all_bits(H.diagnostics(vort=True)))])
    # vdn_profiles
    for name, (n, boxes), axes, kw in (("amr3-nscal2", fw.AMR3, (0, 1, 2), dict(nscal=2)), ("six-boxes-nscal11", six, (0, 2), dict(nscal=11)),
                                       ("one-box", one, (1,), dict(nscal=2)), ("dm2", flat, (0, 1), dict(nscal=2, dm=2, phys=WALLS2))):
        yield from each(fw.hier(pkg, n, boxes, seed=7, **kw),
                        lambda H: [("profiles %s axis %d" % (name, a), lambda a=a: fw.all_bits(fw.profiles(H, a))) for a in axes])
    # vdn_pdf and vdn_pdf2 (make_vorticity fills the ghost cells of u that the vorticity axis reads)

    def pdf_calls(name, axes, pair):
        def calls(H):
            pw.vorticity(H)
            out = [("pdf %s %s[%d] %d bins" % (name, ax[0], ax[1], ax[4]), lambda ax=ax: pw.all_bits(pw.pdf(H, *ax))) for ax in axes]
            if pair:
                out.append(("pdf2 %s" % name, lambda: pw.all_bits2(pw.pdf2(H, *pair))))
            return out
        return calls
    dm2_axes = (("scalar", 1, 0.1, 0.9, 7), ("velocity", 1, -0.9, -0.1, 256), ("magvel", 0, 0.2, 1.2, 64), ("vorticity", 0, -9.0, 13.0, 64))
    dm2_pair = (("scalar", 0, -0.75, 0.8, 64), ("velocity", 1, -0.9, -0.1, 3))
    for name, (n, boxes), axes, pair, kw in (("amr3-nscal2", fw.AMR3, pw.RANK_AXES, pw.RANK_PAIR, dict(nscal=2)), ("six-boxes-nscal11", six, pw.RANK_AXES, None, dict(nscal=11)),
                                             ("dm2", flat, dm2_axes, dm2_pair, dict(nscal=2, dm=2, phys=WALLS2))):
        H = dw.Hier(pkg, n, boxes, seed=9, **kw)
        H.dx = [[2.0 ** -((3, 2, 4)[d] + l) for d in range(H.dm)] for l in range(H.nlev)]
        yield from each(H, pdf_calls(name, axes, pair))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the hashes as JSON")
    a = ap.parse_args()
    import varden_amd
    from varden_amd import advance, boxlib, capi  # noqa: F401
    out = {}
    for name, h in figures(varden_amd):
        print("%s  %s" % (h, name), flush=True)
        out[name] = h
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
