"""python -m varden_amd <inputs file> [--steps N] [--outdir DIR] [--device D] [--files plane|copy] [--diag-int N] [--particles NX,NY,NZ] [--particle-int N] [--prof-int N] [--prof-axis A] [--pdf-int N --pdf-field F --pdf-range LO,HI [--pdf-comp C --pdf-nbins B]] [--iso-int N --iso-field F --iso-comp C --iso-value V]: the reference executable's command line (src/main.f90
reads the inputs file named by the first argument and calls varden()).  Plot and checkpoint files go under --outdir; a 2-D hierarchy writes the 2-D run's own
dm = 2 files (--files copy: those of the 3-D copy it runs as).  --diag-int N overrides the namelist's diag_int: a line of run diagnostics (advance.diagnostics) for the
starting state and after every N-th step, in <outdir>/<diag_file_name>.  --particles NX,NY,NZ and --particle-int N set the namelist's particle_lattice and
particle_int: tracer particles on an even lattice, moved by every step, written every N steps to <outdir>/<particle_base_name>NNNNN.  --prof-int N and --prof-axis A (numbered from 1; -1: the last
direction) override prof_int and prof_axis: the plane-averaged profiles (advance.profiles) of the starting state and after every N-th step, one file
<outdir>/<prof_base_name>NNNNN each.  --pdf-int N, --pdf-field F, --pdf-range LO,HI, --pdf-comp C (numbered from 1) and --pdf-nbins B override pdf_int, pdf_field, pdf_lo and
pdf_hi, pdf_comp and pdf_nbins: the distribution by value (advance.pdf) of the starting state and after every N-th step, one file <outdir>/<pdf_base_name>NNNNN each.  --iso-int N, --iso-field F, --iso-comp C (numbered from 1) and --iso-value V override
iso_int, iso_field, iso_comp and iso_value: the isosurface (advance.isosurface) of the starting state and after every N-th step, one binary PLY file
<outdir>/<iso_base_name>NNNNN.ply each and a line of its triangle count, area and volume above in <outdir>/<iso_base_name>.dat."""
import argparse
import os
import time

from . import advance as adv
from . import inputs


def main():
    ap = argparse.ArgumentParser(prog="python -m varden_amd")
    ap.add_argument("inputs_file")
    ap.add_argument("--steps", type=int, default=None, help="override max_step")
    ap.add_argument("--outdir", default=".")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--files", choices=["plane", "copy"], default="plane", help="files of a 2-D hierarchy: the 2-D run's (plane k = 0, dm = 2) or the 3-D copy's")
    ap.add_argument("--diag-int", type=int, default=None, help="override diag_int: run diagnostics every N steps into diag_file_name (0: none)")
    ap.add_argument("--particles", default=None, help="override particle_lattice: NX,NY,NZ tracer particles on an even lattice (0,0,0: none)")
    ap.add_argument("--particle-int", type=int, default=None, help="override particle_int: a particle file every N steps (0: none)")
    ap.add_argument("--prof-int", type=int, default=None, help="override prof_int: a file of plane-averaged profiles every N steps (0: none)")
    ap.add_argument("--prof-axis", type=int, default=None, help="override prof_axis: the direction of the profiles, numbered from 1 (-1: the last direction)")
    ap.add_argument("--pdf-int", type=int, default=None, help="override pdf_int: a file of the distribution by value (PDF and conditional sums) every N steps (0: none)")
    ap.add_argument("--pdf-field", default=None, choices=("scalar", "velocity", "magvel", "vorticity"), help="override pdf_field: the field whose values are binned")
    ap.add_argument("--pdf-range", default=None, help="override pdf_lo and pdf_hi: LO,HI, the range the bins divide")
    ap.add_argument("--pdf-comp", type=int, default=None, help="override pdf_comp: the component of a scalar or velocity field, numbered from 1")
    ap.add_argument("--pdf-nbins", type=int, default=None, help="override pdf_nbins: the number of bins (1 .. 256)")
    ap.add_argument("--iso-int", type=int, default=None, help="override iso_int: an isosurface file (binary PLY) and a line of its area and volume every N steps (0: none)")
    ap.add_argument("--iso-field", default=None, choices=("scalar", "velocity"), help="override iso_field: the field whose surface is extracted")
    ap.add_argument("--iso-comp", type=int, default=None, help="override iso_comp: the component of the field, numbered from 1")
    ap.add_argument("--iso-value", type=float, default=None, help="override iso_value: the value the surface takes")
    a = ap.parse_args()
    pdf_range = None if a.pdf_range is None else tuple(float(v) for v in a.pdf_range.split(","))
    if pdf_range is not None and len(pdf_range) != 2:
        ap.error("--pdf-range LO,HI")
    lattice = None if a.particles is None else tuple(int(v) for v in (a.particles.split(",") + ["0", "0"])[:3])
    os.makedirs(a.outdir, exist_ok=True)

    def report(G):                                           # the step line of src/varden.f90:347,  1000 format
        print("STEP = %d  TIME = %.15g  DT = %.15g   (mac %d, hg %d cycles)" % (G.istep, G.time, G.dt, adv.last_solver_stats("mac")[0],
                                                                               adv.last_solver_stats("hg")[0]), flush=True)

    t0 = time.time()
    nl, G = inputs.run(open(a.inputs_file).read(), a.steps, report, device=a.device, outdir=a.outdir, files=a.files, diag_int=a.diag_int, particles=lattice,
                        particle_int=a.particle_int, prof_int=a.prof_int, prof_axis=a.prof_axis, pdf_int=a.pdf_int,
                        pdf_field=a.pdf_field, pdf_comp=a.pdf_comp, pdf_range=pdf_range, pdf_nbins=a.pdf_nbins,
                        iso_int=a.iso_int, iso_field=a.iso_field, iso_comp=a.iso_comp, iso_value=a.iso_value)
    print("Total Run time (s) = %.3f" % (time.time() - t0))
    for f in G.files_written:
        print("wrote", f)
    G.close()


if __name__ == "__main__":
    main()
