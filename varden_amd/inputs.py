"""Reads the reference's run-time inputs (a Fortran namelist &PROBIN, e.g. exec/test/inputs_bubble_3d) and drives the path the way
src/varden.f90 does: parameters (src/_parameters), grids (fixed single level, or tag_boxes + make_new_grids), start-up sequence,
time loop with estdt / regrid / advance_timestep, plot files every plot_int steps, checkpoints every chk_int steps, restart = n
continues from chk<n> (src/varden.f90:94-97, 207-229, 349-361)."""
import os
import re

from . import advance as adv
from . import boxlib as bl
from . import plotfile
from .capi import default_params
from .driver import ISO_FIELDS, Varden, VardenAMR

# src/_parameters: the defaults that matter to the path
DEFAULTS = dict(dim_in=2, nscal=2, prob_type=1, grav=0.0, boussinesq=0, max_step=1, stop_time=-1.0, max_levs=1, max_grid_size=256,
                regrid_int=-1, amr_buf_width=-1, n_cellx=32, n_celly=32, n_cellz=32, prob_hi_x=1.0, prob_hi_y=1.0, prob_hi_z=1.0,
                init_iter=4, do_initial_projection=1, init_shrink=1.0, cflfac=0.8, max_dt_growth=1.1, visc_coef=0.0, diff_coef=0.0,
                diffusion_type=1, slope_order=4, use_minion=0, stencil_order=2, verbose=0, mg_verbose=0,
                mg_bottom_solver=-1, hg_bottom_solver=-1, max_mg_bottom_nlevels=1000,
                bcx_lo=14, bcx_hi=14, bcy_lo=14, bcy_hi=14, bcz_lo=14, bcz_hi=14,
                fixed_dt=-1.0, plot_int=0, chk_int=0, restart=-1, plot_base_name="plt", check_base_name="chk", grids_file_name="", job_name="", fixed_grids="",
                diag_int=0, diag_file_name="varden_diag.out", prof_int=0, prof_axis=-1, prof_base_name="prof",          # (the diag_, prof_, pdf_ and particle keys are the project's own, like tag_field)
                pdf_int=0, pdf_field="scalar", pdf_comp=1, pdf_lo=0.0, pdf_hi=0.0, pdf_nbins=64, pdf_base_name="pdf",
                iso_int=0, iso_field="scalar", iso_comp=1, iso_value=0.0, iso_base_name="iso",
                particle_lattice=(0, 0, 0), particle_int=0, particle_base_name="part")


def parse_namelist(text):
    """key = value pairs of the first namelist group; Fortran literals (1.d0, .true., 'str'); indexed keys like u_bc(1,1) or tag_field(1) kept verbatim"""
    out = {}
    body = re.sub(r"!.*", "", text)
    for m in re.finditer(r"([A-Za-z_][\w]*(?:\(\s*\d+\s*(?:,\s*\d+\s*)?\))?)\s*=\s*('[^'\n]*'|\"[^\"\n]*\"|[^\n,/]+)", body):
        key, val = m.group(1).replace(" ", ""), m.group(2).strip()
        low = val.lower()
        if low in (".true.", "t", ".t."):
            out[key] = 1
        elif low in (".false.", "f", ".f."):
            out[key] = 0
        elif val[:1] in "'\"":
            out[key] = val.strip("'\"")
        else:
            num = re.sub(r"[dD]", "e", val)
            try:
                out[key] = int(num)
            except ValueError:
                out[key] = float(num)
    return out


def namelist_tag_criteria(nl):
    """the project's own keys (absent from the reference's _parameters): tag_field(n) = 'scalar' | 'scalar_grad' | 'vorticity' | 'magvel', tag_comp(n) (1-based,
    default 1), tag_gt(n,lev), tag_lt(n,lev) for n = 1 .. 8 -- criterion n tags the cells of level lev where tag_gt < value < tag_lt (a side without a key is open; a
    level without a key repeats the last level given).  Returns the list VardenAMR takes as tag_criteria, or None when no such key is present."""
    from .capi import MAXLEV, TAG_FIELDS, TAG_MAX_CRITERIA
    found = {}
    for key, v in nl.items():
        m = re.fullmatch(r"tag_(field|comp)\((\d+)\)|tag_(gt|lt)\((\d+),(\d+)\)", key)
        if not m:
            if key.startswith("tag_"):
                raise ValueError("inputs: %s: the tagging keys are tag_field(n), tag_comp(n), tag_gt(n,lev), tag_lt(n,lev)" % key)
            continue
        n = int(m.group(2) or m.group(4))
        if not 1 <= n <= TAG_MAX_CRITERIA:
            raise ValueError("inputs: %s: criteria are numbered 1 .. %d" % (key, TAG_MAX_CRITERIA))
        c = found.setdefault(n, dict(gt={}, lt={}))
        if m.group(1):
            c[m.group(1)] = v
        else:
            if not 1 <= int(m.group(5)) <= MAXLEV:
                raise ValueError("inputs: %s: levels are numbered 1 .. %d" % (key, MAXLEV))
            c[m.group(3)][int(m.group(5))] = float(v)
    if not found:
        return None
    out = []
    for n in sorted(found):
        c = found[n]
        if "field" not in c:
            raise ValueError("inputs: criterion %d has thresholds but no tag_field(%d)" % (n, n))
        if c["field"] not in TAG_FIELDS:
            raise ValueError("inputs: tag_field(%d) = %r: one of %s" % (n, c["field"], ", ".join(TAG_FIELDS)))
        crit = dict(field=str(c["field"]), comp=int(c.get("comp", 1)))
        for side in ("gt", "lt"):
            if c[side]:
                vals, last = [], None
                for lev in range(1, max(c[side]) + 1):
                    if lev in c[side]:
                        last = c[side][lev]
                    elif last is None:
                        raise ValueError("inputs: tag_%s(%d,%d) is missing (levels are given from 1 up)" % (side, n, lev))
                    vals.append(last)
                crit[side] = vals
        out.append(crit)
    return out


def namelist_particle_lattice(nl, text=""):
    """the project's own key particle_lattice(1:3) = nx ny nz: tracer particles at the centres of an even lattice over the domain (all zero: none).  Taken from the
    indexed keys particle_lattice(1) .. (3) or from one line `particle_lattice = nx, ny, nz`"""
    out = [int(v) for v in DEFAULTS["particle_lattice"]]
    m = re.search(r"^[^!\n]*\bparticle_lattice\s*=\s*(\d+)[\s,]+(\d+)(?:[\s,]+(\d+))?", text, flags=re.M)
    if m:
        out = [int(m.group(1)), int(m.group(2)), int(m.group(3) or 0)]
    for d in range(3):
        if "particle_lattice(%d)" % (d + 1) in nl:
            out[d] = int(nl["particle_lattice(%d)" % (d + 1)])
    if any(v < 0 for v in out):
        raise ValueError("inputs: particle_lattice = %r: counts are >= 0" % (out,))
    return tuple(out)


def domain_extent(G):
    """the physical extent of the domain a driver object runs on, per direction of its dm"""
    cells = G.n if hasattr(G, "n") else G.ncs
    return [cells[d] * G.dx[0][d] for d in range(G.dm)]


PARTICLE_FILE = "Particles"          # inside a checkpoint directory


def particle_columns(G):
    """what a particle file carries beside positions and states: the velocity and the nscal scalars at the particles (ghost cells filled first, as the next
    step's top fills them)"""
    G.fill_state_ghosts()
    u = G.particles.sample(G.mla, G.uold, G.dx, G.bct, comp=0, nc=G.dm, bccomp=0)
    sc = G.particles.sample(G.mla, G.sold, G.dx, G.bct, comp=0, nc=G.nscal, bccomp=G.dm)
    cols = {"vel%d" % (d + 1): u[:, d] for d in range(G.dm)}
    cols.update({"s%d" % (c + 1): sc[:, c] for c in range(G.nscal)})
    return cols


def namelist_params(nl, dm=None):
    """vdn_params for a namelist dictionary (DEFAULTS updated with parse_namelist's keys); dm: run it in this dimension instead of dim_in"""
    prm = default_params(dm=int(nl["dim_in"]) if dm is None else dm, nscal=int(nl["nscal"]), slope_order=int(nl["slope_order"]), use_minion=int(nl["use_minion"]),
                         boussinesq=int(nl["boussinesq"]), stencil_order=int(nl["stencil_order"]), diffusion_type=int(nl["diffusion_type"]),
                         verbose=int(nl["verbose"]), prob_type=int(nl["prob_type"]), visc_coef=float(nl["visc_coef"]),
                         diff_coef=float(nl["diff_coef"]), cflfac=float(nl["cflfac"]), max_dt_growth=float(nl["max_dt_growth"]),
                         mg_bottom_solver=int(nl["mg_bottom_solver"]), hg_bottom_solver=int(nl["hg_bottom_solver"]),       # src/_parameters:55-57
                         max_mg_bottom_nlevels=int(nl["max_mg_bottom_nlevels"]))
    return prm


def build(text, device=0, max_grid_size_cap=None, outdir=".", extrude_nz=16, extrude_zbc=None, files="plane", nl=None):
    """the driver object for an inputs text: Varden (one level) or VardenAMR (max_levs > 1, grids from the tagged initial data);
    restart >= 0: grids and state from the checkpoint <outdir>/<check_base_name><restart:05d> (src/varden.f90:94-97).
    files: what a 2-D hierarchy (run as its z-uniform 3-D copy) writes and restarts from -- "plane": the 2-D run's own dm = 2 files, "copy": the 3-D copy's.
    nl: the namelist of `text` over DEFAULTS where the caller has parsed it already (run has)"""
    assert files in ("plane", "copy"), files
    if nl is None:
        nl = dict(DEFAULTS)
        nl.update(parse_namelist(text))
    dm = int(nl["dim_in"])
    prm = namelist_params(nl)
    for name in ("u_bc", "v_bc", "w_bc", "rho_bc", "trac_bc"):           # inflow data, probin.template:21-23: name(direction, side)
        for key, v in nl.items():
            m = re.fullmatch(name + r"\((\d),(\d)\)", key)
            if m:
                getattr(prm, name)[int(m.group(1)) - 1][int(m.group(2)) - 1] = float(v)
    phys = [[int(nl["bc%s_lo" % a]), int(nl["bc%s_hi" % a])] for a in "xyz"[:dm]]
    n = tuple(int(nl["n_cell" + a]) for a in "xyz"[:dm])
    prob_hi = tuple(float(nl["prob_hi_" + a]) for a in "xyz"[:dm]) + (1.0,) * (3 - dm)
    mgs = int(nl["max_grid_size"]) if max_grid_size_cap is None else min(int(nl["max_grid_size"]), max_grid_size_cap)
    abw = max(int(nl["amr_buf_width"]), int(nl["regrid_int"]), 1)      # probin.template:147-154 (amr_buf_width >= regrid_int)
    common = dict(prob_type=int(nl["prob_type"]), grav=float(nl["grav"]), init_shrink=float(nl["init_shrink"]),
                  init_iter=int(nl["init_iter"]), do_initial_projection=int(nl["do_initial_projection"]), device=device,
                  fixed_dt=float(nl["fixed_dt"]), stop_time=float(nl["stop_time"]))
    decomp = tuple(max(1, -(-n[d] // mgs)) for d in range(dm)) + (1,) * (3 - dm)
    tagc = namelist_tag_criteria(nl)
    amr = dict(tag_criteria=tagc) if tagc is not None else {}       # (without the keys: the calls as they were)

    def copy_of_2d(boxes2d, **kw):
        """a 2-D hierarchy on the box lists of a dm = 2 checkpoint or grids file, as the z-uniform copy: plotfile.extrude_boxes, extrude_nz << n cells along z on level n"""
        if prob_hi[0] != 1.0 or abs(prob_hi[1] / n[1] - prob_hi[0] / n[0]) > 1e-15:
            raise NotImplementedError("2-D hierarchies: prob_hi_x = 1 and square cells")
        b3 = [plotfile.extrude_boxes(b, int(extrude_nz) << lev, mgs) for lev, b in enumerate(boxes2d)]
        G = VardenAMR(n, b3[1], phys, params=params_of_copy(), finer_levels=b3[2:], base_boxes=b3[0], regrid_int=int(nl["regrid_int"]), amr_buf_width=abw,
                      max_levs=max(int(nl["max_levs"]), len(b3)), max_grid_size=mgs, extrude2d=int(extrude_nz), extrude_zbc=extrude_zbc, **common, **amr, **kw)
        G.files_copy = files == "copy"
        return G

    def params_of_copy():
        prm3 = namelist_params(nl, dm=3)
        for name in ("u_bc", "v_bc", "rho_bc", "trac_bc"):
            for d in range(2):
                for sd in range(2):
                    getattr(prm3, name)[d][sd] = getattr(prm, name)[d][sd]
        return prm3
    if int(nl["restart"]) >= 0:
        chk = plotfile.read_checkfile(os.path.join(outdir, "%s%05d" % (nl["check_base_name"], int(nl["restart"]))))
        rs = dict(restart=chk, restart_step=int(nl["restart"]))
        if chk["nlevs"] == 1:
            return nl, Varden(n, phys, prm, prob_hi=prob_hi, decomp=decomp, **common, **rs)
        if dm == 2:
            if chk["dm"] != 2:
                raise NotImplementedError("restart of a 2-D hierarchy from %s: that checkpoint is a 3-D copy's (dm = %d, written with files=\"copy\"); only dm = 2 "
                                          "checkpoints are read back" % (chk["name"], chk["dm"]))
            return nl, copy_of_2d(chk["boxes"], **rs)
        return nl, VardenAMR(n[0], chk["boxes"][1], phys, params=prm, finer_levels=chk["boxes"][2:], base_boxes=chk["boxes"][0],
                             regrid_int=int(nl["regrid_int"]), amr_buf_width=abw, max_levs=int(nl["max_levs"]), max_grid_size=mgs, **common, **amr, **rs)
    if nl["fixed_grids"]:                                   # initialize_with_fixed_grids, src/initialize.f90:93-150
        if dm == 2:                                         # (a grids file of write_grids: the footprints, dm = 2)
            domains, boxes = plotfile.read_grids(os.path.join(outdir, str(nl["fixed_grids"])))
            assert domains[0] == ((0, 0, 0), (n[0] - 1, n[1] - 1, 0)), "fixed_grids: level-0 domain differs from n_cell"
            if len(boxes) == 1:
                raise NotImplementedError("fixed_grids with one level: use max_grid_size")
            return nl, copy_of_2d(boxes)
        if dm != 3 or len(set(n)) != 1 or any(p != 1.0 for p in prob_hi):
            raise NotImplementedError("hierarchies: 3-D, cubic unit domain in this round")
        domains, boxes = plotfile.read_grids(os.path.join(outdir, str(nl["fixed_grids"])))
        assert domains[0] == ((0, 0, 0), tuple(x - 1 for x in n)), "fixed_grids: level-0 domain differs from n_cell"
        if len(boxes) == 1:
            raise NotImplementedError("fixed_grids with one level: use max_grid_size")
        return nl, VardenAMR(n[0], boxes[1], phys, params=prm, finer_levels=boxes[2:], base_boxes=boxes[0], regrid_int=int(nl["regrid_int"]), amr_buf_width=abw,
                             max_levs=max(int(nl["max_levs"]), len(boxes)), max_grid_size=mgs, **common, **amr)
    if int(nl["max_levs"]) <= 1:
        return nl, Varden(n, phys, prm, prob_hi=prob_hi, decomp=decomp, **common)
    if dm == 2:
        # the 2-D inputs of exec/test (all four adaptive): the hierarchy runs as the z-uniform, z-periodic 3-D copy of the problem (driver.VardenAMR: extrude2d) --
        # plane k = 0 of every field is the 2-D answer and what the plot files and checkpoints hold (plotfile.py; files="copy": the 3-D copy's own files)
        if prob_hi[0] != 1.0 or abs(prob_hi[1] / n[1] - prob_hi[0] / n[0]) > 1e-15:
            raise NotImplementedError("2-D hierarchies: prob_hi_x = 1 and square cells")
        nz = int(extrude_nz)                                  # cells of level 0 along the periodic z of the copy (a multiple of the blocking factor)
        prm3 = params_of_copy()
        base = None
        if any(dc > 1 for dc in decomp[:2]) or nz > mgs:
            bs = [n[0] // decomp[0], n[1] // decomp[1], min(nz, mgs)]
            base = [((kx * bs[0], ky * bs[1], kz * bs[2]), ((kx + 1) * bs[0] - 1, (ky + 1) * bs[1] - 1, (kz + 1) * bs[2] - 1))
                    for kz in range(nz // bs[2]) for ky in range(decomp[1]) for kx in range(decomp[0])]
        levels = VardenAMR.tagged_grids(n, phys, prm3, prob_type=int(nl["prob_type"]), max_levs=int(nl["max_levs"]), buf_wid=abw, max_grid_size=mgs, device=device,
                                        base_boxes=base, extrude2d=nz, **amr)
        if not levels:
            return nl, Varden(n, phys, prm, prob_hi=prob_hi, decomp=decomp, **common)
        G = VardenAMR(n, levels[0], phys, params=prm3, finer_levels=levels[1:], regrid_int=int(nl["regrid_int"]), amr_buf_width=abw,
                      max_levs=int(nl["max_levs"]), max_grid_size=mgs, base_boxes=base, extrude2d=nz, extrude_zbc=extrude_zbc, **common, **amr)
        G.files_copy = files == "copy"
        return nl, G
    if len(set(n)) != 1 or any(p != 1.0 for p in prob_hi):
        raise NotImplementedError("adaptive hierarchies: cubic unit domain in this round")
    # level 0 is cut by max_grid_size like every other level (boxarray_maxsize, src/initialize.f90:204-206)
    base = None
    if any(dc > 1 for dc in decomp):
        bs = [n[d] // decomp[d] for d in range(3)]
        base = [((kx * bs[0], ky * bs[1], kz * bs[2]), ((kx + 1) * bs[0] - 1, (ky + 1) * bs[1] - 1, (kz + 1) * bs[2] - 1))
                for kz in range(decomp[2]) for ky in range(decomp[1]) for kx in range(decomp[0])]
    levels = VardenAMR.tagged_grids(n[0], phys, prm, prob_type=int(nl["prob_type"]), max_levs=int(nl["max_levs"]),
                                    buf_wid=abw, max_grid_size=mgs, device=device, base_boxes=base, **amr)
    if not levels:
        return nl, Varden(n, phys, prm, prob_hi=prob_hi, decomp=decomp, **common)
    return nl, VardenAMR(n[0], levels[0], phys, params=prm, finer_levels=levels[1:], regrid_int=int(nl["regrid_int"]), amr_buf_width=abw,
                         max_levs=int(nl["max_levs"]), max_grid_size=mgs, base_boxes=base, **common, **amr)


def diag_header(nscal, dm):
    """the header line of a diagnostics file"""
    return "#" + "step".rjust(7) + "".join(c.rjust(27) for c in ["time", "dt"]) + "".join(c.rjust(16 if c in ("cells", "nonfinite") else 27) for c in adv.diag_columns(nscal, dm)) + "\n"


def diag_line(istep, time, dt, d):
    """one data line of a diagnostics file: step (i8), time, dt, cells and nonfinite (i16), then volume, the integrals and the extrema (es27.17e3)"""
    v = adv.diag_values(d)
    return "%8d" % istep + plotfile._es(time) + plotfile._es(dt) + "%16d%16d" % (v[0], v[1]) + "".join(plotfile._es(x) for x in v[2:]) + "\n"


def profile_text(P, istep, time):
    """a profile file (prof_int > 0): the format tag, dm, the axis (numbered from 1, as the reference numbers directions), nbins, step and time on a header line each,
    the column names, then one line per bin: the bin centre (es27.17e3), the cell count (i16), every row of advance.profile_columns (es27.17e3).  varden_main writes the
    same, character for character."""
    cols = adv.profile_columns(P.nscal, P.dm)
    head = "# VDN_PROFILES 1\n# dm %d\n# axis %d\n# nbins %d\n# step %d\n# time%s\n" % (P.dm, P.axis + 1, len(P.x), istep, plotfile._es(time))
    head += "#" + "x".rjust(26) + "cells".rjust(16) + "".join(c.rjust(27) for c in cols) + "\n"
    body = ["".join([plotfile._es(P.x[m]), "%16d" % P.cells[m]] + [plotfile._es(v) for v in P.rows[:, m]]) + "\n" for m in range(len(P.x))]
    return head + "".join(body)


def pdf_text(P, istep, time):
    """a pdf file (pdf_int > 0): the format tag, dm, the field's name, comp (numbered from 1), nbins, lo, hi, step, time and nan_cells on a header line each, the column
    names, then one line per slot -- "below", the bins, "above": the slot centre lo + (m + 0.5) w for m = -1 .. nbins (es27.17e3), the cells of all levels (i16), every
    row of advance.pdf_columns (es27.17e3): the layout of a profile file (profile_text)."""
    cols = adv.pdf_columns(P.nscal, P.dm)
    name = P.field if isinstance(P.field, str) else {v: k for k, v in adv.PDF_FIELDS.items()}[int(P.field)]
    head = "# VDN_PDF 1\n# dm %d\n# field %s\n# comp %d\n# nbins %d\n# lo%s\n# hi%s\n# step %d\n# time%s\n# nan_cells %d\n" % (
        P.dm, name, P.comp + 1, P.nbins, plotfile._es(P.lo), plotfile._es(P.hi), istep, plotfile._es(time), P.nan_cells)
    head += "#" + "centre".rjust(26) + "cells".rjust(16) + "".join(c.rjust(27) for c in cols) + "\n"
    total = P.cells.sum(axis=0)
    body = ["".join([plotfile._es(P.centres[m]), "%16d" % total[m]] + [plotfile._es(v) for v in P.rows[:, m]]) + "\n" for m in range(P.nbins + 2)]
    return head + "".join(body)


def pdf_keys(nl, pdf_int=None, pdf_field=None, pdf_comp=None, pdf_range=None, pdf_nbins=None):
    """the pdf keys of a namelist with the arguments over them: (pdf_int, field name, comp numbered from 1, lo, hi, nbins).  With pdf_int > 0 a range with lo < hi and a
    known field are required"""
    k = int(nl["pdf_int"]) if pdf_int is None else int(pdf_int)
    field = str(nl["pdf_field"] if pdf_field is None else pdf_field).strip()
    comp = int(nl["pdf_comp"]) if pdf_comp is None else int(pdf_comp)
    lo, hi = (float(nl["pdf_lo"]), float(nl["pdf_hi"])) if pdf_range is None else (float(pdf_range[0]), float(pdf_range[1]))
    nbins = int(nl["pdf_nbins"]) if pdf_nbins is None else int(pdf_nbins)
    if k > 0:
        if not lo < hi:
            raise ValueError("inputs: pdf_int > 0 needs a range: pdf_lo = %r < pdf_hi = %r" % (lo, hi))
        if field not in adv.PDF_FIELDS:
            raise ValueError("inputs: pdf_field = %r: one of %s" % (field, ", ".join(sorted(adv.PDF_FIELDS))))
    return k, field, comp, lo, hi, nbins


def iso_keys(nl, iso_int=None, iso_field=None, iso_comp=None, iso_value=None):
    """the iso keys of a namelist with the arguments over them: (iso_int, field name, comp numbered from 1, value).  With iso_int > 0 a known field, a 3-D problem
    and a finite value are required"""
    k = int(nl["iso_int"]) if iso_int is None else int(iso_int)
    field = str(nl["iso_field"] if iso_field is None else iso_field).strip()
    comp = int(nl["iso_comp"]) if iso_comp is None else int(iso_comp)
    value = float(nl["iso_value"]) if iso_value is None else float(iso_value)
    if k > 0:
        if field not in ISO_FIELDS:
            raise ValueError("inputs: iso_field = %r: one of %s" % (field, ", ".join(ISO_FIELDS)))
        if int(nl["dim_in"]) != 3:
            raise ValueError("inputs: iso_int > 0 needs dim_in = 3 (it is %d): surfaces are extracted from 3-D fields only" % int(nl["dim_in"]))
        if not abs(value) < float("inf"):
            raise ValueError("inputs: iso_value = %r is not finite" % (value,))
    return k, field, comp, value


def iso_header():
    """the header line of an isosurface .dat file"""
    return "#" + "step".rjust(7) + "time".rjust(27) + "".join(c.rjust(16 if c in ("ntri", "cut_cells") else 27) for c in adv.ISO_DAT_COLUMNS) + "\n"


def iso_line(istep, time, iso):
    """one data line of an isosurface .dat file, in the format of a diagnostics line: step (i8), time (es27.17e3), ntri and cut_cells (i16), area and volume_above (es27.17e3)"""
    return "%8d" % istep + plotfile._es(time) + "%16d%16d" % (iso.ntri, iso.cut_cells) + plotfile._es(iso.area) + plotfile._es(iso.volume_above) + "\n"


def run(text, nsteps=None, report=print, device=0, outdir=".", extrude_nz=16, files="plane", diag_int=None, particles=None, particle_int=None, prof_int=None, prof_axis=None,
        pdf_int=None, pdf_field=None, pdf_comp=None, pdf_range=None, pdf_nbins=None, iso_int=None, iso_field=None, iso_comp=None, iso_value=None):
    """the time loop of src/varden.f90:237-371 for max_step steps (or until stop_time); plot / checkpoint files at step 0 of a fresh
    run and after every plot_int-th / chk_int-th step (:207-221, :349-361) under outdir.  diag_int > 0 (the namelist's key, or the argument over it): the run
    diagnostics of the state the run starts from and after every diag_int-th step, one line each under a header line, in <outdir>/<diag_file_name>; 0: no
    call, no file.  Tracer particles (the namelist's particle_lattice, particle_int, particle_base_name; the arguments particles = (nx, ny, nz) and particle_int over
    them): moved by every step, <particle_base_name>NNNNN with positions, states, velocity and scalars at the start and after every particle_int-th step, a file
    Particles inside every checkpoint, read back by a restart; no lattice: no call, no file.  prof_int > 0 (the namelist's key, or the argument over it): the plane-averaged profiles
    (advance.profiles) of the state the run starts from and after every prof_int-th step along prof_axis (numbered from 1; -1: the problem's last direction), one
    file <prof_base_name>NNNNN each (profile_text); 0: no call, no file.  pdf_int > 0 (the namelist's key, or the argument over it): the distribution by value (advance.pdf)
    of pdf_field / pdf_comp (numbered from 1) on [pdf_lo, pdf_hi) in pdf_nbins bins for the state the run starts from and after every pdf_int-th step, one file
    <pdf_base_name>NNNNN each (pdf_text); pdf_range = (lo, hi) goes over pdf_lo and pdf_hi; 0: no call, no file.  iso_int > 0 (the namelist's key, or the argument over it):
    the surface iso_field / iso_comp (numbered from 1) = iso_value (the drivers' isosurface) of the state the run starts from and after every iso_int-th step, one binary PLY
    file <iso_base_name>NNNNN.ply each (advance.write_iso) and one line -- step, time, ntri, cut_cells, area, volume_above -- in <iso_base_name>.dat; 0: no call, no file"""
    nl = dict(DEFAULTS)
    nl.update(parse_namelist(text))
    pdf_int, pdf_field, pdf_comp, pdf_lo, pdf_hi, pdf_nbins = pdf_keys(nl, pdf_int, pdf_field, pdf_comp, pdf_range, pdf_nbins)      # (refused before anything is built)
    iso_int, iso_field, iso_comp, iso_value = iso_keys(nl, iso_int, iso_field, iso_comp, iso_value)
    nl, G = build(text, device=device, outdir=outdir, extrude_nz=extrude_nz, files=files, nl=nl)
    max_step = int(nl["max_step"]) if nsteps is None else nsteps
    stop_time = float(nl["stop_time"])
    plot_int, chk_int = int(nl["plot_int"]), int(nl["chk_int"])
    G.files_written = []
    G.inputs_text, G.job_name = text, str(nl["job_name"])
    grids_file = os.path.join(outdir, str(nl["grids_file_name"])) if nl["grids_file_name"] else None
    if grids_file and int(nl["restart"]) < 0 and hasattr(G, "nregrids"):
        plotfile.write_grids(grids_file, G, 0)                               # initialize.f90:340: the initial adaptive grids
    regrids_seen = [getattr(G, "nregrids", 0)]

    last = dict(plt=-1, chk=-1)

    def dump(final=False):
        """every plot_int-th / chk_int-th step; final: the last step once more if it has not been written (src/varden.f90:374-377)"""
        if plot_int > 0 and (G.istep % plot_int == 0 or final) and last["plt"] != G.istep:
            G.files_written.append(plotfile.write_plotfile(G, base=os.path.join(outdir, str(nl["plot_base_name"]))))
            last["plt"] = G.istep
        if chk_int > 0 and (G.istep % chk_int == 0 or final) and last["chk"] != G.istep:
            G.files_written.append(plotfile.write_checkfile(G, base=os.path.join(outdir, str(nl["check_base_name"]))))
            if G.particles is not None:
                G.particles.write(os.path.join(outdir, "%s%05d" % (nl["check_base_name"], G.istep), PARTICLE_FILE), time=G.time)
            last["chk"] = G.istep

    # tracer particles: a fresh run seeds the lattice, a restart reads the checkpoint's Particles file; with neither nothing below runs
    particle_int = int(nl["particle_int"]) if particle_int is None else int(particle_int)
    lattice = namelist_particle_lattice(nl, text) if particles is None else tuple(int(v) for v in particles)
    if int(nl["restart"]) >= 0:
        pfile = os.path.join(outdir, "%s%05d" % (nl["check_base_name"], int(nl["restart"])), PARTICLE_FILE)
        if os.path.exists(pfile):
            G.particles = adv.Particles.read(pfile)[0]
    elif any(lattice):
        G.particles = adv.Particles(adv.particle_lattice([max(1, v) for v in lattice[:G.dm]], domain_extent(G)))

    def particle_file():
        path = os.path.join(outdir, "%s%05d" % (nl["particle_base_name"], G.istep))
        G.particles.write(path, time=G.time, columns=particle_columns(G))
        G.files_written.append(path)

    diag_int = int(nl["diag_int"]) if diag_int is None else int(diag_int)
    diag_path = os.path.join(outdir, str(nl["diag_file_name"]))

    def diag():
        with open(diag_path, "a") as f:
            f.write(diag_line(G.istep, G.time, G.dt, G.diagnostics()))

    prof_int = int(nl["prof_int"]) if prof_int is None else int(prof_int)
    prof_axis = int(nl["prof_axis"]) if prof_axis is None else int(prof_axis)

    def prof():
        path = os.path.join(outdir, "%s%05d" % (nl["prof_base_name"], G.istep))
        with open(path, "w") as f:
            f.write(profile_text(G.profiles(int(nl["dim_in"]) - 1 if prof_axis < 1 else prof_axis - 1), G.istep, G.time))
        G.files_written.append(path)

    def pdf():
        path = os.path.join(outdir, "%s%05d" % (nl["pdf_base_name"], G.istep))
        with open(path, "w") as f:
            f.write(pdf_text(G.pdf(pdf_field, pdf_comp - 1, pdf_lo, pdf_hi, pdf_nbins), G.istep, G.time))
        G.files_written.append(path)

    iso_dat = os.path.join(outdir, "%s.dat" % (nl["iso_base_name"],))

    def iso():
        path = os.path.join(outdir, "%s%05d.ply" % (nl["iso_base_name"], G.istep))
        S = G.isosurface(iso_field, iso_comp - 1, iso_value)
        adv.write_iso(path, S, G.time)
        if getattr(G, "rank", 0) == 0:
            with open(iso_dat, "a") as f:
                f.write(iso_line(G.istep, G.time, S))
        G.files_written.append(path)

    if diag_int > 0:
        with open(diag_path, "w") as f:
            f.write(diag_header(G.nscal, G.dm))
        diag()
    if iso_int > 0:
        if getattr(G, "rank", 0) == 0:
            with open(iso_dat, "w") as f:
                f.write(iso_header())
        iso()
    if prof_int > 0:
        prof()
    if pdf_int > 0:
        pdf()
    if int(nl["restart"]) < 0:
        dump()
        if G.particles is not None and particle_int > 0:
            particle_file()
    while G.istep < max_step and (stop_time < 0 or G.time < stop_time):
        G.step()
        if grids_file and getattr(G, "nregrids", 0) != regrids_seen[0]:      # varden.f90:263-264
            regrids_seen[0] = G.nregrids
            plotfile.write_grids(grids_file, G, G.istep)
        if report:
            report(G)
        if diag_int > 0 and G.istep % diag_int == 0:
            diag()
        if prof_int > 0 and G.istep % prof_int == 0:
            prof()
        if pdf_int > 0 and G.istep % pdf_int == 0:
            pdf()
        if iso_int > 0 and G.istep % iso_int == 0:
            iso()
        if G.particles is not None and particle_int > 0 and G.istep % particle_int == 0:
            particle_file()
        dump()
    if G.istep > (int(nl["restart"]) if int(nl["restart"]) >= 0 else 0):
        dump(final=True)
    return nl, G
