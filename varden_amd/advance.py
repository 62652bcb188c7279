"""The reference's hot-path entry points, same names and argument order, over the C-ABI.

    advance_timestep   reference src/advance_timestep.f90:26-44
    estdt              reference src/estdt.f90:15
    hgproject          reference src/hgproject.f90:17-18
    macproject         reference src/macproject.f90:20
    velpred / mkflux / update / mkvelforce / mkscalforce / make_at_halftime : the per-kernel modules

Multifab arguments are lists with one :class:`MultiFab` per level, as in the Fortran (``sold(:)``).
"""
import ctypes as C
import os

from . import capi
from .boxlib import handle_array
from .capi import check


def _dx(dx):
    flat = [float(v) for lev in dx for v in lev] if hasattr(dx[0], "__len__") else [float(v) for v in dx]
    return (C.c_double * len(flat))(*flat)


def advance_timestep(istep, mla, sold, uold, snew, unew, gp, p, ext_vel_force, ext_scal_force,
                     the_bc_tower, dt, time, dx, press_comp, proj_type):
    lib = capi.load()
    check(lib.vdn_advance_timestep(istep, mla.h, handle_array(sold), handle_array(uold), handle_array(snew),
                                   handle_array(unew), handle_array(gp), handle_array(p),
                                   handle_array(ext_vel_force), handle_array(ext_scal_force), the_bc_tower.h,
                                   float(dt), float(time), _dx(dx), press_comp, proj_type))


def estdt(lev, u, s, gp, ext_vel_force, dx, dtold):
    """returns dt (the reference's intent(out) argument)"""
    out = C.c_double()
    check(capi.load().vdn_estdt(lev, u.h, s.h, gp.h, ext_vel_force.h, _dx(dx), float(dtold), C.byref(out)))
    return out.value


def hgproject(proj_type, mla, unew, uold, rhohalf, p, gp, dx, dt, the_bc_tower, press_comp):
    check(capi.load().vdn_hgproject(proj_type, mla.h, handle_array(unew), handle_array(uold), handle_array(rhohalf),
                                    handle_array(p), handle_array(gp), _dx(dx), float(dt), the_bc_tower.h, press_comp))


def macproject(mla, umac, rho, mac_rhs, dx, the_bc_tower, bc_comp):
    """umac: list per level of [umac, vmac, wmac]"""
    flat = [m for lev in umac for m in lev]
    check(capi.load().vdn_macproject(mla.h, handle_array(flat), handle_array(rho), handle_array(mac_rhs), _dx(dx),
                                     the_bc_tower.h, bc_comp))


def last_step_timing():
    t = (C.c_double * 5)()
    capi.load().vdn_last_step_timing(t)
    return dict(scalar=t[0], velocity=t[1], mac=t[2], hg=t[3], total=t[4])


def last_solver_stats(which):
    cyc, r0, r = C.c_int(), C.c_double(), C.c_double()
    capi.load().vdn_last_solver_stats(0 if which == "mac" else 1, C.byref(cyc), C.byref(r0), C.byref(r))
    return cyc.value, r0.value, r.value


def last_bottom_stats(which):
    """Krylov bottom solver of the last cell-centred ("mac") / nodal ("hg") solve: dict(calls, iters, max_iters, breakdowns); zeros with the bottom sweeps"""
    v = [C.c_int() for _ in range(4)]
    check(capi.load().vdn_last_bottom_stats(0 if which == "mac" else 1, *[C.byref(x) for x in v]))
    return dict(calls=v[0].value, iters=v[1].value, max_iters=v[2].value, breakdowns=v[3].value)


def last_bottom_form(which):
    """what the last cell-centred ("mac") / nodal ("hg") solve ran at its bottom level: 0 the sweeps, 1 a Krylov solver in one workgroup, 2 over the whole GPU"""
    return int(capi.load().vdn_last_bottom_form(0 if which == "mac" else 1))


# ---- per-kernel modules (single level) ------------------------------------------------------------
def _iv(x):
    return (C.c_int * len(x))(*[int(v) for v in x])


def slope(s, slope_mf, dir, bccomp, bct):
    check(capi.load().vdn_k_slope(s.h, slope_mf.h, dir, bccomp, bct.h))


def slopes_march(s, sl, bccomp, bct, want_max=False):
    """the predictors' slope launch by itself: the slopes of s along x, y, z into the three multifabs sl; want_max: returns max |s| over the valid cells"""
    m = C.c_double(0.0)
    check(capi.load().vdn_k_slopes_march(s.h, sl[0].h, sl[1].h, sl[2].h, bccomp, bct.h, C.byref(m) if want_max else None))
    return m.value if want_max else None


def velpred(u, umac, force, dx, dt, bct):
    check(capi.load().vdn_k_velpred(u.h, handle_array(umac), force.h, _dx(dx), float(dt), bct.h))


def mkflux(s, sedge, flux, umac, force, mac_rhs, dx, dt, bct, is_vel, is_conservative):
    check(capi.load().vdn_k_mkflux(s.h, handle_array(sedge), handle_array(flux), handle_array(umac), force.h, mac_rhs.h,
                                   _dx(dx), float(dt), bct.h, 1 if is_vel else 0, _iv(is_conservative)))


def update(sold, umac, sedge, flux, force, snew, dx, dt, is_vel, is_cons, bct):
    check(capi.load().vdn_k_update(sold.h, handle_array(umac), handle_array(sedge), handle_array(flux), force.h, snew.h,
                                   _dx(dx), float(dt), 1 if is_vel else 0, _iv(is_cons), bct.h))


def mkvelforce(vel_force, ext_vel_force, s, gp, lapu, visc_fac, bct):
    check(capi.load().vdn_k_mkvelforce(vel_force.h, ext_vel_force.h, s.h, gp.h, lapu.h if lapu else None, float(visc_fac), bct.h))


def mkscalforce(scal_force, ext_scal_force, laps, diff_fac, bct):
    check(capi.load().vdn_k_mkscalforce(scal_force.h, ext_scal_force.h, laps.h if laps else None, float(diff_fac), bct.h))


def make_at_halftime(rhohalf, sold, snew, in_comp, out_comp, bct):
    check(capi.load().vdn_k_make_at_halftime(rhohalf.h, sold.h, snew.h, in_comp, out_comp, bct.h))


def cc_solve(rh, phi, beta, dx, bc, rel_eps, abs_eps=-1.0, max_iter=100, alpha=None):
    """alpha: a cell multifab -- (alpha - div beta grad) phi = rh, the solve of the viscous and diffusive steps"""
    cyc, r0, r = C.c_int(), C.c_double(), C.c_double()
    flat = _iv([bc[d][s] for d in range(3) for s in range(2)])
    if alpha is not None:
        check(capi.load().vdn_cc_solve_alpha(rh.h, phi.h, alpha.h, handle_array(beta), _dx(dx), flat, rel_eps, abs_eps, max_iter,
                                             C.byref(cyc), C.byref(r0), C.byref(r)))
        return cyc.value, r0.value, r.value
    check(capi.load().vdn_cc_solve(rh.h, phi.h, handle_array(beta), _dx(dx), flat, rel_eps, abs_eps, max_iter,
                                   C.byref(cyc), C.byref(r0), C.byref(r)))
    return cyc.value, r0.value, r.value


def cc_smooth(rh, phi, beta, dx, bc, nsweeps):
    flat = _iv([bc[d][s] for d in range(3) for s in range(2)])
    check(capi.load().vdn_cc_smooth(rh.h, phi.h, handle_array(beta), _dx(dx), flat, nsweeps))


def nd_solve(rh, phi, coeffs, u, dx, bc, rel_eps, abs_eps=-1.0, max_iter=100):
    cyc, r0, r = C.c_int(), C.c_double(), C.c_double()
    flat = _iv([bc[d][s] for d in range(3) for s in range(2)])
    check(capi.load().vdn_nd_solve(rh.h, phi.h, coeffs.h, u.h if u else None, _dx(dx), flat, rel_eps, abs_eps, max_iter,
                                   C.byref(cyc), C.byref(r0), C.byref(r)))
    return cyc.value, r0.value, r.value


def bench_cc_smoother(rh, phi, beta, dx, bc, nlaunch, rho=None):
    """rho: the density behind beta -- the pass macproject runs (coefficients recomputed from rho); None: the stored-coefficient pass"""
    ms, cells = C.c_double(), C.c_long()
    flat = _iv([bc[d][s] for d in range(3) for s in range(2)])
    check(capi.load().vdn_bench_cc_smoother(rh.h, phi.h, handle_array(beta), rho.h if rho is not None else None, _dx(dx), flat, nlaunch,
                                            C.byref(ms), C.byref(cells)))
    return ms.value, cells.value


def bench_cc_smoother_in_solve(rh, phi, beta, dx, bc, nsweeps, nlaunch, rho):
    """the colour passes as a solve launches them (sweeps time-skewed over plane slabs): (ms per pass over the whole level, cells); cells = 0: no slab schedule here"""
    ms, cells = C.c_double(), C.c_long()
    flat = _iv([bc[d][s] for d in range(3) for s in range(2)])
    check(capi.load().vdn_bench_cc_smoother_in_solve(rh.h, phi.h, handle_array(beta), rho.h, _dx(dx), flat, nsweeps, nlaunch, C.byref(ms), C.byref(cells)))
    return ms.value, cells.value


# ---- multi-level operators (two levels) -----------------------------------------------------------------------------------
def ml_cc_restriction(crse, fine, icomp=0, nc=None):
    check(capi.load().vdn_ml_cc_restriction(crse.h, fine.h, icomp, crse.nc if nc is None else nc))


def ml_edge_restriction(crse, fine, dir):
    check(capi.load().vdn_ml_edge_restriction(crse.h, fine.h, dir))


def fill_ghost_cells(fine, crse, icomp=0, nc=None):
    check(capi.load().vdn_multifab_fill_ghost_cells(fine.h, crse.h, icomp, fine.nc if nc is None else nc))


def create_umac_grown(fine, crse, dir):
    check(capi.load().vdn_create_umac_grown(fine.h, crse.h, dir))


def ml_restrict_and_fill(mfs, icomp, bcomp, nc, bct, same_boundary=False):
    check(capi.load().vdn_ml_restrict_and_fill(len(mfs), handle_array(mfs), icomp, bcomp, nc, 1 if same_boundary else 0, bct.h))


def make_new_grids(s, lev, buf_wid=2, nest=2, min_eff=0.9, min_width=4, blocking=4, max_grid_size=256, maxboxes=4096):
    """tag_boxes (src/tag_boxes.f90) on component 0 of `s` (the state of level `lev`, 1-based) + FBoxLib's make_new_grids
    (src/initialize.f90:247-248): the boxes of level lev+1 in that level's index space ([] = nothing tagged), and the tag count"""
    boxes = (capi.Box * maxboxes)()
    nb, nt = C.c_int(), C.c_long()
    check(capi.load().vdn_make_new_grids(s.h, lev, buf_wid, nest, min_eff, min_width, blocking, max_grid_size, maxboxes, boxes,
                                         C.byref(nb), C.byref(nt)))
    return [(tuple(boxes[i].lo), tuple(boxes[i].hi)) for i in range(nb.value)], nt.value


def tag_boxes(s, lev):
    """tag_boxes of src/tag_boxes.f90 on component 0 of `s` (level `lev`, 1-based): uint8 array over the level's domain (x first)"""
    import numpy as np
    lo, hi = s.mla.pd[s.lev]
    n = tuple(hi[d] - lo[d] + 1 for d in range(3))
    tags = np.zeros(n, dtype=np.uint8, order="F")
    check(capi.load().vdn_tag_boxes(s.h, lev, tags.ctypes.data_as(C.POINTER(C.c_ubyte))))
    return tags


def tag_criteria(criteria):
    """the ``vdn_tag_criterion`` array for a list of criteria, each a dict ``dict(field="vorticity", comp=1, gt=[...], lt=[...])`` or a tuple
    ``(field, comp, gt, lt)`` (trailing entries may be left out).  field: scalar, scalar_grad, vorticity or magvel; comp: 1-based component of the
    state (default 1; velocity fields ignore it); gt / lt: one threshold per level or a single number -- a list shorter than the hierarchy repeats its
    last value (the reference's ``case default``), a side left out (or None) is open.  Returns (array, count)."""
    if isinstance(criteria, C.Array) and criteria._type_ is capi.TagCriterion:      # built before (the drivers convert once, every regrid passes the array)
        return criteria, len(criteria)
    if isinstance(criteria, (dict, tuple)):
        criteria = [criteria]
    criteria = list(criteria)
    if not 1 <= len(criteria) <= capi.TAG_MAX_CRITERIA:
        raise ValueError("tag criteria: %d given, 1 .. %d allowed" % (len(criteria), capi.TAG_MAX_CRITERIA))
    arr = (capi.TagCriterion * len(criteria))()
    for q, c in enumerate(criteria):
        if isinstance(c, capi.TagCriterion):
            arr[q] = c
            continue
        if not isinstance(c, dict):
            c = dict(zip(("field", "comp", "gt", "lt"), c))
        unknown = set(c) - {"field", "comp", "gt", "lt"}
        if unknown or "field" not in c:
            raise ValueError("tag criterion %d: keys field, comp, gt, lt; got %s" % (q + 1, sorted(c)))
        if c["field"] not in capi.TAG_FIELDS:
            raise ValueError("tag criterion %d: unknown field %r (one of %s)" % (q + 1, c["field"], ", ".join(capi.TAG_FIELDS)))
        arr[q].field = capi.TAG_FIELDS[c["field"]]
        arr[q].comp = int(c.get("comp", 1)) - 1
        for name, open_side in (("gt", -float("inf")), ("lt", float("inf"))):
            v = c.get(name)
            v = [open_side] if v is None else ([float(v)] if not hasattr(v, "__len__") else [float(x) for x in v])
            if not 1 <= len(v) <= capi.MAXLEV:
                raise ValueError("tag criterion %d: %s holds %d thresholds (1 .. %d)" % (q + 1, name, len(v), capi.MAXLEV))
            for lev in range(capi.MAXLEV):
                getattr(arr[q], name)[lev] = v[min(lev, len(v) - 1)]
    return arr, len(criteria)


def _by_args(u, dx, bct, criteria):
    arr, n = tag_criteria(criteria)
    d = None if dx is None else (C.c_double * 3)(*(list(dx) + [1.0] * 3)[:3])
    return u.h if u is not None else None, d, bct.h if bct is not None else None, n, arr


def make_new_grids_by(s, u, dx, bct, lev, criteria, buf_wid=2, nest=2, min_eff=0.9, min_width=4, blocking=4, max_grid_size=256, maxboxes=4096):
    """make_new_grids with the cells of level `lev` (1-based) tagged by `criteria` (see tag_criteria) instead of src/tag_boxes.f90's rules; u, dx and
    bct may be None when no criterion reads the velocity.  Returns the boxes of level lev+1 and the tag count."""
    boxes = (capi.Box * maxboxes)()
    nb, nt = C.c_int(), C.c_long()
    uh, d, bh, n, arr = _by_args(u, dx, bct, criteria)
    check(capi.load().vdn_make_new_grids_by(s.h, uh, d, bh, lev, n, arr, buf_wid, nest, min_eff, min_width, blocking, max_grid_size, maxboxes, boxes,
                                            C.byref(nb), C.byref(nt)))
    return [(tuple(boxes[i].lo), tuple(boxes[i].hi)) for i in range(nb.value)], nt.value


def tag_boxes_by(s, u, dx, bct, lev, criteria):
    """the tag bitmap of `criteria` on level `lev` (1-based): uint8 array over the level's domain (x first)"""
    import numpy as np
    lo, hi = s.mla.pd[s.lev]
    n = tuple(hi[d] - lo[d] + 1 for d in range(3))
    tags = np.zeros(n, dtype=np.uint8, order="F")
    uh, d, bh, nc, arr = _by_args(u, dx, bct, criteria)
    check(capi.load().vdn_tag_boxes_by(s.h, uh, d, bh, lev, nc, arr, tags.ctypes.data_as(C.POINTER(C.c_ubyte))))
    return tags


def fillpatch(fine, crse, icomp, nc):
    """fillpatch(fine, crse, 0, ...) of src/regrid.f90:311-325: valid cells of a new fine level from the coarser one"""
    check(capi.load().vdn_fillpatch(fine.h, crse.h, icomp, nc))


def make_vorticity(vort, comp, u, dx, bct):
    """make_vorticity(vort, comp, u, dx, bc) of src/makevort.f90:16-57 (comp 0-based; fills the ghost cells of u)"""
    d = (C.c_double * 3)(*(list(dx) + [1.0] * 3)[:3])
    check(capi.load().vdn_make_vorticity(vort.h, comp, u.h, d, bct.h))


def make_vorticity_plane(vort, comp, u, dx, bct):
    """makevort_2d's rule (src/makevort.f90:93-156) on every plane of a z-uniform 3-D copy; dx: the two in-plane spacings"""
    d = (C.c_double * 3)(*(list(dx[:2]) + [1.0]))
    check(capi.load().vdn_make_vorticity_plane(vort.h, comp, u.h, d, bct.h))


def make_magvel(magvel, comp, u):
    """make_magvel(magvel, comp, u) of src/makevort.f90:59-91"""
    check(capi.load().vdn_make_magvel(magvel.h, comp, u.h))


def ml_nodal_prolongation(fine, crse):
    check(capi.load().vdn_ml_nodal_prolongation(fine.h, crse.h))


def copy_layouts(dst, dcomp, src, scomp, nc):
    """multifab_copy_c between two multifabs of one level whose box lists differ (src/regrid.f90:333-337)"""
    check(capi.load().vdn_multifab_copy_layouts(dst.h, dcomp, src.h, scomp, nc))


# ---- plot files and checkpoints inside the library (csrc/fabio.hip; one rank) ------------------------------------------------------------
def _cbox(lo, hi):
    b = capi.Box()
    for d in range(3):
        b.lo[d], b.hi[d] = int(lo[d]), int(hi[d])
    return b


def _dv(v):
    return None if v is None else (C.c_double * max(3, len(v)))(*[float(x) for x in v])


def _rr(rr):
    return (C.c_int * max(1, len(rr)))(*[int(r) for r in rr])


def fabio_ml_multifab_write_d(dirname, mfs, rr, names=None, pd=None, prob_lo=None, prob_hi=None, time=0.0, dx=None, staging_bytes=0):
    """fabio_ml_multifab_write_d(mfs, rr, dirname, names, bounding_box, prob_lo, prob_hi, time, dx) of src/varden.f90:568-573: the files of
    plotfile.write_ml_multifab, byte for byte; mfs: one multifab per level, rr: one ratio per pair of levels, pd: (lo, hi) of the level-0 domain"""
    nm = None if names is None else (C.c_char_p * len(names))(*[str(n).encode() for n in names])
    check(capi.load().vdn_fabio_ml_multifab_write_d(str(dirname).encode(), len(mfs), handle_array(mfs), _rr(rr), nm,
                                                    None if pd is None else C.byref(_cbox(*pd)), _dv(prob_lo), _dv(prob_hi), float(time), _dv(dx), int(staging_bytes)))


def fabio_ml_multifab_info(dirname):
    """levels, dimension, components, nodal flags, boxes per level, ratios and time of a hierarchy on disk (text only: needs no GPU)"""
    nl, dm, nc, t = C.c_int(), C.c_int(), C.c_int(), C.c_double()
    nodal, nb, rr = (C.c_int * 3)(), (C.c_int * 4)(), (C.c_int * 4)()
    check(capi.load().vdn_fabio_ml_multifab_info(str(dirname).encode(), C.byref(nl), C.byref(dm), C.byref(nc), nodal, nb, rr, C.byref(t)))
    return dict(nlevs=nl.value, dm=dm.value, ncomp=nc.value, nodal=tuple(nodal), nboxes=list(nb)[:nl.value], rr=list(rr)[:nl.value - 1], time=t.value)


def fabio_ml_multifab_boxes(dirname, lev, nboxes):
    """the cell boxes [(lo, hi)] of one level of a hierarchy on disk, in the file's order (text only)"""
    arr = (capi.Box * max(1, int(nboxes)))()
    check(capi.load().vdn_fabio_ml_multifab_boxes(str(dirname).encode(), int(lev), arr, int(nboxes)))
    return [(tuple(arr[i].lo), tuple(arr[i].hi)) for i in range(int(nboxes))]


def fabio_ml_multifab_read_d(dirname, mfs, staging_bytes=0):
    """the data of a hierarchy on disk into multifabs built on its box lists (valid points; ghost cells keep their values)"""
    check(capi.load().vdn_fabio_ml_multifab_read_d(str(dirname).encode(), len(mfs), handle_array(mfs), int(staging_bytes)))


def checkpoint_write(dirname, state, pressure, rr, time, dt, staging_bytes=0):
    """checkpoint_write(dirname, mfs, mfs_nodal, rrs, time, dt) of src/checkpoint.f90:14-86"""
    check(capi.load().vdn_checkpoint_write(str(dirname).encode(), len(state), handle_array(state), handle_array(pressure), _rr(rr), float(time), float(dt),
                                           int(staging_bytes)))


def checkpoint_info(dirname):
    """the namelist of a checkpoint's Header (src/checkpoint.f90:100-112) and the ratios behind it (text only)"""
    nl, t, dt, rr = C.c_int(), C.c_double(), C.c_double(), (C.c_int * 4)()
    check(capi.load().vdn_checkpoint_info(str(dirname).encode(), C.byref(nl), C.byref(t), C.byref(dt), rr))
    return dict(nlevs=nl.value, time=t.value, dt=dt.value, rr=list(rr)[:nl.value - 1])


# ---- the same files for a 2-D problem run as its z-uniform 3-D copy: dm = 2 files of plane k = 0 ------------------------------------------
def _iv(v):
    return (C.c_int * max(1, len(v)))(*[int(x) for x in v])


def fabio_ml_multifab_write_plane_d(dirname, mfs, rr, comps, names=None, pd=None, prob_lo=None, prob_hi=None, time=0.0, dx=None, staging_bytes=0, vanish=(), defect=True):
    """plane k = 0 of the 3-D multifabs of a z-uniform copy as a dm = 2 hierarchy: file component c = source component comps[c]; the files of
    plotfile.write_ml_multifab(dm=2) for the plane arrays, byte for byte.  Returns (largest |f(i,j,k) - f(i,j,0)| over the listed components of all
    boxes, largest |value| of the components `vanish`), or None with defect=False"""
    nm = None if names is None else (C.c_char_p * len(names))(*[str(n).encode() for n in names])
    out = (C.c_double * 2)()
    check(capi.load().vdn_fabio_ml_multifab_write_plane_d(str(dirname).encode(), len(mfs), handle_array(mfs), _rr(rr), nm, None if pd is None else C.byref(_cbox(*pd)),
                                                          _dv(prob_lo), _dv(prob_hi), float(time), _dv(dx), int(staging_bytes), len(comps), _iv(comps), len(vanish),
                                                          _iv(vanish), out if defect else None))
    return (out[0], out[1]) if defect else None


def fabio_ml_multifab_read_plane_d(dirname, mfs, comps, staging_bytes=0):
    """a dm = 2 hierarchy on disk into the 3-D multifabs of a copy (cut along z in any way): file component c to every valid z-plane of comps[c]"""
    check(capi.load().vdn_fabio_ml_multifab_read_plane_d(str(dirname).encode(), len(mfs), handle_array(mfs), int(staging_bytes), len(comps), _iv(comps)))


def checkpoint_write_plane(dirname, state, pressure, rr, time, dt, comps, vanish=(), staging_bytes=0):
    """checkpoint_write of a z-uniform copy: State = components comps of state, Pressure nodal (1,1); returns the z-uniformity figures of the plane writer"""
    out = (C.c_double * 2)()
    check(capi.load().vdn_checkpoint_write_plane(str(dirname).encode(), len(state), handle_array(state), handle_array(pressure), _rr(rr), float(time), float(dt),
                                                 int(staging_bytes), len(comps), _iv(comps), len(vanish), _iv(vanish), out))
    return out[0], out[1]


# ---- run diagnostics ---------------------------------------------------------------------------------------------------------------------
def diagnostics(mla, u, s, dx, bct, vort=True):
    """vdn_diagnostics over the composite grid of the hierarchy (u, s: one multifab per level; dx: one list per level): a dict of the members of vdn_diag --
    cells, cells_lev, nonfinite, volume, volume_lev, sum_s (sum_s[0]: the mass), momentum, kinetic, enstrophy, s_min, s_max, u_min, u_max, magvel_max,
    vort_min, vort_max -- arrays cut to nlev, nscal and dm entries.  vort=True adds the vorticity terms (0 otherwise): they read one ghost layer of u, which the
    CALLER has filled (the drivers' fill_state_ghosts); bct may be None without them.  Sums have a fixed order, extrema are exact: equal bits call after call and
    on any number of ranks."""
    lib = capi.load()
    prm = capi.Params()
    check(lib.vdn_get_params(C.byref(prm)))
    nlev, dm, ns = len(u), prm.dm, prm.nscal
    levs = dx if hasattr(dx[0], "__len__") else [dx]
    flat = [float(v) for lev in levs for v in (list(lev) + [1.0] * 3)[:3]]
    out = capi.Diag()
    check(lib.vdn_diagnostics(nlev, mla.h, handle_array(u), handle_array(s), (C.c_double * len(flat))(*flat), bct.h if bct is not None else None,
                              capi.DIAG_VORT if vort else 0, C.byref(out)))
    cut = dict(cells_lev=nlev, volume_lev=nlev, sum_s=ns, s_min=ns, s_max=ns, momentum=dm, u_min=dm, u_max=dm)
    return {name: (list(getattr(out, name))[:cut[name]] if name in cut else getattr(out, name)) for name, _ in capi.Diag._fields_}


def diag_columns(nscal, dm):
    """the columns of a diagnostics file after step, time and dt (inputs.run with diag_int > 0; varden_main writes the same): vdn_diag's members in struct
    order without the per-level arrays, arrays cut to nscal and dm entries"""
    cols = ["cells", "nonfinite", "volume"] + ["sum_s%d" % (c + 1) for c in range(nscal)] + ["momentum%d" % (d + 1) for d in range(dm)] + ["kinetic", "enstrophy"]
    for name, n in (("s_min", nscal), ("s_max", nscal), ("u_min", dm), ("u_max", dm)):
        cols += ["%s%d" % (name, c + 1) for c in range(n)]
    return cols + ["magvel_max", "vort_min", "vort_max"]


def diag_values(d):
    """the figures of one diagnostics dict in diag_columns' order"""
    return ([d["cells"], d["nonfinite"], d["volume"]] + d["sum_s"] + d["momentum"] + [d["kinetic"], d["enstrophy"]] + d["s_min"] + d["s_max"] + d["u_min"] + d["u_max"]
            + [d["magvel_max"], d["vort_min"], d["vort_max"]])


# ---- plane-averaged profiles (csrc/profiles.hip; include/varden_amd.h states the definition) ----------------------------------------------
PROFILE_GROUPS = ("volume", "s", "ss", "u", "ru", "ruu", "sua", "s_min", "s_max", "u_min", "u_max")      # the row groups in row order (vdn_profile_layout)


def profiles_layout(dm, nscal):
    """vdn_profiles_layout as a dict: nrow and, per row group of PROFILE_GROUPS, (first row, number of rows)"""
    lay = capi.ProfileLayout()
    check(capi.load().vdn_profiles_layout(int(dm), int(nscal), C.byref(lay)))
    first = [getattr(lay, g) for g in PROFILE_GROUPS] + [lay.nrow]
    out = {g: (first[i], first[i + 1] - first[i]) for i, g in enumerate(PROFILE_GROUPS)}
    out["nrow"] = lay.nrow
    return out


def profile_columns(nscal, dm):
    """the names of the rows in row order (the columns of a profile file after x and cells): components are numbered from 1, ruu by its pair (ruu12 = rho u1 u2),
    sua from the first tracer (sua2)"""
    one = lambda base, n, first=1: ["%s%d" % (base, c + first) for c in range(n)]      # noqa: E731
    return (["volume"] + one("s", nscal) + one("ss", nscal) + one("u", dm) + one("ru", dm) + ["ruu%d%d" % (d + 1, e + 1) for d in range(dm) for e in range(d, dm)]
            + one("sua", nscal - 1, 2) + one("s_min", nscal) + one("s_max", nscal) + one("u_min", dm) + one("u_max", dm))


class Profiles:
    """the result of vdn_profiles along `axis`: x (bin centres), cells (composite cells per bin), rows (nrow, nbins) and every row group by name -- P["volume"] is
    (nbins,), every other group (rows of the group, nbins); ruu_pairs names the (d, e) of ruu's rows.  mean(name) = rows / volume: the plane averages."""

    def __init__(self, axis, dm, nscal, x, rows, cells):
        self.axis, self.dm, self.nscal, self.x, self.rows, self.cells = axis, dm, nscal, x, rows, cells
        self.layout = profiles_layout(dm, nscal)
        self.ruu_pairs = [(d, e) for d in range(dm) for e in range(d, dm)]

    def __getitem__(self, name):
        if name == "cells":
            return self.cells
        if name == "x":
            return self.x
        first, n = self.layout[name]
        return self.rows[first] if name == "volume" else self.rows[first:first + n]

    def keys(self):
        return ("x", "cells") + PROFILE_GROUPS

    def mean(self, name):
        if name not in ("s", "ss", "u", "ru", "ruu", "sua"):
            raise KeyError("mean(%r): a plane average is a sum row divided by the volume row" % (name,))
        return self[name] / self["volume"]


def profiles(mla, u, s, dx, axis):
    """vdn_profiles over the composite grid of the hierarchy (u, s: one multifab per level; dx: one list per level; axis 0-based): a Profiles object.  Bins are the
    planes of the FINEST level along the axis; a coarse cell contributes to each of the fine bins it spans.  No ghost cell is read.  Sums have a fixed order, extrema
    are exact: equal bits call after call and on any number of ranks.  Collective."""
    import numpy as np
    lib = capi.load()
    prm = capi.Params()
    check(lib.vdn_get_params(C.byref(prm)))
    nlev, axis = len(u), int(axis)
    levs = dx if hasattr(dx[0], "__len__") else [dx]
    nbins = lib.vdn_profiles_nbins(nlev, mla.h, axis)
    if nbins < 0:
        check(1)
    nrow = profiles_layout(prm.dm, prm.nscal)["nrow"]
    rows, cells = np.zeros((nrow, nbins)), np.zeros(nbins, dtype=np.int64)
    check(lib.vdn_profiles(nlev, mla.h, handle_array(u), handle_array(s), _dx3(levs), axis, nbins, rows.ctypes.data_as(C.POINTER(C.c_double)),
                           cells.ctypes.data_as(C.POINTER(C.c_longlong))))
    x = (np.arange(nbins) + 0.5) * float(levs[nlev - 1][axis])
    return Profiles(axis, prm.dm, prm.nscal, x, rows, cells)


# ---- PDFs and conditional sums by value (csrc/pdf.hip; include/varden_amd.h states the definition) ------------------------------------------
PDF_GROUPS = ("volume", "q", "s", "u", "ru", "ke")      # the row groups in row order (vdn_pdf_layout)
PDF_FIELDS = {"scalar": 0, "velocity": 1, "magvel": 2, "vorticity": 3}      # VDN_PDF_SCALAR ...
PDF_MAX_BINS, PDF2_MAX_BINS, _MAXLEV = 256, 64, 4


def pdf_layout(dm, nscal):
    """vdn_pdf_layout as a dict: nrow and, per row group of PDF_GROUPS, (first row, number of rows)"""
    lay = capi.PdfLayout()
    check(capi.load().vdn_pdf_layout(int(dm), int(nscal), C.byref(lay)))
    first = [getattr(lay, g) for g in PDF_GROUPS] + [lay.nrow]
    out = {g: (first[i], first[i + 1] - first[i]) for i, g in enumerate(PDF_GROUPS)}
    out["nrow"] = lay.nrow
    return out


def pdf_columns(nscal, dm):
    """the names of the rows in row order (the columns of a pdf file after the slot centre and cells): components are numbered from 1"""
    one = lambda base, n: ["%s%d" % (base, c + 1) for c in range(n)]      # noqa: E731
    return ["volume", "q"] + one("s", nscal) + one("u", dm) + one("ru", dm) + ["ke"]


def _pdf_field(field):
    if isinstance(field, str):
        if field not in PDF_FIELDS:
            raise ValueError("pdf field %r: one of %s" % (field, ", ".join(sorted(PDF_FIELDS))))
        return PDF_FIELDS[field]
    return int(field)


class Pdf:
    """the result of vdn_pdf on the axis (field, comp, lo, hi, nbins): nbins + 2 slots -- "below", the bins, "above".  edges (nbins + 1,), centres (nbins + 2,: lo +
    (m + 0.5) w for m = -1 .. nbins), cells (nlev, nbins + 2), nan_cells, rows (nrow, nbins + 2) and every row group by name -- P["volume"], P["q"], P["ke"] are
    (nbins + 2,), P["s"], P["u"], P["ru"] (rows of the group, nbins + 2).  density(): the PDF over the bins; mean(name): the conditional means row / volume."""

    def __init__(self, field, comp, lo, hi, nbins, dm, nscal, rows, cells, nan_cells):
        import numpy as np
        self.field, self.comp, self.lo, self.hi, self.nbins, self.dm, self.nscal = field, int(comp), float(lo), float(hi), int(nbins), dm, nscal
        self.rows, self.cells, self.nan_cells = rows, cells, int(nan_cells)
        self.w = (self.hi - self.lo) / self.nbins
        self.edges = self.lo + np.arange(self.nbins + 1) * self.w
        self.edges[-1] = self.hi
        self.centres = self.lo + (np.arange(-1, self.nbins + 1) + 0.5) * self.w
        self.layout = pdf_layout(dm, nscal)

    def __getitem__(self, name):
        if name in ("cells", "edges", "centres", "nan_cells"):
            return getattr(self, name)
        first, n = self.layout[name]
        return self.rows[first] if name in ("volume", "q", "ke") else self.rows[first:first + n]

    def keys(self):
        return ("edges", "centres", "cells", "nan_cells") + PDF_GROUPS

    def density(self):
        """volume[1 .. nbins] / (sum of volume over the bins * w): integrates to 1 over [lo, hi) (NaN where no cell lies in the range)"""
        v = self["volume"][1:-1]
        return v / (v.sum() * self.w)

    def mean(self, name):
        """the conditional mean of a summed group per slot: row / volume (NaN in an empty slot)"""
        if name not in ("q", "s", "u", "ru", "ke"):
            raise KeyError("mean(%r): a conditional mean is a sum row divided by the volume row" % (name,))
        import numpy as np
        with np.errstate(divide="ignore", invalid="ignore"):
            return self[name] / self["volume"]


class Pdf2:
    """the result of vdn_pdf2: cells (nlev, n1 + 2, n2 + 2), volume (n1 + 2, n2 + 2), nan_cells, edges1 (n1 + 1,), edges2 (n2 + 1,)"""

    def __init__(self, cells, volume, nan_cells, edges1, edges2):
        self.cells, self.volume, self.nan_cells, self.edges1, self.edges2 = cells, volume, int(nan_cells), edges1, edges2


def _pdf_state(u, dx):
    lib = capi.load()
    prm = capi.Params()
    check(lib.vdn_get_params(C.byref(prm)))
    levs = dx if hasattr(dx[0], "__len__") else [dx]
    flat = [float(v) for lev in levs for v in (list(lev) + [1.0] * 3)[:3]]
    return lib, prm, len(u), (C.c_double * len(flat))(*flat)


def pdf(mla, u, s, dx, bct, field, comp, lo, hi, nbins):
    """vdn_pdf over the composite grid of the hierarchy (u, s: one multifab per level; dx: one list per level): a Pdf object.  field: 'scalar' | 'velocity' | 'magvel' |
    'vorticity' (or the VDN_PDF_ code), comp 0-based.  The vorticity reads one ghost layer of u, which the CALLER has filled (the drivers' fill_state_ghosts), and
    needs bct; the others read no ghost cell and take bct = None.  Counts are exact, sums have a fixed order: equal bits call after call and on any number of ranks.
    Collective."""
    import numpy as np
    lib, prm, nlev, dxc = _pdf_state(u, dx)
    nbins, code = int(nbins), _pdf_field(field)
    nrow = pdf_layout(prm.dm, prm.nscal)["nrow"]
    width = max(nbins, 0) + 2
    rows, cells, nan = np.zeros((nrow, width)), np.zeros((_MAXLEV, width), dtype=np.int64), C.c_longlong(0)
    check(lib.vdn_pdf(nlev, mla.h, handle_array(u), handle_array(s), dxc, bct.h if bct is not None else None, code, int(comp), nbins, float(lo), float(hi),
                      rows.ctypes.data_as(C.POINTER(C.c_double)), cells.ctypes.data_as(C.POINTER(C.c_longlong)), C.byref(nan)))
    return Pdf(field, comp, lo, hi, nbins, prm.dm, prm.nscal, rows, cells[:nlev], nan.value)


def pdf2(mla, u, s, dx, bct, field1, comp1, lo1, hi1, nbins1, field2, comp2, lo2, hi2, nbins2):
    """vdn_pdf2: the joint distribution of two bin fields over the composite grid, counts and volume only: a Pdf2 object.  Fields and ghost cells as for pdf"""
    import numpy as np
    lib, prm, nlev, dxc = _pdf_state(u, dx)
    n1, n2 = int(nbins1), int(nbins2)
    shape = (max(n1, 0) + 2, max(n2, 0) + 2)
    cells, volume, nan = np.zeros((_MAXLEV,) + shape, dtype=np.int64), np.zeros(shape), C.c_longlong(0)
    check(lib.vdn_pdf2(nlev, mla.h, handle_array(u), handle_array(s), dxc, bct.h if bct is not None else None, _pdf_field(field1), int(comp1), n1, float(lo1), float(hi1),
                       _pdf_field(field2), int(comp2), n2, float(lo2), float(hi2), cells.ctypes.data_as(C.POINTER(C.c_longlong)),
                       volume.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nan)))
    e1 = float(lo1) + np.arange(n1 + 1) * ((float(hi1) - float(lo1)) / n1)
    e2 = float(lo2) + np.arange(n2 + 1) * ((float(hi2) - float(lo2)) / n2)
    e1[-1], e2[-1] = float(hi1), float(hi2)
    return Pdf2(cells[:nlev], volume, nan.value, e1, e2)


# ---- values at points and tracer particles (csrc/particles.hip; include/varden_amd.h states the definitions) ------------------------------
def _dx3(dx):
    levs = dx if hasattr(dx[0], "__len__") else [dx]
    flat = [float(v) for lev in levs for v in (list(lev) + [1.0] * 3)[:3]]
    return (C.c_double * len(flat))(*flat)


# ---- isosurfaces (csrc/iso.hip, csrc/iso_cell.h; include/varden_amd.h states the definitions) ---------------------------------------------
ISO_DAT_COLUMNS = ("ntri", "cut_cells", "area", "volume_above")      # the columns of an isosurface .dat file after step and time


class Iso:
    """the result of vdn_isosurface: the members of vdn_iso by name (ntri, ntri_lev, cut_cells, cut_cells_lev, nonfinite_cells, written, area, area_lev, area_vec,
    volume_above, volume; the per-level lists cut to nlev), value (the iso value), tri (written, 3, 3) float64 -- [triangle][vertex][direction] in the output order
    -- and level (written,) uint8; both are None when no triangles were asked for."""

    def __init__(self, value, nlev, out, tri=None, level=None):
        self.value, self.nlev, self.tri, self.level = float(value), int(nlev), tri, level
        for name, ctype in capi.Iso._fields_:
            v = getattr(out, name)
            setattr(self, name, list(v)[:nlev if name.endswith("_lev") else 3] if hasattr(v, "__len__") else v)


def isosurface(mla, mf, comp, bccomp, dx, bct, value, triangles=True):
    """vdn_isosurface: the surface mf(comp) = value over the composite grid of the hierarchy by marching tetrahedra: an Iso.  mf: one cell-centred multifab per level
    with at least one ghost layer that the CALLER has filled; bccomp: the bc tower component of `comp` (0 for the velocity, dm for the scalars); dm = 3 only.
    triangles=True: the call sizes itself -- a count call first, then the triangles.  Counts are exact, sums and the triangle order are fixed: equal bits call after
    call and on any number of ranks.  Collective."""
    import numpy as np
    lib, out, nlev = capi.load(), capi.Iso(), len(mf)
    args = (nlev, mla.h, handle_array(mf), int(comp), int(bccomp), _dx3(dx), bct.h if bct is not None else None, float(value))
    check(lib.vdn_isosurface(*args, 0, None, None, C.byref(out)))
    if not triangles:
        return Iso(value, nlev, out)
    n = int(out.ntri)
    tri, level = np.zeros((n, 3, 3)), np.zeros(n, dtype=np.uint8)
    if n > 0:
        check(lib.vdn_isosurface(*args, n, tri.ctypes.data_as(C.POINTER(C.c_double)), level.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(out)))
        if out.written != n:
            raise capi.VardenError("vdn_isosurface: %d triangles counted, %d written" % (n, out.written))
    return Iso(value, nlev, out, tri, level)


def write_iso(path, iso, time):
    """vdn_isosurface_write: the triangles of an Iso as binary PLY (little endian, a triangle soup with a level per face); rank 0 writes"""
    import numpy as np
    if iso.tri is None:
        raise ValueError("write_iso: the Iso carries no triangles (isosurface(..., triangles=True))")
    tri, level = np.ascontiguousarray(iso.tri, dtype=np.float64), np.ascontiguousarray(iso.level, dtype=np.uint8)
    check(capi.load().vdn_isosurface_write(os.fsencode(path), tri.shape[0], tri.ctypes.data_as(C.POINTER(C.c_double)), level.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                           float(iso.value), float(time)))


def read_iso(path):
    """a file of write_iso: a dict with iso, time, tri (ntri, 3, 3) float64 and level (ntri,) uint8"""
    import numpy as np
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").split("\n")
    if head[:2] != ["ply", "format binary_little_endian 1.0"] or not head[2].startswith("comment VDN_ISO 1 iso "):
        raise ValueError("%s: not an isosurface file" % (path,))
    words = head[2].split()
    nvert, ntri = int(head[3].split()[2]), int(head[7].split()[2])
    if nvert != 3 * ntri or len(raw) != end + 24 * nvert + 14 * ntri:
        raise ValueError("%s: %d vertices and %d faces do not fit %d bytes" % (path, nvert, ntri, len(raw)))
    tri = np.frombuffer(raw, dtype="<f8", count=3 * nvert, offset=end).reshape(ntri, 3, 3).copy()
    faces = np.frombuffer(raw, dtype=np.dtype([("n", "u1"), ("v", "<i4", 3), ("level", "u1")]), count=ntri, offset=end + 24 * nvert)
    return dict(iso=float(words[4]), time=float(words[6]), tri=tri, level=faces["level"].copy(), indices=faces["v"].copy())


def _points(x):
    """positions as a contiguous (n, 3) float64 array; (n, 2) input gets z = 0"""
    import numpy as np
    a = np.atleast_2d(np.asarray(x, dtype=np.float64))
    if a.ndim != 2 or a.shape[1] not in (2, 3):
        raise ValueError("positions: an (n, 2) or (n, 3) array, got shape %r" % (a.shape,))
    if a.shape[1] == 2:
        a = np.concatenate([a, np.zeros((a.shape[0], 1))], axis=1)
    return np.ascontiguousarray(a)


def sample_points(mla, mf, x, dx, bct, comp=0, nc=None, bccomp=0):
    """vdn_sample_points: components comp .. comp + nc - 1 of the cell-centred multifabs mf (one per level, ghost cells filled by the caller) at the physical
    points x (n, 3): (values (n, nc), host level (n,)); a point outside the domain has level -1 and value 0.  bccomp: the bc tower component of `comp`
    (0 for the velocity, dm for the scalars).  Collective."""
    import numpy as np
    pts = _points(x)
    nc = mf[0].nc - comp if nc is None else int(nc)
    val = np.zeros((pts.shape[0], nc))
    lev = np.zeros(pts.shape[0], dtype=np.int32)
    check(capi.load().vdn_sample_points(len(mf), mla.h, handle_array(mf), comp, nc, bccomp, _dx3(dx), bct.h if bct is not None else None, pts.shape[0],
                                        pts.ctypes.data_as(C.POINTER(C.c_double)), val.ctypes.data_as(C.POINTER(C.c_double)),
                                        lev.ctypes.data_as(C.POINTER(C.c_int))))
    return val, lev


class Particles:
    """Lagrangian tracer particles on the device (vdn_particles_*): created at the physical positions x0 (n, 3), moved by `advance` (Heun between two velocity
    fields), never reordered.  state 0: active; 1: left through an inlet or outlet face (frozen at its last position inside)."""

    def __init__(self, x0=None, _handle=None):
        self.h = C.c_void_p()
        if _handle is not None:
            self.h = _handle
            return
        pts = _points(x0)
        check(capi.load().vdn_particles_create(pts.shape[0], pts.ctypes.data_as(C.POINTER(C.c_double)), C.byref(self.h)))

    def _count(self):
        n, a = C.c_long(), C.c_long()
        check(capi.load().vdn_particles_count(self.h, C.byref(n), C.byref(a)))
        return n.value, a.value

    @property
    def n(self):
        return self._count()[0]

    @property
    def active(self):
        return self._count()[1]

    def positions(self):
        import numpy as np
        x = np.zeros((self.n, 3))
        check(capi.load().vdn_particles_get(self.h, x.ctypes.data_as(C.POINTER(C.c_double)), None))
        return x

    def state(self):
        import numpy as np
        s = np.zeros(self.n, dtype=np.int32)
        check(capi.load().vdn_particles_get(self.h, None, s.ctypes.data_as(C.POINTER(C.c_int))))
        return s

    def advance(self, mla, u0, u1, dx, bct, dt):
        """one move from the velocity u0 (old time) to u1 (new time), both with their ghost cells filled"""
        check(capi.load().vdn_particles_advance(self.h, len(u0), mla.h, handle_array(u0), handle_array(u1), _dx3(dx), bct.h if bct is not None else None, float(dt)))

    def sample(self, mla, mf, dx, bct, comp=0, nc=None, bccomp=0, levels=False):
        """sample_points at the particles' positions (which stay on the device): values (n, nc); levels=True: (values, host levels)"""
        import numpy as np
        n = self.n
        nc = mf[0].nc - comp if nc is None else int(nc)
        val = np.zeros((n, nc))
        lev = np.zeros(n, dtype=np.int32)
        check(capi.load().vdn_particles_sample(self.h, len(mf), mla.h, handle_array(mf), comp, nc, bccomp, _dx3(dx), bct.h if bct is not None else None,
                                               val.ctypes.data_as(C.POINTER(C.c_double)), lev.ctypes.data_as(C.POINTER(C.c_int))))
        return (val, lev) if levels else val

    def write(self, path, time=0.0, columns=None):
        """one particle file: header, states, positions and the named columns (a dict name -> (n,) array, kept in its order)"""
        import numpy as np
        columns = columns or {}
        names = [str(k) for k in columns]
        cols = np.ascontiguousarray(np.array([np.asarray(columns[k], dtype=np.float64).ravel() for k in columns]).reshape(len(names), self.n if names else 0))
        nm = (C.c_char_p * max(1, len(names)))(*[k.encode() for k in names])
        check(capi.load().vdn_particles_write(self.h, str(path).encode(), float(time), len(names), nm if names else None,
                                              cols.ctypes.data_as(C.POINTER(C.c_double)) if names else None))

    @staticmethod
    def read(path):
        """(particles, time, columns) of a particle file; the columns are parsed here, positions and states by the library"""
        import numpy as np
        h, t = C.c_void_p(), C.c_double()
        check(capi.load().vdn_particles_read(str(path).encode(), C.byref(h), C.byref(t)))
        P = Particles(_handle=h)
        raw = open(str(path), "rb").read()
        lines = raw.split(b"\n", 4)
        n, ncol = int(lines[2].split()[1]), int(lines[3].split()[1])
        rest = lines[4].split(b"\n", ncol + 1)
        names = [s.decode() for s in rest[:ncol]]
        data = rest[ncol + 1][4 * n + 24 * n:]
        cols = np.frombuffer(data, dtype="<f8", count=ncol * n).reshape(ncol, n)
        return P, t.value, {k: cols[i].copy() for i, k in enumerate(names)}

    def destroy(self):
        if self.h:
            capi.load().vdn_particles_destroy(self.h)
            self.h = None


def particle_lattice(nxyz, prob_hi):
    """the centres of an even nx x ny x nz lattice over the domain (0 .. prob_hi), x fastest: (n, 3); a 2-D domain (two extents) takes nx x ny, z = 0"""
    import numpy as np
    dm = len(prob_hi)
    ax = [(np.arange(int(nxyz[d])) + 0.5) * (float(prob_hi[d]) / int(nxyz[d])) for d in range(dm)]
    if dm == 2:
        ax.append(np.zeros(1))
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
