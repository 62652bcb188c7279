"""The fused mkflux + update march in half workgroups (kk_mk_F_mh: 64 x 4 threads, two workgroups per compute unit, every tile in row segments of 16 or 32
lanes) changes no value: SHA-256 over the valid cells of unew and snew after one advance_timestep, the half form against the 512-thread marches
(VDN_GOD_NARROW=2) and against the face-centred one-thread-per-cell kernels, for both segment widths, chunk lengths 1, 2, 3 (no steady plane), 4 (one)
and >= 6, boxes of one tile, of a second tile with one cell, with remainders in x and y, under walls, a mix without an inlet, the four-rule mix (its
inlet keeps the division, so today's kernel) and full periodicity (no face with a rule: today's kernel), use_minion 0 and 1.  One step carries the three
compiled-in families: density (conservative), tracer, and the velocity components with the forcing formed in place.  VDN_GOD_NARROW=16 / 32 chooses the
segment width and lets boxes of a few thousand cells reach the form (the default takes it from 128 faces on); the library tells which family its
last mkflux march came from (vdn_last_mkflux_form, testing build).  The switches are read at a process's first launch, hence the child processes: one child runs every case of its variant."""
import textwrap

import pytest

from tests.children import ROOT, run_variant

pytestmark = pytest.mark.gpu

BCS = {"walls": [[15, 15]] * 3, "outmix": [[12, 14], [14, 15], [15, 12]], "mix": [[11, 12], [14, 15], [15, 12]], "periodic": [[-1, -1]] * 3}
HALF_BCS = ("walls", "outmix")                     # the boundary sets whose launches take the half form
# boxes (the face range of the march is one wider per direction): (13, 13, 4): a range of 14 x 14 x 5, exactly one tile at W = 16; (14, 14, 5): a range of
# 15 x 15 x 6, two tiles per direction with one cell in the second; (15, 15, 6); remainders in x and y; (30, 16, 9)
SHAPES = ((13, 13, 4), (14, 14, 5), (15, 15, 6), (33, 29, 12), (30, 16, 9))
# VDN_FUSED_KCHUNKS -> chunk length on the 13 face planes of (33, 29, 12)
CHUNKS = {13: 1, 7: 2, 5: 3, 4: 4, 2: 7}

CODE = textwrap.dedent("""
    import sys, hashlib
    sys.path.insert(0, %r)
    import numpy as np
    from varden_amd import driver, capi
    from tests.util import params_for                   # (the inlet of "mix" needs its inflow values)
    BCS, SHAPES = %r, %r
    form_of = capi.load().vdn_last_mkflux_form
    for n in SHAPES:
        for bc in sys.argv[1].split(","):
            for minion in (0, 1):
                rng = np.random.default_rng(7)
                u0 = 0.5 * rng.standard_normal((n[0] + 6, n[1] + 6, n[2] + 6, 3))
                s0 = 1.0 + 0.25 * rng.random((n[0] + 6, n[1] + 6, n[2] + 6, 2))
                # every spacing 1 / 64: the update-carrying marches with cons / use_minion / the forcing mode compiled in
                G = driver.Varden(n, BCS[bc], params_for(BCS[bc], use_minion=minion), prob_hi=tuple(x / 64.0 for x in n), init_iter=0, do_initial_projection=0,
                                  init_shrink=0.1, u0=u0, s0=s0)
                G.step()
                form = form_of()                                # the last mkflux of a step is the velocity's
                h = hashlib.sha256()
                for m in (G.unew[0], G.snew[0]):
                    a = G.gather_valid(m)
                    assert np.isfinite(a).all()
                    h.update(np.ascontiguousarray(a).tobytes())
                print("HASH", "%%dx%%dx%%d" %% n, bc, minion, form, h.hexdigest())
                G.close()
""" % (ROOT, BCS, SHAPES))

PLAIN = {"VDN_GODUNOV_PLAIN": "1", "VDN_SLOPES_MARCH": "0"}
FULL = {"VDN_GOD_NARROW": "2"}                     # the 512-thread marches, remainder column in narrow segments: what ran before the half form


def half(W, **more):
    return dict({"VDN_GOD_NARROW": str(W)}, **more)


_cache = {}


def hashes(bcs, switches):
    """{(shape, bc, minion): (family of the last mkflux march, hash)} of one child under `switches`; a variant runs once per session"""
    key = (bcs, tuple(sorted(switches.items())))
    if key not in _cache:
        r = run_variant(("-c", CODE, ",".join(bcs)), switches, 300)
        _cache[key] = {(t[1], t[2], int(t[3])): (int(t[4]), t[5]) for t in r["HASH"]}
        assert len(_cache[key]) == len(SHAPES) * len(bcs) * 2, r
    return _cache[key]


@pytest.mark.parametrize("W", [16, 32])
def test_half_workgroups_equal_the_full_marches_and_face_centred(gpu, W):
    bcs = tuple(BCS)
    ref, full = hashes(bcs, PLAIN), hashes(bcs, FULL)
    got = hashes(bcs, half(W))
    for case in ref:
        assert ref[case][0] == -1 and full[case][0] in (0, 1), (case, ref[case], full[case])
        # walls / outmix: the half form; the inlet of mix and the missing faces of periodic keep today's kernel
        assert got[case][0] == (W if case[1] in HALF_BCS else full[case][0]), (W, case, got[case], full[case])
        assert got[case][1] == full[case][1] == ref[case][1], (W, case, got[case], full[case], ref[case])


@pytest.mark.parametrize("chunks", list(CHUNKS))
@pytest.mark.parametrize("W", [16, 32])
def test_half_workgroups_in_chunks_of_every_phase_count(gpu, W, chunks):
    nz = SHAPES[3][2] + 1
    assert (nz + chunks - 1) // chunks == CHUNKS[chunks]
    ref = hashes(tuple(BCS), PLAIN)
    got = hashes(HALF_BCS, half(W, VDN_FUSED_KCHUNKS=str(chunks)))
    for case in got:
        assert got[case][0] == W and got[case][1] == ref[case][1], (W, chunks, case, got[case], ref[case])


STEP_CODE = textwrap.dedent("""
    import sys
    sys.path.insert(0, %r)
    import numpy as np
    from oracle import voracle as vo
    from varden_amd import driver, capi
    from tests.util import WALLS, params_for
    n = (40, 32, 24)
    hi = tuple(x / 64.0 for x in n)
    O = vo.Sim(n, WALLS, params_for(WALLS, cflfac=0.9), prob_type=1, init_shrink=0.1, init_iter=1, prob_hi=hi)
    ou, os_ = vo.Fab((0, 0, 0), tuple(x - 1 for x in n), 3, 3), vo.Fab((0, 0, 0), tuple(x - 1 for x in n), 3, 2)
    vo.lib().vo_initdata(ou.ref, os_.ref, O.dx, 1)
    G = driver.Varden(n, WALLS, params_for(WALLS, cflfac=0.9), prob_type=1, init_shrink=0.1, init_iter=1, prob_hi=hi, u0=ou.a, s0=os_.a)
    assert G.dt == O.dt
    O.step(); G.step()
    assert G.dt == O.dt
    g = 3
    out = [capi.load().vdn_last_mkflux_form()]
    for gm, om in ((G.unew[0], O.unew), (G.snew[0], O.snew)):
        a, b = gm.to_numpy()[g:-g, g:-g, g:-g], om.valid()
        out += [float(np.abs(a - b).max()), max(float(np.abs(b).max()), 1e-300)]
    a, b = G.p[0].to_numpy()[1:-1, 1:-1, 1:-1], O.p.valid()
    out += [float(np.abs((a - a.mean()) - (b - b.mean())).max()), max(float(np.abs(b - b.mean()).max()), 1e-300)]
    print("RESULT", *out)
    G.close()
""" % ROOT)


def test_a_step_in_half_workgroups_against_the_oracle(gpu):
    """one advance_timestep after the start-up sequence on a 40 x 32 x 24 box, every mkflux march in half workgroups, to the tolerances of
    tests/test_advance_gpu.py: u, rho and the tracer to 1e-9 of the largest value, the pressure (mean removed) to 1e-6"""
    t = run_variant(("-c", STEP_CODE), half(16), 300)["RESULT"][0]
    form, (eu, su, es, ss, ep, sp) = int(t[1]), (float(v) for v in t[2:8])
    print("form %d  u %.3e / %.3e  s %.3e / %.3e  p %.3e / %.3e" % (form, eu, su, es, ss, ep, sp))
    assert form == 16
    assert eu <= 1e-9 * su and es <= 1e-9 * ss and ep <= 1e-6 * sp, t
