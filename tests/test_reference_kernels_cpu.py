"""The CPU oracle's pointwise kernels against the reference's OWN routines, bit for bit.

oracle/ref/ compiles the reference's array-level routines, unmodified, into oracle/_ref/libvref.so (stand-ins for the five declaration-only modules they
`use`; nothing of the reference is kept in this repository).  Every case of tests/refcases.py runs through the oracle and through that library on the same
input bytes and is compared with tests.util.assert_bits: the bar is 0 ulp (IEEE double on both sides, no contraction, only + - * / abs min max sign sqrt).

Compared region, per routine (the region the reference routine defines for its arguments):

    routine            oracle function(s)                     compared
    -----------------  -------------------------------------  ---------------------------------------------------------------------------------
    slope              vo_slope                               every cell of [lo-1, hi+1] in every direction = the whole slope array, u and s
    velpred            vo_velpred / vo2_velpred               all valid faces of umac, vmac (, wmac)
    mkflux             vo_mkflux / vo2_mkflux                 all valid faces of sedge and of flux, every component
    update             vo_update / vo2_update                 all valid cells of snew
    mkvelforce         vo_mkvelforce / vo2_mkvelforce         the whole array: valid cells + the six (four) face halos; edges and corners untouched
    mkscalforce        vo_mkscalforce / vo2_mkscalforce       the whole array, as mkvelforce
    estdt              vo_estdt / vo2_estdt                   dt
    physbc             vo_physbc                              the whole array, all ghost layers, u and s
    make_at_halftime   vo_make_at_halftime                    the whole one-ghost-layer array
    (the forces and make_at_halftime are compared a second time after the ghost fill their drivers apply to the result: what the C-ABI calls return)
    plot               vo_makevort, vo_makemagvel             all valid cells
    tag_boxes          vo_tag_boxes                           the tag of every valid cell, and whether bl_error was called

The SHA-256 of the reference's output of every case is kept in tests/golden/reference_kernels.json, so that a checkout without the reference tree (and the GPU
test, tests/test_reference_kernels_gpu.py) is still held to the reference's results.  With the library present a stale file fails here;
`python -m tests.test_reference_kernels_cpu --record` rewrites it.
"""
import json
import os
import sys

import pytest

from oracle import voracle as vo
from tests import refcases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_kernels.json")
needs_ref = pytest.mark.skipif(vo.ref_lib() is None, reason="oracle/_ref/libvref.so is not there: build it with `make -C oracle/ref VARDEN_REF=<reference tree>` (needs flang)")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def assert_bits(a, b, what):
    from tests.util import assert_bits as ab
    ab(a, b, what)


def test_case_list_covers_the_suites_boundary_sets():
    """the boundary sets of the existing kernel tests, all of them, plus the two-sided inlets and the box-interior box; every routine in 2-D and 3-D on each"""
    from tests.util import BC_SETS
    from tests.test_dim2_gpu import BC2
    assert all(rc.BC3[k] == v for k, v in BC_SETS.items()) and all(rc.BC2[k] == v for k, v in BC2.items())
    have = {(s["routine"], s["dm"], s.get("bc")) for s in rc.CASES.values()}
    for dm, sets in ((2, rc.BC2), (3, rc.BC3)):
        for bc in sets:
            for r in ("slope", "velpred", "mkflux", "physbc", "plot"):
                assert (r, dm, bc) in have, (r, dm, bc)
        for r in ("update", "mkvelforce", "mkscalforce", "estdt", "make_at_halftime", "tag_boxes"):
            assert (r, dm, None) in have, (r, dm)
    print("%d cases" % len(rc.CASES))
    assert sorted(k.split("#")[0] for k in golden() if "#" not in k) == sorted(rc.CASES) and all(k.split("#")[0] in rc.CASES for k in golden()), "tests/golden/reference_kernels.json does not list exactly the cases of tests/refcases.py: record it again"


@needs_ref
@pytest.mark.parametrize("cid", list(rc.CASES))
def test_oracle_matches_reference(cid):
    spec = rc.CASES[cid]
    ref, ora = rc.run(spec, "ref"), rc.run(spec, "oracle")
    g = golden()
    assert all(g.get(k) == v for k, v in rc.entries(cid, ref).items()), "the recorded hash of %s is stale: python -m tests.test_reference_kernels_cpu --record" % cid
    for (name, a), (_, b) in zip(ref, ora):
        assert_bits(b, a, "%s: %s (oracle vs reference)" % (cid, name))


@pytest.mark.parametrize("cid", list(rc.CASES))
def test_oracle_matches_recorded_reference(cid):
    g = golden()
    assert all(g.get(k) == v for k, v in rc.entries(cid, rc.run(rc.CASES[cid], "oracle")).items()), "%s: the oracle's output is not the reference's recorded output" % cid


def record():
    """rewrite tests/golden/reference_kernels.json from the reference library (needs oracle/_ref/libvref.so)"""
    assert vo.ref_lib() is not None, "oracle/_ref/libvref.so is not there"
    out = {}
    for cid, spec in rc.CASES.items():
        out.update(rc.entries(cid, rc.run(spec, "ref")))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d cases" % len(out))


if __name__ == "__main__":
    if "--record" in sys.argv:
        record()
