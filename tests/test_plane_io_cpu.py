"""The box rules of the dm = 2 files of a 2-D hierarchy that runs as its z-uniform 3-D copy (varden_amd/plotfile.py: footprints, extrude_boxes; the library restates the
footprint rule in csrc/fabio.hip: plane_map) without a GPU: round trips, chunk and box order, the lists that must be refused, and the path from a dm = 2 checkpoint or grids
file back to the 3-D box lists of a copy."""
import types

import numpy as np
import pytest

from varden_amd import plotfile as pf

# two footprints of different extents, one 4 wide in x
B2 = [((0, 0, 0), (3, 6, 0)), ((4, 0, 0), (10, 6, 0))]
B2_FINE = [((2, 2, 0), (5, 8, 0)), ((6, 2, 0), (15, 12, 0)), ((16, 4, 0), (19, 7, 0))]


@pytest.mark.parametrize("boxes2d,nz,mgs,chunks", [(B2, 8, 4, [(0, 3), (4, 7)]), (B2_FINE, 16, 9, [(0, 7), (8, 15)]),          # uneven: 16 by 9 gives two chunks of 8
                                                  (B2_FINE, 16, 32, [(0, 15)]), (B2, 12, 5, [(0, 3), (4, 7), (8, 11)]),          # nz_level < max_grid_size; 12 by 5: three of 4
                                                  (B2, 8, 8, [(0, 7)]), (B2_FINE[:1], 7, 3, [(k, k) for k in range(7)])])          # a prime nz: planes
def test_extrude_then_footprints_is_the_identity(boxes2d, nz, mgs, chunks):
    b3 = pf.extrude_boxes(boxes2d, nz, mgs)
    # chunks in ascending z, the file's box order inside a chunk
    assert b3 == [((lo[0], lo[1], z0), (hi[0], hi[1], z1)) for z0, z1 in chunks for lo, hi in boxes2d]
    assert all(z1 - z0 + 1 <= mgs for z0, z1 in chunks)
    back, index = pf.footprints(b3)
    assert back == boxes2d
    assert index == [g for _ in chunks for g in range(len(boxes2d))]


def test_footprints_take_the_order_of_the_boxes_that_hold_plane_zero():
    # the boxes of plane k = 0 need not come first, nor in the order of the other chunks
    b3 = [((4, 0, 4), (10, 6, 7)), ((4, 0, 0), (10, 6, 3)), ((0, 0, 4), (3, 6, 7)), ((0, 0, 0), (3, 6, 3))]
    back, index = pf.footprints(b3)
    assert back == [B2[1], B2[0]] and index == [0, 0, 1, 1]


def test_footprints_refuse_overlaps_and_strangers():
    with pytest.raises(ValueError, match="overlap"):
        pf.footprints([((0, 0, 0), (5, 6, 3)), ((5, 0, 0), (10, 6, 3))])
    with pytest.raises(ValueError, match="box 2"):          # a box above plane 0 whose footprint is one cell narrower than the one below it
        pf.footprints([((0, 0, 0), (5, 6, 3)), ((6, 0, 0), (10, 6, 3)), ((0, 0, 4), (4, 6, 7))])
    with pytest.raises(ValueError, match="box 0"):          # nothing holds plane 0
        pf.footprints([((0, 0, 1), (5, 6, 3))])


def test_checkpoint_of_planes_gives_back_the_copys_box_lists(tmp_path):
    """write_ml_multifab(dm=2) of plane arrays -> read_checkfile -> extrude_boxes: a hand-written two-level case"""
    rng = np.random.default_rng(5)
    lists = [B2, B2_FINE]
    name = tmp_path / "chk00003"
    name.mkdir()
    for sub, nodal, nc in (("State", (0, 0, 0), 6), ("Pressure", (1, 1, 0), 1)):
        levels = [dict(boxes=list(b), nodal=nodal, fabs=[rng.standard_normal((hi[0] - lo[0] + 1 + nodal[0], hi[1] - lo[1] + 1 + nodal[1], 1, nc)) for lo, hi in b]) for b in lists]
        pf.write_ml_multifab(str(name / sub), levels, [2], dm=2, pd=((0, 0, 0), (10, 6, 0)), nc=nc)
    (name / "Header").write_text("&CHKPOINT\n TIME=%s,\n DT=%s,\n NLEVS=2,\n /\n%12d\n" % (pf._es(0.25).strip(), pf._es(0.125).strip(), 2))
    chk = pf.read_checkfile(str(name))
    assert chk["dm"] == 2 and chk["nlevs"] == 2 and chk["boxes"] == lists and chk["name"] == str(name) and (chk["time"], chk["dt"]) == (0.25, 0.125)
    b3 = [pf.extrude_boxes(b, 8 << n, 9) for n, b in enumerate(chk["boxes"])]
    assert b3[0] == [((0, 0, 0), (3, 6, 7)), ((4, 0, 0), (10, 6, 7))]
    assert b3[1] == [((2, 2, 0), (5, 8, 7)), ((6, 2, 0), (15, 12, 7)), ((16, 4, 0), (19, 7, 7)), ((2, 2, 8), (5, 8, 15)), ((6, 2, 8), (15, 12, 15)), ((16, 4, 8), (19, 7, 15))]
    assert [pf.footprints(b)[0] for b in b3] == lists


def test_grids_file_of_a_copy_holds_the_footprints(tmp_path):
    b3 = [pf.extrude_boxes([((0, 0, 0), (15, 15, 0)), ((16, 0, 0), (31, 15, 0)), ((0, 16, 0), (31, 31, 0))], 16, 16), pf.extrude_boxes(B2_FINE, 32, 16)]
    sim = types.SimpleNamespace(boxes=b3, local=[list(range(len(b))) for b in b3], ncs=(32, 32, 16), dm=3, extrude2d=16, rank=0)
    path = str(tmp_path / "grids")
    pf.write_grids(path, sim, 0)
    domains, levels = pf.read_grids(path)
    assert domains == [((0, 0, 0), (31, 31, 0)), ((0, 0, 0), (63, 63, 0))]
    assert levels == [pf.footprints(b)[0] for b in b3] and levels[1] == B2_FINE
    # files_copy: the 3-D boxes, as before
    sim.files_copy = True
    pf.write_grids(path + "3", sim, 0)
    assert pf.read_grids(path + "3")[1] == b3
