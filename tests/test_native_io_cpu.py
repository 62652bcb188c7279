"""The text side of the library's file I/O (varden_amd/csrc/fabio.hip) without a GPU: vdn_fabio_ml_multifab_info / _boxes and vdn_checkpoint_info parse the
trees varden_amd/plotfile.py writes and return what plotfile.read_ml_multifab / read_checkfile return; a missing directory and a truncated Header fail with a
message instead of reading past what is there."""
import os

import numpy as np
import pytest

from varden_amd import advance as adv
from varden_amd import plotfile
from varden_amd.capi import VardenError

L0_3D = [((0, 0, 0), (7, 5, 3)), ((8, 0, 0), (11, 5, 3)), ((0, 6, 0), (11, 9, 3))]
L1_3D = [((4, 4, 2), (9, 10, 6)), ((10, 4, 2), (15, 8, 6))]
L0_2D = [((0, 0, 0), (9, 5, 0))]
L1_2D = [((2, 2, 0), (7, 6, 0)), ((8, 2, 0), (13, 9, 0)), ((2, 7, 0), (7, 9, 0))]


def _levels(rng, lists, nodal, nc):
    out = []
    for boxes in lists:
        fabs = [np.asfortranarray(rng.uniform(-2.0, 3.0, size=tuple(hi[d] + nodal[d] - lo[d] + 1 for d in range(3)) + (nc,))) for lo, hi in boxes]
        out.append(dict(boxes=list(boxes), nodal=nodal, fabs=fabs))
    return out


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    root = tmp_path_factory.mktemp("native_io_cpu")
    rng = np.random.default_rng(5)
    t3, t2, n3 = str(root / "t3"), str(root / "t2"), str(root / "n3")
    plotfile.write_ml_multifab(t3, _levels(rng, [L0_3D, L1_3D], (0, 0, 0), 3), [2], dm=3, names=["a", "b", "c"], time=0.375, pd=((0, 0, 0), (11, 9, 3)))
    plotfile.write_ml_multifab(t2, _levels(rng, [L0_2D, L1_2D], (0, 0, 0), 2), [2], dm=2, time=1.0e-3)
    plotfile.write_ml_multifab(n3, _levels(rng, [L0_3D, L1_3D], (1, 1, 1), 1), [2], dm=3)
    return dict(t3=t3, t2=t2, n3=n3, root=root)


@pytest.mark.parametrize("key,lists", [("t3", [L0_3D, L1_3D]), ("t2", [L0_2D, L1_2D]), ("n3", [L0_3D, L1_3D])])
def test_info_and_boxes_return_what_the_python_reader_returns(trees, key, lists):
    r = plotfile.read_ml_multifab(trees[key])
    i = adv.fabio_ml_multifab_info(trees[key])
    assert i["nlevs"] == r["nlevs"] == 2 and i["dm"] == r["dm"] and i["time"] == r["time"] and i["rr"] == r["rr"] == [2]
    assert i["ncomp"] == r["levels"][0]["fabs"][0].shape[3] and i["nodal"] == tuple(r["levels"][0]["nodal"])
    assert i["nboxes"] == [len(L["boxes"]) for L in r["levels"]] == [len(b) for b in lists] and i["nboxes"][0] != i["nboxes"][1]
    for n in range(2):
        assert adv.fabio_ml_multifab_boxes(trees[key], n, i["nboxes"][n]) == r["levels"][n]["boxes"] == lists[n]
    with pytest.raises(VardenError, match="boxes"):
        adv.fabio_ml_multifab_boxes(trees[key], 1, i["nboxes"][1] - 1)          # an array too short for the level
    with pytest.raises(VardenError, match="level 2"):
        adv.fabio_ml_multifab_boxes(trees[key], 2, 8)


def _write_chk(name, trees, time, dt):
    """a checkpoint directory as plotfile.write_checkfile lays it out, around two trees that exist already"""
    os.makedirs(name)
    os.symlink(trees["t3"], os.path.join(name, "State"))
    os.symlink(trees["n3"], os.path.join(name, "Pressure"))
    with open(os.path.join(name, "Header"), "w") as f:
        f.write("&CHKPOINT\n TIME=%s,\n DT=%s,\n NLEVS=%d,\n /\n%12d\n" % (plotfile._es(time).strip(), plotfile._es(dt).strip(), 2, 2))


def test_checkpoint_info_returns_what_read_checkfile_returns(trees):
    name = str(trees["root"] / "chk00007")
    _write_chk(name, trees, 0.1 + 0.2, 1.0 / 3.0e5)
    r = plotfile.read_checkfile(name)
    i = adv.checkpoint_info(name)
    assert i == dict(nlevs=r["nlevs"], time=r["time"], dt=r["dt"], rr=r["rr"])
    assert i["time"] == 0.1 + 0.2 and i["dt"] == 1.0 / 3.0e5 and i["rr"] == [2]


def test_missing_directory_and_truncated_header_fail_with_a_message(trees):
    missing = str(trees["root"] / "nothing_here")
    for call in (lambda: adv.fabio_ml_multifab_info(missing), lambda: adv.fabio_ml_multifab_boxes(missing, 0, 4), lambda: adv.checkpoint_info(missing)):
        with pytest.raises(VardenError, match="nothing_here.*No such file or directory"):
            call()
    # Header cut at every quarter: never a fault, always a message that names the file
    whole = open(os.path.join(trees["t3"], "Header")).read()
    for cut in (0, len(whole) // 4, len(whole) // 2, 3 * len(whole) // 4):
        bad = str(trees["root"] / ("cut%d" % cut))
        os.makedirs(bad)
        os.symlink(os.path.join(trees["t3"], "Level_00"), os.path.join(bad, "Level_00"))
        os.symlink(os.path.join(trees["t3"], "Level_01"), os.path.join(bad, "Level_01"))
        with open(os.path.join(bad, "Header"), "w") as f:
            f.write(whole[:cut])
        with pytest.raises(VardenError, match="cut%d/Header" % cut):
            adv.fabio_ml_multifab_info(bad)
    chk = str(trees["root"] / "chk_cut")
    os.makedirs(chk)
    with open(os.path.join(chk, "Header"), "w") as f:
        f.write("&CHKPOINT\n TIME=1.0E+000,\n D")
    with pytest.raises(VardenError, match="chk_cut/Header"):
        adv.checkpoint_info(chk)
    # Cell_H cut inside the box list
    bad = str(trees["root"] / "cellh")
    os.makedirs(os.path.join(bad, "Level_00"))
    with open(os.path.join(bad, "Header"), "w") as f:
        f.write(whole)
    cell_h = open(os.path.join(trees["t3"], "Level_00", "Cell_H")).read()
    with open(os.path.join(bad, "Level_00", "Cell_H"), "w") as f:
        f.write(cell_h[:cell_h.index("((") + 30])
    with pytest.raises(VardenError, match="cellh/Level_00/Cell_H"):
        adv.fabio_ml_multifab_info(bad)
