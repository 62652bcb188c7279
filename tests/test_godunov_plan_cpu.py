"""the tiling and the launch forms of the fused Godunov marches without a GPU: varden_amd/csrc/godunov_plan.h (which thread of which workgroup owns which
cell in the full-tile, the column and the batched grid, the footprint and the touch rule, the form choosers, the chunk rule) held by
tests/cpp/godunov_plan_check.cpp -- once optimised, once under the address and undefined-behaviour sanitizers -- and the header's chunk lengths against
the Python mirror that tests/test_godunov_phases_gpu.py asserts with on the GPU"""
import os
import subprocess

import pytest

from tests.test_godunov_phases_gpu import klen_cols, klen_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY, NZ = (1, 5, 8, 30, 31, 61, 62, 63, 72, 92, 93, 124, 125, 257), (1, 6, 7, 15, 47), (1, 2, 13, 49, 97)      # the sweep of the check program: face ranges


def build(tmp_path, flags):
    exe = str(tmp_path / "godunov_plan_check")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "varden_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "godunov_plan_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_owners_footprints_forms_and_chunks_of_the_marches(tmp_path, flags):
    r = subprocess.run([build(tmp_path, flags)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr


def test_header_and_python_mirror_give_the_same_chunk_lengths(tmp_path):
    """a drift between the expectation of the GPU test (its copy of the chunk rule) and the header fails here; the mirror takes boxes, one face less per direction"""
    cases = [(nx, ny, nz, ch) for nx in NX for ny in NY for nz in NZ for ch in (0, 1, 2, 3, 5, 7, 13, 16)]
    r = subprocess.run([build(tmp_path, ("-O2",)), "klen"] + [str(v) for c in cases for v in c], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()]
    assert len(got) == len(cases)
    for (nx, ny, nz, ch), (cols, tiles) in zip(cases, got):
        want = klen_cols(nx - 1, ny - 1, nz - 1)
        assert (cols, tiles) == (-1 if want is None else want, klen_tiles(nx - 1, ny - 1, nz - 1, chunks=ch)), (nx, ny, nz, ch, cols, tiles)
