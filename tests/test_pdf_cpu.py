"""PDFs and conditional sums by value on the device (vdn_pdf, vdn_pdf2, varden_amd/csrc/pdf.hip): what can be held without a GPU -- the struct and the four entries are
declared, typed and exported, capi.PdfLayout mirrors the C struct member for member, vdn_pdf_layout (a pure host function) gives the offsets of the header's table,
the namelist keys exist, the file text has its header and widths, the command line has its options, the slot rule
(csrc/pdf_bin.h) holds under the sanitizers, and the calls refuse to run uninitialised."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = ["nrow", "volume", "q", "s", "u", "ru", "ke"]
ENTRIES = {"vdn_pdf_layout": 3, "vdn_pdf_layout_sizeof": 0, "vdn_pdf": 14, "vdn_pdf2": 19}
KEYS = dict(pdf_int=0, pdf_field="scalar", pdf_comp=1, pdf_lo=0.0, pdf_hi=0.0, pdf_nbins=64, pdf_base_name="pdf")


def _header():
    txt = open(os.path.join(ROOT, "include", "varden_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_struct_and_signatures():
    from varden_amd import advance as adv
    from varden_amd import capi
    h = _header()
    body = re.search(r"typedef\s+struct\s+vdn_pdf_layout_t\s*\{([^}]*)\}\s*vdn_pdf_layout_t\s*;", h).group(1)
    cm = [m.strip() for m in re.fullmatch(r"\s*int\s+([\w\s,]+);\s*", body).group(1).split(",")]
    assert cm == MEMBERS == [f[0] for f in capi.PdfLayout._fields_]
    assert all(f[1] is C.c_int for f in capi.PdfLayout._fields_) and C.sizeof(capi.PdfLayout) == 4 * len(MEMBERS)
    for name, nargs in ENTRIES.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, h)
        assert decl, name
        assert name in capi.SIGNATURES and len(capi.SIGNATURES[name][1]) == nargs, name
        assert (0 if decl.group(1).strip() == "void" else decl.group(1).count(",") + 1) == nargs, (name, decl.group(1))
    # the codes and the limits: the header and the Python host agree
    for name, code in adv.PDF_FIELDS.items():
        assert re.search(r"\bVDN_PDF_%s\s*=\s*%d\b" % (name.upper(), code), h), name
    assert re.search(r"#define\s+VDN_PDF_MAX_BINS\s+256\b", h) and re.search(r"#define\s+VDN_PDF2_MAX_BINS\s+64\b", h)
    assert (adv.PDF_MAX_BINS, adv.PDF2_MAX_BINS) == (256, 64)
    for lib in ("libvarden_amd.so", "libvarden_amd_testing.so"):
        L = C.CDLL(os.path.join(ROOT, "varden_amd", "csrc", lib), mode=os.RTLD_LOCAL)
        L.vdn_pdf_layout_sizeof.restype = C.c_size_t
        assert L.vdn_pdf_layout_sizeof() == C.sizeof(capi.PdfLayout), lib
        for name in ENTRIES:
            assert hasattr(L, name), (lib, name)
    # the slot rule is a dependency of every object
    mk = open(os.path.join(ROOT, "varden_amd", "csrc", "Makefile")).read()
    assert re.search(r"(?m)^SRC\s*:=.*\bpdf\.hip\b", mk) and len(re.findall(r"(?m)^%.*\.o:.*\bpdf_bin\.h\b", mk)) == 2


@pytest.mark.parametrize("dm,nscal", [(3, 2), (3, 11), (2, 2)])
def test_layout_offsets(dm, nscal):
    """nrow and the offsets against the table of include/varden_amd.h; the row groups tile 0 .. nrow-1 without gap or overlap"""
    from varden_amd import advance as adv
    from varden_amd import capi
    lib = capi.load()
    lay = capi.PdfLayout()
    assert lib.vdn_pdf_layout(dm, nscal, C.byref(lay)) == 0
    count = dict(volume=1, q=1, s=nscal, u=dm, ru=dm, ke=1)
    assert list(count) == MEMBERS[1:] == list(adv.PDF_GROUPS)
    rows = []
    for g in MEMBERS[1:]:
        assert getattr(lay, g) == len(rows), (g, getattr(lay, g), len(rows))
        rows += [g] * count[g]
    assert lay.nrow == len(rows) == nscal + 2 * dm + 3
    assert lay.nrow == {(3, 2): 11, (3, 11): 20, (2, 2): 9}[dm, nscal]
    d = adv.pdf_layout(dm, nscal)
    assert d["nrow"] == lay.nrow and all(d[g] == (getattr(lay, g), count[g]) for g in count)
    cols = adv.pdf_columns(nscal, dm)
    assert len(cols) == lay.nrow and len(set(cols)) == lay.nrow
    assert cols[lay.volume] == "volume" and cols[lay.q] == "q" and cols[lay.s] == "s1" and cols[lay.u] == "u1" and cols[lay.ru] == "ru1" and cols[lay.ke] == "ke"
    # refused: a dimension or a scalar count the library does not run, a NULL struct
    for bad in ((1, 2), (4, 2), (3, 0), (3, 12)):
        assert lib.vdn_pdf_layout(bad[0], bad[1], C.byref(lay)) != 0 and b"vdn_pdf_layout" in lib.vdn_last_error()
    assert lib.vdn_pdf_layout(3, 2, None) != 0


def test_namelist_keys():
    from varden_amd import inputs
    assert {k: inputs.DEFAULTS[k] for k in KEYS} == KEYS
    nl = inputs.parse_namelist("&PROBIN\n pdf_int = 5\n pdf_field = 'vorticity'\n pdf_comp = 2\n pdf_lo = -1.5d0\n pdf_hi = 2.5\n pdf_nbins = 7\n pdf_base_name = 'out/p'\n/\n")
    assert nl == dict(pdf_int=5, pdf_field="vorticity", pdf_comp=2, pdf_lo=-1.5, pdf_hi=2.5, pdf_nbins=7, pdf_base_name="out/p")
    text = open(os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_3d_n32_pdf")).read()
    nl = dict(inputs.DEFAULTS, **inputs.parse_namelist(text))
    assert nl["pdf_int"] == 2 and nl["pdf_field"] == "scalar" and nl["pdf_comp"] == 1 and (nl["pdf_lo"], nl["pdf_hi"], nl["pdf_nbins"]) == (0.5, 10.5, 40)
    assert nl["diag_int"] == 1 and nl["max_levs"] == 2 and nl["n_cellx"] == 32 and nl["prof_int"] == 0
    assert os.path.exists(os.path.join(ROOT, "tests", "golden", "inputs", "README.inputs_bubble_3d_n32_pdf"))


def test_a_run_without_a_range_is_refused():
    """pdf_int > 0 and !(pdf_lo < pdf_hi): a message before anything is built (no GPU is touched); an unknown field too; with pdf_int = 0 the keys are not looked at"""
    from varden_amd import inputs
    base = dict(inputs.DEFAULTS)
    assert inputs.pdf_keys(base) == (0, "scalar", 1, 0.0, 0.0, 64)
    assert inputs.pdf_keys(dict(base, pdf_field="nonsense"))[0] == 0
    for bad in (dict(pdf_int=1), dict(pdf_int=1, pdf_lo=1.0, pdf_hi=1.0), dict(pdf_int=3, pdf_lo=2.0, pdf_hi=1.0), dict(pdf_int=1, pdf_lo=float("nan"), pdf_hi=1.0)):
        with pytest.raises(ValueError, match="pdf_lo"):
            inputs.pdf_keys(dict(base, **bad))
    with pytest.raises(ValueError, match="pdf_field"):
        inputs.pdf_keys(dict(base, pdf_int=1, pdf_hi=1.0, pdf_field="density"))
    assert inputs.pdf_keys(dict(base, pdf_lo=3.0), pdf_int=2, pdf_field="magvel", pdf_comp=2, pdf_range=(0.0, 2.0), pdf_nbins=8) == (2, "magvel", 2, 0.0, 2.0, 8)
    with pytest.raises(ValueError, match="pdf_lo"):
        inputs.run("&PROBIN\n dim_in = 3\n pdf_int = 1\n/\n", report=None)


def test_pdf_text():
    """the file: the tag and nine more header lines, the column names, one line per slot; the names line and the data lines have the same width"""
    import numpy as np
    from varden_amd import advance as adv
    from varden_amd import inputs
    nb = 4
    cells = np.array([[1, 2, 3, 4, 5, 6], [10, 20, 30, 40, 50, 60]], dtype=np.int64)
    P = adv.Pdf("scalar", 0, 0.5, 2.5, nb, 3, 2, np.arange(1, 11 * (nb + 2) + 1, dtype=np.float64).reshape(11, nb + 2), cells, 3)
    lines = inputs.pdf_text(P, 3, 0.5).split("\n")
    assert lines[:10] == ["# VDN_PDF 1", "# dm 3", "# field scalar", "# comp 1", "# nbins 4", "# lo   5.00000000000000000E-001", "# hi   2.50000000000000000E+000", "# step 3",
                          "# time   5.00000000000000000E-001", "# nan_cells 3"] and lines[-1] == ""
    assert lines[10].split() == ["#", "centre", "cells"] + adv.pdf_columns(2, 3) and len(lines) == 11 + nb + 2 + 1
    assert all(len(ln) == 27 + 16 + 27 * 11 for ln in lines[10:-1])
    # slot 0 is "below": its centre is lo - w / 2; the cells column is the sum over the levels
    assert lines[11].startswith("   2.50000000000000000E-001              11   1.00000000000000000E+000   7.00000000000000000E+000")
    assert lines[13].startswith("   1.25000000000000000E+000              33   3.00000000000000000E+000")
    assert np.array_equal(P.edges, [0.5, 1.0, 1.5, 2.0, 2.5]) and np.array_equal(P.centres, [0.25, 0.75, 1.25, 1.75, 2.25, 2.75])
    assert P["volume"].shape == (nb + 2,) and P["s"].shape == (2, nb + 2) and P["ru"].shape == (3, nb + 2) and P["ke"].shape == (nb + 2,) and P.mean("s").shape == (2, nb + 2)
    assert np.array_equal(P.mean("ru"), P.rows[7:10] / P.rows[0]) and set(P.keys()) == set(("edges", "centres", "cells", "nan_cells") + adv.PDF_GROUPS)
    d = P.density()
    assert d.shape == (nb,) and abs((d * P.w).sum() - 1.0) < 1e-15 and np.array_equal(d, P.rows[0, 1:-1] / (P.rows[0, 1:-1].sum() * 0.5))
    with pytest.raises(KeyError):
        P.mean("volume")
    # a field given by its code names itself in the file
    assert inputs.pdf_text(adv.Pdf(3, 0, 0.0, 1.0, nb, 3, 2, P.rows, cells, 0), 0, 0.0).split("\n")[2] == "# field vorticity"


def test_command_line_options():
    r = subprocess.run([sys.executable, "-m", "varden_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for opt in ("--pdf-int", "--pdf-field", "--pdf-range", "--pdf-comp", "--pdf-nbins"):
        assert opt in r.stdout, (opt, r.stdout)


def test_slot_rule(tmp_path):
    exe = str(tmp_path / "pdf_bin_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "varden_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "pdf_bin_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr


def test_numpy_restatement_of_the_slot_rule():
    """tests/_pdf_worker.slots, the rule the GPU tests hold the kernel against, on the edge values of tests/cpp/pdf_bin_check.cpp"""
    import numpy as np
    from tests._pdf_worker import slots
    inf = np.inf
    q = np.array([0.0, -0.0, 1.0, np.nextafter(1.0, -inf), np.nextafter(0.0, -inf), inf, -inf, np.nan, 0.5, 0.125, np.nextafter(0.125, -inf)])
    assert list(slots(q, 0.0, 1.0, 8)) == [1, 1, 9, 8, 0, 9, 0, -1, 5, 2, 1]
    assert list(slots(q, 0.0, 1.0, 1)) == [1, 1, 2, 1, 0, 2, 0, -1, 1, 1, 1]
    assert list(slots(np.array([np.nextafter(0.7, -inf), 0.7, 0.0]), 0.0, 0.7, 7)) == [7, 8, 1]
    assert list(slots(np.array([8.0e307, -8.0e307, 7.9e307]), -8.0e307, 8.0e307, 3)) == [4, 1, 3]


def test_refuses_without_a_gpu():
    """before vdn_init (or where it failed: no GPU) the calls return non-zero with the library's message"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    from varden_amd import capi
    lib = capi.load()
    out, cells, vol, nan = (C.c_double * 44)(), (C.c_longlong * 16)(), (C.c_double * 9)(), C.c_longlong(0)
    dx = (C.c_double * 3)(1.0, 1.0, 1.0)
    rc = lib.vdn_pdf(1, None, None, None, dx, None, 0, 0, 2, 0.0, 1.0, out, cells, C.byref(nan))
    assert rc != 0 and b"vdn_init" in lib.vdn_last_error() and lib.vdn_last_error().startswith(b"vdn_pdf:")
    with pytest.raises(capi.VardenError, match="vdn_pdf"):
        capi.check(rc)
    rc = lib.vdn_pdf2(1, None, None, None, dx, None, 0, 0, 1, 0.0, 1.0, 1, 0, 1, 0.0, 1.0, cells, vol, C.byref(nan))
    assert rc != 0 and b"vdn_init" in lib.vdn_last_error() and lib.vdn_last_error().startswith(b"vdn_pdf2:")
