// fabio.hip -- plot files and checkpoints written and read inside the library: fabio_ml_multifab_write_d / _read_d as the reference calls them
// (src/varden.f90:568-573, src/checkpoint.f90:45-48, 116-122) and checkpoint_write / checkpoint_read (src/checkpoint.f90:14-145).
//
// The file format is defined by varden_amd/plotfile.py (write_ml_multifab, _write_level, write_checkfile): every file written here is byte for byte what
// that module writes for the same data, and the tests hold the two against each other.  One rank only.
//
// Payload of one level = one linear index space: for each box (ascending global index), for each component, z, y, x (x fastest) over the box's valid
// points (the upper nodal point included, ghost cells left out).  The host cuts it into SEGMENTS (box, component, payload offset, length) once per call; a
// launch of kk_fab_pack moves one range [a, b) of the space -- which may begin or end inside a fab, a component or a row -- into the staging buffer, one
// workgroup per piece of FAB_PIECE values of one segment, consecutive lanes writing consecutive staging entries.  The same pass reduces the minimum and the
// maximum of every (box, component) for Cell_H: wave shuffles, LDS, then one atomic pair per workgroup on the ORDER-PRESERVING 64-bit image of the double
// (key_of, vdn_dev.h: sign bit flipped for non-negative values, all bits for negative ones), so the values are exact -- not the shifted sums of vdn_multifab_min_max.  With that
// image -0 sorts below +0: a field holding both reports min = -0, max = +0.  kk_fab_unpack is the inverse over the same table; it writes valid points only.
// dm = 2: the fabs keep the 3-D layout with one valid z-plane (k = 0), which the segment's origin and extents address like any other box.
//
// A 2-D problem that runs as its z-uniform 3-D copy (vdn_set_extruded_2d) writes and reads the 2-D run's files: write_plane packs plane k = 0 of the boxes that hold it with the
// same kk_fab_pack (a plane is a segment of len = nx ny) and, if asked, measures how z-uniform the copy is (kk_plane_defect); read_plane stores the file's plane to every valid
// plane of every box of that footprint (kk_fab_unpack_extrude).  The footprint rule is plane_map's; varden_amd/plotfile.py (footprints, extrude_boxes) states it for the hosts.
#include "vdn_dev.h"
#include <sys/stat.h>
#include <cerrno>
#include <cstdlib>
#include <cctype>
#include <string>

void fabio_release();

namespace {
constexpr int FAB_PIECE = 4096;          // values one workgroup moves: 32 KB read, 32 KB written
constexpr int FAB_THREADS = 256;
constexpr long FAB_STAGING_DEFAULT = 256l << 20;
const char *const FAB_DESC = "FAB ((8, (64 11 52 0 1 12 0 1023)),(8, (8 7 6 5 4 3 2 1)))";

// one (box, component): p = its first valid point; rows of nx contiguous doubles, sy / sz = the fab's row and plane strides
struct FabSeg { double *p; long off, piece0, sy, sz; int len, nx, ny, pad; };

// the piece of the linear space workgroup blockIdx.x takes, clipped to [a, b): segment *S, elements [e0, e1)
DEVI bool fab_piece(const FabSeg *segs, int nseg, long P0, long a, long b, FabSeg &S, int &s, long &e0, long &e1) {
  const long gp = P0 + (long)blockIdx.x;
  int lo = 0, hi = nseg - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (as_constant(segs + mid).piece0 <= gp) lo = mid; else hi = mid - 1; }
  s = lo; S = as_constant(segs + lo);
  const long q0 = (gp - S.piece0) * FAB_PIECE;
  e0 = S.off + q0; e1 = S.off + (q0 + FAB_PIECE < (long)S.len ? q0 + FAB_PIECE : (long)S.len);
  if (e0 < a) e0 = a;
  if (e1 > b) e1 = b;
  return e0 < e1;
}
DEVI long fab_src_index(const FabSeg &S, unsigned q) {
  const unsigned r = q / (unsigned)S.nx, i = q - r * (unsigned)S.nx, k = r / (unsigned)S.ny, j = r - k * (unsigned)S.ny;
  return (long)i + S.sy * (long)j + S.sz * (long)k;
}

__global__ void __launch_bounds__(FAB_THREADS) kk_fab_pack(const FabSeg *segs, int nseg, long P0, long a, long b, double *__restrict__ stage,
                                                           unsigned long long *mmin, unsigned long long *mmax) {
  FabSeg S; int s; long e0, e1;
  if (!fab_piece(segs, nseg, P0, a, b, S, s, e0, e1)) return;      // (uniform over the workgroup)
  unsigned long long mn = ~0ull, mx = 0ull;
  for (long e = e0 + threadIdx.x; e < e1; e += FAB_THREADS) {
    const double v = S.p[fab_src_index(S, (unsigned)(e - S.off))];
    stage[e - a] = v;
    const unsigned long long key = key_of(v);
    mn = key < mn ? key : mn; mx = key > mx ? key : mx;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long n2 = __shfl_down(mn, o, 64), x2 = __shfl_down(mx, o, 64);
    mn = n2 < mn ? n2 : mn; mx = x2 > mx ? x2 : mx;
  }
  __shared__ unsigned long long sm[2][FAB_THREADS / 64];
  if ((threadIdx.x & 63) == 0) { sm[0][threadIdx.x >> 6] = mn; sm[1][threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < FAB_THREADS / 64; w++) { mn = sm[0][w] < mn ? sm[0][w] : mn; mx = sm[1][w] > mx ? sm[1][w] : mx; }
    atomicMin(mmin + s, mn); atomicMax(mmax + s, mx);
  }
}
__global__ void __launch_bounds__(FAB_THREADS) kk_fab_unpack(const FabSeg *segs, int nseg, long P0, long a, long b, const double *__restrict__ stage) {
  FabSeg S; int s; long e0, e1;
  if (!fab_piece(segs, nseg, P0, a, b, S, s, e0, e1)) return;
  for (long e = e0 + threadIdx.x; e < e1; e += FAB_THREADS) S.p[fab_src_index(S, (unsigned)(e - S.off))] = stage[e - a];
}

// the inverse of a PLANE segment for a z-uniform copy: the same pieces of the staged linear space as kk_fab_unpack; every staged value is read once and stored to all
// valid planes of every destination box of that footprint (dsts[dst0[s] .. dst0[s + 1]) for segment s).  Consecutive lanes store consecutive x of one row
struct PlaneDst { double *p; long sy, sz; int nz, pad; };          // p = the first valid point of (box, component); nz = valid planes (the upper node plane included)
__global__ void __launch_bounds__(FAB_THREADS) kk_fab_unpack_extrude(const FabSeg *segs, int nseg, long P0, long a, long b, const double *__restrict__ stage,
                                                                     const int *__restrict__ dst0, const PlaneDst *__restrict__ dsts) {
  FabSeg S; int s; long e0, e1;
  if (!fab_piece(segs, nseg, P0, a, b, S, s, e0, e1)) return;
  const int d0 = as_constant(dst0 + s), d1 = as_constant(dst0 + s + 1);
  for (long e = e0 + threadIdx.x; e < e1; e += FAB_THREADS) {
    const double v = stage[e - a];
    const unsigned q = (unsigned)(e - S.off), j = q / (unsigned)S.nx, i = q - j * (unsigned)S.nx;
    for (int d = d0; d < d1; d++) {
      const PlaneDst D = as_constant(dsts + d);
      double *c = D.p + (long)i + D.sy * (long)j;
      for (int k = 0; k < D.nz; k++) c[D.sz * (long)k] = v;
    }
  }
}
// z-uniformity of a copy, measured against the plane that goes to the file: one (box, component) per segment, DEF_PIECE points of the (x, y) footprint per workgroup; a
// thread keeps the written plane's value of its point in a register and marches over k.  kind 0: max |f(i,j,k) - ref(i,j)| -> out[0]; kind 1 (ref = NULL: a component
// that must vanish): max |f| -> out[1].  Maxima of the order-preserving keys: wave shuffles, LDS, one atomicMax per workgroup.  A NaN comes out as a NaN
constexpr int DEF_PIECE = 1024;
struct DefSeg { const double *p, *ref; long sy, sz, rsy, piece0; int nx, ny, nz, kind; };
__global__ void __launch_bounds__(FAB_THREADS) kk_plane_defect(const DefSeg *segs, int nseg, unsigned long long *out) {
  const long gp = (long)blockIdx.x;
  int lo = 0, hi = nseg - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (as_constant(segs + mid).piece0 <= gp) lo = mid; else hi = mid - 1; }
  const DefSeg S = as_constant(segs + lo);
  const unsigned npts = (unsigned)S.nx * (unsigned)S.ny, q0 = (unsigned)(gp - S.piece0) * DEF_PIECE, q1 = q0 + DEF_PIECE < npts ? q0 + DEF_PIECE : npts;
  unsigned long long mx = key_of(0.0);
  for (unsigned q = q0 + threadIdx.x; q < q1; q += FAB_THREADS) {
    const unsigned j = q / (unsigned)S.nx, i = q - j * (unsigned)S.nx;
    const double r = S.ref ? S.ref[(long)i + S.rsy * (long)j] : 0.0;
    const double *c = S.p + (long)i + S.sy * (long)j;
    for (int k = 0; k < S.nz; k++) { const unsigned long long key = key_of(fabs(c[S.sz * (long)k] - r)); mx = key > mx ? key : mx; }
  }
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long x2 = __shfl_down(mx, o, 64); mx = x2 > mx ? x2 : mx; }
  __shared__ unsigned long long sm[FAB_THREADS / 64];
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < FAB_THREADS / 64; w++) mx = sm[w] > mx ? sm[w] : mx;
    atomicMax(out + S.kind, mx);
  }
}

// ---- host: errors, paths, text ----------------------------------------------------------------------------------------------------------------------
[[noreturn]] void io_fail(const char *what, const std::string &path) { const int e = errno; vdn_fail("%s %s: %s", what, path.c_str(), e ? strerror(e) : "failed"); }
struct File {
  FILE *f = nullptr; std::string path;
  File() {}
  File(const std::string &p, const char *mode) { open(p, mode); }
  void open(const std::string &p, const char *mode) { close_quiet(); path = p; errno = 0; f = fopen(p.c_str(), mode); if (!f) io_fail("cannot open", p); }
  void write(const void *d, size_t n) { errno = 0; if (n && fwrite(d, 1, n, f) != n) io_fail("write to", path); }
  void puts(const std::string &s) { write(s.data(), s.size()); }
  void close() { if (f) { FILE *g = f; f = nullptr; errno = 0; if (fclose(g) != 0) io_fail("write to", path); } }
  void close_quiet() { if (f) { fclose(f); f = nullptr; } }
  ~File() { close_quiet(); }
  File(const File &) = delete; File &operator=(const File &) = delete;
};
void mkdirs(const std::string &dir) {          // os.makedirs(dir, exist_ok = True)
  for (size_t i = 1; i <= dir.size(); i++) {
    if (i != dir.size() && dir[i] != '/') continue;
    const std::string p = dir.substr(0, i);
    errno = 0;
    if (mkdir(p.c_str(), 0777) != 0 && errno != EEXIST) io_fail("cannot create directory", p);
  }
  struct stat st;
  errno = 0;
  if (stat(dir.c_str(), &st) != 0) io_fail("cannot create directory", dir);
  if (!S_ISDIR(st.st_mode)) { errno = ENOTDIR; io_fail("cannot create directory", dir); }
}
std::string fmt(const char *f, ...) { char b[512]; va_list ap; va_start(ap, f); vsnprintf(b, sizeof b, f, ap); va_end(ap); return b; }
// Fortran es27.17e3 (plotfile._es)
std::string es(double x, bool pad = true) {
  char b[64]; snprintf(b, sizeof b, "%.17E", x);
  std::string s = b;
  const size_t e = s.find('E');
  if (e != std::string::npos) { const int ex = atoi(s.c_str() + e + 2); s = s.substr(0, e) + fmt("E%c%03d", s[e + 1], ex); }
  if (pad && s.size() < 27) s = std::string(27 - s.size(), ' ') + s;
  return s;
}
std::string boxstr(const int *lo, const int *hi, const int *nodal, int dm) {
  std::string s = "(";
  const int *v[3] = {lo, hi, nodal};
  for (int g = 0; g < 3; g++) {
    s += g ? " (" : "(";
    for (int d = 0; d < dm; d++) s += (d ? "," : "") + std::to_string(v[g][d]);
    s += ")";
  }
  return s + ")";
}
std::string strip(const std::string &s) {
  size_t a = 0, b = s.size();
  while (a < b && isspace((unsigned char)s[a])) a++;
  while (b > a && isspace((unsigned char)s[b - 1])) b--;
  return s.substr(a, b - a);
}

// a text file as lines; every access is bounds-checked
struct Text {
  std::string path; std::vector<std::string> ln;
  explicit Text(const std::string &p) : path(p) {
    File f(p, "rb");
    std::string all; char buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f.f)) > 0) all.append(buf, n);
    if (ferror(f.f)) io_fail("cannot read", p);
    size_t a = 0;
    for (;;) { const size_t e = all.find('\n', a); if (e == std::string::npos) { ln.push_back(all.substr(a)); break; } ln.push_back(all.substr(a, e - a)); a = e + 1; }
  }
  const std::string &line(size_t i) const { if (i >= ln.size()) vdn_fail("%s: the file ends before line %zu", path.c_str(), i + 1); return ln[i]; }
  std::vector<long> ints(size_t i, size_t at_least) const {
    std::vector<long> v; const char *c = line(i).c_str();
    for (;;) { char *e; const long x = strtol(c, &e, 10); if (e == c) break; v.push_back(x); c = e; }
    if (v.size() < at_least) vdn_fail("%s: line %zu: expected %zu integer(s), found \"%.60s\"", path.c_str(), i + 1, at_least, ln[i].c_str());
    return v;
  }
  std::vector<double> reals(size_t i, size_t at_least) const {
    std::vector<double> v; const char *c = line(i).c_str();
    for (;;) { char *e; const double x = strtod(c, &e); if (e == c) break; v.push_back(x); c = e; }
    if (v.size() < at_least) vdn_fail("%s: line %zu: expected %zu number(s), found \"%.60s\"", path.c_str(), i + 1, at_least, ln[i].c_str());
    return v;
  }
};
// the groups "(a,b,c)" of integers in a box line "((lo) (hi) (nodal))", as re.findall(r"\(([-\d,]+)\)") gives them
std::vector<std::vector<int>> int_groups(const std::string &s) {
  std::vector<std::vector<int>> out;
  for (size_t i = 0; i < s.size(); i++) {
    if (s[i] != '(') continue;
    size_t j = i + 1; std::vector<int> g; bool ok = false;
    while (j < s.size()) {
      char *e; const char *c = s.c_str() + j;
      if (!(isdigit((unsigned char)*c) || *c == '-')) break;
      const long x = strtol(c, &e, 10); if (e == c) break;
      g.push_back((int)x); j = (size_t)(e - s.c_str());
      if (j < s.size() && s[j] == ',') { j++; continue; }
      ok = j < s.size() && s[j] == ')'; break;
    }
    if (ok && !g.empty()) { out.push_back(g); i = j; }
  }
  return out;
}

// ---- Header of a hierarchy and Cell_H of a level, as read_ml_multifab / _read_level parse them ---------------------------------------------------------
struct MlHeader { int nc = 0, dm = 0, nlev = 0; double time = 0; std::vector<int> rr; std::vector<std::string> paths; };
MlHeader read_ml_header(const std::string &dir) {
  Text t(dir + "/Header");
  MlHeader h;
  h.nc = (int)t.ints(1, 1)[0];
  if (h.nc < 1 || h.nc > 4096) vdn_fail("%s: %d components", t.path.c_str(), h.nc);
  const size_t k = 2 + (size_t)h.nc;
  h.dm = (int)t.ints(k, 1)[0]; h.time = t.reals(k + 1, 1)[0]; h.nlev = (int)t.ints(k + 2, 1)[0] + 1;
  if (h.dm < 1 || h.dm > 3 || h.nlev < 1) vdn_fail("%s: dm = %d, %d levels", t.path.c_str(), h.dm, h.nlev);
  for (long r : t.ints(k + 5, (size_t)h.nlev - 1)) h.rr.push_back((int)r);
  for (const std::string &raw : t.ln) {          // the lines "Level_NN/Cell"
    const std::string s = strip(raw);
    if (s.compare(0, 6, "Level_") != 0) continue;
    size_t i = 6; while (i < s.size() && isdigit((unsigned char)s[i])) i++;
    if (i == 6 || i >= s.size() || s[i] != '/' || i + 1 >= s.size()) continue;
    bool word = true; for (size_t j = i + 1; j < s.size(); j++) word = word && (isalnum((unsigned char)s[j]) || s[j] == '_');
    if (word) h.paths.push_back(s);
  }
  if ((int)h.paths.size() < h.nlev) vdn_fail("%s: %d levels announced, %zu level directories named (truncated?)", t.path.c_str(), h.nlev, h.paths.size());
  return h;
}
struct LevelH { std::string dir; int nc = 0, nodal[3] = {0, 0, 0}; std::vector<vdn_box> boxes /* cells */; std::vector<std::string> file; std::vector<long> off; };
LevelH read_level_h(const std::string &dir, const std::string &path /* Level_NN/Cell */) {
  const size_t sl = path.find('/');
  LevelH L; L.dir = dir + "/" + path.substr(0, sl);
  Text t(L.dir + "/" + path.substr(sl + 1) + "_H");
  L.nc = (int)t.ints(2, 1)[0];
  const std::string &l4 = t.line(4);
  char *e; const long nb = strtol(l4.c_str() + (l4.empty() || l4[0] != '(' ? 0 : 1), &e, 10);
  if (nb < 1 || nb > (1 << 24) || L.nc < 1) vdn_fail("%s: %ld boxes, %d components", t.path.c_str(), nb, L.nc);
  for (long b = 0; b < nb; b++) {
    const auto g = int_groups(t.line(5 + (size_t)b));
    if (g.size() < 3 || g[0].size() != g[1].size() || g[0].size() != g[2].size() || g[0].size() > 3)
      vdn_fail("%s: line %ld is not a box: \"%.60s\"", t.path.c_str(), 6 + b, t.line(5 + (size_t)b).c_str());
    vdn_box bx; memset(&bx, 0, sizeof bx);
    for (size_t d = 0; d < 3; d++) L.nodal[d] = d < g[2].size() ? g[2][d] : 0;
    for (size_t d = 0; d < g[0].size(); d++) { bx.lo[d] = g[0][d]; bx.hi[d] = g[1][d] - L.nodal[d]; }
    L.boxes.push_back(bx);
  }
  const size_t k = 5 + (size_t)nb + 2;
  for (long b = 0; b < nb; b++) {
    const std::string &s = t.line(k + (size_t)b);
    char name[256]; long off = -1;
    if (sscanf(s.c_str(), "FabOnDisk: %255s %ld", name, &off) != 2 || off < 0 || strchr(name, '/'))
      vdn_fail("%s: line %zu is not a FabOnDisk line: \"%.60s\"", t.path.c_str(), k + (size_t)b + 1, s.c_str());
    L.file.push_back(name); L.off.push_back(off);
  }
  return L;
}

// ---- the segment table of one level ------------------------------------------------------------------------------------------------------------------
struct LevelPlan {
  int nb = 0, nc = 0;
  std::vector<FabSeg> segs;          // [box * nc + comp]
  std::vector<long> box_off;         // payload offset (doubles) of every box, [nb + 1]
  std::vector<vdn_box> pts;          // valid POINT range of every box (hi includes the nodal point)
  long total() const { return box_off[nb]; }
  long npieces() const { const FabSeg &l = segs.back(); return l.piece0 + (l.len + FAB_PIECE - 1) / FAB_PIECE; }
  long piece_of(long x) const {      // the piece that holds element x
    size_t lo = 0, hi = segs.size() - 1;
    while (lo < hi) { const size_t mid = (lo + hi + 1) >> 1; if (segs[mid].off <= x) lo = mid; else hi = mid - 1; }
    return segs[lo].piece0 + (x - segs[lo].off) / FAB_PIECE;
  }
};
// boxes `idx` of mf (all of them when idx is NULL), components comps[nc] (0 .. nc-1 when comps is NULL).  plane: only the valid points of plane k = 0 (the node plane
// when nodal in z) -- a segment of len = nx ny whose rows the pack kernel addresses like any other box's
LevelPlan plan_level(const vdn_multifab *mf, int nc, const std::vector<int> *idx = nullptr, const int *comps = nullptr, bool plane = false) {
  LevelPlan P; P.nb = idx ? (int)idx->size() : mf->nfabs(); P.nc = nc;
  long off = 0, piece = 0;
  for (int g = 0; g < P.nb; g++) {
    const int i = idx ? (*idx)[g] : g;
    const FV &f = mf->fabs[i]; const vdn_box &b = mf->vbox[i];
    vdn_box pt = b; for (int d = 0; d < 3; d++) pt.hi[d] += mf->nodal[d];
    if (plane) {
      REQUIRE(pt.lo[2] <= 0 && pt.hi[2] >= 0, "fabio: box %d of level %d does not hold plane k = 0", i, mf->lev);
      pt.lo[2] = pt.hi[2] = 0;
    }
    const long nx = pt.hi[0] - pt.lo[0] + 1, ny = pt.hi[1] - pt.lo[1] + 1, nz = pt.hi[2] - pt.lo[2] + 1, len = nx * ny * nz;
    REQUIRE(nx > 0 && ny > 0 && nz > 0 && len < (1l << 31), "fabio: box %d of level %d holds %ld points", i, mf->lev, len);
    REQUIRE(pt.lo[0] >= f.a0 && pt.lo[1] >= f.a1 && pt.lo[2] >= f.a2 && pt.hi[0] < f.a0 + f.n0 && pt.hi[1] < f.a1 + f.n1 && pt.hi[2] < f.a2 + f.n2,
            "fabio: box %d of level %d: the valid points leave the fab", i, mf->lev);
    const long sy = f.n0, sz = (long)f.n0 * f.n1;
    double *p0 = f.p + (pt.lo[0] - f.a0) + sy * (pt.lo[1] - f.a1) + sz * (pt.lo[2] - f.a2);
    P.box_off.push_back(off); P.pts.push_back(pt);
    for (int c = 0; c < nc; c++) {
      FabSeg s; s.p = p0 + f.sc * (comps ? comps[c] : c); s.off = off; s.piece0 = piece; s.sy = sy; s.sz = sz; s.len = (int)len; s.nx = (int)nx; s.ny = (int)ny; s.pad = 0;
      P.segs.push_back(s);
      off += len; piece += (len + FAB_PIECE - 1) / FAB_PIECE;
    }
  }
  P.box_off.push_back(off);
  return P;
}

// ---- staging: device from the per-call arena, host one pinned buffer kept until vdn_finalize -------------------------------------------------------------
double *g_pinned = nullptr; size_t g_pinned_bytes = 0;
double *pinned_staging(size_t bytes) {
  if (bytes > g_pinned_bytes) {
    fabio_release();
    HIPCHK(hipHostMalloc((void **)&g_pinned, bytes, hipHostMallocDefault));
    g_pinned_bytes = bytes;
  }
  return g_pinned;
}
struct Staging { double *dev = nullptr, *host = nullptr; long elems = 0; };
// staging_bytes <= 0: the default.  Neither buffer is made larger than the largest level's payload.
Staging make_staging(long staging_bytes, long largest_level) {
  Staging s;
  const long cap = (staging_bytes > 0 ? staging_bytes : FAB_STAGING_DEFAULT) / 8;
  s.elems = std::max(1l, std::min(cap, largest_level));
  s.dev = (double *)arena_alloc((size_t)s.elems * 8);
  s.host = pinned_staging((size_t)s.elems * 8);
  return s;
}
FabSeg *upload_segs(const LevelPlan &P) {
  FabSeg *d = (FabSeg *)arena_alloc(P.segs.size() * sizeof(FabSeg));
  HIPCHK(hipMemcpyAsync(d, P.segs.data(), P.segs.size() * sizeof(FabSeg), hipMemcpyHostToDevice, ctx().stream));
  HIPCHK(hipStreamSynchronize(ctx().stream));
  return d;
}
void check_one_rank(const char *who) { REQUIRE(ctx().inited, "%s: vdn_init has not been called", who); REQUIRE(ctx().nranks == 1, "%s: several ranks: use the Python writer", who); }
void check_levels(const char *who, int nlev, vdn_multifab *const *mfs) {
  REQUIRE(nlev >= 1 && mfs, "%s: no levels", who);
  for (int n = 0; n < nlev; n++) {
    REQUIRE(mfs[n] && mfs[n]->nfabs() > 0, "%s: level %d has no boxes", who, n);
    REQUIRE((int)mfs[n]->la->boxes[mfs[n]->lev].size() == mfs[n]->nfabs(), "%s: level %d: boxes of other ranks", who, n);
  }
}

// ---- fabio_multifab_write_d of one level (plotfile._write_level) ---------------------------------------------------------------------------------------
void write_level(const std::string &dir, const LevelPlan &P, const int *nodal, int dm, const Staging &st) {
  VdnCtx &c = ctx();
  mkdirs(dir);
  const size_t mark = arena_mark();
  const int nb = P.nb, nc = P.nc, nseg = (int)P.segs.size();
  std::vector<std::string> hdr; std::vector<long> foff;
  long pos = 0;
  for (int g = 0; g < nb; g++) {
    hdr.push_back(FAB_DESC + boxstr(P.pts[g].lo, P.pts[g].hi, nodal, dm) + fmt(" %d\n", nc));
    foff.push_back(pos); pos += (long)hdr[g].size() + 8 * (P.box_off[g + 1] - P.box_off[g]);
  }
  FabSeg *d_segs = upload_segs(P);
  unsigned long long *d_mm = (unsigned long long *)arena_alloc((size_t)nseg * 16);          // minima, then maxima
  HIPCHK(hipMemsetAsync(d_mm, 0xFF, (size_t)nseg * 8, c.stream));
  HIPCHK(hipMemsetAsync(d_mm + nseg, 0, (size_t)nseg * 8, c.stream));
  {
    File f(dir + "/Cell_D_00000", "wb");
    int g = 0;
    for (long a = 0, b; a < P.total(); a = b) {
      b = std::min(a + st.elems, P.total());
      const long P0 = P.piece_of(a), P1 = P.piece_of(b - 1) + 1;
      hipLaunchKernelGGL(kk_fab_pack, dim3((unsigned)(P1 - P0)), dim3(FAB_THREADS), 0, c.stream, d_segs, nseg, P0, a, b, st.dev, d_mm, d_mm + nseg);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(st.host, st.dev, (size_t)(b - a) * 8, hipMemcpyDeviceToHost, c.stream));
      HIPCHK(hipStreamSynchronize(c.stream));
      for (; g < nb && P.box_off[g] < b; g++) {
        if (P.box_off[g] >= a) f.puts(hdr[g]);
        const long lo = std::max(a, P.box_off[g]), hi = std::min(b, P.box_off[g + 1]);
        f.write(st.host + (lo - a), (size_t)(hi - lo) * 8);
        if (P.box_off[g + 1] > b) break;          // the box goes on in the next range
      }
    }
    f.close();
  }
  std::vector<unsigned long long> mm((size_t)nseg * 2);
  HIPCHK(hipMemcpyAsync(mm.data(), d_mm, mm.size() * 8, hipMemcpyDeviceToHost, c.stream));
  HIPCHK(hipStreamSynchronize(c.stream));
  std::string h = fmt("1\n0\n%d\n0\n(%d 0\n", nc, nb);
  for (int g = 0; g < nb; g++) h += boxstr(P.pts[g].lo, P.pts[g].hi, nodal, dm) + "\n";
  h += fmt(")\n%d\n", nb);
  for (int g = 0; g < nb; g++) h += fmt("FabOnDisk: Cell_D_00000 %ld\n", foff[g]);
  for (int w = 0; w < 2; w++) {
    h += fmt("\n%d,%d\n", nb, nc);
    for (int g = 0; g < nb; g++) { for (int q = 0; q < nc; q++) h += es(key_value(mm[(size_t)w * nseg + (size_t)g * nc + q])) + ","; h += "\n"; }
  }
  File fh(dir + "/Cell_H", "wb"); fh.puts(h); fh.close();
  arena_release(mark);
}

// the files of a hierarchy whose levels are described by plans (segments), cell boxes (the Header's box corners) and shared nodal flags
struct MlPlans { std::vector<LevelPlan> plan; std::vector<std::vector<vdn_box>> cells; int nodal[3] = {0, 0, 0}; int dm = 3, nc = 0; };
void write_plans(const char *dirname, const MlPlans &M, const int *rr, const char *const *names, const vdn_box *pd0, const double *prob_lo_in,
                 const double *prob_hi_in, double time, const double *dx0, long staging_bytes) {
  const int nlev = (int)M.plan.size(), dm = M.dm, nc = M.nc;
  long largest = 0;
  for (const LevelPlan &P : M.plan) largest = std::max(largest, P.total());
  vdn_box pd;
  if (pd0) pd = *pd0;
  else {                                         // bounding box of level 0
    pd = M.cells[0][0];
    for (const vdn_box &b : M.cells[0]) for (int d = 0; d < 3; d++) { pd.lo[d] = std::min(pd.lo[d], b.lo[d]); pd.hi[d] = std::max(pd.hi[d], b.hi[d]); }
  }
  double plo[3], phi[3], dx[3];
  for (int d = 0; d < dm; d++) {
    const int n = pd.hi[d] - pd.lo[d] + 1;
    plo[d] = prob_lo_in ? prob_lo_in[d] : 0.0;
    phi[d] = prob_hi_in ? prob_hi_in[d] : (double)n;
    dx[d] = dx0 ? dx0[d] : (phi[d] - plo[d]) / n;
  }
  const std::string dir = dirname;
  mkdirs(dir);
  arena_reset();
  const Staging st = make_staging(staging_bytes, largest);
  for (int n = 0; n < nlev; n++) write_level(dir + fmt("/Level_%02d", n), M.plan[n], M.nodal, dm, st);
  std::string h = fmt("NavierStokes-V1.1\n%d\n", nc);
  for (int q = 0; q < nc; q++) h += (names ? strip(names[q] ? names[q] : "") : fmt("Var-%d", q + 1)) + "\n";
  h += fmt("%d\n", dm) + es(time) + fmt("\n%d\n", nlev - 1);
  for (int d = 0; d < dm; d++) h += es(plo[d]);
  h += "\n";
  for (int d = 0; d < dm; d++) h += es(phi[d]);
  h += "\n";
  for (int n = 0; n + 1 < nlev; n++) h += (n ? " " : "") + std::to_string(rr[n]);
  h += "\n";
  {
    int lo[3], hi[3]; const int zero[3] = {0, 0, 0};
    for (int d = 0; d < 3; d++) { lo[d] = pd.lo[d]; hi[d] = pd.hi[d]; }
    for (int n = 0; n < nlev; n++) {
      h += (n ? " " : "") + boxstr(lo, hi, zero, dm);
      if (n + 1 < nlev) for (int d = 0; d < 3; d++) { lo[d] *= rr[n]; hi[d] = (hi[d] + 1) * rr[n] - 1; }
    }
    h += "\n";
  }
  for (int n = 0; n < nlev; n++) h += n ? " 0" : "0";
  h += "\n";
  std::vector<double> dxs;          // [lev][dm]
  {
    double dxl[3] = {dx[0], dx[1], dx[2]};
    for (int n = 0; n < nlev; n++) {
      for (int d = 0; d < dm; d++) { dxs.push_back(dxl[d]); h += es(dxl[d]); }
      h += "\n";
      if (n + 1 < nlev) for (int d = 0; d < dm; d++) dxl[d] = dxl[d] / rr[n];
    }
  }
  h += "0\n0\n";
  for (int n = 0; n < nlev; n++) {
    h += fmt("%d %d ", n, (int)M.cells[n].size()) + es(time) + "\n0\n";
    for (const vdn_box &b : M.cells[n])
      for (int d = 0; d < dm; d++) h += es(plo[d] + (double)b.lo[d] * dxs[(size_t)n * dm + d]) + es(plo[d] + (double)(b.hi[d] + 1) * dxs[(size_t)n * dm + d]) + "\n";
    h += fmt("Level_%02d/Cell\n", n);
  }
  File f(dir + "/Header", "wb"); f.puts(h); f.close();
}

void write_ml(const char *dirname, int nlev, vdn_multifab *const *mfs, const int *rr, const char *const *names, const vdn_box *pd0, const double *prob_lo_in,
              const double *prob_hi_in, double time, const double *dx0, long staging_bytes) {
  check_one_rank("fabio_ml_multifab_write_d");
  REQUIRE(dirname && *dirname, "fabio_ml_multifab_write_d: no directory name");
  check_levels("fabio_ml_multifab_write_d", nlev, mfs);
  REQUIRE(nlev == 1 || rr, "fabio_ml_multifab_write_d: no refinement ratios");
  MlPlans M; M.dm = ctx().prm.dm; M.nc = mfs[0]->nc; memcpy(M.nodal, mfs[0]->nodal, sizeof M.nodal);
  for (int n = 0; n < nlev; n++) {
    REQUIRE(mfs[n]->nc == M.nc && !memcmp(mfs[n]->nodal, mfs[0]->nodal, sizeof mfs[0]->nodal), "fabio_ml_multifab_write_d: level %d differs from level 0 in components or nodal flags", n);
    M.plan.push_back(plan_level(mfs[n], M.nc)); M.cells.push_back(mfs[n]->vbox);
  }
  write_plans(dirname, M, rr, names, pd0, prob_lo_in, prob_hi_in, time, dx0, staging_bytes);
}

// ---- fabio_ml_multifab_read_d into multifabs built on the file's box lists ----------------------------------------------------------------------------
// the payload of one level, range by range: FAB lines checked against the plan's boxes, the doubles to the staging buffer, then launch(P0, P1, a, b) unpacks the range
template <class Launch> void read_payload(const LevelH &L, const LevelPlan &P, int n, const int *nodal, int dm, const Staging &st, Launch launch) {
  VdnCtx &c = ctx();
  const int nb = P.nb;
  File f;
  int g = 0;
  for (long a = 0, b; a < P.total(); a = b) {
    b = std::min(a + st.elems, P.total());
    for (; g < nb && P.box_off[g] < b; g++) {
      if (P.box_off[g] >= a) {          // the fab begins in this range: its FAB line
        const std::string p = L.dir + "/" + L.file[g];
        if (!f.f || f.path != p) f.open(p, "rb");
        errno = 0;
        if (fseek(f.f, L.off[g], SEEK_SET) != 0) io_fail("cannot seek in", p);
        char line[512];
        if (!fgets(line, sizeof line, f.f)) { if (ferror(f.f)) io_fail("cannot read", p); vdn_fail("level %d, box %d: %s ends before the FAB line (offset %ld)", n, g, p.c_str(), L.off[g]); }
        const std::string want = FAB_DESC + boxstr(P.pts[g].lo, P.pts[g].hi, nodal, dm) + fmt(" %d\n", L.nc);
        if (strncmp(line, FAB_DESC, strlen(FAB_DESC)) != 0) vdn_fail("level %d, box %d: %s, offset %ld: unsupported FAB descriptor (not FAB_DESC): \"%.80s\"", n, g, p.c_str(), L.off[g], line);
        if (want != line) vdn_fail("level %d, box %d: %s, offset %ld: the FAB line names another box or component count: \"%.120s\"", n, g, p.c_str(), L.off[g], line);
      }
      const long lo = std::max(a, P.box_off[g]), hi = std::min(b, P.box_off[g + 1]);
      errno = 0;
      const size_t got = fread(st.host + (lo - a), 8, (size_t)(hi - lo), f.f);
      if (got != (size_t)(hi - lo)) {
        if (ferror(f.f)) io_fail("cannot read", f.path);
        vdn_fail("level %d, box %d: %s is cut short: %ld of the box's %ld values are missing", n, g, f.path.c_str(), P.box_off[g + 1] - lo - (long)got, P.box_off[g + 1] - P.box_off[g]);
      }
      if (P.box_off[g + 1] > b) break;
    }
    const long P0 = P.piece_of(a), P1 = P.piece_of(b - 1) + 1;
    HIPCHK(hipMemcpyAsync(st.dev, st.host, (size_t)(b - a) * 8, hipMemcpyHostToDevice, c.stream));
    launch(P0, P1, a, b);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c.stream));
  }
}
void read_level(const std::string &dir, const std::string &path, int n, vdn_multifab *mf, int dm, const Staging &st) {
  VdnCtx &c = ctx();
  const LevelH L = read_level_h(dir, path);
  const int nb = (int)L.boxes.size();
  REQUIRE(nb == mf->nfabs(), "fabio_ml_multifab_read_d: level %d: the file holds %d boxes, the multifab %d", n, nb, mf->nfabs());
  REQUIRE(L.nc <= mf->nc, "fabio_ml_multifab_read_d: level %d: the file holds %d components, the multifab %d", n, L.nc, mf->nc);
  for (int g = 0; g < nb; g++) {
    const vdn_box &a = L.boxes[g], &b = mf->vbox[g];
    REQUIRE(!memcmp(&a, &b, sizeof a), "fabio_ml_multifab_read_d: level %d, box %d: the file holds (%d,%d,%d)-(%d,%d,%d), the multifab (%d,%d,%d)-(%d,%d,%d)", n, g,
            a.lo[0], a.lo[1], a.lo[2], a.hi[0], a.hi[1], a.hi[2], b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2]);
  }
  REQUIRE(!memcmp(L.nodal, mf->nodal, sizeof L.nodal), "fabio_ml_multifab_read_d: level %d, box 0: the file's nodal flags are (%d,%d,%d), the multifab's (%d,%d,%d)", n,
          L.nodal[0], L.nodal[1], L.nodal[2], mf->nodal[0], mf->nodal[1], mf->nodal[2]);
  const size_t mark = arena_mark();
  const LevelPlan P = plan_level(mf, L.nc);
  const int nseg = (int)P.segs.size();
  FabSeg *d_segs = upload_segs(P);
  read_payload(L, P, n, mf->nodal, dm, st, [&](long P0, long P1, long a, long b) {
    hipLaunchKernelGGL(kk_fab_unpack, dim3((unsigned)(P1 - P0)), dim3(FAB_THREADS), 0, c.stream, d_segs, nseg, P0, a, b, st.dev);
  });
  arena_release(mark);
}

void read_ml(const char *dirname, int nlev, vdn_multifab *const *mfs, long staging_bytes) {
  check_one_rank("fabio_ml_multifab_read_d");
  REQUIRE(dirname && *dirname, "fabio_ml_multifab_read_d: no directory name");
  check_levels("fabio_ml_multifab_read_d", nlev, mfs);
  const std::string dir = dirname;
  const MlHeader H = read_ml_header(dir);
  REQUIRE(H.nlev == nlev, "fabio_ml_multifab_read_d: %s holds %d levels, %d multifabs were given", dirname, H.nlev, nlev);
  REQUIRE(H.dm == ctx().prm.dm, "fabio_ml_multifab_read_d: %s is %d-dimensional, the run %d-dimensional", dirname, H.dm, ctx().prm.dm);
  long largest = 0;
  for (int n = 0; n < nlev; n++) {
    long tot = 0;
    for (int i = 0; i < mfs[n]->nfabs(); i++) { long v = mfs[n]->nc; for (int d = 0; d < 3; d++) v *= mfs[n]->vbox[i].hi[d] - mfs[n]->vbox[i].lo[d] + 1 + mfs[n]->nodal[d]; tot += v; }
    largest = std::max(largest, tot);
  }
  arena_reset();
  const Staging st = make_staging(staging_bytes, largest);
  for (int n = 0; n < nlev; n++) read_level(dir, H.paths[n], n, mfs[n], H.dm, st);
}

// ---- dm = 2 files of a z-uniform 3-D copy: plane k = 0 out, one plane into every plane ---------------------------------------------------------------------------
bool same_footprint(const vdn_box &a, const vdn_box &b) { return a.lo[0] == b.lo[0] && a.lo[1] == b.lo[1] && a.hi[0] == b.hi[0] && a.hi[1] == b.hi[1]; }
// the file boxes of a level (the boxes that hold plane k = 0, in the multifab's order) and, for every box, the file box of its footprint; host checks only
struct PlaneMap { std::vector<int> file_box, of; };
PlaneMap plane_map(const char *who, const vdn_multifab *mf, int n) {
  PlaneMap M; const int nb = mf->nfabs();
  for (int i = 0; i < nb; i++) if (mf->vbox[i].lo[2] <= 0 && mf->vbox[i].hi[2] + mf->nodal[2] >= 0) M.file_box.push_back(i);
  REQUIRE(!M.file_box.empty(), "%s: level %d: no box holds plane k = 0", who, n);
  for (size_t g = 0; g < M.file_box.size(); g++) for (size_t h = 0; h < g; h++) {
    const vdn_box &a = mf->vbox[M.file_box[g]], &b = mf->vbox[M.file_box[h]];
    REQUIRE(a.lo[0] > b.hi[0] || b.lo[0] > a.hi[0] || a.lo[1] > b.hi[1] || b.lo[1] > a.hi[1],
            "%s: level %d, box %d: its footprint (%d,%d)-(%d,%d) overlaps that of box %d; both hold plane k = 0", who, n, M.file_box[g], a.lo[0], a.lo[1], a.hi[0], a.hi[1], M.file_box[h]);
  }
  M.of.assign(nb, -1);
  for (int i = 0; i < nb; i++) {
    for (size_t g = 0; g < M.file_box.size() && M.of[i] < 0; g++) if (same_footprint(mf->vbox[i], mf->vbox[M.file_box[g]])) M.of[i] = (int)g;
    const vdn_box &a = mf->vbox[i];
    REQUIRE(M.of[i] >= 0, "%s: level %d, box %d: its footprint (%d,%d)-(%d,%d) is not that of any box that holds plane k = 0", who, n, i, a.lo[0], a.lo[1], a.hi[0], a.hi[1]);
  }
  return M;
}
void check_comps(const char *who, const char *what, int n, const int *comps, int nc) {
  REQUIRE(n >= 0 && (n == 0 || comps), "%s: no %s", who, what);
  for (int c = 0; c < n; c++) REQUIRE(comps[c] >= 0 && comps[c] < nc, "%s: %s %d = %d, the multifab holds %d", who, what, c, comps[c], nc);
}
double *first_valid(const vdn_multifab *mf, int i, int comp) {
  const FV &f = mf->fabs[i]; const vdn_box &b = mf->vbox[i];
  REQUIRE(b.lo[0] >= f.a0 && b.lo[1] >= f.a1 && b.lo[2] >= f.a2 && b.hi[0] + mf->nodal[0] < f.a0 + f.n0 && b.hi[1] + mf->nodal[1] < f.a1 + f.n1 && b.hi[2] + mf->nodal[2] < f.a2 + f.n2,
          "fabio: box %d of level %d: the valid points leave the fab", i, mf->lev);
  return f.p + (b.lo[0] - f.a0) + (long)f.n0 * (b.lo[1] - f.a1) + (long)f.n0 * f.n1 * (b.lo[2] - f.a2) + f.sc * comp;
}
void write_plane(const char *who, const char *dirname, int nlev, vdn_multifab *const *mfs, const int *rr, const char *const *names, const vdn_box *pd0, const double *prob_lo,
                 const double *prob_hi, double time, const double *dx0, long staging_bytes, int ncomp, const int *comps, int nvanish, const int *vanish, double *defect) {
  VdnCtx &c = ctx();
  check_one_rank(who);
  REQUIRE(dirname && *dirname, "%s: no directory name", who);
  check_levels(who, nlev, mfs);
  REQUIRE(nlev == 1 || rr, "%s: no refinement ratios", who);
  REQUIRE(ncomp >= 1, "%s: no components", who);
  MlPlans M; M.dm = 2; M.nc = ncomp; M.nodal[0] = mfs[0]->nodal[0]; M.nodal[1] = mfs[0]->nodal[1];
  std::vector<PlaneMap> maps;
  for (int n = 0; n < nlev; n++) {
    REQUIRE(!memcmp(mfs[n]->nodal, mfs[0]->nodal, sizeof mfs[0]->nodal), "%s: level %d differs from level 0 in its nodal flags", who, n);
    check_comps(who, "component", ncomp, comps, mfs[n]->nc); check_comps(who, "vanishing component", nvanish, vanish, mfs[n]->nc);
    maps.push_back(plane_map(who, mfs[n], n));
    M.plan.push_back(plan_level(mfs[n], ncomp, &maps[n].file_box, comps, true));
    std::vector<vdn_box> cells;
    for (int i : maps[n].file_box) { vdn_box b = mfs[n]->vbox[i]; b.lo[2] = b.hi[2] = 0; cells.push_back(b); }
    M.cells.push_back(cells);
  }
  write_plans(dirname, M, rr, names, pd0, prob_lo, prob_hi, time, dx0, staging_bytes);
  if (!defect) return;
  const size_t mark = arena_mark();
  std::vector<DefSeg> segs; long piece = 0;
  for (int n = 0; n < nlev; n++) {
    const vdn_multifab *mf = mfs[n];
    for (int i = 0; i < mf->nfabs(); i++) for (int q = 0; q < ncomp + nvanish; q++) {
      const vdn_box &b = mf->vbox[i]; const FV &f = mf->fabs[i];
      DefSeg s; s.kind = q < ncomp ? 0 : 1;
      s.p = first_valid(mf, i, q < ncomp ? comps[q] : vanish[q - ncomp]); s.sy = f.n0; s.sz = (long)f.n0 * f.n1;
      const FabSeg *r = q < ncomp ? &M.plan[n].segs[(size_t)maps[n].of[i] * ncomp + q] : nullptr;
      s.ref = r ? r->p : nullptr; s.rsy = r ? r->sy : 0;
      s.nx = b.hi[0] - b.lo[0] + 1 + mf->nodal[0]; s.ny = b.hi[1] - b.lo[1] + 1 + mf->nodal[1]; s.nz = b.hi[2] - b.lo[2] + 1 + mf->nodal[2];
      s.piece0 = piece; piece += ((long)s.nx * s.ny + DEF_PIECE - 1) / DEF_PIECE;
      segs.push_back(s);
    }
  }
  REQUIRE(piece < (1l << 31), "%s: %ld workgroups", who, piece);
  DefSeg *d_segs = (DefSeg *)arena_alloc(segs.size() * sizeof(DefSeg));
  unsigned long long *d_out = (unsigned long long *)arena_alloc(16), h_out[2] = {0x8000000000000000ull, 0x8000000000000000ull};      // the key of +0
  HIPCHK(hipMemcpyAsync(d_segs, segs.data(), segs.size() * sizeof(DefSeg), hipMemcpyHostToDevice, c.stream));
  HIPCHK(hipMemcpyAsync(d_out, h_out, 16, hipMemcpyHostToDevice, c.stream));
  HIPCHK(hipStreamSynchronize(c.stream));
  hipLaunchKernelGGL(kk_plane_defect, dim3((unsigned)piece), dim3(FAB_THREADS), 0, c.stream, (const DefSeg *)d_segs, (int)segs.size(), d_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h_out, d_out, 16, hipMemcpyDeviceToHost, c.stream));
  HIPCHK(hipStreamSynchronize(c.stream));
  defect[0] = key_value(h_out[0]); defect[1] = key_value(h_out[1]);
  arena_release(mark);
}

void read_plane_level(const std::string &dir, const std::string &path, int n, vdn_multifab *mf, int ncomp, const int *comps, const Staging &st) {
  const char *who = "fabio_ml_multifab_read_plane_d";
  VdnCtx &c = ctx();
  const LevelH L = read_level_h(dir, path);
  const int nb = (int)L.boxes.size();
  REQUIRE(L.nc == ncomp, "%s: level %d: the file holds %d components, %d were named", who, n, L.nc, ncomp);
  REQUIRE(L.nodal[0] == mf->nodal[0] && L.nodal[1] == mf->nodal[1], "%s: level %d, box 0: the file's nodal flags are (%d,%d), the multifab's in-plane ones (%d,%d)", who, n,
          L.nodal[0], L.nodal[1], mf->nodal[0], mf->nodal[1]);
  // every box of the multifab -> its file box
  std::vector<std::vector<int>> dst_of(nb);
  for (int i = 0; i < mf->nfabs(); i++) {
    int hit = -1, hits = 0;
    for (int g = 0; g < nb; g++) if (same_footprint(mf->vbox[i], L.boxes[g])) { hit = g; hits++; }
    const vdn_box &a = mf->vbox[i];
    REQUIRE(hits == 1, "%s: level %d, box %d: its footprint (%d,%d)-(%d,%d) is that of %d boxes of the file", who, n, i, a.lo[0], a.lo[1], a.hi[0], a.hi[1], hits);
    dst_of[hit].push_back(i);
  }
  for (int g = 0; g < nb; g++)
    REQUIRE(!dst_of[g].empty(), "%s: level %d: box %d of the file, (%d,%d)-(%d,%d), is the footprint of no box of the multifab", who, n, g, L.boxes[g].lo[0], L.boxes[g].lo[1],
            L.boxes[g].hi[0], L.boxes[g].hi[1]);
  // the file's linear space: box, component, y, x; the destinations of every (box, component)
  LevelPlan P; P.nb = nb; P.nc = ncomp;
  std::vector<int> dst0; std::vector<PlaneDst> dsts;
  long off = 0, piece = 0;
  for (int g = 0; g < nb; g++) {
    vdn_box pt = L.boxes[g]; pt.hi[0] += L.nodal[0]; pt.hi[1] += L.nodal[1]; pt.lo[2] = pt.hi[2] = 0;
    const long nx = pt.hi[0] - pt.lo[0] + 1, ny = pt.hi[1] - pt.lo[1] + 1, len = nx * ny;
    REQUIRE(nx > 0 && ny > 0 && len < (1l << 31), "%s: box %d of level %d holds %ld points", who, g, n, len);
    P.box_off.push_back(off); P.pts.push_back(pt);
    for (int q = 0; q < ncomp; q++) {
      FabSeg s; s.p = nullptr; s.off = off; s.piece0 = piece; s.sy = nx; s.sz = len; s.len = (int)len; s.nx = (int)nx; s.ny = (int)ny; s.pad = 0;
      P.segs.push_back(s);
      off += len; piece += (len + FAB_PIECE - 1) / FAB_PIECE;
      dst0.push_back((int)dsts.size());
      for (int i : dst_of[g]) {
        const FV &f = mf->fabs[i];
        PlaneDst D; D.p = first_valid(mf, i, comps[q]); D.sy = f.n0; D.sz = (long)f.n0 * f.n1; D.nz = mf->vbox[i].hi[2] - mf->vbox[i].lo[2] + 1 + mf->nodal[2]; D.pad = 0;
        dsts.push_back(D);
      }
    }
  }
  P.box_off.push_back(off); dst0.push_back((int)dsts.size());
  const size_t mark = arena_mark();
  const int nseg = (int)P.segs.size();
  FabSeg *d_segs = upload_segs(P);
  int *d_dst0 = (int *)arena_alloc(dst0.size() * sizeof(int));
  PlaneDst *d_dsts = (PlaneDst *)arena_alloc(dsts.size() * sizeof(PlaneDst));
  HIPCHK(hipMemcpyAsync(d_dst0, dst0.data(), dst0.size() * sizeof(int), hipMemcpyHostToDevice, c.stream));
  HIPCHK(hipMemcpyAsync(d_dsts, dsts.data(), dsts.size() * sizeof(PlaneDst), hipMemcpyHostToDevice, c.stream));
  HIPCHK(hipStreamSynchronize(c.stream));
  read_payload(L, P, n, L.nodal, 2, st, [&](long P0, long P1, long a, long b) {
    hipLaunchKernelGGL(kk_fab_unpack_extrude, dim3((unsigned)(P1 - P0)), dim3(FAB_THREADS), 0, c.stream, d_segs, nseg, P0, a, b, (const double *)st.dev, (const int *)d_dst0,
                       (const PlaneDst *)d_dsts);
  });
  arena_release(mark);
}
void read_plane(const char *dirname, int nlev, vdn_multifab *const *mfs, long staging_bytes, int ncomp, const int *comps) {
  const char *who = "fabio_ml_multifab_read_plane_d";
  check_one_rank(who);
  REQUIRE(dirname && *dirname, "%s: no directory name", who);
  check_levels(who, nlev, mfs);
  REQUIRE(ncomp >= 1, "%s: no components", who);
  for (int n = 0; n < nlev; n++) check_comps(who, "component", ncomp, comps, mfs[n]->nc);
  const std::string dir = dirname;
  const MlHeader H = read_ml_header(dir);
  REQUIRE(H.nlev == nlev, "%s: %s holds %d levels, %d multifabs were given", who, dirname, H.nlev, nlev);
  REQUIRE(H.dm == 2, "%s: %s is %d-dimensional, not a plane file", who, dirname, H.dm);
  REQUIRE(H.nc == ncomp, "%s: %s holds %d components, %d were named", who, dirname, H.nc, ncomp);
  long largest = 0;          // (an upper bound: the staging buffer is never made larger than the largest level's payload)
  for (int n = 0; n < nlev; n++) {
    long tot = 0;
    for (int i = 0; i < mfs[n]->nfabs(); i++) { long v = ncomp; for (int d = 0; d < 2; d++) v *= mfs[n]->vbox[i].hi[d] - mfs[n]->vbox[i].lo[d] + 1 + mfs[n]->nodal[d]; tot += v; }
    largest = std::max(largest, tot);
  }
  arena_reset();
  const Staging st = make_staging(staging_bytes, largest);
  for (int n = 0; n < nlev; n++) read_plane_level(dir, H.paths[n], n, mfs[n], ncomp, comps, st);
}

// text-only entry points: no HIP call, usable without vdn_init and without a GPU
#define TEXT_TRY try {
#define TEXT_CATCH } catch (const std::exception &e) { vdn_set_error("%s", e.what()); return 1; } return 0;
}      // namespace

void fabio_release() {
  if (g_pinned) { (void)hipHostFree(g_pinned); g_pinned = nullptr; g_pinned_bytes = 0; }
}

extern "C" int vdn_fabio_ml_multifab_write_d(const char *dirname, int nlev, vdn_multifab *const *mfs, const int *rr, const char *const *names, const vdn_box *pd0,
                                             const double *prob_lo, const double *prob_hi, double time, const double *dx0, long staging_bytes) {
  VDN_TRY
  write_ml(dirname, nlev, mfs, rr, names, pd0, prob_lo, prob_hi, time, dx0, staging_bytes);
  VDN_CATCH
}
extern "C" int vdn_fabio_ml_multifab_read_d(const char *dirname, int nlev, vdn_multifab *const *mfs, long staging_bytes) {
  VDN_TRY
  read_ml(dirname, nlev, mfs, staging_bytes);
  VDN_CATCH
}
extern "C" int vdn_fabio_ml_multifab_info(const char *dirname, int *nlev, int *dm, int *ncomp, int nodal[3], int *nboxes, int *rr, double *time) {
  TEXT_TRY
  REQUIRE(dirname && *dirname, "fabio_ml_multifab_info: no directory name");
  const MlHeader H = read_ml_header(dirname);
  REQUIRE(H.nlev <= VDN_MAXLEV, "fabio_ml_multifab_info: %s holds %d levels, more than the %d the library takes", dirname, H.nlev, VDN_MAXLEV);
  if (nlev) *nlev = H.nlev;
  if (dm) *dm = H.dm;
  if (ncomp) *ncomp = H.nc;
  if (time) *time = H.time;
  if (rr) for (int n = 0; n + 1 < H.nlev; n++) rr[n] = H.rr[n];
  for (int n = 0; n < H.nlev && (nboxes || (n == 0 && nodal)); n++) {
    const LevelH L = read_level_h(dirname, H.paths[n]);
    if (nboxes) nboxes[n] = (int)L.boxes.size();
    if (n == 0 && nodal) for (int d = 0; d < 3; d++) nodal[d] = L.nodal[d];
  }
  TEXT_CATCH
}
extern "C" int vdn_fabio_ml_multifab_boxes(const char *dirname, int lev, vdn_box *boxes, int maxboxes) {
  TEXT_TRY
  REQUIRE(dirname && *dirname && boxes, "fabio_ml_multifab_boxes: no directory name or no array");
  const MlHeader H = read_ml_header(dirname);
  REQUIRE(lev >= 0 && lev < H.nlev, "fabio_ml_multifab_boxes: %s holds %d levels, level %d was asked for", dirname, H.nlev, lev);
  const LevelH L = read_level_h(dirname, H.paths[lev]);
  REQUIRE((int)L.boxes.size() <= maxboxes, "fabio_ml_multifab_boxes: level %d of %s holds %zu boxes, the array %d", lev, dirname, L.boxes.size(), maxboxes);
  for (size_t g = 0; g < L.boxes.size(); g++) boxes[g] = L.boxes[g];
  TEXT_CATCH
}

extern "C" int vdn_checkpoint_write(const char *dirname, int nlev, vdn_multifab *const *state, vdn_multifab *const *pressure, const int *rr, double time, double dt,
                                    long staging_bytes) {
  VDN_TRY
  check_one_rank("checkpoint_write");
  REQUIRE(dirname && *dirname, "checkpoint_write: no directory name");
  check_levels("checkpoint_write", nlev, state); check_levels("checkpoint_write", nlev, pressure);
  const std::string dir = dirname;
  mkdirs(dir);
  const vdn_box pd = state[0]->la->pd[state[0]->lev];
  write_ml((dir + "/State").c_str(), nlev, state, rr, nullptr, &pd, nullptr, nullptr, 0.0, nullptr, staging_bytes);
  write_ml((dir + "/Pressure").c_str(), nlev, pressure, rr, nullptr, &pd, nullptr, nullptr, 0.0, nullptr, staging_bytes);
  std::string h = "&CHKPOINT\n TIME=" + es(time, false) + ",\n DT=" + es(dt, false) + fmt(",\n NLEVS=%d,\n /\n", nlev);
  for (int n = 0; n + 1 < nlev; n++) h += fmt("%12d\n", rr[n]);
  File f(dir + "/Header", "wb"); f.puts(h); f.close();
  VDN_CATCH
}
extern "C" int vdn_fabio_ml_multifab_write_plane_d(const char *dirname, int nlev, vdn_multifab *const *mfs, const int *rr, const char *const *names, const vdn_box *pd0,
                                                   const double *prob_lo, const double *prob_hi, double time, const double *dx0, long staging_bytes, int ncomp,
                                                   const int *comps, int nvanish, const int *vanish, double *defect) {
  VDN_TRY
  write_plane("fabio_ml_multifab_write_plane_d", dirname, nlev, mfs, rr, names, pd0, prob_lo, prob_hi, time, dx0, staging_bytes, ncomp, comps, nvanish, vanish, defect);
  VDN_CATCH
}
extern "C" int vdn_fabio_ml_multifab_read_plane_d(const char *dirname, int nlev, vdn_multifab *const *mfs, long staging_bytes, int ncomp, const int *comps) {
  VDN_TRY
  read_plane(dirname, nlev, mfs, staging_bytes, ncomp, comps);
  VDN_CATCH
}
extern "C" int vdn_checkpoint_write_plane(const char *dirname, int nlev, vdn_multifab *const *state, vdn_multifab *const *pressure, const int *rr, double time, double dt,
                                          long staging_bytes, int ncomp, const int *comps, int nvanish, const int *vanish, double *defect) {
  VDN_TRY
  check_one_rank("checkpoint_write_plane");
  REQUIRE(dirname && *dirname, "checkpoint_write_plane: no directory name");
  check_levels("checkpoint_write_plane", nlev, state); check_levels("checkpoint_write_plane", nlev, pressure);
  const std::string dir = dirname;
  const vdn_box pd = state[0]->la->pd[state[0]->lev];
  const int p0 = 0; double ds[2] = {0, 0}, dp[2] = {0, 0};
  // (both hierarchies are checked before the first file appears: the State call creates the directory)
  for (int n = 0; n < nlev; n++) { plane_map("checkpoint_write_plane", state[n], n); plane_map("checkpoint_write_plane", pressure[n], n); }
  write_plane("checkpoint_write_plane", (dir + "/State").c_str(), nlev, state, rr, nullptr, &pd, nullptr, nullptr, 0.0, nullptr, staging_bytes, ncomp, comps, nvanish, vanish,
              defect ? ds : nullptr);
  write_plane("checkpoint_write_plane", (dir + "/Pressure").c_str(), nlev, pressure, rr, nullptr, &pd, nullptr, nullptr, 0.0, nullptr, staging_bytes, 1, &p0, 0, nullptr,
              defect ? dp : nullptr);
  if (defect) { defect[0] = (dp[0] > ds[0] || dp[0] != dp[0]) ? dp[0] : ds[0]; defect[1] = ds[1]; }          // (a NaN stays one)
  std::string h = "&CHKPOINT\n TIME=" + es(time, false) + ",\n DT=" + es(dt, false) + fmt(",\n NLEVS=%d,\n /\n", nlev);
  for (int n = 0; n + 1 < nlev; n++) h += fmt("%12d\n", rr[n]);
  File f(dir + "/Header", "wb"); f.puts(h); f.close();
  VDN_CATCH
}
extern "C" int vdn_checkpoint_info(const char *dirname, int *nlev, double *time, double *dt, int *rr) {
  TEXT_TRY
  REQUIRE(dirname && *dirname, "checkpoint_info: no directory name");
  const Text t(std::string(dirname) + "/Header");
  std::string all; for (const std::string &s : t.ln) all += s + "\n";
  // the namelist &CHKPOINT: name = value pairs, Fortran exponents (d) allowed
  bool have[3] = {false, false, false}; double val[3] = {0, 0, 0};
  const char *key[3] = {"time", "dt", "nlevs"};
  for (size_t i = 0; i < all.size();) {
    if (!(isalpha((unsigned char)all[i]) || all[i] == '_')) { i++; continue; }
    size_t j = i; while (j < all.size() && (isalnum((unsigned char)all[j]) || all[j] == '_')) j++;
    std::string name = all.substr(i, j - i); for (char &ch : name) ch = (char)tolower((unsigned char)ch);
    size_t k = j; while (k < all.size() && (all[k] == ' ' || all[k] == '\t')) k++;
    if (k < all.size() && all[k] == '=') {
      k++; while (k < all.size() && (all[k] == ' ' || all[k] == '\t')) k++;
      size_t e = k; while (e < all.size() && (isalnum((unsigned char)all[e]) || strchr("-+._", all[e]))) e++;
      std::string v = all.substr(k, e - k); for (char &ch : v) if (ch == 'd' || ch == 'D') ch = 'e';
      for (int q = 0; q < 3; q++) if (name == key[q]) { char *end; val[q] = strtod(v.c_str(), &end); have[q] = end != v.c_str(); }
      i = e;
    } else i = j;
  }
  REQUIRE(have[0] && have[1] && have[2], "%s: the namelist &CHKPOINT lacks %s (truncated?)", t.path.c_str(), !have[0] ? "time" : !have[1] ? "dt" : "nlevs");
  const int nl = (int)val[2];
  REQUIRE(nl >= 1 && nl <= VDN_MAXLEV, "%s: nlevs = %d", t.path.c_str(), nl);
  const size_t sl = all.find('/');
  REQUIRE(sl != std::string::npos, "%s: the namelist &CHKPOINT is not closed (truncated?)", t.path.c_str());
  const char *c = all.c_str() + sl + 1;
  for (int n = 0; n + 1 < nl; n++) {
    char *end; const long r = strtol(c, &end, 10);
    REQUIRE(end != c, "%s: %d refinement ratio(s) expected after the namelist, %d found", t.path.c_str(), nl - 1, n);
    if (rr) rr[n] = (int)r;
    c = end;
  }
  if (nlev) *nlev = nl;
  if (time) *time = val[0];
  if (dt) *dt = val[1];
  TEXT_CATCH
}
