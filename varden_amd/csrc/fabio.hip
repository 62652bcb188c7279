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
// (sign bit flipped for non-negative values, all bits for negative ones), so the values are exact -- not the shifted sums of vdn_multifab_min_max.  With that
// image -0 sorts below +0: a field holding both reports min = -0, max = +0.  kk_fab_unpack is the inverse over the same table; it writes valid points only.
// dm = 2: the fabs keep the 3-D layout with one valid z-plane (k = 0), which the segment's origin and extents address like any other box.
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

DEVI unsigned long long dkey(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
double key_to_double(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v; memcpy(&v, &b, 8); return v;
}

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
    const unsigned long long key = dkey(v);
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
LevelPlan plan_level(const vdn_multifab *mf, int nc) {
  LevelPlan P; P.nb = mf->nfabs(); P.nc = nc;
  long off = 0, piece = 0;
  for (int i = 0; i < P.nb; i++) {
    const FV &f = mf->fabs[i]; const vdn_box &b = mf->vbox[i];
    vdn_box pt = b; for (int d = 0; d < 3; d++) pt.hi[d] += mf->nodal[d];
    const long nx = pt.hi[0] - pt.lo[0] + 1, ny = pt.hi[1] - pt.lo[1] + 1, nz = pt.hi[2] - pt.lo[2] + 1, len = nx * ny * nz;
    REQUIRE(nx > 0 && ny > 0 && nz > 0 && len < (1l << 31), "fabio: box %d of level %d holds %ld points", i, mf->lev, len);
    REQUIRE(pt.lo[0] >= f.a0 && pt.lo[1] >= f.a1 && pt.lo[2] >= f.a2 && pt.hi[0] < f.a0 + f.n0 && pt.hi[1] < f.a1 + f.n1 && pt.hi[2] < f.a2 + f.n2,
            "fabio: box %d of level %d: the valid points leave the fab", i, mf->lev);
    const long sy = f.n0, sz = (long)f.n0 * f.n1;
    double *p0 = f.p + (pt.lo[0] - f.a0) + sy * (pt.lo[1] - f.a1) + sz * (pt.lo[2] - f.a2);
    P.box_off.push_back(off); P.pts.push_back(pt);
    for (int c = 0; c < nc; c++) {
      FabSeg s; s.p = p0 + f.sc * c; s.off = off; s.piece0 = piece; s.sy = sy; s.sz = sz; s.len = (int)len; s.nx = (int)nx; s.ny = (int)ny; s.pad = 0;
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
void write_level(const std::string &dir, const vdn_multifab *mf, int dm, const Staging &st) {
  VdnCtx &c = ctx();
  mkdirs(dir);
  const size_t mark = arena_mark();
  const LevelPlan P = plan_level(mf, mf->nc);
  const int nb = P.nb, nc = P.nc, nseg = (int)P.segs.size();
  std::vector<std::string> hdr; std::vector<long> foff;
  long pos = 0;
  for (int g = 0; g < nb; g++) {
    hdr.push_back(FAB_DESC + boxstr(P.pts[g].lo, P.pts[g].hi, mf->nodal, dm) + fmt(" %d\n", nc));
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
  for (int g = 0; g < nb; g++) h += boxstr(P.pts[g].lo, P.pts[g].hi, mf->nodal, dm) + "\n";
  h += fmt(")\n%d\n", nb);
  for (int g = 0; g < nb; g++) h += fmt("FabOnDisk: Cell_D_00000 %ld\n", foff[g]);
  for (int w = 0; w < 2; w++) {
    h += fmt("\n%d,%d\n", nb, nc);
    for (int g = 0; g < nb; g++) { for (int q = 0; q < nc; q++) h += es(key_to_double(mm[(size_t)w * nseg + (size_t)g * nc + q])) + ","; h += "\n"; }
  }
  File fh(dir + "/Cell_H", "wb"); fh.puts(h); fh.close();
  arena_release(mark);
}

void write_ml(const char *dirname, int nlev, vdn_multifab *const *mfs, const int *rr, const char *const *names, const vdn_box *pd0, const double *prob_lo_in,
              const double *prob_hi_in, double time, const double *dx0, long staging_bytes) {
  check_one_rank("fabio_ml_multifab_write_d");
  REQUIRE(dirname && *dirname, "fabio_ml_multifab_write_d: no directory name");
  check_levels("fabio_ml_multifab_write_d", nlev, mfs);
  REQUIRE(nlev == 1 || rr, "fabio_ml_multifab_write_d: no refinement ratios");
  const int dm = ctx().prm.dm, nc = mfs[0]->nc;
  long largest = 0;
  for (int n = 0; n < nlev; n++) {
    REQUIRE(mfs[n]->nc == nc && !memcmp(mfs[n]->nodal, mfs[0]->nodal, sizeof mfs[0]->nodal), "fabio_ml_multifab_write_d: level %d differs from level 0 in components or nodal flags", n);
    long tot = 0;
    for (int i = 0; i < mfs[n]->nfabs(); i++) { long v = nc; for (int d = 0; d < 3; d++) v *= mfs[n]->vbox[i].hi[d] - mfs[n]->vbox[i].lo[d] + 1 + mfs[n]->nodal[d]; tot += v; }
    largest = std::max(largest, tot);
  }
  vdn_box pd;
  if (pd0) pd = *pd0;
  else {                                         // bounding box of level 0
    pd = mfs[0]->vbox[0];
    for (const vdn_box &b : mfs[0]->vbox) for (int d = 0; d < 3; d++) { pd.lo[d] = std::min(pd.lo[d], b.lo[d]); pd.hi[d] = std::max(pd.hi[d], b.hi[d]); }
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
  for (int n = 0; n < nlev; n++) write_level(dir + fmt("/Level_%02d", n), mfs[n], dm, st);
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
    h += fmt("%d %d ", n, mfs[n]->nfabs()) + es(time) + "\n0\n";
    for (const vdn_box &b : mfs[n]->vbox)
      for (int d = 0; d < dm; d++) h += es(plo[d] + (double)b.lo[d] * dxs[(size_t)n * dm + d]) + es(plo[d] + (double)(b.hi[d] + 1) * dxs[(size_t)n * dm + d]) + "\n";
    h += fmt("Level_%02d/Cell\n", n);
  }
  File f(dir + "/Header", "wb"); f.puts(h); f.close();
}

// ---- fabio_ml_multifab_read_d into multifabs built on the file's box lists ----------------------------------------------------------------------------
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
        const std::string want = FAB_DESC + boxstr(P.pts[g].lo, P.pts[g].hi, mf->nodal, dm) + fmt(" %d\n", L.nc);
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
    hipLaunchKernelGGL(kk_fab_unpack, dim3((unsigned)(P1 - P0)), dim3(FAB_THREADS), 0, c.stream, d_segs, nseg, P0, a, b, st.dev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c.stream));
  }
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
