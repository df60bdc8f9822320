// tile_patches.hpp -- what tile_plan.cpp reads a mesh through, and the structured patches it cuts out of the tiling.
//
//   Mesh / Incidence   the reference-format arrays, and the faces of every owned element (element_faces)
//   exact_axis         "is this unit normal an exact axis normal?" -- the one place that asks (direction_code, the finders)
//   Patch              one structured block of 256 consecutive elements that the patch kernels evaluate without face records
//   find_patches       2D blocks (find_patches2), else 3D blocks (find_patches3: regular and irregular form), minus the
//                      blocks with an open boundary face (drop_open_patches)
//
// Private to tile_plan.cpp (one translation unit): everything here is inline or in its unnamed namespace.
#ifndef T8GPU_TILE_PATCHES_HPP
#define T8GPU_TILE_PATCHES_HPP

#include <algorithm>
#include <cstdint>
#include <vector>

#include "host_threads.hpp"

namespace {

// The reference-format arrays of one rank: fn = [F][2] (left, right) of the interior faces, then [B] the element of every
// boundary face; normals [F + B][ndim], areas [F + B]. Faces are numbered interior first: boundary face b has id F + b.
struct Mesh {
  int32_t        N = 0, F = 0, B = 0, ndim = 3;
  const int32_t* fn = nullptr;
  const double*  normals = nullptr;
  const double*  areas = nullptr;
  const uint8_t* kinds = nullptr;   // boundary_kinds[B], or null: all walls
  const double*  normal(int32_t f) const { return normals + static_cast<size_t>(ndim) * f; }
  int32_t        left(int32_t f) const { return fn[2 * static_cast<size_t>(f)]; }        // (interior faces)
  int32_t        right(int32_t f) const { return fn[2 * static_cast<size_t>(f) + 1]; }
  int32_t        boundary_element(int32_t b) const { return fn[2 * static_cast<size_t>(F) + b]; }
};

// The faces of every owned element in ascending face id: those of element e are ef[deg[e] .. deg[e + 1]).
struct Incidence {
  const Mesh*          mesh = nullptr;
  std::vector<int32_t> deg, ef;
  int32_t              most = 0;   // faces of one element
  int32_t        count(int32_t e) const { return deg[e + 1] - deg[e]; }
  const int32_t* faces(int32_t e) const { return &ef[deg[e]]; }
  // the element on the left (which = 0) / right (1) of face f; -1 behind a boundary face
  int32_t side(int32_t f, int which) const {
    if (f >= mesh->F) return which == 0 ? mesh->boundary_element(f - mesh->F) : -1;
    return mesh->fn[2 * static_cast<size_t>(f) + which];
  }
};

// Counted and placed in parallel over the faces (atomic cursors; original face order = interior faces first, then
// boundary faces), then every element's short list is sorted back into ascending face id.
inline Incidence element_faces(const Mesh& m) {
  const int32_t N = m.N, F = m.F, B = m.B;
  Incidence     inc;
  inc.mesh = &m;
  std::vector<int32_t>&deg = inc.deg, &ef = inc.ef;
  deg.assign(static_cast<size_t>(N) + 1, 0);
#pragma omp parallel for num_threads(host_threads()) schedule(static)
  for (int32_t f = 0; f < F; f++) {
    const int32_t l = m.left(f), r = m.right(f);
    if (l < N) __atomic_fetch_add(&deg[l + 1], 1, __ATOMIC_RELAXED);
    if (r < N && r != l) __atomic_fetch_add(&deg[r + 1], 1, __ATOMIC_RELAXED);
  }
  for (int32_t b = 0; b < B; b++) deg[m.boundary_element(b) + 1]++;
  for (int32_t e = 0; e < N; e++) deg[e + 1] += deg[e];
  ef.resize(deg[N]);
  std::vector<int32_t> cur(deg.begin(), deg.end() - 1);
#pragma omp parallel for num_threads(host_threads()) schedule(static)
  for (int32_t f = 0; f < F; f++) {
    const int32_t l = m.left(f), r = m.right(f);
    if (l < N) ef[__atomic_fetch_add(&cur[l], 1, __ATOMIC_RELAXED)] = f;
    if (r < N && r != l) ef[__atomic_fetch_add(&cur[r], 1, __ATOMIC_RELAXED)] = f;
  }
  for (int32_t b = 0; b < B; b++) ef[cur[m.boundary_element(b)]++] = F + b;
  int32_t most = 0;
#pragma omp parallel for num_threads(host_threads()) schedule(static) reduction(max : most)
  for (int32_t e = 0; e < N; e++) {
    std::sort(ef.begin() + deg[e], ef.begin() + deg[e + 1]);
    most = std::max(most, deg[e + 1] - deg[e]);
  }
  inc.most = most;
  return inc;
}

// An EXACT axis normal has one component +-1 and the others +-0. axis < 0: anything else.
struct AxisNormal {
  int  axis;
  bool plus;   // it points along +axis
};
inline AxisNormal exact_axis(const double* n, int ndim) {
  int axis = -1;
  for (int k = 0; k < ndim; k++) {
    if (n[k] == 0.0) continue;
    if ((n[k] != 1.0 && n[k] != -1.0) || axis >= 0) return {-1, false};
    axis = k;
  }
  return {axis, axis >= 0 && n[axis] > 0.0};
}
// Direction code of a unit normal: 2 * axis + (1 if it points along +axis) for an exact axis normal, 6 otherwise. Faces of
// Cartesian meshes all have codes < 6; the kernels evaluate such a face without the rotation into the face frame when a
// whole wavefront shares the code.
inline int direction_code(const double* n, int ndim) {
  const AxisNormal a = exact_axis(n, ndim);
  return a.axis < 0 ? 6 : 2 * a.axis + (a.plus ? 1 : 0);
}

// A structured patch: kPatchSide x kPatchSide same-size quadrilaterals that are kPatchElems CONSECUTIVE elements in
// Morton order (x = bit 0 of the local index), every one with exactly four interior faces in the canonical listing:
// its +x and +y faces are its own (left = the element, normal exactly +e_x / +e_y, ids fbase + 2 t and fbase + 2 t + 1
// for local index t), its -x and -y faces are the +x / +y faces of the elements across (right = the element), all with
// one area. The kernel needs no face records for such a tile: neighbours inside the patch follow from the lane index,
// the 64 elements across its four sides are listed in `halo` ([-x side by j | +x side by j | -y side by i | +y side by
// i]), and an element adds its four fluxes in ascending face id: (-x, -y in the order of the owning neighbours' indices,
// which inside the patch is a function of (i, j) alone -- patch_y_first), then +x, +y.
//
// 3D (find_patches3): 8 x 8 x 4 same-size hexahedra = 256 consecutive elements in Morton order (x = bit 0, y = bit 1, z =
// bit 2 of every triple), six interior faces each, own faces +x / +y / +z with ids fbase + 3 t (+1, +2), 256 cells across
// the six sides ([-x 32 by j + 8 k | +x 32 | -y 32 by i + 8 k | +y 32 | -z 64 by i + 8 j | +z 64]). The three - faces are
// added in the order of the owning neighbours' indices: pairwise "-y before -x" iff ctz(j) >= ctz(i), "-z before -x" iff
// ctz(k) >= ctz(i), "-z before -y" iff ctz(k) >= ctz(j); where BOTH coordinates of a pair are 0 the patch's position in
// the forest decides -- three flag bits per patch (bit 0: y before x, bit 1: z before x, bit 2: z before y).
// IRREGULAR 3D patches (flag 0x800): the same 8 x 8 x 4 block with sides that are not listed that way -- a periodic wrap
// (the cell across has the lower index on a + side, the higher one on a - side), a coarser neighbour across a - side (the
// finer cell lists a hanging face), a wall. Every cell still has exactly one face per side, of the patch's area, with one
// element (or a wall) behind it; what varies per cell is WHO lists each side face and the order of the six ids. The
// planner writes that down per cell (Patch::info: own-side mask, wall mask, the six sides in ascending face id, the ids of
// the first own interior / wall face) and the kernel evaluates each side face in its listed orientation; the interior of
// the block is as in a regular patch. Blocks next to the domain boundary (13 % of the c5 benchmark mesh) become patches.
constexpr int kPatchSide = 16, kPatchElems = 256, kPatchHalo = 64, kPatchHalo3 = 256, kPatchInfoWords = 512;
struct Patch {
  int32_t e0 = 0, fbase = 0, flags = 0;   // 2D: flags bit 0: element 0 adds its -y face before its -x face; 3D: see above
  int32_t dim = 2, nh = kPatchHalo;
  double  area = 0;
  double  volume = 0;        // > 0: every element of the patch has exactly this volume (t8gpu_plan_plain_patch_volumes)
  int32_t halo[kPatchHalo3];
  // IRREGULAR 3D patches (flags 0x800, see irregular_patch3): per cell {sides | walls << 6 | summation order << 12, id of its
  // first own interior face or -1, id of its first wall face or -1}; empty for regular patches
  std::vector<int32_t> info;
};

// ---- what the finders share ------------------------------------------------------------------------------------------------

// Every element is tested as a patch START on its own, in parallel: two patches cannot overlap (the checks pin a start
// to the origin of an aligned block -- element e0 + 1 must be its +x neighbour, e0 + 2 the +y neighbour, and so on through
// the Morton pattern), so there is no scan order to respect. Almost every candidate fails at its first element.
// try_start(e0, pt): is the block of kPatchElems elements from e0 a patch? If so, pt describes it. Patches in element order.
template <class TryStart>
std::vector<Patch> scan_patch_starts(int32_t N, TryStart try_start) {
  const int32_t ncand = N >= kPatchElems ? N - kPatchElems + 1 : 0;
  std::vector<std::vector<Patch>> found(static_cast<size_t>(host_threads()));
#pragma omp parallel num_threads(host_threads())
  {
    std::vector<Patch>& mine = found[static_cast<size_t>(omp_get_thread_num())];
#pragma omp for schedule(static)
    for (int32_t e0 = 0; e0 < ncand; e0++) {
      Patch pt;
      if (try_start(e0, pt)) mine.push_back(pt);
    }
  }
  std::vector<Patch> patches;
  for (auto& v : found)   // (static schedule: ascending e0 overall; the guard is belt and braces -- see above)
    for (const Patch& q : v)
      if (patches.empty() || q.e0 >= patches.back().e0 + kPatchElems) patches.push_back(q);
  return patches;
}

// 0 .. naxes - 1: the normal of interior face f is exactly +e_axis (every further component, where present, zero); -1: anything else
inline int plus_axis(const Mesh& m, int32_t f, int naxes) {
  const AxisNormal a = exact_axis(m.normal(f), m.ndim);
  return a.plus && a.axis < naxes ? a.axis : -1;
}

// Cell t of a regular patch in D dimensions that starts at e0 (pt: the patch so far; cell 0 sets its first face id and its
// area). The canonical listing: exactly 2 D interior faces of the patch's area; for every axis one the element lists itself
// (own[a]: left = the element, normal exactly +e_a, id fbase + D t + a, listed last and in axis order) and one the element
// across lists (far[a]: right = the element, same normal).
template <int D>
bool canonical_cell(const Mesh& m, const Incidence& inc, int32_t e0, int t, Patch& pt, int32_t (&own)[D], int32_t (&far)[D]) {
  const int32_t e = e0 + t;
  if (inc.count(e) != 2 * D) return false;
  const int32_t* fl = inc.faces(e);
  for (int a = 0; a < D; a++) own[a] = far[a] = -1;
  for (int q = 0; q < 2 * D; q++) {
    const int32_t f  = fl[q];
    const int     ax = f < m.F ? plus_axis(m, f, D) : -1;
    if (ax < 0 || m.left(f) == m.right(f)) return false;
    if (m.left(f) == e && own[ax] < 0) own[ax] = f;
    else if (m.right(f) == e && far[ax] < 0) far[ax] = f;
    else return false;
  }
  for (int a = 0; a < D; a++)
    if (own[a] < 0 || far[a] < 0) return false;
  if (t == 0) {
    pt.e0    = e0;
    pt.fbase = own[0];
    pt.area  = m.areas[own[0]];
  }
  for (int q = 0; q < 2 * D; q++)
    if (m.areas[fl[q]] != pt.area) return false;
  for (int a = 0; a < D; a++)
    if (own[a] != pt.fbase + D * t + a || fl[D + a] != own[a]) return false;
  return true;
}

// Is slot s (an owned element or a ghost) outside the block that starts at e0? Across a + side that is all a regular patch
// asks. A - side face whose left element is a ghost is reported -- speed estimate -- by the tile of its right element, which
// a patch cannot do: across a - side the element must be OWNED as well (s < N), and such blocks stay generic tiles.
inline bool outside(int32_t s, int32_t e0) { return s < e0 || s >= e0 + kPatchElems; }
inline bool owned_outside(int32_t s, int32_t e0, int32_t N) { return s < N && outside(s, e0); }

// ---- 2D: 16 x 16 quadrilaterals -----------------------------------------------------------------------------------------------

inline int morton2(int i, int j) {
  int t = 0;
  for (int b = 0; b < 4; b++) t |= ((i >> b) & 1) << (2 * b) | ((j >> b) & 1) << (2 * b + 1);
  return t;
}
inline int ctz_or(int v, int big) { return v == 0 ? big : __builtin_ctz(static_cast<unsigned>(v)); }
// does element (i, j) of a patch add its -y face before its -x face? (the face of the neighbour with the lower index
// first: Morton order of (i, j-1) against (i-1, j)). Element (0, 0) has both neighbours outside: decided per patch.
inline bool patch_y_first(int i, int j) { return ctz_or(j, 4) >= ctz_or(i, 4); }

struct Cells2 {   // (i, j) of local index t: the inverse of morton2
  int i[kPatchElems], j[kPatchElems];
  Cells2() {
    for (int a = 0; a < kPatchSide; a++)
      for (int b = 0; b < kPatchSide; b++) i[morton2(a, b)] = a, j[morton2(a, b)] = b;
  }
};

// Anything unexpected (a hanging face, a wall, a periodic wrap that turns a face round, another face numbering) fails a
// check and leaves the elements to the generic tiles.
inline bool regular_patch2(const Mesh& m, const Incidence& inc, const Cells2& at, int32_t e0, Patch& pt) {
  for (int t = 0; t < kPatchElems; t++) {
    int32_t own[2], far[2];   // the element's +x / +y faces, its -x / -y faces
    if (!canonical_cell<2>(m, inc, e0, t, pt, own, far)) return false;
    const int  i = at.i[t], j = at.j[t];
    const bool yfirst = inc.faces(e0 + t)[0] == far[1];
    bool       ok = true;
    if (t == 0) pt.flags = yfirst ? 1 : 0;
    else ok = yfirst == patch_y_first(i, j);
    const int32_t px = m.right(own[0]), py = m.right(own[1]), mx = m.left(far[0]), my = m.left(far[1]);
    if (i < kPatchSide - 1) ok = ok && px == e0 + morton2(i + 1, j); else { ok = ok && outside(px, e0); pt.halo[16 + j] = px; }
    if (i > 0)              ok = ok && mx == e0 + morton2(i - 1, j); else { ok = ok && owned_outside(mx, e0, m.N); pt.halo[j] = mx; }
    if (j < kPatchSide - 1) ok = ok && py == e0 + morton2(i, j + 1); else { ok = ok && outside(py, e0); pt.halo[48 + i] = py; }
    if (j > 0)              ok = ok && my == e0 + morton2(i, j - 1); else { ok = ok && owned_outside(my, e0, m.N); pt.halo[32 + i] = my; }
    if (!ok) return false;
  }
  return true;
}

inline std::vector<Patch> find_patches2(const Mesh& m, const Incidence& inc) {
  const Cells2 at;
  return scan_patch_starts(m.N, [&](int32_t e0, Patch& pt) { return regular_patch2(m, inc, at, e0, pt); });
}

// ---- 3D: 8 x 8 x 4 hexahedra --------------------------------------------------------------------------------------------------

inline int morton3(int i, int j, int k) {   // 8 x 8 x 4: x bits 0, 3, 6; y bits 1, 4, 7; z bits 2, 5
  int t = 0;
  for (int b = 0; b < 3; b++) t |= ((i >> b) & 1) << (3 * b) | ((j >> b) & 1) << (3 * b + 1);
  for (int b = 0; b < 2; b++) t |= ((k >> b) & 1) << (3 * b + 2);
  return t;
}

struct Cells3 {   // (i, j, k) of local index t: the inverse of morton3
  int i[kPatchElems], j[kPatchElems], k[kPatchElems];
  Cells3() {
    for (int a = 0; a < 8; a++)
      for (int b = 0; b < 8; b++)
        for (int c = 0; c < 4; c++) i[morton3(a, b, c)] = a, j[morton3(a, b, c)] = b, k[morton3(a, b, c)] = c;
  }
};

// What both forms demand of a start before anything else: six faces, and the + neighbours of cell (0, 0, 0) are the block's
// cells (1, 0, 0), (0, 1, 0), (0, 0, 1) = e0 + 1, e0 + 2, e0 + 4, across faces e0 lists itself. Seven of eight elements of a
// uniform region fail this, from the face -> element pairs alone (8 bytes per face, against 40 once normals and areas are read).
inline bool may_start3(const Mesh& m, const Incidence& inc, int32_t e0) {
  if (inc.count(e0) != 6) return false;
  const int32_t* fl = inc.faces(e0);
  unsigned       got = 0;
  for (int q = 0; q < 6; q++) {
    const int32_t f = fl[q];
    if (f >= m.F || m.left(f) != e0) continue;
    const int32_t d = m.right(f) - e0;
    if (d == 1 || d == 2 || d == 4) got |= static_cast<unsigned>(d);
  }
  return got == 7u;
}

// Same policy as regular_patch2: every expectation is checked per element against the arrays.
inline bool regular_patch3(const Mesh& m, const Incidence& inc, const Cells3& at, int32_t e0, Patch& pt) {
  for (int t = 0; t < kPatchElems; t++) {
    int32_t own[3], far[3];
    if (!canonical_cell<3>(m, inc, e0, t, pt, own, far)) return false;
    const int32_t* fl = inc.faces(e0 + t);
    const int      i = at.i[t], j = at.j[t], k = at.k[t];
    // position of every - face among the three (ascending face id = ascending index of the owning neighbour)
    int pos[3] = {0, 0, 0};
    for (int a = 0; a < 3; a++)
      for (int q = 0; q < 3; q++)
        if (fl[q] == far[a]) pos[a] = q;
    const bool yx = pos[1] < pos[0], zx = pos[2] < pos[0], zy = pos[2] < pos[1];
    if (t == 0) pt.flags = (yx ? 1 : 0) | (zx ? 2 : 0) | (zy ? 4 : 0);
    // the rule, with the patch's flags where both coordinates of a pair are 0 (their ctz is then the forest's business)
    const bool ryx = (i == 0 && j == 0) ? (pt.flags & 1) != 0 : ctz_or(j, 8) >= ctz_or(i, 8);
    const bool rzx = (i == 0 && k == 0) ? (pt.flags & 2) != 0 : ctz_or(k, 8) >= ctz_or(i, 8);
    const bool rzy = (j == 0 && k == 0) ? (pt.flags & 4) != 0 : ctz_or(k, 8) >= ctz_or(j, 8);
    bool ok = yx == ryx && zx == rzx && zy == rzy;
    const int32_t pl[3] = {m.right(own[0]), m.right(own[1]), m.right(own[2])};
    const int32_t mi[3] = {m.left(far[0]), m.left(far[1]), m.left(far[2])};
    if (i < 7) ok = ok && pl[0] == e0 + morton3(i + 1, j, k); else { ok = ok && outside(pl[0], e0); pt.halo[32 + j + 8 * k] = pl[0]; }
    if (i > 0) ok = ok && mi[0] == e0 + morton3(i - 1, j, k); else { ok = ok && owned_outside(mi[0], e0, m.N); pt.halo[j + 8 * k] = mi[0]; }
    if (j < 7) ok = ok && pl[1] == e0 + morton3(i, j + 1, k); else { ok = ok && outside(pl[1], e0); pt.halo[96 + i + 8 * k] = pl[1]; }
    if (j > 0) ok = ok && mi[1] == e0 + morton3(i, j - 1, k); else { ok = ok && owned_outside(mi[1], e0, m.N); pt.halo[64 + i + 8 * k] = mi[1]; }
    if (k < 3) ok = ok && pl[2] == e0 + morton3(i, j, k + 1); else { ok = ok && outside(pl[2], e0); pt.halo[192 + i + 8 * j] = pl[2]; }
    if (k > 0) ok = ok && mi[2] == e0 + morton3(i, j, k - 1); else { ok = ok && owned_outside(mi[2], e0, m.N); pt.halo[128 + i + 8 * j] = mi[2]; }
    if (!ok) return false;
  }
  return true;
}

// The irregular form (see struct Patch): tried where the regular checks fail. Sides are numbered like t8code faces
// (0 -x, 1 +x, 2 -y, 3 +y, 4 -z, 5 +z), which is also the order in which an element lists its own faces.
inline bool irregular_patch3(const Mesh& m, const Incidence& inc, const Cells3& at, int32_t e0, Patch& pt) {
  pt.e0    = e0;
  pt.fbase = 0;
  pt.flags = 0x800;
  int32_t info[3 * kPatchElems];   // (nearly every candidate fails at its first cell: nothing is allocated before it passes)
  const int ext[3] = {8, 8, 4};
  for (int t = 0; t < kPatchElems; t++) {
    const int32_t e = e0 + t;
    if (inc.count(e) != 6) return false;
    const int32_t* fl      = inc.faces(e);
    const int      ijk[3]  = {at.i[t], at.j[t], at.k[t]};
    uint32_t       own = 0, wall = 0, order = 0, seen = 0;
    int32_t        first_id = -1, wall_first = -1, id_of[6] = {-1, -1, -1, -1, -1, -1};
    for (int q = 0; q < 6; q++) {
      const int32_t    f       = fl[q];
      const bool       is_wall = f >= m.F;
      const int32_t    l = inc.side(f, 0), r = inc.side(f, 1);
      const AxisNormal n = exact_axis(m.normal(f), 3);
      const int        axis = n.axis;
      if (axis < 0) return false;
      if (t == 0 && q == 0) pt.area = m.areas[f];
      if (m.areas[f] != pt.area) return false;
      if ((l == e) == (r == e)) return false;
      const bool mine_ = l == e;   // the element lists the face itself
      const bool plus = mine_ == n.plus;   // (the normal points away from the listing element)
      const int  sd   = 2 * axis + (plus ? 1 : 0);
      if (seen & (1u << sd)) return false;
      seen |= 1u << sd;
      order |= static_cast<uint32_t>(sd) << (3 * q);
      id_of[sd] = f;
      if (mine_) {
        own |= 1u << sd;
        if (is_wall) {
          wall |= 1u << sd;
          if (wall_first < 0) wall_first = f;
        } else if (first_id < 0) {
          first_id = f;
        }
      }
      const int32_t nb     = is_wall ? e : (mine_ ? r : l);
      const bool    inside = plus ? ijk[axis] < ext[axis] - 1 : ijk[axis] > 0;
      if (inside) {   // the interior of the block is as in a regular patch
        int nijk[3] = {ijk[0], ijk[1], ijk[2]};
        nijk[axis] += plus ? 1 : -1;
        if (is_wall || mine_ != plus || nb != e0 + morton3(nijk[0], nijk[1], nijk[2])) return false;
      } else {
        if (!is_wall && !outside(nb, e0)) return false;
        if (!mine_ && nb >= m.N) return false;   // (a face listed by a ghost is reported by its right element's tile: not a patch)
        const int u = axis == 0 ? ijk[1] : ijk[0], v = axis == 2 ? ijk[1] : ijk[2];
        const int base = axis == 0 ? (plus ? 32 : 0) : (axis == 1 ? (plus ? 96 : 64) : (plus ? 192 : 128));
        pt.halo[base + u + 8 * v] = nb;
      }
    }
    // an element lists its own faces in side order, interior faces and walls each with consecutive ids
    const uint32_t own_int = own & ~wall;
    for (int sd = 0; sd < 6; sd++) {
      if (own_int & (1u << sd)) {
        if (id_of[sd] != first_id + __builtin_popcount(own_int & ((1u << sd) - 1u))) return false;
      } else if (wall & (1u << sd)) {
        if (id_of[sd] != wall_first + __builtin_popcount(wall & ((1u << sd) - 1u))) return false;
      }
    }
    info[3 * t]     = static_cast<int32_t>(own | (wall << 6) | (order << 12));
    info[3 * t + 1] = first_id;
    info[3 * t + 2] = wall_first;
  }
  pt.info.assign(info, info + 3 * kPatchElems);
  return true;
}

// regular: blocks in the regular form where they pass its checks; irregular: the other form where they do not (with
// regular = false: every patch in the irregular form -- one kernel, one launch)
inline std::vector<Patch> find_patches3(const Mesh& m, const Incidence& inc, bool regular, bool irregular) {
  if (m.ndim != 3) return {};
  const Cells3 at;
  return scan_patch_starts(m.N, [&](int32_t e0, Patch& pt) {
    if (!may_start3(m, inc, e0)) return false;
    pt.dim = 3;
    pt.nh  = kPatchHalo3;
    return (regular && regular_patch3(m, inc, at, e0, pt)) || (irregular && irregular_patch3(m, inc, at, e0, pt));
  });
}

// ---- the patches of a mesh ----------------------------------------------------------------------------------------------------

// Drops the patches that hold a cell with an open boundary face: the patch kernels know walls only, such cells run through
// the generic tiles (patches are disjoint aligned blocks, so this leaves exactly the blocks a finder that rejected open faces
// would have found).
inline std::vector<Patch> drop_open_patches(std::vector<Patch> patches, const Mesh& m) {
  if (!m.kinds || patches.empty()) return patches;
  std::vector<uint8_t> open(static_cast<size_t>(m.N), 0);
  for (int32_t b = 0; b < m.B; b++)
    if (m.kinds[b] != 0) open[m.boundary_element(b)] = 1;
  auto has_open_cell = [&open](const Patch& pt) {
    return std::find(open.begin() + pt.e0, open.begin() + pt.e0 + kPatchElems, 1) != open.begin() + pt.e0 + kPatchElems;
  };
  patches.erase(std::remove_if(patches.begin(), patches.end(), has_open_cell), patches.end());
  return patches;
}

// The patches of the mesh, found from the reference-format arrays alone, in element order. want bit 0: 2D patches, bit 1: 3D
// patches (where there are no 2D ones: a plan holds one kind), bit 3: irregular 3D patches too, bit 4: no regular 3D ones.
inline std::vector<Patch> find_patches(const Mesh& m, const Incidence& inc, int want) {
  std::vector<Patch> patches;
  if (want & 1) patches = drop_open_patches(find_patches2(m, inc), m);
  if ((want & 2) && patches.empty()) patches = drop_open_patches(find_patches3(m, inc, !(want & 16), (want & 8) != 0), m);
  return patches;
}

}  // namespace

#endif  // T8GPU_TILE_PATCHES_HPP
