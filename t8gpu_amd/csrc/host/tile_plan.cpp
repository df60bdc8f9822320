// tile_plan.cpp -- the face sort / permute + element-window tiling pre-pass of the fused kernels.
//
// Runs once per connectivity rebuild (where the reference runs compute_connectivity_information,
// t8gpu/mesh/mesh_manager.inl:333-481), on the host, from the reference-format arrays
// (face_neighbors, face_normals, face_surfaces). Output: for every tile (a contiguous SFC range of
// owned elements, i.e. a compact window in space)
//   * halo ids    : slots of the outside elements (other tiles' or ghost mirrors) its faces touch,
//   * tile faces  : every face with a side in the tile, re-laid out contiguously (coalesced loads):
//                   packed tile-local (l, r) indices, {nx, ny, nz, area}, original face id,
//   * element CSR : per owned element the tile-local faces it sums, with the sign of its side.
// A face cut by a tile boundary is listed in both tiles (flux evaluated twice, applied to the own
// side only): no atomics, no flux planes in HBM, bitwise-reproducible sums (CSR order = face order).
//
// The phases, in the order build() runs them (its lap() labels in quotes):
//   element_faces        "element -> faces"        faces of every owned element (tile_patches.hpp: Incidence)
//   find_patches         "patches"                 structured blocks that become tiles of their own (tile_patches.hpp)
//   greedy_tiling        "greedy tiling"           elem_off: the other elements cut into tiles under the three caps
//   size_tiles           "per-tile lists (sizes)"  every tile's face and halo list (TileLists), halo_off, face_off, the maxima
//   geometry_dictionary  "geometry dictionary"     geo_table and every original face's row | direction code << 13
//   fill_tiles           "per-tile lists"          halo_ids, face records, CSR entries (fill_patch_tile / fill_generic_tile)
//   order_tiles          "tile classes"            tile_order: deep | near | ghost-reading, patches first inside each
//   ell_rows             "ELL rows"                fixed-width copy of the generic tiles' element face lists
//
// Host-only: covered by the CPU test-suite through a numpy interpreter of the plan, and byte for byte by
// tests/test_tile_plan_digests.py.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <unordered_set>
#include <vector>

#include "host_threads.hpp"
#include "t8gpu_host.h"
#include "tile_patches.hpp"

namespace {

struct TilePlan {
  int32_t N = 0, G = 0, F = 0, B = 0, ndim = 3, tmax = 256, fcap = 512;
  int32_t max_halo = 0, max_faces = 0, max_elems = 0, n_interior = 0, max_slots = 0, n_deep = 0;
  std::vector<int32_t>  elem_off, halo_off, face_off;  // [ntiles + 1]
  // (uvector: sized once, then written completely by the parallel per-tile loops -- no value-initialising pass)
  uvector<int32_t>      halo_ids;                      // slots
  uvector<uint32_t>     face_lr;                       // l | r << 16 (tile-local; r >= 0xFFF0: boundary face, boundary_code)
  uvector<double>       face_geo;                      // [nfaces][4] = nx, ny, nz, area
  uvector<int32_t>      face_orig;                     // original face id if this tile reports its speed, else -1
  std::vector<int32_t>  csr_off;                       // [N + 1]
  uvector<uint16_t>     csr_ent;                       // tile-local face | 0x8000 if the element is the RIGHT side
  std::vector<int32_t>  tile_order;                    // interior tiles first, then tiles that read ghost slots
  // compressed forms used by the pipelined kernel
  int32_t lecap = 512;                                 // max own + halo elements per tile
  int32_t ell_width = 0;                               // padded per-element face-list width (multiple of 8)
  uvector<uint16_t>     ell;                           // [ell rows][ell_width], 0xFFFF = padding (generic tiles' elements only)
  std::vector<int32_t>  ell_row0;                      // [ntiles + 1] first ELL row of each tile
  uvector<uint16_t>     geo_idx;                       // per tile face: row of geo_table (13 bits) | direction code << 13
                                                       // (empty if more than 8191 distinct rows)
  std::vector<double>   geo_table;                     // [n_geo][12]: n, area, t1, 0, t2, 0
  // structured patches (tile_patches.hpp): tiles the patch kernel evaluates without face records
  int32_t want_patches = 0;                            // find_patches' `want` bits
  bool    skip_face_geo = false;                       // leave face_geo empty when the plan has a geometry dictionary
  bool    two_classes = false;                         // no deep / near-boundary split of the interior tiles (flag 32)
  bool    open_faces = false;                          // some boundary face is not a wall
  bool    farfield_faces = false;                      // some boundary face is a far-field face
  std::vector<Patch>   patches;                        // in element order
  std::vector<int32_t> tile_patch;                     // [ntiles] index into patches, or -1 (generic tile)
  int32_t n_patch_class[3] = {0, 0, 0};                // leading patch tiles of the deep / near / ghost-reading class
  int32_t n_irregular_class[3] = {0, 0, 0};            // ... the last so many of which are irregular patches
  int32_t ntiles() const { return static_cast<int32_t>(elem_off.size()) - 1; }
  bool    irregular_tile(int32_t t) const { return tile_patch[t] >= 0 && !patches[tile_patch[t]].info.empty(); }
};

// face_lr code of boundary face b (the r half): 0xFFFF wall, 0xFFFE outflow, 0xFFF0 + k inflow state k, 0xFFF8 + k far field k.
// The kernels decode it in one place (fused_common.hpp: boundary_side).
inline uint32_t boundary_code(const Mesh& m, int32_t b) {
  const int k = m.kinds ? m.kinds[b] : 0;
  if (k >= T8GPU_BOUNDARY_FARFIELD) return 0xFFF8u + static_cast<uint32_t>(k - T8GPU_BOUNDARY_FARFIELD);   // far field k
  return k == 0 ? 0xFFFFu : (k == 1 ? 0xFFFEu : 0xFFF0u + static_cast<uint32_t>(k - 2));
}

// Small open-addressing hash set / map of int32 keys, emptied in O(1) by moving to the next generation: the faces / halo
// elements of the tile under construction (greedy tiling) and the face -> position, element -> slot maps of a tile's lists.
struct StampSet {
  std::vector<int32_t> key, gen, val;
  int32_t              cur = 0;
  uint32_t             mask;
  int                  shift;
  explicit StampSet(int log2cap)
      : key(size_t(1) << log2cap), gen(size_t(1) << log2cap, -1), val(size_t(1) << log2cap), mask((1u << log2cap) - 1u), shift(32 - log2cap) {}
  void clear() { cur++; }
  uint32_t slot(int32_t k) const {   // where k is, or the free slot where it would go
    uint32_t h = (static_cast<uint32_t>(k) * 2654435761u) >> shift;
    while (gen[h] == cur && key[h] != k) h = (h + 1) & mask;
    return h;
  }
  bool contains(int32_t k) const { return gen[slot(k)] == cur; }
  bool insert(int32_t k, int32_t v = 0) {   // true: was not there
    const uint32_t h = slot(k);
    if (gen[h] == cur) return false;
    gen[h] = cur;
    key[h] = k;
    val[h] = v;
    return true;
  }
  int32_t at(int32_t k) const { return val[slot(k)]; }   // (k must be there)
};

// log2 of the capacity of the per-thread StampSets: >= 4 x the entries a tile can hold (a tile ends at fcap faces / lecap slots,
// plus one element's worth; `most` = the faces of one element, which touch twice as many halo elements)
int stamp_capacity_log2(int32_t fcap, int32_t lecap, int32_t most) {
  int log2cap = 12;
  while (log2cap < 30 && (int64_t(1) << log2cap) < 4 * (int64_t(std::max(fcap, lecap)) + 2 * int64_t(most) + 64)) log2cap++;
  return log2cap;
}

// patch_at[e]: the patch that starts at element e, or -1
std::vector<int32_t> patch_starts(const std::vector<Patch>& patches, int32_t N) {
  std::vector<int32_t> patch_at(static_cast<size_t>(N) + 1, -1);
  for (size_t k = 0; k < patches.size(); k++) patch_at[patches[k].e0] = static_cast<int32_t>(k);
  return patch_at;
}

// elem_off of the tiling. Greedy: grow the element range while elements <= tmax, distinct faces <= fcap and own + halo
// elements <= lecap (the kernel's LDS window). The halo count is tracked incrementally: an element that
// joins the tile stops being halo, its neighbours outside the range become halo.
// A patch is a tile of its own, so the stretches of other elements between patches are tiled independently of each other:
// in parallel, one run at a time. Long stretches are cut every kRunCut elements as well (a fixed rule: the tiling does not
// depend on the number of threads); the faces / halo elements of the tile under construction sit in two small hash sets.
std::vector<int32_t> greedy_tiling(const Incidence& inc, const std::vector<int32_t>& patch_at, int32_t tmax, int32_t fcap, int32_t lecap,
                                   int log2cap) {
  constexpr int32_t kRunCut = 1 << 16;
  const int32_t     N = static_cast<int32_t>(inc.deg.size()) - 1;
  std::vector<std::pair<int32_t, int32_t>> runs;
  for (int32_t e = 0; e < N;) {
    if (patch_at[e] >= 0) {
      e += kPatchElems;
      continue;
    }
    const int32_t start = e;
    while (e < N && patch_at[e] < 0 && e - start < kRunCut) e++;
    runs.push_back({start, e});
  }
  std::vector<std::vector<int32_t>> ends(runs.size());
#pragma omp parallel num_threads(host_threads())
  {
    StampSet faces(log2cap), halo(log2cap);
#pragma omp for schedule(dynamic, 1)
    for (int64_t r = 0; r < static_cast<int64_t>(runs.size()); r++) {
      int32_t       e = runs[r].first;
      const int32_t stop = runs[r].second;
      while (e < stop) {
        faces.clear();
        halo.clear();
        int32_t nf = 0, nh = 0;
        const int32_t start = e;
        while (e < stop && e - start < tmax) {
          int32_t add = 0, dh = halo.contains(e) ? -1 : 0;
          for (int32_t j = inc.deg[e]; j < inc.deg[e + 1]; j++) {
            if (faces.insert(inc.ef[j])) add++;   // (inserted even if e is rejected below: the tile ends there, the sets with it)
            for (int w = 0; w < 2; w++) {
              const int32_t o = inc.side(inc.ef[j], w);
              if (o >= 0 && (o < start || o > e) && halo.insert(o)) dh++;
            }
          }
          if (e > start && (nf + add > fcap || (e - start + 1) + nh + dh > lecap)) break;
          nf += add;
          nh += dh;
          e++;
        }
        ends[r].push_back(e);
      }
    }
  }
  std::vector<int32_t> elem_off(1, 0);
  size_t               r = 0;
  for (int32_t e = 0; e < N;) {   // patches and runs alternate in element order
    if (patch_at[e] >= 0) {
      e += kPatchElems;
      elem_off.push_back(e);
    } else {
      elem_off.insert(elem_off.end(), ends[r].begin(), ends[r].end());
      e = runs[r++].second;
    }
  }
  return elem_off;
}

// What the sizing pass keeps for the fill pass (sorting the lists twice was 40 % of the fill) and for order_tiles
struct TileLists {
  std::vector<std::vector<int32_t>> tfs, halos;    // per tile: its faces / the outside elements they touch, ascending
  std::vector<uint8_t>              reads_ghost;   // per tile: some halo element is a ghost
};

// The lists of tile t. A patch tile has no face records; its halo is the elements across its sides in the patch kernel's fixed
// order. A generic tile: distinct faces / outside elements through a hash set, then sorted (half the entries of the raw lists
// are duplicates).
void tile_lists(const TilePlan& P, const Incidence& inc, int32_t t, std::vector<int32_t>& tf, std::vector<int32_t>& halo, StampSet& set) {
  const int32_t e0 = P.elem_off[t], e1 = P.elem_off[t + 1];
  tf.clear();
  if (P.tile_patch[t] >= 0) {
    const Patch& pt = P.patches[P.tile_patch[t]];
    halo.assign(pt.halo, pt.halo + pt.nh);
    return;
  }
  set.clear();
  for (int32_t j = inc.deg[e0]; j < inc.deg[e1]; j++)
    if (set.insert(inc.ef[j])) tf.push_back(inc.ef[j]);
  std::sort(tf.begin(), tf.end());
  halo.clear();
  set.clear();
  for (int32_t f : tf)
    for (int w = 0; w < 2; w++) {
      const int32_t s = inc.side(f, w);
      if (s >= 0 && (s < e0 || s >= e1) && set.insert(s)) halo.push_back(s);
    }
  std::sort(halo.begin(), halo.end());
}

// One sizing pass over the tiling P.elem_off: tile_patch, every tile's lists, halo_off / face_off (prefix sums) and the maxima.
// Tiles are independent: the pass runs over them in parallel.
TileLists size_pass(TilePlan& P, const Incidence& inc, const std::vector<int32_t>& patch_at, int log2cap) {
  const int32_t ntiles = P.ntiles(), N = P.N;
  TileLists     L;
  P.halo_off.assign(static_cast<size_t>(ntiles) + 1, 0);
  P.face_off.assign(static_cast<size_t>(ntiles) + 1, 0);
  P.tile_patch.assign(ntiles, -1);
  for (int32_t t = 0; t < ntiles; t++) P.tile_patch[t] = patch_at[P.elem_off[t]];
  L.reads_ghost.assign(ntiles, 0);
  L.tfs.assign(ntiles, {});
  L.halos.assign(ntiles, {});
#pragma omp parallel num_threads(host_threads())
  {
    StampSet set(log2cap);
#pragma omp for schedule(dynamic, 64)
    for (int32_t t = 0; t < ntiles; t++) {
      std::vector<int32_t>&tf = L.tfs[t], &halo = L.halos[t];
      tile_lists(P, inc, t, tf, halo, set);
      // (an irregular patch keeps its per-cell words where a generic tile keeps face records: 512 entries of face_lr / face_orig)
      P.face_off[t + 1] = P.irregular_tile(t) ? kPatchInfoWords : static_cast<int32_t>(tf.size());
      P.halo_off[t + 1] = static_cast<int32_t>(halo.size());
      L.reads_ghost[t]  = !halo.empty() && *std::max_element(halo.begin(), halo.end()) >= N;
    }
  }
  P.max_halo = P.max_faces = P.max_elems = P.max_slots = 0;
  for (int32_t t = 0; t < ntiles; t++) {
    const int32_t ne = P.elem_off[t + 1] - P.elem_off[t], nh = P.halo_off[t + 1], nf = P.face_off[t + 1];
    if (P.tile_patch[t] < 0) {   // the maxima size the generic kernels' LDS windows: patch tiles are not theirs
      P.max_halo  = std::max(P.max_halo, nh);
      P.max_faces = std::max(P.max_faces, nf);
      P.max_elems = std::max(P.max_elems, ne);
      P.max_slots = std::max(P.max_slots, ne + nh);
    }
    P.halo_off[t + 1] += P.halo_off[t];
    P.face_off[t + 1] += P.face_off[t];
  }
  return L;
}

// The tiling with every generic tile of more than lecap own + halo elements halved until it fits (per greedy tile, in parallel)
std::vector<int32_t> halve_oversized(const std::vector<int32_t>& elem_off, const Incidence& inc, const std::vector<int32_t>& patch_at,
                                     int32_t lecap) {
  const int32_t nt0 = static_cast<int32_t>(elem_off.size()) - 1;
  std::vector<std::vector<int32_t>> cuts(nt0);   // extra offsets inside a greedy tile (almost always none)
#pragma omp parallel num_threads(host_threads())
  {
    std::vector<int32_t>                     out;
    std::vector<std::pair<int32_t, int32_t>> work;
#pragma omp for schedule(dynamic, 64)
    for (int32_t t = 0; t < nt0; t++) {
      if (patch_at[elem_off[t]] >= 0) continue;
      work.assign(1, {elem_off[t], elem_off[t + 1]});
      while (!work.empty()) {
        const auto [a, b] = work.back();
        work.pop_back();
        out.clear();
        for (int32_t j = inc.deg[a]; j < inc.deg[b]; j++)
          for (int w = 0; w < 2; w++) {
            const int32_t o = inc.side(inc.ef[j], w);
            if (o >= 0 && (o < a || o >= b)) out.push_back(o);
          }
        std::sort(out.begin(), out.end());
        const int32_t nh = static_cast<int32_t>(std::unique(out.begin(), out.end()) - out.begin());
        if ((b - a) + nh > lecap && b - a > 1) {
          const int32_t m = a + (b - a) / 2;
          work.push_back({m, b});
          work.push_back({a, m});
        } else if (b != elem_off[t + 1]) {
          cuts[t].push_back(b);
        }
      }
    }
  }
  std::vector<int32_t> off(1, 0);
  for (int32_t t = 0; t < nt0; t++) {
    off.insert(off.end(), cuts[t].begin(), cuts[t].end());
    off.push_back(elem_off[t + 1]);
  }
  return off;
}

// A tile must fit the kernel's LDS window: own + halo elements <= lecap. The greedy loop counts the halo as it goes, so this
// holds by construction; the sizing pass checks it on the exact lists it builds anyway, and only if a tile should ever exceed
// the window are the offenders halved and the lists sized again.
TileLists size_tiles(TilePlan& P, const Incidence& inc, const std::vector<int32_t>& patch_at, int log2cap) {
  TileLists L = size_pass(P, inc, patch_at, log2cap);
  if (P.max_slots > P.lecap) {
    P.elem_off = halve_oversized(P.elem_off, inc, patch_at, P.lecap);
    L          = size_pass(P, inc, patch_at, log2cap);
  }
  return L;
}

// Dictionary of the distinct {nx, ny, nz, area} tuples (exact bit patterns) of the mesh's faces: Cartesian AMR meshes
// have a few dozen, so a tile face carries a 2-byte index instead of 4 float_type values. Built over the ORIGINAL faces
// (every thread collects the distinct tuples of its share; on a curved mesh each gives up after 8192). Fills geo_table and
// returns every original face's row | direction code << 13, which the fill pass copies to the tile faces; both stay empty if
// there are more than 8191 rows.
uvector<uint16_t> geometry_dictionary(const Mesh& m, std::vector<double>& geo_table) {
  using Key = std::array<uint64_t, 4>;   // (compared word by word: the order of the table's rows)
  struct KeyHash {
    size_t operator()(const Key& k) const {
      uint64_t h = 0x9E3779B97F4A7C15ull;
      for (int i = 0; i < 4; i++) h = (h ^ k[i]) * 0xff51afd7ed558ccdull + (h >> 29);
      return static_cast<size_t>(h);
    }
  };
  const int64_t nof = static_cast<int64_t>(m.F) + m.B;
  auto key_of = [&m](int64_t f, double* g) {
    for (int k = 0; k < 3; k++) g[k] = k < m.ndim ? m.normals[static_cast<size_t>(m.ndim) * f + k] : 0.0;
    g[3] = m.areas[f];
    Key key;
    std::memcpy(key.data(), g, 32);
    return key;
  };
  constexpr size_t kMaxRows = 8191;   // 13 bits of row index: the upper 3 bits of geo_idx carry the direction code
  std::vector<Key> uniq;
  bool             too_many = false;
  // (a few dozen tuples repeat millions of times: a small direct-mapped cache of recent keys answers nearly every face)
  constexpr int kCache = 256;
  auto slot_of = [](const Key& k) {
    const uint64_t h = (k[0] ^ (k[1] * 3) ^ (k[2] * 7) ^ (k[3] * 13)) * 0x9E3779B97F4A7C15ull;
    return static_cast<int>(h >> 56);
  };
#pragma omp parallel num_threads(host_threads())
  {
    std::unordered_set<Key, KeyHash> set;
    std::vector<Key>                 cache(kCache);
    std::vector<uint8_t>             full(kCache, 0);
#pragma omp for schedule(static) nowait
    for (int64_t f = 0; f < nof; f++) {
      if (set.size() > kMaxRows) continue;
      double    g[4];
      const Key key = key_of(f, g);
      const int c   = slot_of(key);
      if (full[c] && key == cache[c]) continue;
      cache[c] = key;
      full[c]  = 1;
      set.insert(key);
    }
#pragma omp critical
    {
      if (set.size() > kMaxRows) too_many = true;
      if (!too_many) uniq.insert(uniq.end(), set.begin(), set.end());
    }
  }
  if (!too_many) {
    std::sort(uniq.begin(), uniq.end());   // (sorted: the table does not depend on the order of discovery)
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    too_many = uniq.size() > kMaxRows;
  }
  uvector<uint16_t> orig_gidx;
  if (too_many || nof == 0) return orig_gidx;
  // table row = {nx, ny, nz, area, t1x, t1y, t1z, 0, t2x, t2y, t2z, 0}: the face frame (the reference
  // rebuilds it per face and stage, kernels.cu:174-193) is computed once per distinct normal
  geo_table.assign(uniq.size() * 12, 0.0);
  for (size_t i = 0; i < uniq.size(); i++) {
    double* row = &geo_table[12 * i];
    std::memcpy(row, uniq[i].data(), 32);
    const double* n = row;
    // (flux_math.hpp: face_basis, bit for bit -- its departure from the reference included: inside the cone |r|^2 < 2^-6 around
    //  +-(1, -1, 1) / sqrt 3, where the seed (ny, nz, -nx) is nearly antiparallel to n, the second seed (nz, -nx, ny))
    double t1[3];
    auto project = [n, &t1](double s0, double s1, double s2) {
      t1[0] = s0, t1[1] = s1, t1[2] = s2;
      const double dp = n[0] * t1[0] + n[1] * t1[1] + n[2] * t1[2];
      for (int k = 0; k < 3; k++) t1[k] -= dp * n[k];
      return t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2];
    };
    double r2 = project(n[1], n[2], -n[0]);
    if (r2 < 0.015625) r2 = project(n[2], -n[0], n[1]);
    const double nrm = std::sqrt(r2);
    for (int k = 0; k < 3; k++) row[4 + k] = t1[k] / nrm;
    row[8]  = n[1] * row[6] - n[2] * row[5];
    row[9]  = n[2] * row[4] - n[0] * row[6];
    row[10] = n[0] * row[5] - n[1] * row[4];
  }
  orig_gidx.resize(static_cast<size_t>(nof));
#pragma omp parallel num_threads(host_threads())
  {
    std::vector<Key>      cache(kCache);
    std::vector<uint32_t> value(kCache, 0xFFFFFFFFu);   // row | code << 13 of the cached key
#pragma omp for schedule(static)
    for (int64_t f = 0; f < nof; f++) {
      double    g[4];
      const Key key = key_of(f, g);
      const int c   = slot_of(key);
      if (value[c] == 0xFFFFFFFFu || !(key == cache[c])) {
        const unsigned row  = static_cast<unsigned>(std::lower_bound(uniq.begin(), uniq.end(), key) - uniq.begin());
        const unsigned code = static_cast<unsigned>(direction_code(g, 3));
        cache[c] = key;
        value[c] = row | (code << 13);
      }
      orig_gidx[f] = static_cast<uint16_t>(value[c]);
    }
  }
  return orig_gidx;
}

// A patch tile: no face records and no CSR entries that anybody reads. An irregular patch keeps its per-cell words where a
// generic tile keeps face records: face_lr[q0 + c] = sides | walls | order, face_orig[q0 + c] / [q0 + 256 + c] = first own
// interior / wall id.
void fill_patch_tile(TilePlan& P, const Incidence& inc, int32_t t) {
  for (int32_t j = inc.deg[P.elem_off[t]]; j < inc.deg[P.elem_off[t + 1]]; j++) P.csr_ent[j] = static_cast<uint16_t>(0xFFFFu);   // (never read)
  if (!P.irregular_tile(t)) return;
  const std::vector<int32_t>& info = P.patches[P.tile_patch[t]].info;
  const size_t                q0 = P.face_off[t];
  for (int c = 0; c < kPatchElems; c++) {
    P.face_lr[q0 + c]                 = static_cast<uint32_t>(info[3 * c]);
    P.face_lr[q0 + kPatchElems + c]   = 0u;
    P.face_orig[q0 + c]               = info[3 * c + 1];
    P.face_orig[q0 + kPatchElems + c] = info[3 * c + 2];
  }
  // (face_geo / geo_idx: sized in fill_tiles where the plan has them)
  if (!P.face_geo.empty()) std::fill_n(P.face_geo.begin() + 4 * q0, 4 * kPatchInfoWords, 0.0);
  if (!P.geo_idx.empty()) std::fill_n(P.geo_idx.begin() + q0, kPatchInfoWords, static_cast<uint16_t>(0));
}

// Per-thread scratch of fill_generic_tile
struct FillScratch {
  std::vector<int32_t> order;
  std::vector<uint8_t> codes;
  StampSet             face_at, slot_at;   // face id -> position in the tile's face list, outside element -> halo index
  explicit FillScratch(int log2cap) : face_at(log2cap), slot_at(log2cap) {}
};

// A generic tile: its faces tf become face records and CSR entries; halo (the outside elements they touch, ascending) gives
// the tile-local indices.
void fill_generic_tile(TilePlan& P, const Mesh& m, const Incidence& inc, int32_t t, const std::vector<int32_t>& tf,
                       const std::vector<int32_t>& halo, const uvector<uint16_t>& orig_gidx, FillScratch& s) {
  const int32_t e0 = P.elem_off[t], e1 = P.elem_off[t + 1], ne = e1 - e0;
  s.slot_at.clear();
  for (size_t j = 0; j < halo.size(); j++) s.slot_at.insert(halo[j], static_cast<int32_t>(j));
  auto loc = [&](int32_t el) -> uint32_t {   // tile-local index of an own or halo element
    if (el >= e0 && el < e1) return static_cast<uint32_t>(el - e0);
    return static_cast<uint32_t>(ne + s.slot_at.at(el));
  };
  // Layout of the tile's faces: ascending original id, then inside every block of 256 (one pass of the two-pass
  // kernels = the faces one lane index sees) a stable sort by direction code, so that a wavefront's 64 faces
  // mostly share one direction. The per-element lists below keep ascending original order (only the positions
  // they point at move, and never across a block), so every kernel sums in the same order as before.
  const size_t nft = tf.size();
  s.order.resize(nft);
  s.codes.resize(nft);
  for (size_t j = 0; j < nft; j++) s.codes[j] = static_cast<uint8_t>(direction_code(m.normal(tf[j]), m.ndim));
  for (size_t b = 0; b < nft; b += 256) {   // stable counting sort by code (0..6) inside the block
    const size_t hi = std::min(nft, b + 256);
    size_t       at[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t j = b; j < hi; j++) at[s.codes[j] + 1]++;
    for (int k = 1; k < 8; k++) at[k] += at[k - 1];
    for (size_t j = b; j < hi; j++) s.order[b + at[s.codes[j]]++] = static_cast<int32_t>(j);
  }
  s.face_at.clear();
  for (size_t j = 0; j < nft; j++) s.face_at.insert(tf[s.order[j]], static_cast<int32_t>(j));
  const bool fill_geo = !P.face_geo.empty(), have_dict = !orig_gidx.empty();
  size_t     q = P.face_off[t];
  for (size_t jj = 0; jj < nft; jj++, q++) {
    const int32_t  f = tf[s.order[jj]];
    const int32_t  l = inc.side(f, 0), r = inc.side(f, 1);
    const uint32_t ll = loc(l), rr = r < 0 ? boundary_code(m, f - m.F) : loc(r);
    P.face_lr[q] = ll | (rr << 16);
    if (fill_geo) {
      for (int k = 0; k < 3; k++) P.face_geo[4 * q + k] = k < m.ndim ? m.normal(f)[k] : 0.0;
      P.face_geo[4 * q + 3] = m.areas[f];
    }
    if (have_dict) P.geo_idx[q] = orig_gidx[f];
    // the tile owning the left element reports the speed estimate (left is always owned or, for a
    // face whose left side is a ghost, the tile of the right element does)
    const int32_t reporter = (l < m.N) ? l : r;
    P.face_orig[q] = (reporter >= e0 && reporter < e1) ? f : -1;
  }
  for (int32_t e = e0; e < e1; e++)
    for (int32_t j = inc.deg[e]; j < inc.deg[e + 1]; j++) {
      const int32_t  f   = inc.ef[j];
      const uint16_t idx = static_cast<uint16_t>(s.face_at.at(f));
      const bool     right = inc.side(f, 0) != e;
      P.csr_ent[j] = static_cast<uint16_t>(idx | (right ? 0x8000u : 0u));
    }
}

// The fill pass: the arrays are sized from the offsets of the sizing pass and written in place, tiles in parallel.
// orig_gidx: geometry_dictionary's result (empty: no dictionary, no geo_idx).
void fill_tiles(TilePlan& P, const Mesh& m, const Incidence& inc, const TileLists& L, const uvector<uint16_t>& orig_gidx, int log2cap) {
  const int32_t ntiles = P.ntiles();
  const size_t  nfaces = static_cast<size_t>(P.face_off[ntiles]);
  const bool    have_dict = !orig_gidx.empty();
  P.csr_off = inc.deg;   // one entry per (element, face) incidence
  P.halo_ids.resize(P.halo_off[ntiles]);
  P.face_lr.resize(nfaces);
  if (!(have_dict && P.skip_face_geo)) P.face_geo.resize(4 * nfaces);
  if (have_dict) P.geo_idx.resize(nfaces);
  P.face_orig.resize(nfaces);
  P.csr_ent.resize(inc.ef.size());
#pragma omp parallel num_threads(host_threads())
  {
    FillScratch scratch(log2cap);
#pragma omp for schedule(dynamic, 64)
    for (int32_t t = 0; t < ntiles; t++) {
      std::copy(L.halos[t].begin(), L.halos[t].end(), P.halo_ids.begin() + P.halo_off[t]);
      if (P.tile_patch[t] >= 0) fill_patch_tile(P, inc, t);
      else fill_generic_tile(P, m, inc, t, L.tfs[t], L.halos[t], orig_gidx, scratch);
    }
  }
}

// Three classes for the multi-rank step driver: A = tiles that read ghost slots; B = other tiles that read
// an element owned by an A tile; C = the rest (deep interior). tile_order = C, B, A. A tile of class C
// depends only on B/C tiles of the previous stage, one of class A only on A/B tiles and the ghosts.
// Inside every class the patch tiles come first: a launch over a range of tile_order is a patch-kernel launch over
// the patch tiles in it and a generic launch over the rest. Sets tile_order, n_deep, n_interior, n_patch_class, n_irregular_class.
void order_tiles(TilePlan& P, const std::vector<uint8_t>& reads_ghost) {
  const int32_t        ntiles = P.ntiles();
  std::vector<uint8_t> near_boundary(ntiles, 0);
  std::vector<int32_t> owner(static_cast<size_t>(P.N));
  for (int32_t t = 0; t < ntiles; t++)
    for (int32_t e = P.elem_off[t]; e < P.elem_off[t + 1]; e++) owner[e] = t;
  for (int32_t t = 0; t < ntiles; t++) {
    if (reads_ghost[t]) continue;
    for (int32_t j = P.halo_off[t]; j < P.halo_off[t + 1] && !near_boundary[t]; j++)
      if (reads_ghost[owner[P.halo_ids[j]]]) near_boundary[t] = 1;   // (no ghost ids here: the tile reads none)
  }
  P.tile_order.clear();
  auto append_class = [&](int cls) {   // regular patches, irregular patches, generic tiles
    const int32_t first = static_cast<int32_t>(P.tile_order.size());
    for (int pass = 0; pass < 3; pass++) {
      const int32_t before = static_cast<int32_t>(P.tile_order.size());
      for (int32_t t = 0; t < ntiles; t++) {
        const int c    = reads_ghost[t] ? 2 : ((near_boundary[t] && !P.two_classes) ? 1 : 0);
        const int kind = P.tile_patch[t] < 0 ? 2 : (P.irregular_tile(t) ? 1 : 0);
        if (c == cls && kind == pass) P.tile_order.push_back(t);
      }
      if (pass == 1) {
        P.n_irregular_class[cls] = static_cast<int32_t>(P.tile_order.size()) - before;
        P.n_patch_class[cls]     = static_cast<int32_t>(P.tile_order.size()) - first;
      }
    }
  };
  append_class(0);
  P.n_deep = static_cast<int32_t>(P.tile_order.size());
  append_class(1);
  P.n_interior = static_cast<int32_t>(P.tile_order.size());
  append_class(2);
}

// Fixed-width (ELL) copy of the element face lists: one aligned 16-byte load per 8 entries. Rows exist for the elements of
// GENERIC tiles only (patch tiles read no face lists: 97 % of the benchmark mesh), in tile-index order; tile t's rows
// start at ell_row0[t] (tile_desc word 6), element e of the tile is row ell_row0[t] + (e - elem_off[t]).
// most: the faces of one element (Incidence::most).
void ell_rows(TilePlan& P, int32_t most) {
  const int32_t ntiles = P.ntiles();
  P.ell_width = std::max(8, (most + 7) / 8 * 8);
  P.ell_row0.assign(static_cast<size_t>(ntiles) + 1, 0);
  for (int32_t t = 0; t < ntiles; t++)
    P.ell_row0[t + 1] = P.ell_row0[t] + (P.tile_patch[t] >= 0 ? 0 : P.elem_off[t + 1] - P.elem_off[t]);
  P.ell.resize(static_cast<size_t>(P.ell_row0[ntiles]) * P.ell_width);
#pragma omp parallel for num_threads(host_threads()) schedule(dynamic, 64)
  for (int32_t t = 0; t < ntiles; t++) {
    if (P.tile_patch[t] >= 0) continue;
    for (int32_t e = P.elem_off[t]; e < P.elem_off[t + 1]; e++) {
      uint16_t*     row = &P.ell[static_cast<size_t>(P.ell_row0[t] + (e - P.elem_off[t])) * P.ell_width];
      const int32_t n   = P.csr_off[e + 1] - P.csr_off[e];
      for (int32_t c = 0; c < P.ell_width; c++) row[c] = c < n ? P.csr_ent[P.csr_off[e] + c] : static_cast<uint16_t>(0xFFFFu);
    }
  }
}

void build(TilePlan& P, const Mesh& m) {
  PhaseTimer      timer("tile_plan");
  const Incidence inc = element_faces(m);
  timer.lap("element -> faces");
  P.patches = find_patches(m, inc, P.want_patches);
  const std::vector<int32_t> patch_at = patch_starts(P.patches, m.N);
  timer.lap("patches");
  const int log2cap = stamp_capacity_log2(P.fcap, P.lecap, inc.most);
  P.elem_off = greedy_tiling(inc, patch_at, P.tmax, P.fcap, P.lecap, log2cap);
  timer.lap("greedy tiling");
  const TileLists lists = size_tiles(P, inc, patch_at, log2cap);
  timer.lap("per-tile lists (sizes)");
  const uvector<uint16_t> orig_gidx = geometry_dictionary(m, P.geo_table);
  timer.lap("geometry dictionary");
  fill_tiles(P, m, inc, lists, orig_gidx, log2cap);
  timer.lap("per-tile lists");
  order_tiles(P, lists.reads_ghost);
  timer.lap("tile classes");
  ell_rows(P, inc.most);
  timer.lap("ELL rows");
}

}  // namespace

extern "C" {

// Returns null if a limit of the packed format is exceeded (tile-local index >= 0xFFF0, > 32767 faces).
// flags bit 0 / 1: cut structured 2D / 3D patches (find_patches, find_patches3) out of the tiling; bit 2: the caller does not
// read `face_geo` when the plan has a geometry dictionary (sizes[11] > 0): it is left empty then
// boundary_kinds[B] (null: all walls): t8gpu_host.h
void* t8gpu_plan_plain_create_bc(int32_t N, int32_t G, int32_t F, int32_t B, int32_t ndim, const int32_t* fn,
                                 const double* normals, const double* areas, const uint8_t* kinds, int32_t tmax, int32_t fcap,
                                 int32_t flags) {
  if (N < 0 || F < 0 || B < 0 || ndim < 2 || ndim > 3 || tmax < 1 || tmax > 1024 || fcap < 1) return nullptr;
  bool open_faces = false, farfield_faces = false;
  for (int32_t b = 0; kinds && b < B; b++) {
    if (kinds[b] >= T8GPU_BOUNDARY_FARFIELD + T8GPU_MAX_FARFIELD_STATES) return nullptr;
    open_faces     = open_faces || kinds[b] != 0;
    farfield_faces = farfield_faces || kinds[b] >= T8GPU_BOUNDARY_FARFIELD;
  }
  const Mesh m{N, F, B, ndim, fn, normals, areas, open_faces ? kinds : nullptr};   // (the caller's arrays: read during build() only)
  TilePlan* P = new TilePlan;
  P->open_faces     = open_faces;
  P->farfield_faces = farfield_faces;
  P->N = N; P->G = G; P->F = F; P->B = B; P->ndim = ndim; P->tmax = tmax; P->fcap = fcap;
  P->want_patches  = flags & 27;   // bit 0: 2D patches (16 x 16), bit 1: 3D patches (8 x 8 x 4), bit 3: irregular 3D patches too, bit 4: no regular 3D ones
  P->skip_face_geo = (flags & 4) != 0;   // bit 2: no face_geo rows if the plan has a geometry dictionary
  P->two_classes   = (flags & 32) != 0;  // bit 5: interior tiles in ONE class (n_deep_tiles = n_interior_tiles): a launch over
                                         // [0, n_interior) is then one kernel launch (the two-lane step driver, stepper.hip)
  build(*P, m);
  // tile-local indices stay below the boundary codes (0xFFF0 .. 0xFFFF)
  if (P->max_elems + P->max_halo >= 0xFFF0 || P->max_faces > 0x7FFE) {
    delete P;
    return nullptr;
  }
  return P;
}
void* t8gpu_plan_plain_create_ex(int32_t N, int32_t G, int32_t F, int32_t B, int32_t ndim, const int32_t* fn,
                                 const double* normals, const double* areas, int32_t tmax, int32_t fcap, int32_t flags) {
  return t8gpu_plan_plain_create_bc(N, G, F, B, ndim, fn, normals, areas, nullptr, tmax, fcap, flags);
}
int32_t t8gpu_plan_plain_open_faces(const void* h) { return static_cast<const TilePlan*>(h)->open_faces ? 1 : 0; }
int32_t t8gpu_plan_plain_farfield_faces(const void* h) { return static_cast<const TilePlan*>(h)->farfield_faces ? 1 : 0; }
void* t8gpu_plan_plain_create(int32_t N, int32_t G, int32_t F, int32_t B, int32_t ndim, const int32_t* fn,
                              const double* normals, const double* areas, int32_t tmax, int32_t fcap) {
  return t8gpu_plan_plain_create_ex(N, G, F, B, ndim, fn, normals, areas, tmax, fcap, 0);
}
void t8gpu_plan_plain_destroy(void* h) { delete static_cast<TilePlan*>(h); }

// counts[4] = leading patch tiles of the deep / near-boundary / ghost-reading class of tile_order, and their total
void t8gpu_plan_plain_patch_counts(const void* h, int32_t* counts) {
  const TilePlan* P = static_cast<const TilePlan*>(h);
  for (int c = 0; c < 3; c++) counts[c] = P->n_patch_class[c];
  counts[3] = static_cast<int32_t>(P->patches.size());
}
// counts[3] = how many of the patch tiles of each class are IRREGULAR patches (flag 0x800; the last ones among the class's patches)
void t8gpu_plan_plain_irregular_counts(const void* h, int32_t* counts) {
  const TilePlan* P = static_cast<const TilePlan*>(h);
  for (int c = 0; c < 3; c++) counts[c] = P->n_irregular_class[c];
}
// Optional, after create and before t8gpu_plan_plain_tile_desc: volumes[N] of the owned elements. A patch whose 256 elements
// all have bit for bit the same volume gets it into its descriptor (flag 0x400, words 1 and 3), and the kernels then skip
// the per-element volume load (8 of ~130 bytes per element and stage); any other patch keeps the load. Returns the number
// of patches with a uniform volume.
int32_t t8gpu_plan_plain_patch_volumes(void* h, const double* volumes) {
  TilePlan* P = static_cast<TilePlan*>(h);
  int32_t   n = 0;
  if (!volumes) return 0;
  for (Patch& pt : P->patches) {
    const double v = volumes[pt.e0];
    bool         same = v > 0.0;
    for (int t = 1; t < kPatchElems && same; t++) same = volumes[pt.e0 + t] == v;
    pt.volume = same ? v : 0.0;
    n += same ? 1 : 0;
  }
  return n;
}
// 2 or 3: the kind of the plan's patch tiles (one kind per plan); 0: none
int32_t t8gpu_plan_plain_patch_dim(const void* h) {
  const TilePlan* P = static_cast<const TilePlan*>(h);
  return P->patches.empty() ? 0 : P->patches[0].dim;
}

// sizes[16] = {ntiles, n_halo, n_faces, n_csr, max_elems, max_halo, max_faces, n_interior_tiles, N, F,
//              ell_width, n_geo (0: no dictionary), max_slots, n_deep_tiles, n_patches, n_ell_rows}; the maxima are over the
//              generic tiles only
void t8gpu_plan_plain_sizes(const void* h, int64_t* sizes) {
  const TilePlan* P = static_cast<const TilePlan*>(h);
  sizes[0] = static_cast<int64_t>(P->elem_off.size()) - 1;
  sizes[1] = static_cast<int64_t>(P->halo_ids.size());
  sizes[2] = static_cast<int64_t>(P->face_lr.size());
  sizes[3] = static_cast<int64_t>(P->csr_ent.size());
  sizes[4] = P->max_elems;
  sizes[5] = P->max_halo;
  sizes[6] = P->max_faces;
  sizes[7] = P->n_interior;
  sizes[8] = P->N;
  sizes[9] = P->F;
  sizes[10] = P->ell_width;
  sizes[11] = static_cast<int64_t>(P->geo_table.size() / 12);
  sizes[12] = P->max_slots;
  sizes[13] = P->n_deep;
  sizes[14] = static_cast<int64_t>(P->patches.size());
  sizes[15] = P->ell_width > 0 ? static_cast<int64_t>(P->ell.size() / static_cast<size_t>(P->ell_width)) : 0;   // ELL rows
}

void t8gpu_plan_plain_compressed(const void* h, uint16_t* ell, uint16_t* geo_idx, double* geo_table) {
  const TilePlan* P = static_cast<const TilePlan*>(h);
  if (ell && !P->ell.empty()) std::memcpy(ell, P->ell.data(), P->ell.size() * sizeof(uint16_t));
  if (geo_idx && !P->geo_idx.empty()) std::memcpy(geo_idx, P->geo_idx.data(), P->geo_idx.size() * sizeof(uint16_t));
  if (geo_table && !P->geo_table.empty()) std::memcpy(geo_table, P->geo_table.data(), P->geo_table.size() * sizeof(double));
}

void t8gpu_plan_plain_tile_desc(const void* h, int32_t* tile_desc) {
  const TilePlan* P = static_cast<const TilePlan*>(h);
  for (size_t k = 0; k < P->tile_order.size(); k++) {
    const int32_t t = P->tile_order[k];
    int32_t*      d = tile_desc + 8 * k;
    d[0] = P->elem_off[t]; d[1] = P->elem_off[t + 1] - P->elem_off[t];
    d[2] = P->halo_off[t]; d[3] = P->halo_off[t + 1] - P->halo_off[t];
    d[4] = P->face_off[t]; d[5] = P->face_off[t + 1] - P->face_off[t];
    d[6] = P->ell_row0.empty() ? 0 : P->ell_row0[t];   // generic tiles: first row of the tile in `ell`
    d[7] = 0;
    if (!P->tile_patch.empty() && P->tile_patch[t] >= 0) {   // patch tile: {e0, 256, first halo entry, 64 | 256, fbase, 0x100 | 0x200 (3D) | flags, area}
      const Patch& pt = P->patches[P->tile_patch[t]];
      d[4] = pt.info.empty() ? pt.fbase : P->face_off[t];   // (irregular patch: where its per-cell words start in face_lr / face_orig)
      d[5] = 0x100 | (pt.dim == 3 ? 0x200 : 0) | pt.flags;
      std::memcpy(d + 6, &pt.area, 8);
      if (pt.volume > 0.0) {   // uniform volume: flag 0x400, the double in words 1 and 3 (element / halo counts are implied)
        int32_t w[2];
        std::memcpy(w, &pt.volume, 8);
        d[5] |= 0x400;
        d[1] = w[0];
        d[3] = w[1];
      }
    }
  }
}

// The arrays of t8gpu_plan_plain_arrays / _compressed in place (no copy): ptrs[13] = {elem_off, halo_off, face_off, halo_ids,
// face_lr, face_geo, face_orig, csr_off, csr_ent, tile_order, ell, geo_idx, geo_table}, null where empty; sizes as reported by
// t8gpu_plan_plain_sizes. Valid until t8gpu_plan_plain_destroy.
void t8gpu_plan_plain_array_ptrs(const void* h, const void** ptrs) {
  const TilePlan* P = static_cast<const TilePlan*>(h);
  auto at = [](const auto& v) -> const void* { return v.empty() ? nullptr : static_cast<const void*>(v.data()); };
  ptrs[0] = at(P->elem_off); ptrs[1] = at(P->halo_off); ptrs[2] = at(P->face_off); ptrs[3] = at(P->halo_ids);
  ptrs[4] = at(P->face_lr); ptrs[5] = at(P->face_geo); ptrs[6] = at(P->face_orig); ptrs[7] = at(P->csr_off);
  ptrs[8] = at(P->csr_ent); ptrs[9] = at(P->tile_order); ptrs[10] = at(P->ell); ptrs[11] = at(P->geo_idx);
  ptrs[12] = at(P->geo_table);
}

void t8gpu_plan_plain_arrays(const void* h, int32_t* elem_off, int32_t* halo_off, int32_t* face_off,
                             int32_t* halo_ids, uint32_t* face_lr, double* face_geo, int32_t* face_orig,
                             int32_t* csr_off, uint16_t* csr_ent, int32_t* tile_order) {
  const TilePlan* P = static_cast<const TilePlan*>(h);
  auto cp = [](auto* dst, const auto& v) {
    if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0]));
  };
  cp(elem_off, P->elem_off);
  cp(halo_off, P->halo_off);
  cp(face_off, P->face_off);
  cp(halo_ids, P->halo_ids);
  cp(face_lr, P->face_lr);
  cp(face_geo, P->face_geo);
  cp(face_orig, P->face_orig);
  cp(csr_off, P->csr_off);
  cp(csr_ent, P->csr_ent);
  cp(tile_order, P->tile_order);
}

}  // extern "C"
