// cell_faces.cpp -- element -> interior faces in CSR form, for the gather kernels of csrc/hip/fields.hip (derived output
// fields: a cell sums the terms of its own faces, so it needs the list the face arrays do not hold).
//
// A counting sort over face_neighbors[2 f + {0, 1}] (l, r of interior face f). Rows exist for the owned elements
// [0, n_owned); a side that is a ghost slot (>= n_owned) gets no entry, so a face with one ghost side is listed once.
// Entry = 2 f + side, side 0 where the element is l of face f; within a row the entries ascend in f. For Subgrid
// partitions the elements are the blocks.
//
// Threads split the ELEMENT range, and each scans the whole face list for the sides that fall into its share: no
// atomics, and the order inside a row is the order of the scan on any thread count.
#include <cstdint>

#include "host_threads.hpp"
#include "t8gpu_host.h"

extern "C" int64_t t8gpu_host_cell_faces(int32_t n_owned, int64_t num_faces, const int32_t* face_neighbors, int32_t* offsets,
                                         int32_t* entries) {
  if (n_owned < 0 || num_faces < 0 || num_faces >= (int64_t(1) << 30) || !offsets) return -1;
  if (num_faces > 0 && (!face_neighbors || !entries)) return -1;
  const int64_t n2 = 2 * num_faces;
  for (int32_t e = 0; e <= n_owned; e++) offsets[e] = 0;

  int nthreads = host_threads();
  if (n_owned < 4096 || num_faces < 4096) nthreads = 1;     // (small meshes: one scan)
  int bad = 0;
  // pass 1: offsets[e + 1] = entries of element e
#pragma omp parallel num_threads(nthreads) reduction(| : bad)
  {
    const int     t = omp_get_thread_num(), nt = omp_get_num_threads();
    const int64_t lo = (int64_t)n_owned * t / nt, hi = (int64_t)n_owned * (t + 1) / nt;
    for (int64_t k = 0; k < n2; k++) {
      const int32_t e = face_neighbors[k];
      if (e < 0) bad = 1;
      if (e >= lo && e < hi) offsets[e + 1]++;
    }
  }
  if (bad) return -2;
  for (int32_t e = 0; e < n_owned; e++) offsets[e + 1] += offsets[e];
  const int64_t total = offsets[n_owned];

  // pass 2: fill in ascending f
  uvector<int32_t> cursor(static_cast<size_t>(n_owned));
#pragma omp parallel num_threads(nthreads)
  {
    const int     t = omp_get_thread_num(), nt = omp_get_num_threads();
    const int64_t lo = (int64_t)n_owned * t / nt, hi = (int64_t)n_owned * (t + 1) / nt;
    for (int64_t e = lo; e < hi; e++) cursor[e] = offsets[e];
    for (int64_t k = 0; k < n2; k++) {
      const int32_t e = face_neighbors[k];
      if (e >= lo && e < hi) entries[cursor[e]++] = static_cast<int32_t>(k);   // k = 2 f + side
    }
  }
  return total;
}
