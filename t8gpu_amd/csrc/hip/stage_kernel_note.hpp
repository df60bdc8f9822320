// stage_kernel_note.hpp -- which kernel did the last fused-stage call launch for most of its work? bench.py asks
// (t8gpu_hip_last_stage_kernel) so that PMC figures taken from a committed profile are reported only for the kernel that
// was profiled. Host-side bookkeeping only, kept per host thread (kernels_compat.hip).
#ifndef T8GPU_HIP_STAGE_KERNEL_NOTE_HPP
#define T8GPU_HIP_STAGE_KERNEL_NOTE_HPP

#include <cstdio>

namespace t8gpu_hip {

struct StageKernelNote {
  char      name[192];
  long long weight;
};
StageKernelNote& stage_kernel_note();   // (kernels_compat.hip)

inline void stage_kernel_note_reset() { stage_kernel_note().weight = -1; }

inline int stage_kernel_arg(char* s, size_t n, bool v) { return std::snprintf(s, n, ", %s", v ? "true" : "false"); }
inline int stage_kernel_arg(char* s, size_t n, int v) { return std::snprintf(s, n, ", %d", v); }

// Notes the launch of kernel<T, args...> (args: the launch's compile-time ints and bools, e.g. dispatch()'s constants) by
// its name as rocprofv3 prints it -- the demangled symbol without namespace and parameter list: float / double, decimal
// ints, true / false, separated by ", ". weight: the work units (tiles, blocks) of this launch -- the heaviest launch of a
// call stays.
template <class T, class... A>
void note_stage_kernel(long long weight, const char* kernel, A... args) {
  StageKernelNote& n = stage_kernel_note();
  if (weight <= n.weight) return;
  n.weight     = weight;
  const size_t cap = sizeof(n.name);
  size_t       o   = std::snprintf(n.name, cap, "%s<%s", kernel, sizeof(T) == 8 ? "double" : "float");
  ((o += o < cap ? stage_kernel_arg(n.name + o, cap - o, args) : 0), ...);
  if (o < cap) std::snprintf(n.name + o, cap - o, ">");
}

}  // namespace t8gpu_hip

#endif  // T8GPU_HIP_STAGE_KERNEL_NOTE_HPP
