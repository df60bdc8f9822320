// stage_kernel_note.hpp -- which kernel did the last fused-stage call launch for most of its work? bench.py asks
// (t8gpu_hip_last_stage_kernel) so that PMC figures taken from a committed profile are reported only for the kernel that
// was profiled. The note also keeps the grid of that launch and the name and grid of every launch of the call, in launch order
// (t8gpu_hip_last_stage_workgroups, t8gpu_hip_last_stage_launch): what the tests of the persistent walks assert.
// Host-side bookkeeping only, kept per host thread (kernels_compat.hip).
#ifndef T8GPU_HIP_STAGE_KERNEL_NOTE_HPP
#define T8GPU_HIP_STAGE_KERNEL_NOTE_HPP

#include <cstdio>
#include <cstring>

namespace t8gpu_hip {

constexpr int kStageLaunchesNoted = 8;   // (a stage call launches at most 3 classes x (regular + irregular patches + generic tiles))

struct StageLaunchNote {
  char name[192];
  int  workgroups;
};
struct StageKernelNote {
  char            name[192];
  long long       weight;
  int             workgroups;   // grid of the launch `name` names
  int             n_launches;   // launches of the call, counted past kStageLaunchesNoted
  StageLaunchNote launches[kStageLaunchesNoted];
};
StageKernelNote& stage_kernel_note();   // (kernels_compat.hip)

inline void stage_kernel_note_reset() {
  StageKernelNote& n = stage_kernel_note();
  n.weight           = -1;
  n.n_launches       = 0;
}

inline int stage_kernel_arg(char* s, size_t n, bool v) { return std::snprintf(s, n, ", %s", v ? "true" : "false"); }
inline int stage_kernel_arg(char* s, size_t n, int v) { return std::snprintf(s, n, ", %d", v); }

// Notes the launch of kernel<T, args...> (args: the launch's compile-time ints and bools, e.g. dispatch()'s constants) by
// its name as rocprofv3 prints it -- the demangled symbol without namespace and parameter list: float / double, decimal
// ints, true / false, separated by ", ". weight: the work units (tiles, blocks) of this launch -- the heaviest launch of a
// call stays. workgroups: the launch's grid.
template <class T, class... A>
void note_stage_kernel(long long weight, unsigned workgroups, const char* kernel, A... args) {
  StageKernelNote& n       = stage_kernel_note();
  const bool       heavier = weight > n.weight;
  const int        slot    = n.n_launches++;
  if (!heavier && slot >= kStageLaunchesNoted) return;
  char         local[sizeof(n.name)];
  char* const  name = slot < kStageLaunchesNoted ? n.launches[slot].name : local;
  const size_t cap  = sizeof(n.name);
  size_t       o    = std::snprintf(name, cap, "%s<%s", kernel, sizeof(T) == 8 ? "double" : "float");
  ((o += o < cap ? stage_kernel_arg(name + o, cap - o, args) : 0), ...);
  if (o < cap) std::snprintf(name + o, cap - o, ">");
  if (slot < kStageLaunchesNoted) n.launches[slot].workgroups = static_cast<int>(workgroups);
  if (heavier) {
    n.weight     = weight;
    n.workgroups = static_cast<int>(workgroups);
    std::strcpy(n.name, name);   // (snprintf has terminated it inside `cap`)
  }
}

}  // namespace t8gpu_hip

#endif  // T8GPU_HIP_STAGE_KERNEL_NOTE_HPP
