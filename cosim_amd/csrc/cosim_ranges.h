// cosim_ranges.h -- how a fleet is cut into logical ranges, how many engine-owned streams carry them, and which ranges share one.
// Plain C++17, no HIP: cosim_engine.hip's set_ranges uses it, tests/range_groups.cpp builds it alone.
//
// A caller asks for R ranges (cosim_set_param "ranges"); the engine owns P <= R streams and issues each control step as P launch
// sequences, one per GROUP of consecutive ranges, over the union of the group's envs.  Streams that share a hardware queue run their
// kernels one after the other, so range streams beyond what the process has queues for cost time instead of hiding launch tails
// (DESIGN 4.6): P follows the queues, R stays what the caller asked for.
#pragma once
#include <cstdlib>

namespace cosim {

constexpr int HIP_DEFAULT_HW_QUEUES = 4;   // what the HIP runtime opens per process when GPU_MAX_HW_QUEUES is not set

// Range i of R over n_envs: contiguous, the first (n_envs / unit) % R of them one unit longer, the last takes what is left (an odd
// env under unit 2 never happens: two envs per wave needs an even fleet).  unit 2: even sizes for the two-envs-per-wave kernel.
inline void range_bounds(int n_envs, int ranges, int unit, int i, int* first, int* count) {
  const int units = n_envs / unit, q = units / ranges, r = units % ranges;
  const int f = (i * q + (i < r ? i : r)) * unit;
  *first = f;
  *count = i == ranges - 1 ? n_envs - f : (q + (i < r ? 1 : 0)) * unit;
}

// Group g of P over R ranges holds ranges [group_first(g), group_first(g + 1)): consecutive, never empty for P <= R, sizes differ
// by at most one range.  With P == R every range is its own group.
inline int group_first(int g, int ranges, int streams) { return (int)((long long)g * ranges / streams); }

// the group range i belongs to: the largest g with group_first(g) <= i
inline int group_of(int i, int ranges, int streams) {
  int g = (int)(((long long)(i + 1) * streams - 1) / ranges);
  while (g + 1 < streams && group_first(g + 1, ranges, streams) <= i) g++;
  while (g > 0 && group_first(g, ranges, streams) > i) g--;
  return g;
}

// GPU_MAX_HW_QUEUES as the process has it (null: unset).  Anything that is not a whole positive number counts as unset.
inline int hw_queues_from_env(const char* value) {
  if (!value || !*value) return HIP_DEFAULT_HW_QUEUES;
  char* end = nullptr;
  const long v = std::strtol(value, &end, 10);
  while (end && (*end == ' ' || *end == '\t')) end++;
  if (!end || *end != '\0' || v < 1 || v > 1 << 20) return HIP_DEFAULT_HW_QUEUES;
  return (int)v;
}

// Streams for R ranges in a process with Q hardware queues: half the queues, at least one, at most R.  The caller's own stream and
// the runtime's take queues too; measured on MI355X: Q = 8 carries four range chains side by side, Q = 4 carries two,
// and three or four on Q = 4 put two chains on one queue, where they run back to back.
inline int range_stream_count(int ranges, int hw_queues) {
  int p = hw_queues / 2;
  if (p < 1) p = 1;
  if (ranges < 1) ranges = 1;
  return p < ranges ? p : ranges;
}

// what "range_streams" asked for (0: auto) -> streams in use
inline int range_streams_in_use(int asked, int ranges, int hw_queues) {
  if (ranges < 1) ranges = 1;
  if (asked >= 1) return asked < ranges ? asked : ranges;
  return range_stream_count(ranges, hw_queues);
}

}  // namespace cosim
