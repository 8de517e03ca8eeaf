// csrc/cosim_ranges.h as a plain C++ program (no HIP, no GPU), driven by tests/test_range_groups_host.py.
//
// No arguments: checks every (R, P, fleet size, unit) below and exits 0, or prints the first violation and exits 1:
//   ranges: contiguous from env 0 to n_envs, none empty, sizes differ by at most one unit (the last takes an odd remainder);
//   groups: consecutive ranges, in order, none empty, sizes differ by at most one range, group_of agrees with group_first;
//   unit 2: every group union starts on an even env and (even fleet) has an even size.
// `table`: prints "R Q P" for R in 1..16 and Q in {0, 1, 2, 3, 4, 5, 8, 16, 32}.
// `env [VALUE]`: prints hw_queues_from_env(VALUE), without VALUE of a null pointer (variable not set).
// `use ASKED R Q`: prints range_streams_in_use.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cosim_ranges.h"

using namespace cosim;

static int bad(const char* what, int n, int R, int P, int unit, int i) {
  std::printf("FAIL %s: n_envs %d ranges %d streams %d unit %d at %d\n", what, n, R, P, unit, i);
  return 1;
}

static int check(int n, int R, int unit) {
  std::vector<int> first(R), count(R);
  int at = 0, lo = n, hi = 0;
  for (int i = 0; i < R; i++) {
    range_bounds(n, R, unit, i, &first[i], &count[i]);
    if (first[i] != at) return bad("range not contiguous", n, R, 0, unit, i);
    if (count[i] < 1) return bad("empty range", n, R, 0, unit, i);
    if (unit == 2 && (first[i] & 1)) return bad("odd range start", n, R, 0, unit, i);
    if (unit == 2 && n % 2 == 0 && (count[i] & 1)) return bad("odd range size", n, R, 0, unit, i);
    at += count[i];
    const int c = i == R - 1 ? count[i] - n % unit : count[i];   // the last range also takes the env an odd fleet leaves over
    lo = c < lo ? c : lo; hi = c > hi ? c : hi;
  }
  if (at != n) return bad("ranges do not cover the fleet", n, R, 0, unit, R);
  if (hi - lo > unit) return bad("range sizes differ by more than one unit", n, R, 0, unit, R);
  for (int P = 1; P <= R; P++) {
    if (group_first(0, R, P) != 0 || group_first(P, R, P) != R) return bad("groups do not cover the ranges", n, R, P, unit, 0);
    int glo = R, ghi = 0;
    for (int g = 0; g < P; g++) {
      const int r0 = group_first(g, R, P), r1 = group_first(g + 1, R, P);
      if (r1 <= r0) return bad("empty group", n, R, P, unit, g);
      glo = r1 - r0 < glo ? r1 - r0 : glo; ghi = r1 - r0 > ghi ? r1 - r0 : ghi;
      for (int r = r0; r < r1; r++)
        if (group_of(r, R, P) != g) return bad("group_of disagrees with group_first", n, R, P, unit, r);
      const int gf = first[r0], gc = first[r1 - 1] + count[r1 - 1] - first[r0];
      int sum = 0;
      for (int r = r0; r < r1; r++) sum += count[r];
      if (sum != gc || gc < 1) return bad("group union is not the sum of its ranges", n, R, P, unit, g);
      if (unit == 2 && ((gf & 1) || (n % 2 == 0 && (gc & 1)))) return bad("odd group union", n, R, P, unit, g);
    }
    if (ghi - glo > 1) return bad("group sizes differ by more than one range", n, R, P, unit, P);
    if (P == R && (glo != 1 || ghi != 1)) return bad("P == R must leave one range per group", n, R, P, unit, P);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "table")) {
    const int Q[] = {0, 1, 2, 3, 4, 5, 8, 16, 32};
    for (int R = 1; R <= 16; R++)
      for (int q : Q) std::printf("%d %d %d\n", R, q, range_stream_count(R, q));
    return 0;
  }
  if (argc >= 2 && !std::strcmp(argv[1], "env")) {
    std::printf("%d\n", hw_queues_from_env(argc >= 3 ? argv[2] : nullptr));
    return 0;
  }
  if (argc == 5 && !std::strcmp(argv[1], "use")) {
    std::printf("%d\n", range_streams_in_use(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4])));
    return 0;
  }
  const int fleets[] = {16, 17, 64, 70, 96, 127, 128, 1000, 1024, 4096, 4098, 65537};
  int cases = 0;
  for (int n : fleets)
    for (int R = 1; R <= 16; R++)
      for (int unit = 1; unit <= 2; unit++) {
        if (R * unit > n) continue;
        if (check(n, R, unit)) return 1;
        cases++;
      }
  std::printf("ok %d\n", cases);
  return 0;
}
