// Host driver of the rotation rule and the tile-capacity bound (cosim_amd/csrc/cosim_poltab.h: policy_at, episodes_after,
// policy_tile_capacity), built by tests/test_policy_rotate_host.py as plain C++ (once more with -fsanitize=address,undefined).  It takes
// no input: the cases are made here from a fixed seed.  Every check that fails prints "FAIL <what>" and the exit status is 1; otherwise
// the last line is "OK <rule cases> <bound cases> <cases that meet the bound>".
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "cosim_poltab.h"

using namespace cosim;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL " __VA_ARGS__); printf("\n"); failures++; } } while (0)

// the formula in 64-bit arithmetic, where nothing can overflow
static int64_t rule64(int64_t base, int64_t e, int64_t every, int64_t K) { return (base + (e < 0 ? 0 : e) / every) % K; }

// tiles of one range under `assign`, and what the bound allows
static void bound_case(const std::vector<int32_t>& assign, int K, const char* what, long* cases, long* met, bool must_meet = false) {
  const int n = (int)assign.size();
  const int32_t range[2] = {0, n};
  const PolTiles t = build_policy_tiles(assign.data(), K, range, 1);
  const int cap = policy_tile_capacity(n, K);
  CHECK((int)t.tiles.size() <= cap, "%s: n %d K %d needs %zu tiles, the bound is %d", what, n, K, t.tiles.size(), cap);
  CHECK(t.tile_span[1] == (int)t.tiles.size() && (int)t.rows.size() == n, "%s: spans", what);
  if ((int)t.tiles.size() == cap) ++*met;
  if (must_meet) CHECK((int)t.tiles.size() == cap, "%s: n %d K %d has %zu tiles, expected the bound %d itself", what, n, K, t.tiles.size(), cap);
  ++*cases;
}

int main() {
  std::mt19937_64 rng(20240607);
  long rule_cases = 0, bound_cases = 0, met = 0;
  // ---- the rule against its formula
  const int32_t near_max[] = {INT32_MAX, INT32_MAX - 1, INT32_MAX - 63, INT32_MAX / 2, 0, 1, 2, 31, 32, 33, 63, 64, 65, -1, INT32_MIN};
  for (int K : {1, 2, 3, 5, 63, 64})
    for (int32_t every : {1, 2, 3, 7, 64, 1000, INT32_MAX})
      for (int32_t base = 0; base < K; base += (K > 8 ? 7 : 1)) {
        for (int32_t e : near_max) {
          const int32_t k = policy_at(base, e, every, K);
          CHECK(k >= 0 && k < K && k == rule64(base, e, every, K), "rule: base %d e %d every %d K %d gives %d", base, e, every, K, k);
          rule_cases++;
        }
        for (int q = 0; q < 50; q++) {
          const int32_t e = (int32_t)(rng() % ((uint64_t)INT32_MAX + 1));
          const int32_t k = policy_at(base, e, every, K);
          CHECK(k >= 0 && k < K && k == rule64(base, e, every, K), "rule: base %d e %d every %d K %d gives %d", base, e, every, K, k);
          rule_cases++;
        }
      }
  // K = 1: always policy 0; every = 1: one step per episode; a period of K * every
  for (int32_t e = 0; e < 200; e++) {
    CHECK(policy_at(0, e, 3, 1) == 0, "rule: K = 1, e %d", e);
    CHECK(policy_at(2, e, 1, 5) == (2 + e) % 5, "rule: every = 1, e %d", e);
    CHECK(policy_at(1, e, 4, 3) == policy_at(1, e + 12, 4, 3), "rule: period, e %d", e);
  }
  // the counter: one more per ended episode, held at the top
  CHECK(episodes_after(0, false) == 0 && episodes_after(0, true) == 1 && episodes_after(41, true) == 42, "counter: plain");
  CHECK(episodes_after(INT32_MAX - 1, true) == INT32_MAX && episodes_after(INT32_MAX, true) == INT32_MAX && episodes_after(INT32_MAX, false) == INT32_MAX,
        "counter: held at INT32_MAX");
  // ---- the bound
  CHECK(policy_tile_capacity(1, 64) == 1 && policy_tile_capacity(32, 1) == 2 && policy_tile_capacity(33, 3) == 4 && policy_tile_capacity(1024, 3) == 35 &&
        policy_tile_capacity(65536, 64) == 2112, "capacity: by hand");
  for (int n : {1, 2, 31, 32, 33, 63, 64, 65, 97, 1024, 2113})
    for (int K : {1, 2, 3, 31, 32, 33, 64}) {
      std::vector<int32_t> a(n);
      for (int q = 0; q < 6; q++) {
        for (int i = 0; i < n; i++) a[i] = (int32_t)(rng() % (uint64_t)K);
        bound_case(a, K, "random", &bound_cases, &met);
      }
      for (int i = 0; i < n; i++) a[i] = 0;
      bound_case(a, K, "all rows on one policy", &bound_cases, &met);
      for (int i = 0; i < n; i++) a[i] = K - 1;
      bound_case(a, K, "all rows on the last policy", &bound_cases, &met);
      for (int i = 0; i < n; i++) a[i] = i % K;
      bound_case(a, K, "interleaved", &bound_cases, &met);
      // as many policies as possible with a partial tile: one row each, the rest on policy 0
      for (int i = 0; i < n; i++) a[i] = i < K ? i : 0;
      bound_case(a, K, "one row per policy, the rest on policy 0", &bound_cases, &met);
      // 33 rows on as many policies as the rows allow
      for (int i = 0; i < n; i++) a[i] = (i / 33) % K;
      bound_case(a, K, "33 rows per policy", &bound_cases, &met);
    }
  {
    std::vector<int32_t> a(33 * 64);   // 33 rows on each of 64 policies: 128 tiles, the bound is 66 + 64
    for (size_t i = 0; i < a.size(); i++) a[i] = (int32_t)(i % 64);
    bound_case(a, 64, "33 rows on each of 64 policies", &bound_cases, &met);
    const int32_t range[2] = {0, (int32_t)a.size()};
    CHECK(build_policy_tiles(a.data(), 64, range, 1).tiles.size() == 128, "33 rows on each of 64 policies: 128 tiles");
  }
  for (int n = 1; n < 32; n++) {       // a single row per policy, fewer than a tile's rows: n tiles, and the bound is n
    std::vector<int32_t> a(n);
    for (int i = 0; i < n; i++) a[i] = i;
    bound_case(a, 64, "a single row per policy", &bound_cases, &met, true);
    bound_case(a, n, "a single row per policy, K = n", &bound_cases, &met, true);
  }
  if (failures) return 1;
  printf("OK %ld %ld %ld\n", rule_cases, bound_cases, met);
  return 0;
}
