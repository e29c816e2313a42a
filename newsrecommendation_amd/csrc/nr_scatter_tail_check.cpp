// Host check of nr_scatter_tail.h (built and run by tests/test_scatter_tail_host.py; not part of libnrhip.so):
// for R = 256, nk in {1, 7, 38} and every tile count T in 0 .. 3R + 1 -- with the row count at both ends of the range that
// gives T tiles -- the roles of the launched workgroups cover every (tile, k-step) exactly once, stay inside the grid, split
// nothing below the last round, keep every part non-empty and at most 8 per tile, and R = 0 leaves every tile whole.
#include <cstdio>
#include <vector>

#include "nr_scatter_tail.h"

static int fails = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      if (++fails <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                         \
  } while (0)

static void check_one(int count, int R, int nk, int max_rows) {
  const int T = (count + 255) / 256, grid = nr_scatter_tail_grid(max_rows, R);
  std::vector<int> cover((size_t)T * nk, 0), parts(T, 0);
  int busy = 0;
  for (int wg = 0; wg < grid; ++wg) {
    const ScatterTailRole ro = nr_scatter_tail_role(wg, count, R, nk);
    if (ro.tile < 0) continue;
    ++busy;
    CHECK(ro.tile < T, "count %d R %d nk %d wg %d tile %d", count, R, nk, wg, ro.tile);
    CHECK(0 <= ro.k_begin && ro.k_begin < ro.k_end && ro.k_end <= nk, "count %d R %d nk %d wg %d k [%d, %d)", count, R, nk, wg, ro.k_begin, ro.k_end);
    if (ro.tile >= T || ro.k_begin < 0 || ro.k_end > nk) continue;
    ++parts[ro.tile];
    for (int k = ro.k_begin; k < ro.k_end; ++k) ++cover[(size_t)ro.tile * nk + k];
  }
  for (size_t i = 0; i < cover.size(); ++i) CHECK(cover[i] == 1, "count %d R %d nk %d tile %zu k %zu covered %d times", count, R, nk, i / nk, i % nk, cover[i]);
  // nothing past the grid has a role
  for (int wg = grid; wg < grid + 2 * (R + 1); ++wg)
    CHECK(nr_scatter_tail_role(wg, count, R, nk).tile < 0, "count %d R %d nk %d: wg %d beyond the grid has a role", count, R, nk, wg);
  const int F = R > 0 ? (T / R) * R : T, r = T - F;
  const int S = (r > 0 && 2 * r <= R) ? (R / r < 8 ? (R / r < nk ? R / r : nk) : (8 < nk ? 8 : nk)) : 1;
  for (int t = 0; t < T; ++t) CHECK(parts[t] == (t < F ? 1 : S), "count %d R %d nk %d tile %d has %d parts, expected %d", count, R, nk, t, parts[t], t < F ? 1 : S);
  // the last round never needs more than R workgroups at once
  CHECK(busy - F <= (R > 0 ? R : T), "count %d R %d nk %d: %d workgroups in the last round", count, R, nk, busy - F);
}

int main() {
  const int R = 256, nks[3] = {1, 7, 38};
  for (int nk : nks)
    for (int T = 0; T <= 3 * R + 1; ++T) {
      const int max_rows = (3 * R + 1) * 256;
      if (T == 0) { check_one(0, R, nk, max_rows); check_one(0, 0, nk, max_rows); continue; }
      const int counts[3] = {(T - 1) * 256 + 1, (T - 1) * 256 + 100, T * 256};
      for (int c : counts) {
        check_one(c, R, nk, max_rows);     // launched for the largest count ...
        check_one(c, R, nk, c);            // ... and for exactly this one
        check_one(c, 0, nk, c);            // split off
      }
    }
  // the bench shape's counts (nk = 38): 2, 2, 1 and 8 parts per tail tile
  const int live[4] = {283965, 286182, 259160, 269950}, want[4] = {2, 2, 1, 8};
  for (int b = 0; b < 4; ++b) {
    const int T = (live[b] + 255) / 256, F = (T / R) * R;
    int parts = 0;
    for (int wg = 0; wg < nr_scatter_tail_grid(844800, R); ++wg) parts += nr_scatter_tail_role(wg, live[b], R, 38).tile == F;
    CHECK(parts == want[b], "batch %d: %d parts for the first tail tile, expected %d", b, parts, want[b]);
  }
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("scatter tail roles ok\n");
  return 0;
}
