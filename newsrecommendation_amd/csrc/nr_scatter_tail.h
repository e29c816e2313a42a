// Roles of the table-gradient scatter GEMM's workgroups (gemm_nt_dma_kernel<EPI_SCATTER, ., false, 4>, compact id-sorted rows).
// Plain C++ with no other include: the kernel, its launcher and the host check (nr_scatter_tail_check.cpp) compile this text.
//
// One 256-row tile occupies a CU, so T = ceil(count / 256) tiles run in rounds of R (R = CUs) and the last, partly filled
// round lasts as long as a full one while most CUs idle.  The tiles of that round -- r = T mod R of them -- are therefore
// split over K when at least half of the CUs would idle: S = min(R / r, 8, nk) workgroups per tile, each running a contiguous
// range of the nk k-steps and then the scatter epilogue on its partial sums (the epilogue is linear in the accumulators).
//   workgroup b < F = T - r         tile b, every k-step                        (as without the split)
//   workgroup F + j, j < r * S      tile F + j / S, k-steps [p nk / S, (p + 1) nk / S) with p = j mod S
//   any other workgroup             nothing
// R = 0 switches the split off (every tile one workgroup).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NR_TAIL_HD __host__ __device__
#else
#define NR_TAIL_HD
#endif

constexpr int NR_SCATTER_TAIL_ROWS = 256;        // rows per tile (WM = 4)
constexpr int NR_SCATTER_TAIL_MAX_SPLIT = 8;

struct ScatterTailRole {
  int tile;                // -1: this workgroup has nothing to do
  int k_begin, k_end;      // k-steps [k_begin, k_end) of the tile, never empty
};

NR_TAIL_HD inline ScatterTailRole nr_scatter_tail_role(int wg, int count, int R, int nk) {
  const int T = (count + NR_SCATTER_TAIL_ROWS - 1) / NR_SCATTER_TAIL_ROWS;
  const int F = R > 0 ? (T / R) * R : T, r = T - F;
  if (wg < F) return ScatterTailRole{wg, 0, nk};
  int S = 1;
  if (r > 0 && 2 * r <= R) {
    S = R / r;
    if (S > NR_SCATTER_TAIL_MAX_SPLIT) S = NR_SCATTER_TAIL_MAX_SPLIT;
    if (S > nk) S = nk;
    if (S < 1) S = 1;
  }
  const int j = wg - F;
  if (j >= r * S) return ScatterTailRole{-1, 0, 0};
  const int p = j % S;
  return ScatterTailRole{F + j / S, p * nk / S, (p + 1) * nk / S};
}

// workgroups to launch for at most `max_rows` rows: every tile, and the largest number the split can add (r * S - r < R)
NR_TAIL_HD inline int nr_scatter_tail_grid(int max_rows, int R) {
  return (max_rows + NR_SCATTER_TAIL_ROWS - 1) / NR_SCATTER_TAIL_ROWS + (R > 0 ? R : 0);
}
