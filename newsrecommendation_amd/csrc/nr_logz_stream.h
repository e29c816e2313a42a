// What the passes that stream the corpus in the log-partition's segments share (nr_logz.hip: K13; nr_expect.hip: K17): the plan
// that cuts [1, V) into segments and slices, and the exclusion lists of the stream -- the cursor of a user into its CSR segment
// and the "listed" masks of a chunk.  A news is a term of K17's expectation exactly when it is a term of K13's sum, so there is
// ONE definition of what the stream leaves out.
#pragma once
#include "nr_score_tile.h"

namespace {

constexpr int LZ_MAX_SEGS = 256;
constexpr float LZ_INF = __builtin_inff();

struct LogzPlan {
  int TU, seg, nseg, splits, segs_per;
};
// seg and nseg depend on V alone; `splits` (0: fill the chip, score_auto_splits for user tiles of TU) only groups whole segments
// into slices
inline LogzPlan lz_plan_tile(int U, int V, int TU, int splits) {
  LogzPlan p;
  p.TU = TU;
  const long per = (long)TK_ROWS * LZ_MAX_SEGS;
  p.seg = TK_ROWS * (int)(((long)V - 1 + per - 1) / per);
  p.nseg = (int)(((long)V - 1 + p.seg - 1) / p.seg);
  long s = splits > 0 ? splits : score_auto_splits(U, V, p.TU, LZ_MAX_SEGS);   // nseg <= chunks, nseg <= LZ_MAX_SEGS
  if (s > p.nseg) s = p.nseg;
  if (s < 1) s = 1;
  p.segs_per = (int)((p.nseg + s - 1) / s);
  p.splits = (p.nseg + p.segs_per - 1) / p.segs_per;   // no empty slice
  return p;
}

// The two pieces below are statement macros, not functions: K13's kernels must keep the instruction streams they had when
// this text stood in logz_stream_kernel itself, and the compiler schedules an inlined function's body differently from the same
// statements in place (tools/isa_diff.sh shows it).  Both are used inside a kernel templated on PER_WAVE with `lane` in scope.

// LISTS: the cursor of every user of the wave (user u0 + wave + 8 i of the tile) = the first entry of its segment that is >= v_lo.
// A 64-ary search, the users of the wave side by side (their probes are independent loads): answer in [lo, hi], 64 probes
// lo + lane * step a round; ascending entries make "probe < v_lo" a prefix of p lanes, which leaves (lo + (p - 1) step, lo + p step].
// Every index formed lies in [lo, hi) within the clamped segment; a round shrinks an open range below its step, so the loop ends
// whatever the entries hold.  cur, end: int32_t [PER_WAVE].
#define LZ_SEEK(ca, u0, wave, lane, U_, v_lo, cur, end)                                            \
  {                                                                                                \
    _Pragma("unroll") for (int i = 0; i < PER_WAVE; ++i) {                                         \
      const int u = (u0) + (wave) + TK_WAVES * i;                                                  \
      cur[i] = end[i] = 0;                                                                         \
      if (u < (U_)) (ca).segment(u, cur[i], end[i]);                                               \
    }                                                                                              \
    int32_t hi[PER_WAVE];                                                                          \
    _Pragma("unroll") for (int i = 0; i < PER_WAVE; ++i) hi[i] = end[i];                           \
    for (;;) {                                                                                     \
      int32_t val[PER_WAVE], step[PER_WAVE];                                                       \
      _Pragma("unroll") for (int i = 0; i < PER_WAVE; ++i) {                                       \
        const int32_t n = hi[i] - cur[i];                                                          \
        step[i] = (n + 63) >> 6;                                                                   \
        const long idx = (long)cur[i] + (long)(lane) * step[i];                                    \
        val[i] = n > 0 && idx < hi[i] ? (ca).ids[idx] : 0x7fffffff;                                \
      }                                                                                            \
      bool open = false;                                                                           \
      _Pragma("unroll") for (int i = 0; i < PER_WAVE; ++i) {                                       \
        const int32_t n = hi[i] - cur[i];                                                          \
        if (n <= 0) continue;                                                                      \
        const long idx = (long)cur[i] + (long)(lane) * step[i];                                    \
        const int p = __popcll(__ballot(idx < hi[i] && (long)val[i] < (v_lo)));                    \
        if (p == 0) hi[i] = cur[i];                                                                \
        else if (step[i] == 1) { cur[i] += p; hi[i] = cur[i]; }                                    \
        else {                                                                                     \
          const long nh = (long)cur[i] + (long)p * step[i];                                        \
          cur[i] = (int32_t)((long)cur[i] + (long)(p - 1) * step[i] + 1);                          \
          hi[i] = nh < hi[i] ? (int32_t)nh : hi[i];                                                \
        }                                                                                          \
        open = open || hi[i] > cur[i];                                                             \
      }                                                                                            \
      if (!open) break;                                                                            \
    }                                                                                              \
  }

// LISTS: the entries of one user inside the chunk [vc, vc + 128) are a prefix of what its cursor points at; bit r of (l0, l1) =
// news vc + r is listed.  e_first = the lane's entry ids[cur + lane] (0x7fffffff beyond the segment), loaded by the caller ahead
// of the barrier; the cursor moves past the chunk's entries.
#define LZ_LISTED(ca, e_first, cur, end, vc, lane, l0, l1)                                         \
  {                                                                                                \
    int32_t e = (e_first);                                                                         \
    for (;;) {                                                                                     \
      const int c = __popcll(__ballot((long)(cur) + (lane) < (end) && (long)e < (vc) + TK_ROWS));  \
      for (int j = 0; j < c; ++j) {                                                                \
        const uint32_t r = (uint32_t)((long)__builtin_amdgcn_readlane(e, j) - (vc));               \
        if (r < 64u) l0 |= 1ull << r;                                                              \
        else if (r < 128u) l1 |= 1ull << (r - 64u);                                                \
      }                                                                                            \
      (cur) += c;                                                                                  \
      if (c < 64) break; /* a full probe: the chunk may hold 64 more */                            \
      e = (long)(cur) + (lane) < (end) ? (ca).ids[(long)(cur) + (lane)] : 0x7fffffff;              \
    }                                                                                              \
  }

}  // namespace
