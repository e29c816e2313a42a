// Full-corpus rank evaluation: for every user and each of its held-out targets, the exact 1-based position of that news in the
// user's ranking of the WHOLE table under the order of nr_score_topk (score descending, news id ascending) -- again without the
// [U, V] score matrix.  Scores come from the tile of nr_score_tile.h, so they have the bits nr_score_topk sees: "rank <= k"
// and "is in the top-k row" are the same statement.
//
//   rank_named_kernel       one workgroup per 16 users.  Chunk c of the tile is made of the table rows user c of the group NAMES:
//                           its targets (chunk rows 0 .. 63) and its excluded ids (64 .. 127), gathered by id; of the [16 x 128]
//                           scores only row c is kept.  One wave then settles everything that needs no other news: which
//                           targets are ranked at all (in range, not NaN, not excluded, not a repeat), their 64-bit keys
//                           (score key << 32 | ~id, as in nr_topk.hip) compacted to the front of the row, and for each the number
//                           of distinct excluded news that beat it.
//   rank_named_csr_kernel   the named pass of a call with exclusion lists in CSR form (include/nrhip.h K9 / K10), any length.
//                           Chunk 0 of a user is unchanged: targets in rows 0 .. 63, the first 64 listed ids in rows 64 .. 127.
//                           A user with more listed ids gets further chunks of 128 gathered rows each through the same
//                           ScoreTile<1> sequence, so every listed news has the key bits the stream gives it.  Wave 0 keeps the
//                           target keys in registers across the user's chunks, uncompacted (lane j = target j); per chunk it
//                           adds, per target, the listed news that beat it and clears `ranked` for a target found in the list;
//                           the compaction happens after the user's last chunk.  "Each listed news once" is the strict order
//                           of the segment.  The ids of a chunk are staged in LDS one chunk ahead (two buffers), so the pass
//                           needs no more LDS than rank_named_kernel.  Of the [16 x 128] scores of a chunk one row is used:
//                           16 x the needed work, DESIGN.md section 5 has the arithmetic.
//   rank_count_kernel<MT>   the grid and chunking of topk_select_kernel.  A wave owns 2 * MT users of the tile and holds their
//                           compacted target keys (lane j = target j) and counters in registers; per chunk and user it ballots
//                           "key of this news > key of target j" for the user's REAL targets only and adds the population
//                           counts.  No exclusion test here.  Each slice stores its own counts: integers, added in rank_final,
//                           so the result depends on neither `splits`, the user tile nor any arrival order.
//   rank_final_kernel       one wave per user, one lane per target: rank = 1 + sum of the slices' counts - excluded news that
//                           beat it; 0 and -inf for the not-ranked; the user's metric terms in fp64.
//   rank_reduce_kernel      fixed-order sum of the per-user terms into out_sums (as metrics_reduce_kernel of nr_data.hip).
//
// Group caps (include/nrhip.h K10: the rank in the capped ranking of nr_score_topk(..., group, group_cap)) need, per user and
// target, the number n_g of eligible news of EVERY group g that beat the target.  The GROUP instantiations add that to the same
// passes; a call without `group` launches the instantiations it always launched.
//   rank_group_masks_kernel once per call, independent of the users: for every chunk of 128 ids the counting pass will see (the
//                           chunk starts of its slices, v_lo = 1 + slice * per) and every group g, the two 64-bit masks "news
//                           of this chunk in group g".  A group id outside [0, G) sets no bit: such a news is ungrouped.
//   named kernels, GROUP    gather group[id] of the targets and of the excluded / listed ids; for every target slot j and listed
//                           news that beats it (in range, key != 0, once): counters[u, j, group] -= 1 (integer atomics into the
//                           zeroed [U, T, G] array), so what is not eligible uses up nothing of a cap.
//   rank_count_kernel<MT, POOL, GB>   GB = blocks of 64 groups, lane = group inside a block.  The ballots k0 > tk, k1 > tk are the
//                           128-bit "beats target j" mask in SGPRs; each lane ANDs it with its group's masks of the chunk and
//                           accumulates the population counts in registers [users of the wave][4 targets][GB]; once per slice
//                           they are added to counters[u, slot of target j, g] with integer atomics.  Integers: independent of
//                           `splits`, tile and arrival order.  The total count is untouched.
//   rank_final_group_kernel n_g from the counters; capped out (rank -1, score kept) when the target's own group has n_g >= c,
//                           else rank = uncapped - sum_g max(0, n_g - c); the metric terms as in rank_final_kernel.
#include <math.h>

#include "nr_score_tile.h"

namespace {

constexpr int RK_SLOTS = NR_RANK_MAX_TARGETS;     // chunk rows 0 .. 63: targets, 64 .. 127: excluded ids
constexpr int RK_MAX_SPLITS = 256;
static_assert(NR_RANK_MAX_TARGETS == 64 && NR_TOPK_MAX_EXCLUDE == 64 && TK_ROWS == 128, "one lane per target and per excluded id");

// keys and counters of the counting pass live in registers: the tile is what the vectors and the staging buffers leave room for
inline int rk_user_tile(int N) { return score_user_tile(N, 0); }
// group caps: blocks of 64 groups as the counting pass instantiates them (1, 2, 4, 8), and the user tile whose per-wave counters
// (TU / 8 users x 4 targets x blocks) are 64 registers or fewer
inline int rk_group_blocks(int G) {
  const int b = (G + 63) / 64;
  return b <= 1 ? 1 : b <= 2 ? 2 : b <= 4 ? 4 : 8;
}
inline int rk_group_user_tile(int N, int G) {
  const int tu = rk_user_tile(N), gb = rk_group_blocks(G), most = gb <= 2 ? 64 : gb == 4 ? 32 : 16;
  return tu < most ? tu : most;
}

// workspace: 8-byte arrays first
struct RankWs {
  u64* keys;        // [U, T]           keys of the ranked targets, compacted
  double* terms;    // [U, 2 + 2 n_ks]  counted, MRR_u, then Recall@k_u, nDCG@k_u per k
  int32_t* part;    // [U, splits, T]   per slice: news of the slice that beat compact target p
  int32_t* excl;    // [U, T]           distinct excluded news that beat compact target p
  int32_t* pos;     // [U, T]           target slot j -> compact index, -1 = not ranked
  int32_t* nu;      // [U]              ranked targets of the user
  size_t bytes;
};
inline RankWs rk_carve(void* ws, int U, int T, int n_ks, int splits) {
  RankWs w;
  char* p = reinterpret_cast<char*>(ws);
  const size_t ut = (size_t)U * T;
  w.keys = reinterpret_cast<u64*>(p); p += ut * sizeof(u64);
  w.terms = reinterpret_cast<double*>(p); p += (size_t)U * (2 + 2 * n_ks) * sizeof(double);
  w.part = reinterpret_cast<int32_t*>(p); p += ut * splits * sizeof(int32_t);
  w.excl = reinterpret_cast<int32_t*>(p); p += ut * sizeof(int32_t);
  w.pos = reinterpret_cast<int32_t*>(p); p += ut * sizeof(int32_t);
  w.nu = reinterpret_cast<int32_t*>(p); p += (size_t)U * sizeof(int32_t);
  w.bytes = (size_t)(p - reinterpret_cast<char*>(ws));
  return w;
}

// group caps: read by the GROUP instantiations only
struct GroupArgs {
  const int32_t* group;   // [V]
  const u64* masks;       // [splits * cps, G, 2]  news of chunk (slice, q) in group g: rows 0 .. 63, rows 64 .. 127
  int32_t* cnt;           // [U, T, G]             eligible news of group g that beat target slot j (zeroed, then atomics)
  int32_t* slot;          // [U, T]                compact index p -> target slot j
  int32_t* tgrp;          // [U, T]                group of target slot j, -1 = none
  int G, cap, cps;        // cps = chunks per slice
  // the group of news id (in [1, V)); an id outside [0, G) is "no group": nothing outside the workspace is ever addressed
  __device__ __forceinline__ int32_t of(int32_t id) const {
    const int32_t g = group[id];
    return (uint32_t)g < (uint32_t)G ? g : -1;
  }
};
// the last kernel argument: GroupArgs with caps, nothing without -- the arguments in front of it keep their places
struct NoGroupArgs {};
template <bool GROUP>
using GroupArgsIf = typename std::conditional<GROUP, GroupArgs, NoGroupArgs>::type;
template <bool GROUP>
GroupArgsIf<GROUP> group_args_if(const GroupArgs& ga) {
  if constexpr (GROUP) return ga;
  else return {};
}
inline GroupArgs rk_group_carve(void* ws, size_t at, int U, int T, int G, int splits, int cps, size_t* end) {
  GroupArgs g = {};
  char* p = reinterpret_cast<char*>(ws) + ((at + 7) & ~(size_t)7);
  const size_t ut = (size_t)U * T;
  g.masks = reinterpret_cast<const u64*>(p); p += (size_t)splits * cps * G * 2 * sizeof(u64);
  g.cnt = reinterpret_cast<int32_t*>(p); p += ut * G * sizeof(int32_t);
  g.slot = reinterpret_cast<int32_t*>(p); p += ut * sizeof(int32_t);
  g.tgrp = reinterpret_cast<int32_t*>(p); p += ut * sizeof(int32_t);
  *end = (size_t)(p - reinterpret_cast<char*>(ws));
  return g;
}

struct RankArgs {
  const float* news;
  const float* user;
  const int32_t* targets;
  const int32_t* exclude;
  RankWs w;
  size_t ld_news, ld_user, ld_tgt, ld_excl;
  int V, U, N, T, E, splits, per;
  PoolArgs pool;        // read by the POOL instantiations only
};

// POOL (both kernels): the call has a prior and / or stamps + windows; every key then comes from pool_key (nr_score_tile.h), as
// in topk_select_kernel<MT, true>.  A call without them launches the <false> kernels, the code as it was before pools existed.
// GROUP (all passes): the call has group caps, see the head of the file; `ga` is read by the GROUP instantiations only.
template <bool POOL, bool GROUP = false>
__global__ __launch_bounds__(TK_THREADS) void rank_named_kernel(RankArgs a, GroupArgsIf<GROUP> ga) {
  extern __shared__ __attribute__((aligned(16))) float rk_smem[];
  ScoreTile<1> t(rk_smem, a.N);
  int32_t* sIds = reinterpret_cast<int32_t*>(t.end());        // [16, 128]
  const int tid = t.tid, lane = t.lane, wave = t.wave;
  const int u0 = blockIdx.x * 16;
  const int users = a.U - u0 < 16 ? a.U - u0 : 16;

  t.load_users(a.user, a.ld_user, u0, a.U);
  for (int i = tid; i < 16 * TK_ROWS; i += TK_THREADS) {
    const int ul = i / TK_ROWS, s = i - ul * TK_ROWS;
    int32_t id = 0;
    if (ul < users) {
      if (s < a.T) id = a.targets[(size_t)(u0 + ul) * a.ld_tgt + s];
      else if (s >= RK_SLOTS && s - RK_SLOTS < a.E) id = a.exclude[(size_t)(u0 + ul) * a.ld_excl + s - RK_SLOTS];
    }
    sIds[i] = id;
  }
  __syncthreads();

  ScoreNamedRows rows = {a.news, a.ld_news, sIds, a.V};
  t.load_slab(rows, 0);
  for (int c = 0; c < users; ++c) {
    f32x4 acc[1];
    rows.ids = sIds + c * TK_ROWS;
    t.chunk(rows, acc);
    if (c + 1 < users) {
      rows.ids = sIds + (c + 1) * TK_ROWS;
      t.load_slab(rows, 0);
    }
    t.put_scores(acc);
    if (wave == 0) {
      const size_t u = (size_t)(u0 + c);
      const int32_t tg = sIds[c * TK_ROWS + lane], ex = sIds[c * TK_ROWS + RK_SLOTS + lane];
      const bool t_in = lane < a.T && tg >= 1 && tg < a.V, x_in = lane < a.E && ex >= 1 && ex < a.V;
      u64 kt, kx;
      if constexpr (POOL) {
        // prior and stamp gathered by id: the named news get the key the stream gives them -- 0 outside the user's pool.  Such a
        // target is not ranked; such an excluded news was never counted by the stream, so it must not be taken back either.
        const int32_t lo = a.pool.lo_of(u), hi = a.pool.hi_of(u);
        const uint32_t st = t_in ? pool_key(t.scores()[c * TK_LDS_TILE + lane], a.pool.prior_of(tg), a.pool.stamp_of(tg), lo, hi) : 0u;
        const uint32_t sx = x_in ? pool_key(t.scores()[c * TK_LDS_TILE + RK_SLOTS + lane], a.pool.prior_of(ex), a.pool.stamp_of(ex), lo, hi) : 0u;
        kt = ((u64)st << 32) | (uint32_t)~(uint32_t)tg;
        kx = ((u64)sx << 32) | (uint32_t)~(uint32_t)ex;
      } else {
        kt = news_key(t.scores()[c * TK_LDS_TILE + lane], (uint32_t)tg);
        kx = news_key(t.scores()[c * TK_LDS_TILE + RK_SLOTS + lane], (uint32_t)ex);
      }
      bool ranked = t_in && (kt >> 32) != 0;                  // a NaN score has key 0
      bool x_counts = x_in && (kx >> 32) != 0;                // a NaN news is never counted by the stream: nothing to take back
      for (int j = 0; j < RK_SLOTS; ++j) {
        const int32_t tj = __builtin_amdgcn_readlane(tg, j), xj = __builtin_amdgcn_readlane(ex, j);
        if (j < a.T && lane > j && tg == tj) ranked = false;  // repeats an earlier entry
        if (j < a.E && tg == xj) ranked = false;              // excluded
        if (j < a.E && lane > j && ex == xj) x_counts = false;   // each excluded news once
      }
      const u64 mask = __ballot(ranked);
      const int p = __popcll(mask & ((1ull << lane) - 1ull)), n = __popcll(mask);
      int beaten_by = 0;
      // GROUP: lane = excluded news: what the total takes back, its group takes back as well, per target slot
      int32_t gx = -1;
      if constexpr (GROUP) gx = x_counts ? ga.of(ex) : -1;
      for (int j = 0; j < a.T; ++j) {
        const bool beats = x_counts && kx > lane_u64(kt, j);
        const int cnt = __popcll(__ballot(beats));
        if (lane == j) beaten_by = cnt;
        if constexpr (GROUP) {
          if (beats && gx >= 0) atomicAdd(&ga.cnt[(u * a.T + j) * ga.G + gx], -1);
        }
      }
      if constexpr (GROUP) {
        if (lane < a.T) ga.tgrp[u * a.T + lane] = t_in ? ga.of(tg) : -1;
        if (ranked) ga.slot[u * a.T + p] = lane;
      }
      if (ranked) {
        a.w.keys[u * a.T + p] = kt;
        a.w.excl[u * a.T + p] = beaten_by;
      }
      if (lane < a.T) a.w.pos[u * a.T + lane] = ranked ? p : -1;
      if (lane == 0) a.w.nu[u] = n;
    }
    __syncthreads();                                          // the score tile is the next chunk's staging buffer
  }
}

// The ids of chunk q of a user into dst[0 .. 128): chunk 0 = its targets (rows 0 .. 63) and entries 0 .. 63 of its segment
// ids[b .. b + L) (rows 64 .. 127); chunk q >= 1 = entries 64 + 128 (q - 1) .. of the segment.  0 = no row.
__device__ __forceinline__ void rank_csr_stage(int32_t* dst, const RankArgs& a, const CsrArgs& ca, size_t u, int q, int32_t b, int32_t L, int tid) {
  if (tid >= TK_ROWS) return;
  int32_t id = 0;
  if (q == 0 && tid < RK_SLOTS) {
    if (tid < a.T) id = a.targets[u * a.ld_tgt + tid];
  } else {
    const long i = q == 0 ? tid - RK_SLOTS : (long)RK_SLOTS + (long)TK_ROWS * (q - 1) + tid;
    if (i < L) id = ca.ids[(long)b + i];
  }
  dst[tid] = id;
}

template <bool POOL, bool GROUP = false>
__global__ __launch_bounds__(TK_THREADS) void rank_named_csr_kernel(RankArgs a, CsrArgs ca, GroupArgsIf<GROUP> ga) {
  extern __shared__ __attribute__((aligned(16))) float rk_smem[];
  ScoreTile<1> t(rk_smem, a.N);
  int32_t* sIds = reinterpret_cast<int32_t*>(t.end());        // [2, 128]: this chunk's ids and the next one's
  const int tid = t.tid, lane = t.lane, wave = t.wave;
  const int u0 = blockIdx.x * 16;
  const int users = a.U - u0 < 16 ? a.U - u0 : 16;

  t.load_users(a.user, a.ld_user, u0, a.U);
  // the walk over (user c of the group, chunk q of its list); every thread keeps the same state
  int c = 0, q = 0, buf = 0;
  int32_t seg_b, seg_e;
  ca.segment(u0, seg_b, seg_e);
  int32_t L = seg_e - seg_b;
  rank_csr_stage(sIds, a, ca, (size_t)u0, 0, seg_b, L, tid);
  __syncthreads();

  ScoreNamedRows rows = {a.news, a.ld_news, sIds, a.V};
  t.load_slab(rows, 0);
  // wave 0, across the chunks of one user: lane j = target j
  int32_t tg = 0;
  u64 kt = 0ull;
  bool ranked = false;
  int beaten_by = 0;
  int32_t w_lo = 0, w_hi = 0;
  while (c < users) {
    // the chunk after this one: the user's next 128 entries, or chunk 0 of the next user
    const int nq = L > RK_SLOTS ? 1 + (int)(((long)L - RK_SLOTS + TK_ROWS - 1) / TK_ROWS) : 1;
    int c2 = c, q2 = q + 1;
    int32_t b2 = seg_b, L2 = L;
    if (q2 >= nq) {
      c2 = c + 1;
      q2 = 0;
      if (c2 < users) {
        int32_t e2;
        ca.segment(u0 + c2, b2, e2);
        L2 = e2 - b2;
      }
    }
    // staged now, read after the barriers inside chunk(); the buffer's readers finished before the barrier that ended the last turn
    if (c2 < users) rank_csr_stage(sIds + (buf ^ 1) * TK_ROWS, a, ca, (size_t)(u0 + c2), q2, b2, L2, tid);
    f32x4 acc[1];
    rows.ids = sIds + buf * TK_ROWS;
    t.chunk(rows, acc);
    if (c2 < users) {
      rows.ids = sIds + (buf ^ 1) * TK_ROWS;
      t.load_slab(rows, 0);
    }
    t.put_scores(acc);
    if (wave == 0) {
      const size_t u = (size_t)(u0 + c);
      const int32_t* ids = sIds + buf * TK_ROWS;
      const float* sS = t.scores() + c * TK_LDS_TILE;
      if (q == 0) {
        tg = ids[lane];
        const bool t_in = lane < a.T && tg >= 1 && tg < a.V;
        if constexpr (POOL) {
          w_lo = a.pool.lo_of(u);
          w_hi = a.pool.hi_of(u);
          const uint32_t st = t_in ? pool_key(sS[lane], a.pool.prior_of(tg), a.pool.stamp_of(tg), w_lo, w_hi) : 0u;
          kt = ((u64)st << 32) | (uint32_t)~(uint32_t)tg;
        } else
          kt = news_key(sS[lane], (uint32_t)tg);
        ranked = t_in && (kt >> 32) != 0;                     // a NaN score has key 0
        for (int j = 0; j < a.T; ++j)
          if (lane > j && tg == __builtin_amdgcn_readlane(tg, j)) ranked = false;   // repeats an earlier entry
        beaten_by = 0;
      }
      // the chunk's listed ids: rows lane (chunks >= 1 only) and lane + 64
      const int32_t xa = q == 0 ? 0 : ids[lane], xb = ids[lane + RK_SLOTS];
      const bool a_in = xa >= 1 && xa < a.V, b_in = xb >= 1 && xb < a.V;
      u64 ka, kb;
      if constexpr (POOL) {
        // prior and stamp gathered by id: a listed news gets the key the stream gives it -- 0 outside the user's pool, and then
        // it was never counted by the stream, so it must not be taken back either
        const uint32_t sa = a_in ? pool_key(sS[lane], a.pool.prior_of(xa), a.pool.stamp_of(xa), w_lo, w_hi) : 0u;
        const uint32_t sb = b_in ? pool_key(sS[lane + RK_SLOTS], a.pool.prior_of(xb), a.pool.stamp_of(xb), w_lo, w_hi) : 0u;
        ka = ((u64)sa << 32) | (uint32_t)~(uint32_t)xa;
        kb = ((u64)sb << 32) | (uint32_t)~(uint32_t)xb;
      } else {
        ka = news_key(sS[lane], (uint32_t)xa);
        kb = news_key(sS[lane + RK_SLOTS], (uint32_t)xb);
      }
      const bool a_counts = a_in && (ka >> 32) != 0, b_counts = b_in && (kb >> 32) != 0;   // a NaN news: nothing to take back
      // GROUP: what the total takes back, the listed news' group takes back as well, per target slot
      int32_t grp_a = -1, grp_b = -1;
      if constexpr (GROUP) {
        grp_a = a_counts ? ga.of(xa) : -1;
        grp_b = b_counts ? ga.of(xb) : -1;
      }
      for (int j = 0; j < a.T; ++j) {
        const int32_t tj = __builtin_amdgcn_readlane(tg, j);
        const u64 ktj = lane_u64(kt, j);
        const bool listed = __ballot((a_in && xa == tj) || (b_in && xb == tj)) != 0ull;
        const bool a_beats = a_counts && ka > ktj, b_beats = b_counts && kb > ktj;
        const int cnt = __popcll(__ballot(a_beats)) + __popcll(__ballot(b_beats));
        if (lane == j) {
          if (listed) ranked = false;
          beaten_by += cnt;
        }
        if constexpr (GROUP) {
          if (a_beats && grp_a >= 0) atomicAdd(&ga.cnt[(u * a.T + j) * ga.G + grp_a], -1);
          if (b_beats && grp_b >= 0) atomicAdd(&ga.cnt[(u * a.T + j) * ga.G + grp_b], -1);
        }
      }
      if (q + 1 >= nq) {                                      // the user's last chunk: compact and store
        const u64 mask = __ballot(ranked);
        const int p = __popcll(mask & ((1ull << lane) - 1ull)), n = __popcll(mask);
        if (ranked) {
          a.w.keys[u * a.T + p] = kt;
          a.w.excl[u * a.T + p] = beaten_by;
        }
        if (lane < a.T) a.w.pos[u * a.T + lane] = ranked ? p : -1;
        if (lane == 0) a.w.nu[u] = n;
        if constexpr (GROUP) {
          if (lane < a.T) ga.tgrp[u * a.T + lane] = tg >= 1 && tg < a.V ? ga.of(tg) : -1;
          if (ranked) ga.slot[u * a.T + p] = lane;
        }
      }
    }
    __syncthreads();                                          // the score tile is the next chunk's staging buffer
    c = c2; q = q2; seg_b = b2; L = L2; buf ^= 1;
  }
}

// One wave per (chunk of the counting pass, block of 64 groups), lane = group: the chunk's 128 group ids sit two per lane, and
// every lane collects the bits of the ids that are in its group.  Rows beyond the slice end set no bit.
__global__ __launch_bounds__(256) void rank_group_masks_kernel(const int32_t* __restrict__ group, u64* __restrict__ masks, int V, int G, int per,
                                                                int cps, int n_chunks) {
  const int lane = threadIdx.x & 63;
  const long ci = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ci >= n_chunks) return;
  const long slice = ci / cps, q = ci - slice * cps;
  const long v_lo = 1 + slice * per;
  const long v_hi = v_lo + per < V ? v_lo + per : V;
  const long vc = v_lo + q * TK_ROWS;
  const int32_t g0 = vc + lane < v_hi ? group[vc + lane] : -1, g1 = vc + lane + 64 < v_hi ? group[vc + lane + 64] : -1;
  const int32_t mine = (int32_t)blockIdx.y * 64 + lane;
  u64 m0 = 0ull, m1 = 0ull;
  for (int r = 0; r < 64; ++r) {
    if (__builtin_amdgcn_readlane(g0, r) == mine) m0 |= 1ull << r;
    if (__builtin_amdgcn_readlane(g1, r) == mine) m1 |= 1ull << r;
  }
  if (mine < G) {
    masks[((size_t)ci * G + mine) * 2] = m0;
    masks[((size_t)ci * G + mine) * 2 + 1] = m1;
  }
}

// GB = 0: no group caps, the kernel as it was before they existed.  GB >= 1: blocks of 64 groups, at most NR_RANK_MAX_CAPPED_TARGETS
// targets per row; the counters gcnt[user of the wave][target][block] stay in registers (lane = group), so the host picks the user
// tile that keeps PER_WAVE * 4 * GB at 64 registers or fewer.
template <int MT, bool POOL, int GB = 0>
__global__ __launch_bounds__(TK_THREADS) void rank_count_kernel(RankArgs a, GroupArgsIf<(GB > 0)> ga) {
  constexpr int TU = 16 * MT, PER_WAVE = TU / TK_WAVES;
  constexpr int TC = NR_RANK_MAX_CAPPED_TARGETS, GBN = GB > 0 ? GB : 1;
  extern __shared__ __attribute__((aligned(16))) float rk_smem[];
  ScoreTile<MT> t(rk_smem, a.N);
  const int lane = t.lane, wave = t.wave;
  const int u0 = blockIdx.x * TU;
  const long v_lo = 1 + (long)blockIdx.y * a.per;
  const long v_hi = v_lo + a.per < a.V ? v_lo + a.per : a.V;

  t.load_users(a.user, a.ld_user, u0, a.U);
  // user wave + 8 i of the tile: its n[i] compacted target keys, one per lane, and their counters
  u64 tkey[PER_WAVE];
  int32_t cnt[PER_WAVE];
  int n[PER_WAVE];
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int u = u0 + wave + TK_WAVES * i;
    n[i] = u < a.U ? __builtin_amdgcn_readfirstlane(a.w.nu[u]) : 0;
    tkey[i] = lane < n[i] ? a.w.keys[(size_t)u * a.T + lane] : ~0ull;
    cnt[i] = 0;
  }
  int32_t gcnt[GB > 0 ? PER_WAVE : 1][TC][GBN];
  int32_t slot[GB > 0 ? PER_WAVE : 1];
  if constexpr (GB > 0) {
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      const int u = u0 + wave + TK_WAVES * i;
      slot[i] = lane < n[i] ? ga.slot[(size_t)u * a.T + lane] : 0;
#pragma unroll
      for (int j = 0; j < TC; ++j)
#pragma unroll
        for (int b = 0; b < GB; ++b) gcnt[i][j][b] = 0;
    }
  }
  // POOL: lane i keeps the window of this wave's i-th user; an empty one beyond U
  int32_t w_lo = 1, w_hi = 0;
  if constexpr (POOL) {
    const int u = u0 + wave + TK_WAVES * lane;
    if (lane < PER_WAVE && u < a.U) {
      w_lo = a.pool.lo_of(u);
      w_hi = a.pool.hi_of(u);
    }
  }

  ScoreStreamRows rows = {a.news, a.ld_news, v_lo, v_hi};
  if (v_lo < v_hi) t.load_slab(rows, 0);
  for (long vc = v_lo; vc < v_hi; vc += TK_ROWS) {
    f32x4 acc[MT];
    rows.vc = vc;
    t.chunk(rows, acc);
    rows.vc = vc + TK_ROWS;
    if (rows.vc < v_hi) t.load_slab(rows, 0);                 // in flight while this chunk is counted
    // POOL: prior and stamp of the chunk's 128 news, two per lane, once per chunk and wave (coalesced; in flight over the barrier)
    float p0 = 0.f, p1 = 0.f;
    int32_t s0 = 0, s1 = 0;
    if constexpr (POOL) {
      if (vc + lane < v_hi) {
        p0 = a.pool.prior_of(vc + lane);
        s0 = a.pool.stamp_of(vc + lane);
      }
      if (vc + lane + 64 < v_hi) {
        p1 = a.pool.prior_of(vc + lane + 64);
        s1 = a.pool.stamp_of(vc + lane + 64);
      }
    }
    // GROUP: the chunk's masks of this lane's group in every block, once per chunk and wave (in flight over the barrier)
    u64 gm0[GBN], gm1[GBN];
    if constexpr (GB > 0) {
      const size_t ci = (size_t)blockIdx.y * ga.cps + (size_t)((vc - v_lo) / TK_ROWS);
#pragma unroll
      for (int b = 0; b < GB; ++b) {
        const int g = b * 64 + lane;
        gm0[b] = gm1[b] = 0ull;
        if (g < ga.G) {
          gm0[b] = ga.masks[(ci * ga.G + g) * 2];
          gm1[b] = ga.masks[(ci * ga.G + g) * 2 + 1];
        }
      }
    }
    t.put_scores(acc);
    const float* sS = t.scores();
    const int nvalid = (int)(v_hi - vc < TK_ROWS ? v_hi - vc : TK_ROWS);
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      if (n[i] == 0) continue;
      const int ul = wave + TK_WAVES * i;
      // rows beyond the slice end get key 0; a NaN score gives 0 << 32 | ~id, below every target's key
      u64 k0, k1;
      if constexpr (POOL) {
        // a news outside the user's pool gets 0 << 32 | ~id as well: it never beats a target
        const int32_t lo = __builtin_amdgcn_readlane(w_lo, i), hi = __builtin_amdgcn_readlane(w_hi, i);
        k0 = lane < nvalid ? ((u64)pool_key(sS[ul * TK_LDS_TILE + lane], p0, s0, lo, hi) << 32) | (uint32_t)~(uint32_t)(vc + lane) : 0ull;
        k1 = lane + 64 < nvalid ? ((u64)pool_key(sS[ul * TK_LDS_TILE + lane + 64], p1, s1, lo, hi) << 32) | (uint32_t)~(uint32_t)(vc + lane + 64) : 0ull;
      } else {
        k0 = lane < nvalid ? news_key(sS[ul * TK_LDS_TILE + lane], (uint32_t)(vc + lane)) : 0ull;
        k1 = lane + 64 < nvalid ? news_key(sS[ul * TK_LDS_TILE + lane + 64], (uint32_t)(vc + lane + 64)) : 0ull;
      }
      if constexpr (GB > 0) {
#pragma unroll
        for (int j = 0; j < TC; ++j) {
          if (j >= n[i]) break;
          const u64 tk = lane_u64(tkey[i], j);                // strict >: the target never counts itself
          const u64 b0 = __ballot(k0 > tk), b1 = __ballot(k1 > tk);      // the 128 news of the chunk that beat target j
          cnt[i] += lane == j ? __popcll(b0) + __popcll(b1) : 0;
#pragma unroll
          for (int b = 0; b < GB; ++b)
            if (b * 64 < ga.G) gcnt[i][j][b] += __popcll(b0 & gm0[b]) + __popcll(b1 & gm1[b]);
        }
      } else {
        for (int j = 0; j < n[i]; ++j) {
          const u64 tk = lane_u64(tkey[i], j);                  // strict >: the target never counts itself
          const int c = __popcll(__ballot(k0 > tk)) + __popcll(__ballot(k1 > tk));
          cnt[i] += lane == j ? c : 0;
        }
      }
    }
    __syncthreads();                                          // the score tile is the next chunk's staging buffer
  }
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int u = u0 + wave + TK_WAVES * i;
    if (u < a.U && lane < n[i]) a.w.part[((size_t)u * a.splits + blockIdx.y) * a.T + lane] = cnt[i];
  }
  if constexpr (GB > 0) {
    // this slice's per-group counts into the [U, T, G] counters: integer atomics, any order gives the same sum
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      const int u = u0 + wave + TK_WAVES * i;
#pragma unroll
      for (int j = 0; j < TC; ++j) {
        if (j >= n[i]) break;                                 // n[i] = 0 beyond U
        const int sj = __builtin_amdgcn_readlane(slot[i], j);
#pragma unroll
        for (int b = 0; b < GB; ++b) {
          const int g = b * 64 + lane;
          if (g < ga.G && gcnt[i][j][b] != 0) atomicAdd(&ga.cnt[((size_t)u * a.T + sj) * ga.G + g], gcnt[i][j][b]);
        }
      }
    }
  }
}

struct RankKs {
  int n;
  int k[NR_RANK_MAX_KS];
};

// MRR_u = mean 1 / rank; Recall@k_u = #{rank <= k} / n; nDCG@k_u = sum_{rank <= k} 1 / log2(rank + 1) over the ideal
// sum_{i <= min(n, k)} 1 / log2(i + 1): src/metrics.py:6-24 on the user's whole eligible row with binary labels.  One wave per
// user, lane = target slot; n = the user's ranked targets.  A rank <= 0 adds nothing (0: not ranked; -1: capped out, counted in n).
__device__ __forceinline__ void rank_terms(const RankWs& w, size_t u, int lane, int n, int rank, const RankKs& ks) {
  double* o = w.terms + u * (2 + 2 * ks.n);
  const double gain = rank > 0 ? 1.0 / log2((double)rank + 1.0) : 0.0, ideal = 1.0 / log2((double)lane + 2.0);
  const double rr = wave_sum_d(rank > 0 ? 1.0 / (double)rank : 0.0);
  if (lane == 0) {
    o[0] = n > 0 ? 1.0 : 0.0;
    o[1] = n > 0 ? rr / n : 0.0;
  }
  for (int i = 0; i < ks.n; ++i) {
    const bool hit = rank > 0 && rank <= ks.k[i];
    const int hits = __popcll(__ballot(hit));
    const double dcg = wave_sum_d(hit ? gain : 0.0), idcg = wave_sum_d(lane < n && lane < ks.k[i] ? ideal : 0.0);
    if (lane == 0) {
      o[2 + 2 * i] = n > 0 ? (double)hits / n : 0.0;
      o[3 + 2 * i] = n > 0 ? dcg / idcg : 0.0;
    }
  }
}

__global__ __launch_bounds__(256) void rank_final_kernel(RankWs w, int U, int T, int splits, RankKs ks, int want_terms, int32_t* __restrict__ out_ranks,
                                                          float* __restrict__ out_scores) {
  const int lane = threadIdx.x & 63;
  const size_t u = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= (size_t)U) return;
  const int n = w.nu[u];
  int rank = 0;
  float score = -__builtin_inff();
  if (lane < T) {
    const int p = w.pos[u * T + lane];
    if (p >= 0) {
      int c = -w.excl[u * T + p];
      for (int s = 0; s < splits; ++s) c += w.part[(u * splits + s) * T + p];
      rank = 1 + c;
      score = key_score((uint32_t)(w.keys[u * T + p] >> 32));
    }
    out_ranks[u * T + lane] = rank;
    out_scores[u * T + lane] = score;
  }
  if (!want_terms) return;
  rank_terms(w, u, lane, n, rank, ks);
}

// The finalize pass of a call with group caps.  counters[u, j, g] = n_g of target slot j (stream count minus what the named
// pass took back).  Capped out: the target's own group already has c news in front of it -- rank -1, the score stays.  Otherwise
// every group gives back what it has beyond c: rank = uncapped - sum_g max(0, n_g - c).  n (the ranked targets, capped-out ones
// included) and the metric terms are rank_final_kernel's; a rank of -1 is no hit and adds no reciprocal rank.
__global__ __launch_bounds__(256) void rank_final_group_kernel(RankWs w, const int32_t* __restrict__ gcnt, const int32_t* __restrict__ tgrp, int G, int cap,
                                                                int U, int T, int splits, RankKs ks, int want_terms, int32_t* __restrict__ out_ranks,
                                                                float* __restrict__ out_scores) {
  const int lane = threadIdx.x & 63;
  const size_t u = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= (size_t)U) return;
  const int n = w.nu[u];
  int over = 0;
  for (int j = 0; j < T; ++j) {
    int o = 0;
    for (int g = lane; g < G; g += 64) {
      const int ng = gcnt[(u * T + j) * G + g];
      o += ng > cap ? ng - cap : 0;
    }
    o = wave_sum_i(o);
    if (lane == j) over = o;
  }
  int rank = 0;
  float score = -__builtin_inff();
  if (lane < T) {
    const int p = w.pos[u * T + lane];
    if (p >= 0) {
      int c = -w.excl[u * T + p];
      for (int s = 0; s < splits; ++s) c += w.part[(u * splits + s) * T + p];
      const int gt = tgrp[u * T + lane];
      const bool capped_out = gt >= 0 && gcnt[(u * T + lane) * G + gt] >= cap;
      rank = capped_out ? -1 : 1 + c - over;
      score = key_score((uint32_t)(w.keys[u * T + p] >> 32));
    }
    out_ranks[u * T + lane] = rank;
    out_scores[u * T + lane] = score;
  }
  if (!want_terms) return;
  rank_terms(w, u, lane, n, rank, ks);
}

// fixed-order reduction of the per-user terms: sums[c] = sum_u terms[u, c]
__global__ __launch_bounds__(1024) void rank_reduce_kernel(const double* __restrict__ terms, int U, int W, double* __restrict__ sums) {
  __shared__ double sh[2 + 2 * NR_RANK_MAX_KS][16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int c = 0; c < W; ++c) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < U; i += 1024) acc += terms[(size_t)i * W + c];
    acc = wave_sum_d(acc);
    if (lane == 0) sh[c][wid] = acc;
  }
  __syncthreads();
  if ((int)threadIdx.x < W) {
    double v = 0.0;
    for (int k = 0; k < 16; ++k) v += sh[threadIdx.x][k];
    sums[threadIdx.x] = v;
  }
}

// argument checks shared by the size query and the call; 0 = fine
int rank_check(const nr_rank_desc* d) {
  NR_CHECK_ARG(d != nullptr, "score_rank: null descriptor");
  NR_CHECK_ARG(d->T >= 1 && d->T <= NR_RANK_MAX_TARGETS, "score_rank: T = %d targets per user, must be in [1, %d]", d->T, NR_RANK_MAX_TARGETS);
  NR_CHECK_RC(check_vectors("score_rank", d->V, d->U, d->N));
  NR_CHECK_RC(check_lists("score_rank", d->E, d->excl_offsets, d->excl_ids, d->n_excl));
  NR_CHECK_ARG(d->n_ks >= 0 && d->n_ks <= NR_RANK_MAX_KS, "score_rank: n_ks = %d cut-offs, at most %d", d->n_ks, NR_RANK_MAX_KS);
  NR_CHECK_ARG(d->n_ks == 0 || d->ks != nullptr, "score_rank: null pointer (ks) with n_ks = %d", d->n_ks);
  for (int i = 0; i < d->n_ks; ++i) NR_CHECK_ARG(d->ks[i] >= 1, "score_rank: cut-off k = %d at position %d, must be >= 1", d->ks[i], i);
  NR_CHECK_ARG(d->splits >= 0 && d->splits <= RK_MAX_SPLITS, "score_rank: splits = %d, must be 0 (library's choice) or in [1, %d]", d->splits,
               RK_MAX_SPLITS);
  NR_CHECK_RC(check_pools("score_rank", d->stamp, d->window, d->ld_window));
  NR_CHECK_ARG(d->group == nullptr || (d->group_cap >= 1 && d->group_cap <= NR_TOPK_MAX_K),
               "score_rank: group given with group_cap = %d, the cap must be in [1, %d]", d->group_cap, NR_TOPK_MAX_K);
  NR_CHECK_ARG(d->group != nullptr || d->group_cap == 0, "score_rank: group_cap = %d given without group (the two come together)", d->group_cap);
  NR_CHECK_ARG(d->group != nullptr || d->n_groups == 0, "score_rank: n_groups = %d given without group (the two come together)", d->n_groups);
  NR_CHECK_ARG(d->group == nullptr || (d->n_groups >= 1 && d->n_groups <= NR_RANK_MAX_GROUPS),
               "score_rank: group given with n_groups = %d, must be in [1, %d]", d->n_groups, NR_RANK_MAX_GROUPS);
  NR_CHECK_ARG(d->group == nullptr || d->T <= NR_RANK_MAX_CAPPED_TARGETS,
               "score_rank: T = %d targets per row with group caps, at most %d (lay a user with more over several rows)", d->T,
               NR_RANK_MAX_CAPPED_TARGETS);
  return NR_OK;
}

// slices, slice length and chunks per slice of a call; with group caps the user tile, and with it the library's choice of slices, is
// the capped one
struct RankPlan {
  int TU, splits, per, cps;
};
inline RankPlan rk_plan(const nr_rank_desc* d) {
  RankPlan p;
  const bool grp = d->group != nullptr;
  p.TU = grp ? rk_group_user_tile(d->N, d->n_groups) : rk_user_tile(d->N);
  p.splits = d->splits > 0 ? d->splits : score_auto_splits(d->U, d->V, p.TU, RK_MAX_SPLITS);
  p.per = (int)(((long)d->V - 1 + p.splits - 1) / p.splits);
  p.cps = (p.per + TK_ROWS - 1) / TK_ROWS;
  return p;
}

// the named passes: f(POOL, GROUP) launches its kernel's instantiation
template <class F>
int rank_named_launch(bool pool, bool grp, F&& f) {
  return with_bool(pool, [&](auto p) { return with_bool(grp, [&](auto g) { return f(p, g); }); });
}
// The counting pass for the run-time (tile, pool, blocks of 64 groups; 0 = no caps).  With caps the per-wave counters (TU / 8
// users x 4 targets x blocks) stay within 64 registers, so MT * GB <= 8 (rk_group_user_tile picks the tile accordingly): the
// capped kernel exists for (TU, GB) in {64, 32, 16} x {1, 2}, {32, 16} x {4} and {16} x {8}.
int rank_count_launch(int TU, bool pool, int gb, dim3 grid, size_t smem, hipStream_t s, const RankArgs& a, const GroupArgs& ga) {
  return with_int<64, 32, 16>(TU, [&](auto tu) {
    return with_bool(pool, [&](auto p) {
      return with_int<0, 1, 2, 4, 8>(gb, [&](auto b) {
        constexpr int MT = decltype(tu)::value / 16, GB = decltype(b)::value;
        if constexpr (MT * GB > 8) return (int)NR_ERR_ARG;   // not reached
        else return launch_lds(rank_count_kernel<MT, decltype(p)::value, GB>, grid, dim3(TK_THREADS), smem, s, a, group_args_if<(GB > 0)>(ga));
      });
    });
  });
}

}  // namespace

extern "C" {

size_t nr_score_rank_workspace_bytes(const nr_rank_desc* d) {
  if (rank_check(d) != NR_OK) return 0;
  const RankPlan pl = rk_plan(d);
  size_t bytes = rk_carve(nullptr, d->U, d->T, d->n_ks, pl.splits).bytes;
  if (d->group != nullptr) rk_group_carve(nullptr, bytes, d->U, d->T, d->n_groups, pl.splits, pl.cps, &bytes);
  return bytes;
}

int nr_score_rank(const nr_rank_desc* d, nr_stream_t stream) {
  NR_CHECK_RC(rank_check(d));
  NR_CHECK_ARG(d->news_vecs && d->user && d->targets && d->out_ranks && d->out_scores,
               "score_rank: null pointer (news_vecs, user, targets, out_ranks, out_scores)");
  NR_CHECK_RC(check_rows("score_rank", d->news_vecs, d->ld_news, d->user, d->ld_user, d->N));
  NR_CHECK_ARG(d->ld_targets >= d->T, "score_rank: target row stride %d < T = %d", d->ld_targets, d->T);
  NR_CHECK_ARG(d->E == 0 || d->exclude == nullptr || d->ld_exclude >= d->E, "score_rank: exclusion row stride %d < E = %d", d->ld_exclude, d->E);
  NR_CHECK_RC(check_workspace("score_rank", d->ws, d->ws_bytes, nr_score_rank_workspace_bytes(d)));
  NR_DEVICE_GUARD(stream, d->news_vecs);
  hipStream_t s = (hipStream_t)stream;
  const RankPlan pl = rk_plan(d);
  const int splits = pl.splits, TU = pl.TU;
  const bool grp = d->group != nullptr;
  RankArgs a;
  a.news = d->news_vecs; a.user = d->user; a.targets = d->targets;
  a.exclude = d->exclude;
  a.w = rk_carve(d->ws, d->U, d->T, d->n_ks, splits);
  a.ld_news = (size_t)d->ld_news; a.ld_user = (size_t)d->ld_user; a.ld_tgt = (size_t)d->ld_targets; a.ld_excl = (size_t)d->ld_exclude;
  a.V = d->V; a.U = d->U; a.N = d->N; a.T = d->T; a.E = d->exclude != nullptr ? d->E : 0; a.splits = splits;
  a.per = pl.per;
  GroupArgs ga = {};
  if (grp) {
    size_t end;
    ga = rk_group_carve(d->ws, a.w.bytes, d->U, d->T, d->n_groups, splits, pl.cps, &end);
    ga.group = d->group; ga.G = d->n_groups; ga.cap = d->group_cap; ga.cps = pl.cps;
    const int n_chunks = splits * pl.cps, gb = (d->n_groups + 63) / 64;
    NrProfScope ps(s, "rank_group_masks[V=%d,G=%d,chunks=%d]", d->V, d->n_groups, n_chunks);
    NR_CHECK_HIP(hipMemsetAsync(ga.cnt, 0, (size_t)d->U * d->T * d->n_groups * sizeof(int32_t), s));
    hipLaunchKernelGGL(rank_group_masks_kernel, dim3((unsigned)((n_chunks + 3) / 4), (unsigned)gb), dim3(256), 0, s, d->group,
                       const_cast<u64*>(ga.masks), d->V, d->n_groups, pl.per, pl.cps, n_chunks);
    NR_CHECK_LAUNCH();
  }
  a.pool = pool_args(d->prior, d->stamp, d->window, d->ld_window);
  const bool pool = a.pool.any();
  const CsrArgs ca = csr_args(d->excl_offsets, d->excl_ids, d->n_excl);
  const dim3 named_grid((unsigned)((d->U + 15) / 16));
  if (ca.offsets != nullptr) {
    NrProfScope ps(s, "rank_named_csr[U=%d,N=%d,T=%d,n_excl=%d]", d->U, d->N, d->T, d->n_excl);
    const size_t smem = tk_tile_bytes(16, d->N) + (size_t)2 * TK_ROWS * sizeof(int32_t);
    NR_CHECK_RC(rank_named_launch(pool, grp, [&](auto p, auto g) {
      return launch_lds(rank_named_csr_kernel<p.value, g.value>, named_grid, dim3(TK_THREADS), smem, s, a, ca, group_args_if<g.value>(ga));
    }));
  } else {
    NrProfScope ps(s, "rank_named[U=%d,N=%d,T=%d,E=%d]", d->U, d->N, d->T, a.E);
    const size_t smem = tk_tile_bytes(16, d->N) + (size_t)16 * TK_ROWS * sizeof(int32_t);
    NR_CHECK_RC(rank_named_launch(pool, grp, [&](auto p, auto g) {
      return launch_lds(rank_named_kernel<p.value, g.value>, named_grid, dim3(TK_THREADS), smem, s, a, group_args_if<g.value>(ga));
    }));
  }
  NR_CHECK_LAUNCH();
  {
    const size_t smem = tk_tile_bytes(TU, d->N);
    const dim3 grid((unsigned)((d->U + TU - 1) / TU), (unsigned)splits);
    NrProfScope ps(s, "rank_count[U=%d,V=%d,N=%d,T=%d,TU=%d,splits=%d]", d->U, d->V, d->N, d->T, TU, splits);
    NR_CHECK_RC(rank_count_launch(TU, pool, grp ? rk_group_blocks(d->n_groups) : 0, grid, smem, s, a, ga));
  }
  NR_CHECK_LAUNCH();
  RankKs ks;
  ks.n = d->n_ks;
  for (int i = 0; i < NR_RANK_MAX_KS; ++i) ks.k[i] = i < d->n_ks ? d->ks[i] : 1;
  {
    NrProfScope ps(s, "rank_final[U=%d,T=%d,splits=%d]", d->U, d->T, splits);
    if (grp)
      hipLaunchKernelGGL(rank_final_group_kernel, dim3((unsigned)((d->U + 3) / 4)), dim3(256), 0, s, a.w, (const int32_t*)ga.cnt, (const int32_t*)ga.tgrp,
                         d->n_groups, d->group_cap, d->U, d->T, splits, ks, d->out_sums != nullptr ? 1 : 0, d->out_ranks, d->out_scores);
    else
      hipLaunchKernelGGL(rank_final_kernel, dim3((unsigned)((d->U + 3) / 4)), dim3(256), 0, s, a.w, d->U, d->T, splits, ks, d->out_sums != nullptr ? 1 : 0,
                         d->out_ranks, d->out_scores);
    if (d->out_sums != nullptr)
      hipLaunchKernelGGL(rank_reduce_kernel, dim3(1), dim3(1024), 0, s, (const double*)a.w.terms, d->U, 2 + 2 * d->n_ks, d->out_sums);
  }
  NR_CHECK_LAUNCH();
  return NR_OK;
}

}  // extern "C"
