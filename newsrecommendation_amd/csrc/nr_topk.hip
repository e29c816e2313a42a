// Full-corpus top-k recommendation: score[u, v] = <news_vecs[v], user[u]> over the WHOLE news table and, per user, the k best
// news under the total order (score descending, news id ascending) -- without the [U, V] score matrix ever existing.
//
// The scoring tile (ScoreTile<MT>), the keys, the shared argument checks and the plan helpers are nr_score_tile.h: one definition,
// one set of bits for this unit, nr_rank.hip and nr_logz.hip.
//
//   topk_select_kernel<MT>  grid = user tiles x corpus slices, 8 waves.  A workgroup keeps its TU = 16 * MT users' vectors in
//                           LDS and streams its slice of the table through LDS in chunks of 128 news rows (k-slabs of 32
//                           columns, double buffered through registers).  Wave w forms the [TU x 16] score tile of news rows
//                           16w .. 16w + 15 of the chunk on v_mfma_f32_16x16x4_f32; one (u, v) score is ONE fmaf chain over
//                           the vector width in a fixed order (k-slab, sub-step e, MFMA k-group), whatever the tile, slice or
//                           user-tile size, so its bits do not depend on where it falls.  The chunk's scores go through an
//                           LDS tile (32 KiB per 6.5 MFLOP of MFMA work) so that ONE wave sees all 128 scores of a user: it
//                           compares them with that user's running k-th-best threshold and ballots; nothing passes in the
//                           common case.  What passes is checked against the exclusion list and replaces the worst of
//                           the user's k candidates (two per lane, in registers; a wave-wide minimum finds the next worst).
//                           With a prior and / or stamps + windows (the POOL instantiation) a wave also reads the prior and
//                           stamp of the chunk's 128 news once per chunk, and the keys come from pool_key (nr_score_tile.h):
//                           fl32(dot + prior), 0 for a news outside the user's pool -- before the ballot, so everything after
//                           it is unchanged.
//   topk_merge_kernel       one workgroup per user: bitonic sort of the splits * k candidates in LDS, the first k written out.
//
// Group caps ("at most c news of one group in the row", include/nrhip.h K9; the GROUP instantiation of the selection and
// topk_merge_group_kernel).  The rows that respect the caps are the independent sets of a partition matroid truncated at k,
// keys are distinct, so the greedy row is the unique maximum basis and inserting one candidate x of group g is ONE exchange:
//   g >= 0 and the list holds c keys of g:  x replaces the smallest of those c if it beats it, else it is dropped;
//   otherwise, the list is not full:        x is inserted;
//   otherwise:                              x replaces the overall smallest key (it beat the threshold, so it beats that).
// The threshold stays the score key of the OVERALL worst kept candidate (0 while the list is not full): a saturated group's
// minimum is >= it, so the fast test remains a correct filter; only the slow path changes.  The groups of the kept candidates
// are not stored: a slow-path entry re-gathers group[~id] for its two slots per lane, together with the groups of the
// chunk's 128 news (coalesced) and beside the exclusion row that entry always read -- one memory latency, already paid --
// so the LDS bytes, the user tile and with them the slice count and the workspace size are those of the plain call.
// The capped row of the whole corpus lies in the union of the slices' capped rows (a key outside its slice's basis is the
// minimum of a circuit inside it), so the merge is the same greedy walk over the sorted splits * k keys.
//
// Exclusion lists of any length (CSR, include/nrhip.h K9; the CSR instantiation of the selection).  The dense list is one id
// per lane, read at every slow-path entry; a list of hundreds or thousands of ids does not fit a register row, but a chunk
// covers the ids [vc, vc + 128) and the user's segment is strictly ascending, so at most 128 of its entries can matter to one
// entry.  The entry finds the lower bound of vc in the segment (csr_lower_bound: 64 probes a step, the range narrowed by the
// count of probes < vc, ceil(log64 L) dependent loads), loads the 128 entries from there, two per lane, and keeps those below
// vc + 128; the per-candidate test is then a ballot over two registers.  The fast path, the exchange, the LDS bytes, the user
// tile, the slices, the workspace and the merge kernels are untouched.  A user whose list covers nearly the whole corpus never
// fills its candidates: its threshold stays 0 and every chunk takes the slow path for it -- exact, but slow.
//
// A candidate is one 64-bit key: (order-preserving image of the score) << 32 | ~id.  Larger key = better; key 0 = "nothing"
// (NaN scores map to it and are never kept; it decodes to id 0, score -inf, the fill of a short row).  Ids of a slice arrive in
// ascending order, so a score that only TIES the threshold can never displace a kept one: the fast test is a strict >.
#include "nr_score_tile.h"

namespace {

constexpr int TK_MERGE_MAX = 8192;  // candidates one merge workgroup sorts in LDS (64 KiB)

// beside the tile a user keeps its k candidates and its threshold in LDS
inline size_t tk_user_bytes(int k) { return (size_t)k * sizeof(u64) + sizeof(uint32_t); }
inline size_t tk_lds_bytes(int TU, int N, int k) { return tk_tile_bytes(TU, N) + TU * tk_user_bytes(k); }
inline int tk_max_splits(int k) { return TK_MERGE_MAX / k < 256 ? TK_MERGE_MAX / k : 256; }
// user tile and slices of a call: the caller's `splits`, or enough to fill the chip within what one merge workgroup sorts
struct TopkPlan {
  int TU, splits;
};
inline TopkPlan tk_plan(const nr_topk_desc* d) {
  TopkPlan p;
  p.TU = score_user_tile(d->N, tk_user_bytes(d->k));
  p.splits = d->splits > 0 ? d->splits : score_auto_splits(d->U, d->V, p.TU, tk_max_splits(d->k));
  return p;
}

__device__ __forceinline__ u64 wave_min_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

struct TopkArgs {
  const float* news;
  const float* user;
  const int32_t* exclude;
  u64* part;              // [U, splits, k]
  size_t ld_news, ld_user, ld_excl;
  int V, U, N, k, E, splits, per;
  PoolArgs pool;          // read by the POOL instantiations only
};
// A kernel argument of its own, behind TopkArgs: the kernel argument segment of a call without caps keeps its layout up to there.
struct GroupArgs {
  const int32_t* group;   // [V], read by the GROUP instantiations only
  int cap;
};

// Lower bound of vc in ids[lo .. hi), ascending: lo + the number of entries < vc.  All 64 lanes call it with the same arguments.
// While the range holds more than one load (128 entries, two per lane) lane l probes position lo + n (l + 1) / 65 -- 64
// distinct positions inside the range -- and c, the count of probes < vc, narrows it to the gap between probe c - 1 and probe
// c.  Every index read lies in [lo, hi) of the call, sorted input or not.  tests/test_exclusion_lists_host.py holds this
// arithmetic as a numpy model, statement for statement.
__device__ __forceinline__ int32_t csr_lower_bound(const int32_t* __restrict__ ids, int32_t lo, int32_t hi, int32_t vc, int lane) {
  while (hi - lo > TK_ROWS) {
    const long n = hi - lo;
    const int32_t probe = lo + (int32_t)(n * (lane + 1) / 65);
    const int c = __popcll(__ballot(ids[probe] < vc));
    const int32_t last_below = lo + (int32_t)(n * c / 65), first_not = lo + (int32_t)(n * (c + 1) / 65);   // probes c - 1 and c
    if (c < 64) hi = first_not;
    if (c > 0) lo = last_below + 1;
  }
  const int32_t n = hi - lo;
  const bool b0 = lane < n && ids[lo + lane] < vc, b1 = lane + 64 < n && ids[lo + lane + 64] < vc;
  return lo + __popcll(__ballot(b0)) + __popcll(__ballot(b1));
}

// the slow path's group registers: of the kept candidates (g0, g1: an empty slot and a slot >= k belong to no group) and of
// the chunk's news (n0, n1), two per lane each; nothing at all in a kernel without caps
template <bool GROUP>
struct GroupRegs {
  int32_t g0 = -1, g1 = -1, n0 = -1, n1 = -1;
};
template <>
struct GroupRegs<false> {};

// POOL: the call has a prior and / or stamps + windows; the keys then come from pool_key (nr_score_tile.h).  A call without
// them launches <MT, false, .>, the kernel as it was before pools existed.  GROUP: the call has group caps (the exchange
// rule at the top of this file); a call without them launches <MT, ., false, .>, the kernel as it was before caps existed.
// CSR: the call has exclusion lists in CSR form (a kernel argument of its own again, behind GroupArgs) and no dense list; a
// call without them launches <MT, ., ., false, .>, the kernel as it was before the lists existed.
// SAMPLE: the sampled call (nr_score_sample, include/nrhip.h K12; its arguments behind CsrArgs once more).  It implies POOL and
// changes ONE thing: the keys come from sample_key (nr_score_tile.h), pool_key fed a prior perturbed by tau_u * Gumbel noise
// made in registers.  Caps, lists, slices and the merge see keys as before.  Every other call launches <MT, ., ., ., false>.
template <int MT, bool POOL, bool GROUP, bool CSR, bool SAMPLE>
__global__ __launch_bounds__(TK_THREADS) void topk_select_kernel(TopkArgs a, GroupArgs ga, CsrArgs ca, SampleArgs sa) {
  static_assert(POOL || !SAMPLE, "the sampled keys are pool keys");
  constexpr int TU = 16 * MT;
  extern __shared__ __attribute__((aligned(16))) float tk_smem[];
  ScoreTile<MT> t(tk_smem, a.N);                         // scoring tile: nr_score_tile.h
  u64* sList = reinterpret_cast<u64*>(t.end());          // [TU, k]  candidates, 0 = empty
  uint32_t* sThr = reinterpret_cast<uint32_t*>(sList + (size_t)TU * a.k);   // [TU]  score key of the worst candidate (0: not full)

  const int tid = t.tid, lane = t.lane, wave = t.wave;
  const int u0 = blockIdx.x * TU;
  const long v_lo = 1 + (long)blockIdx.y * a.per;
  const long v_hi = v_lo + a.per < a.V ? v_lo + a.per : a.V;

  t.load_users(a.user, a.ld_user, u0, a.U);
  for (int i = tid; i < TU * a.k; i += TK_THREADS) sList[i] = 0ull;
  if (tid < TU) sThr[tid] = 0u;

  // POOL: lane i keeps the window of this wave's i-th user (tile user wave + 8 i); an empty one beyond U
  int32_t w_lo = 1, w_hi = 0;
  if constexpr (POOL) {
    const int ul = wave + TK_WAVES * lane;
    if (ul < TU && u0 + ul < a.U) {
      w_lo = a.pool.lo_of(u0 + ul);
      w_hi = a.pool.hi_of(u0 + ul);
    }
  }

  // SAMPLE: lane i keeps tau and the counter word of this wave's i-th user; a tau that is negative, NaN or infinite empties
  // the user's window: every key 0, an all-fill row
  float tau_l = 0.f;
  uint32_t key_l = 0u;
  if constexpr (SAMPLE) {
    const int ul = wave + TK_WAVES * lane;
    if (ul < TU && u0 + ul < a.U) {
      tau_l = sa.tau_of(u0 + ul);
      key_l = sa.key_of(u0 + ul);
      if (!(tau_l >= 0.f && tau_l < __builtin_inff())) {
        tau_l = 0.f;
        w_lo = 1;
        w_hi = 0;
      }
    }
  }

  // CSR: lane i keeps the segment [x_lo, x_hi) of this wave's i-th user, clamped; an empty one beyond U
  int32_t x_lo = 0, x_hi = 0;
  if constexpr (CSR) {
    const int ul = wave + TK_WAVES * lane;
    if (ul < TU && u0 + ul < a.U) ca.segment(u0 + ul, x_lo, x_hi);
  }

  ScoreStreamRows rows = {a.news, a.ld_news, v_lo, v_hi};
  if (v_lo < v_hi) t.load_slab(rows, 0);
  for (long vc = v_lo; vc < v_hi; vc += TK_ROWS) {
    f32x4 acc[MT];
    rows.vc = vc;
    t.chunk(rows, acc);
    rows.vc = vc + TK_ROWS;
    if (rows.vc < v_hi) t.load_slab(rows, 0);                 // in flight while this chunk is selected from
    const int nvalid = (int)(v_hi - vc < TK_ROWS ? v_hi - vc : TK_ROWS);
    // POOL: prior and stamp of the chunk's 128 news, two per lane, once per chunk and wave (coalesced; in flight over the barrier)
    float p0 = 0.f, p1 = 0.f;
    int32_t s0 = 0, s1 = 0;
    if constexpr (POOL) {
      if (lane < nvalid) {
        p0 = a.pool.prior_of(vc + lane);
        s0 = a.pool.stamp_of(vc + lane);
      }
      if (lane + 64 < nvalid) {
        p1 = a.pool.prior_of(vc + lane + 64);
        s1 = a.pool.stamp_of(vc + lane + 64);
      }
    }
    t.put_scores(acc);
    const float* sS = t.scores();

    for (int ul = wave, iu = 0; ul < TU && u0 + ul < a.U; ul += TK_WAVES, ++iu) {
      uint32_t k0, k1;
      if constexpr (SAMPLE) {
        const int32_t lo = __builtin_amdgcn_readlane(w_lo, iu), hi = __builtin_amdgcn_readlane(w_hi, iu);
        const float tau = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tau_l), iu));
        const uint32_t ukey = (uint32_t)__builtin_amdgcn_readlane((int)key_l, iu), t0 = sThr[ul];
        k0 = lane < nvalid ? sample_key(sS[ul * TK_LDS_TILE + lane], p0, s0, lo, hi, tau, sa, ukey, (uint32_t)(vc + lane), t0) : 0u;
        k1 = lane + 64 < nvalid ? sample_key(sS[ul * TK_LDS_TILE + lane + 64], p1, s1, lo, hi, tau, sa, ukey, (uint32_t)(vc + lane + 64), t0) : 0u;
      } else if constexpr (POOL) {
        const int32_t lo = __builtin_amdgcn_readlane(w_lo, iu), hi = __builtin_amdgcn_readlane(w_hi, iu);
        k0 = lane < nvalid ? pool_key(sS[ul * TK_LDS_TILE + lane], p0, s0, lo, hi) : 0u;
        k1 = lane + 64 < nvalid ? pool_key(sS[ul * TK_LDS_TILE + lane + 64], p1, s1, lo, hi) : 0u;
      } else {
        k0 = lane < nvalid ? score_key(sS[ul * TK_LDS_TILE + lane]) : 0u;
        k1 = lane + 64 < nvalid ? score_key(sS[ul * TK_LDS_TILE + lane + 64]) : 0u;
      }
      uint32_t thr = sThr[ul];
      if (__ballot(k0 > thr || k1 > thr) == 0ull) continue;
      // slow path: this user's candidates in registers (slots lane and lane + 64; slots >= k can never be the minimum)
      u64* list = sList + (size_t)ul * a.k;
      u64 c0 = lane < a.k ? list[lane] : ~0ull, c1 = lane + 64 < a.k ? list[lane + 64] : ~0ull;
      u64 mn = wave_min_u64(c0 < c1 ? c0 : c1);
      int32_t ex = 0, ex1 = 0;                                // CSR: the entries of the user's segment inside [vc, vc + 128)
      if constexpr (CSR) {
        const int32_t seg_hi = __builtin_amdgcn_readlane(x_hi, iu);
        const int32_t from = csr_lower_bound(ca.ids, __builtin_amdgcn_readlane(x_lo, iu), seg_hi, (int32_t)vc, lane);
        if (lane < seg_hi - from) ex = ca.ids[from + lane];
        if (lane + 64 < seg_hi - from) ex1 = ca.ids[from + lane + 64];
        if (ex >= vc + TK_ROWS) ex = 0;
        if (ex1 >= vc + TK_ROWS) ex1 = 0;
      } else
        ex = (a.exclude != nullptr && lane < a.E) ? a.exclude[(size_t)(u0 + ul) * a.ld_excl + lane] : 0;
      GroupRegs<GROUP> r;
      if constexpr (GROUP) {
        if (lane < a.k && c0 != 0ull) r.g0 = ga.group[(uint32_t)~(uint32_t)c0];
        if (lane + 64 < a.k && c1 != 0ull) r.g1 = ga.group[(uint32_t)~(uint32_t)c1];
        if (lane < nvalid) r.n0 = ga.group[vc + lane];
        if (lane + 64 < nvalid) r.n1 = ga.group[vc + lane + 64];
      }
      for (int half = 0; half < 2; ++half) {
        const uint32_t kh = half ? k1 : k0;
        u64 pass = __ballot(kh > thr);
        while (pass) {
          const int j = __ffsll((long long)pass) - 1;
          pass &= pass - 1;
          const uint32_t key = __shfl(kh, j, 64);
          if (key <= thr) continue;                          // the threshold rose since the ballot
          const uint32_t id = (uint32_t)(vc + half * 64 + j);
          if constexpr (CSR) {
            if (__ballot(ex == (int32_t)id || ex1 == (int32_t)id) != 0ull) continue;
          } else if (__ballot(ex == (int32_t)id) != 0ull) continue; // ids are >= 1: the 0 of an unused lane never matches
          const u64 cand = ((u64)key << 32) | (uint32_t)~id;
          if constexpr (GROUP) {
            const int32_t gc = __shfl(half ? r.n1 : r.n0, j, 64);
            u64 out = mn;                                    // as below, unless the candidate's group is saturated:
            if (gc >= 0 && __popcll(__ballot(r.g0 == gc)) + __popcll(__ballot(r.g1 == gc)) >= ga.cap) {
              const u64 m0 = r.g0 == gc ? c0 : ~0ull, m1 = r.g1 == gc ? c1 : ~0ull;
              out = wave_min_u64(m0 < m1 ? m0 : m1);         // then only the group's own smallest can make room
              if (cand < out) continue;
            }
            const u64 at0 = __ballot(c0 == out);
            if (at0) {
              if (lane == __ffsll((long long)at0) - 1) c0 = cand, r.g0 = gc;
            } else {
              const u64 at1 = __ballot(c1 == out);
              if (lane == __ffsll((long long)at1) - 1) c1 = cand, r.g1 = gc;
            }
          } else {
            const u64 at0 = __ballot(c0 == mn);              // replace the worst (an empty slot while there is one)
            if (at0) {
              if (lane == __ffsll((long long)at0) - 1) c0 = cand;
            } else {
              const u64 at1 = __ballot(c1 == mn);
              if (lane == __ffsll((long long)at1) - 1) c1 = cand;
            }
          }
          mn = wave_min_u64(c0 < c1 ? c0 : c1);
          thr = (uint32_t)(mn >> 32);
        }
      }
      if (lane < a.k) list[lane] = c0;
      if (lane + 64 < a.k) list[lane + 64] = c1;
      if (lane == 0) sThr[ul] = thr;
    }
    __syncthreads();                                          // the score tile is the next chunk's staging buffer
  }
  __syncthreads();
  for (int i = tid; i < TU * a.k; i += TK_THREADS) {
    const int ul = i / a.k, j = i - ul * a.k;
    if (u0 + ul < a.U) a.part[((size_t)(u0 + ul) * a.splits + blockIdx.y) * a.k + j] = sList[i];
  }
}

// one user's n candidates, padded with 0 to P (a power of two), into tk_keys and sorted descending; ends with a barrier
__device__ __forceinline__ void merge_sort_keys(u64* tk_keys, const u64* __restrict__ part, int n, int P, int tid, size_t u) {
  for (int i = tid; i < P; i += 256) tk_keys[i] = i < n ? part[u * n + i] : 0ull;
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < P / 2; t += 256) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const u64 x = tk_keys[lo], y = tk_keys[hi];
        if ((x < y) == desc && x != y) {
          tk_keys[lo] = y;
          tk_keys[hi] = x;
        }
      }
    }
  __syncthreads();
}

__global__ __launch_bounds__(256) void topk_merge_kernel(const u64* __restrict__ part, int n, int P, int k, int32_t* __restrict__ out_ids,
                                                          float* __restrict__ out_scores) {
  extern __shared__ __attribute__((aligned(16))) u64 tk_keys[];
  const int tid = threadIdx.x;
  const size_t u = blockIdx.x;
  merge_sort_keys(tk_keys, part, n, P, tid, u);
  for (int i = tid; i < k; i += 256) {
    const u64 key = tk_keys[i];
    out_ids[u * k + i] = key ? (int32_t)~(uint32_t)key : 0;
    out_scores[u * k + i] = key ? key_score((uint32_t)(key >> 32)) : -__builtin_inff();
  }
}

// The merge of a capped call: after the sort ONE wave walks the keys 64 at a time in sorted order.  Within a group the
// greedy walk takes exactly the first c keys, so key i is taken when its group is negative or (taken keys of its group in
// earlier blocks) + (keys of its group at earlier lanes of this block) < c: per distinct group of the block three ballots,
// no serial walk.  The groups of the <= 128 taken keys live in LDS behind the keys (sTaken, -1 = ungrouped / not yet
// taken), two per lane in registers while a block is decided.  The walk stops at k taken or at the first key 0 (the sort
// puts them last; key 0 is never taken); usually within a few blocks.
__global__ __launch_bounds__(256) void topk_merge_group_kernel(const u64* __restrict__ part, int n, int P, int k,
                                                                const int32_t* __restrict__ group, int cap, int32_t* __restrict__ out_ids,
                                                                float* __restrict__ out_scores) {
  extern __shared__ __attribute__((aligned(16))) u64 tk_keys[];
  int32_t* sTaken = reinterpret_cast<int32_t*>(tk_keys + P);   // [NR_TOPK_MAX_K]
  const int tid = threadIdx.x;
  const size_t u = blockIdx.x;
  merge_sort_keys(tk_keys, part, n, P, tid, u);
  if (tid >= 64) return;                                        // no barrier follows
  const int lane = tid;
  const u64 below = (1ull << lane) - 1ull;
  sTaken[lane] = -1;
  sTaken[lane + 64] = -1;
  int nt = 0;
  for (int base = 0; base < P && nt < k; base += 64) {
    const u64 key = base + lane < P ? tk_keys[base + lane] : 0ull;
    if (__ballot(key != 0ull) == 0ull) break;
    const int32_t g = key != 0ull ? group[(uint32_t)~(uint32_t)key] : -1;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // sTaken: written by other lanes of this wave in the block before
    const int32_t t0 = sTaken[lane], t1 = sTaken[lane + 64];
    bool take = key != 0ull && g < 0;
    u64 todo = __ballot(g >= 0);
    while (todo) {
      const int32_t gl = __shfl(g, __ffsll((long long)todo) - 1, 64);
      const u64 same = __ballot(g == gl);
      const int before = __popcll(__ballot(t0 == gl)) + __popcll(__ballot(t1 == gl));
      if (g == gl) take = before + __popcll(same & below) < cap;
      todo &= ~same;
    }
    const u64 taken = __ballot(take);
    const int pos = nt + __popcll(taken & below);
    if (take && pos < k) {
      out_ids[u * k + pos] = (int32_t)~(uint32_t)key;
      out_scores[u * k + pos] = key_score((uint32_t)(key >> 32));
      sTaken[pos] = g;
    }
    nt += __popcll(taken);
  }
  for (int i = (nt < k ? nt : k) + lane; i < k; i += 64) {
    out_ids[u * k + i] = 0;
    out_scores[u * k + i] = -__builtin_inff();
  }
}

// argument checks shared by the size query and the call; 0 = fine
int topk_check(const nr_topk_desc* d) {
  NR_CHECK_ARG(d != nullptr, "score_topk: null descriptor");
  NR_CHECK_ARG(d->k >= 1 && d->k <= NR_TOPK_MAX_K, "score_topk: k = %d, must be in [1, %d]", d->k, NR_TOPK_MAX_K);
  NR_CHECK_RC(check_vectors("score_topk", d->V, d->U, d->N));
  NR_CHECK_RC(check_lists("score_topk", d->E, d->excl_offsets, d->excl_ids, d->n_excl));
  NR_CHECK_ARG(d->splits >= 0 && d->splits <= tk_max_splits(d->k), "score_topk: splits = %d, must be 0 (library's choice) or in [1, %d] for k = %d",
               d->splits, tk_max_splits(d->k), d->k);
  NR_CHECK_RC(check_pools("score_topk", d->stamp, d->window, d->ld_window));
  NR_CHECK_ARG(d->group == nullptr || (d->group_cap >= 1 && d->group_cap <= NR_TOPK_MAX_K),
               "score_topk: group given with group_cap = %d, the cap must be in [1, %d]", d->group_cap, NR_TOPK_MAX_K);
  NR_CHECK_ARG(d->group != nullptr || d->group_cap == 0, "score_topk: group_cap = %d given without group (the two come together)", d->group_cap);
  return NR_OK;
}

// K12: the model part of a sampled row, fl32(perturbed - fl32(tau_u * g)), from the ids and perturbed scores the merge wrote; the
// noise is made again from (user key, id) -- the same function, the same bits as in the selection.  -inf in fill.
__global__ __launch_bounds__(256) void sample_model_kernel(const int32_t* __restrict__ ids, const float* __restrict__ perturbed, SampleArgs sa,
                                                            int k, long n, float* __restrict__ out_model) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long u = i / k;
  const int32_t id = ids[i];
  float m = -__builtin_inff();
  if (id > 0) m = __fsub_rn(perturbed[i], sample_scaled(sa.tau_of(u), sa.gumbel(sa.key_of(u), (uint32_t)id)));
  out_model[i] = m;
}

// K12 probe: the noise of n (user key, news id) pairs, element-wise
__global__ __launch_bounds__(256) void sample_noise_kernel(SampleArgs sa, const int32_t* __restrict__ user_keys, const int32_t* __restrict__ news_ids,
                                                            int n, float* __restrict__ out_g, uint32_t* __restrict__ out_bits) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t bits = sample_bits((uint32_t)user_keys[i], (uint32_t)news_ids[i], sa.seed_lo, sa.seed_hi, sa.draw);
  if (out_bits != nullptr) out_bits[i] = bits;
  if (out_g != nullptr) out_g[i] = sample_gumbel(bits);
}

// nr_score_topk's checks plus the fields of the sampled call; 0 = fine
int sample_check(const nr_sample_desc* d) {
  NR_CHECK_ARG(d != nullptr, "score_sample: null descriptor");
  NR_CHECK_RC(topk_check(&d->topk));
  NR_CHECK_ARG(d->tau_u != nullptr || (d->tau >= 0.f && d->tau <= 3.402823466e38f), "score_sample: tau = %g, must be finite and >= 0",
               (double)d->tau);
  return NR_OK;
}

// The selection's instantiation for the run-time (tile, pool, caps, CSR lists, sampled): the 36 that exist, a sampled call
// being a pooled one.
int topk_select_launch(int TU, bool pool, bool grouped, bool csr, bool sampled, dim3 grid, size_t smem, hipStream_t s, const TopkArgs& a,
                              const GroupArgs& ga, const CsrArgs& ca, const SampleArgs& sa) {
  return with_int<64, 32, 16>(TU, [&](auto tu) {
    return with_bool(pool || sampled, [&](auto p) {
      return with_bool(grouped, [&](auto g) {
        return with_bool(csr, [&](auto c) {
          return with_bool(sampled, [&](auto sm) {
            constexpr int MT = decltype(tu)::value / 16;
            constexpr bool POOL = decltype(p)::value, GROUP = decltype(g)::value, CSR = decltype(c)::value, SAMPLE = decltype(sm)::value;
            if constexpr (SAMPLE && !POOL) return (int)NR_ERR_ARG;   // not reached: pool || sampled
            else return launch_lds(topk_select_kernel<MT, POOL, GROUP, CSR, SAMPLE>, grid, dim3(TK_THREADS), smem, s, a, ga, ca, sa);
          });
        });
      });
    });
  });
}

}  // namespace

extern "C" {

size_t nr_score_topk_workspace_bytes(const nr_topk_desc* d) {
  if (topk_check(d) != NR_OK) return 0;
  return (size_t)d->U * tk_plan(d).splits * d->k * sizeof(u64);
}

// the two launches of nr_score_topk (sa == nullptr) and of nr_score_sample
static int topk_run(const nr_topk_desc* d, const SampleArgs* sa_in, nr_stream_t stream) {
  NR_CHECK_RC(topk_check(d));
  NR_CHECK_ARG(d->news_vecs && d->user && d->out_ids && d->out_scores, "score_topk: null pointer (news_vecs, user, out_ids, out_scores)");
  NR_CHECK_RC(check_rows("score_topk", d->news_vecs, d->ld_news, d->user, d->ld_user, d->N));
  NR_CHECK_ARG(d->E == 0 || d->exclude == nullptr || d->ld_exclude >= d->E, "score_topk: exclusion row stride %d < E = %d", d->ld_exclude, d->E);
  NR_CHECK_RC(check_workspace("score_topk", d->ws, d->ws_bytes, nr_score_topk_workspace_bytes(d)));
  NR_DEVICE_GUARD(stream, d->news_vecs);
  hipStream_t s = (hipStream_t)stream;
  const TopkPlan pl = tk_plan(d);
  const int splits = pl.splits, TU = pl.TU;
  TopkArgs a;
  a.news = d->news_vecs; a.user = d->user;
  a.exclude = d->E > 0 ? d->exclude : nullptr;
  a.part = reinterpret_cast<u64*>(d->ws);
  a.ld_news = (size_t)d->ld_news; a.ld_user = (size_t)d->ld_user; a.ld_excl = (size_t)d->ld_exclude;
  a.V = d->V; a.U = d->U; a.N = d->N; a.k = d->k; a.E = d->E; a.splits = splits;
  a.per = (int)(((long)d->V - 1 + splits - 1) / splits);
  a.pool = pool_args(d->prior, d->stamp, d->window, d->ld_window);
  const GroupArgs ga = {d->group, d->group_cap};
  const bool sampled = sa_in != nullptr;
  const SampleArgs sa = sampled ? *sa_in : SampleArgs{0u, 0u, 0u, 0.f, nullptr, nullptr};
  const bool grouped = d->group != nullptr;
  const CsrArgs ca = csr_args(d->excl_offsets, d->excl_ids, d->n_excl);
  const size_t smem = tk_lds_bytes(TU, d->N, d->k);
  const dim3 grid((unsigned)((d->U + TU - 1) / TU), (unsigned)splits);
  {
    NrProfScope ps(s, "topk_select[U=%d,V=%d,N=%d,k=%d,TU=%d,splits=%d]", d->U, d->V, d->N, d->k, TU, splits);
    NR_CHECK_RC(topk_select_launch(TU, a.pool.any(), grouped, ca.offsets != nullptr, sampled, grid, smem, s, a, ga, ca, sa));
  }
  NR_CHECK_LAUNCH();
  const int n = splits * d->k;
  int P = 2;
  while (P < n) P <<= 1;
  {
    NrProfScope ps(s, "topk_merge[U=%d,n=%d,k=%d]", d->U, n, d->k);
    if (grouped) {
      const size_t msmem = (size_t)P * sizeof(u64) + NR_TOPK_MAX_K * sizeof(int32_t);   // up to 64.5 KiB: above the default limit
      NR_CHECK_RC(launch_lds(topk_merge_group_kernel, dim3((unsigned)d->U), dim3(256), msmem, s, a.part, n, P, d->k, d->group, d->group_cap, d->out_ids,
                             d->out_scores));
    } else
      hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)d->U), dim3(256), (size_t)P * sizeof(u64), s, (const u64*)a.part, n, P, d->k, d->out_ids,
                         d->out_scores);
  }
  NR_CHECK_LAUNCH();
  return NR_OK;
}

int nr_score_topk(const nr_topk_desc* d, nr_stream_t stream) { return topk_run(d, nullptr, stream); }

size_t nr_score_sample_workspace_bytes(const nr_sample_desc* d) {
  if (sample_check(d) != NR_OK) return 0;
  return nr_score_topk_workspace_bytes(&d->topk);
}

int nr_score_sample(const nr_sample_desc* d, nr_stream_t stream) {
  NR_CHECK_RC(sample_check(d));
  const SampleArgs sa = {(uint32_t)(d->seed & 0xffffffffull), (uint32_t)(d->seed >> 32), d->draw, d->tau, d->tau_u, d->user_keys};
  const int rr = topk_run(&d->topk, &sa, stream);
  if (rr != NR_OK || d->out_model == nullptr) return rr;
  NR_DEVICE_GUARD(stream, d->topk.news_vecs);
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)d->topk.U * d->topk.k;
  {
    NrProfScope ps(s, "sample_model[U=%d,k=%d]", d->topk.U, d->topk.k);
    hipLaunchKernelGGL(sample_model_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const int32_t*)d->topk.out_ids,
                       (const float*)d->topk.out_scores, sa, d->topk.k, n, d->out_model);
  }
  NR_CHECK_LAUNCH();
  return NR_OK;
}

int nr_sample_noise(uint64_t seed, uint32_t draw, const int32_t* user_keys, const int32_t* news_ids, int n, float* out_g, uint32_t* out_bits,
                    nr_stream_t stream) {
  NR_CHECK_ARG(n >= 0, "sample_noise: n = %d pairs, must be >= 0", n);
  if (n == 0) return NR_OK;
  NR_CHECK_ARG(user_keys != nullptr && news_ids != nullptr, "sample_noise: null pointer (user_keys, news_ids)");
  NR_DEVICE_GUARD(stream, news_ids);
  hipStream_t s = (hipStream_t)stream;
  const SampleArgs sa = {(uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), draw, 0.f, nullptr, nullptr};
  {
    NrProfScope ps(s, "sample_noise[n=%d]", n);
    hipLaunchKernelGGL(sample_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sa, user_keys, news_ids, n, out_g, out_bits);
  }
  NR_CHECK_LAUNCH();
  return NR_OK;
}

}  // extern "C"
