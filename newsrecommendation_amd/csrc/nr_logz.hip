// Propensities of full-corpus rows: the log-partition of a user's whole score row, and on it the log-probabilities of the
// entries of named rows -- again without the [U, V] score matrix.  The third consumer of the tile of nr_score_tile.h (after the
// selection of nr_topk.hip and the counting of nr_rank.hip): summing in place of counting.  Scores and eligibility come from
// score_key / pool_key, so one (u, v) pair has here the bits and the verdict it has in nr_score_topk and nr_score_rank.
//
//   logz_stream_kernel<MT, POOL, LISTS>   the grid, chunking, user tile and LDS budget of rank_count_kernel.  [1, V) is cut into
//                           nseg <= 256 SEGMENTS of seg = 128 * ceil((V - 1) / (128 * 256)) ids, a function of V alone; a slice
//                           (blockIdx.y) is a run of whole segments.  A wave owns TU / 8 users; after put_scores lane l holds
//                           news vc + l and vc + l + 64 of the chunk at vc.  Chunk starts are segment start + 128 q, so which
//                           lane sees which id is fixed by V.  Per user and lane: a running (max, sum of exp((x - max) / tau),
//                           count) over the lane's eligible news of the segment, rescaled when the lane's maximum rises -- one
//                           expf per news.  At the segment end: wave maximum (exact), each lane rescales its sum once, xor
//                           butterfly sum, and lane 0 stores ONE (max, sum, count) partial per (user, segment).  Nothing in a
//                           partial depends on the slices, the user tile, the place in it or the other users.
//                           LISTS: exclusion lists in CSR form (include/nrhip.h, K13).  Exclusion happens HERE, in the stream:
//                           the listed news (the clicked history, the row already taken) are typically the heaviest terms of the
//                           sum, and subtracting their weights afterwards would cancel.  Every user of the wave keeps a cursor
//                           into its strictly ascending segment, set by a 64-ary search to the first entry >= the slice start;
//                           per chunk the at most 128 entries inside it become two 64-bit "listed" masks in scalar registers.
//   logz_final_kernel       one wave per user, four partials a lane: maximum of the partials (exact), then their sums rescaled to
//                           it and added in fp64 in a fixed order (the lane's segments ascending, then an xor butterfly), one
//                           log, rounded to fp32 once.
//   logp_rows_kernel<POOL>  the named-row gather of rank_named_kernel (ScoreNamedRows, nr_score_tile.h): one workgroup per 16 users, chunk c = the k <= 128 rows user
//                           c names, so the entries get the stream's score bits.  Then one wave per user finishes in fp64: a
//                           suffix scan of (max, sum) pairs over the row joined with the user's base partition (sequential =
//                           Plackett-Luce without replacement; only positive terms are added), or each entry against the base
//                           alone (independent).
//   logp_grad_kernel<POOL>  the sibling of logp_rows_kernel for the gradient of the sequential row (K19): the same gather and suffix
//                           scan, then a prefix scan of (-M_j, g_j / sigma_j) pairs, which gives the coefficients (a, c) that turn
//                           K17 and K18 into the row's gradient.  O(k log k) fp64 exp per user, every exponent <= 0.
#include <math.h>

#include "nr_logz_stream.h"

namespace {

// The tile is what the vectors and the staging buffers leave room for, as in the counting pass of nr_rank.hip (the segments and
// slices: lz_plan_tile, nr_logz_stream.h)
inline LogzPlan lz_plan(int U, int V, int N, int splits) { return lz_plan_tile(U, V, score_user_tile(N, 0), splits); }

struct LogzArgs {
  const float* news;
  const float* user;
  size_t ld_news, ld_user;
  int V, U, N, seg, nseg, segs_per;
  PoolArgs pool;            // read by the POOL instantiations only
  float tau;                // used when tau_u is null
  const float* tau_u;       // [U] or null
  float* pm;                // [U, nseg] partial maxima, -inf = nothing eligible in the segment
  float* ps;                // [U, nseg] partial sums of exp((x - pm) / tau)
  int32_t* pc;              // [U, nseg] eligible news of the segment
  __device__ __forceinline__ float tau_of(long u) const { return tau_u != nullptr ? tau_u[u] : tau; }
};
// workspace: the three [U, nseg] arrays, 12 bytes per (user, segment), rounded to 8
inline size_t lz_carve(void* ws, int U, int nseg, LogzArgs* a) {
  char* p = reinterpret_cast<char*>(ws);
  const size_t n = (size_t)U * nseg;
  if (a) {
    a->pm = reinterpret_cast<float*>(p);
    a->ps = reinterpret_cast<float*>(p + n * 4);
    a->pc = reinterpret_cast<int32_t*>(p + n * 8);
  }
  return (n * 12 + 7) & ~(size_t)7;
}

// One eligible news x into a lane's running (m, s): s = sum of exp((x_i - m) * it) over what the lane has seen, m their maximum.
// e = exp(-|x - m| * it) serves both cases: a new maximum rescales the sum by it and adds 1, anything else adds it.  x == m adds
// exactly 1 without forming inf - inf; -inf under a finite maximum adds exp(-inf) = 0.
__device__ __forceinline__ void lz_take(float x, float it, float& m, float& s) {
  const bool up = x > m;
  const float d = up ? m - x : x - m;
  const float e = x == m ? 1.f : expf(d * it);
  s = up ? fmaf(s, e, 1.f) : s + e;
  m = up ? x : m;
}

template <int MT, bool POOL, bool LISTS>
__global__ __launch_bounds__(TK_THREADS) void logz_stream_kernel(LogzArgs a, CsrArgs ca) {
  constexpr int TU = 16 * MT, PER_WAVE = TU / TK_WAVES;
  extern __shared__ __attribute__((aligned(16))) float lz_smem[];
  ScoreTile<MT> t(lz_smem, a.N);
  const int lane = t.lane, wave = t.wave;
  const int u0 = blockIdx.x * TU;
  const int s_lo = (int)blockIdx.y * a.segs_per;
  const int s_hi = s_lo + a.segs_per < a.nseg ? s_lo + a.segs_per : a.nseg;
  const long v_lo = 1 + (long)s_lo * a.seg;
  const long v_hi = 1 + (long)s_hi * a.seg < a.V ? 1 + (long)s_hi * a.seg : a.V;
  if (v_lo >= v_hi) return;                                   // the whole workgroup

  t.load_users(a.user, a.ld_user, u0, a.U);
  // user wave + 8 i of the tile: 1 / tau and this lane's running (max, sum, count) of the segment
  float it[PER_WAVE], m[PER_WAVE], s[PER_WAVE];
  int32_t cnt[PER_WAVE];
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int u = u0 + wave + TK_WAVES * i;
    it[i] = __fdiv_rn(1.f, u < a.U ? a.tau_of(u) : 1.f);
    m[i] = -LZ_INF;
    s[i] = 0.f;
    cnt[i] = 0;
  }
  // LISTS: the cursor of every user of the wave = the first entry of its segment that is >= v_lo (LZ_SEEK, nr_logz_stream.h)
  int32_t cur[PER_WAVE], end[PER_WAVE];
  if constexpr (LISTS) LZ_SEEK(ca, u0, wave, lane, a.U, v_lo, cur, end)
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
  t.load_slab(rows, 0);
  for (long vc = v_lo; vc < v_hi; vc += TK_ROWS) {
    f32x4 acc[MT];
    rows.vc = vc;
    t.chunk(rows, acc);
    rows.vc = vc + TK_ROWS;
    if (rows.vc < v_hi) t.load_slab(rows, 0);                 // in flight while this chunk is summed
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
    // LISTS: the next 64 entries of every user's segment from its cursor on (in flight over the barrier)
    int32_t e0[LISTS ? PER_WAVE : 1];
    if constexpr (LISTS) {
#pragma unroll
      for (int i = 0; i < PER_WAVE; ++i) e0[i] = (long)cur[i] + lane < end[i] ? ca.ids[(long)cur[i] + lane] : 0x7fffffff;
    }
    t.put_scores(acc);
    const float* sS = t.scores();
    const int nvalid = (int)(v_hi - vc < TK_ROWS ? v_hi - vc : TK_ROWS);
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      const int ul = wave + TK_WAVES * i;
      // LISTS: the entries inside [vc, vc + 128) are a prefix of what the cursor points at; bit r of (l0, l1) = news vc + r is listed
      u64 l0 = 0ull, l1 = 0ull;
      if constexpr (LISTS) LZ_LISTED(ca, e0[i], cur[i], end[i], vc, lane, l0, l1)
      uint32_t k0, k1;
      if constexpr (POOL) {
        const int32_t lo = __builtin_amdgcn_readlane(w_lo, i), hi = __builtin_amdgcn_readlane(w_hi, i);
        k0 = pool_key(sS[ul * TK_LDS_TILE + lane], p0, s0, lo, hi);
        k1 = pool_key(sS[ul * TK_LDS_TILE + lane + 64], p1, s1, lo, hi);
      } else {
        k0 = score_key(sS[ul * TK_LDS_TILE + lane]);
        k1 = score_key(sS[ul * TK_LDS_TILE + lane + 64]);
      }
      // eligible: a row of the slice, key != 0 (not NaN, inside the pool), not listed; the score is key_score of the key
      const bool el0 = lane < nvalid && k0 != 0u && ((l0 >> lane) & 1ull) == 0ull;
      const bool el1 = lane + 64 < nvalid && k1 != 0u && ((l1 >> lane) & 1ull) == 0ull;
      if (el0) {
        lz_take(key_score(k0), it[i], m[i], s[i]);
        ++cnt[i];
      }
      if (el1) {
        lz_take(key_score(k1), it[i], m[i], s[i]);
        ++cnt[i];
      }
    }
    // segment end: one partial per (user, segment), in an order that V alone fixes
    const long nxt = vc + TK_ROWS;
    if (nxt >= v_hi || (nxt - 1) % a.seg == 0) {
      const size_t sg = (size_t)((vc - 1) / a.seg);
#pragma unroll
      for (int i = 0; i < PER_WAVE; ++i) {
        const int u = u0 + wave + TK_WAVES * i;
        const float M = wave_max(m[i]);
        const float sc = m[i] == M ? 1.f : expf((m[i] - M) * it[i]);
        const float S = wave_sum(s[i] * sc);
        const int C = wave_sum_i(cnt[i]);
        if (lane == 0 && u < a.U) {
          a.pm[(size_t)u * a.nseg + sg] = M;
          a.ps[(size_t)u * a.nseg + sg] = S;
          a.pc[(size_t)u * a.nseg + sg] = C;
        }
        m[i] = -LZ_INF;
        s[i] = 0.f;
        cnt[i] = 0;
      }
    }
    __syncthreads();                                          // the score tile is the next chunk's staging buffer
  }
}

// One wave per user; lane l holds the partials of segments l, l + 64, l + 128, l + 192 (nseg <= 256).
__global__ __launch_bounds__(256) void logz_final_kernel(LogzArgs a, float* __restrict__ out_logsum, float* __restrict__ out_max,
                                                         int32_t* __restrict__ out_count) {
  static_assert(LZ_MAX_SEGS == 4 * 64, "four partials per lane");
  const int lane = threadIdx.x & 63;
  const size_t u = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= (size_t)a.U) return;                               // the whole wave
  float mj[4], sj[4], M = -LZ_INF;
  int32_t n = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = lane + 64 * q;
    mj[q] = -LZ_INF;
    sj[q] = 0.f;
    if (j < a.nseg) {
      mj[q] = a.pm[u * a.nseg + j];
      sj[q] = a.ps[u * a.nseg + j];
      n += a.pc[u * a.nseg + j];
    }
    M = fmaxf(M, mj[q]);
  }
  M = wave_max(M);
  n = wave_sum_i(n);
  const float tau = a.tau_of(u);
  const bool tau_ok = tau > 0.f && tau < LZ_INF;
  float ls;
  if (n == 0) ls = -LZ_INF;
  else if (!tau_ok || !(fabsf(M) < LZ_INF)) ls = __builtin_nanf("");
  else {
    // fp64, in a fixed order: the lane's four segments ascending, then the xor butterfly over the lanes
    const double it = (double)__fdiv_rn(1.f, tau);
    double S = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (mj[q] != -LZ_INF) S += (double)sj[q] * (mj[q] == M ? 1.0 : exp(((double)mj[q] - (double)M) * it));
    ls = (float)log(wave_sum_d(S));
  }
  if (lane == 0) {
    out_logsum[u] = ls;
    out_max[u] = M;
    out_count[u] = n;
  }
}

// ---- K14 ----------------------------------------------------------------------------------------------------------------

struct LogpArgs {
  const float* news;
  const float* user;
  const int32_t* ids;
  size_t ld_news, ld_user, ld_ids;
  int V, U, N, k, sequential;
  PoolArgs pool;
  float tau;
  const float* tau_u;
  const float* base_max;
  const float* base_logsum;
  float* out_logp;
  float* out_total;         // [U] or null
};

// (m, s): s = sum of exp((x_i - m) / tau) over a set with maximum m; (-inf, 0) is the empty set
struct LogpPair {
  double m, s;
};
__device__ __forceinline__ LogpPair lp_join(LogpPair x, LogpPair y, double tau) {
  const double M = fmax(x.m, y.m);
  const double ex = x.m == M ? 1.0 : exp((x.m - M) / tau), ey = y.m == M ? 1.0 : exp((y.m - M) / tau);
  return {M, x.s * ex + y.s * ey};
}
__device__ __forceinline__ LogpPair lp_down(LogpPair x, int o) { return {__shfl_down(x.m, o, 64), __shfl_down(x.s, o, 64)}; }

template <bool POOL>
__global__ __launch_bounds__(TK_THREADS) void logp_rows_kernel(LogpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lp_smem[];
  ScoreTile<1> t(lp_smem, a.N);
  int32_t* sIds = reinterpret_cast<int32_t*>(t.end());        // [16, 128] the ids the users name
  uint32_t* sKey = reinterpret_cast<uint32_t*>(sIds + 16 * TK_ROWS);   // [16, 128] their keys, 0 = no score
  const int tid = t.tid, lane = t.lane, wave = t.wave;
  const int u0 = blockIdx.x * 16;
  const int users = a.U - u0 < 16 ? a.U - u0 : 16;

  t.load_users(a.user, a.ld_user, u0, a.U);
  for (int i = tid; i < 16 * TK_ROWS; i += TK_THREADS) {
    const int ul = i / TK_ROWS, j = i - ul * TK_ROWS;
    sIds[i] = ul < users && j < a.k ? a.ids[(size_t)(u0 + ul) * a.ld_ids + j] : 0;
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
      // of the [16 x 128] scores only row c is kept, as its keys: prior and stamp gathered by id give the key of the stream
      const size_t u = (size_t)(u0 + c);
      int32_t lo = 0, hi = 0;
      if constexpr (POOL) {
        lo = a.pool.lo_of(u);
        hi = a.pool.hi_of(u);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int r = lane + 64 * h;
        const int32_t id = sIds[c * TK_ROWS + r];
        uint32_t key = 0u;
        if (id >= 1 && id < a.V) {
          const float dot = t.scores()[c * TK_LDS_TILE + r];
          if constexpr (POOL) key = pool_key(dot, a.pool.prior_of(id), a.pool.stamp_of(id), lo, hi);
          else key = score_key(dot);
        }
        sKey[c * TK_ROWS + r] = key;
      }
    }
    __syncthreads();                                          // the score tile is the next chunk's staging buffer
  }

  // one wave per user, in fp64; lane l holds entries 2 l and 2 l + 1 of the row
  const double NaN = __builtin_nan(""), NINF = -(double)LZ_INF;
  for (int c = wave; c < users; c += TK_WAVES) {
    const size_t u = (size_t)(u0 + c);
    const float tau_f = a.tau_u != nullptr ? a.tau_u[u] : a.tau;
    const bool tau_ok = tau_f > 0.f && tau_f < LZ_INF;
    const double tau = (double)tau_f;
    const int j0 = 2 * lane, j1 = j0 + 1;
    const int32_t id0 = sIds[c * TK_ROWS + j0], id1 = sIds[c * TK_ROWS + j1];
    const uint32_t key0 = sKey[c * TK_ROWS + j0], key1 = sKey[c * TK_ROWS + j1];
    const bool real0 = id0 >= 1 && id0 < a.V, real1 = id1 >= 1 && id1 < a.V;   // else fill: logp 0, in no sum
    const bool live0 = key0 != 0u, live1 = key1 != 0u;                         // key 0: NaN, in no sum
    const double x0 = (double)key_score(key0), x1 = (double)key_score(key1);
    const double bm = (double)a.base_max[u], bl = (double)a.base_logsum[u];
    double lp0, lp1;
    if (a.sequential) {
      const LogpPair none = {NINF, 0.0};
      const LogpPair P0 = live0 ? LogpPair{x0, 1.0} : none, P1 = live1 ? LogpPair{x1, 1.0} : none;
      // inclusive suffix scan over the lanes: R = entries 2 l .. 127
      LogpPair R = lp_join(P0, P1, tau);
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const LogpPair other = lp_down(R, o);
        if (lane + o < 64) R = lp_join(R, other, tau);
      }
      LogpPair after = lp_down(R, 1);                         // entries 2 l + 2 .. 127
      if (lane == 63) after = none;
      const LogpPair base = {bm, exp(bl)};                    // everything eligible that the row does not name
      const LogpPair S1 = lp_join(P1, lp_join(after, base, tau), tau);
      const LogpPair S0 = lp_join(P0, S1, tau);
      lp0 = (x0 - S0.m) / tau - log(S0.s);
      lp1 = (x1 - S1.m) / tau - log(S1.s);
    } else {
      lp0 = (x0 - bm) / tau - bl;
      lp1 = (x1 - bm) / tau - bl;
    }
    lp0 = !real0 ? 0.0 : (!live0 || !tau_ok) ? NaN : lp0;
    lp1 = !real1 ? 0.0 : (!live1 || !tau_ok) ? NaN : lp1;
    if (j0 < a.k) a.out_logp[u * a.k + j0] = (float)lp0;
    if (j1 < a.k) a.out_logp[u * a.k + j1] = (float)lp1;
    if (a.out_total != nullptr) {
      const double tot = wave_sum_d(lp0 + lp1);              // entries beyond k are fill: 0
      if (lane == 0) a.out_total[u] = (float)tot;
    }
  }
}

// ---- K19 ----------------------------------------------------------------------------------------------------------------

struct LogpGradArgs {
  const float* news;
  const float* user;
  const int32_t* ids;
  size_t ld_news, ld_user, ld_ids, ld_g;
  int V, U, N, k;
  PoolArgs pool;
  float tau;
  const float* tau_u;
  const float* base_max;
  const float* base_logsum;
  const float* g;           // [U, ld_g] or null = 1
  float* out_weight;        // [U]
  float* out_sub_w;         // [U, k]
};

__device__ __forceinline__ LogpPair lp_up(LogpPair x, int o) { return {__shfl_up(x.m, o, 64), __shfl_up(x.s, o, 64)}; }

// The gradient coefficients of the sequential row (include/nrhip.h, K19): the gather and the suffix scan of logp_rows_kernel,
// statement for statement, so an entry has K14's key and step j K14's S_j = (M_j, sigma_j), W_j = exp(M_j / tau) sigma_j.  Then
// g_j / W_j as the pair (-M_j, g_j / sigma_j) -- the same (max, sum) algebra, the sum signed: M_j does not increase with j, so
// an inclusive PREFIX scan of these pairs ends, at a live entry i, on the maximum -M_i, and
//   c_i = g_i - exp((x_i - M_i) / tau) q_i,   a = exp((base_max - M_L) / tau + base_logsum) q_L   (L = the last live entry)
// form no exponent above 0.
template <bool POOL>
__global__ __launch_bounds__(TK_THREADS) void logp_grad_kernel(LogpGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lg_smem[];
  ScoreTile<1> t(lg_smem, a.N);
  int32_t* sIds = reinterpret_cast<int32_t*>(t.end());        // [16, 128] the ids the users name
  uint32_t* sKey = reinterpret_cast<uint32_t*>(sIds + 16 * TK_ROWS);   // [16, 128] their keys, 0 = no score
  const int tid = t.tid, lane = t.lane, wave = t.wave;
  const int u0 = blockIdx.x * 16;
  const int users = a.U - u0 < 16 ? a.U - u0 : 16;

  t.load_users(a.user, a.ld_user, u0, a.U);
  for (int i = tid; i < 16 * TK_ROWS; i += TK_THREADS) {
    const int ul = i / TK_ROWS, j = i - ul * TK_ROWS;
    sIds[i] = ul < users && j < a.k ? a.ids[(size_t)(u0 + ul) * a.ld_ids + j] : 0;
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
      int32_t lo = 0, hi = 0;
      if constexpr (POOL) {
        lo = a.pool.lo_of(u);
        hi = a.pool.hi_of(u);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int r = lane + 64 * h;
        const int32_t id = sIds[c * TK_ROWS + r];
        uint32_t key = 0u;
        if (id >= 1 && id < a.V) {
          const float dot = t.scores()[c * TK_LDS_TILE + r];
          if constexpr (POOL) key = pool_key(dot, a.pool.prior_of(id), a.pool.stamp_of(id), lo, hi);
          else key = score_key(dot);
        }
        sKey[c * TK_ROWS + r] = key;
      }
    }
    __syncthreads();                                          // the score tile is the next chunk's staging buffer
  }

  // one wave per user, in fp64; lane l holds entries 2 l and 2 l + 1 of the row
  const double NINF = -(double)LZ_INF;
  const LogpPair none = {NINF, 0.0};
  for (int c = wave; c < users; c += TK_WAVES) {
    const size_t u = (size_t)(u0 + c);
    const float tau_f = a.tau_u != nullptr ? a.tau_u[u] : a.tau;
    const float bm_f = a.base_max[u], bl_f = a.base_logsum[u];
    const bool dead = !(tau_f > 0.f && tau_f < LZ_INF) || bm_f != bm_f || bl_f != bl_f;   // a = 0, every c = 0
    const double tau = (double)tau_f, bm = (double)bm_f, bl = (double)bl_f;
    const int j0 = 2 * lane, j1 = j0 + 1;
    const uint32_t key0 = sKey[c * TK_ROWS + j0], key1 = sKey[c * TK_ROWS + j1];
    const bool live0 = key0 != 0u, live1 = key1 != 0u;        // a step of the row: a real id (j < k) with a score inside the pool
    const double x0 = (double)key_score(key0), x1 = (double)key_score(key1);
    double g0 = live0 ? 1.0 : 0.0, g1 = live1 ? 1.0 : 0.0;    // the g of anything else is not read
    if (a.g != nullptr) {
      if (live0) g0 = (double)a.g[u * a.ld_g + j0];
      if (live1) g1 = (double)a.g[u * a.ld_g + j1];
    }
    // K14's suffix scan: S_j = the base and the live entries j .. 127
    const LogpPair P0 = live0 ? LogpPair{x0, 1.0} : none, P1 = live1 ? LogpPair{x1, 1.0} : none;
    LogpPair R = lp_join(P0, P1, tau);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const LogpPair other = lp_down(R, o);
      if (lane + o < 64) R = lp_join(R, other, tau);
    }
    LogpPair after = lp_down(R, 1);                           // entries 2 l + 2 .. 127
    if (lane == 63) after = none;
    const LogpPair base = {bm, exp(bl)};                      // everything eligible that the row does not name
    const LogpPair S1 = lp_join(P1, lp_join(after, base, tau), tau);
    const LogpPair S0 = lp_join(P0, S1, tau);
    // inclusive prefix scan of (-M_j, g_j / sigma_j) over the live steps: Q_i = sum_{j <= i} g_j / W_j (sigma_j >= 1 at a live step)
    const LogpPair T0 = live0 ? LogpPair{-S0.m, g0 / S0.s} : none, T1 = live1 ? LogpPair{-S1.m, g1 / S1.s} : none;
    LogpPair Q = lp_join(T0, T1, tau);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const LogpPair other = lp_up(Q, o);
      if (lane >= o) Q = lp_join(other, Q, tau);
    }
    LogpPair before = lp_up(Q, 1);                            // entries 0 .. 2 l - 1
    if (lane == 0) before = none;
    const LogpPair Q0 = lp_join(before, T0, tau), Q1 = lp_join(Q0, T1, tau);
    const LogpPair all = {__shfl(Q.m, 63, 64), __shfl(Q.s, 63, 64)};
    // at a live entry Q_i.m = -M_i, so the exponent is (x_i - M_i) / tau <= 0
    const double c0 = live0 && !dead ? g0 - exp((x0 + Q0.m) / tau) * Q0.s : 0.0;
    const double c1 = live1 && !dead ? g1 - exp((x1 + Q1.m) / tau) * Q1.s : 0.0;
    if (j0 < a.k) a.out_sub_w[u * a.k + j0] = (float)c0;
    if (j1 < a.k) a.out_sub_w[u * a.k + j1] = (float)c1;
    if (lane == 0) {
      // an empty base (max -inf) and a row without a live step have a = 0 exactly; base_max <= M_L, so the exponent's first term is <= 0
      const bool zero = dead || bm == NINF || all.m == NINF;
      a.out_weight[u] = zero ? 0.f : (float)(exp((bm + all.m) / tau + bl) * all.s);
    }
  }
}

// argument checks shared by the size query and the call; 0 = fine
int logz_check(const nr_logz_desc* d) {
  NR_CHECK_ARG(d != nullptr, "score_logz: null descriptor");
  NR_CHECK_RC(check_vectors("score_logz", d->V, d->U, d->N));
  NR_CHECK_RC(check_lists("score_logz", 0, d->excl_offsets, d->excl_ids, d->n_excl));   // this call has no dense list
  NR_CHECK_ARG(d->tau_u != nullptr || (d->tau > 0.f && d->tau < LZ_INF), "score_logz: tau = %g, a scalar temperature must be finite and > 0",
               (double)d->tau);
  const int nseg = lz_plan(d->U, d->V, d->N, 1).nseg;
  NR_CHECK_ARG(d->splits >= 0 && d->splits <= nseg, "score_logz: splits = %d, must be 0 (library's choice) or in [1, %d], the segments of V = %d",
               d->splits, nseg, d->V);
  return check_pools("score_logz", d->stamp, d->window, d->ld_window);
}

// the stream's instantiation for the run-time (tile, pool, lists)
int logz_stream_launch(int TU, bool pool, bool lists, dim3 grid, size_t smem, hipStream_t s, const LogzArgs& a, const CsrArgs& ca) {
  return with_int<64, 32, 16>(TU, [&](auto tu) {
    return with_bool(pool, [&](auto p) {
      return with_bool(lists, [&](auto l) {
        return launch_lds(logz_stream_kernel<decltype(tu)::value / 16, decltype(p)::value, decltype(l)::value>, grid, dim3(TK_THREADS), smem, s, a, ca);
      });
    });
  });
}

}  // namespace

extern "C" {

size_t nr_score_logz_workspace_bytes(const nr_logz_desc* d) {
  if (logz_check(d) != NR_OK) return 0;
  return lz_carve(nullptr, d->U, lz_plan(d->U, d->V, d->N, d->splits).nseg, nullptr);
}

int nr_score_logz(const nr_logz_desc* d, nr_stream_t stream) {
  NR_CHECK_RC(logz_check(d));
  NR_CHECK_ARG(d->news_vecs && d->user && d->out_logsum && d->out_max && d->out_count,
               "score_logz: null pointer (news_vecs, user, out_logsum, out_max, out_count)");
  NR_CHECK_RC(check_rows("score_logz", d->news_vecs, d->ld_news, d->user, d->ld_user, d->N));
  NR_CHECK_RC(check_workspace("score_logz", d->ws, d->ws_bytes, nr_score_logz_workspace_bytes(d)));
  NR_DEVICE_GUARD(stream, d->news_vecs);
  hipStream_t s = (hipStream_t)stream;
  const LogzPlan pl = lz_plan(d->U, d->V, d->N, d->splits);
  LogzArgs a;
  a.news = d->news_vecs; a.user = d->user;
  a.ld_news = (size_t)d->ld_news; a.ld_user = (size_t)d->ld_user;
  a.V = d->V; a.U = d->U; a.N = d->N; a.seg = pl.seg; a.nseg = pl.nseg; a.segs_per = pl.segs_per;
  a.pool = pool_args(d->prior, d->stamp, d->window, d->ld_window);
  a.tau = d->tau; a.tau_u = d->tau_u;
  lz_carve(d->ws, d->U, pl.nseg, &a);
  const CsrArgs ca = csr_args(d->excl_offsets, d->excl_ids, d->n_excl);
  {
    const int TU = pl.TU;
    const size_t smem = tk_tile_bytes(TU, d->N);
    const dim3 grid((unsigned)((d->U + TU - 1) / TU), (unsigned)pl.splits);
    NrProfScope ps(s, "logz_stream[U=%d,V=%d,N=%d,TU=%d,splits=%d,seg=%d]", d->U, d->V, d->N, TU, pl.splits, pl.seg);
    NR_CHECK_RC(logz_stream_launch(TU, a.pool.any(), ca.offsets != nullptr, grid, smem, s, a, ca));
  }
  NR_CHECK_LAUNCH();
  {
    NrProfScope ps(s, "logz_final[U=%d,nseg=%d]", d->U, pl.nseg);
    hipLaunchKernelGGL(logz_final_kernel, dim3((unsigned)((d->U + 3) / 4)), dim3(256), 0, s, a, d->out_logsum, d->out_max, d->out_count);
  }
  NR_CHECK_LAUNCH();
  return NR_OK;
}

int nr_row_logprob(const nr_logprob_desc* d, nr_stream_t stream) {
  NR_CHECK_ARG(d != nullptr, "row_logprob: null descriptor");
  NR_CHECK_ARG(d->k >= 1 && d->k <= NR_TOPK_MAX_K, "row_logprob: k = %d entries per row, must be in [1, %d]", d->k, NR_TOPK_MAX_K);
  NR_CHECK_RC(check_vectors("row_logprob", d->V, d->U, d->N));
  NR_CHECK_ARG(d->tau_u != nullptr || (d->tau > 0.f && d->tau < LZ_INF), "row_logprob: tau = %g, a scalar temperature must be finite and > 0",
               (double)d->tau);
  NR_CHECK_ARG(d->sequential == 0 || d->sequential == 1, "row_logprob: sequential = %d, must be 0 or 1", d->sequential);
  NR_CHECK_RC(check_pools("row_logprob", d->stamp, d->window, d->ld_window));
  NR_CHECK_ARG(d->news_vecs && d->user && d->row_ids && d->base_max && d->base_logsum && d->out_logp,
               "row_logprob: null pointer (news_vecs, user, row_ids, base_max, base_logsum, out_logp)");
  NR_CHECK_RC(check_rows("row_logprob", d->news_vecs, d->ld_news, d->user, d->ld_user, d->N));
  NR_CHECK_ARG(d->ld_ids >= d->k, "row_logprob: id row stride %d < k = %d", d->ld_ids, d->k);
  NR_DEVICE_GUARD(stream, d->news_vecs);
  hipStream_t s = (hipStream_t)stream;
  LogpArgs a;
  a.news = d->news_vecs; a.user = d->user; a.ids = d->row_ids;
  a.ld_news = (size_t)d->ld_news; a.ld_user = (size_t)d->ld_user; a.ld_ids = (size_t)d->ld_ids;
  a.V = d->V; a.U = d->U; a.N = d->N; a.k = d->k; a.sequential = d->sequential;
  a.pool = pool_args(d->prior, d->stamp, d->window, d->ld_window);
  a.tau = d->tau; a.tau_u = d->tau_u;
  a.base_max = d->base_max; a.base_logsum = d->base_logsum;
  a.out_logp = d->out_logp; a.out_total = d->out_total;
  NrProfScope ps(s, "logp_rows[U=%d,N=%d,k=%d,seq=%d]", d->U, d->N, d->k, d->sequential);
  const size_t smem = tk_tile_bytes(16, d->N) + (size_t)2 * 16 * TK_ROWS * sizeof(int32_t);
  NR_CHECK_RC(with_bool(a.pool.any(), [&](auto p) {
    return launch_lds(logp_rows_kernel<decltype(p)::value>, dim3((unsigned)((d->U + 15) / 16)), dim3(TK_THREADS), smem, s, a);
  }));
  NR_CHECK_LAUNCH();
  return NR_OK;
}

int nr_row_logprob_grad(const nr_logprob_grad_desc* d, nr_stream_t stream) {
  NR_CHECK_ARG(d != nullptr, "row_logprob_grad: null descriptor");
  NR_CHECK_ARG(d->k >= 1 && d->k <= NR_TOPK_MAX_K, "row_logprob_grad: k = %d entries per row, must be in [1, %d]", d->k, NR_TOPK_MAX_K);
  NR_CHECK_RC(check_vectors("row_logprob_grad", d->V, d->U, d->N));
  NR_CHECK_ARG(d->tau_u != nullptr || (d->tau > 0.f && d->tau < LZ_INF), "row_logprob_grad: tau = %g, a scalar temperature must be finite and > 0",
               (double)d->tau);
  NR_CHECK_RC(check_pools("row_logprob_grad", d->stamp, d->window, d->ld_window));
  NR_CHECK_ARG(d->news_vecs && d->user && d->row_ids && d->base_max && d->base_logsum && d->out_weight && d->out_sub_w,
               "row_logprob_grad: null pointer (news_vecs, user, row_ids, base_max, base_logsum, out_weight, out_sub_w)");
  NR_CHECK_RC(check_rows("row_logprob_grad", d->news_vecs, d->ld_news, d->user, d->ld_user, d->N));
  NR_CHECK_ARG(d->ld_ids >= d->k, "row_logprob_grad: id row stride %d < k = %d", d->ld_ids, d->k);
  NR_CHECK_ARG(d->g == nullptr || d->ld_g >= d->k, "row_logprob_grad: g row stride %d < k = %d", d->ld_g, d->k);
  NR_DEVICE_GUARD(stream, d->news_vecs);
  hipStream_t s = (hipStream_t)stream;
  LogpGradArgs a;
  a.news = d->news_vecs; a.user = d->user; a.ids = d->row_ids;
  a.ld_news = (size_t)d->ld_news; a.ld_user = (size_t)d->ld_user; a.ld_ids = (size_t)d->ld_ids; a.ld_g = (size_t)d->ld_g;
  a.V = d->V; a.U = d->U; a.N = d->N; a.k = d->k;
  a.pool = pool_args(d->prior, d->stamp, d->window, d->ld_window);
  a.tau = d->tau; a.tau_u = d->tau_u;
  a.base_max = d->base_max; a.base_logsum = d->base_logsum;
  a.g = d->g; a.out_weight = d->out_weight; a.out_sub_w = d->out_sub_w;
  NrProfScope ps(s, "logp_grad[U=%d,N=%d,k=%d]", d->U, d->N, d->k);
  const size_t smem = tk_tile_bytes(16, d->N) + (size_t)2 * 16 * TK_ROWS * sizeof(int32_t);
  NR_CHECK_RC(with_bool(a.pool.any(), [&](auto p) {
    return launch_lds(logp_grad_kernel<decltype(p)::value>, dim3((unsigned)((d->U + 15) / 16)), dim3(TK_THREADS), smem, s, a);
  }));
  NR_CHECK_LAUNCH();
  return NR_OK;
}

}  // extern "C"
