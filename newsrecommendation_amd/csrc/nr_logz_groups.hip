// Propensities under group caps: the log-partition of a user's score row PER GROUP (K15), and on these the log-probabilities of
// the entries of rows drawn by the capped sampler (K16) and the coefficients of their gradient (K21).  The fourth consumer of the tile of nr_score_tile.h, built like
// nr_logz.hip: scores and eligibility come from score_key / pool_key, so one (u, v) pair has here the bits and the verdict it
// has in nr_score_topk, nr_score_sample and nr_score_logz.
//
//   logzg_stream_kernel<MT, POOL, LISTS>   logz_stream_kernel of nr_logz.hip over the group-major order of the corpus (include/
//                           nrhip.h, K15): chunk row r is table row order[p + r] (ScoreOrderedRows), a position whose id is 0 is
//                           padding and never eligible, prior and stamp are gathered by id.  Segments come from a table, never
//                           straddle two bins and hold at most S chunks; a slice (blockIdx.y) is a run of whole segments, cut
//                           by positions so that slices carry about the same number of chunks (lg_plan).  The
//                           per-lane (max, sum, count) chain, the segment-end reduction and the store of ONE partial per (user,
//                           segment) are those of logz_stream_kernel; so are the cursor and the masks of the lists, which are
//                           given in position space.
//   logzg_final_kernel      one thread per (user, bin): the maximum of the bin's partials (exact), their sums rescaled to it and
//                           added in fp64 in ascending segment order, one log, rounded to fp32 once.
//   logp_capped_kernel<POOL>   the named-row gather of logp_rows_kernel, then per user one wave in fp64 (K16): the step t_b at
//                           which the row fills each of its bins, the never-closing bins joined in a fixed order, and the walk
//                           from the last place to the first.  Only positive terms are added.
//   logp_capped_grad_kernel<POOL>   the sibling of logp_capped_kernel for the gradient of the capped row (K21): the same gather, t_b
//                           and walk, each D_j kept as (M_j, sigma_j) by the lane that holds place j; then the inclusive prefix scan
//                           of (-M_j, g_j / sigma_j) of K19, omega per bin and c per entry.
#include <math.h>

#include "nr_score_tile.h"

namespace {

constexpr int LG_MAX_SEGS = 256;            // segments the chunk budget is cut into; every bin may add a short one
constexpr float LG_INF = __builtin_inff();

struct LogzgPlan {
  int TU, splits;
};
// `splits` (0: fill the chip) only groups whole segments into slices; the segments are the caller's table.  Segments differ in
// length (a small bin is one short segment), so a slice is cut by positions, not by segment count: slice y of s takes the
// segments that START in [y * n_pos / s, (y + 1) * n_pos / s) -- at most a segment more than its share of the chunks.  A slice
// may come out empty; every segment falls into exactly one.  With as many slices as segments (few users: the auto choice) slice y
// is segment y.
inline LogzgPlan lg_plan(int U, int V, int N, int nseg, int splits) {
  LogzgPlan p;
  p.TU = score_user_tile(N, 0);
  long s = splits > 0 ? splits : score_auto_splits(U, V, p.TU, nseg);
  if (s > nseg) s = nseg;
  if (s < 1) s = 1;
  p.splits = (int)s;
  return p;
}

struct LogzgArgs {
  const float* news;
  const float* user;
  size_t ld_news, ld_user;
  int V, U, N, nseg, n_pos, n_bins;
  const int32_t* order;     // [n_pos]
  const int32_t* seg_start; // [nseg + 1]
  const int32_t* bin_seg;   // [n_bins + 1]
  PoolArgs pool;            // read by the POOL instantiations only; indexed by news id
  float tau;
  const float* tau_u;
  float* pm;                // [U, nseg] partial maxima, -inf = nothing eligible in the segment
  float* ps;                // [U, nseg] partial sums of exp((x - pm) / tau)
  int32_t* pc;              // [U, nseg] eligible news of the segment
  __device__ __forceinline__ float tau_of(long u) const { return tau_u != nullptr ? tau_u[u] : tau; }
  // a position read from the segment table, clamped into [0, n_pos]
  __device__ __forceinline__ long start_of(int sg) const {
    const int32_t p = seg_start[sg];
    return p < 0 ? 0 : (p > n_pos ? n_pos : p);
  }
  // the first segment that starts at or after position p, nseg if none: a binary search that stays in [0, nseg] whatever the table holds
  __device__ __forceinline__ int first_from(long p) const {
    int lo = 0, hi = nseg;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (start_of(mid) < p) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  }
};
// workspace: the three [U, nseg] arrays, 12 bytes per (user, segment), rounded to 8
inline size_t lg_carve(void* ws, int U, int nseg, LogzgArgs* a) {
  char* p = reinterpret_cast<char*>(ws);
  const size_t n = (size_t)U * nseg;
  if (a) {
    a->pm = reinterpret_cast<float*>(p);
    a->ps = reinterpret_cast<float*>(p + n * 4);
    a->pc = reinterpret_cast<int32_t*>(p + n * 8);
  }
  return (n * 12 + 7) & ~(size_t)7;
}

// lz_take of nr_logz.hip: one eligible news x into a lane's running (m, s)
__device__ __forceinline__ void lg_take(float x, float it, float& m, float& s) {
  const bool up = x > m;
  const float d = up ? m - x : x - m;
  const float e = x == m ? 1.f : expf(d * it);
  s = up ? fmaf(s, e, 1.f) : s + e;
  m = up ? x : m;
}

template <int MT, bool POOL, bool LISTS>
__global__ __launch_bounds__(TK_THREADS) void logzg_stream_kernel(LogzgArgs a, CsrArgs ca) {
  constexpr int TU = 16 * MT, PER_WAVE = TU / TK_WAVES;
  extern __shared__ __attribute__((aligned(16))) float lg_smem[];
  ScoreTile<MT> t(lg_smem, a.N);
  const int lane = t.lane, wave = t.wave;
  const int u0 = blockIdx.x * TU;
  const bool one = (int)gridDim.y == a.nseg;                  // as many slices as segments: slice y is segment y
  const int s_lo = one ? (int)blockIdx.y : a.first_from((long)blockIdx.y * a.n_pos / gridDim.y);
  const int s_hi = one ? s_lo + 1 : blockIdx.y + 1 == gridDim.y ? a.nseg : a.first_from((long)(blockIdx.y + 1) * a.n_pos / gridDim.y);
  if (s_lo >= s_hi) return;                                   // the whole workgroup: no segment starts in this slice's share
  const long v_lo = a.start_of(s_lo), v_hi = a.start_of(s_hi);
  if (v_lo >= v_hi) return;

  t.load_users(a.user, a.ld_user, u0, a.U);
  float it[PER_WAVE], m[PER_WAVE], s[PER_WAVE];
  int32_t cnt[PER_WAVE];
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int u = u0 + wave + TK_WAVES * i;
    it[i] = __fdiv_rn(1.f, u < a.U ? a.tau_of(u) : 1.f);
    m[i] = -LG_INF;
    s[i] = 0.f;
    cnt[i] = 0;
  }
  // LISTS: the cursor of every user of the wave = the first entry (a position) of its segment that is >= v_lo; the 64-ary search of
  // logz_stream_kernel.  Every index formed lies in [lo, hi) within the clamped segment.
  int32_t cur[PER_WAVE], end[PER_WAVE];
  if constexpr (LISTS) {
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      const int u = u0 + wave + TK_WAVES * i;
      cur[i] = end[i] = 0;
      if (u < a.U) ca.segment(u, cur[i], end[i]);
    }
    int32_t hi[PER_WAVE];
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) hi[i] = end[i];
    for (;;) {
      int32_t val[PER_WAVE], step[PER_WAVE];
#pragma unroll
      for (int i = 0; i < PER_WAVE; ++i) {
        const int32_t n = hi[i] - cur[i];
        step[i] = (n + 63) >> 6;
        const long idx = (long)cur[i] + (long)lane * step[i];
        val[i] = n > 0 && idx < hi[i] ? ca.ids[idx] : 0x7fffffff;
      }
      bool open = false;
#pragma unroll
      for (int i = 0; i < PER_WAVE; ++i) {
        const int32_t n = hi[i] - cur[i];
        if (n <= 0) continue;
        const long idx = (long)cur[i] + (long)lane * step[i];
        const int p = __popcll(__ballot(idx < hi[i] && (long)val[i] < v_lo));
        if (p == 0) hi[i] = cur[i];
        else if (step[i] == 1) { cur[i] += p; hi[i] = cur[i]; }
        else {
          const long nh = (long)cur[i] + (long)p * step[i];
          cur[i] = (int32_t)((long)cur[i] + (long)(p - 1) * step[i] + 1);
          hi[i] = nh < hi[i] ? (int32_t)nh : hi[i];
        }
        open = open || hi[i] > cur[i];
      }
      if (!open) break;
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

  int sg = s_lo;                                              // the segment the chunk at vc lies in, and where it ends
  long sg_end = a.start_of(sg + 1);
  ScoreOrderedRows rows = {a.news, a.ld_news, a.order, a.V, v_hi, 0, 0};
  rows.seek(v_lo, t.srow);
  t.load_slab(rows, 0);
  for (long vc = v_lo; vc < v_hi; vc += TK_ROWS) {
    f32x4 acc[MT];
    t.chunk(rows, acc);
    if (vc + TK_ROWS < v_hi) {
      rows.seek(vc + TK_ROWS, t.srow);
      t.load_slab(rows, 0);                                   // in flight while this chunk is summed
    }
    // the ids of the chunk's 128 positions, two per lane (coalesced); POOL: their prior and stamp, gathered by id
    const int32_t i0 = vc + lane < v_hi ? a.order[vc + lane] : 0, i1 = vc + lane + 64 < v_hi ? a.order[vc + lane + 64] : 0;
    const bool r0 = i0 >= 1 && i0 < a.V, r1 = i1 >= 1 && i1 < a.V;
    float p0 = 0.f, p1 = 0.f;
    int32_t s0 = 0, s1 = 0;
    if constexpr (POOL) {
      if (r0) {
        p0 = a.pool.prior_of(i0);
        s0 = a.pool.stamp_of(i0);
      }
      if (r1) {
        p1 = a.pool.prior_of(i1);
        s1 = a.pool.stamp_of(i1);
      }
    }
    int32_t e0[LISTS ? PER_WAVE : 1];
    if constexpr (LISTS) {
#pragma unroll
      for (int i = 0; i < PER_WAVE; ++i) e0[i] = (long)cur[i] + lane < end[i] ? ca.ids[(long)cur[i] + lane] : 0x7fffffff;
    }
    t.put_scores(acc);
    const float* sS = t.scores();
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      const int ul = wave + TK_WAVES * i;
      // LISTS: the entries inside [vc, vc + 128) are a prefix of what the cursor points at; bit r of (l0, l1) = position vc + r is listed
      u64 l0 = 0ull, l1 = 0ull;
      if constexpr (LISTS) {
        int32_t e = e0[i];
        for (;;) {
          const int c = __popcll(__ballot((long)cur[i] + lane < end[i] && (long)e < vc + TK_ROWS));
          for (int j = 0; j < c; ++j) {
            const uint32_t r = (uint32_t)((long)__builtin_amdgcn_readlane(e, j) - vc);
            if (r < 64u) l0 |= 1ull << r;
            else if (r < 128u) l1 |= 1ull << (r - 64u);
          }
          cur[i] += c;
          if (c < 64) break;                                  // a full probe: the chunk may hold 64 more
          e = (long)cur[i] + lane < end[i] ? ca.ids[(long)cur[i] + lane] : 0x7fffffff;
        }
      }
      uint32_t k0, k1;
      if constexpr (POOL) {
        const int32_t lo = __builtin_amdgcn_readlane(w_lo, i), hi = __builtin_amdgcn_readlane(w_hi, i);
        k0 = pool_key(sS[ul * TK_LDS_TILE + lane], p0, s0, lo, hi);
        k1 = pool_key(sS[ul * TK_LDS_TILE + lane + 64], p1, s1, lo, hi);
      } else {
        k0 = score_key(sS[ul * TK_LDS_TILE + lane]);
        k1 = score_key(sS[ul * TK_LDS_TILE + lane + 64]);
      }
      // eligible: a real news (not padding), key != 0 (not NaN, inside the pool), not listed
      const bool el0 = r0 && k0 != 0u && ((l0 >> lane) & 1ull) == 0ull;
      const bool el1 = r1 && k1 != 0u && ((l1 >> lane) & 1ull) == 0ull;
      if (el0) {
        lg_take(key_score(k0), it[i], m[i], s[i]);
        ++cnt[i];
      }
      if (el1) {
        lg_take(key_score(k1), it[i], m[i], s[i]);
        ++cnt[i];
      }
    }
    // segment end: one partial per (user, segment), in an order that the segment table alone fixes
    const long nxt = vc + TK_ROWS;
    if (nxt >= v_hi || nxt >= sg_end) {
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
        m[i] = -LG_INF;
        s[i] = 0.f;
        cnt[i] = 0;
      }
      if (sg + 1 < s_hi) {                                    // sg stays inside the slice whatever the table holds
        ++sg;
        sg_end = a.start_of(sg + 1);
      }
    }
    __syncthreads();                                          // the score tile is the next chunk's staging buffer
  }
}

// One thread per (user, bin): the bin's partials in ascending segment order
__global__ __launch_bounds__(256) void logzg_final_kernel(LogzgArgs a, float* __restrict__ out_logsum, float* __restrict__ out_max,
                                                          int32_t* __restrict__ out_count) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)a.U * a.n_bins) return;
  const size_t u = idx / a.n_bins;
  const int b = (int)(idx - u * a.n_bins);
  int lo = a.bin_seg[b], hi = a.bin_seg[b + 1];
  lo = lo < 0 ? 0 : (lo > a.nseg ? a.nseg : lo);
  hi = hi < lo ? lo : (hi > a.nseg ? a.nseg : hi);
  float M = -LG_INF;
  int32_t n = 0;
  for (int j = lo; j < hi; ++j) {
    M = fmaxf(M, a.pm[u * a.nseg + j]);
    n += a.pc[u * a.nseg + j];
  }
  const float tau = a.tau_of(u);
  const bool tau_ok = tau > 0.f && tau < LG_INF;
  float ls;
  if (n == 0) ls = -LG_INF;
  else if (!tau_ok || !(fabsf(M) < LG_INF)) ls = __builtin_nanf("");
  else {
    const double it = (double)__fdiv_rn(1.f, tau);
    double S = 0.0;
    for (int j = lo; j < hi; ++j) {
      const float mj = a.pm[u * a.nseg + j];
      if (mj != -LG_INF) S += (double)a.ps[u * a.nseg + j] * (mj == M ? 1.0 : exp(((double)mj - (double)M) * it));
    }
    ls = (float)log(S);
  }
  out_logsum[idx] = ls;
  out_max[idx] = M;
  out_count[idx] = n;
}

// ---- K16 ----------------------------------------------------------------------------------------------------------------

struct LogpcArgs {
  const float* news;
  const float* user;
  const int32_t* ids;
  const int32_t* group;
  size_t ld_news, ld_user, ld_ids, ld_base;
  int V, U, N, k, cap, G;
  PoolArgs pool;
  float tau;
  const float* tau_u;
  const float* base_max;
  const float* base_logsum;
  float* out_logp;
  float* out_total;         // [U] or null
};

// (m, s): s = sum of exp((x_i - m) / tau) over a set with maximum m; (-inf, 0) is the empty set
struct LgPair {
  double m, s;
};
__device__ __forceinline__ LgPair lg_join(LgPair x, LgPair y, double tau) {
  const double M = fmax(x.m, y.m);
  const double ex = x.m == M ? 1.0 : exp((x.m - M) / tau), ey = y.m == M ? 1.0 : exp((y.m - M) / tau);
  return {M, x.s * ex + y.s * ey};
}

// per-wave scratch of the fp64 phase; it overlays the staging buffers of the tile, which the gather no longer needs
constexpr int LC_CLOSE = 528;                                 // bytes of the "closes at" table: bins 0 .. 512
constexpr int LC_WAVE_BYTES = 2 * TK_ROWS * 8 + 2 * TK_ROWS * 4 + LC_CLOSE;
static_assert(TK_WAVES * LC_WAVE_BYTES <= TK_STAGE_FLOATS * 4, "the fp64 phase must fit the staging buffers");
static_assert(NR_RANK_MAX_GROUPS + 1 <= LC_CLOSE && LC_WAVE_BYTES % 8 == 0, "one byte per bin");

template <bool POOL>
__global__ __launch_bounds__(TK_THREADS) void logp_capped_kernel(LogpcArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lc_smem[];
  ScoreTile<1> t(lc_smem, a.N);
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

  // one wave per user, in fp64.  Every wave runs both rounds and every barrier; a wave without a user only skips the work.
  char* scratch = reinterpret_cast<char*>(t.sB) + (size_t)wave * LC_WAVE_BYTES;
  double* stM = reinterpret_cast<double*>(scratch);           // [128] stash of the bin that closes at place j: its later entries
  double* stS = stM + TK_ROWS;
  int32_t* sBin = reinterpret_cast<int32_t*>(stS + TK_ROWS);  // [128] bin of a live entry, -1 otherwise
  int32_t* sTc = sBin + TK_ROWS;                              // [128] the place at which the entry's bin closes, -1 = never
  unsigned char* sClose = reinterpret_cast<unsigned char*>(sTc + TK_ROWS);   // [G + 1] that place per bin, 0xff = never
  const double NaN = __builtin_nan(""), NINF = -(double)LG_INF;
  const LgPair none = {NINF, 0.0};
  for (int c0 = 0; c0 < 16; c0 += TK_WAVES) {
    const int c = c0 + wave;
    const bool active = c < users;
    const size_t u = (size_t)(u0 + (active ? c : 0));
    const int j0 = 2 * lane, j1 = j0 + 1;
    int b0 = -1, b1 = -1;
    if (active) {
      // lane l holds entries 2 l and 2 l + 1: the bin of a live entry (group id, or G for no group)
      const int32_t id0 = sIds[c * TK_ROWS + j0], id1 = sIds[c * TK_ROWS + j1];
      if (sKey[c * TK_ROWS + j0] != 0u) {
        const int32_t g = a.group[id0];
        b0 = g >= 0 && g < a.G ? g : a.G;
      }
      if (sKey[c * TK_ROWS + j1] != 0u) {
        const int32_t g = a.group[id1];
        b1 = g >= 0 && g < a.G ? g : a.G;
      }
      sBin[j0] = b0;
      sBin[j1] = b1;
      stM[j0] = stM[j1] = NINF;
      stS[j0] = stS[j1] = 0.0;
      for (int b = lane; b <= a.G; b += 64) sClose[b] = 0xff;
    }
    __syncthreads();
    if (active) {
      // the c-th live entry of a group closes it: the entry with cap - 1 live entries of its bin before it
      int n0 = 0, n1 = 0;
      for (int i = 0; i < j1; ++i) {
        const int32_t bi = sBin[i];
        n0 += (i < j0 && bi == b0) ? 1 : 0;
        n1 += (bi == b1) ? 1 : 0;
      }
      if (b0 >= 0 && b0 < a.G && n0 == a.cap - 1) sClose[b0] = (unsigned char)j0;
      if (b1 >= 0 && b1 < a.G && n1 == a.cap - 1) sClose[b1] = (unsigned char)j1;
    }
    __syncthreads();
    LgPair open = none;
    double tau = 1.0;
    bool tau_ok = false;
    if (active) {
      sTc[j0] = b0 >= 0 && b0 < a.G && sClose[b0] != 0xff ? (int32_t)sClose[b0] : -1;
      sTc[j1] = b1 >= 0 && b1 < a.G && sClose[b1] != 0xff ? (int32_t)sClose[b1] : -1;
      const float tau_f = a.tau_u != nullptr ? a.tau_u[u] : a.tau;
      tau_ok = tau_f > 0.f && tau_f < LG_INF;
      tau = (double)tau_f;
      // the bins that never close, bin G among them: each lane its bins in ascending order, then the xor butterfly
      for (int b = lane; b <= a.G; b += 64)
        if (sClose[b] == 0xff) {
          const LgPair B = {(double)a.base_max[u * a.ld_base + b], exp((double)a.base_logsum[u * a.ld_base + b])};
          open = lg_join(open, B, tau);
        }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const LgPair other = {__shfl_xor(open.m, o, 64), __shfl_xor(open.s, o, 64)};
        open = lg_join(open, other, tau);
      }
    }
    __syncthreads();
    if (active) {
      // the walk, from the last place to the first, the same in every lane (what it reads is wave-uniform; every lane stores
      // the same stash values and reads back what it stored itself)
      LgPair acc = open;
      double tot = 0.0;
      for (int j = a.k - 1; j >= 0; --j) {
        const int32_t id = sIds[c * TK_ROWS + j];
        if (!(id >= 1 && id < a.V)) {                         // fill: logp 0, in no sum
          if (lane == 0) a.out_logp[u * a.k + j] = 0.f;
          continue;
        }
        const uint32_t key = sKey[c * TK_ROWS + j];
        double lp;
        if (key == 0u || !tau_ok) lp = NaN;                   // key 0: in no sum, uses up nothing of a cap
        else {
          const double x = (double)key_score(key);
          const LgPair P = {x, 1.0};
          const int32_t tc = sTc[j];
          if (tc >= 0 && j > tc) {                            // capped out: its weight waits for the step its bin was last open
            const LgPair st = lg_join({stM[tc], stS[tc]}, P, tau);
            stM[tc] = st.m;
            stS[tc] = st.s;
            lp = NINF;
          } else {
            acc = lg_join(acc, P, tau);
            if (tc == j) {                                    // from here down the bin is open: its base and the stashed entries
              const int b = sBin[j];
              const LgPair B = {(double)a.base_max[u * a.ld_base + b], exp((double)a.base_logsum[u * a.ld_base + b])};
              acc = lg_join(acc, lg_join(B, {stM[j], stS[j]}, tau), tau);
            }
            lp = (x - acc.m) / tau - log(acc.s);
          }
        }
        tot += lp;
        if (lane == 0) a.out_logp[u * a.k + j] = (float)lp;
      }
      if (lane == 0 && a.out_total != nullptr) a.out_total[u] = (float)tot;
    }
    __syncthreads();                                          // the scratch is the next round's
  }
}

// ---- K21 ----------------------------------------------------------------------------------------------------------------

struct LogpcGradArgs {
  const float* news;
  const float* user;
  const int32_t* ids;
  const int32_t* group;
  size_t ld_news, ld_user, ld_ids, ld_base, ld_g;
  int V, U, N, k, cap, G;
  PoolArgs pool;
  float tau;
  const float* tau_u;
  const float* base_max;
  const float* base_logsum;
  const float* g;           // [U, ld_g] or null = 1
  float* out_bin_w;         // [U, ld_base]
  float* out_sub_w;         // [U, k]
};

__device__ __forceinline__ LgPair lg_up(LgPair x, int o) { return {__shfl_up(x.m, o, 64), __shfl_up(x.s, o, 64)}; }

// The gradient coefficients of the capped row (include/nrhip.h, K21): the gather, the t_b and the walk of logp_capped_kernel,
// statement for statement, so an entry has K16's key and a live step j K16's D_j = exp(M_j / tau) sigma_j; the lane that holds
// entry j keeps (M_j, sigma_j).  Then K19's inclusive prefix scan of (-M_j, g_j / sigma_j) over the live steps -- the supports of
// the steps are nested, so M_j does not increase with j -- and
//   omega_b = exp((gmax_b - M_{t_b}) / tau + logsum_b) q_{t_b},   c_i = g_i - exp((x_i - M_i) / tau) q_i   (blocked: the q of t_bin(i))
// form no exponent above 0.
template <bool POOL>
__global__ __launch_bounds__(TK_THREADS) void logp_capped_grad_kernel(LogpcGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lc_smem[];
  ScoreTile<1> t(lc_smem, a.N);
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

  // one wave per user, in fp64.  Every wave runs both rounds and every barrier; a wave without a user only skips the work.
  char* scratch = reinterpret_cast<char*>(t.sB) + (size_t)wave * LC_WAVE_BYTES;
  double* stM = reinterpret_cast<double*>(scratch);           // [128] the walk's stash; afterwards the prefix q of every place
  double* stS = stM + TK_ROWS;
  int32_t* sBin = reinterpret_cast<int32_t*>(stS + TK_ROWS);  // [128] bin of a live entry, -1 otherwise
  int32_t* sTc = sBin + TK_ROWS;                              // [128] the place at which the entry's bin closes, -1 = never
  unsigned char* sClose = reinterpret_cast<unsigned char*>(sTc + TK_ROWS);   // [G + 1] that place per bin, 0xff = never
  const double NINF = -(double)LG_INF;
  const LgPair none = {NINF, 0.0};
  for (int c0 = 0; c0 < 16; c0 += TK_WAVES) {
    const int c = c0 + wave;
    const bool active = c < users;
    const size_t u = (size_t)(u0 + (active ? c : 0));
    const int j0 = 2 * lane, j1 = j0 + 1;
    int b0 = -1, b1 = -1;
    if (active) {
      const int32_t id0 = sIds[c * TK_ROWS + j0], id1 = sIds[c * TK_ROWS + j1];
      if (sKey[c * TK_ROWS + j0] != 0u) {
        const int32_t g = a.group[id0];
        b0 = g >= 0 && g < a.G ? g : a.G;
      }
      if (sKey[c * TK_ROWS + j1] != 0u) {
        const int32_t g = a.group[id1];
        b1 = g >= 0 && g < a.G ? g : a.G;
      }
      sBin[j0] = b0;
      sBin[j1] = b1;
      stM[j0] = stM[j1] = NINF;
      stS[j0] = stS[j1] = 0.0;
      for (int b = lane; b <= a.G; b += 64) sClose[b] = 0xff;
    }
    __syncthreads();
    if (active) {
      // the c-th live entry of a group closes it: the entry with cap - 1 live entries of its bin before it
      int n0 = 0, n1 = 0;
      for (int i = 0; i < j1; ++i) {
        const int32_t bi = sBin[i];
        n0 += (i < j0 && bi == b0) ? 1 : 0;
        n1 += (bi == b1) ? 1 : 0;
      }
      if (b0 >= 0 && b0 < a.G && n0 == a.cap - 1) sClose[b0] = (unsigned char)j0;
      if (b1 >= 0 && b1 < a.G && n1 == a.cap - 1) sClose[b1] = (unsigned char)j1;
    }
    __syncthreads();
    LgPair open = none;
    double tau = 1.0;
    bool dead = true;                                         // all zeros: a bad temperature, a NaN in a base
    if (active) {
      sTc[j0] = b0 >= 0 && b0 < a.G && sClose[b0] != 0xff ? (int32_t)sClose[b0] : -1;
      sTc[j1] = b1 >= 0 && b1 < a.G && sClose[b1] != 0xff ? (int32_t)sClose[b1] : -1;
      const float tau_f = a.tau_u != nullptr ? a.tau_u[u] : a.tau;
      const bool tau_ok = tau_f > 0.f && tau_f < LG_INF;
      tau = tau_ok ? (double)tau_f : 1.0;
      bool nan = false;
      // the bins that never close, bin G among them: each lane its bins in ascending order, then the xor butterfly
      for (int b = lane; b <= a.G; b += 64) {
        const float gm = a.base_max[u * a.ld_base + b], bl = a.base_logsum[u * a.ld_base + b];
        nan = nan || gm != gm || (gm != -LG_INF && bl != bl);
        if (sClose[b] == 0xff) {
          const LgPair B = {(double)gm, exp((double)bl)};
          open = lg_join(open, B, tau);
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const LgPair other = {__shfl_xor(open.m, o, 64), __shfl_xor(open.s, o, 64)};
        open = lg_join(open, other, tau);
      }
      dead = !tau_ok || __any(nan);
    }
    __syncthreads();
    LgPair S0 = none, S1 = none;                              // (M_j, sigma_j) of this lane's two places, where they are live steps
    bool step0 = false, step1 = false;
    if (active && !dead) {
      // the walk, from the last place to the first, the same in every lane; the lane that holds place j keeps its D_j
      LgPair acc = open;
      for (int j = a.k - 1; j >= 0; --j) {
        const uint32_t key = sKey[c * TK_ROWS + j];
        if (key == 0u) continue;                              // fill or key 0: no step, in no sum
        const LgPair P = {(double)key_score(key), 1.0};
        const int32_t tc = sTc[j];
        if (tc >= 0 && j > tc) {                              // blocked: its weight waits for the step its bin was last open
          const LgPair st = lg_join({stM[tc], stS[tc]}, P, tau);
          stM[tc] = st.m;
          stS[tc] = st.s;
        } else {
          acc = lg_join(acc, P, tau);
          if (tc == j) {
            const int b = sBin[j];
            const LgPair B = {(double)a.base_max[u * a.ld_base + b], exp((double)a.base_logsum[u * a.ld_base + b])};
            acc = lg_join(acc, lg_join(B, {stM[j], stS[j]}, tau), tau);
          }
          if (j == j0) {
            S0 = acc;
            step0 = true;
          }
          if (j == j1) {
            S1 = acc;
            step1 = true;
          }
        }
      }
    }
    __syncthreads();                                          // the stash is read; its arrays take the prefix sums
    double x0 = 0.0, x1 = 0.0, g0 = 0.0, g1 = 0.0;
    LgPair all = none, Q0 = none, Q1 = none;
    if (active && !dead) {
      x0 = (double)key_score(sKey[c * TK_ROWS + j0]);
      x1 = (double)key_score(sKey[c * TK_ROWS + j1]);
      g0 = step0 ? 1.0 : 0.0;
      g1 = step1 ? 1.0 : 0.0;                                 // the g of anything that is no step is not read
      if (a.g != nullptr) {
        if (step0) g0 = (double)a.g[u * a.ld_g + j0];
        if (step1) g1 = (double)a.g[u * a.ld_g + j1];
      }
      // inclusive prefix scan of (-M_j, g_j / sigma_j) over the live steps (sigma_j >= 1 there)
      const LgPair T0 = step0 ? LgPair{-S0.m, g0 / S0.s} : none, T1 = step1 ? LgPair{-S1.m, g1 / S1.s} : none;
      LgPair Q = lg_join(T0, T1, tau);
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const LgPair other = lg_up(Q, o);
        if (lane >= o) Q = lg_join(other, Q, tau);
      }
      LgPair before = lg_up(Q, 1);                            // places 0 .. 2 l - 1
      if (lane == 0) before = none;
      Q0 = lg_join(before, T0, tau);
      Q1 = lg_join(Q0, T1, tau);
      all = {__shfl(Q.m, 63, 64), __shfl(Q.s, 63, 64)};
      stM[j0] = Q0.m;
      stS[j0] = Q0.s;
      stM[j1] = Q1.m;
      stS[j1] = Q1.s;
    }
    __syncthreads();
    if (active) {
      // c: at a live step q.m = -M_i; a blocked entry takes the q of the step that closed its bin, whose D holds its weight
      double c0v = 0.0, c1v = 0.0;
      if (!dead) {
        const int32_t tc0 = sTc[j0], tc1 = sTc[j1];
        if (step0) c0v = g0 - exp((x0 + Q0.m) / tau) * Q0.s;
        else if (b0 >= 0 && tc0 >= 0 && j0 > tc0) c0v = -exp((x0 + stM[tc0]) / tau) * stS[tc0];
        if (step1) c1v = g1 - exp((x1 + Q1.m) / tau) * Q1.s;
        else if (b1 >= 0 && tc1 >= 0 && j1 > tc1) c1v = -exp((x1 + stM[tc1]) / tau) * stS[tc1];
      }
      if (j0 < a.k) a.out_sub_w[u * a.k + j0] = (float)c0v;
      if (j1 < a.k) a.out_sub_w[u * a.k + j1] = (float)c1v;
      // omega: lanes striding the bins; a closed bin takes the q of its closing step, an open one the q of the last live step
      for (int b = lane; b <= a.G; b += 64) {
        double w = 0.0;
        if (!dead && all.m != NINF) {
          const double gm = (double)a.base_max[u * a.ld_base + b], bl = (double)a.base_logsum[u * a.ld_base + b];
          const int cl = sClose[b];
          const double qm = cl == 0xff ? all.m : stM[cl], qs = cl == 0xff ? all.s : stS[cl];
          if (gm != NINF) w = exp((gm + qm) / tau + bl) * qs;
        }
        a.out_bin_w[u * a.ld_base + b] = (float)w;
      }
    }
    __syncthreads();                                          // the scratch is the next round's
  }
}

// argument checks shared by the size query and the call; 0 = fine
int logzg_check(const nr_logz_groups_desc* d) {
  NR_CHECK_ARG(d != nullptr, "score_logz_groups: null descriptor");
  NR_CHECK_RC(check_vectors("score_logz_groups", d->V, d->U, d->N));
  NR_CHECK_RC(check_lists("score_logz_groups", 0, d->excl_offsets, d->excl_ids, d->n_excl));
  NR_CHECK_ARG(d->tau_u != nullptr || (d->tau > 0.f && d->tau < LG_INF),
               "score_logz_groups: tau = %g, a scalar temperature must be finite and > 0", (double)d->tau);
  NR_CHECK_ARG(d->n_groups >= 1 && d->n_groups <= NR_RANK_MAX_GROUPS, "score_logz_groups: n_groups = %d, must be in [1, %d]", d->n_groups,
               NR_RANK_MAX_GROUPS);
  NR_CHECK_ARG(d->n_pos >= TK_ROWS && d->n_pos % TK_ROWS == 0, "score_logz_groups: n_pos = %d positions, must be a positive multiple of %d",
               d->n_pos, TK_ROWS);
  NR_CHECK_ARG(d->nseg >= 1 && d->nseg <= LG_MAX_SEGS + d->n_groups + 1 && d->nseg <= d->n_pos / TK_ROWS,
               "score_logz_groups: nseg = %d segments, must be in [1, %d] and at most the %d chunks", d->nseg, LG_MAX_SEGS + d->n_groups + 1,
               d->n_pos / TK_ROWS);
  NR_CHECK_ARG(d->splits >= 0 && d->splits <= d->nseg, "score_logz_groups: splits = %d, must be 0 (library's choice) or in [1, %d], the segments",
               d->splits, d->nseg);
  return check_pools("score_logz_groups", d->stamp, d->window, d->ld_window);
}

int logzg_stream_launch(int TU, bool pool, bool lists, dim3 grid, size_t smem, hipStream_t s, const LogzgArgs& a, const CsrArgs& ca) {
  return with_int<64, 32, 16>(TU, [&](auto tu) {
    return with_bool(pool, [&](auto p) {
      return with_bool(lists, [&](auto l) {
        return launch_lds(logzg_stream_kernel<decltype(tu)::value / 16, decltype(p)::value, decltype(l)::value>, grid, dim3(TK_THREADS), smem, s, a, ca);
      });
    });
  });
}

}  // namespace

extern "C" {

size_t nr_score_logz_groups_workspace_bytes(const nr_logz_groups_desc* d) {
  if (logzg_check(d) != NR_OK) return 0;
  return lg_carve(nullptr, d->U, d->nseg, nullptr);
}

int nr_score_logz_groups(const nr_logz_groups_desc* d, nr_stream_t stream) {
  NR_CHECK_RC(logzg_check(d));
  NR_CHECK_ARG(d->news_vecs && d->user && d->order && d->seg_start && d->bin_seg && d->out_logsum && d->out_max && d->out_count,
               "score_logz_groups: null pointer (news_vecs, user, order, seg_start, bin_seg, out_logsum, out_max, out_count)");
  NR_CHECK_RC(check_rows("score_logz_groups", d->news_vecs, d->ld_news, d->user, d->ld_user, d->N));
  NR_CHECK_RC(check_workspace("score_logz_groups", d->ws, d->ws_bytes, nr_score_logz_groups_workspace_bytes(d)));
  NR_DEVICE_GUARD(stream, d->news_vecs);
  hipStream_t s = (hipStream_t)stream;
  const LogzgPlan pl = lg_plan(d->U, d->V, d->N, d->nseg, d->splits);
  LogzgArgs a;
  a.news = d->news_vecs; a.user = d->user;
  a.ld_news = (size_t)d->ld_news; a.ld_user = (size_t)d->ld_user;
  a.V = d->V; a.U = d->U; a.N = d->N; a.nseg = d->nseg; a.n_pos = d->n_pos; a.n_bins = d->n_groups + 1;
  a.order = d->order; a.seg_start = d->seg_start; a.bin_seg = d->bin_seg;
  a.pool = pool_args(d->prior, d->stamp, d->window, d->ld_window);
  a.tau = d->tau; a.tau_u = d->tau_u;
  lg_carve(d->ws, d->U, d->nseg, &a);
  const CsrArgs ca = csr_args(d->excl_offsets, d->excl_ids, d->n_excl);
  {
    const int TU = pl.TU;
    const size_t smem = tk_tile_bytes(TU, d->N);
    const dim3 grid((unsigned)((d->U + TU - 1) / TU), (unsigned)pl.splits);
    NrProfScope ps(s, "logzg_stream[U=%d,V=%d,N=%d,TU=%d,splits=%d,nseg=%d,pos=%d]", d->U, d->V, d->N, TU, pl.splits, d->nseg, d->n_pos);
    NR_CHECK_RC(logzg_stream_launch(TU, a.pool.any(), ca.offsets != nullptr, grid, smem, s, a, ca));
  }
  NR_CHECK_LAUNCH();
  {
    NrProfScope ps(s, "logzg_final[U=%d,bins=%d,nseg=%d]", d->U, a.n_bins, d->nseg);
    const size_t n = (size_t)d->U * a.n_bins;
    hipLaunchKernelGGL(logzg_final_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, d->out_logsum, d->out_max, d->out_count);
  }
  NR_CHECK_LAUNCH();
  return NR_OK;
}

int nr_row_logprob_capped(const nr_logprob_capped_desc* d, nr_stream_t stream) {
  NR_CHECK_ARG(d != nullptr, "row_logprob_capped: null descriptor");
  NR_CHECK_ARG(d->k >= 1 && d->k <= NR_TOPK_MAX_K, "row_logprob_capped: k = %d entries per row, must be in [1, %d]", d->k, NR_TOPK_MAX_K);
  NR_CHECK_RC(check_vectors("row_logprob_capped", d->V, d->U, d->N));
  NR_CHECK_ARG(d->tau_u != nullptr || (d->tau > 0.f && d->tau < LG_INF),
               "row_logprob_capped: tau = %g, a scalar temperature must be finite and > 0", (double)d->tau);
  NR_CHECK_ARG(d->group_cap >= 1 && d->group_cap <= 128, "row_logprob_capped: group_cap = %d, must be in [1, 128]", d->group_cap);
  NR_CHECK_ARG(d->n_groups >= 1 && d->n_groups <= NR_RANK_MAX_GROUPS, "row_logprob_capped: n_groups = %d, must be in [1, %d]", d->n_groups,
               NR_RANK_MAX_GROUPS);
  NR_CHECK_RC(check_pools("row_logprob_capped", d->stamp, d->window, d->ld_window));
  NR_CHECK_ARG(d->news_vecs && d->user && d->row_ids && d->group && d->base_max && d->base_logsum && d->out_logp,
               "row_logprob_capped: null pointer (news_vecs, user, row_ids, group, base_max, base_logsum, out_logp)");
  NR_CHECK_RC(check_rows("row_logprob_capped", d->news_vecs, d->ld_news, d->user, d->ld_user, d->N));
  NR_CHECK_ARG(d->ld_ids >= d->k, "row_logprob_capped: id row stride %d < k = %d", d->ld_ids, d->k);
  NR_CHECK_ARG(d->ld_base >= d->n_groups + 1, "row_logprob_capped: base row stride %d < n_groups + 1 = %d", d->ld_base, d->n_groups + 1);
  NR_DEVICE_GUARD(stream, d->news_vecs);
  hipStream_t s = (hipStream_t)stream;
  LogpcArgs a;
  a.news = d->news_vecs; a.user = d->user; a.ids = d->row_ids; a.group = d->group;
  a.ld_news = (size_t)d->ld_news; a.ld_user = (size_t)d->ld_user; a.ld_ids = (size_t)d->ld_ids; a.ld_base = (size_t)d->ld_base;
  a.V = d->V; a.U = d->U; a.N = d->N; a.k = d->k; a.cap = d->group_cap; a.G = d->n_groups;
  a.pool = pool_args(d->prior, d->stamp, d->window, d->ld_window);
  a.tau = d->tau; a.tau_u = d->tau_u;
  a.base_max = d->base_max; a.base_logsum = d->base_logsum;
  a.out_logp = d->out_logp; a.out_total = d->out_total;
  NrProfScope ps(s, "logp_capped[U=%d,N=%d,k=%d,cap=%d,G=%d]", d->U, d->N, d->k, d->group_cap, d->n_groups);
  const size_t smem = tk_tile_bytes(16, d->N) + (size_t)2 * 16 * TK_ROWS * sizeof(int32_t);
  NR_CHECK_RC(with_bool(a.pool.any(), [&](auto p) {
    return launch_lds(logp_capped_kernel<decltype(p)::value>, dim3((unsigned)((d->U + 15) / 16)), dim3(TK_THREADS), smem, s, a);
  }));
  NR_CHECK_LAUNCH();
  return NR_OK;
}

int nr_row_logprob_capped_grad(const nr_logprob_capped_grad_desc* d, nr_stream_t stream) {
  NR_CHECK_ARG(d != nullptr, "row_logprob_capped_grad: null descriptor");
  NR_CHECK_ARG(d->k >= 1 && d->k <= NR_TOPK_MAX_K, "row_logprob_capped_grad: k = %d entries per row, must be in [1, %d]", d->k, NR_TOPK_MAX_K);
  NR_CHECK_RC(check_vectors("row_logprob_capped_grad", d->V, d->U, d->N));
  NR_CHECK_ARG(d->tau_u != nullptr || (d->tau > 0.f && d->tau < LG_INF),
               "row_logprob_capped_grad: tau = %g, a scalar temperature must be finite and > 0", (double)d->tau);
  NR_CHECK_ARG(d->group_cap >= 1 && d->group_cap <= 128, "row_logprob_capped_grad: group_cap = %d, must be in [1, 128]", d->group_cap);
  NR_CHECK_ARG(d->n_groups >= 1 && d->n_groups <= NR_RANK_MAX_GROUPS, "row_logprob_capped_grad: n_groups = %d, must be in [1, %d]", d->n_groups,
               NR_RANK_MAX_GROUPS);
  NR_CHECK_RC(check_pools("row_logprob_capped_grad", d->stamp, d->window, d->ld_window));
  NR_CHECK_ARG(d->news_vecs && d->user && d->row_ids && d->group && d->base_max && d->base_logsum && d->out_bin_w && d->out_sub_w,
               "row_logprob_capped_grad: null pointer (news_vecs, user, row_ids, group, base_max, base_logsum, out_bin_w, out_sub_w)");
  NR_CHECK_RC(check_rows("row_logprob_capped_grad", d->news_vecs, d->ld_news, d->user, d->ld_user, d->N));
  NR_CHECK_ARG(d->ld_ids >= d->k, "row_logprob_capped_grad: id row stride %d < k = %d", d->ld_ids, d->k);
  NR_CHECK_ARG(d->ld_base >= d->n_groups + 1, "row_logprob_capped_grad: base row stride %d < n_groups + 1 = %d", d->ld_base, d->n_groups + 1);
  NR_CHECK_ARG(d->g == nullptr || d->ld_g >= d->k, "row_logprob_capped_grad: g row stride %d < k = %d", d->ld_g, d->k);
  NR_DEVICE_GUARD(stream, d->news_vecs);
  hipStream_t s = (hipStream_t)stream;
  LogpcGradArgs a;
  a.news = d->news_vecs; a.user = d->user; a.ids = d->row_ids; a.group = d->group;
  a.ld_news = (size_t)d->ld_news; a.ld_user = (size_t)d->ld_user; a.ld_ids = (size_t)d->ld_ids; a.ld_base = (size_t)d->ld_base;
  a.ld_g = (size_t)d->ld_g;
  a.V = d->V; a.U = d->U; a.N = d->N; a.k = d->k; a.cap = d->group_cap; a.G = d->n_groups;
  a.pool = pool_args(d->prior, d->stamp, d->window, d->ld_window);
  a.tau = d->tau; a.tau_u = d->tau_u;
  a.base_max = d->base_max; a.base_logsum = d->base_logsum;
  a.g = d->g; a.out_bin_w = d->out_bin_w; a.out_sub_w = d->out_sub_w;
  NrProfScope ps(s, "logp_capped_grad[U=%d,N=%d,k=%d,cap=%d,G=%d]", d->U, d->N, d->k, d->group_cap, d->n_groups);
  const size_t smem = tk_tile_bytes(16, d->N) + (size_t)2 * 16 * TK_ROWS * sizeof(int32_t);
  NR_CHECK_RC(with_bool(a.pool.any(), [&](auto p) {
    return launch_lds(logp_capped_grad_kernel<decltype(p)::value>, dim3((unsigned)((d->U + 15) / 16)), dim3(TK_THREADS), smem, s, a);
  }));
  NR_CHECK_LAUNCH();
  return NR_OK;
}

}  // extern "C"
