// The entropy of the served distribution and its gradient (include/nrhip.h, K23 and K24).  With K13's base (max, logsum) the
// device forms x_v = fmaf(s_v - max, 1 / tau, -logsum) = log p_v <= 0 and p_v = expf(x_v) exactly as nr_expect.hip does, so the
// centred log-probability is free, and three moments of log p under p give everything:
//   m0 = sum p,  m1 = sum p x,  m2 = sum p x^2:   H = -m1,  Var_p(log p) = m2 - m1^2,  dH / dtau = (m2 - m1^2) / tau,
//   dH / duser = -(J + H E) / tau,  E = sum p news_v (K17),  J = sum p x news_v.
// A pair with p == 0 is a term of no sum (0 log 0 = 0; 0 * -inf is never formed).  Scores and eligibility come from score_key /
// pool_key and the list cursor of nr_logz_stream.h: a news is a term here exactly when it is a term of nr_score_logz's sum.
//
//   entropy_stream_kernel<MT, POOL, LISTS>   the grid, segments, slices, user tile and LDS budget of logz_stream_kernel.  The base
//                           is known, so there is no running maximum: per pair x, p and three per-lane fp64 chains sum p,
//                           sum p x, sum (p x) x over the lane's news of the SLICE, the products formed in fp64 from the fp32 p
//                           and x.  At the slice end an xor butterfly per chain and ONE triple per (user, slice).
//   entropy_final_kernel    a wave per user: the slices ascending in fp64; H = -m1, var = m2 - m1^2 (fp64), mass = m0, each rounded
//                           to fp32 once.
//   affine_stream_kernel<MT, KMAX, POOL, LISTS>   expect_stream_kernel of nr_expect.hip, statement for statement, but for the value
//                           stored to the P tile: p == 0 ? 0 : p * fmaf(beta_u, x, alpha_u).  The fp64 running mass stays sum p.
//   affine_final_kernel     expect_final_kernel without the weight multiply.
//
// The plan, the carve and ex_clean are copies of nr_expect.hip's (its anonymous namespace is not shared; the kernels of that unit
// keep their instruction streams).  The chains are K17's: chunk starts are fixed by V, slices by (V, splits), users of a tile are
// rows of A or lanes' own registers -- no user's bits depend on another's.
#include <math.h>

#include "nr_logz_stream.h"

namespace {

// ---- K23 ----------------------------------------------------------------------------------------------------------------

inline LogzPlan en_plan(int U, int V, int N, int splits) { return lz_plan_tile(U, V, score_user_tile(N, 0), splits); }

struct EntropyArgs {
  const float* news;
  const float* user;
  size_t ld_news, ld_user;
  int V, U, N, seg, nseg, segs_per, splits;
  PoolArgs pool;            // read by the POOL instantiations only
  float tau;                // used when tau_u is null
  const float* tau_u;       // [U] or null
  const float* base_max;    // [U]
  const float* base_logsum; // [U]
  double* pm;               // [U, splits, 3] partial (sum p, sum p x, sum p x^2)
  __device__ __forceinline__ float tau_of(long u) const { return tau_u != nullptr ? tau_u[u] : tau; }
};
inline size_t en_carve(void* ws, int U, int splits, EntropyArgs* a) {
  if (a) a->pm = reinterpret_cast<double*>(ws);
  return (size_t)U * splits * 3 * sizeof(double);
}

// one pair into the lane's three chains; p == 0 (not eligible, or expf underflowed, or x = -inf) is a term of no sum
__device__ __forceinline__ void en_take(float p, float x, double& m0, double& m1, double& m2) {
  if (p > 0.f) {
    const double dp = (double)p, dx = (double)x;
    const double px = dp * dx;
    m0 += dp;
    m1 += px;
    m2 += px * dx;
  }
}

template <int MT, bool POOL, bool LISTS>
__global__ __launch_bounds__(TK_THREADS) void entropy_stream_kernel(EntropyArgs a, CsrArgs ca) {
  constexpr int TU = 16 * MT, PER_WAVE = TU / TK_WAVES;
  extern __shared__ __attribute__((aligned(16))) float en_smem[];
  ScoreTile<MT> t(en_smem, a.N);
  const int lane = t.lane, wave = t.wave;
  const int u0 = blockIdx.x * TU;
  const int s_lo = (int)blockIdx.y * a.segs_per;
  const int s_hi = s_lo + a.segs_per < a.nseg ? s_lo + a.segs_per : a.nseg;
  const long v_lo = 1 + (long)s_lo * a.seg;
  const long v_hi = 1 + (long)s_hi * a.seg < a.V ? 1 + (long)s_hi * a.seg : a.V;
  if (v_lo >= v_hi) return;                                   // the whole workgroup (en_plan leaves no empty slice)

  t.load_users(a.user, a.ld_user, u0, a.U);
  // user wave + 8 i of the tile: 1 / tau, the base, whether the user has terms at all, and this lane's three chains of the slice
  float it[PER_WAVE], bm[PER_WAVE], nbl[PER_WAVE];
  bool live[PER_WAVE];
  double m0[PER_WAVE], m1[PER_WAVE], m2[PER_WAVE];
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int u = u0 + wave + TK_WAVES * i;
    const float tau = u < a.U ? a.tau_of(u) : 1.f;
    it[i] = __fdiv_rn(1.f, tau);
    bm[i] = u < a.U ? a.base_max[u] : -LZ_INF;
    nbl[i] = u < a.U ? -a.base_logsum[u] : 0.f;
    // no terms for a user beyond U, one the finalize answers with NaN (bad tau, NaN base), or one with nothing eligible
    live[i] = u < a.U && tau > 0.f && tau < LZ_INF && fabsf(bm[i]) < LZ_INF && nbl[i] == nbl[i];
    m0[i] = m1[i] = m2[i] = 0.0;
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
      // eligible as in logz_stream_kernel: a row of the slice, key != 0 (not NaN, inside the pool), not listed
      const bool el0 = live[i] && lane < nvalid && k0 != 0u && ((l0 >> lane) & 1ull) == 0ull;
      const bool el1 = live[i] && lane + 64 < nvalid && k1 != 0u && ((l1 >> lane) & 1ull) == 0ull;
      // x = fmaf(s - max, 1 / tau, -logsum), p = expf(x): K17's; s == max: x = -logsum, never 0 * inf where 1 / tau overflowed
      const float d0 = key_score(k0) - bm[i], d1 = key_score(k1) - bm[i];
      const float x0 = d0 == 0.f ? nbl[i] : fmaf(d0, it[i], nbl[i]), x1 = d1 == 0.f ? nbl[i] : fmaf(d1, it[i], nbl[i]);
      en_take(el0 ? expf(x0) : 0.f, x0, m0[i], m1[i], m2[i]);
      en_take(el1 ? expf(x1) : 0.f, x1, m0[i], m1[i], m2[i]);
    }
    __syncthreads();                                          // the score tile is the next chunk's staging buffer
  }

  // slice end: one triple per (user, slice), the lanes added by the xor butterfly
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int u = u0 + wave + TK_WAVES * i;
    const double r0 = wave_sum_d(m0[i]), r1 = wave_sum_d(m1[i]), r2 = wave_sum_d(m2[i]);
    if (lane == 0 && u < a.U) {
      double* o = a.pm + ((size_t)u * a.splits + blockIdx.y) * 3;
      o[0] = r0;
      o[1] = r1;
      o[2] = r2;
    }
  }
}

// fp64 readlane: the value lane l holds, as a scalar (l is wave-uniform)
__device__ __forceinline__ double en_readlane_d(double v, int l) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// One wave per user; lane l loads the triples of slices l, l + 64, l + 128, l + 192 (slices <= nseg <= 256), all in flight at once,
// and the wave then adds them in ASCENDING slice order, each partial read back from its lane as a scalar: the chain of a serial
// loop without its chain of dependent loads (a thread per user took 37 % of the call at U = 64, 196 slices).
__global__ __launch_bounds__(256) void entropy_final_kernel(EntropyArgs a, float* __restrict__ out_entropy, float* __restrict__ out_var,
                                                            float* __restrict__ out_mass) {
  static_assert(LZ_MAX_SEGS == 4 * 64, "four partials per lane");
  const int lane = threadIdx.x & 63;
  const size_t u = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= (size_t)a.U) return;                               // the whole wave
  double p0[4], p1[4], p2[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = lane + 64 * q;
    p0[q] = p1[q] = p2[q] = 0.0;
    if (j < a.splits) {
      const double* p = a.pm + (u * a.splits + j) * 3;
      p0[q] = p[0];
      p1[q] = p[1];
      p2[q] = p[2];
    }
  }
  double m0 = 0.0, m1 = 0.0, m2 = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int cnt = a.splits - 64 * q < 64 ? a.splits - 64 * q : 64;
    for (int j = 0; j < cnt; ++j) {
      m0 += en_readlane_d(p0[q], j);
      m1 += en_readlane_d(p1[q], j);
      m2 += en_readlane_d(p2[q], j);
    }
  }
  if (lane != 0) return;
  const float tau = a.tau_of(u);
  const float bmax = a.base_max[u], bls = a.base_logsum[u];
  // nothing eligible (K13: max -inf, whatever tau is): zeros -- the stream formed no term.  Else a bad tau or a NaN base: NaN
  const bool bad = bmax != -LZ_INF && (!(tau > 0.f && tau < LZ_INF) || bmax != bmax || bls != bls);
  const float NaN = __builtin_nanf("");
  out_entropy[u] = bad ? NaN : (float)(0.0 - m1);
  if (out_var != nullptr) out_var[u] = bad ? NaN : (float)(m2 - m1 * m1);
  if (out_mass != nullptr) out_mass[u] = bad ? NaN : (float)m0;
}

// argument checks shared by the size query and the call; 0 = fine
int entropy_check(const nr_entropy_desc* d) {
  NR_CHECK_ARG(d != nullptr, "score_entropy: null descriptor");
  NR_CHECK_RC(check_vectors("score_entropy", d->V, d->U, d->N));
  NR_CHECK_RC(check_lists("score_entropy", 0, d->excl_offsets, d->excl_ids, d->n_excl));   // this call has no dense list
  NR_CHECK_ARG(d->tau_u != nullptr || (d->tau > 0.f && d->tau < LZ_INF), "score_entropy: tau = %g, a scalar temperature must be finite and > 0",
               (double)d->tau);
  const int nseg = en_plan(d->U, d->V, d->N, 1).nseg;
  NR_CHECK_ARG(d->splits >= 0 && d->splits <= nseg, "score_entropy: splits = %d, must be 0 (library's choice) or in [1, %d], the segments of V = %d",
               d->splits, nseg, d->V);
  return check_pools("score_entropy", d->stamp, d->window, d->ld_window);
}

int entropy_stream_launch(int TU, bool pool, bool lists, dim3 grid, size_t smem, hipStream_t s, const EntropyArgs& a, const CsrArgs& ca) {
  return with_int<64, 32, 16>(TU, [&](auto tu) {
    return with_bool(pool, [&](auto p) {
      return with_bool(lists, [&](auto l) {
        return launch_lds(entropy_stream_kernel<decltype(tu)::value / 16, decltype(p)::value, decltype(l)::value>, grid, dim3(TK_THREADS), smem, s, a, ca);
      });
    });
  });
}

// ---- K24 ----------------------------------------------------------------------------------------------------------------

struct AffineArgs {
  const float* news;
  const float* user;
  size_t ld_news, ld_user;
  int V, U, N, seg, nseg, segs_per, splits;
  PoolArgs pool;            // read by the POOL instantiations only
  float tau;                // used when tau_u is null
  const float* tau_u;       // [U] or null
  const float* base_max;    // [U]
  const float* base_logsum; // [U]
  const float* alpha;       // [U] or null = 1
  const float* beta;        // [U] or null = 0
  float* part;              // [U, splits, N] partial rows
  double* pmass;            // [U, splits] partial masses
  __device__ __forceinline__ float tau_of(long u) const { return tau_u != nullptr ? tau_u[u] : tau; }
};
// workspace: the masses first (8-byte aligned), then the partial rows
inline size_t af_carve(void* ws, int U, int splits, int N, AffineArgs* a) {
  char* p = reinterpret_cast<char*>(ws);
  const size_t n = (size_t)U * splits;
  if (a) {
    a->pmass = reinterpret_cast<double*>(p);
    a->part = reinterpret_cast<float*>(p + n * 8);
  }
  return (n * 8 + n * (size_t)N * 4 + 7) & ~(size_t)7;
}

constexpr size_t AF_PER_USER = TK_LDS_TILE * sizeof(float);   // a user's row of P
// K17's user tile (a function of N alone): 64 users up to 11 slabs, 32 up to 26, else 16
inline int af_user_tile(int N) { return score_user_tile(N, AF_PER_USER); }
inline LogzPlan af_plan(int U, int V, int N, int splits) { return lz_plan_tile(U, V, af_user_tile(N), splits); }

// a component that is not finite counts as 0: its row has weight 0 for every user, and 0 * NaN would reach every user of the tile
__device__ __forceinline__ void af_clean(f32x4& g) {
#pragma unroll
  for (int e = 0; e < 4; ++e) g[e] = fabsf(g[e]) < LZ_INF ? g[e] : 0.f;
}

template <int MT, int KMAX, bool POOL, bool LISTS>
__global__ __launch_bounds__(TK_THREADS) void affine_stream_kernel(AffineArgs a, CsrArgs ca) {
  constexpr int TU = 16 * MT, PER_WAVE = TU / TK_WAVES;
  constexpr int PAIRS = 2 * MT, PARTS = TK_WAVES / PAIRS, PART_ROWS = TK_ROWS / PARTS, STEPS = PART_ROWS / 16;
  static_assert(PAIRS * PARTS == TK_WAVES && STEPS >= 1, "8 waves = pairs x row parts");
  extern __shared__ __attribute__((aligned(16))) float af_smem[];
  ScoreTile<MT> t(af_smem, a.N);
  float* sP = t.end();                                        // [TU, TK_LDS_TILE] the chunk's weights
  const int lane = t.lane, wave = t.wave;
  const int u0 = blockIdx.x * TU;
  const int s_lo = (int)blockIdx.y * a.segs_per;
  const int s_hi = s_lo + a.segs_per < a.nseg ? s_lo + a.segs_per : a.nseg;
  const long v_lo = 1 + (long)s_lo * a.seg;
  const long v_hi = 1 + (long)s_hi * a.seg < a.V ? 1 + (long)s_hi * a.seg : a.V;
  if (v_lo >= v_hi) return;                                   // the whole workgroup (af_plan leaves no empty slice)
  const int ksteps = t.ksteps;                                // <= KMAX by the launch's choice of instantiation

  t.load_users(a.user, a.ld_user, u0, a.U);
  // user wave + 8 i of the tile: 1 / tau, the base, whether the user gets weights at all, this lane's running mass
  float it[PER_WAVE], bm[PER_WAVE], nbl[PER_WAVE];
  bool live[PER_WAVE];
  double mass[PER_WAVE];
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int u = u0 + wave + TK_WAVES * i;
    const float tau = u < a.U ? a.tau_of(u) : 1.f;
    it[i] = __fdiv_rn(1.f, tau);
    bm[i] = u < a.U ? a.base_max[u] : -LZ_INF;
    nbl[i] = u < a.U ? -a.base_logsum[u] : 0.f;
    live[i] = u < a.U && tau > 0.f && tau < LZ_INF && fabsf(bm[i]) < LZ_INF && nbl[i] == nbl[i];
    mass[i] = 0.0;
  }
  // lane i keeps (alpha, beta) of this wave's i-th user -- two registers for the tile, read back as scalars; (1, 0) beyond U
  float al_l = 1.f, be_l = 0.f;
  {
    const int u = u0 + wave + TK_WAVES * lane;
    if (lane < PER_WAVE && u < a.U) {
      if (a.alpha != nullptr) al_l = a.alpha[u];
      if (a.beta != nullptr) be_l = a.beta[u];
    }
  }
  int32_t cur[PER_WAVE], end[PER_WAVE];
  if constexpr (LISTS) LZ_SEEK(ca, u0, wave, lane, a.U, v_lo, cur, end)
  int32_t w_lo = 1, w_hi = 0;
  if constexpr (POOL) {
    const int u = u0 + wave + TK_WAVES * lane;
    if (lane < PER_WAVE && u < a.U) {
      w_lo = a.pool.lo_of(u);
      w_hi = a.pool.hi_of(u);
    }
  }

  // the second contraction: this wave's (user tile, column tile) pair and its part of the chunk's rows
  const int pair = wave % PAIRS, part = wave / PAIRS;
  const int ti = pair >> 1, tj = pair & 1, rbase = part * PART_ROWS;
  const int frow = lane & 15, fg = lane >> 4;
  f32x4 out[KMAX];
#pragma unroll
  for (int ks = 0; ks < KMAX; ++ks) out[ks] = (f32x4){0.f, 0.f, 0.f, 0.f};

  ScoreStreamRows rows = {a.news, a.ld_news, v_lo, v_hi};
  t.load_slab(rows, 0);
  for (long vc = v_lo; vc < v_hi; vc += TK_ROWS) {
    f32x4 acc[MT];
    rows.vc = vc;
    t.chunk(rows, acc);
    t.load_slab(rows, 0);                                     // the same chunk again: in flight while the weights are formed
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
      const bool el0 = live[i] && lane < nvalid && k0 != 0u && ((l0 >> lane) & 1ull) == 0ull;
      const bool el1 = live[i] && lane + 64 < nvalid && k1 != 0u && ((l1 >> lane) & 1ull) == 0ull;
      // x = log p = fmaf(s - max, 1 / tau, -logsum), p = expf(x): K17's; the pair's weight is p (beta x + alpha), 0 where p == 0
      const float d0 = key_score(k0) - bm[i], d1 = key_score(k1) - bm[i];
      const float x0 = d0 == 0.f ? nbl[i] : fmaf(d0, it[i], nbl[i]), x1 = d1 == 0.f ? nbl[i] : fmaf(d1, it[i], nbl[i]);
      const float w0 = el0 ? expf(x0) : 0.f;
      const float w1 = el1 ? expf(x1) : 0.f;
      const float al = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(al_l), i));
      const float be = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(be_l), i));
      sP[ul * TK_LDS_TILE + lane] = w0 == 0.f ? 0.f : w0 * fmaf(be, x0, al);
      sP[ul * TK_LDS_TILE + lane + 64] = w1 == 0.f ? 0.f : w1 * fmaf(be, x1, al);
      mass[i] += (double)w0 + (double)w1;
    }
    __syncthreads();                                          // P is whole; the score tile is the staging buffer again

    // the wave's fragment of P: pa[s][e] = weight of user ti * 16 + frow for chunk row rbase + 16 s + 4 fg + e
    f32x4 pa[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) pa[s] = *reinterpret_cast<const f32x4*>(sP + (ti * 16 + frow) * TK_LDS_TILE + rbase + 16 * s + 4 * fg);
    af_clean(t.g0);
    af_clean(t.g1);
    t.store_slab(0);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < KMAX; ++ks) {
      if (ks < ksteps) {
        if (ks + 1 < ksteps) t.load_slab(rows, ks + 1);
        else if (vc + TK_ROWS < v_hi) {                       // the next chunk's first slab, for ScoreTile::chunk
          rows.vc = vc + TK_ROWS;
          t.load_slab(rows, 0);
        }
        // B[k = fg][n = frow] = slab row rbase + 16 s + 4 fg + e, column tj * 16 + frow: the 64 lanes read 64 different banks
        const float* pb = t.sB + (size_t)(ks & 1) * TK_ROWS * TK_LDB + (rbase + 4 * fg) * TK_LDB + tj * 16 + frow;
#pragma unroll
        for (int s = 0; s < STEPS; ++s)
#pragma unroll
          for (int e = 0; e < 4; ++e) out[ks] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[s][e], pb[(16 * s + e) * TK_LDB], out[ks], 0, 0, 0);
        if (ks + 1 < ksteps) {
          af_clean(t.g0);
          af_clean(t.g1);
          t.store_slab((ks + 1) & 1);
        }
        __syncthreads();
      }
    }
  }

  // slice end.  The mass: one partial per (user, slice)
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int u = u0 + wave + TK_WAVES * i;
    const double m = wave_sum_d(mass[i]);
    if (lane == 0 && u < a.U) a.pmass[(size_t)u * a.splits + blockIdx.y] = m;
  }
  // The rows: out[ks][r] belongs to user ti * 16 + 4 fg + r, column ks * 32 + tj * 16 + frow.  The row parts are added in
  // ascending order, ((part 0 + part 1) + part 2) + part 3, through the user vectors' LDS (the slice is over; [TU, ldu] >= [TU, npad])
  float* sO = t.sU;
  for (int q = 1; q < PARTS; ++q) {
    if (part == q) {
#pragma unroll
      for (int ks = 0; ks < KMAX; ++ks)
        if (ks < ksteps)
#pragma unroll
          for (int r = 0; r < 4; ++r) sO[(size_t)(ti * 16 + 4 * fg + r) * t.ldu + ks * TK_KS + tj * 16 + frow] = out[ks][r];
    }
    __syncthreads();
    if (part == 0) {
#pragma unroll
      for (int ks = 0; ks < KMAX; ++ks)
        if (ks < ksteps)
#pragma unroll
          for (int r = 0; r < 4; ++r) out[ks][r] += sO[(size_t)(ti * 16 + 4 * fg + r) * t.ldu + ks * TK_KS + tj * 16 + frow];
    }
    __syncthreads();
  }
  if (part == 0) {
#pragma unroll
    for (int ks = 0; ks < KMAX; ++ks)
      if (ks < ksteps) {
        const int c = ks * TK_KS + tj * 16 + frow;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int u = u0 + ti * 16 + 4 * fg + r;
          if (u < a.U && c < a.N) a.part[((size_t)u * a.splits + blockIdx.y) * a.N + c] = out[ks][r];
        }
      }
  }
}

struct AffineFinalArgs {
  const int32_t* sub_ids;   // [U, ld_sub] or null
  const float* sub_w;
  size_t ld_sub, ld_out;
  int T, scale_inv_tau;
  float* out;
  float* out_mass;          // [U] or null
};

// One workgroup per user, a thread per component (strided).
__global__ __launch_bounds__(256) void affine_final_kernel(AffineArgs a, AffineFinalArgs f) {
  const size_t u = blockIdx.x;
  const float tau = a.tau_of(u);
  const float bmax = a.base_max[u], bls = a.base_logsum[u];
  // nothing eligible (K13: max -inf, whatever tau is): the stream formed no weight.  Else a bad tau or a NaN base: NaN
  const bool bad = bmax != -LZ_INF && (!(tau > 0.f && tau < LZ_INF) || bmax != bmax || bls != bls);
  const double it = f.scale_inv_tau ? (double)__fdiv_rn(1.f, tau) : 1.0;
  for (int c = threadIdx.x; c < a.N; c += blockDim.x) {
    double e = 0.0;
    for (int s = 0; s < a.splits; ++s) e += (double)a.part[(u * a.splits + s) * a.N + c];
    if (f.sub_ids != nullptr)
      for (int j = 0; j < f.T; ++j) {
        const int32_t id = f.sub_ids[u * f.ld_sub + j];
        if (id >= 1 && id < a.V) e -= (double)f.sub_w[u * f.ld_sub + j] * (double)a.news[(size_t)id * a.ld_news + c];
      }
    f.out[u * f.ld_out + c] = bad ? __builtin_nanf("") : (float)(e * it);
  }
  if (threadIdx.x == 0 && f.out_mass != nullptr) {
    double m = 0.0;
    for (int s = 0; s < a.splits; ++s) m += a.pmass[u * a.splits + s];
    f.out_mass[u] = bad ? __builtin_nanf("") : (float)m;
  }
}

int affine_check(const nr_expect_affine_desc* d) {
  NR_CHECK_ARG(d != nullptr, "score_expect_affine: null descriptor");
  NR_CHECK_RC(check_vectors("score_expect_affine", d->V, d->U, d->N));
  NR_CHECK_RC(check_lists("score_expect_affine", 0, d->excl_offsets, d->excl_ids, d->n_excl));   // this call has no dense list
  NR_CHECK_ARG(d->tau_u != nullptr || (d->tau > 0.f && d->tau < LZ_INF),
               "score_expect_affine: tau = %g, a scalar temperature must be finite and > 0", (double)d->tau);
  const int nseg = af_plan(d->U, d->V, d->N, 1).nseg;
  NR_CHECK_ARG(d->splits >= 0 && d->splits <= nseg,
               "score_expect_affine: splits = %d, must be 0 (library's choice) or in [1, %d], the segments of V = %d", d->splits, nseg, d->V);
  return check_pools("score_expect_affine", d->stamp, d->window, d->ld_window);
}

// the stream's instantiation for the run-time (tile, pool, lists); the tile fixes the k-slabs that can occur with it
int affine_stream_launch(int TU, bool pool, bool lists, dim3 grid, size_t smem, hipStream_t s, const AffineArgs& a, const CsrArgs& ca) {
  return with_bool(pool, [&](auto p) {
    return with_bool(lists, [&](auto l) {
      constexpr bool P = decltype(p)::value, L = decltype(l)::value;
      if (TU == 64) return launch_lds(affine_stream_kernel<4, 11, P, L>, grid, dim3(TK_THREADS), smem, s, a, ca);
      if (TU == 32) return launch_lds(affine_stream_kernel<2, 26, P, L>, grid, dim3(TK_THREADS), smem, s, a, ca);
      return launch_lds(affine_stream_kernel<1, NR_TOPK_MAX_N / TK_KS, P, L>, grid, dim3(TK_THREADS), smem, s, a, ca);
    });
  });
}

}  // namespace

extern "C" {

size_t nr_score_entropy_workspace_bytes(const nr_entropy_desc* d) {
  if (entropy_check(d) != NR_OK) return 0;
  return en_carve(nullptr, d->U, en_plan(d->U, d->V, d->N, d->splits).splits, nullptr);
}

int nr_score_entropy(const nr_entropy_desc* d, nr_stream_t stream) {
  NR_CHECK_RC(entropy_check(d));
  NR_CHECK_ARG(d->news_vecs && d->user && d->base_max && d->base_logsum && d->out_entropy,
               "score_entropy: null pointer (news_vecs, user, base_max, base_logsum, out_entropy)");
  NR_CHECK_RC(check_rows("score_entropy", d->news_vecs, d->ld_news, d->user, d->ld_user, d->N));
  NR_CHECK_RC(check_workspace("score_entropy", d->ws, d->ws_bytes, nr_score_entropy_workspace_bytes(d)));
  NR_DEVICE_GUARD(stream, d->news_vecs);
  hipStream_t s = (hipStream_t)stream;
  const LogzPlan pl = en_plan(d->U, d->V, d->N, d->splits);
  EntropyArgs a;
  a.news = d->news_vecs; a.user = d->user;
  a.ld_news = (size_t)d->ld_news; a.ld_user = (size_t)d->ld_user;
  a.V = d->V; a.U = d->U; a.N = d->N; a.seg = pl.seg; a.nseg = pl.nseg; a.segs_per = pl.segs_per; a.splits = pl.splits;
  a.pool = pool_args(d->prior, d->stamp, d->window, d->ld_window);
  a.tau = d->tau; a.tau_u = d->tau_u;
  a.base_max = d->base_max; a.base_logsum = d->base_logsum;
  en_carve(d->ws, d->U, pl.splits, &a);
  const CsrArgs ca = csr_args(d->excl_offsets, d->excl_ids, d->n_excl);
  {
    const int TU = pl.TU;
    const size_t smem = tk_tile_bytes(TU, d->N);
    const dim3 grid((unsigned)((d->U + TU - 1) / TU), (unsigned)pl.splits);
    NrProfScope ps(s, "entropy_stream[U=%d,V=%d,N=%d,TU=%d,splits=%d,seg=%d]", d->U, d->V, d->N, TU, pl.splits, pl.seg);
    NR_CHECK_RC(entropy_stream_launch(TU, a.pool.any(), ca.offsets != nullptr, grid, smem, s, a, ca));
  }
  NR_CHECK_LAUNCH();
  {
    NrProfScope ps(s, "entropy_final[U=%d,splits=%d]", d->U, pl.splits);
    hipLaunchKernelGGL(entropy_final_kernel, dim3((unsigned)((d->U + 3) / 4)), dim3(256), 0, s, a, d->out_entropy, d->out_var, d->out_mass);
  }
  NR_CHECK_LAUNCH();
  return NR_OK;
}

size_t nr_score_expect_affine_workspace_bytes(const nr_expect_affine_desc* d) {
  if (affine_check(d) != NR_OK) return 0;
  return af_carve(nullptr, d->U, af_plan(d->U, d->V, d->N, d->splits).splits, d->N, nullptr);
}

int nr_score_expect_affine(const nr_expect_affine_desc* d, nr_stream_t stream) {
  NR_CHECK_RC(affine_check(d));
  NR_CHECK_ARG(d->news_vecs && d->user && d->base_max && d->base_logsum && d->out,
               "score_expect_affine: null pointer (news_vecs, user, base_max, base_logsum, out)");
  NR_CHECK_ARG(d->sub_ids == nullptr || d->sub_w != nullptr, "score_expect_affine: sub_ids given without sub_w (the two come together)");
  NR_CHECK_ARG(d->sub_w == nullptr || d->sub_ids != nullptr, "score_expect_affine: sub_w given without sub_ids (the two come together)");
  NR_CHECK_ARG(d->sub_ids == nullptr || (d->T >= 1 && d->T <= NR_TOPK_MAX_K && d->ld_sub >= d->T),
               "score_expect_affine: T = %d named rows per user (row stride %d), must be in [1, %d] with ld_sub >= T", d->T, d->ld_sub,
               NR_TOPK_MAX_K);
  NR_CHECK_RC(check_rows("score_expect_affine", d->news_vecs, d->ld_news, d->user, d->ld_user, d->N));
  NR_CHECK_ARG(d->ld_out >= d->N && (((uintptr_t)d->out) & 15) == 0, "score_expect_affine: out must be 16-byte aligned with ld_out = %d >= N = %d",
               d->ld_out, d->N);
  NR_CHECK_RC(check_workspace("score_expect_affine", d->ws, d->ws_bytes, nr_score_expect_affine_workspace_bytes(d)));
  NR_DEVICE_GUARD(stream, d->news_vecs);
  hipStream_t s = (hipStream_t)stream;
  const LogzPlan pl = af_plan(d->U, d->V, d->N, d->splits);
  AffineArgs a;
  a.news = d->news_vecs; a.user = d->user;
  a.ld_news = (size_t)d->ld_news; a.ld_user = (size_t)d->ld_user;
  a.V = d->V; a.U = d->U; a.N = d->N; a.seg = pl.seg; a.nseg = pl.nseg; a.segs_per = pl.segs_per; a.splits = pl.splits;
  a.pool = pool_args(d->prior, d->stamp, d->window, d->ld_window);
  a.tau = d->tau; a.tau_u = d->tau_u;
  a.base_max = d->base_max; a.base_logsum = d->base_logsum;
  a.alpha = d->alpha; a.beta = d->beta;
  af_carve(d->ws, d->U, pl.splits, d->N, &a);
  const CsrArgs ca = csr_args(d->excl_offsets, d->excl_ids, d->n_excl);
  {
    const int TU = pl.TU;
    const size_t smem = tk_tile_bytes(TU, d->N) + TU * AF_PER_USER;
    const dim3 grid((unsigned)((d->U + TU - 1) / TU), (unsigned)pl.splits);
    NrProfScope ps(s, "affine_stream[U=%d,V=%d,N=%d,TU=%d,splits=%d,seg=%d]", d->U, d->V, d->N, TU, pl.splits, pl.seg);
    NR_CHECK_RC(affine_stream_launch(TU, a.pool.any(), ca.offsets != nullptr, grid, smem, s, a, ca));
  }
  NR_CHECK_LAUNCH();
  {
    AffineFinalArgs f;
    f.sub_ids = d->sub_ids; f.sub_w = d->sub_w;
    f.ld_sub = (size_t)d->ld_sub; f.ld_out = (size_t)d->ld_out;
    f.T = d->sub_ids != nullptr ? d->T : 0; f.scale_inv_tau = d->scale_inv_tau;
    f.out = d->out; f.out_mass = d->out_mass;
    NrProfScope ps(s, "affine_final[U=%d,N=%d,splits=%d,T=%d]", d->U, d->N, pl.splits, f.T);
    hipLaunchKernelGGL(affine_final_kernel, dim3((unsigned)d->U), dim3(256), 0, s, a, f);
  }
  NR_CHECK_LAUNCH();
  return NR_OK;
}

}  // extern "C"
