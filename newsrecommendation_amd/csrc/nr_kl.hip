// The KL divergence of the served distribution to a reference policy and its gradient (include/nrhip.h, K26 and K27).  Two
// policies over the same news, lists and pools: p(. | u) from the user vectors at tau, q(. | u) from the REFERENCE user vectors at
// tau'.  With K13's base of each the device forms, per (user, news) pair,
//   x = log p = fmaf(s  - max , 1 / tau , -logsum ),   p = expf(x)        (K23's formation)
//   y = log q = fmaf(s' - max', 1 / tau', -logsum'),   s' = fl(<news_v, ref_u> + prior_v)
// and d = x - y in fp64 from the two fp32 values.  Four moments under p give everything:
//   m0 = sum p,  m1 = sum p x,  k1 = sum p d,  k2 = sum p d x:   KL = k1,  H = -m1,  Cov_p(d, x) = k2 - k1 m1,  dKL / dtau = -cov / tau,
//   dKL / duser = (1 / tau) sum p (d - KL) news_v = K27 with alpha = -KL, beta = 1, gamma = -1.
// A pair with p == 0 is a term of no sum (0 * +-inf is never formed).  Eligibility is the POLICY's: a news is a term here exactly
// when it is a term of nr_score_logz's sum for the policy's vectors.
//
// The user tile of ScoreTile<MT> holds HU = 8 MT policy users in its rows [0, HU) and their reference partners in rows
// [HU, 2 HU): one pass of the scoring tile gives both score rows, each (row, news) score the ONE fmaf chain every pass forms, so
// s' has the bits score_logz(news, ref, ...) sees.  A wave reads the two score rows of its users from the LDS score tile.
//
//   kl_stream_kernel<MT, POOL, LISTS>     entropy_stream_kernel of nr_entropy.hip with the second score row and four fp64 chains
//   kl_final_kernel                       entropy_final_kernel with four chains
//   expect_kl_stream_kernel<MT, KMAX, POOL, LISTS>   affine_stream_kernel of nr_entropy.hip with the second score row; the value
//                           stored to the P tile is p == 0 ? 0 : p * fmaf(gamma_u, y, fmaf(beta_u, x, alpha_u)).  The second
//                           contraction is K24's over MT / 2 user tiles of 16 (one, half of it padding, for MT = 1).
//   expect_kl_final_kernel  affine_final_kernel, the NaN rule widened by the reference side.
//
// The chains are K17's: chunk starts are fixed by V, slices by (V, splits), users of a tile are rows of A or lanes' own registers
// -- no user's bits depend on another's.
#include <math.h>

#include "nr_logz_stream.h"

namespace {

struct KlArgs {
  const float* news;
  const float* user;
  const float* ref;
  size_t ld_news, ld_user, ld_ref;
  int V, U, N, seg, nseg, segs_per, splits;
  PoolArgs pool;                // read by the POOL instantiations only
  float tau, ref_tau;           // used when tau_u / ref_tau_u is null
  const float* tau_u;           // [U] or null
  const float* ref_tau_u;       // [U] or null
  const float* base_max;        // [U]
  const float* base_logsum;     // [U]
  const float* ref_base_max;    // [U]
  const float* ref_base_logsum; // [U]
  const float* alpha;           // K27: [U] or null = 1
  const float* beta;            // K27: [U] or null = 0
  const float* gamma;           // K27: [U] or null = 0
  double* pm;                   // K26: [U, splits, 4] partial (sum p, sum p x, sum p d, sum p d x)
  float* part;                  // K27: [U, splits, N] partial rows
  double* pmass;                // K27: [U, splits] partial masses
  __device__ __forceinline__ float tau_of(long u) const { return tau_u != nullptr ? tau_u[u] : tau; }
  __device__ __forceinline__ float ref_tau_of(long u) const { return ref_tau_u != nullptr ? ref_tau_u[u] : ref_tau; }
};

// One side of a user: finite temperature > 0, a finite maximum, a logsum that is no NaN
__device__ __forceinline__ bool kl_side_ok(float tau, float bmax, float bls) {
  return tau > 0.f && tau < LZ_INF && fabsf(bmax) < LZ_INF && bls == bls;
}
// What the finalize kernels answer with NaN: the policy has something eligible (K13: max != -inf) and either side is not usable
// -- a bad tau or tau', a NaN in either base, a reference maximum that is not finite (-inf: the reference sees nothing eligible)
__device__ __forceinline__ bool kl_bad(const KlArgs& a, size_t u) {
  const float bmax = a.base_max[u];
  if (bmax == -LZ_INF) return false;
  const float tau = a.tau_of(u), bls = a.base_logsum[u];
  const bool pol = tau > 0.f && tau < LZ_INF && bmax == bmax && bls == bls;
  return !pol || !kl_side_ok(a.ref_tau_of(u), a.ref_base_max[u], a.ref_base_logsum[u]);
}

// The user tile: rows [0, HU) the policy users u0 .. u0 + HU - 1, rows [HU, 2 HU) their reference vectors; zero beyond N and U
template <int MT>
__device__ __forceinline__ void kl_load_users(ScoreTile<MT>& t, const KlArgs& a, int u0) {
  constexpr int HU = 8 * MT;
  const int q = t.npad / 4;
  for (int i = t.tid; i < 2 * HU * q; i += TK_THREADS) {
    const int r = i / q, c = (i - r * q) * 4;
    const int ul = r < HU ? r : r - HU;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (u0 + ul < a.U && c < a.N)
      v = r < HU ? *reinterpret_cast<const f32x4*>(a.user + (size_t)(u0 + ul) * a.ld_user + c)
                 : *reinterpret_cast<const f32x4*>(a.ref + (size_t)(u0 + ul) * a.ld_ref + c);
    *reinterpret_cast<f32x4*>(t.sU + (size_t)r * t.ldu + c) = v;
  }
}

// ---- K26 ----------------------------------------------------------------------------------------------------------------

// users per workgroup: half the rows of K23's tile
inline LogzPlan kl_plan(int U, int V, int N, int splits) { return lz_plan_tile(U, V, score_user_tile(N, 0) / 2, splits); }

inline size_t kl_carve(void* ws, int U, int splits, KlArgs* a) {
  if (a) a->pm = reinterpret_cast<double*>(ws);
  return (size_t)U * splits * 4 * sizeof(double);
}

// one pair into the lane's four chains; p == 0 (not eligible, or expf underflowed, or x = -inf) is a term of no sum
__device__ __forceinline__ void kl_take(float p, float x, float y, double& m0, double& m1, double& k1, double& k2) {
  if (p > 0.f) {
    const double dp = (double)p, dx = (double)x;
    const double pd = dp * (dx - (double)y);
    m0 += dp;
    m1 += dp * dx;
    k1 += pd;
    k2 += pd * dx;
  }
}

template <int MT, bool POOL, bool LISTS>
__global__ __launch_bounds__(TK_THREADS) void kl_stream_kernel(KlArgs a, CsrArgs ca) {
  constexpr int HU = 8 * MT, PER_WAVE = HU / TK_WAVES;
  extern __shared__ __attribute__((aligned(16))) float kl_smem[];
  ScoreTile<MT> t(kl_smem, a.N);
  const int lane = t.lane, wave = t.wave;
  const int u0 = blockIdx.x * HU;
  const int s_lo = (int)blockIdx.y * a.segs_per;
  const int s_hi = s_lo + a.segs_per < a.nseg ? s_lo + a.segs_per : a.nseg;
  const long v_lo = 1 + (long)s_lo * a.seg;
  const long v_hi = 1 + (long)s_hi * a.seg < a.V ? 1 + (long)s_hi * a.seg : a.V;
  if (v_lo >= v_hi) return;                                   // the whole workgroup (kl_plan leaves no empty slice)

  kl_load_users(t, a, u0);
  // user wave + 8 i of the tile: 1 / tau and the base of both sides, whether the user has terms at all, the four chains
  float it[PER_WAVE], bm[PER_WAVE], nbl[PER_WAVE], rit[PER_WAVE], rbm[PER_WAVE], rnbl[PER_WAVE];
  bool live[PER_WAVE];
  double m0[PER_WAVE], m1[PER_WAVE], k1[PER_WAVE], k2[PER_WAVE];
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int u = u0 + wave + TK_WAVES * i;
    const float tau = u < a.U ? a.tau_of(u) : 1.f, rtau = u < a.U ? a.ref_tau_of(u) : 1.f;
    it[i] = __fdiv_rn(1.f, tau);
    rit[i] = __fdiv_rn(1.f, rtau);
    bm[i] = u < a.U ? a.base_max[u] : -LZ_INF;
    nbl[i] = u < a.U ? -a.base_logsum[u] : 0.f;
    rbm[i] = u < a.U ? a.ref_base_max[u] : -LZ_INF;
    rnbl[i] = u < a.U ? -a.ref_base_logsum[u] : 0.f;
    // no terms for a user beyond U, one the finalize answers with NaN, or one with nothing eligible
    live[i] = u < a.U && kl_side_ok(tau, bm[i], nbl[i]) && kl_side_ok(rtau, rbm[i], rnbl[i]);
    m0[i] = m1[i] = k1[i] = k2[i] = 0.0;
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
      const int ul = wave + TK_WAVES * i, rl = HU + ul;
      u64 l0 = 0ull, l1 = 0ull;
      if constexpr (LISTS) LZ_LISTED(ca, e0[i], cur[i], end[i], vc, lane, l0, l1)
      uint32_t k0, k1_, r0, r1;
      if constexpr (POOL) {
        const int32_t lo = __builtin_amdgcn_readlane(w_lo, i), hi = __builtin_amdgcn_readlane(w_hi, i);
        k0 = pool_key(sS[ul * TK_LDS_TILE + lane], p0, s0, lo, hi);
        k1_ = pool_key(sS[ul * TK_LDS_TILE + lane + 64], p1, s1, lo, hi);
        r0 = pool_key(sS[rl * TK_LDS_TILE + lane], p0, s0, lo, hi);
        r1 = pool_key(sS[rl * TK_LDS_TILE + lane + 64], p1, s1, lo, hi);
      } else {
        k0 = score_key(sS[ul * TK_LDS_TILE + lane]);
        k1_ = score_key(sS[ul * TK_LDS_TILE + lane + 64]);
        r0 = score_key(sS[rl * TK_LDS_TILE + lane]);
        r1 = score_key(sS[rl * TK_LDS_TILE + lane + 64]);
      }
      // eligible as in logz_stream_kernel for the policy: a row of the slice, key != 0 (not NaN, inside the pool), not listed
      const bool el0 = live[i] && lane < nvalid && k0 != 0u && ((l0 >> lane) & 1ull) == 0ull;
      const bool el1 = live[i] && lane + 64 < nvalid && k1_ != 0u && ((l1 >> lane) & 1ull) == 0ull;
      // x = fmaf(s - max, 1 / tau, -logsum), p = expf(x): K17's; s == max: x = -logsum, never 0 * inf where 1 / tau overflowed.
      // y the same statement on the reference row (a reference score that is NaN has key 0, whose score reads NaN: y = NaN)
      const float d0 = key_score(k0) - bm[i], d1 = key_score(k1_) - bm[i];
      const float x0 = d0 == 0.f ? nbl[i] : fmaf(d0, it[i], nbl[i]), x1 = d1 == 0.f ? nbl[i] : fmaf(d1, it[i], nbl[i]);
      const float g0 = key_score(r0) - rbm[i], g1 = key_score(r1) - rbm[i];
      const float y0 = g0 == 0.f ? rnbl[i] : fmaf(g0, rit[i], rnbl[i]), y1 = g1 == 0.f ? rnbl[i] : fmaf(g1, rit[i], rnbl[i]);
      kl_take(el0 ? expf(x0) : 0.f, x0, y0, m0[i], m1[i], k1[i], k2[i]);
      kl_take(el1 ? expf(x1) : 0.f, x1, y1, m0[i], m1[i], k1[i], k2[i]);
    }
    __syncthreads();                                          // the score tile is the next chunk's staging buffer
  }

  // slice end: one quadruple per (user, slice), the lanes added by the xor butterfly
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int u = u0 + wave + TK_WAVES * i;
    const double q0 = wave_sum_d(m0[i]), q1 = wave_sum_d(m1[i]), q2 = wave_sum_d(k1[i]), q3 = wave_sum_d(k2[i]);
    if (lane == 0 && u < a.U) {
      double* o = a.pm + ((size_t)u * a.splits + blockIdx.y) * 4;
      o[0] = q0;
      o[1] = q1;
      o[2] = q2;
      o[3] = q3;
    }
  }
}

// fp64 readlane: the value lane l holds, as a scalar (l is wave-uniform)
__device__ __forceinline__ double kl_readlane_d(double v, int l) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// One wave per user; lane l loads the quadruples of slices l, l + 64, l + 128, l + 192 (slices <= nseg <= 256) and the wave adds
// them in ASCENDING slice order, each partial read back from its lane as a scalar (entropy_final_kernel's scheme).
__global__ __launch_bounds__(256) void kl_final_kernel(KlArgs a, float* __restrict__ out_kl, float* __restrict__ out_entropy,
                                                       float* __restrict__ out_cov, float* __restrict__ out_mass) {
  static_assert(LZ_MAX_SEGS == 4 * 64, "four partials per lane");
  const int lane = threadIdx.x & 63;
  const size_t u = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= (size_t)a.U) return;                               // the whole wave
  double p0[4], p1[4], p2[4], p3[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = lane + 64 * q;
    p0[q] = p1[q] = p2[q] = p3[q] = 0.0;
    if (j < a.splits) {
      const double* p = a.pm + (u * a.splits + j) * 4;
      p0[q] = p[0];
      p1[q] = p[1];
      p2[q] = p[2];
      p3[q] = p[3];
    }
  }
  double m0 = 0.0, m1 = 0.0, k1 = 0.0, k2 = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int cnt = a.splits - 64 * q < 64 ? a.splits - 64 * q : 64;
    for (int j = 0; j < cnt; ++j) {
      m0 += kl_readlane_d(p0[q], j);
      m1 += kl_readlane_d(p1[q], j);
      k1 += kl_readlane_d(p2[q], j);
      k2 += kl_readlane_d(p3[q], j);
    }
  }
  if (lane != 0) return;
  const bool bad = kl_bad(a, u);
  const float NaN = __builtin_nanf("");
  out_kl[u] = bad ? NaN : (float)k1;
  if (out_entropy != nullptr) out_entropy[u] = bad ? NaN : (float)(0.0 - m1);
  if (out_cov != nullptr) out_cov[u] = bad ? NaN : (float)(k2 - k1 * m1);
  if (out_mass != nullptr) out_mass[u] = bad ? NaN : (float)m0;
}

int kl_stream_launch(int TR, bool pool, bool lists, dim3 grid, size_t smem, hipStream_t s, const KlArgs& a, const CsrArgs& ca) {
  return with_int<64, 32, 16>(TR, [&](auto tr) {
    return with_bool(pool, [&](auto p) {
      return with_bool(lists, [&](auto l) {
        return launch_lds(kl_stream_kernel<decltype(tr)::value / 16, decltype(p)::value, decltype(l)::value>, grid, dim3(TK_THREADS), smem, s, a, ca);
      });
    });
  });
}

// ---- K27 ----------------------------------------------------------------------------------------------------------------

constexpr size_t XK_P_ROW = TK_LDS_TILE * sizeof(float);     // a user's row of P
inline int xk_p_rows(int TR) { return TR / 2 < 16 ? 16 : TR / 2; }
// score-tile rows by the k-slabs of N, each class inside the LDS and the register budget of its instantiation:
// 64 rows (32 users) up to 13 slabs, 32 rows (16 users) up to 26, else 16 rows (8 users)
constexpr int XK_KMAX_64 = 13, XK_KMAX_32 = 26, XK_KMAX_16 = NR_TOPK_MAX_N / TK_KS;
inline int xk_tile_rows(int N) {
  const int ks = tk_npad(N) / TK_KS;
  return ks <= XK_KMAX_64 ? 64 : ks <= XK_KMAX_32 ? 32 : 16;
}
inline size_t xk_smem(int TR, int N) { return tk_tile_bytes(TR, N) + xk_p_rows(TR) * XK_P_ROW; }
static_assert((size_t)64 * (XK_KMAX_64 * TK_KS + 4) * 4 + TK_STAGE_FLOATS * 4 + 32 * XK_P_ROW <= TK_LDS_MAX, "the 64-row class fits the LDS");
static_assert((size_t)32 * (XK_KMAX_32 * TK_KS + 4) * 4 + TK_STAGE_FLOATS * 4 + 16 * XK_P_ROW <= TK_LDS_MAX, "the 32-row class fits the LDS");
static_assert((size_t)16 * (XK_KMAX_16 * TK_KS + 4) * 4 + TK_STAGE_FLOATS * 4 + 16 * XK_P_ROW <= TK_LDS_MAX, "the 16-row class fits the LDS");
inline LogzPlan xk_plan(int U, int V, int N, int splits) { return lz_plan_tile(U, V, xk_tile_rows(N) / 2, splits); }

// workspace: the masses first (8-byte aligned), then the partial rows
inline size_t xk_carve(void* ws, int U, int splits, int N, KlArgs* a) {
  char* p = reinterpret_cast<char*>(ws);
  const size_t n = (size_t)U * splits;
  if (a) {
    a->pmass = reinterpret_cast<double*>(p);
    a->part = reinterpret_cast<float*>(p + n * 8);
  }
  return (n * 8 + n * (size_t)N * 4 + 7) & ~(size_t)7;
}

// a component that is not finite counts as 0: its row has weight 0 for every user, and 0 * NaN would reach every user of the tile
__device__ __forceinline__ void xk_clean(f32x4& g) {
#pragma unroll
  for (int e = 0; e < 4; ++e) g[e] = fabsf(g[e]) < LZ_INF ? g[e] : 0.f;
}

template <int MT, int KMAX, bool POOL, bool LISTS>
__global__ __launch_bounds__(TK_THREADS) void expect_kl_stream_kernel(KlArgs a, CsrArgs ca) {
  constexpr int HU = 8 * MT, PER_WAVE = HU / TK_WAVES;
  constexpr int MT2 = MT >= 2 ? MT / 2 : 1, PROWS = 16 * MT2;          // user tiles of the second contraction, rows of P
  constexpr int PAIRS = 2 * MT2, PARTS = TK_WAVES / PAIRS, PART_ROWS = TK_ROWS / PARTS, STEPS = PART_ROWS / 16;
  static_assert(PAIRS * PARTS == TK_WAVES && STEPS >= 1 && PROWS >= HU, "8 waves = pairs x row parts");
  extern __shared__ __attribute__((aligned(16))) float xk_smem_[];
  ScoreTile<MT> t(xk_smem_, a.N);
  float* sP = t.end();                                        // [PROWS, TK_LDS_TILE] the chunk's weights
  const int lane = t.lane, wave = t.wave;
  const int u0 = blockIdx.x * HU;
  const int s_lo = (int)blockIdx.y * a.segs_per;
  const int s_hi = s_lo + a.segs_per < a.nseg ? s_lo + a.segs_per : a.nseg;
  const long v_lo = 1 + (long)s_lo * a.seg;
  const long v_hi = 1 + (long)s_hi * a.seg < a.V ? 1 + (long)s_hi * a.seg : a.V;
  if (v_lo >= v_hi) return;                                   // the whole workgroup (xk_plan leaves no empty slice)
  const int ksteps = t.ksteps;                                // <= KMAX by the launch's choice of instantiation

  kl_load_users(t, a, u0);
  if constexpr (PROWS > HU)                                   // rows of P that belong to no user: zero for the whole slice
    for (int i = t.tid; i < (PROWS - HU) * TK_LDS_TILE; i += TK_THREADS) sP[HU * TK_LDS_TILE + i] = 0.f;
  float it[PER_WAVE], bm[PER_WAVE], nbl[PER_WAVE], rit[PER_WAVE], rbm[PER_WAVE], rnbl[PER_WAVE];
  bool live[PER_WAVE];
  double mass[PER_WAVE];
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int u = u0 + wave + TK_WAVES * i;
    const float tau = u < a.U ? a.tau_of(u) : 1.f, rtau = u < a.U ? a.ref_tau_of(u) : 1.f;
    it[i] = __fdiv_rn(1.f, tau);
    rit[i] = __fdiv_rn(1.f, rtau);
    bm[i] = u < a.U ? a.base_max[u] : -LZ_INF;
    nbl[i] = u < a.U ? -a.base_logsum[u] : 0.f;
    rbm[i] = u < a.U ? a.ref_base_max[u] : -LZ_INF;
    rnbl[i] = u < a.U ? -a.ref_base_logsum[u] : 0.f;
    live[i] = u < a.U && kl_side_ok(tau, bm[i], nbl[i]) && kl_side_ok(rtau, rbm[i], rnbl[i]);
    mass[i] = 0.0;
  }
  // lane i keeps (alpha, beta, gamma) of this wave's i-th user, read back as scalars; (1, 0, 0) beyond U
  float al_l = 1.f, be_l = 0.f, ga_l = 0.f;
  {
    const int u = u0 + wave + TK_WAVES * lane;
    if (lane < PER_WAVE && u < a.U) {
      if (a.alpha != nullptr) al_l = a.alpha[u];
      if (a.beta != nullptr) be_l = a.beta[u];
      if (a.gamma != nullptr) ga_l = a.gamma[u];
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
      const int ul = wave + TK_WAVES * i, rl = HU + ul;
      u64 l0 = 0ull, l1 = 0ull;
      if constexpr (LISTS) LZ_LISTED(ca, e0[i], cur[i], end[i], vc, lane, l0, l1)
      uint32_t k0, k1, r0, r1;
      if constexpr (POOL) {
        const int32_t lo = __builtin_amdgcn_readlane(w_lo, i), hi = __builtin_amdgcn_readlane(w_hi, i);
        k0 = pool_key(sS[ul * TK_LDS_TILE + lane], p0, s0, lo, hi);
        k1 = pool_key(sS[ul * TK_LDS_TILE + lane + 64], p1, s1, lo, hi);
        r0 = pool_key(sS[rl * TK_LDS_TILE + lane], p0, s0, lo, hi);
        r1 = pool_key(sS[rl * TK_LDS_TILE + lane + 64], p1, s1, lo, hi);
      } else {
        k0 = score_key(sS[ul * TK_LDS_TILE + lane]);
        k1 = score_key(sS[ul * TK_LDS_TILE + lane + 64]);
        r0 = score_key(sS[rl * TK_LDS_TILE + lane]);
        r1 = score_key(sS[rl * TK_LDS_TILE + lane + 64]);
      }
      const bool el0 = live[i] && lane < nvalid && k0 != 0u && ((l0 >> lane) & 1ull) == 0ull;
      const bool el1 = live[i] && lane + 64 < nvalid && k1 != 0u && ((l1 >> lane) & 1ull) == 0ull;
      // x, p: K17's; y: the same statement on the reference row; the pair's weight is p (gamma y + (beta x + alpha)), 0 where p == 0
      const float d0 = key_score(k0) - bm[i], d1 = key_score(k1) - bm[i];
      const float x0 = d0 == 0.f ? nbl[i] : fmaf(d0, it[i], nbl[i]), x1 = d1 == 0.f ? nbl[i] : fmaf(d1, it[i], nbl[i]);
      const float g0 = key_score(r0) - rbm[i], g1 = key_score(r1) - rbm[i];
      const float y0 = g0 == 0.f ? rnbl[i] : fmaf(g0, rit[i], rnbl[i]), y1 = g1 == 0.f ? rnbl[i] : fmaf(g1, rit[i], rnbl[i]);
      const float w0 = el0 ? expf(x0) : 0.f;
      const float w1 = el1 ? expf(x1) : 0.f;
      const float al = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(al_l), i));
      const float be = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(be_l), i));
      const float ga = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ga_l), i));
      sP[ul * TK_LDS_TILE + lane] = w0 == 0.f ? 0.f : w0 * fmaf(ga, y0, fmaf(be, x0, al));
      sP[ul * TK_LDS_TILE + lane + 64] = w1 == 0.f ? 0.f : w1 * fmaf(ga, y1, fmaf(be, x1, al));
      mass[i] += (double)w0 + (double)w1;
    }
    __syncthreads();                                          // P is whole; the score tile is the staging buffer again

    // the wave's fragment of P: pa[s][e] = weight of user ti * 16 + frow for chunk row rbase + 16 s + 4 fg + e
    f32x4 pa[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) pa[s] = *reinterpret_cast<const f32x4*>(sP + (ti * 16 + frow) * TK_LDS_TILE + rbase + 16 * s + 4 * fg);
    xk_clean(t.g0);
    xk_clean(t.g1);
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
          xk_clean(t.g0);
          xk_clean(t.g1);
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
  // The rows: out[ks][r] belongs to tile user ti * 16 + 4 fg + r, column ks * 32 + tj * 16 + frow.  The row parts are added in
  // ascending order through the user vectors' LDS (the slice is over; [2 HU, ldu] >= [PROWS, npad])
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
          const int ul = ti * 16 + 4 * fg + r;                // a row of P beyond HU is padding, not the next workgroup's user
          const int u = u0 + ul;
          if (ul < HU && u < a.U && c < a.N) a.part[((size_t)u * a.splits + blockIdx.y) * a.N + c] = out[ks][r];
        }
      }
  }
}

struct ExpectKlFinalArgs {
  const int32_t* sub_ids;   // [U, ld_sub] or null
  const float* sub_w;
  size_t ld_sub, ld_out;
  int T, scale_inv_tau;
  float* out;
  float* out_mass;          // [U] or null
};

// One workgroup per user, a thread per component (strided): affine_final_kernel with kl_bad's NaN rule.
__global__ __launch_bounds__(256) void expect_kl_final_kernel(KlArgs a, ExpectKlFinalArgs f) {
  const size_t u = blockIdx.x;
  const bool bad = kl_bad(a, u);
  const double it = f.scale_inv_tau ? (double)__fdiv_rn(1.f, a.tau_of(u)) : 1.0;
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

int expect_kl_stream_launch(int TR, bool pool, bool lists, dim3 grid, size_t smem, hipStream_t s, const KlArgs& a, const CsrArgs& ca) {
  return with_bool(pool, [&](auto p) {
    return with_bool(lists, [&](auto l) {
      constexpr bool P = decltype(p)::value, L = decltype(l)::value;
      if (TR == 64) return launch_lds(expect_kl_stream_kernel<4, XK_KMAX_64, P, L>, grid, dim3(TK_THREADS), smem, s, a, ca);
      if (TR == 32) return launch_lds(expect_kl_stream_kernel<2, XK_KMAX_32, P, L>, grid, dim3(TK_THREADS), smem, s, a, ca);
      return launch_lds(expect_kl_stream_kernel<1, XK_KMAX_16, P, L>, grid, dim3(TK_THREADS), smem, s, a, ca);
    });
  });
}

// ---- host ---------------------------------------------------------------------------------------------------------------

// the shared fields of the two descriptors, K17's refusals in K17's order; plan(U, V, N, 1).nseg = the segments of V, asked for
// only once V, U and N have passed
template <class D>
int kl_check_shared(const char* what, const D* d, LogzPlan (*plan)(int, int, int, int)) {
  NR_CHECK_RC(check_vectors(what, d->V, d->U, d->N));
  NR_CHECK_RC(check_lists(what, 0, d->excl_offsets, d->excl_ids, d->n_excl));   // this call has no dense list
  NR_CHECK_ARG(d->tau_u != nullptr || (d->tau > 0.f && d->tau < LZ_INF), "%s: tau = %g, a scalar temperature must be finite and > 0", what,
               (double)d->tau);
  NR_CHECK_ARG(d->ref_tau_u != nullptr || (d->ref_tau > 0.f && d->ref_tau < LZ_INF),
               "%s: ref_tau = %g, a scalar reference temperature must be finite and > 0", what, (double)d->ref_tau);
  const int nseg = plan(d->U, d->V, d->N, 1).nseg;
  NR_CHECK_ARG(d->splits >= 0 && d->splits <= nseg, "%s: splits = %d, must be 0 (library's choice) or in [1, %d], the segments of V = %d", what,
               d->splits, nseg, d->V);
  return check_pools(what, d->stamp, d->window, d->ld_window);
}
int kl_check(const nr_kl_desc* d) {
  NR_CHECK_ARG(d != nullptr, "score_kl: null descriptor");
  return kl_check_shared("score_kl", d, kl_plan);
}
int expect_kl_check(const nr_expect_kl_desc* d) {
  NR_CHECK_ARG(d != nullptr, "score_expect_kl: null descriptor");
  return kl_check_shared("score_expect_kl", d, xk_plan);
}
// the reference side's pointers and rows
template <class D>
int kl_check_ref(const char* what, const D* d) {
  NR_CHECK_ARG(d->ref != nullptr, "%s: null pointer (ref: the reference user vectors)", what);
  NR_CHECK_ARG(d->ref_base_max != nullptr && d->ref_base_logsum != nullptr,
               "%s: null pointer (ref_base_max, ref_base_logsum: the base of nr_score_logz for the reference vectors)", what);
  NR_CHECK_ARG(d->ld_ref >= d->N && d->ld_ref % 4 == 0 && (((uintptr_t)d->ref) & 15) == 0,
               "%s: ref rows must be 16-byte aligned (ld_ref = %d: a multiple of 4, >= N = %d)", what, d->ld_ref, d->N);
  return NR_OK;
}
template <class D>
void kl_fill(const D* d, const LogzPlan& pl, KlArgs* a) {
  a->news = d->news_vecs; a->user = d->user; a->ref = d->ref;
  a->ld_news = (size_t)d->ld_news; a->ld_user = (size_t)d->ld_user; a->ld_ref = (size_t)d->ld_ref;
  a->V = d->V; a->U = d->U; a->N = d->N; a->seg = pl.seg; a->nseg = pl.nseg; a->segs_per = pl.segs_per; a->splits = pl.splits;
  a->pool = pool_args(d->prior, d->stamp, d->window, d->ld_window);
  a->tau = d->tau; a->tau_u = d->tau_u; a->ref_tau = d->ref_tau; a->ref_tau_u = d->ref_tau_u;
  a->base_max = d->base_max; a->base_logsum = d->base_logsum;
  a->ref_base_max = d->ref_base_max; a->ref_base_logsum = d->ref_base_logsum;
  a->alpha = a->beta = a->gamma = nullptr;
  a->pm = nullptr; a->part = nullptr; a->pmass = nullptr;
}

}  // namespace

extern "C" {

size_t nr_score_kl_workspace_bytes(const nr_kl_desc* d) {
  if (kl_check(d) != NR_OK) return 0;
  return kl_carve(nullptr, d->U, kl_plan(d->U, d->V, d->N, d->splits).splits, nullptr);
}

int nr_score_kl(const nr_kl_desc* d, nr_stream_t stream) {
  NR_CHECK_RC(kl_check(d));
  NR_CHECK_ARG(d->news_vecs && d->user && d->base_max && d->base_logsum && d->out_kl,
               "score_kl: null pointer (news_vecs, user, base_max, base_logsum, out_kl)");
  NR_CHECK_RC(kl_check_ref("score_kl", d));
  NR_CHECK_RC(check_rows("score_kl", d->news_vecs, d->ld_news, d->user, d->ld_user, d->N));
  NR_CHECK_RC(check_workspace("score_kl", d->ws, d->ws_bytes, nr_score_kl_workspace_bytes(d)));
  NR_DEVICE_GUARD(stream, d->news_vecs);
  hipStream_t s = (hipStream_t)stream;
  const LogzPlan pl = kl_plan(d->U, d->V, d->N, d->splits);
  KlArgs a;
  kl_fill(d, pl, &a);
  kl_carve(d->ws, d->U, pl.splits, &a);
  const CsrArgs ca = csr_args(d->excl_offsets, d->excl_ids, d->n_excl);
  {
    const int TR = 2 * pl.TU;
    const size_t smem = tk_tile_bytes(TR, d->N);
    const dim3 grid((unsigned)((d->U + pl.TU - 1) / pl.TU), (unsigned)pl.splits);
    NrProfScope ps(s, "kl_stream[U=%d,V=%d,N=%d,TU=%d,splits=%d,seg=%d]", d->U, d->V, d->N, pl.TU, pl.splits, pl.seg);
    NR_CHECK_RC(kl_stream_launch(TR, a.pool.any(), ca.offsets != nullptr, grid, smem, s, a, ca));
  }
  NR_CHECK_LAUNCH();
  {
    NrProfScope ps(s, "kl_final[U=%d,splits=%d]", d->U, pl.splits);
    hipLaunchKernelGGL(kl_final_kernel, dim3((unsigned)((d->U + 3) / 4)), dim3(256), 0, s, a, d->out_kl, d->out_entropy, d->out_cov, d->out_mass);
  }
  NR_CHECK_LAUNCH();
  return NR_OK;
}

size_t nr_score_expect_kl_workspace_bytes(const nr_expect_kl_desc* d) {
  if (expect_kl_check(d) != NR_OK) return 0;
  return xk_carve(nullptr, d->U, xk_plan(d->U, d->V, d->N, d->splits).splits, d->N, nullptr);
}

int nr_score_expect_kl(const nr_expect_kl_desc* d, nr_stream_t stream) {
  NR_CHECK_RC(expect_kl_check(d));
  NR_CHECK_ARG(d->news_vecs && d->user && d->base_max && d->base_logsum && d->out,
               "score_expect_kl: null pointer (news_vecs, user, base_max, base_logsum, out)");
  NR_CHECK_RC(kl_check_ref("score_expect_kl", d));
  NR_CHECK_ARG(d->sub_ids == nullptr || d->sub_w != nullptr, "score_expect_kl: sub_ids given without sub_w (the two come together)");
  NR_CHECK_ARG(d->sub_w == nullptr || d->sub_ids != nullptr, "score_expect_kl: sub_w given without sub_ids (the two come together)");
  NR_CHECK_ARG(d->sub_ids == nullptr || (d->T >= 1 && d->T <= NR_TOPK_MAX_K && d->ld_sub >= d->T),
               "score_expect_kl: T = %d named rows per user (row stride %d), must be in [1, %d] with ld_sub >= T", d->T, d->ld_sub, NR_TOPK_MAX_K);
  NR_CHECK_RC(check_rows("score_expect_kl", d->news_vecs, d->ld_news, d->user, d->ld_user, d->N));
  NR_CHECK_ARG(d->ld_out >= d->N && (((uintptr_t)d->out) & 15) == 0, "score_expect_kl: out must be 16-byte aligned with ld_out = %d >= N = %d",
               d->ld_out, d->N);
  NR_CHECK_RC(check_workspace("score_expect_kl", d->ws, d->ws_bytes, nr_score_expect_kl_workspace_bytes(d)));
  NR_DEVICE_GUARD(stream, d->news_vecs);
  hipStream_t s = (hipStream_t)stream;
  const LogzPlan pl = xk_plan(d->U, d->V, d->N, d->splits);
  KlArgs a;
  kl_fill(d, pl, &a);
  a.alpha = d->alpha; a.beta = d->beta; a.gamma = d->gamma;
  xk_carve(d->ws, d->U, pl.splits, d->N, &a);
  const CsrArgs ca = csr_args(d->excl_offsets, d->excl_ids, d->n_excl);
  {
    const int TR = 2 * pl.TU;
    const size_t smem = xk_smem(TR, d->N);
    const dim3 grid((unsigned)((d->U + pl.TU - 1) / pl.TU), (unsigned)pl.splits);
    NrProfScope ps(s, "expect_kl_stream[U=%d,V=%d,N=%d,TU=%d,splits=%d,seg=%d]", d->U, d->V, d->N, pl.TU, pl.splits, pl.seg);
    NR_CHECK_RC(expect_kl_stream_launch(TR, a.pool.any(), ca.offsets != nullptr, grid, smem, s, a, ca));
  }
  NR_CHECK_LAUNCH();
  {
    ExpectKlFinalArgs f;
    f.sub_ids = d->sub_ids; f.sub_w = d->sub_w;
    f.ld_sub = (size_t)d->ld_sub; f.ld_out = (size_t)d->ld_out;
    f.T = d->sub_ids != nullptr ? d->T : 0; f.scale_inv_tau = d->scale_inv_tau;
    f.out = d->out; f.out_mass = d->out_mass;
    NrProfScope ps(s, "expect_kl_final[U=%d,N=%d,splits=%d,T=%d]", d->U, d->N, pl.splits, f.T);
    hipLaunchKernelGGL(expect_kl_final_kernel, dim3((unsigned)d->U), dim3(256), 0, s, a, f);
  }
  NR_CHECK_LAUNCH();
  return NR_OK;
}

}  // extern "C"
