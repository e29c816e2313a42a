// The news side of the entropy-regularised full-softmax gradient (include/nrhip.h, K25): for L = sum_u (sum_t g_ut nll(u, t) + h_u H_u)
//   d L / d news_v = sum_u (1 / tau_u) p(v | u) (alpha_u + beta_u x_uv) user_u - sum_{(u, t): target = v} (g_ut / tau_u) user_u,
//   x_uv = log p(v | u),  alpha_u = sum_t g_ut - h_u H_u,  beta_u = -h_u
// over exactly the pairs (u, v) that are terms of K13's sums, without the [U, V] matrix.  K18 (nr_expect_news.hip) with the step
// K24 (nr_entropy.hip) made on K17: the value stored to the P tile is p (a_u + b_u x) in place of c_u p.
//
//   expect_news_affine_stream_kernel<MT, KMAX, POOL, LISTS>   expect_news_stream_kernel<..., ROWS = true> of nr_expect_news.hip,
//                           statement for statement, but for the per-user coefficients and the value stored to the P tile.  Per lane
//                           and streamed user j: a = alpha (* 1 / tau if scale_inv_tau), b = beta (likewise), fin = both finite;
//                           per pair x = fmaf(s - max, 1 / tau, -logsum), p = expf(x) (0 where the pair is not eligible) and
//                           P = (p == 0 || !fin) ? 0 : fl(p * fmaf(b, x, a)).  0 * -inf is never formed; a user whose alpha or
//                           beta is NaN or infinite contributes to no row.  The fp64 running mass adds p (K18's with weight NULL).
//   expect_news_affine_final_kernel   expect_news_final_kernel: the slices ascending in fp64, minus the named terms (gated by the
//                           user being live, not by alpha or beta), one rounding.
//
// The plan, the carve, the live rule and the cleaning of components are copies of nr_expect_news.hip's (its anonymous namespace is
// not shared; the kernels of that unit keep their instruction streams).  The chain of one (news, component) is K18's: which wave
// holds a (news, column) and which users it covers is fixed by N alone, chunk starts by U, slices by (U, splits) -- no row's bits
// depend on another's.  With beta NULL, fmaf(0, x, a) == a and fl(p * a) == fl(a * p): K18's rows with weight = alpha.
#include <math.h>

#include "nr_logz_stream.h"

namespace {

struct AffineNewsArgs {
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
  int scale_inv_tau;
  float* part;              // [V, splits, N] partial rows
  double* pmass;            // [V, splits] partial masses
  __device__ __forceinline__ float tau_of(long u) const { return tau_u != nullptr ? tau_u[u] : tau; }
};
// workspace: the masses first (8-byte aligned), then the partial rows (K18's rows-mode layout and size)
inline size_t ea_carve(void* ws, int V, int splits, int N, AffineNewsArgs* a) {
  char* p = reinterpret_cast<char*>(ws);
  const size_t n = (size_t)V * splits;
  if (a) {
    a->pmass = reinterpret_cast<double*>(p);
    a->part = reinterpret_cast<float*>(p + n * 8);
  }
  return (n * 8 + n * (size_t)N * 4 + 7) & ~(size_t)7;
}

constexpr size_t EA_PER_ROW = TK_LDS_TILE * sizeof(float);   // a news row's row of P
// the news tile (a function of N alone; K17's table: 64 rows up to 11 k-slabs, 32 up to 26, else 16)
inline int ea_news_tile(int N) { return score_user_tile(N, EA_PER_ROW); }
// lz_plan_tile's arithmetic on the U users [0, U) in place of the V - 1 news [1, V); the "user tiles" that fill the chip are news tiles
inline LogzPlan ea_plan(int V, int U, int N, int splits) { return lz_plan_tile(V, U + 1, ea_news_tile(N), splits); }

// a user who gets no weight anywhere, in the stream and in the named terms: a temperature that is not finite and > 0, a base that
// is NaN or infinite (nothing eligible: max = -inf)
__device__ __forceinline__ bool ea_live(float tau, float bmax, float bls) {
  return tau > 0.f && tau < LZ_INF && fabsf(bmax) < LZ_INF && fabsf(bls) < LZ_INF;
}
// a component that is not finite counts as 0 in D: ex_clean's reason with the roles swapped (a user with such a component scores NaN
// or infinite against every news; 0 * NaN in the contraction would reach every news of the tile)
__device__ __forceinline__ void ea_clean(f32x4& g) {
#pragma unroll
  for (int e = 0; e < 4; ++e) g[e] = fabsf(g[e]) < LZ_INF ? g[e] : 0.f;
}

template <int MT, int KMAX, bool POOL, bool LISTS>
__global__ __launch_bounds__(TK_THREADS) void expect_news_affine_stream_kernel(AffineNewsArgs a, CsrArgs ca) {
  constexpr int TV = 16 * MT, PER_WAVE = TV / TK_WAVES;
  constexpr int PAIRS = 2 * MT, PARTS = TK_WAVES / PAIRS, PART_ROWS = TK_ROWS / PARTS, STEPS = PART_ROWS / 16;
  static_assert(PAIRS * PARTS == TK_WAVES && STEPS >= 1, "8 waves = pairs x row parts");
  extern __shared__ __attribute__((aligned(16))) float ea_smem[];
  ScoreTile<MT> t(ea_smem, a.N);
  float* sP = t.end();                                        // [TV, TK_LDS_TILE] the chunk's weights
  const int lane = t.lane, wave = t.wave;
  const int v0 = blockIdx.x * TV;
  const int s_lo = (int)blockIdx.y * a.segs_per;
  const int s_hi = s_lo + a.segs_per < a.nseg ? s_lo + a.segs_per : a.nseg;
  const long u_lo = (long)s_lo * a.seg;
  const long u_hi = (long)s_hi * a.seg < a.U ? (long)s_hi * a.seg : a.U;
  if (u_lo >= u_hi) return;                                   // the whole workgroup (ea_plan leaves no empty slice)
  const int ksteps = t.ksteps;                                // <= KMAX by the launch's choice of instantiation

  t.load_users(a.news, a.ld_news, v0, a.V);                   // the stationary operand: news rows v0 .. v0 + TV - 1
  // news row wave + 8 i of the tile: whether it is a news at all (row 0 never), and this lane's running mass
  bool alive[PER_WAVE];
  double mass[PER_WAVE];
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int v = v0 + wave + TK_WAVES * i;
    alive[i] = v >= 1 && v < a.V;
    mass[i] = 0.0;
  }
  // LISTS: the cursor of every news of the wave into its list of users = the first entry that is >= u_lo (LZ_SEEK, nr_logz_stream.h)
  int32_t cur[PER_WAVE], end[PER_WAVE];
  if constexpr (LISTS) LZ_SEEK(ca, v0, wave, lane, a.V, u_lo, cur, end)
  // POOL: lane i keeps the prior and the stamp of this wave's i-th news; switched off beyond V
  float n_prior = -LZ_INF;
  int32_t n_stamp = 0;
  if constexpr (POOL) {
    const int v = v0 + wave + TK_WAVES * lane;
    if (lane < PER_WAVE && v < a.V) {
      n_prior = a.pool.prior_of(v);
      n_stamp = a.pool.stamp_of(v);
    }
  }

  // the second contraction: this wave's (news tile, column tile) pair and its part of the chunk's users
  const int pair = wave % PAIRS, part = wave / PAIRS;
  const int ti = pair >> 1, tj = pair & 1, rbase = part * PART_ROWS;
  const int frow = lane & 15, fg = lane >> 4;
  f32x4 out[KMAX];
#pragma unroll
  for (int ks = 0; ks < KMAX; ++ks) out[ks] = (f32x4){0.f, 0.f, 0.f, 0.f};

  ScoreStreamRows rows = {a.user, a.ld_user, u_lo, u_hi};
  t.load_slab(rows, 0);
  for (long uc = u_lo; uc < u_hi; uc += TK_ROWS) {
    f32x4 acc[MT];
    // users uc + lane (j = 0) and uc + lane + 64 (j = 1): temperature, base, alpha, beta and window, loaded ahead of the scoring pass
    // (which hides their latency) ...
    float tau[2], bm[2], nbl[2], al[2], be[2];
    int32_t w_lo[2], w_hi[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long u = uc + lane + 64 * j;
      const bool in = u < u_hi;
      tau[j] = in ? a.tau_of(u) : 0.f;                        // beyond the slice: a dead user
      bm[j] = in ? a.base_max[u] : -LZ_INF;
      nbl[j] = in ? a.base_logsum[u] : 0.f;
      al[j] = in && a.alpha != nullptr ? a.alpha[u] : 1.f;
      be[j] = in && a.beta != nullptr ? a.beta[u] : 0.f;
      w_lo[j] = 1;
      w_hi[j] = 0;
      if constexpr (POOL) {
        if (in) {
          w_lo[j] = a.pool.lo_of(u);
          w_hi[j] = a.pool.hi_of(u);
        }
      }
    }
    rows.vc = uc;
    t.chunk(rows, acc);
    t.load_slab(rows, 0);                                     // the same chunk again: in flight while the weights are formed
    // ... and what is formed from them: 1 / tau, -logsum, the two coefficients (whether both are finite), whether the user gets
    // weights at all
    float it[2];
    bool live[2], fin[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      live[j] = ea_live(tau[j], bm[j], nbl[j]);
      it[j] = __fdiv_rn(1.f, tau[j]);
      nbl[j] = -nbl[j];
      if (a.scale_inv_tau) {
        al[j] = __fmul_rn(al[j], it[j]);
        be[j] = __fmul_rn(be[j], it[j]);
      }
      fin[j] = fabsf(al[j]) < LZ_INF && fabsf(be[j]) < LZ_INF;
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
      const int vl = wave + TK_WAVES * i;
      u64 l0 = 0ull, l1 = 0ull;
      if constexpr (LISTS) LZ_LISTED(ca, e0[i], cur[i], end[i], uc, lane, l0, l1)
      uint32_t k0, k1;
      if constexpr (POOL) {
        const float pr = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, n_prior), i));
        const int32_t st = __builtin_amdgcn_readlane(n_stamp, i);
        k0 = pool_key(sS[vl * TK_LDS_TILE + lane], pr, st, w_lo[0], w_hi[0]);
        k1 = pool_key(sS[vl * TK_LDS_TILE + lane + 64], pr, st, w_lo[1], w_hi[1]);
      } else {
        k0 = score_key(sS[vl * TK_LDS_TILE + lane]);
        k1 = score_key(sS[vl * TK_LDS_TILE + lane + 64]);
      }
      // eligible as in logz_stream_kernel: a news, a live user of the slice, key != 0 (not NaN, inside the pool), not listed
      const bool el0 = alive[i] && live[0] && k0 != 0u && ((l0 >> lane) & 1ull) == 0ull;
      const bool el1 = alive[i] && live[1] && k1 != 0u && ((l1 >> lane) & 1ull) == 0ull;
      // x = log p = fmaf(s - max, 1 / tau, -logsum), p = expf(x): K18's; s == max: x = -logsum, never 0 * inf where 1 / tau
      // overflowed.  The pair's weight is p (b x + a): 0 where p == 0 (0 * -inf is never formed) or a coefficient is not finite
      const float d0 = key_score(k0) - bm[0], d1 = key_score(k1) - bm[1];
      const float x0 = d0 == 0.f ? nbl[0] : fmaf(d0, it[0], nbl[0]), x1 = d1 == 0.f ? nbl[1] : fmaf(d1, it[1], nbl[1]);
      const float p0 = el0 ? expf(x0) : 0.f;
      const float p1 = el1 ? expf(x1) : 0.f;
      sP[vl * TK_LDS_TILE + lane] = (p0 == 0.f || !fin[0]) ? 0.f : __fmul_rn(p0, fmaf(be[0], x0, al[0]));
      sP[vl * TK_LDS_TILE + lane + 64] = (p1 == 0.f || !fin[1]) ? 0.f : __fmul_rn(p1, fmaf(be[1], x1, al[1]));
      mass[i] += (double)p0 + (double)p1;
    }
    __syncthreads();                                          // P is whole; the score tile is the staging buffer again

    // the wave's fragment of P: pa[s][e] = weight of news ti * 16 + frow for chunk user rbase + 16 s + 4 fg + e
    f32x4 pa[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) pa[s] = *reinterpret_cast<const f32x4*>(sP + (ti * 16 + frow) * TK_LDS_TILE + rbase + 16 * s + 4 * fg);
    ea_clean(t.g0);
    ea_clean(t.g1);
    t.store_slab(0);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < KMAX; ++ks) {
      if (ks < ksteps) {
        if (ks + 1 < ksteps) t.load_slab(rows, ks + 1);
        else if (uc + TK_ROWS < u_hi) {                     // the next chunk's first slab, for ScoreTile::chunk
          rows.vc = uc + TK_ROWS;
          t.load_slab(rows, 0);
        }
        // B[k = fg][n = frow] = slab row rbase + 16 s + 4 fg + e, column tj * 16 + frow: the 64 lanes read 64 different banks
        const float* pb = t.sB + (size_t)(ks & 1) * TK_ROWS * TK_LDB + (rbase + 4 * fg) * TK_LDB + tj * 16 + frow;
#pragma unroll
        for (int s = 0; s < STEPS; ++s)
#pragma unroll
          for (int e = 0; e < 4; ++e) out[ks] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[s][e], pb[(16 * s + e) * TK_LDB], out[ks], 0, 0, 0);
        if (ks + 1 < ksteps) {
          ea_clean(t.g0);
          ea_clean(t.g1);
          t.store_slab((ks + 1) & 1);
        }
        __syncthreads();
      }
    }
  }

  // slice end.  The mass: one partial per (news, slice)
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int v = v0 + wave + TK_WAVES * i;
    const double m = wave_sum_d(mass[i]);
    if (lane == 0 && v < a.V) a.pmass[(size_t)v * a.splits + blockIdx.y] = m;
  }
  // The rows: out[ks][r] belongs to news ti * 16 + 4 fg + r, column ks * 32 + tj * 16 + frow.  The row parts are added in
  // ascending order, ((part 0 + part 1) + part 2) + part 3, through the news vectors' LDS (the slice is over; [TV, ldu] >= [TV, npad])
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
          const int v = v0 + ti * 16 + 4 * fg + r;
          if (v < a.V && c < a.N) a.part[((size_t)v * a.splits + blockIdx.y) * a.N + c] = out[ks][r];
        }
      }
  }
}

struct AffineNewsFinalArgs {
  CsrArgs named;            // offsets [V + 1], ids = named_user [n]; offsets null = no named terms
  const float* named_w;     // [n]
  size_t ld_out;
  float* out;               // [V, ld_out]
  float* out_mass;          // [V] or null
};

// One workgroup per news row, a thread per component (strided).  The named terms are gated by ea_live alone: alpha and beta weigh
// the stream's pairs, not the targets.
__global__ __launch_bounds__(256) void expect_news_affine_final_kernel(AffineNewsArgs a, AffineNewsFinalArgs f) {
  const size_t v = blockIdx.x;
  int32_t jb = 0, je = 0;
  if (f.named.offsets != nullptr) f.named.segment((long)v, jb, je);
  for (int c = threadIdx.x; c < a.N; c += blockDim.x) {
    double e = 0.0;
    for (int s = 0; s < a.splits; ++s) e += (double)a.part[(v * a.splits + s) * a.N + c];
    for (int32_t j = jb; j < je; ++j) {
      const float w = f.named_w[j];
      const int32_t u = f.named.ids[j];
      if (w == 0.f || u < 0 || u >= a.U) continue;
      const float tau = a.tau_of(u);
      if (!ea_live(tau, a.base_max[u], a.base_logsum[u])) continue;
      const float x = a.user[(size_t)u * a.ld_user + c];
      const double it = a.scale_inv_tau ? (double)__fdiv_rn(1.f, tau) : 1.0;
      if (fabsf(x) < LZ_INF) e -= (double)w * it * (double)x;
    }
    f.out[v * f.ld_out + c] = (float)e;
  }
  if (threadIdx.x == 0 && f.out_mass != nullptr) {
    double m = 0.0;
    for (int s = 0; s < a.splits; ++s) m += a.pmass[v * a.splits + s];
    f.out_mass[v] = (float)m;
  }
}

// argument checks shared by the size query and the call; 0 = fine.  K18's, in K18's order; `out` is required here
int expect_news_affine_check(const nr_expect_news_affine_desc* d) {
  NR_CHECK_ARG(d != nullptr, "score_expect_news_affine: null descriptor");
  NR_CHECK_RC(check_vectors("score_expect_news_affine", d->V, d->U, d->N));
  NR_CHECK_ARG(d->n_excl >= 0, "score_expect_news_affine: n_excl = %d entries of excl_users, must be >= 0", d->n_excl);
  NR_CHECK_ARG(d->n_excl == 0 || d->excl_users == nullptr || d->excl_offsets != nullptr,
               "score_expect_news_affine: excl_users given without excl_offsets (n_excl = %d; the two come together)", d->n_excl);
  NR_CHECK_ARG(d->n_excl == 0 || d->excl_offsets == nullptr || d->excl_users != nullptr,
               "score_expect_news_affine: excl_offsets given without excl_users (n_excl = %d; the two come together)", d->n_excl);
  NR_CHECK_ARG(d->tau_u != nullptr || (d->tau > 0.f && d->tau < LZ_INF),
               "score_expect_news_affine: tau = %g, a scalar temperature must be finite and > 0", (double)d->tau);
  const int nseg = ea_plan(d->V, d->U, d->N, 1).nseg;
  NR_CHECK_ARG(d->splits >= 0 && d->splits <= nseg,
               "score_expect_news_affine: splits = %d, must be 0 (library's choice) or in [1, %d], the segments of U = %d", d->splits, nseg, d->U);
  NR_CHECK_RC(check_pools("score_expect_news_affine", d->stamp, d->window, d->ld_window));
  NR_CHECK_ARG(d->out != nullptr, "score_expect_news_affine: out is null (this call has no mass-only mode: nr_score_expect_news has it)");
  return NR_OK;
}

// the stream's instantiation for the run-time (tile, pool, lists); the tile fixes the k-slabs that can occur with it
int expect_news_affine_stream_launch(int TV, bool pool, bool lists, dim3 grid, size_t smem, hipStream_t s, const AffineNewsArgs& a,
                                     const CsrArgs& ca) {
  return with_bool(pool, [&](auto p) {
    return with_bool(lists, [&](auto l) {
      constexpr bool P = decltype(p)::value, L = decltype(l)::value;
      if (TV == 64) return launch_lds(expect_news_affine_stream_kernel<4, 11, P, L>, grid, dim3(TK_THREADS), smem, s, a, ca);
      if (TV == 32) return launch_lds(expect_news_affine_stream_kernel<2, 26, P, L>, grid, dim3(TK_THREADS), smem, s, a, ca);
      return launch_lds(expect_news_affine_stream_kernel<1, NR_TOPK_MAX_N / TK_KS, P, L>, grid, dim3(TK_THREADS), smem, s, a, ca);
    });
  });
}

}  // namespace

extern "C" {

size_t nr_score_expect_news_affine_workspace_bytes(const nr_expect_news_affine_desc* d) {
  if (expect_news_affine_check(d) != NR_OK) return 0;
  return ea_carve(nullptr, d->V, ea_plan(d->V, d->U, d->N, d->splits).splits, d->N, nullptr);
}

int nr_score_expect_news_affine(const nr_expect_news_affine_desc* d, nr_stream_t stream) {
  NR_CHECK_RC(expect_news_affine_check(d));
  NR_CHECK_ARG(d->news_vecs && d->user && d->base_max && d->base_logsum,
               "score_expect_news_affine: null pointer (news_vecs, user, base_max, base_logsum)");
  const bool named_all = d->named_offsets && d->named_user && d->named_w, named_any = d->named_offsets || d->named_user || d->named_w;
  NR_CHECK_ARG(named_all || !named_any, "score_expect_news_affine: named_offsets, named_user and named_w come together (all three or none)");
  NR_CHECK_ARG(d->n_named >= 0, "score_expect_news_affine: n_named = %d named terms, must be >= 0", d->n_named);
  NR_CHECK_RC(check_rows("score_expect_news_affine", d->news_vecs, d->ld_news, d->user, d->ld_user, d->N));
  NR_CHECK_ARG(d->ld_out >= d->N && (((uintptr_t)d->out) & 15) == 0,
               "score_expect_news_affine: out must be 16-byte aligned with ld_out = %d >= N = %d", d->ld_out, d->N);
  NR_CHECK_RC(check_workspace("score_expect_news_affine", d->ws, d->ws_bytes, nr_score_expect_news_affine_workspace_bytes(d)));
  NR_DEVICE_GUARD(stream, d->news_vecs);
  hipStream_t s = (hipStream_t)stream;
  const LogzPlan pl = ea_plan(d->V, d->U, d->N, d->splits);
  AffineNewsArgs a;
  a.news = d->news_vecs; a.user = d->user;
  a.ld_news = (size_t)d->ld_news; a.ld_user = (size_t)d->ld_user;
  a.V = d->V; a.U = d->U; a.N = d->N; a.seg = pl.seg; a.nseg = pl.nseg; a.segs_per = pl.segs_per; a.splits = pl.splits;
  a.pool = pool_args(d->prior, d->stamp, d->window, d->ld_window);
  a.tau = d->tau; a.tau_u = d->tau_u;
  a.base_max = d->base_max; a.base_logsum = d->base_logsum;
  a.alpha = d->alpha; a.beta = d->beta; a.scale_inv_tau = d->scale_inv_tau;
  ea_carve(d->ws, d->V, pl.splits, d->N, &a);
  const CsrArgs ca = csr_args(d->excl_offsets, d->excl_users, d->n_excl);
  {
    const int TV = pl.TU;
    const size_t smem = tk_tile_bytes(TV, d->N) + TV * EA_PER_ROW;
    const dim3 grid((unsigned)((d->V + TV - 1) / TV), (unsigned)pl.splits);
    NrProfScope ps(s, "expect_news_affine_stream[V=%d,U=%d,N=%d,TV=%d,splits=%d,seg=%d,pool=%d,lists=%d,rows=1]", d->V, d->U, d->N, TV, pl.splits,
                   pl.seg, a.pool.any() ? 1 : 0, ca.offsets != nullptr ? 1 : 0);
    NR_CHECK_RC(expect_news_affine_stream_launch(TV, a.pool.any(), ca.offsets != nullptr, grid, smem, s, a, ca));
  }
  NR_CHECK_LAUNCH();
  {
    AffineNewsFinalArgs f;
    f.named = csr_args(named_all ? d->named_offsets : nullptr, d->named_user, d->n_named);
    f.named_w = d->named_w;
    f.ld_out = (size_t)d->ld_out;
    f.out = d->out; f.out_mass = d->out_mass;
    NrProfScope ps(s, "expect_news_affine_final[V=%d,N=%d,splits=%d,named=%d]", d->V, d->N, pl.splits, f.named.n);
    hipLaunchKernelGGL(expect_news_affine_final_kernel, dim3((unsigned)d->V), dim3(256), 0, s, a, f);
  }
  NR_CHECK_LAUNCH();
  return NR_OK;
}

}  // extern "C"
