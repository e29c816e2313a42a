// The news side of the capped row's gradient (include/nrhip.h, K22): D_v = sum_u cf[u, bin(v)] p_bin(v)(v | u) user_u over
// exactly the pairs (u, v) that are terms of K15's sum for bin(v) -- expect_news_stream_kernel of nr_expect_news.hip (K18) with
// the per-bin treatment of nr_expect_groups.hip (K20).  A tile of POSITIONS of the group-major order stays in LDS, its rows
// gathered through order[]; every bin's run starts at a multiple of 128 positions and the tile is 64, 32 or 16 rows, so a tile
// lies in ONE bin, which the workgroup finds once from bin_start.  The USERS are streamed past it in chunks of 128; per chunk
// the lanes load (gmax, logsum, omega) of THEIR users for THAT bin from the bin-major arrays [n_groups + 1, ld_bin]: 64
// consecutive floats a wave.  Scores, keys, the list cursor (over the lists BY POSITION), the pair weight, the second
// contraction, the slices of the user axis and the partials are K18's; the partials are written at the news ID, so the
// workspace and the finalize need no position map.
//
//   expect_news_groups_stream_kernel<MT, KMAX, POOL, LISTS>   grid = position tiles x user slices.  A tile that holds only padding
//                           (ids 0) returns before it loads anything.  Otherwise K18's loop; a (user, bin) pair that is not
//                           live -- tau not finite and > 0, gmax or logsum not finite, omega not finite or 0 -- has weight 0.
//                           NOT K20's rule (a row of NaN for such a user): on the news side one NaN would reach every row.
//   expect_news_groups_final_kernel   one workgroup per news row: the slices ascending in fp64 (row 0 is in no order and reads
//                           none), minus the named terms, gated by the USER ONLY (tau, w != 0, the index, finite components):
//                           under caps a bin is routinely empty because the row took all of it, and its entries still carry
//                           c != 0.  Rounded to fp32 once.
//
// The chain of one (news, component) is K18's: which wave holds a (news, column) and which users it covers is fixed by N alone,
// chunk starts by U, slices by (U, splits).  News of a tile are rows of A: no row's bits depend on another's, on its place in its
// run or tile, or on the sizes of the other bins.  en_plan, en_carve and en_clean of nr_expect_news.hip are copied: that unit's
// kernels keep the instruction streams they have.
#include <math.h>

#include "nr_logz_stream.h"

namespace {

struct EngArgs {
  const float* news;
  const float* user;
  size_t ld_news, ld_user, ld_bin;
  int V, U, N, seg, nseg, segs_per, splits, n_pos, n_bins;
  const int32_t* order;     // [n_pos]
  const int32_t* bin_start; // [n_bins + 1]
  PoolArgs pool;            // read by the POOL instantiations only; indexed by news id
  float tau;                // used when tau_u is null
  const float* tau_u;       // [U] or null
  const float* base_max;    // [n_bins, ld_bin]
  const float* base_logsum; // [n_bins, ld_bin]
  const float* bin_w;       // [n_bins, ld_bin]
  int scale_inv_tau;
  float* part;              // [V, splits, N] partial rows, by news id
  double* pmass;            // [V, splits] partial masses, by news id
  __device__ __forceinline__ float tau_of(long u) const { return tau_u != nullptr ? tau_u[u] : tau; }
  // the news id of position p; 0 = padding: beyond the order, id 0, or an id outside [1, V) whatever the table holds
  __device__ __forceinline__ int32_t id_at(long p) const {
    const int32_t id = p < n_pos ? order[p] : 0;
    return id >= 1 && id < V ? id : 0;
  }
  // the bin that owns position p: the first b with bin_start[b + 1] > p, clamped into [0, n_bins - 1]
  __device__ __forceinline__ int bin_of(long p) const {
    int lo = 0, hi = n_bins - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (bin_start[mid + 1] <= p) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  }
};
// workspace: the masses first (8-byte aligned), then the partial rows
inline size_t eng_carve(void* ws, int V, int splits, int N, EngArgs* a) {
  char* p = reinterpret_cast<char*>(ws);
  const size_t n = (size_t)V * splits;
  if (a) {
    a->pmass = reinterpret_cast<double*>(p);
    a->part = reinterpret_cast<float*>(p + n * 8);
  }
  return (n * 8 + n * (size_t)N * 4 + 7) & ~(size_t)7;
}

constexpr size_t ENG_PER_ROW = TK_LDS_TILE * sizeof(float);   // a news row's row of P
// K18's tile and plan: the tile a function of N alone, the user axis cut the way lz_plan_tile cuts [1, V)
inline int eng_news_tile(int N) { return score_user_tile(N, ENG_PER_ROW); }
inline LogzPlan eng_plan(int V, int U, int N, int splits) { return lz_plan_tile(V, U + 1, eng_news_tile(N), splits); }

__device__ __forceinline__ bool eng_tau_ok(float tau) { return tau > 0.f && tau < LZ_INF; }
// en_clean of nr_expect_news.hip: a component that is not finite counts as 0
__device__ __forceinline__ void eng_clean(f32x4& g) {
#pragma unroll
  for (int e = 0; e < 4; ++e) g[e] = fabsf(g[e]) < LZ_INF ? g[e] : 0.f;
}

// ScoreTile::load_users with the tile's rows gathered through order[]: tile row r = news row order[p0 + r], zeros for padding
template <int MT>
__device__ __forceinline__ void eng_load_tile(ScoreTile<MT>& t, const EngArgs& a, long p0) {
  for (int i = t.tid; i < ScoreTile<MT>::TU * (t.npad / 4); i += TK_THREADS) {
    const int r = i / (t.npad / 4), c = (i - r * (t.npad / 4)) * 4;
    const int32_t id = a.id_at(p0 + r);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (id != 0 && c < t.N) v = *reinterpret_cast<const f32x4*>(a.news + (size_t)id * a.ld_news + c);
    *reinterpret_cast<f32x4*>(t.sU + (size_t)r * t.ldu + c) = v;
  }
}

template <int MT, int KMAX, bool POOL, bool LISTS>
__global__ __launch_bounds__(TK_THREADS) void expect_news_groups_stream_kernel(EngArgs a, CsrArgs ca) {
  constexpr int TV = 16 * MT, PER_WAVE = TV / TK_WAVES;
  constexpr int PAIRS = 2 * MT, PARTS = TK_WAVES / PAIRS, PART_ROWS = TK_ROWS / PARTS, STEPS = PART_ROWS / 16;
  static_assert(PAIRS * PARTS == TK_WAVES && STEPS >= 1, "8 waves = pairs x row parts");
  extern __shared__ __attribute__((aligned(16))) float eng_smem[];
  ScoreTile<MT> t(eng_smem, a.N);
  float* sP = t.end();                                        // [TV, TK_LDS_TILE] the chunk's weights
  const int lane = t.lane, wave = __builtin_amdgcn_readfirstlane(t.wave);   // uniform: what is per news row stays in scalar registers
  const long p0 = (long)blockIdx.x * TV;                      // the tile's first position
  const int s_lo = (int)blockIdx.y * a.segs_per;
  const int s_hi = s_lo + a.segs_per < a.nseg ? s_lo + a.segs_per : a.nseg;
  const long u_lo = (long)s_lo * a.seg;
  const long u_hi = (long)s_hi * a.seg < a.U ? (long)s_hi * a.seg : a.U;
  if (u_lo >= u_hi) return;                                   // the whole workgroup (eng_plan leaves no empty slice)
  // a tile that holds only padding -- the tail of a bin's run -- loads nothing and writes nothing
  if (!__syncthreads_or(t.tid < TV && a.id_at(p0 + t.tid) != 0)) return;
  const int ksteps = t.ksteps;                                // <= KMAX by the launch's choice of instantiation
  const size_t bin_at = (size_t)a.bin_of(p0) * a.ld_bin;      // the tile's bin: its row of the three bin-major arrays

  eng_load_tile(t, a, p0);                                    // the stationary operand: news rows order[p0 .. p0 + TV - 1]
  // news row wave + 8 i of the tile: whether it is a news at all (padding never), and this lane's running mass
  bool alive[PER_WAVE];
  double mass[PER_WAVE];
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    alive[i] = a.id_at(p0 + wave + TK_WAVES * i) != 0;
    mass[i] = 0.0;
  }
  // LISTS: the cursor of every position of the wave into its list of users = the first entry that is >= u_lo
  int32_t cur[PER_WAVE], end[PER_WAVE];
  if constexpr (LISTS) LZ_SEEK(ca, p0, wave, lane, a.n_pos, u_lo, cur, end)
  // POOL: lane i keeps the prior and the stamp of this wave's i-th news, gathered by id; switched off for padding
  float n_prior = -LZ_INF;
  int32_t n_stamp = 0;
  if constexpr (POOL) {
    const int32_t id = lane < PER_WAVE ? a.id_at(p0 + wave + TK_WAVES * lane) : 0;
    if (id != 0) {
      n_prior = a.pool.prior_of(id);
      n_stamp = a.pool.stamp_of(id);
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
    // users uc + lane (j = 0) and uc + lane + 64 (j = 1): temperature, window, and the base and omega of the tile's bin, loaded
    // ahead of the scoring pass (which hides their latency) ...
    float tau[2], bm[2], nbl[2], om[2];
    int32_t w_lo[2], w_hi[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long u = uc + lane + 64 * j;
      const bool in = u < u_hi;
      tau[j] = in ? a.tau_of(u) : 0.f;                        // beyond the slice: a dead user
      bm[j] = in ? a.base_max[bin_at + u] : -LZ_INF;
      nbl[j] = in ? a.base_logsum[bin_at + u] : 0.f;
      om[j] = in ? a.bin_w[bin_at + u] : 0.f;
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
    // ... and what is formed from them: 1 / tau, -logsum, the coefficient, whether the (user, bin) pair gets weights at all
    float it[2], cf[2];
    bool live[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      live[j] = eng_tau_ok(tau[j]) && fabsf(bm[j]) < LZ_INF && fabsf(nbl[j]) < LZ_INF && om[j] != 0.f && fabsf(om[j]) < LZ_INF;
      it[j] = __fdiv_rn(1.f, tau[j]);
      nbl[j] = -nbl[j];
      cf[j] = a.scale_inv_tau ? __fmul_rn(om[j], it[j]) : om[j];
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
      // eligible as in logzg_stream_kernel: a real news (not padding), a live pair of the slice, key != 0, not listed
      const bool el0 = alive[i] && live[0] && k0 != 0u && ((l0 >> lane) & 1ull) == 0ull;
      const bool el1 = alive[i] && live[1] && k1 != 0u && ((l1 >> lane) & 1ull) == 0ull;
      // p = expf(fmaf(s - gmax, 1 / tau, -logsum)); s == gmax: expf(-logsum), never 0 * inf where 1 / tau overflowed
      const float d0 = key_score(k0) - bm[0], d1 = key_score(k1) - bm[1];
      const float q0 = el0 ? expf(d0 == 0.f ? nbl[0] : fmaf(d0, it[0], nbl[0])) : 0.f;
      const float q1 = el1 ? expf(d1 == 0.f ? nbl[1] : fmaf(d1, it[1], nbl[1])) : 0.f;
      sP[vl * TK_LDS_TILE + lane] = el0 ? __fmul_rn(cf[0], q0) : 0.f;
      sP[vl * TK_LDS_TILE + lane + 64] = el1 ? __fmul_rn(cf[1], q1) : 0.f;
      mass[i] += (el0 ? (double)om[0] * (double)q0 : 0.0) + (el1 ? (double)om[1] * (double)q1 : 0.0);
    }
    __syncthreads();                                          // P is whole; the score tile is the staging buffer again

    // the wave's fragment of P: pa[s][e] = weight of news ti * 16 + frow for chunk user rbase + 16 s + 4 fg + e
    f32x4 pa[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) pa[s] = *reinterpret_cast<const f32x4*>(sP + (ti * 16 + frow) * TK_LDS_TILE + rbase + 16 * s + 4 * fg);
    eng_clean(t.g0);
    eng_clean(t.g1);
    t.store_slab(0);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < KMAX; ++ks) {
      if (ks < ksteps) {
        if (ks + 1 < ksteps) t.load_slab(rows, ks + 1);
        else if (uc + TK_ROWS < u_hi) {                       // the next chunk's first slab, for ScoreTile::chunk
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
          eng_clean(t.g0);
          eng_clean(t.g1);
          t.store_slab((ks + 1) & 1);
        }
        __syncthreads();
      }
    }
  }

  // slice end.  The mass: one partial per (news, slice), at the news id
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int32_t v = a.id_at(p0 + wave + TK_WAVES * i);
    const double m = wave_sum_d(mass[i]);
    if (lane == 0 && v != 0) a.pmass[(size_t)v * a.splits + blockIdx.y] = m;
  }
  // The rows: out[ks][r] belongs to tile row ti * 16 + 4 fg + r, column ks * 32 + tj * 16 + frow.  The row parts are added in
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
    int32_t vr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) vr[r] = a.id_at(p0 + ti * 16 + 4 * fg + r);
#pragma unroll
    for (int ks = 0; ks < KMAX; ++ks)
      if (ks < ksteps) {
        const int c = ks * TK_KS + tj * 16 + frow;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (vr[r] != 0 && c < a.N) a.part[((size_t)vr[r] * a.splits + blockIdx.y) * a.N + c] = out[ks][r];
      }
  }
}

struct EngFinalArgs {
  CsrArgs named;            // offsets [V + 1], ids = named_user [n]; offsets null = no named terms
  const float* named_w;     // [n]
  size_t ld_out;
  float* out;               // [V, ld_out]
  float* out_mass;          // [V] or null
};

// One workgroup per news row, a thread per component (strided).  Row 0 is in no order: nothing was written for it.
__global__ __launch_bounds__(256) void expect_news_groups_final_kernel(EngArgs a, EngFinalArgs f) {
  const size_t v = blockIdx.x;
  const int slices = v == 0 ? 0 : a.splits;
  int32_t jb = 0, je = 0;
  if (f.named.offsets != nullptr) f.named.segment((long)v, jb, je);
  for (int c = threadIdx.x; c < a.N; c += blockDim.x) {
    double e = 0.0;
    for (int s = 0; s < slices; ++s) e += (double)a.part[(v * a.splits + s) * a.N + c];
    for (int32_t j = jb; j < je; ++j) {
      const float w = f.named_w[j];
      const int32_t u = f.named.ids[j];
      if (w == 0.f || u < 0 || u >= a.U) continue;
      const float tau = a.tau_of(u);
      if (!eng_tau_ok(tau)) continue;                         // the user only: under caps an emptied bin still has named terms
      const float x = a.user[(size_t)u * a.ld_user + c];
      const double it = a.scale_inv_tau ? (double)__fdiv_rn(1.f, tau) : 1.0;
      if (fabsf(x) < LZ_INF) e -= (double)w * it * (double)x;
    }
    f.out[v * f.ld_out + c] = (float)e;
  }
  if (threadIdx.x == 0 && f.out_mass != nullptr) {
    double m = 0.0;
    for (int s = 0; s < slices; ++s) m += a.pmass[v * a.splits + s];
    f.out_mass[v] = (float)m;
  }
}

// argument checks shared by the size query and the call; 0 = fine.  K18's of the shared fields in K18's order, K15's of the order
int expect_news_groups_check(const nr_expect_news_groups_desc* d) {
  NR_CHECK_ARG(d != nullptr, "score_expect_news_groups: null descriptor");
  NR_CHECK_RC(check_vectors("score_expect_news_groups", d->V, d->U, d->N));
  NR_CHECK_ARG(d->n_excl >= 0, "score_expect_news_groups: n_excl = %d entries of excl_users, must be >= 0", d->n_excl);
  NR_CHECK_ARG(d->n_excl == 0 || d->excl_users == nullptr || d->excl_offsets != nullptr,
               "score_expect_news_groups: excl_users given without excl_offsets (n_excl = %d; the two come together)", d->n_excl);
  NR_CHECK_ARG(d->n_excl == 0 || d->excl_offsets == nullptr || d->excl_users != nullptr,
               "score_expect_news_groups: excl_offsets given without excl_users (n_excl = %d; the two come together)", d->n_excl);
  NR_CHECK_ARG(d->tau_u != nullptr || (d->tau > 0.f && d->tau < LZ_INF),
               "score_expect_news_groups: tau = %g, a scalar temperature must be finite and > 0", (double)d->tau);
  NR_CHECK_ARG(d->n_groups >= 1 && d->n_groups <= NR_RANK_MAX_GROUPS, "score_expect_news_groups: n_groups = %d, must be in [1, %d]", d->n_groups,
               NR_RANK_MAX_GROUPS);
  NR_CHECK_ARG(d->n_pos >= TK_ROWS && d->n_pos % TK_ROWS == 0, "score_expect_news_groups: n_pos = %d positions, must be a positive multiple of %d",
               d->n_pos, TK_ROWS);
  const int nseg = eng_plan(d->V, d->U, d->N, 1).nseg;
  NR_CHECK_ARG(d->splits >= 0 && d->splits <= nseg,
               "score_expect_news_groups: splits = %d, must be 0 (library's choice) or in [1, %d], the segments of U = %d", d->splits, nseg, d->U);
  return check_pools("score_expect_news_groups", d->stamp, d->window, d->ld_window);
}

// the stream's instantiation for the run-time (tile, pool, lists); the tile fixes the k-slabs that can occur with it, as in K18
int expect_news_groups_stream_launch(int TV, bool pool, bool lists, dim3 grid, size_t smem, hipStream_t s, const EngArgs& a, const CsrArgs& ca) {
  return with_bool(pool, [&](auto p) {
    return with_bool(lists, [&](auto l) {
      constexpr bool P = decltype(p)::value, L = decltype(l)::value;
      if (TV == 64) return launch_lds(expect_news_groups_stream_kernel<4, 11, P, L>, grid, dim3(TK_THREADS), smem, s, a, ca);
      if (TV == 32) return launch_lds(expect_news_groups_stream_kernel<2, 26, P, L>, grid, dim3(TK_THREADS), smem, s, a, ca);
      return launch_lds(expect_news_groups_stream_kernel<1, NR_TOPK_MAX_N / TK_KS, P, L>, grid, dim3(TK_THREADS), smem, s, a, ca);
    });
  });
}

}  // namespace

extern "C" {

size_t nr_score_expect_news_groups_workspace_bytes(const nr_expect_news_groups_desc* d) {
  if (expect_news_groups_check(d) != NR_OK) return 0;
  return eng_carve(nullptr, d->V, eng_plan(d->V, d->U, d->N, d->splits).splits, d->N, nullptr);
}

int nr_score_expect_news_groups(const nr_expect_news_groups_desc* d, nr_stream_t stream) {
  NR_CHECK_RC(expect_news_groups_check(d));
  NR_CHECK_ARG(d->news_vecs && d->user && d->order && d->bin_start && d->base_max && d->base_logsum && d->bin_w && d->out,
               "score_expect_news_groups: null pointer (news_vecs, user, order, bin_start, base_max, base_logsum, bin_w, out)");
  NR_CHECK_ARG(d->ld_bin >= d->U, "score_expect_news_groups: bin-major row stride ld_bin = %d < U = %d", d->ld_bin, d->U);
  const bool named_all = d->named_offsets && d->named_user && d->named_w, named_any = d->named_offsets || d->named_user || d->named_w;
  NR_CHECK_ARG(named_all || !named_any, "score_expect_news_groups: named_offsets, named_user and named_w come together (all three or none)");
  NR_CHECK_ARG(d->n_named >= 0, "score_expect_news_groups: n_named = %d named terms, must be >= 0", d->n_named);
  NR_CHECK_RC(check_rows("score_expect_news_groups", d->news_vecs, d->ld_news, d->user, d->ld_user, d->N));
  NR_CHECK_ARG(d->ld_out >= d->N && (((uintptr_t)d->out) & 15) == 0,
               "score_expect_news_groups: out must be 16-byte aligned with ld_out = %d >= N = %d", d->ld_out, d->N);
  NR_CHECK_RC(check_workspace("score_expect_news_groups", d->ws, d->ws_bytes, nr_score_expect_news_groups_workspace_bytes(d)));
  NR_DEVICE_GUARD(stream, d->news_vecs);
  hipStream_t s = (hipStream_t)stream;
  const LogzPlan pl = eng_plan(d->V, d->U, d->N, d->splits);
  EngArgs a;
  a.news = d->news_vecs; a.user = d->user;
  a.ld_news = (size_t)d->ld_news; a.ld_user = (size_t)d->ld_user; a.ld_bin = (size_t)d->ld_bin;
  a.V = d->V; a.U = d->U; a.N = d->N; a.seg = pl.seg; a.nseg = pl.nseg; a.segs_per = pl.segs_per; a.splits = pl.splits;
  a.n_pos = d->n_pos; a.n_bins = d->n_groups + 1;
  a.order = d->order; a.bin_start = d->bin_start;
  a.pool = pool_args(d->prior, d->stamp, d->window, d->ld_window);
  a.tau = d->tau; a.tau_u = d->tau_u;
  a.base_max = d->base_max; a.base_logsum = d->base_logsum; a.bin_w = d->bin_w;
  a.scale_inv_tau = d->scale_inv_tau;
  eng_carve(d->ws, d->V, pl.splits, d->N, &a);
  const CsrArgs ca = csr_args(d->excl_offsets, d->excl_users, d->n_excl);
  {
    const int TV = pl.TU;
    const size_t smem = tk_tile_bytes(TV, d->N) + TV * ENG_PER_ROW;
    const dim3 grid((unsigned)(d->n_pos / TV), (unsigned)pl.splits);
    NrProfScope ps(s, "expect_news_groups_stream[V=%d,U=%d,N=%d,TV=%d,splits=%d,seg=%d,pos=%d,pool=%d,lists=%d]", d->V, d->U, d->N, TV, pl.splits,
                   pl.seg, d->n_pos, a.pool.any() ? 1 : 0, ca.offsets != nullptr ? 1 : 0);
    NR_CHECK_RC(expect_news_groups_stream_launch(TV, a.pool.any(), ca.offsets != nullptr, grid, smem, s, a, ca));
  }
  NR_CHECK_LAUNCH();
  {
    EngFinalArgs f;
    f.named = csr_args(named_all ? d->named_offsets : nullptr, d->named_user, d->n_named);
    f.named_w = d->named_w;
    f.ld_out = (size_t)d->ld_out;
    f.out = d->out; f.out_mass = d->out_mass;
    NrProfScope ps(s, "expect_news_groups_final[V=%d,N=%d,splits=%d,named=%d]", d->V, d->N, pl.splits, f.named.n);
    hipLaunchKernelGGL(expect_news_groups_final_kernel, dim3((unsigned)d->V), dim3(256), 0, s, a, f);
  }
  NR_CHECK_LAUNCH();
  return NR_OK;
}

}  // extern "C"
