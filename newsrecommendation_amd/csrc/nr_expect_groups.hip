// The expected news vector per bin under per-(user, bin) weights (include/nrhip.h, K20): the gradient of K15's per-group
// log-partitions, out[u] = sum_b omega[u, b] E_{u,b} - sum_t sub_w[u, t] news[sub_ids[u, t]], E_{u,b} the softmax mean INSIDE
// bin b on K15's base of that bin.  expect_stream_kernel of nr_expect.hip over the group-major order logzg_stream_kernel of
// nr_logz_groups.hip streams over: scores and eligibility come from score_key / pool_key and the list cursor of
// nr_logz_stream.h in position space, so a news has weight 0 here exactly when it is no term of its bin's K15 sum.
//
//   expect_groups_stream_kernel<MT, KMAX, POOL, LISTS>   per chunk of 128 positions (rows order[vc ..], ScoreOrderedRows):
//                           1. the scoring tile, put_scores;
//                           2. a wave owns TU / 8 users and turns each one's 128 scores into fl(omega * p), p = expf(fmaf(s -
//                              gmax, 1 / tau, -logsum)) against the user's base OF THE CHUNK'S BIN -- 0 where the position is
//                              padding, not eligible, or omega == 0 -- into P; the lane adds the exact products to a fp64 mass;
//                           3. the chunk's k-slabs a second time through the same staging buffers (the same rows by order[],
//                              L2-hot) and out[TU, N] += P[TU, 128] . rows[128, N] on v_mfma_f32_16x16x4_f32 as in K17.
//                           A segment never straddles two bins: when the segment leaves the bin, the wave reloads (gmax,
//                           -logsum, omega) of its users for the new bin (a clamped search of bin_seg).  Accumulators stay in
//                           registers for the whole slice; one [N] partial and one mass per (user, slice).
//   expect_groups_final_kernel   expect_final_kernel: one workgroup per user, the non-empty slices ascending in fp64, minus
//                           the named rows (fp64, t ascending), times 1 / tau, rounded to fp32 once.
//
// Slices are K15's: slice y of s takes the segments that start in [y n_pos / s, (y + 1) n_pos / s); with as many slices as
// segments slice y is segment y.  The plan and the table reads below are lg_plan's and LogzgArgs' of nr_logz_groups.hip, copied:
// that unit's kernels keep the instruction streams they have.  The chain of one (user, component) is K17's, over the slice's
// chunks in position order; which wave holds what is fixed by N alone, so no user's bits depend on another's.
#include <math.h>

#include "nr_logz_stream.h"

namespace {

constexpr int EG_MAX_SEGS = 256;            // K15's: segments the chunk budget is cut into; every bin may add a short one
constexpr size_t EG_PER_USER = TK_LDS_TILE * sizeof(float);   // a user's row of P, as in K17

struct EgPlan {
  int TU, splits;
};
// lg_plan's rule with K17's user tile
inline EgPlan eg_plan(int U, int V, int N, int nseg, int splits) {
  EgPlan p;
  p.TU = score_user_tile(N, EG_PER_USER);
  long s = splits > 0 ? splits : score_auto_splits(U, V, p.TU, nseg);
  if (s > nseg) s = nseg;
  if (s < 1) s = 1;
  p.splits = (int)s;
  return p;
}

struct EgArgs {
  const float* news;
  const float* user;
  size_t ld_news, ld_user, ld_base;
  int V, U, N, nseg, n_pos, n_bins, splits;
  const int32_t* order;     // [n_pos]
  const int32_t* seg_start; // [nseg + 1]
  const int32_t* bin_seg;   // [n_bins + 1]
  PoolArgs pool;            // read by the POOL instantiations only; indexed by news id
  float tau;
  const float* tau_u;
  const float* base_max;    // [U, ld_base]
  const float* base_logsum; // [U, ld_base]
  const float* bin_w;       // [U, ld_base]
  float* part;              // [U, splits, N] partial rows
  double* pmass;            // [U, splits] partial masses
  __device__ __forceinline__ float tau_of(long u) const { return tau_u != nullptr ? tau_u[u] : tau; }
  // a position read from the segment table, clamped into [0, n_pos]
  __device__ __forceinline__ long start_of(int sg) const {
    const int32_t p = seg_start[sg];
    return p < 0 ? 0 : (p > n_pos ? n_pos : p);
  }
  // the first segment that starts at or after position p, nseg if none; stays in [0, nseg] whatever the table holds
  __device__ __forceinline__ int first_from(long p) const {
    int lo = 0, hi = nseg;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (start_of(mid) < p) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  }
  // the segments [s_lo, s_hi) and positions [v_lo, v_hi) of slice y; false = the slice is empty (stream and finalize agree)
  __device__ __forceinline__ bool slice(int y, int& s_lo, int& s_hi, long& v_lo, long& v_hi) const {
    const bool one = splits == nseg;
    s_lo = one ? y : first_from((long)y * n_pos / splits);
    s_hi = one ? s_lo + 1 : y + 1 == splits ? nseg : first_from((long)(y + 1) * n_pos / splits);
    v_lo = v_hi = 0;
    if (s_lo >= s_hi) return false;
    v_lo = start_of(s_lo);
    v_hi = start_of(s_hi);
    return v_lo < v_hi;
  }
  // the bin that owns segment sg: the first b with bin_seg[b + 1] > sg, clamped into [0, n_bins - 1]; seg_hi = where it ends
  __device__ __forceinline__ int bin_of(int sg, int& seg_hi) const {
    int lo = 0, hi = n_bins - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (bin_seg[mid + 1] <= sg) lo = mid + 1;
      else hi = mid;
    }
    seg_hi = bin_seg[lo + 1];
    return lo;
  }
};
// workspace: the masses first (8-byte aligned), then the partial rows
inline size_t eg_carve(void* ws, int U, int splits, int N, EgArgs* a) {
  char* p = reinterpret_cast<char*>(ws);
  const size_t n = (size_t)U * splits;
  if (a) {
    a->pmass = reinterpret_cast<double*>(p);
    a->part = reinterpret_cast<float*>(p + n * 8);
  }
  return (n * 8 + n * (size_t)N * 4 + 7) & ~(size_t)7;
}

// ex_clean of nr_expect.hip: a component that is not finite counts as 0
__device__ __forceinline__ void eg_clean(f32x4& g) {
#pragma unroll
  for (int e = 0; e < 4; ++e) g[e] = fabsf(g[e]) < LZ_INF ? g[e] : 0.f;
}

template <int MT, int KMAX, bool POOL, bool LISTS>
__global__ __launch_bounds__(TK_THREADS) void expect_groups_stream_kernel(EgArgs a, CsrArgs ca) {
  constexpr int TU = 16 * MT, PER_WAVE = TU / TK_WAVES;
  constexpr int PAIRS = 2 * MT, PARTS = TK_WAVES / PAIRS, PART_ROWS = TK_ROWS / PARTS, STEPS = PART_ROWS / 16;
  static_assert(PAIRS * PARTS == TK_WAVES && STEPS >= 1, "8 waves = pairs x row parts");
  extern __shared__ __attribute__((aligned(16))) float eg_smem[];
  ScoreTile<MT> t(eg_smem, a.N);
  float* sP = t.end();                                        // [TU, TK_LDS_TILE] the chunk's weights
  const int lane = t.lane, wave = __builtin_amdgcn_readfirstlane(t.wave);   // uniform: what is per user stays in scalar registers
  const int u0 = blockIdx.x * TU;
  int s_lo, s_hi;
  long v_lo, v_hi;
  if (!a.slice((int)blockIdx.y, s_lo, s_hi, v_lo, v_hi)) return;   // the whole workgroup; the finalize skips the slice too
  const int ksteps = t.ksteps;                                // <= KMAX by the launch's choice of instantiation

  t.load_users(a.user, a.ld_user, u0, a.U);
  // user wave + 8 i of the tile: 1 / tau; the base and omega of the CURRENT bin; this lane's running mass
  float it[PER_WAVE], bm[PER_WAVE], nbl[PER_WAVE], om[PER_WAVE];
  bool live[PER_WAVE];
  double mass[PER_WAVE];
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int u = u0 + wave + TK_WAVES * i;
    it[i] = __fdiv_rn(1.f, u < a.U ? a.tau_of(u) : 1.f);
    bm[i] = -LZ_INF;
    nbl[i] = 0.f;
    om[i] = 0.f;
    live[i] = false;
    mass[i] = 0.0;
  }
  // LISTS: the cursor of every user of the wave = the first entry (a position) of its list that is >= v_lo
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

  // the second contraction: this wave's (user tile, column tile) pair and its part of the chunk's rows
  const int pair = wave % PAIRS, part = wave / PAIRS;
  const int ti = pair >> 1, tj = pair & 1, rbase = part * PART_ROWS;
  const int frow = lane & 15, fg = lane >> 4;
  f32x4 out[KMAX];
#pragma unroll
  for (int ks = 0; ks < KMAX; ++ks) out[ks] = (f32x4){0.f, 0.f, 0.f, 0.f};

  int sg = s_lo;                                              // the segment the chunk at vc lies in, and where it ends
  long sg_end = a.start_of(sg + 1);
  int bin_hi = s_lo;                                          // the current bin owns the segments below bin_hi: none yet
  ScoreOrderedRows rows = {a.news, a.ld_news, a.order, a.V, v_hi, 0, 0};
  rows.seek(v_lo, t.srow);
  t.load_slab(rows, 0);
  for (long vc = v_lo; vc < v_hi; vc += TK_ROWS) {
    if (sg >= bin_hi) {
      // the bin changed: (gmax, -logsum, omega) of the wave's users for the segment's bin.  No weights for a user beyond U, one
      // the finalize answers with NaN, an empty bin, or omega == 0
      const int b = a.bin_of(sg, bin_hi);
      if (bin_hi <= sg) bin_hi = sg + 1;                      // whatever the table holds, the search is not repeated within a segment
#pragma unroll
      for (int i = 0; i < PER_WAVE; ++i) {
        const int u = u0 + wave + TK_WAVES * i;
        const size_t at = (size_t)(u < a.U ? u : 0) * a.ld_base + b;
        const float tau = u < a.U ? a.tau_of(u) : 0.f;
        bm[i] = u < a.U ? a.base_max[at] : -LZ_INF;
        nbl[i] = u < a.U ? -a.base_logsum[at] : 0.f;
        om[i] = u < a.U ? a.bin_w[at] : 0.f;
        live[i] = tau > 0.f && tau < LZ_INF && om[i] != 0.f && fabsf(om[i]) < LZ_INF && fabsf(bm[i]) < LZ_INF && nbl[i] == nbl[i];
      }
    }
    f32x4 acc[MT];
    t.chunk(rows, acc);
    t.load_slab(rows, 0);                                     // the same chunk again: in flight while the weights are formed
    // the ids of the chunk's 128 positions, two per lane; POOL: their prior and stamp, gathered by id
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
      // eligible as in logzg_stream_kernel: a real news (not padding), key != 0, not listed
      const bool el0 = live[i] && r0 && k0 != 0u && ((l0 >> lane) & 1ull) == 0ull;
      const bool el1 = live[i] && r1 && k1 != 0u && ((l1 >> lane) & 1ull) == 0ull;
      // p as in K17; the pair's weight is ONE more fp32 multiply, the mass takes the exact product
      const float d0 = key_score(k0) - bm[i], d1 = key_score(k1) - bm[i];
      const float q0 = el0 ? expf(d0 == 0.f ? nbl[i] : fmaf(d0, it[i], nbl[i])) : 0.f;
      const float q1 = el1 ? expf(d1 == 0.f ? nbl[i] : fmaf(d1, it[i], nbl[i])) : 0.f;
      sP[ul * TK_LDS_TILE + lane] = el0 ? __fmul_rn(om[i], q0) : 0.f;
      sP[ul * TK_LDS_TILE + lane + 64] = el1 ? __fmul_rn(om[i], q1) : 0.f;
      mass[i] += (el0 ? (double)om[i] * (double)q0 : 0.0) + (el1 ? (double)om[i] * (double)q1 : 0.0);
    }
    __syncthreads();                                          // P is whole; the score tile is the staging buffer again

    // the wave's fragment of P: pa[s][e] = weight of user ti * 16 + frow for chunk row rbase + 16 s + 4 fg + e
    f32x4 pa[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) pa[s] = *reinterpret_cast<const f32x4*>(sP + (ti * 16 + frow) * TK_LDS_TILE + rbase + 16 * s + 4 * fg);
    eg_clean(t.g0);
    eg_clean(t.g1);
    t.store_slab(0);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < KMAX; ++ks) {
      if (ks < ksteps) {
        if (ks + 1 < ksteps) t.load_slab(rows, ks + 1);
        else if (vc + TK_ROWS < v_hi) {                       // the next chunk's first slab, for ScoreTile::chunk
          rows.seek(vc + TK_ROWS, t.srow);
          t.load_slab(rows, 0);
        }
        const float* pb = t.sB + (size_t)(ks & 1) * TK_ROWS * TK_LDB + (rbase + 4 * fg) * TK_LDB + tj * 16 + frow;
#pragma unroll
        for (int s = 0; s < STEPS; ++s)
#pragma unroll
          for (int e = 0; e < 4; ++e) out[ks] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[s][e], pb[(16 * s + e) * TK_LDB], out[ks], 0, 0, 0);
        if (ks + 1 < ksteps) {
          eg_clean(t.g0);
          eg_clean(t.g1);
          t.store_slab((ks + 1) & 1);
        }
        __syncthreads();
      }
    }
    // segment end: sg stays inside the slice whatever the table holds
    if (vc + TK_ROWS >= sg_end && sg + 1 < s_hi) {
      ++sg;
      sg_end = a.start_of(sg + 1);
    }
  }

  // slice end.  The mass: one partial per (user, slice)
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int u = u0 + wave + TK_WAVES * i;
    const double m = wave_sum_d(mass[i]);
    if (lane == 0 && u < a.U) a.pmass[(size_t)u * a.splits + blockIdx.y] = m;
  }
  // The rows, as in expect_stream_kernel: the row parts added in ascending order through the user vectors' LDS
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

struct EgFinalArgs {
  const int32_t* sub_ids;   // [U, ld_sub] or null
  const float* sub_w;
  size_t ld_sub, ld_out;
  int T, scale_inv_tau;
  float* out;
  float* out_mass;          // [U] or null
};

// One workgroup per user, a thread per component (strided).  A slice that streamed nothing wrote nothing and is skipped.
__global__ __launch_bounds__(256) void expect_groups_final_kernel(EgArgs a, EgFinalArgs f) {
  const size_t u = blockIdx.x;
  const float tau = a.tau_of(u);
  const bool tau_ok = tau > 0.f && tau < LZ_INF;
  // NaN for the user: a non-empty bin (gmax != -inf) under a bad temperature, or one with omega != 0 and a base or omega the
  // stream forms no weights from
  int bad = 0;
  for (int b = threadIdx.x; b < a.n_bins; b += blockDim.x) {
    const float bm = a.base_max[u * a.ld_base + b], bl = a.base_logsum[u * a.ld_base + b], om = a.bin_w[u * a.ld_base + b];
    if (bm != -LZ_INF && (!tau_ok || (om != 0.f && (!(fabsf(om) < LZ_INF) || !(bm < LZ_INF) || bl != bl)))) bad = 1;
  }
  // which slices streamed something: the stream's own rule, once per workgroup
  __shared__ unsigned char wrote[EG_MAX_SEGS + NR_RANK_MAX_GROUPS + 1];
  for (int s = threadIdx.x; s < a.splits; s += blockDim.x) {
    int s_lo, s_hi;
    long v_lo, v_hi;
    wrote[s] = a.slice(s, s_lo, s_hi, v_lo, v_hi) ? 1 : 0;
  }
  bad = __syncthreads_or(bad);
  const double it = f.scale_inv_tau ? (double)__fdiv_rn(1.f, tau) : 1.0;
  for (int c = threadIdx.x; c < a.N; c += blockDim.x) {
    double e = 0.0;
    for (int s = 0; s < a.splits; ++s)
      if (wrote[s]) e += (double)a.part[(u * a.splits + s) * a.N + c];
    if (f.sub_ids != nullptr)
      for (int j = 0; j < f.T; ++j) {
        const int32_t id = f.sub_ids[u * f.ld_sub + j];
        if (id >= 1 && id < a.V) e -= (double)f.sub_w[u * f.ld_sub + j] * (double)a.news[(size_t)id * a.ld_news + c];
      }
    f.out[u * f.ld_out + c] = bad ? __builtin_nanf("") : (float)(e * it);
  }
  if (threadIdx.x == 0 && f.out_mass != nullptr) {
    double m = 0.0;
    for (int s = 0; s < a.splits; ++s)
      if (wrote[s]) m += a.pmass[u * a.splits + s];
    f.out_mass[u] = bad ? __builtin_nanf("") : (float)m;
  }
}

// argument checks shared by the size query and the call; 0 = fine.  K15's, in K15's order
int expect_groups_check(const nr_expect_groups_desc* d) {
  NR_CHECK_ARG(d != nullptr, "score_expect_groups: null descriptor");
  NR_CHECK_RC(check_vectors("score_expect_groups", d->V, d->U, d->N));
  NR_CHECK_RC(check_lists("score_expect_groups", 0, d->excl_offsets, d->excl_ids, d->n_excl));
  NR_CHECK_ARG(d->tau_u != nullptr || (d->tau > 0.f && d->tau < LZ_INF),
               "score_expect_groups: tau = %g, a scalar temperature must be finite and > 0", (double)d->tau);
  NR_CHECK_ARG(d->n_groups >= 1 && d->n_groups <= NR_RANK_MAX_GROUPS, "score_expect_groups: n_groups = %d, must be in [1, %d]", d->n_groups,
               NR_RANK_MAX_GROUPS);
  NR_CHECK_ARG(d->n_pos >= TK_ROWS && d->n_pos % TK_ROWS == 0, "score_expect_groups: n_pos = %d positions, must be a positive multiple of %d",
               d->n_pos, TK_ROWS);
  NR_CHECK_ARG(d->nseg >= 1 && d->nseg <= EG_MAX_SEGS + d->n_groups + 1 && d->nseg <= d->n_pos / TK_ROWS,
               "score_expect_groups: nseg = %d segments, must be in [1, %d] and at most the %d chunks", d->nseg, EG_MAX_SEGS + d->n_groups + 1,
               d->n_pos / TK_ROWS);
  NR_CHECK_ARG(d->splits >= 0 && d->splits <= d->nseg, "score_expect_groups: splits = %d, must be 0 (library's choice) or in [1, %d], the segments",
               d->splits, d->nseg);
  return check_pools("score_expect_groups", d->stamp, d->window, d->ld_window);
}

// the stream's instantiation for the run-time (tile, pool, lists); the tile fixes the k-slabs that can occur with it, as in K17
int expect_groups_stream_launch(int TU, bool pool, bool lists, dim3 grid, size_t smem, hipStream_t s, const EgArgs& a, const CsrArgs& ca) {
  return with_bool(pool, [&](auto p) {
    return with_bool(lists, [&](auto l) {
      constexpr bool P = decltype(p)::value, L = decltype(l)::value;
      if (TU == 64) return launch_lds(expect_groups_stream_kernel<4, 11, P, L>, grid, dim3(TK_THREADS), smem, s, a, ca);
      if (TU == 32) return launch_lds(expect_groups_stream_kernel<2, 26, P, L>, grid, dim3(TK_THREADS), smem, s, a, ca);
      return launch_lds(expect_groups_stream_kernel<1, NR_TOPK_MAX_N / TK_KS, P, L>, grid, dim3(TK_THREADS), smem, s, a, ca);
    });
  });
}

}  // namespace

extern "C" {

size_t nr_score_expect_groups_workspace_bytes(const nr_expect_groups_desc* d) {
  if (expect_groups_check(d) != NR_OK) return 0;
  return eg_carve(nullptr, d->U, eg_plan(d->U, d->V, d->N, d->nseg, d->splits).splits, d->N, nullptr);
}

int nr_score_expect_groups(const nr_expect_groups_desc* d, nr_stream_t stream) {
  NR_CHECK_RC(expect_groups_check(d));
  NR_CHECK_ARG(d->news_vecs && d->user && d->order && d->seg_start && d->bin_seg && d->base_max && d->base_logsum && d->bin_w && d->out,
               "score_expect_groups: null pointer (news_vecs, user, order, seg_start, bin_seg, base_max, base_logsum, bin_w, out)");
  NR_CHECK_ARG(d->ld_base >= d->n_groups + 1, "score_expect_groups: base row stride %d < n_groups + 1 = %d", d->ld_base, d->n_groups + 1);
  NR_CHECK_ARG(d->sub_ids == nullptr || d->sub_w != nullptr, "score_expect_groups: sub_ids given without sub_w (the two come together)");
  NR_CHECK_ARG(d->sub_w == nullptr || d->sub_ids != nullptr, "score_expect_groups: sub_w given without sub_ids (the two come together)");
  NR_CHECK_ARG(d->sub_ids == nullptr || (d->T >= 1 && d->T <= NR_TOPK_MAX_K && d->ld_sub >= d->T),
               "score_expect_groups: T = %d named rows per user (row stride %d), must be in [1, %d] with ld_sub >= T", d->T, d->ld_sub,
               NR_TOPK_MAX_K);
  NR_CHECK_RC(check_rows("score_expect_groups", d->news_vecs, d->ld_news, d->user, d->ld_user, d->N));
  NR_CHECK_ARG(d->ld_out >= d->N && (((uintptr_t)d->out) & 15) == 0, "score_expect_groups: out must be 16-byte aligned with ld_out = %d >= N = %d",
               d->ld_out, d->N);
  NR_CHECK_RC(check_workspace("score_expect_groups", d->ws, d->ws_bytes, nr_score_expect_groups_workspace_bytes(d)));
  NR_DEVICE_GUARD(stream, d->news_vecs);
  hipStream_t s = (hipStream_t)stream;
  const EgPlan pl = eg_plan(d->U, d->V, d->N, d->nseg, d->splits);
  EgArgs a;
  a.news = d->news_vecs; a.user = d->user;
  a.ld_news = (size_t)d->ld_news; a.ld_user = (size_t)d->ld_user; a.ld_base = (size_t)d->ld_base;
  a.V = d->V; a.U = d->U; a.N = d->N; a.nseg = d->nseg; a.n_pos = d->n_pos; a.n_bins = d->n_groups + 1; a.splits = pl.splits;
  a.order = d->order; a.seg_start = d->seg_start; a.bin_seg = d->bin_seg;
  a.pool = pool_args(d->prior, d->stamp, d->window, d->ld_window);
  a.tau = d->tau; a.tau_u = d->tau_u;
  a.base_max = d->base_max; a.base_logsum = d->base_logsum; a.bin_w = d->bin_w;
  eg_carve(d->ws, d->U, pl.splits, d->N, &a);
  const CsrArgs ca = csr_args(d->excl_offsets, d->excl_ids, d->n_excl);
  {
    const int TU = pl.TU;
    const size_t smem = tk_tile_bytes(TU, d->N) + TU * EG_PER_USER;
    const dim3 grid((unsigned)((d->U + TU - 1) / TU), (unsigned)pl.splits);
    NrProfScope ps(s, "expect_groups_stream[U=%d,V=%d,N=%d,TU=%d,splits=%d,nseg=%d,pos=%d]", d->U, d->V, d->N, TU, pl.splits, d->nseg, d->n_pos);
    NR_CHECK_RC(expect_groups_stream_launch(TU, a.pool.any(), ca.offsets != nullptr, grid, smem, s, a, ca));
  }
  NR_CHECK_LAUNCH();
  {
    EgFinalArgs f;
    f.sub_ids = d->sub_ids; f.sub_w = d->sub_w;
    f.ld_sub = (size_t)d->ld_sub; f.ld_out = (size_t)d->ld_out;
    f.T = d->sub_ids != nullptr ? d->T : 0; f.scale_inv_tau = d->scale_inv_tau;
    f.out = d->out; f.out_mass = d->out_mass;
    NrProfScope ps(s, "expect_groups_final[U=%d,N=%d,splits=%d,T=%d]", d->U, d->N, pl.splits, f.T);
    hipLaunchKernelGGL(expect_groups_final_kernel, dim3((unsigned)d->U), dim3(256), 0, s, a, f);
  }
  NR_CHECK_LAUNCH();
  return NR_OK;
}

}  // extern "C"
