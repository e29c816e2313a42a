// K11  nr_mmr_select: Maximal Marginal Relevance re-ranking of a pool of the M best (include/nrhip.h).  One launch, one
// workgroup of 4 waves per user, no workspace.
//
// Phase 1: the Gram matrix g(i, j) = <x_i, x_j> of the pool's M news vectors on v_mfma_f32_32x32x2_f32 (exact fp32: one fmaf
// chain per pair).  The rows are gathered by id and streamed in k-slabs of 32 columns through two LDS stages (the next slab
// waits in registers while this one is contracted); the Mp x Mp result (Mp = 32 * MB, MB = ceil(M / 32)) stays in the
// accumulators: g is symmetric, so only the MB (MB + 1) / 2 tiles of 32 x 32 on and above the diagonal are formed (the mirror
// tile is written from the same registers); tile t = wave + 4 q of them belongs to wave `wave`, at most 3 tiles = 48
// accumulator registers a lane at MB = 4.  One (i, j) pair is ONE chain in the order (slab, q, e, lane half h): column 32 slab + 8 q + 4 h + e,
// whatever the tile, M, the place or the user; g(i, j) and g(j, i) contract the same products in the same order and are equal
// bit for bit.  A place that is not live contributes a row of zeros and its id is never turned into an address.
// Phase 2: the finished Gram goes to LDS (over the stages) and wave 0 walks: two places a lane; per step a wave-wide max of the
// values' order-preserving keys (score_key), the lowest place that reaches it (two ballots), then row j of the Gram updates
// maxsim.
#include "nr_score_tile.h"

namespace {

constexpr int MM_THREADS = 256;
constexpr int MM_WAVES = 4;
constexpr int MM_KS = 32;            // columns per k-slab
constexpr int MM_LDB = MM_KS + 4;    // slab row stride: the 32 rows of a fragment read land in different 4-bank groups
constexpr int MM_MAXP = NR_TOPK_MAX_K;

__host__ __device__ constexpr int mm_ldg(int MB) { return 32 * MB + 4; }   // Gram row stride
__host__ __device__ constexpr int mm_region_floats(int MB) {
  return 2 * 32 * MB * MM_LDB > 32 * MB * mm_ldg(MB) ? 2 * 32 * MB * MM_LDB : 32 * MB * mm_ldg(MB);
}
// g is symmetric bit for bit, so only the tiles (bi, bj) with bi <= bj are formed: entry t of the table, 4 bits (bi << 2 | bj),
// row-major over the upper triangle
__host__ __device__ constexpr u64 mm_tri_table(int MB) {
  u64 tab = 0;
  int t = 0;
  for (int bi = 0; bi < MB; ++bi)
    for (int bj = bi; bj < MB; ++bj) tab |= (u64)(bi << 2 | bj) << (4 * t++);
  return tab;
}
inline size_t mm_lds_bytes(int MB) { return (size_t)(MM_MAXP + mm_region_floats(MB)) * 4; }

struct MmrArgs {
  const float* news;
  const int32_t* pool_ids;
  const float* pool_scores;
  const float* penalty_u;
  const int32_t* group;
  int32_t* out_ids;
  float* out_scores;
  int32_t* out_place;
  size_t ld_news, ld_ids, ld_scores;
  int V, N, M, k, cap;
  float penalty;
};

// max over the wave on the DPP path: an inclusive max-scan along each row of 16 lanes, then lane 15 of a row into the next
// row (row_bcast:15, rows 1 and 3) and lane 31 into rows 2 and 3 (row_bcast:31); lane 63 holds the result.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_max_step(uint32_t v) {
  const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xf, false);   // no source lane: v itself
  return o > v ? o : v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  v = dpp_max_step<0x111, 0xf>(v);   // row_shr:1
  v = dpp_max_step<0x112, 0xf>(v);   // row_shr:2
  v = dpp_max_step<0x114, 0xf>(v);   // row_shr:4
  v = dpp_max_step<0x118, 0xf>(v);   // row_shr:8
  v = dpp_max_step<0x142, 0xa>(v);   // row_bcast:15
  v = dpp_max_step<0x143, 0xc>(v);   // row_bcast:31
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

template <int MB>
__global__ __launch_bounds__(MM_THREADS) void mmr_select_kernel(MmrArgs a) {
  constexpr int MP = 32 * MB;
  constexpr int NTRI = MB * (MB + 1) / 2;                   // tiles on and above the diagonal
  constexpr int NT = (NTRI + MM_WAVES - 1) / MM_WAVES;      // tiles per wave, at most
  constexpr u64 TRI = mm_tri_table(MB);
  constexpr int LDG = mm_ldg(MB);
  extern __shared__ __align__(16) float smem[];
  int32_t* sId = reinterpret_cast<int32_t*>(smem);           // [MM_MAXP] id of a live place, 0 otherwise
  float* sB = smem + MM_MAXP;                                // [2, MP, MM_LDB] slabs | [MP, LDG] Gram
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t u = blockIdx.x;
  const int M = a.M, N = a.N;

  if (tid < MM_MAXP) {
    int32_t id = 0;
    if (tid < M) {
      id = a.pool_ids[u * a.ld_ids + tid];
      const float r = a.pool_scores[u * a.ld_scores + tid];
      if (!(id >= 1 && id < a.V && r == r)) id = 0;
    }
    sId[tid] = id;
  }
  __syncthreads();

  // staging: thread -> rows (tid >> 3) + 32 q of the pool, columns 4 (tid & 7) .. + 3 of the slab
  const int srow = tid >> 3, scol = (tid & 7) * 4;
  const float* rowp[MB];
#pragma unroll
  for (int q = 0; q < MB; ++q) {
    const int32_t id = sId[srow + 32 * q];
    rowp[q] = id > 0 ? a.news + (size_t)id * a.ld_news : nullptr;
  }
  f32x4 g[MB];
  auto load_slab = [&](int ks) {
    const int c = ks * MM_KS + scol;
#pragma unroll
    for (int q = 0; q < MB; ++q) {
      g[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (c < N && rowp[q] != nullptr) g[q] = *reinterpret_cast<const f32x4*>(rowp[q] + c);
    }
  };
  auto store_slab = [&](int buf) {
    float* d = sB + (size_t)buf * MP * MM_LDB + srow * MM_LDB + scol;
#pragma unroll
    for (int q = 0; q < MB; ++q) *reinterpret_cast<f32x4*>(d + 32 * q * MM_LDB) = g[q];
  };

  f32x16 acc[NT];
  int ti[NT], tj[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const unsigned t = (unsigned)wave + MM_WAVES * q;
    ti[q] = (int)(TRI >> (4 * t + 2)) & 3; tj[q] = (int)(TRI >> (4 * t)) & 3;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
  }
  const int frow = lane & 31, fk = (lane >> 5) * 4;
  const int ksteps = (N + MM_KS - 1) / MM_KS;
  load_slab(0);
  store_slab(0);
  __syncthreads();
  for (int ks = 0; ks < ksteps; ++ks) {
    if (ks + 1 < ksteps) load_slab(ks + 1);
    const float* slab = sB + (size_t)(ks & 1) * MP * MM_LDB + frow * MM_LDB + fk;
#pragma unroll
    for (int q8 = 0; q8 < 4; ++q8) {
      f32x4 fa[NT], fb[NT];
#pragma unroll
      for (int q = 0; q < NT; ++q)
        if ((unsigned)wave + MM_WAVES * q < NTRI) {
          fa[q] = *reinterpret_cast<const f32x4*>(slab + ti[q] * 32 * MM_LDB + 8 * q8);
          fb[q] = *reinterpret_cast<const f32x4*>(slab + tj[q] * 32 * MM_LDB + 8 * q8);
        }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int q = 0; q < NT; ++q)
          if ((unsigned)wave + MM_WAVES * q < NTRI) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][e], fb[q][e], acc[q], 0, 0, 0);
    }
    if (ks + 1 < ksteps) store_slab((ks + 1) & 1);
    __syncthreads();
  }
  // the Gram over the stages (every wave is past its last slab read): row = place i of the A rows, column = place j
#pragma unroll
  for (int q = 0; q < NT; ++q)
    if ((unsigned)wave + MM_WAVES * q < NTRI) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = ti[q] * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), j = tj[q] * 32 + (lane & 31);
        sB[i * LDG + j] = acc[q][r];
        if (ti[q] != tj[q]) sB[j * LDG + i] = acc[q][r];       // the mirror tile
      }
    }
  __syncthreads();
  if (wave != 0) return;

  // ---- the walk: places lane and lane + 64 ----
  const float p = a.penalty_u != nullptr ? a.penalty_u[u] : a.penalty;
  const bool capped = a.group != nullptr;
  int32_t id[2], grp[2], cnt[2];
  float r[2], rn[2], maxsim[2];
  bool open[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int pl = lane + 64 * c;
    id[c] = sId[pl];
    open[c] = id[c] > 0;
    r[c] = open[c] ? a.pool_scores[u * a.ld_scores + pl] : -__builtin_inff();
    grp[c] = (open[c] && capped) ? a.group[id[c]] : -1;
    cnt[c] = 0;
    maxsim[c] = -__builtin_inff();
    const float gii = pl < MP ? sB[pl * LDG + pl] : 0.f;
    rn[c] = gii > 0.f ? __fdiv_rn(1.0f, __fsqrt_rn(gii)) : 0.f;
  }
  // The places taken go to LDS (over the ids, which are in registers by now) and the row is written in one coalesced pass.
  int32_t* sPl = sId;
  int t = 0;
  for (; t < a.k; ++t) {
    uint32_t key[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      key[c] = 0u;
      if (open[c] && (grp[c] < 0 || cnt[c] < a.cap)) {
        const uint32_t kv = score_key(t == 0 ? r[c] : __builtin_fmaf(-p, maxsim[c], r[c]));
        key[c] = kv > 1u ? kv : 1u;               // a candidate's key is never 0 (a NaN value: unspecified input, still a place)
      }
    }
    const uint32_t best = wave_max_u32(key[0] > key[1] ? key[0] : key[1]);
    if (best == 0u) break;                        // no candidate
    const u64 m0 = __ballot(key[0] == best), m1 = __ballot(key[1] == best);
    const int jc = m0 != 0 ? 0 : 1;               // ties: the lowest place
    const int jl = __builtin_ctzll(jc ? m1 : m0);
    const int j = jl + 64 * jc;                   // a place some lane offered: live, below M
    const int32_t gj = __builtin_amdgcn_readlane(jc ? grp[1] : grp[0], jl);
    const float rnj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(jc ? rn[1] : rn[0]), jl));
    if (lane == 0) sPl[t] = j;
    if (lane == jl) {
      if (jc) open[1] = false; else open[0] = false;
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int pl = lane + 64 * c;
      if (gj >= 0 && grp[c] == gj) ++cnt[c];
      const float gij = pl < MP ? sB[j * LDG + pl] : 0.f;
      const float s = __fmul_rn(__fmul_rn(gij, rn[c]), rnj);
      maxsim[c] = fmaxf(maxsim[c], s);
    }
  }
  for (int i = lane; i < a.k; i += 64) {
    const int pl = i < t ? sPl[i] : -1;
    a.out_ids[u * (size_t)a.k + i] = pl >= 0 ? a.pool_ids[u * a.ld_ids + pl] : 0;
    a.out_scores[u * (size_t)a.k + i] = pl >= 0 ? a.pool_scores[u * a.ld_scores + pl] : -__builtin_inff();
    a.out_place[u * (size_t)a.k + i] = pl;
  }
}

int mmr_check(const nr_mmr_desc* d) {
  NR_CHECK_ARG(d != nullptr, "mmr_select: null descriptor");
  NR_CHECK_ARG(d->M >= 1 && d->M <= NR_TOPK_MAX_K, "mmr_select: M = %d pool places, must be in [1, %d]", d->M, NR_TOPK_MAX_K);
  NR_CHECK_ARG(d->k >= 1 && d->k <= d->M, "mmr_select: k = %d, must be in [1, M = %d]", d->k, d->M);
  NR_CHECK_ARG(d->U >= 0, "mmr_select: U = %d users", d->U);
  NR_CHECK_ARG(d->V >= 1, "mmr_select: V = %d news rows", d->V);
  NR_CHECK_RC(check_width("mmr_select", d->N));
  NR_CHECK_ARG(d->penalty >= 0.f && d->penalty <= 3.402823466e38f, "mmr_select: penalty = %g, must be finite and >= 0",
               (double)d->penalty);
  NR_CHECK_ARG(d->group == nullptr || (d->group_cap >= 1 && d->group_cap <= NR_TOPK_MAX_K),
               "mmr_select: group given with group_cap = %d, the cap must be in [1, %d]", d->group_cap, NR_TOPK_MAX_K);
  NR_CHECK_ARG(d->group != nullptr || d->group_cap == 0, "mmr_select: group_cap = %d given without group (the two come together)", d->group_cap);
  NR_CHECK_ARG(d->news_vecs && d->pool_ids && d->pool_scores && d->out_ids && d->out_scores && d->out_place,
               "mmr_select: null pointer (news_vecs, pool_ids, pool_scores, out_ids, out_scores, out_place)");
  NR_CHECK_ARG(d->ld_news >= d->N && d->ld_news % 4 == 0 && (((uintptr_t)d->news_vecs) & 15) == 0,
               "mmr_select: rows must be 16-byte aligned (ld_news = %d: a multiple of 4, >= N = %d)", d->ld_news, d->N);
  NR_CHECK_ARG(d->ld_pool_ids >= d->M && d->ld_pool_scores >= d->M, "mmr_select: pool row strides %d / %d < M = %d", d->ld_pool_ids,
               d->ld_pool_scores, d->M);
  return NR_OK;
}

}  // namespace

extern "C" {

int nr_mmr_select(const nr_mmr_desc* d, nr_stream_t stream) {
  NR_CHECK_RC(mmr_check(d));
  if (d->U == 0) return NR_OK;
  NR_DEVICE_GUARD(stream, d->news_vecs);
  hipStream_t s = (hipStream_t)stream;
  MmrArgs a;
  a.news = d->news_vecs; a.pool_ids = d->pool_ids; a.pool_scores = d->pool_scores; a.penalty_u = d->penalty_u; a.group = d->group;
  a.out_ids = d->out_ids; a.out_scores = d->out_scores; a.out_place = d->out_place;
  a.ld_news = (size_t)d->ld_news; a.ld_ids = (size_t)d->ld_pool_ids; a.ld_scores = (size_t)d->ld_pool_scores;
  a.V = d->V; a.N = d->N; a.M = d->M; a.k = d->k; a.cap = d->group_cap; a.penalty = d->penalty;
  const int MB = (d->M + 31) / 32;
  const size_t smem = mm_lds_bytes(MB);
  {
    NrProfScope ps(s, "mmr_select[U=%d,N=%d,M=%d,k=%d]", d->U, d->N, d->M, d->k);
    NR_CHECK_RC(with_int<1, 2, 3, 4>(MB, [&](auto mb) {
      return launch_lds(mmr_select_kernel<decltype(mb)::value>, dim3((unsigned)d->U), dim3(MM_THREADS), smem, s, a);
    }));
  }
  NR_CHECK_LAUNCH();
  return NR_OK;
}

}  // extern "C"
