// The exact-fp32 scoring tile of the full-corpus passes and what every pass builds around it.  Its consumers: the top-k
// selection and the sampled selection (nr_topk.hip), the rank counting and its named passes (nr_rank.hip), the log-partition
// stream and the named rows of nr_row_logprob (nr_logz.hip), the expected news vector (nr_expect.hip: the tile followed by a
// second contraction over the chunk); nr_mmr.hip takes score_key and the width check only.  All of them
// must give one (u, v) pair the SAME bits -- "rank <= k", "is in the top-k row" and "is a term of the partition sum" are then
// one statement -- so there is ONE definition of the tile, of the keys, and of the rows a chunk is made of.
//
// A workgroup of 8 waves keeps TU = 16 * MT user vectors in LDS and takes news rows in chunks of 128 (k-slabs of 32 columns,
// double buffered through registers).  Wave w forms the [TU x 16] scores of chunk rows 16w .. 16w + 15 on
// v_mfma_f32_16x16x4_f32; one (u, v) score is ONE fmaf chain over the vector width in a fixed order (k-slab, sub-step e, MFMA
// k-group), whatever the tile, the place of the user in it, or the place of the news row in the chunk.  Where a chunk's rows
// come from is the caller's: a slice of the table (ScoreStreamRows) or rows gathered by id (ScoreNamedRows).
//
// The last section is host code: the argument checks, descriptor fills, plans and the launch helper the units share.
#pragma once
#include <type_traits>

#include "nr_common.h"

namespace {   // per including unit, as when the tile was nr_topk.hip's own: no name of it reaches other units

typedef unsigned long long u64;

constexpr int TK_THREADS = 512;
constexpr int TK_WAVES = TK_THREADS / 64;
constexpr int TK_ROWS = 128;        // news rows per chunk = 16 per wave
constexpr int TK_KS = 32;           // columns per k-slab
constexpr int TK_LDB = TK_KS + 4;   // slab row stride: 16 rows at one column land in 16 different 4-bank groups
constexpr int TK_LDS_TILE = TK_ROWS + 4;
constexpr int TK_STAGE_FLOATS = 2 * TK_ROWS * TK_LDB;   // two slabs; the score tile [TU, TK_LDS_TILE] lives in the same bytes
constexpr size_t TK_LDS_MAX = 160 * 1024;
constexpr int TK_CUS = 256;         // MI355X; the slice count is host arithmetic (the workspace size depends on it)

static_assert(64 * TK_LDS_TILE <= TK_STAGE_FLOATS, "score tile must fit the staging buffers");

__host__ __device__ inline int tk_npad(int N) { return (N + TK_KS - 1) / TK_KS * TK_KS; }
// LDS floats of the tile itself: the user vectors and the staging buffers
inline size_t tk_tile_floats(int TU, int N) { return (size_t)TU * (tk_npad(N) + 4) + TK_STAGE_FLOATS; }

// A score as an unsigned key: larger key = better score; NaN -> 0 ("nothing")
__device__ __forceinline__ uint32_t score_key(float s) {
  if (!(s == s)) return 0u;
  const uint32_t b = __float_as_uint(s + 0.0f);               // -0 -> +0: the two compare equal, so they share a key
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_score(uint32_t key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}
// A news as one 64-bit key: (score key) << 32 | ~id.  Larger = better; equal scores order by ascending id.
__device__ __forceinline__ u64 news_key(float score, uint32_t id) { return ((u64)score_key(score) << 32) | (uint32_t)~id; }
// lane j's 64-bit value, j the same in every lane
__device__ __forceinline__ u64 lane_u64(u64 v, int j) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, j), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), j);
  return ((u64)hi << 32) | lo;
}

// Pools (per-news prior, per-news stamp against a per-user window): the ONE place where a finished dot product becomes the
// final score of (u, v), as its key.  score = fl32(dot + prior): one separate fp32 add after the chain, never contracted into
// it (__fadd_rn).  Key 0 = not eligible: a prior of -inf (the global pool switch), a stamp outside [lo, hi] (lo > hi: nobody),
// or a NaN sum.  The selection, the counting stream and the named ids of the rank pass all come through here, so one (u, v)
// has one key everywhere; key_score() of it is the score that is returned.
__device__ __forceinline__ uint32_t pool_key(float dot, float prior, int32_t stamp, int32_t lo, int32_t hi) {
  const bool in = prior != -__builtin_inff() && stamp >= lo && stamp <= hi;
  return in ? score_key(__fadd_rn(dot, prior)) : 0u;
}
// The optional inputs of a pooled call and their neutral stand-ins: no prior = 0 (dot + 0 has dot's key), no stamps = every
// stamp 0 inside every window [0, 0].
struct PoolArgs {
  const float* prior;       // [V] or null
  const int32_t* stamp;     // [V] or null
  const int32_t* window;    // [U, ld_win] (lo, hi) or null; given exactly when stamp is
  size_t ld_win;
  __device__ __forceinline__ float prior_of(long v) const { return prior != nullptr ? prior[v] : 0.f; }
  __device__ __forceinline__ int32_t stamp_of(long v) const { return stamp != nullptr ? stamp[v] : 0; }
  __device__ __forceinline__ int32_t lo_of(long u) const { return window != nullptr ? window[(size_t)u * ld_win] : 0; }
  __device__ __forceinline__ int32_t hi_of(long u) const { return window != nullptr ? window[(size_t)u * ld_win + 1] : 0; }
  bool any() const { return prior != nullptr || stamp != nullptr || window != nullptr; }
};

// Sampled rows (include/nrhip.h, K12): the Gumbel noise of one (user key a, news id v) pair under (seed, draw), ONE definition
// for the selection (nr_score_sample), its finalize and the probe (nr_sample_noise).
//   bits = Philox4x32-10(counter = (v >> 2, a, draw, 0), key = (seed & 0xffffffff, seed >> 32))[v & 3]
//   u    = ((bits >> 8) + 0.5) * 2^-24, in [2^-25, 1 - 2^-25];   g = -log(-log(u))
// The counter holds the GLOBAL user key and news id, never a tile-, slice- or batch-local index, so a draw does not depend on
// where the pair falls.  Four consecutive news share one Philox block; every lane recomputes the block of its own pair.
// With m = bits >> 8, u = (2 m + 1) 2^-25 is a fp32 number only below 1/2 (2 m + 1 < 2^24); from 1/2 on it is 1 - u =
// (2^25 - 2 m - 1) 2^-25 that is one.  So -log(u) is logf of the exact u in the lower half and -log1pf of the exact -(1 - u) in
// the upper half: no rounding before the first logarithm, and u can never round to 1 (g would be +inf).  g is finite:
// -2.853 < g < 17.329.
__host__ __device__ inline uint32_t sample_bits(uint32_t a, uint32_t v, uint32_t seed_lo, uint32_t seed_hi, uint32_t draw) {
  uint32_t c0 = v >> 2, c1 = a, c2 = draw, c3 = 0u, k0 = seed_lo, k1 = seed_hi;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;   // hi and lo word of each product from one multiply
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const uint32_t w = v & 3u;
  return w == 0u ? c0 : w == 1u ? c1 : w == 2u ? c2 : c3;
}
__host__ __device__ inline float sample_gumbel(uint32_t bits) {
  const uint32_t m = bits >> 8;
  const float t = m < (1u << 23) ? -logf((float)(2u * m + 1u) * 0x1p-25f) : -log1pf(-((float)((1u << 25) - 2u * m - 1u) * 0x1p-25f));
  return -logf(t);
}
// No computed g reaches it (the largest, at bits >> 8 = 2^24 - 1, is 17.3287 to within a few ulp): the skip bound of sample_key.
constexpr float SAMPLE_G_MAX = 17.5f;

// fl32(tau * g) as a product of its own.  This unit is compiled with -ffp-contract=fast, under which __fmul_rn is a plain `*`
// that the compiler fuses with the add or subtract that follows into one v_fmac_f32; the empty asm makes the product opaque,
// at no instruction.  tests/test_gpu_sample.py sees a fused one as a 1-ulp score difference.
__device__ __forceinline__ float sample_scaled(float tau, float g) {
  float n = __fmul_rn(tau, g);
  asm volatile("" : "+v"(n));
  return n;
}

struct SampleArgs {
  uint32_t seed_lo, seed_hi, draw;
  float tau;                  // used when tau_u is null
  const float* tau_u;         // [U] or null
  const int32_t* user_keys;   // [U] or null: the row index
  __device__ __forceinline__ float tau_of(long u) const { return tau_u != nullptr ? tau_u[u] : tau; }
  __device__ __forceinline__ uint32_t key_of(long u) const { return user_keys != nullptr ? (uint32_t)user_keys[u] : (uint32_t)u; }
  __device__ __forceinline__ float gumbel(uint32_t a, uint32_t v) const { return sample_gumbel(sample_bits(a, v, seed_lo, seed_hi, draw)); }
};

// The key of a sampled call: pool_key fed the perturbed prior P(u, v) = fl32(prior + fl32(tau * g)) -- a multiply and an add of
// their own (sample_scaled, __fadd_rn: never one fma), the dot product chain untouched.  So a prior of -inf still switches a news
// off and a NaN still falls under the NaN rule; tau == 0 gives the keys of the plain call (prior + 0); and row u of a sampled
// call is row 0 of nr_score_topk for user u alone with prior = P(u, .), ids and score bits.  tau is finite and >= 0 here: the
// caller turns a user whose tau is not into an empty window.
// The skip: rounding is monotone and tau >= 0, so the key is at most kb, the key under g = SAMPLE_G_MAX.  A pair whose kb does
// not beat `thr` -- any value the user's threshold had, thresholds only rise -- can never be kept, and gets kb in place of its
// key without Philox or logarithms: no bit of any row changes.  pmax < inf keeps the bound honest where tau * SAMPLE_G_MAX
// overflows: dot = -inf would make NaN (key 0) of a pair whose true key is -inf's.
__device__ __forceinline__ uint32_t sample_key(float dot, float prior, int32_t stamp, int32_t lo, int32_t hi, float tau, const SampleArgs& sa,
                                               uint32_t a, uint32_t v, uint32_t thr) {
  const float pmax = __fadd_rn(prior, sample_scaled(tau, SAMPLE_G_MAX));
  const uint32_t kb = pool_key(dot, pmax, stamp, lo, hi);
  if (tau == 0.f || (kb <= thr && pmax < __builtin_inff())) return kb;
  return pool_key(dot, __fadd_rn(prior, sample_scaled(tau, sa.gumbel(a, v))), stamp, lo, hi);
}

// Exclusion lists of any length in CSR form (include/nrhip.h, K9): user u's list is ids[offsets[u] .. offsets[u + 1]), strictly
// ascending.  Read by the CSR instantiations only.  segment() clamps both bounds into [0, n] and keeps e >= b: whatever the
// offsets hold, no index formed from them leaves ids[0 .. n).
struct CsrArgs {
  const int32_t* offsets;   // [U + 1]
  const int32_t* ids;       // [n]
  int n;
  __device__ __forceinline__ void segment(long u, int32_t& b, int32_t& e) const {
    const int32_t x = offsets[u], y = offsets[u + 1];
    b = x < 0 ? 0 : (x > n ? n : x);
    e = y < b ? b : (y > n ? n : y);
  }
};

// chunk row r = news row vc + r of a table slice that ends at v_hi
struct ScoreStreamRows {
  const float* news;
  size_t ld;
  long vc, v_hi;
  __device__ __forceinline__ const float* operator()(int r) const { return vc + r < v_hi ? news + (size_t)(vc + r) * ld : nullptr; }
};

// chunk row r = table row ids[r]; an id outside [1, V) is a row of zeros (its score is never looked at)
struct ScoreNamedRows {
  const float* news;
  size_t ld;
  const int32_t* ids;   // LDS, [128]
  int V;
  __device__ __forceinline__ const float* operator()(int r) const {
    const int32_t id = ids[r];
    return id >= 1 && id < V ? news + (size_t)id * ld : nullptr;
  }
};

// chunk row r = table row order[p + r] of a permuted ("virtual") corpus of n positions that ends at v_hi; id 0 is padding, and
// like any id outside [1, V) a row of zeros.  The tile asks a thread for two rows of a chunk only, r = srow < 64 and srow + 64
// (load_slab), once per k-slab: seek() reads their two ids once per chunk, so the slabs of a chunk cost no further index loads.
struct ScoreOrderedRows {
  const float* news;
  size_t ld;
  const int32_t* order;   // [n] news id of every position
  int V;
  long v_hi;
  int32_t id_lo, id_hi;   // this thread's rows srow and srow + 64 of the chunk seek() was given
  __device__ __forceinline__ void seek(long vc, int srow) {
    id_lo = vc + srow < v_hi ? order[vc + srow] : 0;
    id_hi = vc + srow + 64 < v_hi ? order[vc + srow + 64] : 0;
  }
  __device__ __forceinline__ const float* operator()(int r) const {
    const int32_t id = r < 64 ? id_lo : id_hi;
    return id >= 1 && id < V ? news + (size_t)id * ld : nullptr;
  }
};

template <int MT>
struct ScoreTile {
  static constexpr int TU = 16 * MT;
  float* sU;                     // [TU, ldu]   user vectors, zero beyond N and beyond U
  float* sB;                     // [2, TK_ROWS, TK_LDB] news slabs | [TU, TK_LDS_TILE] scores of a chunk
  int N, npad, ldu, ksteps;
  int tid, lane, wave;
  int srow, scol;                // staging: thread -> rows srow and srow + 64 of the chunk, columns scol .. scol + 3 of the slab
  int frow, fk;
  f32x4 g0, g1;

  __device__ __forceinline__ ScoreTile(float* smem, int n) {
    N = n; npad = tk_npad(n); ldu = npad + 4; ksteps = npad / TK_KS;
    sU = smem; sB = sU + (size_t)TU * ldu;
    tid = threadIdx.x; lane = tid & 63; wave = tid >> 6;
    srow = tid >> 3; scol = (tid & 7) * 4;
    frow = lane & 15; fk = (lane >> 4) * 8;
  }
  __device__ __forceinline__ float* end() const { return sB + TK_STAGE_FLOATS; }

  __device__ __forceinline__ void load_users(const float* user, size_t ld_user, int u0, int U) {
    for (int i = tid; i < TU * (npad / 4); i += TK_THREADS) {
      const int r = i / (npad / 4), c = (i - r * (npad / 4)) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (u0 + r < U && c < N) v = *reinterpret_cast<const f32x4*>(user + (size_t)(u0 + r) * ld_user + c);
      *reinterpret_cast<f32x4*>(sU + (size_t)r * ldu + c) = v;
    }
  }
  // rows(r): address of chunk row r, nullptr = a row of zeros
  template <class Rows>
  __device__ __forceinline__ void load_slab(const Rows& rows, int ks) {
    const int c = ks * TK_KS + scol;
    g0 = (f32x4){0.f, 0.f, 0.f, 0.f};
    g1 = g0;
    if (c < N) {
      const float* p0 = rows(srow);
      const float* p1 = rows(srow + 64);
      if (p0) g0 = *reinterpret_cast<const f32x4*>(p0 + c);
      if (p1) g1 = *reinterpret_cast<const f32x4*>(p1 + c);
    }
  }
  __device__ __forceinline__ void store_slab(int buf) {
    float* d = sB + (size_t)buf * TK_ROWS * TK_LDB + srow * TK_LDB + scol;
    *reinterpret_cast<f32x4*>(d) = g0;
    *reinterpret_cast<f32x4*>(d + 64 * TK_LDB) = g1;
  }
  // Scores of one chunk; slab 0 of it is in g0 / g1 (load_slab(rows, 0)) on entry.
  // acc[i][r] = score of user i * 16 + 4 * (lane >> 4) + r, news row 16 * wave + (lane & 15) of the chunk
  template <class Rows>
  __device__ __forceinline__ void chunk(const Rows& rows, f32x4 (&acc)[MT]) {
    store_slab(0);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MT; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < ksteps; ++ks) {
      if (ks + 1 < ksteps) load_slab(rows, ks + 1);
      const float* pb = sB + (size_t)(ks & 1) * TK_ROWS * TK_LDB + (wave * 16 + frow) * TK_LDB + fk;
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(pb), b1 = *reinterpret_cast<const f32x4*>(pb + 4);
      f32x4 a0[MT], a1[MT];
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const float* pa = sU + (size_t)(i * 16 + frow) * ldu + ks * TK_KS + fk;
        a0[i] = *reinterpret_cast<const f32x4*>(pa);
        a1[i] = *reinterpret_cast<const f32x4*>(pa + 4);
      }
      // sub-step e contracts columns ks * 32 + 8 * g + e, g = 0 .. 3 in the MFMA's own order: the same chain for every (u, v)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[i][e], b0[e], acc[i], 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[i][e], b1[e], acc[i], 0, 0, 0);
      if (ks + 1 < ksteps) store_slab((ks + 1) & 1);
      __syncthreads();
    }
  }
  // The chunk's scores into the LDS tile (it overlays the staging buffers), so that ONE wave sees all 128 scores of a user:
  // score of tile user ul, chunk row r at scores()[ul * TK_LDS_TILE + r].  A __syncthreads() must follow the readers.
  __device__ __forceinline__ void put_scores(const f32x4 (&acc)[MT]) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) sB[(i * 16 + 4 * (lane >> 4) + r) * TK_LDS_TILE + wave * 16 + frow] = acc[i][r];
    __syncthreads();
  }
  __device__ __forceinline__ const float* scores() const { return sB; }
};

// ---- host side: what the entry points of the units share ------------------------------------------------------------------

#define NR_CHECK_RC(...)               \
  do {                                 \
    const int rc__ = (__VA_ARGS__);    \
    if (rc__ != NR_OK) return rc__;    \
  } while (0)

// The argument rules every full-corpus call states the same way; `what` is the call's name in front of the message.  A call
// runs them in the order its refusals have always come in, between its own checks.
inline int check_width(const char* what, int N) {
  NR_CHECK_ARG(N >= 4 && N % 4 == 0 && N <= NR_TOPK_MAX_N, "%s: vector width N = %d must be a multiple of 4 in [4, %d]", what, N, NR_TOPK_MAX_N);
  return NR_OK;
}
inline int check_vectors(const char* what, int V, int U, int N) {
  NR_CHECK_ARG(V >= 2, "%s: V = %d news rows; row 0 is the padding news, so at least 2 are needed", what, V);
  NR_CHECK_ARG(U >= 1, "%s: U = %d users", what, U);
  return check_width(what, N);
}
// the dense list (E ids per user; 0 for a call that has none) and the CSR lists: one form per call, offsets and ids together
inline int check_lists(const char* what, int E, const int32_t* offsets, const int32_t* ids, int n_excl) {
  NR_CHECK_ARG(E >= 0 && E <= NR_TOPK_MAX_EXCLUDE, "%s: E = %d excluded ids per user, at most %d", what, E, NR_TOPK_MAX_EXCLUDE);
  NR_CHECK_ARG(n_excl >= 0, "%s: n_excl = %d entries of excl_ids, must be >= 0", what, n_excl);
  NR_CHECK_ARG(E == 0 || offsets == nullptr, "%s: the dense list (E = %d) and the CSR lists (excl_offsets) are not combined: one list form per call",
               what, E);
  NR_CHECK_ARG(n_excl == 0 || ids == nullptr || offsets != nullptr, "%s: excl_ids given without excl_offsets (n_excl = %d; the two come together)",
               what, n_excl);
  NR_CHECK_ARG(n_excl == 0 || offsets == nullptr || ids != nullptr, "%s: excl_offsets given without excl_ids (n_excl = %d; the two come together)",
               what, n_excl);
  return NR_OK;
}
inline int check_pools(const char* what, const int32_t* stamp, const int32_t* window, int ld_window) {
  NR_CHECK_ARG(stamp == nullptr || window != nullptr, "%s: stamp given without window (the two come together)", what);
  NR_CHECK_ARG(window == nullptr || stamp != nullptr, "%s: window given without stamp (the two come together)", what);
  NR_CHECK_ARG(window == nullptr || ld_window >= 2, "%s: ld_window = %d, a window row is (lo, hi): at least 2", what, ld_window);
  return NR_OK;
}
inline int check_rows(const char* what, const float* news, int ld_news, const float* user, int ld_user, int N) {
  NR_CHECK_ARG(ld_news >= N && ld_news % 4 == 0 && ld_user >= N && ld_user % 4 == 0 && (((uintptr_t)news | (uintptr_t)user) & 15) == 0,
               "%s: rows must be 16-byte aligned (ld_news = %d, ld_user = %d: multiples of 4, >= N = %d)", what, ld_news, ld_user, N);
  return NR_OK;
}
// `need` = what nr_<what>_workspace_bytes answers for the descriptor
inline int check_workspace(const char* what, const void* ws, size_t ws_bytes, size_t need) {
  NR_CHECK_ARG(ws != nullptr && ws_bytes >= need && (((uintptr_t)ws) & 7) == 0,
               "%s: workspace holds %zu bytes, nr_%s_workspace_bytes asks for %zu (8-byte aligned)", what, ws_bytes, what, need);
  return NR_OK;
}

inline PoolArgs pool_args(const float* prior, const int32_t* stamp, const int32_t* window, int ld_window) {
  return {prior, stamp, window, (size_t)ld_window};
}
// offsets == nullptr in the result = the call has no CSR lists.  n == 0: every segment is empty, so that is no CSR call either.
inline CsrArgs csr_args(const int32_t* offsets, const int32_t* ids, int n) {
  const bool csr = offsets != nullptr && ids != nullptr && n > 0;
  return {csr ? offsets : nullptr, csr ? ids : nullptr, csr ? n : 0};
}

// LDS bytes of the tile itself, and the widest user tile that fits with the `per_user` bytes a pass keeps per user beside it (the
// candidates and threshold of the selection; nothing where keys and counters live in registers)
inline size_t tk_tile_bytes(int TU, int N) { return tk_tile_floats(TU, N) * sizeof(float); }
inline int score_user_tile(int N, size_t per_user) {
  for (int tu = 64; tu > 16; tu >>= 1)
    if (tk_tile_bytes(tu, N) + tu * per_user <= TK_LDS_MAX) return tu;
  return 16;
}
// slices: enough workgroups to fill the chip when there are few user tiles, 1-2 when there are many; never more slices than
// chunks, nor than `most`
inline int score_auto_splits(int U, int V, int tile, int most) {
  const long tiles = ((long)U + tile - 1) / tile;
  long s = (TK_CUS + tiles - 1) / tiles;
  const long chunks = ((long)V - 1 + TK_ROWS - 1) / TK_ROWS;
  if (s > chunks) s = chunks;
  if (s > most) s = most;
  return s < 1 ? 1 : (int)s;
}

// A run-time choice as a template argument: f gets std::integral_constant<.., the value>.  with_int knows the values it is
// given and no others, so a call site instantiates exactly the kernels it lists.
template <class F>
int with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
template <int... Vs, class F>
int with_int(int v, F&& f) {
  int rc = NR_ERR_ARG;
  (void)((v == Vs ? (rc = f(std::integral_constant<int, Vs>{}), true) : false) || ...);
  return rc;
}
// One launch of a kernel with dynamic LDS above the default limit: the attribute, then the launch
template <class... A>
int launch_lds(void (*kernel)(A...), dim3 grid, dim3 block, size_t smem, hipStream_t s, std::common_type_t<A>... args) {
  NR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  hipLaunchKernelGGL(kernel, grid, block, smem, s, args...);
  return NR_OK;
}

}  // namespace
