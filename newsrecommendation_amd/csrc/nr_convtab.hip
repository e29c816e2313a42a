// Gradient of NAML's trainable title-embedding table (freeze_embedding=False, src/model/NAML.py:104-107):
//   dx[s,t,:]              = sum_j W_j^T . dy[s,t-j+1,:]                       one NT GEMM over the LIVE titles (nr_api.hip)
//   dtable[id_s, t*D + c] += keep(s,t,c) * scale * dx[s,t,c]    (id_s != 0)    owner-computes scatter, below
// The kernels around that GEMM:
//   conv_table_live     ordered list of the titles that reach the table gradient (id != 0, dy not flagged zero)
//   conv_table_stage    their dy rows copied into the gapped layout of nr_launch_conv_rows (a zero row between titles), so
//                       that the im2col row of a token is 3N contiguous elements: the LDS-DMA GEMM's operand, no 3x copy
//   (nr_launch_sort_rows_by_id groups the list by news id)
//   conv_table_rank     orders every group by position in the batch: the counting sort places with atomics, and the
//                       summation order below must not depend on their arrival order
//   conv_table_scatter  ONE workgroup chunk owns all occurrences of one news id: sums their dx rows in registers, in batch order,
//                       and issues one read-add-store per destination element.  No atomics, so the result is bit-identical
//                       from run to run without a fixed-point shadow of the (multi-GB) gradient; destination offsets are 64-bit.
#include "nr_gemm.h"

namespace {

// Ordered compaction by ONE workgroup (n is a batch's title count: tens of thousands): every thread owns a contiguous run of
// titles, the block scans the counts, the runs are written back to back -- the list is ascending in the title number.
// hdr[0] = live titles, hdr[1] = live titles * T (the GEMM's row count), hdr[2..7] = 0
__global__ __launch_bounds__(1024) void conv_table_live_kernel(const int32_t* __restrict__ ids, int ids_stride, const int32_t* __restrict__ seq_nz,
                                                               int n, int T, int V, int32_t* __restrict__ hdr, int32_t* __restrict__ live_s,
                                                               int32_t* __restrict__ live_id) {
  __shared__ int sSum[1024];
  const int tid = threadIdx.x, per = (n + 1023) / 1024, s0 = min(n, tid * per), s1 = min(n, s0 + per);
  auto live = [&](int s) {
    const int id = ids[(size_t)s * ids_stride];
    return id > 0 && id < V && (seq_nz == nullptr || seq_nz[s] != 0);   // padding_idx row gets no gradient; a zero dy adds nothing
  };
  int c = 0;
  for (int s = s0; s < s1; ++s) c += live(s) ? 1 : 0;
  sSum[tid] = c;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int x = tid >= o ? sSum[tid - o] : 0;
    __syncthreads();
    sSum[tid] += x;
    __syncthreads();
  }
  int k = sSum[tid] - c;
  for (int s = s0; s < s1; ++s)
    if (live(s)) {
      live_s[k] = s;
      live_id[k] = ids[(size_t)s * ids_stride];
      ++k;
    }
  if (tid == 1023) { hdr[0] = sSum[1023]; hdr[1] = sSum[1023] * T; }
  if (tid >= 2 && tid < 8) hdr[tid] = 0;
}

// One workgroup per staged title.  compact: slot b holds live title live_s[b] (b < count); else slot b holds title b.
// Slot b occupies rows b*(T+1)+1 .. b*(T+1)+T of `out` [slots*(T+1)+1, N]; the workgroup also writes the zero rows on both
// sides (neighbours write the same zeros).  ident [slots*T]: the GEMM's (identity) row map.
template <typename E>
__global__ __launch_bounds__(256) void conv_table_stage_kernel(const E* __restrict__ dy, int T, int N, const int32_t* __restrict__ hdr,
                                                               const int32_t* __restrict__ live_s, int compact, E* __restrict__ out,
                                                               int32_t* __restrict__ ident) {
  constexpr int CH = 16 / (int)sizeof(E);
  const int b = blockIdx.x;
  if (compact && b >= hdr[0]) return;
  const int s = compact ? live_s[b] : b;
  const int cpr = N / CH;
  const uint4* src = reinterpret_cast<const uint4*>(dy + (size_t)s * T * N);
  uint4* dst = reinterpret_cast<uint4*>(out + (size_t)b * (T + 1) * N);
  const int body0 = cpr, body1 = (T + 1) * cpr;          // 16-byte chunks [body0, body1) are the T token rows, the rest zero rows
  for (int u = threadIdx.x; u < (T + 2) * cpr; u += 256) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (u >= body0 && u < body1) v = src[u - cpr];
    dst[u] = v;
  }
  if (ident != nullptr)
    for (int t = threadIdx.x; t < T; t += 256) ident[(size_t)b * T + t] = b * T + t;
}

// After the counting sort cursor[id] is the END of id's group and cursor[id - 1] its start (ids are >= 1 here).  Every
// member counts the members of its group that come earlier in the batch and takes that place: ascending live-list position.
__global__ __launch_bounds__(256) void conv_table_rank_kernel(const int32_t* __restrict__ hdr, const int32_t* __restrict__ sort_s,
                                                              const int32_t* __restrict__ sort_id, const int32_t* __restrict__ sort_k,
                                                              const int32_t* __restrict__ cursor, int compact, int32_t* __restrict__ ord_s,
                                                              int32_t* __restrict__ ord_slot) {
  const int count = hdr[0];
  for (int j = blockIdx.x * 256 + threadIdx.x; j < count; j += gridDim.x * 256) {
    const int id = sort_id[j], start = cursor[id - 1], end = cursor[id], k = sort_k[j];
    int rank = 0;
    for (int i = start; i < end; ++i) rank += sort_k[i] < k ? 1 : 0;
    ord_s[start + rank] = sort_s[j];
    ord_slot[start + rank] = compact ? k : sort_s[j];
  }
}

template <typename E, int VEC> struct DxLoad;
template <> struct DxLoad<float, 4> {
  static __device__ __forceinline__ void ld(const float* p, float (&x)[4]) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; x[3] = v[3];
  }
};
template <> struct DxLoad<bf16_t, 4> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float (&x)[4]) {
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
    x[0] = (float)v[0]; x[1] = (float)v[1]; x[2] = (float)v[2]; x[3] = (float)v[3];
  }
};
template <typename E> struct DxLoad<E, 1> {
  static __device__ __forceinline__ void ld(const E* p, float (&x)[1]) { x[0] = (float)p[0]; }
};

// grid (sorted positions, chunks of 256 * U * VEC elements of a [T*D] table row).  Only the workgroups that sit on the first
// member of a group work: they own dtable[id, chunk] -- nobody else touches it in this launch.
constexpr int SC_U = 4, SC_RUN = 256;
template <typename E, int VEC>
__global__ __launch_bounds__(256) void conv_table_scatter_kernel(const E* __restrict__ dx, int ldx, int T, int D, int V, const int32_t* __restrict__ hdr,
                                                                 const int32_t* __restrict__ sort_id, const int32_t* __restrict__ cursor,
                                                                 const int32_t* __restrict__ ord_s, const int32_t* __restrict__ ord_slot,
                                                                 DropCfg drop, float* __restrict__ dtable) {
  __shared__ int sS[SC_RUN], sSlot[SC_RUN];
  const int j = blockIdx.x;
  if (j >= hdr[0]) return;
  const int id = sort_id[j];
  if (id < 1 || id >= V) return;                       // (the live list holds valid ids only: belt and braces in front of a store)
  const int start = cursor[id - 1], end = cursor[id];
  if (j != start) return;
  const int TD = T * D, nvec = TD / VEC;
  int e[SC_U], t[SC_U], c[SC_U];
  float acc[SC_U][VEC];
#pragma unroll
  for (int u = 0; u < SC_U; ++u) {
    const int v = (blockIdx.y * SC_U + u) * 256 + threadIdx.x;
    e[u] = v < nvec ? v * VEC : -1;
    t[u] = e[u] >= 0 ? e[u] / D : 0;
    c[u] = e[u] >= 0 ? e[u] - t[u] * D : 0;
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[u][q] = 0.f;
  }
  for (int r0 = start; r0 < end; r0 += SC_RUN) {
    const int nr = min(SC_RUN, end - r0);
    __syncthreads();
    for (int r = threadIdx.x; r < nr; r += 256) { sS[r] = ord_s[r0 + r]; sSlot[r] = ord_slot[r0 + r]; }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
      const int s = sS[r], slot = sSlot[r];
#pragma unroll
      for (int u = 0; u < SC_U; ++u) {
        if (e[u] < 0) continue;
        float x[VEC];
        DxLoad<E, VEC>::ld(dx + ((size_t)slot * T + t[u]) * ldx + c[u], x);
        uint32_t kb = 0xfu;
        if (drop.thresh) {
          // the forward's draw: element index (s*T + t)*D + c
          const uint32_t eidx = ((uint32_t)s * (uint32_t)T + (uint32_t)t[u]) * (uint32_t)D + (uint32_t)c[u];
          if (VEC == 4 && (eidx & 1u) == 0) {
            kb = nr_keep4(drop.key, eidx, drop.thresh);
          } else {
            kb = 0;
#pragma unroll
            for (int q = 0; q < VEC; ++q) kb |= nr_keep(drop.key, eidx + q, drop.thresh) ? (1u << q) : 0u;
          }
        }
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[u][q] += ((kb >> q) & 1u) ? x[q] * drop.scale : 0.f;
      }
    }
  }
  float* row = dtable + (size_t)id * (size_t)TD;         // 64-bit: V*T*D floats pass 4 GiB from V ~ 120 000
#pragma unroll
  for (int u = 0; u < SC_U; ++u) {
    if (e[u] < 0) continue;
    if constexpr (VEC == 4) {
      f32x4* p = reinterpret_cast<f32x4*>(row + e[u]);
      f32x4 g = *p;
      g[0] += acc[u][0]; g[1] += acc[u][1]; g[2] += acc[u][2]; g[3] += acc[u][3];
      *p = g;
    } else {
      row[e[u]] += acc[u][0];
    }
  }
}

}  // namespace

int nr_launch_conv_table_live(const int32_t* ids, int ids_stride, const int32_t* seq_nz, int n, int T, int V, int32_t* hdr, int32_t* live_s,
                              int32_t* live_id, hipStream_t stream) {
  NR_CHECK_ARG(ids && hdr && live_s && live_id && n > 0 && T > 0 && V > 0 && ids_stride >= 1, "conv_table_live: bad arguments");
  NrProfScope ps(stream, "conv_table_live[n=%d,V=%d]", n, V);
  hipLaunchKernelGGL(conv_table_live_kernel, dim3(1), dim3(1024), 0, stream, ids, ids_stride, seq_nz, n, T, V, hdr, live_s, live_id);
  NR_CHECK_LAUNCH();
  return NR_OK;
}

int nr_launch_conv_table_stage(int dtype, const void* dy, int n, int T, int N, const int32_t* hdr, const int32_t* live_s, bool compact, void* out,
                               int32_t* ident, hipStream_t stream) {
  NR_CHECK_ARG(dy && out && hdr && live_s && n > 0 && N % nr_chunk(dtype) == 0 && (((uintptr_t)dy | (uintptr_t)out) & 15) == 0,
               "conv_table_stage: bad arguments (dy and the workspace must be 16-byte aligned, N a whole number of 16-byte chunks)");
  NrProfScope ps(stream, "conv_table_stage[%s,n=%d,T=%d,N=%d]", dtype == NR_BF16 ? "bf16" : "f32", n, T, N);
  if (dtype == NR_BF16)
    hipLaunchKernelGGL(conv_table_stage_kernel<bf16_t>, dim3(n), dim3(256), 0, stream, (const bf16_t*)dy, T, N, hdr, live_s, compact ? 1 : 0,
                       (bf16_t*)out, ident);
  else
    hipLaunchKernelGGL(conv_table_stage_kernel<float>, dim3(n), dim3(256), 0, stream, (const float*)dy, T, N, hdr, live_s, compact ? 1 : 0,
                       (float*)out, ident);
  NR_CHECK_LAUNCH();
  return NR_OK;
}

int nr_launch_conv_table_rank(const int32_t* hdr, const int32_t* sort_s, const int32_t* sort_id, const int32_t* sort_k, const int32_t* cursor,
                              bool compact, int n, int32_t* ord_s, int32_t* ord_slot, hipStream_t stream) {
  NR_CHECK_ARG(hdr && sort_s && sort_id && sort_k && cursor && ord_s && ord_slot && n > 0, "conv_table_rank: bad arguments");
  NrProfScope ps(stream, "conv_table_rank[n=%d]", n);
  hipLaunchKernelGGL(conv_table_rank_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, hdr, sort_s, sort_id, sort_k, cursor, compact ? 1 : 0,
                     ord_s, ord_slot);
  NR_CHECK_LAUNCH();
  return NR_OK;
}

int nr_launch_conv_table_scatter(int dx_dtype, const void* dx, int ldx, int n, int T, int D, int V, const int32_t* hdr, const int32_t* sort_id,
                                 const int32_t* cursor, const int32_t* ord_s, const int32_t* ord_slot, DropCfg drop, float* dtable,
                                 hipStream_t stream) {
  NR_CHECK_ARG(dx && dtable && hdr && sort_id && cursor && ord_s && ord_slot && n > 0 && T > 0 && D > 0 && V > 0 && ldx >= D,
               "conv_table_scatter: bad arguments");
  const bool vec = D % 4 == 0 && ldx % 4 == 0 && (((uintptr_t)dx) & 15) == 0 && (((uintptr_t)dtable) & 15) == 0;
  const int nvec = T * D / (vec ? 4 : 1);
  const dim3 grid(n, (nvec + 256 * SC_U - 1) / (256 * SC_U));
  NrProfScope ps(stream, "conv_table_scatter[%s,n=%d,T=%d,D=%d,V=%d]", dx_dtype == NR_BF16 ? "bf16" : "f32", n, T, D, V);
#define NR_SC_LAUNCH(E, VEC)                                                                                                              \
  hipLaunchKernelGGL((conv_table_scatter_kernel<E, VEC>), grid, dim3(256), 0, stream, (const E*)dx, ldx, T, D, V, hdr, sort_id, cursor, ord_s, \
                     ord_slot, drop, dtable)
  if (dx_dtype == NR_BF16) { if (vec) NR_SC_LAUNCH(bf16_t, 4); else NR_SC_LAUNCH(bf16_t, 1); }
  else { if (vec) NR_SC_LAUNCH(float, 4); else NR_SC_LAUNCH(float, 1); }
#undef NR_SC_LAUNCH
  NR_CHECK_LAUNCH();
  return NR_OK;
}
