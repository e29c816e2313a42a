// Row-deferred Adam over a [rows, width] fp32 table that lives in a flat bucket (parallel.FlatBucket, table_adam="deferred").
//
// Dense Adam moves EVERY row at every step: a row whose gradient is zero still decays its moments and is pulled along by
// them.  That motion depends only on the row's own p, m, v and on the step number, so it does not have to happen at the step
// itself: row_step[r] counts the steps row r has had, and the steps it is behind are replayed in registers -- the same
// adam1() of nr_adam.h, a gradient of zero, the per-step scalars the dense call derived for that step (kept in `sched`) --
// the next time the row is read.  Same inputs, same instruction sequence, same bits; a step then touches only the rows
// of its batch (15 k of 65 001 at B = 512) instead of streaming p, g, m, v of the whole table.
//
//   adam_rows_claim   one thread per id (or per row, for a flush): atomicMax on row_step[id] decides the ONE owner of a row,
//                     which appends (row, steps the row had) to a work list through a device-side counter -- duplicate ids
//                     cost nothing and cannot race.  id 0 (padding_idx: no gradient, zero moments, never moves) and ids
//                     outside the table are skipped.  The call that does step t also files t's scalars under sched[t].
//   adam_rows_apply   fixed grid, grid-stride over (work item, 16-byte chunk of the row), the count read from the device:
//                     consecutive lanes take consecutive chunks of one row (a 36 000-byte row is 2 250 chunks = 35 full
//                     waves), so every access is a 1 KiB wave-wide stream as in the dense kernel.
#include "nr_common.h"
#include "nr_adam.h"

namespace {

struct RowItem {
  int row, old_step;
};

__global__ __launch_bounds__(256) void adam_rows_claim_kernel(const int32_t* __restrict__ ids, int ids_stride, int n, int rows,
                                                               int32_t* __restrict__ row_step, int target, float2* __restrict__ sched,
                                                               int file_step, float2 file_pair, int* __restrict__ counter,
                                                               RowItem* __restrict__ list) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0 && file_step >= 0) sched[file_step] = file_pair;
  if (i >= n) return;
  const int r = ids != nullptr ? ids[(size_t)i * ids_stride] : i;
  if (r < 1 || r >= rows) return;
  const int old = atomicMax(&row_step[r], target);
  if (old < target) {
    const int slot = atomicAdd(counter, 1);
    list[slot] = RowItem{r, old < 0 ? 0 : old};
  }
}

__global__ __launch_bounds__(256) void adam_rows_apply_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                               float* __restrict__ v, unsigned chunks, const RowItem* __restrict__ list,
                                                               const int* __restrict__ counter, const float2* __restrict__ sched, int upto,
                                                               int apply, AdamCfg c, float zero_g, bf16_t* __restrict__ pack_dst,
                                                               unsigned pack_cols, unsigned pack_ld) {
  const size_t total = (size_t)*counter * chunks;
  const size_t width = (size_t)chunks * 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const unsigned item = (unsigned)(i / chunks), ch = (unsigned)(i - (size_t)item * chunks);
    const RowItem it = list[item];
    const size_t at = ((size_t)it.row * width) / 4 + ch;                 // in 16-byte chunks from the table's base
    f32x4* p4 = reinterpret_cast<f32x4*>(p) + at;
    f32x4* m4 = reinterpret_cast<f32x4*>(m) + at;
    f32x4* v4 = reinterpret_cast<f32x4*>(v) + at;
    f32x4* g4 = reinterpret_cast<f32x4*>(g) + at;
    const f32x4 pv = *p4, mv = *m4, vv = *v4;
    f32x4 gv = {0.f, 0.f, 0.f, 0.f};
    if (apply) gv = *g4;
    float pp[4] = {pv[0], pv[1], pv[2], pv[3]}, mm[4] = {mv[0], mv[1], mv[2], mv[3]}, ww[4] = {vv[0], vv[1], vv[2], vv[3]};
    int replay = upto - it.old_step;                                     // 0 <= old_step, so the trip count is at most upto
    replay = replay < 0 ? 0 : (replay > upto ? upto : replay);
    // a chunk whose moments are all +0.0 stands still under a zero gradient (m, v stay +0, p -= step_size * (0 / eps)):
    // rows that never had a gradient -- most of a flush -- skip the loop, which changes no bit
    const bool still = (__float_as_uint(mm[0]) | __float_as_uint(mm[1]) | __float_as_uint(mm[2]) | __float_as_uint(mm[3]) |
                        __float_as_uint(ww[0]) | __float_as_uint(ww[1]) | __float_as_uint(ww[2]) | __float_as_uint(ww[3])) == 0u;
    if (!still) {
      AdamCfg r = c;
      r.zero_grad = 0;
      for (int s = upto - replay + 1; s <= upto; ++s) {
        const float2 sc = sched[s];
        r.step_size = sc.x;
        r.bc2_sqrt = sc.y;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float gz = zero_g;                                             // a run-time zero: adam1 is compiled as in the dense kernel
          adam1(pp[e], gz, mm[e], ww[e], r);
        }
      }
    }
    if (apply) {
      float gg[4] = {gv[0], gv[1], gv[2], gv[3]};
#pragma unroll
      for (int e = 0; e < 4; ++e) adam1(pp[e], gg[e], mm[e], ww[e], c);
    }
    *p4 = (f32x4){pp[0], pp[1], pp[2], pp[3]};
    if (pack_dst != nullptr) {                                           // as adam_kernel: what nr_cast_pad makes of the new values
      const unsigned e0 = ch * 4, pr = e0 / pack_cols, col = e0 - pr * pack_cols;
      const bf16x4 o = {(bf16_t)pp[0], (bf16_t)pp[1], (bf16_t)pp[2], (bf16_t)pp[3]};
      *reinterpret_cast<bf16x4*>(pack_dst + ((size_t)it.row * (chunks * 4 / pack_cols) + pr) * pack_ld + col) = o;
    }
    *m4 = (f32x4){mm[0], mm[1], mm[2], mm[3]};
    *v4 = (f32x4){ww[0], ww[1], ww[2], ww[3]};
    if (apply && c.zero_grad) *g4 = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
}

constexpr size_t ROWS_WS_HEAD = 16;       // the counter, padded so that the list stays 16-byte aligned

}  // namespace

extern "C" {

size_t nr_adam_rows_workspace_bytes(int n_ids) { return n_ids < 0 ? 0 : ROWS_WS_HEAD + (size_t)n_ids * sizeof(RowItem); }

int nr_adam_rows(const nr_adam_rows_desc* d, nr_stream_t stream) {
  NR_CHECK_ARG(d != nullptr, "adam_rows: null descriptor");
  NR_CHECK_ARG(d->rows >= 1 && d->width >= 4 && d->width % 4 == 0, "adam_rows: table [%d, %d] must have a width that is a multiple of 4", d->rows,
               d->width);
  NR_CHECK_ARG(d->apply == 0 || d->apply == 1, "adam_rows: apply must be 0 (catch-up) or 1 (catch-up + step), got %d", d->apply);
  NR_CHECK_ARG(d->beta1 >= 0.f && d->beta1 < 1.f && d->beta2 >= 0.f && d->beta2 < 1.f && d->eps >= 0.f && d->upto >= 0,
               "adam_rows: bad hyper-parameters");
  NR_CHECK_ARG(d->eps > 0.f, "adam_rows: eps == 0 is refused (dense Adam makes 0/0 = NaN of every row that never had a gradient: "
                             "there is nothing to reproduce)");
  const int n = d->ids != nullptr ? d->n_ids : d->rows;                 // ids == NULL: every row (flush)
  NR_CHECK_ARG(n >= 0 && (d->ids == nullptr || d->ids_stride >= 1), "adam_rows: bad id list (%d ids, stride %d)", d->n_ids, d->ids_stride);
  const size_t need = nr_adam_rows_workspace_bytes(n);
  NR_CHECK_ARG(d->ws != nullptr && d->ws_bytes >= need && (((uintptr_t)d->ws) & 15) == 0,
               "adam_rows: workspace holds %zu bytes, nr_adam_rows_workspace_bytes(%d) asks for %zu (16-byte aligned)", d->ws_bytes, n, need);
  NR_CHECK_ARG(d->sched != nullptr && d->upto + d->apply < d->sched_capacity && (((uintptr_t)d->sched) & 7) == 0,
               "adam_rows: sched holds %d steps, step %d is needed", d->sched_capacity, d->upto + d->apply);
  NR_CHECK_ARG(d->param && d->exp_avg && d->exp_avg_sq && d->row_step && (d->apply == 0 || d->grad), "adam_rows: null pointer");
  NR_CHECK_ARG((((uintptr_t)d->param | (uintptr_t)d->grad | (uintptr_t)d->exp_avg | (uintptr_t)d->exp_avg_sq) & 15) == 0,
               "adam_rows: buffers must be 16-byte aligned");
  NR_CHECK_ARG(d->pack_dst == nullptr || (d->pack_cols >= 4 && d->pack_cols % 4 == 0 && d->width % d->pack_cols == 0 && d->pack_ld >= d->pack_cols &&
                                          d->pack_ld % 4 == 0 && (((uintptr_t)d->pack_dst) & 7) == 0),
               "adam_rows: packed copy (cols %d, ld %d) must split a row of %d into whole rows of a multiple of 4 columns", d->pack_cols, d->pack_ld,
               d->width);
  if (n == 0 && d->apply == 0) return NR_OK;
  NR_DEVICE_GUARD(stream, d->param);
  hipStream_t s = (hipStream_t)stream;
  AdamCfg c;
  c.beta1 = d->beta1; c.beta2 = d->beta2; c.eps = d->eps; c.grad_scale = d->grad_scale; c.zero_grad = d->zero_grad;
  c.step_size = 0.f; c.bc2_sqrt = 1.f;
  int file_step = -1;
  float2 pair = {0.f, 1.f};
  if (d->apply) {                                                        // step upto + 1: its scalars, derived where the dense call derives them
    file_step = d->upto + 1;
    nr_adam_bias(d->lr, d->beta1, d->beta2, file_step, &c.step_size, &c.bc2_sqrt);
    pair.x = c.step_size; pair.y = c.bc2_sqrt;
  }
  int* counter = reinterpret_cast<int*>(d->ws);
  RowItem* list = reinterpret_cast<RowItem*>(reinterpret_cast<char*>(d->ws) + ROWS_WS_HEAD);
  NR_CHECK_HIP(hipMemsetAsync(counter, 0, ROWS_WS_HEAD, s));
  const int target = d->upto + d->apply;
  {
    NrProfScope ps(s, "adam_rows_claim[n=%d,%s,upto=%d,apply=%d]", n, d->ids ? "ids" : "flush", d->upto, d->apply);
    hipLaunchKernelGGL(adam_rows_claim_kernel, dim3((unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1)), dim3(256), 0, s, d->ids, d->ids_stride, n,
                       d->rows, d->row_step, target, reinterpret_cast<float2*>(d->sched), file_step, pair, counter, list);
  }
  NR_CHECK_LAUNCH();
  if (n == 0) return NR_OK;
  const unsigned chunks = (unsigned)d->width / 4;
  const size_t most = ((size_t)n * chunks + 255) / 256;                  // no more workgroups than the longest possible list needs
  {
    NrProfScope ps(s, "adam_rows_apply[n<=%d,width=%d,upto=%d,apply=%d]", n, d->width, d->upto, d->apply);
    hipLaunchKernelGGL(adam_rows_apply_kernel, dim3((unsigned)(most > 8192 ? 8192 : most)), dim3(256), 0, s, d->param, d->grad, d->exp_avg,
                       d->exp_avg_sq, chunks, (const RowItem*)list, (const int*)counter, reinterpret_cast<const float2*>(d->sched), d->upto, d->apply, c,
                       0.f, reinterpret_cast<bf16_t*>(d->pack_dst), (unsigned)(d->pack_dst ? d->pack_cols : 4), (unsigned)d->pack_ld);
  }
  NR_CHECK_LAUNCH();
  return NR_OK;
}

}  // extern "C"
