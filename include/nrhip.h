/* libnrhip — C ABI of the MI355X (gfx950) NRMS / NAML encoder + scorer hot path.
 *
 * The reference (patngnw/NewsRecommendation) is pure Python on ATen ops and has no FFI of
 * its own; each entry point below replaces one ATen op sequence of the reference's
 * src/model/{NRMS,NAML,model_utils}.py and is what a `ctypes` binding inside those modules would call
 * (INTEGRATION.md shows the stub).  Citations are paths under /root/reference/.
 *
 * Conventions
 *  - All pointers are DEVICE pointers unless a comment says host.  Row-major, contiguous
 *    unless a leading dimension (`ld*`, in elements) is given.
 *  - `dtype` selects the storage type of activations / packed weights AND the MFMA operand
 *    type: NR_F32 (v_mfma_f32_16x16x4_f32, exact fp32) or NR_BF16 (v_mfma_f32_16x16x32_bf16,
 *    fp32 accumulate).  Parameters, gradients of parameters, pooled vectors, scores and the
 *    loss are always fp32.
 *  - The caller owns every buffer (outputs, saved activations, workspaces).  The library
 *    never allocates or frees device memory and never synchronises the stream; every call
 *    only enqueues kernels on `stream` (a hipStream_t).
 *  - Returns NR_OK (0) or an NR_ERR_* code; nr_last_error() gives the message.  Nothing
 *    throws across the ABI.
 *  - Leading dimensions of dtype buffers used as GEMM operands must be multiples of one
 *    16-byte chunk (4 fp32 / 8 bf16) and the buffers 16-byte aligned; nr_cast_pad produces
 *    such buffers (zero padded).
 *  - "accumulate" outputs (dw*, db*, dtable, dpad) are ADDED to: zero them first.
 *  - Dropout: Bernoulli keep decisions are a pure function of (seed, element index); the
 *    backward call must receive the same seed.  p == 0 disables it (eval mode).
 */
#ifndef NRHIP_H
#define NRHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NR_F32 0
#define NR_BF16 1

#define NR_OK 0
#define NR_ERR_ARG 1
#define NR_ERR_HIP 2

#define NR_SRC_DENSE 0  /* x is [M, ldx] of dtype                                   */
#define NR_SRC_GATHER 1 /* x is a table [V, ldx] of dtype, row m = table[ids[m*ids_stride]] */

typedef void* nr_stream_t; /* hipStream_t */

int nr_version(void);
/* Copies the calling thread's last error message (NUL terminated) into buf; returns its length. */
int nr_last_error(char* buf, size_t n);
/* Integer switches of the library (a production path and the variant it replaced, which tests compare): name without the
 * NR_ prefix, e.g. "NO_SLABS", "NT_WREG" (full list: csrc/nr_common.h, enum NrOpt).  Defaults are the production
 * configuration; the environment variable NR_<NAME> presets an option once per process.  nr_get_option returns
 * -1 for an unknown name.  Not thread-synchronised with calls in flight: set options between calls.              */
/* sizeof of the descriptor structs as this library was compiled: out[0..3] = nr_mhsa_desc, nr_conv_desc, nr_pool_desc,
 * nr_linear_desc, with n >= 6 also out[4..5] = nr_cast_job, nr_pack_job, with n >= 7 out[6] = nr_adam_rows_desc, with n >= 8 out[7] = nr_topk_desc, with n >= 9 out[8] = nr_rank_desc, with n >= 10 out[9] = nr_mmr_desc, with n >= 11 out[10] = nr_sample_desc, with n >= 12 out[11] = nr_logz_desc, with n >= 13 out[12] = nr_logprob_desc, with n >= 14 out[13] = nr_logz_groups_desc, with n >= 15 out[14] = nr_logprob_capped_desc, with n >= 16 out[15] = nr_expect_desc, with n >= 17 out[16] = nr_expect_news_desc, with n >= 18 out[17] = nr_logprob_grad_desc, with n >= 20 out[18..19] = nr_expect_groups_desc, nr_logprob_capped_grad_desc, with n >= 21 out[20] = nr_expect_news_groups_desc, with n >= 23 out[21..22] = nr_entropy_desc, nr_expect_affine_desc, with n >= 24 out[23] = nr_expect_news_affine_desc.  A binding compares them with its own layout at
 * load time (ABI drift -> refuse to run).                                                                              */
int nr_abi_sizes(size_t* out, int n);
/* Deterministic mode.  Outputs that several workgroups add into (dW, db, dtable, dpad) are accumulated with fp32 atomics
 * by default, so their last bits depend on the arrival order.  With a scratch buffer registered here they are accumulated
 * in 2^-36 fixed point with 64-bit integer atomics (order independent) and flushed onto the fp32 output at the end of
 * each call: gradients are bit-reproducible from run to run.  scratch: DEVICE memory, ZERO filled, 8 bytes per element of
 * the largest set of accumulated outputs of one call (e.g. 3N*(d_model+1) + table_rows*d_model for nr_mhsa_bwd); the
 * library leaves it zero filled after every call.  scratch == NULL switches the mode off.  One stream at a time.
 * Gather sources need `table_rows` in their descriptor in this mode.
 * Not covered: nr_embed_gather_bwd (K1).  That stand-alone entry takes no table size, so it registers no range and adds
 * with fp32 atomics in either mode; the deterministic table gradients are those of the fused gather sources, which carry
 * `table_rows` (nr_mhsa_bwd, nr_conv1d_k3_bwd_table, nr_linear_bwd).                                                  */
int nr_set_deterministic(void* scratch, size_t bytes);
int nr_set_option(const char* name, int value);
int nr_get_option(const char* name);

/* Device: every entry point that takes a stream runs on the device that owns that stream (for the NULL stream: the
 * device that owns its first pointer argument) -- the library switches the calling thread to it for the duration
 * of the call (forward runs on the rank's main thread, backward on the autograd engine thread).                   */

/* ---------------------------------------------------------------------------------------
 * Packing: fp32 master parameter -> dtype operand with zero padded leading dimension.
 * transpose == 0: dst[r, c] = src[r, c]      dst is [rows, ld_dst]
 * transpose == 1: dst[c, r] = src[r, c]      dst is [cols, ld_dst]
 * Replaces the implicit `.float()` / `.cuda()` parameter materialisation of
 * src/model/NRMS.py:70-73 and src/main.py:79.                                              */
int nr_cast_pad(const float* src, int rows, int cols, int ld_src, void* dst, int ld_dst, int dtype,
                int transpose, nr_stream_t stream);
/* The same for up to NR_CAST_BATCH_MAX operands in ONE launch (the weights a training step re-packs after each optimizer
 * step are small: one 6-us launch each otherwise).  `jobs` is host memory; all destinations share `dtype`.            */
#define NR_CAST_BATCH_MAX 16
typedef struct {
  const float* src;
  void* dst;
  int rows, cols, ld_src, ld_dst, transpose;
} nr_cast_job;
int nr_cast_pad_batch(const nr_cast_job* jobs, int n, int dtype, nr_stream_t stream);
/* Conv1d weight [N, D, 3] (src/model/NAML.py:27-32) -> tap-major GEMM operand [N, 3*Dp]
 * (dst[n, tap*Dp + d] = w[n, d, tap]); unpack is the inverse on an fp32 gradient
 * (accumulate != 0: dw += ..., else dw = ...).                                               */
int nr_pack_conv_w(const float* w, int N, int D, void* dst, int Dp, int dtype, nr_stream_t stream);
int nr_unpack_conv_dw(const float* dw_pack, int N, int D, int Dp, float* dw, int accumulate, nr_stream_t stream);
/* The same weight as the [D, ld] operand of the table-gradient GEMM (nr_conv1d_k3_bwd_table): dst[d, j*N + n] = w[n, d, 2 - j],
 * zero from column 3N to ld (ld >= 3N; bf16: a multiple of 32 so that the LDS-DMA GEMM runs whole k-steps).             */
int nr_pack_conv_w_t(const float* w, int N, int D, void* dst, int ld, int dtype, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K1  embedding row gather — nn.Embedding(padding_idx=0) lookup,
 * src/model/NRMS.py:28, src/model/NAML.py:48-50, and the eval-time news-vector gather
 * src/dataset.py:68,72.  out[m, 0:cols] = table[ids[m*ids_stride], 0:cols] (fp32 out).
 * bwd: dtable[ids[m], :] += dout[m, :] for ids[m] != 0 (padding_idx row gets no gradient).
 * The bwd adds with fp32 atomics with and without deterministic mode (it has no table size to register a fixed-point range
 * with, see nr_set_deterministic, and leaves the scratch untouched): with repeated ids its last bits depend on the arrival
 * order.  The fused gather sources, which carry `table_rows`, are the deterministic ones.      */
int nr_embed_gather_fwd(const void* table, int ld_table, int dtype, const int32_t* ids, int n_ids,
                        int ids_stride, int cols, float* out, int ld_out, nr_stream_t stream);
int nr_embed_gather_bwd(const float* dout, int ld_dout, const int32_t* ids, int n_ids, int ids_stride,
                        int cols, float* dtable, int ld_dtable, nr_stream_t stream);
/* Eval-time gather of news vectors straight into the compute dtype (src/dataset.py:68 `news_scoring[click_docs]` + the
 * cast the user encoder would do next): out[m, 0:cols] = (out_dtype) table[ids[m], 0:cols], table fp32.              */
int nr_gather_cast_fwd(const float* table, int ld_table, const int32_t* ids, int n_ids, int cols, void* out, int ld_out,
                       int out_dtype, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K3 (+K1,K2 fused)  multi-head self-attention — MultiHeadSelfAttention.forward +
 * ScaledDotProductAttention.forward, src/model/model_utils.py:39-55,78-95, with the
 * embedding lookup and the two F.dropout calls of src/model/NRMS.py:28-34 folded in.
 *   X      = dropout_in(rows of x)                         [n*L, d_model]
 *   Q|K|V  = X W_{Q|K|V}^T + b                             [n*L, 3N], N = heads*d_head
 *   per head: A = exp(QK^T/sqrt(d)) * mask_j / (sum_j + 1e-8);  ctx = A V
 *   y      = dropout_out(concat_heads ctx)                 [n*L, N]
 * No max-subtraction in the reference; the kernels use the algebraically identical stable
 * form exp(s-m)/(sum exp(s-m) + 1e-8 exp(-m)).                                             */
typedef struct {
  int n, L, d_model, heads, d_head, dtype;
  int src_kind;       /* NR_SRC_DENSE | NR_SRC_GATHER */
  const void* x;      /* dense: [n*L, ldx] dtype; gather: table [V, ldx] dtype */
  int ldx;
  const int32_t* ids; /* gather: [n*L] token ids (int32, as src/preprocess.py:52-54)        */
  float p_in;         /* dropout on X (src/model/NRMS.py:28-30); element index m*d_model + k */
  uint32_t seed_in;
  float p_out;        /* dropout on y (src/model/NRMS.py:32-34); element index m*N + c       */
  uint32_t seed_out;
  const float* mask;  /* [n, L] key-side 0/1 mask or NULL (src/model/model_utils.py:50-51)   */
  const void* w_qkv;  /* [3N, ldw] dtype: rows W_Q | W_K | W_V (nr_cast_pad of each)         */
  int ldw;
  const float* b_qkv; /* [3N] fp32 */
  void* x_rows;       /* optional [n*L, ld_rows] dtype (ld_rows >= d_model rounded up to a chunk): with a gather
                         source nr_mhsa_fwd stores the gathered + dropped-out rows X here and nr_mhsa_bwd reads
                         them back as a dense operand of the weight-gradient GEMM (no second gather / RNG pass);
                         NULL: backward regenerates X from (table, ids, seed_in).                            */
  int ld_rows;
  int32_t* row_ws;    /* optional scratch of nr_mhsa_workspace_bytes(d) bytes (bf16 gather source only).  Padding tokens (id 0) gather the
                         zero row of the table: nr_mhsa_fwd (when x_rows is given too) compacts the other rows on the
                         device, projects those alone and writes the bias into the rest (if table row 0 is not zero every
                         row is kept); nr_mhsa_bwd compacts again and runs the dX GEMM over the rows that reach the
                         table gradient; a pass over dy flags the sequences with a non-zero upstream gradient and the
                         weight-gradient GEMM contracts only the 32-row slabs that touch one (the rest of dQ|dK|dV is exactly
                         zero); all-padding sequences that no live slab comes near are left out of the backward attention altogether
                         (their dQ|dK|dV rows stay unwritten and are never read).  No host synchronisation.  NULL: every row
                         goes through the GEMMs.                    */
  size_t row_ws_bytes; /* size of row_ws in bytes: must be >= nr_mhsa_workspace_bytes(d) when row_ws != NULL (checked) */
  int table_rows;     /* gather source: rows V of the table (needed in deterministic mode only, to size dtable's shadow; else 0) */
  const void* proj_table; /* nr_mhsa_fwd only, optional [V, 3N] dtype = table . W_qkv^T + b_qkv (one nr_gemm_nt over the table):
                         eval mode (p_in == 0, bf16 gather source, qkv == NULL, no backward) gathers the projections of a token
                         from here instead of projecting every occurrence -- same values, ~V/(n*L) of the GEMM work.
                         With a mask, the y rows at MASKED query positions are unspecified (currently zero where the
                         unmasked keys form one run at 32 < L <= 64, a context vector otherwise): the consumer must apply
                         the same mask.  An all-masked sequence gives zero rows. */
  const int32_t* seq_needed; /* optional [n]: 0 = the caller will not use this sequence's output (it reaches the
                         loss through a factor 0, e.g. a masked history slot, src/model/NRMS.py:59-60, model_utils.py:28,51): its y rows
                         are written as exact zeros without being computed.  NULL: every sequence is computed.  With row_ws the
                         forward also leaves the x_rows of all-padding sequences farther than 32 / L + 2 sequences from every
                         needed one unwritten (nothing reads them): pass the SAME flags to nr_mhsa_bwd.                      */
  const int32_t* seq_nz; /* nr_mhsa_bwd only, optional [n]: 0 = the upstream gradient dy of this sequence is exactly zero (the flags
                         nr_additive_pool_bwd leaves in its workspace, see nr_pool_seq_flags); NULL: the library scans dy itself */
  int row_ws_ready;   /* nr_mhsa_bwd only: nonzero = row_ws still holds what nr_mhsa_fwd wrote for these ids (reused as is).
                         REQUIRED when nr_mhsa_fwd was given row_ws: on the bf16 title-level path the forward then leaves
                         the qkv rows of all-padding sequences unwritten (the attention kernels substitute the bias), and the
                         backward attention has to do the same ("The MHSA training plan": what each decision of
                         the forward obliges the backward to do).                                                  */
  int bwd_phase;      /* nr_mhsa_bwd only.  0: the whole backward.  1: everything but the weight / bias gradients (flags, attention
                         backward, dx / table gradient) ; 2: only dw_qkv / db_qkv, after a phase-1 call with the same
                         descriptor and row_ws.  The split lets a data-parallel host start the all-reduce of the (large)
                         table gradient while the weight-gradient GEMM still runs.  Not in deterministic mode.      */
  int y_far_unwritten; /* nr_mhsa_fwd only, with seq_needed: nonzero = the y rows of an unneeded sequence need to be ZEROS only when
                         a needed sequence lies within 32 / L + 2 sequences of it (a 32-row slab of a weight-gradient GEMM can then
                         reach them); farther ones may stay UNWRITTEN.  For callers whose only consumer of y is
                         nr_additive_pool_fwd / _bwd with the same flags on a shape for which nr_pool_contracts_slabs() says 1
                         (it never reads those rows); 0.3 GB of zero stores per step at the news level otherwise.          */
  int dy_far_unwritten; /* nr_mhsa_bwd only: nonzero = the dy rows of a sequence whose seq_nz flag is 0 are zeros only within 32 / L + 2
                         sequences of a flagged one, UNWRITTEN memory farther away (nr_pool_desc.dx_far_unwritten): the backward
                         then takes dy = 0 for every unflagged sequence without reading it.  Needs seq_nz and a descriptor for
                         which nr_mhsa_compact_rows() says 1 (refused otherwise).                                            */
} nr_mhsa_desc;

/* qkv: [n*L, 3N] dtype (saved for backward); y: [n*L, N] dtype.
 * Title-level bf16 gather sources (L <= 32, 3*d_head <= 64, 288 < d_model <= 320) run as ONE fused kernel that keeps
 * Q|K|V on chip; nr_mhsa_fwd_fused(d) returns 1 for such a descriptor, and then qkv may be NULL (inference: the
 * projections are never written to HBM).  On every other path qkv is required.                              */
int nr_mhsa_fwd_fused(const nr_mhsa_desc* d);
/* 1 when nr_mhsa_fwd / nr_mhsa_bwd keep x_rows and dqkv in compact row storage for this descriptor (bf16 gather source with
 * x_rows and row_ws, title-level shapes): only then may dy_far_unwritten be used.  The exported field of the plan both
 * calls share ("The MHSA training plan").                                                              */
int nr_mhsa_compact_rows(const nr_mhsa_desc* d);
/* Bytes of row_ws that nr_mhsa_fwd / nr_mhsa_bwd use for this descriptor (depends on n and L only). */
size_t nr_mhsa_workspace_bytes(const nr_mhsa_desc* d);
int nr_mhsa_fwd(const nr_mhsa_desc* d, void* qkv, void* y, nr_stream_t stream);
/* dy [n*L, N] dtype.  dqkv: workspace [n*L, 3N] dtype.  w_qkv_t: [Kp, ldwt] dtype = w_qkv^T
 * (nr_cast_pad transpose=1; Kp = d_model rounded up to a chunk; needed only if dx/dtable).
 * dw_qkv [3N, d_model], db_qkv [3N]: fp32, accumulated.  dx: dense source -> [n*L, ldx] dtype
 * or NULL; dtable: gather source -> [V, d_model] fp32 accumulated (skips id 0) or NULL.
 * dtable may be NULL on every gather path, compact row storage included (a frozen table: dw_qkv / db_qkv only). */
int nr_mhsa_bwd(const nr_mhsa_desc* d, const void* qkv, const void* dy, void* dqkv, const void* w_qkv_t,
                int ldwt, float* dw_qkv, float* db_qkv, void* dx, float* dtable, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The attention core alone -- ScaledDotProductAttention.forward, src/model/model_utils.py:39-55 -- on given
 * projections.  qkv: [n*L, 3N] dtype, token-major, columns Q | K | V with head h at [h*d_head, (h+1)*d_head) of each
 * (the layout nr_mhsa_fwd produces; the Python surface class packs the reference's [n, h, L, d] views into it).
 * mask: [n, L] key-side 0/1 or NULL.  y: [n*L, N] dtype, heads concatenated (src/model/model_utils.py:94).
 * p_out / seed_out: optional dropout on y (element index m*N + c), 0 = none.
 * bwd: dqkv [n*L, 3N] dtype = gradient of the three projections given dy [n*L, N].
 * Input domain (here and in nr_mhsa_fwd / nr_mhsa_bwd with a materialised Q|K|V): scores s = q.k / sqrt(d_head) with
 * |s| <= 60, and the maximum over ALL keys of a row at most 45 above the maximum over its VALID keys.  The kernels factor
 * the row maximum out of exp(s) and take it over every key, masked ones included: a masked key more than ~87 above every
 * valid key under a maximum above ~60 makes the valid terms and the scaled 1e-8 underflow in fp32, and the result is then
 * not the reference's.  (The gathering forward, proj_table, takes the maximum over the valid keys of a one-run mask.)   */
int nr_sdpa_fwd(const void* qkv, const float* mask, void* y, int n, int L, int heads, int d_head, int dtype, float p_out,
                uint32_t seed_out, nr_stream_t stream);
int nr_sdpa_bwd(const void* qkv, const float* mask, const void* dy, void* dqkv, int n, int L, int heads, int d_head,
                int dtype, float p_out, uint32_t seed_out, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Sequence lengths, per entry point (L = tokens of one sequence; the clicked history at the user level):
 *   nr_sdpa_fwd / nr_sdpa_bwd            1 <= L <= 64 ("bad shape" beyond; unchanged)
 *   nr_sdpa_long_fwd / nr_sdpa_long_bwd  64 < L <= 128 only; any other L is refused before any launch
 *   nr_mhsa_fwd / nr_mhsa_bwd            1 <= L <= 128 (materialised Q|K|V); proj_table stays L <= 64; padding-token
 *                                        substitution, sequence lists and compact rows (row_ws paths) stay L <= 32, the fused
 *                                        title kernel L <= 32
 *   nr_additive_pool_fwd / _bwd          1 <= L <= 128; the fused pooling kernels and the live-slab weight gradient stay L <= 32
 * Routes of the attention core at 64 < L <= 128:
 *   bf16, d_head % 4 == 0, d_head <= 32, qkv / y / dy / dqkv 8-byte aligned: matrix-core kernels, the score matrix as RB x RB
 *     tiles of 32 x 32, RB = ceil(L / 32) (profiler labels attn_long_fwd[bf16, / attn_long_bwd[bf16,)
 *   everything else (fp32; bf16 with a misaligned buffer or d_head % 4 != 0): the LDS/VALU kernels (attn_fwd[ / attn_bwd[),
 *     d_head in {4, 8, 16, 20, 32}
 * Same softmax, same mask-after-exp, same output dropout counters (element index m*N + c) and the same input domain as
 * nr_sdpa_*: |s| <= 60, row maximum over all keys at most 45 above the maximum over the valid keys.  An all-masked sequence
 * gives exact zeros.  No atomics: a repeated call is bit-identical.
 * The pooling core at 64 < L <= 128 gives each lane of its softmax wave two tokens (lane, lane + 64), summed in a fixed order. */
int nr_sdpa_long_fwd(const void* qkv, const float* mask, void* y, int n, int L, int heads, int d_head, int dtype, float p_out,
                     uint32_t seed_out, nr_stream_t stream);
int nr_sdpa_long_bwd(const void* qkv, const float* mask, const void* dy, void* dqkv, int n, int L, int heads, int d_head,
                     int dtype, float p_out, uint32_t seed_out, nr_stream_t stream);

/* Index validation (what torch's embedding / cross_entropy raise IndexError for; the kernels themselves trust their
 * indices).  Counts the entries of ids[i*stride], i < count, outside [0, rows) into *bad (DEVICE int32, accumulated:
 * zero it first).  nr_check_labels does the same for int64 labels outside [0, classes), compared as int64 (2^32 is
 * bad, not 0).  rows / classes == 0 makes every entry bad; count == 0 launches nothing.  The Python layer calls them
 * when ops.CHECK_INDICES is on and raises IndexError.                                                            */
int nr_check_ids(const int32_t* ids, int count, int stride, int rows, int32_t* bad, nr_stream_t stream);
int nr_check_labels(const int64_t* label, int count, int classes, int32_t* bad, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K4 (+K1,K2 fused)  Conv1d(D, N, kernel_size=3, padding=1) over title tokens,
 * src/model/NAML.py:27-32,47-54: row gather of a [T*D] title-embedding row per news id,
 * dropout, im2col-free GEMM against the tap-major packed weight.  y [n*T, N] dtype.         */
typedef struct {
  int n, T, D, Dp, N, dtype;
  const void* table;  /* [V, T*Dp] dtype (nr_cast_pad of the [V*T, D] view with ld_dst = Dp) */
  const int32_t* ids; /* news ids, id of row i = ids[i*ids_stride] (src/model/NAML.py:47)    */
  int ids_stride;
  float p_in;         /* dropout on the gathered [T, D] block (src/model/NAML.py:51-53); element index (i*T+t)*D + d */
  uint32_t seed_in;
  const void* w_pack; /* [N, 3*Dp] dtype (nr_pack_conv_w) */
  const float* bias;  /* [N] */
  void* x_rows;       /* optional scratch [n*(T+1)+1, Dp] dtype: the forward stores the token rows (gather + dropout) here
                         once -- token t of title i at row i*(T+1)+1+t, zero rows in between -- so that the im2col row of
                         a token is 3*Dp CONTIGUOUS elements starting one row above it, and runs the LDS-DMA GEMM on those
                         overlapping rows (no 3x im2col copy); a backward given the same buffer reuses them.
                         NULL: the operand is gathered on the fly inside the GEMMs.                                   */
  int ld_rows;        /* == Dp */
  int32_t* bwd_ws;    /* optional backward scratch of nr_conv_workspace_bytes(d) bytes (bf16, with x_rows): nr_conv1d_k3_bwd flags the
                         titles whose upstream gradient dy is not all zero and contracts only the 32-row slabs that touch
                         one (masked history slots have an exactly zero dy).  NULL: every row is contracted.          */
  size_t bwd_ws_bytes; /* size of bwd_ws in bytes, >= nr_conv_workspace_bytes(d) when bwd_ws != NULL (checked)              */
  const int32_t* seq_nz; /* nr_conv1d_k3_bwd only, optional [n]: 0 = dy of this title is exactly zero (see nr_pool_seq_flags)  */
  const int32_t* seq_needed; /* optional [n]: 0 = the caller will not use this title's output (see nr_mhsa_desc).  nr_conv1d_k3_fwd
                         does not compute row tiles made of such titles only -- their y rows stay UNWRITTEN, the consumer
                         (nr_additive_pool_fwd / _bwd with the same flags) never reads them -- and, on shapes whose backward
                         contracts live slabs only, does not store the x_rows of titles far from every needed one;
                         nr_conv1d_k3_bwd must then be given the same flags and bwd_ws                                         */
  int table_rows;     /* nr_conv1d_k3_bwd_table / nr_conv_table_workspace_bytes only: rows V of the table; else 0               */
} nr_conv_desc;
size_t nr_conv_workspace_bytes(const nr_conv_desc* d);
int nr_conv1d_k3_fwd(const nr_conv_desc* d, void* y, nr_stream_t stream);
/* dw_pack [N, 3*Dp] fp32 accumulated (nr_unpack_conv_dw -> [N, D, 3]); db [N] accumulated.
 * The gradient of a trainable title-embedding table is a call of its own: nr_conv1d_k3_bwd_table.   */
int nr_conv1d_k3_bwd(const nr_conv_desc* d, const void* dy, float* dw_pack, float* db, nr_stream_t stream);
/* Gradient of a trainable title-embedding table (freeze_embedding=False, the default of src/parameters.py:47; src/model/NAML.py:104-107):
 *   dx[s,t,:] = sum_j W_j^T dy[s,t-j+1,:] ;  dtable[id_s, t*D + c] += keep(s,t,c) * scale * dx[s,t,c]   for id_s != 0.
 * dtable: fp32 [table_rows, T*D] contiguous, ACCUMULATED.  dy [n*T, N] dtype; w_t_pack [D, ldwt] dtype (nr_pack_conv_w_t).
 * Reads of the descriptor: n, T, D, N, dtype, ids, ids_stride, p_in, seed_in (the forward's), seq_nz (optional), table_rows.
 * Titles with id 0 or outside [0, table_rows), and titles whose seq_nz flag is 0, are not computed.  All occurrences of one news id
 * are summed by one workgroup in batch order and added with plain stores: no atomics, the result is bit-identical from run to
 * run in every mode (nr_set_deterministic needs no scratch for dtable here).
 * Size: dtable is addressed with 64-bit offsets, so tables of 2^31 elements and more (V*T*D*4 bytes > 4 GiB from V ~ 120 000 at
 * T*D = 9 000) are handled; refused on the host before any launch are table_rows * T >= 2^31 and n*T*max(D, N) >= 2^32.
 * ws: nr_conv_table_workspace_bytes(d) bytes of scratch, 16-byte aligned (checked before any launch).             */
size_t nr_conv_table_workspace_bytes(const nr_conv_desc* d);
int nr_conv1d_k3_bwd_table(const nr_conv_desc* d, const void* dy, const void* w_t_pack, int ldwt, float* dtable, void* ws, size_t ws_bytes,
                           nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K5  additive attention pooling — AttentionPooling.forward, src/model/model_utils.py:13-31
 *   e = tanh(x W1^T + b1); a = exp(e w2 + b2) * mask; a /= sum_L a + 1e-8; out = sum_L a x   */
typedef struct {
  int n, L, N, q, dtype;
  const void* x;     /* [n*L, N] dtype */
  const float* mask; /* [n, L] or NULL */
  const void* w1;    /* [q, ldw1] dtype */
  int ldw1;
  const float* b1;   /* [q] */
  const float* w2;   /* [q] (att_fc2.weight [1, q]) */
  const float* b2;   /* [1] */
  size_t partial_bytes; /* nr_additive_pool_bwd: size of `partial` in bytes, >= nr_pool_workspace_bytes(d) (checked) */
  const int32_t* seq_needed; /* optional [n]: 0 = this sequence's output is not used by the caller.  nr_additive_pool_fwd writes its
                         out row and alpha as zeros and may leave its e rows unwritten; nr_additive_pool_bwd must be given the same
                         flags: the pooled gradient of such a sequence is zero by contract, its dpre / dx rows are written as zeros
                         and its e rows are never read                                                                       */
  int dx_far_unwritten; /* nr_additive_pool_bwd: nonzero = the dx rows of a sequence with a zero pooled gradient need to be zeros only
                         within 32 / L + 2 sequences of one with a gradient; farther ones MAY stay unwritten (0.2 GB of zero stores
                         per step at the news level).  For a caller that hands dx, together with the flags of nr_pool_seq_flags,
                         to nr_mhsa_bwd with dy_far_unwritten set -- nothing else may read those rows.                       */
} nr_pool_desc;
/* 1 when nr_additive_pool_bwd contracts only the 32-row slabs that touch a sequence with a non-zero pooled gradient for this
 * descriptor (n, L, N, q, dtype are read): it then never reads x rows farther than 32 / L + 2 sequences from such a sequence
 * (see nr_mhsa_desc.y_far_unwritten).  0: its weight-gradient GEMM reads every row of x.                                  */
int nr_pool_contracts_slabs(const nr_pool_desc* d);
/* Bytes of the `partial` workspace of nr_additive_pool_bwd. */
size_t nr_pool_workspace_bytes(const nr_pool_desc* d);
/* After nr_additive_pool_bwd (bf16, L <= 32, rows a multiple of 32): the [n] int32 flags inside `partial` that say which
 * sequences had a non-zero pooled gradient g -- exactly the sequences whose dx rows are non-zero.  The producer of x can
 * take them as its `seq_nz` instead of scanning dx.  Returns NULL when this descriptor does not produce flags.        */
const int32_t* nr_pool_seq_flags(const nr_pool_desc* d, const float* partial);
/* e: [n*L, q] dtype (tanh output, saved); alpha: [n*L] fp32 (saved); out: fp32, row i at out + i*ld_out. */
int nr_additive_pool_fwd(const nr_pool_desc* d, void* e, float* alpha, float* out, int ld_out, nr_stream_t stream);
/* g: fp32 d(out), row i at g + i*ld_g.  w1_t [N, ldw1t] dtype = w1^T.  dpre: workspace [n*L, q] dtype.
 * partial: workspace of nr_pool_workspace_bytes(d) bytes, fp32 (one row per workgroup; small n uses one sequence per workgroup; at the news level the
 *          unused tail holds the int32 flags / live-slab list of the sequences whose pooled gradient g is not all zero --
 *          sequences with g == 0 get exact zeros in dpre / dx and are skipped by the att_fc1 weight gradient).
 * dw1 [q,N], db1 [q], dw2 [q], db2 [1]: accumulated.
 * dx: [n*L, N] dtype (overwritten) or NULL.                                                  */
int nr_additive_pool_bwd(const nr_pool_desc* d, const void* e, const float* alpha, const float* g, int ld_g,
                         const void* w1_t, int ldw1t, void* dpre, float* partial, float* dw1, float* db1,
                         float* dw2, float* db2, void* dx, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K6  pad-doc blend — src/model/NRMS.py:59-60, src/model/NAML.py:94-95:
 *   out = x*m + pad*(1-m), written as dtype (the GEMM operand of the user-level ops).
 * mask == NULL: plain fp32 -> dtype cast (user_log_mask=True path).
 * bwd: dx = dout*m (fp32); dpad[c] += sum (1-m) dout (accumulated).                          */
int nr_pad_blend_fwd(const float* x, const float* mask, const float* pad, void* out, int n, int L, int N,
                     int dtype, nr_stream_t stream);
int nr_pad_blend_bwd(const void* dout, const float* mask, float* dx, float* dpad, int n, int L, int N,
                     int dtype, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K7  gather + Linear — category / subcategory view, src/model/NAML.py:19-24,60-68:
 *   out[m, :] = rows(x)[m, :] W^T + b      (fp32 out, row m at out + m*ld_out)               */
typedef struct {
  int M, K, N, dtype;
  int src_kind;
  const void* x; /* dense [M, ldx] dtype or table [V, ldx] dtype */
  int ldx;
  const int32_t* ids;
  int ids_stride;
  const void* w; /* [N, ldw] dtype */
  int ldw;
  const float* bias; /* [N] or NULL */
  const void* w_t;   /* [K, ldwt] dtype = w^T; only read by nr_linear_bwd when dtable != NULL */
  int ldwt;
  size_t dout_ws_bytes; /* nr_linear_bwd: size of dout_ws in bytes, >= nr_linear_workspace_bytes(d) (checked) */
  int table_rows;    /* gather source: rows V of the table (deterministic mode only, see nr_set_deterministic; else 0) */
} nr_linear_desc;
size_t nr_linear_workspace_bytes(const nr_linear_desc* d);
int nr_linear_fwd(const nr_linear_desc* d, float* out, int ld_out, nr_stream_t stream);
/* dout fp32 (row stride ld_dout); dout_ws: workspace of nr_linear_workspace_bytes(d) bytes ([M, Nc] dtype, Nc = N rounded
 * up to a chunk).
 * dw [N, K], db [N] accumulated; dtable [V, K] fp32 accumulated (gather source, skips id 0) or NULL. */
int nr_linear_bwd(const nr_linear_desc* d, const float* dout, int ld_dout, void* dout_ws, float* dw,
                  float* db, float* dtable, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K8  candidate scorer + cross-entropy — torch.bmm + nn.CrossEntropyLoss,
 * src/model/NRMS.py:77,93-94, src/model/NAML.py:111,128-129.
 *   score[b, j] = <cand[b, j, :], user[b, :]>;  loss = mean_b -log softmax(score[b])[label[b]]
 * cand row (b, j) at cand + (b*C + j)*ld_cand.  lossvec: workspace fp32 [B].                 */
int nr_score_ce_fwd(const float* cand, int ld_cand, const float* user, const int64_t* label, float* score,
                    float* loss, float* lossvec, int B, int C, int N, nr_stream_t stream);
/* gloss: DEVICE pointer to the scalar d(loss) (no host sync); gscore: optional [B, C] d(score) added to
 * the cross-entropy term, or NULL.  dcand row (b, j) at dcand + (b*C + j)*ld_dcand; duser [B, N].        */
int nr_score_ce_bwd(const float* cand, int ld_cand, const float* user, const int64_t* label,
                    const float* score, const float* gloss, const float* gscore, float* dcand, int ld_dcand,
                    float* duser, int B, int C, int N, nr_stream_t stream);
/* Eval-time scorer (src/main.py:253): variable-length candidate lists.
 * score[i] = <news_vecs[cand_ids[i]], user[imp_of[i]]>, i in [0, n_cand).                     */
int nr_score_eval(const float* news_vecs, int ld_news, const int32_t* cand_ids, const int32_t* imp_of,
                  const float* user, int ld_user, float* score, int n_cand, int N, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K9  full-corpus top-k recommendation.  The reference only ever scores the candidate lists a behaviors.tsv supplies
 * (src/main.py:253 `np.dot(news_vec, user_vec)` over the `news_scoring[candidate]` rows of src/dataset.py:64-74); this call
 * generalises that dot product to EVERY news of the table and keeps, per user, the k best:
 *   score[u, v] = <news_vecs[v], user[u]>, fp32 operands, fp32 accumulation (v_mfma_f32_16x16x4_f32), v in [1, V)
 *   out_ids[u, :], out_scores[u, :] = the k best eligible news of user u in the total order
 *                                     (score descending, then news id ascending)
 * Row 0 of news_vecs is the unknown / padding news and is never returned.  exclude (optional, [U, E] int32, row stride
 * ld_exclude, E <= 64): ids user u must not be given, e.g. the clicked history; entries that are 0 or outside [1, V) are
 * ignored, duplicates are allowed.  A news whose score is NaN is never returned and does not disturb the others.  With fewer
 * than k eligible news the tail of the row is id 0, score -inf.
 * Special values, as the chain and the keys give them (K10 ranks by the same rules; tests/test_gpu_corpus_sweep.py holds each):
 *   -0         the accumulator starts at +0, so a dot product is -0 only when every product of the chain rounds to -0.  A score
 *              of -0 compares equal to +0: the two tie (news id ascending) and both come back as +0 in out_scores.
 *   subnormal  products and partial sums below 2^-126 are kept as fp32 subnormals, never flushed to zero: the score is the fmaf
 *              chain with gradual underflow, exact where the products and sums are representable.
 *   +-inf      an infinite score is a score like any other: a chain that overflows, an infinite component or a prior of +inf
 *              give +inf or -inf, ordered with everything else (ties by id).  A news whose score is -inf is eligible: it comes
 *              back WITH ITS ID behind every finite score (and is ranked and counted by K10), unlike the fill, whose id is 0.
 *              (-inf) + (+inf) is NaN and falls under the NaN rule.
 * One (u, v) score is one fmaf chain over the vector width in a fixed order: its bits are the same in any user tile, in any
 * corpus slice and for any `splits` (they need not equal nr_score_eval's, which sums in another order).
 * Two launches: the fused scoring + selection pass over a grid of user tiles x `splits` corpus slices, then a per-user merge
 * of the slices' lists.  No [U, V] buffer exists anywhere: ws is U * splits * k * 8 bytes.
 *   N        vector width, a multiple of 4, at most 1024; ld_news, ld_user multiples of 4, buffers 16-byte aligned
 *   k        1 .. 128
 *   splits   0: the library chooses (fills the chip for few users, 1-2 for many); > 0: that many slices, at most
 *            min(256, 8192 / k)
 *   ws       nr_score_topk_workspace_bytes(d) bytes, 8-byte aligned (the size depends on U, V, N, k, splits only; 0 = bad
 *            descriptor -- a refused group / group_cap pairing included --, see nr_last_error)
 * Pools (optional; all zero = off, and the call is then the one it was before they existed, bit for bit).  Shared with
 * nr_score_rank, one definition (pool_key, csrc/nr_score_tile.h):
 *   prior    [V] fp32.  score[u, v] = fl32(dot[u, v] + prior[v]): dot is the finished fmaf chain above, its bits unchanged;
 *            the prior is ONE separate fp32 add after it, not a chain step and not contracted into an fma.  out_scores are
 *            these sums.  prior[v] == -inf makes news v ineligible for every user (the global pool switch); a NaN prior gives
 *            a NaN score, which falls under the NaN rule above; any other value just follows the arithmetic.
 *   stamp    [V] int32 and window [U, 2] int32 (row stride ld_window >= 2): news v is eligible for user u only if
 *            window[u, 0] <= stamp[v] <= window[u, 1], both ends inclusive.  lo > hi is an empty pool: the row is all fill.
 *            The two come together: one without the other is refused.
 * Eligible then means all of: id in [1, V), id not in exclude[u], score not NaN, prior not -inf, stamp inside the window.
 * Order, fill and the independence of `splits` are unchanged; the workspace size does not depend on these fields.
 * Group caps (optional; group == NULL with group_cap == 0 = off, and the call is then today's, bit for bit, on the kernel
 * instantiations it always launched): "at most c news of one category in the row".
 *   group      [V] int32, one group id per news; a negative id = belongs to no group, never capped
 *   group_cap  c in [1, NR_TOPK_MAX_K]
 * The row of user u is then: walk u's eligible news in the total order above (score descending, news id ascending); take a
 * news unless group[v] >= 0 and c news of that group are already taken; stop after k.  Everything else is as without caps:
 * eligible means what it means above (id in [1, V), not excluded, score not NaN, prior not -inf, stamp inside the window), and
 * an ineligible news uses up nothing of its group's cap; the score is fl32(dot + prior), the same fmaf chain, the same bits;
 * the fill is id 0 / -inf when fewer than k news can be taken (G groups, no ungrouped news and G * c < k: at most G * c
 * entries); the row does not depend on `splits`, the user tile or the place in it.  c >= k and an all-negative `group` give
 * the rows of the plain call.  `group` without a cap in [1, 128], or a cap without `group`, is refused (nr_last_error).
 * The cap lives inside the selection (one exchange per candidate) and in the merge, which walks the sorted
 * slice lists with the same rule; the workspace size does not depend on these fields either.
 * Slow case, exact but not fast: while a user's list cannot fill (G * c < k and few ungrouped news) its threshold never
 * rises, and every chunk of the corpus goes through the per-candidate path for that user.
 * nr_score_rank knows the same caps (K10, group / group_cap / n_groups): with equal inputs its capped rank is the place in this
 * row.  Without them it describes the uncapped ranking, of which a capped row is a subsequence: the uncapped rank of the
 * entry at place p (0-based) is >= p + 1, the ranks along a row increase strictly, and the scores are the rank pass's bit
 * for bit.
 * Exclusion lists of any length (optional; excl_offsets == NULL, excl_ids == NULL, n_excl == 0 = off, and the call then
 * launches the kernel instantiations it always launched).  Shared with nr_score_rank.  The dense list above stops at 64 ids;
 * "everything this user has been shown" is hundreds to thousands, so it comes in CSR form:
 *   excl_offsets  [U + 1] int32, non-decreasing: user u's list is excl_ids[excl_offsets[u] .. excl_offsets[u + 1])
 *   excl_ids      [n_excl] int32 news ids; each user's segment STRICTLY ascending (sorted, no repeats)
 *   n_excl        entries of excl_ids
 * Eligible then additionally means "not in user u's segment"; order, fill, NaN rule, pools, group caps, the independence of
 * `splits` and the workspace size are unchanged.  Entries of a segment that are <= 0 or >= V mean nothing (in a sorted segment
 * they sit at its two ends).  A segment that is not strictly ascending gives unspecified rows for that user, but never an
 * access outside excl_ids[0 .. n_excl): the kernels clamp every segment bound into [0, n_excl] (the library cannot check
 * device arrays on the host and does not synchronise to do so).  One list form per call: E > 0 together with excl_offsets,
 * excl_offsets without excl_ids or the reverse (unless n_excl == 0), and n_excl < 0 are refused (nr_last_error).
 * The list is served in the slow path of the selection only: an entry there finds the lower bound of the chunk's first id
 * in the user's segment with a wave-wide search (64 probes a step, ceil(log64 L) dependent loads) and keeps the at most 128
 * entries that can fall into the chunk in two registers per lane.  No LDS, so the user tile, the slices, the workspace and
 * the merge kernels are those of the plain call.
 * Slow case, exact but not fast (as with group caps): a user whose segment covers nearly the whole corpus never fills its
 * list, its threshold never rises, and every chunk goes through the per-candidate path for that user.
 * Layout: excl_offsets, excl_ids, n_excl sit behind `E`, in front of `splits` (n_excl and splits share one 8-byte slot); group
 * and group_cap sit with the other inputs of the selection rule, behind `splits`; nr_topk_desc and nr_rank_desc
 * keep ending in the shared tail ws, ws_bytes, prior, stamp, window, ld_window.  nr_abi_sizes follows by sizeof.           */
#define NR_TOPK_MAX_K 128
#define NR_TOPK_MAX_N 1024
#define NR_TOPK_MAX_EXCLUDE 64
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N, k;
  const int32_t* exclude;
  int ld_exclude, E;
  const int32_t* excl_offsets; /* optional [U + 1], non-decreasing: user u's list is excl_ids[excl_offsets[u] .. excl_offsets[u+1]) */
  const int32_t* excl_ids;     /* optional [n_excl] news ids; each user's segment STRICTLY ascending (sorted, no repeats) */
  int n_excl;                  /* entries of excl_ids; the kernels clamp every segment bound into [0, n_excl] */
  int splits;
  const int32_t* group;  /* optional [V]: group id per news, negative = no group; with group_cap */
  int group_cap;         /* 1 .. NR_TOPK_MAX_K with group, 0 without */
  int32_t* out_ids;
  float* out_scores;
  void* ws;
  size_t ws_bytes;
  const float* prior;    /* optional [V] */
  const int32_t* stamp;  /* optional [V]; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_topk_desc;
size_t nr_score_topk_workspace_bytes(const nr_topk_desc* d);
int nr_score_topk(const nr_topk_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K10  full-corpus rank evaluation.  The reference evaluates by re-ranking the candidates of one impression
 * (src/main.py:249-263: `np.dot(news_vec, user_vec)` over `news_scoring[candidate]`, then src/metrics.py:6-24 mrr_score /
 * ndcg_score on those few dozen scores); this call ranks a user's held-out clicks against EVERY news of the table, the
 * retrieval counterpart of nr_score_topk:
 *   rank[u, j]  = 1-based position of news targets[u, j] among the eligible news of user u in nr_score_topk's total order
 *                 (score descending, then news id ascending); eligible = ids 1 .. V-1 that are not in exclude[u] and whose
 *                 score is not NaN
 *   rank[u, j]  = 0 ("not ranked"), score -inf, when the target is 0 or outside [1, V), is excluded, has a NaN score, or
 *                 repeats an earlier entry of its row
 * Scores are those of nr_score_topk bit for bit (one fmaf chain per (u, v), the same instruction sequence), so
 * 1 <= rank[u, j] <= k holds exactly when targets[u, j] is in the top-k row of user u, at place rank - 1.
 *   targets     [U, T] int32, row stride ld_targets, T in 1 .. 64
 *   exclude     as in nr_topk_desc (optional, [U, E], E <= 64)
 *   ks, n_ks    HOST array of n_ks <= 8 cut-offs k >= 1 for out_sums (n_ks may be 0)
 *   out_ranks   [U, T] int32;  out_scores [U, T] fp32
 *   out_sums    optional DEVICE fp64 [2 + 2 n_ks], OVERWRITTEN: [0] = users with n_u >= 1 ranked targets, [1] = sum MRR_u, then per
 *               k: sum Recall@k_u, sum nDCG@k_u over those users, with (src/metrics.py:6-24 on the user's whole eligible row,
 *               binary labels)  MRR_u = mean_j 1 / rank,  Recall@k_u = #{rank <= k} / n_u,
 *               nDCG@k_u = sum_{rank <= k} 1 / log2(rank + 1)  /  sum_{i = 1 .. min(n_u, k)} 1 / log2(i + 1);
 *               fp64, reduced in a fixed order (bit-reproducible)
 *   N, ld_news, ld_user, splits: as in nr_topk_desc (splits at most 256); the result does not depend on splits
 *   ws          nr_score_rank_workspace_bytes(d) bytes, 8-byte aligned (the query reads U, V, N, T, E, n_ks, ks, splits; 0 = bad
 *               descriptor, see nr_last_error): O(U * T * splits), no [U, V] buffer exists anywhere
 * Three launches (+ one for out_sums): the scores of the named ids (targets and excluded news, gathered rows through the same
 * MFMA tile), the counting pass over user tiles x corpus slices, and a per-user finalize.
 * Pools: prior, stamp, window, ld_window exactly as in nr_topk_desc (all zero = off: the call as it was, bit for bit; one
 * of stamp / window without the other is refused).  The score is fl32(dot + prior), the eligible news are additionally those
 * whose prior is not -inf and whose stamp lies in the user's window, and a target outside its user's pool is "not ranked":
 * rank 0, score -inf.  An excluded id that is itself outside the pool takes nothing off a rank (it was never counted).  The
 * statement "1 <= rank <= k exactly when the target is at place rank - 1 of the top-k row" holds for equal pool inputs.
 * Exclusion lists of any length: excl_offsets, excl_ids, n_excl exactly as in nr_topk_desc (all zero = off: the kernels the
 * call always launched; the same refusals).  A target found in its user's segment is "not ranked"; a listed news takes one
 * off the rank of every target it beats, if it is in range and eligible (not NaN, inside the pool).  The named-id pass then
 * takes a user's list through further chunks of 128 gathered rows (the first 64 ids ride with the targets); the counting
 * pass, the finalize pass and the workspace are unchanged.  The agreement with nr_score_topk holds for equal lists.
 * Group caps (optional; group == NULL, group_cap == 0, n_groups == 0 = off: the call as it is without them -- the same
 * launches, the same workspace bytes): the rank in the CAPPED ranking nr_score_topk(..., group, group_cap) serves.
 *   group      [V] int32, one group id per news; a negative id = belongs to no group (as in nr_topk_desc)
 *   group_cap  c in [1, NR_TOPK_MAX_K]
 *   n_groups   G in [1, NR_RANK_MAX_GROUPS]: the group ids lie in [0, G)
 *   T          at most NR_RANK_MAX_CAPPED_TARGETS per row in a capped call (lay a user with more over several rows)
 * "Eligible" means what it means above: id in [1, V), not excluded (dense list or CSR list), score not NaN, prior not -inf,
 * stamp inside the user's window.  For user u and target t, in the total order (score descending, id ascending), let n_g(t)
 * be the number of eligible news of group g that beat t and n_-(t) the number of eligible ungrouped news that beat t; the
 * uncapped rank is 1 + n_-(t) + sum_g n_g(t).  The capped walk of nr_score_topk takes exactly the first c news of each
 * group, so
 *   t is CAPPED OUT when group[t] >= 0 and n_{group[t]}(t) >= c: it is in no capped row for any k;
 *   otherwise capped_rank(t) = 1 + n_-(t) + sum_g min(c, n_g(t)) = uncapped_rank(t) - sum_g max(0, n_g(t) - c).
 * What is not eligible uses up nothing of a cap (an excluded or listed id, a NaN news, a news outside the pool): the
 * named-id pass takes back, PER GROUP, the excluded / listed news that beat the target (in range and with key != 0 only, each
 * once), and the stream never counts a key-0 news.
 *   out_ranks   the capped rank; 0 with score -inf for what is not ranked today (no entry, out of range, excluded, NaN, outside
 *               the pool, a repeat); -1 WITH ITS FINITE SCORE for a capped-out target: a legitimate held-out click that this
 *               recommender can never show
 *   out_sums    n_u counts the targets with rank != 0; a rank of -1 adds nothing to MRR, Recall@k or nDCG@k; the ideal DCG
 *               stays sum_{i <= min(n_u, k)} 1 / log2(i + 1) -- the ideal is what an uncapped recommender could have shown,
 *               so a cap that hides clicks lowers nDCG@k instead of shrinking its denominator.  Without a negative rank the
 *               sums are what they are without caps, bit for bit.
 * For equal inputs, 1 <= capped_rank <= k exactly when the target is at place capped_rank - 1 of the row of
 * nr_score_topk(..., group, group_cap), with identical score bits, for every k <= 128.
 * Refused (nr_last_error): group without a cap in [1, 128]; a cap, or n_groups, without group; n_groups outside [1, 512]
 * with group; T > NR_RANK_MAX_CAPPED_TARGETS with group.  A group id >= n_groups gives unspecified ranks for the users it
 * concerns, never an access outside the workspace: the kernels treat such a news as ungrouped (the library does not
 * synchronise to validate device arrays, as with the CSR lists).
 * Cost: one prep launch per call (two 64-bit "news of this chunk in group g" masks per chunk of 128 ids and group), one memset
 * of the [U, T, G] int32 counters, and in the counting pass about 8 VALU instructions per (chunk, user, real target, block of
 * 64 groups).  The per-(user, target, group) counters are integers, added with integer atomics once per slice: the result does
 * not depend on splits, the user tile or any arrival order.  Workspace: + U * T * (G + 2) * 4 + chunks * G * 16 bytes.
 * Layout: group, group_cap, n_groups sit behind out_sums, in front of the shared tail.                                     */
#define NR_RANK_MAX_TARGETS 64
#define NR_RANK_MAX_KS 8
#define NR_RANK_MAX_GROUPS 512
#define NR_RANK_MAX_CAPPED_TARGETS 4
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N, T;
  const int32_t* targets;
  int ld_targets;
  const int32_t* exclude;
  int ld_exclude, E;
  const int32_t* excl_offsets; /* optional [U + 1]: as in nr_topk_desc */
  const int32_t* excl_ids;     /* optional [n_excl]: as in nr_topk_desc */
  int n_excl;
  int splits;
  const int* ks; /* host */
  int n_ks;
  int32_t* out_ranks;
  float* out_scores;
  double* out_sums;
  const int32_t* group;  /* optional [V]: group id per news, negative = no group; with group_cap and n_groups */
  int group_cap;         /* 1 .. NR_TOPK_MAX_K with group, 0 without */
  int n_groups;          /* 1 .. NR_RANK_MAX_GROUPS with group, 0 without: group ids lie in [0, n_groups) */
  void* ws;
  size_t ws_bytes;
  const float* prior;    /* optional [V] */
  const int32_t* stamp;  /* optional [V]; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_rank_desc;
size_t nr_score_rank_workspace_bytes(const nr_rank_desc* d);
int nr_score_rank(const nr_rank_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K11  diversified recommendation: Maximal Marginal Relevance (Carbonell & Goldstein 1998) over a pool of the M best.  The
 * reference has nothing of the kind (it scores the candidate lists of behaviors.tsv only), so, as with K9 / K10, the contract
 * is this library's own; metrics.mmr_reference states it on the host.  One launch, no workspace, one workgroup per user.
 *   news_vecs    [V, N] fp32, row stride ld_news; N a multiple of 4, at most NR_TOPK_MAX_N; alignment as in nr_topk_desc
 *   pool_ids     [U, M] int32, row stride ld_pool_ids;  pool_scores [U, M] fp32, row stride ld_pool_scores: what
 *                nr_score_topk wrote for k = M, but any arrays are allowed
 *   M            in [1, NR_TOPK_MAX_K];  k in [1, M]
 *   penalty      scalar fp32, finite and >= 0;  penalty_u optional [U] fp32: when given it replaces the scalar, user by user
 *   group        optional [V] int32 with group_cap = c in [1, 128], together as in nr_topk_desc; a negative id = in no group
 *   out_ids      [U, k] int32;  out_scores [U, k] fp32;  out_place [U, k] int32, all contiguous
 * Place i of user u's pool is LIVE when pool_ids[u, i] is in [1, V) and pool_scores[u, i] is not NaN.  A place that is not live
 * is never taken and its id is never used as an index (nr_score_topk's fill, id 0 / -inf, is not live); a repeated id is
 * simply two places.  With x_i the news vector of place i, r_i its pool score and p_u the user's penalty, all in fp32:
 *   g(i, j)    = <x_i, x_j> over N: ONE fmaf chain in a fixed order; its bits depend on the two vectors and on N only, not on
 *                M, the place, the tile variant, U or the user's position in the grid; g(i, j) == g(j, i) bit for bit
 *   rn_i       = g(i, i) > 0 ? 1 / sqrt(g(i, i)) : 0, square root and division both correctly rounded: an all-zero vector
 *                has similarity 0 to everything and makes no NaN
 *   s(i | j)   = fl(fl(g(i, j) * rn_i) * rn_j): the cosine, as seen from candidate i
 * The walk: S = {} and k times: the candidates are the live places not yet taken (with caps: whose group is negative or has
 * fewer than c places taken so far); value_i = r_i while S is empty, afterwards fmaf(-p_u, maxsim_i, r_i) with
 * maxsim_i = max over j in S of s(i | j); the candidate with the largest value is taken, ties to the LOWEST place (for a pool
 * that nr_score_topk sorted: score descending, then id ascending); no candidate ends the walk.
 *   out_ids    the ids taken, in the order taken;  out_scores their r_i (the relevance, not the MMR value);  out_place their
 *              places in the pool, 0-based;  the tail of a short row is id 0, score -inf, place -1
 * Consequences: with p_u = 0 the row is the pool walked in (score descending, place ascending) order under the cap -- for a
 * sorted pool without caps its first k places, bit for bit.  A row depends only on that user's pool row, its p_u and the
 * vectors that row names.  Values of -0 and +0 tie (the lowest place wins); out_scores returns the pool's own bits, a -0
 * included; a pool score of -inf or +inf is a live score like any other.
 * Unspecified: non-finite vector components, or a NaN or negative entry of penalty_u, give an unspecified row for that user
 * only, never an access outside the arrays (the library cannot check device arrays and does not synchronise).
 * Refused before any launch (nr_last_error; host arithmetic only): a null descriptor or required pointer; M or k out of range;
 * N, ld_news or the alignment of news_vecs against K9's rules; a pool row stride below M; a scalar penalty that is negative or
 * not finite; group without a cap in [1, 128] or a cap without group; U < 0; V < 1.  U == 0 returns 0 without a launch.   */
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const int32_t* pool_ids;
  const float* pool_scores;
  int ld_pool_ids, ld_pool_scores;
  int U, N, M, k;
  float penalty;
  const float* penalty_u; /* optional [U]: replaces `penalty` user by user */
  const int32_t* group;   /* optional [V]: group id per news, negative = no group; with group_cap */
  int group_cap;          /* 1 .. NR_TOPK_MAX_K with group, 0 without */
  int32_t* out_ids;
  float* out_scores;
  int32_t* out_place;
} nr_mmr_desc;
int nr_mmr_select(const nr_mmr_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K12  sampled recommendation: k news WITHOUT replacement, each draw proportional to exp(score / tau_u) over what is left --
 * the Plackett-Luce model -- by the Gumbel-max trick: tau_u * g is added to every score, g an independent standard Gumbel
 * variate per (user, news), and the k largest are taken.  That is nr_score_topk with a per-(user, news) prior made in
 * registers: no [U, V] noise matrix exists.  The reference has nothing of the kind; metrics.sample_reference states the
 * contract on the host.  Every field of `topk` means what it means in K9 (pools, caps, dense and CSR lists, splits, ws).
 * The noise, for user key a (uint32), news id v, seed (uint64) and draw (uint32):
 *   bits(a, v) = Philox4x32-10(counter = (v >> 2, a, draw, 0), key = (seed & 0xffffffff, seed >> 32))[v & 3]
 *                (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85)
 *   u          = ((bits >> 8) + 0.5) * 2^-24, in [2^-25, 1 - 2^-25]
 *   g          = -log(-log(u)) in fp32, finite: -2.853 < g < 17.329; within 7 * 2^-23 * max(1, |g|) of the real value
 * The counter holds the GLOBAL user key and news id, so a draw does not depend on the user tile, the place in it, the corpus
 * slice, `splits`, or which batch or rank the user was put in.  user_keys names the users ([U] int32, taken as uint32; NULL =
 * the row index u): a caller who shards users over ranks or batches passes the same key for the same user and gets the same
 * draw.  `draw` gives independent rows under one seed.
 * The key:  P(u, v) = fl32(prior[v] + fl32(tau_u * g))  (prior[v] = 0 without a prior; a multiply and an add, never one fma),
 * and the final score of (u, v) is fl32(dot + P(u, v)) under the pool rules of K9.  Consequences:
 *   - a prior of -inf still switches a news off; a NaN still falls under the NaN rule;
 *   - tau_u == 0 gives the row of nr_score_topk, bit for bit;
 *   - ROW u OF A SAMPLED CALL IS ROW 0 OF nr_score_topk given user u alone with prior = P(u, .) and everything else equal:
 *     identical ids, identical score bits;
 *   - with caps the law is still the right one: walking down the perturbed order and skipping a saturated group is sequential
 *     sampling from the softmax renormalised over what may still be taken;
 *   - an entry of tau_u that is negative, NaN or infinite gives that user an all-fill row (id 0, -inf), nobody else's changes.
 *   out_scores   topk.out_scores receive the PERTURBED values the row is ordered by
 *   out_model    optional [U, k] fp32: fl32(perturbed - fl32(tau_u * g)), the model score + prior to within rounding; -inf in fill
 *   tau          scalar, used when tau_u == NULL; finite and >= 0, else refused
 * Workspace: nr_score_topk's, U * splits * k * 8 bytes (0 = bad descriptor, see nr_last_error).  The two launches of
 * nr_score_topk (the SAMPLE instantiations of the selection, the merge kernels as they are), plus a tiny finalize when
 * out_model is given.  Refused before any launch: whatever nr_score_topk refuses, and a scalar tau as above.
 * nr_sample_noise is the probe: g and bits of n (user key, news id) pairs, element-wise, DEVICE arrays; either output may be
 * NULL.  It runs the function the selection runs.                                                                       */
typedef struct {
  nr_topk_desc topk;        /* every field as in K9; out_scores receive the PERTURBED values the row is ordered by */
  uint64_t seed;
  uint32_t draw;            /* independent draws under one seed */
  float tau;                /* used when tau_u == NULL; finite, >= 0 */
  const float* tau_u;       /* optional [U] */
  const int32_t* user_keys; /* optional [U]: counter word 1; NULL = the row index u */
  float* out_model;         /* optional [U, k]: fl32(perturbed - fl32(tau_u * g)), the model score + prior to within rounding; -inf in fill */
} nr_sample_desc;
size_t nr_score_sample_workspace_bytes(const nr_sample_desc* d);
int nr_score_sample(const nr_sample_desc* d, nr_stream_t stream);
int nr_sample_noise(uint64_t seed, uint32_t draw, const int32_t* user_keys, const int32_t* news_ids, int n, float* out_g, uint32_t* out_bits,
                    nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K13  full-corpus log-partition.  What a sampled row (K12) is reweighted by is the probability it was drawn with, and that,
 * like the full-softmax log-likelihood of a held-out click, needs per user
 *   log Z_u = log sum_v exp(score(u, v) / tau_u)   over exactly the news nr_score_topk / nr_score_sample call eligible for u.
 * The reference has nothing of the kind; metrics.logz_reference states the contract on the host.  No [U, V] buffer exists.
 * Score and eligibility are K9's, through the same definition (pool_key, csrc/nr_score_tile.h): score = fl32(dot + prior),
 * the dot product the same fmaf chain, the same bits; eligible = id in [1, V), the sum not NaN, prior not -inf, stamp inside
 * the user's window, id not in the user's CSR segment.  Three results per user:
 *   out_max     [U] fp32: the largest eligible score, the bits nr_score_topk returns for k = 1; -inf when nothing is eligible
 *   out_count   [U] int32: the number of eligible news, exact
 *   out_logsum  [U] fp32: log sum_v exp((s(u, v) - out_max[u]) * (1 / tau_u)); >= 0 whenever the maximum is finite
 * and log Z_u = out_max[u] / tau_u + out_logsum[u].  The parts stay apart so that log p(v) = (s_v - max) / tau - logsum never
 * forms a large max / tau.
 *   tau         scalar, used when tau_u == NULL; finite and > 0, else refused.  tau_u: optional [U] fp32.  An entry that is
 *               <= 0, NaN or infinite gives that user out_logsum = NaN; its max and count stay valid, nobody else's row
 *               changes.  1 / tau is ONE fp32 division per user (where it overflows, for a tau at the very bottom of the fp32
 *               range, the weights are those of the limit: 1 for the maxima, 0 below).
 *   lists       excl_offsets, excl_ids, n_excl: K9's CSR lists with K9's rules (strictly ascending segments; segment bounds
 *               clamped into [0, n_excl]; an unsorted segment gives that user an unspecified result, never an access outside
 *               the arrays).  The dense [U, E <= 64] list is not part of this call.  The listed news are left out IN the
 *               stream, never subtracted afterwards: they are typically the heaviest terms of the sum.
 *   edge cases  nothing eligible: count 0, max -inf, logsum -inf.  Largest eligible score +-inf: logsum NaN, max and count as
 *               they are.  A score of -inf under a finite maximum weighs 0 and counts 1.  No NaN and no overflow when
 *               (s - max) / tau spans thousands: every exponent formed is <= 0.
 * The bits of all three depend on the inputs of that user only -- not on `splits`, the user tile, the place in it, or the
 * other users of the call.  [1, V) is cut into nseg <= 256 segments of 128 * ceil((V - 1) / (128 * 256)) ids, a function of V
 * alone; a slice is a run of whole segments; inside a segment every lane keeps a running (max, sum) over its own news (which
 * lane sees which id is fixed by the segment start), a fixed-order wave reduction leaves one (max, sum, count) partial per
 * (user, segment), and a second small kernel merges a user's partials in fp64 in a fixed order.  Two launches, no
 * float atomics, no host synchronisation.  The derived error bound of out_logsum is in DESIGN.md section 5.
 *   splits      0: the library chooses (fills the chip for few users); > 0: that many slices, at most nseg
 *   ws          nr_score_logz_workspace_bytes(d) bytes, 8-byte aligned: U * nseg * 12, rounded; it depends on U and V only
 *               (0 = bad descriptor, see nr_last_error)
 * Refused before any launch (nr_last_error): what K9 refuses for N, ld_news / ld_user, alignment, V, U, stamp without window
 * or the reverse, excl_offsets without excl_ids or the reverse, n_excl < 0; a bad scalar tau; splits outside [0, nseg]; an
 * undersized workspace.  Group caps are not part of this call (the descriptor has no group fields): K15 is the per-group pass.
 * Layout: nr_topk_desc's conventions; the shared tail ws, ws_bytes, prior, stamp, window, ld_window.                       */
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N;
  int splits;
  const int32_t* excl_offsets; /* optional [U + 1]: as in nr_topk_desc */
  const int32_t* excl_ids;     /* optional [n_excl]: as in nr_topk_desc */
  int n_excl;
  float tau;                   /* used when tau_u == NULL; finite, > 0 */
  const float* tau_u;          /* optional [U] */
  float* out_logsum;
  float* out_max;
  int32_t* out_count;
  void* ws;
  size_t ws_bytes;
  const float* prior;    /* optional [V] */
  const int32_t* stamp;  /* optional [V]; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_logz_desc;
size_t nr_score_logz_workspace_bytes(const nr_logz_desc* d);
int nr_score_logz(const nr_logz_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K14  log-probabilities of the entries of named rows, on the partition of K13.  metrics.row_logprob_reference states the
 * contract on the host.  One launch, no workspace: one workgroup per 16 users gathers the k <= 128 table rows a user names
 * through the same MFMA tile (as the named pass of K10), so an entry has the score bits and the key the stream gives it; one
 * wave per user then finishes in fp64 and rounds to fp32 once per output.
 *   row_ids      [U, k] int32, row stride ld_ids, k in [1, NR_TOPK_MAX_K]
 *   base_max, base_logsum   [U] fp32 each: out_max and out_logsum of a K13 call for these users, pools and temperatures
 *   tau, tau_u   as in K13; an entry of tau_u that is <= 0, NaN or infinite gives NaN for every real entry of that user's row
 *   out_logp     [U, k] fp32, contiguous;  out_total optional [U] fp32: the fp64 sum of the row, rounded once (NaN as soon as
 *               one entry of the row is NaN)
 * sequential = 1: Plackett-Luce without replacement, the law of nr_score_sample's rows.  The base must have been computed
 * with the row's ids LEFT OUT of the sum (the caller merges them into the lists of K13).  With s_i the score of entry i, the
 * mass that is left at step j is the base and the entries j .. k-1:
 *   M_j = max(base_max, max_{i >= j} s_i)
 *   L_j = log(exp((base_max - M_j) / tau + base_logsum) + sum_{i >= j} exp((s_i - M_j) / tau))
 *   out_logp[u, j] = (s_j - M_j) / tau - L_j
 * formed as a suffix scan of (max, sum) pairs: only positive terms are added, nothing is subtracted.  A row that takes
 * everything eligible (base count 0: max -inf, logsum -inf) has out_logp == 0 exactly at its last place.
 * sequential = 0: independent entries against the full partition, out_logp[u, j] = (s_j - base_max) / tau - base_logsum with
 * the base computed over everything eligible, the entries included: the full-softmax log-probability of a held-out click.
 * Special entries: an id that is 0 or outside [1, V) is fill -- logp 0, part of no sum.  An entry whose key is 0 (NaN score,
 * prior -inf, stamp outside the window) gets NaN and is part of no sum either.  Whether an entry is in the user's lists, and
 * repeats within a row, are the CALLER'S statement and are not checked: a repeated id is simply two entries.
 * Refused before any launch: a null descriptor or required pointer; k out of range; N, ld_news / ld_user, alignment, V, U,
 * stamp without window or the reverse against K9's rules; ld_ids < k; a bad scalar tau; sequential outside {0, 1}.
 * Group caps are not part of this call: under caps the mass that is left needs per-group partitions, K15 / K16.           */
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N, k;
  const int32_t* row_ids;
  int ld_ids;
  int sequential;           /* 1: Plackett-Luce without replacement; 0: independent entries */
  float tau;                /* used when tau_u == NULL; finite, > 0 */
  const float* tau_u;       /* optional [U] */
  const float* base_max;    /* [U]: out_max of K13 */
  const float* base_logsum; /* [U]: out_logsum of K13 */
  float* out_logp;          /* [U, k] */
  float* out_total;         /* optional [U] */
  const float* prior;    /* optional [V] */
  const int32_t* stamp;  /* optional [V]; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_logprob_desc;
int nr_row_logprob(const nr_logprob_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K15  per-group log-partition: K13 per (user, bin) instead of per user.  Under group caps (K9) a sampled row is sequential
 * sampling from the softmax over what may still be taken, so the mass that is left at a step is a sum over the groups that are
 * still open: the propensity of a capped row (K16) needs the partition of every group apart.  metrics.logz_groups_reference
 * states the contract on the host.  Bins: b = 0 .. n_groups - 1 are the groups, bin n_groups holds the news of no group
 * (negative group id).  Three results per (user, bin), each [U, n_groups + 1] with row stride n_groups + 1, with K13's
 * meaning restricted to the bin's news:
 *   out_max     the largest eligible score of the bin (the bits of K9 / K13); -inf for an empty bin
 *   out_count   the number of eligible news of the bin, exact
 *   out_logsum  log sum exp((s - out_max) * (1 / tau_u)) over the bin, >= 0; -inf for an empty bin; NaN for every non-empty bin
 *               of a user whose tau_u entry is <= 0, NaN or infinite (max and count stay valid), and where out_max is +-inf
 * Score and eligibility are K13's, bit for bit (pool_key, csrc/nr_score_tile.h).
 * The stream runs over the GROUP-MAJOR ORDER of the corpus, which the caller builds once per corpus (ops.GroupOrder):
 *   order      [n_pos] int32: news 1 .. V-1 sorted by (bin, id), every bin's run padded with id 0 up to a multiple of 128
 *              positions (one chunk of the scoring tile); id 0 is never eligible.  n_pos is a multiple of 128.
 *   seg_start  [nseg + 1] int32, ascending positions (multiples of 128), seg_start[0] = 0, seg_start[nseg] = n_pos: with
 *              S = ceil((n_pos / 128) / 256), every bin's run is cut into segments of at most S chunks; a segment never
 *              straddles two bins; nseg <= 256 + n_groups + 1
 *   bin_seg    [n_groups + 2] int32: bin b owns segments bin_seg[b] .. bin_seg[b + 1] - 1
 *   lists      K13's CSR lists IN POSITION SPACE: every id mapped through id -> position and each user's segment re-sorted
 *              (strictly ascending positions).  In position space the stream is ascending again, so K13's cursor and masks apply.
 * A chunk's rows are gathered by order[] (ScoreOrderedRows) into the same MFMA chain; prior and stamp are those of the news id.
 * One (max, sum, count) partial per (user, segment) exactly as in K13 (per-lane chain over the lane's news of the segment,
 * fixed-order wave reduction); a slice is a run of whole segments (slice y of s: the segments that start in [y n_pos / s,
 * (y + 1) n_pos / s), so slices carry about equal numbers of chunks whatever the bin sizes); a second kernel merges, per (user, bin), the bin's partials in
 * fp64 in ascending segment order, takes one log and rounds to fp32 once.  The bits of all three results depend on the user's
 * own inputs and on the order only -- not on `splits`, the batch, the user tile or the place in it.
 * What the arrays hold is the caller's statement: ids of order[] outside [1, V) are rows of zeros that are never eligible, and
 * every position and segment index read from the tables is clamped into its array, so wrong tables give unspecified results,
 * never an access outside the arrays.
 *   ws         nr_score_logz_groups_workspace_bytes(d): U * nseg * 12 bytes rounded to 8 (0 = bad descriptor)
 * Refused before any launch: what K13 refuses; n_groups outside [1, NR_RANK_MAX_GROUPS]; n_pos that is not a positive multiple
 * of 128; nseg outside [1, 256 + n_groups + 1] or above n_pos / 128; splits outside [0, nseg]; a null order, seg_start, bin_seg. */
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N;
  int splits;
  const int32_t* excl_offsets; /* optional [U + 1] */
  const int32_t* excl_ids;     /* optional [n_excl]: POSITIONS, per user strictly ascending */
  int n_excl;
  float tau;                   /* used when tau_u == NULL; finite, > 0 */
  const float* tau_u;          /* optional [U] */
  const int32_t* order;        /* [n_pos] */
  int n_pos;
  const int32_t* seg_start;    /* [nseg + 1] */
  int nseg;
  const int32_t* bin_seg;      /* [n_groups + 2] */
  int n_groups;
  float* out_logsum;           /* [U, n_groups + 1] */
  float* out_max;              /* [U, n_groups + 1] */
  int32_t* out_count;          /* [U, n_groups + 1] */
  void* ws;
  size_t ws_bytes;
  const float* prior;    /* optional [V], indexed by news id */
  const int32_t* stamp;  /* optional [V], indexed by news id; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_logz_groups_desc;
size_t nr_score_logz_groups_workspace_bytes(const nr_logz_groups_desc* d);
int nr_score_logz_groups(const nr_logz_groups_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K16  log-probabilities of the entries of rows drawn under group caps (nr_score_sample with group / group_cap), on the
 * per-group partitions of K15 computed with the row's ids LEFT OUT (merged into the lists).  metrics.capped_row_logprob_reference
 * states the contract on the host.  The law: at step j the candidates are the eligible news not yet taken whose group has
 * fewer than c = group_cap entries in the row so far; news of no group are never capped.  With w_v = exp(s_v / tau), B_b the
 * mass of bin b in the bases, and t_b the step at which the row takes its c-th entry of bin b (infinite for bin n_groups and
 * for bins the row never fills):
 *   D_j = sum_{b : t_b >= j} (B_b + sum_{i >= j, bin(i) = b} w_i),   out_logp[u, j] = s_j / tau - log D_j
 * D_j is formed as a sum over the bins still open -- every term positive -- never as "total minus closed bins".
 * One launch, no workspace: the named-row gather of K14 (the stream's score bits), then one wave per user in fp64 on (max, sum)
 * pairs: t_b for the row's bins; the never-closing bins joined in a fixed order (each lane its bins ascending, then an xor
 * butterfly); a walk over the row from the last place to the first that adds w_j at each step and, on reaching t_b, B_b with
 * the stashed weights of the later entries of b.  One rounding to fp32 per output.
 *   row_ids     [U, k] int32, row stride ld_ids, k in [1, NR_TOPK_MAX_K]
 *   base_max, base_logsum   [U, n_groups + 1] fp32, row stride ld_base: out_max and out_logsum of K15
 *   group       [V] int32 as in K9; an id >= n_groups counts as no group.  group_cap in [1, 128]
 *   out_logp    [U, k] fp32 contiguous; out_total optional [U]: the fp64 sum of the row, rounded once
 * Entries: an id that is 0 or outside [1, V) is fill: 0, part of no sum.  A key-0 entry (NaN score, prior -inf, stamp outside the
 * window) gives NaN, is part of no sum and uses up nothing of a cap.  A bad tau_u entry gives NaN for the real entries of the
 * user; a NaN base gives NaN for every live step at which its bin is still open (a NaN in bin n_groups: every live step).  A live entry whose group already has c live entries before it gives -inf (the capped sampler never draws it): it uses up
 * nothing of a cap, its weight still counts in D_j of every earlier step at which its group was open (the caller left it out of
 * the bases), and out_total is then -inf.  Repeats and membership in the lists are the caller's statement, as in K14.
 * Refused before any launch: what K14 refuses; group_cap outside [1, 128]; n_groups outside [1, NR_RANK_MAX_GROUPS];
 * ld_base < n_groups + 1; a null group.                                                                                   */
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N, k;
  const int32_t* row_ids;
  int ld_ids;
  const int32_t* group;     /* [V] */
  int group_cap, n_groups;
  float tau;                /* used when tau_u == NULL; finite, > 0 */
  const float* tau_u;       /* optional [U] */
  const float* base_max;    /* [U, ld_base]: out_max of K15 */
  const float* base_logsum; /* [U, ld_base]: out_logsum of K15 */
  int ld_base;
  float* out_logp;          /* [U, k] */
  float* out_total;         /* optional [U] */
  const float* prior;    /* optional [V] */
  const int32_t* stamp;  /* optional [V]; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_logprob_capped_desc;
int nr_row_logprob_capped(const nr_logprob_capped_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K17  expected news vector under the full softmax: the gradient of K13's log-partition.  For
 *   nll(u, t) = -(s_ut - max_u) / tau_u + logsum_u     (K14, independent entries)
 *   d nll(u, t) / d user_u = (E_u - news[t]) / tau_u,   E_u = sum_{v eligible} p(v | u) news_v,
 *   p(v | u) = exp((s_uv - max_u) / tau_u - logsum_u)
 * E_u is the softmax-weighted mean news vector over exactly the news K13 sums over: same score bits, same pools, same CSR
 * lists, through the same definitions (pool_key, csrc/nr_score_tile.h; the list cursor and masks, csrc/nr_logz_stream.h).  A
 * news that is not a term of log Z has weight 0.  No [U, V] probability matrix exists: per chunk of 128 news the scoring tile
 * is followed by a second MFMA contraction out[TU, N] += P[TU, 128] . news[128, N] over the same (L2-hot) rows.
 * metrics.expect_reference states the contract on the host.
 *   base_max, base_logsum   [U] fp32: out_max / out_logsum of a K13 call with the SAME vectors, lists, pools and temperatures.
 *               The pass is two-pass by design: with the base known every weight is p <= 1 and no accumulator is rescaled.
 *               p is formed as expf(fmaf(s - max, 1 / tau, -logsum)), 1 / tau ONE fp32 division per user (s == max: the
 *               argument is -logsum, also where 1 / tau overflows).
 *   weight      optional [U] fp32 (NULL = 1): the row's upstream-gradient scale.  A NaN weight gives that user a row of NaN; its
 *               mass and every other user are untouched.
 *   sub_ids, sub_w   optional, both or neither: [U, ld_sub] int32 / fp32, T <= NR_TOPK_MAX_K columns.  Ids outside [1, V) are fill
 *               and skipped; a repeated id is simply two entries.  A named row is subtracted as it is: a component of it that
 *               is not finite reaches that column of out[u] (the cleaning below applies to the sum over v only).
 *   scale_inv_tau   nonzero: the finished row is multiplied by 1 / tau_u
 *   out         [U, ld_out] fp32:  out[u] = (weight_u E_u - sum_t sub_w[u, t] news[sub_ids[u, t]]) (* 1 / tau_u): with
 *               weight = sum_t g_t, sub_w = g the whole gradient of sum_t g_t nll(u, t) with respect to user_u in one call.
 *               Columns N .. ld_out - 1 of a row are never written.  A user with nothing eligible still has its named rows
 *               subtracted (and scaled): out[u] = -sum_t sub_w news[sub_ids], rounded once.
 *   out_mass    optional [U] fp32: sum_v p(v | u) -- 1 up to rounding when the base matches the arguments, a cheap check
 *   edge cases  nothing eligible (base_max = -inf, whatever tau_u holds): E = 0, mass 0.  A largest eligible score of -inf (K13:
 *               max -inf, a count above 0, logsum NaN) reads the same way here and in K23 / K24: base_max = -inf decides, zeros and
 *               mass 0, whatever base_logsum holds.  A tau_u entry that is <= 0, NaN or infinite, or a NaN in the
 *               user's base: a row of NaN and mass NaN; every other user is untouched.  Components of a news row that are not
 *               finite count as 0 in E: such a row's score is NaN or infinite for every user, so it has weight 0 (or its
 *               +inf score makes the base, and with it the row, NaN).
 * Bits.  Per-segment partials as in K13 would cost U * 256 * N floats, so a slice of the corpus (a run of whole segments of
 * K13's plan, a function of V and splits) accumulates in fp32 registers: per (user, component) one MFMA chain over the slice's
 * chunks ascending, per row-part of the chunk (128, 64 or 32 rows: a function of N), the parts added in ascending order; one
 * [N] partial per (user, slice) plus its mass (per-lane fp64 chains, an xor butterfly); a second kernel merges the slices in
 * ascending order in fp64, applies weight, the gather-subtract (fp64, t ascending) and 1 / tau, and rounds to fp32 once.  For
 * a fixed explicit `splits`, row u depends on that user's inputs and V only -- not on the other users, the place in the tile,
 * or U.  splits = 0 lets the library choose by U: the bits may then vary with the batch.  Across different `splits` rows agree
 * within the error bound (derived in DESIGN.md section 5) against the exact result E* of the fp32 inputs:
 *   |E_c - E*_c| <= kappa 2^-24 A_c,   A_c = sum_v p*_v |news_vc|,   kappa = 2 (N + 1) G + 6 C + 5 ln n + 7 K + L + 26
 *   |mass - 1|   <= (6 C + 5 ln n + 7 K + 23) 2^-24
 * with n the eligible news, C = max_v |s_v| / tau, G = max_v (sum_c |user_c news_vc| + |prior_v|) / tau (the score chain: N fma
 * roundings and the prior's add, twice: numerator and partition), K = 2 * seg / 128 the lane chain of K13's base, and L = 128 *
 * (chunks of the longest slice) the fp32 accumulation chain of the second contraction.
 *   ws          nr_score_expect_workspace_bytes(d): U * slices * (N * 4 + 8) bytes, rounded to 8 (0 = bad descriptor); 8-byte
 *               alignment is all it needs: the fp32 partial rows behind the U * slices doubles may start 8 mod 16
 * Refused before any launch: what K13 refuses; a null base_max / base_logsum / out; sub_ids without sub_w or the reverse; T
 * outside [1, NR_TOPK_MAX_K] or ld_sub < T when sub_ids is given; ld_out < N or an out that is not 16-byte aligned; an
 * undersized workspace.  Layout: nr_logz_desc's fields in its order up to tau_u, then this call's, then the shared tail.      */
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N;
  int splits;
  const int32_t* excl_offsets; /* optional [U + 1]: as in nr_topk_desc */
  const int32_t* excl_ids;     /* optional [n_excl]: as in nr_topk_desc */
  int n_excl;
  float tau;                   /* used when tau_u == NULL; finite, > 0 */
  const float* tau_u;          /* optional [U] */
  const float* base_max;       /* [U]: out_max of K13 */
  const float* base_logsum;    /* [U]: out_logsum of K13 */
  const float* weight;         /* optional [U] */
  const int32_t* sub_ids;      /* optional [U, ld_sub]; with sub_w */
  const float* sub_w;          /* optional [U, ld_sub]; with sub_ids */
  int ld_sub, T;
  int scale_inv_tau;
  float* out;                  /* [U, ld_out] */
  int ld_out;
  float* out_mass;             /* optional [U] */
  void* ws;
  size_t ws_bytes;
  const float* prior;    /* optional [V] */
  const int32_t* stamp;  /* optional [V]; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_expect_desc;
size_t nr_score_expect_workspace_bytes(const nr_expect_desc* d);
int nr_score_expect(const nr_expect_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K18  the news side of the full-softmax gradient: K17 with the roles of the two operands swapped.  For
 *   L = sum_u sum_t g_ut nll(u, t),   nll(u, t) = -(s_ut - max_u) / tau_u + logsum_u     (K14, independent entries)
 *   d L / d news_v = D_v - sum_{(u, t): target = v} (g_ut / tau_u) user_u,
 *   D_v = sum_u c_u p(v | u) user_u,   c_u = (sum_t g_ut) / tau_u,   p(v | u) = exp((s_uv - max_u) / tau_u - logsum_u)
 * over exactly the pairs (u, v) that are terms of K13's sums: same score bits (an fp32 fma is commutative in its factors and the
 * chain order is by column only, so the tile of csrc/nr_score_tile.h is used as it is with the news stationary), same pools
 * (pool_key), same lists, row 0 never.  No [U, V] probability matrix exists: a tile of news rows stays in LDS, the users are
 * streamed past it in chunks of 128, and the scoring tile is followed by a second MFMA contraction
 * out[TV, N] += P[TV, 128] . users[128, N] over the same (L2-hot) rows.  metrics.expect_news_reference states the contract on the host.
 *   excl_offsets, excl_users   optional, both or neither: [V + 1] / [n_excl] int32, for news v the ascending 0-based indices of
 *               the users that list it: the transposed CSR of nr_topk_desc's per-user lists (ops.ExclusionLists.by_news)
 *   base_max, base_logsum   [U] fp32: out_max / out_logsum of a K13 call with the SAME vectors, lists, pools and temperatures
 *   weight      optional [U] fp32 (NULL = 1)
 *   scale_inv_tau   nonzero: a user's coefficient is c_u = fl(weight_u * fl(1 / tau_u)), otherwise weight_u; one fp32 multiply
 *               fl(c_u * p) per pair inside the stream
 *   named_offsets, named_user, named_w   optional, all three or none: [V + 1] int32, [n_named] int32, [n_named] fp32 -- the
 *               named terms of news v are entries named_offsets[v] .. named_offsets[v + 1] - 1.  The finalize subtracts
 *               sum_j named_w[j] (* 1 / tau_user if scale_inv_tau) user[named_user[j]] in fp64, j ascending; an entry with
 *               named_w == 0 or a user index outside [0, U) is skipped.  Offsets are clamped into [0, n_named].
 *   out         [V, ld_out] fp32, or NULL: the mass-only mode (no second contraction, kernels of its own, the same mass bits)
 *   out_mass    [V] fp32, or NULL: sum_u weight_u p(v | u), without 1 / tau, summed in fp64 -- the expected exposure of news v.
 *               At least one of the two outputs is given.
 *   edge cases  a pair has weight 0 exactly when v is no term of user u's K13 sum.  A user whose temperature is <= 0, NaN or
 *               infinite, or whose base is NaN or +-inf (nothing eligible: max = -inf), contributes nothing to any row, in the
 *               stream and in the named terms, and puts no NaN anywhere.  Components of a user row that are not finite count as
 *               0 in the second contraction and in the named terms.  Row 0 and rows nobody can be shown are exact zeros, minus
 *               their named terms.
 * Bits.  The user axis [0, U) is cut the way K13 cuts the news axis (seg = 128 ceil(U / (128 * 256)) users a segment, slices =
 * runs of whole segments; splits = 0 lets the library choose by V).  A slice accumulates in fp32 registers: per (news,
 * component) one MFMA chain over the slice's chunks ascending, per user-part of the chunk (128, 64 or 32 users: a function of N),
 * the parts added in ascending order; one [N] partial per (news, slice) plus its mass (per-lane fp64 chains of the exact
 * products weight_u p, an xor butterfly); the finalize (one workgroup per news row) merges the slices in ascending order in
 * fp64, subtracts the named terms and rounds to fp32 once.  No atomics, no arrival order.  For a fixed explicit `splits`, row
 * v's bits depend on that row's own inputs (vector, prior, stamp, list, named terms), on the users, on U and on `splits` -- not
 * on any other news row, nor on the row's place in the table or the tile.  Error bound (derived in DESIGN.md section 5)
 * against the exact result of the fp32 inputs, with n, C, G the maxima over the call's live users of K17's quantities:
 *   |out_vc - out*_vc| <= kappa 2^-24 A_vc,   A_vc = sum_u |c_u| p*_uv |user_uc| + sum_j |d_j| |user_jc|,
 *   kappa = 2 (N + 1) G + 6 C + 5 ln n + 7 K + L + 29,   d_j = named_w[j] (/ tau_user)
 *   |mass_v - mass*_v| <= (6 C + 5 ln n + 7 K + 29) 2^-24 sum_u |weight_u| p_uv   against the p of the device's own scores
 *               (against the p* of exact scores the score chain 2 (N + 1) G enters as well)
 * K = 2 * seg_V / 128 the lane chain of K13's base, L = 128 * (chunks of the longest user slice).
 *   ws          nr_score_expect_news_workspace_bytes(d): V * slices * (N * 4 + 8) bytes, rounded to 8; V * slices * 8 in the
 *               mass-only mode (0 = bad descriptor)
 * Refused before any launch: what K17 refuses of the shared fields; excl_users without excl_offsets or the reverse; splits
 * above the user segments; out and out_mass both null; a null base_max / base_logsum; one or two of the three named arrays;
 * n_named < 0; ld_out < N or an out that is not 16-byte aligned; an undersized workspace.  Layout: nr_expect_desc's fields in
 * its order up to base_logsum, then this call's, then the shared tail.                                                       */
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N;
  int splits;
  const int32_t* excl_offsets; /* optional [V + 1]: by news */
  const int32_t* excl_users;   /* optional [n_excl]: ascending user indices per news */
  int n_excl;
  float tau;                   /* used when tau_u == NULL; finite, > 0 */
  const float* tau_u;          /* optional [U] */
  const float* base_max;       /* [U]: out_max of K13 */
  const float* base_logsum;    /* [U]: out_logsum of K13 */
  const float* weight;         /* optional [U] */
  int scale_inv_tau;
  const int32_t* named_offsets; /* optional [V + 1]; with named_user and named_w */
  const int32_t* named_user;    /* optional [n_named] */
  const float* named_w;         /* optional [n_named] */
  int n_named;
  float* out;                  /* [V, ld_out] or NULL (mass only) */
  int ld_out;
  float* out_mass;             /* [V] or NULL */
  void* ws;
  size_t ws_bytes;
  const float* prior;    /* optional [V] */
  const int32_t* stamp;  /* optional [V]; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_expect_news_desc;
size_t nr_score_expect_news_workspace_bytes(const nr_expect_news_desc* d);
int nr_score_expect_news(const nr_expect_news_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K19  the gradient coefficients of a sequential row: the backward of K14 with sequential = 1.  For a row i_0 .. i_{k-1}, a
 * temperature tau and per-entry upstream gradients g_j, with (K14's quantities)
 *   e_i = exp(s_i / tau),  B = the base: the mass of everything eligible that the row does not name (K13 with the row merged
 *   into the lists),  W_j = B + sum_{i >= j} e_i,  nll_j = -(s_j / tau - log W_j),
 * the gradient of L = sum_j g_j nll_j collapses onto K17 and K18 as they stand:
 *   d L / d user   = (a E_rest - sum_i c_i news[i_i]) / tau          K17: weight = a, sub_ids = row, sub_w = c, scale_inv_tau
 *   d L / d news_v = (a p_rest(v | u) - sum_{i: i_i = v} c_i) user / tau     K18: weight = a, named terms (row, c), scale_inv_tau
 *   a   = sum_j g_j B / W_j,     c_i = g_i - e_i sum_{j <= i} g_j / W_j,
 * E_rest / p_rest the softmax over exactly the news of B: K17 / K18 called with the lists of that K13 call and its base.  This
 * call computes a and c; metrics.row_logprob_grad_reference states the contract on the host.  a = sum_i c_i in exact
 * arithmetic (adding one vector to every news changes no probability).
 * One launch, no workspace: K14's gather through the same MFMA tile (an entry has the stream's score bits and key), K14's
 * suffix scan of (max, sum) pairs S_j = (M_j, sigma_j), W_j = exp(M_j / tau) sigma_j, then an inclusive PREFIX scan of the pairs
 * (-M_j, g_j / sigma_j): M_j does not increase with j and the join is linear in the sum, so g may have any sign, and
 *   c_i = g_i - exp((s_i - M_i) / tau) q_i,   a = exp((base_max - M_L) / tau + base_logsum) q_L   (L the last live entry)
 * form no exponent above 0.  One wave per user in fp64, O(k log k) exponentials; each output is rounded to fp32 once.  The
 * outputs of user u depend on that user's inputs only -- not on the other users of the call or the place in it.
 *   row_ids, base_max, base_logsum, tau, tau_u, pools   as in K14, sequential = 1: the base formed WITHOUT the row's ids
 *   g            optional [U, ld_g] fp32, ld_g >= k; NULL = 1 everywhere
 *   out_weight   [U] fp32: a          out_sub_w   [U, k] fp32, contiguous: c
 * Special entries: fill (an id that is 0 or outside [1, V)) and an entry whose key is 0 (NaN score, prior -inf, stamp outside
 * the window) are no step of the row: c = 0, their g is not read.  A user whose temperature is <= 0, NaN or infinite, or
 * whose base is NaN: a = 0 and every c = 0.  An empty base (max -inf, logsum -inf: the row takes everything eligible) gives
 * a = 0 exactly; the last live entry's step then has logp 0 and adds nothing.  A row without a live entry: all zeros.
 * Error bound (derived in DESIGN.md section 5) against the exact result on the fp32 inputs, e = 2^-24:
 *   |a - a*| <= kappa e sum_j |g_j| B* / W*_j,   |c_i - c*_i| <= kappa e (|g_i| + e*_i sum_{j <= i} |g_j| / W*_j),
 *   kappa = 2 (N + 1) G + 4 ln n + 7 K + 16     (G the score chain of K17, n the news of the base, K = 2 * seg / 128)
 * Refused before any launch: what K14 refuses (sequential aside); g with ld_g < k; a null out_weight or out_sub_w.
 * Layout: nr_logprob_desc without `sequential`, with g, ld_g and the two outputs in place of out_logp, out_total.            */
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N, k;
  const int32_t* row_ids;
  int ld_ids;
  float tau;                /* used when tau_u == NULL; finite, > 0 */
  const float* tau_u;       /* optional [U] */
  const float* base_max;    /* [U]: out_max of K13 */
  const float* base_logsum; /* [U]: out_logsum of K13 */
  const float* g;           /* optional [U, ld_g]: upstream gradient of nll per entry */
  int ld_g;
  float* out_weight;        /* [U]: a */
  float* out_sub_w;         /* [U, k]: c */
  const float* prior;    /* optional [V] */
  const int32_t* stamp;  /* optional [V]; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_logprob_grad_desc;
int nr_row_logprob_grad(const nr_logprob_grad_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K20  the gradient of K15: the expected news vector PER BIN, weighted per (user, bin).  K17 with per-bin bases and a weight
 * omega[u, b] in front of every bin's softmax, streamed over the group-major order K15 streams over:
 *   out[u] = ( sum_b omega[u, b] E_{u,b}  -  sum_t sub_w[u, t] news[sub_ids[u, t]] ) (* 1 / tau_u)
 *   E_{u,b} = sum_{v in bin b, eligible, not listed} p_b(v | u) news_v,   p_b(v | u) = exp((s_uv - gmax_ub) / tau_u - logsum_ub)
 * the softmax INSIDE bin b on K15's base of that bin.  With omega and sub_w from K21 this is the whole user-side gradient of
 * the capped row's loss.  metrics.expect_groups_reference states the contract on the host.
 *   order, n_pos, seg_start, nseg, bin_seg, n_groups, lists IN POSITION SPACE, pools by news id   as in K15
 *   base_max, base_logsum   [U, ld_base] fp32, ld_base >= n_groups + 1: out_max / out_logsum of a K15 call with the SAME arguments
 *   bin_w       [U, ld_base] fp32: omega
 *   sub_ids, sub_w, ld_sub, T, scale_inv_tau   K17's fields and meaning
 *   out         [U, ld_out] fp32;   out_mass optional [U] fp32: sum_v omega p over the EXACT products, summed in fp64 -- up to
 *               rounding sum of omega_b over the non-empty bins
 *               Columns N .. ld_out - 1 of an `out` row are never written.
 * Stream: K17's kernel (the scoring tile, the P tile in LDS, out[TU, N] += P[TU, 128] . rows[128, N] on
 * v_mfma_f32_16x16x4_f32, accumulators in registers for the whole slice, nothing rescaled) with rows read through order[] for
 * both contractions and prior / stamp gathered by id.  A position whose id is 0 is padding: weight 0.  A segment never
 * straddles two bins; when the bin changes the wave reloads (gmax, -logsum, omega) of its users.  The weight of a pair is
 * fl(omega * p), p = expf(fmaf(s - gmax, 1 / tau, -logsum)) exactly as in K17: ONE fp32 multiply per pair.  A (user, bin) with
 * omega == 0 contributes exactly nothing whatever its base holds; so does an empty bin (gmax = -inf).
 * Slices are K15's (slice y of s: the segments that start in [y n_pos / s, (y + 1) n_pos / s)); the user tile is K17's.  A
 * slice without a segment writes nothing and the finalize skips it.  Finalize: K17's -- the slices ascending in fp64, the
 * gather-subtract in fp64 with t ascending, times 1 / tau, one rounding.
 * Bits.  For a fixed explicit `splits`, row u depends on that user's inputs and on the order only -- not on the other users,
 * the place in the tile, or U.  splits = 0 lets the library choose by U.
 * Edge cases, K17's read per bin.  A user whose tau_u entry is <= 0, NaN or infinite and who has a non-empty bin, or who has
 * a non-empty bin with omega != 0 whose gmax is NaN or +inf, whose logsum is NaN, or whose omega is not finite: a row of NaN
 * and mass NaN, every other user untouched.  Non-finite components of a news row count as 0.
 * Error bound (derived in DESIGN.md section 5) against the exact result on the fp32 inputs, e = 2^-24:
 *   |out_c - out*_c| <= kappa e (sum_b |omega_b| sum_v p*_bv |news_vc| + sum_t |sub_w_t| |news[sub_ids_t, c]|) (* 1 / tau)
 *   kappa = 2 (N + 1) G + 6 C + 5 ln n + 7 K + L + 27
 * K17's kappa with one more rounding (fl(omega * p)), n the eligible news of the largest bin, C and G over the bins with
 * omega != 0 (C = max |s_v| / tau there), K = 2 S (S = the chunks of K15's longest segment) and L = 128 * (chunks of
 * this call's longest slice).
 *   |mass - sum_{b non-empty} omega_b| <= (6 C + 5 ln n + 7 K + 23) e sum_{b non-empty} |omega_b|      (K17's mass bound, per bin)
 *   ws          nr_score_expect_groups_workspace_bytes(d): U * slices * (N * 4 + 8) bytes rounded to 8 (0 = bad descriptor)
 * Refused before any launch: everything K15 refuses (null descriptor; V, U, N; the list form; a bad scalar tau; n_groups,
 * n_pos, nseg, splits out of range; stamp without window or the reverse; a null news_vecs, user, order, seg_start, bin_seg;
 * rows off 16 bytes); a null base_max, base_logsum, bin_w or out; ld_base < n_groups + 1; sub_ids without sub_w or the
 * reverse; T outside [1, NR_TOPK_MAX_K] or ld_sub < T when sub_ids is given; ld_out < N or an out off 16 bytes; an undersized
 * workspace.  Layout: nr_logz_groups_desc's fields in its order up to n_groups, then this call's, then the shared tail.   */
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N;
  int splits;
  const int32_t* excl_offsets; /* optional [U + 1] */
  const int32_t* excl_ids;     /* optional [n_excl]: POSITIONS, per user strictly ascending */
  int n_excl;
  float tau;                   /* used when tau_u == NULL; finite, > 0 */
  const float* tau_u;          /* optional [U] */
  const int32_t* order;        /* [n_pos] */
  int n_pos;
  const int32_t* seg_start;    /* [nseg + 1] */
  int nseg;
  const int32_t* bin_seg;      /* [n_groups + 2] */
  int n_groups;
  const float* base_max;       /* [U, ld_base]: out_max of K15 */
  const float* base_logsum;    /* [U, ld_base]: out_logsum of K15 */
  const float* bin_w;          /* [U, ld_base]: omega */
  int ld_base;
  const int32_t* sub_ids;      /* optional [U, ld_sub]; with sub_w */
  const float* sub_w;          /* optional [U, ld_sub]; with sub_ids */
  int ld_sub, T;
  int scale_inv_tau;
  float* out;                  /* [U, ld_out] */
  int ld_out;
  float* out_mass;             /* optional [U] */
  void* ws;
  size_t ws_bytes;
  const float* prior;    /* optional [V], indexed by news id */
  const int32_t* stamp;  /* optional [V], indexed by news id; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_expect_groups_desc;
size_t nr_score_expect_groups_workspace_bytes(const nr_expect_groups_desc* d);
int nr_score_expect_groups(const nr_expect_groups_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K21  the gradient coefficients of a capped row: the backward of K16.  In K16's notation (w_v = exp(s_v / tau), B_b the
 * mass of bin b in the K15 bases formed with the row's ids merged into the lists, t_b the step at which the row takes its
 * c-th live entry of bin b, D_j = sum_{b: t_b >= j} (B_b + sum_{i >= j, bin(i) = b} w_i), nll_j = -(s_j / tau - log D_j)
 * over the live steps j) and upstream gradients g_j, let Q_j = sum_{j' <= j, j' a live step} g_j' / D_j' and Q_b = Q at
 * min(t_b, last live step).  Then
 *   d (sum_j g_j nll_j) / d user_u = ( sum_b omega_b E_b - sum_i c_i news[row_i] ) / tau          (K20)
 *   omega_b = B_b Q_b                       per (user, bin), E_b the softmax mean inside the bin on K15's base
 *   c_i = g_i - w_i Q_i                     for a live step i (K19's form)
 *   c_i = -w_i Q_{bin(i)}                   for a blocked entry (its group already full: K16's -inf entry); it is no step and
 *                                           its g is not read
 * sum_b omega_b = sum_i c_i in exact arithmetic.  metrics.capped_row_logprob_grad_reference states the contract on the host.
 * One launch, one wave per user, fp64, no workspace: K16's gather (the stream's score bits), K16's determination of t_b and
 * its walk from the last place to the first, each D_j kept as the pair (M_j, sigma_j), D_j = exp(M_j / tau) sigma_j; the
 * supports of the steps are nested, so M_j does not increase with j and K19's inclusive prefix scan of (-M_j, g_j / sigma_j)
 * applies:  omega_b = exp((gmax_b - M_{t_b}) / tau + logsum_b) q_{t_b},  c_i = g_i - exp((s_i - M_i) / tau) q_i  form no
 * exponent above 0 -- B_b and w_i are terms of the D they are divided by.  g may have any sign.  Each output is rounded to
 * fp32 once; a user's outputs depend on that user's inputs only.
 *   row_ids, group, group_cap, n_groups, base_max, base_logsum, ld_base, tau, tau_u, pools   as in K16
 *   g            optional [U, ld_g] fp32, ld_g >= k; NULL = 1 everywhere
 *   out_bin_w    [U, ld_base] fp32: omega; bins 0 .. n_groups all written, 0 for empty bins; columns n_groups + 1 .. ld_base - 1
 *                are never written
 *   out_sub_w    [U, k] fp32, contiguous: c
 * Special entries: fill and key-0 entries are no step: c = 0, their g is not read.  A user whose temperature is <= 0, NaN or
 * infinite, or with a NaN in a base (gmax NaN, or logsum NaN in a non-empty bin; every bin is open at step 0, so the row
 * needs them all): all zeros.  A row without a live step: all zeros.
 * Error bound (derived in DESIGN.md section 5) against the exact result on the fp32 inputs, e = 2^-24:
 *   |omega_b - omega*_b| <= kappa e B*_b sum_{j <= t_b} |g_j| / D*_j
 *   |c_i - c*_i| <= kappa e (|g_i| + w*_i sum_{j <= i} |g_j| / D*_j)     (blocked: without |g_i|, the sum up to t_bin(i))
 *   kappa = 2 (N + 1) G + 4 ln n + 7 K + 17
 * K19's kappa plus 1 for the fp64 joins over the open bins and the later entries (at most 513 + 128 of them, each 2^-53);
 * n the eligible news of the largest bin, K = 2 S of K15's segments.
 * Refused before any launch: what K16 refuses (the outputs aside); g with ld_g < k; a null out_bin_w or out_sub_w.
 * Layout: nr_logprob_capped_desc without out_logp / out_total, with g, ld_g and the two outputs in their place.            */
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N, k;
  const int32_t* row_ids;
  int ld_ids;
  const int32_t* group;     /* [V] */
  int group_cap, n_groups;
  float tau;                /* used when tau_u == NULL; finite, > 0 */
  const float* tau_u;       /* optional [U] */
  const float* base_max;    /* [U, ld_base]: out_max of K15 */
  const float* base_logsum; /* [U, ld_base]: out_logsum of K15 */
  int ld_base;
  const float* g;           /* optional [U, ld_g]: upstream gradient of nll per entry */
  int ld_g;
  float* out_bin_w;         /* [U, ld_base]: omega */
  float* out_sub_w;         /* [U, k]: c */
  const float* prior;    /* optional [V] */
  const int32_t* stamp;  /* optional [V]; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_logprob_capped_grad_desc;
int nr_row_logprob_capped_grad(const nr_logprob_capped_grad_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K22  the news side of the capped row's gradient: K18 with K20's per-bin treatment.  With omega[u, b] and c[u, i] of K21,
 *   d L / d news_v = sum_u (omega[u, bin(v)] / tau_u) p_bin(v)(v | u) user_u  -  sum_{(u, i): row_ui = v} (c_ui / tau_u) user_u
 *   p_b(v | u) = exp((s_uv - gmax_ub) / tau_u - logsum_ub)        the softmax INSIDE bin b on K15's base of that bin
 * over exactly the pairs (u, v) that are terms of K15's sum for bin(v): same score bits, same pools, same lists, row 0 never.
 * The same d L / d s_uv that K20 contracts with news_v is contracted with user_u here.  No [U, V] matrix exists: a tile of news
 * rows stays in LDS, the users are streamed past it in chunks of 128, and the scoring tile is followed by a second MFMA
 * contraction out[TV, N] += P[TV, 128] . users[128, N] (K18's kernel).  metrics.expect_news_groups_reference states the contract
 * on the host.
 *   order, n_pos, n_groups   K15's group-major order (ops.GroupOrder).  The stationary tile (64, 32 or 16 rows: K18's table, a
 *               function of N alone) is a tile of POSITIONS whose rows are gathered through order[].  Every bin's run starts at
 *               a multiple of 128 positions, so a tile lies in ONE bin.  A position whose id is 0 (or outside [1, V)) is
 *               padding: it is never alive and nothing is written for it; a tile that holds only padding returns before it
 *               loads anything, so a run's padded tail costs at most one partly filled tile per bin.  Every id in [1, V) must
 *               stand in order[] EXACTLY ONCE (ops.GroupOrder builds it so): a row is written where its id is met, so an id
 *               that is left out leaves its row of `out` and `out_mass` unspecified (the finalize reads workspace nothing
 *               wrote), and one that stands twice gets one of its two partials, whichever is stored last.  Neither reads or
 *               writes outside the arrays.
 *   bin_start   [n_groups + 2] int32: bin b owns positions bin_start[b] .. bin_start[b + 1] - 1.  A workgroup finds its bin once
 *               (a search clamped into [0, n_groups]).
 *   base_max, base_logsum, bin_w   BIN-MAJOR: [n_groups + 1, ld_bin] fp32, ld_bin >= U -- the transposes of K15's out_max /
 *               out_logsum (of a call with the SAME vectors, lists, pools and temperatures) and of K21's omega.  Per chunk the
 *               lanes load the three values of THEIR users for the tile's bin: 64 consecutive floats a wave.
 *   excl_offsets, excl_users   optional, both or neither: the lists BY POSITION, [n_pos + 1] / [n_excl] int32: for position p
 *               the ascending 0-based indices of the users whose list holds order[p] (ops.GroupOrder.by_position)
 *   prior, stamp   indexed by news id, gathered for the tile's rows
 *   scale_inv_tau   nonzero: a pair's coefficient is cf = fl(omega * fl(1 / tau_u)), otherwise omega; the pair's weight is
 *               P = fl(cf * p), p = expf(s == gmax ? -logsum : fmaf(s - gmax, 1 / tau, -logsum)): K18's, omega for `weight`
 *   named_offsets, named_user, named_w, n_named   K18's named terms, offsets [V + 1] BY NEWS ID
 *   out         [V, ld_out] fp32, required.   out_mass   optional [V] fp32: sum_u omega[u, bin(v)] p over the exact products,
 *               summed in fp64, without 1 / tau.  There is no mass-only mode.
 *               Columns N .. ld_out - 1 of an `out` row are never written.
 * Live pairs.  A (user, bin) pair is live exactly when tau_u is finite and > 0, gmax and logsum are finite, and omega is finite
 * and != 0.  A pair that is not live contributes exactly nothing and puts no NaN anywhere.  This differs from K20 ON PURPOSE:
 * K20 answers such a user with a row of NaN, which stays with that user; on the news side one NaN would reach every row of the
 * table.  Components of a user row that are not finite count as 0 in the second contraction and in the named terms.
 * Named terms are gated by the USER ONLY: tau finite and > 0, named_w != 0, an index in [0, U), finite components -- NOT by a
 * base.  Under caps a bin is routinely empty because the row took all of it, and its entries still carry c != 0.  (K18 gates
 * its named terms by the user's single base; that contract is K18's and stays.)  Row 0 is in no order: it reads no partials
 * and is exact zeros minus its named terms.
 * Bits.  The user axis is cut by K18's plan (seg = 128 ceil(U / (128 * 256)) users a segment, slices = runs of whole segments;
 * splits = 0: the library's choice by V).  Per (news, component) K18's chain; one [N] partial and one fp64 mass per (news,
 * slice), written at the news ID, so the workspace is K18's and the finalize (K18's: slices ascending in fp64, minus the named
 * terms with j ascending, one rounding) needs no position map.  For a fixed explicit `splits`, row v's bits depend on v's own
 * inputs (vector, prior, stamp, list, named terms, its bin), on the users and their omega and bases for that bin, on U and on
 * `splits` -- not on any other news, on v's place in its run or tile, or on the sizes of the other bins.  With one bin holding
 * every news, omega = weight and K13's base in that bin's row, rows and mass are K18's bit for bit (live users).
 * Error bound (derived in DESIGN.md section 5) against the exact result of the fp32 inputs, e = 2^-24:
 *   |out_vc - out*_vc| <= kappa e A_vc,   A_vc = sum_u |cf_u| p*_uv |user_uc| + sum_j |d_j| |user_jc|,
 *   kappa = 2 (N + 1) G + 6 C + 5 ln n + 7 K + L + 29,   d_j = named_w[j] (/ tau_user)
 *   |mass_v - mass*_v| <= (6 C + 5 ln n + 7 K + 29) e sum_u |omega_u,bin(v)| p_uv    against the p of the device's own scores
 *               (against the p* of exact scores the score chain 2 (N + 1) G enters as well, as in K18)
 * K18's kappa with omega for weight and K15's per-bin base for K13's: n the eligible news of the largest bin, C and G the
 * maxima over the live (user, bin) pairs, K = 2 S (S = the chunks of K15's longest segment), L = 128 * (chunks of the longest
 * user slice).
 *   ws          nr_score_expect_news_groups_workspace_bytes(d): V * slices * (N * 4 + 8) bytes, rounded to 8 (0 = bad descriptor)
 * Refused before any launch: what K18 refuses of the shared fields (null descriptor; V, U, N; n_excl < 0; excl_users without
 * excl_offsets or the reverse; a bad scalar tau; splits above the user segments; stamp without window or the reverse; rows off
 * 16 bytes); what K15 refuses of n_groups and n_pos; a null news_vecs, user, order, bin_start, base_max, base_logsum, bin_w or
 * out; ld_bin < U; one or two of the three named arrays; n_named < 0; ld_out < N or an out off 16 bytes; an undersized
 * workspace.  Layout: nr_expect_news_desc's fields in its order up to tau_u, then this call's, then the shared tail.        */
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N;
  int splits;
  const int32_t* excl_offsets; /* optional [n_pos + 1]: by position */
  const int32_t* excl_users;   /* optional [n_excl]: ascending user indices per position */
  int n_excl;
  float tau;                   /* used when tau_u == NULL; finite, > 0 */
  const float* tau_u;          /* optional [U] */
  const int32_t* order;        /* [n_pos] */
  int n_pos;
  const int32_t* bin_start;    /* [n_groups + 2] */
  int n_groups;
  const float* base_max;       /* [n_groups + 1, ld_bin]: out_max of K15, transposed */
  const float* base_logsum;    /* [n_groups + 1, ld_bin]: out_logsum of K15, transposed */
  const float* bin_w;          /* [n_groups + 1, ld_bin]: omega, transposed */
  int ld_bin;
  int scale_inv_tau;
  const int32_t* named_offsets; /* optional [V + 1]; with named_user and named_w */
  const int32_t* named_user;    /* optional [n_named] */
  const float* named_w;         /* optional [n_named] */
  int n_named;
  float* out;                  /* [V, ld_out] */
  int ld_out;
  float* out_mass;             /* optional [V] */
  void* ws;
  size_t ws_bytes;
  const float* prior;    /* optional [V], indexed by news id */
  const int32_t* stamp;  /* optional [V], indexed by news id; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_expect_news_groups_desc;
size_t nr_score_expect_news_groups_workspace_bytes(const nr_expect_news_groups_desc* d);
int nr_score_expect_news_groups(const nr_expect_news_groups_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K23  entropy of the served distribution.  With K13's base the device forms x_v = fmaf(s_v - max, 1 / tau, -logsum) = log p_v
 * and p_v = expf(x_v) exactly as K17 does; per user, over exactly the news K13 sums over (same score bits, pools, CSR lists),
 *   m0 = sum p,   m1 = sum p x,   m2 = sum p x^2
 * and three results, each [U] fp32 (metrics.entropy_reference states the contract on the host):
 *   out_entropy   H = -m1 = -sum_v p(v | u) log p(v | u); exp(H) is the effective number of news the user is exposed to
 *   out_var       optional: Var_p(log p) = m2 - m1^2 (formed in fp64); dH / dtau = out_var / tau
 *   out_mass      optional: m0 -- 1 up to rounding when the base matches the arguments (K17's mass)
 * A pair with p == 0 (not eligible, expf underflowed, a score of -inf) is a term of no sum: 0 log 0 = 0, and 0 * -inf is never
 * formed.  No [U, V] matrix exists; the pass is K13's stream (grid, segments, slices, user tile, LDS) without the running
 * maximum -- the base is known.
 *   base_max, base_logsum, tau, tau_u, lists, pools   K17's fields and meaning
 *   edge cases  nothing eligible (base_max = -inf, whatever tau_u holds): 0, 0, 0.  A tau_u entry that is <= 0, NaN or infinite,
 *               or a NaN in the user's base: NaN for that user's three results, nobody else's change.  Exactly one eligible
 *               news: H == 0.0 and var == 0.0 exactly (x = -logsum = -0, p = 1).
 * Bits.  Per pair the products p x and (p x) x are formed in fp64 from the fp32 p and x and added to three per-lane fp64 chains
 * over the lane's news of the slice (which lane sees which id is fixed by V); an xor butterfly leaves one triple per (user,
 * slice); a second kernel adds the slices in ascending order in fp64 and rounds each result to fp32 once.  For a fixed explicit
 * `splits` a user's three results depend on that user's inputs and V only -- not on U, the user tile or the place in it.
 * Error bounds (derived in DESIGN.md section 5; first order in e = 2^-24) against the exact H*, m2* = sum p* x*^2, var* of the
 * fp32 inputs.  x carries the ABSOLUTE error kappa_x e,
 *   kappa_x = 2 (N + 1) G + 6 C + 5 ln n + 7 K + 14          (n, C, G, K as in K17)
 *   |H - H*|     <= ((kappa_x + 8) H* + kappa_x + 1) e + n 2^-119
 *   |var - var*| <= ((kappa_x + 8) (m2* + 2 H*^2) + 4 kappa_x H* + 1) e + n 2^-112
 *   |mass - 1|   <= (6 C + 5 ln n + 7 K + 23) e                                   (K17's)
 * the last terms what weights below the normal range (x < -87) lose.
 *   ws          nr_score_entropy_workspace_bytes(d): U * slices * 24 bytes (0 = bad descriptor)
 * Refused before any launch: what K17 refuses of the shared fields; a null base_max / base_logsum / out_entropy; an undersized
 * workspace.  Layout: nr_logz_desc's fields in its order up to tau_u, then this call's, then the shared tail.                */
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N;
  int splits;
  const int32_t* excl_offsets; /* optional [U + 1]: as in nr_topk_desc */
  const int32_t* excl_ids;     /* optional [n_excl]: as in nr_topk_desc */
  int n_excl;
  float tau;                   /* used when tau_u == NULL; finite, > 0 */
  const float* tau_u;          /* optional [U] */
  const float* base_max;       /* [U]: out_max of K13 */
  const float* base_logsum;    /* [U]: out_logsum of K13 */
  float* out_entropy;          /* [U] */
  float* out_var;              /* optional [U] */
  float* out_mass;             /* optional [U] */
  void* ws;
  size_t ws_bytes;
  const float* prior;    /* optional [V] */
  const int32_t* stamp;  /* optional [V]; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_entropy_desc;
size_t nr_score_entropy_workspace_bytes(const nr_entropy_desc* d);
int nr_score_entropy(const nr_entropy_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K24  K17 with a per-pair weight that is affine in log p: the gradient of the entropy, and of any loss
 *   L = sum_t g_t nll(u, t) + h_u H_u:    d L / d user_u = ((sum_t g_t - h H) E - h J - sum_t g_t news[t]) / tau_u
 * with E = sum_v p_v news_v (K17's) and J = sum_v p_v x_v news_v, x = log p (d H / d user = -(J + H E) / tau).  One contraction,
 *   out[u] = (sum_v r_v news_v - sum_t sub_w[u, t] news[sub_ids[u, t]]) (* 1 / tau_u),   r_v = p_v fmaf(beta_u, x_v, alpha_u),
 * so alpha = sum_t g_t - h H, beta = -h, sub_w = g, scale_inv_tau gives that gradient in one call.
 * metrics.expect_affine_reference states the contract on the host.
 *   alpha       optional [U] fp32 (NULL = 1);  beta  optional [U] fp32 (NULL = 0).  With alpha = 1, beta = 0 rows and mass are K17's
 *               (weight NULL) bit for bit at the same explicit `splits`.  A NaN in a user's alpha or beta gives that user a row
 *               of NaN (where it has a weight at all) and touches nobody else; that user's out_mass stays sum_v p_v.
 *   the other fields, the edge cases and the refusals   K17's; r_v = 0 exactly where p_v == 0 (0 * -inf is never formed)
 *   out_mass    optional [U] fp32: sum_v p_v, K17's mass -- not the sum of r
 * Stream and finalize are K17's (same user tiles and k-slab counts, same LDS, no scratch), the one difference the value stored to
 * the P tile; the finalize has no weight multiply.  Bits: K17's rule.  Error bound (derived in DESIGN.md section 5):
 *   |out_c - out*_c| <= kappa' e A_c,   A_c = sum_v p*_v (|alpha| + |beta| (|x*_v| + 1)) |news_vc|,
 *   kappa' = 2 (N + 1) G + 6 C + 5 ln n + 7 K + L + 28      (K17's kappa + 2: the fma of the weight and its product with p)
 *   ws          nr_score_expect_affine_workspace_bytes(d): K17's size
 * Layout: nr_expect_desc with `weight` replaced by `alpha`, then `beta`.                                                        */
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N;
  int splits;
  const int32_t* excl_offsets; /* optional [U + 1]: as in nr_topk_desc */
  const int32_t* excl_ids;     /* optional [n_excl]: as in nr_topk_desc */
  int n_excl;
  float tau;                   /* used when tau_u == NULL; finite, > 0 */
  const float* tau_u;          /* optional [U] */
  const float* base_max;       /* [U]: out_max of K13 */
  const float* base_logsum;    /* [U]: out_logsum of K13 */
  const float* alpha;          /* optional [U]; NULL = 1 */
  const float* beta;           /* optional [U]; NULL = 0 */
  const int32_t* sub_ids;      /* optional [U, ld_sub]; with sub_w */
  const float* sub_w;          /* optional [U, ld_sub]; with sub_ids */
  int ld_sub, T;
  int scale_inv_tau;
  float* out;                  /* [U, ld_out] */
  int ld_out;
  float* out_mass;             /* optional [U] */
  void* ws;
  size_t ws_bytes;
  const float* prior;    /* optional [V] */
  const int32_t* stamp;  /* optional [V]; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_expect_affine_desc;
size_t nr_score_expect_affine_workspace_bytes(const nr_expect_affine_desc* d);
int nr_score_expect_affine(const nr_expect_affine_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K25  K18 with a per-pair weight that is affine in log p: the news side of K24.  For
 *   L = sum_u (sum_t g_ut nll(u, t) + h_u H_u),   x_uv = log p(v | u),   alpha_u = sum_t g_ut - h_u H_u,   beta_u = -h_u
 *   d L / d news_v = sum_u (1 / tau_u) p(v | u) (alpha_u + beta_u x_uv) user_u - sum_{(u, t): target = v} (g_ut / tau_u) user_u
 * (d nll_t / d z_v = p_v - delta_vt, d H / d z_v = -p_v (x_v + H), z = s / tau) over exactly the pairs (u, v) that are terms of
 * K13's sums.  One contraction,
 *   out[v] = sum_u r_uv user_u - sum_j named_w[j] (* 1 / tau_user) user[named_user[j]],   r_uv = p_uv fmaf(b_u, x_uv, a_u),
 *   a_u = alpha_u (* fl(1 / tau_u) if scale_inv_tau),  b_u = beta_u (likewise),
 * so K24's alpha and beta, named terms (target, g) and scale_inv_tau give that gradient in one call, without the [U, V] matrix.
 * metrics.expect_news_affine_reference states the contract on the host.
 *   alpha       optional [U] fp32 (NULL = 1);  beta  optional [U] fp32 (NULL = 0).  With alpha = w (finite, and finite times
 *               1 / tau) and beta = NULL, rows are K18's with weight = w bit for bit at the same explicit `splits`
 *               (fmaf(0, x, a) == a).  A user whose a or b is NaN or infinite contributes to NO row through the stream and puts
 *               no NaN into the table (K22's choice for its bin weights: one user's NaN would otherwise reach every news).
 *   named_offsets, named_user, named_w, n_named   K18's named terms; gated by K18's rule (a live user, named_w != 0) alone,
 *               not by alpha or beta
 *   out         [V, ld_out] fp32, required: there is no mass-only mode (nr_score_expect_news with out = NULL is that)
 *   out_mass    optional [V] fp32: sum_u p(v | u) over the live users, K18's mass with weight = NULL bit for bit -- not the sum
 *               of r
 *   the other fields and the edge cases   K18's; r_uv = 0 exactly where p_uv == 0 (0 * -inf is never formed)
 * Stream and finalize are K18's rows mode (same news tiles and k-slab counts, same plan of the user axis, same LDS, no
 * scratch), the one difference the value stored to the P tile.  Bits: K18's rule -- for a fixed explicit `splits`, row v's
 * bits depend on that row's own inputs, on the users, on U and on `splits`, not on any other news row, nor on the row's place
 * in the table or the tile.  Error bound (derived in DESIGN.md section 5) against the exact result of the fp32 inputs:
 *   |out_vc - out*_vc| <= kappa'' 2^-24 A_vc,
 *   A_vc = sum_u (1 / tau_u) (|alpha_u| + |beta_u| (|x*_uv| + 1)) p*_uv |user_uc| + sum_j |d_j| |user_jc|,
 *   kappa'' = 2 (N + 1) G + 6 C + 5 ln n + 7 K + L + 31      (K18's kappa + 2: the fma of the weight, and second order; the
 *               + 1 beside |x*| carries the absolute error of x through beta)
 *   |mass_v - mass*_v|   K18's bound with weight = 1
 *   ws          nr_score_expect_news_affine_workspace_bytes(d): K18's rows-mode size, V * slices * (N * 4 + 8) rounded to 8
 * Refused before any launch: what K18 refuses, read onto this descriptor; a null out.
 * Layout: nr_expect_news_desc with `weight` replaced by `alpha`, then `beta`.                                                  */
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N;
  int splits;
  const int32_t* excl_offsets; /* optional [V + 1]: by news */
  const int32_t* excl_users;   /* optional [n_excl]: ascending user indices per news */
  int n_excl;
  float tau;                   /* used when tau_u == NULL; finite, > 0 */
  const float* tau_u;          /* optional [U] */
  const float* base_max;       /* [U]: out_max of K13 */
  const float* base_logsum;    /* [U]: out_logsum of K13 */
  const float* alpha;          /* optional [U]; NULL = 1 */
  const float* beta;           /* optional [U]; NULL = 0 */
  int scale_inv_tau;
  const int32_t* named_offsets; /* optional [V + 1]; with named_user and named_w */
  const int32_t* named_user;    /* optional [n_named] */
  const float* named_w;         /* optional [n_named] */
  int n_named;
  float* out;                  /* [V, ld_out] */
  int ld_out;
  float* out_mass;             /* [V] or NULL */
  void* ws;
  size_t ws_bytes;
  const float* prior;    /* optional [V] */
  const int32_t* stamp;  /* optional [V]; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_expect_news_affine_desc;
size_t nr_score_expect_news_affine_workspace_bytes(const nr_expect_news_affine_desc* d);
int nr_score_expect_news_affine(const nr_expect_news_affine_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K26  KL divergence of the served distribution to a reference policy.  Two policies over the same table, lists and pools: the
 * policy p(. | u) from `user` at tau and the reference q(. | u) from `ref` at ref_tau (a logging or teacher checkpoint).  Per
 * (user, news) pair the device forms
 *   x_v = log p_v = fmaf(s_v  - max , 1 / tau , -logsum ),   p_v = expf(x_v)                  (K23's formation)
 *   y_v = log q_v = fmaf(s'_v - max', 1 / tau', -logsum'),   s'_v = fl(<news_v, ref_u> + prior_v)
 * s' by the same scoring tile and chain as every other score (the reference vectors are further rows of the user tile), so its
 * bits are what nr_score_logz(news, ref, tau', same lists and pools) sees, and (max', logsum') is that call's base.
 * d_v = x_v - y_v is formed in fp64 from the two fp32 values.  Per user, over exactly the news K13 sums over for the POLICY,
 *   m0 = sum p,   m1 = sum p x,   k1 = sum p d,   k2 = sum p d x
 * and four results, each [U] fp32 (metrics.kl_reference states the contract on the host):
 *   out_kl        KL(p || q) = k1.  Not clamped: rounding may leave a tiny negative value
 *   out_entropy   optional: H = -m1 (K23's)
 *   out_cov       optional: Cov_p(d, x) = k2 - k1 m1 (formed in fp64);  d KL / d tau = -out_cov / tau
 *   out_mass      optional: m0
 * A pair with p == 0 is a term of no sum (0 * +-inf is never formed).  No [U, V] matrix exists.
 *   edge cases  nothing eligible for the policy (base_max = -inf, whatever else holds): 0, 0, 0, 0.  Else a tau_u or ref_tau_u
 *               entry that is <= 0, NaN or infinite, a NaN in either base, or a reference maximum that is not finite (-inf: the
 *               reference has nothing eligible while the policy has): NaN for that user's four results, nobody else's change.
 *               The reference equal to the policy (same vectors, temperature and base): out_kl == 0.0 and out_cov == 0.0
 *               exactly (x and y are then the same bits).  A pair that is a term for the policy and whose reference score is
 *               NaN gives y = NaN, and so that user NaN; a reference score of -inf gives KL = +inf.
 * Bits.  Per pair the products are formed in fp64 from the fp32 p, x and y and added to four per-lane fp64 chains over the lane's
 * news of the slice (which lane sees which id is fixed by V); an xor butterfly leaves one quadruple per (user, slice); a second
 * kernel adds the slices in ascending order in fp64 and rounds each result to fp32 once.  For a fixed explicit `splits` a user's
 * results depend on that user's inputs and V only -- not on U, the user tile or the place in it.
 * Error bounds (derived in DESIGN.md section 5; first order in e = 2^-24) against the exact values of the fp32 inputs.  x carries
 * the absolute error kappa_x e (K23's), y carries kappa_y e = the same expression with the reference's (n, C', G'); with
 * A = sum p* |d*|, B = sum p* |d* x*|, D = max_v |d*_v| + 1 over the terms:
 *   |KL - KL*|   <= ((kappa_x + 8) A + kappa_x + kappa_y + 1) e + n 2^-126 D
 *   |cov - cov*| <= ((kappa_x + 8) (B + 2 A H*) + 2 (kappa_x + kappa_y) H* + 2 kappa_x A + 1) e + n 2^-119 D
 *   |H - H*|, |mass - 1|   K23's
 *   ws          nr_score_kl_workspace_bytes(d): U * slices * 32 bytes (0 = bad descriptor)
 * The stream is K13's (segments, slices, LDS) with a tile of 2 x (users per workgroup) rows: 32 users per workgroup up to
 * N = 480, 16 up to 960, else 8.
 * Refused before any launch: what K17 refuses of the shared fields; a scalar ref_tau that is not finite and > 0; a null ref,
 * ref_base_max or ref_base_logsum; an ld_ref that is not a multiple of 4 and >= N, or a ref off a 16-byte boundary; a null
 * base_max / base_logsum / out_kl; an undersized workspace.
 * Layout: nr_entropy_desc's fields in its order up to base_logsum, then the reference's, the results, then the shared tail.  */
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N;
  int splits;
  const int32_t* excl_offsets; /* optional [U + 1]: as in nr_topk_desc */
  const int32_t* excl_ids;     /* optional [n_excl]: as in nr_topk_desc */
  int n_excl;
  float tau;                   /* used when tau_u == NULL; finite, > 0 */
  const float* tau_u;          /* optional [U] */
  const float* base_max;       /* [U]: out_max of K13 for `user` at tau */
  const float* base_logsum;    /* [U]: out_logsum of K13 for `user` at tau */
  const float* ref;            /* [U, ld_ref]: the reference user vectors */
  int ld_ref;
  float ref_tau;               /* used when ref_tau_u == NULL; finite, > 0 */
  const float* ref_tau_u;      /* optional [U] */
  const float* ref_base_max;   /* [U]: out_max of K13 for `ref` at ref_tau */
  const float* ref_base_logsum; /* [U]: out_logsum of K13 for `ref` at ref_tau */
  float* out_kl;               /* [U] */
  float* out_entropy;          /* optional [U] */
  float* out_cov;              /* optional [U] */
  float* out_mass;             /* optional [U] */
  void* ws;
  size_t ws_bytes;
  const float* prior;    /* optional [V] */
  const int32_t* stamp;  /* optional [V]; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_kl_desc;
size_t nr_score_kl_workspace_bytes(const nr_kl_desc* d);
int nr_score_kl(const nr_kl_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K27  K24 with a weight that is also affine in the reference's log-probability: the gradient of K26.  With x, y, p of K26,
 *   out[u] = (sum_v r_v news_v - sum_t sub_w[u, t] news[sub_ids[u, t]]) (* 1 / tau_u),
 *   r_v = p_v fmaf(gamma_u, y_v, fmaf(beta_u, x_v, alpha_u)).
 * d KL(p || q) / d user = (1 / tau) sum_v p_v (d_v - KL) news_v, so d (kappa KL) / d user is one call with alpha = -kappa KL,
 * beta = kappa, gamma = -kappa and scale_inv_tau; added to K24's (alpha, beta) it serves sum_t g_t nll_t + h H + kappa KL in one
 * call.  metrics.expect_kl_reference states the contract on the host.
 *   alpha, beta optional [U] fp32, K24's (NULL = 1 and 0);  gamma  optional [U] fp32 (NULL = 0)
 *               A NaN in a user's alpha, beta or gamma gives that user a row of NaN (where it has a weight at all) and touches
 *               nobody else.  With gamma = 0 (or NULL) and a finite y the weight is K24's; rows then agree with K24's to within
 *               the two bounds (the user tiles, and so the slices chosen for splits = 0, differ).
 *   ref, ld_ref, ref_tau, ref_tau_u, ref_base_max, ref_base_logsum   K26's fields and meaning
 *   the other fields   K24's; r_v = 0 exactly where p_v == 0;  out_mass stays sum_v p_v
 *   edge cases  K26's: nothing eligible for the policy: only the named rows, mass 0; a bad tau / ref_tau entry, a NaN in either
 *               base or a reference maximum that is not finite: a row of NaN and mass NaN for that user, nobody else's change.
 * Stream: K24's with a score tile of twice the rows per user (the scoring tile does twice K24's work per user); the second
 * contraction is K24's.  32 users per workgroup up to 13 k-slabs of 32 columns (N <= 416), 16 up to 26 (N <= 832), else 8; no
 * instantiation uses scratch.  Finalize: K24's.  Bits: K17's rule -- for a fixed explicit `splits` a user's row depends on that
 * user's inputs, V and N only.  Error bound (derived in DESIGN.md section 5):
 *   |out_c - out*_c| <= kappa'' e A_c,   A_c = sum_v p*_v (|alpha| + |beta| (|x*_v| + 1) + |gamma| (|y*_v| + 1)) |news_vc|,
 *   kappa'' = max(kappa' + 1, kappa_y)    (K24's kappa' and the rounding of the gamma fma; the + 1 beside |y*| carries the
 *               absolute error kappa_y e of y through gamma, as the one beside |x*| carries kappa_x <= kappa' through beta)
 *   ws          nr_score_expect_kl_workspace_bytes(d): U * slices * (N * 4 + 8) rounded to 8 (K17's formula)
 * Refused before any launch: what K24 refuses, and K26's refusals of the reference fields.
 * Layout: nr_expect_affine_desc with gamma and K26's six reference fields after `beta`.                                      */
typedef struct {
  const float* news_vecs;
  int ld_news, V;
  const float* user;
  int ld_user, U;
  int N;
  int splits;
  const int32_t* excl_offsets; /* optional [U + 1]: as in nr_topk_desc */
  const int32_t* excl_ids;     /* optional [n_excl]: as in nr_topk_desc */
  int n_excl;
  float tau;                   /* used when tau_u == NULL; finite, > 0 */
  const float* tau_u;          /* optional [U] */
  const float* base_max;       /* [U]: out_max of K13 for `user` at tau */
  const float* base_logsum;    /* [U]: out_logsum of K13 for `user` at tau */
  const float* alpha;          /* optional [U]; NULL = 1 */
  const float* beta;           /* optional [U]; NULL = 0 */
  const float* gamma;          /* optional [U]; NULL = 0 */
  const float* ref;            /* [U, ld_ref]: the reference user vectors */
  int ld_ref;
  float ref_tau;               /* used when ref_tau_u == NULL; finite, > 0 */
  const float* ref_tau_u;      /* optional [U] */
  const float* ref_base_max;   /* [U]: out_max of K13 for `ref` at ref_tau */
  const float* ref_base_logsum; /* [U]: out_logsum of K13 for `ref` at ref_tau */
  const int32_t* sub_ids;      /* optional [U, ld_sub]; with sub_w */
  const float* sub_w;          /* optional [U, ld_sub]; with sub_ids */
  int ld_sub, T;
  int scale_inv_tau;
  float* out;                  /* [U, ld_out] */
  int ld_out;
  float* out_mass;             /* optional [U] */
  void* ws;
  size_t ws_bytes;
  const float* prior;    /* optional [V] */
  const int32_t* stamp;  /* optional [V]; with window */
  const int32_t* window; /* optional [U, ld_window]: (lo, hi); with stamp */
  int ld_window;
} nr_expect_kl_desc;
size_t nr_score_expect_kl_workspace_bytes(const nr_expect_kl_desc* d);
int nr_score_expect_kl(const nr_expect_kl_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * f1  device-side batch assembly -- DatasetTrain.line_mapper's `news_combined[...]` gathers + the positive splice +
 * the DataLoader collate, src/dataset.py:44-49, src/main.py:89-103.  Only news INDICES come from the host (once per
 * epoch); the feature rows are gathered here.
 *   news_combined [n_rows, F] int32 (src/preprocess.py:50-72: title token ids, or [news, category, subcategory] ids)
 *   hist_idx [B, H] news indices (front padded with 0, src/dataset.py:17-24); pos_idx [B]; neg_idx [B, K];
 *   label [B] int64 = position of the positive (random.randint(0, K), src/dataset.py:45)
 *   history [B, H, F] = news_combined[hist_idx]
 *   candidate [B, 1+K, F]: slot j holds neg[j] for j < label, pos for j == label, neg[j-1] beyond (src/dataset.py:46)
 * bad (optional, DEVICE int32, accumulated): number of out-of-range indices / labels met (row 0 / label 0 is used
 * instead; numpy / torch would raise IndexError).  An index outside [0, n_rows) counts once per slot (not once per
 * feature), a label outside [0, K] once per impression, compared as int64; the slots of that impression are then
 * checked in the order label 0 gives.  H == 0 and K == 0 are valid (hist_idx / history resp. neg_idx may be NULL).  */
int nr_assemble_batch(const int32_t* news_combined, int n_rows, int F, const int32_t* hist_idx, const int32_t* pos_idx,
                      const int32_t* neg_idx, const int64_t* label, int B, int H, int K, int32_t* history, int32_t* candidate,
                      int32_t* bad, nr_stream_t stream);

/* One encoder batch, Model.forward's `torch.cat([candidate titles, history titles])` (the reference encodes the two in two
 * passes, src/model/NRMS.py:87,90 / src/model/NAML.py forward; one pass here) plus the "is this title's vector used at all"
 * flags of the rows: out [rows_a + rows_b, F] = [a ; b], flags [rows_a + rows_b] = [1 .. 1 ; mask_b != 0] (flags and mask_b
 * optional; a NULL mask_b flags every row).  mask_b != 0 is the comparison of numbers: +0 and -0 give 0, subnormals and
 * NaN give 1.  rows_a == 0 and rows_b == 0 are valid (both: nothing is launched).                                    */
int nr_stack_rows(const int32_t* a, int rows_a, const int32_t* b, int rows_b, int F, const float* mask_b, int32_t* out,
                  int32_t* flags, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * f2  on-device ranking metrics -- src/metrics.py:5-23 (dcg/ndcg/mrr), sklearn roc_auc_score (src/metrics.py:1),
 * accumulated as src/main.py:249-263 does.  Impression i owns score / label entries [offsets[i], offsets[i+1]).
 * Impressions whose labels are all 0 or all 1 are skipped (src/main.py:250).  Computed in fp64.
 *   per_imp: workspace of nr_eval_metrics_workspace_bytes(n_imp) bytes; afterwards row i = [AUC, MRR, nDCG@5, nDCG@10]
 *            of impression i (AUC = -1 marks a skipped impression)
 *   sums[5] (fp64, overwritten) = [scored impressions, sum AUC, sum MRR, sum nDCG@5, sum nDCG@10], reduced in a
 *            fixed order (bit-reproducible)
 * max_cand: largest candidate count of an impression (host knowledge of `offsets`); at most 4096.
 * Ties between scores: descending order with the LATER candidate first (np.argsort(kind="stable")[::-1]); numpy's
 * default sort leaves the order of tied scores unspecified.  +0 and -0 tie; +-inf and subnormal scores order as numbers.
 * A label != 0 is a positive, and every positive has gain 1 (the reference's labels are 0 / 1, where its 2^y - 1 is the
 * same); an impression without candidates is skipped like any other single-class one.  AUC is the Mann-Whitney
 * statistic with half credit for a positive and a negative that tie.
 * Outside the contract: NaN scores (a NaN compares false with everything, so a positive with a NaN score is counted at
 * rank 0 without any AUC credit and a NaN negative neither outranks nor ties anything: the row is finite but means
 * nothing -- filter NaN before the call), and an impression longer than max_cand (max_cand is not checked against
 * `offsets` on the device; a longer impression overruns its wave's share of LDS).                                */
size_t nr_eval_metrics_workspace_bytes(int n_imp);
int nr_eval_metrics(const float* score, const int32_t* label, const int32_t* offsets, int n_imp, int max_cand, double* per_imp,
                    size_t per_imp_bytes, double* sums, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * f4  Adam (torch.optim.Adam defaults of src/main.py:76: no weight decay, no amsgrad) over ONE flat fp32 bucket:
 *   g' = grad * grad_scale (the 1/world of the gradient all-reduce-mean, src/main.py:82 semantics)
 *   m = lerp(m, g', 1-beta1); v = beta2 v + (1-beta2) g'^2;
 *   param -= lr / (1-beta1^step) * m / (sqrt(v) / sqrt(1-beta2^step) + eps)
 * zero_grad != 0: grad is cleared in the same pass (the next step's optimizer.zero_grad(), src/main.py:108).
 * step >= 1 is the 1-based update count.  Buffers 16-byte aligned.                                               */
int nr_adam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1, float beta2, float eps,
                 int step, float grad_scale, int zero_grad, nr_stream_t stream);
/* The same update, plus the packed bf16 GEMM operands of parameter matrices that live in the bucket (what nr_cast_pad would
 * make of the new values -- bit-identical -- written in the same pass).  Job j: the matrix at elements [first, first + count)
 * of the bucket, `cols` columns per row (a multiple of 4, as is `first`), goes to dst [count / cols, ld_dst] bf16; padding
 * columns of dst are not touched (nr_cast_pad zeroed them when the operand was first made).  At most NR_ADAM_PACK_MAX jobs.
 * Refused before any launch: more jobs, first % 4 != 0, cols < 4 or cols % 4 != 0, count % cols != 0, count >= 2^32,
 * first + count > n, ld_dst < cols or ld_dst % 4 != 0, a dst that is not 8-byte aligned.  Jobs do not reach the n % 4 tail
 * elements, and elements outside every job have no packed copy written.                                              */
#define NR_ADAM_PACK_MAX 4
typedef struct {
  size_t first, count;
  int cols, ld_dst;
  void* dst;
} nr_pack_job;
int nr_adam_step_packed(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1, float beta2, float eps,
                        int step, float grad_scale, int zero_grad, const nr_pack_job* jobs, int n_jobs, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * f4, row-deferred: the same Adam over a [rows, width] fp32 table inside the bucket (an embedding table whose gradient is
 * zero outside the rows of the batch), touching only the rows named by `ids`.  Dense Adam also moves a row whose gradient is
 * zero (its moments decay), but that motion depends only on the row's own p, m, v and the step number: row_step[r] counts the
 * steps row r has had, and the missing ones are REPLAYED -- the dense kernel's arithmetic with a zero gradient and the
 * scalars of that step, kept in `sched` -- before the row is read or stepped again.  The result is bit-identical to
 * nr_adam_step_packed over the whole table at every step.
 *   ids == NULL            every row (a flush: brings the whole table to `upto`, after which it is what dense Adam holds)
 *   ids outside [1, rows)  skipped; row 0 is the padding_idx row: no gradient, zero moments, it never moves
 *   upto                   rows are first brought to `upto` steps by zero-gradient replay
 *   apply                  0: catch-up only (before a forward reads the rows).  1: then step upto + 1 with `grad` (scaled by
 *                          grad_scale), and, with zero_grad != 0, the row's gradient is cleared.  The call derives that step's
 *                          scalars from lr / beta1 / beta2 exactly as nr_adam_step_packed does and files them under
 *                          sched[upto + 1] for later replays: sched (float2 per step, zero filled) needs upto + apply <
 *                          sched_capacity and must see EVERY step once, also one without ids (n_ids = 0, ids non-NULL).
 *   pack_dst               optional packed bf16 copy of the table, [rows * width / pack_cols, pack_ld], kept current for the
 *                          rows written (as nr_pack_job)
 *   ws                     nr_adam_rows_workspace_bytes(n_ids) bytes (a flush: n_ids = rows), 16-byte aligned
 * eps == 0 is refused: dense Adam makes NaN of every never-touched row then.  Two launches, no host synchronisation.  */
typedef struct {
  float *param, *grad, *exp_avg, *exp_avg_sq;
  int rows, width;
  int32_t* row_step;
  float* sched;
  int sched_capacity;
  const int32_t* ids;
  int ids_stride, n_ids;
  int upto, apply, zero_grad;
  float lr, beta1, beta2, eps, grad_scale;
  void* pack_dst;
  int pack_cols, pack_ld;
  void* ws;
  size_t ws_bytes;
} nr_adam_rows_desc;
size_t nr_adam_rows_workspace_bytes(int n_ids);
int nr_adam_rows(const nr_adam_rows_desc* d, nr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Per-kernel timing (measurement only).  While enabled, every kernel launch inside the library is
 * bracketed by hipEventRecord on the launch stream.  nr_prof_collect waits for the recorded events,
 * writes one line per label "label<TAB>launches<TAB>total_ms\n" into buf (host), clears the log and
 * returns the number of bytes written (or a negative NR_ERR_* code).                          */
/* on = 1: every launch; on = 2: only launches that work on >= 65 536 rows (a pair of event records costs ~3 us of
 * stream time, which adds up over the ~60 small launches of a step); on = 3: only launches whose label starts with the
 * prefix given to nr_prof_filter (one kernel: the timed region of a benchmark pays for two event records per step);
 * on = 0: off.                                                                                  */
int nr_prof_enable(int on);
int nr_prof_filter(const char* label_prefix);
int nr_prof_collect(char* buf, size_t n);

/* ---------------------------------------------------------------------------------------
 * The two MFMA GEMM building blocks on dense operands (used by every op above; exported for unit tests
 * and kernel-level measurement).  A [M, lda], B [N, ldb] of dtype; C [M, ldc] of out_dtype:
 *   nr_gemm_nt:  C = A . B^T (+ bias[N]) (tanh if act_tanh)
 *   nr_gemm_tn:  dW[N, ldw] (fp32) += dC[M, ldc]^T . A[M, lda] ; db[N] += column sums of dC (db may be NULL)
 * K (and for nr_gemm_tn N), lda, ldb and the ldc of dC are multiples of the 16-byte chunk, ldc of C a multiple of 4; a call
 * that breaks this, an operand off a 16-byte boundary or an empty problem returns NR_ERR_ARG before anything is launched.
 * B padding (nr_gemm_nt, NR_BF16): when ldb >= roundup32(K), the columns [K, roundup32(K)) of every row of B MUST BE ZERO.
 * The LDS-DMA and weights-in-registers kernels, which such a call may take, run whole 32-deep k-steps and do not predicate
 * the K tail of B.  nr_cast_pad with ld_dst >= roundup32(cols) (ops.pack(..., ld=), and its default ld) produces exactly
 * this.  With ldb < roundup32(K) (e.g. ldb == K) the call takes kernels that predicate the tail, and whatever follows
 * column K -- the next row's data -- is not read.  Columns from roundup32(K) on are never read.  A has NO such requirement:
 * its K tail is clamped to valid columns, so the slack columns [K, lda) of A may hold anything, NaN included.
 * nr_gemm_tn in deterministic mode (nr_set_deterministic) accumulates dW and db in fixed point like every other weight
 * gradient; the scratch then needs (N - 1) * ldw + K + N elements. */
int nr_gemm_nt(int dtype, const void* A, int lda, const void* B, int ldb, const float* bias, int act_tanh, void* C,
               int ldc, int out_dtype, int M, int N, int K, nr_stream_t stream);
int nr_gemm_tn(int dtype, const void* dC, int ldc, const void* A, int lda, float* dW, int ldw, float* db, int M, int N,
               int K, nr_stream_t stream);

/* Test hook: materialise the dropout keep mask (1.0 / 0.0) for `count` element indices. */
int nr_dropout_mask(float* out, uint32_t count, float p, uint32_t seed, nr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NRHIP_H */
