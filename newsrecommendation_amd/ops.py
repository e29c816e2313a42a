"""torch.autograd bindings of the libnrhip C ABI (include/nrhip.h).

PyTorch supplies device memory, the current HIP stream and autograd bookkeeping; every
arithmetic step on the hot path runs in the hand-written HIP kernels.  Tensors must live on
the GPU: there is no CPU fallback (a RuntimeError is raised instead).
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from typing import Optional

import torch
from torch.autograd import Function

from . import _lib
from ._lib import NR_BF16, NR_F32, NR_SRC_DENSE, NR_SRC_GATHER, check, ptr

_DTYPES = {"fp32": NR_F32, "f32": NR_F32, "float32": NR_F32, "bf16": NR_BF16, "bfloat16": NR_BF16}


def dtype_code(name) -> int:
    if isinstance(name, int):
        return name
    try:
        return _DTYPES[str(name).lower()]
    except KeyError:
        raise ValueError(f"compute dtype must be one of {sorted(_DTYPES)}, got {name!r}")


def torch_dtype(code: int) -> torch.dtype:
    return torch.bfloat16 if code == NR_BF16 else torch.float32


def chunk(code: int) -> int:
    return 8 if code == NR_BF16 else 4


def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(*ts) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("newsrecommendation_amd ops need GPU tensors (libnrhip has no CPU fallback); "
                               f"got a tensor on {t.device}")


# Test hook: when True, buffers the kernels are documented to leave partly unwritten (qkv / dqkv rows of all-padding
# sequences) are pre-filled with NaN, so a read of an unwritten row poisons the result instead of passing silently.
POISON_WORKSPACES = False


def _scratch(*shape, dtype, device):
    t = torch.empty(*shape, dtype=dtype, device=device)
    if POISON_WORKSPACES and t.is_floating_point():
        t.fill_(float("nan"))
    return t


# Index validation (what torch.nn.functional.embedding / cross_entropy raise IndexError for).  The kernels trust their
# indices; with CHECK_INDICES on (env NR_CHECK_INDICES=1, or set the attribute) every id / label tensor is range-checked
# on the device before use, at the price of one host synchronisation per check.
CHECK_INDICES = os.environ.get("NR_CHECK_INDICES", "0") not in ("", "0")


def check_ids(ids: torch.Tensor, rows: int, what: str = "index") -> None:
    """Raise IndexError if any entry of the int32 tensor `ids` (any 1-D stride) lies outside [0, rows)."""
    if ids.numel() == 0:
        return
    bad = torch.zeros(1, dtype=torch.int32, device=ids.device)
    if ids.dim() == 1:
        count, stride, base = ids.shape[0], ids.stride(0), ids
    else:
        base = ids.contiguous()
        count, stride = base.numel(), 1
    check(_lib.lib().nr_check_ids(ptr(base), count, stride, int(rows), ptr(bad), _stream()), "nr_check_ids")
    n = int(bad.item())
    if n:
        raise IndexError(f"{what}: {n} entries outside [0, {rows})")


def check_labels(label: torch.Tensor, classes: int) -> None:
    bad = torch.zeros(1, dtype=torch.int32, device=label.device)
    check(_lib.lib().nr_check_labels(ptr(label), label.numel(), int(classes), ptr(bad), _stream()), "nr_check_labels")
    n = int(bad.item())
    if n:
        raise IndexError(f"label: {n} entries outside [0, {classes})")


def _ws(nbytes: int, device) -> torch.Tensor:
    """A workspace of the size the library asked for (bytes -> int32 elements)."""
    return torch.empty((int(nbytes) + 3) // 4, dtype=torch.int32, device=device)


# Zero-gradient hint between two adjacent backward calls: the pooling backward knows which sequences had a zero pooled
# gradient (their dx rows are exact zeros) and leaves [n] flags in its workspace; when the VERY NEXT libnrhip backward call
# is the producer of the pooled tensor (MHSA / conv) and receives that same dx buffer as its dy, it takes the flags
# instead of scanning dy (0.1 ms at the bench shape).  Anything else in between drops the hint.
_bwd_seq = 0
_flag_hint = None


def _enter_backward() -> int:
    global _bwd_seq
    _bwd_seq += 1
    return _bwd_seq


def _offer_flags(seq, dx, n, flags_ptr, keepalive, lazy=False) -> None:
    """lazy: the dx rows of sequences whose flag is 0 are zeros only NEAR flagged ones and unwritten memory elsewhere
    (nr_pool_desc.dx_far_unwritten): the taker must be told, and a consumer that cannot take the flags must not read dx."""
    global _flag_hint
    if dx is not None:
        dx._nr_lazy_rows = bool(lazy)
    # dx._version: autograd may ADD another consumer's gradient into dx in place (same pointer, same size) before the next
    # libnrhip backward sees it -- the flags would then drop sequences whose gradient is no longer zero
    _flag_hint = ((seq, dx.data_ptr(), dx.numel(), n, flags_ptr, keepalive, dx._version, weakref.ref(dx), bool(lazy))
                  if flags_ptr and dx is not None else None)


def _take_flags(seq, dy, n):
    """(device pointer, keep-alive tensor, lazy) of the [n] flags for `dy`, or (0, None, False)."""
    global _flag_hint
    h, _flag_hint = _flag_hint, None
    if h is not None and h[0] == seq - 1 and h[1] == dy.data_ptr() and h[2] == dy.numel() and h[3] == n:
        dx = h[7]()
        if dx is not None and dx._version == h[6] and dy._version == h[6]:
            return h[4], h[5], h[8]
    if getattr(dy, "_nr_lazy_rows", False):
        raise RuntimeError("this gradient was produced with unwritten rows for zero-gradient sequences (additive_pool lazy_dx=True) "
                           "but the flags that say which ones did not reach its consumer: something else ran between the two backward "
                           "calls -- construct the pooling with lazy_dx=False")
    return 0, None, False


# Deterministic mode (nr_set_deterministic): gradients that several workgroups add into are accumulated in fixed point with
# integer atomics, so they are bit-reproducible from run to run.  Costs a zeroed scratch of 8 bytes per accumulated element
# of the largest backward call and a flush pass per call; off by default.
_det_scratch = None


def set_deterministic(on: bool, elements: int = 1 << 24, device=None) -> None:
    """on: register a zero-filled scratch of `elements` int64 (default 16 M = 128 MB: NRMS with a 30 000-row trainable
    word table needs 3*400*301 + 30 000*300 = 9.4 M) with libnrhip; off: plain fp32 atomics again."""
    global _det_scratch
    if on:
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        _det_scratch = torch.zeros(int(elements), dtype=torch.int64, device=dev)
        check(_lib.lib().nr_set_deterministic(ptr(_det_scratch), _det_scratch.numel() * 8), "nr_set_deterministic")
    else:
        check(_lib.lib().nr_set_deterministic(None, 0), "nr_set_deterministic")
        _det_scratch = None


def grad_target(p):
    """The preallocated gradient view of a parameter that lives in a flat bucket (parallel.FlatBucket sets
    `_nr_grad`), or None.  Backward passes ACCUMULATE into such a view directly -- the kernels add into their dW / db /
    dtable outputs anyway -- and hand autograd None for that parameter: no per-call zero fill, no AccumulateGrad copy."""
    return getattr(p, "_nr_grad", None) if p is not None else None


def draw_seed() -> int:
    """A 31-bit dropout seed from torch's CPU generator (reproducible under torch.manual_seed)."""
    return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())


class _PackCache:
    """Packed copies of the small weights that live in a flat parameter bucket (parallel.FlatBucket registers its buffer).
    A training step asks for the same ~9 packs (Q|K|V and att_fc1 weights, plain and transposed) after every optimizer
    step; each used to be its own 6-us launch.  Here the first request after a parameter update (ops.param_epoch moved, or a
    torch-side in-place write bumped the tensor's version) refreshes EVERY pack seen so far in ONE launch (nr_cast_pad_batch).
    Tensors outside a registered bucket are never cached."""
    MAX_ELEMS = 1 << 21                # (larger operands -- embedding tables -- go through _TableCache)

    def __init__(self):
        self._ranges = []              # (first byte, last byte + 1) of registered flat parameter buffers
        self._e = {}                   # key -> [src view, dst, transpose, code, stamp]

    def register_buffer(self, t: torch.Tensor, versions=None) -> None:
        """t: the bucket's flat parameter tensor.  Its packs are served for as long as that tensor object lives.
        versions: optional callable -> tuple of the version counters of the Parameters that live in `t` (a Parameter whose
        `.data` was pointed at a view of `t` keeps its own counter, so `t._version` alone misses torch-side writes to it)."""
        self._ranges.append((weakref.ref(t), t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), versions))

    def clear(self) -> None:
        self._ranges, self._e = [], {}

    def _purge(self) -> None:
        dead = [(a, b) for r, a, b, _ in self._ranges if r() is None]
        if dead:
            self._ranges = [x for x in self._ranges if x[0]() is not None]
            for k in [k for k in self._e if any(a <= k[0] < b for a, b in dead)]:
                del self._e[k]

    def _bucket_versions(self, src):
        """None: `src` lies in no registered bucket (never cached); else the bucket's parameter-version tuple (or ())."""
        self._purge()
        if src.numel() > self.MAX_ELEMS:
            return None
        p = src.data_ptr()
        for _, a, b, versions in self._ranges:
            if a <= p < b:
                return versions() if versions is not None else ()
        return None

    def get(self, src, code, transpose, ld):
        bv = self._bucket_versions(src)
        if bv is None:
            return None
        key = (src.data_ptr(), tuple(src.shape), bool(transpose), int(ld), int(code), src.device.index)
        stamp = (param_epoch, src._version, bv)
        ent = self._e.get(key)
        if ent is not None and ent[4] == stamp:
            return ent[1]
        if ent is None:
            rows, cols = src.shape
            dst = torch.empty(cols if transpose else rows, ld, dtype=torch_dtype(code), device=src.device)
            ent = self._e[key] = [src, dst, bool(transpose), int(code), None]
        # refresh this entry and every other stale one of the same dtype / device in one launch
        def stamp_of(e):
            return (param_epoch, e[0]._version, self._bucket_versions(e[0]))
        todo = [e for k, e in self._e.items()
                if e[3] == code and k[5] == src.device.index and e[4] != stamp_of(e)][:_lib.CAST_BATCH_MAX]
        if not any(e is ent for e in todo):
            todo = [ent] + todo[:_lib.CAST_BATCH_MAX - 1]
        jobs = (_lib.CastJob * len(todo))()
        for j, e in zip(jobs, todo):
            r, c = e[0].shape
            j.src, j.dst, j.rows, j.cols, j.ld_src, j.ld_dst, j.transpose = ptr(e[0]), ptr(e[1]), r, c, c, e[1].shape[1], int(e[2])
        check(_lib.lib().nr_cast_pad_batch(jobs, len(todo), code, _stream()), "nr_cast_pad_batch")
        for e in todo:
            e[4] = stamp_of(e)
        return ent[1]


pack_cache = _PackCache()


def pack(src: torch.Tensor, code: int, transpose: bool = False, ld: Optional[int] = None) -> torch.Tensor:
    """fp32 [rows, cols] -> compute-dtype GEMM operand, leading dimension zero-padded to a 16-byte chunk."""
    _need_gpu(src)
    src = src.detach()
    if src.dtype != torch.float32 or not src.is_contiguous():
        src = src.float().contiguous()
    rows, cols = src.shape
    drows, dcols = (cols, rows) if transpose else (rows, cols)
    # bf16: leading dimension rounded up to 32 and zero padded, so the LDS-DMA GEMM can run whole 32-deep k-steps
    ld = ld or round_up(dcols, 32 if code == NR_BF16 else chunk(code))
    cached = pack_cache.get(src, code, transpose, ld)
    if cached is not None:
        return cached
    dst = torch.empty(drows, ld, dtype=torch_dtype(code), device=src.device)
    check(_lib.lib().nr_cast_pad(ptr(src), rows, cols, cols, ptr(dst), ld, code, int(transpose), _stream()), "nr_cast_pad")
    return dst


class _TableCache:
    """Compute-dtype copies of embedding tables, refreshed when the fp32 master changes (tensor version counter,
    storage pointer, shape), so a frozen table is packed once.

    An entry lives exactly as long as the Parameter it was packed from: the key is `id(weight)`, and a
    `weakref.finalize` on that Parameter evicts the entry when the Parameter is collected, so a recycled `id()` can
    never be served another model's table and dead tables do not stay pinned in HBM.  A held weak reference is
    compared on every hit as well.  Writes that bypass autograd's version counter (`weight.data.copy_(...)`, as a
    parameter broadcast does) need an explicit `table_cache.invalidate(weight)`."""

    def __init__(self):
        self._c = {}
        self._watched = set()            # ids of parameters that carry an eviction finalizer

    def _drop(self, wid):
        for key in [k for k in self._c if k[0] == wid]:
            del self._c[key]

    def _evict(self, wid):                # the parameter died
        self._drop(wid)
        self._watched.discard(wid)

    def invalidate(self, weight=None):
        """Forget the packed copy of `weight` (all copies if None); the next use re-packs from the fp32 master."""
        if weight is None:
            self._c.clear()
        else:
            self._drop(id(weight))

    def current(self, weight):
        """[(code, row_cols, packed copy)] of the up-to-date entries of `weight` (what an optimizer that rewrites the master
        behind autograd's back can refresh in place instead of invalidating, parallel.FlatBucket.adam_step)."""
        w = weight.detach()
        sig = (weight._version, w.data_ptr(), tuple(w.shape))
        return [(k[1], k[2], e[1]) for k, e in self._c.items() if k[0] == id(weight) and e[0] == sig and e[2]() is weight]

    def get(self, weight: torch.Tensor, code: int, row_cols: Optional[int] = None) -> torch.Tensor:
        w = weight.detach()
        cols = row_cols or w.shape[1]
        if code == NR_F32 and cols % 4 == 0 and w.is_contiguous() and w.dtype == torch.float32:
            return w.view(-1, cols)                       # already a valid operand: no copy
        key = (id(weight), code, cols)
        ent = self._c.get(key)
        sig = (weight._version, w.data_ptr(), tuple(w.shape))
        if ent is None or ent[0] != sig or ent[2]() is not weight:
            if id(weight) not in self._watched:
                self._watched.add(id(weight))
                weakref.finalize(weight, self._evict, id(weight))
            ent = (sig, pack(w.reshape(-1, cols), code), weakref.ref(weight))
            self._c[key] = ent
        return ent[1]


table_cache = _TableCache()

# Bumped whenever parameters are rewritten behind autograd's back (parallel.FlatBucket's Adam kernel): caches derived from
# parameter VALUES (not just from their version counters) key on it.
param_epoch = 0


def bump_param_epoch() -> None:
    global param_epoch
    param_epoch += 1


class _ProjectedTables:
    """Eval-mode shortcut of the title-level MHSA: without input dropout Q|K|V of a token are
    `W_{Q|K|V} e_w + b` of its table row e_w -- a function of the token ID alone -- so the [V, d_model] table is projected
    ONCE to [V, 3N] (one GEMM over V rows instead of one over every token occurrence: 100 000 news x 30 tokens -> 30 000
    rows) and the attention kernel gathers projected rows.  Same GEMM kernel, same operands, same rounding as projecting each
    occurrence: the values are identical.  Rebuilt when the table, a weight or the parameter epoch changes."""

    def __init__(self):
        self._c = {}

    def get(self, table, params, wcat, bcat, code):
        sig = (param_epoch, table._version, table.data_ptr()) + tuple((p._version, p.data_ptr()) for p in params)
        ent = self._c.get(id(table))
        if ent is None or ent[0] != sig or ent[2]() is not table:
            tp = table_cache.get(table, code)                                  # [V, ld] packed operand
            w_p = pack(wcat, code)                                             # [3N, ld], same zero-padded K as the table
            if w_p.shape[1] != tp.shape[1]:
                raise RuntimeError(f"projected table: operand leading dimensions differ ({w_p.shape[1]} vs {tp.shape[1]})")
            proj = gemm_nt(tp, w_p, bias=bcat.detach().float().contiguous())   # [V, 3N], bias added, rounded to bf16 once
            if id(table) not in self._c:
                weakref.finalize(table, self._c.pop, id(table), None)
            ent = (sig, proj, weakref.ref(table))
            self._c[id(table)] = ent
        return ent[1]


projected_tables = _ProjectedTables()


# ------------------------------------------------------------------------------------------ MHSA
class MHSAFunction(Function):
    """K3 (+K1, K2): multi-head self-attention, src/model/model_utils.py:78-95 + :39-55, optionally with the
    embedding lookup and the dropouts of src/model/NRMS.py:28-34 folded in (gather source)."""

    @staticmethod
    def forward(ctx, x, wq, bq, wk, bk, wv, bv, ids, mask, cfg):
        # x: dense [n, L, d_model] compute dtype, or (gather) the fp32 table parameter [V, d_model]
        _need_gpu(x, wq, ids, mask)
        code, heads, gather = cfg["code"], cfg["heads"], ids is not None
        N, d_model = wq.shape
        d_head = N // heads
        ch = chunk(code)
        if gather:
            n, L = ids.shape
            src = cfg["table_packed"]
            ids = ids.contiguous()
        else:
            n, L, _ = x.shape
            src = x.contiguous()
            if src.dtype != torch_dtype(code):
                raise RuntimeError(f"dense MHSA input must be {torch_dtype(code)}, got {src.dtype}")
        ldx = src.shape[-1]
        flat = cfg.get("flat")             # W_Q|W_K|W_V (and the biases) adjacent in a flat bucket: no concatenation
        if flat is not None:
            wcat, b_p = flat["w"], flat["b"]
        else:
            wcat = torch.cat([wq, wk, wv], dim=0)
            b_p = torch.cat([bq, bk, bv]).detach().float().contiguous()
        w_p = pack(wcat, code)
        mask_c = mask.contiguous().float() if mask is not None else None
        dev = wq.device
        y = _scratch(n, L, N, dtype=torch_dtype(code), device=dev)      # (poisoned in the tests: far unneeded rows may stay unwritten)
        # training with a gather source: keep the gathered + dropped-out rows for the weight-gradient GEMM
        need_bwd = any(ctx.needs_input_grad[:7])
        keep_rows = gather and any(ctx.needs_input_grad[1:7])
        Kp = round_up(d_model, ch)
        x_rows = torch.empty(n * L, Kp, dtype=torch_dtype(code), device=dev) if keep_rows else None
        d = _lib.MhsaDesc(n=n, L=L, d_model=d_model, heads=heads, d_head=d_head, dtype=code,
                          src_kind=NR_SRC_GATHER if gather else NR_SRC_DENSE, x=ptr(src), ldx=ldx, ids=ptr(ids),
                          p_in=cfg["p_in"], seed_in=cfg["seed_in"], p_out=cfg["p_out"], seed_out=cfg["seed_out"],
                          mask=ptr(mask_c), w_qkv=ptr(w_p), ldw=w_p.shape[1], b_qkv=ptr(b_p),
                          x_rows=ptr(x_rows), ld_rows=Kp, seq_needed=ptr(cfg.get("needed")),
                          y_far_unwritten=int(bool(cfg.get("far_unwritten")) and cfg.get("needed") is not None),
                          table_rows=cfg["table_shape"][0] if gather else 0)     # (sizes the id-sort scratch of the backward)
        # scratch for the device-side compaction of non-padding rows (forward: live rows, their ids, padding rows;
        # backward: live slabs, sequence list) -- sized by the library
        row_ws = _ws(_lib.lib().nr_mhsa_workspace_bytes(C.byref(d)), dev) if keep_rows and code == _lib.NR_BF16 else None
        d.row_ws, d.row_ws_bytes = ptr(row_ws), (row_ws.numel() * 4 if row_ws is not None else 0)
        # the fused title-level kernel keeps Q|K|V on chip: without a backward they are never written to HBM
        fused = bool(_lib.lib().nr_mhsa_fwd_fused(C.byref(d)))
        qkv = None if (fused and not need_bwd) else _scratch(n * L, 3 * N, dtype=torch_dtype(code), device=dev)
        check(_lib.lib().nr_mhsa_fwd(C.byref(d), ptr(qkv), ptr(y), _stream()), "nr_mhsa_fwd")
        cfg["compact_rows"] = bool(keep_rows and _lib.lib().nr_mhsa_compact_rows(C.byref(d)))    # (read by ops.mhsa after apply)
        ctx.cfg, ctx.dims = cfg, (n, L, N, d_model, heads, d_head, ldx, gather)
        ctx.row_ws = row_ws      # the backward attention and the table-gradient GEMM reuse the compaction
        ctx.save_for_backward(src, ids, mask_c, w_p, b_p, wcat, qkv, x_rows)
        return y

    @staticmethod
    def backward(ctx, dy):
        seq = _enter_backward()
        src, ids, mask_c, w_p, b_p, wcat, qkv, x_rows = ctx.saved_tensors
        cfg = ctx.cfg
        n, L, N, d_model, heads, d_head, ldx, gather = ctx.dims
        code, dev = cfg["code"], dy.device
        dy = dy.contiguous()
        if dy.dtype != torch_dtype(code):
            dy = dy.to(torch_dtype(code))
        seq_nz, seq_nz_owner, dy_lazy = _take_flags(seq, dy, n)
        dqkv = _scratch(*qkv.shape, dtype=qkv.dtype, device=dev)
        bucket = cfg.get("flat")
        if bucket is not None:
            dw, db = bucket["gw"], bucket["gb"]                    # accumulated in place
        else:
            flat = torch.zeros(3 * N * d_model + 3 * N, dtype=torch.float32, device=dev)     # dw | db, one fill
            dw, db = flat[:3 * N * d_model].view(3 * N, d_model), flat[3 * N * d_model:]
        need_x = ctx.needs_input_grad[0]
        dx = dtable = w_t = None
        row_ws = getattr(ctx, "row_ws", None)          # what the forward compacted (padding rows of qkv were never written)
        ws_ready = row_ws is not None
        d = _lib.MhsaDesc(n=n, L=L, d_model=d_model, heads=heads, d_head=d_head, dtype=code,
                          src_kind=NR_SRC_GATHER if gather else NR_SRC_DENSE, x=ptr(src), ldx=ldx, ids=ptr(ids),
                          p_in=cfg["p_in"], seed_in=cfg["seed_in"], p_out=cfg["p_out"], seed_out=cfg["seed_out"],
                          mask=ptr(mask_c), w_qkv=ptr(w_p), ldw=w_p.shape[1], b_qkv=ptr(b_p),
                          x_rows=ptr(x_rows), ld_rows=x_rows.shape[1] if x_rows is not None else 0,
                          table_rows=cfg["table_shape"][0] if gather else 0, seq_nz=seq_nz, row_ws_ready=int(ws_ready),
                          dy_far_unwritten=int(dy_lazy),
                          seq_needed=ptr(cfg.get("needed")))     # (the forward may have left far all-padding x_rows unwritten)
        if need_x:
            w_t = pack(wcat, code, transpose=True)                     # [d_model, 3N]
            if gather:
                dtable = cfg.get("table_grad")
                if dtable is None:
                    dtable = torch.zeros(cfg["table_shape"], dtype=torch.float32, device=dev)
                if row_ws is None:
                    row_ws = _ws(_lib.lib().nr_mhsa_workspace_bytes(C.byref(d)), dev)     # live-row compaction scratch
            else:
                dx = torch.empty(n, L, ldx, dtype=torch_dtype(code), device=dev)
        d.row_ws, d.row_ws_bytes = ptr(row_ws), (row_ws.numel() * 4 if row_ws is not None else 0)
        def run(phase):
            d.bwd_phase = phase
            check(_lib.lib().nr_mhsa_bwd(C.byref(d), ptr(qkv), ptr(dy), ptr(dqkv), ptr(w_t), w_t.shape[1] if w_t is not None else 0,
                                         ptr(dw), ptr(db), ptr(dx), ptr(dtable), _stream()), "nr_mhsa_bwd")
        # A data-parallel bucket wants to know the moment the (large) table gradient is complete: the backward then runs in two
        # phases -- table gradient first, the hook starts its all-reduce, the weight-gradient GEMM runs underneath it.
        ready = cfg.get("table_grad_ready") if (gather and cfg.get("table_grad") is not None and _det_scratch is None) else None
        if ready is not None:
            run(1)
            ready()
            run(2)
        else:
            run(0)
        gx = (None if cfg.get("table_grad") is not None else dtable) if gather else dx
        if bucket is not None:
            return (gx, None, None, None, None, None, None, None, None, None)
        return (gx, dw[:N], db[:N], dw[N:2 * N], db[N:2 * N], dw[2 * N:], db[2 * N:], None, None, None)


USE_PROJECTED_TABLE = True      # eval-mode shortcut of the gather MHSA (see _ProjectedTables); off: project every occurrence


def _mhsa_projected(table, params, flat, ids, mask, heads, code, p_out):
    """No-grad, no input dropout, bf16, L <= 64: attention over projections gathered from the once-projected table.
    With a mask, the y rows at MASKED query positions are unspecified (currently zeros where the unmasked keys form one run
    at 32 < L <= 64, a context vector otherwise): the consumer must apply the same mask.  An all-masked sequence gives zeros."""
    wq, bq, wk, bk, wv, bv = params
    if flat is not None:
        wcat, bcat = flat["w"], flat["b"]
    else:
        wcat, bcat = torch.cat([wq, wk, wv], dim=0), torch.cat([bq, bk, bv])
    proj = projected_tables.get(table, params, wcat, bcat, code)
    n, L = ids.shape
    N, d_model = wq.shape
    mask_c = mask.contiguous().float() if mask is not None else None
    y = torch.empty(n, L, N, dtype=torch_dtype(code), device=ids.device)
    tp = table_cache.get(table, code)
    d = _lib.MhsaDesc(n=n, L=L, d_model=d_model, heads=heads, d_head=N // heads, dtype=code, src_kind=NR_SRC_GATHER, x=ptr(tp),
                      ldx=tp.shape[1], ids=ptr(ids), p_in=0.0, seed_in=0, p_out=p_out, seed_out=draw_seed() if p_out > 0 else 0,
                      mask=ptr(mask_c), w_qkv=ptr(proj), ldw=tp.shape[1], b_qkv=ptr(proj), proj_table=ptr(proj))
    check(_lib.lib().nr_mhsa_fwd(C.byref(d), None, ptr(y), _stream()), "nr_mhsa_fwd")
    return y


def needed_flags(needed):
    """[n] int32 flags (1 = the caller uses this sequence's output) from a bool / float / int tensor, or None."""
    if needed is None:
        return None
    if getattr(needed, "_nr_flags01", False):          # stack_rows made them: int32 0 / 1, contiguous
        return needed
    return (needed.reshape(-1) != 0).to(torch.int32).contiguous()


def pool_contracts_slabs(n: int, L: int, N: int, q: int, code: int) -> bool:
    """True when the additive-pooling backward of this shape reads only the x rows near sequences with a gradient (its weight
    gradient contracts live 32-row slabs): the producer of x may then leave far unneeded rows unwritten (mhsa far_unwritten)."""
    d = _lib.PoolDesc(n=int(n), L=int(L), N=int(N), q=int(q), dtype=int(code))
    return bool(_lib.lib().nr_pool_contracts_slabs(C.byref(d)))


def mhsa(x, wq, bq, wk, bk, wv, bv, heads: int, code: int, mask=None, ids=None, table=None, p_in=0.0, p_out=0.0, flat=None,
         needed=None, far_unwritten=False):
    """Dense: x [n, L, d_model] (compute dtype).  Gather: ids int32 [n, L] + fp32 `table` parameter.
    flat: {"w": [3N, d_model], "b": [3N], "gw", "gb"} views of a flat parameter / gradient bucket (parallel.FlatBucket).
    needed: optional [n] int32 flags (needed_flags): sequences with flag 0 reach the loss through a factor 0 only; their
    output rows are exact zeros and are not computed (their gradient is zero, so nothing flows back either).
    far_unwritten: with `needed`, the output rows of unneeded sequences farther than 32 / L + 2 sequences from every needed
    one may stay UNWRITTEN (not even zeros) -- only for a caller whose sole consumer is additive_pool with the same flags on
    a shape for which pool_contracts_slabs() holds."""
    cfg = dict(code=code, heads=heads, p_in=float(p_in), p_out=float(p_out),
               seed_in=draw_seed() if p_in > 0 else 0, seed_out=draw_seed() if p_out > 0 else 0, needed=needed,
               far_unwritten=bool(far_unwritten))
    if flat is not None:
        cfg["flat"] = flat
    if ids is not None:
        if ids.dtype != torch.int32:
            ids = ids.to(torch.int32)
        if CHECK_INDICES:
            check_ids(ids, table.shape[0], "token id")
        N = wq.shape[0]
        if (not torch.is_grad_enabled() and p_in == 0 and code == NR_BF16 and ids.dim() == 2 and ids.shape[1] <= 64
                and (N // heads) % 4 == 0 and N % 8 == 0 and USE_PROJECTED_TABLE):
            return _mhsa_projected(table, (wq, bq, wk, bk, wv, bv), flat, ids.contiguous(), mask, heads, code, float(p_out))
        cfg["table_packed"] = table_cache.get(table, code)
        cfg["table_shape"] = tuple(table.shape)
        if table.requires_grad and torch.is_grad_enabled():
            cfg["table_grad"] = grad_target(table)
            cfg["table_grad_ready"] = getattr(table, "_nr_grad_ready", None)     # parallel.FlatBucket, world > 1
        y = MHSAFunction.apply(table, wq, bq, wk, bk, wv, bv, ids, mask, cfg)
        # the backward of this call will ignore the dy rows of sequences flagged "zero gradient" (compact row storage): a pooling
        # that consumes y alone may leave them unwritten (additive_pool lazy_dx)
        y._nr_takes_lazy_dy = bool(cfg.get("compact_rows"))
        return y
    ch = chunk(code)
    if x.shape[-1] % ch:
        # d_model not a multiple of the 16-byte operand chunk: zero-pad the feature axis of x and of the weights (torch
        # plumbing on a rare shape; autograd slices the gradients back)
        pad = ch - x.shape[-1] % ch
        cfg.pop("flat", None)               # the padded weights are temporaries: gradients go through autograd
        x = torch.nn.functional.pad(x, (0, pad))
        wq, wk, wv = (torch.nn.functional.pad(w, (0, pad)) for w in (wq, wk, wv))
    return MHSAFunction.apply(x, wq, bq, wk, bk, wv, bv, None, mask, cfg)


# ------------------------------------------------------------------------------------------ attention core alone
class SDPAFunction(Function):
    """ScaledDotProductAttention.forward, src/model/model_utils.py:39-55, on packed projections [n*L, 3N]."""

    @staticmethod
    def forward(ctx, qkv, mask, n, L, heads, d_head, code):
        _need_gpu(qkv, mask)
        N = heads * d_head
        mask_c = mask.contiguous().float() if mask is not None else None
        y = torch.empty(n * L, N, dtype=torch_dtype(code), device=qkv.device)
        check(_lib.lib().nr_sdpa_fwd(ptr(qkv), ptr(mask_c), ptr(y), n, L, heads, d_head, code, 0.0, 0, _stream()), "nr_sdpa_fwd")
        ctx.dims = (n, L, heads, d_head, code)
        ctx.save_for_backward(qkv, mask_c)
        return y

    @staticmethod
    def backward(ctx, dy):
        _enter_backward()
        qkv, mask_c = ctx.saved_tensors
        n, L, heads, d_head, code = ctx.dims
        dy = dy.contiguous()
        if dy.dtype != torch_dtype(code):
            dy = dy.to(torch_dtype(code))
        dqkv = torch.empty_like(qkv)
        check(_lib.lib().nr_sdpa_bwd(ptr(qkv), ptr(mask_c), ptr(dy), ptr(dqkv), n, L, heads, d_head, code, 0.0, 0, _stream()),
              "nr_sdpa_bwd")
        return dqkv, None, None, None, None, None, None


class LongSDPAFunction(Function):
    """SDPAFunction for long clicked histories, 64 < L <= 128 (nr_sdpa_long_fwd / nr_sdpa_long_bwd): bf16 with aligned
    buffers runs on the matrix cores (RB x RB tiles of 32 x 32), everything else on the LDS/VALU kernels."""

    @staticmethod
    def forward(ctx, qkv, mask, n, L, heads, d_head, code):
        _need_gpu(qkv, mask)
        N = heads * d_head
        mask_c = mask.contiguous().float() if mask is not None else None
        y = torch.empty(n * L, N, dtype=torch_dtype(code), device=qkv.device)
        check(_lib.lib().nr_sdpa_long_fwd(ptr(qkv), ptr(mask_c), ptr(y), n, L, heads, d_head, code, 0.0, 0, _stream()),
              "nr_sdpa_long_fwd")
        ctx.dims = (n, L, heads, d_head, code)
        ctx.save_for_backward(qkv, mask_c)
        return y

    @staticmethod
    def backward(ctx, dy):
        _enter_backward()
        qkv, mask_c = ctx.saved_tensors
        n, L, heads, d_head, code = ctx.dims
        dy = dy.contiguous()
        if dy.dtype != torch_dtype(code):
            dy = dy.to(torch_dtype(code))
        dqkv = torch.empty_like(qkv)
        check(_lib.lib().nr_sdpa_long_bwd(ptr(qkv), ptr(mask_c), ptr(dy), ptr(dqkv), n, L, heads, d_head, code, 0.0, 0, _stream()),
              "nr_sdpa_long_bwd")
        return dqkv, None, None, None, None, None, None


def sdpa(Q, K, V, code: int, mask=None):
    """Q, K, V: [n, h, L, d] (any strides, e.g. the transposed views of src/model/model_utils.py:89-91); mask: [n, L], or the
    reference's per-head expansion [n, h, L] of it (:86-87) -> [n, h, L, d].  The three tensors are packed into the
    token-major [n*L, 3*h*d] layout of the kernels (torch plumbing), the attention itself runs in libnrhip."""
    _need_gpu(Q, K, V, mask)
    n, h, L, d = Q.shape
    if K.shape != Q.shape or V.shape != Q.shape:
        raise RuntimeError(f"sdpa: Q/K/V shapes differ: {tuple(Q.shape)}, {tuple(K.shape)}, {tuple(V.shape)} (d_k must equal d_v)")
    if mask is not None and mask.dim() == 3:
        if mask.stride(1) != 0 and not bool((mask == mask[:, :1]).all()):
            raise NotImplementedError("sdpa: per-head attention masks do not occur in the reference (the mask is the [n, L] key "
                                      "mask repeated over heads, src/model/model_utils.py:86-87) and are not supported")
        mask = mask[:, 0]
    td = torch_dtype(code)
    # [n, h, L, d] x 3 -> [n, L, 3, h, d] -> [n*L, 3*h*d]
    qkv = torch.stack([t.to(td).permute(0, 2, 1, 3) for t in (Q, K, V)], dim=2).reshape(n * L, 3 * h * d)
    y = (LongSDPAFunction if L > 64 else SDPAFunction).apply(qkv, mask, n, L, h, d, code)
    return y.view(n, L, h, d).permute(0, 2, 1, 3)


# ------------------------------------------------------------------------------------------ pooling
class PoolFunction(Function):
    """K5: AttentionPooling.forward, src/model/model_utils.py:13-31."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, mask, code, needed=None, lazy_dx=False):
        _need_gpu(x, w1, mask)
        n, L, N = x.shape
        q = w1.shape[0]
        x = x.contiguous()
        if x.dtype != torch_dtype(code):
            raise RuntimeError(f"pool input must be {torch_dtype(code)}, got {x.dtype}")
        dev = x.device
        w1_p = pack(w1, code)
        b1_c, w2_c, b2_c = (t.detach().float().contiguous() for t in (b1, w2.reshape(-1), b2))
        mask_c = mask.contiguous().float() if mask is not None else None
        e = torch.empty(n * L, q, dtype=torch_dtype(code), device=dev)
        alpha = torch.empty(n * L, dtype=torch.float32, device=dev)
        out = torch.empty(n, N, dtype=torch.float32, device=dev)
        d = _lib.PoolDesc(n=n, L=L, N=N, q=q, dtype=code, x=ptr(x), mask=ptr(mask_c), w1=ptr(w1_p), ldw1=w1_p.shape[1],
                          b1=ptr(b1_c), w2=ptr(w2_c), b2=ptr(b2_c), seq_needed=ptr(needed))
        check(_lib.lib().nr_additive_pool_fwd(C.byref(d), ptr(e), ptr(alpha), ptr(out), N, _stream()), "nr_additive_pool_fwd")
        ctx.code, ctx.dims = code, (n, L, N, q)
        ctx.needed = needed
        ctx.lazy_dx = bool(lazy_dx)
        # (Function.forward runs with grad mode off: no torch.is_grad_enabled() test here -- it would always say no)
        ctx.targets = tuple(grad_target(p) for p in (w1, b1, w2, b2))
        ctx.save_for_backward(x, mask_c, w1_p, b1_c, w2_c, b2_c, e, alpha, w1)
        return out

    @staticmethod
    def backward(ctx, g):
        seq = _enter_backward()
        x, mask_c, w1_p, b1_c, w2_c, b2_c, e, alpha, w1 = ctx.saved_tensors
        n, L, N, q = ctx.dims
        code, dev = ctx.code, g.device
        g = g.contiguous().float()
        w1_t = pack(w1, code, transpose=True) if ctx.needs_input_grad[0] else None    # [N, q]
        dpre = torch.empty_like(e)
        direct = all(t is not None for t in ctx.targets)
        if direct:
            dw1, db1, dw2, db2 = ctx.targets                      # views of the flat gradient bucket, accumulated in place
        else:
            # one zero fill for the four accumulated gradients (views of a flat buffer; q*N and q are multiples of 4)
            flat = torch.zeros(q * N + 2 * q + 4, dtype=torch.float32, device=dev)
            dw1, db1, dw2, db2 = flat[:q * N].view(q, N), flat[q * N:q * N + q], flat[q * N + q:q * N + 2 * q], flat[q * N + 2 * q:q * N + 2 * q + 1]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        d = _lib.PoolDesc(n=n, L=L, N=N, q=q, dtype=code, x=ptr(x), mask=ptr(mask_c), w1=ptr(w1_p), ldw1=w1_p.shape[1],
                          b1=ptr(b1_c), w2=ptr(w2_c), b2=ptr(b2_c), seq_needed=ptr(ctx.needed), dx_far_unwritten=int(ctx.lazy_dx))
        partial = _ws(_lib.lib().nr_pool_workspace_bytes(C.byref(d)), dev)      # per-workgroup partial rows + slab scratch
        d.partial_bytes = partial.numel() * 4
        check(_lib.lib().nr_additive_pool_bwd(C.byref(d), ptr(e), ptr(alpha), ptr(g), N, ptr(w1_t),
                                              w1_t.shape[1] if w1_t is not None else 0, ptr(dpre), ptr(partial), ptr(dw1),
                                              ptr(db1), ptr(dw2), ptr(db2), ptr(dx), _stream()), "nr_additive_pool_bwd")
        flags_ptr = _lib.lib().nr_pool_seq_flags(C.byref(d), ptr(partial))
        _offer_flags(seq, dx, n, flags_ptr, partial, lazy=ctx.lazy_dx and bool(flags_ptr))
        if direct:
            return dx, None, None, None, None, None, None, None, None
        return dx, dw1, db1, dw2.view(1, q), db2, None, None, None, None


def additive_pool(x, w1, b1, w2, b2, code: int, mask=None, needed=None, lazy_dx=False):
    """needed: optional [n] int32 flags (needed_flags): flag 0 = the pooled vector is not used: zeros, nothing computed.
    lazy_dx: the gradient wrt x may keep UNWRITTEN rows for sequences with a zero pooled gradient that lie far from every
    sequence with one -- only when x is the output of ops.mhsa (gather source) whose `_nr_takes_lazy_dy` is set and nothing
    else consumes x; the MHSA backward then never reads those rows (and raises if the flags did not reach it).
    Scores: the fused title-level forward (bf16, 24 <= L <= 32, 384 < N <= 416, q <= 256, n * L >= 4096, no mask) takes
    exp(s) / (sum + 1e-8) as the model writes it, without subtracting the maximum, so scores beyond the fp32 range of exp
    (s > 88.7; |s| <= |w2|_1 + |b2|) are outside its contract and give NaN there, as they do in the fp32 reference; every
    other shape subtracts the maximum and returns a number (DESIGN.md "Additive pooling: routes as verified and the sweep")."""
    return PoolFunction.apply(x, w1, b1, w2, b2, mask, code, needed, bool(lazy_dx) and x.requires_grad)


# ------------------------------------------------------------------------------------------ pad blend / cast
# Row split whose backward is not a copy.  `torch.split` of the encoder output [candidates ; history] gets its gradient as a
# concatenation of the two consumers' gradients (45 MB written and read again per step at B = 512).  split_rows allocates that
# gradient buffer up front and registers its two halves under the addresses of the two outputs; a libnrhip backward that
# produces the gradient of exactly such a tensor (the pad-doc blend of the history rows, the scorer for the candidates) writes
# into the registered half, and the split's backward recognises the two halves and returns the buffer as it stands.  Anything
# else -- another consumer, an accumulation, a copy in between -- arrives in some other tensor and is concatenated as before.
_grad_out = {}


def _take_grad_out(x):
    if not _grad_out or not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous():
        return None
    return _grad_out.pop((x.data_ptr(), x.numel()), None)


class SplitRowsFunction(Function):
    @staticmethod
    def forward(ctx, x, n_a):
        ctx.n_a, ctx.arena = int(n_a), None
        a, b = x[:n_a], x[n_a:]
        _grad_out.clear()
        if (ctx.needs_input_grad[0] and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
                and 0 < n_a < x.shape[0]):
            ctx.arena = torch.empty_like(x)
            _grad_out[(a.data_ptr(), a.numel())] = ctx.arena[:n_a]
            _grad_out[(b.data_ptr(), b.numel())] = ctx.arena[n_a:]
        return a, b

    @staticmethod
    def backward(ctx, ga, gb):
        arena, n_a = ctx.arena, ctx.n_a
        if (arena is not None and ga is not None and gb is not None and ga.dtype == gb.dtype == torch.float32 and ga.is_contiguous()
                and gb.is_contiguous() and ga.data_ptr() == arena.data_ptr() and gb.data_ptr() == arena[n_a:].data_ptr()
                and ga.numel() == arena[:n_a].numel() and gb.numel() == arena[n_a:].numel()):
            return arena, None
        return torch.cat([ga, gb], dim=0), None


def split_rows(x, n_a: int):
    """x[:n_a], x[n_a:] -- see above."""
    return SplitRowsFunction.apply(x, n_a)


class BlendFunction(Function):
    """K6: x*m + pad_doc*(1-m) (src/model/NRMS.py:59-60, src/model/NAML.py:94-95), emitted in the
    compute dtype.  mask=None is a plain fp32 -> compute-dtype cast with an fp32 gradient."""

    @staticmethod
    def forward(ctx, x, mask, pad, code):
        _need_gpu(x, mask, pad)
        n, L, N = x.shape
        x = x.contiguous().float()
        mask_c = mask.contiguous().float() if mask is not None else None
        pad_c = pad.detach().reshape(-1).float().contiguous() if pad is not None else None
        out = torch.empty(n, L, N, dtype=torch_dtype(code), device=x.device)
        check(_lib.lib().nr_pad_blend_fwd(ptr(x), ptr(mask_c), ptr(pad_c), ptr(out), n, L, N, code, _stream()), "nr_pad_blend_fwd")
        ctx.code, ctx.dims, ctx.pad_shape = code, (n, L, N), (tuple(pad.shape) if pad is not None else None)
        ctx.pad_target = grad_target(pad)
        ctx.dx_out = _take_grad_out(x)                   # split_rows: write dx where the producer's gradient is assembled
        ctx.save_for_backward(mask_c)
        return out

    @staticmethod
    def backward(ctx, dout):
        _enter_backward()
        (mask_c,) = ctx.saved_tensors
        n, L, N = ctx.dims
        dout = dout.contiguous()
        if dout.dtype != torch_dtype(ctx.code):
            dout = dout.to(torch_dtype(ctx.code))
        dx = ctx.dx_out.view(n, L, N) if ctx.dx_out is not None else torch.empty(n, L, N, dtype=torch.float32, device=dout.device)
        direct = ctx.pad_target is not None and mask_c is not None
        dpad = ctx.pad_target if direct else (torch.zeros(N, dtype=torch.float32, device=dout.device) if mask_c is not None else None)
        check(_lib.lib().nr_pad_blend_bwd(ptr(dout), ptr(mask_c), ptr(dx), ptr(dpad), n, L, N, ctx.code, _stream()), "nr_pad_blend_bwd")
        if direct:
            return dx, None, None, None
        return dx, None, (dpad.view(ctx.pad_shape) if dpad is not None and ctx.pad_shape is not None else None), None


def pad_blend(x, mask, pad, code: int):
    return BlendFunction.apply(x, mask, pad, code)


def to_compute(x, code: int):
    """fp32 [n, L, N] -> compute dtype through the blend kernel (no mask)."""
    if x.dtype == torch_dtype(code) and code == NR_F32:
        return x
    return BlendFunction.apply(x, None, None, code)


# ------------------------------------------------------------------------------------------ scorer + CE
class ScoreCEFunction(Function):
    """K8: torch.bmm scorer + nn.CrossEntropyLoss, src/model/NRMS.py:93-94 / src/model/NAML.py:128-129."""

    @staticmethod
    def forward(ctx, cand, user, label):
        _need_gpu(cand, user, label)
        B, Cn, N = cand.shape
        cand, user = cand.contiguous().float(), user.contiguous().float()
        label = label.contiguous().to(torch.int64)
        score = torch.empty(B, Cn, dtype=torch.float32, device=cand.device)
        loss = torch.empty((), dtype=torch.float32, device=cand.device)
        lossvec = torch.empty(B, dtype=torch.float32, device=cand.device)
        check(_lib.lib().nr_score_ce_fwd(ptr(cand), N, ptr(user), ptr(label), ptr(score), ptr(loss), ptr(lossvec), B, Cn, N,
                                         _stream()), "nr_score_ce_fwd")
        ctx.save_for_backward(cand, user, label, score)
        ctx.dcand_out = _take_grad_out(cand)
        ctx.set_materialize_grads(False)                 # an unused `score` output then costs no zero fill in the backward
        return loss, score

    @staticmethod
    def backward(ctx, gloss, gscore):
        _enter_backward()
        cand, user, label, score = ctx.saved_tensors
        B, Cn, N = cand.shape
        gl = gloss.contiguous().float() if gloss is not None else None
        gs = gscore.contiguous().float() if gscore is not None else None
        dcand = ctx.dcand_out.view_as(cand) if ctx.dcand_out is not None else torch.empty_like(cand)
        duser = torch.empty_like(user)
        check(_lib.lib().nr_score_ce_bwd(ptr(cand), N, ptr(user), ptr(label), ptr(score), ptr(gl), ptr(gs), ptr(dcand), N,
                                         ptr(duser), B, Cn, N, _stream()), "nr_score_ce_bwd")
        return dcand, duser, None


def score_ce(cand, user, label):
    if CHECK_INDICES:
        check_labels(label.contiguous().to(torch.int64), cand.shape[1])
    return ScoreCEFunction.apply(cand, user, label)


# ------------------------------------------------------------------------------------------ Conv1d k=3 over gathered titles
class ConvFunction(Function):
    """K4 (+K1, K2): title-embedding row gather -> dropout -> Conv1d(k=3, pad=1), src/model/NAML.py:47-54."""

    @staticmethod
    def forward(ctx, w, b, ids, cfg, table):
        """table: the fp32 [V, T*D] master when it is trainable (an autograd input: its gradient is made by
        nr_conv1d_k3_bwd_table), None for a frozen table -- the forward reads cfg["table_packed"] either way."""
        _need_gpu(w, ids)
        code, T, D = cfg["code"], cfg["T"], cfg["D"]
        table_p = cfg["table_packed"]                 # [V*T, Dp]
        Dp = table_p.shape[1]
        N = w.shape[0]
        n, stride = ids.shape[0], ids.stride(0)
        dev = w.device
        w_p = torch.empty(N, 3 * Dp, dtype=torch_dtype(code), device=dev)
        wc = w.detach().float().contiguous()
        check(_lib.lib().nr_pack_conv_w(ptr(wc), N, D, ptr(w_p), Dp, code, _stream()), "nr_pack_conv_w")
        b_c = b.detach().float().contiguous()
        y = torch.empty(n, T, N, dtype=torch_dtype(code), device=dev)
        # bf16: the token rows (gather + dropout) are stored once, with a zero row between titles: the im2col row of a token is
        # 3 * Dp contiguous elements of that buffer, which feeds the LDS-DMA GEMMs of both passes (no 3x im2col copy)
        x_rows = torch.empty(n * (T + 1) + 1, Dp, dtype=torch.bfloat16, device=dev) if code == _lib.NR_BF16 and n > 0 else None
        d = _lib.ConvDesc(n=n, T=T, D=D, Dp=Dp, N=N, dtype=code, table=ptr(table_p), ids=ids.data_ptr(), ids_stride=stride,
                          p_in=cfg["p_in"], seed_in=cfg["seed_in"], w_pack=ptr(w_p), bias=ptr(b_c), x_rows=ptr(x_rows),
                          ld_rows=Dp, seq_needed=ptr(cfg.get("needed")))
        check(_lib.lib().nr_conv1d_k3_fwd(C.byref(d), ptr(y), _stream()), "nr_conv1d_k3_fwd")
        ctx.cfg, ctx.dims = cfg, (n, T, D, Dp, N, stride)
        ctx.ids = ids                                   # keeps the (possibly strided) id view alive
        ctx.x_rows = x_rows if any(ctx.needs_input_grad[:2]) else None
        ctx.targets = (grad_target(w), grad_target(b))
        ctx.table_grad = table is not None and ctx.needs_input_grad[4]
        if ctx.table_grad:
            ctx.table_shape, ctx.table_target, ctx.w32 = tuple(table.shape), grad_target(table), wc
        ctx.save_for_backward(table_p, w_p, b_c)
        return y

    @staticmethod
    def backward(ctx, dy):
        seq = _enter_backward()
        table_p, w_p, b_c = ctx.saved_tensors
        n, T, D, Dp, N, stride = ctx.dims
        cfg, code, dev = ctx.cfg, ctx.cfg["code"], dy.device
        dy = dy.contiguous()
        if dy.dtype != torch_dtype(code):
            dy = dy.to(torch_dtype(code))
        seq_nz, seq_nz_owner, _lazy = _take_flags(seq, dy, n)
        if _lazy:
            raise RuntimeError("conv1d_k3 backward cannot take a gradient with unwritten rows (additive_pool lazy_dx=True)")
        dwp = torch.zeros(N, 3 * Dp, dtype=torch.float32, device=dev)
        direct = all(t is not None for t in ctx.targets)
        db = ctx.targets[1] if direct else torch.zeros(N, dtype=torch.float32, device=dev)
        d = _lib.ConvDesc(n=n, T=T, D=D, Dp=Dp, N=N, dtype=code, table=ptr(table_p), ids=ctx.ids.data_ptr(), ids_stride=stride,
                          p_in=cfg["p_in"], seed_in=cfg["seed_in"], w_pack=ptr(w_p), bias=ptr(b_c), x_rows=ptr(ctx.x_rows),
                          ld_rows=Dp, seq_nz=seq_nz, seq_needed=ptr(cfg.get("needed")))
        bwd_ws = _ws(_lib.lib().nr_conv_workspace_bytes(C.byref(d)), dev) if ctx.x_rows is not None else None
        d.bwd_ws, d.bwd_ws_bytes = ptr(bwd_ws), (bwd_ws.numel() * 4 if bwd_ws is not None else 0)
        check(_lib.lib().nr_conv1d_k3_bwd(C.byref(d), ptr(dy), ptr(dwp), ptr(db), _stream()), "nr_conv1d_k3_bwd")
        dw = ctx.targets[0] if direct else torch.empty(N, D, 3, dtype=torch.float32, device=dev)
        check(_lib.lib().nr_unpack_conv_dw(ptr(dwp), N, D, Dp, ptr(dw), int(direct), _stream()), "nr_unpack_conv_dw")
        dtable = None
        if ctx.table_grad:
            # trainable title table: dx over the live titles (one more GEMM of the forward's size) and the owner-computes
            # scatter, added straight into the bucket's gradient view when there is one (2.3 GB at 65 000 news: no copy of it)
            V = ctx.table_shape[0]
            dtab = ctx.table_target if ctx.table_target is not None else torch.zeros(ctx.table_shape, dtype=torch.float32, device=dev)
            ldwt = round_up(3 * N, 32 if code == NR_BF16 else chunk(code))
            w_t = torch.empty(D, ldwt, dtype=torch_dtype(code), device=dev)
            check(_lib.lib().nr_pack_conv_w_t(ptr(ctx.w32), N, D, ptr(w_t), ldwt, code, _stream()), "nr_pack_conv_w_t")
            d.table_rows = V
            tws = _ws(_lib.lib().nr_conv_table_workspace_bytes(C.byref(d)), dev)
            if POISON_WORKSPACES:
                tws.fill_(-1)                     # (int32 view: every byte 0xff, a NaN pattern in both operand types)
            check(_lib.lib().nr_conv1d_k3_bwd_table(C.byref(d), ptr(dy), ptr(w_t), ldwt, ptr(dtab), ptr(tws), tws.numel() * 4, _stream()),
                  "nr_conv1d_k3_bwd_table")
            if ctx.table_target is None:
                dtable = dtab
        if direct:
            return None, None, None, None, dtable
        return dw, db, None, None, dtable


def conv1d_k3_gather(table, w, b, ids, T: int, D: int, code: int, p_in=0.0, needed=None):
    """ids: int32 view [n] (any stride) of news ids; table: fp32 [V, T*D], frozen or trainable (a trainable one gets its
    dense [V, T*D] gradient from nr_conv1d_k3_bwd_table; row 0, the padding_idx, gets none).
    needed: optional [n] int32 flags (needed_flags); output rows of unneeded titles may stay unwritten -- pool them with the
    same flags."""
    if CHECK_INDICES:
        check_ids(ids, table.shape[0], "news id")
    # model.NAML.TitleTable holds the packed operand itself (uploaded block by block); a plain fp32 parameter is packed once
    packed = table.packed(code) if hasattr(table, "packed") else table_cache.get(table, code, row_cols=D)
    cfg = dict(code=code, T=T, D=D, p_in=float(p_in), seed_in=draw_seed() if p_in > 0 else 0, table_packed=packed, needed=needed)
    if isinstance(table, torch.Tensor) and table.requires_grad and torch.is_grad_enabled():
        if table.dtype != torch.float32 or not table.is_contiguous() or tuple(table.shape[1:]) != (T * D,):
            raise RuntimeError(f"conv1d_k3_gather: a trainable title table must be contiguous fp32 [V, {T * D}], got "
                               f"{table.dtype} {tuple(table.shape)}")
        return ConvFunction.apply(w, b, ids, cfg, table)
    return ConvFunction.apply(w, b, ids, cfg, None)


# ------------------------------------------------------------------------------------------ gather + Linear (category views)
class GatherLinearFunction(Function):
    """K7: Embedding(padding_idx=0) -> Linear, src/model/NAML.py:19-24,60-68."""

    @staticmethod
    def forward(ctx, emb, w, b, ids, code):
        _need_gpu(emb, w, ids)
        M, stride = ids.shape[0], ids.stride(0)
        N, K = w.shape
        emb_p, w_p = pack(emb, code), pack(w, code)
        b_c = b.detach().float().contiguous()
        out = torch.empty(M, N, dtype=torch.float32, device=w.device)
        d = _lib.LinearDesc(M=M, K=K, N=N, dtype=code, src_kind=NR_SRC_GATHER, x=ptr(emb_p), ldx=emb_p.shape[1],
                            ids=ids.data_ptr(), ids_stride=stride, w=ptr(w_p), ldw=w_p.shape[1], bias=ptr(b_c), w_t=0, ldwt=0)
        check(_lib.lib().nr_linear_fwd(C.byref(d), ptr(out), N, _stream()), "nr_linear_fwd")
        ctx.code, ctx.dims, ctx.ids = code, (M, K, N, stride, tuple(emb.shape)), ids
        ctx.targets = tuple(grad_target(p) for p in (emb, w, b))
        ctx.save_for_backward(emb_p, w_p, b_c, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        _enter_backward()
        emb_p, w_p, b_c, w = ctx.saved_tensors
        M, K, N, stride, emb_shape = ctx.dims
        code, dev = ctx.code, dout.device
        dout = dout.contiguous().float()
        Nc = round_up(N, chunk(code))
        need_t = ctx.needs_input_grad[0]
        direct = ctx.targets[1] is not None and ctx.targets[2] is not None and (ctx.targets[0] is not None or not need_t)
        if direct:
            dtable, dw, db = (ctx.targets[0] if need_t else None), ctx.targets[1], ctx.targets[2]
        else:
            dw = torch.zeros(N, K, dtype=torch.float32, device=dev)
            db = torch.zeros(N, dtype=torch.float32, device=dev)
            dtable = torch.zeros(emb_shape, dtype=torch.float32, device=dev) if need_t else None
        w_t = pack(w, code, transpose=True, ld=Nc) if need_t else None               # [K, Nc]
        d = _lib.LinearDesc(M=M, K=K, N=N, dtype=code, src_kind=NR_SRC_GATHER, x=ptr(emb_p), ldx=emb_p.shape[1],
                            ids=ctx.ids.data_ptr(), ids_stride=stride, w=ptr(w_p), ldw=w_p.shape[1], bias=ptr(b_c),
                            w_t=ptr(w_t), ldwt=Nc if need_t else 0, table_rows=emb_shape[0])
        ws = _ws(_lib.lib().nr_linear_workspace_bytes(C.byref(d)), dev)
        d.dout_ws_bytes = ws.numel() * 4
        check(_lib.lib().nr_linear_bwd(C.byref(d), ptr(dout), N, ptr(ws), ptr(dw), ptr(db), ptr(dtable), _stream()), "nr_linear_bwd")
        if direct:
            return None, None, None, None, None
        return dtable, dw, db, None, None


def gather_linear(emb, w, b, ids, code: int):
    if CHECK_INDICES:
        check_ids(ids, emb.shape[0], "category id")
    return GatherLinearFunction.apply(emb, w, b, ids, code)


# ------------------------------------------------------------------------------------------ plain row gather (eval path)
def embed_gather(table: torch.Tensor, ids: torch.Tensor, code: int = NR_F32) -> torch.Tensor:
    """out[i] = table[ids[i]], no gradient: the eval-time news-vector lookup of src/dataset.py:68,72.  `code`: dtype of the
    result (fp32, or bf16 = gather + the cast the user encoder would do next, in one pass)."""
    _need_gpu(table, ids)
    table = table.detach().float().contiguous()
    ids = ids.to(torch.int32).contiguous()
    if CHECK_INDICES:
        check_ids(ids, table.shape[0], "news index")
    cols = table.shape[1]
    out = torch.empty(*ids.shape, cols, dtype=torch_dtype(code), device=table.device)
    check(_lib.lib().nr_gather_cast_fwd(ptr(table), cols, ptr(ids), ids.numel(), cols, ptr(out), cols, code, _stream()),
          "nr_gather_cast_fwd")
    return out


def score_eval(news_vecs, cand_ids, imp_of, user_vecs) -> torch.Tensor:
    """score[i] = <news_vecs[cand_ids[i]], user_vecs[imp_of[i]]> — the per-impression np.dot of src/main.py:253."""
    _need_gpu(news_vecs, cand_ids, imp_of, user_vecs)
    news_vecs, user_vecs = news_vecs.detach().float().contiguous(), user_vecs.detach().float().contiguous()
    cand_ids, imp_of = cand_ids.to(torch.int32).contiguous(), imp_of.to(torch.int32).contiguous()
    if CHECK_INDICES:
        check_ids(cand_ids, news_vecs.shape[0], "candidate index")
        check_ids(imp_of, user_vecs.shape[0], "impression index")
    N = news_vecs.shape[1]
    out = torch.empty(cand_ids.numel(), dtype=torch.float32, device=news_vecs.device)
    check(_lib.lib().nr_score_eval(ptr(news_vecs), N, ptr(cand_ids), ptr(imp_of), ptr(user_vecs), N, ptr(out),
                                   cand_ids.numel(), N, _stream()), "nr_score_eval")
    return out


def _pool_args(what, V, U, dev, prior, stamp, window):
    """The optional pool inputs of score_topk / score_rank as the tensors the descriptor points at: prior fp32 [V], stamp int32
    [V], window int32 [U, 2], contiguous, on `dev`; None stays None.  stamp and window come together (the library refuses one
    without the other; so does this check, before anything is converted)."""
    if (stamp is None) != (window is None):
        raise RuntimeError(f"{what}: stamp and window come together (got {'stamp' if window is None else 'window'} alone)")
    for name, t, shape, floating in (("prior", prior, (V,), True), ("stamp", stamp, (V,), False), ("window", window, (U, 2), False)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise RuntimeError(f"{what}: {name} must be a tensor of shape {shape}, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
        if t.device != dev:
            raise RuntimeError(f"{what}: {name} is on {t.device}, the news vectors on {dev}")
        if t.is_floating_point() != floating or t.is_complex() or t.dtype == torch.bool:
            raise RuntimeError(f"{what}: {name} must be {'floating point' if floating else 'an integer tensor'}, got {t.dtype}")
    p = None if prior is None else prior.detach().to(torch.float32).contiguous()
    s = None if stamp is None else stamp.detach().to(torch.int32).contiguous()
    w = None if window is None else window.detach().to(torch.int32).contiguous()
    return p, s, w


class ExclusionLists:
    """Per-user exclusion lists of any length in the CSR form nr_score_topk / nr_score_rank take (include/nrhip.h, K9):
    `offsets` int32 [U + 1] and `ids` int32 [nnz], user u's list = ids[offsets[u] : offsets[u + 1]], in canonical form -- per user
    sorted, unique, only ids >= 1.  Build it once per batch of users and hand it to as many score_topk / score_rank calls as
    needed (`exclude=`); it lives on the device of what it was built from (or `device=`), and works on the CPU as well.
      ExclusionLists(t)                  t: integer tensor [U, E] of any width E; 0 or negative = no entry
      ExclusionLists([a_0, ..., a_U-1])  a sequence of U one-dimensional id arrays (tensors, numpy arrays, lists), any lengths
      ExclusionLists.from_sorted(offsets, ids)   trusts the caller: nothing is sorted, checked or cleaned (the raw contract)
    Duplicates, zeros, negatives and any order are fine in the first two; ids >= V are kept and mean nothing to the kernels.
    Canonicalisation is torch index arithmetic: one sort of the keys u * 2^31 + id, unique_consecutive, bincount -> offsets.
    More than 2^31 - 1 entries, or an id above 2^31 - 1, is refused."""

    _ID_BITS = 31

    def __init__(self, lists, device=None):
        if isinstance(lists, torch.Tensor):
            if lists.dim() != 2 or lists.is_floating_point() or lists.is_complex() or lists.dtype == torch.bool:
                raise RuntimeError(f"ExclusionLists: a tensor must be an integer [U, E], got {tuple(lists.shape)} {lists.dtype}")
            t = lists.detach()
            if device is not None:
                t = t.to(device)
            U = t.shape[0]
            users = torch.arange(U, device=t.device, dtype=torch.int64)[:, None].expand(U, t.shape[1]).reshape(-1)
            flat = t.reshape(-1).to(torch.int64)
        else:
            rows = [torch.as_tensor(r).reshape(-1) for r in lists]
            for r in rows:
                if r.numel() and (r.is_floating_point() or r.is_complex() or r.dtype == torch.bool):
                    raise RuntimeError(f"ExclusionLists: id arrays must be integers, got {r.dtype}")
            U = len(rows)
            dev = torch.device(device) if device is not None else (rows[0].device if rows else torch.device("cpu"))
            lens = torch.tensor([r.numel() for r in rows], dtype=torch.int64)
            flat = torch.cat([r.to(torch.int64) for r in rows]).to(dev) if rows else torch.zeros(0, dtype=torch.int64, device=dev)
            users = torch.repeat_interleave(torch.arange(U, dtype=torch.int64), lens).to(dev)
        self.offsets, self.ids = self._canonical(users, flat, U)

    @classmethod
    def _canonical(cls, users, flat, U):
        """offsets, ids of the (user, id) pairs: ids >= 1 only, per user sorted and unique."""
        keep = flat >= 1
        users, flat = users[keep], flat[keep]
        if flat.numel() and int(flat.max()) >= (1 << cls._ID_BITS):
            raise RuntimeError(f"ExclusionLists: news id {int(flat.max())} does not fit int32")
        keys = torch.unique_consecutive(torch.sort((users << cls._ID_BITS) + flat).values)
        if keys.numel() > (1 << 31) - 1:
            raise RuntimeError(f"ExclusionLists: {keys.numel()} entries, at most 2^31 - 1")
        counts = torch.bincount(keys >> cls._ID_BITS, minlength=U)
        offsets = torch.zeros(U + 1, dtype=torch.int64, device=keys.device)
        offsets[1:] = torch.cumsum(counts, 0)
        return offsets.to(torch.int32), (keys & ((1 << cls._ID_BITS) - 1)).to(torch.int32)

    @classmethod
    def from_sorted(cls, offsets, ids):
        """The arrays as they are (converted to contiguous int32 only): per user strictly ascending is the CALLER'S promise."""
        offsets, ids = torch.as_tensor(offsets), torch.as_tensor(ids)
        if offsets.dim() != 1 or offsets.numel() < 1 or ids.dim() != 1 or offsets.device != ids.device:
            raise RuntimeError(f"ExclusionLists.from_sorted: offsets [U + 1] and ids [nnz] on one device, got {tuple(offsets.shape)} on "
                               f"{offsets.device} and {tuple(ids.shape)} on {ids.device}")
        if ids.numel() > (1 << 31) - 1:
            raise RuntimeError(f"ExclusionLists: {ids.numel()} entries, at most 2^31 - 1")
        self = cls.__new__(cls)
        self.offsets, self.ids = offsets.detach().to(torch.int32).contiguous(), ids.detach().to(torch.int32).contiguous()
        return self

    @property
    def U(self) -> int:
        return self.offsets.numel() - 1

    @property
    def device(self):
        return self.ids.device

    def __len__(self) -> int:
        return self.U

    def to(self, device):
        """The same lists on `device` (self if they are there already)."""
        if torch.device(device) == self.device:
            return self
        return ExclusionLists.from_sorted(self.offsets.to(device), self.ids.to(device))

    def _pairs(self):
        """(user, id) of every entry, int64."""
        counts = (self.offsets[1:] - self.offsets[:-1]).to(torch.int64)
        return torch.repeat_interleave(torch.arange(self.U, device=self.device, dtype=torch.int64), counts), self.ids.to(torch.int64)

    def take(self, rows):
        """The lists of users rows[i], i = 0 .. len(rows) - 1 (repeats and any order allowed), as a new object."""
        rows = torch.as_tensor(rows).to(device=self.device, dtype=torch.int64).reshape(-1)
        off = self.offsets.to(torch.int64)
        counts = (off[1:] - off[:-1])[rows]
        new_off = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=self.device)
        new_off[1:] = torch.cumsum(counts, 0)
        if int(new_off[-1]) > (1 << 31) - 1:
            raise RuntimeError(f"ExclusionLists: {int(new_off[-1])} entries, at most 2^31 - 1")
        src = torch.arange(int(new_off[-1]), device=self.device) + torch.repeat_interleave(off[:-1][rows] - new_off[:-1], counts)
        return ExclusionLists.from_sorted(new_off, self.ids[src])

    def by_news(self, V):
        """The transposed lists nr_score_expect_news takes (include/nrhip.h, K18): (offsets int32 [V + 1], users int32 [nnz]), for
        news v the ascending 0-based indices of the users that list it = users[offsets[v] : offsets[v + 1]].  Ids >= V are
        dropped (they mean nothing to the kernels).  Torch index arithmetic on the device of the lists: one sort of the keys
        id * 2^31 + user, bincount -> offsets.  The last result is kept with the object (the lists are not meant to be edited in
        place), so the calls of one batch of users transpose once."""
        V = int(V)
        kept = getattr(self, "_by_news", None)
        if kept is not None and kept[0] == V and kept[1] is self.offsets and kept[2] is self.ids:
            return kept[3]
        users, ids = self._pairs()
        keep = ids < V
        keys = torch.sort((ids[keep] << self._ID_BITS) + users[keep]).values
        offsets = torch.zeros(V + 1, dtype=torch.int64, device=self.device)
        offsets[1:] = torch.cumsum(torch.bincount(keys >> self._ID_BITS, minlength=V), 0)
        out = offsets.to(torch.int32), (keys & ((1 << self._ID_BITS) - 1)).to(torch.int32)
        self._by_news = (V, self.offsets, self.ids, out)
        return out

    def merged(self, other):
        """The per-user union with `other` (an ExclusionLists of the same U, or anything the constructor takes)."""
        if not isinstance(other, ExclusionLists):
            other = ExclusionLists(other, device=self.device)
        if other.U != self.U:
            raise RuntimeError(f"ExclusionLists.merged: {self.U} users against {other.U}")
        (ua, ia), (ub, ib) = self._pairs(), other._pairs()
        out = ExclusionLists.__new__(ExclusionLists)
        out.offsets, out.ids = self._canonical(torch.cat([ua, ub.to(self.device)]), torch.cat([ia, ib.to(self.device)]), self.U)
        return out


def _exclude_args(what, exclude, U, dev, dense=True):
    """`exclude` of score_topk / score_rank as descriptor fields: the dense list (a tensor [U, E <= 64]: exclude, ld_exclude, E, as
    always) or the CSR lists (a wider tensor or an ExclusionLists: excl_offsets, excl_ids, n_excl).  dense=False (score_logz, whose
    descriptor has the CSR fields only): a tensor of any width becomes CSR lists.  Returns (fields, keepalive)."""
    none = {"exclude": None, "ld_exclude": 0, "E": 0} if dense else {}
    if exclude is None:
        return none, None
    if isinstance(exclude, torch.Tensor):
        if exclude.dim() != 2 or exclude.shape[0] != U:
            raise RuntimeError(f"{what}: exclude must be [U = {U}, E], got {tuple(exclude.shape)}")
        E = exclude.shape[1]
        if dense and E <= _lib.NR_TOPK_MAX_EXCLUDE:
            ex = exclude.detach().to(torch.int32).contiguous() if E else None
            return {"exclude": ptr(ex), "ld_exclude": E, "E": E}, ex
        exclude = ExclusionLists(exclude)
    if not isinstance(exclude, ExclusionLists):
        raise RuntimeError(f"{what}: exclude must be a tensor [U, E] or an ExclusionLists, got {type(exclude)}")
    if exclude.U != U or exclude.device != dev:
        raise RuntimeError(f"{what}: the exclusion lists are for {exclude.U} users on {exclude.device}, the call has {U} on {dev}")
    n = exclude.ids.numel()
    return dict(none, excl_offsets=ptr(exclude.offsets), excl_ids=ptr(exclude.ids) if n else None, n_excl=n), exclude


def _group_args(what, group, V, dev):
    """`group` of a capped call as the tensor the descriptor points at: int32 [V] on `dev`, contiguous; None stays None."""
    if group is None:
        return None
    if not isinstance(group, torch.Tensor) or tuple(group.shape) != (V,) or group.dtype != torch.int32 or group.device != dev:
        raise RuntimeError(f"{what}: group must be an int32 tensor of shape ({V},) on {dev}, got "
                           f"{(tuple(group.shape), group.dtype, group.device) if isinstance(group, torch.Tensor) else type(group)}")
    return group.detach().contiguous()


@torch.no_grad()
def score_topk(news_vecs, user_vecs, k, exclude=None, splits=0, prior=None, stamp=None, window=None, group=None, group_cap=None):
    """Full-corpus recommendation (nr_score_topk): for every user the k best news of the whole table under the order (score
    descending, news id ascending), score[u, v] = <news_vecs[v], user_vecs[u]> in exact fp32.  Row 0 of `news_vecs` (the
    padding news) is never returned; `exclude` ([U, E <= 64] news ids per user, 0 = no entry) neither.  No [U, V] score matrix
    is formed.  A wider `exclude` tensor or an ExclusionLists (lists of any length, "everything this user was shown") goes
    through the CSR lists of the library (include/nrhip.h, K9) -- same rows, same bits, as long as E <= 64 could hold them; a
    tensor of at most 64 columns takes the dense path exactly as it always did.  Returns (ids int32 [U, k], scores fp32 [U, k]); a row with fewer than k eligible news ends in id 0, score -inf.
    `splits`: 0 = the library chooses the number of corpus slices; tests force it.
    Pools (include/nrhip.h, K9): `prior` [V] floating point -- the score becomes fl32(dot + prior[v]), one fp32 add after the
    dot product, and the returned scores are these sums; -inf in it takes a news out for every user.  `stamp` [V] and `window`
    [U, 2] integers, together -- user u is only given news with window[u, 0] <= stamp[v] <= window[u, 1] (lo > hi: an all-fill
    row).  Without them the call is the plain one, bit for bit.
    Group caps (include/nrhip.h, K9): `group` [V] int32 on the device, one group id per news (a category, say; negative = in no
    group, never capped) with `group_cap` = c in [1, 128] -- the row is the walk down the same order that skips a news once c
    news of its group are taken, so at most c per group and still k entries where k can be taken (otherwise the usual fill).
    One without the other is refused by the library.  Without them the call launches the kernels it always launched.
    score_rank_capped takes the same two arguments and gives the place in this capped row."""
    d, ids, scores, keep = _topk_desc("score_topk", news_vecs, user_vecs, k, exclude, splits, prior, stamp, window, group, group_cap)
    if d is None:
        return ids, scores
    ws = _ws(_lib.lib().nr_score_topk_workspace_bytes(C.byref(d)), ids.device)      # 0 for a bad descriptor: the call below says why
    d.ws, d.ws_bytes = ptr(ws) if ws.numel() else None, ws.numel() * 4
    check(_lib.lib().nr_score_topk(C.byref(d), _stream()), "nr_score_topk")
    return ids, scores


def _topk_desc(what, news_vecs, user_vecs, k, exclude, splits, prior, stamp, window, group, group_cap):
    """The nr_topk_desc of score_topk / score_sample without its workspace, after the checks the two share.  Returns (descriptor,
    ids, scores, keepalive); the descriptor is None for U == 0 (nothing to launch)."""
    _need_gpu(news_vecs, user_vecs, exclude.ids if isinstance(exclude, ExclusionLists) else exclude, prior, stamp, window, group)
    V, N, U, dev = _vector_args(what, news_vecs, user_vecs)
    ids = torch.empty(U, int(k), dtype=torch.int32, device=dev)
    scores = torch.empty(U, int(k), dtype=torch.float32, device=dev)
    if U == 0:
        return None, ids, scores, None
    ex_fields, ex_keep = _exclude_args(what, exclude, U, dev)
    pr, st, win = _pool_args(what, V, U, dev, prior, stamp, window)
    gr = _group_args(what, group, V, dev)
    d = _lib.TopkDesc(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, user=ptr(user_vecs),
                      ld_user=user_vecs.stride(0) if U > 1 else N, U=U, N=N, k=int(k), **ex_fields,
                      splits=int(splits), out_ids=ptr(ids), out_scores=ptr(scores), prior=ptr(pr), stamp=ptr(st), window=ptr(win),
                      ld_window=2 if win is not None else 0, group=ptr(gr), group_cap=0 if group_cap is None else int(group_cap))
    return d, ids, scores, (ex_keep, pr, st, win, gr)


@torch.no_grad()
def score_sample(news_vecs, user_vecs, k, temperature, seed, draw=0, user_keys=None, exclude=None, splits=0, prior=None, stamp=None, window=None,
                 group=None, group_cap=None):
    """Sampled full-corpus recommendation (nr_score_sample; include/nrhip.h, K12): for every user k news drawn WITHOUT
    replacement, each draw proportional to exp(score / temperature) over what is left (the Plackett-Luce model), by the
    Gumbel-max trick fused into score_topk's selection: temperature * g is added to every score, g a standard Gumbel variate
    per (user, news) made in registers from (seed, draw, user key, news id), and the k largest are taken.  No [U, V] matrix of
    scores or of noise is formed.  Everything else -- `exclude`, `splits`, the pools, the caps -- is score_topk's; with caps
    the row is sequential sampling from the softmax over what may still be taken.
    `temperature`: a float (finite, >= 0) or a floating point tensor [U], one per user; 0 gives score_topk's row, bit for bit;
    a tensor entry that is negative, NaN or infinite gives that user an all-fill row.
    `seed` (64 bits) and `draw` (32 bits) name the draw; `user_keys` (integer tensor [U], taken as uint32; None = 0 .. U-1) name
    the users: the row of a user depends on its key, never on its place in the batch, on `splits` or on the rank it is served
    from, so a caller who shards users passes global user numbers here.
    Returns (ids int32 [U, k], perturbed fp32 [U, k] -- the values the row is ordered by, descending --, model_scores fp32
    [U, k] -- fl32(perturbed - fl32(temperature * g)): the score (+ prior) of the news taken, to within two roundings); a row
    with fewer than k eligible news ends in id 0, -inf, -inf."""
    tau_t = temperature if isinstance(temperature, torch.Tensor) else None
    _need_gpu(tau_t, user_keys)
    d, ids, perturbed, keep = _topk_desc("score_sample", news_vecs, user_vecs, k, exclude, splits, prior, stamp, window, group, group_cap)
    model = torch.empty_like(perturbed)
    if d is None:
        return ids, perturbed, model
    U, dev = ids.shape[0], ids.device
    tau, tau_u = _tau_args("score_sample", temperature, U, dev)
    keys = None
    if user_keys is not None:
        if (not isinstance(user_keys, torch.Tensor) or tuple(user_keys.shape) != (U,) or user_keys.is_floating_point() or user_keys.is_complex()
                or user_keys.dtype == torch.bool or user_keys.device != dev):
            raise RuntimeError(f"score_sample: user_keys must be an integer tensor of shape ({U},) on {dev}, got "
                               f"{(tuple(user_keys.shape), user_keys.dtype, user_keys.device) if isinstance(user_keys, torch.Tensor) else type(user_keys)}")
        keys = user_keys.detach().to(torch.int32).contiguous()
    sd = _lib.SampleDesc(topk=d, seed=int(seed) & 0xFFFFFFFFFFFFFFFF, draw=int(draw) & 0xFFFFFFFF, tau=tau, tau_u=ptr(tau_u), user_keys=ptr(keys), out_model=ptr(model))
    ws = _ws(_lib.lib().nr_score_sample_workspace_bytes(C.byref(sd)), dev)     # 0 for a bad descriptor: the call below says why
    sd.topk.ws, sd.topk.ws_bytes = ptr(ws) if ws.numel() else None, ws.numel() * 4
    check(_lib.lib().nr_score_sample(C.byref(sd), _stream()), "nr_score_sample")
    return ids, perturbed, model


@torch.no_grad()
def sample_noise(seed, draw, user_keys, news_ids):
    """The noise of score_sample for pairs (user_keys[i], news_ids[i]) (nr_sample_noise, the probe of include/nrhip.h K12): two
    integer tensors of one shape on the GPU.  Returns (g fp32, bits int64 holding the 32-bit Philox word), of that shape; g is
    the standard Gumbel variate the selection adds temperature times of -- the same device function."""
    _need_gpu(user_keys, news_ids)
    if user_keys.shape != news_ids.shape or user_keys.device != news_ids.device or user_keys.is_floating_point() or news_ids.is_floating_point():
        raise RuntimeError(f"sample_noise: user_keys and news_ids must be integer tensors of one shape on one device, got "
                           f"{tuple(user_keys.shape)} {user_keys.dtype} and {tuple(news_ids.shape)} {news_ids.dtype}")
    a = user_keys.detach().to(torch.int32).contiguous()
    v = news_ids.detach().to(torch.int32).contiguous()
    g = torch.empty(a.shape, dtype=torch.float32, device=a.device)
    bits = torch.empty(a.shape, dtype=torch.int32, device=a.device)
    check(_lib.lib().nr_sample_noise(int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFF, ptr(a), ptr(v), a.numel(), ptr(g), ptr(bits), _stream()),
          "nr_sample_noise")
    return g, bits.to(torch.int64) & 0xFFFFFFFF


def _vector_args(what, news_vecs, user_vecs):
    """The shape checks of the news and user vectors of every full-corpus call; returns (V, N, U, device)."""
    for name, t in (("news_vecs", news_vecs), ("user_vecs", user_vecs)):
        if t.dim() != 2 or t.dtype != torch.float32 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
            raise RuntimeError(f"{what}: {name} must be a 2-D fp32 tensor with contiguous rows, got {tuple(t.shape)} {t.dtype} "
                               f"strides {tuple(t.stride())}")
    V, N = news_vecs.shape
    U = user_vecs.shape[0]
    if user_vecs.shape[1] != N:
        raise RuntimeError(f"{what}: vector widths differ ({N} vs {user_vecs.shape[1]})")
    return V, N, U, news_vecs.device


def _tau_args(what, temperature, U, dev):
    """`temperature` as (scalar, [U] fp32 tensor or None) of a descriptor."""
    if not isinstance(temperature, torch.Tensor):
        return float(temperature), None
    if tuple(temperature.shape) != (U,) or not temperature.is_floating_point() or temperature.device != dev:
        raise RuntimeError(f"{what}: a temperature tensor must be floating point of shape ({U},) on {dev}, got {tuple(temperature.shape)} "
                           f"{temperature.dtype} on {temperature.device}")
    return 0.0, temperature.detach().to(torch.float32).contiguous()


@torch.no_grad()
def score_logz(news_vecs, user_vecs, temperature, exclude=None, splits=0, prior=None, stamp=None, window=None):
    """Full-corpus log-partition (nr_score_logz; include/nrhip.h, K13): per user log sum_v exp(score(u, v) / temperature) over
    exactly the news score_topk / score_sample call eligible -- same score bits fl32(dot + prior), same pools, same lists --
    without the [U, V] score matrix.  Returns (logsum fp32 [U], smax fp32 [U], count int32 [U]): smax is the largest eligible
    score (score_topk's k = 1 score, bit for bit; -inf when nothing is eligible), count the number of eligible news, and
    logsum = log sum_v exp((score - smax) / temperature) >= 0, so that log Z = smax / temperature + logsum and
    log p(v) = (score_v - smax) / temperature - logsum.  Nothing eligible: (-inf, -inf, 0).
    `temperature`: a float (finite, > 0) or a floating point tensor [U]; a tensor entry that is <= 0, NaN or infinite gives that
    user logsum = NaN and leaves its smax and count, and everybody else, as they are.
    `exclude`: None, an ExclusionLists, or an integer tensor [U, E] of any width (converted to an ExclusionLists: this call
    knows the CSR lists only).  The listed news are left out inside the stream, not subtracted afterwards.
    `splits`: 0 = the library chooses the number of corpus slices; the three results do not depend on it, bit for bit, nor on
    which users share the call."""
    tau_t = temperature if isinstance(temperature, torch.Tensor) else None
    _need_gpu(news_vecs, user_vecs, exclude.ids if isinstance(exclude, ExclusionLists) else exclude, prior, stamp, window, tau_t)
    V, N, U, dev = _vector_args("score_logz", news_vecs, user_vecs)
    logsum = torch.empty(U, dtype=torch.float32, device=dev)
    smax = torch.empty(U, dtype=torch.float32, device=dev)
    count = torch.empty(U, dtype=torch.int32, device=dev)
    if U == 0:
        return logsum, smax, count
    ex_fields, ex_keep = _exclude_args("score_logz", exclude, U, dev, dense=False)
    pr, st, win = _pool_args("score_logz", V, U, dev, prior, stamp, window)
    tau, tau_u = _tau_args("score_logz", temperature, U, dev)
    d = _lib.LogzDesc(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, user=ptr(user_vecs),
                      ld_user=user_vecs.stride(0) if U > 1 else N, U=U, N=N, splits=int(splits), **ex_fields, tau=tau, tau_u=ptr(tau_u), out_logsum=ptr(logsum), out_max=ptr(smax), out_count=ptr(count),
                      prior=ptr(pr), stamp=ptr(st), window=ptr(win), ld_window=2 if win is not None else 0)
    ws = _ws(_lib.lib().nr_score_logz_workspace_bytes(C.byref(d)), dev)      # 0 for a bad descriptor: the call below says why
    d.ws, d.ws_bytes = ptr(ws) if ws.numel() else None, ws.numel() * 4
    check(_lib.lib().nr_score_logz(C.byref(d), _stream()), "nr_score_logz")
    return logsum, smax, count


def _base_args(what, base, U, dev):
    """(logsum, smax) of a score_logz result as contiguous fp32 [U] tensors."""
    bl, bm = base[0], base[1]
    for name, t in (("base logsum", bl), ("base smax", bm)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (U,) or not t.is_floating_point() or t.device != dev:
            raise RuntimeError(f"{what}: {name} must be a floating point tensor of shape ({U},) on {dev}")
    return bl.detach().to(torch.float32).contiguous(), bm.detach().to(torch.float32).contiguous()


@torch.no_grad()
def row_logprob(news_vecs, user_vecs, row_ids, temperature, base, sequential, prior=None, stamp=None, window=None):
    """Log-probabilities of the entries of named rows (nr_row_logprob; include/nrhip.h, K14).  `row_ids`: integer tensor
    [U, k <= 128], 0 (or anything outside [1, V)) = fill.  `base` = (logsum, smax) -- the first two results of score_logz for
    these users, pools and temperatures (a third element, the count, is ignored).
    sequential=True: the row as a draw without replacement (Plackett-Luce, the law of score_sample): entry j against the base
    and the entries j .. k-1.  The base must then have been computed WITHOUT the row's ids (merge them into `exclude` of
    score_logz).  sequential=False: every entry on its own against the base, which must then cover everything eligible, the
    entries included: the full-softmax log-probability of a held-out click.
    Returns (logp fp32 [U, k], total fp32 [U] = the row's sum, formed in fp64): fill entries give 0; an entry outside the pool
    or with a NaN score gives NaN; a bad entry of a temperature tensor gives its user's real entries NaN.  Whether an entry is
    in the user's exclusion lists, and repeats within a row, are the caller's statement and are not checked."""
    tau_t = temperature if isinstance(temperature, torch.Tensor) else None
    _need_gpu(news_vecs, user_vecs, row_ids, prior, stamp, window, tau_t, base[0], base[1])
    V, N, U, dev = _vector_args("row_logprob", news_vecs, user_vecs)
    if row_ids.dim() != 2 or row_ids.shape[0] != U or row_ids.is_floating_point() or row_ids.device != dev:
        raise RuntimeError(f"row_logprob: row_ids must be an integer tensor [U = {U}, k] on {dev}, got {tuple(row_ids.shape)} {row_ids.dtype} "
                           f"on {row_ids.device}")
    k = row_ids.shape[1]
    logp = torch.empty(U, k, dtype=torch.float32, device=dev)
    total = torch.empty(U, dtype=torch.float32, device=dev)
    if U == 0:
        return logp, total
    bl, bm = _base_args("row_logprob", base, U, dev)
    ids = row_ids.detach().to(torch.int32).contiguous()
    pr, st, win = _pool_args("row_logprob", V, U, dev, prior, stamp, window)
    tau, tau_u = _tau_args("row_logprob", temperature, U, dev)
    d = _lib.LogprobDesc(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, user=ptr(user_vecs),
                         ld_user=user_vecs.stride(0) if U > 1 else N, U=U, N=N, k=k, row_ids=ptr(ids), ld_ids=k,
                         sequential=1 if sequential else 0, tau=tau, tau_u=ptr(tau_u), base_max=ptr(bm), base_logsum=ptr(bl),
                         out_logp=ptr(logp), out_total=ptr(total), prior=ptr(pr), stamp=ptr(st), window=ptr(win),
                         ld_window=2 if win is not None else 0)
    check(_lib.lib().nr_row_logprob(C.byref(d), _stream()), "nr_row_logprob")
    return logp, total


def _score_expect(what, news_vecs, user_vecs, temperature, base, exclude, splits, prior, stamp, window, weight, sub_ids, sub_w, scale_inv_tau):
    """One nr_score_expect call (include/nrhip.h, K17): (out [U, N] fp32, mass [U] fp32)."""
    tau_t = temperature if isinstance(temperature, torch.Tensor) else None
    _need_gpu(news_vecs, user_vecs, exclude.ids if isinstance(exclude, ExclusionLists) else exclude, prior, stamp, window, tau_t, base[0], base[1],
              weight, sub_ids, sub_w)
    V, N, U, dev = _vector_args(what, news_vecs, user_vecs)
    out = torch.empty(U, N, dtype=torch.float32, device=dev)
    mass = torch.empty(U, dtype=torch.float32, device=dev)
    if U == 0:
        return out, mass
    bl, bm = _base_args(what, base, U, dev)
    if weight is not None:
        if tuple(weight.shape) != (U,) or not weight.is_floating_point() or weight.device != dev:
            raise RuntimeError(f"{what}: weight must be a floating point tensor of shape ({U},) on {dev}")
        weight = weight.detach().to(torch.float32).contiguous()
    T = 0
    if sub_ids is not None:
        if sub_ids.dim() != 2 or sub_ids.shape[0] != U or sub_ids.is_floating_point() or tuple(sub_w.shape) != tuple(sub_ids.shape):
            raise RuntimeError(f"{what}: the named rows must be integer ids [U = {U}, T] with weights of the same shape")
        T = sub_ids.shape[1]
        sub_ids = sub_ids.detach().to(torch.int32).contiguous()
        sub_w = sub_w.detach().to(torch.float32).contiguous()
    ex_fields, ex_keep = _exclude_args(what, exclude, U, dev, dense=False)
    pr, st, win = _pool_args(what, V, U, dev, prior, stamp, window)
    tau, tau_u = _tau_args(what, temperature, U, dev)
    d = _lib.ExpectDesc(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, user=ptr(user_vecs),
                        ld_user=user_vecs.stride(0) if U > 1 else N, U=U, N=N, splits=int(splits), **ex_fields, tau=tau, tau_u=ptr(tau_u),
                        base_max=ptr(bm), base_logsum=ptr(bl), weight=ptr(weight), sub_ids=ptr(sub_ids), sub_w=ptr(sub_w), ld_sub=T, T=T,
                        scale_inv_tau=1 if scale_inv_tau else 0, out=ptr(out), ld_out=N, out_mass=ptr(mass),
                        prior=ptr(pr), stamp=ptr(st), window=ptr(win), ld_window=2 if win is not None else 0)
    ws = _ws(_lib.lib().nr_score_expect_workspace_bytes(C.byref(d)), dev)    # 0 for a bad descriptor: the call below says why
    d.ws, d.ws_bytes = ptr(ws) if ws.numel() else None, ws.numel() * 4
    check(_lib.lib().nr_score_expect(C.byref(d), _stream()), "nr_score_expect")
    return out, mass


@torch.no_grad()
def score_expect(news_vecs, user_vecs, temperature, base, exclude=None, splits=0, prior=None, stamp=None, window=None, weight=None):
    """The expected news vector under the full softmax (nr_score_expect; include/nrhip.h, K17): per user
    E = sum_v p(v) news_vecs[v], p(v) = exp((score_v - smax) / temperature - logsum), over exactly the news score_logz sums over
    -- the gradient of temperature * log Z with respect to the user vector -- without the [U, V] probability matrix.
    `base` = (logsum, smax[, count]): what score_logz returned for the SAME vectors, temperature, exclude and pools.
    `weight`: optional floating point [U], a scale per row.  The other arguments are score_logz's.
    Returns (expect fp32 [U, N], mass fp32 [U]): mass = sum_v p(v), 1 up to rounding when the base matches the arguments.  A user
    with nothing eligible gets zeros and mass 0; a bad entry of a temperature tensor, or a NaN base, gives that user NaN.
    `splits`: 0 = the library chooses the number of corpus slices by U.  For a fixed splits > 0 a user's row does not depend, bit
    for bit, on the other users of the call; across different splits rows agree to within the bound of DESIGN.md section 5."""
    return _score_expect("score_expect", news_vecs, user_vecs, temperature, base, exclude, splits, prior, stamp, window, weight, None, None, False)


class FullSoftmaxNLLFunction(Function):
    """nll [U, T] of named targets under the full softmax over the corpus, differentiable with respect to the user vectors."""

    @staticmethod
    def forward(ctx, user_vecs, news_vecs, targets, temperature, exclude, splits, prior, stamp, window):
        user = user_vecs.detach()
        U, dev = user.shape[0], user.device
        base = score_logz(news_vecs, user, temperature, exclude=exclude, splits=splits, prior=prior, stamp=stamp, window=window)
        logp, _ = row_logprob(news_vecs, user, targets, temperature, base, False, prior=prior, stamp=stamp, window=window)
        V = news_vecs.shape[0]
        valid = (targets >= 1) & (targets < V) & ~torch.isnan(logp)
        if isinstance(temperature, torch.Tensor):
            valid &= ((temperature > 0) & torch.isfinite(temperature))[:, None]
        nll = torch.where(valid, -logp, torch.zeros_like(logp))
        ctx.save_for_backward(user, news_vecs, targets, valid, base[0], base[1])
        ctx.rest = (temperature, exclude, splits, prior, stamp, window)
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)
        return nll, valid

    @staticmethod
    def backward(ctx, g, _gvalid):
        user, news_vecs, targets, valid, bl, bm = ctx.saved_tensors
        temperature, exclude, splits, prior, stamp, window = ctx.rest
        if g is None:
            return (None,) * 9
        gw = torch.where(valid, g.to(torch.float32), torch.zeros((), dtype=torch.float32, device=g.device))
        with torch.no_grad():
            grad, _ = _score_expect("full_softmax_nll", news_vecs, user, temperature, (bl, bm), exclude, splits, prior, stamp, window,
                                    gw.sum(dim=1), targets, gw, True)
            # a user none of whose targets count (all fill or invalid, a bad temperature) has no gradient: exactly 0, not 0 * NaN
            grad = torch.where(valid.any(dim=1)[:, None], grad, torch.zeros_like(grad))
        return (grad,) + (None,) * 8


def full_softmax_nll(news_vecs, user_vecs, targets, temperature, exclude=None, splits=0, prior=None, stamp=None, window=None):
    """The full-softmax negative log-likelihood of named targets, differentiable with respect to `user_vecs`: the training-side
    counterpart of score_logz / row_logprob.  targets: integer tensor [U, T <= 128], 0 (or anything outside [1, V)) = fill.
    Forward: score_logz, then row_logprob(sequential=False).  Returns (nll fp32 [U, T], valid bool [U, T]): nll = -logp where
    valid and 0 elsewhere; valid is False at fill entries, at entries row_logprob gives NaN (outside the pool, a NaN score) and
    for users whose temperature is not finite and > 0.  A target inside the user's exclusion lists is the caller's statement and
    is not checked, as in row_logprob.
    Backward: ONE nr_score_expect call on the saved base: grad_user = (sum_t g_t E - sum_t g_t news[target_t]) / temperature over the
    valid entries (include/nrhip.h, K17); a user without a valid target gets exactly 0.
    `news_vecs` is a frozen table: one that requires grad is refused.  Temperature, prior and the other arguments get no gradient."""
    if news_vecs.requires_grad:
        raise RuntimeError("full_softmax_nll: news_vecs requires grad, but the table is frozen here: its gradient P^T . users is a "
                           "[V, N] reduction over every user of the call and is not part of this call (detach the table)")
    if targets.dim() != 2 or targets.shape[0] != user_vecs.shape[0] or targets.is_floating_point():
        raise RuntimeError(f"full_softmax_nll: targets must be an integer tensor [U = {user_vecs.shape[0]}, T], got {tuple(targets.shape)} "
                           f"{targets.dtype}")
    if targets.shape[1] < 1 or targets.shape[1] > _lib.NR_TOPK_MAX_K:
        raise RuntimeError(f"full_softmax_nll: T = {targets.shape[1]} targets per user, must be in [1, {_lib.NR_TOPK_MAX_K}]")
    return FullSoftmaxNLLFunction.apply(user_vecs, news_vecs, targets, temperature, exclude, splits, prior, stamp, window)


@torch.no_grad()
def score_entropy(news_vecs, user_vecs, temperature, base, exclude=None, splits=0, prior=None, stamp=None, window=None):
    """The entropy of the served distribution (nr_score_entropy; include/nrhip.h, K23): per user, with
    p(v) = exp((score_v - smax) / temperature - logsum) over exactly the news score_logz sums over,
    entropy = -sum_v p log p, var = Var_p(log p) = sum p log^2 p - (sum p log p)^2 and mass = sum p -- without the [U, V]
    probability matrix.  exp(entropy) is the effective number of news the user is exposed to under score_sample at this
    temperature; var / temperature is the derivative of the entropy with respect to the temperature.
    `base` = (logsum, smax[, count]): what score_logz returned for the SAME vectors, temperature, exclude and pools; the other
    arguments are score_logz's.  Returns (entropy, var, mass), fp32 [U] each.  A user with nothing eligible gets (0, 0, 0); one
    with exactly one eligible news entropy == 0 and var == 0 exactly; a bad entry of a temperature tensor, or a NaN base, gives
    that user NaN.  `splits`: 0 = the library chooses the number of corpus slices by U.  For a fixed splits > 0 a user's results
    do not depend, bit for bit, on the other users of the call; across different splits they agree to within the bounds of
    DESIGN.md section 5."""
    tau_t = temperature if isinstance(temperature, torch.Tensor) else None
    _need_gpu(news_vecs, user_vecs, exclude.ids if isinstance(exclude, ExclusionLists) else exclude, prior, stamp, window, tau_t, base[0], base[1])
    V, N, U, dev = _vector_args("score_entropy", news_vecs, user_vecs)
    ent = torch.empty(U, dtype=torch.float32, device=dev)
    var = torch.empty(U, dtype=torch.float32, device=dev)
    mass = torch.empty(U, dtype=torch.float32, device=dev)
    if U == 0:
        return ent, var, mass
    bl, bm = _base_args("score_entropy", base, U, dev)
    ex_fields, ex_keep = _exclude_args("score_entropy", exclude, U, dev, dense=False)
    pr, st, win = _pool_args("score_entropy", V, U, dev, prior, stamp, window)
    tau, tau_u = _tau_args("score_entropy", temperature, U, dev)
    d = _lib.EntropyDesc(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, user=ptr(user_vecs),
                         ld_user=user_vecs.stride(0) if U > 1 else N, U=U, N=N, splits=int(splits), **ex_fields, tau=tau, tau_u=ptr(tau_u),
                         base_max=ptr(bm), base_logsum=ptr(bl), out_entropy=ptr(ent), out_var=ptr(var), out_mass=ptr(mass),
                         prior=ptr(pr), stamp=ptr(st), window=ptr(win), ld_window=2 if win is not None else 0)
    ws = _ws(_lib.lib().nr_score_entropy_workspace_bytes(C.byref(d)), dev)   # 0 for a bad descriptor: the call below says why
    d.ws, d.ws_bytes = ptr(ws) if ws.numel() else None, ws.numel() * 4
    check(_lib.lib().nr_score_entropy(C.byref(d), _stream()), "nr_score_entropy")
    return ent, var, mass


def _score_expect_affine(what, news_vecs, user_vecs, temperature, base, exclude, splits, prior, stamp, window, alpha, beta, sub_ids, sub_w,
                         scale_inv_tau):
    """One nr_score_expect_affine call (include/nrhip.h, K24): (out [U, N] fp32, mass [U] fp32)."""
    tau_t = temperature if isinstance(temperature, torch.Tensor) else None
    _need_gpu(news_vecs, user_vecs, exclude.ids if isinstance(exclude, ExclusionLists) else exclude, prior, stamp, window, tau_t, base[0], base[1],
              alpha, beta, sub_ids, sub_w)
    V, N, U, dev = _vector_args(what, news_vecs, user_vecs)
    out = torch.empty(U, N, dtype=torch.float32, device=dev)
    mass = torch.empty(U, dtype=torch.float32, device=dev)
    if U == 0:
        return out, mass
    bl, bm = _base_args(what, base, U, dev)
    coef = []
    for name, t in (("alpha", alpha), ("beta", beta)):
        if t is not None:
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (U,) or not t.is_floating_point() or t.device != dev:
                raise RuntimeError(f"{what}: {name} must be a floating point tensor of shape ({U},) on {dev}")
            t = t.detach().to(torch.float32).contiguous()
        coef.append(t)
    T = 0
    if sub_ids is not None:
        if sub_ids.dim() != 2 or sub_ids.shape[0] != U or sub_ids.is_floating_point() or sub_w is None or tuple(sub_w.shape) != tuple(sub_ids.shape):
            raise RuntimeError(f"{what}: the named rows must be integer ids [U = {U}, T] with weights of the same shape")
        T = sub_ids.shape[1]
        sub_ids = sub_ids.detach().to(torch.int32).contiguous()
        sub_w = sub_w.detach().to(torch.float32).contiguous()
    ex_fields, ex_keep = _exclude_args(what, exclude, U, dev, dense=False)
    pr, st, win = _pool_args(what, V, U, dev, prior, stamp, window)
    tau, tau_u = _tau_args(what, temperature, U, dev)
    d = _lib.ExpectAffineDesc(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, user=ptr(user_vecs),
                              ld_user=user_vecs.stride(0) if U > 1 else N, U=U, N=N, splits=int(splits), **ex_fields, tau=tau, tau_u=ptr(tau_u),
                              base_max=ptr(bm), base_logsum=ptr(bl), alpha=ptr(coef[0]), beta=ptr(coef[1]), sub_ids=ptr(sub_ids),
                              sub_w=ptr(sub_w), ld_sub=T, T=T, scale_inv_tau=1 if scale_inv_tau else 0, out=ptr(out), ld_out=N,
                              out_mass=ptr(mass), prior=ptr(pr), stamp=ptr(st), window=ptr(win), ld_window=2 if win is not None else 0)
    ws = _ws(_lib.lib().nr_score_expect_affine_workspace_bytes(C.byref(d)), dev)   # 0 for a bad descriptor: the call below says why
    d.ws, d.ws_bytes = ptr(ws) if ws.numel() else None, ws.numel() * 4
    check(_lib.lib().nr_score_expect_affine(C.byref(d), _stream()), "nr_score_expect_affine")
    return out, mass


@torch.no_grad()
def score_expect_affine(news_vecs, user_vecs, temperature, base, exclude=None, splits=0, prior=None, stamp=None, window=None, alpha=None,
                        beta=None, sub_ids=None, sub_w=None, scale_inv_tau=False):
    """score_expect with a per-pair weight that is affine in log p (nr_score_expect_affine; include/nrhip.h, K24): per user
    out = sum_v p(v) (alpha + beta log p(v)) news_vecs[v] - sum_t sub_w[t] news_vecs[sub_ids[t]], times 1 / temperature when
    scale_inv_tau.  alpha, beta: optional floating point [U] (None = 1 and 0: score_expect's row, bit for bit at the same explicit
    splits).  With E = score_expect's row and J = sum p log p news, alpha = -H, beta = -1, scale_inv_tau gives the gradient of the
    entropy H with respect to the user vector, -(J + H E) / temperature.  sub_ids, sub_w: optional named rows, integer ids
    [U, T <= 128] (0 or out of range = fill) with weights of the same shape.  The other arguments are score_expect's.
    Returns (out fp32 [U, N], mass fp32 [U]): mass = sum_v p(v), as in score_expect.  A NaN in a user's alpha or beta gives that
    user a row of NaN and touches nobody else."""
    return _score_expect_affine("score_expect_affine", news_vecs, user_vecs, temperature, base, exclude, splits, prior, stamp, window, alpha, beta,
                                sub_ids, sub_w, scale_inv_tau)


def _tau_users(temperature, U):
    """A temperature tensor as the kernels take it: a 0-dim tensor becomes [U]."""
    if isinstance(temperature, torch.Tensor) and temperature.dim() == 0:
        return temperature.detach().to(torch.float32).expand(U).contiguous()
    return temperature.detach() if isinstance(temperature, torch.Tensor) else temperature


class FullSoftmaxEntropyFunction(Function):
    """(nll [U, T], valid, entropy [U]) under the full softmax over the corpus, differentiable with respect to the user vectors and,
    when it is a tensor that requires grad, the temperature."""

    @staticmethod
    def forward(ctx, user_vecs, temperature, news_vecs, targets, exclude, splits, prior, stamp, window):
        user = user_vecs.detach()
        U = user.shape[0]
        tau = _tau_users(temperature, U)
        base = score_logz(news_vecs, user, tau, exclude=exclude, splits=splits, prior=prior, stamp=stamp, window=window)
        logp, _ = row_logprob(news_vecs, user, targets, tau, base, False, prior=prior, stamp=stamp, window=window)
        ent, var, _ = score_entropy(news_vecs, user, tau, base, exclude=exclude, splits=splits, prior=prior, stamp=stamp, window=window)
        V = news_vecs.shape[0]
        valid = (targets >= 1) & (targets < V) & ~torch.isnan(logp)
        if isinstance(tau, torch.Tensor):
            valid &= ((tau > 0) & torch.isfinite(tau))[:, None]
        nll = torch.where(valid, -logp, torch.zeros_like(logp))
        ctx.save_for_backward(user, news_vecs, targets, valid, base[0], base[1], logp, ent, var)
        ctx.rest = (tau, exclude, splits, prior, stamp, window)
        ctx.tau_grad = isinstance(temperature, torch.Tensor) and temperature.requires_grad
        ctx.tau_shape = tuple(temperature.shape) if isinstance(temperature, torch.Tensor) else None
        ctx.tau_dtype = temperature.dtype if isinstance(temperature, torch.Tensor) else None
        ctx.mark_non_differentiable(valid, base[2])
        ctx.set_materialize_grads(False)
        return nll, valid, ent, base[2]

    @staticmethod
    def backward(ctx, g, _gvalid, h, _gcount):
        user, news_vecs, targets, valid, bl, bm, logp, ent, var = ctx.saved_tensors
        tau, exclude, splits, prior, stamp, window = ctx.rest
        if g is None and h is None:
            return (None,) * 9
        dev, U = user.device, user.shape[0]
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        gw = torch.where(valid, g.to(torch.float64), zero) if g is not None else torch.zeros(valid.shape, dtype=torch.float64, device=dev)
        # the entropy of a user the forward answers with NaN (bad temperature, NaN base) has no gradient: exactly 0, not 0 * NaN
        hw = torch.where(torch.isnan(ent), zero, h.to(torch.float64)) if h is not None else torch.zeros(U, dtype=torch.float64, device=dev)
        H = torch.where(torch.isnan(ent), zero, ent.to(torch.float64))
        grad_user = grad_tau = None
        with torch.no_grad():
            if ctx.needs_input_grad[0] and h is None:
                # no entropy gradient arrived: full_softmax_nll's backward, call for call, so its bits
                gw32 = torch.where(valid, g.to(torch.float32), torch.zeros((), dtype=torch.float32, device=dev))
                grad_user, _ = _score_expect("full_softmax_nll_entropy", news_vecs, user, tau, (bl, bm), exclude, splits, prior, stamp, window,
                                             gw32.sum(dim=1), targets, gw32, True)
                grad_user = torch.where(valid.any(dim=1)[:, None], grad_user, torch.zeros_like(grad_user))
            elif ctx.needs_input_grad[0]:
                alpha = (gw.sum(dim=1) - hw * H).to(torch.float32)
                grad_user, _ = _score_expect_affine("full_softmax_nll_entropy", news_vecs, user, tau, (bl, bm), exclude, splits, prior, stamp, window,
                                                    alpha, (-hw).to(torch.float32), targets, gw.to(torch.float32), True)
                # a user with neither a valid target nor an entropy gradient gets exactly 0
                grad_user = torch.where((valid.any(dim=1) | (hw != 0))[:, None], grad_user, torch.zeros_like(grad_user))
            if ctx.tau_grad:
                # d nll_t / d tau = (logp_t - m1) / tau, d H / d tau = var / tau, m1 = -H: [U] elementwise work in fp64
                tau64 = (tau if isinstance(tau, torch.Tensor) else torch.full((U,), float(tau), device=dev)).to(torch.float64)
                good = (tau64 > 0) & torch.isfinite(tau64)
                lp = torch.where(valid, logp.to(torch.float64), zero)
                dnll = (gw * (lp + torch.where(valid, H[:, None], zero))).sum(dim=1)
                dent = hw * torch.where(torch.isnan(var), zero, var.to(torch.float64))
                per_user = torch.where(good, (dnll + dent) / torch.where(good, tau64, torch.ones_like(tau64)), zero)
                grad_tau = (per_user.sum() if ctx.tau_shape == () else per_user).to(ctx.tau_dtype)
        return (grad_user, grad_tau) + (None,) * 7


def full_softmax_nll_entropy(news_vecs, user_vecs, targets, temperature, exclude=None, splits=0, prior=None, stamp=None, window=None,
                             return_count=False):
    """full_softmax_nll with the entropy of the served distribution as a third, differentiable result, and a gradient for the
    temperature.  Returns (nll fp32 [U, T], valid bool [U, T], entropy fp32 [U]): nll and valid are full_softmax_nll's, bit for
    bit; entropy = -sum_v p(v) log p(v) over exactly the news of the softmax (score_entropy; include/nrhip.h, K23): 0 for a user
    with nothing eligible, NaN for a user whose temperature is not finite and > 0.
    Forward: score_logz, row_logprob(sequential=False), score_entropy.  Backward: ONE nr_score_expect_affine call on the saved base
    (K24): for upstream gradients g [U, T] of nll and h [U] of entropy,
    grad_user = ((sum_t g_t - h H) E - h J - sum_t g_t news[target_t]) / temperature over the valid entries; a user with neither a
    valid target nor an entropy gradient gets exactly 0.  When the entropy is in no loss (no h arrives) the one call is
    full_softmax_nll's nr_score_expect call instead, so the gradient then has full_softmax_nll's bits.
    return_count=True appends score_logz's count (int32 [U], the eligible news per user) as a fourth result.
    `temperature`: a float, or a floating point tensor, 0-dim or [U].  A tensor that requires grad (an nn.Parameter, say) gets
    d nll_t / d tau = (logp_t + H) / tau and d H / d tau = Var_p(log p) / tau from the saved forward results, [U] elementwise work
    in fp64; a 0-dim tensor gets the sum over the users.  Users whose temperature is not finite and > 0 contribute 0.
    `news_vecs` is a frozen table: one that requires grad is refused (full_softmax_nll_entropy_joint trains it).  Prior and the other
    arguments get no gradient."""
    if news_vecs.requires_grad:
        raise RuntimeError("full_softmax_nll_entropy: news_vecs requires grad, but the table is frozen here: its gradient P^T . users is a "
                           "[V, N] reduction over every user of the call and is not part of this call (detach the table, or use "
                           "full_softmax_nll_entropy_joint, which has that pass)")
    if targets.dim() != 2 or targets.shape[0] != user_vecs.shape[0] or targets.is_floating_point():
        raise RuntimeError(f"full_softmax_nll_entropy: targets must be an integer tensor [U = {user_vecs.shape[0]}, T], got {tuple(targets.shape)} "
                           f"{targets.dtype}")
    if targets.shape[1] < 1 or targets.shape[1] > _lib.NR_TOPK_MAX_K:
        raise RuntimeError(f"full_softmax_nll_entropy: T = {targets.shape[1]} targets per user, must be in [1, {_lib.NR_TOPK_MAX_K}]")
    if isinstance(temperature, torch.Tensor) and (temperature.dim() > 1 or not temperature.is_floating_point()
                                                  or (temperature.dim() == 1 and temperature.shape[0] != user_vecs.shape[0])):
        raise RuntimeError(f"full_softmax_nll_entropy: a temperature tensor must be floating point, 0-dim or of shape ({user_vecs.shape[0]},), got "
                           f"{tuple(temperature.shape)} {temperature.dtype}")
    nll, valid, ent, count = FullSoftmaxEntropyFunction.apply(user_vecs, temperature, news_vecs, targets, exclude, splits, prior, stamp, window)
    return (nll, valid, ent, count) if return_count else (nll, valid, ent)


def _ref_args(what, ref_vecs, N, U, dev):
    """The reference user vectors of a KL call: [U, N] fp32 with contiguous rows on the call's device."""
    if (not isinstance(ref_vecs, torch.Tensor) or ref_vecs.dim() != 2 or ref_vecs.dtype != torch.float32 or tuple(ref_vecs.shape) != (U, N)
            or ref_vecs.stride(1) != 1 or (U > 1 and ref_vecs.stride(0) < N) or ref_vecs.device != dev):
        got = f"{tuple(ref_vecs.shape)} {ref_vecs.dtype} on {ref_vecs.device}" if isinstance(ref_vecs, torch.Tensor) else type(ref_vecs).__name__
        raise RuntimeError(f"{what}: ref_vecs must be a 2-D fp32 tensor of shape ({U}, {N}) with contiguous rows on {dev}, got {got}")
    return ref_vecs.detach()


def _kl_fields(what, news_vecs, user_vecs, ref_vecs, temperature, base, ref_temperature, ref_base, exclude, prior, stamp, window):
    """The descriptor fields K26 and K27 share, and the tensors they point into (kept alive by the caller)."""
    V, N, U, dev = _vector_args(what, news_vecs, user_vecs)
    ref = _ref_args(what, ref_vecs, N, U, dev)
    bl, bm = _base_args(what, base, U, dev)
    rbl, rbm = _base_args(what + " (reference)", ref_base, U, dev)
    ex_fields, ex_keep = _exclude_args(what, exclude, U, dev, dense=False)
    pr, st, win = _pool_args(what, V, U, dev, prior, stamp, window)
    tau, tau_u = _tau_args(what, temperature, U, dev)
    rtau, rtau_u = _tau_args(what + " (reference)", ref_temperature, U, dev)
    fields = dict(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, user=ptr(user_vecs),
                  ld_user=user_vecs.stride(0) if U > 1 else N, U=U, N=N, **ex_fields, tau=tau, tau_u=ptr(tau_u), base_max=ptr(bm),
                  base_logsum=ptr(bl), ref=ptr(ref), ld_ref=ref.stride(0) if U > 1 else N, ref_tau=rtau, ref_tau_u=ptr(rtau_u),
                  ref_base_max=ptr(rbm), ref_base_logsum=ptr(rbl), prior=ptr(pr), stamp=ptr(st), window=ptr(win),
                  ld_window=2 if win is not None else 0)
    return fields, (ref, bl, bm, rbl, rbm, ex_keep, pr, st, win, tau_u, rtau_u)


def _kl_need_gpu(news_vecs, user_vecs, ref_vecs, temperature, base, ref_temperature, ref_base, exclude, prior, stamp, window, *more):
    _need_gpu(news_vecs, user_vecs, ref_vecs, exclude.ids if isinstance(exclude, ExclusionLists) else exclude, prior, stamp, window,
              temperature if isinstance(temperature, torch.Tensor) else None,
              ref_temperature if isinstance(ref_temperature, torch.Tensor) else None, base[0], base[1], ref_base[0], ref_base[1], *more)


@torch.no_grad()
def score_kl(news_vecs, user_vecs, ref_vecs, temperature, base, ref_temperature, ref_base, exclude=None, splits=0, prior=None, stamp=None,
             window=None):
    """KL divergence of the served distribution to a reference policy (nr_score_kl; include/nrhip.h, K26): per user, with
    p(v) = exp((score_v - smax) / temperature - logsum) from `user_vecs` and q(v) the same statement from `ref_vecs` at
    `ref_temperature`, over exactly the news score_logz sums over for `user_vecs` (lists and pools are shared by the two),
    kl = sum p (log p - log q), entropy = -sum p log p, cov = Cov_p(log p - log q, log p) and mass = sum p -- without the two
    [U, V] matrices.  -cov / temperature is the derivative of kl with respect to the policy's temperature.
    `base` = score_logz(news_vecs, user_vecs, temperature, ...), `ref_base` = score_logz(news_vecs, ref_vecs, ref_temperature, ...) for
    the SAME exclude and pools; temperatures are floats or floating point [U] tensors.  Returns (kl, entropy, cov, mass), fp32 [U]
    each; kl is not clamped (rounding may leave a tiny negative value).  A user with nothing eligible gets zeros; a bad entry of
    either temperature tensor, a NaN in either base, or a reference with nothing eligible gives that user NaN; a reference equal to
    the policy gives kl == 0 and cov == 0 exactly.  `splits`: 0 = the library chooses the number of corpus slices by U.  For a
    fixed splits > 0 a user's results do not depend, bit for bit, on the other users of the call."""
    _kl_need_gpu(news_vecs, user_vecs, ref_vecs, temperature, base, ref_temperature, ref_base, exclude, prior, stamp, window)
    V, N, U, dev = _vector_args("score_kl", news_vecs, user_vecs)
    kl, ent, cov, mass = (torch.empty(U, dtype=torch.float32, device=dev) for _ in range(4))
    if U == 0:
        return kl, ent, cov, mass
    fields, keep = _kl_fields("score_kl", news_vecs, user_vecs, ref_vecs, temperature, base, ref_temperature, ref_base, exclude, prior, stamp,
                              window)
    d = _lib.KlDesc(splits=int(splits), out_kl=ptr(kl), out_entropy=ptr(ent), out_cov=ptr(cov), out_mass=ptr(mass), **fields)
    ws = _ws(_lib.lib().nr_score_kl_workspace_bytes(C.byref(d)), dev)        # 0 for a bad descriptor: the call below says why
    d.ws, d.ws_bytes = ptr(ws) if ws.numel() else None, ws.numel() * 4
    check(_lib.lib().nr_score_kl(C.byref(d), _stream()), "nr_score_kl")
    return kl, ent, cov, mass


def _score_expect_kl(what, news_vecs, user_vecs, ref_vecs, temperature, base, ref_temperature, ref_base, exclude, splits, prior, stamp, window,
                     alpha, beta, gamma, sub_ids, sub_w, scale_inv_tau):
    """One nr_score_expect_kl call (include/nrhip.h, K27): (out [U, N] fp32, mass [U] fp32)."""
    _kl_need_gpu(news_vecs, user_vecs, ref_vecs, temperature, base, ref_temperature, ref_base, exclude, prior, stamp, window, alpha, beta, gamma,
                 sub_ids, sub_w)
    V, N, U, dev = _vector_args(what, news_vecs, user_vecs)
    out = torch.empty(U, N, dtype=torch.float32, device=dev)
    mass = torch.empty(U, dtype=torch.float32, device=dev)
    if U == 0:
        return out, mass
    coef = []
    for name, t in (("alpha", alpha), ("beta", beta), ("gamma", gamma)):
        if t is not None:
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (U,) or not t.is_floating_point() or t.device != dev:
                raise RuntimeError(f"{what}: {name} must be a floating point tensor of shape ({U},) on {dev}")
            t = t.detach().to(torch.float32).contiguous()
        coef.append(t)
    T = 0
    if sub_ids is not None:
        if sub_ids.dim() != 2 or sub_ids.shape[0] != U or sub_ids.is_floating_point() or sub_w is None or tuple(sub_w.shape) != tuple(sub_ids.shape):
            raise RuntimeError(f"{what}: the named rows must be integer ids [U = {U}, T] with weights of the same shape")
        T = sub_ids.shape[1]
        sub_ids = sub_ids.detach().to(torch.int32).contiguous()
        sub_w = sub_w.detach().to(torch.float32).contiguous()
    fields, keep = _kl_fields(what, news_vecs, user_vecs, ref_vecs, temperature, base, ref_temperature, ref_base, exclude, prior, stamp, window)
    d = _lib.ExpectKlDesc(splits=int(splits), alpha=ptr(coef[0]), beta=ptr(coef[1]), gamma=ptr(coef[2]), sub_ids=ptr(sub_ids), sub_w=ptr(sub_w),
                          ld_sub=T, T=T, scale_inv_tau=1 if scale_inv_tau else 0, out=ptr(out), ld_out=N, out_mass=ptr(mass), **fields)
    ws = _ws(_lib.lib().nr_score_expect_kl_workspace_bytes(C.byref(d)), dev)  # 0 for a bad descriptor: the call below says why
    d.ws, d.ws_bytes = ptr(ws) if ws.numel() else None, ws.numel() * 4
    check(_lib.lib().nr_score_expect_kl(C.byref(d), _stream()), "nr_score_expect_kl")
    return out, mass


@torch.no_grad()
def score_expect_kl(news_vecs, user_vecs, ref_vecs, temperature, base, ref_temperature, ref_base, exclude=None, splits=0, prior=None, stamp=None,
                    window=None, alpha=None, beta=None, gamma=None, sub_ids=None, sub_w=None, scale_inv_tau=False):
    """score_expect_affine with a weight that is also affine in the reference's log-probability (nr_score_expect_kl;
    include/nrhip.h, K27): per user
    out = sum_v p(v) (alpha + beta log p(v) + gamma log q(v)) news_vecs[v] - sum_t sub_w[t] news_vecs[sub_ids[t]], times
    1 / temperature when scale_inv_tau; p, q, the bases and the temperatures are score_kl's.  alpha, beta, gamma: optional floating
    point [U] (None = 1, 0, 0).  alpha = -kl, beta = 1, gamma = -1, scale_inv_tau gives the gradient of score_kl's kl with respect to
    the user vector.  The other arguments are score_expect_affine's.  Returns (out fp32 [U, N], mass fp32 [U] = sum_v p(v)).  A NaN
    in a user's alpha, beta or gamma, or on the user's reference side, gives that user a row of NaN and touches nobody else."""
    return _score_expect_kl("score_expect_kl", news_vecs, user_vecs, ref_vecs, temperature, base, ref_temperature, ref_base, exclude, splits, prior,
                            stamp, window, alpha, beta, gamma, sub_ids, sub_w, scale_inv_tau)


class PolicyKLFunction(Function):
    """(kl [U], valid [U]) between the served distribution of `user_vecs` and that of the constant `ref_vecs`, differentiable with
    respect to the user vectors and, in the reverse mode, a temperature tensor that requires grad."""

    @staticmethod
    def forward(ctx, user_vecs, temperature, news_vecs, ref_vecs, ref_temperature, reverse, exclude, splits, prior, stamp, window):
        user, ref = user_vecs.detach(), ref_vecs.detach()
        U = user.shape[0]
        tau = _tau_users(temperature, U)
        rtau = tau if ref_temperature is None else _tau_users(ref_temperature, U)
        kw = dict(exclude=exclude, splits=splits, prior=prior, stamp=stamp, window=window)
        base = score_logz(news_vecs, user, tau, **kw)
        rbase = score_logz(news_vecs, ref, rtau, **kw)
        if reverse:
            kl, _, cov, _ = score_kl(news_vecs, user, ref, tau, base, rtau, rbase, **kw)
        else:
            kl, _, cov, _ = score_kl(news_vecs, ref, user, rtau, rbase, tau, base, **kw)
        # not valid: nothing eligible, or what K26 answers with NaN (a bad temperature entry or a NaN base on either side)
        valid = (base[2] > 0) & (rbase[2] > 0) & ~torch.isnan(kl)
        out = torch.where(valid, kl, torch.zeros_like(kl))
        ctx.save_for_backward(user, ref, news_vecs, valid, base[0], base[1], rbase[0], rbase[1], kl, cov)
        ctx.rest = (tau, rtau, reverse, exclude, splits, prior, stamp, window)
        ctx.tau_grad = isinstance(temperature, torch.Tensor) and temperature.requires_grad
        ctx.tau_shape = tuple(temperature.shape) if isinstance(temperature, torch.Tensor) else None
        ctx.tau_dtype = temperature.dtype if isinstance(temperature, torch.Tensor) else None
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)
        return out, valid

    @staticmethod
    def backward(ctx, g, _gvalid):
        user, ref, news_vecs, valid, bl, bm, rbl, rbm, kl, cov = ctx.saved_tensors
        tau, rtau, reverse, exclude, splits, prior, stamp, window = ctx.rest
        if g is None:
            return (None,) * 11
        dev, U = user.device, user.shape[0]
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        kap = torch.where(valid, g.to(torch.float64), zero)           # an invalid user contributes exactly nothing, not 0 * NaN
        live = (valid & (kap != 0))[:, None]
        grad_user = grad_tau = None
        with torch.no_grad():
            if ctx.needs_input_grad[0] and reverse:
                KL = torch.where(valid, kl.to(torch.float64), zero)
                k32 = kap.to(torch.float32)
                grad_user, _ = _score_expect_kl("policy_kl", news_vecs, user, ref, tau, (bl, bm), rtau, (rbl, rbm), exclude, splits, prior, stamp,
                                                window, (-kap * KL).to(torch.float32), k32, -k32, None, None, True)
                grad_user = torch.where(live, grad_user, torch.zeros_like(grad_user))
            elif ctx.needs_input_grad[0]:
                # d KL(q || p) / d user = (E_p - E_q) / tau: two score_expect calls
                kw = dict(exclude=exclude, splits=splits, prior=prior, stamp=stamp, window=window)
                e_p, _ = score_expect(news_vecs, user, tau, (bl, bm), **kw)
                e_q, _ = score_expect(news_vecs, ref, rtau, (rbl, rbm), **kw)
                tau64 = (tau if isinstance(tau, torch.Tensor) else torch.full((U,), float(tau), device=dev)).to(torch.float64)
                rows = (e_p.to(torch.float64) - e_q.to(torch.float64)) * (kap / torch.where(valid, tau64, torch.ones_like(tau64)))[:, None]
                grad_user = torch.where(live, rows, zero).to(torch.float32)
            if ctx.tau_grad:
                # d KL(p || q) / d tau = -Cov_p(log p - log q, log p) / tau: [U] elementwise work in fp64
                tau64 = (tau if isinstance(tau, torch.Tensor) else torch.full((U,), float(tau), device=dev)).to(torch.float64)
                per_user = torch.where(valid, -kap * torch.where(valid, cov.to(torch.float64), zero) / torch.where(valid, tau64, torch.ones_like(tau64)),
                                       zero)
                grad_tau = (per_user.sum() if ctx.tau_shape == () else per_user).to(ctx.tau_dtype)
        return (grad_user, grad_tau) + (None,) * 9


def policy_kl(news_vecs, user_vecs, ref_vecs, temperature, ref_temperature=None, mode="reverse", exclude=None, splits=0, prior=None, stamp=None,
              window=None):
    """The KL divergence between the served distribution p of `user_vecs` (at `temperature`) and the distribution q of a constant
    reference policy `ref_vecs` (at `ref_temperature`; None = the policy's temperature VALUE, a constant) over the full corpus,
    differentiable with respect to `user_vecs`: the trust region of off-policy training, the distillation loss between two user
    encoders, and the drift between two checkpoints.  Lists and pools are shared by the two policies.
    Returns (kl fp32 [U], valid bool [U]); kl = 0 where not valid: nothing eligible, or a temperature entry on either side that is
    not finite and > 0 (or a NaN base).  Such users contribute no gradient.
    mode="reverse": KL(p || q).  Forward: two score_logz calls and one score_kl call (include/nrhip.h, K26).  Backward: ONE
    nr_score_expect_kl call (K27), grad_user = (g / tau) sum_v p_v (log p_v - log q_v - KL) news_v; a temperature tensor (0-dim or
    [U]) that requires grad gets -g cov / tau, [U] elementwise work in fp64 (a 0-dim tensor the sum over the users).
    mode="forward": KL(q || p), the distillation direction.  The value is score_kl with the roles swapped;
    grad_user = g (E_p - E_q) / tau from two score_expect calls.  A temperature that requires grad is refused in this mode.
    `ref_vecs` and `news_vecs` are constants: one that requires grad is refused."""
    if mode not in ("reverse", "forward"):
        raise RuntimeError(f"policy_kl: mode must be 'reverse' (KL(p || q)) or 'forward' (KL(q || p)), got {mode!r}")
    if isinstance(ref_vecs, torch.Tensor) and ref_vecs.requires_grad:
        raise RuntimeError("policy_kl: ref_vecs requires grad, but the reference policy is a constant here (detach it); training both sides "
                           "is a later policy_kl_joint, not part of this call")
    if news_vecs.requires_grad:
        raise RuntimeError("policy_kl: news_vecs requires grad, but the table is frozen here: its gradient is a [V, N] reduction over every "
                           "user of the call and is not part of this call (detach the table; a later policy_kl_joint would have that pass)")
    for name, t in (("temperature", temperature), ("ref_temperature", ref_temperature)):
        if isinstance(t, torch.Tensor) and (t.dim() > 1 or not t.is_floating_point() or (t.dim() == 1 and t.shape[0] != user_vecs.shape[0])):
            raise RuntimeError(f"policy_kl: a {name} tensor must be floating point, 0-dim or of shape ({user_vecs.shape[0]},), got "
                               f"{tuple(t.shape)} {t.dtype}")
    if isinstance(ref_temperature, torch.Tensor) and ref_temperature.requires_grad:
        raise RuntimeError("policy_kl: ref_temperature requires grad, but the reference policy is a constant here (detach it)")
    if mode == "forward" and isinstance(temperature, torch.Tensor) and temperature.requires_grad:
        raise RuntimeError("policy_kl: temperature requires grad, which mode='forward' (KL(q || p)) does not serve: its temperature gradient "
                           "needs moments under q that no pass here forms (use mode='reverse', or detach the temperature)")
    _vector_args("policy_kl", news_vecs, user_vecs)
    return PolicyKLFunction.apply(user_vecs, temperature, news_vecs, ref_vecs, ref_temperature, mode == "reverse", exclude, splits, prior, stamp,
                                  window)


def _score_expect_news(what, news_vecs, user_vecs, temperature, base, exclude, splits, prior, stamp, window, weight, named, scale_inv_tau, rows):
    """One nr_score_expect_news call (include/nrhip.h, K18): (out [V, N] fp32 or None, mass [V] fp32).  named: None or (offsets
    int32 [V + 1], users int32 [n], w fp32 [n]) on the device."""
    tau_t = temperature if isinstance(temperature, torch.Tensor) else None
    _need_gpu(news_vecs, user_vecs, exclude.ids if isinstance(exclude, ExclusionLists) else exclude, prior, stamp, window, tau_t, base[0], base[1],
              weight, *(named or ()))
    V, N, U, dev = _vector_args(what, news_vecs, user_vecs)
    if U == 0:                                                 # nobody: zeros, nothing to launch
        return (torch.zeros(V, N, dtype=torch.float32, device=dev) if rows else None), torch.zeros(V, dtype=torch.float32, device=dev)
    out = torch.empty(V, N, dtype=torch.float32, device=dev) if rows else None     # the finalize writes every row
    mass = torch.empty(V, dtype=torch.float32, device=dev)
    bl, bm = _base_args(what, base, U, dev)
    if weight is not None:
        if tuple(weight.shape) != (U,) or not weight.is_floating_point() or weight.device != dev:
            raise RuntimeError(f"{what}: weight must be a floating point tensor of shape ({U},) on {dev}")
        weight = weight.detach().to(torch.float32).contiguous()
    if exclude is not None and not isinstance(exclude, ExclusionLists):
        if not isinstance(exclude, torch.Tensor) or exclude.dim() != 2 or exclude.shape[0] != U:
            raise RuntimeError(f"{what}: exclude must be a tensor [U = {U}, E] or an ExclusionLists")
        exclude = ExclusionLists(exclude)
    ex_off = ex_users = None
    if exclude is not None:
        if exclude.U != U or exclude.device != dev:
            raise RuntimeError(f"{what}: the exclusion lists are for {exclude.U} users on {exclude.device}, the call has {U} on {dev}")
        ex_off, ex_users = exclude.by_news(V)
    n_excl = 0 if ex_users is None else ex_users.numel()
    n_off = n_user = n_w = None
    if named is not None:
        n_off, n_user, n_w = named
        if tuple(n_off.shape) != (V + 1,) or n_user.dim() != 1 or tuple(n_w.shape) != tuple(n_user.shape):
            raise RuntimeError(f"{what}: the named terms must be offsets [V + 1 = {V + 1}] with users and weights of one length")
        n_off, n_user, n_w = n_off.to(torch.int32).contiguous(), n_user.to(torch.int32).contiguous(), n_w.detach().to(torch.float32).contiguous()
        if n_user.numel() == 0:
            n_off = n_user = n_w = None
    pr, st, win = _pool_args(what, V, U, dev, prior, stamp, window)
    tau, tau_u = _tau_args(what, temperature, U, dev)
    d = _lib.ExpectNewsDesc(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, user=ptr(user_vecs),
                            ld_user=user_vecs.stride(0) if U > 1 else N, U=U, N=N, splits=int(splits),
                            excl_offsets=ptr(ex_off) if n_excl else None, excl_users=ptr(ex_users) if n_excl else None, n_excl=n_excl,
                            tau=tau, tau_u=ptr(tau_u), base_max=ptr(bm), base_logsum=ptr(bl), weight=ptr(weight),
                            scale_inv_tau=1 if scale_inv_tau else 0, named_offsets=ptr(n_off), named_user=ptr(n_user), named_w=ptr(n_w),
                            n_named=0 if n_user is None else n_user.numel(), out=ptr(out), ld_out=N, out_mass=ptr(mass),
                            prior=ptr(pr), stamp=ptr(st), window=ptr(win), ld_window=2 if win is not None else 0)
    ws = _ws(_lib.lib().nr_score_expect_news_workspace_bytes(C.byref(d)), dev)    # 0 for a bad descriptor: the call below says why
    d.ws, d.ws_bytes = ptr(ws) if ws.numel() else None, ws.numel() * 4
    check(_lib.lib().nr_score_expect_news(C.byref(d), _stream()), "nr_score_expect_news")
    return out, mass


@torch.no_grad()
def score_expect_news(news_vecs, user_vecs, temperature, base, exclude=None, splits=0, prior=None, stamp=None, window=None, weight=None, rows=True):
    """The news side of score_expect (nr_score_expect_news; include/nrhip.h, K18): per news
    D_v = sum_u weight_u p(v | u) user_vecs[u], p(v | u) = exp((score_uv - smax_u) / temperature - logsum_u), over exactly the
    pairs score_logz sums over -- the gradient of sum_u weight_u temperature log Z_u with respect to the news vector -- without
    the [U, V] probability matrix.  `base`, `exclude` (PER USER, as everywhere: an ExclusionLists or a tensor [U, E]; it is
    transposed here with ExclusionLists.by_news), the pools and `weight` are score_expect's.
    Returns (out fp32 [V, N] or None, mass fp32 [V]): mass[v] = sum_u weight_u p(v | u), the expected exposure of news v.
    rows=False is the mass-only mode: no second contraction, `out` is None, the same mass bits.  A user whose temperature is not
    finite and > 0, whose base is NaN or infinite, or who has nothing eligible contributes nothing; row 0 is zeros.
    `splits`: 0 = the library chooses the number of USER slices by V.  For a fixed splits > 0 a row's bits do not depend on the
    other news rows or on its place in the table; across different splits rows agree within the bound of DESIGN.md section 5."""
    return _score_expect_news("score_expect_news", news_vecs, user_vecs, temperature, base, exclude, splits, prior, stamp, window, weight, None,
                              False, rows)


def _named_by_news(targets, gw, V):
    """The named terms of K18 from targets [U, T] and their weights gw [U, T] (0 = does not count): entries with gw != 0 and a
    target in [1, V), by a STABLE sort on the news id, so within a news they come (user, t) ascending.  Returns (offsets int32
    [V + 1], users int32 [n], w fp32 [n])."""
    U, T = targets.shape
    tg = targets.reshape(-1).to(torch.int64)
    keep = (gw.reshape(-1) != 0) & (tg >= 1) & (tg < V)
    at = torch.nonzero(keep).reshape(-1)                       # ascending flat index u * T + t
    order = torch.sort(tg[at], stable=True).indices
    at = at[order]
    offsets = torch.zeros(V + 1, dtype=torch.int64, device=targets.device)
    offsets[1:] = torch.cumsum(torch.bincount(tg[at], minlength=V), 0)
    return offsets.to(torch.int32), (at // T).to(torch.int32), gw.reshape(-1)[at].to(torch.float32)


class FullSoftmaxNLLJointFunction(Function):
    """nll [U, T] of named targets under the full softmax over the corpus, differentiable with respect to the user vectors (one
    K17 call) and the news-vector table (one K18 call)."""

    @staticmethod
    def forward(ctx, user_vecs, news_vecs, targets, temperature, exclude, splits, prior, stamp, window):
        user, news = user_vecs.detach(), news_vecs.detach()
        base = score_logz(news, user, temperature, exclude=exclude, splits=splits, prior=prior, stamp=stamp, window=window)
        logp, _ = row_logprob(news, user, targets, temperature, base, False, prior=prior, stamp=stamp, window=window)
        V = news.shape[0]
        valid = (targets >= 1) & (targets < V) & ~torch.isnan(logp)
        if isinstance(temperature, torch.Tensor):
            valid &= ((temperature > 0) & torch.isfinite(temperature))[:, None]
        nll = torch.where(valid, -logp, torch.zeros_like(logp))
        ctx.save_for_backward(user, news, targets, valid, base[0], base[1])
        ctx.rest = (temperature, exclude, splits, prior, stamp, window)
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)
        return nll, valid

    @staticmethod
    def backward(ctx, g, _gvalid):
        user, news, targets, valid, bl, bm = ctx.saved_tensors
        temperature, exclude, splits, prior, stamp, window = ctx.rest
        if g is None:
            return (None,) * 9
        gw = torch.where(valid, g.to(torch.float32), torch.zeros((), dtype=torch.float32, device=g.device))
        grad_user = grad_news = None
        with torch.no_grad():
            if ctx.needs_input_grad[0]:
                grad_user, _ = _score_expect("full_softmax_nll_joint", news, user, temperature, (bl, bm), exclude, splits, prior, stamp, window,
                                             gw.sum(dim=1), targets, gw, True)
                # a user none of whose targets count (all fill or invalid, a bad temperature) has no gradient: exactly 0, not 0 * NaN
                grad_user = torch.where(valid.any(dim=1)[:, None], grad_user, torch.zeros_like(grad_user))
            if ctx.needs_input_grad[1]:
                # K18 takes the user slices by its own plan: `splits` is K13's / K17's cut of the news axis and does not apply
                grad_news, _ = _score_expect_news("full_softmax_nll_joint", news, user, temperature, (bl, bm), exclude, 0, prior, stamp, window,
                                                  gw.sum(dim=1), _named_by_news(targets, gw, news.shape[0]), True, True)
        return (grad_user, grad_news) + (None,) * 7


def full_softmax_nll_joint(news_vecs, user_vecs, targets, temperature, exclude=None, splits=0, prior=None, stamp=None, window=None):
    """full_softmax_nll, differentiable with respect to `user_vecs` AND the table `news_vecs`: either may require grad.  The
    forward is full_softmax_nll's (score_logz, then row_logprob(sequential=False)), bit for bit, and returns (nll fp32 [U, T],
    valid bool [U, T]) as it does.  Backward: grad_user is full_softmax_nll's single nr_score_expect call (K17), bit for bit;
    grad_news [V, N] is ONE nr_score_expect_news call (include/nrhip.h, K18) with weight = sum_t g_t, the 1 / temperature scale
    inside, and the valid targets as its named terms (stable sort by news id; entries with g = 0 and invalid entries dropped):
      grad_news[v] = sum_u (sum_t g_ut) / tau_u p(v | u) user_u  -  sum_{(u, t): target = v} g_ut / tau_u user_u.
    News that are eligible for nobody and named by nobody get an exactly zero row; row 0 always.  A pass whose input does not
    require grad is not launched.  Temperature, prior and the other arguments get no gradient."""
    if targets.dim() != 2 or targets.shape[0] != user_vecs.shape[0] or targets.is_floating_point():
        raise RuntimeError(f"full_softmax_nll_joint: targets must be an integer tensor [U = {user_vecs.shape[0]}, T], got {tuple(targets.shape)} "
                           f"{targets.dtype}")
    if targets.shape[1] < 1 or targets.shape[1] > _lib.NR_TOPK_MAX_K:
        raise RuntimeError(f"full_softmax_nll_joint: T = {targets.shape[1]} targets per user, must be in [1, {_lib.NR_TOPK_MAX_K}]")
    return FullSoftmaxNLLJointFunction.apply(user_vecs, news_vecs, targets, temperature, exclude, splits, prior, stamp, window)


def _score_expect_news_affine(what, news_vecs, user_vecs, temperature, base, exclude, splits, prior, stamp, window, alpha, beta, named,
                              scale_inv_tau):
    """One nr_score_expect_news_affine call (include/nrhip.h, K25): (out [V, N] fp32, mass [V] fp32).  _score_expect_news with the
    two coefficient arrays in place of the weight; named: None or (offsets int32 [V + 1], users int32 [n], w fp32 [n]) on the device."""
    tau_t = temperature if isinstance(temperature, torch.Tensor) else None
    _need_gpu(news_vecs, user_vecs, exclude.ids if isinstance(exclude, ExclusionLists) else exclude, prior, stamp, window, tau_t, base[0], base[1],
              alpha, beta, *(named or ()))
    V, N, U, dev = _vector_args(what, news_vecs, user_vecs)
    if U == 0:                                                 # nobody: zeros, nothing to launch
        return torch.zeros(V, N, dtype=torch.float32, device=dev), torch.zeros(V, dtype=torch.float32, device=dev)
    out = torch.empty(V, N, dtype=torch.float32, device=dev)  # the finalize writes every row
    mass = torch.empty(V, dtype=torch.float32, device=dev)
    bl, bm = _base_args(what, base, U, dev)
    coef = []
    for name, t in (("alpha", alpha), ("beta", beta)):
        if t is not None:
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (U,) or not t.is_floating_point() or t.device != dev:
                raise RuntimeError(f"{what}: {name} must be a floating point tensor of shape ({U},) on {dev}")
            t = t.detach().to(torch.float32).contiguous()
        coef.append(t)
    if exclude is not None and not isinstance(exclude, ExclusionLists):
        if not isinstance(exclude, torch.Tensor) or exclude.dim() != 2 or exclude.shape[0] != U:
            raise RuntimeError(f"{what}: exclude must be a tensor [U = {U}, E] or an ExclusionLists")
        exclude = ExclusionLists(exclude)
    ex_off = ex_users = None
    if exclude is not None:
        if exclude.U != U or exclude.device != dev:
            raise RuntimeError(f"{what}: the exclusion lists are for {exclude.U} users on {exclude.device}, the call has {U} on {dev}")
        ex_off, ex_users = exclude.by_news(V)
    n_excl = 0 if ex_users is None else ex_users.numel()
    n_off = n_user = n_w = None
    if named is not None:
        n_off, n_user, n_w = named
        if tuple(n_off.shape) != (V + 1,) or n_user.dim() != 1 or tuple(n_w.shape) != tuple(n_user.shape):
            raise RuntimeError(f"{what}: the named terms must be offsets [V + 1 = {V + 1}] with users and weights of one length")
        n_off, n_user, n_w = n_off.to(torch.int32).contiguous(), n_user.to(torch.int32).contiguous(), n_w.detach().to(torch.float32).contiguous()
        if n_user.numel() == 0:
            n_off = n_user = n_w = None
    pr, st, win = _pool_args(what, V, U, dev, prior, stamp, window)
    tau, tau_u = _tau_args(what, temperature, U, dev)
    d = _lib.ExpectNewsAffineDesc(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, user=ptr(user_vecs),
                                  ld_user=user_vecs.stride(0) if U > 1 else N, U=U, N=N, splits=int(splits),
                                  excl_offsets=ptr(ex_off) if n_excl else None, excl_users=ptr(ex_users) if n_excl else None, n_excl=n_excl,
                                  tau=tau, tau_u=ptr(tau_u), base_max=ptr(bm), base_logsum=ptr(bl), alpha=ptr(coef[0]), beta=ptr(coef[1]),
                                  scale_inv_tau=1 if scale_inv_tau else 0, named_offsets=ptr(n_off), named_user=ptr(n_user), named_w=ptr(n_w),
                                  n_named=0 if n_user is None else n_user.numel(), out=ptr(out), ld_out=N, out_mass=ptr(mass),
                                  prior=ptr(pr), stamp=ptr(st), window=ptr(win), ld_window=2 if win is not None else 0)
    ws = _ws(_lib.lib().nr_score_expect_news_affine_workspace_bytes(C.byref(d)), dev)   # 0 for a bad descriptor: the call below says why
    d.ws, d.ws_bytes = ptr(ws) if ws.numel() else None, ws.numel() * 4
    check(_lib.lib().nr_score_expect_news_affine(C.byref(d), _stream()), "nr_score_expect_news_affine")
    return out, mass


@torch.no_grad()
def score_expect_news_affine(news_vecs, user_vecs, temperature, base, exclude=None, splits=0, prior=None, stamp=None, window=None, alpha=None,
                             beta=None):
    """score_expect_news with a per-pair weight that is affine in log p (nr_score_expect_news_affine; include/nrhip.h, K25): per news
    out[v] = sum_u p(v | u) (alpha_u + beta_u log p(v | u)) user_vecs[u], over exactly the pairs score_logz sums over, without the
    [U, V] probability matrix.  alpha, beta: optional floating point [U] (None = 1 and 0); with beta None the rows are
    score_expect_news's with weight = alpha, bit for bit at the same explicit splits.  alpha = -H_u, beta = -1 gives the gradient of
    sum_u temperature H_u with respect to the news vector.  The other arguments are score_expect_news's.
    Returns (out fp32 [V, N], mass fp32 [V]): mass[v] = sum_u p(v | u) over the live users, score_expect_news's mass without a
    weight -- not the sum of the affine weights.  A user whose alpha or beta is NaN or infinite contributes to no row (and puts
    no NaN into the table); the dead users are score_expect_news's.  There is no mass-only mode: score_expect_news(rows=False)
    is that."""
    return _score_expect_news_affine("score_expect_news_affine", news_vecs, user_vecs, temperature, base, exclude, splits, prior, stamp, window,
                                     alpha, beta, None, False)


class FullSoftmaxEntropyJointFunction(Function):
    """FullSoftmaxEntropyFunction, differentiable with respect to the news-vector table as well: (nll [U, T], valid, entropy [U],
    count).  The forward, grad_user and grad_tau are that function's own code on the detached table; grad_news is one K25 call, or
    one K18 call when no entropy gradient arrived."""

    @staticmethod
    def forward(ctx, user_vecs, temperature, news_vecs, targets, exclude, splits, prior, stamp, window):
        return FullSoftmaxEntropyFunction.forward(ctx, user_vecs, temperature, news_vecs.detach(), targets, exclude, splits, prior, stamp, window)

    @staticmethod
    def backward(ctx, g, _gvalid, h, _gcount):
        if g is None and h is None:
            return (None,) * 9
        # the user vectors and the temperature: needs_input_grad[0] and ctx.tau_grad decide there what is launched
        grad_user, grad_tau = FullSoftmaxEntropyFunction.backward(ctx, g, _gvalid, h, _gcount)[:2]
        grad_news = None
        if ctx.needs_input_grad[2]:
            user, news, targets, valid, bl, bm, logp, ent, var = ctx.saved_tensors
            tau, exclude, splits, prior, stamp, window = ctx.rest
            dev, U, V = user.device, user.shape[0], news.shape[0]
            with torch.no_grad():
                # K18 / K25 take the user slices by their own plan: `splits` is K13's / K24's cut of the news axis and does not apply
                if h is None:
                    # no entropy gradient arrived: full_softmax_nll_joint's K18 call, so its bits
                    gw32 = torch.where(valid, g.to(torch.float32), torch.zeros((), dtype=torch.float32, device=dev))
                    grad_news, _ = _score_expect_news("full_softmax_nll_entropy_joint", news, user, tau, (bl, bm), exclude, 0, prior, stamp, window,
                                                      gw32.sum(dim=1), _named_by_news(targets, gw32, V), True, True)
                else:
                    # the alpha and beta FullSoftmaxEntropyFunction.backward gives K24, formed the same way
                    zero = torch.zeros((), dtype=torch.float64, device=dev)
                    gw = torch.where(valid, g.to(torch.float64), zero) if g is not None else torch.zeros(valid.shape, dtype=torch.float64, device=dev)
                    hw = torch.where(torch.isnan(ent), zero, h.to(torch.float64))
                    H = torch.where(torch.isnan(ent), zero, ent.to(torch.float64))
                    alpha = (gw.sum(dim=1) - hw * H).to(torch.float32)
                    grad_news, _ = _score_expect_news_affine("full_softmax_nll_entropy_joint", news, user, tau, (bl, bm), exclude, 0, prior, stamp,
                                                             window, alpha, (-hw).to(torch.float32),
                                                             _named_by_news(targets, gw.to(torch.float32), V), True)
        return (grad_user, grad_tau, grad_news) + (None,) * 6


def full_softmax_nll_entropy_joint(news_vecs, user_vecs, targets, temperature, exclude=None, splits=0, prior=None, stamp=None, window=None,
                                   return_count=False):
    """full_softmax_nll_entropy, differentiable with respect to `user_vecs`, the temperature AND the table `news_vecs`: any of them
    may require grad.  The forward is full_softmax_nll_entropy's (score_logz, row_logprob(sequential=False), score_entropy), bit
    for bit, and returns (nll fp32 [U, T], valid bool [U, T], entropy fp32 [U]) as it does (return_count=True appends the count);
    grad_user and the temperature's gradient are its own, call for call.  grad_news [V, N] is ONE nr_score_expect_news_affine call
    (include/nrhip.h, K25) on the saved base with the alpha = sum_t g_t - h H and beta = -h that go to K24, the 1 / temperature
    scale inside, and the valid targets as its named terms:
      grad_news[v] = sum_u p(v | u) (alpha_u + beta_u log p(v | u)) / tau_u user_u  -  sum_{(u, t): target = v} g_ut / tau_u user_u.
    When the entropy is in no loss (no h arrives) it is full_softmax_nll_joint's nr_score_expect_news call instead, so the gradient
    then has that function's bits.  News that are eligible for nobody and named by nobody get an exactly zero row; row 0 always.
    A pass whose input does not require grad is not launched.  Prior and the other arguments get no gradient."""
    if targets.dim() != 2 or targets.shape[0] != user_vecs.shape[0] or targets.is_floating_point():
        raise RuntimeError(f"full_softmax_nll_entropy_joint: targets must be an integer tensor [U = {user_vecs.shape[0]}, T], got "
                           f"{tuple(targets.shape)} {targets.dtype}")
    if targets.shape[1] < 1 or targets.shape[1] > _lib.NR_TOPK_MAX_K:
        raise RuntimeError(f"full_softmax_nll_entropy_joint: T = {targets.shape[1]} targets per user, must be in [1, {_lib.NR_TOPK_MAX_K}]")
    if isinstance(temperature, torch.Tensor) and (temperature.dim() > 1 or not temperature.is_floating_point()
                                                  or (temperature.dim() == 1 and temperature.shape[0] != user_vecs.shape[0])):
        raise RuntimeError(f"full_softmax_nll_entropy_joint: a temperature tensor must be floating point, 0-dim or of shape "
                           f"({user_vecs.shape[0]},), got {tuple(temperature.shape)} {temperature.dtype}")
    nll, valid, ent, count = FullSoftmaxEntropyJointFunction.apply(user_vecs, temperature, news_vecs, targets, exclude, splits, prior, stamp, window)
    return (nll, valid, ent, count) if return_count else (nll, valid, ent)


@torch.no_grad()
def row_logprob_grad(news_vecs, user_vecs, row_ids, temperature, base, g=None, prior=None, stamp=None, window=None):
    """The gradient coefficients of sequential rows (nr_row_logprob_grad; include/nrhip.h, K19): the backward of
    row_logprob(sequential=True).  `row_ids`, `temperature`, `base` and the pools are row_logprob's, the base formed WITHOUT the
    row's ids; `g`: optional floating point [U, k], the upstream gradient of nll_j = -logp_j per entry (None = 1).
    Returns (weight fp32 [U], sub_w fp32 [U, k]) = (a, c) with
      d (sum_j g_j nll_j) / d user = (a E_rest - sum_i c_i news_vecs[row_i]) / temperature,
    E_rest the expected news vector over what the base sums over: nr_score_expect with weight = a, the row and c as its named rows
    and the lists of the base's score_logz call; the news side is nr_score_expect_news with the same weight and (row, c) as its
    named terms.  Fill entries and entries outside the pool or with a NaN score get c = 0 and their g is not read; a user with
    a bad temperature entry or a NaN base gets zeros; an empty base gives a = 0.  a = sum_i c_i up to rounding."""
    tau_t = temperature if isinstance(temperature, torch.Tensor) else None
    _need_gpu(news_vecs, user_vecs, row_ids, prior, stamp, window, tau_t, base[0], base[1], g)
    V, N, U, dev = _vector_args("row_logprob_grad", news_vecs, user_vecs)
    if row_ids.dim() != 2 or row_ids.shape[0] != U or row_ids.is_floating_point() or row_ids.device != dev:
        raise RuntimeError(f"row_logprob_grad: row_ids must be an integer tensor [U = {U}, k] on {dev}, got {tuple(row_ids.shape)} {row_ids.dtype} "
                           f"on {row_ids.device}")
    k = row_ids.shape[1]
    weight = torch.empty(U, dtype=torch.float32, device=dev)
    sub_w = torch.empty(U, k, dtype=torch.float32, device=dev)
    if U == 0:
        return weight, sub_w
    if g is not None:
        if tuple(g.shape) != (U, k) or not g.is_floating_point() or g.device != dev:
            raise RuntimeError(f"row_logprob_grad: g must be a floating point tensor of shape ({U}, {k}) on {dev}")
        g = g.detach().to(torch.float32).contiguous()
    bl, bm = _base_args("row_logprob_grad", base, U, dev)
    ids = row_ids.detach().to(torch.int32).contiguous()
    pr, st, win = _pool_args("row_logprob_grad", V, U, dev, prior, stamp, window)
    tau, tau_u = _tau_args("row_logprob_grad", temperature, U, dev)
    d = _lib.LogprobGradDesc(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, user=ptr(user_vecs),
                             ld_user=user_vecs.stride(0) if U > 1 else N, U=U, N=N, k=k, row_ids=ptr(ids), ld_ids=k, tau=tau,
                             tau_u=ptr(tau_u), base_max=ptr(bm), base_logsum=ptr(bl), g=ptr(g), ld_g=k if g is not None else 0,
                             out_weight=ptr(weight), out_sub_w=ptr(sub_w), prior=ptr(pr), stamp=ptr(st), window=ptr(win),
                             ld_window=2 if win is not None else 0)
    check(_lib.lib().nr_row_logprob_grad(C.byref(d), _stream()), "nr_row_logprob_grad")
    return weight, sub_w


class PlackettLuceNLLFunction(Function):
    """nll [U, k] of the places of sequential rows (Plackett-Luce without replacement over the corpus), differentiable with respect
    to the user vectors (K19, then one K17 call) and the news-vector table (K19, then one K18 call)."""

    @staticmethod
    def forward(ctx, user_vecs, news_vecs, rows, temperature, exclude, splits, prior, stamp, window):
        user, news = user_vecs.detach(), news_vecs.detach()
        V = news.shape[0]
        taken = ExclusionLists(rows)
        if exclude is None:
            lists = taken
        else:
            lists = (exclude if isinstance(exclude, ExclusionLists) else ExclusionLists(exclude)).merged(taken)
        base = score_logz(news, user, temperature, exclude=lists, splits=splits, prior=prior, stamp=stamp, window=window)
        logp, _ = row_logprob(news, user, rows, temperature, base, True, prior=prior, stamp=stamp, window=window)
        valid = (rows >= 1) & (rows < V) & ~torch.isnan(logp)
        if isinstance(temperature, torch.Tensor):
            valid &= ((temperature > 0) & torch.isfinite(temperature))[:, None]
        nll = torch.where(valid, -logp, torch.zeros_like(logp))
        ctx.save_for_backward(user, news, rows, valid, base[0], base[1])
        ctx.rest = (temperature, lists, splits, prior, stamp, window)
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)
        return nll, valid

    @staticmethod
    def backward(ctx, g, _gvalid):
        user, news, rows, valid, bl, bm = ctx.saved_tensors
        temperature, lists, splits, prior, stamp, window = ctx.rest
        if g is None:
            return (None,) * 9
        gw = torch.where(valid, g.to(torch.float32), torch.zeros((), dtype=torch.float32, device=g.device))
        grad_user = grad_news = None
        with torch.no_grad():
            a, c = row_logprob_grad(news, user, rows, temperature, (bl, bm), g=gw, prior=prior, stamp=stamp, window=window)
            if ctx.needs_input_grad[0]:
                grad_user, _ = _score_expect("plackett_luce_nll", news, user, temperature, (bl, bm), lists, splits, prior, stamp, window,
                                             a, rows, c, True)
                # a user none of whose places count (all fill or invalid, a bad temperature) has no gradient: exactly 0, not 0 * NaN
                grad_user = torch.where(valid.any(dim=1)[:, None], grad_user, torch.zeros_like(grad_user))
            if ctx.needs_input_grad[1]:
                # K18 leaves out a user with nothing eligible, named terms included.  A row that takes everything eligible has such a
                # base and still has named terms (a = 0, c != 0); nothing of its stream is eligible, so any finite base gives them
                # back and adds nothing else.  `splits` is K13's / K17's cut of the news axis and does not apply to K18.
                empty = torch.isneginf(bm)
                zero = torch.zeros_like(bm)
                grad_news, _ = _score_expect_news("plackett_luce_nll", news, user, temperature,
                                                  (torch.where(empty, zero, bl), torch.where(empty, zero, bm)), lists, 0, prior, stamp, window,
                                                  a, _named_by_news(rows, c, news.shape[0]), True, True)
        return (grad_user, grad_news) + (None,) * 7


def plackett_luce_nll(news_vecs, user_vecs, rows, temperature, exclude=None, splits=0, prior=None, stamp=None, window=None):
    """The negative log-likelihood of ordered rows under the Plackett-Luce law score_sample draws from, place by place, with a
    gradient for `user_vecs` AND the table `news_vecs` (either may require grad): the training-side counterpart of
    train.sample_propensity.  rows: integer tensor [U, k <= 128], 0 (or anything outside [1, V)) = fill; place j is scored
    against everything eligible that places 0 .. j-1 have not taken.
    Forward: `rows` merged into `exclude` (ExclusionLists(rows), .merged), score_logz on those lists, row_logprob(sequential=True)
    -- what sample_propensity launches, so nll[valid] = -logp of it, bit for bit.  Returns (nll fp32 [U, k], valid bool [U, k]):
    valid is False at fill entries, at entries row_logprob gives NaN (outside the pool, a NaN score) and for users whose
    temperature is not finite and > 0; nll is 0 there.  Repeats within a row and entries inside `exclude` are the caller's
    statement and are not checked, as in row_logprob (train.listwise_loss turns them into fill).
    Backward: ONE nr_row_logprob_grad call (include/nrhip.h, K19) with g zeroed where not valid gives the coefficients (a, c);
    then grad_user = (a E_rest - sum_i c_i news[row_i]) / temperature is one nr_score_expect call (K17: weight a, named rows
    (rows, c), the merged lists, the saved base) and grad_news one nr_score_expect_news call (K18: weight a, named terms (rows,
    c)).  A pass whose input does not require grad is not launched; a user without a valid place gets an exactly zero row.
    Temperature, prior and the other arguments get no gradient."""
    if rows.dim() != 2 or rows.shape[0] != user_vecs.shape[0] or rows.is_floating_point():
        raise RuntimeError(f"plackett_luce_nll: rows must be an integer tensor [U = {user_vecs.shape[0]}, k], got {tuple(rows.shape)} {rows.dtype}")
    if rows.shape[1] < 1 or rows.shape[1] > _lib.NR_TOPK_MAX_K:
        raise RuntimeError(f"plackett_luce_nll: k = {rows.shape[1]} places per row, must be in [1, {_lib.NR_TOPK_MAX_K}]: a sequential row "
                           "cannot be cut into chunks")
    return PlackettLuceNLLFunction.apply(user_vecs, news_vecs, rows, temperature, exclude, splits, prior, stamp, window)


class NewsGatherFunction(Function):
    """out[i] = table[ids[i]] with a gradient for the table: nr_gather_cast_fwd forward, nr_embed_gather_bwd backward."""

    @staticmethod
    def forward(ctx, table, ids, code):
        ctx.save_for_backward(ids)
        ctx.table_shape = tuple(table.shape)
        return embed_gather(table, ids, code)

    @staticmethod
    def backward(ctx, dout):
        _enter_backward()
        (ids,) = ctx.saved_tensors
        V, cols = ctx.table_shape
        dout = dout.contiguous().float().reshape(-1, cols)
        dtable = torch.zeros(V, cols, dtype=torch.float32, device=dout.device)
        if ids.numel():
            check(_lib.lib().nr_embed_gather_bwd(ptr(dout), cols, ptr(ids), ids.numel(), 1, cols, ptr(dtable), cols, _stream()),
                  "nr_embed_gather_bwd")
        return dtable, None, None


def news_gather(table: torch.Tensor, ids: torch.Tensor, code: int = NR_F32) -> torch.Tensor:
    """A differentiable embed_gather: out[i] = table[ids[i]] (fp32 table [V, N]; `code` = dtype of the result), and in backward
    dtable[ids[i]] += dout[i] into a zeroed [V, N] fp32 (nr_embed_gather_bwd).  Row 0, the padding news, gets no gradient.  The
    scatter adds with fp32 atomics: where an id repeats, the last bits of its row depend on the arrival order."""
    _need_gpu(table, ids)
    if table.dim() != 2 or table.dtype != torch.float32:
        raise RuntimeError(f"news_gather: table must be a 2-D fp32 tensor, got {tuple(table.shape)} {table.dtype}")
    ids = ids.to(torch.int32).contiguous()
    if CHECK_INDICES:
        check_ids(ids, table.shape[0], "news index")
    return NewsGatherFunction.apply(table, ids, code)


class GroupOrder:
    """The group-major order of a corpus, which score_logz_groups streams over (include/nrhip.h, K15).  Build it once per corpus
    -- as an ExclusionLists is built once per batch of users -- and hand it to as many calls as needed; everything in it is a
    function of `group` alone.  It lives on the device of `group`; CPU tensors work as well (nothing here launches a kernel).
      group     int32 [V]: one group id per news in [0, n_groups), negative = in no group; n_groups <= 512
      n_groups  None takes max id + 1 (at least 1).  An id >= n_groups raises ValueError.
    Bins b = 0 .. n_groups - 1 are the groups, bin n_groups is "no group".  What it holds:
      order      int32 [n_pos]: news 1 .. V-1 sorted by (bin, id); every bin's run is padded with id 0 up to a multiple of 128
                 positions (one chunk of the scoring tile).  Id 0 is never eligible.
      pos        int32 [V]: the inverse map id -> position (-1 for id 0)
      bin_start  int32 [n_groups + 2]: bin b owns positions bin_start[b] .. bin_start[b + 1] - 1
      seg_start  int32 [nseg + 1], bin_seg int32 [n_groups + 2]: with S = chunks_per_segment = ceil((n_pos / 128) / 256), every
                 bin's run is cut into segments of at most S chunks; a segment never straddles two bins; bin b owns segments
                 bin_seg[b] .. bin_seg[b + 1] - 1; nseg <= 256 + n_groups + 1.
    Two host synchronisations (the largest id, the bin sizes); the tables are host arithmetic on the bin sizes."""

    CHUNK, MAX_SEGS = 128, 256

    def __init__(self, group, n_groups=None):
        if not isinstance(group, torch.Tensor) or group.dim() != 1 or group.dtype != torch.int32 or group.numel() < 2:
            raise RuntimeError(f"GroupOrder: group must be an int32 tensor [V >= 2], got "
                               f"{(tuple(group.shape), group.dtype) if isinstance(group, torch.Tensor) else type(group)}")
        g = group.detach().to(torch.int64)
        dev, V = g.device, g.numel()
        top = int(g.max())
        G = max(top + 1, 1) if n_groups is None else int(n_groups)
        if not 1 <= G <= _lib.NR_RANK_MAX_GROUPS:
            raise ValueError(f"GroupOrder: n_groups = {G}, must be in [1, {_lib.NR_RANK_MAX_GROUPS}]")
        if top >= G:
            raise ValueError(f"GroupOrder: group id {top} >= n_groups = {G}")
        bins = torch.where(g < 0, torch.full_like(g, G), g)[1:]
        ids = torch.arange(1, V, dtype=torch.int64, device=dev)
        srt = torch.sort(bins * V + ids).values                          # (bin, id) ascending
        sb, sid = srt // V, srt % V
        counts = torch.bincount(bins, minlength=G + 1)
        cnt = [int(x) for x in counts.tolist()]
        C = self.CHUNK
        padded = [(c + C - 1) // C * C for c in cnt]
        bin_start = [0]
        for p in padded:
            bin_start.append(bin_start[-1] + p)
        n_pos = bin_start[-1]
        S = max(1, (n_pos // C + self.MAX_SEGS - 1) // self.MAX_SEGS)
        seg_start, bin_seg = [], [0]
        for b in range(G + 1):
            seg_start.extend(range(bin_start[b], bin_start[b + 1], S * C))
            bin_seg.append(len(seg_start))
        seg_start.append(n_pos)
        first = torch.zeros(G + 1, dtype=torch.int64, device=dev)        # of a bin: its first place in the sorted run
        first[1:] = torch.cumsum(counts, 0)[:-1]
        at = torch.tensor(bin_start[:-1], dtype=torch.int64, device=dev)[sb] + (torch.arange(V - 1, dtype=torch.int64, device=dev) - first[sb])
        order = torch.zeros(n_pos, dtype=torch.int32, device=dev)
        order[at] = sid.to(torch.int32)
        pos = torch.full((V,), -1, dtype=torch.int32, device=dev)
        pos[sid] = at.to(torch.int32)
        self.V, self.n_groups, self.n_pos, self.nseg, self.chunks_per_segment = V, G, n_pos, len(seg_start) - 1, S
        self.order, self.pos = order, pos
        self.bin_start = torch.tensor(bin_start, dtype=torch.int32, device=dev)
        self.seg_start = torch.tensor(seg_start, dtype=torch.int32, device=dev)
        self.bin_seg = torch.tensor(bin_seg, dtype=torch.int32, device=dev)

    @property
    def device(self):
        return self.order.device

    def positions(self, lists):
        """An ExclusionLists in position space: every id in [1, V) mapped through id -> position, each user's list re-sorted
        (strictly ascending positions, which is what the stream over `order` meets in ascending order); other ids are dropped."""
        users, ids = lists._pairs()
        keep = (ids >= 1) & (ids < self.V)
        users, ids = users[keep], ids[keep]
        keys = torch.unique_consecutive(torch.sort((users << 31) + self.pos.to(torch.int64)[ids]).values)
        offsets = torch.zeros(lists.U + 1, dtype=torch.int64, device=keys.device)
        offsets[1:] = torch.cumsum(torch.bincount(keys >> 31, minlength=lists.U), 0)
        return ExclusionLists.from_sorted(offsets, keys & ((1 << 31) - 1))

    def by_position(self, lists):
        """The lists transposed BY POSITION, which nr_score_expect_news_groups takes (include/nrhip.h, K22): (offsets int32
        [n_pos + 1], users int32 [nnz]), for position p the ascending 0-based indices of the users whose list holds order[p] =
        users[offsets[p] : offsets[p + 1]].  ExclusionLists.by_news with the ids mapped through `pos`; ids outside [1, V) are
        dropped.  One sort of the keys position * 2^31 + user, bincount -> offsets.  The last result is kept with the lists (as
        by_news keeps its own), so the calls of one batch of users over one order transpose once."""
        kept = getattr(lists, "_by_position", None)
        if kept is not None and kept[0] is self and kept[1] is lists.offsets and kept[2] is lists.ids:
            return kept[3]
        users, ids = lists._pairs()
        keep = (ids >= 1) & (ids < self.V)
        users, ids = users[keep], ids[keep]
        keys = torch.unique_consecutive(torch.sort((self.pos.to(torch.int64)[ids] << 31) + users).values)
        offsets = torch.zeros(self.n_pos + 1, dtype=torch.int64, device=keys.device)
        offsets[1:] = torch.cumsum(torch.bincount(keys >> 31, minlength=self.n_pos), 0)
        out = offsets.to(torch.int32), (keys & ((1 << 31) - 1)).to(torch.int32)
        lists._by_position = (self, lists.offsets, lists.ids, out)
        return out


def _groups_arg(what, groups, V, dev):
    if not isinstance(groups, GroupOrder):
        raise RuntimeError(f"{what}: groups must be an ops.GroupOrder, got {type(groups)}")
    if groups.V != V or groups.device != dev:
        raise RuntimeError(f"{what}: the GroupOrder was built for V = {groups.V} news on {groups.device}, the call has V = {V} on {dev}")
    return groups


@torch.no_grad()
def score_logz_groups(news_vecs, user_vecs, temperature, groups, exclude=None, splits=0, prior=None, stamp=None, window=None):
    """Per-group log-partition (nr_score_logz_groups; include/nrhip.h, K15): score_logz per (user, bin) -- bins 0 .. n_groups - 1
    are the groups of `groups` (an ops.GroupOrder, built once per corpus), bin n_groups is "no group".  Same score bits, pools and
    lists as score_topk / score_sample / score_logz; no [U, V] score matrix.  Returns (logsum fp32, gmax fp32, count int32), each
    [U, n_groups + 1]: gmax is the bin's largest eligible score, count its eligible news, logsum = log sum exp((score - gmax) /
    temperature) >= 0 over the bin; an empty bin gives (-inf, -inf, 0).  exp(gmax / temperature + logsum - log Z) is the bin's
    share of the user's exposure under score_sample; ops.row_logprob_capped builds the propensity of a capped row on these.
    `temperature`, `exclude` (ids; mapped to positions here), `splits` (at most groups.nseg) and the pools are score_logz's; a bad
    entry of a temperature tensor gives that user NaN logsums only.  The three results do not depend, bit for bit, on `splits` or
    on which users share the call."""
    tau_t = temperature if isinstance(temperature, torch.Tensor) else None
    V, N, U, dev = _vector_args("score_logz_groups", news_vecs, user_vecs)
    gr = _groups_arg("score_logz_groups", groups, V, dev)                   # shapes first: these refusals need no GPU
    _need_gpu(news_vecs, user_vecs, exclude.ids if isinstance(exclude, ExclusionLists) else exclude, prior, stamp, window, tau_t, gr.order)
    B = gr.n_groups + 1
    logsum = torch.empty(U, B, dtype=torch.float32, device=dev)
    gmax = torch.empty(U, B, dtype=torch.float32, device=dev)
    count = torch.empty(U, B, dtype=torch.int32, device=dev)
    if U == 0:
        return logsum, gmax, count
    if isinstance(exclude, torch.Tensor):
        if exclude.dim() != 2 or exclude.shape[0] != U:
            raise RuntimeError(f"score_logz_groups: exclude must be [U = {U}, E], got {tuple(exclude.shape)}")
        exclude = ExclusionLists(exclude)
    if isinstance(exclude, ExclusionLists) and exclude.U == U and exclude.device == dev:
        exclude = gr.positions(exclude)
    ex_fields, ex_keep = _exclude_args("score_logz_groups", exclude, U, dev, dense=False)
    pr, st, win = _pool_args("score_logz_groups", V, U, dev, prior, stamp, window)
    tau, tau_u = _tau_args("score_logz_groups", temperature, U, dev)
    d = _lib.LogzGroupsDesc(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, user=ptr(user_vecs),
                            ld_user=user_vecs.stride(0) if U > 1 else N, U=U, N=N, splits=int(splits), **ex_fields, tau=tau, tau_u=ptr(tau_u),
                            order=ptr(gr.order), n_pos=gr.n_pos, seg_start=ptr(gr.seg_start), nseg=gr.nseg, bin_seg=ptr(gr.bin_seg),
                            n_groups=gr.n_groups, out_logsum=ptr(logsum), out_max=ptr(gmax), out_count=ptr(count),
                            prior=ptr(pr), stamp=ptr(st), window=ptr(win), ld_window=2 if win is not None else 0)
    ws = _ws(_lib.lib().nr_score_logz_groups_workspace_bytes(C.byref(d)), dev)      # 0 for a bad descriptor: the call below says why
    d.ws, d.ws_bytes = ptr(ws) if ws.numel() else None, ws.numel() * 4
    check(_lib.lib().nr_score_logz_groups(C.byref(d), _stream()), "nr_score_logz_groups")
    return logsum, gmax, count


@torch.no_grad()
def row_logprob_capped(news_vecs, user_vecs, row_ids, temperature, bases, group, group_cap, n_groups=None, prior=None, stamp=None,
                       window=None):
    """Log-probabilities of the entries of rows drawn under group caps (nr_row_logprob_capped; include/nrhip.h, K16): the law of
    score_sample(..., group, group_cap) -- at step j the candidates are the eligible news not yet taken whose group has fewer
    than group_cap entries in the row so far.  `row_ids`: integer tensor [U, k <= 128], 0 (or anything outside [1, V)) = fill.
    `bases` = (logsum, gmax), each [U, n_groups + 1] -- the first two results of score_logz_groups computed with the row merged
    into `exclude` (a third element, the count, is ignored).  `group` int32 [V] on the device, `group_cap` in [1, 128]; n_groups
    None = the width of the bases - 1.
    Returns (logp fp32 [U, k], total fp32 [U] = the row's sum, formed in fp64).  Fill entries give 0; an entry outside the pool
    or with a NaN score gives NaN, is part of no sum and uses up nothing of a cap; a bad entry of a temperature tensor gives its
    user's real entries NaN.  A live entry whose group already has group_cap live entries before it gives -inf -- the capped
    sampler never draws it; it uses up nothing of a cap, its weight still counts at every earlier step at which its group was
    open, and the total is -inf.  Repeats and membership in the lists are the caller's statement."""
    tau_t = temperature if isinstance(temperature, torch.Tensor) else None
    V, N, U, dev = _vector_args("row_logprob_capped", news_vecs, user_vecs)
    if row_ids.dim() != 2 or row_ids.shape[0] != U or row_ids.is_floating_point() or row_ids.device != dev:
        raise RuntimeError(f"row_logprob_capped: row_ids must be an integer tensor [U = {U}, k] on {dev}, got {tuple(row_ids.shape)} "
                           f"{row_ids.dtype} on {row_ids.device}")
    k = row_ids.shape[1]
    bl, bm = bases[0], bases[1]
    G = int(n_groups) if n_groups is not None else (bl.shape[1] - 1 if isinstance(bl, torch.Tensor) and bl.dim() == 2 else 0)
    for name, t in (("base logsum", bl), ("base gmax", bm)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (U, G + 1) or not t.is_floating_point() or t.device != dev:
            raise RuntimeError(f"row_logprob_capped: {name} must be a floating point tensor of shape ({U}, n_groups + 1 = {G + 1}) on {dev}, "
                               f"got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
    gr = _group_args("row_logprob_capped", group, V, dev)
    _need_gpu(news_vecs, user_vecs, row_ids, prior, stamp, window, tau_t, bl, bm, gr)      # after the shapes: those refusals need no GPU
    logp = torch.empty(U, k, dtype=torch.float32, device=dev)
    total = torch.empty(U, dtype=torch.float32, device=dev)
    if U == 0:
        return logp, total
    bl, bm = bl.detach().to(torch.float32).contiguous(), bm.detach().to(torch.float32).contiguous()
    ids = row_ids.detach().to(torch.int32).contiguous()
    pr, st, win = _pool_args("row_logprob_capped", V, U, dev, prior, stamp, window)
    tau, tau_u = _tau_args("row_logprob_capped", temperature, U, dev)
    d = _lib.LogprobCappedDesc(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, user=ptr(user_vecs),
                               ld_user=user_vecs.stride(0) if U > 1 else N, U=U, N=N, k=k, row_ids=ptr(ids), ld_ids=k, group=ptr(gr),
                               group_cap=int(group_cap), n_groups=G, tau=tau, tau_u=ptr(tau_u), base_max=ptr(bm), base_logsum=ptr(bl),
                               ld_base=G + 1, out_logp=ptr(logp), out_total=ptr(total), prior=ptr(pr), stamp=ptr(st), window=ptr(win),
                               ld_window=2 if win is not None else 0)
    check(_lib.lib().nr_row_logprob_capped(C.byref(d), _stream()), "nr_row_logprob_capped")
    return logp, total


def _bin_args(what, bases, bin_w, U, B, dev):
    """(logsum, gmax, omega) as contiguous fp32 [U, B] tensors: the first two results of score_logz_groups and the weights."""
    out = []
    for name, t in (("base logsum", bases[0]), ("base gmax", bases[1]), ("bin_w", bin_w)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (U, B) or not t.is_floating_point() or t.device != dev:
            raise RuntimeError(f"{what}: {name} must be a floating point tensor of shape ({U}, n_groups + 1 = {B}) on {dev}, "
                               f"got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
        out.append(t.detach().to(torch.float32).contiguous())
    return out


def _score_expect_groups(what, news_vecs, user_vecs, temperature, groups, bases, bin_w, exclude, splits, prior, stamp, window, sub_ids, sub_w,
                         scale_inv_tau):
    """One nr_score_expect_groups call (include/nrhip.h, K20): (out [U, N] fp32, mass [U] fp32).  `exclude` holds ids and is
    mapped to positions here, as in score_logz_groups."""
    tau_t = temperature if isinstance(temperature, torch.Tensor) else None
    V, N, U, dev = _vector_args(what, news_vecs, user_vecs)
    gr = _groups_arg(what, groups, V, dev)                                  # shapes first: these refusals need no GPU
    bl, bm, om = _bin_args(what, bases, bin_w, U, gr.n_groups + 1, dev)
    T = 0
    if sub_ids is not None:
        if sub_ids.dim() != 2 or sub_ids.shape[0] != U or sub_ids.is_floating_point() or tuple(sub_w.shape) != tuple(sub_ids.shape):
            raise RuntimeError(f"{what}: the named rows must be integer ids [U = {U}, T] with weights of the same shape")
        T = sub_ids.shape[1]
        sub_ids = sub_ids.detach().to(torch.int32).contiguous()
        sub_w = sub_w.detach().to(torch.float32).contiguous()
    _need_gpu(news_vecs, user_vecs, exclude.ids if isinstance(exclude, ExclusionLists) else exclude, prior, stamp, window, tau_t, gr.order, bl, bm, om,
              sub_ids, sub_w)
    out = torch.empty(U, N, dtype=torch.float32, device=dev)
    mass = torch.empty(U, dtype=torch.float32, device=dev)
    if U == 0:
        return out, mass
    if isinstance(exclude, torch.Tensor):
        if exclude.dim() != 2 or exclude.shape[0] != U:
            raise RuntimeError(f"{what}: exclude must be [U = {U}, E], got {tuple(exclude.shape)}")
        exclude = ExclusionLists(exclude)
    if isinstance(exclude, ExclusionLists) and exclude.U == U and exclude.device == dev:
        exclude = gr.positions(exclude)
    ex_fields, ex_keep = _exclude_args(what, exclude, U, dev, dense=False)
    pr, st, win = _pool_args(what, V, U, dev, prior, stamp, window)
    tau, tau_u = _tau_args(what, temperature, U, dev)
    B = gr.n_groups + 1
    d = _lib.ExpectGroupsDesc(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, user=ptr(user_vecs),
                              ld_user=user_vecs.stride(0) if U > 1 else N, U=U, N=N, splits=int(splits), **ex_fields, tau=tau, tau_u=ptr(tau_u),
                              order=ptr(gr.order), n_pos=gr.n_pos, seg_start=ptr(gr.seg_start), nseg=gr.nseg, bin_seg=ptr(gr.bin_seg),
                              n_groups=gr.n_groups, base_max=ptr(bm), base_logsum=ptr(bl), bin_w=ptr(om), ld_base=B, sub_ids=ptr(sub_ids),
                              sub_w=ptr(sub_w), ld_sub=T, T=T, scale_inv_tau=1 if scale_inv_tau else 0, out=ptr(out), ld_out=N, out_mass=ptr(mass),
                              prior=ptr(pr), stamp=ptr(st), window=ptr(win), ld_window=2 if win is not None else 0)
    ws = _ws(_lib.lib().nr_score_expect_groups_workspace_bytes(C.byref(d)), dev)    # 0 for a bad descriptor: the call below says why
    d.ws, d.ws_bytes = ptr(ws) if ws.numel() else None, ws.numel() * 4
    check(_lib.lib().nr_score_expect_groups(C.byref(d), _stream()), "nr_score_expect_groups")
    return out, mass


@torch.no_grad()
def score_expect_groups(news_vecs, user_vecs, temperature, groups, bases, bin_w, exclude=None, splits=0, prior=None, stamp=None, window=None):
    """The expected news vector per bin under per-(user, bin) weights (nr_score_expect_groups; include/nrhip.h, K20): per user
    sum_b bin_w[u, b] E_b, E_b = sum_{v in bin b} p_b(v) news_vecs[v], p_b(v) = exp((score_v - gmax_b) / temperature - logsum_b)
    the softmax INSIDE bin b -- the gradient of score_logz_groups' per-group partitions with respect to the user vector, without
    the [U, V] matrix.  `groups`: the ops.GroupOrder of the corpus; `bases` = (logsum, gmax[, count]): what score_logz_groups
    returned for the SAME vectors, temperature, exclude and pools; `bin_w`: floating point [U, n_groups + 1].  The other
    arguments are score_logz_groups' (`exclude` holds ids; `splits` at most groups.nseg).
    Returns (expect fp32 [U, N], mass fp32 [U]): mass = sum_b bin_w_b sum_v p_b(v), up to rounding the sum of bin_w over the
    non-empty bins.  A bin with bin_w == 0 contributes exactly nothing whatever its base holds, and so does an empty bin.  A user
    with a non-empty bin and a bad entry of a temperature tensor, or with a non-empty bin of weight != 0 whose base is NaN (or
    gmax +inf) or whose weight is not finite, gets NaN.  For a fixed splits > 0 a user's row does not depend, bit for bit, on
    the other users of the call; across different splits rows agree to within the bound of DESIGN.md section 5."""
    return _score_expect_groups("score_expect_groups", news_vecs, user_vecs, temperature, groups, bases, bin_w, exclude, splits, prior, stamp,
                                window, None, None, False)


@torch.no_grad()
def row_logprob_capped_grad(news_vecs, user_vecs, row_ids, temperature, bases, group, group_cap, n_groups=None, g=None, prior=None, stamp=None,
                            window=None):
    """The gradient coefficients of rows drawn under group caps (nr_row_logprob_capped_grad; include/nrhip.h, K21): the backward
    of row_logprob_capped.  `row_ids`, `temperature`, `bases`, `group`, `group_cap`, `n_groups` and the pools are
    row_logprob_capped's, the bases formed WITHOUT the row's ids; `g`: optional floating point [U, k], the upstream gradient of
    nll_j = -logp_j per entry (None = 1).
    Returns (bin_w fp32 [U, n_groups + 1], sub_w fp32 [U, k]) = (omega, c) with
      d (sum_j g_j nll_j) / d user = (sum_b omega_b E_b - sum_i c_i news_vecs[row_i]) / temperature,
    E_b the expected news vector inside bin b over what the bases sum over: nr_score_expect_groups with bin_w = omega, the row
    and c as its named rows and the lists of the bases' score_logz_groups call.  Fill entries and entries outside the pool or
    with a NaN score get c = 0 and their g is not read; an entry whose group was already full (logp -inf) is no step either, its
    g is not read, and its c = -w_i Q is the pull of the earlier steps at which its group was open.  A user with a bad
    temperature entry or a NaN base gets zeros; an empty bin gets omega = 0.  sum_b omega_b = sum_i c_i up to rounding."""
    tau_t = temperature if isinstance(temperature, torch.Tensor) else None
    V, N, U, dev = _vector_args("row_logprob_capped_grad", news_vecs, user_vecs)
    if row_ids.dim() != 2 or row_ids.shape[0] != U or row_ids.is_floating_point() or row_ids.device != dev:
        raise RuntimeError(f"row_logprob_capped_grad: row_ids must be an integer tensor [U = {U}, k] on {dev}, got {tuple(row_ids.shape)} "
                           f"{row_ids.dtype} on {row_ids.device}")
    k = row_ids.shape[1]
    bl, bm = bases[0], bases[1]
    G = int(n_groups) if n_groups is not None else (bl.shape[1] - 1 if isinstance(bl, torch.Tensor) and bl.dim() == 2 else 0)
    for name, t in (("base logsum", bl), ("base gmax", bm)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (U, G + 1) or not t.is_floating_point() or t.device != dev:
            raise RuntimeError(f"row_logprob_capped_grad: {name} must be a floating point tensor of shape ({U}, n_groups + 1 = {G + 1}) on "
                               f"{dev}, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
    if g is not None and (not isinstance(g, torch.Tensor) or tuple(g.shape) != (U, k) or not g.is_floating_point() or g.device != dev):
        raise RuntimeError(f"row_logprob_capped_grad: g must be a floating point tensor of shape ({U}, {k}) on {dev}")
    gr = _group_args("row_logprob_capped_grad", group, V, dev)
    _need_gpu(news_vecs, user_vecs, row_ids, prior, stamp, window, tau_t, bl, bm, gr, g)   # after the shapes: those refusals need no GPU
    bin_w = torch.empty(U, G + 1, dtype=torch.float32, device=dev)
    sub_w = torch.empty(U, k, dtype=torch.float32, device=dev)
    if U == 0:
        return bin_w, sub_w
    if g is not None:
        g = g.detach().to(torch.float32).contiguous()
    bl, bm = bl.detach().to(torch.float32).contiguous(), bm.detach().to(torch.float32).contiguous()
    ids = row_ids.detach().to(torch.int32).contiguous()
    pr, st, win = _pool_args("row_logprob_capped_grad", V, U, dev, prior, stamp, window)
    tau, tau_u = _tau_args("row_logprob_capped_grad", temperature, U, dev)
    d = _lib.LogprobCappedGradDesc(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, user=ptr(user_vecs),
                                   ld_user=user_vecs.stride(0) if U > 1 else N, U=U, N=N, k=k, row_ids=ptr(ids), ld_ids=k, group=ptr(gr),
                                   group_cap=int(group_cap), n_groups=G, tau=tau, tau_u=ptr(tau_u), base_max=ptr(bm), base_logsum=ptr(bl),
                                   ld_base=G + 1, g=ptr(g), ld_g=k if g is not None else 0, out_bin_w=ptr(bin_w), out_sub_w=ptr(sub_w),
                                   prior=ptr(pr), stamp=ptr(st), window=ptr(win), ld_window=2 if win is not None else 0)
    check(_lib.lib().nr_row_logprob_capped_grad(C.byref(d), _stream()), "nr_row_logprob_capped_grad")
    return bin_w, sub_w


class CappedPlackettLuceNLLFunction(Function):
    """nll [U, k] of the places of rows drawn under group caps, differentiable with respect to the user vectors (K21, then one
    K20 call).  The news side is CappedPlackettLuceNLLJointFunction's: plackett_luce_nll_capped refuses a table that requires grad."""

    @staticmethod
    def forward(ctx, user_vecs, news_vecs, rows, temperature, groups, group, group_cap, exclude, splits, prior, stamp, window):
        user, news = user_vecs.detach(), news_vecs.detach()
        V = news.shape[0]
        taken = ExclusionLists(rows)
        if exclude is None:
            lists = taken
        else:
            lists = (exclude if isinstance(exclude, ExclusionLists) else ExclusionLists(exclude)).merged(taken)
        bases = score_logz_groups(news, user, temperature, groups, exclude=lists, splits=splits, prior=prior, stamp=stamp, window=window)
        logp, _ = row_logprob_capped(news, user, rows, temperature, bases, group, group_cap, n_groups=groups.n_groups, prior=prior, stamp=stamp,
                                     window=window)
        valid = (rows >= 1) & (rows < V) & torch.isfinite(logp)              # NaN: outside the pool; -inf: its group was full
        if isinstance(temperature, torch.Tensor):
            valid &= ((temperature > 0) & torch.isfinite(temperature))[:, None]
        nll = torch.where(valid, -logp, torch.zeros_like(logp))
        ctx.save_for_backward(user, news, rows, valid, bases[0], bases[1], group)
        ctx.rest = (temperature, groups, group_cap, lists, splits, prior, stamp, window)
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)
        return nll, valid

    @staticmethod
    def backward(ctx, g, _gvalid):
        user, news, rows, valid, bl, bm, group = ctx.saved_tensors
        temperature, groups, group_cap, lists, splits, prior, stamp, window = ctx.rest
        if g is None or not ctx.needs_input_grad[0]:
            return (None,) * 12
        gw = torch.where(valid, g.to(torch.float32), torch.zeros((), dtype=torch.float32, device=g.device))
        with torch.no_grad():
            om, c = row_logprob_capped_grad(news, user, rows, temperature, (bl, bm), group, group_cap, n_groups=groups.n_groups, g=gw, prior=prior,
                                            stamp=stamp, window=window)
            grad_user, _ = _score_expect_groups("plackett_luce_nll_capped", news, user, temperature, groups, (bl, bm), om, lists, splits, prior,
                                                stamp, window, rows, c, True)
            # a user none of whose places count (all fill or invalid, a bad temperature) has no gradient: exactly 0, not 0 * NaN
            grad_user = torch.where(valid.any(dim=1)[:, None], grad_user, torch.zeros_like(grad_user))
        return (grad_user,) + (None,) * 11


def plackett_luce_nll_capped(news_vecs, user_vecs, rows, temperature, groups, group, group_cap, exclude=None, splits=0, prior=None, stamp=None,
                             window=None):
    """The negative log-likelihood of ordered rows under the law score_sample(..., group, group_cap) draws from -- at every place
    the softmax over the eligible news not yet taken whose group has fewer than group_cap entries in the row so far -- with a
    gradient for `user_vecs`: the training-side counterpart of train.sample_propensity_capped.  rows: integer tensor
    [U, k <= 128], 0 (or anything outside [1, V)) = fill.  `groups`: the ops.GroupOrder of `group` (int32 [V] on the device).
    Forward: `rows` merged into `exclude`, score_logz_groups on those lists, row_logprob_capped -- what sample_propensity_capped
    launches, so nll[valid] = -logp of it, bit for bit.  Returns (nll fp32 [U, k], valid bool [U, k]): valid is False at fill
    entries, at entries row_logprob_capped gives NaN (outside the pool, a NaN score) or -inf (the entry's group was already
    full: the capped sampler cannot have drawn it) and for users whose temperature is not finite and > 0; nll is 0 there.
    Repeats within a row and entries inside `exclude` are the caller's statement (train.listwise_loss_capped turns them into fill).
    Backward: ONE nr_row_logprob_capped_grad call (include/nrhip.h, K21) with g zeroed where not valid gives (omega, c); then
    grad_user = (sum_b omega_b E_b - sum_i c_i news[row_i]) / temperature is ONE nr_score_expect_groups call (K20: bin_w omega,
    named rows (rows, c), the merged lists, the saved bases).  A user without a valid place gets an exactly zero row.
    `news_vecs` is a frozen table here: one that requires grad raises RuntimeError -- the news side of this gradient is the pass
    of plackett_luce_nll_capped_joint (nr_score_expect_news_groups, K22); use that.  Temperature, prior and the rest get no gradient."""
    if news_vecs.requires_grad:
        raise RuntimeError("plackett_luce_nll_capped: news_vecs requires grad, but the news side of the capped gradient is a missing pass "
                           "of this function (nr_score_expect_news with per-(user, bin) weights); it is not emulated: detach the table, or "
                           "use plackett_luce_nll_capped_joint")
    if rows.dim() != 2 or rows.shape[0] != user_vecs.shape[0] or rows.is_floating_point():
        raise RuntimeError(f"plackett_luce_nll_capped: rows must be an integer tensor [U = {user_vecs.shape[0]}, k], got {tuple(rows.shape)} "
                           f"{rows.dtype}")
    if rows.shape[1] < 1 or rows.shape[1] > _lib.NR_TOPK_MAX_K:
        raise RuntimeError(f"plackett_luce_nll_capped: k = {rows.shape[1]} places per row, must be in [1, {_lib.NR_TOPK_MAX_K}]: a sequential "
                           "row cannot be cut into chunks")
    if not 1 <= int(group_cap) <= 128:
        raise RuntimeError(f"plackett_luce_nll_capped: group_cap = {group_cap}, must be in [1, 128]")
    _groups_arg("plackett_luce_nll_capped", groups, news_vecs.shape[0], news_vecs.device)
    return CappedPlackettLuceNLLFunction.apply(user_vecs, news_vecs, rows, temperature, groups, group, group_cap, exclude, splits, prior, stamp,
                                               window)


def _score_expect_news_groups(what, news_vecs, user_vecs, temperature, groups, bases, bin_w, exclude, splits, prior, stamp, window, named,
                              scale_inv_tau):
    """One nr_score_expect_news_groups call (include/nrhip.h, K22): (out [V, N] fp32, mass [V] fp32).  `bases` / `bin_w` are
    user-major [U, n_groups + 1] and transposed here; `exclude` holds ids per user and goes through GroupOrder.by_position;
    named: None or (offsets int32 [V + 1], users int32 [n], w fp32 [n]) on the device."""
    tau_t = temperature if isinstance(temperature, torch.Tensor) else None
    V, N, U, dev = _vector_args(what, news_vecs, user_vecs)
    gr = _groups_arg(what, groups, V, dev)                                  # shapes first: these refusals need no GPU
    B = gr.n_groups + 1
    bl, bm, om = _bin_args(what, bases, bin_w, U, B, dev)
    if exclude is not None and not isinstance(exclude, ExclusionLists):
        if not isinstance(exclude, torch.Tensor) or exclude.dim() != 2 or exclude.shape[0] != U:
            raise RuntimeError(f"{what}: exclude must be a tensor [U = {U}, E] or an ExclusionLists")
        exclude = ExclusionLists(exclude)
    if exclude is not None and (exclude.U != U or exclude.device != dev):
        raise RuntimeError(f"{what}: the exclusion lists are for {exclude.U} users on {exclude.device}, the call has {U} on {dev}")
    n_off = n_user = n_w = None
    if named is not None:
        n_off, n_user, n_w = named
        if tuple(n_off.shape) != (V + 1,) or n_user.dim() != 1 or tuple(n_w.shape) != tuple(n_user.shape):
            raise RuntimeError(f"{what}: the named terms must be offsets [V + 1 = {V + 1}] with users and weights of one length")
    _need_gpu(news_vecs, user_vecs, exclude.ids if exclude is not None else None, prior, stamp, window, tau_t, gr.order, bl, bm, om,
              *(named or ()))
    if U == 0:                                                 # nobody: zeros, nothing to launch
        return torch.zeros(V, N, dtype=torch.float32, device=dev), torch.zeros(V, dtype=torch.float32, device=dev)
    out = torch.empty(V, N, dtype=torch.float32, device=dev)   # the finalize writes every row
    mass = torch.empty(V, dtype=torch.float32, device=dev)
    # bin-major [n_groups + 1, U]: a wave's 64 lanes then read 64 consecutive floats of their users for the tile's bin
    bl, bm, om = bl.t().contiguous(), bm.t().contiguous(), om.t().contiguous()
    ex_off = ex_users = None
    if exclude is not None:
        ex_off, ex_users = gr.by_position(exclude)
    n_excl = 0 if ex_users is None else ex_users.numel()
    if named is not None:
        n_off, n_user, n_w = n_off.to(torch.int32).contiguous(), n_user.to(torch.int32).contiguous(), n_w.detach().to(torch.float32).contiguous()
        if n_user.numel() == 0:
            n_off = n_user = n_w = None
    pr, st, win = _pool_args(what, V, U, dev, prior, stamp, window)
    tau, tau_u = _tau_args(what, temperature, U, dev)
    d = _lib.ExpectNewsGroupsDesc(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, user=ptr(user_vecs),
                                  ld_user=user_vecs.stride(0) if U > 1 else N, U=U, N=N, splits=int(splits),
                                  excl_offsets=ptr(ex_off) if n_excl else None, excl_users=ptr(ex_users) if n_excl else None, n_excl=n_excl,
                                  tau=tau, tau_u=ptr(tau_u), order=ptr(gr.order), n_pos=gr.n_pos, bin_start=ptr(gr.bin_start),
                                  n_groups=gr.n_groups, base_max=ptr(bm), base_logsum=ptr(bl), bin_w=ptr(om), ld_bin=U,
                                  scale_inv_tau=1 if scale_inv_tau else 0, named_offsets=ptr(n_off), named_user=ptr(n_user), named_w=ptr(n_w),
                                  n_named=0 if n_user is None else n_user.numel(), out=ptr(out), ld_out=N, out_mass=ptr(mass),
                                  prior=ptr(pr), stamp=ptr(st), window=ptr(win), ld_window=2 if win is not None else 0)
    ws = _ws(_lib.lib().nr_score_expect_news_groups_workspace_bytes(C.byref(d)), dev)     # 0 for a bad descriptor: the call below says why
    d.ws, d.ws_bytes = ptr(ws) if ws.numel() else None, ws.numel() * 4
    check(_lib.lib().nr_score_expect_news_groups(C.byref(d), _stream()), "nr_score_expect_news_groups")
    return out, mass


@torch.no_grad()
def score_expect_news_groups(news_vecs, user_vecs, temperature, groups, bases, bin_w, exclude=None, splits=0, prior=None, stamp=None, window=None):
    """The news side of score_expect_groups (nr_score_expect_news_groups; include/nrhip.h, K22): per news
    D_v = sum_u bin_w[u, bin(v)] p_bin(v)(v | u) user_vecs[u], p_b(v | u) = exp((score_uv - gmax_ub) / temperature - logsum_ub) the
    softmax INSIDE the news' bin, over exactly the pairs score_logz_groups sums over -- the gradient of sum_u sum_b bin_w[u, b]
    temperature log Z_ub with respect to the news vector -- without the [U, V] matrix.  `groups`, `bases` = (logsum, gmax[, count])
    and `bin_w` are score_expect_groups': user-major [U, n_groups + 1] (transposed inside, once per call); `exclude` is PER USER, in
    ids, as everywhere (it goes through GroupOrder.by_position); the pools are score_logz_groups'.
    Returns (out fp32 [V, N], mass fp32 [V]): mass[v] = sum_u bin_w[u, bin(v)] p_bin(v)(v | u).  A (user, bin) pair whose temperature
    is not finite and > 0, whose base is NaN or infinite (an empty bin: gmax = -inf) or whose weight is 0, NaN or infinite
    contributes nothing and leaves no NaN -- unlike score_expect_groups, which gives such a user a NaN row: here one NaN would
    reach every row of the table.  Row 0 is zeros.
    `splits`: 0 = the library chooses the number of USER slices by V (at most the user segments of K18's plan).  For a fixed
    splits > 0 a row's bits do not depend on the other news, on its place in its bin's run, or on the sizes of the other bins;
    across different splits rows agree within the bound of DESIGN.md section 5."""
    return _score_expect_news_groups("score_expect_news_groups", news_vecs, user_vecs, temperature, groups, bases, bin_w, exclude, splits, prior,
                                     stamp, window, None, False)


class CappedPlackettLuceNLLJointFunction(Function):
    """nll [U, k] of the places of rows drawn under group caps, differentiable with respect to the user vectors (K21, then one
    K20 call) and the news-vector table (the same K21 call's coefficients, then one K22 call)."""

    @staticmethod
    def forward(ctx, user_vecs, news_vecs, rows, temperature, groups, group, group_cap, exclude, splits, prior, stamp, window):
        return CappedPlackettLuceNLLFunction.forward(ctx, user_vecs, news_vecs, rows, temperature, groups, group, group_cap, exclude, splits,
                                                     prior, stamp, window)

    @staticmethod
    def backward(ctx, g, _gvalid):
        user, news, rows, valid, bl, bm, group = ctx.saved_tensors
        temperature, groups, group_cap, lists, splits, prior, stamp, window = ctx.rest
        if g is None or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 12
        gw = torch.where(valid, g.to(torch.float32), torch.zeros((), dtype=torch.float32, device=g.device))
        grad_user = grad_news = None
        with torch.no_grad():
            # ONE K21 call for both sides: omega per (user, bin), c per entry
            om, c = row_logprob_capped_grad(news, user, rows, temperature, (bl, bm), group, group_cap, n_groups=groups.n_groups, g=gw, prior=prior,
                                            stamp=stamp, window=window)
            if ctx.needs_input_grad[0]:
                grad_user, _ = _score_expect_groups("plackett_luce_nll_capped_joint", news, user, temperature, groups, (bl, bm), om, lists, splits, prior,
                                                    stamp, window, rows, c, True)
                # a user none of whose places count (all fill or invalid, a bad temperature) has no gradient: exactly 0, not 0 * NaN
                grad_user = torch.where(valid.any(dim=1)[:, None], grad_user, torch.zeros_like(grad_user))
            if ctx.needs_input_grad[1]:
                # K22 takes the user slices by its own plan: `splits` is K15's / K20's cut of the order and does not apply
                grad_news, _ = _score_expect_news_groups("plackett_luce_nll_capped_joint", news, user, temperature, groups, (bl, bm), om, lists, 0,
                                                         prior, stamp, window, _named_by_news(rows, c, news.shape[0]), True)
        return (grad_user, grad_news) + (None,) * 10


def plackett_luce_nll_capped_joint(news_vecs, user_vecs, rows, temperature, groups, group, group_cap, exclude=None, splits=0, prior=None,
                                   stamp=None, window=None):
    """plackett_luce_nll_capped, differentiable with respect to `user_vecs` AND the table `news_vecs`: either may require grad.
    The forward is plackett_luce_nll_capped's (the rows merged into `exclude`, score_logz_groups, row_logprob_capped), bit for
    bit, and returns (nll fp32 [U, k], valid bool [U, k]) as it does.  Backward: ONE nr_row_logprob_capped_grad call (K21) gives
    (omega, c) for both sides; grad_user is plackett_luce_nll_capped's single nr_score_expect_groups call (K20), bit for bit;
    grad_news [V, N] is ONE nr_score_expect_news_groups call (include/nrhip.h, K22) with bin_w = omega, the 1 / temperature scale
    inside, the merged lists, the saved bases, and the row's entries with their c as its named terms (stable sort by news id;
    entries with c = 0 and fill dropped):
      grad_news[v] = sum_u omega[u, bin(v)] / tau_u p_bin(v)(v | u) user_u  -  sum_{(u, i): row_ui = v} c_ui / tau_u user_u.
    A named term does not depend on its bin's base: a bin the row emptied still receives its entries' terms.  News that are
    eligible for nobody and named by nobody get an exactly zero row; row 0 always.  A pass whose input does not require grad is
    not launched (neither requires grad: K21 is not launched either).  Temperature, prior and the other arguments get no gradient."""
    if rows.dim() != 2 or rows.shape[0] != user_vecs.shape[0] or rows.is_floating_point():
        raise RuntimeError(f"plackett_luce_nll_capped_joint: rows must be an integer tensor [U = {user_vecs.shape[0]}, k], got {tuple(rows.shape)} "
                           f"{rows.dtype}")
    if rows.shape[1] < 1 or rows.shape[1] > _lib.NR_TOPK_MAX_K:
        raise RuntimeError(f"plackett_luce_nll_capped_joint: k = {rows.shape[1]} places per row, must be in [1, {_lib.NR_TOPK_MAX_K}]: a "
                           "sequential row cannot be cut into chunks")
    if not 1 <= int(group_cap) <= 128:
        raise RuntimeError(f"plackett_luce_nll_capped_joint: group_cap = {group_cap}, must be in [1, 128]")
    _groups_arg("plackett_luce_nll_capped_joint", groups, news_vecs.shape[0], news_vecs.device)
    return CappedPlackettLuceNLLJointFunction.apply(user_vecs, news_vecs, rows, temperature, groups, group, group_cap, exclude, splits, prior,
                                                    stamp, window)


@torch.no_grad()
def mmr_select(news_vecs, pool_ids, pool_scores, k, penalty, group=None, group_cap=None):
    """Diversified re-ranking of a pool (nr_mmr_select; include/nrhip.h, K11): Maximal Marginal Relevance over the M places of
    every user's pool -- `pool_ids` int32 [U, M] and `pool_scores` fp32 [U, M], M <= 128, what score_topk(k=M) returns, but any
    arrays are allowed.  The row is built greedily: the first entry is the best pool score, every later one the live place not
    yet taken with the largest fmaf(-penalty, max cosine to what is already in the row, pool score); ties go to the lowest
    place.  The cosines come from `news_vecs` in exact fp32 (one Gram matrix per user on the matrix cores, never in HBM).
    `penalty`: a float (finite, >= 0) or a fp32 tensor [U], one penalty per user; 0 gives the pool's own order.
    `group` [V] int32 with `group_cap` = c in [1, 128], together: at most c places of one group in a row (negative = in no
    group), applied inside the walk.  A place whose id is outside [1, V) or whose score is NaN (score_topk's fill) is never taken.
    Returns (ids int32 [U, k], scores fp32 [U, k] -- the pool scores of the places taken, not the MMR values -- and place int32
    [U, k], the 0-based places in the pool); a row with fewer than k places to take ends in id 0, score -inf, place -1."""
    pen_t = penalty if isinstance(penalty, torch.Tensor) else None
    _need_gpu(news_vecs, pool_ids, pool_scores, pen_t, group)
    if news_vecs.dim() != 2 or news_vecs.dtype != torch.float32 or news_vecs.stride(1) != 1 or (news_vecs.shape[0] > 1 and news_vecs.stride(0) < news_vecs.shape[1]):
        raise RuntimeError(f"mmr_select: news_vecs must be a 2-D fp32 tensor with contiguous rows, got {tuple(news_vecs.shape)} {news_vecs.dtype} "
                           f"strides {tuple(news_vecs.stride())}")
    V, N = news_vecs.shape
    dev = news_vecs.device
    for name, t, dt in (("pool_ids", pool_ids, torch.int32), ("pool_scores", pool_scores, torch.float32)):
        if t.dim() != 2 or t.dtype != dt or t.device != dev or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
            raise RuntimeError(f"mmr_select: {name} must be a 2-D {dt} tensor with contiguous rows on {dev}, got {tuple(t.shape)} {t.dtype} "
                               f"strides {tuple(t.stride())} on {t.device}")
    U, M = pool_ids.shape
    if tuple(pool_scores.shape) != (U, M):
        raise RuntimeError(f"mmr_select: pool_ids is {tuple(pool_ids.shape)}, pool_scores {tuple(pool_scores.shape)}")
    pen = None
    if pen_t is not None:
        if tuple(pen_t.shape) != (U,) or not pen_t.is_floating_point() or pen_t.device != dev:
            raise RuntimeError(f"mmr_select: a penalty tensor must be floating point of shape ({U},) on {dev}, got {tuple(pen_t.shape)} "
                               f"{pen_t.dtype} on {pen_t.device}")
        pen = pen_t.detach().to(torch.float32).contiguous()
    gr = _group_args("mmr_select", group, V, dev)
    ids = torch.empty(U, int(k), dtype=torch.int32, device=dev)
    scores = torch.empty(U, int(k), dtype=torch.float32, device=dev)
    place = torch.empty(U, int(k), dtype=torch.int32, device=dev)
    if U == 0:
        return ids, scores, place
    d = _lib.MmrDesc(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, pool_ids=ptr(pool_ids),
                     pool_scores=ptr(pool_scores), ld_pool_ids=pool_ids.stride(0) if U > 1 else M,
                     ld_pool_scores=pool_scores.stride(0) if U > 1 else M, U=U, N=N, M=M, k=int(k),
                     penalty=0.0 if pen is not None else float(penalty), penalty_u=ptr(pen), group=ptr(gr),
                     group_cap=0 if group_cap is None else int(group_cap), out_ids=ptr(ids), out_scores=ptr(scores), out_place=ptr(place))
    check(_lib.lib().nr_mmr_select(C.byref(d), _stream()), "nr_mmr_select")
    return ids, scores, place


@torch.no_grad()
def score_rank(news_vecs, user_vecs, targets, exclude=None, ks=(), splits=0, prior=None, stamp=None, window=None):
    """Full-corpus rank evaluation (nr_score_rank): for every user and each of its targets ([U, T <= 64] news ids, 0 = no entry)
    the exact 1-based position of that news among the user's eligible news of the whole table, in score_topk's order and with
    score_topk's score bits: 1 <= rank <= k exactly when the target is in the user's top-k row.  Rank 0, score -inf: the target
    is 0 or out of range, is in `exclude` ([U, E <= 64]; wider, or an ExclusionLists of any length: the CSR lists, as in
    score_topk), has a NaN score or repeats an earlier entry of its row.  No [U, V]
    score matrix is formed.  Returns (ranks int32 [U, T], scores fp32 [U, T], sums): with cut-offs `ks` (at most 8) sums is a
    DEVICE fp64 tensor [2 + 2 len(ks)] = [users with a ranked target, sum MRR_u, then per k: sum Recall@k_u, sum nDCG@k_u]
    (metrics.retrieval_metrics_reference states the per-user terms); with ks=None no sums are formed and None is returned.
    `splits`: 0 = the library chooses the number of corpus slices; tests force it.
    Pools: `prior`, `stamp`, `window` as in score_topk, with the same score fl32(dot + prior) and the same eligible news, so the
    agreement with score_topk's rows holds for equal pool inputs.  A target outside its user's pool has rank 0, score -inf.
    This call knows no group caps and describes the uncapped ranking; score_rank_capped ranks in the capped one."""
    return _score_rank(news_vecs, user_vecs, targets, exclude, ks, splits, prior, stamp, window, None, None, None)


@torch.no_grad()
def score_rank_capped(news_vecs, user_vecs, targets, group, group_cap, n_groups=None, exclude=None, ks=(), splits=0, prior=None, stamp=None,
                      window=None):
    """score_rank under the group caps of score_topk (include/nrhip.h, K10): `group` [V] int32 on the device and `group_cap` = c as
    in score_topk -- the rank is the place in the capped ranking score_topk(..., group, group_cap) serves: 1 <= rank <= k exactly
    when the target is at place rank - 1 of that row, same score bits.  A target that ranking never shows, because c better
    news of its own group stand in front of it, has rank -1 and keeps its score; in the sums it counts in n_u and adds nothing
    else.  What is not ranked by score_rank stays at rank 0, score -inf.  At most 4 targets per row
    (_lib.NR_RANK_MAX_CAPPED_TARGETS); train.rank_eval_capped lays wider users over several rows.
    `n_groups`: the group ids lie in [0, n_groups), at most 512; None takes group.max() + 1 from the device, which is one
    synchronisation -- pass it where that matters.  Everything else is score_rank's, and it is a function of its own because
    score_rank's argument list is pinned: that call keeps launching the kernels it always launched."""
    if group is None:
        raise RuntimeError("score_rank_capped: group is None; the call without caps is score_rank")
    return _score_rank(news_vecs, user_vecs, targets, exclude, ks, splits, prior, stamp, window, group, group_cap, n_groups)


def _score_rank(news_vecs, user_vecs, targets, exclude, ks, splits, prior, stamp, window, group, group_cap, n_groups):
    """score_rank (group None) and score_rank_capped: one descriptor, one library call."""
    _need_gpu(news_vecs, user_vecs, targets, exclude.ids if isinstance(exclude, ExclusionLists) else exclude, prior, stamp, window, group)
    V, N, U, dev = _vector_args("score_rank", news_vecs, user_vecs)
    if targets.dim() != 2 or targets.shape[0] != U:
        raise RuntimeError(f"score_rank: targets must be [U = {U}, T], got {tuple(targets.shape)}")
    T = targets.shape[1]
    want_sums = ks is not None
    ks = [int(k) for k in (ks or ())]
    ranks = torch.empty(U, T, dtype=torch.int32, device=dev)
    scores = torch.empty(U, T, dtype=torch.float32, device=dev)
    if U == 0:
        return ranks, scores, torch.zeros(2 + 2 * len(ks), dtype=torch.float64, device=dev) if want_sums else None
    sums = torch.empty(2 + 2 * len(ks), dtype=torch.float64, device=dev) if want_sums else None     # the call overwrites it
    tg = targets.detach().to(torch.int32).contiguous()
    ex_fields, ex_keep = _exclude_args("score_rank", exclude, U, dev)
    ks_host = (C.c_int * max(len(ks), 1))(*ks)
    pr, st, win = _pool_args("score_rank", V, U, dev, prior, stamp, window)
    gr = _group_args("score_rank", group, V, dev)
    if gr is not None and n_groups is None:
        n_groups = max(int(gr.max().item()) + 1, 1)                      # the one synchronisation; all ids negative: one empty group
    d = _lib.RankDesc(news_vecs=ptr(news_vecs), ld_news=news_vecs.stride(0) if V > 1 else N, V=V, user=ptr(user_vecs),
                      ld_user=user_vecs.stride(0) if U > 1 else N, U=U, N=N, T=T, targets=ptr(tg), ld_targets=T, **ex_fields,
                      splits=int(splits), ks=ks_host, n_ks=len(ks), out_ranks=ptr(ranks), out_scores=ptr(scores),
                      out_sums=ptr(sums), prior=ptr(pr), stamp=ptr(st), window=ptr(win), ld_window=2 if win is not None else 0,
                      group=ptr(gr), group_cap=0 if group_cap is None else int(group_cap), n_groups=0 if n_groups is None else int(n_groups))
    ws = _ws(_lib.lib().nr_score_rank_workspace_bytes(C.byref(d)), dev)      # 0 for a bad descriptor: the call below says why
    d.ws, d.ws_bytes = ptr(ws) if ws.numel() else None, ws.numel() * 4
    check(_lib.lib().nr_score_rank(C.byref(d), _stream()), "nr_score_rank")
    return ranks, scores, sums


def stack_rows(a, b, mask_b=None, flags=True):
    """[a ; b] of two int32 id matrices with the same row width (candidate titles, then history titles) and, if asked, the int32
    "needed" flags [1 .. 1 ; mask_b != 0] of the stacked rows -- one launch (nr_stack_rows)."""
    _need_gpu(a, b, mask_b)
    a2, b2 = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    if a2.shape[1] != b2.shape[1]:
        raise RuntimeError(f"stack_rows: row widths differ ({a2.shape[1]} vs {b2.shape[1]})")
    a2, b2 = (t if t.dtype == torch.int32 and t.is_contiguous() else t.to(torch.int32).contiguous() for t in (a2, b2))
    m = None
    if mask_b is not None:
        m = mask_b.reshape(-1)
        if m.dtype != torch.float32 or not m.is_contiguous():
            m = m.float().contiguous()
        if m.numel() != b2.shape[0]:
            raise RuntimeError(f"stack_rows: {m.numel()} mask entries for {b2.shape[0]} rows")
    out = torch.empty(a2.shape[0] + b2.shape[0], a2.shape[1], dtype=torch.int32, device=a2.device)
    fl = torch.empty(out.shape[0], dtype=torch.int32, device=out.device) if flags else None
    check(_lib.lib().nr_stack_rows(ptr(a2), a2.shape[0], ptr(b2), b2.shape[0], a2.shape[1], ptr(m), ptr(out), ptr(fl), _stream()), "nr_stack_rows")
    if fl is not None:
        fl._nr_flags01 = True
    return out, fl


def assemble_batch(news_combined, hist_idx, pos_idx, neg_idx, label):
    """Row f1: history [B, H, F] = news_combined[hist_idx]; candidate [B, 1+K, F] = news_combined[neg[:label] + [pos] +
    neg[label:]] (src/dataset.py:40-48 + the DataLoader collate), gathered on the device from int32 index arrays."""
    _need_gpu(news_combined, hist_idx, pos_idx, neg_idx, label)
    comb = news_combined if news_combined.dim() == 2 else news_combined.reshape(news_combined.shape[0], -1)
    if comb.dtype != torch.int32 or not comb.is_contiguous():
        comb = comb.to(torch.int32).contiguous()
    hist_idx, pos_idx, neg_idx = (t.to(torch.int32).contiguous() for t in (hist_idx, pos_idx, neg_idx))
    label = label.to(torch.int64).contiguous()
    B, H = hist_idx.shape
    K, F = neg_idx.shape[1], comb.shape[1]
    dev = comb.device
    history = torch.empty(B, H, F, dtype=torch.int32, device=dev)
    candidate = torch.empty(B, 1 + K, F, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev) if CHECK_INDICES else None
    check(_lib.lib().nr_assemble_batch(ptr(comb), comb.shape[0], F, ptr(hist_idx), ptr(pos_idx), ptr(neg_idx), ptr(label), B, H, K,
                                       ptr(history), ptr(candidate), ptr(bad), _stream()), "nr_assemble_batch")
    if bad is not None and int(bad.item()):
        raise IndexError(f"assemble_batch: {int(bad.item())} news indices / labels out of range")
    return history, candidate


def eval_metrics(score, label, offsets, max_cand=None, return_per_impression=False):
    """Row f2: per-impression AUC / MRR / nDCG@5 / nDCG@10 (src/metrics.py, src/main.py:249-263) over CSR candidate lists.
    Returns a DEVICE fp64 tensor [5] = [scored impressions, sum AUC, sum MRR, sum nDCG@5, sum nDCG@10]
    (+ the [n_imp, 4] per-impression table, AUC = -1 for skipped impressions, if asked)."""
    _need_gpu(score, label, offsets)
    score = score.detach().float().contiguous()
    label, offsets = label.to(torch.int32).contiguous(), offsets.to(torch.int32).contiguous()
    n_imp = offsets.numel() - 1
    if max_cand is None:
        max_cand = int((offsets[1:] - offsets[:-1]).max().item()) if n_imp > 0 else 0
    nbytes = int(_lib.lib().nr_eval_metrics_workspace_bytes(n_imp))
    per_imp = torch.empty(max(nbytes // 8, 4), dtype=torch.float64, device=score.device)
    sums = torch.empty(5, dtype=torch.float64, device=score.device)
    check(_lib.lib().nr_eval_metrics(ptr(score), ptr(label), ptr(offsets), n_imp, int(max_cand), ptr(per_imp), per_imp.numel() * 8,
                                     ptr(sums), _stream()), "nr_eval_metrics")
    if return_per_impression:
        return sums, per_imp[: n_imp * 4].view(n_imp, 4)
    return sums


def dropout_mask(count: int, p: float, seed: int, device) -> torch.Tensor:
    """Test hook: the keep mask the kernels use for element indices [0, count)."""
    out = torch.empty(count, dtype=torch.float32, device=device)
    check(_lib.lib().nr_dropout_mask(ptr(out), count, float(p), int(seed), _stream()), "nr_dropout_mask")
    return out


def gemm_nt(a: torch.Tensor, b: torch.Tensor, bias=None, act_tanh=False, out_dtype=None) -> torch.Tensor:
    """C = a . b^T (+bias)(tanh): the MFMA GEMM building block on dense operands (unit tests / measurement).

    `a` and `b` may be row-strided views (their row strides are passed as lda / ldb).  B padding, bf16: when b.stride(0) >=
    roundup32(K), the columns [K, roundup32(K)) of b's storage must be zero -- the LDS-DMA and weights-in-registers kernels
    run whole 32-deep k-steps and do not predicate the K tail of B; `pack(w, code)` / `pack(w, code, ld=...)` produce such an
    operand.  A column slice of a wider non-zero matrix is therefore only valid for K % 32 == 0 (or with a row stride below
    roundup32(K), which selects the kernels that predicate the tail).  `a` has no such requirement: its K tail is clamped."""
    _need_gpu(a, b)
    code = NR_BF16 if a.dtype == torch.bfloat16 else NR_F32
    M, K = a.shape
    N = b.shape[0]
    out_dtype = out_dtype or a.dtype
    c = torch.empty(M, N, dtype=out_dtype, device=a.device)
    check(_lib.lib().nr_gemm_nt(code, ptr(a), a.stride(0), ptr(b), b.stride(0), ptr(bias), int(act_tanh), ptr(c), N,
                                NR_BF16 if out_dtype == torch.bfloat16 else NR_F32, M, N, K, _stream()), "nr_gemm_nt")
    return c


def gemm_tn(dc: torch.Tensor, a: torch.Tensor, with_bias_grad=True):
    """dW = dc^T . a (fp32), db = column sums of dc: the weight-gradient GEMM building block."""
    _need_gpu(dc, a)
    code = NR_BF16 if a.dtype == torch.bfloat16 else NR_F32
    M, N = dc.shape
    K = a.shape[1]
    dw = torch.zeros(N, K, dtype=torch.float32, device=a.device)
    db = torch.zeros(N, dtype=torch.float32, device=a.device) if with_bias_grad else None
    check(_lib.lib().nr_gemm_tn(code, ptr(dc), dc.stride(0), ptr(a), a.stride(0), ptr(dw), K, ptr(db), M, N, K, _stream()),
          "nr_gemm_tn")
    return dw, db
