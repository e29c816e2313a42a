"""Train / eval loops with the shape of the reference's src/main.py (train :22-142, test :145-277).

File parsing of news.tsv and the title-embedding generation are out of scope: the loops take
the arrays those steps produce (`news_index`, `news_combined`, `embedding_matrix`).  Everything from the sharded
behaviours files onward follows the reference -- model by name, checkpoint dict layout, forward, acc, backward,
gradient all-reduce-mean, Adam, logging -- with the callers either side of the encoder path moved to the device
(SURVEY §8 rows f1, f2, f4):

  input   `args.feed = "device"` (default on the GPU): the shard is parsed ONCE into news-index arrays
          (`data.IndexedTrainShard`), uploaded, and every batch is assembled on the device (`ops.assemble_batch`);
          `"host"`: the reference's `DatasetTrain` + `DataLoader` (src/main.py:89-90), kept for comparison and for CPU runs.
  update  `args.dp_mode = "flat"` (default on the GPU): `parallel.FlatBucket` -- one gradient all-reduce, one fused
          HIP Adam kernel; `"ddp"`: `DistributedDataParallel` + `torch.optim.Adam` as src/main.py:76,82.
          `args.table_adam = "dense"` (default) or `"deferred"` (flat bucket, one rank, NAML): the trainable title table is
          stepped row by row, bit-identical to the dense update (`parallel.FlatBucket`).
  eval    the [N+1, news_dim] news-vector table stays on the device (encode optionally sharded over the ranks +
          all_gather), history vectors are gathered there, scores and the per-impression AUC / MRR / nDCG are computed
          there (`ops.score_eval`, `ops.eval_metrics`); five numbers per rank leave the device and are SUM-reduced to
          rank 0 (src/main.py:269-273).

Every rank runs the same number of batches (`parallel.agree_on_batches`): the reference's shards differ by one sample
and its ranks can hang in the last all-reduce.
"""
import importlib
import itertools
import logging
import os

import numpy as np
import torch
import torch.distributed as dist
from torch.utils.data import DataLoader

from . import _lib, ops, parallel
from .data import DatasetTrain, IndexedTestShard, IndexedTrainShard


def acc(y_true, y_hat):
    """src/utils.py:36-40."""
    y_hat = torch.argmax(y_hat, dim=-1)
    return (y_true == y_hat).sum().float() / y_true.shape[0]


def build_model(args, embedding_matrix, n_category=0, n_subcategory=0):
    """src/main.py:63-64: the model module is chosen by name."""
    module = importlib.import_module(f"newsrecommendation_amd.model.{args.model}")
    return module.Model(args, embedding_matrix, n_category, n_subcategory)


def checkpoint_dict(model, category_dict=None, subcategory_dict=None):
    """src/main.py:118-142 layout; DDP's 'module.' prefix stripped.  Tensors are copied to the HOST: a device-side clone
    would double a frozen multi-GB table in HBM at every epoch end, and a host copy also detaches the FlatBucket views from
    their shared buffer (each entry is saved with its own storage)."""
    def own(v):
        t = v.detach().cpu()
        return t.clone() if t.untyped_storage().nbytes() > t.numel() * t.element_size() else t      # (a view of a CPU bucket)
    sd = {(k[len("module."):] if k.startswith("module.") else k): own(v) for k, v in model.state_dict().items()}
    return {"model_state_dict": sd, "category_dict": category_dict or {}, "subcategory_dict": subcategory_dict or {}}


def load_checkpoint(path):
    """A checkpoint written by the reference (src/main.py:118-142) or by `train()`: tensors + plain dicts only, so the
    loader that executes nothing from the file suffices."""
    return torch.load(path, map_location="cpu", weights_only=True)


def _resolve_device(rank, is_distributed, device):
    if device is not None:
        return torch.device(device)
    return torch.device("cuda", rank if is_distributed else torch.cuda.current_device())


def _count_lines(path):
    with open(path, "rb") as f:
        return sum(1 for _ in f)


class DeviceFeed:
    """Row f1: the shard's index arrays and `news_combined` live on the device; `batch(i)` assembles batch i there."""

    def __init__(self, shard: IndexedTrainShard, news_combined, batch_size, device):
        comb = np.ascontiguousarray(news_combined).reshape(len(news_combined), -1)
        self.comb = torch.as_tensor(comb.astype(np.int32, copy=False), device=device)
        self.hist = torch.as_tensor(shard.hist, device=device)
        self.mask = torch.as_tensor(shard.mask, device=device)
        self.pos = torch.as_tensor(shard.pos, device=device)
        self.neg = torch.as_tensor(shard.neg, device=device)
        self.shard, self.B, self.n, self.device = shard, int(batch_size), len(shard), device
        self.label = None
        self.feat_shape = tuple(np.asarray(news_combined).shape[1:])

    def __len__(self):
        return (self.n + self.B - 1) // self.B                 # DataLoader default: the last partial batch is kept

    def start_epoch(self):
        self.label = torch.as_tensor(self.shard.draw_labels(), device=self.device)      # the epoch's random.randint stream

    def batch(self, i):
        a, b = i * self.B, min(self.n, (i + 1) * self.B)
        label = self.label[a:b]
        history, candidate = ops.assemble_batch(self.comb, self.hist[a:b], self.pos[a:b], self.neg[a:b], label)
        H, C = history.shape[1], candidate.shape[1]
        return (history.view(b - a, H, *self.feat_shape), self.mask[a:b], candidate.view(b - a, C, *self.feat_shape), label)


def train(rank, args, news_index, news_combined, embedding_matrix, category_dict=None, subcategory_dict=None,
          max_steps=None, log=logging.info, device=None, model_factory=None):
    """One rank of the training job (src/main.py:22-142).  rank=None: single process; otherwise rank `rank` of
    `args.nGPU` processes (the process group is created here, `env://`, as src/main.py:31).
    `device` defaults to cuda:<rank>; `model_factory(args, embedding_matrix, n_cat, n_sub)` defaults to `build_model`.
    Returns (model, losses) -- `losses` is a CPU tensor with one entry per step."""
    is_distributed = rank is not None
    rank = rank or 0
    device = _resolve_device(rank, is_distributed, device)
    on_gpu = device.type == "cuda"
    if on_gpu:
        torch.cuda.set_device(device)
    mode = getattr(args, "dp_mode", None) or ("flat" if on_gpu else "ddp")
    table_adam = getattr(args, "table_adam", None) or "dense"
    if table_adam not in parallel.FlatBucket.TABLE_ADAM:
        raise ValueError(f"table_adam must be 'dense' or 'deferred', got {table_adam!r}")
    if table_adam == "deferred" and mode != "flat":
        raise ValueError("table_adam='deferred' is a mode of the flat bucket (dp_mode='flat'): with dp_mode='ddp' torch.optim.Adam "
                         "owns the optimizer state")
    if table_adam == "deferred" and args.model != "NAML":
        raise ValueError("table_adam='deferred' steps NAML's title table row by row; the encoder of " + str(args.model) +
                         " does not announce the rows it reads")
    world = 1
    if is_distributed:
        _, world = parallel.init_distributed(rank, getattr(args, "nGPU", None), device=device)       # src/main.py:31
    model = (model_factory or build_model)(args, embedding_matrix, len(category_dict or {}), len(subcategory_dict or {}))
    if getattr(args, "load_ckpt_name", None):
        model.load_state_dict(load_checkpoint(os.path.join(args.model_dir, args.load_ckpt_name))["model_state_dict"])
    model = model.to(device)                                   # before the optimizer: its state follows the parameters' device
    if getattr(args, "deterministic", False) and on_gpu:       # bit-reproducible gradients (fixed-point integer atomics)
        # (only trainable outputs are ever registered with the fixed-point scratch: a frozen 575 M-value title table is not)
        ops.set_deterministic(True, elements=sum(p.numel() for p in model.parameters() if p.requires_grad) + (1 << 20), device=device)
    net, bucket, optimizer = model, None, None
    if mode == "flat":
        bucket = parallel.FlatBucket(model, lr=args.lr, table_adam=table_adam)        # rank-0 broadcast + one all-reduce + fused Adam per step
        model._nr_bucket = bucket                              # (a plain attribute: callers that want the optimizer state find it here)
    elif mode == "ddp":
        if world > 1:
            net = parallel.wrap_ddp(model, device)             # src/main.py:82
        optimizer = torch.optim.Adam(model.parameters(), lr=args.lr, fused=on_gpu)      # src/main.py:76
        trainable = [p for p in model.parameters() if p.requires_grad]
    else:
        raise ValueError(f"dp_mode must be 'flat' or 'ddp', got {mode!r}")

    data_file = os.path.join(args.train_data_dir, f"behaviors_np{args.npratio}_{rank}.tsv")            # src/main.py:89
    feed_mode = getattr(args, "feed", None) or ("device" if on_gpu else "host")
    if feed_mode == "device":
        feed = DeviceFeed(IndexedTrainShard(data_file, news_index, args), news_combined, args.batch_size, device)
        n_local = len(feed)
    elif feed_mode == "host":
        dataset = DatasetTrain(data_file, news_index, news_combined, args)
        n_local = (_count_lines(data_file) + args.batch_size - 1) // args.batch_size
    else:
        raise ValueError(f"feed must be 'device' or 'host', got {feed_mode!r}")
    n_batches = parallel.agree_on_batches(n_local, device)     # every rank stops together

    losses, step = [], 0
    for ep in range(getattr(args, "start_epoch", 0), args.epochs):
        loss_sum = torch.zeros((), device=device)
        acc_sum = torch.zeros((), device=device)
        net.train()
        if feed_mode == "device":
            feed.start_epoch()
            batches = (feed.batch(i) for i in range(n_batches))
        else:
            batches = itertools.islice(iter(DataLoader(dataset, batch_size=args.batch_size)), n_batches)
        for cnt, (history, history_mask, candidate, label) in enumerate(batches):
            if feed_mode == "host":
                history = history.to(device, non_blocking=True)
                history_mask = history_mask.to(device, non_blocking=True)
                candidate = candidate.to(device, non_blocking=True)
                label = label.to(device, non_blocking=True)
            bz_loss, y_hat = net(history, history_mask, candidate, label)
            if optimizer is not None:
                optimizer.zero_grad()
            bz_loss.backward()
            if bucket is not None:
                bucket.step()
            else:
                optimizer.step()
                if on_gpu:
                    # torch's fused Adam rewrites the parameters without moving their version counters: the packed bf16
                    # copy of a trainable table (ops.table_cache keys on the counter) would be served stale from step 2 on
                    for p in trainable:
                        ops.table_cache.invalidate(p)
                    ops.bump_param_epoch()
            with torch.no_grad():                              # accumulated on the device: no host sync per step
                loss_sum += bz_loss.detach()
                acc_sum += acc(label, y_hat)
                losses.append(bz_loss.detach())
            step += 1
            if cnt % args.log_steps == 0:
                log("[{}][{}] Ed: {}, train_loss: {:.5f}, acc: {:.5f}".format(
                    ep, rank, cnt * args.batch_size, float(loss_sum) / (cnt + 1), float(acc_sum) / (cnt + 1)))
            if max_steps is not None and step >= max_steps:
                break
        if bucket is not None:
            bucket.flush()                                     # a row-deferred table: every row brought to this step before it is saved
        if rank == 0 and getattr(args, "model_dir", None):
            os.makedirs(args.model_dir, exist_ok=True)
            torch.save(checkpoint_dict(net, category_dict, subcategory_dict), os.path.join(args.model_dir, f"epoch-{ep + 1}.pt"))
        if max_steps is not None and step >= max_steps:
            break
    if bucket is not None:
        bucket.flush()
    return model, (torch.stack(losses).float().cpu() if losses else torch.zeros(0))


@torch.no_grad()
def encode_news(model, news_combined, batch_size, device, shard_over_ranks=False):
    """Full-corpus encode (src/main.py:185-198); the [N+1, news_dim] table stays on the device.  With
    `shard_over_ranks` every rank encodes a contiguous 1/world slice and the slices are all-gathered --
    the reference encodes the whole corpus on every rank."""
    # (a tensor that already lives on the device is taken as it is: the slices below are views, `.to(device)` a no-op)
    ids = news_combined.to(torch.int32) if torch.is_tensor(news_combined) else torch.as_tensor(np.asarray(news_combined), dtype=torch.int32)
    n = ids.shape[0]
    batch_size = max(int(batch_size), 16384)                   # the encoder is row-wise: bigger chunks, same vectors, fewer launches
    world = parallel.world_size() if shard_over_ranks else 1
    rank = dist.get_rank() if world > 1 else 0
    per = (n + world - 1) // world
    lo, hi = min(n, rank * per), min(n, (rank + 1) * per)
    out = [model.news_encoder(ids[i:min(hi, i + batch_size)].to(device)) for i in range(lo, hi, batch_size)]
    dim = out[0].shape[1] if out else model.args.news_dim
    mine = torch.cat(out, dim=0) if out else torch.zeros(0, dim, device=device)
    if world == 1:
        return mine
    padded = torch.zeros(per, dim, dtype=mine.dtype, device=device)
    padded[: mine.shape[0]] = mine
    parts = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(parts, padded)                             # [per, news_dim] fp32 per rank (20 MB at 100k news / 8 ranks)
    return torch.cat(parts, dim=0)[:n]


def _short_history_split(shard, H):
    """[(impressions whose first H - 32 history slots are all masked, H - 32), (the others, 0)] as index arrays; part of the
    shard's preparation (numpy over its mask array), kept on the shard object."""
    cached = getattr(shard, "_nr_short_split", None)
    if cached is None or cached[0] != H:
        m = shard.mask
        m = m.detach().cpu().numpy() if torch.is_tensor(m) else np.asarray(m)
        short = ~(m[:, :H - 32] != 0).any(axis=1)
        cached = (H, [(np.nonzero(short)[0].astype(np.int64), H - 32), (np.nonzero(~short)[0].astype(np.int64), 0)], {})
        try:
            shard._nr_short_split = cached
        except AttributeError:
            pass
    return cached[1], cached[2]


def _user_vectors(model, news_vecs, hist, mask, batch_size, device, owner):
    """User vectors [n, news_dim] fp32 of n histories given as indices into the news-vector table (`hist`, `mask`: device
    tensors [n, H]).  `owner` carries the host copy of the mask (`owner.mask`) and keeps the short-history split made from it."""
    n = hist.shape[0]
    user = torch.empty(n, news_vecs.shape[1], dtype=torch.float32, device=device)
    # masked user encoder (src/demo.sh:26): the gather can hand over the compute dtype directly (gather + cast in one pass)
    margs = getattr(model, "args", None)
    code = ops.dtype_code(getattr(margs, "compute_dtype", "fp32")) if getattr(margs, "user_log_mask", False) else ops.NR_F32
    batch_size = max(int(batch_size), 8192)                    # the user encoder is row-wise: bigger chunks, same vectors
    indexed = getattr(model.user_encoder, "forward_indexed", None)                 # history as indices into the vector table
    H = hist.shape[1] if hist.dim() == 2 else 0
    if indexed is not None and getattr(margs, "user_log_mask", False) and H > 32 and n > 0:
        # A masked slot contributes nothing to the masked user encoder (attention keys with weight 0, pooling weight 0:
        # src/model/model_utils.py:28,51), so it can simply be left out.  Histories are front-padded (src/dataset.py:17-24): a
        # user whose first H - 32 slots are all masked is encoded from the LAST 32 slots alone -- one 32 x 32 attention tile per
        # head through the title-shape kernel (2.5 x the item rate of the 64-row kernel) and 32 instead of H pooling rows.  The
        # split is made on the host from the shard's own mask array (no device synchronisation); same vectors.
        groups, on_device = _short_history_split(owner, H)
        for g, (idx_np, off) in enumerate(groups):
            if len(idx_np) == 0:
                continue
            sel = on_device.get((g, str(device)))
            if sel is None:
                sel = on_device[(g, str(device))] = torch.as_tensor(idx_np, device=device)
            h_g = hist.index_select(0, sel)[:, off:].contiguous()
            m_g = mask.index_select(0, sel)[:, off:].contiguous()
            for a in range(0, len(idx_np), batch_size):
                b = min(len(idx_np), a + batch_size)
                user.index_copy_(0, sel[a:b], indexed(news_vecs, h_g[a:b], m_g[a:b]).float())
    else:
        for a in range(0, n, batch_size):
            b = min(n, a + batch_size)
            if indexed is not None:
                user[a:b] = indexed(news_vecs, hist[a:b], mask[a:b])
            else:
                log_vecs = ops.embed_gather(news_vecs, hist[a:b], code)               # [B, H, news_dim], device gather
                user[a:b] = model.user_encoder(log_vecs, mask[a:b])                   # src/main.py:247
    return user


@torch.no_grad()
def score_shard(model, news_vecs, shard: IndexedTestShard, batch_size, device):
    """Rows a13 + f2 on the device: user vectors of every impression of the shard (history vectors gathered from the
    news-vector table), candidate scores (src/main.py:253) and the per-impression ranking metrics.
    Returns (scores [n_cand] device fp32, sums device fp64 [5] = scored count + 4 metric sums)."""
    n = len(shard)
    hist = torch.as_tensor(shard.hist, device=device)
    mask = torch.as_tensor(shard.mask, device=device)
    user = _user_vectors(model, news_vecs, hist, mask, batch_size, device, shard)
    offsets = torch.as_tensor(shard.offsets, device=device)
    counts = shard.offsets[1:] - shard.offsets[:-1]
    imp_of = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=device), torch.as_tensor(counts, device=device).long())
    cand = torch.as_tensor(shard.cand, device=device)
    scores = ops.score_eval(news_vecs, cand, imp_of, user) if cand.numel() else torch.zeros(0, device=device)
    sums = ops.eval_metrics(scores, torch.as_tensor(shard.label, device=device), offsets, max_cand=int(counts.max()) if n else 0)
    return scores, sums


class _Histories:
    """What _user_vectors needs of a shard: the mask on the host."""

    def __init__(self, mask):
        self.mask = mask


def _pool_kwargs(device, prior, news_time, window):
    """recommend's / rank_eval's pool arguments as ops.score_topk's / ops.score_rank's keywords, on `device`; what is None is left
    out, so a call without pools is the call it always was."""
    kw = {}
    if prior is not None:
        kw["prior"] = torch.as_tensor(prior).to(device=device, dtype=torch.float32)
    if news_time is not None:
        kw["stamp"] = torch.as_tensor(news_time).to(device=device, dtype=torch.int32)
    if window is not None:
        kw["window"] = torch.as_tensor(window).to(device=device, dtype=torch.int32)
    return kw


def _exclusions(hist, m, exclude_history, seen, device):
    """What recommend / rank_eval hand to ops.score_topk / ops.score_rank as `exclude`: None, the masked history as a tensor [U, H]
    (H <= 64: the dense list, the call as it always was) or an ops.ExclusionLists (a wider history, or any `seen`: history
    union seen, of any length)."""
    masked = None
    if exclude_history and hist.dim() == 2 and hist.shape[1] > 0:
        masked = (hist * (m != 0).to(torch.int32)).contiguous()
    if seen is None:
        if masked is not None and masked.shape[1] > _lib.NR_TOPK_MAX_EXCLUDE:
            return ops.ExclusionLists(masked)
        return masked
    lists = seen.to(device) if isinstance(seen, ops.ExclusionLists) else ops.ExclusionLists(seen, device=device)
    if lists.U != hist.shape[0]:
        raise RuntimeError(f"seen: lists for {lists.U} users, the call has {hist.shape[0]}")
    return lists if masked is None else lists.merged(masked)


@torch.no_grad()
def recommend(model, news_vecs, hist_idx, mask, k, exclude_history=True, batch_size=8192, prior=None, news_time=None, window=None,
              news_group=None, group_cap=None, seen=None):
    """Full-corpus recommendation: for every user the k best news of the whole table `news_vecs` ([N+1, news_dim], what
    encode_news returns), none of them the padding news 0.  hist_idx [U, H]: the users' clicked histories as news indices,
    front padded with 0 (src/dataset.py:17-24); mask [U, H]: 1 for a real slot.  The user vectors come from the code
    score_shard uses (_user_vectors); scoring and selection are one fused pass (ops.score_topk): no [U, V] score matrix.
    exclude_history: a user is not given what they already clicked -- the WHOLE history, whatever its width.  A history of at
    most 64 slots goes through the kernel's dense list (64 ids per user is where that path ends); a wider one goes through
    exclusion lists of any length (ops.ExclusionLists, the CSR lists of include/nrhip.h K9).
    seen: news a user must not be given beyond its history -- "everything this user has been shown", hundreds to thousands of
    ids: an ops.ExclusionLists (build it once per batch of users), a tensor [U, E] of any width (0 = no entry) or a sequence
    of U id arrays.  The row is then the k best of what is left, still k entries wherever k can be taken: the filter acts
    inside the selection, not on a finished row.
    Returns (ids int32 [U, k], scores fp32 [U, k]) on the device, rows sorted by (score descending, id ascending); a row with
    fewer than k eligible news ends in id 0, score -inf.  Several ranks: the caller shards the users; there is no collective.
    Pools (ops.score_topk): prior [N+1] -- a per-news freshness or popularity term added to the score in fp32, -inf = not in
    the pool at all; news_time [N+1] integer stamps with window [U, 2] -- user u is only given news with
    window[u, 0] <= news_time[v] <= window[u, 1].  The caller supplies the arrays (any integer unit of time).
    Group caps (ops.score_topk): news_group [N+1] integer group ids -- MIND's category or subcategory column, say; negative =
    in no group -- with group_cap = c: a row holds at most c news of one group and is otherwise the same walk down the order,
    so it still has k entries wherever k can be taken.  The cap is applied inside the selection, not to a finished row.
    rank_eval_capped takes the same two arguments and ranks the held-out clicks in this capped ranking."""
    news_vecs, user, exclude, kw, caps = _recommend_args(model, news_vecs, hist_idx, mask, exclude_history, batch_size, prior, news_time, window,
                                                         news_group, group_cap, seen)
    return ops.score_topk(news_vecs, user, k, exclude=exclude, **kw, **caps)


@torch.no_grad()
def recommend_sample(model, news_vecs, hist_idx, mask, k, temperature, seed, draw=0, user_keys=None, exclude_history=True, batch_size=8192,
                     prior=None, news_time=None, window=None, news_group=None, group_cap=None, seen=None):
    """Sampled full-corpus recommendation: recommend's row drawn instead of maximised -- k news without replacement, each draw
    proportional to exp(score / temperature) over what is left (ops.score_sample; include/nrhip.h, K12).  A recommender that
    serves these rows explores (a fresh article gets its share), does not repeat itself on every reload, and logs rows drawn
    from a known distribution.  The user vectors, exclusions, pools and caps are recommend's.
    temperature: a float or a [U] tensor (finite, >= 0; 0 is recommend's row, bit for bit); to choose it relative to a user's
    own score spread see INTEGRATION.md.  seed, draw: the name of the draw.  user_keys [U] integers: global user numbers (None =
    the row index) -- a user's row depends on its key only, not on batch, rank or place.
    Returns (ids int32 [U, k], model_scores fp32 [U, k]): the scores (+ prior) of the news taken, to within rounding -- a row is
    ordered by the perturbed values, not by them; a row with fewer than k eligible news ends in id 0, score -inf."""
    news_vecs, user, exclude, kw, caps = _recommend_args(model, news_vecs, hist_idx, mask, exclude_history, batch_size, prior, news_time, window,
                                                         news_group, group_cap, seen)
    device = news_vecs.device
    if isinstance(temperature, torch.Tensor):
        temperature = temperature.to(device=device, dtype=torch.float32)
    if user_keys is not None:
        user_keys = torch.as_tensor(user_keys).to(device=device)
    ids, _, model_scores = ops.score_sample(news_vecs, user, k, temperature, seed, draw=draw, user_keys=user_keys, exclude=exclude, **kw, **caps)
    return ids, model_scores


def _device_temperature(temperature, U, device):
    """A temperature as ops.score_logz / ops.row_logprob take it.  A scalar that is not finite and > 0 (0 above all: a
    deterministic row) becomes a [U] tensor of it, so that the answer is NaN for everybody instead of a refusal."""
    if isinstance(temperature, torch.Tensor):
        return temperature.to(device=device, dtype=torch.float32)
    t = float(temperature)
    return t if 0.0 < t < float("inf") else torch.full((U,), t, dtype=torch.float32, device=device)


@torch.no_grad()
def log_partition(model, news_vecs, hist_idx, mask, temperature, exclude_history=True, batch_size=8192, prior=None, news_time=None, window=None,
                  seen=None):
    """The log-partition of every user's full-corpus score row at `temperature` (ops.score_logz; include/nrhip.h, K13), over
    exactly the news recommend / recommend_sample would consider for that user under the same arguments: the user vectors,
    exclude_history, seen, prior, news_time and window are recommend's.  No [U, V] score matrix is formed.
    Returns (logsum fp32 [U], smax fp32 [U], count int32 [U]) on the device: smax is the best eligible score (recommend's first
    score, bit for bit), count the number of eligible news, logsum = log sum exp((score - smax) / temperature), so that
    log Z = smax / temperature + logsum and the softmax log-probability of an eligible news is
    (score - smax) / temperature - logsum.  temperature: a float or a [U] tensor, finite and > 0; a tensor entry that is not
    gives that user logsum = NaN."""
    news_vecs, user, exclude, kw, _ = _recommend_args(model, news_vecs, hist_idx, mask, exclude_history, batch_size, prior, news_time, window,
                                                      None, None, seen)
    return ops.score_logz(news_vecs, user, _device_temperature(temperature, user.shape[0], news_vecs.device), exclude=exclude, **kw)


@torch.no_grad()
def sample_propensity(model, news_vecs, hist_idx, mask, ids, temperature, exclude_history=True, batch_size=8192, prior=None, news_time=None,
                      window=None, news_group=None, group_cap=None, seen=None):
    """The probability with which recommend_sample drew its rows: for ids [U, k] returned by recommend_sample called with the
    SAME model, histories, temperature, exclusions and pools, logp[u, j] = log P(entry j is drawn at step j | entries 0 .. j-1
    are taken) under the Plackett-Luce law the rows follow, and total[u] = their sum = log P(the row, in this order) -- what a
    click log of served rows is reweighted by (inverse propensity weighting, off-policy evaluation).
    Two fused passes, no [U, V] matrix: the log-partition over everything eligible EXCEPT the row (ops.score_logz with the row
    merged into the exclusion lists: the row's entries are usually the heaviest terms, so they are left out of the stream rather
    than subtracted), then the row itself on top of that base, step by step, in fp64 (ops.row_logprob, sequential).
    Returns (logp fp32 [U, k], total fp32 [U]) on the device.  Fill entries (id 0, a short row) give 0.  temperature 0 -- as a
    float or as an entry of a [U] tensor -- gives NaN: such a row is recommend's, deterministic, its propensity is 1 and there
    is nothing to reweight by.  Seed, draw and user keys do not enter: the law does not depend on them.
    Group caps are not part of this function: under caps the mass that is left at a step needs per-group partitions, which is
    what sample_propensity_capped computes.  Passing news_group or group_cap here raises ValueError."""
    if news_group is not None or group_cap is not None:
        raise ValueError("sample_propensity: rows drawn under group caps (news_group / group_cap) have no propensity here: "
                         "the remaining mass under caps needs per-group partitions")
    news_vecs, user, exclude, kw, _ = _recommend_args(model, news_vecs, hist_idx, mask, exclude_history, batch_size, prior, news_time, window,
                                                      None, None, seen)
    device = news_vecs.device
    U = user.shape[0]
    rows = torch.as_tensor(ids).to(device=device, dtype=torch.int32)
    if rows.dim() != 2 or rows.shape[0] != U:
        raise RuntimeError(f"sample_propensity: ids must be [U = {U}, k], got {tuple(rows.shape)}")
    taken = ops.ExclusionLists(rows)
    lists = taken if exclude is None else (exclude if isinstance(exclude, ops.ExclusionLists) else ops.ExclusionLists(exclude)).merged(taken)
    tau = _device_temperature(temperature, U, device)
    base = ops.score_logz(news_vecs, user, tau, exclude=lists, **kw)
    return ops.row_logprob(news_vecs, user, rows, tau, base, True, **kw)


def _group_order(news_group, groups, device):
    """news_group as the int32 tensor on `device` and its ops.GroupOrder (`groups` if the caller built one already)."""
    group = torch.as_tensor(news_group).to(device=device, dtype=torch.int32)
    return group, (groups if groups is not None else ops.GroupOrder(group))


@torch.no_grad()
def log_partition_groups(model, news_vecs, hist_idx, mask, temperature, news_group, exclude_history=True, batch_size=8192, prior=None,
                         news_time=None, window=None, seen=None, groups=None):
    """log_partition per group (ops.score_logz_groups; include/nrhip.h, K15): for every user and every bin -- the groups
    0 .. G-1 of news_group [N+1] (MIND's category column, say) and bin G for the news of no group (negative id) -- over the
    news recommend would consider for that user under the same arguments.  Returns (logsum fp32, gmax fp32, count int32), each
    [U, G + 1] on the device: gmax the bin's best eligible score, count its eligible news, logsum = log sum exp((score - gmax) /
    temperature); an empty bin gives (-inf, -inf, 0).  With log_partition's log Z = smax / temperature + logsum,
    exp(gmax / temperature + logsum - log Z) is the category's share of the user's exposure under recommend_sample at this
    temperature.  groups: an ops.GroupOrder of news_group built beforehand (once per corpus); None builds it here."""
    news_vecs, user, exclude, kw, _ = _recommend_args(model, news_vecs, hist_idx, mask, exclude_history, batch_size, prior, news_time, window,
                                                      None, None, seen)
    _, order = _group_order(news_group, groups, news_vecs.device)
    return ops.score_logz_groups(news_vecs, user, _device_temperature(temperature, user.shape[0], news_vecs.device), order, exclude=exclude, **kw)


@torch.no_grad()
def sample_propensity_capped(model, news_vecs, hist_idx, mask, ids, temperature, news_group, group_cap, exclude_history=True, batch_size=8192,
                             prior=None, news_time=None, window=None, seen=None, groups=None):
    """sample_propensity for rows drawn under group caps: for ids [U, k] returned by recommend_sample called with the SAME model,
    histories, temperature, exclusions, pools, news_group and group_cap, logp[u, j] = log P(entry j is drawn at step j | entries
    0 .. j-1 are taken) under the law those rows follow -- at every step the softmax over the eligible news not yet taken whose
    group has fewer than group_cap entries in the row so far -- and total[u] = their sum = log P(the row, in this order).
    Two fused passes, no [U, V] matrix: the log-partition PER GROUP over everything eligible except the row (ops.score_logz_groups
    with the row merged into the exclusion lists), then the row on top of these bases in fp64 (ops.row_logprob_capped): the mass
    left at a step is the sum over the groups still open, every term positive.
    Returns (logp fp32 [U, k], total fp32 [U]) on the device.  Fill entries (id 0, a short row) give 0; temperature 0 gives NaN,
    as in sample_propensity; an entry the capped sampler cannot have drawn (its group was full) gives -inf.
    groups: an ops.GroupOrder of news_group built beforehand (once per corpus); None builds it here."""
    news_vecs, user, exclude, kw, _ = _recommend_args(model, news_vecs, hist_idx, mask, exclude_history, batch_size, prior, news_time, window,
                                                      None, None, seen)
    device = news_vecs.device
    U = user.shape[0]
    group, order = _group_order(news_group, groups, device)
    rows = torch.as_tensor(ids).to(device=device, dtype=torch.int32)
    if rows.dim() != 2 or rows.shape[0] != U:
        raise RuntimeError(f"sample_propensity_capped: ids must be [U = {U}, k], got {tuple(rows.shape)}")
    taken = ops.ExclusionLists(rows)
    lists = taken if exclude is None else (exclude if isinstance(exclude, ops.ExclusionLists) else ops.ExclusionLists(exclude)).merged(taken)
    tau = _device_temperature(temperature, U, device)
    bases = ops.score_logz_groups(news_vecs, user, tau, order, exclude=lists, **kw)
    return ops.row_logprob_capped(news_vecs, user, rows, tau, bases, group, group_cap, n_groups=order.n_groups, **kw)


def _in_lists(exclude, tg):
    """[U, T] bool: is tg[u, j] in user u's exclusion list (None, a dense tensor [U, E] or an ops.ExclusionLists)?"""
    if exclude is None:
        return torch.zeros_like(tg, dtype=torch.bool)
    lists = exclude if isinstance(exclude, ops.ExclusionLists) else ops.ExclusionLists(exclude)
    users, ids = lists._pairs()
    if ids.numel() == 0:
        return torch.zeros_like(tg, dtype=torch.bool)
    keys = (users << 31) + ids                            # ascending: users ascend, each segment ascends
    q = (torch.arange(tg.shape[0], device=tg.device, dtype=torch.int64)[:, None] << 31) + tg.to(torch.int64).clamp(min=0)
    at = torch.searchsorted(keys, q.contiguous()).clamp(max=keys.numel() - 1)
    return keys[at] == q


def _not_ranked(exclude, tg, V):
    """[U, T] bool: what rank_eval does not rank and the kernels do not look at -- fill, a listed news, a later repeat (stable sort
    by id: the first of equal ids is the earliest entry)."""
    srt, at = torch.sort(tg, dim=1, stable=True)
    rep = torch.zeros_like(tg, dtype=torch.bool)
    rep[:, 1:] = srt[:, 1:] == srt[:, :-1]
    return (tg < 1) | (tg >= V) | _in_lists(exclude, tg) | torch.zeros_like(rep).scatter(1, at, rep)


@torch.no_grad()
def target_logprob(model, news_vecs, hist_idx, mask, targets, temperature, exclude_history=True, batch_size=8192, prior=None, news_time=None,
                   window=None, seen=None):
    """The full-softmax log-probability of held-out clicks, the rank-side counterpart of sample_propensity: for targets [U, T]
    (0 = no entry), logp[u, j] = (score - smax) / temperature - logsum over the user's WHOLE eligible row (log_partition under
    the same arguments; ops.row_logprob, independent entries, in fp64 on rank_eval's score bits).  The arguments are rank_eval's;
    the result is NaN exactly where rank_eval gives rank 0: an entry that is 0 or out of range, excluded (history or seen),
    outside the pool, NaN-scored, or a repeat of an earlier entry of its row.  -nansum of it is the full-corpus negative
    log-likelihood, next to rank_eval's MRR and nDCG.  Returns logp fp32 [U, T] on the device."""
    news_vecs, user, exclude, kw, _ = _recommend_args(model, news_vecs, hist_idx, mask, exclude_history, batch_size, prior, news_time, window,
                                                      None, None, seen)
    device = news_vecs.device
    U, V = user.shape[0], news_vecs.shape[0]
    tg = torch.as_tensor(targets).to(device=device, dtype=torch.int32)
    if tg.dim() != 2 or tg.shape[0] != U:
        raise RuntimeError(f"target_logprob: targets must be [U = {U}, T], got {tuple(tg.shape)}")
    tau = _device_temperature(temperature, U, device)
    base = ops.score_logz(news_vecs, user, tau, exclude=exclude, **kw)
    W = _lib.NR_TOPK_MAX_K
    logp = torch.cat([ops.row_logprob(news_vecs, user, tg[:, c:c + W].contiguous(), tau, base, False, **kw)[0] for c in range(0, tg.shape[1], W)],
                     dim=1) if tg.shape[1] else torch.empty(U, 0, dtype=torch.float32, device=device)
    return logp.masked_fill(_not_ranked(exclude, tg, V), float("nan"))


def full_softmax_loss(model, news_vecs, hist_idx, mask, targets, temperature, exclude_history=True, batch_size=8192, prior=None, news_time=None,
                      window=None, seen=None):
    """The full-softmax training loss of held-out clicks over the whole (frozen) news-vector table: target_logprob's quantity with
    a gradient.  For targets [U, T] (0 = no entry), loss = the mean over the valid entries of
    -[(score - smax) / temperature - logsum], the softmax taken over everything recommend would consider for that user under the
    same arguments (exclude_history, seen, prior, news_time, window: target_logprob's).  No negative sampling, no [U, V] matrix:
    forward and backward are fused passes over the table (ops.full_softmax_nll; include/nrhip.h, K13, K14, K17).
    Not under no_grad: the user vectors are formed WITH gradient, batch_size users at a time, as
    model.user_encoder(ops.embed_gather(news_vecs, hist, code), mask), so `loss` is differentiable with respect to the user
    encoder's parameters.  news_vecs is a constant (detached): the news encoder gets no gradient from this loss.
    An entry is valid exactly where target_logprob is not NaN: not fill, not excluded, inside the pool, not NaN-scored, no repeat
    of an earlier entry of its row, and the user's temperature finite and > 0.
    Returns (loss, n): loss a 0-dim fp32 tensor = sum of nll over the valid entries / n (0 when n == 0), n the number of valid
    entries as a 0-dim int64 device tensor.  To train on more users than one call should hold, call it per chunk of users, run
    backward() on loss * n per call -- each call's graph is freed by its own backward -- and divide the accumulated gradients by
    the total n."""
    device = news_vecs.device
    hist = torch.as_tensor(hist_idx).to(device=device, dtype=torch.int32)
    m = torch.as_tensor(mask).to(device=device, dtype=torch.float32)
    news_vecs = news_vecs.detach().float().contiguous()
    U, V = hist.shape[0], news_vecs.shape[0]
    tg = torch.as_tensor(targets).to(device=device, dtype=torch.int32)
    if tg.dim() != 2 or tg.shape[0] != U:
        raise RuntimeError(f"full_softmax_loss: targets must be [U = {U}, T], got {tuple(tg.shape)}")
    exclude = _exclusions(hist, m, exclude_history, seen, device)
    kw = _pool_kwargs(device, prior, news_time, window)
    tau = _device_temperature(temperature, U, device)
    tg = tg.masked_fill(_not_ranked(exclude, tg, V), 0)       # what target_logprob does not score is named as fill: it is in no sum
    margs = getattr(model, "args", None)
    code = ops.dtype_code(getattr(margs, "compute_dtype", "fp32")) if getattr(margs, "user_log_mask", False) else ops.NR_F32
    W = _lib.NR_TOPK_MAX_K
    total = torch.zeros((), dtype=torch.float32, device=device)
    n = torch.zeros((), dtype=torch.int64, device=device)
    step = max(int(batch_size), 1)
    for a in range(0, U, step):
        b = min(U, a + step)
        user = model.user_encoder(ops.embed_gather(news_vecs, hist[a:b], code), m[a:b]).float().contiguous()
        kw_b = dict(kw)
        if "window" in kw_b:
            kw_b["window"] = kw_b["window"][a:b].contiguous()
        tau_b = tau[a:b].contiguous() if isinstance(tau, torch.Tensor) else tau
        ex_b = exclude
        if exclude is not None and (a, b) != (0, U):
            ex_b = exclude.take(torch.arange(a, b, device=device)) if isinstance(exclude, ops.ExclusionLists) else exclude[a:b].contiguous()
        for c in range(0, tg.shape[1], W):
            nll, valid = ops.full_softmax_nll(news_vecs, user, tg[a:b, c:c + W].contiguous(), tau_b, exclude=ex_b, **kw_b)
            total = total + nll.sum()
            n = n + valid.sum()
    return total / n.clamp(min=1).to(torch.float32), n


@torch.no_grad()
def policy_entropy(model, news_vecs, hist_idx, mask, temperature, exclude_history=True, batch_size=8192, prior=None, news_time=None, window=None,
                   seen=None):
    """The entropy of the distribution recommend_sample serves at `temperature`: per user H = -sum_v p(v) log p(v) over exactly the
    news log_partition sums over under the same arguments (ops.score_logz, then ops.score_entropy; include/nrhip.h, K13 and K23),
    and var = Var_p(log p).  exp(H) is the effective number of news a user is exposed to -- the exploration dial of
    recommend_sample -- and var / temperature is dH / dtemperature, which is what a search for the temperature that gives a wanted
    entropy needs.  No [U, V] matrix is formed.  The arguments are log_partition's.
    Returns (entropy fp32 [U], var fp32 [U]) on the device: (0, 0) for a user with nothing or exactly one news eligible, NaN for a
    temperature that is not finite and > 0."""
    news_vecs, user, exclude, kw, _ = _recommend_args(model, news_vecs, hist_idx, mask, exclude_history, batch_size, prior, news_time, window,
                                                      None, None, seen)
    tau = _device_temperature(temperature, user.shape[0], news_vecs.device)
    base = ops.score_logz(news_vecs, user, tau, exclude=exclude, **kw)
    ent, var, _ = ops.score_entropy(news_vecs, user, tau, base, exclude=exclude, **kw)
    return ent, var


def policy_kl(model, ref, news_vecs, hist_idx, mask, temperature, ref_temperature=None, mode="reverse", exclude_history=True, batch_size=8192,
              prior=None, news_time=None, window=None, seen=None):
    """The mean KL divergence, over the full corpus, between the distribution `model` serves and that of a reference policy: the
    trust region of off-policy training (loss + kl_weight * mean_kl against the logging checkpoint), the distillation loss of one
    user encoder into another (mode="forward"), and, under torch.no_grad(), the drift monitor between two checkpoints.
    `ref`: a second model of the same class, whose user vectors are formed under no_grad from the same histories (a logged or
    teacher checkpoint), or a [U, news_dim] tensor of logged user vectors.  The two policies share the table, the histories'
    exclusions and the pools; they differ in user vectors and temperature (ref_temperature None = temperature's value).
    mode="reverse": KL(served || reference); mode="forward": KL(reference || served).  The arguments, the chunking into batch_size
    users and the accumulation are full_softmax_loss_entropy's; per chunk the work is ops.policy_kl (include/nrhip.h, K13, K26,
    K27), differentiable with respect to the user encoder and, in the reverse mode, a temperature that requires grad.
    Returns (mean_kl, n): the mean over the n valid users (something eligible, temperatures finite and > 0), n a device tensor."""
    device = news_vecs.device
    hist = torch.as_tensor(hist_idx).to(device=device, dtype=torch.int32)
    m = torch.as_tensor(mask).to(device=device, dtype=torch.float32)
    news_vecs = news_vecs.detach().float().contiguous()
    U, N = hist.shape[0], news_vecs.shape[1]
    ref_vecs = None
    if isinstance(ref, torch.Tensor):
        if tuple(ref.shape) != (U, N):
            raise RuntimeError(f"policy_kl: logged user vectors must be [U = {U}, news_dim = {N}], got {tuple(ref.shape)}")
        ref_vecs = ref.detach().to(device=device, dtype=torch.float32).contiguous()
    elif not hasattr(ref, "user_encoder"):
        raise RuntimeError(f"policy_kl: ref must be a model with a user_encoder or a [U, news_dim] tensor, got {type(ref).__name__}")
    exclude = _exclusions(hist, m, exclude_history, seen, device)
    kw = _pool_kwargs(device, prior, news_time, window)
    tau = _device_temperature(temperature, U, device)
    rtau = None if ref_temperature is None else _device_temperature(ref_temperature, U, device)
    margs = getattr(model, "args", None)
    code = ops.dtype_code(getattr(margs, "compute_dtype", "fp32")) if getattr(margs, "user_log_mask", False) else ops.NR_F32
    total = torch.zeros((), dtype=torch.float32, device=device)
    n = torch.zeros((), dtype=torch.int64, device=device)
    step = max(int(batch_size), 1)
    for a in range(0, U, step):
        b = min(U, a + step)
        user = model.user_encoder(ops.embed_gather(news_vecs, hist[a:b], code), m[a:b]).float().contiguous()
        if ref_vecs is not None:
            ref_b = ref_vecs[a:b]
        else:
            with torch.no_grad():
                rargs = getattr(ref, "args", None)
                rcode = ops.dtype_code(getattr(rargs, "compute_dtype", "fp32")) if getattr(rargs, "user_log_mask", False) else ops.NR_F32
                ref_b = ref.user_encoder(ops.embed_gather(news_vecs, hist[a:b], rcode), m[a:b]).float().contiguous()
        kw_b = dict(kw)
        if "window" in kw_b:
            kw_b["window"] = kw_b["window"][a:b].contiguous()
        tau_b = tau[a:b].contiguous() if isinstance(tau, torch.Tensor) and tau.dim() == 1 else tau
        rtau_b = rtau[a:b].contiguous() if isinstance(rtau, torch.Tensor) and rtau.dim() == 1 else rtau
        ex_b = exclude
        if exclude is not None and (a, b) != (0, U):
            ex_b = exclude.take(torch.arange(a, b, device=device)) if isinstance(exclude, ops.ExclusionLists) else exclude[a:b].contiguous()
        kl, valid = ops.policy_kl(news_vecs, user, ref_b, tau_b, rtau_b, mode=mode, exclude=ex_b, **kw_b)
        total = total + kl.sum()
        n = n + valid.sum()
    return total / n.clamp(min=1).to(torch.float32), n


def full_softmax_loss_entropy(model, news_vecs, hist_idx, mask, targets, temperature, entropy_weight, exclude_history=True, batch_size=8192,
                              prior=None, news_time=None, window=None, seen=None):
    """full_softmax_loss with an entropy bonus and a temperature that may be learned:
    loss = full_softmax_loss's loss - entropy_weight * mean_entropy, mean_entropy the mean of H_u = -sum_v p(v | u) log p(v | u)
    over the users with anything eligible (and a temperature that is finite and > 0), the softmax the one the loss is taken over.
    The bonus keeps a policy trained from logged rows from collapsing onto a few news.  The arguments, the
    chunking into batch_size users and the valid-entry rules are full_softmax_loss's; forward and backward are fused passes
    (ops.full_softmax_nll_entropy; include/nrhip.h, K13, K14, K23, K24).
    temperature: a float, or a floating point tensor, 0-dim or [U] -- an nn.Parameter gets its gradient (of the loss term and of
    the bonus).  entropy_weight: a float; 0 leaves the entropy out of the graph, and loss and its gradients are then
    full_softmax_loss's, bit for bit.
    Returns (loss, n, mean_entropy): loss and n as in full_softmax_loss, mean_entropy a detached 0-dim fp32 tensor."""
    return _full_softmax_loss_entropy("full_softmax_loss_entropy", False, model, news_vecs, hist_idx, mask, targets, temperature, entropy_weight,
                                      exclude_history, batch_size, prior, news_time, window, seen)


def full_softmax_loss_entropy_joint(model, news_table, hist_idx, mask, targets, temperature, entropy_weight, exclude_history=True, batch_size=8192,
                                    prior=None, news_time=None, window=None, seen=None):
    """full_softmax_loss_entropy with a news-vector table that may require grad: the same loss, the same valid entries, the same
    (loss, n, mean_entropy), and a gradient for `news_table` ([V, news_dim] fp32 on the GPU: a table that is fine-tuned directly, or
    the output of the news encoder) as well as for the user encoder and a temperature that requires grad -- the entropy bonus and
    the learnable temperature while the news side trains.  Built from full_softmax_loss_entropy the way full_softmax_loss_joint is
    built from full_softmax_loss: the table is not detached, the clicked histories are gathered with ops.news_gather (its backward
    is a scatter-add with fp32 atomics: the last bits of the table gradient depend on the arrival order), and the softmax is
    ops.full_softmax_nll_entropy_joint: one nr_score_expect_news_affine call per chunk of users whose entropy is in the loss
    (include/nrhip.h, K25), one nr_score_expect_news call (K18) per chunk otherwise.  entropy_weight = 0 leaves the entropy out of
    the graph: loss and gradients are then full_softmax_loss_joint's.  A table that does not require grad gives
    full_softmax_loss_entropy's gradients; the news pass is then not launched."""
    return _full_softmax_loss_entropy("full_softmax_loss_entropy_joint", True, model, news_table, hist_idx, mask, targets, temperature,
                                      entropy_weight, exclude_history, batch_size, prior, news_time, window, seen)


def _full_softmax_loss_entropy(what, joint, model, news_vecs, hist_idx, mask, targets, temperature, entropy_weight, exclude_history, batch_size,
                               prior, news_time, window, seen):
    """The body of full_softmax_loss_entropy (joint False: the table detached, ops.embed_gather, ops.full_softmax_nll_entropy) and
    of full_softmax_loss_entropy_joint (joint True: the table as it is, ops.news_gather, ops.full_softmax_nll_entropy_joint)."""
    device = news_vecs.device
    hist = torch.as_tensor(hist_idx).to(device=device, dtype=torch.int32)
    m = torch.as_tensor(mask).to(device=device, dtype=torch.float32)
    # joint: no detach -- float() and contiguous() are the identity for a contiguous fp32 table
    news_vecs = news_vecs.float().contiguous() if joint else news_vecs.detach().float().contiguous()
    gather, nll_entropy = (ops.news_gather, ops.full_softmax_nll_entropy_joint) if joint else (ops.embed_gather, ops.full_softmax_nll_entropy)
    U, V = hist.shape[0], news_vecs.shape[0]
    tg = torch.as_tensor(targets).to(device=device, dtype=torch.int32)
    if tg.dim() != 2 or tg.shape[0] != U:
        raise RuntimeError(f"{what}: targets must be [U = {U}, T], got {tuple(tg.shape)}")
    exclude = _exclusions(hist, m, exclude_history, seen, device)
    kw = _pool_kwargs(device, prior, news_time, window)
    tau = _device_temperature(temperature, U, device)
    tg = tg.masked_fill(_not_ranked(exclude, tg, V), 0)       # what target_logprob does not score is named as fill: it is in no sum
    if tg.shape[1] == 0:
        tg = torch.zeros(U, 1, dtype=torch.int32, device=device)     # no targets at all: one column of fill carries the entropy
    margs = getattr(model, "args", None)
    code = ops.dtype_code(getattr(margs, "compute_dtype", "fp32")) if getattr(margs, "user_log_mask", False) else ops.NR_F32
    W = _lib.NR_TOPK_MAX_K
    total = torch.zeros((), dtype=torch.float32, device=device)
    ent_total = torch.zeros((), dtype=torch.float32, device=device)
    n = torch.zeros((), dtype=torch.int64, device=device)
    n_ent = torch.zeros((), dtype=torch.int64, device=device)
    step = max(int(batch_size), 1)
    for a in range(0, U, step):
        b = min(U, a + step)
        user = model.user_encoder(gather(news_vecs, hist[a:b], code), m[a:b]).float().contiguous()
        kw_b = dict(kw)
        if "window" in kw_b:
            kw_b["window"] = kw_b["window"][a:b].contiguous()
        tau_b = tau[a:b].contiguous() if isinstance(tau, torch.Tensor) and tau.dim() == 1 else tau
        ex_b = exclude
        if exclude is not None and (a, b) != (0, U):
            ex_b = exclude.take(torch.arange(a, b, device=device)) if isinstance(exclude, ops.ExclusionLists) else exclude[a:b].contiguous()
        for c in range(0, tg.shape[1], W):
            nll, valid, ent, count = nll_entropy(news_vecs, user, tg[a:b, c:c + W].contiguous(), tau_b, exclude=ex_b, return_count=True, **kw_b)
            if c == 0:                                        # a user's entropy is counted once: with its first block of targets
                counted = (count > 0) & ~torch.isnan(ent)
                ent_total = ent_total + torch.where(counted, ent, torch.zeros_like(ent)).sum()
                n_ent = n_ent + counted.sum()
            total = total + nll.sum()
            n = n + valid.sum()
    loss = total / n.clamp(min=1).to(torch.float32)
    mean_entropy = ent_total / n_ent.clamp(min=1).to(torch.float32)
    if float(entropy_weight) != 0.0:
        loss = loss - float(entropy_weight) * mean_entropy
    return loss, n, mean_entropy.detach()


def full_softmax_loss_joint(model, news_table, hist_idx, mask, targets, temperature, exclude_history=True, batch_size=8192, prior=None,
                            news_time=None, window=None, seen=None):
    """full_softmax_loss with a news-vector table that may require grad: the same loss, the same valid entries, the same
    (loss, n), and a gradient for `news_table` ([V, news_dim] fp32 on the GPU: a table that is fine-tuned directly, or the
    output of the news encoder, whose backward then receives the [V, news_dim] gradient) as well as for the user encoder.
    The table is reached on two paths: the softmax itself (ops.full_softmax_nll_joint: one nr_score_expect_news call per chunk
    of users and 128 targets, include/nrhip.h K18) and the clicked histories, whose vectors are gathered with ops.news_gather
    (its backward is a scatter-add with fp32 atomics: the last bits of the table gradient depend on the arrival order).  A
    table that does not require grad gives full_softmax_loss's gradients; the news pass is then not launched.
    To train on more users than one call should hold, proceed as with full_softmax_loss."""
    device = news_table.device
    hist = torch.as_tensor(hist_idx).to(device=device, dtype=torch.int32)
    m = torch.as_tensor(mask).to(device=device, dtype=torch.float32)
    table = news_table.float().contiguous()                   # no detach: both are the identity for a contiguous fp32 table
    U, V = hist.shape[0], table.shape[0]
    tg = torch.as_tensor(targets).to(device=device, dtype=torch.int32)
    if tg.dim() != 2 or tg.shape[0] != U:
        raise RuntimeError(f"full_softmax_loss_joint: targets must be [U = {U}, T], got {tuple(tg.shape)}")
    exclude = _exclusions(hist, m, exclude_history, seen, device)
    kw = _pool_kwargs(device, prior, news_time, window)
    tau = _device_temperature(temperature, U, device)
    tg = tg.masked_fill(_not_ranked(exclude, tg, V), 0)       # what target_logprob does not score is named as fill: it is in no sum
    margs = getattr(model, "args", None)
    code = ops.dtype_code(getattr(margs, "compute_dtype", "fp32")) if getattr(margs, "user_log_mask", False) else ops.NR_F32
    W = _lib.NR_TOPK_MAX_K
    total = torch.zeros((), dtype=torch.float32, device=device)
    n = torch.zeros((), dtype=torch.int64, device=device)
    step = max(int(batch_size), 1)
    for a in range(0, U, step):
        b = min(U, a + step)
        user = model.user_encoder(ops.news_gather(table, hist[a:b], code), m[a:b]).float().contiguous()
        kw_b = dict(kw)
        if "window" in kw_b:
            kw_b["window"] = kw_b["window"][a:b].contiguous()
        tau_b = tau[a:b].contiguous() if isinstance(tau, torch.Tensor) else tau
        ex_b = exclude
        if exclude is not None and (a, b) != (0, U):
            ex_b = exclude.take(torch.arange(a, b, device=device)) if isinstance(exclude, ops.ExclusionLists) else exclude[a:b].contiguous()
        for c in range(0, tg.shape[1], W):
            nll, valid = ops.full_softmax_nll_joint(table, user, tg[a:b, c:c + W].contiguous(), tau_b, exclude=ex_b, **kw_b)
            total = total + nll.sum()
            n = n + valid.sum()
    return total / n.clamp(min=1).to(torch.float32), n


def listwise_loss(model, news_table, hist_idx, mask, rows, temperature, weight=None, exclude_history=True, batch_size=8192, prior=None,
                  news_time=None, window=None, news_group=None, group_cap=None, seen=None):
    """The listwise training loss on ordered rows -- served rows of recommend_sample, or any ranked list -- under the Plackett-Luce
    law the sampler draws from: sample_propensity's quantity with a gradient.  rows [U, k <= 128] (0 = no entry); place j of a
    row is scored against everything recommend_sample would still consider for that user after places 0 .. j-1 (the user vectors,
    exclude_history, seen, prior, news_time and window are its), and
      loss = sum_u sum_j weight * nll[u, j] / n,   nll[u, j] = -log P(entry j is drawn at step j | entries 0 .. j-1 are taken),
    n the number of rows with at least one valid entry.  weight: None (1: listwise maximum likelihood, ListMLE), [U] (one per row:
    a reward, or a reward times a clipped importance ratio for off-policy policy gradient; negative is allowed) or
    [U, k] (per place: a position discount).  It is a constant: no gradient reaches it.
    No [U, V] matrix: forward and backward are fused passes over the table (ops.plackett_luce_nll; include/nrhip.h, K13, K14,
    K19, K17, K18).  Built like full_softmax_loss_joint: the user vectors are formed WITH gradient, batch_size users at a time,
    from ops.news_gather of the histories, so a `news_table` that requires grad is reached on both paths; one that does not
    gives the user encoder's gradients alone and the news pass is not launched.
    An entry that is 0 or out of range, inside the user's exclusions, or a repeat of an earlier entry of its row is turned into
    fill; an entry outside the pool or NaN-scored, and every entry of a user whose temperature is not finite and > 0, is not valid
    either.  None of these is a step of the row or part of the loss.
    Returns (loss, n): loss a 0-dim fp32 tensor (0 when n == 0), n a 0-dim int64 device tensor.  Rows wider than 128 are
    refused: a sequential row cannot be cut into chunks.  Rows drawn under group caps follow another law
    (sample_propensity_capped); passing news_group or group_cap raises ValueError."""
    if news_group is not None or group_cap is not None:
        raise ValueError("listwise_loss: rows drawn under group caps (news_group / group_cap) follow another law: "
                         "the remaining mass under caps needs per-group partitions")
    device = news_table.device
    hist = torch.as_tensor(hist_idx).to(device=device, dtype=torch.int32)
    m = torch.as_tensor(mask).to(device=device, dtype=torch.float32)
    table = news_table.float().contiguous()                   # no detach: both are the identity for a contiguous fp32 table
    U, V = hist.shape[0], table.shape[0]
    rw = torch.as_tensor(rows).to(device=device, dtype=torch.int32)
    if rw.dim() != 2 or rw.shape[0] != U:
        raise RuntimeError(f"listwise_loss: rows must be [U = {U}, k], got {tuple(rw.shape)}")
    k = rw.shape[1]
    if k < 1 or k > _lib.NR_TOPK_MAX_K:
        raise RuntimeError(f"listwise_loss: k = {k} places per row, must be in [1, {_lib.NR_TOPK_MAX_K}]: a sequential row cannot be cut "
                           "into chunks")
    w = None
    if weight is not None:
        w = torch.as_tensor(weight).detach().to(device=device, dtype=torch.float32)
        if tuple(w.shape) not in ((U,), (U, k)):
            raise RuntimeError(f"listwise_loss: weight must be [U = {U}] or [U, k = {k}], got {tuple(w.shape)}")
        w = w[:, None].expand(U, k) if w.dim() == 1 else w
    exclude = _exclusions(hist, m, exclude_history, seen, device)
    kw = _pool_kwargs(device, prior, news_time, window)
    tau = _device_temperature(temperature, U, device)
    rw = rw.masked_fill(_not_ranked(exclude, rw, V), 0)       # what is no step of the row is named as fill: it is in no sum
    margs = getattr(model, "args", None)
    code = ops.dtype_code(getattr(margs, "compute_dtype", "fp32")) if getattr(margs, "user_log_mask", False) else ops.NR_F32
    total = torch.zeros((), dtype=torch.float32, device=device)
    n = torch.zeros((), dtype=torch.int64, device=device)
    step = max(int(batch_size), 1)
    for a in range(0, U, step):
        b = min(U, a + step)
        user = model.user_encoder(ops.news_gather(table, hist[a:b], code), m[a:b]).float().contiguous()
        kw_b = dict(kw)
        if "window" in kw_b:
            kw_b["window"] = kw_b["window"][a:b].contiguous()
        tau_b = tau[a:b].contiguous() if isinstance(tau, torch.Tensor) else tau
        ex_b = exclude
        if exclude is not None and (a, b) != (0, U):
            ex_b = exclude.take(torch.arange(a, b, device=device)) if isinstance(exclude, ops.ExclusionLists) else exclude[a:b].contiguous()
        nll, valid = ops.plackett_luce_nll(table, user, rw[a:b].contiguous(), tau_b, exclude=ex_b, **kw_b)
        total = total + (nll.sum() if w is None else (nll * w[a:b]).sum())
        n = n + valid.any(dim=1).sum()
    return total / n.clamp(min=1).to(torch.float32), n


def _blocked(rw, group, n_groups, group_cap):
    """[U, k] bool: entries whose group already holds group_cap entries of the row before them (fill, id 0, counts for nothing;
    news of no group are never blocked).  Such an entry is no step of a capped row, and neither it nor any later one of its group
    is: the earlier ones alone use up the cap."""
    bins = group.to(torch.int64)[rw.to(torch.int64)]
    capped = (rw > 0) & (bins >= 0) & (bins < n_groups)
    # a stable sort by group puts a group's entries side by side in row order: an entry's place in its run = the entries before it
    srt, at = torch.sort(torch.where(capped, bins, torch.full_like(bins, n_groups)), dim=1, stable=True)
    pos = torch.arange(rw.shape[1], device=rw.device, dtype=torch.int64)[None, :].expand_as(srt)
    first = torch.ones_like(srt, dtype=torch.bool)
    first[:, 1:] = srt[:, 1:] != srt[:, :-1]
    run = torch.cummax(torch.where(first, pos, torch.zeros_like(pos)), dim=1).values
    return capped & torch.zeros_like(capped).scatter(1, at, (pos - run) >= int(group_cap))


def listwise_loss_capped(model, news_table, hist_idx, mask, rows, temperature, news_group, group_cap, weight=None, exclude_history=True,
                         batch_size=8192, prior=None, news_time=None, window=None, seen=None, groups=None):
    """listwise_loss for rows served under group caps -- recommend_sample(..., news_group, group_cap): sample_propensity_capped's
    quantity with a gradient for the user encoder.  rows [U, k <= 128] (0 = no entry); place j of a row is scored against the
    eligible news not yet taken whose group has fewer than group_cap entries in the row so far, and
      loss = sum_u sum_j weight * nll[u, j] / n,   nll[u, j] = -log P(entry j is drawn at step j | entries 0 .. j-1 are taken),
    n the number of rows with at least one valid entry; weight as in listwise_loss: None, [U] or [U, k], a constant.
    No [U, V] matrix: ops.plackett_luce_nll_capped (include/nrhip.h, K15, K16 forward; K21, K20 backward).  Built like
    listwise_loss: the user vectors are formed WITH gradient, batch_size users at a time.  The news table is frozen here: a
    `news_table` that requires grad is refused; listwise_loss_capped_joint is the function that trains it.
    An entry that is 0 or out of range, inside the user's exclusions, a repeat of an earlier entry of its row, or BLOCKED -- its
    group already holds group_cap entries of the row -- is turned into fill before the forward.  For a blocked entry this
    changes no D_j of a real step: as fill it is not merged into the lists, so its weight sits in its bin's base, which is part
    of D_j at exactly the steps at which the bin is open -- the steps at which K16 counts the weight of a blocked entry.  An entry
    outside the pool or NaN-scored, and every entry of a user whose temperature is not finite and > 0, is not valid either.  The
    entries of a group are counted over the real entries of the row; K16 counts the live ones, so the two agree on every row
    recommend_sample can have served under the same pools (it serves nothing outside the pool).
    Returns (loss, n) as listwise_loss does.  groups: an ops.GroupOrder of news_group built beforehand; None builds it here."""
    if isinstance(news_table, torch.Tensor) and news_table.requires_grad:
        raise RuntimeError("listwise_loss_capped: news_table requires grad, but the news side of the capped gradient is a missing pass "
                           "of this function (nr_score_expect_news with per-(user, bin) weights); it is not emulated: detach the table, "
                           "or use listwise_loss_capped_joint")
    return _listwise_loss_capped("listwise_loss_capped", False, model, news_table, hist_idx, mask, rows, temperature, news_group, group_cap, weight,
                                 exclude_history, batch_size, prior, news_time, window, seen, groups)


def listwise_loss_capped_joint(model, news_table, hist_idx, mask, rows, temperature, news_group, group_cap, weight=None, exclude_history=True,
                               batch_size=8192, prior=None, news_time=None, window=None, seen=None, groups=None):
    """listwise_loss_capped with a news-vector table that may require grad: the same loss, the same valid entries, the same
    (loss, n), and a gradient for `news_table` ([V, news_dim] fp32 on the GPU: a table that is fine-tuned directly, or the output
    of the news encoder) as well as for the user encoder.  The table is reached on two paths: the capped law itself
    (ops.plackett_luce_nll_capped_joint: one nr_score_expect_news_groups call per chunk of users, include/nrhip.h K22, on the
    coefficients of the same K21 call that serves the user side) and the clicked histories, whose vectors are gathered with
    ops.news_gather (a scatter-add with fp32 atomics in backward: the last bits of the table gradient depend on the arrival
    order).  A table that does not require grad gives listwise_loss_capped's gradients; the news pass is then not launched."""
    return _listwise_loss_capped("listwise_loss_capped_joint", True, model, news_table, hist_idx, mask, rows, temperature, news_group, group_cap,
                                 weight, exclude_history, batch_size, prior, news_time, window, seen, groups)


def _listwise_loss_capped(what, joint, model, news_table, hist_idx, mask, rows, temperature, news_group, group_cap, weight, exclude_history,
                          batch_size, prior, news_time, window, seen, groups):
    """The body of listwise_loss_capped (joint = False: the table detached, gathered without gradient) and of
    listwise_loss_capped_joint (joint = True: ops.news_gather and ops.plackett_luce_nll_capped_joint)."""
    if not 1 <= int(group_cap) <= 128:
        raise ValueError(f"{what}: group_cap = {group_cap}, must be in [1, 128]")
    device = news_table.device
    hist = torch.as_tensor(hist_idx).to(device=device, dtype=torch.int32)
    m = torch.as_tensor(mask).to(device=device, dtype=torch.float32)
    table = news_table.float().contiguous() if joint else news_table.detach().float().contiguous()
    U, V = hist.shape[0], table.shape[0]
    rw = torch.as_tensor(rows).to(device=device, dtype=torch.int32)
    if rw.dim() != 2 or rw.shape[0] != U:
        raise RuntimeError(f"{what}: rows must be [U = {U}, k], got {tuple(rw.shape)}")
    k = rw.shape[1]
    if k < 1 or k > _lib.NR_TOPK_MAX_K:
        raise RuntimeError(f"{what}: k = {k} places per row, must be in [1, {_lib.NR_TOPK_MAX_K}]: a sequential row cannot be "
                           "cut into chunks")
    w = None
    if weight is not None:
        w = torch.as_tensor(weight).detach().to(device=device, dtype=torch.float32)
        if tuple(w.shape) not in ((U,), (U, k)):
            raise RuntimeError(f"{what}: weight must be [U = {U}] or [U, k = {k}], got {tuple(w.shape)}")
        w = w[:, None].expand(U, k) if w.dim() == 1 else w
    group, order = _group_order(news_group, groups, device)
    if tuple(group.shape) != (V,):
        raise RuntimeError(f"{what}: news_group must hold one id per news, [V = {V}], got {tuple(group.shape)}")
    exclude = _exclusions(hist, m, exclude_history, seen, device)
    kw = _pool_kwargs(device, prior, news_time, window)
    tau = _device_temperature(temperature, U, device)
    rw = rw.masked_fill(_not_ranked(exclude, rw, V), 0)       # what is no step of the row is named as fill: it is in no sum
    rw = rw.masked_fill(_blocked(rw, group, order.n_groups, group_cap), 0)
    margs = getattr(model, "args", None)
    code = ops.dtype_code(getattr(margs, "compute_dtype", "fp32")) if getattr(margs, "user_log_mask", False) else ops.NR_F32
    total = torch.zeros((), dtype=torch.float32, device=device)
    n = torch.zeros((), dtype=torch.int64, device=device)
    gather = ops.news_gather if joint else ops.embed_gather
    nll_op = ops.plackett_luce_nll_capped_joint if joint else ops.plackett_luce_nll_capped
    step = max(int(batch_size), 1)
    for a in range(0, U, step):
        b = min(U, a + step)
        user = model.user_encoder(gather(table, hist[a:b], code), m[a:b]).float().contiguous()
        kw_b = dict(kw)
        if "window" in kw_b:
            kw_b["window"] = kw_b["window"][a:b].contiguous()
        tau_b = tau[a:b].contiguous() if isinstance(tau, torch.Tensor) else tau
        ex_b = exclude
        if exclude is not None and (a, b) != (0, U):
            ex_b = exclude.take(torch.arange(a, b, device=device)) if isinstance(exclude, ops.ExclusionLists) else exclude[a:b].contiguous()
        nll, valid = nll_op(table, user, rw[a:b].contiguous(), tau_b, order, group, group_cap, exclude=ex_b, **kw_b)
        total = total + (nll.sum() if w is None else (nll * w[a:b]).sum())
        n = n + valid.any(dim=1).sum()
    return total / n.clamp(min=1).to(torch.float32), n


@torch.no_grad()
def expected_exposure(model, news_vecs, hist_idx, mask, temperature, exclude_history=True, batch_size=8192, prior=None, news_time=None,
                      window=None, seen=None):
    """The expected exposure of every news under recommend_sample at `temperature`: exposure[v] = sum_u p(v | u), the expected
    number of these users whose FIRST sampled place goes to news v -- the softmax over everything recommend_sample would consider
    for that user under the same arguments (the user vectors, exclude_history, seen, prior, news_time and window are its).  It sums
    to the number of users with anything eligible.  Two fused passes, no [U, V] matrix: the log-partition (ops.score_logz, K13),
    then the mass-only mode of ops.score_expect_news (include/nrhip.h, K18).  A user whose temperature is not finite and > 0
    (0 above all: a deterministic row) contributes nothing.  Returns exposure fp32 [V] on the device; exposure[0] = 0."""
    news_vecs, user, exclude, kw, _ = _recommend_args(model, news_vecs, hist_idx, mask, exclude_history, batch_size, prior, news_time, window,
                                                      None, None, seen)
    tau = _device_temperature(temperature, user.shape[0], news_vecs.device)
    base = ops.score_logz(news_vecs, user, tau, exclude=exclude, **kw)
    _, mass = ops.score_expect_news(news_vecs, user, tau, base, exclude=exclude, rows=False, **kw)
    return mass


def _recommend_args(model, news_vecs, hist_idx, mask, exclude_history, batch_size, prior, news_time, window, news_group, group_cap, seen):
    """What recommend and recommend_diverse share: the fp32 table, the user vectors, the exclusions, the pool keywords and the
    cap keywords (group / group_cap; what is None is left out) of ops.score_topk."""
    device = news_vecs.device
    hist = torch.as_tensor(hist_idx).to(device=device, dtype=torch.int32)
    m = torch.as_tensor(mask).to(device=device, dtype=torch.float32)
    news_vecs = news_vecs.detach().float().contiguous()
    user = _user_vectors(model, news_vecs, hist, m, batch_size, device, _Histories(mask))
    exclude = _exclusions(hist, m, exclude_history, seen, device)
    kw = _pool_kwargs(device, prior, news_time, window)
    caps = {}
    if news_group is not None:
        caps["group"] = torch.as_tensor(news_group).to(device=device, dtype=torch.int32)
    if group_cap is not None:
        caps["group_cap"] = group_cap
    return news_vecs, user, exclude, kw, caps


@torch.no_grad()
def recommend_diverse(model, news_vecs, hist_idx, mask, k, penalty, pool=128, exclude_history=True, batch_size=8192, prior=None, news_time=None,
                      window=None, news_group=None, group_cap=None, seen=None):
    """Diversified full-corpus recommendation: Maximal Marginal Relevance over the `pool` best news of every user.  The user
    vectors, exclusions, prior and window are recommend's; the pool is drawn with ops.score_topk(k=pool) WITHOUT the caps (the
    best c per group would take away the choice MMR is there to make) and re-ranked by ops.mmr_select (include/nrhip.h, K11)
    WITH them: each step takes the news with the largest score - penalty * (largest cosine to the news already in the row).
    penalty: a float >= 0 or a [U] tensor (penalty 0 is recommend's row, bit for bit, for k <= pool <= 128); to scale it by a
    user's own score spread see INTEGRATION.md.  Returns (ids int32 [U, k], scores fp32 [U, k]): the scores are the relevance
    scores of the news taken, so a row is no longer sorted by them; a row with fewer than k news to take ends in id 0, -inf."""
    news_vecs, user, exclude, kw, caps = _recommend_args(model, news_vecs, hist_idx, mask, exclude_history, batch_size, prior, news_time, window,
                                                         news_group, group_cap, seen)
    pool_ids, pool_scores = ops.score_topk(news_vecs, user, pool, exclude=exclude, **kw)
    if isinstance(penalty, torch.Tensor):
        penalty = penalty.to(device=news_vecs.device, dtype=torch.float32)
    ids, scores, _ = ops.mmr_select(news_vecs, pool_ids, pool_scores, k, penalty, **caps)
    return ids, scores


def _retrieval_sums(ranks, ks):
    """[users with a ranked target, sum MRR_u, then per k: sum Recall@k_u, sum nDCG@k_u] in fp64 from ranks [U, T] (0 = not
    ranked; -1 = capped out: counted in n_u, nothing else): metrics.retrieval_metrics_reference as tensor arithmetic on the
    device of `ranks`."""
    pos = ranks > 0
    r = ranks.double().clamp(min=1.0)
    n = (ranks != 0).sum(1)
    nd = n.clamp(min=1).double()
    counted = (n > 0).double()
    out = [counted.sum(), (torch.where(pos, 1.0 / r, torch.zeros_like(r)).sum(1) / nd * counted).sum()]
    ideal = torch.cumsum(1.0 / torch.log2(torch.arange(ranks.shape[1], device=ranks.device).double() + 2.0), 0)
    for k in ks:
        hit = pos & (ranks <= int(k))
        dcg = torch.where(hit, 1.0 / torch.log2(r + 1.0), torch.zeros_like(r)).sum(1)
        idcg = ideal[(torch.minimum(n, torch.full_like(n, int(k))).clamp(min=1) - 1)]
        out += [(hit.sum(1).double() / nd * counted).sum(), (dcg / idcg * counted).sum()]
    return torch.stack(out)


@torch.no_grad()
def rank_eval(model, news_vecs, hist_idx, mask, targets, ks=(5, 10, 100), exclude_history=True, batch_size=8192, prior=None, news_time=None,
              window=None, seen=None):
    """Full-corpus retrieval evaluation: where does each held-out click of a user stand in that user's ranking of the WHOLE
    table `news_vecs`?  hist_idx, mask, exclude_history, seen and the user vectors are recommend's (_user_vectors; the whole
    history is excluded: up to 64 slots through the kernel's dense list, a wider one -- or any `seen`, the further news per
    user that are out of the ranking -- through ops.ExclusionLists, lists of any length); targets [U, T]: the held-out news
    indices of every user, 0 = no entry.
    Scoring and counting are one fused pass (ops.score_rank): no [U, V] score matrix, and the ranks agree with recommend's
    rows exactly (1 <= rank <= k exactly when the target is in the user's top-k row).
    Returns (ranks int32 [U, T], scores fp32 [U, T], sums fp64 [2 + 2 len(ks)]) on the device: rank 0 / score -inf for an entry
    that is 0 or out of range, excluded (a clicked news under exclude_history), NaN-scored or a repeat of an earlier entry;
    sums = [users with a ranked target, sum MRR_u, then per k: sum Recall@k_u, sum nDCG@k_u].
    More than 64 targets per user: the kernel takes 64 per row, so such a user's non-zero targets (later repeats dropped first)
    are laid over several rows that share its user vector and exclusion list -- a rank only depends on the user vector, the
    exclusions and the target itself, so the rows rank independently and exactly.  The user's metric terms, which need all its
    ranks at once (n_u, the ideal DCG), are then formed here from the gathered ranks in fp64 tensor arithmetic instead of in
    the kernel's finalize pass; the formulas are the same (metrics.retrieval_metrics_reference).
    Several ranks: the caller shards the users and the sums add; there is no collective.
    Pools: prior, news_time, window as in recommend -- the click is ranked inside the pool that was live for this user (for an
    impression: the news published in a window before it), with the prior in the score; a target outside the pool has rank 0.
    The rows of a user with more than 64 targets share its window as well.
    This call knows no group caps and describes the uncapped ranking; rank_eval_capped ranks in the capped one."""
    return _rank_eval(model, news_vecs, hist_idx, mask, targets, ks, exclude_history, batch_size, prior, news_time, window, seen, None, None)


@torch.no_grad()
def rank_eval_capped(model, news_vecs, hist_idx, mask, targets, news_group, group_cap, ks=(5, 10, 100), exclude_history=True, batch_size=8192,
                     prior=None, news_time=None, window=None, seen=None):
    """rank_eval under the group caps of recommend: news_group [N+1] integer group ids (negative = in no group) and group_cap = c.
    The ranks are the places in the capped ranking recommend(..., news_group, group_cap) serves (1 <= rank <= k exactly when the
    click is at place rank - 1 of that row, same score bits), and a click that ranking can never show (c better news of its own
    group in front of it) has rank -1 and keeps its score; in the sums it counts in n_u and adds nothing to MRR, Recall@k or
    nDCG@k, and the ideal DCG keeps its min(n_u, k) terms.  What rank_eval does not rank stays at rank 0, score -inf.  The kernel
    takes 4 targets per row here (_lib.NR_RANK_MAX_CAPPED_TARGETS), so rank_eval's several-rows layout starts at 5 targets
    instead of 65.  The number of groups is max(news_group) + 1, at most 512.  Everything else is rank_eval's; it is a function of
    its own because rank_eval's argument list is pinned."""
    if news_group is None:
        raise RuntimeError("rank_eval_capped: news_group is None; the call without caps is rank_eval")
    return _rank_eval(model, news_vecs, hist_idx, mask, targets, ks, exclude_history, batch_size, prior, news_time, window, seen, news_group, group_cap)


def _rank_eval(model, news_vecs, hist_idx, mask, targets, ks, exclude_history, batch_size, prior, news_time, window, seen, news_group, group_cap):
    """rank_eval (news_group None: ops.score_rank) and rank_eval_capped (ops.score_rank_capped)."""
    device = news_vecs.device
    hist = torch.as_tensor(hist_idx).to(device=device, dtype=torch.int32)
    m = torch.as_tensor(mask).to(device=device, dtype=torch.float32)
    tg = torch.as_tensor(targets).to(device=device, dtype=torch.int32)
    news_vecs = news_vecs.detach().float().contiguous()
    user = _user_vectors(model, news_vecs, hist, m, batch_size, device, _Histories(mask))
    exclude = _exclusions(hist, m, exclude_history, seen, device)
    U, T = tg.shape
    W = _lib.NR_RANK_MAX_TARGETS
    pool = _pool_kwargs(device, prior, news_time, window)
    score_rank = ops.score_rank
    if news_group is not None:
        grp = torch.as_tensor(news_group)
        pool["n_groups"] = max(int(grp.max()) + 1, 1) if grp.numel() else 1
        pool["group"] = grp.to(device=device, dtype=torch.int32)
        pool["group_cap"] = group_cap
        score_rank, W = ops.score_rank_capped, _lib.NR_RANK_MAX_CAPPED_TARGETS
    if T <= W or U == 0:
        return score_rank(news_vecs, user, tg, exclude=exclude, ks=ks, **pool)
    # later repeats -> 0 (stable sort by id: the first of equal ids is the earliest entry), then the non-zero entries to the front
    srt, at = torch.sort(tg, dim=1, stable=True)
    rep = torch.zeros_like(tg, dtype=torch.bool)
    rep[:, 1:] = srt[:, 1:] == srt[:, :-1]
    tg = tg.masked_fill(torch.zeros_like(rep).scatter(1, at, rep), 0)
    order = torch.argsort((tg == 0).to(torch.int8), dim=1, stable=True)
    comp = tg.gather(1, order)
    n_rows = (((tg != 0).sum(1) + W - 1) // W).clamp(min=1)
    row_user = torch.repeat_interleave(torch.arange(U, device=device), n_rows)
    block = torch.arange(row_user.numel(), device=device) - (torch.cumsum(n_rows, 0) - n_rows)[row_user]
    cols = block[:, None] * W + torch.arange(W, device=device)[None, :]
    live = cols < T
    cols = cols.clamp(max=T - 1)
    row_tg = (comp[row_user[:, None], cols] * live).contiguous()
    if "window" in pool:
        pool["window"] = pool["window"][row_user].contiguous()
    if isinstance(exclude, ops.ExclusionLists):
        row_excl = exclude.take(row_user)                     # the rows of a user share its lists
    else:
        row_excl = None if exclude is None else exclude[row_user].contiguous()
    r, sc, _ = score_rank(news_vecs, user[row_user].contiguous(), row_tg, exclude=row_excl, ks=None, **pool)
    ranks_c = torch.zeros(U, T, dtype=torch.int32, device=device)
    scores_c = torch.full((U, T), float("-inf"), dtype=torch.float32, device=device)
    ru = row_user[:, None].expand_as(cols)
    ranks_c[ru[live], cols[live]] = r[live]
    scores_c[ru[live], cols[live]] = sc[live]
    ranks = torch.zeros_like(ranks_c).scatter(1, order, ranks_c)
    scores = torch.zeros_like(scores_c).scatter(1, order, scores_c)
    return ranks, scores, _retrieval_sums(ranks, ks)


def _shard_targets(shard: IndexedTestShard):
    """The clicked candidates of every impression of a shard, cand[label == 1] per CSR row in list order, as one int32 array
    [n, T] (T = the most clicks of an impression, at least 1), rows back padded with 0."""
    n = len(shard)
    clicked = shard.label == 1
    imp = np.repeat(np.arange(n), np.diff(shard.offsets))[clicked]
    per = np.bincount(imp, minlength=n)
    out = np.zeros((n, max(int(per.max()) if n else 0, 1)), dtype=np.int32)
    start = np.cumsum(per) - per
    out[imp, np.arange(len(imp)) - start[imp]] = shard.cand[clicked]
    return out


@torch.no_grad()
def rank_shard(model, news_vecs, shard: IndexedTestShard, ks=(5, 10, 100), prior=None, news_time=None, window=None, seen=None):
    """rank_eval over the impressions of a test shard: every impression is one user (its history), its targets are the news it
    clicked, cand[label == 1] per CSR row in list order, rows back padded with 0.  Returns rank_eval's (ranks, scores, sums).
    prior, news_time, window: rank_eval's pools, window [impressions, 2]; the shard holds no times, the caller supplies them.
    seen: rank_eval's, one list per impression."""
    return rank_eval(model, news_vecs, shard.hist, shard.mask, _shard_targets(shard), ks=ks, prior=prior, news_time=news_time, window=window,
                     seen=seen)


@torch.no_grad()
def rank_shard_capped(model, news_vecs, shard: IndexedTestShard, news_group, group_cap, ks=(5, 10, 100), prior=None, news_time=None, window=None,
                      seen=None):
    """rank_shard under group caps: rank_eval_capped over the impressions of a test shard."""
    return rank_eval_capped(model, news_vecs, shard.hist, shard.mask, _shard_targets(shard), news_group, group_cap, ks=ks, prior=prior,
                            news_time=news_time, window=window, seen=seen)


@torch.no_grad()
def test(rank, args, model, news_index, news_combined, log=logging.info, collect_scores=None, device=None, score_fn=None):
    """One rank of the evaluation job (src/main.py:145-277) on `behaviors_{rank}.tsv`.

    Returns (n_samples, means): n_samples = impressions seen by all ranks, means = [AUC, MRR, nDCG@5, nDCG@10].
    Divisor, as the reference: a single process averages over the SCORED impressions (those with both classes,
    src/main.py:250,275); a distributed run divides the reduced sums by ALL impressions seen (src/main.py:269-273
    reduces `local_sample_num`, which counts the skipped ones too).  `args.eval_divide_by_scored=True` uses the scored
    count in both cases.
    `collect_scores`: optional list that receives (labels, scores) numpy pairs of every impression of this rank.
    `score_fn(model, news_vecs, shard, batch_size, device) -> (scores, sums[5])` defaults to `score_shard` (device)."""
    is_distributed = rank is not None
    rank = rank or 0
    device = torch.device(device) if device is not None else next(model.parameters()).device
    if is_distributed:
        parallel.init_distributed(rank, getattr(args, "nGPU", None), device=device)                  # src/main.py:154
    model.eval()
    news_vecs = encode_news(model, news_combined, args.batch_size, device,
                            shard_over_ranks=is_distributed and getattr(args, "shard_encode", True))
    shard = IndexedTestShard(os.path.join(args.test_data_dir, f"behaviors_{rank}.tsv"), news_index, args)
    scores, sums = (score_fn or score_shard)(model, news_vecs, shard, args.batch_size, device)
    if collect_scores is not None:
        s = scores.cpu().numpy()
        for i in range(len(shard)):
            a, b = shard.offsets[i], shard.offsets[i + 1]
            collect_scores.append((shard.label[a:b], s[a:b]))
    sums = [float(x) for x in (sums.cpu().tolist() if torch.is_tensor(sums) else sums)]
    n_samples, n_scored, metric_sums = parallel.reduce_eval_sums(len(shard), sums[0], sums[1:], device)
    by_scored = getattr(args, "eval_divide_by_scored", False) or not is_distributed
    means = np.asarray(metric_sums) / max(n_scored if by_scored else n_samples, 1)
    if rank == 0:
        log("[*] {} samples: {}".format(n_samples, "\t".join("{:0.2f}".format(x * 100) for x in means)))
    return n_samples, means
