#!/usr/bin/env python
"""NAML training step with a TRAINABLE title table (freeze_embedding=False, the reference's default) -- the configuration
bench.py's NAML leg does not run (it forces the table frozen, src/demo.sh:12).

B = 512, 65 000 news (a [65 001, 9 000] fp32 table: 2.34 GB, and as much again for its gradient and each Adam moment), 3
views, bf16, flat bucket + fused Adam, batches resident on the device.  W untimed warm-up steps, then K steps between
HIP events, as bench.py times them.  Prints one JSON line: ms per step, impressions/s, peak device memory.

  --profile   one more step with the library's per-launch events on: per-kernel ms, the summed time of the table-gradient
              kernels, and the Adam launch with its bytes / time (16 B read + 12 B written per bucket element, + 2 B per
              element of a table whose packed bf16 copy it rewrites)
  --table-adam deferred   parallel.FlatBucket(table_adam="deferred"): the table is stepped row by row (nr_adam_rows), bit-identical
              to the dense update; --profile then also reports the adam_rows_* launches, their summed time, the number of unique
              rows the step updated and the bytes / time of the row kernels (a caught-up row: p, m, v read and written, a stepped
              row: p, g, m, v read and written, + 2 B per element of the packed bf16 copy each time); --flush-after N times a flush after N steps
  --frozen    the same step with the table frozen (nn.Embedding, freeze=True): the frozen run's Adam and conv forward
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from newsrecommendation_amd import _lib, parallel  # noqa: E402
from newsrecommendation_amd.model import NAML  # noqa: E402

TABLE_KERNELS = ("conv_table_live", "conv_table_stage", "gemm_nt_dma_live[bf16,epi=0,", "sort_rows_by_id", "conv_table_rank",
                 "conv_table_scatter")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--news", type=int, default=65000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--frozen", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--table-adam", default="dense", choices=["dense", "deferred"])
    ap.add_argument("--flush-after", type=int, default=0, help="deferred: also time a flush after this many further steps")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    args = bench.make_args(a.dtype)
    args.use_category = args.use_subcategory = True
    args.freeze_embedding, args.stream_title_table = bool(a.frozen), False
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    width = args.num_words_title * args.word_embedding_dim
    table = torch.empty(a.news + 1, width)
    for r0 in range(0, a.news + 1, 8192):
        table[r0:r0 + 8192] = torch.randn(min(8192, a.news + 1 - r0), width, generator=g) * 0.4
    table[0] = 0
    model = NAML.Model(args, table.numpy(), 17, 264).to(dev).train()
    del table
    bucket = parallel.FlatBucket(model, lr=1e-4, table_adam=a.table_adam)
    batches = bench.synth_batches_naml(args, a.batch, a.news, 4, 100, dev)

    def step(i):
        hist, mask, cand, label = batches[i % len(batches)]
        loss, _ = model(hist, mask, cand, label)
        loss.backward()
        bucket.step()
        return loss

    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(a.steps):
        loss = step(a.warmup + i)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    out = {"config": {"model": "NAML", "batch": a.batch, "news": a.news, "dtype": a.dtype, "freeze_embedding": bool(a.frozen),
                      "optimizer": "dense Adam over the flat bucket (reference-default semantics)" if a.table_adam == "dense" else
                      "flat bucket, table rows stepped on demand (table_adam=deferred: dense Adam's values)", "bucket_elements": bucket.numel,
                      "final_loss": float(loss)},
           "ms_per_step": round(ms, 3), "impressions_per_s": round(a.batch / ms * 1e3, 1),
           "peak_device_GB": round(torch.cuda.max_memory_allocated() / 1e9, 2)}
    if a.profile:
        if a.table_adam == "deferred":                              # rows of the profiled step: unique ones, and those a step or more behind
            hist, mask, cand, label = batches[(a.warmup + a.steps) % len(batches)]
            ids = torch.cat([cand.reshape(-1, cand.shape[-1])[:, 0], hist.reshape(-1, hist.shape[-1])[:, 0]]).long()
            uniq = torch.unique(ids[ids > 0])
            n_unique, n_behind = int(uniq.numel()), int((bucket._row_step[uniq] < bucket.t).sum())
        _lib.prof_enable(1)
        _lib.prof_collect()
        step(a.warmup + a.steps)
        torch.cuda.synchronize()
        prof = _lib.prof_collect()
        _lib.prof_enable(0)
        out["kernels_ms"] = {k: round(v[1], 4) for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])}
        tk = {k: v[1] for k, v in prof.items() if k.startswith(TABLE_KERNELS)}
        out["table_gradient_kernels_ms"] = {k: round(v, 4) for k, v in tk.items()}
        out["table_gradient_ms"] = round(sum(tk.values()), 4)
        conv = [v[1] for k, v in prof.items() if k.startswith("gemm_nt_dma") and ",gap=%d]" % args.num_words_title in k and "epi=0" in k
                and not k.startswith("gemm_nt_dma_live")]
        out["conv_forward_gemm_ms"] = round(sum(conv), 4)
        adam = [v[1] for k, v in prof.items() if k.startswith("adam_step")]
        if adam:
            packed = sum(p.numel() for p in bucket.params if p.numel() >= (1 << 20)) if a.dtype == "bf16" else 0
            nbytes = bucket.numel * 28 + packed * 2
            out["adam_ms"], out["adam_GB"], out["adam_TBps"] = round(adam[0], 4), round(nbytes / 1e9, 2), round(nbytes / adam[0] / 1e9, 3)
        rows_k = {k: v[1] for k, v in prof.items() if k.startswith("adam_rows_")}
        if rows_k:
            pk = width * 2 if a.dtype == "bf16" else 0              # the packed bf16 copy of a row, rewritten with it
            out["adam_rows_kernels_ms"] = {k: round(v, 4) for k, v in rows_k.items()}
            out["adam_rows_ms"] = round(sum(rows_k.values()), 4)
            out["unique_rows_updated"], out["rows_caught_up"] = n_unique, n_behind
            for k, v in rows_k.items():
                if k.startswith("adam_rows_apply") and v > 0:
                    nbytes = n_behind * (6 * width * 4 + pk) if "apply=0" in k else n_unique * (8 * width * 4 + pk)
                    out.setdefault("adam_rows_apply_TBps", {})[k] = round(nbytes / v / 1e9, 3)
    if a.flush_after and a.table_adam == "deferred":
        for i in range(a.flush_after):
            step(a.warmup + a.steps + 1 + i)
        torch.cuda.synchronize()
        e0.record()
        bucket.flush()
        e1.record()
        torch.cuda.synchronize()
        out["flush_ms_after_%d_steps" % a.flush_after] = round(e0.elapsed_time(e1), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
