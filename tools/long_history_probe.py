#!/usr/bin/env python
"""Long clicked histories (64 < L <= 128): what the new kernels cost.  Two measurements, one JSON line each.

  core   the bf16 attention core (nr_sdpa_long_fwd / nr_sdpa_long_bwd) at n = 512, L = 100, 20 heads of 20: the aligned call
         (matrix-core route, attn_long_*) against the same call with qkv one element into its buffer
         (LDS/VALU route, attn_fwd[ / attn_bwd[).  HIP events around each call, 30 calls after 5 warm-ups: median and
         min .. max.  "mfma_pays" says whether the matrix-core median beats the LDS/VALU median by more than both spreads.
  step   one NRMS and one NAML training step (fwd + bwd + fused Adam, bench.py's model set-up) at B = 512, bf16, with
         user_log_length = 100 next to 50 in the same run.  The expectation is about the ratio of titles per impression,
         105 / 55 = 1.9; the news level dominates both.

  python tools/long_history_probe.py [--only core|step] [--batch 512]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from newsrecommendation_amd import _lib, parallel  # noqa: E402
from newsrecommendation_amd.model import NAML, NRMS  # noqa: E402


def _timed(fn, calls=30, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def core_probe(n=512, L=100, heads=20, d=20):
    dev, N = torch.device("cuda", 0), heads * d
    g = torch.Generator().manual_seed(1)
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    mask = (torch.rand(n, L, generator=g) < 0.8).float().to(dev)
    out = {"probe": "core", "n": n, "L": L, "heads": heads, "d_head": d, "dtype": "bf16"}

    def view(numel, off):                                 # a contiguous run `off` elements into a 16-byte aligned buffer
        return torch.zeros(numel + 16, dtype=torch.bfloat16, device=dev)[off:off + numel]

    for name, off in (("mfma_aligned", 0), ("valu_misaligned", 1)):
        qkv, y, dy, dqkv = view(n * L * 3 * N, off), view(n * L * N, 0), view(n * L * N, 0), view(n * L * 3 * N, 0)
        qkv.copy_((torch.randn(n * L * 3 * N, generator=g) * 0.7).to(torch.bfloat16))
        dy.copy_(torch.randn(n * L * N, generator=g).to(torch.bfloat16))
        args = (n, L, heads, d, _lib.NR_BF16, 0.0, 0, stream)
        fwd = lambda: _lib.check(lib.nr_sdpa_long_fwd(_lib.ptr(qkv), _lib.ptr(mask), _lib.ptr(y), *args), "fwd")
        bwd = lambda: _lib.check(lib.nr_sdpa_long_bwd(_lib.ptr(qkv), _lib.ptr(mask), _lib.ptr(dy), _lib.ptr(dqkv), *args), "bwd")
        _lib.prof_enable(1)
        _lib.prof_collect()
        fwd(); bwd()
        torch.cuda.synchronize()
        labels = sorted(k for k in _lib.prof_collect() if k.startswith("attn_"))
        _lib.prof_enable(0)
        out[name] = {"labels": labels, "fwd": _timed(fwd), "bwd": _timed(bwd)}
    for p in ("fwd", "bwd"):
        a, b = out["mfma_aligned"][p], out["valu_misaligned"][p]
        spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
        out[p + "_mfma_pays"] = bool(b["median_ms"] - a["median_ms"] > spread)
        out[p + "_ratio_valu_over_mfma"] = round(b["median_ms"] / a["median_ms"], 2)
    return out


def step_probe(B=512, steps=10, warmup=3):
    dev = torch.device("cuda", 0)
    out = {"probe": "step", "batch": B, "dtype": "bf16", "steps": steps}
    for model_name in ("NRMS", "NAML"):
        for Hn in (50, 100):
            args = bench.make_args("bf16")
            args.user_log_length = Hn
            torch.manual_seed(0)
            g = torch.Generator().manual_seed(1)
            if model_name == "NRMS":
                table = torch.randn(30000, args.word_embedding_dim, generator=g) * 0.4
                table[0] = 0
                model = NRMS.Model(args, table.numpy()).to(dev).train()
                batches = bench.synth_batches(args, B, 30000, 4, 100, dev)
            else:
                n_news = 8000
                args.use_category = args.use_subcategory = True
                args.freeze_embedding = True
                table = torch.randn(n_news + 1, args.num_words_title * args.word_embedding_dim, generator=g) * 0.4
                table[0] = 0
                model = NAML.Model(args, table.numpy(), 17, 264).to(dev).train()
                batches = bench.synth_batches_naml(args, B, n_news, 4, 100, dev)
            del table
            bucket = parallel.FlatBucket(model, lr=1e-4)

            def step(i):
                hist, mask, cand, label = batches[i % len(batches)]
                loss, _ = model(hist, mask, cand, label)
                loss.backward()
                bucket.step()
                return loss

            for i in range(warmup):
                step(i)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(steps):
                loss = step(warmup + i)
            e1.record()
            torch.cuda.synchronize()
            out[f"{model_name}_H{Hn}_ms_per_step"] = round(e0.elapsed_time(e1) / steps, 3)
            out[f"{model_name}_H{Hn}_final_loss"] = round(float(loss), 4)
            del model, bucket, batches
            torch.cuda.empty_cache()
        out[f"{model_name}_ratio_H100_over_H50"] = round(out[f"{model_name}_H100_ms_per_step"] / out[f"{model_name}_H50_ms_per_step"], 2)
    out["titles_per_impression_ratio"] = round(105 / 55, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["core", "step"], default=None)
    ap.add_argument("--batch", type=int, default=512)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.only in (None, "core"):
        print(json.dumps(core_probe()), flush=True)
    if a.only in (None, "step"):
        print(json.dumps(step_probe(a.batch)), flush=True)


if __name__ == "__main__":
    main()
