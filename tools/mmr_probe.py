#!/usr/bin/env python
"""Diversified recommendation: the re-ranking (ops.mmr_select) beside the pool draw it follows (ops.score_topk(k = M)).

    python tools/mmr_probe.py [--news 100001] [--dim 400] [--users 64 8192] [--pools 32 128] [--k 10 0] [--penalty 1.0]
                              [--calls 30] [--warmup 5] [--out FILE]

Per (U, M, k; k = 0 means k = M): the pool is drawn once, then every call is timed with a pair of device events, the two calls
alternate call by call (so that a disturbance of the machine hits both), and the median, minimum, maximum and inter-quartile
spread of the timed calls are reported.  The re-ranking's rate counts the Gram matrix it forms, U * Mp^2 * N * 2 FLOPs with
Mp = 32 * ceil(M / 32), against the 155 TFLOP/s measured for fp32 MFMA.  One JSON line per (U, M, k).  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from newsrecommendation_amd import ops  # noqa: E402

PEAK_FP32_MFMA = 155e12


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms):
    a = np.asarray(ms)
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return {"median_ms": round(float(med), 4), "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4),
            "iqr_ms": round(float(q3 - q1), 4), "calls": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--news", type=int, default=100001)
    ap.add_argument("--dim", type=int, default=400)
    ap.add_argument("--users", type=int, nargs="+", default=[64, 8192])
    ap.add_argument("--pools", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 0], help="0 = the whole pool (k = M)")
    ap.add_argument("--penalty", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mmr_probe needs a GPU")
    if args.calls < 20:
        raise SystemExit("at least 20 timed calls")
    g = torch.Generator().manual_seed(0)
    news = (torch.randn(args.news, args.dim, generator=g) * 0.4).cuda()
    lines = []
    for U in args.users:
        user = (torch.randn(U, args.dim, generator=g) * 0.4).cuda()
        for M in args.pools:
            pool_ids, pool_sc = ops.score_topk(news, user, M)
            for k in args.k:
                k = M if k == 0 else min(k, M)
                draw = lambda: ops.score_topk(news, user, M)
                rerank = lambda: ops.mmr_select(news, pool_ids, pool_sc, k, args.penalty)
                for _ in range(args.warmup):
                    draw()
                    rerank()
                torch.cuda.synchronize()
                t_d, t_r = [], []
                for _ in range(args.calls):
                    t_d.append(timed(draw))
                    t_r.append(timed(rerank))
                place = rerank()[2]
                mp = 32 * ((M + 31) // 32)
                row = {"U": U, "V": args.news, "N": args.dim, "M": M, "k": k, "penalty": args.penalty, "pool_draw": stats(t_d), "mmr_select": stats(t_r)}
                row["mmr_over_pool_draw"] = round(row["mmr_select"]["median_ms"] / row["pool_draw"]["median_ms"], 4)
                row["gram_tflops"] = round(2.0 * U * mp * mp * args.dim / (row["mmr_select"]["median_ms"] * 1e-3) / 1e12, 2)
                row["fraction_of_fp32_mfma_peak"] = round(row["gram_tflops"] * 1e12 / PEAK_FP32_MFMA, 4)
                row["moved_fraction"] = round(float((place != torch.arange(k, device=place.device)[None, :]).float().mean()), 4)
                lines.append(row)
                print(json.dumps(row), flush=True)
        del user
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
