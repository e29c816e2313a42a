#!/usr/bin/env python
"""Full-corpus top-k recommendation: the fused call (ops.score_topk) against torch.matmul + torch.topk on the same device.

    python tools/topk_probe.py [--news 100001] [--dim 400] [--k 10] [--users 64 8192] [--calls 30] [--warmup 5] [--out FILE] [--pool]
                                [--group G --group-cap C] [--seen L]

Both sides take the same fp32 inputs.  Per U: every call is timed with a pair of device events, the two sides alternate call
by call (so that a disturbance of the machine hits both), and the median, minimum, maximum and inter-quartile spread of the
timed calls are reported, with the peak device memory of one call above what the inputs occupy.  The fused side's share of the
fp32 MFMA peak counts the algorithmic 2 * U * V * N FLOPs over the WHOLE call (both launches), against 157.3 TFLOP/s.
One JSON line per U, and a last line with the two requirements at the largest U.  Needs a GPU: there is nothing to fall back to.
--pool: instead of the baseline, the same fused call with a prior and a window (ops.score_topk(..., prior=, stamp=, window=)) at
the same shapes, alternating with the plain fused call and timed the same way; one JSON line per U with both and their ratio.
--group G --group-cap C: likewise, the fused call with group caps (ops.score_topk(..., group=, group_cap=C); G random groups,
MIND has 18 categories) alternating with the plain fused call; one JSON line per U with both, their ratio and the plain call's
inter-quartile spread beside the difference of the medians.
--seen L: likewise, the fused call with a list of L random ids per user through the CSR path (ops.ExclusionLists, built once)
alternating with the fused call with the dense list of 50 random ids per user (E = 50); one JSON line per U with both and the
ratio of the medians."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from newsrecommendation_amd import ops  # noqa: E402

PEAK_FP32_MATRIX = 157.3e12


def fused(news, user, k):
    return ops.score_topk(news, user, k)


def baseline(news, user, k):
    sc, ids = torch.topk(torch.matmul(user, news[1:].T), k, dim=1)          # row 0 is the padding news
    return ids + 1, sc


def timed(fn, *a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(*a)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def peak_bytes(fn, *a):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn(*a)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def write(out, lines):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


def stats(ms):
    a = np.asarray(ms)
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return {"median_ms": round(float(med), 4), "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4),
            "iqr_ms": round(float(q3 - q1), 4), "calls": len(ms)}


def pool_inputs(V, U, g):
    """The inputs of --pool: a float prior with a tenth of the news switched off (-inf), stamps 0 .. 999 and per user a window
    that is 500 stamps wide (about half of the corpus is in a user's pool)."""
    prior = torch.randn(V, generator=g) * 0.1
    prior[torch.rand(V, generator=g) < 0.1] = float("-inf")
    stamp = torch.randint(0, 1000, (V,), generator=g, dtype=torch.int32)
    lo = torch.randint(0, 500, (U,), generator=g, dtype=torch.int32)
    return prior.cuda(), stamp.cuda(), torch.stack([lo, lo + 499], 1).contiguous().cuda()


def pool_row(plain, pooled, calls, warmup):
    """--pool: the plain fused call and the pooled one, alternating, timed as everything else here."""
    for _ in range(warmup):
        plain()
        pooled()
    torch.cuda.synchronize()
    t_p, t_q = [], []
    for _ in range(calls):
        t_p.append(timed(plain))
        t_q.append(timed(pooled))
    row = {"mode": "pool", "plain": stats(t_p), "pooled": stats(t_q)}
    row["pooled_over_plain"] = round(row["pooled"]["median_ms"] / row["plain"]["median_ms"], 4)
    return row


def group_row(plain, capped, calls, warmup):
    """--group: the plain fused call and the capped one, alternating, timed as everything else here."""
    row = pool_row(plain, capped, calls, warmup)
    row = {"mode": "group", "plain": row["plain"], "capped": row["pooled"]}
    row["capped_over_plain"] = round(row["capped"]["median_ms"] / row["plain"]["median_ms"], 4)
    row["capped_minus_plain_ms"] = round(row["capped"]["median_ms"] - row["plain"]["median_ms"], 4)
    return row


def seen_row(dense, csr, calls, warmup):
    """--seen: the fused call with the dense list and the one with CSR lists, alternating, timed as everything else here."""
    row = pool_row(dense, csr, calls, warmup)
    row = {"mode": "seen", "dense": row["plain"], "csr": row["pooled"]}
    row["csr_over_dense"] = round(row["csr"]["median_ms"] / row["dense"]["median_ms"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--news", type=int, default=100001)
    ap.add_argument("--dim", type=int, default=400)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--users", type=int, nargs="+", default=[64, 8192])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pool", action="store_true", help="time the pooled fused call against the plain fused call")
    ap.add_argument("--group", type=int, default=0, help="with --group-cap: time the capped fused call (this many random groups) against the plain one")
    ap.add_argument("--group-cap", type=int, default=0)
    ap.add_argument("--seen", type=int, default=0, help="time the fused call with L random ids per user in CSR lists against the dense list of 50")
    args = ap.parse_args()
    if (args.group > 0) != (args.group_cap > 0) or (args.group > 0 and args.pool):
        raise SystemExit("--group G and --group-cap C come together, and not with --pool")
    if args.seen and (args.pool or args.group):
        raise SystemExit("--seen L comes alone")
    if not torch.cuda.is_available():
        raise SystemExit("topk_probe needs a GPU")
    if args.calls < 20:
        raise SystemExit("at least 20 timed calls")
    g = torch.Generator().manual_seed(0)
    news = (torch.randn(args.news, args.dim, generator=g) * 0.4).cuda()
    lines = []
    for U in args.users:
        user = (torch.randn(U, args.dim, generator=g) * 0.4).cuda()
        if args.seen:
            dense = torch.randint(1, args.news, (U, 50), generator=g, dtype=torch.int32).cuda()
            lists = ops.ExclusionLists(torch.randint(1, args.news, (U, args.seen), generator=g, dtype=torch.int32).cuda())
            row = {"U": U, "V": args.news, "N": args.dim, "k": args.k, "E": 50, "seen": args.seen, "listed_ids": int(lists.ids.numel())}
            row.update(seen_row(lambda: ops.score_topk(news, user, args.k, exclude=dense), lambda: ops.score_topk(news, user, args.k, exclude=lists),
                                args.calls, args.warmup))
            lines.append(row)
            print(json.dumps(row), flush=True)
            continue
        if args.group:
            group = torch.randint(0, args.group, (args.news,), generator=g, dtype=torch.int32).cuda()
            row = {"U": U, "V": args.news, "N": args.dim, "k": args.k, "groups": args.group, "group_cap": args.group_cap}
            row.update(group_row(lambda: ops.score_topk(news, user, args.k), lambda: ops.score_topk(news, user, args.k, group=group, group_cap=args.group_cap),
                                 args.calls, args.warmup))
            row["filled_fraction"] = round(float((ops.score_topk(news, user, args.k, group=group, group_cap=args.group_cap)[0] != 0).float().mean()), 6)
            lines.append(row)
            print(json.dumps(row), flush=True)
            continue
        if args.pool:
            prior, stamp, window = pool_inputs(args.news, U, g)
            row = {"U": U, "V": args.news, "N": args.dim, "k": args.k}
            row.update(pool_row(lambda: ops.score_topk(news, user, args.k), lambda: ops.score_topk(news, user, args.k, prior=prior, stamp=stamp, window=window),
                                args.calls, args.warmup))
            row["filled_fraction"] = round(float((ops.score_topk(news, user, args.k, prior=prior, stamp=stamp, window=window)[0] != 0).float().mean()), 6)
            lines.append(row)
            print(json.dumps(row), flush=True)
            continue
        for _ in range(args.warmup):
            fused(news, user, args.k)
            baseline(news, user, args.k)
        torch.cuda.synchronize()
        t_f, t_b = [], []
        for _ in range(args.calls):
            t_f.append(timed(fused, news, user, args.k))
            t_b.append(timed(baseline, news, user, args.k))
        ids_f, sc_f = fused(news, user, args.k)
        ids_b, sc_b = baseline(news, user, args.k)
        row = {"U": U, "V": args.news, "N": args.dim, "k": args.k, "fused": stats(t_f), "baseline": stats(t_b),
               "fused_peak_bytes": peak_bytes(fused, news, user, args.k), "baseline_peak_bytes": peak_bytes(baseline, news, user, args.k),
               "score_matrix_bytes": U * (args.news - 1) * 4,
               "ids_equal_fraction": round(float((ids_f.long() == ids_b).float().mean()), 6),
               "max_score_diff": float((sc_f - sc_b).abs().max())}
        flops = 2.0 * U * args.news * args.dim
        row["fused_tflops"] = round(flops / (row["fused"]["median_ms"] * 1e-3) / 1e12, 2)
        row["fused_fraction_of_fp32_mfma_peak"] = round(row["fused_tflops"] * 1e12 / PEAK_FP32_MATRIX, 4)
        row["baseline_tflops"] = round(flops / (row["baseline"]["median_ms"] * 1e-3) / 1e12, 2)
        lines.append(row)
        print(json.dumps(row), flush=True)
        del user
    if args.pool or args.group or args.seen:
        write(args.out, lines)
        return
    last = lines[-1]
    spread = max(last["fused"]["iqr_ms"], last["baseline"]["iqr_ms"])
    verdict = {"U": last["U"], "spread_ms": spread,
               "time_ok": last["fused"]["median_ms"] <= last["baseline"]["median_ms"] + spread,
               "memory_ok": last["baseline_peak_bytes"] - last["fused_peak_bytes"] >= last["score_matrix_bytes"]}
    lines.append(verdict)
    print(json.dumps(verdict), flush=True)
    write(args.out, lines)


if __name__ == "__main__":
    main()
