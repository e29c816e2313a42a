#!/usr/bin/env python
"""Full-corpus rank evaluation: the fused call (ops.score_rank) against torch.matmul in user blocks + (scores > target).sum on
the same device.

    python tools/rank_probe.py [--news 100001] [--dim 400] [--targets 4] [--exclude 50] [--users 64 8192] [--block 1024]
                               [--calls 30] [--warmup 5] [--out FILE] [--pool] [--seen L] [--group G --group-cap c]

Both sides take the same fp32 inputs.  The baseline forms the [block, V] scores of a block of users, reads the targets' scores
out of them and counts, per target, the news that score strictly higher (what the excluded ones contribute is taken back from
the gathered excluded scores); it leaves out the tie rule, the duplicate handling and the metric sums, all of which the fused
call does.  Per U: every call is timed with a pair of device events, the two sides alternate call by call (so that a
disturbance of the machine hits both), and the median, minimum, maximum and inter-quartile spread of the timed calls are
reported, with the peak device memory of one call above what the inputs occupy.  The fused side's share of the fp32 MFMA peak
counts the algorithmic 2 * U * V * N FLOPs over the WHOLE call (all launches), against 157.3 TFLOP/s.
One JSON line per U, and a last line with the two requirements at the largest U.  Needs a GPU: there is nothing to fall back to.
--pool: instead of the baseline, the same fused call with a prior and a window (ops.score_rank(..., prior=, stamp=, window=)) at
the same shapes, alternating with the plain fused call and timed the same way; one JSON line per U with both and their ratio.
--seen L: likewise, the fused call with a list of L random ids per user through the CSR path (ops.ExclusionLists, built once)
alternating with the fused call with the dense list (--exclude ids per user); one JSON line per U with both, the ratio of the
medians and, from the library's own launch timer, the share of the named-id pass in each call beside the arithmetic
2 % x (1 + ceil((L - 64) / 128)).
--group G --group-cap c: likewise, the capped fused call (ops.score_rank_capped(..., group, group_cap, n_groups=G): G random groups,
every tenth news in none, at most 4 targets per row) alternating with the plain fused call; one JSON line per U with both, the
ratio of the medians, the fractions of capped-out (-1) targets and of targets the cap moved up, and from the library's launch
timer the share of the mask and counting launches.  The arithmetic beside it: about 8 VALU instructions per (chunk, user,
target, block of 64 groups) against 416 MFMAs per wave and chunk at N = 400."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from newsrecommendation_amd import _lib, ops  # noqa: E402

PEAK_FP32_MATRIX = 157.3e12
KS = (5, 10, 100)


def fused(news, user, targets, exclude, block):
    return ops.score_rank(news, user, targets, exclude=exclude, ks=KS)


def baseline(news, user, targets, exclude, block):
    ranks = torch.empty(targets.shape, dtype=torch.int64, device=targets.device)
    for a in range(0, user.shape[0], block):
        sc = torch.matmul(user[a:a + block], news.T)                          # [block, V]
        sc[:, 0] = float("-inf")                                              # row 0 is the padding news
        t = sc.gather(1, targets[a:a + block].long())                         # [block, T]
        x = sc.gather(1, exclude[a:a + block].long())                         # [block, E]
        above = torch.stack([(sc > t[:, j:j + 1]).sum(1) for j in range(t.shape[1])], 1)
        ranks[a:a + block] = 1 + above - (x[:, None, :] > t[:, :, None]).sum(2)
    return ranks


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


def launch_shares(call, prefixes, reps=5):
    """The share of the launches whose label starts with each prefix in the launches of `call`, by the library's per-launch timer."""
    call()
    torch.cuda.synchronize()
    _lib.prof_enable(1)
    _lib.prof_collect()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    got = _lib.prof_collect()
    _lib.prof_enable(0)
    total = sum(ms for _, ms in got.values())
    return {p: round(sum(ms for label, (_, ms) in got.items() if label.startswith(p)) / total, 4) if total > 0 else None for p in prefixes}


def named_share(call, reps=5):
    """The share of the named-id pass in the launches of `call`, by the library's per-launch timer."""
    call()
    torch.cuda.synchronize()
    _lib.prof_enable(1)
    _lib.prof_collect()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    got = _lib.prof_collect()
    _lib.prof_enable(0)
    total = sum(ms for _, ms in got.values())
    named = sum(ms for label, (_, ms) in got.items() if label.startswith("rank_named"))
    return round(named / total, 4) if total > 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--news", type=int, default=100001)
    ap.add_argument("--dim", type=int, default=400)
    ap.add_argument("--targets", type=int, default=4)
    ap.add_argument("--exclude", type=int, default=50)
    ap.add_argument("--users", type=int, nargs="+", default=[64, 8192])
    ap.add_argument("--block", type=int, default=1024, help="users per matmul of the baseline")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pool", action="store_true", help="time the pooled fused call against the plain fused call")
    ap.add_argument("--seen", type=int, default=0, help="time the fused call with L random ids per user in CSR lists against the dense list")
    ap.add_argument("--group", type=int, default=0, help="with --group-cap: time the capped fused call (this many random groups) against the plain one")
    ap.add_argument("--group-cap", type=int, default=0)
    args = ap.parse_args()
    if args.seen and args.pool:
        raise SystemExit("--seen L comes alone")
    if bool(args.group) != bool(args.group_cap) or (args.group and (args.pool or args.seen)):
        raise SystemExit("--group G and --group-cap c come together, and alone")
    if args.group and args.targets > _lib.NR_RANK_MAX_CAPPED_TARGETS:
        raise SystemExit(f"a capped call takes at most {_lib.NR_RANK_MAX_CAPPED_TARGETS} targets per row")
    if not torch.cuda.is_available():
        raise SystemExit("rank_probe needs a GPU")
    if args.calls < 20:
        raise SystemExit("at least 20 timed calls")
    g = torch.Generator().manual_seed(0)
    news = (torch.randn(args.news, args.dim, generator=g) * 0.4).cuda()
    lines = []
    for U in args.users:
        user = (torch.randn(U, args.dim, generator=g) * 0.4).cuda()
        # distinct ids per user: the first T are the targets, the next E the excluded ones (no target is excluded)
        # (a random start per user, then steps of a prime that shares no factor with V - 1 = 2^5 5^5 at the default size)
        n_named, step = args.targets + args.exclude, 7919
        if np.gcd(step, args.news - 1) != 1 or n_named >= args.news - 1:
            raise SystemExit(f"--news - 1 must share no factor with {step} and exceed targets + exclude")
        start = torch.randint(0, args.news - 1, (U, 1), generator=g)
        named = ((start + torch.arange(n_named)[None, :] * step) % (args.news - 1) + 1).to(torch.int32).cuda()
        targets, exclude = named[:, :args.targets].contiguous(), named[:, args.targets:].contiguous()
        a = (news, user, targets, exclude, min(args.block, U))
        if args.seen:
            lists = ops.ExclusionLists(torch.randint(1, args.news, (U, args.seen), generator=g, dtype=torch.int32).cuda())
            csr = lambda: ops.score_rank(news, user, targets, exclude=lists, ks=KS)
            row = {"U": U, "V": args.news, "N": args.dim, "T": args.targets, "E": args.exclude, "seen": args.seen, "listed_ids": int(lists.ids.numel())}
            got = pool_row(lambda: fused(*a), csr, args.calls, args.warmup)
            row.update({"mode": "seen", "dense": got["plain"], "csr": got["pooled"]})
            row["csr_over_dense"] = round(row["csr"]["median_ms"] / row["dense"]["median_ms"], 4)
            row["named_share_dense"], row["named_share_csr"] = named_share(lambda: fused(*a)), named_share(csr)
            row["named_share_formula"] = round(0.02 * (1 + max(0, -(-(args.seen - 64) // 128))), 4)
            lines.append(row)
            print(json.dumps(row), flush=True)
            continue
        if args.group:
            group = torch.randint(0, args.group, (args.news,), generator=g, dtype=torch.int32)
            group[3::10] = -1                                                     # every tenth news is in no group
            group = group.cuda()
            capped = lambda: ops.score_rank_capped(news, user, targets, group, args.group_cap, n_groups=args.group, exclude=exclude, ks=KS)
            row = {"U": U, "V": args.news, "N": args.dim, "T": args.targets, "E": args.exclude, "groups": args.group, "group_cap": args.group_cap}
            got = pool_row(lambda: fused(*a), capped, args.calls, args.warmup)
            row.update({"mode": "group", "plain": got["plain"], "capped": got["pooled"]})
            row["capped_over_plain"] = round(row["capped"]["median_ms"] / row["plain"]["median_ms"], 4)
            r_c, r_p = capped()[0], fused(*a)[0]
            row["capped_out_fraction"] = round(float((r_c == -1).float().mean()), 6)
            row["moved_up_fraction"] = round(float(((r_c > 0) & (r_c < r_p)).float().mean()), 6)
            row["consistent"] = bool((((r_c == 0) == (r_p == 0)) & ((r_c <= 0) | (r_c <= r_p))).all())
            row["launch_shares"] = launch_shares(capped, ("rank_group_masks", "rank_named", "rank_count", "rank_final"))
            lines.append(row)
            print(json.dumps(row), flush=True)
            continue
        if args.pool:
            prior, stamp, window = pool_inputs(args.news, U, g)
            pooled = lambda: ops.score_rank(news, user, targets, exclude=exclude, ks=KS, prior=prior, stamp=stamp, window=window)
            row = {"U": U, "V": args.news, "N": args.dim, "T": args.targets, "E": args.exclude}
            row.update(pool_row(lambda: fused(*a), pooled, args.calls, args.warmup))
            row["ranked_fraction"] = round(float((pooled()[0] > 0).float().mean()), 6)
            lines.append(row)
            print(json.dumps(row), flush=True)
            continue
        for _ in range(args.warmup):
            fused(*a)
            baseline(*a)
        torch.cuda.synchronize()
        t_f, t_b = [], []
        for _ in range(args.calls):
            t_f.append(timed(fused, *a))
            t_b.append(timed(baseline, *a))
        r_f = fused(*a)[0].long()
        r_b = baseline(*a)
        row = {"U": U, "V": args.news, "N": args.dim, "T": args.targets, "E": args.exclude, "block": a[4], "fused": stats(t_f),
               "baseline": stats(t_b), "fused_peak_bytes": peak_bytes(fused, *a), "baseline_peak_bytes": peak_bytes(baseline, *a),
               "score_block_bytes": a[4] * args.news * 4,
               "ranks_equal_fraction": round(float((r_f == r_b).float().mean()), 6),
               "max_rank_diff": int((r_f - r_b).abs().max())}
        flops = 2.0 * U * args.news * args.dim
        row["fused_tflops"] = round(flops / (row["fused"]["median_ms"] * 1e-3) / 1e12, 2)
        row["fused_fraction_of_fp32_mfma_peak"] = round(row["fused_tflops"] * 1e12 / PEAK_FP32_MATRIX, 4)
        row["baseline_tflops"] = round(flops / (row["baseline"]["median_ms"] * 1e-3) / 1e12, 2)
        lines.append(row)
        print(json.dumps(row), flush=True)
        del user
    if args.pool or args.seen or args.group:
        write(args.out, lines)
        return
    last = lines[-1]
    spread = max(last["fused"]["iqr_ms"], last["baseline"]["iqr_ms"])
    verdict = {"U": last["U"], "spread_ms": spread,
               "time_ok": last["fused"]["median_ms"] <= last["baseline"]["median_ms"] + spread,
               "memory_ok": last["baseline_peak_bytes"] - last["fused_peak_bytes"] >= last["score_block_bytes"]}
    lines.append(verdict)
    print(json.dumps(verdict), flush=True)
    write(args.out, lines)


if __name__ == "__main__":
    main()
