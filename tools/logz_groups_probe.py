#!/usr/bin/env python
"""Per-group log-partition (ops.score_logz_groups) beside the plain one (ops.score_logz), and the capped propensity beside
the plain one: what the group-major order costs.

    python tools/logz_groups_probe.py [--news 100001] [--dim 400] [--users 64 8192] [--groups 18 285] [--seen 300] [--calls 30]
                                      [--warmup 5] [--out FILE]

The group column is synthetic and skewed: a tenth of the news in no group, the rest in G groups of sizes proportional to
1 / (1 + rank), assigned by a seeded permutation.  Per (U, G), timed INTERLEAVED in one process, each call between a pair of
device events: score_logz (twice per round, as `plain` and `plain_again`: the difference of their medians is the spread the
others are judged against), score_logz_groups, and both with CSR lists of --seen random ids per user (the grouped call maps
them to positions on every call, as the product path does; `map_lists_ms` is that mapping alone).
`chunk_ratio` is host arithmetic: padded chunks of the group-major order / chunks of the plain stream, the factor on the MFMA
work.  Then the propensity of k = 10 and k = 128 rows as train.sample_propensity and train.sample_propensity_capped compute it
past the user vectors, which they share: merge the row into the lists, the partition, the row pass -- on rows drawn by
ops.score_sample without and with the cap.  One JSON line per (U, G).  Needs a GPU: there is nothing to fall back to."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from newsrecommendation_amd import _lib, ops  # noqa: E402

TAU, CAP = 0.5, 2


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
    return {"median_ms": round(float(med), 4), "min_ms": round(float(a.min()), 4), "iqr_ms": round(float(q3 - q1), 4), "calls": len(ms)}


def interleaved(calls, n, warmup):
    """{name: stats} of the calls {name: fn}, one of each per round."""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(n):
        for name, fn in calls.items():
            ms[name].append(timed(fn))
    return {name: stats(v) for name, v in ms.items()}


def launch_shares(call, reps=5):
    """{label prefix: share} of the launches of `call`, by the library's per-launch timer."""
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
    out = {}
    for label, (_, ms) in got.items():
        key = label.split("[")[0]
        out[key] = round(out.get(key, 0.0) + ms / total, 4) if total > 0 else None
    return out


def skewed_groups(V, G, g):
    """int32 [V]: a tenth of the news in no group, the rest in G groups of sizes ~ 1 / (1 + rank)."""
    w = 1.0 / (1.0 + torch.arange(G, dtype=torch.float64))
    edges = torch.cumsum(w / w.sum() * 0.9, 0)
    draw = torch.rand(V, generator=g, dtype=torch.float64)
    group = torch.searchsorted(edges, draw).to(torch.int32)
    group[group >= G] = -1
    group[0] = -1
    return group


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--news", type=int, default=100001)
    ap.add_argument("--dim", type=int, default=400)
    ap.add_argument("--users", type=int, nargs="+", default=[64, 8192])
    ap.add_argument("--groups", type=int, nargs="+", default=[18, 285])
    ap.add_argument("--seen", type=int, default=300, help="random ids per user in the CSR lists of the listed calls")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("logz_groups_probe needs a GPU")
    if args.calls < 20:
        raise SystemExit("at least 20 timed calls")
    g = torch.Generator().manual_seed(0)
    V = args.news
    news = (torch.randn(V, args.dim, generator=g) * 0.4).cuda()
    lines = []
    for U in args.users:
        user = (torch.randn(U, args.dim, generator=g) * 0.4).cuda()
        lists = ops.ExclusionLists(torch.randint(1, V, (U, args.seen), generator=g, dtype=torch.int32).cuda())
        for G in args.groups:
            group = skewed_groups(V, G, g).cuda()
            order = ops.GroupOrder(group, n_groups=G)
            plain = lambda: ops.score_logz(news, user, TAU)
            calls = {"plain": plain,
                     "groups": lambda: ops.score_logz_groups(news, user, TAU, order),
                     "plain_lists": lambda: ops.score_logz(news, user, TAU, exclude=lists),
                     "groups_lists": lambda: ops.score_logz_groups(news, user, TAU, order, exclude=lists),
                     "plain_again": plain}
            row = {"U": U, "V": V, "N": args.dim, "G": G, "seen": args.seen, "tau": TAU, "n_pos": order.n_pos, "nseg": order.nseg,
                   "chunks_per_segment": order.chunks_per_segment,
                   "chunk_ratio": round((order.n_pos // 128) / ((V - 1 + 127) // 128), 4),
                   "largest_bin": int(torch.bincount(torch.where(group < 0, G, group.to(torch.int64))[1:]).max())}
            row.update(interleaved(calls, args.calls, args.warmup))
            p = row["plain"]["median_ms"]
            row["plain_spread_ms"] = round(abs(row["plain_again"]["median_ms"] - p), 4)
            row["groups_over_plain"] = round(row["groups"]["median_ms"] / p, 4)
            row["groups_lists_over_plain_lists"] = round(row["groups_lists"]["median_ms"] / row["plain_lists"]["median_ms"], 4)
            row["groups_launch_shares"] = launch_shares(calls["groups"])
            row["groups_lists_launch_shares"] = launch_shares(calls["groups_lists"])
            row["map_lists_ms"] = interleaved({"map": lambda: order.positions(lists)}, 20, 3)["map"]["median_ms"]
            gl, gm, gc = calls["groups"]()
            row["count_ok"] = bool((gc.sum(dim=1) == V - 1).all())
            row["logsum_finite"] = bool(torch.isfinite(gl[gc > 0]).all())
            for k in (10, 128):
                free = ops.score_sample(news, user, k, TAU, 7, exclude=lists)[0]
                capped = ops.score_sample(news, user, k, TAU, 7, exclude=lists, group=group, group_cap=CAP)[0]

                def propensity(ids=free):
                    base = ops.score_logz(news, user, TAU, exclude=lists.merged(ops.ExclusionLists(ids)))
                    return ops.row_logprob(news, user, ids, TAU, base, True)

                def propensity_capped(ids=capped):
                    bases = ops.score_logz_groups(news, user, TAU, order, exclude=lists.merged(ops.ExclusionLists(ids)))
                    return ops.row_logprob_capped(news, user, ids, TAU, bases, group, CAP, n_groups=G)

                got = interleaved({f"propensity_k{k}": propensity, f"propensity_capped_k{k}": propensity_capped,
                                   f"row_logprob_k{k}": lambda ids=free, base=ops.score_logz(news, user, TAU, exclude=lists.merged(free)):
                                   ops.row_logprob(news, user, ids, TAU, base, True),
                                   f"row_logprob_capped_k{k}": lambda ids=capped, b=ops.score_logz_groups(news, user, TAU, order, exclude=lists.merged(capped)):
                                   ops.row_logprob_capped(news, user, ids, TAU, b, group, CAP, n_groups=G)}, args.calls, args.warmup)
                row.update(got)
                row[f"capped_over_plain_k{k}"] = round(got[f"propensity_capped_k{k}"]["median_ms"] / got[f"propensity_k{k}"]["median_ms"], 4)
                row[f"capped_rows_filled_k{k}"] = round(float((capped > 0).float().mean()), 4)
            lines.append(row)
            print(json.dumps(row), flush=True)
        del user
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
