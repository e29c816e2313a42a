#!/usr/bin/env python
"""The news-table gradient pass (ops.score_expect_news; include/nrhip.h, K18) beside the user-side pass it mirrors
(ops.score_expect, K17) and the log-partition both stand on (ops.score_logz, K13): the same two contractions with the roles of
the operands swapped.

    python tools/expect_news_probe.py [--news 100001] [--dim 400] [--users 64 8192] [--seen 300] [--calls 30] [--warmup 5] [--out FILE]

Per U the calls are timed INTERLEAVED in one process -- logz plain (twice per round, as `logz_plain` and `logz_again`: the
difference of their two medians is the run-to-run spread the others are judged against), logz with pools and with CSR lists of
--seen random ids per user, and on the base of each of the three: K17 (`expect_*`), K18 with rows (`news_*`) and K18 mass-only
(`mass_*`) -- each call between a pair of device events; the median, minimum, maximum and inter-quartile spread are reported,
with K18 / K17 and mass-only / score_logz per argument set.  The lists are transposed once (ExclusionLists.by_news keeps its
result), in the warm-up.  Then ops.full_softmax_nll_joint forward + backward with both inputs requiring grad beside
ops.full_softmax_nll's (T = 4 targets per user), timed the same way.
One JSON line per U.  Needs a GPU: there is nothing to fall back to."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logz_probe import interleaved, launch_shares  # noqa: E402
from newsrecommendation_amd import ops  # noqa: E402

TAU = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--news", type=int, default=100001)
    ap.add_argument("--dim", type=int, default=400)
    ap.add_argument("--users", type=int, nargs="+", default=[64, 8192])
    ap.add_argument("--seen", type=int, default=300, help="random ids per user in the CSR lists of the listed calls")
    ap.add_argument("--targets", type=int, default=4, help="targets per user of the full_softmax_nll calls")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("expect_news_probe needs a GPU")
    if args.calls < 20:
        raise SystemExit("at least 20 timed calls")
    g = torch.Generator().manual_seed(0)
    V = args.news
    news = (torch.randn(V, args.dim, generator=g) * 0.4).cuda()
    prior = torch.randn(V, generator=g) * 0.1
    prior[torch.rand(V, generator=g) < 0.1] = float("-inf")
    prior = prior.cuda()
    stamp = torch.randint(0, 1000, (V,), generator=g, dtype=torch.int32).cuda()
    lines = []
    for U in args.users:
        user = (torch.randn(U, args.dim, generator=g) * 0.4).cuda()
        lo = torch.randint(0, 500, (U,), generator=g, dtype=torch.int32)
        window = torch.stack([lo, lo + 499], 1).contiguous().cuda()
        lists = ops.ExclusionLists(torch.randint(1, V, (U, args.seen), generator=g, dtype=torch.int32).cuda())
        kws = {"plain": {}, "pool": dict(prior=prior, stamp=stamp, window=window), "lists": dict(exclude=lists)}
        bases = {k: ops.score_logz(news, user, TAU, **kw) for k, kw in kws.items()}
        logz = lambda: ops.score_logz(news, user, TAU)
        calls = {"logz_plain": logz}
        for k, kw in kws.items():
            if k != "plain":
                calls["logz_" + k] = (lambda kw=kw: ops.score_logz(news, user, TAU, **kw))
            calls["expect_" + k] = (lambda k=k, kw=kw: ops.score_expect(news, user, TAU, bases[k], **kw))
            calls["news_" + k] = (lambda k=k, kw=kw: ops.score_expect_news(news, user, TAU, bases[k], **kw))
            calls["mass_" + k] = (lambda k=k, kw=kw: ops.score_expect_news(news, user, TAU, bases[k], rows=False, **kw))
        calls["logz_again"] = logz
        row = {"U": U, "V": V, "N": args.dim, "seen": args.seen, "listed_ids": int(lists.ids.numel()), "tau": TAU}
        row.update(interleaved(calls, args.calls, args.warmup))
        row["logz_spread_ms"] = round(abs(row["logz_again"]["median_ms"] - row["logz_plain"]["median_ms"]), 4)
        for k in kws:
            row[f"news_{k}_over_expect_{k}"] = round(row["news_" + k]["median_ms"] / row["expect_" + k]["median_ms"], 4)
            row[f"mass_{k}_over_logz_{k}"] = round(row["mass_" + k]["median_ms"] / row["logz_" + k]["median_ms"], 4)
        row["news_launch_shares"] = launch_shares(calls["news_plain"])
        out, mass = calls["news_plain"]()
        row["plain_mass_sum_over_U"] = float(mass.double().sum()) / U
        row["plain_rows_finite"] = bool(torch.isfinite(out).all())
        targets = torch.randint(1, V, (U, args.targets), generator=g, dtype=torch.int32).cuda()
        uv = user.clone().requires_grad_(True)
        nv = news.clone().requires_grad_(True)

        def nll_fwd_bwd():
            uv.grad = None
            nll, _ = ops.full_softmax_nll(news, uv, targets, TAU)
            nll.sum().backward()

        def joint_fwd_bwd():
            uv.grad = nv.grad = None
            nll, _ = ops.full_softmax_nll_joint(nv, uv, targets, TAU)
            nll.sum().backward()

        train = interleaved({"nll_fwd_bwd": nll_fwd_bwd, "joint_fwd_bwd": joint_fwd_bwd}, args.calls, args.warmup)
        row.update(train)
        row["joint_over_nll"] = round(train["joint_fwd_bwd"]["median_ms"] / train["nll_fwd_bwd"]["median_ms"], 4)
        lines.append(row)
        print(json.dumps(row), flush=True)
        del user, uv, nv
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
