#!/usr/bin/env python
"""The gradient of rows served under group caps (ops.score_expect_groups, K20; ops.row_logprob_capped_grad, K21; include/nrhip.h)
beside the calls it is built like, and the capped listwise loss (ops.plackett_luce_nll_capped) beside the uncapped one.

    python tools/capgrad_probe.py [--news 100001] [--dim 400] [--users 64 8192] [--groups 18 285] [--places 10] [--cap 2]
                                  [--calls 30] [--warmup 5] [--out FILE]

Groups are skewed (sizes ~ 1 / rank, a tenth of the news in no group).  Per U and group count the calls are timed INTERLEAVED in
one process, each between a pair of device events (median, minimum, maximum and inter-quartile spread):
  score_expect (K17) with the row merged into the lists, beside score_expect_groups (K20) with the same arguments on the bases of
  score_logz_groups -- `chunk_ratio` = (n_pos / 128) / ceil((V - 1) / 128) is the floor K20 cannot go below: every bin's run is
  padded to whole chunks;
  row_logprob_capped (K16) beside row_logprob_capped_grad (K21);
  forward + backward (user gradient) of plackett_luce_nll_capped beside plackett_luce_nll and beside the two forward launches alone
  (train.sample_propensity_capped's: score_logz_groups + row_logprob_capped).
One JSON line per (U, groups).  Needs a GPU: there is nothing to fall back to."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logz_probe import interleaved, launch_shares  # noqa: E402
from newsrecommendation_amd import ops  # noqa: E402

TAU = 0.5


def skewed_groups(V, n_groups, gen):
    """int32 [V]: group sizes ~ 1 / (rank + 1), a tenth of the news in no group"""
    w = 1.0 / torch.arange(1, n_groups + 1, dtype=torch.float64)
    g = torch.multinomial(w / w.sum(), V, replacement=True, generator=gen).to(torch.int32)
    g[torch.rand(V, generator=gen) < 0.1] = -1
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--news", type=int, default=100001)
    ap.add_argument("--dim", type=int, default=400)
    ap.add_argument("--users", type=int, nargs="+", default=[64, 8192])
    ap.add_argument("--groups", type=int, nargs="+", default=[18, 285])
    ap.add_argument("--places", type=int, default=10)
    ap.add_argument("--cap", type=int, default=2)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("capgrad_probe needs a GPU")
    if args.calls < 20:
        raise SystemExit("at least 20 timed calls")
    gen = torch.Generator().manual_seed(0)
    V, k, cap = args.news, args.places, args.cap
    news = (torch.randn(V, args.dim, generator=gen) * 0.4).cuda()
    lines = []
    for n_groups in args.groups:
        group = skewed_groups(V, n_groups, gen).cuda()
        order = ops.GroupOrder(group, n_groups=n_groups)
        for U in args.users:
            user = (torch.randn(U, args.dim, generator=gen) * 0.4).cuda()
            rows = ops.score_sample(news, user, k, TAU, 7, group=group, group_cap=cap)[0]     # served rows under the caps
            lists = ops.ExclusionLists(rows)
            base = ops.score_logz(news, user, TAU, exclude=lists)
            bases = ops.score_logz_groups(news, user, TAU, order, exclude=lists)
            gup = torch.randn(U, k, generator=gen).cuda()
            om, c = ops.row_logprob_capped_grad(news, user, rows, TAU, bases, group, cap, n_groups=n_groups, g=gup)
            a19, _ = ops.row_logprob_grad(news, user, rows, TAU, base, g=gup)
            calls = {"expect": lambda: ops.score_expect(news, user, TAU, base, exclude=lists, weight=a19),
                     "expect_groups": lambda: ops.score_expect_groups(news, user, TAU, order, bases, om, exclude=lists),
                     "logp_capped": lambda: ops.row_logprob_capped(news, user, rows, TAU, bases, group, cap, n_groups=n_groups),
                     "logp_capped_grad": lambda: ops.row_logprob_capped_grad(news, user, rows, TAU, bases, group, cap, n_groups=n_groups, g=gup)}
            row = {"U": U, "V": V, "N": args.dim, "k": k, "cap": cap, "groups": n_groups, "tau": TAU, "nseg": order.nseg, "n_pos": order.n_pos,
                   "chunk_ratio": round((order.n_pos // 128) / math.ceil((V - 1) / 128), 4)}
            row.update(interleaved(calls, args.calls, args.warmup))
            row["expect_groups_over_expect"] = round(row["expect_groups"]["median_ms"] / row["expect"]["median_ms"], 4)
            row["grad_over_logp_capped"] = round(row["logp_capped_grad"]["median_ms"] / row["logp_capped"]["median_ms"], 4)
            row["expect_groups_launch_shares"] = launch_shares(calls["expect_groups"])
            row["omega_minus_sum_c_max"] = float((om.double().sum(dim=1) - c.double().sum(dim=1)).abs().max())
            uv = user.clone().requires_grad_(True)

            def capped():
                uv.grad = None
                out, _ = ops.plackett_luce_nll_capped(news, uv, rows, TAU, order, group, cap)
                (out * gup).sum().backward()

            def free():
                uv.grad = None
                out, _ = ops.plackett_luce_nll(news, uv, rows, TAU)
                (out * gup).sum().backward()

            def propensity():
                b = ops.score_logz_groups(news, user, TAU, order, exclude=lists)
                ops.row_logprob_capped(news, user, rows, TAU, b, group, cap, n_groups=n_groups)

            row.update(interleaved({"pl_capped": capped, "pl": free, "propensity_capped": propensity}, args.calls, args.warmup))
            row["pl_capped_over_pl"] = round(row["pl_capped"]["median_ms"] / row["pl"]["median_ms"], 4)
            row["pl_capped_over_propensity"] = round(row["pl_capped"]["median_ms"] / row["propensity_capped"]["median_ms"], 4)
            lines.append(row)
            print(json.dumps(row), flush=True)
            del uv, user
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
