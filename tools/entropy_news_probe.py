#!/usr/bin/env python
"""The news-table pass of the entropy-regularised full softmax (ops.score_expect_news_affine; include/nrhip.h, K25) beside the pass
it clones (ops.score_expect_news; K18), and the regularised joint loss (ops.full_softmax_nll_entropy_joint) forward + backward
with all three gradients beside ops.full_softmax_nll_entropy's (frozen table) and ops.full_softmax_nll_joint's (no entropy).

    python tools/entropy_news_probe.py [--news 100001] [--dim 400] [--users 64 8192] [--seen 300] [--calls 30] [--warmup 5] [--out FILE]

Per U the calls are timed INTERLEAVED in one process -- K18 plain twice per round (`news_plain`, `news_again`: the difference of
their medians is the run-to-run spread K25 / K18 is judged against), then K18 and K25 plain, with pools and with CSR lists of
--seen random ids per user (transposed once: ExclusionLists.by_news keeps its result) -- each call between a pair of device
events; median, minimum, maximum and inter-quartile spread are reported, with K25 / K18 per kind of argument.  Then the three
losses, forward + backward with T = 4 targets per user, upstream gradients for nll and for the entropy, and a learnable 0-dim
temperature where the function has one.  One JSON line per U.  Needs a GPU: there is nothing to fall back to."""
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
    ap.add_argument("--targets", type=int, default=4, help="targets per user of the loss calls")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("entropy_news_probe needs a GPU")
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
        lists.by_news(V)                                              # the transpose is built once and kept
        alpha, beta = torch.randn(U, generator=g).cuda(), torch.randn(U, generator=g).cuda()
        kws = {"plain": {}, "pool": dict(prior=prior, stamp=stamp, window=window), "lists": dict(exclude=lists)}
        bases = {k: ops.score_logz(news, user, TAU, **kw) for k, kw in kws.items()}
        k18 = lambda: ops.score_expect_news(news, user, TAU, bases["plain"], weight=alpha)
        calls = {"news_plain": k18}
        for k, kw in kws.items():
            if k != "plain":
                calls["news_" + k] = (lambda k=k, kw=kw: ops.score_expect_news(news, user, TAU, bases[k], weight=alpha, **kw))
            calls["news_affine_" + k] = (lambda k=k, kw=kw: ops.score_expect_news_affine(news, user, TAU, bases[k], alpha=alpha, beta=beta, **kw))
        calls["news_again"] = k18
        row = {"U": U, "V": V, "N": args.dim, "seen": args.seen, "listed_ids": int(lists.ids.numel()), "tau": TAU}
        row.update(interleaved(calls, args.calls, args.warmup))
        row["news_spread_ms"] = round(abs(row["news_again"]["median_ms"] - row["news_plain"]["median_ms"]), 4)
        for k in kws:
            row[f"news_affine_{k}_over_news_{k}"] = round(row["news_affine_" + k]["median_ms"] / row["news_" + k]["median_ms"], 4)
        row["news_affine_launch_shares"] = launch_shares(calls["news_affine_plain"])
        out, mass = calls["news_affine_plain"]()
        row["plain_mass_sum_over_users"] = float(mass.double().sum()) / U
        row["plain_rows_finite"] = bool(torch.isfinite(out).all())
        targets = torch.randint(1, V, (U, args.targets), generator=g, dtype=torch.int32).cuda()
        uv, nv = user.clone().requires_grad_(True), news.clone().requires_grad_(True)
        temp = torch.nn.Parameter(torch.tensor(TAU).cuda())

        def nll_entropy_fwd_bwd():                                    # the frozen table: grad_user and grad_tau
            uv.grad, temp.grad = None, None
            nll, _, h = ops.full_softmax_nll_entropy(news, uv, targets, temp)
            (nll.sum() - 0.1 * h.sum()).backward()

        def nll_joint_fwd_bwd():                                      # no entropy: grad_user and grad_news (K17 + K18)
            uv.grad, nv.grad = None, None
            nll, _ = ops.full_softmax_nll_joint(nv, uv, targets, TAU)
            nll.sum().backward()

        def nll_entropy_joint_fwd_bwd():                              # all three gradients (K24 + K25)
            uv.grad, nv.grad, temp.grad = None, None, None
            nll, _, h = ops.full_softmax_nll_entropy_joint(nv, uv, targets, temp)
            (nll.sum() - 0.1 * h.sum()).backward()

        train = interleaved({"nll_entropy_fwd_bwd": nll_entropy_fwd_bwd, "nll_joint_fwd_bwd": nll_joint_fwd_bwd,
                             "nll_entropy_joint_fwd_bwd": nll_entropy_joint_fwd_bwd}, args.calls, args.warmup)
        row.update(train)
        row["nll_entropy_joint_over_nll_entropy"] = round(train["nll_entropy_joint_fwd_bwd"]["median_ms"] / train["nll_entropy_fwd_bwd"]["median_ms"], 4)
        row["nll_entropy_joint_over_nll_joint"] = round(train["nll_entropy_joint_fwd_bwd"]["median_ms"] / train["nll_joint_fwd_bwd"]["median_ms"], 4)
        lines.append(row)
        print(json.dumps(row), flush=True)
        del user, uv, nv
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
