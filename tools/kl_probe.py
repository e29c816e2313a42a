#!/usr/bin/env python
"""The KL pass (ops.score_kl; include/nrhip.h, K26) beside the entropy pass whose stream it doubles (ops.score_entropy) and the
log-partition (ops.score_logz), the KL expectation (ops.score_expect_kl; K27) beside the affine expectation it extends
(ops.score_expect_affine), and the trust-region loss (ops.policy_kl, both modes) forward + backward beside
ops.full_softmax_nll_entropy's.

    python tools/kl_probe.py [--news 100001] [--dim 400] [--users 64 8192] [--seen 300] [--calls 30] [--warmup 5] [--out FILE]

Per U the calls are timed INTERLEAVED in one process -- logz plain twice per round (`logz_plain`, `logz_again`: the difference of
their medians is the run-to-run spread the others are judged against), then logz, entropy, kl, affine and expect_kl plain, with
pools and with CSR lists of --seen random ids per user -- each call between a pair of device events; median, minimum, maximum and
inter-quartile spread are reported, with kl / entropy (arithmetic floor 2: twice K23's scoring MFMAs) and expect_kl / affine (floor
1.5: twice the scoring MFMAs, the same second contraction) per kind of argument.  Then policy_kl in both modes, forward +
backward, beside full_softmax_nll_entropy with T = 4 targets per user.  One JSON line per U.  Needs a GPU: there is nothing to
fall back to."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logz_probe import interleaved, launch_shares  # noqa: E402
from newsrecommendation_amd import ops  # noqa: E402

TAU, RTAU = 0.5, 0.8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--news", type=int, default=100001)
    ap.add_argument("--dim", type=int, default=400)
    ap.add_argument("--users", type=int, nargs="+", default=[64, 8192])
    ap.add_argument("--seen", type=int, default=300, help="random ids per user in the CSR lists of the listed calls")
    ap.add_argument("--targets", type=int, default=4, help="targets per user of the full_softmax_nll_entropy call")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kl_probe needs a GPU")
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
        ref = (user + 0.1 * torch.randn(U, args.dim, generator=g).cuda()).contiguous()      # a logging checkpoint: nearby
        lo = torch.randint(0, 500, (U,), generator=g, dtype=torch.int32)
        window = torch.stack([lo, lo + 499], 1).contiguous().cuda()
        lists = ops.ExclusionLists(torch.randint(1, V, (U, args.seen), generator=g, dtype=torch.int32).cuda())
        alpha, beta, gamma = (torch.randn(U, generator=g).cuda() for _ in range(3))
        kws = {"plain": {}, "pool": dict(prior=prior, stamp=stamp, window=window), "lists": dict(exclude=lists)}
        bases = {k: ops.score_logz(news, user, TAU, **kw) for k, kw in kws.items()}
        rbases = {k: ops.score_logz(news, ref, RTAU, **kw) for k, kw in kws.items()}
        logz = lambda: ops.score_logz(news, user, TAU)
        calls = {"logz_plain": logz}
        for k, kw in kws.items():
            if k != "plain":
                calls["logz_" + k] = (lambda kw=kw: ops.score_logz(news, user, TAU, **kw))
            calls["entropy_" + k] = (lambda k=k, kw=kw: ops.score_entropy(news, user, TAU, bases[k], **kw))
            calls["kl_" + k] = (lambda k=k, kw=kw: ops.score_kl(news, user, ref, TAU, bases[k], RTAU, rbases[k], **kw))
            calls["affine_" + k] = (lambda k=k, kw=kw: ops.score_expect_affine(news, user, TAU, bases[k], alpha=alpha, beta=beta, **kw))
            calls["expect_kl_" + k] = (lambda k=k, kw=kw: ops.score_expect_kl(news, user, ref, TAU, bases[k], RTAU, rbases[k], alpha=alpha,
                                                                              beta=beta, gamma=gamma, **kw))
        calls["logz_again"] = logz
        row = {"U": U, "V": V, "N": args.dim, "seen": args.seen, "listed_ids": int(lists.ids.numel()), "tau": TAU, "ref_tau": RTAU}
        row.update(interleaved(calls, args.calls, args.warmup))
        row["logz_spread_ms"] = round(abs(row["logz_again"]["median_ms"] - row["logz_plain"]["median_ms"]), 4)
        for k in kws:
            row[f"kl_{k}_over_entropy_{k}"] = round(row["kl_" + k]["median_ms"] / row["entropy_" + k]["median_ms"], 4)
            row[f"kl_{k}_over_logz_{k}"] = round(row["kl_" + k]["median_ms"] / row["logz_" + k]["median_ms"], 4)
            row[f"expect_kl_{k}_over_affine_{k}"] = round(row["expect_kl_" + k]["median_ms"] / row["affine_" + k]["median_ms"], 4)
        row["kl_launch_shares"] = launch_shares(calls["kl_plain"])
        row["expect_kl_launch_shares"] = launch_shares(calls["expect_kl_plain"])
        kl, ent, cov, mass = calls["kl_plain"]()
        row["plain_mass_max_dev"] = float((mass - 1).abs().max())
        row["plain_kl_mean"] = float(kl.mean())
        row["plain_results_finite"] = bool(torch.isfinite(kl).all() and torch.isfinite(cov).all())
        targets = torch.randint(1, V, (U, args.targets), generator=g, dtype=torch.int32).cuda()
        uv = user.clone().requires_grad_(True)
        temp = torch.nn.Parameter(torch.tensor(TAU).cuda())

        def nll_entropy_fwd_bwd():
            uv.grad, temp.grad = None, None
            nll, _, h = ops.full_softmax_nll_entropy(news, uv, targets, temp)
            (nll.sum() - 0.1 * h.sum()).backward()

        def kl_reverse_fwd_bwd():
            uv.grad, temp.grad = None, None
            kl, _ = ops.policy_kl(news, uv, ref, temp, RTAU)
            kl.sum().backward()

        def kl_forward_fwd_bwd():
            uv.grad = None
            kl, _ = ops.policy_kl(news, uv, ref, TAU, RTAU, mode="forward")
            kl.sum().backward()

        train = interleaved({"nll_entropy_fwd_bwd": nll_entropy_fwd_bwd, "policy_kl_reverse_fwd_bwd": kl_reverse_fwd_bwd,
                             "policy_kl_forward_fwd_bwd": kl_forward_fwd_bwd}, args.calls, args.warmup)
        row.update(train)
        for k in ("reverse", "forward"):
            row[f"policy_kl_{k}_over_nll_entropy"] = round(train[f"policy_kl_{k}_fwd_bwd"]["median_ms"] / train["nll_entropy_fwd_bwd"]["median_ms"], 4)
        lines.append(row)
        print(json.dumps(row), flush=True)
        del user, uv, ref
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
