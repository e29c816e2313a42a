#!/usr/bin/env python
"""The gradient coefficients of sequential rows (ops.row_logprob_grad; include/nrhip.h, K19) beside the forward they differentiate
(ops.row_logprob, sequential), and the listwise loss built on them (ops.plackett_luce_nll) beside the full-softmax losses.

    python tools/listwise_probe.py [--news 100001] [--dim 400] [--users 64 8192] [--places 10 128] [--calls 30] [--warmup 5] [--out FILE]

Per U and k the calls are timed INTERLEAVED in one process, each between a pair of device events (median, minimum, maximum and
inter-quartile spread):
  row_logprob (twice per round, as `logp` and `logp_again`: the difference of their medians is the run-to-run spread),
  row_logprob_grad with g = None and with a signed g, on the same base (the row merged into the lists of score_logz);
  forward + backward of plackett_luce_nll with a gradient for the users only and for users and table, beside full_softmax_nll
  and full_softmax_nll_joint with the same k ids as independent targets.
The expectation from the code: K19 is about one K14 launch (the same gather; about twice the fp64 scan), the backward K17 (+ K18).
One JSON line per (U, k).  Needs a GPU: there is nothing to fall back to."""
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
    ap.add_argument("--places", type=int, nargs="+", default=[10, 128])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("listwise_probe needs a GPU")
    if args.calls < 20:
        raise SystemExit("at least 20 timed calls")
    g = torch.Generator().manual_seed(0)
    V = args.news
    news = (torch.randn(V, args.dim, generator=g) * 0.4).cuda()
    lines = []
    for U in args.users:
        user = (torch.randn(U, args.dim, generator=g) * 0.4).cuda()
        for k in args.places:
            rows = ops.score_sample(news, user, k, TAU, 7)[0]       # served rows: k news without replacement
            base = ops.score_logz(news, user, TAU, exclude=ops.ExclusionLists(rows))
            gup = torch.randn(U, k, generator=g).cuda()
            logp = lambda: ops.row_logprob(news, user, rows, TAU, base, True)
            calls = {"logp": logp,
                     "grad_ones": lambda: ops.row_logprob_grad(news, user, rows, TAU, base),
                     "grad_signed": lambda: ops.row_logprob_grad(news, user, rows, TAU, base, g=gup),
                     "logp_again": logp}
            row = {"U": U, "V": V, "N": args.dim, "k": k, "tau": TAU}
            row.update(interleaved(calls, args.calls, args.warmup))
            row["logp_spread_ms"] = round(abs(row["logp_again"]["median_ms"] - row["logp"]["median_ms"]), 4)
            row["grad_over_logp"] = round(row["grad_signed"]["median_ms"] / row["logp"]["median_ms"], 4)
            row["grad_launch_shares"] = launch_shares(calls["grad_signed"])
            a, c = calls["grad_signed"]()
            row["a_minus_sum_c_max"] = float((a.double() - c.double().sum(dim=1)).abs().max())
            uv, nv = user.clone().requires_grad_(True), news.clone().requires_grad_(True)

            def run(fn, table, users):
                def call():
                    uv.grad = nv.grad = None
                    out, _ = fn(table, users, rows, TAU)
                    (out * gup).sum().backward()
                return call

            losses = {"pl_user": run(ops.plackett_luce_nll, news, uv), "softmax_user": run(ops.full_softmax_nll, news, uv),
                      "pl_both": run(ops.plackett_luce_nll, nv, uv), "softmax_both": run(ops.full_softmax_nll_joint, nv, uv)}
            row.update(interleaved(losses, args.calls, args.warmup))
            row["pl_over_softmax_user"] = round(row["pl_user"]["median_ms"] / row["softmax_user"]["median_ms"], 4)
            row["pl_over_softmax_both"] = round(row["pl_both"]["median_ms"] / row["softmax_both"]["median_ms"], 4)
            lines.append(row)
            print(json.dumps(row), flush=True)
            del uv, nv
        del user
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
