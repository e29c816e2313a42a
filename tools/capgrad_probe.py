#!/usr/bin/env python
"""The gradient of rows served under group caps (ops.score_expect_groups, K20; ops.row_logprob_capped_grad, K21;
ops.score_expect_news_groups, K22; include/nrhip.h)
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
  the news side: score_expect_news (K18) beside score_expect_news_groups (K22) with the same users, table, lists and named terms --
  `tile_floor` = (non-padding tiles of the order) / (tiles of V) is the floor of that ratio; forward + backward with BOTH gradients
  of plackett_luce_nll_capped_joint beside plackett_luce_nll_capped (user gradient alone) and beside plackett_luce_nll with both
  gradients; the three transposes K22's Python layer makes per call, GroupOrder.by_position and ExclusionLists.by_news, each alone.
One JSON line per (U, groups).  Needs a GPU: there is nothing to fall back to."""
import argparse
import json
import math
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logz_probe import interleaved, launch_shares  # noqa: E402
from newsrecommendation_amd import _lib, ops  # noqa: E402

TAU = 0.5


def skewed_groups(V, n_groups, gen):
    """int32 [V]: group sizes ~ 1 / (rank + 1), a tenth of the news in no group"""
    w = 1.0 / torch.arange(1, n_groups + 1, dtype=torch.float64)
    g = torch.multinomial(w / w.sum(), V, replacement=True, generator=gen).to(torch.int32)
    g[torch.rand(V, generator=gen) < 0.1] = -1
    return g


def stream_tile(call):
    """The news tile of a K22 call, read from the label the library gives its stream launch (`TV=`): the LDS plan is the library's."""
    call()
    torch.cuda.synchronize()
    _lib.prof_enable(1)
    try:
        _lib.prof_collect()
        call()
        torch.cuda.synchronize()
        labels = list(_lib.prof_collect())
    finally:
        _lib.prof_enable(0)
    (label,) = [x for x in labels if x.startswith("expect_news_groups_stream[")]
    return int(re.search(r"TV=(\d+)", label).group(1))


def tile_floor(order, V, TV):
    """(non-padding tiles of the order) / (tiles of V): what K22 streams the users past, beside K18"""
    alive = (order.order.reshape(-1, TV) != 0).any(dim=1).sum().item()
    return alive, math.ceil(V / TV)


def news_side(news, user, rows, lists, base, bases, om, c, a19, gup, order, group, n_groups, cap, args):
    """K22 beside K18 with the same users and table; the capped joint loss (both gradients) beside the frozen-table one and beside
    plackett_luce_nll with both gradients; the three transposes and GroupOrder.by_position each on its own."""
    V, N = news.shape
    named = ops._named_by_news(rows, c, V)
    calls = {"expect_news": lambda: ops._score_expect_news("probe", news, user, TAU, base, lists, 0, None, None, None, a19, named, True, True),
             "expect_news_groups": lambda: ops._score_expect_news_groups("probe", news, user, TAU, order, bases, om, lists, 0, None, None, None,
                                                                         named, True),
             "three_transposes": lambda: (bases[0].t().contiguous(), bases[1].t().contiguous(), om.t().contiguous()),
             "by_position": lambda: order.by_position(ops.ExclusionLists.from_sorted(lists.offsets, lists.ids)),     # a fresh object: nothing kept
             "by_news": lambda: ops.ExclusionLists.from_sorted(lists.offsets, lists.ids).by_news(V)}
    TV = stream_tile(calls["expect_news_groups"])
    alive, tiles_v = tile_floor(order, V, TV)
    out = {"news_tile": TV, "tiles_alive": alive, "tiles_of_V": tiles_v, "tile_floor": round(alive / tiles_v, 4)}
    out.update(interleaved(calls, args.calls, args.warmup))
    out["expect_news_groups_over_expect_news"] = round(out["expect_news_groups"]["median_ms"] / out["expect_news"]["median_ms"], 4)
    out["expect_news_groups_launch_shares"] = launch_shares(calls["expect_news_groups"])
    uv, nv = user.clone().requires_grad_(True), news.clone().requires_grad_(True)

    def joint():
        uv.grad = nv.grad = None
        o, _ = ops.plackett_luce_nll_capped_joint(nv, uv, rows, TAU, order, group, cap)
        (o * gup).sum().backward()

    def frozen():
        uv.grad = None
        o, _ = ops.plackett_luce_nll_capped(news, uv, rows, TAU, order, group, cap)
        (o * gup).sum().backward()

    def free_both():
        uv.grad = nv.grad = None
        o, _ = ops.plackett_luce_nll(nv, uv, rows, TAU)
        (o * gup).sum().backward()

    out.update(interleaved({"pl_capped_joint": joint, "pl_capped_frozen": frozen, "pl_both": free_both}, args.calls, args.warmup))
    out["pl_capped_joint_over_frozen"] = round(out["pl_capped_joint"]["median_ms"] / out["pl_capped_frozen"]["median_ms"], 4)
    out["pl_capped_joint_over_pl_both"] = round(out["pl_capped_joint"]["median_ms"] / out["pl_both"]["median_ms"], 4)
    return out


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
            row.update(news_side(news, user, rows, lists, base, bases, om, c, a19, gup, order, group, n_groups, cap, args))
            lines.append(row)
            print(json.dumps(row), flush=True)
            del uv, user
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
