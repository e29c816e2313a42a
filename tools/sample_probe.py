#!/usr/bin/env python
"""Sampled full-corpus recommendation: the fused call (ops.score_sample) against the plain fused call (ops.score_topk) on the
same device, at the same shapes.

    python tools/sample_probe.py [--news 100001] [--dim 400] [--k 10 128] [--users 64 8192] [--scale 0.1 1.0] [--calls 30] [--warmup 5]
                                 [--label TEXT] [--out FILE]

Both calls take the same fp32 inputs.  The temperature is per user: `scale` times that user's own score standard deviation over
the corpus (estimated on 4096 news).  Per (U, k): every call is timed with a pair of device events, the plain call and the
sampled calls (one per scale) alternate call by call (so that a disturbance of the machine hits all of them), and the median,
minimum, maximum and inter-quartile spread of the timed calls are reported with the ratio of each sampled median to the plain
one.  Each row also carries a CRC of the sampled ids and perturbed scores: two builds of the library (NRHIP_LIB=/path/to/other
libnrhip.so, e.g. one compiled without the skip bound of sample_key) must print the same CRCs, and the ratio of their medians
is what the bound saves.  One JSON line per (U, k).  Needs a GPU: there is nothing to fall back to."""
import argparse
import json
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from newsrecommendation_amd import ops  # noqa: E402

SEED, DRAW = 20240607, 1


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


def crc(*tensors):
    c = 0
    for t in tensors:
        c = zlib.crc32(t.contiguous().cpu().numpy().tobytes(), c)
    return f"{c:08x}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--news", type=int, default=100001)
    ap.add_argument("--dim", type=int, default=400)
    ap.add_argument("--k", type=int, nargs="+", default=[10, 128])
    ap.add_argument("--users", type=int, nargs="+", default=[64, 8192])
    ap.add_argument("--scale", type=float, nargs="+", default=[0.1, 1.0], help="temperature / the user's own score standard deviation")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--label", default="", help="copied into every row (which build this is)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_probe needs a GPU")
    if args.calls < 20:
        raise SystemExit("at least 20 timed calls")
    g = torch.Generator().manual_seed(0)
    news = (torch.randn(args.news, args.dim, generator=g) * 0.4).cuda()
    lines = []
    for U in args.users:
        user = (torch.randn(U, args.dim, generator=g) * 0.4).cuda()
        spread = torch.matmul(user, news[1:4097].T).std(dim=1)
        keys = torch.arange(U, dtype=torch.int32, device="cuda")
        for k in args.k:
            calls = {"plain": lambda: ops.score_topk(news, user, k)}
            for s in args.scale:
                calls[f"sampled_{s:g}"] = (lambda tau: lambda: ops.score_sample(news, user, k, tau, SEED, draw=DRAW, user_keys=keys))(spread * s)
            for _ in range(args.warmup):
                for fn in calls.values():
                    fn()
            torch.cuda.synchronize()
            t = {name: [] for name in calls}
            for _ in range(args.calls):
                for name, fn in calls.items():
                    t[name].append(timed(fn))
            row = {"label": args.label, "U": U, "V": args.news, "N": args.dim, "k": k, "score_std_mean": round(float(spread.mean()), 4),
                   "lib": os.environ.get("NRHIP_LIB", "in-tree")}
            plain_ids, _ = calls["plain"]()
            for name in calls:
                row[name] = stats(t[name])
                if name != "plain":
                    ids, pert, model = calls[name]()
                    row[name]["over_plain"] = round(row[name]["median_ms"] / row["plain"]["median_ms"], 4)
                    row[name]["crc"] = crc(ids, pert, model)
                    row[name]["rows_changed_fraction"] = round(float((ids != plain_ids).any(dim=1).float().mean()), 4)
                    row[name]["first_place_kept_fraction"] = round(float((ids[:, 0] == plain_ids[:, 0]).float().mean()), 4)
            lines.append(row)
            print(json.dumps(row), flush=True)
        del user
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
