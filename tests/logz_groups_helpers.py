"""Shared by tests/test_logz_groups_host.py and tests/test_gpu_logz_groups.py: the group column of the base shape, the law of the
capped sampler on the configuration of sample_helpers, and the tolerances both files derive."""
import itertools
import math

import numpy as np
import torch

from sample_helpers import LAW_TAU, LAW_X

EPS = 2.0 ** -24                           # half an ulp of fp32, relative
V_BASE = 1000
# bin sizes of the base shape (999 news): groups 0 .. 5 and "no group".  One chunk exactly, one chunk and one row, an empty bin,
# one news, several chunks with a tail, the rest; padded runs of 128, 256, 0, 128, 384, 384, 128 positions = 11 chunks
BASE_SIZES = {0: 128, 1: 129, 2: 0, 3: 1, 4: 300, -1: 100}
BASE_GROUPS = 6


def base_group(V=V_BASE, sizes=BASE_SIZES, last=5, seed=29):
    """int32 [V] group ids drawn by a seeded permutation of the news (the order is then a real gather): `sizes` news per group,
    the rest in group `last`; news 0 is in no group."""
    perm = (torch.randperm(V - 1, generator=torch.Generator().manual_seed(seed)) + 1).numpy()
    group = np.full(V, last, dtype=np.int32)
    group[0] = -1
    at = 0
    for g, n in sizes.items():
        group[perm[at:at + n]] = g
        at += n
    return torch.tensor(group)


def three_bins(V, seed=37):
    """int32 [V]: groups 0 and 1 and no group, about a third each, by a seeded draw."""
    g = torch.randint(-1, 2, (V,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    g[0] = -1
    return g


def lzg_bound(count, chunks_per_segment):
    """|logsum - logsum_fp64| <= (4 ln(n) + 7 C + 14) * 2^-24 for a bin of n eligible news: the argument of test_gpu_logz.logz_bound
    with C = 2 * chunks_per_segment, the news one lane sees in one segment of the group-major order (two per chunk).  The three
    rescalings a weight goes through are the same -- the lane's chain, the segment end, the fp64 merge -- and the merge order
    (ascending segments in one thread instead of a butterfly) is fp64 either way: nothing at this scale."""
    return (4.0 * math.log(max(int(count), 2)) + 7.0 * (2 * chunks_per_segment) + 14.0) * EPS


def capped_logp_tolerance(ref, joins):
    """The finalize of row_logprob_capped is fp64 and rounds once: half an ulp of the fp32 result, and `joins` * 2^-49 (1 + |ref|)
    for the fp64 work.  A step's mass is built by at most n_groups + k joins of (max, sum) pairs (the never-closing bins, the
    entries, the bases and stashes of the closing bins); a join is at most two exponentials (1 ulp each), two products, a sum
    and the division of the exponent: 8 roundings of 2^-53 relative on the running mass, 2^-50 a join, and the reference's own
    summation errs likewise: 2^-49 a join.  The final (s - max) / tau - log(mass) adds a few roundings of |ref| size."""
    ref = np.abs(ref)
    return EPS * ref * (1 + 2.0 ** -10) + joins * 2.0 ** -49 * (1 + ref)


# ---- the law under caps (the issue's configuration): news 1 .. 8 with scores LAW_X, c = 1, k = 3 ---------------------------
LAW_GROUP = np.array([-1, 0, 0, 1, 1, 2, -1, -1, 2], dtype=np.int32)      # news 0 .. 8
LAW_CAP, LAW_K = 1, 3
CHI2_PAIRS_MAX = 94.60          # 99.99 % quantile of chi-square, 49 degrees of freedom


def law_pairs():
    """The 50 ordered pairs (first, second place) the cap allows: distinct news that do not share a group."""
    return np.array([(a, b) for a, b in itertools.permutations(range(1, 9), 2) if LAW_GROUP[a] < 0 or LAW_GROUP[a] != LAW_GROUP[b]], dtype=np.int64)


def law_pair_probabilities():
    """float64 [50]: P(first = a, second = b) under sequential sampling from the softmax over what may still be taken."""
    w = np.exp(LAW_X / LAW_TAU)
    p = []
    for a, b in law_pairs():
        closed = [v for v in range(1, 9) if v != a and LAW_GROUP[a] >= 0 and LAW_GROUP[v] == LAW_GROUP[a]]
        p.append(w[a - 1] / w.sum() * w[b - 1] / (w.sum() - w[a - 1] - sum(w[v - 1] for v in closed)))
    return np.array(p)


def law_violations(ids):
    """How many rows of ids [n, k] hold more than LAW_CAP news of one group."""
    bad = 0
    for row in np.asarray(ids, dtype=np.int64):
        g = LAW_GROUP[row[row > 0]]
        g = g[g >= 0]
        bad += int(len(g) and np.bincount(g).max() > LAW_CAP)
    return bad


def law_pairs_chi2(ids, p):
    """Pearson chi-square of the first two places of ids [n, >= 2] against the pair probabilities p (law_pairs' order); every
    drawn pair must be one of the 50."""
    ids = np.asarray(ids, dtype=np.int64)
    index = {(int(a), int(b)): i for i, (a, b) in enumerate(law_pairs())}
    seen = np.zeros(len(index))
    for a, b in ids[:, :2]:
        seen[index[int(a), int(b)]] += 1                                 # KeyError: a pair the cap forbids
    want = len(ids) * np.asarray(p, dtype=np.float64)
    return float(((seen - want) ** 2 / want).sum())


# ---- the enumeration: 5 news, groups {1, 2}, {3, 4} and news 5 in none, c = 1, every ordered row of 3 --------------------
ENUM_X = np.array([0.0, 0.3, -1.2, 2.1, 0.9, -0.4])
ENUM_GROUP = np.array([-1, 0, 0, 1, 1, -1], dtype=np.int32)


def enum_rows():
    rows = np.array(list(itertools.permutations(range(1, 6), 3)), dtype=np.int64)
    forbidden = np.array([({1, 2} <= set(r)) or ({3, 4} <= set(r)) for r in rows.tolist()])
    return rows, forbidden
