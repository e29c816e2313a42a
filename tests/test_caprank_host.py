"""CPU: the host side of the capped rank (include/nrhip.h K10, group / group_cap / n_groups) -- metrics.rank_reference with caps
against metrics.topk_reference with caps and against the closed formula of the contract, a numpy model of the device scheme
(per-slice per-group integer counts, the per-group take-back of the listed ids, the finalize) against the definition,
metrics.retrieval_metrics_reference with -1 entries, the descriptor layout and the workspace arithmetic, the refusals
nr_score_rank makes before it launches anything, and the several-rows layout of train.rank_eval at 4 targets per row."""
import ctypes as C
import math

import numpy as np
import pytest

from newsrecommendation_amd import _lib, metrics

INF = float("inf")


def _case(g, V=None):
    """One random tied integer case: scores [U, V], prior with -inf and NaN, stamps + windows, ragged exclusion lists (ids out of
    range and repeats among them), groups with negative ids, a cap."""
    V = int(g.integers(8, 40)) if V is None else V
    U = int(g.integers(1, 4))
    scores = g.integers(-3, 4, (U, V)).astype(np.float64)
    prior = g.integers(-2, 3, V).astype(np.float64)
    prior[g.random(V) < 0.1] = -INF
    prior[g.random(V) < 0.05] = np.nan
    stamp = g.integers(0, 6, V)
    window = np.sort(g.integers(0, 6, (U, 2)), axis=1)
    if g.random() < 0.2:
        window[0] = [0, 5]
    exclude = [g.integers(-1, V + 3, int(g.integers(0, 9))) for _ in range(U)]
    G = int(g.choice([1, 2, 3, 5, 9]))
    group = g.integers(0, G, V)
    group[g.random(V) < 0.15] = -1 - int(g.integers(0, 3))
    cap = int(g.choice([1, 1, 2, 3]))
    return scores, dict(prior=prior, stamp=stamp, window=window), exclude, group, G, cap


def _eligible(scores, pools, exclude, u):
    """(final scores of user u, eligibility mask) spelled out once more, independently of metrics._pooled."""
    V = scores.shape[1]
    with np.errstate(invalid="ignore"):
        s = scores[u] + pools["prior"]
    ok = ~np.isnan(s) & ~np.isneginf(pools["prior"])
    ok &= (pools["window"][u, 0] <= pools["stamp"]) & (pools["stamp"] <= pools["window"][u, 1])
    ok[0] = False
    for e in exclude[u]:
        if 1 <= e < V:
            ok[e] = False
    return s, ok


def _beats(s, v, t):
    """News v stands in front of news t in the total order (score descending, id ascending)."""
    return s[v] > s[t] or (s[v] == s[t] and v < t)


def test_capped_reference_against_the_capped_topk_reference_and_the_closed_formula():
    g = np.random.default_rng(2024)
    n_capped_out = n_moved = 0
    for case in range(300):
        scores, pools, exclude, group, G, cap = _case(g)
        U, V = scores.shape
        everything = np.tile(np.arange(-1, V + 2), (U, 1))                      # every id, and three that mean nothing
        kw = dict(exclude=exclude, **pools)
        ranks, sc = metrics.rank_reference(scores, targets=everything, group=group, group_cap=cap, **kw)
        plain, plain_sc = metrics.rank_reference(scores, targets=everything, **kw)
        row_ids, row_sc = metrics.topk_reference(scores, k=max(128, V), group=group, group_cap=cap, **kw)
        assert ranks.dtype == np.int32 and ranks.min() >= -1
        for u in range(U):
            s, ok = _eligible(scores, pools, exclude, u)
            for k in (1, 5, 128):
                in_row = {(p + 1, int(v), row_sc[u, p]) for p, v in enumerate(row_ids[u, :k]) if v != 0}
                ranked = {(int(ranks[u, j]), int(everything[u, j]), sc[u, j]) for j in range(V + 3) if 1 <= ranks[u, j] <= k}
                assert in_row == ranked, (case, u, k)
            for j, t in enumerate(everything[u]):
                r = int(ranks[u, j])
                if not (1 <= t < V and ok[t]):
                    assert r == 0 and np.isneginf(sc[u, j]) and plain[u, j] == 0, (case, u, t)
                    continue
                assert r != 0 and sc[u, j] == s[t] == plain_sc[u, j] and plain[u, j] > 0, (case, u, t)
                n_g = np.zeros(G, np.int64)
                n_none = 0
                for v in np.flatnonzero(ok):
                    if _beats(s, v, t):
                        if group[v] >= 0:
                            n_g[group[v]] += 1
                        else:
                            n_none += 1
                assert plain[u, j] == 1 + n_none + n_g.sum()
                if group[t] >= 0 and n_g[group[t]] >= cap:                       # capped out: eligible, and in no row even at k = V
                    assert r == -1 and t not in row_ids[u], (case, u, t)
                    n_capped_out += 1
                else:
                    assert r == 1 + n_none + np.minimum(n_g, cap).sum() == plain[u, j] - np.maximum(n_g - cap, 0).sum(), (case, u, t)
                    n_moved += r != plain[u, j]
    assert n_capped_out > 500 and n_moved > 500                                 # both branches of the contract were exercised


def _device_model(scores, pools, exclude, targets, group, G, cap, bounds):
    """The scheme of csrc/nr_rank.hip in numpy integers.  key(v) != 0 <=> in range, score not NaN, inside the pool: the stream counts
    those, excluded or not, per slice [bounds[i], bounds[i+1]) and per group (a group id outside [0, G) = no group); the named
    pass takes back, in total and per group, each listed news once that is in range, has key != 0 and beats the target; the
    finalize applies the capped-out test to the target's own group and gives back what every group has beyond the cap."""
    U, V = scores.shape
    T = targets.shape[1]
    ranks, out = np.zeros((U, T), np.int32), np.full((U, T), -INF)
    for u in range(U):
        with np.errstate(invalid="ignore"):
            s = scores[u] + pools["prior"]
        key = ~np.isnan(s) & ~np.isneginf(pools["prior"]) & (pools["window"][u, 0] <= pools["stamp"]) & (pools["stamp"] <= pools["window"][u, 1])
        key[0] = False
        listed = sorted({int(e) for e in exclude[u] if 1 <= e < V})
        grp = np.where((group >= 0) & (group < G), group, -1)
        for j in range(T):
            t = int(targets[u, j])
            if not (1 <= t < V) or not key[t] or t in listed or t in [int(x) for x in targets[u, :j]]:
                continue
            total, counters = 0, np.zeros(G, np.int64)
            for x in listed:                                                    # the named pass initialises the counters to minus the take-back
                if key[x] and _beats(s, x, t):
                    total -= 1
                    if grp[x] >= 0:
                        counters[grp[x]] -= 1
            for lo, hi in zip(bounds[:-1], bounds[1:]):                         # one slice: its own integer counts, added
                part, gpart = 0, np.zeros(G, np.int64)
                for v in range(lo, hi):
                    if key[v] and _beats(s, v, t):
                        part += 1
                        if grp[v] >= 0:
                            gpart[grp[v]] += 1
                total += part
                counters += gpart
            assert (counters >= 0).all()
            out[u, j] = s[t]
            if grp[t] >= 0 and counters[grp[t]] >= cap:
                ranks[u, j] = -1
            else:
                ranks[u, j] = 1 + total - np.maximum(counters - cap, 0).sum()
    return ranks, out


def test_device_scheme_model_against_the_definition():
    g = np.random.default_rng(77)
    seen_minus_one = 0
    for case in range(200):
        scores, pools, exclude, group, G, cap = _case(g)
        U, V = scores.shape
        targets = g.integers(-1, V + 2, (U, 4))
        targets[:, 2] = targets[:, 0]                                           # a repeat
        if len(exclude[0]):
            targets[0, 1] = exclude[0][0]                                       # a listed target
        cuts = np.sort(g.integers(1, V + 1, int(g.integers(0, 4))))
        bounds = [1, *cuts.tolist(), V]
        want = metrics.rank_reference(scores, targets=targets, exclude=exclude, group=group, group_cap=cap, **pools)
        got = _device_model(scores, pools, exclude, targets, group, G, cap, bounds)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (case, got[0], want[0])
        seen_minus_one += int((want[0] == -1).sum())
    assert seen_minus_one > 20


def test_neutral_caps_are_the_plain_reference():
    g = np.random.default_rng(5)
    for _ in range(20):
        scores, pools, exclude, group, G, cap = _case(g)
        U, V = scores.shape
        targets = g.integers(0, V, (U, 6))
        want = metrics.rank_reference(scores, targets=targets, exclude=exclude, **pools)
        for kw in (dict(group=np.full(V, -2), group_cap=1), dict(group=group, group_cap=128)):
            got = metrics.rank_reference(scores, targets=targets, exclude=exclude, **pools, **kw)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with pytest.raises(ValueError, match="come together"):
        metrics.rank_reference(scores, targets=targets, group=group)
    with pytest.raises(ValueError, match="group_cap = 129"):
        metrics.rank_reference(scores, targets=targets, group=group, group_cap=129)


def test_retrieval_metrics_with_capped_out_entries():
    l2 = math.log2
    ranks = np.array([[1, -1, 4], [-1, -1, 0], [0, 0, 0], [3, 2, 12]])
    per_user, sums = metrics.retrieval_metrics_reference(ranks, (2, 10))
    want = np.array([
        # n_u = 3: the capped-out click is counted, hits nothing, and the ideal DCG keeps min(3, k) terms
        [1, (1 + 1 / 4) / 3, 1 / 3, 1.0 / (1 + 1 / l2(3)), 2 / 3, (1 + 1 / l2(5)) / (1 + 1 / l2(3) + 1 / l2(4))],
        [1, 0, 0, 0, 0, 0],                                                       # two clicks, neither can be shown: a counted user of zeros
        [0, 0, 0, 0, 0, 0],
        [1, (1 / 3 + 1 / 2 + 1 / 12) / 3, 1 / 3, (1 / l2(3)) / (1 + 1 / l2(3)), 2 / 3, (1 / l2(4) + 1 / l2(3)) / (1 + 1 / l2(3) + 1 / l2(4))],
    ])
    assert np.allclose(per_user, want, rtol=1e-14, atol=0) and sums[0] == 3.0
    assert np.allclose(sums, want.sum(0), rtol=1e-14)
    # without a negative rank: what the function always returned, bit for bit (n_u = #{rank > 0}, the same operations)
    g = np.random.default_rng(3)
    plain = g.integers(0, 50, (40, 7))
    plain[5] = 0
    got_u, got_s = metrics.retrieval_metrics_reference(plain, (1, 5, 100))
    for u, row in enumerate(plain):
        r = row[row > 0].astype(np.float64)
        if len(r) == 0:
            assert not got_u[u].any()
            continue
        assert got_u[u, 0] == 1.0 and got_u[u, 1] == np.sum(1.0 / r) / len(r)
        for i, k in enumerate((1, 5, 100)):
            hit = r[r <= k]
            assert got_u[u, 2 + 2 * i] == len(hit) / len(r)
            assert got_u[u, 3 + 2 * i] == np.sum(1.0 / np.log2(hit + 1.0)) / np.sum(1.0 / np.log2(np.arange(min(len(r), k)) + 2.0))
    assert np.array_equal(got_s, got_u.sum(axis=0))


def test_retrieval_sums_of_the_row_split_with_capped_out_entries():
    import torch
    from newsrecommendation_amd import train
    g = np.random.default_rng(10)
    ranks = g.integers(-1, 200, (9, 11)).astype(np.int32)
    ranks[3] = 0
    ranks[4] = -1
    ranks[5, 1:] = 0
    ks = (1, 5, 10, 100)
    got = train._retrieval_sums(torch.from_numpy(ranks), ks).numpy()
    assert np.allclose(got, metrics.retrieval_metrics_reference(ranks, ks)[1], rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------------------------- the descriptor
_KS = (C.c_int * 3)(5, 10, 100)


def _desc(**changes):
    f = dict(news_vecs=4096, ld_news=400, V=100001, user=4096, ld_user=400, U=8192, N=400, T=4, targets=4096, ld_targets=4, exclude=4096,
             ld_exclude=50, E=50, splits=0, ks=_KS, n_ks=3, out_ranks=4096, out_scores=4096, out_sums=4096, ws=4096)
    f.update(changes)
    d = _lib.RankDesc(**f)
    if "ws_bytes" not in changes:
        d.ws_bytes = _lib.lib().nr_score_rank_workspace_bytes(C.byref(d))
    return d


def test_descriptor_layout():
    names = [f[0] for f in _lib.RankDesc._fields_]
    assert names[-6:] == ["ws", "ws_bytes", "prior", "stamp", "window", "ld_window"]              # the shared tail stays last
    assert names[-9:-6] == ["group", "group_cap", "n_groups"] and names[-10] == "out_sums"
    sizes = (C.c_size_t * 9)()
    assert _lib.lib().nr_abi_sizes(sizes, 9) == 0 and sizes[8] == C.sizeof(_lib.RankDesc)
    assert _lib.NR_RANK_MAX_GROUPS == 512 and _lib.NR_RANK_MAX_CAPPED_TARGETS >= 4
    d = _lib.RankDesc()
    assert d.group is None and d.group_cap == 0 and d.n_groups == 0


def _plain_bytes(U, T, n_ks, splits):
    """The workspace of a call without group caps, as it was before they existed: keys, terms, part, excl, pos, nu."""
    ut = U * T
    return ut * 8 + U * (2 + 2 * n_ks) * 8 + ut * splits * 4 + ut * 4 + ut * 4 + U * 4


def test_workspace_is_todays_without_group_and_grows_only_with_it():
    lib = _lib.lib()
    size = lambda **c: lib.nr_score_rank_workspace_bytes(C.byref(_desc(**c)))
    for U, T, n_ks, splits in ((8192, 4, 3, 2), (64, 4, 3, 7), (65, 64, 0, 1), (3, 1, 3, 256)):
        assert size(U=U, T=T, ld_targets=T, n_ks=n_ks, splits=splits) == _plain_bytes(U, T, n_ks, splits)
    # the library's own choice of slices without caps: 256 CUs over the 64-user tiles of N = 400, at most one slice per chunk
    assert size(U=64) == _plain_bytes(64, 4, 3, 256) and size(U=8192) == _plain_bytes(8192, 4, 3, 2)
    V, U, T = 100001, 8192, 4
    for G in (1, 18, 70, 285, 512):
        for splits in (1, 2, 7):
            per = -(-(V - 1) // splits)
            chunks = splits * -(-per // 128)
            base = (_plain_bytes(U, T, 3, splits) + 7) // 8 * 8
            want = base + chunks * G * 16 + U * T * G * 4 + 2 * U * T * 4      # masks, counters, slot, target groups
            assert size(splits=splits, group=4096, group_cap=2, n_groups=G) == want, (G, splits)
    assert size(splits=2, group=4096, group_cap=2, n_groups=18) < 8192 * 100001 * 4 // 64      # still far below a score matrix


REFUSED = {
    "group_without_cap": (dict(group=4096, n_groups=18), "group_cap = 0"),
    "cap_129": (dict(group=4096, group_cap=129, n_groups=18), "group_cap = 129"),
    "negative_cap": (dict(group=4096, group_cap=-1, n_groups=18), "group_cap = -1"),
    "cap_without_group": (dict(group_cap=2), "group_cap = 2 given without group"),
    "n_groups_without_group": (dict(n_groups=18), "n_groups = 18 given without group"),
    "n_groups_0": (dict(group=4096, group_cap=2), "n_groups = 0"),
    "n_groups_513": (dict(group=4096, group_cap=2, n_groups=513), "n_groups = 513"),
    "T_5_with_caps": (dict(group=4096, group_cap=2, n_groups=18, T=5, ld_targets=5), "T = 5"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_before_any_launch(case):
    change, message = REFUSED[case]
    d = _desc(**change)
    assert d.ws_bytes == 0                                                   # the size query refuses the same descriptors
    rc = _lib.lib().nr_score_rank(C.byref(d), None)
    assert rc == 1 and message in _lib.last_error(), _lib.last_error()


def test_score_rank_capped_has_no_cpu_fallback():
    import torch
    from newsrecommendation_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_rank_capped(torch.zeros(10, 8), torch.zeros(3, 8), torch.ones(3, 2, dtype=torch.int32), torch.zeros(10, dtype=torch.int32), 1,
                              n_groups=1)
    with pytest.raises(RuntimeError, match="group is None"):
        ops.score_rank_capped(torch.zeros(10, 8), torch.zeros(3, 8), torch.ones(3, 2, dtype=torch.int32), None, 1)


def test_capped_entry_points_stand_beside_the_plain_ones():
    """The plain calls keep their argument lists (other host tests pin them); the caps come through functions of their own."""
    import inspect
    from newsrecommendation_amd import ops, train
    assert list(inspect.signature(ops.score_rank_capped).parameters)[:6] == ["news_vecs", "user_vecs", "targets", "group", "group_cap", "n_groups"]
    for fn in (train.rank_eval_capped, train.rank_shard_capped):
        p = inspect.signature(fn).parameters
        assert p["news_group"].default is inspect.Parameter.empty and p["group_cap"].default is inspect.Parameter.empty and "seen" in p
    for plain, capped in ((ops.score_rank, ops.score_rank_capped), (train.rank_eval, train.rank_eval_capped), (train.rank_shard, train.rank_shard_capped)):
        extra = set(inspect.signature(capped).parameters) - set(inspect.signature(plain).parameters)
        assert extra in ({"group", "group_cap", "n_groups"}, {"news_group", "group_cap"})


def test_row_split_of_rank_eval_under_caps_against_the_reference(monkeypatch):
    """train.rank_eval_capped with 9 target columns: a capped call takes 4 targets per row, so the users with more are laid
    over several rows; the device call is replaced by the host reference (the split is tensor arithmetic around it)."""
    import torch
    from newsrecommendation_amd import train
    g = np.random.default_rng(12)
    V, U, T = 60, 5, 9
    news, user = g.integers(-2, 3, (V, 8)).astype(np.float32), g.integers(-2, 3, (U, 8)).astype(np.float32)
    group = g.integers(0, 5, V)
    group[::7] = -1
    targets = np.zeros((U, T), np.int32)
    targets[0] = g.permutation(np.arange(1, V))[:T]                          # 9 targets: three rows
    targets[1, ::3] = g.permutation(np.arange(1, V))[:3]                     # zeros between entries: one row
    targets[2, :6] = g.permutation(np.arange(1, V))[:6]
    targets[2, 6], targets[2, 7] = targets[2, 1], V + 4                      # a repeat across a row boundary, an id >= V
    targets[4, 5] = 17
    hist = g.integers(1, V, (U, 3)).astype(np.int32)
    mask = np.ones((U, 3), np.float32)
    calls = []

    def fake_score_rank_capped(news_vecs, user_vecs, tg, group, group_cap, n_groups=None, exclude=None, ks=(), splits=0):
        assert tg.shape[1] <= _lib.NR_RANK_MAX_CAPPED_TARGETS and ks is None and group.dtype == torch.int32
        calls.append((tuple(tg.shape), group_cap, n_groups))
        r, s = metrics.rank_reference(news_vecs.numpy(), user_vecs.numpy(), targets=tg.numpy(), exclude=None if exclude is None else exclude.numpy(),
                                      group=group.numpy(), group_cap=group_cap)
        return torch.from_numpy(r), torch.from_numpy(s).float(), None

    monkeypatch.setattr(train.ops, "score_rank_capped", fake_score_rank_capped)
    monkeypatch.setattr(train.ops, "score_rank", None)                       # the capped path never takes the plain call
    monkeypatch.setattr(train, "_user_vectors", lambda *a: torch.from_numpy(user))
    ks = (1, 10, 100)
    ranks, scores, sums = train.rank_eval_capped(None, torch.from_numpy(news), hist, mask, targets, group, 1, ks=ks)
    want_r, want_s = metrics.rank_reference(news, user, targets=targets, exclude=hist, group=group, group_cap=1)
    assert (want_r == -1).any() and (want_r > 0).any()
    assert np.array_equal(ranks.numpy(), want_r) and np.array_equal(scores.numpy().astype(np.float64), want_s)
    assert np.allclose(sums.numpy(), metrics.retrieval_metrics_reference(want_r, ks)[1], rtol=1e-12, atol=0)
    assert calls == [((8, 4), 1, 5)]                                         # users 0 and 2 take three and two rows, the others one
