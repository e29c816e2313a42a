"""GPU: group caps in the full-corpus top-k ("at most c news of one group in a row": ops.score_topk(..., group=, group_cap=),
train.recommend(..., news_group=, group_cap=)) against the host statement metrics.topk_reference, against the plain call and
against the project's own uncapped passes.

Every comparison is exact.  Where the reference is float64 the vectors are integer valued and the priors multiples of 1/4, so
every fp32 sum is exact in any order and equals the reference, with plenty of ties; float data is only compared with the
device's own results, bit for bit.  Shapes: V = 17 is a partial chunk, V = 1000 several chunks and slices with a ragged end;
U = 65 crosses the 64-user tile; N = 24 is a padded k-slab, N = 400 full ones; k = 128 fills every lane of the candidate list."""
import numpy as np
import pytest
import torch

from helpers import build_model
from newsrecommendation_amd import metrics, ops, train as TR

pytestmark = pytest.mark.gpu

INF = float("inf")
bits = lambda a: np.ascontiguousarray(a).view(np.int32)


def _ints(V, U, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, (V, N), generator=g).float(), torch.randint(-2, 3, (U, N), generator=g).float()


def _floats(V, U, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(V, N, generator=g) * 0.4, torch.randn(U, N, generator=g) * 0.4


def _groups(V, n_groups, negative, seed):
    """Random group ids in [0, n_groups); with `negative`, every tenth id is in no group (-1, -2 or -3)."""
    group = np.random.default_rng(seed).integers(0, n_groups, V).astype(np.int32)
    if negative:
        no = np.arange(V) % 10 == 3
        group[no] = -1 - (np.arange(V)[no] // 10) % 3
    return group


def _topk(news, user, k, exclude=None, splits=0, group=None, group_cap=None, **kw):
    ex = None if exclude is None else torch.as_tensor(exclude, dtype=torch.int32).cuda()
    dev = {n: torch.from_numpy(np.ascontiguousarray(v)).cuda() for n, v in kw.items()}
    gr = None if group is None else torch.from_numpy(np.ascontiguousarray(group, dtype=np.int32)).cuda()
    ids, sc = ops.score_topk(news, user, k, exclude=ex, splits=splits, group=gr, group_cap=group_cap, **dev)
    assert ids.dtype == torch.int32 and sc.dtype == torch.float32 and ids.shape == sc.shape == (user.shape[0], k)
    return ids.cpu().numpy(), sc.cpu().numpy()


def _host_walk(ids, sc, group, cap, k):
    """One finished uncapped row walked with the cap: (ids, scores) of the first k taken, and how many were taken."""
    out_i, out_s, taken = [], [], {}
    for v, s in zip(ids.tolist(), sc.tolist()):
        if v == 0 or len(out_i) == k:
            break
        g = int(group[v])
        if g >= 0:
            if taken.get(g, 0) >= cap:
                continue
            taken[g] = taken.get(g, 0) + 1
        out_i.append(v)
        out_s.append(s)
    n = len(out_i)
    return np.array(out_i + [0] * (k - n), np.int32), np.array(out_s + [-INF] * (k - n), np.float32), n


def _assert_caps_hold(ids, group, cap):
    for row in ids:
        g = group[row[row != 0]]
        g = g[g >= 0]
        assert len(g) == 0 or np.bincount(g).max() <= cap


@pytest.mark.parametrize("V", [17, 1000])
@pytest.mark.parametrize("N", [24, 400])
def test_exact_grid_against_the_reference(N, V):
    """U in {1, 65} x k in {10, 128} x splits in {0, 1, 3} x cap in {1, 3} x two group layouts: ids and scores equal the
    reference exactly.  One reference per (layout, cap): the 128 best of 65 users; the walk stops after k, so a smaller k is its
    prefix, and a smaller U its rows.  Layout "few": 4 groups, no negative id -- at most 4 * cap entries, the rest fill."""
    news, user = _ints(V, 65, N, seed=1000 * N + V)
    news_d, user_d = news.cuda(), user.cuda()
    layouts = {"few": (np.arange(V) % 4).astype(np.int32), "many": _groups(V, 40, True, seed=V + 2)}
    assert (layouts["few"] >= 0).all() and (layouts["many"] < 0).any() and (layouts["many"] >= 0).any()
    for name, group in layouts.items():
        for cap in (1, 3):
            ref_ids, ref_sc = metrics.topk_reference(news.numpy(), user.numpy(), k=128, group=group, group_cap=cap)
            _assert_caps_hold(ref_ids, group, cap)
            if name == "few":                                                          # short rows: exactly 4 * cap entries, then the fill
                assert ((ref_ids != 0).sum(1) == min(4 * cap, V - 1)).all() and np.isneginf(ref_sc[:, 4 * cap:]).all()
            elif V >= 1000:
                assert (ref_ids[:, :100] != 0).all() and len(np.unique(ref_sc)) < ref_sc.size // 4      # long rows, plenty of ties
            for U in (1, 65):
                for k in (10, 128):
                    for splits in (0, 1, 3):
                        ids, sc = _topk(news_d, user_d[:U].contiguous(), k, splits=splits, group=group, group_cap=cap)
                        assert np.array_equal(ids, ref_ids[:U, :k]), (name, cap, U, k, splits)
                        assert np.array_equal(sc, ref_sc[:U, :k]), (name, cap, U, k, splits)


def test_caps_with_pools_and_exclusions():
    """Prior (some -inf, one NaN) + window + an exclusion list that names every user's three best news: whatever is excluded,
    has a -inf prior, lies outside the window or has a NaN score uses up nothing of its group's cap."""
    V, U, N = 1000, 65, 24
    news, user = _ints(V, U, N, seed=5)
    g = np.random.default_rng(6)
    prior = (g.integers(-8, 9, V) / 4.0).astype(np.float32)
    prior[g.random(V) < 0.1] = -INF
    prior[333] = np.nan
    stamp = g.integers(0, 10, V).astype(np.int32)
    window = np.sort(g.integers(0, 10, (U, 2)), axis=1).astype(np.int32)
    window[0], window[1], window[2] = [2, 7], [5, 4], [0, 9]
    group = _groups(V, 12, True, seed=7)
    pools = dict(prior=prior, stamp=stamp, window=window)
    best = metrics.topk_reference(news.numpy(), user.numpy(), k=3, **pools)[0]
    ex = np.concatenate([best, g.integers(0, V, (U, 5)).astype(np.int32)], 1)
    for cap in (1, 3):
        ref_ids, ref_sc = metrics.topk_reference(news.numpy(), user.numpy(), k=128, exclude=ex, group=group, group_cap=cap, **pools)
        _assert_caps_hold(ref_ids, group, cap)
        assert not (ref_ids == 333).any() and (ref_ids[1] == 0).all() and (ref_ids[2, :10] != 0).all()
        # the cap matters, and so does what does not count: neither the plain pooled row nor the capped row without the exclusions is this row
        assert not np.array_equal(ref_ids[:, :10], metrics.topk_reference(news.numpy(), user.numpy(), k=10, exclude=ex, **pools)[0])
        assert not np.array_equal(ref_ids[:, :10], metrics.topk_reference(news.numpy(), user.numpy(), k=10, group=group, group_cap=cap, **pools)[0])
        for k in (10, 128):
            for splits in (0, 1, 3):
                ids, sc = _topk(news.cuda(), user.cuda(), k, exclude=ex, splits=splits, group=group, group_cap=cap, **pools)
                assert np.array_equal(ids, ref_ids[:, :k]) and np.array_equal(sc, ref_sc[:, :k]), (cap, k, splits)


@pytest.fixture(scope="module")
def float_case():
    """Float data shared by the bitwise tests: 4 099 news, 65 users, N = 400, an exclusion list, and the plain k = 128 rows."""
    V, U = 4099, 65
    news, user = _floats(V, U, 400, seed=11)
    news_d, user_d = news.cuda(), user.cuda()
    ex = np.random.default_rng(2).integers(1, V, (U, 8)).astype(np.int32)
    ids0, sc0 = _topk(news_d, user_d, 128, exclude=ex)
    return V, U, news_d, user_d, ex, ids0, sc0


def test_neutral_inputs_are_the_plain_call_bitwise(float_case):
    V, U, news_d, user_d, ex, ids0, sc0 = float_case
    some = _groups(V, 8, True, seed=3)
    for k in (10, 128):
        for kw in (dict(group=some, group_cap=k), dict(group=np.full(V, -1, np.int32), group_cap=1), dict(group=None, group_cap=None)):
            for splits in (0, 3):
                ids, sc = _topk(news_d, user_d, k, exclude=ex, splits=splits, **kw)
                assert np.array_equal(ids, ids0[:, :k]) and np.array_equal(bits(sc), bits(sc0[:, :k])), (k, kw["group_cap"], splits)


def test_independent_of_splits_and_of_the_place_in_the_tile_bitwise(float_case):
    V, U, news_d, user_d, ex, ids0, sc0 = float_case
    for n_groups, cap, k in ((8, 2, 10), (40, 3, 128)):
        group = _groups(V, n_groups, True, seed=n_groups)
        rows = [_topk(news_d, user_d, k, exclude=ex, splits=s, group=group, group_cap=cap) for s in (0, 1, 3, 7)]
        for ids, sc in rows[1:]:
            assert np.array_equal(ids, rows[0][0]) and np.array_equal(bits(sc), bits(rows[0][1]))
        _assert_caps_hold(rows[0][0], group, cap)
        assert not np.array_equal(rows[0][0], ids0[:, :k])                             # the cap changed something
        for splits in (0, 3):
            ids, sc = _topk(news_d, user_d[64:65].contiguous(), k, exclude=ex[64:65], splits=splits, group=group, group_cap=cap)
            assert np.array_equal(ids[0], rows[0][0][64]) and np.array_equal(bits(sc[0]), bits(rows[0][1][64])), splits


def test_against_the_uncapped_passes(float_case):
    """G = 8, c = 2, k = 10.  The plain k = 128 row walked on the host with the cap reaches 10 entries for every user and is the
    capped call's row, ids and score bits; score_rank (which knows no caps) ranks the capped row's ids strictly increasing,
    each at >= its place + 1, with the row's score bits."""
    V, U, news_d, user_d, ex, ids0, sc0 = float_case
    group = _groups(V, 8, False, seed=8)
    ids, sc = _topk(news_d, user_d, 10, exclude=ex, group=group, group_cap=2)
    for u in range(U):
        w_ids, w_sc, n = _host_walk(ids0[u], sc0[u], group, 2, 10)
        assert n == 10, u
        assert np.array_equal(ids[u], w_ids) and np.array_equal(bits(sc[u]), bits(w_sc)), u
    ranks, rsc, _ = ops.score_rank(news_d, user_d, torch.from_numpy(ids).cuda(), exclude=torch.from_numpy(ex).cuda(), ks=None)
    ranks, rsc = ranks.cpu().numpy(), rsc.cpu().numpy()
    assert (np.diff(ranks, axis=1) > 0).all() and (ranks >= np.arange(1, 11)[None, :]).all()
    assert (ranks > np.arange(1, 11)[None, :]).any()                                   # somebody was skipped
    assert np.array_equal(bits(rsc), bits(sc))


def _arrival_cases(V):
    """(name, scores by id, group by id, k, cap): N = 4, news[v] = (s_v, 0, 0, 0), so the score of user (1, 0, 0, 0) is s_v and
    of user (-1, 0, 0, 0) it is -s_v."""
    v = np.arange(V, dtype=np.float64)
    cases = [("ascending: every candidate exchanges", v.copy(), (np.arange(V) % 5).astype(np.int32), 10, 2),
             ("descending: none does after the fill", V - v, (np.arange(V) % 5).astype(np.int32), 10, 2),
             ("ascending, ungrouped ids among them", v.copy(), np.where(np.arange(V) % 7 == 0, -1, np.arange(V) % 3).astype(np.int32), 10, 3)]
    for off in (0, 97):                                                                # 97: the story straddles the first slice end of splits = 3
        s = -v - 10.0                                                                  # the filler: below everything, ungrouped
        grp = np.full(V, -1, np.int32)
        i = 1 + off
        # group 0 fills its cap (1, 2), two ungrouped (10, 11) fill the list: the group's minimum 1 is the overall minimum.  Then group 0
        # brings 5 (replaces 1), an ungrouped 3 replaces the overall minimum 2
        s[i:i + 6], grp[i:i + 6] = [1, 2, 10, 11, 5, 3], [0, 0, -1, -1, 0, -1]
        cases.append((f"saturated group, its minimum is the overall minimum, offset {off}", s, grp, 4, 2))
        s, grp = -v - 10.0, np.full(V, -1, np.int32)
        # group 0 fills its cap high (20, 21), ungrouped 1, 2 fill the list.  Group 0 brings 22: it must push out 20, not the overall minimum 1;
        # then 5, above the threshold but below the group's minimum: dropped; an ungrouped 3 replaces 1
        s[i:i + 7], grp[i:i + 7] = [20, 21, 1, 2, 22, 5, 3], [0, 0, -1, -1, 0, 0, -1]
        cases.append((f"saturated group, its minimum is not the overall minimum, offset {off}", s, grp, 4, 2))
        s, grp = V - v, (np.arange(V) % 4).astype(np.int32)
        s[V - 1], grp[V - 1] = 1000.0, grp[1]                                          # the best of all comes last, into a group that has long been full
        s[i + 150], grp[i + 150] = 900.0, grp[1]
        cases.append((f"a late best item of a saturated group, offset {off}", s, grp, 8, 2))
    return cases


def test_order_of_arrival():
    V = 300
    user = torch.tensor([[1.0, 0, 0, 0], [-1.0, 0, 0, 0]]).cuda()
    for name, s, group, k, cap in _arrival_cases(V):
        news = torch.zeros(V, 4)
        news[:, 0] = torch.from_numpy(s).float()
        ref_ids, ref_sc = metrics.topk_reference(news.numpy(), user.cpu().numpy(), k=k, group=group, group_cap=cap)
        if "not the overall" in name:
            assert sorted(ref_sc[0].tolist()) == [2.0, 3.0, 21.0, 22.0], name
        if "is the overall" in name:
            assert sorted(ref_sc[0].tolist()) == [3.0, 5.0, 10.0, 11.0], name
        if "late best" in name:
            assert ref_ids[0, 0] == V - 1 and ref_sc[0, 1] == 900.0, name
        for splits in (1, 3):
            ids, sc = _topk(news.cuda(), user, k, splits=splits, group=group, group_cap=cap)
            assert np.array_equal(ids, ref_ids) and np.array_equal(sc, ref_sc), (name, splits, ids, ref_ids)


def _corpus(n_news, seed):
    g = torch.Generator().manual_seed(seed)
    nc = torch.randint(1, 12, (n_news + 1, 4), generator=g, dtype=torch.int32)       # word ids of a 12-word vocabulary
    cut = torch.randint(1, 5, (n_news + 1,), generator=g)
    nc[torch.arange(4)[None, :] >= cut[:, None]] = 0                                  # titles of 1 .. 4 words
    nc[0] = 0
    return nc


def test_recommend_end_to_end():
    """A small NRMS model over 100 news, 6 categories (some news in none), at most 2 per category in a row of 10: the row is the
    host walk of the same call's uncapped k = 128 row, and a call without the arguments is the call it was."""
    model, z, cfg, sd = build_model("nrms_tiny_mask", "fp32")
    n_news, U, H, k, cap = 100, 40, cfg.user_log_length, 10, 2
    V = n_news + 1
    nc = _corpus(n_news, seed=51)
    g = torch.Generator().manual_seed(52)
    hist = torch.randint(1, V, (U, H), generator=g, dtype=torch.int32)
    mask = torch.ones(U, H)
    for u in range(2, U):                                                    # front padded
        n_pad = int(torch.randint(0, H, (1,), generator=g))
        hist[u, :n_pad], mask[u, :n_pad] = 0, 0
    news_vecs = TR.encode_news(model, nc, 64, torch.device("cuda"))
    category = _groups(V, 6, True, seed=54).astype(np.int64)                  # a host array, as the pool arguments are
    full_ids, full_sc = (t.cpu().numpy() for t in TR.recommend(model, news_vecs, hist.numpy(), mask.numpy(), 128))
    got_ids, got_sc = (t.cpu().numpy() for t in TR.recommend(model, news_vecs, hist.numpy(), mask.numpy(), k, news_group=category, group_cap=cap))
    _assert_caps_hold(got_ids, category, cap)
    for u in range(U):
        w_ids, w_sc, n = _host_walk(full_ids[u], full_sc[u], category, cap, k)
        assert n == k, u
        assert np.array_equal(got_ids[u], w_ids) and np.array_equal(bits(got_sc[u]), bits(w_sc)), u
    assert not np.array_equal(got_ids, full_ids[:, :k])
    for kw in ({}, dict(news_group=None, group_cap=None)):
        ids, sc = (t.cpu().numpy() for t in TR.recommend(model, news_vecs, hist.numpy(), mask.numpy(), k, **kw))
        assert np.array_equal(ids, full_ids[:, :k]) and np.array_equal(bits(sc), bits(full_sc[:, :k]))
    with pytest.raises(RuntimeError, match="group_cap"):
        TR.recommend(model, news_vecs, hist.numpy(), mask.numpy(), k, news_group=category)
