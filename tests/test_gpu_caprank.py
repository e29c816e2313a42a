"""GPU: the capped rank (ops.score_rank_capped(..., group, group_cap, n_groups=), train.rank_eval_capped(..., news_group, group_cap)) against
the host statement metrics.rank_reference, against the capped top-k pass, against the plain call and against itself.

Every comparison of ranks and scores is exact.  Where the reference is float64 the vectors are integer valued and the priors
multiples of 1/4, so every fp32 sum is exact in any order and equals the reference, with plenty of ties; float data is only
compared with the device's own results, bit for bit.  Shapes as in test_gpu_groupcap.py: V = 17 is a partial chunk, V = 1000
several chunks and slices with a ragged end; U = 65 crosses every user tile (16, 32, 64); N = 24 is a padded k-slab, N = 400
full ones; G = 70 crosses a block of 64 groups, G = 512 is the most; T = 4 is the most targets of a capped row."""
import numpy as np
import pytest
import torch

from helpers import build_model
from newsrecommendation_amd import _lib, metrics, ops, train as TR

pytestmark = pytest.mark.gpu

INF = float("inf")
TC = _lib.NR_RANK_MAX_CAPPED_TARGETS
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


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _rank(news_d, user_d, tg, exclude=None, splits=0, group=None, group_cap=None, n_groups=None, ks=None, **kw):
    if isinstance(exclude, np.ndarray):
        exclude = _dev(exclude, np.int32)
    pools = {n: _dev(v) for n, v in kw.items()}
    if group is None:                                                              # the call without caps: the function it always was
        assert group_cap is None and n_groups is None
        ranks, sc, sums = ops.score_rank(news_d, user_d, _dev(tg, np.int32), exclude=exclude, ks=ks, splits=splits, **pools)
    else:
        ranks, sc, sums = ops.score_rank_capped(news_d, user_d, _dev(tg, np.int32), _dev(group, np.int32), group_cap, n_groups=n_groups,
                                                exclude=exclude, ks=ks, splits=splits, **pools)
    assert ranks.dtype == torch.int32 and sc.dtype == torch.float32 and ranks.shape == sc.shape == tuple(np.shape(tg))
    if ks is None:
        return ranks.cpu().numpy(), sc.cpu().numpy()
    return ranks.cpu().numpy(), sc.cpu().numpy(), sums.cpu().numpy()


def _topk(news_d, user_d, k, exclude=None, splits=0, group=None, group_cap=None, **kw):
    if isinstance(exclude, np.ndarray):
        exclude = _dev(exclude, np.int32)
    pools = {n: _dev(v) for n, v in kw.items()}
    ids, sc = ops.score_topk(news_d, user_d, k, exclude=exclude, splits=splits, group=_dev(group, np.int32), group_cap=group_cap, **pools)
    return ids.cpu().numpy(), sc.cpu().numpy()


def _target_sets(full, V, seed):
    """Two [U, 4] target layouts from the capped ranks `full` [U, V] of every id: A = (the user's best news, a capped-out one if
    there is any, id 0, a random id), B = (a random id, an id >= V, a repeat of column 0, a random id)."""
    g = np.random.default_rng(seed)
    U = full.shape[0]
    a, b = g.integers(1, V, (U, 4)).astype(np.int32), g.integers(1, V, (U, 4)).astype(np.int32)
    for u in range(U):
        best, out = np.flatnonzero(full[u] == 1), np.flatnonzero(full[u] == -1)
        if len(best):                                                             # none: nothing is eligible for this user
            a[u, 0] = best[0]
        if len(out):
            a[u, 1] = out[g.integers(0, len(out))]
    a[:, 2] = 0
    b[:, 1] = V + g.integers(0, 5, U)
    b[:, 2] = b[:, 0]
    return a, b


@pytest.mark.parametrize("V", [17, 1000])
@pytest.mark.parametrize("N", [24, 400])
def test_exact_grid_against_the_reference(N, V):
    """U in {1, 65} x T in {1, 4} (4 is the capped maximum) x splits in {0, 1, 3} x cap in {1, 3} x G in {3, 18, 70, 512} x two target
    layouts: ranks and scores equal the reference exactly.  One reference per (G, cap, layout) for 65 users and 4 targets: a
    rank does not depend on the targets behind it, so T = 1 is its first column, and a smaller U its rows."""
    news, user = _ints(V, 65, N, seed=1000 * N + V)
    news_d, user_d = news.cuda(), user.cuda()
    every = np.tile(np.arange(V), (65, 1))
    for G in (3, 18, 70, 512):
        group = _groups(V, G, True, seed=V + G)
        assert (group < 0).any() and (group >= 0).any()
        for cap in (1, 3):
            full, _ = metrics.rank_reference(news.numpy(), user.numpy(), targets=every, group=group, group_cap=cap)
            if G == 3 and cap == 1:
                assert (full == -1).sum() > (full > 0).sum()                          # most targets are capped out
            for layout, tg in zip("AB", _target_sets(full, V, seed=G + cap)):
                ref_r, ref_s = metrics.rank_reference(news.numpy(), user.numpy(), targets=tg, group=group, group_cap=cap)
                if layout == "A":
                    assert (ref_r[:, 0] == 1).all() and (ref_r[:, 2] == 0).all() and ((ref_r[:, 1] == -1).any() or G != 3)
                else:
                    assert (ref_r[:, 1:3] == 0).all()
                for U in (1, 65):
                    for T in sorted({1, 4, TC}):
                        for splits in (0, 1, 3):
                            r, s = _rank(news_d, user_d[:U].contiguous(), tg[:U, :T], splits=splits, group=group, group_cap=cap, n_groups=G)
                            assert np.array_equal(r, ref_r[:U, :T]), (G, cap, U, T, splits, np.argwhere(r != ref_r[:U, :T])[:5])
                            assert np.array_equal(s, ref_s[:U, :T].astype(np.float32)), (G, cap, U, T, splits)


@pytest.fixture(scope="module")
def float_case():
    """Float data shared by the bitwise tests: 4 099 news, 65 users, N = 400, an exclusion list."""
    V, U = 4099, 65
    news, user = _floats(V, U, 400, seed=11)
    ex = np.random.default_rng(2).integers(1, V, (U, 8)).astype(np.int32)
    return V, U, news.cuda(), user.cuda(), ex


def _rank_of_rows(news_d, user_d, rows, exclude, **kw):
    """score_rank of every entry of rows [U, K] (K a multiple of 4): the users repeated over K / 4 capped rows of 4 targets."""
    U, K = rows.shape
    rep = torch.arange(U).repeat_interleave(K // TC).cuda()
    ex = None if exclude is None else np.repeat(exclude, K // TC, axis=0)
    r, s = _rank(news_d, user_d[rep].contiguous(), rows.reshape(U * (K // TC), TC), exclude=ex, **kw)
    return r.reshape(U, K), s.reshape(U, K)


@pytest.mark.parametrize("G", [8, 40])
def test_agrees_with_the_capped_topk_pass_bitwise(float_case, G):
    """Every entry at place p of score_topk(group, cap) fed back as a target has capped rank p + 1 and the same score bits; ids
    outside the row have rank > 128 or -1 (and the excluded ones 0)."""
    V, U, news_d, user_d, ex = float_case
    group, cap = _groups(V, G, True, seed=G), 3
    ids, sc = _topk(news_d, user_d, 128, exclude=ex, group=group, group_cap=cap)
    assert (ids != 0).all()
    for splits in (0, 3):
        r, s = _rank_of_rows(news_d, user_d, ids, ex, splits=splits, group=group, group_cap=cap, n_groups=G)
        assert np.array_equal(r, np.tile(np.arange(1, 129, dtype=np.int32), (U, 1))), (splits, np.argwhere(r != np.arange(1, 129)[None, :])[:5])
        assert np.array_equal(bits(s), bits(sc)), splits
    others = np.random.default_rng(G).integers(1, V, (U, 64)).astype(np.int32)
    r, s = _rank_of_rows(news_d, user_d, others, ex, group=group, group_cap=cap, n_groups=G)
    plain, plain_s = _rank_of_rows(news_d, user_d, others, ex)
    n_out = 0
    for u in range(U):
        for j, t in enumerate(others[u]):
            if t in ids[u]:
                assert r[u, j] == 0 or r[u, j] == 1 + int(np.flatnonzero(ids[u] == t)[0])      # 0: a repeat inside its row of 4
            elif plain[u, j] == 0:
                assert r[u, j] == 0 and np.isneginf(s[u, j])
            else:
                assert r[u, j] > 128 or r[u, j] == -1, (u, j, r[u, j])
                assert r[u, j] <= plain[u, j] and bits(s[u, j:j + 1]) == bits(plain_s[u, j:j + 1])
                n_out += r[u, j] == -1
    assert n_out > 0


def _lists_of_lengths(V, U, best, outside, seed):
    """Ragged exclusion lists of 0, 64, 65 and 300 ids (cycling over the users): each names the user's three best news and three
    news outside the pool, the rest is random."""
    g = np.random.default_rng(seed)
    lists = []
    for u in range(U):
        L = (0, 64, 65, 300)[u % 4]
        ids = np.zeros(0, np.int64)
        if L:
            named = np.concatenate([best[u][best[u] > 0], outside[:3]])              # best is 0 where nothing is eligible
            ids = np.unique(np.concatenate([named, g.permutation(np.arange(1, V))[:L]]))
            keep = np.isin(ids, named)
            ids = np.sort(np.concatenate([ids[keep], ids[~keep][:L - keep.sum()]]))
            assert len(ids) == L
        lists.append(ids.astype(np.int32))
    return lists


def test_caps_with_pools_and_exclusions():
    """Prior (some -inf, one NaN) + window + a dense exclusion list or CSR lists of 0, 64, 65 and 300 ids that name every user's
    three best news and news outside the pool: whatever is excluded, listed, NaN or outside the pool uses up nothing of a cap."""
    V, U, N, G = 1000, 65, 24, 12
    news, user = _ints(V, U, N, seed=5)
    news_d, user_d = news.cuda(), user.cuda()
    g = np.random.default_rng(6)
    prior = (g.integers(-8, 9, V) / 4.0).astype(np.float32)
    prior[g.random(V) < 0.1] = -INF
    prior[333] = np.nan
    stamp = g.integers(0, 10, V).astype(np.int32)
    window = np.sort(g.integers(0, 10, (U, 2)), axis=1).astype(np.int32)
    window[0], window[1], window[2] = [2, 7], [5, 4], [0, 9]
    group = _groups(V, G, True, seed=7)
    pools = dict(prior=prior, stamp=stamp, window=window)
    best = metrics.topk_reference(news.numpy(), user.numpy(), k=3, **pools)[0]
    outside = np.flatnonzero(np.isneginf(prior))
    outside = outside[outside > 0]
    dense = np.concatenate([best, np.tile(outside[:2], (U, 1)), g.integers(0, V, (U, 5))], 1).astype(np.int32)
    lists = _lists_of_lengths(V, U, best, outside, seed=8)
    assert sorted({len(x) for x in lists}) == [0, 64, 65, 300]
    every = np.tile(np.arange(V), (U, 1))
    for name, host_ex, dev_ex in (("dense", dense, dense), ("csr", lists, ops.ExclusionLists(lists, device="cuda"))):
        for cap in (1, 3):
            full, _ = metrics.rank_reference(news.numpy(), user.numpy(), targets=every, exclude=host_ex, group=group, group_cap=cap, **pools)
            assert (full[1] == 0).all() and (full[:, 333] == 0).all()                 # an empty window; the NaN news
            without, _ = metrics.rank_reference(news.numpy(), user.numpy(), targets=every, group=group, group_cap=cap, **pools)
            assert not np.array_equal(full, np.where(full == 0, 0, without))           # the lists move capped ranks: they free places of a cap
            for tg in _target_sets(full, V, seed=cap):
                tg[5::20, 3] = best[5::20, 0]                                          # a listed target (users 5, 25, 45: lists of 64 ids)
                ref_r, ref_s = metrics.rank_reference(news.numpy(), user.numpy(), targets=tg, exclude=host_ex, group=group, group_cap=cap, **pools)
                assert (ref_r == -1).any() and (ref_r > 0).any() and (ref_r[5::20, 3] == 0).all()
                for splits in (0, 3):
                    r, s = _rank(news_d, user_d, tg, exclude=dev_ex, splits=splits, group=group, group_cap=cap, n_groups=G, **pools)
                    assert np.array_equal(r, ref_r), (name, cap, splits, np.argwhere(r != ref_r)[:5])
                    assert np.array_equal(s, ref_s.astype(np.float32)), (name, cap, splits)


def test_neutral_inputs_are_the_plain_call_bitwise(float_case):
    V, U, news_d, user_d, ex = float_case
    tg = np.random.default_rng(4).integers(0, V + 3, (U, 4)).astype(np.int32)
    tg[:, 2] = ex[:, 0]
    r0, s0 = _rank(news_d, user_d, tg, exclude=ex)
    assert (r0 > 0).any() and (r0[:, 2] == 0).all()
    many = _groups(V, 512, True, seed=3)                                               # 4 099 news over 512 groups: none has 128
    assert np.bincount(many[many >= 0]).max() <= 128
    for kw in (dict(group=np.full(V, -1, np.int32), group_cap=1), dict(group=np.full(V, -3, np.int32), group_cap=1, n_groups=70),
               dict(group=many, group_cap=128, n_groups=512), dict(group=many, group_cap=128), dict(group=None, group_cap=None, n_groups=None)):
        for splits in (0, 3):
            r, s = _rank(news_d, user_d, tg, exclude=ex, splits=splits, **kw)
            assert np.array_equal(r, r0) and np.array_equal(bits(s), bits(s0)), (kw.get("n_groups"), kw["group_cap"], splits)
    # a call without `group` is the call it was: the reference without caps (integer data)
    news, user = _ints(1000, 65, 24, seed=9)
    tg = np.random.default_rng(5).integers(0, 1003, (65, 64)).astype(np.int32)
    ref_r, ref_s = metrics.rank_reference(news.numpy(), user.numpy(), targets=tg)
    r, s = _rank(news.cuda(), user.cuda(), tg)
    assert np.array_equal(r, ref_r) and np.array_equal(s, ref_s.astype(np.float32))


def test_independent_of_splits_and_of_the_place_in_the_tile_bitwise(float_case):
    V, U, news_d, user_d, ex = float_case
    tg = np.random.default_rng(6).integers(1, V, (U, 4)).astype(np.int32)
    for G, cap in ((8, 2), (40, 3), (285, 1)):
        group = _groups(V, G, True, seed=G)
        rows = [_rank(news_d, user_d, tg, exclude=ex, splits=sp, group=group, group_cap=cap, n_groups=G) for sp in (1, 2, 7, 0)]
        for r, s in rows[1:]:
            assert np.array_equal(r, rows[0][0]) and np.array_equal(bits(s), bits(rows[0][1]))
        r0, s0 = rows[0]
        assert (r0 == -1).any() and (r0 > 0).any()
        plain, _ = _rank(news_d, user_d, tg, exclude=ex)
        assert (r0[r0 > 0] <= plain[r0 > 0]).all() and (r0[r0 > 0] < plain[r0 > 0]).any()          # the cap changed something
        for splits in (0, 3):
            r, s = _rank(news_d, user_d[64:65].contiguous(), tg[64:65], exclude=ex[64:65], splits=splits, group=group, group_cap=cap, n_groups=G)
            assert np.array_equal(r[0], r0[64]) and np.array_equal(bits(s[0]), bits(s0[64])), splits
        back = np.arange(U)[::-1].copy()                                                # every user at another place of every tile
        r, s = _rank(news_d, user_d[torch.from_numpy(back).cuda()].contiguous(), tg[back], exclude=ex[back], group=group, group_cap=cap, n_groups=G)
        assert np.array_equal(r, r0[back]) and np.array_equal(bits(s), bits(s0[back]))


def test_sums():
    """out_sums against retrieval_metrics_reference of the call's own ranks (which the grid test ties to the reference), with the
    relative tolerance test_gpu_rank.py uses for the sums (fp64 terms, another order of summation); two calls give the same bits."""
    V, U, N, G, cap = 1000, 65, 24, 5, 1
    news, user = _ints(V, U, N, seed=21)
    news_d, user_d = news.cuda(), user.cuda()
    group = _groups(V, G, True, seed=22)
    full, _ = metrics.rank_reference(news.numpy(), user.numpy(), targets=np.tile(np.arange(V), (U, 1)), group=group, group_cap=cap)
    tg = _target_sets(full, V, seed=23)[0]
    tg[3] = 0                                                                          # a user without a target
    for u in range(4, 8):                                                              # users whose every click is capped out
        out = np.flatnonzero(full[u] == -1)
        tg[u] = out[:4]
    ks = (1, 5, 10, 100)
    ref_r, _ = metrics.rank_reference(news.numpy(), user.numpy(), targets=tg, group=group, group_cap=cap)
    assert (ref_r[4:8] == -1).all() and (ref_r[3] == 0).all()
    want = metrics.retrieval_metrics_reference(ref_r, ks)[1]
    assert want[0] == U - 1
    got = []
    for splits in (0, 3, 0):
        r, s, sums = _rank(news_d, user_d, tg, splits=splits, group=group, group_cap=cap, n_groups=G, ks=ks)
        assert np.array_equal(r, ref_r)
        assert sums.shape == (2 + 2 * len(ks),) and sums[0] == U - 1 and np.allclose(sums, want, rtol=1e-9, atol=0), (splits, sums, want)
        got.append(sums)
    assert np.array_equal(got[0].view(np.int64), got[2].view(np.int64)) and np.array_equal(got[0].view(np.int64), got[1].view(np.int64))


def _corpus(n_news, seed):
    g = torch.Generator().manual_seed(seed)
    nc = torch.randint(1, 12, (n_news + 1, 4), generator=g, dtype=torch.int32)       # word ids of a 12-word vocabulary
    cut = torch.randint(1, 5, (n_news + 1,), generator=g)
    nc[torch.arange(4)[None, :] >= cut[:, None]] = 0                                  # titles of 1 .. 4 words
    nc[0] = 0
    return nc


def test_rank_eval_end_to_end():
    """The small NRMS model and corpus of test_gpu_groupcap.py::test_recommend_end_to_end, 6 categories, at most 2 per category:
    train.rank_eval_capped(news_group, group_cap) gives every click the place it has in train.recommend's capped row (same score
    bits), -1 to the eligible clicks that row never shows, 0 where the plain call gives 0; user 0 has 11 targets, more than one
    capped row holds."""
    model, z, cfg, sd = build_model("nrms_tiny_mask", "fp32")
    n_news, U, H, cap = 100, 40, cfg.user_log_length, 2
    V = n_news + 1
    nc = _corpus(n_news, seed=51)
    g = torch.Generator().manual_seed(52)
    hist = torch.randint(1, V, (U, H), generator=g, dtype=torch.int32)
    mask = torch.ones(U, H)
    for u in range(2, U):                                                    # front padded
        n_pad = int(torch.randint(0, H, (1,), generator=g))
        hist[u, :n_pad], mask[u, :n_pad] = 0, 0
    news_vecs = TR.encode_news(model, nc, 64, torch.device("cuda")).detach().float().contiguous()
    category = _groups(V, 6, True, seed=54).astype(np.int64)                  # a host array, as the pool arguments are
    T = 11
    targets = np.zeros((U, T), np.int32)
    rng = np.random.default_rng(55)
    targets[0] = rng.permutation(np.arange(1, V))[:T]
    targets[1:, :3] = rng.integers(1, V, (U - 1, 3))
    targets[5, 2], targets[6, 1] = targets[5, 0], int(hist[6, -1])           # a repeat, a clicked news
    ks = (5, 10, 100)
    row_ids, row_sc = (t.cpu().numpy() for t in TR.recommend(model, news_vecs, hist.numpy(), mask.numpy(), 128, news_group=category, group_cap=cap))
    plain = [t.cpu().numpy() for t in TR.rank_eval(model, news_vecs, hist.numpy(), mask.numpy(), targets, ks=ks)]
    ranks, scores, sums = (t.cpu().numpy() for t in TR.rank_eval_capped(model, news_vecs, hist.numpy(), mask.numpy(), targets, category, cap, ks=ks))
    assert ranks.shape == scores.shape == (U, T) and ranks.dtype == np.int32
    assert np.array_equal(ranks == 0, plain[0] == 0) and (ranks[6, 1] == 0) and (ranks[5, 2] == 0)
    assert (ranks == -1).any() and (ranks > 0).any() and (ranks[0] != 0).sum() > TC
    for u in range(U):
        for j in range(T):
            t, r = targets[u, j], ranks[u, j]
            if r > 0:
                assert row_ids[u, r - 1] == t and bits(row_sc[u, r - 1:r]) == bits(scores[u, j:j + 1]), (u, j)
                assert r <= plain[0][u, j]
            elif r == -1:
                assert t not in row_ids[u] and plain[0][u, j] > 0 and bits(scores[u, j:j + 1]) == bits(plain[1][u, j:j + 1]), (u, j)
            else:
                assert np.isneginf(scores[u, j])
    assert np.allclose(sums, metrics.retrieval_metrics_reference(ranks, ks)[1], rtol=1e-9, atol=0)
    again = [t.cpu().numpy() for t in TR.rank_eval(model, news_vecs, hist.numpy(), mask.numpy(), targets, ks=ks)]      # the plain call after it
    assert np.array_equal(again[0], plain[0]) and np.array_equal(bits(again[1]), bits(plain[1])) and np.array_equal(again[2], plain[2])
    with pytest.raises(RuntimeError, match="group_cap"):
        TR.rank_eval_capped(model, news_vecs, hist.numpy(), mask.numpy(), targets, category, None, ks=ks)
    with pytest.raises(RuntimeError, match="news_group is None"):
        TR.rank_eval_capped(model, news_vecs, hist.numpy(), mask.numpy(), targets, None, 2, ks=ks)
    with pytest.raises(RuntimeError, match="T = 5"):
        ops.score_rank_capped(news_vecs, news_vecs[:2].contiguous(), torch.ones(2, 5, dtype=torch.int32).cuda(), _dev(category, np.int32), 2)
