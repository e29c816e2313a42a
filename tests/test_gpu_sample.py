"""GPU: sampled full-corpus recommendation (nr_score_sample / ops.score_sample / train.recommend_sample; include/nrhip.h, K12).
The core statement is differential: row u of a sampled call is row 0 of ops.score_topk for user u alone with the prior
P(u, .) = prior + tau_u * g, g read back through the probe -- ids equal, score bits equal -- at shapes that cross every boundary
of the selection kernel (a chunk tail, several slices, k = 1 / 10 / 128, pools, caps, CSR lists).  Around it: the probe against
the integer-exact host Philox and the fp64 Gumbel, independence of splits / user order / repetition, temperature 0, bad
per-user temperatures, the Plackett-Luce law end to end, and train.recommend_sample."""
import numpy as np
import pytest
import torch

from helpers import build_model
from newsrecommendation_amd import metrics, ops, train as TR
from sample_helpers import (CHI2_FIRST_MAX, CHI2_SECOND_MAX, LAW_DRAW, LAW_SEED, LAW_TAU, LAW_U, LAW_X, law_chi2, law_scores)

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
SEED, DRAW = 0x5EED00012345678, 7          # a seed with a non-zero high word
U, V = 37, 1000                            # 999 real news: chunks of 128 leave a tail of 103; splits = 3 slices of 333

# |g - g64| <= G_C * 2^-23 * max(1, |g64|).  g = -log(t), t = -log(u) with u (or 1 - u) exact in fp32, so the only errors are the
# two library logarithms': at most 3 ulp for logf and 2 ulp for log1pf (the bounds the device library is built to, OpenCL full
# profile), a relative error of t of at most 3 * 2^-23, which is an absolute error of g of the same size, plus 3 ulp(g) <=
# 3 * 2^-23 |g| of the outer logf: 6 * 2^-23 * max(1, |g|), and 7 with the second-order terms.  Measured worst case: see DESIGN.md 5.
G_C = 7.0


def _keys(dev):
    g = torch.Generator().manual_seed(7)
    return (torch.randperm(U, generator=g) + 1000).to(torch.int32).to(dev)


def _vectors(N, dev, seed=11):
    g = torch.Generator().manual_seed(seed)
    news = torch.randn(V, N, generator=g)
    user = torch.randn(U, N, generator=g) / N ** 0.5              # scores of about unit spread
    return news.to(dev), user.to(dev)


def _tau(dev):
    g = torch.Generator().manual_seed(13)
    tau = 0.05 + torch.rand(U, generator=g)
    tau[0], tau[1], tau[2] = 0.0, 5.0, 0.01                         # the plain row; several times the spread; a hair
    return tau.to(dev)


def _pools(dev):
    g = torch.Generator().manual_seed(17)
    prior = 0.3 * torch.randn(V, generator=g)
    prior[17], prior[640] = -INF, NAN
    stamp = torch.randint(0, 100, (V,), generator=g, dtype=torch.int32)
    lo = torch.randint(0, 30, (U,), generator=g, dtype=torch.int32)
    window = torch.stack([lo, lo + torch.randint(20, 70, (U,), generator=g, dtype=torch.int32)], dim=1)
    window[5] = torch.tensor([60, 40])                              # an empty window: an all-fill row
    window[6] = torch.tensor([0, 99])                               # everything
    return dict(prior=prior.to(dev), stamp=stamp.to(dev), window=window.to(dev))


def _noise(keys, dev):
    """g [U, V] fp32 through the probe: the noise the selection adds, for every (user, news) of the test."""
    a = keys[:, None].expand(U, V).contiguous()
    v = torch.arange(V, dtype=torch.int32, device=dev)[None, :].expand(U, V).contiguous()
    g, _ = ops.sample_noise(SEED, DRAW, a, v)
    return g


def test_noise_probe_bits_exact_and_gumbel_within_the_derived_bound():
    dev = torch.device("cuda")
    big = 100001
    rng = np.random.default_rng(5)
    v = np.concatenate([[1, 2, 3, 4, 5, 6, 7, 8, big - 1, big - 2, big - 3, big - 4], rng.integers(1, big, 2048 - 12)])
    a = np.concatenate([[0, 1, 2 ** 31 - 1] * 4, rng.choice([0, 1, 2 ** 31 - 1, 12345], 2048 - 12)])
    a[12:24], v[12:24] = [0] * 4 + [1] * 4 + [2 ** 31 - 1] * 4, [1, 2, 3, 4, 5, big - 1] * 2          # every listed key with listed ids
    assert set(v & 3) == {0, 1, 2, 3}
    worst = 0.0
    for draw in (0, 7):                                             # 2 x 2048 = 4096 pairs
        g, bits = ops.sample_noise(SEED, draw, torch.tensor(a, dtype=torch.int32, device=dev), torch.tensor(v, dtype=torch.int32, device=dev))
        g64, want = metrics.sample_noise_reference(SEED, draw, a, v)
        assert np.array_equal(bits.cpu().numpy().astype(np.uint32), want)
        g = g.cpu().numpy()
        assert g.dtype == np.float32 and np.all(np.isfinite(g))
        err = np.abs(g.astype(np.float64) - g64) / np.maximum(1.0, np.abs(g64)) * 2.0 ** 23
        worst = max(worst, float(err.max()))
    print(f"worst |g - g64| / (2^-23 max(1, |g64|)) = {worst:.3f} (bound {G_C})")
    assert worst <= G_C
    # either output may be left out; a draw is a function of the pair, not of its place in the call
    g2, bits2 = ops.sample_noise(SEED, 7, torch.tensor(a[::-1].copy(), dtype=torch.int32, device=dev), torch.tensor(v[::-1].copy(), dtype=torch.int32, device=dev))
    assert np.array_equal(g2.cpu().numpy()[::-1], g) and np.array_equal(bits2.cpu().numpy()[::-1], bits.cpu().numpy())


@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("N", [400, 36])
def test_row_u_is_the_plain_row_of_user_u_with_the_perturbed_prior(N, k):
    dev = torch.device("cuda")
    news, user = _vectors(N, dev)
    keys, tau, pools = _keys(dev), _tau(dev), _pools(dev)
    g = _noise(keys, dev)
    gen = torch.Generator().manual_seed(19)
    group = torch.randint(-1, 12, (V,), generator=gen, dtype=torch.int32).to(dev)
    lists = ops.ExclusionLists([torch.randperm(V - 1, generator=gen)[:int(n)] + 1 for n in torch.randint(200, 500, (U,), generator=gen)], device=dev)
    variants = [dict(), dict(group=group, group_cap=2), dict(exclude=lists), dict(group=group, group_cap=2, exclude=lists)]
    differ = 0
    for extra in variants:
        ids, pert, model = ops.score_sample(news, user, k, tau, SEED, draw=DRAW, user_keys=keys, splits=3, **pools, **extra)
        plain_ids, _ = ops.score_topk(news, user, k, splits=3, **pools, **extra)
        differ += int((ids != plain_ids).any(dim=1).sum())
        assert torch.equal(ids[0], plain_ids[0])                                       # tau_u = 0
        assert (ids[5] == 0).all() and (pert[5] == -INF).all() and (model[5] == -INF).all()   # the empty window
        for u in range(U):
            p_u = pools["prior"] + tau[u] * g[u]                                        # fp32: one multiply, one add
            one = dict(extra)
            if "exclude" in one:
                one["exclude"] = lists.take([u])
            want_ids, want_sc = ops.score_topk(news, user[u:u + 1], k, splits=3, prior=p_u, stamp=pools["stamp"], window=pools["window"][u:u + 1], **one)
            assert torch.equal(ids[u], want_ids[0]), (u, extra.keys())
            assert torch.equal(pert[u].view(torch.int32), want_sc[0].view(torch.int32)), (u, extra.keys())
        assert not (ids == 17).any() and not (ids == 640).any()                         # prior -inf, prior NaN
    assert differ > 2 * U                                                               # the noise did change rows


def test_model_scores_are_the_plain_scores_to_two_roundings():
    """Without a prior P = fl(tau g) exactly, perturbed = fl(x + P) and model = fl(perturbed - P) with x the plain score: two
    roundings of half an ulp each, of numbers no larger than max(|perturbed|, |x|).  V - 1 = 128 news, so score_topk(k = 128)
    gives x for every id; 8 excluded ids per user leave 8 places of fill."""
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(23)
    Vs, N = 129, 36
    news, user = torch.randn(Vs, N, generator=g).to(dev), (torch.randn(U, N, generator=g) / 6.0).to(dev)
    exclude = torch.stack([torch.randperm(Vs - 1, generator=g)[:8] + 1 for _ in range(U)]).to(torch.int32).to(dev)
    all_ids, all_x = ops.score_topk(news, user, 128)
    x = torch.zeros(U, Vs, device=dev).scatter_(1, all_ids.long(), all_x)
    for tau in (0.3, _tau(dev)):
        ids, pert, model = ops.score_sample(news, user, 128, tau, SEED, user_keys=_keys(dev), exclude=exclude, splits=2)
        live = ids > 0
        assert int(live.sum()) == U * 120 and (model[~live] == -INF).all() and (pert[~live] == -INF).all() and not live[:, 120:].any()
        want = x.gather(1, ids.long())
        big = torch.maximum(pert.abs(), want.abs()).cpu().numpy().astype(np.float32)
        err = (model.double() - want.double()).abs().cpu().numpy()
        ok = live.cpu().numpy()
        worst = float((err[ok] / np.spacing(big[ok]).astype(np.float64)).max())
        print(f"worst |model - x| = {worst:.3f} ulp(max(|perturbed|, |x|))")
        assert worst <= 1.0
        for u in range(U):
            assert not set(ids[u, :120].tolist()) & set(exclude[u].tolist())


def test_rows_do_not_depend_on_splits_user_order_or_repetition():
    dev = torch.device("cuda")
    news, user = _vectors(36, dev)
    keys, tau, pools = _keys(dev), _tau(dev), _pools(dev)
    kw = dict(draw=DRAW, **pools)
    base = ops.score_sample(news, user, 10, tau, SEED, user_keys=keys, splits=3, **kw)
    for splits in (1, 7, 3, 0):                                     # 3 again: the same call twice
        again = ops.score_sample(news, user, 10, tau, SEED, user_keys=keys, splits=splits, **kw)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(base, again)), splits
    rev = ops.score_sample(news, user.flip(0).contiguous(), 10, tau.flip(0), SEED, user_keys=keys.flip(0), splits=3, draw=DRAW,
                           prior=pools["prior"], stamp=pools["stamp"], window=pools["window"].flip(0).contiguous())
    assert all(torch.equal(x.view(torch.int32), y.flip(0).view(torch.int32)) for x, y in zip(base, rev))
    none = ops.score_sample(news, user, 10, tau, SEED, splits=3, **kw)
    arange = ops.score_sample(news, user, 10, tau, SEED, user_keys=torch.arange(U, device=dev), splits=3, **kw)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(none, arange))
    assert not torch.equal(none[0], base[0])                        # other keys, other rows
    other = ops.score_sample(news, user, 10, tau, SEED, user_keys=keys, splits=3, draw=DRAW + 1, **pools)
    assert not torch.equal(other[0], base[0])


def test_temperature_zero_is_score_topk_bit_for_bit():
    dev = torch.device("cuda")
    news, user = _vectors(400, dev)
    pools = _pools(dev)
    gen = torch.Generator().manual_seed(29)
    group = torch.randint(-1, 12, (V,), generator=gen, dtype=torch.int32).to(dev)
    lists = ops.ExclusionLists([torch.randperm(V - 1, generator=gen)[:300] + 1 for _ in range(U)], device=dev)
    dense = torch.randint(0, V, (U, 16), generator=gen, dtype=torch.int32).to(dev)
    for extra in (dict(), pools, dict(group=group, group_cap=2, **pools), dict(exclude=lists, **pools), dict(exclude=dense),
                  dict(group=group, group_cap=2, exclude=lists)):
        for k in (10, 128):
            want_ids, want_sc = ops.score_topk(news, user, k, splits=3, **extra)
            for tau in (0.0, torch.zeros(U, device=dev)):
                ids, pert, model = ops.score_sample(news, user, k, tau, SEED, draw=DRAW, splits=3, **extra)
                assert torch.equal(ids, want_ids) and torch.equal(pert.view(torch.int32), want_sc.view(torch.int32))
                assert torch.equal(model.view(torch.int32), want_sc.view(torch.int32))


def test_bad_per_user_temperatures_give_all_fill_rows_and_leave_the_neighbours_alone():
    dev = torch.device("cuda")
    news, user = _vectors(36, dev)
    keys, tau = _keys(dev), _tau(dev)
    good = ops.score_sample(news, user, 10, tau, SEED, user_keys=keys, splits=3)
    bad_tau = tau.clone()
    bad_at = [3, 20, 36]
    bad_tau[3], bad_tau[20], bad_tau[36] = -1.0, NAN, INF
    ids, pert, model = ops.score_sample(news, user, 10, bad_tau, SEED, user_keys=keys, splits=3)
    keep = torch.ones(U, dtype=torch.bool, device=dev)
    keep[bad_at] = False
    assert (ids[bad_at] == 0).all() and (pert[bad_at] == -INF).all() and (model[bad_at] == -INF).all()
    assert torch.equal(ids[keep], good[0][keep]) and torch.equal(pert[keep], good[1][keep]) and torch.equal(model[keep], good[2][keep])
    assert (good[0] > 0).all()
    for scalar in (-1.0, NAN, INF):
        with pytest.raises(RuntimeError, match="tau"):
            ops.score_sample(news, user, 10, scalar, SEED)


def test_the_law_end_to_end():
    """The configuration of tests/test_sample_host.py through the kernel: news_vecs[v] = (x_v, 0, 0, 0), every user (1, 0, 0, 0)."""
    dev = torch.device("cuda")
    news = torch.zeros(9, 4)
    news[1:, 0] = torch.tensor(LAW_X, dtype=torch.float32)
    user = torch.zeros(LAW_U, 4)
    user[:, 0] = 1.0
    ids, pert, model = ops.score_sample(news.to(dev), user.to(dev), 2, LAW_TAU, LAW_SEED, draw=LAW_DRAW, user_keys=torch.arange(LAW_U, device=dev))
    chi1, chi2, n = law_chi2(ids.cpu().numpy())
    ref_ids, _, _ = metrics.sample_reference(law_scores(), k=2, temperature=LAW_TAU, seed=LAW_SEED, draw=LAW_DRAW, user_keys=np.arange(LAW_U))
    same = float(np.mean(ids.cpu().numpy()[:, 0] == ref_ids[:, 0]))
    print(f"chi2 first place {chi1:.2f}, second place {chi2:.2f} over {n} users; first places equal to the reference's: {same:.4f}")
    assert chi1 <= CHI2_FIRST_MAX and chi2 <= CHI2_SECOND_MAX
    assert same >= 0.99


def test_recommend_sample_on_the_tiny_model():
    tag = "nrms_tiny_mask"
    model, z, cfg, sd = build_model(tag, "fp32")
    n_news, Ur, H, k = 300, 40, cfg.user_log_length, 10
    g = torch.Generator().manual_seed(51)
    nc = torch.randint(1, 12, (n_news + 1, 4), generator=g, dtype=torch.int32)           # titles of 1 .. 4 words, 12-word vocabulary
    nc[torch.arange(4)[None, :] >= torch.randint(1, 5, (n_news + 1,), generator=g)[:, None]] = 0
    nc[0] = 0
    hist = torch.randint(1, n_news + 1, (Ur, H), generator=g, dtype=torch.int32)
    mask = torch.ones(Ur, H)
    for u in range(Ur):
        n_pad = 0 if u == 1 else H if u == 0 else int(torch.randint(0, H, (1,), generator=g))
        hist[u, :n_pad], mask[u, :n_pad] = 0, 0
    dev = torch.device("cuda")
    news_vecs = TR.encode_news(model, nc, 64, dev)
    keys = torch.arange(Ur) + 77
    ids, ms = TR.recommend_sample(model, news_vecs, hist.numpy(), mask.numpy(), k, 0.5, seed=SEED, draw=2, user_keys=keys)
    table, user, exclude, kw, caps = TR._recommend_args(model, news_vecs, hist.numpy(), mask.numpy(), True, 8192, None, None, None, None, None, None)
    want_ids, _, want_ms = ops.score_sample(table, user, k, 0.5, SEED, draw=2, user_keys=keys.to(dev), exclude=exclude)
    assert torch.equal(ids, want_ids) and torch.equal(ms.view(torch.int32), want_ms.view(torch.int32)) and (ids > 0).all()
    clicked = [set(hist[u][mask[u] != 0].tolist()) for u in range(Ur)]
    assert sum(len(clicked[u] & set(ids[u].tolist())) for u in range(Ur)) == 0
    loose, _ = TR.recommend_sample(model, news_vecs, hist.numpy(), mask.numpy(), k, 0.5, seed=SEED, draw=2, user_keys=keys, exclude_history=False)
    assert not torch.equal(loose, ids)
    for tau in (0.0, torch.zeros(Ur)):
        ids0, ms0 = TR.recommend_sample(model, news_vecs, hist.numpy(), mask.numpy(), k, tau, seed=SEED)
        rec_ids, rec_sc = TR.recommend(model, news_vecs, hist.numpy(), mask.numpy(), k)
        assert torch.equal(ids0, rec_ids) and torch.equal(ms0.view(torch.int32), rec_sc.view(torch.int32))
