"""GPU: every cell of the launch tables of the full-corpus calls (csrc/nr_topk.hip, nr_rank.hip, nr_logz.hip) -- the run-time choice
(user tile, pools, list form, caps, blocks of 64 groups, sampled) reaches the instantiation it names.  One small case per cell:
U = 65 users (two user tiles at the widest tile), V = 300 (two full chunks and a tail of 43), splits = 2, T = 4, k = 8; N = 24 / 512 /
1024 give the user tiles 64 / 32 / 16 of every call.  (nr_mmr.hip's four instantiations are the pool widths of
test_gpu_mmr.test_exact_grid_against_the_reference.)

Vectors are integer valued and priors multiples of 1/4 (test_gpu_caprank._ints), so every fp32 sum is exact and ids, ranks, scores,
maxima and counts equal the host statements of metrics.py exactly; the log-sum and the row log-probabilities are held to the derived
bounds of test_gpu_logz.py.  The pool, list and cap inputs all change the answer, and the test says so by itself: the references
of the cells of one call are pairwise different, so a cell that launched without one of its flags fails.  The user tile is read
from the profiler label of the launch."""
import functools
import itertools

import numpy as np
import pytest
import torch

from newsrecommendation_amd import _lib, metrics, ops
from test_gpu_caprank import _dev, _ints, _rank, _topk
from test_gpu_logz import _logp_tolerance, logz_bound

pytestmark = pytest.mark.gpu

U, V, T, K, SPLITS = 65, 300, 4, 8, 2
TILE = {24: 64, 512: 32, 1024: 16}
CAPPED_TILE = {5: 64, 100: 64, 200: 32, 400: 16}            # one, two, four and eight blocks of 64 groups: the widest tile each allows
SEED, DRAW, TAU, TAU_Z = 0x5EED00012345678, 7, 0.75, 4.0
INF = float("inf")
LISTS = (None, "dense", "csr")


@functools.lru_cache(maxsize=None)
def _case(N):
    """The inputs of one N, made once and never written to."""
    news, user = _ints(V, U, N, seed=7000 + N)
    rng = np.random.default_rng(N)
    lo = rng.integers(0, 4, U)
    pools = dict(prior=(rng.integers(-32, 33, V) / 4.0).astype(np.float32), stamp=rng.integers(0, 10, V).astype(np.int32),
                 window=np.stack([lo, lo + rng.integers(3, 7, U)], axis=1).astype(np.int32))
    groups = {}
    for G in CAPPED_TILE:
        groups[G] = rng.integers(0, G, V).astype(np.int32)
        groups[G][::10] = -1
    return dict(N=N, news=news.numpy(), user=user.numpy(), news_d=news.cuda(), user_d=user.cuda(), pools=pools, groups=groups,
                targets=rng.integers(1, V, (U, T)).astype(np.int32), filler=[rng.choice(np.arange(1, V), 70, replace=False) for _ in range(U)])


def _lists(c, form, named):
    """The exclusion lists of a cell as (host statement, device argument): the ids `named` [U, n] -- the best of the cell without
    lists, a target -- as a dense [U, n + 1] tensor with a 0, or as CSR lists with 70 more ids each (a second chunk of the named pass)."""
    if form is None:
        return None, None
    if form == "dense":
        dense = np.concatenate([named, np.zeros((U, 1), dtype=named.dtype)], axis=1).astype(np.int32)
        return dense, _dev(dense)
    rows = [np.concatenate([named[u], c["filler"][u]]) for u in range(U)]
    return rows, ops.ExclusionLists([torch.from_numpy(r) for r in rows], device="cuda")


def _launched(fn):
    """fn() and the profiler labels of what it launched."""
    _lib.prof_enable(1)
    try:
        _lib.prof_collect()
        out = fn()
        torch.cuda.synchronize()
        return out, set(_lib.prof_collect().keys())
    finally:
        _lib.prof_enable(0)


def _all_differ(refs):
    """Every flag of every cell changes the answer: no two cells of the table share a reference."""
    for (a, x), (b, y) in itertools.combinations(refs.items(), 2):
        assert not all(np.array_equal(p, q, equal_nan=True) for p, q in zip(x, y)), (a, b)


def _noise(c):
    """fl32(TAU * g) [U, V], g read back through the probe: the noise the sampled selection adds, keys 0 .. U-1."""
    keys = torch.arange(U, dtype=torch.int32)[:, None].expand(U, V).contiguous().cuda()
    ids = torch.arange(V, dtype=torch.int32)[None, :].expand(U, V).contiguous().cuda()
    g, _ = ops.sample_noise(SEED, DRAW, keys, ids)
    return np.float32(TAU) * g.cpu().numpy()


@pytest.mark.parametrize("N", sorted(TILE))
def test_topk_and_sample_reach_every_instantiation(N):
    """pools x list form x caps x sampled.  The sampled cells are stated through the plain reference on the perturbed scores
    fl32(dot + fl32(prior + fl32(tau g))), formed on the host in fp32 from the probe's g: exact as well."""
    c = _case(N)
    dots = (c["user"].astype(np.float64) @ c["news"].T.astype(np.float64)).astype(np.float32)
    noise = _noise(c)
    refs = {}
    for pool, form, caps, sampled in itertools.product((False, True), LISTS, (False, True), (False, True)):
        pools = c["pools"] if pool else {}
        capped = dict(group=c["groups"][5], group_cap=1) if caps else {}
        if sampled:                                                   # the prior is inside the scores; stamps and windows stay
            scores = (dots + ((pools["prior"] if pool else np.float32(0)) + noise)).astype(np.float64)
            state = functools.partial(metrics.topk_reference, scores, k=K, **{n: v for n, v in pools.items() if n != "prior"}, **capped)
        else:
            state = functools.partial(metrics.topk_reference, c["news"], c["user"], k=K, **pools, **capped)
        best = state()[0]
        assert (best[:, :2] > 0).all()
        host, dev = _lists(c, form, best[:, :2])
        ref_ids, ref_sc = state(exclude=host)
        ref_sc = ref_sc.astype(np.float32)
        where = (N, pool, form, caps, sampled)
        if sampled:
            (ids, sc, model), labels = _launched(lambda: ops.score_sample(c["news_d"], c["user_d"], K, TAU, SEED, draw=DRAW, exclude=dev, splits=SPLITS,
                                                                          group=_dev(capped.get("group")), group_cap=capped.get("group_cap"),
                                                                          **{n: _dev(v) for n, v in pools.items()}))
            ids, sc, model = ids.cpu().numpy(), sc.cpu().numpy(), model.cpu().numpy()
            want = np.where(ref_ids > 0, ref_sc - np.take_along_axis(noise, ref_ids.astype(np.int64), axis=1), np.float32(-INF))
            assert np.array_equal(model, want), where
            assert any(l.startswith("sample_model[") for l in labels), labels
        else:
            (ids, sc), labels = _launched(lambda: _topk(c["news_d"], c["user_d"], K, exclude=dev, splits=SPLITS, **capped, **pools))
        assert np.array_equal(ids, ref_ids), (where, np.argwhere(ids != ref_ids)[:5])
        assert np.array_equal(sc, ref_sc), where
        assert f"topk_select[U={U},V={V},N={N},k={K},TU={TILE[N]},splits={SPLITS}]" in labels, labels
        refs[where] = (ref_ids, ref_sc)
    assert len(refs) == 24
    _all_differ(refs)


@pytest.mark.parametrize("N", sorted(TILE))
def test_rank_reaches_every_instantiation(N):
    """pools x list form without caps and with G = 5; pools x G in {5, 100, 200, 400} without lists: both named passes in all their
    instantiations, the counting pass in every (tile, pool, blocks of groups) it exists for.  The lists name the two best news of
    the cell without lists (they beat every target) and the last target (rank 0)."""
    c = _case(N)
    tg = c["targets"]
    every = np.tile(np.arange(V), (U, 1))
    cells = [(pool, form, G) for pool in (False, True) for form in LISTS for G in (0, 5)]
    cells += [(pool, None, G) for pool in (False, True) for G in (100, 200, 400)]
    refs = {}
    for pool, form, G in cells:
        pools = c["pools"] if pool else {}
        capped = dict(group=c["groups"][G], group_cap=1) if G else {}
        full, _ = metrics.rank_reference(c["news"], c["user"], targets=every, **pools, **capped)
        best = np.stack([np.argsort(np.where(full > 0, full, V + 1), axis=1, kind="stable")[:, j] for j in range(2)], axis=1)
        assert (np.take_along_axis(full, best, axis=1) == [1, 2]).all()
        host, dev = _lists(c, form, np.concatenate([best, tg[:, 3:]], axis=1))
        ref_r, ref_s = metrics.rank_reference(c["news"], c["user"], targets=tg, exclude=host, **pools, **capped)
        where = (N, pool, form, G)
        (r, s), labels = _launched(lambda: _rank(c["news_d"], c["user_d"], tg, exclude=dev, splits=SPLITS, n_groups=G or None, **capped, **pools))
        assert np.array_equal(r, ref_r), (where, np.argwhere(r != ref_r)[:5])
        assert np.array_equal(s, ref_s.astype(np.float32)), where
        if form is not None:
            assert (ref_r[:, 3] == 0).all()
        tile = min(TILE[N], CAPPED_TILE[G]) if G else TILE[N]
        assert f"rank_count[U={U},V={V},N={N},T={T},TU={tile},splits={SPLITS}]" in labels, labels
        assert any(l.startswith("rank_named_csr[" if form == "csr" else "rank_named[") for l in labels), labels
        assert any(l.startswith("rank_group_masks[") for l in labels) == bool(G), labels
        refs[where] = (ref_r, ref_s)
    assert len(refs) == 18
    _all_differ(refs)


@pytest.mark.parametrize("N", sorted(TILE))
def test_logz_and_row_logprob_reach_every_instantiation(N):
    """nr_score_logz: pools x lists (CSR, the only form it knows): maximum and count exact, the log-sum within logz_bound.
    nr_row_logprob: pools, on the 8 best of the cell with a fill entry, against the host base."""
    c = _case(N)
    refs = {}
    for pool, form in itertools.product((False, True), (None, "csr")):
        pools = c["pools"] if pool else {}
        best = metrics.topk_reference(c["news"], c["user"], k=2, **pools)[0]
        host, dev = _lists(c, form, best)
        want = metrics.logz_reference(c["news"], c["user"], temperature=TAU_Z, exclude=host, **pools)
        got, labels = _launched(lambda: ops.score_logz(c["news_d"], c["user_d"], TAU_Z, exclude=dev, splits=SPLITS, **{n: _dev(v) for n, v in pools.items()}))
        logsum, smax, count = (x.cpu().numpy() for x in got)
        where = (N, pool, form)
        assert np.array_equal(count, want[2]) and np.array_equal(smax.astype(np.float64), want[1]), where
        assert (count > 0).all()
        assert all(abs(float(logsum[u]) - want[0][u]) <= logz_bound(count[u], V) for u in range(U)), where
        assert f"logz_stream[U={U},V={V},N={N},TU={TILE[N]},splits={SPLITS},seg=128]" in labels, labels
        refs[where] = (want[1], want[2])
    _all_differ(refs)
    rows = {}
    for pool in (False, True):
        pools = c["pools"] if pool else {}
        ids = metrics.topk_reference(c["news"], c["user"], k=K, **pools)[0]
        ids[:, 3] = 0
        base = metrics.logz_reference(c["news"], c["user"], temperature=TAU_Z, exclude=ids, **pools)
        base = (base[0].astype(np.float32), base[1].astype(np.float32))
        ref, ref_total = metrics.row_logprob_reference(c["news"], c["user"], row_ids=ids, temperature=TAU_Z, base=base, sequential=True, **pools)
        (lp, total), labels = _launched(lambda: ops.row_logprob(c["news_d"], c["user_d"], _dev(ids, np.int32), TAU_Z, (_dev(base[0]), _dev(base[1])), True,
                                                                **{n: _dev(v) for n, v in pools.items()}))
        lp, total = lp.cpu().numpy().astype(np.float64), total.cpu().numpy().astype(np.float64)
        assert np.isfinite(ref).all() and (ref[:, 3] == 0).all() and (lp[:, 3] == 0).all()
        assert (np.abs(lp - ref) <= _logp_tolerance(ref)).all(), (N, pool, np.abs(lp - ref).max())
        assert (np.abs(total - ref_total) <= _logp_tolerance(ref_total)).all(), (N, pool)
        assert f"logp_rows[U={U},N={N},k={K},seq=1]" in labels, labels
        rows[pool] = (ids, ref)
    _all_differ(rows)
