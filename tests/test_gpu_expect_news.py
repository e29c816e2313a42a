"""GPU: the news side of the full-softmax gradient (nr_score_expect_news; ops.score_expect_news / ops.full_softmax_nll_joint /
ops.news_gather; train.full_softmax_loss_joint / train.expected_exposure; include/nrhip.h, K18).  The device is held to a bound
DERIVED from its order of operations (kappa, below) against metrics.expect_news_reference in float64 on the fp32 inputs; bit
statements where the contract makes them (fixed splits: a row does not depend on the other news rows or on its place; the
mass-only mode has the rows mode's mass; the forward and grad_user are full_softmax_nll's)."""
import math

import numpy as np
import pytest
import torch

from helpers import assert_close, build_model
from newsrecommendation_amd import _lib, metrics, ops, train as TR
from oracle import nr_oracle as O

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
EPS = 2.0 ** -24                           # half an ulp of fp32, relative
U_TWO = 128 * 256 + 5                      # the smallest U at which a user segment has two chunks (129 segments of 256 users)
DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _plan(U, splits):
    """Chunks of the longest user slice of the library's plan; splits = 0 (the library chooses) is bounded by one slice."""
    seg = 128 * math.ceil(U / (128 * 256))
    nseg = math.ceil(U / seg)
    segs_per = math.ceil(nseg / min(splits, nseg)) if splits > 0 else nseg
    return segs_per * (seg // 128)


def kappas(N, V, U, splits, n, C, G):
    """(kappa of the rows, kappa of the mass).  |out_vc - out*_vc| <= kappa e A_vc, A_vc = sum_u |c_u| p*_uv |user_uc| + sum_j |d_j| |user_jc|,
    e = 2^-24; out*, p* exact on the fp32 inputs; n, C, G the maxima over the call's live users of K17's quantities (n eligible news,
    C = max |s| / tau, G = max (sum_c |user_c news_vc| + |prior_v|) / tau).  Per term c_u p_uv user_uc, first order in e:
      score chain   the device score is N fma roundings and the prior's add: (N + 1) G e in the exponent, in the numerator and in
                    the user's partition sum: 2 (N + 1) G e relative.
      exponent      fl(s - max) (e), fl(1 / tau) (e), each on |s - max| / tau <= 2 C; the fma's rounding (e) on |argument| <= 2 C + ln n:
                    (6 C + ln n) e; the base's logsum enters the exponent with its own bound (4 ln n + 7 K + 14) e, K = 2 seg_V / 128
                    ("The derived error bound of out_logsum").
      expf          <= 3 ulp = 6 e.
      coefficient   fl(1 / tau), fl(weight * that), fl(c * p): 3 e.
      contraction   every product enters ONE fp32 fma chain of at most L = 128 * (chunks of the longest user slice) steps: L e; the row
                    parts' adds: 3 e; the fp64 merge, the named terms' fl(1 / tau) and the single rounding to fp32: e each on what was added.
      + 2 e for the second-order terms.  Sum: 2 (N + 1) G + 6 C + 5 ln n + 7 K + L + 29.
    The mass is the row bound without the score-chain and accumulation terms (exact fp64 products weight * p, fp64 sums)."""
    seg_v = 128 * math.ceil((V - 1) / (128 * 256))
    common = 6.0 * C + 5.0 * math.log(max(n, 2)) + 7.0 * (2 * seg_v // 128) + 29.0
    return 2.0 * (N + 1) * G + 128.0 * _plan(U, splits) + common, common


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _reference(news, user, tau, hkw, weight=None, named=None, scale=False, dead=()):
    """(out*, A, mass*, M, n, C, G) in float64 on the fp32 inputs.  `dead`: users the reference is told to leave out (a NaN base is the
    device's knowledge, not the reference's): their temperature becomes 0."""
    a, b = news.double().cpu().numpy(), user.double().cpu().numpy()
    U, V = b.shape[0], a.shape[0]
    taus = np.array(metrics._temperatures(_host(tau), U)[0], dtype=np.float64)
    taus[list(dead)] = 0.0
    w = np.ones(U) if weight is None else _host(weight).astype(np.float64)
    nm = None if named is None else tuple(_host(x) for x in named)
    out, mass = metrics.expect_news_reference(a, b, temperature=taus, weight=w, named=nm, scale_inv_tau=scale, **hkw)
    p, live = metrics.softmax_matrix_reference(a, b, temperature=taus, **hkw)
    with np.errstate(divide="ignore", invalid="ignore"):
        it = np.where(live, 1.0 / taus, 0.0)
    c = np.where(live, np.abs(w), 0.0) * (it if scale else 1.0)
    babs = np.abs(np.where(np.isfinite(b), b, 0.0))
    A = p.T @ (c[:, None] * babs)
    if nm is not None:
        off, nu, nw = nm
        news_of = np.repeat(np.arange(V), np.diff(off))
        d = np.abs(nw.astype(np.float64)) * (it[nu] if scale else live[nu].astype(np.float64))
        np.add.at(A, news_of, d[:, None] * babs[nu])
    M = p.T @ np.where(live, np.abs(w), 0.0)
    # weights (and products c * p) below the normal range are lost at no more than 2^-126 each
    A = A + U * 2.0 ** -126 * max(float(c.max()), 1.0) * float(babs.max())
    M = M + U * 2.0 ** -126 * max(float(np.abs(w).max()), 1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        prior = hkw.get("prior")
        s = b @ a.T + (0.0 if prior is None else np.asarray(prior, dtype=np.float64)[None, :])
        mag = np.abs(b) @ np.abs(a).T + (0.0 if prior is None else np.abs(np.asarray(prior, dtype=np.float64))[None, :])
    ok = p > 0
    n = int(ok.sum(axis=1).max()) if U else 0
    with np.errstate(divide="ignore", invalid="ignore"):
        C = float(np.where(ok, np.abs(s) * it[:, None], 0.0).max())
        G = float(np.where(ok, mag * it[:, None], 0.0).max())
    return out, A, mass, M, n, C, G


def _check(news, user, tau, hkw, got, splits, note="", **ref_kw):
    """rows (None in the mass-only mode) and mass of `got` against the reference within the derived bounds; returns the worst ratios."""
    out_d, mass_d = got
    N, V, U = news.shape[1], news.shape[0], user.shape[0]
    out, A, mass, M, n, C, G = _reference(news, user, tau, hkw, **ref_kw)
    kr, km = kappas(N, V, U, splits, n, C, G)
    m = mass_d.double().cpu().numpy()
    assert np.isfinite(m).all(), note
    mratio = float((np.abs(m - mass) / (km * EPS * M)).max())
    ratio = 0.0
    if out_d is not None:
        o = out_d.double().cpu().numpy()
        assert np.isfinite(o).all(), note
        ratio = float((np.abs(o - out) / (kr * EPS * A)).max())
    print(f"expect_news {note}: N={N} V={V} U={U} splits={splits} worst |err| / bound = {ratio:.4f}, mass {mratio:.4f}")
    assert ratio <= 1.0, (note, ratio)
    assert mratio <= 1.0, (note, mratio)
    return ratio, mratio


def _vectors(N, V, U, seed=11):
    g = torch.Generator().manual_seed(seed)
    news = torch.randn(V, N, generator=g)
    user = torch.randn(U, N, generator=g) / N ** 0.5                  # scores of about unit spread
    return news.to(DEV), user.to(DEV)


def _pools(V, U, seed=17):
    g = torch.Generator().manual_seed(seed)
    prior = 0.3 * torch.randn(V, generator=g)
    prior[min(17, V - 1)] = -INF
    if V > 4:
        prior[V // 2] = NAN
    prior[torch.rand(V, generator=g) < 0.1] = -INF
    stamp = torch.randint(0, 100, (V,), generator=g, dtype=torch.int32)
    lo = torch.randint(0, 30, (U,), generator=g, dtype=torch.int32)
    window = torch.stack([lo, lo + torch.randint(20, 70, (U,), generator=g, dtype=torch.int32)], dim=1)
    window[min(5, U - 1)] = torch.tensor([60, 40])                    # lo > hi: nobody -- a user with nothing eligible
    window[0] = torch.tensor([0, 99])
    return dict(prior=prior.to(DEV), stamp=stamp.to(DEV), window=window.to(DEV))


def _list_tensor(V, U, seed=19, E=24):
    """[U, E] ids per user (0 = no entry, ids >= V mean nothing): user 0 the first and the last id, user 1 nothing, user 2 (where
    there is one) every id up to E."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, V + 2, (U, E), generator=g, dtype=torch.int32)
    t[torch.rand(U, E, generator=g) < 0.3] = 0
    t[0] = 0
    t[0, :2] = torch.tensor([1, V - 1])
    if U > 1:
        t[1] = 0
    if U > 2:
        t[2] = torch.arange(1, E + 1) % V
    return t


def _expect_news(news, user, tau, splits=0, rows=True, named=None, scale=False, weight=None, base=None, **kw):
    base = ops.score_logz(news, user, tau, **kw) if base is None else base
    return ops._score_expect_news("score_expect_news", news, user, tau, base, kw.get("exclude"), splits, kw.get("prior"), kw.get("stamp"),
                                  kw.get("window"), weight, named, scale, rows)


def _named(V, U, T, seed, every=None):
    """Named terms from targets [U, T] with repeats, fill ids and (every) one news named by every user."""
    g = torch.Generator().manual_seed(seed)
    targets = torch.randint(1, V, (U, T), generator=g, dtype=torch.int32)
    if T > 1:
        targets[::3, 1] = 0                                           # fill
        targets[1::4, T - 1] = V + 2                                  # fill: out of range
        targets[:, 1 % T] = torch.where(torch.arange(U) % 5 == 1, targets[:, 0], targets[:, 1 % T])     # a repeat: two entries
    if every is not None:
        targets[:, 0] = every
    gw = torch.randn(U, T, generator=g)
    gw[torch.rand(U, T, generator=g) < 0.1] = 0.0                     # dropped
    return targets.to(DEV), gw.to(DEV)


# N: one k-slab, npad > N, MIND's width (news tiles of 64, 64, 32), and 836 for the tile of 16; V: the tile boundaries + 2 (row 0 is
# in the first tile), a partial last tile; U: a single user, a partial last chunk, several slices, two chunks a segment
SHAPES = [(4, 2, 1, 0), (4, 66, 129, 1), (4, 130, 294, 3), (4, 70, U_TWO, 2), (36, 129, 33, 0), (36, 294, 300, 2), (400, 34, 129, 1),
          (400, 294, 70, 0), (836, 18, 130, 2), (836, 294, 17, 1)]


@pytest.mark.parametrize("N,V,U,splits", SHAPES, ids=lambda v: str(v))
def test_rows_and_mass_within_the_derived_bound(N, V, U, splits):
    news, user = _vectors(N, V, U)
    got = _expect_news(news, user, 0.5, splits=splits)
    _check(news, user, 0.5, {}, got, splits, note="plain")
    assert not got[0][0].any() and float(got[1][0]) == 0.0
    only = _expect_news(news, user, 0.5, splits=splits, rows=False)
    assert only[0] is None and torch.equal(_bits(only[1]), _bits(got[1]))
    # everything at once: pools, lists through by_news, a NaN news row, a user with an infinite component, per-user temperatures,
    # weights of both signs, named terms (repeats, fill ids, one news named by every user)
    g = torch.Generator().manual_seed(101 + N + V)
    news, user = _vectors(N, V, U, seed=23)
    if V > 4:
        news[V // 3, N // 2] = NAN
    if U > 8:
        user[7, N - 1] = INF
    tau = (0.3 + torch.rand(U, generator=g)).to(DEV)
    w = torch.randn(U, generator=g).to(DEV)
    pools = _pools(V, U)
    lt = _list_tensor(V, U)
    lists = ops.ExclusionLists(lt, device=DEV)
    T = 3
    targets, gw = _named(V, U, T, seed=7 + V, every=V - 1)
    named = ops._named_by_news(targets, gw, V)
    hkw = dict({k: v.cpu().numpy() for k, v in pools.items()}, exclude=list(lt.numpy()))
    got = _expect_news(news, user, tau, splits=splits, named=named, scale=True, weight=w, exclude=lists, **pools)
    _check(news, user, tau, hkw, got, splits, note="pools+lists+named", weight=w, named=named, scale=True)
    only = _expect_news(news, user, tau, splits=splits, rows=False, weight=w, exclude=lists, **pools)
    assert torch.equal(_bits(only[1]), _bits(got[1]))
    # lists alone and pools alone, without the 1 / tau scale
    for note, kw, h in (("lists", dict(exclude=lists), dict(exclude=hkw["exclude"])), ("pools", pools, {k: v for k, v in hkw.items() if k != "exclude"})):
        if U > 1000:                                                  # the host reference walks the users one by one
            break
        _check(news, user, tau, h, _expect_news(news, user, tau, splits=splits, weight=w, **kw), splits, note=note, weight=w)


def test_eligibility_is_the_log_partitions():
    """U = 1, weight 1, V = 129: mass[v] is 0 exactly where row_logprob(sequential=False) gives NaN or the id is listed, and
    exp(logp) elsewhere; the masses of a call add up to the live users' weights."""
    N, V = 36, 129
    news, user = _vectors(N, V, 1, seed=61)
    news[40, 3] = NAN
    pools = _pools(V, 1)
    listed = torch.tensor([[1, 9, 64, 65, 128, 0, 200]], dtype=torch.int32)
    lists = ops.ExclusionLists(listed, device=DEV)
    tau = 0.6
    base = ops.score_logz(news, user, tau, exclude=lists, **pools)
    _, mass = ops.score_expect_news(news, user, tau, base, exclude=lists, **pools)
    logp, _ = ops.row_logprob(news, user, torch.arange(1, V, dtype=torch.int32, device=DEV)[None, :], tau, base, False, **pools)
    logp = logp[0].double().cpu().numpy()
    m = mass.double().cpu().numpy()
    off = np.isnan(logp)
    off[[0, 8, 63, 64, 127]] = True                                    # the listed ids, as positions of the row 1 .. V-1
    assert m[0] == 0.0 and np.array_equal(m[1:] == 0.0, off) and off.sum() > 10 and (~off).sum() > 50
    hkw = dict({k: v.cpu().numpy() for k, v in pools.items()}, exclude=[listed[0].numpy()])
    _, _, _, _, n, C, G = _reference(news, user, tau, hkw)
    km = kappas(N, V, 1, 0, n, C, G)[1]
    # logp is K14's: formed in fp64 and rounded to fp32 once, |logp| e <= (2 C + ln n) e, with a fl32(1 / tau) of its own (2 C e) and
    # the subtraction's (2 C e): (6 C + ln n + 1) e on top of the mass bound
    p = np.exp(logp[~off])
    assert (np.abs(m[1:][~off] - p) <= (km + 6 * C + math.log(n) + 1) * EPS * p).all()
    assert abs(m.sum() - 1.0) <= km * EPS
    # several users, weights of both signs, two dead users
    U = 33
    news, user = _vectors(N, V, U, seed=67)
    pools = _pools(V, U)
    g = torch.Generator().manual_seed(5)
    w = torch.randn(U, generator=g).to(DEV)
    taus = (0.3 + torch.rand(U, generator=g)).to(DEV)
    taus[9] = 0.0
    base = ops.score_logz(news, user, taus, **pools)
    _, mass = ops.score_expect_news(news, user, taus, base, weight=w, **pools)
    hkw = {k: v.cpu().numpy() for k, v in pools.items()}
    _, _, _, M, n, C, G = _reference(news, user, taus, hkw, weight=w)
    live = torch.ones(U, dtype=torch.bool)
    live[[5, 9]] = False                                               # an empty window, a zero temperature
    assert abs(float(mass.double().sum()) - float(w.double().cpu()[live].sum())) <= kappas(N, V, U, 0, n, C, G)[1] * EPS * M.sum()


@pytest.mark.parametrize("N", [36, 400])
def test_a_rows_bits_depend_on_that_row_alone_at_fixed_splits(N):
    V, U, splits, T = 294, 300, 2, 3
    news, user = _vectors(N, V, U, seed=43)
    pools = _pools(V, U)
    lt = _list_tensor(V, U)
    lists = ops.ExclusionLists(lt, device=DEV)
    targets, gw = _named(V, U, T, seed=3, every=V - 1)
    named = ops._named_by_news(targets, gw, V)
    tau = 0.5
    w = torch.randn(U, generator=torch.Generator().manual_seed(9)).to(DEV)
    base = ops.score_logz(news, user, tau, exclude=lists, **pools)
    call = lambda nv, kw, ex, nm: ops._score_expect_news("score_expect_news", nv, user, tau, base, ex, splits, kw["prior"], kw["stamp"], kw["window"],
                                                         w, nm, True, True)
    out, mass = call(news, pools, lists, named)
    out2, mass2 = call(news, pools, lists, named)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(mass), _bits(mass2))
    # a permuted table, row 0 fixed: new row i is old row perm[i]; prior, stamp, the lists and the named terms go along, the base stays
    perm = torch.cat([torch.zeros(1, dtype=torch.int64), 1 + torch.randperm(V - 1, generator=torch.Generator().manual_seed(3))])
    inv = torch.empty(V + 3, dtype=torch.int64)
    inv[perm] = torch.arange(V)
    inv[V:] = torch.arange(V, V + 3)                                   # ids >= V stay what they are
    pp = dict(prior=pools["prior"][perm.to(DEV)].contiguous(), stamp=pools["stamp"][perm.to(DEV)].contiguous(), window=pools["window"])
    lists_p = ops.ExclusionLists(inv[lt.long()].to(torch.int32), device=DEV)
    named_p = ops._named_by_news(inv[targets.cpu().long()].to(torch.int32).to(DEV), gw, V)
    outp, massp = call(news[perm.to(DEV)].contiguous(), pp, lists_p, named_p)
    assert torch.equal(_bits(outp), _bits(out[perm.to(DEV)])) and torch.equal(_bits(massp), _bits(mass[perm.to(DEV)]))
    # every other news row overwritten with noise: a chosen row keeps its bits
    for v in (1, 31, 32, 150, V - 1):
        noise = torch.randn(V, N, generator=torch.Generator().manual_seed(v)).to(DEV)
        noise[v] = news[v]
        outn, massn = call(noise, pools, lists, named)
        assert torch.equal(_bits(outn[v]), _bits(out[v])) and torch.equal(_bits(massn[v]), _bits(mass[v])), v
    # another slicing: within the bound of each
    hkw = dict({k: v.cpu().numpy() for k, v in pools.items()}, exclude=list(lt.numpy()))
    got3 = ops._score_expect_news("score_expect_news", news, user, tau, base, lists, 3, pools["prior"], pools["stamp"], pools["window"], w, named,
                                  True, True)
    _check(news, user, tau, hkw, got3, 3, note="splits=3", weight=w, named=named, scale=True)


def test_dead_users_contribute_nothing_and_put_no_nan_anywhere():
    N, V, U, splits, T = 36, 130, 70, 1, 2
    news, user = _vectors(N, V, U, seed=71)
    pools = _pools(V, U)                                               # user 5: an empty window, nothing eligible
    g = torch.Generator().manual_seed(13)
    tau = (0.3 + torch.rand(U, generator=g)).to(DEV)
    at = [0, 20, 69]
    tau[at] = torch.tensor([0.0, NAN, INF], device=DEV)
    w = torch.randn(U, generator=g).to(DEV)
    targets, gw = _named(V, U, T, seed=17, every=V - 2)                # every user is named, the dead ones too
    named = ops._named_by_news(targets, gw, V)
    base = [t.clone() for t in ops.score_logz(news, user, tau, **pools)]
    base[0][7] = NAN                                                   # a NaN base
    base[1][8] = INF                                                   # an infinite one
    hkw = {k: v.cpu().numpy() for k, v in pools.items()}
    for scale in (True, False):
        got = _expect_news(news, user, tau, splits=splits, named=named, scale=scale, weight=w, base=base, **pools)
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
        assert not got[0][0].any() and float(got[1][0]) == 0.0
        _check(news, user, tau, hkw, got, splits, note=f"dead users scale={scale}", weight=w, named=named, scale=scale, dead=(7, 8))
    # a weight of NaN on a dead user reaches nothing
    w2 = w.clone()
    w2[[0, 5, 7]] = NAN
    got2 = _expect_news(news, user, tau, splits=splits, named=named, scale=True, weight=w2, base=base, **pools)
    got1 = _expect_news(news, user, tau, splits=splits, named=named, scale=True, weight=w, base=base, **pools)
    assert torch.equal(_bits(got2[0]), _bits(got1[0])) and torch.equal(_bits(got2[1]), _bits(got1[1]))
    # nobody at all: zeros, nothing is launched
    o0, m0 = ops.score_expect_news(news, user[:0], 0.5, [b[:0] for b in base])
    assert o0.shape == (V, N) and m0.shape == (V,) and not o0.any() and not m0.any()


def _labels(fn):
    _lib.prof_enable(1)
    try:
        _lib.prof_collect()
        fn()
        torch.cuda.synchronize()
        return set(_lib.prof_collect().keys())
    finally:
        _lib.prof_enable(0)


@pytest.mark.parametrize("T", [1, 4, 128])
def test_full_softmax_nll_joint_bits_and_the_table_gradient(T):
    N, V, U, tau = 36, 294, 33, 0.7
    news, user = _vectors(N, V, U, seed=53)
    g = torch.Generator().manual_seed(59 + T)
    prior = 0.3 * torch.randn(V, generator=g)
    prior[11] = -INF
    prior[12] = -INF
    lt = _list_tensor(V, U)
    lt[:, 0] = 13                                                     # listed by everybody: eligible for nobody
    lists = ops.ExclusionLists(lt, device=DEV)
    targets = torch.randint(14, V, (U, T), generator=g, dtype=torch.int32)
    targets[3] = 0                                                    # a user whose targets are all fill ...
    targets[5] = 11                                                   # ... and one whose targets are all outside the pool
    if T > 1:
        targets[::3, 1] = 0
        targets[1::4, 2 % T] = 11
        targets[::5, T - 1] = V + 2
    targets = targets.to(DEV)
    kw = dict(exclude=lists, prior=prior.to(DEV))
    gup = torch.randn(U, T, generator=g).to(DEV)
    uv = user.clone().requires_grad_(True)
    nll0, valid0 = ops.full_softmax_nll(news, uv, targets, tau, splits=2, **kw)
    nll0.backward(gup)
    uj, nj = user.clone().requires_grad_(True), news.clone().requires_grad_(True)
    nll, valid = ops.full_softmax_nll_joint(nj, uj, targets, tau, splits=2, **kw)
    assert torch.equal(valid, valid0) and torch.equal(_bits(nll), _bits(nll0)) and not valid.requires_grad
    nll.backward(gup)
    assert torch.equal(_bits(uj.grad), _bits(uv.grad))
    grad = nj.grad
    assert grad.shape == (V, N) and torch.isfinite(grad).all()
    # the float64 autograd gradient of the host statement: log_softmax over the eligible news
    a64, u64 = news.double().cpu().requires_grad_(True), user.double().cpu()
    s = u64 @ a64.T + prior.double()[None, :]
    ok = torch.ones(U, V, dtype=torch.bool)
    ok[:, 0] = False
    ok[:, torch.isneginf(prior)] = False
    ok.scatter_(1, lt.long().clamp(0, V - 1) * (lt < V).long(), False)
    ok[:, 0] = False
    lp = s / tau - torch.logsumexp(torch.where(ok, s / tau, torch.full_like(s, -INF)), dim=1, keepdim=True)
    vc, tc, gc = valid.cpu(), targets.cpu().long().clamp(0, V - 1), gup.double().cpu()
    gw = torch.where(vc, gc, torch.zeros_like(gc))
    (-(torch.where(vc, lp.gather(1, tc), torch.zeros(U, T, dtype=torch.float64)) * gw).sum()).backward()
    # the bound: kappa e A with c_u = sum_t g / tau and the valid targets as named terms, plus the fp32 sum of the T weights on the
    # device ((T - 1) roundings on sum_t |g_ut|) carried through c_u
    gw32 = torch.where(valid, gup, torch.zeros_like(gup))
    named = ops._named_by_news(targets, gw32, V)
    hkw = dict(exclude=list(lt.numpy()), prior=prior.numpy())
    _, A, _, _, n, C, G = _reference(news, user, tau, hkw, weight=gw32.sum(dim=1), named=named, scale=True)
    _, Aabs, _, _, _, _, _ = _reference(news, user, tau, hkw, weight=gw32.abs().sum(dim=1), scale=True)
    bound = kappas(N, V, U, 0, n, C, G)[0] * EPS * A + (T - 1) * EPS * Aabs
    err = np.abs(grad.double().cpu().numpy() - a64.grad.numpy())
    print(f"full_softmax_nll_joint T={T}: worst |grad_news err| / bound = {float((err / bound).max()):.4f}")
    assert (err <= bound).all()
    # news that are eligible for nobody and named by nobody: exactly zero rows
    assert not grad[0].any() and not grad[11].any() and not grad[12].any() and not grad[13].any() and grad[14:].abs().sum(dim=1).gt(0).all()

    def one_side(news_grad, user_grad):
        a, b = news.clone().requires_grad_(news_grad), user.clone().requires_grad_(user_grad)
        out, _ = ops.full_softmax_nll_joint(a, b, targets, tau, splits=2, **kw)
        out.backward(gup)
        return a.grad, b.grad

    res = {}
    only_user = _labels(lambda: res.update(u=one_side(False, True)))
    only_news = _labels(lambda: res.update(n=one_side(True, False)))
    assert any(k.startswith("expect_stream[") for k in only_user) and not any(k.startswith("expect_news") for k in only_user)
    assert any(k.startswith("expect_news_stream[") for k in only_news) and not any(k.startswith("expect_stream[") or k.startswith("expect_final[")
                                                                                  for k in only_news)
    assert res["u"][0] is None and torch.equal(_bits(res["u"][1]), _bits(uv.grad))
    assert res["n"][1] is None and torch.equal(_bits(res["n"][0]), _bits(grad))


def _tiny_case(tag, dt="fp32", scale=1.0):
    model, z, cfg, sd = build_model(tag, dt)
    H, N = cfg.user_log_length, cfg.news_dim
    g = torch.Generator().manual_seed(71)
    Vn, Ur, T = 60, 12, 3
    news_vecs = torch.randn(Vn, N, generator=g) * scale
    news_vecs[0] = 0.0
    hist = torch.randint(1, Vn, (Ur, H), generator=g, dtype=torch.int32)
    mask = torch.ones(Ur, H)
    for u in range(Ur):
        n_pad = u % (H + 1) if u else 0
        n_pad = min(n_pad, H - 1) if cfg.user_log_mask else n_pad     # the masked encoder needs one live slot
        hist[u, :n_pad], mask[u, :n_pad] = 0, 0
    targets = torch.randint(1, Vn, (Ur, T), generator=g, dtype=torch.int32)
    targets[::3, 1] = 0
    targets[1::4, 2] = hist[1::4, -1]                                 # a clicked news: excluded, not scored
    targets[5] = 0
    return model, cfg, sd, news_vecs, hist, mask, targets


def _oracle_loss(tag, cfg, sd, news_vecs, hist, mask, targets, tau):
    """The loss on the CPU with the table as a leaf: the oracle's user encoder on the gathered vectors, then float64 log_softmax over
    the eligible news.  Returns (loss, n, user-encoder gradients, table gradient)."""
    enc = O.nrms_user_encoder if tag.startswith("nrms") else O.naml_user_encoder
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith("user_encoder.")}
    table = news_vecs.clone().requires_grad_(True)
    user = enc(table[hist.long()], mask, sdo, cfg).double()
    s = user @ table.double().T / tau
    Ur, Vn = s.shape
    ok = torch.ones(Ur, Vn, dtype=torch.bool)
    ok[:, 0] = False
    clicked = hist.long() * (mask != 0).long()
    ok.scatter_(1, clicked, False)                                    # the clicked history; a masked slot names news 0
    lp = torch.log_softmax(torch.where(ok, s, torch.full_like(s, -INF)), dim=1)
    t = targets.long()
    valid = (t >= 1) & ok.gather(1, t)
    first = torch.ones_like(valid)
    for j in range(1, t.shape[1]):
        first[:, j] = ~(t[:, j:j + 1] == t[:, :j]).any(dim=1)
    valid &= first
    loss = -(torch.where(valid, lp.gather(1, t), torch.zeros_like(s[:, :t.shape[1]]))).sum() / valid.sum()
    loss.backward()
    return loss.detach(), int(valid.sum()), {k: v.grad for k, v in sdo.items() if v.grad is not None}, table.grad


@pytest.mark.parametrize("tag", ["nrms_tiny_pad", "nrms_tiny_mask", "naml_tiny_3view", "naml_tiny_title_mask"])
def test_full_softmax_loss_joint_on_the_tiny_models(tag):
    """The tolerances are those tests/test_gpu_expect.py holds train.full_softmax_loss to against the same oracle."""
    model, cfg, sd, news_vecs, hist, mask, targets = _tiny_case(tag)
    tau = 0.7
    table = news_vecs.to(DEV).requires_grad_(True)
    loss, n = TR.full_softmax_loss_joint(model, table, hist.numpy(), mask.numpy(), targets.numpy(), tau)
    frozen, n_f = TR.full_softmax_loss(model, table.detach(), hist.numpy(), mask.numpy(), targets.numpy(), tau)
    assert int(n) == int(n_f) and torch.equal(_bits(loss.detach()), _bits(frozen.detach()))
    loss_b, n_b = TR.full_softmax_loss_joint(model, table, hist.numpy(), mask.numpy(), targets.numpy(), tau, batch_size=5)
    assert int(n_b) == int(n)
    assert_close(loss_b, loss, 1e-5, name="loss in batches")
    loss.backward()
    lo, no, go, gt = _oracle_loss(tag, cfg, sd, news_vecs, hist, mask, targets, tau)
    assert no == int(n)
    assert_close(loss, lo, 1e-4, name="loss vs oracle")
    checked = 0
    for name, p in model.named_parameters():
        if not name.startswith("user_encoder.") or not p.requires_grad:
            assert p.grad is None or not p.grad.any(), name
            continue
        if name not in go:                                            # pad_doc under user_log_mask=True: unused in both
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert_close(p.grad, go[name], 1e-6, 2e-4, name="d" + name)
        checked += 1
    assert checked >= 4
    assert_close(table.grad, gt, 1e-6, 2e-4, name="dtable")           # the softmax path plus the history path
    assert not table.grad[0].any() and float(gt.abs().max()) > 0


def test_three_adam_steps_on_the_table_alone_lower_the_loss():
    model, cfg, sd, news_vecs, hist, mask, targets = _tiny_case("nrms_tiny_mask")
    table = news_vecs.to(DEV).requires_grad_(True)
    for p in model.parameters():
        p.requires_grad_(False)
    opt = torch.optim.Adam([table], lr=1e-2)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss, _ = TR.full_softmax_loss_joint(model, table, hist.numpy(), mask.numpy(), targets.numpy(), 0.7)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    assert losses[3] < losses[0] and all(math.isfinite(x) for x in losses), losses


def test_expected_exposure_is_the_column_sum_of_the_softmax():
    model, z, cfg, sd = build_model("nrms_tiny_mask", "fp32")
    H, N, V, U, tau = cfg.user_log_length, cfg.news_dim, 294, 70, 0.6
    g = torch.Generator().manual_seed(83)
    news = torch.randn(V, N, generator=g)
    news[0] = 0.0
    hist = torch.randint(1, V, (U, H), generator=g, dtype=torch.int32)
    mask = torch.ones(U, H)
    hist[::4, :H // 2], mask[::4, :H // 2] = 0, 0
    pools = _pools(V, U)
    got = TR.expected_exposure(model, news.to(DEV), hist.numpy(), mask.numpy(), tau, prior=pools["prior"].cpu().numpy(),
                               news_time=pools["stamp"].cpu().numpy(), window=pools["window"].cpu().numpy())
    assert got.shape == (V,) and got.dtype == torch.float32 and float(got[0]) == 0.0
    _, user, _, _, _ = TR._recommend_args(model, news.to(DEV), hist.numpy(), mask.numpy(), True, 8192, None, None, None, None, None, None)
    hkw = dict({k: v.cpu().numpy() for k, v in pools.items()}, exclude=[(hist[u] * mask[u].int()).numpy() for u in range(U)])
    p, live = metrics.softmax_matrix_reference(news.double().numpy(), user.double().cpu().numpy(), temperature=tau, **hkw)
    _check(news.to(DEV), user, tau, hkw, (None, got), 0, note="expected_exposure")
    assert np.abs(got.double().cpu().numpy() - p.sum(axis=0)).max() < 1e-4 and abs(float(got.double().sum()) - live.sum()) < 1e-3


def test_every_cell_of_the_launch_table_is_launched():
    """3 tiles x pool x lists x rows / mass-only, by the profile labels of the stream."""
    V, U = 40, 9
    want, seen = set(), set()
    for N, TV in ((4, 64), (400, 32), (836, 16)):
        news, user = _vectors(N, V, U, seed=N)
        pools = _pools(V, U)
        lists = ops.ExclusionLists(_list_tensor(V, U), device=DEV)
        for pool in (0, 1):
            for lst in (0, 1):
                kw = dict(pools if pool else {}, **(dict(exclude=lists) if lst else {}))
                base = ops.score_logz(news, user, 0.5, **kw)
                for rows in (0, 1):
                    want.add((TV, pool, lst, rows))
                    for label in _labels(lambda: ops.score_expect_news(news, user, 0.5, base, rows=bool(rows), **kw)):
                        if label.startswith("expect_news_stream["):
                            f = dict(kv.split("=") for kv in label[len("expect_news_stream["):-1].split(","))
                            seen.add((int(f["TV"]), int(f["pool"]), int(f["lists"]), int(f["rows"])))
    assert seen == want and len(want) == 24
