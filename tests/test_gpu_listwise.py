"""GPU: listwise training on served rows (nr_row_logprob_grad; ops.row_logprob_grad / ops.plackett_luce_nll; train.listwise_loss;
include/nrhip.h, K19).  The coefficients (a, c) are held to the bound DERIVED in DESIGN.md section 5 (kappa19, below) against
metrics.row_logprob_grad_reference in float64 on the fp32 inputs; the finished gradients to K17's / K18's kappa-bounds scaled by |a|
plus the coefficient terms, against float64 autograd of the dense sequential statement; bit statements where the contract makes them
(a user's coefficients do not depend on the other users; K13 / K14 are untouched; the forward is sample_propensity's)."""
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
DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _seg(V):
    return 128 * math.ceil((V - 1) / (128 * 256))


def _stats(news, user, taus, exclude, prior=None, stamp=None, window=None):
    """Per user, in float64 on the fp32 inputs, over the news that are eligible under `exclude`: n = how many, C = max |s| / tau,
    G = max (sum_c |user_c news_vc| + |prior_v|) / tau (0 where there is none or the temperature is bad)."""
    a, b = news.double().cpu().numpy(), user.double().cpu().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        scores, pool = metrics._pooled(b @ a.T, prior, stamp, window)
        mag = np.abs(b) @ np.abs(a).T + (0.0 if prior is None else np.abs(np.asarray(prior, dtype=np.float64))[None, :])
    U, V = scores.shape
    n, Cs, Gs = np.zeros(U), np.zeros(U), np.zeros(U)
    for u in range(U):
        ok = ~np.isnan(scores[u]) & pool[u]
        ok[0] = False
        if exclude is not None:
            ex = np.asarray(exclude[u], dtype=np.int64).reshape(-1)
            ok[ex[(ex >= 1) & (ex < V)]] = False
        n[u] = ok.sum()
        if n[u] and taus[u] > 0 and np.isfinite(taus[u]):
            Cs[u] = np.abs(scores[u, ok]).max() / taus[u]
            Gs[u] = mag[u, ok].max() / taus[u]
    return n, Cs, Gs


def kappa19(N, V, n, G):
    """|a - a*| <= kappa e A_a, |c_i - c*_i| <= kappa e A_i with A_a = sum_j |g_j| B* / W*_j, A_i = |g_i| + e*_i sum_{j <= i} |g_j| / W*_j,
    e = 2^-24 ("Listwise training").  Every term of a and c is g_j times a ratio in [0, 1] of two positive sums of
    exp(s / tau) over device scores, one of them holding the base.  First order in e:
      score chain   |s - s*| <= (N + 1) e (sum_c |u_c n_vc| + |prior_v|), i.e. (N + 1) G e in every exponent, numerator and denominator:
                    2 (N + 1) G e relative in the ratio
      base          K13's logsum bound (4 ln n + 7 K + 14) e, K = 2 seg / 128: a relative error of B, at most that in the ratio
      the rest      fp64 scans on the fp32 temperature itself (no fl(1 / tau)): e for all of it; the one rounding to fp32: e.
    Sum: 2 (N + 1) G + 4 ln n + 7 K + 16.  G is taken over the base AND the row (everything eligible under the user's own lists)."""
    return 2.0 * (N + 1) * G + 4.0 * np.log(np.maximum(n, 2)) + 7.0 * (2 * _seg(V) // 128) + 16.0


def kappa17(N, V, splits, n, C, G):
    """K17's kappa (tests/test_gpu_expect.py): 2 (N + 1) G + 6 C + 5 ln n + 7 K + L + 26."""
    seg = _seg(V)
    nseg = math.ceil((V - 1) / seg)
    segs_per = math.ceil(nseg / min(splits, nseg)) if splits > 0 else nseg
    return 2.0 * (N + 1) * G + 6.0 * C + 5.0 * np.log(np.maximum(n, 2)) + 7.0 * (2 * seg // 128) + 128.0 * segs_per * (seg // 128) + 26.0


def kappa18(N, V, U, n, C, G):
    """K18's kappa at splits = 0 (tests/test_gpu_expect_news.py): 2 (N + 1) G + 6 C + 5 ln n + 7 K + L + 29, L one slice of all users."""
    useg = 128 * math.ceil(U / (128 * 256))
    chunks = math.ceil(U / useg) * (useg // 128)
    return 2.0 * (N + 1) * G + 6.0 * C + 5.0 * math.log(max(n, 2)) + 7.0 * (2 * _seg(V) // 128) + 128.0 * chunks + 29.0


def _vectors(N, V, U, seed=11):
    g = torch.Generator().manual_seed(seed)
    news = torch.randn(V, N, generator=g)
    user = torch.randn(U, N, generator=g) / N ** 0.5                  # scores of about unit spread
    return news.to(DEV), user.to(DEV)


def _pools(V, U, seed=17):
    g = torch.Generator().manual_seed(seed)
    prior = 0.3 * torch.randn(V, generator=g)
    prior[torch.randperm(V, generator=g)[: max(V // 10, 1)]] = -INF   # a tenth of the news switched off
    stamp = torch.randint(0, 100, (V,), generator=g, dtype=torch.int32)
    lo = torch.randint(0, 30, (U,), generator=g, dtype=torch.int32)
    window = torch.stack([lo, lo + 60], dim=1)
    return prior, stamp, window


def _rows(V, U, k, seed, fills=True):
    """Rows without repeats: a random order of [1, V) cut to k (a short corpus ends in fill); with `fills`, fill entries inside."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.zeros(U, k, dtype=torch.int32)
    for u in range(U):
        perm = (torch.randperm(V - 1, generator=g)[:k] + 1).to(torch.int32)
        rows[u, : perm.numel()] = perm
    if fills and k > 1:
        rows[::3, k // 2] = 0
        rows[1::4, 0] = V + 2
        rows[2::5, k - 1] = -1
    return rows


def _coefficients(news, user, rows, tau, g=None, lists=None, prior=None, stamp=None, window=None):
    """K13 on the lists merged with the row, then K19: (a, c, base)."""
    taken = ops.ExclusionLists(rows.to(DEV))
    merged = taken if lists is None else ops.ExclusionLists(lists, device=DEV).merged(taken)
    kw = {k: v.to(DEV) for k, v in dict(prior=prior, stamp=stamp, window=window).items() if v is not None}
    base = ops.score_logz(news, user, tau, exclude=merged, **kw)
    a, c = ops.row_logprob_grad(news, user, rows.to(DEV), tau, base, g=None if g is None else g.to(DEV), **kw)
    return a, c, base


def _check(news, user, rows, tau, g, lists, pools, got, note):
    """(a, c) of `got` against the float64 reference within kappa19's bound; |a - sum c| within the sum of the bounds; exact zeros for
    bad-temperature and empty-base users.  Returns the worst fraction of the bound."""
    a_d, c_d = (t.double().cpu().numpy() for t in got)
    N, V, U, k = news.shape[1], news.shape[0], user.shape[0], rows.shape[1]
    taus = np.array(metrics._temperatures(_host(tau.float()) if isinstance(tau, torch.Tensor) else float(np.float32(tau)), U)[0], dtype=np.float64)
    hkw = {kk: _host(v) for kk, v in pools.items() if v is not None}
    r = rows.numpy().astype(np.int64)
    own = [np.zeros(0, dtype=np.int64) if lists is None else np.asarray(lists[u]) for u in range(U)]
    merged = [np.concatenate([own[u], r[u]]) for u in range(U)]
    a64, b64 = news.double().cpu().numpy(), user.double().cpu().numpy()
    base = metrics.logz_reference(a64, b64, temperature=taus, exclude=merged, **hkw)
    gh = None if g is None else g.double().numpy()
    a_r, c_r = metrics.row_logprob_grad_reference(a64, b64, row_ids=r, temperature=taus, base=base[:2], g=gh, **hkw)
    gabs = np.ones((U, k)) if g is None else np.abs(gh)
    A_a, c_abs = metrics.row_logprob_grad_reference(a64, b64, row_ids=r, temperature=taus, base=base[:2], g=gabs, **hkw)
    real = (r >= 1) & (r < V)
    _, pool = metrics._pooled(np.zeros((U, V)), hkw.get("prior"), hkw.get("stamp"), hkw.get("window"))
    step = real & np.take_along_axis(pool, np.clip(r, 0, V - 1), axis=1)   # a real id inside the pool (no score here is NaN)
    A_c = np.where(step, 2.0 * gabs - c_abs, 0.0)                     # c(|g|) = |g_i| - e_i sum |g_j| / W_j, so A_i = 2 |g_i| - c(|g|)
    _, _, G = _stats(news, user, taus, own, **hkw)                    # over the base and the row
    kap = kappa19(N, V, base[2], G)
    tiny = V * 2.0 ** -126 * gabs.sum(axis=1)                         # weights below the normal range are lost at 2^-126 each
    bound_a = kap * EPS * A_a + tiny
    bound_c = kap[:, None] * EPS * A_c + tiny[:, None]
    assert np.isfinite(a_d).all() and np.isfinite(c_d).all(), note
    err_a, err_c = np.abs(a_d - a_r), np.abs(c_d - c_r)
    frac = max(float((err_a / np.maximum(bound_a, 1e-300)).max()), float((err_c / np.maximum(bound_c, 1e-300)).max()))
    ident = np.abs(a_d - c_d.sum(axis=1))
    ident_bound = bound_a + bound_c.sum(axis=1)
    ifrac = float((ident / np.maximum(ident_bound, 1e-300)).max())
    print(f"row_logprob_grad {note}: N={N} V={V} U={U} k={k} worst |err| / bound = {frac:.4f}, |a - sum c| / bound = {ifrac:.4f}")
    assert (err_a <= bound_a).all() and (err_c <= bound_c).all(), (note, frac)
    assert (ident <= ident_bound).all(), (note, ifrac)
    # what is no step has c = 0 exactly; bad-temperature users are zeros; an empty base has a = 0 exactly
    assert not c_d[~step].any() and not c_r[~step].any(), note
    with np.errstate(invalid="ignore"):
        bad = ~(np.isfinite(taus) & (taus > 0))
    assert not a_d[bad].any() and not c_d[bad].any(), note
    assert not a_d[base[2] == 0].any(), note
    return frac


# (N, V, U, k, what): N one k-slab / npad > N / MIND's width; V a single news, exactly one chunk, a partial last chunk; U one user, 16
# users + 1 (two workgroups), 2 * 16 + 1 (the wave stride: waves 0 and 8 of a workgroup's users); k the lane pair, an odd tail, a full row
CASES = [(4, 2, 1, 1, "plain"), (4, 129, 17, 2, "g"), (4, 294, 33, 3, "g pools"), (36, 129, 33, 127, "g lists"),
         (36, 129, 17, 128, "plain"), (36, 294, 17, 128, "g pools lists"), (36, 294, 1, 128, "plain pools"), (400, 129, 17, 1, "g taus"),
         (400, 294, 33, 128, "g pools taus"), (400, 294, 17, 3, "g peaked"), (400, 294, 33, 127, "g flat lists"), (36, 294, 33, 2, "g peaked taus pools"),
         (400, 2, 33, 1, "g flat")]


@pytest.mark.parametrize("N,V,U,k,what", CASES, ids=lambda v: str(v).replace(" ", "-"))
def test_coefficients_within_the_derived_bound(N, V, U, k, what):
    news, user = _vectors(N, V, U, seed=7 + N + V + k)
    rows = _rows(V, U, k, seed=N + k)
    gen = torch.Generator().manual_seed(3 * N + k)
    g = None
    if "g" in what.split():
        g = torch.randn(U, k, generator=gen)                          # signed, with zeros
        g[torch.rand(U, k, generator=gen) < 0.2] = 0.0
    pools = dict(zip(("prior", "stamp", "window"), _pools(V, U) if "pools" in what else (None, None, None)))
    lists = [torch.randint(0, V + 3, (int(torch.randint(0, 40, (1,), generator=gen)),), generator=gen).numpy() for _ in range(U)] if "lists" in what else None
    with torch.no_grad():
        spread = float((user @ news.T).std())
    tau = 0.7
    if "peaked" in what:
        tau = 0.01 * spread                                           # most e_i / W_j underflow to 0
    if "flat" in what:
        tau = 100.0 * spread
    if "taus" in what:
        t = torch.full((U,), float(tau)) * torch.linspace(0.5, 2.0, U)
        for at, v in zip((0, 5, 16), (0.0, NAN, INF)):
            if at < U:
                t[at] = v
        tau = t.to(DEV)
    a, c, _ = _coefficients(news, user, rows, tau, g=g, lists=lists, **pools)
    _check(news, user, rows, tau, g, lists, pools, (a, c), what)


def test_coefficients_of_a_user_do_not_depend_on_the_other_users_and_k13_k14_are_untouched():
    N, V, U, k = 36, 294, 35, 5
    news, user = _vectors(N, V, U, seed=23)
    rows = _rows(V, U, k, seed=29)
    prior, stamp, window = _pools(V, U)
    g = torch.randn(U, k, generator=torch.Generator().manual_seed(31))
    taus = torch.linspace(0.3, 1.5, U).to(DEV)
    kw = dict(prior=prior.to(DEV), stamp=stamp.to(DEV), window=window.to(DEV))
    merged = ops.ExclusionLists(rows.to(DEV))
    before = ops.score_logz(news, user, taus, exclude=merged, **kw)
    lp_before = ops.row_logprob(news, user, rows.to(DEV), taus, before, True, **kw)
    a, c = ops.row_logprob_grad(news, user, rows.to(DEV), taus, before, g=g.to(DEV), **kw)
    after = ops.score_logz(news, user, taus, exclude=merged, **kw)
    lp_after = ops.row_logprob(news, user, rows.to(DEV), taus, after, True, **kw)
    for x, y in zip(before + lp_before, after + lp_after):
        assert torch.equal(_bits(x), _bits(y))
    for u in range(U):
        kw_u = dict(kw, window=kw["window"][u:u + 1].contiguous())
        a1, c1 = ops.row_logprob_grad(news, user[u:u + 1].contiguous(), rows[u:u + 1].to(DEV), taus[u:u + 1].contiguous(),
                                      (before[0][u:u + 1].contiguous(), before[1][u:u + 1].contiguous()), g=g[u:u + 1].to(DEV), **kw_u)
        assert torch.equal(_bits(a1), _bits(a[u:u + 1])) and torch.equal(_bits(c1), _bits(c[u:u + 1])), u
    # a permutation of the users permutes the outputs
    perm = torch.randperm(U, generator=torch.Generator().manual_seed(37))
    pd = perm.to(DEV)
    a2, c2 = ops.row_logprob_grad(news, user[pd].contiguous(), rows[perm].to(DEV), taus[pd].contiguous(), (before[0][pd], before[1][pd]),
                                  g=g[perm].to(DEV), prior=kw["prior"], stamp=kw["stamp"], window=kw["window"][pd].contiguous())
    assert torch.equal(_bits(a2), _bits(a[pd])) and torch.equal(_bits(c2), _bits(c[pd]))
    assert ops.row_logprob_grad(news, user[:0], rows[:0].to(DEV), 0.5, (before[0][:0], before[1][:0]))[1].shape == (0, k)


def _tiny_case(tag, k=5):
    model, z, cfg, sd = build_model(tag, "fp32")
    H, N = cfg.user_log_length, cfg.news_dim
    g = torch.Generator().manual_seed(71)
    Vn, Ur = 60, 12
    news_vecs = torch.randn(Vn, N, generator=g)
    news_vecs[0] = 0.0
    hist = torch.randint(1, Vn, (Ur, H), generator=g, dtype=torch.int32)
    mask = torch.ones(Ur, H)
    for u in range(Ur):
        n_pad = u % (H + 1) if u else 0
        n_pad = min(n_pad, H - 1) if cfg.user_log_mask else n_pad     # the masked encoder needs one live slot
        hist[u, :n_pad], mask[u, :n_pad] = 0, 0
    rows = _rows(Vn, Ur, k, seed=73, fills=False)
    rows[::3, 1] = 0                                                  # fill in the middle
    rows[1::4, 2] = hist[1::4, -1]                                    # a clicked news: excluded, no step
    rows[2, 3] = rows[2, 0]                                           # a later repeat: no step
    rows[5] = 0                                                       # a row without a valid entry
    return model, cfg, sd, news_vecs, hist, mask, rows


def test_plackett_luce_nll_forward_is_sample_propensity_bit_for_bit():
    model, cfg, sd, news_vecs, hist, mask, _ = _tiny_case("nrms_tiny_pad")
    nv = news_vecs.to(DEV)
    Ur, Vn, k = hist.shape[0], nv.shape[0], 59                        # more than anybody has left (news 9 is off): rows end in fill
    prior = torch.zeros(Vn)
    prior[9] = -INF
    with torch.no_grad():
        _, user, exclude, kw, _ = TR._recommend_args(model, nv, hist.numpy(), mask.numpy(), True, 8192, prior, None, None, None, None, None)
    taus = torch.linspace(0.4, 1.2, Ur).to(DEV)
    ids, _, _ = ops.score_sample(nv, user, k, taus, 1234, exclude=exclude, **kw)
    assert (ids[:, -1] == 0).all() and (ids[:, 0] > 0).all()
    for tau in (0.7, taus):
        logp, _ = TR.sample_propensity(model, nv, hist.numpy(), mask.numpy(), ids, tau, prior=prior)
        nll, valid = ops.plackett_luce_nll(nv, user, ids, tau, exclude=exclude, **kw)
        assert torch.equal(valid, ids > 0) and not valid.requires_grad
        assert torch.equal(_bits(nll[valid]), _bits((-logp)[valid])) and not nll[~valid].any() and float(nll.sum()) > 0
    # valid: fill, an entry outside the pool, a bad temperature entry
    rows = ids.clone()
    rows[0, 1], rows[1, 0] = 9, Vn + 4
    bad = taus.clone()
    bad[2], bad[3], bad[4] = 0.0, NAN, INF
    nll, valid = ops.plackett_luce_nll(nv, user, rows, bad, exclude=exclude, **kw)
    want = (rows > 0) & (rows < Vn) & (rows != 9)
    want[2:5] = False
    assert torch.equal(valid, want) and not nll[~valid].any() and torch.isfinite(nll).all()
    logp, _ = TR.sample_propensity(model, nv, hist.numpy(), mask.numpy(), rows, bad, prior=prior)
    assert torch.equal(_bits(nll[valid]), _bits((-logp)[valid]))


def _labels(fn):
    _lib.prof_enable(1)
    try:
        _lib.prof_collect()
        fn()
        torch.cuda.synchronize()
        return set(_lib.prof_collect().keys())
    finally:
        _lib.prof_enable(0)


def _dense_nll(s_over_tau, rest, rows, V):
    """float64 torch: nll [k] of one user's row under the dense sequential statement -- per live step a logsumexp over the base (`rest`,
    bool [V]: eligible and not named by the row) and the live entries from that step on; (nll, live)."""
    k = rows.shape[0]
    real = (rows >= 1) & (rows < V)
    at = rows.clamp(0, V - 1)
    x = s_over_tau[at]
    live = real & torch.isfinite(x)                                   # outside the pool: the caller put -inf there
    keep = torch.triu(torch.ones(k, k, dtype=torch.bool)) & live[None, :]
    row_part = torch.where(keep, x[None, :].expand(k, k), torch.full((k, k), -INF, dtype=torch.float64))
    base_part = torch.where(rest, s_over_tau, torch.full_like(s_over_tau, -INF))[None, :].expand(k, V)
    dummy = torch.where(live, torch.full_like(x, -INF), torch.zeros_like(x))[:, None]   # a dead step sums something finite: no NaN in backward
    lse = torch.logsumexp(torch.cat([row_part, base_part, dummy], dim=1), dim=1)
    safe = torch.where(live, x, torch.zeros_like(x))
    return torch.where(live, -(safe - torch.where(live, lse, torch.zeros_like(lse))), torch.zeros_like(x)), live


@pytest.mark.parametrize("k", [1, 4, 128])
def test_plackett_luce_nll_gradients_against_the_dense_statement(k):
    N, V, U, tau = 36, 294, 33, float(np.float32(0.7))
    news, user = _vectors(N, V, U, seed=53)
    gen = torch.Generator().manual_seed(59 + k)
    prior = 0.3 * torch.randn(V, generator=gen)
    prior[11] = -INF
    raw = [torch.randint(1, V, (int(torch.randint(0, 30, (1,), generator=gen)),), generator=gen).unique() for _ in range(U)]
    raw[2] = torch.arange(1, 40)
    rows = _rows(V, U, k, seed=61 + k, fills=False)
    for u in range(U):                                                # rows name nothing the lists hold (what listwise_loss turns into fill)
        rows[u][torch.isin(rows[u], raw[u].to(torch.int32))] = 0
    rows[3] = 0                                                       # a user whose row is all fill ...
    rows[5] = 11                                                      # ... and one whose row is all outside the pool
    if k > 1:
        rows[::3, 1] = 0
        rows[1::4, 2 % k] = 11
        rows[::5, k - 1] = V + 2
    lists = ops.ExclusionLists(raw, device=DEV)
    kw = dict(exclude=lists, prior=prior.to(DEV))
    rd = rows.to(DEV)
    uj, nj = user.clone().requires_grad_(True), news.clone().requires_grad_(True)
    nll, valid = ops.plackett_luce_nll(nj, uj, rd, tau, splits=2, **kw)
    want_valid = (rd >= 1) & (rd < V) & (rd != 11)
    assert torch.equal(valid, want_valid) and not valid[3].any() and not valid[5].any()
    gup = torch.randn(U, k, generator=gen).to(DEV)
    nll.backward(gup)
    gu, gn = uj.grad, nj.grad
    assert torch.isfinite(gu).all() and torch.isfinite(gn).all() and gn.shape == (V, N)
    live_u = valid.any(dim=1).cpu().numpy()
    assert not gu[3].any() and not gu[5].any() and not gu[torch.from_numpy(~live_u).to(DEV)].any()
    # float64 autograd of the dense statement
    a64, u64 = news.double().cpu().requires_grad_(True), user.double().cpu().requires_grad_(True)
    s = (u64 @ a64.T + prior.double()[None, :]) / tau
    gc = torch.where(valid.cpu(), gup.double().cpu(), torch.zeros(U, k, dtype=torch.float64))
    total = torch.zeros((), dtype=torch.float64)
    nll64 = torch.zeros(U, k, dtype=torch.float64)
    merged = []
    for u in range(U):
        r = rows[u].long()
        rest = torch.ones(V, dtype=torch.bool)
        rest[0] = False
        rest[torch.isneginf(prior)] = False
        rest[raw[u]] = False
        rest[r[(r >= 1) & (r < V)]] = False
        merged.append(np.concatenate([raw[u].numpy(), r.numpy()]))
        nl, live = _dense_nll(s[u], rest, r, V)
        assert torch.equal(live, valid[u].cpu())
        nll64[u] = nl.detach()
        total = total + (gc[u] * nl).sum()
    total.backward()
    # the bounds.  Coefficients: kappa19 on (A_a, A_i); grad_user: K17's kappa e |a| A_c, the coefficient errors on |E| and |news[row]|, and
    # fl(1 / tau) and the final rounding (2 e) on all that was added up; grad_news: K18's kappa e A_vc and the coefficient errors carried
    # through p and the named terms.
    hkw = dict(prior=prior.numpy())
    n_a, b_a = news.double().cpu().numpy(), user.double().cpu().numpy()
    taus = np.full(U, tau)
    base = metrics.logz_reference(n_a, b_a, temperature=taus, exclude=merged, **hkw)
    gh, rn = gc.numpy(), rows.numpy().astype(np.int64)
    a_r, c_r = metrics.row_logprob_grad_reference(n_a, b_a, row_ids=rn, temperature=taus, base=base[:2], g=gh, **hkw)
    A_a, c_abs = metrics.row_logprob_grad_reference(n_a, b_a, row_ids=rn, temperature=taus, base=base[:2], g=np.abs(gh), **hkw)
    A_i = np.where(valid.cpu().numpy(), 2.0 * np.abs(gh) - c_abs, 0.0)
    _, _, G_row = _stats(news, user, taus, [r.numpy() for r in raw], **hkw)
    n_b, C_b, G_b = _stats(news, user, taus, merged, **hkw)
    k19 = kappa19(N, V, base[2], G_row)
    # the forward: log of a ratio kappa19 bounds relatively, so (kappa19 - 1) e absolutely, and the rounding of the result
    nll_bound = (k19[:, None] - 1.0) * EPS + EPS * np.abs(nll64.numpy())
    nll_err = np.abs(nll.detach().double().cpu().numpy() - nll64.numpy())
    assert (nll_err <= nll_bound).all(), float((nll_err / nll_bound).max())
    da, dc = k19 * EPS * A_a, k19[:, None] * EPS * A_i
    p, _ = metrics.softmax_matrix_reference(n_a, b_a, temperature=taus, exclude=merged, **hkw)
    absn, absu = np.abs(n_a), np.abs(b_a)
    at = np.clip(rn, 0, V - 1)
    named_abs = (np.abs(c_r)[:, :, None] * absn[at]).sum(axis=1)      # sum_i |c_i| |news[row_i]|, [U, N]; c = 0 at what is no step
    named_err = (dc[:, :, None] * absn[at]).sum(axis=1)
    E_abs = p @ absn                                                  # A_c of K17 (>= |E|)
    bound_u = (kappa17(N, V, 2, n_b, C_b, G_b)[:, None] * EPS * np.abs(a_r)[:, None] * E_abs + da[:, None] * E_abs + named_err
               + 2 * EPS * (np.abs(a_r)[:, None] * E_abs + named_abs)) / tau
    err_u = np.abs(gu.double().cpu().numpy() - u64.grad.numpy())
    ru = float((err_u[live_u] / np.maximum(bound_u[live_u], 1e-300)).max())
    k18 = kappa18(N, V, U, float(n_b.max()), float(C_b.max()), float(G_b.max()))
    A_v = p.T @ ((np.abs(a_r) / tau)[:, None] * absu)
    dA_v = p.T @ ((da / tau)[:, None] * absu)
    for u in range(U):
        for i in range(k):
            if valid[u, i]:
                A_v[rn[u, i]] += np.abs(c_r[u, i]) / tau * absu[u]
                dA_v[rn[u, i]] += dc[u, i] / tau * absu[u]
    bound_n = k18 * EPS * A_v + dA_v + U * 2.0 ** -126
    err_n = np.abs(gn.double().cpu().numpy() - a64.grad.numpy())
    rnw = float((err_n / np.maximum(bound_n, 1e-300)).max())
    print(f"plackett_luce_nll k={k}: worst |grad_user err| / bound = {ru:.4f}, |grad_news err| / bound = {rnw:.4f}")
    assert (err_u[live_u] <= bound_u[live_u]).all() and not err_u[~live_u].any()
    assert (err_n <= bound_n).all()
    assert not gn[0].any() and not gn[11].any()

    # a pass whose input needs no gradient is not launched; the pass that is launched has the bits of the joint call
    def one_side(news_grad, user_grad):
        x, y = news.clone().requires_grad_(news_grad), user.clone().requires_grad_(user_grad)
        out, _ = ops.plackett_luce_nll(x, y, rd, tau, splits=2, **kw)
        out.backward(gup)
        return x.grad, y.grad

    res = {}
    only_user = _labels(lambda: res.update(u=one_side(False, True)))
    only_news = _labels(lambda: res.update(n=one_side(True, False)))
    assert any(x.startswith("logp_grad[") for x in only_user) and any(x.startswith("expect_stream[") for x in only_user)
    assert not any(x.startswith("expect_news") for x in only_user)
    assert any(x.startswith("logp_grad[") for x in only_news) and any(x.startswith("expect_news_stream[") for x in only_news)
    assert not any(x.startswith("expect_stream[") or x.startswith("expect_final[") for x in only_news)
    assert res["u"][0] is None and torch.equal(_bits(res["u"][1]), _bits(gu))
    assert res["n"][1] is None and torch.equal(_bits(res["n"][0]), _bits(gn))


def test_a_row_that_takes_everything_keeps_its_named_terms_on_the_news_side():
    """An empty base: a = 0, the stream adds nothing, and the gradient is the named terms alone -- on both sides.  K18 by itself leaves
    such a user's named terms out; the autograd layer hands it a finite base for them.  The derived bounds are held in the test above;
    the tolerance here (1e-5 absolute and relative on entries of order |vector| / tau = 1) tells the presence of those terms from their
    absence and leaves room for a few fp32 roundings of sums of at most 8 of them."""
    N, V, U, k, tau = 36, 9, 3, 8, float(np.float32(0.5))
    news, user = _vectors(N, V, U, seed=83)
    rows = _rows(V, U, k, seed=89, fills=False)
    rows[1, 4:] = 0                                                   # user 1 leaves four news to the base
    uj, nj = user.clone().requires_grad_(True), news.clone().requires_grad_(True)
    nll, valid = ops.plackett_luce_nll(nj, uj, rows.to(DEV), tau)
    gup = torch.randn(U, k, generator=torch.Generator().manual_seed(97)).to(DEV)
    nll.backward(gup)
    a64, u64 = news.double().cpu().requires_grad_(True), user.double().cpu().requires_grad_(True)
    s = (u64 @ a64.T) / tau
    total = torch.zeros((), dtype=torch.float64)
    for u in range(U):
        r = rows[u].long()
        rest = torch.ones(V, dtype=torch.bool)
        rest[0] = False
        rest[r[r >= 1]] = False
        nl, _ = _dense_nll(s[u], rest, r, V)
        total = total + (gup[u].double().cpu() * nl).sum()
    total.backward()
    assert_close(uj.grad, u64.grad, 1e-5, 1e-5, name="grad_user")
    assert_close(nj.grad, a64.grad, 1e-5, 1e-5, name="grad_news")
    assert float(nll.detach()[0, k - 1]) == 0.0 and float(nj.grad[1:].abs().sum()) > 0


def _oracle_listwise(tag, cfg, sd, news_vecs, hist, mask, rows, tau, weight):
    """The loss on the CPU with the table as a leaf: the oracle's user encoder on the gathered vectors, then the dense float64 sequential
    statement.  Returns (loss, n rows, user-encoder gradients, table gradient)."""
    enc = O.nrms_user_encoder if tag.startswith("nrms") else O.naml_user_encoder
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith("user_encoder.")}
    table = news_vecs.clone().requires_grad_(True)
    user = enc(table[hist.long()], mask, sdo, cfg).double()
    s = user @ table.double().T / tau
    Ur, Vn = s.shape
    k = rows.shape[1]
    w = torch.ones(Ur, k, dtype=torch.float64) if weight is None else (weight.double()[:, None].expand(Ur, k) if weight.dim() == 1 else weight.double())
    total, n = torch.zeros((), dtype=torch.float64), 0
    clicked = hist.long() * (mask != 0).long()
    for u in range(Ur):
        r = rows[u].long().clone()
        for j in range(k):                                            # excluded entries and later repeats are no step
            if r[j] >= 1 and (bool((clicked[u] == r[j]).any()) or bool((r[:j] == r[j]).any())):
                r[j] = 0
        rest = torch.ones(Vn, dtype=torch.bool)
        rest[0] = False
        rest[clicked[u]] = False
        rest[r[r >= 1]] = False
        nl, live = _dense_nll(s[u], rest, r, Vn)
        total = total + (w[u] * nl).sum()
        n += int(live.any())
    loss = total / max(n, 1)
    loss.backward()
    return loss.detach(), n, {k_: v.grad for k_, v in sdo.items() if v.grad is not None}, table.grad


@pytest.mark.parametrize("tag", ["nrms_tiny_pad", "naml_tiny_3view"])
def test_listwise_loss_on_the_tiny_models(tag):
    """The tolerances are those tests/test_gpu_expect.py holds train.full_softmax_loss to against the same oracle."""
    model, cfg, sd, news_vecs, hist, mask, rows = _tiny_case(tag)
    tau = 0.7
    Ur, k = rows.shape
    gen = torch.Generator().manual_seed(101)
    per_row = torch.randn(Ur, generator=gen)                          # rewards of either sign
    assert (per_row < 0).any() and (per_row > 0).any()
    per_place = 1.0 / torch.log2(torch.arange(k) + 2.0)[None, :] * (1.0 + torch.rand(Ur, k, generator=gen))
    for weight in (None, per_row, per_place):
        model.zero_grad()
        table = news_vecs.to(DEV).requires_grad_(True)
        loss, n = TR.listwise_loss(model, table, hist.numpy(), mask.numpy(), rows.numpy(), tau, weight=weight)
        assert n.dtype == torch.int64 and n.dim() == 0 and n.device.type == "cuda"
        loss_b, n_b = TR.listwise_loss(model, table, hist.numpy(), mask.numpy(), rows.numpy(), tau, weight=weight, batch_size=5)
        assert int(n_b) == int(n)
        assert_close(loss_b, loss, 1e-5, name="loss in batches")
        loss.backward()
        lo, no, go, gt = _oracle_listwise(tag, cfg, sd, news_vecs, hist, mask, rows, tau, weight)
        assert no == int(n) == Ur - 1                                 # rows, not entries: row 5 has no valid entry
        assert_close(loss, lo, 1e-4, name="loss vs oracle")
        checked = 0
        for name, p in model.named_parameters():
            if not name.startswith("user_encoder.") or not p.requires_grad:
                assert p.grad is None or not p.grad.any(), name
                continue
            if name not in go:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
                continue
            assert_close(p.grad, go[name], 1e-6, 2e-4, name="d" + name)
            checked += 1
        assert checked >= 4
        assert_close(table.grad, gt, 1e-6, 2e-4, name="dtable")       # the softmax path plus the history path
        assert not table.grad[0].any() and float(gt.abs().max()) > 0
    # with weight = None the loss is -sample_propensity's total over the rows that count, on the rows listwise_loss scores
    with torch.no_grad():
        loss, n = TR.listwise_loss(model, news_vecs.to(DEV), hist.numpy(), mask.numpy(), rows.numpy(), tau)
    ex = TR._exclusions(hist.to(DEV), mask.to(DEV), True, None, torch.device(DEV))
    clean = rows.to(DEV).masked_fill(TR._not_ranked(ex, rows.to(DEV), news_vecs.shape[0]), 0)
    _, total = TR.sample_propensity(model, news_vecs.to(DEV), hist.numpy(), mask.numpy(), clean, tau)
    assert_close(loss, -total.double().sum() / int(n), 1e-6, 1e-5, name="loss vs sample_propensity")   # an fp32 sum of 60 terms: 60 e relative
    # refusals
    with pytest.raises(ValueError, match="group caps"):
        TR.listwise_loss(model, news_vecs.to(DEV), hist.numpy(), mask.numpy(), rows.numpy(), tau, news_group=np.zeros(60, dtype=np.int32))
    with pytest.raises(RuntimeError, match="cannot be cut"):
        TR.listwise_loss(model, news_vecs.to(DEV), hist.numpy(), mask.numpy(), np.ones((Ur, 129), dtype=np.int32), tau)
    with pytest.raises(RuntimeError, match="weight must be"):
        TR.listwise_loss(model, news_vecs.to(DEV), hist.numpy(), mask.numpy(), rows.numpy(), tau, weight=torch.ones(Ur, k + 1))
    # nothing valid anywhere: loss 0, n 0
    loss0, n0 = TR.listwise_loss(model, news_vecs.to(DEV), hist.numpy(), mask.numpy(), np.zeros((Ur, 3), dtype=np.int32), tau)
    assert float(loss0.detach()) == 0.0 and int(n0) == 0


def test_three_adam_steps_lower_the_listwise_loss():
    model, cfg, sd, news_vecs, hist, mask, rows = _tiny_case("nrms_tiny_mask")
    nv = news_vecs.to(DEV)
    opt = torch.optim.Adam(model.user_encoder.parameters(), lr=1e-2)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss, _ = TR.listwise_loss(model, nv, hist.numpy(), mask.numpy(), rows.numpy(), 0.7)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    assert losses[3] < losses[0] and all(math.isfinite(x) for x in losses), losses
