"""CPU: the host side of listwise training on served rows (include/nrhip.h, K19) -- metrics.row_logprob_grad_reference against
float64 torch autograd of the dense sequential statement (a logsumexp per step over what is left), the identity a = sum c, the
descriptor's place in nr_abi_sizes, the new names, and the refusals nr_row_logprob_grad makes before it launches anything (fake
non-null pointers: a launch would fault, a refusal does not), with the whole text of nr_last_error."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from newsrecommendation_amd import _lib, metrics, ops, train

INF, NAN = float("inf"), float("nan")
V, N, U = 60, 8, 6


def _case(k, seed):
    """Vectors, a prior with a -inf entry, ragged lists, rows with a fill entry in the middle (k > 1), an entry outside the pool, and
    user 4 whose row takes everything its lists leave eligible."""
    rng = np.random.default_rng(seed)
    news, user = rng.standard_normal((V, N)), rng.standard_normal((U, N)) / 2
    prior = 0.3 * rng.standard_normal(V)
    prior[7] = -INF
    lists = [rng.choice(np.arange(1, V), size=rng.integers(0, 20), replace=False) for _ in range(U)]
    rows = np.zeros((U, k), dtype=np.int64)
    for u in range(U):
        free = np.setdiff1d(np.arange(1, V), np.append(lists[u], 7))
        rows[u] = rng.choice(free, size=k, replace=False)
    if k > 1:
        rows[1, k // 2] = 0                                            # fill in the middle of a row
        rows[2, 0] = V + 3                                             # fill: out of range
        rows[3, k - 1] = 7                                             # outside the pool: no step, c = 0
    lists[4] = np.setdiff1d(np.arange(1, V), rows[4])                  # the row is everything eligible: an empty base
    g = rng.standard_normal((U, k))
    g[0, 0] = 0.0
    tau = np.linspace(0.3, 1.5, U)
    return news, user, prior, lists, rows, g, tau


def _dense(news, user, prior, lists, rows, g, tau):
    """float64 autograd of the dense statement: (d L / d user [U, N], d L / d news [V, N]), L = sum_u sum_j g_uj nll_uj, nll_uj = -(s_j / tau -
    logsumexp of s / tau over the base and the live entries j .. k-1)."""
    a = torch.tensor(news, requires_grad=True)
    b = torch.tensor(user, requires_grad=True)
    s = b @ a.T + torch.tensor(prior)[None, :]
    total = torch.zeros((), dtype=torch.float64)
    for u in range(U):
        rest = torch.ones(V, dtype=torch.bool)
        rest[0] = False
        rest[torch.isneginf(torch.tensor(prior))] = False
        live = [j for j in range(rows.shape[1]) if 1 <= rows[u, j] < V and bool(rest[rows[u, j]])]
        rest[torch.as_tensor(lists[u], dtype=torch.long)] = False
        rest[torch.as_tensor([r for r in rows[u] if 1 <= r < V], dtype=torch.long)] = False
        x = s[u] / tau[u]
        for n_j, j in enumerate(live):
            left = torch.cat([x[rest], x[torch.as_tensor([rows[u, i] for i in live[n_j:]], dtype=torch.long)]])
            total = total + g[u, j] * -(x[rows[u, j]] - torch.logsumexp(left, 0))
    total.backward()
    return b.grad.numpy(), a.grad.numpy()


def _from_coefficients(news, user, prior, lists, rows, tau, a, c):
    """The same two gradients from (a, c): (a E_rest - sum_i c_i news[i_i]) / tau and its news side, E_rest / p_rest the float64 softmax
    over the news of the base."""
    merged = [np.concatenate([lists[u], rows[u][(rows[u] >= 1) & (rows[u] < V)]]) for u in range(U)]
    p, _ = metrics.softmax_matrix_reference(news, user, temperature=tau, exclude=merged, prior=prior)
    gu = (a[:, None] * (p @ news)) / tau[:, None]
    gn = p.T @ ((a / tau)[:, None] * user)
    for u in range(U):
        for i in range(rows.shape[1]):
            if 1 <= rows[u, i] < V:
                gu[u] -= c[u, i] * news[rows[u, i]] / tau[u]
                gn[rows[u, i]] -= c[u, i] * user[u] / tau[u]
    return gu, gn


@pytest.mark.parametrize("k", [1, 2, 7])
def test_reference_coefficients_give_the_autograd_gradient_of_the_dense_statement(k):
    news, user, prior, lists, rows, g, tau = _case(k, seed=40 + k)
    merged = [np.concatenate([lists[u], rows[u]]) for u in range(U)]
    base = metrics.logz_reference(news, user, temperature=tau, exclude=merged, prior=prior)
    assert base[2][4] == 0 and base[1][4] == -INF and (base[2][:4] > 0).all()
    a, c = metrics.row_logprob_grad_reference(news, user, row_ids=rows, temperature=tau, base=base[:2], g=g, prior=prior)
    assert a.dtype == np.float64 and c.shape == (U, k)
    want_u, want_n = _dense(news, user, prior, lists, rows, g, tau)
    got_u, got_n = _from_coefficients(news, user, prior, lists, rows, tau, a, c)
    worst = max(float(np.abs(got_u - want_u).max()), float(np.abs(got_n - want_n).max()))
    print(f"k={k}: worst |gradient from (a, c) - autograd| = {worst:.3e}")
    assert worst <= 1e-12
    # a = sum_i c_i: adding one vector to every news changes no probability
    assert np.abs(a - c.sum(axis=1)).max() <= 1e-12
    # the special entries
    assert a[4] == 0.0 and (k == 1 or c[4].any())                      # an empty base: a = 0 exactly, the named terms stay
    if k > 1:
        assert c[1, k // 2] == 0.0 and c[2, 0] == 0.0 and c[3, k - 1] == 0.0
        g2 = g.copy()
        g2[1, k // 2], g2[2, 0], g2[3, k - 1] = 1e30, NAN, INF         # the g of what is no step is not looked at
        a2, c2 = metrics.row_logprob_grad_reference(news, user, row_ids=rows, temperature=tau, base=base[:2], g=g2, prior=prior)
        assert np.array_equal(a2, a) and np.array_equal(c2, c)
    # g = None is g = 1
    a1, c1 = metrics.row_logprob_grad_reference(news, user, row_ids=rows, temperature=tau, base=base[:2], prior=prior)
    ao, co = metrics.row_logprob_grad_reference(news, user, row_ids=rows, temperature=tau, base=base[:2], g=np.ones((U, k)), prior=prior)
    assert np.array_equal(a1, ao) and np.array_equal(c1, co)


def test_reference_dead_users_peaked_rows_and_the_logprob_it_differentiates():
    news, user, prior, lists, rows, g, tau = _case(7, seed=3)
    merged = [np.concatenate([lists[u], rows[u]]) for u in range(U)]
    taus = tau.copy()
    taus[0], taus[1], taus[2] = 0.0, NAN, INF
    base = metrics.logz_reference(news, user, temperature=taus, exclude=merged, prior=prior)
    bl = base[0].copy()
    bl[3] = NAN                                                        # a NaN base
    a, c = metrics.row_logprob_grad_reference(news, user, row_ids=rows, temperature=taus, base=(bl, base[1]), g=g, prior=prior)
    assert not a[:4].any() and not c[:4].any() and c[5].any() and a[5] != 0.0
    # a very peaked row stays finite and keeps a = sum c (every ratio is exp of a difference <= 0)
    a, c = metrics.row_logprob_grad_reference(news, 40.0 * user, row_ids=rows, temperature=1e-3,
                                              base=metrics.logz_reference(news, 40.0 * user, temperature=1e-3, exclude=merged, prior=prior)[:2],
                                              g=g, prior=prior)
    assert np.isfinite(a).all() and np.isfinite(c).all() and np.abs(a - c.sum(axis=1)).max() <= 1e-12 * np.abs(g).sum(axis=1).max()
    # finite differences of row_logprob_reference's own total in the score of one entry: d total / d s_i = c_i / tau with g = 1
    # (the row's nll is -total), with the base held fixed
    scores = user @ news.T
    base = metrics.logz_reference(scores, temperature=tau, exclude=merged, prior=prior)
    _, c = metrics.row_logprob_grad_reference(scores, row_ids=rows, temperature=tau, base=base[:2], prior=prior)
    u, i, h = 5, 3, 1e-6
    up, dn = scores.copy(), scores.copy()
    up[u, rows[u, i]] += h
    dn[u, rows[u, i]] -= h
    tp = metrics.row_logprob_reference(up, row_ids=rows, temperature=tau, base=base[:2], sequential=True, prior=prior)[1][u]
    tm = metrics.row_logprob_reference(dn, row_ids=rows, temperature=tau, base=base[:2], sequential=True, prior=prior)[1][u]
    assert abs((tp - tm) / (2 * h) - c[u, i] / tau[u]) <= 1e-7


def test_descriptor_is_entry_17_of_abi_sizes_and_the_new_names():
    sizes = (C.c_size_t * 18)()
    assert _lib.lib().nr_abi_sizes(sizes, 18) == 0 and sizes[17] == C.sizeof(_lib.LogprobGradDesc) and sizes[16] == C.sizeof(_lib.ExpectNewsDesc)
    assert len(list(sizes)) == 18 and all(sizes)
    seventeen = (C.c_size_t * 18)()
    seventeen[17] = 12345
    assert _lib.lib().nr_abi_sizes(seventeen, 17) == 0 and seventeen[17] == 12345 and list(seventeen)[:17] == list(sizes)[:17]
    assert "nr_row_logprob_grad" in _lib.SIGNATURES and hasattr(_lib.lib(), "nr_row_logprob_grad")
    # K14's fields without `sequential`, the shared tail of the row calls
    names = [f[0] for f in _lib.LogprobGradDesc._fields_]
    assert "sequential" not in names and names[-4:] == ["prior", "stamp", "window", "ld_window"] == [f[0] for f in _lib.LogprobDesc._fields_][-4:]
    assert names[:10] == [f[0] for f in _lib.LogprobDesc._fields_ if f[0] != "sequential"][:10]
    assert list(inspect.signature(ops.row_logprob_grad).parameters) == ["news_vecs", "user_vecs", "row_ids", "temperature", "base", "g", "prior",
                                                                        "stamp", "window"]
    assert list(inspect.signature(ops.plackett_luce_nll).parameters) == ["news_vecs", "user_vecs", "rows", "temperature", "exclude", "splits",
                                                                         "prior", "stamp", "window"]
    assert list(inspect.signature(train.listwise_loss).parameters) == ["model", "news_table", "hist_idx", "mask", "rows", "temperature", "weight",
                                                                       "exclude_history", "batch_size", "prior", "news_time", "window",
                                                                       "news_group", "group_cap", "seen"]
    kinds = inspect.signature(metrics.row_logprob_grad_reference).parameters
    assert list(kinds)[:2] == ["a", "b"] and all(kinds[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(kinds)[2:])


P = 4096                                                               # a fake pointer, 16-byte aligned
GRAD = dict(news_vecs=P, ld_news=400, V=100001, user=P, ld_user=400, U=8192, N=400, k=10, row_ids=P, ld_ids=10, tau=0.5, base_max=P,
            base_logsum=P, out_weight=P, out_sub_w=P)
# the whole text of nr_last_error; K14's wording under this call's name (the shared checks of csrc/nr_score_tile.h)
GRAD_REFUSED = [
    (dict(k=0), "row_logprob_grad: k = 0 entries per row, must be in [1, 128]"),
    (dict(k=129, ld_ids=129), "row_logprob_grad: k = 129 entries per row, must be in [1, 128]"),
    (dict(g=P, ld_g=9), "row_logprob_grad: g row stride 9 < k = 10"),
    (dict(out_weight=None), "row_logprob_grad: null pointer (news_vecs, user, row_ids, base_max, base_logsum, out_weight, out_sub_w)"),
    (dict(out_sub_w=None), "row_logprob_grad: null pointer (news_vecs, user, row_ids, base_max, base_logsum, out_weight, out_sub_w)"),
    (dict(tau=0.0), "row_logprob_grad: tau = 0, a scalar temperature must be finite and > 0"),
    (dict(tau=-0.5), "row_logprob_grad: tau = -0.5, a scalar temperature must be finite and > 0"),
    (dict(tau=NAN), "row_logprob_grad: tau = nan, a scalar temperature must be finite and > 0"),
    (dict(tau=INF), "row_logprob_grad: tau = inf, a scalar temperature must be finite and > 0"),
    (dict(V=1), "row_logprob_grad: V = 1 news rows; row 0 is the padding news, so at least 2 are needed"),
    (dict(U=0), "row_logprob_grad: U = 0 users"),
    (dict(N=402), "row_logprob_grad: vector width N = 402 must be a multiple of 4 in [4, 1024]"),
    (dict(stamp=P), "row_logprob_grad: stamp given without window (the two come together)"),
    (dict(window=P, ld_window=2), "row_logprob_grad: window given without stamp (the two come together)"),
    (dict(ld_ids=9), "row_logprob_grad: id row stride 9 < k = 10"),
    (dict(base_max=None), "row_logprob_grad: null pointer (news_vecs, user, row_ids, base_max, base_logsum, out_weight, out_sub_w)"),
    (dict(user=P + 8), "row_logprob_grad: rows must be 16-byte aligned (ld_news = 400, ld_user = 400: multiples of 4, >= N = 400)"),
]


@pytest.mark.parametrize("change,message", GRAD_REFUSED, ids=[f"{i}-{'-'.join(c)}" for i, (c, _) in enumerate(GRAD_REFUSED)])
def test_row_logprob_grad_refuses_before_any_launch(change, message):
    d = _lib.LogprobGradDesc(**{**GRAD, **change})
    assert _lib.lib().nr_row_logprob_grad(C.byref(d), None) == 1 and _lib.last_error() == message, _lib.last_error()


def test_null_descriptor_and_the_texts_are_k14s():
    assert _lib.lib().nr_row_logprob_grad(None, None) == 1 and _lib.last_error() == "row_logprob_grad: null descriptor"
    # the same rule broken in K14 gives the same sentence under K14's name
    k14 = dict(news_vecs=P, ld_news=400, V=100001, user=P, ld_user=400, U=8192, N=400, k=10, row_ids=P, ld_ids=10, sequential=1, tau=0.5,
               base_max=P, base_logsum=P, out_logp=P)
    for change in (dict(k=0), dict(tau=NAN), dict(V=1), dict(N=402), dict(stamp=P), dict(ld_ids=9), dict(user=P + 8)):
        assert _lib.lib().nr_row_logprob(C.byref(_lib.LogprobDesc(**{**k14, **change})), None) == 1
        said = _lib.last_error()
        assert _lib.lib().nr_row_logprob_grad(C.byref(_lib.LogprobGradDesc(**{**GRAD, **change})), None) == 1
        assert _lib.last_error() == said.replace("row_logprob:", "row_logprob_grad:"), (change, said)
    # a per-user tau replaces the scalar, which is then not looked at: the next rule answers
    d = _lib.LogprobGradDesc(**{**GRAD, "tau": NAN, "tau_u": P, "ld_ids": 9})
    assert _lib.lib().nr_row_logprob_grad(C.byref(d), None) == 1 and "id row stride" in _lib.last_error()


def test_no_cpu_fallback_no_caps_and_no_wide_rows():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.row_logprob_grad(torch.zeros(10, 8), torch.zeros(3, 8), torch.ones(3, 2, dtype=torch.int32), 0.5, (torch.zeros(3), torch.zeros(3)))
    with pytest.raises(RuntimeError, match="must be in \\[1, 128\\]"):
        ops.plackett_luce_nll(torch.zeros(10, 8), torch.zeros(3, 8), torch.ones(3, 129, dtype=torch.int32), 0.5)
    with pytest.raises(ValueError, match="group caps"):
        train.listwise_loss(None, None, None, None, None, 0.5, news_group=np.zeros(4))
    with pytest.raises(ValueError, match="group caps"):
        train.listwise_loss(None, None, None, None, None, 0.5, group_cap=2)
