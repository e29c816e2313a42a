"""CPU: the host side of the news-table gradient pass (include/nrhip.h, K18) -- metrics.expect_news_reference against a direct
fp64 softmax(scores / tau)^T-weighted sum of users and against the autograd gradient of a fp64 sum_u sum_t g_ut nll with respect
to the table, ExclusionLists.by_news against a brute-force transpose, the descriptor's place in nr_abi_sizes, the workspace
sizes, the refusals nr_score_expect_news makes before it launches anything (fake non-null pointers: a launch would fault, a
refusal does not), the new functions' parameter lists, and ops.full_softmax_nll still refusing a table that requires grad."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from newsrecommendation_amd import _lib, metrics, ops, train

INF, NAN = float("inf"), float("nan")
P = 4096                                                               # a fake pointer, 16-byte aligned


def _case(seed=5, nan_row=True):
    rng = np.random.default_rng(seed)
    U, V, N = 9, 41, 8
    news, user = rng.standard_normal((V, N)), rng.standard_normal((U, N))
    if nan_row:
        news[7, 3] = NAN                                               # a NaN row: NaN score for everybody
    prior = 0.3 * rng.standard_normal(V)
    prior[5] = -INF
    stamp = rng.integers(0, 10, V)
    window = np.stack([rng.integers(0, 4, U), rng.integers(5, 10, U)], axis=1)
    window[4] = (6, 2)                                                 # an empty window: a dead user
    exclude = [rng.choice(np.arange(0, V + 3), size=rng.integers(0, 12), replace=False) for _ in range(U)]   # ragged; 0 and >= V mean nothing
    return news, user, prior, stamp, window, exclude


def _eligible(u, news, user, prior, stamp, window, exclude):
    V = news.shape[0]
    return [v for v in range(1, V) if v not in set(exclude[u].tolist()) and prior[v] != -INF and not np.isnan(user[u] @ news[v] + prior[v])
            and window[u, 0] <= stamp[v] <= window[u, 1]]


def test_expect_news_reference_is_the_transposed_softmax_times_the_users():
    news, user, prior, stamp, window, exclude = _case()
    U, V, N = user.shape[0], news.shape[0], news.shape[1]
    tau = np.linspace(0.2, 3.0, U)
    tau[2] = 0.0                                                       # a dead user
    w = np.linspace(-1.0, 2.0, U)
    kw = dict(temperature=tau, exclude=exclude, prior=prior, stamp=stamp, window=window)
    out, mass = metrics.expect_news_reference(news, user, weight=w, **kw)
    scaled, mass_s = metrics.expect_news_reference(news, user, weight=w, scale_inv_tau=True, **kw)
    assert out.dtype == np.float64 and out.shape == (V, N) and mass.shape == (V,)
    want, want_s, want_m = np.zeros((V, N)), np.zeros((V, N)), np.zeros(V)
    for u in range(U):
        el = _eligible(u, news, user, prior, stamp, window, exclude)
        if not el or u == 2:
            assert u in (2, 4)
            continue
        p = torch.softmax(torch.tensor((news[el] @ user[u] + prior[el]) / tau[u], dtype=torch.float64), 0).numpy()
        want[el] += w[u] * p[:, None] * user[u][None, :]
        want_s[el] += w[u] / tau[u] * p[:, None] * user[u][None, :]
        want_m[el] += w[u] * p
    np.testing.assert_allclose(out, want, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(scaled, want_s, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(mass, want_m, rtol=1e-12, atol=1e-14)
    assert np.array_equal(mass, mass_s)                                # the mass never carries 1 / tau
    assert not out[0].any() and not out[7].any() and not out[5].any() and mass[0] == mass[7] == mass[5] == 0.0
    # weight None = 1: the masses of the live users add up to their number
    _, m1 = metrics.expect_news_reference(news, user, **kw)
    assert abs(m1.sum() - (U - 2)) <= 1e-12
    # named terms: subtracted per news, dead users and zero weights skipped, 1 / tau only under scale_inv_tau
    off = np.zeros(V + 1, dtype=np.int64)
    off[4:] = 3
    off[10:] = 5
    named = (off, np.array([0, 2, 1, 4, 3]), np.array([0.5, 7.0, -2.0, 3.0, 0.0]))     # news 3: users 0, 2 (dead), 1; news 9: 4 (dead), 3 (w = 0)
    o2, m2 = metrics.expect_news_reference(news, user, weight=w, named=named, scale_inv_tau=True, **kw)
    d = np.zeros((V, N))
    d[3] = 0.5 / tau[0] * user[0] - 2.0 / tau[1] * user[1]
    np.testing.assert_allclose(o2, want_s - d, rtol=1e-12, atol=1e-14)
    assert np.array_equal(m2, mass)
    o3, _ = metrics.expect_news_reference(news, user, weight=w, named=named, **kw)
    d[3] = 0.5 * user[0] - 2.0 * user[1]
    np.testing.assert_allclose(o3, want - d, rtol=1e-12, atol=1e-14)
    # a user component that is not finite counts as 0
    user2 = user.copy()
    user2[6, 1] = INF
    o4, _ = metrics.expect_news_reference(news, user2, weight=w, **kw)
    assert np.isfinite(o4).all()


def test_expect_news_reference_is_the_gradient_of_the_weighted_nll_with_respect_to_the_table():
    """d/d news of sum_u sum_t g_ut nll(u, t) in float64 autograd = expect_news_reference with weight = sum_t g, scale_inv_tau and
    the valid targets as named terms (ops._named_by_news): pools, lists, fill targets and a dead user."""
    news, user, prior, stamp, window, exclude = _case(seed=8, nan_row=False)
    U, V, N = user.shape[0], news.shape[0], news.shape[1]
    rng = np.random.default_rng(3)
    tau = np.linspace(0.4, 1.5, U)
    T = 4
    targets = rng.integers(1, V, (U, T))
    targets[:, 1] = 0                                                  # fill
    targets[::2, 2] = V + 2                                            # fill: out of range
    targets[1, 3] = targets[1, 0]                                      # a repeat: two entries
    targets[:, 0] = np.where(np.arange(U) % 3 == 0, 12, targets[:, 0])  # one news named by several users
    g = rng.standard_normal((U, T)).astype(np.float32).astype(np.float64)       # fp32 values: the named weights are fp32
    tab = torch.tensor(news, dtype=torch.float64, requires_grad=True)
    total = torch.zeros((), dtype=torch.float64)
    gw = np.zeros((U, T))
    for u in range(U):
        el = _eligible(u, news, user, prior, stamp, window, exclude)
        if not el:
            assert u == 4                                              # the dead user: no term, no named term
            continue
        uv = torch.tensor(user[u])
        logz = torch.logsumexp((tab[el] @ uv + torch.tensor(prior[el])) / tau[u], 0)
        for t in range(T):
            v = int(targets[u, t])
            if 1 <= v < V:                                             # a target's own eligibility is the caller's statement, as in row_logprob
                total = total + g[u, t] * (logz - (tab[v] @ uv + prior[v]) / tau[u])
                gw[u, t] = g[u, t]
    (grad,) = torch.autograd.grad(total, tab)
    named = ops._named_by_news(torch.tensor(targets, dtype=torch.int32), torch.tensor(gw, dtype=torch.float32), V)
    # stable: within a news the entries come (user, t) ascending
    off, nu = named[0].numpy(), named[1].numpy()
    assert off[0] == 0 and off[-1] == len(nu) == int((gw != 0).sum()) and all(np.all(np.diff(nu[off[v]:off[v + 1]]) >= 0) for v in range(V))
    assert off[13] - off[12] >= 3 and off[1] == 0
    out, _ = metrics.expect_news_reference(news, user, temperature=tau, exclude=exclude, prior=prior, stamp=stamp, window=window,
                                           weight=gw.sum(axis=1), named=(off, nu, named[2].double().numpy()), scale_inv_tau=True)
    np.testing.assert_allclose(out, grad.numpy(), rtol=1e-10, atol=1e-12)
    assert not out[0].any()


def test_by_news_is_the_transpose_of_the_lists():
    V = 23
    raw = [[3, 3, 7, 0, 22, 23, 40], [], [7, 1, 22], [], [1, 2, 3, 4, 5, 6, 7], [0, 0], [22]]     # user 0 has entries; empty lists; ids >= V
    lists = ops.ExclusionLists([torch.tensor(r, dtype=torch.int64) for r in raw])
    off, users = lists.by_news(V)
    assert off.dtype == torch.int32 and users.dtype == torch.int32 and off.shape == (V + 1,)
    brute = [[u for u, r in enumerate(raw) if v in r and v >= 1] for v in range(V)]
    assert int(off[0]) == 0 and int(off[-1]) == sum(len(b) for b in brute) == users.numel()
    for v in range(V):
        assert users[int(off[v]):int(off[v + 1])].tolist() == brute[v], v
    assert brute[3] == [0, 4] and brute[22] == [0, 2, 6] and brute[0] == []
    # nothing at all
    off0, users0 = ops.ExclusionLists([torch.zeros(0, dtype=torch.int64)] * 3).by_news(5)
    assert off0.tolist() == [0] * 6 and users0.numel() == 0
    # V below every id: everything is dropped
    off1, users1 = lists.by_news(1)
    assert off1.tolist() == [0, 0] and users1.numel() == 0


BASE = dict(news_vecs=P, ld_news=400, V=100001, user=P, ld_user=400, U=8192, N=400, tau=0.5, base_max=P, base_logsum=P, out=P, ld_out=400)


def _refusal(**fields):
    """(size query's answer, return code of the call, nr_last_error after it); the workspace is what the unbroken descriptor asks for."""
    lib = _lib.lib()
    short = fields.pop("short_ws", False)
    d = _lib.ExpectNewsDesc(**dict(BASE, **fields))
    size = lib.nr_score_expect_news_workspace_bytes(C.byref(d))
    need = lib.nr_score_expect_news_workspace_bytes(C.byref(_lib.ExpectNewsDesc(**BASE)))
    d.ws, d.ws_bytes = P, need - 8 if short else need
    rc = lib.nr_score_expect_news(C.byref(d), None)
    return size, rc, _lib.last_error()


REFUSED = {
    "V=1": (dict(V=1), "score_expect_news: V = 1 news rows; row 0 is the padding news, so at least 2 are needed"),
    "U=0": (dict(U=0), "score_expect_news: U = 0 users"),
    "N=6": (dict(N=6), "score_expect_news: vector width N = 6 must be a multiple of 4 in [4, 1024]"),
    "n_excl<0": (dict(n_excl=-1), "score_expect_news: n_excl = -1 entries of excl_users, must be >= 0"),
    "users-alone": (dict(excl_users=P, n_excl=5), "score_expect_news: excl_users given without excl_offsets (n_excl = 5; the two come together)"),
    "offsets-alone": (dict(excl_offsets=P, n_excl=5), "score_expect_news: excl_offsets given without excl_users (n_excl = 5; the two come together)"),
    "tau=0": (dict(tau=0.0), "score_expect_news: tau = 0, a scalar temperature must be finite and > 0"),
    "splits=65": (dict(splits=65), "score_expect_news: splits = 65, must be 0 (library's choice) or in [1, 64], the segments of U = 8192"),
    "splits<0": (dict(splits=-1), "score_expect_news: splits = -1, must be 0 (library's choice) or in [1, 64], the segments of U = 8192"),
    "stamp-alone": (dict(stamp=P), "score_expect_news: stamp given without window (the two come together)"),
    "window-alone": (dict(window=P, ld_window=2), "score_expect_news: window given without stamp (the two come together)"),
    "ld_window=1": (dict(stamp=P, window=P, ld_window=1), "score_expect_news: ld_window = 1, a window row is (lo, hi): at least 2"),
    "no-output": (dict(out=None), "score_expect_news: out and out_mass are both null (at least one output is needed)"),
}
NAMED = "score_expect_news: named_offsets, named_user and named_w come together (all three or none)"
CALL_ONLY = {
    "null-base_max": (dict(base_max=None), "score_expect_news: null pointer (news_vecs, user, base_max, base_logsum)"),
    "null-base_logsum": (dict(base_logsum=None), "score_expect_news: null pointer (news_vecs, user, base_max, base_logsum)"),
    "null-user": (dict(user=None), "score_expect_news: null pointer (news_vecs, user, base_max, base_logsum)"),
    "named-offsets-alone": (dict(named_offsets=P), NAMED),
    "named-user-alone": (dict(named_user=P, n_named=3), NAMED),
    "named-w-alone": (dict(named_w=P, n_named=3), NAMED),
    "named-without-w": (dict(named_offsets=P, named_user=P, n_named=3), NAMED),
    "named-without-offsets": (dict(named_user=P, named_w=P, n_named=3), NAMED),
    "n_named<0": (dict(named_offsets=P, named_user=P, named_w=P, n_named=-2), "score_expect_news: n_named = -2 named terms, must be >= 0"),
    "ld_news=N+1": (dict(ld_news=401), "score_expect_news: rows must be 16-byte aligned (ld_news = 401, ld_user = 400: multiples of 4, >= N = 400)"),
    "user-misaligned": (dict(user=P + 4), "score_expect_news: rows must be 16-byte aligned (ld_news = 400, ld_user = 400: multiples of 4, >= N = 400)"),
    "ld_out<N": (dict(ld_out=396), "score_expect_news: out must be 16-byte aligned with ld_out = 396 >= N = 400"),
    "out-misaligned": (dict(out=P + 4), "score_expect_news: out must be 16-byte aligned with ld_out = 400 >= N = 400"),
    "short-workspace": (dict(short_ws=True),
                        "score_expect_news: workspace holds 160801600 bytes, nr_score_expect_news_workspace_bytes asks for 160801608 (8-byte aligned)"),
}


@pytest.mark.parametrize("rule", list(REFUSED), ids=str)
def test_bad_descriptor_is_refused_by_the_size_query_and_the_call(rule):
    fields, text = REFUSED[rule]
    assert _refusal(**fields) == (0, 1, text)


@pytest.mark.parametrize("rule", list(CALL_ONLY), ids=str)
def test_bad_call_is_refused_before_any_launch(rule):
    fields, text = CALL_ONLY[rule]
    size, rc, said = _refusal(**fields)
    assert (rc, said) == (1, text) and size > 0


def test_first_refusal_wins_and_null_descriptor():
    assert _refusal(V=1, N=6)[2] == REFUSED["V=1"][1]
    assert _refusal(splits=65, out=None)[2] == REFUSED["splits=65"][1]
    assert _refusal(ld_news=401, short_ws=True)[2] == CALL_ONLY["ld_news=N+1"][1]
    assert _refusal(base_max=None, named_w=P)[2] == CALL_ONLY["null-base_max"][1]
    lib = _lib.lib()
    assert lib.nr_score_expect_news_workspace_bytes(None) == 0 and lib.nr_score_expect_news(None, None) == 1
    assert _lib.last_error() == "score_expect_news: null descriptor"


def _ws(N, V, U, splits, rows=True):
    d = _lib.ExpectNewsDesc(**dict(BASE, ld_news=N, ld_user=N, ld_out=N, N=N, U=U, V=V, splits=splits, out=P if rows else None, out_mass=P))
    return _lib.lib().nr_score_expect_news_workspace_bytes(C.byref(d))


def test_workspace_is_one_row_and_one_mass_per_news_and_slice():
    """V * slices * (N * 4 + 8) bytes, V * slices * 8 in the mass-only mode.  The news tile is K17's user tile: 64 up to N = 352, 32 up
    to N = 832, then 16; the library's slice count fills 256 CUs with news tiles and is at most the segments of U (128 users each
    up to U = 32 768)."""
    per = lambda N, V, s: V * s * (N * 4 + 8)
    assert _ws(400, 100001, 8192, 0) == per(400, 100001, 1)            # 3 126 tiles of 32 news
    assert _ws(400, 100001, 8192, 0, rows=False) == 100001 * 8
    assert _ws(400, 34, 8192, 0) == per(400, 34, 64)                   # 2 tiles -> 128 slices asked, 64 segments
    assert _ws(352, 4096, 8192, 0) == per(352, 4096, 4)                # 64 tiles of 64 news
    assert _ws(356, 4096, 8192, 0) == per(356, 4096, 2)                # 128 tiles of 32
    assert _ws(832, 1024, 8192, 0) == per(832, 1024, 8)                # 32 tiles of 32
    assert _ws(836, 1024, 8192, 0) == per(836, 1024, 4)                # 64 tiles of 16
    assert _ws(400, 294, 300, 2) == per(400, 294, 2) and _ws(400, 294, 300, 3) == per(400, 294, 3)
    assert _ws(400, 294, 300, 3, rows=False) == 294 * 3 * 8
    assert _ws(4, 2, 1, 0) == per(4, 2, 1) and _ws(4, 130, 294, 3) == per(4, 130, 3)
    assert _ws(4, 70, 128 * 256 + 5, 2) == per(4, 70, 2)               # 129 segments of 256 users in 2 slices
    assert _ws(4, 70, 128 * 256 + 5, 0) == per(4, 70, 65)              # 2 tiles -> 128 asked -> 65 slices of 2 segments
    assert _ws(400, 130, 129, 3) == 0                                  # 2 segments: 3 slices are refused


def test_descriptor_is_entry_16_of_abi_sizes_and_the_new_names_exist():
    sizes = (C.c_size_t * 17)()
    assert _lib.lib().nr_abi_sizes(sizes, 17) == 0 and sizes[16] == C.sizeof(_lib.ExpectNewsDesc) and sizes[15] == C.sizeof(_lib.ExpectDesc)
    sixteen = (C.c_size_t * 17)(*([12345] * 17))
    assert _lib.lib().nr_abi_sizes(sixteen, 16) == 0 and sixteen[16] == 12345 and list(sixteen)[:16] == list(sizes)[:16]
    pools = ("prior", "stamp", "window")
    for fn, names in ((metrics.expect_news_reference, ("a", "b", "temperature", "exclude") + pools + ("weight", "named", "scale_inv_tau")),
                      (ops.ExclusionLists.by_news, ("self", "V")),
                      (ops.score_expect_news, ("news_vecs", "user_vecs", "temperature", "base", "exclude", "splits") + pools + ("weight", "rows")),
                      (ops.full_softmax_nll_joint, ("news_vecs", "user_vecs", "targets", "temperature", "exclude", "splits") + pools),
                      (ops.news_gather, ("table", "ids", "code")),
                      (train.full_softmax_loss_joint, ("model", "news_table", "hist_idx", "mask", "targets", "temperature", "exclude_history",
                                                       "batch_size", "prior", "news_time", "window", "seen")),
                      (train.expected_exposure, ("model", "news_vecs", "hist_idx", "mask", "temperature", "exclude_history", "batch_size", "prior",
                                                 "news_time", "window", "seen"))):
        assert tuple(inspect.signature(fn).parameters) == names, fn
    sig = inspect.signature(metrics.expect_news_reference).parameters
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[2:]) and sig["scale_inv_tau"].default is False
    assert inspect.signature(ops.score_expect_news).parameters["rows"].default is True


def test_full_softmax_nll_still_refuses_a_table_that_requires_grad():
    news = torch.randn(10, 8, requires_grad=True)
    user = torch.randn(3, 8, requires_grad=True)
    targets = torch.ones(3, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"news_vecs requires grad.*P\^T \. users.*\[V, N\] reduction over every user.*not part of this call"):
        ops.full_softmax_nll(news, user, targets, 0.5)
