"""CPU: the host side of the entropy passes (include/nrhip.h, K23 and K24) -- metrics.entropy_reference and
metrics.expect_affine_reference against a dense float64 statement written out here (pools, lists, per-user temperatures, bad
entries), the identities dH / duser = -(J + H E) / tau, dH / dtau = Var_p(log p) / tau and dnll / dtau = (log p_t + H) / tau against
float64 autograd of that statement, the descriptors' places in nr_abi_sizes, the workspace sizes and the refusals the two calls
make before they launch anything (fake non-null pointers: a launch would fault, a refusal does not)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from newsrecommendation_amd import _lib, metrics, ops, train

INF, NAN = float("inf"), float("nan")
P = 4096                                                               # a fake pointer, 16-byte aligned


def _case(seed=5):
    rng = np.random.default_rng(seed)
    U, V, N = 9, 41, 8
    news, user = rng.standard_normal((V, N)), rng.standard_normal((U, N))
    news[7, 3] = NAN                                                   # a NaN row: NaN score for everybody
    prior = 0.3 * rng.standard_normal(V)
    prior[5], prior[9] = -INF, NAN
    stamp = rng.integers(0, 10, V)
    window = np.stack([rng.integers(0, 4, U), rng.integers(5, 10, U)], axis=1)
    window[4] = (6, 2)                                                 # an empty window
    exclude = [rng.choice(np.arange(0, V + 3), size=rng.integers(0, 12), replace=False) for _ in range(U)]   # ragged; 0 and >= V mean nothing
    return news, user, prior, stamp, window, exclude


def _eligible(u, news, user, prior, stamp, window, exclude):
    V = news.shape[0]
    return [v for v in range(1, V) if v not in set(exclude[u].tolist()) and prior[v] != -INF and not np.isnan(user[u] @ news[v] + prior[v])
            and window[u, 0] <= stamp[v] <= window[u, 1]]


def _dense(news_el, prior_el, uv, tau):
    """The dense statement for one user: (log p [n], p [n]) as float64 torch tensors with a graph to uv and tau."""
    logp = torch.log_softmax((torch.as_tensor(news_el) @ uv + torch.as_tensor(prior_el)) / tau, 0)
    return logp, logp.exp()


def test_entropy_reference_is_the_dense_statement():
    news, user, prior, stamp, window, exclude = _case()
    U = user.shape[0]
    tau = np.linspace(0.2, 3.0, U)
    kw = dict(exclude=exclude, prior=prior, stamp=stamp, window=window)
    H, var, mass = metrics.entropy_reference(news, user, tau, **kw)
    assert H.dtype == np.float64 and H.shape == var.shape == mass.shape == (U,)
    seen_empty = False
    for u in range(U):
        el = _eligible(u, news, user, prior, stamp, window, exclude)
        if not el:
            seen_empty = True
            assert u == 4 and (H[u], var[u], mass[u]) == (0.0, 0.0, 0.0)
            continue
        assert 7 not in el
        lp, p = _dense(news[el], prior[el], torch.tensor(user[u]), float(tau[u]))
        np.testing.assert_allclose(H[u], float(-(p * lp).sum()), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(var[u], float((p * lp * lp).sum() - (p * lp).sum() ** 2), rtol=1e-10, atol=1e-13)
        assert abs(mass[u] - 1.0) <= 1e-14
    assert seen_empty
    # a bad temperature: that user alone is NaN, unless it has nothing eligible
    bad = tau.copy()
    bad[1], bad[2], bad[4] = 0.0, INF, NAN
    H2, var2, mass2 = metrics.entropy_reference(news, user, bad, **kw)
    assert np.isnan([H2[1], var2[1], mass2[1], H2[2], var2[2], mass2[2]]).all() and (H2[4], var2[4], mass2[4]) == (0.0, 0.0, 0.0)
    keep = [u for u in range(U) if u not in (1, 2, 4)]
    assert np.array_equal(H2[keep], H[keep]) and np.array_equal(var2[keep], var[keep])
    # exactly one eligible news: (0, 0, 1)
    one = [np.array([v for v in range(1, news.shape[0]) if v != 3]) for _ in range(U)]
    H3, var3, mass3 = metrics.entropy_reference(news, user, 0.5, exclude=one)
    assert not H3.any() and not var3.any() and (mass3 == 1.0).all()
    # a score of -inf under a finite maximum (a news row of -inf against positive users): 0 log 0 = 0, the others as without it
    low = news.copy()
    low[7, 3] = 0.5
    low[12] = -INF
    pos = np.abs(user)
    H4, var4, mass4 = metrics.entropy_reference(low, pos, 0.5)
    H5, var5, mass5 = metrics.entropy_reference(low, pos, 0.5, exclude=[[12]] * U)
    assert np.isfinite(H4).all() and np.allclose(H4, H5, rtol=1e-13) and np.allclose(var4, var5, rtol=1e-12) and np.allclose(mass4, 1.0)


def test_expect_affine_reference_is_the_dense_statement():
    news, user, prior, stamp, window, exclude = _case(seed=6)
    U, V = user.shape[0], news.shape[0]
    rng = np.random.default_rng(3)
    tau = np.linspace(0.3, 2.0, U)
    alpha, beta = rng.standard_normal(U), rng.standard_normal(U)
    ids = rng.integers(0, V + 2, (U, 4))
    ids[:, 3] = ids[:, 0]
    sw = rng.standard_normal((U, 4))
    kw = dict(exclude=exclude, prior=prior, stamp=stamp, window=window)
    plain, mass = metrics.expect_affine_reference(news, user, tau, **kw)
    E, m = metrics.expect_reference(news, user, temperature=tau, **kw)
    np.testing.assert_allclose(plain, E, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(mass, m, rtol=1e-14, atol=0)
    out, _ = metrics.expect_affine_reference(news, user, tau, alpha=alpha, beta=beta, sub_ids=ids, sub_w=sw, scale_inv_tau=True, **kw)
    clean = np.where(np.isfinite(news), news, 0.0)
    for u in range(U):
        el = _eligible(u, news, user, prior, stamp, window, exclude)
        real = (ids[u] >= 1) & (ids[u] < V)
        sub = sw[u][real] @ clean[ids[u][real]]
        if not el:
            np.testing.assert_allclose(out[u], -sub / tau[u], rtol=1e-12, atol=1e-14)
            continue
        lp, p = _dense(news[el], prior[el], torch.tensor(user[u]), float(tau[u]))
        want = ((p * (alpha[u] + beta[u] * lp)).numpy() @ clean[el] - sub) / tau[u]
        np.testing.assert_allclose(out[u], want, rtol=1e-11, atol=1e-13)
    bad = tau.copy()
    bad[1] = -1.0
    o2, m2 = metrics.expect_affine_reference(news, user, bad, alpha=alpha, beta=beta, **kw)
    assert np.isnan(o2[1]).all() and np.isnan(m2[1]) and not np.isnan(o2[[0, 2, 3]]).any()


def test_the_gradient_identities_against_float64_autograd():
    """dH / duser = -(J + H E) / tau (expect_affine_reference with alpha = -H, beta = -1, scale_inv_tau), dH / dtau = var / tau,
    d nll_t / d tau = (log p_t + H) / tau, and the whole user gradient of L = sum_t g_t nll_t + h H as ONE affine contraction."""
    news, user, prior, stamp, window, exclude = _case(seed=8)
    news[7, 3] = 0.5                                                   # autograd has no NaN rule
    U, V = user.shape[0], news.shape[0]
    rng = np.random.default_rng(4)
    tau = np.linspace(0.4, 1.5, U)
    kw = dict(exclude=exclude, prior=prior, stamp=stamp, window=window)
    H, var, _ = metrics.entropy_reference(news, user, tau, **kw)
    dH, _ = metrics.expect_affine_reference(news, user, tau, alpha=-H, beta=-np.ones(U), scale_inv_tau=True, **kw)
    g, h = rng.standard_normal((U, 3)), rng.standard_normal(U)
    checked = 0
    for u in range(U):
        el = _eligible(u, news, user, prior, stamp, window, exclude)
        if len(el) < 3:
            continue
        uv = torch.tensor(user[u], requires_grad=True)
        t = torch.tensor(float(tau[u]), dtype=torch.float64, requires_grad=True)
        lp, p = _dense(news[el], prior[el], uv, t)
        ent = -(p * lp).sum()
        gu, gt = torch.autograd.grad(ent, (uv, t), retain_graph=True)
        np.testing.assert_allclose(dH[u], gu.numpy(), rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(var[u] / tau[u], float(gt), rtol=1e-9, atol=1e-12)
        picks = rng.choice(len(el), 3, replace=False)
        for j in picks:
            (gt_nll,) = torch.autograd.grad(-lp[j], t, retain_graph=True)
            np.testing.assert_allclose((float(lp[j].detach()) + H[u]) / tau[u], float(gt_nll), rtol=1e-9, atol=1e-12)
        loss = -(torch.tensor(g[u]) * lp[picks]).sum() + h[u] * ent
        (gl,) = torch.autograd.grad(loss, uv)
        ids = np.asarray(el)[picks][None, :]
        one, _ = metrics.expect_affine_reference(news, user[u:u + 1], tau[u], exclude=[exclude[u]], prior=prior, stamp=stamp, window=window[u:u + 1],
                                                 alpha=np.array([g[u].sum() - h[u] * H[u]]), beta=np.array([-h[u]]), sub_ids=ids, sub_w=g[u][None, :],
                                                 scale_inv_tau=True)
        np.testing.assert_allclose(one[0], gl.numpy(), rtol=1e-9, atol=1e-12)
        checked += 1
    assert checked >= 6


E_BASE = dict(news_vecs=P, ld_news=400, V=100001, user=P, ld_user=400, U=8192, N=400, tau=0.5, base_max=P, base_logsum=P, out_entropy=P)
A_BASE = dict(news_vecs=P, ld_news=400, V=100001, user=P, ld_user=400, U=8192, N=400, tau=0.5, base_max=P, base_logsum=P, out=P, ld_out=400)
CALLS = {"score_entropy": (_lib.EntropyDesc, E_BASE, "nr_score_entropy"), "score_expect_affine": (_lib.ExpectAffineDesc, A_BASE, "nr_score_expect_affine")}


def _refusal(what, **fields):
    """(size query's answer, return code of the call, nr_last_error after it); the workspace is what the unbroken descriptor asks for."""
    lib = _lib.lib()
    desc, base, fn = CALLS[what]
    short = fields.pop("short_ws", False)
    d = desc(**dict(base, **fields))
    size = getattr(lib, fn + "_workspace_bytes")(C.byref(d))
    need = getattr(lib, fn + "_workspace_bytes")(C.byref(desc(**base)))
    d.ws, d.ws_bytes = P, need - 8 if short else need
    rc = getattr(lib, fn)(C.byref(d), None)
    return size, rc, _lib.last_error()


REFUSED = {
    "V=1": (dict(V=1), "{}: V = 1 news rows; row 0 is the padding news, so at least 2 are needed"),
    "U=0": (dict(U=0), "{}: U = 0 users"),
    "N=6": (dict(N=6), "{}: vector width N = 6 must be a multiple of 4 in [4, 1024]"),
    "stamp-alone": (dict(stamp=P), "{}: stamp given without window (the two come together)"),
    "window-alone": (dict(window=P, ld_window=2), "{}: window given without stamp (the two come together)"),
    "ld_window=1": (dict(stamp=P, window=P, ld_window=1), "{}: ld_window = 1, a window row is (lo, hi): at least 2"),
    "ids-alone": (dict(excl_ids=P, n_excl=5), "{}: excl_ids given without excl_offsets (n_excl = 5; the two come together)"),
    "offsets-alone": (dict(excl_offsets=P, n_excl=5), "{}: excl_offsets given without excl_ids (n_excl = 5; the two come together)"),
    "tau=0": (dict(tau=0.0), "{}: tau = 0, a scalar temperature must be finite and > 0"),
    "splits=257": (dict(splits=257), "{}: splits = 257, must be 0 (library's choice) or in [1, 196], the segments of V = 100001"),
}
ENTROPY_CALL_ONLY = {
    "null-base_max": (dict(base_max=None), "score_entropy: null pointer (news_vecs, user, base_max, base_logsum, out_entropy)"),
    "null-base_logsum": (dict(base_logsum=None), "score_entropy: null pointer (news_vecs, user, base_max, base_logsum, out_entropy)"),
    "null-out_entropy": (dict(out_entropy=None), "score_entropy: null pointer (news_vecs, user, base_max, base_logsum, out_entropy)"),
    "ld_news=N+1": (dict(ld_news=401), "score_entropy: rows must be 16-byte aligned (ld_news = 401, ld_user = 400: multiples of 4, >= N = 400)"),
    "user-misaligned": (dict(user=P + 4), "score_entropy: rows must be 16-byte aligned (ld_news = 400, ld_user = 400: multiples of 4, >= N = 400)"),
    "short-workspace": (dict(short_ws=True), "score_entropy: workspace holds 393208 bytes, nr_score_entropy_workspace_bytes asks for 393216 (8-byte aligned)"),
}
AFFINE_CALL_ONLY = {
    "null-base_max": (dict(base_max=None), "score_expect_affine: null pointer (news_vecs, user, base_max, base_logsum, out)"),
    "null-out": (dict(out=None), "score_expect_affine: null pointer (news_vecs, user, base_max, base_logsum, out)"),
    "ids-without-w": (dict(sub_ids=P, T=4, ld_sub=4), "score_expect_affine: sub_ids given without sub_w (the two come together)"),
    "w-without-ids": (dict(sub_w=P, T=4, ld_sub=4), "score_expect_affine: sub_w given without sub_ids (the two come together)"),
    "T=0": (dict(sub_ids=P, sub_w=P, T=0, ld_sub=4),
            "score_expect_affine: T = 0 named rows per user (row stride 4), must be in [1, 128] with ld_sub >= T"),
    "T=129": (dict(sub_ids=P, sub_w=P, T=129, ld_sub=129),
              "score_expect_affine: T = 129 named rows per user (row stride 129), must be in [1, 128] with ld_sub >= T"),
    "ld_sub<T": (dict(sub_ids=P, sub_w=P, T=8, ld_sub=4),
                 "score_expect_affine: T = 8 named rows per user (row stride 4), must be in [1, 128] with ld_sub >= T"),
    "ld_news=N+1": (dict(ld_news=401), "score_expect_affine: rows must be 16-byte aligned (ld_news = 401, ld_user = 400: multiples of 4, >= N = 400)"),
    "ld_out<N": (dict(ld_out=396), "score_expect_affine: out must be 16-byte aligned with ld_out = 396 >= N = 400"),
    "out-misaligned": (dict(out=P + 4), "score_expect_affine: out must be 16-byte aligned with ld_out = 400 >= N = 400"),
    "short-workspace": (dict(short_ws=True), "score_expect_affine: workspace holds 13172728 bytes, nr_score_expect_affine_workspace_bytes asks for "
                                             "13172736 (8-byte aligned)"),
}


@pytest.mark.parametrize("what", list(CALLS))
@pytest.mark.parametrize("rule", list(REFUSED), ids=str)
def test_bad_descriptor_is_refused_by_the_size_query_and_the_call(what, rule):
    fields, text = REFUSED[rule]
    assert _refusal(what, **fields) == (0, 1, text.format(what))


@pytest.mark.parametrize("rule", list(ENTROPY_CALL_ONLY), ids=str)
def test_bad_entropy_call_is_refused_before_any_launch(rule):
    fields, text = ENTROPY_CALL_ONLY[rule]
    size, rc, said = _refusal("score_entropy", **fields)
    assert (rc, said) == (1, text) and size > 0


@pytest.mark.parametrize("rule", list(AFFINE_CALL_ONLY), ids=str)
def test_bad_affine_call_is_refused_before_any_launch(rule):
    fields, text = AFFINE_CALL_ONLY[rule]
    size, rc, said = _refusal("score_expect_affine", **fields)
    assert (rc, said) == (1, text) and size > 0


def test_null_descriptors_and_first_refusal_wins():
    lib = _lib.lib()
    for what, (_, _, fn) in CALLS.items():
        assert getattr(lib, fn + "_workspace_bytes")(None) == 0 and getattr(lib, fn)(None, None) == 1
        assert _lib.last_error() == f"{what}: null descriptor"
        assert _refusal(what, V=1, N=6)[2] == REFUSED["V=1"][1].format(what)


def test_workspace_sizes():
    """K23: one fp64 triple per (user, slice), the slices of score_logz's plan (user tiles of 64 up to N = 400 ...); K24: K17's size."""
    lib = _lib.lib()
    en = lambda N, U, V, s: lib.nr_score_entropy_workspace_bytes(C.byref(_lib.EntropyDesc(**dict(E_BASE, ld_news=N, ld_user=N, N=N, U=U, V=V, splits=s))))
    af = lambda N, U, V, s: lib.nr_score_expect_affine_workspace_bytes(
        C.byref(_lib.ExpectAffineDesc(**dict(A_BASE, ld_news=N, ld_user=N, ld_out=N, N=N, U=U, V=V, splits=s))))
    ex = lambda N, U, V, s: lib.nr_score_expect_workspace_bytes(
        C.byref(_lib.ExpectDesc(**dict(A_BASE, ld_news=N, ld_user=N, ld_out=N, N=N, U=U, V=V, splits=s))))
    assert en(400, 70, 100001, 3) == 70 * 3 * 24 and en(400, 1, 100001, 0) == 196 * 24 and en(4, 1, 2, 0) == 24
    assert en(4, 3, 1 + 128 * 256 + 5, 2) == 3 * 2 * 24 and en(400, 65, 130, 3) == 0
    for shape in ((400, 8192, 100001, 0), (352, 8192, 100001, 0), (832, 64, 100001, 0), (836, 64, 100001, 0), (400, 1, 100001, 0), (400, 70, 100001, 3),
                  (4, 1, 130, 2), (400, 65, 130, 3)):
        assert af(*shape) == ex(*shape), shape


def test_descriptors_are_entries_21_and_22_of_abi_sizes_and_the_new_names_exist():
    sizes = (C.c_size_t * 23)()
    assert _lib.lib().nr_abi_sizes(sizes, 23) == 0
    assert sizes[21] == C.sizeof(_lib.EntropyDesc) and sizes[22] == C.sizeof(_lib.ExpectAffineDesc)
    short = (C.c_size_t * 23)(*([12345] * 23))
    assert _lib.lib().nr_abi_sizes(short, 21) == 0 and short[21] == 12345 and short[22] == 12345 and list(short)[:21] == list(sizes)[:21]
    common = ("news_vecs", "user_vecs", "temperature", "base", "exclude", "splits", "prior", "stamp", "window")
    for fn, names in ((ops.score_entropy, common),
                      (ops.score_expect_affine, common + ("alpha", "beta", "sub_ids", "sub_w", "scale_inv_tau")),
                      (ops.full_softmax_nll_entropy, ("news_vecs", "user_vecs", "targets", "temperature", "exclude", "splits", "prior", "stamp", "window",
                                                      "return_count")),
                      (train.policy_entropy, tuple(inspect.signature(train.log_partition).parameters)),
                      (train.full_softmax_loss_entropy, ("model", "news_vecs", "hist_idx", "mask", "targets", "temperature", "entropy_weight",
                                                         "exclude_history", "batch_size", "prior", "news_time", "window", "seen")),
                      (metrics.entropy_reference, ("news", "user", "temperature", "exclude", "prior", "stamp", "window")),
                      (metrics.expect_affine_reference, ("news", "user", "temperature", "exclude", "prior", "stamp", "window", "alpha", "beta", "sub_ids",
                                                         "sub_w", "scale_inv_tau"))):
        assert tuple(inspect.signature(fn).parameters) == names


def test_full_softmax_nll_entropy_refusals():
    news = torch.randn(10, 8, requires_grad=True)
    user = torch.randn(3, 8, requires_grad=True)
    targets = torch.ones(3, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"full_softmax_nll_entropy: news_vecs requires grad.*P\^T \. users.*\[V, N\] reduction over every user"
                                            r".*not part of this call"):
        ops.full_softmax_nll_entropy(news, user, targets, 0.5)
    with pytest.raises(RuntimeError, match=r"full_softmax_nll_entropy: targets must be an integer tensor \[U = 3, T\]"):
        ops.full_softmax_nll_entropy(news.detach(), user, targets[:2], 0.5)
    with pytest.raises(RuntimeError, match=r"full_softmax_nll_entropy: a temperature tensor must be floating point, 0-dim or of shape \(3,\)"):
        ops.full_softmax_nll_entropy(news.detach(), user, targets, torch.ones(4))
