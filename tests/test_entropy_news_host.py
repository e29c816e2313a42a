"""CPU: the host side of the news-table pass of the entropy-regularised full softmax (include/nrhip.h, K25) --
metrics.expect_news_affine_reference against float64 autograd of the dense statement sum_u (sum_t g nll + h H) with respect to the
news table, a mutant per formula, the descriptor's place in nr_abi_sizes, the workspace size beside K18's, the refusals
nr_score_expect_news_affine makes before it launches anything (fake non-null pointers: a launch would fault, a refusal does
not), the new functions' parameter lists and the Python-level refusals of ops.full_softmax_nll_entropy_joint."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import test_expect_news_host as EN
from newsrecommendation_amd import _lib, metrics, ops, train

INF, NAN = float("inf"), float("nan")
P = EN.P


def _dense_case():
    """V = 41, U = 9, N = 8 with a -inf prior, windows (one empty: a dead user), ragged lists, fill targets, a repeat, one news
    named by several users, per-user temperatures, and fp32-valued upstream gradients g [U, T] and h [U]."""
    news, user, prior, stamp, window, exclude = EN._case(seed=8, nan_row=False)
    U, V = user.shape[0], news.shape[0]
    rng = np.random.default_rng(3)
    tau = np.linspace(0.4, 1.5, U)
    T = 6
    targets = rng.integers(1, V, (U, T))
    targets[:, 1] = 0                                                  # fill
    targets[::2, 2] = V + 2                                            # fill: out of range
    targets[1, 3] = targets[1, 0]                                      # a repeat: two entries
    targets[:, 0] = np.where(np.arange(U) % 3 == 0, 12, targets[:, 0])  # one news named by several users
    g = rng.standard_normal((U, T)).astype(np.float32).astype(np.float64)
    h = rng.standard_normal(U).astype(np.float32).astype(np.float64)
    h[3] = 0.0                                                         # a user whose entropy is in no loss
    return news, user, prior, stamp, window, exclude, tau, targets, g, h


def _autograd(news, user, prior, stamp, window, exclude, tau, targets, g, h):
    """(gradient of sum_u (sum_t g_ut nll(u, t) + h_u H_u) with respect to the table, gw [U, T], H [U]) in float64 autograd; the
    softmax over EN._eligible, a target's own eligibility the caller's statement as in row_logprob."""
    U, V, T = user.shape[0], news.shape[0], targets.shape[1]
    tab = torch.tensor(news, dtype=torch.float64, requires_grad=True)
    total = torch.zeros((), dtype=torch.float64)
    gw, H = np.zeros((U, T)), np.zeros(U)
    for u in range(U):
        el = EN._eligible(u, news, user, prior, stamp, window, exclude)
        if not el:
            assert u == 4                                              # the dead user: no term, no named term
            continue
        uv = torch.tensor(user[u])
        z = (tab[el] @ uv + torch.tensor(prior[el])) / tau[u]
        logz = torch.logsumexp(z, 0)
        x = z - logz
        ent = -(torch.exp(x) * x).sum()
        H[u] = float(ent.detach())
        total = total + h[u] * ent
        for t in range(T):
            v = int(targets[u, t])
            if 1 <= v < V:
                total = total + g[u, t] * (logz - (tab[v] @ uv + prior[v]) / tau[u])
                gw[u, t] = g[u, t]
    (grad,) = torch.autograd.grad(total, tab)
    return grad.numpy(), gw, H


def _reference(case, gw, H, mutant=None):
    """The reference fed the way FullSoftmaxEntropyJointFunction.backward feeds K25: alpha = sum_t g - h H, beta = -h, the valid
    targets as named terms, scale_inv_tau.  mutant: "no_H" (alpha without the entropy), "beta_sign" (beta = +h), "beta_no_tau"
    (beta without 1 / tau)."""
    news, user, prior, stamp, window, exclude, tau, targets, g, h = case
    V = news.shape[0]
    alpha = gw.sum(axis=1) - (0.0 if mutant == "no_H" else h * H)
    beta = h if mutant == "beta_sign" else -h
    if mutant == "beta_no_tau":
        beta = beta * tau                                              # the reference divides it again: the 1 / tau is gone
    named = ops._named_by_news(torch.tensor(targets, dtype=torch.int32), torch.tensor(gw, dtype=torch.float32), V)
    return metrics.expect_news_affine_reference(news, user, temperature=tau, exclude=exclude, prior=prior, stamp=stamp, window=window,
                                                alpha=alpha, beta=beta, named=(named[0].numpy(), named[1].numpy(), named[2].double().numpy()),
                                                scale_inv_tau=True)


def test_affine_reference_is_the_gradient_of_the_regularised_loss_with_respect_to_the_table():
    case = _dense_case()
    grad, gw, H = _autograd(*case)
    out, mass = _reference(case, gw, H)
    assert out.dtype == np.float64 and out.shape == case[0].shape
    np.testing.assert_allclose(out, grad, rtol=1e-10, atol=1e-12)
    assert not out[0].any() and np.abs(grad).max() > 0.1
    # the mass is K18's with weight None: the masses of the live users add up to their number
    _, m18 = metrics.expect_news_reference(case[0], case[1], temperature=case[6], exclude=case[5], prior=case[2], stamp=case[3], window=case[4])
    assert np.array_equal(mass, m18) and abs(mass.sum() - 8) <= 1e-12


@pytest.mark.parametrize("mutant", ["no_H", "beta_sign", "beta_no_tau"])
def test_every_formula_of_the_feed_is_needed(mutant):
    case = _dense_case()
    grad, gw, H = _autograd(*case)
    out, _ = _reference(case, gw, H, mutant)
    assert np.abs(out - grad).max() > 1e-3 * np.abs(grad).max(), mutant


def test_affine_reference_edge_cases():
    news, user, prior, stamp, window, exclude = EN._case()
    U = user.shape[0]
    tau = np.linspace(0.2, 3.0, U)
    kw = dict(temperature=tau, exclude=exclude, prior=prior, stamp=stamp, window=window)
    w = np.linspace(-1.0, 2.0, U)
    # beta None: K18's reference with weight = alpha, with and without 1 / tau
    for scale in (False, True):
        o18, _ = metrics.expect_news_reference(news, user, weight=w, scale_inv_tau=scale, **kw)
        o25, _ = metrics.expect_news_affine_reference(news, user, alpha=w, scale_inv_tau=scale, **kw)
        np.testing.assert_allclose(o25, o18, rtol=1e-13, atol=1e-15)
    # a user whose alpha or beta is not finite contributes nothing: the same as alpha = beta = 0 for it; the mass keeps it
    al, be = w.copy(), np.linspace(0.5, -0.5, U)
    al0, be0 = al.copy(), be.copy()
    al[1], be[6], be[7] = NAN, INF, NAN
    al0[[1, 6, 7]] = be0[[1, 6, 7]] = 0.0
    o_bad, m_bad = metrics.expect_news_affine_reference(news, user, alpha=al, beta=be, **kw)
    o_zero, m_zero = metrics.expect_news_affine_reference(news, user, alpha=al0, beta=be0, **kw)
    assert np.isfinite(o_bad).all() and np.array_equal(o_bad, o_zero) and np.array_equal(m_bad, m_zero)


def test_descriptor_is_entry_23_of_abi_sizes_and_the_new_names_exist():
    sizes = (C.c_size_t * 24)()
    assert _lib.lib().nr_abi_sizes(sizes, 24) == 0 and sizes[23] == C.sizeof(_lib.ExpectNewsAffineDesc) and all(sizes)
    short = (C.c_size_t * 24)(*([12345] * 24))
    assert _lib.lib().nr_abi_sizes(short, 23) == 0 and short[23] == 12345 and list(short)[:23] == list(sizes)[:23]
    # nr_expect_news_desc with `weight` replaced by alpha, then beta
    k18 = [n for n, _ in _lib.ExpectNewsDesc._fields_]
    at = k18.index("weight")
    assert [n for n, _ in _lib.ExpectNewsAffineDesc._fields_] == k18[:at] + ["alpha", "beta"] + k18[at + 1:]
    pools = ("prior", "stamp", "window")
    for fn, names in ((metrics.expect_news_affine_reference, ("a", "b", "temperature", "exclude") + pools + ("alpha", "beta", "named", "scale_inv_tau")),
                      (ops.score_expect_news_affine, ("news_vecs", "user_vecs", "temperature", "base", "exclude", "splits") + pools + ("alpha", "beta")),
                      (ops.full_softmax_nll_entropy_joint, ("news_vecs", "user_vecs", "targets", "temperature", "exclude", "splits") + pools
                       + ("return_count",)),
                      (train.full_softmax_loss_entropy_joint, ("model", "news_table", "hist_idx", "mask", "targets", "temperature", "entropy_weight",
                                                               "exclude_history", "batch_size", "prior", "news_time", "window", "seen"))):
        assert tuple(inspect.signature(fn).parameters) == names, fn
    sig = inspect.signature(metrics.expect_news_affine_reference).parameters
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[2:]) and sig["scale_inv_tau"].default is False
    ref = inspect.signature(train.full_softmax_loss_entropy).parameters
    new = inspect.signature(train.full_softmax_loss_entropy_joint).parameters
    assert [p.default for p in new.values()] == [p.default for p in ref.values()]


BASE = dict(EN.BASE)


def _refusal(**fields):
    """(size query's answer, return code of the call, nr_last_error after it); the workspace is what the unbroken descriptor asks for."""
    lib = _lib.lib()
    short = fields.pop("short_ws", False)
    d = _lib.ExpectNewsAffineDesc(**dict(BASE, **fields))
    size = lib.nr_score_expect_news_affine_workspace_bytes(C.byref(d))
    need = lib.nr_score_expect_news_affine_workspace_bytes(C.byref(_lib.ExpectNewsAffineDesc(**BASE)))
    d.ws, d.ws_bytes = P, need - 8 if short else need
    rc = lib.nr_score_expect_news_affine(C.byref(d), None)
    return size, rc, _lib.last_error()


def _k25(text):
    return text.replace("score_expect_news", "score_expect_news_affine")


# K18's refusals read onto this descriptor: the same sentences under this call's name; a null out has a sentence of its own
REFUSED = {rule: (fields, _k25(text)) for rule, (fields, text) in EN.REFUSED.items() if rule != "no-output"}
REFUSED["null-out"] = (dict(out=None, out_mass=P), "score_expect_news_affine: out is null (this call has no mass-only mode: nr_score_expect_news has it)")
CALL_ONLY = {rule: (fields, _k25(text)) for rule, (fields, text) in EN.CALL_ONLY.items()}


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
    assert _refusal(out=None, base_max=None)[2] == REFUSED["null-out"][1]
    assert _refusal(ld_news=401, short_ws=True)[2] == CALL_ONLY["ld_news=N+1"][1]
    assert _refusal(base_max=None, named_w=P)[2] == CALL_ONLY["null-base_max"][1]
    assert _refusal(named_user=P, ld_out=396)[2] == CALL_ONLY["named-user-alone"][1]
    lib = _lib.lib()
    assert lib.nr_score_expect_news_affine_workspace_bytes(None) == 0 and lib.nr_score_expect_news_affine(None, None) == 1
    assert _lib.last_error() == "score_expect_news_affine: null descriptor"


def test_workspace_is_the_rows_mode_size_of_k18():
    """The shapes of test_expect_news_host.test_workspace_is_one_row_and_one_mass_per_news_and_slice: the same plan of the user
    axis, the library's choice included, and the rows-mode bytes; alpha and beta do not enter."""
    lib = _lib.lib()
    for N, V, U, splits in ((400, 100001, 8192, 0), (400, 34, 8192, 0), (352, 4096, 8192, 0), (356, 4096, 8192, 0), (832, 1024, 8192, 0),
                            (836, 1024, 8192, 0), (400, 294, 300, 2), (400, 294, 300, 3), (4, 2, 1, 0), (4, 130, 294, 3),
                            (4, 70, 128 * 256 + 5, 2), (4, 70, 128 * 256 + 5, 0), (400, 130, 129, 3)):
        shape = dict(ld_news=N, ld_user=N, ld_out=N, N=N, U=U, V=V, splits=splits)
        for extra in (dict(), dict(alpha=P, beta=P, out_mass=P)):
            got = lib.nr_score_expect_news_affine_workspace_bytes(C.byref(_lib.ExpectNewsAffineDesc(**dict(BASE, **shape, **extra))))
            assert got == EN._ws(N, V, U, splits), (N, V, U, splits)
    assert EN._ws(400, 130, 129, 3) == 0 and EN._ws(400, 294, 300, 3) == 294 * 3 * (400 * 4 + 8)


def test_full_softmax_nll_entropy_joint_refusals():
    news = torch.randn(10, 8, requires_grad=True)
    user = torch.randn(3, 8, requires_grad=True)
    targets = torch.ones(3, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"full_softmax_nll_entropy_joint: targets must be an integer tensor \[U = 3, T\]"):
        ops.full_softmax_nll_entropy_joint(news, user, targets[:2], 0.5)
    with pytest.raises(RuntimeError, match=r"full_softmax_nll_entropy_joint: targets must be an integer tensor \[U = 3, T\]"):
        ops.full_softmax_nll_entropy_joint(news, user, targets.float(), 0.5)
    with pytest.raises(RuntimeError, match=r"full_softmax_nll_entropy_joint: T = 129 targets per user, must be in \[1, 128\]"):
        ops.full_softmax_nll_entropy_joint(news, user, torch.ones(3, 129, dtype=torch.int32), 0.5)
    with pytest.raises(RuntimeError, match=r"full_softmax_nll_entropy_joint: a temperature tensor must be floating point, 0-dim or of shape \(3,\)"):
        ops.full_softmax_nll_entropy_joint(news, user, targets, torch.ones(4))
    with pytest.raises(RuntimeError, match=r"full_softmax_nll_entropy_joint: a temperature tensor must be floating point"):
        ops.full_softmax_nll_entropy_joint(news, user, targets, torch.ones(3, dtype=torch.int64))
    # the frozen-table function keeps its refusal and points here
    with pytest.raises(RuntimeError, match=r"full_softmax_nll_entropy: news_vecs requires grad.*not part of this call.*full_softmax_nll_entropy_joint"):
        ops.full_softmax_nll_entropy(news, user, targets, 0.5)
