"""CPU: the host side of the expected-news-vector pass (include/nrhip.h, K17) -- metrics.expect_reference against a direct fp64
softmax(scores / tau) @ news over the eligible set and against the autograd gradient of a fp64 logsumexp, the descriptor's
place in nr_abi_sizes, the workspace sizes and the refusals nr_score_expect makes before it launches anything (fake non-null
pointers: a launch would fault, a refusal does not), and ops.full_softmax_nll refusing a table that requires grad."""
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


def test_expect_reference_is_the_plain_softmax_mean_over_the_eligible_set():
    news, user, prior, stamp, window, exclude = _case()
    U = user.shape[0]
    tau = np.linspace(0.2, 3.0, U)
    w = np.linspace(-1.0, 2.0, U)
    expect, mass = metrics.expect_reference(news, user, temperature=tau, exclude=exclude, prior=prior, stamp=stamp, window=window)
    weighted, _ = metrics.expect_reference(news, user, temperature=tau, exclude=exclude, prior=prior, stamp=stamp, window=window, weight=w)
    assert expect.dtype == np.float64 and expect.shape == user.shape and mass.shape == (U,)
    seen_empty = False
    for u in range(U):
        el = _eligible(u, news, user, prior, stamp, window, exclude)
        if not el:
            seen_empty = True
            assert u == 4 and not expect[u].any() and mass[u] == 0.0
            continue
        assert 7 not in el
        x = torch.tensor((news[el] @ user[u] + prior[el]) / tau[u], dtype=torch.float64)
        direct = torch.softmax(x, 0).numpy() @ news[el]
        np.testing.assert_allclose(expect[u], direct, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(weighted[u], w[u] * direct, rtol=1e-12, atol=1e-14)
        assert abs(mass[u] - 1.0) <= 1e-14
    assert seen_empty
    # a bad temperature: that user alone is NaN, unless it has nothing eligible
    bad = tau.copy()
    bad[1], bad[4] = 0.0, NAN
    e2, m2 = metrics.expect_reference(news, user, temperature=bad, exclude=exclude, prior=prior, stamp=stamp, window=window)
    assert np.isnan(e2[1]).all() and np.isnan(m2[1]) and not e2[4].any() and m2[4] == 0.0
    keep = [u for u in range(U) if u not in (1, 4)]
    assert np.array_equal(e2[keep], expect[keep])


def test_expect_reference_is_the_gradient_of_the_log_partition():
    """d/du [tau * logsumexp(scores / tau)] = E: autograd of the fp64 log-partition with respect to the user vector is expect / tau."""
    news, user, prior, stamp, window, exclude = _case(seed=8)
    news[7, 3] = 0.5                                                   # autograd has no NaN rule
    tau = 0.7
    expect, _ = metrics.expect_reference(news, user, temperature=tau, exclude=exclude, prior=prior, stamp=stamp, window=window)
    for u in range(user.shape[0]):
        el = _eligible(u, news, user, prior, stamp, window, exclude)
        if not el:
            continue
        uv = torch.tensor(user[u], dtype=torch.float64, requires_grad=True)
        logz = torch.logsumexp((torch.tensor(news[el]) @ uv + torch.tensor(prior[el])) / tau, 0)
        (g,) = torch.autograd.grad(logz, uv)
        np.testing.assert_allclose(g.numpy(), expect[u] / tau, rtol=1e-11, atol=1e-13)


BASE = dict(news_vecs=P, ld_news=400, V=100001, user=P, ld_user=400, U=8192, N=400, tau=0.5, base_max=P, base_logsum=P, out=P, ld_out=400)


def _refusal(**fields):
    """(size query's answer, return code of the call, nr_last_error after it); the workspace is what the unbroken descriptor asks for."""
    lib = _lib.lib()
    short = fields.pop("short_ws", False)
    d = _lib.ExpectDesc(**dict(BASE, **fields))
    size = lib.nr_score_expect_workspace_bytes(C.byref(d))
    need = lib.nr_score_expect_workspace_bytes(C.byref(_lib.ExpectDesc(**BASE)))
    d.ws, d.ws_bytes = P, need - 8 if short else need
    rc = lib.nr_score_expect(C.byref(d), None)
    return size, rc, _lib.last_error()


REFUSED = {
    "V=1": (dict(V=1), "score_expect: V = 1 news rows; row 0 is the padding news, so at least 2 are needed"),
    "U=0": (dict(U=0), "score_expect: U = 0 users"),
    "N=6": (dict(N=6), "score_expect: vector width N = 6 must be a multiple of 4 in [4, 1024]"),
    "stamp-alone": (dict(stamp=P), "score_expect: stamp given without window (the two come together)"),
    "window-alone": (dict(window=P, ld_window=2), "score_expect: window given without stamp (the two come together)"),
    "ld_window=1": (dict(stamp=P, window=P, ld_window=1), "score_expect: ld_window = 1, a window row is (lo, hi): at least 2"),
    "ids-alone": (dict(excl_ids=P, n_excl=5), "score_expect: excl_ids given without excl_offsets (n_excl = 5; the two come together)"),
    "offsets-alone": (dict(excl_offsets=P, n_excl=5), "score_expect: excl_offsets given without excl_ids (n_excl = 5; the two come together)"),
    "tau=0": (dict(tau=0.0), "score_expect: tau = 0, a scalar temperature must be finite and > 0"),
    "splits=257": (dict(splits=257), "score_expect: splits = 257, must be 0 (library's choice) or in [1, 196], the segments of V = 100001"),
}
CALL_ONLY = {
    "null-base_max": (dict(base_max=None), "score_expect: null pointer (news_vecs, user, base_max, base_logsum, out)"),
    "null-base_logsum": (dict(base_logsum=None), "score_expect: null pointer (news_vecs, user, base_max, base_logsum, out)"),
    "null-out": (dict(out=None), "score_expect: null pointer (news_vecs, user, base_max, base_logsum, out)"),
    "ids-without-w": (dict(sub_ids=P, T=4, ld_sub=4), "score_expect: sub_ids given without sub_w (the two come together)"),
    "w-without-ids": (dict(sub_w=P, T=4, ld_sub=4), "score_expect: sub_w given without sub_ids (the two come together)"),
    "T=0": (dict(sub_ids=P, sub_w=P, T=0, ld_sub=4), "score_expect: T = 0 named rows per user (row stride 4), must be in [1, 128] with ld_sub >= T"),
    "T=129": (dict(sub_ids=P, sub_w=P, T=129, ld_sub=129),
              "score_expect: T = 129 named rows per user (row stride 129), must be in [1, 128] with ld_sub >= T"),
    "ld_sub<T": (dict(sub_ids=P, sub_w=P, T=8, ld_sub=4), "score_expect: T = 8 named rows per user (row stride 4), must be in [1, 128] with ld_sub >= T"),
    "ld_news=N+1": (dict(ld_news=401), "score_expect: rows must be 16-byte aligned (ld_news = 401, ld_user = 400: multiples of 4, >= N = 400)"),
    "user-misaligned": (dict(user=P + 4), "score_expect: rows must be 16-byte aligned (ld_news = 400, ld_user = 400: multiples of 4, >= N = 400)"),
    "ld_out<N": (dict(ld_out=396), "score_expect: out must be 16-byte aligned with ld_out = 396 >= N = 400"),
    "out-misaligned": (dict(out=P + 4), "score_expect: out must be 16-byte aligned with ld_out = 400 >= N = 400"),
    "short-workspace": (dict(short_ws=True),
                        "score_expect: workspace holds 13172728 bytes, nr_score_expect_workspace_bytes asks for 13172736 (8-byte aligned)"),
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
    assert _refusal(ld_news=401, short_ws=True)[2] == CALL_ONLY["ld_news=N+1"][1]
    lib = _lib.lib()
    assert lib.nr_score_expect_workspace_bytes(None) == 0 and lib.nr_score_expect(None, None) == 1
    assert _lib.last_error() == "score_expect: null descriptor"


def _ws(N, U, V, splits):
    return _lib.lib().nr_score_expect_workspace_bytes(C.byref(_lib.ExpectDesc(**dict(BASE, ld_news=N, ld_user=N, ld_out=N, N=N, U=U, V=V, splits=splits))))


def test_workspace_is_one_row_and_one_mass_per_user_and_slice():
    """U * slices * (N * 4 + 8) bytes.  The user tile is 64 up to N = 352, 32 up to N = 832, then 16 (the P tile beside the vectors and
    the staging buffers in 160 KiB); the library's slice count fills 256 CUs with user tiles and is at most the segments of V."""
    per = lambda N, U, s: U * s * (N * 4 + 8)
    assert _ws(400, 8192, 100001, 0) == per(400, 8192, 1)              # 256 tiles of 32 users
    assert _ws(352, 8192, 100001, 0) == per(352, 8192, 2)              # 128 tiles of 64 users
    assert _ws(356, 8192, 100001, 0) == per(356, 8192, 1)              # 32 users again
    assert _ws(832, 64, 100001, 0) == per(832, 64, 98)                 # 2 tiles of 32 -> 128 slices asked, 98 of 2 segments each
    assert _ws(836, 64, 100001, 0) == per(836, 64, 49)                 # 4 tiles of 16 -> 64 slices asked, 49 of 4 segments each
    assert _ws(400, 1, 100001, 0) == per(400, 1, 196)                  # every segment its own slice
    assert _ws(400, 70, 100001, 3) == per(400, 70, 3)
    assert _ws(4, 1, 2, 0) == per(4, 1, 1) and _ws(4, 1, 130, 2) == per(4, 1, 2)
    assert _ws(4, 3, 1 + 128 * 256 + 5, 2) == per(4, 3, 2)             # 129 segments of 256 ids in 2 slices
    assert _ws(400, 65, 130, 3) == 0                                   # 2 segments: 3 slices are refused


def test_descriptor_is_entry_15_of_abi_sizes_and_the_new_names_exist():
    sizes = (C.c_size_t * 16)()
    assert _lib.lib().nr_abi_sizes(sizes, 16) == 0 and sizes[15] == C.sizeof(_lib.ExpectDesc)
    fifteen = (C.c_size_t * 16)(*([12345] * 16))
    assert _lib.lib().nr_abi_sizes(fifteen, 15) == 0 and fifteen[15] == 12345 and list(fifteen)[:15] == list(sizes)[:15]
    for fn, names in ((ops.score_expect, ("news_vecs", "user_vecs", "temperature", "base", "exclude", "splits", "prior", "stamp", "window", "weight")),
                      (ops.full_softmax_nll, ("news_vecs", "user_vecs", "targets", "temperature", "exclude", "splits", "prior", "stamp", "window")),
                      (train.full_softmax_loss, ("model", "news_vecs", "hist_idx", "mask", "targets", "temperature", "exclude_history", "batch_size",
                                                 "prior", "news_time", "window", "seen")),
                      (metrics.expect_reference, ("a", "b", "temperature", "exclude", "prior", "stamp", "window", "weight"))):
        assert tuple(inspect.signature(fn).parameters) == names


def test_full_softmax_nll_refuses_a_table_that_requires_grad():
    news = torch.randn(10, 8, requires_grad=True)
    user = torch.randn(3, 8, requires_grad=True)
    targets = torch.ones(3, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"news_vecs requires grad.*P\^T \. users.*\[V, N\] reduction over every user.*not part of this call"):
        ops.full_softmax_nll(news, user, targets, 0.5)
