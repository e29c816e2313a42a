"""CPU: the host side of the KL passes (include/nrhip.h, K26 and K27) -- metrics.kl_reference and metrics.expect_kl_reference
against a dense float64 statement KL(softmax(s / tau) || softmax(s' / tau')) written out here (pools, lists, per-user temperatures,
an empty user), the identities dKL / duser = expect_kl(-KL, 1, -1) / tau, dKL / dtau = -cov / tau and the forward mode's
(E_p - E_q) / tau against float64 autograd of that statement, the descriptors' places in nr_abi_sizes, the workspace sizes and the
refusals the two calls make before they launch anything (fake non-null pointers: a launch would fault, a refusal does not)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from newsrecommendation_amd import _lib, metrics, ops, train
from test_entropy_host import P, _case, _dense, _eligible

INF, NAN = float("inf"), float("nan")


def _kl_case(seed=5):
    news, user, prior, stamp, window, exclude = _case(seed)
    rng = np.random.default_rng(seed + 100)
    ref = user + 0.4 * rng.standard_normal(user.shape)
    U = user.shape[0]
    return news, user, ref, np.linspace(0.2, 3.0, U), np.linspace(2.5, 0.4, U), dict(exclude=exclude, prior=prior, stamp=stamp, window=window)


def _dense_kl(news_el, prior_el, uv, tau, rv, rtau):
    """(kl, lp, p, lq) of one user as float64 torch values with a graph to uv and tau."""
    lp, p = _dense(news_el, prior_el, uv, tau)
    lq, _ = _dense(news_el, prior_el, rv, rtau)
    return (p * (lp - lq)).sum(), lp, p, lq


def test_kl_reference_is_the_dense_statement():
    news, user, ref, tau, rtau, kw = _kl_case()
    U = user.shape[0]
    kl, H, cov, mass = metrics.kl_reference(news, user, ref, tau, rtau, **kw)
    assert kl.dtype == np.float64 and kl.shape == H.shape == cov.shape == mass.shape == (U,)
    H0, _, _ = metrics.entropy_reference(news, user, tau, **kw)
    np.testing.assert_allclose(H, H0, rtol=1e-12, atol=1e-14)
    seen_empty = False
    for u in range(U):
        el = _eligible(u, news, user, kw["prior"], kw["stamp"], kw["window"], kw["exclude"])
        if not el:
            seen_empty = True
            assert u == 4 and (kl[u], H[u], cov[u], mass[u]) == (0.0, 0.0, 0.0, 0.0)
            continue
        k, lp, p, lq = _dense_kl(news[el], kw["prior"][el], torch.tensor(user[u]), float(tau[u]), torch.tensor(ref[u]), float(rtau[u]))
        d = lp - lq
        np.testing.assert_allclose(kl[u], float(k), rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(cov[u], float((p * d * lp).sum() - (p * d).sum() * (p * lp).sum()), rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(mass[u], 1.0, rtol=1e-12)
        assert kl[u] > 0
    assert seen_empty
    # the reference equal to the policy: exactly zero; bad temperatures on either side: that user alone
    same = metrics.kl_reference(news, user, user, tau, tau, **kw)
    assert not same[0].any() and not same[2].any()
    bad_t, bad_r = tau.copy(), rtau.copy()
    bad_t[1], bad_r[2], bad_r[4] = 0.0, NAN, INF                        # user 4 has nothing eligible: zeros whatever the temperatures
    got = metrics.kl_reference(news, user, ref, bad_t, bad_r, **kw)
    keep = [u for u in range(U) if u not in (1, 2)]
    for a, b in zip(got, (kl, H, cov, mass)):
        assert np.isnan(a[[1, 2]]).all() and np.array_equal(a[keep], b[keep])


def test_the_gradient_identities_against_autograd():
    news, user, ref, tau, rtau, kw = _kl_case(seed=9)
    U = user.shape[0]
    kl, H, cov, _ = metrics.kl_reference(news, user, ref, tau, rtau, **kw)
    grad, _ = metrics.expect_kl_reference(news, user, ref, tau, rtau, alpha=-kl, beta=np.ones(U), gamma=-np.ones(U), scale_inv_tau=True, **kw)
    e_p, _ = metrics.expect_reference(news, user, temperature=tau, **kw)
    e_q, _ = metrics.expect_reference(news, ref, temperature=rtau, **kw)
    fwd_val = metrics.kl_reference(news, ref, user, rtau, tau, **kw)[0]
    clean = np.where(np.isfinite(news), news, 0.0)
    checked = 0
    for u in range(U):
        el = _eligible(u, news, user, kw["prior"], kw["stamp"], kw["window"], kw["exclude"])
        if not el:
            assert not grad[u].any()
            continue
        uv = torch.tensor(user[u], requires_grad=True)
        t = torch.tensor(float(tau[u]), dtype=torch.float64, requires_grad=True)
        k, lp, p, lq = _dense_kl(clean[el], kw["prior"][el], uv, t, torch.tensor(ref[u]), float(rtau[u]))
        k.backward()
        np.testing.assert_allclose(grad[u], uv.grad.numpy(), rtol=1e-9, atol=1e-12)          # dKL / duser = expect_kl(-KL, 1, -1) / tau
        np.testing.assert_allclose(-cov[u] / tau[u], float(t.grad), rtol=1e-8, atol=1e-11)   # dKL / dtau = -cov / tau
        # the forward mode: KL(q || p) and its gradient (E_p - E_q) / tau with respect to the policy's vector
        uv2 = torch.tensor(user[u], requires_grad=True)
        lp2, _ = _dense(clean[el], kw["prior"][el], uv2, float(tau[u]))
        lq2, q2 = _dense(clean[el], kw["prior"][el], torch.tensor(ref[u]), float(rtau[u]))
        f = (q2 * (lq2 - lp2)).sum()
        f.backward()
        np.testing.assert_allclose(fwd_val[u], float(f), rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose((e_p[u] - e_q[u]) / tau[u], uv2.grad.numpy(), rtol=1e-9, atol=1e-12)
        checked += 1
    assert checked >= 6


def test_expect_kl_reference_is_the_dense_statement():
    news, user, ref, tau, rtau, kw = _kl_case(seed=13)
    U, V = user.shape[0], news.shape[0]
    rng = np.random.default_rng(3)
    al, be, ga = rng.standard_normal(U), rng.standard_normal(U), rng.standard_normal(U)
    ids = rng.integers(-1, V + 2, (U, 4))
    sw = rng.standard_normal((U, 4))
    out, mass = metrics.expect_kl_reference(news, user, ref, tau, rtau, alpha=al, beta=be, gamma=ga, sub_ids=ids, sub_w=sw, scale_inv_tau=True, **kw)
    plain, _ = metrics.expect_kl_reference(news, user, ref, tau, rtau, **kw)
    affine, _ = metrics.expect_affine_reference(news, user, tau, alpha=al, beta=be, **kw)
    g0, _ = metrics.expect_kl_reference(news, user, ref, tau, rtau, alpha=al, beta=be, **kw)
    np.testing.assert_array_equal(g0, affine)                           # gamma = 0: K24's statement
    np.testing.assert_allclose(plain, metrics.expect_reference(news, user, temperature=tau, **kw)[0], rtol=1e-12, atol=1e-14)
    clean = np.where(np.isfinite(news), news, 0.0)
    for u in range(U):
        el = _eligible(u, news, user, kw["prior"], kw["stamp"], kw["window"], kw["exclude"])
        want = np.zeros(news.shape[1])
        if el:
            _, lp, p, lq = _dense_kl(news[el], kw["prior"][el], torch.tensor(user[u]), float(tau[u]), torch.tensor(ref[u]), float(rtau[u]))
            want = ((p * (al[u] + be[u] * lp + ga[u] * lq)).numpy()) @ clean[el]
        with np.errstate(invalid="ignore"):
            for j in range(4):
                if 1 <= ids[u, j] < V:
                    want = want - sw[u, j] * news[ids[u, j]]
        np.testing.assert_allclose(out[u], want / tau[u], rtol=1e-9, atol=1e-12, equal_nan=True)
        assert mass[u] == (0.0 if not el else mass[u]) and (not el or abs(mass[u] - 1.0) < 1e-12)
    # a NaN user of kl_reference: a row of NaN
    bad = rtau.copy()
    bad[0] = -1.0
    out_b, mass_b = metrics.expect_kl_reference(news, user, ref, tau, bad, alpha=al, beta=be, gamma=ga, **kw)
    assert np.isnan(out_b[0]).all() and np.isnan(mass_b[0]) and not np.isnan(mass_b[1:]).any()


K_BASE = dict(news_vecs=P, ld_news=400, V=100001, user=P, ld_user=400, U=8192, N=400, tau=0.5, base_max=P, base_logsum=P, ref=P, ld_ref=400,
              ref_tau=0.7, ref_base_max=P, ref_base_logsum=P, out_kl=P)
X_BASE = dict(news_vecs=P, ld_news=400, V=100001, user=P, ld_user=400, U=8192, N=400, tau=0.5, base_max=P, base_logsum=P, ref=P, ld_ref=400,
              ref_tau=0.7, ref_base_max=P, ref_base_logsum=P, out=P, ld_out=400)
CALLS = {"score_kl": (_lib.KlDesc, K_BASE, "nr_score_kl"), "score_expect_kl": (_lib.ExpectKlDesc, X_BASE, "nr_score_expect_kl")}


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


# what K17 refuses of the shared fields, and the scalar reference temperature: refused by the size query too
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
    "ref_tau=inf": (dict(ref_tau=INF), "{}: ref_tau = inf, a scalar reference temperature must be finite and > 0"),
    "splits=257": (dict(splits=257), "{}: splits = 257, must be 0 (library's choice) or in [1, 196], the segments of V = 100001"),
}
# the reference side, refused by both calls before any launch
REF_REFUSED = {
    "null-ref": (dict(ref=None), "{}: null pointer (ref: the reference user vectors)"),
    "null-ref_base_max": (dict(ref_base_max=None),
                          "{}: null pointer (ref_base_max, ref_base_logsum: the base of nr_score_logz for the reference vectors)"),
    "null-ref_base_logsum": (dict(ref_base_logsum=None),
                             "{}: null pointer (ref_base_max, ref_base_logsum: the base of nr_score_logz for the reference vectors)"),
    "ld_ref=N+1": (dict(ld_ref=401), "{}: ref rows must be 16-byte aligned (ld_ref = 401: a multiple of 4, >= N = 400)"),
    "ld_ref<N": (dict(ld_ref=396), "{}: ref rows must be 16-byte aligned (ld_ref = 396: a multiple of 4, >= N = 400)"),
    "ref-misaligned": (dict(ref=P + 4), "{}: ref rows must be 16-byte aligned (ld_ref = 400: a multiple of 4, >= N = 400)"),
    "ld_news=N+1": (dict(ld_news=401), "{}: rows must be 16-byte aligned (ld_news = 401, ld_user = 400: multiples of 4, >= N = 400)"),
    "user-misaligned": (dict(user=P + 4), "{}: rows must be 16-byte aligned (ld_news = 400, ld_user = 400: multiples of 4, >= N = 400)"),
}
KL_CALL_ONLY = {
    "null-base_max": (dict(base_max=None), "score_kl: null pointer (news_vecs, user, base_max, base_logsum, out_kl)"),
    "null-base_logsum": (dict(base_logsum=None), "score_kl: null pointer (news_vecs, user, base_max, base_logsum, out_kl)"),
    "null-out_kl": (dict(out_kl=None), "score_kl: null pointer (news_vecs, user, base_max, base_logsum, out_kl)"),
    "short-workspace": (dict(short_ws=True), "score_kl: workspace holds 262136 bytes, nr_score_kl_workspace_bytes asks for 262144 (8-byte aligned)"),
}
EXPECT_KL_CALL_ONLY = {
    "null-base_max": (dict(base_max=None), "score_expect_kl: null pointer (news_vecs, user, base_max, base_logsum, out)"),
    "null-out": (dict(out=None), "score_expect_kl: null pointer (news_vecs, user, base_max, base_logsum, out)"),
    "ids-without-w": (dict(sub_ids=P, T=4, ld_sub=4), "score_expect_kl: sub_ids given without sub_w (the two come together)"),
    "w-without-ids": (dict(sub_w=P, T=4, ld_sub=4), "score_expect_kl: sub_w given without sub_ids (the two come together)"),
    "T=0": (dict(sub_ids=P, sub_w=P, T=0, ld_sub=4), "score_expect_kl: T = 0 named rows per user (row stride 4), must be in [1, 128] with ld_sub >= T"),
    "T=129": (dict(sub_ids=P, sub_w=P, T=129, ld_sub=129),
              "score_expect_kl: T = 129 named rows per user (row stride 129), must be in [1, 128] with ld_sub >= T"),
    "ld_sub<T": (dict(sub_ids=P, sub_w=P, T=8, ld_sub=4),
                 "score_expect_kl: T = 8 named rows per user (row stride 4), must be in [1, 128] with ld_sub >= T"),
    "ld_out<N": (dict(ld_out=396), "score_expect_kl: out must be 16-byte aligned with ld_out = 396 >= N = 400"),
    "out-misaligned": (dict(out=P + 4), "score_expect_kl: out must be 16-byte aligned with ld_out = 400 >= N = 400"),
    "short-workspace": (dict(short_ws=True), "score_expect_kl: workspace holds 13172728 bytes, nr_score_expect_kl_workspace_bytes asks for "
                                             "13172736 (8-byte aligned)"),
}


@pytest.mark.parametrize("what", list(CALLS))
@pytest.mark.parametrize("rule", list(REFUSED), ids=str)
def test_bad_descriptor_is_refused_by_the_size_query_and_the_call(what, rule):
    fields, text = REFUSED[rule]
    assert _refusal(what, **fields) == (0, 1, text.format(what))


@pytest.mark.parametrize("what", list(CALLS))
@pytest.mark.parametrize("rule", list(REF_REFUSED), ids=str)
def test_bad_reference_side_is_refused_before_any_launch(what, rule):
    fields, text = REF_REFUSED[rule]
    size, rc, said = _refusal(what, **fields)
    assert (rc, said) == (1, text.format(what)) and size > 0


@pytest.mark.parametrize("rule", list(KL_CALL_ONLY), ids=str)
def test_bad_kl_call_is_refused_before_any_launch(rule):
    fields, text = KL_CALL_ONLY[rule]
    size, rc, said = _refusal("score_kl", **fields)
    assert (rc, said) == (1, text) and size > 0


@pytest.mark.parametrize("rule", list(EXPECT_KL_CALL_ONLY), ids=str)
def test_bad_expect_kl_call_is_refused_before_any_launch(rule):
    fields, text = EXPECT_KL_CALL_ONLY[rule]
    size, rc, said = _refusal("score_expect_kl", **fields)
    assert (rc, said) == (1, text) and size > 0


def test_null_descriptors_and_first_refusal_wins():
    lib = _lib.lib()
    for what, (_, _, fn) in CALLS.items():
        assert getattr(lib, fn + "_workspace_bytes")(None) == 0 and getattr(lib, fn)(None, None) == 1
        assert _lib.last_error() == f"{what}: null descriptor"
        assert _refusal(what, V=1, N=6, ref=None)[2] == REFUSED["V=1"][1].format(what)
        assert _refusal(what, base_max=None, ref=None)[2].startswith(f"{what}: null pointer (news_vecs")


def test_workspace_sizes():
    """K26: one fp64 quadruple per (user, slice), workgroups of 32 users up to N = 480, 16 up to 960, else 8; K27: K17's formula
    U * slices * (N * 4 + 8), workgroups of 32 users up to N = 416, 16 up to 832, else 8 -- the slices of splits = 0 fill 256 CUs."""
    lib = _lib.lib()
    kl = lambda N, U, V, s: lib.nr_score_kl_workspace_bytes(C.byref(_lib.KlDesc(**dict(K_BASE, ld_news=N, ld_user=N, ld_ref=N, N=N, U=U, V=V, splits=s))))
    xk = lambda N, U, V, s: lib.nr_score_expect_kl_workspace_bytes(
        C.byref(_lib.ExpectKlDesc(**dict(X_BASE, ld_news=N, ld_user=N, ld_ref=N, ld_out=N, N=N, U=U, V=V, splits=s))))
    assert kl(400, 70, 100001, 3) == 70 * 3 * 32 and kl(400, 1, 100001, 0) == 196 * 32 and kl(4, 1, 2, 0) == 32
    assert kl(4, 3, 1 + 128 * 256 + 5, 2) == 3 * 2 * 32 and kl(400, 65, 130, 3) == 0
    # auto slices: whole segments (196 of them at V = 100 001) grouped for about 256 / (user tiles) slices: 2, 4, 8 tiles give 98, 49, 28
    assert kl(400, 8192, 100001, 0) == 8192 * 32 and kl(480, 64, 100001, 0) == 64 * 98 * 32 and kl(484, 64, 100001, 0) == 64 * 49 * 32
    assert kl(960, 64, 100001, 0) == 64 * 49 * 32 and kl(964, 64, 100001, 0) == 64 * 28 * 32
    row = lambda N: N * 4 + 8
    assert xk(400, 70, 100001, 3) == 70 * 3 * row(400) and xk(400, 8192, 100001, 0) == 8192 * row(400) and xk(4, 1, 2, 0) == row(4)
    assert xk(416, 64, 100001, 0) == 64 * 98 * row(416) and xk(420, 64, 100001, 0) == 64 * 49 * row(420)
    assert xk(832, 64, 100001, 0) == 64 * 49 * row(832) and xk(836, 64, 100001, 0) == 64 * 28 * row(836)
    assert xk(400, 65, 130, 3) == 0


def test_descriptors_are_entries_24_and_25_of_abi_sizes_and_the_new_names_exist():
    sizes = (C.c_size_t * 26)()
    assert _lib.lib().nr_abi_sizes(sizes, 26) == 0
    assert sizes[24] == C.sizeof(_lib.KlDesc) and sizes[25] == C.sizeof(_lib.ExpectKlDesc)
    short = (C.c_size_t * 26)(*([12345] * 26))
    assert _lib.lib().nr_abi_sizes(short, 24) == 0 and short[24] == 12345 and short[25] == 12345 and list(short)[:24] == list(sizes)[:24]
    # the layouts: nr_entropy_desc up to base_logsum resp. nr_expect_affine_desc with the reference fields after beta; the shared tail
    tail = ["ws", "ws_bytes", "prior", "stamp", "window", "ld_window"]
    names = lambda t: [f[0] for f in t._fields_]
    ref = ["ref", "ld_ref", "ref_tau", "ref_tau_u", "ref_base_max", "ref_base_logsum"]
    assert names(_lib.KlDesc) == names(_lib.EntropyDesc)[:15] + ref + ["out_kl", "out_entropy", "out_cov", "out_mass"] + tail
    assert names(_lib.ExpectKlDesc) == names(_lib.ExpectAffineDesc)[:17] + ["gamma"] + ref + names(_lib.ExpectAffineDesc)[17:]
    assert names(_lib.ExpectKlDesc)[-6:] == tail
    common = ("news_vecs", "user_vecs", "ref_vecs", "temperature", "base", "ref_temperature", "ref_base", "exclude", "splits", "prior", "stamp", "window")
    for fn, want in ((ops.score_kl, common),
                     (ops.score_expect_kl, common + ("alpha", "beta", "gamma", "sub_ids", "sub_w", "scale_inv_tau")),
                     (ops.policy_kl, ("news_vecs", "user_vecs", "ref_vecs", "temperature", "ref_temperature", "mode", "exclude", "splits", "prior",
                                      "stamp", "window")),
                     (train.policy_kl, ("model", "ref", "news_vecs", "hist_idx", "mask", "temperature", "ref_temperature", "mode", "exclude_history",
                                        "batch_size", "prior", "news_time", "window", "seen")),
                     (metrics.kl_reference, ("news", "user", "ref", "tau", "ref_tau", "exclude", "prior", "stamp", "window")),
                     (metrics.expect_kl_reference, ("news", "user", "ref", "tau", "ref_tau", "exclude", "prior", "stamp", "window", "alpha", "beta",
                                                    "gamma", "sub_ids", "sub_w", "scale_inv_tau"))):
        assert tuple(inspect.signature(fn).parameters) == want


def test_policy_kl_refusals():
    news = torch.randn(10, 8)
    user = torch.randn(3, 8, requires_grad=True)
    ref = torch.randn(3, 8)
    with pytest.raises(RuntimeError, match=r"policy_kl: ref_vecs requires grad.*reference policy is a constant.*later policy_kl_joint"):
        ops.policy_kl(news, user, ref.clone().requires_grad_(True), 0.5)
    with pytest.raises(RuntimeError, match=r"policy_kl: news_vecs requires grad.*table is frozen.*later policy_kl_joint"):
        ops.policy_kl(news.clone().requires_grad_(True), user, ref, 0.5)
    with pytest.raises(RuntimeError, match=r"policy_kl: temperature requires grad, which mode='forward'"):
        ops.policy_kl(news, user, ref, torch.nn.Parameter(torch.tensor(0.5)), mode="forward")
    with pytest.raises(RuntimeError, match=r"policy_kl: ref_temperature requires grad"):
        ops.policy_kl(news, user, ref, 0.5, torch.nn.Parameter(torch.tensor(0.5)))
    with pytest.raises(RuntimeError, match=r"policy_kl: mode must be 'reverse'"):
        ops.policy_kl(news, user, ref, 0.5, mode="symmetric")
    with pytest.raises(RuntimeError, match=r"policy_kl: a temperature tensor must be floating point, 0-dim or of shape \(3,\)"):
        ops.policy_kl(news, user, ref, torch.ones(4))
    with pytest.raises(RuntimeError, match=r"no CPU fallback"):
        ops.policy_kl(news, user, ref, 0.5)
