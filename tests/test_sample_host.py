"""CPU: the host side of the sampled recommendation (include/nrhip.h, K12) -- metrics.philox4x32 against the published known
answers, metrics.sample_reference (temperature 0 is topk_reference; a hand-walked capped row; the Plackett-Luce law on 4096
users; seed and draw), the descriptor's place in nr_abi_sizes, the new names, and the refusals nr_score_sample makes before it
launches anything (fake non-null pointers: a launch would fault, a refusal does not)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from newsrecommendation_amd import _lib, metrics, ops, train
from sample_helpers import (CHI2_FIRST_MAX, CHI2_SECOND_MAX, LAW_DRAW, LAW_SEED, LAW_TAU, LAW_U, law_chi2, law_scores)

INF, NAN = float("inf"), float("nan")


def _words(text):
    return [int(w, 16) for w in text.split()]


KNOWN = [("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("counter,key,out", KNOWN, ids=["zeros", "ones", "pi"])
def test_philox4x32_known_answers(counter, key, out):
    got = metrics.philox4x32(np.array(_words(counter), dtype=np.uint64), np.array(_words(key), dtype=np.uint64))
    assert got.dtype == np.uint32 and got.tolist() == _words(out)


def test_philox4x32_broadcasts_and_noise_uses_the_documented_counter():
    ctr = np.array([_words(c) for c, _, _ in KNOWN], dtype=np.uint64)
    key = np.array([_words(k) for _, k, _ in KNOWN], dtype=np.uint64)
    assert metrics.philox4x32(ctr, key).tolist() == [_words(o) for _, _, o in KNOWN]
    # counter = (v >> 2, a, draw, 0), key = (seed lo, seed hi), word v & 3; news 4 .. 7 share a block
    seed, draw, a = 0x0123456789ABCDEF, 7, 2 ** 31 - 1
    g, bits = metrics.sample_noise_reference(seed, draw, np.full(4, a), np.arange(4, 8))
    block = metrics.philox4x32(np.array([1, a, draw, 0], dtype=np.uint64), np.array([0x89ABCDEF, 0x01234567], dtype=np.uint64))
    assert bits.tolist() == block.tolist() and bits.dtype == np.uint32
    u = ((bits >> 8).astype(np.float64) + 0.5) / 2.0 ** 24
    assert np.array_equal(g, -np.log(-np.log(u))) and np.all(np.isfinite(g))
    # the extremes of u: g is finite everywhere
    lo, hi = -np.log(-np.log(2.0 ** -25)), -np.log(-np.log(1.0 - 2.0 ** -25))
    assert -2.8524 < lo < -2.8523 and 17.3286 < hi < 17.3287


def _case(seed=3):
    rng = np.random.default_rng(seed)
    U, V = 9, 41
    scores = rng.standard_normal((U, V))
    scores[2, 7] = NAN
    prior = 0.3 * rng.standard_normal(V)
    prior[5], prior[9] = -INF, NAN
    stamp = rng.integers(0, 10, V)
    window = np.stack([rng.integers(0, 4, U), rng.integers(5, 10, U)], axis=1)
    window[4] = (6, 2)                                                 # an empty window
    group = rng.integers(-1, 4, V)
    exclude = [rng.choice(np.arange(1, V), size=rng.integers(0, 12), replace=False) for _ in range(U)]
    return scores, dict(prior=prior, stamp=stamp, window=window, group=group, group_cap=2, exclude=exclude)


def test_temperature_zero_is_topk_reference():
    scores, kw = _case()
    for k in (1, 7, 40):
        want = metrics.topk_reference(scores, k=k, **kw)
        for tau in (0.0, np.zeros(len(scores))):
            ids, pert, model = metrics.sample_reference(scores, k=k, temperature=tau, seed=99, draw=3, **kw)
            assert np.array_equal(ids, want[0]) and np.array_equal(pert, want[1]) and np.array_equal(model, want[1])
    assert ids.dtype == np.int32 and pert.dtype == np.float64 and model.dtype == np.float64


def test_hand_walked_capped_row_at_positive_temperature():
    """One user (key 11), news 1 .. 6 with scores x, groups (0, 0, 0, 1, 1, -1), cap 1, temperature 0.5.  The row, walked here
    in plain Python from the documented key x + 0.5 g: down the perturbed order, at most one news per group."""
    x = np.array([0.0, 1.0, 0.9, 0.8, 0.2, 0.1, -0.5])
    group = np.array([-1, 0, 0, 0, 1, 1, -1])
    seed, draw, key, tau = 2024, 5, 11, 0.5
    g, _ = metrics.sample_noise_reference(seed, draw, np.full(7, key), np.arange(7))
    pert = x + tau * g
    walk, used = [], set()
    for v in sorted(range(1, 7), key=lambda v: (-pert[v], v)):
        if group[v] >= 0 and group[v] in used:
            continue
        used.add(int(group[v]))
        walk.append(v)
    assert len(walk) == 3 and sorted(group[walk].tolist()) == [-1, 0, 1]
    ids, p, m = metrics.sample_reference(x[None, :], k=4, temperature=tau, seed=seed, draw=draw, user_keys=[key], group=group, group_cap=1)
    assert ids.tolist() == [walk + [0]] and np.array_equal(p[0, :3], pert[walk]) and p[0, 3] == -INF
    assert np.allclose(m[0, :3], x[walk], rtol=0, atol=1e-15) and m[0, 3] == -INF
    # the same user under another row index: the key decides, not the place
    two = metrics.sample_reference(np.tile(x, (2, 1)), k=4, temperature=tau, seed=seed, draw=draw, user_keys=[5, key], group=group, group_cap=1)
    assert np.array_equal(two[0][1], ids[0]) and np.array_equal(two[1][1], p[0])
    # a temperature that is negative, NaN or infinite: an all-fill row, the neighbour untouched
    bad = metrics.sample_reference(np.tile(x, (4, 1)), k=4, temperature=np.array([-1.0, NAN, INF, tau]), seed=seed, draw=draw,
                                   user_keys=[key] * 4, group=group, group_cap=1)
    assert not bad[0][:3].any() and np.all(bad[1][:3] == -INF) and np.all(bad[2][:3] == -INF) and np.array_equal(bad[0][3], ids[0])


@pytest.fixture(scope="module")
def law_rows():
    return metrics.sample_reference(law_scores(), k=2, temperature=LAW_TAU, seed=LAW_SEED, draw=LAW_DRAW, user_keys=np.arange(LAW_U))


def test_the_law_first_and_second_place(law_rows):
    """Gumbel top-k IS Plackett-Luce sampling: the first place follows softmax(x / tau), the second, given the first, the softmax
    over the rest.  Measured with this reference: 12.10 and 5.45 (897 users)."""
    chi1, chi2, n = law_chi2(law_rows[0])
    print(f"chi2 first place {chi1:.2f}, second place {chi2:.2f} over {n} users")
    assert chi1 <= CHI2_FIRST_MAX and chi2 <= CHI2_SECOND_MAX and n > 500


def test_the_law_configuration_has_few_near_ties(law_rows):
    """What tests/test_gpu_sample.py leans on when it asks 99 % of the device's first places to equal the reference's: a first
    place can differ between fp32 and fp64 only where the two best keys nearly tie."""
    gap = law_rows[1][:, 0] - law_rows[1][:, 1]
    assert np.mean(gap > 1e-5) >= 0.995


def test_seed_and_draw_change_the_rows(law_rows):
    for other in (dict(seed=LAW_SEED + 1, draw=LAW_DRAW), dict(seed=LAW_SEED, draw=LAW_DRAW + 1), dict(seed=LAW_SEED + (1 << 32), draw=LAW_DRAW)):
        ids, _, _ = metrics.sample_reference(law_scores(), k=2, temperature=LAW_TAU, user_keys=np.arange(LAW_U), **other)
        assert np.mean(ids[:, 0] != law_rows[0][:, 0]) >= 0.5, other
    again, _, _ = metrics.sample_reference(law_scores(), k=2, temperature=LAW_TAU, seed=LAW_SEED, draw=LAW_DRAW, user_keys=np.arange(LAW_U))
    assert np.array_equal(again, law_rows[0])


def test_descriptor_is_entry_10_of_abi_sizes():
    sizes = (C.c_size_t * 11)()
    assert _lib.lib().nr_abi_sizes(sizes, 11) == 0 and sizes[10] == C.sizeof(_lib.SampleDesc)
    assert sizes[7] == C.sizeof(_lib.TopkDesc) and sizes[9] == C.sizeof(_lib.MmrDesc)
    ten = (C.c_size_t * 11)()
    ten[10] = 12345
    assert _lib.lib().nr_abi_sizes(ten, 10) == 0 and ten[10] == 12345 and list(ten)[:10] == list(sizes)[:10]
    assert _lib.SampleDesc.topk.offset == 0 and _lib.SampleDesc.topk.size == C.sizeof(_lib.TopkDesc)


def test_new_names_and_signatures():
    for name in ("nr_score_sample_workspace_bytes", "nr_score_sample", "nr_sample_noise"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert list(inspect.signature(ops.score_sample).parameters) == [
        "news_vecs", "user_vecs", "k", "temperature", "seed", "draw", "user_keys", "exclude", "splits", "prior", "stamp", "window", "group",
        "group_cap"]
    assert list(inspect.signature(ops.sample_noise).parameters) == ["seed", "draw", "user_keys", "news_ids"]
    assert list(inspect.signature(train.recommend_sample).parameters) == [
        "model", "news_vecs", "hist_idx", "mask", "k", "temperature", "seed", "draw", "user_keys", "exclude_history", "batch_size", "prior",
        "news_time", "window", "news_group", "group_cap", "seen"]
    defaults = inspect.signature(train.recommend_sample).parameters
    assert defaults["draw"].default == 0 and defaults["exclude_history"].default is True and defaults["batch_size"].default == 8192
    kinds = inspect.signature(metrics.sample_reference).parameters
    assert list(kinds)[:2] == ["a", "b"] and all(kinds[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(kinds)[2:])
    assert list(kinds)[2:7] == ["k", "temperature", "seed", "draw", "user_keys"]
    # score_topk and recommend keep their argument lists
    assert list(inspect.signature(ops.score_topk).parameters) == ["news_vecs", "user_vecs", "k", "exclude", "splits", "prior", "stamp", "window",
                                                                  "group", "group_cap"]


TOPK = dict(news_vecs=4096, ld_news=400, V=100001, user=4096, ld_user=400, U=8192, N=400, k=10, out_ids=4096, out_scores=4096)
REFUSED = [(dict(tau=-0.5), {}, "tau"), (dict(tau=NAN), {}, "tau"), (dict(tau=INF), {}, "tau"), (dict(tau=-INF), {}, "tau"),
           (dict(tau=1.0), dict(k=0), "k = 0"), (dict(tau=1.0), dict(k=129), "k = 129"),
           (dict(tau=1.0), dict(group=4096), "group_cap = 0"), (dict(tau=1.0), dict(group=4096, group_cap=129), "group_cap = 129"),
           (dict(tau=1.0), dict(group_cap=3), "without group"), (dict(tau=1.0), dict(stamp=4096), "stamp given without window"),
           (dict(tau=1.0), dict(splits=-1), "splits = -1")]


@pytest.mark.parametrize("sample,topk,message", REFUSED, ids=[f"{i}-{'-'.join(list(s) + list(t))}" for i, (s, t, _) in enumerate(REFUSED)])
def test_refused_before_any_launch(sample, topk, message):
    d = _lib.SampleDesc(topk=_lib.TopkDesc(**{**TOPK, **topk}), seed=1, draw=0, **sample)
    lib = _lib.lib()
    assert lib.nr_score_sample_workspace_bytes(C.byref(d)) == 0 and message in _lib.last_error(), _lib.last_error()
    assert lib.nr_score_sample(C.byref(d), None) == 1 and message in _lib.last_error(), _lib.last_error()


def test_workspace_is_the_plain_call_s_and_null_descriptor():
    lib = _lib.lib()
    for splits, k in ((3, 10), (7, 128), (0, 10)):
        t = _lib.TopkDesc(**{**TOPK, "splits": splits, "k": k})
        d = _lib.SampleDesc(topk=t, seed=1, draw=0, tau=0.25)
        want = lib.nr_score_topk_workspace_bytes(C.byref(t))
        assert want > 0 and lib.nr_score_sample_workspace_bytes(C.byref(d)) == want
        if splits:
            assert want == 8192 * splits * k * 8
    # a per-user tau replaces the scalar, which is then not looked at
    d = _lib.SampleDesc(topk=_lib.TopkDesc(**TOPK), seed=1, draw=0, tau=NAN, tau_u=4096)
    assert lib.nr_score_sample_workspace_bytes(C.byref(d)) > 0
    assert lib.nr_score_sample_workspace_bytes(None) == 0 and "null descriptor" in _lib.last_error()
    assert lib.nr_score_sample(None, None) == 1
    assert lib.nr_sample_noise(1, 0, None, None, -1, None, None, None) == 1 and "n = -1" in _lib.last_error()
    assert lib.nr_sample_noise(1, 0, None, None, 4, None, None, None) == 1 and "null pointer" in _lib.last_error()
    assert lib.nr_sample_noise(1, 0, None, None, 0, None, None, None) == 0


def test_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_sample(torch.zeros(10, 8), torch.zeros(3, 8), 2, 0.5, seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_noise(1, 0, torch.zeros(4, dtype=torch.int32), torch.ones(4, dtype=torch.int32))
