"""GPU: full-corpus rank evaluation (nr_score_rank / ops.score_rank / train.rank_eval / train.rank_shard) against the host
statement of its contract, metrics.rank_reference, and against nr_score_topk, whose order and score bits it must share.

Integer-valued vectors make every dot product an exact fp32 integer in any summation order, with plenty of ties: ranks AND
scores must then equal the reference exactly, which pins the tie rule, the tile tails on both axes, the chunk and slice
boundaries and the sum over slices.  Float data is checked bitwise against ops.score_topk and, against float64 scores, with
the project's fp32 bound of 1e-4 on a score, hence 2e-4 on a comparison of two scores.  The user tile of the counting pass is
64 users (N = 24, N = 400) or 16 (N = 1024)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from helpers import build_model
from oracle import nr_oracle as O
from newsrecommendation_amd import _lib, metrics, ops, train as TR
from newsrecommendation_amd.data import IndexedTestShard

pytestmark = pytest.mark.gpu

TOL = 1e-4
US, TS, SPLITS = (1, 17, 64, 65), (1, 5, 64), (0, 1, 3, 7)
bits = lambda a: np.ascontiguousarray(a).view(np.int32)


def _ints(V, U, N, seed):
    g = torch.Generator().manual_seed(seed)
    news = torch.randint(-2, 3, (V, N), generator=g).float()
    user = torch.randint(-2, 3, (U, N), generator=g).float()
    return news, user


def _floats(V, U, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(V, N, generator=g) * 0.4, torch.randn(U, N, generator=g) * 0.4


def _run(news, user, targets, exclude=None, ks=(), splits=0):
    tg = torch.as_tensor(targets, dtype=torch.int32).cuda()
    ex = None if exclude is None else torch.as_tensor(exclude, dtype=torch.int32).cuda()
    ranks, sc, sums = ops.score_rank(news, user, tg, exclude=ex, ks=ks, splits=splits)
    assert ranks.dtype == torch.int32 and sc.dtype == torch.float32 and ranks.shape == sc.shape == tuple(tg.shape)
    return ranks.cpu().numpy(), sc.cpu().numpy(), None if sums is None else sums.cpu().numpy()


def _same(ranks, sc, ref_r, ref_s):
    """Ranks equal; scores equal where ranked, -inf where not."""
    return np.array_equal(ranks, ref_r) and np.array_equal(sc.astype(np.float64), ref_s)


def _targets(news, user, V, seed):
    """[U, 64]: the user's best news, a zero, V - 1, a repeat of the best, the user's worst news (the first five columns); then
    its second and third best, the ids at chunk edges (1, 128, 129 -- out of range for a small table), another zero, random ids."""
    U = user.shape[0]
    order = metrics.topk_reference(news.numpy(), user.numpy(), k=V - 1)[0]
    g = np.random.default_rng(seed)
    t = g.integers(1, V, (U, 64)).astype(np.int32)
    t[:, 0], t[:, 1], t[:, 2], t[:, 3], t[:, 4] = order[:, 0], 0, V - 1, order[:, 0], order[:, -1]
    t[:, 5], t[:, 6] = order[:, min(1, V - 2)], order[:, min(2, V - 2)]
    t[:, 7], t[:, 8], t[:, 9], t[:, 10] = 1, 128, 129, 0
    return t


@pytest.mark.parametrize("V", [2, 17, 1000, 4099])
@pytest.mark.parametrize("N", [24, 400])
def test_exact_grid(N, V):
    """U in {1, 17, 64, 65} x T in {1, 5, 64} x splits in {0, 1, 3, 7}: ranks and scores equal the reference exactly.  One
    reference per (N, V): 64 targets of 65 users; a smaller T is its first columns (a repeat only looks at earlier entries), a
    smaller U its first rows."""
    news, user = _ints(V, 65, N, seed=1000 * N + V)
    tg = _targets(news, user, V, seed=V)
    ref_r, ref_s = metrics.rank_reference(news.numpy(), user.numpy(), targets=tg)
    assert (ref_r[:, 0] == 1).all() and (ref_r[:, 3] == 0).all() and (ref_r[:, 1] == 0).all()
    if V > 2:
        assert ((ref_r[:, 4] == V - 1) | (tg[:, 4] == tg[:, 2])).all()                              # the worst news is last
    news_d, user_d = news.cuda(), user.cuda()
    for U in US:
        for T in TS:
            for splits in SPLITS:
                ranks, sc, _ = _run(news_d, user_d[:U].contiguous(), tg[:U, :T], splits=splits)
                assert _same(ranks, sc, ref_r[:U, :T], ref_s[:U, :T]), (U, T, splits)


def test_exact_widest_vectors():
    """N = 1024, the widest the call takes: the 16-user tile, 32 k-slabs."""
    news, user = _ints(1000, 33, 1024, seed=5)
    tg = _targets(news, user, 1000, seed=6)[:, :12]
    ref_r, ref_s = metrics.rank_reference(news.numpy(), user.numpy(), targets=tg)
    for splits in (0, 3):
        ranks, sc, _ = _run(news.cuda(), user.cuda(), tg, splits=splits)
        assert _same(ranks, sc, ref_r, ref_s), splits


def test_exclusion_list():
    """E = 8: each user's three best news (so every rank moves), a duplicate, zeros, an id >= V, a negative id, and one entry
    that is a target -- which is then not ranked."""
    news, user = _ints(1000, 65, 24, seed=21)
    tg = _targets(news, user, 1000, seed=22)[:, :16]
    order = metrics.topk_reference(news.numpy(), user.numpy(), k=4)[0]
    ex = np.zeros((65, 8), np.int32)
    ex[:, 0], ex[:, 2], ex[:, 5] = order[:, 1], order[:, 2], order[:, 3]
    ex[:, 3] = order[:, 1]
    ex[:, 4] = tg[:, 11]                                                     # a target
    ex[:, 6] = 1000 + np.arange(65)
    ex[:, 7] = -5
    ref_r, ref_s = metrics.rank_reference(news.numpy(), user.numpy(), targets=tg, exclude=ex)
    plain = metrics.rank_reference(news.numpy(), user.numpy(), targets=tg)[0]
    assert (ref_r[:, 11] == 0).all() and (ref_r[:, 5] == 0).all() and (ref_r[:, 0] == 1).all() and not np.array_equal(ref_r, plain)
    for splits in (0, 1, 3):
        ranks, sc, _ = _run(news.cuda(), user.cuda(), tg, exclude=ex, splits=splits)
        assert _same(ranks, sc, ref_r, ref_s), splits


def test_exclusion_of_all_but_two():
    """E = 64, V = 67: of the 66 eligible news all but two (per user other ones) are excluded; every id is a target."""
    news, user = _ints(67, 17, 24, seed=22)
    g = np.random.default_rng(3)
    ex = np.stack([g.permutation(np.arange(1, 67))[:64] for _ in range(17)]).astype(np.int32)
    tg = np.tile(np.arange(1, 65, dtype=np.int32), (17, 1))
    tg[:, :2] = [65, 66]
    ref_r, ref_s = metrics.rank_reference(news.numpy(), user.numpy(), targets=tg, exclude=ex)
    assert set(np.unique(ref_r)) <= {0, 1, 2}
    for splits in (0, 1, 3):
        ranks, sc, _ = _run(news.cuda(), user.cuda(), tg, exclude=ex, splits=splits)
        assert _same(ranks, sc, ref_r, ref_s), splits


def test_nan_news_is_not_ranked_and_disturbs_nothing():
    news, user = _ints(1000, 65, 24, seed=41)
    bad = 333
    tg = _targets(news, user, 1000, seed=42)[:, :12]
    tg[:, 11] = bad
    ref_r, ref_s = metrics.rank_reference(news.numpy(), user.numpy(), targets=tg, exclude=np.full((65, 1), bad))
    news[bad] = float("nan")
    ex = np.tile(np.array([[bad, 7]], np.int32), (65, 1))                     # an excluded NaN news must not be taken back
    ref_x = metrics.rank_reference(news.numpy(), user.numpy(), targets=tg, exclude=ex)
    for splits in (0, 1, 3):
        ranks, sc, _ = _run(news.cuda(), user.cuda(), tg, splits=splits)
        assert (ranks[:, 11] == 0).all() and np.isneginf(sc[:, 11]).all() and not np.isnan(sc).any()
        assert _same(ranks, sc, ref_r, ref_s), splits
        ranks, sc, _ = _run(news.cuda(), user.cuda(), tg, exclude=ex, splits=splits)
        assert _same(ranks, sc, ref_x[0], ref_x[1]), splits


def _rank_of_rows(news_d, user_d, rows, exclude, splits=0):
    """score_rank over target rows wider than 64: blocks of 64 columns."""
    out = [_run(news_d, user_d, rows[:, a:a + 64], exclude=exclude, splits=splits)[:2] for a in range(0, rows.shape[1], 64)]
    return np.concatenate([o[0] for o in out], 1), np.concatenate([o[1] for o in out], 1)


@pytest.mark.parametrize("with_exclusion", [False, True])
def test_agrees_with_score_topk_bitwise(with_exclusion):
    """Targets = each user's whole top-128 row plus 64 random ids: 1 <= rank <= k exactly when the target is in the top-k row,
    at place rank - 1, with the bits of the top-k score."""
    news, user = _floats(4099, 65, 400, seed=11)
    news_d, user_d = news.cuda(), user.cuda()
    ex = None
    if with_exclusion:
        first = ops.score_topk(news_d, user_d, 3)[0].cpu().numpy()
        ex = np.concatenate([first, np.random.default_rng(5).integers(1, 4099, (65, 40)).astype(np.int32)], 1)
    ex_d = None if ex is None else torch.from_numpy(ex).cuda()
    ids, tsc = (t.cpu().numpy() for t in ops.score_topk(news_d, user_d, 128, exclude=ex_d))
    rnd = np.random.default_rng(6).integers(1, 4099, (65, 64)).astype(np.int32)
    rows = np.concatenate([ids, rnd], 1)
    ranks, sc = _rank_of_rows(news_d, user_d, rows, ex)
    assert np.array_equal(ranks[:, :128], np.tile(np.arange(1, 129), (65, 1)))
    assert np.array_equal(bits(sc[:, :128]), bits(tsc))
    for k in (1, 10, 128):
        for u in range(65):
            row = ids[u, :k].tolist()
            for j in range(128, 192):
                t, r = rows[u, j], ranks[u, j]
                # (a random id that repeats an earlier entry of its 64-column block is not ranked; it is then no statement)
                if r == 0:
                    assert t in rnd[u, :j - 128].tolist() or (ex is not None and t in ex[u].tolist()), (u, j)
                    continue
                assert (1 <= r <= k) == (t in row), (u, j, k)
                if r <= k:
                    assert ids[u, r - 1] == t and bits(sc[u, j:j + 1])[0] == bits(tsc[u, r - 1:r])[0]


def test_position_independence_is_bitwise():
    """Ranks and score bits do not depend on the corpus slices, the place in a user tile or the other users."""
    news, user = _floats(4099, 17, 400, seed=31)
    news_d = news.cuda()
    tg = np.concatenate([ops.score_topk(news_d, user.cuda(), 20)[0].cpu().numpy(),
                         np.random.default_rng(7).integers(1, 4099, (17, 20)).astype(np.int32)], 1)
    r1, s1, _ = _run(news_d, user.cuda(), tg, splits=1)
    assert np.array_equal(r1[:, :20], np.tile(np.arange(1, 21), (17, 1)))
    r5, s5, _ = _run(news_d, user.cuda(), tg, splits=5)
    assert np.array_equal(r5, r1) and np.array_equal(bits(s5), bits(s1))
    perm = torch.randperm(17, generator=torch.Generator().manual_seed(1)).numpy()
    rp, sp, _ = _run(news_d, user[perm].cuda(), tg[perm], splits=1)
    assert np.array_equal(rp, r1[perm]) and np.array_equal(bits(sp), bits(s1[perm]))
    extra = _floats(1, 47, 400, seed=32)[1]
    pad = np.random.default_rng(8).integers(1, 4099, (47, 40)).astype(np.int32)
    rw, sw, _ = _run(news_d, torch.cat([user, extra]).cuda(), np.concatenate([tg, pad]), splits=5)      # U padded from 17 to 64
    assert np.array_equal(rw[:17], r1) and np.array_equal(bits(sw[:17]), bits(s1))
    rs, ss, _ = _run(news_d, torch.cat([extra[:30], user]).cuda(), np.concatenate([pad[:30], tg]), splits=0)      # shifted inside the tile
    assert np.array_equal(rs[30:], r1) and np.array_equal(bits(ss[30:]), bits(s1))


def _check_band(ranks, sc, r, targets, banned=None, min_exact=None):
    """The tolerance-band rule.  r: float64 scores [U, V]; every device rank of a ranked target lies in
    [1 + #{r_v > r_t + 2 TOL}, 1 + #{r_v >= r_t - 2 TOL}] over the eligible v != t, and its score within TOL of r_t; what the
    contract does not rank has rank 0.  Returns the widths of the bands."""
    U, V = r.shape
    ref = metrics.rank_reference(r, targets=targets, exclude=None if banned is None else [sorted(b) for b in banned])[0]
    widths = []
    for u in range(U):
        ok = np.ones(V, bool)
        ok[0] = False
        if banned is not None:
            ok[np.array(sorted(banned[u]), dtype=np.int64)] = False
        for j, t in enumerate(targets[u]):
            if ref[u, j] == 0:
                assert ranks[u, j] == 0 and np.isneginf(sc[u, j]), (u, j)
                continue
            others = ok.copy()
            others[t] = False
            lo = 1 + int((r[u, others] > r[u, t] + 2 * TOL).sum())
            hi = 1 + int((r[u, others] >= r[u, t] - 2 * TOL).sum())
            assert lo <= ref[u, j] <= hi
            assert lo <= ranks[u, j] <= hi, (u, j, lo, int(ranks[u, j]), hi)
            assert abs(sc[u, j] - r[u, t]) <= TOL, (u, j)
            widths.append(hi - lo)
    return np.array(widths)


def test_float_data_within_the_fp32_bound():
    news, user = _floats(4099, 65, 400, seed=11)
    r = user.double().numpy() @ news.double().numpy().T
    tg = np.random.default_rng(11).integers(1, 4099, (65, 5)).astype(np.int32)
    ranks, sc, _ = _run(news.cuda(), user.cuda(), tg)
    widths = _check_band(ranks, sc, r, tg)
    print("bands:", len(widths), "exact:", int((widths == 0).sum()), "widest:", int(widths.max()))
    assert (widths == 0).sum() >= 0.75 * len(widths) and widths.max() <= 4          # the band is not vacuous


def _rank_into(news_d, user_d, tg_d, ks, sums, splits):
    """nr_score_rank through the descriptor, writing the sums into the caller's device buffer `sums`; returns the ranks."""
    (V, N), (U, T) = news_d.shape, tg_d.shape
    ranks = torch.empty(U, T, dtype=torch.int32, device="cuda")
    sc = torch.empty(U, T, dtype=torch.float32, device="cuda")
    d = _lib.RankDesc(news_vecs=news_d.data_ptr(), ld_news=N, V=V, user=user_d.data_ptr(), ld_user=N, U=U, N=N, T=T, targets=tg_d.data_ptr(),
                      ld_targets=T, exclude=None, ld_exclude=0, E=0, splits=splits, ks=(C.c_int * max(len(ks), 1))(*ks), n_ks=len(ks),
                      out_ranks=ranks.data_ptr(), out_scores=sc.data_ptr(), out_sums=sums.data_ptr())
    ws = torch.empty(_lib.lib().nr_score_rank_workspace_bytes(C.byref(d)) // 4 + 1, dtype=torch.int32, device="cuda")
    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 4
    assert _lib.lib().nr_score_rank(C.byref(d), torch.cuda.current_stream().cuda_stream) == 0, _lib.last_error()
    return ranks.cpu().numpy()


def test_sums():
    """out_sums against retrieval_metrics_reference applied to the device's own ranks (fp64 summation order only: 1e-9), with
    users that have no ranked target, for four cut-offs and for none.  Overwritten, not accumulated: ONE device buffer, filled
    with NaN, takes the sums of two calls in a row (other users in the second) and equals the reference after each."""
    news, user = _ints(1000, 65, 24, seed=61)
    tg = _targets(news, user, 1000, seed=62)[:, :12]
    tg[3] = 0
    tg[40, :] = [0, 1000, -4, 0, 0, 0, 0, 0, 0, 0, 0, 2000]
    news_d, user_d = news.cuda(), user.cuda()
    tg_d = torch.from_numpy(tg).cuda()
    for ks in ((1, 5, 10, 100), ()):
        ranks, _, sums = _run(news_d, user_d, tg, ks=ks)
        assert (ranks[3] == 0).all() and (ranks[40] == 0).all()
        want = metrics.retrieval_metrics_reference(ranks, ks)[1]
        assert sums.shape == (2 + 2 * len(ks),) and sums[0] == 63 and np.allclose(sums, want, rtol=1e-9, atol=0)
        again = _run(news_d, user_d, tg, ks=ks, splits=3)[2]
        assert np.array_equal(again, sums)
        buf = torch.full((2 + 2 * len(ks),), float("nan"), dtype=torch.float64, device="cuda")
        for U, splits in ((65, 0), (30, 3), (65, 1)):                        # 63, 29 and again 63 users counted
            r = _rank_into(news_d, user_d[:U].contiguous(), tg_d[:U].contiguous(), ks, buf, splits)
            assert np.array_equal(r, ranks[:U])
            want_u = metrics.retrieval_metrics_reference(r, ks)[1]
            got = buf.cpu().numpy()
            assert got[0] == (63 if U == 65 else 29) and np.allclose(got, want_u, rtol=1e-9, atol=0), (U, splits, got, want_u)
        assert np.array_equal(buf.cpu().numpy(), sums)
    assert _run(news_d, user_d, tg, ks=None)[2] is None
    r0, s0, sums0 = ops.score_rank(news_d, user_d[:0], torch.zeros(0, 4, dtype=torch.int32).cuda(), ks=(5,))
    assert r0.shape == s0.shape == (0, 4) and sums0.cpu().tolist() == [0, 0, 0, 0]


def _corpus(tag, n_news, seed):
    g = torch.Generator().manual_seed(seed)
    if tag.startswith("nrms"):
        nc = torch.randint(1, 12, (n_news + 1, 4), generator=g, dtype=torch.int32)       # word ids of a 12-word vocabulary
        cut = torch.randint(1, 5, (n_news + 1,), generator=g)
        nc[torch.arange(4)[None, :] >= cut[:, None]] = 0                                  # titles of 1 .. 4 words
    else:
        nc = torch.stack([torch.randint(1, 9, (n_news + 1,), generator=g), torch.randint(0, 5, (n_news + 1,), generator=g),
                          torch.randint(0, 7, (n_news + 1,), generator=g)], dim=1).to(torch.int32)
    nc[0] = 0
    return nc


@pytest.mark.parametrize("tag", ["nrms_tiny_mask", "naml_tiny_3view"])
def test_rank_eval_end_to_end_against_the_oracle(tag, tmp_path):
    """encode_news over 300 synthetic news, train.rank_eval for 40 users (an empty history, a full one, a user with 70 targets
    and clicked targets among them) against the oracle's user vectors and float64 scoring of the whole corpus; train.rank_shard
    on a small shard file."""
    model, z, cfg, sd = build_model(tag, "fp32")
    n_news, U, H = 300, 40, cfg.user_log_length
    nc = _corpus(tag, n_news, seed=51)
    g = torch.Generator().manual_seed(52)
    hist = torch.randint(1, n_news + 1, (U, H), generator=g, dtype=torch.int32)
    mask = torch.ones(U, H)
    for u in range(U):                                                       # front padded; user 0 has no history, user 1 a full one
        n_pad = 0 if u == 1 else H if u == 0 else int(torch.randint(0, H, (1,), generator=g))
        hist[u, :n_pad], mask[u, :n_pad] = 0, 0
    rng = np.random.default_rng(53)
    tg = np.zeros((U, 70), np.int32)
    tg[:, :4] = rng.integers(1, n_news + 1, (U, 4))
    tg[2] = rng.permutation(np.arange(1, n_news + 1))[:70]                   # 70 targets: the row split
    tg[1, :4] = [v for v in range(1, 5) if v != int(hist[1, -1])][:3] + [0]
    tg[1, 2], tg[1, 3] = int(hist[1, -1]), tg[1, 2]                          # a clicked target among three others
    tg[5, 1] = 0
    news_vecs = TR.encode_news(model, nc, 64, torch.device("cuda"))

    news_enc, user_enc = (O.nrms_news_encoder, O.nrms_user_encoder) if tag.startswith("nrms") else (O.naml_news_encoder, O.naml_user_encoder)
    with torch.no_grad():
        nv = news_enc(nc.long(), sd, cfg)
        uv = user_enc(nv[hist.long()], mask, sd, cfg)
    r = uv.double().numpy() @ nv.double().numpy().T

    clicked = [set(hist[u][mask[u] != 0].tolist()) for u in range(U)]
    ks = (1, 10, 100)
    for exclude_history in (True, False):
        ranks, sc, sums = TR.rank_eval(model, news_vecs, hist.numpy(), mask.numpy(), tg, ks=ks, exclude_history=exclude_history)
        assert ranks.is_cuda and sums.is_cuda and ranks.shape == sc.shape == (U, 70) and sums.dtype == torch.float64
        ranks, sc = ranks.cpu().numpy(), sc.cpu().numpy()
        _check_band(ranks, sc, r, tg, banned=clicked if exclude_history else None)
        assert (ranks[1, 2] == 0) == exclude_history and ranks[0, 0] > 0 and ranks[5, 1] == 0
        assert (ranks[2] > 0).sum() == 70 - (len(clicked[2] & set(tg[2].tolist())) if exclude_history else 0)
        assert np.allclose(sums.cpu().numpy(), metrics.retrieval_metrics_reference(ranks, ks)[1], rtol=1e-9, atol=0)
        narrow = TR.rank_eval(model, news_vecs, hist.numpy(), mask.numpy(), tg[:, :4], ks=ks, exclude_history=exclude_history)
        keep = np.arange(U) != 2                                             # the same ranks through the kernel's own sums
        assert np.array_equal(narrow[0].cpu().numpy()[keep], ranks[keep, :4])
        assert np.allclose(narrow[2].cpu().numpy(), metrics.retrieval_metrics_reference(narrow[0].cpu().numpy(), ks)[1], rtol=1e-9, atol=0)

    # a shard file of 12 impressions: its targets are cand[label == 1] per impression
    lines = []
    for i in range(12):
        h = " ".join(f"N{v}" for v in hist[i][mask[i] != 0].tolist())
        cand = rng.permutation(np.arange(1, n_news + 1))[:6]
        lab = [1, 0, 0, int(i % 3 == 0), 0, 0]
        lines.append(f"{i}\tU{i}\tt\t{h}\t" + " ".join(f"N{c}-{l}" for c, l in zip(cand, lab)) + "\n")
    path = tmp_path / "behaviors_0.tsv"
    path.write_text("".join(lines))
    shard = IndexedTestShard(str(path), {f"N{v}": v for v in range(1, n_news + 1)}, types.SimpleNamespace(user_log_length=H))
    want_tg = np.zeros((12, 2), np.int32)
    for i in range(12):
        c = shard.cand[shard.offsets[i]:shard.offsets[i + 1]][shard.label[shard.offsets[i]:shard.offsets[i + 1]] == 1]
        want_tg[i, :len(c)] = c
    assert np.array_equal(TR._shard_targets(shard), want_tg) and (want_tg[:, 0] > 0).all() and (want_tg[::3, 1] > 0).all()
    got = TR.rank_shard(model, news_vecs, shard, ks=ks)
    same = TR.rank_eval(model, news_vecs, shard.hist, shard.mask, want_tg, ks=ks)
    assert np.array_equal(got[0].cpu().numpy(), same[0].cpu().numpy()) and np.array_equal(got[2].cpu().numpy(), same[2].cpu().numpy())
    assert np.array_equal(shard.hist, hist[:12].numpy())
    _check_band(got[0].cpu().numpy(), got[1].cpu().numpy(), r[:12], want_tg, banned=clicked[:12])
