"""CPU proof of the corpus sweep (tests/test_gpu_corpus_sweep.py): its case tables, its references and the power of its checker
(all in the first part of that file).  Nothing here touches a GPU.

  (a) the file's references equal the host statements of metrics.py on the case tables: topk_reference, rank_reference,
      mmr_reference, sample_reference (the noise in fp64), the Philox words and the Gumbel values;
  (b) the route functions put at least two cases in every route and the tables hold what the issue lists;
  (c) in every Gaussian case at least 90 % of the rows are decided in every place and every user tile holds a decided row;
  (d) a fp32 numpy stand-in for every entry point, reading its buffers through the strides of the descriptor, passes every layer
      of every case, summing in slab order (the chain of csrc/nr_score_tile.h and csrc/nr_mmr.hip, fma by fma) and with float64
      accumulation rounded once;
  (e) each of eighteen mutants fails the layer named; so do a device that flushes subnormal products (`special`), a rank pass
      that sums in another order than the selection and a sampled prior formed with one fma (`agree`; `exact` on the lattice), a
      second run that differs in one bit (`repeat`), a result that depends on the strides (`layout`), a score at 1.5 times its
      bound (`bound`), sums beyond their bound (`sums`), a wrong Philox word or a g beyond the header's bound (`noise`);
  (f) the refusals the library decides before the device guard, with dummy pointers.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_corpus_sweep as H
from newsrecommendation_amd import _lib, metrics

DEV = "cpu"
TK = {c.name: c for c in H.topk_cases()}
RK = {c.name: c for c in H.rank_cases()}
MM = {c.name: c for c in H.mmr_cases()}
f32, f64, i32 = np.float32, np.float64, np.int32
INF, NAN = float("inf"), float("nan")


# ------------------------------------------------------------------------------------------ the stand-ins
def rd(b, rows, cols, ld):
    """[rows, cols] read from buffer b at row stride ld, as a kernel given that stride would: from the payload's first element on."""
    f = b.flat[b.start:].numpy()
    return np.stack([f[r * ld:r * ld + cols] for r in range(rows)]) if rows else np.zeros((0, cols), f.dtype)


def fma32(a, b, acc):
    """fp32 a b + acc with one rounding (the product of two fp32 values is exact in fp64)."""
    with np.errstate(all="ignore"):
        return (a.astype(f64) * b.astype(f64) + acc.astype(f64)).astype(f32)


def tile_order(N):
    """The chain of ScoreTile::chunk: k-slab, half of the slab's two float4 reads, sub-step e, MFMA k-group g."""
    return [ks * 32 + 8 * g + 4 * h + e for ks in range(H.tk_npad(N) // 32) for h in range(2) for e in range(4) for g in range(4)]


def mmr_order(N):
    """The chain of mmr_select_kernel: k-slab, q, sub-step e, lane half h."""
    return [ks * 32 + 8 * q + 4 * h + e for ks in range((N + 31) // 32) for q in range(4) for e in range(4) for h in range(2)]


def chain(A, B, N, order, acc64, limit=None):
    """out[i, j] = sum over the columns of A[i] B[j] in the given order, zeros from column `limit` (N) on: one fma per column, or
    float64 accumulation rounded once."""
    limit = N if limit is None else limit
    with np.errstate(all="ignore"):
        if acc64:
            return (A[:, :limit].astype(f64) @ B[:, :limit].astype(f64).T).astype(f32)
        acc = np.zeros((A.shape[0], B.shape[0]), f32)
        for col in order:
            acc = fma32(A[:, col:col + 1], B[None, :, col], acc) if col < limit else acc + f32(0)
        return acc


def _dots(P, mutant, acc64):
    c, S = P.c, P.S
    lim = c.N + 4 if mutant == "float4_past_N" else c.N
    user, news = rd(P.inb["user"], c.U, lim, S.user), rd(P.inb["news"], c.V, lim, S.news)
    return chain(user, news, c.N, tile_order(c.N), acc64, lim)


def _pool(P, S, mutant):
    """(prior [V] or None, in-window [U, V] bool) as pool_key reads them."""
    c = P.c
    prior = P.inb["prior"].v[0].numpy() if "prior" in P.inb else None
    inwin = np.ones((c.U, c.V), bool)
    if "stamp" in P.inb:
        stamp, win = P.inb["stamp"].v[0].numpy(), rd(P.inb["window"], c.U, 2, 2 if mutant == "two_for_ld_window" else S.win)
        inwin = (win[:, :1] <= stamp[None, :]) & ((stamp[None, :] < win[:, 1:2]) if mutant == "window_hi_exclusive" else (stamp[None, :] <= win[:, 1:2]))
    if prior is not None:
        inwin &= ~np.isneginf(prior)[None, :]
    return prior, inwin


def _lists(P, S, mutant):
    """Per user the ids it must not be given."""
    c = P.c
    out = [np.zeros(0, np.int64) for _ in range(c.U)]
    if "exclude" in P.inb:
        ex = rd(P.inb["exclude"], c.U, c.E, c.E if mutant == "E_for_ld_exclude" else S.excl)
        out = [ex[u].astype(np.int64) for u in range(c.U)]
    if "offsets" in P.inb:
        off, ids = P.inb["offsets"].v[0].numpy(), P.inb["xids"].v[0].numpy()
        n = len(ids)
        for u in range(c.U):
            b = min(max(int(off[u]), 0), n)
            out[u] = ids[b:max(min(int(off[u + 1]), n), b)].astype(np.int64)
    return [x[(x >= 1) & (x < c.V)] for x in out]


def _order(s, ok, mutant):
    """The eligible ids of one user in the kernel's key order: score descending (-0 folded onto +0), id ascending."""
    with np.errstate(all="ignore"):
        if mutant == "nan_news_returned":
            s = np.where(np.isnan(s), f32(-INF), s)
        if mutant == "neg_inf_as_fill":
            ok = ok & ~np.isneginf(s)
        idx = np.flatnonzero(ok & ~np.isnan(s))
        key = s[idx].astype(f64)
        if mutant == "neg_zero_below":
            key = np.where((key == 0) & np.signbit(key), -1e-300, key)
        return idx[np.lexsort((-idx if mutant == "ties_desc_id" else idx, -key))]


def _walk(order, group, cap, mutant, excluded=()):
    """capped_walk; the mutant lets an excluded news of the order use up its group's cap."""
    if group is None:
        return [v for v in order if v not in excluded], []
    taken, skipped, cnt = [], [], {}
    for v in order:
        g = int(group[v])
        if g >= 0 and cnt.get(g, 0) >= cap:
            skipped.append(v)
            continue
        cnt[g] = cnt.get(g, 0) + 1
        if v not in excluded:
            taken.append(v)
    return taken, skipped


def _user_orders(P, s, mutant):
    """Per user (order of the eligible ids, excluded set for the cap mutant)."""
    c, S = P.c, P.S
    prior, inwin = _pool(P, S, mutant)
    lists = _lists(P, S, mutant)
    out = []
    for u in range(c.U):
        ok = inwin[u].copy()
        ok[0] = False
        ex = set()
        if mutant == "excluded_uses_cap":
            ex = set(lists[u].tolist())
        else:
            ok[lists[u]] = False
        out.append((_order(s[u], ok, mutant).tolist(), ex))
    return out


def _noise_g(seed, draw, keys, ids):
    return H.gumbel64(H.philox_bits(seed, draw, keys, ids)).astype(f32)


def _back(s, mutant):
    """key_score(score_key(s)): -0 comes back as +0."""
    return s if mutant == "neg_zero_below" else s + f32(0)


def standin(mutant=None, acc64=False):
    """call(P) for every entry point, on the CPU buffers of P."""
    def topk(P):
        c, I, S = P.c, P.I, P.S
        s = _dots(P, mutant, acc64)
        prior = P.inb["prior"].v[0].numpy() if "prior" in P.inb else None
        dead = np.zeros(c.U, bool)
        with np.errstate(all="ignore"):
            if P.entry == "sample":
                tau = P.inb["tau_u"].v[0].numpy() if "tau_u" in P.inb else np.full(c.U, I.tau, f32)
                dead = ~((tau >= 0) & (tau < INF))
                tau = np.where(dead, f32(0), tau).astype(f32)
                keys = P.inb["keys"].v[0].numpy() if "keys" in P.inb else np.arange(c.U, dtype=i32)
                if mutant == "noise_tile_local_key":
                    keys = (np.arange(c.U) % 16).astype(i32)
                g = _noise_g(I.seed, I.draw, np.repeat(keys, c.V), np.tile(np.arange(c.V, dtype=i32), c.U)).reshape(c.U, c.V)
                noise = (tau[:, None] * g).astype(f32)
                s = s + ((prior if prior is not None else f32(0)) + noise).astype(f32)
            elif prior is not None:
                s = s + prior[None, :]
        group = P.inb["group"].v[0].numpy() if "group" in P.inb else None
        ids, sc = P.outb["ids"].v, P.outb["scores"].v
        fill = -1 if mutant == "fill_id_minus1" else 0
        for u, (order, ex) in enumerate(_user_orders(P, s, mutant)):
            row = [] if dead[u] else _walk(order, group, c.cap, mutant, ex)[0][:c.k]
            if mutant == "slot64_dropped":
                row = row[:64]
            ids[u], sc[u] = fill, -INF
            if row:
                ids[u, :len(row)] = torch.tensor(row, dtype=torch.int32)
                sc[u, :len(row)] = torch.from_numpy(_back(s[u, row], mutant))
        if "model" in P.outb:
            idn = ids.numpy().astype(np.int64)
            with np.errstate(all="ignore"):
                m = np.where(idn > 0, sc.numpy() - np.take_along_axis(noise, np.clip(idn, 0, c.V - 1), axis=1), f32(-INF)).astype(f32)
            P.outb["model"].v[:] = torch.from_numpy(m)
        if mutant == "ws_overrun":
            P.ws.flat[P.ws.start + P.ws.cols] = 1

    def rank(P):
        c, I, S = P.c, P.I, P.S
        s = _dots(P, mutant, acc64)
        with np.errstate(all="ignore"):
            if "prior" in P.inb:
                s = s + P.inb["prior"].v[0].numpy()[None, :]
        group = P.inb["group"].v[0].numpy() if "group" in P.inb else None
        tg = rd(P.inb["targets"], c.U, c.T, S.tgt)
        ranks, sc = np.zeros((c.U, c.T), i32), np.full((c.U, c.T), -INF, f32)
        for u, (order, ex) in enumerate(_user_orders(P, s, mutant)):
            taken, skipped = _walk(order, group, c.cap, mutant, ex)
            place = {v: p + 1 for p, v in enumerate(taken)}
            place.update({v: -1 for v in skipped})
            seen = set()
            for j, t in enumerate(tg[u].tolist()):
                if t in place and (t not in seen or mutant == "repeated_target_twice"):
                    ranks[u, j], sc[u, j] = place[t], _back(s[u, t:t + 1], mutant)[0]
                    if mutant == "rank_ties_as_wins" and group is None:
                        ranks[u, j] = 1 + sum(1 for v in taken if v != t and s[u, v] >= s[u, t])
                seen.add(t)
        P.outb["ranks"].v[:], P.outb["scores"].v[:] = torch.from_numpy(ranks), torch.from_numpy(sc)
        if "sums" in P.outb:
            shown = np.where(ranks < 0, 0, ranks) if mutant == "idcg_shrunk" else ranks
            P.outb["sums"].v[0] = torch.tensor(H.sums_ref(shown, I.ks)[0], dtype=torch.float64)
            if mutant == "idcg_shrunk":
                P.outb["sums"].v[0, 0] = float((ranks != 0).any(axis=1).sum())

    def mmr(P):
        c, I, S = P.c, P.I, P.S
        pid, r = rd(P.inb["pool_ids"], c.U, c.M, S.pid).astype(np.int64), rd(P.inb["pool_scores"], c.U, c.M, S.psc)
        news = rd(P.inb["news"], c.V, c.N, S.news)
        group = P.inb["group"].v[0].numpy() if "group" in P.inb else None
        pen = P.inb["penalty_u"].v[0].numpy() if "penalty_u" in P.inb else np.full(c.U, I.penalty, f32)
        ids, sc, pl = np.zeros((c.U, c.k), i32), np.full((c.U, c.k), -INF, f32), np.full((c.U, c.k), -1, i32)
        for u in range(c.U):
            live = (pid[u] >= 1) & (pid[u] < c.V) & ~np.isnan(r[u])
            x = news[np.where(live, pid[u], 0)] * live[:, None].astype(f32)
            g = chain(x, x, c.N, mmr_order(c.N), acc64)
            if mutant == "gram_asymmetric":                                 # the lower triangle contracts four columns fewer
                g = np.where(np.tri(c.M, k=-1, dtype=bool), chain(x, x, c.N, mmr_order(c.N), acc64, c.N - 4), g)
            with np.errstate(all="ignore"):
                d = np.diag(g)
                rn = np.where(d > 0, f32(1) / np.sqrt(d), f32(0)).astype(f32)
            grp = np.where(live, group[np.where(live, pid[u], 0)], -1) if group is not None else np.full(c.M, -1)
            taken, cnt, maxsim = np.zeros(c.M, bool), {}, np.full(c.M, -INF, f32)
            for t in range(c.k):
                cand = live & ~taken & np.array([gg < 0 or cnt.get(int(gg), 0) < c.cap for gg in grp])
                if not cand.any():
                    break
                with np.errstate(all="ignore"):
                    val = (r[u] if t == 0 else fma32(np.full(c.M, -pen[u], f32), maxsim, r[u])) + f32(0)
                best = np.where(cand, val, -INF).max()
                hits = np.flatnonzero(cand & (val == best))
                j = int(hits[-1] if mutant == "mmr_ties_highest" else hits[0])
                ids[u, t], sc[u, t], pl[u, t], taken[j] = pid[u, j], r[u, j], j, True
                if grp[j] >= 0:
                    cnt[int(grp[j])] = cnt.get(int(grp[j]), 0) + 1
                with np.errstate(all="ignore"):
                    maxsim = np.maximum(maxsim, ((g[:, j] * rn).astype(f32) * rn[j]).astype(f32))
        for k, a in (("ids", ids), ("scores", sc), ("place", pl)):
            P.outb[k].v[:] = torch.from_numpy(a)

    def noise(P):
        keys, ids = P.inb["keys"].v[0].numpy(), P.inb["ids"].v[0].numpy()
        P.outb["bits"].v[0] = torch.from_numpy(H.philox_bits(P.seed, P.draw, keys, ids).view(i32))
        P.outb["g"].v[0] = torch.from_numpy(_noise_g(P.seed, P.draw, keys, ids))

    table = dict(topk=topk, sample=topk, rank=rank, mmr=mmr, noise=noise)
    return lambda P: table[P.entry](P)


# ------------------------------------------------------------------------------------------ (a)
# (a sampled lattice case is stated through the probe's fp32 g, which metrics.sample_reference does not take: the stand-in tests hold it)
@pytest.mark.parametrize("c", [c for c in H.topk_cases() if c.kind != "special" and not (c.sample == 2 and c.kind != "gauss")], ids=lambda c: c.name)
def test_topk_reference_is_metrics_topk_and_sample_reference(c):
    I = H.corpus_inputs(c)
    lists = I.exclude if I.exclude is not None else I.segs
    caps = dict(group=I.group, group_cap=c.cap) if c.cap else {}
    dot = I.user.astype(f64) @ I.news.astype(f64).T
    if c.sample == 2:
        keys = I.keys if I.keys is not None else np.arange(c.U, dtype=i32)
        g = H.gumbel64(H.philox_bits(I.seed, I.draw, np.repeat(keys, c.V), np.tile(np.arange(c.V, dtype=i32), c.U))).reshape(c.U, c.V)
        r, _ = H.corpus_scores(c, I, g)
        ids, sc = H.topk_ref(c, I, r, H.eligible(c, I))
        tau = I.tau_u if I.tau_u is not None else I.tau
        want = metrics.sample_reference(dot, k=c.k, temperature=tau, seed=I.seed, draw=I.draw, user_keys=None if I.keys is None else I.keys.astype(np.int64) & 0xFFFFFFFF,
                                        exclude=lists, prior=I.prior, stamp=I.stamp, window=I.window, **caps)
        assert np.array_equal(ids, want[0]) and np.allclose(sc, want[1], rtol=1e-12, atol=0)
        return
    r, _ = H.corpus_scores(c, I)
    ids, sc = H.topk_ref(c, I, r, H.eligible(c, I))
    want = metrics.topk_reference(dot, k=c.k, exclude=lists, prior=I.prior, stamp=I.stamp, window=I.window, **caps)
    assert np.array_equal(ids, want[0]) and np.array_equal(sc, want[1])


@pytest.mark.parametrize("c", [c for c in H.rank_cases() if c.kind != "special"], ids=lambda c: c.name)
def test_rank_reference_is_metrics_rank_reference(c):
    I = H.corpus_inputs(c)
    r, _ = H.corpus_scores(c, I)
    ranks, sc = H.rank_ref(c, I, r, H.eligible(c, I))
    caps = dict(group=I.group, group_cap=c.cap) if c.cap else {}
    want = metrics.rank_reference(I.user.astype(f64) @ I.news.astype(f64).T, targets=I.targets, exclude=I.exclude if I.exclude is not None else I.segs, prior=I.prior,
                                  stamp=I.stamp, window=I.window, **caps)
    assert np.array_equal(ranks, want[0]) and np.array_equal(sc, want[1])
    if c.sums:
        got, want_s = H.sums_ref(ranks, I.ks), metrics.retrieval_metrics_reference(ranks, I.ks)[1]
        assert np.allclose(got[0], want_s, rtol=1e-13, atol=0)


@pytest.mark.parametrize("c", H.mmr_cases(), ids=lambda c: c.name)
def test_mmr_reference_is_metrics_mmr_reference(c):
    I = H.mmr_inputs(c)
    caps = dict(group=I.group, group_cap=c.cap) if c.cap else {}
    with np.errstate(all="ignore"):
        want = metrics.mmr_reference(I.news, I.pool_ids, I.pool_scores, k=c.k, penalty=I.penalty_u if I.penalty_u is not None else float(f32(I.penalty)), **caps)
    got = H.mmr_ref(c, I)
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(a, b)
    if c.kind != "special":
        assert np.allclose(got[3], want[3], rtol=1e-9, atol=1e-300)


def test_philox_and_gumbel_are_the_ones_of_metrics():
    rng = np.random.default_rng(3)
    keys, ids = rng.integers(-2 ** 31, 2 ** 31, 4000), rng.integers(0, 2 ** 31, 4000)
    for seed, draw, _ in H.NOISE_CASES:
        g, bits = metrics.sample_noise_reference(seed, draw, keys & 0xFFFFFFFF, ids)
        mine = H.philox_bits(seed, draw, keys.astype(i32), ids.astype(i32))
        assert np.array_equal(mine, bits) and np.allclose(H.gumbel64(mine), g, rtol=1e-12, atol=1e-15)
    edge = np.array([0, 255, 256, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], np.uint32)      # the two ends and the middle of u
    g = H.gumbel64(edge)
    assert np.isfinite(g).all() and -2.853 < g.min() and g.max() < 17.329


# ------------------------------------------------------------------------------------------ (b)
def test_every_route_has_two_cases():
    H._count_routes([H.topk_route(c) for c in H.topk_cases()], H.TK_ROUTES, "top-k and sample")
    H._count_routes([H.rank_route(c) for c in H.rank_cases()], H.RK_ROUTES, "rank")
    H._count_routes([H.mmr_route(c) for c in H.mmr_cases()], H.MM_ROUTES, "mmr")


def test_the_tables_hold_what_the_issue_lists():
    tk, rk, mm = H.topk_cases(), H.rank_cases(), H.mmr_cases()
    swept = [c for c in tk + rk if c.kind != "special"]
    assert {c.N for c in swept} == set(H.TK_NS) | {512} and {c.N for c in tk if c.kind != "special"} == set(H.TK_NS)
    assert {c.V for c in swept} == set(H.TK_VS) and {c.splits for c in swept} == set(H.TK_SPLITS)
    assert {c.k for c in tk} >= set(H.TK_KS) and {c.T for c in rk} >= set(H.RK_TS) and {c.n_ks for c in rk} == set(H.RK_NKS)
    assert {c.E for c in tk} == {c.E for c in rk} == set(H.TK_ES)
    for cases, plan in ((tk, H.tk_plan), (rk, H.rk_plan)):                  # U = 1, TU - 1, TU, TU + 1 of every tile
        for tile in (64, 32, 16):
            assert {c.U for c in cases if plan(c)[0] == tile} >= {1, tile - 1, tile, tile + 1}, tile
    assert any("empty_slices" in H.topk_route(c) for c in tk)
    assert any(c.k == 1 and c.splits == 1 for c in tk)
    assert any(c.cap and not c.ung and c.G * c.cap < c.k for c in tk)
    for c in (TK["lattice-cap-midblock"], TK["gauss-cap-midblock"]):        # the capped merge walk takes its 128th key inside a block of 64, after skips
        I = H.corpus_inputs(c)
        at = H.midblock_positions(c, I, H.corpus_scores(c, I)[0], H.eligible(c, I))
        assert c.k == 128 and sum(1 for p in at if p > 128 and p % 64 != 0) >= 3, (c.name, at)
    assert all(c.T <= 4 for c in rk if c.cap)
    for c in tk + rk:                                                       # the CSR lists: every length in one call where the users allow
        if c.csr and c.U >= 6:
            I = H.corpus_inputs(c)
            assert {len(s) for s in I.segs} == set(H.CSR_LENGTHS) and I.offsets[-1] > len(I.xids)
            assert any((s <= 0).any() and (s >= c.V).any() for s in I.segs) and all((np.diff(s) > 0).all() for s in I.segs)
    assert any(c.csr and c.U >= 6 for c in tk) and any(c.csr and c.U >= 6 for c in rk)
    assert {(c.M, c.k == 1) for c in mm if c.kind != "special"} >= {(M, one) for M in H.MM_MS for one in ((True,) if M == 1 else (True, False))}
    for c in tk + rk + mm:                                                  # padded strides: two different vector strides, the pool strides differ
        S = H.strides(c, "pad")
        assert S.news != S.user and S.news % 4 == 0 and S.user % 4 == 0 and min(S.news, S.user) >= c.N and S.pid != S.psc
    assert {H.strides(c, "pad").excl - c.E for c in tk} == {0, 3} and {H.strides(c, "pad").tgt - c.T for c in rk} == {0, 1}
    assert {H.strides(c, "pad").win for c in tk if c.pool in (1, 3)} == {2, 5}


def test_the_workspace_carve_is_the_size_query():
    """The restated carve against nr_score_*_workspace_bytes (host arithmetic: no device is touched)."""
    d = 1 << 20
    for c in H.topk_cases():
        desc = _lib.TopkDesc(news_vecs=d, ld_news=c.N, V=c.V, user=d, ld_user=c.N, U=c.U, N=c.N, k=c.k, splits=c.splits)
        assert _lib.lib().nr_score_topk_workspace_bytes(C.byref(desc)) == H.tk_ws_bytes(c), c
    for c in H.rank_cases():
        ks = (C.c_int * 8)(*([3] * 8))
        desc = _lib.RankDesc(news_vecs=d, ld_news=c.N, V=c.V, user=d, ld_user=c.N, U=c.U, N=c.N, T=c.T, targets=d, ld_targets=c.T, splits=c.splits, ks=ks, n_ks=c.n_ks,
                             group=d if c.cap else None, group_cap=c.cap, n_groups=c.G if c.cap else 0)
        assert _lib.lib().nr_score_rank_workspace_bytes(C.byref(desc)) == H.rk_ws_bytes(c), c


# ------------------------------------------------------------------------------------------ (c) and (d)
def _decided(c, w, tile):
    if c.kind != "gauss":
        return
    rows = w["decided_rows"]
    assert rows.mean() >= 0.9, (c.name, rows.mean())
    for u0 in range(0, c.U, tile):
        assert rows[u0:u0 + tile].any(), (c.name, u0)


@pytest.mark.parametrize("acc64", (False, True))
@pytest.mark.parametrize("c", H.topk_cases(), ids=lambda c: c.name)
def test_topk_and_sample_standin_passes(c, acc64):
    _decided(c, H.tk_sweep(c, DEV, standin(None, acc64), layout=not acc64), H.tk_plan(c)[0])


@pytest.mark.parametrize("acc64", (False, True))
@pytest.mark.parametrize("c", H.rank_cases(), ids=lambda c: c.name)
def test_rank_standin_passes(c, acc64):
    _decided(c, H.rk_sweep(c, DEV, standin(None, acc64), layout=not acc64), H.rk_plan(c)[0])


@pytest.mark.parametrize("acc64", (False, True))
@pytest.mark.parametrize("c", H.mmr_cases(), ids=lambda c: c.name)
def test_mmr_standin_passes(c, acc64):
    _decided(c, H.mm_sweep(c, DEV, standin(None, acc64), layout=not acc64), 1)


def test_noise_standin_passes():
    for seed, draw, n in H.NOISE_CASES:
        assert H.noise_sweep(seed, draw, n, DEV, standin()) < 1.0


# ------------------------------------------------------------------------------------------ (e)
def _first(cases, pred):
    return next(c for c in cases if pred(c))


MUTANTS = [
    ("ties_desc_id", "topk", lambda c: c.kind == "lattice" and c.V >= 128 and c.k > 1 and not c.sample, "exact"),
    ("float4_past_N", "topk", lambda c: c.kind == "lattice" and c.V >= 128 and c.N % 32 != 0, "exact"),
    ("E_for_ld_exclude", "topk", lambda c: c.kind == "lattice" and c.E >= 1 and c.U > 2 and c.V >= 128 and H.strides(c, "pad").excl > c.E, "exact"),
    ("two_for_ld_window", "topk", lambda c: c.kind == "lattice" and c.pool in (1, 3) and c.U > 2 and c.V >= 128 and H.strides(c, "pad").win == 5, "exact"),
    ("slot64_dropped", "topk", lambda c: c.kind == "lattice" and c.k > 64 and c.V >= 128 and not c.cap and not c.csr, "exact"),
    ("neg_zero_below", "topk", lambda c: c.name == "special-zeros", "special"),
    ("nan_news_returned", "topk", lambda c: c.name == "special-inf", "special"),
    ("fill_id_minus1", "topk", lambda c: c.kind == "lattice" and c.V <= 3 and c.k > 2, "exact"),
    ("neg_inf_as_fill", "topk", lambda c: c.name == "special-inf", "special"),
    ("window_hi_exclusive", "topk", lambda c: c.kind == "lattice" and c.pool in (1, 3) and c.V >= 128, "exact"),
    ("excluded_uses_cap", "topk", lambda c: c.kind == "lattice" and c.cap and (c.E >= 63 or c.csr) and c.V >= 128 and c.U > 2, "exact"),
    ("repeated_target_twice", "rank", lambda c: c.kind == "lattice" and c.T >= 2 and c.V >= 128 and c.U > 2, "exact"),
    ("rank_ties_as_wins", "rank", lambda c: c.kind == "lattice" and not c.cap and c.V >= 128 and c.U > 2, "exact"),
    ("idcg_shrunk", "rank", lambda c: c.name == "lattice-capped-out-sums", "sums"),
    ("mmr_ties_highest", "mmr", lambda c: c.kind == "lattice" and c.M >= 31 and c.k == c.M, "exact"),
    ("gram_asymmetric", "mmr", lambda c: c.kind == "lattice" and c.M >= 31 and c.k == c.M and c.N >= 28, "exact"),
    ("ws_overrun", "topk", lambda c: c.kind == "lattice", "sentinel"),
    ("noise_tile_local_key", "topk", lambda c: c.kind == "lattice" and c.sample == 2 and c.V >= 128 and ("k" in c.opt or c.U > 16), "exact"),
    ("neg_zero_below", "rank", lambda c: c.name == "special-zeros", "special"),
    ("neg_inf_as_fill", "rank", lambda c: c.name == "special-inf", "special"),
    ("nan_news_returned", "rank", lambda c: c.name == "special-inf", "special"),
]
SWEEPS = dict(topk=(H.topk_cases, lambda *a: H.tk_sweep(*a)), rank=(H.rank_cases, lambda *a: H.rk_sweep(*a)), mmr=(H.mmr_cases, lambda *a: H.mm_sweep(*a)))


@pytest.mark.parametrize("mutant,entry,pred,want", MUTANTS, ids=[f"{m[0]}-{m[1]}" for m in MUTANTS])
def test_mutant_fails_its_layer(mutant, entry, pred, want):
    cases, sweep = SWEEPS[entry]
    c = _first(cases(), pred)
    with pytest.raises(H.CorpusCheckError) as e:
        sweep(c, DEV, standin(mutant))
    assert e.value.layer == want, (c.name, str(e.value))


def test_subnormal_products_flushed_fail_special():
    """A device that flushed subnormal products would return zeros for the subnormal case."""
    base = standin()

    def flushed(P):
        base(P)
        sc = P.outb["scores"].v
        sc[sc.abs() < 2.0 ** -126] = 0.0
    for entry, c in (("topk", TK["special-subnormal"]), ("rank", RK["special-subnormal"])):
        with pytest.raises(H.CorpusCheckError) as e:
            SWEEPS[entry][1](c, DEV, flushed)
        assert e.value.layer == "special"


def test_a_second_run_that_differs_in_one_bit_fails_repeat():
    base, n = standin(), [0]

    def flaky(P):
        base(P)
        n[0] += 1
        if n[0] == 2:
            s = P.outb["scores"].v
            s[0, 0] = float(np.nextafter(f32(s[0, 0]), f32(INF)))
    with pytest.raises(H.CorpusCheckError) as e:
        H.tk_sweep(TK["gauss-24"], DEV, flaky)
    assert e.value.layer == "repeat"


def test_a_rank_pass_that_sums_in_another_order_fails_agree():
    """Both orders are inside the bound; "rank <= k exactly when the target is in the row, with identical score bits" needs ONE."""
    slab, once = standin(None, False), standin(None, True)
    c = _first(H.topk_cases(), lambda c: c.kind == "gauss" and not c.sample and not c.cap and c.N >= 28 and c.V >= 128 and c.k >= 63)
    with pytest.raises(H.CorpusCheckError) as e:
        H.tk_sweep(c, DEV, lambda P: (once if P.entry == "rank" else slab)(P), layout=False)
    assert e.value.layer == "agree", str(e.value)


@pytest.mark.parametrize("kind,want", (("gauss", "agree"), ("lattice", "exact")))
def test_a_sampled_call_that_fuses_the_noise_into_one_fma_fails(kind, want):
    """fl32(prior + tau g) with one rounding instead of two: inside the bound, and not the plain call with the perturbed prior
    (Gaussian data), nor the three fp32 roundings of the header (lattice data)."""
    base = standin()
    c = TK["gauss-sample-prior"] if kind == "gauss" else TK["tile64-u2"]
    I = H.corpus_inputs(c)

    def fused(P):
        base(P)
        if P.entry == "sample":                                             # redo the rows with the fused prior through the plain path
            tau, bad = H.taus(c, I)
            keys = I.keys if I.keys is not None else np.arange(c.U, dtype=i32)
            g = _noise_g(I.seed, I.draw, np.repeat(keys, c.V), np.tile(np.arange(c.V, dtype=i32), c.U)).reshape(c.U, c.V)
            for u in np.flatnonzero(~bad):
                c1, I1 = H._one_user(c, I, u, (I.prior.astype(f64) + tau[u].astype(f64) * g[u].astype(f64)).astype(f32))
                P1 = H.problem("topk", c1, I1, DEV)
                base(P1)
                P.outb["ids"].v[u], P.outb["scores"].v[u] = P1.outb["ids"].v[0], P1.outb["scores"].v[0]
    with pytest.raises(H.CorpusCheckError) as e:
        H.tk_sweep(c._replace(opt=c.opt.replace("m", "")), DEV, fused, layout=False)
    assert e.value.layer == want, str(e.value)


def test_a_layout_that_changes_the_bits_fails_layout():
    base = standin()

    def by_stride(P):
        base(P)
        if P.entry == "topk" and P.S.news == P.c.N and P.S.user == P.c.N:
            s = P.outb["scores"].v
            s[0, 0] = float(np.nextafter(f32(s[0, 0]), f32(INF)))
    with pytest.raises(H.CorpusCheckError) as e:
        H.tk_sweep(_first(H.topk_cases(), lambda c: c.kind == "gauss" and not c.sample and c.V >= 128), DEV, by_stride)
    assert e.value.layer == "layout"


@pytest.mark.parametrize("entry", ("topk", "rank"))
def test_one_and_a_half_times_the_bound_fails_bound(entry):
    cases, sweep = SWEEPS[entry]
    c = _first(cases(), lambda c: c.kind == "gauss" and c.V >= 128 and not c.cap and not getattr(c, "sample", 0) and c.pool in (0, 3))
    I = H.corpus_inputs(c)
    r, b = H.corpus_scores(c, I)
    base = standin(None, True)

    def off(P):
        base(P)
        if entry == "topk":
            ids = P.outb["ids"].v.numpy().astype(np.int64)
            u = 0
            P.outb["scores"].v[u, 0] = float(f32(r[u, ids[u, 0]] + 1.5 * b[u, ids[u, 0]]))
        else:
            u, j = np.argwhere(P.outb["ranks"].v.numpy() > 0)[0]
            t = int(I.targets[u, j])
            P.outb["scores"].v[u, j] = float(f32(r[u, t] - 1.5 * b[u, t]))
    with pytest.raises(H.CorpusCheckError) as e:
        sweep(c, DEV, off, False)
    assert e.value.layer == "bound"


def test_sums_off_by_more_than_their_bound_fail_sums():
    c = _first(H.rank_cases(), lambda c: c.kind == "lattice" and c.sums and c.n_ks == 8 and c.U > 2 and c.V >= 128)
    base = standin()

    def off(P):
        base(P)
        s = P.outb["sums"].v
        s[0, 1] = s[0, 1] * (1 + (c.U + 4) * 2.0 ** -52)
    with pytest.raises(H.CorpusCheckError) as e:
        H.rk_sweep(c, DEV, off, False)
    assert e.value.layer == "sums"


def test_noise_off_by_one_bit_or_beyond_the_bound_fails_noise():
    base = standin()

    def bit(P):
        base(P)
        P.outb["bits"].v[0, 0] ^= 1

    def far(P):
        base(P)
        g = P.outb["g"].v
        g[0, 0] = g[0, 0] + 8 * 2.0 ** -23 * max(1.0, abs(float(g[0, 0])))
    for call in (bit, far):
        with pytest.raises(H.CorpusCheckError) as e:
            H.noise_sweep(*H.NOISE_CASES[1], DEV, call)
        assert e.value.layer == "noise"


# ------------------------------------------------------------------------------------------ (f)
def test_refusals_before_the_device_guard():
    lib, d = _lib.lib(), 1 << 20
    ks = (C.c_int * 1)(10)

    def rank(**kw):
        a = dict(news_vecs=d, ld_news=8, V=40, user=d, ld_user=8, U=3, N=8, T=4, targets=d, ld_targets=4, splits=1, ks=ks, n_ks=1, out_ranks=d, out_scores=d, ws=d,
                 ws_bytes=1 << 30)
        a.update(kw)
        return lib.nr_score_rank(C.byref(_lib.RankDesc(**a)), None), _lib.last_error()

    def topk(**kw):
        a = dict(news_vecs=d, ld_news=8, V=40, user=d, ld_user=8, U=3, N=8, k=8, splits=1, out_ids=d, out_scores=d, ws=d, ws_bytes=1 << 30)
        a.update(kw)
        return lib.nr_score_topk(C.byref(_lib.TopkDesc(**a)), None), _lib.last_error()

    def mmr(**kw):
        a = dict(news_vecs=d, ld_news=8, V=40, pool_ids=d, pool_scores=d, ld_pool_ids=8, ld_pool_scores=8, U=3, N=8, M=8, k=8, penalty=1.0, out_ids=d, out_scores=d, out_place=d)
        a.update(kw)
        return lib.nr_mmr_select(C.byref(_lib.MmrDesc(**a)), None), _lib.last_error()

    for call, kw, text in ((rank, dict(T=5, ld_targets=5, group=d, group_cap=2, n_groups=4), "T = 5 targets per row with group caps"), (rank, dict(T=65), "T = 65"),
                           (rank, dict(ld_targets=3), "target row stride"), (rank, dict(group=d, group_cap=2, n_groups=513), "n_groups = 513"),
                           (rank, dict(n_ks=9), "n_ks = 9"), (rank, dict(ws_bytes=8), "workspace"), (rank, dict(ws=d + 4), "workspace"),
                           (topk, dict(k=129), "k = 129"), (topk, dict(N=6), "multiple of 4"), (topk, dict(ld_news=12, ld_user=10), "16-byte aligned"),
                           (topk, dict(news_vecs=d + 8), "16-byte aligned"), (topk, dict(E=65, exclude=d, ld_exclude=65), "E = 65"),
                           (topk, dict(E=4, exclude=d, ld_exclude=3), "exclusion row stride"), (topk, dict(E=2, exclude=d, ld_exclude=2, excl_offsets=d, excl_ids=d, n_excl=3), "one list form"),
                           (topk, dict(stamp=d), "stamp given without window"), (topk, dict(stamp=d, window=d, ld_window=1), "ld_window = 1"),
                           (topk, dict(group=d), "group_cap = 0"), (topk, dict(group_cap=3), "without group"), (topk, dict(splits=1025), "splits = 1025"),
                           (topk, dict(ws_bytes=3 * 8 * 8 - 1), "workspace"), (mmr, dict(k=9), "k = 9"), (mmr, dict(M=129, k=1), "M = 129"),
                           (mmr, dict(ld_pool_scores=7), "pool row strides"), (mmr, dict(penalty=-1.0), "penalty"), (mmr, dict(penalty=INF), "penalty"),
                           (mmr, dict(ld_news=6), "16-byte aligned")):
        rc, err = call(**kw)
        assert rc != 0 and text in err, (kw, rc, err)
    sd = _lib.SampleDesc(topk=_lib.TopkDesc(news_vecs=d, ld_news=8, V=40, user=d, ld_user=8, U=3, N=8, k=8, splits=1, out_ids=d, out_scores=d, ws=d, ws_bytes=1 << 30), tau=-1.0)
    assert lib.nr_score_sample(C.byref(sd), None) != 0 and "tau" in _lib.last_error()
    assert lib.nr_sample_noise(1, 1, d, d, -1, d, d, None) != 0 and "n = -1" in _lib.last_error()
    assert lib.nr_sample_noise(1, 1, None, d, 4, d, d, None) != 0 and "null pointer" in _lib.last_error()
