"""What tests/test_capgrad_news_host.py and tests/test_gpu_capgrad_news.py share: the DENSE statement of the capped row's loss in
float64 torch, whose autograd with respect to the news table is the yardstick of the news-side gradient (include/nrhip.h, K22),
and the composition of the float64 references that is held against it."""
import numpy as np
import torch

from newsrecommendation_amd import metrics


def bins_of(group, G):
    group = np.asarray(group, dtype=np.int64)
    return np.where(group < 0, G, group)


def dense_capped_loss(news, user, rows, g, tau, group, G, cap, exclude=None, prior=None, stamp=None, window=None, steps=None):
    """L = sum_u sum_j g_uj nll_uj of rows under the capped law (metrics.capped_row_logprob_reference), written on the whole score
    row of every user: at a live step j the candidates are the eligible news that the row does not name, plus the row's own live
    entries from place j on, both restricted to the bins that are open at step j.  news: float64 torch [V, N] (may require grad);
    user float64 torch [U, N] (may carry a graph); the rest numpy.  A user whose temperature is not finite and > 0 has no term.
    steps: a list that receives, per user, the bool [k] array of the entries that are steps."""
    V, U = news.shape[0], user.shape[0]
    rows = np.asarray(rows, dtype=np.int64).reshape(U, -1)
    k = rows.shape[1]
    bins = bins_of(group, G)
    taus = np.broadcast_to(np.asarray(tau, dtype=np.float64), (U,))
    total = torch.zeros((), dtype=torch.float64)
    for u in range(U):
        if not (np.isfinite(taus[u]) and taus[u] > 0):
            if steps is not None:
                steps.append(np.zeros(k, dtype=bool))
            continue
        s = news @ user[u]
        if prior is not None:
            s = s + torch.as_tensor(np.asarray(prior, dtype=np.float64))
        ok = ~torch.isnan(s.detach()).numpy()
        if prior is not None:
            ok &= ~np.isneginf(np.asarray(prior, dtype=np.float64))
        if stamp is not None:
            st, win = np.asarray(stamp, dtype=np.int64), np.asarray(window, dtype=np.int64)
            ok &= (win[u, 0] <= st) & (st <= win[u, 1])
        ok[0] = False
        inpool = ok.copy()
        if exclude is not None:
            ex = np.asarray(exclude[u], dtype=np.int64).reshape(-1)
            ok[ex[(ex >= 1) & (ex < V)]] = False
        ids = rows[u]
        real = (ids >= 1) & (ids < V)
        at = np.where(real, ids, 0)
        live = real & inpool[at]
        ok[at[real]] = False                                           # what the row names is no term of a base
        bn = bins[at]
        t_close = np.full(G + 1, k, dtype=np.int64)
        seen, capped = np.zeros(G + 1, dtype=np.int64), np.zeros(k, dtype=bool)
        for j in np.flatnonzero(live):
            if bn[j] < G:
                capped[j] = seen[bn[j]] >= cap
                seen[bn[j]] += 1
                if seen[bn[j]] == cap:
                    t_close[bn[j]] = j
        if steps is not None:
            steps.append(live & ~capped)
        for j in np.flatnonzero(live & ~capped):
            open_bins = t_close >= j
            cand = torch.as_tensor(ok & open_bins[bins])
            later = [int(at[i]) for i in range(j, k) if live[i] and open_bins[bn[i]]]
            terms = torch.cat([s[cand], s[torch.as_tensor(later, dtype=torch.int64)]]) / taus[u]
            total = total + float(g[u, j]) * (torch.logsumexp(terms, 0) - s[int(at[j])] / taus[u])
    return total


def autograd_news_gradient(news, user, rows, g, tau, group, G, cap, **kw):
    """d dense_capped_loss / d news, float64 numpy [V, N]; components of `news` that are not finite get 0."""
    t = torch.as_tensor(np.asarray(news, dtype=np.float64)).clone().requires_grad_()
    loss = dense_capped_loss(t, torch.as_tensor(np.asarray(user, dtype=np.float64)), rows, g, tau, group, G, cap, **kw)
    if not loss.requires_grad:
        return np.zeros(t.shape), float(loss.detach())
    (grad,) = torch.autograd.grad(loss, t)
    return np.nan_to_num(grad.numpy(), nan=0.0), float(loss.detach())


def merged_lists(exclude, rows, U):
    """Per user: the exclusion list with the row's ids merged in (numpy arrays)."""
    rows = np.asarray(rows, dtype=np.int64).reshape(U, -1)
    return [np.concatenate([np.asarray(exclude[u], dtype=np.int64).reshape(-1) if exclude is not None else np.zeros(0, dtype=np.int64),
                            rows[u][rows[u] >= 1]]) for u in range(U)]


def named_by_news(rows, c, V):
    """ops._named_by_news on the host, the weights kept in float64: (offsets [V + 1], users [n], w [n]), within a news (user, place)
    ascending; entries with c == 0 and ids outside [1, V) dropped."""
    c = np.asarray(c, dtype=np.float64)
    flat, w, T = np.asarray(rows, dtype=np.int64).reshape(-1), c.reshape(-1), c.shape[1]
    at = np.flatnonzero((w != 0) & (flat >= 1) & (flat < V))
    at = at[np.argsort(flat[at], kind="stable")]
    off = np.zeros(V + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(flat[at], minlength=V))
    return off, at // T, w[at]


MUTANTS = ("wrong_bin", "named_base_gate", "no_inv_tau")


def composed_reference(news, user, rows, g, tau, group, G, cap, exclude=None, prior=None, stamp=None, window=None, mutant=None):
    """The closed form in float64: K15's bases with the row merged into the lists, K21's (omega, c), and K22's reference with the
    row's entries as named terms.  Returns (grad_news [V, N], A [V, N], omega, c).  `mutant` names a deliberately wrong way of
    putting the pieces together, applied to the INPUTS of the public reference: "wrong_bin" (every bin is given the omega of the
    next one), "named_base_gate" (a named term is dropped where the user's bin of that news is empty in the bases: K18's gating),
    "no_inv_tau" (1 / tau dropped from both sums)."""
    assert mutant is None or mutant in MUTANTS
    news, user = np.asarray(news, dtype=np.float64), np.asarray(user, dtype=np.float64)
    U, V = user.shape[0], news.shape[0]
    merged = merged_lists(exclude, rows, U)
    pools = dict(prior=prior, stamp=stamp, window=window)
    bases = metrics.logz_groups_reference(news, user, temperature=tau, group=group, n_groups=G, exclude=merged, **pools)
    om, c = metrics.capped_row_logprob_grad_reference(news, user, row_ids=rows, temperature=tau, bases=bases[:2], group=group, group_cap=cap,
                                                      n_groups=G, g=g, **pools)
    off, nu, nw = named_by_news(rows, c, V)
    bin_w = om
    if mutant == "wrong_bin":
        bin_w = np.roll(om, -1, axis=1)
    if mutant == "named_base_gate":
        news_of = np.repeat(np.arange(V), np.diff(off))
        nw = np.where(bases[2][nu, bins_of(group, G)[news_of]] == 0, 0.0, nw)      # a weight of 0 is a skipped term
    out, _, A, _ = metrics.expect_news_groups_reference(news, user, temperature=tau, group=group, n_groups=G, bin_w=bin_w, exclude=merged,
                                                        named=(off, nu, nw), scale_inv_tau=mutant != "no_inv_tau", **pools)
    return out, A, om, c
