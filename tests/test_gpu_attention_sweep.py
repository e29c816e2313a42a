"""GPU: every kernel route of the training attention (`nr_sdpa_fwd` / `nr_sdpa_bwd`, and the same launchers inside
`nr_mhsa_fwd` / `nr_mhsa_bwd`) against the fp64 reference, forward and backward.

Part 1, the attention core.  The case list (helpers.attn_cases) walks the dispatch of nr_launch_attn / nr_launch_attn_mfma /
b16::launch -- dtype, L, d_head, heads % 4, L * d_head <= 768, pointer alignment -- so that every kernel family runs:
the bf16 panel kernels (title constants, FULL, predicated, PT = 4), the 64-row kernels (constants, generic), the generic
one-wave-per-head MFMA kernels in bf16 (d_head % 4 != 0, misaligned qkv) and fp32, the LDS/VALU kernels in both dtypes;
output dropout on one case per family; three score regimes and a masked key that carries the row maximum; sequence counts
above the block caps (grid-stride walks) and n = 1, 2, 3 (short software pipelines).  Each case names its route and the
profiler label must show that family ran.  The reference is oracle.nr_oracle.sdpa (+ apply_dropout with the kernels' own keep
mask, ops.dropout_mask) in fp64 with its autograd gradient, on the same bf16-representable inputs; the comparator
(helpers.slice_rel_err) and its tolerances (helpers.ATTN_TOL: from a CPU stand-in kernel and the project's bounds, never
from these kernels) are proven in tests/test_attention_sweep_host.py.  Per case also: every element of y and dqkv is
written (both start as NaN), sentinel zones around them stay untouched, an all-masked sequence gives exactly zero y, a
second run is bit-identical (none of these launches uses an atomic).

Part 2, ops.mhsa(ids=, table=) in bf16 training with padding substitution away from the title shape: per-row substitution
with and without compact row storage, per-sequence substitution (heads % 4 != 0; PT = 4), against fp64 O.mhsa.

Input domain (include/nrhip.h): |s| <= 60 and the maximum over all keys at most 45 above the maximum over the valid keys;
nothing here goes beyond it.
"""
import pytest
import torch

import helpers as H
from oracle import nr_oracle as O
from newsrecommendation_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, SENTINEL = 4096, 1536.0          # elements in front of and behind every output; a value both dtypes hold exactly
SEED = 20240607
CASES = H.attn_cases()
QUANT = ("y", "dq", "dk", "dv")


def _td(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def _code(c):
    return _lib.NR_BF16 if c.dtype == "bf16" else _lib.NR_F32


def _pack(q, k, v):
    """3 x [n, h, L, d] -> the kernels' token-major [n*L, 3*h*d]."""
    n, h, L, d = q.shape
    return torch.stack([t.permute(0, 2, 1, 3) for t in (q, k, v)], dim=2).reshape(n * L, 3 * h * d)


def _unpack(dqkv, n, h, L, d):
    t = dqkv.view(n, L, 3, h, d).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


class _Out:
    """An output buffer between two sentinel zones, NaN-filled."""

    def __init__(self, numel, dtype):
        self.buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
        self.body = self.buf[GUARD:GUARD + numel]
        self.body.fill_(float("nan"))
        assert self.body.data_ptr() % 16 == 0

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.body.numel():] == SENTINEL).all())


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _launch(c, qkv, mask, dy, n, seed):
    """nr_sdpa_fwd + nr_sdpa_bwd over the first n sequences into fresh guarded, NaN-filled buffers sized for c.n sequences."""
    N, stream = c.heads * c.d, torch.cuda.current_stream().cuda_stream
    y, dqkv = _Out(c.n * c.L * N, _td(c)), _Out(c.n * c.L * 3 * N, _td(c))
    mp = _lib.ptr(mask) if mask is not None else None
    args = (n, c.L, c.heads, c.d, _code(c), float(c.p_out), seed if c.p_out > 0 else 0, stream)
    _lib.check(_lib.lib().nr_sdpa_fwd(_lib.ptr(qkv), mp, _lib.ptr(y.body), *args), "nr_sdpa_fwd")
    _lib.check(_lib.lib().nr_sdpa_bwd(_lib.ptr(qkv), mp, _lib.ptr(dy), _lib.ptr(dqkv.body), *args), "nr_sdpa_bwd")
    return y, dqkv


def _profiled(fn):
    _lib.prof_enable(1)
    try:
        _lib.prof_collect()
        out = fn()
        torch.cuda.synchronize()
        labels = set(_lib.prof_collect().keys())
    finally:
        _lib.prof_enable(0)
    return out, labels


WORST = {}      # (route, dtype) -> {quantity: worst error}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_errors_per_route():
    """After the module: the worst slice-relative error per route and quantity over the cases that ran (DESIGN.md quotes it)."""
    yield
    for (route, dtype), w in sorted(WORST.items()):
        print(f"worst {route} {dtype}: " + " ".join(f"{k} {e:.2e}" for k, e in w.items()))


@pytest.mark.parametrize("c", CASES, ids=H.attn_case_id)
def test_attention_core_route_against_fp64(c):
    inp = H.attn_inputs(c)
    n, h, L, d, N = c.n, c.heads, c.L, c.d, c.heads * c.d
    td = _td(c)
    packed = _pack(inp["q"], inp["k"], inp["v"]).to(td)
    if c.align == "misaligned":             # a contiguous view one element into a larger buffer: 2-byte aligned only
        big = torch.zeros(packed.numel() + 16, dtype=td, device=DEV)
        qkv = big[1:1 + packed.numel()].view(packed.shape)
        qkv.copy_(packed)
        assert qkv.data_ptr() % 8 == 2
    else:
        qkv = packed.to(DEV).contiguous()
        assert qkv.data_ptr() % 16 == 0
    dy = inp["dy"].permute(0, 2, 1, 3).reshape(n * L, N).to(td).to(DEV).contiguous()
    keep = None
    if c.p_out > 0:                          # the kernels' own keep mask, indexed like y[n, L, N]
        keep = ops.dropout_mask(n * L * N, c.p_out, SEED, DEV).view(n, L, h, d).permute(0, 2, 1, 3).cpu()
        assert 0.7 < float(keep.mean()) < 0.9
    unit = H.attn_grad_unit(inp["q"], inp["k"], inp["v"], inp["dy"])
    fwd_label, bwd_label = H.ATTN_ROUTE_LABELS[c.route]
    others = {l for pair in H.ATTN_ROUTE_LABELS.values() for l in pair} - {fwd_label, bwd_label}
    worst = WORST.setdefault((c.route, c.dtype), dict.fromkeys(QUANT, 0.0))
    ns = (1, 2, 3, n) if n == 67 else (n,)
    for mode, mask in inp["masks"].items():
        ref = H.attn_ref64(inp["q"], inp["k"], inp["v"], mask, inp["dy"], keep, c.p_out)      # once; prefixes are sliced from it
        mask_d = mask.to(DEV) if mask is not None else None
        for nn in ns:
            (y, dqkv), labels = _profiled(lambda: _launch(c, qkv, mask_d, dy, nn, SEED))
            attn = {l for l in labels if l.startswith(("attn_", "mhsa_"))}
            assert any(l.startswith(fwd_label) for l in attn) and any(l.startswith(bwd_label) for l in attn), (c.route, attn)
            assert not any(l.startswith(o) for l in attn for o in others), (c.route, attn)
            assert y.guards_intact() and dqkv.guards_intact(), (mode, nn)
            yb, gb = y.body.view(n, L * N), dqkv.body.view(n, L * 3 * N)
            assert not bool(torch.isnan(yb[:nn]).any()) and not bool(torch.isnan(gb[:nn]).any()), (mode, nn)     # every element written
            assert bool(torch.isnan(yb[nn:]).all()) and bool(torch.isnan(gb[nn:]).all()), (mode, nn)             # ... and nothing behind
            y2, dqkv2 = _launch(c, qkv, mask_d, dy, nn, SEED)
            assert torch.equal(_bits(y.body), _bits(y2.body)) and torch.equal(_bits(dqkv.body), _bits(dqkv2.body)), (mode, nn)
            yc = yb[:nn].float().cpu().view(nn, L, h, d).permute(0, 2, 1, 3)
            dq, dk, dv = _unpack(gb[:nn].float().cpu().reshape(nn * L, 3 * N), nn, h, L, d)
            got = dict(y=yc, dq=dq, dk=dk, dv=dv)
            m_n = mask[:nn] if mask is not None else None
            err = H.attn_errors(c, got, {k: t[:nn] for k, t in ref.items()}, m_n, unit, H.ATTN_ABS_ZERO[c.dtype])
            print(f"{H.attn_case_id(c)} mask={mode} n={nn}: " + " ".join(f"{k} {e:.2e}" for k, e in err.items()))
            for k in QUANT:
                worst[k] = max(worst[k], err[k])
            if m_n is not None:
                dead = m_n.sum(1) == 0
                if bool(dead.any()):
                    assert float(yc[dead].abs().max()) == 0.0, (mode, nn)                      # all masked: exactly zero
                    assert bool(torch.isfinite(dqkv.body.view(n, -1)[:nn][dead.to(DEV)].float()).all())
            for k in QUANT:
                assert err[k] <= H.ATTN_TOL[c.dtype][k], (H.attn_case_id(c), mode, nn, k, err[k], H.ATTN_TOL[c.dtype][k])


@pytest.mark.parametrize("dtype,heads,d,L,msg", [("bf16", 4, 40, 30, "not instantiated"), ("f32", 4, 12, 40, "not instantiated"),
                                                 ("bf16", 4, 20, 65, "bad shape")])
def test_unsupported_shapes_are_refused_before_any_launch(dtype, heads, d, L, msg):
    assert H.attn_route(dtype, heads, d, L, True) is None
    c = H.AttnCase(dtype, heads, d, L, 3, "aligned", None, "ordinary", 0.0)
    N = heads * d
    qkv = torch.zeros(c.n * L, 3 * N, dtype=_td(c), device=DEV)
    dy = torch.zeros(c.n * L, N, dtype=_td(c), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    y, dqkv = _Out(c.n * L * N, _td(c)), _Out(c.n * L * 3 * N, _td(c))
    args = (c.n, L, heads, d, _code(c), 0.0, 0, stream)
    with pytest.raises(RuntimeError, match=msg):
        _lib.check(_lib.lib().nr_sdpa_fwd(_lib.ptr(qkv), None, _lib.ptr(y.body), *args), "nr_sdpa_fwd")
    with pytest.raises(RuntimeError, match=msg):
        _lib.check(_lib.lib().nr_sdpa_bwd(_lib.ptr(qkv), None, _lib.ptr(dy), _lib.ptr(dqkv.body), *args), "nr_sdpa_bwd")
    with pytest.raises(RuntimeError, match=msg):
        ops.SDPAFunction.apply(qkv, None, c.n, L, heads, d, _code(c))
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.body).all()) and bool(torch.isnan(dqkv.body).all())      # nothing ran
    assert y.guards_intact() and dqkv.guards_intact()


def test_sdpa_function_is_the_same_launch():
    """ops.SDPAFunction (what ops.sdpa and the models call) against the raw C ABI used above: bit-identical y and dqkv."""
    c = CASES[0]
    inp = H.attn_inputs(c)
    n, L, N = c.n, c.L, c.heads * c.d
    qkv = _pack(inp["q"], inp["k"], inp["v"]).to(_td(c)).to(DEV).contiguous().requires_grad_(True)
    dy = inp["dy"].permute(0, 2, 1, 3).reshape(n * L, N).to(_td(c)).to(DEV).contiguous()
    mask = inp["masks"]["rr"].to(DEV)
    y = ops.SDPAFunction.apply(qkv, mask, n, L, c.heads, c.d, _code(c))
    y.backward(dy)
    y0, g0 = _launch(c, qkv.detach(), mask, dy, n, 0)
    assert torch.equal(_bits(y.detach().reshape(-1)), _bits(y0.body)) and torch.equal(_bits(qkv.grad.reshape(-1)), _bits(g0.body))


# ------------------------------------------------------------------- training MHSA with padding substitution
# name: L, heads, d_head, d_model, n, compact rows expected, backward label expected.  n * L is a multiple of 32 and
# >= 16 384 (live 32-row slabs in the weight gradient, which compact row storage and the "_live" sequence list need) except
# in E, whose 4 800 rows are enough for the row compaction (>= 4 096) alone.
MHSA_CASES = {
    "A": (12, 8, 16, 300, 1376, True, "attn_mfma_bwd_rows["),    # per-row substitution + compact rows, FULL generic
    "B": (32, 8, 16, 128, 512, False, "attn_mfma_bwd_live["),    # per-row substitution, no compact storage (L = 32)
    "C": (20, 6, 8, 64, 832, False, "attn_mfma_bwd_live["),      # heads % 4 != 0: per-sequence substitution only
    "D": (30, 4, 32, 64, 560, False, "attn_mfma_bwd_live["),     # PT = 4 with per-sequence substitution
    "E": (30, 20, 20, 300, 160, False, "attn_mfma_bwd["),        # title constants, per-row substitution, dense rows
}


def _mhsa_problem(name, use_mask):
    L, heads, d, D, n, compact, bwd_label = MHSA_CASES[name]
    g = torch.Generator().manual_seed(ord(name) * 7 + int(use_mask))
    V, N = 997, heads * d
    ids = torch.randint(1, V, (n, L), generator=g, dtype=torch.int32)
    ids[torch.rand(n, L, generator=g) < 0.5] = 0                  # ~50 % padding tokens
    ids[::7] = 0                                                  # every 7th sequence all padding
    r = lambda t: t.to(torch.bfloat16).float()                    # bf16-representable: the packed copies are exact
    table = r(torch.randn(V, D, generator=g) * 0.4)
    table[0] = 0
    a = 2 * (6.0 / (N + D)) ** 0.5
    ws = [r((torch.rand(N, D, generator=g) * 2 - 1) * a) for _ in range(3)]
    bs = [(torch.rand(N, generator=g) * 2 - 1) / D ** 0.5 for _ in range(3)]
    dy = r(torch.randn(n, L, N, generator=g) * 0.1)
    mask = None
    if use_mask:
        mask = (torch.rand(n, L, generator=g) < 0.8).float()
        mask[:, 0] = 1
    return ids, table, ws, bs, dy, mask


def _mhsa_reference(ids, table, ws, bs, dy, mask, heads):
    t64 = table.double().requires_grad_(True)
    p64 = [t.double().requires_grad_(True) for t in (ws[0], bs[0], ws[1], bs[1], ws[2], bs[2])]
    y = O.mhsa(O.embed_rows(t64, ids), *p64, n_heads=heads, mask=mask.double() if mask is not None else None)
    y.backward(dy.double())
    return y.detach(), t64.grad, [p.grad for p in p64]


def _mhsa_run(ids, table, ws, bs, dy, mask, heads, needed=None):
    tab = table.to(DEV).requires_grad_(True)
    ps = [t.to(DEV).requires_grad_(True) for t in (ws[0], bs[0], ws[1], bs[1], ws[2], bs[2])]

    def go():
        y = ops.mhsa(None, *ps, heads=heads, code=ops.NR_BF16, mask=mask.to(DEV) if mask is not None else None, ids=ids.to(DEV),
                     table=tab, needed=needed)
        lazy = y._nr_takes_lazy_dy
        y.backward(dy.to(DEV).to(torch.bfloat16))
        return y.detach().float().cpu(), lazy

    (y, lazy), labels = _profiled(go)
    return y, lazy, tab.grad.cpu(), [p.grad.cpu() for p in ps], labels


def _mhsa_check(name, y, dtab, grads, ref, ids, seqs=None):
    """y on the live rows (per-sequence form of the comparator: 2e-2 * max(max|ref| of the sequence, 1e-2 * max|ref|) + 1e-3),
    dW_q|k|v, db_q, db_v and the table gradient (3e-2 * max|ref| + 1e-2); db_k is analytically zero and skipped."""
    y_ref, dtab_ref, g_ref = ref
    n, L = ids.shape
    live = ids != 0
    if seqs is not None:
        live = live & seqs[:, None]
    diff = ((y.double().view(n, L, -1) - y_ref).abs().amax(2) * live).amax(1)
    ymax = y_ref.abs().amax((1, 2))
    bound = 2e-2 * torch.maximum(ymax, 1e-2 * ymax.max()) + 1e-3
    figs = {"y": float((diff / bound).max())}
    assert bool((diff <= bound).all()), (name, "y", float((diff / bound).max()))
    assert bool(torch.isfinite(dtab).all()) and float(dtab[0].abs().max()) == 0.0           # padding_idx row: exactly zero
    for nm, a, b in [("dtable", dtab, dtab_ref)] + [(k, grads[i], g_ref[i]) for i, k in enumerate(("dwq", "dbq", "dwk", "dbk", "dwv", "dbv"))]:
        if nm == "dbk":
            continue
        assert bool(torch.isfinite(a).all()), (name, nm)
        err, tol = float((a.double() - b).abs().max()), 3e-2 * float(b.abs().max()) + 1e-2
        figs[nm] = err / tol
        assert err <= tol, (name, nm, err, tol)
    print(f"mhsa {name}: error / bound " + " ".join(f"{k} {v:.2f}" for k, v in figs.items()))


@pytest.mark.parametrize("name,use_mask", [("A", False), ("A", True), ("B", False), ("B", True), ("C", False), ("D", False), ("E", False)])
def test_training_mhsa_with_padding_substitution_against_fp64(name, use_mask):
    L, heads, d, D, n, compact, bwd_label = MHSA_CASES[name]
    assert (n * L) % 32 == 0 and n * L >= 4096
    prob = _mhsa_problem(name, use_mask)
    ref = _mhsa_reference(*prob, heads)
    y, lazy, dtab, grads, labels = _mhsa_run(*prob, heads)
    attn = sorted(l for l in labels if l.startswith(("attn_", "mhsa_")))
    assert any(l.startswith("attn_mfma_fwd[bf16,") for l in attn), attn
    assert [l for l in attn if l.startswith("attn_mfma_bwd")] and all(l.startswith(bwd_label) for l in attn if l.startswith("attn_mfma_bwd")), attn
    assert lazy is compact
    _mhsa_check(name, y, dtab, grads, ref, prob[0])


def test_training_mhsa_compact_rows_with_mixed_needed_flags():
    """Case A with `needed` flags: the y rows of unneeded sequences are exact zeros (and get a zero gradient by contract)."""
    name = "A"
    L, heads, d, D, n, compact, bwd_label = MHSA_CASES[name]
    ids, table, ws, bs, dy, mask = _mhsa_problem(name, True)
    keep = torch.rand(n, generator=torch.Generator().manual_seed(5)) < 0.6
    dy = dy * keep[:, None, None]
    ref = _mhsa_reference(ids, table, ws, bs, dy, mask, heads)
    y, lazy, dtab, grads, labels = _mhsa_run(ids, table, ws, bs, dy, mask, heads, needed=ops.needed_flags(keep.to(DEV)))
    assert any(l.startswith("attn_mfma_bwd_rows[") for l in labels) and any(l.startswith("attn_mfma_fwd") for l in labels), sorted(labels)
    assert lazy is True
    assert float(y.view(n, -1)[~keep].abs().max()) == 0.0
    _mhsa_check(name + "/needed", y, dtab, grads, ref, ids, seqs=keep)


def test_fused_mhsa_forward_at_a_non_title_shape(monkeypatch):
    """mhsa_fused_fwd (gather + projection + attention in one kernel) runs only without a backward and, in bf16 eval, only when
    the once-projected table is switched off; case A's shape (12 tokens, 8 heads of 16, d_model 300) against fp64."""
    name = "A"
    L, heads, d, D, n, _, _ = MHSA_CASES[name]
    for use_mask in (False, True):
        ids, table, ws, bs, dy, mask = _mhsa_problem(name, use_mask)
        y_ref = _mhsa_reference(ids, table, ws, bs, dy, mask, heads)[0]
        monkeypatch.setattr(ops, "USE_PROJECTED_TABLE", False)
        tab = table.to(DEV)
        ps = [t.to(DEV) for t in (ws[0], bs[0], ws[1], bs[1], ws[2], bs[2])]

        def go():
            with torch.no_grad():
                return ops.mhsa(None, *ps, heads=heads, code=ops.NR_BF16, mask=mask.to(DEV) if mask is not None else None,
                                ids=ids.to(DEV), table=tab).float().cpu()

        y, labels = _profiled(go)
        assert any(l.startswith("mhsa_fused_fwd[") for l in labels) and not any(l.startswith("attn_") for l in labels), sorted(labels)
        live = ids != 0
        diff = ((y.double().view(n, L, -1) - y_ref).abs().amax(2) * live).amax(1)
        ymax = y_ref.abs().amax((1, 2))
        bound = 2e-2 * torch.maximum(ymax, 1e-2 * ymax.max()) + 1e-3
        print(f"mhsa fused fwd mask={use_mask}: error / bound {float((diff / bound).max()):.2f}")
        assert bool((diff <= bound).all()), float((diff / bound).max())
