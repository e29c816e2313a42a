"""GPU: clicked histories of 65 .. 128 slots through every layer -- the attention core (nr_sdpa_long_fwd / nr_sdpa_long_bwd and
ops.LongSDPAFunction), additive pooling, the NRMS and NAML models in training, train.test, train.recommend and the device batch
assembly.

Part 1, the core.  long_helpers.long_cases: L in {65, 95, 96, 97, 100, 127, 128} x (heads, d_head) in {20x20, 4x8, 3x32, 8x16} on
the bf16 matrix-core route (label attn_long_*[bf16), bf16 with qkv one element into its buffer and fp32 with d_head in
{4, 20, 32} on the LDS/VALU kernels (attn_fwd[ / attn_bwd[), one dropout case per family, the three score regimes at 20x20,
L = 100; per case n = 1, 2, 3, 67 sequences, no mask, the seven mask patterns round-robin and, on a 3-block and a 4-block
shape, valid keys only in row block b for every b.  Reference: oracle.nr_oracle.sdpa in fp64 with autograd, comparator and
tolerances (long_helpers.LONG_TOL, from a CPU stand-in and the project's bounds) proven in tests/test_long_history_host.py.
Per launch: outputs go into NaN-filled buffers between sentinel zones (every element written, guards intact), an all-masked
sequence gives exactly zero y, a second launch is bit-identical.

Part 2, pooling against oracle.additive_pool in fp64 (fp32: 1e-4 abs; bf16: 2e-2 max|ref| + 1e-3 outputs, 3e-2 max|ref| + 1e-2
gradients).  Part 3, models against the oracle at the bounds of tests/test_gpu_model_parity.py; train.test at H = 100 within
3e-2 of the oracle's scores; train.recommend with the real tiny NRMS model at H = 80; ops.assemble_batch at H = 100 bit-exact.

Measured on MI355X (worst error / bound over the cases): see DESIGN.md, "Long clicked histories".
"""
import argparse
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import helpers as H
import long_helpers as LH
from oracle import nr_oracle as O
from newsrecommendation_amd import _lib, data as D, ops, train as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, SENTINEL = 4096, 1536.0
SEED = 20241019
CASES = LH.long_cases()
QUANT = ("y", "dq", "dk", "dv")


def _td(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def _code(c):
    return _lib.NR_BF16 if c.dtype == "bf16" else _lib.NR_F32


def _pack(q, k, v):
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
    N, stream = c.heads * c.d, torch.cuda.current_stream().cuda_stream
    y, dqkv = _Out(c.n * c.L * N, _td(c)), _Out(c.n * c.L * 3 * N, _td(c))
    mp = _lib.ptr(mask) if mask is not None else None
    args = (n, c.L, c.heads, c.d, _code(c), float(c.p_out), seed if c.p_out > 0 else 0, stream)
    _lib.check(_lib.lib().nr_sdpa_long_fwd(_lib.ptr(qkv), mp, _lib.ptr(y.body), *args), "nr_sdpa_long_fwd")
    _lib.check(_lib.lib().nr_sdpa_long_bwd(_lib.ptr(qkv), mp, _lib.ptr(dy), _lib.ptr(dqkv.body), *args), "nr_sdpa_long_bwd")
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


def _device_inputs(c, inp):
    n, L, N, td = c.n, c.L, c.heads * c.d, _td(c)
    packed = _pack(inp["q"], inp["k"], inp["v"]).to(td)
    if c.align == "misaligned":             # a contiguous view one element into a larger buffer
        big = torch.zeros(packed.numel() + 16, dtype=td, device=DEV)
        qkv = big[1:1 + packed.numel()].view(packed.shape)
        qkv.copy_(packed)
        assert qkv.data_ptr() % 8 == 2
    else:
        qkv = packed.to(DEV).contiguous()
        assert qkv.data_ptr() % 16 == 0
    dy = inp["dy"].permute(0, 2, 1, 3).reshape(n * L, N).to(td).to(DEV).contiguous()
    return qkv, dy


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_errors_per_route():
    yield
    for (route, dtype), w in sorted(WORST.items()):
        print(f"worst {route} {dtype}: " + " ".join(f"{k} {e:.2e}" for k, e in w.items()))


@pytest.mark.parametrize("c", CASES, ids=H.attn_case_id)
def test_long_attention_core_against_fp64(c):
    inp = LH.long_inputs(c)
    n, h, L, d, N = c.n, c.heads, c.L, c.d, c.heads * c.d
    qkv, dy = _device_inputs(c, inp)
    keep = None
    if c.p_out > 0:
        keep = ops.dropout_mask(n * L * N, c.p_out, SEED, DEV).view(n, L, h, d).permute(0, 2, 1, 3).cpu()
        assert 0.7 < float(keep.mean()) < 0.9
    unit = H.attn_grad_unit(inp["q"], inp["k"], inp["v"], inp["dy"])
    fwd_label, bwd_label = LH.LONG_ROUTE_LABELS[c.route]
    others = LH.ALL_ATTN_LABELS - {fwd_label, bwd_label}
    worst = WORST.setdefault((c.route, c.dtype), dict.fromkeys(QUANT, 0.0))
    for mode, mask in inp["masks"].items():
        ref = H.attn_ref64(inp["q"], inp["k"], inp["v"], mask, inp["dy"], keep, c.p_out)
        mask_d = mask.to(DEV) if mask is not None else None
        for nn in (1, 2, 3, n):
            (y, dqkv), labels = _profiled(lambda: _launch(c, qkv, mask_d, dy, nn, SEED))
            attn = {l for l in labels if l.startswith(("attn_", "mhsa_"))}
            assert any(l.startswith(fwd_label) for l in attn) and any(l.startswith(bwd_label) for l in attn), (c.route, attn)
            assert not any(l.startswith(o) for l in attn for o in others), (c.route, attn)
            assert y.guards_intact() and dqkv.guards_intact(), (mode, nn)
            yb, gb = y.body.view(n, L * N), dqkv.body.view(n, L * 3 * N)
            assert not bool(torch.isnan(yb[:nn]).any()) and not bool(torch.isnan(gb[:nn]).any()), (mode, nn)
            assert bool(torch.isnan(yb[nn:]).all()) and bool(torch.isnan(gb[nn:]).all()), (mode, nn)
            y2, dqkv2 = _launch(c, qkv, mask_d, dy, nn, SEED)
            assert torch.equal(_bits(y.body), _bits(y2.body)) and torch.equal(_bits(dqkv.body), _bits(dqkv2.body)), (mode, nn)
            yc = yb[:nn].float().cpu().view(nn, L, h, d).permute(0, 2, 1, 3)
            dq, dk, dv = _unpack(gb[:nn].float().cpu().reshape(nn * L, 3 * N), nn, h, L, d)
            m_n = mask[:nn] if mask is not None else None
            err = H.attn_errors(c, dict(y=yc, dq=dq, dk=dk, dv=dv), {k: t[:nn] for k, t in ref.items()}, m_n, unit, LH.LONG_ABS_ZERO[c.dtype])
            print(f"{H.attn_case_id(c)} mask={mode} n={nn}: " + " ".join(f"{k} {e:.2e}" for k, e in err.items()))
            for k in QUANT:
                worst[k] = max(worst[k], err[k])
            if m_n is not None:
                dead = m_n.sum(1) == 0
                if bool(dead.any()):
                    assert float(yc[dead].abs().max()) == 0.0, (mode, nn)
                    assert bool(torch.isfinite(dqkv.body.view(n, -1)[:nn][dead.to(DEV)].float()).all())
            for k in QUANT:
                assert err[k] <= LH.LONG_TOL[c.dtype][k], (H.attn_case_id(c), mode, nn, k, err[k], LH.LONG_TOL[c.dtype][k])


@pytest.mark.parametrize("i", [k for k, c in enumerate(CASES) if (c.L, c.regime, c.p_out) == (100, "ordinary", 0.0)],
                         ids=lambda k: H.attn_case_id(CASES[k]))
def test_long_sdpa_function_is_the_same_launch(i):
    """ops.LongSDPAFunction (what ops.sdpa dispatches to above 64 slots) against the raw pair: bit-identical y and dqkv."""
    c = CASES[i]
    inp = LH.long_inputs(c)
    n, L = c.n, c.L
    qkv, dy = _device_inputs(c, inp)
    mask = inp["masks"]["rr"].to(DEV)
    leaf = qkv.detach().requires_grad_(True)
    y = ops.LongSDPAFunction.apply(leaf, mask, n, L, c.heads, c.d, _code(c))
    y.backward(dy)
    y0, g0 = _launch(c, qkv, mask, dy, n, 0)
    assert torch.equal(_bits(y.detach().reshape(-1)), _bits(y0.body)) and torch.equal(_bits(leaf.grad.reshape(-1)), _bits(g0.body))


def test_ops_sdpa_dispatches_by_length_and_both_pairs_refuse_the_other_side():
    g = torch.Generator().manual_seed(3)
    for L, label in ((64, "attn_mfma_fwd[bf16,"), (65, "attn_long_fwd[bf16,")):
        q, k, v = (torch.randn(2, 4, L, 8, generator=g).to(DEV) for _ in range(3))
        y, labels = _profiled(lambda: ops.sdpa(q, k, v, ops.NR_BF16))
        assert any(l.startswith(label) for l in labels), (L, sorted(labels))
        ref = O.sdpa(q.to(torch.bfloat16).double().cpu(), k.to(torch.bfloat16).double().cpu(), v.to(torch.bfloat16).double().cpu())
        assert float((y.double().cpu() - ref).abs().max()) <= 2e-2 * float(ref.abs().max())
    z = torch.zeros(3 * 64, 3 * 32, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match=r"\[65, 128\]"):
        ops.LongSDPAFunction.apply(z, None, 3, 64, 4, 8, ops.NR_BF16)
    z = torch.zeros(3 * 65, 3 * 32, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="bad shape"):
        ops.SDPAFunction.apply(z, None, 3, 65, 4, 8, ops.NR_BF16)


# ------------------------------------------------------------------------------------------ pooling
POOL_CASES = [(L, N, q, n) for L in (65, 100, 128) for (N, q, ns) in ((8, 8, (1, 9, 2049, 8200)), (400, 200, (1, 9))) for n in ns]


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("L,N,q,n", POOL_CASES)
def test_long_additive_pool_against_fp64(L, N, q, n, dt):
    """Forward and every gradient against oracle.additive_pool in fp64; the seven mask patterns round-robin (all-masked
    sequences give exact zeros and a zero input gradient); n crosses the thresholds of the backward's sequences per workgroup.
    The upstream gradient is scaled by 1 / sqrt(n) so that the weight gradients stay of order one at every n."""
    code = ops.dtype_code(dt)
    g = torch.Generator().manual_seed(L * 1000 + N + n)
    r = lambda t: t.to(torch.bfloat16).float()
    x = r(torch.randn(n, L, N, generator=g))
    w1, b1 = r(torch.randn(q, N, generator=g) / N ** 0.5), torch.randn(q, generator=g) * 0.1
    w2, b2 = torch.randn(1, q, generator=g) / q ** 0.5, torch.randn(1, generator=g) * 0.1
    mask, kind = H.masks(n, L, g)
    dout = torch.randn(n, N, generator=g) / n ** 0.5
    p64 = [t.double().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    ref = O.additive_pool(*p64, mask=mask.double())
    ref.backward(dout.double())
    xd = x.to(ops.torch_dtype(code)).to(DEV).requires_grad_(True)
    ps = [t.to(DEV).requires_grad_(True) for t in (w1, b1, w2, b2)]
    out = ops.additive_pool(xd, *ps, code, mask=mask.to(DEV))
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    dead = mask.sum(1) == 0
    if n >= 7:
        assert bool(dead.any())
    if bool(dead.any()):
        assert float(out[dead.to(DEV)].abs().max()) == 0.0 and float(xd.grad[dead.to(DEV)].float().abs().max()) == 0.0
    got = [out, xd.grad] + [p.grad for p in ps]
    want = [ref.detach()] + [p.grad for p in p64]
    for i, (name, a, b) in enumerate(zip(("out", "dx", "dw1", "db1", "dw2", "db2"), got, want)):
        assert bool(torch.isfinite(a.float()).all()), name
        err, mx = float((a.detach().double().cpu().reshape(b.shape) - b).abs().max()), float(b.abs().max())
        tol = 1e-4 if dt == "fp32" else ((2e-2 * mx + 1e-3) if i == 0 else (3e-2 * mx + 1e-2))
        print(f"pool L={L} N={N} q={q} n={n} {dt} {name}: err {err:.2e} bound {tol:.2e}")
        assert err <= tol, (name, err, tol)


# ------------------------------------------------------------------------------------------ models
TINY = dict(num_words_title=4, npratio=1, word_embedding_dim=8, news_dim=8, num_attention_heads=2, news_query_vector_dim=4,
            user_query_vector_dim=4, category_emb_dim=5)
# bf16 operands come in 16-byte chunks: the tiny dims rounded up to multiples of 8
TINY_BF16 = dict(TINY, news_dim=16, news_query_vector_dim=8, user_query_vector_dim=8, category_emb_dim=8)
MIND = {}
MODEL_TOL = {"fp32": (1e-4, 2e-4, 1e-6), "bf16": (3e-2, 1e-1, 3e-4)}


def _front_padded(B, Hn, g):
    """[B, Hn] 0/1 masks of front-padded histories with 0 .. Hn live slots: a length-0 row, a full row, the edges of the
    32-row blocks, and random lengths."""
    forced = [0, Hn, 1, 31, 32, 33, 63, 64, 65, Hn - 1]
    hl = torch.tensor((forced + torch.randint(0, Hn + 1, (max(0, B - len(forced)),), generator=g).tolist())[:B])
    return (torch.arange(Hn)[None, :] >= (Hn - hl)[:, None]).float()


def _model_problem(model, Hn, ulm, dims, B, seed):
    g = torch.Generator().manual_seed(seed)
    naml = model == "NAML"
    cfg = O.default_cfg(user_log_length=Hn, user_log_mask=ulm, **dims,
                        **(dict(use_category=True, use_subcategory=True, freeze_embedding=True) if naml else {}))
    T, Dw, C = cfg.num_words_title, cfg.word_embedding_dim, 1 + cfg.npratio
    mask = _front_padded(B, Hn, g)
    label = torch.randint(0, C, (B,), generator=g, dtype=torch.int64)
    if naml:
        n_news, n_cat, n_sub = 40, 4, 6
        table = torch.randn(n_news + 1, T * Dw, generator=g) * 0.4
        table[0] = 0
        sd = O.init_state_dict("NAML", cfg, table, seed=seed + 1, n_cat=n_cat, n_sub=n_sub)
        ids = lambda shape: torch.stack([torch.randint(1, n_news + 1, shape, generator=g, dtype=torch.int32),
                                         torch.randint(0, n_cat + 1, shape, generator=g, dtype=torch.int32),
                                         torch.randint(0, n_sub + 1, shape, generator=g, dtype=torch.int32)], dim=-1)
        hist, cand = ids((B, Hn)), ids((B, C))
        extra = (n_cat, n_sub)
    else:
        V = 60
        table = torch.randn(V, Dw, generator=g) * 0.4
        table[0] = 0
        sd = O.init_state_dict("NRMS", cfg, table, seed=seed + 1)
        hist = torch.randint(1, V, (B, Hn, T), generator=g, dtype=torch.int32)
        cand = torch.randint(1, V, (B, C, T), generator=g, dtype=torch.int32)
        for t in (hist, cand):
            ln = torch.randint(1, T + 1, t.shape[:2], generator=g)
            t[torch.arange(T)[None, None, :] >= ln[..., None]] = 0
        extra = ()
    hist[mask == 0] = 0
    return cfg, table, sd, (hist, mask, cand, label), extra


def _run_against_oracle(model, dt, cfg, table, sd, batch, extra):
    from newsrecommendation_amd.model import NAML, NRMS
    hist, mask, cand, label = batch
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    fwd = O.naml_forward if model == "NAML" else O.nrms_forward
    lo, so = fwd(hist.long() if model == "NAML" else hist, mask, cand.long() if model == "NAML" else cand, label, sdo, cfg, keep=None)
    lo.backward()
    args = SimpleNamespace(**vars(cfg), compute_dtype=dt)
    m = (NAML.Model(args, table.numpy(), *extra) if model == "NAML" else NRMS.Model(args, table.numpy()))
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    def step():
        loss, score = m(hist.cuda(), mask.cuda(), cand.cuda(), label.cuda())
        loss.backward()
        return loss, score

    (loss, score), labels = _profiled(step)
    tol, gtol, gatol = MODEL_TOL[dt]
    H.assert_close(loss, lo.detach(), tol, name="loss")
    H.assert_close(score, so.detach(), tol, name="score")
    checked = 0
    for name, p in m.named_parameters():
        if p.requires_grad and name in sdo and sdo[name].grad is not None:
            assert p.grad is not None, name
            H.assert_close(p.grad, sdo[name].grad, gatol, gtol, name="d" + name)
            checked += 1
    assert checked >= (8 if model == "NRMS" else 6)
    return labels


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("ulm", [True, False])
@pytest.mark.parametrize("Hn", [65, 100])
@pytest.mark.parametrize("model", ["NRMS", "NAML"])
def test_models_at_tiny_dims_against_the_oracle(model, Hn, ulm, dt):
    """The golden tiny cases' dims (rounded up to bf16's 8-element chunks in bf16) with user_log_length = Hn: loss, scores and
    every parameter gradient.  NRMS runs MHSA and pooling over the Hn slots, NAML pooling alone; user_log_mask=False adds the
    pad_doc blend."""
    dims = TINY if dt == "fp32" else TINY_BF16
    labels = _run_against_oracle(model, dt, *_model_problem(model, Hn, ulm, dims, B=12, seed=Hn + 7 * ulm))
    assert any(l.startswith("pool_core_fwd[") and f",L={Hn}," in l for l in labels), sorted(labels)
    if model == "NRMS":
        want = "attn_long_fwd[bf16," if dt == "bf16" else "attn_fwd[f32,"
        assert any(l.startswith(want) and f",L={Hn}," in l for l in labels), sorted(labels)


@pytest.mark.parametrize("model", ["NRMS", "NAML"])
def test_models_at_mind_dims_with_100_slots(model):
    """B = 8, H = 100, T = 30, D = 300, N = 400, 20 heads, bf16, masked user encoder."""
    labels = _run_against_oracle(model, "bf16", *_model_problem(model, 100, True, MIND, B=8, seed=100))
    if model == "NRMS":
        for pre in ("attn_long_fwd[bf16,", "attn_long_bwd[bf16,"):
            assert any(l.startswith(pre) and ",L=100,h=20,d=20]" in l for l in labels), sorted(labels)


# ------------------------------------------------------------------------------------------ train.test at H = 100
def _rounded64(sd):
    return {k: (v.to(torch.bfloat16) if v.dim() >= 2 else v).double() for k, v in sd.items()}


def test_train_test_at_100_slots_against_the_fp64_oracle(tmp_path):
    """NRMS, bf16, user_log_mask=True, ~300 news, ~200 impressions with histories of 0 .. 110 clicks (truncated to 100): those
    with at most 32 live slots go through the 32-row gather path, the others through the general path at L = 100.  Every score
    within 3e-2 of the oracle's, which encodes all 100 slots of every impression."""
    Hn, T, WD, V, n_news, n_imp = 100, 30, 300, 2000, 300, 200
    rnd = random.Random(5)
    news_ids = [f"N{i}" for i in range(1, n_news + 1)]
    news_index = {nid: i + 1 for i, nid in enumerate(news_ids)}
    g = torch.Generator().manual_seed(5)
    comb = torch.randint(1, V, (n_news + 1, T), generator=g, dtype=torch.int32)
    comb[0] = 0
    for r_ in range(1, n_news + 1):
        comb[r_, rnd.randint(3, T):] = 0
    table = torch.randn(V, WD, generator=g) * 0.4
    table[0] = 0
    forced = (0, 1, 31, 32, 33, 63, 64, 65, 67, 68, 69, 96, 97, 99, 100, 101, 110)
    lines = []
    for i in range(n_imp):
        hl = forced[i] if i < len(forced) else rnd.randint(0, 110)
        hist = " ".join(rnd.choice(news_ids) for _ in range(hl))
        cands = [rnd.choice(news_ids) for _ in range(rnd.randint(2, 12))]
        labs = [1 if rnd.random() < 0.3 else 0 for _ in cands]
        labs[0], labs[1] = 1, 0
        lines.append("\t".join([str(i + 1), "U1", "t", hist, " ".join(f"{c}-{l}" for c, l in zip(cands, labs))]) + "\n")
    os.makedirs(tmp_path / "test", exist_ok=True)
    (tmp_path / "test" / "behaviors.tsv").write_text("".join(lines))
    D.prepare_testing_data(str(tmp_path / "test"), 1)
    cfg = O.default_cfg(user_log_length=Hn, user_log_mask=True)
    args = SimpleNamespace(**vars(cfg), model="NRMS", compute_dtype="bf16", batch_size=128, test_data_dir=str(tmp_path / "test"))
    sd = O.init_state_dict("NRMS", args, table, seed=6)
    from newsrecommendation_amd.model import NRMS
    m = NRMS.Model(args, table.numpy())
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    shard = D.IndexedTestShard(os.path.join(args.test_data_dir, "behaviors_0.tsv"), news_index, args)
    groups, _ = TR._short_history_split(shard, Hn)
    assert len(groups[0][0]) > 10 and len(groups[1][0]) > 100 and groups[0][1] == Hn - 32
    got = []
    (n_seen, means), labels = _profiled(lambda: TR.test(None, args, m, news_index, comb.numpy(), log=lambda *_: None, collect_scores=got))
    assert n_seen == n_imp
    assert any(l.startswith("attn_long_fwd[bf16,") and ",L=100," in l for l in labels), sorted(labels)
    assert any(l.startswith("attn_mfma_fwd_gather[") and ",L=32," in l for l in labels), sorted(labels)
    sd_o = _rounded64(sd)
    nv_o = O.nrms_news_encoder(comb.long(), sd_o, args)
    out_lines = open(os.path.join(args.test_data_dir, "behaviors_0.tsv")).readlines()
    parsed = [O.test_line_to_indices(l, news_index, Hn) for l in out_lines]
    hist = torch.as_tensor(np.stack([p[0] for p in parsed]), dtype=torch.long)
    mask = torch.from_numpy(np.stack([p[1] for p in parsed])).double()
    assert hist.shape == (n_imp, Hn) and int((mask.sum(1) == Hn).sum()) >= 3 and int((mask.sum(1) > 64).sum()) > 50
    assert np.array_equal(hist.numpy(), shard.hist) and np.array_equal(mask.numpy(), shard.mask)     # all 100 slots, both sides
    uv = O.nrms_user_encoder(nv_o[hist], mask, sd_o, args)
    worst = 0.0
    for (h_, m_, cand, labs), (lab_g, s_g), u in zip(parsed, got, uv):
        assert np.array_equal(labs, lab_g)
        worst = max(worst, float(np.abs(s_g - (nv_o[cand] @ u).numpy()).max()))
    print(f"train.test H=100 bf16: worst score error {worst:.2e}")
    assert worst <= 3e-2


# ------------------------------------------------------------------------------------------ train.recommend at H = 80
def test_recommend_and_rank_eval_with_the_real_tiny_model_at_80_slots():
    """The real NRMS user encoder (fp32, tiny golden model) over 80 history slots: user vectors equal the oracle's within 1e-4,
    no recommended id is in the history, and rank_eval ranks every target but the clicked ones."""
    real, z, cfg, sd = H.build_model("nrms_tiny_mask", "fp32")
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(80)
    n_news, U, Hn, k = 300, 9, 80, 10
    V, T = sd[H.table_key("nrms_tiny_mask")].shape[0], cfg.num_words_title
    comb = torch.randint(1, V, (n_news + 1, T), generator=g, dtype=torch.int32)
    comb[0] = 0
    news_vecs = TR.encode_news(real, comb.numpy(), 64, dev)
    hist = torch.randint(1, n_news + 1, (U, Hn), generator=g, dtype=torch.int32)
    mask = _front_padded(U, Hn, g)
    hist[mask == 0] = 0
    uv = TR._user_vectors(real, news_vecs, hist.cuda(), mask.cuda(), 8192, dev, TR._Histories(mask.numpy()))
    sd64 = {k_: v.double() for k_, v in sd.items()}
    uv_o = O.nrms_user_encoder(news_vecs.double().cpu()[hist.long()], mask.double(), sd64, cfg)
    err = float((uv.double().cpu() - uv_o).abs().max())
    print(f"recommend H=80: user vector error {err:.2e}")
    assert err <= 1e-4
    ids, sc = TR.recommend(real, news_vecs, hist.numpy(), mask.numpy(), k)
    ids = ids.cpu().numpy()
    assert ids.shape == (U, k)
    for u in range(U):
        clicked = set(hist[u][mask[u] != 0].tolist())
        assert not (clicked & set(ids[u].tolist())) and 0 not in ids[u].tolist()
    full = int((mask.sum(1) == Hn).nonzero()[0])
    assert len(set(hist[full].tolist())) > 64                           # more distinct clicks than the dense exclusion list holds
    # rank_eval over the same user vectors: a clicked target is not ranked, the others are, with the scores of those vectors
    tg = torch.randint(1, n_news + 1, (U, 6), generator=g, dtype=torch.int32).numpy()
    tg[:, 0] = hist[:, -1].numpy()                                      # the last slot: clicked wherever the history is not empty
    ranks, rsc, sums = TR.rank_eval(real, news_vecs, hist.numpy(), mask.numpy(), tg, ks=(5, 10))
    ranks, rsc = ranks.cpu().numpy(), rsc.cpu().numpy()
    want = (uv_o @ news_vecs.double().cpu().T).numpy()
    for u in range(U):
        clicked = set(hist[u][mask[u] != 0].tolist())
        for j in range(tg.shape[1]):
            if int(tg[u, j]) == 0 or int(tg[u, j]) in clicked or int(tg[u, j]) in tg[u, :j].tolist():
                assert ranks[u, j] == 0, (u, j)
            else:
                assert 1 <= ranks[u, j] <= n_news and abs(float(rsc[u, j]) - want[u, tg[u, j]]) <= 1e-4, (u, j, ranks[u, j])
    assert (ranks[mask.sum(1).numpy() > 0, 0] == 0).all() and (ranks > 0).sum() > 2 * U


# ------------------------------------------------------------------------------------------ batch assembly at H = 100
def test_assemble_batch_at_100_slots_is_bit_exact_with_the_host_stream(tmp_path):
    Hn, K, n_news, F = 100, 4, 500, 7
    rnd = random.Random(9)
    news_ids = [f"N{i}" for i in range(1, n_news + 1)]
    news_index = {nid: i + 1 for i, nid in enumerate(news_ids)}
    lines = []
    for i, hl in enumerate([0, 1, 64, 65, 99, 100, 101, 130] + [rnd.randint(0, 130) for _ in range(29)]):
        hist = " ".join(rnd.choice(news_ids) for _ in range(hl))
        lines.append("\t".join([str(i), "U", "t", hist, rnd.choice(news_ids), " ".join(rnd.choice(news_ids) for _ in range(K))]) + "\n")
    f = tmp_path / "train_0.tsv"
    f.write_text("".join(lines))
    args = argparse.Namespace(user_log_length=Hn, npratio=K)
    comb = np.random.RandomState(0).randint(1, 1000, size=(n_news + 1, F)).astype(np.int32)
    comb[0] = 0
    shard = D.IndexedTrainShard(str(f), news_index, args)
    assert shard.hist.shape == (len(lines), Hn)
    feed = TR.DeviceFeed(shard, comb, batch_size=8, device="cuda")
    random.seed(11)
    feed.start_epoch()
    parts = [[t.cpu() for t in feed.batch(i)] for i in range(len(feed))]
    h, m, c, l = (torch.cat([p[j] for p in parts]).numpy() for j in range(4))
    random.seed(11)
    ds = D.DatasetTrain(str(f), news_index, comb, args)
    hb, mb, cb, lb = next(iter(torch.utils.data.DataLoader(ds, batch_size=len(lines))))
    n = h.shape[0]
    assert n >= len(lines) // 8 * 8 and h.shape[1:] == (Hn, F)
    assert np.array_equal(hb.numpy()[:n], h) and np.array_equal(mb.numpy()[:n], m) and np.array_equal(cb.numpy()[:n], c) and np.array_equal(lb.numpy()[:n], l)
    assert (m.sum(1) == Hn).any() and (m.sum(1) == 0).any()
