"""GPU: oracle parity at PRODUCTION scale -- the kernels that make up the benchmarked step.

The live-row / live-slab / sequence-list paths of libnrhip are size gated (M % 32 == 0 and M >= 200 000 token rows):
the golden cases (M <= 6 600) never reach them.  B = 128 gives M = 128 * 55 * 30 = 211 200 rows, which does, on a
MIND-shaped batch (bench.synth_batches: title tails zero padded, empty history slots, front-padded histories), and the
CPU oracle still finishes it in seconds.  Every case compares loss, score and EVERY parameter gradient at full resolution
with oracle.nrms_forward / naml_forward, asserts through the library's own launch log that the size-gated kernels
really ran, and pre-fills the buffers those kernels leave partly unwritten (qkv / dqkv rows of all-padding sequences)
with NaN so that a read of an unwritten row cannot pass silently.

Tolerances (measured on MI355X, then fixed here):
  fp32 compute: loss / score 1e-4 abs (north_star), gradients 2e-4 * max|g| + 1e-6.
  bf16 compute: loss / score 3e-2 abs; gradients 3e-2 * max|g| + 3e-4 -- the absolute floor covers d W_K.bias, which is
  analytically ~0 (a constant key shift leaves the softmax unchanged) so only bf16 rounding noise of dK remains.
"""
from types import SimpleNamespace

import pytest
import torch

import bench
from helpers import assert_close
from newsrecommendation_amd import _lib, ops
from oracle import nr_oracle as O

pytestmark = pytest.mark.gpu
B = 128


def _launched():
    return set(_lib.prof_collect().keys())


def _has(labels, prefix):
    return any(l.startswith(prefix) for l in labels)


def _grad_report(model, oracle_grads, atol, rtol):
    worst = {}
    for name, p in model.named_parameters():
        if not p.requires_grad or name not in oracle_grads:
            continue
        assert p.grad is not None, name
        assert torch.isfinite(p.grad).all(), f"non-finite gradient in {name} (an unwritten workspace row was read?)"
        ref = oracle_grads[name]
        err = float((p.grad.detach().double().cpu() - ref.double()).abs().max())
        worst[name] = err / (float(ref.abs().max()) + 1e-30)
        assert_close(p.grad, ref, atol, rtol, name="d" + name)
    return worst


def _nrms_case(dt, seed, B=B, V=5000, freeze_embedding=False, user_log_mask=False):
    cfg = O.default_cfg(freeze_embedding=freeze_embedding, user_log_mask=user_log_mask)
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(V, cfg.word_embedding_dim, generator=g) * 0.4
    table[0] = 0
    sd = O.init_state_dict("NRMS", cfg, table, seed=seed + 1)
    from newsrecommendation_amd.model import NRMS
    args = SimpleNamespace(**vars(cfg), compute_dtype=dt)
    m = NRMS.Model(args, table.numpy())
    m.load_state_dict(sd, strict=True)
    hist, mask, cand, label = bench.synth_batches(cfg, B, V, 1, seed + 2, "cpu")[0]
    # the shape the gates need, and the padding structure the skips act on
    assert (B * 55 * 30) % 32 == 0 and B * 55 * 30 >= 200000
    assert int((hist == 0).all(-1).sum()) > B and float((hist == 0).float().mean()) > 0.5 and int((mask.sum(1) == 0).sum()) >= 1
    cand[0, 1] = 0                                     # an all-padding CANDIDATE title (unknown news -> index 0, dataset.py:15)
    return cfg, sd, m.cuda(), (hist, mask, cand, label)


TOL = {"fp32": dict(tol=1e-4, gatol=1e-6, grtol=2e-4), "bf16": dict(tol=3e-2, gatol=3e-4, grtol=3e-2)}


# every size-gated kernel of the benchmarked bf16 step (round-1 and round-2 paths alike): the launch log must show them
# (round 3: compact row storage -- the live rows only in x_rows / dqkv: rows_materialize_live, attn_mfma_bwd_rows, gemm_tn3_rows)
#  fused additive pooling: pool_fused_fwd, pool_fused_bwd)
STEP_KERNELS = ("gemm_tn3_live", "gemm_tn3_rows", "attn_mfma_bwd_rows", "gemm_nt_dma_live", "attn_mfma_fwd_live", "needed_list", "pool_fused_fwd",
                "pool_fused_bwd", "gemm_nt_wreg_live", "rows_materialize_live", "sort_rows_by_id")


def _nrms_against_the_oracle(dt, train, B, V, seed, freeze_embedding=False, user_log_mask=False):
    cfg, sd, m, (hist, mask, cand, label) = _nrms_case(dt, seed, B, V, freeze_embedding, user_log_mask)
    tkey = "news_encoder.embedding_matrix.weight"
    t = TOL[dt]
    m.train(train)
    keep = None
    ops.POISON_WORKSPACES = True
    _lib.prof_enable(1)
    try:
        _lib.prof_collect()
        if train:
            torch.manual_seed(4321)
            seed_in, seed_out = ops.draw_seed(), ops.draw_seed()        # the two draws NewsEncoder.forward makes
            torch.manual_seed(4321)
        loss, score = m(hist.cuda(), mask.cuda(), cand.cuda(), label.cuda())
        loss.backward()
        torch.cuda.synchronize()
        labels = _launched()
    finally:
        _lib.prof_enable(0)
        ops.POISON_WORKSPACES = False
    if dt == "bf16":
        # the kernels of the benchmarked step, not their small-shape stand-ins
        for want in STEP_KERNELS:
            if freeze_embedding and want in ("sort_rows_by_id", "gemm_nt_dma_live"):
                continue
            assert _has(labels, want), (want, sorted(labels))
        if freeze_embedding:
            # a frozen table: compact row storage still runs (attention backward, dW over the live rows), the table-gradient
            # half of it -- the id sort and the scatter-epilogue GEMM -- does not
            assert not _has(labels, "sort_rows_by_id") and not _has(labels, "gemm_nt_dma_live[bf16,epi=2,"), sorted(labels)
    if train:
        n, T, D, N, p = B * 55, cfg.num_words_title, cfg.word_embedding_dim, cfg.news_dim, cfg.drop_rate
        word = ops.dropout_mask(n * T * D, p, seed_in, "cuda").cpu().reshape(n, T, D)
        ctx = ops.dropout_mask(n * T * N, p, seed_out, "cuda").cpu().reshape(n, T, N)
        nc = B * 5
        keep = {"cand_word": word[:nc], "hist_word": word[nc:], "cand_ctx": ctx[:nc], "hist_ctx": ctx[nc:]}
    sdo = {k: v.clone().requires_grad_(not (freeze_embedding and k == tkey)) for k, v in sd.items()}
    lo, so = O.nrms_forward(hist, mask, cand, label, sdo, cfg, keep=keep)
    lo.backward()
    assert torch.isfinite(score).all() and torch.isfinite(loss)
    assert_close(loss, lo.detach(), t["tol"], name="loss")
    assert_close(score, so.detach(), t["tol"], name="score")
    worst = _grad_report(m, {k: v.grad for k, v in sdo.items() if v.grad is not None}, t["gatol"], t["grtol"])
    print(f"nrms B={B} {dt} train={train} freeze={freeze_embedding} ulm={user_log_mask}: loss {float(loss):.6f} vs {float(lo):.6f}; worst grad err / max|g|: "
          + ", ".join(f"{k.split('.', 1)[1]}={v:.2e}" for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:5]))
    tab = dict(m.named_parameters())[tkey]
    if freeze_embedding:
        assert not tab.requires_grad and tab.grad is None
    else:                                                                 # table trainable
        assert float(tab.grad[0].abs().max()) == 0.0                      # padding_idx row
    return labels


@pytest.mark.parametrize("dt,train", [("bf16", False), ("bf16", True), ("fp32", False)])
def test_nrms_b128_every_gradient_against_the_oracle(dt, train):
    _nrms_against_the_oracle(dt, train, B, 5000, 40)


def test_nrms_b512_benched_shape_every_gradient_against_the_oracle():
    """THE benchmarked configuration itself, once: B = 512 (M = 844 800 token rows, 28 160 titles), bf16, training mode with
    the kernels' dropout draws exported to the oracle, a 30 000-row trainable word table (bench.py's workload), poisoned
    workspaces.  Grid-dependent logic -- 8 XCD x persistent-workgroup block lists, whole-chip slab flags, the one-workgroup
    list / scan kernels, the id sort over 275 k live rows -- runs here at the size the bench line is quoted on.  Loss, all
    2 560 scores and EVERY gradient (incl. the full [30 000, 300] table gradient) against the CPU oracle; ~40 s of oracle."""
    _nrms_against_the_oracle("bf16", True, 512, 30000, 60)


@pytest.mark.parametrize("dt,train", [("bf16", True), ("fp32", False)])
def test_naml_b128_every_gradient_against_the_oracle(dt, train):
    cfg = O.default_cfg(use_category=True, use_subcategory=True, freeze_embedding=True)
    g = torch.Generator().manual_seed(50)
    n_news = 2500
    T, D = cfg.num_words_title, cfg.word_embedding_dim
    table = torch.randn(n_news + 1, T * D, generator=g) * 0.4
    table[0] = 0
    sd = O.init_state_dict("NAML", cfg, table, seed=51, n_cat=17, n_sub=264)
    from newsrecommendation_amd.model import NAML
    args = SimpleNamespace(**vars(cfg), compute_dtype=dt)
    m = NAML.Model(args, table.numpy(), 17, 264)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train(train)
    hist, mask, cand, label = bench.synth_batches_naml(cfg, B, n_news, 1, 52, "cpu")[0]
    assert int((mask == 0).sum()) > B                                     # masked history slots: zero upstream gradient
    t = TOL[dt]
    _lib.prof_enable(1)
    try:
        _lib.prof_collect()
        if train:
            torch.manual_seed(99)
            seed_in = ops.draw_seed()
            torch.manual_seed(99)
        loss, score = m(hist.cuda(), mask.cuda(), cand.cuda(), label.cuda())
        loss.backward()
        torch.cuda.synchronize()
        labels = _launched()
    finally:
        _lib.prof_enable(0)
    if dt == "bf16":
        assert _has(labels, "gemm_tn3_live"), sorted(labels)                # conv dW over the live slabs
    keep = None
    if train:
        n = B * 55
        word = ops.dropout_mask(n * T * D, cfg.drop_rate, seed_in, "cuda").cpu().reshape(n, T, D)
        keep = {"cand_word": word[: B * 5], "hist_word": word[B * 5:]}
    sdo = {k: v.clone().requires_grad_(k != "news_encoder.title_embeddings.weight") for k, v in sd.items()}
    lo, so = O.naml_forward(hist, mask, cand, label, sdo, cfg, keep=keep)
    lo.backward()
    assert_close(loss, lo.detach(), t["tol"], name="loss")
    assert_close(score, so.detach(), t["tol"], name="score")
    worst = _grad_report(m, {k: v.grad for k, v in sdo.items() if v.grad is not None}, t["gatol"], t["grtol"])
    print(f"naml B={B} {dt} train={train}: worst grad err / max|g|: "
          + ", ".join(f"{k.split('.', 1)[1]}={v:.2e}" for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:5]))


@pytest.mark.parametrize("train", [False, True])
def test_needed_flags_change_nothing_observable(train):
    """`Model.forward` tells the news encoder which history slots are masked (their vectors reach the loss through a factor 0);
    the kernels then skip them.  Against `args.encode_masked_slots=True` (every title encoded, as the reference does): the same
    loss, scores and gradients -- dropout counters keep the original element indices, so training mode draws the same masks.
    What differs is the order of fp32 atomics only."""
    outs = []
    for encode_all in (True, False):
        cfg, sd, m, (hist, mask, cand, label) = _nrms_case("bf16", 60)
        m.args.encode_masked_slots = encode_all
        m.train(train)
        torch.manual_seed(777)
        loss, score = m(hist.cuda(), mask.cuda(), cand.cuda(), label.cuda())
        loss.backward()
        outs.append((loss.detach().clone(), score.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    (l0, s0, g0), (l1, s1, g1) = outs
    assert torch.equal(s0, s1) and torch.equal(l0, l1)            # forward: bit-identical
    assert g0.keys() == g1.keys()
    for k in g0:
        assert float((g0[k] - g1[k]).abs().max()) <= 1e-5 * float(g0[k].abs().max()) + 1e-8, k


@pytest.mark.parametrize("train", [False, True])
def test_compact_row_storage_changes_nothing_observable(train):
    """Round 3: on the news-level training path x_rows and dqkv hold the LIVE rows only (non-padding tokens, in live-list
    order), the attention backward stores no gradient row for a padding token and produces the bias gradient itself (row /
    column sums of dS and P through the spare 32nd token of its tiles), and the weight-gradient GEMM contracts the live rows
    densely.  Against NR_NO_COMPACT_ROWS = 1 (one row per token, db from the weight-gradient GEMM's selector MFMA): the
    forward is bit-identical; dW_qkv, the table gradient and everything upstream agree up to the order of fp32 additions;
    db_qkv -- a different summation of the same bf16-rounded factors -- to 2e-3 * max|g| (d W_K.bias, analytically ~0, to the
    usual absolute floor).  Workspaces are poisoned: a read of a row the compact path leaves unwritten cannot pass."""
    outs, launched = [], []
    for off in (1, 0):
        _lib.set_option("NO_COMPACT_ROWS", off)
        ops.POISON_WORKSPACES = True
        _lib.prof_enable(1)
        try:
            _lib.prof_collect()
            cfg, sd, m, (hist, mask, cand, label) = _nrms_case("bf16", 90)
            m.train(train)
            torch.manual_seed(778)
            loss, score = m(hist.cuda(), mask.cuda(), cand.cuda(), label.cuda())
            loss.backward()
            torch.cuda.synchronize()
            launched.append(_launched())
        finally:
            _lib.prof_enable(0)
            ops.POISON_WORKSPACES = False
            _lib.set_option("NO_COMPACT_ROWS", 0)
        outs.append((loss.detach().clone(), score.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    assert _has(launched[0], "attn_mfma_bwd_live") and _has(launched[0], "rows_materialize_needed") and not _has(launched[0], "gemm_tn3_rows")
    assert _has(launched[1], "attn_mfma_bwd_rows") and _has(launched[1], "rows_materialize_live") and _has(launched[1], "gemm_tn3_rows")
    (l0, s0, g0), (l1, s1, g1) = outs
    assert torch.equal(s0, s1) and torch.equal(l0, l1)            # forward: bit-identical
    assert g0.keys() == g1.keys()
    for k in g0:
        assert torch.isfinite(g1[k]).all(), k
        err, ref = float((g0[k] - g1[k]).abs().max()), float(g0[k].abs().max())
        if k.startswith("news_encoder.multi_head_self_attn") and k.endswith("bias"):
            assert err <= 2e-3 * ref + 3e-4, (k, err, ref)
        else:
            assert err <= 2e-5 * ref + 1e-8, (k, err, ref)


def test_flat_bucket_over_rccl_single_rank():
    """parallel.FlatBucket on the 'nccl' (= RCCL) backend with one rank: broadcast, the flat all-reduce and the fused Adam run
    against the package's autograd Functions writing straight into the bucket; with a single rank the step must equal the
    plain one (same seeds -> same dropout draws)."""
    import os
    import torch.distributed as dist
    from newsrecommendation_amd import parallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29700 + os.getpid() % 200), RANK="0", WORLD_SIZE="1")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        res = []
        for _ in range(2):
            cfg, sd, m, (hist, mask, cand, label) = _nrms_case("bf16", 70)
            m.train()
            fb = parallel.FlatBucket(m, lr=1e-3)
            assert fb.world == 1 or dist.get_world_size() == 1
            torch.manual_seed(5)
            loss, _ = m(hist.cuda(), mask.cuda(), cand.cuda(), label.cuda())
            loss.backward()
            g = fb.grad.clone()
            fb.allreduce()                                     # RCCL all_reduce over the flat buffer (a copy with one rank)
            assert torch.equal(g, fb.grad)
            fb.adam_step()
            res.append((float(loss), fb.param.clone()))
        assert res[0][0] == res[1][0]
        # two identical runs: parameters agree up to the order of the fp32 atomics in the gradients (Adam's first step is
        # +-lr * sign-like, so compare where the gradient is not noise)
        diff = (res[0][1] - res[1][1]).abs()
        assert float((diff > 1.5e-3).float().mean()) < 1e-3
    finally:
        dist.destroy_process_group()


def test_phased_backward_with_early_table_gradient_hook_equals_the_single_call():
    """Data-parallel overlap: with a `_nr_grad_ready` hook on the word table (parallel.FlatBucket sets it when world > 1) the
    MHSA backward runs in two library calls -- table gradient first, hook, then the weight gradients (nr_mhsa_desc.bwd_phase).
    The gradients must be those of the single call, and the hook must fire exactly once per backward, after the table
    gradient kernel was enqueued (so what it sees at that point in the stream is the complete table gradient)."""
    from newsrecommendation_amd import parallel
    grads, seen = [], []
    for hooked in (False, True):
        cfg, sd, m, (hist, mask, cand, label) = _nrms_case("bf16", 71)
        m.train()
        fb = parallel.FlatBucket(m, lr=1e-3)
        table = m.news_encoder.embedding_matrix.weight
        if hooked:
            table._nr_grad_ready = lambda: seen.append(table._nr_grad.clone())     # stream-ordered snapshot at hook time
        torch.manual_seed(7)
        loss, _ = m(hist.cuda(), mask.cuda(), cand.cuda(), label.cuda())
        loss.backward()
        torch.cuda.synchronize()
        grads.append(fb.grad.clone())
    assert len(seen) == 1
    scale = grads[0].abs().max().item()
    assert (grads[0] - grads[1]).abs().max().item() <= 1e-4 * scale           # order of the fp32 atomics only
    tg = m.news_encoder.embedding_matrix.weight._nr_grad
    assert (seen[0] - tg).abs().max().item() == 0.0                            # nothing touched the table gradient after the hook


@pytest.mark.parametrize("model_name", ["NRMS", "NAML"])
def test_deterministic_mode_gives_bit_identical_gradients(model_name):
    """ops.set_deterministic(True): every gradient several workgroups add into (dW, db, the word-table gradient, pad_doc) is
    accumulated in 2^-36 fixed point with integer atomics -- two runs of the same training step (dropout on) must agree
    BIT FOR BIT at the production-scale shapes, and with the default fp32-atomic run up to the order of its additions."""
    def run():
        if model_name == "NRMS":
            cfg, sd, m, batch = _nrms_case("bf16", 80)
        else:
            from newsrecommendation_amd.model import NAML
            cfg = O.default_cfg(use_category=True, use_subcategory=True, freeze_embedding=True)
            g = torch.Generator().manual_seed(81)
            table = torch.randn(2501, cfg.num_words_title * cfg.word_embedding_dim, generator=g) * 0.4
            table[0] = 0
            sd = O.init_state_dict("NAML", cfg, table, seed=82, n_cat=17, n_sub=264)
            m = NAML.Model(SimpleNamespace(**vars(cfg), compute_dtype="bf16"), table.numpy(), 17, 264)
            m.load_state_dict(sd, strict=True)
            m = m.cuda()
            batch = bench.synth_batches_naml(cfg, B, 2500, 1, 83, "cpu")[0]
        m.train()
        torch.manual_seed(2024)
        loss, score = m(*(x.cuda() for x in batch))
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    plain_loss, plain = run()
    ops.set_deterministic(True)
    try:
        l1, g1 = run()
        l2, g2 = run()
    finally:
        ops.set_deterministic(False)
    assert torch.equal(l1, l2) and torch.equal(l1, plain_loss)
    assert g1.keys() == g2.keys() == plain.keys() and len(g1) >= 10
    for k in g1:
        assert torch.equal(g1[k], g2[k]), f"{k}: not bit-reproducible (max diff {float((g1[k] - g2[k]).abs().max()):.3e})"
        if k.startswith("news_encoder.multi_head_self_attn") and k.endswith("bias"):
            # the default run takes db_qkv from the attention backward (compact row storage), the deterministic one from the
            # weight-gradient GEMM over per-token rows: two summations of the same bf16-rounded factors
            assert float((g1[k] - plain[k]).abs().max()) <= 2e-3 * float(plain[k].abs().max()) + 3e-4, k
            continue
        # (the default run also takes the fused pooling backward -- dA on the matrix cores from bf16 hi + lo factors, dpre and dX
        #  from one kernel -- where this mode runs the two-kernel path: a bf16 rounding of dpre / dX flips here and there;
        #  att_fc1.bias is a column sum of dpre that cancels to ~1e-6: a handful of flipped bf16 roundings of |dpre| ~ 1e-5
        #  elements IS its noise floor, so it is held to the scale of its weight's gradient instead of its own)
        scale = float(plain[k].abs().max())
        if k.endswith("att_fc1.bias"):
            scale = max(scale, float(plain[k[:-4] + "weight"].abs().max()))
        assert float((g1[k] - plain[k]).abs().max()) <= (5e-3 if k.endswith("att_fc1.bias") else 1e-3) * scale + 1e-8, k
