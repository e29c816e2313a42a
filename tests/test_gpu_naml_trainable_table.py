"""GPU: NAML with a TRAINABLE title-embedding table (freeze_embedding=False, the reference's default: src/parameters.py:47,
src/model/NAML.py:104-107) -- the dense [V, T*D] gradient made by nr_conv1d_k3_bwd_table (dx GEMM over the live titles +
owner-computes scatter), through ops.ConvFunction, the flat bucket's Adam and train.train.

The models are built here (tests/helpers.build_model forces the table frozen).  Bounds are the existing ones: the golden
case at test_gpu_model_parity's (loss / score 1e-4, gradients 1e-6 + 2e-4 * max|g|), B = 128 at test_gpu_scale_parity.TOL
(fp32 2e-4 * max|g| + 1e-6; bf16 3e-2 * max|g| + 3e-4), the training loop at test_gpu_reference_settings' (fp32 2e-3, bf16 3e-2
on the loss trajectory)."""
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bench
from helpers import assert_close, batch_of, load_case
from newsrecommendation_amd import _lib, data as D, ops, train as TR
from oracle import nr_oracle as O

pytestmark = pytest.mark.gpu
TKEY = "news_encoder.title_embeddings.weight"
TOL = {"fp32": dict(tol=1e-4, gatol=1e-6, grtol=2e-4), "bf16": dict(tol=3e-2, gatol=3e-4, grtol=3e-2)}
NEW_KERNELS = ("conv_table_live", "conv_table_stage", "conv_table_rank", "conv_table_scatter")
B = 128


def _has(labels, prefix):
    return any(l.startswith(prefix) for l in labels)


def _naml(cfg, table, sd, dt, train, **extra):
    from newsrecommendation_amd.model import NAML
    args = SimpleNamespace(**{**vars(cfg), "compute_dtype": dt, **extra})
    n_cat = sd["news_encoder.category_emb.weight"].shape[0] - 1 if "news_encoder.category_emb.weight" in sd else 0
    n_sub = sd["news_encoder.subcategory_emb.weight"].shape[0] - 1 if "news_encoder.subcategory_emb.weight" in sd else 0
    m = NAML.Model(args, table.numpy() if torch.is_tensor(table) else table, n_cat, n_sub)
    m.load_state_dict(sd, strict=True)
    return m.cuda().train(train)


def test_reference_recorded_table_gradient():
    """naml_tiny_3view as the reference recorded it (freeze_embedding=False), fp32, eval mode: loss, score and every grad::* of
    the fixture -- grad::news_encoder.title_embeddings.weight [9, 32] included -- against the golden and against the oracle."""
    z, cfg, sd = load_case("naml_tiny_3view")
    assert cfg.freeze_embedding is False and "grad::" + TKEY in z.files
    m = _naml(cfg, sd[TKEY], sd, "fp32", False)
    tab = dict(m.named_parameters())[TKEY]
    assert tab.requires_grad
    hist, mask, cand, label = batch_of(z)
    ids = torch.cat([cand.reshape(-1, cand.shape[-1])[:, 0], hist.reshape(-1, hist.shape[-1])[:, 0]]).cpu()
    assert int((ids == 0).sum()) >= 1 and int(torch.bincount(ids.long())[1:].max()) >= 2      # id-0 slots and repeated news
    loss, score = m(hist, mask, cand, label)
    loss.backward()
    torch.cuda.synchronize()
    assert_close(loss, torch.from_numpy(z["loss"]), 1e-4, name="loss vs golden")
    assert_close(score, torch.from_numpy(z["score"]), 1e-4, name="score vs golden")
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    lo, so = O.naml_forward(*(torch.from_numpy(z[k]) for k in ("hist", "mask", "cand", "label")), sdo, cfg)
    lo.backward()
    assert_close(loss, lo.detach(), 1e-4, name="loss vs oracle")
    assert_close(score, so.detach(), 1e-4, name="score vs oracle")
    grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    assert TKEY in grads
    checked = 0
    for k in z.files:
        if k.startswith("grad::"):
            assert k[6:] in grads, k
            err = float((grads[k[6:]].cpu().double() - torch.from_numpy(z[k]).double()).abs().max())
            print(f"{k}: max|diff| {err:.3e} (max|g| {float(np.abs(z[k]).max()):.3e})")
            assert_close(grads[k[6:]], torch.from_numpy(z[k]), 1e-6, 2e-4, name=k + " vs golden")
            checked += 1
    assert checked >= 9
    for name, g in grads.items():
        if sdo[name].grad is not None:
            assert_close(g, sdo[name].grad, 1e-6, 2e-4, name="d" + name + " vs oracle")
    assert float(tab.grad[0].abs().max()) == 0.0                                      # padding_idx row


def _b128_case(dt, train, freeze=False, **extra):
    cfg = O.default_cfg(use_category=True, use_subcategory=True, freeze_embedding=freeze)
    g = torch.Generator().manual_seed(50)
    n_news = 2500
    T, D_ = cfg.num_words_title, cfg.word_embedding_dim
    table = torch.randn(n_news + 1, T * D_, generator=g) * 0.4
    table[0] = 0
    sd = O.init_state_dict("NAML", cfg, table, seed=51, n_cat=17, n_sub=264)
    m = _naml(cfg, table, sd, dt, train, **extra)
    batch = bench.synth_batches_naml(cfg, B, n_news, 1, 52, "cpu")[0]
    return cfg, sd, m, batch


def _step(m, batch, seed=99, poison=True):
    hist, mask, cand, label = batch
    ops.POISON_WORKSPACES = poison
    _lib.prof_enable(1)
    try:
        _lib.prof_collect()
        torch.manual_seed(seed)
        seed_in = ops.draw_seed()
        torch.manual_seed(seed)
        loss, score = m(hist.cuda(), mask.cuda(), cand.cuda(), label.cuda())
        loss.backward()
        torch.cuda.synchronize()
        labels = set(_lib.prof_collect().keys())
    finally:
        _lib.prof_enable(0)
        ops.POISON_WORKSPACES = False
    return loss.detach(), score.detach(), labels, seed_in


@pytest.mark.parametrize("dt,train", [("bf16", True), ("fp32", False)])
def test_naml_b128_trainable_table_every_gradient_against_the_oracle(dt, train):
    """The set-up of test_gpu_scale_parity.test_naml_b128_every_gradient_against_the_oracle (B = 128, 2 500 news, 3 views,
    poisoned workspaces) with a trainable table: loss, score and EVERY gradient, the full [2501, 9000] table gradient included,
    at that file's bounds.  The launch log shows the new kernels; the batch repeats news ids, has id-0 and masked slots; rows
    of news that do not occur in the batch are exactly zero.
    The table gradient is small here (max|g| 2e-4, below the bf16 bound's 3e-4 absolute floor, which exists for d W_K.bias of
    NRMS), so it is ALSO held to the relative part alone, no floor: 3e-2 * max|g| in bf16 (three bf16 roundings -- dy, W, dx --
    of 2^-9 each on sums of <= 1200 products; the same factor the other bf16 gradients get), 2e-4 * max|g| in fp32.
    Measured on MI355X: bf16 1.4e-6 (0.7 % of max|g| 1.98e-4), fp32 2.4e-10 (1.4e-6 of max|g| 1.71e-4)."""
    cfg, sd, m, batch = _b128_case(dt, train)
    hist, mask, cand, label = batch
    T, D_, p = cfg.num_words_title, cfg.word_embedding_dim, cfg.drop_rate
    ids = torch.cat([cand.reshape(-1, 3)[:, 0], hist.reshape(-1, 3)[:, 0]]).long()
    occ = torch.bincount(ids, minlength=2501)
    assert ids.numel() == B * 55 and int(occ[1:].max()) >= 2 and int(occ[0]) > B and int((mask == 0).sum()) > B
    assert bool((hist[mask == 0] == 0).all())
    t = TOL[dt]
    loss, score, labels, seed_in = _step(m, batch)
    for k in NEW_KERNELS:
        assert _has(labels, k), (k, sorted(labels))
    if dt == "bf16":
        assert _has(labels, "gemm_nt_dma_live[bf16,epi=0,") and _has(labels, "sort_rows_by_id"), sorted(labels)
    keep = None
    if train:
        n = B * 55
        word = ops.dropout_mask(n * T * D_, p, seed_in, "cuda").cpu().reshape(n, T, D_)
        keep = {"cand_word": word[: B * 5], "hist_word": word[B * 5:]}
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    lo, so = O.naml_forward(hist, mask, cand, label, sdo, cfg, keep=keep)
    lo.backward()
    assert torch.isfinite(score).all() and torch.isfinite(loss)
    assert_close(loss, lo.detach(), t["tol"], name="loss")
    assert_close(score, so.detach(), t["tol"], name="score")
    worst = {}
    for name, prm in m.named_parameters():
        ref = sdo[name].grad
        if ref is None:
            continue
        assert prm.grad is not None, name
        assert torch.isfinite(prm.grad).all(), f"non-finite gradient in {name}"
        err = float((prm.grad.detach().double().cpu() - ref.double()).abs().max())
        worst[name] = (err, float(ref.abs().max()))
    print(f"naml trainable B={B} {dt} train={train}: " + "; ".join(f"{k.split('.', 1)[1]} err {e:.2e} max|g| {g:.2e}" for k, (e, g) in worst.items()))
    assert TKEY in worst
    for name, prm in m.named_parameters():
        if name in worst:
            assert_close(prm.grad, sdo[name].grad, t["gatol"], t["grtol"], name="d" + name)
    assert_close(dict(m.named_parameters())[TKEY].grad, sdo[TKEY].grad, 0.0, t["grtol"], name="dtable, relative bound alone")
    tg = dict(m.named_parameters())[TKEY].grad.cpu()
    untouched = torch.ones(2501, dtype=torch.bool)
    live = torch.cat([cand.reshape(-1, 3)[:, 0], hist[mask != 0].reshape(-1, 3)[:, 0]]).long()
    untouched[live] = False
    untouched[0] = True
    assert int(untouched.sum()) > 10
    assert float(tg[untouched].abs().max()) == 0.0


@pytest.mark.parametrize("stream", [True, False])
def test_frozen_stays_frozen(stream):
    """freeze_embedding=True (TitleTable, and nn.Embedding with freeze=True): none of the new kernels in a B = 128 step, and loss /
    scores equal the trainable run's bit for bit (same seeds): the forward is the same launch sequence."""
    _, _, m_t, batch = _b128_case("bf16", True)
    l_t, s_t, labels_t, _ = _step(m_t, batch)
    assert _has(labels_t, "conv_table_scatter")
    _, _, m_f, _ = _b128_case("bf16", True, freeze=True, stream_title_table=stream)
    l_f, s_f, labels_f, _ = _step(m_f, batch)
    for k in NEW_KERNELS + ("sort_rows_by_id", "gemm_nt_dma_live[bf16,epi=0,"):
        assert not _has(labels_f, k), (k, sorted(labels_f))
    assert torch.equal(l_t, l_f) and torch.equal(s_t, s_f)
    tab = m_f.news_encoder.title_embeddings
    if not stream:
        assert not tab.weight.requires_grad and tab.weight.grad is None


def test_deterministic_mode_is_bit_reproducible():
    """Two B = 128 backward passes under ops.set_deterministic: torch.equal on the table gradient and on every other one.  The
    table gradient itself needs no fixed-point scratch (the scatter sums in a fixed order), so the scratch is sized for the
    other parameters only."""
    _, _, m, batch = _b128_case("bf16", True)
    small = sum(p.numel() for n, p in m.named_parameters() if n != TKEY)
    ops.set_deterministic(True, elements=small + (1 << 20))
    try:
        runs = []
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            _step(m, batch)
            runs.append({n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    finally:
        ops.set_deterministic(False)
    assert TKEY in runs[0] and float(runs[0][TKEY].abs().max()) > 0
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_large_table_offsets_beyond_4gib():
    """Op level: the same batch once with news ids in [1, 64] on a small table and once with those ids mapped to the top 64 rows
    of a table whose fp32 gradient is 4.7 GB (V = 131 072, T*D = 9 000; created on the device): the 64 touched gradient rows are
    bit-identical between the two, everything below them is exactly zero."""
    T, D_, N, n = 30, 300, 400, 512
    code = ops.dtype_code("bf16")
    g = torch.Generator().manual_seed(7)
    w = (torch.randn(N, D_, 3, generator=g) * 0.05).cuda().requires_grad_(True)
    b = (torch.randn(N, generator=g) * 0.05).cuda().requires_grad_(True)
    ids_small = torch.randint(0, 65, (n,), generator=g, dtype=torch.int32)
    assert int((ids_small == 0).sum()) >= 1
    rows = (torch.randn(65, T * D_, generator=g) * 0.4)
    rows[0] = 0
    dy = torch.randn(n, T, N, generator=g).cuda()

    def run(V, ids):
        table = torch.zeros(V, T * D_, dtype=torch.float32, device="cuda")
        table[V - 64:] = rows[1:].cuda()
        table.requires_grad_(True)
        torch.manual_seed(5)
        y = ops.conv1d_k3_gather(table, w, b, ids.cuda(), T, D_, code, p_in=0.2)
        y.backward(dy.to(y.dtype))
        torch.cuda.synchronize()
        gr = table.grad
        assert gr.shape == (V, T * D_)
        top = gr[V - 64:].clone()
        below = float(gr[: V - 64].abs().max())
        del table, gr, y
        ops.table_cache.invalidate()
        torch.cuda.empty_cache()
        return top, below

    V_small, V_big = 65, 131072
    assert V_big * T * D_ * 4 > 2 ** 32
    ops.set_deterministic(True, elements=3 * N * 320 + N + (1 << 20))
    try:
        top_s, below_s = run(V_small, ids_small)
        ids_big = torch.where(ids_small > 0, ids_small + (V_big - 65), ids_small)
        top_b, below_b = run(V_big, ids_big)
    finally:
        ops.set_deterministic(False)
    assert float(top_s.abs().max()) > 0
    assert below_s == 0.0 and below_b == 0.0
    assert torch.equal(top_s, top_b)


# ---------------------------------------------------------------------------------------------------------- training loop
T_, H_, WD_, ND_, N_NEWS = 30, 50, 300, 400, 600


def _naml_set(tmp, seed=23, n_imp=320):
    rnd = random.Random(seed)
    news_ids = [f"N{i}" for i in range(1, N_NEWS + 1)]
    news_index = {nid: i + 1 for i, nid in enumerate(news_ids)}
    g = torch.Generator().manual_seed(seed)
    comb = torch.stack([torch.arange(N_NEWS + 1, dtype=torch.int32), torch.randint(1, 18, (N_NEWS + 1,), generator=g, dtype=torch.int32),
                        torch.randint(1, 265, (N_NEWS + 1,), generator=g, dtype=torch.int32)], dim=1)
    comb[0] = 0
    table = torch.randn(N_NEWS + 1, T_ * WD_, generator=g) * 0.4
    table[0] = 0
    lines = []
    for i in range(n_imp):
        hist = " ".join(rnd.choice(news_ids) if rnd.random() > 0.1 else "X%d" % i for _ in range(rnd.randint(0, 60)))
        imps = [f"{rnd.choice(news_ids)}-{1 if (j == 0 or rnd.random() < 0.2) else 0}" for j in range(rnd.randint(2, 12))]
        lines.append("\t".join([str(i + 1), "U1", "t", hist, " ".join(imps)]) + "\n")
    os.makedirs(os.path.join(tmp, "train"), exist_ok=True)
    with open(os.path.join(tmp, "train", "behaviors.tsv"), "w") as f:
        f.writelines(lines)
    args = SimpleNamespace(model="NAML", num_words_title=T_, user_log_length=H_, npratio=4, word_embedding_dim=WD_, news_dim=ND_,
                           num_attention_heads=20, news_query_vector_dim=200, user_query_vector_dim=200, drop_rate=0.0,
                           user_log_mask=False, freeze_embedding=False, use_category=True, use_subcategory=True,
                           category_emb_dim=100, lr=3e-4, batch_size=32, epochs=1, log_steps=1000,
                           train_data_dir=os.path.join(tmp, "train"), model_dir=None)
    cats = {f"c{i}": i for i in range(1, 18)}
    subs = {f"s{i}": i for i in range(1, 265)}
    return args, news_index, comb.numpy(), table.numpy(), cats, subs


@pytest.mark.parametrize("dt,mode,feed", [("fp32", "flat", "device"), ("bf16", "flat", "device"), ("fp32", "ddp", "host"), ("bf16", "ddp", "host")])
def test_training_loop_with_a_trainable_table_tracks_the_oracle(tmp_path, dt, mode, feed):
    """train.train on NAML at the reference's dims (batch 32, 3 views, lr 3e-4, dropout 0) with freeze_embedding=False, 8 steps
    against the oracle + torch.optim.Adam (dense Adam over the table: the reference's semantics).  Afterwards: touched rows of
    the table moved, row 0 did not, the packed bf16 copy that ops.table_cache serves equals a fresh pack of the fp32 master, the
    state_dict holds the updated table, and train.encode_news (under no_grad) matches the oracle on the updated table."""
    args, news_index, comb, table, cats, subs = _naml_set(str(tmp_path))
    args.compute_dtype, args.dp_mode, args.feed = dt, mode, feed
    assert D.prepare_training_data(args.train_data_dir, 1, args.npratio, seed=0) >= 8 * args.batch_size
    steps = 8
    torch.manual_seed(0)
    random.seed(0)
    model, losses = TR.train(None, args, news_index, comb, table, cats, subs, max_steps=steps, log=lambda *_: None)
    assert len(losses) == steps and torch.isfinite(losses).all()
    # the oracle from the same initial parameters, on the same batches
    torch.manual_seed(0)
    init = TR.build_model(args, table, len(cats), len(subs)).state_dict()
    params = {k: v.detach().clone().float().requires_grad_(True) for k, v in init.items()}
    opt = torch.optim.Adam(list(params.values()), lr=args.lr)
    random.seed(0)
    ds = D.DatasetTrain(os.path.join(args.train_data_dir, f"behaviors_np{args.npratio}_0.tsv"), news_index, comb, args)
    ref, touched = [], torch.zeros(N_NEWS + 1, dtype=torch.bool)
    for cnt, (h, mk, c, l) in enumerate(torch.utils.data.DataLoader(ds, batch_size=args.batch_size)):
        if cnt == steps:
            break
        loss, _ = O.naml_forward(h, mk, c, l, params, args)
        opt.zero_grad()
        loss.backward()
        opt.step()
        ref.append(float(loss.detach()))
        touched[c.reshape(-1, 3)[:, 0].long()] = True
    touched[0] = False
    worst = max(abs(float(a) - b_) for a, b_ in zip(losses, ref))
    print(f"naml trainable loop {dt} {mode}/{feed}: worst |loss - oracle| over {steps} steps = {worst:.2e}")
    assert worst < (2e-3 if dt == "fp32" else 3e-2), (losses.tolist(), ref)
    tab = model.news_encoder.title_embeddings.weight
    assert tab.requires_grad
    now, was = tab.detach().cpu(), torch.from_numpy(table)
    assert torch.equal(now[0], was[0])                                        # padding_idx row: no gradient, zero moments
    moved = (now != was).any(dim=1)
    assert bool(moved[touched].all()) and int(touched.sum()) > 50
    assert torch.equal(model.state_dict()[TKEY].cpu(), now)
    ck = TR.checkpoint_dict(model, cats, subs)["model_state_dict"][TKEY]
    assert torch.equal(ck, now)
    code = ops.dtype_code(dt)
    if dt == "bf16":
        served = ops.table_cache.get(tab, code, row_cols=WD_)
        fresh = ops.pack(tab.detach().reshape(-1, WD_).clone(), code)
        assert torch.equal(served, fresh)
    # eval-time encode of the whole corpus with the trained (still requires_grad) table
    model.eval()
    with torch.no_grad():
        nv = TR.encode_news(model, comb, 512, torch.device("cuda"))
    sd_o = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    nv_o = O.naml_news_encoder(torch.from_numpy(comb).long(), sd_o, args)
    err = float((nv.cpu().double() - nv_o).abs().max()) / float(nv_o.abs().max())
    print(f"encode_news vs oracle on the updated table: {err:.2e} * max|v|")
    assert err < (1e-4 if dt == "fp32" else 3e-2)
