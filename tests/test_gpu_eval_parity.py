"""GPU: the bf16 evaluation job (src/main.py:145-277 with src/demo.sh:26's masked user encoder) against the fp64 oracle at MIND
dims, and the gathering attention kernel it rests on against fp64 directly.

The eval path is made of parts that no training-side oracle test reaches: the once-projected word table and the attention
kernel that gathers projected rows (`attn_mfma_fwd_gather`, at L = 30 over titles, L = 50 over histories and L = 32 for the
short-history split of train.score_shard), the one-run shortcut of that kernel, the split itself and the device scorer /
ranking metrics.  Here they run through the real entry point, `train.test`, on a synthetic set written through the
package's own sharder, and every number that leaves it is checked against the oracle.

fp64 oracle: the state dict and inputs are cast to float64; the bf16 path is compared with an oracle whose table and weight
matrices were rounded through bf16 first (biases stay fp32, as the kernels read them), so the bounds measure the kernels,
not the input quantisation."""
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import MASKS, masks as _masks, metric_row_as_device
from oracle import nr_oracle as O
from newsrecommendation_amd import _lib, data as D, ops, train as TR

pytestmark = pytest.mark.gpu

T, H, WD, V, N_NEWS, N_IMP = 30, 50, 300, 5000, 3000, 1500
FORCED_HIST = (0, 1, 17, 18, 19, 31, 32, 33, 49, 50, 51, 60)


def _rounded64(sd):
    """fp64 copy of a state dict with every matrix (tables, weights, pad_doc) rounded through bf16 first."""
    return {k: (v.to(torch.bfloat16) if v.dim() >= 2 else v).double() for k, v in sd.items()}


def _test_set(tmp, seed=31):
    """N_NEWS news (titles of 0..30 tokens over a V-word table with a zero row 0), N_IMP test impressions written through the
    sharder.  Histories of 0..60 clicks incl. every length of FORCED_HIST (> 50 are truncated; 18 / 19 sit at the split edge
    H - 32 = 18, 32 / 33 at the 32-row kernel's edge); clicked and candidate ids unknown to news_index (-> index 0, mask 1);
    impressions with a single candidate, all positive, all negative, duplicate candidates, up to 60 candidates."""
    rnd = random.Random(seed)
    news_ids = [f"N{i}" for i in range(1, N_NEWS + 1)]
    news_index = {nid: i + 1 for i, nid in enumerate(news_ids)}
    g = torch.Generator().manual_seed(seed)
    comb = torch.randint(1, V, (N_NEWS + 1, T), generator=g, dtype=torch.int32)
    comb[0] = 0
    for r in range(1, N_NEWS + 1):
        comb[r, rnd.randint(0 if r % 97 == 0 else 3, T):] = 0
    table = torch.randn(V, WD, generator=g) * 0.4
    table[0] = 0

    def nid():
        return rnd.choice(news_ids) if rnd.random() > 0.05 else f"X{rnd.randint(0, 10 ** 6)}"

    lines = []
    for i in range(N_IMP):
        hl = FORCED_HIST[i] if i < len(FORCED_HIST) else rnd.randint(0, 60)
        hist = " ".join(nid() for _ in range(hl))
        kind = i % 10
        nc = 1 if kind == 1 else (rnd.randint(40, 60) if kind == 2 else rnd.randint(2, 14))
        cands = [nid() for _ in range(nc)]
        if kind == 5:
            cands += cands[: max(1, nc // 2)]                                         # duplicate candidates
        labs = [1 if rnd.random() < 0.2 else 0 for _ in cands]
        if kind == 3:
            labs = [1] * len(cands)
        elif kind == 4:
            labs = [0] * len(cands)
        elif kind not in (1,) and sum(labs) == 0:
            labs[rnd.randrange(len(labs))] = 1
        lines.append("\t".join([str(i + 1), "U1", "t", hist, " ".join(f"{c}-{l}" for c, l in zip(cands, labs))]) + "\n")
    os.makedirs(os.path.join(tmp, "test"), exist_ok=True)
    with open(os.path.join(tmp, "test", "behaviors.tsv"), "w") as f:
        f.writelines(lines)
    D.prepare_testing_data(os.path.join(tmp, "test"), 1)
    return news_index, comb, table


def _args(tmp, model, **kw):
    cfg = O.default_cfg(**kw)
    return SimpleNamespace(**vars(cfg), model=model, compute_dtype="bf16", batch_size=128, test_data_dir=os.path.join(tmp, "test"))


def _check_against_oracle(args, got, means, nv_o, sd_o, user_fn, news_index):
    """Per-impression scores vs the fp64 oracle (oracle news vectors -> user encoder -> dot), empty histories, the device
    metric means vs the oracle's metric functions on the device scores, mean AUC of device vs oracle scores."""
    lines = open(os.path.join(args.test_data_dir, "behaviors_0.tsv")).readlines()
    assert len(lines) == len(got) == N_IMP
    parsed = [O.test_line_to_indices(l, news_index, args.user_log_length) for l in lines]
    hist = torch.as_tensor(np.stack([p[0] for p in parsed]), dtype=torch.long)
    mask = torch.from_numpy(np.stack([p[1] for p in parsed])).double()
    uv = user_fn(nv_o[hist], mask, sd_o, args)                                        # [N_IMP, news_dim] fp64
    if args.user_log_mask:
        assert float(uv[mask.sum(1) == 0].abs().max()) == 0.0                         # the oracle's empty user: exactly 0
    worst, sums, cnt, tie_free, auc_d, auc_o = 0.0, np.zeros(4), 0, 0, [], []
    n_unknown = 0
    for (h, m, cand, labels), (lab_g, s_g), u, empty in zip(parsed, got, uv, (mask.sum(1) == 0).tolist()):
        assert np.array_equal(labels, lab_g)
        s_o = (nv_o[cand] @ u).numpy()
        worst = max(worst, float(np.abs(s_g - s_o).max()))
        n_unknown += int((np.asarray(cand) == 0).sum())
        if args.user_log_mask and empty:
            assert np.all(s_g == 0.0), s_g                                            # a zero user vector scores exactly 0
        if labels.mean() in (0, 1):
            continue
        row, tf = metric_row_as_device(labels, s_g)
        tie_free += tf
        sums += row
        cnt += 1
        auc_d.append(row[0])
        auc_o.append(O.auc_score(labels, s_o))
    assert n_unknown > 0 and cnt > 500 and tie_free > 300
    assert np.allclose(means, sums / cnt, atol=1e-9), (means, sums / cnt)
    return worst, abs(float(np.mean(auc_d)) - float(np.mean(auc_o)))


@pytest.mark.parametrize("user_log_mask", [True, False])
def test_nrms_bf16_eval_job_against_the_fp64_oracle(tmp_path, user_log_mask):
    """NRMS, bf16, oracle-initialised weights, through train.test.  user_log_mask=True is src/demo.sh:26 (projected history
    table + gathering attention at L = 50 and, for the short histories, L = 32); False is the pad_doc path.

    Measured on MI355X, bound in brackets (about 3x the measurement; the bf16 score bound 3e-2 at most):
      user_log_mask=True:  news vectors 1.9e-3 * max|v| [6e-3]; scores 8.2e-4 abs [2.5e-3]; mean-AUC gap 7.1e-4 [5e-3]
      user_log_mask=False: news vectors 1.9e-3 * max|v| [6e-3]; scores 7.5e-3 abs [2.5e-2]; mean-AUC gap 1.3e-3 [5e-3]
    ~5 s of oracle per case."""
    news_index, comb, table = _test_set(str(tmp_path))
    args = _args(str(tmp_path), "NRMS", user_log_mask=user_log_mask)
    sd = O.init_state_dict("NRMS", args, table, seed=32)
    from newsrecommendation_amd.model import NRMS
    m = NRMS.Model(args, table.numpy())
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    sd_o = _rounded64(sd)
    dev = torch.device("cuda", torch.cuda.current_device())

    shard = D.IndexedTestShard(os.path.join(args.test_data_dir, "behaviors_0.tsv"), news_index, args)
    groups, _ = TR._short_history_split(shard, H)
    assert len(groups[0][0]) > 0 and len(groups[1][0]) > 0 and groups[0][1] == H - 32

    _lib.prof_enable(1)
    try:
        _lib.prof_collect()
        nv = TR.encode_news(m, comb.numpy(), args.batch_size, dev)
        got = []
        n_seen, means = TR.test(None, args, m, news_index, comb.numpy(), log=lambda *_: None, collect_scores=got)
        torch.cuda.synchronize()
        labels = set(_lib.prof_collect().keys())
    finally:
        _lib.prof_enable(0)
    assert n_seen == N_IMP
    gathers = [l for l in labels if l.startswith("attn_mfma_fwd_gather[")]
    for L in ((30, 50, 32) if user_log_mask else (30,)):
        assert any(f",L={L}," in l for l in gathers), (L, sorted(labels))

    nv_o = O.nrms_news_encoder(torch.from_numpy(comb.numpy()).long(), sd_o, args)     # [N_NEWS + 1, news_dim] fp64
    assert nv.shape == nv_o.shape
    news_err = float((nv.double().cpu() - nv_o).abs().max()) / float(nv_o.abs().max())
    worst, auc_gap = _check_against_oracle(args, got, means, nv_o, sd_o, O.nrms_user_encoder, news_index)
    print(f"NRMS eval ulm={user_log_mask}: news err {news_err:.2e} * max|v|; worst score err {worst:.2e}; mean AUC gap {auc_gap:.2e}")
    assert news_err <= 6e-3
    assert worst <= (2.5e-3 if user_log_mask else 2.5e-2)
    assert auc_gap <= 5e-3


def test_naml_bf16_eval_job_against_the_fp64_oracle(tmp_path):
    """NAML as src/demo.sh runs it: frozen title table (TitleTable), category + subcategory views, masked user encoder, bf16,
    through train.test against O.naml_news_encoder / O.naml_user_encoder in fp64.

    Measured on MI355X, bound in brackets: news vectors 3.4e-3 * max|v| [1e-2]; scores 1.9e-2 abs [3e-2, the bf16 score
    bound]; mean-AUC gap 1.4e-3 [5e-3].  ~5 s of oracle."""
    news_index, comb, words = _test_set(str(tmp_path))
    args = _args(str(tmp_path), "NAML", user_log_mask=True, freeze_embedding=True, use_category=True, use_subcategory=True)
    g = torch.Generator().manual_seed(33)
    n_cat, n_sub = 17, 264
    feats = torch.zeros(N_NEWS + 1, 3, dtype=torch.int32)                  # [title row, category, subcategory]; row 0 unknown
    feats[1:, 0] = torch.arange(1, N_NEWS + 1, dtype=torch.int32)
    feats[1:, 1] = torch.randint(0, n_cat + 1, (N_NEWS,), generator=g, dtype=torch.int32)
    feats[1:, 2] = torch.randint(0, n_sub + 1, (N_NEWS,), generator=g, dtype=torch.int32)
    titles = words[comb.long()].reshape(N_NEWS + 1, T * WD)                # per-news title-embedding rows, row 0 zero
    sd = O.init_state_dict("NAML", args, titles, seed=34, n_cat=n_cat, n_sub=n_sub)
    from newsrecommendation_amd.model import NAML
    m = NAML.Model(args, titles.numpy(), n_cat, n_sub)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    sd_o = _rounded64(sd)
    dev = torch.device("cuda", torch.cuda.current_device())
    nv = TR.encode_news(m, feats.numpy(), args.batch_size, dev)
    got = []
    n_seen, means = TR.test(None, args, m, news_index, feats.numpy(), log=lambda *_: None, collect_scores=got)
    assert n_seen == N_IMP
    nv_o = O.naml_news_encoder(feats.long(), sd_o, args)
    news_err = float((nv.double().cpu() - nv_o).abs().max()) / float(nv_o.abs().max())
    worst, auc_gap = _check_against_oracle(args, got, means, nv_o, sd_o, O.naml_user_encoder, news_index)
    print(f"NAML eval: news err {news_err:.2e} * max|v|; worst score err {worst:.2e}; mean AUC gap {auc_gap:.2e}")
    assert news_err <= 1e-2
    assert worst <= 3e-2
    assert auc_gap <= 5e-3


# ---------------------------------------------------------------------------------------------------- the gathering kernel
def _one_run(mask):
    """[n] bool: the unmasked positions of the sequence form one non-empty run."""
    d = torch.diff(torch.nn.functional.pad(mask, (1, 1)), dim=1)
    return (d > 0).sum(1) == 1


@pytest.mark.parametrize("heads,d_head,d_model", [(20, 20, 300), (20, 20, 400), (8, 16, 128)])
@pytest.mark.parametrize("L", [1, 5, 30, 31, 32, 33, 50, 63, 64])
def test_gathering_attention_against_fp64(L, heads, d_head, d_model):
    """ops.mhsa(ids=, table=) under no_grad in bf16 -- the once-projected table + nr_launch_attn_gather_fwd -- against fp64
    O.mhsa on the gathered rows, for n = 1, 7 and 1 031 sequences, with no mask and with every mask pattern of MASKS (front-,
    back- and middle-run, holes, a single click, all masked), a table whose row 0 is NOT zero (the user level, where row 0 is
    the unknown news's vector).  Contract (include/nrhip.h, proj_table): y rows at masked query positions are unspecified --
    they are exact zeros when the unmasked keys form one run at 32 < L <= 64 (pinned here) -- and an all-masked sequence
    gives exact zeros.  On unmasked query rows: <= 1e-2 * max|y|; measured worst 8.0e-3 * max|y| over all 27 cases (the
    bf16 rounding of the projected table, of P and of y; 3.0e-3 at L = 1).  ~1 s of oracle per case."""
    g = torch.Generator().manual_seed(1000 * L + d_model)
    N, Vt = heads * d_head, 2000
    table = torch.randn(Vt, d_model, generator=g) * 0.5                     # row 0 non-zero
    a = (6.0 / (N + d_model)) ** 0.5
    ws = [(torch.rand(N, d_model, generator=g) * 2 - 1) * a for _ in range(3)]
    bs = [(torch.rand(N, generator=g) * 2 - 1) / d_model ** 0.5 for _ in range(3)]
    n = 1031
    ids = torch.randint(0, Vt, (n, L), generator=g, dtype=torch.int32)
    ids[torch.rand(n, L, generator=g) < 0.15] = 0
    mask, kind = _masks(n, L, g)
    params = [t.cuda() for t in (ws[0], bs[0], ws[1], bs[1], ws[2], bs[2])]
    tab = table.cuda()
    r64 = lambda t: t.to(torch.bfloat16).double()
    x64 = r64(table)[ids.long()]
    p64 = [r64(ws[0]), bs[0].double(), r64(ws[1]), bs[1].double(), r64(ws[2]), bs[2].double()]
    worst = 0.0
    for use_mask in (False, True):
        ref = O.mhsa(x64, *p64, n_heads=heads, mask=mask.double() if use_mask else None)
        scale = float(ref.abs().max())
        for nn_ in (1, 7, n):
            with torch.no_grad():
                y = ops.mhsa(None, *params, heads=heads, code=ops.NR_BF16, mask=mask[:nn_].cuda() if use_mask else None,
                             ids=ids[:nn_].cuda(), table=tab)
            torch.cuda.synchronize()
            y = y.double().cpu().reshape(nn_, L, N)
            assert torch.isfinite(y).all()
            valid = mask[:nn_].bool() if use_mask else torch.ones(nn_, L, dtype=torch.bool)
            err = float((y - ref[:nn_]).abs()[valid].max()) / scale if bool(valid.any()) else 0.0
            worst = max(worst, err)
            assert err <= 1e-2, (use_mask, nn_, err)
            if use_mask:
                dead = mask[:nn_].sum(1) == 0
                assert bool(dead.any()) or nn_ < 7
                assert float(y[dead].abs().max() if bool(dead.any()) else 0.0) == 0.0          # all masked: exact zeros
                if 32 < L <= 64:
                    sel = _one_run(mask[:nn_])[:, None] & ~valid
                    assert float(y[sel].abs().max() if bool(sel.any()) else 0.0) == 0.0      # one run: masked rows are zeros
    print(f"gather attention L={L} h={heads} d={d_head} D={d_model}: worst err {worst:.2e} * max|y|")

