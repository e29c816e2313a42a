"""GPU: the reference's own run settings (src/demo.sh) against the oracle -- a frozen word table (freeze_embedding=True, :12) at
MIND-sized batches, and the masked user encoder (user_log_mask=True) in training.

The fast paths of libnrhip are chosen by shape and flag.  With a frozen table the news-level MHSA backward still keeps its
rows for the weight gradient, so a bf16 batch of >= 4096 token rows takes compact row storage without a table gradient
(nr_mhsa_bwd with dtable == NULL): no id sort, no scatter-epilogue GEMM, the attention backward and dW as usual.  The golden
cases and the earlier frozen tests never reach that branch (they are too small).

Tolerances are the B = 128 oracle tests' own (test_gpu_scale_parity.TOL); the loop test keeps test_gpu_train_loop's 2e-3
fp32 trajectory bound and holds bf16 to 3e-2 per step (the bf16 score bound)."""
import json
import math
import os
import random
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import nr_oracle as O
from newsrecommendation_amd import data as D, train as TR
from test_gpu_scale_parity import _nrms_against_the_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dt,train,freeze,ulm", [("bf16", True, True, False), ("bf16", True, False, True),
                                                 ("bf16", True, True, True), ("fp32", False, True, False)])
def test_nrms_b128_reference_flags_every_gradient_against_the_oracle(dt, train, freeze, ulm):
    """B = 128 (M = 211 200 token rows), MIND-shaped batch, poisoned workspaces: loss, every score and every gradient against
    oracle.nrms_forward with freeze_embedding / user_log_mask as the reference's script sets them (dropout on and the kernels'
    masks exported to the oracle in the training cases).  A frozen table has no gradient at all, and the launch log shows
    compact row storage without its table-gradient half.  ~10 s of oracle per case."""
    _nrms_against_the_oracle(dt, train, 128, 5000, 40, freeze_embedding=freeze, user_log_mask=ulm)


T, H, WD, ND, V, N_NEWS = 30, 50, 300, 400, 5000, 1200


def _mind_set(tmp, seed=21, n_imp=320):
    """A synthetic MIND training set at the reference's dims, written through the package's own sharder: titles of 5..30
    tokens, histories of 0..60 clicks (front padded / truncated to 50), one in ten clicked ids unknown to news_index."""
    rnd = random.Random(seed)
    news_ids = [f"N{i}" for i in range(1, N_NEWS + 1)]
    news_index = {nid: i + 1 for i, nid in enumerate(news_ids)}
    g = torch.Generator().manual_seed(seed)
    comb = torch.randint(1, V, (N_NEWS + 1, T), generator=g, dtype=torch.int32)
    comb[0] = 0
    for r in range(1, N_NEWS + 1):
        comb[r, rnd.randint(5, T):] = 0
    table = torch.randn(V, WD, generator=g) * 0.4
    table[0] = 0
    lines = []
    for i in range(n_imp):
        hist = " ".join(rnd.choice(news_ids) if rnd.random() > 0.1 else "X%d" % i for _ in range(rnd.randint(0, 60)))
        imps = [f"{rnd.choice(news_ids)}-{1 if (j == 0 or rnd.random() < 0.2) else 0}" for j in range(rnd.randint(2, 12))]
        lines.append("\t".join([str(i + 1), "U1", "t", hist, " ".join(imps)]) + "\n")
    os.makedirs(os.path.join(tmp, "train"), exist_ok=True)
    with open(os.path.join(tmp, "train", "behaviors.tsv"), "w") as f:
        f.writelines(lines)
    # src/demo.sh:12-19: frozen table, batch 32, lr 3e-4; user_log_mask=False in training
    args = SimpleNamespace(model="NRMS", num_words_title=T, user_log_length=H, npratio=4, word_embedding_dim=WD, news_dim=ND,
                           num_attention_heads=20, news_query_vector_dim=200, user_query_vector_dim=200, drop_rate=0.0,
                           user_log_mask=False, freeze_embedding=True, use_category=False, use_subcategory=False,
                           category_emb_dim=100, lr=3e-4, batch_size=32, epochs=1, log_steps=1000, dp_mode="flat", feed="device",
                           train_data_dir=os.path.join(tmp, "train"), model_dir=None)
    return args, news_index, comb.numpy(), table.numpy()


_ORACLE_TRAJ = {}


def _oracle_trajectory(args, news_index, news_combined, table, steps):
    """The oracle stepping the same batches (same label RNG) from the same initial parameters with torch-CPU Adam; the frozen
    table is no parameter of the optimizer.  Shared by the fp32 and bf16 cases (the initial parameters do not depend on the
    compute dtype)."""
    if steps not in _ORACLE_TRAJ:
        torch.manual_seed(0)
        init = TR.build_model(args, table).state_dict()
        tkey = "news_encoder.embedding_matrix.weight"
        params = {k: v.detach().clone().float().requires_grad_(k != tkey) for k, v in init.items()}
        opt = torch.optim.Adam([p for p in params.values() if p.requires_grad], lr=args.lr)
        random.seed(0)
        ds = D.DatasetTrain(os.path.join(args.train_data_dir, f"behaviors_np{args.npratio}_0.tsv"), news_index, news_combined, args)
        ref = []
        for cnt, (h, m, c, l) in enumerate(torch.utils.data.DataLoader(ds, batch_size=args.batch_size)):
            if cnt == steps:
                break
            loss, _ = O.nrms_forward(h, m, c, l, params, args)
            opt.zero_grad()
            loss.backward()
            opt.step()
            ref.append(float(loss.detach()))
        _ORACLE_TRAJ[steps] = ref
    return _ORACLE_TRAJ[steps]


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_demo_sh_training_config_tracks_the_oracle(tmp_path, dt):
    """src/demo.sh's training run through train.train: NRMS at T=30, H=50, D=300, N=400, 20 heads, npratio 4, batch 32
    (M = 52 800 token rows: compact row storage in bf16), frozen word table, lr 3e-4, flat bucket + fused Adam, device feed,
    dropout 0.  8 steps against the oracle's trajectory: fp32 <= 2e-3 abs per step (measured on MI355X: 2.4e-7), bf16 <= 3e-2
    (measured: 4.3e-4 and 5.0e-4 in two runs); the frozen table is bit-identical afterwards.  ~10 s of oracle (shared by both cases)."""
    args, news_index, news_combined, table = _mind_set(str(tmp_path))
    args.compute_dtype = dt
    assert D.prepare_training_data(args.train_data_dir, 1, args.npratio, seed=0) >= 8 * args.batch_size
    steps = 8
    torch.manual_seed(0)
    random.seed(0)
    model, losses = TR.train(None, args, news_index, news_combined, table, max_steps=steps, log=lambda *_: None)
    assert len(losses) == steps and torch.isfinite(losses).all()
    tab = model.news_encoder.embedding_matrix.weight
    assert not tab.requires_grad and tab.grad is None
    assert torch.equal(tab.detach().cpu(), torch.from_numpy(table))             # frozen: not touched by the steps
    ref = _oracle_trajectory(args, news_index, news_combined, table, steps)
    worst = max(abs(float(a) - b) for a, b in zip(losses, ref))
    print(f"demo.sh config {dt}: worst |loss - oracle| over {steps} steps = {worst:.2e}; losses {losses.tolist()} oracle {ref}")
    assert worst < (2e-3 if dt == "fp32" else 3e-2), (losses.tolist(), ref)


def test_bench_freeze_embedding_runs():
    """bench.py --freeze-embedding (the flagship step with src/demo.sh:12's frozen table) runs to the end."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--freeze-embedding", "--steps", "2",
                        "--warmup", "1"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["config"]["freeze_embedding"] is True
    assert math.isfinite(line["config"]["final_loss"]), line
