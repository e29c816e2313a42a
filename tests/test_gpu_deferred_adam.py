"""GPU: row-deferred Adam over NAML's trainable title table (parallel.FlatBucket(table_adam="deferred"), nr_adam_rows).

The claim under test is EXACTNESS: dense Adam moves a row whose gradient is zero only as a function of that row's own p, m, v and
the step number, so replaying the missed steps later -- same adam1(), a zero gradient, the scalars the dense call derived for
that step -- gives the same bits.  Every comparison between the two modes below is therefore torch.equal; the only bounds are
those of the oracle trajectory, which are tests/test_gpu_naml_trainable_table.py's own (fp32 2e-3, bf16 3e-2)."""
import os
import random

import pytest
import torch

import bench
from newsrecommendation_amd import _lib, data as D, ops, parallel, train as TR
from oracle import nr_oracle as O
from test_gpu_naml_trainable_table import TKEY, WD_, _naml, _naml_set

pytestmark = pytest.mark.gpu
LR, B1, B2, EPS = 3e-4, 0.9, 0.999, 1e-8


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------- 1. kernel against kernel
def _schedule(V, steps, seed):
    """Per step an int32 id list [n, 3] (column 0 = ids, so the kernel sees a stride of 3) with duplicates, id 0 and ids
    outside the table; EVERY is in every list, NEVER in none, FIRST1 first at step 1, LAST first at the last step, GAP at step 2
    and then not again for 20 steps."""
    every, never, first1, last, gap = V - 1, V - 2, V - 3, V - 4, V - 5
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in range(1, steps + 1):
        ids = torch.randint(1, V, (48,), generator=g)
        ids = ids[(ids != never) & (ids != last) & (ids != gap) & (ids != first1)]
        extra = [every, 0, V, V + 7, -3, int(ids[0]), int(ids[0]), every]
        if s == 1:
            extra.append(first1)
        if s == steps:
            extra.append(last)
        if s in (2, 23):
            extra += [gap, gap]
        ids = torch.cat([ids, torch.tensor(extra)])
        ids = ids[torch.randperm(ids.numel(), generator=g)]
        out.append(torch.stack([ids, ids * 0 + 5, ids * 0 + 9], dim=1).to(torch.int32).cuda())
    return out, dict(every=every, never=never, first1=first1, last=last, gap=gap)


def _rows_call(bufs, row_step, sched, ids, upto, apply, V, W, pack):
    p, g, m, v = bufs
    d = _lib.AdamRowsDesc(param=p.data_ptr(), grad=g.data_ptr(), exp_avg=m.data_ptr(), exp_avg_sq=v.data_ptr(), rows=V, width=W,
                          row_step=row_step.data_ptr(), sched=sched.data_ptr(), sched_capacity=sched.shape[0], upto=upto,
                          apply=apply, zero_grad=1, lr=LR, beta1=B1, beta2=B2, eps=EPS, grad_scale=1.0)
    n = V
    if ids is not None:
        col = ids[:, 0]
        d.ids, d.ids_stride, d.n_ids = col.data_ptr(), col.stride(0), col.numel()
        n = col.numel()
    if pack is not None:
        d.pack_dst, d.pack_cols, d.pack_ld = pack[0].data_ptr(), pack[1], pack[0].shape[1]
    ws = torch.empty((_lib.lib().nr_adam_rows_workspace_bytes(n) + 3) // 4, dtype=torch.int32, device="cuda")
    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 4
    _lib.check(_lib.lib().nr_adam_rows(d, _stream()), "nr_adam_rows")


KERNEL_CASES = {"bf16_packed_copy": (4096, 1200, 300, True), "fp32_no_packed_copy": (4096, 1200, 300, False),
                "table_beyond_4GiB": (120000, 9000, 300, True)}


@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_row_kernels_match_the_dense_kernel_bit_for_bit(case):
    """24 steps, path A = nr_adam_step_packed over the whole [V, width] buffer at every step, path B = nr_adam_rows catch-up +
    apply on the step's ids, then one flush: p, m, v and the packed bf16 copy are torch.equal, g is all zero, and at three
    intermediate steps (one of them the return of the row that was away for 20 steps) the rows just caught up equal A's rows
    after the previous step."""
    V, W, cols, packed = KERNEL_CASES[case]
    steps = 24
    if V * W * 4 > 2 ** 32:
        need = 2 * (4 * V * W * 4 + V * (W // cols) * 320 * 2) + 4 * V * W + (8 << 30)
        if torch.cuda.mem_get_info()[0] < need:
            pytest.skip(f"needs {need / 1e9:.0f} GB of free device memory")
    sched_ids, special = _schedule(V, steps, seed=3)
    gen = torch.Generator(device="cuda").manual_seed(11)
    p0 = torch.randn(V * W, generator=gen, device="cuda") * 0.4
    p0[:W] = 0

    def fresh():
        p = p0.clone()
        bufs = (p, torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p))
        pack = None
        if packed:
            dst = torch.empty(V * (W // cols), 320, dtype=torch.bfloat16, device="cuda")
            _lib.check(_lib.lib().nr_cast_pad(p.data_ptr(), V * (W // cols), cols, cols, dst.data_ptr(), 320, _lib.NR_BF16, 0, _stream()),
                       "nr_cast_pad")
            pack = (dst, cols)
        return bufs, pack

    A, packA = fresh()
    Bb, packB = fresh()
    del p0
    row_step = torch.zeros(V, dtype=torch.int32, device="cuda")
    sched = torch.zeros(64, 2, dtype=torch.float32, device="cuda")
    job = None
    if packed:
        job = (_lib.PackJob * 1)(_lib.PackJob(0, V * W, cols, 320, packA[0].data_ptr()))
    touched_ever = torch.zeros(V, dtype=torch.bool)
    for s in range(1, steps + 1):
        ids = sched_ids[s - 1]
        col = ids[:, 0].long()
        rows = torch.unique(col[(col >= 1) & (col < V)])
        touched_ever[rows.cpu()] = True
        _rows_call(Bb, row_step, sched, ids, s - 1, 0, V, W, packB)
        if s in (3, 23, 24):                                # B's rows after catch-up == A's rows after step s - 1
            for a, b, name in zip(A, Bb, "pgmv"):
                assert torch.equal(a.view(V, W)[rows], b.view(V, W)[rows]), (case, s, name)
            if packed:
                T = W // cols
                assert torch.equal(packA[0].view(V, T * 320)[rows], packB[0].view(V, T * 320)[rows]), (case, s, "packed")
        grad = torch.randn(rows.numel(), W, generator=gen, device="cuda") * 0.01
        A[1].view(V, W)[rows] = grad
        Bb[1].view(V, W)[rows] = grad
        _lib.check(_lib.lib().nr_adam_step_packed(A[0].data_ptr(), A[1].data_ptr(), A[2].data_ptr(), A[3].data_ptr(), V * W, LR, B1, B2, EPS, s,
                                                  1.0, 1, job, 1 if packed else 0, _stream()), "nr_adam_step_packed")
        _rows_call(Bb, row_step, sched, ids, s - 1, 1, V, W, packB)
    assert bool(touched_ever[special["every"]]) and not bool(touched_ever[special["never"]]) and not bool(touched_ever[0])
    # before the flush B lags behind on purpose: the row that was touched at step 1 only has not moved since
    assert not torch.equal(A[0].view(V, W)[special["first1"]], Bb[0].view(V, W)[special["first1"]])
    _rows_call(Bb, row_step, sched, None, steps, 0, V, W, packB)
    torch.cuda.synchronize()
    assert int(row_step[1:].min()) == steps and int(row_step[1:].max()) == steps and int(row_step[0]) == 0
    for a, b, name in zip(A, Bb, ("p", "g", "m", "v")):
        assert torch.equal(a, b), (case, name)
    assert float(Bb[1].abs().max()) == 0.0 and float(A[1].abs().max()) == 0.0
    if packed:
        assert torch.equal(packA[0], packB[0]), (case, "packed copy")
    never = special["never"]
    assert float(Bb[2].view(V, W)[never].abs().max()) == 0.0                      # a row without any gradient never moves
    assert float(Bb[2].view(V, W)[special["last"]].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------- 2., 3. train.train
def _train(tmp, dt, table_adam, steps, deterministic):
    args, news_index, comb, table, cats, subs = _naml_set(tmp, n_imp=480)
    args.compute_dtype, args.dp_mode, args.feed, args.table_adam, args.deterministic = dt, "flat", "device", table_adam, deterministic
    assert D.prepare_training_data(args.train_data_dir, 1, args.npratio, seed=0) >= steps * args.batch_size
    torch.manual_seed(0)
    random.seed(0)
    try:
        model, losses = TR.train(None, args, news_index, comb, table, cats, subs, max_steps=steps, log=lambda *_: None)
    finally:
        if deterministic:
            ops.set_deterministic(False)
    assert len(losses) == steps and torch.isfinite(losses).all()
    return model, losses, (args, news_index, comb, table, cats, subs)


def _assert_same_state(m_a, fb_a, m_b, fb_b, what):
    sa, sb = m_a.state_dict(), m_b.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (what, "model", k)
    ba, bb = fb_a.state_dict(), fb_b.state_dict()
    assert ba["state"].keys() == bb["state"].keys() and TKEY in ba["state"]
    assert (ba["lr"], ba["betas"], ba["eps"]) == (bb["lr"], bb["betas"], bb["eps"])
    for k in ba["state"]:
        assert ba["state"][k]["step"] == bb["state"][k]["step"], (what, k)
        for f in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(ba["state"][k][f], bb["state"][k][f]), (what, "bucket", k, f)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_train_loop_deferred_equals_dense_bit_for_bit(tmp_path, dt):
    """train.train, 12 steps in deterministic mode, table_adam dense against deferred: the losses, every entry of
    model.state_dict() and every entry of the bucket's state_dict() are torch.equal."""
    m_d, l_d, _ = _train(str(tmp_path / "dense"), dt, "dense", 12, True)
    m_r, l_r, _ = _train(str(tmp_path / "deferred"), dt, "deferred", 12, True)
    assert m_d._nr_bucket.table_adam == "dense" and m_r._nr_bucket.table_adam == "deferred"
    assert torch.equal(l_d, l_r), (l_d.tolist(), l_r.tolist())
    _assert_same_state(m_d, m_d._nr_bucket, m_r, m_r._nr_bucket, dt)
    was = torch.from_numpy(_naml_set(str(tmp_path / "again"), n_imp=480)[3])
    moved = (m_r.state_dict()[TKEY].cpu() != was).any(dim=1)
    assert int(moved.sum()) > 50 and not bool(moved[0])


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_train_loop_deferred_tracks_the_oracle(tmp_path, dt):
    """The same 12 steps in the default (non-deterministic) mode against the oracle + torch.optim.Adam, at the bounds of
    test_gpu_naml_trainable_table.test_training_loop_with_a_trainable_table_tracks_the_oracle: fp32 2e-3, bf16 3e-2."""
    steps = 12
    model, losses, (args, news_index, comb, table, cats, subs) = _train(str(tmp_path), dt, "deferred", steps, False)
    torch.manual_seed(0)
    init = TR.build_model(args, table, len(cats), len(subs)).state_dict()
    params = {k: v.detach().clone().float().requires_grad_(True) for k, v in init.items()}
    opt = torch.optim.Adam(list(params.values()), lr=args.lr)
    random.seed(0)
    ds = D.DatasetTrain(os.path.join(args.train_data_dir, f"behaviors_np{args.npratio}_0.tsv"), news_index, comb, args)
    ref = []
    for cnt, (h, mk, c, l) in enumerate(torch.utils.data.DataLoader(ds, batch_size=args.batch_size)):
        if cnt == steps:
            break
        loss, _ = O.naml_forward(h, mk, c, l, params, args)
        opt.zero_grad()
        loss.backward()
        opt.step()
        ref.append(float(loss.detach()))
    worst = max(abs(float(a) - b_) for a, b_ in zip(losses, ref))
    print(f"naml deferred loop {dt}: worst |loss - oracle| over {steps} steps = {worst:.2e}")
    assert worst < (2e-3 if dt == "fp32" else 3e-2), (losses.tolist(), ref)
    # the flushed table against the oracle's densely stepped one: rows that were never in a batch included
    tab_o = params[TKEY].detach()
    err = float((model.state_dict()[TKEY].cpu() - tab_o).abs().max())
    print(f"table vs oracle after {steps} steps: max|diff| {err:.2e}")
    assert err < 12 * args.lr                                   # (each Adam step moves a value by about lr at most)
    if dt == "bf16":
        tab = model.news_encoder.title_embeddings.weight
        served = ops.table_cache.get(tab, ops.dtype_code(dt), row_cols=WD_)
        assert torch.equal(served, ops.pack(tab.detach().reshape(-1, WD_).clone(), ops.dtype_code(dt)))


# ------------------------------------------------------------------------------------------------- 4. - 7. model + bucket loops
N_LOOP, B_LOOP = 2500, 64


def _loop_case(dt, n_batches):
    cfg = O.default_cfg(use_category=True, use_subcategory=True, freeze_embedding=False, drop_rate=0.0)
    g = torch.Generator().manual_seed(60)
    table = torch.randn(N_LOOP + 1, cfg.num_words_title * cfg.word_embedding_dim, generator=g) * 0.4
    table[0] = 0
    sd = O.init_state_dict("NAML", cfg, table, seed=61, n_cat=17, n_sub=264)
    batches = bench.synth_batches_naml(cfg, B_LOOP, N_LOOP, n_batches, 62, "cuda")
    return cfg, sd, batches


def _bucket(cfg, sd, dt, table_adam):
    m = _naml(cfg, sd[TKEY], sd, dt, True)
    return m, parallel.FlatBucket(m, lr=LR, table_adam=table_adam)


def _steps(m, fb, batches):
    out = []
    for hist, mask, cand, label in batches:
        loss, _ = m(hist, mask, cand, label)
        loss.backward()
        fb.step()
        out.append(loss.detach())
    return torch.stack(out)


@pytest.fixture
def deterministic():
    ops.set_deterministic(True, elements=(N_LOOP + 1) * 9000 + (4 << 20))
    yield
    ops.set_deterministic(False)


def _logged_step(m, fb, batch):
    _lib.prof_enable(1)
    try:
        _lib.prof_collect()
        _steps(m, fb, [batch])
        torch.cuda.synchronize()
        return _lib.prof_collect()
    finally:
        _lib.prof_enable(0)


def test_launch_log_of_a_deferred_and_of_a_dense_step():
    """Step 3 of a bf16 run.  deferred: adam_rows_claim and adam_rows_apply run, the only adam_step launch stops in front of the
    table, and the table is not re-packed (no cast_pad over its V*T token rows).  dense: one adam_step over the whole bucket,
    no adam_rows launch; apart from the Adam launches the two modes launch the same kernels."""
    cfg, sd, batches = _loop_case("bf16", 3)
    logs = {}
    shared = ops.pack_cache
    for mode in ("dense", "deferred"):
        # ops.pack_cache refreshes the stale packs of EVERY bucket registered with it in its cast_pad_batch launches (a
        # registration keeps its bucket alive), so the job counts in the log depend on what ran before in this process: each
        # run gets a pack cache of its own, which knows its bucket only
        ops.pack_cache = ops._PackCache()
        try:
            m, fb = _bucket(cfg, sd, "bf16", mode)
            _steps(m, fb, batches[:2])
            logs[mode] = (_logged_step(m, fb, batches[2]), fb.numel, getattr(fb, "_table_off", None))
        finally:
            ops.pack_cache = shared
        del m, fb
        ops.table_cache.invalidate()
    table_pack = f"cast_pad[rows={(N_LOOP + 1) * cfg.num_words_title},"
    dense, numel_d, _ = logs["dense"]
    assert [k for k in dense if k.startswith("adam_step")] == [f"adam_step[n={numel_d}]"], sorted(dense)
    assert dense[f"adam_step[n={numel_d}]"][0] == 1
    assert not any(k.startswith("adam_rows") for k in dense)
    assert not any(k.startswith(table_pack) for k in dense)
    rows, numel_r, table_off = logs["deferred"]
    assert table_off + (N_LOOP + 1) * 9000 <= numel_r
    assert [k for k in rows if k.startswith("adam_step")] == [f"adam_step[n={table_off}]"], sorted(rows)
    claim = [k for k in rows if k.startswith("adam_rows_claim[")]
    apply_ = [k for k in rows if k.startswith("adam_rows_apply[")]
    assert len(claim) == 2 and len(apply_) == 2, sorted(rows)           # the catch-up before the forward, the step after the backward
    assert any("apply=0" in k for k in apply_) and any("apply=1" in k for k in apply_)
    assert not any(k.startswith(table_pack) for k in rows), sorted(rows)
    strip = lambda log: {k for k in log if not k.startswith(("adam_step", "adam_rows"))}
    assert strip(dense) == strip(rows)


def test_eval_forward_between_steps_reads_current_rows(deterministic):
    """After step 5 a no_grad forward in eval() -- over the batch of step 2 and over a batch of its own -- gives the dense run's
    scores bit for bit, and the run ends in the dense run's parameters: reading catches rows up, it does not step them."""
    cfg, sd, batches = _loop_case("bf16", 11)
    res = {}
    for mode in ("dense", "deferred"):
        m, fb = _bucket(cfg, sd, "bf16", mode)
        l1 = _steps(m, fb, batches[:5])
        m.eval()
        with torch.no_grad():
            scores = [m(*batches[1])[1].clone(), m(*batches[10])[1].clone()]
            every = torch.arange(0, N_LOOP + 1, dtype=torch.int32, device="cuda")
            nv = m.news_encoder(torch.stack([every, every % 17, every % 200], dim=1)).clone()
        m.train()
        l2 = _steps(m, fb, batches[5:10])
        res[mode] = (m, fb, torch.cat([l1, l2]), scores, nv)
    for a, b in zip(res["dense"][3], res["deferred"][3]):
        assert torch.equal(a, b)
    assert torch.equal(res["dense"][4], res["deferred"][4])
    assert torch.equal(res["dense"][2], res["deferred"][2])
    _assert_same_state(res["dense"][0], res["dense"][1], res["deferred"][0], res["deferred"][1], "eval between steps")


@pytest.mark.parametrize("first,second", [("deferred", "dense"), ("dense", "deferred")])
def test_checkpoint_moves_between_the_two_modes(deterministic, first, second):
    """6 steps in one mode, model.state_dict() + bucket.state_dict() saved, loaded into a fresh model + bucket of the OTHER mode, 6
    more steps: equal to 12 dense steps."""
    cfg, sd, batches = _loop_case("bf16", 12)
    m_ref, fb_ref = _bucket(cfg, sd, "bf16", "dense")
    l_ref = _steps(m_ref, fb_ref, batches)
    m1, fb1 = _bucket(cfg, sd, "bf16", first)
    l1 = _steps(m1, fb1, batches[:6])
    opt_sd = fb1.state_dict()                                   # (flushes a deferred table: the model's entries below are current)
    model_sd = {k: v.detach().cpu().clone() for k, v in m1.state_dict().items()}
    assert all(st["step"] == 6 for st in opt_sd["state"].values())
    del m1, fb1
    m2, fb2 = _bucket(cfg, model_sd, "bf16", second)
    fb2.load_state_dict(opt_sd)
    l2 = _steps(m2, fb2, batches[6:])
    assert torch.equal(torch.cat([l1, l2]), l_ref)
    _assert_same_state(m_ref, fb_ref, m2, fb2, f"{first} -> {second}")


def test_zero_grad_abort_then_a_normal_step(deterministic):
    """A forward and a backward, zero_grad() instead of step(), then normal steps: the deferred run ends where the dense run doing
    the same ends (the rows of the aborted batch are not stepped)."""
    cfg, sd, batches = _loop_case("bf16", 4)
    res = {}
    for mode in ("dense", "deferred"):
        m, fb = _bucket(cfg, sd, "bf16", mode)
        _steps(m, fb, batches[:1])
        loss, _ = m(*batches[1])
        loss.backward()
        fb.zero_grad()
        assert float(fb.grad.abs().max()) == 0.0
        res[mode] = (m, fb, _steps(m, fb, batches[2:]))
    assert res["deferred"][1]._step_ids == []
    assert torch.equal(res["dense"][2], res["deferred"][2])
    _assert_same_state(res["dense"][0], res["dense"][1], res["deferred"][0], res["deferred"][1], "zero_grad abort")


def test_construction_errors():
    """A model without a large trainable table, and eps == 0, are refused with a ValueError that says why."""
    cfg, sd, _ = _loop_case("bf16", 1)
    from newsrecommendation_amd.model import NAML
    from types import SimpleNamespace
    args = SimpleNamespace(**{**vars(cfg), "compute_dtype": "bf16", "freeze_embedding": True, "stream_title_table": False})
    m = NAML.Model(args, sd[TKEY].numpy(), 17, 264).cuda()
    with pytest.raises(ValueError, match="2\\^20"):
        parallel.FlatBucket(m, lr=LR, table_adam="deferred")
    m2 = _naml(cfg, sd[TKEY], sd, "bf16", True)
    with pytest.raises(ValueError, match="eps"):
        parallel.FlatBucket(m2, lr=LR, eps=0.0, table_adam="deferred")
