"""CPU: the host side of row-deferred Adam (table_adam="deferred"): argument checks of train.train and parallel.FlatBucket, and
the checks nr_adam_rows makes before it launches anything (fake non-null pointers: a launch would fault, a refusal does not)."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from newsrecommendation_amd import _lib, parallel, train as TR


def _args(**kw):
    a = dict(model="NAML", dp_mode="flat", table_adam="deferred", lr=1e-4)
    a.update(kw)
    return SimpleNamespace(**a)


def test_invalid_table_adam_is_a_value_error():
    with pytest.raises(ValueError, match="table_adam must be 'dense' or 'deferred'"):
        TR.train(None, _args(table_adam="sparse"), {}, None, None, device="cpu")
    with pytest.raises(ValueError, match="table_adam"):
        parallel.FlatBucket(torch.nn.Linear(4, 4), lr=1e-3, table_adam="lazy")


def test_ddp_with_deferred_is_a_value_error():
    with pytest.raises(ValueError, match="dp_mode='ddp'"):
        TR.train(None, _args(dp_mode="ddp"), {}, None, None, device="cpu")
    with pytest.raises(ValueError, match="dp_mode='ddp'"):                 # the CPU default of dp_mode is ddp
        TR.train(None, _args(dp_mode=None), {}, None, None, device="cpu")


def test_deferred_needs_a_model_that_announces_its_rows():
    with pytest.raises(ValueError, match="NRMS"):
        TR.train(None, _args(model="NRMS"), {}, None, None, device="cpu")


def test_deferred_needs_a_large_table_and_eps():
    with pytest.raises(ValueError, match="2\\^20"):
        parallel.FlatBucket(torch.nn.Linear(8, 8), lr=1e-3, table_adam="deferred")
    emb = torch.nn.Embedding(1 << 12, 1 << 8)
    before = emb.weight.data_ptr()
    with pytest.raises(ValueError, match="eps"):
        parallel.FlatBucket(emb, lr=1e-3, eps=0.0, table_adam="deferred")
    assert emb.weight.data_ptr() == before and emb.weight.grad is None      # refused before the parameters were moved


def test_default_is_dense():
    fb = parallel.FlatBucket(torch.nn.Linear(8, 8), lr=1e-3)
    assert fb.table_adam == "dense" and fb._table is None
    fb.flush()                                                             # a no-op


def test_workspace_bytes_is_host_arithmetic():
    lib = _lib.lib()
    b0, b1, b2 = (lib.nr_adam_rows_workspace_bytes(n) for n in (0, 28160, 65001))
    assert b0 >= 4 and b0 % 16 == 0
    assert b1 == b0 + 28160 * 8 and b2 == b0 + 65001 * 8                   # the counter + one (row, steps it had) pair per id
    assert lib.nr_adam_rows_workspace_bytes(-1) == 0


def _desc(**changes):
    lib = _lib.lib()
    f = dict(param=4096, grad=4096, exp_avg=4096, exp_avg_sq=4096, rows=65001, width=9000, row_step=4096, sched=4096,
             sched_capacity=64, ids=4096, ids_stride=3, n_ids=28160, upto=5, apply=1, zero_grad=1, lr=1e-4, beta1=0.9, beta2=0.999,
             eps=1e-8, grad_scale=1.0, pack_dst=4096, pack_cols=300, pack_ld=320, ws=4096,
             ws_bytes=lib.nr_adam_rows_workspace_bytes(28160))
    f.update(changes)
    return _lib.AdamRowsDesc(**f)


REFUSED = {
    "eps_zero": (dict(eps=0.0), "eps == 0"),
    "undersized_workspace": (dict(ws_bytes=64), "nr_adam_rows_workspace_bytes"),
    "undersized_workspace_for_a_flush": (dict(ids=None), "nr_adam_rows_workspace_bytes"),
    "no_workspace": (dict(ws=None), "nr_adam_rows_workspace_bytes"),
    "sched_too_short": (dict(upto=63), "sched holds 64 steps"),
    "width_not_multiple_of_4": (dict(width=9001), "multiple of 4"),
    "packed_copy_does_not_split_a_row": (dict(pack_cols=296), "packed copy"),
    "bad_apply": (dict(apply=2), "apply must be"),
    "bad_beta": (dict(beta2=1.0), "hyper-parameters"),
    "negative_upto": (dict(upto=-1), "hyper-parameters"),
    "null_gradient_for_a_step": (dict(grad=None), "null pointer"),
    "misaligned": (dict(exp_avg=4100), "16-byte aligned"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_bad_descriptor_is_refused_before_any_launch(name):
    change, message = REFUSED[name]
    rc = _lib.lib().nr_adam_rows(C.byref(_desc(**change)), None)
    assert rc == 1 and message in _lib.last_error(), (name, _lib.last_error())


def test_null_descriptor_is_refused():
    assert _lib.lib().nr_adam_rows(None, None) == 1 and "null descriptor" in _lib.last_error()
