"""Shared by tests/test_sample_host.py and tests/test_gpu_sample.py: the configuration of "the law" (8 news, 4096 identical users)
and its two Pearson chi-square statistics."""
import numpy as np

LAW_X = np.array([0.3, -0.2, 1.1, 0.9, -1.0, 0.0, 0.5, 0.31])      # scores of news 1 .. 8
LAW_U, LAW_TAU, LAW_SEED, LAW_DRAW = 4096, 0.7, 12345, 0
CHI2_FIRST_MAX = 29.88          # 99.99 % quantile of chi-square, 7 degrees of freedom
CHI2_SECOND_MAX = 27.86         # 99.99 % quantile, 6 degrees of freedom
LAW_GIVEN = 4                   # the second place is examined among the users whose first place is this news


def law_scores():
    """[LAW_U, 9] float64: every user the same row; column 0 is the padding news."""
    return np.tile(np.concatenate([[0.0], LAW_X]), (LAW_U, 1))


def law_chi2(ids):
    """ids [LAW_U, >= 2] -> (chi2 of the first place against softmax(x / tau), chi2 of the second place among the users whose
    first place is LAW_GIVEN against the softmax over the other seven, the number of those users)."""
    ids = np.asarray(ids, dtype=np.int64)
    p = np.exp(LAW_X / LAW_TAU)
    p /= p.sum()
    first = np.bincount(ids[:, 0], minlength=9)[1:9]
    assert first.sum() == len(ids)
    chi1 = float(((first - len(ids) * p) ** 2 / (len(ids) * p)).sum())
    sel = ids[:, 0] == LAW_GIVEN
    rest = np.array([v for v in range(1, 9) if v != LAW_GIVEN])
    q = np.exp(LAW_X[rest - 1] / LAW_TAU)
    q /= q.sum()
    second = np.bincount(ids[sel, 1], minlength=9)[rest]
    assert second.sum() == sel.sum()
    chi2 = float(((second - sel.sum() * q) ** 2 / (sel.sum() * q)).sum())
    return chi1, chi2, int(sel.sum())
