"""CPU: the numpy restatement of the ranking / classification metrics (tests/metrics_ref.py: the algorithm rd_metrics.hip
implements) reproduces every value recorded from sklearn in tests/golden/metrics_cases.npz.

Bound 1e-10 absolute: the integer parts are exact; the float64 sums have at most 65536 terms of magnitude <= 1, i.e. at most
N * 2^-53 ~ 7e-12 of rounding, while a wrong tie rule or a miscounted sample moves a value by >= 1 / N^2 ~ 2e-10 (only at
N = 65536 for a single swapped pair -- there the exact integer numerator is checked as well, against sklearn's AUROC * 2PQ)."""
import json
import os

import numpy as np
import pytest

from tests import metrics_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_cases.npz")
TOL = 1e-10


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and (np.abs(a - b)[~np.isnan(b)] <= TOL).all()


def test_fixture_holds_the_recipes_of_the_test_tree():
    with np.load(GOLD) as g:
        meta = json.loads(str(g["meta"]))
    assert [tuple(c) for c in meta["cases"]] == [tuple(c) for c in R.CASES]
    Ns = {c[2] for c in R.CASES}
    assert {7, 530, 3880, 16384, 16385, 65536} <= Ns


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_restatement_reproduces_sklearn(case):
    name = case[0]
    s, y = R.make_case(*case[1:])
    with np.load(GOLD) as g:
        gold = {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(name + "/")}
    r = R.rank_metrics_ref(s, y)
    assert _close(r["auroc"], gold["auroc"]), (r["auroc"], gold["auroc"])
    assert _close(r["auprc"], gold["auprc"]), (r["auprc"], gold["auprc"])
    assert _close([r["auroc_macro"], r["auprc_macro"]], gold["macro"])
    N = s.shape[0]
    for c in range(s.shape[1]):                        # the exact numerator against sklearn's quotient (exact to 2^-52 relative)
        P = int((y == c).sum())
        if 0 < P < N:
            assert abs(r["num"][c] - gold["auroc"][c] * 2.0 * P * (N - P)) < 0.25, c
    cm = R.confusion_ref(s, y)
    assert np.array_equal(cm, gold["confusion"])
    from raindrop_amd.metrics import summary_from_confusion
    assert np.abs(np.array(summary_from_confusion(cm)) - gold["summary"]).max() <= TOL


def test_degenerate_columns_are_in_the_fixture():
    """no positives -> AUROC NaN, AP 0 (sklearn's convention); all scores equal -> AUROC 0.5, AP = prevalence"""
    with np.load(GOLD) as g:
        assert any(np.isnan(g[k]).any() for k in g.files if k.endswith("/auroc"))
        assert np.isnan(g["absent8_n3880/auroc"][5]) and g["absent8_n3880/auprc"][5] == 0.0
        assert abs(g["equal_n530/auroc"][1] - 0.5) < 1e-15
