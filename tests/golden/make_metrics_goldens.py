"""Writes tests/golden/metrics_cases.npz: sklearn's values for the recipes of tests/metrics_ref.py (needs scikit-learn; the tests do not).

    python tests/golden/make_metrics_goldens.py

Per case: roc_auc_score / average_precision_score of every column against (y == column) and their macro means, the confusion
matrix of argmax, accuracy and precision / recall / f1_score(average="macro", labels=all classes, zero_division=0).  The scores are
NOT stored: the tests regenerate them from the recipe's seed, so the file stays a few KB."""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    import sklearn
    from sklearn import metrics as M
    from tests.metrics_ref import CASES, make_case
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, kind, N, C, seed, prev, levels in CASES:
            s, y = make_case(kind, N, C, seed, prev, levels)
            auroc, auprc = np.full(C, np.nan), np.full(C, np.nan)
            for c in range(C):
                pos = (y == c).astype(int)
                try:
                    auroc[c] = M.roc_auc_score(pos, s[:, c])
                except ValueError:
                    pass
                auprc[c] = M.average_precision_score(pos, s[:, c])
            pred = np.argmax(s, axis=1)
            labels = np.arange(C)
            out[name + "/auroc"], out[name + "/auprc"] = auroc, auprc
            out[name + "/macro"] = np.array([np.mean(auroc), np.mean(auprc)])
            out[name + "/confusion"] = M.confusion_matrix(y, pred, labels=labels).astype(np.int64)
            out[name + "/summary"] = np.array([M.accuracy_score(y, pred)] + [
                f(y, pred, average="macro", labels=labels, zero_division=0) for f in (M.precision_score, M.recall_score, M.f1_score)])
    out["meta"] = np.array(json.dumps({"sklearn": sklearn.__version__, "numpy": np.__version__,
                                       "cases": [list(c) for c in CASES]}))
    path = os.path.join(HERE, "metrics_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(CASES), "cases")


if __name__ == "__main__":
    main()
