"""numpy restatement of the validation metrics (include/raindrop_hip.h "validation metrics") and the recipes of the metric fixtures.

The formulas are sklearn's `roc_auc_score` / `average_precision_score` written out: thresholds are the DISTINCT score values, tied
scores form one group; with tp, fp the cumulative counts at the end of each tie group in descending score order, P positives and
Q = N - P,

    AUROC = sum (fp - fp_prev)(tp + tp_prev) / (2 P Q)          numerator: exact integer
    AP    = sum (tp - tp_prev) / P * tp / (tp + fp)             float64

tests/test_metrics_ref.py pins this restatement to values recorded from sklearn (tests/golden/metrics_cases.npz, written by
tests/golden/make_metrics_goldens.py); the GPU tests then need no sklearn where they run."""
import numpy as np

# (name, kind, N, C, seed, prevalence, quantisation levels [0 = untied])
CASES = [("bin_n%d_p%02d_q%d" % (N, int(prev * 100), lv), "binary", N, 2, 1000 + 7 * i, prev, lv)
         for i, (N, prev, lv) in enumerate((N, prev, lv) for N in (7, 530, 3880, 16384, 16385, 65536)
                                           for prev in (0.04, 0.5) for lv in (0, 64, 3))]
CASES += [("equal_n530", "equal", 530, 2, 11, 0.5, 1), ("separated_n530", "separated", 530, 2, 12, 0.5, 0),
          ("separated_n16385", "separated", 16385, 2, 13, 0.04, 0),
          ("sigmoid8_n3880", "sigmoid8", 3880, 8, 14, 0.0, 0), ("softmax8_n3880", "softmax8", 3880, 8, 15, 0.0, 0),
          ("absent8_n3880", "absent8", 3880, 8, 16, 0.0, 0), ("sigmoid8_n16385", "sigmoid8", 16385, 8, 17, 0.0, 0)]


def make_case(kind, N, C, seed, prev, levels):
    """(scores float32 [N, C], y int64 [N]) of a fixture recipe, regenerated from the seed.  The binary recipes use IEEE-exact
    arithmetic only (the same bits wherever numpy runs)."""
    rng = np.random.default_rng(seed)
    if kind in ("binary", "equal", "separated"):
        y = (rng.random(N) < prev).astype(np.int64)
        if kind == "equal":
            s = np.full(N, 0.5)
        elif kind == "separated":
            s = 0.25 * rng.random(N) + 0.5 * y
        else:
            s = 0.7 * rng.random(N) + 0.3 * y * rng.random(N)
            if levels:
                s = np.floor(s * levels) / levels
        s = s.astype(np.float32)
        return np.stack([np.float32(1) - s, s], 1), y
    y = rng.integers(0, C, size=N).astype(np.int64)
    if kind == "absent8":
        y[y == 5] = 2
    z = rng.standard_normal((N, C)) + 1.5 * np.eye(C)[y]
    if kind == "softmax8":
        e = np.exp(z - z.max(1, keepdims=True))
        return (e / e.sum(1, keepdims=True)).astype(np.float32), y
    return (1.0 / (1.0 + np.exp(-z))).astype(np.float32), y


def rank_column(s, pos):
    """(auroc, ap, integer AUROC numerator) of one score column against the boolean positives."""
    s = np.asarray(s, dtype=np.float32)
    pos = np.asarray(pos, dtype=bool)
    N = s.shape[0]
    order = np.argsort(-s, kind="stable")
    ss, pp = s[order], pos[order]
    ends = np.r_[np.nonzero(np.diff(ss) != 0)[0], N - 1]
    tp = np.cumsum(pp.astype(np.int64))[ends]
    fp = ends + 1 - tp
    tpp, fpp = np.r_[0, tp[:-1]], np.r_[0, fp[:-1]]
    P = int(tp[-1])
    Q = N - P
    num = int(np.sum((fp - fpp) * (tp + tpp)))
    auroc = num / (2.0 * P * Q) if P > 0 and Q > 0 else float("nan")
    ap = float(np.sum((tp - tpp).astype(np.float64) / P * tp / (tp + fp))) if P > 0 else 0.0
    return auroc, ap, num


def rank_metrics_ref(scores, y):
    """dict(auroc [C], auprc [C], num [C] int64, auroc_macro, auprc_macro) with the kernels' conventions (NaN AUROC for a column
    without positives or negatives, AP 0 without positives, plain means)."""
    scores = np.asarray(scores)
    C = scores.shape[1]
    cols = [rank_column(scores[:, c], np.asarray(y) == c) for c in range(C)]
    a, p = np.array([c[0] for c in cols]), np.array([c[1] for c in cols])
    return {"auroc": a, "auprc": p, "num": np.array([c[2] for c in cols], dtype=np.int64),
            "auroc_macro": float(np.mean(a)), "auprc_macro": float(np.mean(p))}


def confusion_ref(scores, y):
    C = scores.shape[1]
    cm = np.zeros((C, C), dtype=np.int64)
    np.add.at(cm, (np.asarray(y), np.argmax(scores, axis=1)), 1)
    return cm
