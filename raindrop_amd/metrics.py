"""Validation metrics on the device (raindrop_amd/csrc/rd_metrics.hip; include/raindrop_hip.h "validation metrics").

`code/Raindrop.py:348-370` copies the logits to the host after every epoch and calls `sklearn.metrics.roc_auc_score` /
`average_precision_score` there; on the test split it adds accuracy and, for PAM, macro precision / recall / F1 (`:385-401`).
Here the ranking statistics and the confusion matrix are computed where the logits are, with sklearn's semantics (thresholds =
distinct scores, ties form one group); results stay device tensors until the caller reads them.

    r = rank_metrics(torch.sigmoid(logits), y)      # r["auroc"], r["auprc"]: 0-d float64 device tensors (means over the columns)
                                                    # r["auroc_per_class"], r["auprc_per_class"]: [C] float64
                                                    # r["auroc_num"]: [C] int64, the exact numerators  sum (fp - fp')(tp + tp')
    b = rank_bootstrap(scores, y, n_boot=1000)      # b["auroc_ci"], b["auprc_ci"]: [C, 2] percentile intervals over 1000 resamples of
                                                    # the rows (raindrop_amd/csrc/rd_metrics_boot.hip; N <= 16384, n_boot <= 4096)
    cm = confusion(logits, y)                       # [C, C] int64, rows = true class, columns = argmax
    acc, prec, rec, f1 = summary_from_confusion(cm.cpu().numpy())

NaN scores are not refused (that would cost a device sync): a NaN with the sign bit clear ranks above +inf, one with it set below
-inf.  There is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(scores, y, what):
    for t in (scores, y):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.RaindropHipError("%s needs ROCm device tensors; there is no CPU fallback" % what)
    if scores.dim() != 2 or scores.dtype != torch.float32 or scores.stride(1) != 1 or scores.stride(0) < scores.shape[1]:
        raise _lib.RaindropHipError("%s: scores must be float32 [N, C] with unit column stride, got %s %s strides %s"
                                    % (what, scores.dtype, tuple(scores.shape), scores.stride()))
    if y.dtype != torch.int64 or y.dim() != 1 or y.shape[0] != scores.shape[0] or not y.is_contiguous() or y.device != scores.device:
        raise _lib.RaindropHipError("%s: y must be contiguous int64 [N] on the scores' device" % what)


def rank_workspace(N, C, device):
    """Workspace tensor `rank_metrics` needs for [N, C] scores (empty-ish for N <= 16384: sorted in LDS)."""
    n = int(_lib.load().rd_rank_metrics_workspace_bytes(int(N), int(C)))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device)


def rank_metrics(scores, y, out=None, workspace=None):
    """One-vs-rest AUROC and average precision of every column of `scores` [N, C] against `y == column` (module docstring).
    `out`: the dict of a previous call, to write into the same tensors (captured use); `workspace`: from `rank_workspace`."""
    _check(scores, y, "rank_metrics")
    N, C = scores.shape
    if N < 1:
        raise _lib.RaindropHipError("rank_metrics: no samples")
    dev = scores.device
    if out is None:
        f64 = dict(dtype=torch.float64, device=dev)
        mean = torch.empty(2, **f64)
        out = {"auroc_per_class": torch.empty(C, **f64), "auprc_per_class": torch.empty(C, **f64), "mean": mean,
               "auroc": mean[0], "auprc": mean[1], "auroc_num": torch.empty(C, dtype=torch.int64, device=dev)}
    ws = rank_workspace(N, C, dev) if workspace is None else workspace
    _lib.call("rd_rank_metrics", int(N), int(C), _p(scores), int(scores.stride(0)), _p(y), _p(out["auroc_per_class"]),
              _p(out["auprc_per_class"]), _p(out["mean"]), _p(out["auroc_num"]), _p(ws), ws.numel(), _stream())
    return out


BOOT_N_MAX, BOOT_R_MAX = 16384, 4096       # rd_rank_bootstrap's envelope (include/raindrop_hip.h)


def bootstrap_workspace(N, C, R, device):
    """Workspace tensor `rank_bootstrap` needs for [N, C] scores and R resamples (the sorted samples of every column, 2 bytes each)."""
    n = int(_lib.load().rd_rank_bootstrap_workspace_bytes(int(N), int(C), int(R)))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device)


def rank_bootstrap(scores, y, n_boot=1000, seed=0, alpha=0.05, out=None, workspace=None):
    """Bootstrap of `rank_metrics`: `n_boot` resamples of the N rows with replacement (one draw per resample, shared by the columns: a
    pure function of (seed, resample, N), include/raindrop_hip.h "resample rule"), every column's statistics on each with sklearn's
    semantics on the expanded resample, and the two-sided percentile interval at level `alpha` over the resamples whose value is
    defined.  N <= 16384, n_boot <= 4096; there is no CPU fallback.  Returns a dict of device tensors:

        auroc_boot, auprc_boot          [R, C] float64 (AUROC NaN where a resample has no positive or no negative of the column)
        auroc_num_boot, pos_boot        [R, C] int64: the exact numerators and the weighted positives P_r
        mean_boot                       [R, 2] float64: the macro means of each resample
        summary                         [2, C + 1, 5] float64: metric (AUROC, AUPRC) x (columns, then the macro mean) x
                                        (n_valid, mean, standard deviation with ddof = 1, lower, upper); the rest are views of it:
        auroc_ci, auprc_ci              [C, 2]    lower, upper = numpy.percentile(valid, [100 alpha / 2, 100 (1 - alpha / 2)])
        auroc_macro_ci, auprc_macro_ci  [2]
        auroc_se, auprc_se              [C + 1]   the bootstrap standard error (entry C: the macro mean's)
        n_valid                         [2, C + 1] resamples that entered, as float64

    `out`: the dict of a previous call, to write into the same tensors (captured use); `workspace`: from `bootstrap_workspace`."""
    _check(scores, y, "rank_bootstrap")
    N, C = scores.shape
    R = int(n_boot)
    if N < 1:
        raise _lib.RaindropHipError("rank_bootstrap: no samples")
    if not 0.0 < float(alpha) < 1.0:
        raise ValueError("rank_bootstrap: alpha must lie in (0, 1), got %r" % (alpha,))
    dev = scores.device
    if out is None:
        f64, i64 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int64, device=dev)
        s = torch.empty((2, C + 1, 5), **f64)
        out = {"auroc_boot": torch.empty((R, C), **f64), "auprc_boot": torch.empty((R, C), **f64),
               "auroc_num_boot": torch.empty((R, C), **i64), "pos_boot": torch.empty((R, C), **i64), "mean_boot": torch.empty((R, 2), **f64),
               "summary": s, "auroc_ci": s[0, :C, 3:], "auprc_ci": s[1, :C, 3:], "auroc_macro_ci": s[0, C, 3:], "auprc_macro_ci": s[1, C, 3:],
               "auroc_se": s[0, :, 2], "auprc_se": s[1, :, 2], "n_valid": s[:, :, 0]}
    elif tuple(out["auroc_boot"].shape) != (R, C):
        raise _lib.RaindropHipError("rank_bootstrap: out= holds %s resamples x columns, this call has %s"
                                    % (tuple(out["auroc_boot"].shape), (R, C)))
    ws = bootstrap_workspace(N, C, R, dev) if workspace is None else workspace
    _lib.call("rd_rank_bootstrap", int(N), int(C), _p(scores), int(scores.stride(0)), _p(y), R, int(seed) & 0xFFFFFFFFFFFFFFFF,
              _p(out["auroc_boot"]), _p(out["auprc_boot"]), _p(out["auroc_num_boot"]), _p(out["pos_boot"]), _p(out["mean_boot"]),
              _p(ws), ws.numel(), _stream())
    _lib.call("rd_rank_bootstrap_summary", R, int(C), _p(out["auroc_boot"]), _p(out["auprc_boot"]), _p(out["mean_boot"]), float(alpha),
              _p(out["summary"]), _stream())
    return out


def bootstrap_counts(N, n_boot, seed, r0=0, nr=None, device="cuda"):
    """uint32-valued int32 tensor [nr, N]: how often resample r0 .. r0 + nr - 1 of `rank_bootstrap(n_boot=, seed=)` draws each row
    (rd_rank_bootstrap_counts: the tests' handle on the resample rule).  Rows sum to N."""
    nr = int(n_boot) - int(r0) if nr is None else int(nr)
    counts = torch.empty((max(nr, 0), int(N)), dtype=torch.int32, device=device)
    with torch.cuda.device(counts.device):
        _lib.call("rd_rank_bootstrap_counts", int(N), int(n_boot), int(seed) & 0xFFFFFFFFFFFFFFFF, int(r0), nr, _p(counts), _stream())
    return counts


def confusion(logits, y, out=None):
    """int64 [C, C] device tensor: rows = true class, columns = argmax of the row (first maximum, as np.argmax)."""
    _check(logits, y, "confusion")
    N, C = logits.shape
    cm = torch.empty((C, C), dtype=torch.int64, device=logits.device) if out is None else out
    _lib.call("rd_confusion", int(N), int(C), _p(logits), int(logits.stride(0)), _p(y), _p(cm), _stream())
    return cm


def summary_from_confusion(cm):
    """(accuracy, macro precision, macro recall, macro F1) from the [C, C] integer matrix on the host -- what
    `precision_score / recall_score / f1_score(average="macro")` return (a class without predictions / samples counts 0, sklearn's
    zero_division default)."""
    cm = np.asarray(cm, dtype=np.float64)
    tp = np.diag(cm)
    pred, true = cm.sum(0), cm.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = np.where(pred > 0, tp / pred, 0.0)
        rec = np.where(true > 0, tp / true, 0.0)
        f1 = np.where(prec + rec > 0, 2 * prec * rec / (prec + rec), 0.0)
    total = cm.sum()
    return (float(tp.sum() / total) if total else float("nan")), float(prec.mean()), float(rec.mean()), float(f1.mean())
