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
    f = fit_temperature(logits, y)                  # f["temperature"]: the T that minimises the NLL of softmax(logits / T)
    k = calibration(logits, y, n_bins=15, temperature=f["result"])     # k["ece"], k["table"] [15, 3]: the reliability diagram
                                                    # (raindrop_amd/csrc/rd_metrics_calib.hip; C <= 64, n_bins <= 256)
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


CALIB_C_MAX, CALIB_M_MAX, FIT_N_MAX = 64, 256, 16384       # rd_calibration's / rd_fit_temperature's envelope (include/raindrop_hip.h)


def calibration_workspace(N, C, n_bins, device):
    """Workspace tensor `calibration` needs for [N, C] logits and `n_bins` bins (the workgroups' per-bin partials)."""
    n = int(_lib.load().rd_calibration_workspace_bytes(int(N), int(C), int(n_bins)))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device)


def calibration(logits, y, n_bins=15, temperature=None, column=None, out=None, workspace=None):
    """Reliability statistics of p = softmax(logits / T) (float64 on the device; include/raindrop_hip.h "Calibration" states the bin
    rule -- `n_bins` equal-width bins closed on the right -- and both Brier definitions).  column=None: top-label mode, confidence =
    max_c p against (argmax == y); column=c: one-vs-rest, confidence = p[:, c] against (y == c).  `temperature`: None (T = 1), a
    Python float (uploaded, no sync) or a float64 device tensor whose element 0 is read -- `fit_temperature(...)["result"]` as it is.
    2 <= C <= 64, n_bins <= 256, N < 2^24; there is no CPU fallback.  Returns a dict of device tensors:

        counts      [n_bins, 2] int64    rows and hits of every bin, exact
        table       [n_bins, 3] float64  rows, mean confidence, hit rate (NaN, NaN for an empty bin)
        summary     [6] float64          ECE, MCE (over the non-empty bins), Brier, NLL (of the full softmax), hit rate, mean confidence;
                                         the rest are 0-d views of it:
        ece, mce, brier, nll, accuracy, confidence

    `out`: the dict of a previous call, to write into the same tensors (captured use); `workspace`: from `calibration_workspace`."""
    _check(logits, y, "calibration")
    N, C = logits.shape
    M = int(n_bins)
    if N < 1:
        raise _lib.RaindropHipError("calibration: no samples")
    col = -1 if column is None else int(column)
    if column is not None and not 0 <= col < C:
        raise ValueError("calibration: column must be None (top-label) or a column of the logits, got %r" % (column,))
    dev = logits.device
    if temperature is None or torch.is_tensor(temperature):
        T = temperature
        if T is not None and (not T.is_cuda or T.dtype != torch.float64 or T.numel() < 1 or T.device != dev
                              or (T.dim() > 0 and not T.is_contiguous())):
            raise _lib.RaindropHipError("calibration: a temperature tensor must be float64 on the logits' device (element 0 is read)")
    else:
        if isinstance(temperature, bool) or not isinstance(temperature, (int, float, np.floating)) or not 0.0 < float(temperature) < float("inf"):
            raise ValueError("calibration: temperature must be None, a positive float or a float64 device tensor, got %r" % (temperature,))
        T = torch.tensor([float(temperature)], dtype=torch.float64, device=dev)
    if out is None:
        s = torch.empty(6, dtype=torch.float64, device=dev)
        out = {"counts": torch.empty((M, 2), dtype=torch.int64, device=dev), "table": torch.empty((M, 3), dtype=torch.float64, device=dev),
               "summary": s, "ece": s[0], "mce": s[1], "brier": s[2], "nll": s[3], "accuracy": s[4], "confidence": s[5]}
    elif tuple(out["counts"].shape) != (M, 2):
        raise _lib.RaindropHipError("calibration: out= holds %d bins, this call has %d" % (out["counts"].shape[0], M))
    ws = calibration_workspace(N, C, M, dev) if workspace is None else workspace
    _lib.call("rd_calibration", int(N), int(C), _p(logits), int(logits.stride(0)), _p(y), _p(T), col, M, _p(out["counts"]),
              _p(out["table"]), _p(out["summary"]), _p(ws), ws.numel(), _stream())
    return out


def fit_temperature(logits, y, out=None):
    """Temperature scaling (Guo et al., 2017): the scalar T that minimises the NLL of softmax(logits / T) against `y`, by a
    safeguarded Newton iteration in 1 / T run by one workgroup in one launch (include/raindrop_hip.h "rd_fit_temperature").  N <= 16384,
    2 <= C <= 64; there is no CPU fallback.  Returns a dict of device tensors:

        result      [8] float64: T, 1 / T, NLL at T = 1, NLL at T, evaluations, status, the gradient at the end, 0; the rest are
                    0-d views of it:
        temperature, nll_before, nll_after, iterations, status      status 0 interior minimum, 1 stopped at T = 0.01 (separable
                    rows), 2 stopped at T = 100, 3 evaluation cap, 4 non-finite gradient (T = 1 is written)

    `result` can be passed to `calibration(temperature=)` as it is: nothing reads it on the host.  `out`: the dict of a previous call."""
    _check(logits, y, "fit_temperature")
    N, C = logits.shape
    if N < 1:
        raise _lib.RaindropHipError("fit_temperature: no samples")
    if out is None:
        r = torch.empty(8, dtype=torch.float64, device=logits.device)
        out = {"result": r, "temperature": r[0], "nll_before": r[2], "nll_after": r[3], "iterations": r[4], "status": r[5]}
    _lib.call("rd_fit_temperature", int(N), int(C), _p(logits), int(logits.stride(0)), _p(y), _p(out["result"]), _stream())
    return out


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
