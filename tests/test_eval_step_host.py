"""CPU: the evaluation fast path has no CPU fallback, as everywhere else -- `EvalStep`, `evaluate_captured` and the device metrics
raise RaindropHipError on host tensors -- and its host-side pieces (the macro summary of a confusion matrix) need no device."""
import numpy as np
import pytest
import torch

from raindrop_amd import _lib, metrics, synth
from raindrop_amd.evalstep import EvalStep
from tests.helpers import build_ours


def _host_model_and_batch(**kw):
    cfg = synth.make_config("P19")
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), "cpu", 3, **kw)
    b = synth.make_batch(cfg, 4, seed=1)
    return m, {k: b[k] for k in ("src", "times", "lengths", "static")}


@pytest.mark.parametrize("kw", [{}, {"use_beta": True}], ids=["default", "use_beta"])
def test_eval_step_refuses_host_tensors(kw):
    m, batch = _host_model_and_batch(**kw)
    with pytest.raises(_lib.RaindropHipError):
        EvalStep(m, batch)
    with pytest.raises(_lib.RaindropHipError):
        EvalStep(m, {})


def test_metrics_refuse_host_tensors():
    s, y = torch.rand(8, 2), torch.randint(0, 2, (8,))
    with pytest.raises(_lib.RaindropHipError):
        metrics.rank_metrics(s, y)
    with pytest.raises(_lib.RaindropHipError):
        metrics.confusion(s, y)


def test_metric_entry_points_report_argument_errors_before_launch():
    lib = _lib.load()
    assert lib.rd_rank_metrics(0, 2, *([None] * 1), 2, *([None] * 6), 0, None) == -1 and b"bad dims" in lib.rd_last_error()
    assert lib.rd_rank_metrics(8, 2, None, 2, *([None] * 6), 0, None) == -1 and b"NULL" in lib.rd_last_error()
    assert lib.rd_confusion(8, 0, None, 2, None, None, None) == -1
    # N <= 16384 is sorted in one workgroup's LDS: no workspace; beyond, C columns of the padded power of two of 8-byte keys
    assert lib.rd_rank_metrics_workspace_bytes(16384, 8) == 0
    assert lib.rd_rank_metrics_workspace_bytes(16385, 8) == 8 * 32768 * 8
    assert lib.rd_rank_metrics_workspace_bytes(65536, 2) == 2 * 65536 * 8


def test_summary_from_confusion():
    cm = np.array([[5, 1, 0], [2, 3, 0], [0, 0, 0]])            # class 2: no samples, no predictions -> counts 0 in the macro means
    acc, prec, rec, f1 = metrics.summary_from_confusion(cm)
    assert acc == 8 / 11
    assert abs(prec - (5 / 7 + 3 / 4 + 0) / 3) < 1e-15 and abs(rec - (5 / 6 + 3 / 5 + 0) / 3) < 1e-15
    p, r = np.array([5 / 7, 3 / 4]), np.array([5 / 6, 3 / 5])
    assert abs(f1 - (2 * p * r / (p + r)).sum() / 3) < 1e-15
