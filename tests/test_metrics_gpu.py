"""GPU: rd_rank_metrics / rd_confusion (raindrop_amd/csrc/rd_metrics.hip) against the values recorded from sklearn
(tests/golden/metrics_cases.npz) within 1e-10 absolute -- the bound tests/test_metrics_ref.py derives --, the exact integer AUROC
numerators against the numpy restatement, run-to-run and workspace-address invariance, and the captured form."""
import numpy as np
import pytest
import torch

from raindrop_amd import metrics
from tests import metrics_ref as R
from tests.test_metrics_ref import GOLD, TOL, _close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(s, y):
    return torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV)


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_rank_metrics_and_confusion_match_sklearn(case):
    name = case[0]
    s, y = R.make_case(*case[1:])
    with np.load(GOLD) as g:
        gold = {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(name + "/")}
    sd, yd = _dev(s, y)
    r = metrics.rank_metrics(sd, yd)
    got = {k: v.cpu().numpy() for k, v in r.items()}
    ref = R.rank_metrics_ref(s, y)
    print(name, "max |auroc - sklearn|", np.nanmax(np.abs(got["auroc_per_class"] - gold["auroc"]), initial=0.0),
          "max |auprc - sklearn|", np.abs(got["auprc_per_class"] - gold["auprc"]).max())
    assert _close(got["auroc_per_class"], gold["auroc"]), (got["auroc_per_class"], gold["auroc"])
    assert _close(got["auprc_per_class"], gold["auprc"]), (got["auprc_per_class"], gold["auprc"])
    assert _close(got["mean"], gold["macro"]) and _close([got["auroc"], got["auprc"]], gold["macro"])
    assert np.array_equal(got["auroc_num"], ref["num"])
    # a second call, and one through another workspace address: the same bits
    ws = metrics.rank_workspace(s.shape[0], s.shape[1], DEV)
    pad = torch.empty(ws.numel() + 4096, dtype=torch.uint8, device=DEV)
    for w in (None, pad[2048:]):
        r2 = metrics.rank_metrics(sd, yd, workspace=w)
        for k in ("auroc_per_class", "auprc_per_class", "mean"):
            assert np.array_equal(r2[k].cpu().numpy().view(np.int64), got[k].view(np.int64)), k
        assert torch.equal(r2["auroc_num"], r["auroc_num"])
    cm = metrics.confusion(sd, yd).cpu().numpy()
    assert np.array_equal(cm, gold["confusion"])
    assert np.abs(np.array(metrics.summary_from_confusion(cm)) - gold["summary"]).max() <= TOL


def test_strided_scores_and_signed_zero_ties():
    """Scores as columns of a wider matrix (row stride > C); -0.0 and +0.0 are one threshold (float equality), as in sklearn."""
    rng = np.random.default_rng(5)
    N = 300
    s = rng.choice(np.array([-0.0, 0.0, 0.5, -0.5], dtype=np.float32), size=(N, 2))
    y = rng.integers(0, 2, N).astype(np.int64)
    wide = torch.zeros((N, 7), device=DEV)
    wide[:, :2] = torch.from_numpy(s).to(DEV)
    r = metrics.rank_metrics(wide[:, :2], torch.from_numpy(y).to(DEV))
    ref = R.rank_metrics_ref(s, y)
    assert np.array_equal(r["auroc_num"].cpu().numpy(), ref["num"])
    assert np.abs(r["auprc_per_class"].cpu().numpy() - ref["auprc"]).max() <= TOL


@pytest.mark.parametrize("N", [3880, 20000])
def test_captured_metrics_follow_new_scores(N):
    """rank_metrics + confusion inside torch.cuda.graph: a replay on new scores in the same buffers gives the new scores' values."""
    rng = np.random.default_rng(N)
    C = 2
    s_buf = torch.zeros((N, C), device=DEV)
    y_buf = torch.zeros((N,), dtype=torch.int64, device=DEV)
    ws = metrics.rank_workspace(N, C, DEV)
    out = metrics.rank_metrics(s_buf, y_buf, workspace=ws)          # lazy initialisations happen outside the capture
    cm = metrics.confusion(s_buf, y_buf)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        metrics.rank_metrics(s_buf, y_buf, out=out, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(g):
        metrics.rank_metrics(s_buf, y_buf, out=out, workspace=ws)
        metrics.confusion(s_buf, y_buf, out=cm)
    for k in range(2):
        s = np.floor(rng.random((N, C)) * 50).astype(np.float32) / 50
        y = rng.integers(0, C, N).astype(np.int64)
        s_buf.copy_(torch.from_numpy(s)); y_buf.copy_(torch.from_numpy(y))
        g.replay()
        ref = R.rank_metrics_ref(s, y)
        assert np.array_equal(out["auroc_num"].cpu().numpy(), ref["num"])
        assert np.abs(out["auroc_per_class"].cpu().numpy() - ref["auroc"]).max() <= TOL
        assert np.abs(out["auprc_per_class"].cpu().numpy() - ref["auprc"]).max() <= TOL
        assert np.array_equal(cm.cpu().numpy(), R.confusion_ref(s, y))
