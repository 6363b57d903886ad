"""GPU: rd_rank_bootstrap / _summary / _counts (raindrop_amd/csrc/rd_metrics_boot.hip) against the numpy restatement
(tests/bootstrap_ref.py) -- multiplicities, numerators and positives EXACT, AUROC the exact quotient with NaNs in the same places,
AUPRC and the summary within the 1e-10 of tests/test_metrics_gpu.py -- with NaN-filled, guarded outputs and workspace; run-to-run
and captured-replay bits; the launch log; rd_rank_metrics untouched; `feed.validate(bootstrap=)` and `fit(bootstrap=)`."""
import ctypes
import functools
import gc

import numpy as np
import pytest
import torch

from raindrop_amd import _lib, feed, metrics, synth
from tests import bootstrap_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENT = -77
KERNELS = {"k_boot_sort", "k_boot_stats", "k_boot_means", "k_boot_summary"}


@pytest.fixture(scope="module", autouse=True)
def _hand_back_device_memory():
    """tests/test_step_launches_gpu.py names buffers by the order in which their addresses first appear: leave no garbage behind."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(scores, y, reference) of a case, computed once and shared (nothing writes into them)."""
    case = next(c for c in B.CASES if c[0] == name)
    s, y = B.make_case(*case)
    ref = B.bootstrap_ref(s, y, case[3], B.SEED)
    for a in (s, y) + tuple(ref.values()):
        a.setflags(write=False)
    return s, y, ref


def _logged(fn):
    lib = _lib.load()
    on, read = lib.rd_debug_launch_log, lib.rd_debug_launch_log_read
    on.argtypes, on.restype = [ctypes.c_int], None
    read.argtypes, read.restype = [ctypes.c_char_p, ctypes.c_size_t], ctypes.c_size_t
    buf = ctypes.create_string_buffer(1 << 12)
    on(1)
    try:
        fn()
        n = read(buf, len(buf))
    finally:
        on(0)
    return set(buf.raw[:n].decode().split())


def _wide(s, y, extra=3):
    """the scores as the first C columns of a wider NaN matrix (ld = C + extra > C), and the labels"""
    N, C = s.shape
    wide = torch.full((N, C + extra), float("nan"), device=DEV)
    wide[:, :C] = torch.from_numpy(np.array(s)).to(DEV)
    return wide[:, :C], torch.from_numpy(np.array(y)).to(DEV)


class _Outs:
    """rank_bootstrap's `out=` and workspace: NaN / a sentinel / 0xFF everywhere, GUARD more elements behind each"""

    def __init__(self, N, C, R):
        shapes = dict(auroc_boot=((R, C), torch.float64), auprc_boot=((R, C), torch.float64), auroc_num_boot=((R, C), torch.int64),
                      pos_boot=((R, C), torch.int64), mean_boot=((R, 2), torch.float64), summary=((2, C + 1, 5), torch.float64))
        self.whole, self.out, self.n = {}, {}, {}
        for k, (shape, dt) in shapes.items():
            n = int(np.prod(shape))
            self.whole[k] = torch.full((n + GUARD,), float("nan") if dt == torch.float64 else SENT, dtype=dt, device=DEV)
            self.out[k], self.n[k] = self.whole[k][:n].view(shape), n
        self.need = int(_lib.load().rd_rank_bootstrap_workspace_bytes(N, C, R))
        assert self.need == 2 * N * C
        self.ws_whole = torch.full((self.need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        self.ws = self.ws_whole[:self.need]

    def guards_intact(self):
        ok = bool((self.ws_whole[self.need:] == 0xFF).all())
        for k, w in self.whole.items():
            g = w[self.n[k]:]
            ok = ok and bool(torch.isnan(g).all() if w.dtype == torch.float64 else (g == SENT).all())
        return ok

    def host(self):
        o = {k: v.cpu().numpy() for k, v in self.out.items()}
        return {"auroc": o["auroc_boot"], "auprc": o["auprc_boot"], "num": o["auroc_num_boot"], "pos": o["pos_boot"],
                "mean": o["mean_boot"], "summary": o["summary"]}


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in a)


def _counts(N, R, seed, r0, nr):
    whole = torch.full((nr * N + GUARD,), SENT, dtype=torch.int32, device=DEV)
    _lib.call("rd_rank_bootstrap_counts", N, R, seed, r0, nr, ctypes.c_void_p(whole.data_ptr()),
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert bool((whole[nr * N:] == SENT).all())
    return whole[:nr * N].view(nr, N).cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("case", B.CASES, ids=[c[0] for c in B.CASES])
def test_bootstrap_equals_the_restatement(case):
    name, N, C, R = case[:4]
    s, y, ref = _case(name)
    sd, yd = _wide(s, y)
    before = {k: v.cpu().numpy() for k, v in metrics.rank_metrics(sd, yd).items()}
    # the multiplicities: the first and the last rows of the R
    names = set()
    for r0, nr in ((0, min(R, 4)), (max(R - 4, 0), R - max(R - 4, 0))):
        names |= _logged(lambda: np.testing.assert_array_equal(_counts(N, R, B.SEED, r0, nr), ref["counts"][r0:r0 + nr]))
    assert "k_boot_counts" in names
    o = _Outs(N, C, R)
    names = _logged(lambda: metrics.rank_bootstrap(sd, yd, n_boot=R, seed=B.SEED, alpha=0.05, out=o.out, workspace=o.ws))
    assert KERNELS <= names, names
    got = o.host()
    with np.errstate(invalid="ignore"):
        print(name, "max |auprc - ref|", np.abs(got["auprc"] - ref["auprc"]).max(), "max |summary - ref|",
              np.nanmax(np.abs(got["summary"] - ref["summary"]), initial=0.0), "NaN AUROC resamples", int(np.isnan(got["auroc"]).sum()))
    assert B.disagreements(got, ref, N) == []
    assert o.guards_intact()
    # a second call into fresh buffers: the same bits; another seed: other resamples
    o2 = _Outs(N, C, R)
    r2 = metrics.rank_bootstrap(sd, yd, n_boot=R, seed=B.SEED, alpha=0.05, out=o2.out, workspace=o2.ws)
    assert _same_bits(o2.host(), got) and o2.guards_intact()
    assert torch.equal(r2["summary"], o2.out["summary"])
    if N > 3 and case[4] != "single_class":                     # (a single class: every resample has the same, empty, statistics)
        o3 = _Outs(N, C, R)
        metrics.rank_bootstrap(sd, yd, n_boot=R, seed=B.SEED + 1, alpha=0.05, out=o3.out, workspace=o3.ws)
        assert not np.array_equal(o3.host()["num"], got["num"])
    # the plain call's views and rd_rank_metrics next to it
    r = metrics.rank_bootstrap(sd, yd, n_boot=R, seed=B.SEED)
    assert r["auroc_ci"].shape == (C, 2) and r["auprc_macro_ci"].shape == (2,) and r["auroc_se"].shape == (C + 1,) and r["n_valid"].shape == (2, C + 1)
    assert np.array_equal(r["summary"].cpu().numpy().view(np.int64), got["summary"].view(np.int64))
    assert np.array_equal(r["auprc_ci"].cpu().numpy().view(np.int64), got["summary"][1, :C, 3:].view(np.int64))
    after = {k: v.cpu().numpy() for k, v in metrics.rank_metrics(sd, yd).items()}
    assert all(np.array_equal(before[k].view(np.int64), after[k].view(np.int64)) for k in before)


def test_envelope_ends_are_refused():
    s = torch.zeros((16385, 2), device=DEV)
    y = torch.zeros(16385, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.RaindropHipError, match="RD_EUNSUPPORTED"):
        metrics.rank_bootstrap(s, y, n_boot=8)
    with pytest.raises(_lib.RaindropHipError, match="RD_EUNSUPPORTED"):
        metrics.rank_bootstrap(s[:100], y[:100], n_boot=4097)
    with pytest.raises(_lib.RaindropHipError, match="RD_EUNSUPPORTED"):
        metrics.rank_bootstrap(s[:100], y[:100], n_boot=0)
    with pytest.raises(_lib.RaindropHipError, match="out="):
        metrics.rank_bootstrap(s[:100], y[:100], n_boot=8, out=metrics.rank_bootstrap(s[:100], y[:100], n_boot=4))


def test_captured_bootstrap_follows_new_scores():
    """rank_bootstrap inside torch.cuda.graph: a replay on new scores in the same buffers gives the new scores' values, and the bits
    of the eager call."""
    N, C, R = 1025, 2, 64
    rng = np.random.default_rng(N)
    s_buf = torch.zeros((N, C), device=DEV)
    y_buf = torch.zeros((N,), dtype=torch.int64, device=DEV)
    ws = metrics.bootstrap_workspace(N, C, R, DEV)
    out = metrics.rank_bootstrap(s_buf, y_buf, n_boot=R, seed=9, workspace=ws)             # lazy initialisations outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        metrics.rank_bootstrap(s_buf, y_buf, n_boot=R, seed=9, out=out, workspace=ws)
    for k in range(2):
        s = np.floor(rng.random((N, C)) * 50).astype(np.float32) / 50
        y = rng.integers(0, C, N).astype(np.int64)
        s_buf.copy_(torch.from_numpy(s)); y_buf.copy_(torch.from_numpy(y))
        g.replay()
        got = {"auroc": out["auroc_boot"], "auprc": out["auprc_boot"], "num": out["auroc_num_boot"], "pos": out["pos_boot"],
               "mean": out["mean_boot"], "summary": out["summary"]}
        got = {k: v.cpu().numpy() for k, v in got.items()}
        assert B.disagreements(got, B.bootstrap_ref(s, y, R, 9), N) == []
        eager = metrics.rank_bootstrap(s_buf, y_buf, n_boot=R, seed=9)
        assert np.array_equal(eager["summary"].cpu().numpy().view(np.int64), got["summary"].view(np.int64))
        assert np.array_equal(eager["auprc_boot"].cpu().numpy().view(np.int64), got["auprc"].view(np.int64))


def _tiny(beta, N=48, seed=82):
    from tests.helpers import build_ours
    cfg = synth.make_config("TINY")
    data = synth.make_batch(cfg, N, seed=seed)
    y = (data["src"][:, :, 0].sum(0).numpy() > 0).astype(np.int64)
    ds = feed.DeviceDataset(data["src"], data["times"], data["static"], torch.from_numpy(y), device=DEV)
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 21, **(dict(use_beta=True) if beta else {}))
    return cfg, ds, m


OLD_KEYS = {"auroc", "auprc", "loss", "accuracy", "precision", "recall", "f1", "auroc_per_class", "auprc_per_class", "confusion"}
NEW_KEYS = {"auroc_ci", "auprc_ci", "auroc_se", "auprc_se", "bootstrap_valid"}


def _equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


@pytest.mark.parametrize("beta", [False, True], ids=["default", "use_beta"])
def test_validate_with_bootstrap_is_rank_bootstrap_on_the_same_logits(beta):
    """the interval brackets nothing by assertion (that is statistics): it is rank_bootstrap's on the same scores, bit for bit, and
    without the keyword the result is what it was"""
    _, ds, m = _tiny(beta)
    v0 = feed.validate(m, ds)
    scores = torch.sigmoid(feed.evaluate_captured(m, ds)).contiguous()
    plain = metrics.rank_metrics(scores, ds.y)
    assert set(v0) == OLD_KEYS
    assert _equal(v0["auroc_per_class"], plain["auroc_per_class"].cpu().numpy()) and _equal(v0["auroc"], plain["auroc_per_class"][1].item())
    names = _logged(lambda: feed.validate(m, ds))
    assert not any(n.startswith("k_boot") for n in names)
    v = feed.validate(m, ds, bootstrap=64, bootstrap_seed=5, ci=0.9)
    assert set(v) == OLD_KEYS | NEW_KEYS
    assert all(_equal(v[k], v0[k]) for k in OLD_KEYS)
    b = metrics.rank_bootstrap(scores, ds.y, n_boot=64, seed=5, alpha=1.0 - 0.9)
    s = b["summary"].cpu().numpy()
    print("auroc", v["auroc"], v["auroc_ci"], "auprc", v["auprc"], v["auprc_ci"], "valid", v["bootstrap_valid"])
    assert _equal(v["auroc_ci"], s[0, 1, 3:]) and _equal(v["auprc_ci"], s[1, 1, 3:])
    assert _equal([v["auroc_se"], v["auprc_se"]], s[:, 1, 2]) and v["bootstrap_valid"] == int(s[0, 1, 0])
    assert isinstance(v["auroc_ci"], tuple) and v["auroc_ci"][0] <= v["auroc_ci"][1]
    assert not _equal(feed.validate(m, ds, bootstrap=64, bootstrap_seed=6, ci=0.9)["auroc_ci"], v["auroc_ci"])


def test_fit_with_bootstrap_reports_the_best_weights_interval():
    from raindrop_amd import trainer
    from tests.helpers import build_ours
    cfg, vds, _ = _tiny(False)
    _, ds, _ = _tiny(False, N=64, seed=81)
    np.random.seed(0)
    m = build_ours(cfg, synth.make_structure(cfg, "ones"), DEV, 3)
    r = trainer.fit(m, ds, vds, 1, batch_size=16, strategy=2, lr=1e-3, scheduler=False, autotune=False, bootstrap=32, bootstrap_seed=4)
    v = feed.validate(m, vds, bootstrap=32, bootstrap_seed=4)
    assert set(r["val_ci"]) == {"auroc", "auprc"} | NEW_KEYS
    assert all(_equal(r["val_ci"][k], v[k]) for k in r["val_ci"])
    if r["best_epoch"] is not None:
        assert r["val_ci"]["auroc"] == r["best_auroc"]
    np.random.seed(0)
    m2 = build_ours(cfg, synth.make_structure(cfg, "ones"), DEV, 3)
    r2 = trainer.fit(m2, ds, vds, 1, batch_size=16, strategy=2, lr=1e-3, scheduler=False, autotune=False)
    assert "val_ci" not in r2 and r2["val_auroc"] == r["val_auroc"] and r2["train_loss"] == r["train_loss"]
