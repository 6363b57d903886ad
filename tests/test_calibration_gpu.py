"""GPU: rd_calibration / rd_fit_temperature (raindrop_amd/csrc/rd_metrics_calib.hip) against the numpy restatement
(tests/calibration_ref.py) -- counts EXACT, the table's means and the six summaries to 1e-12 with NaN in the same places, the fitted T
to 1e-8 relative and both NLLs to 1e-12 -- with NaN-filled, guarded outputs and workspace; the exact-edge cases; both staging forms of
the fit, bit for bit; run-to-run and captured-replay bits; the refusals; `feed.validate(calibration=, temperature=)`, `validate_ema`
and `fit(calibrate=)`.  Measured errors (printed): profiles/calibration_errors.json."""
import ctypes
import functools
import gc

import numpy as np
import pytest
import torch

from raindrop_amd import _lib, feed, metrics, synth
from tests import calibration_ref as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENT = -77
CALIB_KERNELS = {"k_calib_rows", "k_calib_finish"}
FIT_LDS, FIT_GLOBAL = "k_fit_temperature<lds>", "k_fit_temperature<global>"


@pytest.fixture(scope="module", autouse=True)
def _hand_back_device_memory():
    """tests/test_step_launches_gpu.py names buffers by the order in which their addresses first appear: leave no garbage behind."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


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


def _wide(lg, y, extra=K.LD_EXTRA):
    """the logits as the first C columns of a wider NaN matrix (ld = C + extra > C), and the labels"""
    N, C = lg.shape
    wide = torch.full((N, C + extra), float("nan"), device=DEV)
    wide[:, :C] = torch.from_numpy(np.array(lg)).to(DEV)
    return wide[:, :C], torch.from_numpy(np.array(y)).to(DEV)


class _Outs:
    """calibration's `out=` and workspace: NaN / a sentinel / 0xFF everywhere, GUARD more elements behind each"""

    def __init__(self, N, C, M):
        shapes = dict(counts=((M, 2), torch.int64), table=((M, 3), torch.float64), summary=((6,), torch.float64))
        self.whole, self.out, self.n = {}, {}, {}
        for k, (shape, dt) in shapes.items():
            n = int(np.prod(shape))
            self.whole[k] = torch.full((n + GUARD,), float("nan") if dt == torch.float64 else SENT, dtype=dt, device=DEV)
            self.out[k], self.n[k] = self.whole[k][:n].view(shape), n
        self.need = int(_lib.load().rd_calibration_workspace_bytes(N, C, M))
        per = 256 * -(-(-(-N // 256)) // 1024)               # rows per workgroup: whole 256-row chunks, at most 1024 workgroups
        assert self.need == -(-N // per) * (M * 24 + 16)     # a function of N and M alone
        self.ws_whole = torch.full((self.need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        self.ws = self.ws_whole[:self.need]

    def guards_intact(self):
        ok = bool((self.ws_whole[self.need:] == 0xFF).all())
        for k, w in self.whole.items():
            g = w[self.n[k]:]
            ok = ok and bool(torch.isnan(g).all() if w.dtype == torch.float64 else (g == SENT).all())
        return ok

    def untouched(self):
        return self.guards_intact() and bool((self.ws == 0xFF).all()) and bool(torch.isnan(self.out["table"]).all()) \
            and bool(torch.isnan(self.out["summary"]).all()) and bool((self.out["counts"] == SENT).all())

    def host(self):
        return {k: v.cpu().numpy() for k, v in self.out.items()}


def _fit_out():
    whole = torch.full((8 + GUARD,), float("nan"), dtype=torch.float64, device=DEV)
    r = whole[:8]
    return whole, {"result": r, "temperature": r[0], "nll_before": r[2], "nll_after": r[3], "iterations": r[4], "status": r[5]}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("counts", "table", "summary"))


@functools.lru_cache(maxsize=None)
def _case(name):
    lg, y = K.make_case(name)
    lg.setflags(write=False); y.setflags(write=False)
    return lg, y


@pytest.mark.parametrize("case", K.CASES, ids=[c[0] for c in K.CASES])
def test_calibration_equals_the_restatement(case):
    name, N, C, M, column, T = case[:6]
    lg, y = _case(name)
    ld, yd = _wide(lg, y)
    if T == "fit":                                         # the fit's result tensor feeds the call; the reference takes the T it holds
        fit = metrics.fit_temperature(ld, yd)
        assert K.fit_disagreements(fit["result"].cpu().numpy(), K.fit_ref(lg, y)) == []
        t_arg, t_ref = fit["result"], float(fit["temperature"])
    else:
        t_arg, t_ref = T, T
    ref = K.calibration_ref(lg, y, M, t_ref, column)
    o = _Outs(N, C, M)
    names = _logged(lambda: metrics.calibration(ld, yd, n_bins=M, temperature=t_arg, column=column, out=o.out, workspace=o.ws))
    assert names == CALIB_KERNELS, names
    got = o.host()
    print(name, "max |table - ref|, |summary - ref|", K.errors(got, ref), "empty bins", int((got["counts"][:, 0] == 0).sum()))
    assert K.disagreements(got, ref) == []
    assert o.guards_intact()
    # a second call into fresh buffers: the same bits; the plain call's views
    o2 = _Outs(N, C, M)
    metrics.calibration(ld, yd, n_bins=M, temperature=t_arg, column=column, out=o2.out, workspace=o2.ws)
    assert _same_bits(o2.host(), got) and o2.guards_intact()
    r = metrics.calibration(ld, yd, n_bins=M, temperature=t_arg, column=column)
    assert _same_bits({k: r[k].cpu().numpy() for k in ("counts", "table", "summary")}, got)
    views = [r[k].item() for k in ("ece", "mce", "brier", "nll", "accuracy", "confidence")]
    assert np.array_equal(_bits(np.array(views)), _bits(got["summary"]))
    if T == "fit":                                         # chaining: the tensor and the float it holds give the same bits
        r2 = metrics.calibration(ld, yd, n_bins=M, temperature=t_ref, column=column)
        assert _same_bits({k: r2[k].cpu().numpy() for k in ("counts", "table", "summary")}, got)


@pytest.mark.parametrize("name", sorted(K.edge_cases()))
def test_exact_edges_and_empty_bins(name):
    lg, y, M, column, T = K.edge_cases()[name]
    N, C = lg.shape
    ref = K.calibration_ref(lg, y, M, T, column)
    ld, yd = _wide(lg, y)
    o = _Outs(N, C, M)
    metrics.calibration(ld, yd, n_bins=M, temperature=T, column=column, out=o.out, workspace=o.ws)
    got = o.host()
    print(name, K.errors(got, ref), got["counts"][:, 0].tolist())
    assert K.disagreements(got, ref) == [] and o.guards_intact()
    if name == "half":
        assert got["counts"][4].tolist() == [70, 46] and got["table"][4, 1] == 0.5
    if name == "one":
        assert got["counts"][14].tolist() == [130, 104] and got["table"][14, 1] == 1.0
    if name == "one_bin":
        assert got["counts"][6, 0] == 300 and np.isnan(got["table"][[0, 5, 7, 9], 1:]).all() and got["summary"][1] == got["summary"][0]
    if name == "bad_label":
        assert np.isnan(got["summary"][2:4]).all() and got["counts"][:, 0].sum() == 200


@pytest.mark.parametrize("name", [c[0] for c in K.FIT_CASES])
def test_fit_equals_the_restatement(name):
    _, N, C, kind = next(c for c in K.FIT_CASES if c[0] == name)
    lg, y = K.make_fit_case(name)
    ref = K.fit_ref(lg, y)
    ld, yd = _wide(lg, y)
    bits = ctypes.c_uint32(0)
    assert _lib.load().rd_debug_calibration_route(N, C, ctypes.byref(bits)) == 0
    staged = bool(bits.value & 1)
    assert staged == (N * C * 4 <= K.FIT_LDS_BYTES)
    whole, out = _fit_out()
    names = _logged(lambda: metrics.fit_temperature(ld, yd, out=out))
    assert names == {FIT_LDS if staged else FIT_GLOBAL}, names
    r = out["result"].cpu().numpy()
    print(name, "T", r[0], "ref", ref["T"], "rel", abs(r[0] - ref["T"]) / ref["T"], "nll", r[2], r[3], "d nll", r[2] - ref["nll_before"],
          r[3] - ref["nll_after"], "evaluations", r[4], "status", r[5], "g", r[6], "staged", staged)
    assert K.fit_disagreements(r, ref) == []
    assert bool(torch.isnan(whole[8:]).all())
    if kind == "separable":
        assert r[5] == 1 and r[0] == 1e-2
    if kind == "worst":
        assert r[5] == 2 and r[0] == 1e2
    if kind == "constant":
        assert r[5] == 0 and r[0] == 1.0 and r[4] == 1
    if kind == "nan":
        assert r[5] == 4 and r[0] == 1.0 and r[1] == 1.0
    if name in K.INTERIOR:
        assert r[5] == 0 and (r[0] > 1.0) == (kind == "over") and abs(r[6]) < 1e-9 and r[4] < 60
    # a second call: the same bits; and, where the default stages, the form that re-reads global memory: the same bits again
    _, out2 = _fit_out()
    metrics.fit_temperature(ld, yd, out=out2)
    assert np.array_equal(_bits(out2["result"].cpu().numpy()), _bits(r))
    if staged:
        lib = _lib.load()
        lib.rd_debug_set_calibration_stage(0)
        try:
            assert lib.rd_debug_calibration_route(N, C, ctypes.byref(bits)) == 0 and bits.value == 0
            _, out3 = _fit_out()
            names = _logged(lambda: metrics.fit_temperature(ld, yd, out=out3))
        finally:
            lib.rd_debug_set_calibration_stage(1)
        assert names == {FIT_GLOBAL}
        assert np.array_equal(_bits(out3["result"].cpu().numpy()), _bits(r))


def test_captured_calibration_and_fit_follow_new_logits():
    """fit_temperature -> calibration inside torch.cuda.graph, the fit's tensor feeding the statistics: a replay on new logits in the
    same buffers gives the new logits' values, twice the same bits, and the bits of the eager calls"""
    N, C, M = 1025, 3, 15
    l_buf = torch.zeros((N, C), device=DEV)
    y_buf = torch.zeros((N,), dtype=torch.int64, device=DEV)
    ws = metrics.calibration_workspace(N, C, M, DEV)
    fit = metrics.fit_temperature(l_buf, y_buf)            # lazy initialisations outside the capture
    out = metrics.calibration(l_buf, y_buf, n_bins=M, temperature=fit["result"], workspace=ws)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        metrics.fit_temperature(l_buf, y_buf, out=fit)
        metrics.calibration(l_buf, y_buf, n_bins=M, temperature=fit["result"], out=out, workspace=ws)
    for k in range(2):
        lg, y = K.make_logits(900 + k, N, C, 2.0 + k)
        l_buf.copy_(torch.from_numpy(lg)); y_buf.copy_(torch.from_numpy(y))
        g.replay()
        got = {key: out[key].cpu().numpy() for key in ("counts", "table", "summary")}
        r = fit["result"].cpu().numpy()
        assert K.fit_disagreements(r, K.fit_ref(lg, y)) == []
        assert K.disagreements(got, K.calibration_ref(lg, y, M, float(r[0]), None)) == []
        g.replay()
        assert _same_bits({key: out[key].cpu().numpy() for key in got}, got) and np.array_equal(_bits(fit["result"].cpu().numpy()), _bits(r))
        ef = metrics.fit_temperature(l_buf, y_buf)
        eager = metrics.calibration(l_buf, y_buf, n_bins=M, temperature=ef["result"])
        assert np.array_equal(_bits(ef["result"].cpu().numpy()), _bits(r))
        assert _same_bits({key: eager[key].cpu().numpy() for key in got}, got)


def test_envelope_ends_are_refused_and_leave_the_outputs_alone():
    y = torch.zeros(16385, dtype=torch.int64, device=DEV)
    whole, out = _fit_out()
    with pytest.raises(_lib.RaindropHipError, match="RD_EUNSUPPORTED"):
        metrics.fit_temperature(torch.zeros((16385, 2), device=DEV), y, out=out)
    for C in (1, 65):
        with pytest.raises(_lib.RaindropHipError, match="RD_EUNSUPPORTED"):
            metrics.fit_temperature(torch.zeros((100, C), device=DEV), y[:100], out=out)
    assert bool(torch.isnan(whole).all())
    for C, M in ((1, 15), (65, 15), (2, 257), (2, 0)):
        o = _Outs(100, 2, 15)
        with pytest.raises(_lib.RaindropHipError, match="RD_EUNSUPPORTED"):
            _lib.call("rd_calibration", 100, C, ctypes.c_void_p(torch.zeros((100, C), device=DEV).data_ptr()), C, ctypes.c_void_p(y.data_ptr()),
                      None, -1, M, *(ctypes.c_void_p(o.out[k].data_ptr()) for k in ("counts", "table", "summary")),
                      ctypes.c_void_p(o.ws.data_ptr()), o.ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert o.untouched()
    with pytest.raises(_lib.RaindropHipError, match="RD_EUNSUPPORTED"):
        metrics.calibration(torch.zeros((100, 2), device=DEV), y[:100], n_bins=257)
    with pytest.raises(_lib.RaindropHipError, match="out="):
        z = torch.zeros((100, 2), device=DEV)
        metrics.calibration(z, y[:100], n_bins=8, out=metrics.calibration(z, y[:100], n_bins=4))


# ---- validate / validate_ema / fit ----
def _tiny(N=48, seed=82):
    from tests.helpers import build_ours
    cfg = synth.make_config("TINY")
    data = synth.make_batch(cfg, N, seed=seed)
    y = (data["src"][:, :, 0].sum(0).numpy() > 0).astype(np.int64)
    ds = feed.DeviceDataset(data["src"], data["times"], data["static"], torch.from_numpy(y), device=DEV)
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 21)
    return cfg, ds, m


OLD_KEYS = {"auroc", "auprc", "loss", "accuracy", "precision", "recall", "f1", "auroc_per_class", "auprc_per_class", "confusion"}
BOOT_KEYS = {"auroc_ci", "auprc_ci", "auroc_se", "auprc_se", "bootstrap_valid"}
CAL_KEYS = {"ece", "mce", "brier", "nll", "reliability", "reliability_counts"}
FIT_KEYS = {"temperature", "temperature_status", "ece_uncalibrated", "nll_uncalibrated"}
# what a second feed.validate(model, ds) on this model launched before the calibration existed, outside its graph replays (recorded
# from the parent commit's library on an MI355X; the same names in the fp32, bf16x3 and bf16 modes)
VALIDATE_LAUNCHES_BEFORE = ("k_confusion", "k_rank_means", "k_rank_sort<fused>", "k_softmax_xent")


def _equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def test_validate_with_calibration_is_metrics_calibration_on_the_same_logits():
    _, ds, m = _tiny()
    v0 = feed.validate(m, ds)
    assert set(v0) == OLD_KEYS
    names = _logged(lambda: feed.validate(m, ds))
    assert not any(n.startswith(("k_calib", "k_fit")) for n in names), names
    print("validate launches", sorted(names))
    assert names == set(VALIDATE_LAUNCHES_BEFORE)
    logits = feed.evaluate_captured(m, ds)
    for transform in ("sigmoid", "softmax"):
        v1 = feed.validate(m, ds, transform=transform)
        # T = 1, a float, the fit: always of softmax(logits / T), column 1 of the binary task, whatever the transform
        v = feed.validate(m, ds, transform=transform, calibration=10)
        assert set(v) == OLD_KEYS | CAL_KEYS and all(_equal(v[k], v1[k]) for k in OLD_KEYS)
        k = metrics.calibration(logits, ds.y, n_bins=10, column=1)
        assert _equal([v["ece"], v["mce"], v["brier"], v["nll"]], k["summary"][:4].cpu().numpy())
        assert _equal(v["reliability"], k["table"].cpu().numpy()) and v["reliability"].shape == (10, 3)
        assert np.array_equal(v["reliability_counts"], k["counts"].cpu().numpy()) and v["reliability_counts"].dtype == np.int64
        v = feed.validate(m, ds, transform=transform, calibration=15, temperature=2.5)
        k = metrics.calibration(logits, ds.y, n_bins=15, column=1, temperature=2.5)
        assert set(v) == OLD_KEYS | CAL_KEYS and _equal([v["ece"], v["mce"], v["brier"], v["nll"]], k["summary"][:4].cpu().numpy())
        v = feed.validate(m, ds, transform=transform, calibration=15, temperature="fit", bootstrap=16, bootstrap_seed=3)
        assert set(v) == OLD_KEYS | BOOT_KEYS | CAL_KEYS | FIT_KEYS and all(_equal(v[k], v1[k]) for k in OLD_KEYS)
        vb = feed.validate(m, ds, transform=transform, bootstrap=16, bootstrap_seed=3)
        assert all(_equal(v[k], vb[k]) for k in BOOT_KEYS)
        f = metrics.fit_temperature(logits, ds.y)
        k = metrics.calibration(logits, ds.y, n_bins=15, column=1, temperature=f["result"])
        k1 = metrics.calibration(logits, ds.y, n_bins=15, column=1)
        assert _equal([v["ece"], v["mce"], v["brier"], v["nll"]], k["summary"][:4].cpu().numpy())
        assert _equal(v["reliability"], k["table"].cpu().numpy()) and np.array_equal(v["reliability_counts"], k["counts"].cpu().numpy())
        assert _equal(v["temperature"], f["temperature"].item()) and v["temperature_status"] == int(f["status"].item())
        assert _equal([v["ece_uncalibrated"], v["nll_uncalibrated"]], [k1["ece"].item(), k1["nll"].item()])
        print(transform, "T", v["temperature"], "status", v["temperature_status"], "ece", v["ece_uncalibrated"], "->", v["ece"],
              "nll", v["nll_uncalibrated"], "->", v["nll"])
        if v["temperature_status"] == 0:
            assert v["nll"] <= v["nll_uncalibrated"]


def test_validate_ema_passes_the_keywords_through(monkeypatch):
    import contextlib
    seen = {}

    def fake(model, ds, **kw):
        seen.update(kw)
        return "result"
    monkeypatch.setattr(feed, "validate", fake)
    opt = type("O", (), {"ema_weights": lambda self: contextlib.nullcontext()})()
    assert feed.validate_ema(None, None, opt, calibration=12, temperature="fit") == "result"
    assert seen == dict(calibration=12, temperature="fit")


def test_fit_with_calibrate_reports_the_best_weights_temperature():
    from raindrop_amd import trainer
    from tests.helpers import build_ours
    cfg, vds, _ = _tiny()
    _, ds, _ = _tiny(N=64, seed=81)
    np.random.seed(0)
    m = build_ours(cfg, synth.make_structure(cfg, "ones"), DEV, 3)
    r = trainer.fit(m, ds, vds, 1, batch_size=16, strategy=2, lr=1e-3, scheduler=False, autotune=False, calibrate=True, calibration_bins=10)
    v = feed.validate(m, vds, calibration=10, temperature="fit")
    assert set(r["val_calibration"]) == CAL_KEYS | FIT_KEYS == set(trainer.CALIBRATION_KEYS)
    assert all(_equal(r["val_calibration"][k], v[k]) for k in r["val_calibration"])
    assert _equal(r["temperature"], v["temperature"]) and r["val_calibration"]["reliability"].shape == (10, 3)
    np.random.seed(0)
    m2 = build_ours(cfg, synth.make_structure(cfg, "ones"), DEV, 3)
    r2 = trainer.fit(m2, ds, vds, 1, batch_size=16, strategy=2, lr=1e-3, scheduler=False, autotune=False)
    assert "val_calibration" not in r2 and "temperature" not in r2 and r2["val_auroc"] == r["val_auroc"] and r2["train_loss"] == r["train_loss"]
