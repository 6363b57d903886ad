"""CPU: the numpy restatement of the calibration statistics and the temperature fit (tests/calibration_ref.py) is a reference worth
comparing against -- its cases keep clear of what two correct implementations may round differently, and ten wrong statistics each
miss the bounds on some case -- and the host surface of the feature: header, binding, envelope refusals, keyword checks, the
staging route."""
import ctypes
import functools
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from raindrop_amd import _lib, feed, metrics, trainer
from tests import calibration_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _generic(name):
    """(logits, y, M, column, T as a float or None, reference) of a generic case; "fit" resolved by the reference's own minimiser"""
    _, N, C, M, column, T, _ = next(c for c in K.CASES if c[0] == name)
    lg, y = K.make_case(name)
    t = K.fit_ref(lg, y)["T"] if T == "fit" else T
    return lg, y, M, column, t, K.calibration_ref(lg, y, M, t, column)


def _all_cases():
    for c in K.CASES:
        if c[1] <= 5000:                                   # (the 262444-row case checks a kernel path, not the statistics)
            yield (c[0],) + _generic(c[0])
    for name, (lg, y, M, column, T) in K.edge_cases().items():
        yield name, lg, y, M, column, T, K.calibration_ref(lg, y, M, T, column)


@pytest.mark.parametrize("case", K.CASES, ids=[c[0] for c in K.CASES])
def test_generic_cases_keep_clear_of_the_bin_edges(case):
    name, N, C, M, column, T = case[:6]
    lg, y, _, _, t, ref = _generic(name)
    assert lg.shape == (N, C) and lg.dtype == np.float32 and y.shape == (N,)
    margin = K.EDGE_MARGIN_FIT if T == "fit" else K.EDGE_MARGIN
    d = K.edge_distance(ref["conf"], M)
    print(name, "nearest edge", d)
    assert d > margin
    assert ref["counts"][:, 0].sum() == N
    if T == "fit":                                         # a fitted T must be an interior one
        assert K.fit_ref(lg, y)["status"] == 0


def test_edge_cases_are_what_they_claim():
    e = K.edge_cases()
    ref = {k: K.calibration_ref(v[0], v[1], v[2], v[4], v[3]) for k, v in e.items()}
    assert np.all(ref["half"]["conf"] == 0.5) and ref["half"]["counts"][4, 0] == 70 and ref["half"]["counts"][:, 0].sum() == 70
    assert ref["half"]["counts"][4, 1] == 46                                # the argmax is column 0: the 46 rows labelled 0 hit
    assert np.all(ref["one"]["conf"] == 1.0) and ref["one"]["counts"][14, 0] == 130 and ref["one"]["counts"][14, 1] == 104
    c = ref["one_column"]["conf"]
    assert set(np.unique(c)) == {c.min(), 1.0} and 0.0 < c.min() < 1e-40
    assert ref["one_column"]["counts"][0, 0] + ref["one_column"]["counts"][14, 0] == 130
    t = ref["one_bin"]["table"]
    assert ref["one_bin"]["counts"][6, 0] == 300 and np.isnan(t[[0, 1, 2, 3, 4, 5, 7, 8, 9], 1:]).all() and not np.isnan(t[6]).any()
    assert ref["one_bin"]["summary"][1] == abs(t[6, 2] - t[6, 1]) == ref["one_bin"]["summary"][0]
    s = ref["bad_label"]["summary"]
    assert np.isnan(s[2]) and np.isnan(s[3]) and not np.isnan(s[[0, 1, 4, 5]]).any() and ref["bad_label"]["counts"][:, 0].sum() == 200


@pytest.mark.parametrize("variant", K.WRONG)
def test_a_wrong_statistic_misses_the_bound_somewhere(variant):
    """bins closed on the left; T ignored; T multiplied; the modes exchanged; Brier of the label's term alone; ECE as a plain mean of
    the gaps; MCE with the empty bins' 0 / 0 in it; empty bins written as (0, 0) -- a gap of 0 - 0, which no maximum can show, so it
    is the table that catches it; the last maximum; the NLL of the binned column (equal to the full one at C = 2: the C = 3 column
    cases catch it)"""
    caught = []
    for name, lg, y, M, column, T, ref in _all_cases():
        bad = K.disagreements(K.calibration_ref(lg, y, M, T, column, variant=variant), ref)
        if bad:
            caught.append((name, bad))
    print(variant, caught[:4])
    assert caught


def test_the_reference_agrees_with_itself_and_with_first_principles():
    for name, lg, y, M, column, T, ref in _all_cases():
        assert K.disagreements(K.calibration_ref(lg, y, M, T, column), ref) == []
    lg, y, M, column, T, ref = _generic("n1025_c2_col1_fit")
    p1 = K.softmax64(lg, T)[:, 1]
    assert abs(ref["summary"][2] - np.mean((p1 - (y == 1)) ** 2)) < 1e-15              # sklearn's brier_score_loss
    edges = np.linspace(0.0, 1.0, M + 1)
    idx = np.digitize(p1, edges, right=True) - 1                                      # edges[i] < x <= edges[i + 1]
    assert np.array_equal(np.bincount(idx, minlength=M), ref["counts"][:, 0])


@pytest.mark.parametrize("name", [c[0] for c in K.FIT_CASES])
def test_fit_cases_are_clear_cut(name):
    """an interior case has g changing sign strictly inside the bracket with h > 1e-3 at the root; every other one is far from the
    sign that would change its status"""
    lg, y = K.make_fit_case(name)
    ref = K.fit_ref(lg, y)
    kind = next(c[3] for c in K.FIT_CASES if c[0] == name)
    print(name, ref)
    if name in K.INTERIOR:
        glo, ghi = K.fit_terms(lg, y, K.BETA_LO)[0], K.fit_terms(lg, y, K.BETA_HI)[0]
        assert glo < -1e-6 and ghi > 1e-6 and ref["status"] == 0 and K.BETA_LO < ref["beta"] < K.BETA_HI
        assert K.fit_terms(lg, y, ref["beta"])[1] > 1e-3 and abs(ref["g"]) < 1e-10
        assert (ref["T"] > 1.0) == (kind == "over") and ref["nll_after"] < ref["nll_before"]
    elif kind == "separable":
        assert ref["status"] == 1 and ref["T"] == 1e-2 and ref["g"] < -1e-6
    elif kind == "worst":
        assert ref["status"] == 2 and ref["T"] == 1e2 and ref["g"] > 1e-6
    elif kind == "constant":
        assert ref["status"] == 0 and ref["T"] == 1.0 and ref["g"] == 0.0
    elif kind == "nan":
        assert ref["status"] == 4 and ref["T"] == 1.0
    else:
        assert ref["status"] in (0, 1, 2) and (ref["status"] == 0 or abs(ref["g"]) > 1e-6)


def test_the_reference_recovers_a_known_temperature():
    lg, y = K.make_fit_case("over_4096_c2")                # logits = 2.5 x (logits whose softmax generated the labels), N = 4096
    ref = K.fit_ref(lg, y)
    print("T", ref["T"])
    assert abs(ref["T"] - 2.5) <= 0.05 * 2.5


# ---- the host surface ----
NAMES = ("rd_calibration_workspace_bytes", "rd_calibration", "rd_fit_temperature")


def test_header_declares_the_functions_and_the_rules():
    text = open(os.path.join(ROOT, "include", "raindrop_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SIGNATURES
    for phrase in ("e_i < conf <= e_{i+1}", "brier_score_loss", "sum_c (p_nc - [y_n = c])^2", "result f64 [8]", "1 <= N < 2^24", "2 <= C <= 64",
                   "1 <= M <= 256", "1 <= N <= 16384", "Status.", "non-finite"):
        assert phrase in text, phrase
    dbg = open(os.path.join(ROOT, "include", "raindrop_hip_debug.h")).read()
    assert all(k in dbg for k in ("k_calib_rows", "k_calib_finish", "k_fit_temperature<lds>", "k_fit_temperature<global>",
                                  "rd_debug_calibration_route"))


def test_envelope_is_refused_without_a_device():
    lib = _lib.load()
    ws = lib.rd_calibration_workspace_bytes
    assert ws(3880, 2, 15) == 16 * (15 * 24 + 16) and ws(1, 2, 1) == 40 and ws(262444, 2, 15) == 513 * (15 * 24 + 16)
    assert ws((1 << 24) - 1, 64, 256) == 1024 * (256 * 24 + 16)
    for N, C, M in ((0, 2, 15), (1 << 24, 2, 15), (10, 1, 15), (10, 65, 15), (10, 2, 0), (10, 2, 257)):
        assert ws(N, C, M) == 0
        assert lib.rd_calibration(N, C, None, C, None, None, -1, M, None, None, None, None, 0, None) == -2, (N, C, M)
        assert b"outside" in lib.rd_last_error()
    assert lib.rd_calibration(10, 2, None, 2, None, None, -1, 15, None, None, None, None, 0, None) == -1 and b"NULL" in lib.rd_last_error()
    assert lib.rd_calibration(10, 2, None, 1, None, None, -1, 15, None, None, None, None, 0, None) == -1 and b"bad dims" in lib.rd_last_error()
    assert lib.rd_calibration(10, 2, None, 2, None, None, 2, 15, None, None, None, None, 0, None) == -1 and b"column" in lib.rd_last_error()
    assert lib.rd_calibration(10, 2, None, 2, None, None, -2, 15, None, None, None, None, 0, None) == -1
    for N, C in ((0, 2), (16385, 2), (10, 1), (10, 65)):
        assert lib.rd_fit_temperature(N, C, None, C, None, None, None) == -2 and b"outside" in lib.rd_last_error(), (N, C)
    assert lib.rd_fit_temperature(10, 2, None, 2, None, None, None) == -1 and b"NULL" in lib.rd_last_error()
    assert lib.rd_fit_temperature(10, 2, None, 1, None, None, None) == -1


def _route(N, C):
    bits = ctypes.c_uint32(0xFFFFFFFF)
    rc = _lib.load().rd_debug_calibration_route(N, C, ctypes.byref(bits))
    return rc, bits.value & 1, bits.value >> 8


def test_route_query_against_a_hand_table():
    """staged iff N C 4 <= 159 KiB = 162816 bytes: at C = 8 the last N that stages is 5088 (162816 bytes), 5089 (162848) does not"""
    table = [(1, 2, 1, 8), (3880, 2, 1, 31040), (3880, 8, 1, 124160), (5088, 8, 1, 162816), (5089, 8, 0, 0), (16384, 2, 1, 131072),
             (16384, 8, 0, 0), (1025, 64, 0, 0), (636, 64, 1, 162816), (637, 64, 0, 0), (16384, 64, 0, 0)]
    for N, C, stage, lds in table:
        assert _route(N, C) == (0, stage, lds), (N, C)
        assert stage == (N * C * 4 <= K.FIT_LDS_BYTES)
    for N, C in ((0, 2), (16385, 2), (10, 1), (10, 65)):
        assert _route(N, C) == (-2, 0, 0)
    lib = _lib.load()
    lib.rd_debug_set_calibration_stage(0)                  # the tests' switch: nothing stages, and the query says so
    try:
        assert _route(3880, 2) == (0, 0, 0)
    finally:
        lib.rd_debug_set_calibration_stage(1)
    assert _route(3880, 2) == (0, 1, 31040)


def test_metrics_functions_refuse_cpu_tensors_and_bad_arguments():
    p = inspect.signature(metrics.calibration).parameters
    assert [p[k].default for k in ("n_bins", "temperature", "column", "out", "workspace")] == [15, None, None, None, None]
    assert inspect.signature(metrics.fit_temperature).parameters["out"].default is None and callable(metrics.calibration_workspace)
    s, y = torch.zeros((5, 2)), torch.zeros(5, dtype=torch.int64)
    with pytest.raises(_lib.RaindropHipError, match="no CPU fallback"):
        metrics.calibration(s, y)
    with pytest.raises(_lib.RaindropHipError, match="no CPU fallback"):
        metrics.fit_temperature(s, y)
    with pytest.raises(_lib.RaindropHipError):
        metrics.calibration(s.numpy(), y)
    if torch.cuda.is_available():
        sd, yd = s.cuda(), y.cuda()
        for bad_s, bad_y in ((sd.double(), yd), (sd[:, 0], yd), (sd, yd[:4]), (sd, yd.int()), (sd.t(), yd)):
            with pytest.raises(_lib.RaindropHipError):
                metrics.calibration(bad_s, bad_y)
            with pytest.raises(_lib.RaindropHipError):
                metrics.fit_temperature(bad_s, bad_y)
        for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature="fit"), dict(temperature=True), dict(column=2), dict(column=-1)):
            with pytest.raises(ValueError):
                metrics.calibration(sd, yd, **kw)
        with pytest.raises(_lib.RaindropHipError, match="temperature tensor"):
            metrics.calibration(sd, yd, temperature=torch.ones(1, device="cuda"))


BAD = [dict(calibration=0), dict(calibration=257), dict(calibration=2.5), dict(calibration=True), dict(calibration="15"),
       dict(calibration=15, temperature=0.0), dict(calibration=15, temperature=-2.0), dict(calibration=15, temperature="best"),
       dict(calibration=15, temperature=float("inf")), dict(calibration=15, temperature=float("nan")), dict(calibration=15, temperature=True),
       dict(temperature=1.5), dict(temperature="fit")]


@pytest.mark.parametrize("kw", BAD, ids=str)
def test_validate_checks_the_keywords_before_anything_runs(kw):
    with pytest.raises(ValueError, match="calibration|temperature"):
        feed.validate(None, SimpleNamespace(y=None), **kw)
    with pytest.raises(ValueError, match="calibration|temperature"):
        feed.check_calibration(kw.get("calibration"), kw.get("temperature"))


def test_temperature_without_calibration_is_refused_by_name():
    with pytest.raises(ValueError, match="needs calibration"):
        feed.check_calibration(None, "fit")
    with pytest.raises(ValueError, match="needs calibration"):
        feed.validate(None, SimpleNamespace(y=None), temperature=2.0)


def test_validate_and_fit_accept_the_keywords():
    p = inspect.signature(feed.validate).parameters
    assert (p["calibration"].default, p["temperature"].default) == (None, None)
    feed.check_calibration(None)
    feed.check_calibration(1)
    feed.check_calibration(np.int64(256), "fit")
    feed.check_calibration(15, 2.5)
    feed.check_calibration(15, np.float64(0.5))
    with pytest.raises(_lib.RaindropHipError, match="labels"):            # good keywords: the next refusal is the old one
        feed.validate(None, SimpleNamespace(y=None), calibration=15, temperature="fit")
    assert any(q.kind is inspect.Parameter.VAR_KEYWORD for q in inspect.signature(feed.validate_ema).parameters.values())
    assert "optimistic" in feed.validate.__doc__
    p = inspect.signature(trainer.fit).parameters
    assert (p["calibrate"].default, p["calibration_bins"].default) == (False, 15)
    ds = SimpleNamespace(y=torch.zeros(4, dtype=torch.int64), N=4)
    trainer._check_fit_args(ds, ds, 1, 2, 2, calibrate=True, calibration_bins=10)
    trainer._check_fit_args(ds, ds, 1, 2, 2)
    for kw in (dict(calibrate=1), dict(calibrate="yes"), dict(calibrate=True, calibration_bins=0), dict(calibration_bins=257),
               dict(calibration_bins=None)):
        with pytest.raises(ValueError, match="calibrat"):
            trainer.fit(None, ds, ds, 1, batch_size=2, **kw)
