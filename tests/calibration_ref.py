"""numpy float64 restatement of rd_calibration and rd_fit_temperature (include/raindrop_hip.h "Calibration"), the case tables of
tests/test_calibration_ref_host.py / tests/test_calibration_gpu.py and their bounds.

Bounds.  Every reported sum is a mean of N terms of magnitude <= 2, each formed from at most C + 8 float64 operations, so the error
of either implementation is about N (C + 8) 2^-52 / N < 2e-14 at C = 64: TOL = 1e-12 absolute on ECE, MCE, Brier, NLL, hit rate, mean
confidence and the table's means leaves more than 100x; `counts` are exact.  The fit stops at a step or bracket of 1e-12 beta and
Newton is quadratic: |T - T_ref| <= 1e-8 T_ref, both NLLs to 1e-12, the status equal.

The minimiser of the reference is NOT Newton: the same bracket and the same end tests, then plain bisection of g down to a bracket of
1e-14 beta.  `variant=` names a deliberately wrong statistic (WRONG below): the comparison must reject each on some case."""
import numpy as np

TOL = 1e-12
T_RTOL = 1e-8
EDGE_MARGIN = 1e-9                      # no confidence of a generic case lies this close to a bin edge
EDGE_MARGIN_FIT = 1e-6                  # .. of a case whose T is fitted (two minimisers: T differs by up to 1e-8 T)
BETA_LO, BETA_HI = 1e-2, 1e2
FIT_LDS_BYTES = 159 * 1024              # the fit stages its logits in LDS when N C 4 <= this

WRONG = ("left_closed", "ignore_T", "multiply_T", "swap_mode", "brier_on_label", "ece_unweighted", "mce_empty_nan", "empty_rows_zero",
         "argmax_last", "nll_of_column")


def softmax64(logits, T=1.0):
    z = np.asarray(logits, dtype=np.float64) / T
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def bins_of(conf, M, left_closed=False):
    """bin i iff i / M < conf <= (i + 1) / M; a confidence of exactly 0 goes to bin 0; -1 for a NaN"""
    edges = np.arange(M + 1, dtype=np.float64) / np.float64(M)
    if left_closed:
        b = np.searchsorted(edges, conf, side="right") - 1
    else:
        b = np.searchsorted(edges, conf, side="left") - 1
    b = np.clip(b, 0, M - 1)
    return np.where(np.isnan(conf), -1, b)


def calibration_ref(logits, y, M, T=None, column=None, variant=None):
    logits = np.asarray(logits, dtype=np.float32)
    y = np.asarray(y, dtype=np.int64)
    N, C = logits.shape
    t = 1.0 if T is None or variant == "ignore_T" else 1.0 / float(T) if variant == "multiply_T" else float(T)
    p = softmax64(logits, t)
    valid = (y >= 0) & (y < C)
    yc = np.where(valid, y, 0)
    onehot = np.zeros((N, C))
    onehot[np.arange(N), yc] = valid
    if variant == "swap_mode":
        column = (1 if C > 1 else 0) if column is None else None
    if column is None:
        am = (C - 1 - np.argmax(logits[:, ::-1], axis=1)) if variant == "argmax_last" else np.argmax(logits, axis=1)
        conf = p[np.arange(N), am]
        hit = valid & (am == y)
        brier_n = ((p[np.arange(N), yc] - 1.0) ** 2) if variant == "brier_on_label" else ((p - onehot) ** 2).sum(1)
    else:
        conf = p[:, column]
        hit = y == column
        brier_n = (conf - hit) ** 2
    with np.errstate(divide="ignore"):
        nll_n = -np.log(p[np.arange(N), yc])
        if variant == "nll_of_column" and column is not None:
            nll_n = -np.log(np.where(hit, conf, 1.0 - conf))
    nll_n = np.where(valid, nll_n, np.nan)
    brier_n = np.where(valid, brier_n, np.nan)
    b = bins_of(conf, M, variant == "left_closed")
    counts = np.zeros((M, 2), dtype=np.int64)
    sums = np.zeros(M)
    for i in range(M):
        sel = b == i
        counts[i] = sel.sum(), (sel & hit).sum()
        sums[i] = conf[sel].sum()
    n = counts[:, 0].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        table = np.stack([n, np.where(n > 0, sums / n, np.nan), np.where(n > 0, counts[:, 1] / n, np.nan)], 1)
    gap = np.abs(table[:, 2] - table[:, 1])
    full = n > 0
    ece = float((gap[full]).mean()) if variant == "ece_unweighted" else float((n[full] / N * gap[full]).sum())
    mce = float(gap.max()) if variant == "mce_empty_nan" else float(gap[full].max()) if full.any() else 0.0
    if variant == "empty_rows_zero":
        table = np.where(np.isnan(table), 0.0, table)
    summary = np.array([ece, mce, brier_n.mean(), nll_n.mean(), counts[:, 1].sum() / N, sums.sum() / N])
    return {"counts": counts, "table": table, "summary": summary, "conf": conf}


def _close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a) | np.isnan(b)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.all(np.abs(a[~nan] - b[~nan]) <= tol))


def disagreements(got, ref):
    """names of what `got` misses of `ref`: counts exact, the table's rows column exact, its means and the six summaries within TOL,
    NaN where the reference is NaN and nowhere else"""
    bad = []
    if not np.array_equal(np.asarray(got["counts"], dtype=np.int64), ref["counts"]):
        bad.append("counts")
    if not np.array_equal(np.asarray(got["table"])[:, 0], ref["table"][:, 0]):
        bad.append("table_n")
    if not _close(np.asarray(got["table"])[:, 1:], ref["table"][:, 1:], TOL):
        bad.append("table_means")
    for i, k in enumerate(("ece", "mce", "brier", "nll", "accuracy", "confidence")):
        if not _close(np.asarray(got["summary"])[i], ref["summary"][i], TOL):
            bad.append(k)
    return bad


def errors(got, ref):
    """the largest absolute differences, for the record (profiles/calibration_errors.json)"""
    with np.errstate(invalid="ignore"):
        return {"table": float(np.nanmax(np.abs(np.asarray(got["table"])[:, 1:] - ref["table"][:, 1:]), initial=0.0)),
                "summary": float(np.nanmax(np.abs(np.asarray(got["summary"]) - ref["summary"]), initial=0.0))}


# ---- the fit ----
def fit_terms(logits, y, beta):
    """(g, h, NLL) at beta: g = mean(E_p[z] - z_y), h = mean(Var_p[z]), p = softmax(beta z); the row maximum is taken out of z first
    (it moves neither); a label outside [0, C) gives NaN"""
    z = np.asarray(logits, dtype=np.float32).astype(np.float64)
    y = np.asarray(y, dtype=np.int64)
    N, C = z.shape
    with np.errstate(invalid="ignore"):
        d = z - z.max(1, keepdims=True)
        w = np.exp(beta * d)
        S0, S1, S2 = w.sum(1), (w * d).sum(1), (w * d * d).sum(1)
        valid = (y >= 0) & (y < C)
        dy = np.where(valid, d[np.arange(N), np.where(valid, y, 0)], np.nan)
        E = S1 / S0
        return float((E - dy).mean()), float((S2 / S0 - E * E).mean()), float((np.log(S0) - beta * dy).mean())


def fit_ref(logits, y):
    """{T, beta, nll_before, nll_after, status, g}: the header's rule with bisection in place of Newton"""
    g1, _, nll1 = fit_terms(logits, y, 1.0)
    out = {"T": 1.0, "beta": 1.0, "nll_before": nll1, "nll_after": nll1, "status": 0, "g": g1}
    if not np.isfinite(g1):
        out["status"] = 4
        return out
    if g1 == 0.0:
        return out
    up = g1 < 0.0
    end = BETA_HI if up else BETA_LO
    ge, _, nlle = fit_terms(logits, y, end)
    if (ge < 0.0) if up else (ge > 0.0):
        out.update(T=BETA_LO if up else BETA_HI, beta=end, nll_after=nlle, status=1 if up else 2, g=ge)
        return out
    lo, hi = (1.0, BETA_HI) if up else (BETA_LO, 1.0)
    while hi - lo > 1e-14 * lo:
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if fit_terms(logits, y, mid)[0] < 0.0:
            lo = mid
        else:
            hi = mid
    beta = 0.5 * (lo + hi)
    g, _, nll = fit_terms(logits, y, beta)
    out.update(T=1.0 / beta, beta=beta, nll_after=nll, g=g)
    return out


def fit_disagreements(result, ref):
    """result: the eight cells of rd_fit_temperature"""
    r = np.asarray(result, dtype=np.float64)
    bad = []
    if int(r[5]) != ref["status"]:
        bad.append("status %d != %d" % (int(r[5]), ref["status"]))
    if not abs(r[0] - ref["T"]) <= T_RTOL * ref["T"]:
        bad.append("T")
    if not abs(r[1] * r[0] - 1.0) <= 1e-15 * 4:
        bad.append("beta")
    if not _close(r[2], ref["nll_before"], TOL):
        bad.append("nll_before")
    if not _close(r[3], ref["nll_after"], TOL):
        bad.append("nll_after")
    if not (1 <= r[4] <= 100 and r[4] == int(r[4]) and r[7] == 0.0):
        bad.append("cells")
    return bad


# ---- cases ----
def sample_labels(rng, base):
    """labels drawn from softmax(base)"""
    p = softmax64(base)
    u = rng.random(p.shape[0])
    return np.minimum((np.cumsum(p, 1) < u[:, None]).sum(1), p.shape[1] - 1).astype(np.int64)


def make_logits(seed, N, C, spread):
    """(logits f32 [N, C], y): labels follow softmax(base), the logits are spread x base -- spread > 1 is over-confident (T* ~ spread),
    spread < 1 under-confident"""
    rng = np.random.default_rng(seed)
    base = rng.normal(size=(N, C)) * 1.5
    y = sample_labels(rng, base)
    return (spread * base).astype(np.float32), y


# name, N, C, M, column (None: top label), T (None, a float, or "fit"), seed.  The sizes straddle the wave (63 .. 65), the 256-row
# chunk and workgroup (1023 .. 1025, 4099: 17 workgroups) and, in "two_chunks", the 262144 rows above which a workgroup walks more
# than one chunk; the seeds are the first for which no confidence lies within the margin of a bin edge (test_calibration_ref_host.py)
CASES = [
    ("one_row", 1, 2, 1, None, None, 0),
    ("n63_c3_col0", 63, 3, 10, 0, 0.5, 0),
    ("n64_c3_col1", 64, 3, 15, 1, 2.5, 0),
    ("n65_c3_col2", 65, 3, 256, 2, None, 0),
    ("n1025_c3_top", 1025, 3, 15, None, None, 0),
    ("n1023_c8_top", 1023, 8, 15, None, 0.5, 0),
    ("n1024_c64_top", 1024, 64, 10, None, 2.5, 0),
    ("n1025_c2_col1_fit", 1025, 2, 15, 1, "fit", 0),
    ("n4099_c8_top_fit", 4099, 8, 15, None, "fit", 0),
    ("n4099_c2_col1_m256", 4099, 2, 256, 1, None, 0),
    ("n65_c64_col5_m1", 65, 64, 1, 5, 2.5, 0),
    ("n64_c2_top_m256", 64, 2, 256, None, 0.5, 0),
    ("two_chunks", 262444, 2, 15, 1, None, 0),
]
LD_EXTRA = 3                            # the GPU tests give every case a row stride of C + 3


def make_case(name):
    _, N, C, M, column, T, seed = next(c for c in CASES if c[0] == name)
    return make_logits(1000 + 7919 * seed + N * 64 + C, N, C, 1.7)


def edge_distance(conf, M):
    edges = np.arange(M + 1, dtype=np.float64) / np.float64(M)
    return float(np.abs(conf[:, None] - edges[None, :]).min()) if conf.shape[0] * (M + 1) <= 1 << 24 else \
        float(min(np.abs(conf - e).min() for e in edges))


def edge_cases():
    """name -> (logits, y, M, column, T): the exact-edge cases, where the rule itself is under test"""
    out = {}
    # confidence exactly 0.5: M = 10 -> bin 4 (closed on the right); both logits equal: the argmax is column 0
    out["half"] = (np.zeros((70, 2), dtype=np.float32), (np.arange(70) % 3 == 0).astype(np.int64), 10, None, None)
    # a gap of 100: exp(-100) vanishes beside 1, confidence exactly 1.0 -> the last bin
    big = np.zeros((130, 3), dtype=np.float32)
    big[np.arange(130), np.arange(130) % 3] = 100.0
    out["one"] = (big, ((np.arange(130) + (np.arange(130) % 5 == 0)) % 3).astype(np.int64), 15, None, None)
    # .. and its complement in column mode: p = exp(-100) / 1 > 0 in bin 0, and rows of exactly 1.0 in the last
    out["one_column"] = (big, out["one"][1], 15, 1, None)
    # every row in one bin (confidences 0.6 .. 0.7 with M = 10 -> bin 6), the other nine empty: NaN rows, left out of the MCE
    rng = np.random.default_rng(5)
    pc = rng.uniform(0.61, 0.69, 300)
    lg = np.stack([np.zeros(300), np.log(pc / (1 - pc))], 1).astype(np.float32)
    out["one_bin"] = (lg, (rng.random(300) < 0.4).astype(np.int64), 10, None, None)
    # a label outside [0, C): the row is a miss, NLL and Brier NaN; the counts stay exact
    lg2, y2 = make_logits(77, 200, 3, 1.0)
    y2 = y2.copy(); y2[17] = 3; y2[150] = -1
    out["bad_label"] = (lg2, y2, 10, None, None)
    return out


# name, N, C, kind.  Staged in LDS iff N C 4 <= 159 KiB: 16384 x 2 stages, 16384 x 8 and 1025 x 64 do not
FIT_CASES = [
    ("over_4096_c2", 4096, 2, "over"),              # logits = 2.5 x base: T* ~ 2.5
    ("over_16384_c2", 16384, 2, "over"),
    ("over_16384_c8", 16384, 8, "over"),
    ("under_1025_c64", 1025, 64, "under"),
    ("under_1025_c8", 1025, 8, "under"),
    ("over_65_c8", 65, 8, "over"),
    ("under_65_c64", 65, 64, "under"),
    ("n1_c2", 1, 2, "over"),
    ("n2_c8", 2, 8, "over"),
    ("separable", 65, 8, "separable"),
    ("worse_than_chance", 1025, 2, "worst"),
    ("constant_rows", 65, 8, "constant"),
    ("nan_logit", 1025, 8, "nan"),
]
INTERIOR = ("over_4096_c2", "over_16384_c2", "over_16384_c8", "under_1025_c64", "under_1025_c8", "over_65_c8", "under_65_c64")


def make_fit_case(name):
    _, N, C, kind = next(c for c in FIT_CASES if c[0] == name)
    seed = 500 + N * 64 + C
    if kind in ("over", "under", "nan"):
        lg, y = make_logits(seed, N, C, 2.5 if kind != "under" else 0.4)
        if kind == "nan":
            lg = lg.copy(); lg[N // 2, C - 1] = np.nan
        return lg, y
    rng = np.random.default_rng(seed)
    if kind == "separable":                          # small gaps: g is still clearly negative at beta = 100
        lg = (rng.normal(size=(N, C)) * 0.02).astype(np.float32)
        return lg, np.argmax(lg, 1).astype(np.int64)
    if kind == "worst":
        lg = rng.normal(size=(N, C)).astype(np.float32)
        return lg, np.argmin(lg, 1).astype(np.int64)
    assert kind == "constant"
    lg = np.repeat(rng.normal(size=(N, 1)), C, axis=1).astype(np.float32)
    return lg, rng.integers(0, C, N).astype(np.int64)
