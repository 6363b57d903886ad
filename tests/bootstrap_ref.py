"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the bootstrap of the validation metrics (include/raindrop_hip.h "validation
metrics": rd_rank_bootstrap, _summary, _counts; raindrop_amd/csrc/rd_metrics_boot.hip), on tests/rng_ref.py's Threefry.

Resample rule: draw k of resample r reads raw 32-bit word k & 3 of quad r * ceil(N / 4) + (k >> 2) of site 84 under the key `seed`;
a quad is two Threefry-2x32-13 calls, counters 2 q and 2 q + 1, words (x0, x1) of each; the row is floor(word * N / 2^32).
Statistics: tests/metrics_ref.py's formulas with every sample counted m_r[j] times, in the kernels' key order (NaNs rank by sign
and payload, equal payloads tie).  `variant=` names a deliberately WRONG restatement; tests/test_bootstrap_ref_host.py shows that
`disagreements`, the comparison the GPU test uses, rejects each of them."""
import numpy as np

from tests import metrics_ref as M
from tests import rng_ref as RNG

SITE_BOOTSTRAP = 84                  # rd_rng.h enum DropSite, behind the feed's 80..83
N_MAX, R_MAX = 16384, 4096
TOL = 1e-10                          # tests/test_metrics_ref.py TOL: the bound rd_rank_metrics' float64 sums are held to
VARIANTS = ("split_ties", "unweighted_P", "column_draw", "quad_shift", "zero_opens", "nan_as_zero")


def words(seed, r, N, quad_shift=0):
    """uint64 [N] holding the 32-bit words of the N draws of resample r."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    nq = (N + 3) >> 2
    call = np.uint64(2 * (r * nq + quad_shift)) + np.arange((N + 1) >> 1, dtype=np.uint64)
    c1 = (call >> np.uint64(32)) | np.uint64(SITE_BOOTSTRAP << 16)
    x0, x1 = RNG.threefry2x32_13(call & np.uint64(0xFFFFFFFF), c1, np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    return np.stack([x0, x1], axis=1).reshape(-1)[:N]


def draw_indices(seed, r, N, quad_shift=0):
    """int64 [N]: the rows resample r draws, floor(word * N / 2^32) (word < 2^32, N <= 2^14: exact in uint64)."""
    return ((words(seed, r, N, quad_shift) * np.uint64(N)) >> np.uint64(32)).astype(np.int64)


def counts(seed, N, rows, quad_shift=0):
    """int64 [len(rows), N]: m_r for the resamples `rows`; every row sums to N."""
    return np.stack([np.bincount(draw_indices(seed, int(r), N, quad_shift), minlength=N) for r in rows]).astype(np.int64)


def order_key(s):
    """rd_metrics.hip make_key's score part: uint32 whose order is the float32 order, -0.0 == +0.0, NaNs by sign and payload."""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = np.where((u << np.uint64(1)) & np.uint64(0xFFFFFFFF) == 0, np.uint64(0), u)
    neg = (u & np.uint64(0x80000000)) != 0
    return np.where(neg, ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000)).astype(np.int64)


def weighted_column(s, pos, m, variant=None):
    """(auroc [R], ap [R], numerator [R] int64, P [R] int64) of one score column against the boolean positives under the
    multiplicities m [R, N]."""
    key = order_key(s)
    N = key.shape[0]
    order = np.argsort(-key, kind="stable")
    kk, pp = key[order], np.asarray(pos, dtype=bool)[order].astype(np.int64)
    ends = np.r_[kk[1:] != kk[:-1], True]
    if variant == "split_ties":
        ends[:] = True
    W = np.asarray(m, dtype=np.int64)[:, order]
    if variant == "zero_opens":
        W = np.where(W == 0, 1, W)
    tp = np.cumsum(W * pp, axis=1)[:, ends]
    fp = np.cumsum(W, axis=1)[:, ends] - tp
    zero = np.zeros((W.shape[0], 1), dtype=np.int64)
    tpp, fpp = np.c_[zero, tp[:, :-1]], np.c_[zero, fp[:, :-1]]
    P = np.full(W.shape[0], int(pp.sum()), dtype=np.int64) if variant == "unweighted_P" else tp[:, -1].copy()
    Q = N - P
    num = np.sum((fp - fpp) * (tp + tpp), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        auroc = np.where((P > 0) & (Q > 0), num / (2.0 * P * Q), np.nan)
        term = (tp - tpp) / P[:, None].astype(np.float64) * tp / (tp + fp)
    ap = np.where(P > 0, np.where(tp > tpp, term, 0.0).sum(axis=1), 0.0)
    return auroc, ap, num, P


def summary_ref(auroc_b, auprc_b, mean_b, alpha, variant=None):
    """float64 [2, C + 1, 5]: metric x (columns, macro mean) x (n_valid, mean, deviation ddof = 1, lower, upper), written out: the
    valid values ascending, two-pass deviation, the percentile at h = (n - 1) q between its two neighbours."""
    C = auroc_b.shape[1]
    out = np.full((2, C + 1, 5), np.nan)
    for k, (b, mcol) in enumerate(((auroc_b, mean_b[:, 0]), (auprc_b, mean_b[:, 1]))):
        for c in range(C + 1):
            v = np.asarray(b[:, c] if c < C else mcol, dtype=np.float64)
            v = np.where(np.isnan(v), 0.0, v) if variant == "nan_as_zero" else v[~np.isnan(v)]
            v = np.sort(v)
            n = v.shape[0]
            out[k, c, 0] = n
            if n > 0:
                out[k, c, 1] = v.sum() / n
            if n > 1:
                out[k, c, 2] = np.sqrt(((v - out[k, c, 1]) ** 2).sum() / (n - 1))
                for slot, q in ((3, 0.5 * alpha), (4, 1.0 - 0.5 * alpha)):
                    h = (n - 1) * q
                    i = min(max(int(np.floor(h)), 0), n - 1)
                    out[k, c, slot] = v[i] + (v[min(i + 1, n - 1)] - v[i]) * (h - i)
    return out


def bootstrap_ref(scores, y, R, seed, alpha=0.05, variant=None):
    """dict(counts [R, N], auroc, auprc [R, C] float64, num, pos [R, C] int64, mean [R, 2], summary [2, C + 1, 5])."""
    scores, y = np.asarray(scores, dtype=np.float32), np.asarray(y)
    N, C = scores.shape
    shift = 1 if variant == "quad_shift" else 0
    m = counts(seed, N, range(R), shift)
    cols = []
    for c in range(C):
        mc = counts(seed, N, [r * C + c for r in range(R)], shift) if variant == "column_draw" else m
        cols.append(weighted_column(scores[:, c], y == c, mc, variant))
    a, p = np.stack([k[0] for k in cols], 1), np.stack([k[1] for k in cols], 1)
    mean = np.stack([a.sum(1) / C, p.sum(1) / C], 1)
    return {"counts": m, "auroc": a, "auprc": p, "num": np.stack([k[2] for k in cols], 1), "pos": np.stack([k[3] for k in cols], 1),
            "mean": mean, "summary": summary_ref(a, p, mean, alpha, variant)}


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool((np.abs(a - b)[~np.isnan(b)] <= TOL).all())


def disagreements(got, ref, N):
    """Names of the fields in which `got` (the device's, or a variant's) misses `ref`: multiplicities, numerators and positives
    EXACT, AUROC NaN where the reference's is and elsewhere the exact float64 quotient of ITS OWN numerator and positives, AUPRC /
    macro means / summary within TOL with NaNs in the same places, n_valid exact.  [] = agreement."""
    bad = [k for k in ("counts", "num", "pos") if k in got and not np.array_equal(np.asarray(got[k], dtype=np.int64), ref[k])]
    P, num = np.asarray(got["pos"], dtype=np.int64), np.asarray(got["num"], dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        quot = np.where((P > 0) & (N - P > 0), num / (2.0 * P * (N - P)), np.nan)
    a = np.asarray(got["auroc"], dtype=np.float64)
    if not (np.array_equal(np.isnan(a), np.isnan(ref["auroc"])) and np.array_equal(a.view(np.int64)[~np.isnan(a)], quot.view(np.int64)[~np.isnan(a)])):
        bad.append("auroc")
    bad += [k for k in ("auprc", "mean", "summary") if not _close(got[k], ref[k])]
    if not np.array_equal(np.asarray(got["summary"])[:, :, 0], ref["summary"][:, :, 0]):
        bad.append("n_valid")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------
# cases: (name, N, C, R, pattern).  N around the 64-lane wave, the 1024-thread workgroup (one key per thread / two), the sort's
# powers of two and the envelope's end; R around the summary's 256 threads and at the envelope's end.  Large N goes with small R.
# ---------------------------------------------------------------------------------------------------------------------------------
CASES = [("n1_single", 1, 1, 2, "distinct"), ("n2_tied", 2, 2, 257, "tied"), ("n3_one_positive", 3, 1, 255, "one_positive"),
         ("n63_sigmoid8_outside", 63, 8, 256, "sigmoid8_outside"), ("n64_three_levels", 64, 2, 4096, "levels3"),
         ("n65_specials", 65, 2, 2, "specials"), ("n1023_distinct", 1023, 2, 255, "distinct"),
         ("n1024_single_class", 1024, 2, 1, "single_class"), ("n1025_one_positive", 1025, 2, 257, "one_positive"),
         ("n4097_sigmoid8", 4097, 8, 2, "sigmoid8"), ("n16384_levels64", 16384, 2, 2, "levels64")]
SEED = 0x1234ABCD5


def make_case(name, N, C, R, pattern):
    """(scores float32 [N, C], y int64 [N]) of a case, through tests/metrics_ref.make_case."""
    sd = 4000 + N
    if pattern.startswith("sigmoid8"):
        s, y = M.make_case("sigmoid8", N, C, sd, 0.0, 0)
        if pattern.endswith("outside"):
            y[::7], y[3::11] = -1, C                                       # negatives of every column
        return s, y
    lv = {"distinct": 0, "levels3": 3, "levels64": 64}.get(pattern, 0)
    s, y = M.make_case("equal" if pattern == "tied" else "binary", N, 2, sd, 0.5 if pattern in ("tied", "levels3") else 0.04 if N > 64 else 0.5, lv)
    if pattern == "single_class":
        y[:] = 1
    if pattern == "one_positive":
        y[:] = 0
        y[N // 2] = 1
        if C == 1:
            y = 1 - y                                                      # the one positive of column 0
    if pattern == "specials":
        sp = np.array([np.inf, -np.inf, 0.0, -0.0, np.nan, -np.nan, 0.5], dtype=np.float32)
        sp = np.r_[sp, np.array([0x7FC00001, 0xFFC00001, 0x7FC00001], dtype=np.uint32).view(np.float32)]      # payloads: equal ones tie
        pick = np.random.default_rng(sd).integers(0, len(sp), size=(N, 2))
        s = sp[pick]
        s[:, 1] = np.where(np.arange(N) % 3 == 0, s[:, 0], s[:, 1])
    return np.ascontiguousarray(s[:, :C]), y
