"""CPU: conditions on the bootstrap restatement alone (tests/bootstrap_ref.py) -- it is the expanded resample's rank_metrics_ref, a
brute-force pair count, sklearn with sample_weight and numpy's percentile / std -- and the condition that makes
tests/test_bootstrap_metrics_gpu.py worth running: its comparison rejects every wrong restatement."""
import numpy as np
import pytest

from tests import bootstrap_ref as B
from tests import metrics_ref as M

SMALL = [c for c in B.CASES if c[1] <= 65]
BY_NAME = {c[0]: c for c in B.CASES}


def test_known_answer_words_of_the_new_site():
    """words 0 .. 3 of quad r * ceil(N / 4) + (k >> 2) are (x0, x1) of the Threefry calls 2 q and 2 q + 1 at site 84; pinned."""
    seed, N, r = (7 << 32) | 99, 10, 3                                    # ceil(N / 4) = 3: quads 9, 10, 11 = calls 18 .. 22
    w = B.words(seed, r, N)
    for k in range(N):
        call = 2 * (r * 3 + (k >> 2)) + ((k >> 1) & 1)
        x = B.RNG.threefry2x32_13(call, B.SITE_BOOTSTRAP << 16, 99, 7)
        assert int(w[k]) == int(x[k & 1]), k
    assert [int(v) for v in B.words(0, 0, 4)] == KNOWN_SEED0_QUAD0
    assert [int(v) for v in w[:4]] == KNOWN_SEED_QUAD9
    assert not np.array_equal(B.words(seed, r, N), B.words(seed, r, N, quad_shift=1))
    assert np.array_equal(B.words(seed, r, N, quad_shift=1)[:4], B.words(seed, r, N)[4:8])      # the next quad's words
    assert np.array_equal(B.draw_indices(seed, r, N), ((w * np.uint64(N)) >> np.uint64(32)).astype(np.int64))


# recorded from tests/rng_ref.py's threefry2x32_13, which tests/test_rng_ref_host.py ties to Random123's published vectors
KNOWN_SEED0_QUAD0 = [3658941468, 236512890, 1829890082, 2104911449]
KNOWN_SEED_QUAD9 = [1682734176, 3551695061, 1302087005, 4052015474]


@pytest.mark.parametrize("N", [1, 2, 3, 65, 1025, 16384])
def test_rows_of_m_sum_to_N_and_stay_in_range(N):
    m = B.counts(B.SEED, N, [0, 1, 4095])
    assert m.shape == (3, N) and (m.sum(1) == N).all() and m.min() >= 0
    idx = B.draw_indices(B.SEED, 4095, N)
    assert idx.min() >= 0 and idx.max() < N
    if N >= 1025:                                                         # the draw is uniform: about 1 / e of the rows stay out
        assert abs((m == 0).mean() - np.exp(-1.0)) < 0.03
        assert not np.array_equal(m[0], m[1])


@pytest.mark.parametrize("case", [c for c in B.CASES if c[1] <= 1025 and c[4] != "specials"], ids=lambda c: c[0])
def test_weighted_statistics_are_the_expanded_resample_s(case):
    s, y = B.make_case(*case)
    N, C, R = s.shape[0], s.shape[1], min(case[3], 12)
    ref = B.bootstrap_ref(s, y, R, B.SEED)
    for r in range(R):
        idx = B.draw_indices(B.SEED, r, N)
        assert np.array_equal(np.bincount(idx, minlength=N), ref["counts"][r])
        e = M.rank_metrics_ref(s[idx], y[idx])
        assert np.array_equal(e["num"], ref["num"][r])
        assert np.array_equal(np.isnan(e["auroc"]), np.isnan(ref["auroc"][r]))
        assert np.allclose(e["auroc"], ref["auroc"][r], rtol=0, atol=1e-15, equal_nan=True)
        assert np.abs(e["auprc"] - ref["auprc"][r]).max() <= 1e-13
        assert np.array_equal([(y[idx] == c).sum() for c in range(C)], ref["pos"][r])
        assert np.allclose([e["auroc_macro"], e["auprc_macro"]], ref["mean"][r], rtol=0, atol=1e-13, equal_nan=True)


def _brute(key, pos, w):
    """numerator and AP of one column by pair counting / per distinct threshold, Python integers."""
    n = len(key)
    num = sum(int(w[i]) * int(w[j]) * (2 if key[i] > key[j] else 1 if key[i] == key[j] else 0)
              for i in range(n) if pos[i] for j in range(n) if not pos[j])
    P = sum(int(w[i]) for i in range(n) if pos[i])
    ap = 0.0
    for t in sorted(set(key.tolist()), reverse=True):
        at = sum(int(w[i]) for i in range(n) if pos[i] and key[i] == t)
        if at:
            above = sum(int(w[i]) for i in range(n) if key[i] >= t)
            ap += at / P * sum(int(w[i]) for i in range(n) if pos[i] and key[i] >= t) / above
    return num, P, ap


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c[0])
def test_weighted_statistics_equal_a_brute_force_pair_count(case):
    s, y = B.make_case(*case)
    N, C, R = s.shape[0], s.shape[1], min(case[3], 6)
    ref = B.bootstrap_ref(s, y, R, B.SEED)
    for c in range(C):
        key = B.order_key(s[:, c])
        for r in range(R):
            num, P, ap = _brute(key, y == c, ref["counts"][r])
            assert (num, P) == (int(ref["num"][r, c]), int(ref["pos"][r, c]))
            assert abs(ap - ref["auprc"][r, c]) <= 1e-13
            a = ref["auroc"][r, c]
            assert np.isnan(a) if P == 0 or P == N else a == num / (2.0 * P * (N - P))


@pytest.mark.parametrize("name", ["n64_three_levels", "n1023_distinct", "n63_sigmoid8_outside"])
def test_weighted_statistics_equal_sklearn_with_sample_weight(name):
    sk = pytest.importorskip("sklearn.metrics")
    case = BY_NAME[name]
    s, y = B.make_case(*case)
    R = 8
    ref = B.bootstrap_ref(s, y, R, B.SEED)
    checked = 0
    for r in range(R):
        w = ref["counts"][r]
        live = w > 0
        for c in range(s.shape[1]):
            t = (y == c)[live]
            if t.any() and not t.all():
                assert abs(sk.roc_auc_score(t, s[live, c], sample_weight=w[live]) - ref["auroc"][r, c]) <= 1e-12
                assert abs(sk.average_precision_score(t, s[live, c], sample_weight=w[live]) - ref["auprc"][r, c]) <= 1e-12
                checked += 1
    assert checked >= R


def test_summary_is_numpy_percentile_and_std():
    rng = np.random.default_rng(3)
    for R, C, alpha in ((1, 1, 0.05), (2, 2, 0.05), (257, 3, 0.1), (1000, 2, 0.05)):
        a, p = rng.random((R, C)), rng.random((R, C))
        a[rng.random((R, C)) < 0.3] = np.nan
        if R > 2:
            a[:, 0] = np.nan                                              # a column that is never defined
            a[1:, 1] = np.nan                                             # and one with a single valid resample
        mean = np.stack([a.mean(1), p.mean(1)], 1)
        got = B.summary_ref(a, p, mean, alpha)
        for k, b in enumerate((np.c_[a, mean[:, 0]], np.c_[p, mean[:, 1]])):
            for c in range(C + 1):
                v = b[:, c][~np.isnan(b[:, c])]
                assert got[k, c, 0] == len(v)
                want = [v.mean() if len(v) else np.nan] + ([np.std(v, ddof=1)] + list(np.percentile(v, [50 * alpha, 100 - 50 * alpha]))
                                                           if len(v) > 1 else [np.nan] * 3)
                assert np.allclose(got[k, c, 1:], want, rtol=0, atol=1e-14, equal_nan=True), (R, k, c)


# variant -> the cases on which the comparison must reject it (each names the ground the variant stands on)
REJECTED_ON = {"split_ties": ["n64_three_levels", "n16384_levels64"], "unweighted_P": ["n64_three_levels", "n1023_distinct"],
               "column_draw": ["n64_three_levels", "n63_sigmoid8_outside"], "quad_shift": ["n3_one_positive", "n1023_distinct"],
               "zero_opens": ["n64_three_levels", "n1023_distinct"], "nan_as_zero": ["n3_one_positive", "n1025_one_positive"]}


@pytest.mark.parametrize("variant", B.VARIANTS)
def test_wrong_kernels_must_fail(variant):
    for name in REJECTED_ON[variant]:
        case = BY_NAME[name]
        s, y = B.make_case(*case)
        R = min(case[3], 64)
        ref = B.bootstrap_ref(s, y, R, B.SEED)
        assert B.disagreements(ref, ref, s.shape[0]) == []
        bad = B.disagreements(B.bootstrap_ref(s, y, R, B.SEED, variant=variant), ref, s.shape[0])
        assert bad, (variant, name)


def test_one_positive_leaves_a_third_of_the_resamples_undefined():
    case = BY_NAME["n1025_one_positive"]
    s, y = B.make_case(*case)
    ref = B.bootstrap_ref(s, y, case[3], B.SEED)
    frac = np.isnan(ref["auroc"][:, 1]).mean()
    assert abs(frac - np.exp(-1.0)) < 0.1 and ref["summary"][0, 1, 0] == (~np.isnan(ref["auroc"][:, 1])).sum()
    assert (ref["auprc"][np.isnan(ref["auroc"][:, 1]), 1] == 0.0).all()
