"""CPU: the numpy restatement of the augmenting batch gather (tests/feed_aug_ref.py) on its own -- identity at rate 0, the drop rates
and the jitter's moments, the key's dependence on (epoch, cursor), the all-dropped rule, the single rounding of the jitter, the
argument checks of `feed.Augment` / `fit`, and eight deliberately wrong kernels that must each fail the GPU test's comparison."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

from raindrop_amd import _lib
from tests import feed_aug_ref as R
from tests import rng_ref


def _dataset(T, N, F, seed, density=0.7):
    """P_all [T,N,2F], time_all [T,N]: values everywhere (also where the indicator is 0), indicators Bernoulli(density); sample 0 has
    no positive time, sample 1 one, sample 2 all, sample 3 a zero first time followed by positive ones (the reference's undercount),
    the others a random prefix"""
    rng = np.random.default_rng(seed)
    val = rng.standard_normal((T, N, F)).astype(np.float32)
    ind = (rng.random((T, N, F)) < density).astype(np.float32)
    length = rng.integers(0, T + 1, size=N)
    length[:4] = (0, min(1, T), T, T)
    tm = (np.cumsum(rng.random((T, N)) + 0.01, axis=0) * (np.arange(T)[:, None] < length[None, :])).astype(np.float32)
    if N > 3:
        tm[0, 3] = 0.0
    return np.concatenate([val, ind], axis=-1), tm


ALL_ON = dict(p_time=0.3, p_sensor=0.2, p_obs=0.15, noise_c=R.noise_c(0.05))


def test_all_rates_zero_is_the_plain_fancy_index():
    P, tm = _dataset(9, 11, 3, seed=1)
    idx = np.array([3, 0, 10, 2, 2, 1])
    src, times, lengths = R.augment(P, tm, idx, key=77)
    assert np.array_equal(src.view(np.int32), P[:, idx].view(np.int32)) and np.array_equal(times.view(np.int32), tm[:, idx].view(np.int32))
    assert np.array_equal(lengths, (tm[:, idx] > 0).sum(0))


@pytest.mark.parametrize("p", [0.05, 0.2, 0.5])
def test_empirical_drop_rates(p):
    """n >= 1e5 decisions per site: |rate - p| <= 5 sqrt(p (1 - p) / n)"""
    T, N, F, B = 64, 40, 34, 48
    rng = np.random.default_rng(3)
    P = np.concatenate([rng.standard_normal((T, N, F)), np.ones((T, N, F))], axis=-1).astype(np.float32)
    tm = np.tile(np.arange(1, T + 1, dtype=np.float32)[:, None], (1, N))                      # every row a candidate
    idx = rng.integers(0, N, B)
    plain = P[:, idx]

    def within(dropped, n):
        return abs(dropped / n - p) <= 5.0 * np.sqrt(p * (1 - p) / n)

    # observations: T*B*F = 104448 decisions in one batch
    src, _, _ = R.augment(P, tm, idx, key=5, p_obs=p)
    assert T * B * F >= 100000 and within(int((src[:, :, F:] == 0).sum()), T * B * F)
    assert np.array_equal(src[:, :, :F][src[:, :, F:] != 0], plain[:, :, :F][src[:, :, F:] != 0])   # the kept ones untouched
    assert not src[:, :, :F][src[:, :, F:] == 0].any()
    # time steps: T*B = 3072 per batch, 36 batches; sensors: B*F = 1632 per batch, 64 batches
    dropped = n = 0
    for k in range(36):
        _, _, lengths = R.augment(P, tm, idx, key=1000 + k, p_time=p)
        dropped, n = dropped + int((T - lengths).sum()), n + T * B
    assert n >= 100000 and within(dropped, n)
    dropped = n = 0
    for k in range(64):
        src, _, _ = R.augment(P[:1], tm[:1], idx, key=2000 + k, p_sensor=p)
        dropped, n = dropped + int((src[0, :, F:] == 0).sum()), n + B * F
    assert n >= 100000 and within(dropped, n)


def test_jitter_moments_and_bound():
    T, N, F, B, sigma = 64, 8, 34, 48, 0.05
    P = np.concatenate([np.zeros((T, N, F)), np.ones((T, N, F))], axis=-1).astype(np.float32)
    tm = np.ones((T, N), dtype=np.float32)
    src, _, _ = R.augment(P, tm, np.arange(B) % N, key=9, noise_c=R.noise_c(sigma))
    noise = src[:, :, :F].astype(np.float64).ravel()
    assert noise.size >= 100000
    assert abs(noise.var() / sigma ** 2 - 1.0) <= 0.02 and abs(noise.mean()) <= 5 * sigma / np.sqrt(noise.size)
    assert np.abs(noise).max() <= 2 * np.sqrt(3.0) * sigma
    assert np.array_equal(src[:, :, F:], P[:, np.arange(B) % N, F:])


def test_fma32_rounds_once():
    """against exact rational arithmetic, on operands built to sit on and next to float32 rounding ties"""
    rng = np.random.default_rng(4)
    c = R.noise_c(0.05)
    a = ((rng.integers(0, 1 << 18, 4000) - (1 << 17)) * 2.0 ** -16).astype(np.float32)
    v = (rng.standard_normal(4000) * np.exp(3 * rng.standard_normal(4000))).astype(np.float32)
    # ties: v chosen so that a*c + v lies within a few double ulps of the midpoint of two float32 neighbours
    for k in range(0, 2000):
        exact = Fraction(float(a[k])) * Fraction(float(c))
        target = np.float32(rng.standard_normal())
        mid = (Fraction(float(target)) + Fraction(float(np.nextafter(target, np.float32(np.inf))))) / 2
        v[k] = np.float32(float(mid - exact))
    v[-6:] = (0.0, -0.0, 1e-40, -1e-40, 1.17549435e-38, 3e38)
    got = R.fma32(a, c, v)

    def exact_round(x):
        """round a Fraction to float32, ties to even"""
        f = np.float32(float(x))                                   # within one double rounding: a candidate
        cands = sorted({f, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))}, key=float)
        best = min(cands, key=lambda q: (abs(Fraction(float(q)) - x), int(np.float32(q).view(np.uint32)) & 1))
        return np.float32(best)
    for k in range(a.size):
        x = Fraction(float(a[k])) * Fraction(float(c)) + Fraction(float(v[k]))
        if abs(x) > Fraction(3.4e38):
            continue
        assert got[k].view(np.int32) == exact_round(x).view(np.int32) or (x == 0 and got[k] == 0), (k, a[k], v[k], got[k])


def test_masks_depend_on_epoch_and_cursor():
    P, tm = _dataset(12, 9, 3, seed=2)
    idx = np.array([2, 3, 4, 5, 2])
    cap = 7
    seen = {}
    for epoch in range(3):
        for cursor in range(cap):
            key = R.batch_key(11, epoch, cap, cursor)
            out = R.augment(P, tm, idx, key, **ALL_ON)
            assert R.same(out, R.augment(P, tm, idx, R.batch_key(11, epoch, cap, cursor), **ALL_ON))
            seen[(epoch, cursor)] = out
    pairs = list(seen)
    assert all(not R.same(seen[x], seen[y]) for i, x in enumerate(pairs) for y in pairs[i + 1:])
    assert R.batch_key(2 ** 64 - 1, 0, cap, 1) == 0 and R.batch_key(5, 2, 7, 3) == 22            # uint64, wrapping


def test_all_dropped_rule():
    P, tm = _dataset(6, 5, 2, seed=3)
    idx = np.array([0, 1, 2, 3, 4])
    plain = R.augment(P, tm, idx, key=1)
    # at p_time = 0.999 some sample certainly loses every candidate over these keys (and keeps them all); no sample is ever emptied
    hit = 0
    for key in range(40):
        src, times, lengths = R.augment(P, tm, idx, key, p_time=0.999)
        for b in range(5):
            L = int((tm[:, idx[b]] > 0).sum())
            u = rng_ref.uniform4(key, R.SITE_FEED_TIME, (b * 6 + np.arange(L)) >> 2)
            u = u[np.arange(L), (b * 6 + np.arange(L)) & 3]
            if L and not (u >= np.float32(0.999)).any():
                hit += 1
                assert np.array_equal(src[:, b].view(np.int32), plain[0][:, b].view(np.int32)) and lengths[b] == plain[2][b]
            assert lengths[b] >= min(L, 1) or L == 0
    assert hit >= 20


def test_augment_argument_checks():
    from raindrop_amd.feed import Augment
    from raindrop_amd.trainer import _check_fit_args, _resolve_augment
    a = Augment(p_time=0.1, p_sensor=0.2, p_obs=0.3, value_noise=0.05, seed=2 ** 64 + 5)
    assert a.state() == dict(p_time=0.1, p_sensor=0.2, p_obs=0.3, value_noise=0.05, seed=5)
    cell = a.cell(epoch=3)
    assert cell.dtype == np.int64 and cell.nbytes == 32 and cell.view(np.uint64)[:2].tolist() == [5, 3]
    assert cell.view(np.float32)[4:].tolist() == [np.float32(0.1), np.float32(0.2), np.float32(0.3), R.noise_c(0.05)]
    assert Augment().cell().tolist() == [0, 0, 0, 0]
    for bad in (dict(p_time=1.0), dict(p_sensor=-0.1), dict(p_obs=1.5), dict(p_obs=float("nan")), dict(value_noise=-1.0),
                dict(value_noise=float("inf")), dict(p_time="0.1"), dict(p_time=True), dict(seed=1.5), dict(p_obs=0.99999999)):
        with pytest.raises(ValueError):
            Augment(**bad)
    assert _resolve_augment(None) is None and _resolve_augment(a) is a
    assert _resolve_augment(dict(p_sensor=0.2, seed=3)).state()["p_sensor"] == 0.2
    ds = type("D", (), dict(y=np.zeros(4)))()
    for bad in (0.3, "time", [0.1], dict(p_drop=0.1), dict(p_time=2.0)):
        with pytest.raises(ValueError):
            _check_fit_args(ds, ds, 1, 8, 2, augment=bad)
    _check_fit_args(ds, ds, 1, 8, 2, augment=dict(p_obs=0.1))


def test_entry_points_check_their_arguments_before_launch():
    if not os.path.exists(_lib.LIB_PATH):
        from raindrop_amd import build
        build.build(verbose=False)
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    # rd_batch_gather_aug(T, B, W, d_static, N, 11 pointers, aug_cell, draw, stream)
    assert lib.rd_batch_gather_aug(5, 2, 0, 0, 10, *([None] * 12), 0, None) == -1 and b"bad dims" in lib.rd_last_error()
    assert lib.rd_batch_gather_aug(5, 2, 7, 0, 10, *([one] * 12), 0, None) == -1 and b"W = 2F" in lib.rd_last_error()      # odd W
    assert lib.rd_batch_gather_aug(5, 2, 6, 0, 10, *([None] * 12), 0, None) == -1 and b"NULL" in lib.rd_last_error()
    args = [one] * 12
    args[2] = args[3] = args[7] = args[8] = None
    for missing in (0, 1, 4, 5, 6, 9, 11):                          # P_all, time_all, idx, src, times, lengths, aug_cell
        a = list(args)
        a[missing] = None
        assert lib.rd_batch_gather_aug(5, 2, 6, 0, 10, *a, 0, None) == -1 and b"NULL" in lib.rd_last_error(), missing
    assert lib.rd_batch_gather_aug(5, 0, 6, 0, 10, *([None] * 12), 0, None) == 0
    # rd_feed_gather_aug(T, B, W, d_static, N, capacity, 12 pointers, aug_cell, stream)
    for dims in ((5, 2, 0, 0, 10, 4), (5, 2, 6, 0, 0, 4), (5, 2, 6, 0, 10, 0), (5, -1, 6, 0, 10, 4)):
        assert lib.rd_feed_gather_aug(*dims, *([None] * 14)) == -1 and b"bad dims" in lib.rd_last_error(), dims
    assert lib.rd_feed_gather_aug(5, 2, 7, 0, 10, 4, *([one] * 13), None) == -1 and b"W = 2F" in lib.rd_last_error()
    for missing in (0, 1, 3, 4, 5, 6, 7, 9, 10, 12):                # ... and aug_cell
        a = [one] * 13 + [None]
        a[2] = a[8] = None
        a[missing] = None
        assert lib.rd_feed_gather_aug(5, 2, 6, 0, 10, 4, *a) == -1 and b"NULL" in lib.rd_last_error(), missing
    assert lib.rd_feed_gather_aug(5, 0, 6, 0, 10, 4, *([None] * 14)) == 0


def test_kernels_use_no_scratch_and_no_lds():
    from raindrop_amd import build
    build.build(verbose=False)
    hits = {k: v for k, v in build.resource_usage().items() if "k_gather_aug" in k}
    assert len(hits) == 2, sorted(hits)                             # the feed form and the explicit-index form of one body
    for name, u in hits.items():
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["lds"] == 0, (name, u)


# ---- wrong kernels ----------------------------------------------------------------------------------------------------------------------
KEEP_GT_CASE = dict(T=64, N=23, F=34, B=33, p_obs=0.25, seed=None)           # filled in by _keep_gt_seed


def keep_gt_seed(T=64, B=33, F=34, p=0.25, tries=64):
    """the first key under which some observation's uniform EQUALS p: the only place `u > p` and `u >= p` part (u = k 2^-16)"""
    quads = np.arange((T * B * F + 3) // 4, dtype=np.int64)
    for key in range(tries):
        u = rng_ref.uniform4(key, R.SITE_FEED_OBS, quads).reshape(-1)[:T * B * F]
        if (u == np.float32(p)).any():
            return key
    return None


@pytest.mark.parametrize("bug", R.BUGS)
def test_wrong_kernels_fail_the_comparison(bug):
    """every deliberately wrong variant differs from the restatement under the GPU test's comparison, on the GPU test's kind of
    case: samples with L = 0, 1, T, the undercount sample, all four transforms on, NaN-filled outputs"""
    T, N, F = 12, 9, 3
    P, tm = _dataset(T, N, F, seed=6)
    idx = np.array([0, 1, 2, 3, 4, 5, 6])
    epoch, cap, cursor = 2, 5, 1
    rates = dict(ALL_ON)
    if bug == "keep_gt":
        c = KEEP_GT_CASE
        key = keep_gt_seed(c["T"], c["B"], c["F"], c["p_obs"])
        assert key is not None
        P, tm = _dataset(c["T"], c["N"], c["F"], seed=6, density=1.0)
        idx = np.arange(c["B"]) % c["N"]
        good = R.augment(P, tm, idx, key, p_obs=c["p_obs"])
        assert not R.same(good, R.augment(P, tm, idx, key, p_obs=c["p_obs"], bug=bug))
        return
    good = R.augment(P, tm, idx, R.batch_key(3, epoch, cap, cursor), **rates)
    wrong = R.augment(P, tm, idx, R.batch_key(3, epoch, cap, cursor, bug=bug), bug=bug, **rates)
    assert not R.same(good, wrong), bug
    assert R.same(good, R.augment(P, tm, idx, R.batch_key(3, epoch, cap, cursor), **rates))       # and the right one passes it
