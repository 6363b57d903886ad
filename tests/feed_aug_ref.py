"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the augmenting batch gather (raindrop_amd/csrc/rd_feed_aug.hip; DESIGN §3e') on
top of tests/rng_ref.py: what rd_batch_gather_aug / rd_feed_gather_aug must write, bit for bit.

    key  = seed + draw (uint64, wrapping),  draw = epoch * capacity + cursor
    b: slot in the batch, t: row of the SOURCE sample, f: sensor; W = 2F, columns [0, F) values, [F, 2F) observed-indicators
    1. time-step drop   site 80, element b*T + t, candidates t < L = #{t : time[t] > 0}; all dropped -> all kept;
                        rows written: kept candidates in order, source rows [L, T) unchanged, then rows of +0.0
    2. sensor drop      site 81, element b*F + f
    3. observation drop site 82, element (t*B + b)*F + f
    4. jitter           site 83, the whole quad (t*B + b)*F + f: v' = fma(((u0 + u1) + (u2 + u3)) - 2, noise_c, v)
    keep iff u >= p (float32); a rate of 0 draws nothing.

`bug=` builds the deliberately WRONG kernels of tests/test_feed_aug_ref_host.py: each must fail `same`, the comparison the GPU test
makes."""
import numpy as np

from tests import rng_ref

SITE_FEED_TIME, SITE_FEED_SENSOR, SITE_FEED_OBS, SITE_FEED_NOISE = 80, 81, 82, 83
_M64 = 0xFFFFFFFFFFFFFFFF
BUGS = ("obs_output_row", "indicator_kept", "lengths_stale", "tail_dropped", "noise_unobserved", "no_epoch", "keep_gt", "stale_zero_rows")


def noise_c(sigma):
    """float32(sqrt(3) * sigma), formed in double and rounded once (raindrop_amd.feed.Augment.noise_c)"""
    return np.float32(np.sqrt(np.float64(3.0)) * np.float64(sigma))


def batch_key(seed, epoch, capacity, cursor, bug=None):
    draw = (0 if bug == "no_epoch" else int(epoch) * int(capacity)) + int(cursor)
    return (int(seed) + draw) & _M64


def _keep(key, site, idx, p, bug=None):
    if bug == "keep_gt":
        idx = rng_ref._u64(idx)
        u = rng_ref.uniform4(key, site, idx >> np.uint64(2))
        comp = (idx & np.uint64(3)).astype(np.int64)
        return np.take_along_axis(u, comp[..., None], axis=-1)[..., 0] > np.float32(p)
    return rng_ref.keep(key, site, idx, p)


def fma32(a, c, v):
    """float32(a * c + v) rounded ONCE, for float32 arrays a, v and a float32 scalar c where a holds at most 18 significant bits
    (here a = s - 2 with s a multiple of 2^-16 in [0, 4)).  Proof of the float64 route: a * c has at most 18 + 24 = 42 significant
    bits, so the double product is exact.  t = fl64(prod + v) may be inexact; TwoSum gives the exact error e = (prod + v) - t.  When
    e != 0 and t's last mantissa bit is even, t is replaced by its neighbour on e's side, whose last bit is odd: that is rounding to
    odd, and a value rounded to odd at 53 bits rounds to nearest at 24 bits (53 >= 24 + 2) exactly as the unrounded sum does --
    float32 subnormals included, where fewer bits are kept.  tests/test_feed_aug_ref_host.py checks it against `fractions`."""
    prod = a.astype(np.float64) * np.float64(c)
    v64 = v.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = prod + v64
        bb = t - prod
        e = (prod - (t - bb)) + (v64 - bb)                        # TwoSum (Knuth): exact for finite operands
        fix = np.isfinite(t) & (e != 0) & ((t.view(np.uint64) & np.uint64(1)) == 0)
        t = np.where(fix, np.nextafter(t, np.where(e > 0, np.inf, -np.inf)), t)
        return t.astype(np.float32)


def augment(P_all, time_all, idx, key, p_time=0.0, p_sensor=0.0, p_obs=0.0, noise_c=0.0, bug=None, fill=np.nan):
    """(src [T,B,W], times [T,B], lengths [B] int64) of the batch `idx` (indices inside [0, N)) under the batch key `key`.
    `fill`: what the output buffers hold beforehand (only the `stale_zero_rows` bug lets it show)."""
    P_all, time_all = np.asarray(P_all, dtype=np.float32), np.asarray(time_all, dtype=np.float32)
    T, N, W = P_all.shape
    assert W % 2 == 0
    F, B = W // 2, len(idx)
    src = np.full((T, B, W), fill, dtype=np.float32)
    times = np.full((T, B), fill, dtype=np.float32)
    lengths = np.zeros(B, dtype=np.int64)
    f = np.arange(F, dtype=np.int64)
    nc = np.float32(noise_c)
    for b in range(B):
        n = int(idx[b])
        tm = time_all[:, n]
        L = int((tm > 0).sum())
        rows = np.arange(T, dtype=np.int64)
        if p_time > 0:
            cand = np.arange(L, dtype=np.int64)
            keep = _keep(key, SITE_FEED_TIME, b * T + cand, p_time, bug) if L else np.zeros(0, dtype=bool)
            if not keep.any():
                keep = np.ones(L, dtype=bool)
            rows = cand[keep] if bug == "tail_dropped" else np.concatenate([cand[keep], np.arange(L, T, dtype=np.int64)])
        nr = len(rows)
        tq = np.arange(nr, dtype=np.int64) if bug == "obs_output_row" else rows       # the t of the obs / jitter numbering
        val, ind = P_all[rows, n, :F].copy(), P_all[rows, n, F:].copy()
        kill = np.zeros((nr, F), dtype=bool)
        if p_sensor > 0:
            kill |= ~_keep(key, SITE_FEED_SENSOR, b * F + f, p_sensor, bug)[None, :]
        elem = (tq[:, None] * B + b) * F + f[None, :]
        if p_obs > 0 and nr:
            kill |= ~_keep(key, SITE_FEED_OBS, elem, p_obs, bug)
        val[kill] = 0.0
        if bug != "indicator_kept":
            ind[kill] = 0.0
        if nc != 0 and nr:
            u = rng_ref.uniform4(key, SITE_FEED_NOISE, elem)
            s = (u[..., 0] + u[..., 1]) + (u[..., 2] + u[..., 3])                       # float32, exact: multiples of 2^-16 below 4
            on = ~kill if bug == "noise_unobserved" else (~kill & (ind != 0))
            val = np.where(on, fma32(s - np.float32(2.0), nc, val), val)
        src[:nr, b, :F], src[:nr, b, F:] = val, ind
        times[:nr, b] = tm[rows]
        if bug != "stale_zero_rows":
            src[nr:, b], times[nr:, b] = 0.0, 0.0
        lengths[b] = L if bug == "lengths_stale" else int((np.nan_to_num(times[:, b], nan=0.0) > 0).sum())
    return src, times, lengths


def same(a, b):
    """the GPU test's comparison: src and times bit for bit, lengths equal"""
    return (np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
            and np.array_equal(a[2], b[2]))
