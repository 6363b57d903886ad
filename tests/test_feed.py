"""Batch feed: host index plan vs the oracle / the reference's own lines (CPU), and the
device gather vs numpy fancy indexing, bit for bit (GPU)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import feed as O
from raindrop_amd import feed, synth


@pytest.mark.parametrize("strategy,bs", [(2, 128), (2, 6), (3, 128), (1, 8)])
def test_index_plan_matches_oracle(strategy, bs):
    rng = np.random.default_rng(3)
    y = (rng.random(1000) < 0.1).astype(np.int64)
    np.random.seed(11)
    got = feed.epoch_index_plan(y, bs, strategy)
    np.random.seed(11)
    exp = O.epoch_batches(y, bs, strategy)
    assert len(got) == len(exp) > 0
    for a, b in zip(got, exp):
        assert np.array_equal(a, b)
    if strategy == 2:                       # balanced halves, negatives first (Raindrop.py:303-305)
        assert all((y[b[:bs // 2]] == 0).all() and (y[b[bs // 2:]] == 1).all() for b in got)
        assert len(got) == min((y == 0).sum() // (bs // 2), 3 * (y == 1).sum() // (bs // 2))


RECORDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_records.npz")


def _reference_batches(name):
    """(labels, batch size, numpy seed, the reference's batches) of a case of tests/golden/make_reference_records.py FEED_CASES: the
    batches as recorded from the reference's OWN statements (the index bookkeeping of `code/Raindrop.py:261-307`); where the
    reference tree is present they are re-run from the script and must equal the record."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_reference_records as mk
    _, ls, n, rate, bs, seed, epochs = next(c for c in mk.FEED_CASES if c[0] == name)
    ytrain = mk.feed_labels(ls, n, rate)
    with np.load(RECORDS) as z:
        rec = z[name]
    if mk.script_available():
        assert np.array_equal(mk.feed_reference_batches(ytrain, bs, seed, epochs), rec)
    return ytrain, bs, seed, list(rec)


def test_index_plan_matches_reference_script_lines():
    """Pins the oracle: the reference's OWN statements for the strategy-2 plan, one epoch (recorded; re-run from the script
    where the reference tree is present)."""
    ytrain, bs, seed, ref_batches = _reference_batches("feed_plan_b128")
    np.random.seed(seed)
    mine = O.epoch_batches(ytrain, bs, 2)
    assert len(mine) == len(ref_batches) > 0
    for a, b in zip(mine, ref_batches):
        assert np.array_equal(a, b)


def test_epoch_planner_matches_reference_script_over_several_epochs():
    """The script shuffles `expanded_idx_1` / `idx_0` IN PLACE every epoch (`code/Raindrop.py:292-296`): epoch k's order is
    a permutation of epoch k-1's.  `feed.EpochPlanner` must reproduce the batches of every epoch, not only the first;
    checked against the reference's own statements executed in the script's nesting over three epochs (recorded; re-run from
    the script where the reference tree is present)."""
    ytrain, bs, seed, ref = _reference_batches("feed_epochs3_b64")
    np.random.seed(seed)
    planner = feed.EpochPlanner(ytrain, batch_size=bs, strategy=2)
    mine = [b for _ in range(3) for b in planner.next_epoch()]
    assert len(mine) == len(ref) == 3 * planner.n_batches > 0
    for a, b in zip(mine, ref):
        assert np.array_equal(a, b)
    np.random.seed(seed)
    first = feed.epoch_index_plan(ytrain, bs, 2)                 # the one-epoch helper: first epoch only
    assert all(np.array_equal(a, b) for a, b in zip(first, ref[: len(first)]))


def test_gather_oracle_is_fancy_indexing():
    rng = np.random.default_rng(0)
    P = rng.standard_normal((5, 9, 4)).astype(np.float32)
    Tm = np.maximum(rng.standard_normal((5, 9)), 0).astype(np.float32)
    idx = np.array([8, 0, 0, 3])
    Pb, Sb, Tb, yb, ln = O.gather_batch(P, Tm, None, None, idx)
    assert Pb.shape == (5, 4, 4) and Sb is None and yb is None
    assert np.array_equal(ln, (Tm[:, idx] > 0).sum(0)) and ln.dtype == np.int64


def test_device_dataset_refuses_cpu():
    from raindrop_amd import _lib
    with pytest.raises(_lib.RaindropHipError):
        feed.DeviceDataset(np.zeros((2, 3, 4), np.float32), np.zeros((2, 3), np.float32), device="cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,N,B", [("P19", 700, 256), ("PAM", 40, 17), ("TINY", 9, 1), ("P12", 64, 128)])
def test_batch_gather_bit_exact(cfg_name, N, B):
    cfg = synth.make_config(cfg_name)
    b = synth.make_batch(cfg, N, seed=5)
    P, Tm = b["src"].numpy(), b["times"].numpy()
    S = None if b["static"] is None else b["static"].numpy()
    y = b["y"].numpy()
    ds = feed.DeviceDataset(P, Tm, S, y)
    rng = np.random.default_rng(B)
    idx = rng.integers(0, N, size=B)                    # with repeats, like the 3x up-sampled positives
    Pb, Sb, Tb, yb, ln = ds.batch(idx)
    eP, eS, eT, ey, el = O.gather_batch(P, Tm, S, y, idx)
    assert ds.bad_indices() == 0
    assert np.array_equal(Pb.cpu().numpy(), eP) and np.array_equal(Tb.cpu().numpy(), eT)
    assert np.array_equal(ln.cpu().numpy(), el) and ln.dtype == torch.int64
    assert np.array_equal(yb.cpu().numpy(), ey)
    assert (Sb is None and eS is None) or np.array_equal(Sb.cpu().numpy(), eS)
    # buffers of a previous call are reused in place; device-side indices are clamped and counted
    out = ds.alloc(B)
    ds.batch(idx, out=out)
    assert np.array_equal(out["P"].cpu().numpy(), eP)
    bad = torch.tensor([N + 5] + [0] * (B - 1), dtype=torch.int64, device="cuda")
    ds.batch(bad, out=out)
    assert ds.bad_indices() == 1
    assert np.array_equal(out["P"][:, 0].cpu().numpy(), P[:, N - 1])
    with pytest.raises(IndexError):
        ds.batch(np.array([N]))


@pytest.mark.gpu
def test_feed_drives_the_model_and_chunked_eval_matches_one_forward():
    from tests.helpers import build_ours
    cfg = synth.make_config("P19")
    gs = synth.make_structure(cfg, "ones")
    N = 300
    b = synth.make_batch(cfg, N, seed=8)
    ds = feed.DeviceDataset(b["src"], b["times"], b["static"], b["y"])
    m = build_ours(cfg, gs, "cuda", 3).eval()
    np.random.seed(1)
    plan = feed.epoch_index_plan(b["y"].numpy(), batch_size=32, strategy=2)
    P, S, Tm, y, ln = ds.batch(plan[0])
    with torch.no_grad():
        out, _, _ = m(P, S, Tm, ln)
    assert out.shape == (32, 2) and torch.isfinite(out).all()
    full = feed.evaluate_chunked(m, ds, chunk=N)        # utils_rd.evaluate_standard: one forward
    parts = feed.evaluate_chunked(m, ds, chunk=128)
    assert full.shape == (N, 2) and torch.equal(full, parts)
