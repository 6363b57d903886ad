"""CPU: the epoch feed's entry points refuse bad arguments before any launch, `trainer.ReduceOnPlateau` gives torch's rates, and
`EpochFeed` / `fit` refuse what they can refuse without a device."""
import ctypes
import itertools
import os
import types

import numpy as np
import pytest
import torch

from raindrop_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from raindrop_amd import build
        build.build(verbose=False)
    return _lib.load()


def test_feed_entry_points_check_their_arguments_before_launch(lib):
    one = ctypes.c_void_p(16)                                    # a non-NULL address that must never be dereferenced on the host
    # rd_feed_gather(T, B, W, d_static, N, capacity, 13 pointers)
    for dims in ((5, 2, 0, 0, 10, 4), (5, 2, 6, 0, 0, 4), (5, 2, 6, 0, 10, 0), (5, -1, 6, 0, 10, 4), (5, 2, 6, -1, 10, 4)):
        assert lib.rd_feed_gather(*dims, *([None] * 13)) == -1 and b"bad dims" in lib.rd_last_error(), dims
    assert lib.rd_feed_gather(5, 2, 6, 0, 10, 4, *([None] * 13)) == -1 and b"NULL" in lib.rd_last_error()
    # every required tensor on its own: P_all, time_all, y_all, plan, cell, src, times, y_out, lengths (static_*, bad may be NULL)
    for missing in (0, 1, 3, 4, 5, 6, 7, 9, 10):
        args = [one] * 12 + [None]
        args[2] = args[8] = None
        args[missing] = None
        assert lib.rd_feed_gather(5, 2, 6, 0, 10, 4, *args) == -1 and b"NULL" in lib.rd_last_error(), missing
    assert lib.rd_feed_gather(5, 0, 6, 0, 10, 4, *([None] * 13)) == 0
    # rd_feed_record(B, C, capacity, cell, loss, logits, y, loss_hist, correct_hist, stream)
    for dims in ((4, 0, 3), (4, 2, 0), (-1, 2, 3)):
        assert lib.rd_feed_record(*dims, *([None] * 7)) == -1 and b"bad dims" in lib.rd_last_error(), dims
    assert lib.rd_feed_record(4, 2, 3, *([None] * 7)) == -1 and b"NULL" in lib.rd_last_error()
    for missing in range(6):
        args = [one] * 6 + [None]
        args[missing] = None
        assert lib.rd_feed_record(4, 2, 3, *args) == -1 and b"NULL" in lib.rd_last_error(), missing
    assert lib.rd_feed_record(0, 2, 3, *([None] * 7)) == 0


def test_feed_kernels_use_no_scratch():
    from raindrop_amd import build
    build.build(verbose=False)
    hits = {k: v for k, v in build.resource_usage().items() if "k_feed_gather" in k or "k_feed_record" in k}
    assert len(hits) == 2, sorted(hits)
    for name, u in hits.items():
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0, (name, u)


# ---- ReduceOnPlateau against torch.optim.lr_scheduler.ReduceLROnPlateau -------------------------------------------------------------
def _sequences():
    rng = np.random.default_rng(11)
    up = [0.5 + 0.01 * k for k in range(12)]
    return {
        "improving": up,
        "worsening": up[::-1],
        "flat": [0.7] * 12,
        # around the relative / absolute threshold 1e-4 of a best near 0.7: steps of +-0.5, 1 and 2 thresholds
        "noisy": [0.7 + 1e-4 * 0.7 * d for d in rng.choice([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0], size=40)],
        # never better: the rate falls every patience + 1 epochs until min_lr and the eps rule stop it
        "to_min_lr": [0.3] * 60,
        "zero_and_nan": [0.0, 0.0, float("nan"), 0.2, 0.2, float("nan"), 0.1, 0.1],
    }


SETTINGS = [dict(),                                              # the script's: max, 0.1, patience 1, rel 1e-4, min_lr 1e-8, eps 1e-8
            dict(patience=0), dict(patience=2, cooldown=2), dict(factor=0.5, min_lr=1e-5, eps=1e-6),
            dict(factor=0.3, min_lr=0.0, eps=1e-4)]              # eps rule: the rate stops falling once a drop is smaller than eps


@pytest.mark.parametrize("mode,threshold_mode", list(itertools.product(("max", "min"), ("rel", "abs"))))
@pytest.mark.parametrize("setting", range(len(SETTINGS)))
@pytest.mark.parametrize("seq", list(_sequences()))
def test_reduce_on_plateau_gives_torchs_rates(seq, setting, mode, threshold_mode):
    from raindrop_amd.trainer import ReduceOnPlateau
    kw = dict(mode=mode, factor=0.1, patience=1, threshold=1e-4, threshold_mode=threshold_mode, cooldown=0, min_lr=1e-8, eps=1e-8)
    kw.update(SETTINGS[setting])
    p = torch.nn.Parameter(torch.zeros(1))
    sgd = torch.optim.SGD([p], lr=1e-3)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(sgd, **kw)
    opt = types.SimpleNamespace(lr=1e-3)
    ours = ReduceOnPlateau(opt, **kw)
    drops = 0
    for k, m in enumerate(_sequences()[seq]):
        ref.step(m)
        before = opt.lr
        assert ours.step(m) == opt.lr
        drops += opt.lr < before
        assert opt.lr == sgd.param_groups[0]["lr"], (k, m, opt.lr, sgd.param_groups[0]["lr"])
        assert ours.best == ref.best or (ours.best != ours.best and ref.best != ref.best)
        assert (ours.num_bad_epochs, ours.cooldown_counter) == (ref.num_bad_epochs, ref.cooldown_counter)
    if seq == "to_min_lr":                                       # it did reach the floor: min_lr, or where a drop would be < eps
        assert drops >= 2 and ours.step(0.3) == opt.lr == sgd.param_groups[0]["lr"]
        floor = kw["min_lr"]
        assert opt.lr == floor or opt.lr - max(opt.lr * kw["factor"], floor) <= kw["eps"]
    if seq == "improving" and mode == "max" or seq == "worsening" and mode == "min":
        assert drops == 0


def test_reduce_on_plateau_defaults_are_the_scripts():
    from raindrop_amd.trainer import ReduceOnPlateau
    s = ReduceOnPlateau()
    assert (s.mode, s.factor, s.patience, s.threshold, s.threshold_mode, s.cooldown, s.min_lr, s.eps) == \
        ("max", 0.1, 1, 1e-4, "rel", 0, 1e-8, 1e-8)
    for bad in (dict(factor=1.0), dict(mode="up"), dict(threshold_mode="x")):
        with pytest.raises(ValueError):
            ReduceOnPlateau(**bad)


# ---- host refusals --------------------------------------------------------------------------------------------------------------------
def _cpu_ds(y=True):
    """what EpochFeed / fit look at before they touch a device"""
    return types.SimpleNamespace(dev=torch.device("cpu"), y=torch.zeros(8, dtype=torch.int64) if y else None, N=8, T=5, W=6, ds=0,
                                 Pstatic=None)


def test_epoch_feed_needs_a_rocm_device():
    from raindrop_amd.feed import EpochFeed
    with pytest.raises(_lib.RaindropHipError, match="ROCm device"):
        EpochFeed(_cpu_ds(), 4, 2)


def test_fit_refuses_bad_arguments_without_a_device():
    from raindrop_amd.trainer import fit
    ds = _cpu_ds()
    for strategy in (0, 4, "2"):
        with pytest.raises(ValueError, match="strategy"):
            fit(None, ds, ds, 1, batch_size=8, strategy=strategy)
    for strategy in (1, 2):
        with pytest.raises(ValueError, match="even"):
            fit(None, ds, ds, 1, batch_size=7, strategy=strategy)
    with pytest.raises(ValueError, match="batch_size"):
        fit(None, ds, ds, 1, batch_size=0, strategy=3)
    with pytest.raises(_lib.RaindropHipError, match="train_ds carries no labels"):
        fit(None, _cpu_ds(y=False), ds, 1, batch_size=8)
    with pytest.raises(_lib.RaindropHipError, match="val_ds carries no labels"):
        fit(None, ds, _cpu_ds(y=False), 1, batch_size=8)
