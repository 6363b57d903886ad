"""The reference script's training loop (`code/Raindrop.py:256-381`) as one call on the captured path.

`fit` puts together what the library has: `feed.EpochPlanner` (the script's batch plan, same numpy calls), `feed.EpochFeed` (the
plan on the device), `TrainStep` / `BetaTrainStep` with the feed attached, `FlatAdam` inside `capture_full`, `feed.validate` and a
plateau scheduler.  An epoch is one upload of the plan, `n_batches` replays of ONE hipGraph and one read-back of the per-batch
losses and hit counts; validation is the captured evaluation pass.  `ReduceOnPlateau` restates torch's scheduler on the host:
`FlatAdam` keeps ONE base rate, `opt.lr`, which its parameter groups (`optim.ParamGroups`) scale on the device, not a list of
torch `param_groups` for torch's scheduler to act on.
"""
import math

import numpy as np
import torch

from . import _lib, dp, feed as feed_mod
from . import optim as optim_mod
from .optim import FlatAdam

VAL_FIELDS = ("auroc", "auprc", "loss", "accuracy", "precision", "recall", "f1")


class ReduceOnPlateau:
    """`torch.optim.lr_scheduler.ReduceLROnPlateau` for an optimizer that keeps its rate in `opt.lr` (FlatAdam): the same rule, the
    same float arithmetic, so the same rates.  The defaults are the script's (`code/Raindrop.py:257-259`).  `step(metric)` once per
    epoch; `opt` may be given later (`fit` binds its optimizer to a scheduler passed in without one)."""

    def __init__(self, opt=None, mode="max", factor=0.1, patience=1, threshold=1e-4, threshold_mode="rel", cooldown=0, min_lr=1e-8,
                 eps=1e-8):
        if factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        if mode not in ("min", "max"):
            raise ValueError("mode " + str(mode) + " is unknown!")
        if threshold_mode not in ("rel", "abs"):
            raise ValueError("threshold mode " + str(threshold_mode) + " is unknown!")
        self.opt, self.mode, self.factor, self.patience = opt, mode, factor, patience
        self.threshold, self.threshold_mode, self.cooldown, self.min_lr, self.eps = threshold, threshold_mode, cooldown, min_lr, eps
        self.best = math.inf if mode == "min" else -math.inf
        self.cooldown_counter = self.num_bad_epochs = self.last_epoch = 0

    def is_better(self, a, best):
        if self.mode == "min":
            return a < best * (1.0 - self.threshold) if self.threshold_mode == "rel" else a < best - self.threshold
        return a > best * (self.threshold + 1.0) if self.threshold_mode == "rel" else a > best + self.threshold

    def step(self, metric):
        current = float(metric)
        self.last_epoch += 1
        if self.is_better(current, self.best):
            self.best, self.num_bad_epochs = current, 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0                              # bad epochs in the cooldown do not count
        if self.num_bad_epochs > self.patience:
            old = float(self.opt.lr)
            new = max(old * self.factor, self.min_lr)
            if old - new > self.eps:
                self.opt.lr = new
            self.cooldown_counter, self.num_bad_epochs = self.cooldown, 0
        return float(self.opt.lr)


# what `fit(calibrate=True)` keeps of the final validation (feed.validate(calibration=, temperature="fit"))
CALIBRATION_KEYS = ("ece", "mce", "brier", "nll", "reliability", "reliability_counts", "ece_uncalibrated", "nll_uncalibrated", "temperature",
                    "temperature_status")


def _check_fit_args(train_ds, val_ds, epochs, batch_size, strategy, param_groups=None, decoupled_weight_decay=False, lr_schedule=None,
                    warmup_steps=0, accumulate=1, focal_gamma=None, label_smoothing=0.0, augment=None, bootstrap=None, bootstrap_seed=0,
                    calibrate=False, calibration_bins=15):
    """what can be refused without a device"""
    _resolve_augment(augment)
    feed_mod.check_bootstrap(bootstrap, bootstrap_seed)
    if not isinstance(calibrate, bool):
        raise ValueError("calibrate must be True or False, got %r" % (calibrate,))
    if calibration_bins is None:
        raise ValueError("calibration_bins must be an integer in [1, 256], got None")
    feed_mod.check_calibration(calibration_bins)
    if focal_gamma is not None:
        from .step import check_focal, focal_values
        focal_values(None, focal_gamma, 1)                                 # the range of gamma (the weights need the model's class count)
        check_focal(label_smoothing, focal_gamma)
    if isinstance(accumulate, bool) or not isinstance(accumulate, int) or accumulate < 1:
        raise ValueError("accumulate must be an integer >= 1, got %r" % (accumulate,))
    if isinstance(lr_schedule, str):
        if lr_schedule != "warmup_cosine":
            raise ValueError("lr_schedule: the only named schedule is 'warmup_cosine', got %r" % (lr_schedule,))
    elif lr_schedule is not None and not isinstance(lr_schedule, optim_mod.LRSchedule) and not callable(lr_schedule):
        raise ValueError("lr_schedule must be None, an optim.LRSchedule, 'warmup_cosine' or a callable total_steps -> LRSchedule, got %r"
                         % (lr_schedule,))
    if isinstance(warmup_steps, bool) or not isinstance(warmup_steps, int) or warmup_steps < 0:
        raise ValueError("warmup_steps must be a non-negative integer, got %r" % (warmup_steps,))
    if warmup_steps and lr_schedule != "warmup_cosine":
        raise ValueError("warmup_steps belongs to lr_schedule='warmup_cosine' (another schedule carries its own warm-up), got %r with %r"
                         % (warmup_steps, lr_schedule))
    if not isinstance(decoupled_weight_decay, bool):
        raise ValueError("decoupled_weight_decay must be True or False, got %r" % (decoupled_weight_decay,))
    if isinstance(param_groups, str):
        if param_groups != "no_decay":
            raise ValueError("param_groups: the only named recipe is 'no_decay', got %r" % (param_groups,))
    elif param_groups is not None:
        if not isinstance(param_groups, (list, tuple)) or not all(isinstance(r, dict) for r in param_groups):
            raise ValueError("param_groups must be None, 'no_decay' or a list of dict(match=..., lr_scale=1.0, weight_decay=None)")
        if len(param_groups) > optim_mod.GROUP_ROWS - 1:
            raise ValueError("param_groups: %d rules, at most %d" % (len(param_groups), optim_mod.GROUP_ROWS - 1))
        for k, r in enumerate(param_groups):
            if "match" not in r or set(r) - {"match", "lr_scale", "weight_decay"}:
                raise ValueError("param_groups[%d]: dict(match=..., lr_scale=1.0, weight_decay=None), got keys %s" % (k, sorted(r)))
            optim_mod._check_group_value("param_groups[%d]: lr_scale" % k, r.get("lr_scale", 1.0))
            if r.get("weight_decay") is not None:
                optim_mod._check_group_value("param_groups[%d]: weight_decay" % k, r["weight_decay"])
    if strategy not in (1, 2, 3):
        raise ValueError("strategy must be 1, 2 or 3, got %r" % (strategy,))
    if int(batch_size) != batch_size or batch_size <= 0:
        raise ValueError("batch_size must be a positive integer, got %r" % (batch_size,))
    if strategy in (1, 2) and batch_size % 2:
        raise ValueError("strategy %d draws batch_size / 2 samples of each class: batch_size must be even, got %d" % (strategy, batch_size))
    if int(epochs) != epochs or epochs < 0:
        raise ValueError("epochs must be a non-negative integer, got %r" % (epochs,))
    for name, ds in (("train_ds", train_ds), ("val_ds", val_ds)):
        if getattr(ds, "y", None) is None:
            raise _lib.RaindropHipError("fit: %s carries no labels (DeviceDataset(..., y=...))" % name)


def _resolve_augment(augment):
    """fit's `augment` as a feed.Augment (None: none); a dict holds Augment's keywords"""
    if augment is None or isinstance(augment, feed_mod.Augment):
        return augment
    if isinstance(augment, dict):
        unknown = set(augment) - {"p_time", "p_sensor", "p_obs", "value_noise", "seed"}
        if unknown:
            raise ValueError("augment: dict(p_time=0.0, p_sensor=0.0, p_obs=0.0, value_noise=0.0, seed=0), got keys %s" % sorted(augment))
        return feed_mod.Augment(**augment)
    raise ValueError("augment must be None, a feed.Augment or a dict of its keywords, got %r" % (augment,))


def _resolve_schedule(lr_schedule, warmup_steps, total_steps):
    """fit's `lr_schedule` as an LRSchedule for `total_steps` steps (None: none, also for a run of no steps)"""
    if lr_schedule is None or total_steps <= 0:
        return None
    if isinstance(lr_schedule, optim_mod.LRSchedule):
        return lr_schedule
    if lr_schedule == "warmup_cosine":
        if warmup_steps >= total_steps:
            raise ValueError("warmup_steps (%d) must be less than the run's %d steps" % (warmup_steps, total_steps))
        return optim_mod.LRSchedule.warmup_cosine(total_steps, warmup=warmup_steps)
    made = lr_schedule(total_steps)
    if not isinstance(made, optim_mod.LRSchedule):
        raise ValueError("lr_schedule(%d) must return an optim.LRSchedule, got %r" % (total_steps, made))
    return made


def _window_plan(n_batches, accumulate):
    """(optimizer steps, length of the last window) of an epoch of `n_batches` micro-batches taken `accumulate` at a time: every
    window but the last is full, the last one takes what is left (fit closes it with run_full(close_window=True)), none is dropped"""
    n, k = int(n_batches), int(accumulate)
    steps = -(-n // k)
    return steps, (n - (steps - 1) * k if steps else 0)


def _live_names(model):
    from . import synth
    cfg = dict(static=bool(model.static), nlayers=len(model.transformer_encoder.layers))
    return synth.live_parameter_names_beta(cfg) if getattr(model, "use_beta", False) else synth.live_parameter_names(cfg)


def fit(model, train_ds, val_ds, epochs, batch_size=128, strategy=2, lr=1e-4, weight_decay=0.0, max_grad_norm=None, ema_decay=None,
        class_weight=None, label_smoothing=0.0, distance_weight=0.0, transform="sigmoid", scheduler=True, seed=None, autotune=True,
        param_groups=None, decoupled_weight_decay=False, lr_schedule=None, warmup_steps=0, accumulate=1,
        focal_gamma=None, augment=None, bootstrap=None, bootstrap_seed=0, calibrate=False, calibration_bins=15):
    """Train `model` (raindrop_amd.models_rd.Raindrop_v2 on a ROCm device) on `train_ds` for `epochs` epochs, validating on `val_ds`
    after each (both `feed.DeviceDataset` with labels), the way the reference's script does (`code/Raindrop.py:256-381`):

    * batches: `feed.EpochPlanner(train labels, batch_size, strategy)` -- the script's numpy calls in the script's order, so
      `np.random.seed` before the call (or `seed=`, which also seeds the step's dropout stream) reproduces its batches;
    * the step: `TrainStep` (`BetaTrainStep` for a `use_beta` model, with `distance_weight`) on one `feed.EpochFeed`, `FlatAdam(lr,
      weight_decay, max_grad_norm, ema_decay)` inside `capture_full`; `class_weight` / `label_smoothing` set the criterion of the
      step and of the validation loss.  `param_groups` -- a list of `optim.ParamGroups` rules, `dict(match=..., lr_scale=1.0,
      weight_decay=None)`, or "no_decay" (`optim.no_decay`: biases and LayerNorm parameters without weight decay) -- and
      `decoupled_weight_decay` (AdamW) become the optimizer's `groups` / `decoupled`, built on the flat layout made here; the
      scheduler still moves the one base rate every group scales.  `lr_schedule` -- an `optim.LRSchedule`, "warmup_cosine"
      (`LRSchedule.warmup_cosine(total_steps, warmup=warmup_steps)`) or a callable total_steps -> LRSchedule, with total_steps =
      epochs x the planner's batches per epoch -- becomes the optimizer's `schedule`: a per-step rate formed on the device inside
      the captured step, `lr` (and the plateau scheduler) being the base rate it scales.  The model is put into training mode to build the step (that is when dropout is read) and
      gets its previous mode back at the end; evaluation runs with dropout off whatever the mode;
    * per epoch: `load_epoch`, `n_batches` x `run_full`, `feed.history()`; then `feed.validate(model, val_ds, transform=...)` (on the
      averaged weights, `validate_ema`, when `ema_decay` is set), the scheduler's step on `auprc` (:368) and, when `auroc` beats the
      best so far (:369-374), a device copy of the flat parameters (of their average when `ema_decay` is set: what was validated);
    * at the end the best copy goes back into the parameters (:381), so `feed.validate(model, val_ds)` gives `best_auroc` again.

    scheduler: True = `ReduceOnPlateau` with the script's settings, False / None = a constant rate, or a `ReduceOnPlateau` of your own.
    Returns a dict of per-epoch lists -- `train_loss` (the float32 mean of the epoch's per-batch losses), `train_accuracy`, `lr` (the
    rate after the epoch's scheduler step), `val_auroc`, `val_auprc`, `val_loss`, `val_accuracy`, `val_precision`, `val_recall`,
    `val_f1` -- plus `best_epoch` (None when no epoch's auroc exceeded 0) and `best_auroc`; with `lr_schedule` also `lr_step`, the
    device's rate after each epoch's last step (`lr` stays the base rate).

    accumulate=k > 1: gradient accumulation (`TrainStep(accumulate=k)`): every batch of the plan is a MICRO-batch, an optimizer step
    takes k of them (the mean of their gradients, each normalised by its own batch / class-weight sum), and an epoch's last window
    is closed where the plan ends (`run_full(close_window=True)`: the mean over the micro-batches it has), so no micro-batch is
    dropped and no gradient leaks into the next epoch.  Optimizer steps per epoch: ceil(n_batches / k); `lr_schedule` totals and
    `warmup_steps` count optimizer steps.  `train_loss` / `train_accuracy` stay means over the micro-batches.  The result gains
    `optimizer_steps` (the run's total), and `lr_step` then holds one entry per optimizer step: the rate that step applied (the
    double product the device forms), not one per epoch.  The plateau scheduler, validation and EMA validation are untouched.

    focal_gamma: a number in [0, 16] makes the criterion of the step AND of the validation loss the focal loss with `class_weight`
    (`TrainStep(focal_gamma=)`, `feed.validate(focal_gamma=)`); `label_smoothing` must then be 0.  None: as without it.

    augment: a `feed.Augment` (or a dict of its keywords) -- train-time input augmentation inside the TRAINING feed's gather
    (`EpochFeed(augment=)`: time-step, sensor and observation drop, value jitter; fresh masks every batch and epoch from
    (seed, epoch, cursor)).  Validation, the best-weights logic and every other path are untouched.  None: as without it.

    bootstrap=R (1 .. 4096; `val_ds` of at most 16384 samples): once, at the end, on the restored best weights (never per epoch),
    `feed.validate(model, val_ds, bootstrap=R, bootstrap_seed=bootstrap_seed)` with the run's transform and criterion, and the result
    gains `val_ci`: a dict of that validation's `auroc`, `auprc`, `auroc_ci`, `auprc_ci` (95 % percentile intervals), `auroc_se`,
    `auprc_se` and `bootstrap_valid`.  None: as without it.

    calibrate=True (`val_ds` of at most 16384 samples, at most 64 classes): once, at the end, on the restored best weights, beside the
    bootstrap, `feed.validate(model, val_ds, calibration=calibration_bins, temperature="fit")`, and the result gains `temperature` (the
    T fitted on the validation logits: pass it to `validate(test_ds, calibration=, temperature=T)`) and `val_calibration`: a dict of
    that validation's `ece`, `mce`, `brier`, `nll`, `reliability`, `reliability_counts`, `ece_uncalibrated`, `nll_uncalibrated`,
    `temperature` and `temperature_status`.  The calibrated figures are of the split the T was fitted on, so they are optimistic.
    False: as without it.

    One process, one GPU: data-parallel `fit` is not implemented (the feed itself works under data parallelism -- every rank loads
    its own plan rows -- but the planner, the scheduler and the best-checkpoint logic here do not coordinate ranks)."""
    _check_fit_args(train_ds, val_ds, epochs, batch_size, strategy, param_groups, decoupled_weight_decay, lr_schedule, warmup_steps,
                    accumulate, focal_gamma, label_smoothing, augment, bootstrap, bootstrap_seed, calibrate, calibration_bins)
    from .step import TrainStep
    from .step_beta import BetaTrainStep
    if seed is not None:
        np.random.seed(seed)
    B = int(batch_size)
    beta = bool(getattr(model, "use_beta", False))
    if distance_weight and not beta:
        raise ValueError("distance_weight belongs to a use_beta model")
    was_training = model.training
    model.train()
    named = dict(model.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in _live_names(model)], n_buckets=2)
    groups = None
    if param_groups is not None:
        groups = optim_mod.ParamGroups(flat, [optim_mod.no_decay(flat)] if param_groups == "no_decay" else param_groups)
    planner = feed_mod.EpochPlanner(train_ds.y.cpu().numpy(), batch_size=B, strategy=strategy, n_total=train_ds.N)
    schedule = _resolve_schedule(lr_schedule, warmup_steps, int(epochs) * _window_plan(planner.n_batches, accumulate)[0])
    opt = FlatAdam(flat.flatten_parameters(), lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm, ema_decay=ema_decay,
                   groups=groups, decoupled=decoupled_weight_decay, schedule=schedule)
    aug = _resolve_augment(augment)
    fd = feed_mod.EpochFeed(train_ds, B, max(int(planner.n_batches), 1), **({} if aug is None else dict(augment=aug)))
    P, Pstatic, Ptime, y, lengths = train_ds.batch(np.arange(B) % train_ds.N)          # valid contents for the step's checks
    batch = dict(src=P, static=Pstatic if model.static else None, times=Ptime, y=y, lengths=lengths)
    kw = dict(autotune=autotune, class_weight=class_weight, label_smoothing=label_smoothing, feed=fd)
    if seed is not None:
        kw["seed"] = int(seed)
    if accumulate > 1:                                                     # (1: the step as it was built before the keyword)
        kw["accumulate"] = accumulate
    if focal_gamma is not None:
        kw["focal_gamma"] = focal_gamma
    optimizer_steps = 0
    step = BetaTrainStep(model, flat, batch, distance_weight=distance_weight, **kw) if beta else TrainStep(model, flat, batch, **kw)
    sched = ReduceOnPlateau() if scheduler is True else (scheduler or None)
    if sched is not None and sched.opt is None:
        sched.opt = opt
    out = {k: [] for k in ("train_loss", "train_accuracy", "lr") + tuple("val_" + f for f in VAL_FIELDS)}
    if schedule is not None:
        out["lr_step"] = []
    best, best_auroc, best_epoch = None, 0.0, None
    vkw = dict(transform=transform, class_weight=class_weight, label_smoothing=label_smoothing)
    if focal_gamma is not None:
        vkw["focal_gamma"] = focal_gamma
    try:
        step.capture_full(opt)
        for epoch in range(int(epochs)):
            fd.load_epoch(planner.next_epoch())
            while fd.remaining():
                if accumulate == 1:
                    step.run_full()
                    continue
                step.run_full(close_window=fd.remaining() == 1)            # the plan's last micro-batch closes whatever window is open
                if step.window_closed:
                    optimizer_steps += 1
                    if schedule is not None:
                        out["lr_step"].append(opt._step_lr())
            loss, correct = fd.history()
            out["train_loss"].append(float(loss.mean()) if loss.size else float("nan"))
            out["train_accuracy"].append(float(correct.sum()) / max(correct.size * B, 1))
            if schedule is not None and accumulate == 1:
                out["lr_step"].append(opt.current_lr())
            v = feed_mod.validate_ema(model, val_ds, opt, **vkw) if ema_decay is not None else feed_mod.validate(model, val_ds, **vkw)
            for f in VAL_FIELDS:
                out["val_" + f].append(v[f])
            if sched is not None:
                sched.step(v["auprc"])
            out["lr"].append(float(opt.lr))
            if v["auroc"] > best_auroc:
                best_auroc, best_epoch = v["auroc"], epoch
                src = opt.ema if ema_decay is not None else opt.param.data
                best = src.clone() if best is None else best.copy_(src)
        if best is not None:
            opt.param.data.copy_(best)
        val_ci = None
        if bootstrap is not None:                                          # the parameters now hold what `best_auroc` was measured on
            v = feed_mod.validate(model, val_ds, bootstrap=int(bootstrap), bootstrap_seed=int(bootstrap_seed), **vkw)
            val_ci = {k: v[k] for k in ("auroc", "auprc", "auroc_ci", "auprc_ci", "auroc_se", "auprc_se", "bootstrap_valid")}
        val_cal = None
        if calibrate:
            v = feed_mod.validate(model, val_ds, calibration=int(calibration_bins), temperature="fit", **vkw)
            val_cal = {k: v[k] for k in CALIBRATION_KEYS}
    finally:
        step.close()
        model.train(was_training)
    out["best_epoch"], out["best_auroc"] = best_epoch, best_auroc
    if accumulate > 1:
        out["optimizer_steps"] = optimizer_steps
    if bootstrap is not None:
        out["val_ci"] = val_ci
    if calibrate:
        out["temperature"], out["val_calibration"] = val_cal["temperature"], val_cal
    return out
