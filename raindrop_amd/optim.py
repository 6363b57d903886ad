"""Adam over the flat parameter / gradient buffers (`raindrop_amd.dp.FlatGradAllReduce`).

`code/Raindrop.py:256` uses `torch.optim.Adam(model.parameters(), lr=1e-4)`; that keeps working
with this model unchanged.  `FlatAdam` is the fast path: because the live parameters and their
gradients already live in two flat buffers, the whole update is ONE elementwise HIP kernel
(rd_adam_step) instead of a 35-tensor multi-tensor launch.  Same formula as torch (no amsgrad).
"""
import contextlib
import ctypes
import math
import re

import torch

from . import _lib, ops


def _check_max_grad_norm(x):
    """a positive float, or math.inf (the non-finite guard alone)"""
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not x > 0:          # NaN fails `x > 0`
        raise ValueError("max_grad_norm must be None, a positive float or math.inf, got %r" % (x,))
    return float(x)


def _check_ema_decay(x):
    """a float in [0, 1)"""
    if isinstance(x, bool) or not isinstance(x, float) or not 0.0 <= x < 1.0:          # NaN fails the comparison
        raise ValueError("ema_decay must be None or a float in [0, 1), got %r" % (x,))
    return x


def _check_group_value(what, x):
    """a finite float >= 0 (a group's lr_scale or weight_decay)"""
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not 0.0 <= x < math.inf:          # NaN fails the comparison
        raise ValueError("%s must be a finite number >= 0, got %r" % (what, x))
    return float(x)


GROUP_CHUNK = 64         # elements per byte of the chunk map: the alignment dp.FlatGradAllReduce gives every tensor
GROUP_ROWS = 16          # rows of the group cell (include/raindrop_hip.h rd_adam_step_grp)


class ParamGroups:
    """A partition of a flat layout's tensors into at most 16 groups, each with its own `lr_scale` and `weight_decay`.

    layout: a `dp.FlatGradAllReduce` (anything with `names` and `slices`).  rules: a list of
    `dict(match=..., lr_scale=1.0, weight_decay=None)`; rule k makes group k + 1, group 0 is every tensor no rule matches.  `match`
    is a regular expression (`re.search` on the parameter's name), a callable name -> bool, or a list of names;
    `weight_decay=None`: the optimizer's (it follows later assignments of `opt.weight_decay`).
    Raises ValueError for a name that matches two rules, a rule that matches nothing, more than `max_groups - 1` rules, a negative or
    non-finite value, and a slice that does not start on a multiple of 64 (or shares a 64-element chunk with its neighbour).
    `chunk_map` (host, uint8): the group of elements [64c, 64c + 64); the padding behind a tensor has that tensor's group."""

    def __init__(self, layout, rules, max_groups=GROUP_ROWS):
        names, slices = list(layout.names), [(int(lo), int(hi)) for lo, hi in layout.slices]
        if not 1 <= max_groups <= GROUP_ROWS:
            raise ValueError("max_groups must be in 1..%d, got %r" % (GROUP_ROWS, max_groups))
        rules = list(rules)
        if len(rules) > max_groups - 1:
            raise ValueError("%d rules: at most %d (group 0 is what no rule matches)" % (len(rules), max_groups - 1))
        if len(names) != len(slices) or len(set(names)) != len(names):
            raise ValueError("the layout's names must be unique, one per slice")
        group_of = {}
        self.names, self.lr_scale, self.weight_decay = [[]], [1.0], [None]
        for k, rule in enumerate(rules):
            unknown = set(rule) - {"match", "lr_scale", "weight_decay"}
            if unknown or "match" not in rule:
                raise ValueError("rule %d: dict(match=..., lr_scale=1.0, weight_decay=None), got keys %s" % (k, sorted(rule)))
            match = rule["match"]
            if isinstance(match, str):
                hit = [n for n in names if re.search(match, n)]
            elif callable(match):
                hit = [n for n in names if match(n)]
            else:
                listed = list(match)
                missing = [n for n in listed if n not in names]
                if missing:
                    raise ValueError("rule %d names parameters the layout does not hold: %s" % (k, missing))
                hit = [n for n in names if n in listed]
            if not hit:
                raise ValueError("rule %d (%r) matches no parameter" % (k, match))
            twice = [n for n in hit if n in group_of]
            if twice:
                raise ValueError("rule %d and rule %d both match %s" % (group_of[twice[0]] - 1, k, twice))
            group_of.update((n, k + 1) for n in hit)
            wd = rule.get("weight_decay")
            self.names.append(hit)
            self.lr_scale.append(_check_group_value("rule %d: lr_scale" % k, rule.get("lr_scale", 1.0)))
            self.weight_decay.append(None if wd is None else _check_group_value("rule %d: weight_decay" % k, wd))
        self.names[0] = [n for n in names if n not in group_of]
        order = sorted(range(len(names)), key=lambda i: slices[i][0])
        self.n_chunks = max((hi + GROUP_CHUNK - 1) // GROUP_CHUNK for _, hi in slices) if slices else 0
        self.chunk_map = torch.zeros((self.n_chunks,), dtype=torch.uint8)
        for name, (lo, hi) in zip(names, slices):
            if lo % GROUP_CHUNK or lo < 0 or hi < lo:
                raise ValueError("%s starts at %d: every slice must start on a multiple of %d" % (name, lo, GROUP_CHUNK))
        for j, i in enumerate(order):
            lo, hi = slices[i]
            end = slices[order[j + 1]][0] if j + 1 < len(order) else self.n_chunks * GROUP_CHUNK
            if end < hi:
                raise ValueError("%s [%d, %d) overlaps the slice behind it, which starts at %d" % (names[i], lo, hi, end))
            self.chunk_map[lo // GROUP_CHUNK:end // GROUP_CHUNK] = group_of.get(names[i], 0)

    def __len__(self):
        return len(self.names)

    def partition(self):
        """the groups as tuples of names: what has to agree for a state dictionary to be loaded"""
        return tuple(tuple(g) for g in self.names)


def no_decay(layout):
    """the usual rule: no weight decay for every parameter with ndim <= 1 (biases, LayerNorm weights) of a `dp.FlatGradAllReduce`"""
    return dict(match=[n for n, p in zip(layout.names, layout.params) if p.dim() <= 1], weight_decay=0.0)


class LRSchedule:
    """A per-step learning-rate schedule as a TABLE of factors: step t (1-based) of an optimizer with base rate `lr` uses
    `lr * f[min(t - 1, n - 1)]` -- past the end the last factor holds.  An immutable float64 vector of finite, non-negative entries,
    length >= 1.  `FlatAdam(schedule=...)` keeps the table on the device, behind its step state, where the thread that forms the step
    number also forms the rate: no host work per step, inside a whole-step hipGraph too.  A table, not a formula: it is exact (the rate
    is ONE double product, the one `torch.optim.lr_scheduler.LambdaLR` forms from the same factor) and any schedule fits in it, at 8
    bytes per step.  The builders state their formulas with k = t - 1, the 0-based index."""

    __slots__ = ("_f",)

    def __init__(self, factors):
        if isinstance(factors, LRSchedule):
            f = factors._f
        else:
            if isinstance(factors, torch.Tensor):
                factors = factors.detach().cpu().flatten().tolist()
            try:
                f = tuple(factors)
            except TypeError:
                raise ValueError("LRSchedule: a sequence of factors, got %r" % (factors,))
            for x in f:
                if isinstance(x, bool) or not isinstance(x, (int, float)) or not 0.0 <= x < math.inf:          # NaN fails the comparison
                    raise ValueError("LRSchedule: every factor must be a finite number >= 0, got %r" % (x,))
            f = tuple(float(x) for x in f)
        if len(f) < 1:
            raise ValueError("LRSchedule: at least one factor")
        object.__setattr__(self, "_f", f)

    def __setattr__(self, name, value):
        raise AttributeError("LRSchedule is immutable")

    def __len__(self):
        return len(self._f)

    def __getitem__(self, k):
        return self._f[k]

    def __iter__(self):
        return iter(self._f)

    def __eq__(self, other):
        return isinstance(other, LRSchedule) and self._f == other._f

    def __hash__(self):
        return hash(self._f)

    def __repr__(self):
        return "LRSchedule(%d factors: %s%s)" % (len(self._f), ", ".join("%g" % x for x in self._f[:4]), ", ..." if len(self._f) > 4 else "")

    @property
    def factors(self):
        """the factors as a tuple of Python floats (doubles)"""
        return self._f

    def factor(self, t):
        """the factor of step t (1-based; t < 1 reads the first entry)"""
        return self._f[min(max(int(t) - 1, 0), len(self._f) - 1)]

    def tensor(self):
        """a fresh float64 CPU tensor of the factors"""
        return torch.tensor(self._f, dtype=torch.float64)

    @staticmethod
    def _count(what, x, least=1):
        if isinstance(x, bool) or not isinstance(x, int) or x < least:
            raise ValueError("%s must be an integer >= %d, got %r" % (what, least, x))
        return x

    @classmethod
    def linear_warmup(cls, warmup, start=0.0):
        """`warmup` entries: f[k] = start + (1 - start) (k + 1) / warmup for k < warmup - 1, f[warmup - 1] = 1 (which then holds)"""
        cls._count("warmup", warmup)
        start = _check_group_value("start", start)
        return cls([1.0 if k + 1 >= warmup else start + (1.0 - start) * (k + 1) / warmup for k in range(warmup)])

    @classmethod
    def warmup_cosine(cls, total, warmup=0, min_factor=0.0):
        """`total` entries: f[k] = (k + 1) / warmup for k < warmup, then min_factor + (1 - min_factor) (1 + cos(pi x)) / 2 with
        x = (k - warmup) / max(1, total - 1 - warmup): 1 at k = warmup, min_factor at the last entry (which then holds)"""
        cls._count("total", total)
        cls._count("warmup", warmup, 0)
        if warmup >= total:
            raise ValueError("warmup_cosine: warmup (%d) must be less than total (%d)" % (warmup, total))
        lo = _check_group_value("min_factor", min_factor)
        span = max(1, total - 1 - warmup)
        return cls([(k + 1) / warmup if k < warmup else lo + (1.0 - lo) * 0.5 * (1.0 + math.cos(math.pi * ((k - warmup) / span)))
                    for k in range(total)])

    @classmethod
    def step_decay(cls, step_size, gamma, total):
        """`total` entries: f[k] = gamma ** (k // step_size) (torch's StepLR in closed form)"""
        cls._count("step_size", step_size)
        cls._count("total", total)
        gamma = _check_group_value("gamma", gamma)
        return cls([gamma ** (k // step_size) for k in range(total)])

    @classmethod
    def one_cycle(cls, total, pct_start=0.3, div=25.0, final_div=1e4):
        """`total` >= 2 entries, the RATE of torch's OneCycleLR (cosine annealing, two phases) with the base rate as its max_lr: from
        1 / div up to 1 at k = u = pct_start total - 1, then down to 1 / (div final_div) at the last entry;
        f = b + (a - b) (1 + cos(pi x)) / 2 from a to b, x = k / u in the first phase and (k - u) / (total - 1 - u) in the second.
        (The momentum half of the policy is not here: beta1 is a launch argument.)"""
        cls._count("total", total, 2)
        if isinstance(pct_start, bool) or not isinstance(pct_start, float) or not 0.0 < pct_start < 1.0:
            raise ValueError("pct_start must be a float in (0, 1), got %r" % (pct_start,))
        for what, x in (("div", div), ("final_div", final_div)):
            if isinstance(x, bool) or not isinstance(x, (int, float)) or not 1.0 <= x < math.inf:
                raise ValueError("%s must be a finite number >= 1, got %r" % (what, x))
        up_end, end = float(pct_start * total) - 1.0, float(total - 1)
        first, last = 1.0 / div, 1.0 / div / final_div

        def anneal(a, b, x):
            return b + (a - b) / 2.0 * (math.cos(math.pi * x) + 1.0)
        return cls([anneal(first, 1.0, k / up_end if up_end > 0.0 else 1.0) if k <= up_end else anneal(1.0, last, (k - up_end) / (end - up_end))
                    for k in range(total)])

    @classmethod
    def from_lambda(cls, fn, total):
        """f[k] = fn(k), k = 0 .. total - 1: the function one would hand to torch's LambdaLR"""
        cls._count("total", total)
        if not callable(fn):
            raise ValueError("from_lambda: fn must be callable, got %r" % (fn,))
        return cls([fn(k) for k in range(total)])

    @classmethod
    def from_torch(cls, make_scheduler, total):
        """Any torch scheduler as a table: `make_scheduler(optimizer)` builds it on a dummy one-parameter CPU optimizer with lr = 1.0;
        f[k] is the rate that optimizer's step k + 1 would use (the rate in front of the k-th `scheduler.step()`).  torch's chainable
        schedulers form their rates recursively: at another base rate torch's own doubles can differ from base * f[k] in the last
        bit."""
        cls._count("total", total)
        if not callable(make_scheduler):
            raise ValueError("from_torch: make_scheduler must be callable (optimizer -> scheduler), got %r" % (make_scheduler,))
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
        sched = make_scheduler(opt)
        rates = []
        for k in range(total):
            rates.append(float(opt.param_groups[0]["lr"]))
            if k + 1 < total:
                opt.step()
                sched.step()
        return cls(rates)


def _check_schedule(schedule, capacity):
    """(schedule, capacity) of FlatAdam's keywords: (None, None) is off; a capacity alone is the table {1.0} in that much room"""
    if schedule is None and capacity is None:
        return None, None
    if schedule is None:
        schedule = LRSchedule([1.0])
    if not isinstance(schedule, LRSchedule):
        raise ValueError("schedule must be None or an optim.LRSchedule, got %r" % (schedule,))
    if capacity is None:
        capacity = len(schedule)
    if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < len(schedule):
        raise ValueError("schedule_capacity must be an integer >= the schedule's length (%d), got %r" % (len(schedule), capacity))
    return schedule, capacity


class FlatAdam:
    """Adam over the flat buffers; `step()` with host-computed bias corrections, `step_captured()` with the step state on the device.

    max_grad_norm (default None: off -- the launches and the code path of an optimizer built without the keyword): global-norm
    gradient clipping and a non-finite guard INSIDE the step, so that they also exist in a whole-step hipGraph
    (`TrainStep.capture_full`).  A positive float clips like `torch.nn.utils.clip_grad_norm_(params, max_grad_norm)` in front of
    `step()`: the raw gradient is multiplied by min(1, max_norm / (norm + 1e-6)), weight decay is added afterwards; `math.inf` keeps
    only the guard.  On, a step is two launches instead of one (rd_grad_sumsq, rd_adam_step_clip[_dev]); at N > 1 they follow the
    all-reduce, so the norm is that of the averaged gradient and the same bits on every rank.  The threshold lives in a device
    cell: `set_max_grad_norm(x)` (or assigning `max_grad_norm` before `TrainStep.run_full`) is an 8-byte copy, not a new capture.
    `grad_stats()` reads the last norm and scale and the counts of skipped and clipped steps.

    A step whose gradient holds an inf or a NaN is SKIPPED: parameters, exp_avg and exp_avg_sq keep their bits.  It still COUNTS
    as a step: `t` and the device step state {t, beta^t} advance (the state is advanced by the step's first launch, long before
    the norm is known), so `self.t == device_steps()` always holds and the bias corrections of later steps are those of t + 1.
    torch.amp's GradScaler does NOT count a skipped step; after k skips the corrections here are k steps ahead of a GradScaler
    loop's (they tend to 1 either way).

    ema_decay (default None: off -- the launches, the code path, `hyper()` and the `state_dict()` keys of an optimizer built without
    the keyword): an exponential moving average of the flat parameters, `self.ema`, kept INSIDE the update's launch (the EMA twins
    rd_adam_step[_clip]_ema[_dev]: the thread that wrote p_new does ema += (1 - d_t)(p_new - ema) in fp32), so it exists in
    `step()`, `step_captured()` and a whole-step hipGraph alike, with no launch added; it combines with `max_grad_norm`.  `ema`
    starts as a copy of the parameters (torch.optim.swa_utils.AveragedModel's first call).  d_t = ema_decay, or with
    `ema_warmup=True` min(ema_decay, (1 + k) / (10 + k)) with k the number of EMA updates so far, counted on the device
    (`ema_updates()`): a step the non-finite guard skips leaves `ema` untouched and is not counted.  The decay lives in a device
    cell: `set_ema_decay(d)` (or assigning `ema_decay` before `TrainStep.run_full`) is an 8-byte copy, not a new capture; switching
    averaging on or off, or the warm-up, is a new capture / another optimizer.
    `swap_ema()` exchanges parameters and average IN PLACE (rd_swap_f32): whatever holds the parameters' addresses -- a captured
    `EvalStep`, `feed.validate`, the eager forward -- then evaluates the average; `ema_weights()` is the context manager around two
    swaps.  While swapped, `step()` / `step_captured()` (and the whole-step replays) raise instead of training the average.
    The average covers the flat parameters, which is everything: the model has no buffers (no batch-norm statistics).

    groups, decoupled (default None, False: off -- the launches, the code path, `hyper()` and the `state_dict()` keys of an optimizer
    built without the keywords): `groups` is a `ParamGroups` over the layout the flat buffers come from; every group has its own
    learning rate `lr * lr_scale` and its own weight decay (None: the optimizer's `weight_decay`), applied by the update's own launch
    (the _grp twins rd_adam_step[_clip][_ema]_grp[_dev]: one byte per 64 elements names the group, a 16-row device cell holds the
    scalars), so they exist in `step()`, `step_captured()` and a whole-step hipGraph alike and combine with `max_grad_norm` and
    `ema_decay`.  `decoupled=True` is torch.optim.AdamW: p *= 1 - lr * weight_decay in front of the Adam step instead of
    weight_decay * p added to the gradient; without `groups` it runs the grouped forms with one group.  The clipping norm stays the
    GLOBAL norm over all groups, the step count and the average are shared.  `set_group(i, lr_scale=, weight_decay=)` is a copy of
    one 32-byte row, stream-ordered with the launches around it and not a new capture (lr_scale=0.0 holds a group still: its
    parameters keep their bits, its moments go on); assigning `weight_decay` re-resolves the rows of the groups that follow it at
    the next `sync_cells`.  Switching the feature on or off is a new capture / another optimizer.

    schedule, schedule_capacity (default None, None: off -- the eight-double step cell, `hyper()` and the `state_dict()` keys of an
    optimizer built without the keywords): an `LRSchedule`, the rate of step t is `lr * f[min(t - 1, n - 1)]`.  `lr` stays the BASE
    rate -- what the user and `trainer.ReduceOnPlateau` assign.  The table lives behind the device step state (8 + capacity doubles) and
    the one thread that advances that state per step (rd_adam_state_advance, or the first launch of a whole-step hipGraph) also writes
    the step's rate into the slot every update kernel reads: no launch, no argument and no host work per step is added, and the
    feature combines with `max_grad_norm`, `ema_decay`, `groups` (every group scales the scheduled rate) and `decoupled` (the shrink
    uses the scheduled rate, as torch's AdamW under a scheduler) with no code of their own.  `step()` passes the same double product
    as its `lr` argument: the same bits.  A step the non-finite guard skips still moves the position (it moves `t`).  The capacity
    (default: the schedule's length) is fixed for the optimizer's life -- a captured graph holds the cell's address --:
    `set_schedule(s)` with len(s) <= capacity is one stream-ordered copy and not a new capture, a longer one raises,
    `clear_schedule()` installs the table {1.0}.  `schedule_capacity` alone switches the feature on with that table.
    `current_lr()` reads the device's rate back, `schedule_position()` is min(t, n)."""

    def __init__(self, flat_param, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, ema_decay=None,
                 ema_warmup=False, groups=None, decoupled=False, schedule=None, schedule_capacity=None):
        if flat_param.grad is None:
            raise ValueError("flat_param.grad must be the flat gradient buffer")
        if groups is not None and not isinstance(groups, ParamGroups):
            raise ValueError("groups must be None or an optim.ParamGroups, got %r" % (groups,))
        self.groups, self.decoupled = groups, bool(decoupled)
        self.chunk_group = self.group_cell = None
        self.schedule, self.schedule_capacity = _check_schedule(schedule, schedule_capacity)
        self.max_grad_norm = None if max_grad_norm is None else _check_max_grad_norm(max_grad_norm)
        self.clip_cell = self.clip_partial = None
        self.ema_decay = None if ema_decay is None else _check_ema_decay(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.ema = self.ema_cell = None
        self.ema_swapped = False
        self.param = flat_param
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.exp_avg = torch.zeros_like(flat_param.data)
        self.exp_avg_sq = torch.zeros_like(flat_param.data)
        self.t = 0
        self.step_cell = None                # device step state of the captured form (step_captured)
        self._cell_stale = False
        if self.max_grad_norm is not None:
            self._make_clip_buffers()
        if self.ema_decay is not None:
            self._make_ema_buffers()
        if self.groups is not None or self.decoupled:
            self._make_group_buffers()

    def hyper(self):
        """the values a captured launch holds as CONSTANTS (TrainStep.run_full captures again when they change): betas and eps, and
        whether the clipping launches are there at all.  lr and weight_decay live in the device step cell (cell_hyper), the
        clipping threshold in the clip cell: changing them is a small copy, not a new capture."""
        h = (float(self.betas[0]), float(self.betas[1]), float(self.eps))
        if self.max_grad_norm is not None:
            h = h + ("clip",)
        if self.ema_decay is not None:                                   # the EMA twin of the update is another launch
            h = h + ("ema",)
        return h if self.chunk_group is None else h + ("grp",)           # and so is the grouped twin

    def cell_hyper(self):
        return (float(self.lr), float(self.weight_decay))

    # ---- gradient clipping / non-finite guard (max_grad_norm) ----
    def _make_clip_buffers(self):
        """the clip cell {max_norm, last_norm, last_scale, skipped, clipped, 0, 0, 0} (include/raindrop_hip.h rd_adam_step_clip) and
        the partial sums of rd_grad_sumsq; made outside any capture (the constructor, load_state_dict)"""
        dev = self.param.device
        self.clip_partial = torch.zeros((int(_lib.load().rd_grad_sumsq_bytes()) // 8,), dtype=torch.float64, device=dev)
        self.clip_cell = torch.tensor([self.max_grad_norm] + [0.0] * 7, dtype=torch.float64).to(dev)
        self._cell_max_norm = self.max_grad_norm

    def _clip_args(self):
        self.sync_clip_cell()
        return (ops._ptr(self.clip_partial), self.clip_partial.numel() * 8, ops._ptr(self.clip_cell))

    def set_max_grad_norm(self, x):
        """A new threshold (positive float or math.inf) for the steps enqueued from here on, captured ones included: one 8-byte
        copy into the clip cell, stream-ordered with the launches around it."""
        if self.max_grad_norm is None:
            raise ValueError("clipping is off: construct FlatAdam with max_grad_norm (the step's launches differ)")
        self.max_grad_norm = _check_max_grad_norm(x)
        self.sync_clip_cell()

    def sync_clip_cell(self):
        """push a changed `max_grad_norm` into the clip cell (part of sync_cells)"""
        if self.clip_cell is not None and self.max_grad_norm is not None and self._cell_max_norm != self.max_grad_norm:
            self.clip_cell[0:1] = torch.tensor([_check_max_grad_norm(self.max_grad_norm)], dtype=torch.float64,
                                               device=self.clip_cell.device)
            self._cell_max_norm = self.max_grad_norm

    def grad_stats(self):
        """dict(norm, scale, skipped, clipped) of the steps so far -- the last step's gradient norm and the factor applied to it (0.0:
        the step was skipped), and how many steps were skipped / clipped: ONE device-to-host copy (it waits for the stream)."""
        if self.clip_cell is None:
            raise ValueError("clipping is off: construct FlatAdam with max_grad_norm")
        c = self.clip_cell.cpu().tolist()
        return dict(norm=c[1], scale=c[2], skipped=int(c[3]), clipped=int(c[4]))

    # ---- parameter groups / decoupled weight decay (groups, decoupled) ----
    def _make_group_buffers(self):
        """the chunk map (one byte per 64 elements) and the group cell, 16 rows {lr_scale, wd_coupled, wd_decoupled, 0}
        (include/raindrop_hip.h rd_adam_step_grp); made outside any capture (the constructor)"""
        n_chunks = (self.param.numel() + GROUP_CHUNK - 1) // GROUP_CHUNK
        if self.groups is None:              # decoupled alone: one group, everything follows the optimizer
            cmap, self._group_lr_scale, self._group_wd = torch.zeros((n_chunks,), dtype=torch.uint8), [1.0], [None]
        else:
            cmap, self._group_lr_scale, self._group_wd = self.groups.chunk_map, list(self.groups.lr_scale), list(self.groups.weight_decay)
            if cmap.numel() != n_chunks:
                raise ValueError("groups cover %d chunks of %d elements, the flat buffer has %d: another layout?"
                                 % (cmap.numel(), GROUP_CHUNK, n_chunks))
        dev = self.param.device
        self.chunk_group = cmap.to(dev)
        self.group_cell = torch.tensor(self._group_rows(), dtype=torch.float64).to(dev)
        self._cell_group_wd = self.weight_decay

    def _group_row(self, i):
        wd = self.weight_decay if self._group_wd[i] is None else self._group_wd[i]
        wd = _check_group_value("weight_decay", wd)
        return [self._group_lr_scale[i], 0.0, wd, 0.0] if self.decoupled else [self._group_lr_scale[i], wd, 0.0, 0.0]

    def _group_rows(self):
        """all 16 rows; the rows behind the last group stay zero (no map the host builds names them)"""
        k = len(self._group_wd)
        return [self._group_row(i) for i in range(k)] + [[0.0] * 4] * (GROUP_ROWS - k)

    def _groups_on(self):
        if self.group_cell is None:
            raise ValueError("parameter groups are off: construct FlatAdam with groups or decoupled=True (the step's launches differ)")

    def _group_args(self):
        self.sync_group_cell()
        return (ops._ptr(self.chunk_group), ops._ptr(self.group_cell))

    def _write_group_row(self, i):
        self.group_cell[i] = torch.tensor(self._group_row(i), dtype=torch.float64, device=self.group_cell.device)

    def set_group(self, i, lr_scale=None, weight_decay=None):
        """New scalars for group i, for the steps enqueued from here on, captured ones included: one 32-byte copy into the group
        cell, stream-ordered with the launches around it.  None leaves a value as it is; a `weight_decay` given here stops
        following the optimizer's."""
        self._groups_on()
        if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < len(self._group_wd):
            raise ValueError("group %r: the optimizer has groups 0..%d" % (i, len(self._group_wd) - 1))
        if lr_scale is not None:
            lr_scale = _check_group_value("lr_scale", lr_scale)
        if weight_decay is not None:
            weight_decay = _check_group_value("weight_decay", weight_decay)
        self.sync_group_cell()
        if lr_scale is not None:
            self._group_lr_scale[i] = lr_scale
        if weight_decay is not None:
            self._group_wd[i] = weight_decay
        self._write_group_row(i)

    def sync_group_cell(self):
        """push a changed `weight_decay` into the rows of the groups that follow it (part of sync_cells)"""
        if self.group_cell is not None and self._cell_group_wd != self.weight_decay:
            for i, wd in enumerate(self._group_wd):
                if wd is None:
                    self._write_group_row(i)
            self._cell_group_wd = self.weight_decay

    def group_info(self):
        """per group: dict(names, lr_scale, weight_decay) with the decay resolved (a group that follows the optimizer's shows it)"""
        self._groups_on()
        names = self.groups.names if self.groups is not None else [None]
        return [dict(names=None if names[i] is None else list(names[i]), lr_scale=self._group_lr_scale[i],
                     weight_decay=float(self.weight_decay if wd is None else wd)) for i, wd in enumerate(self._group_wd)]

    # ---- exponential moving average of the weights (ema_decay) ----
    def _make_ema_buffers(self, updates=0):
        """`ema` = a copy of the flat parameters, and the EMA cell {d, warm-up, k, k, 0, 0, 0, 0} (include/raindrop_hip.h
        rd_adam_step_ema); made outside any capture (the constructor, load_state_dict)"""
        self.ema = self.param.data.detach().clone()
        self.ema_cell = torch.tensor([self.ema_decay, float(self.ema_warmup), float(updates), float(updates)] + [0.0] * 4,
                                     dtype=torch.float64).to(self.param.device)
        self._cell_ema_decay = self.ema_decay
        self._ema_t = self.t

    def _ema_on(self):
        if self.ema_decay is None or self.ema is None:
            raise ValueError("weight averaging is off: construct FlatAdam with ema_decay (the step's launches differ)")

    def _ema_args(self):
        self.sync_ema_cell()
        return (ops._ptr(self.ema), ops._ptr(self.ema_cell))

    def check_can_step(self, what):
        """raises while the parameters are exchanged with their average; `what`: the caller, for the message"""
        if self.ema_swapped:
            raise _lib.RaindropHipError("%s: the parameters are exchanged with their average (FlatAdam.swap_ema / ema_weights): a "
                                        "step now would train the averaged weights -- swap back first" % what)

    def set_ema_decay(self, d):
        """A new decay (float in [0, 1)) for the steps enqueued from here on, captured ones included: one 8-byte copy into the EMA
        cell, stream-ordered with the launches around it."""
        self._ema_on()
        self.ema_decay = _check_ema_decay(d)
        self.sync_ema_cell()

    def sync_ema_cell(self):
        """push a changed `ema_decay` into the EMA cell (part of sync_cells), and keep the count
        readable when `t` was set from outside (load_state_dict, a restored snapshot): the launches keep the count in the slot the
        NEXT step number's parity selects, so after a jump of `t` the current count is copied into both slots, on the device."""
        if self.ema_cell is None or self.ema_decay is None:
            return
        if self._cell_ema_decay != self.ema_decay:
            self.ema_cell[0:1] = torch.tensor([_check_ema_decay(self.ema_decay)], dtype=torch.float64, device=self.ema_cell.device)
            self._cell_ema_decay = self.ema_decay
        if self._ema_t != self.t:
            cur = 2 + ((self._ema_t + 1) & 1)
            self.ema_cell[2:4] = self.ema_cell[cur:cur + 1].clone()
            self._ema_t = self.t

    def ema_updates(self):
        """updates of the average so far according to the device (skipped steps are not counted): one device-to-host copy"""
        self._ema_on()
        return int(self.ema_cell.cpu().tolist()[2 + ((self._ema_t + 1) & 1)])

    def swap_ema(self):
        """Exchange the flat parameters and their average in place (rd_swap_f32; stream-ordered, capturable): every holder of a
        parameter address sees the other set.  Steps raise until the next swap."""
        self._ema_on()
        _lib.call("rd_swap_f32", self.param.numel(), ops._ptr(self.param.data), ops._ptr(self.ema), ops._stream())
        self.ema_swapped = not self.ema_swapped

    @contextlib.contextmanager
    def ema_weights(self):
        """`with opt.ema_weights(): ...` -- the model (and every captured step that reads its parameters) holds the averaged weights
        inside the block and the training weights, bit for bit, after it."""
        if self.ema_swapped:
            raise _lib.RaindropHipError("FlatAdam.ema_weights: already swapped")
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    # ---- per-step learning-rate schedule (schedule, schedule_capacity) ----
    def _schedule_on(self):
        if self.schedule is None:
            raise ValueError("the learning-rate schedule is off: construct FlatAdam with schedule or schedule_capacity (the step "
                             "cell's size is fixed for the optimizer's life)")

    def _step_lr(self):
        """the rate of step `self.t` as the host forms pass it: the double product the device forms, or the base rate"""
        return float(self.lr) if self.schedule is None else float(float(self.lr) * self.schedule.factor(self.t))

    def _schedule_words(self):
        """{n, 0, f[0 .. n)}: slots 6, 7 and the table, as one contiguous piece of the cell"""
        return [float(len(self.schedule)), 0.0] + list(self.schedule.factors)

    def set_schedule(self, schedule):
        """Another table for the steps enqueued from here on, captured ones included (the position, `t`, stays): one copy into the step
        cell, stream-ordered with the launches around it, not a new capture.  Raises for one longer than `schedule_capacity`."""
        self._schedule_on()
        if not isinstance(schedule, LRSchedule):
            raise ValueError("set_schedule: an optim.LRSchedule, got %r" % (schedule,))
        if len(schedule) > self.schedule_capacity:
            raise ValueError("set_schedule: %d entries, the capacity is %d and fixed (a captured graph holds the cell's address): "
                             "construct FlatAdam with a larger schedule_capacity" % (len(schedule), self.schedule_capacity))
        self.schedule = schedule
        if self.step_cell is not None:
            words = self._schedule_words()
            self.step_cell[6:6 + len(words)] = torch.tensor(words, dtype=torch.float64, device=self.step_cell.device)

    def _check_step_cell(self, what):
        """in front of a launch that advances the step state: the advancing thread trusts slot 6 (the C entry points take no
        length), so the cell must be the 8 + capacity doubles made here and the table must fit -- whatever was assigned from outside"""
        words = 8 + (self.schedule_capacity or 0)
        if self.step_cell.numel() != words or self.step_cell.dtype != torch.float64 or \
                (self.schedule is not None and not (isinstance(self.schedule, LRSchedule) and len(self.schedule) <= self.schedule_capacity)):
            raise _lib.RaindropHipError("%s: the step cell must hold %d doubles and a schedule of at most %s entries (use set_schedule)"
                                        % (what, words, self.schedule_capacity))

    def clear_schedule(self):
        """the table {1.0}: every step from here on uses the base rate (the feature, and the cell, stay)"""
        self.set_schedule(LRSchedule([1.0]))

    def current_lr(self):
        """the rate of the last step applied (before any: of the first): slot 3 of the device step state, one device-to-host copy (it
        waits for the stream) -- or, while host-form steps have left that state behind, the product `step()` passed"""
        if self.step_cell is None or self._cell_stale:
            return self._step_lr()
        return float(self.step_cell[3])

    def schedule_position(self):
        """entries of the table consumed so far: min(t, n)"""
        self._schedule_on()
        return min(int(self.t), len(self.schedule))

    def _enqueue_update(self, dev):
        """The update's launches -- the ONE place that names the sixteen entry points: rd_adam_step [_clip] [_ema] [_grp] [_dev], behind
        rd_grad_sumsq when clipping is on.  dev: the step state is read from the device cell, else `lr`, `weight_decay` and `t` of
        this step travel as arguments.  The cells of what is on are synchronised on the way (the average's, then the threshold's)."""
        clip, ema, grp = self.max_grad_norm is not None, self.ema_decay is not None, self.chunk_group is not None
        p, g = self.param.data, self.param.grad
        args = (p.numel(), ops._ptr(p), ops._ptr(g), ops._ptr(self.exp_avg), ops._ptr(self.exp_avg_sq))
        if dev:
            args += (float(self.betas[0]), float(self.betas[1]), float(self.eps), ops._ptr(self.step_cell))
        else:
            args += (self._step_lr(), float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay), self.t)
        tail = (self._ema_args() if ema else ()) + (self._group_args() if grp else ())
        if clip:                             # the norm's partial sums, then the clipping instantiation of the update
            partial, nbytes, cell = self._clip_args()
            _lib.call("rd_grad_sumsq", p.numel(), ops._ptr(g), partial, nbytes, ops._stream())
            args += (partial, nbytes, cell)
        _lib.call("rd_adam_step" + "_clip" * clip + "_ema" * ema + "_grp" * grp + "_dev" * dev, *args, *tail, ops._stream())

    def step(self):
        self.check_can_step("FlatAdam.step")
        self.sync_ema_cell()                 # (in front of `t += 1`: it sees a `t` that was set from outside; a no-op with averaging off)
        self.t += 1
        self._cell_stale = True              # a captured step that follows re-syncs the device step state (sync_cells)
        if self.ema_decay is not None:
            self._ema_t = self.t
        self._enqueue_update(dev=False)

    def step_captured(self, advance=True):
        """The update as launches a hipGraph can hold (rd_adam_step_dev: step count, beta^t, lr and weight decay live on the device).
        advance=True: a one-thread launch first moves the device state to this step (rd_adam_state_advance); advance=False: the
        caller's step already did (raindrop_amd.step.TrainStep.capture_full registers the cell -- `register_cell` -- and its first
        launch advances it: no extra launch).  Every replay is one step -- the owner of the graph keeps `self.t` in step
        (`note_replay`) and pushes what changed on the host with `sync_cells` (no new capture).  With averaging on, the step number
        that selects the count's slot is the device state's t."""
        self.check_can_step("FlatAdam.step_captured")
        self.sync_step_cell(create_only=True)
        if advance:
            self._check_step_cell("FlatAdam.step_captured")
            _lib.call("rd_adam_state_advance", ops._ptr(self.step_cell), float(self.betas[0]), float(self.betas[1]), ops._stream())
        self._enqueue_update(dev=True)

    def sync_cells(self, full=False):
        """Bring the device cells up to the host's settings in front of a captured step, stream-ordered with the replays around it
        and never a new capture: lr / weight decay (ReduceLROnPlateau, warm-up or cosine schedules), the clipping threshold, the
        averaging decay -- small copies, and only of what changed -- and the whole step state {t, beta^t, lr, wd} when host-side
        steps or load_state_dict left it stale, or always with `full` (in front of a capture)."""
        if full or self._cell_stale:
            self.sync_step_cell()            # (lr and weight decay are part of it)
            self._cell_stale = False
        else:
            self.sync_cell_hyper()
        self.sync_clip_cell()
        self.sync_ema_cell()
        self.sync_group_cell()

    def register_cell(self, on=True):
        """(Un)register the device step state with this host thread's next rd_step_begin launches (include/raindrop_hip.h
        rd_set_adam_state): the step's first launch then advances it."""
        self.sync_step_cell(create_only=True)
        if on:
            self._check_step_cell("FlatAdam.register_cell")
        _lib.call("rd_set_adam_state", ops._ptr(self.step_cell) if on else None, float(self.betas[0]), float(self.betas[1]))

    def sync_step_cell(self, create_only=False):
        """Make the device step state agree with `self.t`, `self.lr`, `self.weight_decay` (before capturing, after load_state_dict,
        after eager steps).  Layout (include/raindrop_hip.h rd_adam_step_dev): {t, beta1^t, beta2^t, lr, 0, wd, 0, 0} with t = steps TAKEN (the step's
        advance launch moves it to the step being applied).  With a schedule: {t, beta1^t, beta2^t, lr of step t, base lr, wd, n, 0}
        and the table behind it, 8 + capacity doubles in all (the entries behind n are 0 and never read)."""
        fresh = getattr(self, "step_cell", None) is None
        if fresh:
            self.step_cell = torch.zeros((8 + (self.schedule_capacity or 0),), dtype=torch.float64, device=self.param.device)
        if fresh or not create_only:
            # beta^t of the betas AS THE KERNELS SEE THEM (float arguments widened to double: rd_adam_step's pow() and the device's
            # running product both start from those) -- 0.999 as a double instead of 0.999f moves 1 - beta2^t by 1e-5 relative
            t = float(self.t)
            b1, b2 = (ctypes.c_float(float(b)).value for b in self.betas)
            if self.schedule is None:
                words = [t, b1 ** t, b2 ** t, float(self.lr), 0.0, float(self.weight_decay), 0.0, 0.0]
            else:
                words = [t, b1 ** t, b2 ** t, self._step_lr(), float(self.lr), float(self.weight_decay)] + self._schedule_words()
                words += [0.0] * (8 + self.schedule_capacity - len(words))
            self.step_cell.copy_(torch.tensor(words, dtype=torch.float64))
            self._cell_hyper = self.cell_hyper()

    def sync_cell_hyper(self):
        """lr / weight decay changed on the host (ReduceLROnPlateau, a warm-up or cosine schedule): two 8-byte cells, stream-ordered
        with the replays around it.  With a schedule `lr` is the BASE rate: slot 4, which the next advance multiplies into slot 3."""
        if self.step_cell is not None and getattr(self, "_cell_hyper", None) != self.cell_hyper():
            vals = torch.tensor([float(self.lr), float(self.weight_decay)], dtype=torch.float64, device=self.step_cell.device)
            if self.schedule is None:
                self.step_cell[3:6:2] = vals
            else:
                self.step_cell[4:6] = vals
            self._cell_hyper = self.cell_hyper()

    def device_steps(self):
        """steps taken according to the device state"""
        return int(float(self.step_cell[0]))

    def note_replay(self):
        self.t += 1
        if self.ema_decay is not None and self._ema_t == self.t - 1:         # the replay moved the count to the next slot
            self._ema_t = self.t

    def zero_grad(self, set_to_none=False):
        self.param.grad.zero_()

    def state_dict(self):
        stats = self.grad_stats() if self.clip_cell is not None else dict(skipped=0, clipped=0)
        sd = dict(t=self.t, exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq, lr=self.lr, betas=self.betas,
                  eps=self.eps, weight_decay=self.weight_decay, max_grad_norm=self.max_grad_norm,
                  grad_skipped=stats["skipped"], grad_clipped=stats["clipped"])
        if self.ema_decay is not None:       # (off: the keys of an optimizer without the keyword)
            if self.ema_swapped:
                raise _lib.RaindropHipError("FlatAdam.state_dict: the parameters are exchanged with their average: swap back first")
            sd.update(ema=self.ema, ema_decay=self.ema_decay, ema_warmup=self.ema_warmup, ema_updates=self.ema_updates())
        if self.group_cell is not None:      # (off: the keys of an optimizer without the keywords)
            names = self.groups.names if self.groups is not None else [None]
            sd.update(decoupled=self.decoupled,
                      groups=[dict(names=None if names[i] is None else list(names[i]), lr_scale=self._group_lr_scale[i], weight_decay=wd)
                              for i, wd in enumerate(self._group_wd)])
        if self.schedule is not None:        # (off: the keys of an optimizer without the keywords)
            sd.update(schedule=list(self.schedule.factors), schedule_capacity=self.schedule_capacity)
        return sd

    def load_state_dict(self, sd):
        """In place (the moment buffers and `ema` keep their addresses: a captured step stays valid); the device step state follows
        at the next captured step.  A dictionary without the `ema` keys leaves the average and its settings as they are; so does
        one without `groups` / `decoupled`.  One whose groups partition the parameters differently than this optimizer's (which
        includes one with groups into an optimizer without) raises before anything is changed: the chunk map is part of a capture.
        A dictionary with a `schedule` into an optimizer without one, one without into an optimizer with one, and a schedule longer
        than this optimizer's capacity raise before anything is changed as well: the step cell's size is part of a capture.  The
        schedule is restored in place; `t` travels, so the run goes on at the entry it had reached."""
        if self.ema_swapped:
            raise _lib.RaindropHipError("FlatAdam.load_state_dict: the parameters are exchanged with their average: swap back first")
        if ("schedule" in sd) != (self.schedule is not None):
            raise ValueError("FlatAdam.load_state_dict: the dictionary %s a learning-rate schedule, this optimizer %s: construct "
                             "FlatAdam with%s schedule / schedule_capacity"
                             % (("holds", "was built without one", "") if "schedule" in sd else ("holds no", "has one", "out")))
        if "schedule" in sd:
            schedule = LRSchedule(sd["schedule"])
            if len(schedule) > self.schedule_capacity:
                raise ValueError("FlatAdam.load_state_dict: a schedule of %d entries, the capacity is %d and fixed"
                                 % (len(schedule), self.schedule_capacity))
        if "groups" in sd:
            mine = None if self.group_cell is None else (self.groups.partition() if self.groups is not None else (None,))
            theirs = tuple(None if g["names"] is None else tuple(g["names"]) for g in sd["groups"])
            if mine != theirs:
                raise ValueError("FlatAdam.load_state_dict: the dictionary's parameter groups are another partition than this "
                                 "optimizer's: construct FlatAdam with the same groups")
            values = [(_check_group_value("lr_scale", g["lr_scale"]),
                       None if g["weight_decay"] is None else _check_group_value("weight_decay", g["weight_decay"])) for g in sd["groups"]]
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.t = int(sd["t"])
        self.lr, self.betas, self.eps, self.weight_decay = sd["lr"], tuple(sd["betas"]), sd["eps"], sd["weight_decay"]
        if "schedule" in sd:                 # (the table reaches the device with the rest of the step state: sync_cells)
            self.schedule = schedule
        self._cell_stale = True
        if "max_grad_norm" in sd:            # (a dictionary from before the keyword leaves the setting and the counts as they are)
            mgn = sd["max_grad_norm"]
            self.max_grad_norm = None if mgn is None else _check_max_grad_norm(mgn)
            if self.max_grad_norm is not None:
                if self.clip_cell is None:
                    self._make_clip_buffers()
                self.sync_clip_cell()
                self.clip_cell[3:5] = torch.tensor([float(sd.get("grad_skipped", 0)), float(sd.get("grad_clipped", 0))],
                                                   dtype=torch.float64, device=self.clip_cell.device)
        if sd.get("ema_decay") is not None:
            self.ema_decay, self.ema_warmup = _check_ema_decay(sd["ema_decay"]), bool(sd.get("ema_warmup", False))
            k = float(sd.get("ema_updates", 0))
            if self.ema is None:             # off -> on: new buffers, and hyper() makes a captured step capture again
                self._make_ema_buffers(int(k))
            else:                            # in place: both count slots, so that any step number finds it
                self.ema_cell.copy_(torch.tensor([self.ema_decay, float(self.ema_warmup), k, k] + [0.0] * 4, dtype=torch.float64))
                self._cell_ema_decay, self._ema_t = self.ema_decay, self.t
            self.ema.copy_(sd["ema"])
        if "groups" in sd:                   # in place: the cell keeps its address
            self._group_lr_scale, self._group_wd = [v[0] for v in values], [v[1] for v in values]
            self.decoupled = bool(sd.get("decoupled", self.decoupled))
            self.group_cell.copy_(torch.tensor(self._group_rows(), dtype=torch.float64))
            self._cell_group_wd = self.weight_decay
