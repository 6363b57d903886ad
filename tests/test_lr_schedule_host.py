"""CPU: the host side of the per-step learning-rate schedule (`optim.LRSchedule`, `FlatAdam(schedule=, schedule_capacity=)`,
`fit(lr_schedule=, warmup_steps=)`) -- every builder against torch's LambdaLR double for double, `from_torch` tables against the
schedulers they record, the words of the step cell, what the host forms enqueue on a stub library, the refusals, and the state
dictionary.  No device is touched: the optimizers here live on CPU tensors and never launch."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from raindrop_amd import optim
from raindrop_amd.optim import FlatAdam, LRSchedule

N = 200
BASES = (1e-3, 3.7e-4, 0.1, 1.0 / 3.0)


def _param(n=N):
    p = torch.nn.Parameter(torch.arange(n, dtype=torch.float32))
    p.grad = torch.zeros(n)
    return p


def _torch_rates(make, total, lr=1.0):
    """the rate each of `total` optimizer steps uses under the scheduler `make(optimizer)` builds: torch's own doubles"""
    o = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched = make(o)
    out = []
    for k in range(total):
        out.append(o.param_groups[0]["lr"])
        if k + 1 < total:
            o.step()
            sched.step()
    return out


def _lambda_rates(fn, total, lr=1.0):
    return _torch_rates(lambda o: torch.optim.lr_scheduler.LambdaLR(o, fn), total, lr)


def _cos(a, b, x):
    return b + (a - b) / 2.0 * (math.cos(math.pi * x) + 1.0)


def _one_cycle(total, pct, div, fdiv):
    u, end = float(pct * total) - 1.0, float(total - 1)
    return lambda k: _cos(1.0 / div, 1.0, k / u) if k <= u else _cos(1.0, 1.0 / div / fdiv, (k - u) / (end - u))


# (builder call, the function one would hand to LambdaLR, entries)
BUILDERS = {
    "linear_warmup": (lambda: LRSchedule.linear_warmup(7), lambda k: 1.0 if k + 1 >= 7 else 0.0 + (1.0 - 0.0) * (k + 1) / 7, 7),
    "linear_warmup_start": (lambda: LRSchedule.linear_warmup(5, start=0.1), lambda k: 1.0 if k + 1 >= 5 else 0.1 + (1.0 - 0.1) * (k + 1) / 5, 5),
    "warmup_cosine": (lambda: LRSchedule.warmup_cosine(23, warmup=4, min_factor=0.05),
                      lambda k: (k + 1) / 4 if k < 4 else 0.05 + (1.0 - 0.05) * 0.5 * (1.0 + math.cos(math.pi * ((k - 4) / 18))), 23),
    "cosine": (lambda: LRSchedule.warmup_cosine(12), lambda k: 0.0 + (1.0 - 0.0) * 0.5 * (1.0 + math.cos(math.pi * (k / 11))), 12),
    "step_decay": (lambda: LRSchedule.step_decay(3, 0.5, 11), lambda k: 0.5 ** (k // 3), 11),
    "one_cycle": (lambda: LRSchedule.one_cycle(20), _one_cycle(20, 0.3, 25.0, 1e4), 20),
    "one_cycle_args": (lambda: LRSchedule.one_cycle(17, pct_start=0.25, div=10.0, final_div=100.0), _one_cycle(17, 0.25, 10.0, 100.0), 17),
    "from_lambda": (lambda: LRSchedule.from_lambda(lambda k: 1.0 / math.sqrt(k + 1.0), 9), lambda k: 1.0 / math.sqrt(k + 1.0), 9),
}


@pytest.mark.parametrize("name", list(BUILDERS))
def test_builders_are_lambda_lr_double_for_double(name):
    build, fn, total = BUILDERS[name]
    s = build()
    assert isinstance(s, LRSchedule) and len(s) == total
    assert list(s.factors) == _lambda_rates(fn, total)               # lr = 1.0: the rate IS the factor
    for base in BASES:                                               # the same product, so the same bits at any base rate
        assert [base * f for f in s.factors] == _lambda_rates(fn, total, lr=base), base


def test_builder_shapes():
    w = LRSchedule.linear_warmup(4)
    assert w.factors == (0.25, 0.5, 0.75, 1.0) and w.factor(1) == 0.25 and w.factor(4) == w.factor(99) == 1.0 and w.factor(0) == 0.25
    c = LRSchedule.warmup_cosine(10, warmup=3, min_factor=0.1)
    assert c.factors[:4] == (1 / 3, 2 / 3, 1.0, 1.0) and abs(c.factors[-1] - 0.1) < 1e-15       # ends on min_factor, which then holds
    assert all(a >= b for a, b in zip(c.factors[3:], c.factors[4:]))
    o = LRSchedule.one_cycle(20)
    assert abs(o.factors[0] - 0.04) < 1e-15 and o.factors[5] == 1.0 == max(o.factors) and abs(o.factors[-1] - 4e-6) < 1e-18
    assert LRSchedule.step_decay(2, 0.1, 5).factors == (1.0, 1.0, 0.1, 0.1, 0.1 ** 2)
    assert LRSchedule([1, 0.5]).tensor().dtype == torch.float64 and LRSchedule(torch.tensor([1.0, 0.5])).factors == (1.0, 0.5)
    assert LRSchedule(np.array([1.0, 0.5]).tolist()) == LRSchedule((1.0, 0.5)) != LRSchedule((1.0,))
    with pytest.raises(AttributeError):
        w.factors = (1.0,)
    with pytest.raises(AttributeError):
        w._f = (1.0,)


TORCH_TABLES = {
    "cosine_annealing": (lambda lr: lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=15, eta_min=0.0), 16),
    "one_cycle": (lambda lr: lambda o: torch.optim.lr_scheduler.OneCycleLR(o, max_lr=lr, total_steps=18), 18),
    "sequential": (lambda lr: lambda o: torch.optim.lr_scheduler.SequentialLR(
        o, [torch.optim.lr_scheduler.LinearLR(o, start_factor=0.1, total_iters=4), torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=12)],
        milestones=[4]), 17),
}


@pytest.mark.parametrize("name", list(TORCH_TABLES))
def test_from_torch_tables_are_the_schedulers_rates(name):
    make, total = TORCH_TABLES[name]
    s = LRSchedule.from_torch(make(1.0), total)
    want = _torch_rates(make(1.0), total)
    assert len(s) == total and list(s.factors) == want and len(set(want)) > total // 2
    # another base rate: torch forms these recursively, so its double can sit one rounding away from base * f[k] -- as the float32
    # the update kernels use, at most one unit in the last place apart
    for base in BASES:
        theirs = np.array(_torch_rates(make(base), total, lr=base), dtype=np.float64).astype(np.float32)
        ours = np.array([base * f for f in s.factors], dtype=np.float64).astype(np.float32)
        ulp = np.abs(theirs.view(np.int32).astype(np.int64) - ours.view(np.int32).astype(np.int64))
        print(name, base, "max float32 ulp distance", int(ulp.max()), "entries apart", int((ulp != 0).sum()))
        assert int(ulp.max()) <= 1


def test_schedule_refusals():
    for bad in ([], (), [-1.0], [1.0, math.nan], [math.inf], [1.0, -math.inf], ["1"], [True], [None], 1.0, None, torch.zeros(0)):
        with pytest.raises(ValueError, match="LRSchedule"):
            LRSchedule(bad)
    for f in (lambda: LRSchedule.linear_warmup(0), lambda: LRSchedule.linear_warmup(2.0), lambda: LRSchedule.linear_warmup(3, start=-0.1),
              lambda: LRSchedule.warmup_cosine(0), lambda: LRSchedule.warmup_cosine(5, warmup=5), lambda: LRSchedule.warmup_cosine(5, warmup=-1),
              lambda: LRSchedule.warmup_cosine(5, min_factor=math.nan), lambda: LRSchedule.step_decay(0, 0.5, 4),
              lambda: LRSchedule.step_decay(2, -0.5, 4), lambda: LRSchedule.step_decay(2, 0.5, 0), lambda: LRSchedule.one_cycle(1),
              lambda: LRSchedule.one_cycle(10, pct_start=1.0), lambda: LRSchedule.one_cycle(10, div=0.5), lambda: LRSchedule.one_cycle(10, final_div=math.inf),
              lambda: LRSchedule.from_lambda(3, 4), lambda: LRSchedule.from_lambda(lambda k: -1.0, 4), lambda: LRSchedule.from_lambda(lambda k: 1.0, 0),
              lambda: LRSchedule.from_torch(None, 4), lambda: LRSchedule.from_torch(lambda o: torch.optim.lr_scheduler.StepLR(o, 1), True)):
        with pytest.raises(ValueError):
            f()
    with pytest.raises(ValueError, match="LRSchedule"):
        FlatAdam(_param(), schedule=[1.0, 0.5])
    for cap in (2, 0, -1, 3.0, True, "4"):
        with pytest.raises(ValueError, match="schedule_capacity"):
            FlatAdam(_param(), schedule=LRSchedule([1.0, 0.5, 0.25]), schedule_capacity=cap)


# ---- the optimizer: cell, calls, set_schedule ---------------------------------------------------------------------------------------------
S12 = LRSchedule.warmup_cosine(12, warmup=3, min_factor=0.1)
B1, B2 = (ctypes.c_float(b).value for b in (0.9, 0.999))


def test_off_is_the_optimizer_without_the_keywords():
    off = FlatAdam(_param(), lr=2.5e-4, weight_decay=0.01)
    assert off.schedule is None and off.schedule_capacity is None
    off.sync_cells(full=True)
    assert tuple(off.step_cell.shape) == (8,) and off.step_cell.tolist() == [0.0, 1.0, 1.0, 2.5e-4, 0.0, 0.01, 0.0, 0.0]
    off.lr = 1e-4
    off.sync_cells()
    assert off.step_cell.tolist() == [0.0, 1.0, 1.0, 1e-4, 0.0, 0.01, 0.0, 0.0]                 # slot 3, as ever; slot 6 stays 0.0
    assert off.hyper() == (0.9, 0.999, 1e-8) and off.current_lr() == 1e-4
    assert sorted(off.state_dict()) == sorted(["t", "exp_avg", "exp_avg_sq", "lr", "betas", "eps", "weight_decay", "max_grad_norm",
                                               "grad_skipped", "grad_clipped"])
    for f in (lambda: off.set_schedule(S12), off.clear_schedule, off.schedule_position):
        with pytest.raises(ValueError, match="off"):
            f()


def test_cell_words_with_a_schedule():
    a = FlatAdam(_param(), lr=2.5e-4, weight_decay=0.01, schedule=S12, schedule_capacity=16)
    assert a.hyper() == (0.9, 0.999, 1e-8)                           # no launch constant: on or off is the same capture
    a.sync_cells(full=True)
    assert tuple(a.step_cell.shape) == (24,) and a.step_cell.dtype == torch.float64 and a.step_cell.data_ptr() % 16 == 0
    assert a.step_cell.tolist() == [0.0, 1.0, 1.0, 2.5e-4 * S12[0], 2.5e-4, 0.01, 12.0, 0.0] + list(S12.factors) + [0.0] * 4
    cell = a.step_cell.data_ptr()
    a.lr, a.weight_decay = 1e-4, 0.02                                # the base rate goes to slot 4; slot 3 is the device's
    a.sync_cells()
    assert a.step_cell.tolist()[:8] == [0.0, 1.0, 1.0, 2.5e-4 * S12[0], 1e-4, 0.02, 12.0, 0.0]
    a.t = 5                                                          # (a jump of t, as load_state_dict makes it)
    a.sync_step_cell()
    assert a.step_cell.tolist()[:8] == [5.0, B1 ** 5.0, B2 ** 5.0, 1e-4 * S12[4], 1e-4, 0.02, 12.0, 0.0]
    assert a.schedule_position() == 5 and a.current_lr() == 1e-4 * S12[4]
    a.t = 40
    assert a.schedule_position() == 12
    s7 = LRSchedule.linear_warmup(7)
    a.set_schedule(s7)                                               # slots 6, 7 and the table; what lies behind n is never read
    assert a.step_cell.tolist()[4:15] == [1e-4, 0.02, 7.0, 0.0] + list(s7.factors) and a.schedule_position() == 7
    a.clear_schedule()
    assert a.step_cell.tolist()[6:9] == [1.0, 0.0, 1.0] and a.schedule == LRSchedule([1.0])
    a.set_schedule(LRSchedule([0.5] * 16))                           # exactly the capacity
    assert a.step_cell.tolist()[6:] == [16.0, 0.0] + [0.5] * 16
    with pytest.raises(ValueError, match="capacity is 16"):
        a.set_schedule(LRSchedule([0.5] * 17))
    with pytest.raises(ValueError, match="LRSchedule"):
        a.set_schedule([0.5])
    assert a.step_cell.data_ptr() == cell and len(a.schedule) == 16  # a refused table changes nothing; none of it moved the cell
    b = FlatAdam(_param(), schedule_capacity=4)                      # capacity alone: the table {1.0} in that much room
    b.sync_cells(full=True)
    assert b.schedule == LRSchedule([1.0]) and b.step_cell.tolist() == [0.0, 1.0, 1.0, 1e-3, 1e-3, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    assert FlatAdam(_param(), schedule=S12).schedule_capacity == 12


@pytest.fixture
def calls(monkeypatch):
    log = []
    monkeypatch.setattr(optim._lib, "call", lambda name, *args: log.append((name, args)))
    monkeypatch.setattr(optim.ops, "_stream", lambda: "stream")
    return log


def test_host_step_passes_the_double_product_and_the_captured_form_adds_no_call(calls):
    a = FlatAdam(_param(), lr=2.5e-4, weight_decay=0.01, schedule=S12, schedule_capacity=16)
    for t in range(1, 16):
        a.step()
        name, args = calls[-1]
        assert name == "rd_adam_step" and args[5] == float((2.5e-4 if t <= 6 else 1e-4) * S12[min(t - 1, 11)]) and args[10] == t
        if t == 6:
            a.lr = 1e-4                                              # the base rate, as ReduceOnPlateau assigns it
            assert a.schedule_position() == 6
    assert calls[-1][1][5] == 1e-4 * S12[11] and len(calls) == 15
    del calls[:]
    a.step_captured()
    assert [c[0] for c in calls] == ["rd_adam_state_advance", "rd_adam_step_dev"]                # the calls of an optimizer without one
    assert calls[0][1][0].value == calls[1][1][-2].value == a.step_cell.data_ptr() and len(calls[0][1]) == 4 and len(calls[1][1]) == 10
    assert a.step_cell.tolist()[:8] == [15.0, B1 ** 15.0, B2 ** 15.0, 1e-4 * S12[11], 1e-4, 0.01, 12.0, 0.0]
    # the advancing thread trusts slot 6: a table assigned around set_schedule, or another cell, is refused in front of the launch
    del calls[:]
    a.schedule = LRSchedule([1.0] * 17)
    for f in (a.step_captured, a.register_cell):
        with pytest.raises(optim._lib.RaindropHipError, match="at most 16"):
            f()
    a.schedule = S12
    a.step_cell = torch.zeros(8, dtype=torch.float64)
    with pytest.raises(optim._lib.RaindropHipError, match="24 doubles"):
        a.step_captured()
    assert calls == []


def test_state_dict_round_trip_and_refusals():
    a = FlatAdam(_param(), lr=2.5e-4, schedule=S12, schedule_capacity=16)
    a.t = 5
    sd = a.state_dict()
    assert sd["schedule"] == list(S12.factors) and sd["schedule_capacity"] == 16 and sd["t"] == 5
    off = FlatAdam(_param(), lr=2.5e-4)
    assert sorted(sd) == sorted(list(off.state_dict()) + ["schedule", "schedule_capacity"])
    b = FlatAdam(_param(), lr=1.0, schedule=LRSchedule.linear_warmup(14), schedule_capacity=14)   # room for 12, not the same capacity
    b.sync_cells(full=True)
    cell = b.step_cell.data_ptr()
    b.load_state_dict(sd)
    assert b.schedule == S12 and b.schedule_capacity == 14 and b.t == 5 and b.schedule_position() == 5
    b.sync_cells()                                                   # in place: the cell keeps its address and gets the table
    assert b.step_cell.data_ptr() == cell
    assert b.step_cell.tolist() == [5.0, B1 ** 5.0, B2 ** 5.0, 2.5e-4 * S12[4], 2.5e-4, 0.0, 12.0, 0.0] + list(S12.factors) + [0.0] * 2
    small = FlatAdam(_param(), schedule=LRSchedule.linear_warmup(4))
    plain = {k: v for k, v in sd.items() if k not in ("schedule", "schedule_capacity")}
    for target, d, word in ((off, sd, "built without"), (small, sd, "capacity is 4"), (a, plain, "holds no"),
                            (small, dict(sd, schedule=[1.0, -1.0]), "LRSchedule")):
        keep = (target.t, target.schedule, target.lr)
        with pytest.raises(ValueError, match=word):
            target.load_state_dict(dict(d, t=9, lr=7.0))
        assert (target.t, target.schedule, target.lr) == keep        # refused before anything was changed
    off.load_state_dict(dict(plain, t=3))                            # without the keys into one without the feature: as ever
    assert off.t == 3 and off.schedule is None


# ---- fit ------------------------------------------------------------------------------------------------------------------------------
def test_fit_refuses_bad_schedule_arguments_without_a_device():
    from raindrop_amd.trainer import _resolve_schedule, fit
    ds = types.SimpleNamespace(dev=torch.device("cpu"), y=torch.zeros(8, dtype=torch.int64), N=8, T=5, W=6, ds=0, Pstatic=None)
    for bad in ("cosine", 3, [1.0, 0.5], 0.5):
        with pytest.raises(ValueError, match="lr_schedule"):
            fit(None, ds, ds, 1, batch_size=8, lr_schedule=bad)
    for bad in (-1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="warmup_steps"):
            fit(None, ds, ds, 1, batch_size=8, lr_schedule="warmup_cosine", warmup_steps=bad)
    for sched in (None, S12, lambda total: S12):                     # a warm-up length belongs to the named schedule alone
        with pytest.raises(ValueError, match="warmup_steps"):
            fit(None, ds, ds, 1, batch_size=8, lr_schedule=sched, warmup_steps=2)
    with pytest.raises(ValueError, match="strategy"):                # the earlier refusals are still there behind good arguments
        fit(None, ds, ds, 1, batch_size=8, strategy=0, lr_schedule="warmup_cosine", warmup_steps=2)
    assert _resolve_schedule(None, 0, 20) is None and _resolve_schedule("warmup_cosine", 0, 0) is None
    assert _resolve_schedule(S12, 0, 20) is S12
    assert _resolve_schedule("warmup_cosine", 3, 20) == LRSchedule.warmup_cosine(20, warmup=3)
    assert _resolve_schedule(lambda total: LRSchedule.one_cycle(total), 0, 20) == LRSchedule.one_cycle(20)
    with pytest.raises(ValueError, match="less than"):
        _resolve_schedule("warmup_cosine", 20, 20)
    with pytest.raises(ValueError, match="must return"):
        _resolve_schedule(lambda total: [1.0] * total, 0, 20)
