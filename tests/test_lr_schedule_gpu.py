"""GPU: the per-step learning-rate schedule on the device (`optim.LRSchedule`, `FlatAdam(schedule=, schedule_capacity=)`: the table
behind the step state, read by the one thread that advances it -- rd_adam_state_advance, or rd_step_begin inside a whole-step
hipGraph).  The reference is the path without the feature: an optimizer built without a schedule whose `lr` the host sets to
base * f[min(t - 1, n - 1)] in front of every step; parameters, both moments and the average must have its bits after every step,
in every form of the update.  Then torch.optim.Adam / AdamW under LambdaLR, the non-finite guard, tables and base rates changed
between replays of one graph, a resumed run, the whole step (TrainStep and BetaTrainStep) and `fit`."""
import functools
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 4 * 256 * 3 + 3                                                # three workgroups of float4 threads and a three-element scalar tail
STEPS, ENTRIES, CAPACITY = 20, 12, 16                              # eight steps past the end of the table: the last factor holds
LR, WD = 1e-3, 0.01
MAX_NORM = 60.0                                                    # the gradient norms run from 28 to 133: the later steps are clipped
# three tensors on 64-element chunk boundaries with padding behind the first two; rules for the second and the third
TENSORS = [("t1", 0, 1000), ("t2", 1024, 2000), ("t3", 2048, N)]
RULES = [dict(match=["t2"], lr_scale=0.5, weight_decay=0.0), dict(match=["t3"], lr_scale=0.25)]
FORMS = [(d, c, e, g) for d in (False, True) for c in (False, True) for e in (False, True) for g in (False, True)]
FORM_IDS = [("dev" if d else "host") + "_clip" * c + "_ema" * e + "_grp" * g for d, c, e, g in FORMS]


def _schedule():
    from raindrop_amd.optim import LRSchedule
    return LRSchedule.warmup_cosine(ENTRIES, warmup=3, min_factor=0.1)


@functools.lru_cache(maxsize=None)
def _data():
    """(initial parameters, the twenty gradients), on the host; gradient s scaled by 0.5 + 0.1 s"""
    g_ = torch.Generator(device="cpu").manual_seed(17)
    p0 = torch.randn(N, generator=g_)
    return p0, [torch.randn(N, generator=g_) * (0.5 + 0.1 * s) for s in range(STEPS)]


def _opt(clip=False, ema=False, grp=False, **kw):
    from raindrop_amd.optim import FlatAdam, ParamGroups
    p = torch.nn.Parameter(_data()[0].clone().to(DEV))
    p.grad = torch.zeros(N, device=DEV)
    if clip:
        kw.setdefault("max_grad_norm", MAX_NORM)
    if ema:
        kw.update(ema_decay=0.9)
    if grp:
        kw.update(groups=ParamGroups(types.SimpleNamespace(names=[t[0] for t in TENSORS], slices=[(lo, hi) for _, lo, hi in TENSORS]), RULES))
    kw.setdefault("lr", LR)
    return p, FlatAdam(p, weight_decay=WD, **kw)


def _pair(clip=False, ema=False, grp=False, schedule=None, **kw):
    """(optimizer with the schedule, the same optimizer without one: the reference the host feeds its rates)"""
    schedule = schedule or _schedule()
    return _opt(clip, ema, grp, schedule=schedule, schedule_capacity=CAPACITY, **kw)[1], _opt(clip, ema, grp, **kw)[1]


def _step(opt, dev, g):
    opt.param.grad.copy_(g)
    if dev:
        opt.sync_cells()                                            # what TrainStep.run_full does in front of a replay
        opt.step_captured(); opt.note_replay()
    else:
        opt.step()


def _fed(ref, dev, g, rate):
    """one step of the reference at `rate`, assigned from the host the way a caller without the feature must"""
    ref.lr = rate
    _step(ref, dev, g)


def _state(opt):
    ts = [opt.param, opt.exp_avg, opt.exp_avg_sq] + ([] if opt.ema is None else [opt.ema])
    return [t.detach().clone().view(torch.int32) for t in ts]


def _assert_same(a, b, where):
    sa, sb = _state(a), _state(b)
    assert len(sa) == len(sb)
    for name, x, y in zip(("p", "m", "v", "ema"), sa, sb):
        assert torch.equal(x, y), (where, name, int((x != y).sum()), (x != y).nonzero()[:4].flatten().tolist())


# ---- 1. every form against the hand-fed optimizer ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_scheduled_steps_have_the_bits_of_hand_fed_rates(form):
    dev, clip, ema, grp = form
    sched, (_, grads) = _schedule(), _data()
    a, ref = _pair(clip, ema, grp)
    assert a.hyper() == ref.hyper() and a.lr == LR
    for s in range(STEPS):
        rate = LR * sched[min(s, ENTRIES - 1)]                       # the float64 product
        g = grads[s].to(DEV)
        _step(a, dev, g)
        _fed(ref, dev, g, rate)
        _assert_same(a, ref, s)
        assert a.current_lr() == rate and a.schedule_position() == min(s + 1, ENTRIES), (s, a.current_lr(), rate)
    assert a.lr == LR and a.t == ref.t == STEPS and (not dev or a.device_steps() == STEPS)
    assert tuple(a.step_cell.shape) == (8 + CAPACITY,) if dev else a.step_cell is None
    if clip:
        st = a.grad_stats()
        assert st == ref.grad_stats() and 0 < st["clipped"] < STEPS and st["skipped"] == 0


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_decoupled_decay_shrinks_by_the_scheduled_rate(dev):
    sched, (_, grads) = _schedule(), _data()
    a, ref = _pair(decoupled=True)
    for s in range(STEPS):
        g = grads[s].to(DEV)
        _step(a, dev, g)
        _fed(ref, dev, g, LR * sched[min(s, ENTRIES - 1)])
        _assert_same(a, ref, s)


# ---- 2. against torch ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _torch_reference(decoupled):
    """the parameters after each of the twenty steps: torch.optim.Adam / AdamW under LambdaLR, float32 on the CPU"""
    p0, grads = _data()
    sched = _schedule()
    q = torch.nn.Parameter(p0.clone())
    o = (torch.optim.AdamW if decoupled else torch.optim.Adam)([q], lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=WD)
    lam = torch.optim.lr_scheduler.LambdaLR(o, lambda k: sched[min(k, ENTRIES - 1)])
    out = []
    for s in range(STEPS):
        q.grad = grads[s].clone()
        o.step()
        lam.step()
        out.append(q.detach().clone())
    return out


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
def test_schedule_against_torch_lambda_lr(decoupled, dev):
    """max |p - torch| < 2e-6 after each step: the bound tests/test_param_groups_gpu.py holds the grouped update to against torch at
    lr = 1e-3, the largest rate of this schedule (factors <= 1 on the base rate 1e-3)"""
    _, grads = _data()
    want = _torch_reference(decoupled)
    p, a = _opt(schedule=_schedule(), schedule_capacity=CAPACITY, decoupled=decoupled)
    worst = 0.0
    for s in range(STEPS):
        _step(a, dev, grads[s].to(DEV))
        worst = max(worst, float((p.detach().cpu() - want[s]).abs().max()))
    print("%s %s: max |p - torch| over %d steps %.3e" % ("dev" if dev else "host", "decoupled" if decoupled else "coupled", STEPS, worst))
    assert worst < 2e-6


# ---- 3. the guard ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_a_skipped_step_consumes_its_entry(dev):
    """guard on: an inf gradient at step 3 keeps every bit and still uses up f[2]; step 4 runs at f[3], like the hand-fed reference"""
    sched, (_, grads) = _schedule(), _data()
    a, ref = _pair(clip=True, ema=True, max_grad_norm=math.inf)
    for s in range(5):
        g = grads[s].clone()
        if s == 2:
            g[1500] = float("inf")
        before = _state(a)
        _step(a, dev, g.to(DEV))
        _fed(ref, dev, g.to(DEV), LR * sched[s])
        _assert_same(a, ref, s)
        assert a.current_lr() == LR * sched[s] and a.schedule_position() == s + 1
        assert all(torch.equal(x, y) for x, y in zip(before, _state(a))) == (s == 2)
    assert a.grad_stats()["skipped"] == ref.grad_stats()["skipped"] == 1 and a.t == 5 and a.ema_updates() == 4


# ---- 4. another table, no table, another base rate: one graph -------------------------------------------------------------------------
def test_set_schedule_clear_schedule_and_the_base_rate_reach_a_captured_graph():
    """step_captured() inside torch.cuda.graph, replayed twenty times: set_schedule (7 entries) in front of step 7, a lower base rate --
    what ReduceOnPlateau assigns -- in front of step 10, clear_schedule in front of step 14; none of them captures again, every step
    has the bits of the hand-fed optimizer"""
    from raindrop_amd.optim import LRSchedule
    sched, (_, grads) = _schedule(), _data()
    seven = LRSchedule.linear_warmup(7, start=0.2)
    a, ref = _pair(clip=True, ema=True, grp=True)
    a.sync_cells(full=True)
    a.param.grad.copy_(grads[0].to(DEV))
    state = [t.clone() for t in (a.param.data, a.exp_avg, a.exp_avg_sq, a.ema, a.ema_cell, a.clip_cell)]
    a.step_captured()                                               # outside the capture first: lazy loads; then put everything back
    torch.cuda.synchronize()
    for t, keep in zip((a.param.data, a.exp_avg, a.exp_avg_sq, a.ema, a.ema_cell, a.clip_cell), state):
        t.copy_(keep)
    a.sync_step_cell()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a.step_captured()
    a.sync_step_cell()
    cell, table, base = a.step_cell.data_ptr(), sched, LR
    for s in range(STEPS):
        if s == 6:
            a.set_schedule(seven); table = seven
        if s == 9:
            a.lr = base = LR * 0.1
        if s == 13:
            a.clear_schedule(); table = LRSchedule([1.0])
        rate = base * table[min(s, len(table) - 1)]
        g = grads[s].to(DEV)
        a.param.grad.copy_(g)
        a.sync_cells()
        graph.replay(); a.note_replay()
        _fed(ref, True, g, rate)
        _assert_same(a, ref, s)
        assert a.current_lr() == rate, (s, a.current_lr(), rate)
    assert a.step_cell.data_ptr() == cell and a.device_steps() == a.t == STEPS and a.grad_stats() == ref.grad_stats()
    assert a.lr == LR * 0.1 and a.schedule_position() == 1
    with pytest.raises(ValueError, match="capacity"):
        a.set_schedule(LRSchedule([1.0] * (CAPACITY + 1)))


# ---- 5. resume -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_a_resumed_run_goes_on_at_its_entry(dev):
    from raindrop_amd.optim import FlatAdam
    _, grads = _data()
    straight = _opt(ema=True, schedule=_schedule(), schedule_capacity=CAPACITY)[1]
    first = _opt(ema=True, schedule=_schedule(), schedule_capacity=CAPACITY)[1]
    for s in range(10):
        _step(straight, dev, grads[s].to(DEV))
    for s in range(5):
        _step(first, dev, grads[s].to(DEV))
    sd = first.state_dict()
    p = torch.nn.Parameter(first.param.detach().clone())
    p.grad = torch.zeros(N, device=DEV)
    second = FlatAdam(p, lr=0.5, ema_decay=0.5, schedule_capacity=CAPACITY)          # another rate, no table of its own
    second.load_state_dict(sd)
    assert second.schedule == _schedule() and second.schedule_position() == 5 and second.lr == LR
    for s in range(5, 10):
        _step(second, dev, grads[s].to(DEV))
        assert second.current_lr() == LR * _schedule()[s]
    _assert_same(second, straight, "resumed")


# ---- 6. off means off ------------------------------------------------------------------------------------------------------------------
def test_without_the_keywords_the_cell_is_eight_doubles():
    _, grads = _data()
    p, off = _opt()
    _step(off, True, grads[0].to(DEV))
    assert tuple(off.step_cell.shape) == (8,) and off.step_cell.tolist()[3:] == [LR, 0.0, WD, 0.0, 0.0] and off.schedule is None
    assert off.hyper() == (0.9, 0.999, 1e-8)
    assert sorted(off.state_dict()) == sorted(["t", "exp_avg", "exp_avg_sq", "lr", "betas", "eps", "weight_decay", "max_grad_norm",
                                               "grad_skipped", "grad_clipped"])


# ---- 7. the whole step as one hipGraph ------------------------------------------------------------------------------------------------
@pytest.fixture(params=["bf16x3", "fp32"])
def precision_mode(request):
    from raindrop_amd import _lib
    _lib.call("rd_set_precision", 1 if request.param == "bf16x3" else 0)
    yield request.param
    _lib.call("rd_set_precision", 1)


def _whole_step(beta, **opt_kw):
    """P19, B = 8, dropout 0, clipping, averaging and no_decay groups at weight decay 0.01 (tests/test_param_groups_gpu.py's model)"""
    from raindrop_amd import dp, optim, synth
    from raindrop_amd.step import TrainStep
    from raindrop_amd.step_beta import BetaTrainStep
    from tests.helpers import build_ours
    cfg = synth.make_config("P19")
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 21, **(dict(use_beta=True) if beta else {})).train()
    named = dict(m.named_parameters())
    names = synth.live_parameter_names_beta(cfg) if beta else synth.live_parameter_names(cfg)
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in names], n_buckets=2)
    groups = optim.ParamGroups(flat, [optim.no_decay(flat)])
    opt = optim.FlatAdam(flat.flatten_parameters(), lr=1e-3, weight_decay=0.01, groups=groups, max_grad_norm=1.0, ema_decay=0.99, **opt_kw)
    buf = {k: (None if v is None else v.to(DEV).clone()) for k, v in synth.make_batch(cfg, 8, seed=33).items()}
    ts = (BetaTrainStep if beta else TrainStep)(m, flat, buf, p_drop=0.0, autotune=False, split=False)
    return ts, opt


@pytest.mark.parametrize("beta", [False, True], ids=["default", "use_beta"])
def test_whole_step_graph_forms_its_own_rates(beta, precision_mode):
    """capture_full with a 10-entry warm-up and cosine table: sixteen replays are bit-equal to the same step with the rates assigned
    by hand in front of each run_full; the capture's warm-up passes leave the position at 0; set_schedule is not a new capture"""
    from raindrop_amd.optim import LRSchedule
    table = LRSchedule.warmup_cosine(10, warmup=3, min_factor=0.05)
    other = LRSchedule.step_decay(2, 0.5, 6)
    ts_a, a = _whole_step(beta, schedule=table)
    ts_b, ref = _whole_step(beta)
    try:
        graph = ts_a.capture_full(a)
        ts_b.capture_full(ref)
        begin = ts_a.plan is not None and bool(ts_a.prep_enc or ts_a.prep_k1) and ts_a.one_begin
        print("use_beta" if beta else "default", precision_mode, "advance inside rd_step_begin:", begin)
        if precision_mode == "bf16x3" and not beta:                  # the step's first launch advances the cell: no launch of its own
            assert begin
        assert a.schedule_position() == 0 and a.device_steps() == 0 and a.t == 0 and a.schedule_capacity == 10
        assert a.step_cell.tolist() == [0.0, 1.0, 1.0, 1e-3 * table[0], 1e-3, 0.01, 10.0, 0.0] + list(table.factors)
        assert ts_a.captures == ts_b.captures == 1
        for s in range(16):
            if s == 12:
                a.set_schedule(other); table = other
            ref.lr = 1e-3 * table[min(s, len(table) - 1)]
            la, lb = ts_a.run_full().clone(), ts_b.run_full().clone()
            assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and bool(torch.isfinite(la)), (s, float(la), float(lb))
            _assert_same(a, ref, s)
            assert a.current_lr() == ref.lr
        assert ts_a.captures == 1 and ts_a.graph_full is graph and a.device_steps() == a.t == 16 and a.lr == 1e-3
        assert a.grad_stats() == ref.grad_stats() and a.ema_updates() == ref.ema_updates() == 16
    finally:
        ts_a.close()
        ts_b.close()


# ---- 8. fit ----------------------------------------------------------------------------------------------------------------------------
def test_fit_with_warmup_cosine_is_the_hand_written_loop():
    """48 samples, batches of 8, two epochs: fit(lr_schedule="warmup_cosine", warmup_steps=3) against the loop of
    tests/test_epoch_feed_gpu.py::test_fit_runs_the_scripts_loop with the rates assigned by hand in front of every step"""
    from raindrop_amd import dp, feed, synth, trainer
    from raindrop_amd.optim import FlatAdam, LRSchedule
    from raindrop_amd.step import TrainStep
    from tests.helpers import build_ours
    cfg = synth.make_config("P19")

    def part(n, seed, rseed):
        data = synth.make_batch(cfg, n, seed=seed)
        y = ((data["src"][:, :, 0].sum(0).numpy() + 0.5 * np.random.default_rng(rseed).standard_normal(n)) > 0).astype(np.int64)
        if y.mean() > 0.5:
            y = 1 - y
        return feed.DeviceDataset(data["src"], data["times"], data["static"], torch.from_numpy(y), device=DEV), y

    def model():
        m = build_ours(cfg, synth.make_structure(cfg, "ones"), DEV, 3)
        m.dropout.p = 0.2
        return m
    (ds, ytrain), (vds, _) = part(48, 71, 5), part(24, 72, 6)
    B, E, base = 8, 2, 1e-3
    np.random.seed(0)
    m = model().train()
    named = dict(m.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)], n_buckets=2)
    opt = FlatAdam(flat.flatten_parameters(), lr=base)
    planner = feed.EpochPlanner(ytrain, batch_size=B, strategy=2, n_total=ds.N)
    nb = int(planner.n_batches)
    assert nb >= 2
    table = LRSchedule.warmup_cosine(E * nb, warmup=3)
    out = ds.alloc(B)
    ds.batch(np.arange(B), out=out)
    step = TrainStep(m, flat, dict(src=out["P"], times=out["Ptime"], static=out["Pstatic"], y=out["y"], lengths=out["lengths"]), autotune=False)
    want, k = [], 0
    try:
        step.capture_full(opt)
        for _ in range(E):
            losses = []
            for idx in planner.next_epoch():
                ds.batch(idx, out=out)
                opt.lr = base * table[k]
                k += 1
                losses.append(step.run_full().clone())
            want.append(torch.stack(losses).cpu().numpy().mean())
    finally:
        step.close()
    np.random.seed(0)
    r = trainer.fit(model().eval(), ds, vds, E, batch_size=B, strategy=2, lr=base, scheduler=False, autotune=False,
                    lr_schedule="warmup_cosine", warmup_steps=3)
    print("train_loss", r["train_loss"], "hand", [float(w) for w in want], "lr_step", r["lr_step"])
    assert [np.float32(x) for x in r["train_loss"]] == want and len(set(r["train_loss"])) == E
    assert r["lr_step"] == [base * table[nb - 1], base * table[2 * nb - 1]] and r["lr"] == [base] * E
    assert abs(r["lr_step"][1]) < 1e-18 < r["lr_step"][0]                              # the cosine ends on its minimum, 0
