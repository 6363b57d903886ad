"""GPU: gradient accumulation in the captured steps (`TrainStep(accumulate=k)`, rd_grad_accumulate / rd_grad_accumulate_close).

The operators against torch bit for bit; an accumulating step against its restatement -- a plain step over the same micro-batches at
equal seed-cell values, `((g1 + g2) + g3) * float32(1/3)` formed by torch -- bit for bit in every form; against ONE step on the
concatenated batch within the data-parallel test's bound (the same mathematical statement: a mean of shard means); the whole-step
graphs with the optimizer inside; a re-capture in the middle of a window; two ranks over gloo; the untouched default; `fit`."""
import ctypes
import importlib.util
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from raindrop_amd import _lib, dp, feed, ops, synth
from raindrop_amd.optim import FlatAdam, LRSchedule
from tests.helpers import build_ours

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                                                       # NaN-filled floats behind every operator buffer
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# tests/test_dp_gpu.py::test_two_rank_step_equals_full_batch_step: a mean of shard-mean gradients against the full batch's gradient,
# relative to the largest entry.  k micro-batches against one large batch is the same statement with shards taken in time.
DP_GRAD_BOUND = 3e-5
# The loss of that statement: every step's fp32 loss is within 1e-6 of the exact mean cross entropy in exact-fp32 arithmetic
# (tests/test_beta_step_gpu.py::test_beta_step_matches_eager_model's `ltol`, tests/test_gpu_parity.py's for the default branch), on
# both sides, and averaging four of them in fp32 adds < 1e-6 at losses of order 1.
DP_LOSS_BOUND = 3e-6


@pytest.fixture(params=["bf16x3", "fp32"])
def precision_mode(request):
    _lib.call("rd_set_precision", 1 if request.param == "bf16x3" else 0)
    yield request.param
    _lib.call("rd_set_precision", 1)


def _to_dev(batch):
    return {k: (None if v is None else v.to(DEV)) for k, v in batch.items()}


def _fill(buf, batch):
    for k, v in batch.items():
        if v is not None:
            buf[k].copy_(v)


def _bits(t):
    return t.view(torch.int32)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _make(cfg, B, beta=False, dropout=0.2, param_seed=21, opt_kw=None, **step_kw):
    """(step, flat, opt or None, batch buffers): a model in training mode from fixed seeds and a step over `B`-sample buffers"""
    from raindrop_amd.step import TrainStep
    from raindrop_amd.step_beta import BetaTrainStep
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, param_seed, **(dict(use_beta=True) if beta else {})).train()
    m.dropout.p = dropout
    named = dict(m.named_parameters())
    names = synth.live_parameter_names_beta(cfg) if beta else synth.live_parameter_names(cfg)
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in names], n_buckets=2)
    opt = None if opt_kw is None else FlatAdam(flat.flatten_parameters(), **opt_kw)
    buf = _to_dev(synth.make_batch(cfg, B, seed=40))
    step_kw.setdefault("autotune", False)
    step = (BetaTrainStep if beta else TrainStep)(m, flat, buf, **step_kw)
    return step, flat, opt, buf


# ---- 1. the operators ---------------------------------------------------------------------------------------------------------------
def _operands(n, seed):
    """g, acc [n] inside NaN-guarded allocations, random with denormals and signed zeros sprinkled in"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        whole = torch.full((n + GUARD,), float("nan"))
        v = torch.randn(n, generator=gen) * torch.exp(4 * torch.randn(n, generator=gen))
        if n:
            special = torch.tensor([1e-40, -3e-39, 0.0, -0.0, 1.4e-45, -1.17549435e-38])
            where = torch.randint(0, n, (min(n, 12),), generator=gen)
            v[where] = special[torch.arange(where.numel()) % special.numel()]
        whole[:n] = v
        out.append(whole.to(DEV))
    return out


def _guard_intact(whole, n):
    want = torch.full((GUARD,), float("nan")).view(torch.int32)
    return torch.equal(_bits(whole[n:]).cpu(), want)


N_OPERATOR = [0, 1, 3, 4, 5, 255, 1024, 1027, (1 << 20) + 3]


@pytest.mark.parametrize("n", N_OPERATOR)
def test_operators_equal_torch_bit_for_bit(n):
    for scale in (1.0 / 3.0, 0.25):
        gw, aw = _operands(n, 1000 + n)
        g, acc = gw[:n], aw[:n]
        assert n < 6 or bool(((g != 0) & (g.abs() < 1.1754944e-38)).any())     # the inputs do hold denormals
        cell = torch.tensor([scale], dtype=torch.float32, device=DEV)
        want_acc = acc + g
        _lib.call("rd_grad_accumulate", n, ops._ptr(gw), ops._ptr(aw), ops._stream())      # (the allocations start where g, acc do)
        torch.cuda.synchronize()
        assert torch.equal(_bits(acc), _bits(want_acc)), (n, "accumulate")
        assert _guard_intact(gw, n) and _guard_intact(aw, n), (n, "accumulate")
        g2 = _operands(n, 2000 + n)[0]                                          # the next micro-batch's gradient
        want_g = (acc + g2[:n]) * cell
        _lib.call("rd_grad_accumulate_close", n, ops._ptr(g2), ops._ptr(aw), ops._ptr(cell), ops._stream())
        torch.cuda.synchronize()
        assert torch.equal(_bits(g2[:n]), _bits(want_g)), (n, scale, "close")
        assert torch.equal(_bits(acc), torch.zeros(n, dtype=torch.int32, device=DEV)), (n, "acc is +0.0")
        assert _guard_intact(g2, n) and _guard_intact(aw, n), (n, "close")
        assert float(cell) == np.float32(scale)                                 # the cell is only read


@pytest.mark.parametrize("n", [5, 1027])
def test_close_propagates_inf_and_cleans_the_accumulator(n):
    gw, aw = _operands(n, 77)
    g, acc = gw[:n], aw[:n]
    acc[n - 1] = float("inf")                                                   # (the scalar tail at both sizes)
    acc[0] = float("nan")
    cell = torch.tensor([0.5], dtype=torch.float32, device=DEV)
    want = (acc + g) * cell
    _lib.call("rd_grad_accumulate_close", n, ops._ptr(g), ops._ptr(acc), ops._ptr(cell), ops._stream())
    torch.cuda.synchronize()
    assert bool(torch.isinf(g[n - 1])) and bool(torch.isnan(g[0])) and bool(torch.isfinite(g[1:n - 1]).all())
    assert torch.equal(_bits(g[1:]), _bits(want[1:]))
    assert torch.equal(_bits(acc), torch.zeros(n, dtype=torch.int32, device=DEV))
    assert _guard_intact(gw, n) and _guard_intact(aw, n)


# ---- 2. the step equals its restatement -----------------------------------------------------------------------------------------------
def _restate(plain, flat, buf, micro, k, opt=None):
    """the plain step over `micro`, `k` at a time: the gradients g_i, the windows' means ((g1 + g2) + ..) * float32(1 / len) formed
    by torch, the losses; with `opt`, every window's mean is put into the flat buffer and `opt.step()` applies it"""
    grads, means, losses = [], [], []
    for w in range(0, len(micro), k):
        s = torch.zeros_like(flat.flat)                                         # the accumulator starts at +0
        win = micro[w:w + k]
        for mb in win:
            _fill(buf, mb)
            losses.append(plain.run().clone())
            grads.append(flat.flat.clone())
            s = s + grads[-1]
        means.append(s * torch.tensor(1.0 / len(win), dtype=torch.float32, device=DEV))
        if opt is not None:
            flat.flat.copy_(means[-1])
            opt.step()
    return grads, means, losses


FORMS = {"eager": dict(use_graph=False, split=False), "graph": dict(use_graph=True, split=False),
         "split": dict(use_graph=True, split=True), "eager_split": dict(use_graph=False, split=True)}


@pytest.mark.parametrize("token_plan", [True, False], ids=["plan", "padded"])
@pytest.mark.parametrize("form", list(FORMS))
def test_step_equals_its_restatement(form, token_plan, precision_mode):
    """TINY, B = 4, dropout 0.2, accumulate = 3: flat.flat after the third run() is ((g1 + g2) + g3) * float32(1/3) of a plain step's
    gradients over the same micro-batches at the same seed-cell values, bit for bit; on the way the buffer holds each micro-batch's
    own gradient, and a second window starts from a clean accumulator."""
    cfg = synth.make_config("TINY")
    micro = [_to_dev(synth.make_batch(cfg, 4, seed=50 + i)) for i in range(6)]
    plain, pflat, _, pbuf = _make(cfg, 4, token_plan=token_plan, **FORMS[form])
    step, flat, _, buf = _make(cfg, 4, token_plan=token_plan, accumulate=3, **FORMS[form])
    try:
        assert step.split == plain.split == FORMS[form]["split"] and (step.graph is not None) == FORMS[form]["use_graph"]
        assert step.acc is not None and not bool(step.acc.any()) and float(step.scale_cell) == np.float32(1.0 / 3.0)
        plain.seed_cell.zero_()
        step.seed_cell.zero_()
        grads, means, _ = _restate(plain, pflat, pbuf, micro, 3)
        assert not torch.equal(grads[0], grads[1])
        for i, mb in enumerate(micro):
            _fill(buf, mb)
            assert step.window_position() == i % 3
            step.run()
            torch.cuda.synchronize()
            closing = i % 3 == 2
            assert step.window_closed == closing
            want = means[i // 3] if closing else grads[i]
            assert torch.equal(_bits(flat.flat), _bits(want)), (form, i)
            assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(flat.params, flat.views))
            if closing:
                assert not bool(_bits(step.acc).any())
        assert step.window_position() == 0 and int(step.seed_cell) == int(plain.seed_cell) == 6
    finally:
        plain.close()
        step.close()


def test_beta_step_equals_its_restatement(precision_mode):
    cfg = synth.make_config("P19")
    micro = [_to_dev(synth.make_batch(cfg, 8, seed=60 + i)) for i in range(3)]
    plain, pflat, _, pbuf = _make(cfg, 8, beta=True, token_plan=True)
    step, flat, _, buf = _make(cfg, 8, beta=True, token_plan=True, accumulate=3)
    try:
        plain.seed_cell.zero_()
        step.seed_cell.zero_()
        _, means, _ = _restate(plain, pflat, pbuf, micro, 3)
        for mb in micro:
            _fill(buf, mb)
            step.run()
        torch.cuda.synchronize()
        assert step.window_closed and torch.equal(_bits(flat.flat), _bits(means[0]))
    finally:
        plain.close()
        step.close()


def test_refusals():
    from raindrop_amd.step import TrainStep
    cfg = synth.make_config("TINY")
    for bad in (0, -1, 2.5, "2", True):
        with pytest.raises(ValueError, match="accumulate"):
            _make(cfg, 4, use_graph=False, accumulate=bad)
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 21).train()
    named = dict(m.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)], n_buckets=2)
    b = {k: v for k, v in _to_dev(synth.make_batch(cfg, 4, seed=3)).items() if k != "y"}
    with pytest.raises(ValueError, match="module_mode"):
        TrainStep(m, flat, b, use_graph=False, module_mode=True, accumulate=2)


# ---- 3. against the large batch ---------------------------------------------------------------------------------------------------------
def test_window_equals_the_large_batch():
    """dropout 0, exact fp32: four micro-batches of 8 against one plain step on the 32 samples"""
    _lib.call("rd_set_precision", 0)
    try:
        cfg = synth.make_config("TINY")
        full = synth.make_batch(cfg, 32, seed=33)
        big, bflat, _, bbuf = _make(cfg, 32, dropout=0.0, use_graph=False)
        step, flat, _, buf = _make(cfg, 8, dropout=0.0, use_graph=False, accumulate=4)
        _fill(bbuf, _to_dev(full))
        loss_big = float(big.run())
        losses = []
        for r in range(4):
            _fill(buf, _to_dev(dp.shard_batch(full, r, 4)))
            losses.append(float(step.run()))
        torch.cuda.synchronize()
        g_ref, g = bflat.flat.cpu().numpy(), flat.flat.cpu().numpy()
        gscale = np.abs(g_ref).max()
        print("max |dg| / max |g| = %.3e, |d loss| = %.3e" % (np.abs(g - g_ref).max() / gscale, abs(np.mean(losses) - loss_big)))
        assert step.window_closed and gscale > 0
        assert np.abs(g - g_ref).max() <= DP_GRAD_BOUND * gscale
        assert abs(float(np.mean(np.asarray(losses, dtype=np.float32))) - loss_big) <= DP_LOSS_BOUND
    finally:
        _lib.call("rd_set_precision", 1)


# ---- 4. the whole-step graphs -----------------------------------------------------------------------------------------------------------
OPT_KW = dict(lr=1e-3, max_grad_norm=1.0, ema_decay=0.9, schedule=LRSchedule.linear_warmup(4, start=0.1))


def _log_hooks():
    lib = _lib.load()
    on, read = lib.rd_debug_launch_log, lib.rd_debug_launch_log_read
    on.argtypes, on.restype = [ctypes.c_int], None
    read.argtypes, read.restype = [ctypes.c_char_p, ctypes.c_size_t], ctypes.c_size_t
    return on, read


class _Counted:
    """a graph whose replays are counted"""

    def __init__(self, graph, name, calls):
        self.graph, self.name, self.calls = graph, name, calls

    def replay(self):
        self.calls.append(self.name)
        self.graph.replay()


def _capture_logged(step, opt, monkeypatch):
    """capture_full with the kernels each captured graph launches read from the launch log: [names of graph 0, names of graph 1]"""
    from raindrop_amd import step as step_mod
    on, read = _log_hooks()
    real, logs = step_mod.capture_graphs, []

    def logged(bodies, warm=None):
        def wrap(body):
            def run():
                on(1)
                try:
                    body()
                    out = ctypes.create_string_buffer(1 << 16)
                    read(out, len(out))
                    logs.append(set(out.value.decode().split("\n")) - {""})
                finally:
                    on(0)
            return run
        return real([wrap(b) for b in bodies], warm=warm or (lambda: [b() for b in bodies]))
    monkeypatch.setattr(step_mod, "capture_graphs", logged)
    try:
        step.capture_full(opt)
    finally:
        monkeypatch.setattr(step_mod, "capture_graphs", real)
    return logs


def _is_update(name):
    return name.startswith("k_adam") or name.startswith("k_sumsq")


def test_whole_step_graphs_update_once_per_window(precision_mode, monkeypatch):
    """accumulate = 2, four run_full(): the micro graph holds no update and no collective, the closing graph does; the optimizer
    moves per window; the parameters equal a second model's, driven by the plain step + the restated mean + opt.step()."""
    cfg = synth.make_config("P19")
    micro = [_to_dev(synth.make_batch(cfg, 8, seed=70 + i)) for i in range(4)]
    plain, pflat, popt, pbuf = _make(cfg, 8, opt_kw=OPT_KW)
    step, flat, opt, buf = _make(cfg, 8, opt_kw=OPT_KW, accumulate=2)
    reduces = []
    monkeypatch.setattr(flat, "allreduce", lambda: reduces.append("all"))
    try:
        logs = _capture_logged(step, opt, monkeypatch)
        assert len(logs) == 2 and step.captures == 1
        micro_log, close_log = logs
        assert "k_grad_accumulate" in micro_log and not any(_is_update(n) or n == "k_grad_accumulate_close" for n in micro_log), micro_log
        assert {"k_grad_accumulate_close", "k_sumsq_partial", "k_adam_clip_ema_dev"} <= close_log and "k_grad_accumulate" not in close_log
        assert (step.plan is not None) == (precision_mode == "bf16x3")
        reduces.clear()                                                         # (the warm-up's and the closing capture's)
        calls = []
        step.graph_full_micro = _Counted(step.graph_full_micro, "micro", calls)
        step.graph_full = _Counted(step.graph_full, "close", calls)
        plain.seed_cell.zero_()
        step.seed_cell.zero_()
        _, means, losses = _restate(plain, pflat, pbuf, micro, 2, opt=popt)
        p0 = opt.param.data.clone()
        for i, mb in enumerate(micro):
            _fill(buf, mb)
            loss = step.run_full()
            torch.cuda.synchronize()
            assert torch.equal(_bits(loss), _bits(losses[i]))
            assert step.window_closed == (i % 2 == 1) and opt.t == (i + 1) // 2
            if i == 0:
                assert torch.equal(_bits(opt.param.data), _bits(p0)) and not bool(opt.exp_avg.any())
                assert opt.device_steps() == 0
        assert calls == ["micro", "close", "micro", "close"] and reduces == []  # (one process: the closing graph's collective is a no-op)
        assert opt.t == 2 and opt.device_steps() == 2 and opt.schedule_position() == 2 and opt.ema_updates() == 2
        torch.cuda.synchronize()
        assert popt.t == 2 and torch.equal(_bits(flat.flat), _bits(means[1]))
        assert torch.equal(_bits(opt.param.data), _bits(popt.param.data))
        assert torch.equal(_bits(opt.exp_avg_sq), _bits(popt.exp_avg_sq)) and torch.equal(_bits(opt.ema), _bits(popt.ema))
        assert float((opt.param.data - p0).abs().max()) > 0 and opt.grad_stats()["skipped"] == 0
    finally:
        plain.close()
        step.close()


def _labelled(cfg, N, seed):
    data = synth.make_batch(cfg, N, seed=seed)
    y = np.random.default_rng(seed).integers(0, cfg["n_classes"], N)
    return feed.DeviceDataset(data["src"], data["times"], data["static"], torch.from_numpy(y), device=DEV)


def test_fed_window_cut_short_and_a_poisoned_window(precision_mode):
    """An EpochFeed of 5 batches, accumulate = 2: run_full x 4, then run_full(close_window=True) -- five records, three updates, the
    third from the fifth micro-batch alone (scale 1.0), against the restatement bit for bit; the accumulator and the position are
    clean.  Then a window with an inf planted in the accumulator: the update is skipped, parameters and moments keep their bits,
    and the next window is clean again."""
    cfg = synth.make_config("TINY")
    B = 8
    ds = _labelled(cfg, 40, seed=71)
    rng = np.random.default_rng(9)
    plan = [rng.integers(0, 40, B) for _ in range(5)]
    fd = feed.EpochFeed(ds, B, capacity=5)
    plain, pflat, popt, _ = _make(cfg, B, opt_kw=OPT_KW)
    step, flat, opt, _ = _make(cfg, B, opt_kw=OPT_KW, accumulate=2, feed=fd)
    out = ds.alloc(B)
    pbuf = dict(src=out["P"], times=out["Ptime"], static=out["Pstatic"], y=out["y"], lengths=out["lengths"])
    try:
        step.capture_full(opt)
        assert fd.remaining() == 0 and not bool(step.acc.any()) and step.window_position() == 0   # the warm-up passes left no trace
        plain.seed_cell.zero_()
        step.seed_cell.zero_()
        micro = []
        for idx in plan:                                                        # the plain step's buffers are its own: hand-fed copies
            ds.batch(idx, out=out)
            micro.append({k: (None if v is None else v.clone()) for k, v in pbuf.items()})
        _, means, losses = _restate(plain, pflat, plain.batch, micro, 2, opt=popt)
        assert len(means) == 3 and popt.t == 3
        fd.load_epoch(plan)
        for i in range(5):
            step.run_full(close_window=(i == 4))
        loss_h, _ = fd.history()
        assert len(loss_h) == 5 and np.array_equal(loss_h.view(np.int32), torch.stack(losses).cpu().numpy().view(np.int32))
        assert opt.t == 3 and step.window_closed and step.window_position() == 0 and fd.remaining() == 0
        assert float(step.scale_cell) == np.float32(0.5)                        # the window's own scale was put back
        assert not bool(_bits(step.acc).any())
        assert torch.equal(_bits(flat.flat), _bits(means[2]))                   # (0 + g5) * 1.0
        torch.cuda.synchronize()
        assert torch.equal(_bits(opt.param.data), _bits(popt.param.data)) and torch.equal(_bits(opt.ema), _bits(popt.ema))
        # a poisoned window: position 0 runs, then an inf lands in the accumulator; the closing replay must skip and clean up
        fd.load_epoch(plan[:4])
        step.run_full()
        step.acc[3] = float("inf")
        before = [t.clone() for t in (opt.param.data, opt.exp_avg, opt.exp_avg_sq, opt.ema)]
        step.run_full()
        torch.cuda.synchronize()
        assert opt.grad_stats()["skipped"] == 1 and opt.t == 4 and opt.ema_updates() == 3
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(before, (opt.param.data, opt.exp_avg, opt.exp_avg_sq, opt.ema)))
        assert not bool(_bits(step.acc).any()) and bool(torch.isinf(flat.flat[3]))
        step.run_full()
        step.run_full()
        torch.cuda.synchronize()
        assert opt.grad_stats()["skipped"] == 1 and bool(torch.isfinite(flat.flat).all()) and opt.ema_updates() == 4
        step.reset_window()
        assert step.window_position() == 0 and not step.window_closed
    finally:
        plain.close()
        step.close()


# ---- 5. a re-capture inside a window ------------------------------------------------------------------------------------------------------
def test_recapture_keeps_the_window(precision_mode):
    cfg = synth.make_config("TINY")
    micro = [_to_dev(synth.make_batch(cfg, 4, seed=80 + i)) for i in range(2)]
    a, aflat, aopt, abuf = _make(cfg, 4, opt_kw=dict(lr=1e-3), accumulate=2)
    b, bflat, bopt, bbuf = _make(cfg, 4, opt_kw=dict(lr=1e-3, betas=(0.8, 0.99)), accumulate=2)
    try:
        a.capture_full(aopt)
        b.capture_full(bopt)
        a.seed_cell.zero_()
        b.seed_cell.zero_()
        for k, (x, xbuf, xopt) in enumerate(((a, abuf, aopt), (b, bbuf, bopt))):
            _fill(xbuf, micro[0])
            x.run_full()
            if k == 0:
                xopt.betas = (0.8, 0.99)                                        # launch constants of the captured update: a new capture
            _fill(xbuf, micro[1])
            x.run_full()
        torch.cuda.synchronize()
        assert a.captures == 2 and b.captures == 1 and a.window_position() == 0 and a.window_closed
        assert int(a.seed_cell) == int(b.seed_cell) == 2 and aopt.t == bopt.t == 1
        for x, y in ((aflat.flat, bflat.flat), (aopt.param.data, bopt.param.data), (aopt.exp_avg, bopt.exp_avg), (aopt.exp_avg_sq, bopt.exp_avg_sq)):
            assert torch.equal(_bits(x), _bits(y))
        assert bool(aopt.exp_avg.any()) and not bool(_bits(a.acc).any())
    finally:
        a.close()
        b.close()


# ---- 6. two ranks on one device over gloo -------------------------------------------------------------------------------------------------
B_GLOBAL = 16


def _dp_window(batches, split, count=None):
    """accumulate = 2 over `batches` (two of them) with run_allreduce(); returns (gradient, collectives per call)"""
    from raindrop_amd.step import TrainStep
    cfg = synth.make_config("P19")
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 21).train()
    named = dict(m.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)], n_buckets=2)
    buf = _to_dev(batches[0])
    ts = TrainStep(m, flat, buf, p_drop=0.0, use_graph=True, autotune=False, split=split, accumulate=2)
    calls = []
    real_all, real_range = flat.allreduce, flat.allreduce_range_async
    flat.allreduce = lambda: (calls.append("all"), real_all())[1]
    flat.allreduce_range_async = lambda lo, hi: (calls.append("range"), real_range(lo, hi))[1]
    per_call = []
    try:
        for b in batches:
            _fill(buf, _to_dev(b))
            del calls[:]
            ts.run_allreduce()
            per_call.append((list(calls), ts.window_closed))
        torch.cuda.synchronize()
        return flat.flat.detach().cpu().numpy().copy(), per_call, ts.split
    finally:
        ts.close()


def _dp_batches():
    cfg = synth.make_config("P19")
    return [synth.make_batch(cfg, B_GLOBAL, seed=s) for s in (33, 34)]


def _dp_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    shards = [dp.shard_batch(b, rank, world) for b in _dp_batches()]
    ret[rank] = [_dp_window(shards, split) for split in (False, True)]
    dist.destroy_process_group()


def test_two_ranks_reduce_once_per_window():
    world, port = 2, _free_port()
    ret = mp.Manager().dict()
    mp.spawn(_dp_worker, args=(world, port, ret), nprocs=world, join=True)
    # the restatement: every rank's window mean from a plain step in this process (no group: world == 1), then the ranks' average
    from raindrop_amd.step import TrainStep
    cfg = synth.make_config("P19")
    means = []
    for r in range(world):
        m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 21).train()
        named = dict(m.named_parameters())
        flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)], n_buckets=2)
        shards = [_to_dev(dp.shard_batch(b, r, world)) for b in _dp_batches()]
        ts = TrainStep(m, flat, shards[0], p_drop=0.0, use_graph=False, split=False)
        gs = []
        for s in shards:
            _fill(ts.batch, s)
            ts.run()
            gs.append(flat.flat.clone())
        means.append(((gs[0] + gs[1]) * 0.5).cpu().numpy())
        ts.close()
    want = (means[0] + means[1]) / np.float32(world)
    gscale = np.abs(want).max()
    for k, split in enumerate((False, True)):
        (g0, calls0, split0), (g1, calls1, split1) = ret[0][k], ret[1][k]
        assert split0 == split1 == split
        closing = ["range", "range"] if split else ["all"]
        assert calls0 == calls1 == [([], False), (closing, True)], (split, calls0)
        assert np.array_equal(g0, g1)
        print("split=%d: max |dg| / max |g| = %.3e" % (split, np.abs(g0 - want).max() / gscale))
        assert np.abs(g0 - want).max() <= DP_GRAD_BOUND * gscale


# ---- 7. the default is untouched ------------------------------------------------------------------------------------------------------------
def test_accumulate_one_is_the_recorded_step():
    """accumulate=1, spelled out: the launch traces of one run() and one run_full() are tests/golden/step_launches.json's (read, never
    regenerated), and the step allocates no accumulator and captures no second graph."""
    from raindrop_amd.step import TrainStep
    spec = importlib.util.spec_from_file_location("make_step_launches", os.path.join(GOLDEN, "make_step_launches.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = json.load(open(os.path.join(GOLDEN, "step_launches.json")))
    _lib.call("rd_set_precision", 1)
    for cfg_name in ("p19", "tiny"):
        cfg, B = gen.configs()[cfg_name]
        with gen.recording() as rec:
            ts = gen._train(rec, cfg, B, split=False, accumulate=1)
        torch.cuda.synchronize()
        assert json.loads(json.dumps(rec.trace)) == want[cfg_name + "/run"]
        assert ts.acc is None and ts.scale_cell is None and ts.window_closed and ts.window_position() == 0
    cfg, B = gen.configs()["p19"]
    with gen.recording() as rec:
        m, b = gen.make(cfg, B)
        flat = gen.flat_of(m, cfg)
        opt = FlatAdam(flat.flatten_parameters(), lr=1e-3)
        ts = TrainStep(m, flat, b, use_graph=False, autotune=False, split=False, accumulate=1)
        ts.capture_full(opt)
        rec.mark("captured")
        ts.run_full()
        assert ts.acc is None and ts.graph_full_micro is None and ts.graph_close is None
        ts.close()
    torch.cuda.synchronize()
    assert json.loads(json.dumps(rec.trace)) == want["p19/full"]


# ---- 8. fit ---------------------------------------------------------------------------------------------------------------------------------
def test_fit_accumulates():
    from raindrop_amd import trainer
    from tests.test_epoch_feed_gpu import _fit_model, _split
    cfg, ds, ytrain, vds = _split()
    E, B, k = 3, 128, 2
    n_batches = feed.EpochPlanner(ytrain, batch_size=B, strategy=2, n_total=ds.N).n_batches
    per_epoch = -(-n_batches // k)
    np.random.seed(0)
    r = trainer.fit(_fit_model(cfg), ds, vds, E, batch_size=B, strategy=2, lr=1e-3, scheduler=False, autotune=False, accumulate=k,
                    lr_schedule="warmup_cosine", warmup_steps=2, max_grad_norm=1.0)
    print("n_batches", n_batches, "optimizer_steps", r["optimizer_steps"], "train_loss", r["train_loss"], "lr_step", r["lr_step"])
    assert n_batches >= 2 and r["optimizer_steps"] == E * per_epoch
    assert len(r["train_loss"]) == E and all(np.isfinite(x) for x in r["train_loss"])
    assert len(r["lr_step"]) == r["optimizer_steps"]
    sched = LRSchedule.warmup_cosine(E * per_epoch, warmup=2)
    assert r["lr_step"] == [1e-3 * f for f in sched.factors]
    assert all(np.isfinite(x) for x in r["val_loss"]) and r["lr"] == [1e-3] * E
