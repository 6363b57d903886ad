"""GPU: the epoch feed -- rd_feed_gather against rd_batch_gather, rd_feed_record against torch.argmax, a step that feeds itself
against the same step fed by hand (bit for bit, in every form of the step), the refusal behind the last batch, and `trainer.fit`
against a hand-written loop over the same pieces."""
import ctypes

import numpy as np
import pytest
import torch

from raindrop_amd import _lib, feed, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                                                       # words behind every output buffer


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _i64(vals):
    return torch.tensor(vals, dtype=torch.int64, device=DEV)


@pytest.fixture(params=["bf16x3", "fp32"])
def precision_mode(request):
    _lib.call("rd_set_precision", 1 if request.param == "bf16x3" else 0)
    yield request.param
    _lib.call("rd_set_precision", 1)


# ---- 1. the gather -----------------------------------------------------------------------------------------------------------------
class _Outs:
    """src, times, static, y, lengths, each with GUARD sentinel words behind it"""
    SENT = {torch.float32: 12345.0, torch.int64: -77}

    def __init__(self, T, B, W, dstat):
        shapes = dict(src=((T, B, W), torch.float32), times=((T, B), torch.float32), y=((B,), torch.int64), lengths=((B,), torch.int64))
        if dstat:
            shapes["static"] = ((B, dstat), torch.float32)
        self.whole, self.t = {}, {"static": None}
        for k, (shape, dt) in shapes.items():
            n = int(np.prod(shape))
            self.whole[k] = torch.full((n + GUARD,), self.SENT[dt], dtype=dt, device=DEV)
            self.t[k] = self.whole[k][:n].view(shape)

    def guards_intact(self):
        return all(bool((w[-GUARD:] == self.SENT[w.dtype]).all()) for w in self.whole.values())

    def same(self, other):
        return all(torch.equal(self.t[k].view(torch.int32) if self.t[k].dtype == torch.float32 else self.t[k],
                               other.t[k].view(torch.int32) if other.t[k].dtype == torch.float32 else other.t[k]) for k in self.whole)


def _gather_case(T, B, W, dstat, N=23, n=5):
    g = torch.Generator().manual_seed(1000 * T + B)
    P = torch.randn((T, N, W), generator=g)
    times = torch.rand((T, N), generator=g) * (torch.rand((T, N), generator=g) < 0.7)
    ds = feed.DeviceDataset(P, times, torch.randn((N, dstat), generator=g) if dstat else None,
                            torch.randint(0, 2, (N,), generator=g), device=DEV)
    plan = torch.randint(0, N, (n, B), generator=g).to(DEV)
    return ds, plan


def _feed_gather(ds, plan, cell, outs, bad, capacity=None):
    T, B, W = outs.t["src"].shape
    o = outs.t
    _lib.call("rd_feed_gather", T, B, W, ds.ds, ds.N, plan.shape[0] if capacity is None else capacity, _p(ds.P), _p(ds.Ptime), _p(ds.Pstatic),
              _p(ds.y), _p(plan), _p(cell), _p(o["src"]), _p(o["times"]), _p(o["static"]), _p(o["y"]), _p(o["lengths"]), _p(bad), _stream())


def _batch_gather(ds, idx, outs, bad):
    T, B, W = outs.t["src"].shape
    o = outs.t
    _lib.call("rd_batch_gather", T, B, W, ds.ds, ds.N, _p(ds.P), _p(ds.Ptime), _p(ds.Pstatic), _p(ds.y), _p(idx), _p(o["src"]),
              _p(o["times"]), _p(o["static"]), _p(o["y"]), _p(o["lengths"]), _p(bad), _stream())


# scalar path, B below one 16-row group and one 4-sample tail group | 16-byte rows, T above the 64-lane loop, ragged B | P19
GATHER_SHAPES = [(5, 3, 6, 0), (70, 19, 8, 5), (60, 32, 68, 6)]


@pytest.mark.parametrize("T,B,W,dstat", GATHER_SHAPES, ids=["T5_B3_W6", "T70_B19_W8", "P19_B32"])
def test_feed_gather_is_batch_gather_of_the_plan_row(T, B, W, dstat):
    ds, plan = _gather_case(T, B, W, dstat)
    n = plan.shape[0]
    bad_f, bad_b = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    # (cursor, n_batches) -> the row that must be read and the cursors counted as bad; the last two: n_batches beyond the plan
    cases = [(0, n, 0, 0), (n // 2, n, n // 2, 0), (n - 1, n, n - 1, 0), (-1, n, n - 1, 1), (n, n, n - 1, 1), (1, 3, 1, 0), (3, 3, 2, 1),
             (n + 2, n + 5, n - 1, 1), (0, 0, 0, 1)]
    for cursor, nb, row, bad_want in cases:
        cell = _i64([cursor, nb])
        got, want = _Outs(T, B, W, dstat), _Outs(T, B, W, dstat)
        _feed_gather(ds, plan, cell, got, bad_f)
        _batch_gather(ds, plan[row].contiguous(), want, bad_b)
        torch.cuda.synchronize()
        assert got.same(want), (cursor, nb)
        assert got.guards_intact() and want.guards_intact(), (cursor, nb)
        assert int(bad_f.item()) == bad_want and int(bad_b.item()) == 0, (cursor, nb)
        assert cell.tolist() == [cursor, nb]                                  # the gather never writes the cell
        assert torch.equal(got.t["lengths"], (got.t["times"] > 0).sum(0))
        bad_f.zero_()
    # sample indices outside [0, N): clamped and counted like rd_batch_gather's
    plan2 = plan.clone()
    plan2[1, 0], plan2[1, B - 1] = -3, ds.N + 5
    got, want = _Outs(T, B, W, dstat), _Outs(T, B, W, dstat)
    _feed_gather(ds, plan2, _i64([1, n]), got, bad_f)
    _batch_gather(ds, plan2[1].contiguous(), want, bad_b)
    torch.cuda.synchronize()
    assert got.same(want) and got.guards_intact()
    assert int(bad_f.item()) == int(bad_b.item()) == (2 if B > 1 else 1)


# ---- 2. the record -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 8])
@pytest.mark.parametrize("B", [1, 19, 256])
def test_feed_record_writes_one_slot_and_advances_the_cursor(B, C):
    g = torch.Generator().manual_seed(B * 10 + C)
    logits = torch.randint(0, 3, (B, C), generator=g).float()                # three values over C classes: ties in most rows
    logits[0] = 1.0                                                           # an all-tie row: class 0 wins
    y = torch.randint(0, C, (B,), generator=g)
    y[0] = 0
    want = int((logits.argmax(1) == y).sum())
    assert B == 1 or int((logits.max(1).values.unsqueeze(1) == logits).sum(1).max()) >= 2        # the inputs do contain ties
    logits_d, y_d = logits.to(DEV), y.to(DEV)
    assert int((logits_d.argmax(1) == y_d).sum()) == want
    cap, n, k = 6, 5, 3
    loss = torch.tensor(3.25, device=DEV)

    def run(cursor, nb):
        cell = _i64([cursor, nb])
        lh = torch.full((cap + GUARD,), -1.0, device=DEV)
        ch = torch.full((cap + GUARD,), -5, dtype=torch.int32, device=DEV)
        _lib.call("rd_feed_record", B, C, cap, _p(cell), _p(loss), _p(logits_d), _p(y_d), _p(lh), _p(ch), _stream())
        torch.cuda.synchronize()
        return cell.tolist(), lh.tolist(), ch.tolist()

    for cursor in (0, k, n - 1):
        cell, lh, ch = run(cursor, n)
        assert cell == [cursor + 1, n]
        assert lh == [3.25 if i == cursor else -1.0 for i in range(cap + GUARD)]
        assert ch == [want if i == cursor else -5 for i in range(cap + GUARD)]
    for cursor, nb in ((-1, n), (n, n), (cap, cap + 4), (0, 0)):             # outside [0, min(n_batches, capacity)): nothing moves
        cell, lh, ch = run(cursor, nb)
        assert cell == [cursor, nb] and lh == [-1.0] * (cap + GUARD) and ch == [-5] * (cap + GUARD)


# ---- 3. a step that feeds itself against the same step fed by hand -----------------------------------------------------------------------
OPT_KW = dict(max_grad_norm=1.0, ema_decay=0.99)


def _labelled(cfg, N, seed):
    data = synth.make_batch(cfg, N, seed=seed)
    y = np.random.default_rng(seed).integers(0, cfg["n_classes"], N)
    return feed.DeviceDataset(data["src"], data["times"], data["static"], torch.from_numpy(y), device=DEV)


def _stepper(cfg, ds, B, beta, fd, **step_kw):
    """(step, opt, out): P19 / TINY model (parameter seed 21, dropout 0.2), FlatAdam with clipping and averaging, and the buffers
    `ds.batch(idx, out=out)` fills, which are the step's batch"""
    from raindrop_amd import dp
    from raindrop_amd.optim import FlatAdam
    from raindrop_amd.step import TrainStep
    from raindrop_amd.step_beta import BetaTrainStep
    from tests.helpers import build_ours
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 21, **(dict(use_beta=True) if beta else {})).train()
    m.dropout.p = 0.2
    named = dict(m.named_parameters())
    names = synth.live_parameter_names_beta(cfg) if beta else synth.live_parameter_names(cfg)
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in names], n_buckets=2)
    opt = FlatAdam(flat.flatten_parameters(), lr=1e-3, **OPT_KW)
    out = ds.alloc(B)
    ds.batch(np.arange(B), out=out)
    batch = dict(src=out["P"], times=out["Ptime"], static=out["Pstatic"], y=out["y"], lengths=out["lengths"])
    step = (BetaTrainStep if beta else TrainStep)(m, flat, batch, autotune=False, feed=fd, **step_kw)
    return step, opt, out


# name -> (configuration, B, use_beta, TrainStep keywords, whole-step graph?)
FORMS = {"full": ("P19", 8, False, {}, True), "run": ("P19", 8, False, {}, False), "eager": ("P19", 8, False, dict(use_graph=False), False),
         "split": ("P19", 8, False, dict(split=True), False), "split_full": ("P19", 8, False, dict(split=True), True),
         "beta": ("P19", 4, True, {}, True), "tiny": ("TINY", 8, False, {}, True)}


@pytest.mark.parametrize("form", list(FORMS))
def test_fed_step_equals_hand_fed_step(form, precision_mode):
    """two identically seeded models, the same row-block masks (autotune=False), the same number of warm-up passes: A is fed by
    ds.batch(idx, out=) in front of every step, B by its feed.  Losses, history, flat parameters and their average bit-equal after
    an epoch of 4 batches and after a second one of 3 on the same graphs."""
    cfg_name, B, beta, step_kw, full = FORMS[form]
    cfg = synth.make_config(cfg_name)
    ds = _labelled(cfg, 40, seed=71)
    rng = np.random.default_rng(9)
    epochs = [[rng.integers(0, 40, B) for _ in range(nb)] for nb in (4, 3)]
    fd = feed.EpochFeed(ds, B, capacity=4)
    a, opt_a, out_a = _stepper(cfg, ds, B, beta, None, **step_kw)
    b, opt_b, _ = _stepper(cfg, ds, B, beta, fd, **step_kw)
    assert a.split == b.split == bool(step_kw.get("split", False))
    try:
        if full:
            a.capture_full(opt_a)
            b.capture_full(opt_b)
        graphs = (b.graph, b.graph_b, b.graph_full)
        assert fd.remaining() == 0 and fd.bad_indices() == 0 and fd.cell.tolist() == [0, 0]      # the warm-up passes left no trace

        def one(step, opt):
            if full:
                return step.run_full().clone()
            loss = step.run().clone()
            opt.step()
            return loss

        for plan in epochs:
            want_loss, want_correct = [], []
            for idx in plan:
                ds.batch(idx, out=out_a)
                want_loss.append(one(a, opt_a))
                want_correct.append(int((a.logits.argmax(1) == out_a["y"]).sum()))
            fd.load_epoch(plan)
            assert fd.remaining() == len(plan)
            got_loss = [one(b, opt_b) for _ in plan]
            loss_h, correct_h = fd.history()
            want = torch.stack(want_loss).cpu().numpy()
            print(form, precision_mode, "losses", want.tolist(), "correct", want_correct)
            assert np.isfinite(want).all() and len(set(want.tolist())) == len(plan)              # different batches, different losses
            assert np.array_equal(torch.stack(got_loss).cpu().numpy().view(np.int32), want.view(np.int32))
            assert loss_h.dtype == np.float32 and np.array_equal(loss_h.view(np.int32), want.view(np.int32))
            assert correct_h.dtype == np.int32 and correct_h.tolist() == want_correct
            assert torch.equal(opt_a.param.data.view(torch.int32), opt_b.param.data.view(torch.int32))
            assert torch.equal(opt_a.ema.view(torch.int32), opt_b.ema.view(torch.int32))
            assert torch.equal(opt_a.exp_avg_sq.view(torch.int32), opt_b.exp_avg_sq.view(torch.int32))
            assert fd.remaining() == 0 and fd.cell.tolist() == [len(plan)] * 2 and fd.bad_indices() == 0
        assert (b.graph, b.graph_b, b.graph_full) == graphs and b.captures == (1 if full else 0)   # no new capture
        assert opt_b.t == opt_a.t == 7 and float((opt_b.ema - opt_b.param.data).abs().max()) > 0.0
    finally:
        a.close()
        b.close()


# ---- 4. behind the last batch ------------------------------------------------------------------------------------------------------------
def test_a_step_past_the_end_is_refused_and_changes_nothing():
    cfg = synth.make_config("TINY")
    ds = _labelled(cfg, 40, seed=72)
    fd = feed.EpochFeed(ds, 8, capacity=3)
    step, opt, _ = _stepper(cfg, ds, 8, False, fd)
    try:
        step.capture_full(opt)
        with pytest.raises(_lib.RaindropHipError, match="used up"):
            step.run_full()                                                    # nothing loaded yet
        fd.load_epoch([np.arange(8), np.arange(8, 16)])
        step.run_full()
        step.run_full()
        torch.cuda.synchronize()
        before = [t.clone() for t in (fd.cell, fd._hist, opt.param.data, opt.ema, opt.exp_avg)]
        for call in (step.run_full, step.run):
            with pytest.raises(_lib.RaindropHipError, match="used up"):
                call()
        torch.cuda.synchronize()
        after = (fd.cell, fd._hist, opt.param.data, opt.ema, opt.exp_avg)
        assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
                   for x, y in zip(before, after))
        assert fd.cell.tolist() == [2, 2] and opt.t == 2 and len(fd.history()[0]) == 2 and fd.bad_indices() == 0
        with pytest.raises(ValueError, match="capacity"):
            fd.load_epoch([np.arange(8)] * 4)
        with pytest.raises(IndexError):
            fd.load_epoch([np.arange(33, 41)])
        with pytest.raises(ValueError, match="batch_size"):
            fd.load_epoch([np.arange(7)])
        assert fd.cell.tolist() == [2, 2]                                      # a refused plan is not uploaded
    finally:
        step.close()


def test_constructor_refusals():
    from raindrop_amd import dp
    from raindrop_amd.step import TrainStep
    from tests.helpers import build_ours
    cfg = synth.make_config("TINY")
    ds = _labelled(cfg, 40, seed=73)
    with pytest.raises(_lib.RaindropHipError, match="labels"):
        feed.EpochFeed(feed.DeviceDataset(ds.P, ds.Ptime, ds.Pstatic, None, device=DEV), 8, 2)
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 21).train()
    named = dict(m.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)], n_buckets=2)
    out = ds.alloc(8)
    ds.batch(np.arange(8), out=out)
    batch = dict(src=out["P"], times=out["Ptime"], static=out["Pstatic"], y=out["y"], lengths=out["lengths"])
    with pytest.raises(ValueError, match="gathers src"):
        TrainStep(m, flat, batch, use_graph=False, feed=feed.EpochFeed(ds, 4, 2))                 # another batch size
    with pytest.raises(ValueError, match="module_mode"):
        TrainStep(m, flat, {k: v for k, v in batch.items() if k != "y"}, use_graph=False, module_mode=True, feed=feed.EpochFeed(ds, 8, 2))


# ---- 5. fit --------------------------------------------------------------------------------------------------------------------------------
def _split():
    """the synthetic split of tests/test_train_loop_gpu.py, the validation part with labels of the same kind"""
    cfg = synth.make_config("P19")

    def part(N, seed, rseed):
        data = synth.make_batch(cfg, N, seed=seed)
        y = ((data["src"][:, :, 0].sum(0).numpy() + 0.5 * np.random.default_rng(rseed).standard_normal(N)) > 0).astype(np.int64)
        if y.mean() > 0.5:
            y = 1 - y                                                          # class 1 is the minority the plan triples
        return feed.DeviceDataset(data["src"], data["times"], data["static"], torch.from_numpy(y), device=DEV), y
    (ds, ytrain), (vds, _) = part(640, 71, 5), part(96, 72, 6)
    return cfg, ds, ytrain, vds


def _fit_model(cfg):
    from tests.helpers import build_ours
    m = build_ours(cfg, synth.make_structure(cfg, "ones"), DEV, 3)
    m.dropout.p = 0.2
    return m


def test_fit_runs_the_scripts_loop(precision_mode):
    from raindrop_amd import dp, trainer
    from raindrop_amd.optim import FlatAdam
    from raindrop_amd.step import TrainStep
    cfg, ds, ytrain, vds = _split()
    B, E = 128, 2
    # the hand-written loop: planner, ds.batch(out=), the whole-step graph
    np.random.seed(0)
    m = _fit_model(cfg).train()
    named = dict(m.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)], n_buckets=2)
    opt = FlatAdam(flat.flatten_parameters(), lr=1e-3)
    planner = feed.EpochPlanner(ytrain, batch_size=B, strategy=2, n_total=ds.N)
    assert planner.n_batches >= 2
    out = ds.alloc(B)
    ds.batch(np.arange(B), out=out)
    step = TrainStep(m, flat, dict(src=out["P"], times=out["Ptime"], static=out["Pstatic"], y=out["y"], lengths=out["lengths"]), autotune=False)
    want = []
    try:
        step.capture_full(opt)
        for _ in range(E):
            losses = []
            for idx in planner.next_epoch():
                ds.batch(idx, out=out)
                losses.append(step.run_full().clone())
            want.append(torch.stack(losses).cpu().numpy().mean())
    finally:
        step.close()
    # the same under fit
    np.random.seed(0)
    m2 = _fit_model(cfg).eval()
    r = trainer.fit(m2, ds, vds, E, batch_size=B, strategy=2, lr=1e-3, scheduler=False, autotune=False)
    print(precision_mode, "train_loss", r["train_loss"], "hand", [float(w) for w in want], "val_auroc", r["val_auroc"], "val_auprc", r["val_auprc"])
    assert all(len(r[k]) == E for k in r if k not in ("best_epoch", "best_auroc"))
    assert sorted(r) == sorted(["train_loss", "train_accuracy", "lr", "best_epoch", "best_auroc"] + ["val_" + f for f in trainer.VAL_FIELDS])
    assert all(w.dtype == np.float32 for w in want) and [np.float32(x) for x in r["train_loss"]] == want
    assert all(0.0 <= x <= 1.0 for x in r["train_accuracy"]) and r["lr"] == [1e-3] * E
    assert r["best_epoch"] is not None and r["best_auroc"] == max(r["val_auroc"]) == r["val_auroc"][r["best_epoch"]]
    assert not m2.training                                                     # fit trained in training mode and put eval() back
    assert feed.validate(m2, vds)["auroc"] == r["best_auroc"]                  # the best weights are the model's


def test_fit_steps_the_scheduler_on_auprc():
    """ReduceOnPlateau(patience=0, threshold_mode='abs', threshold=1.0): an auprc lies in [0, 1], so after the first epoch (better than
    -inf) no epoch can beat the best by more than 1 -- the rule must cut the rate after EVERY later epoch, whatever the model does.
    lr[] must be the rule replayed on the recorded auprc values."""
    from raindrop_amd import trainer
    cfg, ds, _, vds = _split()
    np.random.seed(0)
    kw = dict(patience=0, threshold_mode="abs", threshold=1.0)
    r = trainer.fit(_fit_model(cfg), ds, vds, 3, batch_size=128, lr=1e-3, scheduler=trainer.ReduceOnPlateau(**kw), autotune=False)
    import types
    host = types.SimpleNamespace(lr=1e-3)
    rule = trainer.ReduceOnPlateau(host, **kw)
    want = [rule.step(a) for a in r["val_auprc"]]
    print("auprc", r["val_auprc"], "lr", r["lr"])
    assert r["lr"] == want and want[0] == 1e-3 and want[1] < want[0] and want[2] < want[1]
    assert want[1] == max(1e-3 * 0.1, 1e-8)
