"""GPU: train-time augmentation inside the batch gather -- rd_batch_gather_aug / rd_feed_gather_aug against the numpy restatement
(tests/feed_aug_ref.py) BIT FOR BIT, outputs pre-filled with NaN and followed by guard words; the plain twins' bytes at rate 0; a
fed augmented step against a hand-fed step given the restatement's batches, in every form; `fit(augment=)`."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from raindrop_amd import _lib, feed, synth
from tests import feed_aug_ref as R
from tests.test_feed_aug_ref_host import KEEP_GT_CASE, _dataset, keep_gt_seed

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                                                       # words behind every output buffer
SENT_I64 = -77


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(scope="module", autouse=True)
def _hand_back_device_memory():
    """tests/test_step_launches_gpu.py names buffers by the order in which their addresses first appear: leave no garbage behind."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _hooks():
    lib = _lib.load()
    on, read = lib.rd_debug_launch_log, lib.rd_debug_launch_log_read
    on.argtypes, on.restype = [ctypes.c_int], None
    read.argtypes, read.restype = [ctypes.c_char_p, ctypes.c_size_t], ctypes.c_size_t
    return on, read


def _logged(fn):
    """run fn with the launch log on -> the distinct names the launch sites reported"""
    on, read = _hooks()
    buf = ctypes.create_string_buffer(1 << 12)
    on(1)
    try:
        fn()
        n = read(buf, len(buf))
    finally:
        on(0)
    return set(buf.raw[:n].decode().split())


class _Outs:
    """src, times, static, y, lengths: NaN (floats) / a sentinel (integers) everywhere, GUARD more words behind each; `skew` floats
    in front of src move it off its 8- and 16-byte alignment"""

    def __init__(self, T, B, W, dstat, skew=0):
        shapes = dict(src=((T, B, W), torch.float32), times=((T, B), torch.float32), y=((B,), torch.int64), lengths=((B,), torch.int64))
        if dstat:
            shapes["static"] = ((B, dstat), torch.float32)
        self.whole, self.t, self.n, self.off = {}, {"static": None}, {}, {}
        for k, (shape, dt) in shapes.items():
            n, off = int(np.prod(shape)), (skew if k == "src" else 0)
            fill = float("nan") if dt == torch.float32 else SENT_I64
            self.whole[k] = torch.full((off + n + GUARD,), fill, dtype=dt, device=DEV)
            self.t[k], self.n[k], self.off[k] = self.whole[k][off:off + n].view(shape), n, off
        assert skew == 0 or self.t["src"].data_ptr() % 8 == 4

    def guards_intact(self):
        ok = True
        for k, w in self.whole.items():
            g = torch.cat([w[:self.off[k]], w[self.off[k] + self.n[k]:]])
            ok = ok and bool(torch.isnan(g).all() if w.dtype == torch.float32 else (g == SENT_I64).all())
        return ok

    def same(self, other):
        return all(torch.equal(_bits(self.t[k]), _bits(other.t[k])) for k in self.whole)


def _device_ds(P, tm, dstat, seed):
    g = np.random.default_rng(seed)
    N = P.shape[1]
    st = g.standard_normal((N, dstat)).astype(np.float32) if dstat else None
    y = g.integers(0, 3, N)
    return feed.DeviceDataset(torch.from_numpy(P), torch.from_numpy(tm), None if st is None else torch.from_numpy(st),
                              torch.from_numpy(y), device=DEV), st, y


def _cell(aug, epoch=0):
    return torch.from_numpy(aug.cell(epoch)).to(DEV)


def _batch_gather_aug(ds, idx, outs, bad, cell, draw, W=None):
    T, B, Wo = outs.t["src"].shape
    o = outs.t
    _lib.call("rd_batch_gather_aug", T, B, Wo if W is None else W, ds.ds if o["static"] is not None else 0, ds.N, _p(ds.P), _p(ds.Ptime),
              _p(ds.Pstatic) if o["static"] is not None else None, _p(ds.y), _p(idx), _p(o["src"]), _p(o["times"]), _p(o["static"]),
              _p(o["y"]), _p(o["lengths"]), _p(bad), _p(cell), ctypes.c_uint64(draw), _stream())


def _batch_gather(ds, idx, outs, bad):
    T, B, W = outs.t["src"].shape
    o = outs.t
    _lib.call("rd_batch_gather", T, B, W, ds.ds if o["static"] is not None else 0, ds.N, _p(ds.P), _p(ds.Ptime),
              _p(ds.Pstatic) if o["static"] is not None else None, _p(ds.y), _p(idx), _p(o["src"]), _p(o["times"]), _p(o["static"]),
              _p(o["y"]), _p(o["lengths"]), _p(bad), _stream())


def _check_against_ref(outs, P, tm, st, y, idx, key, aug, what):
    want = R.augment(P, tm, idx, key, aug.p_time, aug.p_sensor, aug.p_obs, aug.noise_c)
    got = (outs.t["src"].cpu().numpy(), outs.t["times"].cpu().numpy(), outs.t["lengths"].cpu().numpy())
    assert R.same(got, want), what
    assert np.array_equal(outs.t["y"].cpu().numpy(), y[idx]), what
    if outs.t["static"] is not None:
        assert np.array_equal(outs.t["static"].cpu().numpy().view(np.int32), st[idx].view(np.int32)), what
    assert outs.guards_intact(), what


# each rate alone, all together, and the rate that reaches the all-dropped rule
RATE_SETS = [dict(p_time=0.3), dict(p_sensor=0.25), dict(p_obs=0.2), dict(value_noise=0.05),
             dict(p_time=0.3, p_sensor=0.25, p_obs=0.2, value_noise=0.05), dict(p_time=0.999, p_obs=0.1)]
# (T, B, F, d_static, skew): F = 1, 3 the scalar path (W % 4 != 0: 2, 6), F = 2, 34 the 8-byte path (W = 4, 68), skew = 1 the scalar
# path at W = 68; T = 64 / 65 / 130 around the 64-row passes of the compaction; B = 16 / 17 / 33 around the 16-slot copy groups and
# the 4-sample tail groups
SHAPES = [(1, 1, 1, 0, 0), (4, 5, 1, 3, 0), (4, 17, 2, 0, 0), (60, 5, 34, 6, 0), (64, 16, 2, 2, 0), (65, 17, 34, 0, 0), (65, 1, 3, 2, 0),
          (130, 33, 3, 4, 0), (130, 16, 34, 0, 0), (64, 33, 34, 5, 1), (60, 17, 3, 0, 0)]


@pytest.mark.parametrize("T,B,F,dstat,skew", SHAPES, ids=["T%d_B%d_F%d%s" % (s[0], s[1], s[2], "_skew" if s[4] else "") for s in SHAPES])
def test_batch_gather_aug_equals_the_restatement(T, B, F, dstat, skew):
    N = 23
    P, tm = _dataset(T, N, F, seed=100 * T + B)
    P[0, :, 0] = np.float32(-0.0)                                            # signed zeros and denormals travel as bits
    if T > 1:
        P[1, :, 0] = np.float32(1e-40)
    ds, st, y = _device_ds(P, tm, dstat, seed=T + B)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    rng = np.random.default_rng(7 * T + B)
    for k, rates in enumerate(RATE_SETS):
        aug = feed.Augment(seed=1000 + k, **rates)
        # samples 0..3 are L = 0, 1, T and the undercount: every one of them leads the batch under some rate set
        idx = np.concatenate([(np.arange(4) + k) % 4, rng.integers(0, N, B)])[:B]
        draw = 5 + 3 * k
        outs = _Outs(T, B, 2 * F, dstat, skew)
        _batch_gather_aug(ds, torch.from_numpy(idx).to(DEV), outs, bad, _cell(aug, epoch=9), draw)     # (the cell's epoch is ignored)
        torch.cuda.synchronize()
        _check_against_ref(outs, P, tm, st, y, idx, R.batch_key(aug.seed, 0, 0, draw), aug, (rates, idx[:4]))
    assert int(bad.item()) == 0
    # DeviceDataset.batch(augment=, draw=) is the same call
    aug = feed.Augment(seed=4, **RATE_SETS[4])
    got = ds.batch(idx, augment=aug, draw=11)
    want = R.augment(P, tm, idx, R.batch_key(4, 0, 0, 11), aug.p_time, aug.p_sensor, aug.p_obs, aug.noise_c)
    assert R.same((got[0].cpu().numpy(), got[2].cpu().numpy(), got[4].cpu().numpy()), want)


def test_keep_is_u_greater_or_equal_p():
    """the case of the host test in which some uniform EQUALS p_obs"""
    c = KEEP_GT_CASE
    key = keep_gt_seed(c["T"], c["B"], c["F"], c["p_obs"])
    P, tm = _dataset(c["T"], c["N"], c["F"], seed=6, density=1.0)
    ds, st, y = _device_ds(P, tm, 0, seed=1)
    idx = np.arange(c["B"]) % c["N"]
    aug = feed.Augment(p_obs=c["p_obs"], seed=key)
    outs = _Outs(c["T"], c["B"], 2 * c["F"], 0)
    _batch_gather_aug(ds, torch.from_numpy(idx).to(DEV), outs, None, _cell(aug), 0)
    torch.cuda.synchronize()
    _check_against_ref(outs, P, tm, st, y, idx, key, aug, "u == p")


def test_out_of_range_indices_and_odd_width():
    T, B, F, N = 9, 6, 2, 23
    P, tm = _dataset(T, N, F, seed=3)
    ds, st, y = _device_ds(P, tm, 3, seed=3)
    idx = np.array([4, -3, 7, N + 5, 2, 2 ** 40])
    clamped = np.clip(idx, 0, N - 1)
    aug = feed.Augment(seed=8, **RATE_SETS[4])
    bad_a, bad_p = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    outs, plain = _Outs(T, B, 2 * F, 3), _Outs(T, B, 2 * F, 3)
    _batch_gather_aug(ds, torch.from_numpy(idx).to(DEV), outs, bad_a, _cell(aug), 2)
    _batch_gather(ds, torch.from_numpy(idx).to(DEV), plain, bad_p)
    torch.cuda.synchronize()
    _check_against_ref(outs, P, tm, st, y, clamped, R.batch_key(8, 0, 0, 2), aug, "clamped")
    assert int(bad_a.item()) == int(bad_p.item()) == 3
    with pytest.raises(_lib.RaindropHipError, match="RD_EINVAL"):
        _batch_gather_aug(ds, torch.from_numpy(clamped).to(DEV), outs, bad_a, _cell(aug), 2, W=2 * F - 1)
    with pytest.raises(ValueError, match="W = 2F"):
        feed.EpochFeed(feed.DeviceDataset(torch.zeros(3, 4, 5), torch.zeros(3, 4), None, torch.zeros(4), device=DEV), 2, 2,
                       augment=feed.Augment())


@pytest.mark.parametrize("T,B,W,dstat,skew", [(5, 3, 6, 0, 0), (70, 19, 8, 5, 0), (60, 32, 68, 6, 0), (60, 17, 68, 0, 1)])
def test_all_rates_zero_writes_the_plain_twins_bytes(T, B, W, dstat, skew):
    N, n = 23, 4
    P, tm = _dataset(T, N, W // 2, seed=T)
    ds, _, _ = _device_ds(P, tm, dstat, seed=T)
    plan = torch.from_numpy(np.random.default_rng(T).integers(0, N, (n, B))).to(DEV)
    cell0 = _cell(feed.Augment(seed=123), epoch=5)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    for cursor in (0, 2, n - 1, n):                                          # (n: outside the plan, clamped and counted by both)
        cur = torch.tensor([cursor, n], dtype=torch.int64, device=DEV)
        got_f, want_f, got_b, want_b = (_Outs(T, B, W, dstat, skew) for _ in range(4))
        o = got_f.t
        names = _logged(lambda: _lib.call(
            "rd_feed_gather_aug", T, B, W, ds.ds, ds.N, n, _p(ds.P), _p(ds.Ptime), _p(ds.Pstatic), _p(ds.y), _p(plan), _p(cur), _p(o["src"]),
            _p(o["times"]), _p(o["static"]), _p(o["y"]), _p(o["lengths"]), _p(bad), _p(cell0), _stream()))
        assert names == {"k_feed_gather_aug"}
        o = want_f.t
        names = _logged(lambda: _lib.call(
            "rd_feed_gather", T, B, W, ds.ds, ds.N, n, _p(ds.P), _p(ds.Ptime), _p(ds.Pstatic), _p(ds.y), _p(plan), _p(cur), _p(o["src"]),
            _p(o["times"]), _p(o["static"]), _p(o["y"]), _p(o["lengths"]), _p(bad), _stream()))
        assert names == {"k_feed_gather"}
        row = plan[min(cursor, n - 1)].contiguous()
        assert _logged(lambda: _batch_gather_aug(ds, row, got_b, bad, cell0, 17)) == {"k_batch_gather_aug"}
        assert _logged(lambda: _batch_gather(ds, row, want_b, bad)) == {"k_batch_gather"}
        torch.cuda.synchronize()
        assert got_f.same(want_f) and got_b.same(want_b) and got_f.same(want_b), cursor
        assert all(x.guards_intact() for x in (got_f, want_f, got_b, want_b)), cursor
        assert int(bad.item()) == (2 if cursor == n else 0)
        bad.zero_()
        assert cur.tolist() == [cursor, n]


# ---- the feed on a tiny model ----------------------------------------------------------------------------------------------------------
AUG = dict(p_time=0.3, p_sensor=0.2, p_obs=0.15, value_noise=0.05, seed=31)
CAP = 4


def _tiny_ds(N=40, seed=71):
    cfg = synth.make_config("TINY")
    data = synth.make_batch(cfg, N, seed=seed)
    y = np.random.default_rng(seed).integers(0, cfg["n_classes"], N)
    host = dict(P=data["src"].numpy(), tm=data["times"].numpy(), st=data["static"].numpy(), y=y)
    return cfg, feed.DeviceDataset(data["src"], data["times"], data["static"], torch.from_numpy(y), device=DEV), host


def _stepper(cfg, ds, B, fd, **step_kw):
    """(step, opt, out): the TINY model (parameter seed 21, no dropout: tests.helpers.build_ours), FlatAdam, and the buffers
    `ds.batch(idx, out=out)` fills, which are the step's batch"""
    from raindrop_amd import dp
    from raindrop_amd.optim import FlatAdam
    from raindrop_amd.step import TrainStep
    from tests.helpers import build_ours
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 21).train()
    assert m.dropout.p == 0.0
    named = dict(m.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)], n_buckets=2)
    opt = FlatAdam(flat.flatten_parameters(), lr=1e-3)
    out = ds.alloc(B)
    ds.batch(np.arange(B), out=out)
    batch = dict(src=out["P"], times=out["Ptime"], static=out["Pstatic"], y=out["y"], lengths=out["lengths"])
    step_kw.setdefault("autotune", False)
    return TrainStep(m, flat, batch, feed=fd, **step_kw), opt, out


def _ref_batch(host, idx, aug, epoch, cursor):
    a = feed.Augment(**aug) if isinstance(aug, dict) else aug
    src, times, lengths = R.augment(host["P"], host["tm"], idx, R.batch_key(a.seed, epoch, CAP, cursor), a.p_time, a.p_sensor, a.p_obs,
                                    a.noise_c)
    return dict(P=src, Ptime=times, lengths=lengths, Pstatic=host["st"][idx], y=host["y"][idx])


def _batch_is(step, ref):
    b = step.batch
    got = dict(P=b["src"], Ptime=b["times"], lengths=b["lengths"], Pstatic=b["static"], y=b["y"])
    return all(np.array_equal(got[k].cpu().numpy().view(np.int32 if got[k].dtype == torch.float32 else np.int64),
                              np.ascontiguousarray(ref[k]).view(np.int32 if ref[k].dtype == np.float32 else np.int64)) for k in ref)


FORMS = {"eager": (dict(use_graph=False), False), "graph": ({}, False), "full": ({}, True), "accumulate2": (dict(accumulate=2), True)}


@pytest.mark.parametrize("form", list(FORMS))
def test_fed_augmented_step_equals_hand_fed_restatement(form):
    """B draws its batches through rd_feed_gather_aug, A is handed the restatement's batches: after every step B's batch buffers hold
    the restatement at (epoch, cursor), and losses, history and parameters are bit-equal over two epochs (3 and 2 batches)."""
    step_kw, full = FORMS[form]
    cfg, ds, host = _tiny_ds()
    B = 8
    rng = np.random.default_rng(9)
    epochs = [[rng.integers(0, 40, B) for _ in range(nb)] for nb in (3, 2)]
    fd = feed.EpochFeed(ds, B, capacity=CAP, augment=feed.Augment(**AUG))
    a, opt_a, out_a = _stepper(cfg, ds, B, None, **step_kw)
    b, opt_b, _ = _stepper(cfg, ds, B, fd, **step_kw)
    try:
        if full:
            a.capture_full(opt_a)
            b.capture_full(opt_b)
        assert fd.cell.tolist() == [0, 0] and fd.augment_state() == dict(feed.Augment(**AUG).state(), epoch=0)
        k = step_kw.get("accumulate", 1)

        def one(step, opt, last):
            if full:
                return step.run_full(close_window=last).clone() if k > 1 else step.run_full().clone()
            loss = step.run().clone()
            opt.step()
            return loss

        for epoch, plan in enumerate(epochs):
            fd.load_epoch(plan)
            assert fd.augment_state()["epoch"] == epoch
            want_loss, got_loss = [], []
            for cursor, idx in enumerate(plan):
                last = cursor == len(plan) - 1
                ref = _ref_batch(host, idx, AUG, epoch, cursor)
                for key, t in out_a.items():
                    t.copy_(torch.from_numpy(np.ascontiguousarray(ref[key])))
                want_loss.append(one(a, opt_a, last))
                got_loss.append(one(b, opt_b, last))
                assert _batch_is(b, ref), (epoch, cursor)
            want = torch.stack(want_loss).cpu().numpy()
            print(form, "epoch", epoch, "losses", want.tolist())
            assert np.isfinite(want).all() and len(set(want.tolist())) == len(plan)
            assert np.array_equal(torch.stack(got_loss).cpu().numpy().view(np.int32), want.view(np.int32))
            assert np.array_equal(fd.history()[0].view(np.int32), want.view(np.int32))
            assert torch.equal(_bits(opt_a.param.data), _bits(opt_b.param.data))
            assert fd.remaining() == 0 and fd.bad_indices() == 0
        assert b.captures == (1 if full else 0)
        # the second epoch's masks were new ones: the same index rows at epoch 0 give another batch
        assert not R.same(tuple(_ref_batch(host, epochs[1][0], AUG, 0, 0)[q] for q in ("P", "Ptime", "lengths")),
                          tuple(_ref_batch(host, epochs[1][0], AUG, 1, 0)[q] for q in ("P", "Ptime", "lengths")))
    finally:
        a.close()
        b.close()


def test_capture_leaves_the_cursor_and_setters_need_no_capture():
    """constructing the step with the autotune's captures and timed replays, then capture_full: the first real replay draws
    (epoch 0, cursor 0); set_augment / set_epoch change what the SAME graph draws; a second load_epoch moves the epoch on"""
    cfg, ds, host = _tiny_ds(seed=72)
    B = 8
    fd = feed.EpochFeed(ds, B, capacity=CAP, augment=feed.Augment(**AUG))
    step, opt, _ = _stepper(cfg, ds, B, fd, autotune=True)
    try:
        step.capture_full(opt)
        graphs, captures = (step.graph, step.graph_full), step.captures
        plan = [np.arange(8), np.arange(8, 16), np.arange(16, 24), np.arange(24, 32)]
        fd.load_epoch(plan)
        step.run_full()
        assert _batch_is(step, _ref_batch(host, plan[0], AUG, 0, 0))
        fd.set_augment(p_sensor=0.5, value_noise=0.0)
        aug2 = dict(AUG, p_sensor=0.5, value_noise=0.0)
        step.run_full()
        assert _batch_is(step, _ref_batch(host, plan[1], aug2, 0, 1)) and not _batch_is(step, _ref_batch(host, plan[1], AUG, 0, 1))
        fd.set_epoch(6)
        step.run_full()
        assert _batch_is(step, _ref_batch(host, plan[2], aug2, 6, 2))
        assert fd.augment_state() == dict(feed.Augment(**aug2).state(), epoch=6)
        fd.load_epoch(plan[:1])                                                # the next epoch: 7
        step.run_full()
        assert _batch_is(step, _ref_batch(host, plan[0], aug2, 7, 0)) and not _batch_is(step, _ref_batch(host, plan[0], aug2, 6, 0))
        assert (step.graph, step.graph_full) == graphs and step.captures == captures
        # snapshot / restore: the cursor goes back, and the batch drawn again is the same one
        fd.load_epoch(plan)
        snap = fd.snapshot()
        step.run_full()
        first = {k: (None if v is None else v.clone()) for k, v in step.batch.items()}
        fd.restore(snap)
        fd._left = len(plan)
        step.run_full()
        assert all(v is None or torch.equal(_bits(v), _bits(step.batch[k])) for k, v in first.items())
        assert _batch_is(step, _ref_batch(host, plan[0], aug2, 8, 0))
        with pytest.raises(ValueError):
            fd.set_augment(p_time=1.0)
        with pytest.raises(ValueError):
            fd.set_augment(p_drop=0.1)
        with pytest.raises(_lib.RaindropHipError):
            feed.EpochFeed(ds, B, CAP).set_epoch(1)
    finally:
        step.close()


def test_plain_feed_allocates_nothing_and_launches_the_plain_gather():
    cfg, ds, _ = _tiny_ds(seed=73)
    fd = feed.EpochFeed(ds, 8, capacity=CAP)
    assert fd.augment is None and fd._aug is None and fd.augment_state() is None
    out = ds.alloc(8)
    batch = dict(src=out["P"], times=out["Ptime"], static=out["Pstatic"], y=out["y"], lengths=out["lengths"])
    fd.load_epoch([np.arange(8)])
    assert _logged(lambda: fd.enqueue_gather(batch)) == {"k_feed_gather"}
    fa = feed.EpochFeed(ds, 8, capacity=CAP, augment=feed.Augment(p_obs=0.1))
    fa.load_epoch([np.arange(8)])
    assert _logged(lambda: fa.enqueue_gather(batch)) == {"k_feed_gather_aug"}
    torch.cuda.synchronize()


def test_fit_with_augment():
    """two epochs on a TINY split: finite losses, another run than the plain one, validation untouched -- the recorded metrics of the
    best epoch are feed.validate's on the weights fit hands back -- and the datasets unchanged"""
    from raindrop_amd import trainer
    from tests.helpers import build_ours
    cfg = synth.make_config("TINY")

    def part(N, seed):
        data = synth.make_batch(cfg, N, seed=seed)
        y = (data["src"][:, :, 0].sum(0).numpy() > 0).astype(np.int64)
        if y.mean() > 0.5:
            y = 1 - y
        return feed.DeviceDataset(data["src"], data["times"], data["static"], torch.from_numpy(y), device=DEV)
    ds, vds = part(96, 81), part(48, 82)
    before = [t.clone() for t in (ds.P, ds.Ptime, vds.P, vds.Ptime)]

    def run(augment):
        np.random.seed(0)
        m = build_ours(cfg, synth.make_structure(cfg, "ones"), DEV, 3)
        return m, trainer.fit(m, ds, vds, 2, batch_size=16, strategy=2, lr=1e-3, scheduler=False, autotune=False, augment=augment)
    m, r = run(feed.Augment(p_sensor=0.2, p_obs=0.1))
    _, r0 = run(None)
    _, r1 = run(dict(p_sensor=0.2, p_obs=0.1))
    print("augmented", r["train_loss"], "plain", r0["train_loss"], "val_auroc", r["val_auroc"])
    assert len(r["train_loss"]) == 2 and np.isfinite(r["train_loss"]).all() and np.isfinite(r["val_loss"]).all()
    assert r["train_loss"] != r0["train_loss"] and r["train_loss"] == r1["train_loss"]
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(before, (ds.P, ds.Ptime, vds.P, vds.Ptime)))
    if r["best_epoch"] is not None:
        v = feed.validate(m, vds)
        e = r["best_epoch"]
        assert (v["auroc"], v["auprc"], v["loss"]) == (r["val_auroc"][e], r["val_auprc"][e], r["val_loss"][e])
        assert v["auroc"] == r["best_auroc"]
    with pytest.raises(ValueError, match="augment"):
        trainer.fit(m, ds, vds, 1, batch_size=16, augment=0.2)
