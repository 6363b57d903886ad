"""GPU: global-norm gradient clipping and the non-finite guard of FlatAdam (`max_grad_norm`; rd_grad_sumsq, rd_adam_step_clip,
rd_adam_step_clip_dev): the norm against float64, the clipped update against torch's clip_grad_norm_ + Adam, bit identity with
the plain kernels when nothing is clipped, skipped steps on inf / NaN gradients, a new threshold inside a captured graph, the whole
step as one hipGraph (clipped, and with a poisoned batch), and two data-parallel ranks."""
import math
import os
import socket
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_MID, N_BIG = 100003, 6_000_011              # odd (a short last float4); the big one is several rounds of workgroups


def _flat(n, seed=1, **kw):
    from raindrop_amd.optim import FlatAdam
    g_ = torch.Generator(device="cpu").manual_seed(seed)
    p = torch.nn.Parameter(torch.randn(n, generator=g_).to(DEV))
    p.grad = torch.zeros(n, device=DEV)
    return p, FlatAdam(p, lr=1e-3, **kw)


def _state(p, opt):
    return p.detach().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# ---- 1. the norm ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 1023, N_MID, N_BIG])
def test_norm_against_float64(n):
    """sqrt of the partial sums (added in index order, as the update launch adds them) against numpy float64 sqrt(sum(g**2)):
    relative error <= n * 2**-52, the worst case of a double accumulation of n exact squares in ANY order; two launches on the same
    data give the same bits; the update launch reports the same norm."""
    from raindrop_amd import _lib, ops
    lib = _lib.load()
    G = lib.rd_grad_sumsq_grid()
    rng = np.random.default_rng(n)
    g = rng.standard_normal(n).astype(np.float32) * np.float32(3.0)
    ref = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    gd = torch.from_numpy(g).to(DEV)
    parts = [torch.full((G,), -1.0, dtype=torch.float64, device=DEV) for _ in range(2)]       # every slot must be written
    for part in parts:
        _lib.call("rd_grad_sumsq", n, ops._ptr(gd), ops._ptr(part), G * 8, ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(parts[0].view(torch.int64), parts[1].view(torch.int64))
    total = 0.0
    for x in parts[0].cpu().tolist():
        total += x
    rel = abs(math.sqrt(total) - ref) / ref
    print("n %d: norm %.17g, float64 %.17g, relative error %.3g (bound %.3g)" % (n, math.sqrt(total), ref, rel, n * 2.0 ** -52))
    assert rel <= n * 2.0 ** -52
    p, opt = _flat(n, max_grad_norm=math.inf)
    p.grad.copy_(gd)
    opt.step()
    st = opt.grad_stats()
    assert abs(st["norm"] - ref) / ref <= n * 2.0 ** -52 and st["scale"] == 1.0 and st["skipped"] == 0 and st["clipped"] == 0


# ---- 2. the clipped update against torch ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_clipped_adam():
    """torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the CPU, 5 steps at n = 100003, lr 1e-3: {weight decay: parameters};
    gradient norms 32, 348, 664, 980, 1296 against max_norm 500: two steps pass unclipped, three are clipped."""
    rng = np.random.default_rng(1)
    p0 = rng.standard_normal(N_MID).astype(np.float32)
    grads = [rng.standard_normal(N_MID).astype(np.float32) * np.float32(0.1 + s) for s in range(5)]
    out = {}
    for wd in (0.0, 0.01):
        ref = torch.nn.Parameter(torch.from_numpy(p0.copy()))
        opt = torch.optim.Adam([ref], lr=1e-3, weight_decay=wd)
        for g in grads:
            ref.grad = torch.from_numpy(g.copy())
            torch.nn.utils.clip_grad_norm_([ref], 500.0)
            opt.step()
        out[wd] = ref.detach().numpy().copy()
    return p0, grads, out


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("form", ["step", "step_captured"])
def test_clipped_update_matches_torch(torch_clipped_adam, form, wd):
    """within 2e-6, the bound tests/test_gpu_parity.py holds rd_adam_step to against torch.optim.Adam"""
    from raindrop_amd.optim import FlatAdam
    p0, grads, want = torch_clipped_adam
    mine = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(DEV))
    mine.grad = torch.zeros(N_MID, device=DEV)
    opt = FlatAdam(mine, lr=1e-3, weight_decay=wd, max_grad_norm=500.0)
    if form == "step_captured":
        opt.sync_step_cell()
    scales = []
    for g in grads:
        mine.grad.copy_(torch.from_numpy(g).to(DEV))
        if form == "step":
            opt.step()
        else:
            opt.step_captured(); opt.note_replay()
        scales.append(opt.grad_stats()["scale"])
    st = opt.grad_stats()
    assert [s == 1.0 for s in scales] == [True, True, False, False, False] and st["clipped"] == 3 and st["skipped"] == 0, (scales, st)
    d = np.abs(mine.detach().cpu().numpy() - want[wd]).max()
    print(form, wd, "max |p - torch| = %.3g" % d)
    assert d < 2e-6


# ---- 3. nothing clipped: the plain kernels' bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [1e30, math.inf])
def test_no_clip_is_bit_identical_to_the_plain_update(max_norm):
    """three captured steps (and three host-state steps) with a threshold nothing reaches leave p, exp_avg, exp_avg_sq bit-equal to
    a FlatAdam without the keyword (weight decay on: the scale is applied before it is added)"""
    for form in ("step_captured", "step"):
        pa, a = _flat(N_MID, seed=3, weight_decay=0.01)
        pb, b = _flat(N_MID, seed=3, weight_decay=0.01, max_grad_norm=max_norm)
        a.sync_step_cell(); b.sync_step_cell()
        g_ = torch.Generator(device="cpu").manual_seed(4)
        for s in range(3):
            g = (torch.randn(N_MID, generator=g_) * (0.5 + s)).to(DEV)
            for p, o in ((pa, a), (pb, b)):
                p.grad.copy_(g)
                if form == "step":
                    o.step()
                else:
                    o.step_captured(); o.note_replay()
        torch.cuda.synchronize()
        assert _same_bits(_state(pa, a), _state(pb, b)), form
        assert b.grad_stats()["scale"] == 1.0 and b.grad_stats()["clipped"] == 0 and a.t == b.t == 3


# ---- 4. skipped steps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N_MID, N_BIG])
def test_non_finite_gradient_skips_the_step(n):
    """one inf, then one NaN in the gradient: p, m, v keep their bits, `skipped` counts, the step count advances on host and device
    alike; the next finite step updates every element.  (6 M elements: several rounds of workgroups -- none may store.)"""
    p, opt = _flat(n, seed=5, max_grad_norm=math.inf)
    opt.sync_step_cell()
    g_ = torch.Generator(device="cpu").manual_seed(6)
    good = torch.randn(n, generator=g_).to(DEV)
    p.grad.copy_(good)
    opt.step_captured(); opt.note_replay()                                   # moments are non-zero from here on
    for k, (bad, at) in enumerate([(math.inf, n - 1), (math.nan, n // 2), (-math.inf, 0)]):
        before = _state(p, opt)
        p.grad.copy_(good)
        p.grad[at] = bad
        opt.step_captured(); opt.note_replay()
        torch.cuda.synchronize()
        st = opt.grad_stats()
        assert _same_bits(before, _state(p, opt)), (bad, at)
        assert st["skipped"] == k + 1 and st["scale"] == 0.0 and not math.isfinite(st["norm"]) and st["clipped"] == 0
        assert opt.device_steps() == opt.t == k + 2
    before = _state(p, opt)
    p.grad.copy_(good)
    opt.step_captured(); opt.note_replay()
    torch.cuda.synchronize()
    after = _state(p, opt)
    assert all(bool((x != y).all()) for x, y in zip(before, after))
    assert all(bool(torch.isfinite(x).all()) for x in after)
    assert opt.grad_stats()["skipped"] == 3 and opt.device_steps() == opt.t == 5
    if n == N_MID:                                                           # the host-state form skips the same way
        before = _state(p, opt)
        p.grad[7] = math.nan
        opt.step()
        torch.cuda.synchronize()
        assert _same_bits(before, _state(p, opt)) and opt.grad_stats()["skipped"] == 4 and opt.t == 6


# ---- 5. a new threshold inside a captured graph -----------------------------------------------------------------------------------
def test_set_max_grad_norm_reaches_a_captured_graph():
    """step_captured() inside torch.cuda.graph; set_max_grad_norm between replays: the next replay clips at the new value without a
    new capture -- bit-equal to an optimizer that enqueues the same launches eagerly"""
    n = N_MID
    pa, a = _flat(n, seed=7, max_grad_norm=math.inf)
    pb, b = _flat(n, seed=7, max_grad_norm=math.inf)
    a.sync_step_cell(); b.sync_step_cell()
    g = torch.randn(n, generator=torch.Generator(device="cpu").manual_seed(8)).to(DEV)
    norm = float(g.double().norm())
    pa.grad.copy_(g); pb.grad.copy_(g)
    a.step_captured(); a.note_replay(); b.step_captured(); b.note_replay()   # outside the capture first: lazy loads
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a.step_captured()
    want = []
    for thr in (math.inf, norm / 4, norm * 2, norm / 10):
        a.set_max_grad_norm(thr); b.set_max_grad_norm(thr)
        graph.replay(); a.note_replay()
        b.step_captured(); b.note_replay()
        torch.cuda.synchronize()
        sa, sb = a.grad_stats(), b.grad_stats()
        assert sa == sb and _same_bits(_state(pa, a), _state(pb, b)), (thr, sa, sb)
        want.append(1.0 if thr > norm else thr / (norm + 1e-6))
        assert abs(sa["scale"] - want[-1]) <= 1e-12 * want[-1], (thr, sa, want[-1])
    assert a.grad_stats()["clipped"] == 2 and a.device_steps() == a.t == 5


# ---- 6. / 7. the whole step as one hipGraph ----------------------------------------------------------------------------------------
def _whole_step(opt_kw):
    """P19, B = 8, model dropout 0: (model, flat, batch buffers, TrainStep, FlatAdam)"""
    from raindrop_amd import dp, synth
    from raindrop_amd.optim import FlatAdam
    from raindrop_amd.step import TrainStep
    from tests.helpers import build_ours
    cfg = synth.make_config("P19")
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 21).train()
    named = dict(m.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)], n_buckets=2)
    opt = FlatAdam(flat.flatten_parameters(), lr=1e-3, **opt_kw)
    buf = {k: (None if v is None else v.to(DEV).clone()) for k, v in synth.make_batch(cfg, 8, seed=33).items()}
    ts = TrainStep(m, flat, buf, p_drop=0.0, autotune=False, split=False)
    return cfg, flat, buf, ts, opt


@pytest.fixture()
def exact_fp32():
    from raindrop_amd import _lib
    _lib.call("rd_set_precision", 0)
    try:
        yield
    finally:
        _lib.call("rd_set_precision", 1)


def _first_norm(ts, flat):
    ts.run()
    torch.cuda.synchronize()
    return float(flat.flat.double().norm())


def test_whole_step_graph_clips_like_clip_grad_norm_and_plain_adam(exact_fp32):
    """TrainStep.capture_full(FlatAdam(max_grad_norm=M)), M = half the first step's norm, four replays, against TrainStep.run() +
    torch's clip_grad_norm_ on the flat gradient (on the device) + plain FlatAdam.step(): parameters within 4e-7 * max(1, |p|)
    after every step, the bound of the captured Adam against the host-state one."""
    _, flat_r, _, ts_r, opt_r = _whole_step({})
    try:
        M = 0.5 * _first_norm(ts_r, flat_r)
        want = []
        for s in range(4):
            loss_r = float(ts_r.run())
            torch.nn.utils.clip_grad_norm_([opt_r.param], M)
            opt_r.step()
            want.append((loss_r, opt_r.param.detach().clone()))
        torch.cuda.synchronize()
    finally:
        ts_r.close()
    _, flat_c, _, ts_c, opt_c = _whole_step(dict(max_grad_norm=M))
    try:
        ts_c.capture_full(opt_c)
        for s, (loss_r, pr) in enumerate(want):
            loss_c = float(ts_c.run_full())
            torch.cuda.synchronize()
            d, bound = float((opt_c.param.detach() - pr).abs().max()), 4e-7 * max(1.0, float(pr.abs().max()))
            st = opt_c.grad_stats()
            print("step %d: loss %.7f | %.7f, norm %.6g scale %.6g, max |dp| %.3g (bound %.3g)" % (s, loss_c, loss_r, st["norm"], st["scale"], d, bound))
            assert d <= bound, (s, d, bound)
            assert abs(loss_c - loss_r) <= 2e-6
        st = opt_c.grad_stats()
        assert st["clipped"] >= 1 and st["skipped"] == 0 and opt_c.device_steps() == opt_c.t == 4
    finally:
        ts_c.close()


def test_whole_step_graph_skips_a_poisoned_replay(exact_fp32):
    """the same captured step; +inf in ONE live observation value of `src` (value half, t < length, observed) for one replay: every
    parameter and both moments keep their bits and `skipped` is 1; with the value restored the following replays are finite and
    move the weights."""
    cfg, flat_r, _, ts_r, _ = _whole_step({})
    M = 0.5 * _first_norm(ts_r, flat_r)
    ts_r.close()
    _, flat, buf, ts, opt = _whole_step(dict(max_grad_norm=M))
    try:
        ts.capture_full(opt)
        assert math.isfinite(float(ts.run_full()))                          # one good step: the moments are non-zero
        F = cfg["d_inp"]
        b = 0
        assert int(buf["lengths"][b]) > 1
        t = 1                                                               # t < length
        f = int(torch.nonzero(buf["src"][t, b, F:])[0])                     # an observed sensor at that step
        keep = buf["src"][t, b, f].clone()
        torch.cuda.synchronize()
        before = _state(opt.param, opt)
        buf["src"][t, b, f] = math.inf
        ts.run_full()
        torch.cuda.synchronize()
        st = opt.grad_stats()
        assert _same_bits(before, _state(opt.param, opt))
        assert st["skipped"] == 1 and not math.isfinite(st["norm"]) and opt.device_steps() == opt.t == 2
        buf["src"][t, b, f] = keep
        for _ in range(2):
            loss = float(ts.run_full())
            torch.cuda.synchronize()
            after = _state(opt.param, opt)
            assert math.isfinite(loss) and all(bool(torch.isfinite(x).all()) for x in after)
            assert bool((after[0] != before[0]).any()) and math.isfinite(opt.grad_stats()["norm"])
            before = after
        assert opt.grad_stats()["skipped"] == 1 and opt.device_steps() == opt.t == 4
    finally:
        ts.close()


# ---- 8. two data-parallel ranks --------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _dp_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from raindrop_amd import dp, synth
    from raindrop_amd.models_rd import Raindrop_v2
    from raindrop_amd.optim import FlatAdam
    from raindrop_amd.step import TrainStep
    dev = torch.device("cuda", 0)
    cfg = synth.make_config("P19")
    m = Raindrop_v2(cfg["d_inp"], cfg["d_model"], cfg["nhead"], cfg["nhid"], cfg["nlayers"], cfg["dropout"], cfg["max_len"],
                    cfg["d_static"], cfg["MAX"], 0.5, cfg["aggreg"], cfg["n_classes"], synth.make_structure(cfg, "sparse"),
                    sensor_wise_mask=False)
    synth.fill_params_(m, seed=21)
    m = m.to(dev).train()
    named = dict(m.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)], n_buckets=2)
    opt = FlatAdam(flat.flatten_parameters(), lr=1e-3, max_grad_norm=1e-3)           # far below any real gradient norm: every step clips
    full = synth.make_batch(cfg, 16, seed=33)
    b = {k: (None if v is None else v.to(dev)) for k, v in dp.shard_batch(full, rank, world).items()}
    ts = TrainStep(m, flat, b, p_drop=0.0, use_graph=False)
    norms = []
    for _ in range(2):
        ts.run()
        flat.allreduce()
        opt.step()
        st = opt.grad_stats()
        norms.append((struct.pack("<d", st["norm"]), st["scale"]))
    torch.cuda.synchronize()
    ret[rank] = (norms, opt.grad_stats(), flat.flat_param.detach().cpu().numpy().copy())
    ts.close()
    dist.destroy_process_group()


def test_two_ranks_clip_by_the_same_norm():
    """world_size 2 on one device (gloo), as tests/test_dp_gpu.py: the optimizer's launches follow the all-reduce, so the norm is the
    averaged gradient's -- the same BITS on both ranks -- and the replicas end with equal parameters"""
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ret = mp.Manager().dict()
    mp.spawn(_dp_worker, args=(world, port, ret), nprocs=world, join=True)
    (n0, s0, p0), (n1, s1, p1) = ret[0], ret[1]
    assert n0 == n1 and s0 == s1, (n0, n1)
    assert all(sc < 1.0 for _, sc in n0) and s0["clipped"] == 2 and s0["skipped"] == 0
    assert np.array_equal(p0, p1)
