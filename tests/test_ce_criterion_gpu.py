"""GPU: class weights and label smoothing in the steps' cross entropy -- `rd_softmax_xent_crit`, `rd_head_train_crit` and the
`class_weight=` / `label_smoothing=` keywords of `TrainStep`, `BetaTrainStep`, `AutogradStep` and `feed.validate`.

The oracle is `torch.nn.functional.cross_entropy(l, y, weight=w, label_smoothing=eps)` in float64 on the CPU (operator and fused
head) or on the eager model's logits (steps).  Bounds are the ones the plain cross entropy's tests apply
(tests/test_gpu_parity.py::test_fused_head_against_float64, ::test_static_train_step_matches_autograd,
tests/test_beta_step_gpu.py::test_beta_step_matches_eager_model, tests/test_grad_clip_gpu.py's whole-step bound).  With the
neutral criterion (eps = 0, every weight 1) the new kernels are the plain ones bit for bit (loss: 2 ulps).  Every test prints the
figures it bounds before it asserts."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import restatement as O2
from raindrop_amd import _lib, dp, feed, synth
from tests.helpers import build_ours

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
HEAD_SHAPES = [(6, 5, 16, 4, 2, 2), (9, 37, 152, 34, 6, 2), (5, 3, 68, 0, 0, 8)]          # T, B, D, Fe, d_static, C


@pytest.fixture(params=["bf16x3", "fp32"])
def precision_mode(request):
    _lib.call("rd_set_precision", 1 if request.param == "bf16x3" else 0)
    yield request.param
    _lib.call("rd_set_precision", 1)


@pytest.fixture()
def exact_fp32():
    _lib.call("rd_set_precision", 0)
    try:
        yield
    finally:
        _lib.call("rd_set_precision", 1)


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _ulps(a, b):
    """distance of two finite fp32 values of equal sign in units in the last place"""
    ia, ib = (int(np.float32(float(v)).view(np.int32)) for v in (a, b))
    return abs(ia - ib)


def _crit(eps, w):
    return torch.tensor([eps] + [float(v) for v in w], dtype=torch.float32, device=DEV)


def _xent_crit(logits, y, crit):
    B, C = logits.shape
    loss, dl = torch.full((1,), 7.0, device=DEV), torch.full((B, C), 7.0, device=DEV)
    _lib.call("rd_softmax_xent_crit", B, C, P(logits), P(y), P(crit), P(loss), P(dl), None)
    torch.cuda.synchronize()
    return loss, dl


# ---- 1. the operator against torch in float64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,C,variant", [(1, 2, "plain"), (5, 2, "plain"), (64, 3, "plain"), (37, 8, "plain"), (300, 16, "plain"),
                                         (64, 3, "absent_class"), (37, 8, "zero_weight_present")])
def test_operator_against_float64(B, C, variant, eps):
    """loss within 1e-6 max(1, |ref|), dlogits within 2e-5 of the reference's max-norm; two launches give the same bits."""
    rng = np.random.default_rng(B * 100 + C)
    lg = torch.from_numpy((rng.standard_normal((B, C)) * 2).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, C - 1 if variant == "absent_class" else C, size=B)).long()
    w = torch.from_numpy(rng.uniform(0.2, 3.0, size=C).astype(np.float32))
    if variant == "zero_weight_present":
        w[int(y[0])] = 0.0
        assert bool((y != y[0]).any())
    if variant == "absent_class":
        assert not bool((y == C - 1).any())
    l64 = lg.double().requires_grad_(True)
    ref = F.cross_entropy(l64, y, weight=w.double(), label_smoothing=eps)
    dref, = torch.autograd.grad(ref, l64)
    crit = _crit(eps, w)
    loss, dl = _xent_crit(lg.to(DEV), y.to(DEV), crit)
    loss2, dl2 = _xent_crit(lg.to(DEV), y.to(DEV), crit)
    el, ed = abs(float(loss) - float(ref)), _rel(dl.cpu().numpy().astype(np.float64), dref.numpy())
    print("B %d C %d %s eps %g: loss %.8f ref %.8f (|d| %.2e), dlogits rel %.2e" % (B, C, variant, eps, float(loss), float(ref), el, ed))
    assert torch.equal(loss, loss2) and torch.equal(dl, dl2)
    assert el < 1e-6 * max(1.0, abs(float(ref)))
    assert ed <= 2e-5


def test_operator_all_weights_zero_is_nan_as_in_torch():
    lg = torch.randn(9, 3, generator=torch.Generator().manual_seed(3))
    y = torch.tensor([0, 1, 2] * 3)
    ref = F.cross_entropy(lg.double(), y, weight=torch.zeros(3, dtype=torch.float64), label_smoothing=0.1)
    loss, _ = _xent_crit(lg.to(DEV), y.to(DEV), _crit(0.1, [0, 0, 0]))
    assert bool(torch.isnan(ref)) and bool(torch.isnan(loss).all())


def test_operator_label_out_of_range_is_nan_and_reads_nothing():
    """one label equal to C: NaN loss (the label is counted nowhere and indexes no logit), and the process goes on"""
    B, C = 5, 4
    lg = torch.randn(B, C, generator=torch.Generator().manual_seed(4)).to(DEV)
    y = torch.tensor([0, 1, C, 3, 2], device=DEV)
    loss, dl = _xent_crit(lg, y, _crit(0.1, [1.0, 2.0, 0.5, 1.5]))
    assert bool(torch.isnan(loss).all())
    y[2] = 2
    loss, dl = _xent_crit(lg, y, _crit(0.1, [1.0, 2.0, 0.5, 1.5]))      # the process survived: the next launch is finite
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dl).all())


# ---- 2. / 3. the fused head ----------------------------------------------------------------------------------------------------
def _head_inputs(T, B, D, Fe, ds, C):
    """the construction of tests/test_gpu_parity.py::test_fused_head_against_float64"""
    rng = np.random.default_rng(T * 100 + B)
    f = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    dh = D + Fe
    r = f(T, B, D)
    lengths = torch.from_numpy(rng.integers(1, T + 1, size=B)).long()
    mask = torch.from_numpy(O2.padding_mask(lengths.numpy(), T))
    stat = f(B, ds) if Fe else None
    par = {"emb_w": f(Fe, ds) * 0.3 if Fe else None, "emb_b": f(Fe) * 0.1 if Fe else None, "w0": f(dh, dh) * 0.1, "b0": f(dh) * 0.1,
           "w2": f(C, dh) * 0.2, "b2": f(C) * 0.1}
    y = torch.from_numpy(rng.integers(0, C, size=B)).long()
    w = torch.from_numpy(rng.uniform(0.2, 3.0, size=C).astype(np.float32))
    return r, lengths, mask, stat, par, y, w


def _run_head(shape, inp, crit):
    """rd_head_train (crit None) or rd_head_train_crit on the padded layout -> loss, logits, dr, {gradients}"""
    T, B, D, Fe, ds, C = shape
    r, lengths, mask, stat, par, y, _ = inp
    lib = _lib.load()
    assert lib.rd_head_train_supported(D, Fe, C)
    dev = lambda t: None if t is None else t.to(DEV).contiguous()
    rd, md, ld, sd, yd = dev(r), dev(mask), dev(lengths), dev(stat), dev(y)
    pd = {k: dev(v) for k, v in par.items()}
    gd = {k: (None if v is None else torch.full_like(pd[k], 7.0)) for k, v in par.items()}
    loss = torch.zeros((), device=DEV); logits = torch.empty(B, C, device=DEV); dr = torch.full((T, B, D), 7.0, device=DEV)
    ws = torch.empty(lib.rd_head_train_workspace_bytes(B, D + Fe, C), dtype=torch.uint8, device=DEV)
    shp = _lib.shape(B, T, 1, 4)
    head = (shp, D, ds, Fe, C, P(rd), P(md), P(ld), P(sd), P(pd["emb_w"]), P(pd["emb_b"]), P(pd["w0"]), P(pd["b0"]), P(pd["w2"]),
            P(pd["b2"]), P(yd))
    tail = (P(loss), P(logits), P(gd["emb_w"]), P(gd["emb_b"]), P(gd["w0"]), P(gd["b0"]), P(gd["w2"]), P(gd["b2"]), P(dr), P(ws),
            ws.numel(), None)
    if crit is None:
        _lib.call("rd_head_train", *head, *tail)
    else:
        _lib.call("rd_head_train_crit", *head, P(crit), *tail)
    torch.cuda.synchronize()
    return loss, logits, dr, gd


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "T%d_B%d_D%d_Fe%d_C%d" % (s[0], s[1], s[2], s[3], s[5]))
def test_fused_head_crit_against_float64(shape):
    """rd_head_train_crit (eps 0.1, random positive weights; padded layout) against the same chain in float64 torch autograd: loss
    1e-6, logits, dr and the six gradients 2e-5 of max-norm; two launches give the same bits."""
    T, B, D, Fe, ds, C = shape
    inp = _head_inputs(*shape)
    r, lengths, mask, stat, par, y, w = inp
    r64 = r.double().requires_grad_(True)
    p64 = {k: (None if v is None else v.double().requires_grad_(True)) for k, v in par.items()}
    keep = (~mask).double().t().unsqueeze(-1)
    agg = (r64 * keep).sum(0) / (lengths.double() + 1).unsqueeze(-1)
    feat = torch.cat([agg, stat.double() @ p64["emb_w"].t() + p64["emb_b"]], 1) if Fe else agg
    logits64 = torch.relu(feat @ p64["w0"].t() + p64["b0"]) @ p64["w2"].t() + p64["b2"]
    loss64 = F.cross_entropy(logits64, y, weight=w.double(), label_smoothing=0.1)
    names = [k for k in ("emb_w", "emb_b", "w0", "b0", "w2", "b2") if par[k] is not None]
    gref = torch.autograd.grad(loss64, [r64] + [p64[k] for k in names])
    crit = _crit(0.1, w)
    loss, logits, dr, gd = _run_head(shape, inp, crit)
    loss2, _, dr2, gd2 = _run_head(shape, inp, crit)
    assert torch.equal(loss, loss2) and torch.equal(dr, dr2) and all(torch.equal(gd[k], gd2[k]) for k in names)
    print("loss %.8f ref %.8f" % (float(loss), float(loss64)))
    assert abs(float(loss) - float(loss64.detach())) < 1e-6 * max(1.0, abs(float(loss64.detach())))
    assert np.abs(logits.cpu().numpy() - logits64.detach().numpy()).max() < 2e-5 * np.abs(logits64.detach().numpy()).max()
    for name, got, ref in zip(["r"] + names, [dr] + [gd[k] for k in names], gref):
        a, b = got.cpu().numpy().astype(np.float64), ref.numpy()
        print(name, "%.2e" % (np.abs(a - b).max() / np.abs(b).max()))
        assert np.abs(a - b).max() <= 2e-5 * np.abs(b).max(), (name, float(np.abs(a - b).max() / np.abs(b).max()))


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "T%d_B%d_D%d_Fe%d_C%d" % (s[0], s[1], s[2], s[3], s[5]))
def test_neutral_criterion_is_the_plain_head(shape):
    """crit = [0, 1, .., 1]: logits, dr and the six gradients are rd_head_train's bit for bit, the loss within 2 fp32 ulps"""
    inp = _head_inputs(*shape)
    C = shape[5]
    loss0, logits0, dr0, g0 = _run_head(shape, inp, None)
    loss1, logits1, dr1, g1 = _run_head(shape, inp, _crit(0.0, [1.0] * C))
    print("loss %.9g | %.9g: %d ulps" % (float(loss0), float(loss1), _ulps(loss0, loss1)))
    assert torch.equal(logits0, logits1) and torch.equal(dr0, dr1)
    for k in g0:
        assert (g0[k] is None and g1[k] is None) or torch.equal(g0[k], g1[k]), k
    assert _ulps(loss0, loss1) <= 2


@pytest.mark.parametrize("B,C", [(1, 2), (5, 2), (64, 3), (37, 8), (300, 16)])
def test_neutral_criterion_is_the_plain_operator(B, C):
    rng = np.random.default_rng(B + C)
    lg = torch.from_numpy((rng.standard_normal((B, C)) * 2).astype(np.float32)).to(DEV)
    y = torch.from_numpy(rng.integers(0, C, size=B)).long().to(DEV)
    loss0, dl0 = torch.zeros(1, device=DEV), torch.zeros(B, C, device=DEV)
    _lib.call("rd_softmax_xent", B, C, P(lg), P(y), P(loss0), P(dl0), None)
    loss1, dl1 = _xent_crit(lg, y, _crit(0.0, [1.0] * C))
    assert torch.equal(dl0, dl1) and _ulps(loss0, loss1) <= 2


# ---- 4. TrainStep against autograd ---------------------------------------------------------------------------------------------
W2 = [0.6, 2.5]


def _p19(seed_model, seed_batch, B=8, **kw):
    cfg = synth.make_config("P19")
    gs = synth.make_structure(cfg, "sparse")
    dv = {k: (None if v is None else v.to(DEV).clone()) for k, v in synth.make_batch(cfg, B, seed=seed_batch).items()}
    m = build_ours(cfg, gs, DEV, seed_model, **kw).train()                     # dropout p forced to 0 by build_ours
    return cfg, m, dv


@pytest.mark.parametrize("use_graph,fused_head", [(False, True), (True, True), (True, False)])
def test_train_step_with_criterion_matches_autograd(use_graph, fused_head, precision_mode, monkeypatch):
    """tests/test_gpu_parity.py::test_static_train_step_matches_autograd with F.cross_entropy(weight=w, label_smoothing=0.1) on the
    eager model's logits as the reference, its tolerances, and two replays bit-equal."""
    from raindrop_amd.step import TrainStep
    monkeypatch.setenv("RD_HEAD_FUSED", "1" if fused_head else "0")
    tol = 5e-5 if (fused_head and precision_mode != "fp32") else 1e-5
    cfg, m, dv = _p19(7, 41)
    live = synth.live_parameter_names(cfg)
    named = dict(m.named_parameters())
    logits, _, _ = m(dv["src"], dv["static"], dv["times"], dv["lengths"])
    loss = F.cross_entropy(logits, dv["y"], weight=torch.tensor(W2, device=DEV), label_smoothing=0.1)
    ref = torch.autograd.grad(loss, [named[n] for n in live])
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in live])
    step = TrainStep(m, flat, dv, use_graph=use_graph, autotune=False, class_weight=W2, label_smoothing=0.1)
    try:
        l1 = step.run().clone()
        g1 = flat.flat.clone()
        l2 = step.run()
        torch.cuda.synchronize()
        assert step.head_fused == fused_head and step.crit is not None
        assert torch.equal(l1, l2) and torch.equal(g1, flat.flat)
        worst = max((_rel(named[n].grad.cpu().numpy(), g.cpu().numpy()), n) for n, g in zip(live, ref))
        print("loss %.8f ref %.8f, worst grad %.2e (%s), tol %g" % (float(l2), float(loss), worst[0], worst[1], tol))
        assert abs(float(l2) - float(loss)) < (1e-6 if tol == 1e-5 else 5e-6)
        for n, g in zip(live, ref):
            assert _rel(named[n].grad.cpu().numpy(), g.cpu().numpy()) < tol, n
    finally:
        step.close()


# ---- 5. set_criterion ----------------------------------------------------------------------------------------------------------
def test_set_criterion_changes_the_captured_step_without_a_new_capture():
    from raindrop_amd.step import TrainStep

    def make(**kw):
        cfg, m, dv = _p19(7, 41)
        named = dict(m.named_parameters())
        flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)])
        return TrainStep(m, flat, dv, use_graph=True, autotune=False, **kw), flat

    a, fa = make(class_weight=W2, label_smoothing=0.1)
    b, fb = make(class_weight=[1.5, 0.25], label_smoothing=0.3)
    plain, _ = make()
    try:
        graph = a.graph
        la0 = a.run().clone()
        a.set_criterion(class_weight=[1.5, 0.25], label_smoothing=0.3)
        la, lb = a.run(), b.run()
        torch.cuda.synchronize()
        print("loss before %.8f, after %.8f, fresh step %.8f" % (float(la0), float(la), float(lb)))
        assert a.graph is graph and a.graph_b is None
        assert not torch.equal(la0, la)
        assert torch.equal(la, lb) and torch.equal(fa.flat, fb.flat)
        with pytest.raises(ValueError):
            a.set_criterion(class_weight=[1.0, -1.0])
        with pytest.raises(_lib.RaindropHipError, match="plain mean cross entropy"):
            plain.set_criterion(class_weight=W2)
        assert plain.crit is None
    finally:
        a.close(); b.close(); plain.close()


# ---- 6. the whole step as one graph --------------------------------------------------------------------------------------------
def test_capture_full_with_criterion_follows_run_plus_flat_adam(exact_fp32):
    """capture_full(FlatAdam), 3 replays, against 3 x (run() + FlatAdam.step()) of an identically initialised model.  The plain-CE
    test of this pair (tests/test_grad_clip_gpu.py, tests/test_dp_gpu.py) bounds the parameters by 4e-7 max(1, |p|) -- the captured
    Adam's device-side bias corrections against the host's -- and the losses by 2e-6: the same bounds here."""
    from raindrop_amd.optim import FlatAdam
    from raindrop_amd.step import TrainStep

    def make():
        cfg, m, dv = _p19(21, 33)
        named = dict(m.named_parameters())
        flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)], n_buckets=2)
        opt = FlatAdam(flat.flatten_parameters(), lr=1e-3)
        return TrainStep(m, flat, dv, p_drop=0.0, autotune=False, split=False, class_weight=W2, label_smoothing=0.1), opt

    ts_r, opt_r = make()
    want = []
    try:
        for _ in range(3):
            loss = float(ts_r.run())
            opt_r.step()
            want.append((loss, opt_r.param.detach().clone()))
        torch.cuda.synchronize()
    finally:
        ts_r.close()
    ts_c, opt_c = make()
    try:
        ts_c.capture_full(opt_c)
        for s, (loss_r, pr) in enumerate(want):
            loss_c = float(ts_c.run_full())
            torch.cuda.synchronize()
            d, bound = float((opt_c.param.detach() - pr).abs().max()), 4e-7 * max(1.0, float(pr.abs().max()))
            print("step %d: loss %.7f | %.7f, max |dp| %.3g (bound %.3g)" % (s, loss_c, loss_r, d, bound))
            assert d <= bound and abs(loss_c - loss_r) <= 2e-6
        assert want[0][0] != want[2][0]
    finally:
        ts_c.close()


# ---- 7. BetaTrainStep, AutogradStep --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 0.05])
def test_beta_step_with_criterion_matches_eager_model(lam, precision_mode):
    """The smallest case of tests/test_beta_step_gpu.py::test_beta_step_matches_eager_model (P19, B = 8, captured, token plan) and
    its tolerances; reference: the eager use_beta model + torch's weighted, smoothed criterion + lambda * distance."""
    from raindrop_amd.step_beta import BetaTrainStep
    tol, ltol = (1e-5, 1e-6) if precision_mode == "fp32" else (5e-5, 5e-6)
    cfg, m, dv = _p19(7, 41, use_beta=True, compute_distance=True)
    named = dict(m.named_parameters())
    live = synth.live_parameter_names_beta(cfg)
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in live])
    step = BetaTrainStep(m, flat, dv, autotune=False, use_graph=True, token_plan=True, distance_weight=lam, class_weight=W2,
                         label_smoothing=0.1)
    try:
        assert step.head_fused and step.crit is not None
        logits, distance, _ = m(dv["src"], dv["static"], dv["times"], dv["lengths"])
        ce = F.cross_entropy(logits, dv["y"], weight=torch.tensor(W2, device=DEV), label_smoothing=0.1)
        ref = torch.autograd.grad(ce + lam * distance, [named[n] for n in live])
        l2 = step.run()
        torch.cuda.synchronize()
        worst = max((_rel(named[n].grad.cpu().numpy(), r.cpu().numpy()), n) for n, r in zip(live, ref))
        print("lambda %g: CE %.8f ref %.8f, distance %.6f, worst grad %.2e (%s)" % (lam, float(l2), float(ce), float(step.distance),
                                                                                  worst[0], worst[1]))
        assert abs(float(l2) - float(ce)) < ltol                              # step.loss stays the CE term
        assert _rel(step.logits.cpu().numpy(), logits.detach().cpu().numpy()) < tol
        assert abs(float(step.distance) - float(distance)) <= 1e-6 * float(distance)
        for n, r in zip(live, ref):
            assert _rel(named[n].grad.cpu().numpy(), r.cpu().numpy()) < tol, n
    finally:
        step.close()


@pytest.mark.parametrize("eps", [0.1, 0.0], ids=["weights_and_smoothing", "weights"])
def test_autograd_step_with_criterion_equals_its_eager_loop(eps):
    """AutogradStep(class_weight, label_smoothing): a replay equals its own loop body run eagerly bit for bit (dropout off).  Without
    smoothing that body is torch's F.cross_entropy(weight=w) itself; with smoothing it is `AutogradStep._criterion`'s capturable
    form of torch's weighted, smoothed criterion (torch's own call refuses stream capture), held to torch's value on the same
    logits within 1e-6 here and to 1e-12 in float64 by tests/test_ce_criterion_host.py."""
    from raindrop_amd.step import AutogradStep
    cfg, mg, dv = _p19(7, 41, use_beta=True, compute_distance=True)
    _, me, _ = _p19(7, 41, use_beta=True, compute_distance=True)
    me.graph_step = False
    st = AutogradStep(mg, dv, optimizer=False, class_weight=W2, label_smoothing=eps)
    loss_g = float(st.run())
    torch.cuda.synchronize()
    lg, _, _ = me(dv["src"], dv["static"], dv["times"], dv["lengths"])
    loss = st._criterion(lg, dv["y"])
    loss.backward()
    ref = F.cross_entropy(lg.detach(), dv["y"], weight=torch.tensor(W2, device=DEV), label_smoothing=eps)
    plain = float(F.cross_entropy(lg.detach(), dv["y"]))
    torch.cuda.synchronize()
    print("captured %.8f eager body %.8f torch's criterion %.8f (plain CE %.8f)" % (loss_g, float(loss), float(ref), plain))
    assert loss_g == float(loss) and loss_g != plain and torch.equal(st.logits, lg.detach())
    assert abs(float(loss) - float(ref)) <= (0.0 if eps == 0.0 else 1e-6 * max(1.0, abs(float(ref))))    # the loss bound of every test here
    ge = {n: p.grad for n, p in me.named_parameters() if p.grad is not None}
    gg = {n: p.grad for n, p in mg.named_parameters() if p.grad is not None}
    assert set(ge) == set(gg)
    for n in ge:
        assert torch.equal(ge[n], gg[n]), n
    st.close()


# ---- 8. validate ---------------------------------------------------------------------------------------------------------------
def test_validate_reports_the_criterion_s_loss_and_nothing_else_changes():
    cfg = synth.make_config("P19")
    val = synth.make_batch(cfg, 50, seed=90)
    y = np.random.default_rng(90).integers(0, 2, 50)
    ds = feed.DeviceDataset(val["src"], val["times"], val["static"], y, device=DEV)
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 5).eval()
    v0 = feed.validate(m, ds, chunk=64)
    v1 = feed.validate(m, ds, chunk=64, class_weight=W2, label_smoothing=0.1)
    scores = torch.sigmoid(feed.evaluate_captured(m, ds, 64)).contiguous()
    loss, _ = _xent_crit(scores, ds.y, _crit(0.1, W2))
    print("loss plain %.8f, criterion %.8f, operator %.8f" % (v0["loss"], v1["loss"], float(loss)))
    assert v1["loss"] == float(loss) and v1["loss"] != v0["loss"]
    assert set(v0) == set(v1)
    for k in v0:
        if k != "loss":
            assert np.array_equal(np.asarray(v0[k]), np.asarray(v1[k])), k
