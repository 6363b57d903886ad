"""GPU: coefficient dropout on the DEFAULT branch (code/Ob_propagation.py:195-196 with use_beta = False): the table launch, the
fused K1 kernels' COEF instantiations, the panel-product path, the eager model, TrainStep (padded layout, token plan, capture_full)
and the module graph.  The independent handle on the mask is the EXISTING batched operator: rows [l*B, (l+1)*B) of a 2B-row
ops.edge_softmax_list_batched(shared list, norm_row=1, p_drop=p_l, seed) are layer l's coefficient rows bit for bit.  Values and
gradients are compared with the composed operator path / a torch restatement run UNDER THAT TABLE.  Shapes: the smallest that reach
each code path -- P19's (34, 60) with B = 3 and lengths 2, 31, 60 (fused kernels, both instantiations), P12's (36, 215, B = 2) and
TINY (panel products), B = 8 for the steps (the recorded launch traces' batch)."""

import numpy as np
import pytest
import torch

from oracle import restatement as O2
from raindrop_amd import _lib, ops, synth
from tests.helpers import build_ours
from tests.test_gpu_parity import _rel, _rel2, precision_mode  # noqa: F401  (tests that take the fixture run in both arithmetic modes)

gpu = pytest.mark.gpu
DEV = "cuda"
P1, P2 = 0.3, 0.5
NAMES = ["R_u", "W1", "b1", "W2", "b2"]


def _graph(F, kind="sparse"):
    gs = torch.ones(F, F) if kind == "ones" else synth.make_structure(dict(d_inp=F), "sparse")
    adj, ei, ew = ops.graph_build(gs.to(DEV))
    _, ssum = ops.edge_softmax_dense(adj)
    return ei.contiguous(), ew.contiguous(), ssum


def _rows_of_existing_operator(ei, ew, F, B, p, seed, layer):
    """layer's rows of the 2B-row call of the existing batched operator (the issue's independent handle)"""
    w = ew.view(1, -1).expand(2 * B, -1).contiguous()
    _, s = ops.edge_softmax_list_batched(ei, w, F, norm_row=1, p_drop=p, seed=seed)
    return s[layer * B:(layer + 1) * B]


# ---- 1. the table ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,F", [(3, 5), (3, 34)])
def test_table_rows_are_the_existing_batched_operators(B, F):
    ei, ew, ssum = _graph(F)
    coef = ops.coef_table(ei, ew, ssum, B, P1, P2, 77)
    assert tuple(coef.shape) == (2, B, F)
    assert torch.equal(coef[0], _rows_of_existing_operator(ei, ew, F, B, P1, 77, 0))
    assert torch.equal(coef[1], _rows_of_existing_operator(ei, ew, F, B, P2, 77, 1))
    assert not torch.equal(coef[0][0], coef[0][1])                               # one decision per (sample, layer, edge)
    assert torch.equal(coef, ops.coef_table(ei, ew, ssum, B, P1, P2, 77)) and not torch.equal(coef, ops.coef_table(ei, ew, ssum, B, P1, P2, 78))
    half = ops.coef_table(ei, ew, ssum, B, P1, 0.0, 77)
    assert torch.equal(half[0], coef[0])
    assert torch.equal(half[1], ssum.view(1, F).expand(B, F))                    # p_l = 0: the plain ssum, bit for bit
    # the registered seed cell enters like at every other site
    cell = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    _lib.call("rd_set_seed_cell", ops._ptr(cell))
    try:
        moved = ops.coef_table(ei, ew, ssum, B, P1, P2, 72)
    finally:
        _lib.call("rd_set_seed_cell", None)
    assert torch.equal(moved, coef)


# ---- 2. the sensor stage against the composed operator path ------------------------------------------------------------------------------
def _stage_case(F, T, B, lengths=None):
    d, K = 4, T * 4
    rng = np.random.default_rng(F * 1000 + T * 10 + B)
    b = synth.make_batch(dict(d_inp=F, max_len=T, static=True, d_static=3, n_classes=2), B, seed=F + B, density=0.5)
    if lengths is not None:
        b["lengths"] = torch.tensor(lengths, dtype=torch.int64)
        live = (torch.arange(T)[:, None] < b["lengths"][None, :]).float()
        b["src"] = b["src"] * live[:, :, None]
    p = {n: synth.param_values("k1c." + n, s, seed=3) for n, s in zip(NAMES, [(1, F * d), (K, K), (K,), (K, K), (K,)])}
    p["R_u"] = p["R_u"] * 3.0
    dz = torch.from_numpy(rng.standard_normal((T, B, F * d + 16)).astype(np.float32)).to(DEV)
    return b, p, dz, _lib.shape(B, T, F, d)


def _stage(b, p, dz, shp, ei, ew, ssum, p_embed, seed):
    q = {n: t.detach().to(DEV).requires_grad_(True) for n, t in p.items()}
    z, mask = ops.sensor_stage(b["src"].to(DEV), b["times"].to(DEV), b["lengths"].to(DEV), ops.timescales(shp.T).to(DEV), ssum, q["R_u"],
                               q["W1"], q["b1"], q["W2"], q["b2"], shp, p_embed, seed, coef_p=(P1, P2), edges=(ei, ew))
    g = torch.autograd.grad(z, [q[n] for n in NAMES], dz)
    torch.cuda.synchronize()
    return z.detach(), mask, [x.detach() for x in g]


def _composed(b, p, dz, shp, coef, p_embed, seed):
    """ops.obs_embed -> ops.linear(act=1) -> a torch multiply by the table -> ops.linear(act=1) -> multiply -> ops.rows_to_tokens"""
    B, T, F, d = shp.B, shp.T, shp.F, shp.d_ob
    K = T * d
    q = {n: t.detach().to(DEV).requires_grad_(True) for n, t in p.items()}
    X = ops.obs_embed(b["src"].to(DEV), q["R_u"], shp, p_embed, seed).view(B * F, K)
    y1 = ops.linear(X, q["W1"], q["b1"], act=1).view(B, F, K) * coef[0][:, :, None]
    y2 = ops.linear(y1.reshape(B * F, K), q["W2"], q["b2"], act=1).view(B, F, K) * coef[1][:, :, None]
    zbuf = torch.zeros((T, B, F * d + 16), dtype=torch.float32, device=DEV)
    z = ops.rows_to_tokens(y2, None, zbuf, shp)
    g = torch.autograd.grad(z, [q[n] for n in NAMES], dz)
    torch.cuda.synchronize()
    return z.detach(), [x.detach() for x in g]


@gpu
@pytest.mark.parametrize("F,T,B,lengths,fused", [(34, 60, 3, (2, 31, 60), "1"), (34, 60, 3, (2, 31, 60), "0"), (36, 215, 2, None, "1"),
                                                 (5, 7, 3, None, "1")], ids=["P19", "P19_unfused", "P12", "TINY"])
def test_sensor_stage_with_table_matches_composed_operators(F, T, B, lengths, fused, precision_mode, monkeypatch):
    """Forward and all five gradients against the composed path under autograd in the same arithmetic mode, embedding dropout 0.2.
    Bounds: tests/test_gpu_parity.py::test_k1_fused_vs_generic_same_arithmetic's -- forward 5e-6 of the max-norm; per gradient at
    most 0.1 % of the entries beyond 2e-5 of its max-norm and a relative L2 error below 1e-3."""
    monkeypatch.setenv("RD_K1_FUSED", fused)
    ei, ew, ssum = _graph(F)
    b, p, dz, shp = _stage_case(F, T, B, lengths)
    seed = 9
    coef = ops.coef_table(ei, ew, ssum, B, P1, P2, seed)
    z, mask, g = _stage(b, p, dz, shp, ei, ew, ssum, 0.2, seed)
    zc, gc = _composed(b, p, dz, shp, coef, 0.2, seed)
    Fd = F * 4
    a, r = z[:, :, :Fd].cpu().numpy(), zc[:, :, :Fd].cpu().numpy()
    print("fwd %.2e" % (np.abs(a - r).max() / np.abs(r).max()))
    assert np.abs(a - r).max() <= 5e-6 * np.abs(r).max()
    for n, x, y in zip(NAMES, g, gc):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        scale = np.abs(y).max() + 1e-30
        bad = np.abs(x - y) > 2e-5 * scale
        print(n, "%.2e %.2e" % (float(np.abs(x - y).max() / scale), _rel2(x, y)))
        assert bad.mean() <= 1e-3, (n, float(bad.mean()), float(np.abs(x - y).max() / scale))
        assert _rel2(x, y) < 1e-3, (n, _rel2(x, y))
    # and the table matters: the plain stage (coef_p = (0, 0)) gives another z
    z0, _ = ops.sensor_stage(b["src"].to(DEV), b["times"].to(DEV), b["lengths"].to(DEV), ops.timescales(T).to(DEV), ssum,
                             *[p[n].to(DEV) for n in NAMES], shp, 0.2, seed)
    assert not torch.equal(z0, z) and torch.equal(z0[:, :, Fd:], z[:, :, Fd:])


@gpu
def test_specialised_coef_kernels_equal_runtime_shape_instantiation(precision_mode, monkeypatch):
    """RD_K1_SPECIALIZE=0: the <3,0,0> COEF instantiations give the <3,34,60> ones' output and gradients bit for bit."""
    if precision_mode != "bf16x3":
        pytest.skip("the fused path exists in split-bf16 mode only")
    ei, ew, ssum = _graph(34)
    b, p, dz, shp = _stage_case(34, 60, 3, (2, 31, 60))
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("RD_K1_SPECIALIZE", mode)
        res[mode] = _stage(b, p, dz, shp, ei, ew, ssum, 0.2, 9)
    assert torch.equal(res["1"][0], res["0"][0]) and torch.equal(res["1"][1], res["0"][1])
    for n, x, y in zip(NAMES, res["1"][2], res["0"][2]):
        assert torch.equal(x, y), n


# ---- 3. the model ----------------------------------------------------------------------------------------------------------------------
def _model(p1=P1, p2=P2, B=3):
    cfg = synth.make_config("P19")
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 7).train()     # the model's own dropout forced to 0 by build_ours
    m.graph_step = False
    m.ob_propagation.dropout, m.ob_propagation_layer2.dropout = p1, p2           # what upstream users set
    batch = synth.make_batch(cfg, B, seed=41)
    if B == 3:
        batch["lengths"] = torch.tensor([2, 31, 60], dtype=torch.int64)
    dv = {k: (None if v is None else v.to(DEV)) for k, v in batch.items()}
    return cfg, m, batch, dv


def _restated(p, cfg, b, s1, s2):
    """oracle/restatement.py's de-duplicated forward with the aggregate scale as a per-(sample, sensor) table per layer"""
    import torch.nn.functional as Fn
    Fs, d, T, B = cfg["d_inp"], cfg["d_ob"], b["src"].shape[0], b["src"].shape[1]
    K = T * d
    h = Fn.relu(torch.repeat_interleave(b["src"][:, :, :Fs], d, dim=-1) * p["R_u"])
    pe = O2.positional_encoding(b["times"], cfg["max_len"])
    mask = torch.from_numpy(O2.padding_mask(b["lengths"].numpy(), T))
    x = h.view(T, B, Fs, d).permute(1, 2, 0, 3).reshape(B, Fs, K)
    y1 = Fn.relu(Fn.linear(x, p["ob_propagation.lin_value.weight"], p["ob_propagation.lin_value.bias"])) * s1[:, :, None]
    y2 = Fn.relu(Fn.linear(y1, p["ob_propagation_layer2.lin_value.weight"], p["ob_propagation_layer2.lin_value.bias"])) * s2[:, :, None]
    r = torch.cat([y2.view(B, Fs, T, d).permute(2, 0, 1, 3).reshape(T, B, Fs * d), pe], dim=2)
    for i in range(cfg["nlayers"]):
        r = O2.encoder_layer(r, mask, p, "transformer_encoder.layers.%d." % i, cfg["nhead"])
    keep = (~mask).permute(1, 0).unsqueeze(2).to(r.dtype)
    agg = torch.sum(r * keep, dim=0) / (b["lengths"].unsqueeze(1) + 1)
    agg = torch.cat([agg, Fn.linear(b["static"], p["emb.weight"], p["emb.bias"])], dim=1)
    hid = Fn.relu(Fn.linear(agg, p["mlp_static.0.weight"], p["mlp_static.0.bias"]))
    return Fn.linear(hid, p["mlp_static.2.weight"], p["mlp_static.2.bias"])


@gpu
def test_model_training_forward_and_gradients_match_restatement_under_the_table(precision_mode):
    """DESIGN (c)'s model bounds: logits 1e-4; gradients 1e-3 of the max-norm in fp32 mode, 5e-3 relative L2 / 2e-2 max-norm in
    split-bf16."""
    cfg, m, batch, dv = _model()
    live = synth.live_parameter_names(cfg)
    named = dict(m.named_parameters())
    torch.manual_seed(5); m._drop_calls = 0
    logits, distance, _ = m(dv["src"], dv["static"], dv["times"], dv["lengths"])
    loss = torch.nn.functional.cross_entropy(logits, dv["y"])
    got = torch.autograd.grad(loss, [named[n] for n in live])
    g = m._graph(torch.device(DEV))
    coef = ops.coef_table(g["edge_index"], g["edge_weights"], g["ssum"], 3, P1, P2, m.forward_seed(1)).cpu()
    assert float(distance) == 0.0                                                # the returned structure does not see the masks
    p = {n: t.detach().cpu().clone().requires_grad_(n in live) for n, t in named.items()}
    ref_logits = _restated(p, cfg, batch, coef[0], coef[1])
    ref = torch.autograd.grad(torch.nn.functional.cross_entropy(ref_logits, batch["y"]), [p[n] for n in live])
    elog = float((logits.detach().cpu() - ref_logits.detach()).abs().max())
    print("logits %.2e" % elog)
    assert elog < 1e-4
    for n, a, r in zip(live, got, ref):
        a, r = a.cpu().numpy(), r.numpy()
        print(n, "%.2e %.2e" % (_rel(a, r), _rel2(a, r)))
        if precision_mode == "fp32":
            assert _rel(a, r) < 1e-3, (n, _rel(a, r))
        else:
            assert _rel2(a, r) < 5e-3 and _rel(a, r) < 2e-2, (n, _rel2(a, r), _rel(a, r))
    # the attributes matter in training mode ...
    m.ob_propagation.dropout = m.ob_propagation_layer2.dropout = 0.0
    plain = m(dv["src"], dv["static"], dv["times"], dv["lengths"])[0].detach()
    assert not torch.equal(plain, logits.detach())
    # ... and only there: model.eval() is bit-equal to the attributes at 0
    m.eval()
    with torch.no_grad():
        e0 = m(dv["src"], dv["static"], dv["times"], dv["lengths"])[0].clone()
        m.ob_propagation.dropout, m.ob_propagation_layer2.dropout = P1, P2
        e1 = m(dv["src"], dv["static"], dv["times"], dv["lengths"])[0].clone()
    assert torch.equal(e0, e1)


@gpu
def test_model_masks_follow_torch_seed_and_call_counter(precision_mode):
    cfg, m, batch, dv = _model()
    run = lambda: m(dv["src"], dv["static"], dv["times"], dv["lengths"])[0].detach().clone()
    torch.manual_seed(5); m._drop_calls = 0
    a = run()
    torch.manual_seed(5); m._drop_calls = 0
    b = run()
    c = run()                                                                    # the next call: another mask
    assert torch.equal(a, b) and not torch.equal(a, c)


# ---- 4. the steps ----------------------------------------------------------------------------------------------------------------------
def _train_step(m, cfg, dv, **kw):
    from raindrop_amd import dp
    from raindrop_amd.step import TrainStep
    named = dict(m.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)])
    kw.setdefault("autotune", False)
    return TrainStep(m, flat, dv, **kw), flat


@gpu
def test_train_step_matches_eager_model_on_both_layouts(precision_mode):
    """Bounds of tests/test_gpu_parity.py::test_static_train_step_matches_autograd (fused head): loss 1e-6 / gradients 1e-5 in fp32
    mode, 5e-6 / 5e-5 in split-bf16.  The step gets the seed the eager forward derives: step seed 0, seed cell = that seed - 1 (the
    step bumps the cell once before it draws).  Plan against padded layout: tests/test_token_plan_gpu.py's bound (loss 2e-6,
    gradients 2e-5 of the max-norm)."""
    tol, ltol = (1e-5, 1e-6) if precision_mode == "fp32" else (5e-5, 5e-6)
    cfg, m, batch, dv = _model(B=8)
    named = dict(m.named_parameters())
    live = synth.live_parameter_names(cfg)
    seed = m.forward_seed(m._drop_calls + 1)
    logits, _, _ = m(dv["src"], dv["static"], dv["times"], dv["lengths"])
    loss = torch.nn.functional.cross_entropy(logits, dv["y"])
    ref = [r.cpu().numpy() for r in torch.autograd.grad(loss, [named[n] for n in live])]
    per_layout = {}
    for token_plan in (False, True):
        step, flat = _train_step(m, cfg, dv, use_graph=False, token_plan=token_plan, seed=0)
        try:
            assert step.sensor.coef_p == (P1, P2) and step.sensor.edge_drop
            if token_plan and step.plan is None:
                assert precision_mode == "fp32"                                  # no token plan in the exact mode: the padded layout again
            step.seed_cell.fill_(seed - 1)
            l2 = float(step.run())
            torch.cuda.synchronize()
            grads = [named[n].grad.cpu().numpy().copy() for n in live]
        finally:
            step.close()
        worst = max((_rel(a, r), n) for n, a, r in zip(live, grads, ref))
        print("plan=%d loss %.2e worst grad %.2e (%s)" % (token_plan, abs(l2 - float(loss)), worst[0], worst[1]))
        assert abs(l2 - float(loss)) < ltol
        for n, a, r in zip(live, grads, ref):
            assert _rel(a, r) < tol, (token_plan, n, _rel(a, r))
        per_layout[token_plan] = (l2, grads)
    (la, ga), (lb, gb) = per_layout[True], per_layout[False]
    assert abs(la - lb) < 2e-6 * max(1.0, abs(lb))
    for n, a, r in zip(live, ga, gb):
        assert _rel(a, r) < 2e-5, (n, _rel(a, r))


@gpu
def test_capture_full_draws_fresh_coefficient_masks_with_model_dropout_off():
    """model.dropout.p = 0 and coefficient dropout 0.3: the seed cell must still advance per replay (two replays, two losses), and
    re-registering the same seed-cell value (with the parameters and the optimizer state restored) reproduces the first."""
    from raindrop_amd.optim import FlatAdam
    cfg, m, batch, dv = _model(P1, 0.0, B=8)
    assert float(m.dropout.p) == 0.0
    named = dict(m.named_parameters())
    from raindrop_amd import dp
    from raindrop_amd.step import TrainStep
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)])
    opt = FlatAdam(flat.flatten_parameters(), lr=0.0)                            # lr 0: the parameters stay, only the masks move
    step = TrainStep(m, flat, dv, autotune=False, seed=99, use_graph=False)
    try:
        step.capture_full(opt)
        step.seed_cell.fill_(17)
        a = float(step.run_full()); torch.cuda.synchronize()
        b = float(step.run_full()); torch.cuda.synchronize()
        step.seed_cell.fill_(17)
        c = float(step.run_full()); torch.cuda.synchronize()
    finally:
        step.close()
    assert a != b and a == c


@gpu
def test_module_graph_takes_the_dropping_path():
    """The captured module step against RD_MODULE_GRAPH=0 (model.graph_step = False) under the same masks, at the module-graph
    tests' bounds (tests/test_graph_module_gpu.py: logits 2e-5, loss 5e-6, gradients 5e-5 of the max-norm or 2e-3 relative L2)."""
    cfg, m, batch, dv = _model(B=8)
    live = synth.live_parameter_names(cfg)

    def loop_step(graph):
        m.graph_step = graph
        for p in m.parameters():
            p.grad = None
        logits, dist, _ = m(dv["src"], dv["static"], dv["times"], dv["lengths"])
        loss = torch.nn.functional.cross_entropy(logits, dv["y"])
        loss.backward()
        return logits.detach().clone(), float(loss), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    loop_step(True)                                                              # builds the runner
    (r,) = [v for v in m._graph_runners.values() if v is not False]
    assert r.step.sensor.edge_drop
    seed = m.forward_seed(m._drop_calls + 1)                                     # what the next EAGER forward draws under
    r.step.seed_cell.fill_(seed - 1 - r.step.seed)                               # the forward graph bumps the cell once
    lg_g, loss_g, g_g = loop_step(True)
    lg_e, loss_e, g_e = loop_step(False)
    m.ob_propagation.dropout = m.ob_propagation_layer2.dropout = 0.0
    lg_0, _, _ = loop_step(False)
    assert not torch.equal(lg_0, lg_e)                                           # the masks matter
    assert np.abs(lg_g.cpu().numpy() - lg_e.cpu().numpy()).max() < 2e-5
    assert abs(loss_g - loss_e) < 5e-6
    for n in live:
        a, b = g_g[n].cpu().numpy().astype(np.float64), g_e[n].cpu().numpy().astype(np.float64)
        assert _rel(a, b) < 5e-5 or _rel2(a, b) < 2e-3, (n, _rel(a, b), _rel2(a, b))
    loop_step(True)                                                              # attributes at 0: a runner of its own, no table launch
    live_runners = [v for v in m._graph_runners.values() if v is not False]
    assert len(live_runners) == 2 and sorted(v.step.sensor.edge_drop for v in live_runners) == [False, True]


# ---- 5. launch surface -----------------------------------------------------------------------------------------------------------------
@gpu
def test_launch_surface_without_dropout_is_the_recorded_one_and_with_it_adds_the_table():
    import importlib.util
    import json
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_step_launches", os.path.join(golden, "make_step_launches.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = json.load(open(os.path.join(golden, "step_launches.json")))
    from raindrop_amd.step import TrainStep

    def trace(cfg_name, p1, p2, **kw):
        cfg, B = gen.configs()[cfg_name]
        _lib.call("rd_set_precision", 1)
        with gen.recording() as rec:
            m, b = gen.make(cfg, B)
            m.ob_propagation.dropout, m.ob_propagation_layer2.dropout = p1, p2
            ts = TrainStep(m, gen.flat_of(m, cfg), b, use_graph=False, autotune=False, split=False, **kw)
            rec.mark("split=%d plan=%d head_fused=%d" % (ts.split, ts.plan is not None, ts.head_fused))
            ts.run(between=lambda: rec.mark("between"))
        torch.cuda.synchronize()
        return json.loads(json.dumps(rec.trace))
    for cfg_name, form, kw in (("p19", "run", {}), ("tiny", "run_padded", dict(token_plan=False))):
        assert trace(cfg_name, 0.0, 0.0, **kw) == want["%s/%s" % (cfg_name, form)]
        names0 = [row[0] for row in want["%s/%s" % (cfg_name, form)]]
        names1 = [row[0] for row in trace(cfg_name, P1, 0.0, **kw)]
        expect = []
        for n in names0:
            if n in ("rd_sensor_stage_fwd", "rd_sensor_stage_fwd_prepared"):
                expect += ["rd_msgpass_coef_table", n + "_coef"]
            else:
                expect.append("rd_msgpass_bwd_coef" if n == "rd_msgpass_bwd" else n)
        assert names1 == expect
