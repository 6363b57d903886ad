"""Coefficient dropout on the use_beta branch (code/Ob_propagation.py:195-196): operator, graph kernels in both forms, layer 2's
batched softmax (forward only: the model refuses layer 2's dropout), the sensor stage and the captured steps.  RNG streams cannot
match torch's, so the semantics are pinned instead: the mask is read back from the outputs and compared with rd_graph_beta_keep's
bytes, and values / gradients are compared with the restatement (O2, CPU autograd) run UNDER THAT MASK.  Shapes: the smallest that
reach each code path -- (N=6, T=5, B=4), P19's (34, 60, 3) in the LDS form and in the workspace form (RD_BETA_LARGE=1), P12's
(36, 215, 2) for the backward's time chunks."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import restatement as O2
from raindrop_amd import _lib, ops, synth
from raindrop_amd.Ob_propagation import Observation_progation
from tests.test_gpu_parity import _rel, precision_mode  # noqa: F401  (as tests/test_beta_step_gpu.py: tests that take the fixture run in both arithmetic modes)

gpu = pytest.mark.gpu
DEV = "cuda"
P = 0.3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rd_graph_beta_fwd_dropout", "rd_graph_beta_bwd_dropout", "rd_graph_beta_keep", "rd_edge_softmax_list_batched_dropout",
               "rd_beta_stage_fwd_dropout", "rd_beta_stage_bwd_dropout"]


def _t(a):
    return torch.from_numpy(np.asarray(a)).to(DEV)


def _case(n, T, B, seed=5):
    """Operator + a sparse random structure (distinct scores: no pruning ties) + batched inputs, as
    tests/test_graph_beta_gpu.py::test_beta_operator_at_dataset_shapes builds them."""
    d, K = 4, T * 4
    op = Observation_progation(K, K, n_nodes=n, ob_dim=d, heads=1)
    synth.fill_params_(op, seed=seed)
    rng = np.random.default_rng(n * 1000 + T)
    adj = (rng.random((n, n)) < 0.3).astype(np.float32) * rng.uniform(0.5, 1.5, (n, n)).astype(np.float32)
    ei, ew = O2.build_graph(adj)
    c = dict(n=n, T=T, B=B, d=d, K=K, op=op, ei=np.asarray(ei), ew=np.asarray(ew),
             X=(rng.standard_normal((B, n, K)) * 0.5).astype(np.float32), PT=rng.standard_normal((B, T, 16)).astype(np.float32),
             R=rng.standard_normal((B, n, K)).astype(np.float32))
    c["Ra"] = rng.standard_normal((B, c["ei"].shape[1] // 2)).astype(np.float32)
    return c


def _vh(c, opd, X):
    B, n, K, T = c["B"], c["n"], c["K"], c["T"]
    V = ops.linear(X.reshape(B * n, K), opd.lin_value.weight, opd.lin_value.bias, act=1).view(B, n, K)
    H = ops.linear(X.reshape(B * n, K), opd.increase_dim.weight, opd.increase_dim.bias, exact=True).view(B, n, T * 32)
    return V, H


def _edge_ids(c, ei2):
    """input-list ids of the kept edges [B,Kk] (the structure has no duplicate edges)."""
    n = c["n"]
    table = np.full((n, n), -1, np.int64)
    table[c["ei"][0], c["ei"][1]] = np.arange(c["ei"].shape[1])
    e2 = ei2.cpu().numpy()
    ids = table[e2[:, 0], e2[:, 1]]
    assert (ids >= 0).all()
    return ids


def _coefficients(c, opd, p, seed):
    """The effective coefficient tensor C[b, s, g, t, ch] read from the outputs: one call per target node g with V = g's indicator."""
    B, n, K, T = c["B"], c["n"], c["K"], c["T"]
    _, H = _vh(c, opd, _t(c["X"]))
    C = torch.zeros((B, n, n, T, 4), device=DEV)
    ei2 = None
    for g in range(n):
        V = torch.zeros((B, n, K), device=DEV)
        V[:, g] = 1.0
        out, ei2, _ = ops.graph_beta(V, H.detach(), opd.map_weights.detach(), _t(c["PT"]), _t(c["ei"]), _t(c["ew"]).reshape(1, -1), 4,
                                     p_drop=p, seed=seed)
        C[:, :, g] = out.view(B, n, T, 4)
    return C, ei2


def _kept_view(c, C, ei2):
    """C on the kept edges, kept-list order: [B,Kk,T,4]"""
    e2 = ei2.cpu().numpy()
    return torch.stack([C[b, e2[b, 0], e2[b, 1]] for b in range(c["B"])]).cpu().numpy()


# ---- 1. the operator no longer refuses ---------------------------------------------------------------------------------------------
@gpu
def test_operator_use_beta_with_dropout_runs_and_follows_the_seed():
    c = _case(34, 60, 1)
    x, pt, ei, ew = _t(c["X"][0]), _t(c["PT"][0]), _t(c["ei"]), _t(c["ew"])
    op = Observation_progation(c["K"], c["K"], n_nodes=34, ob_dim=4, heads=1, dropout=P)
    synth.fill_params_(op, seed=5)
    op = op.to(DEV).train()

    def call():
        return op(x, p_t=pt, edge_index=ei, edge_weights=ew, use_beta=True, return_attention_weights=True)
    torch.manual_seed(5); op._drop_calls = 0
    y1, (e1, a1) = call()
    torch.manual_seed(5); op._drop_calls = 0
    y2, (e2, a2) = call()
    y3, _ = call()                                                              # the next call: another mask
    assert torch.equal(y1, y2) and torch.equal(e1, e2) and torch.equal(a1, a2)
    assert not torch.equal(y1, y3)
    op.eval()
    ye, (ee, ae) = call()
    op.train(); op.dropout = 0.0
    y0, (e0, a0) = call()
    plain = c["op"].to(DEV)                                                      # an operator that never heard of dropout
    yp, (ep, ap) = plain(x, p_t=pt, edge_index=ei, edge_weights=ew, use_beta=True, return_attention_weights=True)
    assert torch.equal(ye, yp) and torch.equal(y0, yp)                           # eval mode and p = 0: today's output, bit for bit
    assert not torch.equal(y1, yp)
    for e, a in ((e1, a1), (ee, ae), (e0, a0)):                                  # the pruned list and the scores do not see p
        assert torch.equal(e, ep) and torch.equal(a, ap)


# ---- 2. mask semantics, read from the outputs --------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,T,B", [(6, 5, 4), (34, 60, 3)])
def test_mask_semantics_read_from_the_outputs(n, T, B):
    c = _case(n, T, B)
    opd = c["op"].to(DEV)
    E = c["ei"].shape[1]
    C0, ei0 = _coefficients(c, opd, 0.0, 0)
    Cp, eip = _coefficients(c, opd, P, 77)
    assert torch.equal(ei0, eip)
    ids = _edge_ids(c, eip)
    k0, kp = _kept_view(c, C0, eip).astype(np.float64), _kept_view(c, Cp, eip).astype(np.float64)
    assert (k0 > 0).all()                                                        # softmax weights of a handful of edges: no underflow
    want = k0 / (1 - P)
    assert np.all((kp == 0) | (np.abs(kp - want) <= 1e-6 * want))
    off = torch.ones((B, n, n), dtype=torch.bool)                                # nothing outside the kept edges
    e2 = eip.cpu()
    for b in range(B):
        off[b, e2[b, 0], e2[b, 1]] = False
    assert float(Cp.cpu()[off].abs().max()) == 0.0
    keep = ops.graph_beta_keep(B, T, E, P, 77, DEV).cpu().numpy()                # [B,E,T,4], every edge of the input list
    keep_kept = np.stack([keep[b, ids[b]] for b in range(B)])
    assert np.array_equal(kp != 0, keep_kept != 0)
    cnt = keep_kept.size
    frac = float((kp != 0).mean())
    print("kept fraction %.5f of %d" % (frac, cnt))
    assert abs(frac - (1 - P)) <= 4 * np.sqrt(P * (1 - P) / cnt) + 2.0 ** -16
    nz = kp != 0
    assert not np.all(nz == nz[..., :1])                                         # four independent channels per (edge, step)
    for b in range(1, B):                                                        # samples draw their own masks: read from the outputs,
        both, i0, ib = np.intersect1d(ids[0], ids[b], return_indices=True)       # on the input edges kept in sample 0 AND in sample b
        assert both.size > 0 and not np.array_equal(nz[0][i0], nz[b][ib])
        assert not np.array_equal(keep[0], keep[b])
    Cq, _ = _coefficients(c, opd, P, 78)
    assert not torch.equal(Cq != 0, Cp != 0)                                     # another seed, another mask
    # a registered seed cell holding k gives the mask of seed + k
    cell = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    V, H = _vh(c, opd, _t(c["X"]))
    args = (V.detach(), H.detach(), opd.map_weights.detach(), _t(c["PT"]), _t(c["ei"]), _t(c["ew"]).reshape(1, -1), 4)
    want_y = ops.graph_beta(*args, p_drop=P, seed=77 + 5)[0]
    _lib.call("rd_set_seed_cell", ops._ptr(cell))
    try:
        got_y = ops.graph_beta(*args, p_drop=P, seed=77)[0]
        got_keep = ops.graph_beta_keep(B, T, E, P, 77, DEV)
    finally:
        _lib.call("rd_set_seed_cell", None)
    assert torch.equal(got_y, want_y) and not torch.equal(got_y, ops.graph_beta(*args, p_drop=P, seed=77)[0])
    assert torch.equal(got_keep, ops.graph_beta_keep(B, T, E, P, 77 + 5, DEV))


# ---- 3. values and gradients against O2 under the kernel's own mask ----------------------------------------------------------------
def _ours(c, opd, p, seed, with_alpha):
    X = _t(c["X"]).requires_grad_(True)
    V, H = _vh(c, opd, X)
    ewd = _t(c["ew"]).reshape(1, -1).clone().requires_grad_(True)
    Y, ei2, alpha = ops.graph_beta(V, H, opd.map_weights, _t(c["PT"]), _t(c["ei"]), ewd, 4, alpha_grad=with_alpha, p_drop=p, seed=seed)
    loss = (Y * _t(c["R"])).sum()
    if with_alpha:
        loss = loss + (alpha * _t(c["Ra"])).sum()
    grads = torch.autograd.grad(loss, [X, opd.lin_value.weight, opd.lin_value.bias, opd.increase_dim.weight, opd.increase_dim.bias,
                                       opd.map_weights, ewd])
    return Y.detach(), ei2, alpha.detach(), [g.detach() for g in grads]


def _o2_under_mask(c, keep_kept, p, with_alpha, monkeypatch):
    """O2.observation_propagation_beta per sample on the CPU, its edge_softmax result multiplied by keep / (1 - p) (kept-list order),
    with the stable argsort of the existing test.  Gradients of sum_b (y_b * R_b).sum() [+ (alpha_b * Ra_b).sum()]."""
    op = c["op"].cpu()
    params = [op.lin_value.weight, op.lin_value.bias, op.increase_dim.weight, op.increase_dim.bias, op.map_weights]
    pr = [q.detach().clone().requires_grad_(True) for q in params]
    X = torch.from_numpy(c["X"]).requires_grad_(True)
    ew = torch.from_numpy(c["ew"]).clone().requires_grad_(True)
    real_argsort, real_softmax = torch.argsort, O2.edge_softmax
    cur = {}
    monkeypatch.setattr(torch, "argsort", lambda t, *a, **k: real_argsort(t, *a, **dict(k, stable=True)))
    monkeypatch.setattr(O2, "edge_softmax", lambda g, index, n: real_softmax(g, index, n) * cur["scale"])
    ys, eis, loss = [], [], 0.0
    for b in range(c["B"]):
        cur["scale"] = torch.from_numpy(keep_kept[b].reshape(keep_kept.shape[1], -1).astype(np.float32)) / (1 - p)
        y, (ei_ref, a_ref) = O2.observation_propagation_beta(X[b], torch.from_numpy(c["PT"][b]), torch.from_numpy(c["ei"]), ew, *pr, 4)
        loss = loss + (y * torch.from_numpy(c["R"][b])).sum()
        if with_alpha:
            loss = loss + (a_ref.reshape(-1) * torch.from_numpy(c["Ra"][b])).sum()
        ys.append(y.detach()); eis.append(ei_ref)
    grads = torch.autograd.grad(loss, [X] + pr + [ew])
    monkeypatch.undo()
    return torch.stack(ys), torch.stack(eis), grads


@gpu
@pytest.mark.parametrize("n,T,B,large,with_alpha", [(6, 5, 4, False, False), (34, 60, 3, False, True), (36, 215, 2, False, False),
                                                    (34, 60, 3, True, True)],
                         ids=["tiny", "p19_alpha", "p12_chunks", "p19_workspace_alpha"])
def test_values_and_gradients_against_o2_under_the_kernels_mask(n, T, B, large, with_alpha, monkeypatch):
    """Bounds: those of test_beta_operator_at_dataset_shapes (p = 0) at the same shapes -- 2e-5 absolute on y, scaled by 1 / (1 - p)
    like the coefficients, and 5e-5 of the max-norm per gradient (x, lin_value, increase_dim, map_weights, and the edge weights'
    through ops.graph_beta); with_alpha adds the alpha cotangent, which the mask must not touch."""
    c = _case(n, T, B)
    opd = c["op"].to(DEV)
    if large:
        monkeypatch.setenv("RD_BETA_LARGE", "1")
    Y, ei2, alpha, grads = _ours(c, opd, P, 31, with_alpha)
    monkeypatch.delenv("RD_BETA_LARGE", raising=False)
    keep = ops.graph_beta_keep(B, T, c["ei"].shape[1], P, 31, DEV).cpu().numpy()
    ids = _edge_ids(c, ei2)
    keep_kept = np.stack([keep[b, ids[b]] for b in range(B)])                    # [B,Kk,T,4]
    y_ref, ei_ref, g_ref = _o2_under_mask(c, keep_kept, P, with_alpha, monkeypatch)
    assert np.array_equal(ei2.cpu().numpy(), ei_ref.numpy())
    dy = float((Y.cpu() - y_ref).abs().max())
    print("y %.2e" % dy)
    assert dy < 2e-5 / (1 - P)
    for name, got, ref in zip(["x", "Wv", "bv", "Wi", "bi", "map", "ew"], grads, g_ref):
        r = ref.numpy().reshape(got.shape)
        rel = float(np.abs(got.cpu().numpy() - r).max() / np.abs(r).max())
        print(name, "%.2e" % rel)
        assert np.abs(got.cpu().numpy() - r).max() <= 5e-5 * np.abs(r).max() + 1e-9, (name, rel)


# ---- 4. the two forms agree ----------------------------------------------------------------------------------------------------------
@gpu
def test_workspace_form_equals_lds_form_with_dropout(monkeypatch):
    """Bounds of tests/test_graph_beta_gpu.py::test_workspace_form_equals_lds_form; the masks are the same bits."""
    c = _case(34, 60, 3)
    opd = c["op"].to(DEV)
    Ys, es, als, gs = _ours(c, opd, P, 13, True)
    Cs, _ = _coefficients(c, opd, P, 13)
    monkeypatch.setenv("RD_BETA_LARGE", "1")
    assert _lib.load().rd_graph_beta_workspace_bytes(3, 34, 240, 60, c["ei"].shape[1]) > 0
    Yl, el, all_, gl = _ours(c, opd, P, 13, True)
    Cl, _ = _coefficients(c, opd, P, 13)
    monkeypatch.delenv("RD_BETA_LARGE", raising=False)
    assert torch.equal(es, el)
    assert torch.equal(Cs != 0, Cl != 0)                                         # bit-equal masks
    assert float((als - all_).abs().max()) <= 1e-7
    assert float((Ys - Yl).abs().max()) <= 2e-6 * float(Ys.abs().max())
    for name, a, b in zip(["X", "Wv", "bv", "Wi", "bi", "map", "ew"], gs, gl):
        assert float((a - b).abs().max()) <= 5e-6 * float(a.abs().max()) + 1e-9, name
    Y2, _, _, g2 = _ours(c, opd, P, 13, True)                                    # fixed order, no atomics: the same bits again
    assert torch.equal(Y2, Ys) and all(torch.equal(a, b) for a, b in zip(g2, gs))


@gpu
def test_rounds_2_to_5_kernels_refuse_dropout(monkeypatch):
    c = _case(6, 5, 4)
    opd = c["op"].to(DEV)
    V, H = _vh(c, opd, _t(c["X"]))
    args = (V.detach(), H.detach(), opd.map_weights.detach(), _t(c["PT"]), _t(c["ei"]), _t(c["ew"]).reshape(1, -1), 4)
    monkeypatch.setenv("RD_BETA_V1", "1")
    ops.graph_beta(*args)                                                        # p = 0 runs
    with pytest.raises(_lib.RaindropHipError, match="RD_EUNSUPPORTED"):
        ops.graph_beta(*args, p_drop=P, seed=1)


# ---- 5. layer 2: the batched per-target softmax --------------------------------------------------------------------------------------
@gpu
def test_batched_edge_softmax_coefficient_dropout():
    """tests/test_gpu_parity.py::test_edge_coefficient_dropout_of_the_operator's check, batched over per-sample edge lists."""
    rng = np.random.default_rng(3)
    B, n, E = 3, 34, 217
    ei = torch.from_numpy(rng.integers(0, n, (B, 2, E))).to(DEV)
    w = torch.from_numpy(rng.standard_normal((B, E)).astype(np.float32)).to(DEV)
    g0, s0 = ops.edge_softmax_list_batched(ei, w, n, norm_row=1)
    g1, s1 = ops.edge_softmax_list_batched(ei, w, n, norm_row=1, p_drop=P, seed=11)
    g2, s2 = ops.edge_softmax_list_batched(ei, w, n, norm_row=1, p_drop=P, seed=11)
    g3, _ = ops.edge_softmax_list_batched(ei, w, n, norm_row=1, p_drop=P, seed=12)
    assert torch.equal(g1, g2) and torch.equal(s1, s2) and not torch.equal(g1, g3)
    kept = g1 != 0
    assert abs(float(kept.float().mean()) - (1 - P)) <= 4 * np.sqrt(P * (1 - P) / (B * E)) + 2.0 ** -16
    assert float((g1[kept] - g0[kept] / (1 - P)).abs().max()) < 1e-6
    assert not torch.equal(kept[0], kept[1])                                     # per-sample masks
    for b in range(B):
        ref_sum = torch.zeros(n, device=DEV).index_add_(0, ei[b, 1], g1[b])
        assert float((s1[b] - ref_sum).abs().max()) < 1e-5
    e1, t1 = ops.edge_softmax_list(ei[0], w[0], n, norm_row=1, p_drop=P, seed=11)   # sample 0 = the one-graph entry point's mask
    assert torch.equal(e1, g1[0]) and torch.equal(t1, s1[0])


# ---- 6. stage and steps (P19 configuration, B = 8, model dropout 0: only the edge masks move) ----------------------------------------
def _model(edge_p=P, **kw):
    from tests.helpers import build_ours
    cfg = synth.make_config("P19")
    gs = synth.make_structure(cfg, "sparse")
    m = build_ours(cfg, gs, DEV, 7, use_beta=True, **kw).train()
    m.dropout.p = 0.0
    m.ob_propagation.dropout = edge_p                                            # layer 1's operator; layer 2's is refused (below)
    return cfg, m


def _batch(cfg, seed=43):
    return {k: (None if v is None else v.to(DEV)) for k, v in synth.make_batch(cfg, 8, seed=seed).items()}


def _beta_step(m, cfg, dv, **kw):
    from raindrop_amd import dp
    from raindrop_amd.step_beta import BetaTrainStep
    named = dict(m.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names_beta(cfg)])
    kw.setdefault("autotune", False)
    return BetaTrainStep(m, flat, dv, p_drop=0.0, **kw), flat


@gpu
@pytest.mark.parametrize("token_plan", [True, False], ids=["plan", "padded"])
def test_beta_step_edge_dropout_graph_equals_enqueued_body(token_plan, precision_mode):
    """tests/test_beta_step_gpu.py::test_beta_step_dropout_graph_equals_enqueued_body with the operators' dropout instead of the
    model's: a replay equals the hand-enqueued body bit for bit at equal seed-cell values, two replays differ, a rewound cell
    repeats the bits (so the backward regenerated the forward's masks)."""
    out = []
    for use_graph in (True, False):
        cfg, m = _model(compute_distance=True)
        step, flat = _beta_step(m, cfg, _batch(cfg), use_graph=use_graph, seed=99, token_plan=token_plan)
        try:
            assert step.sensor.pe1 == P
            step.seed_cell.zero_()
            l1 = float(step.run()); torch.cuda.synchronize(); g1 = flat.flat.clone(); a1 = step.alpha.clone()
            l2 = float(step.run()); torch.cuda.synchronize(); g2 = flat.flat.clone()
            step.seed_cell.zero_()
            l3 = float(step.run()); torch.cuda.synchronize(); g3 = flat.flat.clone(); a3 = step.alpha.clone()
            out.append((l1, g1, l2, g2))
            assert l1 != l2 and not torch.equal(g1, g2)
            assert l1 == l3 and torch.equal(g1, g3)
            assert torch.equal(a1, a3)
        finally:
            step.close()
    (a1, ga1, a2, ga2), (b1, gb1, b2, gb2) = out
    assert a1 == b1 and a2 == b2
    assert torch.equal(ga1, gb1) and torch.equal(ga2, gb2)


@gpu
@pytest.mark.parametrize("use_graph,token_plan", [(True, True), (False, True), (True, False)], ids=["graph", "enqueued", "graph_padded"])
def test_beta_step_with_edge_dropout_matches_eager_model(use_graph, token_plan, precision_mode):
    """Bounds of tests/test_beta_step_gpu.py::test_beta_step_matches_eager_model.  The step gets the seed the eager forward derives
    (Raindrop_v2.forward_seed): step seed 0, seed cell = that seed - 1 (the step bumps the cell once before it draws)."""
    tol, ltol = (1e-5, 1e-6) if precision_mode == "fp32" else (5e-5, 5e-6)
    cfg, m = _model(compute_distance=True)
    named = dict(m.named_parameters())
    live = synth.live_parameter_names_beta(cfg)
    dv = _batch(cfg, 41)
    step, flat = _beta_step(m, cfg, dv, use_graph=use_graph, token_plan=token_plan, seed=0)
    try:
        for _ in range(2):
            seed = m.forward_seed(m._drop_calls + 1)
            logits, distance, _x = m(dv["src"], dv["static"], dv["times"], dv["lengths"])
            loss = torch.nn.functional.cross_entropy(logits, dv["y"])
            ref = torch.autograd.grad(loss, [named[n] for n in live])
            step.seed_cell.fill_(seed - 1)
            l2 = step.run()
            torch.cuda.synchronize()
            worst = max((_rel(named[n].grad.cpu().numpy(), r.cpu().numpy()), n) for n, r in zip(live, ref))
            print("loss %.2e logits %.2e worst grad %.2e (%s)" % (abs(float(l2) - float(loss)), _rel(step.logits.cpu().numpy(),
                  logits.detach().cpu().numpy()), worst[0], worst[1]))
            assert abs(float(l2) - float(loss)) < ltol
            assert _rel(step.logits.cpu().numpy(), logits.detach().cpu().numpy()) < tol
            for n, r in zip(live, ref):
                assert _rel(named[n].grad.cpu().numpy(), r.cpu().numpy()) < tol, n
        # and the masks matter: with the operators' dropout at 0 the eager loss is another one
        m.ob_propagation.dropout = 0.0
        plain = torch.nn.functional.cross_entropy(m(dv["src"], dv["static"], dv["times"], dv["lengths"])[0], dv["y"])
        assert float(plain) != float(loss)
    finally:
        step.close()


@gpu
def test_autograd_step_replays_draw_fresh_edge_masks():
    from raindrop_amd.step import AutogradStep
    cfg, m = _model()
    step = AutogradStep(m, _batch(cfg), optimizer=False)
    try:
        a = float(step.run()); torch.cuda.synchronize()
        b = float(step.run()); torch.cuda.synchronize()
        assert a != b                                                            # no optimizer, model dropout 0: only the edge masks moved
    finally:
        step.close()
    cfg, m = _model(edge_p=0.0)
    step = AutogradStep(m, _batch(cfg), optimizer=False)
    try:
        a = float(step.run()); torch.cuda.synchronize()
        b = float(step.run()); torch.cuda.synchronize()
        assert a == b
    finally:
        step.close()


@gpu
def test_evaluation_never_drops():
    from raindrop_amd.evalstep import EvalStep
    cfg, m = _model()
    m.ob_propagation_layer2.dropout = P                                          # (refused in training mode; evaluation ignores it)
    dv = _batch(cfg)
    ev = {k: v for k, v in dv.items() if k != "y"}
    m.eval()
    with torch.no_grad():
        la = m(dv["src"], dv["static"], dv["times"], dv["lengths"])[0].clone()
    step = EvalStep(m, ev)
    sa = step.run().clone(); torch.cuda.synchronize()
    step.close()
    m.ob_propagation.dropout = m.ob_propagation_layer2.dropout = 0.0
    with torch.no_grad():
        lb = m(dv["src"], dv["static"], dv["times"], dv["lengths"])[0].clone()
    step = EvalStep(m, ev)
    sb = step.run().clone(); torch.cuda.synchronize()
    step.close()
    assert torch.equal(la, lb) and torch.equal(sa, sb)
    m.train(); m.ob_propagation.dropout = P                                      # (training mode does drop)
    assert not torch.equal(m(dv["src"], dv["static"], dv["times"], dv["lengths"])[0].detach(), la)


@gpu
def test_layer2_coefficient_dropout_is_refused_in_training_mode():
    """With ob_propagation_layer2.dropout > 0 layer 2's coefficient sum is no longer 1 per target and the edge scores get a gradient
    through it, which is not built: the eager model, AutogradStep and BetaTrainStep refuse instead of training on an incomplete
    gradient."""
    from raindrop_amd.step import AutogradStep
    cfg, m = _model()
    m.ob_propagation_layer2.dropout = P
    dv = _batch(cfg)
    with pytest.raises(_lib.RaindropHipError, match="RD_EUNSUPPORTED"):
        m(dv["src"], dv["static"], dv["times"], dv["lengths"])
    with pytest.raises(_lib.RaindropHipError, match="RD_EUNSUPPORTED"):
        AutogradStep(m, dv, optimizer=False)
    with pytest.raises(_lib.RaindropHipError, match="RD_EUNSUPPORTED"):
        _beta_step(m, cfg, dv)


@gpu
def test_capture_full_step_draws_the_plain_steps_edge_masks():
    """BetaTrainStep.capture_full(FlatAdam) -- the whole step as one graph -- with edge dropout: at equal seed-cell values its first
    replay gives the loss and the gradients of the plain step's run(), bit for bit, and a rewound cell with restored parameters
    repeats them."""
    from raindrop_amd.optim import FlatAdam
    res = []
    for full in (False, True):
        cfg, m = _model(compute_distance=True)
        from raindrop_amd import dp
        from raindrop_amd.step_beta import BetaTrainStep
        named = dict(m.named_parameters())
        flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names_beta(cfg)])
        opt = FlatAdam(flat.flatten_parameters(), lr=1e-4) if full else None
        step = BetaTrainStep(m, flat, _batch(cfg), p_drop=0.0, autotune=False, seed=99)
        try:
            if full:
                step.capture_full(opt)
            step.seed_cell.zero_()
            loss = float(step.run_full() if full else step.run()); torch.cuda.synchronize()
            res.append((loss, flat.flat.clone()))
        finally:
            step.close()
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])


# ---- 7. host only: the new symbols in the header, the ctypes table and the exports ---------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    import subprocess
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "raindrop_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rd_[a-z0-9_]+)\s*\(", text))
    if not os.path.exists(_lib.LIB_PATH):
        from raindrop_amd import build
        build.build(verbose=False)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
