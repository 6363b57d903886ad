"""GPU: `BetaTrainStep` (raindrop_amd/step_beta.py) -- the hand-enqueued training step of Raindrop_v2(use_beta=True) -- and the two
layout kernels of its sensor stage (raindrop_amd/csrc/rd_beta_stage.hip).

Against the reference's own outputs (the BETA_CASES fixtures and their `_distance` companions, bounds of
tests/test_gpu_parity.py::test_model_use_beta_vs_golden and tests/test_distance_grad_gpu.py), against the kernels the new ones
replace (bit for bit), against the eager model (bounds of test_static_train_step_matches_autograd), under dropout (graph replay ==
hand-enqueued body, bit for bit), as a whole step with FlatAdam (fp32 bounds of tests/test_trajectory_gpu.py), on two ranks (bound of
tests/test_dp_gpu.py), and its refusals.  Every test prints the figures it bounds before it asserts."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from raindrop_amd import _lib, dp, ops, synth
from tests.helpers import BETA_CASES, build_ours, case_inputs, golden_grad, load_golden
from tests.test_gpu_parity import _grad_close, _rel, precision_mode  # noqa: F401  (tests that take it run in both arithmetic modes)

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXTRA = ["ob_propagation.increase_dim.weight", "ob_propagation.increase_dim.bias", "ob_propagation.map_weights"]


def _to_dev(batch):
    return {k: (None if v is None else v.to(DEV)) for k, v in batch.items()}


def _flat(m, cfg, **kw):
    named = dict(m.named_parameters())
    return dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names_beta(cfg)], **kw)


def _step(m, cfg, dv, **kw):
    from raindrop_amd.step_beta import BetaTrainStep
    kw.setdefault("autotune", False)
    flat = _flat(m, cfg)
    return BetaTrainStep(m, flat, dv, **kw), flat


# ---- 1. against the reference's outputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("token_plan", [True, False], ids=["plan", "padded"])
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "enqueued"])
@pytest.mark.parametrize("name", BETA_CASES)
def test_beta_step_vs_golden(name, use_graph, token_plan, precision_mode):
    """Bounds of test_model_use_beta_vs_golden: logits 1e-4, loss 1e-5, distance 1e-5 relative, gradients through _grad_close(1e-3)
    and the recorded norms; the parameters with a non-zero gradient are exactly `live`.  (The token plan exists in the bf16 modes
    only: in fp32 mode both settings run the padded layout.)"""
    g, meta = load_golden(name)
    cfg, gs, batch = case_inputs(meta)
    m = build_ours(cfg, gs, DEV, meta["param_seed"], use_beta=True, compute_distance=True).train()
    step, flat = _step(m, cfg, _to_dev(batch), use_graph=use_graph, token_plan=token_plan)
    try:
        assert (step.plan is not None) == bool(token_plan and step.head_fused and step._plan_supported())
        loss = step.run()
        torch.cuda.synchronize()
        dlog = np.abs(step.logits.cpu().numpy() - g["logits"]).max()
        print(name, "logits %.2e loss %.2e distance %.3e vs %.3e" % (dlog, abs(float(loss) - float(g["loss"])), float(step.distance),
                                                                     float(g["distance"])))
        assert dlog < 1e-4
        assert abs(float(loss) - float(g["loss"])) < 1e-5
        assert abs(float(step.distance) - float(g["distance"])) <= 1e-5 * float(g["distance"]) + 1e-7
        live = [str(x) for x in g["live"]]
        grads = dict(zip(flat.names, flat.views))
        assert sorted(n for n, v in grads.items() if bool(v.ne(0).any())) == sorted(live)
        for n in live:
            exp, got = golden_grad(g, n, grads[n])
            _grad_close(got, exp, 1e-3, n)
            gn = float(g["gradnorm/" + n])
            assert abs(grads[n].double().norm().item() - gn) <= 1e-3 * gn + 1e-12, n
    finally:
        step.close()


# ---- 2. CE + lambda * distance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "enqueued"])
@pytest.mark.parametrize("name", ["p19_beta_sparse", "p12_beta_sparse", "wide80_beta_sparse"])
def test_beta_step_objective_with_distance_vs_golden(name, use_graph, precision_mode):
    """The paper's objective against the reference's autograd (fixtures and lambda of tests/test_distance_grad_gpu.py, its bounds)."""
    g, meta = load_golden(name + "_distance")
    cfg, gs, batch = case_inputs(meta)
    m = build_ours(cfg, gs, DEV, meta["param_seed"], use_beta=True, compute_distance=True).train()
    step, flat = _step(m, cfg, _to_dev(batch), use_graph=use_graph, distance_weight=float(g["lam"]))
    try:
        loss = step.run()
        torch.cuda.synchronize()
        print(name, "CE %.2e distance %.3e vs %.3e" % (abs(float(loss) - float(g["loss"])), float(step.distance), float(g["distance"])))
        assert abs(float(step.distance) - float(g["distance"])) <= 1e-5 * float(g["distance"]) + 1e-7
        assert abs(float(loss) - float(g["loss"])) < 1e-5                      # step.loss stays the CE term
        live = sorted(str(x) for x in g["live"])
        grads = dict(zip(flat.names, flat.views))
        assert sorted(flat.names) == live
        sub = {k[len("obj/"):]: v for k, v in g.items() if k.startswith("obj/")}
        for n in live:
            exp, got = golden_grad(sub, n, grads[n])
            _grad_close(got, exp, 1e-3, n)
            gn = float(sub["gradnorm/" + n])
            assert abs(grads[n].double().norm().item() - gn) <= 1e-3 * gn + 1e-12, n
        # lambda lives in a device cell: changing it changes the next step's gradients without a new capture
        before = grads["ob_propagation.map_weights"].clone()
        step.set_distance_weight(2.0 * float(g["lam"]))
        step.run()
        torch.cuda.synchronize()
        assert not torch.equal(before, grads["ob_propagation.map_weights"])
    finally:
        step.close()


# ---- 3. the new kernels against what they replace -----------------------------------------------------------------------------
def _plan_rows(shp, lengths):
    """(plan tensor, first row of every sample, clamped lengths, live rows) by rd_token_plan"""
    lib = _lib.load()
    sp = ctypes.byref(shp)
    plan = torch.zeros(max(int(lib.rd_token_plan_bytes(sp)) // 4, 64), dtype=torch.int32, device=DEV)
    _lib.call("rd_token_plan", sp, ops._ptr(lengths), ops._ptr(plan), None, 0, ops._stream())
    torch.cuda.synchronize()
    h = plan.cpu().numpy()
    B, T = shp.B, shp.T
    base = 8 + 5 * B + 2 + T + 1                                   # rd_plan.h brow_base / blen_base
    return plan, h[base:base + B], h[base + B:base + 2 * B], int(h[0])


@pytest.mark.parametrize("F,T,Kk", [(34, 60, 217), (36, 215, 300), (80, 24, 1500), (80, 24, 5000), (5, 7, 3)],
                         ids=["p19", "p12", "wide80", "wide80_unstaged", "tiny"])
def test_l2_token_kernels_bit_identical_to_what_they_replace(F, T, Kk, precision_mode):
    """k_beta_l2_tokens_fwd / _bwd against rd_edge_softmax_list_batched(norm_row=1) + rd_rows_to_tokens_fwd / _bwd (+ the ReLU gate
    autograd applies): bit-identical on the padded layout; the plan layout equals the padded one bit for bit on live rows, writes
    nothing else, and the row gradient is exactly zero where a plan-layout dz has no row.  Lengths include 1 and T; some targets
    keep no edge (coefficient 0), duplicates occur.  Kk = 5000: the coefficient pass reads the lists from global memory."""
    B, d = 6, 4
    D, K = F * d + 16, T * d
    rng = np.random.default_rng(F * 100 + T)
    lengths = torch.tensor([1, T, max(T // 2, 1), T, 2 if T > 2 else 1, max(T - 1, 1)], dtype=torch.int64, device=DEV)
    ei2 = torch.from_numpy(rng.integers(0, max(F - 2, 1), size=(B, 2, Kk))).to(DEV)       # the last targets keep no edge
    alpha = torch.from_numpy(rng.standard_normal((B, Kk)).astype(np.float32)).to(DEV)
    y2 = torch.from_numpy(rng.standard_normal((B, F, K)).astype(np.float32)).to(DEV)
    dz = torch.from_numpy(rng.standard_normal((T, B, D)).astype(np.float32)).to(DEV)
    shp = _lib.shape(B, T, F, d)
    sp = ctypes.byref(shp)
    _, ssum = ops.edge_softmax_list_batched(ei2, alpha, F, norm_row=1)
    z_ref = torch.zeros((T, B, D), device=DEV)
    _lib.call("rd_rows_to_tokens_fwd", sp, ops._ptr(y2), ops._ptr(ssum), ops._ptr(z_ref), D, ops._stream())
    dY_ref = torch.empty_like(y2)
    _lib.call("rd_rows_to_tokens_bwd", sp, ops._ptr(dz), D, ops._ptr(ssum), ops._ptr(dY_ref), ops._stream())
    dY_ref = dY_ref * (y2 > 0)
    # padded layout
    z = torch.zeros((T, B, D), device=DEV)
    dY = torch.full_like(y2, float("nan"))
    coef = torch.full((B, F), float("nan"), device=DEV)
    dYc = torch.full_like(y2, float("nan"))
    _lib.call("rd_beta_l2_tokens_fwd", sp, Kk, ops._ptr(ei2), ops._ptr(alpha), ops._ptr(y2), ops._ptr(z), D, ops._ptr(coef), ops._stream())
    _lib.call("rd_beta_l2_tokens_bwd", sp, Kk, ops._ptr(ei2), ops._ptr(alpha), ops._ptr(y2), ops._ptr(dz), D, None, ops._ptr(dY), ops._stream())
    # the stage's form: the backward reads the forward's coefficient table (and needs no lists then)
    _lib.call("rd_beta_l2_tokens_bwd", sp, Kk, None, None, ops._ptr(y2), ops._ptr(dz), D, ops._ptr(coef), ops._ptr(dYc), ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(z, z_ref)
    assert torch.equal(coef, ssum)
    assert torch.equal(dY, dY_ref)
    assert torch.equal(dYc, dY_ref)
    assert bool((ssum == 0).any()) and bool((ssum > 0).any())
    # plan layout
    plan, brow, blen, mlive = _plan_rows(shp, lengths)
    assert mlive == int(lengths.sum()) and list(blen) == [int(x) for x in lengths.cpu()]
    zp = torch.full((T * B, D), 7.0, device=DEV)
    dzp = torch.full((T * B, D), float("nan"), device=DEV)           # rows >= M_live must never be read
    for b in range(B):
        dzp[int(brow[b]):int(brow[b]) + int(blen[b])] = dz[:int(blen[b]), b]
    dYp = torch.full_like(y2, float("nan"))
    _lib.call("rd_set_token_plan", ops._ptr(plan))
    try:
        _lib.call("rd_beta_l2_tokens_fwd", sp, Kk, ops._ptr(ei2), ops._ptr(alpha), ops._ptr(y2), ops._ptr(zp), D, None, ops._stream())
        _lib.call("rd_beta_l2_tokens_bwd", sp, Kk, ops._ptr(ei2), ops._ptr(alpha), ops._ptr(y2), ops._ptr(dzp), D, None, ops._ptr(dYp),
                  ops._stream())
    finally:
        _lib.call("rd_set_token_plan", None)
    torch.cuda.synchronize()
    for b in range(B):
        r0, n = int(brow[b]), int(blen[b])
        assert torch.equal(zp[r0:r0 + n, :F * d], z_ref[:n, b, :F * d]), b
        assert bool((zp[r0:r0 + n, F * d:] == 7.0).all())                                   # the PE columns are not this kernel's
        assert torch.equal(dYp[b].view(F, T, d)[:, :n], dY_ref[b].view(F, T, d)[:, :n]), b
        assert bool((dYp[b].view(F, T, d)[:, n:] == 0).all()), b                            # no row in the plan layout: exact zeros
    assert bool((zp[mlive:] == 7.0).all())


def test_l2_token_kernels_take_an_empty_kept_list(precision_mode):
    """A graph of fewer than two edges keeps none (Kk = int(E * 0.5) = 0): the lists are empty tensors, whose data pointers are NULL.
    Every coefficient is 0 then: z's sensor columns and the row gradient are exact zeros."""
    B, T, F, d = 2, 7, 5, 4
    D = F * d + 16
    shp = _lib.shape(B, T, F, d)
    sp = ctypes.byref(shp)
    y2 = torch.ones((B, F, T * d), device=DEV)
    z = torch.full((T, B, D), 7.0, device=DEV)
    dY = torch.full_like(y2, float("nan"))
    _lib.call("rd_beta_l2_tokens_fwd", sp, 0, None, None, ops._ptr(y2), ops._ptr(z), D, None, ops._stream())
    _lib.call("rd_beta_l2_tokens_bwd", sp, 0, None, None, ops._ptr(y2), ops._ptr(z), D, None, ops._ptr(dY), ops._stream())
    torch.cuda.synchronize()
    assert bool((z[:, :, :F * d] == 0).all()) and bool((z[:, :, F * d:] == 7.0).all())
    assert bool((dY == 0).all())


# ---- 4. the same step as the eager model --------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph,token_plan", [(True, True), (False, True), (True, False)], ids=["graph", "enqueued", "graph_padded"])
def test_beta_step_matches_eager_model(use_graph, token_plan, precision_mode, monkeypatch):
    """Dropout off, three batches copied into the static buffers: loss, logits and every flat gradient against the eager
    model.forward -> cross_entropy -> backward.  Bound: tests/test_gpu_parity.py::test_static_train_step_matches_autograd's for the
    default branch in the same arithmetic (fused head: 5e-5 of the tensor's max-norm in split-bf16, 1e-5 in fp32; loss 5e-6 /
    1e-6).  The kept edge lists equal the eager model's exactly (H is exact fp32 on both sides)."""
    tol, ltol = (1e-5, 1e-6) if precision_mode == "fp32" else (5e-5, 5e-6)
    cfg = synth.make_config("P19")
    gs = synth.make_structure(cfg, "sparse")
    m = build_ours(cfg, gs, DEV, 7, use_beta=True, compute_distance=True).train()
    named = dict(m.named_parameters())
    live = synth.live_parameter_names_beta(cfg)
    seen = {}
    real = ops.graph_beta

    def spy(*a, **k):
        out = real(*a, **k)
        seen["ei2"] = out[1].detach().clone()
        return out
    monkeypatch.setattr(ops, "graph_beta", spy)
    buf = _to_dev(synth.make_batch(cfg, 8, seed=41))
    step, flat = _step(m, cfg, buf, use_graph=use_graph, token_plan=token_plan)
    try:
        assert step.head_fused
        for seed in (41, 42, 43):
            dv = _to_dev(synth.make_batch(cfg, 8, seed=seed))
            for k, v in dv.items():
                buf[k].copy_(v)
            logits, distance, _ = m(dv["src"], dv["static"], dv["times"], dv["lengths"])
            loss = torch.nn.functional.cross_entropy(logits, dv["y"])
            ref = torch.autograd.grad(loss, [named[n] for n in live])
            l2 = step.run()
            torch.cuda.synchronize()
            worst = max((_rel(named[n].grad.cpu().numpy(), r.cpu().numpy()), n) for n, r in zip(live, ref))
            print(seed, "loss %.2e logits %.2e worst grad %.2e (%s)" % (abs(float(l2) - float(loss)), _rel(step.logits.cpu().numpy(),
                  logits.detach().cpu().numpy()), worst[0], worst[1]))
            assert torch.equal(step.ei2, seen["ei2"])
            assert abs(float(l2) - float(loss)) < ltol
            assert _rel(step.logits.cpu().numpy(), logits.detach().cpu().numpy()) < tol
            assert abs(float(step.distance) - float(distance)) <= 1e-6 * float(distance)
            for n, r in zip(live, ref):
                assert _rel(named[n].grad.cpu().numpy(), r.cpu().numpy()) < tol, n
    finally:
        step.close()


# ---- 5. dropout ---------------------------------------------------------------------------------------------------------------
def test_beta_step_dropout_graph_equals_enqueued_body(precision_mode):
    """Dropout 0.2: a graph replay equals the hand-enqueued body bit for bit at equal seed-cell values; two replays differ; the
    gradients are those of the forward's masks (the replay repeated with the cell rewound gives the same bits)."""
    cfg = synth.make_config("P19")
    gs = synth.make_structure(cfg, "sparse")
    dv = _to_dev(synth.make_batch(cfg, 8, seed=43))
    out = []
    for use_graph in (True, False):
        m = build_ours(cfg, gs, DEV, 7, use_beta=True, compute_distance=True).train()
        step, flat = _step(m, cfg, dv, p_drop=0.2, use_graph=use_graph, seed=99)
        try:
            step.seed_cell.zero_()                                    # the capture's warm-up runs bumped it
            l1 = float(step.run()); torch.cuda.synchronize(); g1 = flat.flat.clone(); a1 = step.alpha.clone()
            l2 = float(step.run()); torch.cuda.synchronize(); g2 = flat.flat.clone(); a2 = step.alpha.clone()
            step.seed_cell.zero_()
            l3 = float(step.run()); torch.cuda.synchronize(); g3 = flat.flat.clone(); a3 = step.alpha.clone()
            out.append((l1, g1, l2, g2))
            assert l1 != l2 and not torch.equal(g1, g2)
            assert l1 == l3 and torch.equal(g1, g3)
            # the sensor stage's OWN dropout site follows the cell (the encoder's masks alone would already change the loss): the
            # edge scores are computed from the dropped observation embedding, in front of every encoder layer
            assert not torch.equal(a1, a2) and torch.equal(a1, a3)
        finally:
            step.close()
    (a1, ga1, a2, ga2), (b1, gb1, b2, gb2) = out
    assert a1 == b1 and a2 == b2
    assert torch.equal(ga1, gb1) and torch.equal(ga2, gb2)


# ---- 6. the whole step --------------------------------------------------------------------------------------------------------
def _kept_order_gap(cfg, gs, params, b):
    """tests/golden/make_distance_goldens.py kept_order_gap: the smallest gap between consecutive kept scores (and the first pruned
    one) over the samples of a batch, relative to the largest score, by the fp32 restatement (oracle O2)"""
    from oracle import restatement as O2
    with torch.no_grad():
        _, _, inter = O2.raindrop_v2_forward(params, cfg, b["src"], b["static"], b["times"], b["lengths"], gs, faithful=True,
                                             use_beta=True, return_intermediates=True)
    h, pe = inter["h"], inter["pe"]
    T, B, F_, d = h.shape[0], h.shape[1], cfg["d_inp"], cfg["d_ob"]
    ei, ew = O2.build_graph(gs.numpy())
    worst = np.inf
    for u in range(B):
        x = h[:, u, :].reshape(T, F_, d).permute(1, 0, 2).reshape(F_, T * d)
        sc = O2.beta_edge_scores(x, pe[:, u, :], torch.from_numpy(ei), torch.from_numpy(ew), params["ob_propagation.increase_dim.weight"],
                                 params["ob_propagation.increase_dim.bias"], params["ob_propagation.map_weights"], d).double().numpy()
        top = np.sort(sc)[::-1][: len(sc) // 2 + 1]
        worst = min(worst, float((-np.diff(top)).min() / np.abs(sc).max()))
    return worst


def test_beta_whole_step_follows_the_eager_adam_loop():
    """capture_full(FlatAdam), 5 steps, exact-fp32 mode, dropout off, against the eager loop (model.forward -> CE -> backward ->
    torch.optim.Adam, same lr).  Bounds: the fp32 ones of tests/test_trajectory_gpu.py (losses 2e-6, last logits 1e-5, trained
    weights within 2e-3 of how far training moved them -- 3e-3 for the in_proj_bias tensors, whose zero-gradient key third Adam moves by noise,
    see the comment at the assertion).  Top-K pruning is discontinuous, so the five batch seeds are chosen the
    way tests/golden/make_distance_goldens.py chooses its one: the first seeds (from 300 on) whose batches have no near-tied kept
    scores at the initial weights (relative gap > 1e-6 by the fp32 restatement)."""
    from raindrop_amd.optim import FlatAdam
    from raindrop_amd.step_beta import BetaTrainStep
    lr, nsteps, B = 1e-3, 5, 8
    cfg = synth.make_config("P19")
    gs = synth.make_structure(cfg, "sparse")
    p0 = {n: t.detach() for n, t in build_ours(cfg, gs, "cpu", 7, use_beta=True).named_parameters()}
    batches = []
    for seed in range(300, 360):
        b = synth.make_batch(cfg, B, seed=seed)
        if _kept_order_gap(cfg, gs, p0, b) > 1e-6:
            batches.append(b)
        if len(batches) == nsteps:
            break
    assert len(batches) == nsteps
    _lib.call("rd_set_precision", 0)
    try:
        ma = build_ours(cfg, gs, DEV, 7, use_beta=True).train()
        opt_a = torch.optim.Adam(ma.parameters(), lr=lr)
        la = []
        for b in batches:
            dv = _to_dev(b)
            logits_a, _, _ = ma(dv["src"], dv["static"], dv["times"], dv["lengths"])
            opt_a.zero_grad()
            loss = torch.nn.functional.cross_entropy(logits_a, dv["y"])
            loss.backward()
            opt_a.step()
            la.append(float(loss))
        mb = build_ours(cfg, gs, DEV, 7, use_beta=True).train()
        flat = _flat(mb, cfg, n_buckets=2)
        opt_b = FlatAdam(flat.flatten_parameters(), lr=lr)
        buf = {k: (None if v is None else v.to(DEV).clone()) for k, v in batches[0].items()}
        step = BetaTrainStep(mb, flat, buf, p_drop=0.0, autotune=False, split=False)
        try:
            step.capture_full(opt_b)
            lb = []
            for b in batches:
                for k, v in b.items():
                    if v is not None:
                        buf[k].copy_(v)
                lb.append(float(step.run_full()))
            torch.cuda.synchronize()
            last = step.logits.cpu().numpy().copy()
        finally:
            step.close()
        dl = np.abs(np.array(la) - np.array(lb)).max()
        d_last = np.abs(last - logits_a.detach().cpu().numpy()).max()
        pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
        werrs = sorted(((float((pb[n].detach().cpu().double() - pa[n].detach().cpu().double()).norm())
                         / max(float((pa[n].detach().cpu().double() - p0[n].double()).norm()), 1e-30), n)
                        for n in synth.live_parameter_names_beta(cfg)), reverse=True)
        werr = werrs[0]
        print("whole step: largest weight errors", ["%.2e %s" % w for w in werrs[:4]])
        print("whole step: loss %.2e last logits %.2e weights %.2e (%s)" % (dl, d_last, werr[0], werr[1]))
        D = cfg["d_model"] + 16
        for i in range(cfg["nlayers"]):                              # where an in_proj_bias differs: the q | k | v thirds
            n = "transformer_encoder.layers.%d.self_attn.in_proj_bias" % i
            e, mv = (pb[n] - pa[n]).detach().cpu().double(), pa[n].detach().cpu().double() - p0[n].double()
            print(n, "error / moved norms by q|k|v third:", ["%.2e / %.2e" % (float(e[j * D:(j + 1) * D].norm()),
                                                                              float(mv[j * D:(j + 1) * D].norm())) for j in range(3)])
            for j in (0, 2):                                         # the thirds that HAVE a gradient keep the default-branch bound
                assert float(e[j * D:(j + 1) * D].norm()) < 2e-3 * float(mv[j * D:(j + 1) * D].norm()), (n, j)
        assert opt_b.t == nsteps
        assert dl < 2e-6 and d_last < 1e-5, (dl, d_last)
        # MEASURED: 2.07e-3, all of it in the KEY third of layer 1's in_proj_bias (error 7.8e-5 of 8.0e-5 moved; the q and v thirds
        # agree to 2e-6 of their movement, every other tensor is below the default branch's 2e-3).  The key bias cancels in the
        # softmax: its true gradient is 0, what arrives is rounding noise, and Adam turns noise into O(lr) steps of either sign --
        # in ANY two evaluations that sum in a different order (here: the fused encoder chains against the operator surface).  The
        # 20-step default-branch fixture hides it behind 20 steps of real movement of the other thirds; 5 steps do not.  Bound at
        # the measurement with a 1.45x margin FOR THOSE TENSORS ONLY, whose thirds with a gradient keep 2e-3 above;
        # every other tensor keeps the default branch's 2e-3.
        for e, n in werrs:
            assert e < (3e-3 if n.endswith("self_attn.in_proj_bias") else 2e-3), (e, n)
    finally:
        _lib.call("rd_set_precision", 1)


# ---- 7. data parallel ---------------------------------------------------------------------------------------------------------
B_GLOBAL = 16


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _dp_grad(batch, split):
    """one BetaTrainStep graph step on `batch` + the all-reduce of the flat buffer; returns (loss, flat gradient, split form used)"""
    from raindrop_amd.step_beta import BetaTrainStep
    dev = torch.device("cuda", 0)
    cfg = synth.make_config("P19")
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), dev, 21, use_beta=True).train()
    flat = _flat(m, cfg, n_buckets=2)
    b = {k: (None if v is None else v.to(dev)) for k, v in batch.items()}
    ts = BetaTrainStep(m, flat, b, p_drop=0.0, use_graph=True, autotune=False, split=split)
    try:
        loss = float(ts.run_allreduce())
        torch.cuda.synchronize()
        return loss, flat.flat.detach().cpu().numpy().copy(), (ts.split, ts.graph_b is not None)
    finally:
        ts.close()


def _dp_worker(rank, world, port, ret, split):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    full = synth.make_batch(synth.make_config("P19"), B_GLOBAL, seed=33)
    ret[rank] = _dp_grad(dp.shard_batch(full, rank, world), split)
    dist.destroy_process_group()


@pytest.mark.parametrize("split", [False, True], ids=["one_graph", "two_graphs"])
def test_beta_two_rank_gradients_equal_the_full_batch(split):
    """Two ranks (spawned children sharing cuda:0 over gloo, as tests/test_dp_gpu.py): the all-reduced flat gradient is bit-identical
    on both ranks and equals one process's gradient on the whole batch within that file's bound (3e-5 of the largest entry); the
    one-graph form and the two-graph form whose first bucket's collective starts between the graphs."""
    full = synth.make_batch(synth.make_config("P19"), B_GLOBAL, seed=33)
    _, g_ref, _ = _dp_grad(full, False)
    world, port = 2, _free_port()
    ret = mp.Manager().dict()
    mp.spawn(_dp_worker, args=(world, port, ret, split), nprocs=world, join=True)
    (l0, g0, f0), (l1, g1, f1) = ret[0], ret[1]
    assert f0 == f1 == (split, split)
    assert np.array_equal(g0, g1)
    gscale = np.abs(g_ref).max()
    print("two ranks (%s): max |dg| / max |g| = %.2e" % ("two graphs" if split else "one graph", np.abs(g0 - g_ref).max() / gscale))
    assert np.abs(g0 - g_ref).max() <= 3e-5 * gscale


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------
def test_beta_step_refusals():
    from raindrop_amd.step_beta import BetaTrainStep
    cfg = synth.make_config("P19")
    gs = synth.make_structure(cfg, "sparse")
    b = _to_dev(synth.make_batch(cfg, 8, seed=3))
    m = build_ours(cfg, gs, DEV, 21).train()                                    # the default branch: TrainStep's
    named = dict(m.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)])
    with pytest.raises(_lib.RaindropHipError, match="TrainStep"):
        BetaTrainStep(m, flat, b, use_graph=False)
    m = build_ours(cfg, gs, DEV, 21, use_beta=True).train()                     # no compute_distance: the distance is the constant 0
    with pytest.raises(_lib.RaindropHipError, match="compute_distance"):
        BetaTrainStep(m, _flat(m, cfg), b, use_graph=False, distance_weight=0.1)
    named = dict(m.named_parameters())
    for lacking in EXTRA:
        flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names_beta(cfg) if n != lacking])
        with pytest.raises(_lib.RaindropHipError, match=lacking.replace(".", r"\.")):
            BetaTrainStep(m, flat, b, use_graph=False)
    step = BetaTrainStep(m, _flat(m, cfg), b, use_graph=False)                  # and the CE-only step has no lambda to change
    with pytest.raises(_lib.RaindropHipError, match="distance_weight"):
        step.set_distance_weight(0.5)
    step.close()
