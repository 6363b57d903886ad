"""GPU: the operators behind the differentiable structure distance -- rd_graph_beta_bwd_alpha (the alpha cotangent in both forms of
the use_beta graph operator) and rd_structure_distance_bwd -- and AutogradStep(distance_weight=lambda).
Operator gradients against tests/golden/beta_distance_op.npz (the reference's Observation_progation with per-sample edge weights,
tests/golden/make_distance_goldens.py) to 2e-5 of their max-norm; the distance backward against torch's float64 cdist autograd."""
import os

import numpy as np
import pytest
import torch

from oracle import restatement as O2
from raindrop_amd import _lib, ops, synth
from raindrop_amd.Ob_propagation import Observation_progation
from tests.helpers import GOLDEN, build_ours, case_inputs, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
OP_GRADS = ["gX", "gWv", "gbv", "gWi", "gbi", "gmap", "gEW"]


def _t(a):
    return torch.from_numpy(np.asarray(a)).to(DEV)


def _op_run(g, large, monkeypatch, alpha_grad=True, with_alpha=True):
    """the fixture's operator case through ops.graph_beta -> (Y, edge_index', alpha, gradients in OP_GRADS order)"""
    n, T, d, B = (int(v) for v in g["dims"])
    K = T * d
    op = Observation_progation(K, K, n_nodes=n, ob_dim=d, heads=1)
    synth.fill_params_(op, seed=int(g["param_seed"]))
    op = op.to(DEV)
    ei, _ = O2.build_graph(g["adj"])
    X = _t(g["X"]).requires_grad_(True)
    EW = _t(g["EW"]).requires_grad_(True)
    if large:
        monkeypatch.setenv("RD_BETA_LARGE", "1")
    try:
        V = ops.linear(X.reshape(B * n, K), op.lin_value.weight, op.lin_value.bias, act=1).view(B, n, K)
        H = ops.linear(X.reshape(B * n, K), op.increase_dim.weight, op.increase_dim.bias, exact=True).view(B, n, T * 32)
        Y, ei2, alpha = ops.graph_beta(V, H, op.map_weights, _t(g["PT"]), _t(ei), EW, d, alpha_grad=alpha_grad)
        loss = (Y * _t(g["Ry"])).sum()
        if with_alpha:
            loss = loss + (alpha * _t(g["Ra"])).sum()
        grads = torch.autograd.grad(loss, [X, op.lin_value.weight, op.lin_value.bias, op.increase_dim.weight, op.increase_dim.bias,
                                           op.map_weights, EW])
        torch.cuda.synchronize()
    finally:
        monkeypatch.delenv("RD_BETA_LARGE", raising=False)
    return Y.detach(), ei2, alpha.detach(), [x.detach() for x in grads]


@pytest.mark.parametrize("large", [False, True], ids=["lds", "workspace"])
def test_alpha_cotangent_matches_reference_fixture(large, monkeypatch):
    """d(<alpha, R_a> + <Y, R_y>) with per-sample edge weights (the d edge weight path), in each form of the operator"""
    g = np.load(os.path.join(GOLDEN, "beta_distance_op.npz"))
    Y, ei2, alpha, grads = _op_run(g, large, monkeypatch)
    assert np.array_equal(ei2.cpu().numpy(), g["ei"])
    assert np.abs(alpha.cpu().numpy() - g["alpha"]).max() < 1e-6
    assert np.abs(Y.cpu().numpy() - g["Y"]).max() < 1e-5
    for name, got in zip(OP_GRADS, grads):
        ref = g[name]
        assert np.abs(got.cpu().numpy() - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-9, name


def test_alpha_cotangent_forms_agree(monkeypatch):
    g = np.load(os.path.join(GOLDEN, "beta_distance_op.npz"))
    _, es, _, gs = _op_run(g, False, monkeypatch)
    _, el, _, gl = _op_run(g, True, monkeypatch)
    assert torch.equal(es, el)
    for name, a, b in zip(OP_GRADS, gs, gl):
        assert float((a - b).abs().max()) <= 5e-6 * float(a.abs().max()) + 1e-9, name


@pytest.mark.parametrize("large", [False, True], ids=["lds", "workspace"])
def test_alpha_grad_changes_nothing_without_an_alpha_term(large, monkeypatch):
    """alpha_grad=True with a loss of Y alone: the same bits as alpha_grad=False (no cotangent reaches the kernel)"""
    g = np.load(os.path.join(GOLDEN, "beta_distance_op.npz"))
    Y0, e0, a0, g0 = _op_run(g, large, monkeypatch, alpha_grad=False, with_alpha=False)
    Y1, e1, a1, g1 = _op_run(g, large, monkeypatch, alpha_grad=True, with_alpha=False)
    assert torch.equal(Y0, Y1) and torch.equal(e0, e1) and torch.equal(a0, a1)
    for name, a, b in zip(OP_GRADS, g0, g1):
        assert torch.equal(a, b), name


def _abi_bwd(g, large, monkeypatch, dalpha_mode):
    """rd_graph_beta_fwd, then rd_graph_beta_bwd (dalpha_mode None) or rd_graph_beta_bwd_alpha with dalpha NULL / zeros / the
    fixture's R_a; returns (dV, dH, dmap_part, dw)"""
    n, T, d, B = (int(v) for v in g["dims"])
    K = T * d
    ei, _ = O2.build_graph(g["adj"])
    ei = _t(ei)
    E = ei.shape[1]
    rng = np.random.default_rng(3)
    V = _t(np.abs(rng.standard_normal((B, n, K))).astype(np.float32))
    H = _t(rng.standard_normal((B, n, T * 32)).astype(np.float32))
    mw = _t(rng.standard_normal((n, 16)).astype(np.float32))
    PT = _t(g["PT"])
    EW = _t(g["EW"])
    dout = _t(rng.standard_normal((B, n, K)).astype(np.float32))
    lib = _lib.load()
    Kk = int(lib.rd_graph_beta_kept(E))
    P = ops._ptr
    if large:
        monkeypatch.setenv("RD_BETA_LARGE", "1")
    try:
        ws = ops._workspace(lib.rd_graph_beta_workspace_bytes(B, n, K, T, E), V.device)
        out = torch.empty_like(V)
        ei_out = torch.empty((B, 2, Kk), dtype=torch.int64, device=DEV)
        alpha = torch.empty((B, Kk), dtype=torch.float32, device=DEV)
        beta = torch.empty((B, n, T), dtype=torch.float32, device=DEV)
        kept = torch.empty((B, Kk), dtype=torch.int32, device=DEV)
        _lib.call("rd_graph_beta_fwd", B, n, K, T, d, E, P(V), P(H), P(mw), P(PT), T * 16, P(ei), ei.stride(0), P(EW), E, P(out),
                  P(ei_out), P(alpha), P(beta), P(kept), P(ws), ws.numel(), ops._stream())
        dV, dH = torch.full_like(V, 7.0), torch.full_like(H, 7.0)
        dmap = torch.full((B, n, 16), 7.0, device=DEV)
        dw = torch.full((B, E), 7.0, device=DEV)
        head = (B, n, K, T, d, E, P(V), P(H), P(mw), P(PT), T * 16, P(ei), ei.stride(0), P(EW), E, P(beta), P(kept), P(dout))
        tail = (P(dV), P(dH), P(dmap), P(dw), P(ws), ws.numel(), ops._stream())
        if dalpha_mode is None:
            _lib.call("rd_graph_beta_bwd", *head, *tail)
        else:
            da = {"null": None, "zero": torch.zeros((B, Kk), device=DEV), "fixture": _t(g["Ra"])}[dalpha_mode]
            _lib.call("rd_graph_beta_bwd_alpha", *head, P(da), *tail)
        torch.cuda.synchronize()
    finally:
        monkeypatch.delenv("RD_BETA_LARGE", raising=False)
    return dV, dH, dmap, dw


@pytest.mark.parametrize("large", [False, True], ids=["lds", "workspace"])
def test_bwd_alpha_abi_null_and_zero_are_the_old_backward(large, monkeypatch):
    g = np.load(os.path.join(GOLDEN, "beta_distance_op.npz"))
    base = _abi_bwd(g, large, monkeypatch, None)
    for mode in ("null", "zero"):
        got = _abi_bwd(g, large, monkeypatch, mode)
        for a, b in zip(base, got):
            assert torch.equal(a, b), mode
    # with a cotangent: dH, d map_weights and d edge weight move, dV does not; two runs give the same bits (no atomics)
    r1 = _abi_bwd(g, large, monkeypatch, "fixture")
    r2 = _abi_bwd(g, large, monkeypatch, "fixture")
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)
    assert torch.equal(r1[0], base[0])
    for a, b in zip(r1[1:], base[1:]):
        assert not torch.equal(a, b)


def test_v1_kernels_refuse_a_cotangent(monkeypatch):
    g = np.load(os.path.join(GOLDEN, "beta_distance_op.npz"))
    monkeypatch.setenv("RD_BETA_V1", "1")
    with pytest.raises(_lib.RaindropHipError, match="RD_EUNSUPPORTED"):
        _abi_bwd(g, False, monkeypatch, "fixture")
    _abi_bwd(g, False, monkeypatch, "null")                         # and take none as before


def _torch_grad(A, gscale):
    a = A.detach().double().cpu().requires_grad_(True)
    d = torch.cdist(a.T, a.T, p=2).mean() * gscale
    return torch.autograd.grad(d, a)[0]


@pytest.mark.parametrize("Kk,B", [(214, 256), (578, 256), (6680, 16)])
def test_distance_backward_matches_torch_cdist(Kk, B):
    """alpha_all [Kk,B]: P19's sparse / all-ones structures at B = 256 and a 256-node graph's kept edges at B = 16 (two samples
    identical: D = 0 among non-zero distances)"""
    rng = np.random.default_rng(Kk + B)
    A = (0.05 + 0.02 * rng.standard_normal((Kk, B))).astype(np.float32)
    if B == 16:
        A[:, 5] = A[:, 3]
    a = _t(A).requires_grad_(True)
    dist = ops.structure_distance(a)
    assert dist.grad_fn is not None
    (dist * 1.7).backward()
    ref = _torch_grad(torch.from_numpy(A), 1.7).numpy()
    got = a.grad.double().cpu().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max(), np.abs(got - ref).max() / np.abs(ref).max()
    d64 = torch.cdist(torch.from_numpy(A).double().T, torch.from_numpy(A).double().T).mean().item()
    assert abs(float(dist) - d64) <= 1e-6 * d64
    # no-grad input: the constant, the same value
    assert float(ops.structure_distance(a.detach())) == float(dist)


@pytest.mark.parametrize("Kk,B", [(30, 1), (30, 8), (0, 4)], ids=["one_sample", "identical_columns", "no_edges"])
def test_distance_backward_zero_cases(Kk, B):
    A = np.tile(np.linspace(0.1, 0.4, Kk, dtype=np.float32)[:, None], (1, B))
    a = _t(A).requires_grad_(True)
    dist = ops.structure_distance(a)
    dist.backward()
    assert float(dist) == 0.0
    assert a.grad.shape == (Kk, B)
    assert torch.equal(a.grad, torch.zeros_like(a)) and not torch.isnan(a.grad).any()


def test_autograd_step_trains_the_paper_s_objective():
    """AutogradStep(distance_weight=lambda): the captured step minimises CE + lambda * distance.  Dropout on: a replay equals the
    eager loop body with the same seed cell value and by-value seed, bit for bit (loss, logits, every gradient); lambda = 0 is the
    CE step; a model whose distance is the constant 0 is refused."""
    from raindrop_amd.step import AutogradStep
    g, meta = load_golden("p19_beta_sparse_distance")
    cfg, gs, batch = case_inputs(meta)
    lam = float(g["lam"])

    def model():
        m = build_ours(cfg, gs, DEV, meta["param_seed"], use_beta=True, compute_distance=True).train()
        m.graph_step = False
        m.dropout.p = 0.2
        return m

    mg, me = model(), model()
    buf = {k: (None if v is None else v.to(DEV).clone()) for k, v in batch.items()}
    st = AutogradStep(mg, buf, optimizer=False, distance_weight=lam)
    captured = mg._drop_calls                                        # the by-value seed the capture used
    for cell_value in (7, 11):
        st.seed_cell.fill_(cell_value)
        loss_g = float(st.run())
        torch.cuda.synchronize()
        lg_g = st.logits.clone()
        grads_g = {n: p.grad.clone() for n, p in mg.named_parameters() if p.grad is not None}
        cell = torch.full((1,), cell_value + 1, dtype=torch.int64, device=DEV)     # the graph bumps the cell before its forward
        _lib.call("rd_set_seed_cell", ops._ptr(cell))
        try:
            for p in me.parameters():
                p.grad = None
            me._drop_calls = captured - 1
            lg, dist, _ = me(buf["src"], buf["static"], buf["times"], buf["lengths"])
            loss = torch.nn.functional.cross_entropy(lg, buf["y"]) + lam * dist
            loss.backward()
            torch.cuda.synchronize()
        finally:
            _lib.call("rd_set_seed_cell", None)
        assert loss_g == float(loss) and torch.equal(lg_g, lg.detach())
        grads_e = {n: p.grad for n, p in me.named_parameters() if p.grad is not None}
        assert set(grads_g) == set(grads_e)
        for n in grads_g:
            assert torch.equal(grads_g[n], grads_e[n]), n
        assert float(dist) > 0.0
    # lambda = 0 captures the CE step: with the same masks, the regulariser's share of the gradient is what differs
    m0 = model()
    s0 = AutogradStep(m0, buf, optimizer=False, distance_weight=0.0)
    s0.seed_cell.fill_(11)
    loss0 = float(s0.run())
    torch.cuda.synchronize()
    assert abs(loss_g - lam * float(dist) - loss0) <= 1e-6 * abs(loss0)
    wi = "ob_propagation.increase_dim.weight"
    assert not torch.equal(dict(m0.named_parameters())[wi].grad, grads_g[wi])
    # refusals: lambda * 0 would be silently wrong training
    for kw in (dict(use_beta=True), dict(compute_distance=True), {}):
        m = build_ours(cfg, gs, DEV, meta["param_seed"], **kw).train()
        with pytest.raises(_lib.RaindropHipError, match="distance_weight"):
            AutogradStep(m, buf, optimizer=False, distance_weight=lam)
