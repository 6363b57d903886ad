"""GPU: the gradient of the structure-distance regulariser (code/models_rd.py:345-346) through the whole model, against fixtures made
by the reference's own autograd (tests/golden/make_distance_goldens.py): d distance alone, and d (CE + lambda * distance) -- the
paper's objective -- for Raindrop_v2(use_beta=True, compute_distance=True).  Both arithmetic modes; wide80 (80 sensors) runs the
graph operator's workspace form.  Bounds as tests/test_gpu_parity.py::test_model_use_beta_vs_golden."""
import numpy as np
import pytest
import torch

from tests.helpers import build_ours, case_inputs, golden_grad, load_golden
from tests.test_gpu_parity import _grad_close, precision_mode  # noqa: F401  (autouse: every test here runs in both modes)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIST_CASES = ["p19_beta_sparse", "p12_beta_sparse", "wide80_beta_sparse"]
DIST_LIVE = ["R_u", "ob_propagation.increase_dim.bias", "ob_propagation.increase_dim.weight", "ob_propagation.map_weights"]


def _set(g, prefix):
    """one gradient set of a fixture, under the names tests.helpers.golden_grad reads"""
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


def _check_set(g, prefix, names, grads):
    sub = _set(g, prefix)
    for n in names:
        exp, got = golden_grad(sub, n, grads[n])
        _grad_close(got, exp, 1e-3, n)
        gn = float(sub["gradnorm/" + n])
        assert abs(grads[n].double().norm().item() - gn) <= 1e-3 * gn + 1e-12, (prefix, n)


@pytest.mark.parametrize("name", DIST_CASES)
def test_model_distance_gradient_vs_golden(name, precision_mode):
    g, meta = load_golden(name + "_distance")
    cfg, gs, batch = case_inputs(meta)
    m = build_ours(cfg, gs, DEV, meta["param_seed"], use_beta=True, compute_distance=True).train()
    dv = {k: (None if v is None else v.to(DEV)) for k, v in batch.items()}
    logits, distance, _ = m(dv["src"], dv["static"], dv["times"], dv["lengths"])
    assert distance.requires_grad and distance.grad_fn is not None
    assert abs(float(distance) - float(g["distance"])) <= 1e-5 * float(g["distance"]) + 1e-7
    params = dict(m.named_parameters())
    names = [n for n, p in params.items() if p.requires_grad]
    # d distance alone: exactly the tensors the reference's distance reaches (the autograd engine still runs layer 1's lin_value
    # backward, on a zero gradient: its weights get exact zeros where the reference has none)
    gd = dict(zip(names, torch.autograd.grad(distance, [params[n] for n in names], retain_graph=True, allow_unused=True)))
    dlive = sorted(str(x) for x in g["dlive"])
    assert dlive == DIST_LIVE
    assert sorted(n for n, x in gd.items() if x is not None and bool(x.ne(0).any())) == dlive
    _check_set(g, "dist/", dlive, gd)
    # the paper's objective
    ce = torch.nn.functional.cross_entropy(logits, dv["y"])
    assert abs(float(ce) - float(g["loss"])) < 1e-5
    (ce + float(g["lam"]) * distance).backward()
    live = sorted(str(x) for x in g["live"])
    assert sorted(n for n, p in params.items() if p.grad is not None) == live
    _check_set(g, "obj/", live, {n: params[n].grad for n in live})


def test_distance_changes_nothing_for_a_ce_loss(precision_mode):
    """compute_distance=True makes the scores differentiable; a loss without the distance gets the same bits as without it, and
    eval / no-grad calls return a constant distance"""
    g, meta = load_golden("p19_beta_sparse_distance")
    cfg, gs, batch = case_inputs(meta)
    dv = {k: (None if v is None else v.to(DEV)) for k, v in batch.items()}
    grads = []
    for cd in (False, True):
        m = build_ours(cfg, gs, DEV, meta["param_seed"], use_beta=True, compute_distance=cd).train()
        logits, distance, _ = m(dv["src"], dv["static"], dv["times"], dv["lengths"])
        assert distance.requires_grad == cd
        torch.nn.functional.cross_entropy(logits, dv["y"]).backward()
        grads.append({n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
        with torch.no_grad():
            _, d0, _ = m(dv["src"], dv["static"], dv["times"], dv["lengths"])
        assert not d0.requires_grad
    assert set(grads[0]) == set(grads[1])
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]), n
    # the default branch: the constant 0, no gradient
    m0 = build_ours(cfg, gs, DEV, meta["param_seed"], compute_distance=True).train()
    _, d0, _ = m0(dv["src"], dv["static"], dv["times"], dv["lengths"])
    assert float(d0) == 0.0 and not d0.requires_grad
    assert np.isfinite(float(d0))
