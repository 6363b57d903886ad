"""CPU: conditions on the float64 reference of the sensor stage alone (tests/sensor_stage_ref.py), so that the GPU comparison of
tests/test_sensor_stage_float64_gpu.py is known to bite before any kernel runs:

  * every gate of both layers of every case lies at least GATE_MARGIN from zero, between a quarter and three quarters of the gates
    of each layer are open, and the gate pattern differs from row to row and from column to column;
  * no compared tensor is all-zero (the mask: exactly where no sample is shorter than T);
  * the case table selects the layout edges it claims to (rd_k1_layout.h restated in sensor_stage_ref.layout_numbers);
  * the batched reference equals the per-sample, per-edge form of oracle/restatement.py observation_propagation (the one
    test_sensor_stage_vs_oracle uses) under torch autograd in float64 to 1e-12, and a central finite difference;
  * five wrong references (VARIANTS) each miss a bound of the float64 tie by more than 10 x."""
import numpy as np
import pytest
import torch

from oracle import restatement as O2
from tests import sensor_stage_ref as SR

ALL_CASES = [("padded", n) for n in SR.PADDED_CASES + SR.COEF_CASES] + [("plan", c) for c in SR.PLAN_CASES]
_id = lambda k: k[1] if isinstance(k[1], str) else "%s@%s" % k[1]


def _case(kind, key):
    return SR.case(key) if kind == "padded" else SR.plan_case(*key)


@pytest.mark.parametrize("kind,key", ALL_CASES, ids=[_id(k) for k in ALL_CASES])
def test_gates_are_decisive_balanced_and_row_dependent(kind, key):
    c = _case(kind, key)
    r = SR.reference(c)
    B, F, K = c["B"], c["F"], c["K"]
    assert B <= 40 and B * F <= SR.MAX_ROWS
    assert c["b1"].dtype == np.float32 and c["b2"].dtype == np.float32
    for layer in ("pre1", "pre2"):
        pre = r[layer]
        assert pre.shape == (B, F, K)
        margin, opened = float(np.abs(pre).min()), float((pre > 0).mean())
        print("%s %s: min |pre| = %.2e, open %.1f %%, std %.2f" % (c["name"], layer, margin, 100 * opened, pre.std()))
        assert margin >= SR.GATE_MARGIN, (layer, margin)
        assert 0.25 <= opened <= 0.75, (layer, opened)
        g = (pre > 0).reshape(B * F, K)
        if B * F >= 16:                                  # no two columns gate the rows alike, and the rows do not gate alike either
            assert len(np.unique(g, axis=1).T) > K // 2 and len(np.unique(g, axis=0)) > 1
    # observations stop at the sample's length (no plan slack), the X gate is exact by make_case's own assertion
    obs = c["src"][:, :, :F] != 0
    assert not (obs & (np.arange(c["T"])[:, None, None] >= c["lengths"][None, :, None])).any()
    cmp_ = SR.compared(c, r)
    for name, t in cmp_.items():
        assert np.isfinite(t).all() and np.abs(t).max() > 0, name
    assert r["mask"].any() == bool((c["lengths"] < c["T"]).any())
    if kind == "plan":
        assert cmp_["z"].shape == (c["plan"]["mlive"], 4 * F) and c["plan"]["mlive"] == int(c["lengths"].sum())


def test_case_table_selects_the_edges_it_names():
    N = lambda n: SR.layout_numbers(*SR.SHAPES[n][:3])
    assert N("F1_B3")["per"] == 32 and N("F1_B3")["S"] == 1 and N("F1_B3")["nct"] == 1 and N("F1_B3")["nkc"] == 1
    assert N("F1_B33")["S"] == 2
    assert N("F5")["per"] == 6 and 6 * 5 == 30 and N("F5")["S"] == 2
    assert N("F16")["per"] == 2 and N("F17")["per"] == 1 and N("F31")["per"] == 1
    assert N("F32")["rem"] == 0 and N("F32")["S"] == 3 and N("F32")["nslice"] == 1          # S < 4: the clamp to one slice
    assert N("F33")["q"] == 1 and N("F33")["per"] == 32
    assert [N(n)["S"] for n in ("F34_B15", "F34_B16", "F34_B17")] == [16, 17, 19] and N("F34_B16")["per"] == 16
    assert N("F47")["per"] == 2 and 2 * 15 == 30 and N("F48")["rem"] == 16
    assert [N(n)["RT"] for n in ("B1_RT1", "B1_RT2", "B1_RT3")] == [1, 2, 3] and all(SR.SHAPES[n][2] == 1 for n in ("B1_RT1", "B1_RT2", "B1_RT3"))
    assert [N(n)["RT"] for n in SR.COEF_CASES] == [1, 2, 3, 3]
    assert {SR.SHAPES[n][1] for n in SR.GEOMETRY} >= {4, 8, 12, 20, 32, 48, 56, 60}
    assert {N(n)["nslice"] for n in SR.GEOMETRY} >= {1, 2, 4}
    assert all(SR.in_envelope(*SR.SHAPES[n][:2]) for n in SR.GEOMETRY + SR.COEF_CASES)
    assert not any(SR.in_envelope(*SR.SHAPES[n][:2]) for n in SR.OUTSIDE)
    assert all(SR.in_envelope(*SR.PLAN_SHAPES[s]) for s in SR.PLAN_INSIDE) and not any(SR.in_envelope(*SR.PLAN_SHAPES[s]) for s in SR.PLAN_OUTSIDE)
    assert {SR.PLAN_SHAPES[s] for s in SR.PLAN_INSIDE} == {(34, 60), (34, 56), (16, 32), (17, 12), (48, 20), (1, 4)}
    assert SR.SHAPES["T15"][1] * 4 % 16 != 0 and SR.SHAPES["T61"][1] * 4 == 244 and SR.SHAPES["F49"][0] == 49
    assert SR.SHAPES[SR.SPECIALIZE_TWIN][:2] == (34, 60)
    # length sets: unsorted with ties, zero-length samples, both sides of step 8
    assert SR.lengths_of("ties", 60) == (5, 60, 2, 60, 5, 1, 59, 2, 60) and SR.lengths_of("zero", 60).count(0) == 2
    assert set(SR.lengths_of("l89", 60)) == {8, 9} and set(SR.lengths_of("ones", 60)) == {1} and set(SR.lengths_of("full", 12)) == {12}


@pytest.mark.parametrize("name", ["LIN_P19", "LIN_RT1"])
def test_lin_patterns(name):
    """1 + the last observed step, per sample: 0 (nothing observed), 1, 8, 9 (both sides of a 32-column chunk edge), T; one sensor
    unobserved in every sample"""
    c = SR.case(name)
    T, F = c["T"], c["F"]
    obs = c["src"][:, :, :F] != 0
    lin = [int(np.nonzero(obs[:, b].any(1))[0].max()) + 1 if obs[:, b].any() else 0 for b in range(c["B"])]
    assert lin[:5] == [0, 1, 8, 9, T] and all(l <= L for l, L in zip(lin, c["lengths"]))
    assert {(4 * l + 31) >> 5 for l in lin[:4]} == {0, 1, 2}
    assert not obs[:, :, 2].any() and obs[:, :, 0].any() and obs[:, :, 3].any()


def test_pe_reference_is_the_restatements():
    c = SR.case("F5")
    pe = O2.positional_encoding(torch.from_numpy(c["times"]), c["T"]).numpy()
    assert np.abs(SR.reference(c)["pe"] - pe).max() < 1e-6


def _small(ssum=None):
    return SR.make_case("small", 5, 7, (7, 3, 5), "dense", "padded", ssum=ssum)


def test_reference_equals_the_per_edge_restatement():
    """oracle/restatement.py observation_propagation per sample and per edge (the form test_sensor_stage_vs_oracle uses) in float64
    under autograd: the edge softmax into a target sums to 1, so the batched form's coefficient is ssum = 1."""
    F, T, d = 5, 7, 4
    c = _small(ssum=np.ones(F, np.float32))
    B, K = c["B"], c["K"]
    gs = (np.random.default_rng(1).random((F, F)) * (np.random.default_rng(2).random((F, F)) < 0.5)).astype(np.float32)
    ei_np, ew_np = O2.build_graph(gs)
    ei, ew = torch.from_numpy(ei_np), torch.from_numpy(ew_np).double()
    p = {n: torch.from_numpy(c[n]).double().requires_grad_(True) for n in SR.GRAD_NAMES}
    src = torch.from_numpy(c["src"]).double()
    h = torch.relu(torch.repeat_interleave(src[:, :, :F], d, dim=-1) * p["R_u"])
    cols = []
    for u in range(B):
        x = h[:, u, :].reshape(T, F, d).permute(1, 0, 2).reshape(F, K)
        x, a1 = O2.observation_propagation(x, ei, ew, p["W1"], p["b1"])
        x, _ = O2.observation_propagation(x, ei, a1.squeeze(-1), p["W2"], p["b2"])
        cols.append(x.view(F, T, d).permute(1, 0, 2).reshape(T, F * d))
    out = torch.stack(cols, dim=1)
    g = torch.autograd.grad(out, [p[n] for n in SR.GRAD_NAMES], torch.from_numpy(c["dz"][:, :, :F * d]).double())
    r = SR.reference(c)
    assert np.abs(r["z"] - out.detach().numpy()).max() <= 1e-12 * np.abs(r["z"]).max()
    for n, t in zip(SR.GRAD_NAMES, g):
        assert np.abs(r[n] - t.numpy()).max() <= 1e-12 * np.abs(r[n]).max(), n
    assert np.array_equal(r["mask"], O2.padding_mask(c["lengths"], T))


def test_gradients_equal_a_central_finite_difference():
    """loss = <z, dz>; 12 entries of every parameter, step 1e-6: far inside the gate margins, so the loss is smooth there"""
    c = _small()
    r = SR.reference(c)
    dz = c["dz"][:, :, :4 * c["F"]].astype(np.float64)
    assert min(np.abs(r["pre1"]).min(), np.abs(r["pre2"]).min()) > 1e-3
    rng = np.random.default_rng(0)
    h = 1e-6
    for n in SR.GRAD_NAMES:
        base = c[n].astype(np.float64)
        for flat in rng.choice(base.size, size=min(12, base.size), replace=False):
            vals = []
            for sgn in (+1.0, -1.0):
                q = base.copy()
                q.reshape(-1)[flat] += sgn * h
                vals.append(float((SR.evaluate(dict(c, **{n: q}))["z"] * dz).sum()))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - r[n].reshape(-1)[flat]) <= 1e-6 * np.abs(r[n]).max() + 1e-9, (n, int(flat), fd, r[n].reshape(-1)[flat])


@pytest.mark.parametrize("variant", sorted(SR.VARIANTS))
def test_wrong_references_miss_the_bounds(variant):
    kind, key = SR.VARIANTS[variant]
    c = _case(kind, key)
    if variant == "drop_last_kc":
        assert c["K"] % 32 == 16
    if variant == "leftover_row":
        assert c["F"] % 32 != 0
    ref, wrong = SR.compared(c, SR.reference(c)), SR.compared(c, SR.reference(c, variant))
    worst, at = 0.0, None
    for name in ref:
        e, bound = SR.error_of(name, wrong[name], ref[name], "bf16x3")       # the wider of the two modes' bounds
        if e / bound > worst:
            worst, at = e / bound, name
    print("%s on %s: %s moves by %.1f x its bound" % (variant, c["name"], at, worst))
    assert worst > 10.0, (variant, worst)
