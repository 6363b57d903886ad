"""CPU: conditions on the float64 reference of the use_beta graph operator (tests/beta_operator_ref.py) alone -- what makes
tests/test_beta_operator_float64_gpu.py worth running:

  1. every case keeps adjacent scores apart by its margin and away from zero (pruning is decisive in fp32), and nothing is NaN;
  2. the reference is the operator: torch float64 autograd on oracle/restatement.py observation_propagation_beta (stable argsort)
     at four small cases to 1e-10, with the alpha cotangent and under a mask, and a central finite difference at one;
  3. the ceilings are reachable: the float32 yardstick stays under them in every group;
  4. a wrong kernel fails: each of nine variants misses the working bound of some compared tensor by at least 10 x;
  5. the host mask helper reproduces known quads of SITE_EDGE_COEFF."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import restatement as O2
from tests import beta_operator_ref as BR
from tests import rng_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the conditions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in BR.ALL_CASES if n != "TIE"])
def test_pruning_is_decisive(name):
    c = BR.case(name)
    gap, zero, need = BR.conditions(c)
    assert need >= 8.0 * BR.apriori_score_bound(c["T"])
    assert gap >= need and zero >= need, (name, gap, zero, need)
    if name == "NOOUT":                                       # the graph is what the table says
        src, tgt = c["ei"]
        kept = BR.reference(name, "plain")["kept"]
        assert len(set(range(c["N"])) - set(src.tolist())) >= c["N"] // 3
        assert (tgt == 0).sum() > 0 and 0 not in src and not np.isin(np.nonzero(tgt == 0)[0], kept).any()
    if name == "DUP":
        assert np.array_equal(c["ei"][:, :c["E"] // 2], c["ei"][:, c["E"] // 2:])


def test_tie_case_is_exact_and_ordered_by_edge_id():
    c = BR.case("TIE")
    for dt in (np.float32, np.float64):
        r = BR.evaluate(c, "plain", dt)
        assert np.array_equal(r["alpha"], np.full((c["B"], c["Kk"]), 0.25, dt)) and np.array_equal(r["beta"], np.full_like(r["beta"], 0.25))
        assert np.array_equal(r["kept"], np.broadcast_to(np.arange(c["Kk"]), (c["B"], c["Kk"])))
        assert np.array_equal(r["ei_out"][0], c["ei"][:, :c["Kk"]])


@pytest.mark.parametrize("mode", BR.MODES)
def test_reference_is_finite_and_shaped(mode):
    for name in BR.ALL_CASES:
        c, r = BR.case(name), BR.reference(name, mode)
        for t in BR.COMPARED:
            assert np.isfinite(r[t]).all(), (name, t)
        assert r["kept"].shape == (c["B"], c["E"] // 2) and r["dw"].shape == (c["B"], c["E"])
        pruned = np.ones((c["B"], c["E"]), dtype=bool)
        np.put_along_axis(pruned, r["kept"].astype(np.int64), False, axis=1)
        assert (r["dw"][pruned] == 0).all(), name                                 # dw of pruned edges is exactly 0
        if c["Kk"] == 0:
            assert not r["out"].any() and not r["dV"].any() and not r["dH"].any() and not r["dmap"].any()


# ---- 2. the reference is the operator -----------------------------------------------------------------------------------------------------
def _torch_autograd(c, mode, monkeypatch):
    """O2.observation_propagation_beta per sample in float64 with x = I (so lin_value's weight is V^T and increase_dim's H^T), its
    edge_softmax multiplied by the mask: outputs and the gradients of sum out * dout [+ sum alpha * dalpha]."""
    B, N, T, K, E, Kk = c["B"], c["N"], c["T"], c["K"], c["E"], c["Kk"]
    dbl = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    real_argsort, real_softmax = torch.argsort, O2.edge_softmax
    cur = {}
    monkeypatch.setattr(torch, "argsort", lambda t, *a, **k: real_argsort(t, *a, **dict(k, stable=True)))
    monkeypatch.setattr(O2, "edge_softmax", lambda g, index, n: real_softmax(g, index, n) * cur["scale"])
    keep = BR.keep_mask(c) if mode == "drop" else None
    mw = dbl(c["map_w"]).requires_grad_(True)
    res = dict(out=[], alpha=[], ei_out=[], dV=[], dH=[], dw=[])
    loss, leaves = 0.0, []
    for b in range(B):
        Vt = dbl(c["V"][b].T).requires_grad_(True)                                # [K, N]
        Ht = dbl(c["H"][b].reshape(N, T * 32).T).requires_grad_(True)             # [T 32, N]
        ew = dbl(c["w"][b if c["w_ps"] else 0]).requires_grad_(True)
        kept = BR.reference(c["name"], mode)["kept"][b].astype(np.int64)
        cur["scale"] = dbl(keep[b, kept].reshape(Kk, K)) / (1.0 - BR.P_DROP) if keep is not None else 1.0
        y, (ei, a) = O2.observation_propagation_beta(torch.eye(N, dtype=torch.float64), dbl(c["p_t"][b if c["pt_ps"] else 0]),
                                                     torch.from_numpy(c["ei"]), ew, Vt, torch.zeros(K, dtype=torch.float64), Ht,
                                                     torch.zeros(T * 32, dtype=torch.float64), mw, BR.D_OB)
        loss = loss + (y * dbl(c["dout"][b])).sum()
        if mode != "plain":
            loss = loss + (a * dbl(c["dalpha"][b])).sum()
        res["out"].append(y.detach().numpy()); res["alpha"].append(a.detach().numpy()); res["ei_out"].append(ei.numpy())
        leaves.append((Vt, Ht, ew))
    grads = torch.autograd.grad(loss, [mw] + [t for l in leaves for t in l])
    monkeypatch.undo()
    res["dmap"] = grads[0].numpy()
    for b in range(B):
        gV, gH, gw = grads[1 + 3 * b: 4 + 3 * b]
        res["dV"].append(gV.numpy().T); res["dH"].append(gH.numpy().T); res["dw"].append(gw.numpy())
    return {k: (np.stack(v) if isinstance(v, list) else v) for k, v in res.items()}


@pytest.mark.parametrize("name,mode", [("N2", "plain"), ("SELF", "alpha"), ("E3", "drop"), ("S_WP_PS", "drop"), ("KK63", "alpha")])
def test_reference_equals_torch_autograd_on_the_restatement(name, mode, monkeypatch):
    c = dict(BR.case(name))
    c["V"] = c["V"] + np.float32(0.125)                       # relu(V) = V with slope 1 everywhere (V is a relu's output: >= 0)
    ref = BR.evaluate(c, mode)
    got = _torch_autograd(c, mode, monkeypatch)
    assert np.array_equal(got["ei_out"], ref["ei_out"])
    for t in ("out", "alpha", "dV", "dH", "dmap", "dw"):
        scale = max(float(np.abs(ref[t]).max()), ref["scale"].get(t, 0.0), 1e-30)
        assert float(np.abs(got[t] - ref[t]).max()) <= 1e-10 * scale, (t, float(np.abs(got[t] - ref[t]).max()), scale)


def test_reference_gradients_equal_a_central_finite_difference():
    """d/dh of sum out * dout + sum alpha * dalpha along one random direction of (V, H, map_w, w) against <gradient, direction>, under
    the mask; h = 1e-6 keeps the pruning order (the margin is 1e-2)."""
    base = BR.case("ONESRC")
    c = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v) for k, v in base.items()}
    rng = np.random.default_rng(5)
    d = {k: rng.standard_normal(c[k].shape) for k in ("V", "H", "map_w", "w")}
    ref = BR.evaluate(c, "drop")

    def loss(h):
        r = BR.evaluate(dict(c, **{k: c[k] + h * d[k] for k in d}), "drop")
        assert np.array_equal(r["kept"], ref["kept"])
        return float((r["out"] * c["dout"]).sum() + (r["alpha"] * c["dalpha"]).sum())

    want = float((ref["dV"] * d["V"]).sum() + (ref["dH"].reshape(d["H"].shape) * d["H"]).sum() + (ref["dmap"] * d["map_w"]).sum() +
                 (ref["dw"] * d["w"]).sum())
    h = 1e-6
    fd = (loss(h) - loss(-h)) / (2 * h)
    assert abs(fd - want) <= 1e-7 * abs(want), (fd, want)


# ---- 3. the ceilings are reachable --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(BR.GROUPS))
def test_float32_yardstick_is_under_the_ceilings(group):
    for mode in BR.MODES:
        y = BR.yardstick(group, mode)
        print("beta64 yardstick %s %s: %s" % (group, mode, ", ".join("%s %.2e (%s)" % (t, y[t][0], y[t][1]) for t in BR.COMPARED)))
        for t in BR.COMPARED:
            assert BR.YARD_FACTOR * y[t][0] <= BR.ceiling_of(t, mode), (group, mode, t, y[t])


# ---- 4. a wrong kernel must fail ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(BR.VARIANTS))
def test_a_wrong_kernel_misses_a_working_bound_tenfold(variant):
    name, mode = BR.VARIANTS[variant]
    c = BR.case(name)
    if variant == "drop_pos64":
        assert c["Kk"] == 65
    if variant == "kk_ceil":
        assert c["E"] % 2 == 1
    if variant == "skip_chunk_last":
        assert c["T"] > BR.CHUNK_TC and c["T"] % BR.CHUNK_TC
    if variant == "pad_key":
        assert c["E"] == 4097
    if variant == "w_stride0":
        assert c["w_ps"] and c["B"] > 1
    m = BR.variant_margin(variant)
    print("beta64 variant %s on %s/%s: %.3g x the bound" % (variant, name, mode, m))
    assert m >= 10.0, (variant, m)


def test_the_reference_itself_meets_every_bound():
    """margin 0 for the unmodified reference through the same comparison (the variants' figures are not an artefact of compare())"""
    for name, mode in set(BR.VARIANTS.values()):
        rows, lists_ok = BR.compare(name, mode, BR.evaluate(BR.case(name), mode))
        assert lists_ok and all(e == 0 for _, e, _ in rows)


# ---- 5. the mask helper -------------------------------------------------------------------------------------------------------------------
def _header_constant(path, pattern):
    m = re.search(pattern, open(os.path.join(ROOT, "raindrop_amd", "csrc", path)).read())
    assert m, (path, pattern)
    return m


def test_edge_coeff_helper_is_the_header_s_numbering():
    """Site and numbering as the headers state them (rd_rng.h enum DropSite, rd_graph_beta.h beta_drop_base), known quads through
    the Threefry statement tests/test_rng_ref_host.py ties to the published vectors."""
    assert int(_header_constant("rd_rng.h", r"SITE_EDGE_COEFF\s*=\s*(\d+)").group(1)) == R.SITE_EDGE_COEFF
    _header_constant("rd_graph_beta.h", r"return \(\(uint64_t\)b \* \(uint64_t\)E \+ \(uint64_t\)e\) \* \(uint64_t\)T;")
    B, E, T, p, seed = 3, 7, 5, 0.3, (9 << 32) | 1234
    q = R.edge_coeff_quad(B, E, T)
    assert q.shape == (B, E, T) and np.array_equal(q.reshape(-1), np.arange(B * E * T))      # [B, E, T] order, injective
    keep = R.edge_coeff_keep(seed, B, E, T, p)
    assert keep.shape == (B, E, T, 4) and keep.dtype == bool
    for b, e, t in ((0, 0, 0), (2, 6, 4), (1, 3, 2)):
        quad = (b * E + e) * T + t
        x0, x1 = R.threefry2x32_13(quad, R.SITE_EDGE_COEFF << 16, 1234, 9)
        u = np.array([int(x0) & 0xFFFF, int(x0) >> 16, int(x1) & 0xFFFF, int(x1) >> 16], dtype=np.float32) / np.float32(65536.0)
        assert np.array_equal(keep[b, e, t], u >= np.float32(p))
    # the zero counter / zero key vector of Random123 (0x9d1c5ec6, 0x8bd50731) is quad 0 of site 0 under seed 0
    assert np.array_equal(R.uniform4(0, 0, 0), np.array([0x5ec6, 0x9d1c, 0x0731, 0x8bd5], dtype=np.float32) / np.float32(65536.0))
    frac = R.edge_coeff_keep(77, 4, 64, 32, p).mean()
    assert abs(frac - (1 - p)) < 4 * np.sqrt(p * (1 - p) / (4 * 64 * 32 * 4))


# ---- 6. the route query (needs no device) -------------------------------------------------------------------------------------------------
def _route(c, mode):
    import ctypes
    from raindrop_amd import _lib
    bits = ctypes.c_uint32(0)
    _lib.call("rd_debug_graph_beta_route", c["B"], c["N"], c["T"], c["E"], int(mode != "plain"), int(mode == "drop"), ctypes.byref(bits))
    return {n for i, n in enumerate(_lib.BETA_ROUTE_BITS) if bits.value >> i & 1}, bits.value >> 8


def test_route_query_against_the_hand_written_table(monkeypatch):
    """rd_debug_graph_beta_route (the functions the launch sites call) against the case table: which form, STAGE_V at the capacity
    edge, the backward's chunk per mode (tests/beta_operator_ref.py ROUTE_TC, written out by hand), V1 and the forced workspace form."""
    monkeypatch.delenv("RD_BETA_V1", raising=False)
    monkeypatch.delenv("RD_BETA_LARGE", raising=False)
    for name in BR.ALL_CASES:
        c = BR.case(name)
        for k, mode in enumerate(BR.MODES):
            bits, tc = _route(c, mode)
            if name in BR.WORKSPACE_CASES:
                assert not bits and tc == 0, (name, mode, bits, tc)
                continue
            assert {"fwd_lds", "bwd_lds"} <= bits and "v1" not in bits, (name, mode, bits)
            assert tc == BR.ROUTE_TC.get(name, (c["T"],) * 3)[k], (name, mode, tc)
            assert ("stage_v" in bits) == BR.STAGE_V.get(name, "stage_v" in bits)
    assert {(n, m) for n, m in BR.RAGGED} >= {("CAP_T7", "plain"), ("CAP_T7", "alpha"), ("CAP_T7", "drop"), ("CAP_T5", "alpha")}
    assert _route(BR.case(BR.CHUNK_CASE), "plain")[1] == BR.CHUNK_TC
    monkeypatch.setenv("RD_BETA_V1", "1")
    for name in BR.V1_CASES:
        bits, tc = _route(BR.case(name), "plain")
        assert {"fwd_lds", "bwd_lds", "v1"} <= bits and "stage_v" not in bits and tc == BR.ROUTE_TC_V1.get(name, BR.case(name)["T"])
    monkeypatch.delenv("RD_BETA_V1")
    monkeypatch.setenv("RD_BETA_LARGE", "1")
    for name in BR.FORCED_LARGE:
        assert _route(BR.case(name), "plain") == (set(), 0)
    monkeypatch.delenv("RD_BETA_LARGE")
    import ctypes
    from raindrop_amd import _lib
    assert _lib.load().rd_debug_graph_beta_route(2, 0, 4, 10, 0, 0, ctypes.byref(ctypes.c_uint32(0))) == -1      # bad dims
