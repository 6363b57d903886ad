"""CPU: the case table of tests/panel_ref.py -- the route of every product of every case in every forced panel form against
rd_debug_gemm_route (the library loads without a device; RD_PANEL_WIDE / RD_PANEL_PC are read per call), and, on the float64
reference alone, that every gate is decisive and that the bounds of tests/test_panel_float64_gpu.py see an edge error."""
import numpy as np
import pytest

from raindrop_amd import _lib
from tests import panel_ref as PR
from tests import sensor_stage_ref as SR
from tests import test_gemm_route_host as GR

BT = ("a_aligned", "btiles")


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    for k in GR.READ_ONCE + GR.PER_CALL + ("RD_K1_FUSED",):
        monkeypatch.delenv(k, raising=False)
    yield
    _lib.call("rd_set_precision", GR.BF16X3)


def _force(monkeypatch, form):
    for k, v in PR.FORCE[form].items():
        monkeypatch.setenv(k, v)


def _stage_products(name):
    """the four panel candidates of the generic sensor stage: both forward products (the second scatters, on a plan by the plan)
    and both input gradients (weights read transposed; the tiles are given either way)"""
    M, K = PR.dims(name)
    scatter = ("scatter", "plan") if PR.CASES[name][3] == "plan" else ("scatter",)
    return [GR.product(M, K, K, flags=BT), GR.product(M, K, K, flags=BT + scatter),
            GR.product(M, K, K, sb=(1, K), flags=BT), GR.product(M, K, K, sb=(1, K), flags=BT)]


@pytest.mark.parametrize("mode", (GR.BF16X3, GR.BF16), ids=["bf16x3", "bf16"])
@pytest.mark.parametrize("form", sorted(PR.FORMS))
def test_route_table(form, mode, monkeypatch):
    _lib.call("rd_set_precision", mode)
    _force(monkeypatch, form)
    env = dict(PR.FORCE[form])
    for name in PR.CASES:
        want = PR.launch(name, form)
        assert want[0] == PR.PANEL_NAME[form]
        for p in _stage_products(name):
            r = GR.route(p)
            assert (r["name"], r["grid"], r["lds"]) == (want[0], (want[1], 1, 1), want[2]), (name, form, r)
            assert GR.restate(p, mode, env)[0] == want[0], (name, form)
    for i, (M, N, K) in enumerate(PR.enc_products()):        # the encoder layer's: four forward, four input gradients, all K >= 64
        p = GR.fwd(M, N, K, flags=BT) if i < 4 else GR.product(M, N, K, sb=(1, N), flags=BT)
        assert K >= 64 and GR.route(p)["name"] == PR.PANEL_NAME[form], (M, N, K, form)


def test_unforced_route_is_the_small_form_and_fp32_has_no_panel():
    """why the forms have to be forced: the cost model takes the 64 x 128 form at every shape of the table"""
    for name in PR.CASES:
        for p in _stage_products(name):
            assert GR.route(p)["name"] == "k_gemm_panel", name
    _lib.call("rd_set_precision", GR.FP32)
    assert GR.route(_stage_products("K68")[0])["name"] == "k_gemm"


def test_weight_gradients_are_no_panel_candidates(monkeypatch):
    """the stage's weight gradients reduce over the M rows with row sums: a tiled split-K name under every forced form -- the names
    the GPU module allows next to the panel name in a backward's log"""
    for form in PR.FORMS:
        with monkeypatch.context() as m:
            for k, v in PR.FORCE[form].items():
                m.setenv(k, v)
            for name in PR.CASES:
                M, K = PR.dims(name)
                for second in (False, True):
                    assert GR.route(GR.wgrad(M, K, K, second=second))["name"].startswith(PR.X3), (name, form)


def test_the_table_holds_every_condition():
    cond = {n: PR.conditions(n) for n in PR.CASES}
    assert cond["K64"] == dict(nch=1, tail=0, nkc=2)
    assert cond["K68"] == dict(nch=2, tail=4, nkc=3) and 68 % 16 == 4
    assert cond["K96"] == dict(nch=2, tail=32, nkc=3)
    assert cond["K100"] == dict(nch=2, tail=36, nkc=4)
    assert cond["K128"] == dict(nch=2, tail=0, nkc=4)
    assert cond["K160"] == dict(nch=3, tail=32, nkc=5)
    assert cond["K192"] == dict(nch=3, tail=0, nkc=6)
    assert cond["K260"]["nch"] == 5 and PR.dims("K260")[1] > 256 and PR.dims("K260")[1] % 256 == 4
    assert [PR.dims("M%d" % m)[0] for m in (1, 63, 64, 65, 127, 128, 129)] == [1, 63, 64, 65, 127, 128, 129]
    for name, (M, K, counts) in PR.TILE_COUNTS.items():
        assert PR.dims(name) == (M, K) and tuple(PR.tiles(name, f) for f in ("small", "wide", "pc")) == counts, name
    assert all(t < 8 for t in PR.TILE_COUNTS["M1"][2])
    assert all(t > 8 and t % 8 for t in PR.TILE_COUNTS["TILES"][2]) and PR.TILE_COUNTS["K260"][2][0] == 9
    for name in PR.CASES:                                    # inside the fused envelope the GPU module sets RD_K1_FUSED=0
        F, T, _, _ = PR.CASES[name]
        assert PR.case(name)["envelope"] == SR.in_envelope(F, T)
    assert PR.case("COEF")["coef"].shape == (2, 5, 34) and PR.case("PLAN")["layout"] == "plan"
    L = PR.case("PLAN")["lengths"]
    assert 1 in L and PR.CASES["PLAN"][1] in L
    sub = PR.subset_case(PR.case(PR.ROW_SUBSET["case"]), PR.ROW_SUBSET["samples"])
    assert PR.dims(PR.ROW_SUBSET["case"])[0] > 128 and sub["B"] * sub["F"] == 68 and sub["b1"] is PR.case(PR.ROW_SUBSET["case"])["b1"]


@pytest.mark.parametrize("name", sorted(PR.CASES))
def test_gates_are_decisive_and_the_bounds_bite(name):
    c = PR.case(name)
    r = SR.reference(c)
    for layer in ("pre1", "pre2"):
        assert float(np.abs(r[layer]).min()) >= SR.GATE_MARGIN, (name, layer, float(np.abs(r[layer]).min()))
        if c["B"] * c["F"] >= 8:
            assert 0.25 <= float((r[layer] > 0).mean()) <= 0.75, (name, layer)
    for what, m in PR.edge_margins(c).items():
        assert m > 1.0, (name, what, m)
    for g in SR.GRAD_NAMES:                                  # a gradient that is all zero would be compared with nothing
        assert float(np.abs(r[g]).max()) > 0.0, (name, g)


def test_encoder_case_has_no_gate_near_zero():
    c = PR.enc_case()
    assert (c["D"], c["nhid"], c["T"] * c["B"]) == (84, 136, 165)
    for p in PR.ENC_P:
        ref, pre = PR.enc_reference(p)
        assert pre.shape == (33, 5, 136) and float(np.abs(pre).min()) >= SR.GATE_MARGIN, (p, float(np.abs(pre).min()))
        assert 0.25 <= float((pre > 0).mean()) <= 0.75
        assert set(ref) == set(("y", "x") + PR.DR.ENC_NAMES)
    a, b = PR.enc_reference(0.0)[0]["y"], PR.enc_reference(PR.DR.P_DROP)[0]["y"]
    assert float(np.abs(a - b).max()) > 20 * PR.DR.enc_bound("bf16x3")("y")[1]      # the masks matter at the output's bound


# ---- the one-product bf16 mode: its own biases, its own reference, bounds from the CPU alone ------------------------------------------
@pytest.mark.parametrize("name", sorted(PR.CASES))
def test_bf16_mode_gates_are_decisive_and_its_bounds_bite(name):
    c, r = PR.case16(name), PR.reference16(name)
    for layer in ("pre1", "pre2"):
        assert float(np.abs(r[layer]).min()) >= SR.GATE_MARGIN, (name, layer, float(np.abs(r[layer]).min()))
    # the edges against the LARGEST element-wise bound of the case (split-bf16 term + the largest one-flip term)
    worst = float(r["zflip"].max())
    z, F, T, B = r["z"], c["F"], c["T"], c["B"]
    bound = SR.Z_ABS["bf16x3"] * SR.z_scale(z) + worst
    full = np.flatnonzero(c["lengths"] == T)
    steps = int(c["lengths"][B - 1])
    assert float(np.abs(PR.evaluate16(c, drop_last_k=True)["z"] - z).max()) > bound, (name, "last reduction index", bound)
    assert float(np.abs(z[:steps, B - 1, SR.D_OB * (F - 1):]).max()) > bound, (name, "last row", bound)
    assert float(np.abs(z[T - 1][full]).max()) > bound, (name, "last step's columns", bound)
    ref64 = SR.reference(PR.case(name))
    assert float(np.abs(ref64["z"]).max()) > 0 and all(float(np.abs(r[g]).max()) > 0 for g in SR.GRAD_NAMES)


def test_pairwise_yardstick_is_a_summation_order_figure():
    total, per = PR.pair_sum()
    assert set(per) == set(PR.CASES) and total == 4.0 * max(per.values())
    assert per["K64"] == 0.0                                 # one chunk: both orders are the same sum
    assert 0.0 < total < SR.Z_ABS["bf16x3"], total            # fp32 order effects lie far below the split-bf16 bound
