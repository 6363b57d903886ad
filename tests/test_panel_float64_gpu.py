"""GPU: the three panel products of raindrop_amd/csrc/rd_gemm.hip -- k_gemm_panel (64 x 128, two wave groups on even / odd 64-k
chunks), k_gemm_panel_wide (128 x 256) and k_gemm_panel_pc (128 x 128, producer / consumer waves) -- against float64 across the
places the cost model never selects at the suite's other shapes: one chunk (K = 64: the small form's second group owns nothing),
odd chunk counts, K tails of 4, 32 and 36 (the last chunk's second weight tile missing or 4 deep), N % 16 != 0, N < TN and a ragged
second column block, M = 1, 63 .. 65, 127 .. 129 (the second half-tile of the 128-row forms empty, one row deep, full), one tile on
eight workgroups and tile counts that are no multiple of 8, per-row scales, and the scatter on a token plan.  Every case runs in
EVERY form, forced through RD_PANEL_WIDE / RD_PANEL_PC (read per call).  Cases and routes: tests/panel_ref.py; reference, inputs and
bounds: tests/sensor_stage_ref.py (decisive gates; z 2e-5 x 6, gradients 2e-4 of the float64 max-norm, no entry exempt);
tests/test_panel_ref_host.py holds the route table to rd_debug_gemm_route and shows that the bounds bite.

Every run reads the launch log.  A forward's k_gemm* names must be exactly the forced form's; a backward's panel names likewise,
and the only tiled names next to it are those of the weight gradients (split-K with row sums: no panel candidate).  A case that
falls off its form fails.

  1. the generic sensor stage (ops.sensor_stage_fwd_raw / sensor_stage_bwd_raw, RD_K1_FUSED=0 inside the fused envelope) per case
     and form: z, PE, the mask and the five gradients;
  2. row independence: the same call on two of the five samples (68 of 170 rows) gives the same BITS in their z rows -- an output
     element is one fixed sequence of MFMA steps over its own row of A, whichever rows share its tile;
  3. write-side guard: rd_msgpass_fwd with ldz > 4 F, a sentinel in the padding columns and behind the last row, on the padded
     layout and on a token plan (rows of steps >= length keep the sentinel);
  4. one encoder layer at D = 84, nhid = 136, T = 33, B = 5 under RD_PANEL_WIDE=1 and under RD_PANEL_PC=1, with p = 0 and p = 0.2:
     the dropout + residual and posmask + cscale epilogues of those two forms, against oracle/restatement.py encoder_layer in
     float64 with the host masks of tests/dropout_ref.py at the bounds of test_encoder_layer_dropout_vs_float64.

  5. the one-product bf16 mode (rd_set_precision(2)), every case in all three forms on the same inputs: each form against the
     float64 sums of bf16-rounded operands (panel_ref.evaluate16, biases gap-placed in that arithmetic) -- z element by element at
     the split-bf16 bound plus one flipped bf16 rounding of Y1, gradients at the relative-L2 bound of test_sensor_stage_vs_oracle
     -- and the forms pairwise: PE and mask bit-equal, z within 4 x the CPU's fp32 summation-order difference (panel_ref.pair_sum)
     plus the same one-flip term.  No figure of these bounds comes from the device.

Every measured error is printed (-s) as `panel64 <kind> <case> <form> <mode>: <tensor> <error>, ...`; tools/panel_errors_json.py
turns that output into profiles/panel_float64_errors.json."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from tests import dropout_ref as DR
from tests import panel_ref as PR
from tests import sensor_stage_ref as SR
from tests import test_gemm_route_host as GR

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODE = PR.MODE
COMPARED = ("z", "pe") + SR.GRAD_NAMES
SENTINEL = -12345.0
GUARD = 4096                                             # floats behind the last row of z
ALL_PANELS = set(PR.PANEL_NAME.values())


def _L():
    from raindrop_amd import _lib
    return _lib


def _hooks():
    lib = _L().load()
    on, read = lib.rd_debug_launch_log, lib.rd_debug_launch_log_read
    on.argtypes, on.restype = [ctypes.c_int], None
    read.argtypes, read.restype = [ctypes.c_char_p, ctypes.c_size_t], ctypes.c_size_t
    return on, read


@pytest.fixture(autouse=True)
def _process_wide_settings_handed_back():
    """Before and after each test: split-bf16 arithmetic, launch log off, no token plan registered.  A device error ends the session:
    nothing more is started on a GPU that has faulted."""
    on, _ = _hooks()
    _L().call("rd_set_precision", 1)
    _L().call("rd_set_token_plan", None)
    try:
        yield
    finally:
        on(0)
        _L().call("rd_set_token_plan", None)
        _L().call("rd_set_precision", 1)
        try:
            torch.cuda.synchronize()
        except Exception as e:                              # noqa: BLE001 -- any HIP error here is a fault of the device
            pytest.exit("device error after a panel case: %s" % e, returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _hand_back_device_memory():
    """tests/test_step_launches_gpu.py names buffers by the order in which their addresses first appear: leave no garbage behind."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _logged(fn):
    """run fn with the launch log on -> the distinct names the launch sites reported"""
    on, read = _hooks()
    buf = ctypes.create_string_buffer(1 << 12)
    on(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        need = read(buf, len(buf))
        on(0)
    assert need < len(buf)
    return {n for n in buf.value.decode().split("\n") if n}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _force(monkeypatch, form, envelope=False):
    for k in ("RD_PANEL_WIDE", "RD_PANEL_PC", "RD_K1_FUSED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PR.FORCE[form].items():
        monkeypatch.setenv(k, v)
    if envelope:
        monkeypatch.setenv("RD_K1_FUSED", "0")


def _assert_forward_log(names, form, what):
    gemms = {n for n in names if n.startswith("k_gemm")}
    assert gemms == {PR.PANEL_NAME[form]}, (what, form, sorted(names))


def _assert_backward_log(names, form, what, wgrads):
    """wgrads: the (M, N_out, K_in) weight-gradient products of the call -- the only tiled names a backward may log"""
    assert names & ALL_PANELS == {PR.PANEL_NAME[form]}, (what, form, sorted(names))
    allowed = {GR.route(GR.wgrad(*w, second=s))["name"] for w in wgrads for s in (False, True)}
    assert {n for n in names if n.startswith(PR.X3)} <= allowed, (what, form, sorted(names), sorted(allowed))


def _plan_of(c, shp):
    """a token plan of c's lengths on the device, checked against the host's"""
    L = _L()
    lib = L.load()
    sp = ctypes.byref(shp)
    B = c["B"]
    lengths = _dev(c["lengths"])
    plan = torch.zeros(max(int(lib.rd_token_plan_bytes(sp)) // 4, 64), dtype=torch.int32, device=DEV)
    L.call("rd_token_plan", sp, ctypes.c_void_p(lengths.data_ptr()), ctypes.c_void_p(plan.data_ptr()), None, 0,
           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    h = plan.cpu().numpy()
    pl = c["plan"]
    assert h[0] == pl["mlive"] and np.array_equal(h[8:8 + B + 1], pl["off"]) and np.array_equal(h[9 + B:9 + 2 * B], pl["rank"])
    return plan


def _run(c, form, monkeypatch, prec=1):
    """The stage forward + backward on c's layout in the forced form -> {z, pe, mask, five gradients} as numpy (z / pe on live rows
    in plan order where the case runs on a plan).  Both launch logs are checked here."""
    from raindrop_amd import ops
    L = _L()
    T, B, F, D = c["T"], c["B"], c["F"], c["D"]
    _force(monkeypatch, form, c["envelope"])
    shp = L.shape(B, T, F, SR.D_OB)
    L.call("rd_set_precision", prec)
    src, times, lengths = _dev(c["src"]), _dev(c["times"]), _dev(c["lengths"])
    ts = ops.timescales(T).to(DEV)
    ssum, R_u, W1, b1, W2, b2 = (_dev(c[n]) for n in ("ssum", "R_u", "W1", "b1", "W2", "b2"))
    coef = None if c["coef"] is None else _dev(c["coef"])
    on_plan = c["layout"] == "plan"
    plan = None
    if on_plan:
        ml = c["plan"]["mlive"]
        dz = torch.full((T * B, D), float("nan"), device=DEV)              # rows >= M_live: never to be read
        dz[:ml] = _dev(SR.to_plan(c["dz"], SR.starts_of(c["plan"]), c["lengths"], ml))
        dz = dz.view(T, B, D)
        plan = _plan_of(c, shp)
    else:
        dz = _dev(c["dz"])
    out = {}

    def with_plan(fn):
        def go():
            if on_plan:
                L.call("rd_set_token_plan", ctypes.c_void_p(plan.data_ptr()))
            try:
                fn()
            finally:
                if on_plan:
                    L.call("rd_set_token_plan", None)
        return go

    def fwd():
        out["z"], out["mask"], out["saved"] = ops.sensor_stage_fwd_raw(src, times, lengths, ts, ssum, R_u, W1, b1, W2, b2, shp, 0.0,
                                                                        0, coef)

    def bwd():
        out["g"] = ops.sensor_stage_bwd_raw(src, R_u, W1, W2, ssum, out["saved"], out["z"], dz, shp, 0.0, coef)

    what = c["name"]
    _assert_forward_log(_logged(with_plan(fwd)), form, what)
    _assert_backward_log(_logged(with_plan(bwd)), form, what, [(B * F, c["K"], c["K"])])
    z = out["z"]
    if on_plan:
        z = z.view(T * B, D)[:c["plan"]["mlive"]]
    zc = z.cpu().numpy()
    got = dict(z=zc[..., :F * SR.D_OB], pe=zc[..., F * SR.D_OB:], mask=out["mask"].cpu().numpy())
    got.update((n, t.cpu().numpy()) for n, t in zip(SR.GRAD_NAMES, out["g"]))
    return got


def _compare(kind, c, form, got):
    """print every tensor's error, then hold each to its bound; the mask bit for bit"""
    ref = SR.reference(c)
    cmp_ = SR.compared(c, ref)
    bad, figs = [], []
    for name in COMPARED:
        e, bound = SR.error_of(name, got[name], cmp_[name], MODE)
        figs.append("%s %.2e" % (name, e))
        if not (np.isfinite(got[name]).all() and e <= bound):
            bad.append((name, e, bound))
    print("panel64 %s %s %s %s: %s" % (kind, c["name"], form, MODE, ", ".join(figs)))
    assert np.array_equal(got["mask"], ref["mask"]), "mask"
    assert not bad, (kind, c["name"], form, bad)


# ---- 1. every case in every form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(PR.FORMS))
@pytest.mark.parametrize("name", list(PR.CASES))
def test_panel_forms_vs_float64(name, form, monkeypatch):
    c = PR.case(name)
    _compare("stage", c, form, _run(c, form, monkeypatch))


# ---- 2. row independence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(PR.FORMS))
def test_rows_do_not_depend_on_their_neighbours(form, monkeypatch):
    """Five samples (170 rows: two or three row blocks, the last ragged) against samples 1 and 3 alone (68 rows: other row blocks,
    other neighbours, another half-tile) in the same form: the z rows of those samples bit for bit."""
    c = PR.case(PR.ROW_SUBSET["case"])
    idx = list(PR.ROW_SUBSET["samples"])
    full = _run(c, form, monkeypatch)
    part = _run(PR.subset_case(c, idx), form, monkeypatch)
    for k in ("z", "pe"):
        a, b = part[k], full[k][:, idx]
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (form, k, float(np.abs(a - b).max()))
    assert float(np.abs(part["z"]).max()) > 0.0


# ---- 3. write-side guard -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(PR.FORMS))
@pytest.mark.parametrize("name", PR.GUARD_CASES)
def test_nothing_is_written_outside_z(name, form, monkeypatch):
    """rd_msgpass_fwd with ldz = 4 F + 8: the eight padding columns of every row and GUARD floats behind the last row keep the
    sentinel; on a token plan so do the rows behind the last live one (steps >= length have no row)."""
    L = _L()
    lib = L.load()
    c = PR.case(name)
    T, B, F = c["T"], c["B"], c["F"]
    W = F * SR.D_OB
    ldz = W + 8
    _force(monkeypatch, form, c["envelope"])
    shp = L.shape(B, T, F, SR.D_OB)
    sp = ctypes.byref(shp)
    P = lambda t: ctypes.c_void_p(t.data_ptr())                              # noqa: E731
    src, ssum, R_u, W1, b1, W2, b2 = (_dev(c[n]) for n in ("src", "ssum", "R_u", "W1", "b1", "W2", "b2"))
    nbytes = int(lib.rd_msgpass_saved_bytes(sp))
    saved = torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    buf = torch.full((T * B * ldz + GUARD,), SENTINEL, device=DEV)
    on_plan = c["layout"] == "plan"
    plan = _plan_of(c, shp) if on_plan else None

    def go():
        if on_plan:
            L.call("rd_set_token_plan", P(plan))
        try:
            L.call("rd_msgpass_fwd", sp, P(src), P(R_u), P(W1), P(b1), P(W2), P(b2), P(ssum), 0.0, 0, P(buf), ldz, P(saved), nbytes,
                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        finally:
            if on_plan:
                L.call("rd_set_token_plan", None)

    _assert_forward_log(_logged(go), form, name)
    h = buf.cpu().numpy()
    assert (h[T * B * ldz:] == SENTINEL).all(), "written behind the last row"
    rows = h[:T * B * ldz].reshape(T * B, ldz)
    assert (rows[:, W:] == SENTINEL).all(), "written into the padding columns"
    ref = SR.reference(c)["z"]
    if on_plan:
        ml = c["plan"]["mlive"]
        assert ml < T * B and (rows[ml:] == SENTINEL).all(), "rows of steps >= length written"
        got, want = rows[:ml, :W], SR.to_plan(ref, SR.starts_of(c["plan"]), c["lengths"], ml)
    else:
        got, want = rows[:, :W].reshape(T, B, W), ref
    assert np.isfinite(got).all() and not (got == SENTINEL).any()
    e, bound = SR.error_of("z", got, want, MODE)
    print("panel64 guard %s %s %s: z %.2e" % (c["name"], form, MODE, e))
    assert e <= bound, (name, form, e)


# ---- 4. the encoder layer's epilogues in the forced forms ---------------------------------------------------------------------------------
@pytest.mark.parametrize("p_drop", PR.ENC_P, ids=["p0", "p0.2"])
@pytest.mark.parametrize("form", PR.ENC_FORMS)
def test_encoder_layer_in_the_forced_forms_vs_float64(form, p_drop, monkeypatch):
    """All eight dense products of the layer (in_proj, out_proj + dropout + residual, linear1 + ReLU + dropout, linear2 + dropout +
    residual; the four input gradients, linear1's with the gate mask, the dropped ones with posmask + cscale) on the forced form:
    y and the 13 gradients at the bounds of test_encoder_layer_dropout_vs_float64."""
    from raindrop_amd import ops
    L = _L()
    _force(monkeypatch, form)
    c = PR.enc_case()
    T, B, F = c["T"], c["B"], c["F"]
    M, D, H = T * B, c["D"], c["nhid"]
    xd = c["x"].to(DEV).requires_grad_(True)
    pd = [c["p"][n].to(DEV).requires_grad_(True) for n in ops.ENC_PARAM_NAMES]
    shp = L.shape(B, T, F, 4, nhead=c["nhead"], nhid=H)
    mask, dy = c["mask"].to(DEV), c["dy"].to(DEV)
    out = {}

    def fwd():
        out["y"] = ops.encoder_layer(xd, mask, shp, PR.ENC["layer"], p_drop, DR.SEED, pd)

    def bwd():
        out["g"] = torch.autograd.grad(out["y"], [xd] + pd, dy)

    what = "encoder p=%g" % p_drop
    _assert_forward_log(_logged(fwd), form, what)
    _assert_backward_log(_logged(bwd), form, what, [(M, 3 * D, D), (M, D, D), (M, H, D), (M, D, H)])
    got = dict(y=out["y"].detach().cpu().numpy())
    got.update((n, t.cpu().numpy()) for n, t in zip(["x"] + list(ops.ENC_PARAM_NAMES), out["g"]))
    ref, pre = PR.enc_reference(p_drop)
    assert set(got) == set(ref) and float(np.abs(pre).min()) >= SR.GATE_MARGIN
    bound_of = DR.enc_bound(MODE)
    bad, figs = [], []
    for name, r in ref.items():
        a = got[name].astype(np.float64)
        assert a.shape == r.shape, (name, a.shape, r.shape)
        metric, bound = bound_of(name)
        e = DR.rel2(a, r) if metric == "rel2" else float(np.abs(a - r).max())
        figs.append("%s %.2e" % (name, e))
        if not (np.isfinite(a).all() and e < bound and (metric != "rel2" or DR.rel(a, r) < 0.25)):
            bad.append((name, metric, e, bound))
        # with no gate able to flip, every gradient also meets the float64 bound of the gate-free ties (test_attention_core_vs_float64,
        # plan_layer_ref.GRAD_REL, the stage above): 2e-4 of its max-norm, no entry exempt -- one wrong row of 165 shows
        if metric == "rel2" and not DR.rel(a, r) <= SR.GRAD_REL:
            bad.append((name, "rel", DR.rel(a, r), SR.GRAD_REL))
        if metric == "rel2":
            figs.append("%s/max %.2e" % (name, DR.rel(a, r)))
    print("panel64 encoder p%g %s %s: %s" % (p_drop, form, MODE, ", ".join(figs)))
    assert not bad, (form, p_drop, bad)


# ---- 5. the one-product bf16 mode: every form against bf16-rounded float64, and the forms pairwise ------------------------------------
def _rel2(a, r):
    return float(np.linalg.norm((a - r).ravel()) / (np.linalg.norm(r.ravel()) + 1e-30))


@pytest.mark.parametrize("name", list(PR.CASES))
def test_one_product_mode_forms_vs_rounded_float64_and_pairwise(name, monkeypatch):
    c = PR.case16(name)
    cmp_ = PR.compared16(name)
    ref = PR.reference16(name)
    zb = PR.z_bound16(name)
    total, _ = PR.pair_sum()
    _, s2 = SR._scales(c)
    pair_b = total * max(1.0, float(s2.max())) + cmp_["zflip"]
    got = {form: _run(c, form, monkeypatch, prec=2) for form in ("small", "wide", "pc")}
    bad = []
    for form, g in got.items():
        assert np.array_equal(g["mask"], ref["mask"]), (form, "mask")
        ez = np.abs(g["z"].astype(np.float64) - cmp_["z"])
        epe = float(np.abs(g["pe"] - cmp_["pe"]).max()) if g["pe"].size else 0.0
        figs = ["z %.2e (x bound %.3f, over the split-bf16 term alone: %d of %d)" %
                (float(ez.max()), float((ez / zb).max()), int((ez > zb - cmp_["zflip"]).sum()), ez.size), "pe %.2e" % epe]
        if not (np.isfinite(g["z"]).all() and (ez <= zb).all()):
            bad.append((form, "z", float((ez / zb).max())))
        if not epe <= SR.PE_ABS:
            bad.append((form, "pe", epe))
        for n in SR.GRAD_NAMES:
            a, r = g[n].astype(np.float64), cmp_[n]
            e2, em = _rel2(a, r), DR.rel(a, r)
            figs.append("%s %.2e/%.2e" % (n, e2, em))
            if not (np.isfinite(a).all() and e2 < 2e-2 and em < 0.25):
                bad.append((form, n, e2, em))
        print("panel16 stage %s %s bf16: %s" % (c["name"], form, ", ".join(figs)))
    for fa, fb in (("small", "wide"), ("small", "pc"), ("wide", "pc")):
        a, b = got[fa], got[fb]
        assert np.array_equal(a["mask"], b["mask"]) and np.array_equal(a["pe"].view(np.uint32), b["pe"].view(np.uint32)), (fa, fb)
        dz = np.abs(a["z"].astype(np.float64) - b["z"])
        print("panel16 pair %s %s-%s bf16: z %.2e (x bound %.3f), differing %d of %d" %
              (c["name"], fa, fb, float(dz.max()), float((dz / pair_b).max()), int((dz > 0).sum()), dz.size))
        if not (dz <= pair_b).all():
            bad.append((fa, fb, "z", float((dz / pair_b).max())))
        for n in SR.GRAD_NAMES:
            if not _rel2(a[n].astype(np.float64), b[n].astype(np.float64)) < 2e-2:
                bad.append((fa, fb, n))
    assert not bad, (name, bad)
