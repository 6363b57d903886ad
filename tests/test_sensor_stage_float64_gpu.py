"""GPU: the sensor stage -- observation embedding, both Observation_progation layers, the scatter to [T, B, 4 F + 16], the PE columns
and the padding mask (ops.sensor_stage_fwd_raw / sensor_stage_bwd_raw: rd_sensor_stage_fwd[_coef], rd_msgpass_bwd[_coef]) -- against
float64, across the envelope of the fused kernels (rd_msgpass_fused.hip k_msg_fwd_fused / k_msg_bwd_fused, rd_msgpass_dw.hip k_dw):
every leftover-tile geometry of rd_k1_layout.h (F = 1 .. 48 around `per`), one to fifteen column tiles and reduction lengths with and
without a half step (T = 4 .. 60), one sample per row-tile count, `lin` patterns mixed in a batch, the COEF instantiations, a
registered token plan at six shapes x five length sets, and the shapes just outside (F = 49, K = 244, K % 16 != 0) where the same
entry points route to the generic kernels.  Cases, inputs, reference and bounds: tests/sensor_stage_ref.py
(tests/test_sensor_stage_ref_host.py shows on the reference alone that the gates are decisive and the bounds bite).

  1. padded layout, both arithmetic modes: z, the PE columns, the mask (bit-exact) and the five gradients.  fp32 mode runs the generic
     path, which gets the same tie.  The launch log must name the three fused kernels for envelope cases in bf16x3 and none of them
     otherwise: a case that silently falls back fails;
  2. the COEF instantiations: the table rd_msgpass_coef_table wrote is read back and handed to the reference as data, the gap-placed
     biases are recomputed with those scales (and the margin conditions re-asserted here, since the host cannot know the table);
  3. F = 34, T = 60 under RD_K1_SPECIALIZE=0: the log does not tell instantiations apart, so the runtime-shape <3, 0, 0> twin must
     be bit-equal to the specialised <3, 34, 60> run and both must meet the bounds (and the route query names the instantiation);
  4. a registered token plan (bf16x3): z and PE on live rows, dz rows >= M_live NaN.  The sensor-stage entry points accept a plan at
     every shape -- inside the envelope the fused kernels read it, outside the generic scatter / gather does -- so there is no
     refusal to pin (unlike the encoder layer's widths);
  5. the yardstick: the padded envelope cases under RD_K1_FUSED=0 (the kernels test_sensor_stage_vs_oracle binds) against the same
     reference -- the only source of a bound above 2e-4 (sensor_stage_ref.RAISED).

Every measured error is printed (-s) as `sensor64 <kind> <case> <mode>: <tensor> <error>, ...`."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from raindrop_amd import synth
from tests import sensor_stage_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
FUSED = {"k_msg_fwd_fused", "k_msg_bwd_fused", "k_dw"}
COMPARED = ("z", "pe") + SR.GRAD_NAMES


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
            pytest.exit("device error after a sensor-stage case: %s" % e, returncode=3)


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


def _run(c, mode):
    """The stage forward + backward on c's layout -> ({z, pe, mask, five gradients} as numpy; z / pe on live rows in plan order where
    the case runs on a plan), launch names."""
    from raindrop_amd import ops
    L = _L()
    lib = L.load()
    T, B, F, D = c["T"], c["B"], c["F"], c["D"]
    shp = L.shape(B, T, F, SR.D_OB)
    sp = ctypes.byref(shp)
    L.call("rd_set_precision", 1 if mode == "bf16x3" else 0)
    src, times, lengths = _dev(c["src"]), _dev(c["times"]), _dev(c["lengths"])
    ts = ops.timescales(T).to(DEV)
    ssum, R_u, W1, b1, W2, b2 = (_dev(c[n]) for n in ("ssum", "R_u", "W1", "b1", "W2", "b2"))
    coef = None if c["coef"] is None else _dev(c["coef"])
    on_plan = c["layout"] == "plan"
    ml = c["plan"]["mlive"]
    if on_plan:
        dz = torch.full((T * B, D), float("nan"), device=DEV)              # rows >= M_live: never to be read
        dz[:ml] = _dev(SR.to_plan(c["dz"], SR.starts_of(c["plan"]), c["lengths"], ml))
        dz = dz.view(T, B, D)
        plan = torch.zeros(max(int(lib.rd_token_plan_bytes(sp)) // 4, 64), dtype=torch.int32, device=DEV)
        L.call("rd_token_plan", sp, ctypes.c_void_p(lengths.data_ptr()), ctypes.c_void_p(plan.data_ptr()), None, 0,
               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    else:
        dz = _dev(c["dz"])
    out = {}

    def go():
        if on_plan:
            L.call("rd_set_token_plan", ctypes.c_void_p(plan.data_ptr()))
        try:
            z, mask, saved = ops.sensor_stage_fwd_raw(src, times, lengths, ts, ssum, R_u, W1, b1, W2, b2, shp, 0.0, 0, coef)
            g = ops.sensor_stage_bwd_raw(src, R_u, W1, W2, ssum, saved, z, dz, shp, 0.0, coef)
        finally:
            if on_plan:
                L.call("rd_set_token_plan", None)
        out["z"], out["mask"], out["g"] = z, mask, g

    names = _logged(go)
    z = out["z"]
    if on_plan:
        h = plan.cpu().numpy()
        assert h[0] == ml and np.array_equal(h[8:8 + B + 1], c["plan"]["off"]) and np.array_equal(h[9 + B:9 + 2 * B], c["plan"]["rank"])
        z = z.view(T * B, D)[:ml]
    zc = z.cpu().numpy()
    got = dict(z=zc[..., :F * SR.D_OB], pe=zc[..., F * SR.D_OB:], mask=out["mask"].cpu().numpy())
    got.update((n, t.cpu().numpy()) for n, t in zip(SR.GRAD_NAMES, out["g"]))
    return got, names


def _compare(kind, c, mode, got):
    """print every tensor's error, then hold each to its bound; the mask bit for bit"""
    ref = SR.reference(c)
    cmp_ = SR.compared(c, ref)
    bad, figs = [], []
    for name in COMPARED:
        e, bound = SR.error_of(name, got[name], cmp_[name], mode)
        figs.append("%s %.2e" % (name, e))
        if not (np.isfinite(got[name]).all() and e <= bound):
            bad.append((name, e, bound))
    print("sensor64 %s %s %s: %s" % (kind, c["name"], mode, ", ".join(figs)))
    assert np.array_equal(got["mask"], ref["mask"]), "mask"
    assert not bad, (kind, c["name"], mode, bad)


def _route(c):
    """the route of c's sensor-stage call (rd_debug_sensor_route) in the mode and switches of the moment: the instantiation, which
    the log does not tell"""
    L = _L()
    bits = ctypes.c_uint32(0)
    L.call("rd_debug_sensor_route", ctypes.byref(L.shape(c["B"], c["T"], c["F"], SR.D_OB)), c["D"], 1, int(c["coef"] is not None),
           ctypes.byref(bits))
    return {n for i, n in enumerate(L.SENSOR_ROUTE_BITS) if bits.value >> i & 1} | {"rt%d" % (bits.value >> 8)}


def _assert_route(c, mode, names):
    if c["envelope"] and mode == "bf16x3":
        assert FUSED <= names, (c["name"], mode, sorted(names))
        assert {"fused", "rt%d" % ((c["F"] + 15) // 16)} <= _route(c), (c["name"], sorted(_route(c)))
    else:
        assert not (FUSED & names), (c["name"], mode, sorted(names))
        assert "fused" not in _route(c), (c["name"], mode, sorted(_route(c)))


# ---- 1. padded layout, both modes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", SR.MODES)
@pytest.mark.parametrize("name", SR.PADDED_CASES)
def test_sensor_stage_vs_float64(name, mode):
    c = SR.case(name)
    got, names = _run(c, mode)
    _assert_route(c, mode, names)
    _compare("padded", c, mode, got)


# ---- 2. COEF instantiations -----------------------------------------------------------------------------------------------------------
_COEF = {}


def _coef_case(name):
    """The case built around the table the device wrote: rd_msgpass_coef_table on a sparse structure's edge list, p = (0.3, 0.3)."""
    if name not in _COEF:
        from raindrop_amd import ops
        F, T, B, pattern = SR.SHAPES[name]
        gs = synth.make_structure(dict(d_inp=F), "sparse")
        adj, ei, ew = ops.graph_build(gs.to(DEV))
        _, ssum = ops.edge_softmax_dense(adj)
        coef = ops.coef_table(ei, ew, ssum, B, SR.COEF_P[0], SR.COEF_P[1], SR.COEF_SEED).cpu().numpy()
        assert coef.shape == (2, B, F) and np.isfinite(coef).all() and (coef >= 0).all() and len(np.unique(coef)) > F
        lengths = SR._lengths(SR._rng("lengths", name), T, B, pattern)
        c = SR.make_case(name, F, T, lengths, pattern, "padded", coef=coef, ssum=ssum.cpu().numpy())
        r = SR.reference(c)
        for layer in ("pre1", "pre2"):                       # the conditions of tests/test_sensor_stage_ref_host.py, on the device's table
            assert float(np.abs(r[layer]).min()) >= SR.GATE_MARGIN and 0.25 <= float((r[layer] > 0).mean()) <= 0.75, (name, layer)
        _COEF[name] = c
    return _COEF[name]


@pytest.mark.parametrize("mode", SR.MODES)
@pytest.mark.parametrize("name", SR.COEF_CASES)
def test_coef_instantiations_vs_float64(name, mode):
    c = _coef_case(name)
    got, names = _run(c, mode)
    _assert_route(c, mode, names)
    _compare("coef", c, mode, got)


# ---- 3. the specialised instantiation and its runtime-shape twin ---------------------------------------------------------------------
@pytest.mark.parametrize("name", [SR.SPECIALIZE_TWIN, "C_P19"])
def test_runtime_shape_twin_of_the_specialised_instantiation(name, monkeypatch):
    """F = 34, T = 60: <3, 34, 60> by default, <3, 0, 0> under RD_K1_SPECIALIZE=0 (COEF: the <.., true> pair).  Same source, same
    arithmetic, same order: every output bit-equal, and each run within the float64 bounds."""
    c = _coef_case(name) if name in SR.COEF_CASES else SR.case(name)
    assert (c["F"], c["T"]) == (34, 60)
    spec, names_s = _run(c, "bf16x3")
    assert {"fused", "rt3", "specialised"} <= _route(c)
    monkeypatch.setenv("RD_K1_SPECIALIZE", "0")
    twin, names_t = _run(c, "bf16x3")
    assert {"fused", "rt3"} <= _route(c) and "specialised" not in _route(c)
    assert FUSED <= names_s and FUSED <= names_t
    _compare("specialised", c, "bf16x3", spec)
    _compare("runtime-shape", c, "bf16x3", twin)
    for k in spec:
        assert np.array_equal(spec[k], twin[k]), k


# ---- 4. token plan --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,lset", SR.PLAN_CASES, ids=["%s-%s" % k for k in SR.PLAN_CASES])
def test_sensor_stage_on_a_token_plan_vs_float64(shape, lset):
    c = SR.plan_case(shape, lset)
    got, names = _run(c, "bf16x3")
    _assert_route(c, "bf16x3", names)
    _compare("plan", c, "bf16x3", got)


# ---- 5. the yardstick -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SR.GEOMETRY + SR.COEF_CASES)
def test_yardstick_meets_the_bounds(name, monkeypatch):
    """The generic kernels (RD_K1_FUSED=0) in the same split-bf16 arithmetic on the same inputs against the same reference: what every
    bound above 2e-4 would be derived from (2 x its error where that exceeds 1e-4; none does: sensor_stage_ref.RAISED is empty)."""
    c = _coef_case(name) if name in SR.COEF_CASES else SR.case(name)
    monkeypatch.setenv("RD_K1_FUSED", "0")
    got, names = _run(c, "bf16x3")
    assert not (FUSED & names), sorted(names)
    _compare("yardstick", c, "bf16x3", got)
