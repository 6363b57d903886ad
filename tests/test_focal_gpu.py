"""GPU: the focal loss (focal_gamma=) from the kernels up -- rd_softmax_xent_focal and rd_head_train_focal against the float64
reference of tests/focal_ref.py, their gamma = 0 identity with the `_crit` entry points bit for bit, and every form of the step,
validation and fit on top of them.  Outputs and workspaces are pre-filled with a NaN pattern and followed by a guard tail that must
survive.  Every measured error is printed (-s) beside its yardstick; the last test writes the maxima to the file RD_FOCAL64_REPORT
names (profiles/focal_float64_errors.json is one)."""
import ctypes
import gc
import json
import os

import numpy as np
import pytest
import torch

from raindrop_amd import _lib, dp, feed, synth
from tests import focal_ref as FR
from tests import head_ref as HR
from tests.helpers import build_ours, plan_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0x7FC07FC0                                  # fp32 NaN
GUARD = 64
OUTPUTS = ("loss", "logits") + HR.GRADS
W2 = [1.0, 3.0]
_MEASURED = {}                                       # (kind, tensor) -> (error, yardstick, bound, case)


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hooks():
    lib = _lib.load()
    on, read = lib.rd_debug_launch_log, lib.rd_debug_launch_log_read
    on.argtypes, on.restype = [ctypes.c_int], None
    read.argtypes, read.restype = [ctypes.c_char_p, ctypes.c_size_t], ctypes.c_size_t
    return on, read


def _logged(fn, cap=1 << 16):
    on, read = _hooks()
    buf = ctypes.create_string_buffer(cap)
    on(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        read(buf, len(buf))
        on(0)
    return {n for n in buf.value.decode().split("\n") if n}


@pytest.fixture(autouse=True)
def _process_wide_settings_handed_back():
    _lib.call("rd_set_precision", 1)
    _lib.call("rd_set_token_plan", None)
    try:
        yield
    finally:
        _hooks()[0](0)
        _lib.call("rd_set_token_plan", None)
        _lib.call("rd_set_precision", 1)
        try:
            torch.cuda.synchronize()
        except Exception as e:                              # noqa: BLE001 -- any HIP error here is a fault of the device
            pytest.exit("device error after a focal case: %s" % e, returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _hand_back_device_memory():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(params=["bf16x3", "fp32"])
def precision_mode(request):
    _lib.call("rd_set_precision", 1 if request.param == "bf16x3" else 0)
    yield request.param
    _lib.call("rd_set_precision", 1)


class _Out:
    """n elements of fp32 + GUARD more, all POISON; `used` <= n: the elements the call may write"""

    def __init__(self, n, used=None):
        self.n, self.used = int(n), int(n if used is None else used)
        self.t = torch.empty(self.n + GUARD, dtype=torch.float32, device=DEV)
        self.t.view(torch.int32).fill_(POISON)

    def host(self, *shape):
        return self.t[:self.used].cpu().numpy().reshape(shape)

    def tail_intact(self):
        return bool((self.t[self.used:].view(torch.int32) == POISON).all())


def _in(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a).to(DEV) if a.size else None


def _record(kind, case, rows):
    print("focal64 %s %s: %s" % (kind, case, ", ".join("%s %.2e/%.2e = %.2f" % (t, e, y, e / y if y else 0.0) for t, e, _, y in rows)))
    for t, e, b, y in rows:
        if (kind, t) not in _MEASURED or e > _MEASURED[(kind, t)][0]:
            _MEASURED[(kind, t)] = (e, y, b, case)


# ---- 1. the operator -----------------------------------------------------------------------------------------------------------------------
def _xent(entry, c, buf, y=None):
    """one launch of the stand-alone operator on poisoned outputs -> {loss, dlogits} on the host"""
    B, C = c["B"], c["C"]
    logits, yd, bd = _in(c["logits"]), _in(c["y"] if y is None else y), _in(buf)
    loss, dl = _Out(1), _Out(B * C)
    _lib.call(entry, B, C, _P(logits), _P(yd), _P(bd), _P(loss.t), _P(dl.t), _stream())
    torch.cuda.synchronize()
    assert loss.tail_intact() and dl.tail_intact(), (entry, B, C, "guard tail overwritten")
    return dict(loss=loss.host(1)[0], dlogits=dl.host(B, C))


def _buf(c, first):
    return np.concatenate([[np.float32(first)], c["w"]]).astype(np.float32)


@pytest.mark.parametrize("C", FR.OP_C)
@pytest.mark.parametrize("B", FR.OP_B)
def test_operator_against_float64(B, C):
    c = FR.op_case(B, C)
    for gamma in FR.GAMMAS:
        got = _xent("rd_softmax_xent_focal", c, _buf(c, gamma))
        assert np.isfinite(got["loss"]) and np.isfinite(got["dlogits"]).all(), (B, C, gamma)
        rows = FR.op_compare(got, FR.op_reference(B, C, gamma), FR.op_reference(B, C, gamma, np.float32))
        _record("operator", "B%d_C%d_g%g" % (B, C, gamma), rows)
        assert all(e <= b for _, e, b, _ in rows), (B, C, gamma, rows)
        if gamma > 0 and C > 1 and len(c["confident"]):
            # fp32 q is exactly 0 on these rows: an exact zero row, also for gamma < 1 where q^(gamma - 1) is infinite
            assert not got["dlogits"][c["confident"]].any(), (B, C, gamma)
        if C == 1:
            assert not got["dlogits"].any()
        if gamma == 0:
            crit = _xent("rd_softmax_xent_crit", c, _buf(c, 0.0))
            assert torch.equal(torch.from_numpy(got["dlogits"]), torch.from_numpy(crit["dlogits"])) and got["loss"] == crit["loss"]
        again = _xent("rd_softmax_xent_focal", c, _buf(c, gamma))
        assert again["loss"].tobytes() == got["loss"].tobytes() and again["dlogits"].tobytes() == got["dlogits"].tobytes()


@pytest.mark.parametrize("gamma", FR.SMALL_GAMMAS)
def test_operator_small_gamma_at_a_gap_near_100_is_finite(gamma):
    """q a positive denormal, lse - z_y exactly 0 and q^(gamma - 1) beyond the largest float: finite, and within the bounds"""
    c = FR.small_gamma_case()
    got = _xent("rd_softmax_xent_focal", c, _buf(c, gamma))
    assert np.isfinite(got["loss"]) and np.isfinite(got["dlogits"]).all(), (gamma, got)
    ref = {k: dict(zip(FR.OP_TENSORS, FR.loss_and_dlogits(c["logits"], c["y"], c["w"], gamma, dt))) for k, dt in (("64", np.float64), ("32", np.float32))}
    rows = FR.op_compare(got, ref["64"], ref["32"])
    _record("operator", "GAP100_g%g" % gamma, rows)
    assert all(e <= b for _, e, b, _ in rows), (gamma, rows)


def test_operator_confident_rows_alone_give_a_zero_loss_term():
    """a batch of confidently right rows only (fp32 q == 0 everywhere): gamma > 0 gives loss 0 and all-zero dlogits, never 0 * inf"""
    c = FR.op_case(64, 8)
    rows = c["confident"]
    sub = dict(B=len(rows), C=8, logits=c["logits"][rows], y=c["y"][rows], w=np.ones(8, dtype=np.float32))
    for gamma in (0.5, 1.0, 2.0, 5.0):
        got = _xent("rd_softmax_xent_focal", sub, _buf(sub, gamma))
        assert got["loss"] == 0.0 and not got["dlogits"].any(), (gamma, got["loss"])


@pytest.mark.parametrize("bad", [-1, "C"])
def test_operator_label_out_of_range_is_nan_and_reads_nothing(bad):
    c = FR.op_case(64, 8)
    y = c["y"].copy()
    y[5] = c["C"] if bad == "C" else -1
    got = _xent("rd_softmax_xent_focal", c, _buf(c, 2.0), y=y)
    assert np.isnan(got["loss"]) and np.isfinite(got["dlogits"]).all()


def test_operator_all_weights_zero_is_nan():
    c = FR.op_case(3, 2)
    got = _xent("rd_softmax_xent_focal", c, np.array([2.0, 0.0, 0.0], dtype=np.float32))
    assert np.isnan(got["loss"])


# ---- 2. the fused head ------------------------------------------------------------------------------------------------------------------------
class _Case:
    """the device side of one head_ref case: inputs, the plan where the case has one, fresh poisoned outputs per call"""

    def __init__(self, name, y=None):
        self.c = c = FR.case(name)
        T, B, D = c["T"], c["B"], c["D"]
        self.shp = _lib.shape(B, T, 1, 4)
        self.plan, self.ml = None, T * B
        r = c["r"].reshape(T * B, D)
        if c["layout"] == "plan":
            p = plan_ref(c["lengths"], T)
            self.ml = p["mlive"]
            r = np.full((T * B, D), np.nan, dtype=np.float32)            # rows >= M_live: nothing may read them into a result
            r[:self.ml] = HR.rows_of(c, c["r"])
            lengths = torch.from_numpy(c["lengths"]).to(DEV)
            self.plan = torch.zeros(max(int(_lib.load().rd_token_plan_bytes(ctypes.byref(self.shp))) // 4, 64), dtype=torch.int32, device=DEV)
            _lib.call("rd_token_plan", ctypes.byref(self.shp), _P(lengths), _P(self.plan), None, 0, _stream())
            torch.cuda.synchronize()
            assert int(self.plan[0]) == self.ml
        mask = (~HR.keep_of(c["lengths"], T)).T.astype(np.uint8)
        self.i = dict(r=_in(r), mask=_in(mask), lengths=_in(c["lengths"]), stat=_in(c["stat"]), emb_w=_in(c["emb_w"]), emb_b=_in(c["emb_b"]),
                      w0=_in(c["w0"]), b0=_in(c["b0"]), w2=_in(c["w2"]), b2=_in(c["b2"]), y=_in(c["y"] if y is None else y))
        self.ws_bytes = int(_lib.load().rd_head_train_workspace_bytes(B, c["dh"], c["C"]))

    def run(self, entry, buf):
        """one launch pair on fresh outputs -> ({tensor: host array}, launch names)"""
        c, i = self.c, self.i
        T, B, D, Fe, ds, C, dh = (c[k] for k in ("T", "B", "D", "Fe", "ds", "C", "dh"))
        o = dict(loss=_Out(1), logits=_Out(B * C), dr=_Out(T * B * D, self.ml * D), dW0=_Out(dh * dh), db0=_Out(dh), dW2=_Out(C * dh),
                 db2=_Out(C), demb_w=_Out(Fe * ds), demb_b=_Out(Fe), ws=_Out(self.ws_bytes // 4))
        bd = _in(buf)
        head = [ctypes.byref(self.shp), D, ds, Fe, C] + [_P(i[k]) for k in ("r", "mask", "lengths", "stat", "emb_w", "emb_b", "w0", "b0",
                                                                              "w2", "b2")]
        emb = [_P(o["demb_w"].t) if Fe else None, _P(o["demb_b"].t) if Fe else None]
        args = head + [_P(i["y"]), _P(bd), _P(o["loss"].t), _P(o["logits"].t)] + emb + [_P(o[k].t) for k in ("dW0", "db0", "dW2", "db2", "dr")] \
            + [_P(o["ws"].t), self.ws_bytes, _stream()]

        def go():
            _lib.call("rd_set_token_plan", _P(self.plan))
            try:
                _lib.call(entry, *args)
            finally:
                _lib.call("rd_set_token_plan", None)

        names = _logged(go)
        for k, b in o.items():
            assert b.tail_intact(), (c["name"], entry, k, "guard tail (or a row >= M_live) overwritten")
        shapes = dict(loss=(), logits=(B, C), dr=(self.ml, D) if self.plan is not None else (T, B, D), dW0=(dh, dh), db0=(dh,), dW2=(C, dh),
                      db2=(C,), demb_w=(Fe, ds), demb_b=(Fe,))
        return {k: o[k].host(*shapes[k]) for k in OUTPUTS}, names


@pytest.mark.parametrize("name,gamma", FR.HEAD_RUNS)
def test_head_train_focal_vs_float64(name, gamma):
    k = _Case(name)
    got, names = k.run("rd_head_train_focal", FR.focal_buffer(k.c, gamma))
    assert {n for n in names if n.startswith("k_head_rows")} == {FR.instantiation(k.c)} and "k_head_wgrad" in names, sorted(names)
    for t in OUTPUTS:
        assert np.isfinite(got[t]).all(), (name, t, "not finite: an element was never written")
    rows, nonzero = FR.compare(name, gamma, got)
    _record("head", "%s_g%g" % (name, gamma), rows)
    assert all(e <= b for _, e, b, _ in rows), (name, gamma, [(t, e, b) for t, e, b, _ in rows if not e <= b])
    assert not nonzero, (name, nonzero, "not exactly zero where the reference is")


@pytest.mark.parametrize("name", FR.HEAD_ZERO_RUNS)
def test_gamma_zero_is_the_crit_head_bit_for_bit(name):
    k = _Case(name)
    buf = FR.focal_buffer(k.c, 0.0)                                      # [0, w ..]: also the criterion's buffer at eps = 0
    focal, _ = k.run("rd_head_train_focal", buf)
    crit, names = k.run("rd_head_train_crit", buf)
    assert not any("focal" in n for n in names)
    for t in OUTPUTS:
        assert torch.equal(torch.from_numpy(np.asarray(focal[t])), torch.from_numpy(np.asarray(crit[t]))), (name, t)


@pytest.mark.parametrize("name,gamma", [("DH186", 2.0), ("DH193", 0.5), ("CRIT_B1025", 2.0)])
def test_focal_launches_repeat_their_bits_in_both_arithmetic_modes(name, gamma):
    """the head is fp32 FMA whatever rd_set_precision selects for the GEMMs: four launches, two per mode, one set of bits"""
    k = _Case(name)
    runs = []
    for prec in (1, 1, 0, 0):
        _lib.call("rd_set_precision", prec)
        runs.append(k.run("rd_head_train_focal", FR.focal_buffer(k.c, gamma))[0])
    for other in runs[1:]:
        assert not [t for t in OUTPUTS if runs[0][t].tobytes() != other[t].tobytes()]


@pytest.mark.parametrize("bad", [-1, "C"])
def test_head_bad_label_gives_a_nan_loss_and_intact_guards(bad):
    c = HR.case("C2")
    y = c["y"].copy()
    y[2] = c["C"] if bad == "C" else -1
    got, _ = _Case("C2", y=y).run("rd_head_train_focal", FR.focal_buffer(c, 2.0))
    assert np.isnan(got["loss"]) and np.isfinite(got["logits"]).all()
    rows, _ = FR.compare("C2", 2.0, got, ("logits",))
    assert all(e <= b for _, e, b, _ in rows)


# ---- 3. the steps -----------------------------------------------------------------------------------------------------------------------------
def _p19(seed_model, seed_batch, B=8, **kw):
    cfg = synth.make_config("P19")
    gs = synth.make_structure(cfg, "sparse")
    dv = {k: (None if v is None else v.to(DEV).clone()) for k, v in synth.make_batch(cfg, B, seed=seed_batch).items()}
    m = build_ours(cfg, gs, DEV, seed_model, **kw).train()                     # dropout p forced to 0 by build_ours
    return cfg, m, dv


def _train_step(seed_batch=41, flatten=False, **kw):
    """(step, flat, batch); flatten: the parameters moved into one flat buffer first (what capture_full's optimizer steps)"""
    from raindrop_amd.step import TrainStep
    cfg, m, dv = _p19(7, seed_batch)
    named = dict(m.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)], n_buckets=2)
    if flatten:
        flat.flatten_parameters()
    kw.setdefault("autotune", False)
    return TrainStep(m, flat, dv, **kw), flat, dv


def _close(a, b):
    """within the project's gradient ceiling (tests/head_ref.py CEILING) of the reference's max-norm.  The project's rule is
    min(ceiling, 4 x the fp32 yardstick); there is no float64 evaluation of the whole model to take a yardstick from at the step
    level, so the ceiling alone holds here -- the kernels themselves are held to the full rule in sections 1 and 2"""
    return float((a - b).abs().max()) <= HR.CEILING * float(b.abs().max())


def test_eager_captured_and_whole_step_graphs_give_the_same_bits(precision_mode):
    from raindrop_amd.optim import FlatAdam
    kw = dict(focal_gamma=2.0, class_weight=W2)
    eager, fe, _ = _train_step(use_graph=False, **kw)
    graph, fg, _ = _train_step(use_graph=True, **kw)
    full, ff, _ = _train_step(use_graph=False, split=False, flatten=True, **kw)
    try:
        assert eager.focal is not None and eager.crit is None and eager.head_fused
        names = _logged(lambda: eager.run())
        le, ge = eager.loss.clone(), fe.flat.clone()
        assert "k_head_rows<12,3,focal>" in names and not any("crit" in n for n in names), sorted(names)
        lg = graph.run().clone()
        full.capture_full(FlatAdam(ff.flat_param, lr=1e-4))
        lf = full.run_full().clone()
        torch.cuda.synchronize()
        assert torch.isfinite(le) and torch.equal(le, lg) and torch.equal(le, lf)
        assert torch.equal(ge, fg.flat) and torch.equal(ge, ff.flat)
    finally:
        eager.close(); graph.close(); full.close()


def test_fused_head_step_agrees_with_the_operator_by_operator_head(monkeypatch):
    kw = dict(focal_gamma=2.0, class_weight=W2, use_graph=False)
    fused, ff, _ = _train_step(**kw)
    monkeypatch.setenv("RD_HEAD_FUSED", "0")                           # read per call: the step decides when it is built
    byop, fo, _ = _train_step(**kw)
    monkeypatch.delenv("RD_HEAD_FUSED")
    try:
        assert fused.head_fused and not byop.head_fused
        names = _logged(lambda: byop.run())
        lf = fused.run()
        torch.cuda.synchronize()
        assert "k_softmax_xent_focal" in names and not any(n.startswith("k_head_rows") for n in names), sorted(names)
        print("loss fused %.8f by operator %.8f" % (float(lf), float(byop.loss)))
        assert abs(float(lf) - float(byop.loss)) <= HR.LOSS_CEILING * max(1.0, abs(float(byop.loss)))
        assert _close(ff.flat, fo.flat)
    finally:
        fused.close(); byop.close()


def test_step_loss_is_the_reference_s_on_its_own_logits():
    step, _, dv = _train_step(focal_gamma=2.0, class_weight=W2, use_graph=False)
    try:
        loss = float(step.run())
        logits, y = step.logits.cpu().numpy(), dv["y"].cpu().numpy()
        ref, _ = FR.loss_and_dlogits(logits, y, np.array(W2), 2.0)
        plain, _ = FR.loss_and_dlogits(logits, y, np.ones(2), 0.0)
        print("focal %.8f reference %.8f (plain CE %.8f)" % (loss, ref, plain))
        assert abs(loss - ref) <= HR.LOSS_CEILING * max(1.0, abs(ref)) and abs(loss - plain) > 1e-3
    finally:
        step.close()


def test_set_criterion_changes_gamma_without_a_new_capture():
    a, fa, _ = _train_step(use_graph=True, focal_gamma=2.0, class_weight=W2)
    b, fb, _ = _train_step(use_graph=True, focal_gamma=0.5, class_weight=[1.5, 0.25])
    crit, _, _ = _train_step(use_graph=False, class_weight=W2)
    try:
        graph = a.graph
        la0 = a.run().clone()
        a.set_criterion(class_weight=[1.5, 0.25], focal_gamma=0.5)
        la, lb = a.run(), b.run()
        torch.cuda.synchronize()
        assert a.graph is graph and not torch.equal(la0, la)
        assert torch.equal(la, lb) and torch.equal(fa.flat, fb.flat)
        with pytest.raises(ValueError, match="label_smoothing"):
            a.set_criterion(focal_gamma=0.5, label_smoothing=0.1)
        with pytest.raises(_lib.RaindropHipError, match="not built for the focal loss"):
            crit.set_criterion(class_weight=W2, focal_gamma=2.0)
        assert crit.focal is None
    finally:
        a.close(); b.close(); crit.close()


def test_accumulate_two_closes_a_window_with_the_mean_gradient():
    kw = dict(focal_gamma=2.0, class_weight=W2, use_graph=False)
    acc, fa, dva = _train_step(accumulate=2, **kw)
    one, fo, dvo = _train_step(**kw)
    _, _, other = _p19(7, 43)
    try:
        micro = []
        for batch in (None, other):
            if batch is not None:
                for k, v in batch.items():
                    if v is not None:
                        dva[k].copy_(v); dvo[k].copy_(v)
            one.run()
            micro.append(fo.flat.clone())
            acc.run()
        torch.cuda.synchronize()
        assert acc.window_closed and not torch.equal(micro[0], micro[1])
        assert _close(fa.flat, (micro[0] + micro[1]) * 0.5)
    finally:
        acc.close(); one.close()


def test_beta_step_eager_equals_captured():
    from raindrop_amd.step_beta import BetaTrainStep

    def make(use_graph):
        cfg, m, dv = _p19(7, 41, use_beta=True, compute_distance=True)
        named = dict(m.named_parameters())
        flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names_beta(cfg)])
        return BetaTrainStep(m, flat, dv, autotune=False, use_graph=use_graph, token_plan=True, focal_gamma=2.0), flat

    e, fe = make(False)
    g, fg = make(True)
    try:
        assert e.focal is not None and e.head_fused
        le, lg = e.run().clone(), g.run().clone()
        torch.cuda.synchronize()
        assert torch.isfinite(le) and torch.equal(le, lg) and torch.equal(fe.flat, fg.flat)
    finally:
        e.close(); g.close()


def test_autograd_step_loss_is_the_reference_s():
    from raindrop_amd.step import AutogradStep
    cfg, m, dv = _p19(7, 41)
    st = AutogradStep(m, dv, optimizer=False, focal_gamma=2.0, class_weight=W2)
    try:
        loss = float(st.run())
        torch.cuda.synchronize()
        ref, _ = FR.loss_and_dlogits(st.logits.cpu().numpy(), dv["y"].cpu().numpy(), np.array(W2), 2.0)
        print("autograd %.8f reference %.8f" % (loss, ref))
        assert abs(loss - ref) <= HR.LOSS_CEILING * max(1.0, abs(ref))
    finally:
        st.close()


# ---- 4. validate and fit ------------------------------------------------------------------------------------------------------------------------
def _dataset(n, seed):
    cfg = synth.make_config("P19")
    val = synth.make_batch(cfg, n, seed=seed)
    y = np.random.default_rng(seed).integers(0, 2, n)
    return cfg, feed.DeviceDataset(val["src"], val["times"], val["static"], y, device=DEV)


def test_validate_reports_the_focal_loss_and_nothing_else_changes():
    cfg, ds = _dataset(50, 90)
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 5).eval()
    v0 = feed.validate(m, ds, chunk=64)
    v1 = feed.validate(m, ds, chunk=64, class_weight=W2, focal_gamma=2.0)
    scores = torch.sigmoid(feed.evaluate_captured(m, ds, 64)).contiguous()
    loss, dl = torch.empty(1, device=DEV), torch.empty_like(scores)
    buf = torch.tensor([2.0] + W2, dtype=torch.float32, device=DEV)
    _lib.call("rd_softmax_xent_focal", 50, 2, _P(scores), _P(ds.y), _P(buf), _P(loss), _P(dl), _stream())
    torch.cuda.synchronize()
    assert v1["loss"] == float(loss) and v1["loss"] != v0["loss"] and set(v0) == set(v1)
    for k in v0:
        if k != "loss":
            assert np.array_equal(np.asarray(v0[k]), np.asarray(v1[k])), k


def test_fit_runs_the_focal_kernel_and_no_crit_kernel():
    from raindrop_amd import trainer
    cfg, ds = _dataset(64, 17)
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 5)
    out = {}
    names = _logged(lambda: out.update(trainer.fit(m, ds, ds, epochs=1, batch_size=8, autotune=False, seed=3, focal_gamma=2.0)), cap=1 << 20)
    assert np.isfinite(out["train_loss"]).all() and np.isfinite(out["val_loss"]).all() and len(out["train_loss"]) == 1
    assert "k_head_rows<12,3,focal>" in names and "k_softmax_xent_focal" in names and not any("crit" in n for n in names), sorted(names)


# ---- 5. the figures ----------------------------------------------------------------------------------------------------------------------------
def test_zz_report_measured_errors_beside_the_yardstick():
    """Runs last in the file: the maximum measured error per (kind, tensor) beside the CPU yardstick of the case that gave it; with
    RD_FOCAL64_REPORT=<path> the same figures go to that file as JSON."""
    if not _MEASURED:
        return
    report = {"measured": {}}
    for (kind, t), (e, y, b, case) in sorted(_MEASURED.items()):
        report["measured"].setdefault(kind, {})[t] = {"error": e, "yardstick": y, "bound": b, "case": case}
        print("focal64 max %s %s: %.2e (%s), yardstick %.2e, bound %.2e" % (kind, t, e, case, y, b))
    if os.environ.get("RD_FOCAL64_REPORT"):
        with open(os.environ["RD_FOCAL64_REPORT"], "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
