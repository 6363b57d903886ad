"""GPU: the inference forward (include/raindrop_hip.h "inference forward"; `EvalStep(save_free=True)`, what `feed.validate` builds).

* the logits -- and the structure distance -- are BIT-identical to the saving form (`save_free=False`, the training forward), so the
  bounds of tests/test_eval_step_gpu.py against the eager surface carry over;
* an `_infer` entry point given a buffer of the inference size writes nothing behind it, and refuses a smaller one before any launch;
* replays see weights changed in place, and a training step interleaved with inference replays computes what it computed without."""
import ctypes

import numpy as np
import pytest
import torch

from raindrop_amd import _lib, dp, feed, ops, synth
from raindrop_amd.evalstep import EvalStep
from raindrop_amd.step import TrainStep, _p
from tests.helpers import build_ours

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("src", "times", "lengths", "static")
BETA = {"use_beta": True, "compute_distance": True}


@pytest.fixture(autouse=True, params=["bf16x3", "fp32"])
def precision_mode(request):
    _lib.call("rd_set_precision", 1 if request.param == "bf16x3" else 0)
    yield request.param
    _lib.call("rd_set_precision", 1)


def _batch(cfg, B, seed=41):
    """device batch whose lengths include a sample of length 1 and one of full length"""
    b = synth.make_batch(cfg, B, seed=seed)
    b = {k: (None if b.get(k) is None else b[k].to(DEV).clone()) for k in KEYS}
    b["lengths"][0] = 1
    b["lengths"][1] = b["src"].shape[0]
    return b


def _model(cfg_name, kw, seed=7):
    cfg = synth.make_config(cfg_name)
    return cfg, build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, seed, **kw).eval()


def _covers(step):
    k1, enc = ctypes.c_int32(-1), ctypes.c_int32(-1)
    _lib.call("rd_infer_covers", step.sp, ctypes.byref(k1), ctypes.byref(enc))
    return k1.value, enc.value


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("plan", [None, False], ids=["plan", "padded"])
@pytest.mark.parametrize("kw", [{}, BETA], ids=["default", "use_beta"])
@pytest.mark.parametrize("cfg_name,B", [("P19", 3), ("P19", 32), ("P12", 2)])
def test_logits_equal_the_saving_form_bit_for_bit(cfg_name, B, kw, plan, use_graph, precision_mode):
    cfg, m = _model(cfg_name, kw)
    b = _batch(cfg, B)
    free = EvalStep(m, b, token_plan=plan, use_graph=use_graph, save_free=True)
    saving = EvalStep(m, b, token_plan=plan, use_graph=use_graph, save_free=False)
    assert free.infer and not saving.infer and (free.plan is None) == (saving.plan is None)
    got, want = free.run().clone(), saving.run().clone()
    print(cfg_name, B, kw, precision_mode, "plan" if free.plan is not None else "padded", "covers", _covers(free),
          "bytes", free.buffer_bytes(), saving.buffer_bytes(), "max |diff| = %.3e" % float((got - want).abs().max()))
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    if kw:
        assert torch.equal(free.distance, saving.distance)
    assert torch.equal(free.run(), want)                               # a second replay: nothing the forward reads was clobbered
    if free.buffer_bytes() is not None:
        assert free.buffer_bytes() <= saving.buffer_bytes()
    free.close(); saving.close()


def test_p19_is_covered_and_smaller(precision_mode):
    """Without this the feature could be a no-op: in the default mode both stages of P19 have save-free kernels and every inference
    buffer is strictly smaller than its training twin."""
    _lib.call("rd_set_precision", 1)                                   # the default mode, whatever the fixture chose
    cfg, m = _model("P19", {})
    step = EvalStep(m, _batch(cfg, 32), use_graph=False, save_free=True)
    lib = step.lib
    assert _covers(step) == (1, 1)
    assert 0 < lib.rd_msgpass_infer_bytes(step.sp) < lib.rd_msgpass_saved_bytes(step.sp)
    assert 0 < lib.rd_encoder_layer_infer_bytes(step.sp) < lib.rd_encoder_layer_saved_bytes(step.sp)
    E = ctypes.c_int32(int(step.graph_info["edge_index"].shape[1]))
    assert 0 < lib.rd_beta_stage_infer_bytes(step.sp, E) < lib.rd_beta_stage_saved_bytes(step.sp, E)
    assert step.buffer_bytes() < EvalStep(m, step.batch, use_graph=False, save_free=False).buffer_bytes()


def _sentinel(n):
    return torch.full((int(n),), 0xA5, dtype=torch.uint8, device=DEV)


def _stage_calls(step):
    """(name, full bytes, inference bytes, call(buffer, nbytes) -> rc, check()) per stage entry point, on the step's own inputs.
    `call` runs the stage's prepare into the same buffer first where the stage takes prepared tiles."""
    lib, sp, b, P, st = step.lib, step.sp, step.batch, step.P, ops._stream()
    out = []
    if getattr(step.model, "use_beta", False):
        sn = step.sensor
        E = ctypes.c_int32(sn.E)
        ws = torch.zeros(int(lib.rd_beta_stage_workspace_bytes(sp, E)), dtype=torch.uint8, device=DEV)
        z, mask = torch.zeros_like(step.z), torch.zeros_like(step.mask)
        ei2, alpha = torch.zeros_like(sn.ei2), torch.zeros_like(sn.alpha)      # (kept alive: the call takes raw addresses)
        l1, l2 = "ob_propagation.", "ob_propagation_layer2."

        def beta(buf, n):
            return lib.rd_beta_stage_fwd_infer(
                sp, _p(b["src"]), _p(b["times"]), _p(b["lengths"]), _p(step.ts), _p(P["R_u"]), _p(P[l1 + "lin_value.weight"]),
                _p(P[l1 + "lin_value.bias"]), _p(P[l1 + "increase_dim.weight"]), _p(P[l1 + "increase_dim.bias"]), _p(P[l1 + "map_weights"]),
                _p(P[l2 + "lin_value.weight"]), _p(P[l2 + "lin_value.bias"]), _p(sn.ei), sn.E, _p(sn.ew), sn.E, _p(z), _p(mask),
                _p(ei2), _p(alpha), None, _p(buf), n, _p(ws), ws.numel(), st)
        out.append(("beta", lib.rd_beta_stage_saved_bytes(sp, E), lib.rd_beta_stage_infer_bytes(sp, E), beta,
                    lambda: (torch.equal(z, step.z) and torch.equal(mask, step.mask) and torch.equal(ei2, sn.ei2)
                             and torch.equal(alpha, sn.alpha)), True))
    else:
        W1, b1, W2, b2 = step.sensor._weights(P)
        z, mask = torch.zeros_like(step.z), torch.zeros_like(step.mask)

        def sensor(buf, n):
            rc = lib.rd_step_prepare(sp, 0, None, None, None, _p(W1), _p(W2), _p(buf), n, st)
            return rc or lib.rd_sensor_stage_fwd_infer(sp, _p(b["src"]), _p(b["times"]), _p(b["lengths"]), _p(step.ts), _p(P["R_u"]),
                                                       _p(W1), _p(b1), _p(W2), _p(b2), _p(step.graph_info["ssum"]), _p(z), _p(mask),
                                                       _p(buf), n, 1, st)
        out.append(("sensor", lib.rd_msgpass_saved_bytes(sp), lib.rd_msgpass_infer_bytes(sp), sensor,
                    lambda: torch.equal(z, step.z) and torch.equal(mask, step.mask), _covers(step)[0] == 1))
    y = torch.zeros_like(step.x[1])

    def encoder(buf, n):
        rc = lib.rd_encoder_layer_prepare(sp, ctypes.byref(step.enc_w[0]), _p(buf), n, st)
        return rc or lib.rd_encoder_layer_fwd_infer(sp, 0 | 0x10000, _p(step.x[0]), _p(step.mask), ctypes.byref(step.enc_w[0]), _p(y),
                                                    _p(buf), n, None, 0, st)
    out.append(("encoder", lib.rd_encoder_layer_saved_bytes(sp), lib.rd_encoder_layer_infer_bytes(sp), encoder,
                lambda: torch.equal(y, step.x[1]), _covers(step)[1] == 1))
    return out


@pytest.mark.parametrize("plan", [None, False], ids=["plan", "padded"])
@pytest.mark.parametrize("kw", [{}, {"use_beta": True}], ids=["default", "use_beta"])
def test_nothing_beyond_the_inference_size_is_written(kw, plan, precision_mode):
    """Each `_infer` entry point, told its buffer has the inference size, leaves every byte behind it alone (the buffer really has
    the training size, filled with 0xA5) and computes what the step's own forward computed; told 256 bytes less it returns
    RD_EINVAL without launching.  Where rd_infer_covers says 0 for a stage the entry point is the saving forward: not run here."""
    cfg, m = _model("P19", kw)
    step = EvalStep(m, _batch(cfg, 3), token_plan=plan, use_graph=False, save_free=True)
    step.run()                                                         # the step's z / mask / x[1]; with a plan: the plan tensor
    ran = []

    def body():
        for name, full, inf, call, same, covered in _stage_calls(step):
            if not covered:
                continue
            assert 0 < inf < full, (name, inf, full)
            buf = _sentinel(full)
            assert call(buf, inf - 256) == -1 and b"too small" in step.lib.rd_last_error(), name      # RD_EINVAL before any launch
            torch.cuda.synchronize()
            assert bool((buf == 0xA5).all()), name
            assert call(buf, inf) == 0, (name, step.lib.rd_last_error())
            torch.cuda.synchronize()
            assert bool((buf[inf:] == 0xA5).all()), name
            assert same(), name
            ran.append(name)
    step._with_cell(body)
    print(kw, precision_mode, "plan" if step.plan is not None else "padded", "checked:", ran)
    if precision_mode == "bf16x3":
        assert ran == (["beta", "encoder"] if kw else ["sensor", "encoder"])


@pytest.mark.parametrize("kw", [{}, BETA], ids=["default", "use_beta"])
def test_replay_sees_weights_changed_in_place(kw, precision_mode):
    """As tests/test_eval_step_gpu.py's, for the inference form at P19 B = 8: after `p.add_()` on every live parameter and after
    `load_state_dict` of another seed a replay equals a freshly built step -- of either form --, bit for bit."""
    cfg, m = _model("P19", kw)
    b = _batch(cfg, 8, seed=3)
    step = EvalStep(m, b, save_free=True)
    assert step.infer
    first = step.run().clone()
    live = synth.live_parameter_names_beta(cfg) if kw else synth.live_parameter_names(cfg)
    named = dict(m.named_parameters())
    with torch.no_grad():
        for i, n in enumerate(live):
            named[n].add_(1e-3 * (1 + i % 3))
    got = step.run().clone()
    assert torch.equal(got, EvalStep(m, b, save_free=True).run()) and torch.equal(got, EvalStep(m, b, save_free=False).run())
    assert not torch.equal(got, first)
    other = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 19, **kw)
    m.load_state_dict(other.state_dict())
    got = step.run().clone()
    dgot = None if step.distance is None else step.distance.clone()
    fresh = EvalStep(m, b, save_free=False)
    assert torch.equal(got, fresh.run()) and not torch.equal(got, first)
    if dgot is not None:
        assert torch.equal(dgot, fresh.distance)


def test_inference_between_training_replays_changes_nothing(precision_mode):
    """P19 B = 8, dropout on.  (1) As test_eval_step_leaves_the_training_state_alone: building and replaying an inference step
    leaves state_dict, p.grad and the seed cell alone.  (2) Interleaving: train, infer, train gives the gradients of train, train
    from the same seed cell -- inference touches neither the training step's saved buffers nor the per-thread registrations."""
    cfg = synth.make_config("P19")
    gs = synth.make_structure(cfg, "sparse")
    batch = synth.make_batch(cfg, 8, seed=11)
    dv = {k: (None if v is None else v.to(DEV)) for k, v in batch.items()}
    m = build_ours(cfg, gs, DEV, 7).train()
    named = dict(m.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)])
    ts = TrainStep(m, flat, dv, p_drop=0.2, autotune=False)
    ts.run()
    cell = ts.seed_cell.clone()
    loss_ref = float(ts.run())
    grads_ref = flat.flat.clone()
    ts.seed_cell.copy_(cell)                                           # rewind: the next replay draws the same masks
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    g0 = {n: p.grad.clone() for n, p in named.items() if p.grad is not None}
    es = EvalStep(m, _batch(cfg, 8, seed=12), save_free=True)
    assert es.infer
    es.run(); es.run()
    torch.cuda.synchronize()
    assert all(torch.equal(v, sd0[k]) for k, v in m.state_dict().items())
    assert all(torch.equal(named[n].grad, g) for n, g in g0.items())
    assert torch.equal(ts.seed_cell, cell) and m.training
    loss = float(ts.run())
    assert loss == loss_ref and torch.equal(flat.flat, grads_ref)
    es.run()
    ts.seed_cell.copy_(cell)
    assert float(ts.run()) == loss_ref and torch.equal(flat.flat, grads_ref)
    ts.close(); es.close()


@pytest.mark.parametrize("kw", [{}, {"use_beta": True}], ids=["default", "use_beta"])
def test_evaluate_captured_and_validate_equal_the_saving_form(kw, precision_mode):
    """70 samples at chunk 32: two full chunks and a remainder of 6.  Logits bit-equal, every metric of `validate` equal."""
    cfg = synth.make_config("P19")
    val = synth.make_batch(cfg, 70, seed=90)
    y = np.random.default_rng(90).integers(0, 2, 70)
    ds = feed.DeviceDataset(val["src"], val["times"], val["static"], y, device=DEV)
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 5, **kw).eval()
    a = feed.evaluate_captured(m, ds, chunk=32, save_free=True)
    b = feed.evaluate_captured(m, ds, chunk=32, save_free=False)
    assert a.shape == (70, 2) and torch.equal(a, b)
    steps = list(m._eval_steps.values())
    assert sorted((s.B, s.infer) for s in steps) == [(6, False), (6, True), (32, False), (32, True)]
    assert torch.equal(feed.evaluate_captured(m, ds, chunk=32), a)     # the default is the inference form, from the cache
    va = feed.validate(m, ds, chunk=32, save_free=True)
    vb = feed.validate(m, ds, chunk=32, save_free=False)
    assert set(va) == set(vb)
    for k in va:
        assert np.array_equal(np.asarray(va[k]), np.asarray(vb[k]), equal_nan=True), k
