"""GPU: the forward-only captured step (raindrop_amd/evalstep.py), `feed.evaluate_captured` and `feed.validate`.

Every test runs in both arithmetic modes (split-bf16 and exact fp32; the token plan exists in the bf16 modes only)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from raindrop_amd import _lib, dp, feed, synth
from raindrop_amd.evalstep import EvalStep
from tests import metrics_ref as R
from tests.helpers import BETA_CASES, MODEL_CASES, build_ours, case_inputs, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("src", "times", "lengths", "static")


@pytest.fixture(autouse=True, params=["bf16x3", "fp32"])
def precision_mode(request):
    _lib.call("rd_set_precision", 1 if request.param == "bf16x3" else 0)
    yield request.param
    _lib.call("rd_set_precision", 1)


def _dev_batch(batch):
    return {k: (None if batch.get(k) is None else batch[k].to(DEV).clone()) for k in KEYS}


def _eager(m, b):
    was = m.training
    m.eval()
    try:
        with torch.no_grad():
            out, distance, _ = m(b["src"], b["static"], b["times"], b["lengths"])
    finally:
        m.train(was)
    return out.clone(), distance.clone()


@pytest.mark.parametrize("name", MODEL_CASES + BETA_CASES)
def test_eval_step_vs_reference_fixtures(name, precision_mode):
    """EvalStep.run() against the reference's logits (dropout is zeroed in every fixture): 1e-4, the bound of test_model_vs_golden;
    the structure distance of the paper's branch within 1e-5 relative.  Both layouts where the plan exists."""
    g, meta = load_golden(name)
    cfg, gs, batch = case_inputs(meta)
    beta = name in BETA_CASES
    kw = dict(use_beta=True, compute_distance=True) if beta else {}
    m = build_ours(cfg, gs, DEV, meta["param_seed"], float(meta.get("param_scale", 1.0)), **kw).train()
    want = g["logits_eval"] if "logits_eval" in g else g["logits"]
    for plan in (None, False):
        step = EvalStep(m, _dev_batch(batch), token_plan=plan)
        got = step.run().cpu().numpy()
        err = float(np.abs(got - want).max())
        print(name, precision_mode, "plan" if step.plan is not None else "padded", "max |logits - reference| = %.3e" % err)
        assert err < 1e-4
        if beta:
            d, dref = float(step.distance), float(g["distance"])
            print("   distance %.8e reference %.8e" % (d, dref))
            assert abs(d - dref) <= 1e-5 * dref + 1e-7
        else:
            assert step.distance is None
        assert m.training                                         # the model's mode is left as found
        step.close()


@pytest.mark.parametrize("cfg_name,B,kw", [("P19", 48, {}), ("P12", 12, {}), ("PAM", 6, {}), ("P19", 48, {"use_beta": True, "compute_distance": True}),
                                           ("P12", 12, {"use_beta": True})], ids=["p19", "p12", "pam", "p19_beta_distance", "p12_beta"])
def test_eval_step_vs_eager_surface(cfg_name, B, kw, precision_mode):
    """Against `model.eval(); model.forward` on the same device.  Padded layout (token_plan=False): the step enqueues the eager
    surface's kernels in its order -- bit-equal logits (and distance): MEASURED 0.0 in every case and both modes.  On the token
    plan the bound is the one test_token_plan_beyond_the_p19_envelope documents for the logits, 2e-6 in split-bf16 (the plan does
    not exist in fp32 mode, where the default step is the padded one and bit-equal).  MEASURED on the plan: 0.0 in all four
    cases (PAM has no plan) -- the plan kernels produce the live rows' bits of the padded ones at these shapes and the head is the
    eager surface's on both layouts (rd_masked_mean_fwd follows the plan with the padded layout's summation order).  The plan's
    contract is the bound, not the bits, so the bound is what is asserted.  (With the fused fp32 head, rd_head_forward, the
    same comparison gave 2.2e-6 .. 3.0e-6: the head's arithmetic, not the plan -- why EvalStep does not use it.)"""
    cfg = synth.make_config(cfg_name)
    gs = synth.make_structure(cfg, "sparse")
    m = build_ours(cfg, gs, DEV, 7, **kw).eval()
    b = _dev_batch(synth.make_batch(cfg, B, seed=41))
    ref, dref = _eager(m, b)
    padded = EvalStep(m, b, token_plan=False)
    got = padded.run()
    print(cfg_name, kw, precision_mode, "padded max |diff| = %.3e" % float((got - ref).abs().max()))
    assert padded.plan is None and torch.equal(got, ref)
    if kw.get("compute_distance"):
        print("   distance step %.9e eager %.9e" % (float(padded.distance), float(dref)))
        assert torch.equal(padded.distance, dref)
    auto = EvalStep(m, b)
    got2 = auto.run()
    diff = float((got2 - ref).abs().max())
    print(cfg_name, kw, precision_mode, "plan" if auto.plan is not None else "padded", "max |diff| = %.3e" % diff)
    if auto.plan is None:
        assert torch.equal(got2, ref)
    else:
        assert precision_mode == "bf16x3" and not auto.head_fused
        assert diff < 2e-6
    padded.close(); auto.close()


def _p19_dataset(n, seed=90, labels=False):
    cfg = synth.make_config("P19")
    val = synth.make_batch(cfg, n, seed=seed)
    y = None
    if labels:
        y = np.random.default_rng(seed).integers(0, 2, n)
    return cfg, feed.DeviceDataset(val["src"], val["times"], val["static"], y, device=DEV)


@pytest.mark.parametrize("kw", [{}, {"use_beta": True}], ids=["default", "use_beta"])
def test_evaluate_captured_equals_evaluate_chunked(kw, precision_mode, monkeypatch):
    """1500 samples, chunk 512: two full chunks + a 476 remainder = two captured steps, reused by the second call.  Equal to
    `evaluate_chunked` under the rule of test_eval_step_vs_eager_surface: bit-equal padded (MEASURED 0.0), 2e-6 on the plan
    (MEASURED 0.0 over the 1500 samples, both branches)."""
    cfg, ds = _p19_dataset(1500)
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 5, **kw).train()
    ref = feed.evaluate_chunked(m, ds, chunk=512)
    for plan_env in ("1", "0"):
        monkeypatch.setenv("RD_TOKEN_PLAN", plan_env)
        m.__dict__.pop("_eval_steps", None)
        out = feed.evaluate_captured(m, ds, chunk=512)
        steps = dict(m._eval_steps)
        assert sorted(s.B for s in steps.values()) == [476, 512] and all(s.captures == 1 for s in steps.values())
        out2 = feed.evaluate_captured(m, ds, chunk=512)
        assert dict(m._eval_steps) == steps and all(s.captures == 1 for s in steps.values())
        assert torch.equal(out, out2) and out.shape == (1500, 2) and m.training
        diff = float((out - ref).abs().max())
        on_plan = all(s.plan is not None for s in steps.values())
        print(kw, precision_mode, "RD_TOKEN_PLAN=" + plan_env, "plan" if on_plan else "padded", "max |diff| = %.3e" % diff)
        if on_plan:
            assert plan_env == "1" and diff < 2e-6
        else:
            assert torch.equal(out, ref)


@pytest.mark.parametrize("kw", [{}, {"use_beta": True, "compute_distance": True}], ids=["default", "use_beta"])
def test_replay_sees_weights_changed_in_place(kw, precision_mode):
    """The graph reads the parameters by address and rebuilds the weight tiles in its first launch: after `p.add_()` on every live
    parameter and after `load_state_dict` of another seed a replay equals a freshly built EvalStep, bit for bit."""
    cfg = synth.make_config("P19")
    gs = synth.make_structure(cfg, "sparse")
    m = build_ours(cfg, gs, DEV, 7, **kw).eval()
    b = _dev_batch(synth.make_batch(cfg, 32, seed=3))
    step = EvalStep(m, b)
    first = step.run().clone()
    live = synth.live_parameter_names_beta(cfg) if kw else synth.live_parameter_names(cfg)
    named = dict(m.named_parameters())
    with torch.no_grad():
        for i, n in enumerate(live):
            named[n].add_(1e-3 * (1 + i % 3))
    got = step.run().clone()
    fresh = EvalStep(m, b)
    assert torch.equal(got, fresh.run()) and not torch.equal(got, first)
    other = build_ours(cfg, gs, DEV, 19, **kw)
    m.load_state_dict(other.state_dict())
    got = step.run().clone()
    dgot = None if step.distance is None else step.distance.clone()
    fresh2 = EvalStep(m, b)
    assert torch.equal(got, fresh2.run()) and not torch.equal(got, first)
    if dgot is not None:
        assert torch.equal(dgot, fresh2.distance)
    m2 = m.to("cpu").to(DEV)                                       # moved parameters are refused, as TrainStep does
    if any(p.data_ptr() != q for p, q in zip(m.parameters(), step._ptrs)):
        with pytest.raises(_lib.RaindropHipError):
            step.run()


def test_eval_step_leaves_the_training_state_alone(precision_mode):
    """Constructing and running an EvalStep between two TrainStep replays (dropout on) changes nothing the training run can see:
    state_dict, every p.grad, and the next replay's loss and gradients are bit-identical to a run without it."""
    from raindrop_amd.step import TrainStep
    cfg = synth.make_config("P19")
    gs = synth.make_structure(cfg, "sparse")
    batch = synth.make_batch(cfg, 32, seed=11)
    dv = {k: (None if v is None else v.to(DEV)) for k, v in batch.items()}

    def run(with_eval):
        m = build_ours(cfg, gs, DEV, 7).train()
        named = dict(m.named_parameters())
        flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)])
        ts = TrainStep(m, flat, dv, p_drop=0.2, autotune=False)
        ts.run()
        if with_eval:
            sd0 = {k: v.clone() for k, v in m.state_dict().items()}
            g0 = {n: p.grad.clone() for n, p in named.items() if p.grad is not None}
            cell0 = ts.seed_cell.clone()
            es = EvalStep(m, _dev_batch(batch))
            es.run(); es.run()
            torch.cuda.synchronize()
            assert all(torch.equal(v, sd0[k]) for k, v in m.state_dict().items())
            assert all(torch.equal(named[n].grad, g) for n, g in g0.items())
            assert {n for n, p in named.items() if p.grad is not None} == set(g0)
            assert torch.equal(ts.seed_cell, cell0) and m.training
        loss = float(ts.run())
        out = (loss, flat.flat.clone())
        ts.close()
        return out
    la, ga = run(False)
    lb, gb = run(True)
    assert la == lb and torch.equal(ga, gb)


@pytest.mark.parametrize("transform", ["sigmoid", "softmax", None])
def test_validate_against_host_computation(transform, precision_mode, monkeypatch):
    """`validate` = eager logits -> torch transform -> the numpy restatement of the metrics, with the logits bit-equal (padded
    layout): metrics within 1e-10, loss within 1e-5 of torch's cross entropy on the same scores, and ONE device-to-host read."""
    monkeypatch.setenv("RD_TOKEN_PLAN", "0")
    cfg, ds = _p19_dataset(1500, labels=True)
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 5).eval()
    logits = feed.evaluate_chunked(m, ds, chunk=512)
    scores = torch.sigmoid(logits) if transform == "sigmoid" else torch.softmax(logits, 1) if transform == "softmax" else logits
    loss_ref = float(torch.nn.functional.cross_entropy(scores, ds.y))
    s, y = scores.cpu().numpy(), ds.y.cpu().numpy()
    feed.validate(m, ds, transform=transform, chunk=512)            # captures happen here
    counts = {"cpu": 0, "item": 0, "tolist": 0}
    for name in counts:
        orig = getattr(torch.Tensor, name)

        def wrap(self, *a, _n=name, _o=orig, **k):
            counts[_n] += 1
            return _o(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, wrap)
    v = feed.validate(m, ds, transform=transform, chunk=512)
    monkeypatch.undo()
    assert counts == {"cpu": 1, "item": 0, "tolist": 0}, counts
    ref = R.rank_metrics_ref(s, y)
    print(transform, precision_mode, "auroc %.12f ref %.12f  auprc %.12f ref %.12f  loss %.8f ref %.8f" % (
        v["auroc"], ref["auroc"][1], v["auprc"], ref["auprc"][1], v["loss"], loss_ref))
    assert abs(v["auroc"] - ref["auroc"][1]) <= 1e-10 and abs(v["auprc"] - ref["auprc"][1]) <= 1e-10
    assert np.abs(v["auroc_per_class"] - ref["auroc"]).max() <= 1e-10 and np.abs(v["auprc_per_class"] - ref["auprc"]).max() <= 1e-10
    cm = R.confusion_ref(s, y)
    assert np.array_equal(v["confusion"], cm) and v["accuracy"] == float(np.trace(cm)) / 1500
    assert abs(v["loss"] - loss_ref) < 1e-5


# ---- process groups: two ranks sharing cuda:0 over gloo (the pattern of tests/test_dp_gpu.py), and nccl on a one-rank group ----

def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _captured_logits(precision, group=False):
    _lib.call("rd_set_precision", precision)
    cfg = synth.make_config("P19")
    val = synth.make_batch(cfg, 101, seed=90)                      # odd size: the last shard is shorter
    ds = feed.DeviceDataset(val["src"], val["times"], val["static"], None, device=DEV)
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 5).eval()
    out = feed.evaluate_captured(m, ds, chunk=32, group=dist.group.WORLD if group else None)
    return out.cpu().numpy().copy()


def _group_worker(rank, world, port, backend, precision, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    ret[rank] = _captured_logits(precision, group=True)
    dist.destroy_process_group()


@pytest.mark.parametrize("backend,world", [("gloo", 2), ("nccl", 1)])
def test_evaluate_captured_over_a_process_group(backend, world, precision_mode):
    """Contiguous shards + all-gather (staged through the host for gloo) == the single-process result on every rank, bit for bit.
    nccl on a one-rank group only: no claim about real peers."""
    precision = 1 if precision_mode == "bf16x3" else 0
    ref = _captured_logits(precision)
    port = _free_port()
    ret = mp.Manager().dict()
    mp.spawn(_group_worker, args=(world, port, backend, precision, ret), nprocs=world, join=True)
    assert ret[0].shape == (101, 2)
    for r in range(world):
        assert np.array_equal(ret[r], ref), r
