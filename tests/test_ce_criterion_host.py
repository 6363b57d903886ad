"""CPU: the host side of class weights / label smoothing in the steps' cross entropy -- the accepted criterion values, the C-ABI
triple (header, binding, export) of the two new entry points, the build-time resources of the new kernel instantiations, and which
entry points a step's head enqueues with and without a criterion."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

from raindrop_amd import _lib, build, feed, ops, step as step_mod, step_beta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rd_softmax_xent_crit", "rd_head_train_crit")


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def test_new_symbols_are_declared_bound_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "raindrop_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # one pointer (the criterion) more than the plain entry points
    assert len(_lib.SIGNATURES["rd_head_train_crit"][1]) == len(_lib.SIGNATURES["rd_head_train"][1]) + 1
    assert len(_lib.SIGNATURES["rd_softmax_xent_crit"][1]) == len(_lib.SIGNATURES["rd_softmax_xent"][1]) + 1


def test_argument_errors_are_reported_before_launch(lib):
    one = ctypes.c_void_p(256)                                     # never dereferenced
    assert lib.rd_softmax_xent_crit(0, 2, one, one, one, one, one, None) == -1 and b"bad dims" in lib.rd_last_error()
    assert lib.rd_softmax_xent_crit(4, 2, one, one, None, one, one, None) == -1 and b"NULL" in lib.rd_last_error()
    shp = _lib.shape(4, 6, 1, 4)
    args = [ctypes.byref(shp), 16, 2, 4, 2] + [one] * 21 + [one, 1 << 20, None]
    args[5 + 11] = None                                            # crit
    assert lib.rd_head_train_crit(*args) == -1 and b"NULL" in lib.rd_last_error()
    # support test and workspace query keep their values for the criterion form
    assert lib.rd_head_train_supported(152, 34, 2) == 1 and lib.rd_head_train_supported(152, 34, 17) == 0
    assert lib.rd_head_train_workspace_bytes(256, 186, 2) == ((4 * 256 * 186 + 256 * 2 + 256) * 4 + 255) // 256 * 256


def test_criterion_instantiations_use_no_scratch(lib):
    """the CRIT = true instantiations of k_head_rows and the stand-alone kernel: ScratchSize 0, no VGPR spill, at most 128 VGPRs
    (1024-thread workgroups); the plain instantiations exist beside them"""
    usage = build.resource_usage()
    crit = {k: v for k, v in usage.items() if re.search(r"k_head_rowsILi1ELi\d+ELi\dELb1E", k)}
    plain = {k: v for k, v in usage.items() if re.search(r"k_head_rowsILi1ELi\d+ELi\dELb0E", k)}
    assert len(crit) == 2 and len(plain) == 2
    for name, u in list(crit.items()) + [(k, v) for k, v in usage.items() if "k_softmax_xent_crit" in k]:
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["vgprs"] <= 128, (name, u)
    assert any("k_softmax_xent_crit" in k for k in usage)
    sites = {s for s, _, _ in build.TOUCH_SITES}
    assert {"HEAD_P19", "HEAD", "HEAD_P19_C", "HEAD_C"} <= sites


def test_criterion_values():
    cv = step_mod.criterion_values
    assert cv(None, 0.0, 2) is None
    assert cv(None, 0.1, 3) == [0.1, 1.0, 1.0, 1.0]
    assert cv([0.5, 2.0], 0.0, 2) == [0.0, 0.5, 2.0]
    assert cv(torch.tensor([1.0, 0.0]), 0, 2) == [0.0, 1.0, 0.0]           # a zero weight is allowed
    assert cv((1, 3), 0.25, 2) == [0.25, 1.0, 3.0]
    for bad_w in ([1.0], [1.0, 2.0, 3.0], [1.0, -0.5], [1.0, float("nan")], [float("inf"), 1.0], [1e39, 1.0], torch.ones(2, 1)):
        with pytest.raises(ValueError):
            cv(bad_w, 0.0, 2)
    for bad_eps in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            cv(None, bad_eps, 2)
        with pytest.raises(ValueError):
            cv([1.0, 1.0], bad_eps, 2)


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.6])
def test_autograd_step_criterion_is_torch_s(eps):
    """AutogradStep._criterion -- with smoothing a capturable restatement of torch's weighted, smoothed mean cross entropy -- against
    F.cross_entropy in float64: value and gradient to 1e-12 (one class absent from the batch, one present class of weight 0)"""
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(11, 4, generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    y = torch.tensor([0, 1, 2, 0, 0, 1, 2, 2, 1, 0, 2])
    w = torch.tensor([0.7, 0.0, 2.5, 1.3], dtype=torch.float64)
    s = object.__new__(step_mod.AutogradStep)
    s._crit = (eps, w)
    got = s._criterion(logits, y)
    ref = torch.nn.functional.cross_entropy(logits, y, weight=w, label_smoothing=eps)
    gg, = torch.autograd.grad(got, logits)
    gr, = torch.autograd.grad(ref, logits)
    assert abs(float(got) - float(ref)) <= 1e-12 * abs(float(ref)) and float((gg - gr).abs().max()) <= 1e-12
    s._crit = None
    assert float(s._criterion(logits, y)) == float(torch.nn.functional.cross_entropy(logits, y))


def test_keywords_exist_with_plain_defaults():
    for fn in (step_mod.Step.__init__, step_mod.TrainStep.__init__, step_beta.BetaTrainStep.__init__, step_mod.AutogradStep.__init__,
               feed.validate, step_mod.Step.set_criterion):
        sig = inspect.signature(fn).parameters
        assert sig["class_weight"].default is None and sig["label_smoothing"].default == 0.0, fn


@pytest.mark.parametrize("kw", [dict(class_weight=[1.0]), dict(class_weight=[1.0, -2.0]), dict(class_weight=[1.0, float("nan")]),
                                dict(label_smoothing=1.0), dict(class_weight=[1.0, 1.0], label_smoothing=-0.5)])
def test_constructors_refuse_bad_criteria_before_anything_else(kw):
    """ValueError at construction -- before the batch is looked at, so it needs no device"""
    model = types.SimpleNamespace(n_classes=2, transformer_encoder=types.SimpleNamespace(layers=[0, 1]))
    with pytest.raises(ValueError):
        step_mod.TrainStep(model, None, {}, use_graph=False, split=False, **kw)
    with pytest.raises(ValueError):
        step_mod.AutogradStep(model, {}, **kw)
    with pytest.raises(ValueError):
        step_mod.Step(model, {}, step_mod.SensorStage(), **kw)


def test_forward_only_and_module_steps_refuse_a_criterion():
    model = types.SimpleNamespace(n_classes=2, transformer_encoder=types.SimpleNamespace(layers=[0, 1]))
    with pytest.raises(ValueError, match="evaluates the loss itself"):
        step_mod.Step(model, {}, step_mod.SensorStage(), has_backward=False, class_weight=[1.0, 2.0])
    with pytest.raises(ValueError, match="evaluates the loss itself"):
        step_mod.TrainStep(model, None, {}, use_graph=False, split=False, module_mode=True, label_smoothing=0.1)


def _bare_step(fused, crit, monkeypatch):
    """a Step with the attributes its head stages read (host tensors: only their addresses are taken) and a recording `_call`"""
    monkeypatch.setattr(ops, "_stream", lambda: None)
    B, T, D, C = 3, 4, 8, 2
    z = lambda *sh: torch.zeros(*sh)
    s = object.__new__(step_mod.Step)
    s.model = types.SimpleNamespace(n_classes=C, d_static=0)
    s.batch = {"y": torch.zeros(B, dtype=torch.int64), "lengths": torch.ones(B, dtype=torch.int64), "static": None}
    names = ["mlp_static.0.weight", "mlp_static.0.bias", "mlp_static.2.weight", "mlp_static.2.bias"]
    s.P, s.G = {n: z(4) for n in names}, {n: z(4) for n in names}
    s.B, s.T, s.D, s.Fe, s.nl, s.sp = B, T, D, 0, 2, None
    s.x, s.dx, s.mask = [z(T, B, D)] * 3, [z(T, B, D), z(T, B, D)], z(B, T)
    s.feat, s.dfeat, s.hid, s.dhid, s.logits, s.dlogits = z(B, D), z(B, D), z(B, D), z(B, D), z(B, C), z(B, C)
    s.loss, s.wg_ws, s.head_ws = z(()), torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    s.head_fused, s.crit, s.focal = fused, crit, None
    s.calls = []
    s._call = lambda name, *a: s.calls.append((name, a))
    return s


@pytest.mark.parametrize("fused", [True, False])
def test_a_step_without_a_criterion_calls_neither_crit_entry_point(fused, monkeypatch):
    s = _bare_step(fused, None, monkeypatch)
    s._head_train()
    names = [n for n, _ in s.calls]
    assert not any(n.endswith("_crit") for n in names), names
    assert names == ["rd_head_train"] if fused else ("rd_softmax_xent" in names and names[0] == "rd_masked_mean_fwd")
    with pytest.raises(_lib.RaindropHipError, match="plain mean cross entropy"):
        s.set_criterion(class_weight=[1.0, 2.0])
    assert s.crit is None and not any(n.endswith("_crit") for n, _ in s.calls)


@pytest.mark.parametrize("fused", [True, False])
def test_a_step_with_a_criterion_hands_its_buffer_to_the_crit_entry_point(fused, monkeypatch):
    crit = torch.tensor([0.1, 1.0, 2.0])
    s = _bare_step(fused, crit, monkeypatch)
    s._head_train()
    calls = dict(s.calls)
    name = "rd_head_train_crit" if fused else "rd_softmax_xent_crit"
    other = [n for n in calls if n in ("rd_head_train", "rd_softmax_xent")]
    assert name in calls and not other
    pos = 5 + 11 if fused else 4                                    # `crit` follows `y`
    assert calls[name][pos - 1].value == s.batch["y"].data_ptr() and calls[name][pos].value == crit.data_ptr()
    assert len(calls[name]) == len(_lib.SIGNATURES[name][1])
    # set_criterion: a copy into the SAME buffer, validated like the constructor's arguments
    s.set_criterion(class_weight=[3.0, 0.5], label_smoothing=0.2)
    assert s.crit is crit and torch.equal(crit, torch.tensor([0.2, 3.0, 0.5]))
    s.set_criterion()                                               # the constructor's defaults: the neutral criterion
    assert torch.equal(crit, torch.tensor([0.0, 1.0, 1.0]))
    for kw in (dict(class_weight=[1.0]), dict(class_weight=[1.0, -1.0]), dict(class_weight=[float("nan"), 1.0]), dict(label_smoothing=1.0)):
        with pytest.raises(ValueError):
            s.set_criterion(**kw)
    assert torch.equal(crit, torch.tensor([0.0, 1.0, 1.0]))         # a refused call changes nothing
