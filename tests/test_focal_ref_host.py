"""CPU: the focal loss's float64 reference (tests/focal_ref.py) held to torch, wrong kernels that must miss its bounds, and the host
side of `focal_gamma=`: accepted values, refusals, the route, the C-ABI triple and the compiler's resource report."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from raindrop_amd import _lib, build, feed, step as step_mod, step_beta, trainer
from tests import focal_ref as FR
from tests import head_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rd_softmax_xent_focal", "rd_head_train_focal")


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


# ---- 1. the reference against torch ---------------------------------------------------------------------------------------------------------
def _moderate(B=23, C=5, seed=3):
    """logits whose 1 - p_y stays above 1e-6, so that torch's naive (1 - p_y)^gamma is itself accurate"""
    g = np.random.default_rng(seed)
    z = 2.0 * g.standard_normal((B, C))
    y = g.integers(0, C - 1, size=B).astype(np.int64)                  # the last class is absent
    y[:C - 1] = np.arange(C - 1)
    w = g.uniform(0.5, 1.5, size=C)
    w[1] = 0.0
    return z, y, w


def test_gamma_zero_is_torch_cross_entropy():
    z, y, w = _moderate()
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    for wt in (w, np.ones_like(w)):
        loss, dlog = FR.loss_and_dlogits(z, y, wt, 0.0)
        ref = torch.nn.CrossEntropyLoss(weight=torch.tensor(wt))(zt, torch.tensor(y))
        gr, = torch.autograd.grad(ref, zt)
        assert abs(float(loss) - float(ref)) <= 1e-12 and float(np.abs(dlog - gr.numpy()).max()) <= 1e-12
    plain = torch.nn.functional.cross_entropy(zt, torch.tensor(y))
    assert abs(float(FR.loss_and_dlogits(z, y, np.ones_like(w), 0.0)[0]) - float(plain)) <= 1e-12


@pytest.mark.parametrize("gamma", [0.5, 1.0, 2.0, 5.0])
def test_reference_is_torch_autograd_of_the_textbook_form(gamma):
    z, y, w = _moderate()
    zt, yt, wt = torch.tensor(z, dtype=torch.float64, requires_grad=True), torch.tensor(y), torch.tensor(w)
    logp = torch.log_softmax(zt, 1).gather(1, yt[:, None])[:, 0]
    assert float((1 - logp.exp()).min()) > 1e-6
    ref = -(wt[yt] * (1 - logp.exp()) ** gamma * logp).sum() / wt[yt].sum()
    gr, = torch.autograd.grad(ref, zt)
    loss, dlog = FR.loss_and_dlogits(z, y, w, gamma)
    assert abs(float(loss) - float(ref)) <= 1e-10 and float(np.abs(dlog - gr.numpy()).max()) <= 1e-10


def test_confident_rows_are_exact_zeros_and_never_nan():
    """q == 0 (fp32: a logit gap of 130) with gamma > 0: factor and gradient are exactly 0, also for gamma < 1 where q^(gamma - 1) is
    infinite; gamma == 0 keeps the cross entropy's row"""
    c = FR.op_case(64, 8)
    for gamma in (0.5, 1.0, 2.0, 5.0):
        loss, dlog = FR.loss_and_dlogits(c["logits"], c["y"], c["w"], gamma, np.float32)
        assert np.isfinite(loss) and np.isfinite(dlog).all() and not dlog[c["confident"]].any()
    assert np.isfinite(FR.loss_and_dlogits(c["logits"], c["y"], c["w"], 0.0, np.float32)[1]).all()


# ---- 2. the bounds bite -----------------------------------------------------------------------------------------------------------------------
def _variant_case(variant):
    if variant == "q_one_minus_py_f32":
        # every row confidently right with a gap of 14 .. 18: q ~ 1e-7, where fp32's 1 - p_y is 0 or one ulp of 1
        g = np.random.default_rng(11)
        B, C = 6, 3
        y = np.array([0, 1, 2, 0, 1, 2])
        z = g.standard_normal((B, C))
        z[np.arange(B), y] += g.uniform(14, 18, size=B)
        return z.astype(np.float32), y, np.ones(C, dtype=np.float32), 0.5
    c = FR.op_case(64, 8)
    return c["logits"], c["y"], c["w"], 2.0


@pytest.mark.parametrize("variant", FR.VARIANTS)
def test_wrong_kernels_miss_the_bounds(variant):
    z, y, w, gamma = _variant_case(variant)
    ref64 = dict(zip(FR.OP_TENSORS, FR.loss_and_dlogits(z, y, w, gamma)))
    ref32 = dict(zip(FR.OP_TENSORS, FR.loss_and_dlogits(z, y, w, gamma, np.float32)))
    # the rounded difference is the ONLY fp32 step of that variant (everything else float64), so the miss is q's alone: on such a batch
    # p_y - 1 and lse - z_y cancel in fp32 as well, in any kernel, and the 2e-5 ceiling is what the variant is held to
    isolated = variant == "q_one_minus_py_f32"
    wrong = dict(zip(FR.OP_TENSORS, FR.loss_and_dlogits(z, y, w, gamma, np.float64 if isolated else np.float32, variant=variant)))
    if not isolated:
        right = FR.op_compare(ref32, ref64, ref32)
        assert all(e <= b for _, e, b, _ in right), right              # the fp32 evaluation itself passes
    rows = FR.op_compare(wrong, ref64, ref32)
    assert max(e / b for _, e, b, _ in rows) > 10.0, (variant, rows)


def test_wrong_head_misses_the_bounds_through_the_whole_chain():
    name, gamma = "DH186", 2.0
    got = FR.evaluate(FR.case(name), gamma, np.float32, variant="g_first_term_only")
    rows, _ = FR.compare(name, gamma, got)
    worst = {t: e / b for t, e, b, _ in rows}
    assert all(worst[t] > 10.0 for t in HR.GRADS), worst
    ok, nonzero = FR.compare(name, gamma, FR.reference(name, gamma, np.float32))
    assert all(e <= b for _, e, b, _ in ok) and not nonzero


def test_every_head_run_is_a_head_ref_case_with_decisive_gates():
    for name, gamma in FR.HEAD_RUNS:
        assert gamma in FR.GAMMAS + FR.SMALL_GAMMAS and FR.gate_margin(name) >= HR.GATE_MARGIN, name
    cs = [FR.case(n) for n, _ in FR.HEAD_RUNS]
    assert {186, 192, 193, 256} <= {c["dh"] for c in cs}
    assert {c["B"] for c in cs} >= {1, 3, 257, 1025} and {c["T"] for c in cs} >= {1, 5, 65}
    assert {c["C"] for c in cs} >= {2, 16} and {c["Fe"] == 0 for c in cs} == {True, False}
    assert any(c["layout"] == "plan" and 0 in c["lengths"] for c in cs)
    assert not set(FR.LOCAL_CASES) & set(HR.CASES)                      # head_ref's tables are left as they are


def test_small_gamma_at_a_gap_near_100_is_finite_in_fp32():
    """the hazard of gamma < 1 beyond q == 0: q a positive denormal, lse - z_y already 0, q^(gamma - 1) beyond the largest float.  The
    fp32 evaluation (the yardstick) must be finite there, exactly as the float64 one, and pass its own bounds."""
    c = FR.small_gamma_case()
    z32 = c["logits"]
    lse = np.log(np.exp(z32 - z32.max(1, keepdims=True)).sum(1, dtype=np.float32)) + z32.max(1)
    assert ((lse - z32[np.arange(c["B"]), c["y"]])[[0, 2, 5]] == 0).all()                 # lse - z_y has rounded to 0 on those rows
    for gamma in FR.SMALL_GAMMAS:
        with np.errstate(over="ignore"):
            assert np.isinf(np.exp(np.float32(gamma - 1) * np.log(np.float32(1e-44))))     # and the power overflows
        r64 = dict(zip(FR.OP_TENSORS, FR.loss_and_dlogits(c["logits"], c["y"], c["w"], gamma)))
        r32 = dict(zip(FR.OP_TENSORS, FR.loss_and_dlogits(c["logits"], c["y"], c["w"], gamma, np.float32)))
        for r in (r64, r32):
            assert np.isfinite(r["loss"]) and np.isfinite(r["dlogits"]).all(), gamma
        assert all(e <= b for _, e, b, _ in FR.op_compare(r32, r64, r32))
    # the smallest such batch: one row at a gap of 100 beside an ordinary one
    _, d = FR.loss_and_dlogits([[100, 0], [.3, .1]], [0, 1], np.ones(2), 0.1, np.float32)
    assert np.isfinite(d).all()
    for gamma in FR.SMALL_GAMMAS:
        r32 = FR.reference("FOCAL_GAP100", gamma, np.float32)
        assert all(np.isfinite(r32[t]).all() for t in ("loss",) + HR.COMPARED), gamma
        gap = np.abs(np.diff(FR.reference("FOCAL_GAP100", gamma)["logits"], axis=1))
        assert (gap > 90).all() and (gap < 110).all(), gap


# ---- 3. accepted values and refusals ------------------------------------------------------------------------------------------------------------
def test_focal_values():
    fv = step_mod.focal_values
    assert fv(None, 0.0, 2) == [0.0, 1.0, 1.0] and fv(None, 2, 3) == [2.0, 1.0, 1.0, 1.0]
    assert fv([0.5, 2.0], 16.0, 2) == [16.0, 0.5, 2.0] and fv(torch.tensor([1.0, 0.0]), 0.5, 2) == [0.5, 1.0, 0.0]
    for bad in (-0.1, 16.5, float("nan"), float("inf"), None, "two", True):
        with pytest.raises(ValueError):
            fv(None, bad, 2)
    for bad_w in ([1.0], [1.0, 2.0, 3.0], [1.0, -0.5], [1.0, float("nan")], torch.ones(2, 1)):
        with pytest.raises(ValueError):
            fv(bad_w, 2.0, 2)
    assert step_mod.criterion_values(None, 0.0, 2) is None and step_mod.criterion_values([1, 3], 0.25, 2) == [0.25, 1.0, 3.0]


def test_keywords_exist_and_default_to_none():
    for fn in (step_mod.Step.__init__, step_mod.TrainStep.__init__, step_beta.BetaTrainStep.__init__, step_mod.AutogradStep.__init__,
               feed.validate, step_mod.Step.set_criterion, trainer.fit):
        assert inspect.signature(fn).parameters["focal_gamma"].default is None, fn


@pytest.mark.parametrize("kw", [dict(focal_gamma=-1.0), dict(focal_gamma=17.0), dict(focal_gamma=float("nan")),
                                dict(focal_gamma=2.0, label_smoothing=0.1), dict(focal_gamma=0.0, label_smoothing=0.1),
                                dict(focal_gamma=2.0, class_weight=[1.0]), dict(focal_gamma=2.0, class_weight=[1.0, -2.0])])
def test_constructors_refuse_bad_focal_arguments_before_anything_else(kw):
    model = types.SimpleNamespace(n_classes=2, transformer_encoder=types.SimpleNamespace(layers=[0, 1]))
    with pytest.raises(ValueError):
        step_mod.TrainStep(model, None, {}, use_graph=False, split=False, **kw)
    with pytest.raises(ValueError):
        step_mod.AutogradStep(model, {}, **kw)
    with pytest.raises(ValueError):
        step_mod.Step(model, {}, step_mod.SensorStage(), **kw)


def test_label_smoothing_with_focal_gamma_is_refused_by_name():
    model = types.SimpleNamespace(n_classes=2, transformer_encoder=types.SimpleNamespace(layers=[0, 1]))
    with pytest.raises(ValueError, match="label_smoothing.*focal_gamma"):
        step_mod.Step(model, {}, step_mod.SensorStage(), focal_gamma=2.0, label_smoothing=0.1)
    with pytest.raises(ValueError, match="evaluates the loss itself"):
        step_mod.Step(model, {}, step_mod.SensorStage(), has_backward=False, focal_gamma=2.0)


def test_check_fit_args_refuses_what_needs_no_device():
    ds = types.SimpleNamespace(y=torch.zeros(4, dtype=torch.int64))
    ok = (ds, ds, 1, 4, 2)
    trainer._check_fit_args(*ok)
    trainer._check_fit_args(*ok, focal_gamma=2.0)
    trainer._check_fit_args(*ok, focal_gamma=0.0, label_smoothing=0.0)
    for kw in (dict(focal_gamma=-0.5), dict(focal_gamma=16.1), dict(focal_gamma=float("nan")), dict(focal_gamma="2"),
               dict(focal_gamma=2.0, label_smoothing=0.1)):
        with pytest.raises(ValueError):
            trainer._check_fit_args(*ok, **kw)


def _bare_step(fused, focal, monkeypatch):
    from raindrop_amd import ops
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
    s.head_fused, s.crit, s.focal = fused, None, focal
    s.calls = []
    s._call = lambda name, *a: s.calls.append((name, a))
    return s


@pytest.mark.parametrize("fused", [True, False])
def test_a_focal_step_hands_its_buffer_to_the_focal_entry_point(fused, monkeypatch):
    focal = torch.tensor([2.0, 1.0, 3.0])
    s = _bare_step(fused, focal, monkeypatch)
    s._head_train()
    calls = dict(s.calls)
    name = "rd_head_train_focal" if fused else "rd_softmax_xent_focal"
    assert name in calls and not [n for n in calls if n in ("rd_head_train", "rd_softmax_xent") or n.endswith("_crit")]
    pos = 5 + 11 if fused else 4                                    # the buffer follows `y`
    assert calls[name][pos - 1].value == s.batch["y"].data_ptr() and calls[name][pos].value == focal.data_ptr()
    assert len(calls[name]) == len(_lib.SIGNATURES[name][1])
    s.set_criterion(class_weight=[3.0, 0.5], focal_gamma=0.5)        # a copy into the SAME buffer
    assert s.focal is focal and torch.equal(focal, torch.tensor([0.5, 3.0, 0.5]))
    s.set_criterion(focal_gamma=0.0)
    assert torch.equal(focal, torch.tensor([0.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="label_smoothing"):
        s.set_criterion(focal_gamma=1.0, label_smoothing=0.1)
    with pytest.raises(ValueError, match="label_smoothing"):
        s.set_criterion(label_smoothing=0.1)
    with pytest.raises(_lib.RaindropHipError, match="built for the focal loss"):
        s.set_criterion(class_weight=[1.0, 2.0])
    for kw in (dict(focal_gamma=17.0), dict(focal_gamma=1.0, class_weight=[1.0]), dict(focal_gamma=1.0, class_weight=[1.0, -1.0])):
        with pytest.raises(ValueError):
            s.set_criterion(**kw)
    assert torch.equal(focal, torch.tensor([0.0, 1.0, 1.0]))         # a refused call changes nothing


def test_steps_not_built_focal_refuse_focal_gamma(monkeypatch):
    for crit in (None, torch.tensor([0.0, 1.0, 1.0])):
        s = _bare_step(True, None, monkeypatch)
        s.crit = crit
        with pytest.raises(_lib.RaindropHipError, match="not built for the focal loss"):
            s.set_criterion(focal_gamma=2.0)
        s._head_train()
        assert not any(n.endswith("_focal") for n, _ in s.calls)


def test_autograd_step_focal_criterion_is_the_reference():
    z, y, w = _moderate()
    s = object.__new__(step_mod.AutogradStep)
    s._crit = None
    for gamma in (0.0, 0.5, 2.0):
        s._focal = (gamma, torch.tensor(w))
        zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
        got = s._criterion(zt, torch.tensor(y))
        gg, = torch.autograd.grad(got, zt)
        loss, dlog = FR.loss_and_dlogits(z, y, w, gamma)
        assert abs(float(got) - float(loss)) <= 1e-12 and float(np.abs(gg.numpy() - dlog).max()) <= 1e-12


# ---- 4. the library: symbols, argument errors, route, resources ----------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "raindrop_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.SIGNATURES["rd_head_train_focal"] == _lib.SIGNATURES["rd_head_train_crit"]
    assert _lib.SIGNATURES["rd_softmax_xent_focal"] == _lib.SIGNATURES["rd_softmax_xent_crit"]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in integration for name in NEW)


def test_argument_errors_are_reported_before_launch(lib):
    one = ctypes.c_void_p(256)                                     # never dereferenced
    assert lib.rd_softmax_xent_focal(0, 2, one, one, one, one, one, None) == -1 and b"bad dims" in lib.rd_last_error()
    assert lib.rd_softmax_xent_focal(4, 2, one, one, None, one, one, None) == -1 and b"NULL" in lib.rd_last_error()
    assert lib.rd_softmax_xent_focal(1 << 24, 2, one, one, one, one, one, None) == -1
    shp = _lib.shape(4, 6, 1, 4)
    args = [ctypes.byref(shp), 16, 2, 4, 2] + [one] * 21 + [one, 1 << 20, None]
    args[5 + 11] = None                                            # the focal buffer
    assert lib.rd_head_train_focal(*args) == -1 and b"NULL" in lib.rd_last_error()
    big = _lib.shape(1 << 24, 6, 1, 4)
    args = [ctypes.byref(big), 16, 2, 4, 2] + [one] * 21 + [one, 1 << 20, None]
    assert lib.rd_head_train_focal(*args) == -1 and b"2^24" in lib.rd_last_error()


def _route(lib, mode, B, D, ds, Fe, C, form):
    words, name = (ctypes.c_uint32 * 11)(), ctypes.create_string_buffer(64)
    rc = lib.rd_debug_head_route(mode, B, D, ds, Fe, C, form, words, name, len(name))
    return rc, name.value.decode(), list(words)


# (B, D, d_static, Fe, C) -> name, words[0] bits by hand (narrow iff D + Fe <= 192; emb_lds iff 0 < Fe ds <= 1024 and ds <= 64; focal
# is bit 3; three jobs with a static embedding, two without), touch site, k_head_wgrad tiles
FOCAL_ROUTES = [
    ((256, 152, 6, 34, 2), "k_head_rows<12,3,focal>", 1 | 4 | 8 | 3 << 8, "HEAD_P19_F", 159),
    ((5, 160, 3, 32, 2), "k_head_rows<12,3,focal>", 1 | 4 | 8 | 3 << 8, "HEAD_P19_F", 158),
    ((5, 160, 3, 33, 2), "k_head_rows<16,4,focal>", 4 | 8 | 3 << 8, "HEAD_F", 185),
    ((5, 256, 0, 0, 16), "k_head_rows<16,4,focal>", 8 | 2 << 8, "HEAD_F", 272),
    ((1025, 4, 0, 0, 3), "k_head_rows<12,3,focal>", 1 | 8 | 2 << 8, "HEAD_P19_F", 2),
]


@pytest.mark.parametrize("sizes,name,word0,site,ntiles", FOCAL_ROUTES)
def test_route_of_the_focal_form(lib, monkeypatch, sizes, name, word0, site, ntiles):
    for k in ("RD_HEAD_NARROW", "RD_CODE_TOUCH", "RD_HEAD_FUSED"):
        monkeypatch.delenv(k, raising=False)
    B, D, ds, Fe, C = sizes
    rc, got, w = _route(lib, 0, B, D, ds, Fe, C, 2)
    assert rc == 0 and got == name and w[0] == word0 and w[2] == B and w[3] == ntiles, (got, w)
    assert w[1] == build.read_touch_table()[site] > 0
    # values 0 and 1 answer as before: the same words without bit 3 (and with bit 1 for the criterion), their own names and touch sites
    for form, bit, suffix in ((0, 0, ""), (1, 2, ",crit")):
        rc, n2, w2 = _route(lib, 0, B, D, ds, Fe, C, form)
        assert rc == 0 and n2 == name.replace(",focal", suffix) and w2[0] == (word0 & ~8) | bit and w2[2:] == w[2:], (n2, w2)
        assert w2[1] == build.read_touch_table()[site[:-2] + ("_C" if form else "")]
    assert _route(lib, 1, B, D, ds, Fe, C, 2)[0] != 0 and _route(lib, 0, B, D, ds, Fe, C, 3)[0] != 0
    assert "focal" in _lib.HEAD_ROUTE_BITS and _lib.HEAD_ROUTE_BITS.index("focal") == 3


def test_focal_instantiations_use_no_scratch(lib):
    usage = build.resource_usage()
    focal = {k: v for k, v in usage.items() if re.search(r"k_head_rows_focalILi1ELi\d+ELi\dEE", k)}
    assert len(focal) == 2, sorted(focal)
    for name, u in list(focal.items()) + [(k, v) for k, v in usage.items() if "k_softmax_xent_focal" in k]:
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["vgprs"] <= 128, (name, u)
    assert any("k_softmax_xent_focal" in k for k in usage)
    # the plain and CRIT kernels are still listed, two each
    for flag in ("Lb0E", "Lb1E"):
        assert len([k for k in usage if re.search(r"k_head_rowsILi1ELi\d+ELi\dE" + flag, k)]) == 2
    sites = {s for s, _, _ in build.TOUCH_SITES}
    assert {"HEAD_P19", "HEAD", "HEAD_P19_C", "HEAD_C", "HEAD_P19_F", "HEAD_F"} <= sites
    build.check_code_touch()
