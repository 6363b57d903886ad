"""GPU: the exponential moving average of the weights inside FlatAdam's launches (`ema_decay`, `ema_warmup`; rd_adam_step_ema,
rd_adam_step_ema_dev, rd_adam_step_clip_ema, rd_adam_step_clip_ema_dev, rd_swap_f32): the operator against a float64 recurrence,
parameters and moments bit-equal to the plain twins, skipped steps, determinism, the in-place exchange, the whole step as one
hipGraph (TrainStep and BetaTrainStep) with a new decay between replays, and evaluation on the averaged weights."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_STEPS = 12
# form -> (FlatAdam method, keywords): together the four EMA entry points
FORMS = {"ema": ("step", {}), "ema_dev": ("step_captured", {}), "clip_ema": ("step", dict(max_grad_norm=1.0)),
         "clip_ema_dev": ("step_captured", dict(max_grad_norm=1.0))}
MODES = {"d0.9": dict(ema_decay=0.9), "d0.999_warmup": dict(ema_decay=0.999, ema_warmup=True)}


def _flat(n, seed=1, **kw):
    from raindrop_amd.optim import FlatAdam
    g_ = torch.Generator(device="cpu").manual_seed(seed)
    p = torch.nn.Parameter(torch.randn(n, generator=g_).to(DEV))
    p.grad = torch.zeros(n, device=DEV)
    return p, FlatAdam(p, lr=1e-2, **kw)


def _grads(n, steps=N_STEPS, seed=2):
    g_ = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn(n, generator=g_).to(DEV) for _ in range(steps)]


def _one(p, opt, method, g):
    p.grad.copy_(g)
    if method == "step":
        opt.step()
    else:
        opt.step_captured(); opt.note_replay()


def _bits(*ts):
    return [t.detach().clone().view(torch.int32) for t in ts]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _d_t(mode, k):
    d = mode["ema_decay"]
    return min(d, (1.0 + k) / (10.0 + k)) if mode.get("ema_warmup") else d


# ---- 1. the operator against float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", [1, 5, 1027, 70001])
def test_ema_against_float64(n, form, mode):
    """ema += (1 - d_t)(p_new - ema) in float64 on the host, driven by the fp32 parameters read back after each of 12 steps (random
    gradients): |ema - ref| <= 8 N 2^-24 M, M = max(|p|, |ema|) over the run -- per step at most three fp32 roundings on values of
    magnitude at most 2M plus the rounding of c_t, earlier errors contract by d_t.  With warm-up d_t starts 0.1, 0.18, ..."""
    method, kw = FORMS[form]
    p, opt = _flat(n, seed=n, **kw, **MODES[mode])
    if method == "step_captured":
        opt.sync_step_cell()
    ref = p.detach().cpu().double().numpy().copy()
    assert np.array_equal(opt.ema.cpu().numpy(), ref.astype(np.float32))
    M = float(np.abs(ref).max())
    if mode == "d0.999_warmup":
        assert [round(_d_t(MODES[mode], k), 12) for k in (0, 1)] == [0.1, round(2 / 11, 12)]
    for k, g in enumerate(_grads(n, seed=n + 1)):
        _one(p, opt, method, g)
        pn = p.detach().cpu().double().numpy()
        ref += (1.0 - _d_t(MODES[mode], k)) * (pn - ref)
        M = max(M, float(np.abs(pn).max()), float(opt.ema.abs().max()))
    err = float(np.abs(opt.ema.cpu().double().numpy() - ref).max())
    bound = 8 * N_STEPS * 2.0 ** -24 * M
    print("n %d %s %s: max |ema - float64| = %.3e, bound %.3e, ratio %.3f" % (n, form, mode, err, bound, err / bound))
    assert err <= bound
    assert opt.ema_updates() == N_STEPS and opt.t == N_STEPS
    assert float((opt.ema - p.detach()).abs().max()) > 0.0                      # an average, not a copy


# ---- 1b. all eight forms of the update against float64 ------------------------------------------------------------------------------
ALL_FORMS = {"plain": ("step", {}), "dev": ("step_captured", {}), "clip": ("step", dict(max_grad_norm=1.0)),
             "clip_dev": ("step_captured", dict(max_grad_norm=1.0)),
             **{k: (m, dict(kw, ema_decay=0.9)) for k, (m, kw) in FORMS.items()}}
U = 2.0 ** -24                                                                  # one fp32 rounding, relative


@pytest.mark.parametrize("form", list(ALL_FORMS))
@pytest.mark.parametrize("n", [1, 5, 1027, 70001])
def test_update_against_float64(n, form):
    """p, exp_avg, exp_avg_sq of every entry point -- rd_adam_step [_clip] [_ema] [_dev] -- at the sizes of test 1 (1 and 5: the
    scalar tail alone; 1027: float4 slots and a tail in the last workgroup; 70001: many workgroups), weight decay on, 12 steps.
    Each step is checked on its own, element by element, against the update formed in float64 from the fp32 state read back
    before it, so the bounds are those of ONE step's roundings (U = 2^-24 each, first order, 1% on top for the second):
      gr = g s + wd p: three roundings and, clipping, the float the scale is rounded to: |d gr| <= 4 U A, A = |g s| + |wd p|
      m' = b1 m + (1 - b1) gr: two products, one sum: |d m'| <= U (2 b1 |m| + 6 (1 - b1) A)     (1 - b1, 1 - b2 are exact in fp32)
      v' = b2 v + (1 - b2) gr gr: three products, one sum, gr twice: |d v'| <= U (2 b2 v + 3 (1 - b2) gr^2 + 8 (1 - b2) |gr| A)
      p' = p - u, u = (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps) formed from the fp32 m', v' the launch stored: lr, bc1 and
      sqrt(bc2) rounded to float, one product, one sum, and three divisions and a square root counted at one ulp (2 U) each: 13 U |u|;
      the final difference one more: |d p'| <= U (13 |u| + |p'|).
    The clip forms: s = min(1, 1 / (norm + 1e-6)) from numpy's float64 norm of the same gradient (max_grad_norm = 1: all but the
    smallest gradients are clipped), and the device's own scale must agree with it to (n + 4) 2^-52 relative: n 2^-52 for the norm,
    the bound of test_norm_against_float64, and the sum and the quotient behind it, 2^-53 each on either side."""
    method, kw = ALL_FORMS[form]
    lr, wd, eps = 1e-2, 0.01, 1e-8
    p, opt = _flat(n, seed=n, weight_decay=wd, **kw)
    if method == "step_captured":
        opt.sync_step_cell()
    b1, b2 = (float(np.float32(b)) for b in opt.betas)                          # the betas as the launches see them
    worst = dict(m=0.0, v=0.0, p=0.0)
    for t, g in enumerate(_grads(n, seed=n + 1), start=1):
        p0, m0, v0 = (x.detach().cpu().double().numpy() for x in (p, opt.exp_avg, opt.exp_avg_sq))
        g64 = g.cpu().double().numpy()
        _one(p, opt, method, g)
        p1, m1, v1 = (x.detach().cpu().double().numpy() for x in (p, opt.exp_avg, opt.exp_avg_sq))
        s = 1.0
        if "max_grad_norm" in kw:
            norm = float(np.sqrt(np.sum(g64 ** 2)))
            s = min(1.0, 1.0 / (norm + 1e-6))
            assert abs(opt.grad_stats()["scale"] - s) <= (n + 4) * 2.0 ** -52 * s
        gs, wp = g64 * s, float(np.float32(wd)) * p0
        gr, A = gs + wp, np.abs(gs) + np.abs(wp)
        m_ref = b1 * m0 + (1 - b1) * gr
        v_ref = b2 * v0 + (1 - b2) * gr * gr
        u = (lr / (1 - b1 ** t)) * m1 / (np.sqrt(v1) / math.sqrt(1 - b2 ** t) + float(np.float32(eps)))
        p_ref = p0 - u
        tol = dict(m=U * (2 * b1 * np.abs(m0) + 6 * (1 - b1) * A),
                   v=U * (2 * b2 * v0 + 3 * (1 - b2) * gr * gr + 8 * (1 - b2) * np.abs(gr) * A),
                   p=U * (13 * np.abs(u) + np.abs(p_ref)))
        for key, got, ref in (("m", m1, m_ref), ("v", v1, v_ref), ("p", p1, p_ref)):
            ratio = float((np.abs(got - ref) / (1.01 * tol[key])).max())
            worst[key] = max(worst[key], ratio)
    print("n %d %s: worst error / bound over %d steps: exp_avg %.3f, exp_avg_sq %.3f, p %.3f" % (n, form, N_STEPS, worst["m"], worst["v"], worst["p"]))
    assert worst["m"] <= 1.0 and worst["v"] <= 1.0 and worst["p"] <= 1.0
    assert opt.t == N_STEPS and float(opt.exp_avg.abs().min()) > 0.0            # every element was updated


# ---- 2. parameters and moments are the plain twin's ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_parameters_and_moments_are_bit_equal_to_the_plain_twin(form):
    method, kw = FORMS[form]
    for n in (5, 70001):
        pa, a = _flat(n, seed=3, weight_decay=0.01, **kw)
        pb, b = _flat(n, seed=3, weight_decay=0.01, ema_decay=0.9, ema_warmup=True, **kw)
        a.sync_step_cell(); b.sync_step_cell()
        for s, g in enumerate(_grads(n, seed=4)):
            _one(pa, a, method, g); _one(pb, b, method, g)
            torch.cuda.synchronize()
            assert _same(_bits(pa, a.exp_avg, a.exp_avg_sq), _bits(pb, b.exp_avg, b.exp_avg_sq)), (form, n, s)
        if kw:
            assert a.grad_stats() == b.grad_stats() and (n < 70001 or a.grad_stats()["clipped"] == N_STEPS)


# ---- 3. skipped steps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["clip_ema", "clip_ema_dev"])
def test_skipped_step_is_no_update_of_the_average(form):
    """an inf gradient at step 5: `ema` keeps its bits (and so do p, m, v), the update count stays, and with warm-up the steps that
    follow use the d_t of the lower count (the float64 recurrence with k = count, inside test 1's bound)"""
    method, kw = FORMS[form]
    n, mode = 70001, MODES["d0.999_warmup"]
    p, opt = _flat(n, seed=5, **kw, **mode)
    opt.sync_step_cell()
    ref = p.detach().cpu().double().numpy().copy()
    M, k = float(np.abs(ref).max()), 0
    for s, g in enumerate(_grads(n, seed=6)):
        if s == 5:
            g = g.clone(); g[n // 2] = math.inf
            before = _bits(p, opt.exp_avg, opt.exp_avg_sq, opt.ema)
        _one(p, opt, method, g)
        if s == 5:
            torch.cuda.synchronize()
            assert _same(before, _bits(p, opt.exp_avg, opt.exp_avg_sq, opt.ema))
            assert opt.ema_updates() == 5 and opt.grad_stats()["skipped"] == 1 and opt.t == 6
            continue
        pn = p.detach().cpu().double().numpy()
        ref += (1.0 - _d_t(mode, k)) * (pn - ref)
        k += 1
        M = max(M, float(np.abs(pn).max()), float(opt.ema.abs().max()))
        assert opt.ema_updates() == k
    err, bound = float(np.abs(opt.ema.cpu().double().numpy() - ref).max()), 8 * N_STEPS * 2.0 ** -24 * M
    print("%s: after a skipped step max |ema - float64| = %.3e, bound %.3e, ratio %.3f" % (form, err, bound, err / bound))
    assert err <= bound and opt.grad_stats()["skipped"] == 1 and opt.ema_updates() == N_STEPS - 1
    # (a recurrence that had counted the skipped step would use d_t(6) = 7/16 instead of d_t(5) = 0.4 next: 0.04 |p - ema|, far outside)


# ---- 4. determinism -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_two_runs_from_the_same_state_give_the_same_bits(form):
    method, kw = FORMS[form]
    n, runs = 70001, []
    for _ in range(2):
        p, opt = _flat(n, seed=7, ema_decay=0.999, ema_warmup=True, **kw)
        opt.sync_step_cell()
        for g in _grads(n, steps=6, seed=8):
            _one(p, opt, method, g)
        torch.cuda.synchronize()
        runs.append(_bits(opt.ema, p) + [opt.ema_cell.clone().view(torch.int64)])
    assert _same(runs[0], runs[1])


# ---- 5. the exchange ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 70001])
def test_swap_exchanges_in_place_and_two_swaps_restore(n):
    from raindrop_amd import _lib, ops
    g_ = torch.Generator(device="cpu").manual_seed(n)
    pad = 4                                                                    # words behind the end must stay untouched
    a, b = (torch.randn(n + pad, generator=g_).to(DEV) for _ in range(2))
    a0, b0 = a.clone(), b.clone()
    _lib.call("rd_swap_f32", n, ops._ptr(a), ops._ptr(b), ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(a[:n].view(torch.int32), b0[:n].view(torch.int32)) and torch.equal(b[:n].view(torch.int32), a0[:n].view(torch.int32))
    assert torch.equal(a[n:], a0[n:]) and torch.equal(b[n:], b0[n:])
    _lib.call("rd_swap_f32", n, ops._ptr(a), ops._ptr(b), ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), a0.view(torch.int32)) and torch.equal(b.view(torch.int32), b0.view(torch.int32))


# ---- 6. / 7. the whole step as one hipGraph, and evaluation on the average ---------------------------------------------------------
OPT_KW = dict(ema_decay=0.99, max_grad_norm=1.0)


def _whole_step(beta=False, opt_kw=OPT_KW):
    """P19, B = 8, dropout 0: (model, flat, TrainStep or BetaTrainStep, FlatAdam, batch buffers)"""
    from raindrop_amd import dp, synth
    from raindrop_amd.optim import FlatAdam
    from raindrop_amd.step import TrainStep
    from raindrop_amd.step_beta import BetaTrainStep
    from tests.helpers import build_ours
    cfg = synth.make_config("P19")
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 21, **(dict(use_beta=True) if beta else {})).train()
    named = dict(m.named_parameters())
    names = synth.live_parameter_names_beta(cfg) if beta else synth.live_parameter_names(cfg)
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in names], n_buckets=2)
    opt = FlatAdam(flat.flatten_parameters(), lr=1e-3, **opt_kw)
    buf = {k: (None if v is None else v.to(DEV).clone()) for k, v in synth.make_batch(cfg, 8, seed=33).items()}
    ts = (BetaTrainStep if beta else TrainStep)(m, flat, buf, p_drop=0.0, autotune=False, split=False)
    return cfg, m, flat, ts, opt, buf


@pytest.mark.parametrize("beta", [False, True], ids=["default", "use_beta"])
def test_whole_step_graph_carries_the_average(beta):
    """capture_full with FlatAdam(ema_decay=0.99, max_grad_norm=1.0): six replays against six eager run() + step() from the same
    start, parameters and `ema` bit-equal after every step; set_ema_decay(0.5) after the third takes effect in the fourth without
    a new capture"""
    _, _, _, ts_r, opt_r, _ = _whole_step(beta)
    want = []
    try:
        for s in range(6):
            if s == 3:
                opt_r.set_ema_decay(0.5)
            ts_r.run()
            opt_r.step()
            torch.cuda.synchronize()
            want.append(_bits(opt_r.param, opt_r.ema))
    finally:
        ts_r.close()
    _, _, _, ts, opt, _ = _whole_step(beta)
    try:
        ts.capture_full(opt)
        assert ts.captures == 1
        for s in range(6):
            if s == 3:
                opt.set_ema_decay(0.5)
            ts.run_full()
            torch.cuda.synchronize()
            got = _bits(opt.param, opt.ema)
            print("step %d: max |p - eager| %.3e, max |ema - eager| %.3e" % tuple(
                [s] + [float((x.view(torch.float32) - y.view(torch.float32)).abs().max()) for x, y in zip(got, want[s])]))
            assert _same(got, want[s]), s
        assert ts.captures == 1 and opt.ema_updates() == 6 and opt.device_steps() == opt.t == 6
        assert math.isfinite(opt.grad_stats()["norm"]) and opt.grad_stats()["skipped"] == 0
        # the decay did change the fourth update: 0.5 of the way to p, not 0.01
        assert not torch.equal(want[3][1], want[2][1])
        with opt.ema_weights():
            with pytest.raises(Exception, match="average"):
                ts.run_full()
        assert opt.t == 6 and _same(_bits(opt.param, opt.ema), want[5])
    finally:
        ts.close()


@pytest.fixture(params=["bf16x3", "fp32"])
def precision_mode(request):
    from raindrop_amd import _lib
    _lib.call("rd_set_precision", 1 if request.param == "bf16x3" else 0)
    yield request.param
    _lib.call("rd_set_precision", 1)


def test_evaluation_reads_the_average_through_the_same_captured_step(precision_mode):
    """after six steps: the SAME captured EvalStep inside ema_weights() gives the logits of a second model whose parameters were
    set from opt.ema -- bit-equal on the padded layout, within the token plan's 2e-6 (tests/test_eval_step_gpu.py) on the plan --
    and the pre-swap logits, bit for bit, after the block; so does the eager model.eval() forward; step() inside the block raises;
    a state_dict() round trip into a fresh FlatAdam continues the run bit-equal"""
    from raindrop_amd import _lib, dp, synth
    from raindrop_amd.evalstep import EvalStep
    from raindrop_amd.optim import FlatAdam
    from tests.helpers import build_ours
    cfg, m, flat, ts, opt, buf = _whole_step()
    try:
        for _ in range(6):
            ts.run()
            opt.step()
        eb = {k: buf[k] for k in ("src", "times", "lengths", "static")}
        steps = {"padded": EvalStep(m, eb, token_plan=False, save_free=True), "auto": EvalStep(m, eb, save_free=True)}
        live = {k: s.run().clone() for k, s in steps.items()}
        m2 = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 21).eval()
        named2 = dict(m2.named_parameters())
        for name, (lo, hi) in zip(flat.names, flat.slices):
            named2[name].data.copy_(opt.ema[lo:hi].view_as(named2[name]))
        with torch.no_grad():
            ref = m2(eb["src"], eb["static"], eb["times"], eb["lengths"])[0].clone()
        assert float((ref - live["padded"]).abs().max()) > 0.0                   # the average differs from the training weights
        before = _bits(opt.param, opt.ema)
        with opt.ema_weights():
            for k, s in steps.items():
                got = s.run()
                diff = float((got - ref).abs().max())
                print(precision_mode, k, "plan" if s.plan is not None else "padded", "max |logits(ema) - second model| = %.3e" % diff)
                if s.plan is None:
                    assert torch.equal(got, ref)
                else:
                    assert diff < 2e-6
                assert s.captures == 1
            m.eval()
            with torch.no_grad():
                assert torch.equal(m(eb["src"], eb["static"], eb["times"], eb["lengths"])[0], ref)
            m.train()
            with pytest.raises(_lib.RaindropHipError):
                opt.step()
            with pytest.raises(_lib.RaindropHipError):
                opt.step_captured()
        assert _same(before, _bits(opt.param, opt.ema)) and opt.t == 6
        for k, s in steps.items():
            assert torch.equal(s.run(), live[k]) and s.captures == 1
        # state_dict round trip: a fresh model + FlatAdam loaded from the dictionaries continues like the original
        _, m3, flat3, ts3, opt3, _ = _whole_step(opt_kw=dict(ema_decay=0.5, max_grad_norm=3.0))
        try:
            opt3.param.data.copy_(opt.param.data)
            opt3.load_state_dict(opt.state_dict())
            assert opt3.ema_updates() == 6 and opt3.ema_decay == 0.99 and _same(_bits(opt3.ema), _bits(opt.ema))
            for _ in range(2):
                for t_, o_ in ((ts, opt), (ts3, opt3)):
                    t_.run()
                    o_.step()
            torch.cuda.synchronize()
            assert _same(_bits(opt.param, opt.ema, opt.exp_avg), _bits(opt3.param, opt3.ema, opt3.exp_avg))
            assert opt.ema_updates() == opt3.ema_updates() == 8
        finally:
            ts3.close()
        for s in steps.values():
            s.close()
    finally:
        ts.close()
