"""GPU: FlatAdam's parameter groups and decoupled weight decay (`optim.ParamGroups`, `FlatAdam(groups=, decoupled=)`; the eight
rd_adam_step[_clip][_ema]_grp[_dev] entry points) -- the raw optimizer on a hand-laid flat buffer against torch.optim.Adam / AdamW
with one torch param group per group, neutral groups bit-equal to the plain kernels, the non-finite guard over all groups, the
whole step as one hipGraph (TrainStep and BetaTrainStep) with a group held still between replays, and `fit`."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (size, offset, group): the smallest shapes at which the map can go wrong -- a one-element tensor, 63 / 64 / 65 elements around the
# chunk size, a tensor that crosses the workgroup boundary at 1024, and 70 elements that end in a two-element scalar tail.
# n = 1478: two workgroups, four group boundaries inside the first wave (elements 0..255).
TENSORS = [(1, 0, 1), (63, 64, 2), (64, 128, 0), (65, 192, 1), (1030, 320, 0), (70, 1408, 3)]
N = 1478
LR, WD = 2.5e-4, 0.01                                              # no effective rate exceeds 1e-3 (group 1: 4 x 2.5e-4)
SCALE = [1.0, 4.0, 0.1, 0.0]
DECAY = [None, 0.0, 0.05, None]                                    # None: follows the optimizer's 0.01
STEPS = 5
MAX_NORM = 60.0                                                    # the gradient norms are about 36 (0.1 + s): steps 2, 3, 4 are clipped, 0 and 1 are not
FORMS = [(c, e, d) for c in (False, True) for e in (False, True) for d in (False, True)]
FORM_IDS = ["rd_adam_step" + "_clip" * c + "_ema" * e + "_grp" + "_dev" * d for c, e, d in FORMS]


def _layout():
    import types
    return types.SimpleNamespace(names=["t%d" % (k + 1) for k in range(len(TENSORS))], slices=[(o, o + n) for n, o, _ in TENSORS])


def _rules(neutral=False):
    rules = []
    for r in (1, 2, 3):
        names = ["t%d" % (k + 1) for k, t in enumerate(TENSORS) if t[2] == r]
        rules.append(dict(match=names) if neutral else dict(match=names, lr_scale=SCALE[r], weight_decay=DECAY[r]))
    return rules


@functools.lru_cache(maxsize=None)
def _data():
    """(initial flat parameters, the five flat gradients): standard normal in the tensors, 0 in the padding behind them; gradient s
    scaled by 0.1 + s"""
    g_ = torch.Generator(device="cpu").manual_seed(11)
    live = torch.zeros(N, dtype=torch.bool)
    for n, o, _ in TENSORS:
        live[o:o + n] = True
    p0 = torch.randn(N, generator=g_) * live
    grads = [torch.randn(N, generator=g_) * live * (0.1 + s) for s in range(STEPS)]
    return p0, grads, live


@functools.lru_cache(maxsize=None)
def _torch_reference(clip, decoupled):
    """the flat parameters after each of the five steps: torch.optim.Adam (coupled) / AdamW (decoupled) on the CPU, one torch param
    group per group, clip_grad_norm_ over ALL tensors in front of the step"""
    p0, grads, _ = _data()
    params = [torch.nn.Parameter(p0[o:o + n].clone()) for n, o, _ in TENSORS]
    groups = [dict(params=[q for q, t in zip(params, TENSORS) if t[2] == r], lr=LR * SCALE[r], weight_decay=WD if DECAY[r] is None else DECAY[r])
              for r in range(4)]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(groups, lr=LR, betas=(0.9, 0.999), eps=1e-8)
    out, clipped = [], 0
    for s in range(STEPS):
        for q, (n, o, _) in zip(params, TENSORS):
            q.grad = grads[s][o:o + n].clone()
        if clip:
            clipped += float(torch.nn.utils.clip_grad_norm_(params, MAX_NORM)) > MAX_NORM
        opt.step()
        flat = torch.zeros(N)
        for q, (n, o, _) in zip(params, TENSORS):
            flat[o:o + n] = q.detach()
        out.append(flat)
    assert not clip or 0 < clipped < STEPS                          # the threshold clips some of the five steps, not all
    return out


def _opt(clip, ema, groups=None, **kw):
    from raindrop_amd.optim import FlatAdam
    p0, _, _ = _data()
    p = torch.nn.Parameter(p0.clone().to(DEV))
    p.grad = torch.zeros(N, device=DEV)
    if clip:
        kw.update(max_grad_norm=MAX_NORM)
    if ema:
        kw.update(ema_decay=0.9)
    return p, FlatAdam(p, lr=LR, weight_decay=WD, groups=groups, **kw)


def _one(p, opt, dev, g):
    p.grad.copy_(g)
    if dev:
        opt.step_captured(); opt.note_replay()
    else:
        opt.step()


def _bits(*ts):
    return [t.detach().clone().view(torch.int32) for t in ts]


def _state(opt):
    return _bits(opt.param, opt.exp_avg, opt.exp_avg_sq) + ([] if opt.ema is None else _bits(opt.ema))


# ---- 1. against torch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_groups_against_torch(form, decoupled):
    """max |p - torch| < 2e-6 after each of five steps: the bound tests/test_gpu_parity.py and tests/test_grad_clip_gpu.py hold
    rd_adam_step and the clipped update to at lr = 1e-3, the largest effective rate here.  Group 3 (lr_scale 0) keeps its
    parameters' bits while its moments move; the padding behind every tensor stays 0."""
    from raindrop_amd.optim import ParamGroups
    clip, ema, dev = form
    _, grads, live = _data()
    want = _torch_reference(clip, decoupled)
    p, opt = _opt(clip, ema, groups=ParamGroups(_layout(), _rules()), decoupled=decoupled)
    assert opt.hyper()[-1] == "grp"
    start = _bits(p)[0].cpu()
    worst = 0.0
    for s in range(STEPS):
        _one(p, opt, dev, grads[s].to(DEV))
        worst = max(worst, float((p.detach().cpu() - want[s]).abs().max()))
    print("%s %s: max |p - torch| over %d steps %.3e" % (FORM_IDS[FORMS.index(form)], "decoupled" if decoupled else "coupled", STEPS, worst))
    assert worst < 2e-6
    got, m, v = p.detach().cpu(), opt.exp_avg.cpu(), opt.exp_avg_sq.cpu()
    n3, o3, _ = TENSORS[5]
    assert torch.equal(got.view(torch.int32)[o3:o3 + n3], start[o3:o3 + n3])                   # held still ...
    assert bool((m[o3:o3 + n3] != 0).all()) and bool((v[o3:o3 + n3] > 0).all())                # ... while its moments go on
    assert not torch.equal(got.view(torch.int32)[:o3][live[:o3]], start[:o3][live[:o3]])
    assert bool((got[~live] == 0).all()) and bool((m[~live] == 0).all()) and bool((v[~live] == 0).all())
    if clip:
        st = opt.grad_stats()
        assert st["skipped"] == 0 and 0 < st["clipped"] < STEPS
    assert opt.t == STEPS and (not dev or opt.device_steps() == STEPS)


# ---- 2. neutral groups are the plain kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_neutral_groups_are_bit_equal_to_the_ungrouped_forms(form):
    """every row {1, wd, 0, 0}: p, m, v (and ema) after each of three steps have the bits of the optimizer without groups"""
    from raindrop_amd.optim import ParamGroups
    clip, ema, dev = form
    _, grads, _ = _data()
    p, opt = _opt(clip, ema, groups=ParamGroups(_layout(), _rules(neutral=True)))
    q, ref = _opt(clip, ema)
    assert opt.group_cell.tolist()[:4] == [[1.0, WD, 0.0, 0.0]] * 4 and ref.chunk_group is None
    for s in range(3):
        _one(p, opt, dev, grads[s + 1].to(DEV))                     # (steps 1..3: clipping on and off among them)
        _one(q, ref, dev, grads[s + 1].to(DEV))
        a, b = _state(opt), _state(ref)
        assert len(a) == len(b) == 3 + ema
        for name, x, y in zip(("p", "m", "v", "ema"), a, b):
            assert torch.equal(x, y), (s, name, int((x != y).sum()), (x != y).nonzero()[:4].flatten().tolist())


# ---- 3. the guard ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("ema", [False, True], ids=["", "ema"])
def test_non_finite_gradient_skips_every_group(ema, dev):
    from raindrop_amd.optim import ParamGroups
    _, grads, _ = _data()
    p, opt = _opt(True, ema, groups=ParamGroups(_layout(), _rules()), decoupled=True)
    _one(p, opt, dev, grads[1].to(DEV))                             # one real step first: moments and average are not trivial
    before = _state(opt)
    g = grads[2].clone()
    g[200] = float("inf")                                           # in group 1; groups 0, 2, 3 hold finite gradients only
    _one(p, opt, dev, g.to(DEV))
    assert all(torch.equal(x, y) for x, y in zip(_state(opt), before))
    st = opt.grad_stats()
    assert st["skipped"] == 1 and st["scale"] == 0.0 and opt.t == 2
    if ema:
        assert opt.ema_updates() == 1


# ---- 4. the whole step as one hipGraph ------------------------------------------------------------------------------------------------
def _whole_step(beta):
    """P19, B = 8, dropout 0, no_decay groups at weight decay 0.01 (tests/test_ema_gpu.py's tiny model)"""
    from raindrop_amd import dp, optim, synth
    from raindrop_amd.step import TrainStep
    from raindrop_amd.step_beta import BetaTrainStep
    from tests.helpers import build_ours
    cfg = synth.make_config("P19")
    m = build_ours(cfg, synth.make_structure(cfg, "sparse"), DEV, 21, **(dict(use_beta=True) if beta else {})).train()
    named = dict(m.named_parameters())
    names = synth.live_parameter_names_beta(cfg) if beta else synth.live_parameter_names(cfg)
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in names], n_buckets=2)
    groups = optim.ParamGroups(flat, [optim.no_decay(flat)])
    opt = optim.FlatAdam(flat.flatten_parameters(), lr=1e-3, weight_decay=0.01, groups=groups)
    buf = {k: (None if v is None else v.to(DEV).clone()) for k, v in synth.make_batch(cfg, 8, seed=33).items()}
    ts = (BetaTrainStep if beta else TrainStep)(m, flat, buf, p_drop=0.0, autotune=False, split=False)
    return flat, ts, opt


@pytest.mark.parametrize("beta", [False, True], ids=["default", "use_beta"])
def test_whole_step_graph_holds_a_group_still_without_a_new_capture(beta):
    """capture_full with no_decay groups: after set_group(1, lr_scale=0.0) between replays the SAME graph replays, the biases and
    LayerNorm parameters keep their bits and every other tensor moves"""
    flat, ts, opt = _whole_step(beta)
    try:
        graph = ts.capture_full(opt)
        assert ts.captures == 1 and opt.hyper()[-1] == "grp"
        info = opt.group_info()
        assert len(info) == 2 and info[0]["weight_decay"] == 0.01 and info[1]["weight_decay"] == 0.0
        held = set(info[1]["names"])
        assert held and all(p.dim() <= 1 for n, p in zip(flat.names, flat.params) if n in held) and len(held) < len(flat.names)
        start = _bits(opt.param)[0]
        for _ in range(2):
            ts.run_full()
        torch.cuda.synchronize()
        mid = _bits(opt.param)[0]
        assert all(not torch.equal(mid[lo:hi], start[lo:hi]) for lo, hi in flat.slices)        # with both groups live every tensor moves
        opt.set_group(1, lr_scale=0.0)
        for _ in range(2):
            loss = ts.run_full()
        torch.cuda.synchronize()
        assert ts.captures == 1 and ts.graph_full is graph and opt.device_steps() == opt.t == 4 and bool(torch.isfinite(loss))
        end = _bits(opt.param)[0]
        for name, (lo, hi) in zip(flat.names, flat.slices):
            same = torch.equal(end[lo:hi], mid[lo:hi])
            assert same == (name in held), (name, same)
    finally:
        ts.close()


# ---- 5. fit -----------------------------------------------------------------------------------------------------------------------------
def test_fit_with_a_neutral_rule_is_fit_without_the_keyword():
    """the settings of tests/test_epoch_feed_gpu.py::test_fit_runs_the_scripts_loop: two epochs, the same seed; a rule that changes
    nothing (lr_scale 1, the optimizer's decay) gives the history and the final parameters of fit without param_groups, bit for bit"""
    from raindrop_amd import feed, synth, trainer
    from tests.helpers import build_ours
    cfg = synth.make_config("P19")

    def part(n, seed, rseed):
        data = synth.make_batch(cfg, n, seed=seed)
        y = ((data["src"][:, :, 0].sum(0).numpy() + 0.5 * np.random.default_rng(rseed).standard_normal(n)) > 0).astype(np.int64)
        if y.mean() > 0.5:
            y = 1 - y
        return feed.DeviceDataset(data["src"], data["times"], data["static"], torch.from_numpy(y), device=DEV)
    ds, vds = part(640, 71, 5), part(96, 72, 6)
    runs = []
    for kw in ({}, dict(param_groups=[dict(match=r"bias$")])):
        np.random.seed(0)
        m = build_ours(cfg, synth.make_structure(cfg, "ones"), DEV, 3)
        m.dropout.p = 0.2
        r = trainer.fit(m.eval(), ds, vds, 2, batch_size=128, strategy=2, lr=1e-3, weight_decay=0.01, scheduler=False, autotune=False,
                        **kw)
        runs.append((r, [p.detach().clone().view(torch.int32) for p in m.parameters()]))
    (r0, p0), (r1, p1) = runs
    print("train_loss", r0["train_loss"], r1["train_loss"], "val_auroc", r0["val_auroc"], r1["val_auroc"])
    assert r0 == r1 and len(r0["train_loss"]) == 2
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))
