"""GPU: every dropout site of the training path against float64 torch with HOST-generated masks.

The masks are pure functions of (seed + seed cell, site, element); tests/rng_ref.py restates the generator and each site's element
numbering in numpy, tests/dropout_ref.py multiplies the keep-scales in where torch's nn.Dropout sits.  First the device generator is
tied to the host one bit for bit (rd_scale_dropout), then each site family is compared with p_drop = 0.2 in both precision modes
under the bounds of the same comparisons without dropout (tests/dropout_ref.py `*_bound`; no element is excluded anywhere).  Before
a family is compared, four WRONG masks (shifted by one element, 1/(1-p) left out, sample 0's mask for every sample, the other
layer's site) must move its reference by at least 20 x those bounds.

Measured maximum errors per case and mode: profiles/dropout_reference_errors.json (written when RD_DROPOUT_ERRORS_OUT names a file)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import dropout_ref as DR
from tests import rng_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
P, SEED = DR.P_DROP, DR.SEED
ERRORS = {}


@pytest.fixture(autouse=True, params=list(DR.MODES))
def precision_mode(request):
    """Both arithmetic modes of the dense contractions (tests/test_gpu_parity.py): split-bf16 MFMA and exact fp32 MFMA."""
    from raindrop_amd import _lib
    _lib.call("rd_set_precision", 1 if request.param == "bf16x3" else 0)
    yield request.param
    _lib.call("rd_set_precision", 1)


@pytest.fixture(autouse=True, scope="module")
def _dump_errors():
    yield
    path = os.environ.get("RD_DROPOUT_ERRORS_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(ERRORS, f, indent=1, sort_keys=True)


def _err(metric, a, r):
    return DR.rel(a, r) if metric == "rel" else DR.rel2(a, r) if metric == "rel2" else float(np.abs(a - r).max())


def _compare(case, mode, ref, got, bound_of):
    """Record every tensor's error (ERRORS[case][mode][tensor] = [metric, error, bound]) and then hold each to its bound.  A
    relative-L2 bound (the split-bf16 gradient bound of _grad_close) comes with that function's max-norm bound of 0.25."""
    rec = ERRORS.setdefault(case, {}).setdefault(mode, {})
    bad = []
    for name, r in ref.items():
        a = got[name].astype(np.float64)
        assert a.shape == r.shape, (case, name, a.shape, r.shape)
        metric, bound = bound_of(name)
        e = _err(metric, a, r)
        rec[name] = [metric, e, bound]
        ok = np.isfinite(a).all() and e < bound and (metric != "rel2" or DR.rel(a, r) < 0.25)
        if not ok:
            bad.append((name, metric, e, bound))
    print("%s %s: %s" % (case, mode, " ".join("%s=%.2e" % (n, v[1]) for n, v in rec.items())))
    assert not bad, (case, mode, bad)


def _must_bite(ref_fn, bound_of):
    """Section 4: each wrong variant moves the compared outputs by at least 20 x the bound used for the kernel."""
    ref = ref_fn(None)
    for v in DR.VARIANTS:
        m = DR.variant_margin(ref, ref_fn(v), bound_of)
        assert m >= 20.0, (v, m)


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the device generator equals the host one
# ---------------------------------------------------------------------------------------------------------------------------------
SITES = (1, 2, 16, 17, 32, 33, 48, 49, 64, 65)
SEEDS = (0, 77, 2 ** 32 + 5, 2 ** 63 - 1)
N_GEN = 4099                                  # no multiple of 4, more than one pass of a 256-thread block


def _device_decisions(n, p, seed, site):
    from raindrop_amd import _lib
    x = torch.ones(n, device=DEV)
    out = torch.full((n,), -1.0, device=DEV)
    _lib.call("rd_scale_dropout", n, _P(x), 1.0, float(p), int(seed), int(site), _P(out), None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_device_generator_equals_host_restatement(p, precision_mode):
    """rd_scale_dropout on ones: out = keep / (1 - p) of tests/rng_ref.py bit for bit, for every site number in use, seeds whose
    high word is non-zero, and a length that ends inside a quad."""
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    for site in SITES:
        for seed in SEEDS:
            want = np.where(R.keep(seed, site, np.arange(N_GEN), p), inv, np.float32(0.0)).astype(np.float32)
            got = _device_decisions(N_GEN, p, seed, site)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (site, seed, int((got != want).sum()))


def test_seed_cell_adds_to_the_seed(precision_mode):
    """With a registered seed cell holding 3, seed s gives the bits of seed s + 3 without a cell."""
    from raindrop_amd import _lib
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(P))
    cell = torch.tensor([3], dtype=torch.int64, device=DEV)
    for seed in SEEDS[:3] + (2 ** 32 - 2,):                         # the last: the carry into the key's high word
        plain = _device_decisions(N_GEN, P, seed + 3, 33)
        _lib.call("rd_set_seed_cell", _P(cell))
        try:
            with_cell = _device_decisions(N_GEN, P, seed, 33)
        finally:
            _lib.call("rd_set_seed_cell", None)
        want = np.where(R.keep(seed + 3, 33, np.arange(N_GEN), P), inv, np.float32(0.0)).astype(np.float32)
        assert np.array_equal(with_cell, plain) and np.array_equal(plain, want), seed


# ---------------------------------------------------------------------------------------------------------------------------------
# 3a. observation embedding, alone and through the sensor stage
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,F", [(7, 3, 5), (60, 5, 34)])
def test_obs_embed_vs_float64(T, B, F, precision_mode):
    from raindrop_amd import _lib, ops
    bound = DR.obs_bound(precision_mode)
    if (T, B, F) == (7, 3, 5):
        _must_bite(lambda v: DR.obs_reference(T, B, F, v), bound)
    c = DR.obs_case(T, B, F)
    ru = c["R_u"].to(DEV).requires_grad_(True)
    X = ops.obs_embed(c["src"].to(DEV), ru, _lib.shape(B, T, F, c["d"]), P, SEED)
    (g,) = torch.autograd.grad(X, ru, c["dX"].to(DEV))
    got = dict(X=X.detach().cpu().numpy(), dR_u=g.cpu().numpy())
    _compare("obs_embed T%d B%d F%d" % (T, B, F), precision_mode, DR.obs_reference(T, B, F), got, bound)


@pytest.mark.parametrize("F,T,B", [(34, 60, 5), (16, 60, 3)])
def test_sensor_stage_vs_float64(F, T, B, precision_mode):
    """(34, 60, 5): the fused K1 in split-bf16 mode, whose backward reads the forward's mask back as gate bits; (16, 60, 3): the
    generic path.  z's message-passing columns and the five gradients."""
    from raindrop_amd import _lib, ops
    bound = DR.sensor_bound(precision_mode)
    if F == 16:
        _must_bite(lambda v: DR.sensor_reference(F, T, B, v), bound)
    c = DR.sensor_case(F, T, B)
    b, d = c["batch"], c["d"]
    pd = {n: t.to(DEV).requires_grad_(True) for n, t in c["p"].items()}
    adj, _, _ = ops.graph_build(c["gs"].to(DEV))
    _, ssum = ops.edge_softmax_dense(adj)
    z, _ = ops.sensor_stage(b["src"].to(DEV), b["times"].to(DEV), b["lengths"].to(DEV), ops.timescales(T).to(DEV), ssum,
                            pd["R_u"], pd["W1"], pd["b1"], pd["W2"], pd["b2"], _lib.shape(B, T, F, d), P, SEED)
    g = torch.autograd.grad(z, [pd[n] for n in DR.SENSOR_NAMES], c["dz"].to(DEV))
    got = dict(z=z[:, :, : F * d].detach().cpu().numpy())
    got.update((n, t.cpu().numpy()) for n, t in zip(DR.SENSOR_NAMES, g))
    _compare("sensor_stage F%d T%d B%d" % (F, T, B), precision_mode, DR.sensor_reference(F, T, B), got, bound)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3b. attention core
# ---------------------------------------------------------------------------------------------------------------------------------
ATTN_CASES = [(60, 9, 34, 2, 0), (33, 4, 34, 2, 1), (64, 3, 12, 4, 0), (65, 3, 17, 2, 1), (130, 4, 12, 4, 0)]


@pytest.mark.parametrize("T,B,F,nhead,layer", ATTN_CASES)
def test_attention_core_dropout_vs_float64(T, B, F, nhead, layer, precision_mode):
    """rd_attention_fwd / rd_attention_bwd with p_drop = 0.2, seed 77: out, lse (of the UNDROPPED scores) and dqkv.  Single tile,
    T no multiple of 4, one key past a tile, multi tile; one sample of full length, one of length <= 20, one with a non-prefix
    key mask.  The materialised-score attention (RD_ATTN_BIG=1 at (12, 3, 3, 2); the wide heads of (40, 3, 60, 2)) cannot be
    entered here -- rd_attention_fwd refuses it with RD_EINVAL, "runs as materialised products inside the layer only" -- so these
    two shapes are compared through the layer, in test_encoder_layer_dropout_vs_float64."""
    from raindrop_amd import _lib
    bound = DR.attn_bound(precision_mode)
    if (T, B) == (33, 4):
        _must_bite(lambda v: DR.attn_reference(T, B, F, nhead, layer, v), bound)
    c = DR.attn_case(T, B, F, nhead)
    D = c["D"]
    qd, md, dd = c["qkv"].to(DEV), c["mask"].to(DEV), c["dout"].to(DEV)
    out = torch.zeros(T, B, D, device=DEV); lse = torch.zeros(B, nhead, T, device=DEV)
    dqkv = torch.zeros(T, B, 3 * D, device=DEV); ws = torch.zeros(B, nhead, T, device=DEV)
    shp = _lib.shape(B, T, F, 4, nhead=nhead, nhid=2 * F * 4)
    _lib.call("rd_attention_fwd", ctypes.byref(shp), layer, _P(qd), _P(md), P, SEED, _P(out), _P(lse), None)
    _lib.call("rd_attention_bwd", ctypes.byref(shp), layer, _P(qd), _P(md), P, SEED, _P(out), _P(lse), _P(dd), _P(dqkv), _P(ws), None)
    torch.cuda.synchronize()
    got = dict(out=out.cpu().numpy(), lse=lse.cpu().numpy(), dqkv=dqkv.cpu().numpy())
    _compare("attention T%d B%d F%d H%d" % (T, B, F, nhead), precision_mode,
             DR.attn_reference(T, B, F, nhead, layer), got, bound)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3c. encoder layer, padded layout
# ---------------------------------------------------------------------------------------------------------------------------------
ENC_CASES = [(7, 3, 5, 2, 1, None), (60, 6, 34, 2, 0, None), (60, 6, 34, 2, 1, "RD_ENC_FUSE=0"), (215, 2, 36, 2, 1, None),
             (16, 2, 256, 2, 0, None), (12, 3, 3, 2, 1, "RD_ATTN_BIG=1"), (40, 3, 60, 2, 0, None)]


@pytest.mark.parametrize("T,B,F,nhead,layer,env", ENC_CASES)
def test_encoder_layer_dropout_vs_float64(T, B, F, nhead, layer, env, precision_mode, monkeypatch):
    """ops.encoder_layer with p_drop = 0.2 against oracle/restatement.py encoder_layer in float64 with the four host masks: the
    output and all 13 gradients.  (60, 6, 34, 2) also under RD_ENC_FUSE=0 (the three row-block launches), (215, ..) the multi-tile
    attention, (16, 2, 256, 2) the tiled GEMM's dropout epilogue with the add + LN kernels (D = 1040); (12, 3, 3, 2) under
    RD_ATTN_BIG=1 and (40, 3, 60, 2) (head_dim 128) the materialised-score attention, which exists inside the layer only."""
    from raindrop_amd import _lib, ops
    bound = DR.enc_bound(precision_mode)
    if T == 7:
        _must_bite(lambda v: DR.enc_reference(T, B, F, nhead, layer, v), bound)
    if env is not None:
        monkeypatch.setenv(*env.split("="))
    c = DR.enc_case(T, B, F, nhead)
    xd = c["x"].to(DEV).requires_grad_(True)
    pd = [c["p"][n].to(DEV).requires_grad_(True) for n in ops.ENC_PARAM_NAMES]
    shp = _lib.shape(B, T, F, 4, nhead=nhead, nhid=c["nhid"])
    y = ops.encoder_layer(xd, c["mask"].to(DEV), shp, layer, P, SEED, pd)
    g = torch.autograd.grad(y, [xd] + pd, c["dy"].to(DEV))
    torch.cuda.synchronize()
    got = dict(y=y.detach().cpu().numpy())
    got.update((n, t.cpu().numpy()) for n, t in zip(["x"] + list(ops.ENC_PARAM_NAMES), g))
    assert set(got) == set(("y", "x") + DR.ENC_NAMES)
    _compare("encoder_layer T%d B%d F%d H%d%s" % (T, B, F, nhead, " " + env if env else ""), precision_mode,
             DR.enc_reference(T, B, F, nhead, layer), got, bound)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3d. the whole step on the token plan: the path the benchmark runs
# ---------------------------------------------------------------------------------------------------------------------------------
def step_bound(mode):
    """test_static_train_step_matches_autograd with the fused head: every gradient within 5e-5 of its max-norm (1e-5 in fp32 mode),
    the loss within 5e-6 (1e-6); the logits, which that test does not compare, are held to the gradients' bound.  That test
    excludes no ReLU-fence element, and neither does this one."""
    tol = 5e-5 if mode == "bf16x3" else 1e-5
    return lambda name: ("abs", 5e-6 if mode == "bf16x3" else 1e-6) if name == "loss" else ("rel", tol)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "captured"])
def test_token_plan_step_dropout_vs_float64(use_graph, precision_mode):
    """TrainStep(token_plan=True, p_drop=0.2) on P19, B = 9, lengths with 1, T and ties, run once -- eagerly, and as one captured
    replay -- against oracle/restatement.py raindrop_v2_forward + cross entropy in float64 with the masks numbered by the plan's
    rows and ranks (exact-fp32 mode: the padded layout's rows and sample indices) under the effective seed step.seed +
    step.seed_cell read back after the run."""
    from raindrop_amd import dp, synth
    from raindrop_amd.step import TrainStep
    from tests.helpers import build_ours
    c = DR.step_case()
    cfg = c["cfg"]
    dv = {k: (None if v is None else v.to(DEV)) for k, v in c["batch"].items()}
    m = build_ours(cfg, c["gs"], DEV, DR.STEP_PARAM_SEED).train()
    live = synth.live_parameter_names(cfg)
    named = dict(m.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in live])
    step = TrainStep(m, flat, dv, use_graph=use_graph, token_plan=True, p_drop=P, autotune=False)
    try:
        # the token plan exists in the split-bf16 modes; the exact-fp32 mode runs the same step on the padded layout
        assert (step.plan is not None) == (precision_mode == "bf16x3") and (step.graph is not None) == use_graph and step.p_drop == P
        on_plan = step.plan is not None
        loss = float(step.run())
        torch.cuda.synchronize()
        seed_eff = int(step.seed) + int(step.seed_cell.item())
        got = dict(loss=np.array([loss]), logits=step.logits.cpu().numpy())
        got.update((n, named[n].grad.detach().cpu().numpy()) for n in live)
    finally:
        step.close()
    bound = step_bound(precision_mode)
    _must_bite(lambda v: DR.step_reference(seed_eff, on_plan, v), bound)
    ref = DR.step_reference(seed_eff, on_plan)
    assert set(ref) == set(got)
    _compare("token_plan_step %s" % ("captured" if use_graph else "eager"), precision_mode, ref, got, bound)
