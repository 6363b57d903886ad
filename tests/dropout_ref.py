"""TEST INFRASTRUCTURE ONLY -- float64 references of the train-mode (dropout on) arithmetic, with the masks of tests/rng_ref.py
multiplied in where torch's nn.Dropout sits, and the deliberately WRONG variants of those masks that show the comparisons bite.

Used by tests/test_dropout_reference_gpu.py (device against these references) and tests/test_rng_ref_host.py (the wrong variants
must move the references by at least 20 x the bounds, checked on the CPU).  Inputs and references are built once per case and
shared between the precision modes (functools.lru_cache); nothing mutates them."""
import functools
import math

import numpy as np
import torch

from oracle import restatement as O2
from raindrop_amd import synth
from tests import rng_ref as R
from tests.helpers import plan_ref

P_DROP = 0.2
SEED = 77
# the wrong variants of section "the tests must be able to fail": the mask shifted by one element, 1/(1-p) left out, sample 0's
# mask reused for every sample, the other layer's site (observation embedding, which has no layer: the next site number)
VARIANTS = ("shift", "noscale", "sample0", "layer")
ENC_NAMES = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
             "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
             "norm2.bias")


class Masks:
    """Keep-scales (float64 torch: 0 or 1/(1-p)) of every site for one launch geometry.
    rows [T, B]: the row of (step, sample) -- rng_ref.padded_rows or rng_ref.plan_rows; bh_rank: None on the padded layout, the
    plan's rank[b] on a token plan; live bool [T, B] or None: steps that exist (a token plan has no rows for t >= len; the
    reference's values there feed nothing, their scale is 1)."""

    def __init__(self, seed, p, T, B, rows=None, bh_rank=None, live=None, variant=None):
        assert variant is None or variant in VARIANTS
        self.seed, self.p, self.T, self.B, self.variant = int(seed), float(p), T, B, variant
        self.rows = R.padded_rows(T, B) if rows is None else rows
        self.bh_rank, self.live = bh_rank, live

    def _site(self, family, layer):
        if self.variant == "layer":
            return family + 1 if family == R.SITE_OBS_EMBED else R.site_of(family, layer ^ 1)
        return R.site_of(family, layer)

    def _finish(self, keep, batch_axis, live=None):
        if self.variant == "shift":
            keep = np.roll(keep.reshape(-1), 1).reshape(keep.shape)
        if self.variant == "sample0":
            keep = np.broadcast_to(np.take(keep, [0], axis=batch_axis), keep.shape)
        scale = keep.astype(np.float64) * (1.0 if self.variant == "noscale" else 1.0 / (1.0 - self.p))
        if live is not None:
            scale = np.where(live, scale, 1.0)
        return torch.from_numpy(np.ascontiguousarray(scale))

    def obs(self, F, d):
        """[T, B, F*d]: observation embedding (indexed by the caller's sample on either layout)."""
        return self._finish(R.keep(self.seed, self._site(R.SITE_OBS_EMBED, 0), R.obs_embed_index(self.T, self.B, F, d), self.p), 1)

    def prob(self, layer, H):
        """[B, H, T, T]: attention probabilities."""
        return self._finish(R.attn_keep(self.seed, self._site(R.SITE_ATTN_PROB, layer), R.attn_bh(self.B, H, self.bh_rank), self.T,
                                        self.p), 0)

    def rowlocal(self, family, layer, N):
        """[T, B, N]: attention output / FFN hidden / FFN output."""
        live = None if self.live is None else self.live[:, :, None]
        idx = R.row_local_index(np.where(self.live, self.rows, 0) if self.live is not None else self.rows, N)
        return self._finish(R.keep(self.seed, self._site(family, layer), idx, self.p), 1, live)

    def encoder(self, layer, H, D, nhid):
        """the four masks of one encoder layer in the order oracle/restatement.py encoder_layer calls `drop`"""
        return [self.prob(layer, H), self.rowlocal(R.SITE_ATTN_OUT, layer, D), self.rowlocal(R.SITE_FFN_HID, layer, nhid),
                self.rowlocal(R.SITE_FFN_OUT, layer, D)]


class DropHook:
    """The `drop=` callable of the restatement: hands out the given keep-scales in call order."""

    def __init__(self, scales):
        self.scales, self.i = list(scales), 0

    def __call__(self, t):
        m = self.scales[self.i]
        self.i += 1
        assert tuple(m.shape) == tuple(t.shape), (self.i - 1, tuple(m.shape), tuple(t.shape))
        return t * m


def rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def rel2(a, b):
    return float(np.linalg.norm((a - b).ravel().astype(np.float64)) / (np.linalg.norm(b.ravel().astype(np.float64)) + 1e-30))


def _np(d):
    return {k: v.detach().numpy() for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# a. observation embedding and the sensor stage
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def obs_case(T, B, F, d=4):
    rng = np.random.default_rng(T * 7 + B)
    src = torch.from_numpy(rng.standard_normal((T, B, 2 * F)).astype(np.float32))
    src[:, :, :F] *= torch.from_numpy((rng.random((T, B, F)) < 0.6).astype(np.float32))
    R_u = torch.from_numpy(rng.standard_normal((1, F * d)).astype(np.float32))
    dX = torch.from_numpy(rng.standard_normal((B, F, T * d)).astype(np.float32))
    return dict(T=T, B=B, F=F, d=d, src=src, R_u=R_u, dX=dX)


@functools.lru_cache(maxsize=None)
def obs_reference(T, B, F, variant=None):
    """X[b, f, t*d + c] = drop(relu(src[t, b, f] * R_u[f*d + c])) and dR_u, float64."""
    c = obs_case(T, B, F)
    d = c["d"]
    ru = c["R_u"].double().requires_grad_(True)
    h = torch.relu(torch.repeat_interleave(c["src"][:, :, :F].double(), d, dim=-1) * ru)
    h = h * Masks(SEED, P_DROP, T, B, variant=variant).obs(F, d)
    X = h.view(T, B, F, d).permute(1, 2, 0, 3).reshape(B, F, T * d)
    (g,) = torch.autograd.grad(X, ru, c["dX"].double())
    return _np(dict(X=X, dR_u=g))


SENSOR_NAMES = ("R_u", "W1", "b1", "W2", "b2")


@functools.lru_cache(maxsize=None)
def sensor_case(F, T, B):
    d, K = 4, T * 4
    b = synth.make_batch(dict(d_inp=F, max_len=T, static=True, d_static=3, n_classes=2), B, seed=F + B, density=0.6)
    shapes = [(1, F * d), (K, K), (K,), (K, K), (K,)]
    p = {n: synth.param_values("k1r." + n, s, seed=4) for n, s in zip(SENSOR_NAMES, shapes)}
    p["R_u"] = p["R_u"] * 3.0
    gs = synth.make_structure(dict(d_inp=F), "sparse")
    dz = torch.from_numpy(np.random.default_rng(F + T).standard_normal((T, B, F * d + 16)).astype(np.float32))
    return dict(F=F, T=T, B=B, d=d, batch=b, p=p, gs=gs, dz=dz)


@functools.lru_cache(maxsize=None)
def sensor_reference(F, T, B, variant=None):
    """The de-duplicated (non-faithful) branch of oracle/restatement.py raindrop_v2_forward up to `out`, float64, the mask after the
    ReLU of the embedding; z's message-passing columns and the five gradients."""
    c = sensor_case(F, T, B)
    d, K = c["d"], T * c["d"]
    p = {n: t.double().requires_grad_(True) for n, t in c["p"].items()}
    _, s = O2.aggregate_coefficients(c["gs"].numpy())
    s = s.double()
    h = torch.relu(torch.repeat_interleave(c["batch"]["src"][:, :, :F].double(), d, dim=-1) * p["R_u"])
    h = h * Masks(SEED, P_DROP, T, B, variant=variant).obs(F, d)
    x = h.view(T, B, F, d).permute(1, 2, 0, 3).reshape(B, F, K)
    y1 = torch.relu(torch.nn.functional.linear(x, p["W1"], p["b1"])) * s[None, :, None]
    y2 = torch.relu(torch.nn.functional.linear(y1, p["W2"], p["b2"])) * s[None, :, None]
    out = y2.view(B, F, T, d).permute(2, 0, 1, 3).reshape(T, B, F * d)
    g = torch.autograd.grad(out, [p[n] for n in SENSOR_NAMES], c["dz"][:, :, : F * d].double())
    res = dict(z=out)
    res.update(zip(SENSOR_NAMES, g))
    return _np(res)


# ---------------------------------------------------------------------------------------------------------------------------------
# b. attention core
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def attn_case(T, B, F, nhead):
    """qkv, dout and a key mask: sample 0 full length, sample 1 of length <= 20 (dead key tiles), the last sample an arbitrary
    non-prefix mask (key 0 always live)."""
    D = F * 4 + 16
    rng = np.random.default_rng(T * 13 + B)
    qkv = torch.from_numpy(rng.standard_normal((T, B, 3 * D)).astype(np.float32))
    dout = torch.from_numpy(rng.standard_normal((T, B, D)).astype(np.float32))
    lengths = rng.integers(1, T + 1, size=B)
    lengths[0] = T
    lengths[1] = min(T, 20) - 3
    m = O2.padding_mask(lengths, T)
    m[B - 1] = rng.random(T) < 0.3
    m[B - 1, 0] = False
    return dict(T=T, B=B, F=F, nhead=nhead, D=D, qkv=qkv, dout=dout, mask=torch.from_numpy(m))


@functools.lru_cache(maxsize=None)
def attn_reference(T, B, F, nhead, layer, variant=None):
    """softmax(q k^T / sqrt(hd), masked keys at -inf), THEN the keep-scale, times v (torch: F.multi_head_attention_forward drops the
    normalised probabilities); lse is the log-sum-exp of the scaled, masked, UNDROPPED scores."""
    c = attn_case(T, B, F, nhead)
    D, hd = c["D"], c["D"] // nhead
    q64 = c["qkv"].double().requires_grad_(True)
    q, k, v = q64[..., :D], q64[..., D:2 * D], q64[..., 2 * D:]
    sh = lambda t: t.reshape(T, B, nhead, hd).permute(1, 2, 0, 3)                       # [B,H,T,hd]
    S = (sh(q) / math.sqrt(hd)) @ sh(k).transpose(-1, -2)
    S = S.masked_fill(c["mask"][:, None, None, :], float("-inf"))
    keep = Masks(SEED, P_DROP, T, B, variant=variant).prob(layer, nhead)
    out = ((torch.softmax(S, -1) * keep) @ sh(v)).permute(2, 0, 1, 3).reshape(T, B, D)
    (g,) = torch.autograd.grad(out, q64, c["dout"].double())
    return _np(dict(out=out, lse=torch.logsumexp(S, -1), dqkv=g))


# ---------------------------------------------------------------------------------------------------------------------------------
# c. encoder layer, padded layout
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def enc_case(T, B, F, nhead):
    D, nhid = F * 4 + 16, 2 * F * 4
    rng = np.random.default_rng(T * 31 + B)
    x = torch.from_numpy(rng.standard_normal((T, B, D)).astype(np.float32))
    lengths = rng.integers(1, T + 1, size=B)
    lengths[0] = T
    mask = torch.from_numpy(O2.padding_mask(lengths, T))
    dy = torch.from_numpy(rng.standard_normal((T, B, D)).astype(np.float32))
    shapes = {"self_attn.in_proj_weight": (3 * D, D), "self_attn.in_proj_bias": (3 * D,),
              "self_attn.out_proj.weight": (D, D), "self_attn.out_proj.bias": (D,),
              "linear1.weight": (nhid, D), "linear1.bias": (nhid,), "linear2.weight": (D, nhid),
              "linear2.bias": (D,), "norm1.weight": (D,), "norm1.bias": (D,), "norm2.weight": (D,), "norm2.bias": (D,)}
    p = {n: synth.param_values("L." + n, shapes[n], seed=T) for n in ENC_NAMES}
    return dict(T=T, B=B, F=F, nhead=nhead, D=D, nhid=nhid, x=x, mask=mask, dy=dy, p=p)


@functools.lru_cache(maxsize=None)
def enc_reference(T, B, F, nhead, layer, variant=None):
    """oracle/restatement.py encoder_layer in float64 with the four masks of `layer`; the output and all 13 gradients."""
    c = enc_case(T, B, F, nhead)
    xr = c["x"].double().requires_grad_(True)
    pr = {("L." + n): t.double().requires_grad_(True) for n, t in c["p"].items()}
    hook = DropHook(Masks(SEED, P_DROP, T, B, variant=variant).encoder(layer, nhead, c["D"], c["nhid"]))
    y = O2.encoder_layer(xr, c["mask"], pr, "L.", nhead, drop=hook)
    assert hook.i == 4
    g = torch.autograd.grad(y, [xr] + [pr["L." + n] for n in ENC_NAMES], c["dy"].double())
    res = dict(y=y)
    res.update(zip(("x",) + ENC_NAMES, g))
    return _np(res)


# ---------------------------------------------------------------------------------------------------------------------------------
# d. whole step on the token plan
# ---------------------------------------------------------------------------------------------------------------------------------
STEP_B, STEP_PARAM_SEED = 9, 7


@functools.lru_cache(maxsize=None)
def step_case():
    """P19 (F = 34, T = 60, two layers), B = 9; lengths include 1, T and ties (sample 0 is full length)."""
    cfg = synth.make_config("P19")
    gs = synth.make_structure(cfg, "sparse")
    batch = synth.make_batch(cfg, STEP_B, seed=33)
    T = cfg["max_len"]
    want = [T, 1, 17, 17, T, 40, 5, 40, 29]
    times = torch.cumsum(torch.rand(T, STEP_B, generator=torch.Generator().manual_seed(3)) + 0.01, 0)
    dead = torch.arange(T)[:, None] >= torch.tensor(want)[None, :]
    times[dead] = 0
    batch["times"] = times
    batch["src"] = batch["src"].clone()
    batch["src"][dead] = 0
    batch["lengths"] = torch.sum(times > 0, dim=0)
    assert batch["lengths"].tolist() == want
    return dict(cfg=cfg, gs=gs, batch=batch)


def step_params64():
    from tests.helpers import build_ours
    c = step_case()
    live = set(synth.live_parameter_names(c["cfg"]))
    m = build_ours(c["cfg"], c["gs"], "cpu", STEP_PARAM_SEED)
    return {n: t.detach().double().requires_grad_(True) for n, t in m.named_parameters() if n in live}


@functools.lru_cache(maxsize=None)
def step_reference(seed_eff, on_plan=True, variant=None):
    """oracle/restatement.py raindrop_v2_forward + cross entropy in float64 under the masks of effective seed `seed_eff`, numbered
    by the plan's rows and ranks (tests/helpers.plan_ref) or, `on_plan` False, by the padded layout.  loss, logits and every live
    gradient."""
    c = step_case()
    cfg, b = c["cfg"], c["batch"]
    T, B, F, d, H = cfg["max_len"], STEP_B, cfg["d_inp"], cfg["d_ob"], cfg["nhead"]
    D, nhid = F * d + 16, cfg["nhid"]
    pl = plan_ref(b["lengths"].numpy(), T)
    live = np.arange(T)[:, None] < np.clip(b["lengths"].numpy(), 0, T)[None, :]
    if on_plan:
        mk = Masks(seed_eff, P_DROP, T, B, rows=R.plan_rows(pl["off"], pl["rank"], T), bh_rank=pl["rank"], live=live, variant=variant)
    else:
        mk = Masks(seed_eff, P_DROP, T, B, variant=variant)
    scales = [mk.obs(F, d)]
    for layer in range(cfg["nlayers"]):
        scales += mk.encoder(layer, H, D, nhid)
    hook = DropHook(scales)
    p64 = step_params64()
    b64 = {k: (v.double() if (v is not None and v.is_floating_point()) else v) for k, v in b.items()}
    logits, _ = O2.raindrop_v2_forward(p64, cfg, b64["src"], b64["static"], b64["times"], b64["lengths"], c["gs"].double(),
                                       faithful=False, drop=hook)
    assert hook.i == len(scales)
    loss = torch.nn.functional.cross_entropy(logits, b["y"])
    names = sorted(p64)
    grads = torch.autograd.grad(loss, [p64[n] for n in names])
    res = dict(loss=loss.reshape(1), logits=logits)
    res.update(zip(names, grads))
    return _np(res)


# ---------------------------------------------------------------------------------------------------------------------------------
# the wrong variants against the bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def variant_margin(ref, wrong, bound_of):
    """How far a wrong variant moves the compared outputs, in units of the bound the kernel is held to: max over the compared
    tensors of error(wrong, ref) / bound, with `bound_of(name) -> (metric, bound)` the same metric and bound the device comparison
    uses for that tensor (metric: "rel" max-norm relative, "rel2" relative L2, "abs" max absolute)."""
    worst = 0.0
    for name, r in ref.items():
        metric, bound = bound_of(name)
        w = wrong[name]
        e = rel(w, r) if metric == "rel" else rel2(w, r) if metric == "rel2" else float(np.abs(w - r).max())
        worst = max(worst, e / bound)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# bounds: the project's dropout-off bounds of the same comparisons (tests/test_gpu_parity.py), per precision mode
# ---------------------------------------------------------------------------------------------------------------------------------
MODES = ("bf16x3", "fp32")


def obs_bound(mode):
    """Element-wise fp32 work, the same in both modes.  X is two roundings (the product, the 1/(1-p) scale) of 2^-24 each: 1e-6 of
    the max-norm.  dR_u sums T*B <= 300 fp32 terms per entry: worst case 300 * 2^-24 = 1.8e-5 of the sum of magnitudes: 2e-5."""
    return lambda name: ("rel", 1e-6 if name == "X" else 2e-5)


def sensor_bound(mode):
    """test_sensor_stage_vs_oracle: z within 2e-5 * TOL['x'] absolute, gradients through _grad_close(.., 1e-4, ..)."""
    x = 6.0 if mode == "bf16x3" else 1.0
    return lambda name: ("abs", 2e-5 * x) if name == "z" else (("rel", 1e-4) if mode == "fp32" else ("rel2", 2e-2))


def attn_bound(mode):
    """test_attention_core_vs_float64: 2e-4 of the max-norm, 2e-5 in fp32 mode."""
    tol = 2e-4 if mode == "bf16x3" else 2e-5
    return lambda name: ("rel", tol)


def enc_bound(mode):
    """test_encoder_layer_vs_oracle: output within 5e-5 * TOL['x'] absolute, gradients through _grad_close(.., 2e-4, ..) (fp32
    mode: max-norm relative 2e-4; split-bf16: relative L2 2e-2 and max-norm relative 0.25, no element excluded)."""
    x = 6.0 if mode == "bf16x3" else 1.0
    return lambda name: ("abs", 5e-5 * x) if name == "y" else (("rel", 2e-4) if mode == "fp32" else ("rel2", 2e-2))
