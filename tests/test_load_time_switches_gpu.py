"""GPU: the kernel paths behind the switches the library reads ONCE per process (function-local statics: RD_LN_VEC, RD_LN_FUSE,
RD_LNB_FUSE, RD_REDUCE_WIDE, RD_ROWGEMM, RD_GEMM_XCD, RD_SPLITK_XCD, RD_WGRAD_TILE, RD_ATTN_FWD_W8, RD_ATTN_BWD_W8, RD_GEMM_PANEL,
RD_GEMM_NPRE).  monkeypatch.setenv cannot reach them, so each value runs in a fresh child process (tests/switch_child.py), one
child per case and one for the default environment, started strictly one after the other and each exactly once; nothing is
removed from the inherited environment.

Per case (CASES below):
  * PATH.  The launch log of the child (include/raindrop_hip_debug.h rd_debug_launch_log: the names the launch sites report) must
    hold the kernels the switch selects and none of those it replaces -- `expect`: (regex over item keys, names that must occur in
    the union of those items' logs, names that must not; a trailing * makes a name a prefix).  The default child asserts the
    complementary names.  tests/test_load_time_switches_host.py checks that every name is one a launch site can report.
  * ACCURACY against float64 (oracle.restatement, the attention formula of test_attention_core_vs_float64, dy^T x in double), at
    the bounds the suite holds the default path to in the split-bf16 mode (BOUNDS below names the test each comes from).
  * AGAINST THE DEFAULT CHILD.  Bit-identical where the switch only changes which workgroup computes a tile or when loads are issued:
      RD_GEMM_XCD    -- rd_gemm.hip k_gemm_bf16x3 `swz`, k_gemm_panel* `lin`: the map blockIdx -> (row block, column block) only; every
                        tile is still one workgroup's whole reduction in the same order;
      RD_SPLITK_XCD  -- k_gemm_bf16x3 `slice_xcd`: the map blockIdx -> (tile, reduction slice z) only; the slices' bounds
                        (k_per_split) and the fixed-order reduce over z are unchanged;
      RD_GEMM_NPRE   -- the <.., NPRE = 4> instantiation requests its (at most four) 64-k tiles up front and then stages and
                        multiplies them in the same order with the same MFMA sequence as the looped form.
    Everywhere else the summation order changes (another tile shape, another reduce tree, LayerNorm partials per 16 rows, ..): the
    float64 bound only, the distance to the default child is printed.
  * DROPOUT (p = 0.2) has no float64 reference: the attention kernels are compared with the exact-fp32 kernels of the same child
    under the same seed (RD_ATTN_B16=0, read per call), the encoder layer with the default child's run; twice the p = 0 bound of
    the same quantity (a wrong mask moves an element by O(1)).
  * No NaN in any output (the children pre-fill recycled device memory and their own output buffers with NaN).
  * `step` under RD_LN_FUSE=0 / RD_LNB_FUSE=0 / RD_ROWGEMM=0: plan_supported read the same environment, so step.plan is None, the
    step does not raise, and loss / logits / gradients meet the default child's (token plan on) within the bounds
    test_static_train_step_matches_autograd holds its two sides to.

Attention in the single-product bf16 mode has no bound in the suite against float64.  The one used here comes from the format: bf16
rounds to 8 significant bits, unit roundoff u = 2^-9; the longest chain from qkv to dqkv rounds eight operands (q, k for the
scores; p, v for the output; dout, v for dP; dS and q / k for the gradients), each by at most u of its value, and a score error
enters the probabilities through exp with derivative <= 1: 8 u first order, doubled for the second-order terms and the
max-norm over a few thousand elements = 16 u = 3.1e-2 of the tensor's max-norm (the logits bound test_plain_bf16_mode_against_golden
uses for this mode is 3e-2 as well).  An index or mask error is O(1).

FAULTS.  A child that ends on a signal, on exit status 134 / 139, at its time limit or with a HIP error is recorded; every later case
of the module then FAILS at once, naming it, without starting another GPU process.  Nothing is retried."""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from oracle import restatement as O2
from tests import switch_child as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# wall time of the default child (all probes, 71 items) measured on an MI355X box: 3.7 s (the other children 2.1 - 3.2 s); the limit
# is five times that, at least 120 s
MEASURED_DEFAULT_CHILD_S = 3.7
CHILD_TIMEOUT_S = max(120.0, 5.0 * MEASURED_DEFAULT_CHILD_S)

U_BF16 = 2.0 ** -9
BOUNDS = {
    "attn_bf16x3": 2e-4,                 # test_attention_core_vs_float64 (split-bf16 mode), max-norm relative
    "attn_bf16": 16 * U_BF16,            # module docstring
    "layer_y": 5e-5 * 6.0,               # test_row_block_layer_vs_float64 / test_encoder_layer_vs_oracle, absolute
    "layer_gate_free": 2e-4,             # test_row_block_layer_vs_float64: linear2 / norm2 gradients, max-norm relative
    "grad_l2": 2e-2, "grad_max": 0.25,   # test_gpu_parity._grad_close in the split-bf16 mode
    # test_linear_fwd_bwd / test_split_k_weight_gradients_vs_float64 and test_sensor_stage_vs_oracle: their exact-fp32 figures, WITHOUT
    # the factor 6 those tests grant the split-bf16 mode (measured here in that mode: y / dx <= 8.6e-6, dW <= 5.8e-6, db <= 2.7e-7, z 5.4e-7)
    "linear_y": 1e-5, "linear_dw": 2e-5, "linear_db": 2e-5,
    "sensor_z": 2e-5, "sensor_pe": 2e-6,
    "step_loss": 5e-6, "step_rel": 5e-5,                                     # test_static_train_step_matches_autograd (fused head, split-bf16)
}

B16_ITEMS = r"^attn/.*/p0(\.2)?$"        # the bf16 attention kernels (not the exact-fp32 ones of the dropout comparison)
RB_ATTN_ITEMS = r"^enc_rb/.*/T(13B5|37B27)/"
BIG_WGRAD = r"^linear/wgrad/M(3001|4099|5000)N"
ALL = "attn,enc_rb,enc_small,linear,sensor_p12,step"

# case id -> (environment, probes, [(items regex, must occur, must not occur)], bit-identical to the default child)
CASES = {
    "default": ({}, ALL, [
        (B16_ITEMS, ["k_attn_fwd_one_b16w", "k_attn_bwd_one_b16w"], ["k_attn_fwd_one_b16", "k_attn_bwd_one_b16"]),
        (RB_ATTN_ITEMS, ["k_attn_fwd_one_b16w", "k_attn_bwd_one_b16w"], ["k_attn_fwd_one_b16", "k_attn_bwd_one_b16"]),
        (r"^enc_rb/", ["k_rowgemm", "k_rowgemm_ln", "k_rowgemm_lnb", "k_twg", "k_twg_reduce"],
         ["k_add_ln_fwd*", "k_ln_bwd*", "k_gemm_panel*", "k_reduce_wide", "k_splitk_reduce2"]),
        (r"^enc_small/", ["k_add_ln_fwd_v", "k_ln_bwd_v"], ["k_add_ln_fwd_r*", "k_ln_bwd_r*", "k_rowgemm*"]),
        (r"^enc_small/T(130|40)B", ["k_gemm_panel*"], []),
        (r"^linear/", ["k_gemm_bf16x3_64x64_npre", "k_gemm_bf16x3_64x64"], ["k_gemm_bf16x3_*_rowmajor", "k_gemm_bf16x3_*_zgrid"]),
        (r"^linear/fb/M(7|64)N", ["k_gemm_bf16x3_64x64_npre"], ["k_gemm_bf16x3_64x64"]),
        (r"^linear/wgrad/", ["k_gemm_bf16x3_64x64", "k_gemm_bf16x3_64x64_npre", "k_reduce_wide"], ["k_splitk_reduce2", "k_gemm_bf16x3_128x128*"]),
        (r"^sensor_p12/.*/stream1", ["k_gemm_panel"], ["k_gemm_panel_rowmajor", "k_gemm_panel_wide*", "k_gemm_panel_pc*"]),
        (r"^sensor_p12/.*/stream0", ["k_gemm_panel", "k_gemm_bf16x3_64x64"], ["k_gemm_bf16x3_128x128*", "k_gemm_bf16x3_*_rowmajor"]),
    ], False),
    "RD_ATTN_FWD_W8=0": ({"RD_ATTN_FWD_W8": "0"}, "attn,enc_rb@T13B5@T37B27", [
        (B16_ITEMS, ["k_attn_fwd_one_b16", "k_attn_bwd_one_b16w"], ["k_attn_fwd_one_b16w", "k_attn_bwd_one_b16"]),
        (RB_ATTN_ITEMS, ["k_attn_fwd_one_b16", "k_attn_bwd_one_b16w"], ["k_attn_fwd_one_b16w", "k_attn_bwd_one_b16"]),
    ], False),
    "RD_ATTN_BWD_W8=0": ({"RD_ATTN_BWD_W8": "0"}, "attn,enc_rb@T13B5@T37B27", [
        (B16_ITEMS, ["k_attn_fwd_one_b16w", "k_attn_bwd_one_b16"], ["k_attn_fwd_one_b16", "k_attn_bwd_one_b16w"]),
        (RB_ATTN_ITEMS, ["k_attn_fwd_one_b16w", "k_attn_bwd_one_b16"], ["k_attn_fwd_one_b16", "k_attn_bwd_one_b16w"]),
    ], False),
    "RD_LN_FUSE=0": ({"RD_LN_FUSE": "0"}, "enc_rb,step", [
        (r"^enc_rb/", ["k_rowgemm", "k_add_ln_fwd_v", "k_twg", "k_rowgemm_lnb"], ["k_rowgemm_ln", "k_add_ln_fwd_r*", "k_add_ln_fwd"]),
    ], False),
    "RD_LNB_FUSE=0": ({"RD_LNB_FUSE": "0"}, "enc_rb,step", [
        (r"^enc_rb/", ["k_rowgemm", "k_rowgemm_ln", "k_ln_bwd_v", "k_twg", "k_twg_reduce"], ["k_rowgemm_lnb", "k_ln_bwd_r*", "k_ln_bwd"]),
    ], False),
    "RD_LN_VEC=0": ({"RD_LN_VEC": "0"}, "enc_small", [
        (r"^enc_small/", ["k_add_ln_fwd_r1", "k_add_ln_fwd_r2", "k_add_ln_fwd_r4", "k_ln_bwd_r1", "k_ln_bwd_r2", "k_ln_bwd_r4"],
         ["k_add_ln_fwd_v", "k_ln_bwd_v"]),
        (r"^enc_small/T130B", ["k_add_ln_fwd_r2", "k_ln_bwd_r2"], ["k_add_ln_fwd_r1", "k_add_ln_fwd_r4"]),
        (r"^enc_small/T40B", ["k_add_ln_fwd_r4", "k_ln_bwd_r4"], ["k_add_ln_fwd_r1", "k_add_ln_fwd_r2"]),
    ], False),
    "RD_LN_VEC=0 RD_LN_FUSE=0 RD_LNB_FUSE=0": ({"RD_LN_VEC": "0", "RD_LN_FUSE": "0", "RD_LNB_FUSE": "0"}, "enc_rb", [
        (r"^enc_rb/", ["k_rowgemm", "k_add_ln_fwd_r3", "k_ln_bwd_r3", "k_twg", "k_twg_reduce"],
         ["k_rowgemm_ln", "k_rowgemm_lnb", "k_add_ln_fwd_v", "k_ln_bwd_v"]),
    ], False),
    "RD_ROWGEMM=0": ({"RD_ROWGEMM": "0"}, "enc_rb,step", [
        (r"^enc_rb/", ["k_add_ln_fwd_v", "k_ln_bwd_v", "k_gemm_panel*"], ["k_rowgemm*", "k_twg*"]),
        (r"^enc_rb/.*/T37B27/", ["k_gemm_bf16x3_64x64"], ["k_gemm_bf16x3_*_zgrid"]),     # 999 rows: split-K weight gradients
    ], False),
    "RD_GEMM_PANEL=0": ({"RD_GEMM_PANEL": "0"}, "sensor_p12,enc_small", [
        (r"^sensor_p12/", ["k_gemm_bf16x3_*"], ["k_gemm_panel*"]),
        (r"^enc_small/", ["k_gemm_bf16x3_*"], ["k_gemm_panel*"]),
    ], False),
    "RD_GEMM_XCD=0": ({"RD_GEMM_XCD": "0"}, "linear,sensor_p12", [
        (r"^linear/fb/", ["k_gemm_bf16x3_64x64_rowmajor", "k_gemm_bf16x3_64x64_npre_rowmajor"], []),
        (r"^linear/fb/M(7|64)N", ["k_gemm_bf16x3_64x64_npre_rowmajor"], ["k_gemm_bf16x3_64x64_npre", "k_gemm_bf16x3_64x64"]),
        (r"^sensor_p12/", ["k_gemm_panel_rowmajor"], ["k_gemm_panel"]),
    ], True),
    "RD_SPLITK_XCD=0": ({"RD_SPLITK_XCD": "0"}, "linear@wgrad", [
        (r"^linear/wgrad/", ["k_gemm_bf16x3_64x64_zgrid", "k_gemm_bf16x3_64x64_npre_zgrid", "k_reduce_wide"],
         ["k_gemm_bf16x3_64x64", "k_gemm_bf16x3_64x64_npre"]),
    ], True),
    "RD_WGRAD_TILE=128": ({"RD_WGRAD_TILE": "128"}, "linear@wgrad,sensor_p12@stream0", [
        (BIG_WGRAD, ["k_gemm_bf16x3_128x128"], ["k_gemm_bf16x3_64x64"]),
        (r"^linear/wgrad/M1025N64", ["k_gemm_bf16x3_64x64_npre"], ["k_gemm_bf16x3_128x128"]),  # fewer than 96 rows: the 64 x 64 tile stays
        (r"^sensor_p12/", ["k_gemm_bf16x3_128x128"], []),
    ], False),
    "RD_REDUCE_WIDE=0": ({"RD_REDUCE_WIDE": "0"}, "linear@wgrad", [
        (r"^linear/wgrad/", ["k_splitk_reduce2", "k_gemm_bf16x3_64x64"], ["k_reduce_wide"]),
    ], False),
    "RD_GEMM_NPRE=0": ({"RD_GEMM_NPRE": "0"}, "linear", [
        (r"^linear/", ["k_gemm_bf16x3_64x64"], ["k_gemm_bf16x3_64x64_npre*"]),
    ], True),
}
SWITCHES = sorted({k for env, _, _, _ in CASES.values() for k in env})


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _rel2(a, b):
    return float(np.linalg.norm((a - b).ravel().astype(np.float64)) / (np.linalg.norm(b.ravel().astype(np.float64)) + 1e-30))


def _matches(name, pattern):
    return re.fullmatch(re.escape(pattern).replace(r"\*", ".*"), name) is not None


# ---- the children -----------------------------------------------------------------------------------------------------------------
class _Runs:
    """results by case id; `fault` = description of the first child that faulted, hung or was killed"""
    results, fault, tmp = {}, None, None


@pytest.fixture(scope="module", autouse=True)
def _scratch(tmp_path_factory):
    _Runs.results, _Runs.fault = {}, None
    _Runs.tmp = str(tmp_path_factory.mktemp("switch_children"))
    yield
    _Runs.results = {}


def _child(case):
    """The child of `case`, started on first use (at most one alive at a time: subprocess.run returns when it has ended)."""
    if case in _Runs.results:
        return _Runs.results[case]
    if _Runs.fault:
        pytest.fail("no GPU process started: an earlier child faulted -- " + _Runs.fault)
    env, probes, _, _ = CASES[case]
    out = os.path.join(_Runs.tmp, re.sub(r"[^A-Za-z0-9_]+", "_", case) + ".npz")
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, "-m", "tests.switch_child", "--probes", probes, "--out", out], env={**os.environ, **env},
                           timeout=CHILD_TIMEOUT_S, cwd=ROOT, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _Runs.fault = "child '%s' reached its time limit of %.0f s" % (case, CHILD_TIMEOUT_S)
        pytest.fail(_Runs.fault)
    wall = time.time() - t0
    tail = (r.stdout + r.stderr)[-2000:]
    print("child '%s': exit status %d after %.1f s" % (case, r.returncode, wall))
    if r.returncode < 0 or r.returncode in (134, 139):
        _Runs.fault = "child '%s' ended with status %d: %s" % (case, r.returncode, tail)
        pytest.fail(_Runs.fault)
    if r.returncode not in (0, 3) or not os.path.exists(out):
        pytest.fail("child '%s' ended with status %d and no result: %s" % (case, r.returncode, tail))
    z = np.load(out)
    res = {"log": json.loads(str(z["__log__"])), "err": json.loads(str(z["__err__"])), "wall": wall,
           "t": {k: z[k] for k in z.files if not k.startswith("__")}}
    if res["err"] and re.search(r"hip|illegal|fault|memory access", " ".join(res["err"].values()), re.I):
        _Runs.fault = "child '%s' met a device error: %s" % (case, res["err"])
        pytest.fail(_Runs.fault)
    _Runs.results[case] = res
    return res


def _item(res, key):
    pre = key + "|"
    return {k[len(pre):]: v for k, v in res["t"].items() if k.startswith(pre)}


# ---- float64 references, computed once per session ---------------------------------------------------------------------------------
_REF = {}


def _ref(kind, *args):
    k = (kind,) + args
    if k not in _REF:
        _REF[k] = {"attn": _ref_attn, "layer": _ref_layer, "linear": _ref_linear, "wgrad": _ref_wgrad, "sensor": _ref_sensor}[kind](*args)
    return _REF[k]


def _ref_attn(T, B, F, nhead):
    D = F * 4 + 16
    hd = D // nhead
    qkv, mask, dout = C.attn_inputs(T, B, F, nhead)
    q64 = qkv.double().requires_grad_(True)
    q, k, v = q64[..., :D], q64[..., D:2 * D], q64[..., 2 * D:]
    sh = lambda t: t.reshape(T, B, nhead, hd).permute(1, 2, 0, 3)
    S = (sh(q) / np.sqrt(hd)) @ sh(k).transpose(-1, -2)
    S = S.masked_fill(mask[:, None, None, :], float("-inf"))
    out64 = (torch.softmax(S, -1) @ sh(v)).permute(2, 0, 1, 3).reshape(T, B, D)
    (g64,) = torch.autograd.grad(out64, q64, dout.double())
    return {"out": out64.detach().numpy(), "dqkv": g64.numpy()}


def _ref_layer(T, B, D, nhid, nhead):
    from tests.test_rowgemm_variants_gpu import ENC_NAMES
    x, mask, dy, p = C.layer_inputs(T, B, D, nhid)
    x64 = x.double().requires_grad_(True)
    p64 = {("L." + n): t.double().requires_grad_(True) for n, t in p.items()}
    y = O2.encoder_layer(x64, mask, p64, "L.", nhead)
    g = torch.autograd.grad(y, [x64] + [p64["L." + n] for n in ENC_NAMES], dy.double())
    out = {"y": y.detach().numpy()}
    out.update({"d:" + n: t.numpy() for n, t in zip(("x",) + tuple(ENC_NAMES), g)})
    return out


def _ref_linear(M, N, K, act):
    x, W, b, dy = (t.double().requires_grad_(True) for t in C.linear_inputs(M, N, K))
    y = torch.nn.functional.linear(x, W, b)
    y = torch.relu(y) if act else y
    gx, gW, gb = torch.autograd.grad(y, [x, W, b], dy.detach())
    return {"y": y.detach().numpy(), "dx": gx.numpy(), "dW": gW.numpy(), "db": gb.numpy()}


def _ref_wgrad(M, N, K):
    x, dy = C.wgrad_inputs(M, N, K)
    return {"dW": (dy.double().t() @ x.double()).numpy(), "db": dy.double().sum(0).numpy()}


def _ref_sensor(B, kind):
    """the faithful per-sample, per-edge restatement of the stage (test_sensor_stage_vs_oracle), in float64"""
    cfg, gs, b, p, dz = C.sensor_inputs(B, kind)
    T, F, d = cfg["max_len"], cfg["d_inp"], 4
    K = T * d
    n = C.SENSOR_NAMES
    p = {k: t.double().requires_grad_(True) for k, t in p.items()}
    h = torch.relu(torch.repeat_interleave(b["src"][:, :, :F].double(), d, dim=-1) * p["R_u"])
    ei_np, ew_np = O2.build_graph(gs.numpy())
    ei, ew = torch.from_numpy(ei_np), torch.from_numpy(ew_np).double()
    cols = []
    for u in range(B):
        x = h[:, u, :].reshape(T, F, d).permute(1, 0, 2).reshape(F, K)
        x, a1 = O2.observation_propagation(x, ei, ew, p[n[1]], p[n[2]])
        x, _ = O2.observation_propagation(x, ei, a1.squeeze(-1), p[n[3]], p[n[4]])
        cols.append(x.view(F, T, d).permute(1, 0, 2).reshape(T, F * d))
    out_ref = torch.stack(cols, dim=1)
    g = torch.autograd.grad(out_ref, [p[k] for k in n], dz[:, :, : F * d].double())
    out = {"z": out_ref.detach().numpy(), "pe": O2.positional_encoding(b["times"], T).numpy(),
           "mask": O2.padding_mask(b["lengths"].numpy(), T)}
    out.update({"d:" + k: t.numpy() for k, t in zip(n, g)})
    return out


# ---- checks of one item ------------------------------------------------------------------------------------------------------------
GATE_FREE = ("linear2.weight", "linear2.bias", "norm2.weight", "norm2.bias")


def _check_layer(got, ref, scale, gate_free, bad, figs, key):
    ey = float(np.abs(got["y"] - ref["y"]).max())
    figs.append("%s y %.2e" % (key, ey))
    if not ey < BOUNDS["layer_y"] * scale:
        bad.append((key, "y", ey))
    for n in ref:
        if not n.startswith("d:"):
            continue
        e, e2 = _rel(got[n], ref[n]), _rel2(got[n], ref[n])
        figs.append("%s %.2e/%.2e" % (n[2:], e, e2))
        if gate_free and n[2:] in GATE_FREE:
            ok = e < BOUNDS["layer_gate_free"] * scale
        else:
            ok = e2 < BOUNDS["grad_l2"] * scale and e < BOUNDS["grad_max"] * scale
        if not ok:
            bad.append((key, n, e, e2))


def _check_item(key, res, dres, is_default, bad, figs):
    got = _item(res, key)
    for n, a in got.items():
        if a.dtype.kind == "f" and not np.isfinite(a).all():
            bad.append((key, n, "%d non-finite values" % int((~np.isfinite(a)).sum())))
    if any(b[0] == key for b in bad):
        return
    parts = key.split("/")
    if parts[0] == "attn":
        T, B, F, H = map(int, re.fullmatch(r"T(\d+)B(\d+)F(\d+)H(\d+)", parts[1]).groups())
        bound = BOUNDS["attn_" + parts[2]]
        if parts[3] == "p0":
            ref = _ref("attn", T, B, F, H)
            for n in ("out", "dqkv"):
                e = _rel(got[n], ref[n])
                figs.append("%s %s %.2e" % (key, n, e))
                if not e < bound:
                    bad.append((key, n, e, bound))
        elif parts[3] == "p0.2":
            ref = _item(res, key + "-fp32kernels")               # exact-fp32 kernels, same seed, same child
            for n in ("out", "dqkv"):
                e = _rel(got[n], ref[n])
                figs.append("%s %s vs fp32 kernels %.2e" % (key, n, e))
                if not e < 2 * bound:
                    bad.append((key, n, e, 2 * bound))
    elif parts[0] == "enc_rb":
        D, nhid = map(int, parts[1].split("x"))
        T, B = map(int, re.fullmatch(r"T(\d+)B(\d+)", parts[2]).groups())
        if parts[3] == "p0":
            _check_layer(got, _ref("layer", T, B, D, nhid, 2), 1.0, True, bad, figs, key)
        elif not is_default:
            _check_layer(got, _item(dres, key), 2.0, True, bad, figs, key + " vs default")
    elif parts[0] == "enc_small":
        T, B, F, H = map(int, re.fullmatch(r"T(\d+)B(\d+)F(\d+)H(\d+)", parts[1]).groups())
        _check_layer(got, _ref("layer", T, B, 4 * F + 16, 8 * F, H), 1.0, False, bad, figs, key)
    elif parts[0] == "linear":
        dims = tuple(map(int, re.findall(r"\d+", parts[2])))
        ref = _ref("linear", *dims) if parts[1] == "fb" else _ref("wgrad", *dims)
        for n, b in (("y", "linear_y"), ("dx", "linear_y"), ("dW", "linear_dw"), ("db", "linear_db")):
            if n in got:
                e = _rel(got[n], ref[n])
                figs.append("%s %s %.2e" % (key, n, e))
                if not e < BOUNDS[b]:
                    bad.append((key, n, e, BOUNDS[b]))
    elif parts[0] == "sensor_p12":
        B, kind = re.fullmatch(r"B(\d+)(\w+)", parts[1]).groups()
        ref = _ref("sensor", int(B), kind)
        nz = ref["z"].shape[-1]
        ez, epe = float(np.abs(got["z"][:, :, :nz] - ref["z"]).max()), float(np.abs(got["z"][:, :, nz:] - ref["pe"]).max())
        figs.append("%s z %.2e pe %.2e" % (key, ez, epe))
        if not (ez < BOUNDS["sensor_z"] and epe < BOUNDS["sensor_pe"] and np.array_equal(got["mask"].astype(bool), ref["mask"])):
            bad.append((key, "z / pe / mask", ez, epe))
        for n in C.SENSOR_NAMES:
            e, e2 = _rel(got["d:" + n], ref["d:" + n]), _rel2(got["d:" + n], ref["d:" + n])
            figs.append("%s %.2e/%.2e" % (n, e, e2))
            if not (e2 < BOUNDS["grad_l2"] and e < BOUNDS["grad_max"]):
                bad.append((key, n, e, e2))
    elif parts[0] == "step":
        if is_default:
            if int(got["plan_none"]) != 0:
                bad.append((key, "the default step did not take the token plan"))
            return
        ref = _item(dres, key)
        if int(got["plan_none"]) != 1:
            bad.append((key, "step.plan is not None although plan_supported read the switch"))
        el = abs(float(got["loss"]) - float(ref["loss"]))
        figs.append("%s loss %.2e" % (key, el))
        if not el < BOUNDS["step_loss"]:
            bad.append((key, "loss", el))
        for n in ref:
            if n == "logits" or n.startswith("d:"):
                e = _rel(got[n], ref[n])
                figs.append("%s %.2e" % (n, e))
                if not e < BOUNDS["step_rel"]:
                    bad.append((key, n, e))


@pytest.mark.parametrize("case", list(CASES), ids=[c.replace(" ", "+") for c in CASES])
def test_switch_path(case):
    default = _child("default")
    res = default if case == "default" else _child(case)
    env, probes, expect, identical = CASES[case]
    bad, figs = [], []
    if res["err"]:
        bad.append(("raised", res["err"]))
    keys = C.item_keys(probes)
    missing = [k for k in keys if k not in res["log"]]
    if missing and not res["err"]:
        bad.append(("items not run", missing))
    # ---- path ----
    for pattern, want, never in expect:
        items = [k for k in res["log"] if re.search(pattern, k)]
        names = sorted({n for k in items for n in res["log"][k]})
        if not items:
            bad.append(("path", pattern, "no item matches"))
        for w in want:
            if not any(_matches(n, w) for n in names):
                bad.append(("path", pattern, "missing " + w, names))
        for w in never:
            hit = [n for n in names if _matches(n, w)]
            if hit:
                bad.append(("path", pattern, "launched " + ", ".join(hit)))
    # ---- values ----
    for key in keys:
        if key in res["log"] and key not in res["err"]:
            _check_item(key, res, default, case == "default", bad, figs)
    # ---- against the default child ----
    worst = 0.0
    if case != "default":
        for k, a in res["t"].items():
            if k.split("|")[0] in res["err"] or k not in default["t"]:
                continue
            d = default["t"][k]
            if identical and not np.array_equal(a, d):
                bad.append(("not bit-identical to the default child", k, _rel(a, d) if a.dtype.kind == "f" else None))
            if a.dtype.kind == "f" and a.size and np.isfinite(a).all():
                worst = max(worst, _rel(a, d))
    print("case %s (%.1f s): %s" % (case, res["wall"], "; ".join(figs)))
    print("case %s: largest max-norm distance of any tensor to the default child %.3e" % (case, worst))
    assert not bad, bad
