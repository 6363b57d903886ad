"""Child process of tests/test_load_time_switches_gpu.py (not collected by pytest: run as a module).

    python -m tests.switch_child --probes attn,enc_rb@T13B5@T37B27 --out FILE.npz

Twelve switches of the library are read once, into function-local statics, when the code that asks for them first runs; only a
fresh process can see another value.  This module runs under WHATEVER environment it was started with -- it sets none of those
switches -- turns the host-side launch log on (include/raindrop_hip_debug.h rd_debug_launch_log), runs the named probes once each on
fixed seeds and writes, per item of a probe, every output tensor and the names the launch sites reported while the item ran.
The per-call switches a probe needs to reach the launches it is about (RD_ENC_FUSE, RD_ATTN_FUSE, RD_ATTN_B16, RD_PANEL_WIDE,
RD_PANEL_PC, RD_K1_WGRAD_STREAM: all read at every call) are set around the call and handed back.

A probe name may carry filters, `name@part@part`: only the items whose key contains one of the parts run.

Before an item runs, blocks of device memory at least as large as its outputs are filled with NaN and handed back to torch's
caching allocator (one block of the outputs' size + a handful of small ones for the small-block pool), and every output buffer the
probe allocates itself starts as NaN: a tile no workgroup wrote reads as NaN in the parent, not as a stale correct value.

The inputs of the probes are host functions of this module (`*_inputs`): the parent computes its float64 references from the same
tensors.  File layout: `<item key>|<tensor name>` arrays, `__log__` (JSON {item key: [launch names]}), `__err__` (JSON {item key:
text of the exception}); the first item that raises ends the run (exit status 3) -- nothing is started after a failed call.
"""
import argparse
import contextlib
import ctypes
import json
import os
import sys

import numpy as np
import torch

from oracle import restatement as O2
from raindrop_amd import synth

DEV = "cuda"

# (T, B, F, nhead): single-tile attention (T <= 64); head_dim 18 / 42 / 76 / 16 / 96
ATTN_SHAPES = [(7, 3, 5, 2), (16, 5, 17, 2), (33, 4, 34, 2), (60, 9, 34, 2), (64, 3, 12, 4), (64, 2, 44, 2)]
ATTN_MODES = [(1, "bf16x3"), (2, "bf16")]
ATTN_SEED = 77
# (F, D, nhid) of the row-block kernels and (T, B): tests/test_rowgemm_variants_gpu.py WIDTHS / SMALL
RB_WIDTHS = [(34, 152, 272), (35, 156, 260)]
RB_SHAPES = [(7, 3), (13, 5), (37, 27), (70, 3)]
# (T, B, F, nhead) outside the row-block kernels: D = 36, 64, 84, 256 -> 1, 1, 2, 4 column groups of 64
SMALL_SHAPES = [(7, 3, 5, 2), (64, 3, 12, 4), (130, 2, 17, 2), (40, 3, 60, 2)]
LINEAR_SHAPES = [(7, 5, 3, 1), (64, 64, 32, 0), (130, 186, 186, 1), (257, 34, 6, 0), (513, 272, 152, 1), (1000, 456, 152, 0)]
WGRAD_SHAPES = [(1025, 64, 48), (3001, 456, 152), (4099, 152, 152), (5000, 272, 152)]
SENSOR_CASES = [(3, "ones"), (5, "sparse")]
SENSOR_NAMES = ["R_u", "ob_propagation.lin_value.weight", "ob_propagation.lin_value.bias",
                "ob_propagation_layer2.lin_value.weight", "ob_propagation_layer2.lin_value.bias"]
STEP_B = 6


# ---- inputs (host tensors; shared with the parent's references) --------------------------------------------------------------------
def attn_inputs(T, B, F, nhead):
    """qkv, key mask, dout as tests/test_gpu_parity.py test_attention_core_vs_float64 builds them"""
    D = F * 4 + 16
    rng = np.random.default_rng(T * 13 + B)
    qkv = torch.from_numpy(rng.standard_normal((T, B, 3 * D)).astype(np.float32))
    lengths = torch.from_numpy(rng.integers(1, T + 1, size=B)).long()
    lengths[0] = T
    if B > 2:
        lengths[1] = min(T, 20)
    mask = torch.from_numpy(O2.padding_mask(lengths.numpy(), T))
    dout = torch.from_numpy(rng.standard_normal((T, B, D)).astype(np.float32))
    return qkv, mask, dout


def layer_inputs(T, B, D, nhid):
    from tests.test_rowgemm_variants_gpu import _layer_inputs
    return _layer_inputs(T, B, D, nhid, seed=T * 31 + B)


def linear_inputs(M, N, K):
    """x, W, b, dy as tests/test_gpu_parity.py test_linear_fwd_bwd builds them"""
    rng = np.random.default_rng(M * 7 + N)
    x = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32))
    W = torch.from_numpy((rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal((N,)).astype(np.float32))
    dy = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32))
    return x, W, b, dy


def wgrad_inputs(M, N, K):
    rng = np.random.default_rng(M + 3 * N + K)
    x = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32))
    dy = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32))
    return x, dy


def sensor_inputs(B, kind):
    """P12 case of tests/test_gpu_parity.py test_sensor_stage_vs_oracle: configuration, structure, batch, parameters, dz"""
    cfg = synth.make_config("P12")
    gs = synth.make_structure(cfg, kind)
    b = synth.make_batch(cfg, B, seed=21)
    T, F, d = cfg["max_len"], cfg["d_inp"], 4
    K = T * d
    shapes = [(1, F * d), (K, K), (K,), (K, K), (K,)]
    p = {n: synth.param_values(n, s, seed=5) for n, s in zip(SENSOR_NAMES, shapes)}
    dz = torch.from_numpy(np.random.default_rng(3).standard_normal((T, B, F * d + 16)).astype(np.float32))
    return cfg, gs, b, p, dz


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _poison(nbytes):
    """NaN into the blocks the next allocations are carved from (see the module docstring)"""
    blocks = [_nan(max(1, nbytes // 4))] + [_nan(16384) for _ in range(16)]
    torch.cuda.synchronize()
    del blocks


def _np(t):
    return t.detach().cpu().numpy()


def _numel(*ts):
    return sum(int(t.numel()) for t in ts)


# ---- probes: each yields (item key, bytes of its outputs, function -> {name: array}) -----------------------------------------------
def probe_attn():
    from raindrop_amd import _lib
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def run(T, B, F, nhead, mode, p_drop, b16):
        D = F * 4 + 16
        qkv, mask, dout = (t.to(DEV) for t in attn_inputs(T, B, F, nhead))
        out, lse, dqkv, ws = _nan(T, B, D), _nan(B, nhead, T), _nan(T, B, 3 * D), _nan(B, nhead, T)
        shp = _lib.shape(B, T, F, 4, nhead=nhead, nhid=2 * F * 4)
        _lib.call("rd_set_precision", mode)
        try:
            with _env(**({} if b16 else {"RD_ATTN_B16": "0"})):
                _lib.call("rd_attention_fwd", ctypes.byref(shp), 0, P(qkv), P(mask), p_drop, ATTN_SEED, P(out), P(lse), None)
                _lib.call("rd_attention_bwd", ctypes.byref(shp), 0, P(qkv), P(mask), p_drop, ATTN_SEED, P(out), P(lse), P(dout), P(dqkv),
                          P(ws), None)
            torch.cuda.synchronize()
        finally:
            _lib.call("rd_set_precision", 1)
        return {"out": _np(out), "lse": _np(lse), "dqkv": _np(dqkv)}

    for T, B, F, nhead in ATTN_SHAPES:
        nbytes = 4 * (T * B * (F * 4 + 16) * 4 + 2 * B * nhead * T)
        for mode, mname in ATTN_MODES:
            tag = "attn/T%dB%dF%dH%d/%s" % (T, B, F, nhead, mname)
            yield tag + "/p0", nbytes, (lambda a=(T, B, F, nhead, mode): run(*a, 0.0, True))
            yield tag + "/p0.2", nbytes, (lambda a=(T, B, F, nhead, mode): run(*a, 0.2, True))
            yield tag + "/p0.2-fp32kernels", nbytes, (lambda a=(T, B, F, nhead, mode): run(*a, 0.2, False))


def _layer(T, B, F, D, nhid, nhead, p_drop, row_blocks):
    from raindrop_amd import _lib
    from tests.test_rowgemm_variants_gpu import ENC_NAMES, _run_layer, _to_dev
    x, mask, dy, p = _to_dev(*layer_inputs(T, B, D, nhid))
    shp = _lib.shape(B, T, F, 4, nhead=nhead, nhid=nhid)
    with _env(**({"RD_ENC_FUSE": "0", "RD_ATTN_FUSE": "0"} if row_blocks else {})):
        y, g = _run_layer(x, mask, dy, p, shp, p_drop)
    out = {"y": y}
    out.update({"d:" + n: a for n, a in zip(("x",) + tuple(ENC_NAMES), g)})
    return out


def _layer_bytes(T, B, D, nhid):
    return 4 * (2 * T * B * D + 4 * D * D + 2 * D * nhid + 9 * D + nhid)


def probe_enc_rb():
    for F, D, nhid in RB_WIDTHS:
        for T, B in RB_SHAPES:
            for p_drop in (0.0, 0.2):
                yield ("enc_rb/%dx%d/T%dB%d/p%g" % (D, nhid, T, B, p_drop), _layer_bytes(T, B, D, nhid),
                       (lambda a=(T, B, F, D, nhid, 2, p_drop): _layer(*a, True)))


def probe_enc_small():
    for T, B, F, nhead in SMALL_SHAPES:
        D, nhid = 4 * F + 16, 8 * F
        yield ("enc_small/T%dB%dF%dH%d" % (T, B, F, nhead), _layer_bytes(T, B, D, nhid),
               (lambda a=(T, B, F, D, nhid, nhead, 0.0): _layer(*a, False)))


def probe_linear():
    from raindrop_amd import _lib, ops

    def fwd_bwd(M, N, K, act):
        x, W, b, dy = (t.to(DEV) for t in linear_inputs(M, N, K))
        x.requires_grad_(True), W.requires_grad_(True), b.requires_grad_(True)
        y = ops.linear(x, W, b, act)
        hx, hW, hb = torch.autograd.grad(y, [x, W, b], dy)
        torch.cuda.synchronize()
        return {"y": _np(y), "dx": _np(hx), "dW": _np(hW), "db": _np(hb)}

    def wgrad(M, N, K):
        """rd_linear_bwd_weight by itself: the split-K product and its fixed-order reduce are the only launches of the item"""
        x, dy = (t.to(DEV) for t in wgrad_inputs(M, N, K))
        dW, db = _nan(N, K), _nan(N)
        nbytes = _lib.load().rd_linear_bwd_weight_workspace_bytes(M, N, K)
        ws = _nan(max(64, (nbytes + 3) // 4))
        _lib.call("rd_linear_bwd_weight", M, N, K, ops._ptr(dy), N, ops._ptr(x), K, ops._ptr(dW), ops._ptr(db), ops._ptr(ws), ws.numel() * 4,
                  ops._stream())
        torch.cuda.synchronize()
        return {"dW": _np(dW), "db": _np(db)}

    for M, N, K, act in LINEAR_SHAPES:
        yield "linear/fb/M%dN%dK%da%d" % (M, N, K, act), 4 * (M * N + M * K + N * K + N), (lambda a=(M, N, K, act): fwd_bwd(*a))
    for M, N, K in WGRAD_SHAPES:
        yield "linear/wgrad/M%dN%dK%d" % (M, N, K), 4 * (N * K + N), (lambda a=(M, N, K): wgrad(*a))


def probe_sensor_p12():
    from raindrop_amd import _lib, ops

    def run(B, kind, stream):
        cfg, gs, b, p, dz = sensor_inputs(B, kind)
        T, F, d = cfg["max_len"], cfg["d_inp"], 4
        pd = {n: t.detach().to(DEV).requires_grad_(True) for n, t in p.items()}
        adj, _, _ = ops.graph_build(gs.to(DEV))
        _, ssum = ops.edge_softmax_dense(adj)
        shp = _lib.shape(B, T, F, d)
        n = SENSOR_NAMES
        with _env(RD_PANEL_WIDE="0", RD_PANEL_PC="0", **({} if stream else {"RD_K1_WGRAD_STREAM": "0"})):
            z, mask = ops.sensor_stage(b["src"].to(DEV), b["times"].to(DEV), b["lengths"].to(DEV), ops.timescales(T).to(DEV), ssum,
                                       pd[n[0]], pd[n[1]], pd[n[2]], pd[n[3]], pd[n[4]], shp)
            g = torch.autograd.grad(z, [pd[k] for k in n], dz.to(DEV))
            torch.cuda.synchronize()
        out = {"z": _np(z), "mask": _np(mask)}
        out.update({"d:" + k: _np(t) for k, t in zip(n, g)})
        return out

    for B, kind in SENSOR_CASES:
        for stream in (1, 0):
            yield ("sensor_p12/B%d%s/stream%d" % (B, kind, stream), 4 * (215 * B * 160 + 2 * 860 * 861 + 144),
                   (lambda a=(B, kind, stream): run(*a)))


def probe_step():
    def run():
        from raindrop_amd import dp
        from raindrop_amd.step import TrainStep
        from tests.helpers import build_ours
        cfg = synth.make_config("P19")
        gs = synth.make_structure(cfg, "sparse")
        batch = synth.make_batch(cfg, STEP_B, seed=23, min_len=2)
        dv = {k: (None if v is None else v.to(DEV).clone()) for k, v in batch.items()}
        m = build_ours(cfg, gs, DEV, 7).train()                     # dropout p forced to 0 by build_ours
        live = synth.live_parameter_names(cfg)
        named = dict(m.named_parameters())
        flat = dp.FlatGradAllReduce([(n, named[n]) for n in live])
        step = TrainStep(m, flat, dv, use_graph=False, token_plan=True, autotune=False)
        try:
            plan_none = step.plan is None
            step.run()
            torch.cuda.synchronize()
            out = {"loss": np.float64(float(step.loss)), "logits": _np(step.logits).copy(), "plan_none": np.int64(plan_none)}
            out.update({"d:" + n: _np(named[n].grad).copy() for n in live})
            return out
        finally:
            step.close()

    yield "step/P19B%d" % STEP_B, 64 << 20, run


PROBES = {"attn": probe_attn, "enc_rb": probe_enc_rb, "enc_small": probe_enc_small, "linear": probe_linear,
          "sensor_p12": probe_sensor_p12, "step": probe_step}


def item_keys(spec):
    """the item keys `--probes spec` runs, in order (no device needed: the parent sizes its expectations with this)"""
    return [k for k, _, _ in _items(spec)]


def _items(spec):
    for part in spec.split(","):
        name, *filters = part.split("@")
        for key, nbytes, fn in PROBES[name]():
            if not filters or any(f in key for f in filters):
                yield key, nbytes, fn


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--probes", required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    from raindrop_amd import _lib
    lib = _lib.load()
    log_on, log_read = lib.rd_debug_launch_log, lib.rd_debug_launch_log_read
    log_on.argtypes, log_on.restype = [ctypes.c_int], None
    log_read.argtypes, log_read.restype = [ctypes.c_char_p, ctypes.c_size_t], ctypes.c_size_t
    buf = ctypes.create_string_buffer(1 << 16)
    arrays, log, err = {}, {}, {}
    for key, nbytes, fn in _items(args.probes):
        _poison(nbytes)
        log_on(1)
        try:
            outs = fn()
        except Exception as e:                                       # the first failed call ends the run: nothing starts after it
            err[key] = "%s: %s" % (type(e).__name__, e)
            print("switch_child: %s raised %s" % (key, err[key]), flush=True)
            break
        finally:
            need = log_read(buf, len(buf))
            assert need < len(buf), "launch log longer than the read buffer"
            log[key] = sorted(n for n in buf.value.decode().split("\n") if n)
            log_on(0)
        for n, a in outs.items():
            arrays[key + "|" + n] = np.asarray(a)
    np.savez(args.out, __log__=np.array(json.dumps(log)), __err__=np.array(json.dumps(err)), **arrays)
    return 3 if err else 0


if __name__ == "__main__":
    sys.exit(main())
