"""CPU: the route of an encoder layer (csrc/rd_temporal.hip enc_route, read through rd_debug_encoder_route) against a table written
by hand from the conditions the layer's entry points evaluated before the route existed, its invariants over a grid of widths,
and step.plan_supported against plan_ok.

The library loads without a device.  Per-call switches are set with monkeypatch; RD_ROWGEMM, RD_LN_FUSE and RD_LNB_FUSE are read
once per process, so each of their rows runs in a fresh child (tests/encoder_route_child.py, which prints the routes of every
configuration as JSON)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from raindrop_amd import _lib, step, synth
from tests.encoder_route_child import CONFIGS, MODES, all_routes, route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READ_ONCE = ("RD_ROWGEMM=0", "RD_LN_FUSE=0", "RD_LNB_FUSE=0")
PER_CALL = ("RD_ENC_FUSE=0", "RD_ATTN_FUSE=0", "RD_TILE_WGRAD=0", "RD_ATTN_BIG=1", "RD_ENC_LEAN=0", "RD_TILE_WGRAD_GENERIC=0")

# The split-bf16 modes (bf16x3 and bf16 take the same route).  (configuration, switch) -> (fields set without a plan, fields a token
# plan adds).  Exact fp32: FP32 below.  Derivation, per configuration, from the parent's conditions:
#   rowgemm_ok(N, K): bf16 mode, RD_ROWGEMM, all of N, K, lda, ldc multiples of 4, ceil(K / 32) in {5, 9, 15}
#   P19   D 152 / nhid 272 / 3D 456 -> 5 / 9 / 15: rg, dx, tw; D <= 256: lnf1, lnf2; ceil(D / 32) == 5: lnb; (152, 272) is a compiled
#         chain pair: chains; T 60 <= 64, head_dim 76 <= 80 and a multiple of 4: fused attention; the one pair with an inference chain
#   P12   160 / 288 / 480 -> 5 / 9 / 15, compiled pair (160, 288): as P19 but T 215 > 64 (no fused attention), no inference chain
#   RB156 156 / 260 / 468 -> 5 / 9 / 15 but no compiled pair (no chains), head_dim 78 is no multiple of 4 (no fused attention)
#   PAM   D 84 -> ceil 3: tiled family, panel form; D < 256: the split-K weight gradients stay
#   SYN256 D 1040 -> ceil 33: tiled family, panel form; D >= 256 and M >= 1024: tw2; head_dim 520 > 96: big
D19 = "rg dx_rowblock tw lnf1 lnf2 lnb chain_fwd chain_bwd attn_tiles infer plan_ok"
D12 = "rg dx_rowblock tw lnf1 lnf2 lnb chain_fwd chain_bwd plan_ok"
D156 = "rg dx_rowblock tw lnf1 lnf2 lnb plan_ok"
TABLE = {
    # P19 -- tests/test_load_time_switches_gpu.py::test_switch_path[default] (enc_rb 152x272, step);
    #        tests/test_plan_layer_gpu.py::test_plan_layer_vs_float64 (plan)
    ("P19", ""): (D19, "afuse_fwd afuse_bwd lean"),
    # test_load_time_switches_gpu.py::test_switch_path[RD_ROWGEMM=0]
    ("P19", "RD_ROWGEMM=0"): ("panel", ""),
    # test_load_time_switches_gpu.py::test_switch_path[RD_LN_FUSE=0]: no epilogue -> no forward chain, no inference forward, no plan;
    # the backward chain and (afuse_* do not look at lnf1 / lnf2) both fused attention launches stay
    ("P19", "RD_LN_FUSE=0"): ("rg dx_rowblock tw lnb chain_bwd attn_tiles", "afuse_fwd afuse_bwd lean"),
    # test_load_time_switches_gpu.py::test_switch_path[RD_LNB_FUSE=0]: the asymmetry -- afuse_fwd stays, afuse_bwd goes with chain_bwd
    ("P19", "RD_LNB_FUSE=0"): ("rg dx_rowblock tw lnf1 lnf2 chain_fwd attn_tiles infer", "afuse_fwd lean"),
    # tests/test_gpu_parity.py::test_fused_row_local_chains_match_row_block_products (its RD_ENC_FUSE=0 side)
    ("P19", "RD_ENC_FUSE=0"): ("rg dx_rowblock tw lnf1 lnf2 lnb attn_tiles plan_ok", "lean"),
    # tests/test_plan_layer_gpu.py::test_fused_attention_vs_the_launches_it_replaces_on_the_plan (its RD_ATTN_FUSE=0 side)
    ("P19", "RD_ATTN_FUSE=0"): ("rg dx_rowblock tw lnf1 lnf2 lnb chain_fwd chain_bwd infer plan_ok", "lean"),
    # tests/test_gpu_parity.py::test_encoder_tile_weight_gradients_match_split_k (its RD_TILE_WGRAD=0 side): lnb needs tw
    ("P19", "RD_TILE_WGRAD=0"): ("rg dx_rowblock lnf1 lnf2 chain_fwd attn_tiles", ""),
    # tests/test_gpu_parity.py::test_materialised_attention_matches_tiled
    ("P19", "RD_ATTN_BIG=1"): ("rg dx_rowblock tw big lnf1 lnf2 lnb chain_fwd chain_bwd attn_tiles", "afuse_fwd afuse_bwd lean"),
    # tests/test_rowgemm_variants_gpu.py::test_lean_chains_equal_the_chains_with_saved_hidden
    ("P19", "RD_ENC_LEAN=0"): (D19, "afuse_fwd afuse_bwd"),
    # (no panel form at this width: the switch changes nothing)
    ("P19", "RD_TILE_WGRAD_GENERIC=0"): (D19, "afuse_fwd afuse_bwd lean"),
    # P12 -- tests/test_rowgemm_variants_gpu.py::test_row_block_layer_vs_float64[160x288]; test_plan_layer_vs_float64 (plan)
    ("P12", ""): (D12, "lean"),
    ("P12", "RD_ROWGEMM=0"): ("panel", ""),
    ("P12", "RD_LN_FUSE=0"): ("rg dx_rowblock tw lnb chain_bwd", "lean"),
    ("P12", "RD_LNB_FUSE=0"): ("rg dx_rowblock tw lnf1 lnf2 chain_fwd", "lean"),
    ("P12", "RD_ENC_FUSE=0"): ("rg dx_rowblock tw lnf1 lnf2 lnb plan_ok", "lean"),
    ("P12", "RD_ATTN_FUSE=0"): (D12, "lean"),
    ("P12", "RD_TILE_WGRAD=0"): ("rg dx_rowblock lnf1 lnf2 chain_fwd", ""),
    ("P12", "RD_ATTN_BIG=1"): ("rg dx_rowblock tw big lnf1 lnf2 lnb chain_fwd chain_bwd", "lean"),
    ("P12", "RD_ENC_LEAN=0"): (D12, ""),
    ("P12", "RD_TILE_WGRAD_GENERIC=0"): (D12, "lean"),
    # RB156 -- test_load_time_switches_gpu.py::test_switch_path (enc_rb 156x260 under each read-once switch);
    #          tests/test_rowgemm_variants_gpu.py::test_row_block_layer_vs_float64[156x260]
    ("RB156", ""): (D156, "lean"),
    ("RB156", "RD_ROWGEMM=0"): ("panel", ""),
    ("RB156", "RD_LN_FUSE=0"): ("rg dx_rowblock tw lnb", "lean"),
    ("RB156", "RD_LNB_FUSE=0"): ("rg dx_rowblock tw lnf1 lnf2", "lean"),
    ("RB156", "RD_ENC_FUSE=0"): (D156, "lean"),
    ("RB156", "RD_ATTN_FUSE=0"): (D156, "lean"),
    ("RB156", "RD_TILE_WGRAD=0"): ("rg dx_rowblock lnf1 lnf2", ""),
    ("RB156", "RD_ATTN_BIG=1"): ("rg dx_rowblock tw big lnf1 lnf2 lnb", "lean"),
    ("RB156", "RD_ENC_LEAN=0"): (D156, ""),
    ("RB156", "RD_TILE_WGRAD_GENERIC=0"): (D156, "lean"),
    # PAM -- tests/test_gpu_parity.py::test_encoder_layer_vs_oracle, test_switch_path[default] (enc_small F17): only RD_ATTN_BIG moves it
    ("PAM", ""): ("panel", ""),
    ("PAM", "RD_ROWGEMM=0"): ("panel", ""),
    ("PAM", "RD_LN_FUSE=0"): ("panel", ""),
    ("PAM", "RD_LNB_FUSE=0"): ("panel", ""),
    ("PAM", "RD_ENC_FUSE=0"): ("panel", ""),
    ("PAM", "RD_ATTN_FUSE=0"): ("panel", ""),
    ("PAM", "RD_TILE_WGRAD=0"): ("panel", ""),
    ("PAM", "RD_ATTN_BIG=1"): ("panel big", ""),
    ("PAM", "RD_ENC_LEAN=0"): ("panel", ""),
    ("PAM", "RD_TILE_WGRAD_GENERIC=0"): ("panel", ""),
    # SYN256 -- tests/test_gpu_parity.py::test_wide_encoder_tile_weight_gradients_match_split_k (both sides of RD_TILE_WGRAD_GENERIC)
    ("SYN256", ""): ("panel tw2 big", ""),
    ("SYN256", "RD_ROWGEMM=0"): ("panel tw2 big", ""),
    ("SYN256", "RD_LN_FUSE=0"): ("panel tw2 big", ""),
    ("SYN256", "RD_LNB_FUSE=0"): ("panel tw2 big", ""),
    ("SYN256", "RD_ENC_FUSE=0"): ("panel tw2 big", ""),
    ("SYN256", "RD_ATTN_FUSE=0"): ("panel tw2 big", ""),
    ("SYN256", "RD_TILE_WGRAD=0"): ("panel big", ""),
    ("SYN256", "RD_ATTN_BIG=1"): ("panel tw2 big", ""),
    ("SYN256", "RD_ENC_LEAN=0"): ("panel tw2 big", ""),
    ("SYN256", "RD_TILE_WGRAD_GENERIC=0"): ("panel big", ""),
}


def FP32(cfg, switch):
    """Exact fp32: no row-block kernel, no panel form, no tile stream -- only `big` can be set (wide heads, or forced)"""
    return ("big" if cfg == "SYN256" or switch == "RD_ATTN_BIG=1" else ""), ""


def _check(switch, got):
    bad = []
    for cfg in CONFIGS:
        for mode in MODES:
            base, extra = FP32(cfg, switch) if mode == 0 else TABLE[(cfg, switch)]
            for plan in (0, 1):
                want = sorted(set(base.split()) | (set(extra.split()) if plan else set()))
                have = got["%s/%d/%d" % (cfg, mode, plan)]
                if have != want:
                    bad.append((cfg, MODES[mode], "plan" if plan else "padded", "want", want, "got", have))
    assert not bad, (switch, bad)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for sw in READ_ONCE + PER_CALL:
        monkeypatch.delenv(sw.split("=")[0], raising=False)
    monkeypatch.delenv("RD_ENC_SPECIALIZE", raising=False)
    yield
    _lib.call("rd_set_precision", 1)


def test_table_is_complete():
    assert set(TABLE) == {(c, s) for c in CONFIGS for s in ("",) + READ_ONCE + PER_CALL}
    assert all(set((a + " " + b).split()) <= set(_lib.ROUTE_BITS) for a, b in TABLE.values())
    for name in ("P19", "P12", "PAM", "SYN256"):
        cfg = synth.make_config(name)
        B, T, F, nhid = CONFIGS[name]
        assert (T, F, nhid) == (cfg["max_len"], cfg["d_inp"], cfg["nhid"]), name


@pytest.mark.parametrize("switch", ("",) + PER_CALL, ids=lambda s: s or "default")
def test_route_table_per_call_switches(switch, monkeypatch):
    if switch:
        monkeypatch.setenv(*switch.split("="))
    _check(switch, all_routes())


@pytest.mark.parametrize("switch", READ_ONCE)
def test_route_table_read_once_switches(switch):
    env = {k: v for k, v in os.environ.items() if k.split("=")[0] not in {s.split("=")[0] for s in READ_ONCE + PER_CALL}}
    env[switch.split("=")[0]] = switch.split("=")[1]
    env["CUDA_VISIBLE_DEVICES"] = env["HIP_VISIBLE_DEVICES"] = ""           # a CPU child
    res = subprocess.run([sys.executable, "-m", "tests.encoder_route_child"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    _check(switch, json.loads(res.stdout.strip().splitlines()[-1]))


GRID_F = list(range(1, 65)) + [256]
GRID_T = (7, 60, 64, 65, 215)


def _covers(name, shp, second):
    a, b = ctypes.c_int32(-1), ctypes.c_int32(-1)
    _lib.call(name, ctypes.byref(shp), ctypes.byref(a), ctypes.byref(b))
    return (b if second else a).value


@pytest.mark.parametrize("mode", sorted(MODES), ids=[MODES[m] for m in sorted(MODES)])
def test_route_invariants_and_plan_supported(mode):
    lib = _lib.load()
    _lib.call("rd_set_precision", mode)
    disagree = []
    for F in GRID_F:
        for T in GRID_T:
            B, nhid, D = 3, 8 * F, 4 * F + 16
            shp = _lib.shape(B, T, F, 4, nhead=2, nhid=nhid)
            for plan in (False, True):
                r = route(B, T, F, nhid, plan)
                tag = (F, T, plan, sorted(r))
                if "chain_fwd" in r:
                    assert {"lnf1", "lnf2", "rg"} <= r, tag
                if "chain_bwd" in r:
                    assert {"lnb", "tw"} <= r, tag
                if r & {"afuse_fwd", "afuse_bwd"}:
                    assert plan, tag
                if "infer" in r:
                    assert "tw" in r and "big" not in r, tag
                if "lean" in r:
                    assert plan and "tw" in r, tag
                if "plan_ok" in r:
                    assert ("afuse_fwd" in r) == ("afuse_bwd" in r), tag
                assert _covers("rd_step_prepare_covers", shp, False) == ("rg" in r), tag
                assert _covers("rd_infer_covers", shp, True) == ("infer" in r), tag
                small = lib.rd_encoder_layer_infer_bytes(ctypes.byref(shp)) < lib.rd_encoder_layer_saved_bytes(ctypes.byref(shp))
                assert small == ("infer" in r), tag
                # plan_supported -> plan_ok, but for the widths tests/test_plan_layer_gpu.py pins as refused (ceil(3 D / 32) != 15)
                if step.plan_supported(F, 4, T, D, 2, nhid, mode) and (3 * D + 31) // 32 == 15 and "plan_ok" not in r:
                    disagree.append(tag)
    assert not disagree, disagree

