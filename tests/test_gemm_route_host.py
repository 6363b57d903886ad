"""CPU: the route of a launch_gemm call (csrc/rd_gemm.hip gemm_check + gemm_route, read through rd_debug_gemm_route) against a table
written by hand from the conditions the six functions of the parent evaluated (launch_gemm, panel_ok, panel_form, dispatch_bf16x3,
launch_bf16x3, launch_bf16x3_n), against an independent restatement of the two cost models over a grid, under every switch, and for
every error of gemm_check.  The library loads without a device.  RD_PANEL_WIDE / RD_PANEL_PC are read per call (monkeypatch);
RD_GEMM_NPRE, RD_GEMM_PANEL, RD_GEMM_XCD, RD_SPLITK_XCD, RD_PANEL_WIDE_COST and RD_PANEL_PC_COST once per process (a child process:
`python -m tests.test_gemm_route_host`).  The one GPU test at the end ties the query's name to the launch log.

The conditions, as the parent had them (modes: fp32 = 0, bf16x3 = 1, bf16 = 2; nsplit, pair = max(nsplit, 1), 2 with a second problem):
  layout    akc = sa_k == 1 and not (row sums and sa_m == 1); bkc = sb_k == 1
  family    fp32 mode: k_gemm, grid (ceil N/64, ceil M/64, batches or nsplit).  Else panel if RD_GEMM_PANEL != 0, weight tiles given,
            sa_k == 1, sa_m % 4 == 0, A on a 16-byte boundary, nsplit <= 1, not batched, no second problem, no row sums, K >= 64;
            else k_gemm_bf16x3
  panel     rounds(tm, tn) = ceil(ceil(M/tm) ceil(N/tn) / 256); small 64x128 costs 100 rounds, wide 128x256 280 (RD_PANEL_WIDE_COST),
            pc 128x128 180 (RD_PANEL_PC_COST); wide, then pc, replaces the best so far if strictly cheaper, small counting 0.95 of
            its cost; RD_PANEL_WIDE / RD_PANEL_PC = 0 excludes, = 1 forces (pc before wide).  grid 8 ceil(tiles / 8);
            LDS planes tm 80 2 + 4 tn with 8 planes (small) or 4
  tile      tile_hint == 1: 128x128.  Else the first cheapest of 64x64, 128x64, 128x128, 64x128, 64x160 (bkc only):
            cost = padded M N (1 + 16/tm + 16/tn), x 4 if bigger than 64x64 with blocks = tiles nsplit < 2048, x 192 / blocks if
            blocks < 192.  (The last term never decides: below 2048 blocks every bigger tile is already four times dearer and has
            fewer blocks than 64x64.  Restated anyway.)
  npre      64x64, RD_GEMM_NPRE != 0, ceil(M/64) ceil(N/64) nsplit pair <= 128 and (nsplit > 1 ? k_per_split : K) <= 256
  map       split-K: slice per XCD, grid 8 ceil(nsplit pair / 8) tiles -- or "_zgrid" (RD_SPLITK_XCD=0), grid (ceil(M/tm) ceil(N/tn),
            1, nsplit pair); single pass: XCD round-robin or "_rowmajor" (RD_GEMM_XCD=0), grid 8 ceil(ceil(M/tm) / 8) ceil(N/tn), z =
            batches or pair
  LDS       max(2 (tm + tn) 80 2, tm (tn + 4) 4) + 4 tn
No two of the parent's conditions were found to disagree."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from raindrop_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32, BF16X3, BF16 = 0, 1, 2
MODES = {FP32: "fp32", BF16X3: "bf16x3", BF16: "bf16"}
X3 = "k_gemm_bf16x3_"
TILES = {"64x64": (64, 64), "128x64": (128, 64), "128x128": (128, 128), "64x128": (64, 128), "64x160": (64, 160)}
PANEL = {"small": (64, 128, 8), "wide": (128, 256, 4), "pc": (128, 128, 4)}
PANEL_NAME = {"small": "k_gemm_panel", "wide": "k_gemm_panel_wide", "pc": "k_gemm_panel_pc"}
READ_ONCE = ("RD_GEMM_NPRE", "RD_GEMM_PANEL", "RD_GEMM_XCD", "RD_SPLITK_XCD", "RD_PANEL_WIDE_COST", "RD_PANEL_PC_COST")
PER_CALL = ("RD_PANEL_WIDE", "RD_PANEL_PC")
FLAG = {n: 1 << i for i, n in enumerate(_lib.GEMM_ROUTE_FLAGS)}


def cdiv(a, b):
    return -(-a // b)


def product(M, N, K, sa=None, sb=None, nsplit=0, kps=0, hint=0, flags=("a_aligned",)):
    """a product by value; sa / sb: (row stride, k stride) of A / B, default both k-contiguous and dense"""
    return dict(M=M, N=N, K=K, sa=sa or (K, 1), sb=sb or (K, 1), nsplit=nsplit, kps=kps, hint=hint, flags=tuple(flags))


def fwd(M, N, K, ldx=None, **kw):              # rd_linear_fwd: y[M, N] = x[M, K] W[N, K]^T
    return product(M, N, K, sa=(ldx or K, 1), **kw)


def dgrad(M, Nout, Kin, lddy=None):            # rd_linear_bwd_input: dx[M, Kin] = dy[M, Nout] W[Nout, Kin]
    return product(M, Kin, Nout, sa=(lddy or Nout, 1), sb=(1, Kin))


def splitk(red, rows, cols):
    kps = ctypes.c_int32(0)
    return _lib.load().rd_debug_splitk_plan(red, rows, cols, ctypes.byref(kps)), kps.value


def wgrad(M, Nout, Kin, lddy=None, ldx=None, second=False):    # rd_linear_bwd_weight: dW[Nout, Kin] = dy[M, Nout]^T x[M, Kin], db on the side
    ns, kps = splitk(M, Nout, Kin)
    return product(Nout, Kin, M, sa=(1, lddy or Nout), sb=(1, ldx or Kin), nsplit=ns, kps=kps,
                   flags=("a_aligned", "rowsum") + (("second",) if second else ()))


def query(p):
    """-> (rc, route): name, grid, lds and the fields of words[0]"""
    words, name = (ctypes.c_uint32 * 5)(), ctypes.create_string_buffer(64)
    rc = _lib.load().rd_debug_gemm_route(p["M"], p["N"], p["K"], p["sa"][0], p["sa"][1], p["sb"][0], p["sb"][1], p["nsplit"], p["kps"],
                                         p["hint"], sum(FLAG[f] for f in p["flags"]), words, name, len(name))
    w = words[0]
    return rc, dict(name=name.value.decode(), grid=tuple(words[1:4]), lds=words[4], family=_lib.GEMM_FAMILIES[w & 3], akc=w >> 2 & 1,
                    bkc=w >> 3 & 1, one_product=w >> 4 & 1, map=_lib.GEMM_MAPS[w >> 5 & 3], npre=w >> 8 & 15, tile=w >> 12 & 15)


def route(p):
    rc, r = query(p)
    assert rc == 0, (p, _lib.load().rd_last_error())
    return r


# ---- the independent restatement ---------------------------------------------------------------------------------------------------
def restate(p, mode, env=None):
    """(name, grid, lds) by the docstring's rules; env: the switches that are set"""
    env = env or {}
    on = lambda k: int(env.get(k, 1)) != 0                                   # noqa: E731
    M, N, K, fl = p["M"], p["N"], p["K"], set(p["flags"])
    ns, pair = max(p["nsplit"], 1), 2 if "second" in fl else 1
    bkc = p["sb"][1] == 1
    if mode == FP32:
        return "k_gemm", (cdiv(N, 64), cdiv(M, 64), 2 if "batched" in fl else ns), 0
    if (on("RD_GEMM_PANEL") and "btiles" in fl and p["sa"][1] == 1 and p["sa"][0] % 4 == 0 and "a_aligned" in fl and ns == 1
            and not fl & {"batched", "second", "rowsum"} and K >= 64):
        cost = {"small": 100, "wide": int(env.get("RD_PANEL_WIDE_COST", 280)), "pc": int(env.get("RD_PANEL_PC_COST", 180))}
        price = {f: cdiv(cdiv(M, tm) * cdiv(N, tn), 256) * cost[f] for f, (tm, tn, _) in PANEL.items()}
        force = {"wide": int(env.get("RD_PANEL_WIDE", -1)), "pc": int(env.get("RD_PANEL_PC", -1))}
        best, bc = "small", price["small"] * 0.95
        for f in ("wide", "pc"):
            if force[f] != 0 and price[f] < bc:
                best, bc = f, price[f]
        for f in ("wide", "pc"):
            if force[f] == 1:
                best = f
        tm, tn, planes = PANEL[best]
        return (PANEL_NAME[best] + ("" if on("RD_GEMM_XCD") else "_rowmajor"), (8 * cdiv(cdiv(M, tm) * cdiv(N, tn), 8), 1, 1),
                planes * tm * 80 * 2 + 4 * tn)
    best, bcost = "128x128", None
    for t, (tm, tn) in (() if p["hint"] == 1 else TILES.items()):
        if tn == 160 and not bkc:
            continue
        blocks = cdiv(M, tm) * cdiv(N, tn) * ns
        c = float(cdiv(M, tm) * tm) * (cdiv(N, tn) * tn) * (1.0 + 16.0 / tm + 16.0 / tn)
        if blocks < 2048 and (tm, tn) != (64, 64):
            c *= 4.0
        if blocks < 192:
            c *= 192.0 / blocks
        if bcost is None or c < bcost:
            best, bcost = t, c
    tm, tn = TILES[best]
    npre = (best == "64x64" and on("RD_GEMM_NPRE") and cdiv(M, 64) * cdiv(N, 64) * ns * pair <= 128
            and (p["kps"] if ns > 1 else K) <= 256)
    nz = 2 if "batched" in fl else ns * pair
    if ns > 1:
        sfx, grid = ("", (8 * cdiv(nz, 8) * cdiv(M, tm) * cdiv(N, tn), 1, 1)) if on("RD_SPLITK_XCD") else ("_zgrid", (cdiv(M, tm) * cdiv(N, tn), 1, nz))
    else:
        sfx, grid = "" if on("RD_GEMM_XCD") else "_rowmajor", (8 * cdiv(cdiv(M, tm), 8) * cdiv(N, tn), 1, nz)
    return X3 + best + ("_npre" if npre else "") + sfx, grid, max(2 * (tm + tn) * 80 * 2, tm * (tn + 4) * 4) + 4 * tn


# ---- the hand table: id -> (product, name in the bf16 modes, grid, LDS bytes).  fp32: always k_gemm, no LDS -------------------------
L64, L128x64, L128, L64x128, L64x160 = 41216, 61696, 82432, 61952, 72320          # max(planes, stage) + bias, worked out per tile
BT = ("a_aligned", "btiles")
P12 = dict(M=9216, N=860, K=860)               # sensor stage at P12, B = 256: [B F, T d_ob] x [T d_ob, T d_ob]
TABLE = {
    # all-K-up-front form: blocks <= 128 | 129 ..., kspan <= 256 | 257
    "npre/7x5x3": (fwd(7, 5, 3), X3 + "64x64_npre", (8, 1, 1), L64),
    "npre/blocks128": (fwd(512, 1024, 256), X3 + "64x64_npre", (128, 1, 1), L64),
    "npre/blocks144": (fwd(513, 1024, 256), X3 + "64x64", (256, 1, 1), L64),
    "npre/blocks136": (fwd(512, 1025, 256), X3 + "64x64", (136, 1, 1), L64),
    "npre/K257": (fwd(512, 1024, 257), X3 + "64x64", (128, 1, 1), L64),
    # ... under split-K: 64 x 64 outputs, nsplit slices of k_per_split; and with a second problem
    "npre/splitk128": (product(64, 64, 128 * 64, sa=(1, 64), sb=(1, 64), nsplit=128, kps=64), X3 + "64x64_npre", (128, 1, 1), L64),
    "npre/splitk129": (product(64, 64, 129 * 64, sa=(1, 64), sb=(1, 64), nsplit=129, kps=64), X3 + "64x64", (136, 1, 1), L64),
    "npre/splitk-kps256": (product(64, 64, 1024, sa=(1, 64), sb=(1, 64), nsplit=4, kps=256), X3 + "64x64_npre", (8, 1, 1), L64),
    "npre/splitk-kps320": (product(64, 64, 1280, sa=(1, 64), sb=(1, 64), nsplit=4, kps=320), X3 + "64x64", (8, 1, 1), L64),
    "npre/pair64": (product(64, 64, 4096, sa=(1, 64), sb=(1, 64), nsplit=64, kps=64, flags=("a_aligned", "second")), X3 + "64x64_npre", (128, 1, 1), L64),
    "npre/pair65": (product(64, 64, 4160, sa=(1, 64), sb=(1, 64), nsplit=65, kps=64, flags=("a_aligned", "second")), X3 + "64x64", (136, 1, 1), L64),
    # tile cost model: 2048 blocks of 128 x 64 | 2016; 64 x 160 with a k-contiguous B only; the hint
    "tile/2048blocks": (fwd(8189, 2043, 72), X3 + "128x64", (2048, 1, 1), L128x64),
    "tile/2016blocks": (fwd(8061, 2043, 72), X3 + "64x64", (128 * 32, 1, 1), L64),
    "tile/64x160": (fwd(4093, 5115, 72), X3 + "64x160", (64 * 32, 1, 1), L64x160),
    "tile/no-64x160": (dgrad(4093, 72, 5115), X3 + "128x64", (32 * 80, 1, 1), L128x64),
    "tile/hint": (product(64, 48, 1025, sa=(1, 64), sb=(1, 48), nsplit=17, kps=64, hint=1, flags=("a_aligned", "rowsum")), X3 + "128x128", (24, 1, 1), L128),
    "tile/batched": (product(40, 40, 16, flags=("a_aligned", "batched")), X3 + "64x64_npre", (8, 1, 2), L64),
    # panel_ok, each clause on its own (the base case first)
    "panel/P12": (product(**P12, flags=BT), "k_gemm_panel_pc", (504, 1, 1), 82432),
    "panel/K64": (product(9216, 860, 64, sa=(64, 1), flags=BT), "k_gemm_panel_pc", (504, 1, 1), 82432),
    "panel/K63": (product(9216, 860, 63, sa=(64, 1), flags=BT), X3 + "64x64", (144 * 14, 1, 1), L64),
    "panel/sa_m%4": (product(**P12, sa=(862, 1), flags=BT), X3 + "64x64", (144 * 14, 1, 1), L64),
    "panel/unaligned": (product(**P12, flags=("btiles",)), X3 + "64x64", (144 * 14, 1, 1), L64),
    "panel/no-tiles": (product(**P12), X3 + "64x64", (144 * 14, 1, 1), L64),
    "panel/nsplit": (product(**P12, nsplit=2, kps=448, flags=BT), X3 + "64x64", (8 * 144 * 14, 1, 1), L64),
    "panel/batched": (product(**P12, flags=BT + ("batched",)), X3 + "64x64", (144 * 14, 1, 2), L64),
    "panel/second": (product(**P12, flags=BT + ("second",)), X3 + "64x64", (144 * 14, 1, 2), L64),
    "panel/rowsum": (product(**P12, flags=BT + ("rowsum",)), X3 + "64x64", (144 * 14, 1, 1), L64),
    # panel_form.  PAM (1088 x 2400): small 323 tiles = 2 rounds (200), wide 90 = 1 (280), pc 171 = 1 (180 < 190).  SYN256 (4096 x 2048):
    # small 1024 = 4 (400), wide 256 = 1 (280 < 380), pc 512 = 2 (360).  17 x 528 small tiles = 36 rounds (3600 -> 3420), pc 9 x 528 = 19
    # rounds (3420: a tie, not taken), wide 9 x 264 = 10 rounds (2800); 16 x 561 small tiles = 36 rounds, pc 8 x 561 = 18 (3240)
    "form/PAM": (product(1088, 2400, 2400, flags=BT), "k_gemm_panel_pc", (176, 1, 1), 82432),
    "form/SYN256": (product(4096, 2048, 2048, flags=BT), "k_gemm_panel_wide", (256, 1, 1), 82944),
    "form/tie-wide": (product(1088, 67584, 64, flags=BT), "k_gemm_panel_wide", (2376, 1, 1), 82944),
    "form/small": (product(64, 128, 64, flags=BT), "k_gemm_panel", (8, 1, 1), 82432),
}
# the same under RD_PANEL_WIDE / RD_PANEL_PC (read per call)
FORCED = {
    ("form/tie-wide", "RD_PANEL_WIDE=0"): ("k_gemm_panel", (8976, 1, 1), 82432),                  # the 5 % rule at the tie: small stays
    ("form/SYN256", "RD_PANEL_WIDE=0"): ("k_gemm_panel_pc", (512, 1, 1), 82432),                  # 360 < 380
    ("panel/P12", "RD_PANEL_PC=0"): ("k_gemm_panel", (1008, 1, 1), 82432),                        # wide 560 >= 380
    ("panel/P12", "RD_PANEL_WIDE=1"): ("k_gemm_panel_wide", (288, 1, 1), 82944),
    ("panel/P12", "RD_PANEL_WIDE=1 RD_PANEL_PC=1"): ("k_gemm_panel_pc", (504, 1, 1), 82432),
    ("form/small", "RD_PANEL_PC=1"): ("k_gemm_panel_pc", (8, 1, 1), 82432),
    ("panel/K63", "RD_PANEL_PC=1"): (X3 + "64x64", (144 * 14, 1, 1), L64),                        # no panel, nothing to force
}
TIE_PC = product(1024, 71808, 64, flags=BT)    # 16 x 561 small tiles: pc is strictly cheaper


def _tile_test_products():
    """the shapes of tests/test_gemm_tiles_gpu.py with the tile that test asserts in the launch log (None: fp32)"""
    from tests import test_gemm_tiles_gpu as G
    for case, tile, M, N, layout, act, ldy, mode in G.FWD:
        K, ldx, off = G.LAYOUTS[layout]
        yield "fwd/" + case, product(M, N, K, sa=(ldx, 1), flags=() if off else ("a_aligned",)), tile, mode
    for case, tile, M, Kin, layout, gated, mode in G.DGRAD:
        Nout, lddy, off = G.LAYOUTS[layout]
        yield "dgrad/" + case, product(M, Kin, Nout, sa=(lddy, 1), sb=(1, Kin), flags=() if off else ("a_aligned",)), tile, mode
    for case, tile, M, Nout, Kin, want, slices, lddy, ldx, mode in G.WGRAD:
        try:
            _lib.load().rd_debug_set_splitk_want(want)
            p = wgrad(M, Nout, Kin, lddy, ldx)
        finally:
            _lib.load().rd_debug_set_splitk_want(0)
        assert max(p["nsplit"], 1) == slices, case
        yield "wgrad/" + case, p, tile, mode


def _model_products(name, B):
    """the dense products of the sensor stage and one encoder layer of a configuration, forward and input gradients"""
    cfg = synth.make_config(name)
    T, F, D, H = cfg["max_len"], cfg["d_inp"], cfg["d_model"], cfg["nhid"]
    Ks = 4 * T
    yield "sensor", product(B * F, Ks, Ks, flags=BT)
    yield "sensor-dx", product(B * F, Ks, Ks, flags=BT)
    for tag, n, k in (("in_proj", 3 * D, D), ("out_proj", D, D), ("linear1", H, D), ("linear2", D, H)):
        yield tag, product(T * B, n, k, flags=BT)
        yield tag + "-dx", dgrad(T * B, n, k)
        yield tag + "-dw", wgrad(T * B, n, k)


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    for k in READ_ONCE + PER_CALL:
        monkeypatch.delenv(k, raising=False)
    yield
    _lib.call("rd_set_precision", BF16X3)


def _setenv(monkeypatch, switch):
    env = dict(kv.split("=") for kv in switch.split())
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return env


@pytest.mark.parametrize("mode", sorted(MODES), ids=[MODES[m] for m in sorted(MODES)])
def test_hand_table(mode):
    _lib.call("rd_set_precision", mode)
    bad = []
    for case, (p, name, grid, lds) in TABLE.items():
        r = route(p)
        if mode == FP32:
            want = ("k_gemm", (cdiv(p["N"], 64), cdiv(p["M"], 64), 2 if "batched" in p["flags"] else max(p["nsplit"], 1)), 0)
        else:
            want = (name, grid, lds)
        if (r["name"], r["grid"], r["lds"]) != want:
            bad.append((case, want, (r["name"], r["grid"], r["lds"])))
        assert restate(p, mode) == want, case                 # the restatement is held to the hand table too
    assert not bad, (MODES[mode], bad)


@pytest.mark.parametrize("mode", (BF16X3, BF16), ids=["bf16x3", "bf16"])
def test_forced_panel_forms(mode, monkeypatch):
    _lib.call("rd_set_precision", mode)
    for (case, switch), want in FORCED.items():
        with monkeypatch.context() as m:
            env = _setenv(m, switch)
            r = route(TABLE[case][0])
            assert (r["name"], r["grid"], r["lds"]) == want == restate(TABLE[case][0], mode, env), (case, switch)
    with monkeypatch.context() as m:                          # one round fewer than the tie: pc is taken (wide, 9 rounds = 2520, excluded)
        m.setenv("RD_PANEL_WIDE", "0")
        assert route(TIE_PC)["name"] == "k_gemm_panel_pc"


def test_tile_test_shapes_take_the_tiles_that_test_asserts():
    n = 0
    for case, p, tile, mode in _tile_test_products():
        _lib.call("rd_set_precision", mode)
        r = route(p)
        assert r["name"] == ("k_gemm" if mode == FP32 else X3 + tile), (case, r)
        assert restate(p, mode)[0] == r["name"], case
        n += 1
    assert n >= 29


def test_switch_test_rows():
    """the names tests/test_load_time_switches_gpu.py asserts for its linear/ and sensor_p12/ rows in the default case"""
    from tests import switch_child as C
    _lib.call("rd_set_precision", BF16X3)
    for M, N, K, act in C.LINEAR_SHAPES:
        name = route(fwd(M, N, K))["name"]
        assert name in (X3 + "64x64", X3 + "64x64_npre"), (M, N, K)
        if M in (7, 64):
            assert name == X3 + "64x64_npre" and route(dgrad(M, N, K))["name"] == name and route(wgrad(M, N, K))["name"] == name
    for M, N, K in C.WGRAD_SHAPES:
        assert route(wgrad(M, N, K))["name"] in (X3 + "64x64", X3 + "64x64_npre"), (M, N, K)
    assert route(wgrad(1025, 64, 48))["name"] == X3 + "64x64_npre"
    for B, _ in C.SENSOR_CASES:                               # the child forces RD_PANEL_WIDE = RD_PANEL_PC = 0
        assert route(product(B * 36, 860, 860, flags=BT))["name"] in PANEL_NAME.values()


@pytest.mark.parametrize("mode", sorted(MODES), ids=[MODES[m] for m in sorted(MODES)])
def test_model_products_follow_the_restatement(mode):
    _lib.call("rd_set_precision", mode)
    for cfg, B in (("P12", 256), ("PAM", 64), ("SYN256", 16)):
        for tag, p in _model_products(cfg, B):
            r = route(p)
            assert (r["name"], r["grid"], r["lds"]) == restate(p, mode), (cfg, tag)
    if mode != FP32:
        forms = {c: route(next(_model_products(c, B))[1])["name"] for c, B in (("P12", 256), ("PAM", 64), ("SYN256", 16))}
        assert forms == {"P12": "k_gemm_panel_pc", "PAM": "k_gemm_panel_pc", "SYN256": "k_gemm_panel_wide"}


GRID_MN = (1, 63, 64, 65, 127, 129, 191, 257, 513, 1000, 1025, 2043, 4093, 4157, 5115, 8061, 8125, 8189)
GRID_K = (3, 63, 64, 256, 257, 860)


def _grid(mode, env=None):
    """a few thousand products: every (M, N, K) of the grid as a forward, an input gradient, a panel candidate and a split-K pair"""
    bad, n = [], 0
    for M in GRID_MN:
        for N in GRID_MN:
            for K in GRID_K:
                ps = [fwd(M, N, K), dgrad(M, K, N), product(M, N, K, sa=(K + (-K) % 4, 1), flags=BT)]
                if K == 256:
                    ps.append(product(M, N, 4 * K, sa=(1, M), sb=(1, N), nsplit=4, kps=K, flags=("a_aligned", "rowsum", "second")))
                for p in ps:
                    r = route(p)
                    n += 1
                    if (r["name"], r["grid"], r["lds"]) != restate(p, mode, env):
                        bad.append((p, r, restate(p, mode, env)))
    return n, bad


@pytest.mark.parametrize("mode", sorted(MODES), ids=[MODES[m] for m in sorted(MODES)])
def test_restatement_over_a_grid(mode):
    _lib.call("rd_set_precision", mode)
    n, bad = _grid(mode)
    assert n > 5000 and not bad, (n, bad[:5])


def test_words_agree_with_the_name():
    for mode in MODES:
        _lib.call("rd_set_precision", mode)
        for case, (p, _, _, _) in TABLE.items():
            r = route(p)
            assert r["one_product"] == (mode == BF16), case
            assert r["akc"] == (p["sa"][1] == 1 and not ("rowsum" in p["flags"] and p["sa"][0] == 1)) and r["bkc"] == (p["sb"][1] == 1), case
            if r["family"] == "fp32":
                assert r["name"] == "k_gemm" and mode == FP32
                continue
            if r["family"] == "panel":
                stem = PANEL_NAME[_lib.GEMM_PANEL_FORMS[r["tile"]]]
            else:
                stem = X3 + _lib.GEMM_TILES[r["tile"]] + ("_npre" if r["npre"] else "")
                assert r["npre"] in (0, 4) and (not r["npre"] or r["tile"] == 0), case
            assert r["name"] == stem + {"xcd": "", "slice_xcd": "", "rowmajor": "_rowmajor", "zgrid": "_zgrid"}[r["map"]], (case, r)
            assert (r["map"] in ("slice_xcd", "zgrid")) == (p["nsplit"] > 1), case


def test_nothing_to_launch():
    rc, r = query(fwd(0, 5, 3))
    assert rc == 0 and r["name"] == "" and r["family"] is None and r["grid"] == (0, 0, 0)


# ---- errors: gemm_check's, with the code and message of the launch, in its order of precedence -----------------------------------------
ERRORS = [
    ("A stride", product(8, 8, 8, sa=(2, 2)), (-1, -1), "A needs a unit stride"),
    ("A stride/rowsum", product(8, 8, 8, sa=(1, 1), sb=(8, 1), flags=("rowsum",)), (0, 0), None),      # 1-wide operand: row-contiguous, fine
    ("B stride", product(8, 8, 8, sb=(2, 2)), (-1, -1), "B needs a unit stride"),
    ("A before B", product(8, 8, 8, sa=(2, 2), sb=(2, 2)), (-1, -1), "A needs a unit stride"),
    ("batched+split", product(8, 8, 128, nsplit=2, kps=64, flags=("batched",)), (-1, -1), "batched form"),
    ("batched+second", product(8, 8, 8, flags=("batched", "second")), (-1, -1), "batched form"),
    ("batched+rowsum", product(8, 8, 8, flags=("batched", "rowsum")), (-1, -1), "batched form"),
    ("batched+scatter", product(8, 8, 8, flags=("batched", "scatter")), (-1, -1), "batched form"),
    ("B before batched", product(8, 8, 8, sb=(2, 2), flags=("batched", "second")), (-1, -1), "B needs a unit stride"),
    ("plan without scatter", product(8, 8, 8, flags=("plan",)), (-2, -2), "plan-following scatter"),
    ("plan, N % 4", product(8, 6, 8, flags=("plan", "scatter")), (-2, -2), "plan-following scatter"),
    ("plan", product(8, 8, 8, flags=("plan", "scatter")), (-2, 0), "plan-following scatter"),          # a bf16 mode only
    ("batched before plan", product(8, 8, 8, flags=("batched", "scatter", "plan")), (-1, -1), "batched form"),
    ("k_per_split", product(8, 8, 200, nsplit=2, kps=100), (0, -1), "k_per_split must be a multiple of 64"),     # not in fp32
    ("plan before k_per_split", product(8, 8, 200, nsplit=2, kps=100, flags=("plan", "scatter")), (-2, -2), "plan-following scatter"),
]


@pytest.mark.parametrize("case,p,codes,msg", ERRORS, ids=[e[0] for e in ERRORS])
def test_errors(case, p, codes, msg):
    for mode, want in ((FP32, codes[0]), (BF16X3, codes[1]), (BF16, codes[1])):
        _lib.call("rd_set_precision", mode)
        rc, r = query(p)
        assert rc == want, (case, MODES[mode], rc)
        if rc:
            assert msg in _lib.load().rd_last_error().decode() and r["name"] == "", case
        else:
            assert r["name"], case


# ---- the switches read once per process: a child --------------------------------------------------------------------------------------
CHILD_SWITCHES = ("", "RD_GEMM_NPRE=0", "RD_GEMM_PANEL=0", "RD_GEMM_XCD=0", "RD_SPLITK_XCD=0", "RD_GEMM_XCD=0 RD_SPLITK_XCD=0",
                  "RD_PANEL_WIDE_COST=150", "RD_PANEL_PC_COST=400")
# by hand, bf16 modes: (7x5x3 forward, its split-K weight gradient (1025, 64, 48), the P12 panel, SYN256's panel)
CHILD_NAMES = {
    "": (X3 + "64x64_npre", X3 + "64x64_npre", "k_gemm_panel_pc", "k_gemm_panel_wide"),
    "RD_GEMM_NPRE=0": (X3 + "64x64", X3 + "64x64", "k_gemm_panel_pc", "k_gemm_panel_wide"),
    "RD_GEMM_PANEL=0": (X3 + "64x64_npre", X3 + "64x64_npre", X3 + "64x64", X3 + "64x64"),
    "RD_GEMM_XCD=0": (X3 + "64x64_npre_rowmajor", X3 + "64x64_npre", "k_gemm_panel_pc_rowmajor", "k_gemm_panel_wide_rowmajor"),
    "RD_SPLITK_XCD=0": (X3 + "64x64_npre", X3 + "64x64_npre_zgrid", "k_gemm_panel_pc", "k_gemm_panel_wide"),
    "RD_GEMM_XCD=0 RD_SPLITK_XCD=0": (X3 + "64x64_npre_rowmajor", X3 + "64x64_npre_zgrid", "k_gemm_panel_pc_rowmajor", "k_gemm_panel_wide_rowmajor"),
    "RD_PANEL_WIDE_COST=150": (X3 + "64x64_npre", X3 + "64x64_npre", "k_gemm_panel_wide", "k_gemm_panel_wide"),      # P12: 2 x 150 < 360
    "RD_PANEL_PC_COST=400": (X3 + "64x64_npre", X3 + "64x64_npre", "k_gemm_panel", "k_gemm_panel_wide"),          # P12: 560, 800 >= 380
}


def _child_report(env):
    out = {}
    for mode in MODES:
        _lib.call("rd_set_precision", mode)
        four = [route(p)["name"] for p in (fwd(7, 5, 3), wgrad(1025, 64, 48), TABLE["panel/P12"][0], TABLE["form/SYN256"][0])]
        n, bad = _grid(mode, env)
        out[MODES[mode]] = {"names": four, "grid": n, "bad": [repr(b) for b in bad[:3]]}
    return out


@pytest.mark.parametrize("switch", CHILD_SWITCHES, ids=lambda s: s.replace(" ", ",") or "default")
def test_read_once_switches_in_a_child(switch):
    env = {k: v for k, v in os.environ.items() if k not in READ_ONCE + PER_CALL}
    env.update(kv.split("=") for kv in switch.split())
    env["CUDA_VISIBLE_DEVICES"] = env["HIP_VISIBLE_DEVICES"] = ""           # a CPU child
    res = subprocess.run([sys.executable, "-m", "tests.test_gemm_route_host", switch], cwd=ROOT, env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    rep = json.loads(res.stdout.strip().splitlines()[-1])
    for mode, r in rep.items():
        assert r["grid"] > 5000 and not r["bad"], (switch, mode, r["bad"])
        assert tuple(r["names"]) == (("k_gemm",) * 4 if mode == "fp32" else CHILD_NAMES[switch]), (switch, mode, r["names"])


# ---- GPU: the name the query gives is the one GEMM name in the launch log ------------------------------------------------------------
# rd_linear_fwd at (M, N, K): 7x5x3; M = 64 | 65; K = 256 | 257 at 8 x 16 = 128 workgroups (and 129 rows: 3 x 16); one split-K weight
# gradient at M = 1025
GPU_FWD = [(7, 5, 3), (64, 40, 32), (65, 40, 32), (512, 1024, 256), (512, 1024, 257), (129, 1024, 256)]
GPU_WGRAD = (1025, 64, 48)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (BF16X3, FP32), ids=["bf16x3", "fp32"])
def test_query_names_the_launch(mode):
    import torch
    dev = "cuda"
    lib = _lib.load()
    on, read = lib.rd_debug_launch_log, lib.rd_debug_launch_log_read
    on.argtypes, on.restype = [ctypes.c_int], None
    read.argtypes, read.restype = [ctypes.c_char_p, ctypes.c_size_t], ctypes.c_size_t
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                          # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def logged(fn):
        buf = ctypes.create_string_buffer(1 << 12)
        on(1)
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            assert read(buf, len(buf)) < len(buf)
            on(0)
        return {n for n in buf.value.decode().split("\n") if n.startswith("k_gemm")}

    _lib.call("rd_set_precision", mode)
    try:
        g = torch.Generator().manual_seed(5)
        for M, N, K in GPU_FWD:
            x, W, b = (torch.randn(s, generator=g).to(dev) for s in ((M, K), (N, K), (N,)))
            y = torch.empty(M, N, device=dev)
            names = logged(lambda: _lib.call("rd_linear_fwd", M, N, K, ptr(x), K, ptr(W), ptr(b), ptr(y), N, 0, stream))
            assert names == {route(fwd(M, N, K))["name"]}, (M, N, K, names)
        M, N, K = GPU_WGRAD
        dy, x = torch.randn(M, N, generator=g).to(dev), torch.randn(M, K, generator=g).to(dev)
        dW, db = torch.empty(N, K, device=dev), torch.empty(N, device=dev)
        nbytes = int(lib.rd_linear_bwd_weight_workspace_bytes(M, N, K))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        names = logged(lambda: _lib.call("rd_linear_bwd_weight", M, N, K, ptr(dy), N, ptr(x), K, ptr(dW), ptr(db), ptr(ws), nbytes, stream))
        p = wgrad(M, N, K)
        assert p["nsplit"] == 17 and names == {route(p)["name"]}, names
    finally:
        on(0)
        _lib.call("rd_set_precision", BF16X3)


if __name__ == "__main__":
    print(json.dumps(_child_report(dict(kv.split("=") for kv in sys.argv[1].split()))))
