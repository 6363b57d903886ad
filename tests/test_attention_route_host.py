"""CPU: the route of a pass of the attention core (csrc/rd_attention.hip attn_route + attn_check, read through rd_debug_attention_route)
against a table written by hand from the conditions the parent evaluated in dispatch_attn, attn_b16_ok, attn_b16_mt_ok, attn_vec_ok, the
three launchers launch_attn / launch_attn_b16 / launch_attn_b16_mt and attn_big, against an independent restatement over a grid, under
every switch, and for both refusals.  The library loads without a device.  RD_ATTN_B16, RD_ATTN_B16_MT and RD_ATTN_BIG are read per call
(monkeypatch); RD_ATTN_FWD_W8 and RD_ATTN_BWD_W8 once per process (a child process: `python -m tests.test_attention_route_host`).  The
one GPU test at the end ties the query's names to the launch log.

The conditions, as the parent had them (modes: fp32 = 0, bf16x3 = 1, bf16 = 2; D = F d_ob + d_pe, hd = D / H).  Constants: TS = 64,
LDP = 68, LDT = 72, QROWS = 128, 512 threads in a multi-tile block, LDH = 16 nth + 4, LDB = 32 ceil(16 nth / 32) + 16.
  nth       ceil(hd / 16)
  vec       hd % 4 == 0 and D % 4 == 0 and aligned (qkv, out and dout all on 16-byte boundaries)
  big       hd > 96 or RD_ATTN_BIG != 0: materialised scores, no tiled launch; the callers decided it (attn_big) before dispatch_attn
  passes    forward: one launch.  Backward: T <= 64 one launch (the single-tile kernel), else dq then dk / dv
  single-tile split-bf16   a bf16 mode, RD_ATTN_B16 != 0, T <= 64, hd <= 96.  wide = the pass's switch (RD_ATTN_FWD_W8 / RD_ATTN_BWD_W8) != 0
            or a token plan; names k_attn_{fwd,bwd}_one_b16, + "w" when wide.  grid B H; block 512 wide, 256 narrow.
            LDS forward (6 64 LDB + (LDB >= 72 ? 0 : 2 64 72)) 2, + 4 64 4 when wide; backward (8 64 LDB + 4 64 72) 2 + 2 64 4.
            one_product (bf16 mode) goes as an argument
  multi-tile split-bf16    a bf16 mode, RD_ATTN_B16_MT != 0, T > 64, hd <= 96.  names k_attn_fwd_b16, k_attn_bwd_dq_b16, k_attn_bwd_dkv_b16.
            grid (ceil(T / 128), B H); block 512.  LDS 4 64 LDB 2 + 64 for forward and dq, 4 64 LDB 2 + 2 64 4 for dk / dv.
            one_product = plain bf16 mode, a template flag
  exact fp32 tiled         otherwise.  names k_attn_fwd, k_attn_bwd_one (T <= 64), k_attn_bwd_dq, k_attn_bwd_dkv.  grid (ceil(T / 64), B H),
            the single-tile backward B H; block 256.  LDS: forward attribute 4 (3 64 LDH + 64 68), forward launch 4 3 64 LDH when
            T <= 64 and LDH >= 68 (P overlays Q), else the attribute's; dq 4 (4 64 LDH + 64 68 + 128); dkv and one 4 (4 64 LDH + 2 64 68 + 128)
  refusals  a token plan outside the two split-bf16 families: RD_EUNSUPPORTED, "token plan: only the split-bf16 attention kernels ...";
            hd > 96 reaching the tiled kernels: RD_EUNSUPPORTED, "attention head_dim %d > 96 not built".  The plan's comes first.
No two of the parent's conditions were found to disagree.  One gap: dispatch_attn itself never looked at RD_ATTN_BIG -- its three callers
did (attn_big) before they called it, so no call reached it with the switch set.  The route reads the switch, reports the materialised
family (no launch), and a pass that gets such a route with hd <= 96 refuses it by a message of its own; no caller can."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from raindrop_amd import _lib
from tests.encoder_route_child import route as encoder_route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32, BF16X3, BF16 = 0, 1, 2
MODES = {FP32: "fp32", BF16X3: "bf16x3", BF16: "bf16"}
READ_ONCE = ("RD_ATTN_FWD_W8", "RD_ATTN_BWD_W8")
PER_CALL = ("RD_ATTN_B16", "RD_ATTN_B16_MT", "RD_ATTN_BIG")
PLAN_MSG = "token plan: only the split-bf16 attention kernels (head_dim <= 96, bf16 modes) read it"


def cdiv(a, b):
    return -(-a // b)


def shp(T, B, F, nhead, d_ob=4, d_pe=16, nhid=64):
    """the layer's shape by value: D = F d_ob + d_pe, hd = D / nhead"""
    return dict(T=T, B=B, F=F, nhead=nhead, d_ob=d_ob, d_pe=d_pe, nhid=nhid)


def heads(T, B, H, hd):
    """a shape with H heads of hd columns (d_ob = 1, d_pe = 0: F = D)"""
    return shp(T, B, H * hd, H, d_ob=1, d_pe=0)


def dims(s):
    D = s["F"] * s["d_ob"] + s["d_pe"]
    return D, D // s["nhead"]


def query(s, pas, plan=False, aligned=True):
    """-> (rc, route): names, the fields of words[0] and per launch (grid x, grid y, block, attribute LDS, launch LDS)"""
    shape = _lib.shape(s["B"], s["T"], s["F"], s["d_ob"], d_pe=s["d_pe"], nhead=s["nhead"], nhid=s["nhid"])
    words, name = (ctypes.c_uint32 * 11)(*([0xffffffff] * 11)), ctypes.create_string_buffer(64)
    rc = _lib.load().rd_debug_attention_route(ctypes.byref(shape), _lib.ATTN_PASSES.index(pas), int(plan), int(aligned), words, name, len(name))
    w = words[0]
    r = dict(names=name.value.decode(), family=_lib.ATTN_FAMILIES[w & 3], nth=w >> 8 & 15, nlaunch=w >> 12 & 3,
             launches=[tuple(words[1 + 5 * i:6 + 5 * i]) for i in range(2)])
    r.update({n: w >> (2 + i) & 1 for i, n in enumerate(_lib.ATTN_ROUTE_BITS)})
    return rc, r


def route(s, pas, plan=False, aligned=True):
    rc, r = query(s, pas, plan, aligned)
    assert rc == 0, (s, pas, plan, _lib.load().rd_last_error())
    return r


def row(r):
    """a route in the hand table's form"""
    return r["names"], r["nth"], r["vec"], r["wide"], r["launches"][:r["nlaunch"]]


# ---- the independent restatement ---------------------------------------------------------------------------------------------------
def restate(s, mode, pas, plan, aligned, env=None):
    """(rc, family, one_product, row) by the docstring's rules; env: the switches that are set"""
    env = env or {}
    on = lambda k, d=1: int(env.get(k, d)) != 0                              # noqa: E731
    T, BH = s["T"], s["B"] * s["nhead"]
    D, hd = dims(s)
    if hd > 96 or on("RD_ATTN_BIG", 0):
        return -2, "big", 0, ("", 0, 0, 0, [])
    nth = cdiv(hd, 16)
    vec = int(hd % 4 == 0 and D % 4 == 0 and aligned)
    ldh, ldb = 16 * nth + 4, 32 * cdiv(16 * nth, 32) + 16
    fwd = pas == "fwd"
    if mode != FP32 and T <= 64 and on("RD_ATTN_B16"):
        wide = int(on("RD_ATTN_FWD_W8" if fwd else "RD_ATTN_BWD_W8") or plan)
        if fwd:
            lds = (6 * 64 * ldb + (0 if ldb >= 72 else 2 * 64 * 72)) * 2 + (4 * 64 * 4 if wide else 0)
        else:
            lds = (8 * 64 * ldb + 4 * 64 * 72) * 2 + 2 * 64 * 4
        name = "k_attn_%s_one_b16%s" % (pas, "w" if wide else "")
        return 0, "one_b16", int(mode == BF16), (name, nth, vec, wide, [(BH, 1, 512 if wide else 256, lds, lds)])
    if mode != FP32 and T > 64 and on("RD_ATTN_B16_MT"):
        grid, planes = (cdiv(T, 128), BH), 4 * 64 * ldb * 2
        ls = [("k_attn_fwd_b16", planes + 64)] if fwd else [("k_attn_bwd_dq_b16", planes + 64), ("k_attn_bwd_dkv_b16", planes + 2 * 64 * 4)]
        return 0, "mt_b16", int(mode == BF16), (",".join(n for n, _ in ls), nth, vec, 0, [grid + (512, b, b) for _, b in ls])
    grid = (cdiv(T, 64), BH)
    attr = 4 * (3 * 64 * ldh + 64 * 68)
    dq, dkv = 4 * (4 * 64 * ldh + 64 * 68 + 128), 4 * (4 * 64 * ldh + 2 * 64 * 68 + 128)
    if fwd:
        names, ls = "k_attn_fwd", [grid + (256, attr, 4 * 3 * 64 * ldh if T <= 64 and ldh >= 68 else attr)]
    elif T <= 64:
        names, ls = "k_attn_bwd_one", [(BH, 1, 256, dkv, dkv)]
    else:
        names, ls = "k_attn_bwd_dq,k_attn_bwd_dkv", [grid + (256, dq, dq), grid + (256, dkv, dkv)]
    return (-2 if plan else 0), "fp32", 0, (names, nth, vec, 0, ls)


# ---- the hand table: id -> (shape, plan, aligned, bf16 modes forward, backward, fp32 mode forward, backward) ----------------------------
# a route: (names, nth, vec, wide, [(grid x, grid y, block, attribute LDS, launch LDS) per launch]).  LDS, worked out per nth:
#   nth  LDH  LDB | one_b16 fwd (+1024 wide)  one_b16 bwd | mt fwd, dq  mt dkv | fp32 fwd attr  overlaid    dq   dkv / one
#    1    20   48 |        55296                    86528 |      24640   25088 |         32768        -   38400    55808
#    3    52   80 |        61440                   119296 |      41024   41472 |         57344        -   71168    88576
#    4    68   80 |        61440                   119296 |      41024   41472 |         69632    52224   87552   104960
#    5    84  112 |        86016                   152064 |      57408   57856 |         81920    64512  103936   121344
#    6   100  112 |        86016                   152064 |      57408   57856 |         94208    76800  120320   137728
MT = "k_attn_bwd_dq_b16,k_attn_bwd_dkv_b16"
F2 = "k_attn_bwd_dq,k_attn_bwd_dkv"
P19, P12, PAM, SYN256 = shp(60, 8, 34, 2, nhid=272), shp(215, 4, 36, 2, nhid=288), shp(600, 4, 17, 2, nhid=136), shp(512, 2, 256, 2, nhid=2048)
BIG = ("", 0, 0, 0, [])
TABLE = {
    # the shapes the suite and the benchmark run.  P19: T 60, D 152, hd 76, 16 (sample, head) pairs
    "P19": (P19, False, True,
            ("k_attn_fwd_one_b16w", 5, 1, 1, [(16, 1, 512, 87040, 87040)]), ("k_attn_bwd_one_b16w", 5, 1, 1, [(16, 1, 512, 152064, 152064)]),
            ("k_attn_fwd", 5, 1, 0, [(1, 16, 256, 81920, 64512)]), ("k_attn_bwd_one", 5, 1, 0, [(16, 1, 256, 121344, 121344)])),
    "P19/unaligned": (P19, False, False,
                      ("k_attn_fwd_one_b16w", 5, 0, 1, [(16, 1, 512, 87040, 87040)]), ("k_attn_bwd_one_b16w", 5, 0, 1, [(16, 1, 512, 152064, 152064)]),
                      ("k_attn_fwd", 5, 0, 0, [(1, 16, 256, 81920, 64512)]), ("k_attn_bwd_one", 5, 0, 0, [(16, 1, 256, 121344, 121344)])),
    # a token plan: the eight-wave form whatever the switches say; the exact-fp32 family refuses it (None)
    "P19/plan": (P19, True, True,
                 ("k_attn_fwd_one_b16w", 5, 1, 1, [(16, 1, 512, 87040, 87040)]), ("k_attn_bwd_one_b16w", 5, 1, 1, [(16, 1, 512, 152064, 152064)]),
                 None, None),
    # P12: T 215, D 160, hd 80: 2 super-tiles of 128 rows, 4 tiles of 64
    "P12": (P12, False, True,
            ("k_attn_fwd_b16", 5, 1, 0, [(2, 8, 512, 57408, 57408)]), (MT, 5, 1, 0, [(2, 8, 512, 57408, 57408), (2, 8, 512, 57856, 57856)]),
            ("k_attn_fwd", 5, 1, 0, [(4, 8, 256, 81920, 81920)]), (F2, 5, 1, 0, [(4, 8, 256, 103936, 103936), (4, 8, 256, 121344, 121344)])),
    "P12/plan": (P12, True, True,
                 ("k_attn_fwd_b16", 5, 1, 0, [(2, 8, 512, 57408, 57408)]), (MT, 5, 1, 0, [(2, 8, 512, 57408, 57408), (2, 8, 512, 57856, 57856)]),
                 None, None),
    # PAM: T 600, D 84, hd 42: head rows are not 16-byte aligned -> vec off
    "PAM": (PAM, False, True,
            ("k_attn_fwd_b16", 3, 0, 0, [(5, 8, 512, 41024, 41024)]), (MT, 3, 0, 0, [(5, 8, 512, 41024, 41024), (5, 8, 512, 41472, 41472)]),
            ("k_attn_fwd", 3, 0, 0, [(10, 8, 256, 57344, 57344)]), (F2, 3, 0, 0, [(10, 8, 256, 71168, 71168), (10, 8, 256, 88576, 88576)])),
    # SYN256: D 1040, hd 520 -> materialised scores
    "SYN256": (SYN256, False, True, BIG, BIG, BIG, BIG),
    # hd 16 (the narrowest tile count; LDB 48 < 72: P^T has planes of its own), T 16
    "hd16": (shp(16, 2, 4, 2), False, True,
             ("k_attn_fwd_one_b16w", 1, 1, 1, [(4, 1, 512, 56320, 56320)]), ("k_attn_bwd_one_b16w", 1, 1, 1, [(4, 1, 512, 86528, 86528)]),
             ("k_attn_fwd", 1, 1, 0, [(1, 4, 256, 32768, 32768)]), ("k_attn_bwd_one", 1, 1, 0, [(4, 1, 256, 55808, 55808)])),
    # hd 42 at T = 64, the last single-tile length; LDH 52 < 68: no overlay
    "hd42/T64": (shp(64, 2, 17, 2), False, True,
                 ("k_attn_fwd_one_b16w", 3, 0, 1, [(4, 1, 512, 62464, 62464)]), ("k_attn_bwd_one_b16w", 3, 0, 1, [(4, 1, 512, 119296, 119296)]),
                 ("k_attn_fwd", 3, 0, 0, [(1, 4, 256, 57344, 57344)]), ("k_attn_bwd_one", 3, 0, 0, [(4, 1, 256, 88576, 88576)])),
    # T = 65: one key past a tile
    "hd16/T65": (shp(65, 2, 4, 2), False, True,
                 ("k_attn_fwd_b16", 1, 1, 0, [(1, 4, 512, 24640, 24640)]), (MT, 1, 1, 0, [(1, 4, 512, 24640, 24640), (1, 4, 512, 25088, 25088)]),
                 ("k_attn_fwd", 1, 1, 0, [(2, 4, 256, 32768, 32768)]), (F2, 1, 1, 0, [(2, 4, 256, 38400, 38400), (2, 4, 256, 55808, 55808)])),
    # hd 64: LDH = 68 = LDP, the narrowest head whose P overlays Q
    "hd64/T64": (shp(64, 3, 12, 1), False, True,
                 ("k_attn_fwd_one_b16w", 4, 1, 1, [(3, 1, 512, 62464, 62464)]), ("k_attn_bwd_one_b16w", 4, 1, 1, [(3, 1, 512, 119296, 119296)]),
                 ("k_attn_fwd", 4, 1, 0, [(1, 3, 256, 69632, 52224)]), ("k_attn_bwd_one", 4, 1, 0, [(3, 1, 256, 104960, 104960)])),
    # hd 96, the widest tiled head: single tile and T 130
    "hd96/T64": (shp(64, 2, 20, 1), False, True,
                 ("k_attn_fwd_one_b16w", 6, 1, 1, [(2, 1, 512, 87040, 87040)]), ("k_attn_bwd_one_b16w", 6, 1, 1, [(2, 1, 512, 152064, 152064)]),
                 ("k_attn_fwd", 6, 1, 0, [(1, 2, 256, 94208, 76800)]), ("k_attn_bwd_one", 6, 1, 0, [(2, 1, 256, 137728, 137728)])),
    "hd96/T130": (shp(130, 2, 20, 1), False, True,
                  ("k_attn_fwd_b16", 6, 1, 0, [(2, 2, 512, 57408, 57408)]), (MT, 6, 1, 0, [(2, 2, 512, 57408, 57408), (2, 2, 512, 57856, 57856)]),
                  ("k_attn_fwd", 6, 1, 0, [(3, 2, 256, 94208, 94208)]), (F2, 6, 1, 0, [(3, 2, 256, 120320, 120320), (3, 2, 256, 137728, 137728)])),
    # hd 97 (D 388, four heads), one column past the widest tiled head
    "hd97": (shp(16, 2, 93, 4), False, True, BIG, BIG, BIG, BIG),
}
# the same under the per-call switches, bf16 modes: (row, switch) -> (forward, backward); None: refused (plan), BIG: no launch
FORCED = {
    ("P19", "RD_ATTN_B16=0"): TABLE["P19"][5:7],
    ("P19/plan", "RD_ATTN_B16=0"): (None, None),
    ("P12", "RD_ATTN_B16=0"): TABLE["P12"][3:5],               # not its switch
    ("P12", "RD_ATTN_B16_MT=0"): TABLE["P12"][5:7],
    ("P12/plan", "RD_ATTN_B16_MT=0"): (None, None),
    ("hd16", "RD_ATTN_B16_MT=0"): TABLE["hd16"][3:5],          # not its switch
    ("P19", "RD_ATTN_BIG=1"): (BIG, BIG),
    ("PAM", "RD_ATTN_BIG=1"): (BIG, BIG),
}


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    for k in READ_ONCE + PER_CALL:
        monkeypatch.delenv(k, raising=False)
    yield
    _lib.call("rd_set_precision", BF16X3)


def _expect(want, s, pas, plan, aligned, mode, env=None):
    """the query against one hand-table entry; the restatement is held to the entry too"""
    rc, r = query(s, pas, plan, aligned)
    src, fam, one, rrow = restate(s, mode, pas, plan, aligned, env)
    if want is None:                                          # a plan outside the split-bf16 families
        assert rc == src == -2 and PLAN_MSG in _lib.load().rd_last_error().decode(), (s, pas, rc)
        return
    assert row(r) == want == rrow, (s, pas, MODES[mode], row(r), want, rrow)
    assert (r["family"], r["one_product"]) == (fam, one) and rc == src == (-2 if want == BIG else 0), (s, pas, r, rc)
    assert (r["family"] == "big") == (want == BIG) == (r["nlaunch"] == 0)


@pytest.mark.parametrize("mode", sorted(MODES), ids=[MODES[m] for m in sorted(MODES)])
def test_hand_table(mode):
    _lib.call("rd_set_precision", mode)
    for case, (s, plan, aligned, bf, bb, ff, fb) in TABLE.items():
        for pas, want in (("fwd", ff if mode == FP32 else bf), ("bwd", fb if mode == FP32 else bb)):
            _expect(want, s, pas, plan, aligned, mode)


@pytest.mark.parametrize("mode", (BF16X3, BF16), ids=["bf16x3", "bf16"])
def test_per_call_switches_on_the_table(mode, monkeypatch):
    _lib.call("rd_set_precision", mode)
    for (case, switch), wants in FORCED.items():
        s, plan, aligned = TABLE[case][:3]
        with monkeypatch.context() as m:
            k, v = switch.split("=")
            m.setenv(k, v)
            for pas, want in zip(("fwd", "bwd"), wants):
                _expect(want, s, pas, plan, aligned, mode, {k: v})


GRID_T = (1, 16, 63, 64, 65, 128, 129, 300)
GRID_HD = (4, 16, 17, 42, 48, 80, 96)


def _grid(mode, env=None):
    """every (T, hd, H, B, pass, plan, aligned) of the grid: the query against the restatement"""
    bad, n, seen = [], 0, set()
    for T in GRID_T:
        for hd in GRID_HD:
            for H in (1, 2, 4):
                for B in (1, 5):
                    s = heads(T, B, H, hd)
                    for pas in _lib.ATTN_PASSES:
                        for plan in (False, True):
                            for aligned in (True, False):
                                rc, r = query(s, pas, plan, aligned)
                                src, fam, one, rrow = restate(s, mode, pas, plan, aligned, env)
                                n += 1
                                seen.update(r["names"].split(","))
                                if (rc, r["family"], r["one_product"], row(r)) != (src, fam, one, rrow):
                                    bad.append((s, pas, plan, aligned, rc, r, (src, fam, one, rrow)))
    return n, bad, seen


@pytest.mark.parametrize("mode", sorted(MODES), ids=[MODES[m] for m in sorted(MODES)])
def test_restatement_over_a_grid(mode):
    _lib.call("rd_set_precision", mode)
    n, bad, seen = _grid(mode)
    assert n == 8 * 7 * 3 * 2 * 8 and not bad, (n, bad[:3])
    if mode == FP32:
        assert seen == {"k_attn_fwd", "k_attn_bwd_one", "k_attn_bwd_dq", "k_attn_bwd_dkv"}
    else:                                                     # the default switches reach neither the narrow form nor the exact-fp32 family
        assert seen == {"k_attn_fwd_one_b16w", "k_attn_bwd_one_b16w", "k_attn_fwd_b16", "k_attn_bwd_dq_b16", "k_attn_bwd_dkv_b16"}


@pytest.mark.parametrize("switch", ("RD_ATTN_B16=0", "RD_ATTN_B16_MT=0", "RD_ATTN_BIG=1", "RD_ATTN_B16=0 RD_ATTN_B16_MT=0"))
@pytest.mark.parametrize("mode", sorted(MODES), ids=[MODES[m] for m in sorted(MODES)])
def test_per_call_switches_over_the_grid(mode, switch, monkeypatch):
    _lib.call("rd_set_precision", mode)
    env = dict(kv.split("=") for kv in switch.split())
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n, bad, seen = _grid(mode, env)
    assert n == 8 * 7 * 3 * 2 * 8 and not bad, (switch, bad[:3])
    if switch == "RD_ATTN_BIG=1":
        assert seen == {""}
    elif len(env) == 2:
        assert seen == {"k_attn_fwd", "k_attn_bwd_one", "k_attn_bwd_dq", "k_attn_bwd_dkv"}


def test_words_past_the_last_launch_are_zero():
    for s, pas, n in ((P19, "fwd", 1), (P12, "bwd", 2), (SYN256, "fwd", 0)):
        rc, r = query(s, pas)
        assert r["nlaunch"] == n and all(l == (0,) * 5 for l in r["launches"][n:]) and r["names"].count(",") == max(n - 1, 0)


# ---- refusals: attn_check's, with the code and message of the pass --------------------------------------------------------------------
def test_refusals(monkeypatch):
    err = lambda: _lib.load().rd_last_error().decode()                       # noqa: E731
    for mode in MODES:
        _lib.call("rd_set_precision", mode)
        for pas in _lib.ATTN_PASSES:
            # a token plan on a family that does not read it: every shape in exact fp32, none in a bf16 mode ...
            for s in (P19, P12, PAM):
                rc, r = query(s, pas, plan=True)
                assert rc == (-2 if mode == FP32 else 0), (MODES[mode], pas, rc)
                assert (PLAN_MSG in err() and r["family"] == "fp32") if rc else r["family"] in ("one_b16", "mt_b16")
            # ... head_dim > 96 reaching the tiled kernels; with a plan, the plan's refusal comes first
            rc, r = query(SYN256, pas)
            assert rc == -2 and "attention head_dim 520 > 96 not built" in err() and r["family"] == "big" and r["names"] == ""
            rc, r = query(heads(16, 2, 1, 97), pas)
            assert rc == -2 and "attention head_dim 97 > 96 not built" in err()
            assert query(heads(16, 2, 1, 96), pas)[0] == 0
            rc, r = query(SYN256, pas, plan=True)
            assert rc == -2 and PLAN_MSG in err()
    # a bf16 mode with the family's switch off: the plan is refused there too
    _lib.call("rd_set_precision", BF16X3)
    monkeypatch.setenv("RD_ATTN_B16", "0")
    assert query(P19, "fwd", plan=True)[0] == -2 and PLAN_MSG in err()
    assert query(P12, "fwd", plan=True)[0] == 0
    monkeypatch.setenv("RD_ATTN_BIG", "1")
    rc, r = query(P19, "fwd")
    assert rc == -2 and "RD_ATTN_BIG" in err() and "only the layer runs" in err() and r["family"] == "big"
    # a bad shape or pass is an error of its own
    assert query(shp(16, 2, 5, 5), "fwd")[0] == -1 and "not divisible" in err()
    shape = _lib.shape(2, 16, 4, 4, nhid=64)
    words, name = (ctypes.c_uint32 * 11)(), ctypes.create_string_buffer(64)
    assert _lib.load().rd_debug_attention_route(ctypes.byref(shape), 2, 0, 1, words, name, len(name)) == -1 and "pass" in err()


# ---- consistency with the other queries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ("", "RD_ATTN_BIG=1"))
def test_encoder_route_big_is_the_attention_family(switch, monkeypatch):
    if switch:
        monkeypatch.setenv(*switch.split("="))
    for mode in MODES:
        _lib.call("rd_set_precision", mode)
        for case, (s, plan, aligned, *_) in TABLE.items():
            assert (s["d_ob"], s["d_pe"]) == (4, 16)              # what the encoder child's query is written at
            enc = encoder_route(s["B"], s["T"], s["F"], s["nhid"], plan, nhead=s["nhead"])
            for pas in _lib.ATTN_PASSES:
                assert ("big" in enc) == (query(s, pas, plan, aligned)[1]["family"] == "big") == (bool(switch) or case in ("SYN256", "hd97")), (case, pas)


# rd_encoder_layer_saved_bytes / rd_encoder_layer_workspace_bytes, recorded from the parent build (they follow attn_big)
RECORDED_BYTES = [(P19, "", 6245632, 14777344), (P12, "", 9774336, 22128896), (SYN256, "", 137819136, 385770240),
                  (P19, "RD_ATTN_BIG=1", 6706432, 15007744)]


def test_layer_buffer_sizes_are_the_parents(monkeypatch):
    lib = _lib.load()
    for s, switch, saved, ws in RECORDED_BYTES:
        with monkeypatch.context() as m:
            if switch:
                m.setenv(*switch.split("="))
            shape = _lib.shape(s["B"], s["T"], s["F"], 4, nhead=s["nhead"], nhid=s["nhid"])
            assert (lib.rd_encoder_layer_saved_bytes(ctypes.byref(shape)), lib.rd_encoder_layer_workspace_bytes(ctypes.byref(shape))) == (saved, ws)


# ---- the switches read once per process: a child --------------------------------------------------------------------------------------
CHILD_SWITCHES = ("", "RD_ATTN_FWD_W8=0", "RD_ATTN_BWD_W8=0", "RD_ATTN_FWD_W8=0 RD_ATTN_BWD_W8=0")
# by hand, bf16 modes, P19: (forward, backward) without a plan -- with one, both are the eight-wave form under every switch
NARROW_F, NARROW_B = ["k_attn_fwd_one_b16", 5, 1, 0, [[16, 1, 256, 86016, 86016]]], ["k_attn_bwd_one_b16", 5, 1, 0, [[16, 1, 256, 152064, 152064]]]
WIDE_F, WIDE_B = (json.loads(json.dumps(TABLE["P19"][i])) for i in (3, 4))
CHILD_ROWS = {"": (WIDE_F, WIDE_B), "RD_ATTN_FWD_W8=0": (NARROW_F, WIDE_B), "RD_ATTN_BWD_W8=0": (WIDE_F, NARROW_B),
              "RD_ATTN_FWD_W8=0 RD_ATTN_BWD_W8=0": (NARROW_F, NARROW_B)}


def _child_report(env):
    out = {}
    for mode in MODES:
        _lib.call("rd_set_precision", mode)
        n, bad, seen = _grid(mode, env)
        out[MODES[mode]] = {"rows": [row(route(P19, pas, plan)) for plan in (False, True) for pas in _lib.ATTN_PASSES if not (plan and mode == FP32)],
                            "grid": n, "bad": [repr(b) for b in bad[:3]], "seen": sorted(seen)}
    return out


@pytest.mark.parametrize("switch", CHILD_SWITCHES, ids=lambda s: s.replace(" ", ",") or "default")
def test_read_once_switches_in_a_child(switch):
    env = {k: v for k, v in os.environ.items() if k not in READ_ONCE + PER_CALL}
    env.update(kv.split("=") for kv in switch.split())
    env["CUDA_VISIBLE_DEVICES"] = env["HIP_VISIBLE_DEVICES"] = ""           # a CPU child
    res = subprocess.run([sys.executable, "-m", "tests.test_attention_route_host", switch], cwd=ROOT, env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    rep = json.loads(res.stdout.strip().splitlines()[-1])
    for mode, r in rep.items():
        assert r["grid"] == 8 * 7 * 3 * 2 * 8 and not r["bad"], (switch, mode, r["bad"])
        if mode == "fp32":
            assert r["rows"] == json.loads(json.dumps(list(TABLE["P19"][5:7]))), (switch, r["rows"])
            continue
        assert r["rows"] == list(CHILD_ROWS[switch]) + [WIDE_F, WIDE_B], (switch, mode, r["rows"])
        assert ("k_attn_fwd_one_b16" in r["seen"]) == ("FWD_W8" in switch) and ("k_attn_bwd_one_b16" in r["seen"]) == ("BWD_W8" in switch)


# ---- GPU: the names the query gives are the attention names in the launch log ------------------------------------------------------------
# (T, B, F, nhead) at d_ob = 4, d_pe = 16: a short single tile; hd 42 at T = 64, no 16-byte rows; one key past a tile; hd 96 over three tiles
GPU_SHAPES = [(16, 2, 4, 2), (64, 2, 17, 2), (65, 2, 4, 2), (130, 2, 20, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES), ids=[MODES[m] for m in sorted(MODES)])
def test_query_names_the_launches(mode, monkeypatch):
    import torch
    dev = "cuda"
    lib = _lib.load()
    on, read = lib.rd_debug_launch_log, lib.rd_debug_launch_log_read
    on.argtypes, on.restype = [ctypes.c_int], None
    read.argtypes, read.restype = [ctypes.c_char_p, ctypes.c_size_t], ctypes.c_size_t
    P = lambda t: ctypes.c_void_p(t.data_ptr())                            # noqa: E731

    def logged(T, B, F, nhead):
        s = shp(T, B, F, nhead)
        D, _ = dims(s)
        g = torch.Generator().manual_seed(T)
        qkv, dout = torch.randn(T, B, 3 * D, generator=g).to(dev), torch.randn(T, B, D, generator=g).to(dev)
        mask = torch.zeros(B, T, dtype=torch.uint8, device=dev)
        mask[1, T - T // 3:] = 1
        out, lse, ws = torch.empty(T, B, D, device=dev), torch.empty(B, nhead, T, device=dev), torch.empty(B, nhead, T, device=dev)
        dqkv = torch.empty_like(qkv)
        assert all(t.data_ptr() % 16 == 0 for t in (qkv, out, dout))
        shape = _lib.shape(B, T, F, 4, nhead=nhead, nhid=64)
        buf = ctypes.create_string_buffer(1 << 12)
        on(1)
        try:
            _lib.call("rd_attention_fwd", ctypes.byref(shape), 0, P(qkv), P(mask), 0.0, 0, P(out), P(lse), None)
            _lib.call("rd_attention_bwd", ctypes.byref(shape), 0, P(qkv), P(mask), 0.0, 0, P(out), P(lse), P(dout), P(dqkv), P(ws), None)
            torch.cuda.synchronize()
        finally:
            assert read(buf, len(buf)) < len(buf)
            on(0)
        want = {n for pas in _lib.ATTN_PASSES for n in route(s, pas)["names"].split(",")}
        return {n for n in buf.value.decode().split("\n") if n.startswith("k_attn")}, want

    _lib.call("rd_set_precision", mode)
    try:
        for dims4 in GPU_SHAPES:
            got, want = logged(*dims4)
            assert got == want and len(want) in (2, 3), (dims4, got, want)
        monkeypatch.setenv("RD_ATTN_B16", "0")
        got, want = logged(*GPU_SHAPES[0])
        assert got == want == {"k_attn_fwd", "k_attn_bwd_one"}, (got, want)
    finally:
        on(0)
        _lib.call("rd_set_precision", BF16X3)


if __name__ == "__main__":
    print(json.dumps(_child_report(dict(kv.split("=") for kv in sys.argv[1].split()))))
