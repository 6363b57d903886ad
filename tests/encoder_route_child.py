"""Child process of tests/test_encoder_route_host.py (not collected by pytest: run as a module).

    python -m tests.encoder_route_child

prints, as one JSON line, the route of an encoder layer (rd_debug_encoder_route) for every configuration, arithmetic mode and
with / without a token plan, under WHATEVER environment it was started with: RD_ROWGEMM, RD_LN_FUSE and RD_LNB_FUSE are read once
per process, so only a fresh process can see another value.  Needs no device."""
import ctypes
import json

from raindrop_amd import _lib

MODES = {0: "fp32", 1: "bf16x3", 2: "bf16"}
# name -> (B, T, F, nhid): synth.make_config's widths (D = 4 F + 16, nhid = 8 F) and the (35, 156, 260) width of
# tests/switch_child.py RB_WIDTHS.  SYN256 at B = 2: M = 1024 rows, the smallest at which tw2 applies
CONFIGS = {"P19": (8, 60, 34, 272), "P12": (4, 215, 36, 288), "PAM": (4, 600, 17, 136), "SYN256": (2, 512, 256, 2048),
           "RB156": (5, 13, 35, 260)}


def route(B, T, F, nhid, with_plan, nhead=2):
    """the set of EncRoute fields (_lib.ROUTE_BITS) that are set"""
    shp = _lib.shape(B, T, F, 4, nhead=nhead, nhid=nhid)
    bits = ctypes.c_uint32(0xffffffff)
    _lib.call("rd_debug_encoder_route", ctypes.byref(shp), int(with_plan), ctypes.byref(bits))
    assert bits.value < (1 << len(_lib.ROUTE_BITS))
    return {n for i, n in enumerate(_lib.ROUTE_BITS) if bits.value >> i & 1}


def all_routes():
    """{"<config>/<mode>/<plan>": sorted fields} in the environment this process started with"""
    out = {}
    for cfg, dims in CONFIGS.items():
        for mode in MODES:
            _lib.call("rd_set_precision", mode)
            for plan in (0, 1):
                out["%s/%d/%d" % (cfg, mode, plan)] = sorted(route(*dims, plan))
    _lib.call("rd_set_precision", 1)
    return out


if __name__ == "__main__":
    print(json.dumps(all_routes()))
