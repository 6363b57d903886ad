"""CPU: the route of a sensor-stage call (csrc/rd_k1_route.h k1_route, read through rd_debug_sensor_route) against a table written by
hand from the conditions the entry points of rd_msgpass.hip / rd_msgpass_fused.hip evaluated before the route existed, its
invariants over a grid of shapes, and the queries that must agree with it (rd_step_prepare_covers, rd_infer_covers, the four byte
queries).  The library loads without a device; RD_K1_FUSED, RD_K1_SPECIALIZE and RD_K1_WGRAD_STREAM are read per call, so
monkeypatch sets them and no child process is needed.

The conditions, as the parent had them (bf16x3 = mode 1, bf16 = 2, fp32 = 0):
  fused         mode bf16x3, RD_K1_FUSED != 0, d_ob == 4, F <= 48, K = 4 T in [16, 240] and a multiple of 16, B*T < 2^22
  rt            ceil(F / 16) of a fused call
  specialised   fused, F == 34, T == 60, RD_K1_SPECIALIZE != 0, ldz == 4 F + 16 -- and d_pe == 16 where the call writes PE
                (rd_msgpass_fwd and the backward write none: whatever d_pe is)
  infer         fused, F == 34, T == 60, RD_K1_SPECIALIZE != 0, d_pe == 16: the shape alone, no ldz.  The one place where two of the
                parent's tests disagree: a PE-less call at another ldz (P19/plain/ldz200 below) is not specialised though the shape
                has an inference forward; every sensor-stage call has ldz = 4 F + d_pe, where the two coincide
  tiles         not fused and mode != fp32
  wgrad_stream  tiles, M = B F >= 2048, K >= 512, K % 4 == 0, M >= 4 K, RD_K1_WGRAD_STREAM != 0 (and RD_TILE_WGRAD != 0)"""
import ctypes

import pytest

from raindrop_amd import _lib, synth

MODES = {0: "fp32", 1: "bf16x3", 2: "bf16"}
SWITCHES = ("", "RD_K1_FUSED=0", "RD_K1_SPECIALIZE=0", "RD_K1_WGRAD_STREAM=0")
BYTE_QUERIES = ("rd_msgpass_workspace_bytes", "rd_msgpass_saved_bytes", "rd_msgpass_infer_bytes", "rd_obs_embed_bwd_workspace_bytes")

# name -> ((B, T, F, d_ob, d_pe), ldz (None: F d_ob + d_pe, the model's z), with_pe, with_coef,
#          bf16x3: default, RD_K1_SPECIALIZE=0;   generic = bf16x3 under RD_K1_FUSED=0 and the bf16 mode: default, RD_K1_WGRAD_STREAM=0)
# fp32: nothing is ever set but `coef`.  `coef` is left out of the strings: it is set exactly where with_coef is.
G = ("tiles", "tiles")
CASES = {
    # the envelope edges of tests/test_sensor_stage_float64_gpu.py: F = 16/17, 32/33, 48/49
    "F16": ((3, 8, 16, 4, 16), None, 1, 0, "fused rt1", "fused rt1") + G,
    "F17": ((3, 8, 17, 4, 16), None, 1, 0, "fused rt2", "fused rt2") + G,
    "F32": ((3, 8, 32, 4, 16), None, 1, 0, "fused rt2", "fused rt2") + G,
    "F33": ((3, 8, 33, 4, 16), None, 1, 0, "fused rt3", "fused rt3") + G,
    "F48": ((3, 8, 48, 4, 16), None, 1, 0, "fused rt3", "fused rt3") + G,
    "F49": ((3, 8, 49, 4, 16), None, 1, 0, "tiles", "tiles") + G,
    # T = 60/61 (K = 240/244), K no multiple of 16, K < 16, d_ob != 4
    "T60": ((3, 60, 5, 4, 16), None, 1, 0, "fused rt1", "fused rt1") + G,
    "T61": ((3, 61, 5, 4, 16), None, 1, 0, "tiles", "tiles") + G,
    "T15": ((3, 15, 5, 4, 16), None, 1, 0, "tiles", "tiles") + G,
    "T4": ((3, 4, 5, 4, 16), None, 1, 0, "fused rt1", "fused rt1") + G,
    "T3": ((3, 3, 5, 4, 16), None, 1, 0, "tiles", "tiles") + G,
    "D2": ((3, 8, 5, 2, 16), None, 1, 0, "tiles", "tiles") + G,
    "D8": ((3, 4, 5, 8, 16), None, 1, 0, "tiles", "tiles") + G,
    # B*T at the 2^22 bound: 2^22 - 4 rows fused, 2^22 not
    "BT_below": (((1 << 20) - 1, 4, 1, 4, 16), None, 1, 0, "fused rt1", "fused rt1") + G,
    "BT_at": ((1 << 20, 4, 1, 4, 16), None, 1, 0, "tiles", "tiles") + G,
    # P19, the model's layout (ldz = 152, d_pe = 16): sensor-stage call, with the table, PE-less call (rd_msgpass_fwd, the backward)
    "P19": ((8, 60, 34, 4, 16), None, 1, 0, "fused rt3 specialised infer", "fused rt3") + G,
    "P19/coef": ((8, 60, 34, 4, 16), None, 1, 1, "fused rt3 specialised infer", "fused rt3") + G,
    "P19/plain": ((8, 60, 34, 4, 16), 152, 0, 0, "fused rt3 specialised infer", "fused rt3") + G,
    "P19/plain/coef": ((8, 60, 34, 4, 16), 152, 0, 1, "fused rt3 specialised infer", "fused rt3") + G,
    # P19 out of the model's layout: another row stride; d_pe = 8 with PE (ldz = 144) and without at ldz = 152 (specialised: no PE is
    # written, so d_pe is not looked at -- but the shape has no inference forward)
    "P19/plain/ldz200": ((8, 60, 34, 4, 16), 200, 0, 0, "fused rt3 infer", "fused rt3") + G,
    "P19/plain/ldz200/coef": ((8, 60, 34, 4, 16), 200, 0, 1, "fused rt3 infer", "fused rt3") + G,
    "P19/pe8": ((8, 60, 34, 4, 8), None, 1, 0, "fused rt3", "fused rt3") + G,
    "P19/pe8/coef": ((8, 60, 34, 4, 8), None, 1, 1, "fused rt3", "fused rt3") + G,
    "P19/pe8/plain152": ((8, 60, 34, 4, 8), 152, 0, 0, "fused rt3 specialised", "fused rt3") + G,
    "P19/T56": ((8, 56, 34, 4, 16), None, 1, 0, "fused rt3", "fused rt3") + G,
    "P19/F35": ((8, 60, 35, 4, 16), None, 1, 0, "fused rt3", "fused rt3") + G,
    # the generic side.  P12 (K = 860): the stream at M = B F >= 4 K = 3440 rows, B = 96 (3456), not at B = 95 (3420); SYN256
    # (K = 2048, M = 4096 < 4 K) and PAM (K = 2400, M = 1088 < 2048) keep the split-K GEMMs
    "P12": ((256, 215, 36, 4, 16), None, 1, 0, "tiles wgrad_stream", "tiles wgrad_stream", "tiles wgrad_stream", "tiles"),
    "P12/coef": ((256, 215, 36, 4, 16), None, 1, 1, "tiles wgrad_stream", "tiles wgrad_stream", "tiles wgrad_stream", "tiles"),
    "P12/B96": ((96, 215, 36, 4, 16), None, 1, 0, "tiles wgrad_stream", "tiles wgrad_stream", "tiles wgrad_stream", "tiles"),
    "P12/B95": ((95, 215, 36, 4, 16), None, 1, 0, "tiles", "tiles") + G,
    "PAM": ((64, 600, 17, 4, 16), None, 1, 0, "tiles", "tiles") + G,
    "SYN256": ((16, 512, 256, 4, 16), None, 1, 0, "tiles", "tiles") + G,
}


def _shape(dims):
    B, T, F, d_ob, d_pe = dims
    return _lib.shape(B, T, F, d_ob, d_pe=d_pe, nhead=2, nhid=8 * F)


def route(dims, ldz=None, with_pe=1, with_coef=0):
    """the set K1Route fields (_lib.SENSOR_ROUTE_BITS) plus "rt<n>" of a fused call"""
    B, T, F, d_ob, d_pe = dims
    shp = _shape(dims)
    bits = ctypes.c_uint32(0xffffffff)
    _lib.call("rd_debug_sensor_route", ctypes.byref(shp), F * d_ob + d_pe if ldz is None else ldz, with_pe, with_coef, ctypes.byref(bits))
    assert bits.value & ~0x33f == 0, hex(bits.value)
    r = {n for i, n in enumerate(_lib.SENSOR_ROUTE_BITS) if bits.value >> i & 1}
    return r | ({"rt%d" % (bits.value >> 8)} if bits.value >> 8 else set())


def expected(name, mode, switch):
    dims, ldz, pe, coef, x3, x3_spec0, gen, gen_ws0 = CASES[name]
    if mode == 0:
        want = ""
    elif mode == 2 or switch == "RD_K1_FUSED=0":
        want = gen_ws0 if switch == "RD_K1_WGRAD_STREAM=0" else gen
    elif "fused" not in x3:                                  # bf16x3 outside the envelope: the generic side's columns
        want = gen_ws0 if switch == "RD_K1_WGRAD_STREAM=0" else x3
    else:
        want = x3_spec0 if switch == "RD_K1_SPECIALIZE=0" else x3
    return set(want.split()) | ({"coef"} if coef else set())


def _covers(name, shp, second):
    a, b = ctypes.c_int32(-1), ctypes.c_int32(-1)
    _lib.call(name, ctypes.byref(shp), ctypes.byref(a), ctypes.byref(b))
    return (b if second else a).value


def _bytes(shp):
    lib = _lib.load()
    out = []
    for q in BYTE_QUERIES:
        fn = getattr(lib, q)
        fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_void_p]
        out.append(fn(ctypes.byref(shp)))
    return out


def queries_agree(name, mode, switch):
    """What the library's public queries must answer for a case of the table (this half needs no route query: it was run once against
    the parent commit's library, which passed it, before the route was written).  Returns the four byte counts."""
    dims = CASES[name][0]
    want = expected(name, mode, switch)
    shp = _shape(dims)
    tag = (name, MODES[mode], switch)
    # the covers queries see the shape alone: `infer` as the table has it for a call in the model's layout
    sensor_form = expected(name.split("/plain")[0], mode, switch) if "/plain" in name else want
    assert _covers("rd_step_prepare_covers", shp, True) == ("fused" in want), tag
    assert _covers("rd_infer_covers", shp, False) == ("infer" in sensor_form), tag
    ws, saved, infer, embed = n = _bytes(shp)
    assert (infer < saved) == ("infer" in sensor_form) and infer <= saved, tag
    return n


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for sw in SWITCHES[1:] + ("RD_TILE_WGRAD=0",):
        monkeypatch.delenv(sw.split("=")[0], raising=False)
    yield
    _lib.call("rd_set_precision", 1)


def test_table_is_complete():
    for name in ("P19", "P12", "PAM", "SYN256"):
        cfg = synth.make_config(name)
        assert CASES[name][0][1:3] == (cfg["max_len"], cfg["d_inp"]), name
    words = set(_lib.SENSOR_ROUTE_BITS) | {"rt1", "rt2", "rt3"}
    assert all(set(" ".join(c[4:]).split()) <= words for c in CASES.values())
    assert {"P19/plain/ldz200", "P19/plain/ldz200/coef"} == {n for n, c in CASES.items() if "infer" in c[4] and "specialised" not in c[4]}     # the reported disagreement


@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: s or "default")
@pytest.mark.parametrize("mode", sorted(MODES), ids=[MODES[m] for m in sorted(MODES)])
def test_route_table(mode, switch, monkeypatch):
    if switch:
        monkeypatch.setenv(*switch.split("="))
    _lib.call("rd_set_precision", mode)
    bad = []
    for name, (dims, ldz, pe, coef) in ((n, c[:4]) for n, c in CASES.items()):
        got, want = route(dims, ldz, pe, coef), expected(name, mode, switch)
        if got != want:
            bad.append((name, "want", sorted(want), "got", sorted(got)))
        queries_agree(name, mode, switch)
    assert not bad, (MODES[mode], switch, bad)


def test_byte_queries_do_not_depend_on_mode_or_switches(monkeypatch):
    """but for rd_msgpass_infer_bytes, which follows `infer` (checked against the table in queries_agree)"""
    _lib.call("rd_set_precision", 1)
    base = {name: queries_agree(name, 1, "") for name in CASES}
    for switch in SWITCHES:
        if switch:
            monkeypatch.setenv(*switch.split("="))
        for mode in MODES:
            _lib.call("rd_set_precision", mode)
            for name in CASES:
                n = queries_agree(name, mode, switch)
                assert n[:2] + n[3:] == base[name][:2] + base[name][3:], (name, MODES[mode], switch)
                assert n[2] in (base[name][2], n[1]), (name, MODES[mode], switch)      # the inference size, or the saved size
        if switch:
            monkeypatch.delenv(switch.split("=")[0])


def test_wgrad_stream_follows_the_tile_stream_switch(monkeypatch):
    _lib.call("rd_set_precision", 2)
    assert "wgrad_stream" in route(CASES["P12"][0])
    monkeypatch.setenv("RD_TILE_WGRAD", "0")
    assert route(CASES["P12"][0]) == {"tiles"}


GRID_F = list(range(1, 52)) + [64, 256]
GRID_T = (3, 4, 15, 56, 60, 61, 215)


@pytest.mark.parametrize("switch", SWITCHES[:3], ids=lambda s: s or "default")
@pytest.mark.parametrize("mode", sorted(MODES), ids=[MODES[m] for m in sorted(MODES)])
def test_route_invariants(mode, switch, monkeypatch):
    """over sensor-stage calls (PE, ldz = 4 F + d_pe) and PE-less calls on the same z, with and without the table"""
    if switch:
        monkeypatch.setenv(*switch.split("="))
    _lib.call("rd_set_precision", mode)
    for F in GRID_F:
        for T in GRID_T:
            for d_pe in (16, 8):
                dims = (3, T, F, 4, d_pe)
                shp = _shape(dims)
                for pe in (1, 0):
                    for coef in (0, 1):
                        r = route(dims, None, pe, coef)
                        tag = (F, T, d_pe, pe, coef, sorted(r))
                        rt = {w for w in r if w.startswith("rt")}
                        assert (rt == {"rt%d" % ((F + 15) // 16)}) if "fused" in r else not rt, tag
                        if "specialised" in r:
                            assert {"rt3", "fused"} <= r, tag
                        if "infer" in r:
                            assert "specialised" in r, tag
                        if "fused" in r:
                            assert not r & {"tiles", "wgrad_stream"}, tag
                        if "wgrad_stream" in r:
                            assert "tiles" in r, tag
                        assert ("coef" in r) == bool(coef), tag
                        assert _covers("rd_step_prepare_covers", shp, True) == ("fused" in r), tag
                        assert _covers("rd_infer_covers", shp, False) == ("infer" in r), tag
