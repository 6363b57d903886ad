"""GPU: the use_beta graph operator (rd_graph_beta_fwd / _bwd / _bwd_alpha / _fwd_dropout / _bwd_dropout through the C-ABI) against
float64 across the envelope of both forms -- the LDS form's 16-wave kernels (rd_graph_beta.hip k_graph_beta_fwd2 / _bwd2: ballot
tails at Kk = 63 / 64 / 65 / 129, node counts around the 16 waves, nodes without out-edges, self-loops, duplicated edges, one source
or one target owning every edge, E = 0 .. 3, E = 4096 with V staged and not, ragged backward chunks), the workspace form's k_bl_*
launches (rd_graph_beta_large.hip: the hand-over at E = 4097 and N = 65, three and four 4096-key sort chunks with pad keys, two
list-staging passes, N = 1024, the refusal at 1025), every batch-stride combination, the tie rule, and a reduced list on the rounds
2-5 kernels (RD_BETA_V1=1).  Cases, inputs, reference and bounds: tests/beta_operator_ref.py (tests/test_beta_operator_ref_host.py
shows on the reference alone that pruning is decisive in every case and that the bounds bite).

Every run: forward then backward in one of three modes (no dalpha; dalpha; p_drop = 0.3 with dalpha under the host-generated mask of
tests/rng_ref.py), the launch log on, every output buffer and the workspace pre-filled with a NaN pattern and followed by a guard tail
of the same pattern that must survive (a write-side guard: no input is made illegal).  Compared: out, edge_index_out, alpha_out,
beta_save, kept, dV, dH, the sum of dmap_part over the batch, dw.  The log must prove the form (k_graph_beta_*2, k_bl_*, or the
rounds 2-5 names), rd_debug_graph_beta_route the variant inside the LDS form (STAGE_V, the backward's chunk).

Every measured error is printed (-s) as `beta64 <kind> <case> <mode>: <tensor> <error>/<bound>, ...`; the last test writes the
maxima per group beside the CPU yardstick to the file RD_BETA64_REPORT names (profiles/beta_operator_float64_errors.json is one)."""
import ctypes
import gc
import json
import os

import numpy as np
import pytest
import torch

from tests import beta_operator_ref as BR
from tests import rng_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0x7FC07FC0                                  # fp32 NaN; as int32 / int64 far outside every legal index
GUARD = 64                                           # elements behind the last legal one
RD_EINVAL, RD_EUNSUPPORTED = -1, -2
LDS_NAMES, V1_NAMES = {"k_graph_beta_fwd2", "k_graph_beta_bwd2"}, {"k_graph_beta_fwd", "k_graph_beta_bwd"}
# test_workspace_form_equals_lds_form holds the two forms' alpha to 1e-7 ABSOLUTE on tests/golden/beta_batched.npz, whose scores have
# max-norm 0.0584.  The scores here reach 2.0, where one fp32 ulp is 2.4e-7: the same bound, stated relative to the max-norm.
FORMS_ALPHA_REL = 1e-7 / 0.0584
_MEASURED = {}                                       # (kind, group, mode, tensor) -> (error, case)


def _L():
    from raindrop_amd import _lib
    return _lib


def _hooks():
    lib = _L().load()
    on, read = lib.rd_debug_launch_log, lib.rd_debug_launch_log_read
    on.argtypes, on.restype = [ctypes.c_int], None
    read.argtypes, read.restype = [ctypes.c_char_p, ctypes.c_size_t], ctypes.c_size_t
    return on, read


@pytest.fixture(autouse=True)
def _process_wide_settings_handed_back(monkeypatch):
    """Before and after each test: split-bf16 arithmetic, launch log off, no seed cell, neither per-call switch set.  A device error
    ends the session: nothing more is started on a GPU that has faulted."""
    on, _ = _hooks()
    _L().call("rd_set_precision", 1)
    _L().call("rd_set_seed_cell", None)
    monkeypatch.delenv("RD_BETA_V1", raising=False)
    monkeypatch.delenv("RD_BETA_LARGE", raising=False)
    try:
        yield
    finally:
        on(0)
        _L().call("rd_set_seed_cell", None)
        _L().call("rd_set_precision", 1)
        try:
            torch.cuda.synchronize()
        except Exception as e:                              # noqa: BLE001 -- any HIP error here is a fault of the device
            pytest.exit("device error after a beta-operator case: %s" % e, returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _hand_back_device_memory():
    """tests/test_step_launches_gpu.py names buffers by the order in which their addresses first appear: leave no garbage behind."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _logged(fn):
    """run fn with the launch log on -> the distinct names the launch sites reported"""
    on, read = _hooks()
    buf = ctypes.create_string_buffer(1 << 12)
    on(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        need = read(buf, len(buf))
        on(0)
    assert need < len(buf)
    return {n for n in buf.value.decode().split("\n") if n}


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _in(a):
    """a host array on the device, followed by a few zeros (so an empty input still has an address)"""
    a = np.ascontiguousarray(a)
    t = torch.zeros(a.size + 4, dtype=torch.from_numpy(a).dtype, device=DEV)
    t[:a.size] = torch.from_numpy(a.reshape(-1)).to(DEV)
    return t


class _Out:
    """n elements of `dtype` + GUARD more, all POISON"""

    def __init__(self, n, dtype=torch.float32):
        self.n = int(n)
        self.t = torch.empty(self.n + GUARD, dtype=dtype, device=DEV)
        self.t.view(torch.int32).fill_(POISON)

    def host(self, *shape):
        return self.t[:self.n].cpu().numpy().reshape(shape)

    def tail_intact(self):
        return bool((self.t[self.n:].view(torch.int32) == POISON).all())

    def untouched(self):
        return bool((self.t.view(torch.int32) == POISON).all())


def _route(c, mode):
    """({names of the set bits}, Tc) of rd_debug_graph_beta_route under the switches of the moment"""
    L = _L()
    bits = ctypes.c_uint32(0)
    L.call("rd_debug_graph_beta_route", c["B"], c["N"], c["T"], c["E"], int(mode != "plain"), int(mode == "drop"), ctypes.byref(bits))
    return {n for i, n in enumerate(L.BETA_ROUTE_BITS) if bits.value >> i & 1}, bits.value >> 8


def _buffers(c):
    B, N, T, K, E, Kk = c["B"], c["N"], c["T"], c["K"], c["E"], c["Kk"]
    lib = _L().load()
    ws_bytes = int(lib.rd_graph_beta_workspace_bytes(B, N, K, T, E))
    o = dict(out=_Out(B * N * K), ei_out=_Out(B * 2 * Kk, torch.int64), alpha=_Out(B * Kk), beta=_Out(B * N * T),
             kept=_Out(B * Kk, torch.int32), dV=_Out(B * N * K), dH=_Out(B * N * T * 32), dmap=_Out(B * N * 16), dw=_Out(B * E),
             ws=_Out(ws_bytes // 4))
    assert ws_bytes % 4 == 0 and o["ws"].t.data_ptr() % 256 == 0
    return o, ws_bytes


def _inputs(c):
    return dict(V=_in(c["V"]), H=_in(c["H"]), map_w=_in(c["map_w"]), p_t=_in(c["p_t"]), ei=_in(c["ei"]), w=_in(c["w"]),
                dout=_in(c["dout"]), dalpha=_in(c["dalpha"]))


def _head(c, i):
    """the arguments every entry point starts with"""
    return [c["B"], c["N"], c["K"], c["T"], BR.D_OB, c["E"], _P(i["V"]), _P(i["H"]), _P(i["map_w"]), _P(i["p_t"]),
            c["T"] * 16 if c["pt_ps"] else 0, _P(i["ei"]), c["E"], _P(i["w"]), c["E"] if c["w_ps"] else 0]


def _fwd_args(c, i, o, mode, ws_ptr, ws_bytes):
    drop = [ctypes.c_float(BR.P_DROP), ctypes.c_uint64(BR.DROP_SEED)] if mode == "drop" else []
    return ("rd_graph_beta_fwd_dropout" if mode == "drop" else "rd_graph_beta_fwd",
            _head(c, i) + drop + [_P(o["out"].t), _P(o["ei_out"].t), _P(o["alpha"].t), _P(o["beta"].t), _P(o["kept"].t), ws_ptr, ws_bytes,
                                  _stream()])


def _bwd_args(c, i, o, mode, ws_ptr, ws_bytes):
    tail = [_P(o["dV"].t), _P(o["dH"].t), _P(o["dmap"].t), _P(o["dw"].t), ws_ptr, ws_bytes, _stream()]
    saved = [_P(o["beta"].t), _P(o["kept"].t), _P(i["dout"])]
    if mode == "plain":
        return "rd_graph_beta_bwd", _head(c, i) + saved + tail
    if mode == "alpha":
        return "rd_graph_beta_bwd_alpha", _head(c, i) + saved + [_P(i["dalpha"])] + tail
    return ("rd_graph_beta_bwd_dropout",
            _head(c, i) + [ctypes.c_float(BR.P_DROP), ctypes.c_uint64(BR.DROP_SEED)] + saved + [_P(i["dalpha"])] + tail)


def _run(name, mode):
    """forward + backward of a case under the switches of the moment -> ({compared tensors as numpy}, launch names)"""
    L = _L()
    c = BR.case(name)
    B, N, T, K, E, Kk = c["B"], c["N"], c["T"], c["K"], c["E"], c["Kk"]
    i = _inputs(c)
    o, ws_bytes = _buffers(c)
    ws_ptr = _P(o["ws"].t)

    def go():
        for n, a in (_fwd_args(c, i, o, mode, ws_ptr, ws_bytes), _bwd_args(c, i, o, mode, ws_ptr, ws_bytes)):
            L.call(n, *a)

    names = _logged(go)
    for k, buf in o.items():
        assert buf.tail_intact(), (name, mode, k, "guard tail overwritten")
    got = dict(out=o["out"].host(B, N, K), ei_out=o["ei_out"].host(B, 2, Kk), alpha=o["alpha"].host(B, Kk), beta=o["beta"].host(B, N, T),
               kept=o["kept"].host(B, Kk), dV=o["dV"].host(B, N, K), dH=o["dH"].host(B, N, T * 32),
               dmap=o["dmap"].host(B, N, 16).astype(np.float64).sum(0), dw=o["dw"].host(B, E))
    got["ws_bytes"] = ws_bytes
    return got, names


def _compare(kind, name, mode, got):
    """print every tensor's error beside its bound, record the maxima, then hold each to its bound and the lists bit for bit"""
    c = BR.case(name)
    rows, lists_ok = BR.compare(name, mode, got)
    print("beta64 %s %s %s: %s" % (kind, name, mode, ", ".join("%s %.2e/%.2e" % r for r in rows)))
    for t, e, _ in rows:
        key = (kind, c["group"], mode, t)
        if key not in _MEASURED or e > _MEASURED[key][0]:
            _MEASURED[key] = (e, name)
    for t in BR.COMPARED:
        assert np.isfinite(got[t]).all(), (name, mode, t, "not finite: an element was never written")
    assert lists_ok, (name, mode, "kept lists differ from the float64 order")
    bad = [r for r in rows if not r[1] <= r[2]]
    assert not bad, (kind, name, mode, bad)
    if c["Kk"] == 0:                                         # nothing kept: exact zeros
        for t in ("out", "dV", "dH", "dmap", "dw"):
            assert not np.asarray(got[t]).any(), (name, t)
    ref = BR.reference(name, mode)
    pruned = np.ones((c["B"], c["E"]), dtype=bool)
    np.put_along_axis(pruned, ref["kept"].astype(np.int64), False, axis=1)
    assert (got["dw"][pruned] == 0).all(), (name, "dw of a pruned edge")


def _assert_form(name, mode, names, form):
    c = BR.case(name)
    bits, tc = _route(c, mode)
    bl = {n for n in names if n.startswith("k_bl_")}
    if form == "workspace":
        assert bl and not (names & (LDS_NAMES | V1_NAMES)), (name, sorted(names))
        assert not ({"fwd_lds", "bwd_lds"} & bits) and tc == 0, (name, bits, tc)
        return
    want = V1_NAMES if form == "v1" else LDS_NAMES
    assert want <= names and not bl and not (names & ((LDS_NAMES | V1_NAMES) - want)), (name, form, sorted(names))
    assert {"fwd_lds", "bwd_lds"} <= bits and (("v1" in bits) == (form == "v1")), (name, bits)
    if form == "v1":
        assert tc == BR.ROUTE_TC_V1.get(name, c["T"]), (name, tc)
        return
    assert tc == BR.ROUTE_TC.get(name, (c["T"],) * 3)[BR.MODES.index(mode)], (name, mode, tc)
    if (name, mode) in BR.RAGGED:
        assert tc < c["T"] and c["T"] % tc, (name, mode, tc)
    if name in BR.STAGE_V:
        assert ("stage_v" in bits) == BR.STAGE_V[name], (name, bits)


# ---- 1. both forms against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", BR.MODES)
@pytest.mark.parametrize("name", BR.LDS_CASES)
def test_lds_form_vs_float64(name, mode):
    got, names = _run(name, mode)
    assert got["ws_bytes"] == 0, (name, "rd_graph_beta_workspace_bytes must be 0 where the LDS form runs")
    _assert_form(name, mode, names, "lds")
    _compare("lds", name, mode, got)


@pytest.mark.parametrize("mode", BR.MODES)
@pytest.mark.parametrize("name", BR.WORKSPACE_CASES)
def test_workspace_form_vs_float64(name, mode):
    got, names = _run(name, mode)
    assert got["ws_bytes"] > 0
    _assert_form(name, mode, names, "workspace")
    _compare("workspace", name, mode, got)


def test_chunk_case_is_the_one_the_host_variant_models():
    """tests/beta_operator_ref.py's skip_chunk_last variant drops step CHUNK_TC - 1: the first pass of the plain backward must end there"""
    assert _route(BR.case(BR.CHUNK_CASE), "plain")[1] == BR.CHUNK_TC


# ---- 2. the same cases on the other form, and the two forms against each other -----------------------------------------------------------
@pytest.mark.parametrize("mode", BR.MODES)
@pytest.mark.parametrize("name", BR.FORCED_LARGE)
def test_forced_workspace_form_vs_float64_and_vs_lds_form(name, mode, monkeypatch):
    """RD_BETA_LARGE=1: the k_bl_* launches on graphs the LDS kernels take; then both forms' outputs against each other under the
    bounds of tests/test_graph_beta_gpu.py::test_workspace_form_equals_lds_form."""
    small, names_s = _run(name, mode)
    _assert_form(name, mode, names_s, "lds")
    monkeypatch.setenv("RD_BETA_LARGE", "1")
    large, names_l = _run(name, mode)
    assert large["ws_bytes"] > 0
    _assert_form(name, mode, names_l, "workspace")
    monkeypatch.delenv("RD_BETA_LARGE")
    _compare("forced-workspace", name, mode, large)
    for t in BR.LISTS:
        assert np.array_equal(small[t], large[t]), t
    assert float(np.abs(small["alpha"] - large["alpha"]).max()) <= FORMS_ALPHA_REL * float(np.abs(small["alpha"]).max())
    assert float(np.abs(small["out"] - large["out"]).max()) <= 2e-6 * float(np.abs(small["out"]).max())
    for t in BR.GRADS:
        assert float(np.abs(small[t] - large[t]).max()) <= 5e-6 * float(np.abs(small[t]).max()) + 1e-9, t


# ---- 3. the rounds 2-5 kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BR.V1_CASES)
def test_rounds_2_to_5_kernels_vs_float64(name, monkeypatch):
    monkeypatch.setenv("RD_BETA_V1", "1")
    got, names = _run(name, "plain")
    _assert_form(name, "plain", names, "v1")
    monkeypatch.delenv("RD_BETA_V1")
    _compare("v1", name, "plain", got)


# ---- 4. the arithmetic mode does not reach this operator ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BR.PRECISION_CASES)
def test_precision_mode_changes_no_bit(name):
    """rd_set_precision (RD_PRECISION) selects the GEMM arithmetic; the operator is scalar fp32 in either mode"""
    runs = []
    for prec in (1, 0):
        _L().call("rd_set_precision", prec)
        got, _ = _run(name, "drop")
        _compare("precision%d" % prec, name, "drop", got)
        runs.append(got)
    for t in BR.COMPARED + BR.LISTS:
        assert np.array_equal(runs[0][t], runs[1][t]), (name, t)


# ---- 5. the mask ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["KK65", "S_WP_PS"])
def test_keep_bytes_equal_the_host_mask(name):
    """rd_graph_beta_keep against tests/rng_ref.py edge_coeff_keep, the seed cell unregistered and registered (seed + cell)"""
    L = _L()
    c = BR.case(name)
    B, E, T = c["B"], c["E"], c["T"]

    def device_keep(seed):
        buf = _Out((B * E * T * 4 + 3) // 4, torch.int32)
        L.call("rd_graph_beta_keep", B, T, E, ctypes.c_float(BR.P_DROP), ctypes.c_uint64(seed), _P(buf.t), _stream())
        torch.cuda.synchronize()
        assert buf.tail_intact()
        return buf.t[:buf.n].view(torch.uint8).cpu().numpy()[:B * E * T * 4].reshape(B, E, T, 4)

    plain = device_keep(BR.DROP_SEED)
    assert np.array_equal(plain, BR.keep_mask(c).astype(np.uint8))
    cell = torch.tensor([5], dtype=torch.int64, device=DEV)
    L.call("rd_set_seed_cell", _P(cell))
    try:
        with_cell = device_keep(BR.DROP_SEED - 5)
        shifted = device_keep(BR.DROP_SEED)
    finally:
        L.call("rd_set_seed_cell", None)
    assert np.array_equal(with_cell, plain)
    assert np.array_equal(shifted, R.edge_coeff_keep(BR.DROP_SEED + 5, B, E, T, BR.P_DROP).astype(np.uint8))
    assert not np.array_equal(shifted, plain)


# ---- 6. refusals: nothing launched, nothing written ----------------------------------------------------------------------------------------
def _refused(c, mutate, want_rc):
    """forward and backward with the workspace arguments changed by `mutate`: both return want_rc, the log stays empty and every
    output keeps its pattern"""
    lib = _L().load()
    i = _inputs(c)
    o, ws_bytes = _buffers(c)
    ws_ptr, ws_b = mutate(o["ws"].t.data_ptr(), ws_bytes)
    rcs = []

    def go():
        n, a = _fwd_args(c, i, o, "plain", ctypes.c_void_p(ws_ptr), ws_b)
        rcs.append(getattr(lib, n)(*a))
        n, a = _bwd_args(c, i, o, "plain", ctypes.c_void_p(ws_ptr), ws_b)
        rcs.append(getattr(lib, n)(*a))

    names = _logged(go)
    assert rcs == [want_rc, want_rc], (rcs, lib.rd_last_error())
    assert not names, sorted(names)
    for k, buf in o.items():
        assert buf.untouched(), k


def test_short_or_misaligned_workspace_is_einval():
    c = BR.case("H_N65")
    _refused(c, lambda p, n: (p, n - 1), RD_EINVAL)
    _refused(c, lambda p, n: (p + 128, n), RD_EINVAL)
    _refused(c, lambda p, n: (0, n), RD_EINVAL)


def test_more_than_1024_nodes_is_unsupported():
    N, E, T, B = BR.REFUSED_N, 40, 4, 1
    rng = np.random.default_rng(0)
    c = dict(N=N, E=E, T=T, B=B, K=4 * T, Kk=E // 2, w_ps=True, pt_ps=True,
             V=rng.random((B, N, 4 * T)).astype(np.float32), H=rng.random((B, N, T, 32)).astype(np.float32),
             map_w=rng.random((N, 16)).astype(np.float32), p_t=rng.random((B, T, 16)).astype(np.float32),
             ei=rng.integers(0, N, size=(2, E)).astype(np.int64), w=rng.random((B, E)).astype(np.float32),
             dout=rng.random((B, N, 4 * T)).astype(np.float32), dalpha=rng.random((B, E // 2)).astype(np.float32))
    assert _L().load().rd_graph_beta_workspace_bytes(B, N, 4 * T, T, E) > 0
    _refused(c, lambda p, n: (p, n), RD_EUNSUPPORTED)
    assert b"1024" in _L().load().rd_last_error()


# ---- 7. the figures ------------------------------------------------------------------------------------------------------------------------
def test_zz_report_measured_errors_beside_the_yardstick():
    """Runs last in the file.  Prints the maximum measured error per (kind, group, mode, tensor) beside the CPU yardstick and the
    bound; with RD_BETA64_REPORT=<path> the same figures go to that file as JSON (profiles/beta_operator_float64_errors.json is one)."""
    if not _MEASURED:                                        # selected alone: nothing to report
        return
    report = {"yardstick": {}, "measured": {}, "fixes": []}
    for group in BR.GROUPS:
        for mode in BR.MODES:
            y = BR.yardstick(group, mode)
            report["yardstick"]["%s/%s" % (group, mode)] = {t: {"error": y[t][0], "case": y[t][1]} for t in BR.COMPARED}
    for (kind, group, mode, t), (e, name) in sorted(_MEASURED.items()):
        report["measured"].setdefault("%s/%s/%s" % (kind, group, mode), {})[t] = {"error": e, "case": name}
        y = BR.yardstick(group, mode)[t][0]
        print("beta64 max %s %s %s %s: %.2e (%s), yardstick %.2e" % (kind, group, mode, t, e, name, y))
    if os.environ.get("RD_BETA64_REPORT"):
        with open(os.environ["RD_BETA64_REPORT"], "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
