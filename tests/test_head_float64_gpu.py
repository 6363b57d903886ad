"""GPU: the fused classifier head (rd_head.hip: the four k_head_rows instantiations and k_head_wgrad, through rd_head_train,
rd_head_train_crit, rd_head_forward and rd_head_backward of the C-ABI) against float64 across its envelope -- the instantiation edge
at dh = 192 / 193, dh = 256, the lane-slot and row edges, T = 1 .. 600 (the masked mean's later passes), B = 1 .. 513 (k_head_wgrad's
256-row chunks), C = 1 .. 16 with C dh up to 4096 (the w2 tail loop), the static embedding in LDS and in place with one and two
k-tiles in its weight job, the token plan with ties, zero lengths, one sample and the wide widths, and the criterion with 1024 / 1025
labels, an absent class and a class of weight zero.  Cases, inputs, reference and bounds: tests/head_ref.py
(tests/test_head_ref_host.py shows on the reference alone that the gates are decisive in every case and that the bounds bite).

Every run has the launch log on; every output and the workspace are pre-filled with a NaN pattern and followed by a guard tail of the
same pattern that must survive; on the plan r's rows >= M_live are NaN and dr's must keep the pattern.  The log must name the
instantiation tests/head_ref.py expects and rd_debug_head_route must agree with it.

Every measured error is printed (-s) as `head64 <kind> <case> <form>: <tensor> <error>/<yardstick> = <ratio>, ...`; the last test writes
the maxima per group to the file RD_HEAD64_REPORT names (profiles/head_float64_errors.json is one)."""
import ctypes
import gc
import json
import os

import numpy as np
import pytest
import torch

from tests import head_ref as HR
from tests.helpers import plan_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0x7FC07FC0                                  # fp32 NaN
GUARD = 64                                           # elements behind the last legal one
OUTPUTS = ("loss", "logits") + HR.GRADS
_MEASURED = {}                                       # (kind, group, form, tensor) -> (error, yardstick, case)


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
def _process_wide_settings_handed_back():
    """Before and after each test: split-bf16 arithmetic, launch log off, no token plan, trailing launches immediate.  A device error
    ends the session: nothing more is started on a GPU that has faulted."""
    on, _ = _hooks()
    _L().call("rd_set_precision", 1)
    _L().call("rd_set_token_plan", None)
    _L().call("rd_set_defer_trailing", 0)
    try:
        yield
    finally:
        on(0)
        _L().call("rd_set_defer_trailing", 0)
        _L().call("rd_set_token_plan", None)
        _L().call("rd_set_precision", 1)
        try:
            torch.cuda.synchronize()
        except Exception as e:                              # noqa: BLE001 -- any HIP error here is a fault of the device
            pytest.exit("device error after a head case: %s" % e, returncode=3)


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
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _in(a):
    """a host array on the device (None where it is empty: the head takes no static block at Fe = 0)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a).to(DEV) if a.size else None


class _Out:
    """n elements of fp32 + GUARD more, all POISON; `used` <= n: the elements the call may write"""

    def __init__(self, n, used=None):
        self.n, self.used = int(n), int(n if used is None else used)
        self.t = torch.empty(self.n + GUARD, dtype=torch.float32, device=DEV)
        self.t.view(torch.int32).fill_(POISON)

    def host(self, *shape):
        return self.t[:self.used].cpu().numpy().reshape(shape)

    def tail_intact(self):
        return bool((self.t[self.used:].view(torch.int32) == POISON).all())


def _route(c, mode, crit):
    L = _L()
    words, name = (ctypes.c_uint32 * 11)(), ctypes.create_string_buffer(64)
    L.call("rd_debug_head_route", mode, c["B"], c["D"], c["ds"], c["Fe"], c["C"], int(crit), words, name, len(name))
    return name.value.decode(), list(words)


class _Case:
    """the device side of one case: inputs, the plan where the case has one, fresh poisoned outputs per call"""

    def __init__(self, name, y=None):
        L = _L()
        self.c = c = HR.case(name)
        T, B, D = c["T"], c["B"], c["D"]
        self.shp = L.shape(B, T, 1, 4)
        self.plan, self.ml = None, T * B
        r = c["r"].reshape(T * B, D)
        if c["layout"] == "plan":
            p = plan_ref(c["lengths"], T)
            self.ml = p["mlive"]
            r = np.full((T * B, D), np.nan, dtype=np.float32)            # rows >= M_live: nothing may read them into a result
            r[:self.ml] = HR.rows_of(c, c["r"])
            lengths = torch.from_numpy(c["lengths"]).to(DEV)
            self.plan = torch.zeros(max(int(L.load().rd_token_plan_bytes(ctypes.byref(self.shp))) // 4, 64), dtype=torch.int32, device=DEV)
            L.call("rd_token_plan", ctypes.byref(self.shp), _P(lengths), _P(self.plan), None, 0, _stream())
            torch.cuda.synchronize()
            h = self.plan.cpu().numpy()
            assert h[0] == self.ml and np.array_equal(h[8:8 + B + 1], p["off"]) and np.array_equal(h[9 + B:9 + 2 * B], p["rank"])
        mask = (~HR.keep_of(c["lengths"], T)).T.astype(np.uint8)
        self.i = dict(r=_in(r), mask=_in(mask), lengths=_in(c["lengths"]), stat=_in(c["stat"]), emb_w=_in(c["emb_w"]), emb_b=_in(c["emb_b"]),
                      w0=_in(c["w0"]), b0=_in(c["b0"]), w2=_in(c["w2"]), b2=_in(c["b2"]), y=_in(c["y"] if y is None else y),
                      crit=_in(c["crit"]), dlog_in=_in(c["dlog_in"]))
        self.ws_bytes = int(L.load().rd_head_train_workspace_bytes(B, c["dh"], c["C"]))
        assert self.ws_bytes % 4 == 0

    def outputs(self):
        c = self.c
        T, B, D, Fe, ds, C, dh = (c[k] for k in ("T", "B", "D", "Fe", "ds", "C", "dh"))
        o = dict(loss=_Out(1), logits=_Out(B * C), dr=_Out(T * B * D, self.ml * D), dW0=_Out(dh * dh), db0=_Out(dh), dW2=_Out(C * dh),
                 db2=_Out(C), demb_w=_Out(Fe * ds), demb_b=_Out(Fe), ws=_Out(self.ws_bytes // 4))
        assert o["dr"].t.data_ptr() % 16 == 0 and self.i["r"].data_ptr() % 16 == 0
        return o

    def call(self, entry, o, dlog_in=None, after=None):
        """one entry point on fresh outputs `o` -> the launch names"""
        L, c, i = _L(), self.c, self.i
        head = [ctypes.byref(self.shp), c["D"], c["ds"], c["Fe"], c["C"]] + [_P(i[k]) for k in ("r", "mask", "lengths", "stat", "emb_w", "emb_b",
                                                                                          "w0", "b0", "w2", "b2")]
        emb = [_P(o["demb_w"].t) if c["Fe"] else None, _P(o["demb_b"].t) if c["Fe"] else None]
        grads = emb + [_P(o[k].t) for k in ("dW0", "db0", "dW2", "db2", "dr")]
        tail = [_P(o["ws"].t), self.ws_bytes, _stream()]
        if entry == "rd_head_train":
            args = head + [_P(i["y"]), _P(o["loss"].t), _P(o["logits"].t)] + grads + tail
        elif entry == "rd_head_train_crit":
            args = head + [_P(i["y"]), _P(i["crit"]), _P(o["loss"].t), _P(o["logits"].t)] + grads + tail
        elif entry == "rd_head_forward":
            args = head + [_P(o["logits"].t)] + tail
        else:
            args = head + [_P(i["dlog_in"] if dlog_in is None else dlog_in)] + grads + tail

        def go():
            L.call("rd_set_token_plan", _P(self.plan))
            try:
                L.call(entry, *args)
                if after:
                    after()
            finally:
                L.call("rd_set_token_plan", None)

        names = _logged(go)
        for k, buf in o.items():
            assert buf.tail_intact(), (c["name"], entry, k, "guard tail (or a row >= M_live) overwritten")
        return names

    def host(self, o, which=OUTPUTS):
        c = self.c
        shapes = dict(loss=(), logits=(c["B"], c["C"]), dr=(self.ml, c["D"]) if self.plan is not None else (c["T"], c["B"], c["D"]),
                      dW0=(c["dh"], c["dh"]), db0=(c["dh"],), dW2=(c["C"], c["dh"]), db2=(c["C"],), demb_w=(c["Fe"], c["ds"]), demb_b=(c["Fe"],))
        return {k: o[k].host(*shapes[k]) for k in which}

    def own_dlogits(self, o):
        """d loss / d logits as rd_head_train left them in the workspace (rd_head.hip head_launch: feat | hid | dhid | demb, each
        [B, dh], then dlog [B, C], then the per-sample losses)"""
        c = self.c
        off = 4 * c["B"] * c["dh"]
        return o["ws"].t[off:off + c["B"] * c["C"]].clone()


def _assert_form(c, names, mode, crit, wgrad=True):
    want = HR.instantiation(c, crit)
    rows = {n for n in names if n.startswith("k_head_rows")}
    assert rows == {want}, (c["name"], sorted(names), want)
    assert ("k_head_wgrad" in names) == wgrad, (c["name"], sorted(names))
    name, words = _route(c, mode, crit)
    assert name == want and bool(words[0] & 1) == (c["dh"] <= HR.NARROW_DH) and bool(words[0] & 2) == crit, (c["name"], name, words)
    assert bool(words[0] & 4) == (0 < c["Fe"] * c["ds"] <= 1024 and c["ds"] <= 64) and words[2] == c["B"], (c["name"], words)


def _compare(kind, name, form, got):
    """print every tensor's error beside its yardstick, record the maxima, then hold each to its bound and the exact zeros"""
    c = HR.case(name)
    rows, nonzero = HR.compare(name, form, got)
    print("head64 %s %s %s: %s" % (kind, name, form, ", ".join("%s %.2e/%.2e = %.2f" % (t, e, y, e / y if y else 0.0) for t, e, _, y in rows)))
    for t, e, _, y in rows:
        key = (kind, c["group"], form, t)
        if key not in _MEASURED or e > _MEASURED[key][0]:
            _MEASURED[key] = (e, y, name)
    for t in HR.tensors_of(form):
        assert np.isfinite(got[t]).all(), (name, form, t, "not finite: an element was never written")
    bad = [(t, e, b) for t, e, b, _ in rows if not e <= b]
    assert not bad, (kind, name, form, bad)
    assert not nonzero, (name, form, nonzero, "not exactly zero where the reference is")


def _same_bits(a, b, which):
    return [k for k in which if a[k].tobytes() != b[k].tobytes()]


# ---- 1. every case against float64 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HR.ALL_CASES)
def test_head_train_vs_float64(name):
    k = _Case(name)
    o = k.outputs()
    names = k.call("rd_head_train", o)
    _assert_form(k.c, names, 0, False)
    _compare("train", name, "plain", k.host(o))


@pytest.mark.parametrize("name", HR.CRIT_CASES)
def test_head_train_crit_vs_float64(name):
    k = _Case(name)
    o = k.outputs()
    names = k.call("rd_head_train_crit", o)
    _assert_form(k.c, names, 0, True)
    _compare("crit", name, "crit", k.host(o))


@pytest.mark.parametrize("name", HR.COT_CASES)
def test_head_backward_vs_float64_under_a_random_cotangent(name):
    k = _Case(name)
    o = k.outputs()
    names = k.call("rd_head_backward", o)
    _assert_form(k.c, names, 2, False)
    assert not o["loss"].t.isfinite().any() and not o["logits"].t.isfinite().any()          # neither is an output of this entry point
    _compare("backward", name, "cot", k.host(o, HR.GRADS))


@pytest.mark.parametrize("name", ["DH193", "PLAN_ZEROS", "T65"])
def test_zero_cotangent_gives_exact_zeros(name):
    k = _Case(name)
    o = k.outputs()
    k.call("rd_head_backward", o, dlog_in=torch.zeros(k.c["B"] * k.c["C"], device=DEV))
    got = k.host(o, HR.GRADS)
    assert all(not got[t].any() for t in HR.GRADS), [t for t in HR.GRADS if got[t].any()]


# ---- 2. the entry points against each other, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HR.ALL_CASES)
def test_entry_points_agree_bit_for_bit(name):
    """rd_head_forward's logits are rd_head_train's; rd_head_backward under rd_head_train's own dlogits (read from the workspace)
    gives its dr and six gradients; a second rd_head_train gives the first one's bits"""
    k = _Case(name)
    o = k.outputs()
    k.call("rd_head_train", o)
    train = k.host(o)
    f = k.outputs()
    names = k.call("rd_head_forward", f)
    _assert_form(k.c, names, 1, False, wgrad=False)
    assert not _same_bits(train, k.host(f, ("logits",)), ("logits",))
    assert all(not f[t].t.isfinite().any() for t in f if t not in ("logits", "ws")), "rd_head_forward wrote more than the logits"
    b = k.outputs()
    k.call("rd_head_backward", b, dlog_in=k.own_dlogits(o))
    assert not _same_bits(train, k.host(b, HR.GRADS), HR.GRADS), _same_bits(train, k.host(b, HR.GRADS), HR.GRADS)
    again = k.outputs()
    k.call("rd_head_train", again)
    assert not _same_bits(train, k.host(again), OUTPUTS), _same_bits(train, k.host(again), OUTPUTS)


@pytest.mark.parametrize("name", HR.ORDER_CASES)
def test_criterion_launches_repeat_their_bits(name):
    k = _Case(name)
    runs = []
    for _ in range(2):
        o = k.outputs()
        k.call("rd_head_train_crit", o)
        runs.append(k.host(o))
    assert not _same_bits(runs[0], runs[1], OUTPUTS)


def test_deferred_trailing_form_equals_the_immediate_one():
    """rd_set_defer_trailing(1): rd_head_train parks its weight-gradient launch, rd_flush_trailing runs it"""
    L = _L()
    k = _Case(HR.DEFER_CASE)
    o = k.outputs()
    k.call("rd_head_train", o)
    now = k.host(o)
    d = k.outputs()
    L.call("rd_set_defer_trailing", 1)
    try:
        names = k.call("rd_head_train", d, after=lambda: L.call("rd_flush_trailing", _stream()))
    finally:
        L.call("rd_set_defer_trailing", 0)
    _assert_form(k.c, names, 0, False)
    _compare("deferred", HR.DEFER_CASE, "plain", k.host(d))
    assert not _same_bits(now, k.host(d), OUTPUTS)


def test_precision_mode_changes_no_bit():
    """rd_set_precision selects the GEMM arithmetic; the head is fp32 FMA in every mode"""
    k = _Case(HR.PRECISION_CASE)
    runs = []
    for prec in (1, 0):
        _L().call("rd_set_precision", prec)
        o = k.outputs()
        k.call("rd_head_train", o)
        _compare("precision%d" % prec, HR.PRECISION_CASE, "plain", k.host(o))
        runs.append(k.host(o))
    assert not _same_bits(runs[0], runs[1], OUTPUTS)


# ---- 3. a label outside [0, C) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,form", [("rd_head_train", "plain"), ("rd_head_train_crit", "crit")])
def test_bad_label_gives_a_nan_loss_and_the_next_launch_is_clean(entry, form):
    name = "C2"
    c = HR.case(name)
    y = c["y"].copy()
    y[2] = c["C"]
    k = _Case(name, y=y)
    o = k.outputs()
    k.call(entry, o)
    got = k.host(o)
    assert np.isnan(got["loss"]) and np.isfinite(got["logits"]).all()
    assert HR.error_of("logits", got["logits"], HR.reference(name, form)["logits"]) <= HR.bound_of(name, form, "logits")
    k2 = _Case(name)
    o2 = k2.outputs()
    k2.call(entry, o2)
    _compare("after-bad-label", name, form, k2.host(o2))


# ---- 4. the figures ------------------------------------------------------------------------------------------------------------------------
def test_zz_report_measured_errors_beside_the_yardstick():
    """Runs last in the file.  Prints the maximum measured error per (kind, group, form, tensor) beside the CPU yardstick of the case
    that gave it; with RD_HEAD64_REPORT=<path> the same figures go to that file as JSON (profiles/head_float64_errors.json is one)."""
    if not _MEASURED:                                        # selected alone: nothing to report
        return
    report = {"measured": {}, "kernel_fixes": []}
    for (kind, group, form, t), (e, y, name) in sorted(_MEASURED.items()):
        report["measured"].setdefault("%s/%s/%s" % (kind, group, form), {})[t] = {
            "error": e, "yardstick": y, "bound": HR.bound_of(name, form, t), "case": name}
        print("head64 max %s %s %s %s: %.2e (%s), yardstick %.2e" % (kind, group, form, t, e, name, y))
    if os.environ.get("RD_HEAD64_REPORT"):
        with open(os.environ["RD_HEAD64_REPORT"], "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
