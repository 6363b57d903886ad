"""GPU: ONE encoder layer on a registered token plan -- the fused in_proj + attention launches (rd_attnfuse.hip k_attn_fwd_fused /
k_attn_bwd_fused), the lean k_enc_post_fwd / k_enc_pre_bwd chains and the weight-gradient stream fed from row tiles in the plan's
per-sample group space -- against float64, across the envelope in which a layer reaches them: D = 152 / 160 (head_dim 76 / 80: all
five 16-column tiles full), T = 64 (a full tile), T = 7 (< 16), sample lengths 1 and every 16-row group edge, an odd and an even
number of groups, zero-length samples, one sample.  D = 136 / 144, which attnfuse_ok() admits by itself, cannot reach them (the
row-block path needs ceil(3 D / 32) == 15): section 6 pins that a plan refuses those widths loudly.  Cases, inputs, reference and
bounds: tests/plan_layer_ref.py (tests/test_plan_layer_host.py shows on the reference alone that the bounds bite).

The entry points are called through the C-ABI (rd_token_plan, rd_set_token_plan, rd_encoder_layer_fwd / _bwd / _fwd_infer) with x,
y, dy, dx as [T B, D] buffers whose first M_live rows are in plan order.  Every run has the launch log on and asserts the kernels it
is about were reported and the per-(sample, head) attention kernels were not: a case that falls off the fused path fails.

  1. float64 tie (split-bf16, dropout off): y, dx on live rows and all 12 parameter gradients;
  2. read-side guard, in every case of 1: rows >= M_live of x and dy are NaN; saved, workspace, y, dx and the gradients are pre-filled
     with a NaN pattern -- everything compared must be finite and within 1's bounds, and rows >= M_live of y and dx keep the pattern;
  3. RD_ATTN_FUSE=1 against =0 on the same plan, both bf16 modes, dropout off and on;
  4. dropout p = 0.2 against float64 with host-generated masks numbered by plan rows and ranks;
  5. the save-free inference forward equals the training forward bit for bit on live rows;
  6. D = 136 / 144 with a plan registered: RD_EINVAL from every entry point, nothing launched, nothing written.

The yardstick (test_yardstick_meets_the_bounds) is the same inputs on the padded layout with RD_ENC_FUSE=0 and RD_ATTN_FUSE=0 -- the
kernels test_row_block_layer_vs_float64 and test_encoder_layer_vs_oracle tie to float64 -- against the same reference: the only
source of a bound above the project's 2e-4 (tests/plan_layer_ref.py RAISED)."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from oracle import restatement as O2
from tests import dropout_ref as DR
from tests import plan_layer_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0x7FC07FC0                                  # fp32 NaN = a pair of bf16 NaNs
FUSED = {"k_attn_fwd_fused", "k_attn_bwd_fused", "k_enc_post_fwd", "k_enc_pre_bwd"}
_ids = lambda cases: ["%s-%s" % c for c in cases]


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
    """Before and after each test: split-bf16 arithmetic, launch log off, no token plan registered."""
    on, _ = _hooks()
    _L().call("rd_set_precision", 1)
    _L().call("rd_set_token_plan", None)
    try:
        yield
    finally:
        on(0)
        _L().call("rd_set_token_plan", None)
        _L().call("rd_set_precision", 1)


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


def _poisoned_bytes(n):
    t = torch.empty((max(int(n), 256) + 3) // 4 * 4, dtype=torch.uint8, device=DEV)
    t.view(torch.int32).fill_(POISON)
    return t


def _poisoned(*shape):
    t = torch.empty(*shape, dtype=torch.float32, device=DEV)
    t.view(torch.int32).fill_(POISON)
    return t


def _is_poison(t):
    return bool((t.contiguous().view(torch.int32) == POISON).all())


def _rows(c, a):
    """[M_live, D] host rows -> [T B, D] device buffer, rows >= M_live NaN"""
    buf = torch.full((c["T"] * c["B"], c["D"]), float("nan"), device=DEV)
    buf[: a.shape[0]] = torch.from_numpy(a).to(DEV)
    return buf


def _assert_fused(names, tag):
    assert FUSED <= names, (tag, sorted(names))
    assert not any(n.startswith("k_attn_fwd_one") or n == "k_attn_fwd_b16" for n in names), (tag, sorted(names))


def _run_plan(c, mode=1, p_drop=0.0, infer=False):
    """The layer on the plan of c["lengths"], forward + backward (infer: the inference forward alone) -> ({y, x, 12 gradients} on
    live rows as numpy, launch names).  Every buffer the calls write is pre-filled with POISON, every row they must not read is NaN."""
    L = _L()
    lib = L.load()
    T, B, D, ml = c["T"], c["B"], c["D"], c["plan"]["mlive"]
    shp = L.shape(B, T, c["F"], 4, nhead=PR.NHEAD, nhid=c["nhid"])
    sp = ctypes.byref(shp)
    L.call("rd_set_precision", mode)
    lengths = torch.from_numpy(c["lengths"]).to(DEV)
    plan = torch.zeros(max(int(lib.rd_token_plan_bytes(sp)) // 4, 64), dtype=torch.int32, device=DEV)
    L.call("rd_token_plan", sp, _P(lengths), _P(plan), None, 0, _stream())
    x, dy = _rows(c, c["x"]), _rows(c, c["dy"])
    mask = torch.from_numpy(O2.padding_mask(c["lengths"], T)).to(DEV)
    params = [c["p"][n].to(DEV).contiguous() for n in PR.ENC_NAMES]
    grads = [_poisoned(p.shape) for p in params]
    w, g = L.RdEncoderPtrs(*[t.data_ptr() for t in params]), L.RdEncoderPtrs(*[t.data_ptr() for t in grads])
    y, dx = _poisoned(T * B, D), _poisoned(T * B, D)
    ws = _poisoned_bytes(lib.rd_encoder_layer_workspace_bytes(sp))
    saved = _poisoned_bytes(lib.rd_encoder_layer_infer_bytes(sp) if infer else lib.rd_encoder_layer_saved_bytes(sp))

    def go():
        L.call("rd_set_token_plan", _P(plan))
        try:
            if infer:
                L.call("rd_encoder_layer_fwd_infer", sp, PR.LAYER, _P(x), _P(mask), ctypes.byref(w), _P(y), _P(saved), saved.numel(),
                       _P(ws), ws.numel(), _stream())
                return
            L.call("rd_encoder_layer_fwd", sp, PR.LAYER, _P(x), _P(mask), ctypes.byref(w), float(p_drop), PR.SEED, _P(y), _P(saved),
                   saved.numel(), _P(ws), ws.numel(), _stream())
            L.call("rd_encoder_layer_bwd", sp, PR.LAYER, _P(x), _P(mask), ctypes.byref(w), float(p_drop), PR.SEED, _P(saved),
                   saved.numel(), _P(dy), _P(dx), ctypes.byref(g), _P(ws), ws.numel(), _stream())
        finally:
            L.call("rd_set_token_plan", None)

    names = _logged(go)
    h = plan.cpu().numpy()
    assert h[0] == ml and np.array_equal(h[8:8 + B + 1], c["plan"]["off"]) and np.array_equal(h[9 + B:9 + 2 * B], c["plan"]["rank"])
    assert _is_poison(y[ml:]), "y: rows >= M_live written"
    got = dict(y=y[:ml].cpu().numpy())
    if not infer:
        assert _is_poison(dx[ml:]), "dx: rows >= M_live written"
        got["x"] = dx[:ml].cpu().numpy()
        got.update((n, t.cpu().numpy()) for n, t in zip(PR.ENC_NAMES, grads))
    return got, names


def _run_padded(c, p_drop, monkeypatch):
    """The yardstick: the samples of non-zero length on the padded layout through the row-block launches and the per-(sample, head)
    attention kernels (RD_ENC_FUSE=0, RD_ATTN_FUSE=0), results gathered into plan order."""
    from raindrop_amd import ops
    monkeypatch.setenv("RD_ENC_FUSE", "0")
    monkeypatch.setenv("RD_ATTN_FUSE", "0")
    T, Lg, pl = c["T"], c["lengths"], c["plan"]
    keep = np.nonzero(Lg > 0)[0]
    st, Lk = PR.starts_of(pl)[keep], Lg[keep]
    xd = torch.from_numpy(PR.to_padded(c["x"], PR.starts_of(pl), Lg, T)[:, keep]).to(DEV).contiguous().requires_grad_(True)
    dyd = torch.from_numpy(PR.to_padded(c["dy"], PR.starts_of(pl), Lg, T)[:, keep]).to(DEV).contiguous()
    mask = torch.from_numpy(O2.padding_mask(Lk, T)).to(DEV)
    pd = [c["p"][n].to(DEV).requires_grad_(True) for n in PR.ENC_NAMES]
    shp = _L().shape(len(keep), T, c["F"], 4, nhead=PR.NHEAD, nhid=c["nhid"])
    out = {}

    def go():
        y = ops.encoder_layer(xd, mask, shp, PR.LAYER, p_drop, PR.SEED, pd)
        g = torch.autograd.grad(y, [xd] + pd, dyd)
        out["y"] = PR.to_plan(y.detach().cpu().numpy(), st, Lk, pl["mlive"])
        out["x"] = PR.to_plan(g[0].cpu().numpy(), st, Lk, pl["mlive"])
        out.update((n, t.cpu().numpy()) for n, t in zip(PR.ENC_NAMES, g[1:]))

    names = _logged(go)
    assert not (FUSED & names) and "k_attn_fwd_one_b16w" in names, sorted(names)
    return out


def _compare(tag, got, ref, bound_of):
    """print every tensor's error (y: max absolute; gradients: of the max-norm), then hold each to its bound"""
    bad, figs = [], []
    for name in ("y",) + PR.GRAD_NAMES:
        a, r = got[name].astype(np.float64), ref[name]
        assert a.shape == r.shape, (tag, name, a.shape, r.shape)
        metric, bound = bound_of(name)
        e = float(np.abs(a - r).max()) if metric == "abs" else DR.rel(a, r)
        figs.append("%s %.2e" % (name, e))
        if not (np.isfinite(a).all() and e <= bound):
            bad.append((name, e, bound))
    print("%s: %s" % (tag, ", ".join(figs)))
    assert not bad, (tag, bad)


def _env(c, monkeypatch):
    if c["env"]:
        monkeypatch.setenv(*c["env"].split("="))


# ---- 1 + 2. float64 tie with the read-side guard -----------------------------------------------------------------------------------
LIVE_CASES = [cs for cs in PR.TIE_CASES if cs[1] != "Z33"]


@pytest.mark.parametrize("width,lset", LIVE_CASES, ids=_ids(LIVE_CASES))
def test_plan_layer_vs_float64(width, lset, monkeypatch):
    c = PR.case(width, lset)
    _env(c, monkeypatch)
    got, names = _run_plan(c)
    _assert_fused(names, (width, lset))
    _compare("plan %s %s" % (width, lset), got, PR.reference(width, lset), PR.bound_of)


@pytest.mark.parametrize("width", ["W152", "W160"])
def test_zero_length_samples_vs_float64(width, monkeypatch):
    """Z33: lengths (33, 0, 20, 0) -- rd_plan.h clamps lengths to [0, T], so 0 is a legal input.  The reference holds the two live
    samples only: a zero-length sample owns no row and contributes to no gradient (its workgroups return at once; the group space
    ends with the length-20 sample on an odd group, whose owner zeroes the unowned half chunk)."""
    c = PR.case(width, "Z33")
    got, names = _run_plan(c)
    _assert_fused(names, (width, "Z33"))
    _compare("plan %s Z33" % width, got, PR.reference(width, "Z33"), PR.bound_of)


@pytest.mark.parametrize("width,lset", PR.TIE_CASES, ids=_ids(PR.TIE_CASES))
def test_yardstick_meets_the_bounds(width, lset, monkeypatch):
    """The padded unfused path on the same inputs against the same reference: what every bound above 2e-4 is derived from."""
    c = PR.case(width, lset)
    _compare("yardstick %s %s" % (width, lset), _run_padded(c, 0.0, monkeypatch), PR.reference(width, lset), PR.bound_of)


# ---- 3. the fused attention launch against the launches it replaces, on the same plan ---------------------------------------------
FUSE_CASES = [(w, s) for w in ("W152", "W160") for s in ("G64", "S7")]
FUSE_BOUNDS = {1: (2e-6, 2e-5),          # test_fused_attention_launch_vs_the_three_launches_it_replaces
               2: (2e-5, 1e-3)}          # test_token_plan_beyond_the_p19_envelope, single-product mode


@pytest.mark.parametrize("p_drop", [0.0, PR.P_DROP])
@pytest.mark.parametrize("mode", [1, 2], ids=["bf16x3", "bf16"])
@pytest.mark.parametrize("width,lset", FUSE_CASES, ids=_ids(FUSE_CASES))
def test_fused_attention_vs_the_launches_it_replaces_on_the_plan(width, lset, mode, p_drop, monkeypatch):
    """RD_ATTN_FUSE=1 against =0 (in_proj row-block product, attention per (rank, head), in_proj input-gradient product) on the same
    plan, seed and masks; mode 2 runs the ONE = true instantiations."""
    c = PR.case(width, lset)
    got1, names1 = _run_plan(c, mode, p_drop)
    _assert_fused(names1, (width, lset, mode))
    monkeypatch.setenv("RD_ATTN_FUSE", "0")
    got0, names0 = _run_plan(c, mode, p_drop)
    assert not ({"k_attn_fwd_fused", "k_attn_bwd_fused"} & names0) and {"k_attn_fwd_one_b16w", "k_enc_post_fwd", "k_enc_pre_bwd"} <= names0, \
        sorted(names0)
    ytol, gtol = FUSE_BOUNDS[mode]
    _compare("fused vs unfused %s %s mode %d p %.1f" % (width, lset, mode, p_drop), got1, {k: v.astype(np.float64) for k, v in got0.items()},
             lambda name: ("abs", ytol) if name == "y" else ("rel", gtol))


# ---- 4. dropout against float64 with host masks -------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,lset", PR.DROPOUT_CASES, ids=_ids(PR.DROPOUT_CASES))
def test_plan_layer_dropout_vs_float64(width, lset):
    """p = 0.2: the four masks of the layer numbered by plan rows (row-local sites) and by rank (attention probabilities), applied
    through the drop= hook of the float64 restatement."""
    c = PR.case(width, lset)
    got, names = _run_plan(c, 1, PR.P_DROP)
    _assert_fused(names, (width, lset))
    _compare("plan dropout %s %s" % (width, lset), got, PR.reference(width, lset, PR.P_DROP), PR.bound_of)


@pytest.mark.parametrize("width,lset", PR.DROPOUT_CASES, ids=_ids(PR.DROPOUT_CASES))
def test_dropout_yardstick_meets_the_bounds(width, lset, monkeypatch):
    """The padded unfused path under ITS masks (numbered by padded rows and samples) against its own masked reference."""
    c = PR.case(width, lset)
    _compare("yardstick dropout %s %s" % (width, lset), _run_padded(c, PR.P_DROP, monkeypatch),
             PR.reference(width, lset, PR.P_DROP, None, "padded"), PR.bound_of)


# ---- 5. save-free inference forward -------------------------------------------------------------------------------------------------
INFER_CASES = [(w, s) for w in PR.PLAN_WIDTHS for s in ("G64", "S7", "ONE64", "ONE1")]


@pytest.mark.parametrize("width,lset", INFER_CASES, ids=_ids(INFER_CASES))
def test_inference_forward_equals_training_forward_on_the_plan(width, lset, monkeypatch):
    """rd_encoder_layer_fwd_infer on the plan, buffer sized by rd_encoder_layer_infer_bytes: y bit-identical to the training
    forward's at p = 0 on live rows.  Where rd_infer_covers reports the encoder (the 152 / 272 widths) the log names the save-free
    instantiations; at 160 / 288, which has none, the entry point is the saving forward into a buffer of the training size, and must
    give the same y through the fused launches."""
    c = PR.case(width, lset)
    _env(c, monkeypatch)
    L = _L()
    shp = L.shape(c["B"], c["T"], c["F"], 4, nhead=PR.NHEAD, nhid=c["nhid"])
    enc = ctypes.c_int32(-1)
    L.call("rd_infer_covers", ctypes.byref(shp), None, ctypes.byref(enc))
    assert enc.value == (1 if width == "W152" else 0)
    train, names_t = _run_plan(c)
    _assert_fused(names_t, (width, lset))
    infer, names = _run_plan(c, infer=True)
    if enc.value:
        assert {"k_attn_fwd_fused<save-free>", "k_enc_post_infer"} <= names and not ({"k_attn_fwd_fused", "k_enc_post_fwd"} & names), \
            sorted(names)
    else:
        assert {"k_attn_fwd_fused", "k_enc_post_fwd"} <= names, sorted(names)
    assert not any(n.startswith("k_attn_fwd_one") or n == "k_attn_fwd_b16" for n in names), sorted(names)
    assert np.isfinite(infer["y"]).all() and np.array_equal(infer["y"], train["y"])


# ---- 6. widths the plan refuses -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("specialize", [None, "0"], ids=["default", "RD_ENC_SPECIALIZE=0"])
@pytest.mark.parametrize("width,lset", PR.REFUSED_CASES, ids=_ids(PR.REFUSED_CASES))
def test_widths_outside_the_row_block_envelope_are_refused_on_a_plan(width, lset, specialize, monkeypatch):
    """D = 136 / 144 (head_dim 68 / 72) pass attnfuse_ok() and, under RD_ENC_SPECIALIZE=0, encfuse_ok() -- but in_proj's input
    gradient (K = 3 D: 13 / 14 reduction chunks) has no row-block kernel, so the layer is not on the row-block + tile-stream path and
    no plan-aware kernel exists for it.  With a plan registered every entry point must say so (RD_EINVAL, "token plan") before it
    launches or writes anything -- never run the padded kernels on plan-ordered rows."""
    from raindrop_amd._lib import RaindropHipError
    assert PR.in_proj_chunks(width) in (13, 14) and all(PR.in_proj_chunks(w) == 15 for w in PR.PLAN_WIDTHS)
    if specialize is not None:
        monkeypatch.setenv("RD_ENC_SPECIALIZE", specialize)
    L = _L()
    lib = L.load()
    c = PR.case(width, lset)
    T, B, D = c["T"], c["B"], c["D"]
    shp = L.shape(B, T, c["F"], 4, nhead=PR.NHEAD, nhid=c["nhid"])
    sp = ctypes.byref(shp)
    lengths = torch.from_numpy(c["lengths"]).to(DEV)
    plan = torch.zeros(max(int(lib.rd_token_plan_bytes(sp)) // 4, 64), dtype=torch.int32, device=DEV)
    L.call("rd_token_plan", sp, _P(lengths), _P(plan), None, 0, _stream())
    x, dy = _rows(c, c["x"]), _rows(c, c["dy"])
    mask = torch.from_numpy(O2.padding_mask(c["lengths"], T)).to(DEV)
    params = [c["p"][n].to(DEV).contiguous() for n in PR.ENC_NAMES]
    grads = [_poisoned(p.shape) for p in params]
    w, g = L.RdEncoderPtrs(*[t.data_ptr() for t in params]), L.RdEncoderPtrs(*[t.data_ptr() for t in grads])
    y, dx = _poisoned(T * B, D), _poisoned(T * B, D)
    ws = _poisoned_bytes(lib.rd_encoder_layer_workspace_bytes(sp))
    saved = _poisoned_bytes(lib.rd_encoder_layer_saved_bytes(sp))
    enc = ctypes.c_int32(-1)
    L.call("rd_infer_covers", sp, None, ctypes.byref(enc))
    assert enc.value == 0 and lib.rd_encoder_layer_infer_bytes(sp) == lib.rd_encoder_layer_saved_bytes(sp)
    calls = [("rd_encoder_layer_fwd", (sp, PR.LAYER, _P(x), _P(mask), ctypes.byref(w), 0.0, PR.SEED, _P(y), _P(saved), saved.numel(), _P(ws),
                                       ws.numel(), _stream())),
             ("rd_encoder_layer_fwd_infer", (sp, PR.LAYER, _P(x), _P(mask), ctypes.byref(w), _P(y), _P(saved), saved.numel(), _P(ws),
                                             ws.numel(), _stream())),
             ("rd_encoder_layer_bwd", (sp, PR.LAYER, _P(x), _P(mask), ctypes.byref(w), 0.0, PR.SEED, _P(saved), saved.numel(), _P(dy),
                                       _P(dx), ctypes.byref(g), _P(ws), ws.numel(), _stream()))]

    def go():
        L.call("rd_set_token_plan", _P(plan))
        try:
            for name, args in calls:
                with pytest.raises(RaindropHipError, match="RD_EINVAL.*token plan"):
                    L.call(name, *args)
        finally:
            L.call("rd_set_token_plan", None)

    names = _logged(go)
    assert not names, sorted(names)
    assert all(_is_poison(t) for t in [y, dx, ws, saved] + grads)
