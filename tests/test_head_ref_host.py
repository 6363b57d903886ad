"""CPU: conditions on tests/head_ref.py alone -- the float64 reference of the fused classifier head agrees with torch float64 autograd
in all three loss forms on both layouts and with a central finite difference; every case's ReLU gates keep the margin; every bound is
finite and positive; each wrong-kernel variant misses a bound by more than 10 x on the case the table names for its branch.  Then what
rd_head.hip decides before any launch: the refusals (no device needed: the checks precede every launch) and rd_debug_head_route
against a table written out by hand."""
import ctypes
import os

import numpy as np
import pytest
import torch

from raindrop_amd import _lib, build
from tests import head_ref as HR

RD_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


# ---- 1. the reference against torch autograd and a finite difference ------------------------------------------------------------------------
def _torch_chain(c, form):
    """the head as torch float64 operators on the padded layout -> (loss or None, logits, {gradient name: array})"""
    T, B, D, Fe, C = c["T"], c["B"], c["D"], c["Fe"], c["C"]
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_(True)
    r, emb_w, emb_b, w0, b0, w2, b2 = (t64(c[k]) for k in ("r", "emb_w", "emb_b", "w0", "b0", "w2", "b2"))
    stat, y = torch.from_numpy(c["stat"].astype(np.float64)), torch.from_numpy(c["y"])
    lengths = torch.from_numpy(c["lengths"])
    keep = (torch.arange(T)[:, None] < lengths[None, :]).double().unsqueeze(-1)
    agg = (r * keep).sum(0) / (lengths.double() + 1).unsqueeze(-1)
    feat = torch.cat([agg, stat @ emb_w.t() + emb_b], 1) if Fe else agg
    logits = torch.relu(feat @ w0.t() + b0) @ w2.t() + b2
    if form == "plain":
        loss = torch.nn.functional.cross_entropy(logits, y)
    elif form == "crit":
        crit = torch.from_numpy(c["crit"].astype(np.float64))
        loss = torch.nn.CrossEntropyLoss(weight=crit[1:], label_smoothing=float(c["crit"][0].astype(np.float64)))(logits, y)
    else:
        loss = (logits * torch.from_numpy(c["dlog_in"].astype(np.float64))).sum()
    wrt = dict(dr=r, dW0=w0, db0=b0, dW2=w2, db2=b2)
    if Fe:
        wrt.update(demb_w=emb_w, demb_b=emb_b)
    g = dict(zip(wrt, (t.numpy() for t in torch.autograd.grad(loss, list(wrt.values())))))
    if not Fe:
        g.update(demb_w=np.zeros((0, c["ds"])), demb_b=np.zeros(0))
    if c["layout"] == "plan":
        g["dr"] = HR.rows_of(c, g["dr"])
    return (None if form == "cot" else float(loss.detach())), logits.detach().numpy(), g


@pytest.mark.parametrize("form", HR.FORMS)
@pytest.mark.parametrize("name", ["DH17", "T65", "DH4", "EMB_DS17", "PLAN_TIES", "PLAN_ZEROS", "CRIT_ABSENT", "CRIT_W0", "C1", "B1"])
def test_reference_agrees_with_torch_float64_autograd(name, form):
    c = HR.case(name)
    ref = HR.evaluate(c, form)
    loss, logits, g = _torch_chain(c, form)
    if form != "cot":
        assert abs(float(ref["loss"]) - loss) <= 1e-13 * max(1.0, abs(loss))
    assert np.abs(ref["logits"] - logits).max() <= 1e-13 * max(1.0, np.abs(logits).max())
    for t in HR.GRADS:
        assert ref[t].shape == g[t].shape, (t, ref[t].shape, g[t].shape)
        if g[t].size:
            assert np.abs(ref[t] - g[t]).max() <= 1e-12 * max(np.abs(g[t]).max(), 1e-300) + 1e-18, (name, form, t)


@pytest.mark.parametrize("form", ["plain", "crit"])
def test_reference_agrees_with_a_central_finite_difference(form):
    """d loss / d (a few entries of every input with a gradient) on a tiny case, h = 1e-6: the gates sit 1e-3 away, the loss is smooth"""
    c = HR.case("DH17")
    ref = HR.evaluate(c, form)
    rng = np.random.default_rng(5)
    h = 1e-6
    for key, t in (("r", "dr"), ("w0", "dW0"), ("b0", "db0"), ("w2", "dW2"), ("b2", "db2"), ("emb_w", "demb_w"), ("emb_b", "demb_b")):
        live = np.argwhere(np.broadcast_to(HR.keep_of(c["lengths"], c["T"])[:, :, None], c["r"].shape)) if key == "r" else None
        for _ in range(4):
            idx = tuple(live[rng.integers(len(live))]) if key == "r" else tuple(rng.integers(0, s) for s in c[key].shape)
            vals = []
            for sgn in (1.0, -1.0):
                d = dict(c)
                d[key] = c[key].astype(np.float64)
                d[key][idx] += sgn * h
                vals.append(float(HR.evaluate(d, form)["loss"]))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - ref[t][idx]) <= 1e-8 * np.abs(ref[t]).max() + 1e-10, (key, idx, fd, ref[t][idx])


# ---- 2. the cases ------------------------------------------------------------------------------------------------------------------------
def test_case_table_reaches_every_branch_it_names():
    dh = lambda n: HR.dh_of(HR.CASES[n])
    assert (dh("DH192"), dh("DH193"), dh("DH186")) == (192, 193, 186) and dh("DH256_F0") == dh("DH256_F32") == 256
    assert [dh(n) for n in HR.GROUPS["lane_slots"]] == [64, 65, 128, 129, 16, 17, 4]
    assert [HR.CASES[n]["T"] for n in HR.GROUPS["steps"]] == [1, 16, 17, 64, 65, 128, 129, 600] and HR.CASES["T600"]["B"] == 3
    assert [HR.CASES[n]["B"] for n in HR.GROUPS["batch"]] == [1, 255, 256, 257, 513]
    assert [HR.CASES[n]["C"] * dh(n) for n in ("C4_DH256", "C5_DH205", "C16_DH256")] == [1024, 1025, 4096]
    assert {HR.CASES[n]["C"] for n in HR.GROUPS["classes"]} >= {1, 2, 16}
    emb = lambda n: (HR.CASES[n]["Fe"], HR.CASES[n]["ds"])
    assert [emb(n) for n in ("EMB_32x32", "EMB_33x32", "EMB_DS64", "EMB_DS65", "EMB_DS17")] == [(32, 32), (33, 32), (16, 64), (4, 65), (4, 17)]
    assert HR.CASES["FE16"]["Fe"] == 16 and HR.CASES["FE17"]["Fe"] == 17 and HR.FE0_CASES
    assert [HR.CASES[n]["B"] for n in ("CRIT_B1024", "CRIT_B1025")] == [1024, 1025]
    for n in HR.ALL_CASES:
        c = HR.case(n)
        assert c["D"] % 4 == 0 and c["dh"] <= 256 and 1 <= c["C"] <= 16 and (c["Fe"] == 0) == (c["ds"] == 0)
    # lengths: T, 1, both sides of 64 / 128, zero; the plan's sets
    seen = set()
    for n in HR.GROUPS["steps"]:
        seen |= set(HR.case(n)["lengths"].tolist())
    assert {0, 1, 63, 64, 65, 127, 128, 129, 600} <= seen
    ties = HR.case("PLAN_TIES")["lengths"]
    assert len(set(ties.tolist())) < len(ties) and list(ties) != sorted(ties, reverse=True)
    z = HR.case("PLAN_ZEROS")["lengths"]
    assert z[-1] == 0 and 0 in z[1:-2] and z.max() > 0
    assert HR.case("PLAN_SINGLE")["B"] == 1 and set(HR.case("PLAN_ONES")["lengths"].tolist()) == {1}
    assert sorted(dh(n) for n in ("PLAN_DH186", "PLAN_DH193", "PLAN_DH256")) == [186, 193, 256]
    assert 2 not in HR.case("CRIT_ABSENT")["y"] and HR.case("CRIT_W0")["crit"][2] == 0 and 1 in HR.case("CRIT_W0")["y"]
    for n in HR.CRIT_CASES:
        c = HR.case(n)
        assert float((c["crit"][1:][c["y"]]).sum()) > 0, n                            # W stays positive
    for v, (n, form) in HR.VARIANTS.items():
        assert (n, form) in HR.RUNS, v


@pytest.mark.parametrize("name", HR.ALL_CASES)
def test_gates_are_decisive(name):
    c = HR.case(name)
    pre = HR.reference(name, "plain")["pre"]
    assert np.abs(pre).min() >= HR.GATE_MARGIN, (name, float(np.abs(pre).min()))
    if c["B"] > 1:
        assert ((pre > 0).any(0) & (pre < 0).any(0)).all(), name                      # every unit: a row open and a row shut
    else:
        assert (pre > 0).any() and (pre < 0).any()
    # the float32 evaluation opens the same gates: the yardstick measures rounding, not a flipped unit
    assert np.array_equal(HR.reference(name, "plain", np.float32)["pre"] > 0, pre > 0)


@pytest.mark.parametrize("name,form", HR.RUNS)
def test_bounds_are_finite_positive_and_under_the_ceilings(name, form):
    ref = HR.reference(name, form)
    for t in HR.tensors_of(form):
        b = HR.bound_of(name, form, t)
        if t != "loss" and (np.asarray(ref[t]).size == 0 or not np.asarray(ref[t]).any()):
            assert b == 0.0 and HR.error_of(t, np.zeros_like(ref[t]), ref[t]) == 0.0    # exactly zero: only exact zeros pass
            continue
        assert np.isfinite(b) and 0 < b <= (HR.LOSS_CEILING if t == "loss" else HR.CEILING), (name, form, t, b)
        assert b >= HR.YARD_FACTOR * HR.FLOOR_ULPS * 2.0 ** -24 or t == "loss"
    # the float64 reference compared with itself passes, exact zeros included
    rows, nonzero = HR.compare(name, form, ref)
    assert not nonzero and all(e == 0 for _, e, _, _ in rows)


def test_padded_steps_and_zero_cotangents_are_exact_zeros_of_the_reference():
    c = HR.case("T65")
    dr = HR.reference("T65", "plain")["dr"]
    assert not dr[~HR.keep_of(c["lengths"], c["T"])].any() and dr[HR.keep_of(c["lengths"], c["T"])].all()
    z = HR.evaluate(c, "cot", dlog_in=np.zeros((c["B"], c["C"]), np.float32))
    assert all(not z[t].any() for t in HR.GRADS)
    one = HR.reference("C1", "plain")
    assert float(one["loss"]) == 0.0 and all(not one[t].any() for t in HR.GRADS)


@pytest.mark.parametrize("variant", sorted(HR.VARIANTS))
def test_a_wrong_kernel_misses_a_bound_by_more_than_10x(variant):
    assert HR.variant_margin(variant) > 10.0, variant


# ---- 3. refusals: the checks precede every launch --------------------------------------------------------------------------------------------
_A = 0x100000                                            # never dereferenced: every call below is refused on the host


def _train_args(T=7, B=5, D=16, ds=3, Fe=4, C=2, crit=False, ws_short=0, **ptr):
    """the arguments of rd_head_train[_crit] with made-up, 16-byte aligned pointers; ptr: name -> another value for one of them"""
    names = ["r", "mask", "lengths", "stat", "emb_w", "emb_b", "w0", "b0", "w2", "b2", "y"] + (["crit"] if crit else []) \
        + ["loss", "logits", "g_emb_w", "g_emb_b", "g_w0", "g_b0", "g_w2", "g_b2", "dr", "ws"]
    p = {n: _A + 4096 * i for i, n in enumerate(names)}
    p.update(ptr)
    shp = _lib.shape(B, T, 1, 4)
    nbytes = int(_lib.load().rd_head_train_workspace_bytes(B, D + Fe, C)) - ws_short
    return [ctypes.byref(shp), D, ds, Fe, C] + [ctypes.c_void_p(p[n]) for n in names] + [max(nbytes, 0), None], shp


REFUSALS = {
    "D % 4 != 0": (dict(D=18), b"unsupported sizes"),
    "dh = 257": (dict(D=252, Fe=5), b"unsupported sizes"),
    "C = 0": (dict(C=0), b"unsupported sizes"),
    "C = 17": (dict(C=17), b"unsupported sizes"),
    "B = 0": (dict(B=0), b"bad shape"),
    "misaligned r": (dict(r=_A + 4), b"16-byte aligned"),
    "misaligned dr": (dict(dr=_A + 8), b"16-byte aligned"),
    "workspace one byte short": (dict(ws_short=1), b"workspace too small"),
    "Fe > 0 with a null stat": (dict(stat=None), b"static embedding tensors missing"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refused_before_any_launch(lib, what):
    kw, message = REFUSALS[what]
    on, read = lib.rd_debug_launch_log, lib.rd_debug_launch_log_read
    on.argtypes, on.restype = [ctypes.c_int], None
    read.argtypes, read.restype = [ctypes.c_char_p, ctypes.c_size_t], ctypes.c_size_t
    on(1)
    try:
        for crit in (False, True):
            args, _keep = _train_args(crit=crit, **kw)
            rc = getattr(lib, "rd_head_train_crit" if crit else "rd_head_train")(*args)
            assert rc == RD_EINVAL and message in lib.rd_last_error(), (what, rc, lib.rd_last_error())
        assert read(None, 0) == 0
    finally:
        on(0)


def test_forward_and_backward_share_the_refusals(lib):
    args, _keep = _train_args(D=18)
    fwd = args[:5] + args[5:15] + [args[17]] + args[-3:]                               # .. b2, logits, workspace, bytes, stream
    bwd = args[:5] + args[5:15] + [args[16]] + args[18:]                               # .. b2, dlogits, the six gradients, dr, ..
    assert lib.rd_head_forward(*fwd) == RD_EINVAL and b"unsupported sizes" in lib.rd_last_error()
    assert lib.rd_head_backward(*bwd) == RD_EINVAL and b"unsupported sizes" in lib.rd_last_error()


def test_the_criterion_refuses_2_pow_24_samples(lib):
    args, _keep = _train_args(B=1 << 24, D=4, Fe=0, ds=0, crit=True)
    assert lib.rd_head_train_crit(*args) == RD_EINVAL and b"2^24" in lib.rd_last_error()


# ---- 4. the route ------------------------------------------------------------------------------------------------------------------------
def _route(lib, mode, B, D, ds, Fe, C, crit):
    words, name = (ctypes.c_uint32 * 11)(), ctypes.create_string_buffer(64)
    rc = lib.rd_debug_head_route(mode, B, D, ds, Fe, C, int(crit), words, name, len(name))
    assert rc == 0, lib.rd_last_error()
    w = list(words)
    n = w[0] >> 8 & 3
    return dict(name=name.value.decode(), bits={b for i, b in enumerate(_lib.HEAD_ROUTE_BITS) if w[0] >> i & 1}, touch=w[1], grid=w[2],
                ntiles=w[3], rider=w[4], jobs=[(w[8 + j] >> 16, w[8 + j] & 0xFFFF, w[5 + j]) for j in range(n)], raw=w)


# (mode, B, D, d_static, Fe, C, crit) -> name, bits, touch site, k_head_wgrad tiles, deferred blocks, jobs as (n tiles, k tiles, blk0).
# Worked out by hand from head_route: dh = D + Fe, narrow iff dh <= 192, emb_lds iff 0 < Fe ds <= 1024 and ds <= 64, job tiles
# ceil(N / 16) x ceil(K / 16) for (dh, dh), (C, dh), (Fe, ds), four tiles per deferred block.
ROUTE_TABLE = [
    ((0, 256, 152, 6, 34, 2, 0), "k_head_rows<12,3>", {"narrow", "emb_lds"}, "HEAD_P19", 159, 40, [(12, 12, 0), (1, 12, 144), (3, 1, 156)]),
    ((0, 256, 152, 6, 34, 2, 1), "k_head_rows<12,3,crit>", {"narrow", "crit", "emb_lds"}, "HEAD_P19_C", 159, 40,
     [(12, 12, 0), (1, 12, 144), (3, 1, 156)]),
    ((0, 5, 160, 3, 32, 2, 0), "k_head_rows<12,3>", {"narrow", "emb_lds"}, "HEAD_P19", 158, 40, [(12, 12, 0), (1, 12, 144), (2, 1, 156)]),
    ((0, 5, 160, 3, 33, 2, 0), "k_head_rows<16,4>", {"emb_lds"}, "HEAD", 185, 47, [(13, 13, 0), (1, 13, 169), (3, 1, 182)]),
    ((2, 5, 160, 3, 33, 2, 0), "k_head_rows<16,4>", {"emb_lds"}, "HEAD", 185, 47, [(13, 13, 0), (1, 13, 169), (3, 1, 182)]),
    ((0, 5, 256, 0, 0, 16, 1), "k_head_rows<16,4,crit>", {"crit"}, "HEAD_C", 272, 68, [(16, 16, 0), (1, 16, 256)]),
    ((0, 5, 16, 32, 32, 2, 0), "k_head_rows<12,3>", {"narrow", "emb_lds"}, "HEAD_P19", 16, 4, [(3, 3, 0), (1, 3, 9), (2, 2, 12)]),
    ((0, 5, 16, 32, 33, 2, 0), "k_head_rows<12,3>", {"narrow"}, "HEAD_P19", 26, 7, [(4, 4, 0), (1, 4, 16), (3, 2, 20)]),
    ((0, 5, 16, 64, 16, 2, 0), "k_head_rows<12,3>", {"narrow", "emb_lds"}, "HEAD_P19", 10, 3, [(2, 2, 0), (1, 2, 4), (1, 4, 6)]),
    ((0, 5, 16, 65, 4, 2, 0), "k_head_rows<12,3>", {"narrow"}, "HEAD_P19", 11, 3, [(2, 2, 0), (1, 2, 4), (1, 5, 6)]),
    ((0, 5, 16, 17, 4, 2, 0), "k_head_rows<12,3>", {"narrow", "emb_lds"}, "HEAD_P19", 8, 2, [(2, 2, 0), (1, 2, 4), (1, 2, 6)]),
    ((1, 256, 152, 6, 34, 2, 0), "k_head_rows<12,3>", {"narrow", "emb_lds"}, "HEAD_P19", 0, 0, []),
    ((0, 1025, 4, 0, 0, 3, 1), "k_head_rows<12,3,crit>", {"narrow", "crit"}, "HEAD_P19_C", 2, 1, [(1, 1, 0), (1, 1, 1)]),
]


@pytest.mark.parametrize("row", ROUTE_TABLE, ids=lambda r: "-".join(map(str, r[0])))
def test_route_query_against_the_hand_table(lib, row, monkeypatch):
    (mode, B, D, ds, Fe, C, crit), name, bits, site, ntiles, rider, jobs = row
    touch = build.read_touch_table()
    got = _route(lib, mode, B, D, ds, Fe, C, crit)
    assert (got["name"], got["bits"], got["grid"], got["ntiles"], got["rider"], got["jobs"]) == (name, bits, B, ntiles, rider, jobs), got
    assert got["touch"] == touch[site] > 0, (got["touch"], site, touch)
    assert got["raw"][5 + len(jobs):8] == [0] * (3 - len(jobs)) and got["raw"][8 + len(jobs):] == [0] * (3 - len(jobs))


def test_route_of_every_case_names_the_instantiation_the_table_expects(lib):
    for name, form in HR.RUNS:
        c = HR.case(name)
        got = _route(lib, 2 if form == "cot" else 0, c["B"], c["D"], c["ds"], c["Fe"], c["C"], form == "crit")
        assert got["name"] == HR.instantiation(c, form == "crit"), (name, form, got["name"])
        assert ("emb_lds" in got["bits"]) == (0 < c["Fe"] * c["ds"] <= 1024 and c["ds"] <= 64), name
    assert "emb_lds" in _route(lib, 0, 5, 16, 32, 32, 2, 0)["bits"] and "emb_lds" not in _route(lib, 0, 5, 16, 32, 33, 2, 0)["bits"]


def test_route_query_refuses_what_the_head_refuses(lib):
    words, name = (ctypes.c_uint32 * 11)(), ctypes.create_string_buffer(b"x" * 8, 64)
    for args in ((0, 5, 18, 3, 4, 2, 0), (0, 5, 252, 3, 5, 2, 0), (0, 5, 16, 3, 4, 0, 0), (0, 5, 16, 3, 4, 17, 0), (0, 0, 16, 3, 4, 2, 0),
                 (0, 5, 16, 0, 4, 2, 0), (2, 5, 16, 3, 4, 2, 1), (3, 5, 16, 3, 4, 2, 0)):
        assert lib.rd_debug_head_route(*args, words, name, len(name)) == RD_EINVAL, args
        assert name.value == b"" and not any(words)
    assert lib.rd_debug_head_route(0, 5, 16, 3, 4, 2, 0, None, name, len(name)) == RD_EINVAL
