"""CPU: the host side of FlatAdam's parameter groups and decoupled weight decay (`optim.ParamGroups`, `optim.no_decay`,
`FlatAdam(groups=, decoupled=)`) -- the chunk map byte for byte and every refusal, what the sixteen (clip, ema, grp, dev) forms
enqueue on a stub library, what stays exactly as it was with the keywords off, the group cell under `set_group` and `weight_decay`
assignments, the state dictionary, the argument checks of the grouped C-ABI entry points (RD_EINVAL before anything is launched: no
device is touched here) and what `fit` refuses without a device."""
import ctypes
import math
import types

import pytest
import torch

from raindrop_amd import _lib, optim
from raindrop_amd.optim import FlatAdam, ParamGroups

# the hand-made layout of tests/test_param_groups_gpu.py: (name, size, offset); 1478 elements, 24 chunks of 64
TENSORS = [("t1.bias", 1, 0), ("t2.weight", 63, 64), ("t3.weight", 64, 128), ("t4.bias", 65, 192), ("t5.weight", 1030, 320),
           ("t6.weight", 70, 1408)]
N = 1478
RULES = [dict(match=r"\.bias$", lr_scale=4.0, weight_decay=0.0), dict(match=["t2.weight"], lr_scale=0.1, weight_decay=0.05),
         dict(match=lambda n: n.startswith("t6"), lr_scale=0.0)]
# chunk -> group: t1 (1 chunk, group 1), t2 (1, group 2), t3 (1, group 0), t4 (65 elements and their padding: 2 chunks, group 1),
# t5 (1030 elements: 17 chunks, group 0), t6 (70 elements: 2 chunks, the second one partial, group 3)
CHUNK_MAP = [1, 2, 0, 1, 1] + [0] * 17 + [3, 3]


def _layout(tensors=TENSORS):
    return types.SimpleNamespace(names=[t[0] for t in tensors], slices=[(o, o + n) for _, n, o in tensors],
                                 params=[torch.zeros(n) if name.endswith("bias") else torch.zeros(1, n) for name, n, _ in tensors])


def _param(n=N):
    p = torch.nn.Parameter(torch.arange(n, dtype=torch.float32))
    p.grad = torch.zeros(n)
    return p


# ---- ParamGroups ----------------------------------------------------------------------------------------------------------------------
def test_chunk_map_byte_for_byte():
    g = ParamGroups(_layout(), RULES)
    assert g.chunk_map.dtype == torch.uint8 and g.chunk_map.tolist() == CHUNK_MAP and g.n_chunks == (N + 63) // 64 == 24
    assert len(g) == 4 and g.names == [["t3.weight", "t5.weight"], ["t1.bias", "t4.bias"], ["t2.weight"], ["t6.weight"]]   # group 0: the remainder
    assert g.lr_scale == [1.0, 4.0, 0.1, 0.0] and g.weight_decay == [None, 0.0, 0.05, None]
    assert g.partition() == (("t3.weight", "t5.weight"), ("t1.bias", "t4.bias"), ("t2.weight",), ("t6.weight",))
    none = ParamGroups(_layout(), [])
    assert none.chunk_map.tolist() == [0] * 24 and none.names == [[t[0] for t in TENSORS]]
    # the order of the layout's entries does not matter, their offsets do
    back = ParamGroups(_layout(TENSORS[::-1]), RULES)
    assert back.chunk_map.tolist() == CHUNK_MAP


def test_no_decay_is_every_parameter_with_at_most_one_dimension():
    rule = optim.no_decay(_layout())
    assert rule == dict(match=["t1.bias", "t4.bias"], weight_decay=0.0)
    g = ParamGroups(_layout(), [rule])
    assert g.chunk_map.tolist() == [1, 0, 0, 1, 1] + [0] * 19 and g.weight_decay == [None, 0.0] and g.lr_scale == [1.0, 1.0]


def test_refusals():
    lay = _layout()
    with pytest.raises(ValueError, match="both match"):
        ParamGroups(lay, [dict(match="bias"), dict(match=["t1.bias"])])
    with pytest.raises(ValueError, match="matches no parameter"):
        ParamGroups(lay, [dict(match="nothing")])
    with pytest.raises(ValueError, match="does not hold"):
        ParamGroups(lay, [dict(match=["t9.weight"])])
    ParamGroups(_layout([("p%d" % i, 1, 64 * i) for i in range(15)]), [dict(match="p%d$" % i) for i in range(15)])     # 15 rules: fine
    with pytest.raises(ValueError, match="at most 15"):
        ParamGroups(_layout([("p%d" % i, 1, 64 * i) for i in range(16)]), [dict(match="p%d$" % i) for i in range(16)])
    with pytest.raises(ValueError, match="at most 1"):
        ParamGroups(lay, [dict(match="t1"), dict(match="t2")], max_groups=2)
    with pytest.raises(ValueError, match="max_groups"):
        ParamGroups(lay, [], max_groups=17)
    for key in ("lr_scale", "weight_decay"):
        for bad in (-1.0, -0.0 - 1e-9, math.inf, -math.inf, math.nan, "1", True):
            with pytest.raises(ValueError, match=key):
                ParamGroups(lay, [dict(match="t1", **{key: bad})])
    with pytest.raises(ValueError, match="lr_scale"):
        ParamGroups(lay, [dict(match="t1", lr_scale=None)])
    with pytest.raises(ValueError, match="keys"):
        ParamGroups(lay, [dict(match="t1", lr=2.0)])
    with pytest.raises(ValueError, match="keys"):
        ParamGroups(lay, [dict(lr_scale=2.0)])
    with pytest.raises(ValueError, match="multiple of 64"):
        ParamGroups(_layout([("a", 3, 0), ("b", 5, 32)]), [])
    with pytest.raises(ValueError, match="overlaps"):
        ParamGroups(_layout([("a", 65, 0), ("b", 5, 64)]), [])
    with pytest.raises(ValueError, match="ParamGroups"):
        FlatAdam(_param(), groups=RULES)
    with pytest.raises(ValueError, match="another layout"):
        FlatAdam(_param(N + 64), groups=ParamGroups(_layout(), RULES))


# ---- dispatch on the stub library (tests/test_adam_dispatch_host.py with the grp flag) --------------------------------------------------
HOST = (N, "p", "g", "m", "v", 2.5e-4, 0.9, 0.999, 1e-8, 0.01, 1)
DEVA = (N, "p", "g", "m", "v", 0.9, 0.999, 1e-8, "state")
SUMSQ = ("rd_grad_sumsq", (N, "g", "partial", 1024, "stream"))
ADVANCE = ("rd_adam_state_advance", ("state", 0.9, 0.999, "stream"))
CLIP, EMA, GRP = ("partial", 1024, "clip"), ("ema", "ema_cell"), ("chunk_group", "group_cell", "stream")
# (clip, ema, dev) -> the calls of ONE step of an optimizer with groups on
EXPECTED = {
    (False, False, False): [("rd_adam_step_grp", HOST + GRP)],
    (True, False, False): [SUMSQ, ("rd_adam_step_clip_grp", HOST + CLIP + GRP)],
    (False, True, False): [("rd_adam_step_ema_grp", HOST + EMA + GRP)],
    (True, True, False): [SUMSQ, ("rd_adam_step_clip_ema_grp", HOST + CLIP + EMA + GRP)],
    (False, False, True): [ADVANCE, ("rd_adam_step_grp_dev", DEVA + GRP)],
    (True, False, True): [ADVANCE, SUMSQ, ("rd_adam_step_clip_grp_dev", DEVA + CLIP + GRP)],
    (False, True, True): [ADVANCE, ("rd_adam_step_ema_grp_dev", DEVA + EMA + GRP)],
    (True, True, True): [ADVANCE, SUMSQ, ("rd_adam_step_clip_ema_grp_dev", DEVA + CLIP + EMA + GRP)],
}


def _opt(clip=False, ema=False, **kw):
    if clip:
        kw.update(max_grad_norm=1.0)
    if ema:
        kw.update(ema_decay=0.9)
    return FlatAdam(_param(), lr=2.5e-4, weight_decay=0.01, **kw)


def _reduced(a, calls):
    named = dict(p=a.param.data, g=a.param.grad, m=a.exp_avg, v=a.exp_avg_sq, state=a.step_cell, partial=a.clip_partial, clip=a.clip_cell,
                 ema=a.ema, ema_cell=a.ema_cell, chunk_group=a.chunk_group, group_cell=a.group_cell)
    names = {t.data_ptr(): k for k, t in named.items() if t is not None}
    out = []
    for name, args in calls:
        row = tuple(names[x.value] if isinstance(x, ctypes.c_void_p) else x for x in args)      # (KeyError: a pointer to none of the buffers)
        assert all(x == "stream" or type(x) in (int, float, str) for x in row), (name, row)
        out.append((name, row))
    return out


@pytest.fixture
def calls(monkeypatch):
    log = []
    monkeypatch.setattr(optim._lib, "call", lambda name, *args: log.append((name, args)))
    monkeypatch.setattr(optim.ops, "_stream", lambda: "stream")
    return log


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("ema", [False, True], ids=["", "ema"])
@pytest.mark.parametrize("clip", [False, True], ids=["", "clip"])
def test_grouped_forms_enqueue_the_grp_entry_points(calls, clip, ema, dev):
    a = _opt(clip, ema, groups=ParamGroups(_layout(), RULES))
    if dev:
        a.step_captured()
    else:
        a.step()
    assert _reduced(a, calls) == EXPECTED[(clip, ema, dev)]
    assert a.chunk_group.dtype == torch.uint8 and a.chunk_group.tolist() == CHUNK_MAP
    assert a.group_cell.dtype == torch.float64 and tuple(a.group_cell.shape) == (16, 4) and a.group_cell.data_ptr() % 16 == 0
    if dev:                                                         # the same launches again, without the advance
        del calls[:]
        a.step_captured(advance=False)
        assert _reduced(a, calls) == EXPECTED[(clip, ema, dev)][1:]


def test_off_enqueues_todays_calls_and_decoupled_alone_the_grp_forms(calls):
    off = _opt()
    assert off.groups is None and not off.decoupled and off.chunk_group is None and off.group_cell is None
    off.step()
    assert _reduced(off, calls) == [("rd_adam_step", HOST + ("stream",))]
    del calls[:]
    off.step_captured()
    assert _reduced(off, calls) == [ADVANCE, ("rd_adam_step_dev", DEVA + ("stream",))]
    del calls[:]
    w = _opt(decoupled=True)                                        # one group, everything in it
    w.step()
    assert _reduced(w, calls) == EXPECTED[(False, False, False)]
    assert w.chunk_group.tolist() == [0] * 24
    assert w.group_cell.tolist() == [[1.0, 0.0, 0.01, 0.0]] + [[0.0] * 4] * 15


# ---- hyper(), the cell, the state dictionary ---------------------------------------------------------------------------------------------
def test_off_is_the_optimizer_without_the_keywords():
    off = _opt()
    assert off.hyper() == (0.9, 0.999, 1e-8)
    assert sorted(off.state_dict()) == sorted(["t", "exp_avg", "exp_avg_sq", "lr", "betas", "eps", "weight_decay", "max_grad_norm",
                                               "grad_skipped", "grad_clipped"])
    off.sync_group_cell()                                           # a no-op, like sync_clip_cell with clipping off
    off.sync_cells(full=True)
    for f in (lambda: off.set_group(0, lr_scale=2.0), off.group_info):
        with pytest.raises(ValueError, match="off"):
            f()
    on = _opt(groups=ParamGroups(_layout(), RULES))
    assert on.hyper() == off.hyper() + ("grp",)                     # on / off are different captures
    assert _opt(decoupled=True).hyper() == off.hyper() + ("grp",)
    assert _opt(True, True, decoupled=True).hyper() == off.hyper() + ("clip", "ema", "grp")
    assert sorted(on.state_dict()) == sorted(list(off.state_dict()) + ["groups", "decoupled"])


@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
def test_cell_rows_set_group_and_weight_decay_assignment(decoupled):
    a = _opt(groups=ParamGroups(_layout(), RULES), decoupled=decoupled)
    row = (lambda s, wd: [s, 0.0, wd, 0.0]) if decoupled else (lambda s, wd: [s, wd, 0.0, 0.0])
    zeros = [[0.0] * 4] * 12
    assert a.group_cell.tolist() == [row(1.0, 0.01), row(4.0, 0.0), row(0.1, 0.05), row(0.0, 0.01)] + zeros
    h, cell = a.hyper(), a.group_cell.data_ptr()
    a.set_group(1, lr_scale=2.0)                                    # one row; the decay it had stays
    a.set_group(3, lr_scale=0.5)
    assert a.group_cell.tolist() == [row(1.0, 0.01), row(2.0, 0.0), row(0.1, 0.05), row(0.5, 0.01)] + zeros
    a.weight_decay = 0.02                                           # plain assignment: pushed by the sync TrainStep.run_full calls
    assert a.group_cell.tolist()[0] == row(1.0, 0.01)
    a.sync_cells()
    # only the groups that FOLLOW the optimizer's decay moved: 0 and 3; 1 and 2 keep their own
    assert a.group_cell.tolist() == [row(1.0, 0.02), row(2.0, 0.0), row(0.1, 0.05), row(0.5, 0.02)] + zeros
    a.set_group(3, weight_decay=0.3)                                # its own from now on
    a.weight_decay = 0.04
    a.sync_group_cell()
    assert a.group_cell.tolist() == [row(1.0, 0.04), row(2.0, 0.0), row(0.1, 0.05), row(0.5, 0.3)] + zeros
    assert a.hyper() == h and a.group_cell.data_ptr() == cell      # none of it is a new capture
    assert a.group_info() == [dict(names=["t3.weight", "t5.weight"], lr_scale=1.0, weight_decay=0.04),
                              dict(names=["t1.bias", "t4.bias"], lr_scale=2.0, weight_decay=0.0),
                              dict(names=["t2.weight"], lr_scale=0.1, weight_decay=0.05),
                              dict(names=["t6.weight"], lr_scale=0.5, weight_decay=0.3)]
    for bad in (dict(lr_scale=-1.0), dict(weight_decay=math.nan), dict(lr_scale=math.inf), dict(weight_decay="0")):
        with pytest.raises(ValueError):
            a.set_group(0, **bad)
    for i in (-1, 4, 1.0, True):
        with pytest.raises(ValueError, match="group"):
            a.set_group(i, lr_scale=1.0)
    assert a.group_info()[0] == dict(names=["t3.weight", "t5.weight"], lr_scale=1.0, weight_decay=0.04)


def test_state_dict_round_trip_and_other_partitions():
    a = _opt(groups=ParamGroups(_layout(), RULES), decoupled=True)
    a.set_group(1, lr_scale=2.0)
    sd = a.state_dict()
    assert sd["decoupled"] is True and sd["groups"] == [
        dict(names=["t3.weight", "t5.weight"], lr_scale=1.0, weight_decay=None), dict(names=["t1.bias", "t4.bias"], lr_scale=2.0, weight_decay=0.0),
        dict(names=["t2.weight"], lr_scale=0.1, weight_decay=0.05), dict(names=["t6.weight"], lr_scale=0.0, weight_decay=None)]
    b = _opt(groups=ParamGroups(_layout(), RULES))                  # the same partition, other values, coupled
    cell, cmap = b.group_cell.data_ptr(), b.chunk_group.data_ptr()
    b.load_state_dict(dict(sd, t=3, weight_decay=0.02))
    assert b.group_cell.data_ptr() == cell and b.chunk_group.data_ptr() == cmap                # in place: a captured step stays valid
    assert b.t == 3 and b.decoupled and b.hyper() == a.hyper()
    assert b.group_cell.tolist()[:4] == [[1.0, 0.0, 0.02, 0.0], [2.0, 0.0, 0.0, 0.0], [0.1, 0.0, 0.05, 0.0], [0.0, 0.0, 0.02, 0.0]]
    old = {k: v for k, v in sd.items() if k not in ("groups", "decoupled")}
    b.load_state_dict(dict(old, t=9))                               # a dictionary without the keys: the settings stay
    assert b.t == 9 and b.decoupled and b.group_info()[1]["lr_scale"] == 2.0
    other = _opt(groups=ParamGroups(_layout(), RULES[:2]))          # t6 in group 0 there
    for target in (other, _opt(), _opt(decoupled=True)):
        keep = target.t
        with pytest.raises(ValueError, match="another partition"):
            target.load_state_dict(dict(sd, t=5))
        assert target.t == keep                                     # refused before anything was changed
    one = _opt(decoupled=True)
    with pytest.raises(ValueError, match="another partition"):
        a.load_state_dict(one.state_dict())
    two = _opt(decoupled=True)
    two.load_state_dict(dict(one.state_dict(), weight_decay=0.5))
    assert two.group_cell.tolist()[0] == [1.0, 0.0, 0.5, 0.0]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
GRP_ENTRY_POINTS = ["rd_adam_step" + "_clip" * c + "_ema" * e + "_grp" + "_dev" * d for c in (0, 1) for e in (0, 1) for d in (0, 1)]


def test_signatures_are_the_twins_plus_map_and_cell():
    for name in GRP_ENTRY_POINTS:
        twin = name.replace("_grp", "")
        assert _lib.SIGNATURES[name][0] == _lib.SIGNATURES[twin][0]
        assert _lib.SIGNATURES[name][1] == _lib.SIGNATURES[twin][1][:-1] + [ctypes.c_void_p] * 3, name


def test_entry_points_refuse_bad_arguments_before_launch():
    lib = _lib.load()
    nbytes = lib.rd_grad_sumsq_bytes()
    buf = (ctypes.c_double * (nbytes // 8 + 256))()                 # host memory: only its ADDRESS is looked at
    a = (ctypes.addressof(buf) + 15) & ~15
    ok = [a, a + 64, a + 128, a + 192]                              # param, grad, exp_avg, exp_avg_sq
    part, clip, state, ema, ecell, cmap, gcell = a + 256, a + 256 + nbytes, a + 320 + nbytes, a + 384 + nbytes, a + 448 + nbytes, \
        a + 512 + nbytes + 1, a + 576 + nbytes                      # (the map is bytes: any address)

    def call(name, n=16, ptrs=ok, cm=cmap, gc=gcell):
        args = [n] + list(ptrs) + ([0.9, 0.999, 1e-8, state] if name.endswith("_dev") else [1e-3, 0.9, 0.999, 1e-8, 0.0, 1])
        if "_clip" in name:
            args += [part, nbytes, clip]
        if "_ema" in name:
            args += [ema, ecell]
        return getattr(lib, name)(*args, cm, gc, None)

    def bad(rc, word):
        assert rc == -1 and word in lib.rd_last_error(), (rc, lib.rd_last_error())

    for name in GRP_ENTRY_POINTS:
        bad(call(name, cm=None), b"NULL chunk_group / group_cell")
        bad(call(name, gc=None), b"NULL chunk_group / group_cell")
        bad(call(name, gc=gcell + 8), b"group_cell must be 16-byte aligned")
        bad(call(name, n=0), b"bad n")                              # every grouped form refuses an empty update
        bad(call(name, n=-3), b"bad n")
        bad(call(name, ptrs=[None] + ok[1:]), b"NULL")
        bad(call(name, ptrs=ok[:3] + [ok[3] + 4]), b"aligned")
    assert lib.rd_adam_step(0, *ok, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None) == 0                 # (plain rd_adam_step alone accepts it)


# ---- fit ------------------------------------------------------------------------------------------------------------------------------
def test_fit_refuses_bad_group_arguments_without_a_device():
    from raindrop_amd.trainer import fit
    ds = types.SimpleNamespace(dev=torch.device("cpu"), y=torch.zeros(8, dtype=torch.int64), N=8, T=5, W=6, ds=0, Pstatic=None)
    for bad, word in (("decay", "no_decay"), (dict(match="x"), "list"), ([("x", 1.0)], "list"), ([dict(lr_scale=2.0)], "keys"),
                      ([dict(match="x", lr=1.0)], "keys"), ([dict(match="x", lr_scale=-1.0)], "lr_scale"),
                      ([dict(match="x", weight_decay=math.inf)], "weight_decay"), ([dict(match="p%d" % i) for i in range(16)], "at most 15")):
        with pytest.raises(ValueError, match=word):
            fit(None, ds, ds, 1, batch_size=8, param_groups=bad)
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError, match="decoupled_weight_decay"):
            fit(None, ds, ds, 1, batch_size=8, decoupled_weight_decay=bad)
    with pytest.raises(ValueError, match="strategy"):               # the earlier refusals are still there behind good group arguments
        fit(None, ds, ds, 1, batch_size=8, strategy=0, param_groups="no_decay", decoupled_weight_decay=True)
