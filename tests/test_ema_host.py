"""CPU: the host side of FlatAdam's weight averaging (`ema_decay`, `ema_warmup`) -- keyword validation, what stays exactly as it was
with the keyword off, the cell, the state_dict round trip (old dictionaries included), the swapped flag on a stub library -- and the
argument checks of the new C-ABI entry points, which answer RD_EINVAL before anything is launched (no device is touched here)."""
import ctypes
import os
import re

import pytest
import torch

from raindrop_amd import _lib, optim
from raindrop_amd.optim import FlatAdam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rd_adam_step_ema", "rd_adam_step_ema_dev", "rd_adam_step_clip_ema", "rd_adam_step_clip_ema_dev", "rd_swap_f32")


def _param(n=8):
    p = torch.nn.Parameter(torch.arange(n, dtype=torch.float32))
    p.grad = torch.zeros(n)
    return p


def test_keyword_validation():
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf"), 0, 1, "0.9", True, [0.9]):
        with pytest.raises(ValueError):
            FlatAdam(_param(), ema_decay=bad)
    for good in (0.0, 0.5, 0.999):
        a = FlatAdam(_param(), ema_decay=good)
        assert a.ema_decay == good and not a.ema_warmup and not a.ema_swapped
        assert a.ema_cell.dtype == torch.float64 and a.ema_cell.tolist() == [good, 0.0] + [0.0] * 6
        assert torch.equal(a.ema, a.param.data) and a.ema.data_ptr() != a.param.data_ptr()          # AveragedModel's first-call copy
    w = FlatAdam(_param(), ema_decay=0.9, ema_warmup=True)
    assert w.ema_cell.tolist()[:2] == [0.9, 1.0]
    for bad in (-1.0, 1.0, None, 1):
        with pytest.raises(ValueError):
            w.set_ema_decay(bad)
    assert w.ema_decay == 0.9


def test_off_is_the_optimizer_without_the_keyword():
    off = FlatAdam(_param(), lr=1e-4)
    assert off.ema_decay is None and off.ema is None and off.ema_cell is None and not off.ema_swapped
    assert off.hyper() == (0.9, 0.999, 1e-8)
    assert FlatAdam(_param(), max_grad_norm=1.0).hyper() == (0.9, 0.999, 1e-8, "clip")
    assert sorted(off.state_dict()) == sorted(["t", "exp_avg", "exp_avg_sq", "lr", "betas", "eps", "weight_decay", "max_grad_norm",
                                               "grad_skipped", "grad_clipped"])
    off.sync_ema_cell()                                             # a no-op, like sync_clip_cell with clipping off
    for f in (off.swap_ema, off.ema_updates, lambda: off.set_ema_decay(0.5), lambda: off.ema_weights().__enter__()):
        with pytest.raises(ValueError):
            f()
    on = FlatAdam(_param(), ema_decay=0.9)
    assert on.hyper() == off.hyper() + ("ema",)                     # on / off are different captures
    assert FlatAdam(_param(), ema_decay=0.9, max_grad_norm=1.0).hyper() == off.hyper() + ("clip", "ema")


def test_decay_changes_are_cell_updates_not_new_constants():
    a = FlatAdam(_param(), ema_decay=0.9)
    h, cell = a.hyper(), a.ema_cell.data_ptr()
    a.set_ema_decay(0.5)
    assert a.hyper() == h and a.ema_cell[0].item() == 0.5 and a.ema_cell.data_ptr() == cell
    a.ema_decay = 0.25                                              # plain assignment: pushed by the sync TrainStep.run_full calls
    a.sync_ema_cell()
    assert a.hyper() == h and a.ema_cell[0].item() == 0.25
    assert a.ema_updates() == 0


def test_count_follows_a_step_number_set_from_outside():
    """the launches keep the count in the slot the next step number's parity selects; when `t` jumps, sync_ema_cell copies the
    current count into both slots, so that whichever parity comes next finds it"""
    a = FlatAdam(_param(), ema_decay=0.9)
    a.ema_cell[2:4] = torch.tensor([7.0, 3.0], dtype=torch.float64)     # as after a launch of an even step: slot (t + 1) & 1 = 1 is current
    assert a.t == 0 and a.ema_updates() == 3
    a.t = 5
    assert a.ema_updates() == 3                                     # still read where the launches left it
    a.sync_ema_cell()
    assert a.ema_cell.tolist()[2:4] == [3.0, 3.0] and a.ema_updates() == 3
    a.note_replay()                                                 # a replay of step 6 reads slot 0 and writes slot 1
    a.ema_cell[3] = 4.0
    assert a.t == 6 and a.ema_updates() == 4


def test_state_dict_round_trip_and_old_dictionaries():
    a = FlatAdam(_param(), ema_decay=0.9, ema_warmup=True)
    a.ema.mul_(0.5)
    a.ema_cell[2:4] = torch.tensor([4.0, 4.0], dtype=torch.float64)
    sd = a.state_dict()
    assert sd["ema_decay"] == 0.9 and sd["ema_warmup"] is True and sd["ema_updates"] == 4 and sd["ema"] is a.ema
    b = FlatAdam(_param(), ema_decay=0.5)
    ema, cell = b.ema.data_ptr(), b.ema_cell.data_ptr()
    b.load_state_dict(dict(sd, t=3))
    assert b.ema.data_ptr() == ema and b.ema_cell.data_ptr() == cell                       # in place: a captured step stays valid
    assert b.t == 3 and b.ema_decay == 0.9 and b.ema_warmup and b.ema_updates() == 4 and torch.equal(b.ema, a.ema)
    assert b.ema_cell.tolist() == [0.9, 1.0, 4.0, 4.0, 0.0, 0.0, 0.0, 0.0] and b.hyper() == a.hyper()
    c = FlatAdam(_param())                                          # off -> on by a dictionary that has it on
    c.load_state_dict(sd)
    assert c.ema_decay == 0.9 and c.ema_updates() == 4 and torch.equal(c.ema, a.ema) and c.hyper() == a.hyper()
    old = {k: v for k, v in sd.items() if not k.startswith("ema")}
    b.ema.add_(1.0)
    keep = b.ema.clone()
    b.load_state_dict(dict(old, t=9))                               # a dictionary from before the keyword: average and settings stay
    assert b.t == 9 and b.ema_decay == 0.9 and torch.equal(b.ema, keep) and b.ema_updates() == 4
    d = FlatAdam(_param())
    d.load_state_dict(old)
    assert d.ema_decay is None and d.ema is None and "ema" not in d.state_dict()


def test_swapped_flag_on_a_stub(monkeypatch):
    """swap_ema / ema_weights toggle the flag around rd_swap_f32 (stubbed: it exchanges the two host buffers); while it is set the
    steps, the state dictionary and a whole-step replay raise, and nothing has been enqueued by then"""
    calls = []
    a = FlatAdam(_param(), ema_decay=0.9)
    a.ema.zero_()

    def stub(name, *args):
        calls.append(name)
        assert name == "rd_swap_f32" and args[0] == a.param.numel()
        tmp = a.param.data.clone(); a.param.data.copy_(a.ema); a.ema.copy_(tmp)

    monkeypatch.setattr(optim._lib, "call", stub)
    monkeypatch.setattr(optim.ops, "_stream", lambda: None)
    p0 = a.param.data.clone()
    with a.ema_weights() as o:
        assert o is a and a.ema_swapped and calls == ["rd_swap_f32"]
        assert torch.equal(a.param.data, torch.zeros(8)) and torch.equal(a.ema, p0)
        for f in (a.step, a.step_captured, a.state_dict, lambda: a.load_state_dict({}), lambda: a.ema_weights().__enter__()):
            with pytest.raises(_lib.RaindropHipError):
                f()
        assert a.t == 0 and calls == ["rd_swap_f32"]
        from raindrop_amd.step import TrainStep
        ts = TrainStep.__new__(TrainStep)                           # run_full looks at the flag before anything else of the step
        ts.graph_full, ts._full_opt = object(), a
        ts._param_ptrs = lambda: 0
        ts._ptrs = 0
        with pytest.raises(_lib.RaindropHipError, match="average"):
            ts.run_full()
    assert not a.ema_swapped and calls == ["rd_swap_f32"] * 2 and torch.equal(a.param.data, p0)
    with pytest.raises(KeyError):                                   # the block's exception passes, the weights are swapped back
        with a.ema_weights():
            raise KeyError("x")
    assert not a.ema_swapped and len(calls) == 4 and torch.equal(a.param.data, p0)


def test_validate_ema_runs_validate_inside_the_swap(monkeypatch):
    from raindrop_amd import feed
    a = FlatAdam(_param(), ema_decay=0.9)
    monkeypatch.setattr(optim._lib, "call", lambda name, *args: None)
    monkeypatch.setattr(optim.ops, "_stream", lambda: None)
    seen = []
    monkeypatch.setattr(feed, "validate", lambda model, ds, **kw: seen.append((model, ds, kw, a.ema_swapped)) or {"auroc": 0.5})
    assert feed.validate_ema("m", "ds", a, chunk=64) == {"auroc": 0.5}
    assert seen == [("m", "ds", {"chunk": 64}, True)] and not a.ema_swapped


def test_symbols_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "raindrop_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    twin = {"rd_adam_step_ema": "rd_adam_step", "rd_adam_step_ema_dev": "rd_adam_step_dev", "rd_adam_step_clip_ema": "rd_adam_step_clip",
            "rd_adam_step_clip_ema_dev": "rd_adam_step_clip_dev"}
    for new, old in twin.items():                                   # the twin's arguments, then ema and ema_cell in front of the stream
        assert _lib.SIGNATURES[new][1] == _lib.SIGNATURES[old][1][:-1] + [ctypes.c_void_p] * 3


def test_entry_points_refuse_bad_arguments_before_launch():
    lib = _lib.load()
    G, nbytes = lib.rd_grad_sumsq_grid(), lib.rd_grad_sumsq_bytes()
    buf = (ctypes.c_double * (4 * G + 64))()                      # host memory: only its ADDRESS is looked at
    a = (ctypes.addressof(buf) + 15) & ~15
    ok = [a, a + 64, a + 128, a + 192]                            # param, grad, exp_avg, exp_avg_sq
    part, clip, state, ema, cell = a + 256, a + 256 + nbytes, a + 320 + nbytes, a + 384 + nbytes, a + 448 + nbytes

    def bad(rc, word):
        assert rc == -1 and word in lib.rd_last_error(), (rc, lib.rd_last_error())

    def host(n=16, ptrs=ok, step=1, e=ema, c=cell):
        return lib.rd_adam_step_ema(n, *ptrs, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, e, c, None)

    def dev(n=16, ptrs=ok, st=state, e=ema, c=cell):
        return lib.rd_adam_step_ema_dev(n, *ptrs, 0.9, 0.999, 1e-8, st, e, c, None)

    def chost(n=16, ptrs=ok, step=1, e=ema, c=cell, partial=part, cl=clip):
        return lib.rd_adam_step_clip_ema(n, *ptrs, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, partial, nbytes, cl, e, c, None)

    def cdev(n=16, ptrs=ok, st=state, e=ema, c=cell, partial=part, cl=clip):
        return lib.rd_adam_step_clip_ema_dev(n, *ptrs, 0.9, 0.999, 1e-8, st, partial, nbytes, cl, e, c, None)

    for f in (host, dev, chost, cdev):
        bad(f(n=0), b"bad n")
        bad(f(n=-3), b"bad n")
        for k in range(4):
            bad(f(ptrs=ok[:k] + [None] + ok[k + 1:]), b"NULL")
            bad(f(ptrs=ok[:k] + [ok[k] + 4] + ok[k + 1:]), b"aligned")
        bad(f(e=None), b"NULL")
        bad(f(c=None), b"NULL")
        bad(f(e=ema + 4), b"aligned")
        bad(f(c=cell + 8), b"aligned")
    for f in (chost, cdev):
        bad(f(partial=None), b"NULL")
        bad(f(cl=clip + 8), b"aligned")
    bad(host(step=0), b"step")
    bad(chost(step=0), b"step")
    bad(dev(st=None), b"state")
    bad(cdev(st=state + 8), b"state")
    bad(lib.rd_swap_f32(0, ok[0], ok[1], None), b"bad n")
    bad(lib.rd_swap_f32(-1, ok[0], ok[1], None), b"bad n")
    bad(lib.rd_swap_f32(8, None, ok[1], None), b"NULL")
    bad(lib.rd_swap_f32(8, ok[0], None, None), b"NULL")
    bad(lib.rd_swap_f32(8, ok[0] + 4, ok[1], None), b"aligned")
    bad(lib.rd_swap_f32(8, ok[0], ok[1] + 8, None), b"aligned")
