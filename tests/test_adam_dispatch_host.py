"""CPU: what FlatAdam.step() / step_captured() enqueue, on a stub library -- for each of the eight (clip, ema, dev) forms the exact
sequence of entry points and, per call, the argument tuple with every pointer reduced to the buffer it names; the bookkeeping
(`t`, `_cell_stale`, `_ema_t`) after each call; and a swapped optimizer raising before anything is enqueued.  The table is the
behaviour of the four-way `if` ladders the single dispatch replaced, written out."""
import ctypes

import pytest
import torch

from raindrop_amd import _lib, optim
from raindrop_amd.optim import FlatAdam

N = 8
BUFFERS = ("p", "g", "m", "v")
# (clip, ema, dev) -> the calls of ONE step on a fresh optimizer (lr 1e-3, weight decay 0.01, default betas / eps): step() for the
# host forms (its `step` argument is t = 1), step_captured(advance=True) for the _dev forms (advance=False: the same without the first row)
EXPECTED = {
    (False, False, False): [
        ("rd_adam_step", (8, "p", "g", "m", "v", 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, "stream"))],
    (True, False, False): [
        ("rd_grad_sumsq", (8, "g", "partial", 1024, "stream")),
        ("rd_adam_step_clip", (8, "p", "g", "m", "v", 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, "partial", 1024, "clip", "stream"))],
    (False, True, False): [
        ("rd_adam_step_ema", (8, "p", "g", "m", "v", 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, "ema", "ema_cell", "stream"))],
    (True, True, False): [
        ("rd_grad_sumsq", (8, "g", "partial", 1024, "stream")),
        ("rd_adam_step_clip_ema", (8, "p", "g", "m", "v", 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, "partial", 1024, "clip", "ema", "ema_cell",
                                   "stream"))],
    (False, False, True): [
        ("rd_adam_state_advance", ("state", 0.9, 0.999, "stream")),
        ("rd_adam_step_dev", (8, "p", "g", "m", "v", 0.9, 0.999, 1e-8, "state", "stream"))],
    (True, False, True): [
        ("rd_adam_state_advance", ("state", 0.9, 0.999, "stream")),
        ("rd_grad_sumsq", (8, "g", "partial", 1024, "stream")),
        ("rd_adam_step_clip_dev", (8, "p", "g", "m", "v", 0.9, 0.999, 1e-8, "state", "partial", 1024, "clip", "stream"))],
    (False, True, True): [
        ("rd_adam_state_advance", ("state", 0.9, 0.999, "stream")),
        ("rd_adam_step_ema_dev", (8, "p", "g", "m", "v", 0.9, 0.999, 1e-8, "state", "ema", "ema_cell", "stream"))],
    (True, True, True): [
        ("rd_adam_state_advance", ("state", 0.9, 0.999, "stream")),
        ("rd_grad_sumsq", (8, "g", "partial", 1024, "stream")),
        ("rd_adam_step_clip_ema_dev", (8, "p", "g", "m", "v", 0.9, 0.999, 1e-8, "state", "partial", 1024, "clip", "ema", "ema_cell",
                                       "stream"))],
}


def _opt(clip, ema):
    p = torch.nn.Parameter(torch.arange(N, dtype=torch.float32))
    p.grad = torch.zeros(N)
    kw = dict(max_grad_norm=1.0) if clip else {}
    if ema:
        kw.update(ema_decay=0.9)
    return FlatAdam(p, lr=1e-3, weight_decay=0.01, **kw)


def _names(a):
    """address -> which of the optimizer's buffers it is (looked up after the call: step_captured makes the step cell itself)"""
    named = dict(p=a.param.data, g=a.param.grad, m=a.exp_avg, v=a.exp_avg_sq, state=a.step_cell, partial=a.clip_partial,
                 clip=a.clip_cell, ema=a.ema, ema_cell=a.ema_cell)
    return {t.data_ptr(): k for k, t in named.items() if t is not None}


def _reduced(a, calls):
    names = _names(a)
    out = []
    for name, args in calls:
        row = []
        for x in args:
            if isinstance(x, ctypes.c_void_p):
                x = names[x.value]                                  # (KeyError: a pointer to something that is none of the buffers)
            assert x == "stream" or type(x) in (int, float, str), (name, x)
            row.append(x)
        out.append((name, tuple(row)))
    return out


@pytest.fixture
def calls(monkeypatch):
    log = []
    monkeypatch.setattr(optim._lib, "call", lambda name, *args: log.append((name, args)))
    monkeypatch.setattr(optim.ops, "_stream", lambda: "stream")
    return log


@pytest.mark.parametrize("ema", [False, True], ids=["", "ema"])
@pytest.mark.parametrize("clip", [False, True], ids=["", "clip"])
def test_step_enqueues_the_host_form(calls, clip, ema):
    a = _opt(clip, ema)
    if ema:                                                         # as after a launch of an even step: slot 1 holds the count
        a.ema_cell[2:4] = torch.tensor([7.0, 3.0], dtype=torch.float64)
    a.step()
    want = EXPECTED[(clip, ema, False)]
    assert _reduced(a, calls) == want
    assert a.t == 1 and a._cell_stale and (not ema or a._ema_t == 1) and a.step_cell is None
    if ema:                                                         # the cell was synchronised BEFORE `t` moved: no slot was copied
        assert a.ema_cell.tolist()[2:4] == [7.0, 3.0]
    del calls[:]
    a.step()                                                        # the next one: the same calls with step = 2
    assert _reduced(a, calls) == [(n_, tuple(2 if k == 10 and n_ != "rd_grad_sumsq" else x for k, x in enumerate(r))) for n_, r in want]
    assert a.t == 2 and a._cell_stale and (not ema or a._ema_t == 2)
    if ema:
        assert a.ema_cell.tolist()[2:4] == [7.0, 3.0]
        a.t = 9                                                     # set from outside: the sync in front of `t += 1` sees the jump
        del calls[:]
        a.step()
        assert [c[0] for c in calls] == [w[0] for w in want] and calls[-1][1][10] == 10
        assert a.t == 10 and a._ema_t == 10 and a.ema_cell.tolist()[2:4] == [3.0, 3.0]


@pytest.mark.parametrize("advance", [True, False], ids=["advance", "no_advance"])
@pytest.mark.parametrize("ema", [False, True], ids=["", "ema"])
@pytest.mark.parametrize("clip", [False, True], ids=["", "clip"])
def test_step_captured_enqueues_the_dev_form(calls, clip, ema, advance):
    a = _opt(clip, ema)
    assert a.step_cell is None
    a.step_captured(advance=advance)
    want = EXPECTED[(clip, ema, True)][0 if advance else 1:]
    assert _reduced(a, calls) == want
    # the host's count is the owner's business (note_replay); the step cell exists now and holds the state of t = 0
    assert a.t == 0 and not a._cell_stale and (not ema or a._ema_t == 0)
    assert a.step_cell.tolist() == [0.0, 1.0, 1.0, 1e-3, 0.0, 0.01, 0.0, 0.0]
    cell = a.step_cell.data_ptr()
    a.note_replay()
    assert a.t == 1 and (not ema or a._ema_t == 1)
    del calls[:]
    a.step_captured(advance=advance)                                # the same launches again, on the same cell
    assert _reduced(a, calls) == want and a.step_cell.data_ptr() == cell
    assert a.t == 1 and not a._cell_stale and (not ema or a._ema_t == 1)


def test_default_of_step_captured_is_advance(calls):
    a = _opt(False, False)
    a.step_captured()
    assert _reduced(a, calls) == EXPECTED[(False, False, True)]


@pytest.mark.parametrize("ema", [False, True], ids=["", "ema"])
@pytest.mark.parametrize("clip", [False, True], ids=["", "clip"])
def test_swapped_optimizer_raises_before_anything_is_enqueued(calls, clip, ema):
    a = _opt(clip, ema)
    a.ema_swapped = True
    for f in (a.step, a.step_captured, lambda: a.step_captured(advance=False)):
        with pytest.raises(_lib.RaindropHipError, match="average"):
            f()
    assert calls == [] and a.t == 0 and not a._cell_stale and a.step_cell is None
