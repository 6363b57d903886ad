"""CPU: the host side of FlatAdam's global-norm clipping / non-finite guard (`max_grad_norm`) -- keyword validation, what a captured
step holds as a constant, the state_dict round trip (old dictionaries included) -- and the argument checks of the new C-ABI entry
points, which answer RD_EINVAL before anything is launched (no device is touched here)."""
import ctypes
import math

import pytest
import torch

from raindrop_amd import _lib
from raindrop_amd.optim import FlatAdam


def _param(n=8):
    p = torch.nn.Parameter(torch.zeros(n))
    p.grad = torch.zeros(n)
    return p


def test_keyword_validation():
    off = FlatAdam(_param(), lr=1e-4)
    assert off.max_grad_norm is None and off.clip_cell is None and off.clip_partial is None
    assert off.hyper() == (0.9, 0.999, 1e-8)                      # off: the constants of an optimizer without the keyword
    for good in (1.0, 0.25, 3, math.inf):
        a = FlatAdam(_param(), max_grad_norm=good)
        assert a.max_grad_norm == float(good) and a.hyper() != off.hyper()       # on / off are different captures
        assert a.clip_cell.dtype == torch.float64 and a.clip_cell.tolist() == [float(good)] + [0.0] * 7
        assert a.clip_partial.dtype == torch.float64 and a.clip_partial.numel() * 8 == _lib.load().rd_grad_sumsq_bytes()
    for bad in (0.0, -1.0, -math.inf, math.nan, "1.0", True, [1.0]):
        with pytest.raises(ValueError):
            FlatAdam(_param(), max_grad_norm=bad)
    a = FlatAdam(_param(), max_grad_norm=2.0)
    for bad in (0.0, -3.0, math.nan, None):
        with pytest.raises(ValueError):
            a.set_max_grad_norm(bad)
    assert a.max_grad_norm == 2.0
    with pytest.raises(ValueError):
        off.set_max_grad_norm(1.0)                                # the launches differ: on is decided at construction
    with pytest.raises(ValueError):
        off.grad_stats()


def test_threshold_changes_are_cell_updates_not_new_constants():
    a = FlatAdam(_param(), max_grad_norm=2.0)
    h = a.hyper()
    a.set_max_grad_norm(0.5)
    assert a.hyper() == h and a.clip_cell[0].item() == 0.5
    a.max_grad_norm = math.inf                                    # plain assignment: pushed by the sync TrainStep.run_full calls
    a.sync_clip_cell()
    assert a.hyper() == h and a.clip_cell[0].item() == math.inf
    assert a.grad_stats() == dict(norm=0.0, scale=0.0, skipped=0, clipped=0)


def test_state_dict_round_trip_and_old_dictionaries():
    a = FlatAdam(_param(), max_grad_norm=2.0)
    a.clip_cell[3:5] = torch.tensor([3.0, 5.0], dtype=torch.float64)          # as if three steps were skipped and five clipped
    sd = a.state_dict()
    assert sd["max_grad_norm"] == 2.0 and sd["grad_skipped"] == 3 and sd["grad_clipped"] == 5
    b = FlatAdam(_param(), max_grad_norm=7.0)
    cell = b.clip_cell.data_ptr()
    b.load_state_dict(dict(sd, t=4))
    assert b.t == 4 and b.max_grad_norm == 2.0 and b.clip_cell.data_ptr() == cell         # in place: a captured step stays valid
    assert b.clip_cell.tolist()[0] == 2.0 and b.grad_stats()["skipped"] == 3 and b.grad_stats()["clipped"] == 5
    c = FlatAdam(_param())                                        # off -> on by a dictionary that has it on
    c.load_state_dict(sd)
    assert c.max_grad_norm == 2.0 and c.grad_stats()["clipped"] == 5 and c.hyper() == a.hyper()
    old = {k: v for k, v in sd.items() if k not in ("max_grad_norm", "grad_skipped", "grad_clipped")}
    b.load_state_dict(dict(old, t=9))                             # a dictionary from before the keyword: setting and counts stay
    assert b.t == 9 and b.max_grad_norm == 2.0 and b.grad_stats()["skipped"] == 3
    d = FlatAdam(_param())
    d.load_state_dict(old)
    assert d.max_grad_norm is None and d.clip_cell is None
    sd_off = d.state_dict()
    assert sd_off["max_grad_norm"] is None and sd_off["grad_skipped"] == 0 and sd_off["grad_clipped"] == 0


def test_entry_points_refuse_bad_arguments_before_launch():
    lib = _lib.load()
    G, nbytes = lib.rd_grad_sumsq_grid(), lib.rd_grad_sumsq_bytes()
    assert G > 0 and nbytes == 8 * G
    buf = (ctypes.c_double * (4 * G + 16))()                      # host memory: only its ADDRESS is looked at
    a = (ctypes.addressof(buf) + 15) & ~15                        # 16-byte aligned
    ok = [a, a + 64, a + 128, a + 192]                            # param, grad, exp_avg, exp_avg_sq
    part, cell, state = a + 256, a + 256 + nbytes, a + 320 + nbytes
    EINVAL = -1

    def bad(rc, word):
        assert rc == EINVAL and word in lib.rd_last_error(), (rc, lib.rd_last_error())

    bad(lib.rd_grad_sumsq(16, None, part, nbytes, None), b"NULL")
    bad(lib.rd_grad_sumsq(16, ok[1], None, nbytes, None), b"NULL")
    bad(lib.rd_grad_sumsq(0, ok[1], part, nbytes, None), b"bad n")
    bad(lib.rd_grad_sumsq(-5, ok[1], part, nbytes, None), b"bad n")
    bad(lib.rd_grad_sumsq(16, ok[1] + 4, part, nbytes, None), b"aligned")
    bad(lib.rd_grad_sumsq(16, ok[1], part + 8, nbytes, None), b"aligned")
    bad(lib.rd_grad_sumsq(16, ok[1], part, nbytes - 8, None), b"too small")

    def host(n=16, ptrs=ok, step=1, partial=part, pb=nbytes, clip=cell):
        return lib.rd_adam_step_clip(n, *ptrs, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, partial, pb, clip, None)

    def dev(n=16, ptrs=ok, st=state, partial=part, pb=nbytes, clip=cell):
        return lib.rd_adam_step_clip_dev(n, *ptrs, 0.9, 0.999, 1e-8, st, partial, pb, clip, None)

    for f in (host, dev):
        bad(f(n=0), b"bad n")
        for k in range(4):
            bad(f(ptrs=ok[:k] + [None] + ok[k + 1:]), b"NULL")
            bad(f(ptrs=ok[:k] + [ok[k] + 4] + ok[k + 1:]), b"aligned")
        bad(f(partial=None), b"NULL")
        bad(f(clip=None), b"NULL")
        bad(f(partial=part + 8), b"aligned")
        bad(f(clip=cell + 8), b"aligned")
        bad(f(pb=nbytes - 1), b"too small")
    bad(host(step=0), b"bad step")
    bad(dev(st=None), b"state")
    bad(dev(st=state + 8), b"state")
