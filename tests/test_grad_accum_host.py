"""CPU: gradient accumulation -- what `fit` refuses without a device, its window arithmetic, the two C-ABI symbols in the header and
the ctypes table, their argument checks (RD_EINVAL before any launch; an empty buffer is legal), and the host-side refusals of the
`accumulate` keyword that need no step to be built."""
import ctypes
import os
import re
import types

import pytest

from raindrop_amd import _lib, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rd_grad_accumulate", "rd_grad_accumulate_close")


def _ds():
    return types.SimpleNamespace(y=[0, 1])


@pytest.mark.parametrize("bad", [0, -1, 2.5, "2", True, None])
def test_fit_refuses_a_bad_accumulate(bad):
    with pytest.raises(ValueError, match="accumulate"):
        trainer._check_fit_args(_ds(), _ds(), 1, 8, 2, accumulate=bad)


@pytest.mark.parametrize("good", [1, 2, 7])
def test_fit_accepts_a_positive_integer(good):
    trainer._check_fit_args(_ds(), _ds(), 1, 8, 2, accumulate=good)
    trainer._check_fit_args(_ds(), _ds(), 1, 8, 2)                             # the default


@pytest.mark.parametrize("n_batches,k,steps,last", [(7, 2, 4, 1), (8, 4, 2, 4), (1, 4, 1, 1), (5, 1, 5, 1), (0, 3, 0, 0), (9, 3, 3, 3)])
def test_window_arithmetic(n_batches, k, steps, last):
    """optimizer steps = ceil(n_batches / k); every window but the last is full and no micro-batch is dropped"""
    assert trainer._window_plan(n_batches, k) == (steps, last)
    assert steps == -(-n_batches // k) and (steps == 0 or (steps - 1) * k + last == n_batches) and 0 <= last <= k


def test_symbols_in_header_and_table():
    text = open(os.path.join(ROOT, "include", "raindrop_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(rd_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
    P = ctypes.c_void_p
    assert _lib.SIGNATURES["rd_grad_accumulate"] == (ctypes.c_int32, [ctypes.c_int64, P, P, P])
    assert _lib.SIGNATURES["rd_grad_accumulate_close"] == (ctypes.c_int32, [ctypes.c_int64, P, P, P, P])


def test_argument_errors_are_reported_before_launch():
    """NULL / misaligned pointers and n < 0 come back as RD_EINVAL with a message; n == 0 is RD_OK without a launch (no device here)"""
    if not os.path.exists(_lib.LIB_PATH):
        from raindrop_amd import build
        build.build(verbose=False)
    lib = _lib.load()
    a, b, cell = 0x1000, 0x2000, 0x3000                                        # never dereferenced: every call below returns first

    def bad(rc, what):
        assert rc == -1 and what in lib.rd_last_error(), (rc, lib.rd_last_error())
    bad(lib.rd_grad_accumulate(-1, a, b, None), b"bad n")
    bad(lib.rd_grad_accumulate(8, None, b, None), b"NULL")
    bad(lib.rd_grad_accumulate(8, a, None, None), b"NULL")
    bad(lib.rd_grad_accumulate(8, a + 4, b, None), b"aligned")
    bad(lib.rd_grad_accumulate(8, a, b + 8, None), b"aligned")
    bad(lib.rd_grad_accumulate_close(-3, a, b, cell, None), b"bad n")
    bad(lib.rd_grad_accumulate_close(8, None, b, cell, None), b"NULL")
    bad(lib.rd_grad_accumulate_close(8, a, None, cell, None), b"NULL")
    bad(lib.rd_grad_accumulate_close(8, a, b, None, None), b"NULL")
    bad(lib.rd_grad_accumulate_close(8, a + 4, b, cell, None), b"aligned")
    bad(lib.rd_grad_accumulate_close(8, a, b + 12, cell, None), b"aligned")
    bad(lib.rd_grad_accumulate_close(8, a, b, cell + 2, None), b"aligned")
    assert lib.rd_grad_accumulate(0, a, b, None) == 0
    assert lib.rd_grad_accumulate_close(0, a, b, cell, None) == 0
