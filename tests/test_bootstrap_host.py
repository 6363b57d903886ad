"""CPU: the host surface of the bootstrap of the validation metrics -- the header declares the four functions and the library
refuses what lies outside their envelope without touching a device; `metrics.rank_bootstrap` refuses CPU tensors and bad shapes;
`feed.validate` / `validate_ema` / `trainer.fit` take and check the new keywords."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from raindrop_amd import _lib, feed, metrics, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rd_rank_bootstrap_workspace_bytes", "rd_rank_bootstrap", "rd_rank_bootstrap_summary", "rd_rank_bootstrap_counts")


def test_header_declares_the_four_functions_and_the_rule():
    text = open(os.path.join(ROOT, "include", "raindrop_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SIGNATURES
    for phrase in ("SITE_BOOTSTRAP", "floor(word * N / 2^32)", "N <= 16384", "R <= 4096", "[2][C + 1][5]"):
        assert phrase in text, phrase
    rng = open(os.path.join(ROOT, "raindrop_amd", "csrc", "rd_rng.h")).read()
    assert re.search(r"SITE_BOOTSTRAP\s*=\s*84\b", rng)
    dbg = open(os.path.join(ROOT, "include", "raindrop_hip_debug.h")).read()
    assert all(k in dbg for k in ("k_boot_sort", "k_boot_stats", "k_boot_means", "k_boot_summary", "k_boot_counts"))


def test_envelope_is_refused_without_a_device():
    lib = _lib.load()
    ws = lib.rd_rank_bootstrap_workspace_bytes
    assert ws(3880, 2, 1000) == 3880 * 2 * 2 and ws(16384, 8, 4096) == 16384 * 8 * 2
    assert ws(16385, 2, 10) == 0 and ws(10, 2, 4097) == 0 and ws(0, 2, 10) == 0 and ws(10, 0, 10) == 0 and ws(10, 65536, 10) == 0
    for N, C, R in ((16385, 2, 10), (10, 2, 4097), (10, 2, 0), (0, 2, 10), (10, 65536, 10)):
        rc = lib.rd_rank_bootstrap(N, C, None, C, None, R, 0, None, None, None, None, None, None, 0, None)
        assert rc == -2 and b"outside" in lib.rd_last_error(), (N, C, R)
    assert lib.rd_rank_bootstrap(10, 2, None, 2, None, 10, 0, None, None, None, None, None, None, 0, None) == -1
    assert b"NULL" in lib.rd_last_error()
    assert lib.rd_rank_bootstrap(10, 2, None, 1, None, 10, 0, None, None, None, None, None, None, 0, None) == -1
    assert lib.rd_rank_bootstrap_summary(4097, 2, None, None, None, 0.05, None, None) == -2
    assert lib.rd_rank_bootstrap_summary(10, 2, None, None, None, 1.0, None, None) == -1 and b"alpha" in lib.rd_last_error()
    assert lib.rd_rank_bootstrap_summary(10, 2, None, None, None, 0.05, None, None) == -1
    assert lib.rd_rank_bootstrap_counts(16385, 10, 0, 0, 1, None, None) == -2
    assert lib.rd_rank_bootstrap_counts(10, 10, 0, 8, 3, None, None) == -1 and b"bad rows" in lib.rd_last_error()
    assert lib.rd_rank_bootstrap_counts(10, 10, 0, 0, 0, None, None) == 0               # no rows: nothing to launch
    assert lib.rd_rank_bootstrap_counts(10, 10, 0, 0, 1, None, None) == -1


def test_rank_bootstrap_refuses_cpu_tensors_and_bad_shapes():
    assert inspect.signature(metrics.rank_bootstrap).parameters["n_boot"].default == 1000
    assert [inspect.signature(metrics.rank_bootstrap).parameters[k].default for k in ("seed", "alpha", "out", "workspace")] == [0, 0.05, None, None]
    assert callable(metrics.bootstrap_workspace)
    s, y = torch.zeros((5, 2)), torch.zeros(5, dtype=torch.int64)
    with pytest.raises(_lib.RaindropHipError, match="no CPU fallback"):
        metrics.rank_bootstrap(s, y, n_boot=4)
    with pytest.raises(_lib.RaindropHipError):
        metrics.rank_bootstrap(s.numpy(), y, n_boot=4)
    if torch.cuda.is_available():
        sd, yd = s.cuda(), y.cuda()
        for bad_s, bad_y in ((sd.double(), yd), (sd[:, 0], yd), (sd, yd[:4]), (sd, yd.int()), (sd.t(), yd)):
            with pytest.raises(_lib.RaindropHipError):
                metrics.rank_bootstrap(bad_s, bad_y, n_boot=4)
        with pytest.raises(ValueError, match="alpha"):
            metrics.rank_bootstrap(sd, yd, n_boot=4, alpha=1.5)


BAD = [dict(bootstrap=0), dict(bootstrap=4097), dict(bootstrap=2.5), dict(bootstrap=True), dict(bootstrap="100"),
       dict(bootstrap=10, bootstrap_seed=-1), dict(bootstrap=10, bootstrap_seed=1.5), dict(bootstrap=10, bootstrap_seed=2 ** 64)]


@pytest.mark.parametrize("kw", BAD + [dict(bootstrap=10, ci=0.0), dict(bootstrap=10, ci=1.0), dict(bootstrap=10, ci="95")], ids=str)
def test_validate_checks_the_keywords_before_anything_runs(kw):
    ds = SimpleNamespace(y=None)
    with pytest.raises(ValueError, match="bootstrap|ci must"):
        feed.validate(None, ds, **kw)
    with pytest.raises(ValueError, match="bootstrap|ci must"):
        feed.check_bootstrap(kw.get("bootstrap"), kw.get("bootstrap_seed", 0), kw.get("ci", 0.95))


def test_validate_accepts_the_keywords():
    p = inspect.signature(feed.validate).parameters
    assert (p["bootstrap"].default, p["bootstrap_seed"].default, p["ci"].default) == (None, 0, 0.95)
    feed.check_bootstrap(None)
    feed.check_bootstrap(1, 0, 0.5)
    feed.check_bootstrap(np.int64(4096), 2 ** 64 - 1, 0.99)
    with pytest.raises(_lib.RaindropHipError, match="labels"):            # good keywords: the next refusal is the old one
        feed.validate(None, SimpleNamespace(y=None), bootstrap=64, bootstrap_seed=3, ci=0.9)
    assert any(q.kind is inspect.Parameter.VAR_KEYWORD for q in inspect.signature(feed.validate_ema).parameters.values())


@pytest.mark.parametrize("kw", BAD, ids=str)
def test_fit_checks_the_keywords_without_a_device(kw):
    ds = SimpleNamespace(y=torch.zeros(4, dtype=torch.int64), N=4)
    with pytest.raises(ValueError, match="bootstrap"):
        trainer.fit(None, ds, ds, 1, batch_size=2, **kw)


def test_fit_accepts_the_keywords():
    p = inspect.signature(trainer.fit).parameters
    assert (p["bootstrap"].default, p["bootstrap_seed"].default) == (None, 0)
    ds = SimpleNamespace(y=torch.zeros(4, dtype=torch.int64), N=4)
    trainer._check_fit_args(ds, ds, 1, 2, 2, bootstrap=1000, bootstrap_seed=7)
    trainer._check_fit_args(ds, ds, 1, 2, 2)
