"""CPU: the structure-distance gradient fixtures (tests/golden/make_distance_goldens.py, made by the reference's own autograd) --
re-checked against the independent restatement (oracle O2) everywhere, regenerated from the reference itself where its tree is
present -- and the argument checks of the new C-ABI entry points (no device needed)."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from oracle import ref_loader, restatement as O2
from raindrop_amd import _lib, synth
from tests.helpers import GOLDEN, case_inputs, load_golden, oracle_params

DIST_CASES = ["p19_beta_sparse", "p12_beta_sparse", "wide80_beta_sparse"]


def _gen():
    spec = importlib.util.spec_from_file_location("make_distance_goldens", os.path.join(GOLDEN, "make_distance_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", DIST_CASES)
def test_restatement_distance_gradient_matches_golden(name):
    """d distance (code/models_rd.py:345-346) of the restatement's use_beta forward equals the reference's, stored in the fixture"""
    g, meta = load_golden(name + "_distance")
    cfg, gs, batch = case_inputs(meta)
    dlive = [str(x) for x in g["dlive"]]
    p = oracle_params(meta)
    for n in dlive:
        p[n].requires_grad_(True)
    _, dist = O2.raindrop_v2_forward(p, cfg, batch["src"], batch["static"], batch["times"], batch["lengths"], gs, faithful=True,
                                     use_beta=True)
    assert abs(float(dist) - float(g["distance"])) <= 1e-6 * float(g["distance"])
    grads = dict(zip(dlive, torch.autograd.grad(dist, [p[n] for n in dlive])))
    for n in dlive:
        exp = g["dist/grad/" + n]
        got = grads[n].reshape(-1)[:: int(g["dist/gradstride/" + n])].numpy()
        assert np.abs(got - exp).max() <= 1e-4 * np.abs(exp).max(), n
        assert abs(grads[n].double().norm().item() - float(g["dist/gradnorm/" + n])) <= 1e-4 * float(g["dist/gradnorm/" + n]), n
    assert float(g["lam"]) == meta["lam"] > 0.0


@pytest.mark.skipif(not ref_loader.available(), reason="reference tree not present")
@pytest.mark.parametrize("name", DIST_CASES + ["beta_distance_op"])
def test_fixture_regenerates_from_the_reference(name):
    gen = _gen()
    if name == gen.OP_NAME:
        out = gen.op_case()
        with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
            g = {k: z[k] for k in z.files}
    else:
        g, meta = load_golden(name + "_distance")
        out = gen.model_case(name, batch_seed=meta["batch_seed"])
    assert sorted(out) == sorted(g)
    # The reference runs on CPU torch, whose fp32 reductions split their sums by the number of threads: a regeneration on another
    # machine agrees to rounding (measured up to 3e-6 of a tensor's max-norm), not bit for bit.
    for k, v in out.items():
        v, ref = np.asarray(v), g[k]
        if k == "meta":
            got, want = json.loads(str(v)), json.loads(str(ref))
            for key in ("batch_seed", "lam"):
                assert got[key] == want[key], key
            continue
        if v.dtype.kind in "iuUSb":
            assert np.array_equal(v, ref), k
        elif "/gradsum/" in k:            # a sum of both signs over many entries: |d sum| <= sqrt(n) |d grad|, bounded by the norm
            assert abs(float(v) - float(ref)) <= 1e-3 * float(g[k.replace("/gradsum/", "/gradnorm/")]), k
        else:
            assert v.shape == ref.shape and np.abs(v - ref).max() <= 1e-4 * (np.abs(ref).max() + 1e-30), k


def test_distance_backward_argument_checks():
    lib = _lib.load() if os.path.exists(_lib.LIB_PATH) else None
    if lib is None:
        from raindrop_amd import build
        build.build(verbose=False)
        lib = _lib.load()
    assert lib.rd_structure_distance_bwd_workspace_bytes(578, 256) == 256 * 256 * 4
    assert lib.rd_structure_distance_bwd_workspace_bytes(0, 0) == 0
    assert lib.rd_structure_distance_bwd(5, 0, None, None, None, 0, None, None) == -1 and b"bad dims" in lib.rd_last_error()
    assert lib.rd_structure_distance_bwd(5, 4, None, None, None, 64, None, None) == -1 and b"NULL" in lib.rd_last_error()
    # the alpha-cotangent backward checks its arguments like rd_graph_beta_bwd: d_ob must be 4, tensors non-NULL
    assert lib.rd_graph_beta_bwd_alpha(2, 6, 15, 5, 3, 10, *([None] * 4), 0, None, 10, None, 0, *([None] * 8), None, 0, None) == -2
    assert lib.rd_graph_beta_bwd_alpha(2, 6, 20, 5, 4, 10, *([None] * 4), 0, None, 10, None, 0, *([None] * 8), None, 0, None) == -1
    assert b"NULL" in lib.rd_last_error()
