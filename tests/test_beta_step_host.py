"""CPU: the build-time facts of the use_beta training step (raindrop_amd/step_beta.py, raindrop_amd/csrc/rd_beta_stage.hip) -- the
library cross-compiles with the new unit and exports its C-ABI, the two new layout kernels do not spill, and the flat buffer's
parameter list for the paper's branch is the set the reference's own backward reaches (the fixtures' `live` key)."""
import os
import re

import pytest

from raindrop_amd import _lib, build, synth
from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE = ["rd_beta_stage_workspace_bytes", "rd_beta_stage_saved_bytes", "rd_beta_stage_fwd", "rd_beta_stage_bwd",
         "rd_beta_l2_tokens_fwd", "rd_beta_l2_tokens_bwd"]


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def test_stage_symbols_in_header_table_and_exports(lib):
    assert os.path.join(build.CSRC, "rd_beta_stage.hip") in build.sources()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "raindrop_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rd_[a-z0-9_]+)\s*\(", text))
    for name in STAGE:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.rd_arch() == b"gfx950"


def test_stage_argument_errors_and_sizes(lib):
    import ctypes
    shp = _lib.shape(8, 60, 34, 4)
    sp = ctypes.byref(shp)
    assert lib.rd_beta_stage_saved_bytes(sp, 400) > 8 * 34 * 60 * 32 * 4          # holds H [B,F,T*32] at least
    assert lib.rd_beta_stage_workspace_bytes(sp, 400) > 8 * 34 * 60 * 32 * 4
    bad = _lib.shape(8, 60, 34, 3)                                                # d_ob != 4: refused before any launch
    rc = lib.rd_beta_l2_tokens_fwd(ctypes.byref(bad), 10, None, None, None, None, 152, None, None)
    assert rc == -1 and b"d_ob" in lib.rd_last_error()
    rc = lib.rd_beta_l2_tokens_fwd(sp, 10, None, None, None, None, 152, None, None)
    assert rc == -1 and b"NULL" in lib.rd_last_error()


def test_new_kernels_do_not_spill(lib):
    usage = build.resource_usage()
    for frag in ("k_beta_l2_tokens_fwd", "k_beta_l2_tokens_bwd"):
        hits = [(k, v) for k, v in usage.items() if frag in k]
        assert hits, frag
        for name, u in hits:
            assert u["scratch"] == 0 and u["vgpr_spill"] == 0, (name, u)


@pytest.mark.parametrize("case", ["p19_beta_sparse", "p12_beta_sparse", "wide80_beta_sparse"])
def test_live_parameter_names_beta_is_the_fixture_s_live_set(case):
    g, meta = load_golden(case)
    cfg = synth.make_config(meta["cfg"])
    names = synth.live_parameter_names_beta(cfg)
    assert len(names) == len(set(names))
    assert set(names) == set(str(x) for x in g["live"])
    default = synth.live_parameter_names(cfg)
    extra = ["ob_propagation.increase_dim.weight", "ob_propagation.increase_dim.bias", "ob_propagation.map_weights"]
    assert [n for n in names if n not in extra] == default                       # the default list, order kept
    assert not any(n in default for n in extra)                                  # live_parameter_names itself is unchanged
    i = names.index("ob_propagation.lin_value.bias")
    assert names[i + 1:i + 4] == extra                                           # next to ob_propagation.lin_value.*: forward order
