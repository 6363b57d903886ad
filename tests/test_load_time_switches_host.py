"""CPU: the bookkeeping around tests/test_load_time_switches_gpu.py.

  * INVENTORY.  Every environment switch a HIP source reads inside a `static` initialiser (once per process: no test can flip it
    in-process) is either a case of the GPU file or listed in EXEMPT with its reason -- a switch added later cannot arrive untested.
  * CASE TABLE.  The kernels the GPU file expects in (or bans from) the launch log are names a launch site really reports: string
    literals inside a `check_launch(...)` call of the sources.
  * LAUNCH-LOG HOOKS (include/raindrop_hip_debug.h).  They load without a device; nothing launched -> empty; a call rejected by its
    argument checks records nothing."""
import ctypes
import glob
import os
import re

import pytest

from raindrop_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raindrop_amd", "csrc")

# read-once switches WITHOUT a case of their own, each with the reason
EXEMPT = {
    "RD_SPLITK_WANT": "has an in-process setter (rd_debug_set_splitk_want); the environment only seeds it",
    "RD_RG_ROWS32": "seeds rd_set_rowgemm_rows32; every mask runs in tests/test_rowgemm_variants_gpu.py",
    "RD_RG_WAVES16": "seeds rd_set_rowgemm_waves16; every mask runs in tests/test_rowgemm_variants_gpu.py",
    "RD_PLAN_FIRST": "position of the token-plan workgroup in k_wsplit's grid (first or last blockIdx.y); same kernel, same work per "
                     "workgroup, no launch name to tell the sides apart -- not covered",
    "RD_WSPLIT_GX": "width of k_wsplit's grid (A/B only); the kernel strides over its tiles by gridDim.x -- not covered",
    "RD_K1_WARM": "0 passes null prefetch pointers to the fused message-passing backward: loads whose values are never used -- not covered",
    "RD_CODE_TOUCH": "0 sets the head kernel's own-code prefetch length to zero: no arithmetic depends on it -- not covered",
    "RD_HEAD_NARROW": "0 runs the generic k_head_rows instantiation where the <1, 12, 3> one applies; that instantiation is what every "
                      "wider head runs in test_fused_head_against_float64 -- its use at dh <= 192 is not covered",
    "RD_PANEL_WIDE_COST": "cost constant of panel_form's choice; each form it can choose is forced per call (RD_PANEL_WIDE / RD_PANEL_PC) "
                          "in test_sensor_stage_vs_oracle",
    "RD_PANEL_PC_COST": "as RD_PANEL_WIDE_COST",
}


def _sources():
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")))}


def _static_switches():
    found = set()
    for text in _sources().values():
        for stmt in re.findall(r"\bstatic\b[^;{]*=\s*\[\]\s*\{[^}]*\}", text):
            found.update(re.findall(r'getenv\("(RD_[A-Z0-9_]+)"\)', stmt))
    return found


def _launch_names():
    names = set()
    for text in _sources().values():
        for call in re.findall(r"check_launch\(([^;]*?)\)\s*[;)]", text):
            names.update(re.findall(r'"([A-Za-z0-9_]+)"', call))
        # rd_gemm.hip reports its route's name, check_launch(r.name): the literals of the one function that names a route
        for body in re.findall(r"\nstatic const char\* \w+_name\(const \w+Route& r\) \{\n(.*?)\n\}\n", text, re.S):
            names.update(re.findall(r'"([A-Za-z0-9_]+)"', body))
    return names


def test_every_read_once_switch_is_a_case_or_exempt():
    from tests import test_load_time_switches_gpu as G
    found = _static_switches()
    assert len(found) >= 12, found
    cased = set(G.SWITCHES)
    assert not (cased & set(EXEMPT)), cased & set(EXEMPT)
    assert found == cased | set(EXEMPT), {"read once but neither a case nor exempt": sorted(found - cased - set(EXEMPT)),
                                          "listed but not read once": sorted((cased | set(EXEMPT)) - found)}
    assert all(len(r) > 20 for r in EXEMPT.values())
    # the issue's twelve are cases, not exemptions, and every case but the default sets at least one of them
    assert {"RD_LN_VEC", "RD_LN_FUSE", "RD_LNB_FUSE", "RD_REDUCE_WIDE", "RD_ROWGEMM", "RD_GEMM_XCD", "RD_SPLITK_XCD", "RD_WGRAD_TILE",
            "RD_ATTN_FWD_W8", "RD_ATTN_BWD_W8", "RD_GEMM_PANEL", "RD_GEMM_NPRE"} <= cased
    assert [c for c, (env, _, _, _) in G.CASES.items() if not env] == ["default"]


def test_case_table_names_only_reported_launch_names():
    from tests import test_load_time_switches_gpu as G
    names = _launch_names()
    assert {"k_rowgemm", "k_rowgemm_ln", "k_add_ln_fwd_r3", "k_gemm_bf16x3_128x128", "k_gemm_panel_rowmajor",
            # the tiles only tests/test_gemm_tiles_gpu.py selects: it asserts these names in the launch log
            "k_gemm_bf16x3_128x64", "k_gemm_bf16x3_64x128", "k_gemm_bf16x3_64x160"} <= names
    unknown = []
    for case, (_, probes, expect, _) in G.CASES.items():
        for pattern, want, never in expect:
            re.compile(pattern)
            assert want or never, (case, pattern)
            for w in want + never:
                if not any(G._matches(n, w) for n in names):
                    unknown.append((case, w))
    assert not unknown, unknown


def test_case_probes_exist_and_filters_select_items():
    from tests import switch_child as C
    from tests import test_load_time_switches_gpu as G
    for case, (_, probes, expect, _) in G.CASES.items():
        keys = C.item_keys(probes)
        assert keys and len(set(keys)) == len(keys), case
        for pattern, _, _ in expect:
            assert any(re.search(pattern, k) for k in keys), (case, pattern)
    assert len(C.item_keys(G.ALL)) == len(set(C.item_keys(G.ALL)))


@pytest.fixture(scope="module")
def hooks():
    if not os.path.exists(_lib.LIB_PATH):
        from raindrop_amd import build
        build.build(verbose=False)
    lib = _lib.load()
    on, read = lib.rd_debug_launch_log, lib.rd_debug_launch_log_read
    on.argtypes, on.restype = [ctypes.c_int], None
    read.argtypes, read.restype = [ctypes.c_char_p, ctypes.c_size_t], ctypes.c_size_t
    yield lib, on, read
    on(0)


def test_launch_log_is_empty_until_something_launches(hooks):
    lib, on, read = hooks
    buf = ctypes.create_string_buffer(b"x" * 63, 64)
    assert read(buf, len(buf)) == 0 and buf.value == b""          # off (the default): nothing recorded
    on(1)
    buf = ctypes.create_string_buffer(b"x" * 63, 64)
    assert read(buf, len(buf)) == 0 and buf.value == b""
    assert read(None, 0) == 0                                      # length query


def test_rejected_call_records_nothing(hooks):
    lib, on, read = hooks
    on(1)
    assert lib.rd_linear_fwd(4, 0, 8, None, 8, None, None, None, 8, 0, None) == -1 and b"bad dims" in lib.rd_last_error()
    shp = _lib.shape(2, 5, 3, 4)
    assert lib.rd_msgpass_fwd(ctypes.byref(shp), *([None] * 7), 0.0, 0, None, 12, None, 0, None) == -1
    buf = ctypes.create_string_buffer(64)
    assert read(buf, len(buf)) == 0 and buf.value == b""
    on(0)
