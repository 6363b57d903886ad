"""No GPU: the mask settings of tests/test_rowgemm_variants_gpu.py reach every k_rowgemm instantiation of the built library.

`raindrop_amd/csrc/rd_rowgemm.hip` builds the row-block product 21 times; launch_rowgemm / launch_rowgemm_ln / launch_rowgemm_lnb
pick one by reduction length and by the bits of the two masks (rd_set_rowgemm_rows32 / rd_set_rowgemm_waves16: 1 plain K <= 160,
2 plain K <= 288, 4 LayerNorm epilogue, 8 LayerNorm-backward prologue).  The dispatch is mirrored here in a few lines of Python and
evaluated over the GPU module's SETTINGS: an instantiation added to the library, or a candidate added to TrainStep's autotune,
without a test setting that runs it fails here."""
import re

import pytest

from raindrop_amd import build
from raindrop_amd.step import TrainStep
from tests.test_rowgemm_variants_gpu import CORNERS, REFERENCE, SETTINGS

# template arguments <KC, ROWS, NJ, LN, LNB, WV>


def _form(kc, rows32, waves16, ln=0, lnb=0):
    return (kc, 32 if rows32 else 64, 1 if waves16 else 2, ln, lnb, 16 if waves16 else 8)


def plain(kc, r32, w16):
    """launch_rowgemm: reduction steps kc = ceil(K / 32)"""
    if kc == 15:
        return (15, 32, 1, 0, 0, 8)                    # K = 3D: one form
    bit = {5: 1, 9: 2}[kc]
    return _form(kc, r32 & bit, w16 & bit)


def ln_epilogue(kc, r32, w16):
    """launch_rowgemm_ln: KP == 160 -> KC 5, otherwise 9"""
    return _form(kc, r32 & 4, w16 & 4, ln=1)


def ln_backward(r32, w16):
    """launch_rowgemm_lnb: K = LayerNorm width, KC 5"""
    return _form(5, r32 & 8, w16 & 8, lnb=1)


def selected(r32, w16):
    """what one encoder layer (forward + backward, row-block path, widths with ceil(D / 32) = 5, ceil(nhid / 32) = 9) launches:
    in_proj, linear1 and the out_proj / linear2 input gradients (plain, K = D or nhid), out_proj + LayerNorm1 (K = D),
    linear2 + LayerNorm2 (K = nhid), the two LayerNorm-backward prologues (K = D) and the K = 3D product"""
    return {plain(5, r32, w16), plain(9, r32, w16), plain(15, r32, w16), ln_epilogue(5, r32, w16), ln_epilogue(9, r32, w16),
            ln_backward(r32, w16)}


BUILT = ([(kc, rows, nj, 0, 0, wv) for kc in (5, 9) for rows in (32, 64) for nj, wv in ((2, 8), (1, 16))] + [(15, 32, 1, 0, 0, 8)] +
         [(kc, rows, nj, 1, 0, wv) for kc in (5, 9) for rows in (32, 64) for nj, wv in ((2, 8), (1, 16))] +
         [(5, rows, nj, 0, 1, wv) for rows in (32, 64) for nj, wv in ((2, 8), (1, 16))])


def _fragment(t):
    return "k_rowgemmILi%dELi%dELi%dELb%dELb%dELi%dE" % t


@pytest.fixture(scope="module")
def usage():
    build.build(verbose=False)
    u = build.resource_usage()
    assert len(u) > 100, "no resource-usage records: was the library built by raindrop_amd.build?"
    return u


def test_library_holds_exactly_the_21_row_block_instantiations(usage):
    assert len(BUILT) == 21 and len(set(BUILT)) == 21
    names = [k for k in usage if "k_rowgemmI" in k]
    found = set()
    for k in names:
        m = re.search(r"k_rowgemmILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])ELi(\d+)E", k)
        assert m, k
        found.add(tuple(int(v) for v in m.groups()))
    assert len(names) == 21, sorted(names)
    assert found == set(BUILT), (sorted(found - set(BUILT)), sorted(set(BUILT) - found))
    for t in BUILT:
        assert sum(_fragment(t) in k for k in names) == 1, t


def test_dispatch_mirror_matches_the_launchers():
    """the mirror against the source it mirrors: every launch_rowgemm_kc<...> the three launchers name is a form the mirror can
    return, and the other way round"""
    import os
    src = open(os.path.join(build.CSRC, "rd_rowgemm.hip")).read()
    host = src[src.index("bool rowgemm_ln_ok"):]
    named = set()
    for m in re.finditer(r"launch_rowgemm_kc<([^>]*)>", host):
        a = [v.strip() for v in m.group(1).split(",")]
        a += ["false", "false", "8"][len(a) - 3:]                          # defaults: LN = false, LNB = false, WV = 8
        named.add((int(a[0]), int(a[1]), int(a[2]), int(a[3] == "true"), int(a[4] == "true"), int(a[5])))
    mirror = set()
    for r32 in range(16):
        for w16 in range(16):
            mirror |= selected(r32, w16)
    assert named == mirror == set(BUILT), (sorted(named ^ mirror), sorted(mirror ^ set(BUILT)))


def test_settings_select_every_instantiation():
    assert selected(*REFERENCE) == {(5, 32, 2, 0, 0, 8), (9, 32, 2, 0, 0, 8), (15, 32, 1, 0, 0, 8), (5, 32, 1, 1, 0, 16),
                                    (9, 32, 1, 1, 0, 16), (5, 32, 1, 0, 1, 16)}       # the six forms the rest of the suite runs
    reached = set()
    for r32, w16 in SETTINGS:
        reached |= selected(r32, w16)
    assert reached == set(BUILT), sorted(set(BUILT) - reached)
    corners = set()
    for r32, w16 in CORNERS:                            # the large shape runs the corners only: they must suffice
        corners |= selected(r32, w16)
    assert corners == set(BUILT), sorted(set(BUILT) - corners)


def test_settings_hold_every_pair_the_autotune_can_leave_behind():
    assert TrainStep.TUNE_WAVES[0] == REFERENCE[1] and REFERENCE[0] in TrainStep.TUNE_HEIGHTS
    for h in TrainStep.TUNE_HEIGHTS:
        for w in TrainStep.TUNE_WAVES:
            assert (h, w) in SETTINGS, (h, w)
