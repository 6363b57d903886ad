"""CPU: conditions on the float64 reference of the token-plan encoder layer alone (tests/plan_layer_ref.py), so that the GPU
comparison of tests/test_plan_layer_gpu.py is known to bite before any kernel runs:

  * every FFN gate of every case lies at least GATE_MARGIN from zero (with the dropout masks too where the case runs with them), and
    between a quarter and three quarters of the gates are open -- both directions of the gate code run, none can flip;
  * G64 has an odd number of 16-row groups (an unowned half chunk that some workgroup must zero), G64e an even one;
  * three wrong references (a live key masked, the heads' V blocks exchanged, two adjacent samples' rows exchanged in plan order)
    each miss the bounds of the float64 tie by at least 10 x on y and on in_proj_weight's gradient."""
import numpy as np
import pytest

from tests import dropout_ref as DR
from tests import plan_layer_ref as PR
from tests.helpers import plan_ref


@pytest.mark.parametrize("width,lset", PR.TIE_CASES, ids=["%s-%s" % c for c in PR.TIE_CASES])
def test_gates_are_decisive_and_balanced(width, lset):
    c = PR.case(width, lset)
    refs = [PR.reference(width, lset)]
    if (width, lset) in PR.DROPOUT_CASES:
        refs += [PR.reference(width, lset, PR.P_DROP), PR.reference(width, lset, PR.P_DROP, None, "padded")]
    assert c["c"] in (2.0, 4.0, 8.0, 16.0, 32.0, 64.0)
    bias = c["p"]["linear1.bias"].numpy()
    assert np.array_equal(bias, c["c"] * np.where(np.arange(c["nhid"]) % 2 == 0, 1.0, -1.0))
    for r in refs:
        pre = r["pre"]
        assert pre.shape == (c["plan"]["mlive"], c["nhid"]) and c["plan"]["mlive"] == int(np.clip(c["lengths"], 0, c["T"]).sum())
        margin, opened = float(np.abs(pre).min()), float((pre > 0).mean())
        print("%s %s: c = %g, min |pre| = %.3f, open %.1f %%" % (width, lset, c["c"], margin, 100 * opened))
        assert margin >= PR.GATE_MARGIN, margin
        assert 0.25 <= opened <= 0.75, opened
        assert all(np.isfinite(v).all() for v in r.values())
    if c["c"] > 2.0:                                   # the smallest such c: half of it leaves a gate inside the margin
        half = PR._evaluate(c, c["p"]["linear1.bias"] * 0.5, grads=False)["pre"]
        rest = [half] + [PR._evaluate(c, c["p"]["linear1.bias"] * 0.5, PR.P_DROP, layout=lay, grads=False)["pre"]
                         for lay in (("plan", "padded") if (width, lset) in PR.DROPOUT_CASES else ())]
        assert min(float(np.abs(q).min()) for q in rest) < PR.GATE_MARGIN


def test_widths_that_reach_the_fused_path():
    """The row-block kernels exist for 5, 9 and 15 reduction chunks of 32; in_proj's input gradient reduces over 3 D.  Of the widths
    attnfuse_ok() admits (D = 136, 144, 152, 160) only 152 and 160 give 15: those run every case, the other two are pinned as
    refusals on the GPU."""
    assert [PR.in_proj_chunks(w) for w in ("W136", "W144", "W152", "W160")] == [13, 14, 15, 15]
    assert set(PR.PLAN_WIDTHS) | set(PR.REFUSED_WIDTHS) == set(PR.WIDTHS) and {w for w, _ in PR.TIE_CASES} == set(PR.PLAN_WIDTHS)
    for w, (F, D, nhid, _) in PR.WIDTHS.items():
        assert D == 4 * F + 16 and -(-D // 32) == 5 and -(-nhid // 32) == 9 and D % 8 == 0


def test_group_count_parity():
    assert PR.groups("G64") == 31 and PR.groups("G64e") == 30
    T, lengths = PR.LENGTHS["G64"]
    assert {1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64} <= set(lengths) and T == 64 and list(lengths) != sorted(lengths, reverse=True)
    pl = plan_ref(lengths, T)
    assert pl["mlive"] == sum(lengths) and (pl["coff"][-1] + 1) // 2 == 16
    assert PR.case("W160", "S7")["plan"]["mlive"] == 11 and PR.groups("S7") == 3
    assert PR.groups("Z33") == 5 and PR.case("W160", "Z33")["plan"]["mlive"] == 53


def test_zero_length_samples_are_absent_from_the_reference():
    """Z33's reference equals the reference of its two live samples alone (same plan rows: the zero-length samples rank last)."""
    c = PR.case("W152", "Z33")
    two = dict(c, lengths=c["lengths"][[0, 2]], B=2, plan=plan_ref(c["lengths"][[0, 2]], c["T"]))
    a, b = PR.reference("W152", "Z33"), PR._evaluate(two, c["p"]["linear1.bias"])
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("variant", PR.VARIANTS)
def test_wrong_references_miss_the_bounds(variant):
    ref, wrong = PR.reference("W160", "G64"), PR.reference("W160", "G64", 0.0, variant)
    for name in ("y", PR.W_IN):
        m = DR.variant_margin({name: ref[name]}, wrong, PR.bound_of)
        print("%s %s: %.1f x the bound" % (variant, name, m))
        assert m >= 10.0, (variant, name, m)
