"""GPU: every form of the captured steps enqueues what tests/golden/step_launches.json says -- entry point by entry point,
argument by argument, buffer by buffer (tests/golden/make_step_launches.py has the format).  The fixture was recorded before the
host layer was restructured into stages and a part table and is never regenerated from later code: a replay is a captured graph,
so equal traces are equal graphs."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_step_launches", os.path.join(GOLDEN, "make_step_launches.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
WANT = json.load(open(os.path.join(GOLDEN, "step_launches.json")))


def test_fixture_covers_every_case():
    assert sorted(WANT) == sorted("%s/%s" % cf for cf in gen.cases())


@pytest.mark.parametrize("cfg_name,form", gen.cases(), ids=["%s-%s" % cf for cf in gen.cases()])
def test_launch_trace_is_the_recorded_one(cfg_name, form):
    got, want = gen.record(cfg_name, form), WANT["%s/%s" % (cfg_name, form)]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "call %d of %s/%s" % (k, cfg_name, form)
    assert len(got) == len(want)
