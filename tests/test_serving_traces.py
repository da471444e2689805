"""CPU: plan_online's traces over the seeded cases of _serving_cases.py equal, digest for digest, those recorded in
serving_traces.json by tools/record_serving_traces.py on the commit named there -- the schedule as it was before Scheduler and
plan_online shared one step driver.  The file is a pin, not a snapshot to refresh (see the tool's docstring)."""
import hashlib
import json
import os

import pytest

from gsv.serving import plan_online
from _serving_cases import TRACE_SEEDS, TRACE_VARIANTS, trace_case

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "serving_traces.json")) as _f:
    RECORDED = json.load(_f)["digests"]


def test_every_variant_and_seed_is_recorded():
    assert sorted(RECORDED) == sorted(TRACE_VARIANTS) and all(len(RECORDED[v]) == len(TRACE_SEEDS) == 200 for v in TRACE_VARIANTS)


@pytest.mark.parametrize("variant", TRACE_VARIANTS)
def test_traces_equal_the_recorded_ones(variant):
    bad = [s for s in TRACE_SEEDS
           if hashlib.sha256(repr(plan_online(**trace_case(s, variant), with_steps=True)).encode()).hexdigest() != RECORDED[variant][s]]
    assert bad == [], f"{variant}: the traces of seeds {bad} differ from the recorded ones"
