"""CPU: the numpy restatement of the flight audit (tests/swarm_audit_reference.py) against closed-form cases: head-on
approach, static and moving cylinders, goal arrival, the switch to a new record, an agent without any record."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swarm_audit_reference as ref  # noqa: E402

CASES = {c["name"]: c for c in ref.closed_form_cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_closed_form(name):
    c = CASES[name]
    acc, events, margins = ref.run_case(c)
    ref.check_expect(c, acc, events)
    assert ref.near_threshold(margins) == 0, "a case decision sits on its threshold"


def test_event_order_and_incremental_fold():
    c = CASES["head_on"]
    acc, events, _ = ref.run_case(c)
    assert events == sorted(events, key=lambda e: (e[0], e[1], e[3], e[2]))
    # two calls of 10 ticks (the second continues from the first's last table) give the one call's result
    a1, e1, _ = ref.audit(c["tables"][:10], None, c["fallback"], c["goals"], c["cyl"], 0.0, 0, 0.1, 0, 2)
    a2, e2, _ = ref.audit(c["tables"][10:], c["tables"][9], c["fallback"], c["goals"], c["cyl"], 0.0, 10, 0.1, 0, 2, acc=a1)
    assert e1 + e2 == events
    for k in acc:
        assert np.array_equal(acc[k], a2[k]), k


def test_whole_samples_only():
    c = CASES["fallback"]
    with pytest.raises(ValueError):
        ref.audit(c["tables"], None, c["fallback"], c["goals"], c["cyl"], 0.0, 0, 0.1, 0, 1, sample_dt=0.03)
