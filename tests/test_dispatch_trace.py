"""What the controllers hand the HIP bindings, pinned on the CPU (tests/dispatch_trace.py).

Every scenario's recorded calls -- group tuples, qk_src, store targets, slots, fold tuples, the
latent step's arguments, and the stores' layout after each step -- must equal the golden trace."""
import json

import pytest

import dispatch_trace as dt


@pytest.fixture(scope="module")
def traced():
    with open(dt.GOLDEN) as f:
        golden = json.load(f)
    return golden, dt.trace(dt.load())


def test_scenarios_are_the_goldens(traced):
    golden, got = traced
    assert sorted(got) == sorted(golden["scenarios"])


@pytest.mark.parametrize("name", sorted(dt.scenarios(dt.load())))
def test_dispatch_trace(traced, name):
    golden, got = traced
    want = [golden["records"][i] for i in golden["scenarios"][name]]
    have = json.loads(json.dumps(got[name]))
    assert len(have) == len(want)
    for n, (h, w) in enumerate(zip(have, want)):
        assert h == w, f"{name}: event {n} differs"
