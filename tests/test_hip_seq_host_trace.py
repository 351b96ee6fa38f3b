"""The host code of the seq engines -- the flow's and the behaviour net's inference plans, their training plans under the
fused steps and under autograd, every switch of them -- each on the smallest shape that takes its branches
(tests/seq_host_cases.py), against what the commit named in tests/seq_host_trace.json did: the same native calls in the same
order on the same streams with the same return codes, and bit-identical outputs, gradients and updated parameters."""
import importlib.util
import json
import os

import pytest

import seq_host_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("fused_conv_trace_under_test", os.path.join(ROOT, "tools", "fused_conv_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(os.path.join(ROOT, "tests", "seq_host_trace.json")))


def test_fixture_covers_every_required_entry_point_and_a_second_stream(fixture):
    """No GPU: the recording names its commit, holds every case, reaches every entry point of seq_host_cases.REQUIRED and
    has calls on a second stream."""
    assert fixture["header"].startswith("recorded from commit ")
    assert set(fixture["cases"]) == set(sc.CASES)
    assert sc.missing_coverage(fixture["cases"]) == []


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sc.CASES))
def test_case_does_what_the_recording_did(fixture, name):
    rec, raw = sc.record_case(name)
    assert _tool().compare(fixture, name, rec, raw) == []
