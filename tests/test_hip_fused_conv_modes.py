"""The host modes of ops.FusedConv and of the deferred weight-gradient queue, each on a shape of its own that runs in a
moment (tests/fused_conv_cases.py), against what the commit named in tests/fused_conv_trace.json did: the same native
calls in the same order on the same streams with the same return codes, the same profiler records, and bit-identical
outputs, input gradients and parameter gradients."""
import importlib.util
import json
import os

import pytest

import fused_conv_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("fused_conv_trace_under_test", os.path.join(ROOT, "tools", "fused_conv_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(os.path.join(ROOT, "tests", "fused_conv_trace.json")))


def test_fixture_covers_every_required_entry_point(fixture):
    """No GPU: the recording names its commit, holds every case and reaches every entry point / return code of
    fused_conv_cases.REQUIRED."""
    assert fixture["header"].startswith("recorded from commit ")
    assert set(fixture["cases"]) == set(fc.CASES)
    assert fc.missing_coverage(fixture["cases"]) == []


def test_descriptor_builders_state_each_geometry_once():
    """No GPU: the data gradient reads dy as the source of a transposed gather over the forward's input map; the weight
    gradient's flags follow the scheme (f32: bit 0, x6: none, h2: bit 1)."""
    from behavior_driven_video_synthesis_amd import ops
    d = ops._dgrad_desc(2, 64, 8, 8, 16, 16, 16, 3, 2, 1, 32, m_off=32, aux_act=ops.ACT_ELU, aux_drop_p=0.1, aux_drop_seed=5)
    assert (d.mode, d.C1, d.C2, d.Hs, d.Ws, d.M, d.m_off, d.Ho, d.Wo, d.stride) == (1, 64, 0, 8, 8, 16, 32, 16, 16, 2)
    assert (d.in_act, d.drop_p, d.aux_act, d.aux_drop_seed) == (ops.ACT_NONE, 0.0, ops.ACT_ELU, 5)
    f = ops._fwd_desc(2, 16, 16, 16, 16, 64, 8, 8, 3, 2, 1, 64, ops.ACT_ELU, 0.0, 0.1, 7, ops.ACT_RELU, 1)
    assert (f.mode, f.C1, f.C2, f.M, f.Mpad, f.Ho, f.drop_seed, f.out_act, f.d2s, f.aux_act) == (0, 16, 16, 64, 64, 8, 7, ops.ACT_RELU, 1, 0)
    assert [ops._wgrad_desc(2, 16, 0, 8, 8, 32, 8, 8, 3, 1, 1, s).flags for s in (0, 1, 2)] == [1, 0, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(fc.CASES))
def test_mode_does_what_the_recording_did(fixture, name):
    rec, raw = fc.record_case(name)
    assert _tool().compare(fixture, name, rec, raw) == []
