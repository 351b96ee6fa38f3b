"""The collector guard of the graph recorder (ops._collector_off, the part of ops._graph_recording that needs no device)."""
import gc

import pytest

from behavior_driven_video_synthesis_amd.ops import _collector_off


@pytest.fixture(autouse=True)
def _collector_as_found():
    was_on = gc.isenabled()
    yield
    gc.enable() if was_on else gc.disable()


def test_collector_is_off_inside_and_back_on_after():
    gc.enable()
    with _collector_off():
        assert not gc.isenabled()
    assert gc.isenabled()


def test_collector_comes_back_when_the_body_raises():
    gc.enable()
    with pytest.raises(KeyError):
        with _collector_off():
            assert not gc.isenabled()
            raise KeyError("the body failed")
    assert gc.isenabled()


def test_a_collector_that_was_off_stays_off():
    gc.disable()
    with _collector_off():
        assert not gc.isenabled()
    assert not gc.isenabled()
    with pytest.raises(KeyError):
        with _collector_off():
            raise KeyError("the body failed")
    assert not gc.isenabled()


def test_nested_guards_restore_in_order():
    gc.enable()
    with _collector_off():
        with _collector_off():
            assert not gc.isenabled()
        assert not gc.isenabled()
    assert gc.isenabled()
