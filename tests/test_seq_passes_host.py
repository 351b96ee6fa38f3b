"""The bookkeeping of the training engines' pass slots (``seq_passes.PassPool``) on its own: no GPU, no library."""
import gc

import pytest

from behavior_driven_video_synthesis_amd.seq_passes import PassLease, PassPool


def test_a_pass_takes_the_lowest_free_slot():
    pool = PassPool(4)
    key = (64, 50, 50, 50)
    assert [pool.acquire(key) for _ in range(3)] == [0, 1, 2]
    pool.release(key, 1)
    assert pool.alive(key) == 2
    assert pool.acquire(key) == 1          # the hole before the end
    assert pool.acquire(key) == 3
    pool.release(key, 0)
    pool.release(key, 3)
    assert pool.acquire(key) == 0
    for slot in (0, 1, 2):
        pool.release(key, slot)
    assert pool.alive(key) == 0 and not pool._live          # nothing is kept for a shape that has no pass alive
    pool.release(key, 2)                                    # releasing twice is harmless
    assert pool.acquire(key) == 0


def test_one_pass_at_a_time_never_leaves_slot_zero():
    pool = PassPool(4)
    for _ in range(10):
        lease = pool.lease("k")
        assert lease.slot == 0
        del lease
    assert pool.alive("k") == 0


def test_the_slot_is_released_when_its_owner_dies():
    pool = PassPool(2)
    a, b = pool.lease("k"), pool.lease("k")
    assert isinstance(a, PassLease) and (a.slot, b.slot, a.key) == (0, 1, "k") and pool.alive("k") == 2
    del a
    gc.collect()
    assert pool.alive("k") == 1
    c = pool.lease("k")
    assert c.slot == 0

    class Node:            # what an autograd node is to the lease: an object that holds it, in a cycle the collector has to find
        pass
    n = Node()
    n.self, n.token = n, ("plan", b)
    del b
    assert pool.alive("k") == 2            # the holder is alive: so is the pass, whether or not its backward has run
    del n
    gc.collect()
    assert pool.alive("k") == 1
    c.release()
    c.release()                            # by hand, and twice: the finalizer runs once
    assert pool.alive("k") == 0
    del c
    gc.collect()
    assert pool.alive("k") == 0 and pool.lease("k").slot == 0


def test_the_cap_raises_and_says_what_to_do():
    pool = PassPool(4, "the behaviour net")
    pool.max_passes = 2
    key = (5, 6, 6, 6)
    held = [pool.lease(key), pool.lease(key)]
    with pytest.raises(RuntimeError) as err:
        pool.lease(key)
    msg = str(err.value)
    assert "max_passes = 2" in msg and "2 passes" in msg and "alive" in msg and "the behaviour net" in msg and str(key) in msg
    assert pool.alive(key) == 2            # the refused pass took nothing, evicted nothing
    assert [h.slot for h in held] == [0, 1]
    pool.max_passes = 3                    # the cap is read at every acquire
    assert pool.lease(key).slot == 2
    with pytest.raises(RuntimeError):
        PassPool(0).acquire("k")


def test_every_shape_key_has_its_own_slot_range():
    pool = PassPool(2)
    a0, a1 = pool.lease((64, 50)), pool.lease((64, 50))
    b0 = pool.lease((64, 49))              # a shape not seen before starts at 0 whatever the others hold
    assert (a0.slot, a1.slot, b0.slot) == (0, 1, 0)
    with pytest.raises(RuntimeError):
        pool.lease((64, 50))
    b1 = pool.lease((64, 49))              # ... and a full shape does not take room from another one
    assert b1.slot == 1
    del a0
    gc.collect()
    assert pool.alive((64, 50)) == 1 and pool.alive((64, 49)) == 2 and pool.alive("never seen") == 0
