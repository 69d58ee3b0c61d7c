"""``sdsm_choose_sides_host``: which streams of the side pool a launch uses, as a pure function of a given "shares a hardware queue"
relation (index 0 the caller's stream, 1 + i pool stream i).  The launch path applies the same function to what its probes find."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope='module')
def choose():
    from superdsm_amd import _capi
    L = _capi.lib()

    def run(n_pool, pairs, want, directed=False):
        n = n_pool + 1
        shares = np.zeros((n, n), np.uint8)
        for a, b in pairs:
            shares[a, b] = 1
            if not directed:
                shares[b, a] = 1
        out = np.full(max(want, 1) + 2, -7, np.int32)                  # two guard entries behind the `want` that are written
        clean = L.sdsm_choose_sides_host(n_pool, shares.ctypes.data_as(C.c_void_p), want, out.ctypes.data_as(C.c_void_p))
        assert (out[want:] == -7).all(), 'wrote beyond out[want]'
        return clean, out[:want].tolist()

    return run


CALLER = 0


def pool(i):
    return 1 + i


def test_nothing_shares(choose):
    assert choose(8, [], 3) == (3, [0, 1, 2])
    assert choose(8, [], 4) == (4, [0, 1, 2, 3])
    assert choose(3, [], 3) == (3, [0, 1, 2])


def test_the_caller_shares_with_a_pool_stream(choose):
    assert choose(8, [(CALLER, pool(2))], 3) == (3, [0, 1, 3])
    assert choose(8, [(CALLER, pool(2))], 4) == (4, [0, 1, 3, 4])
    assert choose(8, [(CALLER, pool(0))], 3) == (3, [1, 2, 3])


def test_two_pool_streams_share_with_each_other(choose):
    assert choose(8, [(pool(0), pool(1))], 3) == (3, [0, 2, 3])
    assert choose(8, [(pool(0), pool(1))], 4) == (4, [0, 2, 3, 4])
    # a stream that was passed over does not block a later one that shares with it only
    assert choose(8, [(pool(0), pool(1)), (pool(1), pool(2))], 3) == (3, [0, 2, 3])


def test_four_queues_dealt_round_robin(choose):
    """Four hardware queues, streams dealt in turn, the caller's stream on the queue of pool streams 1 and 5."""
    queue = {CALLER: 1, **{pool(i): i % 4 for i in range(8)}}
    pairs = [(a, b) for a in queue for b in queue if a < b and queue[a] == queue[b]]
    assert choose(8, pairs, 3) == (3, [0, 2, 3])
    assert choose(8, pairs, 4) == (3, [0, 2, 3, -1])                  # there is no fifth queue: class 2b stays behind the global-memory class


def test_fewer_than_three_clean_sides_are_replaced_in_order(choose):
    """Class 1b (side 3) goes behind the groups / class 2 (side 2) first, then side 2 behind side 1."""
    two = [(CALLER, pool(i)) for i in range(2, 8)]
    assert choose(8, two, 3) == (2, [0, 1, 1])
    assert choose(8, two, 4) == (2, [0, 1, 1, -1])
    one = [(CALLER, pool(i)) for i in range(8) if i != 4]
    assert choose(8, one, 3) == (1, [4, 4, 4])
    assert choose(8, one, 4) == (1, [4, 4, 4, -1])
    # two queues in all: the caller's and one more
    queue = {CALLER: 0, **{pool(i): i % 2 for i in range(8)}}
    pairs = [(a, b) for a in queue for b in queue if a < b and queue[a] == queue[b]]
    assert choose(8, pairs, 3) == (1, [1, 1, 1])


def test_everything_on_one_queue(choose):
    everything = [(a, b) for a in range(9) for b in range(a + 1, 9)]
    assert choose(8, everything, 3) == (0, [0, 0, 0])
    assert choose(8, everything, 4) == (0, [0, 0, 0, -1])
    assert choose(1, [(CALLER, pool(0))], 3) == (0, [0, 0, 0])


def test_empty_pool(choose):
    from superdsm_amd import _capi
    assert choose(0, [], 3) == (0, [-1, -1, -1])
    assert choose(0, [], 4) == (0, [-1, -1, -1, -1])
    out = np.full(3, -7, np.int32)
    assert _capi.lib().sdsm_choose_sides_host(0, None, 3, out.ctypes.data_as(C.c_void_p)) == 0 and out.tolist() == [-1, -1, -1]


def test_want_larger_than_the_pool(choose):
    assert choose(2, [], 3) == (2, [0, 1, 1])
    assert choose(2, [], 4) == (2, [0, 1, 1, -1])
    assert choose(3, [], 4) == (3, [0, 1, 2, -1])
    assert choose(1, [], 3) == (1, [0, 0, 0])
    assert choose(8, [], 0) == (0, [])


def test_bad_arguments(choose):
    from superdsm_amd import _capi
    L = _capi.lib()
    out = np.zeros(4, np.int32)
    shares = np.zeros((3, 3), np.uint8)
    assert L.sdsm_choose_sides_host(-1, shares.ctypes.data_as(C.c_void_p), 3, out.ctypes.data_as(C.c_void_p)) == -1
    assert L.sdsm_choose_sides_host(2, shares.ctypes.data_as(C.c_void_p), -1, out.ctypes.data_as(C.c_void_p)) == -1
    assert L.sdsm_choose_sides_host(2, shares.ctypes.data_as(C.c_void_p), 3, None) == -1
    assert L.sdsm_choose_sides_host(2, None, 3, out.ctypes.data_as(C.c_void_p)) == -1


@pytest.mark.parametrize('seed', range(4))
def test_the_relation_is_read_symmetrically(choose, seed):
    """An entry set in one direction only counts as much as one set in both, whichever direction it is."""
    rng = np.random.default_rng(seed)
    pairs = [(a, b) for a in range(9) for b in range(a + 1, 9) if rng.random() < 0.25]
    want = choose(8, pairs, 4)
    assert choose(8, pairs, 4, directed=True) == want
    assert choose(8, [(b, a) for a, b in pairs], 4, directed=True) == want
    flipped = [(b, a) if rng.random() < 0.5 else (a, b) for a, b in pairs]
    assert choose(8, flipped, 4, directed=True) == want
    # and the answer is what the rule says: no chosen stream shares with the caller's or with another chosen one
    clean, out = want
    rel = {frozenset(p) for p in pairs}
    members = [CALLER] + [pool(i) for i in out[:clean]]
    assert all(frozenset((a, b)) not in rel for a in members for b in members if a != b)
    assert len(set(out[:clean])) == clean and out[:clean] == sorted(out[:clean])


def test_the_report_before_any_launch_is_readable(choose):
    from superdsm_amd import _capi
    out = np.full(8, -7, np.int32)
    assert _capi.lib().sdsm_side_queue_report(out.ctypes.data_as(C.c_void_p)) == 0
    assert (out != -7).all()
