"""The launch lists of a plan (sdsm_plan.hip, layout_plan; read through sdsm_plan_lists) are host logic: pinned entry by entry by
tests/golden/plan_lists.json for three plans, and checked for the structure every launch relies on.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from superdsm_amd import _capi, testing

NAMES = testing.PLAN_LIST_NAMES
KEYS = [f'{name}/mode{mode}' for name, (_, modes) in testing.PLAN_LIST_CASES.items() for mode in modes]


@pytest.fixture(scope='module')
def built():
    """key -> (pixels per candidate, spans, order, group members, row workgroups) of every case and mode, each plan built once."""
    lib = _capi.lib()
    out = {}
    for name, (sides, modes) in testing.PLAN_LIST_CASES.items():
        plan = testing.plan_of_squares(sides)
        n = len(sides)
        for mode in modes:
            spans, order = testing.plan_lists(plan, mode)
            g, r = np.zeros(n, np.int32), np.zeros(n, np.int32)
            assert lib.sdsm_plan_schedule(plan, g.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p)) == 0
            out[f'{name}/mode{mode}'] = (np.array(sides) ** 2, spans, order, g, r)
        lib.sdsm_plan_destroy(plan)
    return out


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, 'plan_lists.json')) as f:
        return json.load(f)


def _lists(spans, order):
    return {name: order[first:first + count] for name, (first, count) in zip(NAMES, spans.tolist())}


def test_the_cases_cover_every_list(built, golden):
    assert sorted(golden) == sorted(KEYS)
    count = {key: dict(zip(NAMES, built[key][1][:, 1].tolist())) for key in KEYS}
    assert count['setup_split/mode0']['setup_small'] == 300 and count['setup_split/mode0']['setup_big'] == 2     # Mcap = 24 * 24 = 576 > 512: the middle setup class; 300 >= 256 small regions
    assert count['clusters/mode0']['group_members'] > 0 and count['clusters/mode0']['row_members'] > 0
    assert count['clusters/mode0']['setup_small'] == 0 and count['clusters/mode0']['setup_big'] == 0
    assert count['clusters/mode1']['group_members'] > count['clusters/mode0']['group_members'] and count['clusters/mode2']['group_members'] == 0
    assert count['no_groups/mode0']['group_members'] == 0 and count['no_groups/mode0']['row_members'] == 0


@pytest.mark.parametrize('key', KEYS)
def test_launch_lists_equal_the_recorded_ones(built, golden, key):
    _, spans, order, _, _ = built[key]
    assert spans.tolist() == golden[key]['spans']
    assert order.tolist() == golden[key]['order']


def _is_subsequence(sub, seq):
    it = iter(seq)
    return all(any(v == w for w in it) for v in sub)


@pytest.mark.parametrize('key', KEYS)
def test_launch_lists_have_the_structure_a_launch_relies_on(built, key):
    N, spans, order, g, r = built[key]
    n = len(N)
    # the spans are contiguous and cover `order` exactly
    assert spans[0, 0] == 0 and (spans[1:, 0] == spans[:-1, 0] + spans[:-1, 1]).all() and spans[-1, 0] + spans[-1, 1] == len(order)
    L = _lists(spans, order)
    # all candidates, largest first, equal ones in the order of the plan
    assert L['all'].tolist() == np.argsort(-N, kind='stable').tolist() and len(L['all']) == n
    every = L['all'].tolist()
    for name in ('beyond_1', 'beyond_2', 'setup_small', 'setup_big'):
        assert _is_subsequence(L[name].tolist(), every), name
    assert len(L['setup_small']) + len(L['setup_big']) in (0, n) and not set(L['setup_small'].tolist()) & set(L['setup_big'].tolist())
    # member lists: (candidate | member << 24), the candidates in the order of `all`, each with the members sdsm_plan_schedule gives it
    assert L['group_members'].tolist() == [c | (m << 24) for c in every for m in range(g[c])]
    assert L['row_members'].tolist() == [c | (m << 24) for c in every for m in range(r[c])]
