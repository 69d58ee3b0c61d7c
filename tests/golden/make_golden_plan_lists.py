"""Writes tests/golden/plan_lists.json: the launch lists (sdsm_plan_lists: seven spans and the `order` array) of the host-only plans of
superdsm_amd.testing.PLAN_LIST_CASES in each of their scheduling modes, as the library built them when the file was written.  The file
pins the lists: it is written once and regenerated only by a change that means to alter what a plan schedules.  Needs the built library,
no GPU.  Run from the repository root: ``python tests/golden/make_golden_plan_lists.py``."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def lists():
    from superdsm_amd import _capi, testing
    out = {}
    for name, (sides, modes) in testing.PLAN_LIST_CASES.items():
        plan = testing.plan_of_squares(sides)
        for mode in modes:
            spans, order = testing.plan_lists(plan, mode)
            out[f'{name}/mode{mode}'] = dict(spans=spans.tolist(), order=order.tolist())
        _capi.lib().sdsm_plan_destroy(plan)
    return out


if __name__ == '__main__':
    with open(os.path.join(HERE, 'plan_lists.json'), 'w') as f:
        json.dump(lists(), f, separators=(',', ':'))
        f.write('\n')
