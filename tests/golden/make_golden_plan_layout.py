"""Writes tests/golden/plan_layout.json: what the host-only plans of superdsm_amd.testing.PLAN_LAYOUT_CASES hand their kernels in each of
their scheduling modes (sdsm_plan_image: the kernel arguments over a null workspace, so every workspace offset and every scalar the layout
decides; the candidate descriptors, one hash per field), the size queries and sdsm_plan_layout, as the library built them when the file was
written.  The file pins the workspace: it is written once and regenerated only by a change that means to alter the layout.  The process-wide
inputs of the kernel arguments (group timeout, solver diagnostics, debug buffer, light limit) are at their defaults in a fresh process.  Needs
the built library, no GPU.  Run from the repository root: ``python tests/golden/make_golden_plan_layout.py``."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def layouts():
    from superdsm_amd import _capi, testing
    out = {}
    for name, (sides, modes, kw) in testing.PLAN_LAYOUT_CASES.items():
        plan = testing.plan_of_squares(sides, **kw)
        for mode in modes:
            _capi.check(_capi.lib().sdsm_plan_set_latency_mode(plan, mode), 'sdsm_plan_set_latency_mode')
            out[f'{name}/mode{mode}'] = testing.plan_layout_of(plan, len(sides))[0]
        _capi.lib().sdsm_plan_destroy(plan)
    return out


if __name__ == '__main__':
    with open(os.path.join(HERE, 'plan_layout.json'), 'w') as f:
        json.dump(layouts(), f, separators=(',', ':'))
        f.write('\n')
