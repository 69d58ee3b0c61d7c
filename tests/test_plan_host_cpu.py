"""The plan unit (superdsm_amd/csrc/sdsm_plan.hip) links alone and makes no device call: tests/host/plan_check.cpp builds the plans of
testing.PLAN_LAYOUT_CASES with it under AddressSanitizer and UndefinedBehaviorSanitizer (the runtime is linked into the executable), walks
every mode and query, makes the rejected calls, and writes what each recorded mode hands out.  The run must end clean, and its files must
equal tests/golden/plan_layout.json and tests/golden/plan_lists.json.  No GPU; a failing compile fails the test."""
import json
import os
import subprocess

import numpy as np
import pytest

from superdsm_amd import _capi, testing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [f'{name}/mode{mode}' for name, (_, modes, _) in testing.PLAN_LAYOUT_CASES.items() for mode in modes]


@pytest.fixture(scope='module')
def outdir(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('plan_check')
    cases, prog = tmp / 'cases.txt', tmp / 'plan_check'
    cases.write_text(testing.plan_cases_text())
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    build = subprocess.run([hipcc, '-x', 'hip', '--offload-host-only', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                            '-o', str(prog), os.path.join(ROOT, 'tests', 'host', 'plan_check.cpp'), os.path.join(ROOT, 'superdsm_amd', 'csrc', 'sdsm_plan.hip')],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(prog), str(cases), str(tmp)], capture_output=True, text=True, timeout=120)
    assert (run.returncode, run.stderr) == (0, ''), run.stderr
    return tmp


def test_the_cases_are_those_of_both_fixtures(golden_dir):
    with open(os.path.join(golden_dir, 'plan_layout.json')) as f:
        assert sorted(json.load(f)) == sorted(KEYS)
    with open(os.path.join(golden_dir, 'plan_lists.json')) as f:
        assert set(json.load(f)) <= set(KEYS)


@pytest.mark.parametrize('key', KEYS)
def test_the_stand_alone_plan_equals_the_recorded_one(outdir, golden_dir, key):
    base = os.path.join(str(outdir), key.replace('/', '.'))
    sizes = np.fromfile(base + '.sizes', np.int64)
    rec = testing.plan_layout_record(np.fromfile(base + '.params', np.uint8), np.fromfile(base + '.cand', _capi.CAND_DESC_DTYPE), sizes[:4], sizes[4:])
    with open(os.path.join(golden_dir, 'plan_layout.json')) as f:
        assert rec == json.load(f)[key]
    with open(os.path.join(golden_dir, 'plan_lists.json')) as f:
        lists = json.load(f)
    if key in lists:
        words = np.fromfile(base + '.lists', np.int32)
        assert words[:14].reshape(7, 2).tolist() == lists[key]['spans'] and words[14:].tolist() == lists[key]['order']
