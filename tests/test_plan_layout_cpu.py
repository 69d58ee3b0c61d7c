"""The workspace of a plan -- every block's offset, the workspace size, the scalars the layout decides and the per-candidate descriptors -- is
host logic: pinned by tests/golden/plan_layout.json through sdsm_plan_image (the kernel arguments over a null workspace, the descriptors
field by field), the size queries and sdsm_plan_layout, for the plans of testing.PLAN_LAYOUT_CASES in each of their modes.  No GPU."""
import json
import os

import numpy as np
import pytest

from superdsm_amd import _capi, testing

KEYS = [f'{name}/mode{mode}' for name, (_, modes, _) in testing.PLAN_LAYOUT_CASES.items() for mode in modes]


@pytest.fixture(scope='module')
def built():
    """key -> (record, kernel arguments by name, descriptors) of every case and mode, each plan built once."""
    lib = _capi.lib()
    # the process-wide inputs of the kernel arguments at their defaults, as they were when the fixture was written
    assert (lib.sdsm_set_light_envelope_limit(-1), lib.sdsm_set_group_timeout_us(0.0), lib.sdsm_set_solver_diagnostics(0), lib.sdsm_set_debug_buffer(None)) == (0, 0, 0, 0)
    out = {}
    for name, (sides, modes, kw) in testing.PLAN_LAYOUT_CASES.items():
        plan = testing.plan_of_squares(sides, **kw)
        for mode in modes:
            _capi.check(lib.sdsm_plan_set_latency_mode(plan, mode), 'sdsm_plan_set_latency_mode')
            rec, params, cand = testing.plan_layout_of(plan, len(sides))
            out[f'{name}/mode{mode}'] = (rec, params.view(_capi.PLAN_PARAMS_DTYPE)[0], cand)
        lib.sdsm_plan_destroy(plan)
    return out


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, 'plan_layout.json')) as f:
        return json.load(f)


def test_the_formats_are_those_of_the_library(built):
    lay = built['clusters/mode0'][0]['layout']
    names = _capi.PLAN_LAYOUT_NAMES
    assert len(names) == 16 and lay[names.index('cand_size')] == _capi.CAND_DESC_DTYPE.itemsize and lay[names.index('state_size')] == _capi.CAND_STATE_DTYPE.itemsize


def test_the_cases_show_what_they_are_there_for(built, golden):
    assert sorted(golden) == sorted(KEYS)
    # the list cases in each of their modes
    assert {f'{name}/mode{mode}' for name, (_, modes) in testing.PLAN_LIST_CASES.items() for mode in modes} <= set(KEYS)
    _, P, cand = built['two_images/mode0']
    assert P['n_images'] == 2 and sorted(set(cand['image'].tolist())) == [0, 1] and P['img']['H'][0] != P['img']['H'][1] and P['img']['W'][0] != P['img']['W'][1]
    rec, P, _ = built['no_deform/mode0']
    assert P['no_deform'] == 1 and P['k'] == 1 and P['zcap_run'] == 1
    rec, P, _ = built['dense_grid/mode0']
    assert P['zshift'] == 2 and P['zcap_run'] % 4 == 0 and rec['layout'][_capi.PLAN_LAYOUT_NAMES.index('zcap_run')] == P['zcap_run']
    assert (built['setup_split/mode0'][2]['hglob_off'] >= 0).any()
    cand = built['clusters/mode0'][2]
    pooled = cand['wide_off'] >= 0
    assert (pooled & (cand['wide_g'] > 0)).any() and (pooled & (cand['wide_g'] == 0) & (cand['rows_g'] > 0)).any()
    sides = testing.PLAN_LAYOUT_CASES['stray_labels'][0]
    cand = built['stray_labels/mode0'][2]
    assert cand['N'].tolist() == [s * s for s in sides] and (cand['fp_len'] == 4).all()       # label 0, a label beyond the atoms and an empty atom add nothing
    rec, P, cand = built['empty/mode0']
    assert P['n'] == 0 and len(cand) == 0 and rec['workspace_bytes'] > 0


@pytest.mark.parametrize('key', KEYS)
def test_layout_equals_the_recorded_one(built, golden, key):
    rec, P, _ = built[key]
    want = golden[key]
    for field in rec['cand']:
        assert rec['cand'][field] == want['cand'][field], f'CandDesc.{field}'
    for name in ('workspace_bytes', 'mask_bytes', 'total_pixels', 'xi_count'):
        assert rec[name] == want[name], name
    assert dict(zip(_capi.PLAN_LAYOUT_NAMES, rec['layout'])) == dict(zip(_capi.PLAN_LAYOUT_NAMES, want['layout']))
    assert rec['params'] == want['params'], {f: P[f].tolist() for f in P.dtype.names if f != 'img'}


@pytest.mark.parametrize('key', KEYS)
def test_blocks_lie_inside_the_workspace_in_256_byte_steps(built, key):
    rec, P, _ = built[key]
    blocks = ('cand', 'state', 'fp_labels', 'order', 'psf', 'crop_y', 'crop_rc', 'run_meta', 'run_q0', 'run_aux', 'crop_cc', 'dist', 'tmp_y', 'tmp_rc', 'inv',
              'grid_rc', 'ell_im', 'ell_w', 'env_fst', 'env_rb', 'hglob', 'wide_pool', 'wide_ticket')
    off = [int(P[b]) for b in blocks]
    assert off[0] == 0 and off == sorted(off) and len(set(off)) == len(off) and all(o % 256 == 0 for o in off)
    assert off[-1] + 256 == rec['workspace_bytes'] and int(P['cls_count']) == off[-1] + 64        # the launch words end the workspace
    assert [int(v) for v in (P['prof'], P['prof2'], P['x0'], P['solver_diag'])] == [0, 0, 0, 0] and int(P['wide_timeout']) == 5000000


def test_plan_image_checks_its_sizes():
    import ctypes as C
    lib = _capi.lib()
    plan = testing.plan_of_squares([30, 40])
    params, cand = np.zeros(_capi.PLAN_PARAMS_BYTES + 8, np.uint8), np.zeros(3, _capi.CAND_DESC_DTYPE)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.sdsm_plan_image(plan, ptr(params), _capi.PLAN_PARAMS_BYTES, ptr(cand), 2 * 112) == 0
    for pb, cb in ((_capi.PLAN_PARAMS_BYTES + 8, 2 * 112), (_capi.PLAN_PARAMS_BYTES - 8, 2 * 112), (_capi.PLAN_PARAMS_BYTES, 3 * 112), (_capi.PLAN_PARAMS_BYTES, 112)):
        assert lib.sdsm_plan_image(plan, ptr(params), pb, ptr(cand), cb) == -1 and b'sdsm_plan_image' in lib.sdsm_last_error()
    assert lib.sdsm_plan_image(None, ptr(params), _capi.PLAN_PARAMS_BYTES, ptr(cand), 2 * 112) == -1
    assert lib.sdsm_plan_image(plan, None, _capi.PLAN_PARAMS_BYTES, ptr(cand), 2 * 112) == -1
    lib.sdsm_plan_destroy(plan)
