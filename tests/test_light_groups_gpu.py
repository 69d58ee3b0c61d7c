"""Light workgroup groups (sdsm_solve_class: SDSM_CLS_WIDE_LIGHT, members that share their compute units with class 1): the class a group
runs in changes nothing in its candidate's bytes.  Needs an MI355X.

Shapes: testing.make_scene('synthetic256') -- 42 candidates, regions up to ~8000 pixels.  Latency mode forms groups of 2 to 4 members from
3072 pixels on, all of them light by size (a few dozen unknowns, envelopes of some hundred doubles); throughput mode and mode 2 solve the
same regions by single workgroups.  A plan this small has light groups only on request (the library grants them to plans of more than 1024
candidates): the module asks for them through sdsm_set_light_envelope_limit.  The second test moves the light class's envelope limit (sdsm_set_light_envelope_limit, the diagnostic
entry point: no region this small reaches 12 400 doubles) between the envelopes of two grouped regions of that scene."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLS_WIDE, CLS_WIDE2B, CLS_WIDE_LIGHT = 5, 6, 7


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    from superdsm_amd import _capi
    _capi.lib()
    return torch


@pytest.fixture(scope='module', autouse=True)
def light_groups_on_request(gpu):
    from superdsm_amd import _capi
    _capi.check(_capi.lib().sdsm_set_light_envelope_limit(12400), 'sdsm_set_light_envelope_limit')
    yield
    _capi.check(_capi.lib().sdsm_set_light_envelope_limit(-1), 'sdsm_set_light_envelope_limit')


def _members(batch):
    from superdsm_amd import _capi
    g = np.zeros(batch.n, np.int32)
    _capi.check(_capi.lib().sdsm_plan_schedule(batch.plan, g.ctypes.data_as(C.c_void_p), None), 'sdsm_plan_schedule')
    return g


def _classes(batch):
    """sdsm_plan_solve_classes on what the setup kernel of the batch's last launch left: the class every candidate ran in."""
    from superdsm_amd import _capi
    st = batch.inspect_states()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    status, M, env = (np.array([s[k] for s in st], np.int32) for k in ('status', 'M', 'env_size'))
    cls = np.full(batch.n, -9, np.int32)
    _capi.check(_capi.lib().sdsm_plan_solve_classes(batch.plan, p(status), p(M), p(env), p(cls)), 'sdsm_plan_solve_classes')
    return cls, env


def _solve(gpu, scene, fps, mode):
    from superdsm_amd import engine
    img = engine.DeviceImage(scene['y'], None, scene['atoms'], scene['dsm_cfg']['background_margin'])
    batch = engine.Batch(img, fps, scene['dsm_cfg'], want_xi=True, mode=mode)
    batch.masks_dev.zero_()                                  # (words of candidates without a solve are not written)
    batch.launch()
    gpu.cuda.synchronize()
    recs = batch.records()
    cls, env = _classes(batch)
    return dict(batch=batch, records=recs, masks=batch.masks_dev.cpu().numpy().copy(), xi=batch.xi_dev.cpu().numpy().copy(), members=_members(batch), cls=cls, env=env,
                fragments=batch.fragments(recs))


@pytest.fixture(scope='module')
def solved(gpu):
    """synthetic256, every candidate, in throughput (0), latency (1) and group-free (2) mode; the oracle's records.  Shared, read only."""
    from oracle import oracle
    from superdsm_amd import testing
    scene = testing.make_scene('synthetic256')
    out = {mode: _solve(gpu, scene, scene['footprints'], mode) for mode in (0, 1, 2)}
    orecs, _, _ = oracle.compute_objects(scene['y'], None, scene['atoms'], scene['footprints'], scene['dsm_cfg'], nthreads=0)
    return scene, out, orecs


def test_three_modes_same_bytes_and_the_oracles_energies(solved):
    scene, out, orecs = solved
    ref = out[2]
    assert len(ref['records']) == 42 and (ref['members'] == 0).all()
    lat = out[1]
    grouped = lat['members'] > 0
    N = ref['records']['n_pixels']
    print('synthetic256 latency mode: members', lat['members'][grouped].tolist(), 'envelopes', lat['env'][grouped].tolist(), 'classes', lat['cls'][grouped].tolist())
    assert grouped.sum() >= 10 and ((lat['members'] >= 2) & (lat['members'] <= 4))[grouped].all() and (grouped == (N > 3072)).all()
    assert (lat['cls'][grouped] == CLS_WIDE_LIGHT).all()                    # light by size: every group of this scene
    assert not np.isin(out[2]['cls'], (CLS_WIDE, CLS_WIDE2B, CLS_WIDE_LIGHT)).any()
    for mode in (0, 1):
        assert out[mode]['records'].tobytes() == ref['records'].tobytes(), f'mode {mode}: other record bytes than without groups'
        assert out[mode]['masks'].tobytes() == ref['masks'].tobytes(), f'mode {mode}: other mask bytes than without groups'
        assert out[mode]['xi'].tobytes() == ref['xi'].tobytes(), f'mode {mode}: other xi than without groups'
    recs = ref['records']
    np.testing.assert_array_equal(recs['n_pixels'], orecs['N'])
    for k in range(len(recs)):
        assert recs['status'][k] == orecs['status'][k]
        tol = 1e-6 * orecs['N'][k] / 1000 + 1e-5 * abs(orecs['energy'][k])      # the tolerance of test_gpu_parity.py for this workload
        assert abs(recs['energy'][k] - orecs['energy'][k]) <= tol, (k, recs['energy'][k], orecs['energy'][k])


def test_two_groups_on_either_side_of_the_light_limit(gpu, solved):
    """The limit is SHRUNK through sdsm_set_light_envelope_limit to the envelope of the smaller of two grouped regions (equal to the limit: light; the other one above:
    the layout of class 2b).  Both give the bytes of the group-free solve."""
    from superdsm_amd import _capi
    scene, out, _ = solved
    lat, ref = out[1], out[2]
    idx = np.flatnonzero(lat['members'] > 0)
    a, b = idx[np.argmin(lat['env'][idx])], idx[np.argmax(lat['env'][idx])]
    limit = int(lat['env'][a])
    assert 21 < limit < lat['env'][b] <= 11000
    L = _capi.lib()
    assert L.sdsm_set_light_envelope_limit(12401) != _capi.SDSM_OK          # more than the layout holds
    _capi.check(L.sdsm_set_light_envelope_limit(limit), 'sdsm_set_light_envelope_limit')
    try:
        two = _solve(gpu, scene, [scene['footprints'][a], scene['footprints'][b]], 1)
        _capi.check(L.sdsm_set_light_envelope_limit(-1), 'sdsm_set_light_envelope_limit')
        default, _ = _classes(out[1]['batch'])                                  # the default: no light groups in a plan of 42 candidates
    finally:
        _capi.check(L.sdsm_set_light_envelope_limit(12400), 'sdsm_set_light_envelope_limit')
    assert (default[idx] == CLS_WIDE).all()
    print('limit', limit, 'envelopes', two['env'].tolist(), 'members', two['members'].tolist(), 'classes', two['cls'].tolist())
    assert (two['members'] >= 2).all() and two['env'].tolist() == [limit, int(lat['env'][b])]
    assert two['cls'].tolist() == [CLS_WIDE_LIGHT, CLS_WIDE2B]
    assert two['records'].tobytes() == ref['records'][[a, b]].tobytes()
    for k, i in enumerate((a, b)):
        assert tuple(two['fragments'][k][0]) == tuple(ref['fragments'][i][0]) and np.array_equal(two['fragments'][k][1], ref['fragments'][i][1])
    xo, xr = two['batch'].xi_offsets(), ref['batch'].xi_offsets()
    for k, i in enumerate((a, b)):
        m = int(ref['records']['n_deform'][i])
        assert two['xi'][xo[k]:xo[k] + m].tobytes() == ref['xi'][xr[i]:xr[i] + m].tobytes()
    after, _ = _classes(out[1]['batch'])                                        # the module's request is back
    assert (after[idx] == CLS_WIDE_LIGHT).all()


def test_light_group_of_more_than_256_unknowns(gpu):
    """6 + M between 257 and 288 is the one size range of the light layout that no 256-thread class has: the factorisation's back substitution there must be
    the one every other class uses for that many unknowns (the blocked one rounds differently).  Candidate 1 of the `group_regime` fixture: 67 167 pixels,
    M = 263, envelope below 11 000; its group in throughput mode is light, and gives the bytes of the single workgroup of mode 2."""
    import json
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'optimum_group_regime.npz'))
    cfg = dict(json.loads(str(d['cfg'])), init='elliptical')
    scene = dict(y=d['y'], atoms=d['atoms'], dsm_cfg=cfg)
    fps = [d['c1_fp'].tolist()]
    grp, one = _solve(gpu, scene, fps, 0), _solve(gpu, scene, fps, 2)
    M = int(grp['records']['n_deform'][0])
    print('group_regime candidate 1: M', M, 'envelope', grp['env'].tolist(), 'members', grp['members'].tolist(), 'class', grp['cls'].tolist())
    assert 256 < 6 + M <= 288 and grp['members'][0] >= 2 and grp['cls'].tolist() == [CLS_WIDE_LIGHT] and one['members'][0] == 0
    assert grp['records'].tobytes() == one['records'].tobytes() and grp['xi'].tobytes() == one['xi'].tobytes() and grp['masks'].tobytes() == one['masks'].tobytes()
