"""The exchange of a workgroup group (wide_finish, wide_barrier): groups of at most WIDE_DIRECT_MAX_G = 3 members add
the published blocks of a long vector (the Hessian envelope) directly after ONE rendezvous, larger groups reduce-scatter, meet again
and all-gather.  The sums are integers: either way a group gives the bytes of a single workgroup.

Scene: testing.make_scene('synthetic256') in latency mode -- 42 candidates, groups of 2 to 4 members from 3072 pixels on; a vector is
long from WIDE_RS_MIN = 512 words on (envelope + M + the 42 moment words).  The member counts are asserted below: at least one group
on either side of WIDE_DIRECT_MAX_G exchanges long vectors, so both branches run.  Reference: the same candidates without groups
(mode 2).  That a group still gives up after its time limit: tests/test_given_up_gpu.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDE_DIRECT_MAX_G, WIDE_RS_MIN, MOMENT_WORDS = 3, 512, 42


def _solve(mode):
    """One launch of the scene: records, xi and mask words as bytes, the members of every candidate, the words of its long exchange."""
    import torch
    from superdsm_amd import _capi, engine, testing
    scene = testing.make_scene('synthetic256')
    img = engine.DeviceImage(scene['y'], None, scene['atoms'], scene['dsm_cfg']['background_margin'])
    batch = engine.Batch(img, scene['footprints'], scene['dsm_cfg'], want_xi=True, mode=mode)
    batch.masks_dev.zero_()
    out = []
    for _ in range(2):                                       # the same launch twice in a row
        batch.launch()
        torch.cuda.synchronize()
        out.append((batch.records().tobytes(), batch.xi_dev.cpu().numpy().tobytes(), batch.masks_dev.cpu().numpy().tobytes()))
    members = np.zeros(batch.n, np.int32)
    _capi.check(_capi.lib().sdsm_plan_schedule(batch.plan, members.ctypes.data_as(C.c_void_p), None), 'sdsm_plan_schedule')
    st = batch.inspect_states()
    words = np.array([s['env_size'] + s['M'] + MOMENT_WORDS if s['M'] > 0 else 0 for s in st])
    status = batch.records()['status'].copy()
    return out, members, words, status


@pytest.fixture(scope='module')
def launches():
    import torch
    from superdsm_amd import _capi
    assert torch.cuda.is_available(), 'these tests need a GPU'
    _capi.lib()
    return {mode: _solve(mode) for mode in (1, 2)}


def test_both_branches_of_the_exchange_run(launches):
    _, members, words, status = launches[1]
    grouped = members > 0
    long_vec = words >= WIDE_RS_MIN
    print('synthetic256, latency mode: members', members[grouped].tolist(), 'words of the Hessian exchange', words[grouped].tolist())
    assert ((members[grouped] >= 2) & (members[grouped] <= 8)).all()
    assert (grouped & long_vec & (members <= WIDE_DIRECT_MAX_G)).sum() >= 1, 'no group of at most 3 members exchanges a long vector'
    assert (grouped & long_vec & (members > WIDE_DIRECT_MAX_G)).sum() >= 1, 'no group of at least 4 members exchanges a long vector'
    assert (launches[2][1] == 0).all()                       # mode 2: no groups
    assert (status != 5).all() and (status == launches[2][3]).all()   # (SDSM_CAND_GIVEN_UP = 5: nobody waited for a partner in vain)


def test_groups_give_the_bytes_of_single_workgroups(launches):
    for a, b, what in zip(launches[1][0][0], launches[2][0][0], ('records', 'xi', 'masks')):
        assert a == b, f'{what} of the grouped launch differ from the launch without groups'


def test_the_same_launch_twice(launches):
    for mode in (1, 2):
        first, second = launches[mode][0]
        for a, b, what in zip(first, second, ('records', 'xi', 'masks')):
            assert a == b, f'mode {mode}: {what} differ between two launches in a row'
