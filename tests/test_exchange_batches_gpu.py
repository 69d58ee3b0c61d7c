"""The exchange of a workgroup group in batches (wide_finish): a thread requests the 16-byte pairs of all other
members for a batch of entries before it uses the first, its own partials come from LDS, the psi-type sums are fetched by the lanes of a
wavefront and added in member and position order.  The sums of the long vectors are integers and the psi-type sums keep their order: a
group gives the bytes of a single workgroup, whatever its size, its layout and the lengths it exchanges.

Scenes.  (i) testing.make_scene('synthetic256'), latency mode against mode 2, as tests/test_group_exchange_gpu.py -- here in the 512-thread
group layouts AND in the light layout (sdsm_set_light_envelope_limit).  (ii) The 80 x 96 blob of tests/test_loss_arithmetic_gpu.py (one
atom, one candidate of 2266 or 3043 pixels) under the settings of tests/test_newton_step_gpu.py, which give it 47 to 342 unknowns and
envelopes of 1055 to 11 051 doubles, and under smooth_subsample = 16 (a dozen unknowns).  A plan of one such region forms no group by
itself: the diagnostic knobs of the layout (SDSM_WIDE_TP_MIN_PIXELS, SDSM_WIDE_SLICE; INTEGRATION.md -- results do not depend on them) deal
it to 2, 3 and 4 members in throughput mode, and to one more where the plan grants its bonus member (regions whose bound on the unknowns
exceeds the light class: 3, 4 and 5).  A member's slice is a whole number of super-chunks (512 runs) and the regions have 607 and 805
runs, so from three members on some members have NO run at all (they publish no psi-type sum) -- asserted from sdsm_plan_schedule and
the states.

What a thread moves per batch: the direct path (at most 3 members, or fewer than WIDE_RS_MIN = 512 words) 4 pairs = 8 words, a batch of
4096 words per 512-thread workgroup; the reduce-scatter (4 members and 512 words or more) 2 pairs = 4 words of the member's share, a
batch of 2048 words.  The exchanged lengths env + M + 42 are asserted to lie on both sides of one batch, in both layouts and on both
paths, and to include one below WIDE_RS_MIN."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDE_DIRECT_MAX_G, WIDE_RS_MIN, MOMENT_WORDS = 3, 512, 42
THREADS = 512                                   # of every group layout
DIRECT_BATCH, RS_BATCH = 2 * 4 * THREADS, 2 * 2 * THREADS      # words per batch and workgroup (WIDE_XB = 4, WIDE_RB = 2 pairs per thread)
SUPER_RUNS = 64 * 8                             # runs of a super-chunk (SDSM_SUPER chunks of 64)
CLS_WIDE, CLS_WIDE2B, CLS_WIDE_LIGHT = 5, 6, 7
LIGHT_NMAX, LIGHT_EMAX = 288, 12400

BLOBS = {                                       # dsm/* settings of the blob scenes (tests/test_newton_step_gpu.py: STEP_SCENES) and one with a dozen unknowns
    'm12': dict(margin=8, kw=dict(smooth_subsample=16)),
    'm47': dict(margin=8, kw=dict(smooth_subsample=8)),
    'm123': dict(margin=8, kw=dict(smooth_subsample=5)),
    'm252': dict(margin=4, kw=dict(smooth_subsample=3, smooth_amount=2)),
    'm342': dict(margin=8, kw=dict(smooth_subsample=3, smooth_amount=1)),
}
GROUP_SIZES = (2, 3, 4)


def _members(batch):
    from superdsm_amd import _capi
    g = np.zeros(batch.n, np.int32)
    _capi.check(_capi.lib().sdsm_plan_schedule(batch.plan, g.ctypes.data_as(C.c_void_p), None), 'sdsm_plan_schedule')
    return g


def _classes(batch, st):
    from superdsm_amd import _capi
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    status, M, env = (np.array([s[k] for s in st], np.int32) for k in ('status', 'M', 'env_size'))
    cls = np.full(batch.n, -9, np.int32)
    _capi.check(_capi.lib().sdsm_plan_solve_classes(batch.plan, p(status), p(M), p(env), p(cls)), 'sdsm_plan_solve_classes')
    return cls


def _launch_twice(img, fps, cfg, mode):
    """Two launches in a row of one batch: their (records, xi, masks) bytes; members, classes and states of the plan."""
    import torch
    from superdsm_amd import engine
    batch = engine.Batch(img, fps, cfg, want_xi=True, mode=mode)
    batch.masks_dev.zero_()
    out = []
    for _ in range(2):
        batch.launch()
        torch.cuda.synchronize()
        out.append((batch.records().tobytes(), batch.xi_dev.cpu().numpy().tobytes(), batch.masks_dev.cpu().numpy().tobytes()))
    st = batch.inspect_states()
    return dict(out=out, members=_members(batch), cls=_classes(batch, st), states=st, status=batch.records()['status'].copy(), n_pixels=batch.records()['n_pixels'].copy())


def _words(s):
    return s['env_size'] + s['M'] + MOMENT_WORDS


def _empty_members(NR, g):
    """Members of a group of g whose slice holds no run (solve_candidate: slices of whole super-chunks)."""
    chunk = -(-(-(-NR // g)) // SUPER_RUNS) * SUPER_RUNS
    return sum(1 for w in range(g) if w * chunk >= NR)


class _Knobs:
    """The layout knobs of the plans created inside the block (read by the library at every layout of a plan)."""
    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope='module')
def lib():
    import torch
    from superdsm_amd import _capi
    assert torch.cuda.is_available(), 'these tests need a GPU'
    yield _capi.lib()
    _capi.check(_capi.lib().sdsm_set_light_envelope_limit(-1), 'sdsm_set_light_envelope_limit')


def _with_light(lib, light, fn):
    from superdsm_amd import _capi
    _capi.check(lib.sdsm_set_light_envelope_limit(LIGHT_EMAX if light else -1), 'sdsm_set_light_envelope_limit')
    try:
        return fn()
    finally:
        _capi.check(lib.sdsm_set_light_envelope_limit(-1), 'sdsm_set_light_envelope_limit')


@pytest.fixture(scope='module')
def synthetic(lib):
    """synthetic256: mode 2, and latency mode in the 512-thread group layouts (light False) and in the light layout (True)."""
    from superdsm_amd import engine, testing
    scene = testing.make_scene('synthetic256')
    img = engine.DeviceImage(scene['y'], None, scene['atoms'], scene['dsm_cfg']['background_margin'])
    run = lambda mode: _launch_twice(img, scene['footprints'], scene['dsm_cfg'], mode)
    return dict(ref=run(2), groups={light: _with_light(lib, light, lambda: run(1)) for light in (False, True)})


@pytest.fixture(scope='module')
def blobs(lib):
    """Per blob scene: the group-free launch and the launches as a group of 2, 3 and 4 members, in both kinds of layout."""
    from superdsm_amd import engine, testing as T
    from test_loss_arithmetic_gpu import _blob_scene
    y, atoms = _blob_scene()
    images, out = {}, {}
    for name, sc in BLOBS.items():
        if sc['margin'] not in images:
            images[sc['margin']] = engine.DeviceImage(y, None, atoms, sc['margin'])
        img, cfg = images[sc['margin']], T._toy_cfg(background_margin=sc['margin'], **sc['kw'])
        ref = _launch_twice(img, [[1]], cfg, 2)
        N = int(ref['n_pixels'][0])
        groups = {}
        for g in GROUP_SIZES:
            slice_pixels = -(-N // g)                        # one member per slice_pixels pixels: ceil(N / slice_pixels) = g (asserted from the plan below)
            with _Knobs(SDSM_WIDE_TP_MIN_PIXELS=N - 1, SDSM_WIDE_SLICE=slice_pixels):
                for light in (False, True):
                    groups[g, light] = _with_light(lib, light, lambda: _launch_twice(img, [[1]], cfg, 0))
        out[name] = dict(ref=ref, groups=groups, N=N)
    return out


def _same_bytes(a, b, label):
    for x, y, what in zip(a, b, ('records', 'xi', 'masks')):
        assert x == y, f'{label}: {what} differ'


def test_synthetic256_groups_in_both_layouts_give_the_bytes_of_single_workgroups(synthetic):
    ref = synthetic['ref']
    assert (ref['members'] == 0).all()
    for light, run in synthetic['groups'].items():
        grouped = run['members'] > 0
        words = np.array([_words(s) if s['M'] > 0 else 0 for s in run['states']])
        print(f'synthetic256, latency mode, light {light}: members', run['members'][grouped].tolist(), 'classes', run['cls'][grouped].tolist(), 'words', words[grouped].tolist())
        assert grouped.sum() >= 10 and ((run['members'][grouped] >= 2) & (run['members'][grouped] <= 4)).all()
        assert (run['cls'][grouped] == (CLS_WIDE_LIGHT if light else CLS_WIDE)).all()
        assert (grouped & (words >= WIDE_RS_MIN) & (run['members'] <= WIDE_DIRECT_MAX_G)).any() and (grouped & (words >= WIDE_RS_MIN) & (run['members'] > WIDE_DIRECT_MAX_G)).any()
        assert (run['status'] != 5).all() and (run['status'] == ref['status']).all()       # (SDSM_CAND_GIVEN_UP = 5)
        _same_bytes(run['out'][0], ref['out'][0], f'light {light}: grouped launch against the launch without groups')
        _same_bytes(run['out'][1], run['out'][0], f'light {light}: second launch against the first')
    _same_bytes(ref['out'][1], ref['out'][0], 'mode 2: second launch against the first')


def test_blob_plans_cover_the_lengths_and_the_empty_slices(blobs):
    """What the equality test below stands on, asserted from the plans and the states alone."""
    direct, scatter, empty, short = {False: [], True: []}, {False: [], True: []}, 0, 0
    for name, b in blobs.items():
        assert (b['ref']['members'] == 0).all() and b['ref']['status'][0] != 5
        for (asked, light), run in b['groups'].items():
            s, cls, g = run['states'][0], int(run['cls'][0]), int(run['members'][0])
            assert run['members'].shape == (1,) and asked <= g <= asked + 1, (name, asked, run['members'])   # (+ 1: the bonus member of a region that may not be light)
            fits_light = 6 + s['M'] <= LIGHT_NMAX and s['env_size'] <= LIGHT_EMAX
            assert cls in (CLS_WIDE, CLS_WIDE2B, CLS_WIDE_LIGHT) and (cls == CLS_WIDE_LIGHT) == (light and fits_light), (name, g, light, cls)
            assert s['M'] > 0 and s['status'] == 0
            nt = _words(s)
            empty += _empty_members(s['NR'], g) > 0
            short += nt < WIDE_RS_MIN
            if nt < WIDE_RS_MIN or g <= WIDE_DIRECT_MAX_G:
                direct[cls == CLS_WIDE_LIGHT].append(nt)
            else:
                share = ((-(-nt // g)) + 7) & ~7
                scatter[cls == CLS_WIDE_LIGHT].append(share)
        print(name, 'N', b['N'], 'NR', b['groups'][2, False]['states'][0]['NR'], 'words', _words(b['groups'][2, False]['states'][0]),
              'classes', {k: int(v['cls'][0]) for k, v in b['groups'].items()})
    print('direct path, words:', direct, ' reduce-scatter, words of a share:', scatter)
    assert empty >= 1 and short >= 1
    for light in (False, True):                              # both layouts: one batch is not enough for some, more than enough for others; odd and even lengths
        assert min(direct[light]) < DIRECT_BATCH < max(direct[light]), (light, direct[light])
        assert min(scatter[light]) < RS_BATCH < max(scatter[light]), (light, scatter[light])
        assert any(v % 2 for v in direct[light]) and any(v % 2 == 0 for v in direct[light])


def test_blob_groups_give_the_bytes_of_a_single_workgroup(blobs):
    for name, b in blobs.items():
        ref = b['ref']
        _same_bytes(ref['out'][1], ref['out'][0], f'{name}, no group: second launch against the first')
        for (g, light), run in b['groups'].items():
            label = f'{name}, {g} members, light {light}'
            assert run['status'].tolist() == ref['status'].tolist(), label
            _same_bytes(run['out'][0], ref['out'][0], label + ': against the launch without a group')
            _same_bytes(run['out'][1], run['out'][0], label + ': second launch against the first')
