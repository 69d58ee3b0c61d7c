"""sdsm_k_post_set against the reference's full-image formulation (oracle/postprocess_oracle.py) at its edges: every record field
against the same sums in np.longdouble with bounds derived from the number of terms, refined masks bit for bit against
``process_mask``.  The cases (superdsm_amd/testing.py) and the conditions that make these demands fair are checked without a GPU in
tests/test_postprocess_cpu.py.

Bounds (eps = 2^-52; a float64 sum of n positive terms in any order is within n eps relative): a mean (n + 16) eps, ``fg_std`` the
bound of a two-pass evaluation 4 n eps, the contrast the sum of its two means' bounds; n = the pixels that enter the sum."""
import numpy as np
import pytest
import scipy.ndimage as ndi

from superdsm_amd import testing

pytestmark = pytest.mark.gpu

LAUNCHES = {L['name']: L for L in testing.post_launches()}          # built once, at collection: the tests show up under the names of the cases
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    from superdsm_amd import _capi
    _capi.lib()
    return torch


def _bg(im, exterior_offset):
    from oracle import postprocess_oracle as po
    if im['bg'] is not None:
        return im['bg']
    return po.background_mask(im['g'].shape, [(o.fg_offset, o.fg_fragment) for o in im['objects']], exterior_offset)


def _items(torch, images, exterior_offset):
    """What process_objects_gpu_multi takes: the generator's g and g_mask_processing uploaded as they are (the kernel and the oracle
    read the same bytes)."""
    return [(im['objects'], torch.as_tensor(np.ascontiguousarray(im['g'])).cuda(), torch.as_tensor(np.ascontiguousarray(im['gs'])).cuda(), _bg(im, exterior_offset))
            for im in images]


def _field(got, want, bound, what, worst, gs_abs=0.0):
    got, want = float(got), float(want)
    if not np.isfinite(want):
        assert (np.isnan(got) and np.isnan(want)) or got == want, (what, got, want)
        return
    err = abs(got - want)
    if want != 0 and bound > 0:
        worst[what[-1]] = max(worst.get(what[-1], 0.0), err / (bound * abs(want) + gs_abs))
    assert err <= bound * abs(want) + gs_abs, (what, got, want, err / abs(want) if want else err, bound)


def _check_image(label, im, bg, recs, refined, settings, worst, gs_ref=None, gs_abs=0.0):
    """Every object of one image against the oracle and extended precision: the record fields and, unless ``refined`` is None (the
    caller compares the masks itself), the refined masks; ``gs_ref``/``gs_abs``: the smoothed image the reference sums and the
    absolute allowance for the device's own filter (stage level only)."""
    from oracle import postprocess_oracle as po
    scale, offset, epsilon, m, stdamp = settings
    gs = im['gs'] if gs_ref is None else gs_ref
    assert len(recs) == len(im['objects']) and (refined is None or len(refined) == len(recs))
    for k, o in enumerate(im['objects']):
        what = (label, k, o.tag)
        ref = testing.post_reference(im['g'], gs, bg, o.fg_offset, o.fg_fragment, *settings)
        assert recs['area'][k] == ref['n_in'] == o.fg_fragment.sum(), what
        refines = m > 0 and stdamp > 0
        if ref['n_in'] == 0:
            assert recs['status'][k] == 2, what
            if refines and refined is not None:
                off, frag = po.extract_fragment(np.zeros(im['g'].shape, bool))
                assert np.array_equal(refined[k][0], off) and np.array_equal(refined[k][1], frag), what
            continue
        assert recs['status'][k] == (0 if refines else 3), what
        b_in, b_ext = (ref['n_in'] + 16) * EPS, (ref['n_ext'] + 16) * EPS
        _field(recs['interior_mean'][k], ref['interior_mean'], b_in, what + ('interior_mean',), worst)
        _field(recs['exterior_mean'][k], ref['exterior_mean'], b_ext, what + ('exterior_mean',), worst)
        _field(recs['contrast'][k], ref['contrast'], b_in + b_ext, what + ('contrast',), worst)
        _field(recs['fg_mean'][k], ref['fg_mean'], b_in, what + ('fg_mean',), worst, gs_abs)
        _field(recs['fg_std'][k], ref['fg_std'], 4 * ref['n_in'] * EPS, what + ('fg_std',), worst, 2 * gs_abs)
        with np.errstate(all='ignore'):
            want = po.compute_contrast(o.fg_offset, o.fg_fragment, im['g'], scale, offset, epsilon, bg)
        if np.isfinite(want):          # the oracle's own float64 value: it carries its own rounding, twice the bound
            assert abs(recs['contrast'][k] - want) <= 2 * (b_in + b_ext) * abs(want), what + ('oracle contrast', recs['contrast'][k], want)
        else:
            assert (np.isnan(want) and np.isnan(recs['contrast'][k])) or want == recs['contrast'][k], what + ('oracle contrast', recs['contrast'][k], want)
        if refined is None:
            continue
        if not refines:
            assert refined[k] is None and po.process_mask(o.fg_offset, o.fg_fragment, gs, m, stdamp) == (None, None), what
            assert (recs['r0'][k], recs['c0'][k], recs['h'][k], recs['w'][k]) == (*o.fg_offset, *o.fg_fragment.shape), what
            continue
        off, frag = po.process_mask(o.fg_offset, o.fg_fragment, gs, m, stdamp)
        differ = 'masks differ' if frag.shape != refined[k][1].shape else f'{int((frag != refined[k][1]).sum())} pixels differ'
        assert np.array_equal(refined[k][0], off) and refined[k][1].shape == frag.shape and np.array_equal(refined[k][1], frag), what + (differ,)


@pytest.mark.parametrize('name', list(LAUNCHES))
def test_launch_matches_the_full_image_oracle(gpu, name):
    """One launch of the case list: geometry, image shapes, parameter values, boundary lists in LDS and in the global pool
    (three pooled objects over two images: non-zero bpool_off), degenerate inputs, and the record fields on images with a constant of
    0, 1e2, 1e4 and 1e6 added (where sum(x^2) / n - mean^2 has no digit of the variance left)."""
    from superdsm_amd import postprocess
    L = LAUNCHES[name]
    items = _items(gpu, L['images'], L['settings'][1])
    got = postprocess.process_objects_gpu_multi(items, *L['settings']) if len(items) > 1 else [postprocess.process_objects_gpu(*items[0], *L['settings'])]
    worst = {}
    for j, (im, item, (recs, refined)) in enumerate(zip(L['images'], items, got)):
        _check_image(f"{L['name']} / image {j}", im, item[3], recs, refined, L['settings'], worst)
    print(L['name'], 'worst error / bound:', {k: f'{v:.3g}' for k, v in worst.items()})
    if L['name'] == 'no background':
        assert np.isnan(got[0][0]['exterior_mean'][0]) and np.isnan(got[0][0]['contrast'][0]) and got[0][1][0][1].any()
    if L['name'] == 'constant g':
        assert got[0][0]['interior_mean'][0] == np.inf and np.isnan(got[0][0]['contrast'][0])
    if L['name'] == 'dyadic plateaus':
        recs, refined = got[0]
        assert recs['fg_mean'][0] == 0.25 and recs['fg_std'][0] == 0
        assert np.array_equal(refined[0][0], [10, 8]) and refined[0][1].shape == (13, 13) and refined[0][1].sum() > 121      # grows into the 0.25 plateau only: not up, not to the right
    if L['name'] == 'pooled':
        assert [int(a > 12288) for r, _ in got for a in r['area']] == [0, 1, 0, 1, 0, 1, 0]


@pytest.mark.parametrize('settings', [(5, 5, 1e-4, 0, 2), (5, 5, 1e-4, 1, 0), (2.5, 2, 1e-4, 2, -1.5)])
def test_no_refinement(gpu, settings):
    """mask_max_distance = 0 or mask_stdamp <= 0: no refined mask, status 3, the contrast response as ever."""
    from superdsm_amd import postprocess
    L = LAUNCHES[f'parameters {testing.POST_PARAMETER_SETS[0]}']
    items = _items(gpu, L['images'], settings[1])
    recs, refined = postprocess.process_objects_gpu(*items[0], *settings)
    assert refined == [None] * len(recs) and (recs['status'] == 3).all()
    _check_image('no refinement', L['images'][0], items[0][3], recs, refined, settings, {})


def test_fractional_mask_distance_is_refused(gpu):
    from superdsm_amd import postprocess
    L = LAUNCHES[f'parameters {testing.POST_PARAMETER_SETS[0]}']
    items = _items(gpu, L['images'], 5)
    with pytest.raises(NotImplementedError):
        postprocess.process_objects_gpu(*items[0], 5, 5, 1e-4, 1.5, 2)
    with pytest.raises(NotImplementedError):
        postprocess.process_objects_gpu_multi(items, 5, 5, 1e-4, 2.5, 2)


def test_sets_match_the_oracle_image_by_image(gpu):
    """A set of 32 images of mixed shapes (images without objects first, in the middle and last) and a list of 35 (split by in_sets):
    every object of every image against the oracle; the list reversed gives the same bytes per image."""
    from superdsm_amd import _capi, postprocess
    images = testing.post_set_images()
    settings = testing.POST_DEFAULT
    items = _items(gpu, images, settings[1])
    assert len(items) == 35 and _capi.MAX_SET_IMAGES == 32
    worst = {}
    for name, part in (('set of 32', slice(0, 32)), ('list of 35', slice(0, 35))):
        got = postprocess.process_objects_gpu_multi(items[part], *settings)
        assert len(got) == len(items[part])
        for j, (im, item, (recs, refined)) in enumerate(zip(images[part], items[part], got)):
            _check_image(f'{name} / image {j}', im, item[3], recs, refined, settings, worst)
        back = postprocess.process_objects_gpu_multi(items[part][::-1], *settings)[::-1]
        for (recs, refined), (recs_b, refined_b) in zip(got, back):
            assert recs.tobytes() == recs_b.tobytes() and len(refined) == len(refined_b)
            for a, b in zip(refined, refined_b):
                assert a[0].tobytes() == b[0].tobytes() and a[1].shape == b[1].shape and a[1].tobytes() == b[1].tobytes()
    print('sets worst error / bound:', {k: f'{v:.3g}' for k, v in worst.items()})


class _Cover:
    def __init__(self, solution):
        self.solution = solution


def _stage_data(im):
    return dict(cover=_Cover(im['objects']), y_img=None, atoms=None, g_raw=im['g'], dsm_cfg=None)


def _stage_refined(stage, im, cfg, recs):
    """The refined masks the stage decides on, of every object of an image (those it then discards included): the batch of the
    stage's own prepared inputs, which must give the stage's records."""
    from superdsm_amd import postprocess
    P, _, objects, g_dev, g_mask, item = stage._prepare_host(_stage_data(im), cfg.get('postprocess', {}))
    bg, = stage._background_masks([item])
    again, refined = postprocess.process_objects_gpu(objects, g_dev, g_mask, bg, P['exterior_scale'], P['exterior_offset'], P['contrast_epsilon'],
                                                     P['mask_max_distance'], P['mask_stdamp'])
    assert again.tobytes() == recs.tobytes()
    return refined


def test_process_many_groups_by_settings_and_matches_the_oracle(gpu):
    """Postprocessing.process_many over four images of which two differ in exterior_scale: the records of every image (last_records,
    in the order of its objects) against the oracle with that image's settings, the refined masks of all objects and the surviving
    objects with their final masks against compute_contrast / process_mask.  The stage smooths on the device (pinned to SciPy within
    1e-15 absolute by test_postprocess_objects_match_reference_fixtures): fg_mean gets that much absolute allowance, fg_std twice."""
    from oracle import postprocess_oracle as po
    from superdsm_amd import config, postprocess
    images, settings = testing.post_stage_images()
    datas = [_stage_data(im) for im in images]
    cfgs = [config.Config({'postprocess': dict(s)}) for s in settings]
    stage = postprocess.Postprocessing()
    stage.process_many(datas, cfgs, out='muted')
    assert len(stage.last_records) == len(images)
    all_records = list(stage.last_records)
    worst = {}
    for j, (im, s, cfg, data, recs) in enumerate(zip(images, settings, cfgs, datas, all_records)):
        full = (s.get('exterior_scale', 5), 5, 1e-4, 1, 2)
        bg = _bg(im, 5)
        gs = ndi.gaussian_filter(im['g'], 3)
        kept = {id(p.original): p for p in data['postprocessed_objects']}
        _check_image(f'stage / image {j}', im, bg, recs, None, full, worst, gs_ref=gs, gs_abs=1e-15)     # the record fields; the masks follow
        refined = _stage_refined(stage, im, cfg, recs)
        for k, o in enumerate(im['objects']):
            off, frag = po.process_mask(o.fg_offset, o.fg_fragment, gs, 1, 2)
            assert np.array_equal(refined[k][0], off) and refined[k][1].shape == frag.shape and np.array_equal(refined[k][1], frag), (j, k)
            want = po.compute_contrast(o.fg_offset, o.fg_fragment, im['g'], *full[:3], bg)
            assert (id(o) in kept) == (want >= s['min_contrast'] and po.compute_eccentricity(o.fg_fragment) <= 0.99), (j, k, want)
            if id(o) in kept:
                off, frag = po.process_mask(o.fg_offset, o.fg_fragment, gs, 1, 2, True)
                assert np.array_equal(kept[id(o)].fg_offset, off) and np.array_equal(kept[id(o)].fg_fragment, frag), (j, k)
    # the same images one by one: the same records
    for data, cfg, recs in zip(datas, cfgs, all_records):
        stage(dict(data), cfg, out='muted')
        assert stage.last_records.tobytes() == recs.tobytes()
    print('stage worst error / bound:', {k: f'{v:.3g}' for k, v in worst.items()})


def test_stage_keeps_an_object_whose_contrast_is_nan(gpu):
    """No pixel near the object may enter the background estimate (the stage's own background mask is empty): exterior_mean and
    contrast are NaN, ``NaN < min_contrast`` is False and the reference keeps the object (postprocess.py:198), with the mask that
    process_mask gives it.  Through ``process`` and through ``process_many``."""
    from oracle import postprocess_oracle as po
    from superdsm_amd import config, postprocess
    im, s = testing.post_stage_nan_image()
    o, = im['objects']
    cfg = config.Config({'postprocess': dict(s)})
    gs = ndi.gaussian_filter(im['g'], 3)
    with np.errstate(all='ignore'):
        assert np.isnan(po.compute_contrast(o.fg_offset, o.fg_fragment, im['g'], 5, 5, 1e-4, _bg(im, 5)))
    off, frag = po.process_mask(o.fg_offset, o.fg_fragment, gs, 1, 2, True)
    stage = postprocess.Postprocessing()
    data = _stage_data(im)
    stage(data, cfg, out='muted')
    one = stage.last_records
    many = [_stage_data(im), _stage_data(im)]
    stage.process_many(many, cfg, out='muted')
    for d, recs in [(data, one)] + list(zip(many, stage.last_records)):
        assert len(recs) == 1 and np.isnan(recs['exterior_mean'][0]) and np.isnan(recs['contrast'][0]) and np.isfinite(recs['interior_mean'][0])
        _check_image('stage / no background', im, _bg(im, 5), recs, None, (5, 5, 1e-4, 1, 2), {}, gs_ref=gs, gs_abs=1e-15)
        kept, = d['postprocessed_objects']
        assert kept.original is o and np.array_equal(kept.fg_offset, off) and np.array_equal(kept.fg_fragment, frag)
