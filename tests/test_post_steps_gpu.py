"""The exact steps of the post-processing stage on the device -- hole filling (sdsm_post_fill_holes), the background mask
(sdsm_post_background_multi), the glare test (sdsm_post_glare_multi) -- against SciPy and oracle/postprocess_oracle.py, bit for bit:
the outputs are booleans and integers, there are no tolerances.  The cases (superdsm_amd/testing.py) are checked without a GPU in
tests/test_post_steps_cpu.py."""
import numpy as np
import pytest
import scipy.ndimage as ndi

from superdsm_amd import testing

pytestmark = pytest.mark.gpu

FILL = testing.fill_cases()                                  # built once, at collection
FILL_WANT = {k: ndi.binary_fill_holes(a) for k, a in FILL.items()}
BG = testing.bg_cases()
GLARE = testing.glare_cases()


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    from superdsm_amd import _capi
    _capi.lib()
    return torch


def _same(got, want):
    return got.dtype == bool and got.shape == want.shape and np.array_equal(got, want)


# ---- hole filling ------------------------------------------------------------------------------------------------------------------------
def test_fill_every_case_in_one_launch(gpu):
    """Windows of all sizes in one launch (offsets), the one above the LDS cut-over among them (global-memory flood)."""
    from superdsm_amd import postprocess
    names = list(FILL)
    got = postprocess.fill_holes_gpu([FILL[k] for k in names])
    bad = [k for k, g in zip(names, got) if not _same(g, FILL_WANT[k])]
    assert not bad, bad
    back = postprocess.fill_holes_gpu([FILL[k] for k in names[::-1]])[::-1]
    assert all(np.array_equal(a, b) for a, b in zip(got, back))


@pytest.mark.parametrize('name', [k for k in FILL if 'cut-over' not in k])
def test_fill_alone(gpu, name):
    from superdsm_amd import postprocess
    got, = postprocess.fill_holes_gpu([FILL[name]])
    assert _same(got, FILL_WANT[name]), int((got != FILL_WANT[name]).sum())


def test_fill_window_equals_crop(gpu):
    """Every fragment inside larger clear windows at several offsets: the filled window is the filled fragment at its place."""
    from superdsm_amd import postprocess
    wins, want = [], []
    for name, a in FILL.items():
        if a.shape[0] > 100 or not a.any():
            continue
        rows, cols = np.flatnonzero(a.any(1)), np.flatnonzero(a.any(0))
        crop = a[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1]
        filled = ndi.binary_fill_holes(crop)
        for pads in testing.FILL_PADS:
            wins.append(testing.fill_embedded(crop, pads))
            want.append((name, pads, testing.fill_embedded(filled, pads)))
    got = postprocess.fill_holes_gpu(wins)
    bad = [(name, pads) for g, (name, pads, w) in zip(got, want) if not _same(g, w)]
    assert not bad, bad


# ---- background mask ---------------------------------------------------------------------------------------------------------------------
def _objects(items):
    return [testing.PostFragment(off, frag) for off, frag in items]


@pytest.mark.parametrize('r', testing.BG_RADII)
def test_background_mask(gpu, r):
    """Every case alone and the set of three images (different shapes, the one in the middle without objects) at one radius: equal to
    the oracle's erosion, and every image of the set equal to its single-image call."""
    from oracle import postprocess_oracle as po
    from superdsm_amd import postprocess
    single = {}
    for name, (shape, items) in BG.items():
        got = postprocess.background_mask_gpu(_objects(items), shape, r)
        assert got.is_cuda and got.dtype == gpu.uint8 and tuple(got.shape) == tuple(shape), name
        single[name] = got.cpu().numpy()
        want = po.background_mask(shape, items, r)
        assert set(np.unique(single[name])) <= {0, 1} and np.array_equal(single[name].astype(bool), want), (name, r, int((single[name].astype(bool) != want).sum()))
    assert single['no objects'].all() and single['1x1'].all() and not single['whole image'].any()
    many = postprocess.background_mask_gpu_multi([(_objects(BG[k][1]), BG[k][0]) for k in testing.BG_SET], r)
    for k, got in zip(testing.BG_SET, many):
        assert np.array_equal(got.cpu().numpy(), single[k]), (k, r)
    many = postprocess.background_mask_gpu_multi([(_objects(BG[k][1]), BG[k][0]) for k in BG], float(r))         # all cases as one set
    assert all(np.array_equal(got.cpu().numpy(), single[k]) for k, got in zip(BG, many))


# ---- glare test --------------------------------------------------------------------------------------------------------------------------
def _glare_want(c, min_layer, num_layers):
    """(pixels of the eroded mask, bits of the layers with several components) and the verdict, by the oracle's operations."""
    from oracle import postprocess_oracle as po
    off, frag = c['offset'], c['fragment']
    mask = po.binary_erosion(frag, po.disk(2))
    sect = c['g'][off[0]:off[0] + frag.shape[0], off[1]:off[1] + frag.shape[1]]
    data = sect[mask]
    bits = 0
    if data.size:
        with np.errstate(all='ignore'):
            for l, prop in enumerate(np.linspace(min_layer, 1, num_layers, endpoint=False)):
                bits |= int(ndi.label(mask & (sect > (data.max() - data.min()) * prop + data.min()))[0].max() > 1) << l
    try:
        with np.errstate(all='ignore'):
            verdict = po.is_glare(off, frag, c['g'], min_layer, num_layers)
    except ValueError:
        verdict = 'empty'
    return (int(mask.sum()), bits), verdict


@pytest.mark.parametrize('min_layer', [0, 0.5])
@pytest.mark.parametrize('num_layers', [1, 5, 32])
def test_glare(gpu, num_layers, min_layer):
    """All cases as one set (one image each), against the oracle's layers and verdict and against ``postprocess._is_glare``."""
    from superdsm_amd import postprocess
    names = list(GLARE)
    images = [([testing.PostFragment(GLARE[k]['offset'], GLARE[k]['fragment'])], gpu.as_tensor(GLARE[k]['g']).cuda()) for k in names]
    flags = postprocess.glare_flags_gpu_multi(images, min_layer, num_layers)
    for k, (objs, _), f in zip(names, images, flags):
        (count, bits), verdict = _glare_want(GLARE[k], min_layer, num_layers)
        assert f.shape == (1, 2) and (int(f[0, 0]), int(f[0, 1]) & 0xffffffff) == (count, bits), (k, f, count, bin(bits))
        if verdict == 'empty':
            with pytest.raises(ValueError):
                postprocess.glare_decision(f[0])
            with pytest.raises(ValueError):
                postprocess._is_glare(objs[0], GLARE[k]['g'], min_layer, num_layers)
            continue
        with np.errstate(all='ignore'):
            assert postprocess.glare_decision(f[0]) == verdict == postprocess._is_glare(objs[0], GLARE[k]['g'], min_layer, num_layers), k
        if (min_layer, num_layers) == (0.5, 5):
            assert verdict == GLARE[k]['expect'], k


def test_glare_objects_of_one_image_and_limits(gpu):
    """Several objects of one image in one launch (boxes at different places of the same smoothed image); 33 layers are refused."""
    from superdsm_amd import postprocess
    g = testing._peaks((80, 120), [(20, 25), (55, 60), (55, 84), (22, 90)], 7)
    items = [((4, 5), testing._ellipse(33, 41)), ((38, 40), testing._ellipse(35, 65)), ((10, 70), testing._rect(25, 40)), ((0, 0), testing._rect(80, 120))]
    objs = [testing.PostFragment(*it) for it in items]
    flags, = postprocess.glare_flags_gpu_multi([(objs, gpu.as_tensor(g).cuda())], 0.5, 5)
    verdicts = []
    for (off, frag), f in zip(items, flags):
        (count, bits), verdict = _glare_want(dict(g=g, offset=off, fragment=frag), 0.5, 5)
        assert (int(f[0]), int(f[1])) == (count, bits)
        assert postprocess.glare_decision(f) == verdict
        verdicts.append(verdict)
    assert verdicts == [True, False, True, False]
    with pytest.raises(NotImplementedError):
        postprocess.glare_flags_gpu_multi([(objs, gpu.as_tensor(g).cuda())], 0.5, 33)


def test_glare_threshold_is_rounded_twice(gpu):
    """The tie case found on the CPU: a pixel exactly at the twice-rounded threshold stays out of the layer; a fused multiply-add in the
    kernel would put it in as a second component."""
    from superdsm_amd import postprocess
    t = testing.glare_tie_case()
    obj = testing.PostFragment(t['offset'], t['fragment'])
    flags, = postprocess.glare_flags_gpu_multi([([obj], gpu.as_tensor(t['g']).cuda())], t['min_layer'], t['num_layers'])
    assert (int(flags[0, 0]), int(flags[0, 1])) == (int(t['fragment'].sum()), 0)
    assert postprocess.glare_decision(flags[0]) is True and postprocess._is_glare(obj, t['g'], t['min_layer'], t['num_layers']) is True


# ---- the stage ---------------------------------------------------------------------------------------------------------------------------
class _Cover:
    def __init__(self, solution):
        self.solution = solution


def _stage_data(im):
    return dict(cover=_Cover(im['objects']), y_img=None, atoms=None, g_raw=im['g'], dsm_cfg=None)


def _stage_want(im, s):
    """The surviving objects of one image, assembled from the oracle: index -> (offset, fragment)."""
    from oracle import postprocess_oracle as po
    items = [(o.fg_offset, o.fg_fragment) for o in im['objects']]
    offset, scale, fill = s.get('exterior_offset', 5), s.get('exterior_scale', 5), s.get('fill_holes', True)
    bg = po.background_mask(im['g'].shape, items, offset)
    gs = ndi.gaussian_filter(im['g'], 3)
    want, glare = {}, []
    for k, (off, frag) in enumerate(items):
        is_glare = s.get('min_glare_radius', np.inf) < np.sqrt(frag.sum() / np.pi) and po.is_glare(off, frag, gs, 0.5, 5)
        glare.append(bool(is_glare))
        new_off, new_frag = po.process_mask(off, frag, gs, 1, s.get('mask_stdamp', 2), fill)
        contrast = po.compute_contrast(off, frag, im['g'], scale, offset, 1e-4, bg)
        if new_frag.any() and not is_glare and contrast >= s['min_contrast'] and po.compute_eccentricity(frag) <= 0.99:
            want[k] = (new_off, new_frag)
    return want, glare


def test_stage_runs_without_the_host_passes(gpu, monkeypatch):
    """``process`` and ``process_many`` on images with mixed settings (one without hole filling, one with a finite glare radius and
    another exterior_offset, a third that shares the second's settings and so its launches, two with ``mask_stdamp = 0`` whose original
    fragments are filled) while the three host passes raise when called: the survivors and their masks are those assembled from the
    oracle's background_mask, process_mask(..., fill_holes) and is_glare."""
    import superdsm_amd._morph
    from superdsm_amd import config, postprocess
    images, settings = testing.post_steps_stage_images()
    wants = [_stage_want(im, s) for im, s in zip(images, settings)]
    assert any(w[1] for w in wants[1:]) and all(0 < len(w[0]) for w in wants) and any(len(w[0]) < len(im['objects']) for w, im in zip(wants, images))
    assert settings[1] == settings[2] and settings[3] == settings[4] and settings[3]['mask_stdamp'] == 0

    def gone(name):
        def fail(*a, **k):
            raise AssertionError(f'{name} was called')
        return fail
    monkeypatch.setattr(ndi, 'binary_fill_holes', gone('scipy.ndimage.binary_fill_holes'))
    monkeypatch.setattr(superdsm_amd._morph, 'binary_erosion', gone('_morph.binary_erosion'))
    monkeypatch.setattr(postprocess, '_is_glare', gone('postprocess._is_glare'))
    cfgs = [config.Config({'postprocess': dict(s)}) for s in settings]
    stage = postprocess.Postprocessing()
    many = [_stage_data(im) for im in images]
    stage.process_many(many, cfgs, out='muted')
    records = list(stage.last_records)
    singles = []
    for im, cfg in zip(images, cfgs):
        data = _stage_data(im)
        stage(data, cfg, out='muted')
        singles.append((data, stage.last_records))
    for j, (im, (want, _)) in enumerate(zip(images, wants)):
        for data, recs in ((many[j], records[j]), singles[j]):
            assert recs.tobytes() == records[j].tobytes()
            index = {id(o): k for k, o in enumerate(im['objects'])}
            kept = {index[id(p.original)]: p for p in data['postprocessed_objects']}
            assert sorted(kept) == sorted(want), (j, sorted(kept), sorted(want))
            for k, (off, frag) in want.items():
                assert np.array_equal(kept[k].fg_offset, off) and kept[k].fg_fragment.dtype == bool and kept[k].fg_fragment.shape == frag.shape and \
                    np.array_equal(kept[k].fg_fragment, frag), (j, k)
