"""The per-object post-processing without a GPU: the case generator of tests/test_postprocess_gpu.py meets the conditions that make its
demands fair (everything here comes from oracle/postprocess_oracle.py and np.longdouble, nothing from the kernel), the host's bit
packing round-trips, and objects outside their image are refused before anything reaches the device."""
import numpy as np
import pytest

from oracle import postprocess_oracle as po
from superdsm_amd import _capi, postprocess, testing

EPS = float(np.finfo(np.float64).eps)


def _bg(im, exterior_offset):
    if im['bg'] is not None:
        return im['bg']
    return po.background_mask(im['g'].shape, [(o.fg_offset, o.fg_fragment) for o in im['objects']], exterior_offset)


def test_extended_precision_is_extended():
    assert np.finfo(np.longdouble).eps < 1e-18


GS_ABS = 1e-15          # the device's Gaussian against SciPy's, absolute (test_postprocess_objects_match_reference_fixtures)


def _stage_launches():
    """The images of the stage tests as launches: the stage smooths the raw image itself, ``gs`` is SciPy's Gaussian of it."""
    import scipy.ndimage as ndi
    images, settings = testing.post_stage_images()
    nan_image, nan_settings = testing.post_stage_nan_image()
    out = []
    for j, (im, s) in enumerate(zip(images + [nan_image], settings + [nan_settings])):
        im = dict(im, gs=ndi.gaussian_filter(im['g'], 3))
        out.append(dict(name=f'stage {j}', images=[im], settings=(s.get('exterior_scale', 5), 5, 1e-4, 1, 2), exact=False, gs_abs=GS_ABS))
    return out


def test_guard_band_holds_for_every_mask_case():
    """In extended precision no pixel of a superset (dilation xor erosion) lies within 4 n eps (|mean| + amp) of a threshold, so a
    float64 evaluation in any order decides every pixel as process_mask does.  Exceptions, exact by construction: the dyadic
    plateaus and objects of one pixel (mean = the pixel, std = 0: the pixel ties with its own mean in every precision).  The stage
    images are smoothed on the device, within GS_ABS of the SciPy Gaussian the oracle reads: a pixel and the mean move by that much,
    the standard deviation by at most twice that (what the GPU test allows fg_std), so the margin must exceed the band by
    (2 + 2 stdamp) GS_ABS as well.  The oracle's own float64 contrast must meet the bound the GPU test holds the kernel to, (n_in + 16)
    eps + (n_ext + 16) eps against extended precision: the GPU test compares the two float64 values at twice that bound."""
    checked, worst = 0, 0.0
    launches = testing.post_launches()
    sets = [dict(name='set', images=testing.post_set_images(), settings=testing.POST_DEFAULT, exact=False)]
    stage = _stage_launches()
    for L in launches + sets + stage:
        scale, offset, epsilon, _, stdamp = L['settings']
        for j, im in enumerate(L['images']):
            bg = _bg(im, offset)
            for k, o in enumerate(im['objects']):
                what = (L['name'], j, k, o.tag)
                ref = testing.post_reference(im['g'], im['gs'], bg, o.fg_offset, o.fg_fragment, *L['settings'])
                assert ref['n_in'] == o.fg_fragment.sum()
                if ref['n_in'] == 0:
                    continue
                with np.errstate(all='ignore'):
                    c = po.compute_contrast(o.fg_offset, o.fg_fragment, im['g'], scale, offset, epsilon, bg)
                if np.isfinite(float(ref['contrast'])):
                    err = abs(c - float(ref['contrast'])) / abs(float(ref['contrast'])) / ((ref['n_in'] + ref['n_ext'] + 32) * EPS)
                    assert err <= 1, what + ('oracle contrast', c, ref['contrast'], err)
                    worst = max(worst, err)
                else:
                    assert np.isnan(c) and np.isnan(float(ref['contrast'])), what
                if L['exact'] or ref['n_in'] <= 1:
                    continue
                assert ref['margin'] > ref['band'] + (2 + 2 * stdamp) * L.get('gs_abs', 0.0), what + (ref['margin'], ref['band'])
                checked += 1
    print(f'oracle contrast: worst error / bound {worst:.3g}')
    assert checked > 160
    assert any(L['exact'] for L in launches) and len(stage) == 5


def test_stage_nan_case_has_no_background():
    """The rim around the object is narrower than the erosion disk: the oracle's background mask is empty and its contrast NaN."""
    im, s = testing.post_stage_nan_image()
    o, = im['objects']
    bg = _bg(im, 5)
    assert not bg.any()
    with np.errstate(all='ignore'):
        assert np.isnan(po.compute_contrast(o.fg_offset, o.fg_fragment, im['g'], 5, 5, 1e-4, bg))
    assert po.compute_eccentricity(o.fg_fragment) <= 0.99


def test_case_list_is_what_it_claims():
    launches = {L['name']: L for L in testing.post_launches()}
    combs = [im['objects'][0].fg_fragment for im in launches['combs']['images']]
    assert [testing.post_boundary_count(f) for f in combs] == [12288, 12289] == [testing.POST_LDS_BOUNDARY, testing.POST_LDS_BOUNDARY + 1]
    assert [int(f.sum()) for f in combs] == [12288, 12289]
    solids = [im['objects'][0].fg_fragment for im in launches['areas']['images']]
    assert [int(f.sum()) for f in solids] == [12288, 12289] and all(testing.post_boundary_count(f) < 500 for f in solids)
    # the pooled launch: the host's rule (areas > 12288) over the objects of the launch in order
    pooled = [int(o.fg_fragment.sum()) > testing.POST_LDS_BOUNDARY for im in launches['pooled']['images'] for o in im['objects']]
    assert pooled == [False, True, False, True, False, True, False] and len(launches['pooled']['images']) == 2
    assert sum(int(o.fg_fragment.sum()) > testing.POST_LDS_BOUNDARY for o in launches['pooled']['images'][1]['objects']) == 1
    # every parameter value of the list appears
    settings = [L['settings'] for L in launches.values()]
    assert {0.5, 2.5, 5, 7.3} <= {s[0] for s in settings} and {0, 0.5, 2, 5, 6.7} <= {s[1] for s in settings}
    assert {1, 2, 3, 5, 8, 16} <= {s[3] for s in settings} and {0.5, 1.5, 2, 3} <= {s[4] for s in settings}
    big = launches['520x696']
    assert big['settings'][3] == 16 and big['images'][0]['g'].shape == (520, 696)
    assert any(tuple(o.fg_offset) == (0, 0) for o in big['images'][0]['objects'])
    assert any(o.fg_offset[0] + o.fg_fragment.shape[0] == 520 and o.fg_offset[1] + o.fg_fragment.shape[1] == 696 for o in big['images'][0]['objects'])
    assert {im['g'].shape for L in launches.values() for im in L['images']} >= {(1, 1), (1, 300), (300, 1), (37, 53), (520, 696)}
    tags = [o.tag for o in launches['geometry']['images'][0]['objects']]
    assert tags.count('corner') == 4 and {'top', 'bottom', 'left', 'right', 'pixel', '1xN', 'Nx1', 'holes', 'two parts', 'empty rim', 'empty'} <= set(tags)
    # positive intensities: no sum of the record fields cancels
    assert all((im['g'] > 0).all() and (im['gs'] > 0).all() for L in launches.values() for im in L['images'])
    for c in testing.POST_CONSTANTS:
        ims, base = launches[f'fields + {c:g}']['images'], launches['fields + 0']['images']
        assert all(np.array_equal(a['g'], b['g'] + c) and np.array_equal(a['gs'], b['gs'] + c) for a, b in zip(ims, base))
    # the image sets
    images = testing.post_set_images()
    assert len(images) == 35 > _capi.MAX_SET_IMAGES == 32
    assert [i for i, im in enumerate(images[:32]) if not im['objects']] == [0, 15, 16, 31]
    assert len({im['g'].shape for im in images[:32]}) >= 5 and max(max(im['g'].shape) for im in images) <= 64


def test_stage_cases_decide_away_from_the_contrast_threshold():
    images, settings = testing.post_stage_images()
    kept = 0
    for im, s in zip(images, settings):
        bg = _bg(im, 5)
        for o in im['objects']:
            c = po.compute_contrast(o.fg_offset, o.fg_fragment, im['g'], s.get('exterior_scale', 5), 5, 1e-4, bg)
            assert abs(c - s['min_contrast']) > 1e-6
            kept += c >= s['min_contrast']
    assert 0 < kept < sum(len(im['objects']) for im in images)
    assert settings[0]['exterior_scale'] != settings[1].get('exterior_scale', 5)


def _word_buffer(windows, contents):
    """The device's output format built with NumPy: every window row-major, LSB first, in whole uint32 words."""
    words = postprocess.window_words(windows)
    off = postprocess._exclusive(words)
    buf = np.zeros(int(words.sum()), np.uint32)
    for o, win in zip(off, contents):
        for e in np.flatnonzero(win.reshape(-1)):
            buf[o + (e >> 5)] |= np.uint32(1) << np.uint32(e & 31)
    return buf.view(np.uint8), off, words


@pytest.mark.parametrize('m', [1, 3, 16])
def test_bit_packing_round_trips(m):
    H, W = 41, 37
    rng = np.random.default_rng(m)
    objs = [testing.PostFragment((0, 0), rng.random((5, 7)) < 0.6), testing.PostFragment((0, 30), rng.random((6, 7)) < 0.6),
            testing.PostFragment((38, 0), rng.random((3, 11)) < 0.6), testing.PostFragment((36, 34), rng.random((5, 3)) < 0.6),
            testing.PostFragment((15, 12), rng.random((9, 13)) < 0.6), testing.PostFragment((20, 20), np.ones((1, 1), bool)),
            testing.PostFragment((0, 0), rng.random((H, W)) < 0.5), testing.PostFragment((7, 3), rng.random((4, 8)) < 0.6)]
    boxes, words, packed, areas = postprocess.pack_fragments(objs)
    assert any((h * w) % 32 for _, _, h, w in boxes) and any((h * w) % 32 == 0 for _, _, h, w in boxes)
    for o, box, nw, buf, area in zip(objs, boxes, words, packed, areas):
        h, w = o.fg_fragment.shape
        assert tuple(box) == (o.fg_offset[0], o.fg_offset[1], h, w) and nw == (h * w + 31) // 32 and buf.size == 4 * nw and area == o.fg_fragment.sum()
        bits = np.unpackbits(buf, bitorder='little')
        assert np.array_equal(bits[:h * w].reshape(h, w).astype(bool), o.fg_fragment) and not bits[h * w:].any()
        u32 = buf.view(np.uint32)
        assert all(bool((u32[e >> 5] >> np.uint32(e & 31)) & 1) == bool(o.fg_fragment.reshape(-1)[e]) for e in range(h * w))
    windows = postprocess.grown_windows(boxes, H, W, m)
    for (r0, c0, h, w), (wr, wc, wh, ww) in zip(boxes, windows):
        assert (wr, wc) == (max(0, r0 - m), max(0, c0 - m)) and (wr + wh, wc + ww) == (min(H, r0 + h + m), min(W, c0 + w + m))
    assert (windows[:, 0] == 0).any() and (windows[:, 1] == 0).any() and (windows[:, 0] + windows[:, 2] == H).any() and (windows[:, 1] + windows[:, 3] == W).any()
    assert (windows[:, 0] > 0).any() and np.array_equal(postprocess.window_words(windows), (windows[:, 2] * windows[:, 3] + 31) // 32)
    # refined masks in the windows: random ones, one that is empty
    contents = [rng.random((int(wh), int(ww))) < 0.3 for _, _, wh, ww in windows]
    contents[4][:] = False
    new_bits, new_off, new_words = _word_buffer(windows, contents)
    recs = np.zeros(len(objs), _capi.POST_RECORD_DTYPE)
    want = []
    for k, ((wr, wc, wh, ww), win) in enumerate(zip(windows, contents)):
        full = np.zeros((H, W), bool)
        full[wr:wr + wh, wc:wc + ww] = win
        off, frag = po.extract_fragment(full)
        want.append((off, frag))
        if win.any():
            recs['r0'][k], recs['c0'][k], recs['h'][k], recs['w'][k] = off[0], off[1], frag.shape[0], frag.shape[1]
    got = postprocess._unpack_refined(recs, boxes, new_bits, new_off, new_words, H, W, m)
    for (a_off, a_frag), (b_off, b_frag) in zip(got, want):
        assert np.array_equal(a_off, b_off) and a_frag.shape == b_frag.shape and np.array_equal(a_frag, b_frag)
    assert got[4][1].shape == (1, 1) and not got[4][1].any()
    assert postprocess._unpack_refined(recs, boxes, None, new_off, new_words, H, W, 0) == [None] * len(objs)


@pytest.mark.parametrize('off, shape', [((-1, 0), (3, 3)), ((0, -1), (3, 3)), ((18, 0), (3, 3)), ((0, 28), (3, 3)), ((0, 0), (21, 3)), ((0, 0), (3, 31)),
                                        ((5, 5), (0, 3)), ((5, 5), (3, 0))])
def test_objects_outside_the_image_are_refused_on_the_host(monkeypatch, off, shape):
    """As render refuses them (test_objects_outside_the_image_are_refused): ValueError before the library is loaded or anything is
    uploaded -- the kernel reads its images at every pixel of a box."""
    def no_device():
        raise AssertionError('the device must not be reached')
    monkeypatch.setattr(_capi, 'lib', no_device)
    g = np.ones((20, 30))
    good = testing.PostFragment((2, 2), np.ones((3, 3), bool))
    bad = testing.PostFragment(off, np.ones(shape, bool))
    with pytest.raises(ValueError, match='outside'):
        postprocess.process_objects_gpu_multi([([good], g, g, None), ([good, bad], g, g, None)], *testing.POST_DEFAULT)
    with pytest.raises(ValueError, match='outside'):
        postprocess.process_objects_gpu([bad], g, g, None, *testing.POST_DEFAULT)


def test_fractional_mask_distance_is_refused_on_the_host(monkeypatch):
    monkeypatch.setattr(_capi, 'lib', lambda: (_ for _ in ()).throw(AssertionError('the device must not be reached')))
    g = np.ones((20, 30))
    with pytest.raises(NotImplementedError):
        postprocess.process_objects_gpu([testing.PostFragment((2, 2), np.ones((3, 3), bool))], g, g, None, 5, 5, 1e-4, 1.5, 2)
