"""What the cases of tests/test_post_steps_gpu.py claim about themselves (superdsm_amd/testing.py: hole filling, background mask,
glare test), the packing helpers, and the argument checks of the device functions, which come before any device call.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.ndimage as ndi

from superdsm_amd import _capi, postprocess, testing


def _objects(items):
    return [testing.PostFragment(off, frag) for off, frag in items]


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library fails the test."""
    def refuse():
        raise AssertionError('the device library was used')
    monkeypatch.setattr(_capi, 'lib', refuse)


def test_windows_round_trip():
    rng = np.random.default_rng(1)
    wins = [rng.random((h, w)) < 0.5 for w in testing.FILL_WIDTHS for h in (1, 7, 9)] + [np.ones((1, 1), bool), np.zeros((40, 1), bool), rng.random((1, 40)) < 0.5]
    dims, offsets, bits = postprocess.pack_windows(wins)
    assert dims.dtype == np.int32 and offsets.dtype == np.int64 and bits.dtype == np.uint8 and bits.size % 4 == 0
    assert [tuple(d) for d in dims] == [w.shape for w in wins]
    words = [(w.size + 31) // 32 for w in wins]
    assert list(offsets) == list(np.cumsum([0] + words[:-1])) and bits.size == 4 * sum(words)
    back = postprocess.unpack_windows(bits, offsets, dims)
    assert all(a.dtype == bool and np.array_equal(a, b) for a, b in zip(back, wins))
    # the format of pack_fragments: the same bits
    boxes, nwords, packed, _ = postprocess.pack_fragments(_objects([((0, 0), w) for w in wins]))
    assert np.array_equal(np.concatenate(packed), bits) and list(nwords) == words


def test_flood_workspace_cut_over():
    cut = _capi.POST_FLOOD_WORDS
    assert cut == testing.FILL_LDS_WORDS == 4096
    off, total = postprocess.flood_workspace([(2048, 33), (2049, 33), (1, 1), (129, 1024)], 2)
    assert list(off) == [-1, 0, -1, 2 * 4098] and total == 2 * 4098 + 2 * 129 * 32
    C = testing.fill_cases()
    words = lambda a: a.shape[0] * ((a.shape[1] + 31) // 32)
    assert words(C['at the cut-over']) == cut and words(C['above the cut-over']) == cut + 2
    assert all(words(a) <= cut for k, a in C.items() if k != 'above the cut-over')


def test_fill_cases_are_what_they_say():
    C = testing.fill_cases()
    fill = ndi.binary_fill_holes
    assert {(1, 1), (1, 40), (40, 1)} <= {a.shape for a in C.values()}
    for w in testing.FILL_WIDTHS:
        shapes = [a.shape for k, a in C.items() if k.startswith('random') and a.shape[1] == w]
        assert shapes and all(h % 2 == 1 and ((h * w) % 32 or w % 32 == 0) for h, w in shapes)   # odd heights; unless the width is whole words, rows straddle words and the last word is partial
        assert fill(C[f'frame {w}']).sum() > C[f'frame {w}'].sum()
    assert fill(C['ring']).all() and not C['ring'].all()
    assert np.array_equal(fill(C['ring open to the border']), C['ring open to the border'])
    d = C['ring with a diagonal gap']
    assert fill(d).sum() > d.sum() and np.array_equal(fill(d, structure=np.ones((3, 3))), d)   # closed for 4-, open for 8-connected background
    n = C['nested rings']
    assert ndi.label(~n)[1] == 3 and fill(n)[1:-1, 1:-1].all()
    assert C['all ones'].all() and not C['all zeros'].any()
    s = C['spiral 63']
    assert s.shape == (63, 63) and ndi.label(~s)[1] == 1 and (~s).sum() > 1900 and np.array_equal(fill(s), s)
    # one pixel wide: every corridor pixel has at most two corridor neighbours
    nb = sum(np.roll(np.pad(~s, 1), sh, ax)[1:-1, 1:-1] for sh, ax in ((1, 0), (-1, 0), (1, 1), (-1, 1)))
    assert (nb[~s] <= 2).all()
    assert np.array_equal(fill(C['comb']), C['comb']) and fill(C['comb in a frame']).all()


def test_window_equals_crop():
    """Filling a fragment inside a larger clear window equals filling the fragment: what lets the stage fill the refined windows."""
    for name, a in testing.fill_cases().items():
        if a.shape[0] > 100 or not a.any():
            continue
        rows, cols = np.flatnonzero(a.any(1)), np.flatnonzero(a.any(0))
        crop = a[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1]
        want = ndi.binary_fill_holes(crop)
        for pads in testing.FILL_PADS:
            got = ndi.binary_fill_holes(testing.fill_embedded(crop, pads))
            assert np.array_equal(got, testing.fill_embedded(want, pads)), (name, pads)


def test_bg_cases_are_what_they_say():
    from oracle import postprocess_oracle as po
    C = testing.bg_cases()
    assert set(testing.BG_SET) <= set(C) and C['no objects'][1] == [] and C['1x1'][0] == (1, 1)
    assert len({C[k][0] for k in testing.BG_SET}) == 3 and testing.BG_RADII == (0, 1, 5, 16, 32)
    assert C['corners'][0][1] % 64
    for r in testing.BG_RADII:
        assert po.background_mask(*C['no objects'], r).all() and po.background_mask(*C['1x1'], r).all()
        assert not po.background_mask(*C['whole image'], r).any()
    shape, objs = C['corners']
    fg = ~po.background_mask(shape, objs, 0)
    assert fg[0, 0] and fg[0, -1] and fg[-1, 0] and fg[-1, -1]
    assert po.background_mask(shape, [], 32).all()                                           # the border does not erode
    shape, objs = C['overlapping']                                                            # assignment, not union: a later box clears bits
    union = np.zeros(shape, bool)
    for off, frag in objs:
        union[off[0]:off[0] + frag.shape[0], off[1]:off[1] + frag.shape[1]] |= frag
    assert (union & po.background_mask(shape, objs, 0)).any()


def test_glare_cases_are_what_they_say():
    from oracle import postprocess_oracle as po
    for name, c in testing.glare_cases().items():
        obj = testing.PostFragment(c['offset'], c['fragment'])
        if c['expect'] == 'empty':
            assert not po.binary_erosion(c['fragment'], po.disk(2)).any()
            with pytest.raises(ValueError):
                po.is_glare(c['offset'], c['fragment'], c['g'])
            with pytest.raises(ValueError):
                postprocess._is_glare(obj, c['g'])
            continue
        with np.errstate(all='ignore'):
            assert po.is_glare(c['offset'], c['fragment'], c['g']) == c['expect'] == postprocess._is_glare(obj, c['g']), name
    c = testing.glare_cases()['two peaks, highest layer only']
    m = po.binary_erosion(c['fragment'], po.disk(2))
    sect = c['g'][c['offset'][0]:c['offset'][0] + m.shape[0], c['offset'][1]:c['offset'][1] + m.shape[1]]
    data = sect[m]
    counts = [ndi.label(m & (sect > (data.max() - data.min()) * p + data.min()))[1] for p in np.linspace(0.5, 1, 5, endpoint=False)]
    assert counts == [1, 1, 1, 1, 2]
    c = testing.glare_cases()['diagonal contact']
    layer = c['g'][c['offset'][0]:, c['offset'][1]:][:41, :70] > 0.5
    assert ndi.label(layer)[1] == 2 and ndi.label(layer, structure=np.ones((3, 3)))[1] == 1
    c = testing.glare_cases()['border on all sides']
    assert c['fragment'].all() and po.binary_erosion(c['fragment'], po.disk(2)).all()


def test_tie_case_separates_fused_from_twice_rounded():
    """A triple for which (max - min) * prop + min rounded once (a fused multiply-add) is smaller than rounded twice, in exact rational
    arithmetic; the pixel placed at the twice-rounded threshold is not above it, so the host definition keeps one component."""
    from oracle import postprocess_oracle as po
    t = testing.glare_tie_case()
    assert t is not None, 'no triple found'
    mx, mn, prop = t['max'], t['min'], t['prop']
    d = mx - mn
    assert Fraction(d) == Fraction(mx) - Fraction(mn)
    product = Fraction(d) * Fraction(prop)
    twice = float(np.float64(d) * np.float64(prop)) + mn
    assert Fraction(np.float64(d) * np.float64(prop)) != product                             # the product is rounded
    fused = (product + Fraction(mn)).numerator / (product + Fraction(mn)).denominator        # correctly rounded
    assert twice == t['twice'] and fused == t['fused'] and fused < twice
    assert abs(Fraction(fused) - (product + Fraction(mn))) <= abs(Fraction(twice) - (product + Fraction(mn)))
    assert np.linspace(t['min_layer'], 1, t['num_layers'], endpoint=False).tolist() == [prop]
    g, off, frag = t['g'], t['offset'], t['fragment']
    sect = g[off[0]:off[0] + frag.shape[0], off[1]:off[1] + frag.shape[1]]
    assert po.binary_erosion(frag, po.disk(2)).all() and sect.max() == mx and sect.min() == mn and (sect == twice).sum() == 1
    assert not (sect > twice)[sect == twice].any() and (sect > fused)[sect == twice].all()
    assert ndi.label(sect > twice)[1] == 1 and ndi.label(sect > fused)[1] == 2               # the host definition excludes the pixel; a fused threshold would not
    assert po.is_glare(off, frag, g, t['min_layer'], t['num_layers']) is True
    assert postprocess._is_glare(testing.PostFragment(off, frag), g, t['min_layer'], t['num_layers']) is True


def test_glare_decision():
    assert postprocess.glare_decision(np.array([12, 0])) is True
    assert postprocess.glare_decision(np.array([12, 0b10000])) is False
    with pytest.raises(ValueError):
        postprocess.glare_decision(np.array([0, 0]))


def test_background_radius():
    assert [postprocess.background_radius(v) for v in (0, 1, 5, 5.0, 32, np.int64(7))] == [0, 1, 5, 5, 32, 7]
    assert [postprocess.background_radius(v) for v in (-1, 33, 2.5, np.inf, np.nan, None)] == [None] * 6


class _G:
    """Stands in for a device tensor where only the shape is looked at before the refusal."""
    shape = (20, 30)


def test_arguments_are_checked_before_any_device_call(no_device):
    inside, outside = _objects([((2, 3), np.ones((4, 5), bool))]), _objects([((17, 3), np.ones((4, 5), bool))])
    negative = _objects([((-1, 0), np.ones((2, 2), bool))])
    for bad in (outside, negative):
        with pytest.raises(ValueError):
            postprocess.background_mask_gpu(bad, (20, 30), 5)
        with pytest.raises(ValueError):
            postprocess.background_mask_gpu_multi([(inside, (20, 30)), (bad, (20, 30))], 5)
        with pytest.raises(ValueError):
            postprocess.glare_flags_gpu_multi([(bad, _G())], 0.5, 5)
    for offset in (2.5, 33, -1):
        with pytest.raises(NotImplementedError):
            postprocess.background_mask_gpu(inside, (20, 30), offset)
    with pytest.raises(ValueError):
        postprocess.background_mask_gpu(inside, (0, 30), 5)
    with pytest.raises(NotImplementedError):
        postprocess.glare_flags_gpu_multi([(inside, _G())], 0.5, 33)
    with pytest.raises(ValueError):
        postprocess.glare_flags_gpu_multi([(inside, _G())], 0.5, 0)
    for bad in (np.zeros((0, 4), bool), np.zeros(5, bool), np.zeros((2, 2, 2), bool)):
        with pytest.raises(ValueError):
            postprocess.fill_holes_gpu([np.ones((2, 2), bool), bad])
    assert postprocess.fill_holes_gpu([]) == []


def test_stage_case_is_what_it_says():
    """The stage-level scene: holes that the filling closes, an object the glare test removes and one it keeps."""
    from oracle import postprocess_oracle as po
    images, settings = testing.post_steps_stage_images()
    assert settings[0]['fill_holes'] is False and 'fill_holes' not in settings[1] and np.isfinite(settings[1]['min_glare_radius'])
    assert 'min_glare_radius' not in settings[0]
    verdicts = []
    for o in images[1]['objects']:
        assert np.sqrt(o.fg_fragment.sum() / np.pi) > settings[1]['min_glare_radius']
        verdicts.append(po.is_glare(o.fg_offset, o.fg_fragment, ndi.gaussian_filter(images[1]['g'], 3)))
    assert True in verdicts and False in verdicts
    for im in images:
        assert any(ndi.binary_fill_holes(o.fg_fragment).sum() > o.fg_fragment.sum() for o in im['objects'])
