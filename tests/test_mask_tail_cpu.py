"""The plain reference of the mask tail (superdsm_amd.testing.tail_reference) against the CPU oracle at the oracle's own parameters, and on
the crafted ring cases whose flags are written out by hand.  No GPU."""
import numpy as np
import pytest

from oracle import oracle
from superdsm_amd import testing


def _oracle_mask(rec, frag, shape):
    full = np.zeros(shape, bool)
    if frag.any():
        r, c = rec['fg_offset']
        full[r:r + frag.shape[0], c:c + frag.shape[1]] = frag
    return full


@pytest.mark.parametrize('workload,step', [('synthetic256', 1), ('bbbc039_like', 9)])
def test_reference_reproduces_the_oracle_at_the_oracles_parameters(workload, step):
    """Sign of the longdouble surface at the oracle's (theta, xi) = the oracle's fragment, box and flag; at most 1 region pixel in 10 000
    inside the guard band (measured: none of 127 944 and 97 951 pixels; smallest |S| / A 2^-22.3 on synthetic256, 2^-28.5 on the 56
    candidates of bbbc039_like)."""
    scene = testing.make_scene(workload)
    fps, cfg, y, atoms = scene['footprints'][::step], scene['dsm_cfg'], scene['y'], scene['atoms']
    recs, frags, params = oracle.compute_objects(y, None, atoms, fps, cfg, nthreads=0)
    total = undecided = solved = 0
    smallest = np.inf
    for k, fp in enumerate(fps):
        if recs['status'][k] in (2, 3):                     # trivial / error: no surface
            continue
        solved += 1
        ref = testing.tail_reference(y, None, atoms, fp, cfg, params[k][:6], params[k][6:])
        assert ref['n_pixels'] == recs['N'][k] and params[k].size == 6 + recs['M'][k]
        expected = testing.tail_paste(ref['box'], ref['expected'], y.shape)
        decided = testing.tail_paste(ref['box'], ref['decided'], y.shape)
        region = testing.tail_paste(ref['box'], ref['region'], y.shape)
        mine = _oracle_mask(recs[k], frags[k], y.shape)
        assert not (mine & ~region).any()
        assert np.array_equal(mine[decided], expected[decided]), (k, int((mine != expected)[decided].sum()))
        und = int((region & ~decided).sum())
        if ref['fg_box'] is None:
            assert not frags[k].any() and tuple(recs['fg_shape'][k]) == (1, 1)
        else:
            assert tuple(recs['fg_offset'][k]) + tuple(recs['fg_shape'][k]) == ref['fg_box'], k
        if ref['on_boundary'] is not None:
            assert ref['on_boundary'] == recs['on_boundary'][k], k
        else:
            undecided += 1                                  # (counted with the pixels: a flag inside the band)
        total += ref['n_pixels']
        undecided += und
        smallest = min(smallest, float(ref['ratio'].min()))
    print(f'{workload}: {solved} candidates, {total} region pixels, {undecided} undecided, smallest |S| / A = 2^{np.log2(smallest):.1f}')
    assert solved >= 40
    assert undecided * 10000 <= total, (undecided, total)


@pytest.mark.parametrize('shape', testing.TAIL_CRAFTED_SHAPES)
def test_crafted_ring_cases_are_what_they_claim(shape):
    """The flags and masks written out by hand in testing.tail_crafted_cases; nothing undecided (dyadic surfaces, far from the band)."""
    im = testing.tail_crafted_image(shape)
    H, W = shape
    region = oracle.region_mask(im['y'], None, im['atoms'], im['footprint'], im['cfg']['background_margin'])
    assert region.all() and (im['y'] > 0).sum() > 1
    sm = oracle.smooth_matrix(region, im['cfg']['smooth_amount'], im['cfg']['gaussian_shape_multiplier'], im['cfg']['smooth_subsample'])
    assert sm.M > 0
    cases = testing.tail_crafted_cases(shape, sm.M)
    assert len(cases) == 10
    for name, case in cases.items():
        ref = testing.tail_reference(im['y'], None, im['atoms'], im['footprint'], im['cfg'], case['params'][:6], case['params'][6:])
        assert ref['box'] == (0, 0, H, W) and ref['decided'].all() and ref['ratio'].min() > 2.0 ** -20 and ref['ring_ratio'] > 2.0 ** -20, name
        assert ref['on_boundary'] == case['on_boundary'], name
        if case['mask'] == 'empty':
            assert not ref['expected'].any() and ref['fg_box'] is None, name
        elif case['mask'] == 'full':
            assert ref['expected'].all() and ref['fg_box'] == (0, 0, H, W), name
        else:                                               # intricate: both values inside runs of 4 pixels, many changes along a row
            e = ref['expected']
            assert 0.3 < e.mean() < 0.7 and (e[:, 1:] != e[:, :-1]).sum() > 3 * H and (e[1:] != e[:-1]).any(axis=1).sum() > H // 3, name
            cells = e[:, :W // 4 * 4].reshape(H, W // 4, 4)
            assert (cells.any(axis=2) & ~cells.all(axis=2)).sum() > H, name


def test_ring_positions_by_hand():
    """One surface per ring position: positive at exactly that pixel's line.  The ring is rows -1 and H and columns -1 and W of the image,
    normalised by H - 1 and W - 1, corners included -- and nothing farther out or nearer in."""
    shape = H, W = 24, 37
    im = testing.tail_crafted_image(shape)
    th = lambda **kw: testing._pixel_theta(shape, **kw)
    flag = lambda theta: testing.tail_reference(im['y'], None, im['atoms'], im['footprint'], im['cfg'], theta)['on_boundary']
    assert flag(th(r=-1.0, k=-0.5)) == 1 and flag(th(r=-1.0, k=-1.5)) == 0              # positive from row -1 / from row -2 upwards
    assert flag(th(r=1.0, k=0.5 - H)) == 1 and flag(th(r=1.0, k=-0.5 - H)) == 0         # from row H / from row H + 1 downwards
    assert flag(th(c=-1.0, k=-0.5)) == 1 and flag(th(c=-1.0, k=-1.5)) == 0
    assert flag(th(c=1.0, k=0.5 - W)) == 1 and flag(th(c=1.0, k=-0.5 - W)) == 0
    assert flag(th(r=-1.0, c=-1.0, k=-1.5)) == 1 and flag(th(r=-1.0, c=-1.0, k=-2.5)) == 0     # the corner (-1, -1) alone / nothing
    assert flag(th(r=1.0, c=1.0, k=0.5 - H - W)) == 1 and flag(th(r=1.0, c=1.0, k=-0.5 - H - W)) == 0
    assert flag(th(k=0.0)) is None and flag(th(k=2.0 ** -60)) == 1                       # exactly zero: inside the band; A = |c|: decided
    for i, name, params, expect in testing.tail_two_image_cases((5, 5)):
        other = testing.TAIL_CRAFTED_SHAPES[i]
        im2 = testing.tail_crafted_image(other)
        ref = testing.tail_reference(im2['y'], None, im2['atoms'], im2['footprint'], im2['cfg'], params[:6])
        assert ref['on_boundary'] == expect and not ref['expected'].any(), name
        # the same surface in PIXEL coordinates, looked at with the other image's ring: the opposite answer for the controls, none for the others
        Ho, Wo = testing.TAIL_CRAFTED_SHAPES[1 - i]
        zu, zv = other[0] - 1.0, other[1] - 1.0
        S = lambda r, c: 2 * params[3] * r / zu + 2 * params[4] * c / zv + params[5]
        ring = [S(r, c) for r in (-1, Ho) for c in range(-1, Wo + 1)] + [S(r, c) for c in (-1, Wo) for r in range(-1, Ho + 1)]
        assert (max(ring) > 0) == (expect == 0), name


def test_counts_ignore_zeros_of_either_sign():
    sc = testing.straddling_rows_scene()
    ref = testing.tail_reference(sc['y'], None, sc['atoms'], sc['footprints'][0], sc['cfg'], np.zeros(6))
    region = testing.tail_paste(ref['box'], ref['region'], sc['y'].shape)
    zeros = region & (sc['y'] == 0)
    assert zeros.sum() == 10 and np.signbit(sc['y'][zeros]).sum() == 4
    assert ref['n_positive'] + ref['n_negative'] + 10 == ref['n_pixels'] and ref['n_positive'] > 1
    assert ref['box'][3] == 77 and ref['box'][3] % 32 and ref['box'][3] > 64
    assert ref['on_boundary'] is None and not ref['decided'].any()          # theta = 0: S = 0 = A everywhere
