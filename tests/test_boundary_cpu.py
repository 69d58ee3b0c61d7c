"""The host definitions of the boundary distances (superdsm_amd/boundary.py) against second routes: the boundary by an edge-padded
comparison with the four shifted copies of the map and by ``_morph``, the minimal distances by SciPy's exact EDT, the scores by hand."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def disc(shape, centre, radius):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return (yy - centre[0]) ** 2 + (xx - centre[1]) ** 2 <= radius * radius


def catalogue():
    """{name: (a, b)}: 64 x 64 pairs of label maps with every case of the boundary definition."""
    s = (64, 64)
    out = {}
    a, b = np.zeros(s, np.int32), np.zeros(s, np.int32)
    a[disc(s, (30, 30), 12)] = 1
    b[disc(s, (32, 33), 11)] = 1
    out['disc'] = (a, b)
    a, b = np.zeros(s, np.int32), np.zeros(s, np.int32)
    a[disc(s, (30, 30), 14)] = 3
    a[disc(s, (30, 30), 5)] = 0
    b[disc(s, (31, 29), 13)] = 2
    out['disc with a hole'] = (a, b)
    a, b = np.zeros(s, np.int32), np.zeros(s, np.int32)
    a[20, 21] = 7
    b[disc(s, (22, 22), 6)] = 1
    out['one-pixel object'] = (a, b)
    a, b = np.zeros(s, np.int32), np.zeros(s, np.int32)
    a[0:9, 20:40] = 1
    a[55:64, 0:7] = 2
    b[0:7, 22:43] = 4
    b[disc(s, (63, 0), 9)] = 9
    out['border and corner'] = (a, b)
    a, b = np.zeros(s, np.int32), np.zeros(s, np.int32)
    a[10:40, 10:25] = 1
    a[10:40, 25:44] = 2
    a[40:50, 10:44] = 65535
    b[12:48, 8:40] = 1
    b[12:48, 40:50] = 300
    out['touching objects'] = (a, b)
    a, b = np.ones(s, np.int32), np.zeros(s, np.int32)
    b[disc(s, (30, 30), 10)] = 5
    out['a label fills the image'] = (a, b)
    a, b = np.zeros(s, np.int32), np.zeros(s, np.int32)
    for k, (cy, cx, r) in enumerate([(14, 14, 9), (16, 44, 10), (46, 30, 12)], start=1):
        a[disc(s, (cy, cx), r)] = k
        b[disc(s, (cy + 2, cx - 1), r - 1)] = 10 * k
    b[disc(s, (40, 30), 3)] = 4
    b[disc(s, (2, 60), 1)] = 5                                 # an expected object that nothing overlaps
    out['three pairs'] = (a, b)
    return out


CATALOGUE = catalogue()


def shifted_boundary(labels):
    """The second route: a pixel differs from one of the four shifted copies of the edge-padded map."""
    p = np.pad(labels, 1, mode='edge')
    c = p[1:-1, 1:-1]
    return (labels != 0) & ((c != p[:-2, 1:-1]) | (c != p[2:, 1:-1]) | (c != p[1:-1, :-2]) | (c != p[1:-1, 2:]))


@pytest.mark.parametrize('name', list(CATALOGUE))
def test_boundary_definition_by_shifted_copies_and_by_morphology(name):
    from superdsm_amd import _morph, boundary
    for labels in CATALOGUE[name]:
        want = shifted_boundary(labels)
        assert np.array_equal(boundary.boundary_mask(labels), want)
        present, offsets, coords = boundary.label_boundaries_host(labels)
        assert present.dtype == np.int32 and coords.dtype == np.int32 and present.tolist() == sorted(set(labels[labels != 0].tolist()))
        assert len(offsets) == len(present) + 1 and offsets[-1] == len(coords) == want.sum()
        for k, l in enumerate(present):
            mask = labels == l
            rr, cc = np.nonzero(mask & ~_morph.binary_erosion(mask, _morph.disk(1)))
            assert coords[offsets[k]:offsets[k + 1]].tolist() == np.stack([rr, cc], axis=1).tolist()         # raster order


def test_consequences_of_the_definition():
    from superdsm_amd import boundary
    a, _ = CATALOGUE['one-pixel object']
    assert boundary.label_boundaries_host(a)[2].tolist() == [[20, 21]]                       # its own boundary
    a, _ = CATALOGUE['disc with a hole']
    inner = boundary.boundary_mask(a) & disc(a.shape, (30, 30), 7)
    assert inner.sum() > 20                                                                  # the hole has an inner boundary
    a, _ = CATALOGUE['touching objects']
    m = boundary.boundary_mask(a)
    assert m[15, 24] and m[15, 25] and m[39, 20] and m[40, 20]                               # both sides of a contact
    a, _ = CATALOGUE['a label fills the image']
    present, offsets, coords = boundary.label_boundaries_host(a)
    assert present.tolist() == [1] and offsets.tolist() == [0, 0] and coords.shape == (0, 2)
    a, _ = CATALOGUE['border and corner']
    m = boundary.boundary_mask(a)
    assert not m[0, 30] and m[8, 30] and not m[63, 0] and not m[60, 0] and m[55, 3] and m[60, 6]     # the image border makes none


@pytest.mark.parametrize('name', list(CATALOGUE))
def test_minima_maxima_and_sums_against_the_exact_edt(name):
    from superdsm_amd import boundary
    a, b = CATALOGUE[name]
    table = boundary.pair_distances_host(a, b)
    assert table.dtype == boundary.PAIR_DISTANCE_DTYPE and table.dtype.itemsize == 64
    want_pairs = sorted({(int(x), int(y)) for x, y in zip(a.ravel(), b.ravel()) if x and y})
    assert list(zip(table['a'].tolist(), table['b'].tolist())) == want_pairs and len(want_pairs) >= 1      # no pair is left out
    ma, mb = shifted_boundary(a), shifted_boundary(b)
    for row in table:
        ba, bb = ma & (a == row['a']), mb & (b == row['b'])
        assert (row['boundary_a'], row['boundary_b'], row['reserved']) == (ba.sum(), bb.sum(), 0)
        assert row['flags'] == (0 if ba.any() else 1) | (0 if bb.any() else 2)
        if row['flags']:
            assert (row['max_d2_ab'], row['max_d2_ba'], row['sum_q_ab'], row['sum_q_ba'], row['nsd_num'], row['nsd_den']) == (-1, -1, 0, 0, 0, 0)
            continue
        to_b, to_a = ndi.distance_transform_edt(~bb), ndi.distance_transform_edt(~ba)
        d2_ab, d2_ba = np.rint(to_b[ba] ** 2).astype(np.int64), np.rint(to_a[bb] ** 2).astype(np.int64)
        assert np.array_equal(boundary.min_d2(np.argwhere(ba), np.argwhere(bb)), d2_ab)          # per pixel, exactly
        assert np.array_equal(boundary.min_d2(np.argwhere(bb), np.argwhere(ba)), d2_ba)
        assert (row['max_d2_ab'], row['max_d2_ba']) == (d2_ab.max(), d2_ba.max())
        assert row['sum_q_ab'] == sum(math.isqrt(int(v) << 32) for v in d2_ab) and row['sum_q_ba'] == sum(math.isqrt(int(v) << 32) for v in d2_ba)
        in_a, in_b = a == row['a'], b == row['b']
        union, one = in_a | in_b, in_a ^ in_b
        assert row['nsd_den'] == sum(math.isqrt(int(v) << 32) for v in np.rint(to_b[union] ** 2).astype(np.int64))
        assert row['nsd_num'] == sum(math.isqrt(int(v) << 32) for v in np.rint(to_b[one] ** 2).astype(np.int64))
        # the float route: q rounds every distance down by less than one quantum of 2^-16 pixel, so numerator and denominator (in
        # quanta) each fall short by less than the number of their pixels, and the ratio (<= 1) moves by less than pixels / denominator
        if row['nsd_den']:
            nsd = boundary.distance_scores(table)['pairs']
            got = float(nsd['nsd'][(table['a'] == row['a']) & (table['b'] == row['b'])][0])
            tol = union.sum() / row['nsd_den'] + 4 * np.finfo(np.float64).eps
            assert abs(got - to_b[one].sum() / to_b[union].sum()) <= tol


def test_hand_worked_cases():
    from superdsm_amd import boundary
    a, b = np.zeros((6, 7), np.int32), np.zeros((6, 7), np.int32)
    a[0, 0], b[3, 4] = 1, 2
    t = boundary.pair_distances_host(a, b, [(1, 2)])
    assert (t['max_d2_ab'][0], t['max_d2_ba'][0], t['sum_q_ab'][0], t['sum_q_ba'][0]) == (25, 25, 5 * 65536, 5 * 65536)
    assert (t['nsd_num'][0], t['nsd_den'][0]) == (5 * 65536, 5 * 65536)                      # a's pixel at distance 5, b's own at 0
    s = boundary.distance_scores(t)
    assert s['pairs']['hausdorff'][0] == 5.0 == s['pairs']['hausdorff_ab'][0] == s['pairs']['hausdorff_ba'][0] == s['pairs']['mean_surface'][0]
    assert s['pairs']['nsd'][0] == 1.0
    assert len(boundary.pair_distances_host(a, b)) == 0                                      # they do not overlap: no default pair
    # identical objects: 0 everywhere, NSD 0
    a, _ = CATALOGUE['disc']
    t = boundary.pair_distances_host(a, a)
    assert len(t) == 1 and (t['max_d2_ab'][0], t['max_d2_ba'][0], t['sum_q_ab'][0], t['sum_q_ba'][0], t['nsd_num'][0]) == (0, 0, 0, 0, 0) and t['nsd_den'][0] > 0
    s = boundary.distance_scores(t)
    assert s['pairs']['hausdorff'][0] == 0.0 == s['pairs']['nsd'][0] == s['pairs']['mean_surface'][0] == s['mean_hausdorff'] == s['mean_nsd']
    # identical one-pixel objects: a zero denominator, nan
    a = np.zeros((5, 5), np.int32)
    a[2, 3] = 4
    t = boundary.pair_distances_host(a, a)
    assert (t['flags'][0], t['max_d2_ab'][0], t['nsd_num'][0], t['nsd_den'][0]) == (0, 0, 0, 0)
    s = boundary.distance_scores(t)
    assert s['pairs']['hausdorff'][0] == 0.0 and math.isnan(s['pairs']['nsd'][0]) and math.isnan(s['mean_nsd']) and s['expected']['nsd_label'][0] == -1
    assert s['expected']['hausdorff_label'][0] == 4 and s['n_without_partner'] == 0
    # a flagged pair: nan scores, counted
    a, b = CATALOGUE['a label fills the image']
    t = boundary.pair_distances_host(a, b, [(1, 5), (1, 6), (2, 5)])
    assert t['flags'].tolist() == [1, 3, 1] and t['boundary_b'].tolist() == [int(shifted_boundary(b).sum()), 0, int(shifted_boundary(b).sum())]
    s = boundary.distance_scores(t)
    assert np.isnan(s['pairs']['hausdorff']).all() and np.isnan(s['pairs']['nsd']).all() and np.isnan(s['pairs']['mean_surface']).all()
    assert s['n_flagged'] == 3 and s['n_without_partner'] == 2 == s['n_expected'] and math.isnan(s['mean_hausdorff'])


def _rows(rows):
    from superdsm_amd import boundary
    t = np.zeros(len(rows), boundary.PAIR_DISTANCE_DTYPE)
    for k, r in enumerate(rows):
        for name, v in r.items():
            t[name][k] = v
    return t


def test_scores_decide_in_integers_with_ties_to_the_smaller_label():
    from superdsm_amd import boundary
    big = 2 ** 60
    t = _rows([
        dict(a=9, b=1, boundary_a=4, boundary_b=4, max_d2_ab=16, max_d2_ba=9, sum_q_ab=65536, sum_q_ba=3 * 65536, nsd_num=1, nsd_den=3),
        dict(a=4, b=1, boundary_a=4, boundary_b=4, max_d2_ab=9, max_d2_ba=16, nsd_num=2, nsd_den=6),                # ties in both: 4 wins
        dict(a=2, b=1, boundary_a=4, boundary_b=4, max_d2_ab=25, max_d2_ba=0, nsd_num=5, nsd_den=6),
        # two ratios that are one float64 (big / (3 big) and (big + 1) / (3 big + 3) round alike) but differ as fractions
        dict(a=7, b=2, boundary_a=1, boundary_b=1, max_d2_ab=4, max_d2_ba=4, nsd_num=big + 1, nsd_den=3 * big + 2),
        dict(a=8, b=2, boundary_a=1, boundary_b=1, max_d2_ab=1, max_d2_ba=4, nsd_num=big, nsd_den=3 * big),
        dict(a=5, b=3, boundary_a=0, boundary_b=7, max_d2_ab=-1, max_d2_ba=-1, flags=1),
    ])
    assert (big + 1) / (3 * big + 2) == big / (3 * big) and (big + 1) * (3 * big) > big * (3 * big + 2)
    s = boundary.distance_scores(t, expected_labels=[1, 2, 3, 11])
    e = s['expected']
    assert e['label'].tolist() == [1, 2, 3, 11] and e['n_partners'].tolist() == [3, 2, 0, 0]
    assert e['hausdorff_label'].tolist() == [4, 7, -1, -1] and e['hausdorff'][:2].tolist() == [4.0, 2.0] and np.isnan(e['hausdorff'][2:]).all()
    assert e['nsd_label'].tolist() == [4, 8, -1, -1] and e['nsd'][0] == 2 / 6
    assert s['n_expected'] == 4 and s['n_without_partner'] == 2 and s['n_flagged'] == 1
    assert s['mean_hausdorff'] == 3.0 and s['mean_nsd'] == (2 / 6 + big / (3 * big)) / 2
    p = s['pairs']
    assert p['hausdorff'][:3].tolist() == [4.0, 4.0, 5.0] and p['hausdorff_ab'][0] == 4.0 and p['hausdorff_ba'][0] == 3.0
    assert p['mean_surface'][0] == 0.5 and math.isnan(p['hausdorff'][5])
    # without the expected labels: those of the table
    s = boundary.distance_scores(t)
    assert s['expected']['label'].tolist() == [1, 2, 3] and s['n_without_partner'] == 1
    with pytest.raises(TypeError):
        boundary.distance_scores(np.zeros(3))


def test_error_paths_need_no_allocation():
    from superdsm_amd import boundary
    huge = np.broadcast_to(np.int32(0), (40000, 40000))                                     # a view of one element
    for f in (boundary.pair_distances_host, boundary.pair_distances, boundary.compare_boundaries):
        with pytest.raises(ValueError, match=r'H\^2 \+ W\^2 < 2\^31'):
            f(huge, huge)
        with pytest.raises(ValueError, match=r'H\^2 \+ W\^2 < 2\^31'):
            f(np.broadcast_to(np.float64(0), (40000, 40000)), huge)                          # the shape decides before the type
        with pytest.raises(ValueError, match=r'H\^2 \+ W\^2 < 2\^31'):
            f(np.broadcast_to(np.int32(0), (1, 46341)), np.broadcast_to(np.int32(0), (1, 46341)))
        with pytest.raises(ValueError, match='differ in shape'):
            f(np.zeros((4, 5), np.int32), np.zeros((5, 4), np.int32))
        with pytest.raises(TypeError):
            f(np.zeros((4, 5)), np.zeros((4, 5), np.int32))
        with pytest.raises(TypeError):
            f(np.zeros((4, 5), np.int32), np.zeros((4, 5), np.float32))
    for f in (boundary.label_boundaries_host, boundary.label_boundaries):
        with pytest.raises(ValueError, match=r'H\^2 \+ W\^2 < 2\^31'):
            f(huge)
        with pytest.raises(TypeError):
            f(np.zeros((4, 5)))
    boundary.check_shape((1, 46340))
    ok = np.zeros((1, 46340), np.int32)
    ok[0, 0] = ok[0, -1] = 1
    t = boundary.pair_distances_host(ok, ok)
    assert t['boundary_a'].tolist() == [2] and t['max_d2_ab'].tolist() == [0]
    bad = np.zeros((4, 5), np.int64)
    for v in (65536, -1, 2 ** 40):
        bad[1, 2] = v
        with pytest.raises(ValueError, match='labels 0 .. 65535'):
            boundary.pair_distances_host(bad, np.zeros((4, 5), np.int32))
        with pytest.raises(ValueError, match='labels 0 .. 65535'):
            boundary.label_boundaries_host(bad)
    with pytest.raises(ValueError, match='labels 0 .. 65535'):
        boundary.pair_distances(bad, np.zeros((4, 5), np.int32))                             # 2^40: int32 cannot hold it, refused on the host
    for pairs in ([(0, 1)], [(1, 65536)], [(-1, 2)]):
        with pytest.raises(ValueError, match='pairs'):
            boundary.pair_distances_host(np.zeros((4, 5), np.int32), np.zeros((4, 5), np.int32), pairs)


def test_constants_and_record_match_the_header():
    from superdsm_amd import _capi, boundary
    text = open(os.path.join(ROOT, 'include', 'sdsm.h')).read()
    defines = dict(re.findall(r'#define (SDSM_BOUNDARY_[A-Z_]+) (\d+)', text))
    assert {k: int(v) for k, v in defines.items()} == {'SDSM_BOUNDARY_MAX_LABELS': _capi.BOUNDARY_MAX_LABELS, 'SDSM_BOUNDARY_TILE': _capi.BOUNDARY_TILE,
                                                       'SDSM_BOUNDARY_CHUNK': _capi.BOUNDARY_CHUNK}
    body = re.search(r'typedef struct \{([^}]*)\} sdsm_pair_distance;', text).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r'(int32_t|int64_t)\s+([^;]+);', body):
        fields += [(n.strip(), '<i4' if ctype == 'int32_t' else '<i8') for n in names.split(',')]
    assert np.dtype(fields) == boundary.PAIR_DISTANCE_DTYPE == _capi.PAIR_DISTANCE_DTYPE and boundary.PAIR_DISTANCE_DTYPE.itemsize == 64
    assert boundary.MAX_LABELS == 65536 and boundary.QUANTUM == 65536


def test_the_kernels_quantiser_is_the_integer_root():
    """The code the distance kernel runs per query pixel, compiled for the host: every d2 around every square and both ends of the range."""
    from superdsm_amd import _capi, boundary
    rng = np.random.default_rng(11)
    sq = np.arange(1, 46341, dtype=np.int64) ** 2
    d2 = np.concatenate([np.arange(0, 4096), 2 ** 31 - 1 - np.arange(4096), sq - 1, sq, np.minimum(sq + 1, 2 ** 31 - 1), rng.integers(0, 2 ** 31, 200000),
                         [-1, -2 ** 31]]).astype(np.int32)
    out = np.full(len(d2), -7, np.int64)
    assert _capi.lib().sdsm_quantised_distance(d2.ctypes.data_as(C.c_void_p), len(d2), out.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(out[:-2], boundary.quantise(d2[:-2])) and out[-2:].tolist() == [0, 0]
    assert boundary.quantise([0, 1, 2, 25, 2 ** 31 - 1]).tolist() == [0, 65536, 92681, 5 * 65536, math.isqrt((2 ** 31 - 1) << 32)]


def test_work_list_names_every_chunk_once():
    from superdsm_amd import _capi, boundary
    ch = _capi.BOUNDARY_CHUNK
    counts_a, counts_b = np.zeros((2, 8, 2), np.int32), np.zeros((2, 8, 2), np.int32)
    counts_a[0, 1], counts_b[0, 2] = (3 * ch + 1, ch), (5, 5)
    counts_a[1, 3], counts_b[1, 4] = (7, 0), (9, 9)                                         # a without a boundary: flagged, no item
    counts_a[1, 5], counts_b[1, 4] = (2 * ch, ch + 1), (9, 9)
    rows = [(0, 1, 2, 0), (1, 3, 4, 0), (1, 5, 4, 0), (0, 7, 2, 0)]
    items = boundary.work_items(rows, counts_a, counts_b)
    assert items.dtype == np.int32 and (items[:, 3] == 0).all()
    want = [(0, 0, 0), (0, 1, 0)] + [(0, 2, c) for c in range(4)] + [(0, 3, 0)] + [(2, 0, 0), (2, 0, 1), (2, 1, 0), (2, 2, 0), (2, 2, 1), (2, 3, 0)]
    assert [tuple(r) for r in items[:, :3].tolist()] == want
    assert boundary.work_items(np.zeros((0, 4), np.int32), counts_a, counts_b).shape == (0, 4)


def test_csv_of_the_scores(tmp_path):
    import csv
    from superdsm_amd import boundary
    a, b = CATALOGUE['three pairs']
    s = boundary.compare_boundaries_host(a, b)
    assert s['n_expected'] == 5 and s['n_without_partner'] == 1 and s['expected']['hausdorff_label'].tolist() == [3, -1, 1, 2, 3]
    path = tmp_path / 'd.csv'
    boundary.write_distance_csv(path, s)
    rows = list(csv.reader(open(path)))
    assert rows[0][:4] == ['table', 'a', 'b', 'flags'] and len(rows) == 1 + len(s['pairs']) + len(s['expected'])
    head = rows[0]
    assert [r[0] for r in rows[1:]] == ['pairs'] * len(s['pairs']) + ['expected'] * 5
    assert float(rows[1][head.index('hausdorff')]) == s['pairs']['hausdorff'][0] and rows[1][head.index('label')] == ''
    assert int(rows[-1][head.index('label')]) == s['expected']['label'][-1] and rows[-1][head.index('a')] == ''
