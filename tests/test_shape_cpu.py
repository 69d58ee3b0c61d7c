"""The host definitions of the contour shape tables (superdsm_amd/shape.py) against independent statements: the perimeter classes
against the literal SciPy statement, the edge counts against a loop over the pixels, the hull against Qhull, the largest distance
against ``pdist``, the smallest caliper against exact fractions, and worked values by hand.  Parity against scikit-image is unpinned:
it is not available here."""
import csv
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import scipy.ndimage as ndi
from scipy.spatial import ConvexHull
from scipy.spatial.distance import pdist

from test_measure_cpu import Obj, ellipse, label_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def masks(seed=3, n=40):
    """Random masks: noise of several densities, ellipses, and noise eaten into ellipses."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        if k % 3 == 0:
            m = rng.random((rng.integers(1, 20), rng.integers(1, 40))) < rng.choice([0.2, 0.5, 0.8, 0.95])
        elif k % 3 == 1:
            m = ellipse(rng, 14)
        else:
            m = ellipse(rng, 14, erode=False)
            m = m & (rng.random(m.shape) < 0.9)
        if m.any():
            out.append(m)
    return out


def one(mask, offset=(0, 0), shape=None):
    from superdsm_amd import shape as sh
    mask = np.asarray(mask, bool)
    shape = shape or (mask.shape[0] + offset[0] + 3, mask.shape[1] + offset[1] + 3)
    table, offsets, vertices = sh.shape_objects_host([Obj(offset, mask)], shape)
    return table[0], vertices[offsets[0]:offsets[1]]


def test_class_counts_equal_the_bins_of_the_scipy_statement():
    for m in masks():
        P = m.astype(int)
        conv = ndi.convolve(P - ndi.binary_erosion(P, ndi.generate_binary_structure(2, 1), border_value=0), np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]]),
                            mode='constant', cval=0)
        hist = np.bincount(conv.ravel(), minlength=50)
        row, _ = one(m)
        assert row['perim_n1'] == hist[[5, 7, 15, 17, 25, 27]].sum()
        assert row['perim_n2'] == hist[[21, 33]].sum()
        assert row['perim_n3'] == hist[[13, 23]].sum()
        assert row['border_pixels'] == hist[1::2].sum()              # the odd bins are exactly the border pixels


def test_edge_counts_equal_a_loop_over_the_pixels():
    for m in masks(seed=4, n=15):
        h, w = m.shape
        inside = lambda r, c: 0 <= r < h and 0 <= c < w and m[r, c]
        er = ec = border = 0
        for r in range(h):
            for c in range(w):
                if m[r, c]:
                    a, b = (not inside(r - 1, c)) + (not inside(r + 1, c)), (not inside(r, c - 1)) + (not inside(r, c + 1))
                    er, ec, border = er + a, ec + b, border + (a + b > 0)
        row, _ = one(m)
        assert (row['area'], row['edges_r'], row['edges_c'], row['border_pixels']) == (m.sum(), er, ec, border)


def test_hull_equals_qhull_and_feret_equals_pdist():
    from superdsm_amd import shape as sh
    for m in masks(seed=5):
        row, verts = one(m, offset=(2, 5))
        corners = sh.pixel_corners(m, (2, 5))
        q = ConvexHull(corners)
        assert abs(row['hull_area2'] / 2 - q.volume) <= 1e-12 * q.volume
        assert sorted(map(tuple, verts.tolist())) == sorted(map(tuple, corners[q.vertices].tolist()))
        assert row['n_vertices'] == len(q.vertices) and row['hull_area2'] >= 2 * row['area']
        assert row['feret_max_d2'] == pdist(corners.astype(np.float64), 'sqeuclidean').max()          # integers below 2^53: exact
        # counter-clockwise from the smallest (row, column), no collinear triple
        v = [tuple(p) for p in verts.tolist()]
        assert v[0] == min(v)
        n = len(v)
        for k in range(n):
            o, a, b = v[k], v[(k + 1) % n], v[(k + 2) % n]
            assert (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0]) > 0


def test_min_feret_equals_a_brute_force_in_fractions():
    from superdsm_amd import shape as sh
    for m in masks(seed=6, n=20):
        table, offsets, vertices = sh.shape_objects_host([Obj((0, 0), m)], m.shape)
        hull = [tuple(p) for p in vertices.tolist()]
        n = len(hull)
        best = None
        for k in range(n):
            (r0, c0), (r1, c1) = hull[k], hull[(k + 1) % n]
            w2 = max(Fraction((abs((r1 - r0) * (q[1] - c0) - (c1 - c0) * (q[0] - r0))) ** 2, (r1 - r0) ** 2 + (c1 - c0) ** 2) for q in hull)
            best = w2 if best is None or w2 < best else best
        d = sh.derive(table, offsets, vertices)[0]
        # one division and one root there, one conversion and one root here, each correctly rounded: a few units in the last place
        assert abs(d['min_feret_diameter'] - math.sqrt(best)) <= 4 * np.spacing(math.sqrt(best))
        assert d['min_feret_diameter'] <= d['max_feret_diameter'] and d['feret_aspect_ratio'] >= 1
        assert 0 <= d['min_feret_angle'] < math.pi


def fields(row):
    return tuple(int(row[k]) for k in ('area', 'border_pixels', 'edges_r', 'edges_c', 'perim_n1', 'perim_n2', 'perim_n3', 'n_vertices', 'hull_area2', 'feret_max_d2'))


def test_worked_values():
    # a single pixel: the estimator gives 0
    row, v = one([[1]], (4, 6))
    assert fields(row) == (1, 1, 2, 2, 0, 0, 0, 4, 2, 2) and v.tolist() == [[4, 6], [5, 6], [5, 7], [4, 7]] and row['flags'] == 0
    # a 1 x 5 line: the ends have one border neighbour (v = 3, no class), the three inner ones two (v = 5)
    row, v = one(np.ones((1, 5)))
    assert fields(row) == (5, 5, 10, 2, 3, 0, 0, 4, 10, 26) and row['flags'] == 1
    # a 2 x 2 block: every pixel has two orthogonal and one diagonal border neighbour (v = 15)
    row, v = one(np.ones((2, 2)), (1, 1))
    assert fields(row) == (4, 4, 4, 4, 4, 0, 0, 4, 8, 8)
    # a plus sign: the centre is interior; every arm has two diagonal border neighbours (v = 21)
    row, v = one([[0, 1, 0], [1, 1, 1], [0, 1, 0]], (1, 1))
    assert fields(row) == (5, 4, 6, 6, 0, 4, 0, 8, 14, 10)
    # a diagonal of four pixels: the ends v = 11 (no class), the inner ones v = 21
    row, v = one(np.eye(4), (1, 1))
    assert fields(row) == (4, 4, 8, 8, 0, 2, 0, 6, 14, 32)
    assert v.tolist() == [[1, 1], [2, 1], [5, 4], [5, 5], [4, 5], [1, 2]]


def test_degenerate_objects_and_overlap():
    from superdsm_amd import shape as sh
    objs = [Obj((0, 0), np.zeros((3, 4))), Obj((1, 1), np.ones((2, 3))), Obj((0, 2), np.ones((3, 3)))]          # empty; two that overlap
    table, offsets, vertices = sh.shape_objects_host(objs, (3, 5))
    assert table[0].tobytes() == np.zeros(1, sh.TABLE_DTYPE).tobytes() and offsets.tolist() == [0, 0, 4, 8]
    assert (table['area'][1], table['flags'][1], table['area'][2], table['flags'][2]) == (6, 1, 9, 1)
    alone = sh.shape_objects_host(objs[2:], (3, 5))
    assert alone[0][0].tobytes()[4:] == table[2].tobytes()[4:] and (alone[2] == vertices[4:]).all()                 # each is measured alone
    full, _, v = sh.shape_objects_host([Obj((0, 0), np.ones((1, 1)))], (1, 1))
    assert fields(full[0]) == (1, 1, 2, 2, 0, 0, 0, 4, 2, 2) and full['flags'][0] == 1


def test_label_form_takes_other_labels_as_outside():
    from superdsm_amd import shape as sh
    rng = np.random.default_rng(8)
    labels = label_scene(rng)
    table, offsets, vertices = sh.shape_labels_host(labels)
    present = sorted(set(labels.ravel().tolist()) - {0})
    assert table['label'].tolist() == present
    for k, l in enumerate(present):
        rr, cc = np.nonzero(labels == l)
        f = (labels == l)[rr.min():rr.max() + 1, cc.min():cc.max() + 1]
        t, o, v = sh.shape_objects_host([Obj((rr.min(), cc.min()), f)], labels.shape)
        assert t[0].tobytes()[4:] == table[k].tobytes()[4:] and (v == vertices[offsets[k]:offsets[k + 1]]).all()
    # two touching labels: the common edge counts for both
    two = np.array([[1, 1, 2, 2]] * 2)
    t, _, _ = sh.shape_labels_host(two)
    assert t['edges_c'].tolist() == [4, 4] and t['border_pixels'].tolist() == [4, 4]
    # an absent label and the background give zero rows with keep_absent; another background label
    gap = np.array([[0, 1, 1], [0, 3, 3]])
    t, o, v = sh.shape_labels_host(gap, keep_absent=True)
    assert t['label'].tolist() == [0, 1, 2, 3] and t['area'].tolist() == [0, 2, 0, 2] and o.tolist() == [0, 0, 4, 4, 8]
    t, _, _ = sh.shape_labels_host(gap, background_label=3)
    assert t['label'].tolist() == [0, 1] and t['area'].tolist() == [2, 2]


def test_validation():
    from superdsm_amd import shape as sh
    with pytest.raises(ValueError):
        sh.shape_objects_host([Obj((0, 0), np.ones((2, 2)))], (70000, 4))
    with pytest.raises(ValueError):
        sh.shape_objects_host([Obj((3, 3), np.ones((2, 2)))], (4, 4))                   # the box leaves the image
    with pytest.raises(ValueError):
        sh.shape_objects_host([Obj((0, 0), np.ones((0, 2)))], (4, 4))                   # an empty box
    with pytest.raises(TypeError):
        sh.shape_labels_host(np.zeros((4, 4)))                                          # a float label map
    with pytest.raises(TypeError):
        sh.shape_labels_host(np.zeros((4, 4, 2), int))
    with pytest.raises(ValueError):
        sh.shape_labels_host(np.array([[0, -1]]))
    with pytest.raises(ValueError):
        sh.shape_labels_host(np.array([[0, 65536]]))


def test_record_layout_is_that_of_the_header():
    import ctypes as C
    from superdsm_amd import _capi, shape as sh
    text = open(os.path.join(ROOT, 'include', 'sdsm.h')).read()
    body = re.search(r'typedef struct \{([^}]*)\} sdsm_shape_record;', text).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    declared = []
    for ctype, names in re.findall(r'(int64_t|int32_t)\s+([^;]+);', body):
        declared += [(n.strip(), {'int64_t': 'i8', 'int32_t': 'i4'}[ctype]) for n in names.split(',')]
    assert declared == _capi._SHAPE_FIELDS
    assert _capi.SHAPE_RECORD_DTYPE.itemsize == 80 and _capi.SHAPE_RECORD_DTYPE.fields['n_vertices'][1] == 72
    assert sh.TABLE_DTYPE.names[1:] == _capi.SHAPE_RECORD_DTYPE.names
    assert int(re.search(r'#define SDSM_SHAPE_MAX_CHAIN (\d+)', text).group(1)) == _capi.SHAPE_MAX_CHAIN
    assert 'SDSM_SHAPE_MAX_WINDOW_WORDS (1ll << 26)' in text and _capi.SHAPE_MAX_WINDOW_WORDS == 1 << 26
    lib = _capi.lib()
    boxes = [(0, 0, h, w) for h in (0, 1, 2, 7, 300, 65535) for w in (0, 1, 3, 40, 65535)]
    assert sh.vertex_slots(boxes).tolist() == [lib.sdsm_shape_vertex_slots(b[2], b[3]) for b in boxes]


def test_vertex_slots_hold_every_hull():
    from superdsm_amd import shape as sh
    for m in masks(seed=9):
        row, _ = one(m)
        assert row['n_vertices'] <= sh.vertex_slots([(0, 0) + m.shape])[0]


def test_derive_on_a_zero_row_and_on_a_square():
    from superdsm_amd import shape as sh
    d = sh.derive(np.zeros(1, sh.TABLE_DTYPE), np.zeros(2, np.int64), np.zeros((0, 2), np.int32))[0]
    assert (d['area'], d['perimeter'], d['crack_perimeter'], d['convex_area'], d['convex_perimeter'], d['max_feret_diameter']) == (0, 0, 0, 0, 0, 0)
    assert all(math.isnan(d[k]) for k in ('circularity', 'solidity', 'min_feret_diameter', 'min_feret_angle', 'feret_aspect_ratio'))
    t, o, v = sh.shape_objects_host([Obj((1, 1), np.ones((4, 4)))], (8, 8))
    d = sh.derive(t, o, v)[0]
    # 12 border pixels: the 4 corners v = 5, the 8 others v = 15 -- all n1
    assert (d['perimeter'], d['crack_perimeter'], d['convex_area'], d['solidity'], d['convex_perimeter']) == (12.0, 16.0, 16.0, 1.0, 16.0)
    assert d['circularity'] == 4 * math.pi * 16 / 144 and d['max_feret_diameter'] == math.sqrt(32) and d['min_feret_diameter'] == 4.0
    assert d['feret_aspect_ratio'] == math.sqrt(32) / 4 and not d['on_boundary']
    # a 2 x 6 rectangle: the smallest caliper is across the long edges
    t, o, v = sh.shape_objects_host([Obj((0, 0), np.ones((2, 6)))], (8, 8))
    d = sh.derive(t, o, v)[0]
    assert d['min_feret_diameter'] == 2.0 and d['min_feret_angle'] == 0.0 and d['on_boundary']
    mixed = sh.shape_objects_host([Obj((0, 0), np.array([[0, 1, 1], [1, 1, 0], [1, 0, 0]]))], (5, 5))
    dm = sh.derive(*mixed)[0]
    tm = mixed[0][0]
    assert dm['perimeter'] == tm['perim_n1'] + tm['perim_n2'] * math.sqrt(2) + tm['perim_n3'] * ((1 + math.sqrt(2)) / 2)


def test_csv_writer(tmp_path):
    from superdsm_amd import shape as sh
    res = sh.shape_objects_host([Obj((1, 1), np.ones((2, 2))), Obj((0, 0), np.zeros((1, 1)))], (6, 6))
    path = tmp_path / 'shape.csv'
    sh.write_shape_csv(path, *res)
    rows = list(csv.reader(open(path)))
    assert rows[0][:4] == ['label', 'area', 'on_boundary', 'perimeter'] and rows[0][-1] == 'hull' and len(rows) == 3
    rec = dict(zip(rows[0], rows[1]))
    assert rec['area'] == '4' and rec['perimeter'] == '4.0' and rec['hull_area2'] == '8' and rec['hull'] == '1 1;3 1;3 3;1 3'
    assert dict(zip(rows[0], rows[2]))['circularity'] == 'nan' and dict(zip(rows[0], rows[2]))['hull'] == ''
    assert open(path).read().startswith('"label","area"')
