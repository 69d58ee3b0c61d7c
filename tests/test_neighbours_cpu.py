"""The neighbourhood tables of superdsm_amd/neighbours.py without a GPU: the ``*_host`` definitions against SciPy's exact Euclidean distance
transform and a plain-Python walk over the pixel sides, hand-worked maps, ``derive`` on a scene with ties, the graph and the CSV, the
argument errors, the orchestration of the GPU form over a host restatement of the launch, and the two inline helpers of
csrc/sdsm_neighbours.h through their exported symbols and alone under the sanitizers."""
import csv
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import scipy.ndimage as ndi

from test_measure_cpu import label_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REACHES = (1, 2, 25, 400)


def rows(pairs):
    return [tuple(int(v) for v in p) for p in pairs.tolist()]


def scenes():
    rng = np.random.default_rng(21)
    out = [label_scene(rng) for _ in range(3)] + [label_scene(rng, (61, 47), 25)]
    framed = np.zeros((40, 50), np.int32)                    # labels that lie on the frame, where the frame makes no boundary
    framed[:, :12], framed[10:30, 20:31], framed[35:, 30:], framed[:5, 12:15] = 1, 2, 3, 4
    return out + [framed]


def edt_minima(labels, queries=None):
    """{(a, b): smallest squared distance from a pixel of a (of ``queries``, if given) to a pixel of b}, a != b, by the exact EDT."""
    present = [int(l) for l in np.unique(labels) if l != 0]
    out = {}
    for b in present:
        d = ndi.distance_transform_edt(labels != b)
        d2 = np.rint(d * d).astype(np.int64)                 # (the EDT is exact: the square of its root rounds back to the integer)
        for a in present:
            if a != b:
                where = (labels == a) if queries is None else (labels == a) & queries
                if where.any():
                    out[(a, b)] = int(d2[where].min())
    return out


# ---- the definitions ------------------------------------------------------------------------------------------------------------------
def test_pairs_against_the_exact_distance_transform():
    from superdsm_amd import neighbours
    for labels in scenes():
        minima = edt_minima(labels)
        assert all(minima[(a, b)] == minima[(b, a)] for a, b in minima)
        for max_d2 in REACHES:
            want = sorted((a, b, d2) for (a, b), d2 in minima.items() if a < b and d2 <= max_d2)
            got = neighbours.neighbour_pairs_host(labels, max_d2)
            assert got.dtype == neighbours.PAIR_DTYPE and [r[:3] for r in rows(got)] == want
            assert ((got['contact_edges'] > 0) == (got['min_d2'] == 1)).all()
        assert len(neighbours.neighbour_pairs_host(labels, 400)) > len(neighbours.neighbour_pairs_host(labels, 1)) > 0


def test_boundary_pixels_alone_find_every_minimum():
    from superdsm_amd import boundary
    for labels in scenes():
        edge = boundary.boundary_mask(labels)
        assert (edge != (labels != 0)).any()                 # there are interior pixels, or this would show nothing
        assert edt_minima(labels, edge) == edt_minima(labels)


def side_walk(labels, n_labels):
    """[edges_background, edges_labels, edges_frame] per label and {(a, b): crack edges}, by a walk over every side of every pixel."""
    H, W = labels.shape
    counts, cracks = np.zeros((n_labels, 3), np.int64), {}
    for r in range(H):
        for c in range(W):
            l = int(labels[r, c])
            if l == 0:
                continue
            for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
                if not (0 <= rr < H and 0 <= cc < W):
                    counts[l, 2] += 1
                elif labels[rr, cc] == 0:
                    counts[l, 0] += 1
                elif labels[rr, cc] != l:
                    counts[l, 1] += 1
                    if l < labels[rr, cc]:                   # (each crack edge is met from both sides: counted from the smaller label)
                        cracks[(l, int(labels[rr, cc]))] = cracks.get((l, int(labels[rr, cc])), 0) + 1
    return counts, cracks


def test_label_rows():
    from superdsm_amd import boundary, neighbours
    for labels in scenes():
        n_labels = int(labels.max()) + 1
        counts, cracks = side_walk(labels, n_labels)
        present, offsets, _ = boundary.label_boundaries_host(labels)
        for max_d2 in REACHES:
            table, pairs = neighbours.neighbour_labels_host(labels, max_d2), neighbours.neighbour_pairs_host(labels, max_d2)
            assert table.dtype == neighbours.LABEL_DTYPE and len(table) == n_labels and (table['reserved'] == 0).all()
            assert table['area'].tolist() == np.bincount(labels.ravel(), minlength=n_labels).tolist()
            assert table['boundary'][present].tolist() == np.diff(offsets).tolist() and table['boundary'].sum() == offsets[-1]
            assert np.array_equal(np.stack([table[k] for k in ('edges_background', 'edges_labels', 'edges_frame')], axis=1), counts)
            assert {(a, b): n for a, b, _, n in rows(pairs) if n} == cracks
            sums = np.zeros(n_labels, np.int64)
            np.add.at(sums, pairs['a'], pairs['contact_edges'])
            np.add.at(sums, pairs['b'], pairs['contact_edges'])
            assert sums.tolist() == table['edges_labels'].tolist()
            assert (table['close'] <= table['boundary']).all() and table[0].tolist()[:3] == (0, 0, 0) and table['boundary'][0] == table['close'][0] == 0
            # close, pixel by pixel: a boundary pixel with another label >= 1 in its disk
            edge = boundary.boundary_mask(labels)
            if max_d2 <= 25:
                close = np.zeros(n_labels, np.int64)
                R = math.isqrt(max_d2)
                padded = np.pad(labels, R)
                yy, xx = np.mgrid[-R:R + 1, -R:R + 1]
                disk = yy * yy + xx * xx <= max_d2
                for r, c in zip(*np.nonzero(edge)):
                    window = padded[r:r + 2 * R + 1, c:c + 2 * R + 1][disk]
                    close[labels[r, c]] += bool(((window != 0) & (window != labels[r, c])).any())
                assert table['close'].tolist() == close.tolist()
        wide = neighbours.neighbour_labels_host(labels, 2, n_labels=n_labels + 5)
        assert len(wide) == n_labels + 5 and wide[:n_labels].tobytes() == neighbours.neighbour_labels_host(labels, 2).tobytes() and not wide[n_labels:].view(np.uint8).any()


# ---- hand-worked cases ----------------------------------------------------------------------------------------------------------------
def test_two_pixels_at_offset_3_4():
    from superdsm_amd import neighbours
    for flip in (False, True):
        m = np.zeros((9, 9), np.uint8)
        m[1, 2], m[4, 6] = 1, 2
        m = m[:, ::-1] if flip else m
        assert len(neighbours.neighbour_pairs_host(m, 24)) == 0
        assert rows(neighbours.neighbour_pairs_host(m, 25)) == [(1, 2, 25, 0)]
        assert neighbours.neighbour_labels_host(m, 24)['close'].tolist() == [0, 0, 0]
        t = neighbours.neighbour_labels_host(m, 25)
        assert t['close'].tolist() == [0, 1, 1] and t['boundary'].tolist() == [0, 1, 1] and t['edges_background'].tolist() == [0, 4, 4]


def test_checkerboard_and_stripes():
    from superdsm_amd import neighbours
    yy, xx = np.mgrid[0:6, 0:8]
    board = 1 + (yy + xx) % 2
    assert rows(neighbours.neighbour_pairs_host(board, 1)) == [(1, 2, 1, 6 * 7 + 5 * 8)]         # every inner side is a crack edge
    t = neighbours.neighbour_labels_host(board, 1)
    assert t['area'].tolist() == [0, 24, 24] and t['boundary'].tolist() == [0, 24, 24] == t['close'].tolist()
    assert t['edges_labels'].tolist() == [0, 82, 82] and t['edges_frame'].tolist() == [0, 14, 14] and t['edges_background'].tolist() == [0, 0, 0]
    stripes = np.tile(np.array([1, 2, 3, 1]), (5, 1))        # columns one pixel wide; label 1 at both ends, once beside 2, once beside 3
    assert rows(neighbours.neighbour_pairs_host(stripes, 1)) == [(1, 2, 1, 5), (1, 3, 1, 5), (2, 3, 1, 5)]
    assert rows(neighbours.neighbour_pairs_host(stripes, 4)) == [(1, 2, 1, 5), (1, 3, 1, 5), (2, 3, 1, 5)]
    t = neighbours.neighbour_labels_host(stripes, 1)
    assert t['edges_labels'].tolist() == [0, 10, 10, 10] and t['edges_frame'].tolist() == [0, 4 + 10, 2, 2] and t['close'].tolist() == [0, 10, 5, 5]
    gap = np.array([[1, 0, 0, 2, 0, 3]])
    assert rows(neighbours.neighbour_pairs_host(gap, 4)) == [(2, 3, 4, 0)]
    assert rows(neighbours.neighbour_pairs_host(gap, 9)) == [(1, 2, 9, 0), (2, 3, 4, 0)]
    assert rows(neighbours.neighbour_pairs_host(gap, 25)) == [(1, 2, 9, 0), (1, 3, 25, 0), (2, 3, 4, 0)]


def test_a_ring_with_another_label_in_its_hole():
    from superdsm_amd import neighbours
    m = np.zeros((11, 11), np.int32)
    m[1:10, 1:10] = 1
    m[3:8, 3:8] = 0
    m[5, 5] = 7
    assert rows(neighbours.neighbour_pairs_host(m, 8)) == []
    assert rows(neighbours.neighbour_pairs_host(m, 9)) == [(1, 7, 9, 0)]
    t = neighbours.neighbour_labels_host(m, 9)
    assert t['area'][[1, 7]].tolist() == [81 - 25, 1] and t['boundary'][[1, 7]].tolist() == [32 + 20, 1]
    assert t['close'][[1, 7]].tolist() == [4, 1]             # the four pixels of the inner outline straight across from the centre
    assert t['edges_background'][[1, 7]].tolist() == [36 + 20, 4] and t['edges_frame'].sum() == 0 and len(t) == 8
    m[4:7, 4:7] = 7                                           # grown until it touches nothing, then fills the hole
    assert rows(neighbours.neighbour_pairs_host(m, 4)) == [(1, 7, 4, 0)]
    m[3:8, 3:8] = 7
    assert rows(neighbours.neighbour_pairs_host(m, 1)) == [(1, 7, 1, 20)]
    t = neighbours.neighbour_labels_host(m, 1)
    assert t['edges_labels'][[1, 7]].tolist() == [20, 20] and t['close'][[1, 7]].tolist() == [20, 16] and t['boundary'][[1, 7]].tolist() == [32 + 20, 16]


def test_full_empty_and_thin_maps():
    from superdsm_amd import neighbours
    full = np.full((4, 6), 3, np.int64)
    t = neighbours.neighbour_labels_host(full, 4096)
    assert len(neighbours.neighbour_pairs_host(full, 4096)) == 0
    assert t[3].tolist() == (0, 0, 20, 24, 0, 0, 0) and not t[:3].view(np.uint8).any()          # no boundary: frame edges only
    empty = np.zeros((5, 7), np.uint16)
    t = neighbours.neighbour_labels_host(empty, 2)
    assert len(neighbours.neighbour_pairs_host(empty, 2)) == 0 and len(t) == 1 and t[0].tolist() == (0, 0, 0, 35, 0, 0, 0)
    one = neighbours.neighbour_labels_host(np.array([[2]]), 1)
    assert one[2].tolist() == (0, 0, 4, 1, 0, 0, 0) and len(neighbours.neighbour_pairs_host(np.array([[2]]), 1)) == 0
    line = np.array([[1, 1, 2, 0, 3]])
    for m in (line, line.T):
        assert rows(neighbours.neighbour_pairs_host(m, 1)) == [(1, 2, 1, 1)]
        assert rows(neighbours.neighbour_pairs_host(m, 4)) == [(1, 2, 1, 1), (2, 3, 4, 0)]
        t = neighbours.neighbour_labels_host(m, 4)
        assert t['edges_frame'].tolist() == [0, 5, 2, 3] and t['edges_labels'].tolist() == [0, 1, 1, 0] and t['edges_background'].tolist() == [0, 0, 1, 1]
        assert t['boundary'].tolist() == [0, 1, 1, 1] and t['close'].tolist() == [0, 1, 1, 1] and t['area'].tolist() == [1, 2, 1, 1]
    none = np.zeros((0, 4), np.int32)
    assert len(neighbours.neighbour_pairs_host(none, 1)) == 0 and neighbours.neighbour_labels_host(none, 1).tolist() == [(0, 0, 0, 0, 0, 0, 0)]


# ---- derive, the graph, the CSV ---------------------------------------------------------------------------------------------------------
def tie_scene():
    """Label 5 in the middle; 2 and 9 two pixels to its left and right (d2 = 4 both), 3 touching it from above, 6 alone far away."""
    m = np.zeros((12, 30), np.int32)
    m[5, 10] = 5
    m[5, 8], m[5, 12], m[4, 10] = 2, 9, 3
    m[10, 28] = 6
    return m


def test_derive_on_a_scene_with_ties():
    from superdsm_amd import neighbours
    m = tie_scene()
    table, pairs = neighbours.neighbour_labels_host(m, 4), neighbours.neighbour_pairs_host(m, 4)
    assert rows(pairs) == [(2, 5, 4, 0), (3, 5, 1, 1), (5, 9, 4, 0)]             # 2 - 3 and 3 - 9 are at d2 = 5
    d = neighbours.derive(table, pairs)
    assert d.dtype == neighbours.DERIVED_DTYPE and d['label'].tolist() == [2, 3, 5, 6, 9]
    five = d[2]
    assert (five['n_neighbours'], five['n_touching']) == (3, 1)
    assert (five['first_label'], five['first_d2'], five['first_distance']) == (3, 1, 1.0)
    assert (five['second_label'], five['second_d2'], five['second_distance']) == (2, 4, 2.0)      # 2 before 9: the smaller label wins the tie
    assert five['close_fraction'] == 1.0 and five['contact_fraction'] == 0.25 and not five['on_frame']
    two, six = d[0], d[3]
    assert (two['n_neighbours'], two['first_label'], two['first_d2'], two['second_label'], two['second_d2']) == (1, 5, 4, -1, -1)
    assert two['first_distance'] == 2.0 and np.isnan(two['second_distance']) and two['contact_fraction'] == 0.0
    assert (six['n_neighbours'], six['n_touching'], six['first_label'], six['first_d2'], six['second_label'], six['second_d2']) == (0, 0, -1, -1, -1, -1)
    assert np.isnan(six['first_distance']) and np.isnan(six['second_distance']) and six['close_fraction'] == 0.0
    wider = neighbours.derive(neighbours.neighbour_labels_host(m, 5), neighbours.neighbour_pairs_host(m, 5))
    assert (wider[1]['n_neighbours'], wider[1]['first_label'], wider[1]['second_label'], wider[1]['second_d2']) == (3, 5, 2, 5)
    assert wider[1]['second_distance'] == math.sqrt(5)
    # 0 / 0: a label that fills its image has no boundary; one on the frame
    full = np.full((3, 3), 1)
    d = neighbours.derive(neighbours.neighbour_labels_host(full, 1), neighbours.neighbour_pairs_host(full, 1))
    assert np.isnan(d['close_fraction'][0]) and d['contact_fraction'][0] == 0.0 and d['on_frame'][0]
    third = np.array([[1, 1, 2]])
    d = neighbours.derive(neighbours.neighbour_labels_host(third, 1), neighbours.neighbour_pairs_host(third, 1))
    assert d['contact_fraction'].tolist() == [1 / 6, 1 / 4] and d['close_fraction'].tolist() == [1.0, 1.0]


def test_adjacency_and_csv(tmp_path):
    from superdsm_amd import neighbours
    m = tie_scene()
    table, pairs = neighbours.neighbour_labels_host(m, 5), neighbours.neighbour_pairs_host(m, 5)
    offsets, nb = neighbours.adjacency(pairs, len(table))
    assert offsets.dtype == np.int64 and nb.dtype == np.int32 and len(offsets) == 11 and offsets[-1] == 2 * len(pairs)
    lists = {l: nb[offsets[l]:offsets[l + 1]].tolist() for l in range(10)}
    assert lists == {0: [], 1: [], 2: [3, 5], 3: [2, 5, 9], 4: [], 5: [2, 3, 9], 6: [], 7: [], 8: [], 9: [3, 5]}
    assert neighbours.adjacency(pairs[:0], 3)[0].tolist() == [0, 0, 0, 0]
    path = tmp_path / 'n.csv'
    neighbours.write_neighbour_csv(path, table, pairs)
    read = list(csv.reader(open(path)))
    head, body = read[0], read[1:]
    derived = neighbours.derive(table, pairs)
    assert head[:3] == ['table', 'label', 'edges_background'] and [r[0] for r in body] == ['labels'] * len(derived) + ['pairs'] * len(pairs)
    for r, d in zip(body, derived):                          # the round trip: integers and floats come back as they were
        assert int(r[head.index('label')]) == d['label'] and int(r[head.index('area')]) == table['area'][d['label']]
        for k in neighbours.DERIVED_DTYPE.names[1:]:
            back = r[head.index(k)]
            assert back == repr(d[k].item()) and (np.isnan(d[k]) if back == 'nan' else type(d[k].item())(eval(back)) == d[k])
        assert r[head.index('min_d2')] == ''
    for r, p in zip(body[len(derived):], pairs):
        assert tuple(int(r[head.index(k)]) for k in neighbours.PAIR_DTYPE.names) == tuple(p.tolist()) and r[head.index('label')] == ''


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def test_reach_d2():
    from superdsm_amd import neighbours
    assert [neighbours.reach_d2(d) for d in (0, 1, 2, 64, np.int64(5))] == [0, 1, 4, 4096, 25]
    assert neighbours.reach_d2(Fraction(3, 2)) == 2 and neighbours.reach_d2(Fraction(7, 5)) == 1 and neighbours.reach_d2(Fraction(141422, 100000)) == 2
    for bad in (1.5, '2', None, True, np.float64(2)):
        with pytest.raises(TypeError):
            neighbours.reach_d2(bad)
    with pytest.raises(ValueError):
        neighbours.reach_d2(-1)


def test_argument_errors():
    from superdsm_amd import neighbours
    m = tie_scene()
    for f in (neighbours.neighbour_pairs_host, neighbours.neighbour_labels_host, neighbours.neighbour_tables, lambda l, d: neighbours.neighbour_tables_many([l], d)):
        for bad in (0, -1, 4097):
            with pytest.raises(ValueError, match='max_d2'):
                f(m, bad)
        for bad in (2.0, None, '4', True):
            with pytest.raises(TypeError, match='max_d2'):
                f(m, bad)
        with pytest.raises(TypeError, match='integer image'):
            f(m.astype(np.float64), 2)
        with pytest.raises(ValueError, match='two-dimensional'):
            f(m[0], 2)
        with pytest.raises(ValueError, match=r'H\^2 \+ W\^2'):
            f(np.lib.stride_tricks.as_strided(np.zeros(1, np.int8), (40000, 40000), (0, 0)), 2)
    for f in (neighbours.neighbour_pairs_host, neighbours.neighbour_labels_host):
        for v in (-1, 65536):
            bad = m.copy()
            bad[0, 0] = v
            with pytest.raises(ValueError, match='labels 0 .. 65535'):
                f(bad, 2)
    with pytest.raises(ValueError, match='n_labels = 9'):
        neighbours.neighbour_labels_host(m, 2, n_labels=9)
    for bad in (0, 65537):
        with pytest.raises(ValueError, match='n_labels'):
            neighbours.neighbour_labels_host(m, 2, n_labels=bad)
        with pytest.raises(ValueError, match='n_labels'):
            neighbours.neighbour_tables(m, 2, n_labels=bad)
    with pytest.raises(TypeError, match='n_labels'):
        neighbours.neighbour_labels_host(m, 2, n_labels=10.0)
    for bad in (0, 3, -4):
        with pytest.raises(ValueError, match='capacity'):
            neighbours.neighbour_tables(m, 2, capacity=bad)
    with pytest.raises(ValueError, match='largest label is 70000'):
        neighbours.neighbour_tables(np.full((2, 2), 70000), 2)
    with pytest.raises(ValueError, match='labels 0 .. 65535'):
        neighbours.neighbour_tables(np.full((2, 2), 2 ** 31, np.int64), 2)
    table, pairs = neighbours.neighbour_labels_host(m, 4), neighbours.neighbour_pairs_host(m, 4)
    for args in ((table['area'], pairs), (table, np.zeros(2, np.int32)), (table[None], pairs), (table, pairs[None])):
        with pytest.raises(TypeError):
            neighbours.derive(*args)
    with pytest.raises(ValueError, match='rows of the label table'):
        neighbours.derive(table[:6], pairs)
    with pytest.raises(TypeError):
        neighbours.adjacency(np.zeros(2, np.int32), 4)
    with pytest.raises(ValueError, match='labels 0 .. 5'):
        neighbours.adjacency(pairs, 6)
    with pytest.raises(TypeError, match='max_d2'):
        neighbours.neighbours_results([])                    # (max_d2 has no default)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_records_and_limit_mirror_the_header():
    from superdsm_amd import _capi, neighbours
    text = open(os.path.join(ROOT, 'include', 'sdsm.h')).read()
    assert int(re.search(r'#define SDSM_NEIGHBOUR_MAX_D2 (\d+)', text).group(1)) == _capi.NEIGHBOUR_MAX_D2 == neighbours.MAX_D2 == 4096
    for name, dtype in (('sdsm_neighbour_label', _capi.NEIGHBOUR_LABEL_DTYPE), ('sdsm_neighbour_pair', _capi.NEIGHBOUR_PAIR_DTYPE)):
        body, size = re.search(r'typedef struct \{([^}]*)\} ' + name + r';\s*/\* (\d+) bytes', text).groups()
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        fields = [(n.strip(), {'int64_t': '<i8', 'int32_t': '<i4'}[t]) for t, names in re.findall(r'(int64_t|int32_t) ([^;]+);', body) for n in names.split(',')]
        assert np.dtype(fields) == dtype and dtype.itemsize == int(size)
    inline = open(os.path.join(ROOT, 'superdsm_amd', 'csrc', 'sdsm_neighbours.h')).read()
    assert int(re.search(r'#define SDSM_NEIGHBOUR_MAX_D2_INLINE (\d+)', inline).group(1)) == 4096


def test_the_helpers_through_their_exported_symbols():
    from superdsm_amd import _capi
    L = _capi.lib()
    for max_d2 in (1, 2, 3, 4, 4095, 4096):
        R = math.isqrt(max_d2)
        for d_row in range(-R - 2, R + 3):
            want = math.isqrt(max_d2 - d_row * d_row) if d_row * d_row <= max_d2 else -1
            assert L.sdsm_neighbour_halfwidth(max_d2, d_row) == want, (max_d2, d_row)
    assert [L.sdsm_neighbour_halfwidth(*a) for a in ((0, 0), (-5, 0), (4097, 0), (4096, 65), (4096, -2 ** 31), (2 ** 31 - 1, 1))] == [-1] * 6
    key = (7 << 32) | 9
    h = (key * 0x9E3779B97F4A7C15) % 2 ** 64
    for bits in (0, 1, 12, 14, 40):
        assert L.sdsm_neighbour_slot(key, 1 << bits) == (h ^ (h >> 31)) & ((1 << bits) - 1)
    assert [L.sdsm_neighbour_slot(key, c) for c in (0, -1, 3, 6, -2 ** 63)] == [-1] * 5
    slots = {L.sdsm_neighbour_slot((a << 32) | b, 1 << 14) for a in range(1, 40) for b in range(a + 1, 41)}
    assert len(slots) > 0.95 * 39 * 40 / 2                   # 780 keys of small labels spread over 16 384 slots


def test_entry_points_refuse_bad_arguments_with_text():
    from superdsm_amd import _capi
    L = _capi.lib()
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    single = lambda H=8, W=8, lab=p, max_d2=2, n_labels=4, rec=p, cap=4, keys=p, mn=p, ct=p, st=p: L.sdsm_neighbours(H, W, lab, max_d2, n_labels, rec, cap, keys, mn, ct, st, None)
    for kw, text in ((dict(max_d2=0), b'max_d2'), (dict(max_d2=4097), b'max_d2'), (dict(max_d2=-3), b'max_d2'), (dict(H=0), b'bad image table'),
                     (dict(H=40000, W=40000), b'H * H + W * W < 2^31'), (dict(lab=None), b'null'), (dict(rec=None), b'null'), (dict(keys=None), b'null'),
                     (dict(mn=None), b'null'), (dict(ct=None), b'null'), (dict(st=None), b'null'), (dict(n_labels=0), b'n_labels'),
                     (dict(n_labels=65537), b'n_labels'), (dict(cap=0), b'capacity'), (dict(cap=6), b'capacity')):
        assert single(**kw) != 0 and text in L.sdsm_last_error(), (kw, L.sdsm_last_error())
    i64, i32 = lambda *v: (C.c_int64 * len(v))(*v), lambda *v: (C.c_int32 * len(v))(*v)
    table = (_capi.SetImage * 33)(*[_capi.SetImage(0, 2, 2)] * 33)
    multi = lambda n, rec_off, n_labels, tab_off, cap, max_d2=2: L.sdsm_neighbours_multi(table, n, p, max_d2, rec_off, n_labels, p, tab_off, cap, p, p, p, p, None)
    for args, text in (((0, i64(0), i32(2), i64(0), i64(4)), b'1 .. 32 images'), ((33, i64(*[0] * 33), i32(*[2] * 33), i64(*[0] * 33), i64(*[4] * 33)), b'1 .. 32 images'),
                       ((2, None, i32(2, 2), i64(0, 4), i64(4, 4)), b'null'), ((2, i64(0, 2), None, i64(0, 4), i64(4, 4)), b'null'),
                       ((2, i64(0, 2), i32(2, 2), None, i64(4, 4)), b'null'), ((2, i64(0, 2), i32(2, 2), i64(0, 4), None), b'null'),
                       ((2, i64(0, 1), i32(2, 2), i64(0, 4), i64(4, 4)), b'records of two images overlap'), ((2, i64(0, -2), i32(2, 2), i64(0, 4), i64(4, 4)), b'rec_off'),
                       ((2, i64(0, 2), i32(2, 2), i64(0, 3), i64(4, 4)), b'tables of two images overlap'), ((2, i64(0, 2), i32(2, 2), i64(0, -4), i64(4, 4)), b'table_off'),
                       ((2, i64(0, 2), i32(2, 2), i64(0, 4), i64(4, 4), 5000), b'max_d2')):
        assert multi(*args) != 0 and text in L.sdsm_last_error(), (args[0], L.sdsm_last_error())


# ---- the orchestration of the GPU form, over a host restatement of the launch ----------------------------------------------------------------
def host_launch(l32, max_d2, n_labels, capacities, names):
    """What ``neighbours._launch_set`` returns, from the host definitions: the pairs in an open-addressing table of the given capacity,
    probed linearly from ``sdsm_neighbour_slot``; a pair without a slot is counted in status[1] and dropped."""
    from superdsm_amd import _capi, neighbours
    L = _capi.lib()
    out = []
    skipped = [int(((lab < 0) | (lab >= n_lab)).sum()) for lab, n_lab in zip(l32, n_labels)]
    if any(skipped):
        raise ValueError(f'{sum(skipped)} pixels of images {[i for i, n in zip(names, skipped) if n]} carry a label outside 0 .. n_labels - 1')
    for lab, n_lab, cap in zip(l32, n_labels, capacities):
        status = np.zeros(2, np.int32)
        keys, values = np.full(cap, 2 ** 64 - 1, np.uint64), np.stack([np.full(cap, -1, np.int32), np.zeros(cap, np.int32)], axis=1)
        for a, b, d2, n in neighbours.neighbour_pairs_host(lab, max_d2).tolist():
            key = (a << 32) | b
            s = L.sdsm_neighbour_slot(key, cap)
            for _ in range(cap):
                if keys[s] == 2 ** 64 - 1:
                    keys[s], values[s] = key, (d2, n)
                    break
                s = (s + 1) % cap
            else:
                status[1] += 1
        out.append((neighbours.neighbour_labels_host(lab, max_d2, n_lab), keys, values, status))
    return out


def test_tables_many_grows_splits_and_names(monkeypatch):
    from superdsm_amd import neighbours
    monkeypatch.setattr(neighbours, '_launch_set', host_launch)
    rng = np.random.default_rng(3)
    block = np.arange(1, 65, dtype=np.int64).reshape(8, 8)
    want = (neighbours.neighbour_labels_host(block, 8), neighbours.neighbour_pairs_host(block, 8))
    assert len(want[1]) > 500
    for capacity in (1, 64, None):
        info = {}
        table, pairs = neighbours.neighbour_tables(block, 8, capacity=capacity, info=info)
        assert table.tobytes() == want[0].tobytes() and pairs.tobytes() == want[1].tobytes() and pairs.dtype == neighbours.PAIR_DTYPE
        assert info['capacity'] == [max(2048, neighbours.DEFAULT_CAPACITY if capacity is None else 0)]     # at most half full: 2 * pairs <= capacity
    maps = [np.kron(rng.integers(0, 4, (3 + k % 3, 4)), np.ones((2, 2), np.int64)).astype([np.uint8, np.int32, np.int64][k % 3]) for k in range(33)]
    maps[7] = np.zeros((0, 3), np.int32)                     # an empty image: empty tables, no launch
    info = {}
    got = neighbours.neighbour_tables_many(maps, 5, capacity=2, info=info)
    assert len(got) == 33 and len(info['capacity']) == 33 and info['capacity'][7] == 2
    for m, (table, pairs) in zip(maps, got):
        assert table.tobytes() == neighbours.neighbour_labels_host(m, 5).tobytes() and pairs.tobytes() == neighbours.neighbour_pairs_host(m, 5).tobytes()
    fixed = neighbours.neighbour_tables_many(maps[:3], 5, n_labels=9)
    assert all(len(t) == 9 and t.tobytes() == neighbours.neighbour_labels_host(m, 5, 9).tobytes() for m, (t, _) in zip(maps, fixed))
    bad = maps[:3] + [np.array([[1, -1]])]
    with pytest.raises(ValueError, match=r'1 pixels of images \[3\]'):
        neighbours.neighbour_tables_many(bad, 5)
    with pytest.raises(ValueError, match=r'pixels of images \[0, 1, 2\]'):
        neighbours.neighbour_tables_many([np.full((2, 2), 3)] * 3, 5, n_labels=3)


# ---- the inline helpers alone under the sanitizers ------------------------------------------------------------------------------------------
def test_the_helpers_alone_under_the_sanitizers(tmp_path):
    """tests/host/neighbours_check.cpp, which includes csrc/sdsm_neighbours.h, as host code only with AddressSanitizer and
    UndefinedBehaviorSanitizer linked into the executable (as tests/test_texture_cpu.py builds its program).  No GPU; a failing compile
    fails the test.  Nothing is loaded into Python under a sanitizer."""
    prog = tmp_path / 'neighbours_check'
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    build = subprocess.run([hipcc, '-x', 'hip', '--offload-host-only', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                            '-o', str(prog), os.path.join(ROOT, 'tests', 'host', 'neighbours_check.cpp')], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(prog)], capture_output=True, text=True, timeout=120)
    assert (run.returncode, run.stderr) == (0, ''), (run.returncode, run.stderr)
    disk = lambda d2: sum(2 * math.isqrt(d2 - r * r) + 1 for r in range(-math.isqrt(d2), math.isqrt(d2) + 1))
    assert [int(line) for line in run.stdout.splitlines()] == [disk(d2) for d2 in (1, 2, 25, 400, 4096)] and disk(1) == 5 and disk(2) == 9
