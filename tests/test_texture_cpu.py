"""The texture tables of superdsm_amd/texture.py without a GPU: the ``*_host`` definitions against a brute force, the level rule at its
edges, ``derive`` against the same formulas in fractions and mpmath to the bounds its docstring states, the argument errors, and the two
inline helpers of csrc/sdsm_texture.h through their exported symbols and alone under the sanitizers."""
import csv
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from test_measure_cpu import Obj, ellipse, label_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = 5e-324
OFFSETS = [(0, 1), (1, 1), (1, 0), (1, -1), (-2, 3), (0, -5), (25, 0), (-3, -32)]    # negative ones, and larger than any fragment here


def brute(pixels, g, edges, offs):
    """Per offset the dict (i, j) -> count of the pixels (a set of (r, c)): a loop over pixels and offsets, the level by counting edges."""
    level = lambda v: sum(1 for e in edges if e <= v)
    tables = []
    for dr, dc in offs:
        t = {}
        for r, c in pixels:
            if (r + dr, c + dc) in pixels and math.isfinite(g[r, c]) and math.isfinite(g[r + dr, c + dc]):
                a, b = level(g[r, c]), level(g[r + dr, c + dc])
                t[min(a, b), max(a, b)] = t.get((min(a, b), max(a, b)), 0) + 1
        tables.append(t)
    return tables


def cells_of(res, k, o):
    p = res[1][k, o]
    e = res[2][int(p['first']):int(p['first']) + int(p['n_entries'])]
    return {(int(x['i']), int(x['j'])): int(x['count']) for x in e}


def check_against_brute(res, pixel_sets, g, edges, offs):
    from superdsm_amd import texture as tx
    table, pairs, entries = res
    assert table.dtype == tx.TABLE_DTYPE and pairs.dtype == tx.PAIRS_DTYPE and entries.dtype == tx.ENTRY_DTYPE
    assert pairs.shape == (len(pixel_sets), len(offs))
    assert pairs['first'].reshape(-1).tolist() == np.concatenate([[0], np.cumsum(pairs['n_entries'].reshape(-1))[:-1]]).tolist()
    assert len(entries) == pairs['n_entries'].sum()
    for k, pixels in enumerate(pixel_sets):
        for o, t in enumerate(brute(pixels, g, edges, offs)):
            assert cells_of(res, k, o) == t, (k, offs[o])
            assert pairs[k, o]['n_pairs'] == sum(t.values())
            keys = [(int(x['i']), int(x['j'])) for x in entries[int(pairs[k, o]['first']):int(pairs[k, o]['first']) + int(pairs[k, o]['n_entries'])]]
            assert keys == sorted(t)                                             # ascending (i, j), no zero cell
        vals = [g[p] for p in pixels if math.isfinite(g[p])]
        levels = [sum(1 for e in edges if e <= v) for v in vals]
        assert (table[k]['area'], table[k]['n_finite']) == (len(pixels), len(vals))
        assert (table[k]['level_min'], table[k]['level_max']) == ((min(levels), max(levels)) if vals else (len(edges) + 1, -1))


@pytest.mark.parametrize('G', [1, 2, 5, 256])
def test_objects_equal_a_brute_force(G):
    from superdsm_amd import texture as tx
    rng = np.random.default_rng(G)
    shape = (40, 44)
    g = rng.random(shape)
    g[rng.random(shape) < 0.03] = np.nan
    edges = tx.uniform_edges(0.0, 1.0, G)
    objs = [Obj((rng.integers(0, 20), rng.integers(0, 24)), rng.random((rng.integers(1, 21), rng.integers(1, 21))) < 0.7) for _ in range(5)]
    objs.append(Obj((0, 0), np.zeros((3, 4), bool)))
    pixel_sets = [{(int(r) + int(o.fg_offset[0]), int(c) + int(o.fg_offset[1])) for r, c in zip(*np.nonzero(o.fg_fragment))} for o in objs]
    res = tx.texture_objects_host(objs, shape, g, edges, OFFSETS)
    check_against_brute(res, pixel_sets, g, edges, OFFSETS)
    assert res[0]['flags'][-1] == tx.NO_FINITE_PIXEL and (res[1]['n_pairs'][-1] == 0).all()
    assert (res[1]['n_entries'][:, 6:] == 0).all()                                # (25, 0) and (-3, -32) reach past every fragment


@pytest.mark.parametrize('G', [1, 2, 5, 256])
def test_labels_equal_a_brute_force(G):
    from superdsm_amd import texture as tx
    rng = np.random.default_rng(10 + G)
    labels = label_scene(rng, shape=(36, 40), n=7)
    g = rng.normal(size=labels.shape)
    g[rng.random(labels.shape) < 0.03] = np.inf
    edges = tx.uniform_edges(-2.0, 2.0, G)
    res = tx.texture_labels_host(labels, g, edges, OFFSETS)
    ls = [l for l in range(1, 8) if (labels == l).any()]
    assert res[0]['label'].tolist() == ls
    check_against_brute(res, [{(int(r), int(c)) for r, c in zip(*np.nonzero(labels == l))} for l in ls], g, edges, OFFSETS)
    kept = tx.texture_labels_host(labels, g, edges, OFFSETS, keep_absent=True)
    assert kept[0]['label'].tolist() == list(range(8)) and kept[0]['area'][0] == 0 and kept[0]['level_min'][0] == G and kept[0]['level_max'][0] == -1
    assert kept[2].tobytes() == res[2].tobytes()
    for k, l in enumerate(ls):
        for o in range(len(OFFSETS)):
            assert cells_of(kept, l, o) == cells_of(res, k, o)


def test_a_full_rectangle_and_an_offset_against_its_negative():
    from superdsm_amd import texture as tx
    rng = np.random.default_rng(3)
    g = rng.random((30, 30))
    edges = tx.uniform_edges(0.0, 1.0, 6)
    for h, w in ((1, 1), (3, 7), (12, 5)):
        obj = [Obj((2, 3), np.ones((h, w), bool))]
        res = tx.texture_objects_host(obj, g.shape, g, edges, OFFSETS[:6])
        neg = tx.texture_objects_host(obj, g.shape, g, edges, [(-a, -b) for a, b in OFFSETS[:6]])
        for o, (dr, dc) in enumerate(OFFSETS[:6]):
            assert res[1][0, o]['n_pairs'] == max(0, h - abs(dr)) * max(0, w - abs(dc))
            assert sum(cells_of(res, 0, o).values()) == res[1][0, o]['n_pairs']
            assert cells_of(res, 0, o) == cells_of(neg, 0, o)
        assert neg[1].tobytes() == res[1].tobytes() and neg[2].tobytes() == res[2].tobytes()


# ---- the level rule ------------------------------------------------------------------------------------------------------------------
def test_values_on_below_and_above_an_edge_and_negative_zero():
    from superdsm_amd import texture as tx
    edges = np.array([-1.0, 0.0, 0.1, 2.0 ** 40])
    for k, e in enumerate(edges):
        below, above = np.nextafter(e, -np.inf), np.nextafter(e, np.inf)
        assert tx.levels_of([below, e, above], edges).tolist() == [k, k + 1, k + 1]
    assert tx.levels_of([-0.0, 0.0, -TINY], edges).tolist() == [2, 2, 1]          # -0.0 compares as 0.0
    sub = np.array([-TINY, 0.0, TINY, 3 * TINY])                                   # subnormal edges
    assert tx.levels_of([-2 * TINY, -TINY, -0.0, TINY, 2 * TINY, 3 * TINY, 1.0], sub).tolist() == [0, 1, 2, 3, 3, 4, 4]
    assert tx.levels_of([np.nan, np.inf, -np.inf, 5.0], []).tolist() == [-1, -1, -1, 0]
    g = np.array([[0.1, np.nextafter(0.1, 0), 0.1, -0.0]])
    res = tx.texture_objects_host([Obj((0, 0), np.ones((1, 4)))], g.shape, g, [0.0, 0.1], [(0, 1)])
    assert cells_of(res, 0, 0) == {(1, 2): 3} and (res[0]['level_min'][0], res[0]['level_max'][0]) == (1, 2)


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_a_non_finite_pixel_is_excluded_and_flagged_and_its_neighbours_lose_the_pair(bad):
    from superdsm_amd import texture as tx
    g = np.zeros((5, 5))
    g[2, 2] = bad
    res = tx.texture_objects_host([Obj((1, 1), np.ones((3, 3))), Obj((0, 0), np.ones((2, 2))), Obj((2, 2), np.ones((1, 1)))], g.shape, g, [], tx.DEFAULT_OFFSETS)
    assert res[0]['flags'].tolist() == [tx.NONFINITE_INSIDE, tx.FRAME, tx.NONFINITE_INSIDE | tx.NO_FINITE_PIXEL]
    assert res[0]['n_finite'].tolist() == [8, 4, 0] and res[0]['area'].tolist() == [9, 4, 1]
    assert res[1]['n_pairs'][0].tolist() == [4, 2, 4, 2]                         # of 6, 4, 6, 4: every pair through the centre is lost
    assert (res[0]['level_min'][2], res[0]['level_max'][2]) == (1, -1) and (res[1]['n_pairs'][2] == 0).all()


def test_uniform_edges_and_a_range_too_narrow():
    from superdsm_amd import texture as tx
    e = tx.uniform_edges(-1.0, 3.0, 8)
    assert e.tolist() == (-1.0 + 4.0 * (np.arange(1, 8) / 8)).tolist() and len(tx.uniform_edges(0, 1, 1)) == 0
    assert len(tx.uniform_edges(0.0, 1.0, 256)) == 255
    for lo, hi, levels in ((1.0, 1.0, 3), (1.0, np.nextafter(1.0, 2), 4), (0.0, 100 * TINY, 256), (2.0, 1.0, 3), (0.0, np.inf, 2), (np.nan, 1.0, 2)):
        with pytest.raises(ValueError, match='narrow'):
            tx.uniform_edges(lo, hi, levels)
    with pytest.raises(ValueError):
        tx.uniform_edges(0, 1, 257)
    img = np.array([[np.nan, 2.0], [6.0, -np.inf]])
    assert tx.image_edges(img, 4).tolist() == [3.0, 4.0, 5.0] and len(tx.image_edges(np.full((2, 2), np.nan), 1)) == 0
    assert tx.uniform_edges(1.0, 1.0, 2).tolist() == [1.0] and tx.image_edges(np.full((2, 2), 7.0), 2).tolist() == [7.0]    # one edge is increasing
    with pytest.raises(ValueError):
        tx.image_edges(np.full((2, 2), 7.0), 3)
    with pytest.raises(ValueError):
        tx.image_edges(np.full((2, 2), np.nan), 2)


# ---- derive ----------------------------------------------------------------------------------------------------------------------------
def test_checkerboard_stripes_and_a_constant_object():
    from superdsm_amd import texture as tx
    one = [Obj((0, 0), np.ones((8, 8)))]
    board = (np.indices((8, 8)).sum(0) % 2).astype(float)
    d = tx.derive(*tx.texture_objects_host(one, (8, 8), board, [0.5], [(0, 1)]), offsets=[(0, 1)])[0, 0]
    assert (d['contrast'], d['correlation'], d['asm'], d['entropy'], d['n_pairs']) == (1.0, -1.0, 0.5, 1.0, 56)
    assert (d['dissimilarity'], d['idm'], d['sum_average'], d['sum_variance'], d['difference_entropy'], d['imc1']) == (1.0, 0.5, 1.0, 0.0, 0.0, -1.0)
    stripes = np.repeat((np.arange(8) % 2).astype(float)[:, None], 8, axis=1)      # horizontal stripes: rows alternate
    offs = [(0, 1), (1, 0)]
    d = tx.derive(*tx.texture_objects_host(one, (8, 8), stripes, [0.5], offs), offsets=offs)[0]
    assert (d['contrast'][0], d['correlation'][0], d['asm'][0], d['entropy'][0], d['idm'][0]) == (0.0, 1.0, 0.5, 1.0, 1.0)   # along a stripe: P = diag(N, N)
    assert (d['contrast'][1], d['correlation'][1], d['asm'][1], d['entropy'][1]) == (1.0, -1.0, 0.5, 1.0)                   # across: the checkerboard's table
    assert d['d_row'].tolist() == [0, 1] and d['d_col'].tolist() == [1, 0]
    flat = np.full((8, 8), 3.25)
    d = tx.derive(*tx.texture_objects_host(one, (8, 8), flat, [1.0, 2.0, 5.0], [(1, 1)]))[0, 0]
    assert (d['entropy'], d['asm'], d['contrast'], d['variance'], d['imc2'], d['mean'], d['sum_entropy']) == (0.0, 1.0, 0.0, 0.0, 0.0, 2.0, 0.0)
    assert math.isnan(d['correlation']) and math.isnan(d['imc1']) and not math.copysign(1, d['entropy']) < 0
    assert d['on_boundary'] and not d['nonfinite_inside']


def test_a_row_without_pairs_reads_nan_throughout():
    from superdsm_amd import texture as tx
    g = np.zeros((6, 6))
    g[4, 4] = np.nan
    objs = [Obj((1, 1), np.ones((1, 1))), Obj((4, 4), np.ones((1, 1))), Obj((2, 2), np.zeros((2, 2))), Obj((1, 1), np.ones((2, 2)))]
    res = tx.texture_objects_host(objs, g.shape, g, [], [(0, 1), (3, 0)])
    d = tx.derive(*res)
    for f in tx.FEATURES:
        assert np.isnan(d[f][:3]).all() and np.isnan(d[f][3, 1])
        assert np.isnan(d[f][3, 0]) == (f in ('correlation', 'imc1'))             # a constant object with two pairs
    assert d['no_finite_pixel'][:, 0].tolist() == [False, True, True, False] and d['n_pairs'].tolist() == [[0, 0], [0, 0], [0, 0], [2, 0]]
    assert tx.derive(*tx.texture_objects_host([], g.shape, g, [], [(0, 1)])).shape == (0, 1)


def _reference_features(P):
    """The features of the symmetric integer matrix P by their printed formulas: rationals as fractions, entropies in mpmath."""
    G, tot = len(P), int(P.sum())
    p = [[Fraction(int(P[a, b]), tot) for b in range(G)] for a in range(G)]
    px = [sum(row) for row in p]
    mu = sum(a * px[a] for a in range(G))
    var = sum((a - mu) ** 2 * px[a] for a in range(G))
    ps, pd = {}, {}
    for a in range(G):
        for b in range(G):
            ps[a + b] = ps.get(a + b, 0) + p[a][b]
            pd[abs(a - b)] = pd.get(abs(a - b), 0) + p[a][b]
    mp = lambda f: mpmath.mpf(f.numerator) / mpmath.mpf(f.denominator)
    H = lambda qs: -sum(mp(q) * mpmath.log(mp(q), 2) for q in qs if q > 0)
    f6 = sum(k * q for k, q in ps.items())
    cells = [(a, b) for a in range(G) for b in range(G) if p[a][b] > 0]
    R = dict(asm=sum(q * q for row in p for q in row), contrast=sum((a - b) ** 2 * p[a][b] for a, b in cells),
             correlation=(sum(a * b * p[a][b] for a, b in cells) - mu * mu) / var if var else None, variance=var,
             idm=sum(p[a][b] / (1 + (a - b) ** 2) for a, b in cells), sum_average=f6, sum_variance=sum((k - f6) ** 2 * q for k, q in ps.items()),
             difference_variance=sum(k * k * q for k, q in pd.items()) - sum(k * q for k, q in pd.items()) ** 2,
             dissimilarity=sum(abs(a - b) * p[a][b] for a, b in cells), mean=mu)
    HXY, HX = H([p[a][b] for a, b in cells]), H(px)
    HXY1 = -sum(mp(p[a][b]) * mpmath.log(mp(px[a]) * mp(px[b]), 2) for a, b in cells)
    HXY2 = -sum(mp(px[a]) * mp(px[b]) * mpmath.log(mp(px[a]) * mp(px[b]), 2) for a in range(G) for b in range(G) if px[a] > 0 and px[b] > 0)
    E = dict(entropy=HXY, sum_entropy=H(ps.values()), difference_entropy=H(pd.values()), HX=HX, imc1=(HXY - HXY1) / HX if HX > 0 else None,
             imc2=mpmath.sqrt(max(0, 1 - mpmath.power(2, -2 * (HXY2 - HXY)))), energy=mpmath.sqrt(mp(R['asm'])))
    return R, E


def _objects_for_derive(seed=77):
    rng = np.random.default_rng(seed)
    shape = (48, 48)
    g = rng.random(shape) + np.linspace(0, 1, 48)[:, None] * rng.random()
    objs = [Obj((rng.integers(0, 20), rng.integers(0, 20)), ellipse(rng, 11)) for _ in range(10)]
    return objs, shape, g


@pytest.mark.parametrize('G', [2, 3, 8, 32])
def test_every_column_is_within_its_stated_bound_of_fractions_and_mpmath(G):
    """Ten random objects at four offsets per level count, other objects for every count: forty objects, forty rows each.  The rational columns within 0.5 ulp (they are correctly
    rounded quotients), energy within 1 ulp, idm within 260 * 2^-53 relative, the entropies within entropy_bound(m, H), imc1 and imc2
    within the bounds that the docstring of derive composes from those."""
    from superdsm_amd import texture as tx
    objs, shape, g = _objects_for_derive(100 + G)
    res = tx.texture_objects_host(objs, shape, g, tx.image_edges(g, G))
    d = tx.derive(*res, offsets=tx.DEFAULT_OFFSETS)
    m_xy, m_s, m_d, m_x = tx.entropy_terms(res[1], res[2])
    mpf = lambda x: mpmath.mpf(float(x))
    rows = 0
    for k, o in ((k, o) for k in range(len(objs)) for o in range(4) if res[1][k, o]['n_pairs'] > 0):
        with mpmath.workprec(200):
            rows += 1
            R, E = _reference_features(tx.dense(res[1][k, o], res[2], G))
            for f, exact in R.items():
                got = float(d[f][k, o])
                if exact is None:
                    assert math.isnan(got), f
                elif f != 'idm':                                                  # (a float sum: its own bound below)
                    assert abs(Fraction(got) - exact) <= Fraction(math.ulp(got)) / 2, (f, k, o, got, float(exact))
            assert abs(mpf(d['energy'][k, o]) - E['energy']) <= math.ulp(d['energy'][k, o])
            assert abs(Fraction(float(d['idm'][k, o])) - R['idm']) <= 260 * Fraction(2) ** -53 * R['idm']
            e_xy, e_x = tx.entropy_bound(m_xy[k, o], float(E['entropy'])), tx.entropy_bound(m_x[k, o], float(E['HX']))
            assert abs(mpf(d['entropy'][k, o]) - E['entropy']) <= e_xy
            assert abs(mpf(d['sum_entropy'][k, o]) - E['sum_entropy']) <= tx.entropy_bound(m_s[k, o], float(E['sum_entropy']))
            assert abs(mpf(d['difference_entropy'][k, o]) - E['difference_entropy']) <= tx.entropy_bound(m_d[k, o], float(E['difference_entropy']))
            if E['imc1'] is None:
                assert math.isnan(d['imc1'][k, o])
            else:
                assert abs(mpf(d['imc1'][k, o]) - E['imc1']) <= 1.01 * (e_xy + 3 * e_x) / float(E['HX']) + 2.0 ** -51
            assert abs(mpf(d['imc2'][k, o]) - E['imc2']) <= math.sqrt(1.4 * (e_xy + 2 * e_x) + 2.0 ** -48) + 2.0 ** -52
    assert rows >= 36


def test_pooled_equals_the_integer_sum_of_dense_over_the_offsets():
    from superdsm_amd import texture as tx
    objs, shape, g = _objects_for_derive()
    objs.append(Obj((0, 0), np.zeros((2, 2))))
    res = tx.texture_objects_host(objs, shape, g, tx.image_edges(g, 16), OFFSETS)
    pp, pe = tx.pooled(res[1], res[2])
    assert pp.shape == (len(objs), 1) and pe.dtype == tx.POOLED_ENTRY_DTYPE and len(pe) == pp['n_entries'].sum()
    for k in range(len(objs)):
        total = sum(tx.dense(res[1][k, o], res[2], 16) for o in range(len(OFFSETS)))
        assert (tx.dense(pp[k, 0], pe, 16) == total).all() and pp[k, 0]['n_pairs'] == res[1]['n_pairs'][k].sum() and 2 * pp[k, 0]['n_pairs'] == total.sum()
        e = pe[int(pp[k, 0]['first']):int(pp[k, 0]['first']) + int(pp[k, 0]['n_entries'])]
        keys = [(int(x['i']), int(x['j'])) for x in e]
        assert keys == sorted(set(keys)) and (e['count'] > 0).all()
    d = tx.derive(res[0], pp, pe)
    assert d.shape == (len(objs), 1) and np.isnan(d['asm'][-1, 0]) and not np.isnan(d['asm'][:-1]).any()


def test_csv_round_trip(tmp_path):
    from superdsm_amd import texture as tx
    objs, shape, g = _objects_for_derive()
    res = tx.texture_objects_host(objs[:3] + [Obj((0, 0), np.zeros((2, 2)))], shape, g, tx.image_edges(g, 8))
    path = tmp_path / 'texture.csv'
    tx.write_texture_csv(path, *res, offsets=tx.DEFAULT_OFFSETS)
    rows = list(csv.reader(open(path)))
    d = tx.derive(*res, offsets=tx.DEFAULT_OFFSETS)
    assert rows[0] == list(tx.DERIVED_DTYPE.names) + ['level_min', 'level_max', 'n_entries', 'cells'] and len(rows) == 1 + 4 * 4
    for line, row in enumerate(rows[1:]):
        k, o = divmod(line, 4)
        rec = dict(zip(rows[0], row))
        assert (int(rec['label']), int(rec['d_row']), int(rec['d_col'])) == (k,) + tx.DEFAULT_OFFSETS[o]
        assert (int(rec['area']), int(rec['n_finite']), int(rec['n_pairs']), int(rec['level_min']), int(rec['level_max']), int(rec['n_entries'])) == \
               (res[0][k]['area'], res[0][k]['n_finite'], res[1][k, o]['n_pairs'], res[0][k]['level_min'], res[0][k]['level_max'], res[1][k, o]['n_entries'])
        cells = {(int(a), int(b)): int(c) for a, b, c in (cell.split(':') for cell in rec['cells'].split())}
        assert cells == cells_of(res, k, o) and list(cells) == sorted(cells)
        for f in tx.FEATURES:
            assert float(rec[f]) == d[f][k, o] or (math.isnan(float(rec[f])) and math.isnan(d[f][k, o]))
    assert dict(zip(rows[0], rows[-1]))['asm'] == 'nan' and dict(zip(rows[0], rows[-1]))['cells'] == ''


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from superdsm_amd import texture as tx
    g = np.zeros((4, 4))
    one = [Obj((0, 0), np.ones((2, 2)))]
    lab = np.zeros((4, 4), int)
    for host in (lambda e, o: tx.texture_objects_host(one, (4, 4), g, e, o), lambda e, o: tx.texture_labels_host(lab, g, e, o),
                 lambda e, o: tx.texture_objects_many([one], [(4, 4)], [g], [e], o), lambda e, o: tx.texture_labels_many([lab], [g], [e], o)):
        with pytest.raises(ValueError, match='levels'):
            host(np.arange(256.0), [(0, 1)])                                       # G = 257
        for bad in ([1.0, 0.5], [0.0, 0.0], [0.0, np.nan], [np.inf], [[0.0, 1.0]]):
            with pytest.raises(ValueError, match='edges'):
                host(bad, [(0, 1)])
        for bad in ([(0, 0)], [(33, 0)], [(0, -33)], [(0, 1)] * 2, [(1, 2), (-1, -2)], [(k, 1) for k in range(9)], [], [(0.5, 1)], [(1, 2, 3)]):
            with pytest.raises(ValueError, match='offset'):
                host([0.5], bad)
    assert len(tx.check_offsets([(32, -32)] + [(k, 1) for k in range(7)])) == 8 and len(tx.check_edges(np.arange(255.0))) == 255
    with pytest.raises(ValueError, match='same length'):
        tx.texture_objects_many([one, one], [(4, 4)] * 2, [g, g], [[0.5], [0.2, 0.7]])
    with pytest.raises(ValueError, match='one list per image'):
        tx.texture_labels_many([lab, lab], [g, g], [[0.5]])
    with pytest.raises(ValueError, match='intensity'):
        tx.texture_objects_host(one, (4, 4), None, [0.5])
    with pytest.raises(ValueError):
        tx.texture_objects_host(one, (4, 4), np.zeros((4, 5)), [0.5])
    with pytest.raises(ValueError):
        tx.texture_objects_host([Obj((3, 3), np.ones((2, 2)))], (4, 4), g, [0.5])      # the box leaves the image
    with pytest.raises(ValueError):
        tx.texture_objects_many([[Obj((3, 3), np.ones((2, 2)))]], [(4, 4)], [g], [[0.5]])
    with pytest.raises(ValueError):
        tx.texture_objects_host(one, (65536, 1), g, [0.5])
    for many in (tx.texture_labels_host, tx.texture_labels):
        with pytest.raises(TypeError):
            many(np.zeros((4, 4)), g, [0.5])                                       # labels that are no integers
        with pytest.raises(TypeError):
            many(np.zeros((4, 4, 2), int), g, [0.5])
    with pytest.raises(ValueError, match='labels'):
        tx.texture_labels_host(np.array([[0, 65536]]), np.zeros((1, 2)), [0.5])
    with pytest.raises(ValueError, match='labels'):
        tx.texture_labels_host(np.array([[0, -1]]), np.zeros((1, 2)), [0.5])
    res = tx.texture_objects_host(one, (4, 4), g, [0.5])
    with pytest.raises(ValueError):
        tx.derive(res[0], res[1][:, :2], res[2])
    with pytest.raises(ValueError):
        tx.derive(res[0], res[1], res[2], offsets=[(0, 1)])


# ---- the C side ----------------------------------------------------------------------------------------------------------------------------
def test_record_layouts_and_limits_are_those_of_the_header():
    from superdsm_amd import _capi, texture as tx
    text = open(os.path.join(ROOT, 'include', 'sdsm.h')).read()
    kinds = {'int64_t': 'i8', 'uint64_t': 'u8', 'int32_t': 'i4', 'uint32_t': 'u4', 'uint16_t': 'u2', 'double': 'f8'}
    for struct, dtype, size in (('record', _capi.TEXTURE_RECORD_DTYPE, 32), ('pairs', _capi.TEXTURE_PAIRS_DTYPE, 24), ('entry', _capi.TEXTURE_ENTRY_DTYPE, 8)):
        body = re.search(r'typedef struct \{([^}]*)\} sdsm_texture_' + struct + ';', text).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        declared = []
        for ctype, names in re.findall(r'(uint64_t|int64_t|uint32_t|int32_t|uint16_t|double)\s+([^;]+);', body):
            declared += [(n.strip(), kinds[ctype]) for n in names.split(',')]
        assert declared == [(n, dtype[n].str[1:]) for n in dtype.names] and dtype.itemsize == size
        offset = 0
        for n in dtype.names:                                                     # no padding: the C layout is the packed one
            assert dtype.fields[n][1] == offset
            offset += dtype[n].itemsize
    assert tx.TABLE_DTYPE.names[1:] == _capi.TEXTURE_RECORD_DTYPE.names
    for name, value in (('MAX_LEVELS', _capi.TEXTURE_MAX_LEVELS), ('MAX_OFFSETS', _capi.TEXTURE_MAX_OFFSETS), ('MAX_REACH', _capi.TEXTURE_MAX_REACH)):
        assert int(re.search(rf'#define SDSM_TEXTURE_{name} (\d+)', text).group(1)) == value
    assert (_capi.TEXTURE_MAX_LEVELS, _capi.TEXTURE_MAX_OFFSETS, _capi.TEXTURE_MAX_REACH) == (256, 8, 32)
    assert int(re.search(r'#define SDSM_TEXTURE_MAX_SLOTS \(1ll << (\d+)\)', text).group(1)) == int(math.log2(_capi.TEXTURE_MAX_SLOTS))


def _level_cases():
    rng = np.random.default_rng(5)
    edges = np.sort(np.concatenate([[-TINY, 0.0, TINY], rng.normal(size=252) * 10.0 ** rng.integers(-300, 300, 252)]))
    assert len(edges) == 255 and (edges[1:] > edges[:-1]).all()
    values = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), [-0.0, 1e308, -1e308], rng.normal(size=50)])
    return edges, values


def test_the_two_inline_helpers_through_their_exported_symbols():
    from superdsm_amd import _capi, texture as tx
    L = _capi.lib()
    edges, values = _level_cases()
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for n_edges in (0, 1, 2, 255):
        e = np.ascontiguousarray(edges[:n_edges])
        got = [L.sdsm_texture_level(ptr(e) if n_edges else None, n_edges, float(v)) for v in values]
        assert got == np.searchsorted(e, values, side='right').tolist() == tx.levels_of(values, e).tolist()
    e = np.array([1.0])
    assert [L.sdsm_texture_level(ptr(e), 1, v) for v in (np.nan, np.inf, -np.inf)] == [-1] * 3
    assert L.sdsm_texture_level(ptr(e), -1, 0.0) == L.sdsm_texture_level(ptr(e), 256, 0.0) == L.sdsm_texture_level(None, 1, 0.0) == -1
    for G in (1, 2, 256):
        place = 0
        for i in range(G):
            for j in range(i, G):
                assert L.sdsm_texture_cell(G, i, j) == place == i * G - i * (i - 1) // 2 + (j - i)
                place += 1
        assert place == G * (G + 1) // 2
        assert L.sdsm_texture_cell(G, 0, G) == L.sdsm_texture_cell(G, -1, 0) == -1 and (G == 1 or L.sdsm_texture_cell(G, 1, 0) == -1)
    assert L.sdsm_texture_cell(0, 0, 0) == L.sdsm_texture_cell(257, 0, 0) == -1


def test_the_entry_points_refuse_bad_arguments_with_text():
    from superdsm_amd import _capi
    L = _capi.lib()
    one = (C.c_int32 * 2)(0, 1)
    call = lambda n, levels, n_o, offs: L.sdsm_texture_objects(8, 8, n, None, None, None, None, levels, None, n_o, offs, None, None, None, None, None, None)
    for args, text in (((-1, 2, 1, one), b'n <='), ((1, 0, 1, one), b'levels'), ((1, 257, 1, one), b'levels'), ((1, 2, 0, one), b'offsets'),
                       ((1, 2, 9, one), b'offsets'), ((1, 2, 1, None), b'offsets'), ((1, 2, 1, (C.c_int32 * 2)(0, 0)), b'offsets'),
                       ((1, 2, 1, (C.c_int32 * 2)(33, 0)), b'offsets'), ((1, 2, 2, (C.c_int32 * 4)(1, 2, -1, -2)), b'offsets'),
                       ((1, 2, 2, (C.c_int32 * 4)(1, 2, 1, 2)), b'offsets'), ((1, 2, 1, one), b'null')):
        assert call(*args) != 0 and text in L.sdsm_last_error(), (args, L.sdsm_last_error())
    assert call(0, 2, 1, one) == 0                                            # no objects: no launch


def test_the_helpers_alone_under_the_sanitizers(tmp_path):
    """tests/host/texture_check.cpp with sdsm_host.cpp as host code only, AddressSanitizer and UndefinedBehaviorSanitizer linked into the
    executable (as tests/test_intensity_cpu.py builds its program).  No GPU; a failing compile fails the test."""
    edges, values = _level_cases()
    (tmp_path / 'cases.txt').write_text(f'{len(edges)}\n' + ''.join(float(v).hex() + '\n' for v in np.concatenate([edges, values])))
    prog = tmp_path / 'texture_check'
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    build = subprocess.run([hipcc, '-x', 'hip', '--offload-host-only', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                            '-o', str(prog),
                            os.path.join(ROOT, 'tests', 'host', 'texture_check.cpp'), os.path.join(ROOT, 'superdsm_amd', 'csrc', 'sdsm_host.cpp')],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(prog), str(tmp_path / 'cases.txt')], capture_output=True, text=True, timeout=120)
    assert (run.returncode, run.stderr) == (0, ''), run.stderr
    assert [int(line) for line in run.stdout.splitlines()] == np.searchsorted(edges, values, side='right').tolist()
    (tmp_path / 'none.txt').write_text('0\n' + ''.join(float(v).hex() + '\n' for v in values[:5]))
    run = subprocess.run([str(prog), str(tmp_path / 'none.txt')], capture_output=True, text=True, timeout=120)
    assert (run.returncode, run.stderr, run.stdout) == (0, '', '0\n' * 5)
