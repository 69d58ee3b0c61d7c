"""The host definitions of the connected parts (superdsm_amd/parts.py) against a breadth-first search written here and against
scipy.ndimage.label, the bit-quad identity against directly counted holes, the selections, the argument checks, the host helper of the
C ABI through ctypes and alone under the sanitizers, and the CSV writer.  No GPU."""
import csv
import ctypes as C
import itertools
import os
import subprocess
from collections import deque

import numpy as np
import pytest
from scipy import ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEPS = {4: ((-1, 0), (0, -1), (0, 1), (1, 0)), 8: tuple((dr, dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1) if dr or dc)}
SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (13, 17), (33, 40), (40, 40))


def flood(same, start, seen, steps):
    """The places reachable from ``start`` over places where ``same`` holds, by breadth-first search; they are marked in ``seen``."""
    H, W = same.shape
    seen[start] = True
    queue, out = deque([start]), [start]
    while queue:
        r, c = queue.popleft()
        for dr, dc in steps:
            q = (r + dr, c + dc)
            if 0 <= q[0] < H and 0 <= q[1] < W and same[q] and not seen[q]:
                seen[q] = True
                queue.append(q)
                out.append(q)
    return out


def search(labels, connectivity):
    """(part map, part rows, label rows, holes per label) of a label map by breadth-first search in raster order."""
    H, W = labels.shape
    part_map, seen = np.zeros((H, W), np.int32), np.zeros((H, W), bool)
    parts = []
    for r, c in itertools.product(range(H), range(W)):
        if labels[r, c] and not seen[r, c]:
            px = np.array(flood(labels == labels[r, c], (r, c), seen, STEPS[connectivity]))
            part_map[px[:, 0], px[:, 1]] = len(parts) + 1
            parts.append(dict(label=int(labels[r, c]), area=len(px), first=r * W + c, r0=px[:, 0].min(), c0=px[:, 1].min(), r1=px[:, 0].max() + 1,
                              c1=px[:, 1].max() + 1))
    n_labels = int(labels.max()) + 1 if labels.size else 1
    rows = [dict(n_parts=0, area=0, largest_area=0, largest_part=0, q1=0, q3=0, qd=0) for _ in range(n_labels)]
    per_label = [0] * n_labels
    for k, p in enumerate(parts, 1):
        row = rows[p['label']]
        p['index_in_label'] = per_label[p['label']]
        per_label[p['label']] += 1
        row['n_parts'] += 1
        row['area'] += p['area']
        if p['area'] > row['largest_area']:
            row['largest_area'], row['largest_part'] = p['area'], k
    holes = [0] * n_labels
    for l in range(1, n_labels):
        if not rows[l]['n_parts']:
            continue
        M = np.pad(labels == l, 1)
        for i, j in itertools.product(range(H + 1), range(W + 1)):
            w = M[i:i + 2, j:j + 2]
            n = int(w.sum())
            rows[l]['q1'] += n == 1
            rows[l]['q3'] += n == 3
            rows[l]['qd'] += n == 2 and w[0, 0] == w[1, 1]
        seen_c, n_comp = np.zeros(M.shape, bool), 0
        for r, c in itertools.product(range(H + 2), range(W + 2)):
            if not M[r, c] and not seen_c[r, c]:
                flood(~M, (r, c), seen_c, STEPS[12 - connectivity])
                n_comp += 1
        holes[l] = n_comp - 1
    return part_map, parts, rows, holes


def random_maps():
    rng = np.random.default_rng(5)
    for shape, n, density in itertools.product(SHAPES, (1, 2, 3), (0.3, 0.5, 0.7)):
        yield np.where(rng.random(shape) < density, rng.integers(1, n + 1, shape), 0).astype(np.int32)


@pytest.fixture(scope='module')
def searched():
    """Every random map with its search results under both adjacencies, computed once."""
    return [(m, c, search(m, c)) for m in random_maps() for c in (4, 8)]


def rows_equal(table, rows, names):
    assert len(table) == len(rows)
    for k, (got, want) in enumerate(zip(table, rows)):
        assert {n: int(got[n]) for n in names} == {n: int(want[n]) for n in names}, k


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_parts_host_against_the_search(searched):
    from superdsm_amd import parts
    for m, connectivity, (want_map, want_parts, want_rows, _) in searched:
        part_map, table, labels = parts.parts_host(m, connectivity)
        assert part_map.dtype == np.int32 and part_map.shape == m.shape and np.array_equal(part_map, want_map)
        assert table.dtype == parts.PART_DTYPE and labels.dtype == parts.LABEL_DTYPE
        rows_equal(table, want_parts, ('label', 'area', 'first', 'r0', 'c0', 'r1', 'c1', 'index_in_label'))
        rows_equal(labels, want_rows, ('n_parts', 'area', 'largest_area', 'largest_part', 'q1', 'q3', 'qd'))
        assert not labels['reserved'].any() and labels[0].tobytes() == bytes(32)
        if m.max() <= 1:
            ref, k = ndi.label(m, parts.structure(connectivity))
            assert np.array_equal(part_map, ref) and len(table) == k


def test_holes_host_against_the_search(searched):
    from superdsm_amd import parts
    for m, connectivity, (_, _, _, want_holes) in searched:
        assert parts.holes_host(m, connectivity).tolist() == want_holes


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_quad_identity(searched):
    from superdsm_amd import parts
    for m, connectivity, (_, _, want_rows, want_holes) in searched:
        _, _, labels = parts.parts_host(m, connectivity)
        q1, q3, qd = (labels[n].astype(np.int64) for n in ('q1', 'q3', 'qd'))
        assert not ((q1 - q3 + 2 * qd) % 4).any() and not ((q1 - q3 - 2 * qd) % 4).any()
        d = parts.derive(labels, connectivity)
        assert d.dtype == parts.DERIVED_DTYPE and d['holes'].tolist() == want_holes
        assert d['euler'].tolist() == [r['n_parts'] - h for r, h in zip(want_rows, want_holes)]
        for row, want in zip(d, want_rows):
            assert (np.isnan(row['largest_fraction']) if want['area'] == 0 else row['largest_fraction'] == want['largest_area'] / want['area'])
    bad = np.zeros(2, parts.LABEL_DTYPE)
    bad['q1'][1] = 3
    with pytest.raises(ValueError, match='multiple of 4'):
        parts.derive(bad, 4)


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_selections(searched):
    from superdsm_amd import parts
    K = parts.Keep
    for m, connectivity, (want_map, want_parts, want_rows, _) in searched[::3]:
        split, largest, all_, big = parts.keep_maps_host(m, [K.split(), K.largest(), K.min_area(1), K.min_area(4)], connectivity)
        assert all(x.dtype == np.int32 and x.shape == m.shape for x in (split, largest, all_, big))
        assert np.array_equal(split, want_map) and np.array_equal(all_, m)
        is_largest = np.isin(want_map, [r['largest_part'] for r in want_rows if r['largest_part']])
        assert np.array_equal(largest, np.where(is_largest, m, 0))
        rest = np.where(is_largest, 0, m)
        assert np.array_equal(largest + rest, m) and not (largest.astype(bool) & rest.astype(bool)).any()
        areas = np.array([0] + [p['area'] for p in want_parts])
        assert np.array_equal(big, np.where(areas[want_map] >= 4, m, 0))


def test_of_two_parts_of_equal_area_the_first_wins():
    from superdsm_amd import parts
    m = np.array([[0, 3, 3, 0, 0], [0, 0, 0, 0, 7], [3, 3, 0, 0, 7], [0, 0, 0, 3, 0]])
    for connectivity in (4, 8):
        _, table, labels = parts.parts_host(m, connectivity)
        assert table['label'].tolist() == [3, 7, 3, 3] and table['index_in_label'].tolist() == [0, 0, 1, 2]
        assert (labels[3]['largest_part'], labels[3]['largest_area'], labels[3]['n_parts']) == (1, 2, 3) and labels[7]['largest_part'] == 2
        largest, = parts.keep_maps_host(m, parts.Keep.largest(), connectivity)
        assert np.array_equal(largest, np.where(np.arange(4)[:, None] < 1, m, 0) + np.where(m == 7, 7, 0))


def test_more_selections_than_a_call_takes():
    from superdsm_amd import parts
    K = parts.Keep
    m = np.ones((3, 3), np.int32)
    assert len(parts.keep_maps_host(m, [K.min_area(a) for a in range(1, 9)])) == 8
    with pytest.raises(ValueError, match='at most 8'):
        parts.keep_maps_host(m, [K.min_area(a) for a in range(1, 10)])
    with pytest.raises(ValueError, match='at most 8'):
        parts.keep_maps_many([m], [K.split()] * 9)           # (before any launch)
    with pytest.raises(TypeError):
        parts.keep_maps_host(m, ['largest'])
    assert K.min_area(3) == K.min_area(3) != K.min_area(4) and repr(K.min_area(3)) == 'Keep.min_area(3)' and K.split().spec() == (0, 0)


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    from superdsm_amd import parts
    ok = np.array([[1, 2, 0, 3]] * 3)
    with pytest.raises(TypeError, match='integer image'):
        parts.parts_host(ok.astype(float))
    with pytest.raises(TypeError, match='integer image'):
        parts.parts(ok.astype(np.float32))                   # (before any launch)
    for form in (parts.parts_host, parts.parts, parts.holes_host, parts.label_mask_host, parts.label_mask):
        for connectivity in (6, 0, '4', True, 4.0):
            with pytest.raises(ValueError, match='connectivity'):
                form(ok, connectivity)
    with pytest.raises(ValueError, match='connectivity'):
        parts.derive(np.zeros(1, parts.LABEL_DTYPE), 6)
    for v in (-1, 65536):
        bad = ok.copy()
        bad[1, 2] = v
        with pytest.raises(ValueError, match='labels'):
            parts.parts_host(bad)
        with pytest.raises(ValueError, match='labels'):
            parts.keep_maps_host(bad, [parts.Keep.split()])
    assert parts.parts_host(np.where(ok == 3, 65535, ok))[2]['n_parts'][65535] == 1
    for a in (0, -1, 2 ** 31):
        with pytest.raises(ValueError, match='min_area'):
            parts.Keep.min_area(a)
    for a in (1.0, True, '3'):
        with pytest.raises(TypeError, match='min_area'):
            parts.Keep.min_area(a)
    with pytest.raises(TypeError, match='mask'):
        parts.label_mask_host(ok.astype(float))
    with pytest.raises(TypeError, match='LABEL_DTYPE'):
        parts.derive(np.zeros(3, np.int32), 4)


def test_an_image_without_pixels():
    """Empty maps and tables in the host form and, with no launch (so without a GPU), in the GPU form."""
    from superdsm_amd import parts
    K = parts.Keep
    for shape in ((0, 5), (3, 0), (0, 0)):
        m = np.zeros(shape, np.int64)
        for form in (parts.parts_host, parts.parts, parts.label_mask_host, parts.label_mask):
            part_map, table, labels = form(m, 8)
            assert part_map.shape == shape and part_map.dtype == np.int32
            assert table.shape == (0,) and table.dtype == parts.PART_DTYPE and labels.dtype == parts.LABEL_DTYPE and labels.tobytes() == bytes(32)
        for form in (parts.keep_maps_host, parts.keep_maps):
            maps = form(m, [K.split(), K.largest(), K.min_area(2)])
            assert [x.shape for x in maps] == [shape] * 3 and all(x.dtype == np.int32 for x in maps)
        assert parts.holes_host(m).tolist() == [0]
    assert parts.parts_many([]) == [] and parts.keep_maps_many([], [K.split()]) == []


def test_a_mask_is_label_one():
    from superdsm_amd import parts
    rng = np.random.default_rng(9)
    mask = rng.random((17, 23)) < 0.5
    for connectivity in (4, 8):
        want, k = ndi.label(mask, parts.structure(connectivity))
        for given in (mask, mask.astype(np.uint8) * 200, np.where(mask, -3, 0)):
            part_map, table, labels = parts.label_mask_host(given, connectivity)
            assert np.array_equal(part_map, want) and len(table) == k and len(labels) == 2 and labels[1]['area'] == mask.sum()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_quad_helper_for_all_windows():
    from superdsm_amd import _capi
    quad = _capi.lib().sdsm_parts_quad
    for bits in itertools.product((0, 1), repeat=4):
        n = sum(bits)
        want = 1 if n == 1 else 2 if n == 3 else 3 if n == 2 and bits[0] == bits[3] else 0
        for label, other in ((1, 0), (65535, 1), (7, 65535)):
            window = [label if b else other for b in bits]
            assert quad(*window, label) == want, (window, label)
            assert quad(*window, 12345) == 0                 # a label that is absent: no class
        assert quad(*[9 if b else 0 for b in bits], 0) == (1 if n == 3 else 2 if n == 1 else 3 if n == 2 and bits[0] == bits[3] else 0)


def test_the_layouts_are_mirrored():
    from superdsm_amd import _capi, parts
    assert _capi.PART_DTYPE.itemsize == _capi.PART_LABEL_DTYPE.itemsize == 32 and _capi.KEEP_SPEC_DTYPE.itemsize == 8
    assert _capi.PART_DTYPE.names == ('label', 'area', 'first', 'r0', 'c0', 'r1', 'c1', 'index_in_label')
    assert _capi.PART_LABEL_DTYPE.names == ('n_parts', 'area', 'largest_area', 'largest_part', 'q1', 'q3', 'qd', 'reserved')
    header = open(os.path.join(ROOT, 'include', 'sdsm.h')).read()
    assert f'#define SDSM_PARTS_MAX_KEEPS {parts.MAX_KEEPS}\n' in header
    for name, value in (('SPLIT', _capi.KEEP_SPLIT), ('LARGEST', _capi.KEEP_LARGEST), ('MIN_AREA', _capi.KEEP_MIN_AREA)):
        assert f'#define SDSM_KEEP_{name} {value} ' in header


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_quad_helper_alone_under_the_sanitizers(tmp_path):
    """tests/host/parts_check.cpp with sdsm_host.cpp as host code only, AddressSanitizer and UndefinedBehaviorSanitizer linked into the
    executable (as tests/test_depth_cpu.py builds its program).  No GPU; a failing compile fails the test."""
    cases = [tuple(l if b else o for b in bits) + (l,) for bits in itertools.product((0, 1), repeat=4) for l, o in ((1, 0), (65535, 2), (3, 65535))]
    (tmp_path / 'cases.txt').write_text(''.join(' '.join(map(str, case)) + '\n' for case in cases))
    prog = tmp_path / 'parts_check'
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    build = subprocess.run([hipcc, '-x', 'hip', '--offload-host-only', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                            '-o', str(prog),
                            os.path.join(ROOT, 'tests', 'host', 'parts_check.cpp'), os.path.join(ROOT, 'superdsm_amd', 'csrc', 'sdsm_host.cpp')],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(prog), str(tmp_path / 'cases.txt')], capture_output=True, text=True, timeout=120)
    assert (run.returncode, run.stderr) == (0, ''), (run.returncode, run.stderr)
    want = []
    for a, b, c, d, l in cases:
        n = (a == l) + (b == l) + (c == l) + (d == l)
        want.append(1 if n == 1 else 2 if n == 3 else 3 if n == 2 and (a == l) == (d == l) else 0)
    assert [int(line) for line in run.stdout.splitlines()] == want


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_csv_round_trip(tmp_path):
    from superdsm_amd import parts
    m = np.zeros((12, 14), np.int32)
    m[1:6, 1:6], m[2:5, 2:5], m[3, 3] = 2, 0, 5              # a ring of label 2 around a pixel of label 5
    m[8:11, 2:4], m[8, 8], m[9, 9], m[10, 12] = 2, 7, 7, 7
    for connectivity in (4, 8):
        _, _, labels = parts.parts_host(m, connectivity)
        d = parts.derive(labels, connectivity)
        path = tmp_path / f'parts{connectivity}.csv'
        parts.write_parts_csv(path, labels, connectivity)
        with open(path, newline='') as fp:
            rows = list(csv.reader(fp))
        assert rows[0] == ['label', 'connectivity'] + list(parts.DERIVED_DTYPE.names) and [int(r[0]) for r in rows[1:]] == [2, 5, 7]
        assert all(f'"{v}"' in open(path).read() for v in rows[1])           # every field is quoted
        for r in rows[1:]:
            l = int(r[0])
            assert int(r[1]) == connectivity
            for name, text in zip(parts.DERIVED_DTYPE.names, r[2:]):
                assert (float(text) if name == 'largest_fraction' else int(text)) == d[l][name].item()
        assert (d[2]['n_parts'], d[2]['holes'], d[2]['largest_area'], d[2]['largest_fraction']) == (2, 1, 16, 16 / 22)
        assert (d[7]['n_parts'], d[7]['holes']) == ((3, 0) if connectivity == 4 else (2, 0))
