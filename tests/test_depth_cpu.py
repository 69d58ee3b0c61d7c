"""The host definitions of the depth tables (superdsm_amd/depth.py) against a brute-force distance transform and hand cases, the host
helpers of the C ABI against Python integers, the derived columns and the CSV writer.  No GPU."""
import csv
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from test_measure_cpu import Obj, ellipse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def disc(radius):
    y, x = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    return y * y + x * x <= radius * radius


def brute_d2(mask):
    """d2 of every pixel of a fragment as the minimum over ALL outside places of the fragment padded by the largest possible depth."""
    mask = np.asarray(mask, bool)
    pad = (min(mask.shape) + 1) // 2
    big = np.pad(mask, pad)
    orr, occ = np.nonzero(~big)
    out = np.zeros(mask.shape, np.int64)
    for r, c in zip(*np.nonzero(mask)):
        out[r, c] = ((orr - (r + pad)) ** 2 + (occ - (c + pad)) ** 2).min()
    return out


def test_record_layout_is_mirrored():
    from superdsm_amd import _capi, depth as dp
    assert _capi.DEPTH_RECORD_DTYPE.itemsize == 80 and _capi.DEPTH_RECORD_DTYPE.itemsize % 16 == 0 and _capi.DEPTH_SHELL_DTYPE.itemsize == 32
    assert dp.TABLE_DTYPE.names == ('label',) + _capi.DEPTH_RECORD_DTYPE.names
    header = open(os.path.join(ROOT, 'include', 'sdsm.h')).read()
    assert f'#define SDSM_DEPTH_LDS_PIXELS {_capi.DEPTH_LDS_PIXELS} ' in header and f'#define SDSM_DEPTH_MAX_SHELLS {_capi.DEPTH_MAX_SHELLS}\n' in header
    assert f'#define SDSM_DEPTH_WS_PIXEL_BYTES {_capi.DEPTH_WS_PIXEL_BYTES} ' in header


@pytest.mark.parametrize('seed', range(6))
def test_the_host_definition_equals_the_brute_force_minimum(seed):
    from superdsm_amd import depth as dp
    rng = np.random.default_rng(seed)
    mask = rng.random((12, 12)) < (0.55 + 0.08 * seed)
    d2 = dp.squared_depth(mask)
    assert d2.dtype == np.int64 and np.array_equal(d2, brute_d2(mask))
    assert (d2[mask] >= 1).all() and not d2[~mask].any() and d2.max() <= 36
    table, shells = dp.depth_objects_host([Obj((3, 4), mask)], (20, 20), None, 4)
    v = np.sort(brute_d2(mask)[mask])
    k = int(np.argmax(brute_d2(mask)[mask]))
    rr, cc = np.nonzero(mask)
    row = table[0]
    assert (row['area'], row['max_d2'], row['n_max'], row['sum_d2'], row['n_rim']) == (len(v), v[-1], (v == v[-1]).sum(), v.sum(), (v == 1).sum())
    assert (row['max_row'], row['max_col']) == (3 + rr[k], 4 + cc[k])
    assert row['sum_q'] == sum(math.isqrt(int(x) << 32) for x in v)
    assert (row['med_d2_lo'], row['med_d2_hi']) == (v[(len(v) - 1) // 2], v[len(v) // 2])
    assert shells['count'][0].tolist() == [int(((v >= lo) & (v <= hi)).sum()) for lo, hi in ((1, 1), (2, 4), (5, 9), (10, 10 ** 9))]


def test_hand_cases():
    from superdsm_amd import depth as dp
    one = dp.depth_objects_host([Obj((4, 5), np.ones((1, 1)))], (9, 9))[0][0]
    assert (one['area'], one['max_d2'], one['max_row'], one['max_col'], one['n_max'], one['sum_d2'], one['sum_q'], one['n_rim'], one['flags']) == \
        (1, 1, 4, 5, 1, 1, 65536, 1, 0)
    corner = dp.depth_objects_host([Obj((0, 0), np.ones((3, 3)))], (9, 9))[0][0]                  # the frame is outside like the box
    assert (corner['max_d2'], corner['max_row'], corner['max_col'], corner['n_max'], corner['n_rim'], corner['flags']) == (4, 1, 1, 1, 8, 1)
    hole = np.ones((5, 5), bool)
    hole[2, 2] = False
    assert dp.squared_depth(hole).tolist() == [[1, 1, 1, 1, 1], [1, 2, 1, 2, 1], [1, 1, 0, 1, 1], [1, 2, 1, 2, 1], [1, 1, 1, 1, 1]]
    row = dp.depth_objects_host([Obj((1, 1), hole)], (9, 9))[0][0]
    assert (row['area'], row['max_d2'], row['max_row'], row['max_col'], row['n_max'], row['n_rim'], row['med_d2_lo'], row['med_d2_hi'], row['flags']) == \
        (24, 2, 2, 2, 4, 20, 1, 1, 0)
    empty, shells = dp.depth_objects_host([Obj((1, 1), np.zeros((3, 4)))], (9, 9), np.ones((9, 9)), 3)
    assert empty.tobytes() == np.zeros(1, dp.TABLE_DTYPE).tobytes() and shells.tobytes() == bytes(3 * 32)
    with pytest.raises(ValueError, match='n_shells'):
        dp.depth_objects_host([], (9, 9), None, 33)
    with pytest.raises(ValueError):
        dp.depth_objects_host([Obj((7, 7), np.ones((3, 3)))], (9, 9))


def test_shells_take_intensities_as_the_measurement_tables_do():
    from superdsm_amd import depth as dp, measure
    rng = np.random.default_rng(3)
    shape = (50, 60)
    g = rng.normal(size=shape) * 1e3
    g[10, 12], g[11, 12] = np.nan, -np.inf
    objs = [Obj((2, 3), disc(9)), Obj((25, 30), ellipse(rng, 10))]
    table, shells = dp.depth_objects_host(objs, shape, g, 32)
    m = measure.measure_objects_host(objs, shape, g)
    assert table['scale_exp'].tolist() == m['scale_exp'].tolist() and shells['count'].sum(axis=1).tolist() == m['area'].tolist()
    assert shells['n_finite'].sum(axis=1).tolist() == m['n_finite'].tolist() and shells['n_finite'][0].sum() == table['area'][0] - 2
    for k in range(2):                                                       # the limbs of the shells add up to the object's
        total = sum(dp.shell_sum_exact(s) for s in shells[k])
        assert total == int(m['gsum_hi'][k]) * 2 ** 32 + int(m['gsum_lo'][k])
    none = dp.depth_objects_host(objs, shape, None, 32)
    assert none[0]['scale_exp'].tolist() == [0, 0] and not none[1]['n_finite'].any() and np.array_equal(none[1]['count'], shells['count'])


def test_n_rim_equals_the_border_pixels_of_the_shape_tables():
    from superdsm_amd import depth as dp, shape as sh
    rng = np.random.default_rng(17)
    ring = disc(9) & ~np.pad(disc(4), 5)
    objs = [Obj((rng.integers(0, 30), rng.integers(0, 30)), ellipse(rng, 14)) for _ in range(8)] + [Obj((0, 0), ring), Obj((45, 45), rng.random((19, 19)) < 0.7)]
    assert dp.depth_objects_host(objs, (64, 64))[0]['n_rim'].tolist() == sh.shape_objects_host(objs, (64, 64))[0]['border_pixels'].tolist()


def test_labels_see_their_neighbours_as_outside():
    from superdsm_amd import depth as dp
    touching = np.zeros((9, 40), np.int32)
    touching[1:6, 2:20], touching[1:8, 20:37], touching[6:8, 2:20] = 1, 2, 5
    table, shells = dp.depth_labels_host(touching, None, 4)
    assert table['label'].tolist() == [1, 2, 5] and table['max_d2'].tolist() == [9, 16, 1] and shells.shape == (3, 4)
    by_object = dp.depth_objects_host([Obj((1, 2), np.ones((5, 18))), Obj((1, 20), np.ones((7, 17))), Obj((6, 2), np.ones((2, 18)))], touching.shape, None, 4)
    by_object[0]['label'] = [1, 2, 5]
    assert by_object[0].tobytes() == table.tobytes() and by_object[1].tobytes() == shells.tobytes()
    kept = dp.depth_labels_host(touching, None, 4, keep_absent=True)
    assert kept[0]['label'].tolist() == [0, 1, 2, 3, 4, 5] and kept[0]['area'].tolist() == [0, 90, 119, 0, 0, 36] and not kept[1][[0, 3, 4]]['count'].any()


# ---- the host helpers of the C ABI ---------------------------------------------------------------------------------------------------
def test_the_shell_helper_equals_the_integer_root():
    from superdsm_amd import _capi, depth as dp
    shell = _capi.lib().sdsm_depth_shell
    k = np.arange(1, 32769, dtype=np.int64)
    around = np.unique(np.concatenate([k * k - 1, k * k, k * k + 1, k * k + 2]))
    values = np.concatenate([np.arange(1, 70001), around[around > 70000]])
    assert values.max() == 2 ** 30 + 2
    for n_shells in (1, 2, 32):
        for d2 in values.tolist():
            want = min(n_shells - 1, math.isqrt(d2 - 1))
            if shell(d2, n_shells) != want:
                raise AssertionError(f'sdsm_depth_shell({d2}, {n_shells}) = {shell(d2, n_shells)}, expected {want}')
    assert [dp.shell_of(d2, 32) for d2 in (1, 2, 4, 5, 9, 10)] == [shell(d2, 32) for d2 in (1, 2, 4, 5, 9, 10)] == [0, 1, 1, 2, 2, 3]
    assert [shell(0, 8), shell(-5, 8), shell(2 ** 31, 8), shell(5, 0), shell(5, 33), shell(5, -1)] == [-1] * 6


def test_the_workspace_helper_at_the_cap():
    from superdsm_amd import _capi, depth as dp
    ws, cap = _capi.lib().sdsm_depth_workspace_pixels, _capi.DEPTH_LDS_PIXELS
    assert (ws(96, 128), ws(97, 128), ws(1, cap), ws(1, cap + 1), ws(cap + 1, 1), ws(0, 7), ws(7, 0), ws(-1, -1)) == (0, 97 * 128, 0, cap + 1, cap + 1, 0, 0, 0)
    boxes = [(0, 0, 96, 128), (5, 5, 97, 128), (0, 0, 0, 7), (0, 0, 511, 511)]
    assert dp.workspace_pixels(boxes).tolist() == [ws(b[2], b[3]) for b in boxes]


def test_the_shell_helper_alone_under_the_sanitizers(tmp_path):
    """tests/host/depth_check.cpp with sdsm_host.cpp as host code only, AddressSanitizer and UndefinedBehaviorSanitizer linked into the
    executable (as tests/test_intensity_cpu.py builds its program).  No GPU; a failing compile fails the test."""
    cases = [(d2, s) for s in (1, 2, 32) for d2 in (1, 2, 4, 5, 9, 10, 1024, 1025, 65025, 65536, 65537, 2 ** 30, 2 ** 30 + 1, 2 ** 31 - 1)]
    (tmp_path / 'cases.txt').write_text(''.join(f'{d2} {s}\n' for d2, s in cases))
    prog = tmp_path / 'depth_check'
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    build = subprocess.run([hipcc, '-x', 'hip', '--offload-host-only', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                            '-o', str(prog),
                            os.path.join(ROOT, 'tests', 'host', 'depth_check.cpp'), os.path.join(ROOT, 'superdsm_amd', 'csrc', 'sdsm_host.cpp')],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(prog), str(tmp_path / 'cases.txt')], capture_output=True, text=True, timeout=120)
    assert (run.returncode, run.stderr) == (0, ''), (run.returncode, run.stderr)
    assert [int(line) for line in run.stdout.splitlines()] == [min(s - 1, math.isqrt(d2 - 1)) for d2, s in cases]


# ---- derived columns and the CSV ---------------------------------------------------------------------------------------------------------
def test_derive_on_a_disc_of_radius_20():
    from superdsm_amd import depth as dp
    shape = (60, 70)
    g = np.fromfunction(lambda r, c: 1.0 + ((r * 7 + c * 3) % 11) / 8, shape)
    table, shells = dp.depth_objects_host([Obj((5, 9), disc(20)), Obj((50, 2), np.zeros((2, 2)))], shape, g, 8)
    d = dp.derive(table, shells)
    row, n = table[0], int(table[0]['area'])
    assert row['max_d2'] == 401 and (row['max_row'], row['max_col']) == (25, 29) and n == int(disc(20).sum())
    assert d['max_radius'][0] == math.sqrt(401) and d['thickness'][0] == 2 * math.sqrt(401) - 1
    assert d['mean_radius'][0] == int(row['sum_q']) / 65536 / n and abs(d['mean_radius'][0] - np.sqrt(dp.squared_depth(disc(20))[disc(20)]).mean()) < 2 ** -16
    assert d['median_radius'][0] == 0.5 * math.sqrt(int(row['med_d2_lo'])) + 0.5 * math.sqrt(int(row['med_d2_hi']))
    assert d['rms_radius'][0] == math.sqrt(int(row['sum_d2']) / n)
    assert (d['center_row'][0], d['center_col'][0], d['on_boundary'][0]) == (25, 29, False)
    e = int(row['scale_exp'])
    sums = [int(s['gsum_hi']) * 2 ** 32 + int(s['gsum_lo']) for s in shells[0]]
    for s in range(8):
        assert d[f'shell{s}_fraction'][0] == int(shells[0, s]['count']) / n
        assert d[f'shell{s}_mean_intensity'][0] == math.ldexp(sums[s] / int(shells[0, s]['n_finite']), e - 62)
        assert d[f'shell{s}_intensity_fraction'][0] == sums[s] / sum(sums)
    assert abs(sum(d[f'shell{s}_fraction'][0] for s in range(8)) - 1) < 1e-12 and shells[0, 7]['count'] == (dp.squared_depth(disc(20)) > 49).sum()
    assert d['area'][1] == 0 and all(np.isnan(d[name][1]) for name in d.dtype.names[5:])
    with pytest.raises(ValueError, match='shells'):
        dp.derive(table, shells[:1])


def test_csv_round_trip(tmp_path):
    from superdsm_amd import _capi, depth as dp
    rng = np.random.default_rng(4)
    shape = (40, 40)
    table, shells = dp.depth_objects_host([Obj((1, 1), disc(8)), Obj((20, 15), ellipse(rng, 9)), Obj((0, 30), np.zeros((2, 2)))], shape, rng.random(shape), 3)
    dp.write_depth_csv(tmp_path / 'depth.csv', table, shells)
    rows = list(csv.reader(open(tmp_path / 'depth.csv')))
    d = dp.derive(table, shells)
    assert len(rows) == 4 and rows[0][:len(d.dtype.names)] == list(d.dtype.names) and len(set(rows[0])) == len(rows[0])
    col = {name: i for i, name in enumerate(rows[0])}
    for k in range(3):
        for name in d.dtype.names:
            v = eval(rows[k + 1][col[name]], {'nan': math.nan, 'inf': math.inf})
            assert v == d[name][k] or (v != v and d[name][k] != d[name][k]), (k, name)
        for name in ('max_d2', 'max_row', 'max_col', 'n_max', 'sum_d2', 'sum_q', 'med_d2_lo', 'med_d2_hi', 'n_rim', 'flags', 'scale_exp'):
            assert int(rows[k + 1][col[name]]) == table[name][k]
        for s in range(3):
            for name in _capi.DEPTH_SHELL_DTYPE.names:
                assert int(rows[k + 1][col[f'shell{s}_{name}']]) == shells[k, s][name]
