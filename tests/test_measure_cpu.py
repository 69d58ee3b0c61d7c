"""The host definitions of the measurement tables (superdsm_amd/measure.py) pin themselves to SciPy and to exact arithmetic: centroids
to ``ndi.center_of_mass`` bit for bit, the regression rows to ``render.label_map_rows``, the eccentricity to the same formula in
60-digit decimal, the intensity sums to the exact rational sum of the pixels."""
import csv
import decimal
import math
from fractions import Fraction

import numpy as np
import pytest
import scipy.ndimage as ndi


class Obj:
    def __init__(self, offset, fragment):
        self.fg_offset, self.fg_fragment = np.asarray(offset), np.asarray(fragment, bool)


def ellipse(rng, max_axis=30, erode=True):
    """A random filled ellipse, partly eroded: a random half-plane of it loses its boundary pixels."""
    a, b, t = rng.uniform(2, max_axis), rng.uniform(2, max_axis), rng.uniform(0, np.pi)
    m = int(max(a, b)) + 2
    y, x = np.mgrid[-m:m + 1, -m:m + 1].astype(float)
    u, v = x * np.cos(t) + y * np.sin(t), -x * np.sin(t) + y * np.cos(t)
    f = (u / a) ** 2 + (v / b) ** 2 <= 1
    if erode and rng.random() < 0.7:
        side = (x * np.cos(t + 1) + y * np.sin(t + 1)) > rng.uniform(-2, 2)
        f = np.where(side, ndi.binary_erosion(f), f)
    rr, cc = np.nonzero(f)
    return f[rr.min():rr.max() + 1, cc.min():cc.max() + 1]


def label_scene(rng, shape=(90, 120), n=14):
    """A label map of random ellipses and boxes (later ones over earlier ones) and the objects that produced it."""
    labels = np.zeros(shape, np.int32)
    for l in range(1, n + 1):
        f = ellipse(rng, 12) if l % 3 else np.ones((rng.integers(1, 9), rng.integers(1, 9)), bool)
        r0, c0 = rng.integers(0, shape[0] - f.shape[0] + 1), rng.integers(0, shape[1] - f.shape[1] + 1)
        labels[r0:r0 + f.shape[0], c0:c0 + f.shape[1]][f] = l
    return labels


def test_record_layout_is_mirrored():
    import ctypes as C
    from superdsm_amd import _capi, measure
    assert _capi.MEASURE_RECORD_DTYPE.itemsize == C.sizeof(_capi.MeasureRecord) == 112
    assert measure.TABLE_DTYPE.names[1:] == _capi.MEASURE_RECORD_DTYPE.names
    assert _capi.MEASURE_RECORD_DTYPE.fields['n_finite'][1] == 72 and _capi.MEASURE_RECORD_DTYPE.fields['gmin'][1] == 96


def test_centroids_equal_center_of_mass_bit_for_bit_and_rows_equal_label_map_rows():
    from superdsm_amd import measure, render
    rng = np.random.default_rng(5)
    for trial in range(4):
        labels = label_scene(rng)
        table = measure.measure_labels_host(labels)
        d = measure.derive(table)
        present = sorted(set(labels.ravel().tolist()) - {0})
        assert table['label'].tolist() == present
        for row, drow in zip(table, d):
            cy, cx = ndi.center_of_mass(labels == row['label'])
            assert (drow['centroid_r'], drow['centroid_c']) == (cy, cx)                 # the same float64, not merely close
            assert row['area'] == (labels == row['label']).sum()
        assert measure.rows_from_table(table) == render.label_map_rows(labels)
    # a uint16 label map with the wrapped background label 65535 (render.rasterize_labels, background_label = -1)
    wrapped = labels.astype(np.uint16)
    wrapped[wrapped == 0] = 65535
    t = measure.measure_labels_host(wrapped, background_label=65535)
    assert t['label'].tolist() == present and (t['area'] == table['area']).all()


def test_objects_and_labels_agree_and_match_python_integers():
    """Objects cut out of a label map give the label form's records; at the far corner of the largest image the sums are those of
    Python integers (sum_rr passes 2^32 many times over: a 32-bit accumulator anywhere would not)."""
    from superdsm_amd import measure
    rng = np.random.default_rng(11)
    labels = label_scene(rng)
    g = rng.normal(size=labels.shape)
    by_label = measure.measure_labels_host(labels, g)
    objs = []
    for l in by_label['label']:
        rr, cc = np.nonzero(labels == l)
        objs.append(Obj((rr.min(), cc.min()), (labels == l)[rr.min():rr.max() + 1, cc.min():cc.max() + 1]))
    by_object = measure.measure_objects_host(objs, labels.shape, g)
    for name in measure.TABLE_DTYPE.names[1:]:
        assert (by_object[name] == by_label[name]).all(), name
    frag = ellipse(rng, 25)
    off = (65535 - frag.shape[0], 32000 - frag.shape[1])
    t = measure.measure_objects_host([Obj(off, frag)], (65535, 32000))[0]
    rr, cc = (v.tolist() for v in np.nonzero(frag))
    R, Cc = [r + off[0] for r in rr], [c + off[1] for c in cc]
    assert int(t['sum_rr']) == sum(r * r for r in R) > 2 ** 32 and int(t['sum_rc']) == sum(r * c for r, c in zip(R, Cc))
    assert int(t['sum_cc']) == sum(c * c for c in Cc) and (int(t['sum_r']), int(t['sum_c']), int(t['area'])) == (sum(R), sum(Cc), len(R))
    assert (t['r0'], t['c0'], t['r1'], t['c1'], t['flags']) == (off[0], off[1], 65535, 32000, 1)


def test_eccentricity_within_3_ulp_of_the_exact_formula():
    """400 random, partly eroded ellipses at offsets up to 65 000 against the same formula in 60-digit decimal.  The bound is derived:
    three correctly rounded conversions, root <= 1.5 ulp, s + root <= 2 ulp, the quotient <= 4 ulp, the square root halves that and
    adds half an ulp: 3 ulp of the result.  Against the float pass of post-processing (not the definition) 1e-12 absolute documents
    the distance."""
    from superdsm_amd import _capi, measure
    from superdsm_amd.postprocess import _compute_eccentricity
    decimal.getcontext().prec = 60
    rng = np.random.default_rng(2024)
    worst_ulp = worst_abs = 0.0
    for trial in range(400):
        f = ellipse(rng, 30) if trial % 8 else ellipse(rng, 6, erode=False)
        off = rng.integers(0, 65001, 2)
        rec = measure._zero_records(1, 0)
        rr, cc = np.nonzero(f)
        measure._fill_record(rec, rr + off[0], cc + off[1], (65535, 65535), None, 0)
        ecc = float(measure.derive(measure._as_table(rec, [0]))['eccentricity'][0])
        n, sr, sc, srr, src, scc = (int(rec[k][0]) for k in ('area', 'sum_r', 'sum_c', 'sum_rr', 'sum_rc', 'sum_cc'))
        A, B, D = n * srr - sr * sr, n * src - sr * sc, n * scc - sc * sc
        p, q, s = decimal.Decimal(A - D), decimal.Decimal(2 * B), decimal.Decimal(A + D)
        root = (p * p + q * q).sqrt()
        ref = (2 * root / (s + root)).sqrt() if s + root != 0 else decimal.Decimal(0)
        err = abs(decimal.Decimal(ecc) - ref)
        ulp = decimal.Decimal(math.ulp(float(ref))) if ref != 0 else decimal.Decimal(0)
        assert err <= 3 * ulp, (trial, ecc, ref)
        worst_ulp = max(worst_ulp, float(err / ulp) if ulp else 0.0)
        worst_abs = max(worst_abs, abs(ecc - _compute_eccentricity(f)))
    print(f'eccentricity: worst {worst_ulp:.2f} ulp against decimal, worst {worst_abs:.2e} against the float pass')
    assert worst_abs <= 1e-12


def _check_intensity_rows(table, pixel_values, e):
    """Per row: the recombined limbs against the exact rational sum of the finite pixels: n_finite * 2^(e - 63), half a quantum per pixel
    by construction.  math.fsum is that exact sum rounded to float64 once more, and its rounding alone can exceed the bound (27 pixels
    of N(0, 1e6): fsum is 1.07e-13 from the exact sum, the bound is 1.2e-14), so against fsum the bound is allowed fsum's half ulp on top;
    the assertion against the exact sum is the stricter of the two.  Min and max as NumPy's."""
    from superdsm_amd import measure
    for row, vals in zip(table, pixel_values):
        v = vals[np.isfinite(vals)]
        assert row['scale_exp'] == e and row['n_finite'] == len(v)
        assert bool(row['flags'] & 2) == (len(v) < len(vals))
        S = measure.intensity_sum_exact(row)
        bound = len(v) * Fraction(2) ** (e - 63)
        assert abs(S - sum((Fraction(float(x)) for x in v), Fraction(0))) <= bound
        try:
            fs = math.fsum(v.tolist())
        except OverflowError:                                                 # (a sum beyond the float64 range: the exact check stands alone)
            fs = None
        if fs is not None:
            assert abs(S - Fraction(fs)) <= bound + Fraction(math.ulp(fs)) / 2
        if len(v):
            assert row['gmin'] == np.min(v) and row['gmax'] == np.max(v)
        else:
            assert row['gmin'] == np.inf and row['gmax'] == -np.inf


def test_intensity_limbs_recombine():
    from superdsm_amd import measure
    rng = np.random.default_rng(3)
    labels = label_scene(rng, (40, 50), 6)
    present = sorted(set(labels.ravel().tolist()))
    huge = np.full(labels.shape, 1e-300)
    huge[7, 9] = 1e300
    holes = rng.normal(size=labels.shape)
    rr, cc = np.nonzero(labels == present[1])
    holes[rr[0], cc[0]], holes[rr[-1], cc[-1]] = np.nan, np.inf
    images = {'signed': rng.normal(size=labels.shape) * 1e3, 'negative': -rng.random(labels.shape) - 0.5, 'zero': np.zeros(labels.shape),
              'huge and tiny': huge, 'nan and inf': holes, 'tiny': rng.random(labels.shape) * 2.0 ** -970, 'largest': np.full(labels.shape, np.finfo(float).max)}
    for name, g in images.items():
        e = measure.scale_exponent(g)
        fin = np.abs(g[np.isfinite(g)])
        assert e == 0 if not fin.any() else (fin.max() < Fraction(2) ** e and (e == -960 or fin.max() >= Fraction(2) ** (e - 1))), name
        table = measure.measure_labels_host(labels, g, background_label=None)
        assert table['label'].tolist() == present
        _check_intensity_rows(table, [g[labels == l] for l in present], e)
        d = measure.derive(table)
        for row, drow, l in zip(table, d, present):
            if row['n_finite'] and name != 'largest':
                assert drow['integrated_intensity'] == float(measure.intensity_sum_exact(row))
                assert drow['mean_intensity'] == float(measure.intensity_sum_exact(row) / int(row['n_finite']))
    assert measure.scale_exponent(images['tiny']) == -960 and measure.scale_exponent(images['largest']) == 1024
    assert measure.scale_exponent(images['zero']) == 0 and measure.scale_exponent(np.full((2, 2), np.nan)) == 0
    assert measure.scale_exponent(np.array([[1.0]])) == 1 and measure.scale_exponent(np.array([[-0.75]])) == 0
    zero = measure.measure_labels_host(labels, images['zero'], background_label=None)
    assert (zero['gsum_lo'] == 0).all() and (zero['gsum_hi'] == 0).all() and (zero['gmin'] == 0).all()
    t = measure.measure_labels_host(labels, np.where(labels > 0, -0.0, 0.0), background_label=None)
    assert not np.signbit(t['gmin']).any() and not np.signbit(t['gmax']).any()            # -0.0 reads +0.0


def test_empty_object_and_derived_columns():
    from superdsm_amd import measure
    objs = [Obj((3, 4), np.zeros((2, 3), bool)), Obj((0, 0), np.ones((1, 1), bool)), Obj((2, 2), np.ones((4, 6), bool))]
    t = measure.measure_objects_host(objs, (8, 9), np.arange(72.0).reshape(8, 9))
    assert t[0]['area'] == 0 and (t[0]['r0'], t[0]['c0'], t[0]['r1'], t[0]['c1'], t[0]['flags'], t[0]['n_finite']) == (0, 0, 0, 0, 0, 0)
    assert t[0]['gmin'] == np.inf and t[0]['gmax'] == -np.inf
    d = measure.derive(t)
    assert np.isnan(d['centroid_r'][0]) and np.isnan(d['mean_intensity'][0]) and d['integrated_intensity'][0] == 0
    assert (d['centroid_r'][1], d['centroid_c'][1], d['eccentricity'][1], d['on_boundary'][1]) == (0.0, 0.0, 0.0, True)
    assert d['equivalent_radius'][2] == math.sqrt(24 / math.pi) and not d['on_boundary'][2]
    assert d['mean_intensity'][2] == np.arange(72.0).reshape(8, 9)[2:6, 2:8].mean() and d['max_intensity'][2] == 5 * 9 + 7
    # a 4 x 6 rectangle: central moments (h^2 - 1) / 12 and (w^2 - 1) / 12
    l1, l2 = 35 / 12, 15 / 12
    assert d['major_axis_length'][2] == pytest.approx(4 * math.sqrt(l1), rel=1e-15) and d['minor_axis_length'][2] == pytest.approx(4 * math.sqrt(l2), rel=1e-15)
    assert d['eccentricity'][2] == pytest.approx(math.sqrt(1 - l2 / l1), rel=1e-15)


def test_csv_round_trip(tmp_path):
    from superdsm_amd import measure
    rng = np.random.default_rng(8)
    labels = label_scene(rng, (40, 50), 5)
    table = measure.measure_labels_host(labels, rng.random(labels.shape))
    path = tmp_path / 'table.csv'
    measure.write_measurements_csv(path, table)
    text = path.read_text()
    assert text.startswith('"label","area","centroid_r"')
    with open(path, newline='') as fp:
        rows = list(csv.reader(fp))
    d = measure.derive(table)
    assert len(rows) == 1 + len(table) and [float(r[2]) for r in rows[1:]] == d['centroid_r'].tolist()
    assert [float(r[rows[0].index('mean_intensity')]) for r in rows[1:]] == d['mean_intensity'].tolist()


def test_limits_raise_before_any_upload():
    """The checks of the GPU forms come before the device is touched, so they hold on a machine without one."""
    from superdsm_amd import measure
    ok = Obj((1, 1), np.ones((2, 2), bool))
    with pytest.raises(ValueError):
        measure.measure_objects([ok, Obj((7, 1), np.ones((2, 2), bool))], (8, 8))         # a box leaving the image
    with pytest.raises(ValueError):
        measure.measure_objects([Obj((-1, 0), np.ones((2, 2), bool))], (8, 8))
    with pytest.raises(ValueError):
        measure.measure_objects([ok], (8, 8), np.zeros((8, 9)))                             # an intensity of another shape
    with pytest.raises(TypeError):
        measure.measure_labels(np.zeros((8, 8)))                                            # a label map that is not an integer type
    with pytest.raises(ValueError):
        measure.measure_labels(np.zeros((8, 8), np.int32), np.zeros((4, 4)))
    with pytest.raises(ValueError):
        measure.measure_labels(np.zeros((8, 8), np.int32), n_labels=65537)
    with pytest.raises(ValueError):
        measure.measure_labels_host(np.full((2, 2), 65536))
    with pytest.raises(ValueError):
        measure.measure_labels_host(np.full((2, 2), -1))
