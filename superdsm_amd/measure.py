"""Per-object measurement tables: counts, sizes, positions, shapes and intensities of the objects of a segmentation, from objects
(bit-packed fragments, which may overlap) or from label maps, for one image or a set of images.

The reference keeps its only per-object measurements in a test helper (tests/regression/validate.py:31-36: area and centre of mass
per label) and one ``regionprops(...).eccentricity`` call (superdsm/postprocess.py:340-344).  Here a table is a structured array
with one row per object or label that holds EXACT integers (``sdsm_measure_record``, include/sdsm.h): pixel count, first and second
moments of the coordinates, bounding box, and the intensity sum as two limbs of the integers ``rint(ldexp(g, 62 - e))``, with ``e``
fixed per image by its largest finite ``|g|``.  Integer sums do not depend on the order, so the GPU forms (sdsm_measure.hip) give the
bytes of the ``*_host`` definitions below, whatever the launch or the set size.  Everything that is not an integer -- centroids,
radii, eccentricity, axis lengths, mean intensities -- is computed in ONE place, :func:`derive`, on the host from those integers.

The standard deviation of the intensities is not part of a table: a one-pass sum of squares minus the squared mean loses the digits
that post-processing was changed to keep.  The second pass it needs is :mod:`intensity`, which centres the squares on each object's own
minimum and adds the median, quantiles and the median absolute deviation."""
import csv
import math
from fractions import Fraction

import numpy as np

from . import _capi
from .imageset import in_sets
from .postprocess import _check_boxes, _exclusive, pack_fragments

TABLE_DTYPE = np.dtype([('label', 'i4')] + _capi._MEASURE_FIELDS)     # 'label': the label, or the index of the object in its image
SCALE_EXP_MIN, SCALE_EXP_MAX = -960, 1024

DERIVED_DTYPE = np.dtype([('label', 'i4'), ('area', 'i8'), ('centroid_r', 'f8'), ('centroid_c', 'f8'), ('equivalent_radius', 'f8'),
                          ('on_boundary', '?'), ('eccentricity', 'f8'), ('major_axis_length', 'f8'), ('minor_axis_length', 'f8'),
                          ('integrated_intensity', 'f8'), ('mean_intensity', 'f8'), ('min_intensity', 'f8'), ('max_intensity', 'f8'),
                          ('nonfinite_inside', '?')])


# ---- the definitions: NumPy and Python integers ---------------------------------------------------------------------------------------
def scale_exponent(intensity):
    """``e`` of an image: the smallest exponent with (largest finite ``|g|``) < 2^e, clamped to -960 .. 1024; 0 for an image without a
    non-zero finite pixel.  The intensity quantum of the image's table is 2^(e - 62)."""
    g = np.asarray(intensity, np.float64)
    a = np.abs(g[np.isfinite(g)])
    m = float(a.max()) if a.size else 0.0
    if m == 0.0:
        return 0
    return min(SCALE_EXP_MAX, max(SCALE_EXP_MIN, math.frexp(m)[1]))          # m = f * 2^x with 0.5 <= f < 1: 2^(x - 1) <= m < 2^x


def quantize(values, e):
    """The integers that finite intensities add to a table: ``rint(ldexp(g, 62 - e))`` (ties to even), |q| <= 2^62."""
    return np.rint(np.ldexp(np.asarray(values, np.float64), 62 - int(e))).astype(np.int64)


def _zero_records(n, e):
    recs = np.zeros(n, _capi.MEASURE_RECORD_DTYPE)
    recs['scale_exp'], recs['gmin'], recs['gmax'] = e, np.inf, -np.inf
    return recs


def _fill_record(rec, rr, cc, shape, g, e):
    """The record of the pixels (rr, cc) -- image coordinates -- of an image of ``shape`` with the intensities ``g`` (or None)."""
    if len(rr) == 0:
        return
    r, c = np.asarray(rr).astype(np.int64), np.asarray(cc).astype(np.int64)
    ru, cu = r.astype(np.uint64), c.astype(np.uint64)                          # r, c <= 65534 and < 2^31 pixels: below 2^63, nothing wraps
    rec['area'] = len(r)
    rec['sum_r'], rec['sum_c'] = int(r.sum(dtype=np.int64)), int(c.sum(dtype=np.int64))
    rec['sum_rr'], rec['sum_rc'], rec['sum_cc'] = (int((a * b).sum(dtype=np.uint64)) for a, b in ((ru, ru), (ru, cu), (cu, cu)))
    r0, c0, r1, c1 = int(r.min()), int(c.min()), int(r.max()) + 1, int(c.max()) + 1
    rec['r0'], rec['c0'], rec['r1'], rec['c1'] = r0, c0, r1, c1
    flags = int(r0 == 0 or c0 == 0 or r1 == shape[0] or c1 == shape[1])
    if g is not None:
        vals = g[r, c]
        fin = np.isfinite(vals)
        v = vals[fin]
        flags |= 2 * int(not fin.all())
        if len(v):
            q = quantize(v, e)
            rec['n_finite'] = len(v)
            rec['gsum_lo'] = int((q & 0xffffffff).astype(np.uint64).sum(dtype=np.uint64))      # < 2^31 pixels * 2^32
            rec['gsum_hi'] = int((q >> 32).sum(dtype=np.int64))                                # |q >> 32| <= 2^30
            rec['gmin'], rec['gmax'] = v.min() + 0.0, v.max() + 0.0                            # (-0.0 + 0.0 = +0.0)
    rec['flags'] = flags


def _check_intensity(intensity, shape):
    if intensity is None:
        return None
    g = np.asarray(intensity)
    if g.dtype.kind not in 'fiub' or g.shape != tuple(shape):
        raise ValueError(f'intensity: a real image of the shape of its label map or objects, {tuple(shape)}; got {g.dtype} {g.shape}')
    return np.ascontiguousarray(g, np.float64)


def _check_shape(shape):
    shape = tuple(int(v) for v in shape)
    if len(shape) != 2 or min(shape) < 1 or max(shape) > 65535 or shape[0] * shape[1] >= 2 ** 31 - 1:
        raise ValueError(f'shape {shape}: the measurement tables take H x W images with H, W <= 65535 and H * W < 2^31, see DESIGN.md "Limits"')
    return shape


def _object_boxes(objects):
    return np.array([(int(o.fg_offset[0]), int(o.fg_offset[1])) + tuple(o.fg_fragment.shape) for o in objects], np.int64).reshape(-1, 4)


def _as_table(recs, labels):
    table = np.zeros(len(recs), TABLE_DTYPE)
    table['label'] = labels
    for name in _capi.MEASURE_RECORD_DTYPE.names:
        table[name] = recs[name]
    return table


def measure_objects_host(objects, shape, intensity=None):
    """The table of a list of objects (``fg_offset``, ``fg_fragment``) of an image of ``shape``, object by object; row k is object k."""
    shape = _check_shape(shape)
    objects = list(objects)
    _check_boxes(_object_boxes(objects), shape)
    g = _check_intensity(intensity, shape)
    e = scale_exponent(g) if g is not None else 0
    recs = _zero_records(len(objects), e)
    for k, obj in enumerate(objects):
        rr, cc = np.nonzero(np.asarray(obj.fg_fragment, bool))
        _fill_record(recs[k:k + 1], rr + int(obj.fg_offset[0]), cc + int(obj.fg_offset[1]), shape, g, e)
    return _as_table(recs, np.arange(len(objects)))


def _check_labels(labels):
    labels = np.asarray(labels)
    if labels.dtype.kind not in 'iu' or labels.ndim != 2:
        raise TypeError(f'labels: a two-dimensional integer image; got {labels.dtype}, {labels.ndim} dimensions')
    _check_shape(labels.shape)
    return labels


def label_records_host(labels, n_labels, intensity=None):
    """The records of the labels 0 .. ``n_labels`` - 1 of a label map, label by label (what sdsm_measure_labels writes): absent labels keep
    the zero record.  Returns (records, number of pixels with a label outside the range)."""
    labels = _check_labels(labels)
    g = _check_intensity(intensity, labels.shape)
    e = scale_exponent(g) if g is not None else 0
    recs = _zero_records(n_labels, e)
    for l in sorted(frozenset(labels.reshape(-1).tolist())):
        if 0 <= l < n_labels:
            rr, cc = np.nonzero(labels == l)
            _fill_record(recs[l:l + 1], rr, cc, labels.shape, g, e)
    return recs, int(((labels < 0) | (labels >= n_labels)).sum())


def _present(recs, background_label):
    keep = recs['area'] > 0
    if background_label is not None and 0 <= background_label < len(recs):
        keep[background_label] = False
    ls = np.nonzero(keep)[0]
    return _as_table(recs[ls], ls)


def _label_count(labels):
    """Labels 0 .. max of a label map, checked against the limits of the label form."""
    lo, hi = int(labels.min()), int(labels.max())
    if lo < 0 or hi >= _capi.MEASURE_MAX_LABELS:
        raise ValueError(f'labels {lo} .. {hi}: the measurement tables take the labels 0 .. {_capi.MEASURE_MAX_LABELS - 1}, see DESIGN.md "Limits"')
    return hi + 1


def measure_labels_host(labels, intensity=None, background_label=0):
    """The table of a label map, label by label: the present labels without ``background_label`` (None: all), in ascending order."""
    labels = _check_labels(labels)
    return _present(label_records_host(labels, _label_count(labels), intensity)[0], background_label)


# ---- derived columns: one function for the host and the GPU forms -----------------------------------------------------------------------
def intensity_sum_exact(row):
    """The intensity sum of a row as the exact rational (gsum_hi * 2^32 + gsum_lo) * 2^(e - 62)."""
    return Fraction(int(row['gsum_hi']) * 2 ** 32 + int(row['gsum_lo'])) * Fraction(2) ** (int(row['scale_exp']) - 62)


def _scaled(x, e):
    try:
        return math.ldexp(x, e)
    except OverflowError:                                                     # (a sum beyond the float64 range)
        return math.copysign(math.inf, x)


def _shape_columns(n, sr, sc, srr, src, scc):
    """(eccentricity, major axis, minor axis) of the ellipse with the second central moments of the pixels.  The differences are taken
    in Python integers before the one conversion, so nothing cancels in floating point."""
    A, B, D = n * srr - sr * sr, n * src - sr * sc, n * scc - sc * sc         # n^2 times the central moments
    p, q, s = float(A - D), float(2 * B), float(A + D)
    root = math.sqrt(p * p + q * q)
    ecc = math.sqrt(2 * root / (s + root)) if s + root != 0 else 0.0
    n2 = float(n * n)
    return ecc, 4 * math.sqrt((s + root) / 2 / n2), 4 * math.sqrt(max(0.0, (s - root) / 2) / n2)


def derive(table):
    """The derived columns of a table (``DERIVED_DTYPE``), on the host from its exact integers.  Rows without a pixel read NaN."""
    out = np.zeros(len(table), DERIVED_DTYPE)
    out['label'], out['area'] = table['label'], table['area']
    with np.errstate(invalid='ignore', divide='ignore'):
        out['centroid_r'] = table['sum_r'].astype(np.float64) / table['area'].astype(np.float64)      # one division of exact integers
        out['centroid_c'] = table['sum_c'].astype(np.float64) / table['area'].astype(np.float64)
    out['equivalent_radius'] = np.sqrt(table['area'] / np.pi)                 # obj_radius of superdsm/postprocess.py:296
    out['on_boundary'], out['nonfinite_inside'] = (table['flags'] & 1) != 0, (table['flags'] & 2) != 0
    out['min_intensity'], out['max_intensity'] = table['gmin'], table['gmax']
    for k, row in enumerate(table):
        n, nf, e = int(row['area']), int(row['n_finite']), int(row['scale_exp'])
        if n == 0:
            out['eccentricity'][k] = out['major_axis_length'][k] = out['minor_axis_length'][k] = np.nan
        else:
            out['eccentricity'][k], out['major_axis_length'][k], out['minor_axis_length'][k] = _shape_columns(
                n, int(row['sum_r']), int(row['sum_c']), int(row['sum_rr']), int(row['sum_rc']), int(row['sum_cc']))
        S = int(row['gsum_hi']) * 2 ** 32 + int(row['gsum_lo'])
        out['integrated_intensity'][k] = _scaled(float(S), e - 62)
        out['mean_intensity'][k] = _scaled(float(Fraction(S, nf)), e - 62) if nf else np.nan
    return out


def rows_from_table(table):
    """The rows of ``render.label_map_rows`` (tests/regression/validate.py:31-36) from the table of a label map without its background:
    ``(str(area), str(round(centre_x, 1)), str(round(centre_y, 1)))``, sorted by the centre columns."""
    d = derive(table)
    rows = [(str(int(a)), str(round(cx, 1)), str(round(cy, 1))) for a, cx, cy in zip(d['area'], d['centroid_c'], d['centroid_r'])]
    rows.sort(key=lambda row: row[1:3])
    return rows


def write_measurements_csv(path, table):
    """A table with its derived columns as CSV, every field quoted (as ``render.write_rows_csv``)."""
    d = derive(table)
    names = list(DERIVED_DTYPE.names) + ['bbox_r0', 'bbox_c0', 'bbox_r1', 'bbox_c1', 'n_finite']
    with open(path, 'w', newline='') as fp:
        w = csv.writer(fp, delimiter=',', quoting=csv.QUOTE_ALL)
        w.writerow(names)
        for drow, row in zip(d, table):
            w.writerow([repr(v.item()) for v in drow] + [repr(int(row[k])) for k in ('r0', 'c0', 'r1', 'c1', 'n_finite')])


# ---- the GPU forms (sdsm_measure.hip) ---------------------------------------------------------------------------------------------
class _MeasureSet:
    """One set of up to ``_capi.MAX_SET_IMAGES`` images on the current device and the two calls of the measurement kernels."""

    def __init__(self, shapes, intensities):
        from .render import _DeviceSet
        self.S = S = _DeviceSet(shapes)
        self.n_im = len(S.shapes)
        self.d_g = S.pack(intensities, np.float64) if intensities is not None else None
        self.d_gmax = S.torch.empty(self.n_im, dtype=S.torch.float64, device=S.dev)
        self.d_exp = S.torch.empty(self.n_im, dtype=S.torch.int32, device=S.dev)

    def _records(self, d_out, n):
        return d_out.cpu().numpy()[:n * _capi.MEASURE_RECORD_DTYPE.itemsize].view(_capi.MEASURE_RECORD_DTYPE).copy()

    def record_buffer(self, n):
        return self.S.torch.empty(max(1, n) * _capi.MEASURE_RECORD_DTYPE.itemsize, dtype=self.S.torch.uint8, device=self.S.dev)

    def objects(self, obj_image, boxes, words, packed):
        """The records of the objects of the set (``packed``: the bit-packed fragments, one uint8 array of whole words each)."""
        S, n = self.S, len(boxes)
        d_out = self.record_buffer(n)
        d_image, d_boxes, d_off = S._up(np.asarray(obj_image, np.int32)), S._up(np.asarray(boxes, np.int32).reshape(-1, 4)), S._up(_exclusive(words))
        d_bits = S._up(np.concatenate(packed) if len(packed) else np.zeros(4, np.uint8))
        S.capi.check(S.L.sdsm_measure_objects_multi(S.table, self.n_im, n, S._p(d_image), S._p(d_boxes), S._p(d_off), S._p(d_bits), S._p(self.d_g),
                                                    S._p(self.d_gmax), S._p(self.d_exp), S._p(d_out), S._stream()), 'sdsm_measure_objects_multi')
        return self._records(d_out, n)

    def label_range(self, d_labels):
        S = self.S
        d_range = S.torch.empty(2 * self.n_im, dtype=S.torch.int32, device=S.dev)
        S.capi.check(S.L.sdsm_render_label_range_multi(S.table, self.n_im, S._p(d_labels), None, None, None, S._p(d_range), None, S._stream()),
                     'sdsm_render_label_range_multi')
        return d_range.cpu().numpy().reshape(-1, 2)

    def labels(self, labels, n_labels=None, d_out=None):
        """The records of the labels 0 .. n_labels[i] - 1 of every image (``n_labels`` None: up to each image's highest label, found on the
        device), one array per image, and per image the number of pixels with a label outside that range (they are skipped).  ``d_out``:
        a record buffer of the caller's (its contents do not matter: the call clears it)."""
        S = self.S
        d_labels = S.pack(labels, np.int32)
        if n_labels is None:
            rng = self.label_range(d_labels)
            if (rng[:, 0] < 0).any() or (rng[:, 1] >= _capi.MEASURE_MAX_LABELS).any():
                raise ValueError(f'labels {rng[:, 0].min()} .. {rng[:, 1].max()}: the measurement tables take the labels 0 .. {_capi.MEASURE_MAX_LABELS - 1}, '
                                 'see DESIGN.md "Limits"')
            n_labels = rng[:, 1] + 1
        n_labels = np.asarray(n_labels, np.int64)
        rec_off = _exclusive(n_labels)
        total = int(n_labels.sum())
        d_out = self.record_buffer(total) if d_out is None else d_out
        d_bad = S.torch.empty(self.n_im, dtype=S.torch.int32, device=S.dev)
        S.capi.check(S.L.sdsm_measure_labels_multi(S.table, self.n_im, S._p(d_labels), (S.C.c_int64 * self.n_im)(*[int(v) for v in rec_off]),
                                                   (S.C.c_int32 * self.n_im)(*[int(v) for v in n_labels]), S._p(self.d_g), S._p(self.d_gmax), S._p(self.d_exp),
                                                   S._p(d_out), S._p(d_bad), S._stream()), 'sdsm_measure_labels_multi')
        recs = self._records(d_out, total)
        return [recs[o:o + n] for o, n in zip(rec_off, n_labels)], d_bad.cpu().numpy()

    def scale_exponents(self):
        """``e`` per image as the device found it (0 without intensities)."""
        return self.d_exp.cpu().numpy()


def _intensities(intensities, shapes):
    if intensities is None:
        return None
    intensities = list(intensities)
    if len(intensities) != len(shapes) or any(g is None for g in intensities):
        raise ValueError('intensities: None, or one image per label map / list of objects')
    return [_check_intensity(g, s) for g, s in zip(intensities, shapes)]


def measure_objects_many(objects_per_image, shapes, intensities=None):
    """:func:`measure_objects` for a list of images: one launch per ``_capi.MAX_SET_IMAGES`` images (larger lists are split).  Per image
    the bytes of :func:`measure_objects_host`."""
    objs = [list(o) for o in objects_per_image]
    shapes = [_check_shape(s) for s in shapes]
    if len(shapes) != len(objs):
        raise ValueError('shapes: one per list of objects')
    for o, s in zip(objs, shapes):
        _check_boxes(_object_boxes(o), s)
    gs = _intensities(intensities, shapes)
    out = []
    for part in in_sets(len(objs)):
        packs = [pack_fragments(o) for o in objs[part]]
        M = _MeasureSet(shapes[part], gs[part] if gs is not None else None)
        recs = M.objects(np.concatenate([np.full(len(pk[0]), i, np.int32) for i, pk in enumerate(packs)]), np.concatenate([pk[0] for pk in packs]),
                         np.concatenate([pk[1] for pk in packs]), [b for pk in packs for b in pk[2]])
        first = _exclusive([len(pk[0]) for pk in packs] + [0])
        out += [_as_table(recs[first[i]:first[i] + len(pk[0])], np.arange(len(pk[0]))) for i, pk in enumerate(packs)]
    return out


def measure_objects(objects, shape, intensity=None):
    """The table of a list of objects (``fg_offset``, ``fg_fragment``; they may overlap) of an image of ``shape`` on the GPU, one
    workgroup per object; row k is object k.  ``intensity``: an image of that shape, or None."""
    return measure_objects_many([objects], [shape], [intensity] if intensity is not None else None)[0]


def measure_labels_many(labels_list, intensities=None, background_label=0, n_labels=None):
    """:func:`measure_labels` for a list of label maps, one launch per ``_capi.MAX_SET_IMAGES`` images.  ``n_labels``: None, or per image
    the number of labels 0 .. n - 1 the caller vouches for (a label outside raises ``ValueError``)."""
    from .render import _int32_labels
    labels_list = [_check_labels(l) for l in labels_list]
    gs = _intensities(intensities, [l.shape for l in labels_list])
    l32 = [_int32_labels(l) for l in labels_list]
    if n_labels is not None:
        n_labels = [int(n) for n in n_labels]
        if len(n_labels) != len(l32) or not all(1 <= n <= _capi.MEASURE_MAX_LABELS for n in n_labels):
            raise ValueError(f'n_labels: one count in 1 .. {_capi.MEASURE_MAX_LABELS} per label map, see DESIGN.md "Limits"')
    out = []
    for part in in_sets(len(l32)):
        M = _MeasureSet([l.shape for l in l32[part]], gs[part] if gs is not None else None)
        recs, bad = M.labels(l32[part], n_labels[part] if n_labels is not None else None)
        if bad.any():
            raise ValueError(f'{int(bad.sum())} pixels of images {(part.start + np.nonzero(bad)[0]).tolist()} carry a label outside 0 .. n_labels - 1')
        out += [_present(r, background_label) for r in recs]
    return out


def measure_labels(labels, intensity=None, background_label=0, n_labels=None):
    """The table of a label map (integer, labels 0 .. 65535) on the GPU: the present labels without ``background_label`` (None: all), in
    ascending order.  The highest label is found on the device (sdsm_render_label_range)."""
    return measure_labels_many([labels], [intensity] if intensity is not None else None, background_label, [n_labels] if n_labels is not None else None)[0]


def measure_result(data, objects='postprocessed_objects', intensity='g_raw'):
    """The table of the objects of pipeline data: ``objects`` an output name or a list of objects, ``intensity`` a key of ``data``, an
    image, or None."""
    objs = list(data[objects]) if isinstance(objects, str) else list(objects)
    g = data[intensity] if isinstance(intensity, str) else intensity
    return measure_objects(objs, data['g_raw'].shape, g)


def label_map_rows_many(labels_list):
    """``render.label_map_rows`` for a list of label maps (labels 0 .. 65535, 0 the background), built from their GPU tables."""
    return [rows_from_table(t) for t in measure_labels_many(labels_list, None, 0)]


def label_map_rows_gpu(labels):
    """``render.label_map_rows`` from the GPU table of the label map: one pass over the image instead of one per label.  The existing
    function stays the definition."""
    return label_map_rows_many([labels])[0]
