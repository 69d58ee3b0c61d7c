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
from .postprocess import _check_boxes, _exclusive, pack_object_sets

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


def _require_intensity(intensity, shape):
    if intensity is None:
        raise ValueError('intensity: the intensity tables need an image')
    return _check_intensity(intensity, shape)


def _check_shape(shape):
    shape = tuple(int(v) for v in shape)
    if len(shape) != 2 or min(shape) < 1 or max(shape) > 65535 or shape[0] * shape[1] >= 2 ** 31 - 1:
        raise ValueError(f'shape {shape}: the measurement tables take H x W images with H, W <= 65535 and H * W < 2^31, see DESIGN.md "Limits"')
    return shape


def _object_boxes(objects):
    return np.array([(int(o.fg_offset[0]), int(o.fg_offset[1])) + tuple(o.fg_fragment.shape) for o in objects], np.int64).reshape(-1, 4)


def _label_table(dtype, labels, recs):
    """The table of ``dtype`` -- a 'label' column in front of the fields of the records -- of the records ``recs`` of ``labels``."""
    table = np.zeros(len(recs), dtype)
    table['label'] = labels
    for name in dtype.names[1:]:
        table[name] = recs[name]
    return table


def _as_table(recs, labels):
    return _label_table(TABLE_DTYPE, labels, recs)


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
        return self.S.records(d_out, n, _capi.MEASURE_RECORD_DTYPE)

    def record_buffer(self, n):
        return self.S.record_buffer(n, _capi.MEASURE_RECORD_DTYPE)

    def objects(self, obj_image, boxes, words, packed):
        """The records of the objects of the set (``packed``: the bit-packed fragments, one uint8 array of whole words each)."""
        S, n = self.S, len(boxes)
        d_out = self.record_buffer(n)
        d_objects = S.upload_objects(obj_image, boxes, words, packed)
        S.capi.check(S.L.sdsm_measure_objects_multi(S.table, self.n_im, n, *map(S._p, d_objects), S._p(self.d_g), S._p(self.d_gmax), S._p(self.d_exp),
                                                    S._p(d_out), S._stream()), 'sdsm_measure_objects_multi')
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


class _LabelWindows:
    """The windows of the labels of a set of label maps (``M``: its ``_MeasureSet``), as the label forms of the shape, intensity, texture
    and depth tables take them: the boxes of the present labels without ``background_label`` from sdsm_measure_labels (one download),
    one window of ceil(h w / 32) words per label, and the device arrays that name them.  Raises before any kernel of the caller's is
    launched where the labels or the windows pass the limits."""

    def __init__(self, M, labels, background_label, what):
        S = self.S = M.S
        n_im = self.n_im = len(S.shapes)
        self.d_labels = S.pack(labels, np.int32)
        rng = M.label_range(self.d_labels)
        if (rng[:, 0] < 0).any() or (rng[:, 1] >= _capi.MEASURE_MAX_LABELS).any():
            raise ValueError(f'labels {rng[:, 0].min()} .. {rng[:, 1].max()}: the {what} tables take the labels 0 .. {_capi.MEASURE_MAX_LABELS - 1}, '
                             'see DESIGN.md "Limits"')
        self.n_labels = n_labels = (rng[:, 1] + 1).astype(np.int64)
        self.rec_off = rec_off = _exclusive(n_labels)
        self.c_off, self.c_n = (S.C.c_int64 * n_im)(*[int(v) for v in rec_off]), (S.C.c_int32 * n_im)(*[int(v) for v in n_labels])
        self.d_bad = S.torch.empty(n_im, dtype=S.torch.int32, device=S.dev)
        d_rec = M.record_buffer(int(n_labels.sum()))
        S.capi.check(S.L.sdsm_measure_labels_multi(S.table, n_im, S._p(self.d_labels), self.c_off, self.c_n, None, None, None, S._p(d_rec), S._p(self.d_bad),
                                                   S._stream()), 'sdsm_measure_labels_multi')
        mrec = M._records(d_rec, int(n_labels.sum()))
        keep = mrec['area'] > 0
        if background_label is not None:
            for i in range(n_im):
                if 0 <= background_label < n_labels[i]:
                    keep[rec_off[i] + background_label] = False
        self.idx = idx = np.nonzero(keep)[0]
        self.boxes = boxes = np.stack([mrec['r0'][idx], mrec['c0'][idx], mrec['r1'][idx] - mrec['r0'][idx], mrec['c1'][idx] - mrec['c0'][idx]], axis=1).astype(np.int32)
        self.obj_image = obj_image = (np.searchsorted(rec_off, idx, side='right') - 1).astype(np.int32)
        words = (boxes[:, 2].astype(np.int64) * boxes[:, 3] + 31) // 32
        self.total = total = int(words.sum())
        if total > _capi.SHAPE_MAX_WINDOW_WORDS:                               # (nothing of the caller's kernels has been launched)
            raise ValueError(f'the windows of the labels take {total} words: the label form of the {what} tables takes up to {_capi.SHAPE_MAX_WINDOW_WORDS} '
                             'per set, see DESIGN.md "Limits"')
        label_obj = np.full(int(n_labels.sum()), -1, np.int32)
        label_obj[idx] = np.arange(len(idx), dtype=np.int32)
        self.d_label_obj = S._up(label_obj)
        self.d_image, self.d_boxes, self.d_off, self.d_bits = S.upload_objects(obj_image, boxes, words, None)      # (the call fills the windows)

    def args(self):
        """The ten arguments that follow the image table in every ``sdsm_*_labels_multi`` call: d_labels, rec_off, n_labels, d_label_obj,
        n, d_obj_image, d_boxes, d_bits_off, window_words, d_bits."""
        p = self.S._p
        return p(self.d_labels), self.c_off, self.c_n, p(self.d_label_obj), len(self.idx), p(self.d_image), p(self.d_boxes), p(self.d_off), self.total, p(self.d_bits)

    def per_image(self):
        """Per image (labels measured, number of labels, first window, end of its windows)."""
        first = np.searchsorted(self.obj_image, np.arange(self.n_im + 1))
        return [((self.idx[a:b] - self.rec_off[i]).astype(np.int64), int(self.n_labels[i]), a, b) for i, (a, b) in enumerate(zip(first[:-1], first[1:]))]


# ---- what the GPU forms of the table families share in front of their sets (shape, intensity, texture and depth import it from here) ----
def _intensities(intensities, shapes, required=False):
    """One checked float64 image per shape.  ``required``: the family needs them (intensity, texture); otherwise (measure, depth) None
    stands for no intensities at all and is returned."""
    if intensities is None and not required:
        return None
    intensities = [] if intensities is None else list(intensities)
    if len(intensities) != len(shapes) or (not required and any(g is None for g in intensities)):
        raise ValueError('intensities: ' + ('' if required else 'None, or ') + 'one image per label map / list of objects')
    return [_require_intensity(g, s) for g, s in zip(intensities, shapes)]


def _object_sets(objects_per_image, shapes, intensities=None, required=False):
    """The front of every ``*_objects_many``: the lists checked -- all of them, before anything touches the device --, then per set of up
    to ``_capi.MAX_SET_IMAGES`` images ``(part, shapes, intensities or None, packed, first)``: its slice of the lists, the packed objects
    and the split by image of ``postprocess.pack_object_sets``.  A set is packed when the caller's loop comes to it."""
    objs = [list(o) for o in objects_per_image]
    shapes = [_check_shape(s) for s in shapes]
    if len(shapes) != len(objs):
        raise ValueError('shapes: one per list of objects')
    for o, s in zip(objs, shapes):
        _check_boxes(_object_boxes(o), s)
    gs = _intensities(intensities, shapes, required)
    return ((part, shapes[part], gs[part] if gs is not None else None) + pack_object_sets(objs[part])[:2] for part in in_sets(len(objs)))


def _label_sets(labels_list, intensities=None, required=False):
    """The front of every ``*_labels_many``: the label maps checked and as int32, then per set ``(part, label maps, shapes, intensities or
    None)``."""
    from .render import _int32_labels
    labels_list = [_check_labels(l) for l in labels_list]
    gs = _intensities(intensities, [l.shape for l in labels_list], required)
    l32 = [_int32_labels(l) for l in labels_list]
    return [(part, l32[part], [l.shape for l in l32[part]], gs[part] if gs is not None else None) for part in in_sets(len(l32))]


def _keep_absent(empty, ls, recs):
    """``keep_absent`` of a label form: (labels, records) with one record per label 0 .. n - 1 -- the n ``empty`` records with the measured
    ``recs`` written at the labels ``ls``."""
    empty[ls] = recs
    return np.arange(len(empty)), empty


def _result_inputs(data, objects, intensity=None):
    """What every ``*_result`` hands on: (objects, shape, intensities) of pipeline data -- ``objects`` an output name or a list of
    objects, ``intensity`` a key of ``data``, an image, or None."""
    objs = list(data[objects]) if isinstance(objects, str) else list(objects)
    g = data[intensity] if isinstance(intensity, str) else intensity
    return objs, data['g_raw'].shape, g


def measure_objects_many(objects_per_image, shapes, intensities=None):
    """:func:`measure_objects` for a list of images: one launch per ``_capi.MAX_SET_IMAGES`` images (larger lists are split).  Per image
    the bytes of :func:`measure_objects_host`."""
    out = []
    for _, shapes_part, gs, packed, first in _object_sets(objects_per_image, shapes, intensities):
        recs = _MeasureSet(shapes_part, gs).objects(*packed)
        out += [_as_table(recs[a:b], np.arange(b - a)) for a, b in zip(first[:-1], first[1:])]
    return out


def measure_objects(objects, shape, intensity=None):
    """The table of a list of objects (``fg_offset``, ``fg_fragment``; they may overlap) of an image of ``shape`` on the GPU, one
    workgroup per object; row k is object k.  ``intensity``: an image of that shape, or None."""
    return measure_objects_many([objects], [shape], [intensity] if intensity is not None else None)[0]


def measure_labels_many(labels_list, intensities=None, background_label=0, n_labels=None):
    """:func:`measure_labels` for a list of label maps, one launch per ``_capi.MAX_SET_IMAGES`` images.  ``n_labels``: None, or per image
    the number of labels 0 .. n - 1 the caller vouches for (a label outside raises ``ValueError``)."""
    labels_list = list(labels_list)
    sets = _label_sets(labels_list, intensities)
    if n_labels is not None:
        n_labels = [int(n) for n in n_labels]
        if len(n_labels) != len(labels_list) or not all(1 <= n <= _capi.MEASURE_MAX_LABELS for n in n_labels):
            raise ValueError(f'n_labels: one count in 1 .. {_capi.MEASURE_MAX_LABELS} per label map, see DESIGN.md "Limits"')
    out = []
    for part, l32, shapes, gs in sets:
        recs, bad = _MeasureSet(shapes, gs).labels(l32, n_labels[part] if n_labels is not None else None)
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
    return measure_objects(*_result_inputs(data, objects, intensity))


def label_map_rows_many(labels_list):
    """``render.label_map_rows`` for a list of label maps (labels 0 .. 65535, 0 the background), built from their GPU tables."""
    return [rows_from_table(t) for t in measure_labels_many(labels_list, None, 0)]


def label_map_rows_gpu(labels):
    """``render.label_map_rows`` from the GPU table of the label map: one pass over the image instead of one per label.  The existing
    function stays the definition."""
    return label_map_rows_many([labels])[0]
