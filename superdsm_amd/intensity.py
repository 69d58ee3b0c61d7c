"""Intensity distribution tables: standard deviation, median, quantiles and median absolute deviation of the intensities of the objects
of a segmentation, from objects (bit-packed fragments, which may overlap; each is measured alone) or from label maps, for one image or a
set of images.

This is the second pass that :mod:`measure` leaves out: its table has a sum, a minimum and a maximum per object and nothing about how the
intensities are distributed.  As there, a result holds per object or label one row of EXACT values (``sdsm_intensity_record``,
include/sdsm.h) -- integer sums, and order statistics, which are elements of the input --, the GPU forms (sdsm_intensity.hip) give the
bytes of the ``*_host`` definitions below, and every float that is not an element of the input is made in ONE place, :func:`derive`.
All of it is over the FINITE intensities of an object's pixels; -0.0 reads +0.0.

  area, n_finite, gmin, gmax     as in ``measure``; +inf / -inf without a finite pixel
  range_exp e                    d = gmax - gmin in float64; the smallest exponent with d < 2^e, clamped to -960 .. 1024; 0 when d == 0
  sum_p, sum_pp_lo, sum_pp_hi    a finite pixel adds p = rint(ldexp(g - gmin, 30 - e)) (one IEEE subtraction, ties to even, 0 <= p <= 2^30)
                                 to sum_p, bits 0 .. 31 of p^2 to sum_pp_lo and p^2 >> 32 to sum_pp_hi.  Integer sums: no order, and the
                                 variance (n S2 - (sum p)^2) / n^2 * 4^(e - 30) is taken in Python integers, so nothing cancels.
  med_lo, med_hi                 the order statistics at the two ranks of the quantile 1 / 2; med = 0.5 med_lo + 0.5 med_hi
  mad_lo, mad_hi                 the same two order statistics of the keys |g - med| (one IEEE subtraction each, +inf where it overflows)
  flags                          bit 0: the bounding box of the pixels touches the image frame; bit 1: a non-finite pixel inside; bit 2:
                                 no finite pixel; bit 3: gmax - gmin is not finite (then e = 1024 and the three sums stay 0)

A result is ``(table, order)``: ``order[k, q]`` holds the two order statistics ``v_lo, v_hi`` of quantile q of row k -- the elements at
the ranks lo and hi of the sorted finite intensities, where for n = n_finite and the quantile num / den (the nearest fraction with
den <= 10^6) h = (n - 1) num, lo = h div den, rem = h mod den, hi = lo + (rem != 0).  Without a finite pixel both are the quiet NaN.

**Accuracy** of the derived columns.  The root of the variance differs from the exact population standard deviation of the doubles by
less than 2^(e - 30): quantisation moves a pixel by at most half a unit 2^(e - 30) and the subtraction by at most 2^(e - 54), and the
standard deviation is a seminorm of the centred vector, so these errors add at most linearly.  A derived quantile,
``v_lo + (v_hi - v_lo) * (rem / den)``, is four roundings of values <= 2 max(|v_lo|, |v_hi|): within 4 ulp of that maximum of the
exact rational interpolation (where v_hi - v_lo does not overflow); it is not promised to be bit-identical to ``np.quantile``."""
import csv
import math
from fractions import Fraction
from functools import partial

import numpy as np

from . import _capi
from .measure import (SCALE_EXP_MAX, SCALE_EXP_MIN, _check_labels, _check_shape, _keep_absent, _label_count, _label_sets, _label_table, _LabelWindows,
                      _MeasureSet, _object_boxes, _object_sets, _require_intensity, _result_inputs)
from .postprocess import _check_boxes

TABLE_DTYPE = np.dtype([('label', 'i4')] + _capi._INTENSITY_FIELDS)   # 'label': the label, or the index of the object in its image
DEFAULT_QUANTILES = (0.25, 0.5, 0.75)
QUIET_NAN = np.array([0x7ff8000000000000], np.uint64).view(np.float64)[0]
FRAME, NONFINITE_INSIDE, NO_FINITE_PIXEL, RANGE_NOT_FINITE = 1, 2, 4, 8           # the flag bits


# ---- the definitions: NumPy and Python integers ---------------------------------------------------------------------------------------
def quantile_fractions(quantiles):
    """The quantiles as (num, den) with den <= 10^6: each the nearest such fraction (the rule of ``compare.scores``)."""
    qs = [float(q) for q in quantiles]
    if len(qs) > _capi.INTENSITY_MAX_QUANTILES:
        raise ValueError(f'{len(qs)} quantiles: the intensity tables take up to {_capi.INTENSITY_MAX_QUANTILES} per call, see DESIGN.md "Limits"')
    if any(not 0 <= q <= 1 for q in qs):
        raise ValueError(f'quantiles {tuple(qs)}: 0 <= q <= 1 required')
    fr = [Fraction(q).limit_denominator(_capi.INTENSITY_MAX_DEN) for q in qs]
    return [(f.numerator, f.denominator) for f in fr]


def quantile_ranks(n, num, den):
    """(lo, hi, rem) of the quantile num / den of n >= 1 sorted values, in Python integers (``sdsm_quantile_ranks``)."""
    lo, rem = divmod((int(n) - 1) * int(num), int(den))
    return lo, lo + (rem != 0), rem


def range_exponent(d):
    """``e`` of a finite range d >= 0: the smallest exponent with d < 2^e, clamped to -960 .. 1024; 0 for d == 0."""
    return 0 if d == 0 else min(SCALE_EXP_MAX, max(SCALE_EXP_MIN, math.frexp(float(d))[1]))


def _empty_records(n):
    recs = np.zeros(n, _capi.INTENSITY_RECORD_DTYPE)
    recs['gmin'], recs['gmax'], recs['flags'] = np.inf, -np.inf, NO_FINITE_PIXEL
    for name in ('med_lo', 'med_hi', 'mad_lo', 'mad_hi'):
        recs[name] = QUIET_NAN
    return recs


def _fill_record(rec, order, rr, cc, shape, g, fracs):
    """The record and the order statistics of the pixels (rr, cc) -- image coordinates -- of an image of ``shape`` with the intensities g."""
    if len(rr) == 0:
        return
    r, c = np.asarray(rr).astype(np.int64), np.asarray(cc).astype(np.int64)
    rec['area'] = len(r)
    flags = FRAME * int(r.min() == 0 or c.min() == 0 or r.max() + 1 == shape[0] or c.max() + 1 == shape[1])
    vals = g[r, c]
    fin = np.isfinite(vals)
    v = np.sort(vals[fin]) + 0.0                                              # (-0.0 + 0.0 = +0.0)
    n = len(v)
    flags |= NONFINITE_INSIDE * int(not fin.all())
    if n == 0:
        rec['flags'] = flags | NO_FINITE_PIXEL
        return
    rec['n_finite'], rec['gmin'], rec['gmax'] = n, v[0], v[-1]
    with np.errstate(over='ignore'):
        d = v[-1] - v[0]
    if not np.isfinite(d):
        flags |= RANGE_NOT_FINITE
        rec['range_exp'] = SCALE_EXP_MAX
    else:
        e = range_exponent(d)
        p = [int(x) for x in np.rint(np.ldexp(v - v[0], 30 - e))]             # Python integers from here on
        rec['range_exp'], rec['sum_p'] = e, sum(p)
        rec['sum_pp_lo'], rec['sum_pp_hi'] = sum((x * x) & 0xffffffff for x in p), sum((x * x) >> 32 for x in p)
    for q, (num, den) in enumerate(fracs):
        lo, hi, _ = quantile_ranks(n, num, den)
        order[q] = v[lo], v[hi]
    lo, hi, _ = quantile_ranks(n, 1, 2)
    med = 0.5 * v[lo] + 0.5 * v[hi]                                           # two products, one sum
    with np.errstate(over='ignore'):
        keys = np.sort(np.abs(v - med))
    rec['med_lo'], rec['med_hi'], rec['mad_lo'], rec['mad_hi'], rec['flags'] = v[lo], v[hi], keys[lo], keys[hi], flags


_table = partial(_label_table, TABLE_DTYPE)                           # _table(labels, recs)


def _empty_order(n, n_q):
    return np.full((n, n_q, 2), QUIET_NAN, np.float64)


def intensity_objects_host(objects, shape, intensity, quantiles=DEFAULT_QUANTILES):
    """``(table, order)`` of a list of objects (``fg_offset``, ``fg_fragment``) of an image of ``shape`` with the intensities
    ``intensity``, object by object; row k is object k.  Objects may overlap: each is measured alone."""
    shape = _check_shape(shape)
    objects = list(objects)
    _check_boxes(_object_boxes(objects), shape)
    g = _require_intensity(intensity, shape)
    fracs = quantile_fractions(quantiles)
    recs, order = _empty_records(len(objects)), _empty_order(len(objects), len(fracs))
    for k, obj in enumerate(objects):
        rr, cc = np.nonzero(np.asarray(obj.fg_fragment, bool))
        _fill_record(recs[k:k + 1], order[k], rr + int(obj.fg_offset[0]), cc + int(obj.fg_offset[1]), shape, g, fracs)
    return _table(np.arange(len(objects)), recs), order


def intensity_labels_host(labels, intensity, quantiles=DEFAULT_QUANTILES, background_label=0, keep_absent=False):
    """``(table, order)`` of a label map, label by label: the present labels without ``background_label`` (None: all) in ascending order;
    with ``keep_absent`` one row per label 0 .. max, the empty row for an absent label and for the background label."""
    labels = _check_labels(labels)
    g = _require_intensity(intensity, labels.shape)
    fracs = quantile_fractions(quantiles)
    n = _label_count(labels)
    recs, order = _empty_records(n), _empty_order(n, len(fracs))
    for l in sorted(frozenset(labels.reshape(-1).tolist())):
        if l != background_label:
            rr, cc = np.nonzero(labels == l)
            _fill_record(recs[l:l + 1], order[l], rr, cc, labels.shape, g, fracs)
    ls = np.arange(n) if keep_absent else np.nonzero(recs['area'] > 0)[0]
    return _table(ls, recs[ls]), order[ls]


# ---- derived columns: one function for the host and the GPU forms ----------------------------------------------------------------------
_DERIVED_HEAD = [('label', 'i4'), ('area', 'i8'), ('n_finite', 'i8'), ('on_boundary', '?'), ('nonfinite_inside', '?'), ('range_not_finite', '?'),
                 ('min_intensity', 'f8'), ('max_intensity', 'f8'), ('mean_intensity', 'f8'), ('std_intensity', 'f8'), ('variance', 'f8'), ('median', 'f8')]


def quantile_names(quantiles):
    """The column of every quantile in :func:`derive`: ``q0.25``, ``q0.5``, ``q0.333333`` ..."""
    names = [f'q{float(Fraction(num, den)):.6g}' for num, den in quantile_fractions(quantiles)]
    if len(set(names)) != len(names):
        raise ValueError(f'quantiles {tuple(quantiles)}: a quantile is named twice')
    return names


def derived_dtype(quantiles=DEFAULT_QUANTILES):
    fr = quantile_fractions(quantiles)
    return np.dtype(_DERIVED_HEAD + [(n, 'f8') for n in quantile_names(quantiles)] + ([('iqr', 'f8')] if (1, 4) in fr and (3, 4) in fr else []) + [('mad', 'f8')])


def variance_exact(row):
    """The variance of a row in units of 4^(e - 30), as the exact rational (n S2 - (sum p)^2) / n^2."""
    n, sp = int(row['n_finite']), int(row['sum_p'])
    return Fraction(n * (int(row['sum_pp_hi']) * 2 ** 32 + int(row['sum_pp_lo'])) - sp * sp, n * n)


def _scaled(x, e):
    try:
        return math.ldexp(x, e)
    except OverflowError:
        return math.copysign(math.inf, x)


def derive(table, order, quantiles=DEFAULT_QUANTILES):
    """The derived columns of a result (:func:`derived_dtype`), on the host from its exact values: ``std_intensity`` and ``variance``
    (the differences in Python integers), ``mean_intensity`` = gmin + (sum p) / n * 2^(e - 30), ``median``, one column per quantile,
    ``iqr`` when 0.25 and 0.75 are among them, ``mad``.  Rows without a finite pixel read NaN; so do mean, standard deviation and
    variance of a row whose range is not finite."""
    fracs = quantile_fractions(quantiles)
    names = quantile_names(quantiles)
    order = np.asarray(order, np.float64)
    if order.shape != (len(table), len(fracs), 2):
        raise ValueError(f'order: {(len(table), len(fracs), 2)} expected for this table and these quantiles, got {order.shape}')
    out = np.zeros(len(table), derived_dtype(quantiles))
    for name in out.dtype.names[6:]:
        out[name] = np.nan
    out['label'], out['area'], out['n_finite'] = table['label'], table['area'], table['n_finite']
    out['on_boundary'], out['nonfinite_inside'], out['range_not_finite'] = ((table['flags'] & b) != 0 for b in (FRAME, NONFINITE_INSIDE, RANGE_NOT_FINITE))
    for k, row in enumerate(table):
        n, e = int(row['n_finite']), int(row['range_exp'])
        if n == 0:
            continue
        o = out[k:k + 1]
        o['min_intensity'], o['max_intensity'] = row['gmin'], row['gmax']
        if not row['flags'] & RANGE_NOT_FINITE:
            var = float(variance_exact(row))
            o['variance'], o['std_intensity'] = _scaled(var, 2 * (e - 30)), _scaled(math.sqrt(var), e - 30)
            o['mean_intensity'] = float(row['gmin']) + _scaled(float(Fraction(int(row['sum_p']), n)), e - 30)
        with np.errstate(over='ignore', invalid='ignore'):
            o['median'] = 0.5 * row['med_lo'] + 0.5 * row['med_hi']
            o['mad'] = 0.5 * row['mad_lo'] + 0.5 * row['mad_hi']
            for q, (name, (num, den)) in enumerate(zip(names, fracs)):
                v_lo, v_hi = order[k, q]
                o[name] = v_lo + (v_hi - v_lo) * (quantile_ranks(n, num, den)[2] / den)
    if 'iqr' in out.dtype.names:
        with np.errstate(over='ignore', invalid='ignore'):
            out['iqr'] = out[names[fracs.index((3, 4))]] - out[names[fracs.index((1, 4))]]
    return out


def write_intensity_csv(path, table, order, quantiles=DEFAULT_QUANTILES):
    """A result with its derived columns as CSV, every field quoted (as ``measure.write_measurements_csv``); after the derived columns
    the exact ones: the record's integers, and per quantile its two order statistics."""
    d = derive(table, order, quantiles)
    names = quantile_names(quantiles)
    exact = ['range_exp', 'sum_p', 'sum_pp_lo', 'sum_pp_hi', 'med_lo', 'med_hi', 'mad_lo', 'mad_hi']
    with open(path, 'w', newline='') as fp:
        w = csv.writer(fp, delimiter=',', quoting=csv.QUOTE_ALL)
        w.writerow(list(d.dtype.names) + exact + [f'{n}_{side}' for n in names for side in ('lo', 'hi')])
        for k, (drow, row) in enumerate(zip(d, table)):
            w.writerow([repr(v.item()) for v in drow] + [repr(row[n].item()) for n in exact] + [repr(float(v)) for v in np.asarray(order[k]).reshape(-1)])


# ---- the GPU forms (sdsm_intensity.hip) -----------------------------------------------------------------------------------------------
class _IntensitySet:
    """One set of up to ``_capi.MAX_SET_IMAGES`` images with their intensities on the current device and the two calls of the intensity
    kernel."""

    def __init__(self, shapes, intensities):
        self.M = _MeasureSet(shapes, intensities)     # (the intensities packed; the label form takes the boxes of the labels from there)
        self.S = self.M.S
        self.n_im = len(self.S.shapes)

    def buffers(self, n, n_q):
        """The two outputs of a call; their contents do not matter."""
        S = self.S
        return dict(d_out=S.record_buffer(n, _capi.INTENSITY_RECORD_DTYPE), d_order=S.torch.empty(max(1, n * n_q * 2), dtype=S.torch.float64, device=S.dev))

    def _quantiles(self, fracs):
        C = self.S.C
        return len(fracs), (C.c_int32 * max(1, len(fracs)))(*[f[0] for f in fracs]), (C.c_int32 * max(1, len(fracs)))(*[f[1] for f in fracs])

    def _download(self, B, n, n_q):
        return self.S.records(B['d_out'], n, _capi.INTENSITY_RECORD_DTYPE), B['d_order'].cpu().numpy()[:n * n_q * 2].reshape(n, n_q, 2).copy()

    def objects(self, obj_image, boxes, words, packed, fracs, B=None):
        """(records, order) of the objects of the set (``packed``: the bit-packed fragments, one uint8 array of whole words each)."""
        S, n = self.S, len(boxes)
        n_q, num, den = self._quantiles(fracs)
        B = self.buffers(n, n_q) if B is None else B
        d_objects = S.upload_objects(obj_image, boxes, words, packed)
        S.capi.check(S.L.sdsm_intensity_objects_multi(S.table, self.n_im, n, *map(S._p, d_objects), S._p(self.M.d_g), n_q, num, den, S._p(B['d_out']),
                                                      S._p(B['d_order']), S._stream()), 'sdsm_intensity_objects_multi')
        return self._download(B, n, n_q)

    def labels(self, labels, background_label, fracs):
        """Per image (labels measured, number of labels, records, order) of the label maps of the set: the windows of the labels
        (``measure._LabelWindows``), then sdsm_intensity_labels."""
        S = self.S
        w = _LabelWindows(self.M, labels, background_label, 'intensity')
        n = len(w.idx)
        n_q, num, den = self._quantiles(fracs)
        B = self.buffers(n, n_q)
        S.capi.check(S.L.sdsm_intensity_labels_multi(S.table, self.n_im, *w.args(), S._p(self.M.d_g), n_q, num, den, S._p(B['d_out']), S._p(B['d_order']),
                                                     S._p(w.d_bad), S._stream()), 'sdsm_intensity_labels_multi')
        recs, order = self._download(B, n, n_q)
        return [(ls, n_labels, recs[a:b], order[a:b]) for ls, n_labels, a, b in w.per_image()]


def intensity_objects_many(objects_per_image, shapes, intensities, quantiles=DEFAULT_QUANTILES):
    """:func:`intensity_objects` for a list of images: one launch per ``_capi.MAX_SET_IMAGES`` images (larger lists are split).  Per image
    the bytes of :func:`intensity_objects_host`."""
    sets = _object_sets(objects_per_image, shapes, intensities, required=True)
    fracs = quantile_fractions(quantiles)
    out = []
    for _, shapes_part, gs, packed, first in sets:
        recs, order = _IntensitySet(shapes_part, gs).objects(*packed, fracs)
        out += [(_table(np.arange(b - a), recs[a:b]), order[a:b]) for a, b in zip(first[:-1], first[1:])]
    return out


def intensity_objects(objects, shape, intensity, quantiles=DEFAULT_QUANTILES):
    """``(table, order)`` of a list of objects (``fg_offset``, ``fg_fragment``; they may overlap) of an image of ``shape`` with the
    intensities ``intensity`` on the GPU, one workgroup per object; row k is object k.  The bytes of :func:`intensity_objects_host`."""
    return intensity_objects_many([objects], [shape], [intensity], quantiles)[0]


def intensity_labels_many(labels_list, intensities, quantiles=DEFAULT_QUANTILES, background_label=0, keep_absent=False):
    """:func:`intensity_labels` for a list of label maps, one launch per ``_capi.MAX_SET_IMAGES`` images."""
    sets = _label_sets(labels_list, intensities, required=True)
    fracs = quantile_fractions(quantiles)
    out = []
    for _, l32, shapes, gs in sets:
        for ls, n_labels, recs, order in _IntensitySet(shapes, gs).labels(l32, background_label, fracs):
            if keep_absent:
                full_order = _empty_order(n_labels, len(fracs))
                full_order[ls] = order
                (ls, recs), order = _keep_absent(_empty_records(n_labels), ls, recs), full_order
            out.append((_table(ls, recs), order))
    return out


def intensity_labels(labels, intensity, quantiles=DEFAULT_QUANTILES, background_label=0, keep_absent=False):
    """``(table, order)`` of a label map (integer, labels 0 .. 65535) on the GPU: the present labels without ``background_label`` (None:
    all) in ascending order, or with ``keep_absent`` one row per label 0 .. max.  The bytes of :func:`intensity_labels_host`."""
    return intensity_labels_many([labels], [intensity], quantiles, background_label, keep_absent)[0]


def intensity_result(data, objects='postprocessed_objects', intensity='g_raw', quantiles=DEFAULT_QUANTILES):
    """The intensity table of the objects of pipeline data: ``objects`` an output name or a list of objects, ``intensity`` a key of
    ``data`` or an image."""
    return intensity_objects(*_result_inputs(data, objects, intensity), quantiles)
