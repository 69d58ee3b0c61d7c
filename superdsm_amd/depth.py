"""Depth tables: the largest inscribed circle, the mean and median radius and the intensity profile from rim to core of the objects of a
segmentation, from objects (bit-packed fragments, which may overlap; each is measured alone) or from label maps, for one image or a set
of images.

The other tables describe an object's size, outline, grey values, their arrangement and its surroundings; this one says how far inside
its object a pixel lies.  As there, a result holds per object or label one row of EXACT integers (``sdsm_depth_record``, include/sdsm.h)
and per shell one more (``sdsm_depth_shell_record``), the GPU forms (sdsm_depth.hip) give the bytes of the ``*_host`` definitions below,
and every float is made in ONE place, :func:`derive`.

An object is the set P of the set bits of its fragment, as in the shape tables.  Everything else is outside P: the rest of its box, other
objects or labels, the outside of the image.  ``d2(p)`` for p in P is the smallest squared Euclidean distance, an integer, from p to a
lattice place outside P.  A place one step beyond the image frame, or beyond the box, counts like any other outside pixel.  So
``d2 >= 1`` for every p in P, and ``d2 <= ceil(min(h, w) / 2)^2`` over the tight box.  Images are H x W with H, W <= 65 535 and
H W < 2^31, so d2 <= 2^30, sum_d2 < 2^61 and sum_q < 2^62: nothing wraps.

  area                      pixels of P
  max_d2                    largest d2: the squared radius of the largest inscribed circle, in the convention above
  max_row, max_col          the pixel with d2 == max_d2 that is smallest in (row, column) order, image coordinates
  n_max                     pixels with d2 == max_d2
  sum_d2                    sum of d2
  sum_q                     sum of q(d2), q = floor(sqrt(d2 2^32)): the distance in units of 2^-16 pixel (``sdsm_quantised_distance``)
  med_d2_lo, med_d2_hi      the order statistics of d2 at the two ranks of the quantile 1 / 2 (``intensity.quantile_ranks(area, 1, 2)``)
  n_rim                     pixels with d2 == 1; ``border_pixels`` of the shape tables
  flags                     bit 0: the bounding box of P touches the image frame
  scale_exp                 e of the image's intensities as in :mod:`measure`; 0 without an intensity image and in the zero row

A result is ``(table, shells)``: ``shells[k, s]`` is the row of shell s of table row k.  With ``n_shells`` = S, 1 <= S <= 32, the shell of
a pixel is ``min(S - 1, isqrt(d2 - 1))``, that is ceil(sqrt(d2)) - 1 capped: shell 0 holds d2 == 1, shell 1 d2 in 2 .. 4, shell 2 d2 in
5 .. 9; the last shell collects every deeper pixel.

  count                     pixels of the shell
  n_finite                  those with a finite intensity
  gsum_lo, gsum_hi          the two limbs of the sum of rint(ldexp(g, 62 - e)) over the finite pixels, as in :mod:`measure`

The intensity image is optional: without it only ``count`` is filled.  A non-finite pixel is counted in ``count``, not in ``n_finite``,
and adds nothing to the sums.  An object without a pixel has the zero row and zero shells."""
import csv
import math
from fractions import Fraction
from functools import partial

import numpy as np

from . import _capi
from .intensity import quantile_ranks
from .measure import (_check_intensity, _check_labels, _check_shape, _keep_absent, _label_count, _label_sets, _label_table, _LabelWindows, _MeasureSet,
                      _object_boxes, _object_sets, _result_inputs, _scaled, quantize, scale_exponent)
from .postprocess import _check_boxes, _exclusive

TABLE_DTYPE = np.dtype([('label', 'i4')] + _capi._DEPTH_FIELDS)        # 'label': the label, or the index of the object in its image
DEFAULT_SHELLS = 8
FRAME = 1                                                              # the flag bit


# ---- the definitions: NumPy, SciPy's exact distance transform and Python integers --------------------------------------------------------
def check_shells(n_shells):
    n_shells = int(n_shells)
    if not 1 <= n_shells <= _capi.DEPTH_MAX_SHELLS:
        raise ValueError(f'n_shells {n_shells}: the depth tables take 1 .. {_capi.DEPTH_MAX_SHELLS} shells, see DESIGN.md "Limits"')
    return n_shells


def shell_of(d2, n_shells):
    """The shell of the squared depth d2 >= 1 (``sdsm_depth_shell``), in Python integers."""
    return min(int(n_shells) - 1, math.isqrt(int(d2) - 1))


def squared_depth(mask):
    """``d2`` of every pixel of a boolean fragment (0 outside the object): SciPy's exact Euclidean distance transform of the fragment
    padded by one ring of outside pixels -- a place further out is never nearer than its projection onto the ring."""
    from scipy import ndimage
    mask = np.asarray(mask, bool)
    dist = ndimage.distance_transform_edt(np.pad(mask, 1))[1:-1, 1:-1]
    sq = dist * dist
    d2 = np.rint(sq).astype(np.int64)
    assert np.abs(sq - d2).max(initial=0.0) < 1e-3, 'the squares of the distances are integers up to rounding'
    return d2


def _zero(n, n_shells):
    return np.zeros(n, _capi.DEPTH_RECORD_DTYPE), np.zeros((n, n_shells), _capi.DEPTH_SHELL_DTYPE)


def _fill_record(rec, shells, mask, offset, shape, g, e):
    """The record and the shell rows of the object with the fragment ``mask`` at ``offset`` of an image of ``shape`` with the intensities g
    (or None) of scale exponent e."""
    mask = np.asarray(mask, bool)
    rr, cc = np.nonzero(mask)                                                 # (row, column) order
    if len(rr) == 0:
        return
    d2 = squared_depth(mask)[rr, cc]
    r, c = rr + int(offset[0]), cc + int(offset[1])
    k = int(np.argmax(d2))                                                    # the first of the maxima
    values, counts = np.unique(d2, return_counts=True)
    order = np.sort(d2)
    lo, hi, _ = quantile_ranks(len(d2), 1, 2)
    rec['area'], rec['max_d2'], rec['max_row'], rec['max_col'] = len(d2), d2[k], r[k], c[k]
    rec['n_max'], rec['n_rim'] = int((d2 == d2[k]).sum()), int((d2 == 1).sum())
    rec['sum_d2'] = sum(int(v) * int(n) for v, n in zip(values, counts))      # Python integers
    rec['sum_q'] = sum(math.isqrt(int(v) << 32) * int(n) for v, n in zip(values, counts))
    rec['med_d2_lo'], rec['med_d2_hi'] = order[lo], order[hi]
    rec['flags'] = FRAME * int(r.min() == 0 or c.min() == 0 or r.max() + 1 == shape[0] or c.max() + 1 == shape[1])
    rec['scale_exp'] = e
    n_shells = len(shells)
    shell_of_value = {int(v): shell_of(v, n_shells) for v in values}
    s = np.array([shell_of_value[int(v)] for v in d2], np.int64)
    shells['count'] = np.bincount(s, minlength=n_shells)
    if g is not None:
        vals = g[r, c]
        fin = np.isfinite(vals)
        q = quantize(vals[fin], e)
        shells['n_finite'] = np.bincount(s[fin], minlength=n_shells)
        for t in range(n_shells):
            qt = q[s[fin] == t]
            shells['gsum_lo'][t] = int((qt & 0xffffffff).astype(np.uint64).sum(dtype=np.uint64))
            shells['gsum_hi'][t] = int((qt >> 32).sum(dtype=np.int64))


_table = partial(_label_table, TABLE_DTYPE)                            # _table(labels, recs)


def depth_objects_host(objects, shape, intensity=None, n_shells=DEFAULT_SHELLS):
    """``(table, shells)`` of a list of objects (``fg_offset``, ``fg_fragment``) of an image of ``shape``, object by object; row k is
    object k.  Objects may overlap: each is measured alone.  ``intensity``: an image of that shape, or None."""
    shape = _check_shape(shape)
    objects = list(objects)
    _check_boxes(_object_boxes(objects), shape)
    g = _check_intensity(intensity, shape)
    n_shells = check_shells(n_shells)
    e = scale_exponent(g) if g is not None else 0
    recs, shells = _zero(len(objects), n_shells)
    for k, obj in enumerate(objects):
        _fill_record(recs[k:k + 1], shells[k], obj.fg_fragment, obj.fg_offset, shape, g, e)
    return _table(np.arange(len(objects)), recs), shells


def depth_labels_host(labels, intensity=None, n_shells=DEFAULT_SHELLS, background_label=0, keep_absent=False):
    """``(table, shells)`` of a label map, label by label -- a pixel of another label is outside --: the present labels without
    ``background_label`` (None: all) in ascending order; with ``keep_absent`` one row per label 0 .. max, the zero row for an absent
    label and for the background label."""
    labels = _check_labels(labels)
    g = _check_intensity(intensity, labels.shape)
    n_shells = check_shells(n_shells)
    e = scale_exponent(g) if g is not None else 0
    n = _label_count(labels)
    recs, shells = _zero(n, n_shells)
    for l in sorted(frozenset(labels.reshape(-1).tolist())):
        if l != background_label:
            rr, cc = np.nonzero(labels == l)
            r0, c0 = int(rr.min()), int(cc.min())
            _fill_record(recs[l:l + 1], shells[l], (labels == l)[r0:int(rr.max()) + 1, c0:int(cc.max()) + 1], (r0, c0), labels.shape, g, e)
    ls = np.arange(n) if keep_absent else np.nonzero(recs['area'] > 0)[0]
    return _table(ls, recs[ls]), shells[ls]


# ---- derived columns: one function for the host and the GPU forms ----------------------------------------------------------------------
_DERIVED_HEAD = [('label', 'i4'), ('area', 'i8'), ('on_boundary', '?'), ('center_row', 'i4'), ('center_col', 'i4'), ('max_radius', 'f8'),
                 ('mean_radius', 'f8'), ('median_radius', 'f8'), ('rms_radius', 'f8'), ('thickness', 'f8')]


def derived_dtype(n_shells):
    n_shells = check_shells(n_shells)
    return np.dtype(_DERIVED_HEAD + [(f'shell{s}_{what}', 'f8') for s in range(n_shells) for what in ('fraction', 'mean_intensity', 'intensity_fraction')])


def shell_sum_exact(row):
    """The intensity sum of a shell row as the integer gsum_hi 2^32 + gsum_lo, in units of 2^(e - 62)."""
    return int(row['gsum_hi']) * 2 ** 32 + int(row['gsum_lo'])


def derive(table, shells):
    """The derived columns of a result (:func:`derived_dtype`), on the host from its exact integers: ``max_radius`` = sqrt(max_d2),
    ``mean_radius`` = sum_q / 2^16 / area, ``median_radius`` = 0.5 sqrt(med_d2_lo) + 0.5 sqrt(med_d2_hi), ``rms_radius`` =
    sqrt(sum_d2 / area), ``thickness`` = 2 max_radius - 1 (the width of the widest place, in pixels), ``center_row`` / ``center_col`` the
    inscribed circle's centre; per shell its fraction of the object's pixels, its mean intensity and its fraction of the object's
    summed intensity (the sums in Python integers).  Rows without a pixel read NaN; so do the intensity columns of a shell without a
    finite pixel, and the intensity fractions of an object whose summed intensity is zero."""
    shells = np.asarray(shells)
    if shells.ndim != 2 or len(shells) != len(table) or shells.dtype != _capi.DEPTH_SHELL_DTYPE:
        raise ValueError(f'shells: one row of sdsm_depth_shell_record per table row and shell expected, got {shells.dtype} {shells.shape}')
    n_shells = shells.shape[1]
    out = np.zeros(len(table), derived_dtype(n_shells))
    for name in out.dtype.names[5:]:
        out[name] = np.nan
    out['label'], out['area'], out['on_boundary'] = table['label'], table['area'], (table['flags'] & FRAME) != 0
    out['center_row'], out['center_col'] = table['max_row'], table['max_col']
    for k, row in enumerate(table):
        n, e = int(row['area']), int(row['scale_exp'])
        if n == 0:
            continue
        o = out[k:k + 1]
        o['max_radius'] = math.sqrt(int(row['max_d2']))
        o['mean_radius'] = float(Fraction(int(row['sum_q']), 65536 * n))
        o['median_radius'] = 0.5 * math.sqrt(int(row['med_d2_lo'])) + 0.5 * math.sqrt(int(row['med_d2_hi']))
        o['rms_radius'] = math.sqrt(Fraction(int(row['sum_d2']), n))
        o['thickness'] = 2 * math.sqrt(int(row['max_d2'])) - 1
        sums = [shell_sum_exact(s) for s in shells[k]]
        total = sum(sums)
        for s in range(n_shells):
            nf = int(shells[k, s]['n_finite'])
            o[f'shell{s}_fraction'] = float(Fraction(int(shells[k, s]['count']), n))
            if nf:
                o[f'shell{s}_mean_intensity'] = _scaled(float(Fraction(sums[s], nf)), e - 62)
                if total:
                    o[f'shell{s}_intensity_fraction'] = float(Fraction(sums[s], total))
    return out


def write_depth_csv(path, table, shells):
    """A result with its derived columns as CSV, every field quoted (as ``measure.write_measurements_csv``); after the derived columns
    the exact ones: the record's integers, then per shell its four."""
    d = derive(table, shells)
    exact = [n for n, _ in _capi._DEPTH_FIELDS if n not in ('area',)]
    n_shells = np.asarray(shells).shape[1]
    with open(path, 'w', newline='') as fp:
        w = csv.writer(fp, delimiter=',', quoting=csv.QUOTE_ALL)
        w.writerow(list(d.dtype.names) + exact + [f'shell{s}_{n}' for s in range(n_shells) for n, _ in _capi._DEPTH_SHELL_FIELDS])
        for k, (drow, row) in enumerate(zip(d, table)):
            w.writerow([repr(v.item()) for v in drow] + [repr(row[n].item()) for n in exact]
                       + [repr(shells[k, s][n].item()) for s in range(n_shells) for n, _ in _capi._DEPTH_SHELL_FIELDS])


# ---- the GPU forms (sdsm_depth.hip) ---------------------------------------------------------------------------------------------------
def workspace_pixels(boxes):
    """Workspace pixels of the objects with the boxes (r0, c0, h, w): ``sdsm_depth_workspace_pixels``, h w for a box above
    ``_capi.DEPTH_LDS_PIXELS`` pixels and 0 for one that LDS holds."""
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    px = np.where((b[:, 2] < 1) | (b[:, 3] < 1), 0, b[:, 2] * b[:, 3])
    return np.where(px > _capi.DEPTH_LDS_PIXELS, px, 0).astype(np.int64)


class _DepthSet:
    """One set of up to ``_capi.MAX_SET_IMAGES`` images, with their intensities or without, on the current device and the two calls of
    the depth kernel."""

    def __init__(self, shapes, intensities):
        self.M = _MeasureSet(shapes, intensities)     # (the intensities packed; the label form takes the boxes of the labels from there)
        self.S = self.M.S
        self.n_im = len(self.S.shapes)

    def buffers(self, boxes, n_shells):
        """The outputs and the workspace of a call; their contents do not matter."""
        S, n = self.S, len(boxes)
        ws = workspace_pixels(boxes)
        total = int(ws.sum())
        return dict(d_out=S.record_buffer(n, _capi.DEPTH_RECORD_DTYPE), d_shells=S.record_buffer(n * n_shells, _capi.DEPTH_SHELL_DTYPE),
                    d_ws_off=S._up(_exclusive(ws)) if total else None, ws_pixels=total,
                    d_ws=S.torch.empty(total * _capi.DEPTH_WS_PIXEL_BYTES, dtype=S.torch.uint8, device=S.dev) if total else None)

    def _workspace(self, B, ws_bytes):
        """The four workspace arguments; ``ws_bytes``: the size named to the call instead of the buffer's own."""
        S = self.S
        own = B['ws_pixels'] * _capi.DEPTH_WS_PIXEL_BYTES
        return S._p(B['d_ws_off']), S._p(B['d_ws']), B['ws_pixels'], own if ws_bytes is None else int(ws_bytes)

    def _download(self, B, n, n_shells):
        recs = self.S.records(B['d_out'], n, _capi.DEPTH_RECORD_DTYPE)
        shells = self.S.records(B['d_shells'], n * n_shells, _capi.DEPTH_SHELL_DTYPE).reshape(n, n_shells)
        if (recs['flags'] & _capi.DEPTH_NO_WORKSPACE).any():
            raise _capi.SdsmError('an object above the LDS tile was named no workspace, see DESIGN.md "Limits"')
        return recs, shells

    def objects(self, obj_image, boxes, words, packed, n_shells, B=None, ws_bytes=None):
        """(records, shells) of the objects of the set (``packed``: the bit-packed fragments, one uint8 array of whole words each)."""
        S, n = self.S, len(boxes)
        B = self.buffers(boxes, n_shells) if B is None else B
        d_objects = S.upload_objects(obj_image, boxes, words, packed)
        S.capi.check(S.L.sdsm_depth_objects_multi(S.table, self.n_im, n, *map(S._p, d_objects), S._p(self.M.d_g), S._p(self.M.d_gmax), S._p(self.M.d_exp), n_shells,
                                                  *self._workspace(B, ws_bytes), S._p(B['d_out']), S._p(B['d_shells']), S._stream()), 'sdsm_depth_objects_multi')
        return self._download(B, n, n_shells)

    def labels(self, labels, background_label, n_shells):
        """Per image (labels measured, number of labels, records, shells) of the label maps of the set: the windows of the labels
        (``measure._LabelWindows``), then sdsm_depth_labels."""
        S = self.S
        w = _LabelWindows(self.M, labels, background_label, 'depth')
        n = len(w.idx)
        B = self.buffers(w.boxes, n_shells)
        S.capi.check(S.L.sdsm_depth_labels_multi(S.table, self.n_im, *w.args(), S._p(self.M.d_g), S._p(self.M.d_gmax), S._p(self.M.d_exp), n_shells,
                                                 *self._workspace(B, None), S._p(B['d_out']), S._p(B['d_shells']), S._p(w.d_bad), S._stream()),
                     'sdsm_depth_labels_multi')
        recs, shells = self._download(B, n, n_shells)
        return [(ls, n_labels, recs[a:b], shells[a:b]) for ls, n_labels, a, b in w.per_image()]


def depth_objects_many(objects_per_image, shapes, intensities=None, n_shells=DEFAULT_SHELLS):
    """:func:`depth_objects` for a list of images: one launch per ``_capi.MAX_SET_IMAGES`` images (larger lists are split).  Per image the
    bytes of :func:`depth_objects_host`."""
    sets = _object_sets(objects_per_image, shapes, intensities)
    n_shells = check_shells(n_shells)
    out = []
    for _, shapes_part, gs, packed, first in sets:
        recs, shells = _DepthSet(shapes_part, gs).objects(*packed, n_shells)
        out += [(_table(np.arange(b - a), recs[a:b]), shells[a:b]) for a, b in zip(first[:-1], first[1:])]
    return out


def depth_objects(objects, shape, intensity=None, n_shells=DEFAULT_SHELLS):
    """``(table, shells)`` of a list of objects (``fg_offset``, ``fg_fragment``; they may overlap) of an image of ``shape`` on the GPU, one
    workgroup per object; row k is object k.  ``intensity``: an image of that shape, or None.  The bytes of :func:`depth_objects_host`."""
    return depth_objects_many([objects], [shape], [intensity] if intensity is not None else None, n_shells)[0]


def depth_labels_many(labels_list, intensities=None, n_shells=DEFAULT_SHELLS, background_label=0, keep_absent=False):
    """:func:`depth_labels` for a list of label maps, one launch per ``_capi.MAX_SET_IMAGES`` images."""
    sets = _label_sets(labels_list, intensities)
    n_shells = check_shells(n_shells)
    out = []
    for _, l32, shapes, gs in sets:
        for ls, n_labels, recs, shells in _DepthSet(shapes, gs).labels(l32, background_label, n_shells):
            if keep_absent:
                full, full_shells = _zero(n_labels, n_shells)
                full_shells[ls] = shells
                (ls, recs), shells = _keep_absent(full, ls, recs), full_shells
            out.append((_table(ls, recs), shells))
    return out


def depth_labels(labels, intensity=None, n_shells=DEFAULT_SHELLS, background_label=0, keep_absent=False):
    """``(table, shells)`` of a label map (integer, labels 0 .. 65535) on the GPU: the present labels without ``background_label`` (None:
    all) in ascending order, or with ``keep_absent`` one row per label 0 .. max.  The bytes of :func:`depth_labels_host`."""
    return depth_labels_many([labels], [intensity] if intensity is not None else None, n_shells, background_label, keep_absent)[0]


def depth_result(data, objects='postprocessed_objects', intensity='g_raw', n_shells=DEFAULT_SHELLS):
    """The depth table of the objects of pipeline data: ``objects`` an output name or a list of objects, ``intensity`` a key of ``data``,
    an image, or None."""
    return depth_objects(*_result_inputs(data, objects, intensity), n_shells)
