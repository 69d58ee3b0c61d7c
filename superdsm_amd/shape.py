"""Contour shape tables: perimeter, circularity, convex hull, solidity and Feret diameters of the objects of a segmentation, from
objects (bit-packed fragments, which may overlap; each is measured alone) or from label maps, for one image or a set of images.

These are the columns of a morphometry table that the pixel moments of :mod:`measure` cannot give: they need a pass that looks at the
neighbours of a pixel, and a hull.  As there, a table is a structured array with one row of EXACT integers per object or label
(``sdsm_shape_record``, include/sdsm.h), the GPU forms (sdsm_shape.hip) give the bytes of the ``*_host`` definitions below, and
everything that is not an integer is computed in ONE place, :func:`derive`, on the host from the integers and the hull vertices.

An object is the set P of its pixels; EVERYTHING else is outside P, the outside of the image included: a pixel on the image frame is a
border pixel and its edge on the frame counts.  (This differs from ``boundary.boundary_mask``, where the image frame makes no
boundary.)  In the label form a pixel that carries another label is outside.

  area            |P|
  border_pixels   pixels of P with a 4-neighbour outside P
  edges_r/_c      unit edges between a pixel of P and an outside pixel above or below / left or right; their sum is the crack length
  perim_n1/2/3    the classes of the 4-neighbourhood perimeter estimator: for a border pixel v = 1 + 2 (border pixels among its orthogonal
                  neighbours) + 10 (among its diagonal ones); n1: v in {5, 7, 15, 17, 25, 27}, n2: {21, 33}, n3: {13, 23} -- the bins of
                  ``ndi.convolve(P - ndi.binary_erosion(P, cross, border_value=0), [[10, 2, 10], [2, 1, 2], [10, 2, 10]], mode='constant')``
  hull            of the corners of the closed unit squares of the pixels, on the lattice 0 .. H x 0 .. W: vertices (row, column),
                  counter-clockwise in the (row, column) plane from the smallest (row, column), collinear points dropped
  n_vertices, hull_area2 (twice the area, shoelace), feret_max_d2 (largest squared distance of two vertices, int64)
  flags           bit 0: the object touches the image frame

A result is ``(table, offsets, vertices)``: the hull of row k is ``vertices[offsets[k]:offsets[k + 1]]`` (int32 (row, column) pairs, one
compact list), as the boundary lists of :mod:`boundary`.

**Parity unpinned** against scikit-image (``regionprops``), which is not available where this was written: the perimeter is pinned to the
SciPy statement above, the hull to Qhull (``scipy.spatial.ConvexHull``), by tests/test_shape_cpu.py."""
import csv
import math
from functools import partial

import numpy as np
import scipy.ndimage as ndi

from . import _capi
from .measure import (_check_labels, _check_shape, _keep_absent, _label_count, _label_sets, _label_table, _LabelWindows, _MeasureSet, _object_boxes,
                      _object_sets, _result_inputs)
from .postprocess import _check_boxes, _exclusive

TABLE_DTYPE = np.dtype([('label', 'i4')] + _capi._SHAPE_FIELDS)       # 'label': the label, or the index of the object in its image
DERIVED_DTYPE = np.dtype([('label', 'i4'), ('area', 'i8'), ('on_boundary', '?'), ('perimeter', 'f8'), ('crack_perimeter', 'f8'), ('circularity', 'f8'),
                          ('convex_area', 'f8'), ('solidity', 'f8'), ('convex_perimeter', 'f8'), ('max_feret_diameter', 'f8'),
                          ('min_feret_diameter', 'f8'), ('min_feret_angle', 'f8'), ('feret_aspect_ratio', 'f8')])
_CROSS = ndi.generate_binary_structure(2, 1)
_WEIGHTS = np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]])
_N1, _N2, _N3 = (5, 7, 15, 17, 25, 27), (21, 33), (13, 23)


# ---- the definitions: NumPy / SciPy and Python integers -------------------------------------------------------------------------------
def convex_hull(points):
    """The hull of lattice points (an iterable of (row, column)) by the monotone chain, in Python integers: the vertices counter-clockwise
    in the (row, column) plane from the smallest (row, column), collinear points dropped."""
    pts = sorted(set((int(r), int(c)) for r, c in points))
    if len(pts) <= 2:
        return pts

    def chain(seq):
        st = []
        for p in seq:
            while len(st) >= 2 and (st[-1][0] - st[-2][0]) * (p[1] - st[-2][1]) - (st[-1][1] - st[-2][1]) * (p[0] - st[-2][0]) <= 0:
                st.pop()
            st.append(p)
        return st
    return chain(pts)[:-1] + chain(reversed(pts))[:-1]


def pixel_corners(mask, offset=(0, 0)):
    """The corners of the unit squares of the set pixels of ``mask`` as lattice points (row, column), each once."""
    rr, cc = np.nonzero(np.asarray(mask, bool))
    if len(rr) == 0:
        return np.zeros((0, 2), np.int64)
    p = np.concatenate([np.stack([rr + a, cc + b], axis=1) for a in (0, 1) for b in (0, 1)]).astype(np.int64)
    return np.unique(p, axis=0) + np.asarray(offset, np.int64)


def _fill_record(rec, mask, offset, shape):
    """The record of the object ``mask`` (a window at ``offset`` of an image of ``shape``); returns its hull vertices, image coordinates."""
    P = np.asarray(mask, bool)
    if not P.any():
        return []
    border = P.astype(np.int64) - ndi.binary_erosion(P, _CROSS, border_value=0)
    hist = np.bincount(ndi.convolve(border, _WEIGHTS, mode='constant', cval=0).reshape(-1), minlength=50)
    pad = np.pad(P, 1)
    rec['area'], rec['border_pixels'] = int(P.sum()), int(border.sum())
    rec['edges_r'] = int((P & ~pad[:-2, 1:-1]).sum()) + int((P & ~pad[2:, 1:-1]).sum())
    rec['edges_c'] = int((P & ~pad[1:-1, :-2]).sum()) + int((P & ~pad[1:-1, 2:]).sum())
    rec['perim_n1'], rec['perim_n2'], rec['perim_n3'] = (int(hist[list(b)].sum()) for b in (_N1, _N2, _N3))
    hull = convex_hull(pixel_corners(P, offset).tolist())
    n = len(hull)
    rec['n_vertices'] = n
    rec['hull_area2'] = sum(hull[k][0] * hull[(k + 1) % n][1] - hull[(k + 1) % n][0] * hull[k][1] for k in range(n))
    rec['feret_max_d2'] = max((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 for p in hull for q in hull)
    rr, cc = np.nonzero(P)
    r0, c0, r1, c1 = (int(rr.min()) + int(offset[0]), int(cc.min()) + int(offset[1]), int(rr.max()) + 1 + int(offset[0]), int(cc.max()) + 1 + int(offset[1]))
    rec['flags'] = int(r0 == 0 or c0 == 0 or r1 == shape[0] or c1 == shape[1])
    return hull


_table = partial(_label_table, TABLE_DTYPE)                           # _table(labels, recs)


def _result(labels, recs, hulls):
    offsets = np.concatenate([[0], np.cumsum([len(h) for h in hulls])]).astype(np.int64)
    return _table(labels, recs), offsets, np.array([p for h in hulls for p in h], np.int32).reshape(-1, 2)


def shape_objects_host(objects, shape):
    """``(table, offsets, vertices)`` of a list of objects (``fg_offset``, ``fg_fragment``) of an image of ``shape``, object by object;
    row k is object k.  Objects may overlap: each is measured alone."""
    shape = _check_shape(shape)
    objects = list(objects)
    _check_boxes(_object_boxes(objects), shape)
    recs = np.zeros(len(objects), _capi.SHAPE_RECORD_DTYPE)
    hulls = [_fill_record(recs[k:k + 1], obj.fg_fragment, (int(obj.fg_offset[0]), int(obj.fg_offset[1])), shape) for k, obj in enumerate(objects)]
    return _result(np.arange(len(objects)), recs, hulls)


def shape_labels_host(labels, background_label=0, keep_absent=False):
    """``(table, offsets, vertices)`` of a label map, label by label: the present labels without ``background_label`` (None: all) in
    ascending order; with ``keep_absent`` one row per label 0 .. max, the zero row for an absent label and for the background label.  A
    pixel that carries another label is outside the object."""
    labels = _check_labels(labels)
    n = _label_count(labels)
    recs = np.zeros(n, _capi.SHAPE_RECORD_DTYPE)
    hulls = [[] for _ in range(n)]
    for l in sorted(frozenset(labels.reshape(-1).tolist())):
        if l != background_label:
            rr, cc = np.nonzero(labels == l)
            r0, c0 = int(rr.min()), int(cc.min())
            hulls[l] = _fill_record(recs[l:l + 1], labels[r0:int(rr.max()) + 1, c0:int(cc.max()) + 1] == l, (r0, c0), labels.shape)
    ls = np.arange(n) if keep_absent else np.nonzero(recs['area'] > 0)[0]
    return _result(ls, recs[ls], [hulls[l] for l in ls])


# ---- derived columns: one function for the host and the GPU forms ----------------------------------------------------------------------
def min_feret(hull):
    """(width, angle) of the smallest caliper over the edges of a hull (a list of (row, column) vertices): for edge k the width is the
    largest distance of a vertex from its line, m_k / sqrt(L_k) with the integers m_k = max |cross| and L_k = the squared length.  The
    edge is chosen in exact integer arithmetic (m_k^2 L_j < m_j^2 L_k, the first among equals), then one division and one root.  The
    angle is that of the chosen edge, ``atan2(d_row, d_col)`` folded into [0, pi)."""
    n = len(hull)
    if n < 3:
        return math.nan, math.nan
    best = None
    for k in range(n):
        (r0, c0), (r1, c1) = hull[k], hull[(k + 1) % n]
        dr, dc = r1 - r0, c1 - c0
        m = max(abs(dr * (q[1] - c0) - dc * (q[0] - r0)) for q in hull)
        L = dr * dr + dc * dc
        if best is None or m * m * best[1] < best[0] * best[0] * L:
            best = (m, L, dr, dc)
    m, L, dr, dc = best
    return m / math.sqrt(L), math.atan2(dr, dc) % math.pi


def derive(table, offsets, vertices):
    """The derived columns of a result (``DERIVED_DTYPE``), on the host from its exact integers and hull vertices.  Ratios without a
    denominator read NaN."""
    out = np.zeros(len(table), DERIVED_DTYPE)
    out['label'], out['area'], out['on_boundary'] = table['label'], table['area'], (table['flags'] & 1) != 0
    area = table['area'].astype(np.float64)
    out['perimeter'] = table['perim_n1'] + table['perim_n2'] * math.sqrt(2) + table['perim_n3'] * ((1 + math.sqrt(2)) / 2)
    out['crack_perimeter'] = table['edges_r'] + table['edges_c']
    out['convex_area'] = table['hull_area2'] / 2
    out['max_feret_diameter'] = np.sqrt(table['feret_max_d2'].astype(np.float64))
    with np.errstate(invalid='ignore', divide='ignore'):
        out['circularity'] = np.where(out['perimeter'] > 0, 4 * math.pi * area / out['perimeter'] ** 2, np.nan)
        out['solidity'] = np.where(table['hull_area2'] > 0, 2 * area / table['hull_area2'], np.nan)
    for k in range(len(table)):
        hull = [(int(r), int(c)) for r, c in vertices[offsets[k]:offsets[k + 1]]]
        n = len(hull)
        out['convex_perimeter'][k] = math.fsum(math.sqrt((hull[j][0] - hull[(j + 1) % n][0]) ** 2 + (hull[j][1] - hull[(j + 1) % n][1]) ** 2) for j in range(n))
        out['min_feret_diameter'][k], out['min_feret_angle'][k] = min_feret(hull)
    with np.errstate(invalid='ignore', divide='ignore'):
        out['feret_aspect_ratio'] = out['max_feret_diameter'] / out['min_feret_diameter']
    return out


def write_shape_csv(path, table, offsets, vertices):
    """A result with its derived columns as CSV, every field quoted (as ``measure.write_measurements_csv``); the hull as
    ``row column;row column;...``."""
    d = derive(table, offsets, vertices)
    names = list(DERIVED_DTYPE.names) + [n for n in _capi.SHAPE_RECORD_DTYPE.names if n not in ('area', 'flags')] + ['hull']
    with open(path, 'w', newline='') as fp:
        w = csv.writer(fp, delimiter=',', quoting=csv.QUOTE_ALL)
        w.writerow(names)
        for k, (drow, row) in enumerate(zip(d, table)):
            hull = ';'.join(f'{int(r)} {int(c)}' for r, c in vertices[offsets[k]:offsets[k + 1]])
            w.writerow([repr(v.item()) for v in drow] + [repr(int(row[n])) for n in names[len(DERIVED_DTYPE.names):-1]] + [hull])


# ---- the GPU forms (sdsm_shape.hip) ---------------------------------------------------------------------------------------------------
def vertex_slots(boxes):
    """Vertex slots of the objects with the boxes (r0, c0, h, w): ``sdsm_shape_vertex_slots``, 2 * min(h + 1, 2 w + 2) -- a chain of a hull
    has one vertex per lattice row at most, and at most w edges to either side and a vertical one."""
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    return np.where((b[:, 2] < 1) | (b[:, 3] < 1), 0, 2 * np.minimum(b[:, 2] + 1, 2 * b[:, 3] + 2)).astype(np.int64)


class _ShapeSet:
    """One set of up to ``_capi.MAX_SET_IMAGES`` images on the current device and the two calls of the shape kernels."""

    def __init__(self, shapes):
        self.M = _MeasureSet(shapes, None)       # (the label form takes the boxes of the labels from the measurement kernels)
        self.S = self.M.S
        self.n_im = len(self.S.shapes)

    def _buffers(self, boxes):
        S, n = self.S, len(boxes)
        slots = vertex_slots(boxes)
        total = max(1, int(slots.sum()))
        i32 = dict(dtype=S.torch.int32, device=S.dev)
        return dict(d_slot_off=S._up(_exclusive(slots)), d_slots=S.torch.empty(2 * total, **i32), d_verts=S.torch.empty(2 * total, **i32),
                    d_vert_off=S.torch.empty(n + 1, dtype=S.torch.int64, device=S.dev), d_out=S.record_buffer(n, _capi.SHAPE_RECORD_DTYPE))

    def _download(self, B, n):
        recs = self.S.records(B['d_out'], n, _capi.SHAPE_RECORD_DTYPE)
        if (recs['flags'] & _capi.SHAPE_CHAIN_OVERFLOW).any():
            raise _capi.SdsmError(f'a hull chain passed {_capi.SHAPE_MAX_CHAIN} vertices, see DESIGN.md "Limits"')
        offsets = B['d_vert_off'].cpu().numpy().copy()
        return recs, offsets, B['d_verts'][:2 * int(offsets[-1])].cpu().numpy().reshape(-1, 2).copy()

    def objects(self, obj_image, boxes, words, packed):
        """(records, offsets, vertices) of the objects of the set (``packed``: the bit-packed fragments, one uint8 array of whole words each)."""
        S, n = self.S, len(boxes)
        B = self._buffers(boxes)
        d_objects = S.upload_objects(obj_image, boxes, words, packed)
        S.capi.check(S.L.sdsm_shape_objects_multi(S.table, self.n_im, n, *map(S._p, d_objects), S._p(B['d_slot_off']), S._p(B['d_slots']), S._p(B['d_out']),
                                                  S._p(B['d_vert_off']), S._p(B['d_verts']), S._stream()), 'sdsm_shape_objects_multi')
        return self._download(B, n)

    def labels(self, labels, background_label):
        """Per image (labels measured, records, offsets, vertices) of the label maps of the set: the windows of the labels
        (``_LabelWindows``), then sdsm_shape_labels."""
        S = self.S
        w = _LabelWindows(self.M, labels, background_label, 'shape')
        n = len(w.idx)
        B = self._buffers(w.boxes)
        S.capi.check(S.L.sdsm_shape_labels_multi(S.table, self.n_im, *w.args(), S._p(B['d_slot_off']), S._p(B['d_slots']), S._p(B['d_out']),
                                                 S._p(B['d_vert_off']), S._p(B['d_verts']), S._p(w.d_bad), S._stream()), 'sdsm_shape_labels_multi')
        recs, offsets, vertices = self._download(B, n)
        return [(ls, n_labels) + _split(recs, offsets, vertices, a, b) for ls, n_labels, a, b in w.per_image()]


def _split(recs, offsets, vertices, a, b):
    """The objects a .. b - 1 of a call: (records, offsets from 0, their vertices)."""
    return recs[a:b], offsets[a:b + 1] - offsets[a], vertices[offsets[a]:offsets[b]]


def shape_objects_many(objects_per_image, shapes):
    """:func:`shape_objects` for a list of images: one launch per ``_capi.MAX_SET_IMAGES`` images (larger lists are split).  Per image the
    bytes of :func:`shape_objects_host`."""
    out = []
    for _, shapes_part, _, packed, first in _object_sets(objects_per_image, shapes):
        recs, offsets, vertices = _ShapeSet(shapes_part).objects(*packed)
        for a, b in zip(first[:-1], first[1:]):
            r, o, v = _split(recs, offsets, vertices, a, b)
            out.append((_table(np.arange(b - a), r), o, v))
    return out


def shape_objects(objects, shape):
    """``(table, offsets, vertices)`` of a list of objects (``fg_offset``, ``fg_fragment``; they may overlap) of an image of ``shape`` on
    the GPU, one workgroup per object; row k is object k."""
    return shape_objects_many([objects], [shape])[0]


def shape_labels_many(labels_list, background_label=0, keep_absent=False):
    """:func:`shape_labels` for a list of label maps, one launch per ``_capi.MAX_SET_IMAGES`` images."""
    out = []
    for _, l32, shapes, _ in _label_sets(labels_list):
        for ls, n_labels, recs, offsets, vertices in _ShapeSet(shapes).labels(l32, background_label):
            if keep_absent:
                counts = np.zeros(n_labels, np.int64)
                counts[ls] = np.diff(offsets)
                offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
                ls, recs = _keep_absent(np.zeros(n_labels, _capi.SHAPE_RECORD_DTYPE), ls, recs)
            out.append((_table(ls, recs), offsets, vertices))
    return out


def shape_labels(labels, background_label=0, keep_absent=False):
    """``(table, offsets, vertices)`` of a label map (integer, labels 0 .. 65535) on the GPU: the present labels without
    ``background_label`` (None: all) in ascending order, or with ``keep_absent`` one row per label 0 .. max.  The bytes of
    :func:`shape_labels_host`."""
    return shape_labels_many([labels], background_label, keep_absent)[0]


def shape_result(data, objects='postprocessed_objects'):
    """The shape table of the objects of pipeline data: ``objects`` an output name or a list of objects."""
    return shape_objects(*_result_inputs(data, objects)[:2])
