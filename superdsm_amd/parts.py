"""Connected parts of a label map: which pixels of a label hang together, as a part map, a table per part and a table per label with
the number of parts, the largest part and the holes, and new label maps that keep the largest part of every label, the parts of a least
area, or every part as a label of its own.  ``render.rasterize_labels*`` can cut an object in two, a ``zones.ring`` around a nucleus that
touches its neighbour is several arcs, post-processed masks keep specks: ``depth``, ``shape`` and the ``compare`` scores take such a label
as one object, and with the maps of this module they need not.  :func:`label_mask` is the entry for a segmentation that comes as a
foreground mask.

Everything is defined in integers, so that the GPU form (sdsm_parts.hip) gives the bytes of the host definitions :func:`parts_host` and
:func:`keep_maps_host` whatever the launch, the tiling or the set size:

* A **label map** L is a two-dimensional integer image with the labels 0 .. 65535, 0 the background, and H^2 + W^2 < 2^31
  (``boundary.check_shape``), so that a raster index r * W + c fits int32.  It is extended by label 0 outside the image frame.
* ``connectivity`` is 4 or 8.  A **part** is a maximal set of pixels of one label >= 1 that are connected under that adjacency; pixels
  of different labels are never connected, however they touch.  The parts of an image are **numbered** 1 .. K by their first pixel in
  raster order, the smallest r * W + c.  For a map with the single label 1 this is the numbering of ``scipy.ndimage.label`` with the
  matching structure.
* The **part map** is an int32 image: the part number of every pixel, 0 on the background.
* The **part table** (``PART_DTYPE``, ``sdsm_part_record``) has one row per part, in part order: ``label``, ``area``, ``first`` (the
  raster index of the part's first pixel), the tight box ``r0``, ``c0``, ``r1``, ``c1`` (``r1`` and ``c1`` exclusive) and
  ``index_in_label``, 0 for the label's first part in part order.
* The **label table** (``LABEL_DTYPE``, ``sdsm_part_label_record``) has one row per label 0 .. n_labels - 1, n_labels the largest label
  + 1; the row of label 0 is all zero.  ``n_parts``; ``area``; ``largest_area`` and ``largest_part``, the part number of the largest
  part -- of several parts of the largest area the smallest part number wins; ``q1``, ``q3``, ``qd``, the bit-quad counts of the label's
  mask M = (L == l) over all (H + 1) * (W + 1) windows of 2 x 2 places of the zero-padded mask: windows with exactly one pixel of M, with
  exactly three, and with exactly the two of a diagonal.
* :func:`derive` adds ``euler`` = (q1 - q3 + 2 qd) / 4 under connectivity 4 and (q1 - q3 - 2 qd) / 4 under 8 (the division is exact),
  ``holes`` = ``n_parts`` - ``euler`` and ``largest_fraction`` = ``largest_area`` / ``area``.
* **Holes**, stated directly (:func:`holes_host`): the components of the complement of M in the image padded by one pixel, under the
  dual adjacency (8 for connectivity 4, 4 for 8), without the one that reaches the padding.  Other labels inside a ring are complement,
  so they count as a hole of the ring.  Holes per part are not given: run the module again on the ``split`` map.
* **Selections** turn (L, part map, tables) into int32 label maps, up to ``MAX_KEEPS`` per call:

  ====================  ====================  ==============================================
  selection             a pixel gets          if (otherwise 0)
  ====================  ====================  ==============================================
  ``Keep.split()``      its part number       L >= 1
  ``Keep.largest()``    L                     its part is ``largest_part`` of its label
  ``Keep.min_area(a)``  L                     the area of its part is >= a, 1 <= a < 2^31
  ====================  ====================  ==============================================

  The labels of a ``largest`` or ``min_area`` map are a subset of those of L.  A ``split`` map has K labels, and K is bounded by the
  pixels alone: the other modules take it only while K <= 65535 (DESIGN.md "Limits"); nothing is clamped.

K is not known before the device has numbered the parts, so the GPU form downloads the per-image counts and sizes the part table then.
``index_in_label`` is filled on the host in both forms (a count along the part order, from the ``label`` column)."""
import csv

import numpy as np

from . import _capi
from .boundary import check_shape
from .imageset import in_sets

MAX_KEEPS = _capi.PARTS_MAX_KEEPS
MAX_LABELS = _capi.BOUNDARY_MAX_LABELS
PART_DTYPE, LABEL_DTYPE = _capi.PART_DTYPE, _capi.PART_LABEL_DTYPE
DERIVED_DTYPE = np.dtype([(n, '<i4') for n in LABEL_DTYPE.names if n != 'reserved'] + [('euler', '<i4'), ('holes', '<i4'), ('largest_fraction', '<f8')])


# ---- the definitions ------------------------------------------------------------------------------------------------------------------
def _check_map(labels, what='labels'):
    check_shape(np.shape(labels), what)                      # (the shape alone decides first)
    labels = np.asarray(labels)
    if labels.dtype.kind not in 'iu':
        raise TypeError(f'{what}: an integer image; got {labels.dtype}')
    if labels.size and (int(labels.min()) < 0 or int(labels.max()) >= MAX_LABELS):
        raise ValueError(f'{what}: labels {int(labels.min())} .. {int(labels.max())}; the connected parts take the labels 0 .. {MAX_LABELS - 1}, '
                         'see DESIGN.md "Limits"')
    return labels


def check_connectivity(connectivity):
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or int(connectivity) not in (4, 8):
        raise ValueError(f'connectivity {connectivity!r}: 4 or 8')
    return int(connectivity)


def structure(connectivity):
    """The 3 x 3 structuring element of ``scipy.ndimage.label`` for the adjacency."""
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
    return cross if check_connectivity(connectivity) == 4 else np.ones((3, 3), bool)


class Keep:
    """One rule that turns (L, part map, tables) into a label map; made by :meth:`split`, :meth:`largest` or :meth:`min_area`.  ``kind``
    is the constructor's name, ``area`` the least area (None where the kind has none)."""
    __slots__ = ('kind', 'area')

    def __init__(self, kind, area):
        self.kind, self.area = kind, area

    @classmethod
    def split(cls):
        """Every part becomes a label of its own: its part number."""
        return cls('split', None)

    @classmethod
    def largest(cls):
        """Every label keeps its largest part (of several of that area the first in part order)."""
        return cls('largest', None)

    @classmethod
    def min_area(cls, area):
        """Every label keeps its parts of at least ``area`` pixels."""
        if isinstance(area, bool) or not isinstance(area, (int, np.integer)):
            raise TypeError(f'min_area: an integer number of pixels; got {type(area).__name__}')
        if not 1 <= int(area) < 2 ** 31:
            raise ValueError(f'min_area {int(area)}: 1 <= area < 2^31 required')
        return cls('min_area', int(area))

    def spec(self):
        """The selection as (kind, min_area) of ``sdsm_keep_spec``."""
        return ({'split': _capi.KEEP_SPLIT, 'largest': _capi.KEEP_LARGEST, 'min_area': _capi.KEEP_MIN_AREA}[self.kind], self.area or 0)

    def __eq__(self, other):
        return isinstance(other, Keep) and (self.kind, self.area) == (other.kind, other.area)

    def __hash__(self):
        return hash((self.kind, self.area))

    def __repr__(self):
        return f'Keep.{self.kind}({"" if self.area is None else self.area})'


split, largest, min_area = Keep.split, Keep.largest, Keep.min_area


def check_keeps(keeps):
    """``keeps`` as a list of :class:`Keep`: ``TypeError`` for anything else in it, ``ValueError`` for more than ``MAX_KEEPS``."""
    keeps = [keeps] if isinstance(keeps, Keep) else list(keeps)
    for k in keeps:
        if not isinstance(k, Keep):
            raise TypeError(f'keeps: Keep.split / largest / min_area; got {type(k).__name__}')
    if len(keeps) > MAX_KEEPS:
        raise ValueError(f'{len(keeps)} selections: a call takes at most {MAX_KEEPS}, see DESIGN.md "Limits"')
    return keeps


def _index_in_label(label):
    """Per part, in part order, how many earlier parts carry its label."""
    label = np.asarray(label, np.int64)
    order = np.argsort(label, kind='stable')
    sorted_label = label[order]
    first = np.searchsorted(sorted_label, sorted_label, side='left')
    out = np.empty(len(label), np.int32)
    out[order] = np.arange(len(label)) - first
    return out


def _label_boxes(labels):
    """(label, box slices) for every present label >= 1."""
    from scipy import ndimage as ndi
    return [(l + 1, sl) for l, sl in enumerate(ndi.find_objects(labels)) if sl is not None]


def parts_host(labels, connectivity=4):
    """``(part_map, part_table, label_table)`` of a label map, the plain statement of the module's docstring with SciPy and NumPy: per
    label, ``scipy.ndimage.label`` of its mask inside its box; the parts of all labels are then numbered by their first raster index."""
    from scipy import ndimage as ndi
    labels, st = _check_map(labels).astype(np.int32), structure(connectivity)
    H, W = labels.shape
    n_labels = int(labels.max()) + 1 if labels.size else 1
    found, comps = [], []                                    # (first, label, its component number), (label, box, component map of the box)
    table = np.zeros(n_labels, LABEL_DTYPE)
    for l, sl in (_label_boxes(labels) if labels.size else []):
        mask = labels[sl] == l
        comp, k = ndi.label(mask, st)
        r, c = np.nonzero(comp)
        firsts = np.full(k + 1, H * W, np.int64)
        np.minimum.at(firsts, comp[r, c], (r + sl[0].start) * W + c + sl[1].start)
        found += [(int(firsts[j]), l, j) for j in range(1, k + 1)]
        comps.append((l, sl, comp))
        P = np.pad(mask, 1).astype(np.int8)
        a, b, c_, d = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
        m = a + b + c_ + d
        table[l]['q1'], table[l]['q3'], table[l]['qd'] = (m == 1).sum(), (m == 3).sum(), ((m == 2) & (a == d)).sum()
    found.sort()                                             # (first pixels differ: the order is theirs)
    number = {(l, j): k for k, (_, l, j) in enumerate(found, 1)}
    part_map = np.zeros((H, W), np.int32)
    for l, sl, comp in comps:
        lut = np.array([0] + [number[l, j] for j in range(1, int(comp.max()) + 1)], np.int32)
        part_map[sl] += lut[comp]                            # (the masks of the labels are disjoint)
    parts = np.zeros(len(found), PART_DTYPE)
    parts['first'], parts['label'] = [f[0] for f in found], [f[1] for f in found]
    parts['area'] = np.bincount(part_map.reshape(-1), minlength=len(found) + 1)[1:]
    for k, box in enumerate(ndi.find_objects(part_map) if len(found) else []):
        parts[k]['r0'], parts[k]['c0'], parts[k]['r1'], parts[k]['c1'] = box[0].start, box[1].start, box[0].stop, box[1].stop
    parts['index_in_label'] = _index_in_label(parts['label'])
    _fill_label_table(table, parts)
    return part_map, parts, table


def _fill_label_table(table, parts):
    """n_parts, area, largest_area and largest_part of a label table from the part table."""
    for k, p in enumerate(parts, 1):
        row = table[p['label']]
        row['n_parts'] += 1
        row['area'] += p['area']
        if p['area'] > row['largest_area']:                  # (strictly: of equal areas the first part stays)
            row['largest_area'], row['largest_part'] = p['area'], k


def holes_host(labels, connectivity=4):
    """Per label 0 .. n_labels - 1 its holes, stated directly (int32; 0 for label 0 and absent labels): the components of the complement
    of its mask in the image padded by one pixel, under the dual adjacency, without the component that reaches the padding."""
    from scipy import ndimage as ndi
    labels = _check_map(labels).astype(np.int32)
    dual = structure(8 if check_connectivity(connectivity) == 4 else 4)
    out = np.zeros(int(labels.max()) + 1 if labels.size else 1, np.int32)
    for l, sl in (_label_boxes(labels) if labels.size else []):
        _, k = ndi.label(~np.pad(labels[sl] == l, 1), dual)  # (what lies outside the box of the label is complement that reaches the padding)
        out[l] = k - 1
    return out


def _check_label_table(table):
    table = np.asarray(table)
    if table.dtype != LABEL_DTYPE or table.ndim != 1:
        raise TypeError('label_table: a table of LABEL_DTYPE, as parts gives it')
    return table


def derive(label_table, connectivity):
    """The label table (without ``reserved``) with three more columns (``DERIVED_DTYPE``), one row per label 0 .. n_labels - 1: ``euler``
    and ``holes`` from the bit quads by the formula of the module's docstring, every step in integers, and ``largest_fraction``, one
    division of the two integers (nan for a label without pixels)."""
    table, connectivity = _check_label_table(label_table), check_connectivity(connectivity)
    out = np.zeros(len(table), DERIVED_DTYPE)
    for n in LABEL_DTYPE.names:
        if n != 'reserved':
            out[n] = table[n]
    q1, q3, qd = (table[n].astype(np.int64) for n in ('q1', 'q3', 'qd'))
    four = q1 - q3 + (2 if connectivity == 4 else -2) * qd
    if (four % 4).any():
        raise ValueError('label_table: q1 - q3 +- 2 qd is not a multiple of 4: these are not the bit quads of a mask')
    out['euler'] = four // 4
    out['holes'] = table['n_parts'] - out['euler']
    area = table['area'].astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        out['largest_fraction'] = np.where(area > 0, table['largest_area'] / np.where(area > 0, area, 1.0), np.nan)
    return out


def write_parts_csv(path, label_table, connectivity):
    """The label table of one image with the columns of :func:`derive` as a CSV, every field quoted (as ``boundary.write_distance_csv``):
    a row per present label >= 1.  Floats are written by ``repr``, so reading them back gives the same float64."""
    derived = derive(label_table, connectivity)
    with open(path, 'w', newline='') as fp:
        w = csv.writer(fp, delimiter=',', quoting=csv.QUOTE_ALL)
        w.writerow(['label', 'connectivity'] + list(DERIVED_DTYPE.names))
        for l in range(1, len(derived)):
            if derived[l]['area'] > 0:
                w.writerow([repr(l), repr(int(connectivity))] + [repr(derived[l][n].item()) for n in DERIVED_DTYPE.names])


def _keep_map(keep, labels, part_map, parts, table):
    """One selection's int32 map, by the table of the module's docstring."""
    if keep.kind == 'split':
        return part_map.astype(np.int32)
    fg = part_map >= 1
    at = np.where(fg, part_map - 1, 0)
    if keep.kind == 'largest':
        ok = fg & (table['largest_part'][np.where(fg, labels, 0)] == part_map)
    else:
        ok = fg & (parts['area'][at] >= keep.area) if len(parts) else fg
    return np.where(ok, labels, 0).astype(np.int32)


def keep_maps_host(labels, keeps, connectivity=4):
    """The int32 maps of ``keeps`` (in their order) of a label map, from :func:`parts_host`."""
    keeps = check_keeps(keeps)
    labels = _check_map(labels)
    part_map, parts, table = parts_host(labels, connectivity)
    return [_keep_map(k, labels.astype(np.int64), part_map, parts, table) for k in keeps]


def _mask_as_labels(mask):
    """``mask != 0`` as a map of label 1, for a boolean or integer mask."""
    check_shape(np.shape(mask), 'mask')
    mask = np.asarray(mask)
    if mask.dtype.kind not in 'biu':
        raise TypeError(f'mask: a boolean or integer image; got {mask.dtype}')
    return (mask != 0).astype(np.int32)


def label_mask_host(mask, connectivity=4):
    """:func:`parts_host` of ``mask != 0`` as label 1."""
    return parts_host(_mask_as_labels(mask), connectivity)


# ---- the GPU form (sdsm_parts.hip) --------------------------------------------------------------------------------------------------------
def _as_int32(labels, what):
    """The map as int32 for the upload.  The shape is checked first; a label outside 0 .. 65535 is left to the device, which counts it,
    unless int32 cannot hold it."""
    check_shape(np.shape(labels), what)
    labels = np.asarray(labels)
    if labels.dtype.kind not in 'iu':
        raise TypeError(f'{what}: an integer image; got {labels.dtype}')
    if labels.dtype.itemsize > 4 or labels.dtype == np.uint32:
        if labels.size and (int(labels.min()) < -2 ** 31 or int(labels.max()) >= 2 ** 31):
            raise ValueError(f'{what}: labels {int(labels.min())} .. {int(labels.max())}; the connected parts take the labels 0 .. {MAX_LABELS - 1}, '
                             'see DESIGN.md "Limits"')
    return labels.astype(np.int32)


def _launch_set(l32, connectivity, keeps, names):
    """The launches for a set of up to ``_capi.MAX_SET_IMAGES`` int32 label maps: per image ``(part_map, part_table, label_table, [keep
    maps])``.  Labelling and label table first; then, with the downloaded counts, the part table; then the selections.  Pixels with a
    label outside 0 .. 65535 raise ``ValueError`` naming their images."""
    from .render import _DeviceSet
    S = _DeviceSet([x.shape for x in l32])
    C, t, n, nk = S.C, S.torch, len(l32), len(keeps)
    d_map = S.pack(l32, np.int32)
    n_labels = [min(max(int(l.max()), 0) + 1, MAX_LABELS) for l in l32]     # (a larger or negative label is counted by the device)
    rec_off = np.concatenate([[0], np.cumsum(n_labels)]).astype(np.int64)
    c_rec_off, c_n_labels = (C.c_int64 * n)(*[int(v) for v in rec_off[:n]]), (C.c_int32 * n)(*n_labels)
    ws_bytes = S.L.sdsm_parts_workspace_bytes_multi(S.table, n, c_rec_off, c_n_labels)
    d_ws = t.empty((ws_bytes + 7) // 8, dtype=t.int64, device=S.dev)
    d_rec = t.empty(int(rec_off[-1]) * LABEL_DTYPE.itemsize, dtype=t.uint8, device=S.dev)
    d_part_map = t.empty(S.total, dtype=t.int32, device=S.dev)
    d_count, d_status = (t.empty(n, dtype=t.int32, device=S.dev) for _ in range(2))
    S.capi.check(S.L.sdsm_parts_multi(S.table, n, S._p(d_map), connectivity, c_rec_off, c_n_labels, S._p(d_rec), S._p(d_part_map), S._p(d_count),
                                      S._p(d_status), S._p(d_ws), ws_bytes, S._stream()), 'sdsm_parts_multi')
    status, count = d_status.cpu().numpy(), d_count.cpu().numpy()
    bad = np.nonzero(status)[0]
    if len(bad):
        raise ValueError(f'{int(status.sum())} pixels of images {[names[i] for i in bad]} carry a label outside 0 .. {MAX_LABELS - 1}; the connected '
                         f'parts take the labels 0 .. {MAX_LABELS - 1}, see DESIGN.md "Limits"')
    part_off = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    c_part_off, c_n_parts = (C.c_int64 * n)(*[int(v) for v in part_off[:n]]), (C.c_int32 * n)(*[int(v) for v in count])
    d_parts = t.empty(max(int(part_off[-1]), 1) * PART_DTYPE.itemsize, dtype=t.uint8, device=S.dev)
    S.capi.check(S.L.sdsm_parts_table_multi(S.table, n, S._p(d_map), S._p(d_part_map), c_part_off, c_n_parts, S._p(d_parts), S._stream()),
                 'sdsm_parts_table_multi')
    per_keep = []
    if nk:
        specs = np.array([k.spec() for k in keeps], np.int32).reshape(nk, 2).view(_capi.KEEP_SPEC_DTYPE)
        d_keep = t.empty(nk * S.total, dtype=t.int32, device=S.dev)
        S.capi.check(S.L.sdsm_parts_keep_multi(S.table, n, S._p(d_map), S._p(d_part_map), c_rec_off, c_n_labels, S._p(d_rec), c_part_off, c_n_parts,
                                               S._p(d_parts), nk, specs.ctypes.data_as(C.c_void_p), S.total, S._p(d_keep), S._stream()),
                     'sdsm_parts_keep_multi')
        flat = d_keep.cpu().numpy()
        per_keep = [S.layout.unpack(flat[z * S.total:(z + 1) * S.total]) for z in range(nk)]
    rec = d_rec.cpu().numpy().view(LABEL_DTYPE)
    parts = d_parts.cpu().numpy().view(PART_DTYPE)[:int(part_off[-1])]
    part_maps = S.unpack(d_part_map)
    out = []
    for i in range(n):
        table = parts[part_off[i]:part_off[i + 1]].copy()
        table['index_in_label'] = _index_in_label(table['label'])
        out.append((part_maps[i], table, rec[rec_off[i]:rec_off[i + 1]].copy(), [per_keep[z][i] for z in range(nk)]))
    return out


def _many(labels_list, connectivity, keeps):
    connectivity = check_connectivity(connectivity)
    l32 = [_as_int32(l, 'labels') for l in labels_list]
    out = [None] * len(l32)
    full = [i for i, l in enumerate(l32) if l.size]          # (an image without pixels has empty maps and tables and no launch)
    for i in set(range(len(l32))) - set(full):
        empty = lambda: np.zeros(l32[i].shape, np.int32)
        out[i] = (empty(), np.zeros(0, PART_DTYPE), np.zeros(1, LABEL_DTYPE), [empty() for _ in keeps])
    for part in in_sets(len(full)):
        idx = full[part]
        for i, res in zip(idx, _launch_set([l32[i] for i in idx], connectivity, keeps, idx)):
            out[i] = res
    return out


def parts_many(labels_list, connectivity=4):
    """``(part_map, part_table, label_table)`` per label map of a list: the bytes of :func:`parts_host`.  One set of launches per
    ``_capi.MAX_SET_IMAGES`` images (longer lists are split); a pixel with a label outside 0 .. 65535 raises ``ValueError`` naming its
    image."""
    return [(m, p, t) for m, p, t, _ in _many(list(labels_list), connectivity, [])]


def parts(labels, connectivity=4):
    """``(part_map, part_table, label_table)`` of one label map on the GPU: the bytes of :func:`parts_host`.  The set of this one image."""
    return parts_many([labels], connectivity)[0]


def keep_maps_many(labels_list, keeps, connectivity=4):
    """Per label map of a list the int32 maps of ``keeps``, in their order: the bytes of :func:`keep_maps_host`."""
    keeps = check_keeps(keeps)
    return [maps for _, _, _, maps in _many(list(labels_list), connectivity, keeps)]


def keep_maps(labels, keeps, connectivity=4):
    """The int32 maps of ``keeps`` of one label map on the GPU: the bytes of :func:`keep_maps_host`.  The set of this one image."""
    return keep_maps_many([labels], keeps, connectivity)[0]


def label_mask_many(masks, connectivity=4):
    """:func:`parts_many` of ``mask != 0`` as label 1, for boolean or integer masks: the entry for a foreground mask.  The part map is
    what ``scipy.ndimage.label`` gives with the matching structure."""
    return parts_many([_mask_as_labels(m) for m in masks], connectivity)


def label_mask(mask, connectivity=4):
    """:func:`label_mask_many` for one mask."""
    return label_mask_many([mask], connectivity)[0]


def parts_results(datas, objects='postprocessed_objects', *, connectivity=4, merge_overlap_threshold=np.inf, dilate=0):
    """``(part_map, part_table, label_table)`` per pipeline data object of a list: the label maps of ``objects`` (an output name, or one
    list of objects per image) by ``render.rasterize_labels_many`` (background 0, objects made disjoint), then :func:`parts_many`."""
    from .render import rasterize_labels_many
    connectivity = check_connectivity(connectivity)
    return parts_many(rasterize_labels_many(datas, objects, merge_overlap_threshold, dilate), connectivity)


def parts_result(data, objects='postprocessed_objects', *, connectivity=4, merge_overlap_threshold=np.inf, dilate=0):
    """:func:`parts_results` for one pipeline data object (``objects``: an output name or a list of objects)."""
    from .render import _objects_of
    return parts_results([data], [_objects_of(data, objects)], connectivity=connectivity, merge_overlap_threshold=merge_overlap_threshold, dilate=dilate)[0]
