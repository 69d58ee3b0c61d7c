"""How the objects of one segmentation lie to each other: which labels touch and along how much of their outline, how wide the gap to
the closest other label is, how many neighbours a label has within a given distance, which labels sit on the image frame.  ``measure``,
``shape``, ``intensity`` and ``texture`` describe each object by itself, ``compare`` and ``boundary`` set one segmentation against
another; this module describes one label map against itself.  Label maps only: objects come in through
``render.rasterize_labels_many``, which makes them disjoint.

Everything is defined in integers, so that the GPU form (``k_neighbours``, sdsm_neighbours.hip) gives the bytes of the host definitions
:func:`neighbour_pairs_host` and :func:`neighbour_labels_host` whatever the launch, the set size or the capacity of the pair table:

* A label map is a two-dimensional integer image with the labels 0 .. 65535, 0 the background, and H^2 + W^2 < 2^31
  (``boundary.check_shape``).
* Two pixels are **within reach** iff their squared Euclidean distance is <= ``max_d2``, 1 <= ``max_d2`` <= ``MAX_D2`` = 4096 (a reach
  of 64 pixels).  ``max_d2`` = 1 sees edge contacts only, 2 the 8-connected ones; :func:`reach_d2` turns a distance into ``max_d2``.
* **Pairs.**  An unordered pair of labels a < b, both >= 1, has a row iff some pixel of a and some pixel of b are within reach.
  ``min_d2`` is the smallest squared distance between a pixel of a and a pixel of b, ``contact_edges`` the number of crack edges between
  them: 4-adjacent pixel pairs with one pixel in a and one in b, each counted once.  Rows are sorted by (a, b).
* **Labels.**  One row per label 0 <= l < ``n_labels``: ``area``; ``boundary``, the boundary pixels exactly as
  ``boundary.boundary_mask`` defines them (the image frame makes no boundary); ``close``, the boundary pixels of l that have a pixel of
  another label >= 1 within reach; ``edges_background``, ``edges_labels``, ``edges_frame``, the pixel sides of l that face label 0, face
  another label >= 1, or lie on the image frame.  Label 0's row holds its area and zeros.  The sum of ``contact_edges`` over the pairs
  of l is ``edges_labels`` of l, and ``close`` <= ``boundary``.

The host definitions compare the map with its shift for every offset of the half-plane of the disk.  The kernel searches from boundary
pixels only, which is enough: let p in a and q in b be a closest pair of pixels of two disjoint labels and suppose p is no boundary
pixel of a.  Step from p by one pixel along an axis on which p and q differ.  That pixel lies between p and q on that axis, so inside
the image; it carries a, as all 4-neighbours of p inside the image do; and it is strictly closer to q.  So p was not closest.  The GPU
tests pin this against the host definitions, which compare all pixels.

Floats are made in ONE place, :func:`derive`.  Parity with CellProfiler's ``MeasureObjectNeighbors`` is UNPINNED (it was not available
to compare with); by its documentation it differs in that it dilates the objects and counts overlaps of the dilated objects, and its
closest distances are between centroids."""
import csv
import math
from fractions import Fraction

import numpy as np

from . import _capi
from .boundary import boundary_mask, check_shape
from .compare import grow_tables
from .imageset import in_sets

MAX_D2 = _capi.NEIGHBOUR_MAX_D2
MAX_LABELS = _capi.BOUNDARY_MAX_LABELS
LABEL_DTYPE = _capi.NEIGHBOUR_LABEL_DTYPE
PAIR_DTYPE = _capi.NEIGHBOUR_PAIR_DTYPE
DEFAULT_CAPACITY = 1 << 14            # slots of an image's pair table at the first launch (256 KB per image, as compare's); grown by compare.grow_tables
DERIVED_DTYPE = np.dtype([('label', 'i4'), ('n_neighbours', 'i4'), ('n_touching', 'i4'),
                          ('first_label', 'i4'), ('first_d2', 'i4'), ('first_distance', 'f8'),
                          ('second_label', 'i4'), ('second_d2', 'i4'), ('second_distance', 'f8'),
                          ('close_fraction', 'f8'), ('contact_fraction', 'f8'), ('on_frame', '?')])


# ---- the definitions ------------------------------------------------------------------------------------------------------------------
def reach_d2(distance):
    """``max_d2`` of a reach of ``distance`` pixels: floor(distance^2), exactly, for an int or a ``fractions.Fraction``.  Anything else
    (a float has no exact square to floor) raises ``TypeError``."""
    if isinstance(distance, bool) or not isinstance(distance, (int, np.integer, Fraction)):
        raise TypeError(f'distance: an int or a fractions.Fraction; got {type(distance).__name__}')
    d = Fraction(int(distance)) if not isinstance(distance, Fraction) else distance
    if d < 0:
        raise ValueError(f'distance {distance}: >= 0 required')
    return math.floor(d * d)


def check_max_d2(max_d2):
    """``max_d2`` as an int; ``TypeError`` unless it is an integer, ``ValueError`` unless 1 <= max_d2 <= ``MAX_D2``."""
    if isinstance(max_d2, bool) or not isinstance(max_d2, (int, np.integer)):
        raise TypeError(f'max_d2: an integer (see reach_d2); got {type(max_d2).__name__}')
    if not 1 <= int(max_d2) <= MAX_D2:
        raise ValueError(f'max_d2 {int(max_d2)}: 1 <= max_d2 <= {MAX_D2} required (a reach of 64 pixels), see DESIGN.md "Limits"')
    return int(max_d2)


def _check_n_labels(n_labels):
    if isinstance(n_labels, bool) or not isinstance(n_labels, (int, np.integer)):
        raise TypeError(f'n_labels: an integer or None; got {type(n_labels).__name__}')
    if not 1 <= int(n_labels) <= MAX_LABELS:
        raise ValueError(f'n_labels {int(n_labels)}: 1 <= n_labels <= {MAX_LABELS} required')
    return int(n_labels)


def _check_map(labels, what='labels'):
    check_shape(np.shape(labels), what)                      # (the shape alone decides first)
    labels = np.asarray(labels)
    if labels.dtype.kind not in 'iu':
        raise TypeError(f'{what}: an integer image; got {labels.dtype}')
    if labels.size and (int(labels.min()) < 0 or int(labels.max()) >= MAX_LABELS):
        raise ValueError(f'{what}: labels {int(labels.min())} .. {int(labels.max())}; the neighbourhood tables take the labels 0 .. {MAX_LABELS - 1}, '
                         'see DESIGN.md "Limits"')
    return labels


def halfplane_offsets(max_d2):
    """The offsets (d_row, d_col) with 0 < d_row^2 + d_col^2 <= ``max_d2`` of the half-plane d_row > 0, or d_row == 0 and d_col > 0, row by
    row (n x 2, int64): one of every offset and its negative."""
    max_d2 = check_max_d2(max_d2)
    out = [(0, dc) for dc in range(1, math.isqrt(max_d2) + 1)]
    for dr in range(1, math.isqrt(max_d2) + 1):
        w = math.isqrt(max_d2 - dr * dr)
        out += [(dr, dc) for dc in range(-w, w + 1)]
    return np.array(out, np.int64).reshape(-1, 2)


def _views(x, dr, dc):
    """The pixels p and p + (d_row, d_col), d_row >= 0, of an image as two views of equal shape (possibly empty)."""
    H, W = x.shape
    return x[:max(H - dr, 0), max(-dc, 0):max(W - max(dc, 0), 0)], x[dr:, max(dc, 0):max(W - max(-dc, 0), 0)]


def _pairs_from_keys(keys, d2, contact):
    order = np.argsort(keys, kind='stable')
    keys = keys[order]
    pairs = np.zeros(len(keys), PAIR_DTYPE)
    pairs['a'], pairs['b'] = keys >> np.uint64(32), keys & np.uint64(0xffffffff)
    pairs['min_d2'], pairs['contact_edges'] = d2[order], contact[order]
    return pairs


def neighbour_pairs_host(labels, max_d2):
    """The pair table of a label map (``PAIR_DTYPE``: ``a``, ``b``, ``min_d2``, ``contact_edges``; a < b, sorted by (a, b)): for every
    offset of :func:`halfplane_offsets` the map is compared with its shift, the places where both labels are >= 1 and differ are kept, and
    the squared length of the offset is reduced by the pair of labels with min; the offsets (0, 1) and (1, 0) count the crack edges."""
    labels, max_d2 = _check_map(labels).astype(np.int64), check_max_d2(max_d2)
    fg = labels > 0
    keys, d2s, edges = [], [], []
    for dr, dc in halfplane_offsets(max_d2).tolist():
        fp, fq = _views(fg, dr, dc)
        m = fp & fq
        if not m.any():
            continue
        p, q = _views(labels, dr, dc)
        m &= p != q
        a, b = p[m], q[m]
        k, n = np.unique((np.minimum(a, b).astype(np.uint64) << np.uint64(32)) | np.maximum(a, b).astype(np.uint64), return_counts=True)
        keys.append(k)
        d2s.append(np.full(len(k), dr * dr + dc * dc, np.int64))
        edges.append(n if dr * dr + dc * dc == 1 else np.zeros(len(k), np.int64))
    if not keys:
        return np.zeros(0, PAIR_DTYPE)
    keys, inverse = np.unique(np.concatenate(keys), return_inverse=True)
    d2, contact = np.full(len(keys), MAX_D2 + 1, np.int64), np.zeros(len(keys), np.int64)
    np.minimum.at(d2, inverse, np.concatenate(d2s))
    np.add.at(contact, inverse, np.concatenate(edges))
    return _pairs_from_keys(keys, d2, contact)


def neighbour_labels_host(labels, max_d2, n_labels=None):
    """The label table of a label map (``LABEL_DTYPE``), one row per label 0 <= l < ``n_labels`` (None: the largest label + 1); a label
    >= ``n_labels`` raises ``ValueError``.  See the module's docstring for the columns."""
    labels, max_d2 = _check_map(labels).astype(np.int64), check_max_d2(max_d2)
    top = int(labels.max()) + 1 if labels.size else 1
    n_labels = top if n_labels is None else _check_n_labels(n_labels)
    if top > n_labels:
        raise ValueError(f'labels: the largest label is {top - 1}; n_labels = {n_labels} takes the labels 0 .. {n_labels - 1}')
    count = lambda values: np.bincount(values.reshape(-1), minlength=n_labels)
    out = np.zeros(n_labels, LABEL_DTYPE)
    out['area'] = count(labels)
    if not labels.size:
        return out
    edge = boundary_mask(labels)
    out['boundary'] = count(labels[edge])
    out['edges_frame'] = count(labels[0]) + count(labels[-1]) + count(labels[:, 0]) + count(labels[:, -1])
    for dr, dc in ((1, 0), (0, 1)):
        p, q = _views(labels, dr, dc)
        differ = p != q
        out['edges_background'] += count(p[differ & (q == 0)]) + count(q[differ & (p == 0)])
        out['edges_labels'] += count(p[differ & (q > 0)]) + count(q[differ & (p > 0)])
    fg = labels > 0
    close = np.zeros(labels.shape, bool)
    for dr, dc in halfplane_offsets(max_d2).tolist():
        fp, fq = _views(fg, dr, dc)
        m = fp & fq
        if not m.any():
            continue
        p, q = _views(labels, dr, dc)
        m &= p != q
        cp, cq = _views(close, dr, dc)
        cp |= m
        cq |= m
    out['close'] = count(labels[close & edge])
    for name in ('edges_background', 'edges_labels', 'edges_frame'):
        out[name][0] = 0                                     # (the background has an area and nothing else)
    return out


# ---- floats: one function for the host and the GPU forms ------------------------------------------------------------------------------
def _ratio(num, den):
    """num / den by one division of exact integers; nan where den is 0."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(den != 0, num / np.where(den != 0, den, 1.0), np.nan)


def _check_tables(table, pairs):
    table, pairs = np.asarray(table), np.asarray(pairs)
    if table.dtype != LABEL_DTYPE or table.ndim != 1:
        raise TypeError('table: a table of LABEL_DTYPE, as neighbour_tables gives it')
    if pairs.dtype != PAIR_DTYPE or pairs.ndim != 1:
        raise TypeError('pairs: a table of PAIR_DTYPE, as neighbour_tables gives it')
    if len(pairs) and (int(pairs['a'].min()) < 1 or int(pairs['b'].max()) >= len(table) or (pairs['a'] >= pairs['b']).any()):
        raise ValueError(f'pairs: 1 <= a < b < {len(table)} (the rows of the label table) required')
    return table, pairs


def _both_ways(pairs):
    """Every pair from either side, sorted by (own label, min_d2, other label): (own, other, min_d2, contact_edges), int64."""
    own = np.concatenate([pairs['a'], pairs['b']]).astype(np.int64)
    other = np.concatenate([pairs['b'], pairs['a']]).astype(np.int64)
    d2 = np.concatenate([pairs['min_d2'], pairs['min_d2']]).astype(np.int64)
    contact = np.concatenate([pairs['contact_edges'], pairs['contact_edges']]).astype(np.int64)
    order = np.lexsort((other, d2, own))
    return own[order], other[order], d2[order], contact[order]


def derive(table, pairs):
    """The neighbourhood columns of a morphometry table (``DERIVED_DTYPE``), one row per present label >= 1 (area > 0), from the two
    integer tables of one image:

    ``n_neighbours``, the labels within reach; ``n_touching``, those with ``contact_edges`` > 0; ``first_label`` / ``first_d2`` /
    ``first_distance`` and ``second_*``, the closest and the second closest label by ascending (``min_d2``, label) -- of two labels at the
    same distance the smaller comes first -- with the squared gap and its root, -1 / -1 / nan where there is none;
    ``close_fraction`` = ``close`` / ``boundary``; ``contact_fraction`` = ``edges_labels`` / (``edges_background`` + ``edges_labels`` +
    ``edges_frame``); ``on_frame`` = ``edges_frame`` > 0.  0 / 0 gives nan.  Every decision is one of integers, and every float is rounded
    once: one division of exact integers, one square root of an exact integer."""
    table, pairs = _check_tables(table, pairs)
    present = np.nonzero(table['area'] > 0)[0]
    present = present[present >= 1]
    out = np.zeros(len(present), DERIVED_DTYPE)
    out['label'] = present
    out['first_label'] = out['first_d2'] = out['second_label'] = out['second_d2'] = -1
    out['first_distance'] = out['second_distance'] = np.nan
    own, other, d2, contact = _both_ways(pairs)
    start = np.searchsorted(own, present, side='left')
    stop = np.searchsorted(own, present, side='right')
    out['n_neighbours'] = stop - start
    touching = np.concatenate([[0], np.cumsum(contact > 0)])
    out['n_touching'] = touching[stop] - touching[start]
    for rank, name in ((0, 'first'), (1, 'second')):
        have = stop - start > rank
        at = start[have] + rank
        out[name + '_label'][have], out[name + '_d2'][have] = other[at], d2[at]
        out[name + '_distance'][have] = np.sqrt(d2[at].astype(np.float64))
    rows = table[present]
    out['close_fraction'] = _ratio(rows['close'], rows['boundary'])
    out['contact_fraction'] = _ratio(rows['edges_labels'], rows['edges_background'] + rows['edges_labels'] + rows['edges_frame'])
    out['on_frame'] = rows['edges_frame'] > 0
    return out


def adjacency(pairs, n_labels):
    """The pair table as a graph in compressed rows: ``(offsets, neighbours)`` with the labels within reach of label l as
    ``neighbours[offsets[l]:offsets[l + 1]]`` (int32, ascending) for 0 <= l < ``n_labels``; ``offsets`` int64, n_labels + 1 entries."""
    pairs, n_labels = np.asarray(pairs), _check_n_labels(n_labels)
    if pairs.dtype != PAIR_DTYPE or pairs.ndim != 1:
        raise TypeError('pairs: a table of PAIR_DTYPE, as neighbour_tables gives it')
    if len(pairs) and (int(min(pairs['a'].min(), pairs['b'].min())) < 0 or int(max(pairs['a'].max(), pairs['b'].max())) >= n_labels):
        raise ValueError(f'pairs: labels 0 .. {n_labels - 1} required')
    own = np.concatenate([pairs['a'], pairs['b']]).astype(np.int64)
    other = np.concatenate([pairs['b'], pairs['a']]).astype(np.int32)
    order = np.lexsort((other, own))
    offsets = np.concatenate([[0], np.cumsum(np.bincount(own, minlength=n_labels))]).astype(np.int64)
    return offsets, other[order]


def write_neighbour_csv(path, table, pairs):
    """The tables of one image as one CSV, every field quoted (as ``boundary.write_distance_csv``): a row per present label >= 1 with its
    integer columns and the columns of :func:`derive`, then a row per pair; the table's name first, and a column that the row's table
    does not have stays empty.  Floats are written by ``repr``, so reading them back gives the same float64."""
    table, pairs = _check_tables(table, pairs)
    derived = derive(table, pairs)
    integer = [n for n in LABEL_DTYPE.names if n != 'reserved']
    cols = ['label'] + integer + [n for n in DERIVED_DTYPE.names if n != 'label'] + list(PAIR_DTYPE.names)
    with open(path, 'w', newline='') as fp:
        w = csv.writer(fp, delimiter=',', quoting=csv.QUOTE_ALL)
        w.writerow(['table'] + cols)
        for d in derived:
            row = table[d['label']]
            w.writerow(['labels'] + [repr(row[k].item()) if k in integer else repr(d[k].item()) if k in DERIVED_DTYPE.names else '' for k in cols])
        for p in pairs:
            w.writerow(['pairs'] + [repr(p[k].item()) if k in PAIR_DTYPE.names else '' for k in cols])


# ---- the GPU form (k_neighbours, sdsm_neighbours.hip) -----------------------------------------------------------------------------------
def _as_int32(labels, what):
    """The map as int32 for the upload.  The shape is checked first; a label outside 0 .. n_labels - 1 is left to the device, which counts
    it, unless int32 cannot hold it."""
    check_shape(np.shape(labels), what)
    labels = np.asarray(labels)
    if labels.dtype.kind not in 'iu':
        raise TypeError(f'{what}: an integer image; got {labels.dtype}')
    if labels.dtype.itemsize > 4 or labels.dtype == np.uint32:
        if labels.size and (int(labels.min()) < -2 ** 31 or int(labels.max()) >= 2 ** 31):
            raise ValueError(f'{what}: labels {int(labels.min())} .. {int(labels.max())}; the neighbourhood tables take the labels 0 .. {MAX_LABELS - 1}, '
                             'see DESIGN.md "Limits"')
    return labels.astype(np.int32)


def _launch_set(l32, max_d2, n_labels, capacities, names):
    """One launch for a set of up to ``_capi.MAX_SET_IMAGES`` int32 label maps: per image (label records, keys, (min_d2, contact_edges)
    per slot, status).  Pixels with a label outside 0 .. n_labels - 1 raise ``ValueError`` naming their images."""
    from .render import _DeviceSet
    S = _DeviceSet([x.shape for x in l32])
    C, t, n = S.C, S.torch, len(l32)
    d_map = S.pack(l32, np.int32)
    rec_off = np.concatenate([[0], np.cumsum(n_labels)]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(capacities)]).astype(np.int64)
    d_rec = t.empty(int(rec_off[-1]) * LABEL_DTYPE.itemsize, dtype=t.uint8, device=S.dev)
    d_keys = t.empty(int(off[-1]), dtype=t.int64, device=S.dev)
    d_min, d_contact = (t.empty(int(off[-1]), dtype=t.int32, device=S.dev) for _ in range(2))
    d_status = t.empty(2 * n, dtype=t.int32, device=S.dev)
    S.capi.check(S.L.sdsm_neighbours_multi(S.table, n, S._p(d_map), max_d2, (C.c_int64 * n)(*[int(v) for v in rec_off[:n]]),
                                           (C.c_int32 * n)(*[int(v) for v in n_labels]), S._p(d_rec), (C.c_int64 * n)(*[int(v) for v in off[:n]]),
                                           (C.c_int64 * n)(*[int(c) for c in capacities]), S._p(d_keys), S._p(d_min), S._p(d_contact), S._p(d_status),
                                           S._stream()), 'sdsm_neighbours_multi')
    status = d_status.cpu().numpy().reshape(n, 2)
    bad = np.nonzero(status[:, 0])[0]
    if len(bad):
        raise ValueError(f'{int(status[:, 0].sum())} pixels of images {[names[i] for i in bad]} carry a label outside 0 .. n_labels - 1 '
                         f'(n_labels {[int(n_labels[i]) for i in bad]}); the neighbourhood tables take the labels 0 .. {MAX_LABELS - 1}, see DESIGN.md "Limits"')
    rec, keys = d_rec.cpu().numpy().view(LABEL_DTYPE), d_keys.cpu().numpy().view(np.uint64)
    values = np.stack([d_min.cpu().numpy(), d_contact.cpu().numpy()], axis=1)
    return [(rec[rec_off[i]:rec_off[i + 1]].copy(), keys[off[i]:off[i + 1]], values[off[i]:off[i + 1]], status[i]) for i in range(n)]


def neighbour_tables_many(labels_list, max_d2, n_labels=None, capacity=None, info=None):
    """``(table, pairs)`` per label map of a list: the bytes of :func:`neighbour_labels_host` and :func:`neighbour_pairs_host`.  One
    launch per ``_capi.MAX_SET_IMAGES`` images (longer lists are split).  ``n_labels``: the rows of every label table (None: per image
    its largest label + 1); a pixel with a label outside 0 .. n_labels - 1 raises ``ValueError`` naming its image.  ``capacity``: the
    slots of an image's pair table at the first launch, a power of two (None: ``DEFAULT_CAPACITY``); it is doubled, for the images that
    need it alone, until the table holds all pairs at most half full (``compare.grow_tables``).  ``info``: a dict that receives
    ``capacity``, the slots each image ended at."""
    labels_list, max_d2 = list(labels_list), check_max_d2(max_d2)
    capacity = DEFAULT_CAPACITY if capacity is None else int(capacity)
    if capacity < 1 or capacity & (capacity - 1):
        raise ValueError(f'capacity {capacity}: a power of two >= 1')
    fixed = None if n_labels is None else _check_n_labels(n_labels)
    l32 = [_as_int32(l, 'labels') for l in labels_list]
    rows = []
    for i, l in enumerate(l32):
        top = max(int(l.max()), 0) + 1 if l.size else 1
        if fixed is None and top > MAX_LABELS:
            raise ValueError(f'labels of image {i}: the largest label is {top - 1}; the neighbourhood tables take the labels 0 .. {MAX_LABELS - 1}, '
                             'see DESIGN.md "Limits"')
        rows.append(top if fixed is None else fixed)
    out, caps = [None] * len(l32), [capacity] * len(l32)
    full = [i for i, l in enumerate(l32) if l.size]          # (an empty image has empty tables and no launch)
    for i in set(range(len(l32))) - set(full):
        out[i] = (np.zeros(rows[i], LABEL_DTYPE), np.zeros(0, PAIR_DTYPE))
    for part in in_sets(len(full)):
        idx = full[part]
        records = {}

        def launch(todo, cs):
            res = _launch_set([l32[idx[k]] for k in todo], max_d2, [rows[idx[k]] for k in todo], cs, [idx[k] for k in todo])
            for k, r in zip(todo, res):
                records[k] = r[0]                            # (complete after every launch, whatever became of the pairs)
            return [r[1:] for r in res]

        tables, c = grow_tables(launch, len(idx), capacity, names=idx)
        for k, (keys, values) in enumerate(tables):
            out[idx[k]], caps[idx[k]] = (records[k], _pairs_from_keys(keys, values[:, 0], values[:, 1])), c[k]
    if info is not None:
        info['capacity'] = caps
    return out


def neighbour_tables(labels, max_d2, n_labels=None, capacity=None, info=None):
    """``(table, pairs)`` of one label map on the GPU: the bytes of :func:`neighbour_labels_host` and :func:`neighbour_pairs_host`.  The
    set of this one image."""
    return neighbour_tables_many([labels], max_d2, n_labels, capacity, info)[0]


def neighbours_results(datas, objects='postprocessed_objects', *, max_d2, merge_overlap_threshold=np.inf, dilate=0):
    """``(table, pairs)`` per pipeline data object of a list: the label maps of ``objects`` (an output name, or one list of objects per
    image) by ``render.rasterize_labels_many`` (background 0, objects made disjoint), then :func:`neighbour_tables_many`."""
    from .render import rasterize_labels_many
    return neighbour_tables_many(rasterize_labels_many(datas, objects, merge_overlap_threshold, dilate), max_d2)


def neighbours_result(data, objects='postprocessed_objects', *, max_d2, merge_overlap_threshold=np.inf, dilate=0):
    """:func:`neighbours_results` for one pipeline data object (``objects``: an output name or a list of objects)."""
    from .render import _objects_of
    return neighbours_results([data], [_objects_of(data, objects)], max_d2=max_d2, merge_overlap_threshold=merge_overlap_threshold, dilate=dilate)[0]
