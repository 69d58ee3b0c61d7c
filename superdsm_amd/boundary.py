"""How far the contours of two segmentations of one image lie apart: per pair of overlapping objects the Hausdorff distance, the mean
surface distance and the normalised sum of distances (NSD), the boundary measures that evaluations of deformable shape models report
beside SEG.  ``compare`` counts pixels; this module measures distances between contours.

Everything is defined in integers, so that the GPU forms (``k_label_pixel_counts``, ``k_label_pixel_lists``, ``k_pair_distances``,
sdsm_measure.hip) give the bytes of the host definitions :func:`label_boundaries_host` and :func:`pair_distances_host` whatever the
launch, the set size or the work split:

* A pixel of label l != 0 is a **boundary pixel** of l iff one of its 4-neighbours *inside the image* carries another label (the
  background or another object).  The image border makes no boundary: ``mask & ~_morph.binary_erosion(mask, _morph.disk(1))``, the
  convention of the published boundary measures.  So a one-pixel object is its own boundary, a hole has an inner boundary, two
  touching objects each have a boundary along the contact, and a label that fills the whole image has none.
* Squared distances between pixels are integers below 2^31 (H^2 + W^2 < 2^31 is required of every image).
* A distance enters a sum as q(d2) = floor(sqrt(d2 * 2^32)), the integer square root (``math.isqrt(d2 << 32)``): the distance in
  units of 2^-16 pixel, rounded down.  A sum of q over fewer than 2^31 pixels stays below 2^63.

The scores (:func:`distance_scores`) are computed in ONE place, on the host, from those integers; they follow the published definitions
and are not pinned to a third-party implementation.  The image-wide measures (foreground against foreground) and quantile Hausdorff
distances are out of scope."""
import csv
import math

import numpy as np

from . import _capi
from .compare import _pairs_from_keys, grow_tables, overlap_pairs_host
from .imageset import in_sets

PAIR_DISTANCE_DTYPE = _capi.PAIR_DISTANCE_DTYPE
MAX_LABELS = _capi.BOUNDARY_MAX_LABELS
QUANTUM = 65536                                   # q counts 1 / 65536 pixel

PAIR_SCORE_DTYPE = np.dtype([('a', 'i4'), ('b', 'i4'), ('flags', 'i4'), ('hausdorff', 'f8'), ('hausdorff_ab', 'f8'), ('hausdorff_ba', 'f8'),
                             ('mean_surface', 'f8'), ('nsd', 'f8')])
EXPECTED_DISTANCE_DTYPE = np.dtype([('label', 'i4'), ('n_partners', 'i4'), ('hausdorff', 'f8'), ('hausdorff_label', 'i4'), ('nsd', 'f8'),
                                    ('nsd_label', 'i4')])


# ---- the definitions ------------------------------------------------------------------------------------------------------------------
def check_shape(shape, what='labels'):
    """``ValueError`` unless ``shape`` is H x W with H^2 + W^2 < 2^31 (every squared distance fits int32).  Reads the shape alone."""
    if len(shape) != 2:
        raise ValueError(f'{what}: a two-dimensional image; got {len(shape)} dimensions')
    h, w = int(shape[0]), int(shape[1])
    if h * h + w * w >= 2 ** 31:
        raise ValueError(f'{what}: shape {(h, w)}; the boundary distances take images with H^2 + W^2 < 2^31, see DESIGN.md "Limits"')


def _check_map(labels, what):
    check_shape(np.shape(labels), what)                      # (the shape alone decides first)
    labels = np.asarray(labels)
    if labels.dtype.kind not in 'iu':
        raise TypeError(f'{what}: an integer image; got {labels.dtype}')
    if labels.size and (int(labels.min()) < 0 or int(labels.max()) >= MAX_LABELS):
        raise ValueError(f'{what}: labels {int(labels.min())} .. {int(labels.max())}; the boundary distances take the labels 0 .. {MAX_LABELS - 1}, '
                         'see DESIGN.md "Limits"')
    return labels


def _check_maps(a, b):
    sa, sb = np.shape(a), np.shape(b)
    if len(sa) == 2 and len(sb) == 2 and tuple(sa) != tuple(sb):
        raise ValueError(f'the two label maps differ in shape: {tuple(sa)} and {tuple(sb)}')
    return _check_map(a, 'a'), _check_map(b, 'b')


def boundary_mask(labels):
    """The pixels that are boundary pixels of their own label (see the module's docstring)."""
    labels = _check_map(labels, 'labels')
    other = np.zeros(labels.shape, bool)
    other[1:] |= labels[1:] != labels[:-1]
    other[:-1] |= labels[:-1] != labels[1:]
    other[:, 1:] |= labels[:, 1:] != labels[:, :-1]
    other[:, :-1] |= labels[:, :-1] != labels[:, 1:]
    return other & (labels != 0)


def quantise(d2):
    """q(d2) = floor(sqrt(d2 * 2^32)) of an array of squared distances (integers >= 0), as int64: ``math.isqrt``, value by value."""
    d2 = np.asarray(d2, np.int64)
    values, inverse = np.unique(d2.reshape(-1), return_inverse=True)
    return np.array([math.isqrt(int(v) << 32) for v in values], np.int64)[inverse].reshape(d2.shape)


def _lists_from_mask(labels, mask):
    """(present non-background labels ascending, offsets, (row, col) int32 of the pixels of ``mask`` label by label in raster order)."""
    present = np.unique(labels[labels != 0]).astype(np.int32)
    rr, cc = np.nonzero(mask)
    lab = labels[rr, cc]
    order = np.argsort(lab, kind='stable')                   # (np.nonzero lists in raster order; the stable sort keeps it per label)
    coords = np.stack([rr[order], cc[order]], axis=1).astype(np.int32).reshape(-1, 2)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(np.searchsorted(present, lab), minlength=len(present)))]).astype(np.int64)
    return present, offsets, coords


def label_boundaries_host(labels):
    """The boundary pixels of every label of a label map (integer, labels 0 .. 65535, 0 the background): ``(present_labels, offsets,
    coords)`` with the present labels other than 0 in ascending order (int32) and the boundary pixels of label ``present_labels[k]`` as
    ``coords[offsets[k]:offsets[k + 1]]``, ``(row, col)`` int32 in raster order.

    A pixel of label l is a boundary pixel iff one of its 4-neighbours inside the image carries another label; the image border makes
    no boundary.  A one-pixel object is its own boundary; a hole has an inner boundary; two touching objects each have a boundary along
    the contact; a label that fills the whole image has none (an empty range)."""
    labels = _check_map(labels, 'labels')
    return _lists_from_mask(labels, boundary_mask(labels))


def _check_pairs(pairs):
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    if pairs.size and (pairs.min() < 1 or pairs.max() >= MAX_LABELS):
        raise ValueError(f'pairs: labels 1 .. {MAX_LABELS - 1} (the background has no boundary)')
    return pairs


def _default_pairs(table):
    """The pairs of non-background labels of a contingency table (``PAIR_DTYPE``), in its order."""
    fg = (table['a'] != 0) & (table['b'] != 0)
    return np.stack([table['a'][fg], table['b'][fg]], axis=1).astype(np.int64).reshape(-1, 2)


def min_d2(queries, targets, block=1 << 22):
    """Per row of ``queries`` (n x 2 integer coordinates) the smallest squared distance to a row of ``targets`` (m x 2, m >= 1), by
    comparing every query with every target (int64)."""
    queries, targets = np.asarray(queries, np.int64).reshape(-1, 2), np.asarray(targets, np.int64).reshape(-1, 2)
    out = np.empty(len(queries), np.int64)
    step = max(1, block // max(1, len(targets)))
    for lo in range(0, len(queries), step):
        q = queries[lo:lo + step]
        out[lo:lo + step] = ((q[:, None, 0] - targets[None, :, 0]) ** 2 + (q[:, None, 1] - targets[None, :, 1]) ** 2).min(axis=1)
    return out


def pair_distances_host(a, b, pairs=None):
    """The table of ``PAIR_DISTANCE_DTYPE`` of two label maps of equal shape, one 64-byte row per pair (label of ``a``, label of ``b``) in
    the order of ``pairs`` (n x 2; None: the pairs of non-background labels of ``compare.overlap_pairs_host(a, b)`` in its sorted order).

    ``boundary_a``, ``boundary_b``: the boundary pixels of each; ``max_d2_ab`` / ``max_d2_ba``: the maximum over the boundary pixels of
    one object of the minimal squared distance to the boundary of the other; ``sum_q_ab`` / ``sum_q_ba``: the sums of q(min d2) over the
    same pixels; ``nsd_num``: the sum over the pixels in exactly one of the two objects of q(min d2 to the boundary of b); ``nsd_den``:
    the same sum over the pixels in either object.  ``flags`` bit 0: the boundary of a is empty (also when the label does not occur),
    bit 1: the same for b; with a flag the maxima are -1 and the sums 0."""
    a, b = _check_maps(a, b)
    pairs = _default_pairs(overlap_pairs_host(a, b)) if pairs is None else _check_pairs(pairs)
    out = np.zeros(len(pairs), PAIR_DISTANCE_DTYPE)
    if not len(pairs):
        return out
    sides = []
    for lab in (a, b):
        present, offsets, coords = label_boundaries_host(lab)
        sides.append({int(l): coords[offsets[k]:offsets[k + 1]] for k, l in enumerate(present)})
    empty = np.zeros((0, 2), np.int32)
    for k, (la, lb) in enumerate(pairs):
        ba, bb = sides[0].get(int(la), empty), sides[1].get(int(lb), empty)
        row = out[k]
        row['a'], row['b'], row['boundary_a'], row['boundary_b'] = la, lb, len(ba), len(bb)
        row['flags'] = (1 if not len(ba) else 0) | (2 if not len(bb) else 0)
        row['max_d2_ab'] = row['max_d2_ba'] = -1
        if row['flags']:
            continue
        ab, ba_ = min_d2(ba, bb), min_d2(bb, ba)
        row['max_d2_ab'], row['max_d2_ba'] = ab.max(), ba_.max()
        row['sum_q_ab'], row['sum_q_ba'] = quantise(ab).sum(), quantise(ba_).sum()
        in_a, in_b = a == la, b == lb
        rr, cc = np.nonzero(in_a | in_b)
        q = quantise(min_d2(np.stack([rr, cc], axis=1), bb))
        row['nsd_den'] = q.sum()
        row['nsd_num'] = q[(in_a ^ in_b)[rr, cc]].sum()
    return out


# ---- scores: one function for the host and the GPU forms ------------------------------------------------------------------------------
def _nan_ratio(num, den):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(den != 0, num / np.where(den != 0, den, 1.0), np.nan)


def distance_scores(distances, expected_labels=None):
    """The scores of a table of ``PAIR_DISTANCE_DTYPE`` with ``a`` = actual and ``b`` = expected labels.  Returns a dict:

    ``pairs`` (``PAIR_SCORE_DTYPE``), one row per row of ``distances``: ``hausdorff`` = sqrt(max(max_d2_ab, max_d2_ba)) with the two
    directed values ``hausdorff_ab`` and ``hausdorff_ba``; ``mean_surface`` = (sum_q_ab + sum_q_ba) / (boundary_a + boundary_b) / 65536;
    ``nsd`` = nsd_num / nsd_den, nan on a zero denominator (identical one-pixel objects).  A flagged pair (an empty boundary) has nan
    scores and is counted in ``n_flagged``.

    ``expected`` (``EXPECTED_DISTANCE_DTYPE``), one row per expected object (``expected_labels``; None: the labels b of the table):
    ``n_partners``, its rows without a flag; ``hausdorff``, the smallest Hausdorff distance over them, and ``hausdorff_label``, the
    actual label that attains it; ``nsd`` and ``nsd_label``, the smallest NSD (over the rows with a non-zero denominator) and its
    label; nan and -1 where there is none.  Both minima are decided in integers, ties going to the smaller label: Hausdorff by
    ``max_d2``, NSD by cross-multiplication in Python integers.

    Image level: ``mean_hausdorff`` and ``mean_nsd``, the means of those two over the expected objects that have one (nan if none
    has), ``n_expected``, ``n_without_partner``, the expected objects without a partner, and ``n_flagged``.

    The scores follow the published definitions (Hausdorff distance; NSD as the sum of the boundary distances over the symmetric
    difference divided by the sum over the union).  They are UNPINNED: no third-party implementation was available to compare with, as
    with SEG and AP in ``compare``."""
    d = np.asarray(distances)
    if d.dtype != PAIR_DISTANCE_DTYPE or d.ndim != 1:
        raise TypeError('distances: a table of PAIR_DISTANCE_DTYPE, as pair_distances gives it')
    ok = d['flags'] == 0
    pairs = np.zeros(len(d), PAIR_SCORE_DTYPE)
    pairs['a'], pairs['b'], pairs['flags'] = d['a'], d['b'], d['flags']
    nan = np.full(len(d), np.nan)
    pairs['hausdorff_ab'] = np.where(ok, np.sqrt(np.maximum(d['max_d2_ab'], 0).astype(np.float64)), nan)
    pairs['hausdorff_ba'] = np.where(ok, np.sqrt(np.maximum(d['max_d2_ba'], 0).astype(np.float64)), nan)
    pairs['hausdorff'] = np.where(ok, np.sqrt(np.maximum(np.maximum(d['max_d2_ab'], d['max_d2_ba']), 0).astype(np.float64)), nan)
    pairs['mean_surface'] = np.where(ok, _nan_ratio(d['sum_q_ab'] + d['sum_q_ba'], d['boundary_a'].astype(np.int64) + d['boundary_b']) / QUANTUM, nan)
    pairs['nsd'] = np.where(ok, _nan_ratio(d['nsd_num'], d['nsd_den']), nan)
    labels = np.unique(d['b']) if expected_labels is None else np.unique(np.asarray(expected_labels, np.int64))
    expected = np.zeros(len(labels), EXPECTED_DISTANCE_DTYPE)
    expected['label'] = labels
    expected['hausdorff'] = expected['nsd'] = np.nan
    expected['hausdorff_label'] = expected['nsd_label'] = -1
    row_of = {int(l): k for k, l in enumerate(labels)}
    best_h, best_n = {}, {}                                  # per expected label: (max_d2, a), (num, den, a)
    for k in np.nonzero(ok)[0]:
        la, lb = int(d['a'][k]), int(d['b'][k])
        if lb not in row_of:
            continue
        expected['n_partners'][row_of[lb]] += 1
        h = (max(int(d['max_d2_ab'][k]), int(d['max_d2_ba'][k])), la)
        if lb not in best_h or h < best_h[lb]:
            best_h[lb] = h
        num, den = int(d['nsd_num'][k]), int(d['nsd_den'][k])
        if den > 0:
            cur = best_n.get(lb)
            if cur is None or num * cur[1] < cur[0] * den or (num * cur[1] == cur[0] * den and la < cur[2]):
                best_n[lb] = (num, den, la)
    for lb, (d2, la) in best_h.items():
        expected['hausdorff'][row_of[lb]], expected['hausdorff_label'][row_of[lb]] = math.sqrt(d2), la
    for lb, (num, den, la) in best_n.items():
        expected['nsd'][row_of[lb]], expected['nsd_label'][row_of[lb]] = num / den, la
    have_h, have_n = expected['hausdorff_label'] >= 0, expected['nsd_label'] >= 0
    return {
        'pairs': pairs, 'expected': expected, 'n_expected': len(labels),
        'mean_hausdorff': float(expected['hausdorff'][have_h].mean()) if have_h.any() else float('nan'),
        'mean_nsd': float(expected['nsd'][have_n].mean()) if have_n.any() else float('nan'),
        'n_without_partner': int((expected['n_partners'] == 0).sum()), 'n_flagged': int((~ok).sum()),
    }


def _expected_labels(b):
    b = np.asarray(b)
    return np.unique(b[b != 0])


def compare_boundaries_host(actual, expected):
    """:func:`distance_scores` of the host table of two label maps, over all expected objects."""
    return distance_scores(pair_distances_host(actual, expected), _expected_labels(expected))


def write_distance_csv(path, result):
    """The two tables of :func:`distance_scores` as one CSV, every field quoted (as ``compare.write_scores_csv``): a row per pair and per
    expected object with its table's name first, then the columns of ``PAIR_SCORE_DTYPE`` and of ``EXPECTED_DISTANCE_DTYPE`` (a column
    that the row's table does not have stays empty)."""
    cols = list(dict.fromkeys(PAIR_SCORE_DTYPE.names + EXPECTED_DISTANCE_DTYPE.names))
    with open(path, 'w', newline='') as fp:
        w = csv.writer(fp, delimiter=',', quoting=csv.QUOTE_ALL)
        w.writerow(['table'] + cols)
        for name in ('pairs', 'expected'):
            for row in result[name]:
                w.writerow([name] + [repr(row[k].item()) if k in row.dtype.names else '' for k in cols])


# ---- the GPU forms (sdsm_measure.hip) -------------------------------------------------------------------------------------------------
def _as_int32(labels, what):
    """The map as int32 for the upload.  The shape is checked first; a label outside 0 .. 65535 is left to the device, which counts it,
    unless int32 cannot hold it."""
    check_shape(np.shape(labels), what)
    labels = np.asarray(labels)
    if labels.dtype.kind not in 'iu':
        raise TypeError(f'{what}: an integer image; got {labels.dtype}')
    if labels.dtype.itemsize > 4 or labels.dtype == np.uint32:
        if labels.size and (int(labels.min()) < -2 ** 31 or int(labels.max()) >= 2 ** 31):
            raise ValueError(f'{what}: labels {int(labels.min())} .. {int(labels.max())}; the boundary distances take the labels 0 .. {MAX_LABELS - 1}, '
                             'see DESIGN.md "Limits"')
    return labels.astype(np.int32)


def work_items(pair_rows, counts_a, counts_b, chunk=None):
    """The work list of ``sdsm_pair_distances``: per pair without an empty boundary and per phase (0: boundary of a, 1: boundary of b, 2:
    pixels of a, 3: pixels of b) one item ``(pair, phase, chunk, 0)`` per ``_capi.BOUNDARY_CHUNK`` query pixels.  ``pair_rows``: n x 4
    (image, a, b, 0); ``counts_*``: per image the (labels x 2) array of (pixels, boundary pixels)."""
    chunk = _capi.BOUNDARY_CHUNK if chunk is None else int(chunk)
    pair_rows = np.asarray(pair_rows, np.int64).reshape(-1, 4)
    im, la, lb = pair_rows[:, 0], pair_rows[:, 1], pair_rows[:, 2]
    ca, cb = counts_a[im, la], counts_b[im, lb]              # n x 2
    n_queries = np.stack([ca[:, 1], cb[:, 1], ca[:, 0], cb[:, 0]], axis=1).astype(np.int64)
    n_queries[(ca[:, 1] == 0) | (cb[:, 1] == 0)] = 0
    n_chunks = (n_queries + chunk - 1) // chunk               # n x 4
    flat = n_chunks.reshape(-1)
    total = int(flat.sum())
    items = np.zeros((total, 4), np.int32)
    if total:
        slot = np.repeat(np.arange(len(flat)), flat)
        items[:, 0], items[:, 1] = slot // 4, slot % 4
        items[:, 2] = np.arange(total) - np.repeat(np.cumsum(flat) - flat, flat)
    return items


class _BoundarySet:
    """The device side of one set of up to ``_capi.MAX_SET_IMAGES`` pairs of label maps: both maps uploaded once, their per-label counts and
    pixel lists, and the launches that share them."""

    def __init__(self, *maps):
        from .render import _DeviceSet
        self.S = S = _DeviceSet([x.shape for x in maps[0]])
        self.n = n = len(maps[0])
        self.n_maps = m = len(maps)                          # 2: (a, b); 1: the lists of one map alone
        t, L = S.torch, MAX_LABELS
        self.d_map = [S.pack(x, np.int32) for x in maps]
        self.d_counts = [t.empty(n * 2 * L, dtype=t.int32, device=S.dev) for _ in range(m)]
        self.d_start = [t.empty(n * L, dtype=t.int32, device=S.dev) for _ in range(m)]
        self.d_list = [t.empty(S.total, dtype=t.int32, device=S.dev) for _ in range(m)]
        self.d_cursor = t.empty(n * 2 * L, dtype=t.int32, device=S.dev)
        self.d_bad = t.empty(m * n, dtype=t.int32, device=S.dev)
        for k in range(m):
            S.capi.check(S.L.sdsm_label_pixel_counts_multi(S.table, n, S._p(self.d_map[k]), S._p(self.d_counts[k]), S._p(self.d_bad[k * n:]), S._stream()),
                         'sdsm_label_pixel_counts_multi')
            S.capi.check(S.L.sdsm_label_pixel_lists_multi(S.table, n, S._p(self.d_map[k]), S._p(self.d_counts[k]), S._p(self.d_start[k]),
                                                          S._p(self.d_cursor), S._p(self.d_list[k]), S._stream()), 'sdsm_label_pixel_lists_multi')
        self._counts = None

    def counts(self, names=None):
        """Per map the (image, label, 2) array of (pixels, boundary pixels); raises the ``ValueError`` of the host path for labels outside
        0 .. 65535."""
        if self._counts is None:
            bad = self.d_bad.cpu().numpy().reshape(self.n_maps, self.n)
            if bad.any():
                names = list(range(self.n)) if names is None else list(names)
                raise ValueError(f'{int(bad.sum())} pixels of images {[names[i] for i in np.nonzero(bad.any(axis=0))[0]]} carry a label outside '
                                 f'0 .. {MAX_LABELS - 1}; the boundary distances take the labels 0 .. {MAX_LABELS - 1}, see DESIGN.md "Limits"')
            self._counts = [c.cpu().numpy().reshape(self.n, MAX_LABELS, 2) for c in self.d_counts]
        return self._counts

    def lists(self, k):
        """Per image of map ``k`` what :func:`label_boundaries_host` returns."""
        S = self.S
        counts = self.counts()[k]
        start = self.d_start[k].cpu().numpy().reshape(self.n, MAX_LABELS)
        packed = self.d_list[k].cpu().numpy().view(np.uint32)
        out = []
        for i in range(self.n):
            present = np.nonzero(counts[i, :, 0])[0]
            present = present[present != 0]
            lens = counts[i, present, 1].astype(np.int64)
            mine = packed[S.offsets[i]:]
            parts = [np.sort(mine[s:s + m]) for s, m in zip(start[i, present], lens)]          # (r << 16 | c: sorted is raster order)
            v = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
            coords = np.stack([v >> 16, v & 0xffff], axis=1).astype(np.int32).reshape(-1, 2)
            out.append((present.astype(np.int32), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), coords))
        return out

    def overlap(self, capacity):
        """The contingency tables of the images (``compare.PAIR_DTYPE``) from the maps already on the device."""
        S, C = self.S, self.S.C

        def launch(todo, caps):
            m = len(todo)
            table = (_capi.SetImage * m)(*[S.table[i] for i in todo])
            off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
            d_keys, d_cnt = (S.torch.empty(int(off[-1]), dtype=S.torch.int64, device=S.dev) for _ in range(2))
            d_status = S.torch.empty(2 * m, dtype=S.torch.int32, device=S.dev)
            S.capi.check(S.L.sdsm_overlap_pairs_multi(table, m, S._p(self.d_map[0]), S._p(self.d_map[1]), (C.c_int64 * m)(*[int(v) for v in off[:m]]),
                                                      (C.c_int64 * m)(*[int(c) for c in caps]), S._p(d_keys), S._p(d_cnt), S._p(d_status), S._stream()),
                         'sdsm_overlap_pairs_multi')
            keys, cnt, status = d_keys.cpu().numpy().view(np.uint64), d_cnt.cpu().numpy(), d_status.cpu().numpy().reshape(m, 2)
            return [(keys[off[i]:off[i + 1]], cnt[off[i]:off[i + 1]], status[i]) for i in range(m)]

        tables, _ = grow_tables(launch, self.n, capacity)
        return [_pairs_from_keys(keys, cnt) for keys, cnt in tables]

    def distances(self, pairs_per_image):
        """Per image the table of ``PAIR_DISTANCE_DTYPE`` of its pairs (n x 2 each)."""
        S = self.S
        sizes = [len(p) for p in pairs_per_image]
        total = int(sum(sizes))
        if not total:                                        # (no pair: no launch)
            return [np.zeros(0, PAIR_DISTANCE_DTYPE) for _ in sizes]
        rows = np.zeros((total, 4), np.int32)
        rows[:, 0] = np.repeat(np.arange(self.n), sizes)
        rows[:, 1:3] = np.concatenate([np.asarray(p, np.int64).reshape(-1, 2) for p in pairs_per_image])
        ca, cb = self.counts()
        items = work_items(rows, ca, cb)
        d_rows, d_items = S._up(rows), S._up(items if len(items) else np.zeros((1, 4), np.int32))
        d_rec = S.torch.empty(total * PAIR_DISTANCE_DTYPE.itemsize, dtype=S.torch.uint8, device=S.dev)
        S.capi.check(S.L.sdsm_pair_distances_multi(S.table, self.n, S._p(self.d_map[0]), S._p(self.d_map[1]), S._p(self.d_counts[0]), S._p(self.d_counts[1]),
                                                   S._p(self.d_start[0]), S._p(self.d_start[1]), S._p(self.d_list[0]), S._p(self.d_list[1]), total,
                                                   S._p(d_rows), len(items), S._p(d_items), S._p(d_rec), S._stream()), 'sdsm_pair_distances_multi')
        rec = d_rec.cpu().numpy().view(PAIR_DISTANCE_DTYPE)
        bounds = np.concatenate([[0], np.cumsum(sizes)])
        return [rec[bounds[i]:bounds[i + 1]].copy() for i in range(self.n)]


def _prepare(a_list, b_list):
    a_list, b_list = list(a_list), list(b_list)
    if len(a_list) != len(b_list):
        raise ValueError('one label map b per label map a')
    for a, b in zip(a_list, b_list):                         # shapes first: nothing is converted for a refused call
        check_shape(np.shape(a), 'a')
        check_shape(np.shape(b), 'b')
        if tuple(np.shape(a)) != tuple(np.shape(b)):
            raise ValueError(f'the two label maps differ in shape: {tuple(np.shape(a))} and {tuple(np.shape(b))}')
    return [_as_int32(a, 'a') for a in a_list], [_as_int32(b, 'b') for b in b_list]


def _tables_many(a_list, b_list, pairs_list=None, capacity=None, want_expected=False):
    """([distance table per image], [expected labels per image] or None)."""
    from .compare import DEFAULT_CAPACITY
    a32, b32 = _prepare(a_list, b_list)
    if pairs_list is not None:
        pairs_list = [_check_pairs(p) for p in pairs_list]
        if len(pairs_list) != len(a32):
            raise ValueError('one pair list per label map')
    capacity = DEFAULT_CAPACITY if capacity is None else int(capacity)
    out, labels = [np.zeros(0, PAIR_DISTANCE_DTYPE)] * len(a32), [np.zeros(0, np.int64)] * len(a32)
    full = [i for i, a in enumerate(a32) if a.size]          # (an empty image has an empty table and no launch)
    for i in set(range(len(a32))) - set(full):
        if pairs_list is not None and len(pairs_list[i]):
            out[i] = pair_distances_host(a32[i], b32[i], pairs_list[i])
    for part in in_sets(len(full)):
        idx = full[part]
        B = _BoundarySet([a32[i] for i in idx], [b32[i] for i in idx])
        counts = B.counts(names=idx)
        pairs = [pairs_list[i] for i in idx] if pairs_list is not None else [_default_pairs(t) for t in B.overlap(capacity)]
        for k, table in enumerate(B.distances(pairs)):
            out[idx[k]] = table
            if want_expected:
                present = np.nonzero(counts[1][k, :, 0])[0]
                labels[idx[k]] = present[present != 0]
    return out, labels if want_expected else None


def pair_distances_many(a_list, b_list, pairs_list=None, capacity=None):
    """:func:`pair_distances` for a list of pairs of label maps: the maps of up to ``_capi.MAX_SET_IMAGES`` images are uploaded once and
    shared by the overlap launch (``pairs_list`` None) and the distance launches; longer lists are split.  Per image the bytes of
    :func:`pair_distances_host`.  ``pairs_list``: None, or one pair list (n x 2) per image.  ``capacity`` as
    ``compare.overlap_pairs_many`` takes it."""
    return _tables_many(a_list, b_list, pairs_list, capacity)[0]


def pair_distances(a, b, pairs=None, capacity=None):
    """The table of ``PAIR_DISTANCE_DTYPE`` of two label maps on the GPU: the bytes of :func:`pair_distances_host`.  The set of this one
    image."""
    return pair_distances_many([a], [b], None if pairs is None else [pairs], capacity)[0]


def label_boundaries_many(labels_list):
    """:func:`label_boundaries` for a list of label maps, one set of launches per ``_capi.MAX_SET_IMAGES`` images."""
    l32 = [_as_int32(l, 'labels') for l in labels_list]
    empty = (np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros((0, 2), np.int32))
    out = [empty] * len(l32)
    full = [i for i, l in enumerate(l32) if l.size]
    for part in in_sets(len(full)):
        idx = full[part]
        maps = [l32[i] for i in idx]
        B = _BoundarySet(maps)
        B.counts(names=idx)
        for k, lists in enumerate(B.lists(0)):
            out[idx[k]] = lists
    return out


def label_boundaries(labels):
    """The boundary pixels of every label on the GPU: what :func:`label_boundaries_host` returns (the device lists are in arrival order
    and are sorted here)."""
    return label_boundaries_many([labels])[0]


def compare_boundaries_many(actual_list, expected_list, capacity=None):
    """:func:`distance_scores` of the GPU tables of a list of pairs of label maps, each over all expected objects of its image."""
    tables, labels = _tables_many(actual_list, expected_list, None, capacity, want_expected=True)
    return [distance_scores(t, l) for t, l in zip(tables, labels)]


def compare_boundaries(actual, expected, capacity=None):
    """:func:`distance_scores` of the GPU table of two label maps (``actual``, ``expected``), over all expected objects."""
    return compare_boundaries_many([actual], [expected], capacity)[0]


def compare_results_boundaries(datas, expected_list, objects='postprocessed_objects', merge_overlap_threshold=np.inf, dilate=0, **kw):
    """:func:`compare_boundaries_many` of a list of pipeline data objects against one expected label map each: the label maps of
    ``objects`` (an output name, or one list of objects per image) by ``render.rasterize_labels_many`` (background 0)."""
    from .render import rasterize_labels_many
    return compare_boundaries_many(rasterize_labels_many(datas, objects, merge_overlap_threshold, dilate), expected_list, **kw)


def compare_result_boundaries(data, expected, objects='postprocessed_objects', merge_overlap_threshold=np.inf, dilate=0, **kw):
    """:func:`compare_results_boundaries` for one pipeline data object (``objects``: an output name or a list of objects)."""
    from .render import _objects_of
    return compare_results_boundaries([data], [expected], [_objects_of(data, objects)], merge_overlap_threshold, dilate, **kw)[0]
