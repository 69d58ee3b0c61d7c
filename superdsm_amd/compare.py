"""How far apart are two segmentations of one image: the contingency table of their label maps and the scores that follow from it.

The reference compares label maps by its regression rule only (``render.label_map_rows`` / ``compare_rows``: every object's area and
rounded centre must match).  Here the comparison is graded.  Its one data structure is the table of the pixel counts of every pair of
labels (a, b) that occurs -- integers only, so the GPU form (``k_overlap_pairs``, sdsm_measure.hip) gives the bytes of the host
definition :func:`overlap_pairs_host` whatever the launch or the set size.  Everything else -- per-object Jaccard indices, the Cell
Tracking Challenge's SEG, the DSB-2018 average precision over IoU thresholds, splits and merges -- is computed in ONE place,
:func:`scores`, on the host from those counts: every decision is a comparison of integers, and a quantity becomes a float by one final
division.  The scores follow the published definitions; they are not pinned to a third-party implementation."""
import csv
from fractions import Fraction

import numpy as np

from .imageset import in_sets

PAIR_DTYPE = np.dtype([('a', '<i4'), ('b', '<i4'), ('count', '<i8')])
DEFAULT_THRESHOLDS = tuple(round(0.5 + 0.05 * k, 2) for k in range(10))          # 0.5, 0.55, ..., 0.95 (DSB 2018)
# Slots of an image's global table at the first launch.  A table is 16 bytes per slot and is downloaded whole: 256 KB per image, below
# the label maps' own upload from 256 x 256 on.  It is accepted up to 8192 pairs (see grow_tables), which covers thousands of objects.
DEFAULT_CAPACITY = 1 << 14
_FREE = np.uint64(0xffffffffffffffff)

_OBJECT_FIELDS = [('label', 'i4'), ('area', 'i8'), ('best', 'i4'), ('intersection', 'i8'), ('union', 'i8'), ('jaccard', 'f8'),
                  ('seg_match', 'i4'), ('seg_jaccard', 'f8')]
EXPECTED_DTYPE = np.dtype(_OBJECT_FIELDS + [('n_split', 'i4')])
ACTUAL_DTYPE = np.dtype(_OBJECT_FIELDS + [('n_merged', 'i4')])


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def _check_map(labels, what):
    labels = np.asarray(labels)
    if labels.dtype.kind not in 'iu':
        raise TypeError(f'{what}: an integer image; got {labels.dtype}')
    if labels.ndim != 2:
        raise ValueError(f'{what}: a two-dimensional image; got {labels.ndim} dimensions')
    if labels.size and (int(labels.min()) < 0 or int(labels.max()) >= 2 ** 31):
        raise ValueError(f'{what}: labels {int(labels.min())} .. {int(labels.max())}; the comparison takes the labels 0 .. 2^31 - 1, see DESIGN.md "Limits"')
    return labels


def _check_maps(a, b):
    a, b = _check_map(a, 'a'), _check_map(b, 'b')
    if a.shape != b.shape:
        raise ValueError(f'the two label maps differ in shape: {a.shape} and {b.shape}')
    if a.size >= 2 ** 31 - 1:
        raise ValueError(f'shape {a.shape}: the comparison takes images with H * W < 2^31, see DESIGN.md "Limits"')
    return a, b


def _pairs_from_keys(keys, counts):
    """The table of the (unique) keys ``a << 32 | b`` and their counts, sorted by (a, b): the order of the keys, as labels are >= 0."""
    order = np.argsort(keys, kind='stable')
    keys = keys[order]
    pairs = np.zeros(len(keys), PAIR_DTYPE)
    pairs['a'], pairs['b'], pairs['count'] = keys >> np.uint64(32), keys & np.uint64(0xffffffff), counts[order]
    return pairs


def overlap_pairs_host(a, b):
    """The contingency table of two label maps of equal shape (integer, labels 0 .. 2^31 - 1): every pair (a, b) that occurs on at
    least one pixel with its pixel count (``PAIR_DTYPE``), pairs with a background member included, sorted by (a, b)."""
    a, b = _check_maps(a, b)
    keys, counts = np.unique((a.reshape(-1).astype(np.uint64) << np.uint64(32)) | b.reshape(-1).astype(np.uint64), return_counts=True)
    return _pairs_from_keys(keys, counts.astype(np.int64))


# ---- scores: one function for the host and the GPU forms ------------------------------------------------------------------------------
def _ratio(num, den):
    """num / den by one division of exact integers; nan where den is 0."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(den != 0, num / np.where(den != 0, den, 1.0), np.nan)


def _side(own, other, n, area_own, area_other, labels_own, dtype, count_name):
    """The per-object table of one side.  ``own`` / ``other``: per pair of non-background labels the index of this side's label (into
    ``labels_own`` / ``area_own``) and the other side's label; ``n``: its pixels; ``area_other``: the other label's area per pair."""
    out = np.zeros(len(labels_own), dtype)
    out['label'], out['area'] = labels_own, area_own
    out['best'] = out['seg_match'] = -1
    union = area_own[own] + area_other - n
    first = np.lexsort((other, -n, own))                     # per object: the largest intersection first, ties to the smaller label
    first = first[np.r_[True, own[first][1:] != own[first][:-1]]] if len(first) else first
    k = own[first]
    out['best'][k], out['intersection'][k], out['union'][k] = other[first], n[first], union[first]
    out['jaccard'] = _ratio(out['intersection'], np.where(out['best'] >= 0, out['union'], 1))
    match = 2 * n > area_own[own]                            # the CTC rule: more than half of this object; at most one label can
    out['seg_match'][own[match]] = other[match]
    out['seg_jaccard'][own[match]] = _ratio(n[match], union[match])
    inside = 2 * n > area_other                              # the other label lies mostly inside this object
    out[count_name] = np.bincount(own[inside], minlength=len(labels_own))
    return out


def scores(pairs, thresholds=DEFAULT_THRESHOLDS, background_label=0):
    """The scores of a contingency table with ``a`` = actual and ``b`` = expected labels (``PAIR_DTYPE``, as the ``overlap_pairs*``
    functions give it).  Returns a dict:

    ``expected`` (``EXPECTED_DTYPE``), one row per expected label other than the background: ``label``, ``area``; ``best``, the actual
    label other than the background with the largest intersection (ties to the smaller label; -1 if the object lies on background
    only) with ``intersection``, ``union`` and ``jaccard``; ``seg_match``, the one actual label with 2 * intersection > area (the rule
    of the Cell Tracking Challenge), else -1, and its ``seg_jaccard``, else 0; ``n_split``, the number of actual labels that lie mostly
    (2 * intersection > their area) inside this object.  ``actual`` (``ACTUAL_DTYPE``): the mirror image, with ``n_merged``.

    Image level: ``n_actual``, ``n_expected``; ``seg``, the mean of ``seg_jaccard`` over the expected objects; ``foreground_dice`` and
    ``foreground_jaccard`` of the pixels other than the background; per threshold t (arrays in the order of ``thresholds``): ``tp``, the
    pairs of non-background labels with intersection >= t * union, ``fp`` = n_actual - tp, ``fn`` = n_expected - tp, ``precision``,
    ``recall``, ``f1`` and ``ap`` = tp / (tp + fp + fn) (DSB 2018); ``mean_ap``; ``splits`` / ``merges``, the expected / actual objects
    with ``n_split`` / ``n_merged`` >= 2; ``missed`` / ``spurious``, the expected / actual objects with ``best`` == -1.  A zero
    denominator gives nan.

    Every decision is a comparison of integers: a threshold is taken as the nearest fraction p / q with q <= 10^6 and tested as
    intersection * q >= p * union.  Thresholds below 0.5 raise ``ValueError``: matches are then no longer one to one."""
    pairs = np.asarray(pairs)
    if pairs.dtype != PAIR_DTYPE or pairs.ndim != 1:
        raise TypeError('pairs: a table of PAIR_DTYPE, as overlap_pairs gives it')
    fracs = [Fraction(float(t)).limit_denominator(10 ** 6) for t in thresholds]
    if any(not Fraction(1, 2) <= f <= 1 for f in fracs):
        raise ValueError(f'thresholds {tuple(thresholds)}: 0.5 <= t <= 1 required; below 0.5 matches are not one to one (an assignment is out of scope)')
    bg = int(background_label)
    a, b, n = pairs['a'].astype(np.int64), pairs['b'].astype(np.int64), pairs['count'].astype(np.int64)
    labels_a, ia = np.unique(a, return_inverse=True)
    labels_b, ib = np.unique(b, return_inverse=True)
    area_a, area_b = np.zeros(len(labels_a), np.int64), np.zeros(len(labels_b), np.int64)      # row and column sums, in integers
    np.add.at(area_a, ia, n)
    np.add.at(area_b, ib, n)
    fg = (a != bg) & (b != bg)
    # indices among the non-background labels of each side
    keep_a, keep_b = labels_a != bg, labels_b != bg
    pos_a, pos_b = np.cumsum(keep_a) - 1, np.cumsum(keep_b) - 1
    oa, ob, on = pos_a[ia[fg]], pos_b[ib[fg]], n[fg]
    la, lb, ar_a, ar_b = labels_a[keep_a], labels_b[keep_b], area_a[keep_a], area_b[keep_b]
    expected = _side(ob, la[oa], on, ar_b, ar_a[oa], lb, EXPECTED_DTYPE, 'n_split')
    actual = _side(oa, lb[ob], on, ar_a, ar_b[ob], la, ACTUAL_DTYPE, 'n_merged')
    n_actual, n_expected = len(la), len(lb)
    union = ar_a[oa] + ar_b[ob] - on
    tp = np.array([int((on * f.denominator >= f.numerator * union).sum()) for f in fracs], np.int64)
    fp, fn = n_actual - tp, n_expected - tp
    fg_a, fg_b, both = int(ar_a.sum()), int(ar_b.sum()), int(on.sum())
    ap = _ratio(tp, tp + fp + fn)
    return {
        'expected': expected, 'actual': actual, 'n_actual': n_actual, 'n_expected': n_expected,
        'seg': float(expected['seg_jaccard'].sum() / n_expected) if n_expected else float('nan'),
        'foreground_dice': float(_ratio(2 * both, fg_a + fg_b)), 'foreground_jaccard': float(_ratio(both, fg_a + fg_b - both)),
        'thresholds': np.array([float(t) for t in thresholds], np.float64), 'tp': tp, 'fp': fp, 'fn': fn,
        'precision': _ratio(tp, tp + fp), 'recall': _ratio(tp, tp + fn), 'f1': _ratio(2 * tp, 2 * tp + fp + fn), 'ap': ap,
        'mean_ap': float(ap.mean()) if len(ap) else float('nan'),
        'splits': int((expected['n_split'] >= 2).sum()), 'merges': int((actual['n_merged'] >= 2).sum()),
        'missed': int((expected['best'] == -1).sum()), 'spurious': int((actual['best'] == -1).sum()),
    }


def compare_labels_host(actual, expected, **kw):
    """:func:`scores` of the host table of two label maps."""
    return scores(overlap_pairs_host(actual, expected), **kw)


def write_scores_csv(path, result):
    """The two per-object tables of :func:`scores` as one CSV, every field quoted (as ``measure.write_measurements_csv``): a row per
    object with its table's name first, the columns the tables share, then ``n_split`` (expected rows) and ``n_merged`` (actual rows)."""
    shared = [name for name, _ in _OBJECT_FIELDS]
    with open(path, 'w', newline='') as fp:
        w = csv.writer(fp, delimiter=',', quoting=csv.QUOTE_ALL)
        w.writerow(['table'] + shared + ['n_split', 'n_merged'])
        for name, own in (('expected', 'n_split'), ('actual', 'n_merged')):
            for row in result[name]:
                w.writerow([name] + [repr(row[k].item()) for k in shared] + [repr(int(row[own])) if k == own else '' for k in ('n_split', 'n_merged')])


# ---- the GPU forms (k_overlap_pairs, sdsm_measure.hip) -----------------------------------------------------------------------------
def grow_tables(launch, n_images, capacity, names=None):
    """The tables of ``n_images`` images from ``launch(indices, capacities)``, which gives per index ``(keys, counts, status)``: the
    whole table (uint64 keys, free slots ~0; int64 counts) and the two status words of ``sdsm_overlap_pairs``.  An image whose launch
    dropped a pair (status[1] != 0) is launched again, alone with the others of its kind, at twice the capacity, and so is one whose
    table came back more than half full: past that load the probe sequences of the table (linear probing, 1 / (1 - load)^2) and the
    time of the launch grow without bound, so the capacity an image ends at is one at which its table works as designed.  This ends: a
    table of >= 2 * H * W slots neither overflows nor is more than half full.  Pixels with a negative label raise ``ValueError``.
    (the images are named by ``names``, else by their index).  Returns ([(keys, counts) of the occupied slots per image], [capacity
    per image])."""
    names = list(range(n_images)) if names is None else list(names)
    caps = [int(capacity)] * n_images
    done = [None] * n_images
    todo = list(range(n_images))
    while todo:
        out = launch(todo, [caps[i] for i in todo])
        bad = [(i, int(st[0])) for i, (_, _, st) in zip(todo, out) if st[0]]
        if bad:
            raise ValueError(f'{sum(n for _, n in bad)} pixels of images {[names[i] for i, _ in bad]} carry a negative label')
        again = []
        for i, (keys, counts, st) in zip(todo, out):
            used = keys != _FREE
            if st[1] != 0 or 2 * int(used.sum()) > caps[i]:
                caps[i] *= 2
                again.append(i)
            else:
                done[i] = (keys[used], counts[used])
        todo = again
    return done, caps


def _launch_set(a32, b32, capacities):
    """One launch for a set of up to ``_capi.MAX_SET_IMAGES`` pairs of int32 label maps: per image (keys, counts, status)."""
    from .render import _DeviceSet
    S = _DeviceSet([x.shape for x in a32])
    n = len(a32)
    d_a, d_b = S.pack(a32, np.int32), S.pack(b32, np.int32)
    off = np.concatenate([[0], np.cumsum(capacities)]).astype(np.int64)
    d_keys = S.torch.empty(int(off[-1]), dtype=S.torch.int64, device=S.dev)
    d_counts = S.torch.empty(int(off[-1]), dtype=S.torch.int64, device=S.dev)
    d_status = S.torch.empty(2 * n, dtype=S.torch.int32, device=S.dev)
    S.capi.check(S.L.sdsm_overlap_pairs_multi(S.table, n, S._p(d_a), S._p(d_b), (S.C.c_int64 * n)(*[int(v) for v in off[:n]]),
                                              (S.C.c_int64 * n)(*[int(c) for c in capacities]), S._p(d_keys), S._p(d_counts), S._p(d_status),
                                              S._stream()), 'sdsm_overlap_pairs_multi')
    keys, counts, status = d_keys.cpu().numpy().view(np.uint64), d_counts.cpu().numpy(), d_status.cpu().numpy().reshape(n, 2)
    return [(keys[off[i]:off[i + 1]], counts[off[i]:off[i + 1]], status[i]) for i in range(n)]


def _as_int32(labels, what):
    labels = np.asarray(labels)
    if labels.dtype.kind not in 'iu':
        raise TypeError(f'{what}: an integer image; got {labels.dtype}')
    if labels.ndim != 2:
        raise ValueError(f'{what}: a two-dimensional image; got {labels.ndim} dimensions')
    if labels.dtype.itemsize > 4 or labels.dtype == np.uint32:
        if labels.size and (int(labels.min()) < -2 ** 31 or int(labels.max()) >= 2 ** 31):
            raise ValueError(f'{what}: the comparison takes the labels 0 .. 2^31 - 1, see DESIGN.md "Limits"')
    return labels.astype(np.int32)                           # (a negative label stays negative: the kernel counts it)


def overlap_pairs_many(a_list, b_list, capacity=None, info=None):
    """:func:`overlap_pairs` for a list of pairs of label maps: one launch per ``_capi.MAX_SET_IMAGES`` images (longer lists are split).
    Per image the bytes of :func:`overlap_pairs_host`.  ``capacity``: the slots of an image's table at the first launch, a power of two
    (None: ``DEFAULT_CAPACITY``); it is doubled, for the images that need it alone, until the table holds all pairs at most half full
    (:func:`grow_tables`).  ``info``: a dict that receives ``capacity``, the slots each image ended at."""
    a_list, b_list = list(a_list), list(b_list)
    if len(a_list) != len(b_list):
        raise ValueError('one label map b per label map a')
    capacity = DEFAULT_CAPACITY if capacity is None else int(capacity)
    if capacity < 1 or capacity & (capacity - 1):
        raise ValueError(f'capacity {capacity}: a power of two >= 1')
    a32, b32 = [_as_int32(a, 'a') for a in a_list], [_as_int32(b, 'b') for b in b_list]
    for a, b in zip(a32, b32):
        if a.shape != b.shape:
            raise ValueError(f'the two label maps differ in shape: {a.shape} and {b.shape}')
        if a.size >= 2 ** 31 - 1:
            raise ValueError(f'shape {a.shape}: the comparison takes images with H * W < 2^31, see DESIGN.md "Limits"')
    out, caps = [None] * len(a32), [capacity] * len(a32)
    full = [i for i, a in enumerate(a32) if a.size]          # (an empty image has an empty table and no launch)
    for i in range(len(a32)):
        if not a32[i].size:
            out[i] = np.zeros(0, PAIR_DTYPE)
    for part in in_sets(len(full)):
        idx = full[part]
        tables, c = grow_tables(lambda todo, cs: _launch_set([a32[idx[k]] for k in todo], [b32[idx[k]] for k in todo], cs), len(idx), capacity, names=idx)
        for k, (keys, counts) in enumerate(tables):
            out[idx[k]], caps[idx[k]] = _pairs_from_keys(keys, counts), c[k]
    if info is not None:
        info['capacity'] = caps
    return out


def overlap_pairs(a, b, capacity=None, info=None):
    """The contingency table of two label maps on the GPU: the bytes of :func:`overlap_pairs_host`.  The set of this one image."""
    return overlap_pairs_many([a], [b], capacity, info)[0]


def compare_labels_many(actual_list, expected_list, capacity=None, **kw):
    """:func:`scores` of the GPU tables of a list of pairs of label maps."""
    return [scores(p, **kw) for p in overlap_pairs_many(actual_list, expected_list, capacity)]


def compare_labels(actual, expected, capacity=None, **kw):
    """:func:`scores` of the GPU table of two label maps (``actual``, ``expected``)."""
    return compare_labels_many([actual], [expected], capacity, **kw)[0]


def compare_results(datas, expected_list, objects='postprocessed_objects', merge_overlap_threshold=np.inf, dilate=0, **kw):
    """:func:`scores` of a list of pipeline data objects against one expected label map each: the label maps of ``objects`` (an output
    name, or one list of objects per image) by ``render.rasterize_labels_many`` (background 0), then :func:`compare_labels_many`."""
    from .render import rasterize_labels_many
    return compare_labels_many(rasterize_labels_many(datas, objects, merge_overlap_threshold, dilate), expected_list, **kw)


def compare_result(data, expected, objects='postprocessed_objects', merge_overlap_threshold=np.inf, dilate=0, **kw):
    """:func:`compare_results` for one pipeline data object (``objects``: an output name or a list of objects)."""
    from .render import _objects_of
    return compare_results([data], [expected], [_objects_of(data, objects)], merge_overlap_threshold, dilate, **kw)[0]
