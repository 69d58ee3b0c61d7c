"""Skeleton tables: the midline of the objects of a segmentation with its end and branch points and its length, from objects (bit-packed
fragments, which may overlap; each is thinned alone) or from label maps, for one image or a set of images.

The other tables describe an object's size, outline, grey values, their arrangement, its surroundings, its inside and how it hangs
together; this one says what FORM it has along its own midline: how long a bent cell is, how many arms it has, whether it is a ring,
how wide it is across its axis.  As there, a result holds per object or label one row of EXACT integers (``sdsm_skeleton_record``,
include/sdsm.h), the GPU forms (sdsm_skeleton.hip) give the bytes of the ``*_host`` definitions below, the skeletons included, and
every float is made in ONE place, :func:`derive`.

**Neighbourhood code.**  For a pixel p of a binary image X, bit k of ``code(p)`` is the pixel at offset k of the ring, clockwise from
north: N(-1,0), NE(-1,1), E(0,1), SE(1,1), S(1,0), SW(1,-1), W(0,-1), NW(-1,-1).  Everything outside the object's box or the image
frame is 0.  x_k is that bit; indices are taken modulo 8.

**Removal rule.**  For a direction d of N, S, E, W (ring bits 0, 4, 2, 6) ``deletable(code, d)`` holds iff x_d = 0 (a border pixel on
side d), the 8-connectivity number, the sum over k in {0, 2, 4, 6} of (1 - x_k) (x_{k+1} or x_{k+2}), is 1 (the pixel is simple), and at
least two of the eight x_k are set (neither an end nor isolated).  41 codes of 256 are deletable per direction.

**Thinning.**  A subiteration for d removes, simultaneously, every pixel of X with ``deletable(code, d)``, the codes taken before any
removal of that subiteration.  A cycle is the four subiterations N, S, E, W.  The skeleton S of an object P is X after repeating cycles
from X = P until one whole cycle removes nothing; ``cycles`` counts the cycles that removed a pixel.  S is a subset of P with the same
8-connected parts and the same holes, and thinning S again removes nothing (tests/test_skeleton_cpu.py); a 2 x 2 block inside S can
occur at noisy junctions.

  area                      pixels of P
  n_skeleton                pixels of S
  n_end                     pixels of S with exactly one ring neighbour in S
  n_isolated                pixels of S with none
  n_branch                  pixels of S with >= 3 transitions 0 -> 1 around their ring in S (Rutovitz crossing number >= 3)
  n_orth                    unordered pairs of 4-adjacent pixels of S
  n_diag                    unordered pairs of diagonally adjacent pixels of S whose two common 4-neighbours are both outside S
  cycles                    as above
  first_row, first_col      the first pixel of S in raster order, image coordinates
  flags                     bit 0: the bounding box of P touches the image frame; bit 30: no workspace named for a box above the LDS limit
  reserved                  0

An object without a pixel has the zero row."""
import csv
import math

import numpy as np

from . import _capi
from .measure import (_check_labels, _check_shape, _keep_absent, _label_count, _label_sets, _label_table, _LabelWindows, _MeasureSet, _object_boxes, _object_sets,
                      _result_inputs)
from .postprocess import _check_boxes, _exclusive, unpack_windows

TABLE_DTYPE = np.dtype([('label', 'i4')] + _capi._SKELETON_FIELDS)     # 'label': the label, or the index of the object in its image
FRAME = 1                                                              # the flag bit
RING = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))
DIRECTIONS = (0, 4, 2, 6)                                              # N, S, E, W: the subiterations of a cycle, as ring bits


# ---- the definitions: NumPy and Python integers -------------------------------------------------------------------------------------------
def deletable(code, direction):
    """The removal rule for the neighbourhood code 0 .. 255 and the direction 0 (N), 4 (S), 2 (E) or 6 (W), stated as in the docstring."""
    code, d = int(code), int(direction)
    if not 0 <= code <= 255 or d not in DIRECTIONS:
        raise ValueError(f'deletable({code}, {d}): a code 0 .. 255 and a direction of 0, 4, 2, 6 (N, S, E, W)')
    x = [(code >> k) & 1 for k in range(8)]
    connectivity = sum((1 - x[k]) * (x[(k + 1) % 8] | x[(k + 2) % 8]) for k in (0, 2, 4, 6))
    return x[d] == 0 and connectivity == 1 and sum(x) >= 2


def _neighbours(X):
    """The eight ring neighbours of every pixel of the masks X (..., h, w), outside the box 0."""
    h, w = X.shape[-2:]
    P = np.pad(X, [(0, 0)] * (X.ndim - 2) + [(1, 1), (1, 1)])
    return [P[..., 1 + dr:1 + dr + h, 1 + dc:1 + dc + w] for dr, dc in RING]


def _removed(X, d):
    n = _neighbours(X)
    simple = sum((~n[k] & (n[k + 1] | n[(k + 2) % 8])).astype(np.int8) for k in (0, 2, 4, 6)) == 1
    many = sum(a.astype(np.int8) for a in n) >= 2
    return X & simple & many & ~n[d]


def thin_stack(masks):
    """``(skeletons, cycles)`` of a stack of masks (n, h, w), each thinned alone: the definition, on all of them at once (a mask at its
    fixed point loses nothing in the cycles the others still need)."""
    X = np.array(masks, bool)
    if X.ndim != 3:
        raise ValueError(f'masks: a stack (n, h, w); got shape {X.shape}')
    cycles = np.zeros(len(X), np.int64)
    while X.size:
        removed = np.zeros(len(X), bool)
        for d in DIRECTIONS:
            rm = _removed(X, d)
            removed |= rm.any(axis=(1, 2))
            X &= ~rm
        if not removed.any():
            break
        cycles += removed
    return X, cycles


def thin_host(mask):
    """``(skeleton, cycles)`` of a boolean h x w mask."""
    mask = np.asarray(mask)
    if mask.ndim != 2:
        raise ValueError(f'mask: a two-dimensional mask; got shape {mask.shape}')
    S, cycles = thin_stack(mask.astype(bool)[None])
    return S[0], int(cycles[0])


def _zero(n):
    return np.zeros(n, _capi.SKELETON_RECORD_DTYPE)


def _fill_record(rec, mask, offset, shape):
    """The record of the object with the fragment ``mask`` at ``offset`` of an image of ``shape``; returns its skeleton."""
    mask = np.asarray(mask, bool)
    rr, cc = np.nonzero(mask)
    if len(rr) == 0:
        return np.zeros(mask.shape, bool)
    S, cycles = thin_host(mask)
    n = _neighbours(S)
    count = sum(a.astype(np.int8) for a in n)
    transitions = sum((~n[k] & n[(k + 1) % 8]).astype(np.int8) for k in range(8))
    sr, sc = np.nonzero(S)                                                    # (row, column) order
    r0, c0 = int(offset[0]), int(offset[1])
    rec['area'], rec['n_skeleton'], rec['cycles'] = len(rr), len(sr), cycles
    rec['n_end'], rec['n_isolated'], rec['n_branch'] = int((S & (count == 1)).sum()), int((S & (count == 0)).sum()), int((S & (transitions >= 3)).sum())
    rec['n_orth'] = int((S & n[2]).sum()) + int((S & n[4]).sum())
    rec['n_diag'] = int((S & n[3] & ~n[2] & ~n[4]).sum()) + int((S & n[5] & ~n[6] & ~n[4]).sum())
    rec['first_row'], rec['first_col'] = r0 + int(sr[0]), c0 + int(sc[0])
    rec['flags'] = FRAME * int(r0 + rr.min() == 0 or c0 + cc.min() == 0 or r0 + rr.max() + 1 == shape[0] or c0 + cc.max() + 1 == shape[1])
    return S


_table = lambda labels, recs: _label_table(TABLE_DTYPE, labels, recs)


def skeleton_objects_host(objects, shape):
    """``(table, fragments)`` of a list of objects (``fg_offset``, ``fg_fragment``) of an image of ``shape``, object by object; row k is
    object k and ``fragments[k]`` the bool h x w skeleton in its box.  Objects may overlap: each is thinned alone."""
    shape = _check_shape(shape)
    objects = list(objects)
    _check_boxes(_object_boxes(objects), shape)
    recs = _zero(len(objects))
    frags = [_fill_record(recs[k:k + 1], obj.fg_fragment, obj.fg_offset, shape) for k, obj in enumerate(objects)]
    return _table(np.arange(len(objects)), recs), frags


def skeleton_labels_host(labels, background_label=0, keep_absent=False):
    """``(table, skeleton_map)`` of a label map, label by label -- a pixel of another label is outside --: the present labels without
    ``background_label`` (None: all) in ascending order; with ``keep_absent`` one row per label 0 .. max, the zero row for an absent
    label and for the background label.  ``skeleton_map``: int32, a skeleton pixel keeps its label, everything else is 0."""
    labels = _check_labels(labels)
    n = _label_count(labels)
    recs = _zero(n)
    out = np.zeros(labels.shape, np.int32)
    for l in sorted(frozenset(labels.reshape(-1).tolist())):
        if l != background_label:
            rr, cc = np.nonzero(labels == l)
            r0, c0, r1, c1 = int(rr.min()), int(cc.min()), int(rr.max()) + 1, int(cc.max()) + 1
            S = _fill_record(recs[l:l + 1], (labels == l)[r0:r1, c0:c1], (r0, c0), labels.shape)
            out[r0:r1, c0:c1][S] = l
    ls = np.arange(n) if keep_absent else np.nonzero(recs['area'] > 0)[0]
    return _table(ls, recs[ls]), out


# ---- derived columns: one function for the host and the GPU forms ----------------------------------------------------------------------
DERIVED_DTYPE = np.dtype([('label', 'i4'), ('area', 'i8'), ('on_boundary', '?'), ('skeleton_pixels', 'i8'), ('ends', 'i8'), ('branch_pixels', 'i8'),
                          ('length', 'f8'), ('mean_width', 'f8')])


def derive(table):
    """The derived columns of a table (``DERIVED_DTYPE``), on the host from its exact integers: ``length`` = n_orth + sqrt(2) n_diag (the
    length of the chain of pixel centres), ``ends`` = n_end, ``branch_pixels`` = n_branch, ``mean_width`` = area / n_skeleton,
    ``on_boundary`` from the flag.  The floats of a row without a pixel read NaN."""
    out = np.zeros(len(table), DERIVED_DTYPE)
    out['label'], out['area'], out['on_boundary'] = table['label'], table['area'], (table['flags'] & FRAME) != 0
    out['skeleton_pixels'], out['ends'], out['branch_pixels'] = table['n_skeleton'], table['n_end'], table['n_branch']
    for k, row in enumerate(table):
        if int(row['area']) == 0:
            out['length'][k] = out['mean_width'][k] = np.nan
        else:
            out['length'][k] = int(row['n_orth']) + math.sqrt(2) * int(row['n_diag'])
            out['mean_width'][k] = int(row['area']) / int(row['n_skeleton'])
    return out


def write_skeleton_csv(path, table):
    """A table with its derived columns as CSV, every field quoted (as ``measure.write_measurements_csv``), floats by ``repr``; after the
    derived columns the exact ones."""
    d = derive(table)
    exact = [n for n, _ in _capi._SKELETON_FIELDS if n not in ('area',)]
    with open(path, 'w', newline='') as fp:
        w = csv.writer(fp, delimiter=',', quoting=csv.QUOTE_ALL)
        w.writerow(list(d.dtype.names) + exact)
        for drow, row in zip(d, table):
            w.writerow([repr(v.item()) for v in drow] + [repr(row[n].item()) for n in exact])


# ---- the GPU forms (sdsm_skeleton.hip) ------------------------------------------------------------------------------------------------
def path_of(boxes):
    """The path of the kernel for the boxes (r0, c0, h, w): 0 wavefront registers, 1 LDS, 2 workspace; by the box alone."""
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    words = b[:, 2] * ((b[:, 3] + 63) // 64)
    return np.where((b[:, 2] <= _capi.SKELETON_WAVE_SIDE) & (b[:, 3] <= _capi.SKELETON_WAVE_SIDE), 0, np.where(words <= _capi.SKELETON_LDS_WORDS, 1, 2))


def workspace_words(boxes):
    """64-bit workspace words of the objects with the boxes (r0, c0, h, w): ``sdsm_skeleton_workspace_words``, 2 h ceil(w / 64) for a box
    above ``_capi.SKELETON_LDS_WORDS`` words and 0 for one that LDS or a wavefront holds."""
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    words = np.where((b[:, 2] < 1) | (b[:, 3] < 1), 0, b[:, 2] * ((b[:, 3] + 63) // 64))
    return np.where(path_of(b) == 2, 2 * words, 0).astype(np.int64)


class _SkeletonSet:
    """One set of up to ``_capi.MAX_SET_IMAGES`` images on the current device and the two calls of the skeleton kernel."""

    def __init__(self, shapes):
        self.M = _MeasureSet(shapes, None)            # (the label form takes the boxes of the labels from there)
        self.S = self.M.S
        self.n_im = len(self.S.shapes)

    def buffers(self, boxes, words, with_map=False):
        """The outputs and the workspace of a call for windows of ``words`` uint32 words; their contents do not matter."""
        S, n = self.S, len(boxes)
        ws = workspace_words(boxes)
        total = int(ws.sum())
        return dict(d_out=S.record_buffer(n, _capi.SKELETON_RECORD_DTYPE), d_skel=S.torch.empty(max(1, int(np.sum(words))), dtype=S.torch.int32, device=S.dev),
                    d_ws_off=S._up(_exclusive(ws)) if total else None, ws_words=total,
                    d_ws=S.torch.empty(total * 8, dtype=S.torch.uint8, device=S.dev) if total else None,
                    d_map=S.torch.empty(max(1, S.total), dtype=S.torch.int32, device=S.dev) if with_map else None)

    def _workspace(self, B, ws_bytes):
        """The four workspace arguments; ``ws_bytes``: the size named to the call instead of the buffer's own."""
        S = self.S
        return S._p(B['d_ws_off']), S._p(B['d_ws']), B['ws_words'], B['ws_words'] * 8 if ws_bytes is None else int(ws_bytes)

    def _download(self, B, boxes, words):
        n = len(boxes)
        recs = self.S.records(B['d_out'], n, _capi.SKELETON_RECORD_DTYPE)
        if (recs['flags'] & _capi.SKELETON_NO_WORKSPACE).any():
            raise _capi.SdsmError('an object above the LDS limit was named no workspace, see DESIGN.md "Limits"')
        bits = B['d_skel'].cpu().numpy().view(np.uint8)
        return recs, unpack_windows(bits, _exclusive(words), np.asarray(boxes).reshape(-1, 4)[:, 2:])

    def objects(self, obj_image, boxes, words, packed, B=None, ws_bytes=None):
        """(records, skeleton fragments) of the objects of the set (``packed``: the bit-packed fragments, one uint8 array of whole words
        each)."""
        S, n = self.S, len(boxes)
        B = self.buffers(boxes, words) if B is None else B
        d_objects = S.upload_objects(obj_image, boxes, words, packed)
        S.capi.check(S.L.sdsm_skeleton_objects_multi(S.table, self.n_im, n, *map(S._p, d_objects), *self._workspace(B, ws_bytes), S._p(B['d_out']), S._p(B['d_skel']),
                                                     S._stream()), 'sdsm_skeleton_objects_multi')
        return self._download(B, boxes, words)

    def labels(self, labels, background_label, B=None):
        """Per image (labels measured, number of labels, records, skeleton map) of the label maps of the set: the windows of the labels
        (``measure._LabelWindows``), then sdsm_skeleton_labels."""
        S = self.S
        w = _LabelWindows(self.M, labels, background_label, 'skeleton')
        words = (w.boxes[:, 2].astype(np.int64) * w.boxes[:, 3] + 31) // 32
        B = self.buffers(w.boxes, words, with_map=True) if B is None else B
        d_obj_label = S._up((w.idx - w.rec_off[w.obj_image]).astype(np.int32)) if len(w.idx) else None
        S.capi.check(S.L.sdsm_skeleton_labels_multi(S.table, self.n_im, *w.args(), S._p(d_obj_label), *self._workspace(B, None), S._p(B['d_out']), S._p(B['d_skel']),
                                                    S._p(B['d_map']), S._p(w.d_bad), S._stream()), 'sdsm_skeleton_labels_multi')
        recs, _ = self._download(B, w.boxes, words)
        maps = S.unpack(B['d_map'][:S.total])
        return [(ls, n_labels, recs[a:b], m) for (ls, n_labels, a, b), m in zip(w.per_image(), maps)]


def skeleton_objects_many(objects_per_image, shapes):
    """:func:`skeleton_objects` for a list of images: one launch per ``_capi.MAX_SET_IMAGES`` images (larger lists are split).  Per image
    the bytes of :func:`skeleton_objects_host`."""
    out = []
    for _, shapes_part, _, packed, first in _object_sets(objects_per_image, shapes, None):
        recs, frags = _SkeletonSet(shapes_part).objects(*packed)
        out += [(_table(np.arange(b - a), recs[a:b]), frags[a:b]) for a, b in zip(first[:-1], first[1:])]
    return out


def skeleton_objects(objects, shape):
    """``(table, fragments)`` of a list of objects (``fg_offset``, ``fg_fragment``; they may overlap) of an image of ``shape`` on the GPU,
    one wavefront or workgroup per object; row k is object k.  The bytes of :func:`skeleton_objects_host`."""
    return skeleton_objects_many([objects], [shape])[0]


def skeleton_labels_many(labels_list, background_label=0, keep_absent=False):
    """:func:`skeleton_labels` for a list of label maps, one launch per ``_capi.MAX_SET_IMAGES`` images."""
    out = []
    for _, l32, shapes, _ in _label_sets(labels_list, None):
        for ls, n_labels, recs, m in _SkeletonSet(shapes).labels(l32, background_label):
            if keep_absent:
                ls, recs = _keep_absent(_zero(n_labels), ls, recs)
            out.append((_table(ls, recs), m))
    return out


def skeleton_labels(labels, background_label=0, keep_absent=False):
    """``(table, skeleton_map)`` of a label map (integer, labels 0 .. 65535) on the GPU: the present labels without ``background_label``
    (None: all) in ascending order, or with ``keep_absent`` one row per label 0 .. max.  The bytes of :func:`skeleton_labels_host`."""
    return skeleton_labels_many([labels], background_label, keep_absent)[0]


def skeleton_result(data, objects='postprocessed_objects'):
    """The skeleton table and fragments of the objects of pipeline data: ``objects`` an output name or a list of objects."""
    return skeleton_objects(*_result_inputs(data, objects, None)[:2])
