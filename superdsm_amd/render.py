"""Label maps of segmentation results and the reference's regression metric.

``rasterize_labels`` restates superdsm/render.py:388-451 (objects -> uniquely labelled uint16 image: optional merging of
strongly overlapping objects, overlapping pixels handed to the nearest object by a marker-based watershed on the distance map,
exactly coinciding objects kept).  ``label_map_rows`` / ``compare_rows`` restate tests/regression/validate.py:31-36,76-80: a
label map is summarised as the SET of rows (area, round(centre x, 1), round(centre y, 1)) -- strings -- and two results agree iff
the sets are equal; this is how the reference's committed ``tests/regression/expected/<host>/<task>/<image>.csv`` files are
compared.  Host code (the reference's own is NumPy / scikit-image on the host too); the watershed of scikit-image is replaced by
a priority flood with its documented semantics (4-connectivity, ties by insertion order)."""
import csv
import heapq
import math

import numpy as np
import scipy.ndimage as ndi

from . import _morph
from .imageset import SetLayout, in_sets
from .postprocess import _exclusive, grown_windows, pack_object_sets, window_words


def render_objects_foregrounds(shape, objects):
    """One full-image bool mask per object, in turn (superdsm/_aux.py:51-56)."""
    for obj in objects:
        foreground = np.zeros(shape, bool)
        obj.fill_foreground(foreground)
        yield foreground


def rasterize_objects(data, objects, dilate=0):
    """Yields the (optionally dilated / eroded) masks of the objects that have any foreground (render.py:368-385)."""
    if isinstance(objects, str):
        objects = list(data[objects])
    for foreground in render_objects_foregrounds(data['g_raw'].shape, objects):
        if dilate > 0:
            foreground = _morph.binary_dilation(foreground, _morph.disk(dilate))
        elif dilate < 0:
            foreground = _morph.binary_erosion(foreground, _morph.disk(-dilate))
        if foreground.any():
            yield foreground.copy()


def _watershed(image, markers, mask):
    """Marker-based watershed by priority flood (what ``skimage.segmentation.watershed(image, markers, mask=mask)`` computes with
    its defaults): pixels enter a heap keyed by (image value, insertion order); a popped pixel gives its label to its unlabelled
    4-neighbours inside ``mask``, which enter the heap in turn.  Only marker pixels with an unlabelled neighbour can ever label
    anything, so only those are queued (in raster order, which keeps the relative insertion order of the full algorithm)."""
    out = np.where(mask, markers, 0).astype(np.int64)
    todo = mask & (out == 0)
    if not todo.any():
        return out
    H, W = out.shape
    near = ndi.binary_dilation(todo, structure=np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)) & (out > 0)
    heap = []
    age = 0
    for r, c in zip(*np.nonzero(near)):
        heap.append((float(image[r, c]), age, int(r), int(c)))
        age += 1
    heapq.heapify(heap)
    while heap:
        _, _, r, c = heapq.heappop(heap)
        lab = out[r, c]
        for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
            if 0 <= rr < H and 0 <= cc < W and out[rr, cc] == 0 and mask[rr, cc]:
                out[rr, cc] = lab
                heapq.heappush(heap, (float(image[rr, cc]), age, rr, cc))
                age += 1
    return out


def rasterize_labels(data, objects='postprocessed_objects', merge_overlap_threshold=np.inf, dilate=0, background_label=0):
    """Integer image of uniquely labelled segmentation masks (render.py:388-451).

    :param data: pipeline data (``g_raw`` gives the shape).
    :param objects: name of the output to rasterise, or a list of objects with ``fill_foreground``.
    :param merge_overlap_threshold: pairs overlapping by more than this fraction of the smaller one are merged.
    :param dilate: dilate (> 0) or erode (< 0) every mask by a disk of this radius first.
    :param background_label: label of the background (non-positive).
    """
    assert background_label <= 0
    objects = list(rasterize_objects(data, objects, dilate))

    pairs = [(i1, i2) for i1 in range(len(objects)) for i2 in range(i1)] if merge_overlap_threshold <= 1 else []
    inter = [np.logical_and(objects[i1], objects[i2]).sum() for i1, i2 in pairs]
    members = _merge_members(len(objects), pairs, inter, [obj.sum() for obj in objects], merge_overlap_threshold)
    objects = [np.sum([objects[k] for k in ks], axis=0) > 0 for ks in members]

    result = np.zeros(data['g_raw'].shape, 'uint16')
    if len(objects) > 0:
        overlaps = np.sum(objects, axis=0) > 1
        for l, obj in enumerate(objects, 1):
            result[obj] = l
        background = result == 0
        result[overlaps] = 0
        dist = ndi.distance_transform_edt(result == 0)
        result = _watershed(dist, result, ~background)
        assert not (result < 0).any() and not (result >= 2 ** 16).any()
        result = result.astype('uint16')
    # two or more objects that coincide exactly have been eliminated by the steps above: give them a label each (render.py:443-447)
    for obj in objects:
        lost = ((result > 0) * 1 - (obj > 0) * 1 < 0)
        if lost.any():
            result[lost] = result.max() + 1
    # (the reference assigns the non-positive background label into its uint16 image: under the NumPy it pins, 1.20, a negative
    #  value wraps -- background_label = -1 reads 65535 --, kept here)
    result[result == 0] = np.array(background_label).astype('uint16')
    return result


# ---- label maps on the GPU (render.py:388-451 in kernel phases, sdsm_render.hip) ------------------------------------------------------
def _check_radius(radius, what):
    if float(radius) != int(radius) or abs(int(radius)) > 16:
        raise NotImplementedError(f'{what} = {radius!r}: the GPU label maps and overlays take integer disk radii up to 16 only, see DESIGN.md "Limits"')
    return int(radius)


class _DeviceSet:
    """One set of up to ``_capi.MAX_SET_IMAGES`` images on the current device: its packed layout (:class:`SetLayout`) and what every
    call of a ``*_multi`` entry point needs."""

    def __init__(self, shapes):
        import ctypes as C
        import torch
        from . import _capi
        self.C, self.torch, self.capi, self.L = C, torch, _capi, _capi.lib()
        self.layout = SetLayout(shapes)
        self.shapes, self.table, self.offsets, self.total = self.layout.shapes, self.layout.table, self.layout.offsets, self.layout.total
        self.dev = torch.device('cuda', torch.cuda.current_device())

    def _up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def _p(self, t):
        return self.C.c_void_p(t.data_ptr() if t is not None else None)

    def _stream(self):
        return self.C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def pack(self, arrays, dtype, channels=1):
        return self._up(self.layout.pack(arrays, dtype, channels))

    def unpack(self, d, channels=1, tail=()):
        return self.layout.unpack(d.cpu().numpy(), channels, tail)

    def upload_objects(self, obj_image, boxes, words, packed):
        """The packed objects of a call (``postprocess.pack_object_sets``) on the device: ``(d_obj_image, d_boxes, d_bits_off, d_bits)``,
        the offsets the exclusive scan of the word counts, the bits of no object four bytes nobody reads.  ``packed`` None: room for
        the words instead, for windows that a call fills on the device.  The caller keeps the arrays until its download."""
        if packed is None:
            d_bits = self.torch.empty(max(1, int(np.sum(words))), dtype=self.torch.int32, device=self.dev)
        else:
            d_bits = self._up(np.concatenate(packed) if len(packed) else np.zeros(4, np.uint8))
        return self._up(np.asarray(obj_image, np.int32)), self._up(np.asarray(boxes, np.int32).reshape(-1, 4)), self._up(_exclusive(words)), d_bits

    def record_buffer(self, n, dtype):
        """Room for ``n`` records of ``dtype`` (for one where n is 0); its contents do not matter."""
        return self.torch.empty(max(1, n) * dtype.itemsize, dtype=self.torch.uint8, device=self.dev)

    def records(self, d_out, n, dtype):
        """The first ``n`` records of a record buffer, downloaded."""
        return d_out.cpu().numpy()[:n * dtype.itemsize].view(dtype).copy()

    def pack_bases(self, bases):
        """The images under an overlay, H x W or H x W x 3 each: (packed float64 buffer, channels); grey ones are tripled if any has colour."""
        ch = 3 if any(b.ndim == 3 for b in bases) else 1
        return self.pack([b if b.ndim == 3 or ch == 1 else np.dstack([b] * 3) for b in bases], np.float64, ch), ch


class _GpuSet(_DeviceSet):
    """The device side of the label maps of one set: the packed pixel buffers, the uploaded objects and one method per kernel phase.
    (The CPU tests replace this class by a host restatement to exercise the orchestration.)"""

    def __init__(self, shapes):
        super().__init__(shapes)
        self.d_label = self.torch.empty(self.total, dtype=self.torch.int32, device=self.dev)
        self.d_cover = self.torch.empty(self.total, dtype=self.torch.uint8, device=self.dev)
        self.d_target = self.torch.empty(self.total, dtype=self.torch.uint8, device=self.dev)
        self.n = 0

    def load(self, obj_image, boxes, words, packed):
        self.n = len(boxes)
        self.obj_image, self.boxes, self.bits_off = np.asarray(obj_image, np.int32), np.asarray(boxes, np.int32).reshape(-1, 4), _exclusive(words)     # (for select)
        self.d_obj_image, self.d_boxes, self.d_bits_off, self.d_bits = self.upload_objects(obj_image, boxes, words, packed)

    def _objects(self):
        self.d_obj_image, self.d_boxes, self.d_bits_off = self._up(self.obj_image), self._up(self.boxes), self._up(self.bits_off)

    def morph(self, radius):
        """Phase 1: every object dilated / eroded; the objects become their windows.  Returns (window boxes, areas)."""
        H, W = (np.array([s[k] for s in self.shapes], np.int64)[self.obj_image] for k in (0, 1))
        win = grown_windows(self.boxes, H, W, abs(radius))
        new_words = window_words(win)
        new_off = _exclusive(new_words)
        d_new_off = self._up(new_off)
        d_new = self.torch.empty(max(1, int(new_words.sum())) * 4, dtype=self.torch.uint8, device=self.dev)
        d_area = self.torch.empty(max(1, self.n), dtype=self.torch.int32, device=self.dev)
        self.capi.check(self.L.sdsm_render_morph_multi(self.table, len(self.shapes), self.n, self._p(self.d_obj_image), self._p(self.d_boxes), self._p(self.d_bits_off),
                                                       self._p(self.d_bits), int(radius), self._p(d_new_off), self._p(d_new), self._p(d_area), self._stream()), 'sdsm_render_morph_multi')
        areas = d_area.cpu().numpy()[:self.n].astype(np.int64)
        self.boxes, self.bits_off, self.d_bits = win.astype(np.int32), new_off, d_new
        self._objects()
        return self.boxes, areas

    def select(self, keep):
        self.obj_image, self.boxes, self.bits_off = self.obj_image[keep], self.boxes[keep], self.bits_off[keep]
        self.n = len(self.boxes)
        self._objects()

    def overlaps(self, pairs):
        """Phase 2: |A n B| of every pair (global object indices)."""
        pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        if len(pairs) == 0:
            return np.zeros(0, np.int64)
        d_pairs = self._up(pairs)
        d_inter = self.torch.empty(len(pairs), dtype=self.torch.int32, device=self.dev)
        self.capi.check(self.L.sdsm_render_overlaps(len(pairs), self._p(d_pairs), self._p(self.d_boxes), self._p(self.d_bits_off), self._p(self.d_bits), self._p(d_inter),
                                                    self._stream()), 'sdsm_render_overlaps')
        return d_inter.cpu().numpy().astype(np.int64)

    def paint(self, obj_label):
        """Phase 3."""
        self.d_obj_label = self._up(np.asarray(obj_label, np.int32))
        self.capi.check(self.L.sdsm_render_paint_multi(self.table, len(self.shapes), self.n, self._p(self.d_obj_image), self._p(self.d_boxes), self._p(self.d_bits_off),
                                                       self._p(self.d_bits), self._p(self.d_obj_label), self._p(self.d_label), self._p(self.d_cover), self._p(self.d_target),
                                                       self._stream()), 'sdsm_render_paint_multi')

    def flood_inputs(self, capacity):
        """Phases 4 and 5: the distance map and, per image, the entries of the flood sorted by raster index."""
        n_im = len(self.shapes)
        nbytes = self.L.sdsm_edt_exact_workspace_bytes_multi(self.table, n_im)
        ws = self.torch.empty(max(1, nbytes), dtype=self.torch.uint8, device=self.dev)
        d_dist = self.torch.empty(self.total, dtype=self.torch.float64, device=self.dev)
        self.capi.check(self.L.sdsm_edt_exact_multi(self.table, n_im, self._p(self.d_target), self._p(d_dist), self._p(ws), nbytes, self._stream()), 'sdsm_edt_exact_multi')
        cap = (self.C.c_int64 * n_im)(*[int(c) for c in capacity])
        cap_off = _exclusive(np.asarray(capacity, np.int64))
        d_entries = self.torch.empty(max(1, int(np.sum(capacity))) * 16, dtype=self.torch.uint8, device=self.dev)
        d_counts = self.torch.empty(n_im, dtype=self.torch.int32, device=self.dev)
        self.capi.check(self.L.sdsm_render_compact_multi(self.table, n_im, self._p(self.d_label), self._p(self.d_cover), self._p(d_dist), cap, self._p(d_entries),
                                                         self._p(d_counts), self._stream()), 'sdsm_render_compact_multi')
        counts = d_counts.cpu().numpy()
        if (counts > np.asarray(capacity)).any():
            raise self.capi.SdsmError('sdsm_render_compact_multi: more flood pixels than object pixels')
        out = []
        for i in range(n_im):
            if counts[i] == 0:
                out.append(np.zeros(0, self.capi.RENDER_ENTRY_DTYPE))
                continue
            e = d_entries[16 * int(cap_off[i]):16 * (int(cap_off[i]) + int(counts[i]))].cpu().numpy().view(self.capi.RENDER_ENTRY_DTYPE)
            out.append(e[np.argsort(e['idx'], kind='stable')])
        return out

    def scatter(self, pix, lab):
        if len(pix) == 0:
            return
        d_pix, d_lab = self._up(np.asarray(pix, np.int64)), self._up(np.asarray(lab, np.int32))
        self.capi.check(self.L.sdsm_render_scatter(len(pix), self._p(d_pix), self._p(d_lab), self._p(self.d_label), self._stream()), 'sdsm_render_scatter')

    def lost(self, obj_group, n_groups):
        """Phase 6, counting: (pixels without a label per group 1 .. n_groups, highest label per image)."""
        d_group = self._up(np.asarray(obj_group, np.int32))
        d_lost = self.torch.empty(n_groups + 1, dtype=self.torch.int32, device=self.dev)
        d_max = self.torch.empty(len(self.shapes), dtype=self.torch.int32, device=self.dev)
        self.capi.check(self.L.sdsm_render_lost_multi(self.table, len(self.shapes), self.n, self._p(self.d_obj_image), self._p(self.d_boxes), self._p(self.d_bits_off),
                                                      self._p(self.d_bits), self._p(d_group), n_groups, self._p(self.d_label), self._p(d_lost), self._p(d_max), self._stream()),
                        'sdsm_render_lost_multi')
        return d_lost.cpu().numpy(), d_max.cpu().numpy()

    def fill(self, sel, new_label):
        """Phase 6, filling: the unlabelled pixels of the objects ``sel`` get ``new_label``; returns whether there were any."""
        d_sel = self._up(np.asarray(sel, np.int32))
        d_filled = self.torch.empty(1, dtype=self.torch.int32, device=self.dev)
        self.capi.check(self.L.sdsm_render_fill_multi(self.table, len(self.shapes), len(sel), self._p(d_sel), self._p(self.d_obj_image), self._p(self.d_boxes),
                                                      self._p(self.d_bits_off), self._p(self.d_bits), self._p(self.d_obj_label), int(new_label), self._p(self.d_label),
                                                      self._p(d_filled), self._stream()), 'sdsm_render_fill_multi')
        return int(d_filled.cpu().numpy()[0]) > 0

    def finish(self, background_label):
        """Phase 7 and the download: the uint16 label map of every image."""
        d_out = self.torch.empty(self.total, dtype=self.torch.int16, device=self.dev)
        self.capi.check(self.L.sdsm_render_finish(self.total, self._p(self.d_label), int(background_label), self._p(d_out), self._stream()), 'sdsm_render_finish')
        return [a.view(np.uint16) for a in self.unpack(d_out)]

    def region_flags(self, labels, radius, background_label):
        """rasterize_regions for the set (kind 3 of the overlay kernel): (borders, background) per image."""
        d_labels = self.pack(labels, np.int32)
        d_out = self.torch.empty(self.total, dtype=self.torch.uint8, device=self.dev)
        bgc = (self.C.c_double * 4)(0, 0, 0, 0) if background_label is not None else None
        self.capi.check(self.L.sdsm_render_overlay_multi(self.table, len(self.shapes), self._p(d_labels), None, 1, 3, int(radius), None, bgc,
                                                         int(background_label if background_label is not None else 0), self._p(d_out), self._stream()), 'sdsm_render_overlay_multi')
        return [((f & 1) != 0, (f & 2) != 0) for f in self.unpack(d_out)]

    def overlay(self, labels, bases, kind, radius, color, bg, background_label):
        """The overlay kernel for the set.  ``labels``: None (the label maps this set holds) or one integer array per image;
        ``bases``: one float64 array per image, H x W or H x W x 3."""
        n_im = len(self.shapes)
        d_labels = self.pack(labels, np.int32) if labels is not None else self.d_label
        d_base, ch = self.pack_bases(bases)
        d_out = self.torch.empty(self.total * 3, dtype=self.torch.uint8, device=self.dev)
        col = (self.C.c_double * 3)(*[float(v) for v in color])
        bgc = (self.C.c_double * 4)(*[float(v) for v in bg]) if bg is not None else None
        self.capi.check(self.L.sdsm_render_overlay_multi(self.table, n_im, self._p(d_labels), self._p(d_base), ch, int(kind), int(radius), col, bgc,
                                                         int(background_label if background_label is not None else 0), self._p(d_out), self._stream()), 'sdsm_render_overlay_multi')
        return self.unpack(d_out, 3, (3,))


def _candidate_pairs(boxes, all_pairs):
    """The pairs (i1, i2 < i1) of one image in the order of render.py:398-399, restricted to those whose boxes intersect (any other pair
    overlaps by 0, which exceeds no threshold >= 0)."""
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    r1, c1 = b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]
    pairs = []
    for i1 in range(1, len(b)):
        if all_pairs:
            i2 = np.arange(i1)
        else:
            i2 = np.nonzero((b[:i1, 0] < r1[i1]) & (b[i1, 0] < r1[:i1]) & (b[:i1, 1] < c1[i1]) & (b[i1, 1] < c1[:i1]))[0]
        if len(i2):
            pairs.append(np.stack([np.full(len(i2), i1), i2], axis=1))
    return np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int64)


def _merge_members(n, pairs, inter, areas, merge_overlap_threshold):
    """The merge bookkeeping of render.py:397-418, as in :func:`rasterize_labels`: the member lists of the surviving labels, in
    dictionary order."""
    merge_list = []
    for (i1, i2), ab in zip(pairs, inter):
        overlap = ab / (0. + min(areas[i1], areas[i2]))
        if overlap > merge_overlap_threshold:
            merge_list.append((int(i1), int(i2)))
    labels = list(range(1, 1 + n))
    members = {label: [label - 1] for label in labels}
    for merge_idx, (i1, i2) in enumerate(merge_list):
        new_label = n + 1 + merge_idx
        l1, l2 = labels[i1], labels[i2]
        if l1 == l2:
            continue
        merged = members[l1] + members[l2]
        for k in merged:
            labels[k] = new_label
        members[new_label] = merged
        del members[l1], members[l2]
    return list(members.values())


def _labels_set(shapes, objects_per_image, merge_overlap_threshold, dilate, background_label, keep_set=False):
    """rasterize_labels for one set of at most ``_capi.MAX_SET_IMAGES`` images: every phase one call for the whole set."""
    S = _GpuSet(shapes)
    packed_set, _, areas = pack_object_sets(objects_per_image)
    obj_image, boxes = packed_set[:2]
    Hs, Ws = (np.array([s[k] for s in S.shapes], np.int64)[obj_image] for k in (0, 1))
    b = boxes.astype(np.int64)
    if ((b[:, 0] < 0) | (b[:, 1] < 0) | (b[:, 2] < 0) | (b[:, 3] < 0) | (b[:, 0] + b[:, 2] > Hs) | (b[:, 1] + b[:, 3] > Ws)).any():
        raise ValueError('an object reaches outside its image (fg_offset, fg_fragment.shape against g_raw.shape)')
    S.load(*packed_set)
    if dilate != 0 and len(boxes):                                       # phase 1 (render.py:380-384)
        boxes, areas = S.morph(dilate)
    keep = areas > 0                                                     # render.py:385
    if not keep.all():
        S.select(keep)
        obj_image, boxes, areas = obj_image[keep], boxes[keep], areas[keep]
    first = np.searchsorted(obj_image, np.arange(len(shapes) + 1))       # the objects of image i: first[i] .. first[i + 1]
    pairs = [np.zeros((0, 2), np.int64)] * len(shapes)
    if merge_overlap_threshold <= 1:                                     # phase 2 (render.py:397-403)
        pairs = [_candidate_pairs(boxes[first[i]:first[i + 1]], merge_overlap_threshold < 0) for i in range(len(shapes))]
    inter = S.overlaps(np.concatenate([p + first[i] for i, p in enumerate(pairs)])) if sum(len(p) for p in pairs) else np.zeros(0, np.int64)
    obj_label, obj_group, groups, k0, g0 = np.zeros(len(boxes), np.int32), np.zeros(len(boxes), np.int32), [], 0, 0
    for i in range(len(shapes)):
        n_i = first[i + 1] - first[i]
        members = _merge_members(n_i, pairs[i], inter[k0:k0 + len(pairs[i])], areas[first[i]:first[i + 1]], merge_overlap_threshold)
        k0 += len(pairs[i])
        if len(members) >= 2 ** 16:
            raise ValueError(f'{len(members)} labels: a uint16 label map holds at most 65535')
        for l, ks in enumerate(members, 1):
            obj_label[first[i] + np.asarray(ks, np.int64)] = l
            obj_group[first[i] + np.asarray(ks, np.int64)] = g0 + l
            groups.append((i, first[i] + np.asarray(ks, np.int64)))
        g0 += len(members)
    S.paint(obj_label)                                                   # phase 3 (render.py:425-431)
    if len(boxes):
        capacity = [min(h * w, int(areas[first[i]:first[i + 1]].sum())) for i, (h, w) in enumerate(S.shapes)]
        entries = S.flood_inputs(capacity)                               # phases 4, 5 (render.py:432-433)
        pix, lab, unreached = [], [], False
        for i, e in enumerate(entries):
            if len(e) == 0 or not (e['label'] == 0).any():
                continue
            flooded = flood_sparse(e['idx'], e['label'], e['dist'], *S.shapes[i])
            todo = e['label'] == 0
            unreached |= bool((flooded[todo] == 0).any())
            pix.append(S.offsets[i] + e['idx'][todo].astype(np.int64))
            lab.append(flooded[todo])
        if pix:
            S.scatter(np.concatenate(pix), np.concatenate(lab))
        if unreached:                                                    # phase 6 (render.py:443-447)
            lost, vmax = S.lost(obj_group, len(groups))
            vmax = [int(v) for v in vmax]
            for g, (i, ks) in enumerate(groups, 1):
                if lost[g] == 0:
                    continue
                if vmax[i] + 1 >= 2 ** 16:
                    raise ValueError('more than 65535 labels: a uint16 label map cannot hold them')
                if S.fill(ks, vmax[i] + 1):
                    vmax[i] += 1
    if keep_set:                                                         # the label map stays on the device (background 0) for an overlay
        return None, S
    return S.finish(background_label)                                    # phase 7 (render.py:449)


def flood_sparse(idx, label, dist, H, W):
    """``_watershed`` on the sparse set of pixels it can touch (native host code, sdsm_flood_sparse): entries sorted by raster index,
    label > 0 for the marker pixels next to an unlabelled one, 0 for the unlabelled ones.  Returns the labels after the flood."""
    import ctypes as C
    from . import _capi
    idx, label, dist = np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(label, np.int32), np.ascontiguousarray(dist, np.float64)
    out = np.zeros(len(idx), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _capi.check(_capi.lib().sdsm_flood_sparse(len(idx), p(idx), p(label), p(dist), int(H), int(W), p(out)), 'sdsm_flood_sparse')
    return out


def _objects_of(data, objects):
    return list(data[objects]) if isinstance(objects, str) else list(objects)


def _labels_many(datas, objects, merge_overlap_threshold, dilate, background_label, keep_sets=False):
    assert background_label <= 0
    if dilate != 0:
        _check_radius(dilate, 'dilate')
    datas = list(datas)
    if isinstance(objects, str):
        objs = [list(d[objects]) for d in datas]
    else:
        objs = [list(o) for o in objects]                                # one list of objects per image
        if len(objs) != len(datas):
            raise ValueError('objects: an output name or one list of objects per image')
    results, sets = [], []
    for part in in_sets(len(datas)):
        res = _labels_set([d['g_raw'].shape for d in datas[part]], objs[part], merge_overlap_threshold, int(dilate), int(background_label), keep_set=keep_sets)
        if keep_sets:
            sets.append(res[1])
        else:
            results += res
    return (results, sets) if keep_sets else results


def rasterize_labels_many(datas, objects='postprocessed_objects', merge_overlap_threshold=np.inf, dilate=0, background_label=0):
    """:func:`rasterize_labels` for a list of pipeline data objects on the GPU: one launch per kernel phase for up to
    ``_capi.MAX_SET_IMAGES`` images (larger lists are split).  ``objects``: an output name, or one list of objects per image.
    Per image byte-equal to :func:`rasterize_labels` and to :func:`rasterize_labels_gpu`."""
    return _labels_many(datas, objects, merge_overlap_threshold, dilate, background_label)


def rasterize_labels_gpu(data, objects='postprocessed_objects', merge_overlap_threshold=np.inf, dilate=0, background_label=0):
    """:func:`rasterize_labels` on the GPU (the same arguments, the same bytes): the set of this one image."""
    return _labels_many([data], [_objects_of(data, objects)], merge_overlap_threshold, dilate, background_label)[0]


# ---- overlays (render.py:137-365) -------------------------------------------------------------------------------------------------
COLORMAP = {'r': [0], 'g': [1], 'b': [2], 'y': [0, 1], 't': [1, 2], 'w': [0, 1, 2]}


def normalize_image(img, spread=1, ret_minmax=False):
    """Contrast enhancement (render.py:137-166): intensities clipped to mean +- spread * std (within the image's range), then mapped to
    [0, 1].  NumPy on the host: its statistics decide bytes of the overlays, so they are computed in NumPy's fixed order."""
    img = np.asarray(img)
    if not np.allclose(img.std(), 0):
        minval, maxval = max([img.min(), img.mean() - spread * img.std()]), min([img.max(), img.mean() + spread * img.std()])
        img = img.clip(minval, maxval)
    else:
        minval, maxval = 0, 1
    img = img - img.min()
    img /= img.max()
    return (img, minval, maxval) if ret_minmax else img


def _fetch_image(data, normalize_img=True):
    img = data['g_raw']
    return normalize_image(img) if normalize_img else img


def _fetch_rgb_image(data, normalize_img=True, override_img=None):
    """The RGB image under the contours, clipped to [0, 1] (render.py:174-187)."""
    if override_img is not None:
        img = override_img if override_img.ndim == 3 else np.dstack([override_img] * 3)
    elif 'g_rgb' in data:
        img = data['g_rgb']
        if img.max() > 1:
            img = img / 255
    else:
        img = _fetch_image(data, normalize_img)
        img = np.dstack([img] * 3)
    img = img.copy()
    img[img < 0] = 0
    img[img > 1] = 1
    return img


def rasterize_regions_host(regions, background_label=None, radius=3):
    """(borders, background) of a label image, label by label (render.py:246-262): the border of a region is what a disk erosion takes
    from it (the image border does not erode); ``background`` is the eroded region of ``background_label``."""
    regions = np.asarray(regions)
    borders, background = np.zeros(regions.shape, bool), np.zeros(regions.shape, bool)
    for i in range(int(regions.max()) + 1):
        region_mask = regions == i
        interior = _morph.binary_erosion(region_mask, _morph.disk(radius))
        borders |= region_mask & ~interior
        if i == background_label:
            background = interior.astype(bool)
    return borders, background


def _base_image(img):
    assert img.ndim == 2 or (img.ndim == 3 and img.shape[2] in (1, 3)), f'image has wrong dimensions: {img.shape}'
    img = np.asarray(img, np.float64)
    return img if img.ndim == 2 or img.shape[2] == 3 else img[:, :, 0]


def render_regions_over_image_host(img, regions, background_label=None, color=(0, 1, 0), bg=(0.6, 1, 0.6, 0.3), **kwargs):
    """Host definition of :func:`render_regions_over_image` (render.py:265-287)."""
    base = _base_image(img)
    result = np.dstack([base] * 3) if base.ndim == 2 else base.copy()
    borders, background = rasterize_regions_host(regions, background_label, **kwargs)
    for i in range(3):
        result[:, :, i][borders] = color[i]
    for i in range(3):
        result[background, i] = bg[i] * bg[3] + result[background, i] * (1 - bg[3])
    return (255 * result).clip(0, 255).astype('uint8')


def _regions_many(imgs, regions, background_label, color, bg, radius=3):
    radius = _check_radius(radius, 'radius')
    if radius < 0:
        raise ValueError('radius < 0')
    out = []
    for part in in_sets(len(imgs)):
        S = _GpuSet([np.asarray(r).shape for r in regions[part]])
        out += S.overlay(regions[part], [_base_image(np.asarray(i)) for i in imgs[part]], 0, radius, color, bg if background_label is not None else None, background_label)
    return out


def rasterize_regions_many(regions, background_label=None, radius=3):
    """:func:`rasterize_regions` for a list of label images, one launch per ``_capi.MAX_SET_IMAGES`` images."""
    radius = _check_radius(radius, 'radius')
    if radius < 0:
        raise ValueError('radius < 0')
    regions, out = list(regions), []
    for part in in_sets(len(regions)):
        out += _GpuSet([np.asarray(r).shape for r in regions[part]]).region_flags(regions[part], radius, background_label)
    return out


def rasterize_regions(regions, background_label=None, radius=3):
    """(borders, background) of a label image with labels >= 0 (render.py:246-262) on the GPU, in one pass: with mn / mx the smallest /
    largest label over the in-image pixels of disk(radius), a pixel is border iff mn != mx, background iff mn == mx == background_label."""
    return rasterize_regions_many([regions], background_label, radius)[0]


def render_regions_over_image_many(imgs, regions, background_label=None, color=(0, 1, 0), bg=(0.6, 1, 0.6, 0.3), **kwargs):
    """:func:`render_regions_over_image` for a list of images and their label images (one launch per ``_capi.MAX_SET_IMAGES``)."""
    return _regions_many(list(imgs), list(regions), background_label, color, bg, **kwargs)


def render_regions_over_image(img, regions, background_label=None, color=(0, 1, 0), bg=(0.6, 1, 0.6, 0.3), **kwargs):
    """RGB uint8 image of the regions' borders over ``img`` (render.py:265-287), on the GPU; ``kwargs``: ``radius`` (default 3)."""
    return _regions_many([img], [regions], background_label, color, bg, **kwargs)[0]


def _atoms_base(data, normalize_img, override_img):
    img = _fetch_image(data, normalize_img) if override_img is None else override_img
    return img / img.max()


def render_atoms_host(data, normalize_img=True, discarded_color=(0.3, 1, 0.3, 0.1), border_radius=2, border_color=(0, 1, 0), override_img=None):
    """Host definition of :func:`render_atoms` (render.py:190-215), label by label."""
    return render_regions_over_image_host(_atoms_base(data, normalize_img, override_img), data['atoms'], background_label=0, bg=discarded_color, radius=border_radius, color=border_color)


def render_atoms_many(datas, normalize_img=True, discarded_color=(0.3, 1, 0.3, 0.1), border_radius=2, border_color=(0, 1, 0), override_imgs=None, _key='atoms'):
    """:func:`render_atoms` for a list of pipeline data objects; ``override_imgs``: one image (or None) per data object."""
    datas = list(datas)
    over = list(override_imgs) if override_imgs is not None else [None] * len(datas)
    return _regions_many([_atoms_base(d, normalize_img, o) for d, o in zip(datas, over)], [d[_key] for d in datas], 0, border_color, discarded_color, border_radius)


def render_atoms(data, normalize_img=True, discarded_color=(0.3, 1, 0.3, 0.1), border_radius=2, border_color=(0, 1, 0), override_img=None):
    """The atomic image regions over the image (render.py:190-215), on the GPU."""
    return render_atoms_many([data], normalize_img, discarded_color, border_radius, border_color, [override_img])[0]


def render_foreground_clusters_host(data, normalize_img=True, discarded_color=(0.3, 1, 0.3, 0.1), border_radius=2, border_color=(0, 1, 0), override_img=None):
    """Host definition of :func:`render_foreground_clusters` (render.py:218-243), label by label."""
    return render_regions_over_image_host(_atoms_base(data, normalize_img, override_img), data['clusters'], background_label=0, bg=discarded_color, radius=border_radius, color=border_color)


def render_foreground_clusters_many(datas, normalize_img=True, discarded_color=(0.3, 1, 0.3, 0.1), border_radius=2, border_color=(0, 1, 0), override_imgs=None):
    """:func:`render_foreground_clusters` for a list of pipeline data objects."""
    return render_atoms_many(datas, normalize_img, discarded_color, border_radius, border_color, override_imgs, _key='clusters')


def render_foreground_clusters(data, normalize_img=True, discarded_color=(0.3, 1, 0.3, 0.1), border_radius=2, border_color=(0, 1, 0), override_img=None):
    """The regions of possibly clustered objects over the image (render.py:218-243), on the GPU."""
    return render_foreground_clusters_many([data], normalize_img, discarded_color, border_radius, border_color, [override_img])[0]


def _result_args(border_width, border_position, color):
    assert border_width % 2 == 0
    assert color in COLORMAP
    if border_position == 'outer':
        raise NotImplementedError("border_position = 'outer' has no one-pass form (it depends on the foreground of the other objects and a second dilation), see DESIGN.md \"Limits\"")
    if border_position not in ('center', 'inner'):
        raise ValueError(f'border_position = {border_position!r}')
    radius = border_width // 2
    return radius if border_position == 'center' else 2 * radius


def _result_base(data, normalize_img, override_img, grey_ok=False):
    """The image under the contours (render.py:352-353).  ``grey_ok``: a grey base stays one channel (its three channels would be
    equal, the maximum too: the same values, a third of the upload)."""
    if grey_ok and (override_img.ndim == 2 if override_img is not None else 'g_rgb' not in data):
        img = (override_img if override_img is not None else _fetch_image(data, normalize_img)).copy()
        img[img < 0] = 0
        img[img > 1] = 1
        return img / img.max()
    im_seg = _fetch_rgb_image(data, normalize_img, override_img)
    im_seg /= im_seg.max()
    return im_seg


def contour_mask_host(mask, radius, where):
    """The contour of one object's mask (render.py:291-327, ContourPaint), 'center' or 'inner'."""
    if where == 'center':
        selem = _morph.disk(radius)
        return np.logical_xor(_morph.binary_erosion(mask, selem), _morph.binary_dilation(mask, selem))
    assert where == 'inner'
    return np.logical_xor(mask, _morph.binary_erosion(mask, _morph.disk(2 * radius)))


def render_result_over_image_host(data, objects='postprocessed_objects', merge_overlap_threshold=np.inf, normalize_img=True, border_width=6,
                                  border_position='center', override_img=None, color='g'):
    """Host definition of :func:`render_result_over_image` (render.py:330-365): one erosion / dilation per label."""
    _result_args(border_width, border_position, color)
    im_seg = _result_base(data, normalize_img, override_img)
    seg_objects = rasterize_labels(data, objects, merge_overlap_threshold=merge_overlap_threshold)
    for l in sorted(set(seg_objects.flatten().tolist()) - {0}):
        seg_bnd = contour_mask_host(seg_objects == l, border_width // 2, border_position)
        for i in range(3):
            im_seg[seg_bnd, i] = (1 if i in COLORMAP[color] else 0)
    return (255 * im_seg).round().clip(0, 255).astype('uint8')


def render_result_over_image_many(datas, objects='postprocessed_objects', merge_overlap_threshold=np.inf, normalize_img=True, border_width=6,
                                  border_position='center', override_imgs=None, color='g'):
    """:func:`render_result_over_image` for a list of pipeline data objects: the label maps stay on the device between
    :func:`rasterize_labels_many` and the overlay kernel."""
    radius = _result_args(border_width, border_position, color)
    _check_radius(radius, 'border_width' if border_position == 'inner' else 'border_width // 2')
    datas = list(datas)
    over = list(override_imgs) if override_imgs is not None else [None] * len(datas)
    _, sets = _labels_many(datas, objects, merge_overlap_threshold, 0, 0, keep_sets=True)
    rgb = [1.0 if i in COLORMAP[color] else 0.0 for i in range(3)]
    out = []
    for part, S in zip(in_sets(len(datas)), sets):
        bases = [_result_base(d, normalize_img, o, grey_ok=True) for d, o in zip(datas[part], over[part])]
        out += S.overlay(None, bases, 1 if border_position == 'center' else 2, radius, rgb, None, 0)
    return out


def render_result_over_image(data, objects='postprocessed_objects', merge_overlap_threshold=np.inf, normalize_img=True, border_width=6,
                             border_position='center', override_img=None, color='g'):
    """The contours of the segmentation result over the image (render.py:330-365), on the GPU: 'center' paints the pixels with
    mx > 0 and mn != mx over disk(border_width // 2), 'inner' those with a label > 0 and mn != mx over disk(border_width)
    (mn / mx: smallest / largest label in the disk); 'outer' is not supported."""
    return render_result_over_image_many([data], [_objects_of(data, objects)], merge_overlap_threshold, normalize_img, border_width, border_position, [override_img], color)[0]


# ---- colour maps: y-maps and coloured labels (render.py:102-134, :454-508) -------------------------------------------------------
class _PixelSet(_DeviceSet):
    """The calls of the colour-map and graph kernels for one set (no label-map buffers: lighter than :class:`_GpuSet`)."""

    def colormap_values(self, ys, clims, table):
        """source 0 of the colour-map kernel: (pictures, NaN flag per image)."""
        n_im = len(self.shapes)
        d_src, d_lut = self.pack(ys, np.float64), self._up(table)
        d_flags = self.torch.empty(n_im, dtype=self.torch.int32, device=self.dev)
        d_out = self.torch.empty(self.total * 3, dtype=self.torch.float64, device=self.dev)
        clim = (self.C.c_double * (4 * n_im))(*[float(v) for c in clims for v in c])
        self.capi.check(self.L.sdsm_render_colormap_multi(self.table, n_im, 0, self._p(d_src), self._p(d_lut), len(table) - 3, clim, None, None, None, None, None, 0,
                                                          self._p(d_flags), self._p(d_out), self._stream()), 'sdsm_render_colormap_multi')
        return self.unpack(d_out, 3, (3,)), d_flags.cpu().numpy() != 0

    def _perm(self, perms):
        """The permutation tables of the set: (device table or None, host offsets, host minima)."""
        n_im = len(self.shapes)
        if perms is None:
            return None, None, None
        off = _exclusive(np.array([len(t) for _, t in perms] + [0], np.int64))
        d_perm = self._up(np.concatenate([t for _, t in perms] + [np.zeros(1, np.int32)]).astype(np.int32))
        return d_perm, (self.C.c_int64 * (n_im + 1))(*[int(v) for v in off]), (self.C.c_int32 * n_im)(*[int(lo) for lo, _ in perms])

    def permute(self, labels, perms):
        """shuffle_labels: the permuted labels (int32) per image."""
        d_labels = self.pack(labels, np.int32)
        d_perm, off, lo = self._perm(perms)
        d_out = self.torch.empty(self.total, dtype=self.torch.int32, device=self.dev)
        self.capi.check(self.L.sdsm_render_label_range_multi(self.table, len(self.shapes), self._p(d_labels), self._p(d_perm), off, lo, None, self._p(d_out), self._stream()),
                        'sdsm_render_label_range_multi')
        return self.unpack(d_out, 1)

    def colormap_labels(self, labels, perms, table, bg_label, bg_color):
        """source 1: the label range (integer atomics) and the colouring, without a round trip between them."""
        n_im = len(self.shapes)
        d_labels, d_lut = self.pack(labels, np.int32), self._up(table)
        d_perm, off, lo = self._perm(perms)
        d_range = self.torch.empty(2 * n_im, dtype=self.torch.int32, device=self.dev)
        d_out = self.torch.empty(self.total * 3, dtype=self.torch.float64, device=self.dev)
        self.capi.check(self.L.sdsm_render_label_range_multi(self.table, n_im, self._p(d_labels), self._p(d_perm), off, lo, self._p(d_range), None, self._stream()),
                        'sdsm_render_label_range_multi')
        bgc = (self.C.c_double * 3)(*[float(v) for v in bg_color]) if bg_label is not None else None
        self.capi.check(self.L.sdsm_render_colormap_multi(self.table, n_im, 1, self._p(d_labels), self._p(d_lut), len(table) - 3, None, self._p(d_perm), off, lo,
                                                          self._p(d_range), bgc, int(bg_label if bg_label is not None else 0), None, self._p(d_out), self._stream()),
                        'sdsm_render_colormap_multi')
        return self.unpack(d_out, 3, (3,))

    def graph(self, prims, bases, rim_radius, disk_radius, reach, core_d2, ring_d2, colors):
        n_im = len(self.shapes)
        d_base, ch = self.pack_bases(bases)
        d_prims = self._up(prims) if len(prims) else None
        d_key = self.torch.empty(self.total, dtype=self.torch.int32, device=self.dev)
        d_out = self.torch.empty(self.total * 3, dtype=self.torch.uint8, device=self.dev)
        col = (self.C.c_double * 12)(*[float(v) for v in colors])
        self.capi.check(self.L.sdsm_render_graph_multi(self.table, n_im, len(prims), self._p(d_prims), float(rim_radius), float(disk_radius), int(reach), int(core_d2),
                                                       int(ring_d2), col, self._p(d_base), ch, self._p(d_key), self._p(d_out), self._stream()), 'sdsm_render_graph_multi')
        return self.unpack(d_out, 3, (3,))


def colormap_table(cmap):
    """The table the colour-map kernel takes: ``(N + 3) x 4`` float64, the ``N`` colours, then those for values below, above and
    "bad".  ``cmap``: such a table, the name of a matplotlib colour map, or a matplotlib ``Colormap`` (matplotlib is imported for the
    last two only)."""
    if isinstance(cmap, (np.ndarray, list, tuple)):
        table = np.ascontiguousarray(cmap, np.float64)
    else:
        if isinstance(cmap, str):
            import matplotlib
            cmap = matplotlib.colormaps[cmap]
        if not cmap._isinit:
            cmap._init()
        table = np.ascontiguousarray(cmap._lut, np.float64)
        assert (cmap._i_under, cmap._i_over, cmap._i_bad) == (cmap.N, cmap.N + 1, cmap.N + 2) and len(table) == cmap.N + 3
    if table.ndim != 2 or table.shape[1] != 4 or table.shape[0] < 4:
        raise ValueError('a colour-map table is (N + 3) x 4: the N colours, then under, over, bad')
    return table


def _check_table(table):
    from . import _capi
    if len(table) - 3 > _capi.RENDER_MAX_COLORS:
        raise NotImplementedError(f'a colour map of {len(table) - 3} entries: the GPU colour maps take up to {_capi.RENDER_MAX_COLORS}, see DESIGN.md "Limits"')
    return table


def colormap_lookup_host(table, x):
    """matplotlib's ``Colormap.__call__`` for float input on a table of :func:`colormap_table` (colors.py, _get_rgba_and_mask): scaled
    by ``N``; exactly ``N`` reads entry ``N - 1``; negative values read "under" (-0.0 is not negative), values >= ``N`` "over", NaN
    "bad"; everything else is truncated.  The arithmetic runs in the float type of ``x``, as there.  Returns ``x.shape + (4,)``."""
    table = np.asarray(table, np.float64)
    N = len(table) - 3
    xa = np.array(x, copy=True)
    if xa.dtype.kind != 'f':
        raise TypeError('colormap_lookup_host takes floating-point values (matplotlib reads integers as indices)')
    with np.errstate(invalid='ignore', over='ignore'):
        xa *= N
        xa[xa == N] = N - 1
        under, over, bad = xa < 0, xa >= N, np.isnan(xa)
        idx = xa.astype(int)
    idx[under], idx[over], idx[bad] = N, N + 1, N + 2
    return table.take(idx, axis=0, mode='clip')


def _ymap_input(data, clim):
    y = data if isinstance(data, np.ndarray) else data['y']
    if clim is None:
        clim = (-y.std(), +y.std())
    return y, clim


def render_ymap_host(data, clim=None, cmap='bwr'):
    """Host definition of :func:`render_ymap` (render.py:102-134): a row ``(clim[0], ..., clim[0], clim[1])`` is put before ``y``, the
    whole is clipped to ``clim``, its minimum subtracted, divided by its maximum and looked up; the row and the alpha channel go."""
    y, clim = _ymap_input(data, clim)
    z = np.full((1, y.shape[1]), clim[0])
    z[0, -1] = clim[1]
    y = np.concatenate((z, y), axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        y = y.clip(*clim)
        y -= y.min()
        y /= y.max()
    return colormap_lookup_host(colormap_table(cmap), y)[1:, :, :3]


def render_ymap_many(datas, clim=None, cmap='bwr'):
    """:func:`render_ymap` for a list of data objects or ``y`` arrays (one launch per ``_capi.MAX_SET_IMAGES`` images); ``clim=None``
    is each image's own ``(-y.std(), +y.std())``, NumPy's on the host: one number that decides bytes.

    Without a NaN, and with ``clim[0] < clim[1]``, the clipped padded array has the minimum ``clim[0]`` and the maximum ``clim[1]``
    exactly, so the kernel computes ``(clip(y) - clim[0]) / (clim[1] - clim[0])`` without a reduction.  In general the two numbers are
    what the definition's arithmetic gives on the pair ``(clim[0], clim[1])`` alone: with ``clim[0] >= clim[1]`` the clip leaves
    ``clim[1]`` everywhere, 0 / 0 follows and every pixel is "bad" (so is the ``y`` that is constant under ``clim=None``).  A NaN in
    ``y`` makes ``y.min()`` NaN: the kernel flags it and every pixel of that picture is "bad"."""
    table = _check_table(colormap_table(cmap))
    ys, clims = [], []
    for data in datas:
        y, c = _ymap_input(data, clim)
        if y.ndim != 2 or y.shape[1] < 2 or y.dtype != np.float64:
            raise NotImplementedError('render_ymap on the GPU takes float64 H x W images with W >= 2 (the definition computes in the type of y; in one column the '
                                      'padding row holds clim[1] alone), see DESIGN.md "Limits"')
        lo, hi = float(c[0]), float(c[1])
        with np.errstate(invalid='ignore'):
            pair = np.array([lo, hi]).clip(lo, hi)
            sub = pair.min()
            pair -= sub
        ys.append(y)
        clims.append((lo, hi, sub, pair.max()))
    out = []
    for part in in_sets(len(ys)):
        pics, bad = _PixelSet([y.shape for y in ys[part]]).colormap_values(ys[part], clims[part], table)
        out += [np.broadcast_to(table[-1, :3], p.shape).copy() if b else p for p, b in zip(pics, bad)]
    return out


def render_ymap(data, clim=None, cmap='bwr'):
    """The offset image intensities ``y`` through a colour map (render.py:102-134), on the GPU: float64 ``H x W x 3``."""
    return render_ymap_many([data], clim, cmap)[0]


def _shuffle_map(labels, bg_label, seed):
    """render.py:462-467: the present label values in the iteration order of their ``frozenset`` and their shuffle by NumPy's legacy
    generator.  Both orders decide the result, so this is the reference's construction step by step."""
    values0 = frozenset(labels.flatten())
    if bg_label is not None:
        values0 -= {bg_label}
    values0 = list(values0)
    if seed is not None:
        np.random.seed(seed)
    values1 = np.asarray(values0).copy()
    np.random.shuffle(values1)
    return values0, values1


def shuffle_labels_host(labels, bg_label=None, seed=None):
    """Host definition of :func:`shuffle_labels` (render.py:454-473), label by label.  As in the reference the result starts from
    zeros: the pixels of ``bg_label`` read 0 afterwards (``bg_label`` itself only if it is 0)."""
    labels = np.asarray(labels)
    result = np.zeros_like(labels)
    for l0, l1 in zip(*_shuffle_map(labels, bg_label, seed)):
        result[labels == l0] = l1
    return result


def _int32_labels(labels, extra_zero=False):
    """The labels as int32, refused where the reference's own arithmetic (``labels - labels.min()``, ``labels.max() - labels.min()`` in
    the labels' dtype) would wrap or the values do not fit."""
    labels = np.asarray(labels)
    if labels.dtype.kind not in 'iu' or labels.ndim != 2:
        raise TypeError('labels: a two-dimensional integer image')
    if labels.dtype.kind == 'i' or labels.dtype.itemsize >= 4:
        mn, mx = int(labels.min()), int(labels.max())
        if extra_zero:
            mn, mx = min(mn, 0), max(mx, 0)
        if mn < -2 ** 31 or mx >= 2 ** 31 or (labels.dtype.kind == 'i' and mx - mn > np.iinfo(labels.dtype).max) or mx - mn >= 2 ** 31:
            raise ValueError('labels: the values must fit int32 and their range the labels\' own dtype')
    return labels.astype(np.int32)


def _perm_table(labels, bg_label, seed):
    """The shuffle as a lookup table: (lowest label of the table, int32 table indexed by label - lowest); labels that are not shuffled
    (``bg_label``) read 0."""
    values0, values1 = _shuffle_map(labels, bg_label, seed)
    if len(values0) == 0:
        return 0, np.zeros(1, np.int32)
    v0 = np.asarray(values0).astype(np.int64)
    lo, n = int(v0.min()), int(v0.max()) - int(v0.min()) + 1
    if n > 2 ** 24:
        raise NotImplementedError(f'labels spread over {n} values: the permutation table of the GPU form holds up to 2^24, see DESIGN.md "Limits"')
    table = np.zeros(n, np.int32)
    table[v0 - lo] = np.asarray(values1).astype(np.int64)
    return lo, table


def shuffle_labels_many(labels, bg_label=None, seed=None):
    """:func:`shuffle_labels` for a list of label images.  The permutation of each image is built on the host exactly as the reference
    does (:func:`_shuffle_map`; with a seed every image is shuffled from that seed, as separate calls would); the GPU applies it."""
    labels = [np.asarray(l) for l in labels]
    l32 = [_int32_labels(l, extra_zero=True) for l in labels]
    perms = [_perm_table(l, bg_label, seed) for l in labels]
    out = []
    for part in in_sets(len(labels)):
        out += [r.astype(l.dtype) for r, l in zip(_PixelSet([l.shape for l in labels[part]]).permute(l32[part], perms[part]), labels[part])]
    return out


def shuffle_labels(labels, bg_label=None, seed=None):
    """Randomly permutes the values of a label image (render.py:454-473); the lookup runs on the GPU."""
    return shuffle_labels_many([labels], bg_label, seed)[0]


def colorize_labels_host(labels, bg_label=0, cmap='gist_rainbow', bg_color=(0, 0, 0), shuffle=None):
    """Host definition of :func:`colorize_labels` (render.py:476-508).  An image of one label divides 0 by 0: NaN, the "bad" colour,
    everywhere but on the background."""
    labels = np.asarray(labels)
    if shuffle is not None:
        labels = shuffle_labels_host(labels, bg_label=bg_label, seed=shuffle)
    with np.errstate(invalid='ignore', divide='ignore'):
        img = colormap_lookup_host(colormap_table(cmap), (labels - labels.min()) / float(labels.max() - labels.min()))
    img = img[:, :, :3]
    if bg_label is not None:
        img[labels == bg_label] = np.asarray(bg_color)[None, None, :]
    return img


def colorize_labels_many(labels, bg_label=0, cmap='gist_rainbow', bg_color=(0, 0, 0), shuffle=None):
    """:func:`colorize_labels` for a list of label images (one launch per ``_capi.MAX_SET_IMAGES``): the permutation as a table lookup,
    the minimum and maximum of the (shuffled) labels by integer atomics, ``(label - min) / float(max - min)`` in float64 and the
    colour-map lookup per pixel."""
    table = _check_table(colormap_table(cmap))
    labels = [np.asarray(l) for l in labels]
    l32 = [_int32_labels(l, extra_zero=shuffle is not None) for l in labels]
    perms = [_perm_table(l, bg_label, shuffle) for l in labels] if shuffle is not None else None
    out = []
    for part in in_sets(len(labels)):
        out += _PixelSet([l.shape for l in labels[part]]).colormap_labels(l32[part], perms[part] if perms is not None else None, table, bg_label, bg_color)
    return out


def colorize_labels(labels, bg_label=0, cmap='gist_rainbow', bg_color=(0, 0, 0), shuffle=None):
    """A colour picture of a label image (render.py:476-508), on the GPU: float64 ``H x W x 3``."""
    return colorize_labels_many([labels], bg_label, cmap, bg_color, shuffle)[0]


# ---- adjacency graphs (render.py:13-99) ---------------------------------------------------------------------------------------------
# scikit-image is not a dependency: the two functions of skimage.draw that the reference calls are restated from their documented rules.
def line_pixels_host(r0, c0, r1, c1):
    """The pixels of ``skimage.draw.line(r0, c0, r1, c1)``: integer Bresenham.  The longer axis drives (the columns on a tie), one pixel
    per step; the error term starts at ``2 * d_short - d_long``; after a pixel the minor coordinate steps while the term is >= 0; the
    last pixel is the end point itself."""
    r0, c0, r1, c1 = int(r0), int(c0), int(r1), int(c1)
    dr, dc = abs(r1 - r0), abs(c1 - c0)
    sr, sc = (1 if r1 - r0 > 0 else -1), (1 if c1 - c0 > 0 else -1)
    steep = dr > dc
    major, minor, d_long, d_short, s_major, s_minor = (r0, c0, dr, dc, sr, sc) if steep else (c0, r0, dc, dr, sc, sr)
    rr, cc = np.zeros(d_long + 1, np.int64), np.zeros(d_long + 1, np.int64)
    err = 2 * d_short - d_long
    for i in range(d_long):
        rr[i], cc[i] = (major, minor) if steep else (minor, major)
        while err >= 0:
            minor += s_minor
            err -= 2 * d_long
        major += s_major
        err += 2 * d_short
    rr[d_long], cc[d_long] = r1, c1
    return rr, cc


def disk_pixels_host(center, radius, shape):
    """The pixels of ``skimage.draw.disk(center, radius, shape=shape)``: ``((r - r0) / radius) ** 2 + ((c - c0) / radius) ** 2 < 1`` in
    float64, within the image."""
    r = np.arange(shape[0], dtype=np.float64)[:, None]
    c = np.arange(shape[1], dtype=np.float64)[None, :]
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.nonzero(((r - center[0]) / radius) ** 2 + ((c - center[1]) / radius) ** 2 < 1)


def draw_line_host(p1, p2, thickness, shape):
    """Host definition of ``draw_line`` (render.py:13-44): float64 mask of the straight line between two end points.  A thickness whose
    threshold ``(thickness + 1) / 2`` is (close to) an integer gives the pixels nearer than the threshold to a line pixel (Euclidean
    distance transform in the end points' box grown by the reach); any other thickness blends the two neighbouring odd ones."""
    assert thickness >= 1
    threshold = (thickness + 1) / 2
    if np.allclose(threshold, round(threshold)):
        p1, p2 = np.asarray(p1), np.asarray(p2)
        n = math.ceil(threshold) - 1
        box = np.array((np.minimum(p1, p2) - n, np.maximum(p1, p2) + n)).clip(0, np.subtract(shape, 1))
        buf = np.zeros(1 + box[1] - box[0])
        rr, cc = line_pixels_host(*(p1 - box[0]), *(p2 - box[0]))
        buf[rr, cc] = 1
        result = np.zeros(shape)
        result[box[0, 0]:box[1, 0] + 1, box[0, 1]:box[1, 1] + 1] = ndi.distance_transform_edt(buf == 0) < threshold
        return result
    thickness1 = 2 * int((thickness + 1) // 2) - 1
    thickness2 = thickness1 + 2
    buf1, buf2 = draw_line_host(p1, p2, thickness1, shape), draw_line_host(p1, p2, thickness2, shape)
    return (buf2 * (thickness - thickness1) / (thickness2 - thickness1) + buf1).clip(0, 1)


def _graph_base(data, normalize_img, override_img):
    """The image under the graph (render.py:77-83): float64, one channel where it is grey."""
    if override_img is not None:
        assert override_img.ndim == 3 and override_img.shape[2] >= 3
        img = override_img[:, :, :3].copy()
        if (img > 1).any():
            img = img / 255
        return img
    img = _fetch_image(data, normalize_img)
    return img / img.max()


def _graph_lines(data, lines):
    return list(data['adjacencies'].get_edge_lines()) if lines is None else list(lines)


def render_adjacencies_host(data, normalize_img=True, edge_thickness=3, endpoint_radius=5, endpoint_edge_thickness=2, edge_color=(1, 0, 0),
                            endpoint_color=(1, 0, 0), endpoint_edge_color=(0, 0, 0), override_img=None, lines=None):
    """Host definition of :func:`render_adjacencies` (render.py:47-99).  The painting order is part of it: every seed's rim, the lines
    in list order (a later line over an earlier one), every seed's disk."""
    img = _graph_base(data, normalize_img, override_img)
    if img.ndim == 2:
        img = np.dstack([img] * 3)
    shape = img.shape[:2]
    for endpoint in data['seeds']:
        mask = disk_pixels_host(endpoint, endpoint_radius + endpoint_edge_thickness, shape)
        for i in range(3):
            img[:, :, i][mask] = endpoint_edge_color[i]
    for line in _graph_lines(data, lines):
        buf = draw_line_host(line[0], line[1], edge_thickness, shape)
        mask = buf > 0
        for i in range(3):
            img[:, :, i][mask] = buf[mask] * edge_color[i]
    for endpoint in data['seeds']:
        mask = disk_pixels_host(endpoint, endpoint_radius, shape)
        for i in range(3):
            img[:, :, i][mask] = endpoint_color[i]
    return (255 * img).clip(0, 255).astype('uint8')


def _d2_limit(threshold):
    """The largest integer d2 with ``sqrt(d2) < threshold``, the test of the definition on the squared distances (integers) that the
    distance transform takes the root of; -1 if there is none."""
    d2 = np.arange((math.ceil(threshold) + 1) ** 2, dtype=np.float64)
    ok = np.nonzero(np.sqrt(d2) < threshold)[0]
    return int(ok.max()) if len(ok) else -1


def _line_args(thickness, color):
    """(reach, core_d2, ring_d2, core colour, ring colour) of the graph kernel for a line thickness (render.py:22-44, :91-94)."""
    if not thickness >= 1:
        raise ValueError('edge_thickness >= 1 required')
    if not thickness <= 33:
        raise NotImplementedError(f'edge_thickness = {thickness!r}: the GPU adjacency graphs take line thicknesses up to 33, see DESIGN.md "Limits"')
    threshold = (thickness + 1) / 2
    if np.allclose(threshold, round(threshold)):
        core = ring = _d2_limit(threshold)
        values = np.array([1., 1.])
    else:
        thickness1 = 2 * int((thickness + 1) // 2) - 1
        thickness2 = thickness1 + 2
        core, ring = _d2_limit((thickness1 + 1) / 2), _d2_limit((thickness2 + 1) / 2)
        values = (np.array([1., 1.]) * (thickness - thickness1) / (thickness2 - thickness1) + np.array([1., 0.])).clip(0, 1)
    return math.isqrt(ring), core, ring, [values[0] * c for c in color], [values[1] * c for c in color]


def _graph_points(points, shape, what, image):
    """``points`` (n x 2, or n x 2 x 2 for lines) as int32 after the checks the kernels do not make: integers inside the image."""
    a = np.asarray(points)
    if a.size == 0:
        return np.zeros((0,) + ((2,) if what == 'seeds' else (2, 2)), np.int32)
    if a.dtype.kind not in 'iu' and not (a.dtype.kind == 'f' and (a == np.floor(a)).all()):
        raise ValueError(f'image {image}: {what} must have integer coordinates')
    a = a.astype(np.int64).reshape((-1, 2) if what == 'seeds' else (-1, 2, 2))
    if (a < 0).any() or (a[..., 0] >= shape[0]).any() or (a[..., 1] >= shape[1]).any():
        raise ValueError(f'image {image}: {what} outside the image')
    if len(a) > 65535:
        raise ValueError(f'image {image}: {len(a)} {what}: at most 65535 per image')
    return a.astype(np.int32)


def render_adjacencies_many(datas, normalize_img=True, edge_thickness=3, endpoint_radius=5, endpoint_edge_thickness=2, edge_color=(1, 0, 0),
                            endpoint_color=(1, 0, 0), endpoint_edge_color=(0, 0, 0), override_imgs=None, lines=None):
    """:func:`render_adjacencies` for a list of pipeline data objects (one launch per ``_capi.MAX_SET_IMAGES`` images);
    ``override_imgs`` / ``lines``: one image / one list of lines (or None) per data object."""
    from . import _capi
    datas = list(datas)
    over = list(override_imgs) if override_imgs is not None else [None] * len(datas)
    lines = list(lines) if lines is not None else [None] * len(datas)
    rim, disk = endpoint_radius + endpoint_edge_thickness, endpoint_radius
    for v, what in ((rim, 'endpoint_radius + endpoint_edge_thickness'), (disk, 'endpoint_radius')):
        if not v >= 0:
            raise ValueError(f'{what} = {v!r}: a radius >= 0')
        if v > _capi.RENDER_MAX_SEED_RADIUS:
            raise NotImplementedError(f'{what} = {v!r}: the GPU adjacency graphs take end points up to radius {_capi.RENDER_MAX_SEED_RADIUS} with their rim, see DESIGN.md "Limits"')
    reach, core_d2, ring_d2, core_color, ring_color = _line_args(edge_thickness, edge_color)
    colors = list(endpoint_edge_color) + list(endpoint_color) + core_color + ring_color
    bases, prims = [], []
    for k, (d, o, l) in enumerate(zip(datas, over, lines)):
        base = _graph_base(d, normalize_img, o)
        if base.dtype != np.float64:
            raise NotImplementedError(f'image {k}: the image under the graph is {base.dtype} after its preparation; the GPU form paints float64 images, see DESIGN.md "Limits"')
        seeds = _graph_points(d['seeds'], base.shape[:2], 'seeds', k)
        ends = _graph_points(_graph_lines(d, l), base.shape[:2], 'lines', k)
        p = np.zeros((len(seeds) + len(ends), 8), np.int32)
        p[:len(seeds), 1], p[:len(seeds), 3:5] = np.arange(len(seeds)), seeds
        p[len(seeds):, 0], p[len(seeds):, 1], p[len(seeds):, 3:7] = 1, np.arange(len(ends)), ends.reshape(-1, 4)
        bases.append(base)
        prims.append(p)
    out = []
    for part in in_sets(len(datas)):
        for j, p in enumerate(prims[part]):
            p[:, 2] = j
        out += _PixelSet([b.shape[:2] for b in bases[part]]).graph(np.concatenate(prims[part]), bases[part], rim, disk, reach, core_d2, ring_d2, colors)
    return out


def render_adjacencies(data, normalize_img=True, edge_thickness=3, endpoint_radius=5, endpoint_edge_thickness=2, edge_color=(1, 0, 0),
                       endpoint_color=(1, 0, 0), endpoint_edge_color=(0, 0, 0), override_img=None, lines=None):
    """The adjacency graph over the image (render.py:47-99), on the GPU.  ``lines``: the edges as ``((r, c), (r, c))`` pairs in painting
    order; None takes ``data['adjacencies'].get_edge_lines()`` as it comes."""
    return render_adjacencies_many([data], normalize_img, edge_thickness, endpoint_radius, endpoint_edge_thickness, edge_color, endpoint_color, endpoint_edge_color,
                                   [override_img], [lines])[0]


# ---- the pictures of the reference's export tool (export.py:97-126) ----------------------------------------------------------------
EXPORT_DEFAULT_BORDER = {'seg': 8, 'fgc': 2, 'adj': 2, 'atm': 6}


def _export_ymap_inputs(y, ymap):
    """export.py:101-103: ``y`` clipped and squashed by a logistic curve, with the matching colour limits and the colour map's name."""
    lo, hi, gain, name = (tf(v) for v, tf in zip(ymap.lstrip('/').split(':'), (float, float, float, str)))
    squash = lambda v: np.exp(gain * v) / (1 + np.exp(gain * v)) - 0.5
    return squash(y.clip(lo, hi)), squash(np.array((lo, hi))), name


def export_views(datas, mode='seg', border=None, border_position='center', enhance=False, ymap='-0.8:+1:5:seismic', host=False):
    """The pictures that the reference's ``export`` tool writes for ``mode`` in 'seg', 'fgc', 'adj', 'atm' (export.py:116-126), one per
    pipeline data object, composed of the functions above on the GPU (``host=True``: of their ``*_host`` definitions, the same bytes).
    ``border``, ``border_position``, ``enhance`` and ``ymap`` are that tool's options; it reads and writes no file."""
    if mode not in EXPORT_DEFAULT_BORDER:
        raise ValueError(f'Unknown mode: "{mode}"')
    datas = list(datas)
    width = EXPORT_DEFAULT_BORDER[mode] if border is None else border
    each = lambda fn, **kw: [fn(d, **{k: (v[i] if k == 'override_img' else v) for k, v in kw.items()}) for i, d in enumerate(datas)]
    if mode == 'seg':
        kw = dict(border_width=width, border_position=border_position, normalize_img=enhance)
        return each(render_result_over_image_host, **kw) if host else render_result_over_image_many(datas, **kw)
    if mode == 'atm':
        kw = dict(border_color=(0, 1, 0), border_radius=width // 2, normalize_img=enhance)
        return each(render_atoms_host, **kw) if host else render_atoms_many(datas, **kw)
    ymaps = []
    spec = [_export_ymap_inputs(d['y'], ymap) for d in datas]
    if host:
        ymaps = [render_ymap_host(v, clim=c, cmap=name) for v, c, name in spec]
    else:
        for v, c, name in spec:                                          # (one colour limit per call; the tool's is the same for all)
            ymaps.append(render_ymap(v, clim=c, cmap=name))
    kw = dict(border_color=(0, 0, 0), border_radius=width // 2)
    if mode == 'fgc':
        return each(render_foreground_clusters_host, override_img=ymaps, **kw) if host else render_foreground_clusters_many(datas, override_imgs=ymaps, **kw)
    atoms = each(render_atoms_host, override_img=ymaps, **kw) if host else render_atoms_many(datas, override_imgs=ymaps, **kw)
    kw = dict(edge_color=(0, 1, 0), endpoint_color=(0, 1, 0))
    return each(render_adjacencies_host, override_img=atoms, **kw) if host else render_adjacencies_many(datas, override_imgs=atoms, **kw)


# ---- regression metric (tests/regression/validate.py) -----------------------------------------------------------------
def label_map_rows(labels):
    """The rows of validate.py:31-36 for one label map: per label ``(str(area), str(round(centre_x, 1)), str(round(centre_y, 1)))``,
    sorted by the centre columns as the CSV writer does (validate.py:38)."""
    labels = np.asarray(labels)
    rows = []
    for l in sorted(frozenset(labels.reshape(-1).tolist()) - {0}):
        cc = labels == l
        cy, cx = ndi.center_of_mass(cc)
        rows.append((str(int(cc.sum())), str(round(cx, 1)), str(round(cy, 1))))
    rows.sort(key=lambda row: row[1:3])
    return rows


def write_rows_csv(path, rows):
    with open(path, 'w', newline='') as fp:
        csv.writer(fp, delimiter=',', quoting=csv.QUOTE_ALL).writerows([['Object size', 'Center X', 'Center Y']] + list(rows))


def read_rows_csv(path):
    with open(path, newline='') as fp:
        return [tuple(row) for k, row in enumerate(csv.reader(fp, delimiter=',', quoting=csv.QUOTE_ALL)) if k > 0]


def compare_rows(actual_rows, expected_rows):
    """validate.py:76-80: (missing, spurious) as sets; the results agree iff both are empty."""
    a, e = frozenset(map(tuple, actual_rows)), frozenset(map(tuple, expected_rows))
    return e - a, a - e


def regression_agreement(actual_rows, expected_rows):
    """Fraction of the expected objects that are matched exactly, and the two mismatch counts."""
    missing, spurious = compare_rows(actual_rows, expected_rows)
    n = max(1, len(frozenset(map(tuple, expected_rows))))
    return dict(expected=len(frozenset(map(tuple, expected_rows))), missing=len(missing), spurious=len(spurious), matched_fraction=1 - len(missing) / n)
