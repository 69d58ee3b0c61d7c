"""``postprocess`` stage: discards spurious objects and refines the masks (reference: superdsm/postprocess.py:13-344).

Same stage name, inputs (``cover, y_img, atoms, g_raw, dsm_cfg``), output (``postprocessed_objects``), hyper-parameters and
``configure_ex`` factors as the reference.  The reference hands every object of the cover to a Ray task that runs two
Euclidean distance transforms of the WHOLE image (contrast, postprocess.py:254-266; the region of the normalised energy,
:289-291).  Here the per-object work of an image is ONE batch of the HIP engine (sdsm_post_objects: contrast response and
mask refinement on a window around each object; the two smoothed images by the separable Gaussian kernels); the normalised
energy needs no recomputation (``Object.cvxprog_region_size``).  The exact bit problems around that batch run on the device too,
each one launch per set of images: the background mask (sdsm_post_background_multi; integer ``exterior_offset`` up to 32, any
other value keeps the SciPy erosion), hole filling (sdsm_post_fill_holes; in the stage over the refined windows while they are still
on the device) and the glare test on the smoothed image where it was computed (sdsm_post_glare_multi).  What stays on
the host: the eccentricity and the accept / discard decisions.  There is no CPU path for the batch; ``_is_glare`` is kept as the
host definition the device is tested against."""
import math
import os
import time

import numpy as np
import scipy.ndimage as ndi

from . import _capi, _morph
from .imageset import in_sets
from .objects import BaseObject
from .output import get_output
from .pipeline import Stage


class PostprocessedObject(BaseObject):
    """A segmented object after post-processing (postprocess.py:244-251)."""

    def __init__(self, original):
        self.original = original
        self.fg_offset = original.fg_offset
        self.fg_fragment = original.fg_fragment


def _is_glare(obj, g_smooth, min_layer=0.5, num_layers=5):
    """Top ``1 - min_layer`` of the smoothed intensity profile connected at every of ``num_layers`` levels (postprocess.py:269-286)."""
    h, w = obj.fg_fragment.shape
    sect = g_smooth[obj.fg_offset[0]:obj.fg_offset[0] + h, obj.fg_offset[1]:obj.fg_offset[1] + w]
    mask = _morph.binary_erosion(obj.fg_fragment, _morph.disk(2))
    data = sect[mask]
    for prop in np.linspace(min_layer, 1, num_layers, endpoint=False):
        layer = np.logical_and(mask, sect > (data.max() - data.min()) * prop + data.min())
        if ndi.label(layer)[0].max() > 1:
            return False
    return True


def _compute_eccentricity(fragment):
    """Eccentricity of the ellipse with the region's second moments (what ``skimage.measure.regionprops(...).eccentricity`` is,
    postprocess.py:340-344): sqrt(1 - l2 / l1) of the eigenvalues l1 >= l2 of the inertia tensor."""
    if not fragment.any():
        return 0
    rr, cc = np.nonzero(fragment)
    r, c = rr - rr.mean(), cc - cc.mean()
    a, b, d = (r * r).mean(), (r * c).mean(), (c * c).mean()
    half, root = (a + d) / 2, math.sqrt(((a - d) / 2) ** 2 + b * b)
    l1, l2 = half + root, half - root
    return 0.0 if l1 == 0 else math.sqrt(max(0.0, 1 - l2 / l1))


def gaussian_filter_gpu(g_dev, sigma):
    """scipy.ndimage.gaussian_filter(g, sigma) on the device (a float64 H x W tensor in, a new tensor out)."""
    import ctypes as C
    import torch
    L = _capi.lib()
    H, W = (int(v) for v in g_dev.shape)
    out = torch.empty_like(g_dev)
    nbytes = L.sdsm_gaussian_workspace_bytes(H, W, float(sigma))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=g_dev.device)
    with torch.cuda.device(g_dev.device):
        _capi.check(L.sdsm_gaussian_filter(C.c_void_p(g_dev.data_ptr()), H, W, float(sigma), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'sdsm_gaussian_filter')
    return out


def _refinement_radius(mask_max_distance, mask_stdamp):
    if mask_max_distance > 0 and mask_stdamp > 0 and float(mask_max_distance) != int(mask_max_distance):
        # skimage.morphology.disk(r) of a fractional radius (postprocess.py:316-337) is not a disk of int(r): refuse instead of truncating
        raise NotImplementedError(f'mask_max_distance = {mask_max_distance!r}: the GPU mask refinement takes integer radii (<= 16) only, see DESIGN.md "Limits"')
    return int(mask_max_distance) if (mask_max_distance > 0 and mask_stdamp > 0) else 0


def pack_fragments(objects):
    """Boxes (n x 4 int32: r0, c0, h, w), word counts and the bit-packed fragments (row-major, LSB first, whole uint32 words) of a list
    of objects, and their areas: the object format of sdsm_post_objects and of the label-map kernels (render.py)."""
    n = len(objects)
    boxes = np.zeros((n, 4), np.int32)
    words = np.zeros(n, np.int64)
    packed = []
    for k, obj in enumerate(objects):
        h, w = obj.fg_fragment.shape
        boxes[k] = (int(obj.fg_offset[0]), int(obj.fg_offset[1]), h, w)
        bits = np.packbits(np.ascontiguousarray(obj.fg_fragment, bool).reshape(-1), bitorder='little')
        nw = (h * w + 31) // 32
        buf = np.zeros(nw * 4, np.uint8)
        buf[:bits.size] = bits
        packed.append(buf)
        words[k] = nw
    areas = np.array([int(o.fg_fragment.sum()) for o in objects], np.int64)
    return boxes, words, packed, areas


def pack_object_sets(objects_per_image):
    """The object lists of one set of images in the packed-object format of the ``*_multi`` calls: ``(obj_image, boxes, words, packed)``
    -- per object its image, and the boxes, word counts and bit-packed fragments of :func:`pack_fragments`, image after image --, then
    ``first`` (the objects of image i are ``first[i]`` .. ``first[i + 1]`` - 1) and the areas."""
    packs = [pack_fragments(objs) for objs in objects_per_image]
    obj_image = np.concatenate([np.full(len(pk[0]), i, np.int32) for i, pk in enumerate(packs)])
    boxes, words, areas = (np.concatenate([pk[k] for pk in packs]) for k in (0, 1, 3))
    first = np.concatenate([[0], np.cumsum([len(pk[0]) for pk in packs])])
    return (obj_image, boxes, words, [b for pk in packs for b in pk[2]]), first, areas


def grown_windows(boxes, H, W, m):
    """The windows box +- m clipped to the image, n x 4 int64 (r0, c0, h, w); ``H`` / ``W``: scalars or one value per box."""
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    r0, c0 = np.maximum(0, b[:, 0] - m), np.maximum(0, b[:, 1] - m)
    return np.stack([r0, c0, np.minimum(H, b[:, 0] + b[:, 2] + m) - r0, np.minimum(W, b[:, 1] + b[:, 3] + m) - c0], axis=1)


def window_words(windows):
    """Words of the bit-packed windows."""
    return ((windows[:, 2] * windows[:, 3] + 31) // 32).astype(np.int64)


def _pack_objects(objects, H, W, m):
    """The per-object inputs of sdsm_post_objects: boxes, words of the bit-packed fragments and of the refined windows, the packed
    fragments, areas."""
    boxes, words, packed, areas = pack_fragments(objects)
    return boxes, words, window_words(grown_windows(boxes, H, W, m)), packed, areas


def _exclusive(counts):
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64) if len(counts) else np.zeros(0, np.int64)


def _unpack_refined(recs, boxes, new_bits, new_off, new_words, H, W, m):
    """The refined masks (before hole filling) of the objects of one image: (offset, fragment) or None where the device did not refine."""
    refined = []
    for k in range(len(recs)):
        if m == 0:
            refined.append(None)
            continue
        r0, c0, h, w = (int(v) for v in boxes[k])
        nr0, nc0 = max(0, r0 - m), max(0, c0 - m)
        nh, nwid = min(H, r0 + h + m) - nr0, min(W, c0 + w + m) - nc0
        if recs['h'][k] <= 0:
            refined.append((np.zeros(2, int), np.zeros((1, 1), bool)))            # extract_foreground_fragment of an empty mask
            continue
        win = np.unpackbits(new_bits[4 * new_off[k]:4 * (new_off[k] + new_words[k])], bitorder='little')[:nh * nwid].reshape(nh, nwid).astype(bool)
        fr, fc = int(recs['r0'][k]) - nr0, int(recs['c0'][k]) - nc0
        refined.append((np.array([int(recs['r0'][k]), int(recs['c0'][k])]), win[fr:fr + int(recs['h'][k]), fc:fc + int(recs['w'][k])]))
    return refined


def _inv_gstd(g):
    """1 / g.std() in two passes, as NumPy's (postprocess.py:255): an error of the mean enters the variance squared only, so the
    normaliser keeps its digits on an image that is not normalised (torch's one-pass std loses mean / std of them).  A constant image
    whose deviations all round to 0 gives inf: the contrast comes out NaN and nothing is discarded (postprocess.py:254-266)."""
    d = g - g.mean()
    gstd = float(d.mul_(d).mean().sqrt())
    return 1.0 / gstd if gstd > 0 else float('inf')


def _check_boxes(boxes, shape):
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    if ((b[:, :2] < 0) | (b[:, 2:] <= 0) | (b[:, :2] + b[:, 2:] > tuple(int(v) for v in shape))).any():
        raise ValueError('an object reaches outside its image or has an empty box (fg_offset, fg_fragment.shape against g.shape)')


def background_radius(exterior_offset):
    """The disk radius of the device route of the background mask, or None where ``exterior_offset`` keeps the host route (not an
    integer in 0 .. ``_capi.POST_MAX_BG_RADIUS``)."""
    try:
        r = int(exterior_offset)
    except (TypeError, ValueError, OverflowError):
        return None
    return r if r == exterior_offset and 0 <= r <= _capi.POST_MAX_BG_RADIUS else None


def background_mask_gpu_multi(images, exterior_offset, device=None):
    """``background_mask`` (postprocess.py:152-155) of a set of images, ``images`` = ``(objects, shape)`` per image: the objects painted
    in their order (``fill_foreground`` assigns the whole box), the complement eroded by ``disk(exterior_offset)`` with the image border
    not eroding.  One sdsm_post_background_multi launch per ``_capi.MAX_SET_IMAGES`` images; returns one uint8 H x W device tensor per
    image, equal to the SciPy erosion bit for bit."""
    import ctypes as C
    r = background_radius(exterior_offset)
    if r is None:
        raise NotImplementedError(f'exterior_offset = {exterior_offset!r}: the GPU background mask takes integer radii 0 .. {_capi.POST_MAX_BG_RADIUS} only, see DESIGN.md "Limits"')
    packs = []
    for objects, shape in images:                            # refuse before anything is uploaded
        if len(shape) != 2 or min(shape) < 1:
            raise ValueError(f'image shape {tuple(shape)!r}')
        pk = pack_fragments(objects)
        _check_boxes(pk[0], shape)
        packs.append(pk)
    import torch
    L = _capi.lib()
    dev = torch.device('cuda' if device is None else device)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = []
    for part, pks in ((images[sl], packs[sl]) for sl in in_sets(len(images))):
        table = (_capi.PostBgImage * len(part))()
        work = []
        for j, (objects, shape) in enumerate(part):
            H, W = (int(v) for v in shape)
            bg, wk = torch.empty((H, W), dtype=torch.uint8, device=dev), torch.empty(H * W + (H * W + 3) // 4, dtype=torch.int32, device=dev)
            out.append(bg)
            work.append(wk)
            table[j].d_bg, table[j].d_work, table[j].H, table[j].W, table[j].n_objects = bg.data_ptr(), wk.data_ptr(), H, W, len(objects)
        n = sum(len(o) for o, _ in part)
        boxes = np.concatenate([pk[0] for pk in pks]) if n else np.zeros((1, 4), np.int32)
        bits_off = _exclusive(np.concatenate([pk[1] for pk in pks])) if n else np.zeros(1, np.int64)
        d_boxes, d_bits_off = to_dev(boxes), to_dev(bits_off)
        d_bits = to_dev(np.concatenate([b for pk in pks for b in pk[2]])) if n else torch.zeros(4, dtype=torch.uint8, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        with torch.cuda.device(dev):
            _capi.check(L.sdsm_post_background_multi(table, len(part), p(d_boxes), p(d_bits_off), p(d_bits), r, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                        'sdsm_post_background_multi')         # (the work images and the uploads go back to the allocator in stream order)
    return out


def background_mask_gpu(objects, shape, exterior_offset, device=None):
    """``background_mask`` of one image on the device: the set of this image (:func:`background_mask_gpu_multi`)."""
    return background_mask_gpu_multi([(objects, shape)], exterior_offset, device)[0]


def pack_windows(windows):
    """Bit-packed windows as sdsm_post_fill_holes takes them: ``(dims, offsets, bits)`` = n x 2 int32 (h, w), the first uint32 word of
    each window, and the bits (row-major, LSB first, continuous over the rows, whole words per window) as uint8."""
    dims = np.zeros((len(windows), 2), np.int32)
    packed = []
    for k, win in enumerate(windows):
        win = np.asarray(win)
        if win.ndim != 2 or win.size == 0:
            raise ValueError(f'window {k}: a non-empty 2-d mask is required, not shape {win.shape}')
        dims[k] = win.shape
        bits = np.packbits(np.ascontiguousarray(win, bool).reshape(-1), bitorder='little')
        buf = np.zeros((win.size + 31) // 32 * 4, np.uint8)
        buf[:bits.size] = bits
        packed.append(buf)
    words = (dims[:, 0].astype(np.int64) * dims[:, 1] + 31) // 32
    return dims, _exclusive(words), (np.concatenate(packed) if packed else np.zeros(0, np.uint8))


def unpack_windows(bits, offsets, dims):
    """The bool windows of a buffer packed as :func:`pack_windows` packs it."""
    out = []
    for off, (h, w) in zip(offsets, dims):
        h, w = int(h), int(w)
        out.append(np.unpackbits(bits[4 * int(off):4 * (int(off) + (h * w + 31) // 32)], bitorder='little')[:h * w].reshape(h, w).astype(bool))
    return out


def flood_workspace(dims, planes):
    """Offsets (in words, -1: the window is flooded in LDS) and total words of the global-memory workspace of windows of ``dims``
    (n x 2: h, w) whose whole-word rows exceed ``_capi.POST_FLOOD_WORDS``, ``planes`` bit planes each."""
    d = np.asarray(dims, np.int64).reshape(-1, 2)
    words = d[:, 0] * ((d[:, 1] + 31) // 32)
    need = np.where(words > _capi.POST_FLOOD_WORDS, planes * words, 0)
    return np.where(need > 0, _exclusive(need), -1).astype(np.int64), int(need.sum())


def _fill_holes_device(d_bits, dims, offsets, in_place=False):
    """sdsm_post_fill_holes on the current stream over windows already on the device (``d_bits``: uint8 tensor); returns the filled
    windows as a device tensor of the same layout, and the per-window status for :func:`_fill_status` once the caller has downloaded."""
    import ctypes as C
    import torch
    L = _capi.lib()
    dev = d_bits.device
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = len(dims)
    ws_off, ws_words = flood_workspace(dims, 2)
    d_out = d_bits if in_place else torch.empty_like(d_bits)
    d_dims, d_off, d_status = to_dev(np.asarray(dims, np.int32)), to_dev(np.asarray(offsets, np.int64)), torch.zeros(max(1, n), dtype=torch.int32, device=dev)
    d_ws, d_ws_off = (torch.empty(ws_words, dtype=torch.int32, device=dev), to_dev(ws_off)) if ws_words else (None, None)
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
    with torch.cuda.device(dev):
        _capi.check(L.sdsm_post_fill_holes(n, p(d_dims), p(d_off), p(d_bits), p(d_out), p(d_ws), p(d_ws_off), p(d_status),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'sdsm_post_fill_holes')
    return d_out, d_status[:n]


def _fill_status(d_status):
    """Refuses the windows of a sdsm_post_fill_holes launch if one of them was not flooded; read after the launch's results, so that
    the host waits for the stream once."""
    if d_status.cpu().numpy().any():
        raise _capi.SdsmError('sdsm_post_fill_holes: a window had no workspace')


def fill_holes_gpu(windows, device=None):
    """``scipy.ndimage.binary_fill_holes`` (default structure) of every 2-d mask of ``windows`` in one sdsm_post_fill_holes launch; returns
    the filled bool arrays."""
    dims, offsets, bits = pack_windows(windows)
    if not len(windows):
        return []
    import torch
    d_bits = torch.from_numpy(bits).to(torch.device('cuda' if device is None else device))
    d_out, d_status = _fill_holes_device(d_bits, dims, offsets, in_place=True)
    filled = d_out.cpu().numpy()
    _fill_status(d_status)
    return unpack_windows(filled, offsets, dims)


def glare_proportions(min_layer, num_layers):
    """The layer proportions of the glare test (postprocess.py:283), refused beyond what the device takes before anything runs."""
    num_layers = int(num_layers)
    if num_layers > _capi.POST_MAX_GLARE_LAYERS:
        raise NotImplementedError(f'glare_detection_num_layers = {num_layers}: the GPU glare test takes up to {_capi.POST_MAX_GLARE_LAYERS} layers, see DESIGN.md "Limits"')
    if num_layers < 1:
        raise ValueError('the glare test needs at least one layer')
    return np.ascontiguousarray(np.linspace(min_layer, 1, num_layers, endpoint=False), np.float64)


def glare_flags_gpu_multi(images, min_layer=0.5, num_layers=5):
    """The device part of the glare test (``_is_glare``) for the objects of a set of images, ``images`` = ``(objects, g_smooth)`` per image
    (``g_smooth``: float64 H x W device tensor, one device for all): one sdsm_post_glare_multi launch per ``_capi.MAX_SET_IMAGES`` images.
    Returns per image an n x 2 int32 array: the pixels of the fragment eroded by ``disk(2)`` and the bit mask of the layers with more than
    one component; :func:`glare_decision` turns a row into what ``_is_glare`` returns."""
    import ctypes as C
    props = glare_proportions(min_layer, num_layers)
    packs = []
    for objects, g in images:
        pk = pack_fragments(objects)
        _check_boxes(pk[0], g.shape)
        packs.append(pk)
    import torch
    L = _capi.lib()
    results = []
    for part, pks in ((images[sl], packs[sl]) for sl in in_sets(len(images))):
        n = sum(len(o) for o, _ in part)
        if n == 0:
            results += [np.zeros((0, 2), np.int32) for _ in part]
            continue
        dev = part[0][1].device
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        table = (_capi.PostImage * len(part))()
        for j, (objects, g) in enumerate(part):
            if g.dtype != torch.float64 or not g.is_contiguous():
                raise ValueError('the smoothed image must be a contiguous float64 tensor')
            table[j].d_g, table[j].H, table[j].W, table[j].n_objects = g.data_ptr(), int(g.shape[0]), int(g.shape[1]), len(objects)
        boxes = np.concatenate([pk[0] for pk in pks])
        ws_off, ws_words = flood_workspace(boxes[:, 2:], 3)
        d_boxes, d_bits_off = to_dev(boxes), to_dev(_exclusive(np.concatenate([pk[1] for pk in pks])))
        d_bits = to_dev(np.concatenate([b for pk in pks for b in pk[2]]))
        d_ws, d_ws_off = (torch.empty(ws_words, dtype=torch.int32, device=dev), to_dev(ws_off)) if ws_words else (None, None)
        d_out = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
        with torch.cuda.device(dev):
            _capi.check(L.sdsm_post_glare_multi(table, len(part), p(d_boxes), p(d_bits_off), p(d_bits), props.ctypes.data_as(C.POINTER(C.c_double)), len(props),
                                                p(d_ws), p(d_ws_off), p(d_out), C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'sdsm_post_glare_multi')
            flags = d_out.cpu().numpy()
        if (flags[:, 0] < 0).any():
            raise _capi.SdsmError('sdsm_post_glare_multi: an object had no workspace or an invalid box')
        first = 0
        for objects, _ in part:
            results.append(flags[first:first + len(objects)].copy())
            first += len(objects)
    return results


def glare_decision(flags):
    """What ``_is_glare`` returns for one row of :func:`glare_flags_gpu_multi`: the first layer with more than one component ends its
    loop with False; an empty eroded mask fails as the maximum of an empty array does."""
    if int(flags[0]) == 0:
        raise ValueError('zero-size array to reduction operation maximum which has no identity')
    return int(flags[1]) == 0


def process_objects_gpu(objects, g, g_mask_processing, background_mask, exterior_scale, exterior_offset, contrast_epsilon,
                        mask_max_distance, mask_stdamp, device=None):
    """Contrast response and refined mask (before hole filling) of every object of one image: the set of this image
    (:func:`process_objects_gpu_multi`).  ``g`` / ``g_mask_processing``: float64 device tensors; ``background_mask``: bool array or uint8
    device tensor.  Returns (records POST_RECORD_DTYPE, list of (offset, fragment) or None where the device did not refine)."""
    return process_objects_gpu_multi([(objects, g, g_mask_processing, background_mask)], exterior_scale, exterior_offset, contrast_epsilon,
                                     mask_max_distance, mask_stdamp)[0]


def process_objects_gpu_multi(images, exterior_scale, exterior_offset, contrast_epsilon, mask_max_distance, mask_stdamp):
    """Contrast response and refined mask of the objects of a set of images, ``images`` = ``(objects, g, g_mask_processing,
    background_mask)`` per image (one device for all): one sdsm_post_objects_multi launch per ``_capi.MAX_SET_IMAGES`` images.
    Returns ``(records, refined)`` per image, what the image gives as a set of its own."""
    return _process_objects(images, exterior_scale, exterior_offset, contrast_epsilon, mask_max_distance, mask_stdamp, None)


def _process_objects(images, exterior_scale, exterior_offset, contrast_epsilon, mask_max_distance, mask_stdamp, fill_holes):
    """:func:`process_objects_gpu_multi` (``fill_holes`` None), or the masks the stage decides on (postprocess.py:316-337; ``fill_holes``
    True / False): with hole filling, sdsm_post_fill_holes runs on the stream behind the refinement over the refined windows, and only
    the filled windows are downloaded; where nothing is refined it fills the original fragments.

    Filling the window equals filling the cropped fragment: a background component that does not touch the mask's bounding box is
    enclosed by mask pixels, all inside the box, so it cannot reach the window's margin either; and every background pixel outside the
    box is connected to the margin.  The bounding box of the filled mask is that of the unfilled one: the box in the record stays
    valid."""
    import ctypes as C
    m = _refinement_radius(mask_max_distance, mask_stdamp)
    all_packs = []
    for objects, g, *_ in images:                            # the kernel reads the image at every pixel of a box: refuse before anything is uploaded
        pk = _pack_objects(objects, *g.shape, m)
        _check_boxes(pk[0], g.shape)
        all_packs.append(pk)
    import torch
    L = _capi.lib()
    results = []
    for part, packs in ((images[sl], all_packs[sl]) for sl in in_sets(len(images))):
        dev = part[0][1].device
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        table = (_capi.PostImage * len(part))()
        keep = []
        for j, (objects, g, gs, bg) in enumerate(part):
            H, W = (int(v) for v in g.shape)
            bg = bg if torch.is_tensor(bg) else to_dev(np.asarray(bg, np.uint8))
            keep.append(bg)
            table[j].d_g, table[j].d_gs, table[j].d_bg = g.data_ptr(), gs.data_ptr(), bg.data_ptr()
            table[j].H, table[j].W, table[j].n_objects = H, W, len(objects)
            table[j].inv_gstd = _inv_gstd(g) if len(objects) else 0.0
        n = sum(len(o) for o, *_ in part)
        if n == 0:
            results += [(np.zeros(0, _capi.POST_RECORD_DTYPE), []) for _ in part]
            continue
        boxes = np.concatenate([pk[0] for pk in packs])
        words, new_words, areas = (np.concatenate([pk[k] for pk in packs]) for k in (1, 2, 4))
        bits_off, new_off = _exclusive(words), _exclusive(new_words)
        need_pool = areas > 12288
        bpool_off = np.where(need_pool, np.concatenate([[0], np.cumsum(np.where(need_pool, areas, 0))[:-1]]), -1).astype(np.int64)
        d_boxes, d_bits_off, d_new_off, d_bpool_off = to_dev(boxes), to_dev(bits_off), to_dev(new_off), to_dev(bpool_off)
        d_bits = to_dev(np.concatenate([b for pk in packs for b in pk[3]]))
        d_new = torch.zeros(max(1, int(new_words.sum())) * 4, dtype=torch.uint8, device=dev)
        d_pool = torch.empty(max(1, int(np.where(need_pool, areas, 0).sum())) * 4, dtype=torch.uint8, device=dev)
        d_out = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        with torch.cuda.device(dev):
            _capi.check(L.sdsm_post_objects_multi(table, len(part), p(d_boxes), p(d_bits_off), p(d_bits), p(d_new_off), p(d_new), p(d_pool),
                                                  p(d_bpool_off), float(exterior_scale), float(exterior_offset), float(contrast_epsilon), m,
                                                  float(mask_stdamp), p(d_out), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                        'sdsm_post_objects_multi')
            d_filled = d_fill_status = None
            if fill_holes and m > 0:
                wins = np.concatenate([grown_windows(pk[0], *(int(v) for v in g.shape), m) for (_, g, *_), pk in zip(part, packs) if len(pk[0])])
                _, d_fill_status = _fill_holes_device(d_new, wins[:, 2:], new_off, in_place=True)
            elif fill_holes:
                d_filled, d_fill_status = _fill_holes_device(d_bits, boxes[:, 2:], bits_off)
            recs = d_out.cpu().numpy().view(_capi.POST_RECORD_DTYPE).copy()
            new_bits = d_new.cpu().numpy() if m > 0 else None
            filled_bits = d_filled.cpu().numpy() if d_filled is not None else None
            if d_fill_status is not None:
                _fill_status(d_fill_status)
        if (recs['status'] == 1).any():
            raise _capi.SdsmError('sdsm_post_objects_multi: boundary list overflow')
        first = 0
        for (objects, g, *_), pk in zip(part, packs):
            H, W = (int(v) for v in g.shape)
            k = slice(first, first + len(objects))
            r = recs[k].copy()
            # the refined windows of this image, offsets relative to its first word
            refined = _unpack_refined(r, pk[0], new_bits, new_off[k], new_words[k], H, W, m) if len(objects) else []
            if filled_bits is not None:                      # nothing refined: the original fragments, filled
                refined = [(o.fg_offset, f) for o, f in zip(objects, unpack_windows(filled_bits, bits_off[k], pk[0][:, 2:]))]
            results.append((r, refined))
            first += len(objects)
    return results


class Postprocessing(Stage):
    """Stage ``postprocess`` (hyper-parameters as documented in superdsm/postprocess.py:13-110)."""

    ENABLED_BY_DEFAULT = True

    def __init__(self):
        super().__init__('postprocess', inputs=['cover', 'y_img', 'atoms', 'g_raw', 'dsm_cfg'], outputs=['postprocessed_objects'])

    @staticmethod
    def _settings(cfg):
        """The stage's hyper-parameters (postprocess.py:13-110), read as the reference reads them."""
        P = dict(
            # simple post-processing
            max_norm_energy=cfg.get('max_norm_energy', 0.2),
            discard_image_boundary=cfg.get('discard_image_boundary', False),
            min_boundary_obj_radius=cfg.get('min_boundary_obj_radius', 0),
            min_obj_radius=cfg.get('min_object_radius', 0),
            max_obj_radius=cfg.get('max_object_radius', np.inf),
            max_eccentricity=cfg.get('max_eccentricity', 0.99),
            max_boundary_eccentricity=cfg.get('max_boundary_eccentricity', np.inf),
            # contrast-based post-processing
            exterior_scale=cfg.get('exterior_scale', 5),
            exterior_offset=cfg.get('exterior_offset', 5),
            min_contrast=cfg.get('min_contrast', 1.35),
            contrast_epsilon=cfg.get('contrast_epsilon', 1e-4),
            # mask-based post-processing
            mask_stdamp=cfg.get('mask_stdamp', 2),
            mask_max_distance=cfg.get('mask_max_distance', 1),
            mask_smoothness=cfg.get('mask_smoothness', 3),
            fill_holes=cfg.get('fill_holes', True),
            # autofluorescence glare removal
            glare_detection_smoothness=cfg.get('glare_detection_smoothness', 3),
            glare_detection_num_layers=cfg.get('glare_detection_num_layers', 5),
            glare_detection_min_layer=cfg.get('glare_detection_min_layer', 0.5),
            min_glare_radius=cfg.get('min_glare_radius', np.inf))
        P['min_boundary_glare_radius'] = cfg.get('min_boundary_glare_radius', P['min_glare_radius'])
        if P['max_boundary_eccentricity'] is None:
            P['max_boundary_eccentricity'] = P['max_eccentricity']
        return P

    def _prepare_host(self, input_data, cfg):
        """Settings, cover, objects and the device images of one image."""
        import torch
        P = self._settings(cfg)
        g_raw = np.asarray(input_data['g_raw'], np.float64)
        solution = list(input_data['cover'].solution)
        # (the reference's filter reads the loop variable of the loop above, postprocess.py:180: all objects or none)
        objects = [obj for obj in solution if (solution[-1].fg_fragment.any() if solution else False)]
        g_dev = torch.as_tensor(np.ascontiguousarray(g_raw)).cuda()
        g_mask = gaussian_filter_gpu(g_dev, P['mask_smoothness'])
        # the mask is built where the image is: a caller that stands host arrays in for the device images (the CPU pipeline of the
        # regression-metric test does, through _process_objects and gaussian_filter_gpu) gets the host mask it always got
        offset = P['exterior_offset'] if torch.is_tensor(g_dev) else None
        return P, solution, objects, g_dev, g_mask, (solution, g_raw.shape, P['exterior_offset'], offset)

    @staticmethod
    def _background_masks(items):
        """The pixels allowed for the background estimate of the contrast (postprocess.py:152-155) of ``items`` = ``(solution, shape,
        exterior_offset, device_offset)`` per image: one launch per offset the device takes (:func:`background_mask_gpu_multi`), the
        SciPy erosion of the whole image for any other offset (``device_offset`` None: the image is not on a device)."""
        masks, groups = [None] * len(items), {}
        for i, (solution, shape, offset, device_offset) in enumerate(items):
            if background_radius(device_offset) is not None:
                groups.setdefault(background_radius(device_offset), []).append(i)
                continue
            background_mask = np.zeros(shape, bool)
            for c in solution:
                c.fill_foreground(background_mask)
            masks[i] = _morph.binary_erosion(~background_mask, _morph.disk(offset))
        for r, members in groups.items():
            for i, bg in zip(members, background_mask_gpu_multi([items[i][:2] for i in members], r)):
                masks[i] = bg
        return masks

    @staticmethod
    def _glare(items):
        """The glare test (postprocess.py:188-190) of ``items`` = ``(P, objects, g_dev)`` per image: per image a dict object index ->
        is_glare of the objects whose radius exceeds their glare radius.  The smoothed image stays on the device; one launch
        (:func:`glare_flags_gpu_multi`) per setting of the layers."""
        tested, groups = [], {}
        for i, (P, objects, g_dev) in enumerate(items):
            need = [k for k, o in enumerate(objects)
                    if (P['min_boundary_glare_radius'] if o.on_boundary else P['min_glare_radius']) < math.sqrt(o.fg_fragment.sum() / math.pi)]
            tested.append(dict.fromkeys(need, True))
            if need and P['glare_detection_num_layers'] >= 1:            # (without layers the reference's loop is empty: glare)
                glare_proportions(P['glare_detection_min_layer'], P['glare_detection_num_layers'])
                groups.setdefault((P['glare_detection_min_layer'], P['glare_detection_num_layers']), []).append(i)
        for (min_layer, num_layers), members in groups.items():
            images = [([items[i][1][k] for k in tested[i]], gaussian_filter_gpu(items[i][2], items[i][0]['glare_detection_smoothness'])) for i in members]
            for i, flags in zip(members, glare_flags_gpu_multi(images, min_layer, num_layers)):
                for k, row in zip(list(tested[i]), flags):
                    tested[i][k] = glare_decision(row)
        return tested

    def _run(self, inputs, cfgs, out, logs):
        """The stage for a set of images, ``inputs`` = the stage inputs of every image, ``cfgs`` = its stage config: the Gaussians image
        by image, then the background masks, the objects (:func:`_process_objects` with the hole filling behind the refinement) and the
        glare test of all images, each in one launch (images whose settings for a step differ go to launches of their own), then the
        decisions image by image.  Returns what every image produced and its records."""
        hosts = [self._prepare_host(inp, c) for inp, c in zip(inputs, cfgs)]
        masks = self._background_masks([h[5] for h in hosts])
        prepared = [(P, objects, g_dev, g_mask, bg) for (P, _, objects, g_dev, g_mask, _), bg in zip(hosts, masks)]
        keys = ('exterior_scale', 'exterior_offset', 'contrast_epsilon', 'mask_max_distance', 'mask_stdamp')
        groups = {}
        for i, prep in enumerate(prepared):
            groups.setdefault(tuple(prep[0][k] for k in keys) + (bool(prep[0]['fill_holes']),), []).append(i)
        per_object = [None] * len(prepared)
        for settings, members in groups.items():
            res = _process_objects([(prepared[i][1], prepared[i][2], prepared[i][3], prepared[i][4]) for i in members], *settings)
            for i, r in zip(members, res):
                per_object[i] = r
        glares = self._glare([prep[:3] for prep in prepared])
        produced = [self._decide(prep[0], prep[1], recs, final, glare, out, log)
                    for prep, (recs, final), glare, log in zip(prepared, per_object, glares, logs)]
        return produced, [r[0] for r in per_object]

    def process(self, input_data, cfg, out, log_root_dir):
        # one image is the set of one: it takes the route of process_many, which fills the refined windows while they are still on the
        # device
        (produced,), (self.last_records,) = self._run([input_data], [cfg], get_output(out), [log_root_dir])
        return produced

    def process_many(self, datas, cfg, out=None, log_root_dirs=None):
        """The stage for a set of images, with the contract of ``GlobalEnergyMinimization.process_many`` (a list of pipeline data
        dicts, one config for all or a list; returns the wall time).  Equal to ``process`` on every image; ``last_records`` becomes the
        list of the images' records."""
        t0 = time.time()
        datas = list(datas)
        cfgs = list(cfg) if isinstance(cfg, (list, tuple)) else [cfg] * len(datas)
        cfgs = [c.get(self.cfgns, {}) for c in cfgs]
        logs = list(log_root_dirs) if log_root_dirs is not None else [None] * len(datas)
        inputs = [{inner: d[outer] for outer, inner in self.inputs.items()} for d in datas]
        produced, self.last_records = self._run(inputs, cfgs, get_output(out), logs)
        for data, result in zip(datas, produced):
            for inner, outer in self.outputs.items():
                data[outer] = result[inner]
        return time.time() - t0

    def _decide(self, P, objects, recs, masks, glare, out, log_root_dir):
        """The host part of one image (postprocess.py:175-243): eccentricity, accept or discard.  ``masks``: the final mask (offset,
        fragment) of every object, holes filled where the settings say so, or None where the object keeps its own; ``glare``: object index
        -> is_glare of the tested objects."""
        postprocessed_objects, log_entries = [], []
        for k, original in enumerate(objects):
            obj_radius = math.sqrt(original.fg_fragment.sum() / math.pi)
            is_glare = glare.get(k, False)
            norm_energy = original.energy / original.cvxprog_region_size                    # postprocess.py:289-291 without the second distance transform
            contrast_response = float(recs['contrast'][k])
            fg_offset, fg_fragment = masks[k] if masks[k] is not None else (None, None)     # postprocess.py:316-337
            eccentricity = _compute_eccentricity(original.fg_fragment)

            obj = PostprocessedObject(original)
            if fg_fragment is not None and fg_offset is not None:
                obj.fg_fragment, obj.fg_offset = fg_fragment.copy(), np.asarray(fg_offset).copy()
                if not obj.fg_fragment.any():
                    log_entries.append((obj, 'empty foreground'))
                    continue
            if is_glare:
                log_entries.append((obj, f'glare removed (radius: {obj_radius})'))
                continue
            if norm_energy > P['max_norm_energy']:
                log_entries.append((obj, f'energy rate too high ({norm_energy})'))
                continue
            if contrast_response < P['min_contrast']:
                log_entries.append((obj, f'contrast too low ({contrast_response})'))
                continue
            if original.on_boundary:
                if eccentricity > P['max_boundary_eccentricity']:
                    log_entries.append((obj, f'boundary object eccentricity too high ({eccentricity})'))
                    continue
                if P['discard_image_boundary']:
                    log_entries.append((obj, 'boundary object discarded'))
                    continue
                if not (P['min_boundary_obj_radius'] <= obj_radius <= P['max_obj_radius']):
                    log_entries.append((obj, f'boundary object and/or too small/large (radius: {obj_radius})'))
                    continue
            else:
                if eccentricity > P['max_eccentricity']:
                    log_entries.append((obj, f'eccentricity too high ({eccentricity})'))
                    continue
                if not P['min_obj_radius'] <= obj_radius <= P['max_obj_radius']:
                    log_entries.append((obj, f'object too small/large (radius: {obj_radius})'))
                    continue
            postprocessed_objects.append(obj)

        if log_root_dir is not None:
            os.makedirs(log_root_dir, exist_ok=True)
            with open(os.path.join(log_root_dir, 'postprocessing.txt'), 'w') as log_file:
                for c, comment in log_entries:
                    location = (c.fg_offset + np.divide(c.fg_fragment.shape, 2)).round().astype(int)
                    log_file.write(f'object at x={location[1]}, y={location[0]}: {comment}{os.linesep}')
        out.write(f'Remaining objects: {len(postprocessed_objects)} of {len(objects)}')
        return {'postprocessed_objects': postprocessed_objects}

    def configure_ex(self, scale, radius, diameter):
        return {
            'min_object_radius': (radius, 0.0),
            'max_object_radius': (radius, np.inf),
            'min_glare_radius': (radius, np.inf),
        }
