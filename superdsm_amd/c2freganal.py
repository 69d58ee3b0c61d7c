"""Coarse-to-fine region analysis: ``y_mask``, atoms, adjacencies, seeds and clusters of an image (reference:
superdsm/c2freganal.py:82-288, ``C2F_RegionAnalysis``).

Two implementations of one stage live here:

* the definition: a plain, sequential restatement of the reference's ``process`` and ``_process_cluster_impl`` on NumPy / SciPy
  (:func:`region_analysis_host`), which takes the normalised-energy function as a parameter;
* the GPU path of the stage, for a set of images (:func:`region_analysis_gpu_multi`; :func:`region_analysis_gpu` is the set of one
  image): the cluster markers and the exact EDT of all images in HIP (``sdsm_c2f_markers_multi``, ``sdsm_edt_exact_multi``), then
  :func:`region_analysis_lockstep`: the marker flood in native host code (``sdsm_watershed``) and the split loops of all clusters
  of all images in lock step.  Every cluster advances until it needs energies, the requests of all clusters form one round, solved
  by ``engine.Batch`` plans of at most 16 cluster crops each, all queued on one stream.  The driver takes the flood and the solver
  of the rounds as parameters, so it runs without a GPU as well.

Both drive the same split loop (:func:`_split_cluster`, a generator that yields its energy requests).  The conventions the
restatement fixes where the reference leaves them to scikit-image or to chance are listed in DESIGN.md (row f5): the heap flood of
:func:`watershed`, the 4-connected labelling of the seed maxima and the lower label on equal scores, clusters in ascending label
order.
"""
import collections
import ctypes as C
import hashlib
import heapq
import math
import time

import numpy as np
import scipy.ndimage as ndi

from . import _capi, _morph
from .atoms import AtomAdjacencyGraph
from .c2f_energy import C2FError, energy_config, record_result
from .image import Image
from .imageset import SetLayout, in_sets
from .objects import CvxprogError, Object
from .output import get_output
from .pipeline import Stage

DEFAULTS = dict(seed_connectivity=8, min_atom_radius=15, max_atom_norm_energy=0.05, min_norm_energy_improvement=0.1,
                max_cluster_marker_irregularity=0.2)
MAX_CROPS_PER_PLAN = 16          # cluster crops per engine.Batch plan (sdsm_plan_create_multi takes 1 .. 16 images)
_CROP_ALIGN = 256                # elements: every crop of a round starts 256-element aligned in the packed device buffers


# ---- the definition: host restatement --------------------------------------------------------------------------------------------

def watershed(image, markers, mask=None):
    """The marker flood (``segm.watershed``) under the restated rule: 4-connectivity, neighbours visited up, left, right, down; the
    priority of a pixel is its own value, ties by push age, then by raster index; markers inside the mask are pushed first, in raster
    order, with age 0; a pixel is labelled when it is pushed; pixels outside the mask are never labelled."""
    image = np.asarray(image, np.float64)
    H, W = image.shape
    ok = np.ones(H * W, bool) if mask is None else np.asarray(mask, bool).ravel()
    lab = np.where(ok, np.asarray(markers).ravel(), 0).astype(np.int32)
    val = image.ravel().tolist()
    heap = [(val[p], 0, p) for p in np.flatnonzero(lab).tolist()]
    heapq.heapify(heap)
    age = 0
    while heap:
        p = heapq.heappop(heap)[2]
        r, c = divmod(p, W)
        for q, inside in ((p - W, r > 0), (p - 1, c > 0), (p + 1, c + 1 < W), (p + W, r + 1 < H)):
            if inside and ok[q] and lab[q] == 0:
                lab[q] = lab[p]
                age += 1
                heapq.heappush(heap, (val[q], age, q))
    return lab.reshape(H, W)


def watershed_native(image, markers, mask=None):
    """:func:`watershed` in native host code (``sdsm_watershed``)."""
    image = np.ascontiguousarray(image, np.float64)
    markers = np.ascontiguousarray(markers, np.int32)
    H, W = image.shape
    assert markers.shape == (H, W)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    out = np.empty((H, W), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _capi.check(_capi.lib().sdsm_watershed(p(image), p(markers), None if m is None else p(m), H, W, p(out)), 'sdsm_watershed')
    return out


def _normalize_labels_map(labels, first_label=0, skip_labels=()):
    """c2freganal.py:38-47: the present labels, sorted and without ``skip_labels``, renumbered from ``first_label``."""
    present = np.unique(labels)
    keep = present[~np.isin(present, list(skip_labels))]
    result = np.zeros_like(labels)
    new = np.arange(first_label, first_label + len(keep))
    if len(keep):
        pos = np.searchsorted(keep, labels)
        hit = (pos < len(keep)) & (keep[np.minimum(pos, len(keep) - 1)] == labels)
        result[hit] = new[pos[hit]]
    return result, {int(o): int(n) for o, n in zip(keep, new)}


def cluster_markers_host(y, max_cluster_marker_irregularity):
    """The first lines of ``process`` (c2freganal.py:110-123): ``(y_mask, cluster_markers)``."""
    y = np.asarray(y)
    fg_mask = y > 0
    fg_bd = np.logical_xor(fg_mask, _morph.binary_erosion(fg_mask, _morph.disk(1)))
    cluster_markers = ndi.label(fg_mask)[0]
    n = int(cluster_markers.max())
    area = np.bincount(cluster_markers.ravel(), minlength=n + 1)
    bd = np.bincount(cluster_markers[fg_bd], minlength=n + 1)
    present = area > 0                                  # label 0 only if there is background
    irregular = np.zeros(n + 1, bool)
    irregular[present] = bd[present] / area[present] > max_cluster_marker_irregularity
    y_mask = ~irregular[cluster_markers]
    cluster_markers[~y_mask] = cluster_markers.min()
    return y_mask, _normalize_labels_map(cluster_markers, first_label=0)[0]


def _get_next_seed(region, where, score, connectivity=4):
    """c2freganal.py:15-28: the local maxima of ``region.model`` inside ``region.mask & where`` (window maximum with mode
    'reflect'), labelled 4-connected; the one with the highest maximum of ``score`` wins, the lower label on equal scores."""
    if connectivity == 4:
        footprint = _morph.disk(1)
    elif connectivity == 8:
        footprint = np.ones((3, 3))
    else:
        raise ValueError(f'unknown connectivity: {connectivity}')
    mask = np.logical_and(region.mask, where)
    image = region.model
    image_max = ndi.maximum_filter(image, footprint=footprint)
    max_mask = np.logical_and(image_max == image, mask)
    if max_mask.any():
        maxima, n = ndi.label(max_mask)
        labels = np.arange(1, n + 1)
        scores = np.asarray(ndi.maximum(score, maxima, labels))
        best = 0
        for i in range(1, n):                           # max() over ascending labels: the first maximum wins
            if scores[i] > scores[best]:
                best = i
        if scores[best] > -np.inf:
            return maxima == labels[best]
    return None


def _watershed_split(region, markers, flood):
    """c2freganal.py:31-35, with the flood as a parameter."""
    markers_map = np.zeros(region.model.shape, np.int32)
    for marker_label, marker in enumerate(markers, start=1):
        if marker.sum() != 1:
            # `assert markers_map[marker] == 0` of the reference cannot evaluate a seed of several pixels (ValueError)
            raise C2FError(f'a split seed of {int(marker.sum())} pixels')
        assert not markers_map[marker].any()
        markers_map[marker] = marker_label
    ws = flood(region.model.max() - region.model.clip(0, np.inf), markers_map, region.mask)
    return [ws == marker_label for marker_label in range(1, len(markers) + 1)]


def _hash_mask(mask):
    return hashlib.sha1(np.ascontiguousarray(mask, np.uint8)).digest()


def _split_cluster(cluster_label, cluster, masked_cluster, params, flood):
    """``_process_cluster_impl`` (c2freganal.py:215-288) as a state machine: a generator that yields ``(atoms_map, footprints)``
    whenever it needs normalised energies the cache of the cluster does not hold, is sent one result per footprint (a float, None or
    the exception its computation raised) and returns ``(leaf_candidates, atoms_map)``."""
    min_atom_size = math.pi * (params['min_atom_radius'] ** 2)
    max_atom_norm_energy = params['max_atom_norm_energy']
    min_norm_energy_improvement = params['min_norm_energy_improvement']
    connectivity = params['seed_connectivity']
    cache = {}

    def energies(objs):
        keys = [_hash_mask(np.logical_and(masked_cluster.mask, o.get_mask(atoms_map))) for o in objs]
        todo = {}
        for k, o in zip(keys, objs):
            if k not in cache and k not in todo:
                todo[k] = sorted(o.footprint)
        if todo:
            results = yield atoms_map, list(todo.values())
            cache.update(zip(todo, results))
        return [cache[k] for k in keys]

    root_candidate = Object()
    root_candidate.footprint = frozenset([1])
    root_candidate.seed = _get_next_seed(masked_cluster, cluster.model > 0, cluster.model, connectivity)
    atoms_map = cluster.mask.astype(int) * 1
    leaf_candidates = []
    split_queue = collections.deque()
    (energy,) = yield from energies([root_candidate])
    if isinstance(energy, Exception):
        raise energy                                    # the root's errors propagate
    if energy is None:
        raise C2FError(f'cluster {cluster_label}: its region has no normalised energy (all intensities have one sign)')
    root_candidate.normalized_energy = energy
    if root_candidate.normalized_energy > max_atom_norm_energy:
        split_queue.append(root_candidate)
    else:
        leaf_candidates.append(root_candidate)
    if root_candidate.seed is None:
        raise C2FError(f'cluster {cluster_label}: no seed (no local maximum of y > 0 inside y_mask)')

    seed_distances = ndi.distance_transform_edt(~root_candidate.seed)
    while split_queue:
        c0 = split_queue.popleft()
        c0_mask = c0.get_mask(atoms_map)
        if c0_mask.sum() < 2 * min_atom_size:
            leaf_candidates.append(c0)                  # the region is too small to be split
            continue
        c1, c2 = Object(), Object()
        c1.seed = c0.seed
        c2.seed = _get_next_seed(masked_cluster, np.all((cluster.model > 0, c0_mask, seed_distances >= 1), axis=0), seed_distances,
                                 connectivity)
        if c2.seed is None:
            leaf_candidates.append(c0)
            continue
        assert not np.logical_and(c1.seed, c2.seed).any()
        seed_distances = np.minimum(seed_distances, ndi.distance_transform_edt(~c2.seed))
        new_atom_label = atoms_map.max() + 1
        try:
            c1_mask, c2_mask = _watershed_split(cluster.get_region(c0_mask), (c1.seed, c2.seed), flood)
        except C2FError as e:
            raise C2FError(f'cluster {cluster_label}: {e}') from None
        if c1_mask.sum() < min_atom_size:
            c0.seed = c2.seed                           # change the seed for the current region ...
            split_queue.append(c0)                      # ... and try again with a different seed
            continue
        if c2_mask.sum() < min_atom_size:
            split_queue.append(c0)                      # try again with a different seed
            continue
        atoms_map_previous = atoms_map.copy()
        atoms_map[c2_mask] = new_atom_label
        c1.footprint = frozenset(c0.footprint)
        c2.footprint = frozenset([new_atom_label])
        assert c1_mask[cluster.mask].any() and not np.logical_and(~cluster.mask, c1_mask).any()
        assert c2_mask[cluster.mask].any() and not np.logical_and(~cluster.mask, c2_mask).any()
        e1, e2 = yield from energies([c1, c2])
        c1.normalized_energy = None if isinstance(e1, Exception) else e1      # c2freganal.py:250-254
        c2.normalized_energy = None if isinstance(e2, Exception) else e2
        if c1.normalized_energy is None and c2.normalized_energy is None:
            split_queue.append(c0)
            atoms_map = atoms_map_previous
            continue
        if c1.normalized_energy is None and c2.normalized_energy is not None:
            c0.seed = c2.seed
            split_queue.append(c0)
            atoms_map = atoms_map_previous
            continue
        if c1.normalized_energy is not None and c2.normalized_energy is None:
            split_queue.append(c0)
            atoms_map = atoms_map_previous
            continue
        norm_energy_improvement = 1 - max((c1.normalized_energy, c2.normalized_energy)) / c0.normalized_energy
        if norm_energy_improvement < min_norm_energy_improvement:
            split_queue.append(c0)
            atoms_map = atoms_map_previous
        else:
            for c in (c1, c2):
                if c.normalized_energy > max_atom_norm_energy:
                    split_queue.append(c)
                else:
                    leaf_candidates.append(c)

    assert frozenset(list(c.footprint)[0] for c in leaf_candidates) == frozenset(atoms_map.reshape(-1)) - {0}
    return leaf_candidates, atoms_map


def _cluster_regions(y, y_mask, clusters, cluster_label, box=None):
    """``y.get_region(clusters == cluster_label, shrink=True)`` and its part inside ``y_mask``; ``box`` (the cluster's slices, as
    ``ndi.find_objects`` returns them) spares the comparison over the whole image.  ``full_mask`` is left at the crop's mask."""
    if box is None:
        box = ndi.find_objects(np.asarray(clusters == cluster_label, np.int32))[0]
    mask = np.logical_and(clusters[box] == cluster_label, y.mask[box])
    cluster = Image(y.model[box], mask, offset=(np.int64(box[0].start), np.int64(box[1].start)))
    return cluster, cluster.get_region(cluster.shrink_mask(y_mask))


def _process_cluster_impl(clusters, cluster_label, y, y_mask, params, dsm_cfg, energy, flood=watershed, box=None):
    """One cluster, sequentially: ``energy(y_crop, mask_crop, atoms_map, footprint, dsm_cfg)`` is asked one footprint at a time.
    Returns ``(cluster, leaf_candidates, atoms_map)``."""
    cluster, masked_cluster = _cluster_regions(y, y_mask, clusters, cluster_label, box)
    steps = _split_cluster(cluster_label, cluster, masked_cluster, params, flood)
    try:
        request = next(steps)
        while True:
            atoms_map, footprints = request
            results = []
            for fp in footprints:
                try:
                    results.append(energy(cluster.model, masked_cluster.mask, atoms_map, fp, dsm_cfg))
                except Exception as e:          # noqa: BLE001 -- c2freganal.py:250-254 catches everything
                    results.append(e)
            request = steps.send(results)
    except StopIteration as stop:
        leaf_candidates, atoms_map = stop.value
    return cluster, leaf_candidates, atoms_map


def _assemble(y, y_mask, clusters, per_cluster):
    """c2freganal.py:145-175: atom labels offset cluster by cluster (ascending cluster label), seeds, normalised labels,
    adjacency graph."""
    atoms_map = np.zeros(y.shape, int)
    atom_candidate_by_label = {}
    top = 0                                             # atoms_map.max() so far
    for cluster, leaf_candidates, cluster_atoms_map in per_cluster:
        offset = top
        (r0, r1), (c0, c1) = [(int(o), int(o) + s) for o, s in zip(cluster.offset, cluster.mask.shape)]
        box = atoms_map[r0:r1, c0:c1]
        box[cluster.mask] = offset + cluster_atoms_map[cluster.mask]
        top = max(top, int(box.max()))
        for c in leaf_candidates:
            atom_candidate_by_label[offset + list(c.footprint)[0]] = c
            c.seed = np.round(ndi.center_of_mass(c.seed)).astype(int) + np.asarray(cluster.offset, int)
    atoms_map, label_translation = _normalize_labels_map(atoms_map, first_label=1, skip_labels=[0])
    atom_candidate_by_label = {label_translation[old]: c for old, c in atom_candidate_by_label.items()}
    seeds = [atom_candidate_by_label[label].seed for label in sorted(label_translation.values())]
    adjacencies = AtomAdjacencyGraph(atoms_map, clusters, y > 0, seeds)
    return {'y_mask': y_mask, 'atoms': atoms_map, 'adjacencies': adjacencies, 'seeds': seeds, 'clusters': clusters}


def _params(cfg=None, **overrides):
    params = {k: (cfg.get(k, v) if cfg is not None else v) for k, v in DEFAULTS.items()}
    params.update({k: v for k, v in overrides.items() if v is not None})
    return params


def normalized_energy_one(y_crop, mask_crop, atoms_map, footprint, dsm_cfg):
    """One request of the restatement answered by ``c2f_energy.normalized_energies`` on its own."""
    from . import c2f_energy
    return c2f_energy.normalized_energies(y_crop, mask_crop, atoms_map, [footprint], dsm_cfg)[0]


def region_analysis_host(y, dsm_cfg, energy=normalized_energy_one, flood=watershed, **params):
    """The definition of the stage (c2freganal.py:103-175): SciPy markers and EDT, the Python heap flood, clusters in ascending label
    order, ``energy`` asked one footprint at a time."""
    params = _params(**params)
    dsm_cfg = dict(dsm_cfg)
    dsm_cfg['smooth_amount'] = np.inf
    y = np.asarray(y, np.float64)
    y_mask, cluster_markers = cluster_markers_host(y, params['max_cluster_marker_irregularity'])
    clusters = flood(ndi.distance_transform_edt(cluster_markers == 0), cluster_markers)
    yi = Image.create_from_array(y, normalize=False)
    boxes = ndi.find_objects(clusters)
    per_cluster = [_process_cluster_impl(clusters, label, yi, y_mask, params, dsm_cfg, energy, flood, boxes[label - 1])
                   for label in range(1, len(boxes) + 1) if boxes[label - 1] is not None]
    return _assemble(y, y_mask, clusters, per_cluster)


# ---- the GPU path ----------------------------------------------------------------------------------------------------------------

def _device():
    import torch
    if not torch.cuda.is_available():
        raise _capi.SdsmError('no HIP device available: the region analysis has no CPU fallback')
    return torch


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def cluster_markers_gpu(y, max_cluster_marker_irregularity):
    """``sdsm_c2f_markers``: ``(y_mask, cluster_markers)`` as :func:`cluster_markers_host` computes them, plus the device copies
    ``(d_markers, count)``."""
    torch = _device()
    L = _capi.lib()
    d_y = y.to('cuda', torch.float64).contiguous() if torch.is_tensor(y) else torch.from_numpy(np.ascontiguousarray(y, np.float64)).cuda()
    H, W = (int(v) for v in d_y.shape)
    d_mask = torch.empty((H, W), dtype=torch.uint8, device=d_y.device)
    d_markers = torch.empty((H, W), dtype=torch.int32, device=d_y.device)
    d_count = torch.zeros(1, dtype=torch.int32, device=d_y.device)
    nbytes = L.sdsm_c2f_markers_workspace_bytes(H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d_y.device)
    _capi.check(L.sdsm_c2f_markers(C.c_void_p(d_y.data_ptr()), H, W, float(max_cluster_marker_irregularity), C.c_void_p(d_mask.data_ptr()),
                                   C.c_void_p(d_markers.data_ptr()), C.c_void_p(d_count.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes,
                                   _stream(torch)), 'sdsm_c2f_markers')
    return d_mask.cpu().numpy().astype(bool), d_markers.cpu().numpy(), d_markers, int(d_count.item())


def edt_exact_gpu(target):
    """``sdsm_edt_exact``: ``ndi.distance_transform_edt(target == 0)`` (``target``: array or device tensor, nonzero = target)."""
    torch = _device()
    L = _capi.lib()
    d_t = (target != 0).to('cuda', torch.uint8).contiguous() if torch.is_tensor(target) else \
        torch.from_numpy(np.ascontiguousarray(np.asarray(target) != 0, np.uint8)).cuda()
    H, W = (int(v) for v in d_t.shape)
    out = torch.empty((H, W), dtype=torch.float64, device=d_t.device)
    nbytes = L.sdsm_edt_exact_workspace_bytes(H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d_t.device)
    _capi.check(L.sdsm_edt_exact(C.c_void_p(d_t.data_ptr()), H, W, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes,
                                 _stream(torch)), 'sdsm_edt_exact')
    return out.cpu().numpy()


def markers_and_edt_gpu_multi(ys, max_cluster_marker_irregularity):
    """:func:`cluster_markers_gpu` and then :func:`edt_exact_gpu` of the markers, for a set of images: one packed upload of all ``y``,
    ``sdsm_c2f_markers_multi`` and ``sdsm_edt_exact_multi`` over up to ``_capi.MAX_SET_IMAGES`` images per call, one download per kind of result.
    ``max_cluster_marker_irregularity``: one threshold for all or one per image.  Returns ``(y_mask, cluster_markers, count,
    distances)`` per image, equal to the single-image functions."""
    torch = _device()
    L = _capi.lib()
    ys = [np.asarray(y, np.float64) for y in ys]
    thrs = list(max_cluster_marker_irregularity) if np.ndim(max_cluster_marker_irregularity) else [max_cluster_marker_irregularity] * len(ys)
    results = []
    for part in in_sets(len(ys)):
        lay = SetLayout([y.shape for y in ys[part]], align=_CROP_ALIGN)
        table, total, n = lay.table, lay.total, len(lay.shapes)
        d_y = torch.from_numpy(lay.pack(ys[part], np.float64)).cuda()
        # one buffer for everything that comes back: distances (float64), markers (int32), y_mask (uint8), counts (int32)
        d_res = torch.empty(13 * total + 4 * n, dtype=torch.uint8, device=d_y.device)
        d_dist = d_res[:8 * total].view(torch.float64)
        d_markers = d_res[8 * total:12 * total].view(torch.int32)
        d_mask = d_res[12 * total:13 * total]
        d_count = d_res[13 * total:].view(torch.int32)
        thr = (C.c_double * n)(*[float(t) for t in thrs[part]])
        m_bytes = L.sdsm_c2f_markers_workspace_bytes_multi(table, n)
        e_bytes = L.sdsm_edt_exact_workspace_bytes_multi(table, n)
        ws = torch.empty(max(m_bytes, e_bytes), dtype=torch.uint8, device=d_y.device)     # the EDT follows the markers on one stream
        p = lambda t: C.c_void_p(t.data_ptr())
        _capi.check(L.sdsm_c2f_markers_multi(table, n, p(d_y), thr, p(d_mask), p(d_markers), p(d_count), p(ws), m_bytes, _stream(torch)),
                    'sdsm_c2f_markers_multi')
        d_target = (d_markers != 0).to(torch.uint8)
        _capi.check(L.sdsm_edt_exact_multi(table, n, p(d_target), p(d_dist), p(ws), e_bytes, _stream(torch)), 'sdsm_edt_exact_multi')
        # one download per kind of result, as the calls for a single image make them: the 13 bytes per pixel in one piece pass the
        # size (4 MiB) from which the runtime pins the host buffer in place already for one 520 x 696 image, and releasing such a
        # buffer stalls the queues for 20 - 30 ms in the energy round that follows
        dist, markers = lay.unpack(d_dist.cpu().numpy()), lay.unpack(d_markers.cpu().numpy())
        mask, count = lay.unpack(d_mask.cpu().numpy()), d_count.cpu().numpy()
        results += [(mask[k].astype(bool), markers[k], int(count[k]), dist[k]) for k in range(n)]
    return results


def edt_exact_gpu_multi(targets):
    """:func:`edt_exact_gpu` of every image of a set (``sdsm_edt_exact_multi``, up to ``_capi.MAX_SET_IMAGES`` images per call)."""
    torch = _device()
    L = _capi.lib()
    targets = [np.asarray(t) != 0 for t in targets]
    out = []
    for part in in_sets(len(targets)):
        lay = SetLayout([t.shape for t in targets[part]], align=_CROP_ALIGN)
        table, n = lay.table, len(lay.shapes)
        d_t = torch.from_numpy(lay.pack(targets[part], np.uint8)).cuda()
        d_out = torch.empty(lay.total, dtype=torch.float64, device=d_t.device)
        nbytes = L.sdsm_edt_exact_workspace_bytes_multi(table, n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=d_t.device)
        _capi.check(L.sdsm_edt_exact_multi(table, n, C.c_void_p(d_t.data_ptr()), C.c_void_p(d_out.data_ptr()), C.c_void_p(ws.data_ptr()),
                                           nbytes, _stream(torch)), 'sdsm_edt_exact_multi')
        out += lay.unpack(d_out.cpu().numpy())
    return out


class _CropImage:
    """What ``engine.Batch`` needs of a ``DeviceImage``, for one cluster crop of a round: views into the round's packed buffers."""

    def __init__(self, device, H, W, n_atoms, margin, y, atoms, valid):
        self.device, self.H, self.W, self.n_atoms, self.background_margin = device, H, W, n_atoms, margin
        self.y, self.atoms, self.valid = y, atoms, valid
        self.atom_stats = None


class EnergyRounds:
    """Solves the energy requests of many cluster crops at once: one upload of the packed crops, ``sdsm_image_prepare`` per crop,
    plans of at most 16 crops queued on the current stream, candidates given up by a workgroup group solved again without groups
    (mode 2)."""

    def __init__(self, dsm_cfg):
        self.cfg, self.margin = energy_config(dsm_cfg)
        self.log = []                                   # per round: dict(crops, plans, candidates, resolved, seconds)

    @property
    def launches(self):
        return sum(r['plans'] + r['resolve_plans'] for r in self.log)

    def solve(self, requests):
        """requests: ``(y_crop, mask_crop, atoms_map, footprints)`` per crop; returns one list of results per request."""
        from . import engine
        torch = _device()
        L = _capi.lib()
        t0 = time.perf_counter()
        dev = torch.device('cuda', torch.cuda.current_device())
        shapes = [r[0].shape for r in requests]
        sizes = [int(h) * int(w) for h, w in shapes]
        offs = np.zeros(len(requests) + 1, np.int64)
        np.cumsum([(s + _CROP_ALIGN - 1) // _CROP_ALIGN * _CROP_ALIGN for s in sizes], out=offs[1:])
        y_all = np.zeros(offs[-1], np.float64)
        m_all = np.zeros(offs[-1], np.uint8)
        a_all = np.zeros(offs[-1], np.int32)
        n_atoms = []
        for k, (y, m, a, _) in enumerate(requests):
            y_all[offs[k]:offs[k] + sizes[k]] = y.ravel()
            m_all[offs[k]:offs[k] + sizes[k]] = m.ravel()
            a_all[offs[k]:offs[k] + sizes[k]] = a.ravel()
            n_atoms.append(int(a.max()))
        d_y, d_m, d_a = (torch.from_numpy(v).to(dev) for v in (y_all, m_all, a_all))
        d_valid = torch.empty(int(offs[-1]), dtype=torch.uint8, device=dev)
        soffs = np.zeros(len(requests) + 1, np.int64)
        np.cumsum([(na + 1) * _capi.ATOM_STATS_STRIDE for na in n_atoms], out=soffs[1:])
        d_stats = torch.empty(int(soffs[-1]), dtype=torch.int32, device=dev)
        ws_bytes = max(L.sdsm_image_workspace_bytes(int(h), int(w)) for h, w in shapes)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)       # one stream: the prepares run one after the other
        stream = _stream(torch)
        images = []
        for k, (h, w) in enumerate(shapes):
            o, n = int(offs[k]), sizes[k]
            im = _CropImage(dev, int(h), int(w), n_atoms[k], self.margin, d_y[o:o + n], d_a[o:o + n], d_valid[o:o + n])
            _capi.check(L.sdsm_image_prepare(C.c_void_p(im.y.data_ptr()), C.c_void_p(d_m[o:o + n].data_ptr()), C.c_void_p(im.atoms.data_ptr()),
                                             im.H, im.W, self.margin, im.n_atoms, C.c_void_p(im.valid.data_ptr()),
                                             C.c_void_p(d_stats[int(soffs[k]):].data_ptr()), C.c_void_p(ws.data_ptr()), ws_bytes, stream),
                        'sdsm_image_prepare')
            images.append(im)
        stats = d_stats.cpu().numpy()                   # synchronises: the planner needs the per-atom statistics on the host
        for k, im in enumerate(images):
            im.atom_stats = np.ascontiguousarray(stats[int(soffs[k]):int(soffs[k + 1])])
        # plans of at most 16 crops
        batches = []
        for lo in range(0, len(requests), MAX_CROPS_PER_PLAN):
            ks = range(lo, min(lo + MAX_CROPS_PER_PLAN, len(requests)))
            fps = [list(fp) for k in ks for fp in requests[k][3]]
            image_of = [j for j, k in enumerate(ks) for _ in requests[k][3]]
            b = engine.Batch([images[k] for k in ks], fps, self.cfg, latency_mode=True, image_of=image_of)
            b.starting_points(self.cfg.get('init'))
            b.launch()
            batches.append(b)
        recs = torch.cat([b.records_dev[:b.n * _capi.RECORD_DTYPE.itemsize] for b in batches]).cpu().numpy().view(_capi.RECORD_DTYPE).copy()
        # candidates a workgroup group gave up: again, in plans without groups; only their rows are read back
        resolved, resolve_plans, first = 0, 0, 0
        for b in batches:
            again = b.resolve_given_up(recs['status'][first:first + b.n])
            if again.size:
                recs[first + again] = rr = b.records(again)
                if (rr['status'] == _capi.CAND_GIVEN_UP).any():
                    raise C2FError('a candidate was given up in a plan without workgroup groups')
                resolved, resolve_plans = resolved + again.size, resolve_plans + 1
            first += b.n
        results, i = [], 0
        for r in requests:
            results.append([record_result(recs[i + j], i + j) for j in range(len(r[3]))])
            i += len(r[3])
        self.log.append(dict(crops=len(requests), plans=len(batches), candidates=len(recs), resolved=int(resolved),
                             resolve_plans=resolve_plans, seconds=time.perf_counter() - t0))
        return results


def _same_config(a, b):
    try:
        return bool(a == b)
    except Exception:                                   # noqa: BLE001 -- values without a truth value of ==: treat as different
        return False


def region_analysis_lockstep(ys, dsm_cfgs, params, marked, flood=watershed_native, new_rounds=EnergyRounds):
    """The host part of the stage for a set of images, after the device phase: ``marked`` holds ``(y_mask, cluster_markers, count,
    distances)`` per image (:func:`markers_and_edt_gpu_multi`).  The flood per image, then the split loops of ALL clusters of ALL
    images in lock step, keyed ``(image, label)`` and taken in that order: every cluster advances until it needs energies, and every
    round's requests go through one ``solve`` per distinct energy configuration (one for a set with one configuration).
    ``new_rounds(dsm_cfg)`` makes the object that answers them, once per distinct configuration; of it only ``solve(requests)``,
    ``log`` and ``launches`` are read (:class:`EnergyRounds`).  A candidate's record does not depend on the plan it is solved in
    (DESIGN.md section 4), so every image's outputs are those of the image alone, and the set takes as many rounds as its image with
    the most.

    ``dsm_cfgs`` / ``params``: one per image.  An image whose split fails (``C2FError``, ``CvxprogError``) leaves the set; the others
    finish.  Returns ``(outputs, stats, set_stats, errors)``: per image its outputs (None where it failed), its phase timings (the
    energy rounds shared evenly) and its error (or None)."""
    t_all = time.perf_counter()
    n = len(ys)
    params = [_params(**p) for p in params]
    dsm_cfgs = [dict(c, smooth_amount=np.inf) for c in dsm_cfgs]
    ys = [np.asarray(y, np.float64) for y in ys]
    stats = [dict(rounds=[], host_split_s=0.0) for _ in range(n)]
    errors = [None] * n
    groups = []                                         # (energy configuration, rounds object, images)
    for i, c in enumerate(dsm_cfgs):
        key = energy_config(c)
        for g in groups:
            if _same_config(g[0], key):
                g[2].append(i)
                break
        else:
            groups.append((key, new_rounds(c), [i]))
    flood_s = 0.0
    clusters, labels, images = [None] * n, [None] * n, [None] * n
    for i, (y, (y_mask, cluster_markers, _, distances)) in enumerate(zip(ys, marked)):
        tf = time.perf_counter()
        clusters[i] = flood(distances, cluster_markers)
        stats[i]['flood_s'] = time.perf_counter() - tf
        flood_s += stats[i]['flood_s']
        images[i] = Image.create_from_array(y, normalize=False)

    done, pending = [dict() for _ in range(n)], {}

    def fail(i, e):
        errors[i] = e
        for k in [k for k in pending if k[0] == i]:
            del pending[k]

    host_s = 0.0
    for i in range(n):
        th = time.perf_counter()
        boxes = ndi.find_objects(clusters[i])
        labels[i] = [label for label in range(1, len(boxes) + 1) if boxes[label - 1] is not None]
        for label in labels[i]:
            cluster, masked_cluster = _cluster_regions(images[i], marked[i][0], clusters[i], label, boxes[label - 1])
            steps = _split_cluster(label, cluster, masked_cluster, params[i], flood)
            try:
                pending[i, label] = (cluster, masked_cluster, steps, next(steps))
            except StopIteration as stop:
                done[i][label] = (cluster, *stop.value)
            except (C2FError, CvxprogError) as e:
                fail(i, e)
                break
        dt = time.perf_counter() - th
        stats[i]['host_split_s'] += dt
        host_s += dt
    n_rounds = 0
    while pending:
        n_rounds += 1
        order = sorted(pending)
        for i in sorted({k[0] for k in order}):
            stats[i]['rounds'].append(dict(crops=sum(1 for k in order if k[0] == i)))
        for _, rounds, members in groups:
            keys = [k for k in order if k[0] in members]
            if not keys:
                continue
            requests = [(pending[k][0].model, pending[k][1].mask, pending[k][3][0], pending[k][3][1]) for k in keys]
            results = rounds.solve(requests)
            for k, res in zip(keys, results):
                if k not in pending:                    # its image failed earlier in this round
                    continue
                th = time.perf_counter()
                cluster, masked_cluster, steps, _ = pending.pop(k)
                try:
                    pending[k] = (cluster, masked_cluster, steps, steps.send(res))
                except StopIteration as stop:
                    done[k[0]][k[1]] = (cluster, *stop.value)
                except (C2FError, CvxprogError) as e:
                    fail(k[0], e)
                dt = time.perf_counter() - th
                stats[k[0]]['host_split_s'] += dt
                host_s += dt
    outputs = [None] * n
    assemble_s = 0.0
    for i in range(n):
        if errors[i] is not None:
            continue
        ta = time.perf_counter()
        outputs[i] = _assemble(ys[i], marked[i][0], clusters[i], [done[i][k] for k in labels[i]])
        stats[i].update(assemble_s=time.perf_counter() - ta, clusters=len(labels[i]))
        assemble_s += stats[i]['assemble_s']
    logs = [r for _, rounds, _ in groups for r in rounds.log]
    set_stats = dict(images=n, flood_s=flood_s, host_split_s=host_s, assemble_s=assemble_s, n_rounds=n_rounds, rounds=logs,
                     launches=sum(rounds.launches for _, rounds, _ in groups), energy_s=sum(r['seconds'] for r in logs),
                     total_s=time.perf_counter() - t_all)
    for st in stats:
        st['energy_s'] = set_stats['energy_s'] / max(n, 1)
    return outputs, stats, set_stats, errors


def region_analysis_gpu_multi(ys, dsm_cfgs, params):
    """The stage's GPU path for a set of images: the markers and EDT of all images in one pass (:func:`markers_and_edt_gpu_multi`),
    then :func:`region_analysis_lockstep` with the native flood and :class:`EnergyRounds`.  Returns what it returns, with the wall
    clock of the device phase (``markers_edt_s``, per image an even share) added to the stats."""
    t0 = time.perf_counter()
    ys = [np.asarray(y, np.float64) for y in ys]
    params = [_params(**p) for p in params]
    marked = markers_and_edt_gpu_multi(ys, [p['max_cluster_marker_irregularity'] for p in params])
    markers_edt_s = time.perf_counter() - t0
    outputs, stats, set_stats, errors = region_analysis_lockstep(ys, dsm_cfgs, params, marked)
    set_stats.update(markers_edt_s=markers_edt_s, total_s=time.perf_counter() - t0)
    for st in stats:
        st['markers_edt_s'] = markers_edt_s / max(len(ys), 1)
    return outputs, stats, set_stats, errors


def _set_of_one(outputs, stats, set_stats, errors):
    """What a set of one image returned, as the call for a single image returns it: ``(outputs, stats)``, the image's stats updated
    with the set's (``rounds`` is then the log of the energy rounds); the image's own exception is raised if it failed."""
    if errors[0] is not None:
        raise errors[0]
    return outputs[0], dict(stats[0], **set_stats)


def region_analysis_gpu(y, dsm_cfg, **params):
    """The stage's GPU path for one image, the set of this image (:func:`region_analysis_gpu_multi`); returns ``(outputs, stats)``
    with the wall clock of every phase and the log of the energy rounds."""
    return _set_of_one(*region_analysis_gpu_multi([y], [dsm_cfg], [params]))


class C2F_RegionAnalysis(Stage):
    """The coarse-to-fine region analysis (c2freganal.py:82-207): requires ``y`` and ``dsm_cfg``, produces ``y_mask``, ``atoms``,
    ``adjacencies``, ``seeds`` and ``clusters``.  Hyper-parameters (``c2f-region-analysis/...``) and defaults as in the reference:
    ``seed_connectivity`` (8), ``min_atom_radius`` (15, or ``AF_min_atom_radius`` x radius with a default factor of 0.33),
    ``max_atom_norm_energy`` (0.05), ``min_norm_energy_improvement`` (0.1), ``max_cluster_marker_irregularity`` (0.2).  Runs
    :func:`region_analysis_gpu_multi`, for ``process`` on the set of its one image; the phase timings and the energy rounds of the
    last call are kept in ``last_stats``."""

    ENABLED_BY_DEFAULT = True

    def __init__(self):
        super().__init__('c2f-region-analysis', inputs=['y', 'dsm_cfg'], outputs=['y_mask', 'atoms', 'adjacencies', 'seeds', 'clusters'])
        self.last_stats = None

    def process(self, input_data, cfg, out, log_root_dir):
        out.intermediate('Analyzing cluster markers...')
        result, self.last_stats = region_analysis_gpu(input_data['y'], input_data['dsm_cfg'], **_params(cfg))
        out.write(f'Extracted {self.last_stats["clusters"]} clusters, {int(result["atoms"].max())} atoms '
                  f'({len(self.last_stats["rounds"])} energy rounds)')
        return result

    def process_many(self, datas, cfg, out=None, log_root_dirs=None):
        """The stage for a set of images (:func:`region_analysis_gpu_multi`), with the contract of
        ``GlobalEnergyMinimization.process_many``: ``datas`` is a list of pipeline data dicts (inputs read from, outputs written to
        each), ``cfg`` one config for all or a list; returns the wall time.  The outputs of every image equal those of ``process`` on
        it alone.  ``last_stats`` becomes the list of the images' stats, ``last_set_stats`` those of the set.  An image that fails
        (``C2FError``, ``CvxprogError``) gets no outputs; the others do, and then the first failure is raised with ``image_index``,
        ``image_indices`` (every failed image) and ``image_errors`` (image -> its exception)."""
        datas = list(datas)
        cfgs = list(cfg) if isinstance(cfg, (list, tuple)) else [cfg] * len(datas)
        cfgs = [c.get(self.cfgns, {}) for c in cfgs]
        out = get_output(out)
        t0 = time.time()
        outputs, self.last_stats, self.last_set_stats, errors = region_analysis_gpu_multi(
            [d['y'] for d in datas], [d['dsm_cfg'] for d in datas], [_params(c) for c in cfgs])
        for i, (data, result) in enumerate(zip(datas, outputs)):
            if result is None:
                continue
            for inner, outer in self.outputs.items():
                data[outer] = result[inner]
            out.write(f'Image {i}: extracted {self.last_stats[i]["clusters"]} clusters, {int(result["atoms"].max())} atoms '
                      f'({len(self.last_stats[i]["rounds"])} energy rounds)')
        failed = [i for i, e in enumerate(errors) if e is not None]
        if failed:
            e = errors[failed[0]]
            e.image_index, e.image_indices, e.image_errors = failed[0], failed, {i: errors[i] for i in failed}
            raise e
        return time.time() - t0

    def configure_ex(self, scale, radius, diameter):
        return {
            'min_atom_radius': (radius, 0.33, dict(type=int)),
        }
