"""New label maps out of one label map: the labels grown into the background (a cell approximation around each nucleus), the band
around each label (the "cytoplasm ring"), the core of a label without its rim, and the rim alone.  ``measure``, ``shape``,
``intensity``, ``texture``, ``neighbours`` and ``depth`` each have a ``*_labels`` form that takes any label map, so with the maps of
this module they become compartment tables with no change of their own: ``intensity.intensity_labels(ring_map, g)`` is the perinuclear
intensity.  Label maps only: objects come in through ``render.rasterize_labels_many``, which makes them disjoint.

Everything is defined in integers, so that the GPU form (``k_zones``, sdsm_zones.hip) gives the bytes of the host definitions
:func:`nearest_other_host` and :func:`zone_maps_host` whatever the launch or the set size:

* A label map L is a two-dimensional integer image with the labels 0 .. 65535, 0 the background, and H^2 + W^2 < 2^31
  (``boundary.check_shape``).  It is extended by label 0 everywhere outside the image frame.
* **Nearest other**, ``nearest_other(labels, max_d2)`` with 1 <= ``max_d2`` <= ``MAX_D2`` = 4096 (a reach of 64 pixels;
  ``neighbours.reach_d2`` turns a distance into ``max_d2``).  For a pixel p look at all lattice places q, inside or outside the image,
  with 0 < |p - q|^2 <= ``max_d2`` and L(q) != L(p).  If there is none, ``d2(p)`` = 0 and ``other(p)`` = 0.  Otherwise the q with the
  smallest key (|p - q|^2, L(q)) -- of several places at the smallest distance the smallest label wins -- gives ``d2(p)``, that squared
  distance, and ``other(p)``, that label.
* So for a **background pixel** ``other`` is the nearest label >= 1 and ``d2`` its squared distance; the frame never counts, because it
  is label 0 too.  For a **pixel of a label l >= 1** ``d2`` is its squared depth in the convention of ``depth`` -- other labels, the
  background and the outside of the image are all outside the object -- and ``other`` says what it faces: 0 for background or frame,
  else the touching or closest label.
* **Zones.**  A zone turns (L, d2, other) into one label map; write d2' for ``d2``, or +infinity where nothing was found:

  ==================  ====================  =============================================  =================
  zone                a pixel gets          if (otherwise 0)                               constraint
  ==================  ====================  =============================================  =================
  ``grown(hi)``       L(p), or other(p)     L(p) >= 1; or L(p) == 0 and 1 <= d2 <= hi
  ``ring(lo, hi)``    other(p)              L(p) == 0 and lo < d2 <= hi                    0 <= lo < hi
  ``core(lo)``        L(p)                  L(p) >= 1 and d2' > lo                         lo >= 1
  ``rim(hi)``         L(p)                  L(p) >= 1 and 1 <= d2 <= hi
  ==================  ====================  =============================================  =================

  All bounds are squared distances, integers, >= 0 (``hi`` >= 1) and <= ``MAX_D2``.  The reach of a launch is the largest bound of its
  zones: a pixel without a place within that reach has none within any smaller bound, and its depth exceeds every ``lo``.
* By construction, with + the union of disjoint supports: ``grown(hi)`` = labels + ``ring(0, hi)``; labels = ``core(x)`` + ``rim(x)``;
  ``ring(0, a)`` + ``ring(a, b)`` = ``ring(0, b)``.

The host definition compares the zero-padded map with its shift for every offset of the full disk.  The kernel is separable instead:
per column the nearest place with another label is the place in the pixel's row, or an end of the run of equal labels through it (see
sdsm_zones.hip); the GPU tests pin it against the host definition.

Parity with scikit-image's ``expand_labels`` and CellProfiler's "Distance-N" secondary objects is UNPINNED (neither was available to
compare with); by its documentation ``expand_labels`` differs from ``grown`` only in which of several equidistant labels wins."""
import math

import numpy as np

from . import _capi
from .boundary import check_shape
from .imageset import in_sets
from .neighbours import check_max_d2

MAX_D2 = _capi.ZONE_MAX_D2
MAX_ZONES = _capi.ZONE_MAX_ZONES
MAX_LABELS = _capi.BOUNDARY_MAX_LABELS
assert MAX_D2 == _capi.NEIGHBOUR_MAX_D2                     # (check_max_d2 is the one of the neighbourhood tables)


# ---- the definitions ------------------------------------------------------------------------------------------------------------------
def _bound(value, what, least):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise TypeError(f'{what}: an integer squared distance (see neighbours.reach_d2); got {type(value).__name__}')
    if not least <= int(value) <= MAX_D2:
        raise ValueError(f'{what} {int(value)}: {least} <= {what} <= {MAX_D2} required (a reach of 64 pixels), see DESIGN.md "Limits"')
    return int(value)


class Zone:
    """One rule that turns (L, d2, other) into a label map; made by :meth:`grown`, :meth:`ring`, :meth:`core` or :meth:`rim`.  ``kind``
    is the constructor's name, ``lo`` and ``hi`` the bounds (squared distances; None where the kind has none)."""
    __slots__ = ('kind', 'lo', 'hi')

    def __init__(self, kind, lo, hi):
        self.kind, self.lo, self.hi = kind, lo, hi

    @classmethod
    def grown(cls, hi):
        """Every label keeps its pixels and takes the background pixels within ``hi`` that it is nearest to."""
        return cls('grown', None, _bound(hi, 'hi', 1))

    @classmethod
    def ring(cls, lo, hi):
        """The background pixels with ``lo`` < d2 <= ``hi``, each with the label it is nearest to."""
        lo, hi = _bound(lo, 'lo', 0), _bound(hi, 'hi', 1)
        if lo >= hi:
            raise ValueError(f'ring({lo}, {hi}): lo < hi required')
        return cls('ring', lo, hi)

    @classmethod
    def core(cls, lo):
        """The pixels of every label that lie deeper than ``lo``: d2 > ``lo``."""
        return cls('core', _bound(lo, 'lo', 1), None)

    @classmethod
    def rim(cls, hi):
        """The pixels of every label with d2 <= ``hi``."""
        return cls('rim', None, _bound(hi, 'hi', 1))

    @property
    def reach(self):
        """The largest bound: the ``max_d2`` this zone needs."""
        return max(v for v in (self.lo, self.hi, 1) if v is not None)

    def spec(self):
        """The zone as (side, keep_own, lo_d2, hi_d2) of ``sdsm_zone_spec``."""
        if self.kind in ('grown', 'ring'):
            return (_capi.ZONE_SIDE_BACKGROUND, int(self.kind == 'grown'), self.lo or 0, self.hi)
        return (_capi.ZONE_SIDE_OBJECT, 0, self.lo or 0, _capi.ZONE_NO_UPPER if self.hi is None else self.hi)

    def __eq__(self, other):
        return isinstance(other, Zone) and (self.kind, self.lo, self.hi) == (other.kind, other.lo, other.hi)

    def __hash__(self):
        return hash((self.kind, self.lo, self.hi))

    def __repr__(self):
        return f'Zone.{self.kind}({", ".join(str(v) for v in (self.lo, self.hi) if v is not None)})'


grown, ring, core, rim = Zone.grown, Zone.ring, Zone.core, Zone.rim


def check_zones(zones):
    """``zones`` as a list of :class:`Zone`: ``TypeError`` for anything else in it, ``ValueError`` for more than ``MAX_ZONES``."""
    zones = [zones] if isinstance(zones, Zone) else list(zones)
    for z in zones:
        if not isinstance(z, Zone):
            raise TypeError(f'zones: Zone.grown / ring / core / rim; got {type(z).__name__}')
    if len(zones) > MAX_ZONES:
        raise ValueError(f'{len(zones)} zones: a call takes at most {MAX_ZONES}, see DESIGN.md "Limits"')
    return zones


def zones_reach(zones):
    """``max_d2`` of a launch for ``zones``: the largest bound of them (1 without zones)."""
    return max([z.reach for z in zones], default=1)


def _check_map(labels, what='labels'):
    check_shape(np.shape(labels), what)                      # (the shape alone decides first)
    labels = np.asarray(labels)
    if labels.dtype.kind not in 'iu':
        raise TypeError(f'{what}: an integer image; got {labels.dtype}')
    if labels.size and (int(labels.min()) < 0 or int(labels.max()) >= MAX_LABELS):
        raise ValueError(f'{what}: labels {int(labels.min())} .. {int(labels.max())}; the zone maps take the labels 0 .. {MAX_LABELS - 1}, '
                         'see DESIGN.md "Limits"')
    return labels


def disk_offsets(max_d2):
    """The offsets (d_row, d_col) with 0 < d_row^2 + d_col^2 <= ``max_d2``, row by row (n x 2, int64): the full disk without its centre."""
    max_d2 = check_max_d2(max_d2)
    out = []
    for dr in range(-math.isqrt(max_d2), math.isqrt(max_d2) + 1):
        w = math.isqrt(max_d2 - dr * dr)
        out += [(dr, dc) for dc in range(-w, w + 1) if dr or dc]
    return np.array(out, np.int64).reshape(-1, 2)


def nearest_other_host(labels, max_d2):
    """``(d2, other)`` of a label map as int32 maps, the plain statement of the module's docstring: for every offset of the full disk the
    map, padded with zeros by the reach, is compared with its shift, and the key ``d2 << 16 | label`` of the places that differ is
    reduced with min."""
    labels, max_d2 = _check_map(labels).astype(np.uint32), check_max_d2(max_d2)
    H, W = labels.shape
    R = math.isqrt(max_d2)
    none = np.uint32(0xffffffff)                             # (above every key: MAX_D2 << 16 | 65535 < 2^29)
    best = np.full((H, W), none, np.uint32)
    if labels.size:
        padded = np.pad(labels, R)
        key, same = np.empty((H, W), np.uint32), np.empty((H, W), bool)
        for dr, dc in disk_offsets(max_d2).tolist():
            q = padded[R + dr:R + dr + H, R + dc:R + dc + W]
            np.bitwise_or(q, np.uint32((dr * dr + dc * dc) << 16), out=key)
            np.equal(q, labels, out=same)
            np.copyto(key, none, where=same)
            np.minimum(best, key, out=best)
    found = best != none
    return np.where(found, best >> 16, 0).astype(np.int32), np.where(found, best & 0xffff, 0).astype(np.int32)


def _zone_map(zone, labels, d2, other):
    """One zone's int32 map from (L, d2, other), by the table of the module's docstring; d2 == 0 is "nothing found"."""
    fg, found = labels >= 1, d2 >= 1
    if zone.kind in ('grown', 'ring'):
        band = ~fg & found & (d2 > (zone.lo or 0)) & (d2 <= zone.hi)
        out = np.where(band, other, 0)
        return np.where(fg, labels, out).astype(np.int32) if zone.kind == 'grown' else out.astype(np.int32)
    if zone.kind == 'core':
        return np.where(fg & (~found | (d2 > zone.lo)), labels, 0).astype(np.int32)
    return np.where(fg & found & (d2 <= zone.hi), labels, 0).astype(np.int32)


def zone_maps_host(labels, zones):
    """The int32 maps of ``zones`` (in their order) of a label map, from :func:`nearest_other_host` at the reach of the zones."""
    zones = check_zones(zones)
    labels = _check_map(labels)
    d2, other = nearest_other_host(labels, zones_reach(zones))
    return [_zone_map(z, labels.astype(np.int64), d2, other) for z in zones]


# ---- the GPU form (k_zones, sdsm_zones.hip) ---------------------------------------------------------------------------------------------
def _as_int32(labels, what):
    """The map as int32 for the upload.  The shape is checked first; a label outside 0 .. 65535 is left to the device, which counts it,
    unless int32 cannot hold it."""
    check_shape(np.shape(labels), what)
    labels = np.asarray(labels)
    if labels.dtype.kind not in 'iu':
        raise TypeError(f'{what}: an integer image; got {labels.dtype}')
    if labels.dtype.itemsize > 4 or labels.dtype == np.uint32:
        if labels.size and (int(labels.min()) < -2 ** 31 or int(labels.max()) >= 2 ** 31):
            raise ValueError(f'{what}: labels {int(labels.min())} .. {int(labels.max())}; the zone maps take the labels 0 .. {MAX_LABELS - 1}, '
                             'see DESIGN.md "Limits"')
    return labels.astype(np.int32)


def _launch_set(l32, max_d2, zones, want_nearest, names):
    """One launch for a set of up to ``_capi.MAX_SET_IMAGES`` int32 label maps: per image ``(d2, other, [zone maps])`` (d2 and other None
    unless asked for).  Pixels with a label outside 0 .. 65535 raise ``ValueError`` naming their images."""
    from .render import _DeviceSet
    S = _DeviceSet([x.shape for x in l32])
    t, n, nz = S.torch, len(l32), len(zones)
    d_map = S.pack(l32, np.int32)
    d_d2, d_other = (t.empty(S.total, dtype=t.int32, device=S.dev) for _ in range(2)) if want_nearest else (None, None)
    d_zone = t.empty(nz * S.total, dtype=t.int32, device=S.dev) if nz else None
    d_status = t.empty(n, dtype=t.int32, device=S.dev)
    specs = np.array([z.spec() for z in zones], np.int32).reshape(nz, 4).view(_capi.ZONE_SPEC_DTYPE)
    S.capi.check(S.L.sdsm_zones_multi(S.table, n, S._p(d_map), max_d2, nz, specs.ctypes.data_as(S.C.c_void_p), S.total, S._p(d_d2), S._p(d_other),
                                      S._p(d_zone), S._p(d_status), S._stream()), 'sdsm_zones_multi')
    status = d_status.cpu().numpy()
    bad = np.nonzero(status)[0]
    if len(bad):
        raise ValueError(f'{int(status.sum())} pixels of images {[names[i] for i in bad]} carry a label outside 0 .. {MAX_LABELS - 1}; the zone maps '
                         f'take the labels 0 .. {MAX_LABELS - 1}, see DESIGN.md "Limits"')
    d2, other = (S.unpack(d_d2), S.unpack(d_other)) if want_nearest else ([None] * n, [None] * n)
    flat = d_zone.cpu().numpy() if nz else None
    per_zone = [S.layout.unpack(flat[z * S.total:(z + 1) * S.total]) for z in range(nz)]
    return [(d2[i], other[i], [per_zone[z][i] for z in range(nz)]) for i in range(n)]


def _many(labels_list, max_d2, zones, want_nearest):
    l32 = [_as_int32(l, 'labels') for l in labels_list]
    out = [None] * len(l32)
    full = [i for i, l in enumerate(l32) if l.size]          # (an image without pixels has empty maps and no launch)
    for i in set(range(len(l32))) - set(full):
        empty = lambda: np.zeros(l32[i].shape, np.int32)
        out[i] = ((empty(), empty()) if want_nearest else (None, None)) + ([empty() for _ in zones],)
    for part in in_sets(len(full)):
        idx = full[part]
        for i, res in zip(idx, _launch_set([l32[i] for i in idx], max_d2, zones, want_nearest, idx)):
            out[i] = res
    return out


def nearest_other_many(labels_list, max_d2):
    """``(d2, other)`` per label map of a list, as int32 maps: the bytes of :func:`nearest_other_host`.  One launch per
    ``_capi.MAX_SET_IMAGES`` images (longer lists are split); a pixel with a label outside 0 .. 65535 raises ``ValueError`` naming its
    image."""
    return [(d2, other) for d2, other, _ in _many(list(labels_list), check_max_d2(max_d2), [], True)]


def nearest_other(labels, max_d2):
    """``(d2, other)`` of one label map on the GPU: the bytes of :func:`nearest_other_host`.  The set of this one image."""
    return nearest_other_many([labels], max_d2)[0]


def zone_maps_many(labels_list, zones):
    """Per label map of a list the int32 maps of ``zones``, in their order: the bytes of :func:`zone_maps_host`.  One launch per
    ``_capi.MAX_SET_IMAGES`` images (longer lists are split), at the reach of the zones; a pixel with a label outside 0 .. 65535 raises
    ``ValueError`` naming its image."""
    zones = check_zones(zones)
    return [maps for _, _, maps in _many(list(labels_list), zones_reach(zones), zones, False)]


def zone_maps(labels, zones):
    """The int32 maps of ``zones`` of one label map on the GPU: the bytes of :func:`zone_maps_host`.  The set of this one image."""
    return zone_maps_many([labels], zones)[0]


def zones_results(datas, objects='postprocessed_objects', *, zones, merge_overlap_threshold=np.inf, dilate=0):
    """The zone maps per pipeline data object of a list: the label maps of ``objects`` (an output name, or one list of objects per image)
    by ``render.rasterize_labels_many`` (background 0, objects made disjoint), then :func:`zone_maps_many`."""
    from .render import rasterize_labels_many
    zones = check_zones(zones)
    return zone_maps_many(rasterize_labels_many(datas, objects, merge_overlap_threshold, dilate), zones)


def zones_result(data, objects='postprocessed_objects', *, zones, merge_overlap_threshold=np.inf, dilate=0):
    """:func:`zones_results` for one pipeline data object (``objects``: an output name or a list of objects)."""
    from .render import _objects_of
    return zones_results([data], [_objects_of(data, objects)], zones=zones, merge_overlap_threshold=merge_overlap_threshold, dilate=dilate)[0]
