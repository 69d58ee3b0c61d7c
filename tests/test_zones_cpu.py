"""The host definitions of the zone label maps (superdsm_amd/zones.py) and their argument checks, without a GPU: nearest_other_host
against a per-pixel brute force in Python integers, against SciPy's distance transform on the background and against depth's squared
depth inside an object, the tie rule, the identities between the zones, and the entry of the C ABI."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy import ndimage

from test_measure_cpu import label_scene


def brute_force(labels, max_d2):
    """(d2, other) pixel by pixel in Python integers: every lattice place of the square of the reach, inside or outside the image."""
    labels = np.asarray(labels)
    H, W = labels.shape
    R = math.isqrt(max_d2)
    at = lambda r, c: int(labels[r, c]) if 0 <= r < H and 0 <= c < W else 0
    d2, other = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    for r in range(H):
        for c in range(W):
            keys = [(dr * dr + dc * dc, at(r + dr, c + dc)) for dr in range(-R, R + 1) for dc in range(-R, R + 1)
                    if 0 < dr * dr + dc * dc <= max_d2 and at(r + dr, c + dc) != at(r, c)]
            if keys:
                d2[r, c], other[r, c] = min(keys)
    return d2, other


def same(got, want):
    return all(g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == len(want)


def small_maps():
    rng = np.random.default_rng(41)
    maps = [np.where(rng.random((12, 12)) < 0.3, rng.integers(1, 4, (12, 12)), 0), np.where(rng.random((7, 12)) < 0.8, rng.integers(1, 3, (7, 12)), 0),
            np.kron(rng.integers(0, 4, (4, 3)), np.ones((3, 4), np.int64)), np.zeros((5, 6), np.int64), np.full((6, 5), 9, np.uint16),
            np.array([[65535]]), rng.integers(0, 3, (1, 11)), rng.integers(0, 3, (11, 1)), np.zeros((0, 5), np.int32)]
    maps[0][3, 4] = 65535
    return maps


@pytest.mark.parametrize('max_d2', [1, 2, 4, 5, 8, 9, 400])
def test_nearest_other_host_equals_the_brute_force(max_d2):
    from superdsm_amd import zones
    for m in small_maps():
        assert same(zones.nearest_other_host(m, max_d2), brute_force(m, max_d2)), (max_d2, m)
    d2, other = zones.nearest_other_host(np.zeros((5, 6), np.int64), max_d2)
    assert not d2.any() and not other.any()                  # all background: the frame is background too
    d2, other = zones.nearest_other_host(np.full((6, 5), 9), max_d2)
    assert not other.any() and (d2[0] == 1).all() and d2[2, 2] == (9 if max_d2 >= 9 else 0)


def test_background_pixels_equal_scipys_distance_transform():
    from superdsm_amd import zones
    labels = label_scene(np.random.default_rng(42), (60, 80), 9)
    sq = ndimage.distance_transform_edt(labels == 0) ** 2
    want = np.rint(sq).astype(np.int64)
    assert np.abs(sq - want).max() < 1e-6
    for max_d2 in (1, 10, 169):
        d2, other = zones.nearest_other_host(labels, max_d2)
        bg, near = labels == 0, want <= max_d2
        assert (bg & near).sum() > 20 and np.array_equal(d2[bg & near], want[bg & near])
        assert not d2[bg & ~near].any() and not other[bg & ~near].any() and (other[bg & near] >= 1).all()


def test_object_pixels_equal_the_squared_depth():
    from superdsm_amd import depth, zones
    yy, xx = np.mgrid[0:40, 0:50]
    labels = (((yy - 14) / 15.0) ** 2 + ((xx - 20) / 22.0) ** 2 <= 1).astype(np.int32) * 3      # one object that touches the frame at the top and the left
    assert labels[0].any() and labels[:, 0].any() and not labels[-1].any()
    want = depth.squared_depth(labels > 0)
    for max_d2 in (1, 20, 144):
        d2, other = zones.nearest_other_host(labels, max_d2)
        fg, near = labels > 0, want <= max_d2
        assert (fg & near).sum() > 20 and np.array_equal(d2[fg & near], want[fg & near])
        assert not d2[fg & ~near].any() and not other[fg].any()
    assert want.max() > 144                                  # (so the last reach leaves deep pixels without a place)


def tie_maps():
    """(map, pixel, (d2, other) at that pixel): a background pixel midway between the labels 7 and 3 gets 3, in a row, in a column and
    diagonally, whichever side the 3 is on; a labelled pixel as far from label 5 as from the frame gets 0."""
    out = []
    for a, b in ((7, 3), (3, 7)):
        m = np.zeros((9, 9), np.int32)
        m[4, 1], m[4, 7] = a, b
        out.append((m, (4, 4), (9, 3)))
        out.append((m.T.copy(), (4, 4), (9, 3)))
        m = np.zeros((9, 9), np.int32)
        m[2, 2], m[6, 6] = a, b
        out.append((m, (4, 4), (8, 3)))
        out.append((m[:, ::-1].copy(), (4, 4), (8, 3)))
        m = np.zeros((9, 9), np.int32)
        m[2, 4], m[4, 6] = a, b                              # one above, one to the right: the column's run end against the row's place
        out.append((m, (4, 4), (4, 3)))
    m = np.full((7, 9), 2, np.int32)
    m[:, 5:] = 5                                             # pixel (2, 2) of label 2: three places from the frame above and from label 5
    out.append((m, (2, 2), (9, 0)))
    out.append((m.T.copy(), (2, 2), (9, 0)))
    return out


def test_the_tie_rule():
    from superdsm_amd import zones
    for m, (r, c), want in tie_maps():
        d2, other = zones.nearest_other_host(m, 16)
        assert (int(d2[r, c]), int(other[r, c])) == want, (m, want)
        assert same((d2, other), brute_force(m, 16))


def union(a, b):
    assert not ((a != 0) & (b != 0)).any(), 'the supports are disjoint'
    return a + b


def test_the_identities():
    from superdsm_amd import zones
    Z = zones.Zone
    labels = label_scene(np.random.default_rng(43))
    g, r0, r1, r01, c, m = zones.zone_maps_host(labels, [Z.grown(40), Z.ring(0, 40), Z.ring(0, 9), Z.ring(9, 40), Z.core(4), Z.rim(4)])
    assert all(x.dtype == np.int32 for x in (g, r0, r1, r01, c, m))
    assert np.array_equal(g, union(labels, r0)) and np.array_equal(labels, union(c, m)) and np.array_equal(union(r1, r01), r0)
    assert r1.any() and r01.any() and c.any() and m.any() and (r0 != 0).sum() > (r1 != 0).sum()
    d2, other = zones.nearest_other_host(labels, 40)
    assert np.array_equal(r0 != 0, (labels == 0) & (d2 >= 1)) and np.array_equal(m != 0, (labels > 0) & (d2 >= 1) & (d2 <= 4))
    # the reach of the zones is their largest bound, and a larger reach changes nothing
    assert same(zones.zone_maps_host(labels, [Z.core(4), Z.rim(4), Z.ring(0, 9)]), [c, m, r1])
    assert zones.zones_reach([Z.core(4), Z.ring(2, 3)]) == 4 and zones.zones_reach([Z.rim(7)]) == 7 and zones.zones_reach([]) == 1


def test_argument_checks():
    from fractions import Fraction
    from superdsm_amd import neighbours, zones
    Z = zones.Zone
    ok = np.array([[0, 1], [2, 0]])
    for make in (lambda: Z.grown(4.0), lambda: Z.ring(0, 9.0), lambda: Z.ring(1.0, 9), lambda: Z.core(2.5), lambda: Z.rim(np.float64(4)), lambda: Z.rim(True)):
        with pytest.raises(TypeError):
            make()
    for make in (lambda: Z.ring(9, 9), lambda: Z.ring(10, 9), lambda: Z.ring(-1, 9), lambda: Z.grown(4097), lambda: Z.ring(0, 4097), lambda: Z.core(4097),
                 lambda: Z.rim(4097), lambda: Z.core(0), lambda: Z.rim(0), lambda: Z.grown(0)):
        with pytest.raises(ValueError):
            make()
    assert Z.grown(4096).hi == 4096 and Z.ring(0, neighbours.reach_d2(Fraction(7, 2))) == Z.ring(0, 12) and repr(Z.ring(1, 5)) == 'Zone.ring(1, 5)'
    with pytest.raises(ValueError, match='at most 8'):
        zones.check_zones([Z.rim(1)] * 9)
    assert len(zones.check_zones([Z.rim(1)] * 8)) == 8
    with pytest.raises(TypeError):
        zones.check_zones([Z.rim(1), ('ring', 0, 4)])
    with pytest.raises(ValueError, match='at most 8'):
        zones.zone_maps_host(ok, [Z.rim(1)] * 9)
    for v in (65536, -1):
        bad = ok.copy().astype(np.int64)
        bad[1, 1] = v
        with pytest.raises(ValueError, match='labels'):
            zones.nearest_other_host(bad, 4)
        with pytest.raises(ValueError, match='labels'):
            zones.zone_maps_host(bad, [Z.rim(1)])
    with pytest.raises(TypeError):
        zones.nearest_other_host(ok.astype(float), 4)
    with pytest.raises(TypeError):
        zones.nearest_other_host(ok, 4.0)
    for max_d2 in (0, 4097):
        with pytest.raises(ValueError):
            zones.nearest_other_host(ok, max_d2)
    with pytest.raises(ValueError):
        zones.nearest_other_host(np.zeros((2, 2, 2), int), 4)
    assert zones.MAX_D2 == 4096 and zones.MAX_ZONES == 8


def test_the_entry_of_the_c_abi():
    from superdsm_amd import _capi, zones
    assert 'sdsm_zones_multi' in _capi.SYMBOLS and 'sdsm_zones' in _capi.SYMBOLS
    assert _capi.ZONE_SPEC_DTYPE.itemsize == 16 and _capi.ZONE_SPEC_DTYPE.names == ('side', 'keep_own', 'lo_d2', 'hi_d2')
    assert (_capi.ZONE_MAX_D2, _capi.ZONE_MAX_ZONES, _capi.ZONE_NO_UPPER) == (4096, 8, 2 ** 31 - 1)
    Z = zones.Zone
    assert [z.spec() for z in (Z.grown(9), Z.ring(2, 9), Z.core(4), Z.rim(4))] == [(0, 1, 0, 9), (0, 0, 2, 9), (1, 0, 4, 2 ** 31 - 1), (1, 0, 0, 4)]
    lib = _capi.lib()
    table = (_capi.SetImage * 1)()
    table[0].offset, table[0].H, table[0].W = 0, 4, 4
    spec = np.array([(1, 0, 4, 3)], _capi.ZONE_SPEC_DTYPE)
    one = C.c_void_p(16)                                     # (never dereferenced: the arguments are refused first)
    call = lambda max_d2, n_zones: lib.sdsm_zones_multi(table, 1, one, max_d2, n_zones, spec.ctypes.data_as(C.c_void_p), 16, None, None, one, one, None)
    assert call(4097, 1) != 0 and b'max_d2' in lib.sdsm_last_error()
    assert call(9, 9) != 0 and b'n_zones' in lib.sdsm_last_error()
    assert call(9, 1) != 0 and b'lo_d2 < hi_d2' in lib.sdsm_last_error()
    spec[0] = (0, 0, 0, 10)
    assert call(9, 1) != 0 and b'hi_d2 <= max_d2' in lib.sdsm_last_error()
