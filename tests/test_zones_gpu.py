"""The GPU form of the zone label maps (k_zones, sdsm_zones.hip) against the host definitions of superdsm_amd/zones.py, map by map with
``np.array_equal`` and the dtype, on the smallest maps at which the kernel can still go wrong: places on the rim of the disk and in its
widest row, nearest places across every kind of tile seam with the largest halo, runs of equal labels that cross tile seams and the
halo, images smaller than a tile and than the reach, ties on tile seams, the ends of the label range, all zone kinds into dirty buffers,
sets.  The kernel's tile is 32 rows x 64 columns (ZTH x ZTW of sdsm_zones.hip); its halo classes end at a reach of 4, 16 and 64 pixels."""
import numpy as np
import pytest

from test_measure_cpu import label_scene
from test_zones_cpu import tie_maps

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 32, 64


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    return torch.device('cuda', 0)


def same(got, want, what=''):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype == np.int32 and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)
            raise AssertionError(f'{what}: map {k}: {len(at)} pixels differ, the first at {tuple(at[0])}: {g[tuple(at[0])]} (GPU) != {w[tuple(at[0])]} (host)')


def check_nearest(maps, max_d2):
    """(d2, other) of every map of a list, in one call, against nearest_other_host; returns the host maps."""
    from superdsm_amd import zones
    got = zones.nearest_other_many(maps, max_d2)
    want = [zones.nearest_other_host(m, max_d2) for m in maps]
    assert len(got) == len(maps)
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, f'image {i}, max_d2 {max_d2}')
    return want


def check_zones(maps, zs):
    from superdsm_amd import zones
    got = zones.zone_maps_many(maps, zs)
    want = [zones.zone_maps_host(m, zs) for m in maps]
    assert len(got) == len(maps)
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, f'image {i}, zones {zs}')
    return want


# 1 ---------------------------------------------------------------------------------------------------------------------------------
OFFSETS = ((3, 4), (0, 64), (64, 0), (45, 45), (45, 46))     # d2 = 25, 4096, 4096, 4050 and 4141: the rim, the widest row, just outside


def two_pixels(dr, dc, flip):
    m = np.zeros((26 + dr, 36 + dc), np.int32)
    m[20, 30], m[20 + dr, 30 + dc] = 1, 2                    # (20, 30) and its partner lie in different tiles for all but (3, 4)
    return m[:, ::-1] if flip else m


@pytest.mark.parametrize('max_d2,seen', [(24, [0] * 5), (25, [1, 0, 0, 0, 0]), (4095, [1, 0, 0, 1, 0]), (4096, [1, 1, 1, 1, 0])])
def test_the_threshold(gpu, max_d2, seen):
    """Two single-pixel labels, each map and its mirror image: both labelled pixels face the background at d2 = 1, and every background
    pixel between and around them gets the nearer label, or nothing (every pixel of every map is compared).  The same maps without
    label 1: its place sees label 2 iff their squared distance is <= max_d2."""
    pairs = [two_pixels(dr, dc, flip) for dr, dc in OFFSETS for flip in (False, True)]
    alone = [np.where(m == 1, 0, m) for m in pairs[::2]]
    want = check_nearest(pairs + alone, max_d2)
    for m, (d2, other) in zip(pairs, want):
        first, second = tuple(np.argwhere(m == 1)[0]), tuple(np.argwhere(m == 2)[0])
        assert (int(d2[first]), int(other[first])) == (int(d2[second]), int(other[second])) == (1, 0)
    for (dr, dc), sees, (d2, other) in zip(OFFSETS, seen, want[len(pairs):]):
        assert (int(d2[20, 30]), int(other[20, 30])) == ((dr * dr + dc * dc, 2) if sees else (0, 0)), (dr, dc, max_d2)


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def lattice(shape, r_off, c_off, pitch=37):
    m = np.zeros(shape, np.int32)
    rr, cc = np.meshgrid(np.arange(r_off, shape[0], pitch), np.arange(c_off, shape[1], pitch), indexing='ij')
    m[rr, cc] = 1 + np.arange(rr.size).reshape(rr.shape)
    return m


@pytest.mark.parametrize('shift', [(0, 0), (TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W), (199 - 5 * 37, 299 - 8 * 37)])
def test_seams_with_the_largest_halo(gpu, shift):
    """Single-pixel labels on a lattice of pitch 37 in a 200 x 300 map at max_d2 = 4096: the nearest label of most background pixels lies in
    another tile, across a tile edge or a tile corner, and the halo is 64 pixels.  The shifted lattices put pixels on row and column 0 of
    the image (and of a tile), on the last row (31) and column (63) of a tile, on the first of the next (32, 64), and on the last row
    (199) and column (299) of the image."""
    m = lattice((200, 300), *shift)
    probe = {(0, 0): (0, 0), (31, 63): (31, 63), (32, 64): (32, 64)}.get(shift, (199, 299))
    assert m[probe]
    (d2, other), = check_nearest([m], 4096)
    assert (other[m == 0] > 0).mean() > 0.9 and (other[m > 0] == 0).all() and (d2[m > 0] == 1).all()
    assert (other[40:150, 70:250][m[40:150, 70:250] == 0] > 0).all() and d2[40:150, 70:250].max() <= 2 * 18 * 18     # between lattice places


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def bars(vertical):
    """Label 1 as a bar 3 pixels wide and 150 long across the tile seams, label 2 as a block two pixels beside it along a part of it."""
    m = np.zeros((160, 80), np.int32)
    m[5:155, 62:65] = 1                                      # columns 62 .. 64: over the seam between the tile columns 0 and 1, rows over 5 tile rows
    m[40:100, 67:75] = 2
    m[120:130, 65:70] = 3                                    # touches the bar
    return m if vertical else m.T.copy()


def test_runs_across_seams(gpu):
    from superdsm_amd import zones
    Z = zones.Zone
    maps = [bars(True), bars(False)]
    for zs in ([Z.core(4), Z.rim(4)], [Z.core(1), Z.rim(1), Z.core(4), Z.rim(4), Z.ring(0, 400), Z.grown(30)]):       # halo classes 4 and 64
        want = check_zones(maps, zs)
        for m, w in zip(maps, want):
            assert np.array_equal(w[0] + w[1], m)
    assert not want[0][2][:, 62:65].any() and (want[0][0][:, 63] == 1).sum() == 148       # the bar's core at 4 is empty, at 1 its middle column without the ends
    check_nearest(maps, 4096)                                # runs of 150 equal labels and of background against the cap at reach + 1
    check_nearest(maps, 150)


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_images_smaller_than_a_tile_and_than_the_reach(gpu):
    from superdsm_amd import zones
    Z = zones.Zone
    rng = np.random.default_rng(31)
    maps = [np.array([[4]]), np.array([[0]]), rng.integers(0, 4, (1, 7)), rng.integers(0, 4, (7, 1)), rng.integers(0, 3, (5, 9)),
            np.zeros((5, 9), np.int32), np.full((5, 9), 6, np.uint16), np.zeros((0, 5), np.int32), np.zeros((3, 0), np.int64)]
    for max_d2 in (1, 17, 4096):
        want = check_nearest(maps, max_d2)
        assert not want[5][0].any() and not want[5][1].any()                 # all background: nothing is found
        assert not want[6][1].any() and (want[6][0][0] == 1).all()           # all one label: only the frame
        assert want[7][0].shape == (0, 5) and want[8][1].shape == (3, 0)
    assert want[6][0][2, 4] == 9 and want[0][0][0, 0] == 1
    zs = [Z.grown(4096), Z.ring(1, 4096), Z.core(4), Z.rim(4)]
    want = check_zones(maps, zs)
    assert [w.shape for w in want[7]] == [(0, 5)] * 4 and want[6][2][2, 4] == 6 and not want[5][0].any()
    same(zones.zone_maps(maps[7], zs), want[7])              # an image without pixels alone: no launch
    same(zones.nearest_other(maps[8], 9), (np.zeros((3, 0), np.int32),) * 2)


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_ties_on_tile_seams(gpu):
    """The cases of the CPU test with the pixel in question on the last row and column of a tile and on the first of the next; the
    cases with the frame on a seam between tile columns and between tile rows."""
    maps, expect = [], []
    for m, (r, c), want in tie_maps():
        if want[1] == 0:
            continue                                         # (the frame cannot be moved: below)
        for corner in ((TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W)):
            big = np.zeros((48, 90), np.int32)
            big[corner[0] - r:corner[0] - r + m.shape[0], corner[1] - c:corner[1] - c + m.shape[1]] = m
            maps.append(big)
            expect.append((corner, want))
    wide = np.full((7, 70), 2, np.int32)
    wide[:, 66:] = 5                                         # pixel (2, 63): three places from the frame above and from label 5 in the next tile
    maps += [wide, wide.T.copy()]
    expect += [((2, 63), (9, 0)), ((63, 2), (9, 0))]
    for max_d2 in (16, 400):                                 # the halo classes 4 and 64
        for (at, want), (d2, other) in zip(expect, check_nearest(maps, max_d2)):
            assert (int(d2[at]), int(other[at])) == want


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_label_range(gpu):
    from superdsm_amd import zones
    Z = zones.Zone
    m = np.zeros((5, 70), np.int64)
    m[:, 10:40], m[:, 40:66], m[4, 69] = 1, 65535, 65534
    (d2, other), = check_nearest([m], 25)
    assert other[2, 39] == 65535 and other[2, 40] == 1 and other[3, 66] == 65535 and other[4, 68] == 65534 and d2[2, 39] == 1
    check_zones([m.astype(np.uint16), m], [Z.grown(25), Z.rim(1)])
    ok = np.array([[1, 2, 0, 3]] * 3)
    for v in (70000, -1, 65536, -2 ** 31, 2 ** 31 - 1):
        bad = ok.copy().astype(np.int64)
        bad[1, 2] = bad[2, 3] = v
        with pytest.raises(ValueError, match=r'2 pixels of images \[1\] carry a label outside'):
            zones.nearest_other_many([ok, bad, ok], 2)
        with pytest.raises(ValueError, match=r'pixels of images \[0\]'):
            zones.zone_maps(bad, [Z.rim(1)])
    check_nearest([ok, ok], 2)                               # the other images of that list, in a later call
    with pytest.raises(ValueError, match='labels'):
        zones.nearest_other(np.array([[0, 2 ** 31]]), 2)


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_all_zone_kinds_into_dirty_buffers(gpu):
    """sdsm_zones through the C ABI, 8 zones of all four kinds in one launch, into buffers filled with garbage: every pixel of every map is
    written, and the same call twice gives the same bytes."""
    import torch
    from superdsm_amd import _capi, zones
    from superdsm_amd.render import _DeviceSet
    Z = zones.Zone
    labels = label_scene(np.random.default_rng(71), (70, 150), 25)
    zs = [Z.grown(100), Z.ring(0, 100), Z.ring(0, 9), Z.ring(9, 100), Z.core(4), Z.rim(4), Z.core(1), Z.grown(1)]
    max_d2 = zones.zones_reach(zs)
    assert max_d2 == 100
    want_n, want_z = zones.nearest_other_host(labels, max_d2), zones.zone_maps_host(labels, zs)
    H, W = labels.shape
    S = _DeviceSet([labels.shape])
    d_map = S.pack([labels], np.int32)
    specs = np.array([z.spec() for z in zs], np.int32).view(_capi.ZONE_SPEC_DTYPE)
    for garbage in (-1, 0x5a5a5a5a, -1):
        d_d2, d_other = (torch.empty(H * W, dtype=torch.int32, device=S.dev).fill_(garbage) for _ in range(2))
        d_zone = torch.empty(len(zs) * H * W, dtype=torch.int32, device=S.dev).fill_(garbage)
        d_status = torch.empty(1, dtype=torch.int32, device=S.dev).fill_(garbage)
        _capi.check(S.L.sdsm_zones(H, W, S._p(d_map), max_d2, len(zs), specs.ctypes.data_as(S.C.c_void_p), S._p(d_d2), S._p(d_other), S._p(d_zone),
                                   S._p(d_status), S._stream()), 'sdsm_zones')
        assert d_status.cpu().numpy().tolist() == [0]
        same((d_d2.cpu().numpy().reshape(H, W), d_other.cpu().numpy().reshape(H, W)), want_n, 'nearest other')
        same(list(d_zone.cpu().numpy().reshape(len(zs), H, W)), want_z, 'zones')
    # the maps of the nearest-other transform are optional, and so are the zones
    d_zone.fill_(-1)
    _capi.check(S.L.sdsm_zones(H, W, S._p(d_map), max_d2, len(zs), specs.ctypes.data_as(S.C.c_void_p), None, None, S._p(d_zone), S._p(d_status),
                               S._stream()), 'sdsm_zones')
    same(list(d_zone.cpu().numpy().reshape(len(zs), H, W)), want_z, 'zones alone')
    g, r0, r1, r01, c, m = want_z[:6]
    assert np.array_equal(g, labels + r0) and np.array_equal(labels, c + m) and np.array_equal(r1 + r01, r0) and r01.any() and c.any()


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_sets_equal_single_images_and_long_lists_are_split(gpu):
    from superdsm_amd import zones
    Z = zones.Zone
    rng = np.random.default_rng(72)
    maps = [label_scene(rng, (37, 53), 9), label_scene(rng, (90, 120), 14).astype(np.uint16), label_scene(rng, (33, 129), 16).astype(np.int64),
            label_scene(rng, (65, 64), 9)]
    wide = np.zeros((37, 60), np.int64)                      # a view with unaligned rows, one column short of the first map
    wide[:, 3:56] = maps[0]
    maps.append(wide[:, 3:55])
    assert len(set(m.shape for m in maps)) == 5
    zs = [Z.grown(30), Z.core(2)]
    many_n, many_z = zones.nearest_other_many(maps, 30), zones.zone_maps_many(maps, zs)
    for m, n, z in zip(maps, many_n, many_z):
        same(n, zones.nearest_other_host(m, 30))
        same(z, zones.zone_maps_host(m, zs))
        same(zones.nearest_other(m, 30), n)
        same(zones.zone_maps(m, zs), z)
    tiny = [rng.integers(0, 4, (3, 3)) for _ in range(33)]
    check_nearest(tiny, 10)
    check_zones(tiny, [Z.ring(0, 2), Z.rim(1)])


# 9 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_d2', [1, 2, 16, 17, 256, 257])
def test_random_scenes(gpu, max_d2):
    """Every halo class at both of its ends: a reach of 1 and 4, of 4 (17 has the root 4) and 16, of 16 (257) and more."""
    rng = np.random.default_rng(8)
    maps = [label_scene(rng) for _ in range(2)] + [label_scene(rng, (61, 47), 25), label_scene(rng, (130, 200), 40)]
    want = check_nearest(maps, max_d2)
    assert all((other[m == 0] > 0).any() and (other[m > 0] > 0).any() for m, (_, other) in zip(maps, want))


# 10 --------------------------------------------------------------------------------------------------------------------------------
def test_result_of_objects(gpu):
    from superdsm_amd import render, testing, zones
    Z = zones.Zone
    objs = [testing.PostFragment((1, 1), np.ones((9, 12), bool)), testing.PostFragment((4, 16), np.ones((3, 3), bool))]
    data = {'g_raw': np.random.default_rng(71).random((20, 25)), 'postprocessed_objects': objs}
    labels = render.rasterize_labels(data)
    assert labels.max() == 2
    zs = [Z.ring(0, 25), Z.core(4), Z.grown(9)]
    want = zones.zone_maps_host(labels, zs)
    same(zones.zones_result(data, zones=zs), want)
    same(zones.zones_result(data, objects=objs, zones=zs), want)
    for got in zones.zones_results([data, data], zones=zs):
        same(got, want)
    assert (want[0] == 1).any() and (want[0] == 2).any() and want[1].any()


def test_the_maps_go_into_the_tables_as_they_come(gpu):
    from superdsm_amd import intensity, zones
    rng = np.random.default_rng(73)
    labels = label_scene(rng, (70, 90), 10)
    g = rng.normal(size=labels.shape)
    ring_gpu, ring_host = zones.zone_maps(labels, [zones.Zone.ring(0, 25)])[0], zones.zone_maps_host(labels, [zones.Zone.ring(0, 25)])[0]
    table, order = intensity.intensity_labels(ring_gpu, g)
    want_t, want_o = intensity.intensity_labels_host(ring_host, g)
    assert table.dtype == want_t.dtype and table.tobytes() == want_t.tobytes() and order.dtype == want_o.dtype and order.tobytes() == want_o.tobytes()
    assert len(table) >= 8 and (table['area'] > 0).all()
