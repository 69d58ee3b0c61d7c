"""The GPU form of the neighbourhood tables (k_neighbours, sdsm_neighbours.hip) against the host definitions of
superdsm_amd/neighbours.py, byte for byte and field by field, on the smallest maps at which the kernel can still go wrong: pairs on the
rim of the disk and in its widest row, closest pairs across every kind of tile seam with the largest halo, images smaller than a tile and
than the reach, the ends of the label range, crack edges at tile seams, more pairs in a tile than its LDS table holds, growing tables,
dirty buffers, sets.  The kernel's tile is 32 rows x 64 columns (NTH x NTW of sdsm_neighbours.hip); its halo classes end at a reach of 4,
16 and 64 pixels."""
import numpy as np
import pytest

from test_measure_cpu import ellipse, label_scene

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 32, 64


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    return torch.device('cuda', 0)


def check(got, labels, max_d2, n_labels=None):
    """One image's (table, pairs) against the host definitions: dtypes, lengths, then every field, then the bytes."""
    from superdsm_amd import neighbours
    table, pairs = got
    want_t, want_p = neighbours.neighbour_labels_host(labels, max_d2, n_labels), neighbours.neighbour_pairs_host(labels, max_d2)
    assert table.dtype == neighbours.LABEL_DTYPE and pairs.dtype == neighbours.PAIR_DTYPE
    assert len(table) == len(want_t) and [tuple(p) for p in pairs[['a', 'b']].tolist()] == [tuple(p) for p in want_p[['a', 'b']].tolist()]
    for name in neighbours.PAIR_DTYPE.names:
        assert np.array_equal(pairs[name], want_p[name]), (name, pairs[pairs[name] != want_p[name]][:5], want_p[pairs[name] != want_p[name]][:5])
    for name in neighbours.LABEL_DTYPE.names:
        differ = np.nonzero(table[name] != want_t[name])[0]
        assert not len(differ), (name, differ[:5], table[name][differ[:5]], want_t[name][differ[:5]])
    assert table.tobytes() == want_t.tobytes() and pairs.tobytes() == want_p.tobytes()
    return want_t, want_p


def check_many(maps, max_d2, **kw):
    from superdsm_amd import neighbours
    got = neighbours.neighbour_tables_many(maps, max_d2, **kw)
    assert len(got) == len(maps)
    return [check(g, m, max_d2, kw.get('n_labels')) for g, m in zip(got, maps)]


# 1 ---------------------------------------------------------------------------------------------------------------------------------
OFFSETS = ((3, 4), (0, 64), (64, 0), (45, 45), (45, 46))     # d2 = 25, 4096, 4096, 4050 and 4141: the rim, the widest row, just outside


def two_pixels(dr, dc, flip):
    m = np.zeros((90, 100), np.int32)
    m[20, 30], m[20 + dr, 30 + dc] = 1, 2                    # (20, 30) and its partner lie in different tiles for all but (3, 4)
    return m[:, ::-1] if flip else m


def test_the_threshold(gpu):
    maps = [two_pixels(dr, dc, flip) for dr, dc in OFFSETS for flip in (False, True)]
    for max_d2, rows in ((24, [0] * 5), (25, [1, 0, 0, 0, 0]), (4095, [1, 0, 0, 1, 0]), (4096, [1, 1, 1, 1, 0])):
        want = check_many(maps, max_d2)
        assert [len(p) for _, p in want] == [n for n in rows for _ in range(2)], max_d2
        assert [int(t['close'].sum()) for t, _ in want] == [2 * n for n in rows for _ in range(2)]
    assert [p['min_d2'].tolist() for _, p in want[::2]] == [[25], [4096], [4096], [4050], []]


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def lattice(shape, r_off, c_off, pitch=37):
    m = np.zeros(shape, np.int32)
    rr, cc = np.meshgrid(np.arange(r_off, shape[0], pitch), np.arange(c_off, shape[1], pitch), indexing='ij')
    m[rr, cc] = 1 + np.arange(rr.size).reshape(rr.shape)
    return m


def test_seams_with_the_largest_halo(gpu):
    """Single-pixel labels on a lattice of pitch 37 in a 200 x 300 map at max_d2 = 4096: the neighbours of a pixel lie 37 rows and / or
    columns away, so with tiles of 32 x 64 every closest pair crosses a tile edge or a tile corner, and the halo is 64 pixels.  The
    shifted lattices put pixels on row and column 0 of the image (and of a tile), on the last row (31) and column (63) of a tile, on the
    first of the next (32, 64), and on the last row (199) and column (299) of the image."""
    shifts = ((5, 11), (0, 0), (TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W), (199 - 5 * 37, 299 - 8 * 37))
    maps = [lattice((200, 300), r, c) for r, c in shifts]
    assert maps[1][0, 0] and maps[2][31, 63] and maps[3][32, 64] and maps[4][199, 299] and maps[4][199, 3] and maps[4][14, 299]
    want = check_many(maps, 4096)
    for m, (t, p) in zip(maps, want):
        n_r, n_c = len(range(np.nonzero(m)[0].min(), 200, 37)), len(range(np.nonzero(m)[1].min(), 300, 37))
        assert len(p) == n_r * (n_c - 1) + (n_r - 1) * n_c + 2 * (n_r - 1) * (n_c - 1) and set(p['min_d2'].tolist()) == {37 * 37, 2 * 37 * 37}
        assert (t['close'][1:] == 1).all() and (t['edges_background'][1:] + t['edges_frame'][1:] == 4).all()
    assert want[4][0]['edges_frame'].sum() == 6 + 9 + 0 + 0 and want[1][0]['edges_frame'].sum() == 6 + 9
    check_many(maps[:2], 37 * 37)                            # the diagonal neighbours fall out; a halo of 37


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_images_smaller_than_a_tile_and_than_the_reach(gpu):
    rng = np.random.default_rng(31)
    maps = [np.array([[4]]), np.array([[0]]), rng.integers(0, 4, (1, 70)), rng.integers(0, 4, (70, 1)), rng.integers(0, 3, (3, 5)),
            np.zeros((40, 70), np.int32), np.full((40, 70), 6, np.uint16), np.full((1, 1), 0, np.int64),
            np.kron(rng.integers(0, 5, (1, 14)), np.ones((1, 5), np.int64)), np.kron(rng.integers(0, 5, (14, 1)), np.ones((5, 1), np.int64))]
    for max_d2 in (1, 2, 17, 4096):
        want = check_many(maps, max_d2)
        assert len(want[0][1]) == len(want[1][1]) == len(want[5][1]) == len(want[6][1]) == 0
        assert want[6][0][6].tolist() == (0, 0, 220, 2800, 0, 0, 0) and want[0][0][4].tolist() == (0, 0, 4, 1, 0, 0, 0)
    assert len(want[2][1]) >= 3 and len(want[3][1]) >= 3 and len(want[8][1]) >= 3


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_label_range(gpu):
    from superdsm_amd import neighbours
    m = np.zeros((5, 70), np.int64)
    m[2, 10:40], m[2, 40:66], m[4, 69] = 1, 65535, 65534
    (t, p), = check_many([m], 25)
    assert len(t) == 65536 and [tuple(r) for r in p.tolist()] == [(1, 65535, 1, 1), (65534, 65535, 20, 0)]
    ok = np.array([[1, 2, 0, 3]] * 3)
    for v, n_labels in ((-1, None), (-2 ** 31, None), (7, 7), (65536, 65536), (2 ** 31 - 1, 4)):
        bad = ok.copy().astype(np.int64)
        bad[1, 2] = bad[2, 3] = v
        with pytest.raises(ValueError, match=r'2 pixels of images \[1\] carry a label outside'):
            neighbours.neighbour_tables_many([ok, bad, ok], 2, n_labels=n_labels)
        with pytest.raises(ValueError, match=r'pixels of images \[0\]'):
            neighbours.neighbour_tables(bad, 2, n_labels=n_labels)
    check_many([ok, ok], 2, n_labels=4)
    check_many([ok], 2, n_labels=65536)


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_contacts(gpu):
    yy, xx = np.mgrid[0:70, 0:131]
    board = (1 + (yy + xx) % 2).astype(np.int32)             # odd sizes, 3 x 3 tiles: every crack edge once, whatever tile owns it
    stripes = (1 + xx % 5).astype(np.int32)                  # columns one pixel wide
    rows = (1 + yy % 3).astype(np.int32).copy()
    ring = np.zeros((80, 140), np.int32)
    ring[5:75, 5:135] = 1
    ring[20:60, 20:120] = 0
    ring[24:56, 24:116] = 2                                  # in the hole, five pixels from the ring all round
    filled = ring.copy()
    filled[20:60, 20:120] = 2                                # the hole filled: contact all round, across all tile seams
    for max_d2 in (1, 2, 25):
        want = check_many([board, stripes, rows, ring, filled], max_d2)
        assert want[0][1].tolist() == [(1, 2, 1, 70 * 130 + 69 * 131)]
        touching = want[1][1][want[1][1]['contact_edges'] > 0]
        assert touching.tolist() == [(a, b, 1, 70 * 26) for a, b in ((1, 2), (1, 5), (2, 3), (3, 4), (4, 5))] and len(want[1][1]) == (10 if max_d2 == 25 else 5)
        assert want[3][1].tolist() == ([(1, 2, 25, 0)] if max_d2 == 25 else []) and want[4][1].tolist() == [(1, 2, 1, 2 * (40 + 100))]


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_many_labels_in_one_disk_and_a_growing_table(gpu):
    """A 16 x 16 block of 256 distinct single-pixel labels over a tile corner at max_d2 = 64: a lane meets a new label at every step, a
    tile meets thousands of pairs, far more than the 256 slots of its LDS table, so most go down the global path."""
    from superdsm_amd import neighbours
    m = np.zeros((64, 128), np.int32)
    m[24:40, 56:72] = 1 + np.random.default_rng(6).permutation(256).reshape(16, 16)
    want_t, want_p = neighbours.neighbour_labels_host(m, 64), neighbours.neighbour_pairs_host(m, 64)
    assert len(want_p) > 15000
    grown, ample = {}, {}
    a = neighbours.neighbour_tables(m, 64, capacity=1, info=grown)                    # the table doubles over several launches
    b = neighbours.neighbour_tables(m, 64, capacity=1 << 17, info=ample)
    check(a, m, 64)
    check(b, m, 64)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert ample['capacity'] == [1 << 17] and grown['capacity'] == [1 << 15] and 2 * len(want_p) <= 1 << 15 < 4 * len(want_p)
    assert (want_t['close'][1:] == 1).all()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_dirty_buffers_and_the_same_call_twice(gpu):
    """sdsm_neighbours through the C ABI into buffers that live across calls, dirtied with 0xff and 0x00: the call clears what it writes."""
    import torch
    from superdsm_amd import _capi, neighbours
    from superdsm_amd.render import _DeviceSet
    labels = label_scene(np.random.default_rng(71), (70, 150), 25)
    n_labels, cap, max_d2 = int(labels.max()) + 3, 256, 30
    want_t, want_p = neighbours.neighbour_labels_host(labels, max_d2, n_labels), neighbours.neighbour_pairs_host(labels, max_d2)
    assert 4 <= len(want_p) <= cap // 2
    S = _DeviceSet([labels.shape])
    d_map = S.pack([labels], np.int32)
    d_rec = torch.empty(n_labels * 40, dtype=torch.uint8, device=S.dev)
    d_keys = torch.empty(cap, dtype=torch.int64, device=S.dev)
    d_min, d_contact, d_status = (torch.empty(n, dtype=torch.int32, device=S.dev) for n in (cap, cap, 2))
    results = []
    for byte in (0xff, 0x00, 0xff, 0xff):                    # (the last two: the same call twice)
        for t in (d_rec, d_keys, d_min, d_contact, d_status):
            t.view(torch.uint8).fill_(byte)
        _capi.check(S.L.sdsm_neighbours(labels.shape[0], labels.shape[1], S._p(d_map), max_d2, n_labels, S._p(d_rec), cap, S._p(d_keys), S._p(d_min),
                                        S._p(d_contact), S._p(d_status), S._stream()), 'sdsm_neighbours')
        results.append([t.cpu().numpy().copy() for t in (d_rec, d_keys, d_min, d_contact, d_status)])
    for rec, keys, mins, contact, status in results:         # (the slot a pair ends in may depend on who came first: the sorted table may not)
        assert rec.view(neighbours.LABEL_DTYPE).tobytes() == want_t.tobytes() and status.tolist() == [0, 0]
        used = keys != -1
        assert used.sum() == len(want_p) and (mins[~used] == -1).all() and (contact[~used] == 0).all()
        assert neighbours._pairs_from_keys(keys.view(np.uint64)[used], mins[used], contact[used]).tobytes() == want_p.tobytes()


def test_sets_equal_single_images_and_long_lists_are_split(gpu):
    from superdsm_amd import neighbours
    rng = np.random.default_rng(72)
    maps = [label_scene(rng, (37, 53), 9), label_scene(rng, (90, 120), 14).astype(np.uint16), label_scene(rng, (33, 129), 16).astype(np.int64)]
    wide = np.zeros((37, 60), np.int64)                      # a view with unaligned rows
    wide[:, 3:56] = maps[0]
    maps.append(wide[:, 3:56])
    for max_d2 in (2, 30):
        many = neighbours.neighbour_tables_many(maps, max_d2)
        for m, g in zip(maps, many):
            want_t, want_p = check(g, m, max_d2)
            one = neighbours.neighbour_tables(m, max_d2)
            assert one[0].tobytes() == want_t.tobytes() and one[1].tobytes() == want_p.tobytes() and len(want_p) >= 1
    tiny = [np.kron(rng.integers(0, 4, (3 + k % 3, 4)), np.ones((2, 3), np.int64)) for k in range(33)]
    info = {}
    got = neighbours.neighbour_tables_many(tiny, 10, capacity=4, info=info)
    assert len(got) == 33 and len(info['capacity']) == 33
    for m, g, c in zip(tiny, got, info['capacity']):
        _, want_p = check(g, m, 10)
        assert c >= max(4, 2 * len(want_p)) and c & (c - 1) == 0


# 8 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_d2', [1, 2, 9, 400])
def test_random_scenes(gpu, max_d2):
    rng = np.random.default_rng(8)
    maps = [label_scene(rng) for _ in range(3)] + [label_scene(rng, (61, 47), 25), label_scene(rng, (130, 200), 40)]
    want = check_many(maps, max_d2)
    assert all(len(p) >= 2 for _, p in want) and sum(int((p['contact_edges'] > 0).sum()) for _, p in want) >= 10
    if max_d2 == 400:
        assert any((t['close'] < t['boundary']).any() for t, _ in want) and any(p['min_d2'].max() > 200 for _, p in want)


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_result_of_objects(gpu):
    from superdsm_amd import neighbours, render, testing
    rng = np.random.default_rng(9)
    shape = (90, 120)
    objs = []
    for k in range(8):                                       # fragments that overlap their neighbours: the label map makes them disjoint
        f = ellipse(rng, 12, erode=False)
        objs.append(testing.PostFragment((2 + 18 * (k // 4) + int(rng.integers(0, 4)), 2 + 14 * (k % 4) + int(rng.integers(0, 4))), f))
    data = {'g_raw': np.zeros(shape), 'postprocessed_objects': objs}
    labels = render.rasterize_labels(data)
    assert labels.max() >= 6
    for max_d2 in (2, 100):
        want_t, want_p = check(neighbours.neighbours_result(data, max_d2=max_d2), labels, max_d2)
        assert len(want_p) >= 4
        again = neighbours.neighbours_result(data, objects=objs, max_d2=max_d2)
        both = neighbours.neighbours_results([data, data], max_d2=max_d2)
        for g in (again, both[0], both[1]):
            assert g[0].tobytes() == want_t.tobytes() and g[1].tobytes() == want_p.tobytes()
    d = neighbours.derive(want_t, want_p)
    assert len(d) == len(np.unique(labels)) - 1 and (d['n_neighbours'] >= d['n_touching']).all() and d['n_touching'].sum() > 0
