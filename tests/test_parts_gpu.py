"""The GPU form of the connected parts (sdsm_parts.hip) against the host definitions of superdsm_amd/parts.py -- the part map with
``np.array_equal`` and the dtype, the two tables byte by byte -- on the smallest maps at which the kernels can still go wrong: pixel
pairs across every kind of tile seam, chains that wind through many tiles, more parts and labels than a tile's tables hold, rings over
tile corners, images smaller than a tile, the ends of the label range, dirty buffers, sets.  The tile kernel's tile is 32 rows x 64
columns (PTH x PTW of sdsm_parts.hip), its label table has 256 slots, and a workgroup of the raster kernels takes 2048 pixels."""
import numpy as np
import pytest
from scipy import ndimage as ndi

from test_measure_cpu import label_scene

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 32, 64
LABEL_SLOTS = 256
CHUNK = 2048


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    return torch.device('cuda', 0)


def same_map(got, want, what=''):
    assert got.dtype == want.dtype == np.int32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = np.argwhere(got != want)
        raise AssertionError(f'{what}: {len(at)} pixels differ, the first at {tuple(at[0])}: {got[tuple(at[0])]} (GPU) != {want[tuple(at[0])]} (host)')


def same_table(got, want, what=''):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        k = next(i for i in range(len(got)) if got[i] != want[i])
        raise AssertionError(f'{what}: row {k}: {got[k]} (GPU) != {want[k]} (host)')


def same(got, want, what=''):
    same_map(got[0], want[0], what + ' part map')
    same_table(got[1], want[1], what + ' part table')
    same_table(got[2], want[2], what + ' label table')


def check(maps, connectivities=(4, 8)):
    """Every map of a list, in one call per adjacency, against parts_host; returns the host results per adjacency."""
    from superdsm_amd import parts
    out = {}
    for c in connectivities:
        got = parts.parts_many(maps, c)
        out[c] = [parts.parts_host(m, c) for m in maps]
        assert len(got) == len(maps)
        for i, (g, w) in enumerate(zip(got, out[c])):
            same(g, w, f'image {i}, connectivity {c}:')
    return out


def holes(res, connectivity):
    from superdsm_amd import parts
    return parts.derive(res[2], connectivity)['holes'].tolist()


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def bars(shape):
    """Bars of one label across the seam to the right, the seam below and the corner of the first tile; each is one part."""
    m = np.zeros(shape, np.int32)
    m[5, TILE_W - 3:TILE_W + 1] = 1                          # over the right seam
    m[TILE_H - 3:TILE_H + 1, 7] = 1                          # over the lower seam
    for k in range(-2, 2):
        m[TILE_H + k - 1, TILE_W + k - 1] = 1                # a diagonal through the corner: one part under 8 only
    m[TILE_H - 2:TILE_H + 1, TILE_W - 9:TILE_W - 6] = 2      # a block over the lower seam
    m[20, TILE_W - 1:TILE_W + 1] = 3                         # two pixels, one on either side of the right seam
    return m


@pytest.mark.parametrize('shape', [(33, 65), (64, 128), (40, 70)])
def test_seams(gpu, shape):
    down, up = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    down[TILE_H - 1, TILE_W - 1] = down[TILE_H, TILE_W] = 4  # the pair (31, 63) - (32, 64) alone
    up[TILE_H - 1, TILE_W] = up[TILE_H, TILE_W - 1] = 4      # the pair (31, 64) - (32, 63) alone
    both = down + up                                         # a block of 2 x 2 over the corner
    res = check([bars(shape), down, up, both])
    for i in (1, 2):
        assert len(res[4][i][1]) == 2 and len(res[8][i][1]) == 1 and res[8][i][1]['area'][0] == 2
    assert len(res[4][3][1]) == 1 and res[4][0][2]['n_parts'].tolist() == [0, 6, 1, 1] and res[8][0][2]['n_parts'].tolist() == [0, 3, 1, 1]


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def serpentine(shape):
    """A path one pixel wide: every other row, joined at alternating ends."""
    m = np.zeros(shape, np.int32)
    m[::2] = 1
    m[1::4, -1] = 1
    m[3::4, 0] = 1
    return m


def comb(shape):
    """Teeth of label 1 on every other column that join in the last row only, and bars of label 2 between them that end above it."""
    m = np.zeros(shape, np.int32)
    m[:, ::2] = 1
    m[-1] = 1
    m[:-2, 1::2] = 2
    return m


def spiral(h, w):
    """A rectangular spiral one pixel wide with one pixel between its turns."""
    m = np.zeros((h, w), np.int32)
    r0, c0, r1, c1 = 0, 0, h - 1, w - 1
    while r1 - r0 >= 2 and c1 - c0 >= 2:
        m[r0, c0:c1 + 1] = m[r0:r1 + 1, c1] = m[r1, c0:c1 + 1] = 1
        m[r0 + 2:r1 + 1, c0] = 1
        m[r0 + 2, c0:c0 + 2] = 1
        r0, c0, r1, c1 = r0 + 2, c0 + 2, r1 - 2, c1 - 2
    return m


def test_long_chains(gpu):
    s = serpentine((70, 140))
    maps = [s, s[::-1].copy(), s[:, ::-1].copy(), s.T.copy(), comb((70, 140)), comb((70, 140))[::-1].copy(), spiral(TILE_H - 1, TILE_W - 1),
            spiral(70, 140)]
    res = check(maps)
    for c in (4, 8):
        assert [len(res[c][i][1]) for i in (0, 1, 2, 3, 6, 7)] == [1] * 6 and res[c][0][1]['area'][0] == s.sum()
        assert res[c][1][1]['first'][0] == 0 or res[c][1][1]['first'][0] == 139     # the flipped path starts in the first row all the same
        part_map, table, labels = res[c][4]
        assert labels['n_parts'].tolist() == [0, 1, 70] and table['label'][:4].tolist() == [1, 2, 2, 2] and (part_map[:, ::2] == 1).all()
        assert res[c][5][2]['n_parts'].tolist() == [0, 1, 70] and res[c][5][0][0, 0] == 1
    assert holes(res[4][7], 4) == [0, 0] and (maps[7] == 0).any()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_many_parts_and_labels(gpu):
    board = (np.indices((2 * TILE_H, 2 * TILE_W)).sum(0) % 2 + 1).astype(np.int32)
    grid = 1 + np.random.default_rng(6).permutation(1600).reshape(40, 40).astype(np.int32)
    block = np.zeros((64, 128), np.int32)
    block[24:40, 56:72] = 1 + np.random.default_rng(6).permutation(256).reshape(16, 16)
    assert grid.max() > LABEL_SLOTS
    res = check([board, grid, block])
    part_map, table, labels = res[4][0]
    assert len(table) == 8192 > CHUNK and np.array_equal(part_map.reshape(-1), np.arange(1, 8193)) and (table['area'] == 1).all()
    assert labels['n_parts'].tolist() == [0, 4096, 4096] and labels['largest_part'].tolist() == [0, 1, 2]
    assert len(res[8][0][1]) == 2 and res[8][0][2]['largest_area'].tolist() == [0, 4096, 4096]
    for c in (4, 8):
        assert len(res[c][1][1]) == 1600 and (res[c][1][2]['n_parts'][1:] == 1).all() and (res[c][1][2]['q1'][1:] == 4).all()
        assert len(res[c][2][1]) == 256


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_one_label_apart_and_two_labels_touching(gpu):
    apart = np.zeros((70, 140), np.int32)
    apart[3:9, 4:12] = apart[50:60, 100:130] = 5             # the first and the last tile
    touching = np.zeros((70, 140), np.int32)
    touching[10:60, :70], touching[10:60, 70:] = 1, 2        # a long edge inside a tile column
    touching[30:33] = np.where(np.arange(140) % 2, 1, 2)     # and interleaved columns across everything
    scene = label_scene(np.random.default_rng(41), (90, 120), 14)
    res = check([apart, touching, scene])
    for c in (4, 8):
        assert res[c][0][1]['label'].tolist() == [5, 5] and res[c][0][1]['area'].tolist() == [48, 300] and res[c][0][2][5]['largest_part'] == 2
        assert set(np.unique(res[c][1][0][touching == 1])) .isdisjoint(np.unique(res[c][1][0][touching == 2]))
    assert res[4][2][2]['n_parts'].max() >= 2                # the scene's ellipses cut each other


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_holes(gpu):
    ring = np.zeros((20, 20), np.int32)
    ring[3:12, 3:12], ring[5:10, 5:10] = 1, 0
    filled = ring.copy()
    filled[6:9, 6:9] = 2                                     # another label inside counts as a hole of the ring
    diamond = np.zeros((5, 5), np.int32)
    diamond[1, 2] = diamond[2, 1] = diamond[2, 3] = diamond[3, 2] = 1
    c_shape = np.zeros((12, 12), np.int32)
    c_shape[2:10, 0:8], c_shape[4:8, 0:6] = 1, 0             # open towards the frame on the left
    bay = np.zeros((12, 12), np.int32)
    bay[0:6, 2:9], bay[0:4, 4:7] = 1, 0                      # a bay that only the frame closes
    corner = np.zeros((2 * TILE_H, 2 * TILE_W), np.int32)
    corner[TILE_H - 6:TILE_H + 6, TILE_W - 8:TILE_W + 8], corner[TILE_H - 3:TILE_H + 3, TILE_W - 4:TILE_W + 4] = 3, 0
    res = check([ring, filled, diamond, c_shape, bay, corner])
    for c in (4, 8):
        assert holes(res[c][0], c) == [0, 1] and holes(res[c][1], c) == [0, 1, 0] and holes(res[c][3], c) == [0, 0] and holes(res[c][4], c) == [0, 0]
        assert holes(res[c][5], c) == [0, 0, 0, 1] and len(res[c][5][1]) == 1
    assert (len(res[8][2][1]), holes(res[8][2], 8)) == (1, [0, 1]) and (len(res[4][2][1]), holes(res[4][2], 4)) == (4, [0, 0])


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_shapes_and_sets(gpu):
    from superdsm_amd import parts
    rng = np.random.default_rng(31)
    maps = [np.array([[4]]), np.array([[0]]), rng.integers(0, 3, (1, 200)), rng.integers(0, 3, (200, 1)), rng.integers(0, 3, (5, 9)),
            np.zeros((5, 9), np.int32), np.full((5, 9), 6, np.uint16), np.zeros((0, 5), np.int32), rng.integers(0, 2, (31, 63)).astype(np.int64),
            np.zeros((3, 0), np.int64), rng.integers(0, 4, (37, 70)).astype(np.uint8)]
    wide = np.zeros((37, 80), np.int64)                      # a view with unaligned rows
    wide[:, 3:73] = maps[-1]
    maps.append(wide[:, 3:72])
    res = check(maps)
    for c in (4, 8):
        assert res[c][0][1].tolist() == [(4, 1, 0, 0, 0, 1, 1, 0)] and len(res[c][0][2]) == 5 and len(res[c][1][1]) == 0 and len(res[c][5][2]) == 1
        assert res[c][7][0].shape == (0, 5) and res[c][9][0].shape == (3, 0) and res[c][6][1]['area'].tolist() == [45]
        many = parts.parts_many(maps, c)
        for m, w in zip(maps, many):
            same(parts.parts(m, c), w, 'one by one:')        # the set's bytes are the single image's
        for g, w in zip(parts.parts_many(maps, c), many):
            same(g, w, 'the same call again:')
    tiny = [rng.integers(0, 3, (3, 4)) for _ in range(33)]   # two sets
    check(tiny)


def test_into_dirty_buffers(gpu):
    """sdsm_parts and the two calls behind it through the C ABI into buffers filled with garbage, workspace included: every pixel of every
    map and every field of every record is written, and the same calls twice give the same bytes."""
    import torch
    from superdsm_amd import _capi, parts
    from superdsm_amd.render import _DeviceSet
    K = parts.Keep
    labels = label_scene(np.random.default_rng(71), (70, 150), 25)
    keeps = [K.split(), K.largest(), K.min_area(20)]
    H, W = labels.shape
    n_labels = int(labels.max()) + 1
    S = _DeviceSet([labels.shape])
    C, L = S.C, S.L
    d_map = S.pack([labels], np.int32)
    off, nl = (C.c_int64 * 1)(0), (C.c_int32 * 1)(n_labels)
    ws_bytes = L.sdsm_parts_workspace_bytes_multi(S.table, 1, off, nl)
    assert ws_bytes >= 8 * H * W
    specs = np.array([k.spec() for k in keeps], np.int32).view(_capi.KEEP_SPEC_DTYPE)
    for connectivity in (4, 8):
        want = parts.parts_host(labels, connectivity)
        want_keep = parts.keep_maps_host(labels, keeps, connectivity)
        for garbage in (-1, 0x5a5a5a5a, -1):
            fill = lambda n: torch.empty(n, dtype=torch.int32, device=S.dev).fill_(garbage)
            d_ws, d_rec, d_part_map, d_count, d_status = fill((ws_bytes + 3) // 4 + 2), fill(8 * n_labels), fill(H * W), fill(1), fill(1)
            _capi.check(L.sdsm_parts(H, W, S._p(d_map), connectivity, n_labels, S._p(d_rec), S._p(d_part_map), S._p(d_count), S._p(d_status), S._p(d_ws),
                                     ws_bytes, S._stream()), 'sdsm_parts')
            assert d_status.cpu().numpy().tolist() == [0] and d_count.cpu().numpy().tolist() == [len(want[1])]
            k = len(want[1])
            d_parts, d_keep = fill(8 * k), fill(len(keeps) * H * W)
            n_parts = (C.c_int32 * 1)(k)
            _capi.check(L.sdsm_parts_table_multi(S.table, 1, S._p(d_map), S._p(d_part_map), off, n_parts, S._p(d_parts), S._stream()), 'sdsm_parts_table_multi')
            _capi.check(L.sdsm_parts_keep_multi(S.table, 1, S._p(d_map), S._p(d_part_map), off, nl, S._p(d_rec), off, n_parts, S._p(d_parts), len(keeps),
                                                specs.ctypes.data_as(C.c_void_p), H * W, S._p(d_keep), S._stream()), 'sdsm_parts_keep_multi')
            table = d_parts.cpu().numpy().view(parts.PART_DTYPE)
            assert not table['index_in_label'].any()         # the device leaves it to the caller
            table['index_in_label'] = want[1]['index_in_label']
            same((d_part_map.cpu().numpy().reshape(H, W), table, d_rec.cpu().numpy().view(parts.LABEL_DTYPE)), want, f'connectivity {connectivity}:')
            for g, w in zip(d_keep.cpu().numpy().reshape(len(keeps), H, W), want_keep):
                same_map(g, w, 'selection')
    # what the entry points refuse
    d_any = torch.zeros(64, dtype=torch.int32, device=S.dev)
    assert L.sdsm_parts(H, W, S._p(d_map), 6, n_labels, S._p(d_rec), S._p(d_part_map), S._p(d_count), S._p(d_status), S._p(d_ws), ws_bytes, S._stream()) != 0
    assert b'connectivity' in L.sdsm_last_error()
    assert L.sdsm_parts(H, W, S._p(d_map), 4, n_labels, S._p(d_rec), S._p(d_part_map), S._p(d_count), S._p(d_status), S._p(d_ws), ws_bytes - 1, S._stream()) != 0
    assert b'workspace' in L.sdsm_last_error()
    bad = np.array([(2, 0)], _capi.KEEP_SPEC_DTYPE)
    assert L.sdsm_parts_keep_multi(S.table, 1, S._p(d_map), S._p(d_part_map), off, nl, S._p(d_rec), off, n_parts, S._p(d_parts), 1,
                                   bad.ctypes.data_as(C.c_void_p), H * W, S._p(d_any), S._stream()) != 0
    assert b'min_area' in L.sdsm_last_error()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_label_range(gpu):
    from superdsm_amd import parts
    m = np.zeros((5, 70), np.int64)
    m[:, 10:40], m[:, 40:66], m[4, 69], m[0, 0] = 1, 65535, 65534, 65535
    res = check([m.astype(np.uint16), m])
    assert len(res[4][0][2]) == 65536 and res[4][0][2][65535]['n_parts'] == 2 and res[4][0][1]['label'].tolist() == [65535, 1, 65535, 65534]
    ok = np.array([[1, 2, 0, 3]] * 3)
    for v in (65536, -1, 70000, -2 ** 31, 2 ** 31 - 1):
        bad = ok.copy().astype(np.int64)
        bad[1, 2] = bad[2, 3] = v
        with pytest.raises(ValueError, match=r'2 pixels of images \[1\] carry a label outside'):
            parts.parts_many([ok, bad, ok], 8)
        with pytest.raises(ValueError, match=r'pixels of images \[0\]'):
            parts.keep_maps(bad, [parts.Keep.largest()])
    check([ok, ok])                                          # the other images of that list, in a later call
    with pytest.raises(ValueError, match='labels'):
        parts.parts(np.array([[0, 2 ** 31]]))


# 8 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(50, 70), (97, 131)])
def test_random_maps(gpu, shape):
    rng = np.random.default_rng(8)
    maps = [np.where(rng.random(shape) < density, rng.integers(1, n + 1, shape), 0) for n in (1, 2, 3) for density in (0.3, 0.5, 0.7)]
    res = check(maps)
    assert all(len(res[4][i][1]) > len(res[8][i][1]) > 1 for i in range(len(maps)))


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_selections(gpu):
    from superdsm_amd import parts
    K = parts.Keep
    tie = np.zeros((40, 70), np.int32)
    tie[2:4, 60:62] = tie[34:36, 66:68] = tie[20, 5:9] = 3   # three parts of area 4 in three tiles: the first wins
    tie[10:12, 10:13] = tie[36, 0:6] = 9                     # two of area 6
    scene = label_scene(np.random.default_rng(43), (90, 120), 14)
    keeps = [K.split(), K.largest(), K.min_area(1), K.min_area(5), K.min_area(2 ** 31 - 1), K.largest(), K.min_area(30), K.split()]
    for c in (4, 8):
        got = parts.keep_maps_many([tie, scene, np.zeros((0, 4), np.int32)], keeps, c)
        for m, g in zip((tie, scene, np.zeros((0, 4), np.int32)), got):
            want = parts.keep_maps_host(m, keeps, c)
            assert len(g) == len(want) == 8
            for a, b in zip(g, want):
                same_map(a, b, f'connectivity {c}')
        largest = got[0][1]
        assert (largest[2:4, 60:62] == 3).all() and (largest[10:12, 10:13] == 9).all() and largest.sum() == 4 * 3 + 6 * 9
        assert np.array_equal(got[0][2], tie) and not got[0][4].any() and np.array_equal(got[0][3], np.where(tie == 9, 9, 0))
        same_map(parts.keep_maps(scene, K.largest(), c)[0], got[1][1])


# 10 --------------------------------------------------------------------------------------------------------------------------------
def test_label_mask(gpu):
    from superdsm_amd import parts
    rng = np.random.default_rng(10)
    masks = [rng.random((70, 140)) < 0.55, rng.random((33, 65)) < 0.4, (rng.random((40, 40)) < 0.6).astype(np.uint8) * 255]
    for c in (4, 8):
        for mask, (part_map, table, labels) in zip(masks, parts.label_mask_many(masks, c)):
            want, k = ndi.label(mask, parts.structure(c))
            same_map(part_map, want.astype(np.int32), f'connectivity {c}')
            assert len(table) == k and (table['label'] == 1).all() and len(labels) == 2 and labels[1]['n_parts'] == k
        same(parts.label_mask(masks[0], c), parts.label_mask_host(masks[0], c))


# 11 --------------------------------------------------------------------------------------------------------------------------------
def test_result_of_objects(gpu):
    from superdsm_amd import parts, render, testing
    objs = [testing.PostFragment((1, 1), np.ones((9, 12), bool)), testing.PostFragment((4, 0), np.ones((3, 20), bool)),
            testing.PostFragment((14, 16), np.ones((3, 3), bool))]
    data = {'g_raw': np.random.default_rng(71).random((20, 25)), 'postprocessed_objects': objs}
    labels = render.rasterize_labels(data)
    for c in (4, 8):
        want = parts.parts_host(labels, c)
        same(parts.parts_result(data, connectivity=c), want)
        same(parts.parts_result(data, objects=objs, connectivity=c), want)
        for got in parts.parts_results([data, data], connectivity=c):
            same(got, want)
    assert labels.max() == 3 and len(want[1]) >= 3


def test_the_maps_go_into_the_tables_as_they_come(gpu):
    from superdsm_amd import measure, parts
    labels = label_scene(np.random.default_rng(73), (70, 90), 10)
    split_gpu, split_host = parts.keep_maps(labels, parts.Keep.split())[0], parts.keep_maps_host(labels, parts.Keep.split())[0]
    same_map(split_gpu, split_host)
    table = measure.measure_labels(split_gpu)
    want = measure.measure_labels_host(split_host)
    assert table.dtype == want.dtype and table.tobytes() == want.tobytes() and len(table) == split_host.max() > 5
