"""The GPU forms of the boundary distances (k_label_pixel_counts, k_label_pixel_lists, k_pair_distances, sdsm_measure.hip) against the
host definitions of superdsm_amd/boundary.py, byte for byte, on the smallest shapes at which the kernels can still go wrong: lists that
straddle the LDS tile and the query chunk, coordinates above 32 767 and squared distances near 2^31, unaligned widths, absent labels,
sets, dirty buffers."""
import numpy as np
import pytest

from test_boundary_cpu import CATALOGUE, disc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    return torch.device('cuda', 0)


def same_lists(x, y):
    return all(np.array_equal(p, q) and p.dtype == q.dtype for p, q in zip(x, y))


def same_scores(x, y):
    assert x.keys() == y.keys()
    for k in x:
        if isinstance(x[k], np.ndarray):
            assert x[k].dtype == y[k].dtype and x[k].tobytes() == y[k].tobytes(), k
        else:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=True), k


def lines(n_a, n_b, shift=2):
    """Two one-pixel-wide lines in the middle row of a 3-row image: every pixel is a boundary pixel, so the lists have n_a and n_b entries."""
    W = max(n_a, n_b + shift) + 3
    a, b = np.zeros((3, W), np.int32), np.zeros((3, W), np.int32)
    a[1, :n_a] = 1
    b[1, shift:shift + n_b] = 1
    return a, b


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CATALOGUE))
def test_catalogue_tables_lists_and_scores(gpu, name):
    from superdsm_amd import boundary
    a, b = CATALOGUE[name]
    host = boundary.pair_distances_host(a, b)
    got = boundary.pair_distances(a, b)
    assert got.dtype == boundary.PAIR_DISTANCE_DTYPE and got.tobytes() == host.tobytes() and len(host) >= 1
    for labels in (a, b):
        assert same_lists(boundary.label_boundaries(labels), boundary.label_boundaries_host(labels))
    same_scores(boundary.compare_boundaries(a, b), boundary.distance_scores(host, np.unique(b[b != 0])))
    same_scores(boundary.compare_boundaries(a, b), boundary.compare_boundaries_host(a, b))


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_checkerboard_spans_several_tiles_and_chunks(gpu):
    from superdsm_amd import _capi, boundary
    yy, xx = np.mgrid[0:128, 0:128]
    a = ((yy + xx) % 2 == 0).astype(np.int32)
    b = np.zeros((128, 128), np.int32)
    b[disc(b.shape, (70, 60), 18)] = 3
    host = boundary.pair_distances_host(a, b)
    assert host['boundary_a'].tolist() == [8192] and 8192 > 4 * max(_capi.BOUNDARY_TILE, _capi.BOUNDARY_CHUNK)
    assert boundary.pair_distances(a, b).tobytes() == host.tobytes()
    assert boundary.pair_distances(b, a).tobytes() == boundary.pair_distances_host(b, a).tobytes()         # the long list as the target
    assert same_lists(boundary.label_boundaries(a), boundary.label_boundaries_host(a))


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_lists_around_the_tile_and_the_chunk(gpu):
    from superdsm_amd import _capi, boundary
    sizes = sorted({s + d for s in (_capi.BOUNDARY_TILE, _capi.BOUNDARY_CHUNK) for d in (-1, 0, 1)} | {2 * _capi.BOUNDARY_CHUNK + 1})
    maps = [lines(n, m) for n in sizes for m in (sizes[0], n)]
    got = boundary.pair_distances_many([a for a, _ in maps], [b for _, b in maps])
    for (a, b), g in zip(maps, got):
        host = boundary.pair_distances_host(a, b)
        assert (host['boundary_a'][0], host['boundary_b'][0]) == ((a == 1).sum(), (b == 1).sum()) and g.tobytes() == host.tobytes()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_coordinates_above_32767_and_distances_near_2_31(gpu):
    from superdsm_amd import boundary
    a, b = np.zeros((3, 40000), np.uint16), np.zeros((3, 40000), np.int64)
    a[:, 0:3], b[:, 39997:40000] = 1, 2
    host = boundary.pair_distances_host(a, b, [(1, 2)])
    assert host['max_d2_ab'][0] == 39995 ** 2 > 1.5e9 and host['max_d2_ba'][0] == 39995 ** 2 and host['nsd_den'][0] > 2 ** 32
    assert boundary.pair_distances(a, b, [(1, 2)]).tobytes() == host.tobytes()
    assert len(boundary.pair_distances(a, b)) == 0                                          # they do not overlap
    assert same_lists(boundary.label_boundaries(b), boundary.label_boundaries_host(b))


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_unaligned_widths(gpu):
    from superdsm_amd import boundary
    from test_measure_cpu import label_scene
    rng = np.random.default_rng(5)
    a, b = label_scene(rng, (37, 53), 9), label_scene(rng, (37, 53), 8)
    host = boundary.pair_distances_host(a, b)
    assert len(host) > 5 and boundary.pair_distances(a, b).tobytes() == host.tobytes()
    wide = np.zeros((37, 60), np.int64)                                                     # a view with unaligned rows
    wide[:, 3:56] = a
    assert boundary.pair_distances(wide[:, 3:56], b.astype(np.uint16)).tobytes() == host.tobytes()
    a, b = np.array([[0, 1, 1, 1, 0, 2, 2]]), np.array([[1, 1, 0, 2, 2, 2, 0]])
    host = boundary.pair_distances_host(a, b)
    assert len(host) == 3 and boundary.pair_distances(a, b).tobytes() == host.tobytes()
    assert same_lists(boundary.label_boundaries(a), boundary.label_boundaries_host(a))


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_pair_lists_absent_labels_repeats_and_none(gpu):
    from superdsm_amd import boundary
    a, b = CATALOGUE['three pairs']
    pairs = [(1, 10), (77, 10), (3, 30), (1, 10), (2, 65535), (3, 4)]
    host = boundary.pair_distances_host(a, b, pairs)
    got = boundary.pair_distances(a, b, pairs)
    assert got.tobytes() == host.tobytes()
    assert got['flags'].tolist() == [0, 1, 0, 0, 2, 0] and got[0].tobytes() == got[3].tobytes() and got['max_d2_ab'][1] == -1
    none = boundary.pair_distances(a, b, [])
    assert none.dtype == boundary.PAIR_DISTANCE_DTYPE and len(none) == 0
    assert len(boundary.pair_distances(np.zeros((0, 5), np.int32), np.zeros((0, 5), np.int32))) == 0      # an empty image: no launch


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_sets_equal_single_images_and_long_lists_are_split(gpu):
    from superdsm_amd import boundary
    from test_measure_cpu import label_scene
    rng = np.random.default_rng(7)
    shapes = [(1, 7), (37, 53), (64, 64)]
    a_list = [label_scene(rng, s, 5) if s[0] > 1 else np.array([[0, 1, 1, 1, 0, 2, 2]]) for s in shapes]
    b_list = [label_scene(rng, s, 6) if s[0] > 1 else np.array([[1, 1, 0, 2, 2, 2, 0]]) for s in shapes]
    many = boundary.pair_distances_many(a_list, b_list)
    for a, b, g in zip(a_list, b_list, many):
        host = boundary.pair_distances_host(a, b)
        assert len(host) and g.tobytes() == host.tobytes() and boundary.pair_distances(a, b).tobytes() == host.tobytes()
    for got, want in zip(boundary.label_boundaries_many(a_list), [boundary.label_boundaries_host(a) for a in a_list]):
        assert same_lists(got, want)
    a33 = [np.kron(rng.integers(0, 4, (5 + k % 3, 6)), np.ones((2, 3), np.int64)) for k in range(33)]
    b33 = [np.roll(x, 1, axis=1) for x in a33]
    got = boundary.pair_distances_many(a33, b33)
    assert len(got) == 33
    for a, b, g in zip(a33, b33, got):
        assert g.tobytes() == boundary.pair_distances_host(a, b).tobytes()
    for s, a, b in zip(boundary.compare_boundaries_many(a33[:3], b33[:3]), a33, b33):
        same_scores(s, boundary.compare_boundaries_host(a, b))


# 8 ---------------------------------------------------------------------------------------------------------------------------------
class Raw:
    """The three entry points through the C ABI on buffers that live across calls."""

    def __init__(self, a, b):
        import torch
        from superdsm_amd import _capi
        from superdsm_amd.render import _DeviceSet
        self.S, self.shape, L = _DeviceSet([a.shape]), a.shape, _capi.BOUNDARY_MAX_LABELS
        S = self.S
        self.d_map = [S.pack([a], np.int32), S.pack([b], np.int32)]
        new = lambda n: torch.empty(n, dtype=torch.int32, device=S.dev)
        self.d_counts, self.d_start, self.d_list = [new(2 * L), new(2 * L)], [new(L), new(L)], [new(S.total), new(S.total)]
        self.d_cursor, self.d_bad, self.d_rec = new(2 * L), new(2), new(16 * 64)
        self.torch = torch

    def dirty(self, byte):
        for t in self.d_counts + self.d_start + self.d_list + [self.d_cursor, self.d_bad, self.d_rec]:
            t.view(self.torch.uint8).fill_(byte)

    def __call__(self, pairs):
        from superdsm_amd import _capi, boundary
        S, (H, W), L = self.S, self.shape, _capi.BOUNDARY_MAX_LABELS
        for k in range(2):
            _capi.check(S.L.sdsm_label_pixel_counts(H, W, S._p(self.d_map[k]), S._p(self.d_counts[k]), S._p(self.d_bad[k:]), S._stream()), 'counts')
            _capi.check(S.L.sdsm_label_pixel_lists(H, W, S._p(self.d_map[k]), S._p(self.d_counts[k]), S._p(self.d_start[k]), S._p(self.d_cursor),
                                                   S._p(self.d_list[k]), S._stream()), 'lists')
        counts = [c.cpu().numpy().reshape(1, L, 2) for c in self.d_counts]
        rows = np.zeros((len(pairs), 4), np.int32)
        rows[:, 1:3] = pairs
        items = boundary.work_items(rows, counts[0], counts[1])
        d_rows, d_items = S._up(rows), S._up(items)
        _capi.check(S.L.sdsm_pair_distances(H, W, S._p(self.d_map[0]), S._p(self.d_map[1]), S._p(self.d_counts[0]), S._p(self.d_counts[1]),
                                            S._p(self.d_start[0]), S._p(self.d_start[1]), S._p(self.d_list[0]), S._p(self.d_list[1]), len(rows), S._p(d_rows),
                                            len(items), S._p(d_items), S._p(self.d_rec), S._stream()), 'distances')
        rec = self.d_rec.cpu().numpy().view(boundary.PAIR_DISTANCE_DTYPE)[:len(rows)]
        starts = [s.cpu().numpy() for s in self.d_start]
        lists = []
        for k in range(2):                                                                  # every label's two parts, each sorted
            packed = self.d_list[k].cpu().numpy().view(np.uint32)
            for l in np.nonzero(counts[k][0, 1:, 0])[0] + 1:
                s, n, nb = starts[k][l], counts[k][0, l, 0], counts[k][0, l, 1]
                lists.append((np.sort(packed[s:s + nb]), np.sort(packed[s + nb:s + n])))
        return rec.copy(), counts, starts, lists, self.d_bad.cpu().numpy()


def test_dirty_buffers_do_not_matter(gpu):
    from superdsm_amd import boundary
    a, b = CATALOGUE['touching objects']
    pairs = [(1, 1), (2, 1), (2, 300), (65535, 1), (9, 1)]
    host = boundary.pair_distances_host(a, b, pairs)
    raw = Raw(a, b)
    results = []
    for byte in (0xff, 0x00, 0xa5):
        raw.dirty(byte)
        results.append(raw(pairs))
    rec, counts, starts, lists, bad = results[0]
    assert rec.tobytes() == host.tobytes() and bad.tolist() == [0, 0]
    present, offsets, coords = boundary.label_boundaries_host(a)
    assert [(int(v >> 16), int(v & 0xffff)) for part in lists[:len(present)] for v in part[0]] == [tuple(rc) for rc in coords.tolist()]
    assert sum(len(p[0]) + len(p[1]) for p in lists) == (a != 0).sum() + (b != 0).sum()
    for other in results[1:]:
        assert other[0].tobytes() == rec.tobytes() and other[4].tolist() == [0, 0]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(other[1] + other[2], counts + starts))
        assert all(p[0].tobytes() == q[0].tobytes() and p[1].tobytes() == q[1].tobytes() for p, q in zip(other[3], lists))


def test_entry_points_check_their_arguments(gpu):
    from superdsm_amd import _capi
    a, b = CATALOGUE['disc']
    raw = Raw(a, b)
    S = raw.S
    p = S._p(raw.d_cursor)
    assert S.L.sdsm_label_pixel_counts(1, 46341, p, p, p, S._stream()) != 0 and b'H * H + W * W < 2^31' in _capi.lib().sdsm_last_error()
    assert S.L.sdsm_label_pixel_lists(40000, 40000, p, p, p, p, p, S._stream()) != 0 and b'H * H + W * W < 2^31' in _capi.lib().sdsm_last_error()
    assert S.L.sdsm_pair_distances(64, 64, p, p, p, p, p, p, p, p, -1, p, 0, p, p, S._stream()) != 0
    assert S.L.sdsm_pair_distances(64, 64, p, p, p, p, p, p, p, p, 1, None, 0, p, p, S._stream()) != 0 and b'null' in _capi.lib().sdsm_last_error()
    assert S.L.sdsm_pair_distances(64, 64, None, None, None, None, None, None, None, None, 0, None, 0, None, None, S._stream()) == 0      # no pair: no launch
    table = (_capi.SetImage * 33)(*[_capi.SetImage(0, 1, 1)] * 33)
    assert S.L.sdsm_label_pixel_counts_multi(table, 33, p, p, p, S._stream()) != 0 and b'1 .. 32 images' in _capi.lib().sdsm_last_error()


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_results_against_an_expected_map(gpu):
    from superdsm_amd import boundary, render, testing
    rng = np.random.default_rng(9)
    from test_measure_cpu import ellipse
    shape = (90, 120)
    objs, moved = [], []
    for k in range(6):
        f = ellipse(rng, 12, erode=False)
        r0, c0 = 2 + 45 * (k // 3) + int(rng.integers(0, 4)), 2 + 38 * (k % 3) + int(rng.integers(0, 4))
        objs.append(testing.PostFragment((r0, c0), f))
        moved.append(testing.PostFragment((r0 + 1, c0 + 2), f))
    data, other = {'g_raw': np.zeros(shape), 'postprocessed_objects': objs}, {'g_raw': np.zeros(shape), 'postprocessed_objects': moved}
    expected = render.rasterize_labels(other)
    want = boundary.compare_boundaries_host(render.rasterize_labels(data), expected)
    assert want['n_expected'] == 6 and want['n_without_partner'] == 0 and want['mean_hausdorff'] > 0 and 0 < want['mean_nsd'] < 1
    same_scores(boundary.compare_result_boundaries(data, expected), want)
    same_scores(boundary.compare_result_boundaries(data, expected, objects=objs), want)
    both = boundary.compare_results_boundaries([data, other], [expected, expected])
    same_scores(both[0], want)
    assert both[1]['mean_hausdorff'] == 0.0 == both[1]['mean_nsd']


# 10 --------------------------------------------------------------------------------------------------------------------------------
def test_labels_out_of_range_found_on_the_device(gpu):
    from superdsm_amd import boundary
    a, b = CATALOGUE['disc']
    for v in (65536, -1, -2 ** 31, 2 ** 31 - 1):
        bad = a.copy()
        bad[5, 6] = bad[7, 8] = v
        with pytest.raises(ValueError, match=r'2 pixels of images \[1\] .* labels 0 .. 65535'):
            boundary.pair_distances_many([a, bad], [b, b])
        with pytest.raises(ValueError, match='labels 0 .. 65535'):
            boundary.pair_distances(a, bad, [(1, 1)])
        with pytest.raises(ValueError, match='labels 0 .. 65535'):
            boundary.label_boundaries(bad)
        with pytest.raises(ValueError, match='labels 0 .. 65535'):
            boundary.pair_distances_host(a, bad)
