"""The GPU form of the contingency table (k_overlap_pairs, sdsm_measure.hip) against ``compare.overlap_pairs_host``, byte for byte, on
the smallest shapes at which the kernel can still go wrong: more pairs than any LDS table holds, unaligned rows, a tail band, sets,
a table that is too small, keys that share their low bits, negative labels, dirty buffers."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FREE = 0xffffffffffffffff


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    return torch.device('cuda', 0)


class Raw:
    """sdsm_overlap_pairs through the C ABI on buffers that live across calls."""

    def __init__(self, shape, capacity):
        import torch
        from superdsm_amd.render import _DeviceSet
        self.S, self.shape, self.capacity, self.torch = _DeviceSet([shape]), shape, capacity, torch
        self.d_keys = torch.empty(capacity, dtype=torch.int64, device=self.S.dev)
        self.d_counts = torch.empty(capacity, dtype=torch.int64, device=self.S.dev)
        self.d_status = torch.empty(2, dtype=torch.int32, device=self.S.dev)

    def dirty(self, byte):
        for t in (self.d_keys, self.d_counts, self.d_status):
            t.view(self.torch.uint8).fill_(byte)

    def __call__(self, a, b, capacity=None):
        S = self.S
        d_a, d_b = S.pack([a], np.int32), S.pack([b], np.int32)
        code = S.L.sdsm_overlap_pairs(self.shape[0], self.shape[1], S._p(d_a), S._p(d_b), self.capacity if capacity is None else capacity, S._p(self.d_keys),
                                      S._p(self.d_counts), S._p(self.d_status), S._stream())
        return code, self.d_keys.cpu().numpy().view(np.uint64), self.d_counts.cpu().numpy(), self.d_status.cpu().numpy()


def occupied(keys, counts):
    return {(int(k) >> 32, int(k) & 0xffffffff): int(n) for k, n in zip(keys, counts) if int(k) != FREE}


def truth(a, b):
    """{(a, b): pixels} over the pixels where both labels are >= 0."""
    ok = (a >= 0) & (b >= 0)
    k, n = np.unique((a[ok].astype(np.uint64) << np.uint64(32)) | b[ok].astype(np.uint64), return_counts=True)
    return {(int(x) >> 32, int(x) & 0xffffffff): int(c) for x, c in zip(k, n)}


def blobs(shape, side, shift=(0, 0), first=1):
    """Square blobs of ``side`` pixels with a background grid between them, moved by ``shift``."""
    r, c = np.mgrid[0:shape[0], 0:shape[1]]
    r, c = r + shift[0], c + shift[1]
    lab = first + (r // side) * (shape[1] // side + 2) + c // side
    lab[(r % side < 3) | (c % side < 2)] = 0
    return lab.astype(np.int32)


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_one_band_of_16384_distinct_pairs_goes_straight_to_the_global_table_and_grows_it(gpu):
    from superdsm_amd import compare
    rng = np.random.default_rng(1)
    a = 1 + np.arange(128 * 128, dtype=np.int32).reshape(128, 128)
    b = rng.integers(0, 64, a.shape).astype(np.int32)
    host = compare.overlap_pairs_host(a, b)
    assert len(host) == 16384
    info = {}
    got = compare.overlap_pairs(a, b, info=info)
    assert got.dtype == compare.PAIR_DTYPE and got.tobytes() == host.tobytes()
    assert compare.DEFAULT_CAPACITY < 32768 <= info['capacity'][0]


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_tail_band_unaligned_rows_and_runs_across_segments(gpu):
    from superdsm_amd import compare
    shape = (129, 131)                                                        # 16 899 pixels: one full band and 515 more
    a, b = blobs(shape, 40), blobs(shape, 33, (5, 7), 100)
    host = compare.overlap_pairs_host(a, b)
    assert host['count'].max() > 16 * 40 and len(host) > 30                   # runs longer than a segment, rows longer than one
    assert compare.overlap_pairs(a, b).tobytes() == host.tobytes()
    # a view with unaligned rows of an int64 map goes the same way
    wide = np.zeros((129, 140), np.int64)
    wide[:, 3:134] = a
    assert compare.overlap_pairs(wide[:, 3:134], b.astype(np.uint16)).tobytes() == host.tobytes()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_sets_equal_single_images_and_long_lists_are_split(gpu):
    from superdsm_amd import compare
    rng = np.random.default_rng(3)
    shapes = [(1, 1), (37, 53), (129, 131)]
    a_list = [blobs(s, 9) for s in shapes]
    b_list = [np.where(rng.random(s) < 0.9, blobs(s, 11, (2, 1), 50), 7).astype(np.int32) for s in shapes]
    many = compare.overlap_pairs_many(a_list, b_list)
    for a, b, got in zip(a_list, b_list, many):
        host = compare.overlap_pairs_host(a, b)
        assert got.tobytes() == host.tobytes() and compare.overlap_pairs(a, b).tobytes() == host.tobytes()
    a33 = [rng.integers(0, 4, (5 + k % 3, 6)).astype(np.int32) for k in range(33)]
    b33 = [rng.integers(0, 3, x.shape).astype(np.int32) for x in a33]
    info = {}
    got = compare.overlap_pairs_many(a33, b33, capacity=32, info=info)
    assert len(got) == 33 and info['capacity'] == [32] * 33
    for a, b, g in zip(a33, b33, got):
        assert g.tobytes() == compare.overlap_pairs_host(a, b).tobytes()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_full_table_is_reported_not_waited_on(gpu):
    from superdsm_amd import compare
    r, c = np.mgrid[0:16, 0:16]
    a = (1 + (r // 2) * 8 + c // 2).astype(np.int32)                          # 64 labels of 2 x 2 pixels
    b = ((r // 2 + c // 2) % 3).astype(np.int32)
    want = truth(a, b)
    assert len(want) == 64
    code, keys, counts, status = Raw(a.shape, 8)(a, b)
    assert code == 0 and status[0] == 0 and status[1] > 0
    got = occupied(keys, counts)
    assert len(got) == 8 and all(p in want and 0 < n <= want[p] for p, n in got.items())
    assert int(counts.sum()) == sum(got.values()) < a.size
    info = {}
    assert compare.overlap_pairs(a, b, capacity=8, info=info).tobytes() == compare.overlap_pairs_host(a, b).tobytes()
    assert info['capacity'] == [128]                                          # 64 pairs, at most half full


def test_entry_point_checks_its_arguments(gpu):
    from superdsm_amd import _capi
    a = np.zeros((4, 4), np.int32)
    raw = Raw(a.shape, 16)
    for capacity in (0, 12, -8):
        code, *_ = raw(a, a, capacity=capacity)
        assert code != 0 and b'capacity' in _capi.lib().sdsm_last_error()
    S = raw.S
    assert S.L.sdsm_overlap_pairs(65536, 32768, S._p(raw.d_keys), S._p(raw.d_keys), 16, S._p(raw.d_keys), S._p(raw.d_counts), S._p(raw.d_status), S._stream()) != 0
    assert b'H * W < 2^31' in _capi.lib().sdsm_last_error()
    table = (_capi.SetImage * 33)(*[_capi.SetImage(0, 1, 1)] * 33)
    off = (S.C.c_int64 * 33)(*range(33))
    cap = (S.C.c_int64 * 33)(*[1] * 33)
    assert S.L.sdsm_overlap_pairs_multi(table, 33, S._p(raw.d_keys), S._p(raw.d_keys), off, cap, S._p(raw.d_keys), S._p(raw.d_counts), S._p(raw.d_status),
                                        S._stream()) != 0
    assert b'1 .. 32 images' in _capi.lib().sdsm_last_error()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_keys_that_share_their_low_bits(gpu):
    from superdsm_amd import compare
    rng = np.random.default_rng(5)
    values = np.array([65536 * k for k in range(8)] + [2 ** 31 - 1], np.int64)
    a, b = values[rng.integers(0, 9, (32, 32))], values[rng.integers(0, 9, (32, 32))]
    host = compare.overlap_pairs_host(a, b)
    assert len(host) == 81 and host['a'].max() == 2 ** 31 - 1 == host['b'].max()
    assert compare.overlap_pairs(a, b).tobytes() == host.tobytes()
    assert compare.overlap_pairs(a.astype(np.uint32), b, capacity=1).tobytes() == host.tobytes()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_negative_labels_are_counted_skipped_and_refused(gpu):
    from superdsm_amd import compare
    rng = np.random.default_rng(6)
    a, b = blobs((40, 50), 8), blobs((40, 50), 7, (1, 2))
    a[rng.random(a.shape) < 0.02] = -1
    b[rng.random(b.shape) < 0.02] = -(2 ** 31)
    a[0, 0] = b[0, 0] = -5
    n_bad = int(((a < 0) | (b < 0)).sum())
    assert n_bad > 20
    code, keys, counts, status = Raw(a.shape, 1024)(a, b)
    assert code == 0 and status.tolist() == [n_bad, 0]
    assert occupied(keys, counts) == truth(a, b)
    with pytest.raises(ValueError, match=rf'{n_bad} pixels of images \[1\]'):
        compare.overlap_pairs_many([np.maximum(a, 0), a], [np.maximum(b, 0), b])


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_second_launch_into_dirtied_buffers_gives_the_same_bytes(gpu):
    a, b = blobs((70, 90), 12), blobs((70, 90), 10, (3, 4), 30)
    raw = Raw(a.shape, 512)
    raw.dirty(0xA5)
    code, keys, counts, status = raw(a, b)
    assert code == 0 and status.tolist() == [0, 0] and occupied(keys, counts) == truth(a, b)
    raw.dirty(0xA5)
    code2, keys2, counts2, status2 = raw(a, b)
    order, order2 = np.argsort(keys), np.argsort(keys2)
    assert code2 == 0 and keys[order].tobytes() == keys2[order2].tobytes() and counts[order].tobytes() == counts2[order2].tobytes()
    assert status2.tobytes() == status.tobytes() and int((keys != FREE).sum()) == len(truth(a, b))


# 8 ---------------------------------------------------------------------------------------------------------------------------------
class Obj:
    def __init__(self, offset, fragment):
        self.fg_offset, self.fg_fragment = np.asarray(offset, int), np.asarray(fragment, bool)


def layout_objects(shape, layout, shift=0):
    objs = []
    for e in layout:
        (cy, cx), (p, q) = e['centre'], e['axes']
        cx += shift
        R = int(math.ceil(max(p, q))) + 1
        r0, r1, c0, c1 = max(0, int(cy) - R), min(shape[0], int(cy) + R + 1), max(0, int(cx) - R), min(shape[1], int(cx) + R + 1)
        yy, xx = np.mgrid[r0:r1, c0:c1]
        ca, sa = math.cos(e['angle']), math.sin(e['angle'])
        u, v = (yy - cy) * ca + (xx - cx) * sa, -(yy - cy) * sa + (xx - cx) * ca
        objs.append(Obj((r0, c0), (u / p) ** 2 + (v / q) ** 2 <= 1))
    return objs


def same_scores(x, y):
    assert x.keys() == y.keys()
    for k in x:
        if isinstance(x[k], np.ndarray) and x[k].dtype.names:
            assert x[k].dtype == y[k].dtype and all(np.array_equal(x[k][f], y[k][f], equal_nan=x[k][f].dtype.kind == 'f') for f in x[k].dtype.names), k
        else:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=np.asarray(x[k]).dtype.kind == 'f'), k


def test_scores_of_the_gpu_table_equal_the_host_scores(gpu):
    from superdsm_amd import compare, render, synth
    spec = synth.WORKLOADS['synthetic256']
    layout = synth.random_layout(spec['shape'], spec['n'], spec['radius'], spec['seed'], min_sep=2.2)      # as testing.make_scene lays it out
    g = np.zeros(spec['shape'])
    data = {'g_raw': g, 'postprocessed_objects': layout_objects(spec['shape'], layout)}
    moved = {'g_raw': g, 'postprocessed_objects': layout_objects(spec['shape'], layout, shift=2)}
    actual, expected = render.rasterize_labels_gpu(data), render.rasterize_labels_gpu(moved)
    host = compare.compare_labels_host(actual, expected)
    got = compare.compare_labels(actual, expected)
    same_scores(got, host)
    assert 0.5 < host['seg'] < 1 and host['n_expected'] >= 5
    same_scores(compare.compare_result(data, expected), host)
    same_scores(compare.compare_results([data, moved], [expected, expected])[0], host)
    assert compare.compare_results([data, moved], [expected, expected])[1]['seg'] == 1.0
