"""The GPU forms of the texture tables (sdsm_texture.hip) against the ``*_host`` definitions of superdsm_amd/texture.py: every field of every
row, every pair count and every entry byte for byte, on the smallest inputs at which the kernel can still go wrong -- fragment rows that
straddle words with neighbour bits from the word before and the word after, the last cell and the last edge of the largest triangle, all
pairs in one cell, and launches into dirtied buffers after a launch with more levels."""
import numpy as np
import pytest

from test_measure_cpu import Obj, ellipse, label_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    return torch.device('cuda', 0)


def same(g, h, what=''):
    """Two results (table, pairs, entries), byte for byte."""
    from superdsm_amd import texture as tx
    for part, dtype, name in ((0, tx.TABLE_DTYPE, 'table'), (1, tx.PAIRS_DTYPE, 'pairs'), (2, tx.ENTRY_DTYPE, 'entries')):
        assert g[part].dtype == h[part].dtype == dtype and g[part].shape == h[part].shape, f'{what}: {name} {g[part].shape} (GPU) != {h[part].shape} (host)'
        for field in dtype.names:
            if g[part][field].tobytes() != h[part][field].tobytes():
                k = tuple(np.argwhere(g[part][field] != h[part][field])[0])
                raise AssertionError(f'{what}: field {field} of {name}{k}: {g[part][field][k]!r} (GPU) != {h[part][field][k]!r} (host)')


def compact(res):
    """``first`` is the running sum of ``n_entries``, and the keys are strictly ascending within each (k, o)."""
    _, pairs, entries = res
    flat = pairs.reshape(-1)
    assert flat['first'].tolist() == (np.cumsum(flat['n_entries']) - flat['n_entries']).tolist() and len(entries) == flat['n_entries'].sum()
    key = entries['i'].astype(np.int64) * 65536 + entries['j']
    for p in flat:
        k = key[int(p['first']):int(p['first']) + int(p['n_entries'])]
        assert (k[1:] > k[:-1]).all()
    assert (entries['i'] <= entries['j']).all() and (entries['count'] > 0).all()


def objects_gpu_raw(objects, shape, g, edges, offsets, garbage_tails=False, dirty=None):
    """(table, pairs, entries) of sdsm_texture_objects for ``objects``; ``garbage_tails``: the bits of every last word past h * w are set;
    ``dirty``: the byte the workspace and the three outputs are filled with before the launch."""
    from superdsm_amd import texture as tx
    from superdsm_amd.postprocess import pack_fragments
    boxes, words, packed, _ = pack_fragments(objects)
    if garbage_tails:
        for b, bits in zip(boxes, packed):
            n = int(b[2]) * int(b[3])
            if n % 32:
                w = bits.view(np.uint32)
                w[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)
    T = tx._TextureSet([shape], [np.ascontiguousarray(g, np.float64)], [tx.check_edges(edges)], tx.check_offsets(offsets))
    B = None
    if dirty is not None:
        B = T.buffers(len(boxes), int(T.slot_offsets(boxes)[-1]))
        for t in B.values():
            t.fill_(dirty)
    recs, pairs, entries = T.objects(np.zeros(len(boxes), np.int32), boxes, words, packed, B)
    return tx._table(np.arange(len(boxes)), recs), pairs, entries


# ---- fragment shapes -------------------------------------------------------------------------------------------------------------------
def test_one_pixel_two_pixels_an_empty_fragment_and_no_objects(gpu):
    from superdsm_amd import texture as tx
    g = np.arange(30.0).reshape(5, 6)
    edges = tx.uniform_edges(0, 30, 5)
    objs = [Obj((2, 2), np.ones((1, 1))), Obj((1, 1), np.ones((1, 2))), Obj((3, 0), np.ones((2, 1))), Obj((0, 0), np.zeros((3, 3))), Obj((4, 5), np.ones((1, 1)))]
    host = tx.texture_objects_host(objs, g.shape, g, edges)
    assert host[1]['n_pairs'].tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    res = tx.texture_objects(objs, g.shape, g, edges)
    same(res, host, 'tiny fragments')
    compact(res)
    none = tx.texture_objects([], g.shape, g, edges)
    same(none, tx.texture_objects_host([], g.shape, g, edges), 'no objects')
    assert none[1].shape == (0, 4) and len(none[2]) == 0


WORD_OFFSETS = [(0, 1), (0, 31), (0, 32), (1, -1), (1, -32)]


@pytest.mark.parametrize('w', [1, 31, 32, 33, 65])
def test_neighbour_bits_cross_word_boundaries_and_tail_bits_are_ignored(gpu, w):
    from superdsm_amd import texture as tx
    rng = np.random.default_rng(w)
    shape = (40, 100)
    g = rng.random(shape)
    g[rng.random(shape) < 0.02] = np.nan
    edges = tx.uniform_edges(0, 1, 7)
    objs = []
    for h in (1, 3, 7, 13):                                                  # h * w mostly no multiple of 32
        f = rng.random((h, w)) < 0.8
        objs.append(Obj((rng.integers(0, shape[0] - h + 1), rng.integers(0, shape[1] - w + 1)), f))
    objs.append(Obj((20, 30), np.ones((5, w))))
    host = tx.texture_objects_host(objs, shape, g, edges, WORD_OFFSETS)
    same(objects_gpu_raw(objs, shape, g, edges, WORD_OFFSETS, garbage_tails=True), host, f'width {w}, garbage tails')
    res = tx.texture_objects(objs, shape, g, edges, WORD_OFFSETS)
    same(res, host, f'width {w}')
    compact(res)
    both = [(0, -1), (0, -31), (0, -32), (-1, 1), (-1, 32)]                   # the same tables from the bits before
    neg = tx.texture_objects(objs, shape, g, edges, both)
    assert neg[1].tobytes() == res[1].tobytes() and neg[2].tobytes() == res[2].tobytes()


def test_a_padded_box_gives_the_rows_of_the_tight_box(gpu):
    from superdsm_amd import texture as tx
    rng = np.random.default_rng(21)
    tight = ellipse(rng, 20)
    padded = np.zeros((tight.shape[0] + 5, tight.shape[1] + 37), bool)
    padded[2:2 + tight.shape[0], 33:33 + tight.shape[1]] = tight
    shape = (80, 120)
    g = rng.random(shape)
    edges = tx.uniform_edges(0, 1, 16)
    offs = [(0, 1), (1, 1), (1, 0), (1, -1), (3, -7)]
    a = tx.texture_objects([Obj((12, 43), tight)], shape, g, edges, offs)
    same(a, tx.texture_objects([Obj((10, 10), padded)], shape, g, edges, offs), 'tight against padded')
    same(a, tx.texture_objects_host([Obj((12, 43), tight)], shape, g, edges, offs), 'tight')


def test_fragments_taller_and_wider_than_a_workgroup_pass_with_the_largest_row_offset(gpu):
    from superdsm_amd import texture as tx
    rng = np.random.default_rng(22)
    shape = (310, 320)
    g = rng.normal(size=shape)
    edges = tx.uniform_edges(-2, 2, 12)
    objs = [Obj((3, 5), rng.random((300, 70)) < 0.9), Obj((5, 10), rng.random((70, 300)) < 0.9)]
    offs = [(32, 0), (32, -5), (-32, 32), (0, 32), (1, 1)]
    res = tx.texture_objects(objs, shape, g, edges, offs)
    same(res, tx.texture_objects_host(objs, shape, g, edges, offs), '300 x 70 and 70 x 300')
    compact(res)


def test_an_offset_larger_than_the_fragment_and_an_object_in_the_image_corner(gpu):
    from superdsm_amd import texture as tx
    rng = np.random.default_rng(23)
    shape = (12, 40)
    g = rng.random(shape)
    edges = tx.uniform_edges(0, 1, 4)
    objs = [Obj((0, 0), np.ones((4, 5))), Obj((8, 35), np.ones((4, 5))), Obj((0, 35), np.ones((3, 5))), Obj((9, 0), np.ones((3, 33)))]
    offs = [(4, 0), (0, 5), (-4, -5), (32, 32), (-32, 1), (1, -32), (0, 32), (3, 4)]      # most point out of every box
    host = tx.texture_objects_host(objs, shape, g, edges, offs)
    assert (host[1]['n_entries'][:3, :7] == 0).all() and host[1]['n_pairs'][:, 7].tolist() == [1, 1, 0, 0]
    assert host[1]['n_pairs'][3].tolist() == [0, 3 * 28, 0, 0, 0, 2, 3, 0]            # the 3 x 33 box: (1, -32) and (0, 32) just fit
    assert (host[0]['flags'] == tx.FRAME).all()
    same(tx.texture_objects(objs, shape, g, edges, offs), host, 'corners')


# ---- levels ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('G', [1, 2, 64, 255, 256])
def test_level_counts(gpu, G):
    from superdsm_amd import texture as tx
    rng = np.random.default_rng(G)
    shape = (50, 60)
    g = rng.random(shape)
    edges = tx.uniform_edges(0, 1, G)
    objs = [Obj((rng.integers(0, 20), rng.integers(0, 20)), ellipse(rng, 12)) for _ in range(4)]
    res = tx.texture_objects(objs, shape, g, edges)
    same(res, tx.texture_objects_host(objs, shape, g, edges), f'{G} levels')
    compact(res)


def test_a_ramp_reaches_the_last_cell_and_the_last_edge(gpu):
    from superdsm_amd import texture as tx
    g = np.arange(512.0).reshape(16, 32)
    edges = np.arange(2.0, 512.0, 2.0)                                        # 255 edges: the level of v is v // 2
    objs = [Obj((0, 0), np.ones((16, 32)))]
    host = tx.texture_objects_host(objs, g.shape, g, edges, [(0, 1), (1, 0)])
    assert (host[0]['level_min'][0], host[0]['level_max'][0]) == (0, 255)
    assert tuple(host[2][host[1][0, 0]['n_entries'] - 1]) == (255, 255, 1) and tuple(host[2][0]) == (0, 0, 1)
    res = tx.texture_objects(objs, g.shape, g, edges, [(0, 1), (1, 0)])
    same(res, host, 'ramp')
    compact(res)


def test_values_on_below_and_above_an_edge_and_non_finite_pixels(gpu):
    from superdsm_amd import texture as tx
    tiny = 5e-324
    edges = np.array([-1.0, -tiny, 0.0, tiny, 0.1, 2.0 ** 40])
    vals = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), [-0.0, np.nan, np.inf, -np.inf, 1e300, -1e300]])
    rng = np.random.default_rng(5)
    g = rng.choice(vals, size=(24, 24))
    objs = [Obj((0, 0), np.ones((24, 24))), Obj((3, 4), ellipse(rng, 9, erode=False)), Obj((5, 5), np.ones((1, 1)))]
    g[5, 5] = np.nan
    host = tx.texture_objects_host(objs, g.shape, g, edges)
    assert host[0]['flags'].tolist()[0] == tx.FRAME | tx.NONFINITE_INSIDE and host[0]['flags'][2] == tx.NONFINITE_INSIDE | tx.NO_FINITE_PIXEL
    same(tx.texture_objects(objs, g.shape, g, edges), host, 'edge values')


# ---- contention and reuse ----------------------------------------------------------------------------------------------------------------
def test_a_flat_object_has_all_pairs_of_an_offset_in_one_cell(gpu):
    from superdsm_amd import texture as tx
    g = np.full((64, 64), 0.7)
    edges = tx.uniform_edges(0, 1, 256)
    objs = [Obj((0, 0), np.ones((64, 64)))]
    res = tx.texture_objects(objs, g.shape, g, edges)
    same(res, tx.texture_objects_host(objs, g.shape, g, edges), 'flat')
    assert res[1]['n_pairs'][0].tolist() == [4032, 3969, 4032, 3969] and res[2]['count'].tolist() == [4032, 3969, 4032, 3969]
    assert (res[2]['i'] == 179).all() and (res[2]['j'] == 179).all()


def test_two_overlapping_objects_are_each_measured_alone(gpu):
    from superdsm_amd import texture as tx
    rng = np.random.default_rng(31)
    g = rng.random((30, 30))
    edges = tx.uniform_edges(0, 1, 8)
    a, b = Obj((2, 2), np.ones((12, 14))), Obj((8, 9), rng.random((15, 13)) < 0.8)
    res = tx.texture_objects([a, b], g.shape, g, edges)
    same(res, tx.texture_objects_host([a, b], g.shape, g, edges), 'overlapping')
    alone = tx.texture_objects([b], g.shape, g, edges)
    assert alone[1]['n_pairs'].tolist() == res[1]['n_pairs'][1:].tolist()
    assert alone[2].tobytes() == res[2][int(res[1][1, 0]['first']):].tobytes()


def test_launches_into_dirtied_buffers_and_after_more_levels_give_the_same_bytes(gpu):
    from superdsm_amd import texture as tx
    rng = np.random.default_rng(32)
    shape = (64, 64)
    g = rng.random(shape)
    g[10, 10] = np.inf
    objs = [Obj((rng.integers(0, 30), rng.integers(0, 30)), ellipse(rng, 14)) for _ in range(5)] + [Obj((0, 0), np.zeros((3, 3)))]
    few, many = tx.uniform_edges(0, 1, 5), tx.uniform_edges(0, 1, 256)
    host_few, host_many = tx.texture_objects_host(objs, shape, g, few), tx.texture_objects_host(objs, shape, g, many)
    for dirty in (0xab, 0xff, 0x00):
        same(objects_gpu_raw(objs, shape, g, few, tx.DEFAULT_OFFSETS, dirty=dirty), host_few, f'buffers filled with {dirty:#x}')
    same(objects_gpu_raw(objs, shape, g, many, tx.DEFAULT_OFFSETS, dirty=0xcd), host_many, '256 levels')       # raises the dynamic LDS limit
    same(objects_gpu_raw(objs, shape, g, few, tx.DEFAULT_OFFSETS, dirty=0xcd), host_few, '5 levels after 256')
    same(objects_gpu_raw(objs, shape, g, many, tx.DEFAULT_OFFSETS), host_many, '256 levels again')


# ---- offsets -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offsets', [[(2, -3)], [(0, 1), (1, 1), (1, 0), (1, -1), (0, 2), (2, 2), (-2, 0), (5, -2)]])
def test_offset_lists_of_one_and_eight(gpu, offsets):
    from superdsm_amd import texture as tx
    rng = np.random.default_rng(len(offsets))
    shape = (50, 60)
    g = rng.gamma(2.0, size=shape)
    edges = tx.image_edges(g, 32)
    objs = [Obj((rng.integers(0, 20), rng.integers(0, 20)), ellipse(rng, 12)) for _ in range(6)]
    res = tx.texture_objects(objs, shape, g, edges, offsets)
    assert res[1].shape == (6, len(offsets))
    same(res, tx.texture_objects_host(objs, shape, g, edges, offsets), f'{len(offsets)} offsets')
    compact(res)


# ---- label form ------------------------------------------------------------------------------------------------------------------------
def test_labels_touching_absent_nested_and_another_background(gpu):
    from superdsm_amd import texture as tx
    rng = np.random.default_rng(41)
    touching = np.zeros((9, 40), np.int32)
    touching[1:6, 2:20], touching[1:8, 20:37], touching[6:8, 2:20] = 1, 2, 5          # 3 and 4 do not occur
    g = rng.random(touching.shape)
    g[2, 3] = np.nan
    edges = tx.uniform_edges(0, 1, 6)
    res = tx.texture_labels(touching, g, edges)
    same(res, tx.texture_labels_host(touching, g, edges), 'touching labels')
    assert res[1]['n_pairs'][0, 0] == 5 * 17 - 2 and res[1]['n_pairs'][0, 2] == 4 * 18 - 2     # no pair across 1 | 2 or 1 / 5
    kept = tx.texture_labels(touching, g, edges, keep_absent=True)
    same(kept, tx.texture_labels_host(touching, g, edges, keep_absent=True), 'absent labels')
    assert kept[0]['label'].tolist() == [0, 1, 2, 3, 4, 5] and kept[0]['area'].tolist() == [0, 90, 119, 0, 0, 36] and kept[0]['n_finite'][1] == 89
    compact(kept)
    nested = np.zeros((20, 22), np.int32)
    nested[2:18, 3:19] = 7                                                            # a ring ...
    nested[6:14, 7:15] = 0
    nested[8:12, 9:13] = 3                                                            # ... around a blob
    g = rng.random(nested.shape)
    same(tx.texture_labels(nested, g, edges), tx.texture_labels_host(nested, g, edges), 'nested boxes')
    same(tx.texture_labels(nested, g, edges, background_label=7), tx.texture_labels_host(nested, g, edges, background_label=7), 'background 7')
    same(tx.texture_labels(nested, g, edges, background_label=None), tx.texture_labels_host(nested, g, edges, background_label=None), 'no background')


def test_label_form_equals_the_object_form_for_exclusive_objects(gpu):
    from superdsm_amd import texture as tx
    rng = np.random.default_rng(42)
    labels = label_scene(rng, shape=(97, 131), n=20)
    g = rng.gamma(2.0, size=labels.shape)
    edges = tx.image_edges(g, 16)
    by_label = tx.texture_labels(labels, g, edges)
    same(by_label, tx.texture_labels_host(labels, g, edges), 'label scene')
    objs = []
    for l in by_label[0]['label']:
        rr, cc = np.nonzero(labels == l)
        objs.append(Obj((rr.min(), cc.min()), (labels == l)[rr.min():rr.max() + 1, cc.min():cc.max() + 1]))
    by_object = tx.texture_objects(objs, labels.shape, g, edges)
    by_object[0]['label'] = by_label[0]['label']
    same(by_object, by_label, 'objects against labels')


def test_limits_and_caps_raise_before_a_launch(gpu, monkeypatch):
    from superdsm_amd import _capi, texture as tx
    g = np.zeros((2, 2))
    with pytest.raises(ValueError, match='labels'):
        tx.texture_labels(np.array([[0, 3], [-1, 3]]), g, [0.5])
    with pytest.raises(ValueError, match='labels'):
        tx.texture_labels(np.array([[0, 65536]]), np.zeros((1, 2)), [0.5])
    with pytest.raises(TypeError):
        tx.texture_labels(np.zeros((2, 2)), g, [0.5])
    with pytest.raises(ValueError):
        tx.texture_objects([Obj((3, 3), np.ones((2, 2)))], (4, 4), np.zeros((4, 4)), [0.5])
    lab = np.arange(1, 201, dtype=np.int32).reshape(10, 20) // 50
    monkeypatch.setattr(_capi, 'TEXTURE_MAX_SLOTS', 30)                       # 4 offsets * min(h * w, 3 cells) of the labels 1 .. 4: 40 entries
    with pytest.raises(ValueError, match='entries'):
        tx.texture_labels(lab, np.zeros((10, 20)), [0.5])
    with pytest.raises(ValueError, match='entries'):
        tx.texture_objects([Obj((0, 0), np.ones((2, 2)))] * 3, (4, 4), np.zeros((4, 4)), [0.5])      # 3 * 4 * 3 = 36
    assert len(tx.texture_objects([Obj((0, 0), np.ones((2, 2)))] * 2, (4, 4), np.zeros((4, 4)), [0.5])[0]) == 2
    monkeypatch.setattr(_capi, 'SHAPE_MAX_WINDOW_WORDS', 3)
    with pytest.raises(ValueError, match='windows'):
        tx.texture_labels(lab, np.zeros((10, 20)), [0.5])


# ---- sets ------------------------------------------------------------------------------------------------------------------------------
def test_sets_with_different_shapes_and_edges_equal_the_per_image_calls(gpu):
    from superdsm_amd import texture as tx
    rng = np.random.default_rng(51)
    shapes = [(60, 80), (33, 47), (90, 41)]
    gs = [rng.normal(size=s) * (k + 1) + k for k, s in enumerate(shapes)]
    edges = [tx.image_edges(g, 12) for g in gs]                              # different edges per image
    assert edges[0].tolist() != edges[2].tolist()
    per_image = [[], [], []]
    for i in (0, 2):                                                         # the second image has no objects
        for _ in range(6):
            f = ellipse(rng, 14)
            per_image[i].append(Obj((rng.integers(0, shapes[i][0] - f.shape[0] + 1), rng.integers(0, shapes[i][1] - f.shape[1] + 1)), f))
    many = tx.texture_objects_many(per_image, shapes, gs, edges)
    assert len(many) == 3 and len(many[1][0]) == 0 and many[1][1].shape == (0, 4) and len(many[1][2]) == 0
    for objs, s, g, e, m in zip(per_image, shapes, gs, edges, many):
        same(m, tx.texture_objects(objs, s, g, e), 'set against single call')
        same(m, tx.texture_objects_host(objs, s, g, e), 'set against host')
        compact(m)
    maps = [label_scene(rng, shape=shapes[0], n=9), np.zeros(shapes[1], np.int32), label_scene(rng, shape=shapes[2], n=7)]
    for lab, g, e, m in zip(maps, gs, edges, tx.texture_labels_many(maps, gs, edges)):
        same(m, tx.texture_labels(lab, g, e), 'label set against single call')
        same(m, tx.texture_labels_host(lab, g, e), 'label set against host')


def test_a_list_longer_than_a_set_is_split(gpu):
    from superdsm_amd import _capi, texture as tx
    rng = np.random.default_rng(61)
    n = _capi.MAX_SET_IMAGES + 1
    shapes = [(12 + k % 5, 15 + k % 7) for k in range(n)]
    gs = [rng.random(s) for s in shapes]
    edges = [tx.uniform_edges(0, 1 + k, 4) for k in range(n)]
    per_image = [[Obj((k % 3, k % 4), rng.random((6, 9)) < 0.7)] for k in range(n)]
    many = tx.texture_objects_many(per_image, shapes, gs, edges)
    assert len(many) == n
    for objs, s, g, e, m in zip(per_image, shapes, gs, edges, many):
        same(m, tx.texture_objects_host(objs, s, g, e), 'split list')
    maps = [np.where(rng.random(s) < 0.5, 0, rng.integers(1, 4, s)).astype(np.int32) for s in shapes]
    for lab, g, e, m in zip(maps, gs, edges, tx.texture_labels_many(maps, gs, edges)):
        same(m, tx.texture_labels_host(lab, g, e), 'split list of label maps')


def test_result_of_pipeline_data(gpu):
    from superdsm_amd import texture as tx
    rng = np.random.default_rng(71)
    objs = [Obj((1, 1), np.ones((9, 12))), Obj((4, 6), np.ones((3, 3)))]
    data = {'g_raw': rng.random((20, 25)), 'postprocessed_objects': objs}
    res = tx.texture_result(data, levels=16)
    same(res, tx.texture_objects_host(objs, (20, 25), data['g_raw'], tx.image_edges(data['g_raw'], 16)), 'texture_result')
    flat = np.full((20, 25), 2.5)
    d = tx.derive(*tx.texture_result(data, objs[1:], flat, edges=[1.0, 2.0, 3.0], offsets=[(0, 1)]), offsets=[(0, 1)])[0, 0]
    assert (d['n_pairs'], d['asm'], d['entropy'], d['contrast'], d['mean']) == (6, 1.0, 0.0, 0.0, 2.0)
