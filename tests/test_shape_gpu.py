"""The GPU forms of the contour shape tables (sdsm_shape.hip) against the ``*_host`` definitions of superdsm_amd/shape.py: every field of
every row and the hull vertex lists byte for byte, on the smallest shapes at which the kernels can still go wrong -- rows that straddle
words, more rows than a band holds (254, and fewer for wide windows), more words than a column tile holds (126), frames and holes."""
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
    """Two results (table, offsets, vertices), byte for byte."""
    from superdsm_amd import shape as sh
    assert g[0].dtype == h[0].dtype == sh.TABLE_DTYPE and len(g[0]) == len(h[0]), what
    for name in sh.TABLE_DTYPE.names:
        if g[0][name].tobytes() != h[0][name].tobytes():
            k = int(np.nonzero(g[0][name] != h[0][name])[0][0])
            raise AssertionError(f'{what}: field {name} of row {k}: {g[0][name][k]!r} (GPU) != {h[0][name][k]!r} (host)')
    assert g[1].dtype == h[1].dtype == np.int64 and g[1].tobytes() == h[1].tobytes(), f'{what}: offsets'
    assert g[2].dtype == h[2].dtype == np.int32 and g[2].shape == h[2].shape and g[2].tobytes() == h[2].tobytes(), f'{what}: vertices'


def objects_gpu_raw(objects, shape, garbage_tails=False):
    """(table, offsets, vertices) of sdsm_shape_objects for ``objects``; ``garbage_tails``: the bits of every last word past h * w are set."""
    from superdsm_amd import shape as sh
    from superdsm_amd.postprocess import pack_fragments
    boxes, words, packed, _ = pack_fragments(objects)
    if garbage_tails:
        for b, bits in zip(boxes, packed):
            n = int(b[2]) * int(b[3])
            if n % 32:
                w = bits.view(np.uint32)
                w[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)
    recs, offsets, vertices = sh._ShapeSet([shape]).objects(np.zeros(len(boxes), np.int32), boxes, words, packed)
    return sh._table(np.arange(len(boxes)), recs), offsets, vertices


def filled_ellipse(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return ((y - (h - 1) / 2) / (h / 2)) ** 2 + ((x - (w - 1) / 2) / (w / 2)) ** 2 <= 1


def staircase(n=9):
    return np.tril(np.ones((n, n), bool))


def ring(n=11):
    f = np.ones((n, n), bool)
    f[3:n - 3, 3:n - 3] = False
    return f


CASES = {
    'single pixel': ([Obj((3, 4), np.ones((1, 1)))], (9, 9)),
    'horizontal lines': ([Obj((k, 2), np.ones((1, n))) for k, n in enumerate((1, 2, 32, 33, 65))], (8, 70)),
    'vertical lines': ([Obj((2, k), np.ones((n, 1))) for k, n in enumerate((1, 2, 32, 33, 65))], (70, 8)),
    'checkerboard 5 x 5': ([Obj((1, 1), np.indices((5, 5)).sum(axis=0) % 2 == 0)], (8, 8)),
    'staircase': ([Obj((0, 3), staircase())], (12, 14)),
    'ring with a hole': ([Obj((2, 2), ring())], (16, 16)),
    'fills its 7 x 9 image': ([Obj((0, 0), np.ones((7, 9)))], (7, 9)),
    '1 x 1 image': ([Obj((0, 0), np.ones((1, 1)))], (1, 1)),
    'ellipse 300 x 40': ([Obj((5, 7), filled_ellipse(300, 40))], (310, 60)),
    'ellipse 40 x 300': ([Obj((5, 7), filled_ellipse(40, 300))], (60, 310)),
    'two overlapping objects': ([Obj((2, 2), filled_ellipse(12, 17)), Obj((6, 9), filled_ellipse(15, 9))], (30, 30)),
    'empty fragment': ([Obj((1, 1), np.zeros((4, 37))), Obj((0, 0), np.ones((2, 2)))], (8, 40)),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_objects_equal_the_host_definition(gpu, name):
    from superdsm_amd import shape as sh
    objects, shape = CASES[name]
    host = sh.shape_objects_host(objects, shape)
    same(sh.shape_objects(objects, shape), host, name)
    if name == 'ring with a hole':
        assert host[0]['border_pixels'][0] == 40 + 20 and host[0]['hull_area2'][0] == 2 * 121         # the inner border counts, the hull ignores the hole
    if name == 'fills its 7 x 9 image':
        assert host[0]['flags'][0] == 1 and host[0]['n_vertices'][0] == 4
    if name == 'checkerboard 5 x 5':
        assert host[0]['perim_n1'][0] == 0 and host[0]['perim_n2'][0] + host[0]['perim_n3'][0] > 0   # diagonal-only classes
    if name == 'empty fragment':
        assert host[0][0].tobytes() == np.zeros(1, sh.TABLE_DTYPE).tobytes() and host[1].tolist() == [0, 0, 4]


@pytest.mark.parametrize('w', [1, 31, 32, 33, 65])
def test_fragment_rows_straddle_words_and_tail_bits_are_ignored(gpu, w):
    from superdsm_amd import shape as sh
    rng = np.random.default_rng(w)
    shape = (40, 100)
    objs = []
    for h in (1, 3, 7, 13):                                                  # h * w mostly no multiple of 32
        f = rng.random((h, w)) < 0.6
        objs.append(Obj((rng.integers(0, shape[0] - h + 1), rng.integers(0, shape[1] - w + 1)), f))
    host = sh.shape_objects_host(objs, shape)
    same(objects_gpu_raw(objs, shape, garbage_tails=True), host, f'width {w}, garbage tails')
    same(sh.shape_objects(objs, shape), host, f'width {w}')


@pytest.mark.parametrize('h,w,density', [(3, 4100, 0.5), (6, 4033, 0.9), (2, 8200, 0.3), (300, 70, 0.97)])
def test_column_tiles_and_short_bands(gpu, h, w, density):
    """Windows wider than a column tile (126 words = 4032 columns: a band is then a single row), in two and three tiles with a tile
    boundary inside a run of pixels, and a window of many bands of random bits."""
    from superdsm_amd import shape as sh
    rng = np.random.default_rng(h * w)
    f = rng.random((h, w)) < density
    f[:, 4020:4040] = True
    objs, shape = [Obj((1, 2), f)], (h + 2, w + 5)
    same(objects_gpu_raw(objs, shape, garbage_tails=True), sh.shape_objects_host(objs, shape), f'{h} x {w}')


def test_a_padded_box_gives_the_rows_of_the_tight_box(gpu):
    from superdsm_amd import shape as sh
    rng = np.random.default_rng(21)
    tight = ellipse(rng, 20)
    padded = np.zeros((tight.shape[0] + 5, tight.shape[1] + 37), bool)
    padded[2:2 + tight.shape[0], 33:33 + tight.shape[1]] = tight
    shape = (80, 120)
    a = sh.shape_objects([Obj((12, 43), tight)], shape)
    b = sh.shape_objects([Obj((10, 10), padded)], shape)
    same(a, b, 'tight against padded')
    same(a, sh.shape_objects_host([Obj((12, 43), tight)], shape), 'tight')


def test_random_ellipses_area_equals_measure_and_a_second_launch_gives_the_same_bytes(gpu):
    from superdsm_amd import measure, shape as sh
    rng = np.random.default_rng(31)
    shape = (120, 150)
    objs = []
    for _ in range(40):
        f = ellipse(rng, 25)
        objs.append(Obj((rng.integers(0, shape[0] - f.shape[0] + 1), rng.integers(0, shape[1] - f.shape[1] + 1)), f))
    first = sh.shape_objects(objs, shape)
    same(first, sh.shape_objects_host(objs, shape), 'ellipses')
    same(sh.shape_objects(objs, shape), first, 'second launch')
    assert (first[0]['area'] == measure.measure_objects(objs, shape)['area']).all()
    assert (first[0]['flags'] & 1 == measure.measure_objects_host(objs, shape)['flags'] & 1).all()


# ---- label form ------------------------------------------------------------------------------------------------------------------------
def test_labels_touching_absent_nested_and_another_background(gpu):
    from superdsm_amd import shape as sh
    touching = np.zeros((9, 40), np.int32)
    touching[1:6, 2:20], touching[1:8, 20:37], touching[6:8, 2:20] = 1, 2, 5          # 3 and 4 do not occur
    same(sh.shape_labels(touching), sh.shape_labels_host(touching), 'touching labels')
    kept = sh.shape_labels(touching, keep_absent=True)
    same(kept, sh.shape_labels_host(touching, keep_absent=True), 'absent labels')
    assert kept[0]['label'].tolist() == [0, 1, 2, 3, 4, 5] and kept[0]['area'].tolist() == [0, 90, 119, 0, 0, 36] and kept[0]['n_vertices'][3] == 0
    assert kept[0]['edges_c'][1] == 2 * 5                                             # the edge against label 2 counts
    nested = np.zeros((20, 22), np.int32)
    nested[2:18, 3:19] = 7                                                            # a ring ...
    nested[6:14, 7:15] = 0
    nested[8:12, 9:13] = 3                                                            # ... around a blob
    same(sh.shape_labels(nested), sh.shape_labels_host(nested), 'nested boxes')
    same(sh.shape_labels(nested, background_label=7), sh.shape_labels_host(nested, background_label=7), 'background 7')
    same(sh.shape_labels(nested, background_label=None), sh.shape_labels_host(nested, background_label=None), 'no background')
    wrapped = nested.astype(np.uint16)
    wrapped[wrapped == 0] = 65535
    same(sh.shape_labels(wrapped, background_label=65535), sh.shape_labels_host(wrapped, background_label=65535), 'background 65535')


def test_label_form_equals_the_object_form_for_exclusive_objects(gpu):
    from superdsm_amd import shape as sh
    rng = np.random.default_rng(41)
    labels = label_scene(rng, shape=(97, 131), n=20)
    by_label = sh.shape_labels(labels)
    same(by_label, sh.shape_labels_host(labels), 'label scene')
    objs = []
    for l in by_label[0]['label']:
        rr, cc = np.nonzero(labels == l)
        objs.append(Obj((rr.min(), cc.min()), (labels == l)[rr.min():rr.max() + 1, cc.min():cc.max() + 1]))
    by_object = sh.shape_objects(objs, labels.shape)
    by_object[0]['label'] = by_label[0]['label']
    same(by_object, by_label, 'objects against labels')


def test_label_limits_and_window_cap_raise(gpu, monkeypatch):
    from superdsm_amd import _capi, shape as sh
    with pytest.raises(ValueError, match='labels'):
        sh.shape_labels(np.array([[0, 3], [-1, 3]]))
    with pytest.raises(ValueError, match='labels'):
        sh.shape_labels(np.array([[0, 65536]]))
    with pytest.raises(TypeError):
        sh.shape_labels(np.zeros((3, 3)))
    with pytest.raises(ValueError):
        sh.shape_objects([Obj((3, 3), np.ones((2, 2)))], (4, 4))
    monkeypatch.setattr(_capi, 'SHAPE_MAX_WINDOW_WORDS', 3)
    with pytest.raises(ValueError, match='windows'):
        sh.shape_labels(np.arange(1, 201, dtype=np.int32).reshape(10, 20) // 50)


# ---- sets ------------------------------------------------------------------------------------------------------------------------------
def test_sets_equal_the_per_image_calls(gpu):
    from superdsm_amd import shape as sh
    rng = np.random.default_rng(51)
    shapes = [(60, 80), (33, 47), (90, 41)]
    per_image = [[], [], []]
    for i in (0, 2):                                                         # the second image has no objects
        for _ in range(6):
            f = ellipse(rng, 14)
            per_image[i].append(Obj((rng.integers(0, shapes[i][0] - f.shape[0] + 1), rng.integers(0, shapes[i][1] - f.shape[1] + 1)), f))
    many = sh.shape_objects_many(per_image, shapes)
    assert len(many) == 3 and len(many[1][0]) == 0 and many[1][1].tolist() == [0] and many[1][2].shape == (0, 2)
    for objs, s, m in zip(per_image, shapes, many):
        same(m, sh.shape_objects(objs, s), 'set against single call')
        same(m, sh.shape_objects_host(objs, s), 'set against host')
    maps = [label_scene(rng, shape=shapes[0], n=9), np.zeros(shapes[1], np.int32), label_scene(rng, shape=shapes[2], n=7)]
    many = sh.shape_labels_many(maps)
    for lab, m in zip(maps, many):
        same(m, sh.shape_labels(lab), 'label set against single call')
        same(m, sh.shape_labels_host(lab), 'label set against host')


def test_a_list_longer_than_a_set_is_split(gpu):
    from superdsm_amd import _capi, shape as sh
    rng = np.random.default_rng(61)
    n = _capi.MAX_SET_IMAGES + 3
    shapes = [(12 + k % 5, 15 + k % 7) for k in range(n)]
    per_image = [[Obj((k % 3, k % 4), rng.random((6, 9)) < 0.7)] for k in range(n)]
    many = sh.shape_objects_many(per_image, shapes)
    assert len(many) == n
    for objs, s, m in zip(per_image, shapes, many):
        same(m, sh.shape_objects_host(objs, s), 'split list')
    maps = [np.where(rng.random(s) < 0.5, 0, rng.integers(1, 4, s)).astype(np.int32) for s in shapes]
    for lab, m in zip(maps, sh.shape_labels_many(maps)):
        same(m, sh.shape_labels_host(lab), 'split list of label maps')


def test_result_of_pipeline_data(gpu):
    from superdsm_amd import shape as sh
    objs = [Obj((1, 1), filled_ellipse(9, 12)), Obj((4, 6), np.ones((3, 3)))]
    data = {'g_raw': np.zeros((20, 25)), 'postprocessed_objects': objs}
    same(sh.shape_result(data), sh.shape_objects_host(objs, (20, 25)), 'shape_result')
    d = sh.derive(*sh.shape_result(data, objs[1:]))[0]
    assert (d['perimeter'], d['min_feret_diameter'], d['solidity']) == (8.0, 3.0, 1.0)
