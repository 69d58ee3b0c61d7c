"""The GPU forms of the intensity distribution tables (sdsm_intensity.hip) against the ``*_host`` definitions of superdsm_amd/intensity.py:
every field of every row and every order statistic byte for byte, on the smallest inputs at which the kernel can still go wrong -- keys
that differ only in their first or their last radix digit, ties across a rank, fragment rows that straddle words, and objects at, above
and apparently above the number of keys that LDS holds."""
import numpy as np
import pytest

from test_intensity_cpu import VALUE_CASES, QUANTILES, Obj, object_of_values
from test_measure_cpu import ellipse, label_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    return torch.device('cuda', 0)


def same(g, h, what=''):
    """Two results (table, order), byte for byte."""
    from superdsm_amd import intensity as it
    assert g[0].dtype == h[0].dtype == it.TABLE_DTYPE and len(g[0]) == len(h[0]), what
    for name in it.TABLE_DTYPE.names:
        if g[0][name].tobytes() != h[0][name].tobytes():
            k = int(np.nonzero(g[0][name].view(np.uint8).reshape(len(g[0]), -1) != h[0][name].view(np.uint8).reshape(len(g[0]), -1))[0][0])
            raise AssertionError(f'{what}: field {name} of row {k}: {g[0][name][k]!r} (GPU) != {h[0][name][k]!r} (host)')
    assert g[1].dtype == h[1].dtype == np.float64 and g[1].shape == h[1].shape, f'{what}: order {g[1].shape} != {h[1].shape}'
    if g[1].tobytes() != h[1].tobytes():
        k = np.argwhere(g[1].view(np.uint64) != h[1].view(np.uint64))[0]
        raise AssertionError(f'{what}: order{tuple(k)}: {g[1][tuple(k)]!r} (GPU) != {h[1][tuple(k)]!r} (host)')


def objects_gpu_raw(objects, shape, g, quantiles, garbage_tails=False, dirty=None):
    """(table, order) of sdsm_intensity_objects for ``objects``; ``garbage_tails``: the bits of every last word past h * w are set;
    ``dirty``: the byte both outputs are filled with before the launch."""
    from superdsm_amd import intensity as it
    from superdsm_amd.postprocess import pack_fragments
    boxes, words, packed, _ = pack_fragments(objects)
    if garbage_tails:
        for b, bits in zip(boxes, packed):
            n = int(b[2]) * int(b[3])
            if n % 32:
                w = bits.view(np.uint32)
                w[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)
    fracs = it.quantile_fractions(quantiles)
    I = it._IntensitySet([shape], [np.ascontiguousarray(g, np.float64)])
    B = None
    if dirty is not None:
        B = I.buffers(len(boxes), len(fracs))
        B['d_out'].fill_(dirty)
        B['d_order'].view(I.S.torch.uint8).fill_(dirty)
    recs, order = I.objects(np.zeros(len(boxes), np.int32), boxes, words, packed, fracs, B)
    return it._table(np.arange(len(boxes)), recs), order


# ---- values --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(VALUE_CASES))
def test_value_cases_equal_the_host_definition(gpu, name):
    from superdsm_amd import intensity as it
    objs, g = object_of_values(VALUE_CASES[name], (64, 64))
    host = it.intensity_objects_host(objs, (64, 64), g, QUANTILES)
    same(it.intensity_objects(objs, (64, 64), g, QUANTILES), host, name)


def bits_to_double(bits):
    return np.array(bits, np.uint64).view(np.float64)


RADIX_CASES = {
    # keys that differ only in the lowest byte: every round but the last sees one bin
    'lowest byte': bits_to_double([0x3ff0000000000000 + k for k in (7, 3, 200, 255, 0, 3, 91, 128, 127)]),
    # keys that differ only in the sign or the top byte: the first round decides
    'sign and top byte': bits_to_double([0x3ff0000000000000, 0xbff0000000000000, 0x7fe0000000000000, 0xffe0000000000000, 0x0010000000000000,
                                         0x8010000000000000, 0x4000000000000000, 0xc000000000000000]),
    # lo and hi of the median in different top-digit bins: -1 and +1 around an even count
    'ranks in two top bins': np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]),
    'every byte differs': bits_to_double([0x0123456789abcdef, 0x4123456789abcdef, 0x4123456789abcdee, 0x4122456789abcdef, 0x412345678aabcdef,
                                          0xc123456789abcdef, 0x4123456789abcdef]),
}


@pytest.mark.parametrize('name', sorted(RADIX_CASES))
def test_first_and_last_radix_round(gpu, name):
    from superdsm_amd import intensity as it
    objs, g = object_of_values(RADIX_CASES[name], (64, 64))
    host = it.intensity_objects_host(objs, (64, 64), g, QUANTILES)
    same(it.intensity_objects(objs, (64, 64), g, QUANTILES), host, name)
    if name == 'ranks in two top bins':
        assert host[1][0, QUANTILES.index(0.5)].tolist() == [-1.0, 1.0]


@pytest.mark.parametrize('w', [1, 31, 32, 33, 65])
def test_fragment_rows_straddle_words_and_tail_bits_are_ignored(gpu, w):
    from superdsm_amd import intensity as it
    rng = np.random.default_rng(w)
    shape = (40, 100)
    g = rng.normal(size=shape)
    g[rng.random(shape) < 0.02] = np.nan
    objs = []
    for h in (1, 3, 7, 13):                                                  # h * w mostly no multiple of 32
        f = rng.random((h, w)) < 0.6
        objs.append(Obj((rng.integers(0, shape[0] - h + 1), rng.integers(0, shape[1] - w + 1)), f))
    host = it.intensity_objects_host(objs, shape, g)
    same(objects_gpu_raw(objs, shape, g, it.DEFAULT_QUANTILES, garbage_tails=True), host, f'width {w}, garbage tails')
    same(it.intensity_objects(objs, shape, g), host, f'width {w}')


def test_a_padded_box_gives_the_rows_of_the_tight_box(gpu):
    from superdsm_amd import intensity as it
    rng = np.random.default_rng(21)
    tight = ellipse(rng, 20)
    padded = np.zeros((tight.shape[0] + 5, tight.shape[1] + 37), bool)
    padded[2:2 + tight.shape[0], 33:33 + tight.shape[1]] = tight
    shape = (80, 120)
    g = rng.random(shape)
    a = it.intensity_objects([Obj((12, 43), tight)], shape, g)
    same(a, it.intensity_objects([Obj((10, 10), padded)], shape, g), 'tight against padded')
    same(a, it.intensity_objects_host([Obj((12, 43), tight)], shape, g), 'tight')


# ---- the key cap ---------------------------------------------------------------------------------------------------------------------
def test_objects_at_above_and_apparently_above_the_key_cap(gpu):
    """Exactly SDSM_INTENSITY_LDS_KEYS finite pixels (staged), one more (65 x 64 minus pixels: every round re-reads the image), and more
    pixels than the cap of which only the cap are finite (still staged).  All three in one launch, with ties and a MAD that needs them."""
    from superdsm_amd import _capi, intensity as it
    cap = _capi.INTENSITY_LDS_KEYS
    assert cap == 4096
    rng = np.random.default_rng(7)
    shape = (70, 200)
    g = np.round(rng.normal(size=shape) * 40) / 8                            # many ties
    full = np.ones((65, 64), bool)
    at_cap = full.copy()
    at_cap.reshape(-1)[rng.choice(65 * 64, 65 * 64 - cap, replace=False)] = False
    above = full.copy()
    above.reshape(-1)[rng.choice(65 * 64, 65 * 64 - cap - 1, replace=False)] = False
    objs = [Obj((1, 2), at_cap), Obj((3, 66), above), Obj((5, 131), full)]
    block = np.zeros(65 * 64, bool)
    block[rng.choice(65 * 64, 65 * 64 - cap, replace=False)] = True
    holes = np.zeros(shape, bool)
    holes[5:70, 131:195] = block.reshape(65, 64)
    g[holes] = np.where(rng.random(int(holes.sum())) < 0.5, np.nan, np.inf)
    host = it.intensity_objects_host(objs, shape, g, QUANTILES)
    assert host[0]['n_finite'].tolist() == [cap, cap + 1, cap] and host[0]['area'].tolist() == [cap, cap + 1, 65 * 64]
    same(it.intensity_objects(objs, shape, g, QUANTILES), host, 'key cap')


def test_an_object_beyond_the_cap_with_continuous_values(gpu):
    from superdsm_amd import intensity as it
    rng = np.random.default_rng(8)
    shape = (90, 100)
    g = 1e6 + 1e-6 * rng.random(shape)
    objs = [Obj((2, 3), rng.random((80, 90)) < 0.8)]
    same(it.intensity_objects(objs, shape, g), it.intensity_objects_host(objs, shape, g), 'beyond the cap')


# ---- quantile lists ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('quantiles', [(0.5,), (0.0, 0.1, 0.25, 1 / 3, 0.5, 0.75, 0.999999, 1.0), ()])
def test_quantile_lists_of_one_and_eight(gpu, quantiles):
    from superdsm_amd import intensity as it
    rng = np.random.default_rng(len(quantiles))
    shape = (50, 60)
    g = rng.normal(size=shape) * 10 ** rng.integers(-3, 4, shape).astype(float)
    objs = [Obj((rng.integers(0, 20), rng.integers(0, 20)), ellipse(rng, 12)) for _ in range(6)]
    host = it.intensity_objects_host(objs, shape, g, quantiles)
    assert host[1].shape == (6, len(quantiles), 2)
    same(it.intensity_objects(objs, shape, g, quantiles), host, f'{len(quantiles)} quantiles')


def test_mad_with_subnormal_inputs_is_not_contracted(gpu):
    """med = 0.5 * v_lo + 0.5 * v_hi in units t of the smallest subnormal: each product rounds (ties to even) before the sum.  With the
    middle pair (1 t, 2 t) the products are 0 and 1 t, med = 1 t; fma(0.5, 1 t, 1 t) rounds 1.5 t to 2 t.  With (2 t, 3 t) they are
    1 t and 2 t, med = 3 t; fma(0.5, 3 t, 1 t) rounds 2.5 t to 2 t.  Either contraction changes the MAD pair."""
    from superdsm_amd import intensity as it
    t = 5e-324
    for vals, med, mad in (([0, 1 * t, 2 * t, 9 * t], 1 * t, (1 * t, 1 * t)), ([0, 2 * t, 3 * t, 9 * t], 3 * t, (1 * t, 3 * t))):
        objs, g = object_of_values(np.array(vals), (64, 64))
        host = it.intensity_objects_host(objs, (64, 64), g)
        assert 0.5 * host[0]['med_lo'][0] + 0.5 * host[0]['med_hi'][0] == med
        assert (host[0]['mad_lo'][0], host[0]['mad_hi'][0]) == mad
        same(it.intensity_objects(objs, (64, 64), g), host, f'subnormal MAD, med = {med / t} t')


def test_a_second_launch_into_dirtied_outputs_gives_the_same_bytes(gpu):
    from superdsm_amd import intensity as it
    rng = np.random.default_rng(31)
    shape = (64, 64)
    g = rng.normal(size=shape)
    g[10, 10] = np.inf
    objs = [Obj((rng.integers(0, 30), rng.integers(0, 30)), ellipse(rng, 14)) for _ in range(5)] + [Obj((0, 0), np.zeros((3, 3)))]
    host = it.intensity_objects_host(objs, shape, g)
    for dirty in (0xab, 0xff, 0x00):
        same(objects_gpu_raw(objs, shape, g, it.DEFAULT_QUANTILES, dirty=dirty), host, f'outputs filled with {dirty:#x}')


# ---- label form ------------------------------------------------------------------------------------------------------------------------
def test_labels_touching_absent_nested_and_another_background(gpu):
    from superdsm_amd import intensity as it
    rng = np.random.default_rng(41)
    touching = np.zeros((9, 40), np.int32)
    touching[1:6, 2:20], touching[1:8, 20:37], touching[6:8, 2:20] = 1, 2, 5          # 3 and 4 do not occur
    g = rng.normal(size=touching.shape)
    g[2, 3] = np.nan
    same(it.intensity_labels(touching, g), it.intensity_labels_host(touching, g), 'touching labels')
    kept = it.intensity_labels(touching, g, keep_absent=True)
    same(kept, it.intensity_labels_host(touching, g, keep_absent=True), 'absent labels')
    assert kept[0]['label'].tolist() == [0, 1, 2, 3, 4, 5] and kept[0]['area'].tolist() == [0, 90, 119, 0, 0, 36] and kept[0]['n_finite'][1] == 89
    nested = np.zeros((20, 22), np.int32)
    nested[2:18, 3:19] = 7                                                            # a ring ...
    nested[6:14, 7:15] = 0
    nested[8:12, 9:13] = 3                                                            # ... around a blob
    g = rng.normal(size=nested.shape)
    same(it.intensity_labels(nested, g), it.intensity_labels_host(nested, g), 'nested boxes')
    same(it.intensity_labels(nested, g, background_label=7), it.intensity_labels_host(nested, g, background_label=7), 'background 7')
    same(it.intensity_labels(nested, g, background_label=None), it.intensity_labels_host(nested, g, background_label=None), 'no background')


def test_label_form_equals_the_object_form_for_exclusive_objects(gpu):
    from superdsm_amd import intensity as it
    rng = np.random.default_rng(42)
    labels = label_scene(rng, shape=(97, 131), n=20)
    g = rng.gamma(2.0, size=labels.shape)
    by_label = it.intensity_labels(labels, g, QUANTILES)
    same(by_label, it.intensity_labels_host(labels, g, QUANTILES), 'label scene')
    objs = []
    for l in by_label[0]['label']:
        rr, cc = np.nonzero(labels == l)
        objs.append(Obj((rr.min(), cc.min()), (labels == l)[rr.min():rr.max() + 1, cc.min():cc.max() + 1]))
    by_object = it.intensity_objects(objs, labels.shape, g, QUANTILES)
    by_object[0]['label'] = by_label[0]['label']
    same(by_object, by_label, 'objects against labels')


def test_label_limits_and_window_cap_raise(gpu, monkeypatch):
    from superdsm_amd import _capi, intensity as it
    g = np.zeros((2, 2))
    with pytest.raises(ValueError, match='labels'):
        it.intensity_labels(np.array([[0, 3], [-1, 3]]), g)
    with pytest.raises(ValueError, match='labels'):
        it.intensity_labels(np.array([[0, 65536]]), np.zeros((1, 2)))
    with pytest.raises(TypeError):
        it.intensity_labels(np.zeros((2, 2)), g)
    with pytest.raises(ValueError):
        it.intensity_objects([Obj((3, 3), np.ones((2, 2)))], (4, 4), np.zeros((4, 4)))
    with pytest.raises(ValueError, match='intensity'):
        it.intensity_objects([Obj((0, 0), np.ones((2, 2)))], (4, 4), None)
    monkeypatch.setattr(_capi, 'SHAPE_MAX_WINDOW_WORDS', 3)
    with pytest.raises(ValueError, match='windows'):
        it.intensity_labels(np.arange(1, 201, dtype=np.int32).reshape(10, 20) // 50, np.zeros((10, 20)))


# ---- sets ------------------------------------------------------------------------------------------------------------------------------
def test_sets_equal_the_per_image_calls(gpu):
    from superdsm_amd import intensity as it
    rng = np.random.default_rng(51)
    shapes = [(60, 80), (33, 47), (90, 41)]
    gs = [rng.normal(size=s) for s in shapes]
    per_image = [[], [], []]
    for i in (0, 2):                                                         # the second image has no objects
        for _ in range(6):
            f = ellipse(rng, 14)
            per_image[i].append(Obj((rng.integers(0, shapes[i][0] - f.shape[0] + 1), rng.integers(0, shapes[i][1] - f.shape[1] + 1)), f))
    many = it.intensity_objects_many(per_image, shapes, gs)
    assert len(many) == 3 and len(many[1][0]) == 0 and many[1][1].shape == (0, 3, 2)
    for objs, s, g, m in zip(per_image, shapes, gs, many):
        same(m, it.intensity_objects(objs, s, g), 'set against single call')
        same(m, it.intensity_objects_host(objs, s, g), 'set against host')
    maps = [label_scene(rng, shape=shapes[0], n=9), np.zeros(shapes[1], np.int32), label_scene(rng, shape=shapes[2], n=7)]
    for lab, g, m in zip(maps, gs, it.intensity_labels_many(maps, gs)):
        same(m, it.intensity_labels(lab, g), 'label set against single call')
        same(m, it.intensity_labels_host(lab, g), 'label set against host')


def test_a_list_longer_than_a_set_is_split(gpu):
    from superdsm_amd import _capi, intensity as it
    rng = np.random.default_rng(61)
    n = _capi.MAX_SET_IMAGES + 1
    shapes = [(12 + k % 5, 15 + k % 7) for k in range(n)]
    gs = [rng.normal(size=s) for s in shapes]
    per_image = [[Obj((k % 3, k % 4), rng.random((6, 9)) < 0.7)] for k in range(n)]
    many = it.intensity_objects_many(per_image, shapes, gs)
    assert len(many) == n
    for objs, s, g, m in zip(per_image, shapes, gs, many):
        same(m, it.intensity_objects_host(objs, s, g), 'split list')
    maps = [np.where(rng.random(s) < 0.5, 0, rng.integers(1, 4, s)).astype(np.int32) for s in shapes]
    for lab, g, m in zip(maps, gs, it.intensity_labels_many(maps, gs)):
        same(m, it.intensity_labels_host(lab, g), 'split list of label maps')


def test_result_of_pipeline_data(gpu):
    from superdsm_amd import intensity as it
    rng = np.random.default_rng(71)
    objs = [Obj((1, 1), np.ones((9, 12))), Obj((4, 6), np.ones((3, 3)))]
    data = {'g_raw': rng.random((20, 25)), 'postprocessed_objects': objs}
    same(it.intensity_result(data), it.intensity_objects_host(objs, (20, 25), data['g_raw']), 'intensity_result')
    flat = np.full((20, 25), 2.5)
    d = it.derive(*it.intensity_result(data, objs[1:], flat))[0]
    assert (d['std_intensity'], d['median'], d['mad'], d['iqr'], d['mean_intensity']) == (0.0, 2.5, 0.0, 0.0, 2.5)
