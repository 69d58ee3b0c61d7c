"""The GPU forms of the measurement tables (sdsm_measure.hip) against the ``*_host`` definitions of superdsm_amd/measure.py: every
integer field, limb, flag, box and min / max byte for byte, on the smallest shapes at which the kernels can still go wrong."""
import numpy as np
import pytest

from test_measure_cpu import Obj, ellipse, label_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    return torch.device('cuda', 0)


def same_bytes(a, b, what=''):
    from superdsm_amd import _capi
    assert len(a) == len(b), what
    for name in _capi.MEASURE_RECORD_DTYPE.names:
        if a[name].tobytes() != b[name].tobytes():
            k = int(np.nonzero(a[name].view(np.uint64 if a[name].dtype.itemsize == 8 else np.uint32) != b[name].view(np.uint64 if a[name].dtype.itemsize == 8 else np.uint32))[0][0])
            raise AssertionError(f'{what}: field {name} of row {k}: {a[name][k]!r} (GPU) != {b[name][k]!r} (host)')


def objects_gpu_raw(objects, shape, g, garbage_tails=False):
    """The records of sdsm_measure_objects for ``objects``; ``garbage_tails``: the bits of every last word past h * w are set."""
    from superdsm_amd import measure
    from superdsm_amd.postprocess import pack_fragments
    boxes, words, packed, _ = pack_fragments(objects)
    if garbage_tails:
        for b, bits in zip(boxes, packed):
            n = int(b[2]) * int(b[3])
            if n % 32:
                w = bits.view(np.uint32)
                w[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)
    M = measure._MeasureSet([shape], [g] if g is not None else None)
    return M.objects(np.zeros(len(boxes), np.int32), boxes, words, packed)


# ---- fragments (1a) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w', [1, 31, 32, 33, 65])
def test_fragment_rows_straddle_words_and_tail_bits_are_ignored(gpu, w):
    from superdsm_amd import measure
    rng = np.random.default_rng(w)
    shape = (40, 100)
    g = rng.normal(size=shape) * 100
    objs = []
    for h in (1, 3, 7, 13):                                                  # h * w mostly no multiple of 32
        f = rng.random((h, w)) < 0.6
        f[0, 0] = True
        objs.append(Obj((rng.integers(0, shape[0] - h + 1), rng.integers(0, shape[1] - w + 1)), f))
    assert w == 32 or any((o.fg_fragment.size % 32) for o in objs)
    host = measure.measure_objects_host(objs, shape, g)
    same_bytes(objects_gpu_raw(objs, shape, g, garbage_tails=True), host, f'width {w}, garbage tails')
    same_bytes(measure.measure_objects(objs, shape, g), host, f'width {w}')
    same_bytes(measure.measure_objects(objs, shape), measure.measure_objects_host(objs, shape), f'width {w}, no intensity')


def test_tiny_empty_corner_and_overlapping_fragments(gpu):
    from superdsm_amd import measure
    rng = np.random.default_rng(1)
    H, W = 20, 30
    g = rng.normal(size=(H, W))
    two = np.ones((2, 2), bool)
    objs = [Obj((5, 6), np.ones((1, 1), bool)), Obj((3, 3), np.zeros((4, 5), bool))]
    objs += [Obj(o, two) for o in ((0, 0), (0, W - 2), (H - 2, 0), (H - 2, W - 2))]                    # the four corners: flag bit 0
    objs += [Obj(o, two) for o in ((1, 1), (1, W - 3), (H - 3, 1), (H - 3, W - 3))]                    # one pixel inside: not
    objs += [Obj((8, 8), ellipse(rng, 5)), Obj((9, 10), ellipse(rng, 5))]                               # two overlapping objects
    host = measure.measure_objects_host(objs, (H, W), g)
    assert host['flags'][2:6].tolist() == [1] * 4 and host['flags'][6:10].tolist() == [0] * 4 and host['area'][1] == 0
    same_bytes(measure.measure_objects(objs, (H, W), g), host, 'corners')
    same_bytes(objects_gpu_raw(objs, (H, W), g, garbage_tails=True), host, 'corners, garbage tails')


@pytest.fixture(scope='module')
def tall():
    """A 65535 x 33 image with about 2000 pixels at rows 63 000 .. 65 534: sum_rr passes 2^32 (and 2^42)."""
    rng = np.random.default_rng(65535)
    H, W = 65535, 33
    frag = rng.random((H - 63000, W)) < 2000 / ((H - 63000) * W)
    frag[0, 0] = frag[-1, -1] = True
    g = rng.normal(size=(H, W))
    return (H, W), frag, g


def test_fragment_at_the_bottom_of_the_tallest_image(gpu, tall):
    from superdsm_amd import measure
    shape, frag, g = tall
    objs = [Obj((63000, 0), frag)]
    host = measure.measure_objects_host(objs, shape, g)
    assert host['sum_rr'][0] > 2 ** 42 and 1500 < host['area'][0] < 2500
    same_bytes(measure.measure_objects(objs, shape, g), host, 'tall image')


# ---- labels (1b) ---------------------------------------------------------------------------------------------------------------------
def labels_gpu_raw(labels, n_labels, g=None):
    from superdsm_amd import measure
    M = measure._MeasureSet([labels.shape], [g] if g is not None else None)
    recs, bad = M.labels([labels.astype(np.int32)], [n_labels])
    return recs[0], int(bad[0]), int(M.scale_exponents()[0])


def test_label_spanning_bands_and_segments_and_absent_labels(gpu):
    """200 x 300 pixels are four bands; label 7 runs through all of them and through many segments, so its partial sums meet in global
    memory.  Labels 15 .. 39 are absent: zero records."""
    from superdsm_amd import measure
    rng = np.random.default_rng(4)
    labels = label_scene(rng, (200, 300), 14)
    labels[:, 100:117] = 7
    labels[13::29, :] = 7
    g = rng.normal(size=labels.shape)
    host, bad = measure.label_records_host(labels, 40, g)
    assert bad == 0 and (host['area'][15:] == 0).all()
    recs, gbad, e = labels_gpu_raw(labels, 40, g)
    assert gbad == 0 and e == measure.scale_exponent(g)
    same_bytes(recs, host, 'bands')
    same_bytes(measure.measure_labels(labels, g), measure.measure_labels_host(labels, g), 'bands, table')
    same_bytes(measure.measure_labels(labels), measure.measure_labels_host(labels), 'bands, no intensity')


def test_more_labels_in_a_band_than_table_slots(gpu):
    """64 x 64 pixels, each its own label: 4096 labels in one band, more than any LDS table, so the fallback to global atomics runs."""
    from superdsm_amd import measure
    rng = np.random.default_rng(6)
    labels = rng.permutation(4096).reshape(64, 64).astype(np.int32)
    g = rng.normal(size=labels.shape)
    host, _ = measure.label_records_host(labels, 4096, g)
    recs, bad, _ = labels_gpu_raw(labels, 4096, g)
    assert bad == 0
    same_bytes(recs, host, 'every pixel its own label')


def test_labels_alternating_pixel_by_pixel(gpu):
    from superdsm_amd import measure
    rng = np.random.default_rng(7)
    labels = np.zeros((37, 131), np.int32)
    labels[:, 0::2], labels[:, 1::2] = 1, 2
    labels[20:, 0::3] = 3
    g = rng.normal(size=labels.shape)
    host, _ = measure.label_records_host(labels, 4, g)
    recs, bad, _ = labels_gpu_raw(labels, 4, g)
    assert bad == 0
    same_bytes(recs, host, 'alternating labels')


def test_label_outside_the_range_is_counted_and_skipped(gpu):
    from superdsm_amd import measure
    rng = np.random.default_rng(9)
    labels = label_scene(rng, (60, 70), 9)
    g = rng.normal(size=labels.shape)
    n_labels = int(labels.max())                                             # the highest label equals n_labels
    host, host_bad = measure.label_records_host(labels, n_labels, g)
    recs, bad, _ = labels_gpu_raw(labels, n_labels, g)
    assert bad == host_bad == int((labels == n_labels).sum()) > 0
    same_bytes(recs, host, 'the other labels')                              # nothing else is corrupted
    with pytest.raises(ValueError):
        measure.measure_labels(labels, g, n_labels=n_labels)
    same_bytes(measure.measure_labels(labels, g), measure.measure_labels_host(labels, g), 'a valid call afterwards')


def test_one_label_over_2048_squared_at_the_image_maximum(gpu):
    """Every pixel adds the largest integer the image's scale allows: gsum_hi carries about 2^52 and the limbs must recombine."""
    from superdsm_amd import measure
    labels = np.full((2048, 2048), 3, np.int32)
    g = np.full(labels.shape, 0.75)
    host, _ = measure.label_records_host(labels, 4, g)
    assert host['gsum_hi'][3] == 2048 * 2048 * 3 * 2 ** 28 and host['gsum_lo'][3] == 0
    recs, bad, e = labels_gpu_raw(labels, 4, g)
    assert bad == 0 and e == 0
    same_bytes(recs, host, '2048 x 2048')
    assert measure.intensity_sum_exact(measure._as_table(recs, np.arange(4))[3]) == 2048 * 2048 * 3 / 4


def test_label_at_the_bottom_of_the_tallest_image(gpu, tall):
    from superdsm_amd import measure
    shape, frag, g = tall
    labels = np.zeros(shape, np.int32)
    labels[63000:][frag] = 5
    host = measure.measure_labels_host(labels, g, background_label=None)
    assert host['label'].tolist() == [0, 5] and host['sum_rr'][1] > 2 ** 42
    same_bytes(measure.measure_labels(labels, g, background_label=None), host, 'tall image')
    same_bytes(measure.measure_labels(labels.astype(np.uint16), g), host[1:], 'tall image, uint16 labels')


# ---- intensity, both forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['signed', 'nan and inf', 'negative zero', 'tiny', 'zero', 'largest', 'huge and tiny'])
def test_intensities_of_both_forms(gpu, kind):
    from superdsm_amd import measure
    rng = np.random.default_rng(12)
    labels = label_scene(rng, (50, 60), 8)
    g = rng.normal(size=labels.shape) * 1e3
    if kind == 'nan and inf':
        rr, cc = np.nonzero(labels == 2)
        g[rr[0], cc[0]], g[rr[-1], cc[-1]], g[0, 0] = np.nan, -np.inf, np.inf
        g[labels == 4] = np.nan                                              # an object without a finite pixel
    elif kind == 'negative zero':
        g = np.where(rng.random(labels.shape) < 0.5, -0.0, 0.0)
        g[labels == 3] = -0.0
        g[labels == 4] = rng.choice([-0.0, -1.0, 0.0], size=int((labels == 4).sum()))
    elif kind == 'tiny':
        g = rng.random(labels.shape) * 2.0 ** -971
        g[1, 1] = 2.0 ** -970                                                # the clamp of e
        g[2, 2] = 5e-324
    elif kind == 'zero':
        g = np.zeros(labels.shape)
    elif kind == 'largest':
        g = np.where(rng.random(labels.shape) < 0.5, -1.0, 1.0) * np.finfo(float).max
        g[3, 3] = 1.0
    elif kind == 'huge and tiny':
        g = np.full(labels.shape, 1e-300)
        g[7, 9] = 1e300
    e = measure.scale_exponent(g)
    assert {'tiny': e == -960, 'zero': e == 0, 'largest': e == 1024}.get(kind, True)
    host = measure.measure_labels_host(labels, g, background_label=None)
    gpu_table = measure.measure_labels(labels, g, background_label=None)
    assert (gpu_table['scale_exp'] == e).all()
    same_bytes(gpu_table, host, f'labels, {kind}')
    objs = []
    for l in host['label']:
        rr, cc = np.nonzero(labels == l)
        objs.append(Obj((rr.min(), cc.min()), (labels == l)[rr.min():rr.max() + 1, cc.min():cc.max() + 1]))
    by_object = measure.measure_objects(objs, labels.shape, g)
    same_bytes(by_object, measure.measure_objects_host(objs, labels.shape, g), f'objects, {kind}')
    same_bytes(by_object, host, f'objects against labels, {kind}')


# ---- sets ----------------------------------------------------------------------------------------------------------------------------
def _scene_objects(rng, shape, n):
    objs = []
    for _ in range(n):
        f = ellipse(rng, 7)
        objs.append(Obj((rng.integers(0, shape[0] - f.shape[0] + 1), rng.integers(0, shape[1] - f.shape[1] + 1)), f))
    return objs


def test_sets_give_the_bytes_of_the_single_image_calls(gpu):
    from superdsm_amd import measure
    rng = np.random.default_rng(21)
    shapes = [(40, 70), (129, 33), (64, 257)]
    labels = [label_scene(rng, s, 7) for s in shapes]
    gs = [rng.normal(size=s) * 10.0 ** k for k, s in enumerate(shapes)]       # a scale of its own per image
    objs = [_scene_objects(rng, s, 5 + k) for k, s in enumerate(shapes)]
    objs[1] = []                                                             # an image without objects
    by_labels = measure.measure_labels_many(labels, gs)
    by_objects = measure.measure_objects_many(objs, shapes, gs)
    for k in range(3):
        same_bytes(by_labels[k], measure.measure_labels(labels[k], gs[k]), f'labels of image {k}')
        same_bytes(by_labels[k], measure.measure_labels_host(labels[k], gs[k]), f'labels of image {k}, host')
        same_bytes(by_objects[k], measure.measure_objects(objs[k], shapes[k], gs[k]), f'objects of image {k}')
        same_bytes(by_objects[k], measure.measure_objects_host(objs[k], shapes[k], gs[k]), f'objects of image {k}, host')
    assert len({int(t['scale_exp'][0]) for t in by_labels}) == 3


def test_33_images_are_two_sets(gpu):
    from superdsm_amd import measure, render
    rng = np.random.default_rng(33)
    labels = [rng.integers(0, 4, (8, 8)).astype(np.int32) for _ in range(33)]
    gs = [rng.normal(size=(8, 8)) for _ in range(33)]
    objs = [[Obj((k % 5, k % 3), rng.random((3, 4)) < 0.7)] for k in range(33)]
    by_labels = measure.measure_labels_many(labels, gs)
    by_objects = measure.measure_objects_many(objs, [(8, 8)] * 33, gs)
    rows = measure.label_map_rows_many(labels)
    for k in range(33):
        same_bytes(by_labels[k], measure.measure_labels_host(labels[k], gs[k]), f'labels of image {k}')
        same_bytes(by_objects[k], measure.measure_objects_host(objs[k], (8, 8), gs[k]), f'objects of image {k}')
        assert rows[k] == render.label_map_rows(labels[k])


def test_second_launch_into_a_dirtied_record_buffer_gives_the_same_bytes(gpu):
    from superdsm_amd import measure
    rng = np.random.default_rng(44)
    shapes = [(150, 200), (64, 64)]
    labels = [label_scene(rng, shapes[0], 12), rng.permutation(4096).reshape(64, 64).astype(np.int32)]
    gs = [rng.normal(size=s) for s in shapes]
    n_labels = [20, 4096]
    M = measure._MeasureSet(shapes, gs)
    first, bad = M.labels(labels, n_labels)
    d_out = M.record_buffer(sum(n_labels))
    d_out.fill_(0xA5)
    second, bad2 = M.labels(labels, n_labels, d_out=d_out)
    third, _ = M.labels(labels, n_labels, d_out=d_out)                       # over the records of the launch before
    assert not bad.any() and not bad2.any()
    for k in range(2):
        same_bytes(second[k], first[k], f'dirtied buffer, image {k}')
        same_bytes(third[k], first[k], f'third launch, image {k}')
        same_bytes(first[k], measure.label_records_host(labels[k], n_labels[k], gs[k])[0], f'host, image {k}')


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_tables_of_a_pipeline_result(gpu):
    from superdsm_amd import automation, config, measure, pipeline, render, synth
    spec = synth.WORKLOADS['bbbc039_like']
    shape, layout = synth.bbbc039_like_layout(spec['seed'], 0)
    g = synth.render_image(shape, layout, spec['seed'])
    pl = pipeline.create_reference_pipeline()
    cfg = automation.create_configs(pl, config.Config({'AF_scale': 10}), [g])[0][0]
    data = pl.process_image(g, cfg, out='muted')[0]
    objs = list(data['postprocessed_objects'])
    assert len(objs) > 10
    table = measure.measure_result(data)
    same_bytes(table, measure.measure_objects_host(objs, data['g_raw'].shape, data['g_raw']), 'pipeline objects')
    d = measure.derive(table)
    assert (d['area'] == [int(o.fg_fragment.sum()) for o in objs]).all() and np.isfinite(d['mean_intensity']).all()
    label_map = render.rasterize_labels_gpu(data)
    assert measure.label_map_rows_gpu(label_map) == render.label_map_rows(label_map)


# ---- limits ----------------------------------------------------------------------------------------------------------------------------
def test_limits_raise_and_a_valid_call_follows(gpu):
    from superdsm_amd import measure
    rng = np.random.default_rng(55)
    shape = (30, 40)
    labels, g = label_scene(rng, shape, 5), rng.normal(size=shape)
    objs = _scene_objects(rng, shape, 4)

    def valid():
        same_bytes(measure.measure_objects(objs, shape, g), measure.measure_objects_host(objs, shape, g), 'valid objects')
        same_bytes(measure.measure_labels(labels, g), measure.measure_labels_host(labels, g), 'valid labels')

    with pytest.raises(ValueError):
        measure.measure_objects(objs + [Obj((29, 0), np.ones((2, 2), bool))], shape, g)       # a box leaving the image
    valid()
    with pytest.raises(TypeError):
        measure.measure_labels(labels.astype(np.float64), g)                                 # a label map that is not an integer type
    valid()
    with pytest.raises(ValueError):
        measure.measure_labels(labels, g[:, :-1])                                            # an intensity of another shape
    with pytest.raises(ValueError):
        measure.measure_objects(objs, shape, g[:-1])
    valid()
    with pytest.raises(ValueError):
        measure.measure_labels(labels - 1)                                                   # a negative label, found on the device
    valid()
