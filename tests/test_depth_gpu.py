"""The GPU forms of the depth tables (sdsm_depth.hip) against the ``*_host`` definitions of superdsm_amd/depth.py: every field of every row
and every shell byte for byte, on the smallest inputs at which the kernel can still go wrong -- fragment rows that straddle words, every
kind of outside (box, frame, hole, another label), ties of the inscribed circle and of the median, the early stop of the row scan, the
shell cap, the uint16 edge of d2 and both sides of the LDS tile."""
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
    """Two results (table, shells), byte for byte."""
    from superdsm_amd import _capi, depth as dp
    assert g[0].dtype == h[0].dtype == dp.TABLE_DTYPE and len(g[0]) == len(h[0]), what
    for name in dp.TABLE_DTYPE.names:
        if g[0][name].tobytes() != h[0][name].tobytes():
            k = int(np.nonzero(g[0][name] != h[0][name])[0][0])
            raise AssertionError(f'{what}: field {name} of row {k}: {g[0][name][k]!r} (GPU) != {h[0][name][k]!r} (host)')
    assert g[1].dtype == h[1].dtype == _capi.DEPTH_SHELL_DTYPE and g[1].shape == h[1].shape, f'{what}: shells {g[1].shape} != {h[1].shape}'
    for name in _capi.DEPTH_SHELL_DTYPE.names:
        if g[1][name].tobytes() != h[1][name].tobytes():
            k = tuple(np.argwhere(g[1][name] != h[1][name])[0])
            raise AssertionError(f'{what}: shell field {name} at {k}: {g[1][name][k]!r} (GPU) != {h[1][name][k]!r} (host)')


def objects_gpu_raw(objects, shape, g, n_shells, garbage_tails=False, dirty=None, boxes=None, ws_bytes=None):
    """(table, shells) of sdsm_depth_objects for ``objects``; ``garbage_tails``: the bits of every last word past h * w are set; ``dirty``:
    the byte the outputs and the workspace are filled with before the launch; ``boxes``: the boxes named to the call instead of the
    objects' own; ``ws_bytes``: the workspace size named to the call."""
    from superdsm_amd import depth as dp
    from superdsm_amd.postprocess import pack_fragments
    own, words, packed, _ = pack_fragments(objects)
    boxes = own if boxes is None else np.asarray(boxes, np.int32)
    if garbage_tails:
        for b, bits in zip(own, packed):
            n = int(b[2]) * int(b[3])
            if n % 32:
                w = bits.view(np.uint32)
                w[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)
    D = dp._DepthSet([shape], [np.ascontiguousarray(g, np.float64)] if g is not None else None)
    B = D.buffers(boxes, n_shells)
    if dirty is not None:
        for name in ('d_out', 'd_shells', 'd_ws'):
            if B[name] is not None:
                B[name].fill_(dirty)
    recs, shells = D.objects(np.zeros(len(boxes), np.int32), boxes, words, packed, n_shells, B, ws_bytes)
    return dp._table(np.arange(len(boxes)), recs), shells


def check(objs, shape, g=None, n_shells=8, what=''):
    from superdsm_amd import depth as dp
    host = dp.depth_objects_host(objs, shape, g, n_shells)
    same(dp.depth_objects(objs, shape, g, n_shells), host, what)
    return host


def disc(radius):
    y, x = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    return y * y + x * x <= radius * radius


# ---- words ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w', [31, 32, 33, 65])
def test_fragment_rows_straddle_words_and_tail_bits_are_ignored(gpu, w):
    from superdsm_amd import depth as dp
    rng = np.random.default_rng(w)
    shape = (40, 120)
    g = rng.normal(size=shape)
    objs = []
    for h in (3, 7, 13):                                                     # h * w mostly no multiple of 32
        for f in (np.ones((h, w), bool), rng.random((h, w)) < 0.8):
            objs.append(Obj((rng.integers(0, shape[0] - h + 1), 1 + 2 * rng.integers(0, (shape[1] - w) // 2)), f))     # an odd column offset
    host = dp.depth_objects_host(objs, shape, g)
    same(objects_gpu_raw(objs, shape, g, dp.DEFAULT_SHELLS, garbage_tails=True), host, f'width {w}, garbage tails')
    same(dp.depth_objects(objs, shape, g), host, f'width {w}')


# ---- what is outside -------------------------------------------------------------------------------------------------------------------
def test_box_frame_lines_and_a_diagonal(gpu):
    shape = (30, 41)
    box = np.ones((9, 12), bool)
    objs = [Obj((10, 14), box), Obj((0, 14), box), Obj((21, 14), box), Obj((10, 0), box), Obj((10, 29), box), Obj((0, 0), box), Obj((21, 29), box),
            Obj((3, 2), np.ones((1, 17), bool)), Obj((2, 5), np.ones((19, 1), bool)), Obj((4, 4), np.eye(15, dtype=bool)), Obj((7, 7), np.ones((1, 1), bool))]
    host = check(objs, shape, None, 8, 'outside rules')
    t = host[0]
    assert t['max_d2'][:7].tolist() == [25] * 7 and t['flags'][:7].tolist() == [0, 1, 1, 1, 1, 1, 1]            # the frame is outside like the box
    assert t['max_d2'][7:].tolist() == [1, 1, 1, 1] and t['n_rim'][7:].tolist() == [17, 19, 15, 1]


def test_holes_ties_and_the_two_median_ranks(gpu):
    hole = np.ones((9, 9), bool)
    hole[4, 4] = False
    ring = disc(9) & ~np.pad(disc(4), 5)
    bridge = np.zeros((15, 34), bool)                                        # two discs joined by a one-pixel bridge: 268 pixels,
    bridge[:, :15] |= disc(7)                                                # whose two middle ranks hold d2 = 4 (shell 1) and 5 (shell 2)
    bridge[1:14, 21:34] |= disc(6)
    bridge[7, 14:22] = True
    odd = np.ones((5, 7), bool)
    objs = [Obj((1, 1), hole), Obj((12, 2), ring), Obj((1, 14), np.ones((4, 6), bool)), Obj((33, 3), bridge), Obj((1, 24), odd), Obj((8, 24), odd[:, :6])]
    from superdsm_amd import depth as dp
    t = dp.depth_objects_host(objs, (50, 50), None, 8)[0]
    assert (t['area'][3], t['med_d2_lo'][3], t['med_d2_hi'][3]) == (268, 4, 5) and dp.shell_of(4, 8) != dp.shell_of(5, 8)      # the median between two shells
    assert (t['area'][0], t['med_d2_lo'][0], t['med_d2_hi'][0]) == (80, 2, 4)                      # and the rank above is another value: one more pass
    assert t['area'][4] % 2 == 1 and t['area'][5] % 2 == 0 and t['med_d2_lo'][5] == t['med_d2_hi'][5]          # an even area whose two ranks tie
    assert (t['max_d2'][2], t['max_row'][2], t['max_col'][2], t['n_max'][2]) == (4, 2, 15, 8)      # rows 1 .. 2 x columns 1 .. 4 of the box: the first wins
    assert (t['max_d2'][0], t['n_max'][0], t['n_rim'][0]) == (8, 4, 32 + 4)                        # the diagonal neighbours of the hole's neighbours
    check(objs, (50, 50), None, 8, 'holes and ties')


def test_two_maxima_in_a_row_the_smaller_column_wins(gpu):
    """Full boxes whose deepest pixels tie: 3 x 4 has two of them in one row, 3 x 6 four, 4 x 6 eight in two rows (d2 = 4 wherever the
    nearest side is two steps away).  The smallest (row, column) wins every time."""
    for (h, w), n_max in (((3, 4), 2), ((3, 6), 4), ((4, 6), 8)):
        t = check([Obj((2, 3), np.ones((h, w), bool))], (9, 12), None, 4, f'{h} x {w}')[0]
        assert (t['max_d2'][0], t['max_row'][0], t['max_col'][0], t['n_max'][0]) == (4, 3, 4, n_max)


def test_the_row_scan_stops_early_only_where_it_may(gpu):
    corner = np.ones((12, 12), bool)
    corner[0, 0] = False                                                     # the nearest outside place of (1, 1) is strictly diagonal
    ell = np.zeros((30, 30), bool)                                           # the row neighbour is far, the column neighbour near
    ell[:, :4] = True
    ell[26:, :] = True
    host = check([Obj((3, 3), corner), Obj((20, 3), ell)], (60, 40), None, 8, 'early stop')
    from superdsm_amd import depth as dp
    assert dp.squared_depth(corner)[1, 1] == 2


# ---- shells ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_shells', [1, 2, 32])
def test_shell_counts_of_discs(gpu, n_shells):
    rng = np.random.default_rng(n_shells)
    shape = (100, 100)
    g = rng.gamma(2.0, size=shape)
    objs = [Obj((5, 7), disc(20))] + ([Obj((10, 12), disc(40))] if n_shells == 32 else [])
    host = check(objs, shape, g, n_shells, f'{n_shells} shells')
    assert host[1]['count'].sum(axis=1).tolist() == host[0]['area'].tolist()
    if n_shells == 32:
        assert host[1]['count'][0, 21:].sum() == 0 and host[1]['count'][0, 20] > 0           # radius 20: shallower than 32 shells
        assert host[0]['max_d2'][1] > 32 * 32 and host[1]['count'][1, 31] > 1                # radius 40: the last shell collects


def test_intensities_nonfinite_signed_zero_subnormal_none_and_zero(gpu):
    from superdsm_amd import depth as dp
    rng = np.random.default_rng(5)
    shape = (40, 50)
    objs = [Obj((3, 4), disc(9)), Obj((20, 22), np.ones((11, 13), bool))]
    g = rng.normal(size=shape)
    g[8, 10], g[12, 13], g[13, 13], g[25, 30] = np.nan, np.inf, -0.0, 5e-324
    host = check(objs, shape, g, 6, 'special values')
    assert host[1]['n_finite'].sum() == host[1]['count'].sum() - 2
    tiny = np.zeros(shape)
    tiny[12, 13], tiny[4, 12] = 5e-324, -1.5e-323                            # every finite pixel subnormal: e = -960
    assert check(objs, shape, tiny, 6, 'subnormal image')[0]['scale_exp'].tolist() == [-960, -960]
    none = check(objs, shape, None, 6, 'no intensity image')
    assert not none[1]['n_finite'].any() and not none[1]['gsum_lo'].any() and none[0]['scale_exp'].tolist() == [0, 0]
    zero = check(objs, shape, np.zeros(shape), 6, 'constant zero')
    assert zero[0]['scale_exp'].tolist() == [0, 0] and zero[1]['n_finite'].sum() == zero[1]['count'].sum()


# ---- the uint16 edge and the LDS tile ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('side, max_d2', [(509, 65025), (511, 65536)])
def test_full_squares_at_the_uint16_edge(gpu, side, max_d2):
    host = check([Obj((1, 2), np.ones((side, side), bool))], (514, 515), None, 8, f'{side} x {side}')
    assert host[0]['max_d2'][0] == max_d2 and host[0]['n_max'][0] == 1


def test_boxes_at_above_and_far_above_the_lds_tile(gpu):
    from superdsm_amd import _capi, depth as dp
    cap = _capi.DEPTH_LDS_PIXELS
    assert cap == 96 * 128
    rng = np.random.default_rng(9)
    shape = (200, 420)
    g = rng.normal(size=shape)
    at = rng.random((96, 128)) < 0.97
    above = rng.random((97, 128)) < 0.97
    sparse = np.zeros((150, 260), bool)                                      # far above the cap, few pixels in it
    sparse[20:25, 30:35] = True
    sparse[140, 250] = True
    objs = [Obj((0, 0), at), Obj((100, 3), above), Obj((30, 150), sparse), Obj((2, 300), disc(30))]
    assert dp.workspace_pixels([(0, 0) + o.fg_fragment.shape for o in objs]).tolist() == [0, 97 * 128, 150 * 260, 0]
    host = check(objs, shape, g, 8, 'LDS tile')
    assert host[0]['area'][2] == 26 and host[0]['max_d2'][2] == 9
    same(objects_gpu_raw(objs, shape, g, 8, dirty=0xa5), host, 'dirtied workspace')


def test_a_workspace_too_small_is_an_argument_error_before_any_launch(gpu):
    from superdsm_amd import _capi, depth as dp
    from superdsm_amd.postprocess import pack_fragments
    objs = [Obj((0, 0), np.ones((3, 3), bool)), Obj((0, 0), np.ones((97, 128), bool))]
    boxes, words, packed, _ = pack_fragments(objs)
    D = dp._DepthSet([(120, 130)], None)
    B = D.buffers(boxes, 4)
    B['d_out'].fill_(0xa5)
    need = 97 * 128 * _capi.DEPTH_WS_PIXEL_BYTES
    with pytest.raises(_capi.SdsmError, match='workspace is too small'):
        D.objects(np.zeros(2, np.int32), boxes, words, packed, 4, B, ws_bytes=need - 1)
    assert bool((B['d_out'] == 0xa5).all()), 'nothing was launched'
    with pytest.raises(_capi.SdsmError, match='n_shells'):
        D.objects(np.zeros(2, np.int32), boxes, words, packed, 33, B)
    recs, _ = D.objects(np.zeros(2, np.int32), boxes, words, packed, 4, B, ws_bytes=need)
    assert recs['max_d2'].tolist() == [4, 49 * 49]


# ---- degenerate objects ------------------------------------------------------------------------------------------------------------------
def test_degenerate_objects_give_zero_rows_between_sound_ones(gpu):
    from superdsm_amd import depth as dp
    rng = np.random.default_rng(13)
    shape = (30, 30)
    g = rng.normal(size=shape)
    sound = [Obj((2, 3), disc(5)), Obj((12, 9), rng.random((9, 14)) < 0.8), Obj((0, 0), np.ones((4, 4), bool)), Obj((20, 20), disc(4))]
    leaving, empty_box, no_bits = Obj((25, 3), np.ones((9, 3), bool)), Obj((5, 5), np.ones((2, 3), bool)), Obj((7, 7), np.zeros((5, 6), bool))
    objs = [sound[0], leaving, sound[1], empty_box, sound[2], no_bits, sound[3]]
    boxes = np.array([(int(o.fg_offset[0]), int(o.fg_offset[1])) + o.fg_fragment.shape for o in objs], np.int32)
    boxes[3, 2] = 0                                                          # h == 0
    got = objects_gpu_raw(objs, shape, g, 5, dirty=0xa5, boxes=boxes)
    host = dp.depth_objects_host(sound, shape, g, 5)
    want_t, want_s = np.zeros(7, dp.TABLE_DTYPE), np.zeros((7, 5), host[1].dtype)
    want_t[[0, 2, 4, 6]], want_s[[0, 2, 4, 6]] = host[0], host[1]
    want_t['label'] = np.arange(7)
    same(got, (want_t, want_s), 'degenerate objects')


# ---- sets, labels, repeatability -------------------------------------------------------------------------------------------------------
def test_sets_equal_the_per_image_calls_and_overlapping_objects_are_measured_alone(gpu):
    from superdsm_amd import depth as dp
    rng = np.random.default_rng(51)
    shapes = [(60, 80), (1, 1), (90, 41)]
    gs = [rng.normal(size=s) for s in shapes]
    a, b = disc(9), disc(7)
    per_image = [[Obj((5, 5), a), Obj((10, 12), b)] + [Obj((rng.integers(0, 30), rng.integers(0, 40)), ellipse(rng, 12)) for _ in range(4)],
                 [Obj((0, 0), np.ones((1, 1), bool))],
                 [Obj((rng.integers(0, 60), rng.integers(0, 10)), ellipse(rng, 12)) for _ in range(5)]]
    many = dp.depth_objects_many(per_image, shapes, gs, 6)
    assert len(many) == 3 and many[1][0]['max_d2'].tolist() == [1] and many[1][0]['flags'].tolist() == [1]
    for objs, s, g, m in zip(per_image, shapes, gs, many):
        same(m, dp.depth_objects(objs, s, g, 6), 'set against single call')
        same(m, dp.depth_objects_host(objs, s, g, 6), 'set against host')
    alone = dp.depth_objects(per_image[0][:1], shapes[0], gs[0], 6)
    assert many[0][0][:1].tobytes() == alone[0].tobytes() and many[0][1][:1].tobytes() == alone[1].tobytes()
    maps = [label_scene(rng, shape=shapes[0], n=9), np.ones((1, 1), np.int32), label_scene(rng, shape=shapes[2], n=7)]
    for lab, g, m in zip(maps, gs, dp.depth_labels_many(maps, gs, 6)):
        same(m, dp.depth_labels(lab, g, 6), 'label set against single call')
        same(m, dp.depth_labels_host(lab, g, 6), 'label set against host')


def test_a_list_of_33_images_is_split_into_two_sets_and_every_image_equals_the_host(gpu):
    """One image more than a set holds (``_capi.MAX_SET_IMAGES`` = 32): the last image is a set of its own, and the objects and labels of
    every image are those of its own place in the list.  8 x 8 images with one small object, or a few labels, each; image 5 has no
    object and label map 7 no label."""
    from superdsm_amd import _capi, depth as dp
    rng = np.random.default_rng(33)
    n = _capi.MAX_SET_IMAGES + 1
    assert n == 33
    shapes = [(8, 8)] * n
    gs = [rng.normal(size=s) for s in shapes]
    per_image = [[Obj((rng.integers(0, 4), rng.integers(0, 4)), np.ones((rng.integers(2, 5), rng.integers(2, 5)), bool))] for _ in range(n)]
    per_image[5] = []
    many = dp.depth_objects_many(per_image, shapes, gs, 3)
    assert len(many) == n and [len(m[0]) for m in many] == [len(o) for o in per_image]
    for i, (objs, g, m) in enumerate(zip(per_image, gs, many)):
        same(m, dp.depth_objects_host(objs, (8, 8), g, 3), f'objects of image {i}')
    maps = []
    for i in range(n):
        lab = np.zeros((8, 8), np.int32)
        for l in range(1, 2 + i % 3):                                        # 1 .. 3 labels, later ones over earlier ones
            r0, c0 = rng.integers(0, 6, size=2)
            lab[r0:r0 + 3, c0:c0 + 3] = l
        maps.append(lab)
    maps[7][:] = 0
    many = dp.depth_labels_many(maps, gs, 3)
    assert len(many) == n
    for i, (lab, g, m) in enumerate(zip(maps, gs, many)):
        same(m, dp.depth_labels_host(lab, g, 3), f'labels of image {i}')
    same(dp.depth_labels_many(maps[-2:], None, 3, keep_absent=True)[1], dp.depth_labels_host(maps[-1], None, 3, keep_absent=True), 'absent labels kept')


def test_labels_scene_touching_out_of_range_and_absent(gpu):
    from superdsm_amd import depth as dp
    rng = np.random.default_rng(42)
    labels = label_scene(rng, shape=(97, 131), n=20)
    g = rng.gamma(2.0, size=labels.shape)
    same(dp.depth_labels(labels, g, 6), dp.depth_labels_host(labels, g, 6), 'label scene')
    same(dp.depth_labels(labels), dp.depth_labels_host(labels), 'label scene without intensities')
    touching = np.zeros((9, 40), np.int32)
    touching[1:6, 2:20], touching[1:8, 20:37], touching[6:8, 2:20] = 1, 2, 5          # 3 and 4 do not occur
    host = dp.depth_labels_host(touching, None, 4)
    same(dp.depth_labels(touching, None, 4), host, 'touching labels')
    assert host[0]['max_d2'].tolist() == [9, 16, 1]                                   # the neighbour is outside: 5 x 18, 7 x 17, 2 x 18
    kept = dp.depth_labels(touching, None, 4, keep_absent=True)
    same(kept, dp.depth_labels_host(touching, None, 4, keep_absent=True), 'absent labels')
    assert kept[0]['label'].tolist() == [0, 1, 2, 3, 4, 5] and kept[0]['area'].tolist() == [0, 90, 119, 0, 0, 36]
    same(dp.depth_labels(touching, None, 4, background_label=None), dp.depth_labels_host(touching, None, 4, background_label=None), 'no background')
    with pytest.raises(ValueError, match='labels'):
        dp.depth_labels(np.array([[0, 3], [-1, 3]]))


def test_a_label_outside_the_range_is_counted_and_skipped(gpu):
    """The raw label call with n_labels below the highest label: its pixels are counted in d_bad and belong to no window."""
    from superdsm_amd import depth as dp
    from superdsm_amd.measure import _LabelWindows
    labels = np.zeros((12, 12), np.int32)
    labels[1:6, 1:6], labels[7:11, 2:9] = 1, 2
    host = dp.depth_labels_host(labels, None, 4)
    with_bad = labels.copy()
    with_bad[0, 8:12] = 77                                                   # four pixels of a label the call does not know
    D = dp._DepthSet([labels.shape], None)
    w = _LabelWindows(D.M, [labels], 0, 'depth')
    w.d_labels = D.S.pack([with_bad], np.int32)
    S, B = D.S, D.buffers(w.boxes, 4)
    S.capi.check(S.L.sdsm_depth_labels_multi(S.table, 1, S._p(w.d_labels), w.c_off, w.c_n, S._p(w.d_label_obj), len(w.idx), S._p(w.d_image), S._p(w.d_boxes),
                                             S._p(w.d_off), w.total, S._p(w.d_bits), None, None, None, 4, None, None, 0, 0, S._p(B['d_out']),
                                             S._p(B['d_shells']), S._p(w.d_bad), S._stream()), 'sdsm_depth_labels_multi')
    recs, shells = D._download(B, len(w.idx), 4)
    assert w.d_bad.cpu().numpy().tolist() == [4]
    same((dp._table([1, 2], recs), shells), host, 'labels beside a label out of range')


def test_a_second_launch_into_dirtied_buffers_gives_the_same_bytes(gpu):
    from superdsm_amd import depth as dp
    rng = np.random.default_rng(31)
    shape = (64, 64)
    g = rng.normal(size=shape)
    g[10, 10] = np.inf
    objs = [Obj((rng.integers(0, 30), rng.integers(0, 30)), ellipse(rng, 14)) for _ in range(5)] + [Obj((0, 0), np.zeros((3, 3)))]
    host = dp.depth_objects_host(objs, shape, g)
    for dirty in (0xa5, 0xff):
        same(objects_gpu_raw(objs, shape, g, dp.DEFAULT_SHELLS, dirty=dirty), host, f'outputs filled with {dirty:#x}')


def test_n_rim_equals_the_border_pixels_of_the_shape_tables(gpu):
    from superdsm_amd import depth as dp, shape as sh
    rng = np.random.default_rng(17)
    objs = [Obj((rng.integers(0, 30), rng.integers(0, 30)), ellipse(rng, 14)) for _ in range(6)]
    assert dp.depth_objects(objs, (64, 64))[0]['n_rim'].tolist() == sh.shape_objects(objs, (64, 64))[0]['border_pixels'].tolist()


def test_result_of_pipeline_data(gpu):
    from superdsm_amd import depth as dp
    rng = np.random.default_rng(71)
    objs = [Obj((1, 1), disc(4)), Obj((4, 12), np.ones((3, 3)))]
    data = {'g_raw': rng.random((20, 25)), 'postprocessed_objects': objs}
    same(dp.depth_result(data), dp.depth_objects_host(objs, (20, 25), data['g_raw']), 'depth_result')
    same(dp.depth_result(data, intensity=None, n_shells=3), dp.depth_objects_host(objs, (20, 25), None, 3), 'depth_result without intensities')
    d = dp.derive(*dp.depth_result(data, objs[1:], np.full((20, 25), 2.5)))[0]
    assert (d['max_radius'], d['thickness'], d['center_row'], d['center_col'], d['shell0_mean_intensity'], d['shell1_fraction']) == (2.0, 3.0, 5, 13, 2.5, 1 / 9)
