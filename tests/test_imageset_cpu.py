"""The one image-set layer without a GPU: ``imageset.SetLayout`` / ``in_sets`` on the host, and the single-image entry points of the C
ABI, which are sets of one image: what they refuse and what their workspace queries answer."""
import ctypes as C

import numpy as np
import pytest

SHAPES = [(520, 696), (1, 1), (1, 4099), (4099, 1), (512, 512), (33, 70)]


@pytest.mark.parametrize('align', [64, 256])
def test_set_layout_offsets_and_round_trip(align):
    from superdsm_amd import _capi
    from superdsm_amd.imageset import SetLayout
    lay = SetLayout(SHAPES, align=align)
    up = lambda n: (n + align - 1) // align * align
    want = np.concatenate([[0], np.cumsum([up(h * w) for h, w in SHAPES])])
    assert lay.shapes == SHAPES and lay.offsets.dtype == np.int64 and lay.offsets.tolist() == want[:-1].tolist() and lay.total == want[-1]
    assert isinstance(lay.table, _capi.SetImage * len(SHAPES))
    assert [(t.offset, t.H, t.W) for t in lay.table] == [(o, h, w) for o, (h, w) in zip(want[:-1].tolist(), SHAPES)]
    assert all(o % align == 0 for o in lay.offsets) and lay.total % align == 0

    rng = np.random.default_rng(7)
    for dtype, channels, tail in ((np.float64, 1, ()), (np.int32, 1, ()), (np.uint8, 1, ()), (np.float64, 3, (3,))):
        arrays = [(rng.random((h, w) + tail) * 200).astype(dtype) + 1 for h, w in SHAPES]      # no zero: the padding is told apart
        flat = lay.pack(arrays, dtype, channels)
        assert flat.dtype == dtype and flat.shape == (lay.total * channels,)
        for o, (h, w), a in zip(lay.offsets, SHAPES, arrays):
            assert np.array_equal(flat[o * channels:(o + h * w) * channels], a.reshape(-1))
        assert np.count_nonzero(flat) == sum(a.size for a in arrays)                            # everything between the images is zero
        back = lay.unpack(flat, channels, tail)
        assert len(back) == len(arrays)
        for a, b in zip(arrays, back):
            assert b.dtype == dtype and b.shape == a.shape and np.array_equal(a, b) and not np.shares_memory(b, flat)
    # a converting pack: values, not bytes
    assert np.array_equal(lay.unpack(lay.pack([np.full(s, 3, np.uint16) for s in SHAPES], np.int32))[2], np.full((1, 4099), 3, np.int32))


def test_set_layout_takes_one_to_max_images():
    from superdsm_amd import _capi
    from superdsm_amd.imageset import SetLayout
    assert _capi.MAX_SET_IMAGES == 32
    for n in (0, 33):
        with pytest.raises(ValueError, match='1 .. 32 images'):
            SetLayout([(4, 5)] * n)
    assert SetLayout([(4, 5)] * 32).total == 32 * 64 and SetLayout([(4, 5)], align=256).total == 256


def test_in_sets():
    from superdsm_amd.imageset import in_sets
    assert in_sets(0) == []
    assert in_sets(1) == [slice(0, 32)] and in_sets(32) == [slice(0, 32)]
    assert in_sets(33) == [slice(0, 32), slice(32, 64)]
    assert in_sets(70) == [slice(0, 32), slice(32, 64), slice(64, 96)]
    items = list(range(70))
    assert [len(items[part]) for part in in_sets(70)] == [32, 32, 6] and sum((items[part] for part in in_sets(70)), []) == items


def _align256(b):
    return (b + 255) // 256 * 256


def test_single_image_workspace_queries_keep_their_numbers():
    """The sizes the single-image queries gave before they became sets of one: markers 4 * align256(4 n) + align256(4 * chunks) + 256
    with chunks of 4096 pixels, EDT 2 * align256(4 n).  They answer for every H, W >= 1, also where the call refuses the shape."""
    from superdsm_amd import _capi
    L = _capi.lib()
    recorded = {'sdsm_c2f_markers_workspace_bytes': [5791488, 1536, 67072, 67072, 4194816, 38400],
                'sdsm_edt_exact_workspace_bytes': [2895360, 512, 33280, 33280, 2097152, 18944]}
    for (h, w), markers, edt in zip(SHAPES, *recorded.values()):
        n = h * w
        assert L.sdsm_c2f_markers_workspace_bytes(h, w) == markers == 4 * _align256(4 * n) + _align256(4 * ((n + 4095) // 4096)) + 256
        assert L.sdsm_edt_exact_workspace_bytes(h, w) == edt == 2 * _align256(4 * n)
        one = (_capi.SetImage * 1)()
        one[0].offset, one[0].H, one[0].W = 0, h, w
        assert L.sdsm_c2f_markers_workspace_bytes_multi(one, 1) == markers and L.sdsm_edt_exact_workspace_bytes_multi(one, 1) == edt
    for query in (L.sdsm_c2f_markers_workspace_bytes, L.sdsm_edt_exact_workspace_bytes):
        assert query(0, 5) == 0 and query(5, 0) == 0 and query(-1, -1) == 0
    assert L.sdsm_edt_exact_workspace_bytes(65536, 1) == 524288 and L.sdsm_c2f_markers_workspace_bytes(65536, 1) == 1049088
    assert L.sdsm_c2f_markers_workspace_bytes(46341, 46341) == 34361910784 and L.sdsm_edt_exact_workspace_bytes(46341, 46341) == 17179906560


def test_single_image_entry_points_refuse_what_they_refused():
    from superdsm_amd import _capi
    L = _capi.lib()
    fake = C.c_void_p(4096)                              # never dereferenced: every call below fails its checks first
    big = 1 << 40
    OK, ARG, WS = 0, -1, -3

    def markers(H=10, W=12, y=fake, mask=fake, out=fake, count=fake, ws=fake, ws_bytes=big):
        return L.sdsm_c2f_markers(y, H, W, 0.2, mask, out, count, ws, ws_bytes, None)

    assert markers(H=0) == ARG and markers(W=0) == ARG and markers(H=-3) == ARG
    assert markers(H=46341, W=46341) == ARG                                 # H * W >= 2^31
    for name in ('y', 'mask', 'out', 'count', 'ws'):
        assert markers(**{name: None}) == ARG
    assert markers(ws_bytes=L.sdsm_c2f_markers_workspace_bytes(10, 12) - 1) == WS
    assert 'workspace' in L.sdsm_last_error().decode()
    assert markers(H=65536, W=1, ws_bytes=16) == WS                         # a long thin image is in range for the markers

    def edt(H=10, W=12, target=fake, out=fake, ws=fake, ws_bytes=big):
        return L.sdsm_edt_exact(target, H, W, out, ws, ws_bytes, None)

    assert edt(H=0) == ARG and edt(W=0) == ARG
    assert edt(H=65536, W=2) == ARG and edt(H=2, W=65536) == ARG
    for name in ('target', 'out', 'ws'):
        assert edt(**{name: None}) == ARG
    assert edt(ws_bytes=L.sdsm_edt_exact_workspace_bytes(10, 12) - 1) == WS
    assert 'workspace' in L.sdsm_last_error().decode()
    assert edt(H=65535, W=1, ws_bytes=16) == WS

    def post(H=20, W=30, n=1, g=fake, gs=fake, bg=fake, boxes=fake, bits_off=fake, bits=fake, new_off=fake, new_bits=fake, pool=None,
             pool_off=None, exterior_scale=5.0, exterior_offset=5.0, max_distance=1, stdamp=2.0, out=fake):
        return L.sdsm_post_objects(g, gs, bg, H, W, n, boxes, bits_off, bits, new_off, new_bits, pool, pool_off, exterior_scale,
                                   exterior_offset, 1e-4, 1.0, max_distance, stdamp, out, None)

    assert post(H=0) == ARG and post(W=0) == ARG and post(H=65536) == ARG and post(W=65536) == ARG and post(n=-1) == ARG
    assert post(n=0, g=None, gs=None, bg=None, boxes=None, bits_off=None, bits=None, out=None) == OK     # nothing to do: no pointer is looked at
    assert post(n=0, H=0) == ARG and post(n=0, W=65536) == ARG
    for name in ('g', 'gs', 'bg', 'boxes', 'bits_off', 'bits', 'out'):
        assert post(**{name: None}) == ARG
    assert post(exterior_scale=0.0) == ARG and post(exterior_offset=-1.0) == ARG and post(max_distance=-1) == ARG and post(max_distance=17) == ARG
    assert post(new_off=None) == ARG and post(new_bits=None) == ARG         # the refinement needs its output buffers
    assert post(pool=fake) == ARG and post(pool_off=fake) == ARG            # the boundary pool and its offsets go together
