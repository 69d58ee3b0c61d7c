"""Y-maps, coloured labels and adjacency graphs without a GPU: the colour-map lookup against matplotlib itself, the host definitions
of ``render_ymap`` / ``colorize_labels`` / ``shuffle_labels`` against the reference's sequence written out with matplotlib, the
restated ``skimage.draw.line`` / ``disk`` and the thick line from their definitions (never from themselves), the painting order of
``render_adjacencies_host``, the closed forms the graph kernel relies on, and the new entry points of include/sdsm.h."""
import ctypes as C
import itertools
import os
import re
import runpy

import numpy as np
import pytest

from superdsm_amd import _capi, render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
NAMES = ('bwr', 'seismic', 'gist_rainbow')


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def tables():
    f = np.load(os.path.join(GOLDEN, 'colormaps.npz'))
    return {name: f[name] for name in NAMES}


# ---- colour maps ---------------------------------------------------------------------------------------------------------------------
def lookup_inputs():
    k = np.arange(257) / 256
    x = [0., 1., np.nextafter(1, 0), np.nextafter(1, 2), -0.0, -0.3, np.nan, np.inf, -np.inf]
    return np.concatenate([x, k, np.nextafter(k, -1), np.nextafter(k, 2), np.random.default_rng(0).random(10 ** 5) * 1.2 - 0.1])


@pytest.mark.parametrize('name', NAMES)
def test_lookup_equals_matplotlib(name):
    matplotlib = pytest.importorskip('matplotlib')
    x = lookup_inputs()
    want = matplotlib.colormaps[name](x)
    got = render.colormap_lookup_host(tables()[name], x)
    assert same(got, want)
    assert same(render.colormap_lookup_host(tables()[name], x.reshape(-1, 4)), matplotlib.colormaps[name](x.reshape(-1, 4)))
    # the three ways to name a colour map give one table
    assert same(render.colormap_table(name), tables()[name]) and same(render.colormap_table(matplotlib.colormaps[name]), tables()[name])


def test_lookup_rules_on_a_table_without_matplotlib():
    """The rules one by one on a table whose entries name themselves."""
    N = 7
    table = np.repeat(np.arange(N + 3, dtype=np.float64)[:, None], 4, axis=1)
    look = lambda v: render.colormap_lookup_host(table, np.array([v]))[0, 0]
    assert look(0.0) == 0 and look(-0.0) == 0 and look(1.0) == N - 1 and look(np.nextafter(1, 0)) == N - 1
    assert look(np.nextafter(1, 2)) == N + 1 and look(np.inf) == N + 1
    assert look(-1e-300) == N and look(-np.inf) == N and look(np.nan) == N + 2
    assert look(2.999 / N) == 2 and look(3 / N) in (2, 3)            # truncation (3 / 7 * 7 may round either way)
    with pytest.raises(ValueError):
        render.colormap_table(np.zeros((5, 3)))


def test_committed_tables_are_what_the_generator_produces():
    pytest.importorskip('matplotlib')
    made = runpy.run_path(os.path.join(GOLDEN, 'make_golden_colormaps.py'))['tables']()
    have = tables()
    assert sorted(made) == sorted(have)
    for name in NAMES:
        assert same(made[name], have[name]) and have[name].shape == (259, 4)


@pytest.mark.parametrize('name', ['bwr', 'seismic'])
def test_ymap_host_is_the_reference_sequence(name):
    matplotlib = pytest.importorskip('matplotlib')
    cmap = matplotlib.colormaps[name]
    rng = np.random.default_rng(4)
    y0 = rng.standard_normal((37, 53)) * 0.7
    squash = lambda v: np.exp(5 * v) / (1 + np.exp(5 * v)) - 0.5
    for y_in, clim_in in ((y0, None), (squash(y0.clip(-0.8, 1)), squash(np.array([-0.8, 1.])))):
        y, clim = y_in, clim_in
        if clim is None:
            clim = (-y.std(), +y.std())
        z = np.full((1, y.shape[1]), clim[0])
        z[0, -1] = clim[1]
        y = np.concatenate((z, y), axis=0)
        y = y.clip(*clim)
        y -= y.min()
        y /= y.max()
        want = cmap(y)[1:][:, :, :3]
        assert same(render.render_ymap_host(y_in, clim=clim_in, cmap=name), want)
        assert same(render.render_ymap_host({'y': y_in}, clim=clim_in, cmap=tables()[name]), want)
        assert same(render.render_ymap_host(y_in, clim=clim_in, cmap=cmap), want)


def test_ymap_host_degenerate_inputs():
    """What NumPy makes of them: a NaN anywhere, a constant image under clim=None and clim[0] >= clim[1] all end in NaN everywhere,
    the "bad" colour."""
    t = tables()['bwr']
    bad = np.broadcast_to(t[-1, :3], (6, 9, 3))
    y = np.random.default_rng(1).standard_normal((6, 9))
    ynan = y.copy()
    ynan[2, 3] = np.nan
    assert same(render.render_ymap_host(ynan, clim=(-1, 1), cmap=t), bad.copy())
    assert same(render.render_ymap_host(ynan, cmap=t), bad.copy())
    assert same(render.render_ymap_host(np.full((6, 9), 0.25), cmap=t), bad.copy())
    assert same(render.render_ymap_host(y, clim=(0.5, 0.5), cmap=t), bad.copy())
    assert same(render.render_ymap_host(y, clim=(0.5, -0.5), cmap=t), bad.copy())
    yinf = y.copy()
    yinf[0, 0], yinf[1, 1] = np.inf, -np.inf
    out = render.render_ymap_host(yinf, clim=(-1, 1), cmap=t)
    assert same(out[0, 0], t[255, :3]) and same(out[1, 1], t[0, :3])


# ---- labels --------------------------------------------------------------------------------------------------------------------------
def label_image(seed=0, shape=(40, 50), n=12, dtype=np.uint16):
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, dtype)
    for l in range(1, n + 1):
        r, c = int(rng.integers(0, shape[0] - 6)), int(rng.integers(0, shape[1] - 6))
        lab[r:r + 6, c:c + 6] = l * 3
    return lab


def test_shuffle_and_colorize_host():
    lab = label_image()
    a, b = render.shuffle_labels_host(lab, bg_label=0, seed=5), render.shuffle_labels_host(lab, bg_label=0, seed=5)
    assert same(a, b) and a.dtype == lab.dtype
    assert np.array_equal(a == 0, lab == 0)                                              # the background stays
    present = sorted(set(lab.ravel().tolist()) - {0})
    mapping = {l: set(a[lab == l].tolist()) for l in present}
    assert all(len(v) == 1 for v in mapping.values())
    assert sorted(v.pop() for v in mapping.values()) == present                          # a permutation of the present labels
    assert not same(render.shuffle_labels_host(lab, bg_label=0, seed=6), a)
    full = render.shuffle_labels_host(lab, seed=5)                                       # no background: 0 is shuffled too
    assert sorted(set(full.ravel().tolist())) == [0] + present
    # the reference's own construction, written out
    values0 = list(frozenset(lab.flatten()) - {0})
    np.random.seed(5)
    values1 = np.asarray(values0).copy()
    np.random.shuffle(values1)
    want = np.zeros_like(lab)
    for l0, l1 in zip(values0, values1):
        want[lab == l0] = l1
    assert same(a, want)

    t = tables()['gist_rainbow']
    img = render.colorize_labels_host(lab, cmap=t, bg_color=(0.1, 0.2, 0.3))
    assert img.shape == lab.shape + (3,) and img.dtype == np.float64
    assert same(img[lab == 0], np.broadcast_to(np.array([0.1, 0.2, 0.3]), ((lab == 0).sum(), 3)).copy())
    assert same(img[lab == 36][0], t[255, :3]) and same(img[lab == 18][0], t[int(18 / 36 * 256), :3])
    assert same(render.colorize_labels_host(lab, cmap=t, shuffle=5), render.colorize_labels_host(a, cmap=t))
    one = np.full((40, 20), 7, np.uint16)                                                # a single label: 0 / 0, "bad" everywhere
    assert same(render.colorize_labels_host(one, cmap=t, bg_label=7, bg_color=(1, 0, 1)), np.broadcast_to(np.array([1., 0., 1.]), (40, 20, 3)).copy())
    assert same(render.colorize_labels_host(one, cmap=t), np.broadcast_to(t[-1, :3], one.shape + (3,)).copy())
    two = np.zeros((5, 5), np.int32)
    assert same(render.colorize_labels_host(two, cmap=t, bg_color=(1, 1, 0)), np.broadcast_to(np.array([1., 1., 0.]), (5, 5, 3)).copy())
    two[1, 1] = 4
    nobg = render.colorize_labels_host(two, cmap=t, bg_label=None)
    assert same(nobg[0, 0], t[0, :3]) and same(nobg[1, 1], t[255, :3])


def test_colorize_host_equals_the_reference_sequence_with_matplotlib():
    matplotlib = pytest.importorskip('matplotlib')
    lab = label_image(3)
    cmap = matplotlib.colormaps['gist_rainbow']
    img = cmap((lab - lab.min()) / float(lab.max() - lab.min()))[:, :, :3]
    img[lab == 0] = np.asarray((0, 0, 0))[None, None, :]
    assert same(render.colorize_labels_host(lab), img)


def test_permutation_table_is_the_shuffle():
    lab = label_image(2, dtype=np.int32) - 4                                             # negative labels too
    for bg in (None, -4, 5):
        lo, table = render._perm_table(lab, bg, 9)
        k = lab.astype(np.int64) - lo
        got = np.where((k >= 0) & (k < len(table)), table[k.clip(0, len(table) - 1)], 0).astype(lab.dtype)
        assert same(got, render.shuffle_labels_host(lab, bg_label=bg, seed=9))
    with pytest.raises(ValueError):
        render._int32_labels(np.array([[-100, 100]], np.int8))                            # max - min wraps in int8
    with pytest.raises(ValueError):
        render._int32_labels(np.array([[0, 2 ** 40]], np.int64))
    with pytest.raises(TypeError):
        render._int32_labels(np.zeros((3, 3)))


# ---- lines and disks -------------------------------------------------------------------------------------------------------------
LINES = [((5, 5), (5, 5)), ((3, 2), (3, 30)), ((3, 30), (3, 2)), ((2, 7), (31, 7)), ((31, 7), (2, 7)), ((1, 1), (20, 20)), ((20, 1), (1, 20)),
         ((20, 20), (1, 1)), ((1, 20), (20, 1))] + \
        [((16 + sr * dr, 16 + sc * dc) if flip else (16, 16), (16, 16) if flip else (16 + sr * dr, 16 + sc * dc))
         for sr, sc in itertools.product((1, -1), repeat=2) for dr, dc in ((4, 13), (13, 4), (7, 9), (1, 15), (15, 2)) for flip in (0, 1)]


@pytest.mark.parametrize('p1,p2', LINES)
def test_line_pixels_from_the_definition(p1, p2):
    rr, cc = render.line_pixels_host(*p1, *p2)
    dr, dc = abs(p2[0] - p1[0]), abs(p2[1] - p1[1])
    assert (rr[0], cc[0]) == p1 and (rr[-1], cc[-1]) == p2
    assert len(rr) == max(dr, dc) + 1
    major, minor = (rr, cc) if dr > dc else (cc, rr)
    assert np.array_equal(np.abs(np.diff(major)), np.ones(len(rr) - 1))               # one pixel per step of the driving axis
    assert (np.abs(np.diff(minor)) <= 1).all()                                        # 8-connected
    if max(dr, dc):
        a, b = (p1, p2)
        m0, m1, s0, s1 = (a[0], b[0], a[1], b[1]) if dr > dc else (a[1], b[1], a[0], b[0])
        real = s0 + (major - m0) * (s1 - s0) / (m1 - m0)
        assert (np.abs(minor - real) <= 0.5).all()
    # the closed form the kernel uses: minor offset of step i = floor((2 ds i + dl) / (2 dl))
    dl, ds = max(dr, dc), min(dr, dc)
    i = np.arange(dl + 1)
    closed = (2 * ds * i + dl) // (2 * dl) if dl else np.zeros(1, int)
    assert np.array_equal(np.abs(minor - minor[0]), closed)


def brute_mask(p1, p2, threshold, shape):
    rr, cc = render.line_pixels_host(*p1, *p2)
    out = np.zeros(shape, bool)
    for r in range(shape[0]):
        for c in range(shape[1]):
            out[r, c] = np.sqrt(((rr - r) ** 2 + (cc - c) ** 2).min()) < threshold
    return out


@pytest.mark.parametrize('thickness', [1, 2, 2.5, 3, 4, 5])
def test_thick_line_is_the_brute_force_distance_test(thickness):
    shape = (24, 29)
    for p1, p2 in (((5, 4), (17, 22)), ((0, 0), (23, 28)), ((23, 3), (2, 0)), ((0, 10), (0, 28)), ((12, 28), (12, 28)), ((20, 14), (3, 16))):
        got = render.draw_line_host(p1, p2, thickness, shape)
        assert got.dtype == np.float64 and got.shape == shape
        threshold = (thickness + 1) / 2
        if threshold == int(threshold):
            want = brute_mask(p1, p2, threshold, shape).astype(np.float64)
        else:
            t1 = 2 * int((thickness + 1) // 2) - 1
            inner, outer = brute_mask(p1, p2, (t1 + 1) / 2, shape), brute_mask(p1, p2, (t1 + 3) / 2, shape)
            want = np.where(inner, 1.0, np.where(outer, (thickness - t1) / 2, 0.0))
        assert same(got, want), (thickness, p1, p2)
        # what the kernel is given: integer limits on the squared distance and one value for the ring
        reach, core, ring, core_color, ring_color = render._line_args(thickness, (1, 0.5, 0))
        rr, cc = render.line_pixels_host(*p1, *p2)
        R, Cc = np.mgrid[0:shape[0], 0:shape[1]]
        d2 = ((R[..., None] - rr) ** 2 + (Cc[..., None] - cc) ** 2).min(axis=2)
        assert reach == int(np.floor(np.sqrt(ring))) and reach <= 16
        assert same(np.where(d2 <= core, core_color[1], np.where(d2 <= ring, ring_color[1], 0.0)), got * 0.5)


def test_line_thickness_arguments():
    assert render._line_args(3, (1, 1, 1))[:3] == (1, 3, 3) and render._line_args(1, (1, 1, 1))[:3] == (0, 0, 0)
    assert render._line_args(2, (1, 1, 1))[:3] == (1, 0, 3) and render._line_args(33, (1, 1, 1))[:3] == (16, 288, 288)
    assert render._d2_limit(2.0) == 3 and render._d2_limit(5.0) == 24
    with pytest.raises(NotImplementedError, match='Limits'):
        render._line_args(33.5, (1, 1, 1))
    with pytest.raises(ValueError):
        render._line_args(0.5, (1, 1, 1))


@pytest.mark.parametrize('radius', list(range(1, 13)) + [2.5, 7])
def test_disk_is_the_literal_expression(radius):
    shape = (31, 27)
    for center in ((15, 13), (0, 0), (30, 26), (0, 12), (14, 26), (5, 5)):
        want = np.zeros(shape, bool)
        for r in range(shape[0]):
            for c in range(shape[1]):
                want[r, c] = ((np.float64(r) - center[0]) / radius) ** 2 + ((np.float64(c) - center[1]) / radius) ** 2 < 1
        got = np.zeros(shape, bool)
        got[render.disk_pixels_host(center, radius, shape)] = True
        assert same(got, want)


# ---- the graph picture ---------------------------------------------------------------------------------------------------------------
def test_adjacencies_host_painting_order_and_base():
    shape = (40, 60)
    data = {'g_raw': np.random.default_rng(0).random(shape), 'seeds': [(20, 10), (20, 50), (5, 30)]}
    lines = [((20, 10), (20, 50)), ((5, 30), (35, 30)), ((20, 10), (5, 30))]
    kw = dict(edge_color=(0, 0, 1), endpoint_color=(1, 0, 0), endpoint_edge_color=(0, 1, 0), endpoint_radius=3, endpoint_edge_thickness=2)
    out = render.render_adjacencies_host(data, lines=lines, edge_thickness=3, **kw)
    assert out.dtype == np.uint8 and out.shape == shape + (3,)
    assert tuple(out[20, 10]) == (255, 0, 0)                  # under a rim, a line and a disk: the disk
    assert tuple(out[20, 14]) == (0, 0, 255)                  # under a rim and a line (outside the disk of radius 3): the line
    assert tuple(out[17, 7]) == (0, 255, 0)                   # rim only (3^2 + 3^2 = 18 < 25, >= 9)
    assert tuple(out[20, 30]) == (0, 0, 255)
    base = render.normalize_image(data['g_raw'])
    base = base / base.max()
    assert tuple(out[38, 58]) == tuple((255 * base[38, 58]).clip(0, 255).astype('uint8') for _ in range(3))
    # two lines of fractional thickness crossing: the later line's value stays
    frac = render.render_adjacencies_host(data, lines=lines[:2], edge_thickness=2, **kw)
    assert tuple(frac[21, 30]) == (0, 0, 255)                 # ring of line 0 (0.5), core of line 1 (1.0): line 1 is later
    assert tuple(frac[20, 31]) == (0, 0, 127)                 # core of line 0, ring of line 1: 0.5 * 255 truncated
    swapped = render.render_adjacencies_host(data, lines=lines[1::-1], edge_thickness=2, **kw)
    assert tuple(swapped[21, 30]) == (0, 0, 127) and tuple(swapped[20, 31]) == (0, 0, 255)
    # an override image in 0 .. 255 is divided by 255, one in 0 .. 1 is not
    over = np.random.default_rng(1).integers(0, 256, shape + (4,)).astype(np.uint8)
    a = render.render_adjacencies_host(data, lines=lines, override_img=over, **kw)
    assert tuple(a[38, 58]) == tuple((255 * (over[38, 58, :3] / 255)).clip(0, 255).astype('uint8'))
    b = render.render_adjacencies_host(data, lines=lines, override_img=over[:, :, :3] / 255, **kw)
    assert same(a, b)
    # lines default to the graph's edge lines
    class Graph:
        def get_edge_lines(self):
            return lines
    assert same(render.render_adjacencies_host(dict(data, adjacencies=Graph()), edge_thickness=3, **kw), out)


def band_walk(data, lines, edge_thickness=3, endpoint_radius=5, endpoint_edge_thickness=2, edge_color=(1, 0, 0), endpoint_color=(1, 0, 0),
              endpoint_edge_color=(0, 0, 0)):
    """The two passes of the graph kernel (k_graph_mark, k_graph_paint of sdsm_render.hip) step by step in Python, from the arguments the
    wrapper hands to it: the per-pixel maximum of a painting-order key over the seeds' boxes and the lines' bands, then the painting."""
    base = render._graph_base(data, True, None)
    H, W = base.shape
    n, core_d2, ring_d2, core_color, ring_color = render._line_args(edge_thickness, edge_color)
    rim, disk = endpoint_radius + endpoint_edge_thickness, endpoint_radius
    RIM, LINE, DISK = 1, 1 << 20, 1 << 21
    key = np.zeros((H, W), np.int64)
    R = int(np.ceil(max(rim, disk)))
    with np.errstate(all='ignore'):
        for r0, c0 in data['seeds']:
            for r in range(max(0, r0 - R), min(H, r0 + R + 1)):
                for c in range(max(0, c0 - R), min(W, c0 + R + 1)):
                    dr, dc = np.float64(r - r0), np.float64(c - c0)
                    if (dr / disk) ** 2 + (dc / disk) ** 2 < 1:
                        key[r, c] = max(key[r, c], DISK)
                    elif (dr / rim) ** 2 + (dc / rim) ** 2 < 1:
                        key[r, c] = max(key[r, c], RIM)
    for idx, ((r0, c0), (r1, c1)) in enumerate(lines):
        steep = abs(r1 - r0) > abs(c1 - c0)
        dl, ds = max(abs(r1 - r0), abs(c1 - c0)), min(abs(r1 - r0), abs(c1 - c0))
        sr, sc = (1 if r1 - r0 > 0 else -1), (1 if c1 - c0 > 0 else -1)
        sl, ss, l0, s0 = (sr, sc, r0, c0) if steep else (sc, sr, c0, r0)
        minor = [0 if dl == 0 else (2 * ds * j + dl) // (2 * dl) for j in range(dl + 1)]
        for k in range(-n, dl + n + 1):
            for off in range(-2 * n, 2 * n + 1):
                m = minor[min(max(k, 0), dl)] + off
                r, c = (l0 + sl * k, s0 + ss * m) if steep else (s0 + ss * m, l0 + sl * k)
                if r < 0 or c < 0 or r >= H or c >= W:
                    continue
                best = min((j - k) ** 2 + (minor[j] - m) ** 2 for j in range(max(0, k - n), min(dl, k + n) + 1))
                if best <= ring_d2:
                    key[r, c] = max(key[r, c], LINE | (idx << 1) | (1 if best <= core_d2 else 0))
    out = np.dstack([base] * 3)
    for ch in range(3):
        out[..., ch] = np.where(key >= DISK, endpoint_color[ch], np.where(key >= LINE, np.where(key & 1, core_color[ch], ring_color[ch]),
                                                                          np.where(key >= RIM, endpoint_edge_color[ch], base)))
    return (255 * out).clip(0, 255).astype('uint8')


def test_the_kernels_band_walk_gives_the_definition():
    rng = np.random.default_rng(5)
    data = {'g_raw': rng.random((50, 64)), 'seeds': [(10, 10), (44, 60), (25, 32), (0, 63), (49, 0)]}
    lines = [((10, 10), (44, 60)), ((44, 60), (10, 10)), ((25, 32), (0, 63)), ((49, 0), (0, 63)), ((10, 10), (10, 60)), ((49, 0), (10, 0)), ((25, 32), (25, 32)),
             ((3, 40), (40, 34)), ((46, 20), (30, 61))]
    for thickness in (1, 2, 2.5, 3, 7.25, 33):
        kw = dict(edge_thickness=thickness, edge_color=(0.9, 0.3, 0.1), endpoint_color=(0, 0, 1), endpoint_edge_color=(1, 1, 0.5))
        assert same(band_walk(data, lines, **kw), render.render_adjacencies_host(data, lines=lines, **kw)), thickness
    for kw in (dict(endpoint_radius=40, endpoint_edge_thickness=24), dict(endpoint_radius=0, endpoint_edge_thickness=0), dict(endpoint_radius=2.5, endpoint_edge_thickness=1.5)):
        assert same(band_walk(data, lines, **kw), render.render_adjacencies_host(data, lines=lines, **kw)), kw


def test_limits_are_refused_before_any_device_work():
    shape = (30, 30)
    data = {'g_raw': np.random.default_rng(0).random(shape), 'seeds': [(5, 5)]}
    with pytest.raises(NotImplementedError, match='Limits'):
        render.render_adjacencies(data, lines=[], endpoint_radius=63, endpoint_edge_thickness=2)
    with pytest.raises(NotImplementedError, match='Limits'):
        render.render_adjacencies(data, lines=[], edge_thickness=34)
    for seeds, lines in (([(30, 5)], []), ([(5, -1)], []), ([(5, 5)], [((5, 5), (5, 30))]), ([(5.5, 5)], [])):
        with pytest.raises(ValueError, match='outside|integer'):
            render.render_adjacencies(dict(data, seeds=seeds), lines=lines)
    with pytest.raises(ValueError, match='65535'):
        render.render_adjacencies(data, lines=[((1, 1), (2, 2))] * 65536)
    with pytest.raises(NotImplementedError, match='Limits'):
        render.render_adjacencies(data, lines=[], override_img=np.zeros(shape + (3,), np.float32))
    with pytest.raises(NotImplementedError, match='Limits'):
        render.render_ymap(np.zeros((5, 1)), cmap=tables()['bwr'])
    with pytest.raises(NotImplementedError, match='Limits'):
        render.render_ymap(np.zeros((5, 5)), cmap=np.zeros((1028, 4)))
    with pytest.raises(ValueError, match='mode'):
        render.export_views([data], 'img')


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ['sdsm_render_label_range', 'sdsm_render_label_range_multi', 'sdsm_render_colormap', 'sdsm_render_colormap_multi', 'sdsm_render_graph',
               'sdsm_render_graph_multi']
_CTYPES = {'int': C.c_int, 'int64_t': C.c_int64, 'double': C.c_double, 'size_t': C.c_size_t}
_HOST_POINTERS = {'const sdsm_set_image': C.POINTER(_capi.SetImage), 'const double': C.POINTER(C.c_double), 'const int64_t': C.POINTER(C.c_int64),
                  'const int32_t': C.POINTER(C.c_int32)}


def test_new_symbols_resolve_with_the_declared_argument_types():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sdsm.h')).read(), flags=re.S)
    lib = _capi.lib()
    for name in NEW_SYMBOLS:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', text)
        assert m, f'{name} is not declared in include/sdsm.h'
        res, args = _capi.SYMBOLS[name]
        assert res is C.c_int and getattr(lib, name).argtypes == args
        declared = [a.strip() for a in m.group(1).split(',')]
        assert len(declared) == len(args), name
        for d, a in zip(declared, args):
            if '*' in d:
                assert a is C.c_void_p or a is _HOST_POINTERS[d.split('*')[0].strip()], (name, d)
            else:
                assert a is _CTYPES[d.rsplit(' ', 1)[0].replace('const ', '').strip()], (name, d)
    assert _capi.RENDER_MAX_COLORS == 1024 and '#define SDSM_RENDER_MAX_COLORS 1024' in text
    assert _capi.RENDER_MAX_SEED_RADIUS == 64 and '#define SDSM_RENDER_MAX_SEED_RADIUS 64' in text


def test_argument_checks_come_before_any_device_work():
    lib = _capi.lib()
    many = (_capi.SetImage * 33)()
    for k in range(33):
        many[k].offset, many[k].H, many[k].W = 64 * k, 8, 8
    x = C.c_void_p(256)              # never dereferenced: every call below is refused on its arguments
    col, clim = (C.c_double * 12)(), (C.c_double * 4)(0, 1, 0, 1)
    off, lo = (C.c_int64 * 34)(), (C.c_int32 * 33)()
    assert lib.sdsm_render_colormap(8, 8, 0, x, x, 0, clim, None, 0, 0, None, None, 0, x, x, None) == -1 and b'1024' in lib.sdsm_last_error()
    assert lib.sdsm_render_colormap(8, 8, 0, x, x, 1025, clim, None, 0, 0, None, None, 0, x, x, None) == -1
    assert lib.sdsm_render_colormap(8, 8, 2, x, x, 256, clim, None, 0, 0, None, None, 0, x, x, None) == -1
    assert lib.sdsm_render_colormap(8, 8, 0, x, x, 256, None, None, 0, 0, None, None, 0, x, x, None) == -1      # values without clim
    assert lib.sdsm_render_colormap(8, 8, 0, x, x, 256, clim, None, 0, 0, None, None, 0, None, x, None) == -1   # ... without flags
    assert lib.sdsm_render_colormap(8, 8, 1, x, x, 256, None, None, 0, 0, None, None, 0, None, x, None) == -1   # labels without a range
    assert lib.sdsm_render_colormap(8, 8, 1, x, x, 256, None, x, -1, 0, x, None, 0, None, x, None) == -1 and b'permutation' in lib.sdsm_last_error()
    assert lib.sdsm_render_label_range(8, 8, x, None, 0, 0, None, None, None) == -1
    assert lib.sdsm_render_label_range(8, 8, None, None, 0, 0, x, None, None) == -1
    assert lib.sdsm_render_label_range(0, 8, x, None, 0, 0, x, None, None) == -1 and b'image table' in lib.sdsm_last_error()
    g = lambda **kw: lib.sdsm_render_graph(8, 8, kw.get('n', 1), kw.get('prims', x), kw.get('rim', 7.0), kw.get('disk', 5.0), kw.get('reach', 1), kw.get('core', 3),
                                           kw.get('ring', 3), col, kw.get('base', x), kw.get('ch', 1), x, x, None)
    assert g(rim=64.5) == -1 and b'radius' in lib.sdsm_last_error()
    assert g(disk=-1.0) == -1 and g(rim=float('nan')) == -1
    assert g(reach=17, ring=300, core=300) == -1 and b'line_reach' in lib.sdsm_last_error()
    assert g(ring=4) == -1 and g(core=4) == -1 and g(core=-2) == -1
    assert g(ch=2) == -1 and g(prims=None) == -1 and g(base=None) == -1 and g(n=-1) == -1
    for n_images, table in ((33, many), (0, many)):
        assert lib.sdsm_render_colormap_multi(table, n_images, 0, x, x, 256, clim, None, None, None, None, None, 0, x, x, None) == -1 and b'32 images' in lib.sdsm_last_error()
        assert lib.sdsm_render_label_range_multi(table, n_images, x, None, off, lo, x, None, None) == -1
        assert lib.sdsm_render_graph_multi(table, n_images, 1, x, 7.0, 5.0, 1, 3, 3, col, x, 1, x, x, None) == -1
