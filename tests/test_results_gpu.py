"""Label maps and overlays on the GPU: byte equality (``np.array_equal`` and equal ``dtype``) of ``render.rasterize_labels_gpu`` /
``rasterize_labels_many`` with the host definition ``render.rasterize_labels``, and of every overlay with its ``*_host`` definition,
on fixtures, pipeline results and constructed scenes that force every branch; a second launch of every call gives the same bytes."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    from superdsm_amd import _capi
    _capi.lib()
    return torch


class Obj:
    def __init__(self, offset, fragment):
        self.fg_offset, self.fg_fragment = np.asarray(offset, int), np.asarray(fragment, bool)

    def fill_foreground(self, out, value=True):
        h, w = self.fg_fragment.shape
        out[self.fg_offset[0]:self.fg_offset[0] + h, self.fg_offset[1]:self.fg_offset[1] + w][self.fg_fragment] = value


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def disc_objects(shape, n, rmin, rmax, seed, square=False):
    """Random discs (or squares: plenty of distance ties) cut at the image border."""
    rng = np.random.default_rng(seed)
    H, W = shape
    objs = []
    for _ in range(n):
        r = int(rng.integers(rmin, rmax + 1))
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        r0, r1, c0, c1 = max(0, cy - r), min(H, cy + r + 1), max(0, cx - r), min(W, cx + r + 1)
        yy, xx = np.mgrid[r0:r1, c0:c1]
        frag = np.ones(yy.shape, bool) if square else (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        objs.append(Obj((r0, c0), frag))
    return objs


def data_of(shape, seed=0, rgb=False):
    rng = np.random.default_rng(1000 + seed)
    d = {'g_raw': rng.random(shape) * 3 - 0.5}
    if rgb:
        d['g_rgb'] = rng.integers(0, 256, shape + (3,)).astype(np.float64)
    return d


def golden_objects():
    f = np.load(os.path.join(GOLDEN, 'render.npz'))
    shape = tuple(int(v) for v in f['shape'])
    return shape, [Obj(f[f'o{k}_offset'], f[f'o{k}_fragment']) for k in range(int(f['n']))]


def scenes():
    """name -> (shape, objects)."""
    out = {}
    shape, objs = golden_objects()
    out['golden'] = (shape, objs)
    out['heavy_discs'] = ((96, 128), disc_objects((96, 128), 40, 5, 14, 1))
    out['heavy_squares'] = ((80, 90), disc_objects((80, 90), 30, 3, 9, 2, square=True))
    base = disc_objects((64, 70), 6, 4, 9, 3)
    out['coincide2'] = ((64, 70), base[:3] + [Obj(base[1].fg_offset, base[1].fg_fragment)] + base[3:])
    out['coincide3'] = ((64, 70), [Obj(base[0].fg_offset, base[0].fg_fragment)] + base + [Obj(base[0].fg_offset, base[0].fg_fragment), Obj(base[5].fg_offset, base[5].fg_fragment)])
    out['none'] = ((33, 47), [])
    out['tiny_and_border'] = ((50, 61), disc_objects((50, 61), 25, 1, 4, 4) + [Obj((0, 0), np.ones((5, 61), bool)), Obj((47, 20), np.ones((3, 3), bool)), Obj((10, 10), np.zeros((4, 4), bool))])
    out['one_pixel_image'] = ((1, 1), [Obj((0, 0), np.ones((1, 1), bool))])
    return out


def check_labels(render, data, objs, **kw):
    want = render.rasterize_labels(data, objs, **kw)
    got = render.rasterize_labels_gpu(data, objs, **kw)
    again = render.rasterize_labels_gpu(data, objs, **kw)
    assert want.dtype == np.uint16
    assert same(got, want), (kw, int((got != want).sum()))
    assert same(again, got)
    return want


@pytest.mark.parametrize('name', list(scenes()))
@pytest.mark.parametrize('thr', [0, 0.3, 1, np.inf])
def test_labels_merge_thresholds(gpu, name, thr):
    from superdsm_amd import render
    shape, objs = scenes()[name]
    check_labels(render, data_of(shape), objs, merge_overlap_threshold=thr)


@pytest.mark.parametrize('name', list(scenes()))
@pytest.mark.parametrize('dilate', [-3, 2, 16])
def test_labels_dilate_and_erode(gpu, name, dilate):
    from superdsm_amd import render
    shape, objs = scenes()[name]
    check_labels(render, data_of(shape), objs, dilate=dilate)
    check_labels(render, data_of(shape), objs, dilate=dilate, merge_overlap_threshold=0.3, background_label=-1)


def test_labels_background_label_and_flood_is_exercised(gpu):
    from superdsm_amd import render
    shape, objs = scenes()['heavy_squares']
    want = check_labels(render, data_of(shape), objs, background_label=-1)
    assert (want == 65535).any()
    # the scene does make the flood decide pixels: the overlaps are many
    masks = np.sum(list(render.rasterize_objects(data_of(shape), objs)), axis=0)
    assert (masks > 1).sum() > 200
    for name in ('coincide2', 'coincide3'):
        shape, objs = scenes()[name]
        lab = check_labels(render, data_of(shape), objs)
        assert len(np.unique(lab)) - 1 >= 2


def test_radius_above_16_is_refused(gpu):
    from superdsm_amd import render
    shape, objs = golden_objects()
    with pytest.raises(NotImplementedError, match='Limits'):
        render.rasterize_labels_gpu(data_of(shape), objs, dilate=17)
    with pytest.raises(NotImplementedError, match='Limits'):
        render.render_result_over_image(data_of(shape), objs, border_width=18, border_position='inner')
    with pytest.raises(NotImplementedError, match='Limits'):
        render.render_result_over_image(data_of(shape), objs, border_position='outer')


def _pipeline_data(kind):
    from superdsm_amd import automation, config, pipeline, synth
    if kind == 'synthetic256':
        spec = synth.WORKLOADS['synthetic256']
        layout = synth.random_layout(spec['shape'], spec['n'], spec['radius'], spec['seed'], min_sep=2.2)
        g = synth.render_image(spec['shape'], layout, spec['seed'])
    else:
        spec = synth.WORKLOADS['bbbc039_like']
        shape, layout = synth.bbbc039_like_layout(spec['seed'], 0)
        g = synth.render_image(shape, layout, spec['seed'])
    pl = pipeline.create_reference_pipeline()
    cfg = automation.create_configs(pl, config.Config({'AF_scale': 10}), [g])[0][0]
    return pl.process_image(g, cfg, out='muted')[0]


@pytest.fixture(scope='module')
def pipeline_results(gpu):
    return {k: _pipeline_data(k) for k in ('synthetic256', 'bbbc039_like')}


@pytest.mark.parametrize('kind', ['synthetic256', 'bbbc039_like'])
def test_labels_and_overlays_of_pipeline_results(gpu, pipeline_results, kind):
    from superdsm_amd import render
    data = pipeline_results[kind]
    assert len(data['postprocessed_objects']) > 0
    for kw in (dict(), dict(merge_overlap_threshold=0.3), dict(dilate=2), dict(dilate=-3, background_label=-1)):
        check_labels(render, data, 'postprocessed_objects', **kw)
    for pos in ('center', 'inner'):
        want = render.render_result_over_image_host(data, border_position=pos)
        got = render.render_result_over_image(data, border_position=pos)
        assert same(got, want) and got.dtype == np.uint8
    for fn, host in ((render.render_atoms, render.render_atoms_host), (render.render_foreground_clusters, render.render_foreground_clusters_host)):
        want, got = host(data), fn(data)
        assert same(got, want) and same(fn(data), got)


def test_labels_many(gpu):
    from superdsm_amd import render
    sc = scenes()
    names = ['heavy_discs', 'coincide3', 'none']
    datas = [data_of(sc[n][0], k) for k, n in enumerate(names)]
    objs = [sc[n][1] for n in names]
    for kw in (dict(), dict(merge_overlap_threshold=0.3, dilate=2), dict(dilate=-3, background_label=-1)):
        got = render.rasterize_labels_many(datas, objs, **kw)
        again = render.rasterize_labels_many(datas, objs, **kw)
        for d, o, g, a in zip(datas, objs, got, again):
            assert same(g, render.rasterize_labels_gpu(d, o, **kw)) and same(g, render.rasterize_labels(d, o, **kw)) and same(a, g)
    # 33 images: one more than a call takes
    shapes = [(20 + 3 * k, 70 - k) for k in range(33)]
    datas = [data_of(s, k) for k, s in enumerate(shapes)]
    objs = [disc_objects(s, 3 + k % 5, 2, 7, 50 + k) for k, s in enumerate(shapes)]
    got = render.rasterize_labels_many(datas, objs, merge_overlap_threshold=0.5)
    again = render.rasterize_labels_many(datas, objs, merge_overlap_threshold=0.5)
    assert len(got) == 33 and len(again) == 33 and all(same(a, g) for a, g in zip(again, got))
    for d, o, g in zip(datas, objs, got):
        assert same(g, render.rasterize_labels_gpu(d, o, merge_overlap_threshold=0.5))
    for d, o in list(zip(datas, objs))[::8]:
        assert same(render.rasterize_labels_gpu(d, o, merge_overlap_threshold=0.5), render.rasterize_labels(d, o, merge_overlap_threshold=0.5))


@pytest.mark.parametrize('name', list(scenes()))
@pytest.mark.parametrize('pos', ['center', 'inner'])
@pytest.mark.parametrize('width', [2, 6, 16])
def test_result_overlay(gpu, name, pos, width):
    from superdsm_amd import render
    shape, objs = scenes()[name]
    rng = np.random.default_rng(5)
    cases = [(data_of(shape, 1), None), (data_of(shape, 2, rgb=True), None), (data_of(shape, 3), rng.random(shape) * 1.4 - 0.2), (data_of(shape, 4), rng.random(shape + (3,)))]
    for k, (data, override) in enumerate(cases):
        kw = dict(border_width=width, border_position=pos, override_img=override, color='gytw'[k], merge_overlap_threshold=[np.inf, 0.3][k % 2])
        want = render.render_result_over_image_host(data, objs, **kw)
        got = render.render_result_over_image(data, objs, **kw)
        assert same(got, want), (k, int((got != want).sum()))
        assert same(render.render_result_over_image(data, objs, **kw), got)


def test_result_overlay_many(gpu):
    from superdsm_amd import render
    sc = scenes()
    names = ['heavy_discs', 'golden', 'none']
    datas = [data_of(sc[n][0], k, rgb=(k == 1)) for k, n in enumerate(names)]
    objs = [sc[n][1] for n in names]
    names = list(sc)
    datas = [data_of(sc[n][0], k, rgb=(k % 3 == 1)) for k, n in enumerate(names)]
    objs = [sc[n][1] for n in names]
    for kw in (dict(border_width=4), dict(border_width=6, border_position='inner', merge_overlap_threshold=0.3, color='t')):
        got = render.render_result_over_image_many(datas, objs, **kw)
        again = render.render_result_over_image_many(datas, objs, **kw)
        assert len(got) == len(datas)
        for d, o, g, a in zip(datas, objs, got, again):
            assert same(g, render.render_result_over_image_host(d, o, **kw)) and same(a, g)
            assert same(g, render.render_result_over_image(d, o, **kw))


@pytest.mark.parametrize('radius', [1, 2, 3, 5, 16])
def test_region_overlays(gpu, radius):
    from superdsm_amd import render
    rng = np.random.default_rng(radius)
    for shape in ((70, 95), (33, 200), (1, 40)):
        # a label image of blocks of random labels: the labels do not overlap, 0 is the discarded background
        regions = np.kron(rng.integers(0, 6, (shape[0] // 8 + 1, shape[1] // 11 + 1)), np.ones((8, 11), int))[:shape[0], :shape[1]]
        img = rng.random(shape)
        for bgl in (None, 0, 3):
            b, k = render.rasterize_regions(regions, bgl, radius)
            bh, kh = render.rasterize_regions_host(regions, bgl, radius)
            assert same(b, bh) and same(k, kh)
            b2, k2 = render.rasterize_regions(regions, bgl, radius)
            assert same(b2, b) and same(k2, k)
            for im in (img, rng.random(shape + (3,)), img[:, :, None]):
                want = render.render_regions_over_image_host(im, regions, background_label=bgl, radius=radius, color=(0.2, 1, 0.5))
                got = render.render_regions_over_image(im, regions, background_label=bgl, radius=radius, color=(0.2, 1, 0.5))
                assert same(got, want), int((got != want).sum())
                assert same(render.render_regions_over_image(im, regions, background_label=bgl, radius=radius, color=(0.2, 1, 0.5)), got)
        data = {'g_raw': img * 7 - 2, 'atoms': regions, 'clusters': (regions > 2) * regions}
        for fn, host in ((render.render_atoms, render.render_atoms_host), (render.render_foreground_clusters, render.render_foreground_clusters_host)):
            for kw in (dict(border_radius=radius), dict(border_radius=radius, normalize_img=False), dict(border_radius=radius, override_img=img + 0.5)):
                assert same(fn(data, **kw), host(data, **kw))
        other = dict(data, g_raw=data['g_raw'][::-1].copy(), atoms=regions[::-1].copy(), clusters=data['clusters'][::-1].copy())
        for many_fn, host in ((render.render_atoms_many, render.render_atoms_host), (render.render_foreground_clusters_many, render.render_foreground_clusters_host)):
            many, again = many_fn([data, other], border_radius=radius), many_fn([data, other], border_radius=radius)
            assert same(many[0], host(data, border_radius=radius)) and same(many[1], host(other, border_radius=radius))
            assert same(again[0], many[0]) and same(again[1], many[1])
        rm, rm2 = render.rasterize_regions_many([regions, regions[::-1]], 0, radius), render.rasterize_regions_many([regions, regions[::-1]], 0, radius)
        for (b, k), (b2, k2), reg in zip(rm, rm2, (regions, regions[::-1])):
            bh, kh = render.rasterize_regions_host(reg, 0, radius)
            assert same(b, bh) and same(k, kh) and same(b2, b) and same(k2, k)
        im2 = [img, img[::-1]]
        ro = render.render_regions_over_image_many(im2, [regions, regions[::-1]], background_label=0, radius=radius)
        ro2 = render.render_regions_over_image_many(im2, [regions, regions[::-1]], background_label=0, radius=radius)
        for g, a, i_, reg in zip(ro, ro2, im2, (regions, regions[::-1])):
            assert same(g, render.render_regions_over_image_host(i_, reg, background_label=0, radius=radius)) and same(a, g)


def test_objects_outside_the_image_are_refused(gpu):
    from superdsm_amd import render
    for off, frag in (((-1, 3), np.ones((4, 4), bool)), ((3, -2), np.ones((4, 4), bool)), ((28, 3), np.ones((4, 4), bool)), ((3, 38), np.ones((4, 4), bool))):
        with pytest.raises(ValueError, match='outside'):
            render.rasterize_labels_gpu(data_of((30, 40)), [Obj((5, 5), np.ones((3, 3), bool)), Obj(off, frag)])
