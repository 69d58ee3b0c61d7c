"""Image sets on the GPU: the image-set kernels byte-equal to their single-image entry points, ``C2F_RegionAnalysis.process_many``
and ``Pipeline.process_images`` equal to the image-by-image runs, and an image that fails leaving the others' results alone."""
import math

import numpy as np
import pytest
import scipy.ndimage as ndi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    from superdsm_amd import _capi
    _capi.lib()
    return torch


def _bbbc_g(index):
    from superdsm_amd import synth
    spec = synth.WORKLOADS['bbbc039_like']
    shape, layout = synth.bbbc039_like_layout(spec['seed'], index)
    return synth.render_image(shape, layout, spec['seed'] + 7919 * index)


def _bbbc_y(index):
    from superdsm_amd import synth
    return synth.offset_image(_bbbc_g(index), synth.WORKLOADS['bbbc039_like']['scale'])


def _synthetic512():
    from superdsm_amd import synth
    spec = synth.WORKLOADS['synthetic512']
    layout = synth.random_layout(spec['shape'], spec['n'], spec['radius'], spec['seed'], min_sep=1.2)
    return synth.offset_image(synth.render_image(spec['shape'], layout, spec['seed']), spec['scale'])


def _snake(H, W, step=2):
    y = -np.ones((H, W))
    for r in range(0, H, 2 * step):
        y[r, :] = 1
        if r + step < H:
            y[r:r + step + 1, (W - 1) if (r // (2 * step)) % 2 == 0 else 0] = 1
    return y


def _spiral(n):
    y = -np.ones((n, n))
    r0, c0, r1, c1 = 0, 0, n - 1, n - 1
    while r0 <= r1 and c0 <= c1:
        y[r0, c0:c1 + 1] = 1
        y[r0:r1 + 1, c1] = 1
        if r1 > r0 + 1:
            y[r1, c0 + 2:c1 + 1] = 1
        if c1 > c0 + 3 and r1 > r0 + 3:
            y[r0 + 2:r1 + 1, c0 + 2] = 1
        r0, c0, r1, c1 = r0 + 2, c0 + 2, r1 - 2, c1 - 2
    return y


def _mixed_set():
    rng = np.random.default_rng(11)
    ys = [_bbbc_y(i) for i in range(8)] + [_synthetic512()]
    ys += [np.ones((1, 1)), np.where(rng.random((1, 3001)) < 0.6, 1.0, -1.0), np.where(rng.random((2999, 1)) < 0.6, 1.0, -1.0),
           -np.ones((33, 70)), np.ones((45, 61)), _snake(301, 260), _snake(97, 1025, 1), _spiral(257)]
    thrs = [0.2] * 9 + [0.2, 0.5, 0.5, 0.2, 0.2, 0.2, 0.0, 0.2]
    return ys, thrs


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def test_multi_markers_and_edt_equal_the_single_image_entry_points(gpu):
    from superdsm_amd.c2freganal import cluster_markers_gpu, cluster_markers_host, edt_exact_gpu, edt_exact_gpu_multi, markers_and_edt_gpu_multi
    ys, thrs = _mixed_set()
    got = markers_and_edt_gpu_multi(ys, thrs)
    for k, (y, thr, (mask, markers, count, dist)) in enumerate(zip(ys, thrs, got)):
        s_mask, s_markers, _, s_count = cluster_markers_gpu(y, thr)
        assert _bytes(mask) == _bytes(s_mask) and _bytes(markers) == _bytes(s_markers) and count == s_count, k
        assert _bytes(dist) == _bytes(edt_exact_gpu(s_markers)), k
        h_mask, h_markers = cluster_markers_host(y, thr)
        assert np.array_equal(mask, h_mask) and np.array_equal(markers, h_markers) and count == h_markers.max(), k
        assert _bytes(dist) == _bytes(ndi.distance_transform_edt(h_markers == 0)), k
    # the same set in reversed order gives the same bytes per image
    back = markers_and_edt_gpu_multi(ys[::-1], thrs[::-1])[::-1]
    for a, b in zip(got, back):
        assert all(_bytes(x) == _bytes(z) for x, z in zip((a[0], a[1], a[3]), (b[0], b[1], b[3]))) and a[2] == b[2]
    # more images than one call takes: split by the caller, the same results
    twice = markers_and_edt_gpu_multi(ys + ys, thrs + thrs)
    assert len(ys + ys) > 32 and all(_bytes(a[3]) == _bytes(b[3]) for a, b in zip(twice, got + got))
    # EDT of arbitrary targets
    targets = [y > 0 for y in ys] + [np.zeros((17, 23), bool)]
    for t, d in zip(targets, edt_exact_gpu_multi(targets)):
        assert _bytes(d) == _bytes(ndi.distance_transform_edt(~t))


class _Frag:
    def __init__(self, off, frag):
        self.fg_offset, self.fg_fragment = np.asarray(off), np.asarray(frag, bool)
        self.on_boundary = False

    def fill_foreground(self, out, value=True):
        h, w = self.fg_fragment.shape
        out[self.fg_offset[0]:self.fg_offset[0] + h, self.fg_offset[1]:self.fg_offset[1] + w] = value * self.fg_fragment


def _post_images():
    """Three images: ellipses from the BBBC039-like layouts (one touching the border), none, and a striped object whose mask boundary
    (> 12288 pixels) needs the global boundary pool."""
    from superdsm_amd import _morph
    rng = np.random.default_rng(4)
    out = []
    for index in (0, 3):
        g = _bbbc_g(index)
        lab, n = ndi.label(g > 0.3)
        objs = [_Frag((sl[0].start, sl[1].start), lab[sl] == k + 1) for k, sl in enumerate(ndi.find_objects(lab)) if sl is not None][:40]
        objs.append(_Frag((0, 0), np.ones((7, 9), bool)))
        out.append((g, objs))
    out.append((rng.random((200, 300)), []))
    g = rng.random((400, 420)) * 0.3
    frag = np.zeros((220, 210), bool)
    frag[::2] = True
    g[100:320, 120:330][frag] += 0.5
    out.append((g, [_Frag((100, 120), frag)]))
    assert frag.sum() > 12288
    result = []
    for g, objs in out:
        bg = np.zeros(g.shape, bool)
        for o in objs:
            o.fill_foreground(bg)
        result.append((g, objs, _morph.binary_erosion(~bg, _morph.disk(5))))
    return result


@pytest.mark.parametrize('settings', [(5, 5, 1e-4, 1, 2), (3, 2, 1e-4, 2, 1.5), (5, 5, 1e-4, 0, 2)])
def test_post_objects_multi_equals_single(gpu, settings):
    from superdsm_amd import postprocess
    items = []
    for g, objs, bg in _post_images():
        g_dev = gpu.as_tensor(g).cuda()
        items.append((objs, g_dev, postprocess.gaussian_filter_gpu(g_dev, 3), bg))
    got = postprocess.process_objects_gpu_multi(items, *settings)
    assert len(got) == len(items)
    for (objs, g_dev, gs, bg), (recs, refined) in zip(items, got):
        want_recs, want_refined = postprocess.process_objects_gpu(objs, g_dev, gs, bg, *settings)
        assert recs.tobytes() == want_recs.tobytes()
        assert len(refined) == len(want_refined) == len(objs)
        for a, b in zip(refined, want_refined):
            assert (a is None) == (b is None) == (settings[3] == 0)
            if a is not None:
                assert np.array_equal(a[0], b[0]) and a[1].shape == b[1].shape and np.array_equal(a[1], b[1])
    assert len(got[2][0]) == 0 and got[3][0]['area'][0] > 12288


def test_post_objects_of_one_image_and_of_none(gpu):
    """The single-image function is the set of one image: equal to that image's part of a larger set (with an image without objects
    before it), and an image without objects gives empty records whatever stands beside it."""
    from superdsm_amd import _capi, postprocess
    settings = (5, 5, 1e-4, 1, 2)
    items = []
    for g, objs, bg in _post_images():
        g_dev = gpu.as_tensor(g).cuda()
        items.append((objs, g_dev, postprocess.gaussian_filter_gpu(g_dev, 3), bg))
    assert len(items[2][0]) == 0 and len(items[3][0]) == 1
    want = postprocess.process_objects_gpu_multi(items, *settings)
    for k in (0, 3):
        recs, refined = postprocess.process_objects_gpu(*items[k], *settings)
        (recs1, refined1), = postprocess.process_objects_gpu_multi([items[k]], *settings)
        assert recs.dtype == _capi.POST_RECORD_DTYPE and recs.tobytes() == recs1.tobytes() == want[k][0].tobytes() and len(recs) == len(items[k][0])
        for a, b, c in zip(refined, refined1, want[k][1]):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[1], c[1])
    recs, refined = postprocess.process_objects_gpu(*items[2], *settings)
    assert recs.dtype == _capi.POST_RECORD_DTYPE and len(recs) == 0 and refined == []
    assert postprocess.process_objects_gpu_multi([], *settings) == []
    both = postprocess.process_objects_gpu_multi([items[2], items[2]], *settings)
    assert [(len(r), f) for r, f in both] == [(0, []), (0, [])]


def _dsm_cfg():
    from superdsm_amd import synth
    return synth.dsm_config_for_scale(10, 0.00033)


_PARAMS = dict(min_atom_radius=int(0.33 * 10 * math.sqrt(2)))


def _assert_same_c2f(got, want):
    assert np.array_equal(got['y_mask'], want['y_mask'])
    assert np.array_equal(got['clusters'], want['clusters'])
    assert np.array_equal(got['atoms'], want['atoms'])
    assert [tuple(s) for s in got['seeds']] == [tuple(s) for s in want['seeds']]
    ga, wa = got['adjacencies'], want['adjacencies']
    assert ga.atom_labels == wa.atom_labels
    for a in wa.atom_labels:
        assert ga[a] == wa[a] and ga.get_cluster_label(a) == wa.get_cluster_label(a)


def test_c2f_process_many_equals_process(gpu):
    from superdsm_amd import c2freganal as cr, config
    ys = [_bbbc_y(i) for i in range(8)] + [_synthetic512()]
    cfg = config.Config({'c2f-region-analysis': dict(_PARAMS)})
    stage = cr.C2F_RegionAnalysis()
    datas = [dict(y=y, dsm_cfg=_dsm_cfg()) for y in ys]
    stage.process_many(datas, cfg, out='muted')
    counts = []
    for y, data, stats in zip(ys, datas, stage.last_stats):
        want, want_stats = cr.region_analysis_gpu(y, _dsm_cfg(), **_PARAMS)
        _assert_same_c2f(data, want)
        assert len(stats['rounds']) == len(want_stats['rounds']) and stats['clusters'] == want_stats['clusters']
        counts.append(len(want_stats['rounds']))
    assert stage.last_set_stats['n_rounds'] == max(counts) > min(counts) >= 1


def _pipeline_and_configs(imgs):
    from superdsm_amd import automation, config, pipeline
    pl = pipeline.create_reference_pipeline()
    cfgs = [c for c, _ in automation.create_configs(pl, config.Config({'AF_scale': 10}), imgs)]
    return pl, cfgs


def _assert_same_image(got, want):
    from superdsm_amd import render
    _assert_same_c2f(got, want)
    gs, ws = list(got['cover'].solution), list(want['cover'].solution)
    assert [sorted(o.footprint) for o in gs] == [sorted(o.footprint) for o in ws]
    assert [o.energy for o in gs] == [o.energy for o in ws]
    gp, wp = got['postprocessed_objects'], want['postprocessed_objects']
    assert len(gp) == len(wp) > 0
    for a, b in zip(gp, wp):
        assert np.array_equal(a.fg_offset, b.fg_offset) and np.array_equal(a.fg_fragment, b.fg_fragment)
    assert np.array_equal(render.rasterize_labels(got), render.rasterize_labels(want))


def test_process_images_end_to_end_equals_process_image(gpu):
    imgs = [_bbbc_g(i) for i in range(4)]
    pl, cfgs = _pipeline_and_configs(imgs)
    results = pl.process_images(imgs, cfgs, out='muted')
    assert len(results) == 4
    for g, cfg, (data, got_cfg, timings) in zip(imgs, cfgs, results):
        want, want_cfg, want_t = pl.process_image(g, cfg, out='muted')
        _assert_same_image(data, want)
        assert got_cfg.entries == want_cfg.entries and set(timings) == set(want_t)


def test_failed_image_leaves_the_others_alone(gpu, monkeypatch):
    from superdsm_amd import c2freganal as cr
    imgs = [_bbbc_g(i) for i in (1, 2, 5)]
    pl, cfgs = _pipeline_and_configs(imgs)
    wants = [pl.process_image(g, c, out='muted')[0] for g, c in zip(imgs, cfgs)]
    y_bad = wants[1]['y']
    split_cluster = cr._split_cluster

    def split(cluster_label, cluster, masked_cluster, params, flood):
        (r0, c0), (h, w) = (int(v) for v in cluster.offset), cluster.model.shape
        if cluster.model.shape == y_bad[r0:r0 + h, c0:c0 + w].shape and np.array_equal(cluster.model, y_bad[r0:r0 + h, c0:c0 + w]):
            return failing(cluster_label)
        return split_cluster(cluster_label, cluster, masked_cluster, params, flood)

    def failing(cluster_label):
        raise cr.C2FError(f'cluster {cluster_label}: made to fail')
        yield                                              # (a generator, as the split loop is)

    monkeypatch.setattr(cr, '_split_cluster', split)
    with pytest.raises(cr.C2FError) as info:
        pl.process_images(imgs, cfgs, out='muted')
    e = info.value
    assert e.image_index == 1 and e.image_indices == [1] and len(e.results) == 3
    assert 'atoms' not in e.results[1][0] and 'postprocessed_objects' not in e.results[1][0]
    for k in (0, 2):
        data, _, timings = e.results[k]
        _assert_same_image(data, wants[k])
        assert 'postprocess' in timings
