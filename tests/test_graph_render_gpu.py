"""Y-maps, coloured labels, adjacency graphs and the export views on the GPU: byte equality (``np.array_equal`` and equal ``dtype``)
of every function with its ``*_host`` definition, of every ``*_many`` with the single-image call, and of a second launch with the
first.  The colour maps come from tests/golden/colormaps.npz: nothing here needs matplotlib."""
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


@pytest.fixture(scope='module')
def cmaps():
    f = np.load(os.path.join(GOLDEN, 'colormaps.npz'))
    return {name: f[name] for name in ('bwr', 'seismic', 'gist_rainbow')}


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


class Obj:
    def __init__(self, offset, fragment):
        self.fg_offset, self.fg_fragment = np.asarray(offset, int), np.asarray(fragment, bool)

    def fill_foreground(self, out, value=True):
        h, w = self.fg_fragment.shape
        out[self.fg_offset[0]:self.fg_offset[0] + h, self.fg_offset[1]:self.fg_offset[1] + w][self.fg_fragment] = value


def _bbbc_g(index):
    from superdsm_amd import synth
    spec = synth.WORKLOADS['bbbc039_like']
    shape, layout = synth.bbbc039_like_layout(spec['seed'], index)
    return synth.render_image(shape, layout, spec['seed'] + 7919 * index)


@pytest.fixture(scope='module')
def c2f_datas(gpu):
    """The 8 BBBC039-like images through the real preprocessing and the C2F stage: ``y``, ``atoms``, ``clusters``, ``adjacencies``,
    ``seeds``."""
    from superdsm_amd import automation, config, pipeline
    imgs = [_bbbc_g(i) for i in range(8)]
    pl = pipeline.create_reference_pipeline()
    cfgs = [c for c, _ in automation.create_configs(pl, config.Config({'AF_scale': 10}), imgs)]
    return [r[0] for r in pl.process_images(imgs, cfgs, last_stage='c2f-region-analysis', out='muted')]


# ---- y-maps --------------------------------------------------------------------------------------------------------------------------
def test_ymap(gpu, cmaps, c2f_datas):
    from superdsm_amd import render
    rng = np.random.default_rng(0)
    y_real = c2f_datas[0]['y']
    y_inf = rng.standard_normal((61, 83))
    y_inf[rng.random(y_inf.shape) < 0.02] = np.inf
    y_inf[rng.random(y_inf.shape) < 0.02] = -np.inf
    y_nan = rng.standard_normal((40, 70))
    y_nan[17, 33] = np.nan
    squash = lambda v: np.exp(5 * v) / (1 + np.exp(5 * v)) - 0.5
    cases = [(y_real, None, 'bwr'), (c2f_datas[0], None, 'seismic'), (squash(y_real.clip(-0.8, 1)), squash(np.array([-0.8, 1.])), 'seismic'),
             (y_inf, (-1.5, 0.5), 'bwr'), (y_nan, None, 'bwr'), (y_nan, (-1, 1), 'gist_rainbow'), (np.full((30, 31), 0.25), None, 'bwr'),
             (np.full((30, 31), 0.25), (0, 1), 'bwr'), (rng.standard_normal((9, 2)), (0.5, 0.5), 'bwr'), (rng.standard_normal((9, 20)), (0.5, -0.5), 'seismic')]
    for k, (y, clim, name) in enumerate(cases):
        want = render.render_ymap_host(y, clim=clim, cmap=cmaps[name])
        got = render.render_ymap(y, clim=clim, cmap=cmaps[name])
        assert got.dtype == np.float64 and same(got, want), (k, int((got != want).sum()))
        assert same(render.render_ymap(y, clim=clim, cmap=cmaps[name]), got)
    bad = np.broadcast_to(cmaps['bwr'][-1, :3], y_nan.shape + (3,))
    assert same(render.render_ymap(y_nan, cmap=cmaps['bwr']), bad.copy())            # a single NaN: every pixel "bad"
    assert same(render.render_ymap(np.full((30, 31), 0.25), cmap=cmaps['bwr']), np.broadcast_to(cmaps['bwr'][-1, :3], (30, 31, 3)).copy())
    # a small table: N = 5
    t5 = rng.random((8, 4))
    assert same(render.render_ymap(y_inf, clim=(-2, 2), cmap=t5), render.render_ymap_host(y_inf, clim=(-2, 2), cmap=t5))


def test_ymap_many(gpu, cmaps, c2f_datas):
    from superdsm_amd import render
    for clim in (None, (-0.3, 0.4)):
        many = render.render_ymap_many(c2f_datas, clim=clim, cmap=cmaps['bwr'])
        assert len(many) == 8
        for d, m in zip(c2f_datas, many):
            assert same(m, render.render_ymap(d, clim=clim, cmap=cmaps['bwr']))
        assert same(many[3], render.render_ymap_host(c2f_datas[3], clim=clim, cmap=cmaps['bwr']))
    rng = np.random.default_rng(1)
    ys = [rng.standard_normal((20 + 3 * k, 70 - k)) for k in range(33)]                # 33 images: one more than a launch takes
    ys[7][3, 3] = np.nan
    many, again = render.render_ymap_many(ys, cmap=cmaps['seismic']), render.render_ymap_many(ys, cmap=cmaps['seismic'])
    assert len(many) == 33
    for y, m, a in zip(ys, many, again):
        assert same(m, render.render_ymap(y, cmap=cmaps['seismic'])) and same(a, m)
    for k in (0, 7, 32):
        assert same(many[k], render.render_ymap_host(ys[k], cmap=cmaps['seismic']))


# ---- labels --------------------------------------------------------------------------------------------------------------------------
def disc_objects(shape, n, rmin, rmax, seed):
    rng = np.random.default_rng(seed)
    H, W = shape
    objs = []
    for _ in range(n):
        r = int(rng.integers(rmin, rmax + 1))
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        r0, r1, c0, c1 = max(0, cy - r), min(H, cy + r + 1), max(0, cx - r), min(W, cx + r + 1)
        yy, xx = np.mgrid[r0:r1, c0:c1]
        objs.append(Obj((r0, c0), (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r))
    return objs


def label_maps(render):
    f = np.load(os.path.join(GOLDEN, 'render.npz'))
    shape = tuple(int(v) for v in f['shape'])
    objs = [Obj(f[f'o{k}_offset'], f[f'o{k}_fragment']) for k in range(int(f['n']))]
    out = [render.rasterize_labels_gpu({'g_raw': np.zeros(shape)}, objs)]
    out.append(render.rasterize_labels_gpu({'g_raw': np.zeros((96, 128))}, disc_objects((96, 128), 40, 5, 14, 1)))
    out.append(render.rasterize_labels_gpu({'g_raw': np.zeros((50, 61))}, disc_objects((50, 61), 25, 1, 4, 4), background_label=-1))
    return out


def test_colorize_and_shuffle(gpu, cmaps):
    from superdsm_amd import render
    t = cmaps['gist_rainbow']
    maps = label_maps(render)
    assert all(m.dtype == np.uint16 and len(np.unique(m)) > 3 for m in maps)
    rng = np.random.default_rng(2)
    maps.append((rng.integers(-5, 9, (33, 47)) * 7).astype(np.int32))                  # negative labels, gaps
    maps.append(np.full((20, 25), 7, np.uint16))                                       # one label
    maps.append(np.zeros((20, 25), np.int64))                                          # background only
    for k, lab in enumerate(maps):
        for kw in (dict(), dict(shuffle=3), dict(bg_label=None), dict(bg_label=None, shuffle=11), dict(bg_label=7, bg_color=(0.2, 0.4, 1), shuffle=0),
                   dict(bg_label=65535, bg_color=(1, 1, 1))):
            want = render.colorize_labels_host(lab, cmap=t, **kw)
            got = render.colorize_labels(lab, cmap=t, **kw)
            assert got.dtype == np.float64 and same(got, want), (k, kw, int((got != want).sum()))
            assert same(render.colorize_labels(lab, cmap=t, **kw), got)
        for kw in (dict(seed=4), dict(seed=4, bg_label=0), dict(seed=5, bg_label=7)):
            want = render.shuffle_labels_host(lab, **kw)
            got = render.shuffle_labels(lab, **kw)
            assert same(got, want), (k, kw)
    one = render.colorize_labels(maps[4], cmap=t, bg_label=0)
    assert same(one, np.broadcast_to(t[-1, :3], one.shape).copy())                     # max == min: "bad" everywhere
    many, again = render.colorize_labels_many(maps, cmap=t, shuffle=3), render.colorize_labels_many(maps, cmap=t, shuffle=3)
    for lab, m, a in zip(maps, many, again):
        assert same(m, render.colorize_labels(lab, cmap=t, shuffle=3)) and same(a, m)
    for lab, m in zip(maps, render.shuffle_labels_many(maps, bg_label=0, seed=8)):
        assert same(m, render.shuffle_labels(lab, bg_label=0, seed=8))


def test_colorize_many_of_pipeline_label_images(gpu, cmaps, c2f_datas):
    from superdsm_amd import render
    t = cmaps['gist_rainbow']
    atoms = [d['atoms'] for d in c2f_datas]
    for kw in (dict(), dict(shuffle=1)):
        many = render.colorize_labels_many(atoms, cmap=t, **kw)
        assert len(many) == 8
        for a, m in zip(atoms, many):
            assert same(m, render.colorize_labels(a, cmap=t, **kw))
        assert same(many[5], render.colorize_labels_host(atoms[5], cmap=t, **kw))
    rng = np.random.default_rng(3)
    labs = [rng.integers(0, 4 + k, (20 + 3 * k, 70 - k)).astype(np.uint16) for k in range(33)]
    many, again = render.colorize_labels_many(labs, cmap=t, shuffle=2), render.colorize_labels_many(labs, cmap=t, shuffle=2)
    assert len(many) == 33
    for l, m, a in zip(labs, many, again):
        assert same(m, render.colorize_labels(l, cmap=t, shuffle=2)) and same(a, m)
    for k in (0, 31, 32):
        assert same(many[k], render.colorize_labels_host(labs[k], cmap=t, shuffle=2))


# ---- adjacency graphs ----------------------------------------------------------------------------------------------------------------
def check_graph(render, data, **kw):
    want = render.render_adjacencies_host(data, **kw)
    got = render.render_adjacencies(data, **kw)
    again = render.render_adjacencies(data, **kw)
    assert got.dtype == np.uint8 and same(got, want), (sorted(kw), int((got != want).any(axis=2).sum()))
    assert same(again, got)
    return got


def test_adjacencies_of_the_c2f_stage(gpu, c2f_datas):
    from superdsm_amd import render
    for data in c2f_datas[:2]:
        lines = data['adjacencies'].get_edge_lines()
        assert len(lines) > 0 and len(data["seeds"]) > 20
        base = check_graph(render, data, lines=lines)
        assert same(render.render_adjacencies(data), base)                             # the same list, fetched by the function
        check_graph(render, data, lines=lines, edge_thickness=2.5, edge_color=(0, 1, 0.5), normalize_img=False)
        check_graph(render, data, lines=lines, edge_thickness=1, endpoint_radius=2, endpoint_edge_thickness=1)


def synthetic_graph(shape=(1024, 1024), n_seeds=60, n_edges=220, seed=0):
    rng = np.random.default_rng(seed)
    H, W = shape
    seeds = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H - 1, W // 3), (H // 3, W - 1)]
    seeds += [(int(rng.integers(0, H)), int(rng.integers(0, W))) for _ in range(n_seeds - len(seeds))]
    lines = [(seeds[0], seeds[3]), (seeds[1], seeds[2]), (seeds[0], seeds[1]), (seeds[2], seeds[3]), (seeds[0], seeds[2]), (seeds[4], seeds[4])]
    while len(lines) < n_edges:
        a, b = rng.integers(0, len(seeds), 2)
        lines.append((seeds[a], seeds[b]))
    return {'g_raw': rng.random(shape) * 3 - 0.5, 'seeds': seeds}, lines


@pytest.mark.parametrize('thickness', [1, 3, 2.5])
def test_adjacencies_synthetic_graph(gpu, thickness):
    from superdsm_amd import render
    data, lines = synthetic_graph()
    assert len(lines) >= 200
    kw = dict(lines=lines, edge_thickness=thickness, edge_color=(0.9, 0.3, 0.1), endpoint_color=(0, 0, 1), endpoint_edge_color=(1, 1, 0.5))
    check_graph(render, data, **kw)
    rng = np.random.default_rng(7)
    check_graph(render, data, override_img=rng.integers(0, 256, (1024, 1024, 3)).astype(np.uint8), **kw)
    if thickness == 3:
        check_graph(render, data, override_img=rng.random((1024, 1024, 4)), endpoint_radius=12.5, endpoint_edge_thickness=3, **kw)


def test_adjacencies_small_cases(gpu):
    from superdsm_amd import render
    rng = np.random.default_rng(5)
    data = {'g_raw': rng.random((70, 90)), 'seeds': [(10, 10), (60, 80), (35, 45), (0, 89), (69, 0)]}
    lines = [((10, 10), (60, 80)), ((60, 80), (10, 10)), ((35, 45), (0, 89)), ((69, 0), (0, 89)), ((10, 10), (10, 80)), ((69, 0), (10, 0)), ((35, 45), (35, 45))]
    for thickness in (1, 1.5, 2, 3, 4, 5, 7.25, 16, 33):
        check_graph(render, data, lines=lines, edge_thickness=thickness)
    check_graph(render, data, lines=lines, endpoint_radius=40, endpoint_edge_thickness=24)       # the largest rim
    check_graph(render, data, lines=lines, endpoint_radius=0, endpoint_edge_thickness=0)
    check_graph(render, data, lines=[])
    check_graph(render, dict(data, seeds=[]), lines=lines)
    check_graph(render, {'g_raw': rng.random((1, 40)), 'seeds': [(0, 5)]}, lines=[((0, 5), (0, 39))])


def test_adjacencies_many(gpu, c2f_datas):
    from superdsm_amd import render
    lines = [d['adjacencies'].get_edge_lines() for d in c2f_datas]
    many, again = render.render_adjacencies_many(c2f_datas, lines=lines), render.render_adjacencies_many(c2f_datas, lines=lines)
    assert len(many) == 8
    for d, l, m, a in zip(c2f_datas, lines, many, again):
        assert same(m, render.render_adjacencies(d, lines=l)) and same(a, m)
    assert same(many[6], render.render_adjacencies_host(c2f_datas[6], lines=lines[6]))
    rng = np.random.default_rng(9)
    datas, lls = [], []
    for k in range(33):
        shape = (40 + 3 * k, 120 - k)
        seeds = [(int(rng.integers(0, shape[0])), int(rng.integers(0, shape[1]))) for _ in range(4 + k % 5)]
        datas.append({'g_raw': rng.random(shape), 'seeds': seeds})
        lls.append([(seeds[i], seeds[(i + 1 + k % 2) % len(seeds)]) for i in range(len(seeds))])
    overs = [rng.random(d['g_raw'].shape + (3,)) if k % 3 == 0 else None for k, d in enumerate(datas)]
    many = render.render_adjacencies_many(datas, lines=lls, override_imgs=overs, edge_thickness=2)
    again = render.render_adjacencies_many(datas, lines=lls, override_imgs=overs, edge_thickness=2)
    assert len(many) == 33
    for d, l, o, m, a in zip(datas, lls, overs, many, again):
        assert same(m, render.render_adjacencies(d, lines=l, override_img=o, edge_thickness=2)) and same(a, m)
    for k in (0, 16, 32):
        assert same(many[k], render.render_adjacencies_host(datas[k], lines=lls[k], override_img=overs[k], edge_thickness=2))


# ---- the export views ----------------------------------------------------------------------------------------------------------------
def test_export_views(gpu, c2f_datas, monkeypatch):
    """``ymap`` names a colour map by name (matplotlib); the GPU machine may lack it, so names are resolved from the fixture."""
    from superdsm_amd import render
    f = np.load(os.path.join(GOLDEN, 'colormaps.npz'))
    table_of = render.colormap_table
    monkeypatch.setattr(render, 'colormap_table', lambda cmap: f[cmap] if isinstance(cmap, str) else table_of(cmap))
    datas = c2f_datas[:3]
    for mode, kw in (('fgc', {}), ('adj', {}), ('atm', {}), ('atm', dict(enhance=True, border=4)), ('adj', dict(border=6, ymap='-0.5:+0.5:3:bwr')), ('fgc', dict(ymap='/-1:+1:2:seismic'))):
        want = render.export_views(datas, mode, host=True, **kw)
        got = render.export_views(datas, mode, **kw)
        assert len(got) == 3
        for w, g in zip(want, got):
            assert g.dtype == np.uint8 and same(g, w), (mode, kw, int((g != w).any(axis=2).sum()))
    adj = render.export_views(datas[:1], 'adj')[0]
    assert (adj == np.array([0, 255, 0], np.uint8)).all(axis=2).sum() > 100            # green edges and end points were painted


# ---- limits ------------------------------------------------------------------------------------------------------------------------
def test_limits_raise_before_anything_is_launched(gpu, cmaps):
    from superdsm_amd import render
    data = {'g_raw': np.random.default_rng(0).random((30, 30)), 'seeds': [(5, 5)]}
    with pytest.raises(NotImplementedError, match='Limits'):
        render.render_adjacencies(data, lines=[], endpoint_radius=60, endpoint_edge_thickness=5)
    with pytest.raises(NotImplementedError, match='Limits'):
        render.render_adjacencies(data, lines=[], edge_thickness=33.5)
    with pytest.raises(ValueError, match='outside'):
        render.render_adjacencies(dict(data, seeds=[(5, 30)]), lines=[])
    with pytest.raises(ValueError, match='outside'):
        render.render_adjacencies(data, lines=[((5, 5), (-1, 5))])
    with pytest.raises(ValueError, match='65535'):
        render.render_adjacencies(dict(data, seeds=[(1, 1)] * 65536), lines=[])
    with pytest.raises(NotImplementedError, match='Limits'):
        render.render_ymap(np.zeros((5, 5)), cmap=np.zeros((1028, 4)))
    with pytest.raises(NotImplementedError, match='Limits'):
        render.render_ymap(np.zeros((5, 5), np.float32), cmap=cmaps['bwr'])
    with pytest.raises(NotImplementedError, match='Limits'):
        render.colorize_labels(np.array([[0, 2 ** 25]], np.int32), cmap=cmaps['bwr'], bg_label=None, shuffle=1)
    with pytest.raises(ValueError, match='int32'):
        render.colorize_labels(np.array([[0, 2 ** 40]], np.int64), cmap=cmaps['bwr'])
