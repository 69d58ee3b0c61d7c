"""Image sets without a GPU: the orchestration of ``Pipeline.process_images`` with fake stages, ``automation.create_configs`` with
``AF_scale`` set, and the host side of the image-set entry points of the C ABI (workspace queries, argument checks, table layouts)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- orchestration with fake stages ----------------------------------------------------------------------------------------------

class _Failure(Exception):
    pass


def _fake_stages():
    """Three stages: 'a' (image by image), 'b' (with process_many), 'c' (image by image); every call is logged."""
    from superdsm_amd.pipeline import Stage

    calls = []

    class A(Stage):
        def __init__(self):
            super().__init__('a', inputs=['g_raw'], outputs=['x'])

        def process(self, input_data, cfg, out, log_root_dir):
            calls.append(('a', float(input_data['g_raw'].sum()), cfg.get('factor', 1)))
            return {'x': input_data['g_raw'] * cfg.get('factor', 1)}

    class B(Stage):
        def __init__(self):
            super().__init__('b', inputs=['x'], outputs=['z'])

        def process(self, input_data, cfg, out, log_root_dir):
            calls.append(('b-one', float(input_data['x'].sum()), cfg.get('fail', False)))
            return {'z': input_data['x'] + 1}

        def process_many(self, datas, cfg, out=None, log_root_dirs=None):
            cfgs = list(cfg) if isinstance(cfg, (list, tuple)) else [cfg] * len(datas)
            calls.append(('b-many', [float(d['x'].sum()) for d in datas]))
            failed = []
            for i, (d, c) in enumerate(zip(datas, cfgs)):
                if c.get(self.cfgns, {}).get('fail', False):
                    failed.append(i)
                    continue
                d['z'] = d['x'] + 1
            if failed:
                from superdsm_amd.c2freganal import C2FError
                e = C2FError(f'image {failed[0]} failed')
                e.image_index, e.image_indices = failed[0], failed
                raise e
            return 0.5

    class Cst(Stage):
        def __init__(self):
            super().__init__('c', inputs=['z'], outputs=['w'])

        def process(self, input_data, cfg, out, log_root_dir):
            calls.append(('c', float(input_data['z'].sum())))
            return {'w': input_data['z'] * 2}

    return [A(), B(), Cst()], calls


def _pipeline():
    from superdsm_amd.pipeline import create_pipeline
    stages, calls = _fake_stages()
    return create_pipeline(stages), calls


def _images(n):
    return [(np.arange(12.0).reshape(3, 4) + 1) ** (k + 1) for k in range(n)]       # different after normalize_image


def _cfg(**kw):
    from superdsm_amd.config import Config
    return Config(kw)


def _norm(g):
    from superdsm_amd.image import normalize_image
    return normalize_image(g)


def _same_data(got, want):
    return set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)


def test_process_many_runs_once_with_all_images_in_order_the_others_per_image():
    pl, calls = _pipeline()
    imgs = _images(3)
    results = pl.process_images(imgs, _cfg(), out='muted')
    assert [c[0] for c in calls] == ['a', 'a', 'a', 'b-many', 'c', 'c', 'c']
    assert calls[3][1] == [float(_norm(g).sum()) for g in imgs]
    assert len(results) == 3
    for g, (data, cfg, timings) in zip(imgs, results):
        want, want_cfg, want_t = _pipeline()[0].process_image(g, _cfg(), out='muted')
        assert _same_data(data, want) and cfg.entries == want_cfg.entries
        assert set(timings) == set(want_t) == {'a', 'b', 'c'}
        assert timings['b'] == pytest.approx(0.5 / 3, abs=0.05)   # the set's wall time, shared evenly


def test_empty_set():
    pl, calls = _pipeline()
    assert pl.process_images([], _cfg()) == []
    assert calls == []


def test_per_image_configs_reach_their_images():
    pl, calls = _pipeline()
    imgs = _images(3)
    results = pl.process_images(imgs, [_cfg(a={'factor': k + 2}) for k in range(3)], out='muted')
    assert [c[2] for c in calls if c[0] == 'a'] == [2, 3, 4]
    for k, (data, cfg, _) in enumerate(results):
        assert cfg['a/factor'] == k + 2
        assert np.array_equal(data['x'], _norm(imgs[k]) * (k + 2))


def test_disabled_stages_fire_skip_per_image():
    pl, calls = _pipeline()
    events = []
    for stage in pl.stages:
        for name in ('start', 'end', 'skip'):
            stage.add_callback(name, lambda ev, data, s=stage.name: events.append((s, ev)))
    results = pl.process_images(_images(2), [_cfg(b={'enabled': False}), _cfg(b={'enabled': False})], last_stage='b', out='muted')
    assert events.count(('b', 'skip')) == 2 and ('b', 'start') not in events
    assert events.count(('a', 'start')) == events.count(('a', 'end')) == 2
    assert not any(c[0].startswith('b') for c in calls)
    assert all(t['b'] == 0 for _, _, t in results)
    # the stage disabled for one image only: process_many sees the other one
    pl, calls = _pipeline()
    pl.process_images(_images(2), [_cfg(b={'enabled': False}), _cfg()], last_stage='b', out='muted')
    assert [c for c in calls if c[0] == 'b-many'] == [('b-many', [float(_norm(_images(2)[1]).sum())])]


@pytest.mark.parametrize('first_stage, last_stage', [(None, None), ('a', 'a'), (None, 'b'), ('b', None), ('a+', 'b'), ('b+', None),
                                                     ('c', 'a'), ('a', None), ('c', 'c')])
def test_stage_selection_as_process_image(first_stage, last_stage):
    imgs = _images(2)
    datas = [d for d, _, _ in _pipeline()[0].process_images(imgs, _cfg(), out='muted')]
    got = _pipeline()[0].process_images(imgs, _cfg(), first_stage=first_stage, last_stage=last_stage, datas=[dict(d) for d in datas],
                                        out='muted')
    for k, (data, _, timings) in enumerate(got):
        want, _, want_t = _pipeline()[0].process_image(imgs[k], _cfg(), first_stage=first_stage, last_stage=last_stage,
                                                       data=dict(datas[k]), out='muted')
        assert set(timings) == set(want_t)
        assert _same_data(data, want)


def test_failure_isolation():
    from superdsm_amd.c2freganal import C2FError
    pl, calls = _pipeline()
    imgs = _images(4)
    with pytest.raises(C2FError) as info:
        pl.process_images(imgs, [_cfg(), _cfg(b={'fail': True}), _cfg(), _cfg(b={'fail': True})], out='muted')
    e = info.value
    assert e.image_index == 1 and e.image_indices == [1, 3]
    assert len(e.results) == 4
    # the failed images leave the set: stage 'c' ran for images 0 and 2 only
    assert [c[1] for c in calls if c[0] == 'c'] == [float((_norm(imgs[k]) + 1).sum()) for k in (0, 2)]
    for k in (0, 2):
        data, _, timings = e.results[k]
        assert _same_data(data, _pipeline()[0].process_image(imgs[k], _cfg(), out='muted')[0]) and set(timings) == {'a', 'b', 'c'}
    for k in (1, 3):
        data, _, timings = e.results[k]
        assert 'z' not in data and 'w' not in data and 'c' not in timings


def test_failure_of_a_per_image_stage_is_isolated_too():
    from superdsm_amd.objects import CvxprogError
    pl, _ = _pipeline()
    stage_c = pl.stages[2]
    process = stage_c.process
    first = float((_norm(_images(3)[0]) + 1).sum())

    def failing(input_data, cfg, out, log_root_dir):
        if float(input_data['z'].sum()) == first:
            raise CvxprogError(cidx=7)
        return process(input_data, cfg, out, log_root_dir)

    stage_c.process = failing
    with pytest.raises(CvxprogError) as info:
        pl.process_images(_images(3), _cfg(), out='muted')
    assert info.value.image_index == 0 and info.value.image_indices == [0]
    assert 'w' not in info.value.results[0][0] and all('w' in info.value.results[k][0] for k in (1, 2))


def test_other_errors_are_not_isolated():
    pl, _ = _pipeline()

    def broken(input_data, cfg, out, log_root_dir):
        raise _Failure('not a failure of one image')

    pl.stages[0].process = broken
    with pytest.raises(_Failure):
        pl.process_images(_images(2), _cfg(), out='muted')


# ---- create_configs ----------------------------------------------------------------------------------------------------------------

def test_create_configs_with_af_scale_equals_create_config():
    from superdsm_amd import automation, pipeline
    pl = pipeline.create_reference_pipeline()
    base = _cfg(AF_scale=11.5)
    got = automation.create_configs(pl, base, _images(3))
    want_cfg, want_scale = automation.create_config(pl, base)
    assert len(got) == 3
    for cfg, scale in got:
        assert scale == want_scale == 11.5
        assert cfg.entries == want_cfg.entries
    assert got[0][0] is not got[1][0]
    assert automation.create_configs(pl, base, []) == []


# ---- C ABI of the image-set entry points (host side only) --------------------------------------------------------------------------

def _table(shapes):
    from superdsm_amd import _capi
    t = (_capi.SetImage * max(1, len(shapes)))()
    off = 0
    for k, (h, w) in enumerate(shapes):
        t[k].offset, t[k].H, t[k].W = off, h, w
        off += h * w
    return t


def _fields(header, name):
    body = re.search(r'typedef struct \{([^{}]*)\} ' + name + ';', header).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    return [n for decl in body.split(';') if decl.strip() for n in re.findall(r'(\w+)\s*(?=,|$)', decl.strip())]


def test_set_table_layouts_match_the_header():
    from superdsm_amd import _capi
    header = open(os.path.join(ROOT, 'include', 'sdsm.h')).read()
    assert int(re.search(r'#define SDSM_MAX_SET_IMAGES (\d+)', header).group(1)) == _capi.MAX_SET_IMAGES >= 16
    assert C.sizeof(_capi.SetImage) == 16
    assert [(n, getattr(_capi.SetImage, n).offset) for n, _ in _capi.SetImage._fields_] == [('offset', 0), ('H', 8), ('W', 12)]
    assert C.sizeof(_capi.PostImage) == 48
    assert [(n, getattr(_capi.PostImage, n).offset) for n, _ in _capi.PostImage._fields_] == [
        ('d_g', 0), ('d_gs', 8), ('d_bg', 16), ('H', 24), ('W', 28), ('inv_gstd', 32), ('n_objects', 40), ('reserved', 44)]
    assert _fields(header, 'sdsm_set_image') == [n for n, _ in _capi.SetImage._fields_]
    assert _fields(header, 'sdsm_post_image') == [n for n, _ in _capi.PostImage._fields_]


def test_multi_workspace_queries_are_host_only_and_monotone():
    from superdsm_amd import _capi
    L = _capi.lib()
    shapes = [(520, 696), (1, 1), (1, 4099), (4099, 1), (512, 512), (33, 70)]
    for query, single in ((L.sdsm_c2f_markers_workspace_bytes_multi, L.sdsm_c2f_markers_workspace_bytes),
                          (L.sdsm_edt_exact_workspace_bytes_multi, L.sdsm_edt_exact_workspace_bytes)):
        sizes = [query(_table(shapes[:k]), k) for k in range(1, len(shapes) + 1)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[0] >= single(*shapes[0]) > 0
        assert all(sizes[-1] >= single(*sh) for sh in shapes)
        assert query(_table([]), 0) == 0
        assert query(_table(shapes * 6), len(shapes) * 6) == 0          # 36 > SDSM_MAX_SET_IMAGES
        assert query(None, 1) == 0
        assert query(_table([(0, 5)]), 1) == 0
    assert L.sdsm_edt_exact_workspace_bytes_multi(_table([(65536, 1)]), 1) == 0
    assert L.sdsm_c2f_markers_workspace_bytes_multi(_table([(65536, 1)]), 1) > 0


def test_multi_entry_points_refuse_bad_arguments():
    from superdsm_amd import _capi
    L = _capi.lib()
    fake = C.c_void_p(4096)                              # never dereferenced: every call below fails its checks first
    t = _table([(10, 12), (3, 4)])
    thr = (C.c_double * 2)(0.2, 0.2)
    big = 1 << 30
    ARG, WS = -1, -3

    def markers(table, n, thr=thr, ws=big, y=fake):
        return L.sdsm_c2f_markers_multi(table, n, y, thr, fake, fake, fake, fake, ws, None)

    def edt(table, n, ws=big, target=fake):
        return L.sdsm_edt_exact_multi(table, n, target, fake, fake, ws, None)

    assert markers(t, 0) == ARG and markers(t, 33) == ARG and markers(None, 2) == ARG
    assert markers(t, 2, thr=None) == ARG and markers(t, 2, y=None) == ARG
    assert markers(_table([(10, 12), (0, 4)]), 2) == ARG
    neg = _table([(10, 12)])
    neg[0].offset = -1
    assert markers(neg, 1) == ARG and edt(neg, 1) == ARG
    assert markers(_table([(46341, 46341)]), 1) == ARG                # H * W >= 2^31
    assert markers(t, 2, ws=16) == WS
    assert 'workspace' in L.sdsm_last_error().decode()
    assert edt(t, 0) == ARG and edt(t, 33) == ARG and edt(t, 2, target=None) == ARG
    assert edt(_table([(65536, 2)]), 1) == ARG and edt(t, 2, ws=16) == WS

    ims = (_capi.PostImage * 2)()
    for k in range(2):
        ims[k].d_g = ims[k].d_gs = ims[k].d_bg = 4096
        ims[k].H, ims[k].W, ims[k].inv_gstd, ims[k].n_objects = 20, 30, 1.0, 1

    def post(images, n, max_distance=1, exterior_scale=5.0, boxes=fake, pool=None):
        return L.sdsm_post_objects_multi(images, n, boxes, fake, fake, fake, fake, pool, None, exterior_scale, 5.0, 1e-4, max_distance,
                                         2.0, fake, None)

    assert post(ims, 0) == ARG and post(ims, 33) == ARG and post(None, 1) == ARG
    assert post(ims, 2, max_distance=17) == ARG and post(ims, 2, exterior_scale=0.0) == ARG
    assert post(ims, 2, boxes=None) == ARG and post(ims, 2, pool=fake) == ARG
    ims[1].n_objects = -1
    assert post(ims, 2) == ARG
    ims[1].n_objects, ims[1].H = 1, 0
    assert post(ims, 2) == ARG
    ims[1].H, ims[1].d_g = 20, None
    assert post(ims, 2) == ARG
    ims[0].n_objects = ims[1].n_objects = 0                # no objects at all: nothing to do, whatever the per-object arrays
    assert post(ims, 2, boxes=None) == 0
