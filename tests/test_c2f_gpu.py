"""The coarse-to-fine region analysis on the GPU: the markers and exact-EDT kernels against SciPy, byte for byte, and the lock-step stage
against the sequential restatement."""
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


def _bbbc_y(index):
    from superdsm_amd import synth
    spec = synth.WORKLOADS['bbbc039_like']
    shape, layout = synth.bbbc039_like_layout(spec['seed'], index)
    seed = spec['seed'] + 7919 * index
    return synth.offset_image(synth.render_image(shape, layout, seed), spec['scale'])


_CACHE = {}


def _synthetic_y(workload):
    if workload not in _CACHE:
        from superdsm_amd import synth
        spec = synth.WORKLOADS[workload]
        layout = synth.random_layout(spec['shape'], spec['n'], spec['radius'], spec['seed'],
                                     min_sep={'synthetic4096': 0.6, 'synthetic512': 1.2}[workload])
        _CACHE[workload] = synth.offset_image(synth.render_image(spec['shape'], layout, spec['seed']), spec['scale'])
    return _CACHE[workload]


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


def _marker_cases():
    rng = np.random.default_rng(5)
    cases = []
    for d in (0.05, 0.3, 0.5, 0.59, 0.7, 0.95):
        cases.append((f'random{d}', np.where(rng.random((203, 317)) < d, rng.random((203, 317)) + 0.01, -rng.random((203, 317)))))
    cases += [('snake', _snake(301, 260)), ('snake1', _snake(97, 1025, 1)), ('spiral', _spiral(257)),
              ('row', np.where(rng.random((1, 4099)) < 0.6, 1.0, -1.0)), ('col', np.where(rng.random((4099, 1)) < 0.6, 1.0, -1.0)),
              ('odd', np.where(rng.random((67, 129)) < 0.55, 1.0, 0.0)), ('one', np.ones((1, 1))), ('allfg', np.ones((33, 70))),
              ('allbg', -np.ones((33, 70))), ('zeros', np.zeros((40, 41)))]
    cases += [(f'bbbc{i}', _bbbc_y(i)) for i in range(8)]
    return cases


def test_markers_kernel_equals_scipy(gpu):
    from superdsm_amd.c2freganal import cluster_markers_gpu, cluster_markers_host
    for name, y in _marker_cases():
        for thr in (0.2, 0.5, 0.0, -1.0):
            want_mask, want = cluster_markers_host(y, thr)
            got_mask, got, _, count = cluster_markers_gpu(y, thr)
            assert np.array_equal(got_mask, want_mask), (name, thr)
            assert np.array_equal(got, want), (name, thr)
            assert count == want.max(), (name, thr)


def test_markers_kernel_equals_scipy_4096(gpu):
    from superdsm_amd.c2freganal import cluster_markers_gpu, cluster_markers_host
    y = _synthetic_y('synthetic4096')
    want_mask, want = cluster_markers_host(y, 0.2)
    got_mask, got, _, count = cluster_markers_gpu(y, 0.2)
    assert np.array_equal(got_mask, want_mask) and np.array_equal(got, want) and count == want.max() > 1000


def test_exact_edt_equals_scipy(gpu):
    from superdsm_amd.c2freganal import edt_exact_gpu
    cases = [(name, y > 0) for name, y in _marker_cases()]
    one = np.zeros((97, 131), bool)
    one[40, 77] = True
    corners = np.zeros((150, 99), bool)
    corners[0, 0] = corners[-1, -1] = corners[0, -1] = True
    far = np.zeros((1, 3000), bool)
    far[0, 0] = True
    big = np.zeros((1500, 1600), bool)
    big[0, 0] = True
    big[1499, 3] = True
    cases += [('one', one), ('corners', corners), ('far', far), ('farT', far.T.copy()), ('big', big), ('none', np.zeros((17, 23), bool))]
    for name, t in cases:
        got = edt_exact_gpu(t)
        want = ndi.distance_transform_edt(~t)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), name
    assert edt_exact_gpu(big).max() > 1000


def test_exact_edt_equals_scipy_4096(gpu):
    from superdsm_amd.c2freganal import edt_exact_gpu
    y = _synthetic_y('synthetic4096')
    for t in (y > 0, np.pad(np.ones((1, 1), bool), ((0, 4095), (0, 4095)))):
        assert np.array_equal(edt_exact_gpu(t).view(np.uint64), ndi.distance_transform_edt(~t).view(np.uint64))


def _dsm_cfg():
    from superdsm_amd import synth
    return synth.dsm_config_for_scale(10, 0.00033)


_PARAMS = dict(min_atom_radius=int(0.33 * 10 * math.sqrt(2)))


def _assert_same(got, want):
    assert np.array_equal(got['y_mask'], want['y_mask'])
    assert np.array_equal(got['clusters'], want['clusters'])
    assert np.array_equal(got['atoms'], want['atoms'])
    assert [tuple(s) for s in got['seeds']] == [tuple(s) for s in want['seeds']]
    ga, wa = got['adjacencies'], want['adjacencies']
    assert ga.atom_labels == wa.atom_labels
    for a in wa.atom_labels:
        assert ga[a] == wa[a] and ga.get_cluster_label(a) == wa.get_cluster_label(a)


@pytest.mark.parametrize('image', [f'bbbc{i}' for i in range(8)] + ['synthetic512'])
def test_stage_equals_sequential_restatement(gpu, image):
    from superdsm_amd import c2freganal as cr
    y = _bbbc_y(int(image[4:])) if image.startswith('bbbc') else _synthetic_y(image)
    got, stats = cr.region_analysis_gpu(y, _dsm_cfg(), **_PARAMS)
    want = cr.region_analysis_host(y, _dsm_cfg(), energy=cr.normalized_energy_one, **_PARAMS)
    _assert_same(got, want)
    assert got['atoms'].max() > stats['clusters'] > 10
    resolves = sum(r['resolve_plans'] for r in stats['rounds'])
    assert stats['launches'] <= len(stats['rounds']) * math.ceil(stats['clusters'] / cr.MAX_CROPS_PER_PLAN) + resolves


def test_given_up_candidates_are_solved_again(gpu):
    """Regions larger than one workgroup get a workgroup group in latency mode; with a timeout of ~0 the groups give up and the
    candidates are solved again without groups."""
    from superdsm_amd import _capi, c2freganal as cr
    rng = np.random.default_rng(3)
    rr, cc = np.mgrid[:260, :300]
    y = -0.1 + 0.01 * rng.standard_normal(rr.shape)
    y += 0.6 * np.exp(-(((rr - 120) / 70.0) ** 2 + ((cc - 140) / 80.0) ** 2) ** 2)
    y += 0.5 * np.exp(-(((rr - 130) / 40.0) ** 2 + ((cc - 240) / 35.0) ** 2) ** 2)
    want, _ = cr.region_analysis_gpu(y, _dsm_cfg(), **_PARAMS)
    L = _capi.lib()
    try:
        _capi.check(L.sdsm_set_group_timeout_us(0.001), 'sdsm_set_group_timeout_us')
        got, stats = cr.region_analysis_gpu(y, _dsm_cfg(), **_PARAMS)
    finally:
        _capi.check(L.sdsm_set_group_timeout_us(0.0), 'sdsm_set_group_timeout_us')
    assert sum(r['resolved'] for r in stats['rounds']) > 0
    _assert_same(got, want)


def _oracle_energy(y_crop, mask_crop, atoms_map, footprint, dsm_cfg):
    """The reference's energy computer (c2freganal.py:58-79) with the CPU oracle's cvxprog in place of cvxopt."""
    from oracle import oracle
    near = ndi.distance_transform_edt(y_crop <= 0) <= dsm_cfg['background_margin']
    m = np.isin(atoms_map, list(footprint)) & mask_crop & near
    vals = y_crop[m]
    if (vals > 0).all() or (vals < 0).all():
        return None
    cfg = {k: v for k, v in dsm_cfg.items() if k in ('scale', 'epsilon', 'alpha', 'smooth_subsample', 'gaussian_shape_multiplier', 'init')}
    cfg['smooth_amount'] = np.inf
    _, info = oracle.cvxprog(y_crop, m, cfg)
    return info['energy'] / m.sum()


@pytest.mark.parametrize('index', [0, 5])
def test_restatement_with_oracle_energies_gives_the_same_atoms(gpu, monkeypatch, index):
    """The GPU stage against the restatement fed by the CPU oracle's cvxprog; every threshold decision of the oracle run is further
    from its threshold than the energies' tolerance, so the equality is not luck."""
    from superdsm_amd import c2freganal as cr
    y = _bbbc_y(index)
    got, _ = cr.region_analysis_gpu(y, _dsm_cfg(), **_PARAMS)
    margins = []
    split_cluster = cr._split_cluster

    def recording(cluster_label, cluster, masked_cluster, params, flood):
        """The split loop, its requests answered by the oracle; records how far every decision is from its threshold."""
        steps = split_cluster(cluster_label, cluster, masked_cluster, params, flood)
        by_region = {}
        region = lambda atoms_map, labels: np.packbits(masked_cluster.mask & np.isin(atoms_map, labels)).tobytes()
        try:
            request = next(steps)
            while True:
                atoms_map, fps = request
                res = [_oracle_energy(cluster.model, masked_cluster.mask, atoms_map, fp, _dsm_cfg()) for fp in fps]
                for fp, v in zip(fps, res):
                    by_region[region(atoms_map, fp)] = v
                    if v is not None:                      # leaf or split again (relative: the energy tolerance is relative)
                        margins.append(abs(v - params['max_atom_norm_energy']) / abs(v))
                e0 = by_region.get(region(atoms_map, fps[0] + fps[-1])) if len(fps) == 2 else None
                if e0 is not None and None not in res:     # accept the split or not
                    margins.append(abs(1 - max(res) / e0 - params['min_norm_energy_improvement']))
                request = steps.send(res)
        except StopIteration as stop:
            return stop.value
        yield                                              # (a generator that needs nothing from its driver)

    monkeypatch.setattr(cr, '_split_cluster', recording)
    want = cr.region_analysis_host(y, _dsm_cfg(), energy=None, **_PARAMS)
    monkeypatch.setattr(cr, '_split_cluster', split_cluster)
    _assert_same(got, want)
    assert margins and min(margins) > 1e-4, min(margins)


def test_reference_pipeline_end_to_end(gpu):
    from superdsm_amd import automation, config, pipeline, synth
    spec = synth.WORKLOADS['bbbc039_like']
    shape, layout = synth.bbbc039_like_layout(spec['seed'], 2)
    g = synth.render_image(shape, layout, spec['seed'] + 7919 * 2)
    pl = pipeline.create_reference_pipeline()
    cfg, _ = automation.create_config(pl, config.Config({'AF_scale': 10}))
    data, cfg, timings = pl.process_image(g, cfg)
    atoms, adj, seeds = data['atoms'], data['adjacencies'], data['seeds']
    assert atoms.max() == len(seeds) > 10
    for a in adj.atom_labels:
        assert sum(atoms[tuple(int(v) for v in s)] == a for s in seeds) == 1
        for b in adj[a]:
            assert a in adj[b] and adj.get_cluster_label(a) == adj.get_cluster_label(b)
    assert len(data['objects']) > 0 and len(data['postprocessed_objects']) > 0
    assert set(timings) == {'preprocess', 'dsm', 'c2f-region-analysis', 'global-energy-minimization', 'postprocess'}
