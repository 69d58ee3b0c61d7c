"""Parity of the HIP path (through the C ABI) against the oracle and the golden fixtures.  Needs an MI355X."""
import json
import os

import numpy as np
import pytest

from test_oracle_golden import OPTIMUM_TAGS, TIGHT_DEFORMABLE, reference_optimum_checks

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def unpack(bits, shape):
    shape = tuple(int(s) for s in shape)
    return np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape).astype(bool)


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    from superdsm_amd import _capi
    _capi.lib()     # fails loudly if libsdsm_hip.so is missing
    return torch


def _golden_scene(tag):
    d = np.load(os.path.join(G, f'optimum_{tag}.npz'))
    cfg = json.loads(str(d['cfg']))
    fps = [d[f'c{k}_fp'].tolist() for k in range(int(d['n_cases']))]
    return d, dict(cfg, init='elliptical'), fps


def _tight(d, k):
    return float(d[f'c{k}_gnorm_dsm']) < 1e-8 and float(d[f'c{k}_gnorm_ell']) < 1e-8


def _modes(tag):
    """`group_regime` is solved in throughput mode (0: groups for its regions above 8192 pixels), latency mode (1: groups of other
    sizes, for every region above 3072 pixels) and without groups (2: the same regions through single workgroups) -- a failure that
    shows in modes 0 / 1 only is the group's."""
    return (0, 1, 2) if tag == 'group_regime' else (None,)


def _group_members(batch):
    import ctypes as C
    from superdsm_amd import _capi
    g = np.zeros(batch.n, np.int32)
    _capi.check(_capi.lib().sdsm_plan_schedule(batch.plan, g.ctypes.data_as(C.c_void_p), None), 'sdsm_plan_schedule')
    return g


# ---------------------------------------------------------------------------------------------------------
# per-image preparation: EDT(y <= 0) <= margin, atom extents (objects.py:126-127)
# ---------------------------------------------------------------------------------------------------------
def test_image_prepare_matches_oracle(gpu):
    from oracle import oracle
    from superdsm_amd import engine
    d = np.load(os.path.join(G, 'region.npz'))
    shape = tuple(int(v) for v in d['shape'])
    y, atoms = d['y'], d['atoms']
    y_mask = unpack(d['y_mask'], shape)
    for margin in (3, 8, 2.5):
        img = engine.DeviceImage(y, y_mask, atoms, margin)
        valid = img.valid.cpu().numpy().astype(bool)
        expect = y_mask & (oracle.edt_sq(y <= 0) <= margin * margin)
        np.testing.assert_array_equal(valid, expect)
        stats = img.atom_stats.reshape(-1, 6)
        for l in range(1, int(atoms.max()) + 1):
            m = expect & (atoms == l)
            assert stats[l, 0] == m.sum()
            if m.any():
                rr, cc = np.nonzero(m)
                assert tuple(stats[l, 1:5]) == (rr.min(), rr.max(), cc.min(), cc.max())
    np.testing.assert_array_equal(engine.DeviceImage(y, None, atoms, 8).valid.cpu().numpy().astype(bool), unpack(d['edt_le_8'], shape))


# ---------------------------------------------------------------------------------------------------------
# setup kernel: region crops, greedy grid, float32-exact G~ rows (dsm.py:137-237)
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', OPTIMUM_TAGS)
def test_setup_matches_oracle_exactly(gpu, tag):
    from oracle import oracle
    from superdsm_amd import engine
    d, cfg, fps = _golden_scene(tag)
    y, atoms = d['y'], d['atoms']
    img = engine.DeviceImage(y, None, atoms, cfg['background_margin'])
    batch = engine.Batch(img, fps, cfg)
    batch.launch()
    gpu.cuda.synchronize()
    info = batch.inspect()
    if tag == 'group_regime':
        # the sample is what it claims: tight candidates of 40 000 .. 75 000 pixels solved by groups, one of them a union of two atoms,
        # a smaller group, and tight candidates of the same scene that the plan's own schedule leaves to single workgroups (the control)
        N = np.array([int(d[f'c{k}_N']) for k in range(len(fps))])
        members = _group_members(batch)
        assert (batch.records()['n_pixels'] == N).all() and all(_tight(d, k) and int(d[f'c{k}_M']) > 0 for k in range(len(fps)))
        large = (N >= 40000) & (N <= 75000)
        assert large.sum() >= 2 and (members[large] >= 2).all() and any(len(fps[k]) == 2 for k in np.flatnonzero(large))
        assert ((members > 0) == (N > 8192)).all() and (N > 12288).sum() >= 3
        control = members == 0
        assert control.sum() >= 2 and (N[control] <= 8192).all()
        env = np.array([st['env_size'] for st in batch.inspect_states()])
        print('group_regime: N', N.tolist(), 'group members', members.tolist(), 'Hessian envelope', env.tolist())
        assert (env <= 11000).all()                      # as the fixture's docstring says: all its groups have the LDS layout of class 2
    for k, fp in enumerate(fps):
        mask = oracle.region_mask(y, None, atoms, fp, cfg['background_margin'])
        np.testing.assert_array_equal(mask, unpack(d[f'c{k}_region'], y.shape))
        s = info[k]
        rr, cc = np.nonzero(mask)                       # raster order
        assert s['N'] == mask.sum() == int(d[f'c{k}_N'])
        np.testing.assert_array_equal(s['r'], rr)
        np.testing.assert_array_equal(s['c'], cc)
        np.testing.assert_array_equal(s['y'], y[mask])
        sm = oracle.smooth_matrix(mask, cfg['smooth_amount'], cfg['gaussian_shape_multiplier'], cfg['smooth_subsample'])
        assert s['M'] == sm.M == int(d[f'c{k}_M'])
        assert (s['hc'], s['wc']) == sm.compressed_shape
        np.testing.assert_array_equal(s['grid_r'], sm.grid_r)
        np.testing.assert_array_equal(s['grid_c'], sm.grid_c)
        nnz = np.diff(sm.indptr)
        np.testing.assert_array_equal(s['nnz'], nnz)
        for i in range(s['N']):                         # every row, all entries: indices and float32-exact weights
            lo, hi = sm.indptr[i], sm.indptr[i + 1]
            np.testing.assert_array_equal(s['idx'][:nnz[i], i], sm.indices[lo:hi])
            np.testing.assert_array_equal(s['w'][:nnz[i], i].astype(np.float64), sm.data[lo:hi])


@pytest.mark.parametrize('name', ['blob', 'two_blobs_gaps', 'too_small', 'no_regular_grid_point', 'dense_grid_m_gt_128', 'l_shape', 'gowt1_like', 'odd_params'])
def test_setup_matches_reference_smooth_matrix(gpu, name):
    """G~ of the reference itself (golden CSR) for hand-made masks, including the edge cases: empty rows/cols
    inside the bbox, region too small for the PSF, no regular grid point inside the mask, M > 128 (numpy's
    pairwise float32 summation splits)."""
    from superdsm_amd import engine
    d = np.load(os.path.join(G, f'smoothmat_{name}.npz'))
    mask = unpack(d['mask'], d['mask_shape'])
    sigma, mult, sub = d['params']
    H, W = mask.shape[0] + 6, mask.shape[1] + 9
    atoms = np.zeros((H, W), np.int32)
    atoms[3:3 + mask.shape[0], 4:4 + mask.shape[1]][mask] = 1
    atoms[atoms == 0] = 2
    y = np.where(atoms == 1, 1.0, -1.0)               # every region pixel is foreground -> EDT term is 0 there
    cfg = dict(scale=1000, epsilon=1.0, alpha=0.01, smooth_amount=float(sigma), smooth_subsample=int(sub),
               gaussian_shape_multiplier=float(mult), background_margin=0, init='elliptical', max_iters=1)
    img = engine.DeviceImage(y, None, atoms, 0)
    batch = engine.Batch(img, [[1]], cfg)
    batch.launch()
    gpu.cuda.synchronize()
    s = batch.inspect()[0]
    N, M = (int(v) for v in d['shape'])
    assert (s['N'], s['M']) == (N, M)
    if M == 0:
        return
    grid = np.zeros((s['hc'], s['wc']), bool)
    grid[s['grid_r'], s['grid_c']] = True
    np.testing.assert_array_equal(grid, unpack(d['grid'], d['grid_shape']))
    indptr, indices, data = d['indptr'], d['indices'], d['data']
    np.testing.assert_array_equal(s['nnz'], np.diff(indptr))
    got_idx = np.concatenate([s['idx'][:s['nnz'][i], i] for i in range(N)])
    got_w = np.concatenate([s['w'][:s['nnz'][i], i] for i in range(N)]).astype(np.float64)
    np.testing.assert_array_equal(got_idx, indices)
    np.testing.assert_array_equal(got_w, data)       # float32-exact


# ---------------------------------------------------------------------------------------------------------
# solves: tight optima of the reference's energy, masks, boundary flag
# ---------------------------------------------------------------------------------------------------------
def _paste(off, frag, shape):
    out = np.zeros(shape, bool)
    out[off[0]:off[0] + frag.shape[0], off[1]:off[1] + frag.shape[1]] = frag
    return out


@pytest.mark.parametrize('tag', OPTIMUM_TAGS)
def test_solve_reaches_reference_optima(gpu, tag):
    """Energies, masks and boundary flags at the optima the reference's own Energy reaches; `group_regime` (regions of up to 67 167
    pixels, sigma_G = 8, grid step 16) in the three scheduling modes, whose records must also be the same bytes."""
    from oracle import oracle
    from superdsm_amd import _capi, testing
    d, cfg, fps = _golden_scene(tag)
    scene = dict(y=d['y'], atoms=d['atoms'], dsm_cfg=cfg, footprints=fps)
    orecs, ofrags, oparams = oracle.compute_objects(d['y'], None, d['atoms'], fps, cfg, nthreads=0)
    first = None
    for mode in _modes(tag):
        res = testing.solve_scene_gpu(scene, want_xi=True, mode=mode)
        recs, frags = res['records'], res['fragments']
        if tag == 'group_regime':
            members = _group_members(res['batch'])
            assert (members > 0).any() if mode != 2 else not members.any()
        checked = 0
        for k in range(len(fps)):
            N, M = int(d[f'c{k}_N']), int(d[f'c{k}_M'])
            assert (recs['n_pixels'][k], recs['n_deform'][k]) == (N, M)
            psi_ref = float(d[f'c{k}_psi_dsm'])
            tol = 1e-6 * N / 1000 + 1e-5 * abs(psi_ref)          # fp tolerance on energies
            tight = _tight(d, k)
            # the energy the kernel reports is the reference's energy function at the kernel's own parameters
            mask = oracle.region_mask(d['y'], None, d['atoms'], fps[k], cfg['background_margin'])
            J = oracle.Energy(d['y'], mask, cfg['epsilon'], cfg['alpha'], cfg['smooth_amount'], cfg['gaussian_shape_multiplier'], cfg['smooth_subsample'])
            xo = res['xi_offsets'][k]
            p = np.concatenate([recs['theta'][k], res['xi'][xo:xo + M]])
            assert abs(J(p) - recs['energy'][k]) <= 1e-9 * max(1.0, abs(recs['energy'][k])), (mode, k, J(p), recs['energy'][k])
            if tight:
                assert recs['status'][k] == _capi.CAND_OPTIMAL
                ref = _paste(d[f'c{k}_fg_offset'], unpack(d[f'c{k}_fg_fragment'], d[f'c{k}_fg_shape']), d['y'].shape)
                got = _paste(*frags[k], d['y'].shape)
                dice = 2 * (ref & got).sum() / max(1, ref.sum() + got.sum())
                print(f'{tag} mode {mode} cand {k} N={N} M={M}: |psi - psi_ref| / tol = {abs(recs["energy"][k] - psi_ref) / tol:.3e}, Dice = {dice:.6f}')
                assert abs(recs['energy'][k] - psi_ref) <= tol, (mode, k, recs['energy'][k], psi_ref)
                assert abs(recs['energy'][k] - orecs['energy'][k]) <= tol
                assert dice >= 0.999, (mode, k, dice)
                assert bool(recs['on_boundary'][k]) == bool(d[f'c{k}_on_boundary'])
                checked += 1
            else:
                assert recs['energy'][k] <= psi_ref + tol          # near-separable: no finite minimiser
        assert checked == TIGHT_DEFORMABLE[tag]                    # (every tight pick of the four fixtures has M > 0)
        if first is None:
            first = recs.tobytes(), res['xi'].tobytes()
        assert (recs.tobytes(), res['xi'].tobytes()) == first, f'mode {mode}: other bytes than mode {_modes(tag)[0]}'


def test_solve_matches_oracle_on_synthetic256(gpu):
    """BASELINE.json configs[0]: 256x256 synthetic image, every candidate, GPU vs CPU oracle."""
    from oracle import oracle
    from superdsm_amd import testing
    scene = testing.make_scene('synthetic256', max_size=3)
    res = testing.solve_scene_gpu(scene)
    recs, frags = res['records'], res['fragments']
    orecs, ofrags, _ = oracle.compute_objects(scene['y'], None, scene['atoms'], scene['footprints'], scene['dsm_cfg'], nthreads=0)
    n = len(scene['footprints'])
    np.testing.assert_array_equal(recs['n_pixels'], orecs['N'])
    np.testing.assert_array_equal(recs['n_deform'], orecs['M'])
    worst_dice = 1.0
    for k in range(n):
        assert recs['status'][k] == orecs['status'][k], (k, recs['status'][k], orecs['status'][k])
        tol = 1e-6 * orecs['N'][k] / 1000 + 1e-5 * abs(orecs['energy'][k])
        assert abs(recs['energy'][k] - orecs['energy'][k]) <= tol, (k, recs['energy'][k], orecs['energy'][k])
        assert bool(recs['on_boundary'][k]) == bool(orecs['on_boundary'][k])
        dice = testing.dice(frags[k][0], frags[k][1], orecs['fg_offset'][k], ofrags[k], scene['y'].shape)
        worst_dice = min(worst_dice, dice)
    assert worst_dice >= 0.999, worst_dice


def test_solve_matches_oracle_on_synthetic512(gpu):
    """BASELINE.json north_star's reporting config -- a synthetic 512x512 nuclei image --: every candidate, GPU vs CPU oracle (energies,
    status, boundary flag, masks), alone and as one of two images of a plan (the same bytes)."""
    from oracle import oracle
    from superdsm_amd import engine, testing
    scene = testing.make_scene('synthetic512', max_size=3)
    res = testing.solve_scene_gpu(scene)
    recs, frags = res['records'], res['fragments']
    orecs, ofrags, _ = oracle.compute_objects(scene['y'], None, scene['atoms'], scene['footprints'], scene['dsm_cfg'], nthreads=0)
    n = len(scene['footprints'])
    assert n > 200 and recs['n_deform'].max() + 6 > 128, 'the scene is meant to reach beyond solve class 1'
    np.testing.assert_array_equal(recs['n_pixels'], orecs['N'])
    np.testing.assert_array_equal(recs['n_deform'], orecs['M'])
    for k in range(n):
        assert recs['status'][k] == orecs['status'][k], (k, recs['status'][k], orecs['status'][k])
        tol = 1e-6 * orecs['N'][k] / 1000 + 1e-5 * abs(orecs['energy'][k])
        assert abs(recs['energy'][k] - orecs['energy'][k]) <= tol, (k, recs['energy'][k], orecs['energy'][k])
        assert bool(recs['on_boundary'][k]) == bool(orecs['on_boundary'][k])
        assert testing.dice(frags[k][0], frags[k][1], orecs['fg_offset'][k], ofrags[k], scene['y'].shape) >= 0.999, k
    img = res['image']
    two = engine.Batch([img, img], scene['footprints'] * 2, scene['dsm_cfg'], image_of=np.repeat(np.arange(2, dtype=np.int32), n))
    two.launch()
    gpu.cuda.synchronize()
    r2 = two.records()
    assert r2[:n].tobytes() == recs.tobytes() and r2[n:].tobytes() == recs.tobytes()


def test_full_size_properties_bbbc039_like(gpu):
    """BASELINE.json configs[1] at full size: properties that do not need the CPU oracle on every candidate."""
    from oracle import oracle
    from superdsm_amd import _capi, testing
    scene = testing.make_scene('bbbc039_like', max_size=3)
    fps = scene['footprints']
    res = testing.solve_scene_gpu(scene)
    recs = res['records']
    ok = recs['status'] == _capi.CAND_OPTIMAL
    assert ok.all(), np.unique(recs['status'], return_counts=True)
    assert np.isfinite(recs['energy'][ok]).all() and (recs['energy'][ok] >= 0).all()
    # the DSM can only improve on the elliptical model it starts from (monotone line search)
    assert (recs['energy'][ok] <= recs['energy_ell'][ok] * (1 + 1e-9) + 1e-9).all()
    # idempotence: a second launch of the same plan gives the same records
    res['batch'].launch()
    gpu.cuda.synchronize()
    recs2 = res['batch'].records()
    # ... bit for bit: every sum over the pixels is an integer (fixed-point) sum or a sum in a fixed order
    assert recs2.tobytes() == recs.tobytes()
    # permutation invariance: candidates are independent, and a candidate's numbers do not depend on its place in the plan
    perm = np.random.default_rng(0).permutation(len(fps))
    res3 = testing.solve_scene_gpu(scene, footprints=[fps[i] for i in perm])
    assert res3['records'].tobytes() == recs[perm].tobytes()
    # fragments stay inside the region bounding box and contain only region pixels
    img, batch = res['image'], res['batch']
    for k in range(0, len(fps), 17):
        off, frag = res['fragments'][k]
        r0, c0, h, w = batch.mask_info[k]
        if recs['fg_h'][k] > 0:
            assert r0 <= off[0] and off[0] + frag.shape[0] <= r0 + h and c0 <= off[1] and off[1] + frag.shape[1] <= c0 + w
            assert frag[0].any() and frag[-1].any() and frag[:, 0].any() and frag[:, -1].any()     # minimal bounding box
    # spot check against the oracle on a subset (keeps the CPU time bounded)
    sub = list(range(0, len(fps), 25))
    orecs, ofrags, _ = oracle.compute_objects(scene['y'], None, scene['atoms'], [fps[i] for i in sub], scene['dsm_cfg'], nthreads=0)
    for j, k in enumerate(sub):
        tol = 1e-6 * orecs['N'][j] / 1000 + 1e-5 * abs(orecs['energy'][j])
        assert abs(recs['energy'][k] - orecs['energy'][j]) <= tol, (k, recs['energy'][k], orecs['energy'][j])
        assert testing.dice(res['fragments'][k][0], res['fragments'][k][1], orecs['fg_offset'][j], ofrags[j], scene['y'].shape) >= 0.999


@pytest.mark.parametrize('layout,from_gpu_preprocessing', [(2, True), (5, False), (7, False)])
def test_stage_with_exact_pruning_on_further_layouts_matches_cpu_oracle(gpu, monkeypatch, layout, from_gpu_preprocessing):
    """The whole stage with pruning='exact' (bounds from max-weight set packing and the cluster costs, globalenergymin.py:340-350) on
    three more of the reference's BBBC039 object tables: the GPU-driven run against the same host logic driven by the CPU oracle --
    same batches, same cover, same counters, same segmentation.  Once (`from_gpu_preprocessing`) the offset intensities come from the
    GPU's Preprocessing kernels (g_raw -> y -> atoms) instead of the SciPy formula of the scene builder."""
    from oracle import oracle
    from superdsm_amd import config, engine, globalenergymin, objects, synth, testing
    from superdsm_amd.atoms import AtomAdjacencyGraph
    scene = testing.make_scene('bbbc039_like', max_size=2, layout_index=layout)
    if from_gpu_preprocessing:
        y = engine.preprocess(scene['g'], sigma2=scene['scale'])                      # preprocess.py:39-68 on the GPU
        assert np.abs(y - scene['y']).max() <= 1e-12
        spec = dict(synth.WORKLOADS['bbbc039_like'])
        _, lay = synth.bbbc039_like_layout(spec['seed'], layout)
        atoms, clusters, seeds = synth.make_atoms(y, lay, spec['seed'] + 7919 * layout)
        scene = dict(scene, y=y, atoms=atoms, clusters=clusters, seeds=seeds, adjacencies=AtomAdjacencyGraph(atoms, clusters, y > 0, seeds))
    stage = globalenergymin.GlobalEnergyMinimization()
    mk = lambda: dict(y=scene['y'], y_mask=np.ones(scene['y'].shape, bool), atoms=scene['atoms'], adjacencies=scene['adjacencies'], dsm_cfg=scene['dsm_cfg'])
    cfg = config.Config({'global-energy-minimization': {'beta': 150.0, 'pruning': 'exact', 'speculation': 0}})
    batches = {'gpu': [], 'cpu': []}
    real = objects.compute_objects

    def spy(objs, *a, **k):
        objs = list(objs)
        batches['gpu'].append(sorted(sorted(o.footprint) for o in objs))
        return real(objs, *a, **k)

    def oracle_compute(objs, y, atoms, dsm_cfg, log_root_dir, status_line=None, out=None, shard=None):
        objs = list(objs)
        batches['cpu'].append(sorted(sorted(o.footprint) for o in objs))
        if not objs:
            return
        recs, frags, _ = oracle.compute_objects(y.model, None, atoms, [sorted(o.footprint) for o in objs], dsm_cfg, nthreads=0)
        for o, r, f in zip(objs, recs, frags):
            o.energy, o.is_optimal, o.on_boundary, o.processing_time = float(r['energy']), bool(r['is_optimal']), bool(r['on_boundary']), 0
            o.fg_offset, o.fg_fragment = np.array(r['fg_offset']), f

    monkeypatch.setattr(globalenergymin, 'compute_objects', spy)
    d_gpu = mk()
    stage(d_gpu, cfg, out='muted')
    monkeypatch.setattr(globalenergymin, 'compute_objects', oracle_compute)
    d_cpu = mk()
    stage(d_cpu, cfg, out='muted')
    assert batches['gpu'] == batches['cpu']
    cov = lambda d: sorted(sorted(int(a) for a in o.footprint) for o in d['cover'].solution)
    assert cov(d_gpu) == cov(d_cpu)
    assert abs(d_gpu['cover'].costs - d_cpu['cover'].costs) <= 1e-5 * abs(d_cpu['cover'].costs)
    for k in d_gpu['performance'].attributes:
        assert getattr(d_gpu['performance'], k) == getattr(d_cpu['performance'], k)
    seg = [np.zeros(scene['y'].shape, bool) for _ in range(2)]
    for o in d_gpu['cover'].solution:
        o.fill_foreground(seg[0])
    for o in d_cpu['cover'].solution:
        o.fill_foreground(seg[1])
    assert 2 * (seg[0] & seg[1]).sum() / max(1, seg[0].sum() + seg[1].sum()) >= 0.999


# ---------------------------------------------------------------------------------------------------------
# preprocessing (preprocess.py:39-68)
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ['a', 'b', 'c', 'd'])
def test_preprocess_matches_reference(gpu, key):
    from superdsm_amd import engine
    d = np.load(os.path.join(G, f'preprocess_{key}.npz'))
    cfg = json.loads(str(d['cfg']))
    y = engine.preprocess(d['g_raw'], cfg.get('sigma1', np.sqrt(2)), cfg.get('sigma2', 40), cfg.get('offset_clip', 3), cfg.get('lower_clip_mean', False))
    np.testing.assert_allclose(y, d['y'], rtol=0, atol=1e-13)     # tolerance: fp64 re-association in mean / std only


# ---------------------------------------------------------------------------------------------------------
# the stage behind the reference's plugin API (globalenergymin.py:97-180)
# ---------------------------------------------------------------------------------------------------------
def test_stage_end_to_end_matches_cpu_oracle(gpu, monkeypatch):
    """GlobalEnergyMinimization.process on the GPU vs the same generation logic driven by the CPU oracle: same
    batches of candidates, same min-weight set cover, same masks."""
    from oracle import oracle
    from superdsm_amd import config, globalenergymin, objects, testing
    scene = testing.make_scene('synthetic256', max_size=2)
    beta = 150.0
    stage = globalenergymin.GlobalEnergyMinimization()
    data = dict(y=scene['y'], y_mask=np.ones(scene['y'].shape, bool), atoms=scene['atoms'], adjacencies=scene['adjacencies'], dsm_cfg=scene['dsm_cfg'])
    cfg = config.Config({'global-energy-minimization': {'beta': beta, 'pruning': 'exact'}})
    gpu_batches = []
    real = objects.compute_objects

    def spy(objs, *a, **k):
        objs = list(objs)
        gpu_batches.append(sorted(sorted(o.footprint) for o in objs))
        return real(objs, *a, **k)

    monkeypatch.setattr(globalenergymin, 'compute_objects', spy)
    stage(data, cfg, out='muted')
    cover_gpu = sorted(sorted(int(a) for a in o.footprint) for o in data['cover'].solution)
    costs_gpu = data['cover'].costs

    cpu_batches = []

    def oracle_compute(objs, y, atoms, dsm_cfg, log_root_dir, status_line=None, out=None, shard=None):
        objs = list(objs)
        cpu_batches.append(sorted(sorted(o.footprint) for o in objs))
        if not objs:
            return
        recs, frags, _ = oracle.compute_objects(y.model, None, atoms, [sorted(o.footprint) for o in objs], dsm_cfg, nthreads=0)
        for o, r, f in zip(objs, recs, frags):
            o.energy, o.is_optimal, o.on_boundary, o.processing_time = float(r['energy']), bool(r['is_optimal']), bool(r['on_boundary']), 0
            o.fg_offset, o.fg_fragment = np.array(r['fg_offset']), f

    monkeypatch.setattr(globalenergymin, 'compute_objects', oracle_compute)
    data2 = dict(data)
    stage(data2, cfg, out='muted')
    assert gpu_batches == cpu_batches
    assert cover_gpu == sorted(sorted(int(a) for a in o.footprint) for o in data2['cover'].solution)
    assert abs(costs_gpu - data2['cover'].costs) <= 1e-5 * abs(costs_gpu)
    for k in data['performance'].attributes:
        assert getattr(data['performance'], k) == getattr(data2['performance'], k)
    seg_gpu = np.zeros(scene['y'].shape, bool)
    seg_cpu = np.zeros(scene['y'].shape, bool)
    for o in data['cover'].solution:
        o.fill_foreground(seg_gpu)
    for o in data2['cover'].solution:
        o.fill_foreground(seg_cpu)
    dice = 2 * (seg_gpu & seg_cpu).sum() / max(1, seg_gpu.sum() + seg_cpu.sum())
    assert dice >= 0.999, dice


def test_preprocess_stage_in_pipeline(gpu):
    from superdsm_amd import config, pipeline
    from superdsm_amd.preprocess import Preprocessing
    d = np.load(os.path.join(G, 'preprocess_a.npz'))
    pl = pipeline.create_pipeline([Preprocessing()])
    data, _, _ = pl.process_image(d['g_raw'], config.Config({'preprocess': json.loads(str(d['cfg']))}), out='muted')
    np.testing.assert_allclose(data['y'], d['y'], rtol=0, atol=1e-13)


# ---------------------------------------------------------------------------------------------------------
# BASELINE.json configs[2] / configs[3] stand-ins: large sigma_G (65x65 PSF), large regions, M up to ~300
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('workload', ['gowt1_like', 'nih3t3_like'])
def test_large_scale_workloads_match_oracle(gpu, workload):
    from oracle import oracle
    from superdsm_amd import _capi, testing
    scene = testing.make_scene(workload, max_size=3)
    fps = scene['footprints']
    res = testing.solve_scene_gpu(scene)
    recs = res['records']
    assert (recs['status'] == _capi.CAND_OPTIMAL).all(), np.unique(recs['status'], return_counts=True)
    # every size class incl. the global-memory one (6 + M > 172) must be exercised by these scenes
    n = recs['n_deform'] + 6
    assert (n > 172).any() and ((n > 84) & (n <= 172)).any() and (n <= 40).any()
    sample = list(range(len(fps)))                          # every candidate (90 / 234: seconds for the oracle on the box's cores)
    orecs, ofrags, _ = oracle.compute_objects(scene['y'], None, scene['atoms'], [fps[i] for i in sample], scene['dsm_cfg'], nthreads=0)
    for j, k in enumerate(sample):
        assert (recs['n_pixels'][k], recs['n_deform'][k]) == (orecs['N'][j], orecs['M'][j])
        tol = 1e-6 * orecs['N'][j] / 1000 + 1e-5 * abs(orecs['energy'][j])
        assert abs(recs['energy'][k] - orecs['energy'][j]) <= tol, (k, recs['energy'][k], orecs['energy'][j])
        assert testing.dice(res['fragments'][k][0], res['fragments'][k][1], orecs['fg_offset'][j], ofrags[j], scene['y'].shape) >= 0.999
        assert bool(recs['on_boundary'][k]) == bool(orecs['on_boundary'][j])


# ---------------------------------------------------------------------------------------------------------
# edge cases of the reference's per-candidate driver (objects.py:177-212) and of the operator's other callers
# ---------------------------------------------------------------------------------------------------------
def test_edge_cases_trivial_masked_border_and_elliptical_only(gpu):
    from oracle import oracle
    from superdsm_amd import _capi, engine, image, objects
    from superdsm_amd import testing
    sc = testing.edge_case_scene()        # a nucleus with a hole of the mask inside, one cut by the border, a single positive pixel, a union of two atoms
    y, y_mask, atoms, cfg, fps = sc['y'], sc['y_mask'], sc['atoms'], sc['cfg'], sc['footprints']
    H, W = y.shape
    img = engine.DeviceImage(y, y_mask, atoms, cfg['background_margin'])
    batch = engine.Batch(img, fps, cfg)
    batch.launch()
    gpu.cuda.synchronize()
    recs = batch.records()
    frags = batch.fragments(recs)
    orecs, ofrags, _ = oracle.compute_objects(y, y_mask, atoms, fps, cfg, nthreads=0)
    # [2]: exactly one positive pixel -> trivial (objects.py:184-191): energy 0, is_optimal False, fragment [[False]]
    assert recs['status'][1] == _capi.CAND_TRIVIAL and orecs['status'][1] == 2 and recs['energy'][1] == 0
    np.testing.assert_array_equal(frags[1][1], [[False]])
    for k in (0, 2, 3):
        assert recs['status'][k] == orecs['status'][k] == 0
        assert (recs['n_pixels'][k], recs['n_deform'][k]) == (orecs['N'][k], orecs['M'][k])
        tol = 1e-6 * orecs['N'][k] / 1000 + 1e-5 * abs(orecs['energy'][k])
        assert abs(recs['energy'][k] - orecs['energy'][k]) <= tol
        assert bool(recs['on_boundary'][k]) == bool(orecs['on_boundary'][k])
        full = np.zeros((H, W), bool)
        full[frags[k][0][0]:frags[k][0][0] + frags[k][1].shape[0], frags[k][0][1]:frags[k][0][1] + frags[k][1].shape[1]] = frags[k][1]
        assert not (full & ~y_mask).any()                                    # masked-out pixels never enter a fragment
    assert bool(recs['on_boundary'][2])                                       # the nucleus at the border reaches the pad ring
    # the same through the reference-style API, incl. an empty batch and the in-place contract
    yi = image.Image.create_from_array(y, normalize=False, mask=y_mask)
    objs = []
    for fp in fps:
        o = objects.Object()
        o.footprint = set(fp)
        objs.append(o)
    objects.compute_objects([], yi, atoms, cfg, None, out='muted')
    objects.compute_objects(objs, yi, atoms, dict(cfg, cachesize=1, cp_timeout=300, smooth_mat_max_allocations=np.inf), None, out='muted')
    assert objs[1].energy == 0 and objs[1].is_optimal is False and objs[0].is_optimal is True
    assert objs[0].copy().cvxprog_region_size == orecs['N'][0] and abs(objects.compute_norm_energy(objs[0]) - orecs['energy'][0] / orecs['N'][0]) <= 1e-8   # postprocess.py:289-291
    assert abs(objs[0].energy - orecs['energy'][0]) <= 1e-5 * abs(orecs['energy'][0]) + 1e-6
    # elliptical models only (smooth_amount = inf): what the reference's C2F stage asks of the operator (c2freganal.py:126)
    cfg_inf = dict(cfg, smooth_amount=np.inf)
    b2 = engine.Batch(img, [[1], [3]], cfg_inf)
    b2.launch()
    gpu.cuda.synchronize()
    r2 = b2.records()
    o2, _, _ = oracle.compute_objects(y, y_mask, atoms, [[1], [3]], cfg_inf, nthreads=0)
    assert (r2['n_deform'] == 0).all() and (o2['M'] == 0).all()
    np.testing.assert_allclose(r2['energy'], o2['energy'], rtol=1e-5, atol=1e-6)     # separable toy regions: psi ~ 1e-8
    assert (r2['energy'] <= r2['energy_ell'] + 1e-9).all()


def test_sharder_single_rank_equals_direct_batch(gpu):
    """The multi-GPU code path (dist.Sharder: shard, solve on this rank's GPU, all-gather, unpack) with one rank."""
    import torch.distributed as dist
    from superdsm_amd import dist as sdist
    from superdsm_amd import engine, testing
    scene = testing.make_scene('synthetic256', max_size=2)
    fps = scene['footprints']
    created = False
    if not dist.is_initialized():
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:29533', rank=0, world_size=1)
        created = True
    try:
        img = engine.DeviceImage(scene['y'], None, scene['atoms'], scene['dsm_cfg']['background_margin'])
        cfg = {k: v for k, v in scene['dsm_cfg'].items() if k != 'background_margin'}
        recs, frags = sdist.Sharder(device='cpu').solve(img, fps, cfg)
        ref = testing.solve_scene_gpu(scene)
        # a candidate's record does not depend on its plan (every sum over the pixels is an integer sum or a sum in a fixed order): the same bytes
        assert recs.tobytes() == ref['records'].tobytes()
        for a, b in zip(frags, ref['fragments']):
            assert tuple(a[0]) == tuple(b[0]) and np.array_equal(a[1], b[1])
    finally:
        if created:
            dist.destroy_process_group()


def _rccl_one_rank(q, port):
    """Child process: the collectives of the N-GPU paths on the REAL backend (RCCL, device tensors) with a world of one rank."""
    import os
    import traceback
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
        import torch
        import torch.distributed as dist
        from superdsm_amd import dist as sdist
        from superdsm_amd import engine, testing
        torch.cuda.set_device(0)
        dist.init_process_group('nccl', rank=0, world_size=1)
        scene = testing.make_scene('synthetic256', max_size=2)
        fps = scene['footprints']
        img = engine.DeviceImage(scene['y'], None, scene['atoms'], scene['dsm_cfg']['background_margin'])
        cfg = {k: v for k, v in scene['dsm_cfg'].items() if k != 'background_margin'}
        # (1) bench.py --gpus N: barrier, gather of device records + masks to rank 0, max-reduction of the time on the device
        batch = engine.Batch(img, fps, scene['dsm_cfg'])
        batch.launch()
        g = sdist.RecordGather(batch, 1, 0, sizes=[[batch.records_dev.numel(), batch.masks_dev.numel()]])
        dist.barrier()
        g.run()
        torch.cuda.synchronize()
        rec_bytes, mask_bytes = g.unpack()[0]
        direct = batch.records()
        ok1 = bool((rec_bytes[:direct.nbytes] == direct.view('u1').reshape(-1)).all()) and bool((mask_bytes == batch.masks_dev.cpu().numpy()).all())
        t = torch.tensor([1.5], dtype=torch.float64, device='cuda')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        # (2) Sharder: device-to-device all-gather of the packed block
        recs, frags = sdist.Sharder().solve(img, fps, cfg)
        # (3) image sets: the one gather of per-image results
        got = sdist.gather_objects([(0, [[1, 2]], 3.5, 7)], dst=0)
        dist.destroy_process_group()
        q.put(('ok', ok1, float(t.item()), recs['energy'].tolist(), direct['energy'].tolist(), got))
    except BaseException:                       # noqa: BLE001 -- reported to the parent
        q.put(('error', traceback.format_exc()))


def test_collectives_of_the_multi_gpu_paths_run_on_rccl_with_one_rank(gpu):
    """`bench.py --gpus N`, `dist.Sharder` and the image-set gather use the backend "nccl" (= RCCL) with device tensors on a real
    node; the gloo tests cannot see a mistake in THOSE calls (dtypes, device placement, gather of uint8 blocks).  A world of one
    rank on the one GPU of the box runs exactly those calls through RCCL, in a child process of its own."""
    import multiprocessing as mp
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_one_rank, args=(q, port))
    p.start()
    res = q.get(timeout=300)
    p.join(60)
    assert res[0] == 'ok', res[1]
    _, ok1, tmax, e_shard, e_direct, got = res
    assert ok1 and tmax == 1.5
    assert e_shard == e_direct                           # (the same bits: a candidate's numbers do not depend on its plan)
    assert got == [[(0, [[1, 2]], 3.5, 7)]]


def test_latency_mode_gives_the_same_results(gpu):
    """sdsm_plan_set_latency_mode only changes which workgroup size solves the large regions."""
    from superdsm_amd import engine, testing
    scene = testing.make_scene('bbbc039_like', max_size=2)
    fps = scene['footprints'][-40:]                     # the cluster universes: the largest regions of the image
    img = engine.DeviceImage(scene['y'], None, scene['atoms'], scene['dsm_cfg']['background_margin'])
    cfg = {k: v for k, v in scene['dsm_cfg'].items() if k != 'background_margin'}
    out = []
    for mode in (False, True):
        b = engine.Batch(img, fps, cfg, latency_mode=mode)
        b.launch()
        gpu.cuda.synchronize()
        out.append((b.records(), b.fragments(b.records())))
    (r0, f0), (r1, f1) = out
    assert (r0['n_pixels'] > 3072).any(), 'the sample must contain regions that change class'
    assert (r0['status'] == r1['status']).all() and (r0['n_deform'] == r1['n_deform']).all()
    assert r1.tobytes() == r0.tobytes()                  # ... nothing else: the same records, the same masks
    for a, b in zip(f0, f1):
        assert tuple(a[0]) == tuple(b[0]) and np.array_equal(a[1], b[1])


def test_wide_envelope_and_long_rows_use_the_global_memory_class(gpu):
    """A dense grid (smooth_subsample 3): G~ rows of ~100 entries (the generic row path, not the 28-entry register
    path) and a Hessian envelope far beyond the LDS classes (class 3: envelope in global memory)."""
    from oracle import oracle
    from superdsm_amd import engine
    from superdsm_amd import testing
    sc = testing.dense_grid_scene()
    y, atoms, cfg = sc['y'], sc['atoms'], sc['cfg']
    H, W = y.shape
    img = engine.DeviceImage(y, None, atoms, cfg['background_margin'])
    batch = engine.Batch(img, [[1]], cfg)
    batch.launch()
    gpu.cuda.synchronize()
    rec = batch.records()[0]
    ins = batch.inspect()[0]
    orecs, ofrags, _ = oracle.compute_objects(y, None, atoms, [[1]], cfg, nthreads=0)
    n = 6 + int(rec['n_deform'])
    assert ins['zmax'] > 28, 'rows must exceed the register path'
    assert 152 < n <= 1024 and int(ins['env_size']) > 11000, 'the envelope must exceed the LDS classes'
    assert rec['status'] == orecs['status'][0] == 0 and rec['n_deform'] == orecs['M'][0]
    tol = 1e-6 * orecs['N'][0] / 1000 + 1e-5 * abs(orecs['energy'][0])
    assert abs(rec['energy'] - orecs['energy'][0]) <= tol
    frag = batch.fragments(batch.records())[0]
    from superdsm_amd import testing
    assert testing.dice(frag[0], frag[1], orecs['fg_offset'][0], ofrags[0], (H, W)) >= 0.999


def test_c2f_normalized_energies_match_oracle(gpu, monkeypatch):
    """the operator the C2F stage calls (c2freganal.py:58-79) -- elliptical models only, region on the
    cluster crop, None for one-signed regions, no single-positive-pixel shortcut, cache per region."""
    import scipy.ndimage as ndi
    from oracle import oracle
    from superdsm_amd import c2f_energy, engine, image, objects
    rng = np.random.default_rng(21)
    H, W = 70, 96
    rr, cc = np.mgrid[:H, :W]
    y = -0.12 + 0.02 * rng.standard_normal((H, W))
    y = np.minimum(y, -0.005)
    y[((rr - 34) / 20.0) ** 2 + ((cc - 30) / 17.0) ** 2 <= 1] = 0.3          # two touching nuclei: one cluster
    y[((rr - 36) / 16.0) ** 2 + ((cc - 62) / 19.0) ** 2 <= 1] = 0.25
    atoms_map = np.ones((H, W), np.int64)
    atoms_map[:, 46:] = 2                                                    # the split
    atoms_map[30:40, 25:33] = 3                                              # a part inside a nucleus: all positive -> None
    atoms_map[:6, :6] = 4                                                    # background corner ...
    y[2, 2] = 0.2                                                            # ... with a single positive pixel
    y_mask = np.ones((H, W), bool)
    y_mask[:, 90:] = False
    cfg = dict(scale=1000, epsilon=1.0, alpha=0.033, smooth_amount=4, smooth_subsample=8, gaussian_shape_multiplier=2,
               background_margin=7, init='elliptical', cachesize=1, cp_timeout=300, smooth_mat_max_allocations=np.inf)
    yi = image.Image.create_from_array(y, normalize=False)
    cluster = yi.get_region(np.ones((H, W), bool), shrink=True)
    masked = cluster.get_region(cluster.shrink_mask(y_mask))
    fps = [{1}, {2}, {1, 2}, {3}, {4}, {1, 3}]
    objs = []
    for fp in fps:
        o = objects.Object()
        o.footprint = frozenset(fp)
        objs.append(o)
    comp = c2f_energy.get_cached_normalized_energy_computer(yi, cluster)
    got = comp.compute_many(objs, masked, atoms_map, cfg)
    # host restatement with the oracle's cvxprog on the same regions
    near = ndi.distance_transform_edt(y <= 0) <= cfg['background_margin']
    cfg_inf = {k: v for k, v in cfg.items() if k in ('scale', 'epsilon', 'alpha', 'smooth_subsample', 'gaussian_shape_multiplier', 'init')}
    cfg_inf['smooth_amount'] = np.inf
    for fp, g in zip(fps, got):
        m = np.isin(atoms_map, list(fp)) & y_mask & near
        vals = y[m]
        if (vals > 0).all() or (vals < 0).all():
            assert g is None, fp
            continue
        _, info = oracle.cvxprog(y, m, cfg_inf)
        want = info['energy'] / m.sum()
        assert g is not None and abs(g - want) <= 1e-5 * abs(want) + 1e-9, (fp, g, want)
    assert got[3] is None and got[4] is not None          # the all-positive part; the single positive pixel is solved, not skipped
    # cache: asking again launches nothing
    calls = []
    real = engine.Batch
    monkeypatch.setattr(engine, 'Batch', lambda *a, **k: calls.append(1) or real(*a, **k))
    again = [comp(o, masked, atoms_map, cfg) for o in objs]
    assert calls == [] and again == got


@pytest.mark.parametrize('seed,sigma,subsample', [(1, 4, 8), (2, 2, 4), (3, 6, 12), (4, 4, 5), (5, 3, 6)])
def test_random_shapes_and_hyperparameters_match_oracle(gpu, seed, sigma, subsample):
    """Irregular regions (concave, with holes, thin bridges, cut by the image border and by y_mask) under several
    (smooth_amount, smooth_subsample) pairs: grids that are not lattices, non-monotone Hessian envelopes, rows of G~ of
    very different lengths.  Energies against the oracle, masks by Dice."""
    from oracle import oracle
    from superdsm_amd import engine, testing
    rng = np.random.default_rng(100 + seed)
    H, W = 90, 110
    rr, cc = np.mgrid[:H, :W]
    y = -0.15 + 0.03 * rng.standard_normal((H, W))
    for _ in range(7):                                                        # overlapping blobs of random shape
        r0, c0 = rng.uniform(5, H - 5), rng.uniform(5, W - 5)
        a, b, th = rng.uniform(6, 22), rng.uniform(6, 22), rng.uniform(0, np.pi)
        u = (rr - r0) * np.cos(th) + (cc - c0) * np.sin(th)
        v = -(rr - r0) * np.sin(th) + (cc - c0) * np.cos(th)
        y += rng.uniform(0.25, 0.5) * np.exp(-1.3 * ((u / a) ** 2 + (v / b) ** 2) ** 1.5)
    y_mask = np.ones((H, W), bool)
    for _ in range(3):                                                        # holes in the admissible area
        r0, c0 = rng.integers(10, H - 10), rng.integers(10, W - 10)
        y_mask[r0:r0 + rng.integers(2, 7), c0:c0 + rng.integers(2, 9)] = False
    # atoms: a random Voronoi partition (irregular, concave unions)
    seeds = np.stack([rng.uniform(0, H, 9), rng.uniform(0, W, 9)], 1)
    atoms = 1 + np.argmin((rr[..., None] - seeds[:, 0]) ** 2 + (cc[..., None] - seeds[:, 1]) ** 2, axis=2).astype(np.int32)
    fps = [[a] for a in range(1, 10)] + [[1, 2], [3, 4, 5], [2, 6, 7, 8], [1, 3, 5, 7, 9], list(range(1, 10))]
    cfg = dict(scale=1000, epsilon=1.0, alpha=0.04, smooth_amount=sigma, smooth_subsample=subsample, gaussian_shape_multiplier=2,
               background_margin=6, init='elliptical')
    img = engine.DeviceImage(y, y_mask, atoms, cfg['background_margin'])
    batch = engine.Batch(img, fps, cfg)
    batch.launch()
    gpu.cuda.synchronize()
    recs = batch.records()
    frags = batch.fragments(recs)
    orecs, ofrags, _ = oracle.compute_objects(y, y_mask, atoms, fps, cfg, nthreads=0)
    checked = 0
    for k in range(len(fps)):
        if orecs['status'][k] == 2:                                           # trivial (single positive pixel)
            assert recs['status'][k] == 2
            continue
        assert (recs['n_pixels'][k], recs['n_deform'][k]) == (orecs['N'][k], orecs['M'][k]), k
        if orecs['status'][k] != 0 or recs['status'][k] != 0:
            assert recs['energy'][k] <= orecs['energy'][k] * (1 + 1e-6) + 1e-9, k   # a fallback on either side: not worse than the oracle's value
            continue
        tol = 1e-6 * orecs['N'][k] / 1000 + 1e-5 * abs(orecs['energy'][k])
        assert abs(recs['energy'][k] - orecs['energy'][k]) <= tol, (k, recs['energy'][k], orecs['energy'][k])
        assert testing.dice(frags[k][0], frags[k][1], orecs['fg_offset'][k], ofrags[k], (H, W)) >= 0.999, k
        checked += 1
    assert checked >= 8


def test_workgroup_group_elliptical_only_and_trivial_cases(gpu):
    """A region of > 12288 pixels is solved by a group of workgroups; here with smooth_amount = inf (6 parameters, every
    pass still sliced and all-reduced) and next to ordinary candidates in the same batch."""
    from oracle import oracle
    from superdsm_amd import engine
    rng = np.random.default_rng(31)
    H, W = 190, 210
    rr, cc = np.mgrid[:H, :W]
    y = -0.1 + 0.02 * rng.standard_normal((H, W))
    y += 0.45 * np.exp(-(((rr - 95) / 60.0) ** 2 + ((cc - 100) / 75.0) ** 2) ** 2)
    atoms = np.ones((H, W), np.int32)
    atoms[:, 150:] = 2
    for sm in (np.inf, 6.0):
        cfg = dict(scale=1000, epsilon=1.0, alpha=0.05, smooth_amount=sm, smooth_subsample=12, gaussian_shape_multiplier=2,
                   background_margin=10, init='elliptical')
        fps = [[1], [2], [1, 2]]
        img = engine.DeviceImage(y, None, atoms, cfg['background_margin'])
        for mode in (False, True):
            batch = engine.Batch(img, fps, cfg, latency_mode=mode)
            batch.launch()
            gpu.cuda.synchronize()
            recs = batch.records()
            orecs, _, _ = oracle.compute_objects(y, None, atoms, fps, cfg, nthreads=0)
            assert recs['n_pixels'].max() > 12288
            for k in range(3):
                assert recs['status'][k] == orecs['status'][k] == 0 and recs['n_deform'][k] == orecs['M'][k]
                tol = 1e-6 * orecs['N'][k] / 1000 + 1e-5 * abs(orecs['energy'][k])
                assert abs(recs['energy'][k] - orecs['energy'][k]) <= tol, (sm, mode, k, recs['energy'][k], orecs['energy'][k])


# ---------------------------------------------------------------------------------------------------------
# round 2: the fixtures of the reference's elliptical optimum / parameters, point evaluations, BASELINE configs[4],
# forced protocol branches
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', OPTIMUM_TAGS)
def test_elliptical_optimum_and_parameters_match_reference(gpu, tag):
    """`c{k}_psi_ell` (the reference's Energy of the 6-parameter model driven to its optimum: ALL of what the C2F operator
    returns), the moment initialisation's energy, and the DSM optimum's parameters theta / xi (`c{k}_x_dsm`)."""
    from superdsm_amd import testing
    d, cfg, fps = _golden_scene(tag)
    scene = dict(y=d['y'], atoms=d['atoms'], dsm_cfg=cfg, footprints=fps)
    for mode in _modes(tag):
        res = testing.solve_scene_gpu(scene, want_xi=True, mode=mode)
        recs = res['records']
        checked = 0
        for k in range(len(fps)):
            N, M = int(d[f'c{k}_N']), int(d[f'c{k}_M'])
            psi_ell = float(d[f'c{k}_psi_ell'])
            tol = 1e-6 * N / 1000 + 1e-5 * abs(psi_ell)
            if float(d[f'c{k}_gnorm_ell']) < 1e-8:
                assert abs(recs['energy_ell'][k] - psi_ell) <= tol, (mode, k, recs['energy_ell'][k], psi_ell)
            else:
                assert recs['energy_ell'][k] <= psi_ell + tol                    # near-separable: no finite minimiser
            if _tight(d, k):
                x = d[f'c{k}_x_dsm']
                xo = res['xi_offsets'][k]
                th, xi = recs['theta'][k], res['xi'][xo:xo + M]
                # the optimum is only determined to the solver's stopping accuracy (cond(Hessian) ~ 1e9 in these coordinates)
                assert np.abs(th - x[:6]).max() <= 5e-3 * np.abs(x[:6]).max(), (mode, k, th, x[:6])
                if M:
                    # Systems of several hundred unknowns -- `large_systems` -- have flat directions: grid points that few pixels see, under a
                    # regulariser that is all but linear at |xi| ~ 1e3; the stopping rule lambda^2 / 2 <= 1e-7 + 1e-6 f leaves them undetermined to
                    # a few per cent of the scale while the energy is within 1e-6 relative, hence the raw 5e-2 there.  What makes that bound
                    # safe is reference_optimum_checks below: the difference costs at most 2 tol in the metric of the reference's Hessian
                    # (assertion 2), its part in the stiff eigen-directions stays at the 5e-3 of the other tags (3), and the surfaces agree
                    # (5).  `group_regime` keeps the 5e-3 of the other tags: the CPU oracle's solver ends 4.7e-4 s from the reference there.
                    loose = tag == 'large_systems'
                    assert np.abs(xi - x[6:]).max() <= (5e-2 if loose else 5e-3) * max(1.0, np.abs(x[6:]).max()), (mode, k)
                    assert np.linalg.norm(xi - x[6:]) <= (5e-2 if loose else 5e-3) * max(1.0, np.linalg.norm(x[6:])), (mode, k)
                    reference_optimum_checks(tag, d, k, cfg, np.concatenate([th, xi]), label=f'{tag} mode {mode}')
                checked += 1
        assert checked == TIGHT_DEFORMABLE[tag]                                  # every tight pick (all of them have M > 0)


def test_point_evaluations_match_reference_energy(gpu):
    """psi, grad psi and the polynomial block of the Hessian of the solve kernels' evaluators (sdsm_batch_eval) at the 21
    parameter points of energy.npz (values of the reference's Energy incl. the exp() guard path, dsm.py:298-300)."""
    from superdsm_amd import engine
    d = np.load(os.path.join(G, 'energy.npz'))
    cfg0 = json.loads(str(d['cfg']))
    y, atoms = d['y'], d['atoms']
    img = engine.DeviceImage(y, None, atoms, cfg0['background_margin'])
    n_guard = 0
    for k in range(int(d['n_cases'])):
        deform = bool(d[f'c{k}_deform'])
        cfg = dict(cfg0, alpha=float(d[f'c{k}_alpha']), smooth_amount=cfg0['smooth_amount'] if deform else np.inf, init='elliptical', max_iters=1)
        batch = engine.Batch(img, [d[f'c{k}_fp'].tolist()], cfg)
        batch.launch()
        p = d[f'c{k}_params']
        assert int(batch.records()['n_deform'][0]) + 6 == p.size
        ev = batch.evaluate([p])[0]
        val, grad, H = float(d[f'c{k}_value']), d[f'c{k}_grad'], d[f'c{k}_hessian_lower']
        n_guard += int(d[f'c{k}_n_guarded'])
        assert abs(ev['psi'] - val) <= 1e-10 * abs(val), (k, ev['psi'], val)
        assert abs(ev['psi_value'] - val) <= 1e-10 * abs(val), (k, ev['psi_value'], val)
        np.testing.assert_allclose(ev['grad'], grad, rtol=1e-10, atol=1e-10 * np.abs(grad).max())
        # Hessian: kappa = theta - theta^2 loses digits in the reference as theta -> 1 (absolute error ~1e-16 per pixel; the kernels
        # use the product form u / (1 + u)^2, reciprocal to 2e-15): entries agree to 1e-13 of their natural scale sum y^2 |q_a q_b| <= 4 sum y^2
        sel = np.isin(atoms, d[f'c{k}_fp'])
        np.testing.assert_allclose(np.tril(ev['hess_theta']), H[:6, :6], rtol=1e-9, atol=4e-13 * float((y[sel] ** 2).sum()))
    assert n_guard > 0


def test_synthetic4096_matches_oracle(gpu):
    """BASELINE.json configs[4]: 4096x4096, ~2000 dense overlapping nuclei, every candidate (connected subsets <= 3 +
    universes) in one batch; a sample of >= 64 candidates against the CPU oracle on all host cores."""
    from oracle import oracle
    from superdsm_amd import _capi, testing
    scene = testing.make_scene('synthetic4096', max_size=3)
    fps = scene['footprints']
    res = testing.solve_scene_gpu(scene)
    recs = res['records']
    st, cnt = np.unique(recs['status'], return_counts=True)
    assert set(st.tolist()) <= {_capi.CAND_OPTIMAL, _capi.CAND_FALLBACK, _capi.CAND_TRIVIAL}, dict(zip(st.tolist(), cnt.tolist()))
    assert (recs['status'] == _capi.CAND_OPTIMAL).mean() > 0.99
    n = recs['n_deform'] + 6
    assert (n > 172).any() and ((n > 128) & (n <= 172)).any() and (n <= 40).any()       # every size class
    ok = recs['status'] == _capi.CAND_OPTIMAL
    assert np.isfinite(recs['energy'][ok]).all() and (recs['energy'][ok] <= recs['energy_ell'][ok] * (1 + 1e-9) + 1e-9).all()
    order = np.argsort(recs['n_pixels'])
    its = recs['iters_ell'] + recs['iters_dsm']
    sample = set(order[-12:].tolist()) | set(order[:6].tolist()) | set(order[len(order) // 2 - 3:len(order) // 2 + 3].tolist())
    sample |= set(np.argsort(recs['n_deform'])[-10:].tolist()) | set(np.argsort(its)[-12:].tolist())
    sample |= set(np.random.default_rng(4).choice(len(fps), 40, replace=False).tolist())
    # the solve classes between the common one and the global-memory one (1b: 6 + M <= 256, 2 / 2b: up to 512 with their envelope in LDS)
    for lo, hi in ((129, 200), (201, 256), (257, 340), (341, 512)):
        pool = np.flatnonzero((n >= lo) & (n <= hi))
        assert pool.size, (lo, hi)
        sample |= set(np.random.default_rng(lo).choice(pool, min(5, pool.size), replace=False).tolist())
    sample |= set(np.random.default_rng(5).choice(len(fps), 420, replace=False).tolist())
    # every candidate of the global-memory class (envelope beyond the LDS classes) and of class 2b
    env = np.array([d['env_size'] for d in res['batch'].inspect_states()])
    sample |= set(np.flatnonzero(env > 11000).tolist())
    sample = sorted(sample)
    assert len(sample) >= 500
    orecs, ofrags, _ = oracle.compute_objects(scene['y'], None, scene['atoms'], [fps[i] for i in sample], scene['dsm_cfg'], nthreads=0)
    for j, k in enumerate(sample):
        assert (recs['n_pixels'][k], recs['n_deform'][k]) == (orecs['N'][j], orecs['M'][j]), k
        if orecs['status'][j] == 2:
            assert recs['status'][k] == _capi.CAND_TRIVIAL
            continue
        tol = 1e-6 * orecs['N'][j] / 1000 + 1e-5 * abs(orecs['energy'][j])
        if orecs['energy'][j] < 1e-3:                      # separable region: psi has no finite minimiser, inf psi = 0; the value is the stopping rule's
            assert recs['energy'][k] <= orecs['energy'][j] + tol, (k, recs['energy'][k], orecs['energy'][j])
        elif np.abs(orecs['theta'][j]).max() > 1e9 and orecs['energy'][j] < 1e-4 * orecs['N'][j] * np.log(2):
            # a region that is separable but for a pixel or two: the model runs off (theta ~ 1e14 after 80 iterations here), the Hessian
            # is singular to working precision and WHERE the iteration stops is decided by the rounding of its pivots; both values are
            # 1e-4 of the energy of the empty model (N ln 2) and mean "no energy" to the set cover (beta >= 100)
            assert recs['energy'][k] < 1e-4 * orecs['N'][j] * np.log(2), (k, recs['energy'][k], orecs['energy'][j])
            continue
        else:
            assert abs(recs['energy'][k] - orecs['energy'][j]) <= tol, (k, recs['energy'][k], orecs['energy'][j])
        assert testing.dice(res['fragments'][k][0], res['fragments'][k][1], orecs['fg_offset'][j], ofrags[j], scene['y'].shape) >= 0.999, k
        if bool(recs['on_boundary'][k]) != bool(orecs['on_boundary'][j]) and orecs['energy'][j] >= 1e-3:
            # on_boundary = "S > 0 somewhere on the 1-px pad ring of the IMAGE" (objects.py:209): the quadratic extrapolated thousands of
            # pixels away from its region.  The flags may only differ where that maximum is zero to the accuracy of the parameters
            # (the optimum is determined to the stopping tolerance): both models' ring maxima within 1 % of the ring's range of S.
            # (Not for separable regions, inf psi = 0: their parameters run off -- |theta| ~ 1e10 and more -- and where the iteration
            # stops decides the sign of S far away; the masks agree all the same.)
            mg, rg = _ring_max(recs['theta'][k], scene['y'].shape)
            mo, ro = _ring_max(orecs['theta'][j], scene['y'].shape)
            assert abs(mg) <= 0.01 * rg and abs(mo) <= 0.01 * ro, (k, mg, rg, mo, ro)


def _ring_max(theta, shape):
    """(max of the polynomial surface over the 1-px pad ring of the image, max |S| there) for theta in full-image-normalised
    coordinates (dsm.py:113-128: x_norm = (x_pad - 1) / (shape - 1))."""
    H, W = shape
    a1, a2, a3, b1, b2, c = (float(v) for v in theta)
    r = np.concatenate([np.full(W + 2, -1.0), np.full(W + 2, float(H)), np.arange(-1, H + 1, dtype=float), np.arange(-1, H + 1, dtype=float)]) / (H - 1)
    q = np.concatenate([np.arange(-1, W + 1, dtype=float), np.arange(-1, W + 1, dtype=float), np.full(H + 2, -1.0), np.full(H + 2, float(W))]) / (W - 1)
    S = a1 * r * r + a2 * q * q + 2 * a3 * r * q + 2 * b1 * r + 2 * b2 * q + c
    return float(S.max()), float(np.abs(S).max())


@pytest.mark.parametrize('layout', [4, 6, 7])
def test_further_bbbc039_layouts_every_candidate_matches_oracle(gpu, layout):
    """Three more of the reference's BBBC039 object tables (488 / 655 / 855 candidates; 117 .. 170 objects, denser images with small
    atoms whose regions are separable or nearly so): every candidate against the oracle -- energy, status, mask -- and the number
    of passes over the pixels: a solve that wanders (lost digits in its sums) shows up there first."""
    from oracle import oracle
    from superdsm_amd import testing
    scene = testing.make_scene('bbbc039_like', max_size=3, layout_index=layout)
    fps = scene['footprints']
    res = testing.solve_scene_gpu(scene)
    recs = res['records']
    orecs, ofrags, _ = oracle.compute_objects(scene['y'], None, scene['atoms'], fps, scene['dsm_cfg'], nthreads=0)
    np.testing.assert_array_equal(recs['n_pixels'], orecs['N'])
    np.testing.assert_array_equal(recs['n_deform'], orecs['M'])
    np.testing.assert_array_equal(recs['status'], orecs['status'])
    ev = recs['evals_full'].astype(np.int64) + recs['evals_value']
    assert (ev <= 2 * orecs['evals'] + 40).all(), np.flatnonzero(ev > 2 * orecs['evals'] + 40)
    assert abs(int(ev.sum()) - int(orecs['evals'].sum())) <= 0.03 * orecs['evals'].sum()
    for k in range(len(fps)):
        if orecs['status'][k] == 2:
            continue
        tol = 1e-6 * orecs['N'][k] / 1000 + 1e-5 * abs(orecs['energy'][k])
        if orecs['energy'][k] < 1e-4 * orecs['N'][k] * np.log(2) and (orecs['energy'][k] < 1e-3 or np.abs(orecs['theta'][k]).max() > 1e9):
            # separable (or all but): inf psi = 0 is not attained, the value is the stopping rule's -- "no energy" on both sides
            assert recs['energy'][k] < 1e-4 * orecs['N'][k] * np.log(2), (k, recs['energy'][k], orecs['energy'][k])
        else:
            assert abs(recs['energy'][k] - orecs['energy'][k]) <= tol, (k, recs['energy'][k], orecs['energy'][k])
            assert testing.dice(res['fragments'][k][0], res['fragments'][k][1], orecs['fg_offset'][k], ofrags[k], scene['y'].shape) >= 0.999, k


def test_bbbc039_like_every_candidate_matches_oracle(gpu):
    """BASELINE.json configs[1] stand-in at full size: all 501 candidates against the oracle (energies, status, masks)."""
    from oracle import oracle
    from superdsm_amd import testing
    scene = testing.make_scene('bbbc039_like', max_size=3)
    fps = scene['footprints']
    res = testing.solve_scene_gpu(scene)
    recs = res['records']
    orecs, ofrags, _ = oracle.compute_objects(scene['y'], None, scene['atoms'], fps, scene['dsm_cfg'], nthreads=0)
    np.testing.assert_array_equal(recs['n_pixels'], orecs['N'])
    np.testing.assert_array_equal(recs['n_deform'], orecs['M'])
    np.testing.assert_array_equal(recs['status'], orecs['status'])
    worst = 1.0
    for k in range(len(fps)):
        tol = 1e-6 * orecs['N'][k] / 1000 + 1e-5 * abs(orecs['energy'][k])
        assert abs(recs['energy'][k] - orecs['energy'][k]) <= tol, (k, recs['energy'][k], orecs['energy'][k])
        assert bool(recs['on_boundary'][k]) == bool(orecs['on_boundary'][k])
        worst = min(worst, testing.dice(res['fragments'][k][0], res['fragments'][k][1], orecs['fg_offset'][k], ofrags[k], scene['y'].shape))
    assert worst >= 0.999, worst


def _two_blob_scene(seed=3, H=96, W=128):
    from superdsm_amd import testing
    return testing.two_blob_scene(seed, H, W)


@pytest.mark.parametrize('max_iters', [1, 2, 3, 6])
def test_iteration_cap_forces_the_elliptical_retry_and_unknown_status(gpu, max_iters):
    """A Newton iteration cap of a few steps makes the first elliptical solve end 'unknown' -> the retry from the moment
    initialisation (objects.py:337-355, record flag bit 0) and an 'unknown' DSM solve that still counts as optimal because
    it is not worse than its start (objects.py:399-400).  Flags, iteration counts and energies against the oracle run with
    the same cap."""
    from oracle import oracle
    from superdsm_amd import _capi, engine
    y, atoms = _two_blob_scene()
    cfg = dict(scale=1000, epsilon=1.0, alpha=0.033, smooth_amount=4, smooth_subsample=8, gaussian_shape_multiplier=2,
               background_margin=8, init='elliptical', max_iters=max_iters)
    fps = [[1], [2], [1, 2]]
    img = engine.DeviceImage(y, None, atoms, cfg['background_margin'])
    batch = engine.Batch(img, fps, cfg)
    batch.launch()
    gpu.cuda.synchronize()
    recs = batch.records()
    for k, fp in enumerate(fps):
        mask = oracle.region_mask(y, None, atoms, fp, cfg['background_margin'])
        _, info = oracle.cvxprog(y, mask, cfg)
        assert recs['status'][k] == info['status'] == _capi.CAND_OPTIMAL
        assert (recs['flags'][k] & 1) == info['retried'], (k, recs['flags'][k], info)
        assert recs['iters_ell'][k] == info['iters_ell'] and recs['iters_dsm'][k] == info['iters_dsm'] <= max_iters
        assert abs(recs['energy'][k] - info['energy']) <= 1e-7 * abs(info['energy']), (k, recs['energy'][k], info['energy'])
        assert abs(recs['energy_ell'][k] - info['energy_ell']) <= 1e-7 * abs(info['energy_ell'])
        assert recs['energy'][k] <= recs['energy_ell'][k] * (1 + 1e-12)
    if max_iters <= 3:
        assert (recs['flags'] & 1).all(), 'a cap this small must leave the first elliptical solve unfinished'


def test_failed_dsm_solve_falls_back_and_failed_elliptical_solve_is_an_error(gpu):
    """alpha = inf: the regulariser makes psi non-finite for M >= 1 (the reference's Energy raises, dsm.py:325-331) -> the
    DSM solve is an 'exception' -> status fallback with the elliptical parameters (objects.py:406-410).  A non-finite
    intensity makes the elliptical solves fail twice -> CvxprogError carrying the candidate index (objects.py:351-353)."""
    from oracle import oracle
    from superdsm_amd import _capi, engine, image, objects
    y, atoms = _two_blob_scene(seed=4)
    cfg = dict(scale=1000, epsilon=1.0, alpha=np.inf, smooth_amount=4, smooth_subsample=8, gaussian_shape_multiplier=2,
               background_margin=8, init='elliptical')
    fps = [[1], [2]]
    img = engine.DeviceImage(y, None, atoms, cfg['background_margin'])
    batch = engine.Batch(img, fps, cfg, want_xi=True)
    batch.launch()
    gpu.cuda.synchronize()
    recs = batch.records()
    frags = batch.fragments(recs)
    ell = engine.Batch(img, fps, dict(cfg, alpha=0.033, smooth_amount=np.inf))      # the elliptical models alone
    ell.launch()
    gpu.cuda.synchronize()
    erecs = ell.records()
    efrags = ell.fragments(erecs)
    for k, fp in enumerate(fps):
        mask = oracle.region_mask(y, None, atoms, fp, cfg['background_margin'])
        _, info = oracle.cvxprog(y, mask, cfg)
        assert recs['status'][k] == _capi.CAND_FALLBACK and info['status'] == 1
        assert recs['n_deform'][k] == info['M'] > 0
        # (the elliptical-only batch sums the pixels in another order -- its crop is not sorted by G~ row length --, so its iterates differ in the last digits)
        np.testing.assert_allclose(recs['theta'][k], erecs['theta'][k], rtol=0, atol=1e-5 * np.abs(erecs['theta'][k]).max())
        assert abs(recs['energy_ell'][k] - erecs['energy'][k]) <= 1e-9 * abs(erecs['energy'][k])
        assert (batch.xi_dev.cpu().numpy() == 0).all()
        np.testing.assert_array_equal(frags[k][1], efrags[k][1])
    # through the reference-style API a fallback is not an error: is_optimal False, counted in the status line
    yi = image.Image.create_from_array(y, normalize=False)
    objs = [objects.Object() for _ in fps]
    for o, fp in zip(objs, fps):
        o.footprint = set(fp)
    objects.compute_objects(objs, yi, atoms, cfg, None, out='muted')
    assert all(o.is_optimal is False for o in objs)
    # a candidate whose elliptical solves both fail
    y2 = y.copy()
    y2[40, 30] = np.inf
    cfg2 = dict(cfg, alpha=0.033)
    img2 = engine.DeviceImage(y2, None, atoms, cfg2['background_margin'])
    b2 = engine.Batch(img2, fps, cfg2)
    b2.launch()
    gpu.cuda.synchronize()
    r2 = b2.records()
    assert r2['status'][0] == _capi.CAND_ERROR and r2['status'][1] == _capi.CAND_OPTIMAL
    m0 = oracle.region_mask(y2, None, atoms, fps[0], cfg2['background_margin'])
    assert oracle.cvxprog(y2, m0, cfg2)[1]['status'] == 3
    yi2 = image.Image.create_from_array(y2, normalize=False)
    with pytest.raises(objects.CvxprogError) as err:
        objects.compute_objects(objs, yi2, atoms, cfg2, None, out='muted')
    assert err.value.cidx == 0


def test_more_than_1018_deformation_parameters_are_solved_by_the_global_memory_class(gpu):
    """6 + M > 1024 exceeds the LDS classes and the workgroup groups; the global-memory class holds vectors of 2048 unknowns (round 4: the
    reference has no limit, objects.py:396-410): a DSM solve within the tolerance of the CPU oracle for an ordinary region (M = 1176) and for
    one that would otherwise be solved by a workgroup group (17 k pixels, M = 1908) -- and through compute_objects optimal objects."""
    from oracle import oracle
    from superdsm_amd import _capi, engine, image, objects, testing
    rng = np.random.default_rng(8)
    H, W = 150, 170
    rr, cc = np.mgrid[:H, :W]
    y = -0.1 + 0.02 * rng.standard_normal((H, W))
    y += 0.4 * np.exp(-(((rr - 75) / 50.0) ** 2 + ((cc - 85) / 58.0) ** 2) ** 2)
    atoms = np.ones((H, W), np.int32)
    atoms[:, 100:] = 2
    cfg = dict(scale=1000, epsilon=1.0, alpha=0.05, smooth_amount=2, smooth_subsample=3, gaussian_shape_multiplier=2,
               background_margin=12, init='elliptical')
    fps = [[1], [2], [1, 2]]
    orecs, ofrags, _ = oracle.compute_objects(y, None, atoms, fps, cfg, nthreads=0)
    img = engine.DeviceImage(y, None, atoms, cfg['background_margin'])
    batch = engine.Batch(img, fps, cfg)
    batch.launch()
    gpu.cuda.synchronize()
    recs = batch.records()
    frags = batch.fragments(recs)
    assert recs['n_pixels'][2] > 12288 and recs['n_pixels'][0] <= 12288
    assert (recs['n_deform'][[0, 2]] > 1018).all() and recs['n_deform'][1] <= 1018
    np.testing.assert_array_equal(recs['n_deform'], orecs['M'])
    assert (recs['status'] == _capi.CAND_OPTIMAL).all(), recs['status']
    for k in range(3):
        tol = 1e-6 * orecs['N'][k] / 1000 + 1e-5 * abs(orecs['energy'][k])
        assert abs(recs['energy'][k] - orecs['energy'][k]) <= tol, (k, recs['energy'][k], orecs['energy'][k])
        assert recs['energy'][k] < recs['energy_ell'][k]
        assert testing.dice(frags[k][0], frags[k][1], orecs['fg_offset'][k], ofrags[k], y.shape) >= 0.999, k
    yi = image.Image.create_from_array(y, normalize=False)
    objs = []
    for fp in fps:
        o = objects.Object()
        o.footprint = set(fp)
        objs.append(o)
    objects.compute_objects(objs, yi, atoms, cfg, None, out='muted')
    assert [o.is_optimal for o in objs] == [True, True, True]
    for k in range(3):
        assert objs[k].energy == recs['energy'][k]


def test_regions_beyond_the_setup_tables_get_the_elliptical_result_not_an_abort(gpu):
    """More grid points than the setup kernel's tables hold (here: smooth_subsample 2 on a 17 k-pixel region: M ~ 4300 > 2048): status
    UNSUPPORTED WITH the elliptical result -- through compute_objects a usable object (the elliptical solution as a fallback with a warning),
    never an abort of the batch (objects.py:399-410: failure => fallback); the other candidates of the batch are solved as usual."""
    from superdsm_amd import _capi, engine, image, objects, testing
    sc = testing.beyond_setup_tables_scene()
    y, atoms, cfg, fps = sc['y'], sc['atoms'], sc['cfg'], sc['footprints']
    img = engine.DeviceImage(y, None, atoms, cfg['background_margin'])
    batch = engine.Batch(img, fps, cfg)
    batch.launch()
    gpu.cuda.synchronize()
    recs = batch.records()
    assert recs['status'][0] == _capi.CAND_UNSUPPORTED and recs['status'][1] == _capi.CAND_OPTIMAL, recs['status']
    ell = engine.Batch(img, fps, dict(cfg, smooth_amount=np.inf))
    ell.launch()
    gpu.cuda.synchronize()
    erecs = ell.records()
    assert abs(recs['energy'][0] - erecs['energy'][0]) <= 1e-6 * abs(erecs['energy'][0])
    assert abs(recs['energy'][0] - recs['energy_ell'][0]) <= 1e-9 * abs(recs['energy'][0])
    yi = image.Image.create_from_array(y, normalize=False)
    objs = []
    for fp in fps:
        o = objects.Object()
        o.footprint = set(fp)
        objs.append(o)
    with pytest.warns(RuntimeWarning, match='elliptical solution is returned'):
        objects.compute_objects(objs, yi, atoms, cfg, None, out='muted')
    assert not objs[0].is_optimal
    assert abs(objs[0].energy - erecs['energy'][0]) <= 1e-6 * abs(erecs['energy'][0])
    assert objs[0].fg_fragment.any() and objs[0].fg_fragment.shape == tuple(int(v) for v in (recs['fg_h'][0], recs['fg_w'][0]))


# ---------------------------------------------------------------------------------------------------------
# plans over several images, image sets in lock step (BASELINE.json configs[3]), scheduling corner cases
# ---------------------------------------------------------------------------------------------------------
def _flipped(scene):
    """A second, different image with the same hyper-parameters: the scene mirrored (atoms, clusters and graph rebuilt)."""
    from superdsm_amd import synth
    from superdsm_amd.atoms import AtomAdjacencyGraph
    y = np.ascontiguousarray(scene['y'][::-1, ::-1])
    atoms = np.ascontiguousarray(scene['atoms'][::-1, ::-1])
    clusters = np.ascontiguousarray(scene['clusters'][::-1, ::-1])
    H, W = y.shape
    seeds = [(H - 1 - int(r), W - 1 - int(c)) for r, c in scene['seeds']]
    adj = AtomAdjacencyGraph(atoms, clusters, y > 0, seeds)
    return dict(scene, y=y, atoms=atoms, clusters=clusters, seeds=seeds, adjacencies=adj, footprints=synth.enumerate_candidates(adj, max_size=3))


def test_multi_image_plan_equals_single_image_plans(gpu):
    """sdsm_plan_create_multi: candidates of three images (two shapes) in ONE launch give the records and masks of three
    single-image launches."""
    from superdsm_amd import engine, testing
    a = testing.make_scene('synthetic256', max_size=2)
    b = _flipped(a)
    c = testing.make_scene('bbbc039_like', max_size=2)
    c = dict(c, footprints=c['footprints'][::9])
    scenes = [a, b, c]
    cfg = a['dsm_cfg']
    assert c['dsm_cfg'] == cfg
    imgs = [engine.DeviceImage(s['y'], None, s['atoms'], cfg['background_margin']) for s in scenes]
    fps, image_of = [], []
    for k, s in enumerate(scenes):
        fps += s['footprints']
        image_of += [k] * len(s['footprints'])
    order = np.random.default_rng(1).permutation(len(fps))            # candidates of the images interleaved
    multi = engine.Batch(imgs, [fps[i] for i in order], cfg, image_of=[image_of[i] for i in order])
    multi.launch()
    mrec, mmask = multi.download()
    mrec = mrec.copy()
    mfr = multi.fragments(mrec, masks=mmask)
    pos = {int(i): j for j, i in enumerate(order)}
    k0 = 0
    for k, s in enumerate(scenes):
        single = engine.Batch(imgs[k], s['footprints'], cfg)
        single.launch()
        srec, smask = single.download()
        sfr = single.fragments(srec, masks=smask)
        for i in range(len(s['footprints'])):
            j = pos[k0 + i]
            assert (mrec['n_pixels'][j], mrec['n_deform'][j], mrec['status'][j]) == (srec['n_pixels'][i], srec['n_deform'][i], srec['status'][i])
            # byte for byte: a candidate's record and mask do not depend on the plan it is in (other images, other candidates,
            # another scheduling mode -- the single-image plan runs 192- and the other 256-thread workgroups for the same regions)
            assert mrec[j].tobytes() == srec[i].tobytes(), (k, i)
            assert tuple(mfr[j][0]) == tuple(sfr[i][0]) and np.array_equal(mfr[j][1], sfr[i][1])
        k0 += len(s['footprints'])


def test_image_set_in_lock_step_equals_image_by_image(gpu):
    """BASELINE.json configs[3] (image set): GlobalEnergyMinimization.process_many solves generation k of all images as one
    multi-image batch; covers, costs and performance counters equal those of the stage run image by image, and the
    NIH3T3-like image's cover equals the one the CPU oracle drives."""
    from oracle import oracle
    from superdsm_amd import config, globalenergymin, testing
    base = testing.make_scene('nih3t3_like', max_size=2)
    scenes = [base, _flipped(base), dict(base, y=np.ascontiguousarray(base['y'] * 0.97))]
    beta = 1200.0
    cfg = config.Config({'global-energy-minimization': {'beta': beta, 'pruning': 'isbi24'}})
    stage = globalenergymin.GlobalEnergyMinimization()
    mk = lambda s: dict(y=s['y'], y_mask=np.ones(s['y'].shape, bool), atoms=s['atoms'], adjacencies=s['adjacencies'], dsm_cfg=s['dsm_cfg'])
    together = [mk(s) for s in scenes]
    stage.process_many(together, cfg, out='muted')
    assert stage.last_lockstep.batches >= 1                  # (with the generations solved ahead the whole set may need a single batch)
    cov = lambda dd: sorted(sorted(int(a) for a in o.footprint) for o in dd['cover'].solution)
    plain = [mk(s) for s in scenes]                          # the reference's batches (one per generation) in lock step: the same covers
    stage.process_many(plain, config.Config({'global-energy-minimization': {'beta': beta, 'pruning': 'isbi24', 'speculation': 0}}), out='muted')
    assert stage.last_lockstep.batches >= 2
    for d, q in zip(together, plain):
        assert cov(d) == cov(q) and d['cover'].costs == q['cover'].costs
    for s, d in zip(scenes, together):
        alone = mk(s)
        stage(alone, cfg, out='muted')
        assert cov(d) == cov(alone)
        assert d['cover'].costs == alone['cover'].costs
        # `process` and `process_many`: identical energies, bit for bit (a candidate's numbers do not depend on its batch: the threshold
        # comparisons of globalenergymin.py:361 cannot flip between the two)
        ea = {tuple(sorted(int(a) for a in o.footprint)): float(o.energy).hex() for o in alone['objects']}
        ed = {tuple(sorted(int(a) for a in o.footprint)): float(o.energy).hex() for o in d['objects']}
        assert ea == ed
        for k in d['performance'].attributes:
            assert getattr(d['performance'], k) == getattr(alone['performance'], k)
    # the first image against the oracle-driven stage
    def oracle_compute(objs, y, atoms, dsm_cfg, log_root_dir, status_line=None, out=None, shard=None):
        objs = list(objs)
        if not objs:
            return
        recs, frags, _ = oracle.compute_objects(y.model, None, atoms, [sorted(o.footprint) for o in objs], dsm_cfg, nthreads=0)
        for o, r, f in zip(objs, recs, frags):
            o.energy, o.is_optimal, o.on_boundary, o.processing_time = float(r['energy']), bool(r['is_optimal']), bool(r['on_boundary']), 0
            o.fg_offset, o.fg_fragment = np.array(r['fg_offset']), f
    ref = mk(scenes[0])
    import unittest.mock as mock
    with mock.patch.object(globalenergymin, 'compute_objects', oracle_compute):
        stage(ref, cfg, out='muted')
    assert sorted(sorted(int(a) for a in o.footprint) for o in ref['cover'].solution) == sorted(sorted(int(a) for a in o.footprint) for o in together[0]['cover'].solution)
    seg = [np.zeros(scenes[0]['y'].shape, bool) for _ in range(2)]
    for o in together[0]['cover'].solution:
        o.fill_foreground(seg[0])
    for o in ref['cover'].solution:
        o.fill_foreground(seg[1])
    assert 2 * (seg[0] & seg[1]).sum() / max(1, seg[0].sum() + seg[1].sum()) >= 0.999


def test_generations_solved_ahead_give_the_same_stage_results_in_fewer_batches(gpu):
    """The stage with its default (one generation solved ahead per engine batch, globalenergymin._Speculation) against
    `speculation: 0` (the reference's batches exactly) on the BBBC039-like image: same generations, same cover, same counters,
    energies equal (a candidate's solve does not depend on what else is in its batch), about half the round trips."""
    from superdsm_amd import config, globalenergymin, testing
    scene = testing.make_scene('bbbc039_like', max_size=3)
    mk = lambda: dict(y=scene['y'], y_mask=np.ones(scene['y'].shape, bool), atoms=scene['atoms'], adjacencies=scene['adjacencies'], dsm_cfg=scene['dsm_cfg'])
    stage = globalenergymin.GlobalEnergyMinimization()
    runs = {}
    for depth in (0, None, 2):
        gem = {'beta': 150.0, 'pruning': 'isbi24'}
        if depth is not None:
            gem['speculation'] = depth
        d = mk()
        stage(d, config.Config({'global-energy-minimization': gem}), out='muted')
        runs[depth] = d
    plain = runs[0]
    assert not hasattr(plain['performance'], 'engine_batches')
    for depth in (None, 2):
        d = runs[depth]
        assert sorted(sorted(int(a) for a in o.footprint) for o in d['cover'].solution) == sorted(sorted(int(a) for a in o.footprint) for o in plain['cover'].solution)
        assert [sorted(o.footprint) for o in d['objects']] == [sorted(o.footprint) for o in plain['objects']]
        assert [o.energy for o in d['objects']] == [o.energy for o in plain['objects']]          # the same bits
        assert d['cover'].costs == plain['cover'].costs
        for k in d['performance'].attributes:
            assert getattr(d['performance'], k) == getattr(plain['performance'], k)
    assert runs[None]['performance'].engine_batches <= 5 and runs[2]['performance'].engine_batches <= 4    # 8 batches without


def test_given_up_workgroup_group_is_solved_again_without_groups(gpu):
    """With a (diagnostic) time limit of a fraction of a microsecond the members of a workgroup group give their candidate up at
    the first all-reduce: status GIVEN_UP for exactly the grouped candidates, everything else unaffected; compute_objects solves
    them again without groups and nothing is raised."""
    from oracle import oracle
    from superdsm_amd import _capi, engine, image, objects
    rng = np.random.default_rng(31)
    H, W = 190, 210
    rr, cc = np.mgrid[:H, :W]
    y = -0.1 + 0.02 * rng.standard_normal((H, W))
    y += 0.45 * np.exp(-(((rr - 95) / 60.0) ** 2 + ((cc - 100) / 75.0) ** 2) ** 2)
    atoms = np.ones((H, W), np.int32)
    atoms[:, 150:] = 2
    cfg = dict(scale=1000, epsilon=1.0, alpha=0.05, smooth_amount=6.0, smooth_subsample=12, gaussian_shape_multiplier=2,
               background_margin=10, init='elliptical')
    fps = [[1], [2], [1, 2]]
    orecs, _, _ = oracle.compute_objects(y, None, atoms, fps, cfg, nthreads=0)
    img = engine.DeviceImage(y, None, atoms, cfg['background_margin'])
    L = _capi.lib()
    L.sdsm_set_group_timeout_us(0.02)
    try:
        batch = engine.Batch(img, fps, cfg)
        batch.launch()
        gpu.cuda.synchronize()
        recs = batch.records()
        grouped = recs['n_pixels'] > 12288
        assert grouped.any() and not grouped.all()
        assert (recs['status'][grouped] == _capi.CAND_GIVEN_UP).all() and (recs['status'][~grouped] == _capi.CAND_OPTIMAL).all()
        for k in np.flatnonzero(~grouped):
            assert abs(recs['energy'][k] - orecs['energy'][k]) <= 1e-6 * orecs['N'][k] / 1000 + 1e-5 * abs(orecs['energy'][k])
        yi = image.Image.create_from_array(y, normalize=False)
        objs = [objects.Object() for _ in fps]
        for o, fp in zip(objs, fps):
            o.footprint = set(fp)
        objects.compute_objects(objs, yi, atoms, cfg, None, out='muted')         # mode 1 groups give up too; the retry has none
        for k, o in enumerate(objs):
            assert o.is_optimal and abs(o.energy - orecs['energy'][k]) <= 1e-6 * orecs['N'][k] / 1000 + 1e-5 * abs(orecs['energy'][k])
    finally:
        L.sdsm_set_group_timeout_us(0.0)
    batch.launch()                                                               # default limit again: the groups complete
    gpu.cuda.synchronize()
    assert (batch.records()['status'] == _capi.CAND_OPTIMAL).all()


def test_groups_of_both_lds_layouts_give_the_bytes_of_single_workgroups(gpu):
    """The largest candidates of two BBBC039-like images with 14-17 k-pixel clusters: in throughput mode (mode 0) the regions above
    12 288 pixels are solved by workgroup groups -- with the LDS layout of class 2 when the Hessian envelope has at most 11 000 doubles,
    with that of class 2b (up to 15 300) otherwise -- in mode 2 by single workgroups; latency mode (1) groups the mid-size regions too.
    The records are the same 128 bytes, and they match the CPU oracle."""
    from oracle import oracle
    from superdsm_amd import engine, testing
    fps, image_of, scenes = [], [], []
    for k, layout in enumerate((1, 2)):
        sc = testing.make_scene('bbbc039_like', layout_index=layout)
        cnt = np.bincount(sc['atoms'].ravel())
        big = sorted(sc['footprints'], key=lambda fp: -sum(cnt[a] for a in fp))[:14]
        scenes.append(dict(sc, footprints=big))
        fps += big
        image_of += [k] * len(big)
    cfg = scenes[0]['dsm_cfg']
    imgs = [engine.DeviceImage(sc['y'], None, sc['atoms'], cfg['background_margin']) for sc in scenes]
    recs = {}
    for mode in (0, 1, 2):
        b = engine.Batch(imgs, fps, cfg, image_of=image_of, mode=mode)
        b.launch()
        gpu.cuda.synchronize()
        recs[mode] = b.records().copy()
        if mode == 0:
            env = np.array([st['env_size'] for st in b.inspect_states()])
    N = recs[0]['n_pixels']
    grouped = N > 12288
    assert (grouped & (env <= 11000)).any() and (grouped & (env > 11000) & (env <= 15170)).any(), 'the sample must hold groups of both layouts'
    assert (recs[0]['status'] == 0).all()
    for mode in (1, 2):
        assert recs[mode].tobytes() == recs[0].tobytes(), mode
    k0 = 0
    for sc in scenes:
        orecs, _, _ = oracle.compute_objects(sc['y'], None, sc['atoms'], sc['footprints'], sc['dsm_cfg'], nthreads=0)
        r = recs[0][k0:k0 + len(sc['footprints'])]
        assert (r['status'] == orecs['status']).all()
        assert (np.abs(r['energy'] - orecs['energy']) <= 1e-6 * orecs['N'] / 1000 + 1e-5 * np.abs(orecs['energy'])).all()
        k0 += len(sc['footprints'])


def test_callable_dsm_init_starts_the_deformable_solve_where_the_caller_says(gpu):
    """dsm/init as a callable (reference: objects.py:385-386, ``params = init(J.smooth_mat.shape[1])``): it is called with the number of columns of
    the candidate's G~ -- known after the setup kernel -- and its return value is where the DSM solve starts (no elliptical model first).
    init(m) = zeros is the reference's ``init=None`` path: the same bytes; another start: the oracle's solver from the same point reaches
    the same energy, and the reported energy is the reference's energy function at the returned parameters."""
    from oracle import oracle
    from superdsm_amd import _capi, engine, image, objects, testing
    scene = testing.make_scene('synthetic256', max_size=2)
    fps, cfg = scene['footprints'][:40], scene['dsm_cfg']
    img = engine.DeviceImage(scene['y'], None, scene['atoms'], cfg['background_margin'])
    b0 = engine.Batch(img, fps, dict(cfg, init=None))
    b0.launch()
    r0 = b0.records()
    called = []
    def zeros(m):
        called.append(m)
        return np.zeros(6 + m)
    b1 = engine.Batch(img, fps, dict(cfg, init=zeros))
    start = objects._starting_points(b1, dict(cfg, init=zeros))
    b1.launch()
    r1 = b1.records()
    assert r0.tobytes() == r1.tobytes()
    solved = r0['status'] != _capi.CAND_TRIVIAL
    assert solved.sum() >= 30 and called == r0['n_deform'][solved].tolist() and [s is not None for s in start] == solved.tolist()
    with pytest.raises(_capi.SdsmError, match='elliptical'):                # a plan that solves the elliptical model first has no use for starting points
        engine.Batch(img, fps, cfg).set_start(start)
    # the same for regions whose rows of G~ a second kernel builds and that workgroup groups solve (the counts come from the first setup kernel alone)
    big = testing.make_scene('gowt1_like', max_size=2)
    bimg = engine.DeviceImage(big['y'], None, big['atoms'], big['dsm_cfg']['background_margin'])
    g0 = engine.Batch(bimg, big['footprints'], dict(big['dsm_cfg'], init=None))
    g0.launch()
    g1 = engine.Batch(bimg, big['footprints'], dict(big['dsm_cfg'], init=zeros))
    objects._starting_points(g1, dict(big['dsm_cfg'], init=zeros))
    g1.launch()
    rg = g0.records()
    assert rg.tobytes() == g1.records().tobytes() and rg['n_pixels'].max() > 40000 and rg['n_deform'].max() > 128
    # a start of its own: a circle around the image centre and small alternating deformations
    def circle(m):
        xi = 0.01 * (-1.0) ** np.arange(m)
        return np.concatenate([[-100.0, -100.0, 0.0, 50.0, 50.0, -49.0], xi])
    yi = image.Image.create_from_array(scene['y'], normalize=False)
    objs = [objects.Object() for _ in fps]
    for o, fp in zip(objs, fps):
        o.footprint = set(fp)
    objects.compute_objects(objs, yi, scene['atoms'], dict(cfg, init=circle), None, out='muted')
    with pytest.raises(ValueError, match='finite parameters'):
        objects.compute_objects(objs[:3], yi, scene['atoms'], dict(cfg, init=lambda m: np.zeros(5 + m)), None, out='muted')
    b2 = engine.Batch(img, fps, dict(cfg, init=circle), want_xi=True)
    objects._starting_points(b2, dict(cfg, init=circle))
    b2.launch()
    r2, xi, xo = b2.records(), b2.xi_dev.cpu().numpy(), b2.xi_offsets()
    checked = 0
    for k in np.flatnonzero(solved)[:12]:
        mask = oracle.region_mask(scene['y'], None, scene['atoms'], fps[k], cfg['background_margin'])
        J = oracle.Energy(scene['y'], mask, cfg['epsilon'], cfg['alpha'], cfg['smooth_amount'], cfg['gaussian_shape_multiplier'], cfg['smooth_subsample'])
        assert J.M == r2['n_deform'][k]
        p = np.concatenate([r2['theta'][k], xi[xo[k]:xo[k] + J.M]])
        assert abs(J(p) - r2['energy'][k]) <= 1e-9 * max(1.0, abs(r2['energy'][k]))
        assert objs[k].energy == r2['energy'][k]                            # compute_objects went the same way
        x, info = J.newton(circle(J.M), cfg['scale'] / J.N)
        if info['status'] == 0 and r2['status'][k] == _capi.CAND_OPTIMAL:
            tol = 1e-6 * J.N / 1000 + 1e-5 * abs(info['value'])
            assert abs(r2['energy'][k] - info['value']) <= tol, (k, r2['energy'][k], info['value'])
            checked += 1
        else:                                                               # fallback: the initialisation itself (objects.py:409-410)
            assert r2['status'][k] in (_capi.CAND_FALLBACK, _capi.CAND_OPTIMAL)
            if r2['status'][k] == _capi.CAND_FALLBACK:
                np.testing.assert_allclose(p, circle(J.M), rtol=1e-12, atol=1e-12)
    assert checked >= 6, checked


def test_launch_refuses_a_workspace_uploaded_before_a_layout_change(gpu, tmp_path):
    """sdsm_plan_set_latency_mode changes the launch lists that sdsm_batch_upload put on the device: a launch with the stale
    tables is an argument error, not undefined behaviour.  Also: per-candidate log files of compute_objects."""
    import ctypes as C
    from superdsm_amd import _capi, engine, image, objects, testing
    scene = testing.make_scene('synthetic256', max_size=2)
    img = engine.DeviceImage(scene['y'], None, scene['atoms'], scene['dsm_cfg']['background_margin'])
    batch = engine.Batch(img, scene['footprints'], scene['dsm_cfg'])
    batch.launch()
    L = _capi.lib()
    assert L.sdsm_plan_set_latency_mode(batch.plan, 1) == 0
    with pytest.raises(_capi.SdsmError, match='stale'):
        batch.launch()
    assert L.sdsm_plan_set_latency_mode(batch.plan, 7) == -1
    yi = image.Image.create_from_array(scene['y'], normalize=False)
    objs = [objects.Object() for _ in scene['footprints'][:5]]
    for o, fp in zip(objs, scene['footprints']):
        o.footprint = set(fp)
    objects.compute_objects(objs, yi, scene['atoms'], scene['dsm_cfg'], str(tmp_path / 'gen1'), out='muted')
    logs = sorted(os.listdir(tmp_path / 'gen1'))
    assert logs == [f'{i}.txt' for i in range(5)] and 'Newton iterations' in open(tmp_path / 'gen1' / '0.txt').read()
    with pytest.raises(NotImplementedError):
        objects.compute_objects(objs, yi, scene['atoms'], dict(scene['dsm_cfg'], sparsity_tol=1e-3), None, out='muted')
    # dsm/hessian_sparsity_tol only thins the Hessian the reference hands to cvxopt (dsm.py:377-383): same psi, same gradient, same optimum -- accepted, same results
    e0 = [o.energy for o in objs]
    objects.compute_objects(objs, yi, scene['atoms'], dict(scene['dsm_cfg'], hessian_sparsity_tol=1e-3), None, out='muted')
    assert [o.energy for o in objs] == e0
    # the device-image cache follows the content, not the address
    d0 = objects.device_image(yi, scene['atoms'], 8)
    assert objects.device_image(yi, scene['atoms'], 8) is d0
    atoms2 = scene['atoms'].copy()
    atoms2[atoms2 == 1] = 2
    assert objects.device_image(yi, atoms2, 8) is not d0


# ---------------------------------------------------------------------------------------------------------
# post-processing, per-object work (superdsm/postprocess.py:254-337)
# ---------------------------------------------------------------------------------------------------------
class _Frag:
    def __init__(self, off, frag):
        self.fg_offset, self.fg_fragment = np.asarray(off), np.asarray(frag, bool)

    def fill_foreground(self, out, value=True):
        h, w = self.fg_fragment.shape
        out[self.fg_offset[0]:self.fg_offset[0] + h, self.fg_offset[1]:self.fg_offset[1] + w] = value * self.fg_fragment


def test_postprocess_objects_match_reference_fixtures(gpu):
    """Contrast response and refined masks of sdsm_post_objects against the outputs of the reference's own _compute_contrast /
    _process_mask (tests/golden/postprocess.npz), for two parameter sets each."""
    from superdsm_amd import postprocess
    d = np.load(os.path.join(G, 'postprocess.npz'))
    g = d['g']
    bg = np.unpackbits(d['background_mask'])[:g.size].reshape(g.shape).astype(bool)
    objs = [_Frag(d[f'o{k}_offset'], d[f'o{k}_fragment']) for k in range(int(d['n']))]
    g_dev = gpu.as_tensor(g).cuda()
    gs = postprocess.gaussian_filter_gpu(g_dev, 3)
    import scipy.ndimage as ndi
    np.testing.assert_allclose(gs.cpu().numpy(), ndi.gaussian_filter(g, 3), rtol=0, atol=1e-15)
    for key, (scale, offset), tag, (dist, amp, fill) in (('contrast', (5, 5), 'a', (1, 2, True)), ('contrast_b', (3, 2), 'b', (2, 1.5, False))):
        recs, refined = postprocess.process_objects_gpu(objs, g_dev, gs, bg, scale, offset, 1e-4, dist, amp)
        for k in range(len(objs)):
            assert abs(recs['contrast'][k] - float(d[f'o{k}_{key}'])) <= 1e-10 * abs(float(d[f'o{k}_{key}'])), (key, k)
            off, frag = refined[k]
            if fill:
                frag = ndi.binary_fill_holes(frag)
            np.testing.assert_array_equal(off, d[f'o{k}_mask_{tag}_offset'])
            np.testing.assert_array_equal(frag, d[f'o{k}_mask_{tag}_fragment'].astype(bool))
            assert recs['area'][k] == objs[k].fg_fragment.sum()


def test_postprocess_stage_on_a_segmented_scene_matches_oracle(gpu):
    """The whole downstream chain on the BBBC039-like scene: global energy minimisation -> Postprocessing stage -> label map ->
    regression rows; the per-object numbers against the full-image CPU restatement (oracle/postprocess_oracle.py), incl. an
    object whose boundary list lives in global memory."""
    import scipy.ndimage as ndi
    from oracle import postprocess_oracle as po
    from superdsm_amd import config, globalenergymin, postprocess, render, testing
    scene = testing.make_scene('bbbc039_like', max_size=2)
    data = dict(g_raw=scene['g'], y=scene['y'], y_mask=np.ones(scene['y'].shape, bool), atoms=scene['atoms'], adjacencies=scene['adjacencies'], dsm_cfg=scene['dsm_cfg'])
    cfg = config.Config({'global-energy-minimization': {'beta': 150.0, 'pruning': 'isbi24'}, 'postprocess': {'min_contrast': 1.2}})
    globalenergymin.GlobalEnergyMinimization()(data, cfg, out='muted')
    stage = postprocess.Postprocessing()
    stage(data, cfg, out='muted')
    sol = list(data['cover'].solution)
    post = data['postprocessed_objects']
    assert 0 < len(post) <= len(sol)
    g = scene['g']
    bg = po.background_mask(g.shape, [(o.fg_offset, o.fg_fragment) for o in sol], 5)
    gs = ndi.gaussian_filter(g, 3)
    recs = stage.last_records
    kept = {id(p.original): p for p in post}
    for k, o in enumerate(sol):
        want = po.compute_contrast(o.fg_offset, o.fg_fragment, g, 5, 5, 1e-4, bg)
        assert abs(recs['contrast'][k] - want) <= 1e-9 * abs(want), k
        if id(o) in kept:
            off, frag = po.process_mask(o.fg_offset, o.fg_fragment, gs, 1, 2, True)
            np.testing.assert_array_equal(kept[id(o)].fg_offset, off)
            np.testing.assert_array_equal(kept[id(o)].fg_fragment, frag)
            assert abs(o.energy / o.cvxprog_region_size) <= 0.2 and want >= 1.2
    labels = render.rasterize_labels(data)
    rows = render.label_map_rows(labels)
    assert len(rows) == len(post) == labels.max()
    assert render.regression_agreement(rows, rows)['matched_fraction'] == 1.0
    # a very large object: boundary list in global memory
    rr, cc = np.mgrid[:520, :696]
    big = _Frag((40, 60), ((rr[40:440, 60:560] - 240) / 200.0) ** 2 + ((cc[40:440, 60:560] - 310) / 250.0) ** 2 <= 1)
    assert big.fg_fragment.sum() > 12288
    g_dev = gpu.as_tensor(g).cuda()
    bgb = po.background_mask(g.shape, [(big.fg_offset, big.fg_fragment)], 5)
    r2, f2 = postprocess.process_objects_gpu([big], g_dev, postprocess.gaussian_filter_gpu(g_dev, 3), bgb, 5, 5, 1e-4, 1, 2)
    want = po.compute_contrast(big.fg_offset, big.fg_fragment, g, 5, 5, 1e-4, bgb)
    assert abs(r2['contrast'][0] - want) <= 1e-9 * abs(want)
    off, frag = po.process_mask(big.fg_offset, big.fg_fragment, gs, 1, 2, False)
    np.testing.assert_array_equal(f2[0][0], off)
    np.testing.assert_array_equal(f2[0][1], frag)


# ---------------------------------------------------------------------------------------------------------
# scale estimation (superdsm/automation.py:41-68)
# ---------------------------------------------------------------------------------------------------------
def test_scale_estimation_masks_match_scipy_and_scale_follows_the_object_size(gpu):
    """The Laplacian-of-Gaussian masks of the scale estimation (GPU separable filters with SciPy's derivative-of-Gaussian
    weights, radii up to 566 taps) against scipy.ndimage.gaussian_laplace; the estimated scale grows with the size of the
    objects and create_config works without AF_scale.  (The blob detector itself is scikit-image arithmetic in the reference:
    restated, parity unpinned -- see superdsm_amd/automation.py.)"""
    import scipy.ndimage as ndi
    from superdsm_amd import automation, config
    from superdsm_amd.globalenergymin import GlobalEnergyMinimization
    rng = np.random.default_rng(0)
    H, W = 300, 380

    def scene(r):
        rr, cc = np.mgrid[:H, :W]
        im = 0.02 * rng.standard_normal((H, W))
        for _ in range(8):
            r0, c0 = rng.uniform(r, H - r), rng.uniform(r, W - r)
            im += np.exp(-(((rr - r0) ** 2 + (cc - c0) ** 2) / (r * r)) ** 2)
        return im

    im = automation.normalize_image(scene(25))
    sigmas = np.array([7.07, 14.14, 70.7, 141.4])
    masks = automation._log_negative_masks(im, sigmas)
    for s in sigmas:
        ref = ndi.gaussian_laplace(im, s)
        differ = masks[s] != (ref < 0)
        assert differ.mean() < 1e-4 and (np.abs(ref[differ]) < 1e-12 * np.abs(ref).max()).all(), s
    scales = [automation._estimate_scale(scene(r))[0] for r in (22, 45)]
    assert scales[0] < scales[1] and 10 < scales[0] < 50
    class _P:
        stages = [GlobalEnergyMinimization()]
    cfg, scale = automation.create_config(_P(), config.Config({}), scene(25))
    assert abs(cfg['global-energy-minimization/beta'] - 0.66 * scale ** 2) <= 1e-9 * scale ** 2


def test_regression_metric_gpu_pipeline_vs_cpu_oracle_pipeline(gpu):
    """The reference's end-to-end criterion (tests/regression/validate.py: the SET of (area, centre x, centre y) rows of the label
    map) between the GPU pipeline -- global energy minimisation, post-processing, label map -- and the same host logic driven by
    the CPU restatements (oracle solves, full-image post-processing arithmetic, SciPy's Gaussian) on the BBBC039-like scene.  The
    real expected CSVs need the BBBC039 images, which are not available offline; the reference's own two CI hosts disagree on
    0.14 % of the objects."""
    import unittest.mock as mock
    import scipy.ndimage as ndi
    from oracle import oracle, postprocess_oracle as po
    from superdsm_amd import _capi, config, globalenergymin, postprocess, render, testing
    scene = testing.make_scene('bbbc039_like', max_size=2)
    cfg = config.Config({'global-energy-minimization': {'beta': 150.0, 'pruning': 'isbi24'}, 'postprocess': {'min_contrast': 1.2}})
    mk = lambda: dict(g_raw=scene['g'], y=scene['y'], y_mask=np.ones(scene['y'].shape, bool), atoms=scene['atoms'], adjacencies=scene['adjacencies'], dsm_cfg=scene['dsm_cfg'])

    def run(data):
        globalenergymin.GlobalEnergyMinimization()(data, cfg, out='muted')
        postprocess.Postprocessing()(data, cfg, out='muted')
        return render.label_map_rows(render.rasterize_labels(data))

    rows_gpu = run(mk())

    def oracle_compute(objs, y, atoms, dsm_cfg, log_root_dir, status_line=None, out=None, shard=None):
        objs = list(objs)
        if not objs:
            return
        recs, frags, _ = oracle.compute_objects(y.model, None, atoms, [sorted(o.footprint) for o in objs], dsm_cfg, nthreads=0)
        for o, r, f in zip(objs, recs, frags):
            o.energy, o.is_optimal, o.on_boundary, o.processing_time = float(r['energy']), bool(r['is_optimal']), bool(r['on_boundary']), 0
            o.fg_offset, o.fg_fragment, o.cvxprog_region_size = np.array(r['fg_offset']), f, int(r['N'])

    def cpu_objects(images, scale, offset, eps, dist, amp, fill_holes):
        results = []
        for objects, g, gs, bg in images:           # g: the stage's device image, here a _Host around the host array
            recs = np.zeros(len(objects), _capi.POST_RECORD_DTYPE)
            masks = []
            for k, o in enumerate(objects):
                recs['contrast'][k] = po.compute_contrast(o.fg_offset, o.fg_fragment, g.a, scale, offset, eps, bg)
                masks.append(po.process_mask(o.fg_offset, o.fg_fragment, gs, dist, amp, fill_holes))
            results.append((recs, masks))
        return results

    class _Host:                                    # stands in for the device tensors of the stage: the CPU pipeline never touches the GPU
        def __init__(self, a):
            self.a = a
        def cuda(self):
            return self
    with mock.patch.object(globalenergymin, 'compute_objects', oracle_compute), \
         mock.patch.object(postprocess, '_process_objects', cpu_objects), \
         mock.patch.object(postprocess, 'gaussian_filter_gpu', lambda g, sigma: ndi.gaussian_filter(g.a, sigma)), \
         mock.patch('torch.as_tensor', lambda a, *k, **kw: _Host(a)):
        _Host.__array__ = lambda self, *a, **k: self.a
        data = mk()
        globalenergymin.GlobalEnergyMinimization()(data, cfg, out='muted')
        # the stage calls g_dev = torch.as_tensor(g).cuda(); with the patches above g_dev wraps the host array
        postprocess.Postprocessing()(data, cfg, out='muted')
        rows_cpu = render.label_map_rows(render.rasterize_labels(data))
    agree = render.regression_agreement(rows_gpu, rows_cpu)
    assert agree['expected'] > 50
    assert agree['matched_fraction'] >= 0.99 and agree['spurious'] <= max(1, agree['expected'] // 100), agree


def test_launches_reproduce_their_results_bit_for_bit(gpu):
    """The sums of a solve do not depend on the order in which lanes, wavefronts or workgroups add to them: everything that is summed
    over the pixels is an integer (fixed-point) sum -- gradient, Hessian, coordinate moments --, except psi, whose chunk totals (64 runs,
    a wavefront butterfly) are added in a fixed order.  So a launch repeated -- alone, with the candidates of a second copy of the
    image interleaved (which changes what runs beside what and how many workgroups share the very large regions), or in another
    scheduling mode (another workgroup size, other size classes, no workgroup groups at all) -- returns the same 128-byte records and
    the same masks."""
    from superdsm_amd import engine, testing
    for workload, stride in (('bbbc039_like', 1), ('gowt1_like', 1)):
        scene = testing.make_scene(workload, max_size=3 if workload == 'bbbc039_like' else 2)
        fps = scene['footprints'][::stride]
        cfg = scene['dsm_cfg']
        img = engine.DeviceImage(scene['y'], None, scene['atoms'], cfg['background_margin'])
        one = engine.Batch(img, fps, cfg)
        runs = []
        for _ in range(2):
            one.launch()
            rec, mask = one.download()
            runs.append((rec.copy(), np.array(mask, copy=True)))
        assert (runs[0][0]['status'] != 1).any()
        assert runs[0][0].tobytes() == runs[1][0].tobytes()
        assert (runs[0][1] == runs[1][1]).all()
        for mode in (1, 2):                                              # latency scheduling; no workgroup groups
            other = engine.Batch(img, fps, cfg, mode=mode)
            other.launch()
            orec, omask = other.download()
            assert orec.tobytes() == runs[0][0].tobytes(), (workload, mode, np.flatnonzero(orec['energy'] != runs[0][0]['energy'])[:5])
            assert (omask == runs[0][1]).all()
        img2 = engine.DeviceImage(scene['y'].copy(), None, scene['atoms'].copy(), cfg['background_margin'])
        both = engine.Batch([img, img2], [fp for fp in fps for _ in range(2)], cfg, image_of=[k for _ in fps for k in range(2)])
        both.launch()
        rec2, mask2 = both.download()
        fr1 = one.fragments(runs[0][0], masks=runs[0][1])
        fr2 = both.fragments(rec2, masks=mask2)
        for i in range(len(fps)):
            assert rec2[2 * i].tobytes() == rec2[2 * i + 1].tobytes(), (workload, i)          # the two copies inside one launch
            # also for the regions of more than 12 288 pixels, which are solved by a workgroup group while the launch has compute units
            # to spare (the doubled plan may give them fewer members or none): integer sums and the fixed order of the psi sums do not
            # depend on how many workgroups share a candidate
            assert rec2[2 * i].tobytes() == runs[0][0][i].tobytes(), (workload, i)
            for k in range(2):
                assert tuple(fr2[2 * i + k][0]) == tuple(fr1[i][0]) and np.array_equal(fr2[2 * i + k][1], fr1[i][1])


@pytest.mark.parametrize('factor', [2.0 ** -40, 2.0 ** -10, 8.0])
def test_intensity_scale_does_not_matter_for_the_fixed_point_sums(gpu, factor):
    """The solve kernel accumulates the scattered gradient / Hessian contributions as integers in units chosen per candidate from
    the exponent of max|y| (sdsm_k_setup: CandState.yexp).  psi = sum log(1 + exp(-y S)) only sees the products y S: an image
    scaled by a constant -- 16-bit raw intensities, or tiny ones -- has the same regions, and the same optima up to the scale of
    the parameters and to the regulariser (which does not scale): GPU and CPU oracle must agree on the scaled image as they do on
    the unscaled one.  (Scales of 64 and more -- raw 16-bit intensities -- are outside the solver's domain: the regulariser then
    hardly matters, the approximate Hessian of DESIGN.md section 4 converges slowly and oracle and GPU both stop at the iteration cap;
    the reference normalises images to [0, 1], pipeline.py:192.)"""
    from oracle import oracle
    from superdsm_amd import testing
    scene = testing.make_scene('synthetic256', max_size=2)
    scene = dict(scene, y=scene['y'] * factor)
    res = testing.solve_scene_gpu(scene)
    recs, frags = res['records'], res['fragments']
    orecs, ofrags, _ = oracle.compute_objects(scene['y'], None, scene['atoms'], scene['footprints'], scene['dsm_cfg'], nthreads=0)
    np.testing.assert_array_equal(recs['n_pixels'], orecs['N'])
    np.testing.assert_array_equal(recs['n_deform'], orecs['M'])
    for k in range(len(scene['footprints'])):
        assert recs['status'][k] == orecs['status'][k], (k, recs['status'][k], orecs['status'][k])
        tol = 1e-6 * orecs['N'][k] / 1000 + 1e-5 * abs(orecs['energy'][k])
        assert abs(recs['energy'][k] - orecs['energy'][k]) <= tol, (k, recs['energy'][k], orecs['energy'][k])
        assert testing.dice(frags[k][0], frags[k][1], orecs['fg_offset'][k], ofrags[k], scene['y'].shape) >= 0.999


def _launch_child(q, unset_queues, seconds, go):
    """Child process: launches of the GOWT1-like frame (every solve class and workgroup groups in one launch); `unset_queues`: without
    the GPU_MAX_HW_QUEUES default of the package (the environment is arranged before anything touches the GPU)."""
    import hashlib
    import os
    import time
    import traceback
    try:
        if unset_queues:
            os.environ.pop('GPU_MAX_HW_QUEUES', None)
            os.environ['SDSM_SET_HW_QUEUES'] = '0'
        import numpy as np
        import torch
        from superdsm_amd import _capi, testing
        scene = testing.make_scene('gowt1_like', max_size=3)
        res = testing.solve_scene_gpu(scene)
        batch = res['batch']
        if go is not None:
            go.wait(120)                                    # all children launch at the same time
        times, n_given_up, digests = [], 0, set()
        t_end = time.perf_counter() + seconds
        while time.perf_counter() < t_end or len(times) < 5:
            t1 = time.perf_counter()
            batch.launch()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t1) * 1e3)
            recs = batch.records()
            gu = recs['status'] == _capi.CAND_GIVEN_UP
            n_given_up += int(gu.sum())
            if not gu.any():
                digests.add(hashlib.sha1(np.ascontiguousarray(recs).tobytes()).hexdigest())
        q.put(('ok', sorted(digests), float(np.median(times)), float(np.max(times)), n_given_up, len(times), int(_capi.lib().sdsm_side_queues_distinct()),
               os.environ.get('GPU_MAX_HW_QUEUES')))
    except BaseException:                                   # noqa: BLE001 -- reported to the parent
        q.put(('error', traceback.format_exc()))


def test_launch_order_does_not_rest_on_the_environment_or_on_having_the_card_alone(gpu):
    """VERDICT r03 #7.  (a) A fresh process WITHOUT the package's GPU_MAX_HW_QUEUES default: the same bytes, and not much slower (the gate of
    class 1 observes residency, it does not assume a queue layout).  (b) Three processes launching on the one card at the same time (the
    deployment DESIGN section 6 recommends for the stage): the same bytes whenever no group was given up, and no launch stalls for long --
    a group whose members do not become resident together is given up after 50 ms and solved again by the caller, not after 10 s."""
    import hashlib
    import multiprocessing as mp
    import time
    from superdsm_amd import _capi, testing
    scene = testing.make_scene('gowt1_like', max_size=3)
    res = testing.solve_scene_gpu(scene)
    batch = res['batch']
    recs = res['records']
    assert (recs['status'] == _capi.CAND_OPTIMAL).all()
    assert _capi.lib().sdsm_side_queues_distinct() == 1, 'the test process itself imports superdsm_amd first: its streams must run side by side'
    digest = hashlib.sha1(np.ascontiguousarray(recs).tobytes()).hexdigest()
    times = []
    for _ in range(10):
        t1 = time.perf_counter()
        batch.launch()
        gpu.cuda.synchronize()
        times.append((time.perf_counter() - t1) * 1e3)
    t_here = float(np.median(times))
    ctx = mp.get_context('spawn')
    # (a)
    q = ctx.Queue()
    p = ctx.Process(target=_launch_child, args=(q, True, 0.5, None))
    p.start()
    out = q.get(timeout=300)
    p.join(60)
    assert out[0] == 'ok', out[1]
    _, digests, t_med, t_max, n_gu, n_launch, distinct, env = out
    assert env is None and digests == [digest] and n_gu == 0
    assert t_med <= 1.3 * t_here + 0.5, (t_med, t_here, distinct)
    # (b)
    q = ctx.Queue()
    go = ctx.Barrier(3)
    ps = [ctx.Process(target=_launch_child, args=(q, False, 1.0, go)) for _ in range(3)]
    for p in ps:
        p.start()
    outs = [q.get(timeout=300) for _ in ps]
    for p in ps:
        p.join(60)
    for out in outs:
        assert out[0] == 'ok', out[1]
        _, digests, t_med, t_max, n_gu, n_launch, distinct, env = out
        assert digests in ([digest], []), 'a launch that shares the card gives the same records'
        assert t_max <= 100.0 + 3 * 1.3 * t_here * 3, (t_max, t_here)          # three processes share the card; a given-up group costs 50 ms once, not 10 s
        assert n_launch >= 5
