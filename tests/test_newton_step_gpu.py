"""A second full evaluation at an unchanged iterate (stop test repeated with the true curvature, larger diagonal shift after a failed
pivot) takes the pixel sums the first one kept instead of a second pass over the pixels, and leaves every result bit for bit as it
is.  It can be switched off per process (sdsm_set_solver_diagnostics) and counts its events
(sdsm_batch_solver_counters).
Scene: synthetic256 (the smoke test's: 42 candidates, N <= 10 454, M ~ 10 .. 162 -- class 1, class 1b and the 512-thread classes, in
latency mode a workgroup group); the oracle makes 41 such second evaluations on it."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RECOMPUTE = 1
ERR_ARGUMENT = -1                                    # SDSM_ERR_ARGUMENT (include/sdsm.h)


@functools.lru_cache(maxsize=None)
def _scene():
    from superdsm_amd import testing
    return testing.make_scene('synthetic256')


@functools.lru_cache(maxsize=None)
def _solve(mode, flags):
    """(records, xi, packed masks) as bytes and the event counters of one launch of the scene under the given diagnostics."""
    import torch
    from superdsm_amd import _capi, engine
    scene = _scene()
    L = _capi.lib()
    _capi.check(L.sdsm_set_solver_diagnostics(flags), 'sdsm_set_solver_diagnostics')
    try:
        img = engine.DeviceImage(scene['y'], None, scene['atoms'], scene['dsm_cfg']['background_margin'])
        batch = engine.Batch(img, scene['footprints'], scene['dsm_cfg'], want_xi=True, mode=mode)
        batch.launch()
        torch.cuda.synchronize()
        recs = batch.records()
        out = (recs.tobytes(), batch.xi_dev.cpu().numpy().tobytes(), batch.masks_dev.cpu().numpy().tobytes())
        with_m = recs['n_deform'] > 0
        return out, batch.solver_counters(), int(recs['evals_full'][with_m].sum()), int(with_m.sum())
    finally:
        _capi.check(L.sdsm_set_solver_diagnostics(0), 'sdsm_set_solver_diagnostics')


def test_reused_sums_equal_a_second_pass():
    reused = []
    for mode in (0, 1, 2):
        out, cnt, evals, ncand = _solve(mode, 0)
        out_r, cnt_r, evals_r, _ = _solve(mode, RECOMPUTE)
        print(f'mode {mode}: {cnt["evals_reused"]} of {evals} full evaluations of {ncand} candidates with M > 0 served from kept sums '
              f'({100.0 * cnt["evals_reused"] / evals:.2f} %); with recomputation {cnt_r["evals_reused"]}')
        for a, b, what in zip(out, out_r, ('records', 'xi', 'masks')):
            assert a == b, f'mode {mode}: {what} differ between kept sums and a second pass'
        assert evals == evals_r                      # evals_full counts evaluations, served or computed
        assert cnt_r['evals_reused'] == 0, (mode, cnt_r)
        reused.append(cnt['evals_reused'])
        # a third of the 42 candidates: the oracle makes 41 such evaluations here; the slack is for envelopes that do not fit twice
        # and for second evaluations at another fixed-point scale
        assert cnt['evals_reused'] >= 14, (mode, cnt)


def test_entry_points():
    import torch
    from superdsm_amd import _capi, engine
    L = _capi.lib()
    try:
        for bad in (2, 4, 1 << 30, -1):
            assert L.sdsm_set_solver_diagnostics(bad) == ERR_ARGUMENT, bad
        for good in (1, 0):
            assert L.sdsm_set_solver_diagnostics(good) == _capi.SDSM_OK, good
    finally:
        L.sdsm_set_solver_diagnostics(0)
    scene = _scene()
    img = engine.DeviceImage(scene['y'], None, scene['atoms'], scene['dsm_cfg']['background_margin'])
    batch = engine.Batch(img, scene['footprints'][:4], scene['dsm_cfg'])
    torch.cuda.synchronize()
    assert batch.solver_counters() == dict(evals_reused=0)      # before any launch
    out = np.zeros(4, np.int64)
    assert L.sdsm_batch_solver_counters(None, None, out.ctypes.data_as(C.c_void_p)) == ERR_ARGUMENT


# =========================================================================================================
# One Newton step of the solve kernels, piece by piece (sdsm_batch_eval_step: eval_full, factor_solve and eval_line called as they stand,
# in the LDS layout of every solve class) against np.longdouble references (superdsm_amd/testing.py: hessian_reference, step_residual;
# tests/test_newton_step_cpu.py checks those against the oracle and a float64 Cholesky solve).
#
# Scenes: the 80 x 96 blob of tests/test_loss_arithmetic_gpu.py (one atom, one candidate) under settings that put it into every class;
# the figures are asserted from inspect_states():
#   scene     margin  subsample  amount     N     M    n   envelope  hzmax   class   layouts that hold it            back substitution
#   m47          8        8        4      3043    47   53     1055      6     1      all six in LDS                  wave<1> (n <= 64; n mod 4 = 1)
#   m86          8        6        2      3043    86   92     1674      4     1      all six in LDS                  wave<2> in the class-1 layouts, wave<4> elsewhere (n mod 4 = 0)
#   m123         8        5        4      3043   123  129     5093     13     1b     1b, 2, 2b, light                wave<4> (128 < n <= 256)
#   m252         4        3        2      2266   252  258    11051     12     2b     2b, light                       wave<8> in 2b, wave<5> in light (256 < n <= 288)
#   m342         8        3        1      3043   342  348    10014      5     2      2, 2b                           wave<8> (256 < n <= 512, 512 threads)
#   class 3      8        3       1.5     3043   342  348    16302      8     3      3 (Hessian in global memory)    wave<8>; two points only
#   ell          8        -       inf     3043     0    6       21      0     1      all six in LDS                  the 6 x 6 solve in registers
# hzmax <= 8 (m47, m86, m342, class 3): the leading entries of a run in registers; hzmax > 8 (m123, m252): read from memory.  The blocked
# back substitution needs more than 512 unknowns (a region of tens of thousands of pixels): not reached here.
# Points: the constant term alone (c = 0, +-1), the kernel's own optimum, the optimum perturbed with xi scaled by 1e-3, 1 and 1e3; for
# M > 0 also c = 800 / min|y| (every curvature weight is exactly 0).
# Every bound is derived next to its use from the operation counts of the kernel, none is fitted; every test prints its worst
# error / bound per scene (and layout).
# =========================================================================================================
STEP_LIMITS = {'class 1': (128, 2560), 'class 1 latency': (128, 2560), 'class 1b': (256, 7168), 'class 2': (1024, 11000), 'class 2b': (512, 15170),
               'light': (288, 12400)}                      # 6 + M and envelope doubles a layout holds (sdsm_common.h); class 3: the candidates the plan gave a slot in global memory
STEP_SCENES = {
    'm47': dict(margin=8, kw=dict(smooth_subsample=8), figures=(3043, 47, 1055, 6), cls='class 1'),
    'm86': dict(margin=8, kw=dict(smooth_subsample=6, smooth_amount=2), figures=(3043, 86, 1674, 4), cls='class 1'),
    'm123': dict(margin=8, kw=dict(smooth_subsample=5), figures=(3043, 123, 5093, 13), cls='class 1b'),
    'm252': dict(margin=4, kw=dict(smooth_subsample=3, smooth_amount=2), figures=(2266, 252, 11051, 12), cls='class 2b'),
    'm342': dict(margin=8, kw=dict(smooth_subsample=3, smooth_amount=1), figures=(3043, 342, 10014, 5), cls='class 2'),
    'class 3': dict(margin=8, kw=dict(smooth_subsample=3, smooth_amount=1.5), figures=(3043, 342, 16302, 8), cls='class 3'),
    'ell': dict(margin=8, kw=dict(smooth_amount=np.inf), figures=(3043, 0, 21, 0), cls='class 1'),
}
STEP_TAUS = ((0.0, 1.0), (1e-12, 0.5), (1e-4, 4.0))        # (tau, t0 of the sweep along the Newton direction of that launch)
STEP_T0 = (1.0, 0.5, 4.0, 2.0 ** -36)
ZERO_CURVATURE = 'c = 800 / min|y|'


def _step_layouts(name):
    N, M, env, _ = STEP_SCENES[name]['figures']
    if STEP_SCENES[name]['cls'] == 'class 3':
        return ['class 3']
    return [lay for lay, (nmax, emax) in STEP_LIMITS.items() if 6 + M <= nmax and env <= emax]


def _step_points(name, opt, ymin):
    M = STEP_SCENES[name]['figures'][1]
    rng = np.random.default_rng(3)
    points = {}
    for c in (0.0, 1.0, -1.0):
        p = np.zeros(6 + M)
        p[5] = c
        points[f'c = {c:g}'] = p
    points['optimum'] = opt.copy()
    for scale in (1e-3, 1.0, 1e3):
        p = opt.copy()
        p[:6] *= 1 + 0.01 * rng.standard_normal(6)
        if M:
            p[6:] = scale * (p[6:] + np.abs(p[6:]).mean() * rng.standard_normal(M))
        points[f'perturbed, xi x {scale:g}'] = p
    if name == 'class 3':
        points = {k: points[k] for k in ('c = 0', 'optimum')}
    elif M:
        p = np.zeros(6 + M)
        p[5] = 800 / ymin
        points[ZERO_CURVATURE] = p
    return points


def _given_direction(opt, M):
    """A caller's direction with large xi components (theta part in the full-image-normalised frame, as the parameters)."""
    rng = np.random.default_rng(17)
    return np.concatenate([0.05 * np.abs(opt[:6]) * rng.standard_normal(6), 50.0 * rng.standard_normal(M)])


def collect_steps(scenes=None):
    """Every launch of the step probe these tests look at: per scene ONE solve (the workspace, the kernel's optimum), the setup's
    leading flags, and per point the probe in every layout that holds the candidate.  A record's envelope is dropped where it has the
    bytes of the first record of its (point, mu) -- ``env_same`` says so."""
    import torch
    from superdsm_amd import engine, testing as T
    from test_loss_arithmetic_gpu import _blob_scene
    y, atoms = _blob_scene()
    ymin = float(np.abs(y).min())
    images, out = {}, {}
    for name in (scenes or STEP_SCENES):
        sc = STEP_SCENES[name]
        if sc['margin'] not in images:
            images[sc['margin']] = engine.DeviceImage(y, None, atoms, sc['margin'])
        cfg = T._toy_cfg(background_margin=sc['margin'], **sc['kw'])
        batch = engine.Batch(images[sc['margin']], [[1]], cfg, want_xi=True)
        batch.launch()
        torch.cuda.synchronize()
        rec, st = batch.records()[0], batch.inspect_states()[0]
        M = int(rec['n_deform'])
        ins = batch.inspect()[0]
        opt = np.concatenate([rec['theta'], batch.xi_dev.cpu().numpy()[:M]])
        info = dict(N=int(rec['n_pixels']), M=M, env_size=st['env_size'] if M else 21, hzmax=st['hzmax'] if M else 0, box=np.array(batch.mask_info[0]), opt=opt,
                    status=int(rec['status']), setup={k: ins[k] for k in ('idx', 'w', 'lead', 'nnz', 'hnz', 'r', 'c', 'run_hnz', 'hzmax')})
        layouts, recs, base = _step_layouts(name), [], {}
        given = _given_direction(opt, M)

        def probe(point, p, layout, kind, mu=0.0, tau=0.0, t0=1.0):
            d = {'newton': None, 'given': [given], 'zero': [np.zeros(6 + M)]}[kind]
            res = batch.evaluate_step(layout, [p], direction=d, reg_mu=mu, tau=tau, t0=t0, dense=False)[0]
            if res['rc'] >= 0:
                first = base.setdefault((point, mu), res['env'])
                res['env_same'] = first is not res['env'] and first.tobytes() == res['env'].tobytes()
                if res['env_same']:
                    res['env'] = None
            recs.append(dict(point=point, layout=layout, kind=kind, mu=mu, tau=tau, t0=t0, res=res))

        points = _step_points(name, opt, ymin)
        psi_value = {}
        for point, p in points.items():
            psi_value[point] = batch.evaluate([p])[0]['psi_value']
            if point == ZERO_CURVATURE:
                for layout in layouts:
                    for tau in (0.0, 1e-4):
                        probe(point, p, layout, 'newton', tau=tau)
                continue
            for layout in layouts:
                for tau, t0 in STEP_TAUS:
                    probe(point, p, layout, 'newton', tau=tau, t0=t0)
                probe(point, p, layout, 'zero')
            probe(point, p, layouts[0], 'newton', mu=0.25, t0=2.0 ** -36)
            probe(point, p, layouts[0], 'newton', mu=1.0)
            for t0 in STEP_T0:
                probe(point, p, layouts[0], 'given', t0=t0)
        for layout in list(STEP_LIMITS) + ['class 3']:                     # the layouts that do not hold the candidate
            if layout not in layouts:
                probe('optimum', points['optimum'], layout, 'newton')
        torch.cuda.synchronize()
        out[name] = dict(info, cfg=cfg, layouts=layouts, points=points, given=given, psi_value=psi_value, recs=recs)
    return dict(y=y, atoms=atoms, scenes=out)


@pytest.fixture(scope='module')
def steps():
    import torch
    from superdsm_amd import _capi, testing as T
    assert torch.cuda.is_available(), 'these tests need a GPU'
    if not T.longdouble_is_extended():
        pytest.skip('np.longdouble has fewer than 64 significand bits here: no extended-precision reference')
    _capi.lib()
    return collect_steps()


def _recs(sc, **want):
    return [r for r in sc['recs'] if r['res']['rc'] >= 0 and all(r[k] == v for k, v in want.items())]


def _env_of(sc, r):
    """The record's envelope (its own, or that of the first record of its point and mu)."""
    if r['res']['env'] is not None:
        return r['res']['env']
    return next(q['res']['env'] for q in sc['recs'] if q['res']['rc'] >= 0 and q['point'] == r['point'] and q['mu'] == r['mu'] and q['res']['env'] is not None)


_REF = {}


def _reference(steps, name, point, mu):
    """hessian_reference and the bounds of tests/test_loss_arithmetic_gpu.py at one point of a scene, computed once."""
    from superdsm_amd import testing as T
    import test_loss_arithmetic_gpu as LA
    key = (name, point, mu)
    if key not in _REF:
        sc = steps['scenes'][name]
        p, M = sc['points'][point], sc['M']
        ref = T.hessian_reference(steps['y'], None, steps['atoms'], [1], sc['cfg'], p[:6], p[6:] if M else None, box=sc['box'], reg_mu=mu)
        ref['alpha'] = float(sc['cfg']['alpha'])
        assert ref['M'] == M and ref['N'] == sc['N']
        _REF[key] = (ref, LA._eval_bounds(ref))
    return _REF[key]


def _worst(got, want, bound):
    """max |got - want| / bound over the entries (0 where they are equal); got must be finite."""
    X = np.longdouble
    got, want, bound = np.asarray(got, X), np.asarray(want, X), np.asarray(bound, X)
    assert np.isfinite(got.astype(np.float64)).all()
    with np.errstate(all='ignore'):
        ratio = np.where(got == want, X(0), np.abs(got - want) / bound)
    assert not np.isnan(ratio).any()
    return float(ratio.max()) if ratio.size else 0.0


def test_step_scenes_are_what_the_table_says(steps):
    """N, M, envelope and hzmax of every scene, its class, both Hessian paths, and rc = -1 (with nothing else) from every layout that
    does not hold the candidate."""
    for name, sc in steps['scenes'].items():
        assert (sc['N'], sc['M'], sc['env_size'], sc['hzmax']) == STEP_SCENES[name]['figures'], (name, sc['N'], sc['M'], sc['env_size'], sc['hzmax'])
        assert sc['status'] == 0 and sc['layouts'][0] == STEP_SCENES[name]['cls']              # optimal; the first layout that holds it is its class
        other = [r for r in sc['recs'] if r['layout'] not in sc['layouts']]
        assert len(other) == 7 - len(sc['layouts'])
        for r in other:
            if r['layout'] != 'class 3':
                assert r['res'] == dict(rc=-1), (name, r['layout'])
            print(f'{name}: layout {r["layout"]}: rc {r["res"]["rc"]}')
        assert all(r['res']['rc'] >= 0 for r in sc['recs'] if r['layout'] in sc['layouts'])
    hz = {name: sc['hzmax'] for name, sc in steps['scenes'].items() if sc['M']}
    assert min(hz.values()) <= 8 < max(hz.values()), hz
    n = {name: 6 + sc['M'] for name, sc in steps['scenes'].items()}
    assert n['m47'] % 4 and n['m47'] <= 64 and n['m86'] % 4 == 0 and 64 < n['m86'] <= 128 < n['m123'] <= 256 < n['m252'] <= 288 < n['m342'] <= 512


def test_leading_flags_equal_the_oracle_rule(steps):
    """(a) Which entries of every pixel's row of G~ are leading ones: bits 16 .. 19 of ell_im against the oracle's float32 rule, exactly
    (both compare the same float32 weights: test_setup_matches_oracle_exactly holds G~ bit for bit); hzmax = the largest per-run count."""
    from oracle import oracle
    from superdsm_amd import testing as T
    for name, sc in steps['scenes'].items():
        if sc['M'] == 0:
            continue
        cfg, su = sc['cfg'], sc['setup']
        region = oracle.region_mask(steps['y'], None, steps['atoms'], [1], cfg['background_margin'])
        rr, cc = np.nonzero(region)
        sm = oracle.smooth_matrix(region, cfg['smooth_amount'], cfg['gaussian_shape_multiplier'], cfg['smooth_subsample'])
        assert np.array_equal(su['r'], rr) and np.array_equal(su['c'], cc) and np.array_equal(su['nnz'], np.diff(sm.indptr))
        row = np.repeat(np.arange(rr.size), np.diff(sm.indptr))
        o = np.lexsort((sm.indices, row))                                  # the rows by column index, as inspect() reports them
        lead = T.leading_entries(sm.indptr, sm.data)
        have = (np.arange(su['idx'].shape[0])[:, None] < su['nnz'][None, :]).T
        assert np.array_equal(su['idx'].T[have], sm.indices[o]) and np.array_equal(su['w'].T[have], sm.data[o].astype(np.float32))
        assert np.array_equal(su['lead'].T[have], lead[o]), name
        assert not su['lead'].T[~have].any() and np.array_equal(su['hnz'], np.add.reduceat(lead.astype(np.int64), sm.indptr[:-1]))
        env = T.envelope_reference(rr, cc, sm.M, sm.indptr, sm.indices, lead)
        assert np.array_equal(np.sort(su['run_hnz']), np.sort(env['run_hz'])), name
        assert su['hzmax'] == sc['hzmax'] == int(su['run_hnz'].max()) == env['hzmax'], name
        print(f'{name}: {int(lead.sum())} of {lead.size} entries are leading ones; per run at most {env["hzmax"]}')


def test_envelope_structure(steps):
    """(b) rb, fst and rend as exported: fst a multiple of the panel width and non-decreasing, the rows tile the envelope without
    overlap, rend what the binary search defines -- all three equal to the envelope the oracle's leading entries define -- and every
    non-zero entry of the reference lies inside the envelope."""
    from oracle import oracle
    from superdsm_amd import engine, testing as T
    for name, sc in steps['scenes'].items():
        M, n = sc['M'], 6 + sc['M']
        recs = _recs(sc)
        rb, fst, rend = recs[0]['res']['rb'], recs[0]['res']['fst'], recs[0]['res']['rend']
        for r in recs:
            assert np.array_equal(r['res']['rb'], rb) and np.array_equal(r['res']['fst'], fst) and np.array_equal(r['res']['rend'], rend), (name, r['layout'])
        if M == 0:
            assert rb.tolist() == [0, 1, 3, 6, 10, 15] and not fst.any() and rend.size == 0
            continue
        assert (fst[:M] % T.PANEL == 0).all() and (np.diff(fst[:M]) >= 0).all() and (fst[:M] <= np.arange(M)).all() and not fst[M:].any()
        lo, hi = rb + fst, rb + np.arange(n)
        assert lo[0] == 0 and (lo[1:] == hi[:-1] + 1).all() and hi[-1] + 1 == sc['env_size']
        assert rend.size == (M + T.PANEL - 1) // T.PANEL
        for p, re in enumerate(rend):
            assert fst[re] <= T.PANEL * p and (re == M - 1 or fst[re + 1] > T.PANEL * p), (name, p)
        cfg = sc['cfg']
        region = oracle.region_mask(steps['y'], None, steps['atoms'], [1], cfg['background_margin'])
        rr, cc = np.nonzero(region)
        sm = oracle.smooth_matrix(region, cfg['smooth_amount'], cfg['gaussian_shape_multiplier'], cfg['smooth_subsample'])
        env = T.envelope_reference(rr, cc, M, sm.indptr, sm.indices, T.leading_entries(sm.indptr, sm.data))
        assert np.array_equal(fst, env['fst']) and np.array_equal(rb, env['rb']) and np.array_equal(rend, env['rend']) and env['env_size'] == sc['env_size'], name
        stored = engine.expand_envelope(np.zeros(sc['env_size']), rb, fst)[1]
        ref = _reference(steps, name, 'optimum', 0.0)[0]
        assert stored[ref['hess'] != 0].all(), name
        print(f'{name}: envelope of {sc["env_size"]} doubles, {int((ref["hess"] != 0).sum())} of its {int(stored.sum())} entries (both triangles) coupled by a pixel')


def _entry_bounds(ref, bd, mu):
    """Bounds on the exported gradient and Hessian in the local frame, in the notation of tests/test_loss_arithmetic_gpu.py (H = 2^-53;
    dr, dd: the moved residual and curvature weight of a pixel; unit_g, unit_h: the fixed-point quanta).  J_i = (q(u_i, v_i), the leading
    weights of pixel i), an entry is sum_i d_i J_ia J_ib.
      xi-xi:     fl(d w_a) rounds once, the products with w_b are exact inside the multiply-adds onto the fixed-point constant, each of
                 which rounds to the quantum -- half a quantum per PIXEL that couples a and b (an absent product adds an exact 0) --, the
                 conversion of the integer sum rounds once: sum_i w_a w_b (dd_i + 2 H d_i) + (pixels coupling a, b) unit_h / 2.
      theta-xi:  theta_rows: fl(d w) 1; v carries 2 roundings, v^2 5; a term of m2 = sum d w v^2 1 + 5 + 1 = 7 and 3 additions: 10; u^2 5
                 (the product with it is exact inside the multiply-add); the conversion 1: 16 H; ONE multiply-add per run and row: half a
                 quantum per run, and a run has at least one pixel that holds the entry: sum_i |q_k| w_a (dd_i + 16 H d_i) + (pixels) unit_h / 2.
      theta-theta, theta gradient: the moments, as _eval_bounds counts them (26 + 3 and 14 + 3 roundings, two-word fixed point), without
                 the change of frame: sum_i |q_k q_l| (dd_i + 29 H d_i) + N unit_h 2^-49; F_k (sum dr + 17 H sum |r| + N unit_g 2^-49).
      xi gradient: frame independent: _eval_bounds' bound.
      regulariser on the xi diagonal (add_regulariser): t2 = sqrt(xi^2 + eps) carries (1 + 1) / 2 + 2 = 3 H (a square root within one ulp),
                 1 / t2 5 H (a division within one ulp), t2^3 11 H, xi^2 / t2^3 14 H; their difference, the product with alpha: at most
                 (5 + 14 + 1 + 1) H alpha / t2 = 21 H alpha / t2 (both terms are <= 1 / t2); the blend gd + mu (alpha / t2 - gd): alpha / t2
                 5 H, the difference 21 + 1, the product and the sum 2: (22 + 28 mu) H alpha / t2 in all; the addition to the entry: H of it."""
    from superdsm_amd import testing as T
    import test_loss_arithmetic_gpu as LA
    X, H = np.longdouble, LA.H
    N, M, n = ref['N'], ref['M'], 6 + ref['M']
    qa = np.abs(ref['q_local'])
    G_dd, G_d = T.lead_gram(qa, bd['dd'], ref['smat'], ref['lead'], M), T.lead_gram(qa, ref['d'], ref['smat'], ref['lead'], M)
    c = np.full((n, n), 2.0)
    c[:6, :] = c[:, :6] = 16.0
    c[:6, :6] = 29.0
    if M:
        ones = (ref['smat'][0], ref['smat'][1], np.ones(ref['smat'][2].size))
        pixels = T.lead_gram(np.ones((6, N)), np.ones(N), ones, ref['lead'], M)
    else:
        pixels = np.full((n, n), X(N))
    quanta = pixels * bd['unit_h'] / 2
    quanta[:6, :6] = N * bd['unit_h'] * X(2) ** -49
    b_hess = G_dd + c * H * G_d + quanta
    if M:
        j = 6 + np.arange(M)
        b_hess[j, j] += (22 + 28 * mu) * H * ref['reg_major'] + H * np.abs(ref['hess'][j, j])
    yabs = np.abs(ref['y']).astype(X)
    b_grad = np.concatenate([LA.F6 * (bd['dr'].sum() + 17 * H * (yabs * ref['theta_hat']).sum() + N * bd['unit_g'] * X(2) ** -49), bd['grad'][6:]])
    return b_grad * LA.SECOND_ORDER, b_hess * LA.SECOND_ORDER, pixels


def test_entries_within_derived_bounds(steps):
    """(c) psi (both evaluators), the gradient and EVERY entry of the exported envelope against hessian_reference, for mu = 0, 0.25, 1;
    entries inside the envelope that no pixel couples are exactly 0."""
    from superdsm_amd import engine
    for name, sc in steps['scenes'].items():
        worst = {}
        for point in sc['points']:
            for mu in (0.0, 0.25, 1.0):
                recs = _recs(sc, point=point, mu=mu, tau=0.0, kind='newton')
                if point == ZERO_CURVATURE and mu:
                    continue
                assert recs, (name, point, mu)
                r = recs[0]['res']
                ref, bd = _reference(steps, name, point, mu)
                b_grad, b_hess, pixels = _entry_bounds(ref, bd, mu)
                hess, stored = engine.expand_envelope(_env_of(sc, recs[0]), r['rb'], r['fst'])
                assert (ref['hess'][~stored] == 0).all()
                uncoupled = stored & (pixels == 0) & ~np.eye(6 + sc['M'], dtype=bool)
                assert (hess[uncoupled] == 0).all(), (name, point, mu)
                if point == ZERO_CURVATURE:
                    assert (hess[:6, :] == 0).all() and (hess[6:, 6:][~np.eye(sc['M'], dtype=bool)] == 0).all()      # (f): every d_i = 0
                res = {'psi': _worst(r['psi'], ref['psi'], bd['psi']), 'psi_value': _worst(r['psi_value'], ref['psi'], bd['psi']),
                       'grad theta': _worst(r['grad'][:6], ref['grad_local'][:6], b_grad[:6]), 'grad xi': _worst(r['grad'][6:], ref['grad_local'][6:], b_grad[6:]),
                       'hess theta-theta': _worst(hess[:6, :6], ref['hess'][:6, :6], b_hess[:6, :6]), 'hess theta-xi': _worst(hess[:6, 6:], ref['hess'][:6, 6:], b_hess[:6, 6:])}
                if sc['M']:
                    dg = np.eye(sc['M'], dtype=bool)
                    res['hess xi-xi'] = _worst(hess[6:, 6:][~dg], ref['hess'][6:, 6:][~dg], b_hess[6:, 6:][~dg])
                    res['hess xi diagonal'] = _worst(hess[6:, 6:][dg], ref['hess'][6:, 6:][dg], b_hess[6:, 6:][dg])
                print(f'{name}, {point}, mu = {mu:g}: ' + ', '.join(f'{k} {v:.3f}' for k, v in res.items()))
                for k, v in res.items():
                    worst[k] = max(worst.get(k, 0.0), v)
        print(f'{name}: worst error / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
        assert max(worst.values()) <= 1, (name, worst)


def test_same_bytes_in_every_layout(steps):
    """(d) The fixed-point sums do not depend on the launch: psi, the gradient and the envelope are the same bytes in
    every layout that holds the candidate (and for every tau and t0: the evaluation does not see them); the direction and lam2 are the
    same bytes in the two class-1 layouts (mode 0 = mode 1).  Other pairs of layouts: printed."""
    for name, sc in steps['scenes'].items():
        agree = {}
        for point in sc['points']:
            recs = _recs(sc, point=point, mu=0.0)
            first = recs[0]['res']
            for r in recs[1:]:
                q = r['res']
                assert q['env_same'] and q['grad'].tobytes() == first['grad'].tobytes() and q['psi'] == first['psi'] and q['psi_value'] == first['psi_value'], (name, point, r['layout'])
            for tau, _ in STEP_TAUS:
                by = {r['layout']: r['res'] for r in recs if r['kind'] == 'newton' and r['tau'] == tau}
                for a in by:
                    for b in by:
                        if a < b and by[a]['rc'] == 0 and by[b]['rc'] == 0:
                            same = by[a]['dir'].tobytes() == by[b]['dir'].tobytes() and by[a]['lam2'] == by[b]['lam2']
                            agree[(a, b)] = agree.get((a, b), True) and same
                            if {a, b} == {'class 1', 'class 1 latency'}:
                                assert same, (name, point, tau)
        differ = [f'{a} / {b}' for (a, b), same in sorted(agree.items()) if not same]
        print(f'{name}: direction and lam2 are the same bytes at every point in {len(agree) - len(differ)} of {len(agree)} pairs of layouts' + (': not in ' + ', '.join(differ) if differ else ''))
        assert name not in ('m47', 'm86', 'ell') or ('class 1', 'class 1 latency') in agree


def test_newton_step_backward_error(steps):
    """(e) (H + tau diag H) d + g and lam2 + g.d from the exported float64 H, g, d, within the bounds of testing.step_residual (gamma is
    derived there), for tau = 0, 1e-12, 1e-4 in every layout and for mu = 0.25, 1 in the candidate's own, wherever the factorisation
    succeeded -- and it must succeed wherever the Jacobi-scaled exported matrix has no eigenvalue below 1e-6 (roundings move an
    eigenvalue of that matrix by about n 2^-53).  (f) At c = 800 / min|y| the theta block is exactly zero: return code 1 for both tau."""
    from superdsm_amd import engine, testing as T
    X = np.longdouble
    for name, sc in steps['scenes'].items():
        worst, solved, definite = {}, 0, {}
        for r in _recs(sc, kind='newton'):
            q = r['res']
            if r['point'] == ZERO_CURVATURE:
                assert q['rc'] == 1 and np.isnan(q['lam2']) and np.isnan(q['dir']).all(), (name, r['layout'], r['tau'])
                continue
            hess = engine.expand_envelope(_env_of(sc, r), q['rb'], q['fst'])[0]
            key = (r['point'], r['mu'])
            if key not in definite:
                s = 1 / np.sqrt(np.maximum(np.diag(hess), 1e-300))
                definite[key] = float(np.linalg.eigvalsh(hess * np.outer(s, s)).min()) >= 1e-6 and (np.diag(hess) > 0).all()
            if definite[key]:
                assert q['rc'] == 0, (name, r['point'], r['layout'], r['tau'])
            if q['rc'] != 0:
                assert q['rc'] in (1, 2) and np.isnan(q['lam2']) and np.isnan(q['dir']).all()
                continue
            assert np.isfinite(q['dir']).all() and q['lam2'] >= 0
            res = T.step_residual(hess, q['grad'], q['dir'], r['tau'])
            lam = float(abs(X(q['lam2']) - res['lam2']) / res['lam2_bound']) if res['lam2_bound'] > 0 else float(X(q['lam2']) != res['lam2'])
            w = worst.setdefault(r['layout'], [0.0, 0.0])
            w[0], w[1] = max(w[0], res['ratio']), max(w[1], lam)
            solved += 1
        for layout, (a, b) in worst.items():
            print(f'{name}, {layout}: residual / bound {a:.4f}, |lam2 + g.d| / bound {b:.4f}')
        npoints = len(sc['points']) - (ZERO_CURVATURE in sc['points'])
        assert sum(definite[(p, 0.0)] for p in ('c = 0', 'c = 1', 'c = -1', 'optimum') if p in sc['points']) >= (2 if name == 'class 3' else 3), (name, definite)
        assert solved >= 3 * len(sc['layouts']) * sum(definite[(p, 0.0)] for p in sc['points'] if p != ZERO_CURVATURE) and len(definite) == 3 * npoints
        assert max(max(v) for v in worst.values()) <= 1, (name, worst)


def _line_reference(ref, direction, local, t0, cfg):
    """psi(x + t d) for t = t0 2^-k, k = 0 .. 3, in np.longdouble, and its bound: the psi bound of _eval_bounds at the moved point
    (S = S(x) + t S(d): the sum of the absolute terms is A(x) + t A(d)), and what forming the argument in two parts adds: y S(x), y S(d),
    their product with t and the sum round once each: 3 H |y| (A(x) + t A(d)) instead of the one rounding of y S.  The theta part of a
    caller's direction goes through reparam like the point (16 H of the absolute terms, (a) of tests/test_loss_arithmetic_gpu.py); a
    Newton direction (``local``) is taken as the kernel left it.  Regulariser: xi + t d_xi rounds twice before the square: the square
    root moves by at most 2 H (|xi| + t |d_xi|) per term (its slope is below 1)."""
    import test_loss_arithmetic_gpu as LA
    X, H = np.longdouble, LA.H
    N, M = ref['N'], ref['M']
    ql, y = ref['q_local'], ref['y'].astype(X)
    d = np.asarray(direction, np.float64).astype(X)
    dth = d[:6] if local else ref['R'] @ d[:6]
    dth_abs = np.zeros(6, X) if local else ref['R'] @ np.abs(d[:6])
    S0, Sd, Ad = (ref['theta_local'][:, None] * ql).sum(axis=0), (dth[:, None] * ql).sum(axis=0), (np.abs(dth)[:, None] * np.abs(ql)).sum(axis=0)
    if M:
        indptr, indices, data = ref['smat']
        assert (np.diff(indptr) > 0).all()
        w, xi = data.astype(X), ref['xi']
        S0 = S0 + np.add.reduceat(w * xi[indices], indptr[:-1])
        Sd = Sd + np.add.reduceat(w * d[6:][indices], indptr[:-1])
        Ad = Ad + np.add.reduceat(w * np.abs(d[6:])[indices], indptr[:-1])
    al, ep = X(float(cfg['alpha'])), X(float(cfg['epsilon']))
    vals, bounds = [], []
    for k in range(4):
        t = X(t0) * X(2) ** -k
        A = ref['A'] + t * Ad
        dS = (14 + ref['nnz']) * H * A + 16 * H * (LA.F6 * (ref['theta_local_abs'] + t * dth_abs)).sum()
        dt = np.abs(y) * dS * (1 + H) + 3 * H * np.abs(y) * A
        tt = y * (S0 + t * Sd)
        with np.errstate(all='ignore'):
            E = np.exp(-np.abs(tt))
            phi = np.maximum(-tt, X(0)) + np.log1p(E)
            th = np.where(tt >= 0, E / (1 + E), 1 / (1 + E))
        phi_sum, reg_sum, move = phi.sum(), X(0), X(0)
        if M:
            xt = ref['xi'] + t * d[6:]
            reg_sum = al * np.sqrt(xt * xt + ep).sum()
            move = al * 2 * H * (np.abs(ref['xi']) + t * np.abs(d[6:])).sum()
        psi = phi_sum + max(reg_sum - ref['reg0'], X(0))
        vals.append(psi)
        bounds.append(LA._psi_bound(N, M, tt, th, dt, phi_sum, reg_sum, ref['reg0'], psi) + move)
    return np.array(vals), np.array(bounds)


def test_line_sweep_within_derived_bounds(steps):
    """(g) The four values of the line-search sweep against psi(x + t d) in np.longdouble: along the Newton direction of every launch
    (t0 = 1, 0.5, 4 with tau = 0, 1e-12, 1e-4 in every layout; 2^-36 with mu = 0.25), along a caller's direction with large xi
    components (all four t0))."""
    X = np.longdouble
    for name, sc in steps['scenes'].items():
        worst, count = {}, {}
        for r in _recs(sc):
            q = r['res']
            if r['point'] == ZERO_CURVATURE:
                assert np.isnan(q['line']).all()
                continue
            if r['kind'] == 'zero':                                        # (test_line_sweep_along_a_zero_direction)
                continue
            if r['kind'] == 'newton' and q['rc'] != 0:
                assert np.isnan(q['line']).all()
                continue
            ref = _reference(steps, name, r['point'], 0.0)[0]
            vals, bounds = _line_reference(ref, q['dir'] if r['kind'] == 'newton' else sc['given'], r['kind'] == 'newton', r['t0'], sc['cfg'])
            key = (r['kind'], r['t0'])
            worst[key] = max(worst.get(key, 0.0), _worst(q['line'], vals, bounds))
            count[key] = count.get(key, 0) + 1
        for key in sorted(worst):
            print(f'{name}: along the {"Newton" if key[0] == "newton" else "given"} direction, t0 = {key[1]:g}: worst error / bound {worst[key]:.3f} ({count[key]} sweeps)')
        assert {k for k in worst if k[0] == 'given'} == {('given', t0) for t0 in STEP_T0} and {k[1] for k in worst if k[0] == 'newton'} == set(STEP_T0), (name, sorted(worst))
        assert max(worst.values()) <= 1, (name, worst)


def test_line_sweep_along_a_zero_direction(steps):
    """(g) Along d = 0 all four values of the sweep equal the psi_value of sdsm_batch_eval bit for bit, in every layout.
    (This test found that they did not: in 27 of 184 sweeps -- the same points in every layout, never with xi = 0 -- all four were one unit
    in the last place of psi off.  eval_line wrote S(x) as v^2 x1 + v b + a like poly_surface, and the compiler fused the OTHER product
    into the multiply-add there; the multiply-adds of eval_line are now written out in poly_surface's compiled form.  DESIGN.md section 2.)"""
    off = []
    for name, sc in steps['scenes'].items():
        for r in _recs(sc, kind='zero'):
            q, want = r['res'], sc['psi_value'][r['point']]
            assert q['psi_value'] == want, (name, r['point'], r['layout'])
            if not (q['line'] == want).all():
                off.append((name, r['point'], r['layout'], ((q['line'] - want) / np.spacing(want)).tolist()))
    for o in off:
        print('sweep along d = 0 differs from psi_value: %s, %s, %s: %s ulp' % o)
    assert not off, f'{len(off)} sweeps along d = 0 differ from psi_value'


def test_step_entry_point_arguments(steps):
    import torch
    from superdsm_amd import _capi, engine
    from test_loss_arithmetic_gpu import _blob_scene
    L = _capi.lib()
    y, atoms = _blob_scene()
    img = engine.DeviceImage(y, None, atoms, 8)
    batch = engine.Batch(img, [[1]], steps['scenes']['ell']['cfg'])
    p = np.zeros(6)
    batch.launch()
    torch.cuda.synchronize()
    for kw in (dict(reg_mu=-0.1), dict(reg_mu=1.5), dict(tau=-1.0), dict(t0=0.0), dict(reg_mu=float('nan'))):
        with pytest.raises(_capi.SdsmError):
            batch.evaluate_step('class 1', [p], **kw)
    d_out = torch.empty(64, dtype=torch.float64, device=img.device)
    args = (batch.plan, engine._ptr(batch.ws), batch.ws_bytes)
    assert L.sdsm_batch_eval_step(*args, 7, 0.0, 0.0, 1.0, engine._ptr(d_out), None, engine._ptr(d_out), 64, None) == ERR_ARGUMENT       # unknown layout
    assert L.sdsm_batch_eval_step(*args, 0, 0.0, 0.0, 1.0, None, None, engine._ptr(d_out), 64, None) == ERR_ARGUMENT
    small = batch.evaluate_step('class 1', [p])[0]
    assert small['rc'] == 0 and small['hess'].shape == (6, 6) and small['stored'].all()
    d_par = torch.zeros(6, dtype=torch.float64, device=img.device)
    with torch.cuda.device(img.device):
        assert L.sdsm_batch_eval_step(*args, 0, 0.0, 0.0, 1.0, engine._ptr(d_par), None, engine._ptr(d_out), 20, engine._stream()) == _capi.SDSM_OK
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert out[0] == -1 and np.isnan(out[1:20]).all()                       # a block that does not fit its stride: rc -1, nothing else
