"""The references of tests/test_newton_step_gpu.py, checked without a GPU: testing.hessian_reference (np.longdouble, the solver's
approximate Hessian in the candidate's local frame) against the reference's own Hessians (tests/golden/energy.npz) and against the
oracle's float64 matrix (orc_energy_eval_thr); the leading rule and the envelope against each other; the backward-error bound of the
Newton step (testing.step_residual) against a float64 Cholesky solve -- which must pass -- and the same solve with one factor entry
moved by 1e-9 -- which must fail."""
import json
import os

import numpy as np
import pytest
import scipy.linalg

from superdsm_amd import testing as T

if not T.longdouble_is_extended():
    pytest.skip('np.longdouble has fewer than 64 significand bits here: no extended-precision reference', allow_module_level=True)

X = np.longdouble
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _blob():
    from test_loss_arithmetic_gpu import _blob_scene
    return _blob_scene()


def _to_global(ref):
    """R^T H R and R^T g with R extended by the identity on xi: the local frame's theta is R theta."""
    n = 6 + ref['M']
    Rf = np.eye(n, dtype=X)
    Rf[:6, :6] = ref['R']
    return Rf.T @ ref['hess'] @ Rf, Rf.T @ ref['grad_local']


def test_exact_hessian_reproduces_the_golden_hessians():
    """hess_thr = 0, reg_mu = 0: every entry is a leading one and the curvature is the true one -- the reference's Hessian
    (dsm.py:352-385) at every point of tests/golden/energy.npz (18 cases), at the tolerances the suite already holds against that file."""
    d = np.load(os.path.join(G, 'energy.npz'))
    cfg0 = json.loads(str(d['cfg']))
    y, atoms = d['y'], d['atoms']
    assert int(d['n_cases']) >= 18
    for k in range(int(d['n_cases'])):
        deform = bool(d[f'c{k}_deform'])
        cfg = dict(cfg0, alpha=float(d[f'c{k}_alpha']), smooth_amount=cfg0['smooth_amount'] if deform else np.inf)
        p = d[f'c{k}_params']
        ref = T.hessian_reference(y, None, atoms, d[f'c{k}_fp'].tolist(), cfg, p[:6], p[6:] if p.size > 6 else None, hess_thr=0.0, reg_mu=0.0)
        assert 6 + ref['M'] == p.size
        Hg, gg = _to_global(ref)
        ref_H, ref_g = d[f'c{k}_hessian_lower'], d[f'c{k}_grad']
        # (the tolerance of test_point_evaluations_match_reference_energy, tests/test_gpu_parity.py: the reference forms kappa = theta - theta^2 in
        # float64, an absolute error of ~1e-16 per pixel where theta -> 1, this one the product form: 1e-13 of the natural scale of an entry,
        # sum y^2 |J_a J_b| <= 4 sum y^2)
        sel = np.isin(atoms, d[f'c{k}_fp'])
        np.testing.assert_allclose(np.tril(Hg).astype(np.float64), ref_H, rtol=1e-9, atol=4e-13 * float((y[sel] ** 2).sum()))
        np.testing.assert_allclose(gg.astype(np.float64), ref_g, rtol=1e-10, atol=1e-10 * np.abs(ref_g).max())
        np.testing.assert_allclose(float(ref['psi']), float(d[f'c{k}_value']), rtol=1e-12)


def _points(M, seed=7):
    rng = np.random.default_rng(seed)
    th = np.array([-3.0, -2.0, 0.3, 1.2, 1.1, 0.4])
    out = [np.concatenate([th, np.zeros(M)]), np.concatenate([th, 0.5 * rng.standard_normal(M)]),
           np.concatenate([th * 1.5, 1e-3 * rng.standard_normal(M)]), np.concatenate([0.2 * th, 300.0 * rng.standard_normal(M)])]
    out[0][5] = 0.0
    return out


@pytest.mark.parametrize('reg_mu', [0.0, 0.25, 1.0])
def test_thresholded_hessian_matches_the_oracle(reg_mu):
    """hess_thr = 0.1: the oracle's float64 matrix (energy_eval_thr, what orc_newton factors) at four points of the blob, entries to
    1e-10 of their natural scale sqrt(h_aa h_bb)."""
    from oracle import oracle
    y, atoms = _blob()
    cfg = T._toy_cfg(background_margin=8)
    region = oracle.region_mask(y, None, atoms, [1], 8)
    E = oracle.Energy(y, region, cfg['epsilon'], cfg['alpha'], cfg['smooth_amount'], cfg['gaussian_shape_multiplier'], cfg['smooth_subsample'])
    assert E.M == 47
    for p in _points(E.M):
        ref = T.hessian_reference(y, None, atoms, [1], cfg, p[:6], p[6:], reg_mu=reg_mu)
        v, g, Ho = E.eval_thr(p, T.HESS_THR, reg_mu)
        Hg, gg = _to_global(ref)
        scale = np.sqrt(np.diag(Ho))
        assert (scale > 0).all()
        assert float((np.abs(Hg - Ho) / np.outer(scale, scale)).max()) <= 1e-10
        assert (Hg[Ho != 0] != 0).all()                                 # (the converse holds to the tolerance above only: the oracle skips a pixel whose float64 kappa is 0)
        np.testing.assert_allclose(gg.astype(np.float64), g, rtol=1e-10, atol=1e-10 * np.abs(g).max())
        np.testing.assert_allclose(float(ref['psi']), v, rtol=1e-12)
        exact = T.hessian_reference(y, None, atoms, [1], cfg, p[:6], p[6:], reg_mu=reg_mu, hess_thr=0.0)
        assert (exact['hess'] != 0).sum() > (ref['hess'] != 0).sum()   # ... and some are


def test_leading_rule_and_envelope():
    """The float32 comparison of the leading rule at its edge, and the envelope the leading entries define: every coupled pair lies
    inside it, first columns are multiples of the panel width and non-decreasing, rows do not overlap, rend is the last row that
    reaches a panel."""
    from oracle import oracle
    w = np.array([1.0, 0.1, np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(0)), 0.5, 0.05])
    lead = T.leading_entries(np.array([0, 4, 6]), w)
    assert lead.tolist() == [True, bool(np.float32(0.1) >= np.float32(0.1) * np.float32(1.0)), True, False, True, bool(np.float32(0.05) >= np.float32(0.1) * np.float32(0.5))]
    assert T.leading_entries(np.array([0, 4, 6]), w, 0.0).all()
    y, atoms = _blob()
    for kw, want in ((dict(smooth_subsample=8), (47, 1055, 6)), (dict(smooth_subsample=5), (123, 5093, 13))):
        cfg = T._toy_cfg(background_margin=8, **kw)
        region = oracle.region_mask(y, None, atoms, [1], 8)
        rr, cc = np.nonzero(region)
        sm = oracle.smooth_matrix(region, cfg['smooth_amount'], cfg['gaussian_shape_multiplier'], cfg['smooth_subsample'])
        lead = T.leading_entries(sm.indptr, sm.data)
        env = T.envelope_reference(rr, cc, sm.M, sm.indptr, sm.indices, lead)
        M = sm.M
        assert (M, env['env_size'], env['hzmax']) == want
        fst, rb = env['fst'], env['rb']
        assert (fst[:M] % T.PANEL == 0).all() and (np.diff(fst[:M]) >= 0).all() and (fst[:M] <= np.arange(M)).all() and (fst[M:] == 0).all()
        lo, hi = rb + fst, rb + np.arange(M + 6)                       # storage of row a: [rb + fst, rb + a]
        assert lo[0] == 0 and (lo[1:] == hi[:-1] + 1).all() and hi[-1] + 1 == env['env_size']
        for p, re in enumerate(env['rend']):
            assert fst[re] <= T.PANEL * p and (re == M - 1 or fst[re + 1] > T.PANEL * p)
        ref = T.hessian_reference(y, None, atoms, [1], cfg, [-3.0, -2.0, 0.3, 1.2, 1.1, 0.4], np.zeros(M))
        a, b = np.nonzero(ref['hess'][6:, 6:])
        assert (np.minimum(a, b) >= fst[np.maximum(a, b)]).all() and a.size > M


def _spd_system(n, seed):
    """n = 53, 129: the reference matrix of the blob (smooth_subsample 8, 5) at a perturbed point, float64, with its gradient; else a
    random positive definite matrix, badly scaled (the bound is componentwise)."""
    rng = np.random.default_rng(seed)
    if n in (53, 129):
        y, atoms = _blob()
        cfg = T._toy_cfg(background_margin=8, smooth_subsample={53: 8, 129: 5}[n])
        ref = T.hessian_reference(y, None, atoms, [1], cfg, [-3.0, -2.0, 0.3, 1.2, 1.1, 0.4], 0.5 * rng.standard_normal(n - 6))
        assert ref['hess'].shape == (n, n)
        return ref['hess'].astype(np.float64), ref['grad_local'].astype(np.float64)
    B = rng.standard_normal((n, n + 5))
    s = 10.0 ** rng.uniform(-4, 4, n)
    return (B @ B.T) * np.outer(s, s), rng.standard_normal(n) * s


@pytest.mark.parametrize('n', [6, 53, 129, 348])
@pytest.mark.parametrize('tau', [0.0, 1e-12, 1e-4])
def test_step_bound_holds_a_float64_cholesky_and_rejects_a_perturbed_one(n, tau):
    Hm, g = _spd_system(n, n)
    A = Hm + tau * np.diag(np.diag(Hm))
    c = scipy.linalg.cholesky(A, lower=True)
    d = scipy.linalg.cho_solve((c, True), -g)
    res = T.step_residual(Hm, g, d, tau)
    print(f'n = {n}, tau = {tau:g}: float64 Cholesky solve: residual / bound = {res["ratio"]:.3f}')
    assert res['ratio'] < 1
    z = scipy.linalg.solve_triangular(c, -g, lower=True)
    assert abs(X(float(z @ z)) - res['lam2']) <= res['lam2_bound']     # lam2 as the kernel forms it: the squared norm of the forward substitution
    # one factor entry moved by 1e-9 of itself -- the one that carries the most of the solution: (row, column) maximising |l_ik d_i d_k|
    w = np.abs(np.tril(c, -1) * np.outer(d, d))
    i, k = np.unravel_index(int(np.argmax(w)), w.shape)
    c2 = c.copy()
    c2[i, k] *= 1 + 1e-9
    bad = T.step_residual(Hm, g, scipy.linalg.cho_solve((c2, True), -g), tau)
    print(f'n = {n}, tau = {tau:g}: factor entry ({i}, {k}) moved by 1e-9: residual / bound = {bad["ratio"]:.3g}')
    assert bad['ratio'] > 1
