"""The loss arithmetic of the solve kernels, value by value: exp_neg, log_w (with its table in LDS), softplus_neg, loss_terms, rcp_f64 and
rsqrt_f64 as compiled for the device (sdsm_probe_loss_arithmetic: one launch, the production functions called as they stand) against
np.longdouble references (superdsm_amd/testing.py; tests/test_loss_arithmetic_cpu.py checks those against mpmath).

Every bound is one of the kernel's own claims (the comments of sdsm_solve.hip) or is composed from them here, next to its assertion;
none is fitted to what the device returns.  Every test prints its worst error as a fraction of its bound and where it occurred."""
import numpy as np
import pytest

from superdsm_amd import testing as T

pytestmark = pytest.mark.gpu

if not T.longdouble_is_extended():
    pytest.skip('np.longdouble has fewer than 64 significand bits here: no extended-precision reference', allow_module_level=True)

X = np.longdouble
H = 2.0 ** -53                    # unit roundoff of float64: fl(a op b) = (a op b)(1 + d), |d| <= H, for a normal result
SUB = X(2) ** -1075               # half the subnormal quantum (below float64's range: a longdouble): the absolute error of a rounding whose result is subnormal
TINY = 2.0 ** -1022               # smallest normal double
# the claims (sdsm_solve.hip)
E_EXP = 1.8e-16                   # exp_neg: relative
E_LOG_ABS = 2.0 ** -53            # log_w: absolute (1.1e-16)
E_LOG_REL = 5e-16                 # log_w: relative
E_RCP = 2.2e-15                   # rcp_f64: relative
E_RSQRT = 4.2e-15                 # rsqrt_f64: relative
SECOND_ORDER = 1 + 1e-6           # covers the products of two of the relative terms below (each < 1e-14: their products < 1e-28 of the value)


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    from superdsm_amd import _capi
    _capi.lib()     # fails loudly if libsdsm_hip.so is missing
    return torch


@pytest.fixture(scope='module')
def probe(gpu):
    """ONE launch of the probe over all inputs, and the references at the t the DEVICE formed (checked to be fl(y S))."""
    from superdsm_amd import engine
    inp = T.loss_probe_inputs()
    n = max(inp['y'].size, inp['x_unit'].size + inp['x_normal'].size)
    assert n <= T.LOSS_PROBE_MAX
    pad = lambda a: np.concatenate([a, np.ones(n - a.size)])
    y, S, x = pad(inp['y']), pad(inp['S']), pad(np.concatenate([inp['x_unit'], inp['x_normal']]))
    out = engine.probe_loss_arithmetic(y, S, x)
    with np.errstate(all='ignore'):
        t = y * S
    assert np.array_equal(out['t'], t, equal_nan=True) and np.array_equal(np.signbit(out['t']), np.signbit(t)), 'the device forms t = y * S in one rounded product'
    return dict(out, y=y, S=S, x=x, n_unit=inp['x_unit'].size, n_x=inp['x_unit'].size + inp['x_normal'].size, fin=np.isfinite(t), ref=T.loss_reference(t, y))


def _report(name, err, bound, where, arg_name='t'):
    """Worst err / bound over the elements, printed with its argument; returns it."""
    err, bound = np.asarray(err, X), np.asarray(bound, X)
    with np.errstate(all='ignore'):
        ratio = np.where(err == 0, X(0), err / bound)
    assert not np.isnan(ratio).any(), name
    k = int(np.argmax(ratio))
    print(f'{name}: worst error / bound = {float(ratio[k]):.3f} at {arg_name} = {float(np.asarray(where)[k])!r} (error {err[k]:.3e}, bound {bound[k]:.3e}; {err.size} values)')
    return float(ratio[k])


def _bound_exp(E):
    """exp_neg's claim: 1.8e-16 relative; where the exact result is below 2^-1022 the ldexp rounds a second time, to a subnormal: half a
    subnormal quantum on top."""
    return E_EXP * E + np.where(E < TINY, X(SUB), X(0))


def test_exp_neg(probe):
    a = np.minimum(np.abs(probe['t']), T.LOSS_GUARD)           # what softplus_neg / loss_terms hand to exp_neg (NaN -> 750)
    a = np.where(np.isnan(a), T.LOSS_GUARD, a)
    u, E = probe['exp'], np.exp(-a.astype(X))
    assert np.isfinite(u).all() and (u >= 0).all() and (u <= 1).all()
    assert (u[a == T.LOSS_GUARD] == 0).all() and (a == T.LOSS_GUARD).sum() > 1000                 # exactly 0 at the guard
    assert (u[a == 0] == 1).all()
    worst = _report('exp_neg', np.abs(u.astype(X) - E), _bound_exp(E), a, 'a')
    sub = (E < TINY) & (E > X(2.0) ** -1076)
    assert sub.sum() > 20000
    _report('exp_neg, normal results', np.abs(u.astype(X) - E)[E >= TINY], _bound_exp(E)[E >= TINY], a[E >= TINY], 'a')
    _report('exp_neg, subnormal results', np.abs(u.astype(X) - E)[sub], _bound_exp(E)[sub], a[sub], 'a')
    assert worst <= 1


def test_log_w(probe):
    """log_w(u, fl(1 + u)) at the u exp_neg returned, against log(fl(1 + u))."""
    u, L = probe['exp'], probe['log']
    w = 1.0 + u                                                 # the same rounded sum the device forms
    ref = T.log_reference(w)
    err = np.abs(L.astype(X) - ref)
    pts, edges = T.loss_table_points()
    for p in pts:                                               # the inputs reach every table point from both sides (s = 0 and either sign)
        near = u[np.abs(u - p) <= 4 * np.spacing(p)]
        assert near.size and near.min() <= p <= near.max(), p
    print(f'log_w: {sum(int((u == p).any()) for p in pts)} of 65 table points hit exactly')
    worst_abs = _report('log_w, absolute', err, np.full(u.size, E_LOG_ABS), u, 'u')
    worst_rel = _report('log_w, relative', err, E_LOG_REL * ref, u, 'u')
    assert (L[u == 0] == 0).all() and (u == 0).sum() > 1000                                        # w = 1 gives 0
    assert (L[u == 1] == float(np.log(X(2)))).all() and (u == 1).sum() >= 2                        # w = 2 gives the rounded ln 2
    assert float(np.log(X(2))) == float.fromhex('0x1.62e42fefa39efp-1')
    # monotone non-decreasing over the sorted sample (equal u: equal bits)
    order = np.argsort(u, kind='stable')
    us, Ls = u[order], L[order]
    assert (np.diff(Ls) >= 0).all(), us[np.flatnonzero(np.diff(Ls) < 0)[:5]]
    # Both sides of every bin edge.  The bin follows w: j = floor(64 (w - 1) + 1 / 2) (exact in float64).  The largest w of bin j (series
    # argument s near +1 / 128) and the smallest of bin j + 1 (table entry j + 1, s near -1 / 128) are neighbouring doubles or nearly so;
    # each branch is within the absolute bound of the true logarithm, so the step between them differs from the true step,
    # log(w_hi) - log(w_lo), by at most twice that bound.
    ws = 1.0 + us
    jbin = np.floor(64.0 * (ws - 1.0) + 0.5).astype(int)
    worst_edge = 0.0
    for j in range(64):
        lo, hi = np.flatnonzero(jbin == j)[-1], np.flatnonzero(jbin == j + 1)[0]
        assert hi == lo + 1 and 0 < ws[hi] - ws[lo] <= 2 * np.spacing(ws[lo]), (j, ws[lo], ws[hi])
        step = X(Ls[hi]) - X(Ls[lo])
        true = T.log_reference(ws[hi]) - T.log_reference(ws[lo])
        worst_edge = max(worst_edge, float(abs(step - true) / (2 * E_LOG_ABS)))
    print(f'log_w, step across the bin edges: worst error / bound = {worst_edge:.3f}')
    assert worst_abs <= 1 and worst_rel <= 1 and worst_edge <= 1


def _bound_softplus(t, ref):
    """log(1 + exp(-t)) as the kernels form it, fl(log_w(u, w) + max(-t, 0)) with u = exp_neg(min(|t|, 750)), w = fl(1 + u), against the
    exact F = max(-t, 0) + log(1 + E), E = exp(-|t|):
      (i)   u for E: |log(1 + u) - log(1 + E)| <= |u - E| (the derivative 1 / (1 + .) is <= 1) <= exp_neg's bound; beyond the guard
            u = 0 for an E < exp(-750) < 2^-1075, which the subnormal term of that bound covers;
      (ii)  the rounding of 1 + u: w = (1 + u)(1 + d), |d| <= H, moves the logarithm by |log(1 + d)| <= H / (1 - H);
      (iii) log_w's absolute bound;
      (iv)  the final addition (max(-t, 0) is exact; + t * 0 adds an exact zero): H of its result, which is within (i) .. (iii) of F."""
    E = np.exp(-np.abs(t.astype(X)))
    b0 = _bound_exp(E) + H / (1 - H) + E_LOG_ABS
    return b0 + H * (ref + b0)


def test_softplus_and_phi(probe):
    t, fin = probe['t'], probe['fin']
    sp, phi = probe['softplus'], probe['phi']
    assert np.array_equal(sp.view(np.uint64), phi.view(np.uint64)), 'softplus_neg and the phi of loss_terms return the same bits'
    assert np.isnan(sp[~fin]).all() and (~fin).sum() >= 5                                          # NaN for a non-finite t
    low = fin & (t <= -T.LOSS_GUARD)
    assert (sp[low] == -t[low]).all() and low.sum() > 1000                                         # exactly |t| below the guard
    assert (sp[fin] >= 0).all()
    ref = probe['ref']['softplus'][fin]
    worst = _report('softplus_neg / phi', np.abs(sp[fin].astype(X) - ref), _bound_softplus(t[fin], ref), t[fin])
    assert worst <= 1


def _bound_theta_rel(t):
    """theta = 1 / (1 + exp(t)) as loss_terms forms it, relative.  With u = E (1 + e1), |e1| <= E_EXP (exp_neg), w = (1 + u)(1 + d),
    |d| <= H, rw = rcp_f64(w) = (1 + p) / w, |p| <= E_RCP:
      t >= 0:  theta = fl(u rw) = [E / (1 + E)] (1 + e1) [(1 + E) / (1 + u)] (1 + p) / (1 + d) (1 + d1); |(1 + E) / (1 + u) - 1| <=
               |u - E| / (1 + u) <= E_EXP: 2 E_EXP + E_RCP + 2 H;
      t < 0:   theta = rw = [1 / (1 + E)] [(1 + E) / (1 + u)] (1 + p) / (1 + d): E_EXP + E_RCP + H.
    (Subnormal u or products: the absolute terms of the callers.)"""
    return np.where(t >= 0, 2 * E_EXP + E_RCP + 2 * H, E_EXP + E_RCP + H) * SECOND_ORDER


def test_residual_r(probe):
    """r = fl(-y theta) against -y / (1 + exp(t)), on both branches of t >= 0: theta's relative bound and H for the product; where u,
    u rw or y theta is subnormal (t beyond ~708, or a small |y|) each of those roundings is absolute, half a subnormal quantum: u's and
    the quotient's scaled by |y| (rw <= 1), the last one as it is.  Beyond the guard theta is exactly 0 (t >= 750, exact value
    |y| exp(-750) / .. < |y| 2^-1075) or exactly rcp_f64(1) = 1 (t <= -750)."""
    t, y, fin = probe['t'][probe['fin']], probe['y'][probe['fin']], probe['fin']
    r, ref = probe['r'][fin], probe['ref']['r'][fin]
    bound = (_bound_theta_rel(t) + H) * SECOND_ORDER * np.abs(ref) + (2 * np.abs(y).astype(X) + 1) * SUB
    err = np.abs(r.astype(X) - ref)
    pos = t >= 0
    assert pos.sum() > 100000 and (~pos).sum() > 100000
    w1 = _report('r = -y theta, t >= 0', err[pos], bound[pos], t[pos])
    w2 = _report('r = -y theta, t < 0', err[~pos], bound[~pos], t[~pos])
    mid = np.abs(ref) > X(2) ** -900                            # (no subnormal anywhere near: the relative bound alone)
    _report('r = -y theta, normal results', err[mid], bound[mid], t[mid])
    assert (np.sign(r) == -np.sign(y))[r != 0].all()
    assert w1 <= 1 and w2 <= 1


def test_curvature_term(probe):
    """dcurv = fl(fl(y y) fl(q rw)), q = fl(u rw), against y^2 E / (1 + E)^2 -- the product form, which must hold its RELATIVE accuracy
    where theta is within 1e-16 of 1 (t < -37) and must never be negative.  In the notation of _bound_theta_rel:
    q rw = [E / (1 + E)^2] (1 + e1) [(1 + E) / (1 + u)]^2 (1 + p)^2 / (1 + d)^2 and four roundings (y y, u rw, q rw, the product):
    3 E_EXP + 2 E_RCP + 6 H.  Subnormal u, q or q rw: half a subnormal quantum each, scaled by y^2 (rw <= 1); a subnormal result: one more."""
    t, y, fin = probe['t'][probe['fin']], probe['y'][probe['fin']], probe['fin']
    d, ref = probe['dcurv'][fin], probe['ref']['dcurv'][fin]
    assert (d >= 0).all() and np.isfinite(d).all()
    y2 = y.astype(X) ** 2
    bound = (3 * E_EXP + 2 * E_RCP + 6 * H) * SECOND_ORDER * ref + (3 * y2 + 1) * SUB
    err = np.abs(d.astype(X) - ref)
    near_one = t < -37.0                                        # theta = 1 / (1 + exp(t)) >= 1 - 1e-16
    assert near_one.sum() > 50000 and (1 - probe['ref']['theta'][fin][near_one]).max() < 1e-16
    w1 = _report('dcurv', err, bound, t)
    mid = ref > X(2) ** -900                                    # (no subnormal anywhere near: the relative bound alone)
    _report('dcurv, normal results', err[mid], bound[mid], t[mid])
    w2 = _report('dcurv, theta within 1e-16 of 1', err[near_one], bound[near_one], t[near_one])
    assert w1 <= 1 and w2 <= 1


def test_rcp_and_rsqrt(probe):
    """rcp_f64 (2.2e-15 relative) on w in [1, 2] -- the arguments the passes give it -- and on 2^-1021 .. 2^1021, where the
    reciprocal and its hardware estimate are normal too; rsqrt_f64 (4.2e-15 relative) on [1, 2] and over the whole normal range."""
    x = probe['x'][:probe['n_x']]
    xl = x.astype(X)
    unit = np.arange(x.size) < probe['n_unit']
    rcp, rsq = probe['rcp'][:x.size], probe['rsqrt'][:x.size]
    ok = unit | ((x >= 2.0 ** -1021) & (x <= 2.0 ** 1021))
    assert unit.sum() > 100000 and (ok & ~unit).sum() > 100000 and (x[unit].min(), x[unit].max()) == (1.0, 2.0)
    r_ref, q_ref = 1 / xl, 1 / np.sqrt(xl)
    w = [_report('rcp_f64, w in [1, 2]', np.abs(rcp.astype(X) - r_ref)[unit], (E_RCP * r_ref)[unit], x[unit], 'x'),
         _report('rcp_f64, normal range', np.abs(rcp.astype(X) - r_ref)[ok], (E_RCP * r_ref)[ok], x[ok], 'x'),
         _report('rsqrt_f64, w in [1, 2]', np.abs(rsq.astype(X) - q_ref)[unit], (E_RSQRT * q_ref)[unit], x[unit], 'x'),
         _report('rsqrt_f64, normal range', np.abs(rsq.astype(X) - q_ref), E_RSQRT * q_ref, x, 'x')]
    assert max(w) <= 1


# ---------------------------------------------------------------------------------------------------------
# Point evaluations (sdsm_batch_eval: the evaluators of the solve kernels) against testing.energy_reference, held to bounds derived
# from the per-pixel bounds above and from how the kernels sum (sections 4 and 5, and the limits section).
#
# Notation.  Pixel i: y_i, t_i = y_i S_i, theta_i = 1 / (1 + e^t_i), kappa_i, r_i = -y_i theta_i, d_i = y_i^2 kappa_i (the reference's
# values).  A_i: the sum of the absolute values of the terms of S_i in the candidate's local frame, where the kernels evaluate it
# (|u|, |v| <= 1; theta_local = R theta, every entry of R >= 0).  F = (1, 1, 2, 2, 2, 1) bounds |q_k| there.
#
# (a) S.  theta_local is formed in float64 (reparam): P0 = 1 / (inv_h z) carries 3 roundings, O0 one; a term of a local coefficient
#     is a product of a parameter and two such factors (<= 6 H from the factors, 2 from the products), a coefficient the sum of <= 6
#     terms (5 more): <= 16 H of the sum of its absolute terms, `theta_local_abs`.  That moves S_i by <= 16 H sum_k F_k theta_local_abs_k.
#     The evaluation itself: a coordinate carries 2 roundings, its square 5, a polynomial term <= 7, the sums of the 6 terms <= 5 more
#     on the longest path, every product w xi one (w is a float32, exact) and its addition one: (14 + nnz_i) H A_i with room to spare
#     (fused multiply-adds only remove roundings).
# (b) t_i = fl(y_i S_i): |dt_i| <= |y_i| dS_i (1 + H) + H |t_i|.
# (c) phi: the per-pixel bound of softplus_neg at t_i, and the move of its argument: |phi'| = theta, |phi''| = kappa <= 1 / 4:
#     theta_i dt_i + dt_i^2 / 8.
# (d) r, d: their relative bounds (test_residual_r, test_curvature_term) and the move of t: r' = y kappa (|theta''| <= 0.1), d' = y^2
#     kappa (1 - 2 theta), |.| <= y^2 kappa (|kappa''| <= 0.2).
# ---------------------------------------------------------------------------------------------------------
REL_R = (2 * E_EXP + E_RCP + 3 * H) * SECOND_ORDER            # the larger branch of _bound_theta_rel and the product with y
REL_D = (3 * E_EXP + 2 * E_RCP + 6 * H) * SECOND_ORDER
F6 = np.array([1, 1, 2, 2, 2, 1], X)


def _psi_bound(N, M, t, th, dt, phi_sum, reg_sum, reg0, psi):
    """The bound on psi of a pass whose arguments t_i are within dt_i of the reference's t_i ((c) above and the order of the sums)."""
    E = np.exp(-np.abs(t))
    phi = np.maximum(-t, X(0)) + np.log1p(E)
    b0 = _bound_exp(E) + H / (1 - H) + E_LOG_ABS
    pix = ((b0 + H * (phi + b0)) * SECOND_ORDER + th * dt + dt * dt / 8).sum()                           # (c)
    # psi.  Summation order: the <= 4 pixels of a run one after the other, the 64 runs of a chunk by a wavefront
    # butterfly (6 levels), the 8 chunk totals of a super-chunk one after the other, then the super-chunk sums one after the other; a
    # super-chunk is 512 runs and a run holds at least one pixel: at most ceil(N / 512) + 1 of them.  All terms are >= 0, so the sum
    # is off by at most (the longest chain of additions) H (the sum of the terms as computed).
    depth = 4 + 6 + 8 + -(-N // 512) + 1
    b_psi = pix + depth * H * (phi_sum + pix) * SECOND_ORDER
    if M > 0:
        # regulariser alpha sum sqrt(xi^2 + eps) - alpha sqrt(eps) M: a term carries <= 4 roundings (square, sum, a square root within
        # one ulp), every lane adds ceil(M / 64) of them, 6 butterfly levels, the product with alpha, the difference; alpha sqrt(eps) M
        # is formed in float64 on the host (3): (ceil(M / 64) + 14) H of the two magnitudes
        b_psi = b_psi + (-(-M // 64) + 14) * H * (reg_sum + reg0)
    return (b_psi + H * abs(psi)) * SECOND_ORDER                                                         # pixel part + regulariser


def _eval_bounds(ref):
    N, M = ref['N'], ref['M']
    y, t, th, ka, A = np.abs(ref['y']).astype(X), ref['t'], ref['theta_hat'], ref['kappa'], ref['A']
    dS = (14 + ref['nnz']) * H * A + 16 * H * (F6 * ref['theta_local_abs']).sum()                       # (a)
    dt = y * dS * (1 + H) + H * np.abs(t)                                                                # (b)
    assert float(dt.max()) < 1e-6                                                                        # (second-order terms are what they are said to be)
    b_psi = _psi_bound(N, M, t, th, dt, ref['phi_sum'], ref['reg_sum'], ref['reg0'], ref['psi'])
    # the fixed-point quanta (fx_exponents; DESIGN, limits: 2^-48 of the largest possible term): gradient terms < 2^(yexp + b), Hessian
    # terms < 2^(2 yexp + min(b, -1)), 2^b >= psi / ln 2 >= every theta (b = 0 from psi >= ln 2 on); a term keeps `bits` bits below that.
    # The evaluation is scaled by the device's own psi, which lies within b_psi of the reference's: the larger exponent of the two.
    lg = int(np.ceil(np.log2(N))) if N > 1 else 0
    bits = min(48, 59 - lg)
    tb = float((ref['psi'] + b_psi) * X(1.442696484))
    b = 0 if not tb < 1.0 else (-400 if tb <= 0 else max(-400, int(np.frexp(tb)[1])))
    unit_g, unit_h = X(2) ** (ref['yexp'] + b - bits), X(2) ** (2 * ref['yexp'] + min(b, -1) - bits)
    dr = REL_R * y * th + y * (ka * dt + X(0.05) * dt * dt) + (2 * y + 1) * SUB                          # (d)
    dd = REL_D * y * y * ka + y * y * (ka * dt + X(0.1) * dt * dt) + (3 * y * y + 1) * SUB
    rho = (F6[:, None] * ref['R']).sum(axis=0)                                                           # rho_a = sum_k R_ka F_k
    # theta gradient: g_a = sum_k R_ka g_local_k, g_local_k = F-multiple of a moment sum_i r_i u^a v^b, |u^a v^b| <= 1.  A moment's
    # term carries <= 14 roundings before it is added (v 2, v^2 5, r v^2 6, the run's 4 terms 3 more; u^2 5 -- the product with it and the
    # sum are exact to 2^-48 of the quantum: two-word fixed point, half of THAT quantum per run), the conversion of the two words 3; the
    # entries of R 10 (reparam of a unit vector), the product and the 6-term sum 7: 36 H sum |r|, and the moved r.
    b_grad = np.zeros(6 + M, X)
    b_grad[:6] = rho * (dr.sum() + 36 * H * ref['abs_r'] + N * unit_g * X(2) ** -49)
    # theta block of the Hessian, H_ab = sum_kl R_ka R_lb H_local_kl, the same way: a term <= 26 roundings (d v^4: 15, u^4: 11), the
    # conversion 3, R H R: 22 per product and a 36-term sum: 90 H sum d.
    b_hess = np.outer(rho, rho) * (dd.sum() + 90 * H * ref['abs_d'] + N * unit_h * X(2) ** -49)
    if M > 0:
        # xi gradient: sum_i w_ij r_i by fused multiply-adds onto the fixed-point constant, each rounding to the quantum: half a quantum
        # per pixel that has the entry; the moved r through the weights; the conversion (H of the sum); the regulariser's alpha xi / sqrt
        # (5 roundings, |xi / sqrt| <= 1) and the final addition.
        indptr, indices, data = ref['smat']
        row = np.repeat(np.arange(N), np.diff(indptr))
        moved, mag, cnt = np.zeros(M, X), np.zeros(M, X), np.zeros(M, X)
        np.add.at(moved, indices, data.astype(X) * dr[row])
        np.add.at(mag, indices, data.astype(X) * (y * th)[row])
        np.add.at(cnt, indices, (data != 0).astype(X))
        b_grad[6:] = moved + cnt * unit_g / 2 + H * mag + 5 * H * X(ref['alpha']) + H * np.abs(ref['grad'][6:])
    return dict(psi=b_psi, grad=b_grad * SECOND_ORDER, hess=b_hess * SECOND_ORDER, dt=dt, dr=dr, dd=dd, unit_g=unit_g, unit_h=unit_h)     # (the last five: for tests/test_newton_step_gpu.py)


def _blob_scene():
    """80 x 96: one blob, |y| in [0.1, 4], one atom; the region (margin 8) has about 3000 pixels."""
    rng = np.random.default_rng(12)
    Hh, Ww = 80, 96
    rr, cc = np.mgrid[:Hh, :Ww]
    y = 3.2 * np.exp(-(((rr - 38) / 17.0) ** 2 + ((cc - 50) / 23.0) ** 2)) - 1.0 + 0.15 * rng.standard_normal((Hh, Ww))
    y = np.where(y >= 0, 1.0, -1.0) * np.clip(np.abs(y), 0.1, 4.0)
    return y, np.ones((Hh, Ww), np.int32)


# layout of sdsm_launch_eval -> the dsm/* settings that put the blob's candidate there: 6 + M <= 128 and an envelope <= 2560 doubles:
# 256 threads; beyond either: 512 threads (smooth_subsample 5: M = 123, one unknown past the limit); smooth_amount = inf: the
# elliptical model (M = 0, pure data term; 256 threads).  The global-memory layout (more than 1018 unknowns: the dense-grid scene of
# tests/test_gpu_parity.py, 13 000 pixels and seconds per reference) is left out.
LAYOUTS = {'256 threads': dict(smooth_subsample=8), '512 threads': dict(smooth_subsample=5), 'elliptical': dict(smooth_amount=np.inf)}
_WORST = {}


def _compare(label, batch, k, params, y, atoms, fp, cfg, M):
    """One evaluation of candidate k of `batch` at `params` against the reference; worst error / bound per quantity into _WORST."""
    ev = batch.evaluate([params] if batch.n == 1 else params)[k]
    p = params if batch.n == 1 else params[k]
    ref = T.energy_reference(y, None, atoms, fp, cfg, p[:6], p[6:] if M > 0 else None, box=batch.mask_info[k])
    ref['alpha'] = float(cfg['alpha'])
    assert ref['M'] == M
    bd = _eval_bounds(ref)
    out = {}
    for name, got, want, bound in (('psi', ev['psi'], ref['psi'], bd['psi']), ('psi_value', ev['psi_value'], ref['psi'], bd['psi']),
                                   ('grad theta', ev['grad'][:6], ref['grad'][:6], bd['grad'][:6]), ('grad xi', ev['grad'][6:], ref['grad'][6:], bd['grad'][6:]),
                                   ('hess theta', ev['hess_theta'], ref['hess_theta'], bd['hess'])):
        got, want, bound = np.atleast_1d(np.asarray(got, X)), np.atleast_1d(want), np.atleast_1d(bound)
        if got.size == 0:
            continue
        assert np.isfinite(got.astype(np.float64)).all(), (label, name)
        with np.errstate(all='ignore'):
            ratio = np.where(got == want, X(0), np.abs(got - want) / bound)
        out[name] = float(ratio.max())
        key = (label.split(':')[0], name)
        _WORST[key] = max(_WORST.get(key, 0.0), out[name])
    return out


@pytest.fixture(scope='module')
def blob(gpu):
    """The blob's candidate solved once per layout (full solve: the workspace for the evaluations, and the kernel's own optimum)."""
    from superdsm_amd import engine
    y, atoms = _blob_scene()
    img = engine.DeviceImage(y, None, atoms, 8)
    out = {}
    for name, kw in LAYOUTS.items():
        cfg = T._toy_cfg(background_margin=8, **kw)
        batch = engine.Batch(img, [[1]], cfg, want_xi=True)
        batch.launch()
        gpu.cuda.synchronize()
        rec = batch.records()[0]
        st = batch.inspect_states()[0]
        M = int(rec['n_deform'])
        small = 6 + M <= 128 and (st['env_size'] if M else 21) <= 2560
        assert small == (name != '512 threads') and (M == 0) == (name == 'elliptical'), (name, M, st)
        xi = batch.xi_dev.cpu().numpy()[:M]
        out[name] = dict(batch=batch, cfg=cfg, M=M, opt=np.concatenate([rec['theta'], xi]), y=y, atoms=atoms, image=img)
    return out


@pytest.mark.parametrize('layout', list(LAYOUTS))
def test_point_evaluations_within_derived_bounds(blob, layout):
    """psi (both evaluators), the gradient and the theta block of the Hessian at: the constant term alone, c = 0 (every t = 0), +-1,
    +-40 / min|y| (1 + u rounds to 1 on every pixel of one sign), +-800 / min|y| (every pixel beyond the guard); the kernel's own optimum;
    perturbations of it with xi scaled by 1e-3, 1 and 1e3."""
    s = blob[layout]
    y, M = s['y'], s['M']
    ymin = float(np.abs(y).min())
    rng = np.random.default_rng(3)
    points = {}
    for c in (0.0, 1.0, -1.0, 40 / ymin, -40 / ymin, 800 / ymin, -800 / ymin):
        p = np.zeros(6 + M)
        p[5] = c
        points[f'c = {c:g}'] = p
    points['optimum'] = s['opt']
    for scale in (1e-3, 1.0, 1e3):
        p = s['opt'].copy()
        p[:6] *= 1 + 0.01 * rng.standard_normal(6)
        if M:
            p[6:] = scale * (p[6:] + np.abs(p[6:]).mean() * rng.standard_normal(M))
        points[f'perturbed, xi x {scale:g}'] = p
    worst = {}
    for name, p in points.items():
        res = _compare(f'{layout}: {name}', s['batch'], 0, p, y, s['atoms'], [1], s['cfg'], M)
        print(f'{layout}, {name}: ' + ', '.join(f'{k} {v:.3f}' for k, v in res.items()))
        for k, v in res.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f'{layout}: worst error / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1, worst


def test_golden_points_within_derived_bounds(gpu):
    """The 21 points of tests/golden/energy.npz (the scene and set-up of test_point_evaluations_match_reference_energy, which holds them
    to the reference's float64 values at 1e-10) against the extended-precision energy, to the derived bounds."""
    import json
    import os
    from superdsm_amd import engine
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'energy.npz'))
    cfg0 = json.loads(str(d['cfg']))
    y, atoms = d['y'], d['atoms']
    img = engine.DeviceImage(y, None, atoms, cfg0['background_margin'])
    worst = {}
    for k in range(int(d['n_cases'])):
        deform = bool(d[f'c{k}_deform'])
        cfg = dict(cfg0, alpha=float(d[f'c{k}_alpha']), smooth_amount=cfg0['smooth_amount'] if deform else np.inf, init='elliptical', max_iters=1)
        fp = d[f'c{k}_fp'].tolist()
        batch = engine.Batch(img, [fp], cfg)
        batch.launch()
        p = d[f'c{k}_params']
        res = _compare(f'golden: case {k}', batch, 0, p, y, atoms, fp, cfg, p.size - 6)
        print(f'golden case {k} (M = {p.size - 6}): ' + ', '.join(f'{q} {v:.3f}' for q, v in res.items()))
        for q, v in res.items():
            worst[q] = max(worst.get(q, 0.0), v)
    print('golden points: worst error / bound: ' + ', '.join(f'{q} {v:.3f}' for q, v in worst.items()))
    assert max(worst.values()) <= 1, worst
