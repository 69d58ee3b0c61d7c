"""What the GPU tests of the loss arithmetic stand on, without a GPU: the table of log_w (sdsm_logtab.h) is what its generator prints and
what its comment says, entry by entry (mpmath); the np.longdouble references of superdsm_amd/testing.py agree with mpmath; the
extended-precision energy agrees with the reference's float64 values of tests/golden/energy.npz."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from superdsm_amd import testing as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'superdsm_amd', 'csrc', 'sdsm_logtab.h')
mp = pytest.importorskip('mpmath')
mp.mp.prec = 256

needs_extended = pytest.mark.skipif(not T.longdouble_is_extended(), reason='np.longdouble has fewer than 64 significand bits here')


def test_generator_reproduces_the_header(tmp_path):
    """tools/gen_logtab.c, built with the C compiler of oracle/Makefile (CC, default gcc), prints sdsm_logtab.h byte for byte."""
    exe = str(tmp_path / 'gen_logtab')
    subprocess.check_call([os.environ.get('CC', 'gcc'), '-O2', '-o', exe, os.path.join(ROOT, 'tools', 'gen_logtab.c'), '-lm'])
    out = subprocess.check_output([exe])
    assert out == open(HEADER, 'rb').read()
    first = out.decode().splitlines()[0]
    assert 'ROUNDED' in first and 'log(1 / ic_j)' in first and 'log(c_j)' not in first      # the comment says what the table holds


def _table():
    text = open(HEADER).read()
    body = text[text.index('{', text.index('sdsm_logtab[')) + 1:text.rindex('}')]
    vals = [float.fromhex(tok) for tok in re.findall(r'-?0x[0-9a-f.]+p[+-]?\d+', body)]
    assert len(vals) == 130
    return np.array(vals).reshape(65, 2)


def _is_correctly_rounded(x, exact):
    """x is a double nearest to the mpmath number ``exact`` (no other double is strictly nearer)."""
    e = abs(mp.mpf(x) - exact)
    return e <= abs(mp.mpf(float(np.nextafter(x, np.inf))) - exact) and e <= abs(mp.mpf(float(np.nextafter(x, -np.inf))) - exact)


def test_table_entries():
    tab = _table()
    assert tab[0, 0] == 1.0 and tab[0, 1] == 0.0                                     # w = 1 gives exactly 0
    for j in range(65):
        ic, lc = float(tab[j, 0]), float(tab[j, 1])
        assert ic == 1.0 / (1.0 + j / 64.0), j                                       # 1 / c_j, rounded once
        if j:
            assert _is_correctly_rounded(lc, mp.log(1 / mp.mpf(ic))), j              # the logarithm of the reciprocal of THAT value
    assert tab[64, 0] == 0.5 and _is_correctly_rounded(float(tab[64, 1]), mp.log(2)) and float(tab[64, 1]) == float.fromhex('0x1.62e42fefa39efp-1')
    # the degree-7 series leans on |s| = |w ic_j - 1| <= 1 / 128 (+ the rounding of ic_j) over bin j, whose ends are the bin edges
    worst = mp.mpf(0)
    for j in range(65):
        for e in (j - 0.5, j + 0.5):
            if 0 <= e <= 64:
                worst = max(worst, abs((1 + mp.mpf(e) / 64) * mp.mpf(float(tab[j, 0])) - 1))
    assert worst <= mp.mpf(1) / 128 + mp.mpf(2) ** -52, worst
    # the bin the kernel takes, from the high word of w = fl(1 + u): ((hi - 0x3ff00000 + 0x2000) >> 14) = floor(64 (w - 1) + 1 / 2), at
    # every table point and bin edge and their neighbouring doubles
    pts, edges = T.loss_table_points()
    for w in 1.0 + T.ulp_neighbours(np.concatenate([pts, edges]), 2):
        if 1 <= w <= 2:
            hi = int(np.float64(w).view(np.uint64)) >> 32
            assert (hi - 0x3ff00000 + 0x2000) >> 14 == int(mp.floor(64 * (mp.mpf(float(w)) - 1) + mp.mpf(0.5))), w


def _sample():
    """At most 2000 of the probe's inputs: a regular sample of the whole list (its exact cases come first) and the hand-picked ones."""
    inp = T.loss_probe_inputs()
    with np.errstate(all='ignore'):
        t = inp['y'] * inp['S']
    pick = np.unique(np.linspace(0, t.size - 1, 1900).astype(int))
    t, y = t[pick], inp['y'][pick]
    extra = np.array([0.0, -0.0, 2.0 ** -1074, -2.0 ** -1074, 750.0, -750.0, 1e300, -1e300, 36.7, -36.7, 708.5, -745.0])
    t, y = np.concatenate([t, extra]), np.concatenate([y, np.full(extra.size, 0.75)])
    fin = np.isfinite(t)
    return t[fin], y[fin]


@needs_extended
def test_longdouble_references_against_mpmath():
    """exp, softplus, theta, kappa, r, dcurv and the logarithm of the references, to 2^-60 relative (longdouble carries 2^-64 per
    operation).  Below longdouble's normal range (exp(-1e300)) the reference may underflow: it must then be tiny itself."""
    t, y = _sample()
    assert 1000 < t.size <= 2000
    ref = T.loss_reference(t, y)
    tol, tiny = mp.mpf(2) ** -60, mp.mpf(2) ** -16382
    to_mp = lambda v: mp.mpf(int(np.frexp(v)[0] * np.longdouble(2) ** 64)) * mp.mpf(2) ** (int(np.frexp(v)[1]) - 64)     # exact
    worst = mp.mpf(0)

    def check(name, got, exact, k):
        nonlocal worst
        got = to_mp(got)
        if abs(exact) < tiny:
            assert abs(got) <= tiny, (name, t[k])
            return
        err = abs(got - exact) / abs(exact)
        worst = max(worst, err)
        assert err <= tol, (name, float(t[k]), float(err))

    for k in range(t.size):
        tk, yk = mp.mpf(float(t[k])), mp.mpf(float(y[k]))
        E = mp.exp(-abs(tk))
        check('E', ref['E'][k], mp.exp(-min(abs(tk), 750)), k)
        check('softplus', ref['softplus'][k], max(-tk, 0) + mp.log1p(E), k)
        theta = E / (1 + E) if tk >= 0 else 1 / (1 + E)
        check('theta', ref['theta'][k], theta, k)
        check('kappa', ref['kappa'][k], E / (1 + E) ** 2, k)
        check('r', ref['r'][k], -yk * theta, k)
        check('dcurv', ref['dcurv'][k], yk * yk * E / (1 + E) ** 2, k)
    pts, edges = T.loss_table_points()
    w = 1.0 + T.ulp_neighbours(np.concatenate([pts, edges]), 2)
    w = w[(w >= 1) & (w <= 2)]
    lw = T.log_reference(w)
    for k in range(w.size):
        check('log', lw[k], mp.log(mp.mpf(float(w[k]))), k % t.size)
    print(f'np.longdouble references against mpmath: worst relative error 2^{float(mp.log(worst, 2)):.1f}')


@needs_extended
def test_energy_reference_matches_the_golden_points():
    """testing.energy_reference (np.longdouble; the oracle's region and G~) at the 21 points of energy.npz, to the fixture's 1e-10:
    value, gradient and the theta block of the Hessian of the reference's Energy."""
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'energy.npz'))
    cfg0 = json.loads(str(d['cfg']))
    y, atoms = d['y'], d['atoms']
    n_guard = 0
    for k in range(int(d['n_cases'])):
        deform = bool(d[f'c{k}_deform'])
        cfg = dict(cfg0, alpha=float(d[f'c{k}_alpha']), smooth_amount=cfg0['smooth_amount'] if deform else np.inf)
        p = d[f'c{k}_params']
        ref = T.energy_reference(y, None, atoms, d[f'c{k}_fp'].tolist(), cfg, p[:6], p[6:] if deform else None)
        assert ref['M'] + 6 == p.size
        val, grad, H = float(d[f'c{k}_value']), d[f'c{k}_grad'], d[f'c{k}_hessian_lower']
        n_guard += int(d[f'c{k}_n_guarded'])
        assert abs(float(ref['psi']) - val) <= 1e-10 * abs(val), (k, ref['psi'], val)
        np.testing.assert_allclose(ref['grad'].astype(np.float64), grad, rtol=1e-10, atol=1e-10 * np.abs(grad).max())
        # (the reference's kappa = theta - theta^2 cancels as theta -> 1: the tolerance of the GPU test of the same fixture)
        sel = np.isin(atoms, d[f'c{k}_fp'])
        np.testing.assert_allclose(np.tril(ref['hess_theta'].astype(np.float64)), H[:6, :6], rtol=1e-9, atol=4e-13 * float((y[sel] ** 2).sum()))
        # the local frame is a change of basis: S is the same in both
        assert np.all(ref['A'] >= np.abs(ref['t'] / np.where(ref['y'] == 0, 1, ref['y'])) * (1 - 1e-15))
    assert n_guard > 0
