"""CPU-side pins of tests/test_image_kernels_gpu.py: the library's Gaussian weights, the association order the GPU comparisons rely
on, and the restated dispatch of sdsm_prepare.hip with the coverage of the GPU case lists.  No GPU needed."""
import math
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi
from scipy.ndimage._filters import _gaussian_kernel1d

import test_image_kernels_gpu as gk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGMAS = sorted({0.3, 1.0, math.sqrt(2), 141.4} | {s for s, _ in gk.GAUSSIAN_CASES} | {c[1] for c in gk.PREPROCESS_CASES})


@pytest.mark.parametrize('sigma', SIGMAS)
def test_library_weights_are_symmetric_and_scipys_to_the_last_bits(sigma):
    """sdsm_gauss_kernel_host restates _gaussian_kernel1d with libm's exp: the exponentials differ from numpy's by at most 1 ulp,
    which the normalisation by their sum can carry to 2 ulp of a tap."""
    w = gk.library_weights(sigma)
    R = gk.gauss_radius(sigma)
    assert len(w) == 2 * R + 1
    np.testing.assert_array_equal(w, w[::-1])
    ref = _gaussian_kernel1d(sigma, 0, R)
    assert (np.abs(w - ref) <= 2 * np.spacing(ref)).all()
    assert abs(w.sum() - 1) <= 4 * gk.EPS


@pytest.mark.parametrize('shape,R', [((1, 1), 0), ((1, 1), 40), ((1, 3), 1240), ((7, 5), 9), ((7, 5), 23), ((40, 33), 77), ((64, 70), 8)])
def test_association_order_restatement_equals_correlate1d(shape, R):
    """The order the kernels accumulate in (centre, then the pairs from the outermost inwards, reflect boundary, any R) is
    correlate1d's, bit for bit: what the GPU tests compare against is that order and nothing looser."""
    rng = np.random.default_rng(R)
    x = rng.standard_normal(shape) * np.exp(rng.uniform(-5, 5, shape))
    for order in (0, 2):
        w = gk.scipy_weights(R, order)
        for axis in (0, 1):
            np.testing.assert_array_equal(gk.correlate_restated(x, w, axis), ndi.correlate1d(x, w, axis=axis, mode='reflect'))


def test_dispatch_restatement_follows_the_source():
    """The budgets restated in the GPU module are the ones sdsm_prepare.hip dispatches on."""
    src = open(os.path.join(ROOT, 'superdsm_amd', 'csrc', 'sdsm_prepare.hip')).read()
    define = lambda name: re.search(rf'#define {name} (.+)', src).group(1).split('//')[0].strip()
    assert int(define('GT_K')) == gk.GT_K
    assert eval(define('GT_LDS_MAX')) == gk.GT_LDS_MAX
    assert int(define('GC_ROWS')) == gk.GC_ROWS and int(define('GR_ROWS')) == gk.GR_ROWS
    assert define('GR_COLS') == '(32 * GT_K)' and gk.GR_COLS == 32 * gk.GT_K
    assert src.count('160 * 1024 - 1024') == 3 and gk.LDS_LIMIT == 160 * 1024 - 1024
    assert f'if (radius <= {gk.EDT_BITS_MAX_RADIUS}) {{' in src


# the dispatch table: first and last radius of every row
DISPATCH_TABLE = [((0, 95), 'cols_t<32>', 'rows_t'), ((96, 191), 'cols_t<16>', 'rows_t'), ((192, 286), 'cols<32>', 'rows_t'),
                  ((287, 326), 'cols<8>', 'rows_t'), ((327, 1240), 'cols<8>', 'rows'), ((1241, 10048), None, 'rows'), ((10049, 10049), None, None)]


def test_dispatch_table():
    for (lo, hi), col, row in DISPATCH_TABLE:
        for R in range(lo, hi + 1):
            assert (gk.col_kernel(R), gk.row_kernel(R)) == (col, row), R
    assert gk.preprocess_fused(math.sqrt(2), 47.87) and not gk.preprocess_fused(math.sqrt(2), 47.875)
    assert [gk.edt_path(m) for m in (0, 0.5, 62.5, 63, 63.01, 64)] == ['bits'] * 4 + ['bytes'] * 2


def test_gpu_cases_reach_every_path():
    """Every row of the table on both passes, next to both sides of every boundary; both preprocessing paths with both EDT
    paths under them; both EDT paths of the image preparation with and without targets."""
    sep = [(R0, R1) for _, R0, R1 in gk.SEPARABLE_CASES]
    assert {gk.col_kernel(R0) for R0, _ in sep} == {'cols_t<32>', 'cols_t<16>', 'cols<32>', 'cols<8>'}
    assert {gk.row_kernel(R1) for _, R1 in sep} == {'rows_t', 'rows'}
    radii = {R for pair in sep for R in pair}
    for R in (0, 1, 7, 8, 9, 95, 96, 191, 192, 286, 287, 326, 327, 1240):
        assert R in radii, R
    assert sum(R % 8 != 0 for R in radii) >= 10
    shapes = {s for s, _, _ in gk.SEPARABLE_CASES}
    assert {(1, 1), (1, 300), (300, 1), (7, 5), (64, 256), (65, 257), (129, 513), (520, 696), (1024, 1024)} <= shapes
    assert {(gk.col_kernel(gk.gauss_radius(s)), gk.row_kernel(gk.gauss_radius(s))) for s, _ in gk.GAUSSIAN_CASES} == \
        {(c, r) for _, c, r in DISPATCH_TABLE[:5]}
    pre = [(gk.preprocess_fused(math.sqrt(2), s2), gk.col_kernel(gk.gauss_radius(s2)), gk.row_kernel(gk.gauss_radius(s2)), gk.edt_path(s2), clip, lcm)
           for _, s2, clip, lcm, _ in gk.PREPROCESS_CASES]
    assert {p[:3] for p in pre} == {(True, 'cols_t<32>', 'rows_t'), (True, 'cols_t<16>', 'rows_t'), (False, 'cols<32>', 'rows_t'),
                                    (False, 'cols<8>', 'rows_t'), (False, 'cols<8>', 'rows')}
    assert {(p[0], p[3]) for p in pre if not math.isinf(p[4])} == {(True, 'bits'), (False, 'bits'), (False, 'bytes')}
    both = {(a, b) for a in (True, False) for b in (True, False)}
    assert {(p[0], math.isinf(p[4])) for p in pre} == both and {(p[0], p[5]) for p in pre} == both
    assert {s2 for _, s2, _, _, _ in gk.PREPROCESS_CASES} == {10, 24, 40, 42.43, 47.9, 63, 63.5, 75, 90}
    assert {s for s, *_ in gk.PREPROCESS_CASES} == {(520, 696), (1024, 1024), (1344, 1024), (1, 700), (700, 1), (50, 40)}
    edt = {(t if isinstance(t, str) else 'single', gk.edt_path(m)) for _, t, m, _ in gk.EDT_CASES}
    assert edt == {(t, p) for t in ('random', 'all', 'none', 'single') for p in ('bits', 'bytes')}
    assert {m for _, _, m, _ in gk.EDT_CASES} == {0.5, 1, 2.5, 8, 62.5, 63, 63.01, 64, 100}
    assert {t[2] for _, t, _, _ in gk.EDT_CASES if not isinstance(t, str)} == {63, 64, 255, 256, 257}
