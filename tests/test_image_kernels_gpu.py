"""The per-image kernels of sdsm_prepare.hip -- separable Gaussian filters, preprocessing, bounded EDT, atom statistics -- against
SciPy on every implementation they choose between.  Needs an MI355X.

Which kernel runs is decided on the host by the filter radius R = int(4 sigma + 0.5) and the LDS budgets (`separable2d`,
`tiled_fits`, `launch_bounded_edt`); `col_kernel`, `row_kernel`, `preprocess_fused` and `edt_path` below restate that choice, and
tests/test_image_kernels_cpu.py checks that the case lists of this module reach every one of them.

Bit for bit: the kernels accumulate in SciPy's association order (centre tap, then the pairs from the outermost inwards, unfused
multiply and add), so with the same weights they equal `scipy.ndimage.correlate1d(mode='reflect')` along axis 0 and then axis 1
exactly.  The library computes its Gaussian weights with libm's `exp`, which differs from numpy's in the last bit now and then:
comparisons with the library's weights (read through `sdsm_gauss_kernel_host`, a host function) are exact, the comparison with
`ndi.gaussian_filter` itself is held to an error bound.
"""
import ctypes as C
import functools
import math
import zlib

import numpy as np
import pytest
import scipy.ndimage as ndi
from scipy.ndimage._filters import _gaussian_kernel1d

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps

# ---------------------------------------------------------------------------------------------------------
# restatement of the host-side dispatch of sdsm_prepare.hip
# ---------------------------------------------------------------------------------------------------------
GT_K, GT_LDS_MAX, LDS_LIMIT = 8, 64 * 1024, 160 * 1024 - 1024     # register-tiled kernels' budget; plain kernels' budget
GC_ROWS, GR_ROWS, GR_COLS = 64, 8, 32 * 8
EDT_BITS_MAX_RADIUS = 63


def gauss_radius(sigma):
    return int(4.0 * sigma + 0.5)


def col_kernel(R):
    """Kernel of the axis-0 pass for radius R (None: the filter is refused)."""
    if (8 * GT_K + 2 * R + 1) * 32 * 8 <= GT_LDS_MAX:
        return 'cols_t<32>'
    if (16 * GT_K + 2 * R + 1) * 16 * 8 <= GT_LDS_MAX:
        return 'cols_t<16>'
    if (GC_ROWS + 2 * R) * 32 * 8 <= LDS_LIMIT:
        return 'cols<32>'
    if (GC_ROWS + 2 * R) * 8 * 8 <= LDS_LIMIT:
        return 'cols<8>'
    return None


def row_kernel(R):
    """Kernel of the axis-1 pass for radius R (None: the filter is refused)."""
    span = GR_COLS + 2 * R + 1
    if GR_ROWS * (span + (span >> 3) + 1) * 8 <= GT_LDS_MAX:
        return 'rows_t'
    if (256 + 2 * R) * 8 <= LDS_LIMIT:
        return 'rows'
    return None


def preprocess_fused(sigma1, sigma2):
    """sdsm_preprocess clips on load and combines in the last pass only when both filters fit the register-tiled kernels."""
    return all(col_kernel(R) in ('cols_t<32>', 'cols_t<16>') and row_kernel(R) == 'rows_t' for R in (gauss_radius(sigma1), gauss_radius(sigma2)))


def edt_path(margin):
    """Bounded EDT of radius ceil(margin): ballot / bit-word kernels up to 63, the byte-mask kernels above."""
    return 'bits' if max(int(math.ceil(margin)), 0) <= EDT_BITS_MAX_RADIUS else 'bytes'


# ---------------------------------------------------------------------------------------------------------
# plain CPU references
# ---------------------------------------------------------------------------------------------------------
def reflect_index(i, n):
    """scipy.ndimage's 'reflect' boundary (d c b a | a b c d | d c b a), for any distance outside the line."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def correlate_restated(x, w, axis):
    """Symmetric correlation in SciPy's association order: x[i] w[R], then + (x[i - j] + x[i + j]) w[R - j] for j = R .. 1."""
    x = np.moveaxis(np.asarray(x, np.float64), axis, 0)
    n, R = x.shape[0], len(w) // 2
    i = np.arange(n)
    acc = x * w[R]
    for j in range(R, 0, -1):
        acc = acc + (x[reflect_index(i - j, n)] + x[reflect_index(i + j, n)]) * w[R - j]
    return np.moveaxis(acc, 0, axis)


def separable_ref(x, w0, w1):
    """axis 0 with w0, then axis 1 with w1 (scipy.ndimage's order of the axes)."""
    return ndi.correlate1d(ndi.correlate1d(x, w0, axis=0, mode='reflect'), w1, axis=1, mode='reflect')


def scipy_weights(R, order):
    """SciPy's own taps of radius R (sigma = (R + 0.25) / 4, so that int(4 sigma + 0.5) == R), reversed as gaussian_filter uses them."""
    return np.ascontiguousarray(_gaussian_kernel1d((R + 0.25) / 4.0, order, R)[::-1])


def library_weights(sigma):
    """The taps libsdsm_hip.so filters with (sdsm_gauss_kernel_host: host code, no GPU)."""
    from superdsm_amd import _capi
    fn = _capi.lib().sdsm_gauss_kernel_host
    fn.restype, fn.argtypes = None, [C.c_double, C.c_int, C.c_void_p]
    R = gauss_radius(sigma)
    w = np.empty(2 * R + 1)
    fn(float(sigma), R, w.ctypes.data_as(C.c_void_p))
    return w


def gauss_lib(x, sigma):
    w = library_weights(sigma)
    return separable_ref(x, w, w)


def preprocess_ref(g, sigma1, sigma2, offset_clip, lower_clip_mean):
    """Preprocessing.process (superdsm/preprocess.py:46-64) as synth.offset_image states it, with the library's weights."""
    off = gauss_lib(g, sigma2)
    if math.isinf(offset_clip):
        comb = off
    else:
        clip_abs = offset_clip * g.std()
        offc = gauss_lib(g.clip(0, clip_abs), sigma2)
        t = ndi.distance_transform_edt(~(g > clip_abs))
        t = (sigma2 - t).clip(0, np.inf)
        t = (t / t.max()) ** 2
        comb = (1 - t) * offc + t * off
    if lower_clip_mean:
        comb = np.maximum(comb, g.mean())
    return gauss_lib(g, sigma1) - comb


# ---------------------------------------------------------------------------------------------------------
# inputs (one per shape and kind, reused by the cases: read only)
# ---------------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode())


@functools.lru_cache(maxsize=None)
def wide_range_input(shape):
    """normal * exp(uniform(-5, 5)): a dropped or doubled tap cannot hide below the others."""
    rng = np.random.default_rng(_seed('wide', shape))
    return rng.standard_normal(shape) * np.exp(rng.uniform(-5, 5, shape))


def _blobs(shape, rng, n=12):
    """Noise plus bright blobs: a few per cent of the pixels lie above 3 std (the clipped area of the preprocessing)."""
    g = 0.05 * rng.standard_normal(shape)
    rr = np.arange(shape[0])[:, None]
    cc = np.arange(shape[1])[None, :]
    for _ in range(n):
        r0, c0, a = rng.uniform(0, shape[0]), rng.uniform(0, shape[1]), rng.uniform(2, min(40, max(shape) / 8))
        g = g + rng.uniform(0.2, 3) * np.exp(-0.5 * (rr - r0) ** 2 / (a * a)) * np.exp(-0.5 * (cc - c0) ** 2 / (a * a))
    return g


@functools.lru_cache(maxsize=None)
def preprocess_input(shape, kind):
    """'generic': real-valued.  'dyadic': multiples of 2^-10 whose mean is one too, so that the sums behind mean and std are exact in
    any order and the GPU's reduction tree must give numpy's mean and std bit for bit."""
    rng = np.random.default_rng(_seed('preprocess', shape, kind))
    g = _blobs(shape, rng)
    if kind == 'dyadic':
        q = np.round(g * 1024).ravel()
        n = q.size
        d = int(round(q.sum() / n)) * n - int(q.sum())                    # move the integer sum onto a multiple of n
        q[rng.choice(n, abs(d), replace=False)] += np.sign(d)
        g = q.reshape(shape) / 1024
    return g


# ---------------------------------------------------------------------------------------------------------
# GPU calls through the C ABI
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    from superdsm_amd import _capi
    _capi.lib()     # fails loudly if libsdsm_hip.so is missing
    return torch


def separable_gpu(torch, x, w0, w1, out=None):
    """sdsm_separable_filter(x, w0 along axis 0, w1 along axis 1) on the current stream; `out`: a device tensor to write."""
    from superdsm_amd import _capi
    L = _capi.lib()
    H, W = x.shape
    R0, R1 = len(w0) // 2, len(w1) // 2
    d_in = torch.as_tensor(np.ascontiguousarray(x, np.float64)).cuda()
    if out is None:
        out = torch.full_like(d_in, np.nan)
    nbytes = L.sdsm_separable_workspace_bytes(H, W, R0, R1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d_in.device)
    hp = lambda w: w.ctypes.data_as(C.c_void_p)
    dp = lambda t: C.c_void_p(t.data_ptr())
    _capi.check(L.sdsm_separable_filter(dp(d_in), H, W, hp(w0), R0, hp(w1), R1, dp(out), dp(ws), nbytes,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'sdsm_separable_filter')
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------
# 1. separable filter with SciPy's own weights: bit for bit
# ---------------------------------------------------------------------------------------------------------
# (shape, R0, R1): R0 picks the axis-0 kernel, R1 the axis-1 kernel (see col_kernel / row_kernel)
SEPARABLE_CASES = [
    ((1, 1), 0, 0), ((1, 1), 7, 327), ((1, 1), 1240, 9),
    ((1, 300), 1, 8), ((1, 300), 96, 287), ((1, 300), 327, 95),
    ((300, 1), 8, 1), ((300, 1), 287, 96), ((300, 1), 191, 326),
    ((7, 5), 9, 7), ((7, 5), 95, 191), ((7, 5), 192, 286), ((7, 5), 326, 327), ((7, 5), 1240, 1240),     # R beyond the image
    ((64, 256), 0, 1), ((64, 256), 7, 9), ((64, 256), 96, 191), ((64, 256), 286, 192),
    ((65, 257), 1, 0), ((65, 257), 9, 8), ((65, 257), 95, 96), ((65, 257), 192, 326), ((65, 257), 287, 327), ((65, 257), 1240, 3),
    ((129, 513), 3, 13), ((129, 513), 21, 45), ((129, 513), 191, 192), ((129, 513), 327, 286), ((129, 513), 1239, 1241),
    ((520, 696), 6, 6), ((520, 696), 170, 170), ((520, 696), 192, 95), ((520, 696), 326, 287),
    ((1024, 1024), 12, 5), ((1024, 1024), 96, 160), ((1024, 1024), 287, 327),
]


def _sep_id(case):
    shape, R0, R1 = case
    return f'{shape[0]}x{shape[1]}-R{R0}:{col_kernel(R0)}-R{R1}:{row_kernel(R1)}'


@pytest.mark.parametrize('case', SEPARABLE_CASES, ids=_sep_id)
def test_separable_filter_bit_exact(gpu, case):
    shape, R0, R1 = case
    x = wide_range_input(shape)
    for w0, w1 in ((scipy_weights(R0, 0), scipy_weights(R1, 2)), (scipy_weights(R0, 2), scipy_weights(R1, 0))):
        np.testing.assert_array_equal(separable_gpu(gpu, x, w0, w1), separable_ref(x, w0, w1))


# ---------------------------------------------------------------------------------------------------------
# 2. gaussian_filter_gpu: exact with the library's weights, within 4 eps of ndi.gaussian_filter
# ---------------------------------------------------------------------------------------------------------
GAUSSIAN_CASES = [(3, (1024, 1024)), (23.75, (520, 696)), (23.9, (520, 696)), (42.43, (129, 513)), (47.9, (520, 696)),
                  (71.7, (65, 257)), (81.7, (129, 513)), (150, (300, 257))]


@pytest.mark.parametrize('sigma,shape', GAUSSIAN_CASES,
                         ids=[f'sigma{s}-R{gauss_radius(s)}:{col_kernel(gauss_radius(s))}:{row_kernel(gauss_radius(s))}' for s, _ in GAUSSIAN_CASES])
def test_gaussian_filter(gpu, sigma, shape):
    from superdsm_amd import postprocess
    x = wide_range_input(shape)
    got = postprocess.gaussian_filter_gpu(gpu.as_tensor(x).cuda(), sigma).cpu().numpy()
    np.testing.assert_array_equal(got, gauss_lib(x, sigma))
    # SciPy's own weights differ from libm's in the last bits: at most a few eps of the filtered magnitude
    assert (np.abs(got - ndi.gaussian_filter(x, sigma)) <= 4 * EPS * ndi.gaussian_filter(np.abs(x), sigma)).all()


# ---------------------------------------------------------------------------------------------------------
# 3. engine.preprocess on the fused and the unfused path
# ---------------------------------------------------------------------------------------------------------
# (shape, sigma2, offset_clip, lower_clip_mean, input kind); sigma1 = sqrt(2) (R = 6).  sigma2 > 47.875 (R > 191) is unfused;
# ceil(sigma2) is the EDT radius (63: bit kernels, 63.5 and above: byte kernels)
PREPROCESS_CASES = [
    ((520, 696), 10, 3, False, 'dyadic'), ((520, 696), 40, 3, True, 'generic'), ((1024, 1024), 24, 3, False, 'generic'),
    ((1344, 1024), 42.43, 3, False, 'dyadic'), ((1344, 1024), 40, np.inf, False, 'generic'), ((520, 696), 42.43, np.inf, False, 'dyadic'),
    ((520, 696), 47.9, 3, False, 'dyadic'), ((520, 696), 63, 3, True, 'dyadic'), ((520, 696), 63.5, 3, False, 'generic'),
    ((1024, 1024), 75, 3, False, 'dyadic'), ((1024, 1024), 63, np.inf, True, 'generic'), ((520, 696), 90, np.inf, True, 'generic'),
    ((520, 696), 90, 3, False, 'dyadic'), ((1, 700), 24, 3, True, 'generic'), ((1, 700), 63.5, 3, False, 'dyadic'),
    ((700, 1), 10, 3, False, 'dyadic'), ((700, 1), 75, np.inf, False, 'generic'), ((50, 40), 47.9, 3, True, 'generic'),
    ((50, 40), 90, 3, False, 'dyadic'), ((50, 40), 10, np.inf, True, 'dyadic'),
]


def _pre_id(case):
    shape, s2, clip, lcm, kind = case
    R2 = gauss_radius(s2)
    return (f'{shape[0]}x{shape[1]}-sigma{s2}-{"fused" if preprocess_fused(math.sqrt(2), s2) else "unfused"}-{col_kernel(R2)}-{row_kernel(R2)}'
            f'-edt_{edt_path(s2)}-clip{clip}-lcm{int(lcm)}-{kind}')


@pytest.mark.parametrize('case', PREPROCESS_CASES, ids=_pre_id)
def test_preprocess(gpu, case):
    from superdsm_amd import engine
    shape, sigma2, offset_clip, lower_clip_mean, kind = case
    g = preprocess_input(shape, kind)
    sigma1 = math.sqrt(2)
    if not math.isinf(offset_clip):
        clip_abs = offset_clip * g.std()
        assert (np.abs(g - clip_abs) > 1e-9 * clip_abs).all()          # the clipped area does not hang on the last bit of std
        assert 0 < (g > clip_abs).sum() < g.size
    y = engine.preprocess(g, sigma1, sigma2, offset_clip, lower_clip_mean)
    ref = preprocess_ref(g, sigma1, sigma2, offset_clip, lower_clip_mean)
    uses_reductions = not math.isinf(offset_clip) or lower_clip_mean
    if kind == 'dyadic':
        # the sums of mean and std are exact: nothing may differ
        assert math.fsum(g.ravel()) == g.sum() and math.fsum(((g - g.mean()) ** 2).ravel()) == ((g - g.mean()) ** 2).sum()
    if kind == 'dyadic' or not uses_reductions:
        np.testing.assert_array_equal(y, ref)
    else:
        # mean and std come from a different summation order than numpy's: y to 2 ulp of the image's magnitude
        np.testing.assert_allclose(y, ref, rtol=0, atol=2 * EPS * np.abs(g).max())


# ---------------------------------------------------------------------------------------------------------
# 4. bounded EDT and atom statistics (engine.DeviceImage)
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edt_scene(shape, targets):
    """y (targets: y > 0), y_mask, atoms.  targets: 'random' (sparse: nearest target up to ~100 away), 'all', 'none' or
    ('single', r, c).  Non-targets are y <= 0 incl. 0 and -0; a subnormal positive value is a target."""
    H, W = shape
    rng = np.random.default_rng(_seed('edt', shape, targets))
    y = -rng.uniform(0, 1, shape)
    y[rng.uniform(size=shape) < 0.01] = 0.0
    y[rng.uniform(size=shape) < 0.01] = -0.0
    if targets == 'random':
        k = max(1, H * W // 12000)
        t = rng.choice(H * W, k, replace=False)
        y.ravel()[t] = rng.uniform(0, 1, k)
        y.ravel()[t[::7]] = 5e-324
        if H * W >= 4:                                                    # a small cluster: distances 0 .. 1 around it
            y[H // 2:H // 2 + 2, W // 3:W // 3 + 2] = 1.0
    elif targets == 'all':
        y = rng.uniform(0, 1, shape)
        y.ravel()[::5] = 5e-324
    elif targets != 'none':
        _, r, c = targets
        y[r, c] = 1.0
    y_mask = rng.uniform(size=shape) < 0.9
    # atoms: cells of 8 x 9 pixels (> 256 labels on the larger images), a tenth of the labels absent, label 0 here and there,
    # and a band of per-pixel random labels (many labels per wavefront of k_stats)
    atoms = (np.arange(H)[:, None] // 8) * ((W + 8) // 9) + np.arange(W)[None, :] // 9 + 1
    n = int(atoms.max())
    absent = rng.choice(np.arange(1, n + 1), max(1, n // 10), replace=False)
    atoms[np.isin(atoms, absent)] = 0
    band = min(H, 5)
    atoms[:band] = rng.integers(0, n + 1, (band, W))
    atoms[-1, -1] = n + 3                                                  # the largest label
    return y, y_mask, atoms.astype(np.int32)


# (shape, targets, margin, with y_mask)
EDT_CASES = (
    [((2, 2), 'random', m, True) for m in (0.5, 1, 100)]
    + [((2, 700), 'random', m, False) for m in (2.5, 63, 64)]
    + [((700, 2), 'random', m, True) for m in (8, 62.5, 63.01)]
    + [((300, 257), 'random', m, m != 8) for m in (0.5, 1, 2.5, 8, 62.5, 63, 63.01, 64, 100)]
    + [((520, 696), 'random', m, True) for m in (8, 63, 63.01, 100)]
    + [((1024, 1024), 'random', m, True) for m in (2.5, 62.5, 64, 100)]
    + [((2, 2), 'none', 1, True), ((300, 257), 'none', 8, True), ((300, 257), 'none', 100, False), ((2, 700), 'none', 63, True),
       ((700, 2), 'none', 64, True), ((520, 696), 'none', 0.5, True)]
    + [((2, 700), 'all', 0.5, True), ((300, 257), 'all', 63, True), ((300, 257), 'all', 100, True)]
    # one target whose nearest pixels lie in another 64-column word / 256-column block / 64-row tile
    + [((300, 600), ('single', r, c), m, True) for (r, c) in ((63, 63), (64, 64), (127, 255), (128, 256), (191, 257))
       for m in (62.5, 63, 100)]
)


def _edt_id(case):
    shape, targets, margin, with_mask = case
    t = targets if isinstance(targets, str) else f'at{targets[1]},{targets[2]}'
    return f'{shape[0]}x{shape[1]}-{t}-margin{margin}-{edt_path(margin)}{"-mask" if with_mask else ""}'


@pytest.mark.parametrize('case', EDT_CASES, ids=_edt_id)
def test_bounded_edt_and_atom_stats(gpu, case):
    from superdsm_amd import engine
    shape, targets, margin, with_mask = case
    y, y_mask, atoms = edt_scene(shape, targets)
    img = engine.DeviceImage(y, y_mask if with_mask else None, atoms, margin)
    d2 = np.round(ndi.distance_transform_edt(y <= 0) ** 2)               # with no target at all: SciPy's virtual pixel at (-1, 0)
    expect = (d2 <= margin * margin) & (y_mask if with_mask else True)
    np.testing.assert_array_equal(img.valid.cpu().numpy().astype(bool), expect)
    n = int(atoms.max())
    assert img.n_atoms == n
    stats = img.atom_stats.reshape(-1, 6)
    lab = np.where(expect & (atoms > 0), atoms, 0)
    area = np.bincount(lab.ravel(), minlength=n + 1)
    np.testing.assert_array_equal(stats[1:, 0], area[1:])
    boxes = ndi.find_objects(lab, max_label=n)
    for l, box in enumerate(boxes, start=1):
        if box is not None:
            assert tuple(stats[l, 1:5]) == (box[0].start, box[0].stop - 1, box[1].start, box[1].stop - 1), l


# ---------------------------------------------------------------------------------------------------------
# 5. the radius limits of sdsm_separable_filter
# ---------------------------------------------------------------------------------------------------------
def test_radius_limits(gpu):
    from superdsm_amd import _capi
    x = wide_range_input((40, 50))
    weights = lambda R0, R1: (scipy_weights(R0, 0), scipy_weights(R1, 0))
    for R0, R1 in ((1240, 7), (7, 10048)):                                # the longest filters of the two passes
        w0, w1 = weights(R0, R1)
        np.testing.assert_array_equal(separable_gpu(gpu, x, w0, w1), separable_ref(x, w0, w1))
    for R0, R1, what in ((1241, 7, 'column pass'), (7, 10049, 'row pass')):
        w0, w1 = weights(R0, R1)
        out = gpu.full(x.shape, 7.0, dtype=gpu.float64, device='cuda')
        with pytest.raises(_capi.SdsmError, match='1240 for the column pass and 10048 for the row pass'):
            separable_gpu(gpu, x, w0, w1, out=out)
        gpu.cuda.synchronize()
        assert (out.cpu().numpy() == 7.0).all(), what                     # refused before anything was launched
    w0, w1 = weights(30, 40)                                                   # the stream goes on as before
    np.testing.assert_array_equal(separable_gpu(gpu, x, w0, w1), separable_ref(x, w0, w1))
