"""The device determinant-of-Hessian detector of the scale estimation (sdsm_log_masks, sdsm_integral_image, sdsm_doh_cube,
sdsm_doh_peaks; automation._DohDevice / estimate_scales) against the host restatement in superdsm_amd/automation.py, bit for bit:
every comparison is exact.  Needs an MI355X."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    from superdsm_amd import _capi
    _capi.lib()     # fails loudly if libsdsm_hip.so is missing
    return torch


def sigmas():
    from superdsm_amd import automation
    return automation._sigma_list(20, 200, 10)


def disc_scene(H, W, r, seed, n=8):
    """The generator of test_gpu_parity's scale-estimation test: Gaussian-ish discs of radius r on noise."""
    rng = np.random.default_rng(seed)
    rr, cc = np.mgrid[:H, :W]
    im = 0.02 * rng.standard_normal((H, W))
    for _ in range(n):
        r0, c0 = rng.uniform(r, H - r), rng.uniform(r, W - r)
        im += np.exp(-(((rr - r0) ** 2 + (cc - c0) ** 2) / (r * r)) ** 2)
    return im


def bbbc039_image():
    """The raw image of testing.make_scene('bbbc039_like') (without the atoms and candidates of the scene)."""
    from superdsm_amd import synth
    spec = dict(synth.WORKLOADS['bbbc039_like'])
    shape, layout = synth.bbbc039_like_layout(spec['seed'], 0)
    return synth.render_image(shape, layout, spec['seed'])


def normalized(im):
    from superdsm_amd import automation
    im = automation.normalize_image(im)
    im /= im.max()
    return im


def p(t):
    return C.c_void_p(t.data_ptr())


def test_integral_image_is_numpys_cumsum(gpu):
    from superdsm_amd import _capi
    L = _capi.lib()
    stream = C.c_void_p(gpu.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    for shape in [(1, 1), (1, 97), (97, 1), (300, 380), (1024, 1344), (65, 130)]:
        im = rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)       # magnitudes that make the order of the sums matter
        want = im.cumsum(0).cumsum(1)
        d_im = gpu.as_tensor(im).cuda()
        d_ii = gpu.empty_like(d_im)
        _capi.check(L.sdsm_integral_image(p(d_im), shape[0], shape[1], p(d_ii), stream), 'sdsm_integral_image')
        np.testing.assert_array_equal(d_ii.cpu().numpy(), want, err_msg=str(shape))
        _capi.check(L.sdsm_integral_image(p(d_im), shape[0], shape[1], p(d_im), stream), 'sdsm_integral_image')     # in place
        np.testing.assert_array_equal(d_im.cpu().numpy(), want, err_msg=str(shape))


def test_log_masks_are_those_of_the_separable_filter(gpu):
    """sdsm_log_masks (all scales in one call, weights on the device) gives the masks that two sdsm_separable_filter calls per sigma
    and their sum's sign give -- what _log_negative_masks computed before it went through the detector."""
    from superdsm_amd import _capi, automation
    L = _capi.lib()
    stream = C.c_void_p(gpu.cuda.current_stream().cuda_stream)
    im = normalized(disc_scene(300, 380, 25, 1))
    H, W = im.shape
    got = automation._log_negative_masks(im, sigmas())
    d_in = gpu.as_tensor(im).cuda()
    a, b = gpu.empty_like(d_in), gpu.empty_like(d_in)
    radii, w = automation._log_weights(sigmas())
    off = 0
    for sigma, R in zip(sigmas(), radii):
        w0, w2 = np.ascontiguousarray(w[off:off + 2 * R + 1]), np.ascontiguousarray(w[off + 2 * R + 1:off + 4 * R + 2])
        off += 4 * R + 2
        nbytes = L.sdsm_separable_workspace_bytes(H, W, int(R), int(R))
        ws = gpu.empty(nbytes, dtype=gpu.uint8, device=d_in.device)
        hp = lambda x: x.ctypes.data_as(C.c_void_p)
        _capi.check(L.sdsm_separable_filter(p(d_in), H, W, hp(w2), int(R), hp(w0), int(R), p(a), p(ws), nbytes, stream), 'sdsm_separable_filter')
        _capi.check(L.sdsm_separable_filter(p(d_in), H, W, hp(w0), int(R), hp(w2), int(R), p(b), p(ws), nbytes, stream), 'sdsm_separable_filter')
        np.testing.assert_array_equal(got[sigma], ((a + b) < 0).cpu().numpy(), err_msg=str(sigma))
    assert sorted(got) == sorted(sigmas())


@pytest.mark.parametrize('shape', [(40, 50), (300, 380)])
def test_cube_slices_are_the_host_determinant(gpu, shape):
    """Every scale's slice of the cube against mask * _hessian_matrix_det(ii, sigma), masks from _log_negative_masks; at 40 x 50
    every window of the larger sigmas is clipped."""
    from superdsm_amd import automation
    im = normalized(disc_scene(shape[0], shape[1], min(shape) // 5, 2, n=3))
    masks = automation._log_negative_masks(im, sigmas())
    dev = automation._DohDevice(sigmas()).load(im)
    ii = im.cumsum(0).cumsum(1)
    np.testing.assert_array_equal(dev.integral_image(), ii)
    cube = dev.cube()
    assert cube.shape == (len(sigmas()),) + shape
    for k, s in enumerate(sigmas()):
        np.testing.assert_array_equal(cube[k], masks[s] * automation._hessian_matrix_det(ii, s), err_msg=str(s))
    assert any(0 < masks[s].mean() < 1 for s in sigmas())


def host_cube(im, sigma_list, masks):
    from superdsm_amd import automation
    ii = im.cumsum(0).cumsum(1)
    return np.dstack([masks[s] * automation._hessian_matrix_det(ii, s) for s in sigma_list])


def host_ordered_coords(cube, threshold):
    """The ordered peak coordinates of _blob_doh (its lines up to the pruning) on the host cube."""
    import scipy.ndimage as ndi
    peaks = (cube == ndi.maximum_filter(cube, footprint=np.ones((3, 3, 3)), mode='nearest')) & (cube > threshold)
    coords = np.transpose(np.nonzero(peaks))
    return coords[np.argsort(-cube[tuple(coords.T)], kind='stable')]


def device_ordered_coords(peaks):
    coords = np.stack([peaks['r'], peaks['c'], peaks['s']], axis=1).astype(np.intp)
    order = np.lexsort((coords[:, 2], coords[:, 1], coords[:, 0]))
    coords, values = coords[order], peaks['value'][order]
    return coords[np.argsort(-values, kind='stable')]


SCENES = {
    'noise': lambda: np.random.default_rng(3).random((200, 260)),
    'bbbc039_like': bbbc039_image,
    'discs_r22': lambda: disc_scene(300, 380, 22, 4),
    'discs_r45': lambda: disc_scene(300, 380, 45, 5),
}


@pytest.mark.parametrize('name', sorted(SCENES))
def test_peaks_and_blobs_are_blob_doh(gpu, name):
    from superdsm_amd import automation
    im = normalized(SCENES[name]())
    masks = automation._log_negative_masks(im, sigmas())
    dev = automation._DohDevice(sigmas()).load(im)
    tiny = automation._DohDevice(sigmas(), capacity=1).load(im)          # every peak list re-run with room for all of it
    cube = host_cube(im, sigmas(), masks)
    n_voxels = cube.size
    for threshold in (0.01, 0.0, 1e9):
        want_coords = host_ordered_coords(cube, threshold)
        peaks, total = dev.peaks(threshold)
        assert total == len(want_coords) and len(peaks) == total
        np.testing.assert_array_equal(device_ordered_coords(peaks), want_coords)
        want = automation._blob_doh(im, sigmas(), threshold=threshold, mask=masks)
        np.testing.assert_array_equal(dev.blobs(threshold), want)
        np.testing.assert_array_equal(tiny.blobs(threshold), want)
        if threshold == 1e9:
            assert total == 0 and len(want) == 0
        else:
            assert total > 1 and len(want) > 0
    assert n_voxels == len(sigmas()) * im.size


def test_all_peaks_rule(gpu):
    """A constant image with threshold -1: every voxel is a peak, which gives nothing (the peaks.all() rule)."""
    from superdsm_amd import automation
    im = np.zeros((60, 70))
    masks = automation._log_negative_masks(im, sigmas())
    for dev in (automation._DohDevice(sigmas()).load(im), automation._DohDevice(sigmas(), capacity=5).load(im)):
        _, total = dev.peaks(-1)
        assert total == len(sigmas()) * im.size
        assert dev.blobs(-1).shape == (0, 3)
    assert automation._blob_doh(im, sigmas(), threshold=-1, mask=masks).shape == (0, 3)


def host_estimate_scale(im, min_radius=20, max_radius=200, num_radii=10, thresholds=[0.01]):
    """_estimate_scale as it was before the device detector: the host restatement (_blob_doh) on the GPU's LoG masks."""
    from superdsm_amd import automation
    sigma_list = np.linspace(min_radius, max_radius, num_radii) / math.sqrt(2)
    sigma_list = np.concatenate([[sigma_list.min() / 2], sigma_list])
    im_norm = automation.normalize_image(im)
    im_norm /= im_norm.max()
    blobs_mask = automation._log_negative_masks(im_norm, sigma_list)
    mean_radius = None
    for threshold in sorted(thresholds, reverse=True):
        blobs_doh = automation._blob_doh(im_norm, sigma_list, threshold=threshold, mask=blobs_mask)
        blobs_doh = blobs_doh[~np.isclose(blobs_doh[:, 2], sigma_list.min())]
        if len(blobs_doh) == 0:
            continue
        radii = blobs_doh[:, 2] * math.sqrt(2)
        radii_median = np.median(radii)
        radii_mad = np.mean(np.abs(radii - np.median(radii)))
        radii_inliers = np.logical_and(radii >= radii_median - radii_mad, radii <= radii_median + radii_mad)
        mean_radius = np.mean(radii[radii_inliers])
        break
    if mean_radius is None:
        raise ValueError('scale estimation failed')
    return mean_radius / math.sqrt(2), blobs_doh, radii_inliers


def assert_same_estimate(got, want):
    assert got[0] == want[0]
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])


@pytest.mark.parametrize('name,kw', [('bbbc039_like', {}), ('discs_r22', {}), ('discs_r45', dict(thresholds=[0.5, 0.01, 0.001])),
                                     ('discs_r22', dict(min_radius=10, max_radius=100, num_radii=6))])
def test_estimate_scale_equals_the_host_evaluation(gpu, name, kw):
    from superdsm_amd import automation
    im = SCENES[name]()
    assert_same_estimate(automation._estimate_scale(im, **kw), host_estimate_scale(im, **kw))


def test_estimate_scales_over_a_mixed_set(gpu):
    from superdsm_amd import automation
    images = [disc_scene(300, 380, 22, 6), bbbc039_image(), disc_scene(250, 420, 45, 7, n=5), disc_scene(300, 380, 30, 8)]
    got = automation.estimate_scales(images)
    assert len(got) == len(images)
    for im, g in zip(images, got):
        assert_same_estimate(g, automation._estimate_scale(im))
    with np.errstate(invalid='ignore'), pytest.raises(ValueError, match='scale estimation failed'):
        automation._estimate_scale(np.full((50, 60), 3.0))
    with np.errstate(invalid='ignore'), pytest.raises(ValueError, match='scale estimation failed'):
        automation.estimate_scales([images[0], np.full((50, 60), 3.0)])
