"""Host half of the device determinant-of-Hessian detector (superdsm_amd/automation.py): the peaks that the device compacts in no
particular order, put back into np.nonzero's order and through the peaks.all() rule, give exactly ``_blob_doh``.  The peak lists
here come from the host restatement's own cube, shuffled.  CPU only."""
import math

import numpy as np
import pytest
import scipy.ndimage as ndi

from superdsm_amd import _capi, automation

SIGMAS = automation._sigma_list(20, 200, 10)


def scene(H, W, r, seed, n=8):
    """The generator of the scale-estimation test in test_gpu_parity.py: Gaussian-ish discs of radius r on noise."""
    rng = np.random.default_rng(seed)
    rr, cc = np.mgrid[:H, :W]
    im = 0.02 * rng.standard_normal((H, W))
    for _ in range(n):
        r0, c0 = rng.uniform(r, H - r), rng.uniform(r, W - r)
        im += np.exp(-(((rr - r0) ** 2 + (cc - c0) ** 2) / (r * r)) ** 2)
    return automation.normalize_image(im)


def host_cube(image, sigma_list, mask):
    ii = np.asarray(image, np.float64).cumsum(0).cumsum(1)
    return np.dstack([mask[s] * automation._hessian_matrix_det(ii, s) for s in sigma_list])


def shuffled_peaks(cube, threshold, seed):
    """The peak records as sdsm_doh_peaks writes them (cube laid out as row, column, scale here), in random order."""
    peaks = (cube == ndi.maximum_filter(cube, footprint=np.ones((3, 3, 3)), mode='nearest')) & (cube > threshold)
    r, c, s = np.nonzero(peaks)
    rec = np.zeros(len(r), _capi.DOH_PEAK_DTYPE)
    rec['r'], rec['c'], rec['s'], rec['value'] = r, c, s, cube[r, c, s]
    return rec[np.random.default_rng(seed).permutation(len(rec))], len(rec)


def random_masks(shape, sigma_list, seed):
    rng = np.random.default_rng(seed)
    return {s: rng.random(shape) < 0.7 for s in sigma_list}


CASES = [
    ('noise', lambda: np.random.default_rng(1).random((60, 80)), None, 0.0),
    ('noise_masked', lambda: np.random.default_rng(2).random((70, 50)), 'random', 0.0),
    ('discs_r22', lambda: scene(150, 190, 22, 3), 'random', 0.01),
    ('discs_r45', lambda: scene(200, 210, 45, 4, n=4), None, 0.01),
]


@pytest.mark.parametrize('name,make,mask_kind,threshold', CASES, ids=[c[0] for c in CASES])
def test_shuffled_peak_list_reproduces_blob_doh(name, make, mask_kind, threshold):
    im = make()
    mask = random_masks(im.shape, SIGMAS, 5) if mask_kind == 'random' else {s: np.ones(im.shape, bool) for s in SIGMAS}
    want = automation._blob_doh(im, SIGMAS, threshold=threshold, mask=mask)
    cube = host_cube(im, SIGMAS, mask)
    for seed in (0, 1):
        peaks, total = shuffled_peaks(cube, threshold, seed)
        assert total > 1
        got = automation._blobs_from_peaks(peaks, total, cube.size, SIGMAS)
        np.testing.assert_array_equal(got, want)
    assert len(want) > 0


def test_all_peaks_and_no_peaks_give_nothing():
    im = np.zeros((40, 50))
    assert automation._blob_doh(im, SIGMAS, threshold=-1).shape == (0, 3)       # every voxel a peak: the all-peaks rule
    cube = host_cube(im, SIGMAS, {s: np.ones(im.shape, bool) for s in SIGMAS})
    peaks, total = shuffled_peaks(cube, -1, 0)
    assert total == cube.size
    assert automation._blobs_from_peaks(peaks, total, cube.size, SIGMAS).shape == (0, 3)
    assert automation._blobs_from_peaks(peaks[:3], total, cube.size, SIGMAS).shape == (0, 3)   # (the list is not needed then)
    im = scene(60, 70, 10, 6)
    assert automation._blob_doh(im, SIGMAS, threshold=1e9).shape == (0, 3)
    peaks, total = shuffled_peaks(host_cube(im, SIGMAS, {s: np.ones(im.shape, bool) for s in SIGMAS}), 1e9, 0)
    assert total == 0 and automation._blobs_from_peaks(peaks, total, cube.size, SIGMAS).shape == (0, 3)


def test_box_and_filter_parameters_are_the_restatements():
    box, w_i = automation._box_params(SIGMAS)
    for k, sigma in enumerate(SIGMAS):
        size = int(3 * sigma)
        assert tuple(box[k]) == (size, (size - 1) // 2, size // 3) and w_i[k] == 1.0 / size / size
    radii, w = automation._log_weights(SIGMAS)
    assert radii.tolist() == [int(4.0 * float(s) + 0.5) for s in SIGMAS]
    assert len(w) == sum(2 * (2 * R + 1) for R in radii)
    off = 0
    for R in radii:
        w0, w2 = w[off:off + 2 * R + 1], w[off + 2 * R + 1:off + 4 * R + 2]
        np.testing.assert_array_equal(w0, w0[::-1])
        np.testing.assert_array_equal(w2, w2[::-1])
        off += 4 * R + 2


def test_scale_rule_over_host_blobs_is_the_reference_loop():
    """``_scale_from_blobs`` (the median / MAD rule that _estimate_scale applies to the device's blobs) over the host restatement
    equals the loop of automation.py:55-68 written out, for several thresholds; no blobs at all raises."""
    im = scene(160, 200, 22, 7)
    masks = {s: ndi.gaussian_laplace(im, s) < 0 for s in SIGMAS}
    thresholds = [0.5, 0.01, 0.001]
    got = automation._scale_from_blobs(lambda t: automation._blob_doh(im, SIGMAS, threshold=t, mask=masks), SIGMAS, thresholds)
    for threshold in sorted(thresholds, reverse=True):
        blobs = automation._blob_doh(im, SIGMAS, threshold=threshold, mask=masks)
        blobs = blobs[~np.isclose(blobs[:, 2], SIGMAS.min())]
        if len(blobs) == 0:
            continue
        radii = blobs[:, 2] * math.sqrt(2)
        med = np.median(radii)
        mad = np.mean(np.abs(radii - np.median(radii)))
        inl = np.logical_and(radii >= med - mad, radii <= med + mad)
        want = (np.mean(radii[inl]) / math.sqrt(2), blobs, inl)
        break
    assert got[0] == want[0]
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])
    with pytest.raises(ValueError, match='scale estimation failed'):
        automation._scale_from_blobs(lambda t: np.empty((0, 3)), SIGMAS, thresholds)
