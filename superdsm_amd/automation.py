"""AF_ expansion of scale-dependent hyper-parameters and automatic scale estimation (reference: superdsm/automation.py).

``create_config`` is automation.py:80-102.  ``_estimate_scale`` restates automation.py:41-68: determinant-of-Hessian blobs on
11 scales (radii 20 … 200 pixels), restricted to pixels where the Laplacian of Gaussian is negative; the scale is the mean
radius of the inlier blobs / sqrt(2).  PARITY UNPINNED: the reference takes ``_hessian_matrix_det``, ``peak_local_max`` and
``_prune_blobs`` from scikit-image, which is not available to this build; they are restated from their documented behaviour (box
filters on the integral image as in SURF; local maxima of a 3x3x3 neighbourhood above the threshold; of two blobs overlapping by
more than ``overlap`` the smaller one is dropped) and checked on synthetic images of known scale only.

The host functions below (``_integ``, ``_hessian_matrix_det``, ``_blob_doh``, ``_prune_blobs``) are that restatement; the detector
that ``_estimate_scale`` and ``estimate_scales`` run is its device twin (``_DohDevice``), bit for bit: the Laplacian-of-Gaussian
masks (separable filters with up to 1100 taps, SciPy's own derivative-of-Gaussian weights), the integral image, the
determinant-of-Hessian cube of all scales and the peak compaction are HIP kernels (sdsm_log_masks, sdsm_integral_image,
sdsm_doh_cube, sdsm_doh_peaks); the host puts the few peaks into ``np.nonzero``'s order and prunes them."""
import math

import numpy as np
import scipy.ndimage as ndi
from scipy.spatial import cKDTree


def normalize_image(img, spread=1):
    """Contrast enhancement (superdsm/render.py:137-165)."""
    img = np.asarray(img, np.float64)
    if not np.allclose(img.std(), 0):
        minval, maxval = max(img.min(), img.mean() - spread * img.std()), min(img.max(), img.mean() + spread * img.std())
        img = img.clip(minval, maxval)
    img = img - img.min()
    return img / img.max()


def _integ(ii, r, c, rl, cl):
    """Clamped box sum on the integral image (rows r .. r + rl, columns c .. c + cl as scikit-image's ``_integ`` takes them):
    the origin is clipped FIRST and the far corner is measured from the clipped origin, so a window that starts above / left of
    the image slides into it instead of shrinking (parity unpinned, see the module docstring)."""
    H, W = ii.shape
    r1, c1 = np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)
    r2, c2 = np.clip(r1 + rl, 0, H - 1), np.clip(c1 + cl, 0, W - 1)
    ans = ii[r1[:, None], c1[None, :]] + ii[r2[:, None], c2[None, :]] - ii[r1[:, None], c2[None, :]] - ii[r2[:, None], c1[None, :]]
    return np.maximum(0, ans)


def _hessian_matrix_det(ii, sigma):
    """Approximate determinant of the Hessian at scale ``sigma`` from box filters on the integral image ``ii``."""
    size = int(3 * sigma)
    H, W = ii.shape
    s2, s3, w = (size - 1) // 2, size // 3, size
    w_i = 1.0 / size / size
    r, c = np.arange(H), np.arange(W)
    tl = _integ(ii, r - s3, c - s3, s3, s3)
    br = _integ(ii, r + 1, c + 1, s3, s3)
    bl = _integ(ii, r - s3, c + 1, s3, s3)
    tr = _integ(ii, r + 1, c - s3, s3, s3)
    dxy = -(bl + tr - tl - br) * w_i
    mid = _integ(ii, r - s3 + 1, c - s2, 2 * s3 - 1, w)
    side = _integ(ii, r - s3 + 1, c - s3 // 2, 2 * s3 - 1, s3)
    dxx = -(mid - 3 * side) * w_i
    mid = _integ(ii, r - s2, c - s3 + 1, w, 2 * s3 - 1)
    side = _integ(ii, r - s3 // 2, c - s3 + 1, s3, 2 * s3 - 1)
    dyy = -(mid - 3 * side) * w_i
    return dxx * dyy - 0.81 * (dxy * dxy)


def _disk_overlap(d, r1, r2):
    ratio1 = np.clip((d ** 2 + r1 ** 2 - r2 ** 2) / (2 * d * r1), -1, 1)
    ratio2 = np.clip((d ** 2 + r2 ** 2 - r1 ** 2) / (2 * d * r2), -1, 1)
    a, b, c, e = -d + r2 + r1, d - r2 + r1, d + r2 - r1, d + r2 + r1
    area = r1 ** 2 * math.acos(ratio1) + r2 ** 2 * math.acos(ratio2) - 0.5 * math.sqrt(abs(a * b * c * e))
    return area / (math.pi * min(r1, r2) ** 2)


def _blob_overlap(b1, b2):
    root = math.sqrt(2)
    if b1[-1] == b2[-1] == 0:
        return 0.0
    if b1[-1] > b2[-1]:
        max_sigma, r1, r2 = b1[-1], 1.0, b2[-1] / b1[-1]
    else:
        max_sigma, r1, r2 = b2[-1], b1[-1] / b2[-1], 1.0
    p1, p2 = b1[:2] / (max_sigma * root), b2[:2] / (max_sigma * root)
    d = math.sqrt(float(((p2 - p1) ** 2).sum()))
    if d > r1 + r2:
        return 0.0
    if d <= abs(r1 - r2):
        return 1.0
    return _disk_overlap(d, r1, r2)


def _prune_blobs(blobs, overlap):
    """Of two blobs whose disks (radius sigma * sqrt(2)) overlap by more than ``overlap`` of the smaller, drop the smaller."""
    sigma = blobs[:, -1].max()
    pairs = sorted(cKDTree(blobs[:, :-1]).query_pairs(2 * sigma * math.sqrt(blobs.shape[1] - 1)))
    for i, j in pairs:
        if _blob_overlap(blobs[i], blobs[j]) > overlap:
            if blobs[i][-1] > blobs[j][-1]:
                blobs[j][-1] = 0
            else:
                blobs[i][-1] = 0
    return blobs[blobs[:, -1] > 0]


def _blob_doh(image, sigma_list, threshold=0.01, overlap=.5, mask=None):
    """Determinant-of-Hessian blobs (automation.py:13-38): rows (r, c, sigma)."""
    image = np.asarray(image, np.float64)
    if mask is None:
        mask = np.ones(image.shape, bool)
    if not isinstance(mask, dict):
        mask = {sigma: mask for sigma in sigma_list}
    ii = image.cumsum(0).cumsum(1)
    cube = np.dstack([mask[s] * _hessian_matrix_det(ii, s) for s in sigma_list])
    peaks = (cube == ndi.maximum_filter(cube, footprint=np.ones((3, 3, 3)), mode='nearest')) & (cube > threshold)
    if peaks.all():
        peaks[:] = False
    coords = np.transpose(np.nonzero(peaks))
    if coords.size == 0:
        return np.empty((0, 3))
    coords = coords[np.argsort(-cube[tuple(coords.T)], kind='stable')]
    lm = coords.astype(np.float64)
    lm[:, -1] = np.asarray(sigma_list)[coords[:, -1]]
    return _prune_blobs(lm, overlap)


def _blobs_from_peaks(peaks, total, n_voxels, sigma_list, overlap=.5):
    """The tail of ``_blob_doh`` from the cube's peaks in any order (``_capi.DOH_PEAK_DTYPE`` records, ``total`` of them, out of
    ``n_voxels`` voxels): every voxel a peak gives nothing (``peaks.all()``); otherwise the peaks are put into ``np.nonzero``'s order,
    lexicographic in (r, c, s), then stable-sorted by descending value and pruned."""
    if total == n_voxels or total == 0:
        return np.empty((0, 3))
    assert len(peaks) == total, 'incomplete peak list'
    coords = np.stack([peaks['r'], peaks['c'], peaks['s']], axis=1).astype(np.intp)
    order = np.lexsort((coords[:, 2], coords[:, 1], coords[:, 0]))
    coords, values = coords[order], peaks['value'][order]
    coords = coords[np.argsort(-values, kind='stable')]
    lm = coords.astype(np.float64)
    lm[:, -1] = np.asarray(sigma_list)[coords[:, -1]]
    return _prune_blobs(lm, overlap)


def _log_weights(sigma_list):
    """SciPy's weights of the two terms of ``ndi.gaussian_laplace`` (``_gaussian_kernel1d`` of order 0 and 2, radius
    int(4 sigma + 0.5), reversed as ``correlate1d`` applies them; both symmetric): the radii and, per sigma, the 2 R + 1 weights of
    order 0 followed by the 2 R + 1 of order 2."""
    from scipy.ndimage._filters import _gaussian_kernel1d
    radii, parts = [], []
    for sigma in sigma_list:
        R = int(4.0 * float(sigma) + 0.5)
        radii.append(R)
        parts += [_gaussian_kernel1d(float(sigma), 0, R)[::-1], _gaussian_kernel1d(float(sigma), 2, R)[::-1]]
    return np.asarray(radii, np.int32), np.ascontiguousarray(np.concatenate(parts), np.float64)


def _box_params(sigma_list):
    """``size``, ``s2``, ``s3`` and ``w_i`` of ``_hessian_matrix_det`` per sigma, computed as it computes them."""
    box, w_i = np.zeros((len(sigma_list), 3), np.int32), np.zeros(len(sigma_list))
    for k, sigma in enumerate(sigma_list):
        size = int(3 * sigma)
        box[k] = size, (size - 1) // 2, size // 3
        w_i[k] = 1.0 / size / size
    return box, w_i


class _DohDevice:
    """The device twin of ``_log_negative_masks`` + ``_blob_doh`` for one sigma list.  The filter weights go to the device once;
    the workspaces grow on demand and are reused over an image set.  ``load(im)`` uploads an image and computes its LoG masks,
    integral image and determinant-of-Hessian cube on the current stream without waiting for any of it; ``blobs(threshold)``
    compacts the cube's peaks and downloads them once.  ``capacity``: peak records downloaded at first; more peaks than that
    re-run the compaction alone with room for all of them."""

    def __init__(self, sigma_list, capacity=4096):
        import torch
        from . import _capi
        self._torch, self._capi, self._L = torch, _capi, _capi.lib()
        self.sigma_list = np.asarray(sigma_list, np.float64)
        if not 1 <= len(self.sigma_list) <= _capi.DOH_MAX_SCALES:
            raise ValueError(f'the device detector takes 1 to {_capi.DOH_MAX_SCALES} scales')
        self.radii, weights = _log_weights(self.sigma_list)
        self.box, self.w_i = _box_params(self.sigma_list)
        self._d_weights = torch.as_tensor(weights).cuda()
        self.capacity = max(int(capacity), 1)
        self._bufs = {}
        self.shape = None

    def _buf(self, name, nbytes):
        b = self._bufs.get(name)
        if b is None or b.numel() < nbytes:
            self._bufs[name] = b = self._torch.empty(max(int(nbytes), 1), dtype=self._torch.uint8, device=self._d_weights.device)
        return b

    def _f64(self, name, n):
        return self._buf(name, 8 * n)[:8 * n].view(self._torch.float64)

    @staticmethod
    def _p(t):
        import ctypes as C
        return C.c_void_p(t.data_ptr())

    def _stream(self):
        import ctypes as C
        return C.c_void_p(self._torch.cuda.current_stream().cuda_stream)

    def _masks(self, im):
        import ctypes as C
        im = np.ascontiguousarray(im, np.float64)
        H, W = self.shape = im.shape
        n, S = H * W, len(self.sigma_list)
        d_im = self._f64('im', n)
        d_im.copy_(self._torch.from_numpy(im).reshape(-1))
        nbytes = self._L.sdsm_log_masks_workspace_bytes(H, W)
        d_masks = self._buf('masks', S * n)
        self._capi.check(self._L.sdsm_log_masks(self._p(d_im), H, W, S, self.radii.ctypes.data_as(C.c_void_p), self._p(self._d_weights),
                                                self._p(d_masks), self._p(self._buf('ws', nbytes)), nbytes, self._stream()), 'sdsm_log_masks')
        return d_im, d_masks

    def log_masks(self, im):
        """``{sigma: ndi.gaussian_laplace(im, sigma) < 0}``: one download for all sigmas."""
        _, d_masks = self._masks(im)
        H, W = self.shape
        masks = d_masks[:len(self.sigma_list) * H * W].cpu().numpy().view(bool).reshape(-1, H, W)
        return {sigma: masks[k] for k, sigma in enumerate(self.sigma_list)}

    def load(self, im):
        import ctypes as C
        d_im, d_masks = self._masks(im)
        H, W = self.shape
        S, stream = len(self.sigma_list), self._stream()
        d_ii, d_cube = self._f64('ii', H * W), self._f64('cube', S * H * W)
        self._capi.check(self._L.sdsm_integral_image(self._p(d_im), H, W, self._p(d_ii), stream), 'sdsm_integral_image')
        self._capi.check(self._L.sdsm_doh_cube(self._p(d_ii), H, W, S, self.box.ctypes.data_as(C.c_void_p), self.w_i.ctypes.data_as(C.c_void_p),
                                               self._p(d_masks), self._p(d_cube), stream), 'sdsm_doh_cube')
        return self

    def integral_image(self):
        """The integral image of the loaded image (a download: diagnostics and tests)."""
        return self._f64('ii', self.shape[0] * self.shape[1]).cpu().numpy().reshape(self.shape)

    def cube(self):
        """The cube of the loaded image as (scale, row, column) (a download: diagnostics and tests)."""
        return self._f64('cube', len(self.sigma_list) * self.shape[0] * self.shape[1]).cpu().numpy().reshape((-1,) + self.shape)

    def peaks(self, threshold):
        """The peaks of the loaded image's cube above ``threshold``, in no particular order, and their total."""
        H, W = self.shape
        S, hdr = len(self.sigma_list), self._capi.DOH_PEAKS_HEADER_BYTES
        cap = self.capacity
        while True:
            nbytes = hdr + cap * self._capi.DOH_PEAK_DTYPE.itemsize
            d_out = self._buf('peaks', nbytes)
            self._capi.check(self._L.sdsm_doh_peaks(self._p(self._f64('cube', S * H * W)), H, W, S, float(threshold), self._p(d_out), cap,
                                                    self._stream()), 'sdsm_doh_peaks')
            host = d_out[:nbytes].cpu().numpy()
            total = int(host[:8].view(np.int64)[0])
            if total <= cap or total == S * H * W:      # (every voxel a peak: the list is not needed)
                break
            cap = total
        return host[hdr:hdr + min(total, cap) * self._capi.DOH_PEAK_DTYPE.itemsize].view(self._capi.DOH_PEAK_DTYPE), total

    def blobs(self, threshold, overlap=.5):
        """``_blob_doh(im, sigma_list, threshold, overlap, mask=_log_negative_masks(im, sigma_list))`` of the loaded image."""
        peaks, total = self.peaks(threshold)
        return _blobs_from_peaks(peaks, total, len(self.sigma_list) * self.shape[0] * self.shape[1], self.sigma_list, overlap)


def _log_negative_masks(im, sigma_list):
    """``{sigma: ndi.gaussian_laplace(im, sigma) < 0}`` (automation.py:52) with the filters on the GPU.  The weights are SciPy's own
    (``_gaussian_kernel1d`` of order 0 and 2: both symmetric), the axes are filtered in SciPy's order."""
    return _DohDevice(sigma_list).log_masks(im)


def _sigma_list(min_radius, max_radius, num_radii):
    sigma_list = np.linspace(min_radius, max_radius, num_radii) / math.sqrt(2)
    return np.concatenate([[sigma_list.min() / 2], sigma_list])


def _estimate_scale(im, min_radius=20, max_radius=200, num_radii=10, thresholds=[0.01], inlier_tol=np.inf):
    """Estimates the scale sigma of the objects of an image (automation.py:41-68).  Returns (scale, blobs, inlier mask)."""
    return estimate_scales([im], min_radius, max_radius, num_radii, thresholds, inlier_tol)[0]


def estimate_scales(images, min_radius=20, max_radius=200, num_radii=10, thresholds=[0.01], inlier_tol=np.inf):
    """``_estimate_scale`` of every image of a set (the images may differ in shape): one device detector, its workspaces reused
    from image to image.  Raises ValueError('scale estimation failed') as soon as an image yields no blobs."""
    sigma_list = _sigma_list(min_radius, max_radius, num_radii)
    dev = _DohDevice(sigma_list)
    out = []
    for im in images:
        im_norm = normalize_image(im)
        im_norm /= im_norm.max()
        dev.load(im_norm)
        out.append(_scale_from_blobs(dev.blobs, sigma_list, thresholds))
    return out


def _scale_from_blobs(blob_doh, sigma_list, thresholds):
    """The rule of automation.py:55-68 over ``blob_doh(threshold)`` -> blobs (rows r, c, sigma)."""
    mean_radius = None
    for threshold in sorted(thresholds, reverse=True):
        blobs_doh = blob_doh(threshold)
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


def _expand(cfg, key, factor, default_user_factor, type=None, min=None, max=None):
    *ns, leaf = key.split('/')
    af_key = '/'.join(ns + ['AF_' + leaf])
    cfg.set_default(key, factor * cfg.get(af_key, default_user_factor), True)
    if type is not None:
        cfg.update(key, func=type)
    if min is not None:
        cfg.update(key, func=lambda value: value if value >= min else min)
    if max is not None:
        cfg.update(key, func=lambda value: value if value <= max else max)


def create_config(pipeline, base_cfg, img=None):
    """Scale-dependent hyper-parameters from ``AF_scale`` or, if that is not set, from the estimated scale of ``img``
    (automation.py:80-102): the set of this one image (:func:`create_configs`)."""
    if img is None and base_cfg.copy().get('AF_scale', None) is None:
        raise ValueError('AF_scale is not set and there is no image to estimate the scale from')
    return create_configs(pipeline, base_cfg, [img])[0]


def _configure(pipeline, cfg, scale):
    for stage in pipeline.stages:
        for key, spec in stage.configure(scale).items():
            assert len(spec) in (2, 3), f'{type(stage).__name__}.configure returned tuple of unknown length ({len(spec)})'
            _expand(cfg, f'{stage.cfgns}/{key}', spec[0], spec[1], **(spec[2] if len(spec) == 3 else {}))


def create_configs(pipeline, base_cfg, images):
    """The config sequence of automation.py:80-102 for every image of a set: ``(cfg, scale)`` per image.  Without ``AF_scale``,
    :func:`estimate_scales` estimates the scales of all images in one call."""
    images = list(images)
    scale = base_cfg.copy().get('AF_scale', None)
    scales = [scale] * len(images) if scale is not None else [s[0] for s in estimate_scales(images, num_radii=10, thresholds=[0.01])]
    result = []
    for scale in scales:
        cfg = base_cfg.copy()
        cfg.get('AF_scale', None)                       # (as the reference's get: the key is there afterwards, None if it was unset)
        _configure(pipeline, cfg, scale)
        result.append((cfg, scale))
    return result
