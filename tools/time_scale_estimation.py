"""Wall-clock of the scale estimation per image, host restatement against the device detector (upload through result).

    python tools/time_scale_estimation.py [--repeat N] [--host-max-pixels P]

Scenes: Gaussian-ish discs of radius 25 on noise at 520x696, 1024x1344 and 4096x4096.  "host" is the path _estimate_scale took
before the device detector: the LoG masks on the GPU, then _blob_doh (integral image, determinant cube, 3x3x3 maximum filter,
pruning) in NumPy / SciPy.  "gpu" is _estimate_scale (one image, detector set up per call) and estimate_scales over a set of four
copies (per image).  The phases of one image follow, in ms, each timed to a synchronisation: normalize_image on the host, the
upload of the normalised image alone, upload + LoG masks, integral image + cube, peak compaction + download."""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scene(H, W, r=25, seed=0):
    rng = np.random.default_rng(seed)
    im = 0.02 * rng.standard_normal((H, W))
    n = max(8, int(8 * H * W / (300 * 380)))
    half = 3 * r
    yy, xx = np.mgrid[-half:half + 1, -half:half + 1]
    for _ in range(n):
        r0, c0 = int(rng.uniform(r, H - r)), int(rng.uniform(r, W - r))
        blob = np.exp(-((yy ** 2 + xx ** 2) / (r * r)) ** 2)
        a0, a1, b0, b1 = max(r0 - half, 0), min(r0 + half + 1, H), max(c0 - half, 0), min(c0 + half + 1, W)
        im[a0:a1, b0:b1] += blob[a0 - r0 + half:a1 - r0 + half, b0 - c0 + half:b1 - c0 + half]
    return im


def host_estimate(im, sigma_list, automation):
    im_norm = automation.normalize_image(im)
    im_norm /= im_norm.max()
    masks = automation._log_negative_masks(im_norm, sigma_list)
    return automation._scale_from_blobs(lambda t: automation._blob_doh(im_norm, sigma_list, threshold=t, mask=masks), sigma_list, [0.01])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--host-max-pixels', type=int, default=1 << 25)
    a = ap.parse_args()
    import torch
    from superdsm_amd import automation
    sync = torch.cuda.synchronize
    sigma_list = automation._sigma_list(20, 200, 10)
    automation._estimate_scale(scene(200, 260))                         # warm-up: library load, kernels, allocator
    print(f'{"image":>10} {"host s":>8} {"gpu ms":>8} {"set ms/img":>10} {"norm":>6} {"upload":>7} {"masks":>7} {"ii+cube":>8} {"peaks":>7} {"blobs":>6} '
          f'{"scale":>8}  same')
    for H, W in [(520, 696), (1024, 1344), (4096, 4096)]:
        im = scene(H, W)
        host_s, same = float('nan'), '-'
        got = automation._estimate_scale(im)
        if H * W <= a.host_max_pixels:
            t0 = time.perf_counter()
            want = host_estimate(im, sigma_list, automation)
            host_s = time.perf_counter() - t0
            same = str(want[0] == got[0] and np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[2]))
        ts = []
        for _ in range(a.repeat):
            sync()
            t0 = time.perf_counter()
            automation._estimate_scale(im)
            ts.append(time.perf_counter() - t0)
        sync()
        t0 = time.perf_counter()
        automation.estimate_scales([im] * 4)
        set_ms = (time.perf_counter() - t0) / 4 * 1e3
        dev = automation._DohDevice(sigma_list)
        ph = []
        t0 = time.perf_counter()
        im_norm = automation.normalize_image(im)
        im_norm /= im_norm.max()
        norm_ms = (time.perf_counter() - t0) * 1e3
        dev.load(im_norm)
        sync()
        t0 = time.perf_counter()
        torch.as_tensor(im_norm).cuda()
        sync()
        upload_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        dev._masks(im_norm)
        sync()
        ph.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        dev.load(im_norm)                                                # (masks again + integral image + cube)
        sync()
        ph.append(time.perf_counter() - t0 - ph[0])
        t0 = time.perf_counter()
        dev.peaks(0.01)
        ph.append(time.perf_counter() - t0)
        print(f'{f"{H}x{W}":>10} {host_s:8.2f} {min(ts) * 1e3:8.1f} {set_ms:10.1f} {norm_ms:6.1f} {upload_ms:7.1f} {ph[0] * 1e3:7.1f} {ph[1] * 1e3:8.1f} '
              f'{ph[2] * 1e3:7.1f} {len(got[1]):6d} {got[0]:8.3f}  {same}', flush=True)


if __name__ == '__main__':
    main()
