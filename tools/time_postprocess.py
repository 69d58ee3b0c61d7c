"""Wall clock of the ``postprocess`` stage, upload through result (``Postprocessing.process`` on one image, ``process_many`` on a set),
and of its three exact steps alone -- background mask, hole filling, glare test -- as the host passes (SciPy) and, where this commit
has them, as the device steps, on one BBBC039-like image, the set of 8, a synthetic 1024^2 image and the synthetic 4096^2 image.  The
objects are the ellipses of the workloads' layouts with a hole punched into every third, so no pipeline run is needed.  The runs of the
inputs alternate; the median of --repeat runs is printed.  Runs on a commit without the device steps too (the baseline): the stage rows
then measure the host passes in place.

    python tools/time_postprocess.py [--repeat 3] [--no-4096]
"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import scipy.ndimage as ndi

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from superdsm_amd import _morph, config, postprocess, synth, testing  # noqa: E402


class Cover:
    def __init__(self, solution):
        self.solution = solution


def layout_objects(shape, layout):
    objs = []
    for k, e in enumerate(layout):
        cy, cx = e['centre']
        a, b = e['axes']
        R = int(math.ceil(max(a, b))) + 1
        r0, r1, c0, c1 = max(0, int(cy) - R), min(shape[0], int(cy) + R + 1), max(0, int(cx) - R), min(shape[1], int(cx) + R + 1)
        yy, xx = np.mgrid[r0:r1, c0:c1]
        ca, sa = math.cos(e['angle']), math.sin(e['angle'])
        u, v = (yy - cy) * ca + (xx - cx) * sa, -(yy - cy) * sa + (xx - cx) * ca
        frag = (u / a) ** 2 + (v / b) ** 2 <= 1
        if k % 3 == 0:
            frag &= (u / a) ** 2 + (v / b) ** 2 > 0.04
        rows, cols = np.flatnonzero(frag.any(1)), np.flatnonzero(frag.any(0))
        if rows.size:
            objs.append(testing.PostFragment((r0 + rows[0], c0 + cols[0]), frag[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1]))
    return objs


def bbbc(index):
    spec = synth.WORKLOADS['bbbc039_like']
    shape, layout = synth.bbbc039_like_layout(spec['seed'], index)
    return synth.render_image(shape, layout, spec['seed'] + 7919 * index), layout_objects(shape, layout)


def synthetic(side, n, seed=1005):
    layout = synth.random_layout((side, side), n, 15, seed, min_sep=0.6)
    return np.random.default_rng(seed).random((side, side)), layout_objects((side, side), layout)


def data_of(g, objects):
    return dict(cover=Cover(objects), y_img=None, atoms=None, g_raw=g, dsm_cfg=None)


def sync():
    import torch
    torch.cuda.synchronize()


def clock(fn):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return 1e3 * (time.perf_counter() - t0)


def report(rows, repeat):
    """``rows``: name -> callable; the callables alternate, ``repeat`` rounds after one warm-up round."""
    for fn in rows.values():
        fn()
    times = {name: [] for name in rows}
    for _ in range(repeat):
        for name, fn in rows.items():
            times[name].append(clock(fn))
    for name, t in times.items():
        print(f'{name:64s} median {statistics.median(t):10.2f} ms   ({", ".join(f"{v:.2f}" for v in t)})', flush=True)


def host_background(g, objects, r=5):
    mask = np.zeros(g.shape, bool)
    for o in objects:
        o.fill_foreground(mask)
    return _morph.binary_erosion(~mask, _morph.disk(r))


def step_rows(name, g, objects):
    """The three steps alone on one image: host pass and device step."""
    import torch
    rows = {f'{name}: background mask, host (SciPy erosion + upload)': lambda: torch.from_numpy(host_background(g, objects).view(np.uint8)).cuda(),
            f'{name}: hole filling, host (binary_fill_holes per object)': lambda: [ndi.binary_fill_holes(o.fg_fragment) for o in objects]}
    g_dev = torch.as_tensor(np.ascontiguousarray(g)).cuda()
    g_glare = postprocess.gaussian_filter_gpu(g_dev, 3)
    rows[f'{name}: glare test, host (image download + _is_glare per object)'] = lambda: (lambda gg: [postprocess._is_glare(o, gg) for o in objects])(g_glare.cpu().numpy())
    if hasattr(postprocess, 'background_mask_gpu'):
        dims, offsets, bits = postprocess.pack_windows([o.fg_fragment for o in objects])
        d_bits = torch.from_numpy(bits).cuda()
        rows[f'{name}: background mask, device (pack + upload + kernels)'] = lambda: postprocess.background_mask_gpu(objects, g.shape, 5)
        rows[f'{name}: hole filling, device (kernel on resident windows)'] = lambda: postprocess._fill_holes_device(d_bits, dims, offsets)
        rows[f'{name}: hole filling, device (pack + upload + kernel + download)'] = lambda: postprocess.fill_holes_gpu([o.fg_fragment for o in objects])
        rows[f'{name}: glare test, device (pack + upload + kernel + flags)'] = lambda: postprocess.glare_flags_gpu_multi([(objects, g_glare)], 0.5, 5)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--no-4096', action='store_true')
    a = ap.parse_args()
    one, eight = bbbc(0), [bbbc(i) for i in range(8)]
    inputs = [('bbbc039_like', *one), ('synthetic1024', *synthetic(1024, 125))] + ([] if a.no_4096 else [('synthetic4096', *synthetic(4096, 2000))])
    stage = postprocess.Postprocessing()
    default, glare_on = config.Config({'postprocess': {}}), config.Config({'postprocess': {'min_glare_radius': 0.0}})
    rows = {}
    for name, g, objects in inputs:
        print(f'{name}: {g.shape}, {len(objects)} objects', flush=True)
        for label, cfg in (('defaults', default), ('glare test on', glare_on)):
            rows[f'{name}: stage, process, {label}'] = lambda g=g, objects=objects, cfg=cfg: stage(data_of(g, objects), cfg, out='muted')
    for label, cfg in (('defaults', default), ('glare test on', glare_on)):
        rows[f'8 x bbbc039_like: stage, process_many, {label}'] = lambda cfg=cfg: stage.process_many([data_of(g, o) for g, o in eight], cfg, out='muted')
        rows[f'8 x bbbc039_like: stage, process one by one, {label}'] = lambda cfg=cfg: [stage(data_of(g, o), cfg, out='muted') for g, o in eight]
    report(rows, a.repeat)
    for name, g, objects in inputs:
        report(step_rows(name, g, objects), a.repeat)


if __name__ == '__main__':
    main()
