"""Wall clock of the label maps and result overlays: the host definition (``render.rasterize_labels``, ``render_result_over_image_host``)
against the GPU path (``rasterize_labels_gpu`` / ``_many``, ``render_result_over_image`` / ``_many``), upload through result, on one
BBBC039-like image, the set of 8, a synthetic 1024^2 image and the synthetic 4096^2 image.  The objects are the ellipses of the
workloads' layouts (the 4096^2 layout overlaps heavily), so no pipeline run is needed.  Runs alternate; the share of the host flood
and of the result download of the GPU path is printed.  The host definition holds one full-image mask per object: on 4096^2 with
2000 objects that is 32 GB, so it only runs there with --host-4096.

    python tools/time_results.py [--repeat 3] [--host-4096]
"""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from superdsm_amd import render, synth  # noqa: E402


class Obj:
    def __init__(self, offset, fragment):
        self.fg_offset, self.fg_fragment = np.asarray(offset, int), np.asarray(fragment, bool)

    def fill_foreground(self, out, value=True):
        h, w = self.fg_fragment.shape
        out[self.fg_offset[0]:self.fg_offset[0] + h, self.fg_offset[1]:self.fg_offset[1] + w][self.fg_fragment] = value


def layout_objects(shape, layout):
    objs = []
    for e in layout:
        cy, cx = e['centre']
        a, b = e['axes']
        R = int(math.ceil(max(a, b))) + 1
        r0, r1, c0, c1 = max(0, int(cy) - R), min(shape[0], int(cy) + R + 1), max(0, int(cx) - R), min(shape[1], int(cx) + R + 1)
        yy, xx = np.mgrid[r0:r1, c0:c1]
        ca, sa = math.cos(e['angle']), math.sin(e['angle'])
        u, v = (yy - cy) * ca + (xx - cx) * sa, -(yy - cy) * sa + (xx - cx) * ca
        frag = (u / a) ** 2 + (v / b) ** 2 <= 1
        if frag.any():
            objs.append(Obj((r0, c0), frag))
    return objs


def bbbc(index):
    spec = synth.WORKLOADS['bbbc039_like']
    shape, layout = synth.bbbc039_like_layout(spec['seed'], index)
    return {'g_raw': synth.render_image(shape, layout, spec['seed'] + 7919 * index), 'postprocessed_objects': layout_objects(shape, layout)}


def synthetic(side, n, seed=1005):
    layout = synth.random_layout((side, side), n, 15, seed, min_sep=0.6)
    rng = np.random.default_rng(seed)
    return {'g_raw': rng.random((side, side)), 'postprocessed_objects': layout_objects((side, side), layout)}


SHARE = {'flood': 0.0, 'download': 0.0}


def instrument():
    flood, finish = render.flood_sparse, render._GpuSet.finish

    def timed_flood(*a):
        t0 = time.perf_counter()
        r = flood(*a)
        SHARE['flood'] += time.perf_counter() - t0
        return r

    def timed_finish(self, bg):
        import torch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = finish(self, bg)
        SHARE['download'] += time.perf_counter() - t0
        return r
    render.flood_sparse, render._GpuSet.finish = timed_flood, timed_finish


def timed(fn):
    import torch
    torch.cuda.synchronize()
    SHARE['flood'] = SHARE['download'] = 0.0
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, 1e3 * (time.perf_counter() - t0), 1e3 * SHARE['flood'], 1e3 * SHARE['download']


def compare(name, host, gpu, repeat, equal):
    gpu()                                                     # warm-up: library load, first launch of every kernel
    rows = []
    for _ in range(repeat):                                   # the two alternate, so that drift of the host hits both
        h = timed(host) if host else None
        g = timed(gpu)
        if h:
            assert equal(h[0], g[0]), name + ': the GPU result differs from the host definition'
        rows.append((h[1] if h else float('nan'), g[1], g[2], g[3]))
    for k, (th, tg, tf, td) in enumerate(rows):
        print(f'{name:44s} run {k}: host {th:10.1f} ms   gpu {tg:9.1f} ms   (host flood {tf:7.1f} ms, finish + download {td:7.1f} ms)', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--host-4096', action='store_true')
    a = ap.parse_args()
    instrument()
    eq = lambda x, y: x.dtype == y.dtype and np.array_equal(x, y)
    eq_list = lambda x, y: all(eq(p, q) for p, q in zip(x, y))
    one, eight = bbbc(0), [bbbc(i) for i in range(8)]
    inputs = [('bbbc039_like', one, True), ('synthetic1024 (125 objects)', synthetic(1024, 125), True), ('synthetic4096 (2000 objects)', synthetic(4096, 2000), a.host_4096)]
    for name, d, with_host in inputs:
        print(f'{name}: {d["g_raw"].shape}, {len(d["postprocessed_objects"])} objects', flush=True)
        compare(name + ' labels', (lambda: render.rasterize_labels(d)) if with_host else None, lambda: render.rasterize_labels_gpu(d), a.repeat, eq)
        compare(name + ' labels, merge 0.5', (lambda: render.rasterize_labels(d, merge_overlap_threshold=0.5)) if with_host else None,
                lambda: render.rasterize_labels_gpu(d, merge_overlap_threshold=0.5), a.repeat, eq)
        compare(name + ' overlay', (lambda: render.render_result_over_image_host(d)) if with_host else None, lambda: render.render_result_over_image(d), a.repeat, eq)
    compare('8 x bbbc039_like labels: host loop / gpu set', lambda: [render.rasterize_labels(d) for d in eight], lambda: render.rasterize_labels_many(eight), a.repeat, eq_list)
    compare('8 x bbbc039_like labels: gpu loop / gpu set', lambda: [render.rasterize_labels_gpu(d) for d in eight], lambda: render.rasterize_labels_many(eight), a.repeat, eq_list)
    compare('8 x bbbc039_like overlay: host loop / gpu set', lambda: [render.render_result_over_image_host(d) for d in eight], lambda: render.render_result_over_image_many(eight), a.repeat, eq_list)
    compare('8 x bbbc039_like overlay: gpu loop / gpu set', lambda: [render.render_result_over_image(d) for d in eight], lambda: render.render_result_over_image_many(eight), a.repeat, eq_list)


if __name__ == '__main__':
    main()
