"""Wall clock of the depth tables: the host definition (``depth.depth_objects_host``) against the GPU call (``depth.depth_objects``, upload
through result), three alternating runs each, on one BBBC039-like image with its objects, a synthetic 1024^2 image and the synthetic
4096^2 image with 2000 objects.  ``shape.shape_objects`` runs on the same objects in the same session as the yardstick: it reads the same
bits and also looks at every pixel's neighbourhood.  The label form (``depth.depth_labels``) is timed on the label map that
``rasterize_labels_gpu`` gives for the same objects; its host definition passes over the whole image once per label and is not run at
4096^2 (unless --host-4096).

The launches alone (inputs on the device, no download) are timed by events on the stream: for the objects of each input, and for three
made-up sets of 64 objects each -- disks whose box fits the LDS tile (radius 50: 101 x 101), disks whose box needs the workspace (radius
60: 121 x 121) and filaments (3 x 120), whose cost should be that of their depth and not of their length.

    python tools/time_depth.py [--repeat 3] [--host-4096]
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from superdsm_amd import _capi, depth, render, shape  # noqa: E402
from time_measure import compare, timed  # noqa: E402
from time_results import bbbc, synthetic  # noqa: E402


def same(x, y):
    return all(p.tobytes() == q.tobytes() for p, q in zip(x, y))


class Piece:
    def __init__(self, offset, fragment):
        self.fg_offset, self.fg_fragment = np.asarray(offset), np.asarray(fragment, bool)


def pieces(fragment, side=1024, n=64):
    step = side // 8
    return [Piece((step * (k // 8), step * (k % 8)), fragment) for k in range(n)]


def disk(radius):
    y, x = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    return y * y + x * x <= radius * radius


def kernels_alone(name, objs, g, repeat):
    """The launches of sdsm_depth_objects (with intensities) and of sdsm_shape_objects on the same fragments, by events on the stream."""
    import torch
    from superdsm_amd.postprocess import pack_fragments, _exclusive
    D = depth._DepthSet([g.shape], [np.ascontiguousarray(g, np.float64)])
    S, M = D.S, D.M
    boxes, words, packed, _ = pack_fragments(objs)
    n = len(boxes)
    B = D.buffers(boxes, depth.DEFAULT_SHELLS)
    ws = D._workspace(B, None)
    T = shape._ShapeSet([g.shape])._buffers(boxes)
    d_boxes, d_off, d_bits = S._up(boxes), S._up(_exclusive(words)), S._up(np.concatenate(packed))
    calls = {'sdsm_depth_objects': lambda: S.L.sdsm_depth_objects_multi(S.table, 1, n, None, S._p(d_boxes), S._p(d_off), S._p(d_bits), S._p(M.d_g), S._p(M.d_gmax),
                                                                        S._p(M.d_exp), depth.DEFAULT_SHELLS, *ws, S._p(B['d_out']), S._p(B['d_shells']), S._stream()),
             'sdsm_shape_objects': lambda: S.L.sdsm_shape_objects_multi(S.table, 1, n, None, S._p(d_boxes), S._p(d_off), S._p(d_bits), S._p(T['d_slot_off']),
                                                                        S._p(T['d_slots']), S._p(T['d_out']), S._p(T['d_vert_off']), S._p(T['d_verts']), S._stream())}
    for what, call in calls.items():
        ms = []
        for _ in range(repeat + 1):                           # (the first is the warm-up)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            _capi.check(call(), what)
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        print(f'{name + " " + what + ": launches alone":60s} gpu {statistics.median(ms[1:]):9.3f} ms   (median of {repeat}; {", ".join(f"{t:.3f}" for t in ms[1:])})', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--host-4096', action='store_true', help='run the host definition of the label form on the 4096^2 image as well')
    a = ap.parse_args()
    inputs = [('bbbc039_like', bbbc(0), True), ('synthetic1024 (125 objects)', synthetic(1024, 125), True), ('synthetic4096 (2000 objects)', synthetic(4096, 2000), a.host_4096)]
    for name, d, host_labels in inputs:
        g, shp, objs = d['g_raw'], d['g_raw'].shape, d['postprocessed_objects']
        labels = render.rasterize_labels_gpu(d)
        t = depth.depth_objects(objs, shp, g)
        px = depth.workspace_pixels([(0, 0) + o.fg_fragment.shape for o in objs])
        print(f'{name}: {shp}, {len(objs)} objects of up to {int(t[0]["area"].max())} pixels and depth {np.sqrt(float(t[0]["max_d2"].max())):.1f}, {int((px > 0).sum())} boxes '
              f'beyond the {_capi.DEPTH_LDS_PIXELS} pixels of LDS', flush=True)
        compare(name + ' depth objects', lambda: depth.depth_objects_host(objs, shp, g), lambda: depth.depth_objects(objs, shp, g), a.repeat, equal=same)
        compare(name + ' shape objects (yardstick)', lambda: shape.shape_objects_host(objs, shp), lambda: shape.shape_objects(objs, shp), a.repeat, equal=same)
        compare(name + ' depth labels', (lambda: depth.depth_labels_host(labels, g)) if host_labels else None, lambda: depth.depth_labels(labels, g), a.repeat, equal=same)
        td = [timed(lambda: depth.derive(*t))[1] for _ in range(a.repeat)]
        print(f'{name + " derive (on the host, from the GPU result)":60s} host {statistics.median(td):10.1f} ms   ({", ".join(f"{v:.2f}" for v in td)})', flush=True)
        kernels_alone(name, objs, g, a.repeat)
    g = np.random.default_rng(5).random((1024, 1024))
    for fragment, text in ((disk(50), '64 disks of radius 50 (LDS)'), (disk(60), '64 disks of radius 60 (workspace)'), (np.ones((3, 120), bool), '64 filaments of 3 x 120')):
        objs = pieces(fragment)
        assert same(depth.depth_objects(objs, g.shape, g), depth.depth_objects_host(objs, g.shape, g))
        kernels_alone(text, objs, g, a.repeat)


if __name__ == '__main__':
    main()
