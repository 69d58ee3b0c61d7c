"""Wall clock of the contour shape tables: the host definition (``shape.shape_objects_host``) against the GPU call
(``shape.shape_objects``, upload through result), three alternating runs each, and the kernels alone (inputs on the device, no download)
by events on the stream, on one BBBC039-like image with its 105 objects, a synthetic 1024^2 image and the synthetic 4096^2 image with
2000 objects.  ``measure.measure_objects`` and its kernel run on the same objects in the same session as the yardstick: they read the
same bits.  The label form (``shape.shape_labels``) is timed on the label map that ``rasterize_labels_gpu`` gives for the same objects;
its host definition passes over the whole image once per label and is not run at 4096^2 (unless --host-4096).

    python tools/time_shape.py [--repeat 3] [--host-4096]
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from superdsm_amd import _capi, measure, render, shape  # noqa: E402
from time_measure import compare, timed  # noqa: E402
from time_results import bbbc, synthetic  # noqa: E402


def same(x, y):
    return all(p.tobytes() == q.tobytes() for p, q in zip(x, y))


def kernels_alone(name, objs, shp, repeat):
    """The launches of sdsm_shape_objects and of sdsm_measure_objects (no intensity) on the same fragments, by events on the stream."""
    import torch
    from superdsm_amd.postprocess import pack_fragments, _exclusive
    T = shape._ShapeSet([shp])
    S, M = T.S, T.M
    boxes, words, packed, _ = pack_fragments(objs)
    n = len(boxes)
    B = T._buffers(boxes)
    d_boxes, d_off, d_bits, d_rec = S._up(boxes), S._up(_exclusive(words)), S._up(np.concatenate(packed)), M.record_buffer(n)
    calls = {'sdsm_shape_objects': lambda: S.L.sdsm_shape_objects_multi(S.table, 1, n, None, S._p(d_boxes), S._p(d_off), S._p(d_bits), S._p(B['d_slot_off']),
                                                                        S._p(B['d_slots']), S._p(B['d_out']), S._p(B['d_vert_off']), S._p(B['d_verts']), S._stream()),
             'sdsm_measure_objects': lambda: S.L.sdsm_measure_objects_multi(S.table, 1, n, None, S._p(d_boxes), S._p(d_off), S._p(d_bits), None, None, None,
                                                                            S._p(d_rec), S._stream())}
    for what, call in calls.items():
        ms = []
        for _ in range(repeat + 1):                           # (the first is the warm-up)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            _capi.check(call(), what)
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        print(f'{name + " " + what + ": launches alone":52s} gpu {statistics.median(ms[1:]):9.3f} ms   (median of {repeat}; {", ".join(f"{t:.3f}" for t in ms[1:])})', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--host-4096', action='store_true', help='run the host definition of the label form on the 4096^2 image as well')
    a = ap.parse_args()
    inputs = [('bbbc039_like', bbbc(0), True), ('synthetic1024 (125 objects)', synthetic(1024, 125), True), ('synthetic4096 (2000 objects)', synthetic(4096, 2000), a.host_4096)]
    for name, d, host_labels in inputs:
        shp, objs = d['g_raw'].shape, d['postprocessed_objects']
        labels = render.rasterize_labels_gpu(d)
        t = shape.shape_objects(objs, shp)
        print(f'{name}: {shp}, {len(objs)} objects, {int(t[0]["n_vertices"].sum())} hull vertices, fragments of up to {max(o.fg_fragment.shape[0] for o in objs)} x '
              f'{max(o.fg_fragment.shape[1] for o in objs)}', flush=True)
        compare(name + ' shape objects', lambda: shape.shape_objects_host(objs, shp), lambda: shape.shape_objects(objs, shp), a.repeat, equal=same)
        compare(name + ' measure objects (yardstick)', lambda: measure.measure_objects_host(objs, shp), lambda: measure.measure_objects(objs, shp), a.repeat,
                equal=lambda x, y: x.tobytes() == y.tobytes())
        compare(name + ' shape labels', (lambda: shape.shape_labels_host(labels)) if host_labels else None, lambda: shape.shape_labels(labels), a.repeat, equal=same)
        td = [timed(lambda: shape.derive(*t))[1] for _ in range(a.repeat)]
        print(f'{name + " derive (on the host, from the GPU result)":52s} host {statistics.median(td):10.1f} ms   ({", ".join(f"{v:.2f}" for v in td)})', flush=True)
        kernels_alone(name, objs, shp, a.repeat)


if __name__ == '__main__':
    main()
