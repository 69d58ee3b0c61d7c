"""Wall clock of the measurement tables: the host definitions (``measure.measure_labels_host``, ``measure_objects_host``) against
the GPU forms (``measure_labels`` / ``_many``, ``measure_objects`` / ``_many``), upload through table, median of alternating runs, on
one BBBC039-like image, the set of 8, a synthetic 1024^2 image and the synthetic 4096^2 image.  Per input: the label map that
``rasterize_labels_gpu`` gives for the ellipses of the workload's layout (with the image as intensity), and those objects themselves.
The host definition of the label form passes over the whole image once per label: on 4096^2 with 2000 labels it is not run (unless
--host-4096), and nothing is extrapolated.

    python tools/time_measure.py [--repeat 3] [--host-4096]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from superdsm_amd import _capi, measure, render  # noqa: E402
from time_results import bbbc, synthetic  # noqa: E402


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, 1e3 * (time.perf_counter() - t0)


def same(x, y):
    tables = lambda v: v if isinstance(v, list) else [v]
    return all(len(p) == len(q) and all(p[n].tobytes() == q[n].tobytes() for n in _capi.MEASURE_RECORD_DTYPE.names) for p, q in zip(tables(x), tables(y)))


def compare(name, host, gpu, repeat, equal=same):
    gpu()                                                     # warm-up: library load, first launch of every kernel
    th, tg = [], []
    for _ in range(repeat):                                   # the two alternate, so that drift of the host hits both
        h = timed(host) if host else None
        g = timed(gpu)
        if h:
            assert equal(h[0], g[0]), name + ': the GPU table differs from the host definition'
            th.append(h[1])
        tg.append(g[1])
    host_text = f'{statistics.median(th):10.1f} ms' if th else '      not run'
    print(f'{name:52s} host {host_text}   gpu {statistics.median(tg):9.2f} ms   (median of {repeat}; gpu runs {", ".join(f"{t:.2f}" for t in tg)})', flush=True)


def kernels_alone(name, labels, objs, g, repeat):
    """The launches of one call alone (inputs already on the device, no download), by events on the stream."""
    import torch
    from superdsm_amd.postprocess import pack_fragments, _exclusive
    M = measure._MeasureSet([g.shape], [g])
    S = M.S
    d_labels = S.pack([labels.astype(np.int32)], np.int32)
    n_labels = int(labels.max()) + 1
    d_rec, d_bad = M.record_buffer(n_labels), torch.empty(1, dtype=torch.int32, device=S.dev)
    boxes, words, packed, _ = pack_fragments(objs)
    d_boxes, d_off, d_bits, d_out = S._up(boxes), S._up(_exclusive(words)), S._up(np.concatenate(packed)), M.record_buffer(len(boxes))
    off, nl = (S.C.c_int64 * 1)(0), (S.C.c_int32 * 1)(n_labels)
    calls = {'labels': lambda dg: S.L.sdsm_measure_labels_multi(S.table, 1, S._p(d_labels), off, nl, S._p(dg), S._p(M.d_gmax), S._p(M.d_exp), S._p(d_rec), S._p(d_bad), S._stream()),
             'objects': lambda dg: S.L.sdsm_measure_objects_multi(S.table, 1, len(boxes), None, S._p(d_boxes), S._p(d_off), S._p(d_bits), S._p(dg), S._p(M.d_gmax), S._p(M.d_exp),
                                                                  S._p(d_out), S._stream())}
    for what, call in calls.items():
        for dg, text in ((M.d_g, ''), (None, ', no intensity')):
            ms = []
            for _ in range(repeat + 1):                       # (the first is the warm-up)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                _capi.check(call(dg), what)
                t1.record()
                torch.cuda.synchronize()
                ms.append(t0.elapsed_time(t1))
            print(f'{name + " " + what + text + ": launches alone":52s} gpu {statistics.median(ms[1:]):9.3f} ms   (median of {repeat}; {", ".join(f"{t:.3f}" for t in ms[1:])})', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--host-4096', action='store_true')
    a = ap.parse_args()
    one, eight = bbbc(0), [bbbc(i) for i in range(8)]
    inputs = [('bbbc039_like', one, True), ('synthetic1024 (125 objects)', synthetic(1024, 125), True), ('synthetic4096 (2000 objects)', synthetic(4096, 2000), a.host_4096)]
    for name, d, host_labels in inputs:
        g, objs = d['g_raw'], d['postprocessed_objects']
        labels = render.rasterize_labels_gpu(d)
        print(f'{name}: {g.shape}, {len(objs)} objects, {len(np.unique(labels)) - 1} labels', flush=True)
        compare(name + ' labels', (lambda: measure.measure_labels_host(labels, g)) if host_labels else None, lambda: measure.measure_labels(labels, g), a.repeat)
        compare(name + ' labels, no intensity', (lambda: measure.measure_labels_host(labels)) if host_labels else None, lambda: measure.measure_labels(labels), a.repeat)
        compare(name + ' regression rows', (lambda: render.label_map_rows(labels)) if host_labels else None, lambda: measure.label_map_rows_gpu(labels), a.repeat,
                equal=lambda x, y: x == y)
        compare(name + ' objects', lambda: measure.measure_objects_host(objs, g.shape, g), lambda: measure.measure_objects(objs, g.shape, g), a.repeat)
        kernels_alone(name, labels, objs, g, a.repeat)
    gs, objs = [d['g_raw'] for d in eight], [d['postprocessed_objects'] for d in eight]
    labels = render.rasterize_labels_many(eight)
    shapes = [g.shape for g in gs]
    compare('8 x bbbc039_like labels: host loop / gpu set', lambda: [measure.measure_labels_host(l, g) for l, g in zip(labels, gs)], lambda: measure.measure_labels_many(labels, gs), a.repeat)
    compare('8 x bbbc039_like labels: one gpu call per image', None, lambda: [measure.measure_labels(l, g) for l, g in zip(labels, gs)], a.repeat)
    compare('8 x bbbc039_like objects: host loop / gpu set', lambda: [measure.measure_objects_host(o, s, g) for o, s, g in zip(objs, shapes, gs)],
            lambda: measure.measure_objects_many(objs, shapes, gs), a.repeat)
    compare('8 x bbbc039_like objects: one gpu call per image', None, lambda: [measure.measure_objects(o, s, g) for o, s, g in zip(objs, shapes, gs)], a.repeat)


if __name__ == '__main__':
    main()
