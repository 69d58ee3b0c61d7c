"""Wall clock of the intensity distribution tables: the host definition (``intensity.intensity_objects_host``) against the GPU call
(``intensity.intensity_objects``, upload through result), three alternating runs each, on one BBBC039-like image with its objects, a
synthetic 1024^2 image and the synthetic 4096^2 image with 2000 objects.  ``measure.measure_objects`` WITH intensities runs on the same
objects in the same session as the yardstick: it reads the same bits and the same pixels, once.  The label form
(``intensity.intensity_labels``) is timed on the label map that ``rasterize_labels_gpu`` gives for the same objects; its host definition
passes over the whole image once per label and is not run at 4096^2 (unless --host-4096).

The launches alone (inputs on the device, no download) are timed by events on the stream: for the objects of each input, and for two
made-up sets of 64 disks each, one whose keys are staged in LDS (radius 35: 3 853 pixels) and one beyond SDSM_INTENSITY_LDS_KEYS (radius
37: 4 293 pixels), so that the cost of re-reading the image in every round of the selection is a number.

    python tools/time_intensity.py [--repeat 3] [--host-4096]
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from superdsm_amd import _capi, intensity, measure, render  # noqa: E402
from time_measure import compare, timed  # noqa: E402
from time_results import bbbc, synthetic  # noqa: E402


def same(x, y):
    return all(p.tobytes() == q.tobytes() for p, q in zip(x, y))


class Disk:
    def __init__(self, centre, radius):
        y, x = np.mgrid[-radius:radius + 1, -radius:radius + 1]
        self.fg_offset, self.fg_fragment = np.array([centre[0] - radius, centre[1] - radius]), y * y + x * x <= radius * radius


def disks(radius, side=1024, n=64):
    step = side // 8
    return [Disk((step // 2 + step * (k // 8), step // 2 + step * (k % 8)), radius) for k in range(n)]


def kernels_alone(name, objs, g, repeat):
    """The launches of sdsm_intensity_objects and of sdsm_measure_objects (with intensities) on the same fragments, by events on the stream."""
    import torch
    from superdsm_amd.postprocess import pack_fragments, _exclusive
    I = intensity._IntensitySet([g.shape], [np.ascontiguousarray(g, np.float64)])
    S, M = I.S, I.M
    boxes, words, packed, _ = pack_fragments(objs)
    n = len(boxes)
    n_q, num, den = I._quantiles(intensity.quantile_fractions(intensity.DEFAULT_QUANTILES))
    B = I.buffers(n, n_q)
    d_boxes, d_off, d_bits, d_rec = S._up(boxes), S._up(_exclusive(words)), S._up(np.concatenate(packed)), M.record_buffer(n)
    calls = {'sdsm_intensity_objects': lambda: S.L.sdsm_intensity_objects_multi(S.table, 1, n, None, S._p(d_boxes), S._p(d_off), S._p(d_bits), S._p(M.d_g), n_q, num,
                                                                                den, S._p(B['d_out']), S._p(B['d_order']), S._stream()),
             'sdsm_measure_objects': lambda: S.L.sdsm_measure_objects_multi(S.table, 1, n, None, S._p(d_boxes), S._p(d_off), S._p(d_bits), S._p(M.d_g), S._p(M.d_gmax),
                                                                            S._p(M.d_exp), S._p(d_rec), S._stream())}
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
        t = intensity.intensity_objects(objs, shp, g)
        print(f'{name}: {shp}, {len(objs)} objects of up to {int(t[0]["n_finite"].max())} pixels, {int((t[0]["n_finite"] > _capi.INTENSITY_LDS_KEYS).sum())} beyond '
              f'the {_capi.INTENSITY_LDS_KEYS} keys of LDS', flush=True)
        compare(name + ' intensity objects', lambda: intensity.intensity_objects_host(objs, shp, g), lambda: intensity.intensity_objects(objs, shp, g), a.repeat, equal=same)
        compare(name + ' measure objects with intensities (yardstick)', lambda: measure.measure_objects_host(objs, shp, g), lambda: measure.measure_objects(objs, shp, g),
                a.repeat, equal=lambda x, y: x.tobytes() == y.tobytes())
        compare(name + ' intensity labels', (lambda: intensity.intensity_labels_host(labels, g)) if host_labels else None, lambda: intensity.intensity_labels(labels, g),
                a.repeat, equal=same)
        td = [timed(lambda: intensity.derive(*t))[1] for _ in range(a.repeat)]
        print(f'{name + " derive (on the host, from the GPU result)":60s} host {statistics.median(td):10.1f} ms   ({", ".join(f"{v:.2f}" for v in td)})', flush=True)
        kernels_alone(name, objs, g, a.repeat)
    g = np.random.default_rng(5).random((1024, 1024))
    for radius, text in ((35, 'staged in LDS'), (37, 'beyond the key cap')):
        objs = disks(radius)
        assert same(intensity.intensity_objects(objs, g.shape, g), intensity.intensity_objects_host(objs, g.shape, g))
        kernels_alone(f'64 disks of {int(objs[0].fg_fragment.sum())} pixels ({text})', objs, g, a.repeat)


if __name__ == '__main__':
    main()
