"""Wall clock of the texture tables: the host definition (``texture.texture_objects_host``) against the GPU call
(``texture.texture_objects``, upload through result), three alternating runs each, on one BBBC039-like image with its objects, a
synthetic 1024^2 image and the synthetic 4096^2 image with 2000 objects, at 8, 64 and 256 levels over the finite range of the image and
the default offsets.  ``intensity.intensity_objects`` runs on the same objects in the same session as the yardstick: it reads the same
bits and the same pixels.  ``derive`` is timed on the GPU result.

The launches alone (inputs on the device, no download) are timed by events on the stream, for the objects of each input at each level
count, and at 256 levels for the same objects over a flat image (every pair in one cell: the contended LDS add) and over a noise image
(the pairs spread over the triangle), for the contention question of DESIGN.md section 5.

    python tools/time_texture.py [--repeat 3] [--skip-host-4096]
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from superdsm_amd import _capi, intensity, texture  # noqa: E402
from time_measure import compare, timed  # noqa: E402
from time_results import bbbc, synthetic  # noqa: E402

LEVELS = (8, 64, 256)


def same(x, y):
    return all(p.tobytes() == q.tobytes() for p, q in zip(x, y))


def kernels_alone(name, objs, g, levels, repeat):
    """The launches of sdsm_texture_objects (the pair kernel, the scan and the gather), by events on the stream."""
    import torch
    from superdsm_amd.postprocess import pack_fragments, _exclusive
    T = texture._TextureSet([g.shape], [np.ascontiguousarray(g, np.float64)], [texture.image_edges(g, levels) if np.ptp(g) > 0 else texture.uniform_edges(0, 1, levels)],
                            texture.check_offsets(texture.DEFAULT_OFFSETS))
    S = T.S
    boxes, words, packed, _ = pack_fragments(objs)
    n = len(boxes)
    slot_off = T.slot_offsets(boxes)
    B = T.buffers(n, int(slot_off[-1]))
    d_boxes, d_off, d_bits, d_slot_off = S._up(boxes), S._up(_exclusive(words)), S._up(np.concatenate(packed)), S._up(slot_off)
    call = lambda: S.L.sdsm_texture_objects_multi(S.table, 1, n, None, S._p(d_boxes), S._p(d_off), S._p(d_bits), S._p(T.M.d_g), T.levels, S._p(T.d_edges), T.n_o,
                                                  T.c_offsets, S._p(d_slot_off), S._p(B['d_slots']), S._p(B['d_out']), S._p(B['d_pairs']), S._p(B['d_entries']), S._stream())
    ms = []
    for _ in range(repeat + 1):                               # (the first is the warm-up)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _capi.check(call(), 'sdsm_texture_objects')
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    print(f'{name + f" G = {levels}: launches alone":64s} gpu {statistics.median(ms[1:]):9.3f} ms   (median of {repeat}; {", ".join(f"{t:.3f}" for t in ms[1:])})', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--skip-host-4096', action='store_true', help='do not run the host definition on the 4096^2 image')
    a = ap.parse_args()
    inputs = [('bbbc039_like', bbbc(0), True), ('synthetic1024 (125 objects)', synthetic(1024, 125), True),
              ('synthetic4096 (2000 objects)', synthetic(4096, 2000), not a.skip_host_4096)]
    for name, d, host in inputs:
        g, shp, objs = d['g_raw'], d['g_raw'].shape, d['postprocessed_objects']
        print(f'{name}: {shp}, {len(objs)} objects of up to {max(int(o.fg_fragment.sum()) for o in objs)} pixels', flush=True)
        compare(name + ' intensity objects (yardstick)', None, lambda: intensity.intensity_objects(objs, shp, g), a.repeat, equal=same)
        for G in LEVELS:
            edges = texture.image_edges(g, G)
            compare(f'{name} texture objects G = {G}', (lambda: texture.texture_objects_host(objs, shp, g, edges)) if host else None,
                    lambda: texture.texture_objects(objs, shp, g, edges), a.repeat, equal=same)
            t = texture.texture_objects(objs, shp, g, edges)
            td = [timed(lambda: texture.derive(*t, offsets=texture.DEFAULT_OFFSETS))[1] for _ in range(a.repeat)]
            print(f'{f"{name} derive G = {G} ({len(t[2])} entries, on the host)":64s} host {statistics.median(td):10.1f} ms   ({", ".join(f"{v:.2f}" for v in td)})', flush=True)
            kernels_alone(name, objs, g, G, a.repeat)
        rng = np.random.default_rng(9)
        kernels_alone(name + ' over a flat image', objs, np.full(shp, 0.5), 256, a.repeat)
        kernels_alone(name + ' over a noise image', objs, rng.random(shp), 256, a.repeat)


if __name__ == '__main__':
    main()
