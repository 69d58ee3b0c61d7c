"""Wall clock and launch time of the skeleton tables on the eight BBBC039-like label maps that tools/time_parts.py uses (what
``rasterize_labels_gpu`` gives for the ellipses of the workload's layouts) and on their objects, as one set: ``skeleton_labels_many`` and
``skeleton_objects_many`` (upload through result) beside the host definitions on the same inputs and beside ``depth_labels_many`` /
``depth_objects_many``, the library's other one-workgroup-per-object kernel and the yardstick here.  The three alternate, ``--repeat``
times after a warm-up; medians and the runs themselves are printed, GPU results are checked against the host definitions first.

The launches alone (objects on the device, no download) are timed by events on the stream, ``--inner`` launches per window, in
alternating windows of ``sdsm_skeleton_objects_multi`` and ``sdsm_depth_objects_multi`` (without intensities) on the same fragments; and
for three made-up sets of 256 objects each: discs of radius 30 (61 x 61, the wavefront path, 21 cycles), the same discs in 100 x 100
boxes (LDS path) and in 61 x 3300 boxes (workspace path).  Also printed: the split of the objects over the three paths and the largest
``cycles``.  Needs a GPU.

    python tools/time_skeleton.py [--repeat 5] [--inner 20]
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from superdsm_amd import _capi, depth, render, skeleton  # noqa: E402
from time_measure import timed  # noqa: E402
from time_results import bbbc  # noqa: E402

N_IMAGES = 8


class Piece:
    def __init__(self, offset, fragment):
        self.fg_offset, self.fg_fragment = np.asarray(offset), np.asarray(fragment, bool)


def same_objects(g, h):
    return all(a[0].tobytes() == b[0].tobytes() and all(np.array_equal(p, q) for p, q in zip(a[1], b[1])) for a, b in zip(g, h))


def same_labels(g, h):
    return all(a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) for a, b in zip(g, h))


def alternate(name, calls, repeat):
    """``calls``: (text, function) pairs run in turn ``repeat`` times after one warm-up of each GPU form; medians in ms."""
    times = {text: [] for text, _ in calls}
    for _ in range(repeat):
        for text, fn in calls:
            times[text].append(timed(fn)[1])
    for text, _ in calls:
        print(f'{name + " " + text:64s} {statistics.median(times[text]):10.2f} ms   (median of {repeat}; {", ".join(f"{t:.2f}" for t in times[text])})', flush=True)


def window(launch, inner):
    """Milliseconds per launch of ``inner`` launches between two events."""
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(inner):
        launch()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / inner


def kernels_alone(name, objects_per_image, shapes, inner, repeat):
    """The launches of sdsm_skeleton_objects_multi and sdsm_depth_objects_multi on the same set, by events on the stream."""
    from superdsm_amd.postprocess import pack_object_sets
    (obj_image, boxes, words, packed), _, _ = pack_object_sets(objects_per_image)
    n, n_im = len(boxes), len(shapes)
    K, D = skeleton._SkeletonSet(shapes), depth._DepthSet(shapes, None)
    S = K.S
    d_objects = S.upload_objects(obj_image, boxes, words, packed)
    BK, BD = K.buffers(boxes, words), D.buffers(boxes, depth.DEFAULT_SHELLS)
    wk, wd = K._workspace(BK, None), D._workspace(BD, None)

    def launch_skeleton():
        _capi.check(S.L.sdsm_skeleton_objects_multi(S.table, n_im, n, *map(S._p, d_objects), *wk, S._p(BK['d_out']), S._p(BK['d_skel']), S._stream()), 'sdsm_skeleton_objects_multi')

    def launch_depth():
        _capi.check(S.L.sdsm_depth_objects_multi(S.table, n_im, n, *map(S._p, d_objects), None, None, None, depth.DEFAULT_SHELLS, *wd, S._p(BD['d_out']), S._p(BD['d_shells']),
                                                 S._stream()), 'sdsm_depth_objects_multi')

    window(launch_skeleton, inner)
    window(launch_depth, inner)
    ts, td = [], []
    for _ in range(repeat):
        ts.append(window(launch_skeleton, inner))
        td.append(window(launch_depth, inner))
    paths = np.bincount(skeleton.path_of(boxes), minlength=3)
    cycles = S.records(BK['d_out'], n, _capi.SKELETON_RECORD_DTYPE)['cycles']
    print(f'{name}: {n} objects, paths wavefront / LDS / workspace {paths.tolist()}, largest cycles {int(cycles.max(initial=0))}', flush=True)
    for what, t in (('sdsm_skeleton_objects', ts), ('sdsm_depth_objects (yardstick)', td)):
        print(f'{name + " " + what + ": launch alone":64s} {statistics.median(t):10.4f} ms   (median of {repeat} windows of {inner}; {", ".join(f"{v:.4f}" for v in t)})', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this tool needs a GPU'
    datas = [bbbc(i) for i in range(N_IMAGES)]
    maps = [render.rasterize_labels_gpu(d).astype(np.int32) for d in datas]
    objs = [d['postprocessed_objects'] for d in datas]
    shapes = [m.shape for m in maps]
    host_l = [skeleton.skeleton_labels_host(m) for m in maps]
    host_o = [skeleton.skeleton_objects_host(o, s) for o, s in zip(objs, shapes)]
    assert same_labels(skeleton.skeleton_labels_many(maps), host_l) and same_objects(skeleton.skeleton_objects_many(objs, shapes), host_o), 'the GPU form differs from the host definition'
    depth.depth_labels_many(maps), depth.depth_objects_many(objs, shapes)                                                      # warm-up
    name = f'bbbc039_like x {N_IMAGES}'
    print(f'{name}: {sum(len(t) for t, _ in host_l)} labels, {sum(len(o) for o in objs)} objects, largest cycles {max(int(t["cycles"].max(initial=0)) for t, _ in host_l + host_o)}',
          flush=True)
    alternate(name + ' labels:', [('skeleton_labels_many (GPU, wall clock)', lambda: skeleton.skeleton_labels_many(maps)),
                                  ('depth_labels_many (GPU, wall clock, yardstick)', lambda: depth.depth_labels_many(maps)),
                                  ('skeleton_labels_host', lambda: [skeleton.skeleton_labels_host(m) for m in maps])], a.repeat)
    alternate(name + ' objects:', [('skeleton_objects_many (GPU, wall clock)', lambda: skeleton.skeleton_objects_many(objs, shapes)),
                                   ('depth_objects_many (GPU, wall clock, yardstick)', lambda: depth.depth_objects_many(objs, shapes)),
                                   ('skeleton_objects_host', lambda: [skeleton.skeleton_objects_host(o, s) for o, s in zip(objs, shapes)])], a.repeat)
    kernels_alone(name + ' objects', objs, shapes, a.inner, a.repeat)
    from superdsm_amd.measure import _LabelWindows
    K = skeleton._SkeletonSet(shapes)
    w = _LabelWindows(K.M, maps, 0, 'skeleton')
    print(f'{name} labels: {len(w.idx)} windows, paths wavefront / LDS / workspace {np.bincount(skeleton.path_of(w.boxes), minlength=3).tolist()}', flush=True)
    y, x = np.mgrid[-30:31, -30:31]
    disc = y * y + x * x <= 900
    mid = np.zeros((100, 100), bool)
    mid[20:81, 20:81] = disc
    far = np.zeros((61, 3300), bool)
    far[:, 1000:1061] = disc
    for fragment, text in ((disc, '256 discs of radius 30 (wavefront)'), (mid, '256 discs of radius 30 in 100 x 100 (LDS)'), (far, '256 discs of radius 30 in 61 x 3300 (workspace)')):
        pieces = [Piece((0, 0), fragment) for _ in range(256)]
        assert same_objects([skeleton.skeleton_objects(pieces[:2], (128, 3300))], [skeleton.skeleton_objects_host(pieces[:2], (128, 3300))])
        kernels_alone(text, [pieces], [(128, 3300)], max(a.inner // 4, 2), a.repeat)


if __name__ == '__main__':
    main()
