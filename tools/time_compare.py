"""Wall clock of the contingency table of two label maps: the host definition (``compare.overlap_pairs_host``, ``np.unique`` over H * W
64-bit keys) against the GPU form (``compare.overlap_pairs`` / ``_many``), upload through table, median of alternating runs, on one
BBBC039-like image, the set of 8, a synthetic 1024^2 image and the synthetic 4096^2 image (the host form runs there too).  The label
maps are what ``rasterize_labels_gpu`` gives for the ellipses of the workload's layout and for the same layout moved by two pixels.
The launch alone (inputs on the device, the table cleared by the call, no download) is timed by events on the stream.

    python tools/time_compare.py [--repeat 3]
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from superdsm_amd import _capi, compare, render  # noqa: E402
from time_measure import timed  # noqa: E402
from time_results import Obj, bbbc, synthetic  # noqa: E402


def moved(d, by=2):
    """The objects of ``d`` two pixels to the right (clipped at the image's edge)."""
    W = d['g_raw'].shape[1]
    objs = []
    for o in d['postprocessed_objects']:
        c0 = int(o.fg_offset[1]) + by
        frag = o.fg_fragment[:, :max(0, min(o.fg_fragment.shape[1], W - c0))]
        if frag.any():
            objs.append(Obj((int(o.fg_offset[0]), c0), frag))
    return {'g_raw': d['g_raw'], 'postprocessed_objects': objs}


def run(name, host, gpu, repeat):
    gpu()                                                     # warm-up: library load, first launch
    th, tg = [], []
    for _ in range(repeat):                                   # the two alternate, so that drift of the host hits both
        h, g = timed(host), timed(gpu)
        same = all(x.tobytes() == y.tobytes() for x, y in zip(h[0], g[0])) if isinstance(h[0], list) else h[0].tobytes() == g[0].tobytes()
        assert same, name + ': the GPU table differs from the host definition'
        th.append(h[1])
        tg.append(g[1])
    print(f'{name:44s} host {statistics.median(th):9.2f} ms ({", ".join(f"{t:.2f}" for t in th)})   gpu {statistics.median(tg):9.2f} ms '
          f'({", ".join(f"{t:.2f}" for t in tg)})', flush=True)


def launch_alone(name, a, b, capacity, repeat):
    import torch
    S = render._DeviceSet([a.shape])
    d_a, d_b = S.pack([a.astype(np.int32)], np.int32), S.pack([b.astype(np.int32)], np.int32)
    d_keys, d_counts = (torch.empty(capacity, dtype=torch.int64, device=S.dev) for _ in range(2))
    d_status = torch.empty(2, dtype=torch.int32, device=S.dev)
    ms = []
    for _ in range(repeat + 1):                               # (the first is the warm-up)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _capi.check(S.L.sdsm_overlap_pairs(a.shape[0], a.shape[1], S._p(d_a), S._p(d_b), capacity, S._p(d_keys), S._p(d_counts), S._p(d_status), S._stream()),
                    'sdsm_overlap_pairs')
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    assert d_status.cpu().numpy().tolist() == [0, 0]
    print(f'{name + ": clear + launch alone":44s} gpu {statistics.median(ms[1:]):9.3f} ms ({", ".join(f"{t:.3f}" for t in ms[1:])}), {capacity} slots', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    a = ap.parse_args()
    one, eight = bbbc(0), [bbbc(i) for i in range(8)]
    for name, d in (('bbbc039_like', one), ('synthetic1024 (125 objects)', synthetic(1024, 125)), ('synthetic4096 (2000 objects)', synthetic(4096, 2000))):
        actual, expected = render.rasterize_labels_gpu(d), render.rasterize_labels_gpu(moved(d))
        info = {}
        pairs = compare.overlap_pairs(actual, expected, info=info)
        s = compare.scores(pairs)
        print(f'{name}: {actual.shape}, {s["n_actual"]} / {s["n_expected"]} labels, {len(pairs)} pairs, {info["capacity"][0]} slots, SEG {s["seg"]:.4f}, '
              f'mean AP {s["mean_ap"]:.4f}', flush=True)
        run(name, lambda: compare.overlap_pairs_host(actual, expected), lambda: compare.overlap_pairs(actual, expected), a.repeat)
        launch_alone(name, actual, expected, info['capacity'][0], a.repeat)
    actual, expected = render.rasterize_labels_many(eight), render.rasterize_labels_many([moved(d) for d in eight])
    run('8 x bbbc039_like: host loop / gpu set', lambda: [compare.overlap_pairs_host(x, y) for x, y in zip(actual, expected)],
        lambda: compare.overlap_pairs_many(actual, expected), a.repeat)
    run('8 x bbbc039_like: host loop / gpu per image', lambda: [compare.overlap_pairs_host(x, y) for x, y in zip(actual, expected)],
        lambda: [compare.overlap_pairs(x, y) for x, y in zip(actual, expected)], a.repeat)


if __name__ == '__main__':
    main()
