"""Wall clock of the boundary-distance table of two label maps: the host definition (``boundary.pair_distances_host``, every query pixel
against every boundary pixel in NumPy) against the GPU form (``boundary.pair_distances`` / ``_many``), upload through table, median of
alternating runs, on one BBBC039-like image, the set of 8, a synthetic 1024^2 image and the synthetic 4096^2 image.  The label maps are
what ``rasterize_labels_gpu`` gives for the ellipses of the workload's layout and for the same layout moved by two pixels.  The host
definition compares the whole image with a label once per pair, which takes minutes at 4096^2 with 2000 pairs: it runs there only with
``--host-4096`` and is otherwise reported as not run.  The launches alone (maps on the device, no download) are timed by events on the
stream, and the steps of one GPU call by the wall clock with a synchronisation after each.

    python tools/time_boundary.py [--repeat 3] [--host-4096]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from superdsm_amd import _capi, boundary, compare, render  # noqa: E402
from time_compare import moved  # noqa: E402
from time_measure import timed  # noqa: E402
from time_results import bbbc, synthetic  # noqa: E402


def same(h, g):
    return all(x.tobytes() == y.tobytes() for x, y in zip(h, g)) if isinstance(h, list) else h.tobytes() == g.tobytes()


def run(name, host, gpu, repeat):
    gpu()                                                     # warm-up: library load, first launch
    th, tg = [], []
    for _ in range(repeat):                                   # the two alternate, so that drift of the host hits both
        g = timed(gpu)
        tg.append(g[1])
        if host is not None:
            h = timed(host)
            assert same(h[0], g[0]), name + ': the GPU table differs from the host definition'
            th.append(h[1])
    hs = f'host {statistics.median(th):10.2f} ms ({", ".join(f"{t:.2f}" for t in th)})' if th else 'host not run'
    print(f'{name:44s} {hs}   gpu {statistics.median(tg):9.2f} ms ({", ".join(f"{t:.2f}" for t in tg)})', flush=True)


def steps(name, a, b, repeat):
    """The steps of one GPU call, each closed by a synchronisation (so their sum exceeds the call's own wall clock a little)."""
    import torch
    a32, b32 = a.astype(np.int32), b.astype(np.int32)
    rows = []
    for _ in range(repeat):
        t = [time.perf_counter()]

        def lap():
            torch.cuda.synchronize()
            t.append(time.perf_counter())
        B = boundary._BoundarySet([a32], [b32])
        lap()                                                 # pack, upload, counts and lists of both maps
        tables = B.overlap(compare.DEFAULT_CAPACITY)
        lap()                                                 # contingency table: launch and download
        counts = B.counts()
        lap()                                                 # counts of both maps: 2 x 512 KB down
        pairs = [boundary._default_pairs(tables[0])]
        items = boundary.work_items(np.concatenate([np.zeros((len(pairs[0]), 1), np.int64), pairs[0], np.zeros((len(pairs[0]), 1), np.int64)], axis=1), *counts)
        lap()                                                 # the work list on the host (built again inside distances())
        B.distances(pairs)
        lap()                                                 # work list, upload, launch, records down
        rows.append([1e3 * (y - x) for x, y in zip(t[:-1], t[1:])])
    med = [statistics.median(c) for c in zip(*rows)]
    print(f'{name + ": steps":44s} upload+counts+lists {med[0]:.2f}, overlap table {med[1]:.2f}, counts down {med[2]:.2f}, work list {med[3]:.2f} '
          f'({len(items)} items), distances {med[4]:.2f} ms', flush=True)


def launches_alone(name, a, b, repeat):
    import torch
    B = boundary._BoundarySet([a.astype(np.int32)], [b.astype(np.int32)])
    S, L = B.S, _capi.BOUNDARY_MAX_LABELS
    pairs = boundary._default_pairs(B.overlap(compare.DEFAULT_CAPACITY)[0])
    rows = np.zeros((len(pairs), 4), np.int32)
    rows[:, 1:3] = pairs
    items = boundary.work_items(rows, *B.counts())
    d_rows, d_items = S._up(rows), S._up(items)
    d_rec = torch.empty(len(rows) * 64, dtype=torch.uint8, device=S.dev)
    ms = {'counts + lists (one map)': [], 'distances': []}
    for _ in range(repeat + 1):                               # (the first is the warm-up)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        _capi.check(S.L.sdsm_label_pixel_counts_multi(S.table, 1, S._p(B.d_map[0]), S._p(B.d_counts[0]), S._p(B.d_bad), S._stream()), 'counts')
        _capi.check(S.L.sdsm_label_pixel_lists_multi(S.table, 1, S._p(B.d_map[0]), S._p(B.d_counts[0]), S._p(B.d_start[0]), S._p(B.d_cursor),
                                                     S._p(B.d_list[0]), S._stream()), 'lists')
        ev[1].record()
        _capi.check(S.L.sdsm_pair_distances_multi(S.table, 1, S._p(B.d_map[0]), S._p(B.d_map[1]), S._p(B.d_counts[0]), S._p(B.d_counts[1]), S._p(B.d_start[0]),
                                                  S._p(B.d_start[1]), S._p(B.d_list[0]), S._p(B.d_list[1]), len(rows), S._p(d_rows), len(items), S._p(d_items),
                                                  S._p(d_rec), S._stream()), 'distances')
        ev[2].record()
        torch.cuda.synchronize()
        ms['counts + lists (one map)'].append(ev[0].elapsed_time(ev[1]))
        ms['distances'].append(ev[1].elapsed_time(ev[2]))
    print(f'{name + ": launches alone":44s} ' + ', '.join(f'{k} {statistics.median(v[1:]):.3f} ms ({", ".join(f"{t:.3f}" for t in v[1:])})' for k, v in ms.items())
          + f', {len(rows)} pairs, {len(items)} items', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--host-4096', action='store_true', help='run the host definition on the 4096^2 image as well (minutes)')
    a = ap.parse_args()
    one, eight = bbbc(0), [bbbc(i) for i in range(8)]
    for name, d, with_host in (('bbbc039_like', one, True), ('synthetic1024 (125 objects)', synthetic(1024, 125), True),
                               ('synthetic4096 (2000 objects)', synthetic(4096, 2000), a.host_4096)):
        actual, expected = render.rasterize_labels_gpu(d), render.rasterize_labels_gpu(moved(d))
        s = boundary.compare_boundaries(actual, expected)
        print(f'{name}: {actual.shape}, {s["n_expected"]} expected labels, {len(s["pairs"])} pairs, mean Hausdorff {s["mean_hausdorff"]:.4f}, '
              f'mean NSD {s["mean_nsd"]:.4f}, {s["n_without_partner"]} without partner', flush=True)
        run(name, (lambda: boundary.pair_distances_host(actual, expected)) if with_host else None, lambda: boundary.pair_distances(actual, expected), a.repeat)
        steps(name, actual, expected, a.repeat)
        launches_alone(name, actual, expected, a.repeat)
    actual, expected = render.rasterize_labels_many(eight), render.rasterize_labels_many([moved(d) for d in eight])
    run('8 x bbbc039_like: host loop / gpu set', lambda: [boundary.pair_distances_host(x, y) for x, y in zip(actual, expected)],
        lambda: boundary.pair_distances_many(actual, expected), a.repeat)
    run('8 x bbbc039_like: host loop / gpu per image', None, lambda: [boundary.pair_distances(x, y) for x, y in zip(actual, expected)], a.repeat)


if __name__ == '__main__':
    main()
