"""Wall clock of the neighbourhood tables of one label map: the host definitions (``neighbours.neighbour_labels_host`` and
``neighbour_pairs_host``, the map against its shift for every offset of the half disk in NumPy) against the GPU form
(``neighbours.neighbour_tables``), upload through sorted tables, median of alternating runs, on one BBBC039-like image, a synthetic
1024^2 image and the synthetic 4096^2 image, at max_d2 = 2, 100 and 4096.  The label maps are what ``rasterize_labels_gpu`` gives for
the ellipses of the workload's layout.  The host definitions cost (offsets x pixels): they run ``--repeat`` times up to 2e9, once up
to ``--host-limit`` (default 2e10) and are reported as not run beyond.  ``compare.overlap_pairs`` (the map against itself) and
``boundary.label_boundaries`` of the same map in the same session are the yardsticks for "one pass over a label map".  The launches
alone (map on the device, no download) are timed by events on the stream.

    python tools/time_neighbours.py [--repeat 3] [--host-limit 2e10]
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from superdsm_amd import _capi, boundary, compare, neighbours, render  # noqa: E402
from time_measure import timed  # noqa: E402
from time_results import bbbc, synthetic  # noqa: E402

REACHES = (2, 100, 4096)


def same(h, g):
    return all(x.tobytes() == y.tobytes() for x, y in zip(h, g))


def run(name, host, host_runs, gpu, repeat):
    gpu()                                                     # warm-up: library load, first launch
    th, tg = [], []
    for k in range(repeat):                                   # the two alternate, so that drift of the host hits both
        g = timed(gpu)
        tg.append(g[1])
        if k < host_runs:
            h = timed(host)
            assert same(h[0], g[0]), name + ': the GPU tables differ from the host definitions'
            th.append(h[1])
    hs = f'host {statistics.median(th):10.2f} ms ({", ".join(f"{t:.2f}" for t in th)})' if th else 'host not run'
    print(f'{name:44s} {hs}   gpu {statistics.median(tg):9.2f} ms ({", ".join(f"{t:.2f}" for t in tg)})', flush=True)


def yardsticks(name, labels, repeat):
    for what, fn in (('overlap_pairs (the map against itself)', lambda: compare.overlap_pairs(labels, labels)), ('label_boundaries', lambda: boundary.label_boundaries(labels))):
        fn()
        t = [timed(fn)[1] for _ in range(repeat)]
        print(f'{name + ": " + what:60s} gpu {statistics.median(t):9.2f} ms ({", ".join(f"{v:.2f}" for v in t)})', flush=True)


def launches_alone(name, labels, repeat):
    import torch
    from superdsm_amd.render import _DeviceSet
    S = _DeviceSet([labels.shape])
    n_labels, cap = int(labels.max()) + 1, 1 << 16
    d_map = S.pack([labels.astype(np.int32)], np.int32)
    d_rec = torch.empty(n_labels * neighbours.LABEL_DTYPE.itemsize, dtype=torch.uint8, device=S.dev)
    d_keys = torch.empty(cap, dtype=torch.int64, device=S.dev)
    d_min, d_contact, d_status = (torch.empty(n, dtype=torch.int32, device=S.dev) for n in (cap, cap, 2))
    out = []
    for max_d2 in REACHES:
        ms = []
        for _ in range(repeat + 1):                           # (the first is the warm-up)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            _capi.check(S.L.sdsm_neighbours(labels.shape[0], labels.shape[1], S._p(d_map), max_d2, n_labels, S._p(d_rec), cap, S._p(d_keys), S._p(d_min),
                                            S._p(d_contact), S._p(d_status), S._stream()), 'sdsm_neighbours')
            ev[1].record()
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        assert d_status.cpu().numpy().tolist() == [0, 0]
        out.append(f'max_d2 {max_d2}: {statistics.median(ms[1:]):.3f} ms ({", ".join(f"{t:.3f}" for t in ms[1:])})')
    print(f'{name + ": launches alone":44s} ' + ', '.join(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--host-limit', type=float, default=2e10, help='largest (offsets x pixels) at which the host definitions still run, once')
    a = ap.parse_args()
    for name, d in (('bbbc039_like', bbbc(0)), ('synthetic1024 (125 objects)', synthetic(1024, 125)), ('synthetic4096 (2000 objects)', synthetic(4096, 2000))):
        labels = render.rasterize_labels_gpu(d)
        for max_d2 in REACHES:
            table, pairs = neighbours.neighbour_tables(labels, max_d2)
            dv = neighbours.derive(table, pairs)
            print(f'{name}: {labels.shape}, max_d2 {max_d2}: {len(dv)} labels, {len(pairs)} pairs, {int((pairs["contact_edges"] > 0).sum())} touching, '
                  f'{int(table["boundary"].sum())} boundary pixels, {int(table["close"].sum())} close', flush=True)
            cost = len(neighbours.halfplane_offsets(max_d2)) * labels.size
            host_runs = a.repeat if cost <= 2e9 else 1 if cost <= a.host_limit else 0
            run(f'{name}, max_d2 {max_d2}', lambda: (neighbours.neighbour_labels_host(labels, max_d2), neighbours.neighbour_pairs_host(labels, max_d2)), host_runs,
                lambda: neighbours.neighbour_tables(labels, max_d2), a.repeat)
        yardsticks(name, labels, a.repeat)
        launches_alone(name, labels, a.repeat)


if __name__ == '__main__':
    main()
