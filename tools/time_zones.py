"""Launch time of the zone label maps (``sdsm_zones_multi``, k_zones) on the eight BBBC039-like label maps as one set, at max_d2 = 64,
1024 and 4096 with ``ring(0, max_d2)`` + ``core(4)`` asked for: maps on the device, no download, ``--inner`` launches between two events
on the stream, median of ``--repeat`` such windows after a warm-up window.  Beside it, in alternating windows of the same session, the
launch of the neighbourhood tables (``sdsm_neighbours_multi``) on the same maps at the same max_d2, which stages the same tiles, and
the host route the zone maps replace: ``scipy.ndimage.distance_transform_edt(labels == 0, return_indices=True)`` per image (the sum
over the eight images, median of ``--repeat`` runs).  The label maps are what ``rasterize_labels_gpu`` gives for the ellipses of the
workload's layouts.  The zone maps of the first image are checked against ``zones.zone_maps_host`` at the smallest reach before anything
is timed.  Needs a GPU.

    python tools/time_zones.py [--repeat 5] [--inner 20]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from superdsm_amd import _capi, neighbours, render, zones  # noqa: E402
from time_results import bbbc  # noqa: E402

REACHES = (64, 1024, 4096)
N_IMAGES = 8


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


def main():
    import torch
    from scipy import ndimage
    from superdsm_amd.render import _DeviceSet
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool needs a GPU'
    maps = [render.rasterize_labels_gpu(bbbc(i)).astype(np.int32) for i in range(N_IMAGES)]
    print(f'{N_IMAGES} label maps: shapes {sorted(set(m.shape for m in maps))}, {sum(int(m.max()) for m in maps)} labels, '
          f'{sum(m.size for m in maps)} pixels, {sum(int((m > 0).sum()) for m in maps)} of them labelled', flush=True)
    check = [zones.Zone.ring(0, REACHES[0]), zones.Zone.core(4)]
    assert all(np.array_equal(g, h) for g, h in zip(zones.zone_maps(maps[0], check), zones.zone_maps_host(maps[0], check))), 'the GPU maps differ from the host definition'

    S = _DeviceSet([m.shape for m in maps])
    C, n = S.C, len(maps)
    d_map = S.pack(maps, np.int32)
    d_zone = torch.empty(2 * S.total, dtype=torch.int32, device=S.dev)
    d_status = torch.empty(2 * n, dtype=torch.int32, device=S.dev)
    n_labels = [int(m.max()) + 1 for m in maps]
    cap = 1 << 16
    rec_off = np.concatenate([[0], np.cumsum(n_labels)]).astype(np.int64)
    d_rec = torch.empty(int(rec_off[-1]) * neighbours.LABEL_DTYPE.itemsize, dtype=torch.uint8, device=S.dev)
    d_keys = torch.empty(n * cap, dtype=torch.int64, device=S.dev)
    d_min, d_contact = (torch.empty(n * cap, dtype=torch.int32, device=S.dev) for _ in range(2))
    a_rec, a_lab = (C.c_int64 * n)(*[int(v) for v in rec_off[:n]]), (C.c_int32 * n)(*n_labels)
    a_off, a_cap = (C.c_int64 * n)(*[i * cap for i in range(n)]), (C.c_int64 * n)(*[cap] * n)

    rows = []
    for max_d2 in REACHES:
        specs = np.array([z.spec() for z in (zones.Zone.ring(0, max_d2), zones.Zone.core(4))], np.int32).view(_capi.ZONE_SPEC_DTYPE)

        def launch_zones():
            _capi.check(S.L.sdsm_zones_multi(S.table, n, S._p(d_map), max_d2, 2, specs.ctypes.data_as(C.c_void_p), S.total, None, None, S._p(d_zone),
                                             S._p(d_status), S._stream()), 'sdsm_zones_multi')

        def launch_neighbours():
            _capi.check(S.L.sdsm_neighbours_multi(S.table, n, S._p(d_map), max_d2, a_rec, a_lab, S._p(d_rec), a_off, a_cap, S._p(d_keys), S._p(d_min),
                                                  S._p(d_contact), S._p(d_status), S._stream()), 'sdsm_neighbours_multi')

        window(launch_zones, a.inner)                         # warm-up of both
        assert not d_status.cpu().numpy()[:n].any()
        window(launch_neighbours, a.inner)
        assert not d_status.cpu().numpy().any(), 'a pair table of the neighbourhood launch was too small'
        tz, tn = [], []
        for _ in range(a.repeat):                             # the two alternate
            tz.append(window(launch_zones, a.inner))
            tn.append(window(launch_neighbours, a.inner))
        th = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            for m in maps:
                ndimage.distance_transform_edt(m == 0, return_indices=True)
            th.append(1e3 * (time.perf_counter() - t0))
        rows.append((max_d2, statistics.median(tz), statistics.median(tn), statistics.median(th)))
        print(f'max_d2 {max_d2:5d}: zones {rows[-1][1]:8.3f} ms ({", ".join(f"{t:.3f}" for t in tz)})   neighbours {rows[-1][2]:8.3f} ms '
              f'({", ".join(f"{t:.3f}" for t in tn)})   scipy edt with indices, {N_IMAGES} images {rows[-1][3]:8.1f} ms ({", ".join(f"{t:.1f}" for t in th)})', flush=True)
    print('| max_d2 | zones launch (ms) | neighbours launch (ms) | SciPy EDT with indices, 8 images (ms) |')
    print('|---|---|---|---|')
    for r in rows:
        print(f'| {r[0]} | {r[1]:.3f} | {r[2]:.3f} | {r[3]:.1f} |')


if __name__ == '__main__':
    main()
