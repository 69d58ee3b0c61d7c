"""Launch time of the connected parts (``sdsm_parts_multi``: labelling, part map and label table; ``sdsm_parts_table_multi``: the part
records) under both adjacencies, on three scenes: the eight BBBC039-like label maps as one set (what ``rasterize_labels_gpu`` gives for
the ellipses of the workload's layouts), one 512 x 512 map and one 4096 x 4096 map of overlapping discs (later discs over earlier ones,
so labels come in pieces).  Maps on the device, no download; ``--inner`` launches between two events on the stream after a warm-up
window (a quarter as many on the largest scene).  Beside it, in alternating windows of the same process, the yardstick:
``sdsm_c2f_markers_multi`` on the foreground y = (labels > 0) of the same maps, the only other connected-component labelling of the
library (binary, 4-connected, one union per pixel pair in global memory, with the irregularity counts of its stage).

Every run is a fresh process: this program starts itself ``--runs`` times with ``--child``, one after the other, and reports per scene
the median over the runs and the runs themselves.  The part map of the first BBBC039-like image is checked against ``parts.parts_host``
before anything is timed.  Needs a GPU.

    python tools/time_parts.py [--runs 3] [--inner 20]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N_IMAGES = 8


def discs(side, n, seed):
    """``n`` discs of radius 6 .. 18 with the labels 1 .. n at random places of a side x side map, later ones over earlier ones."""
    rng = np.random.default_rng(seed)
    m = np.zeros((side, side), np.int32)
    for l in range(1, n + 1):
        rad = int(rng.integers(6, 19))
        r, c = (int(v) for v in rng.integers(rad, side - rad, 2))
        y, x = np.mgrid[-rad:rad + 1, -rad:rad + 1]
        m[r - rad:r + rad + 1, c - rad:c + rad + 1][y * y + x * x <= rad * rad] = l
    return m


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


def time_scene(name, maps, inner, repeat):
    """One JSON line per adjacency: the medians of ``repeat`` alternating windows of the three launches."""
    import torch
    from superdsm_amd import _capi, parts
    from superdsm_amd.render import _DeviceSet
    S = _DeviceSet([m.shape for m in maps])
    C, L, n = S.C, S.L, len(maps)
    d_map = S.pack(maps, np.int32)
    n_labels = [int(m.max()) + 1 for m in maps]
    rec_off = np.concatenate([[0], np.cumsum(n_labels)]).astype(np.int64)
    a_rec, a_lab = (C.c_int64 * n)(*[int(v) for v in rec_off[:n]]), (C.c_int32 * n)(*n_labels)
    ws_bytes = L.sdsm_parts_workspace_bytes_multi(S.table, n, a_rec, a_lab)
    d_ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=S.dev)
    d_rec = torch.empty(int(rec_off[-1]) * parts.LABEL_DTYPE.itemsize, dtype=torch.uint8, device=S.dev)
    d_part_map = torch.empty(S.total, dtype=torch.int32, device=S.dev)
    d_count, d_status = (torch.empty(n, dtype=torch.int32, device=S.dev) for _ in range(2))
    # the yardstick's buffers
    d_y = S.pack([(m > 0).astype(np.float64) for m in maps], np.float64)
    d_mask = torch.empty(S.total, dtype=torch.uint8, device=S.dev)
    d_markers = torch.empty(S.total, dtype=torch.int32, device=S.dev)
    d_n = torch.empty(n, dtype=torch.int32, device=S.dev)
    c2f_bytes = L.sdsm_c2f_markers_workspace_bytes_multi(S.table, n)
    d_c2f_ws = torch.empty((c2f_bytes + 7) // 8, dtype=torch.int64, device=S.dev)
    irregular = (C.c_double * n)(*[2.0] * n)                 # no component is irregular: every one is numbered

    def launch_c2f():
        _capi.check(L.sdsm_c2f_markers_multi(S.table, n, S._p(d_y), irregular, S._p(d_mask), S._p(d_markers), S._p(d_n), S._p(d_c2f_ws), c2f_bytes,
                                             S._stream()), 'sdsm_c2f_markers_multi')

    for connectivity in (4, 8):
        def launch_parts():
            _capi.check(L.sdsm_parts_multi(S.table, n, S._p(d_map), connectivity, a_rec, a_lab, S._p(d_rec), S._p(d_part_map), S._p(d_count), S._p(d_status),
                                           S._p(d_ws), ws_bytes, S._stream()), 'sdsm_parts_multi')

        window(launch_parts, inner)                          # warm-up; the counts size the part table
        assert not d_status.cpu().numpy().any()
        count = d_count.cpu().numpy()
        part_off = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
        a_part, a_k = (C.c_int64 * n)(*[int(v) for v in part_off[:n]]), (C.c_int32 * n)(*[int(v) for v in count])
        d_parts = torch.empty(max(int(part_off[-1]), 1) * parts.PART_DTYPE.itemsize, dtype=torch.uint8, device=S.dev)

        def launch_table():
            _capi.check(L.sdsm_parts_table_multi(S.table, n, S._p(d_map), S._p(d_part_map), a_part, a_k, S._p(d_parts), S._stream()), 'sdsm_parts_table_multi')

        window(launch_table, inner)
        window(launch_c2f, inner)
        tp, tt, tc = [], [], []
        for _ in range(repeat):                              # the three alternate
            tp.append(window(launch_parts, inner))
            tt.append(window(launch_table, inner))
            tc.append(window(launch_c2f, inner))
        print(json.dumps({'scene': name, 'connectivity': connectivity, 'pixels': int(sum(m.size for m in maps)), 'parts': int(count.sum()),
                          'c2f_components': int(d_n.cpu().numpy().sum()), 'parts_ms': statistics.median(tp), 'table_ms': statistics.median(tt),
                          'c2f_ms': statistics.median(tc)}), flush=True)


def child(inner, repeat):
    import torch
    from superdsm_amd import parts, render
    from time_results import bbbc
    assert torch.cuda.is_available(), 'this tool needs a GPU'
    maps = [render.rasterize_labels_gpu(bbbc(i)).astype(np.int32) for i in range(N_IMAGES)]
    for connectivity in (4, 8):
        got, want = parts.parts(maps[0], connectivity), parts.parts_host(maps[0], connectivity)
        assert np.array_equal(got[0], want[0]) and all(g.tobytes() == w.tobytes() for g, w in zip(got[1:], want[1:])), 'the GPU form differs from the host definition'
    time_scene('bbbc039_like x 8', maps, inner, repeat)
    time_scene('discs 512', [discs(512, 150, 21)], inner, repeat)
    time_scene('discs 4096', [discs(4096, 9600, 22)], max(inner // 4, 2), repeat)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return child(a.inner, a.repeat)
    runs = []
    for k in range(a.runs):                                  # fresh processes, one at a time; this one never opens the GPU
        out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--inner', str(a.inner), '--repeat', str(a.repeat)],
                             capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            sys.exit(f'run {k} failed ({out.returncode}):\n{out.stdout}\n{out.stderr}')
        runs.append([json.loads(line) for line in out.stdout.splitlines() if line.startswith('{')])
        print(f'run {k}: {len(runs[-1])} rows', flush=True)
    print('| scene | connectivity | pixels | parts | labelling + label table (ms) | part table (ms) | c2f markers (ms) |')
    print('|---|---|---|---|---|---|---|')
    for rows in zip(*runs):
        r = rows[0]
        cell = lambda key: f'{statistics.median(x[key] for x in rows):.3f} ({", ".join(f"{x[key]:.3f}" for x in rows)})'
        print(f'| {r["scene"]} | {r["connectivity"]} | {r["pixels"]} | {r["parts"]} | {cell("parts_ms")} | {cell("table_ms")} | {cell("c2f_ms")} |')


if __name__ == '__main__':
    main()
