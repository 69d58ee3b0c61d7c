"""Diagnostic (needs a build with -DSDSM_PROFILE -DSDSM_PROFILE_WALL): the workgroups of sdsm_k_setup on the wall clock -- how many are
resident over time, which ten end last (N, M and their phase times) and the mean time of a workgroup.  The stamps of the last of three
launches are reported.   usage: SDSM_HIP_LIB=superdsm_amd/libsdsm_hip_prof.so python tools/setup_timeline.py <workload> [images]"""
import ctypes as C, os, sys, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from superdsm_amd import _capi, engine, testing
wl = sys.argv[1]
nimg = int(sys.argv[2]) if len(sys.argv) > 2 else 1
scenes = [testing.make_scene(wl, max_size=3, layout_index=k % 8 if wl == 'bbbc039_like' else 0) for k in range(nimg)]
fps = [fp for sc in scenes for fp in sc['footprints']]
image_of = np.concatenate([np.full(len(sc['footprints']), k, np.int32) for k, sc in enumerate(scenes)])
imgs = [engine.DeviceImage(sc['y'], None, sc['atoms'], sc['dsm_cfg']['background_margin']) for sc in scenes]
batch = engine.Batch(imgs if nimg > 1 else imgs[0], fps, scenes[0]['dsm_cfg'], image_of=image_of if nimg > 1 else None)
n = len(fps)
prof = torch.zeros(n * 26, dtype=torch.int64, device='cuda')        # 16 n solve counters | 8 n setup counters | 2 n wall stamps of the setup workgroups
_capi.lib().sdsm_set_debug_buffer(C.c_void_p(prof.data_ptr()))
for _ in range(3):
    prof.zero_()
    batch.launch()
    torch.cuda.synchronize()
recs = batch.records()
buf = prof.cpu().numpy()
phase = buf[16 * n:24 * n].reshape(-1, 8).astype(np.float64) / 2400.0          # us (2.4 GHz shader clock)
wall = buf[24 * n:].reshape(-1, 2).astype(np.float64) / 100.0                   # us (100 MHz wall clock)
have = wall[:, 1] > 0
t0 = wall[have, 0].min()
start, end = wall[:, 0] - t0, wall[:, 1] - t0
N, M = recs['n_pixels'], recs['n_deform']
print(f'{wl} x {nimg}: {n} candidates, {have.sum()} setup workgroups with stamps; kernel span (first start .. last end) {end[have].max():.0f} us')
print(f'mean workgroup time {(end - start)[have].mean():.1f} us, median {np.median((end - start)[have]):.1f} us, sum {(end - start)[have].sum() / 1e3:.1f} ms')
print('resident setup workgroups over time (start of the 50 us bin: workgroups resident at its start)')
span = end[have].max()
print('  ' + '  '.join(f'{int(t)}: {int(((start <= t) & (end > t) & have).sum())}' for t in np.arange(0, span, 50.0)))
print('the ten workgroups that end last: end, start [us] | N, M | scan, coordinates, greedy grid, sort of the grid, run lengths + counting sort, rows, envelope [us]')
for i in np.argsort(-np.where(have, end, -1))[:10]:
    print(f'  end {end[i]:7.1f} start {start[i]:7.1f} | N={N[i]:6d} M={M[i]:4d} | ' + ' '.join(f'{phase[i, k]:6.1f}' for k in range(7)))
for lo, hi in ((0, 500), (500, 1000), (1000, 2500), (2500, 4096), (4096, 1 << 30)):
    sel = have & (N >= lo) & (N < hi)
    if sel.any():
        print(f'  regions of {lo} <= N < {hi}: {sel.sum()} workgroups, mean {(end - start)[sel].mean():.1f} us, last end {end[sel].max():.0f} us')
