"""Wall clock of the coarse-to-fine region analysis, phase by phase, on the 8 BBBC039-like images, synthetic512 and synthetic 4096²:
markers and EDT, cluster flood, host split logic, energy rounds (count, plans and candidates per round, time), total.  With --host, the
restatement (SciPy markers and EDT, Python heap flood, CPU-oracle energies one request at a time) on the same inputs, for comparison.

    python tools/time_c2f.py [--host] [--skip-4096] [--host-4096]
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import scipy.ndimage as ndi

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from superdsm_amd import c2freganal as cr, synth  # noqa: E402


def images(skip_4096):
    spec = synth.WORKLOADS['bbbc039_like']
    for i in range(8):
        shape, layout = synth.bbbc039_like_layout(spec['seed'], i)
        yield f'bbbc039_like[{i}]', synth.offset_image(synth.render_image(shape, layout, spec['seed'] + 7919 * i), spec['scale'])
    for w in ('synthetic512',) + (() if skip_4096 else ('synthetic4096',)):
        s = synth.WORKLOADS[w]
        layout = synth.random_layout(s['shape'], s['n'], s['radius'], s['seed'], min_sep={'synthetic4096': 0.6, 'synthetic512': 1.2}[w])
        yield w, synth.offset_image(synth.render_image(s['shape'], layout, s['seed']), s['scale'])


def oracle_energy(y_crop, mask_crop, atoms_map, footprint, dsm_cfg):
    from oracle import oracle
    near = ndi.distance_transform_edt(y_crop <= 0) <= dsm_cfg['background_margin']
    m = np.isin(atoms_map, list(footprint)) & mask_crop & near
    vals = y_crop[m]
    if (vals > 0).all() or (vals < 0).all():
        return None
    cfg = {k: v for k, v in dsm_cfg.items() if k in ('scale', 'epsilon', 'alpha', 'smooth_subsample', 'gaussian_shape_multiplier', 'init')}
    cfg['smooth_amount'] = np.inf
    return oracle.cvxprog(y_crop, m, cfg)[1]['energy'] / m.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--host', action='store_true', help='also time the host restatement with CPU-oracle energies')
    ap.add_argument('--host-4096', action='store_true', help='include synthetic 4096² in the host restatement (slow)')
    ap.add_argument('--skip-4096', action='store_true')
    a = ap.parse_args()
    cfg = synth.dsm_config_for_scale(10, 0.00033)
    params = dict(min_atom_radius=int(0.33 * 10 * math.sqrt(2)))
    cr.region_analysis_gpu(next(images(True))[1], cfg, **params)             # warm-up: library load, first launches
    for name, y in images(a.skip_4096):
        out, st = cr.region_analysis_gpu(y, cfg, **params)
        r = st['rounds']
        print(f'{name} {y.shape[0]}x{y.shape[1]}: clusters {st["clusters"]}, atoms {int(out["atoms"].max())} | '
              f'markers+EDT {1e3 * st["markers_edt_s"]:.1f} ms, flood {1e3 * st["flood_s"]:.1f} ms, '
              f'host split logic {1e3 * st["host_split_s"]:.1f} ms, assembly {1e3 * st["assemble_s"]:.1f} ms, '
              f'energy rounds {len(r)} ({1e3 * st["energy_s"]:.1f} ms; plans/round max {max((x["plans"] for x in r), default=0)}, '
              f'candidates/round {min((x["candidates"] for x in r), default=0)}..{max((x["candidates"] for x in r), default=0)}, '
              f'launches {st["launches"]}, re-solved {sum(x["resolved"] for x in r)}) | total {1e3 * st["total_s"]:.1f} ms', flush=True)
        if a.host and (y.size < 4096 * 4096 or a.host_4096):
            t0 = time.perf_counter()
            ym, cm = cr.cluster_markers_host(y, 0.2)
            t1 = time.perf_counter()
            d = ndi.distance_transform_edt(cm == 0)
            t2 = time.perf_counter()
            cr.watershed(d, cm)
            t3 = time.perf_counter()
            host = cr.region_analysis_host(y, cfg, energy=oracle_energy, **params)
            t4 = time.perf_counter()
            same = np.array_equal(host['atoms'], out['atoms'])
            print(f'    host restatement: markers {1e3 * (t1 - t0):.1f} ms, EDT {1e3 * (t2 - t1):.1f} ms, heap flood {1e3 * (t3 - t2):.1f} ms, '
                  f'total with oracle energies {t4 - t3:.2f} s (atoms equal to the GPU path: {same})', flush=True)


if __name__ == '__main__':
    main()
