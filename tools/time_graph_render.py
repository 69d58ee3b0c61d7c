"""Times the y-map, coloured-label and adjacency-graph pictures, upload through result, against their *_host definitions (DESIGN.md
section 8): one BBBC039-like image, the set of 8, synthetic 1024^2 and 4096^2.  GPU and host runs alternate, three of each; the
median is printed.  `python tools/time_graph_render.py [--skip-4096] [--json FILE]`."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superdsm_amd import render, synth                                                  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')


def alternate(gpu_fn, host_fn, runs=3):
    import torch
    gpu_fn()                                                                            # first launch: module load, allocator
    g, h = [], []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter(); gpu_fn(); g.append(time.perf_counter() - t)
        if host_fn is not None:
            t = time.perf_counter(); host_fn(); h.append(time.perf_counter() - t)
    return 1e3 * float(np.median(g)), (1e3 * float(np.median(h)) if h else None)


def bbbc_datas(n):
    from superdsm_amd import automation, config, pipeline
    spec = synth.WORKLOADS['bbbc039_like']
    imgs = []
    for i in range(n):
        shape, layout = synth.bbbc039_like_layout(spec['seed'], i)
        imgs.append(synth.render_image(shape, layout, spec['seed'] + 7919 * i))
    pl = pipeline.create_reference_pipeline()
    cfgs = [c for c, _ in automation.create_configs(pl, config.Config({'AF_scale': 10}), imgs)]
    return [r[0] for r in pl.process_images(imgs, cfgs, last_stage='c2f-region-analysis', out='muted')]


def synthetic(side, seed=0):
    rng = np.random.default_rng(seed)
    n = max(40, side * side // 8000)
    seeds = [(int(rng.integers(0, side)), int(rng.integers(0, side))) for _ in range(n)]
    pts = np.array(seeds)
    lines = []
    for a in range(n):                                                                  # each seed to its three nearest ones
        for b in np.argsort(((pts - pts[a]) ** 2).sum(axis=1))[1:4]:
            if a < b:
                lines.append((seeds[a], seeds[int(b)]))
    cells = np.kron(rng.integers(0, 500, (side // 32, side // 32)), np.ones((32, 32), int)).astype(np.uint16)
    return {'g_raw': rng.random((side, side)), 'y': rng.standard_normal((side, side)), 'seeds': seeds, 'atoms': cells}, lines


def main():
    f = np.load(os.path.join(GOLDEN, 'colormaps.npz'))
    bwr, rainbow = f['bwr'], f['gist_rainbow']
    rows = []

    def row(what, case, gpu_fn, host_fn):
        g, h = alternate(gpu_fn, host_fn)
        rows.append(dict(function=what, case=case, gpu_ms=round(g, 2), host_ms=None if h is None else round(h, 2)))
        print(f'{what:22s} {case:14s} gpu {g:9.2f} ms   host ' + ('        -' if h is None else f'{h:9.2f} ms'), flush=True)

    datas = bbbc_datas(8)
    lines = [d['adjacencies'].get_edge_lines() for d in datas]
    d0 = datas[0]
    row('render_ymap', 'bbbc039 x1', lambda: render.render_ymap(d0, cmap=bwr), lambda: render.render_ymap_host(d0, cmap=bwr))
    row('render_ymap', 'bbbc039 x8', lambda: render.render_ymap_many(datas, cmap=bwr), lambda: [render.render_ymap_host(d, cmap=bwr) for d in datas])
    row('colorize_labels', 'bbbc039 x1', lambda: render.colorize_labels(d0['atoms'], cmap=rainbow, shuffle=1), lambda: render.colorize_labels_host(d0['atoms'], cmap=rainbow, shuffle=1))
    row('colorize_labels', 'bbbc039 x8', lambda: render.colorize_labels_many([d['atoms'] for d in datas], cmap=rainbow, shuffle=1),
        lambda: [render.colorize_labels_host(d['atoms'], cmap=rainbow, shuffle=1) for d in datas])
    row('render_adjacencies', 'bbbc039 x1', lambda: render.render_adjacencies(d0, lines=lines[0]), lambda: render.render_adjacencies_host(d0, lines=lines[0]))
    row('render_adjacencies', 'bbbc039 x8', lambda: render.render_adjacencies_many(datas, lines=lines), lambda: [render.render_adjacencies_host(d, lines=l) for d, l in zip(datas, lines)])
    for side in (1024, 4096):
        if side == 4096 and '--skip-4096' in sys.argv:
            continue
        d, l = synthetic(side)
        case = f'{side}^2'
        row('render_ymap', case, lambda: render.render_ymap(d, cmap=bwr), lambda: render.render_ymap_host(d, cmap=bwr))
        row('colorize_labels', case, lambda: render.colorize_labels(d['atoms'], cmap=rainbow), lambda: render.colorize_labels_host(d['atoms'], cmap=rainbow))
        row('colorize_labels shuffle', case, lambda: render.colorize_labels(d['atoms'], cmap=rainbow, shuffle=1),
            (lambda: render.colorize_labels_host(d['atoms'], cmap=rainbow, shuffle=1)) if side == 1024 else None)
        row(f'render_adjacencies {len(l)}e', case, lambda: render.render_adjacencies(d, lines=l), (lambda: render.render_adjacencies_host(d, lines=l)) if side == 1024 else None)
    if '--json' in sys.argv:
        with open(sys.argv[sys.argv.index('--json') + 1], 'w') as fp:
            json.dump(rows, fp, indent=1)


if __name__ == '__main__':
    main()
