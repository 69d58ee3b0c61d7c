"""Per-image wall clock of a ``process_image`` loop against ``Pipeline.process_images`` on the 8 BBBC039-like images, stage by stage,
with the reference pipeline (``AF_scale`` = 10).  Also the C2F phases of the set, and the markers + EDT of the set (one call) against
8 single-image calls.  Both runs must give the same atoms and the same postprocessed objects; the script checks that.

    python tools/time_image_sets.py [--repeat N]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from superdsm_amd import automation, c2freganal as cr, config, pipeline, synth  # noqa: E402


def images():
    spec = synth.WORKLOADS['bbbc039_like']
    out = []
    for i in range(8):
        shape, layout = synth.bbbc039_like_layout(spec['seed'], i)
        out.append(synth.render_image(shape, layout, spec['seed'] + 7919 * i))
    return out


def loop(pl, imgs, cfgs):
    t0 = time.perf_counter()
    res = [pl.process_image(g, c, out='muted') for g, c in zip(imgs, cfgs)]
    return res, time.perf_counter() - t0


def batched(pl, imgs, cfgs):
    t0 = time.perf_counter()
    res = pl.process_images(imgs, cfgs, out='muted')
    return res, time.perf_counter() - t0


def stage_ms(res):
    names = list(res[0][2])
    return {n: 1e3 * np.mean([t[n] for _, _, t in res]) for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    a = ap.parse_args()
    import torch
    imgs = images()
    pl = pipeline.create_reference_pipeline()
    cfgs = [c for c, _ in automation.create_configs(pl, config.Config({'AF_scale': 10}), imgs)]
    loop(pl, imgs[:2], cfgs[:2])                          # warm-up: library load, first launches of every kernel
    batched(pl, imgs[:2], cfgs[:2])
    for r in range(a.repeat):                             # the two alternate, so that drift of the host hits both
        res_l, t_l = loop(pl, imgs, cfgs)
        res_b, t_b = batched(pl, imgs, cfgs)
        for (dl, _, _), (db, _, _) in zip(res_l, res_b):
            assert np.array_equal(dl['atoms'], db['atoms'])
            pl_, pb_ = dl['postprocessed_objects'], db['postprocessed_objects']
            assert len(pl_) == len(pb_) and all(np.array_equal(x.fg_fragment, y.fg_fragment) for x, y in zip(pl_, pb_))
        sl, sb = stage_ms(res_l), stage_ms(res_b)
        print(f'run {r}: per image, process_image loop {1e3 * t_l / len(imgs):.1f} ms, process_images {1e3 * t_b / len(imgs):.1f} ms '
              f'(outputs equal)', flush=True)
        for n in sl:
            print(f'    {n:28s} loop {sl[n]:8.2f} ms   set {sb[n]:8.2f} ms', flush=True)
    c2f = pl.stages[[s.name for s in pl.stages].index('c2f-region-analysis')]
    st = c2f.last_set_stats
    n = st['images']
    print(f'C2F phases of the set, per image: markers+EDT {1e3 * st["markers_edt_s"] / n:.2f} ms, flood {1e3 * st["flood_s"] / n:.2f} ms, '
          f'host split logic {1e3 * st["host_split_s"] / n:.2f} ms, assembly {1e3 * st["assemble_s"] / n:.2f} ms, '
          f'{st["n_rounds"]} energy rounds {1e3 * st["energy_s"] / n:.2f} ms ({st["launches"]} plan launches), '
          f'total {1e3 * st["total_s"] / n:.2f} ms', flush=True)
    ys = [d['y'] for d, _, _ in res_b]
    for r in range(a.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for y in ys:
            _, markers, d_markers, _ = cr.cluster_markers_gpu(y, 0.2)
            cr.edt_exact_gpu(d_markers)
        t1 = time.perf_counter()
        cr.markers_and_edt_gpu_multi(ys, 0.2)
        t2 = time.perf_counter()
        print(f'markers + EDT of the 8 images: 8 single-image calls {1e3 * (t1 - t0):.2f} ms, one set call {1e3 * (t2 - t1):.2f} ms', flush=True)


if __name__ == '__main__':
    main()
