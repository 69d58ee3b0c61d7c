"""Generates tests/golden/overlays.npz: the reference's overlays (superdsm/render.py:137-365) on a small scene of disjoint objects.

Runs only where the reference is checked out (see _refshim.py); the fixture it writes is data.  The shim's watershed stand-in refuses
to flood, so the objects of the scene are disjoint.  ``rasterize_regions`` calls the grey-level ``skimage.morphology.erosion``, which
the shim does not provide: on a bool image it is a binary erosion with a border that does not erode, installed here.

    python tests/golden/make_golden_overlays.py
"""
import os
import sys

import numpy as np
import scipy.ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _refshim  # noqa: E402

_refshim.install()
sys.modules['skimage.morphology'].erosion = lambda img, se: scipy.ndimage.binary_erosion(np.asarray(img, bool), structure=np.asarray(se, bool), border_value=True)

import superdsm.objects as robjects  # noqa: E402
import superdsm.render as rrender  # noqa: E402


class _Obj(robjects.BaseObject):
    def __init__(self, offset, fragment):
        self.fg_offset = np.asarray(offset)
        self.fg_fragment = np.asarray(fragment, bool)


def main():
    rng = np.random.default_rng(17)
    shape = (72, 88)

    def blob(h, w):
        rr, cc = np.mgrid[:h, :w]
        return ((rr - (h - 1) / 2) / (h / 2)) ** 2 + ((cc - (w - 1) / 2) / (w / 2)) ** 2 <= 1

    # disjoint objects, two of them touching (no gap between their masks), two at the image border
    objs = [((0, 4), blob(13, 17)), ((20, 30), blob(18, 12)), ((20, 42), blob(18, 9)), ((50, 0), blob(15, 15)), ((58, 70), blob(14, 18)),
            ((5, 60), rng.random((11, 13)) > 0.25), ((44, 40), np.ones((3, 2), bool))]
    g_raw = rng.normal(0.2, 0.05, shape)
    for off, fr in objs:
        g_raw[off[0]:off[0] + fr.shape[0], off[1]:off[1] + fr.shape[1]][fr] += 0.5
    g_raw[3, 80] = 4.0                                                   # an outlier: normalize_image clips it
    atoms = np.kron(rng.permutation(20).reshape(4, 5) % 7, np.ones((18, 18), int))[:shape[0], :shape[1]]
    clusters = np.where(atoms > 3, atoms - 3, 0)
    data = {'g_raw': g_raw, 'atoms': atoms, 'clusters': clusters}
    robjs = [_Obj(o, f) for o, f in objs]
    override = rng.random(shape) * 1.3 - 0.1
    g_rgb = rng.integers(0, 256, shape + (3,)).astype(np.float64)

    out = dict(g_raw=g_raw, atoms=atoms.astype(np.int32), clusters=clusters.astype(np.int32), override=override, g_rgb=g_rgb, n=np.asarray(len(objs)))
    for k, (off, fr) in enumerate(objs):
        out[f'o{k}_offset'] = np.asarray(off)
        out[f'o{k}_fragment'] = np.asarray(fr, np.uint8)
    out['normalized'], out['normalized_min'], out['normalized_max'] = rrender.normalize_image(g_raw, ret_minmax=True)
    out['normalized_half'] = rrender.normalize_image(g_raw, spread=0.5)
    out['result_center'] = rrender.render_result_over_image(data, robjs)
    out['result_inner'] = rrender.render_result_over_image(data, robjs, border_width=4, border_position='inner', color='y')
    out['result_override'] = rrender.render_result_over_image(data, robjs, border_width=2, override_img=override)
    out['result_rgb'] = rrender.render_result_over_image(dict(data, g_rgb=g_rgb), robjs, color='r')
    out['atoms_overlay'] = rrender.render_atoms(data)
    out['clusters_overlay'] = rrender.render_foreground_clusters(data, border_radius=3)
    out['atoms_override'] = rrender.render_atoms(data, normalize_img=False, override_img=override)
    path = os.path.join(HERE, 'overlays.npz')
    np.savez_compressed(path, **out)
    print(f'overlays.npz: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
