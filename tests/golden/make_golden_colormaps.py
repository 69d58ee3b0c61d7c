"""Writes tests/golden/colormaps.npz: the lookup tables of the matplotlib colour maps that the y-map and label pictures use, as the
colour-map kernel takes them -- ``(N + 3) x 4`` float64: the ``N`` colours, then the colours for values below, above and "bad".
Needs matplotlib only (the tables were taken from matplotlib 3.10.8); tests/test_graph_render_cpu.py checks the committed file
against what this produces."""
import os

import numpy as np

NAMES = ('bwr', 'seismic', 'gist_rainbow')


def tables():
    import matplotlib
    out = {}
    for name in NAMES:
        cmap = matplotlib.colormaps[name]
        if not cmap._isinit:
            cmap._init()
        assert (cmap._i_under, cmap._i_over, cmap._i_bad) == (cmap.N, cmap.N + 1, cmap.N + 2)
        out[name] = np.ascontiguousarray(cmap._lut, np.float64)
        assert out[name].shape == (cmap.N + 3, 4)
    return out


if __name__ == '__main__':
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'colormaps.npz'), **tables())
