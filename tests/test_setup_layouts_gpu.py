"""The setup kernel's two layouts of the region state (LDS block / global arrays, csrc/sdsm_setup.hip RegionArrays) and its
raster-order pixel arrays, on hand-made regions at the shapes where they can go wrong: grid, runs and G~ are read back as
test_gpu_parity.test_setup_matches_reference_smooth_matrix does and must equal oracle.region_mask / oracle.smooth_matrix exactly
(float32 weights bit for bit).  Needs an MI355X."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_OK, ST_TRIVIAL = 0, 2


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    from superdsm_amd import _capi
    _capi.lib()
    return torch


def _state_budget():
    """SetupLimS::STATE of csrc/sdsm_launch.h: bytes of the LDS block of the region state; a region takes 6 bytes per pixel and 6 per
    run of the plan's bound on its runs (sdsm_setup.hip, setup_state_bytes)."""
    text = open(os.path.join(ROOT, 'superdsm_amd', 'csrc', 'sdsm_launch.h')).read()
    m = re.search(r'struct SetupLimS \{[^}]*\bSTATE = (\d+)', text)
    assert m, 'SetupLimS::STATE not found'
    return int(m.group(1))


def _cfg(sigma=2.0, sub=4, margin=0, **kw):
    from superdsm_amd import testing
    return testing._toy_cfg(smooth_amount=float(sigma), smooth_subsample=int(sub), gaussian_shape_multiplier=2.0, background_margin=margin,
                            alpha=0.01, max_iters=1, **kw)


def _scene(masks, col0=4, gap=6, y_of=None):
    """The masks one below the other (``gap`` rows apart, first column ``col0`` -- one value or one per mask): atoms 1 .. n are the
    masks, n + 1 everything else; y = +1 on the masks (``y_of``: per mask an array of its own), -1 elsewhere."""
    col0 = [col0] * len(masks) if np.isscalar(col0) else list(col0)
    H = gap + sum(m.shape[0] + gap for m in masks)
    W = max(c + m.shape[1] for c, m in zip(col0, masks)) + 5
    atoms = np.full((H, W), len(masks) + 1, np.int32)
    y = np.full((H, W), -1.0)
    placed, r = [], gap
    for k, (m, c) in enumerate(zip(masks, col0)):
        box = (slice(r, r + m.shape[0]), slice(c, c + m.shape[1]))
        atoms[box][m] = k + 1
        y[box][m] = 1.0 if y_of is None or y_of[k] is None else y_of[k][m]
        full = np.zeros((H, W), bool)
        full[box] = m
        placed.append(full)
        r += m.shape[0] + gap
    return y, atoms, placed


def _cand_block(batch):
    from superdsm_amd import _capi
    lay = batch.layout()
    return batch.ws[lay['cand']:lay['cand'] + lay['cand_size'] * batch.n].cpu().numpy().view(_capi.CAND_DESC_DTYPE)


def _check_candidate(s, y, atoms, fp, cfg, placed=None):
    """One entry of Batch.inspect() against the oracle: region pixels in raster order, grid, and every row of G~."""
    from oracle import oracle
    mask = oracle.region_mask(y, None, atoms, fp, cfg['background_margin'])
    if placed is not None:
        np.testing.assert_array_equal(mask, placed)
    rr, cc = np.nonzero(mask)
    assert s['status'] == ST_OK and s['N'] == mask.sum()
    np.testing.assert_array_equal(s['r'], rr)
    np.testing.assert_array_equal(s['c'], cc)
    np.testing.assert_array_equal(s['y'], y[mask])
    sm = oracle.smooth_matrix(mask, cfg['smooth_amount'], cfg['gaussian_shape_multiplier'], cfg['smooth_subsample'])
    assert s['M'] == sm.M
    assert (s['hc'], s['wc']) == sm.compressed_shape
    np.testing.assert_array_equal(s['grid_r'], sm.grid_r)
    np.testing.assert_array_equal(s['grid_c'], sm.grid_c)
    nnz = np.diff(sm.indptr)
    np.testing.assert_array_equal(s['nnz'], nnz)
    sel = np.arange(s['idx'].shape[0])[None, :] < nnz[:, None]          # [pixel, slot]
    np.testing.assert_array_equal(s['idx'].T[sel], sm.indices)
    np.testing.assert_array_equal(s['w'].T[sel].astype(np.float64), sm.data)     # float32-exact
    return sm


def _run(gpu, masks, cfg, col0=4, y_of=None):
    from superdsm_amd import engine
    y, atoms, placed = _scene(masks, col0=col0, y_of=y_of)
    img = engine.DeviceImage(y, None, atoms, cfg['background_margin'])
    batch = engine.Batch(img, [[k + 1] for k in range(len(masks))], cfg)
    batch.launch()
    gpu.cuda.synchronize()
    return batch, batch.inspect(), y, atoms, placed


def _rows(widths, width):
    """A mask with one row per entry of ``widths``: that many pixels from column 0."""
    m = np.zeros((len(widths), width), bool)
    for r, w in enumerate(widths):
        m[r, :w] = True
    return m


def test_region_at_the_lds_budget_and_one_pixel_above(gpu):
    """83 full rows of 36 pixels (9 cells) and a last row of 10 / 11 pixels: pixels + bound on the runs = STATE / 6 exactly, and one
    more.  The first region again two columns to the right: its bounding box then spans 10 cells per row, the bound on its runs
    passes the budget, so the same pixels go through the global layout -- and must give the same rows, pixel by pixel."""
    budget = _state_budget() // 6
    cells, w = 9, 36
    h = (budget + w) // (w + cells)                                      # (h - 1) w + k + h cells = budget, 1 <= k <= w
    k = budget - ((h - 1) * w + h * cells)
    assert 1 <= k < w, 'choose another width for this budget'
    at, above = _rows([w] * (h - 1) + [k], w), _rows([w] * (h - 1) + [k + 1], w)
    cfg = _cfg(sigma=4.0, sub=8)
    batch, info, y, atoms, placed = _run(gpu, [at, above, at], cfg, col0=[4, 4, 6])
    cand = _cand_block(batch)
    assert [int(c['N']) + int(c['NRcap']) for c in cand] == [budget, budget + 1, budget + h]
    assert all(int(c['rows_g']) == 0 for c in cand)
    sms = [_check_candidate(info[i], y, atoms, [i + 1], cfg, placed[i]) for i in range(3)]
    assert sms[0].M > 16                                                  # the lattice search, not the all-points loop
    for f in ('grid_r', 'grid_c', 'nnz', 'idx', 'w', 'lead', 'hnz'):
        np.testing.assert_array_equal(info[0][f], info[2][f])


@pytest.mark.parametrize('nr', [1, 63, 64, 65, 257])
def test_number_of_runs(gpu, nr):
    """Regions of exactly ``nr`` runs, 16 columns = 4 cells wide: a chunk of 64 positions that is not full, exactly full, one run into
    the next chunk; 257 runs: a second trip of the 256-thread loops over the runs.  One run alone is a region without G~."""
    full, rest = divmod(nr, 4)
    mask = _rows([16] * full + ([4 * rest] if rest else []), 16)
    cfg = _cfg(sigma=2.0, sub=4)
    batch, info, y, atoms, placed = _run(gpu, [mask], cfg)
    assert info[0]['NR'] == nr
    sm = _check_candidate(info[0], y, atoms, [1], cfg, placed[0])
    assert (sm.M > 0) == (nr > 1)


def test_single_pixel_runs_and_every_cell_pattern(gpu):
    """Every pattern of present pixels of a 4-column cell (0b1001 and the single pixels among them), each in every column of cells."""
    mask = np.zeros((30, 60), bool)
    for r in range(30):
        for j in range(15):
            p = (j + r) % 15 + 1
            mask[r, 4 * j:4 * j + 4] = [(p >> b) & 1 for b in range(4)]
    cfg = _cfg(sigma=2.0, sub=4)
    batch, info, y, atoms, placed = _run(gpu, [mask], cfg)
    assert info[0]['NR'] == 30 * 15 and set(np.bincount(info[0]['run_pixels'], minlength=5)[1:] > 0) == {True}
    sm = _check_candidate(info[0], y, atoms, [1], cfg, placed[0])
    assert sm.M > 0


def test_thin_arm_far_from_the_lattice(gpu):
    """A 48 x 48 block (144 lattice points) with an arm of one pixel row on a row between the lattice rows: no lattice position along
    the arm holds a pixel, so its far pixels find no grid point within three rings and look at all of them; the greedy steps then
    add points along the arm."""
    mask = np.zeros((48, 48 + 70), bool)
    mask[:, :48] = True
    mask[21, 48:] = True
    cfg = _cfg(sigma=2.0, sub=4)
    batch, info, y, atoms, placed = _run(gpu, [mask], cfg)
    sm = _check_candidate(info[0], y, atoms, [1], cfg, placed[0])
    assert sm.M > 144 and (sm.grid_r[sm.grid_c >= 48] == 21).all() and (sm.grid_c >= 48 + 20).any()


def test_null_matrix_region(gpu):
    """Two rows of pixels against a PSF of 9 x 9: hc <= k / 2, no G~ (dsm.py:187); its runs keep their scan order."""
    mask = np.ones((2, 30), bool)
    cfg = _cfg(sigma=2.0, sub=4)
    batch, info, y, atoms, placed = _run(gpu, [mask], cfg)
    sm = _check_candidate(info[0], y, atoms, [1], cfg, placed[0])
    assert sm.M == 0 and info[0]['NR'] == 16 and (info[0]['nnz'] == 0).all()


def test_one_positive_pixel_is_trivial(gpu):
    """A single positive pixel with its margin of negative ones: the trivial rule (objects.py:184-191), beside an ordinary region."""
    from oracle import oracle
    blob = np.ones((20, 24), bool)
    dot = np.ones((5, 5), bool)
    ydot = np.full((5, 5), -0.5)
    ydot[2, 2] = 1.0
    cfg = _cfg(sigma=2.0, sub=4, margin=2)
    batch, info, y, atoms, placed = _run(gpu, [blob, dot], cfg, y_of=[None, ydot])
    _check_candidate(info[0], y, atoms, [1], cfg)
    states = batch.inspect_states()
    mask = oracle.region_mask(y, None, atoms, [2], cfg['background_margin'])
    assert states[1]['status'] == ST_TRIVIAL and info[1]['npos'] == 1 and int(_cand_block(batch)[1]['N']) == mask.sum()


def test_two_images_in_one_plan(gpu):
    from superdsm_amd import engine
    cfg = _cfg(sigma=2.0, sub=4)
    a = _rows([20] * 14 + [7], 20)
    b = np.zeros((25, 33), bool)
    b[np.add.outer(np.arange(25), np.arange(33)) % 3 != 0] = True
    scenes = [_scene([m], col0=c) for m, c in ((a, 4), (b, 7))]
    imgs = [engine.DeviceImage(y, None, atoms, 0) for y, atoms, _ in scenes]
    batch = engine.Batch(imgs, [[1], [1]], cfg, image_of=np.array([0, 1], np.int32))
    batch.launch()
    gpu.cuda.synchronize()
    info = batch.inspect()
    for i, (y, atoms, placed) in enumerate(scenes):
        _check_candidate(info[i], y, atoms, [1], cfg, placed[0])


def test_second_launch_leaves_the_same_outputs(gpu):
    """One plan launched twice: the outputs of the setup phase are the same bytes after the second launch (nothing of a launch
    survives in the state that only lives in LDS), for regions of both layouts in one plan."""
    budget = _state_budget() // 6
    small = _rows([36] * 30 + [5], 36)
    large = np.ones((budget // 40 + 2, 40), bool)                          # pixels alone pass the budget: the global layout
    cfg = _cfg(sigma=4.0, sub=8)
    batch, info, y, atoms, placed = _run(gpu, [small, large], cfg)
    assert small.sum() * 2 <= budget < large.sum()
    lay = batch.layout()
    nruns, nell = lay['total_runs'], lay['total_ell']
    sizes = dict(state=lay['state_size'] * batch.n, crop_y=32 * nruns, crop_rc=4 * nruns, run_meta=4 * nruns, ell_im=4 * nell, ell_w=16 * nell)
    snap = lambda: {k: batch.ws[lay[k]:lay[k] + v].cpu().numpy().copy() for k, v in sizes.items()}
    first = snap()
    batch.launch()
    gpu.cuda.synchronize()
    second, info2 = snap(), batch.inspect()
    for k in sizes:
        np.testing.assert_array_equal(first[k], second[k], err_msg=k)
    for i in range(2):
        _check_candidate(info2[i], y, atoms, [i + 1], cfg, placed[i])
        np.testing.assert_array_equal(info[i]['grid_r'], info2[i]['grid_r'])
        np.testing.assert_array_equal(info[i]['grid_c'], info2[i]['grid_c'])
