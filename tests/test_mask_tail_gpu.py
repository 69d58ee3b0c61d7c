"""The mask tail of the solve kernel, pixel by pixel, at the parameters the kernel itself returns: the raw mask words, the fragment box,
``on_boundary`` and the two counts of every record against superdsm_amd.testing.tail_reference (the sign of the surface in np.longdouble,
guard band 2^-40 A -- derived there, not fitted).  Needs an MI355X.

Measured on an MI355X (printed by every test, per launch): no pixel and no flag of any scene inside the band, no mismatching pixel; the
smallest |S| / A of a region pixel over all scenes is 2^-22.3 (synthetic256), of a ring pixel 2^-18.3 -- eighteen binary orders above the
band of 2^-40.  The docstrings of the tests give the figures of their scenes."""
import ctypes as C

import numpy as np
import pytest

from superdsm_amd import testing

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    from superdsm_amd import _capi
    _capi.lib()     # fails loudly if libsdsm_hip.so is missing
    return torch


_REFERENCES = {}


def _reference(im, fp, cfg, theta, xi):
    """The reference of one candidate, computed once per (image, footprint, parameters): the launches of a scene return the same bytes."""
    key = (id(im['y']), tuple(fp), repr(sorted((k, v) for k, v in cfg.items() if not callable(v))), theta.tobytes(), None if xi is None else xi.tobytes())
    if key not in _REFERENCES:
        _REFERENCES[key] = (im['y'], testing.tail_reference(im['y'], im.get('y_mask'), im['atoms'], fp, cfg, theta, xi))      # (keeps y alive: its id is the key)
    return _REFERENCES[key][1]


def _check_launch(name, batch, images, image_of, fps, cfg):
    """Every assertion of the issue on the results of the batch's last launch.  Returns (records, list of references); prints the
    figures of the launch before it asserts anything about the pixels."""
    from superdsm_amd import _capi
    recs = batch.records()
    xi_all, xo = batch.xi_dev.cpu().numpy(), batch.xi_offsets()
    raw = batch.masks_dev.cpu().numpy()
    frags = batch.fragments(recs, masks=raw)
    pixels = undecided = undecided_flags = 0
    smallest, smallest_ring = np.inf, np.inf
    errors, refs = [], []
    for k, fp in enumerate(fps):
        im = images[image_of[k]]
        shape = im['y'].shape
        st, M = int(recs['status'][k]), int(recs['n_deform'][k])
        assert st != _capi.CAND_GIVEN_UP, (name, k)
        surface = st in (_capi.CAND_OPTIMAL, _capi.CAND_FALLBACK, _capi.CAND_UNSUPPORTED)
        theta = np.ascontiguousarray(recs['theta'][k], np.float64)
        xi = xi_all[xo[k]:xo[k] + M].copy() if surface and st != _capi.CAND_UNSUPPORTED and M > 0 else None     # (unsupported: the elliptical result)
        ref = _reference(im, fp, cfg, theta if surface else np.zeros(6), xi)
        refs.append(ref)
        # the counts: every status
        got = (int(recs['n_pixels'][k]), int(recs['n_positive'][k]), int(recs['n_negative'][k]))
        if got != (ref['n_pixels'], ref['n_positive'], ref['n_negative']) or got[0] != int(batch.n_pixels[k]):
            errors.append(f'candidate {k} (status {st}): n_pixels, n_positive, n_negative = {got}, reference {(ref["n_pixels"], ref["n_positive"], ref["n_negative"])}')
        if not surface:
            assert st in (_capi.CAND_TRIVIAL, _capi.CAND_ERROR), (name, k, st)
            if frags[k][1].shape != (1, 1) or frags[k][1].any():
                errors.append(f'candidate {k} (status {st}): fragment {frags[k][1].shape}, not [[False]]')
            continue
        # the raw words of the candidate's box
        r0, c0, h, w = (int(v) for v in batch.mask_info[k])
        off, nwords = int(batch.mask_offset[k]), (h * w + 31) // 32
        assert off % 4 == 0 and off + 4 * nwords <= raw.size
        bits = np.unpackbits(raw[off:off + 4 * nwords], bitorder='little')          # bit i of the box: word i >> 5, bit i & 31 (little-endian words)
        if bits[h * w:].any():
            errors.append(f'candidate {k}: {int(bits[h * w:].sum())} bits set past h * w = {h * w} in the last word')
        mine = testing.tail_paste((r0, c0, h, w), bits[:h * w].reshape(h, w).astype(bool), shape)
        region = testing.tail_paste(ref['box'], ref['region'], shape)
        inbox = testing.tail_paste((r0, c0, h, w), np.ones((h, w), bool), shape)
        assert not (region & ~inbox).any(), (name, k, 'the region must lie inside the box of the plan')
        expected = testing.tail_paste(ref['box'], ref['expected'], shape)
        decided = testing.tail_paste(ref['box'], ref['decided'], shape)
        ratio = testing.tail_paste(ref['box'], ref['ratio'], shape, fill=np.inf)
        if (mine & ~region).any():
            errors.append(f'candidate {k}: {int((mine & ~region).sum())} bits set outside the region')
        wrong = decided & (mine != expected)
        if wrong.any():
            rr, cc = np.nonzero(wrong)
            errors.append(f'candidate {k}: {int(wrong.sum())} decided pixels differ; (row, column, log2 |S| / A): '
                          + ', '.join(f'({r}, {c}, {np.log2(ratio[r, c]):.1f})' for r, c in list(zip(rr, cc))[:8]))
        # the box of the kernel's OWN bits, exactly
        box = tuple(int(recs[f][k]) for f in ('fg_r0', 'fg_c0', 'fg_h', 'fg_w'))
        if mine.any():
            fr, fc = np.flatnonzero(mine.any(axis=1)), np.flatnonzero(mine.any(axis=0))
            own = (int(fr[0]), int(fc[0]), int(fr[-1] - fr[0] + 1), int(fc[-1] - fc[0] + 1))
            if box != own:
                errors.append(f'candidate {k}: fg box {box}, bounding box of its own bits {own}')
            elif not (tuple(frags[k][0]) == own[:2] and np.array_equal(frags[k][1], mine[own[0]:own[0] + own[2], own[1]:own[1] + own[3]])):
                errors.append(f'candidate {k}: the unpacked fragment is not the raw bits')
        elif box[2] != 0:
            errors.append(f'candidate {k}: no bit set, fg_h = {box[2]}')
        if (box[2] == 0) != (not mine.any()):
            errors.append(f'candidate {k}: fg_h = {box[2]} with {int(mine.sum())} bits set')
        if ref['on_boundary'] is None:
            undecided_flags += 1
        elif int(recs['on_boundary'][k]) != ref['on_boundary']:
            errors.append(f'candidate {k}: on_boundary {int(recs["on_boundary"][k])}, reference {ref["on_boundary"]} (smallest |S| / A on the ring 2^{np.log2(ref["ring_ratio"]):.1f})')
        pixels += ref['n_pixels']
        undecided += int((region & ~decided).sum())
        smallest, smallest_ring = min(smallest, float(ratio.min())), min(smallest_ring, ref['ring_ratio'])
    lg = lambda v: f'2^{np.log2(v):.1f}' if 0 < v < np.inf else repr(v)
    print(f'{name}: {len(fps)} candidates, {pixels} region pixels, {undecided} undecided pixels, {undecided_flags} undecided flags, '
          f'smallest |S| / A {lg(smallest)} (ring: {lg(smallest_ring)})')
    for e in errors:
        print(f'{name}: {e}')
    assert not errors, (name, errors[:4])
    return recs, refs, dict(pixels=pixels, undecided=undecided, undecided_flags=undecided_flags)


def _run(gpu, name, images, fps, cfg, image_of=None, mode=None, start=None, max_undecided=None):
    """One batch; a launch into fresh mask words and one into words filled with 0xFF (a reused buffer), each checked.  ``start``: called
    with the batch before the first launch (starting points).  The caps: 1 undecided pixel in 10 000, 1 undecided flag."""
    from superdsm_amd import engine
    devs = [engine.DeviceImage(im['y'], im.get('y_mask'), im['atoms'], cfg['background_margin']) for im in images]
    image_of = [0] * len(fps) if image_of is None else list(image_of)
    batch = engine.Batch(devs if len(devs) > 1 else devs[0], fps, cfg, want_xi=True, mode=mode, image_of=image_of if len(devs) > 1 else None)
    if start is not None:
        start(batch)
    out = None
    for fill in (None, 0xFF):
        if fill is not None:
            batch.masks_dev.fill_(fill)
        batch.launch()
        gpu.cuda.synchronize()
        recs, refs, tally = _check_launch(name + (' (reused mask words)' if fill is not None else ''), batch, images, image_of, fps, cfg)
        cap = tally['pixels'] // 10000 if max_undecided is None else max_undecided
        assert tally['undecided'] <= cap and tally['undecided_flags'] <= (1 if max_undecided is None else max_undecided), tally
        if out is not None:
            assert recs.tobytes() == out[0].tobytes()
        out = (recs, refs, batch, devs)
    return out


def _members(batch):
    from superdsm_amd import _capi
    g = np.zeros(batch.n, np.int32)
    _capi.check(_capi.lib().sdsm_plan_schedule(batch.plan, g.ctypes.data_as(C.c_void_p), None), 'sdsm_plan_schedule')
    return g


def _solve_classes(batch, recs, mode):
    """sdsm_solve_class of sdsm_common.h for every candidate: '1', '1b' (256 threads), '2', '2b', '3' (512 threads) or 'group'."""
    states, members = batch.inspect_states(), _members(batch)
    pixmax = 3072 if mode == 1 else np.inf                   # SDSM_WIDE_PIXELS: latency mode
    out = []
    for k, st in enumerate(states):
        M, N = int(recs['n_deform'][k]), int(recs['n_pixels'][k])
        n, env = 6 + M, st['env_size'] if M > 0 else 21
        if st['status'] != 0:
            out.append('none')
        elif members[k] > 0:
            out.append('group')
        elif n <= 128 and env <= 2560 and N <= pixmax:
            out.append('1')
        elif n <= 256 and env <= 7168 and N <= pixmax:
            out.append('1b')
        elif n <= 1024 and env <= 11000:
            out.append('2')
        elif n <= 512 and env <= 15170:
            out.append('2b')
        else:
            out.append('3')
    return out


@pytest.mark.parametrize('mode', [0, 1])
def test_synthetic256_every_pixel_at_the_returned_parameters(gpu, mode):
    """42 candidates, 127 944 region pixels: classes 1 and 1b (and two workgroup groups of 512 threads) in throughput mode, 15 groups in
    latency mode.  Measured: 0 undecided pixels, 0 undecided flags, smallest |S| / A 2^-22.3, on the ring 2^-18.3, in both modes."""
    scene = testing.make_scene('synthetic256')
    im = dict(y=scene['y'], y_mask=None, atoms=scene['atoms'])
    recs, refs, batch, _ = _run(gpu, f'synthetic256 mode {mode}', [im], scene['footprints'], scene['dsm_cfg'], mode=mode)
    assert len(recs) == 42 and (recs['status'] == 0).all()
    classes = _solve_classes(batch, recs, mode)
    print(f'synthetic256 mode {mode}: classes', {c: classes.count(c) for c in sorted(set(classes))})
    if mode == 0:
        assert '1' in classes and '1b' in classes, classes
    else:
        assert 'group' in classes and set(classes) & {'2', '2b', '3', 'group'} and '1' in classes, classes
        assert all(c in ('group', '2', '2b', '3') for c, n in zip(classes, recs['n_pixels']) if n > 3072)


def test_dense_grid_global_memory_class_and_long_rows(gpu):
    """Measured: 5 205 pixels, 0 undecided, smallest |S| / A 2^-20.1 (ring 2^-4.5)."""
    sc = testing.dense_grid_scene()
    recs, refs, batch, _ = _run(gpu, sc['name'], [sc], sc['footprints'], sc['cfg'])
    st = batch.inspect_states()[0]
    assert recs['status'][0] == 0 and st['zmax'] > 28 and 152 < 6 + recs['n_deform'][0] <= 1024 and st['env_size'] > 11000
    assert _solve_classes(batch, recs, 0) == ['3']


@pytest.mark.parametrize('smooth_amount', [4, np.inf])
def test_edge_cases_mask_hole_border_trivial_and_union(gpu, smooth_amount):
    """Measured: 3 932 pixels, 0 undecided; smallest |S| / A 2^-18.0 (ring 2^-14.7) with G~, 2^-22.0 (ring 2^-13.3) without.  The trivial
    candidate's counts are those of its region (records used to carry zeros there)."""
    from superdsm_amd import _capi
    sc = testing.edge_case_scene()
    cfg = dict(sc['cfg'], smooth_amount=smooth_amount)
    recs, refs, batch, _ = _run(gpu, f'{sc["name"]}, smooth_amount {smooth_amount}', [sc], sc['footprints'], cfg)
    assert recs['status'].tolist() == [0, _capi.CAND_TRIVIAL, 0, 0]
    assert recs['n_positive'][1] == 1 and recs['on_boundary'][2] == 1 and refs[2]['on_boundary'] == 1
    assert ((recs['n_deform'] == 0).all() if smooth_amount == np.inf else (recs['n_deform'][[0, 2, 3]] > 0).all())
    hole = ~sc['y_mask']
    assert not testing.tail_paste(refs[0]['box'], refs[0]['region'], hole.shape)[hole].any()


def test_region_beyond_the_setup_tables_counts_on_the_other_path(gpu):
    """Measured: 18 337 pixels, 0 undecided, smallest |S| / A 2^-21.4 (ring 2^-4.8)."""
    from superdsm_amd import _capi
    sc = testing.beyond_setup_tables_scene()
    recs, refs, batch, _ = _run(gpu, sc['name'], [sc], sc['footprints'], sc['cfg'])
    assert recs['status'].tolist() == [_capi.CAND_UNSUPPORTED, _capi.CAND_OPTIMAL] and recs['evals_full'][0] > 0
    assert refs[0]['expected'].any() and recs['fg_h'][0] > 0


def test_rows_that_straddle_mask_words_and_zero_intensities(gpu):
    """Measured: 3 080 pixels, 0 undecided, smallest |S| / A 2^-15.6 (ring 2^-4.1)."""
    sc = testing.straddling_rows_scene()
    recs, refs, batch, _ = _run(gpu, sc['name'], [sc], sc['footprints'], sc['cfg'])
    w = int(batch.mask_info[0, 3])
    assert w == 77 and recs['status'][0] == 0 and recs['n_deform'][0] > 0
    assert recs['n_positive'][0] + recs['n_negative'][0] + 10 == recs['n_pixels'][0]        # five 0.0 and four -0.0 ... and one more 0.0


def test_error_candidate_has_no_fragment_and_exact_counts(gpu):
    """A non-finite intensity: both elliptical solves fail (status ERROR); the candidate beside it is solved as usual."""
    from superdsm_amd import _capi
    y, atoms = testing.two_blob_scene(seed=4)
    y[40, 30] = np.inf
    im = dict(y=y, y_mask=None, atoms=atoms)
    recs, refs, batch, _ = _run(gpu, 'non-finite intensity', [im], [[1], [2]], testing._toy_cfg())
    assert recs['status'].tolist() == [_capi.CAND_ERROR, _capi.CAND_OPTIMAL]


def _given_parameters(batch, cfg, given):
    """Starting points through the callable ``dsm/init``; with ``alpha = inf`` they are what comes back (status FALLBACK)."""
    from superdsm_amd import objects
    start = objects._starting_points(batch, cfg)
    assert len(start) == len(given) == batch.n and all(np.array_equal(s, g) for s, g in zip(start, given))


def _assert_returned_as_given(batch, recs, given):
    from superdsm_amd import _capi
    xi_all, xo = batch.xi_dev.cpu().numpy(), batch.xi_offsets()
    for k, p in enumerate(given):
        M = p.size - 6
        assert recs['status'][k] == _capi.CAND_FALLBACK and recs['n_deform'][k] == M > 0, (k, recs['status'][k], recs['n_deform'][k])
        assert xi_all[xo[k]:xo[k] + M].tobytes() == p[6:].tobytes(), k
        # (the kernel keeps theta in a candidate-local basis: the way there and back mixes the six components)
        assert np.abs(recs['theta'][k] - p[:6]).max() <= 1e-12 * np.abs(p[:6]).max(), (k, recs['theta'][k], p[:6])


@pytest.mark.parametrize('shape', testing.TAIL_CRAFTED_SHAPES)
def test_crafted_surfaces_through_the_tail(gpu, shape):
    """Ring corners, ring lines, a paraboloid over the whole image, an intricate mask: parameters of the test's choice (testing.tail_crafted_cases),
    nothing undecided; the flags and masks are those written out by hand.  Measured: smallest |S| / A 2^-11.7 / 2^-12.5 (ring 2^-7.9)."""
    im = testing.tail_crafted_image(shape)
    H, W = shape
    given, names = [], []

    def init(m):
        cases = testing.tail_crafted_cases(shape, m)
        name = list(cases)[len(given)]
        names.append(name)
        given.append(cases[name]['params'])
        return cases[name]['params']
    cfg = dict(im['cfg'], init=init)
    n = len(testing.tail_crafted_cases(shape, 1))
    recs, refs, batch, _ = _run(gpu, f'crafted {H} x {W}', [im], [im['footprint']] * n, cfg, start=lambda b: _given_parameters(b, cfg, given), max_undecided=0)
    _assert_returned_as_given(batch, recs, given)
    cases = testing.tail_crafted_cases(shape, given[0].size - 6)
    for k, name in enumerate(names):
        case = cases[name]
        assert recs['on_boundary'][k] == case['on_boundary'] == refs[k]['on_boundary'], name
        box = tuple(int(recs[f][k]) for f in ('fg_r0', 'fg_c0', 'fg_h', 'fg_w'))
        if case['mask'] == 'empty':
            assert box == (0, 0, 0, 0) and not refs[k]['expected'].any(), (name, box)
        elif case['mask'] == 'full':
            assert box == (0, 0, H, W) == refs[k]['box'] and refs[k]['expected'].all(), (name, box)
        else:
            assert box == refs[k]['fg_box'] and 0.3 < refs[k]['expected'].mean() < 0.7, (name, box)


def test_every_candidate_of_a_two_image_plan_uses_the_ring_of_its_own_image(gpu):
    """24 x 37 and 37 x 24 in one plan: surfaces positive on the ring of their own image only, and controls positive only where the ring of
    the other image would lie.  Measured: 0 undecided, smallest |S| / A 2^-7.2."""
    ims = [testing.tail_crafted_image(s) for s in testing.TAIL_CRAFTED_SHAPES]
    given, meta = [], []

    def init(m):
        i, name, params, flag = testing.tail_two_image_cases((m, m))[len(given)]
        meta.append((i, name, flag))
        given.append(params)
        return params
    cfg = dict(ims[0]['cfg'], init=init)
    image_of = [c[0] for c in testing.tail_two_image_cases((1, 1))]
    assert image_of == [0, 1, 0, 1, 0, 1]
    recs, refs, batch, _ = _run(gpu, 'two-image plan', ims, [[1]] * len(image_of), cfg, image_of=image_of,
                                start=lambda b: _given_parameters(b, cfg, given), max_undecided=0)
    _assert_returned_as_given(batch, recs, given)
    assert [m[0] for m in meta] == image_of
    for k, (i, name, flag) in enumerate(meta):
        assert recs['on_boundary'][k] == flag == refs[k]['on_boundary'] and recs['fg_h'][k] == 0, name
