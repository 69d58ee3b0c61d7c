"""The second attempt for candidates whose workgroup group was given up (``engine.Batch.resolve_given_up``) and its callers.  The
groups are made to give up with the diagnostic ``sdsm_set_group_timeout_us`` (a fraction of a microsecond): by design, nothing faults."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FOOTPRINTS = [[1], [2], [1, 2]]
CFG = dict(scale=1000, epsilon=1.0, alpha=0.05, smooth_amount=6.0, smooth_subsample=12, gaussian_shape_multiplier=2,
           background_margin=8, init='elliptical')


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    from superdsm_amd import _capi
    _capi.lib()
    return torch


@contextlib.contextmanager
def tiny_group_timeout():
    from superdsm_amd import _capi
    L = _capi.lib()
    _capi.check(L.sdsm_set_group_timeout_us(0.001), 'sdsm_set_group_timeout_us')
    try:
        yield
    finally:
        _capi.check(L.sdsm_set_group_timeout_us(0.0), 'sdsm_set_group_timeout_us')


def spy_on_resolve(monkeypatch):
    """The index arrays that the calls of ``Batch.resolve_given_up`` return from here on."""
    from superdsm_amd import engine
    resolved, resolve = [], engine.Batch.resolve_given_up
    monkeypatch.setattr(engine.Batch, 'resolve_given_up', lambda self, status=None: resolved.append(resolve(self, status)) or resolved[-1])
    return resolved


def scene(seed=5, n=96):
    """One blob of about 30 pixels radius in an n x n image, atoms = left and right half: with the margin of 8 pixels each half's
    region has about 2300 pixels (a single workgroup in latency mode), their union about 4600 (above 3072: a workgroup group)."""
    rng = np.random.default_rng(seed)
    rr, cc = np.mgrid[:n, :n]
    y = -0.1 + 0.02 * rng.standard_normal((n, n))
    y += 0.5 * np.exp(-(((rr - n / 2) / 28.0) ** 2 + ((cc - n / 2) / 28.0) ** 2) ** 3)
    atoms = np.ones((n, n), np.int32)
    atoms[:, n // 2:] = 2
    return y, atoms


def wavy(m):
    return np.concatenate([np.zeros(6), 0.01 * (-1.0) ** np.arange(m)])


def mask_bytes(batch, masks, i):
    """The bytes of candidate i's bit-packed mask."""
    nb = 4 * ((int(batch.mask_info[i, 2]) * int(batch.mask_info[i, 3]) + 31) // 32)
    o = int(batch.mask_offset[i])
    return masks[o:o + nb].tobytes()


@pytest.mark.parametrize('init', ['elliptical', wavy], ids=['elliptical', 'callable'])
def test_resolve_given_up_replaces_exactly_the_given_up_candidates(gpu, init):
    from superdsm_amd import _capi, engine
    y, atoms = scene()
    cfg = dict(CFG, init=init)
    img = engine.DeviceImage(y, None, atoms, cfg['background_margin'])
    ref = engine.Batch(img, FOOTPRINTS, cfg, mode=2)
    ref.starting_points(init)
    ref.launch()
    want, want_masks = ref.records(), ref.masks_dev.cpu().numpy()
    assert (want['status'] != _capi.CAND_GIVEN_UP).all()
    batch = engine.Batch(img, FOOTPRINTS, cfg, latency_mode=True)
    start = batch.starting_points(init)
    assert (start is None) == (batch.start is None) == (init == 'elliptical')
    with tiny_group_timeout():
        batch.launch()
        first, first_masks = batch.records(), batch.masks_dev.cpu().numpy()
        given_up = first['status'] == _capi.CAND_GIVEN_UP
        assert given_up.any() and not given_up.all()
        assert (given_up == (first['n_pixels'] > 3072)).all()
        again = batch.resolve_given_up()
    assert again.tolist() == np.flatnonzero(given_up).tolist()
    got, got_masks = batch.records(), batch.masks_dev.cpu().numpy()
    for i in range(len(FOOTPRINTS)):
        rec, masks = (want, want_masks) if given_up[i] else (first, first_masks)
        assert got[i].tobytes() == rec[i].tobytes(), i
        assert mask_bytes(batch, got_masks, i) == mask_bytes(batch, masks, i), i
    # the default limit again: the groups complete, and there is nothing to solve again
    batch.launch()
    before = batch.records_dev.clone()
    assert batch.resolve_given_up().size == 0 and batch.resolve_given_up(batch.records()['status']).size == 0
    assert gpu.equal(before, batch.records_dev) and before.cpu().numpy().view(_capi.RECORD_DTYPE)[:3].tobytes() == want.tobytes()


def test_resolve_given_up_refuses_a_batch_with_xi(gpu):
    from superdsm_amd import _capi, engine
    y, atoms = scene()
    batch = engine.Batch(engine.DeviceImage(y, None, atoms, CFG['background_margin']), FOOTPRINTS, CFG, want_xi=True, latency_mode=True)
    batch.launch()
    with pytest.raises(_capi.SdsmError, match='want_xi'):
        batch.resolve_given_up()


def test_normalized_energies_solve_given_up_candidates_again(gpu, monkeypatch):
    """Under the tiny timeout ``normalized_energies`` returns the floats of the default timeout, never a non-finite one, and the
    computer caches those."""
    from superdsm_amd import c2f_energy, engine, image, objects
    y, atoms = scene(seed=6)
    atoms_map = atoms.astype(np.int64)
    atoms_map[44:52, 30:38] = 3                              # inside the blob: all positive -> None
    fps = [{1}, {2}, {1, 2}, {3}, {1, 2, 3}]
    cfg = dict(CFG, cachesize=1, cp_timeout=300)
    yi = image.Image.create_from_array(y, normalize=False)
    cluster = yi.get_region(np.ones(y.shape, bool), shrink=True)
    masked = cluster.get_region(cluster.shrink_mask(np.ones(y.shape, bool)))
    want = c2f_energy.normalized_energies(masked.model, masked.mask, atoms_map, fps, cfg)
    assert want[3] is None and all(v is not None and np.isfinite(v) for k, v in enumerate(want) if k != 3)
    resolved = spy_on_resolve(monkeypatch)
    objs = []
    for fp in fps:
        o = objects.Object()
        o.footprint = frozenset(fp)
        objs.append(o)
    comp = c2f_energy.get_cached_normalized_energy_computer(yi, cluster)
    with tiny_group_timeout():
        got = c2f_energy.normalized_energies(masked.model, masked.mask, atoms_map, fps, cfg)
        cached = comp.compute_many(objs, masked, atoms_map, cfg)
    assert len(resolved) == 2 and all(r.size > 0 for r in resolved)        # the test is about candidates that were given up
    assert got == want and cached == want
    assert len(comp.cache) == len(fps) and all(v is None or np.isfinite(v) for v in comp.cache.values())
    calls = []
    real = engine.Batch
    monkeypatch.setattr(engine, 'Batch', lambda *a, **k: calls.append(1) or real(*a, **k))
    assert comp.compute_many(objs, masked, atoms_map, cfg) == want and calls == []


def test_compute_objects_multi_solves_given_up_candidates_again(gpu, monkeypatch):
    """Two images in one batch under the tiny timeout: energies and fragments of a run with the default timeout."""
    from superdsm_amd import image, objects

    def run():
        jobs = []
        for seed in (5, 7):
            y, atoms = scene(seed)
            objs = [objects.Object() for _ in FOOTPRINTS]
            for o, fp in zip(objs, FOOTPRINTS):
                o.footprint = set(fp)
            jobs.append((objs, image.Image.create_from_array(y, normalize=False), atoms))
        objects.compute_objects_multi(jobs, CFG, out='muted')
        return [o for objs, _, _ in jobs for o in objs]

    want = run()
    resolved = spy_on_resolve(monkeypatch)
    with tiny_group_timeout():
        got = run()
    assert len(got) == 6 and [r.tolist() for r in resolved] == [[2, 5]]      # the union of either image was given up, and only it
    for g, w in zip(got, want):
        assert g.energy == w.energy and np.isfinite(g.energy) and g.is_optimal == w.is_optimal and g.on_boundary == w.on_boundary
        assert tuple(g.fg_offset) == tuple(w.fg_offset) and np.array_equal(g.fg_fragment, w.fg_fragment)
