"""A second full evaluation at an unchanged iterate (stop test repeated with the true curvature, larger diagonal shift after a failed
pivot) takes the pixel sums the first one kept instead of a second pass over the pixels, and leaves every result bit for bit as it
is.  It can be switched off per process (sdsm_set_solver_diagnostics) and counts its events
(sdsm_batch_solver_counters).
Scene: synthetic256 (the smoke test's: 42 candidates, N <= 10 454, M ~ 10 .. 162 -- class 1, class 1b and the 512-thread classes, in
latency mode a workgroup group); the oracle makes 41 such second evaluations on it."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RECOMPUTE = 1
ERR_ARGUMENT = -1                                    # SDSM_ERR_ARGUMENT (include/sdsm.h)


@functools.lru_cache(maxsize=None)
def _scene():
    from superdsm_amd import testing
    return testing.make_scene('synthetic256')


@functools.lru_cache(maxsize=None)
def _solve(mode, flags):
    """(records, xi, packed masks) as bytes and the event counters of one launch of the scene under the given diagnostics."""
    import torch
    from superdsm_amd import _capi, engine
    scene = _scene()
    L = _capi.lib()
    _capi.check(L.sdsm_set_solver_diagnostics(flags), 'sdsm_set_solver_diagnostics')
    try:
        img = engine.DeviceImage(scene['y'], None, scene['atoms'], scene['dsm_cfg']['background_margin'])
        batch = engine.Batch(img, scene['footprints'], scene['dsm_cfg'], want_xi=True, mode=mode)
        batch.launch()
        torch.cuda.synchronize()
        recs = batch.records()
        out = (recs.tobytes(), batch.xi_dev.cpu().numpy().tobytes(), batch.masks_dev.cpu().numpy().tobytes())
        with_m = recs['n_deform'] > 0
        return out, batch.solver_counters(), int(recs['evals_full'][with_m].sum()), int(with_m.sum())
    finally:
        _capi.check(L.sdsm_set_solver_diagnostics(0), 'sdsm_set_solver_diagnostics')


def test_reused_sums_equal_a_second_pass():
    reused = []
    for mode in (0, 1, 2):
        out, cnt, evals, ncand = _solve(mode, 0)
        out_r, cnt_r, evals_r, _ = _solve(mode, RECOMPUTE)
        print(f'mode {mode}: {cnt["evals_reused"]} of {evals} full evaluations of {ncand} candidates with M > 0 served from kept sums '
              f'({100.0 * cnt["evals_reused"] / evals:.2f} %); with recomputation {cnt_r["evals_reused"]}')
        for a, b, what in zip(out, out_r, ('records', 'xi', 'masks')):
            assert a == b, f'mode {mode}: {what} differ between kept sums and a second pass'
        assert evals == evals_r                      # evals_full counts evaluations, served or computed
        assert cnt_r['evals_reused'] == 0, (mode, cnt_r)
        reused.append(cnt['evals_reused'])
        # a third of the 42 candidates: the oracle makes 41 such evaluations here; the slack is for envelopes that do not fit twice
        # and for second evaluations at another fixed-point scale
        assert cnt['evals_reused'] >= 14, (mode, cnt)


def test_entry_points():
    import torch
    from superdsm_amd import _capi, engine
    L = _capi.lib()
    try:
        for bad in (2, 4, 1 << 30, -1):
            assert L.sdsm_set_solver_diagnostics(bad) == ERR_ARGUMENT, bad
        for good in (1, 0):
            assert L.sdsm_set_solver_diagnostics(good) == _capi.SDSM_OK, good
    finally:
        L.sdsm_set_solver_diagnostics(0)
    scene = _scene()
    img = engine.DeviceImage(scene['y'], None, scene['atoms'], scene['dsm_cfg']['background_margin'])
    batch = engine.Batch(img, scene['footprints'][:4], scene['dsm_cfg'])
    torch.cuda.synchronize()
    assert batch.solver_counters() == dict(evals_reused=0)      # before any launch
    out = np.zeros(4, np.int64)
    assert L.sdsm_batch_solver_counters(None, None, out.ctypes.data_as(C.c_void_p)) == ERR_ARGUMENT
