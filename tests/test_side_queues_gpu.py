"""The side streams of a launch from caller streams of PyTorch's pool, in a process that has HIP's default of four hardware queues: for every
caller stream the library must find three side streams that run beside it and beside each other, and the launch returns the same bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FOOTPRINTS = [[1], [2], [1, 2]]
CFG = dict(scale=1000, epsilon=1.0, alpha=0.05, smooth_amount=6.0, smooth_subsample=12, gaussian_shape_multiplier=2,
           background_margin=8, init='elliptical')
N_POOL_STREAMS = 6
CHILD_SECONDS = 120


def scene(seed=5, n=96):
    """The scene of tests/test_given_up_gpu.py: one blob, atoms = left and right half; in latency mode each half is a class-1 candidate
    (about 2300 pixels) and their union (about 4600, above 3072) a workgroup group."""
    rng = np.random.default_rng(seed)
    rr, cc = np.mgrid[:n, :n]
    y = -0.1 + 0.02 * rng.standard_normal((n, n))
    y += 0.5 * np.exp(-(((rr - n / 2) / 28.0) ** 2 + ((cc - n / 2) / 28.0) ** 2) ** 3)
    atoms = np.ones((n, n), np.int32)
    atoms[:, n // 2:] = 2
    return y, atoms


def _child(q):
    """Fresh process: four hardware queues, PyTorch's stream pool before the library's; one launch per caller stream."""
    import os
    import traceback
    try:
        os.environ['GPU_MAX_HW_QUEUES'] = '4'
        os.environ['SDSM_SET_HW_QUEUES'] = '0'
        import torch
        streams = [torch.cuda.Stream() for _ in range(N_POOL_STREAMS)]
        from superdsm_amd import _capi, engine
        L = _capi.lib()
        y, atoms = scene()
        batch = engine.Batch(engine.DeviceImage(y, None, atoms, CFG['background_margin']), FOOTPRINTS, CFG, latency_mode=True)
        torch.cuda.synchronize()
        results = []
        for st in [torch.cuda.default_stream()] + streams:
            with torch.cuda.stream(st):
                batch.launch()
            distinct = int(L.sdsm_side_queues_distinct())
            report = np.zeros(8, np.int32)
            _capi.check(L.sdsm_side_queue_report(report.ctypes.data), 'sdsm_side_queue_report')
            st.synchronize()
            with torch.cuda.stream(st):
                recs = batch.records()
                masks = batch.masks_dev.cpu().numpy()
            results.append((distinct, report.tolist(), np.ascontiguousarray(recs).tobytes(), recs['n_pixels'].tolist(), recs['status'].tolist(), masks.tobytes()))
        q.put(('ok', results, os.environ.get('GPU_MAX_HW_QUEUES'), int(_capi.CAND_GIVEN_UP)))
    except BaseException:                                   # noqa: BLE001 -- reported to the parent
        q.put(('error', traceback.format_exc()))


def test_every_caller_stream_gets_three_side_streams_of_its_own():
    import multiprocessing as mp
    import queue
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_child, args=(q,))
    p.start()
    out = ('error', 'the child was not heard')
    try:
        try:
            out = q.get(timeout=CHILD_SECONDS)
        except queue.Empty:
            out = ('error', f'no answer from the child within {CHILD_SECONDS} s')
    finally:
        if out[0] == 'ok':
            p.join(30)
        if p.is_alive():
            p.kill()
            p.join(10)
    assert out[0] == 'ok', out[1]
    _, results, env, given_up = out
    assert env == '4' and len(results) == 1 + N_POOL_STREAMS
    _, _, want_recs, n_pixels, status, want_masks = results[0]
    # the launch has a workgroup group next to class-1 candidates, and the group completed
    assert max(n_pixels) > 3072 and min(n_pixels) <= 3072 and given_up not in status
    for k, (distinct, report, recs, _, _, masks) in enumerate(results):
        print(f'caller stream {k}: distinct {distinct}, report (pool, clean, probes, side 1..4, undecided) {report}')
    for k, (distinct, report, recs, _, _, masks) in enumerate(results):
        assert distinct == 1, (k, distinct, report)
        assert report[1] == 3 and report[0] >= 3, (k, report)
        sides = report[3:6]
        assert len(set(sides)) == 3 and all(0 <= s < report[0] for s in sides) and report[6] == -1, (k, report)
        assert recs == want_recs, k
        assert masks == want_masks, k
