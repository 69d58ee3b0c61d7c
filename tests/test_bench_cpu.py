"""bench.py --dump-outputs without a GPU: what the dump writes from a step's records and fragments."""
import os

import numpy as np

import bench
from superdsm_amd import _capi


def _step(n, box_hw, seed=0):
    rng = np.random.default_rng(seed)
    recs = np.zeros(n, _capi.RECORD_DTYPE)
    recs['energy'] = rng.random(n)
    recs['theta'] = rng.random((n, 6))
    recs['fg_h'] = rng.integers(1, min(box_hw[0], 16) + 1, n)          # (a fragment lies inside its box)
    recs['fg_w'] = rng.integers(1, min(box_hw[1], 16) + 1, n)
    boxes = np.zeros((n, 4), np.int32)
    boxes[:, 2:] = box_hw
    frags = [((i, 2 * i), rng.random((h, w)) < 0.5) for i, (h, w) in enumerate(zip(recs['fg_h'], recs['fg_w']))]
    return recs, boxes, frags


def _dump(tmp_path, name, recs, boxes, frags):
    d = tmp_path / name
    asked = []

    def fragments(sel):
        asked.append(sel.copy())
        return [f if s else (None, None) for f, s in zip(frags, sel)]
    bench.dump_outputs(str(d), recs, boxes, fragments)
    return d, {f[:-4]: np.load(d / f) for f in os.listdir(d)}, asked


def test_dump_outputs_writes_records_and_a_fixed_mask_sample_within_the_budget(tmp_path):
    box = (1024, 1024)                                    # 4 MB of float32 per box: the budget holds 12 of the 40 candidates
    recs, boxes, frags = _step(40, box)
    d, out, asked = _dump(tmp_path, 'a', recs, boxes, frags)
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
    for name in recs.dtype.names:
        if name != 'reserved':
            np.testing.assert_array_equal(out[f'records_{name}'], recs[name].astype(np.float64))
    take = out['masks_candidates'].astype(int)
    assert len(take) == (bench.DUMP_MASK_BYTES // (4 * box[0] * box[1])) and np.all(np.diff(take) > 0)
    assert np.array_equal(np.flatnonzero(asked[0]), take)
    np.testing.assert_array_equal(out['masks_origin'], [frags[i][0] for i in take])
    np.testing.assert_array_equal(out['masks_shape'], [frags[i][1].shape for i in take])
    np.testing.assert_array_equal(out['masks'], np.concatenate([frags[i][1].ravel() for i in take]).astype(np.float32))
    # the sample depends on the plan's boxes alone: other results, same candidates
    recs2, _, frags2 = _step(40, box, seed=1)
    _, out2, _ = _dump(tmp_path, 'b', recs2, boxes, frags2)
    np.testing.assert_array_equal(out2['masks_candidates'], out['masks_candidates'])


def test_dump_outputs_takes_every_mask_of_a_small_step(tmp_path):
    recs, boxes, frags = _step(30, (20, 30))
    _, out, _ = _dump(tmp_path, 'a', recs, boxes, frags)
    np.testing.assert_array_equal(out['masks_candidates'], np.arange(30))
    assert out['masks'].size == sum(f[1].size for f in frags)
