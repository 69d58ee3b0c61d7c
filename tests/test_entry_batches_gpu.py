"""The entry loops of the passes over the pixels (smooth_add, smooth_add2, the gradient loops of eval_full): whole
batches of EBATCH = 4 entries run as straight-line code, one guarded tail of 1 to 3 entries follows, the first HZREG = 8 entries of a run
are loaded straight into the registers of its leading entries, and an entry is masked only where the lane has that many leading entries.
None of this may change a bit of any result: everything here is compared byte for byte with tests/golden/entry_batches.npz, recorded on
an MI355X from the commit BEFORE the loops were rewritten (gpu_fixture() below is the recorder: np.savez_compressed of what it returns).

Scenes: the 80 x 96 blob of tests/test_loss_arithmetic_gpu.py (one atom, one candidate) under settings chosen for the entry counts kh the
chunks of 64 runs are padded to (a chunk's rows are padded to the count of its first run; the runs are sorted by their counts) and for the
leading entries hz of the runs -- read back from the run words of the workspace and asserted below:
  kh mod 4 = 0, 1, 2, 3 and kh = 1, 3, 4, 8, 9 (one short tail alone; one whole batch alone; two batches: the leading registers full; two and a tail),
  runs with hz = 1 and hz = 8 = HZREG leading entries in candidates that keep them in registers, and candidates with more than HZREG leading
  entries in a run, in class 1 and in class 1b (they are read from memory).
No run of a candidate that is solved has hz = 0: every pixel's largest weight is a leading entry, and a pixel without an entry makes its
candidate an error (SDSM_CAND_ERROR: malformed rows, no solve) -- the exploration of 88 settings of this blob found hz = 0 in those alone.
The lanes beyond a slice's last run are the ones that pass through with hz = 0; every scene here has such lanes (NR is no multiple of 64).
Every scene is solved (its own class: class 1, class 1b, and class 3 for the one with hz = 8), evaluated at two fixed points by sdsm_k_eval,
and taken through one Newton step (sdsm_k_step_probe: full evaluation, factorisation, line sweep along a given direction) in the layouts of
class 1, class 1b and the light group class -- the last one is a group of one member -- wherever the layout holds it."""
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'entry_batches.npz')
EBATCH, HZREG = 4, 8
LIMITS = {'class 1': (128, 2560), 'class 1b': (256, 7168), 'light': (288, 12400)}     # 6 + M and envelope doubles a layout holds (sdsm_common.h)
SCENES = {
    # name: background margin, dsm/* settings on top of testing._toy_cfg, (M, envelope, hzmax) and the class it is solved in
    'kh 1-6': (4, dict(smooth_subsample=5, smooth_amount=1), (92, 1283, 3), 'class 1'),
    'kh 8-25': (8, dict(smooth_subsample=8, smooth_amount=4), (47, 1055, 6), 'class 1'),
    'hz 12': (4, dict(smooth_subsample=6, smooth_amount=4), (62, 1890, 12), 'class 1'),
    '1b, kh 1-6': (8, dict(smooth_subsample=5, smooth_amount=1), (123, 1917, 3), 'class 1b'),
    '1b, hz 13': (8, dict(smooth_subsample=5, smooth_amount=4), (123, 5093, 13), 'class 1b'),
    'hz 8': (8, dict(smooth_subsample=3, smooth_amount=1.5), (342, 16302, 8), 'class 3'),
}
NEEDED_KH = (1, 3, 4, 8, 9)
ENV_WHOLE = 4096                                # longer envelopes are kept as their SHA-256


def _layouts(M, env, cls):
    return ['class 3'] if cls == 'class 3' else [lay for lay, (nmax, emax) in LIMITS.items() if 6 + M <= nmax and env <= emax]


def _run_words(batch):
    """Entries and leading entries of the runs of candidate 0 in stored order (run_meta), and the entry count every chunk is padded to."""
    from superdsm_amd import _capi
    lay = batch.layout()
    ws = batch.ws.cpu().numpy()
    blk = lambda name, dt, cnt: ws[lay[name]:lay[name] + np.dtype(dt).itemsize * cnt].view(dt)
    cand, state = blk('cand', _capi.CAND_DESC_DTYPE, batch.n), blk('state', _capi.CAND_STATE_DTYPE, batch.n)
    NR, ro = int(state[0]['NR']), int(cand[0]['run_off'])
    meta = blk('run_meta', np.uint32, lay['total_runs'])[ro:ro + NR]
    assert lay['zcap_run'] <= 256                            # sort classes of ONE entry count: a chunk is padded to the count of its first run
    nnz, hz = (meta & 0xfff).astype(np.int64), ((meta >> 12) & 0xfff).astype(np.int64)
    return nnz, hz, nnz[::64].copy()


def _points(M):
    rng = np.random.default_rng(5)
    a = np.zeros(6 + M)
    a[5] = 1.0
    b = np.concatenate([[-0.5, -0.4, 0.05, 0.1, -0.1, 0.8] * (1 + 0.05 * rng.standard_normal(6)), 0.3 * rng.standard_normal(M)])
    d = np.concatenate([0.02 * rng.standard_normal(6), 0.5 * rng.standard_normal(M)])
    return {'c = 1': a, 'seeded': b}, d


def gpu_fixture():
    """Everything the fixture holds, computed by the loaded library: {key: array}; and the run figures per scene."""
    import torch
    from superdsm_amd import engine, testing as T
    from test_loss_arithmetic_gpu import _blob_scene
    y, atoms = _blob_scene()
    images, out, figures = {}, {}, {}
    for name, (margin, kw, _, cls) in SCENES.items():
        if margin not in images:
            images[margin] = engine.DeviceImage(y, None, atoms, margin)
        batch = engine.Batch(images[margin], [[1]], T._toy_cfg(background_margin=margin, **kw), want_xi=True)
        batch.launch()
        torch.cuda.synchronize()
        rec, st = batch.records(), batch.inspect_states()[0]
        M = int(rec['n_deform'][0])
        nnz, hz, kh = _run_words(batch)
        figures[name] = dict(M=M, env=st['env_size'], hzmax=st['hzmax'], status=int(rec['status'][0]), nnz=nnz, hz=hz, kh=kh)
        out[f'{name}/records'] = np.frombuffer(rec.tobytes(), np.uint8).copy()
        out[f'{name}/xi'] = batch.xi_dev.cpu().numpy()[:M].copy()
        points, d = _points(M)
        for pname, p in points.items():
            ev = batch.evaluate([p])[0]
            out[f'{name}/{pname}/eval'] = np.concatenate([[ev['psi'], ev['psi_value']], ev['grad'], ev['hess_theta'].ravel()])
            for layout in _layouts(M, st['env_size'], cls):
                res = batch.evaluate_step(layout, [p], direction=[d], reg_mu=0.0, tau=0.0, t0=1.0, dense=False)[0]
                assert res['rc'] >= 0, (name, pname, layout)
                out[f'{name}/{pname}/{layout}/step'] = np.concatenate([[res['rc'], res['psi_value'], res['psi'], res['lam2']], res['line'], res['grad'], res['dir']])
                env = res['env']
                out[f'{name}/{pname}/{layout}/env'] = env.copy() if len(env) <= ENV_WHOLE else np.frombuffer(hashlib.sha256(env.tobytes()).digest(), np.uint8).copy()
    return out, figures


@pytest.fixture(scope='module')
def computed():
    import torch
    from superdsm_amd import _capi
    assert torch.cuda.is_available(), 'these tests need a GPU'
    _capi.lib()
    return gpu_fixture()


def test_the_scenes_cover_the_entry_counts_and_the_leading_entries(computed):
    _, figures = computed
    kh_all, hz_fast, slow = set(), set(), set()
    for name, f in figures.items():
        M, env, hzmax = SCENES[name][2]
        cls = SCENES[name][3]
        print(name, 'M', f['M'], 'envelope', f['env'], 'hzmax', f['hzmax'], 'runs', len(f['nnz']), 'kh', sorted(set(f['kh'].tolist())), 'hz', sorted(set(f['hz'].tolist())))
        assert (f['status'], f['M'], f['env'], f['hzmax']) == (0, M, env, hzmax), name
        assert (f['hz'] >= 1).all() and (f['hz'] <= f['nnz']).all() and f['hz'].max() == hzmax and (f['nnz'] <= np.repeat(f['kh'], 64)[:len(f['nnz'])]).all()
        assert len(f['nnz']) % 64 != 0                       # lanes beyond the last run: they pass through as empty runs
        fits = lambda lay: 6 + M <= LIMITS[lay][0] and env <= LIMITS[lay][1]
        assert cls == ('class 1' if fits('class 1') else 'class 1b' if fits('class 1b') else 'class 3')
        kh_all |= set(f['kh'].tolist())
        if hzmax <= HZREG:
            hz_fast |= set(f['hz'].tolist())
        else:
            slow.add(cls)
    assert set(NEEDED_KH) <= kh_all and {k % EBATCH for k in kh_all} == {0, 1, 2, 3}, sorted(kh_all)
    assert {1, HZREG} <= hz_fast and slow == {'class 1', 'class 1b'}, (sorted(hz_fast), slow)


def test_every_result_has_the_bytes_of_the_fixture(computed):
    out, _ = computed
    gold = np.load(GOLDEN)
    assert sorted(gold.files) == sorted(out), (sorted(set(gold.files) ^ set(out)))
    assert any('/light/' in k for k in out) and any('/class 1/' in k for k in out) and any('/class 1b/' in k for k in out)
    differ = [k for k in sorted(out) if out[k].dtype != gold[k].dtype or out[k].tobytes() != gold[k].tobytes()]
    assert not differ, differ
