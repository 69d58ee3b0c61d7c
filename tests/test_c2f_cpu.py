"""The coarse-to-fine region analysis without a GPU: the stage contract, the native marker flood against a heapq statement of the
rule, every branch of the split loop under a scripted energy and flood, and the cluster markers on edge cases."""
import heapq
import math

import numpy as np
import pytest


def _flood_rule(image, markers, mask):
    """The restated flood in its own words: markers (inside the mask) first in raster order with age 0; pop the smallest (value,
    age, index); label and push the unlabelled admissible neighbours up, left, right, down."""
    H, W = image.shape
    out = np.zeros((H, W), np.int64)
    heap = []
    for r in range(H):
        for c in range(W):
            if markers[r, c] and (mask is None or mask[r, c]):
                out[r, c] = markers[r, c]
                heap.append((image[r, c], 0, r * W + c))
    heapq.heapify(heap)
    age = 0
    while heap:
        _, _, p = heapq.heappop(heap)
        r, c = divmod(p, W)
        for rr, cc in ((r - 1, c), (r, c - 1), (r, c + 1), (r + 1, c)):
            if 0 <= rr < H and 0 <= cc < W and out[rr, cc] == 0 and (mask is None or mask[rr, cc]):
                out[rr, cc] = out[r, c]
                age += 1
                heapq.heappush(heap, (image[rr, cc], age, rr * W + cc))
    return out


def test_stage_contract_and_af_min_atom_radius():
    from superdsm_amd import C2F_RegionAnalysis, automation, config, pipeline
    stage = C2F_RegionAnalysis()
    assert stage.name == 'c2f-region-analysis'
    assert list(stage.inputs) == ['y', 'dsm_cfg']
    assert list(stage.outputs) == ['y_mask', 'atoms', 'adjacencies', 'seeds', 'clusters']
    from superdsm_amd.c2freganal import DEFAULTS
    assert DEFAULTS == dict(seed_connectivity=8, min_atom_radius=15, max_atom_norm_energy=0.05, min_norm_energy_improvement=0.1,
                            max_cluster_marker_irregularity=0.2)
    assert stage.configure_ex(10, 14, 28) == {'min_atom_radius': (14, 0.33, dict(type=int))}
    pl = pipeline.create_reference_pipeline()
    assert [s.name for s in pl.stages] == ['preprocess', 'dsm', 'c2f-region-analysis', 'global-energy-minimization', 'postprocess']
    cfg, scale = automation.create_config(pl, config.Config({'AF_scale': 10}))
    assert cfg.get('c2f-region-analysis/min_atom_radius', None) == int(0.33 * 10 * math.sqrt(2))
    cfg, _ = automation.create_config(pl, config.Config({'AF_scale': 10, 'c2f-region-analysis': {'AF_min_atom_radius': 0.5}}))
    assert cfg.get('c2f-region-analysis/min_atom_radius', None) == int(0.5 * 10 * math.sqrt(2))


def test_native_flood_hand_cases():
    from superdsm_amd.c2freganal import watershed, watershed_native
    # a plateau between two markers: the left marker's flood arrives first (raster order of the markers, then push age)
    img = np.zeros((1, 5))
    mk = np.array([[1, 0, 0, 0, 2]])
    for f in (watershed, watershed_native):
        assert f(img, mk).tolist() == [[1, 1, 1, 2, 2]]
    # a pixel is labelled when it is pushed; the lower value is popped first, so marker 2 reaches the middle through its valley
    img = np.array([[0., 3., 3., 1., 0.]])
    mk = np.array([[1, 0, 0, 0, 2]])
    for f in (watershed, watershed_native):
        assert f(img, mk).tolist() == [[1, 1, 2, 2, 2]]
    # pixels outside the mask are never labelled, markers outside it are dropped, unreachable pixels stay 0
    img = np.zeros((3, 3))
    mk = np.array([[1, 0, 0], [0, 0, 0], [0, 0, 2]])
    mask = np.array([[1, 0, 1], [0, 0, 1], [1, 1, 0]], bool)
    for f in (watershed, watershed_native):
        assert f(img, mk, mask).tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 0]]
    # neighbour order up, left, right, down: the pixel under the marker is pushed last and popped last among equals
    img = np.zeros((2, 2))
    mk = np.array([[1, 0], [0, 0]])
    for f in (watershed, watershed_native):
        assert f(img, mk).tolist() == [[1, 1], [1, 1]]


@pytest.mark.parametrize('seed', range(12))
def test_native_flood_matches_heapq_rule(seed):
    from superdsm_amd.c2freganal import watershed, watershed_native
    rng = np.random.default_rng(seed)
    H, W = (int(v) for v in rng.integers(1, 40, 2))
    img = rng.integers(0, 3 + seed % 4, (H, W)).astype(float)          # few distinct values: plateau ties everywhere
    mk = np.zeros((H, W), np.int32)
    for label in range(1, int(rng.integers(2, 7))):
        r, c = rng.integers(0, H), rng.integers(0, W)
        mk[r:r + int(rng.integers(1, 4)), c:c + int(rng.integers(1, 4))] = label     # markers of several pixels
    mask = None if seed % 3 == 0 else rng.random((H, W)) > 0.25
    want = _flood_rule(img, mk, mask)
    assert np.array_equal(watershed_native(img, mk, mask), want)
    assert np.array_equal(watershed(img, mk, mask), want)


# ---- the split loop ----------------------------------------------------------------------------------------------------------------

class _Script:
    """A flood that cuts the admissible pixels in raster order (the first k get label 1) and an energy that answers from a list."""

    def __init__(self, cuts, energies):
        self.cuts, self.energies = list(cuts), list(energies)
        self.markers, self.requests = [], []

    def flood(self, image, markers, mask):
        self.markers.append(markers.copy())
        idx = np.flatnonzero(mask)
        k = self.cuts.pop(0)
        k = len(idx) - k[1] if isinstance(k, tuple) else k                 # ('c2', n): the last n pixels get label 2
        out = np.zeros(mask.size, np.int32)
        out[idx[:k]] = 1
        out[idx[k:]] = 2
        return out.reshape(mask.shape)

    def energy(self, y_crop, mask_crop, atoms_map, footprint, dsm_cfg):
        self.requests.append((tuple(footprint), int(np.isin(atoms_map, footprint).sum())))
        v = self.energies.pop(0)
        if isinstance(v, Exception):
            raise v
        return v


def _cluster_scene():
    from superdsm_amd.image import Image
    rr, cc = np.mgrid[:30, :60]
    y = 0.2 + 0.1 * np.cos(2 * np.pi * rr / 6) * np.cos(2 * np.pi * cc / 6) + 1e-4 * cc    # a grid of isolated maxima
    return Image.create_from_array(y, normalize=False), np.ones(y.shape, int), np.ones(y.shape, bool)


def _run(script, **params):
    from superdsm_amd import c2freganal as cr
    yi, clusters, y_mask = _cluster_scene()
    p = cr._params(**{'min_atom_radius': 2, **params})
    return cr._process_cluster_impl(clusters, 1, yi, y_mask, p, {}, script.energy, flood=script.flood)


def test_split_loop_reaches_every_branch():
    n = 30 * 60
    s = _Script(cuts=[10, ('c2', 10), 900, 901, 902, 903, n - 20],
                energies=[1.0,                       # root: above max_atom_norm_energy -> split
                          None, None,                # both None: try again
                          None, 0.5,                 # c1 None: c0 takes c2's seed
                          0.5, RuntimeError('x'),    # c2 raises -> None: try again
                          0.95, 0.95,                # improvement 0.05 < 0.1: try again
                          0.05, 0.5])                # accepted: c1 at max_atom_norm_energy is a leaf, c2 is queued ...
    cluster, leaves, atoms_map = _run(s)
    assert s.cuts == [] and s.energies == []
    # c1 too small (10 px < pi * 2^2): the next try keeps c2's seed as c1's
    assert np.array_equal(s.markers[1] == 1, s.markers[0] == 2)
    # c2 too small: c0 keeps its seed
    assert np.array_equal(s.markers[2] == 1, s.markers[1] == 1)
    # (None, value): the seed is swapped; (value, None) and (None, None): it is not
    assert np.array_equal(s.markers[3] == 1, s.markers[2] == 1)
    assert np.array_equal(s.markers[4] == 1, s.markers[3] == 2)
    assert np.array_equal(s.markers[5] == 1, s.markers[4] == 1)
    assert np.array_equal(s.markers[6] == 1, s.markers[5] == 1)
    # rejected splits leave atoms_map as it was: every request is for label 1 or the one new label 2
    assert [fp for fp, _ in s.requests] == [(1,)] + [(1,), (2,)] * 5
    assert [size for _, size in s.requests] == [n, 900, 900, 901, 899, 902, 898, 903, 897, n - 20, 20]
    # ... and too small to be split again (20 px < 2 pi 2^2): a leaf
    assert sorted(np.unique(atoms_map).tolist()) == [1, 2] and (atoms_map == 2).sum() == 20
    assert sorted((sorted(c.footprint)[0], c.normalized_energy) for c in leaves) == [(1, 0.05), (2, 0.5)]


def test_split_loop_leaf_and_small_root():
    n = 30 * 60
    s = _Script(cuts=[], energies=[0.05])                   # at max_atom_norm_energy: no split
    _, leaves, atoms_map = _run(s)
    assert len(leaves) == 1 and (atoms_map == 1).all() and s.markers == []
    s = _Script(cuts=[], energies=[0.5])                    # above it, but smaller than two atoms: no split
    _, leaves, atoms_map = _run(s, min_atom_radius=int(math.sqrt(n / 2 / math.pi)) + 1)
    assert len(leaves) == 1 and (atoms_map == 1).all() and s.markers == []


def test_split_loop_errors_of_the_root():
    from superdsm_amd.c2freganal import C2FError
    with pytest.raises(C2FError, match='cluster 1'):
        _run(_Script(cuts=[], energies=[None]))
    with pytest.raises(ZeroDivisionError):
        _run(_Script(cuts=[], energies=[ZeroDivisionError('root')]))


def test_split_loop_cache_answers_repeats():
    # two splits with the same cut ask for the same regions: the second is answered by the cache of the cluster
    s = _Script(cuts=[900, 900], energies=[1.0, 0.95, 0.95])
    with pytest.raises(IndexError):                             # the third split finds no cut left in the script
        _run(s)
    assert len(s.requests) == 3 and len(s.markers) == 3 and s.energies == []


# ---- markers and label assembly ----------------------------------------------------------------------------------------------------

def test_cluster_markers_edge_cases():
    from superdsm_amd.c2freganal import cluster_markers_host
    y = -np.ones((6, 7))
    m, cm = cluster_markers_host(y, 0.2)
    assert m.all() and not cm.any()
    m, cm = cluster_markers_host(y, -0.5)                       # the background is "irregular" (0 > thr) as well
    assert not m.any() and not cm.any()
    m, cm = cluster_markers_host(-y, 0.2)                       # all foreground: one component, relabelled 0
    assert m.all() and not cm.any()
    y = -np.ones((10, 12))
    y[1, 1:9] = 1                                               # a line: irregularity 1, masked although it comes first
    y[4:9, 3:8] = 1                                             # a 5 x 5 square: 16 / 25
    y[9, 11] = 1                                                # one pixel in the corner: 1 / 1
    m, cm = cluster_markers_host(y, 0.7)
    assert not m[1, 1:9].any() and m[4:9, 3:8].all() and not m[9, 11] and m[y < 0].all()
    assert (cm[4:9, 3:8] == 1).all() and cm.max() == 1 and (cm > 0).sum() == 25


def test_cluster_markers_border_does_not_erode():
    from superdsm_amd.c2freganal import cluster_markers_host
    y = -np.ones((10, 10))
    y[:4, :4] = 1                                               # the border does not erode: 7 boundary pixels of 16 = 0.4375
    y[6:, 6:] = 1
    assert cluster_markers_host(y, 0.44)[1].max() == 2
    m, cm = cluster_markers_host(y, 0.43)
    assert cm.max() == 0 and not m[:4, :4].any() and not m[6:, 6:].any()


def test_normalize_labels_map():
    from superdsm_amd.c2freganal import _normalize_labels_map
    res, tr = _normalize_labels_map(np.array([[3, 5], [5, 7]]), first_label=0)
    assert res.tolist() == [[0, 1], [1, 2]] and tr == {3: 0, 5: 1, 7: 2}
    res, tr = _normalize_labels_map(np.array([[0, 4], [9, 4]]), first_label=1, skip_labels=[0])
    assert res.tolist() == [[0, 1], [2, 1]] and tr == {4: 1, 9: 2}


def test_host_restatement_assembles_atoms_seeds_and_adjacencies():
    """The whole restatement on a synthetic image with a deterministic fake energy (the parts of a split improve while they are big)."""
    from superdsm_amd import c2freganal as cr, synth
    layout = synth.random_layout((96, 128), 5, 12, 3, min_sep=0.9)
    g = synth.render_image((96, 128), layout, 3)
    y = synth.offset_image(g, 10)

    def energy(y_crop, mask_crop, atoms_map, footprint, dsm_cfg):
        n = int((np.isin(atoms_map, footprint) & mask_crop).sum())
        return n / 4000.0

    out = cr.region_analysis_host(y, dict(background_margin=8), energy=energy, flood=cr.watershed_native, min_atom_radius=4)
    atoms, clusters, adj = out['atoms'], out['clusters'], out['adjacencies']
    assert atoms.max() == len(out['seeds']) > clusters.max() >= 1
    assert ((atoms > 0) == (clusters > 0)).all()
    for a in range(1, atoms.max() + 1):
        s = tuple(int(v) for v in out['seeds'][a - 1])
        assert atoms[s] == a
        for b in adj[a]:
            assert a in adj[b] and adj.get_cluster_label(a) == adj.get_cluster_label(b)
    # the same with the Python heap flood
    again = cr.region_analysis_host(y, dict(background_margin=8), energy=energy, min_atom_radius=4)
    assert np.array_equal(again['atoms'], atoms) and np.array_equal(again['clusters'], clusters)


# ---- the lock-step driver of a set of images ------------------------------------------------------------------------------------------

def _fake_energy(y_crop, mask_crop, atoms_map, footprint, dsm_cfg):
    """The fake energy of test_host_restatement_assembles_atoms_seeds_and_adjacencies."""
    n = int((np.isin(atoms_map, footprint) & mask_crop).sum())
    return n / 4000.0


class _Rounds:
    """What the driver reads of an ``EnergyRounds``: every request answered footprint by footprint with ``energy``."""

    def __init__(self, dsm_cfg, energy=_fake_energy):
        self.dsm_cfg, self.energy, self.log, self.launches = dsm_cfg, energy, [], 0

    def solve(self, requests):
        self.launches += 1
        self.log.append(dict(crops=len(requests), plans=1, candidates=sum(len(r[3]) for r in requests), resolved=0, resolve_plans=0, seconds=0.0))
        return [[self.energy(y, m, a, fp, self.dsm_cfg) for fp in fps] for y, m, a, fps in requests]


def _lockstep_images():
    from superdsm_amd import synth
    ys = []
    for shape, n, r, seed in (((96, 128), 6, 12, 7), ((64, 96), 2, 10, 5), ((96, 128), 5, 12, 3)):
        layout = synth.random_layout(shape, n, r, seed, min_sep=0.9)
        ys.append(synth.offset_image(synth.render_image(shape, layout, seed), 10))
    return ys + [-np.ones((20, 30))]


def _lockstep(ys, dsm_cfgs, new_rounds=_Rounds):
    """The driver behind a host stand-in for the device phase, with the Python heap flood."""
    import scipy.ndimage as ndi
    from superdsm_amd import c2freganal as cr
    params = cr._params(min_atom_radius=4)
    marked = []
    for y in ys:
        y_mask, markers = cr.cluster_markers_host(y, params['max_cluster_marker_irregularity'])
        marked.append((y_mask, markers, int(markers.max()), ndi.distance_transform_edt(markers == 0)))
    return cr.region_analysis_lockstep(ys, dsm_cfgs, [params] * len(ys), marked, flood=cr.watershed, new_rounds=new_rounds)


def _assert_same_outputs(got, want):
    assert np.array_equal(got['y_mask'], want['y_mask'])
    assert np.array_equal(got['clusters'], want['clusters'])
    assert np.array_equal(got['atoms'], want['atoms'])
    assert [tuple(s) for s in got['seeds']] == [tuple(s) for s in want['seeds']]
    ga, wa = got['adjacencies'], want['adjacencies']
    assert ga.atom_labels == wa.atom_labels
    for a in wa.atom_labels:
        assert ga[a] == wa[a] and ga.get_cluster_label(a) == wa.get_cluster_label(a)


@pytest.fixture(scope='module')
def lockstep_reference():
    """The four images and what the sequential definition gives for each, with the same energy and flood."""
    from superdsm_amd import c2freganal as cr
    ys = _lockstep_images()
    return ys, [cr.region_analysis_host(y, dict(background_margin=8), energy=_fake_energy, min_atom_radius=4) for y in ys]


def test_lockstep_driver_equals_the_sequential_definition(lockstep_reference):
    """All clusters of four images in lock step (3, 1, 2 and 0 rounds; 4, 2, 3 and 0 clusters) against ``region_analysis_host`` image by
    image; the set takes as many rounds as its image with the most; the order of the images does not matter."""
    ys, want = lockstep_reference
    cfgs = [dict(background_margin=8) for _ in ys]
    made = []

    def new_rounds(c):
        made.append(_Rounds(c))
        return made[-1]

    outputs, stats, set_stats, errors = _lockstep(ys, cfgs, new_rounds)
    assert errors == [None] * 4 and len(made) == 1                  # one configuration: one rounds object
    for got, ref in zip(outputs, want):
        _assert_same_outputs(got, ref)
    assert [int(w['clusters'].max()) for w in want] == [4, 2, 3, 0]
    assert [st['clusters'] for st in stats] == [4, 2, 3, 0]
    assert set_stats['n_rounds'] == 3 and [len(st['rounds']) for st in stats] == [3, 1, 2, 0]
    assert len(set_stats['rounds']) == 3 and set_stats['launches'] == made[0].launches == 3
    assert stats[0]['rounds'][0]['crops'] == 4 and set_stats['rounds'][0]['crops'] == 4 + 2 + 3      # round 1: every cluster's root
    back, back_stats, back_set, back_errors = _lockstep(ys[::-1], cfgs)
    assert back_errors == [None] * 4 and back_set['n_rounds'] == 3 and [len(st['rounds']) for st in back_stats] == [0, 2, 1, 3]
    for got, ref in zip(back[::-1], want):
        _assert_same_outputs(got, ref)


def test_lockstep_driver_takes_a_failing_image_out_of_the_set(lockstep_reference):
    """The third image has a configuration of its own (so the driver forms two groups) whose rounds object answers None: its first
    cluster has no normalised energy, the image leaves the set with a ``C2FError`` and the other three finish as they do alone.  The
    call for a single image raises that image's own exception."""
    from superdsm_amd import c2freganal as cr
    ys, want = lockstep_reference
    cfgs = [dict(background_margin=8) for _ in ys]
    cfgs[2]['epsilon'] = 2.0
    made = []

    def new_rounds(c):
        made.append(_Rounds(c, energy=(lambda *a: None) if 'epsilon' in c else _fake_energy))
        return made[-1]

    outputs, stats, set_stats, errors = _lockstep(ys, cfgs, new_rounds)
    assert len(made) == 2 and 'epsilon' in made[1].dsm_cfg and 'epsilon' not in made[0].dsm_cfg
    assert [e is None for e in errors] == [True, True, False, True] and outputs[2] is None
    assert isinstance(errors[2], cr.C2FError) and 'cluster 1:' in str(errors[2])
    for i in (0, 1, 3):
        _assert_same_outputs(outputs[i], want[i])
    assert set_stats['n_rounds'] == 3 and [len(st['rounds']) for st in stats] == [3, 1, 1, 0]
    assert made[1].launches == 1 and made[0].launches == 3 and set_stats['launches'] == 4
    # the set of one image, as region_analysis_gpu returns it
    one = _lockstep(ys[2:3], cfgs[2:3], new_rounds)
    with pytest.raises(cr.C2FError, match='cluster 1:') as info:
        cr._set_of_one(*one)
    assert info.value is one[3][0] and not hasattr(info.value, 'image_index')
    out, st = cr._set_of_one(*_lockstep(ys[:1], cfgs[:1]))
    _assert_same_outputs(out, want[0])
    assert st['clusters'] == 4 and len(st['rounds']) == 3 and st['launches'] == 3
    assert {'crops', 'plans', 'candidates', 'resolved', 'resolve_plans', 'seconds'} <= set(st['rounds'][0])
    assert {'flood_s', 'host_split_s', 'assemble_s', 'energy_s', 'total_s'} <= set(st)


def _energy_record(status=0, energy=-30.0, n=100, pos=40, neg=60):
    from superdsm_amd import _capi
    r = np.zeros(1, _capi.RECORD_DTYPE)
    r['status'], r['energy'], r['n_pixels'], r['n_positive'], r['n_negative'] = status, energy, n, pos, neg
    return r[0]


def test_record_reader_returns_errors_as_objects_and_never_a_non_finite_value():
    """The one reader of the energy path (``c2f_energy.record_result``): None for a region without an energy, an error object for a
    failed, given-up or non-finite record, ``energy / n`` otherwise."""
    from superdsm_amd import _capi, c2f_energy, c2freganal
    from superdsm_amd.objects import CvxprogError
    assert c2freganal.C2FError is c2f_energy.C2FError
    read = c2f_energy.record_result
    assert read(_energy_record(), 3) == -30.0 / 100 and isinstance(read(_energy_record(), 3), float)
    assert read(_energy_record(status=_capi.CAND_FALLBACK, energy=12.5, n=8, pos=1, neg=7), 0) == 12.5 / 8
    for r in (_energy_record(n=0, pos=0, neg=0), _energy_record(pos=100, neg=0), _energy_record(pos=0, neg=100),
              _energy_record(status=_capi.CAND_GIVEN_UP, energy=np.nan, pos=100, neg=0)):
        assert read(r, 0) is None
    for status in (_capi.CAND_ERROR, _capi.CAND_UNSUPPORTED):
        e = read(_energy_record(status=status), 7)
        assert isinstance(e, CvxprogError) and e.cidx == 7
    for r in (_energy_record(status=_capi.CAND_GIVEN_UP, energy=np.nan), _energy_record(status=_capi.CAND_GIVEN_UP),
              _energy_record(energy=np.nan), _energy_record(energy=np.inf), _energy_record(energy=-np.inf)):
        e = read(r, 5)
        assert isinstance(e, c2f_energy.C2FError) and not isinstance(e, float) and 'candidate 5' in str(e)


def test_energy_config_drops_every_cpu_only_key():
    from superdsm_amd import c2f_energy, objects
    dsm_cfg = dict({k: 1 for k in objects._CPU_ONLY_KEYS}, scale=1000, smooth_amount=4, background_margin=7, init='elliptical')
    cfg, margin = c2f_energy.energy_config(dsm_cfg)
    assert len(objects._CPU_ONLY_KEYS) == 5 and not set(objects._CPU_ONLY_KEYS) & set(cfg)
    assert cfg == dict(scale=1000, smooth_amount=np.inf, no_trivial_rule=True, init='elliptical') and margin == 7.0
    assert dsm_cfg['smooth_amount'] == 4 and 'background_margin' in dsm_cfg          # the caller's dict is left alone
