"""Scene construction and one-call GPU solves shared by tests, __graft_entry__.smoke() and bench.py."""
import numpy as np

from . import synth
from .atoms import AtomAdjacencyGraph


def make_scene(workload='synthetic256', max_size=3, alpha_factor=None, layout_index=0):
    """Synthetic image -> y, atoms, adjacency graph, candidate footprints and the dsm/* hyper-parameters of the
    BASELINE.json config the workload stands for.  ``layout_index`` (bbbc039_like only): which of the
    eight reference object tables places the nuclei."""
    spec = dict(synth.WORKLOADS[workload])
    if workload == 'bbbc039_like':
        shape, layout = synth.bbbc039_like_layout(spec['seed'], layout_index)
        spec['seed'] += 7919 * layout_index
        af = 0.00033 if alpha_factor is None else alpha_factor       # examples/BBBC039/task.json: AF_alpha
    else:
        shape = spec['shape']
        layout = synth.random_layout(shape, spec['n'], spec['radius'], spec['seed'], min_sep={'synthetic4096': 0.6, 'synthetic512': 1.2}.get(workload, 2.2))
        af = {'synthetic256': 0.00033, 'synthetic512': 0.00033, 'synthetic4096': 0.00033, 'gowt1_like': 0.0005, 'nih3t3_like': 0.000375}[workload] if alpha_factor is None else alpha_factor
    g = synth.render_image(shape, layout, spec['seed'])
    y = synth.offset_image(g, spec['scale'])
    atoms, clusters, seeds = synth.make_atoms(y, layout, spec['seed'])
    adj = AtomAdjacencyGraph(atoms, clusters, y > 0, seeds)
    footprints = synth.enumerate_candidates(adj, max_size=max_size)
    return dict(workload=workload, g=g, y=y, atoms=atoms, clusters=clusters, seeds=seeds, adjacencies=adj, footprints=footprints,
                dsm_cfg=synth.dsm_config_for_scale(spec['scale'], af), scale=spec['scale'])


def solve_scene_gpu(scene, footprints=None, want_xi=False, mode=None):
    from . import engine
    import torch
    fps = scene['footprints'] if footprints is None else footprints
    img = engine.DeviceImage(scene['y'], None, scene['atoms'], scene['dsm_cfg']['background_margin'])
    batch = engine.Batch(img, fps, scene['dsm_cfg'], want_xi=want_xi, mode=mode)
    batch.launch()
    torch.cuda.synchronize()
    recs = batch.records()
    frags = batch.fragments(recs)
    out = dict(records=recs, fragments=frags, batch=batch, image=img)
    if want_xi:
        out['xi'] = batch.xi_dev.cpu().numpy()
        out['xi_offsets'] = batch.xi_offsets()
    return out


def plan_inputs(sides, n_images=1, stray=False, **cfg):
    """The arguments of sdsm_plan_create(_multi) for one candidate per atom, atoms = squares of the given side lengths on a grid (statistics
    only: area, extents).  ``n_images`` > 1: the candidates are dealt to the images in turn, and the images differ in shape.  ``stray``:
    every footprint also names label 0, a label above the image's atoms and an atom of area 0 (the plan skips all three).  ``cfg``: dsm/* keys
    that replace the defaults of these plans."""
    n = len(sides)
    pitch = max(list(sides) + [2])
    per_row = 60000 // pitch
    mine = [list(range(im, n, n_images)) for im in range(n_images)]
    H, W, n_atoms, stats, label = [], [], [], [], {}
    for im, cands in enumerate(mine):
        st = np.zeros((len(cands) + 1 + bool(stray), 6), np.int32)
        for k, ci in enumerate(cands, start=1):
            sd = sides[ci]
            r, c = ((k - 1) // per_row) * pitch, ((k - 1) % per_row) * pitch
            st[k] = (sd * sd, r, r + sd - 1, c, c + sd - 1, 0)
            label[ci] = k
        H.append(((max(len(cands), 1) - 1) // per_row + 1) * pitch + 7 * im)
        W.append(per_row * pitch + 13 * im)
        n_atoms.append(len(st) - 1)
        stats.append(st)
    assert max(H) <= 65535
    fps = [[label[ci]] + ([0, n_atoms[ci % n_images] + 2, n_atoms[ci % n_images]] if stray else []) for ci in range(n)]
    return dict(H=np.array(H, np.int32), W=np.array(W, np.int32), n_atoms=np.array(n_atoms, np.int32), stats=stats,
                cfg=dict(dict(alpha=0.033, smooth_amount=4, smooth_subsample=8, background_margin=0), **cfg), n=n,
                offsets=np.concatenate([[0], np.cumsum([len(f) for f in fps])]).astype(np.int32), labels=np.array(sum(fps, []), np.int32).reshape(-1),
                image_of=(np.arange(n) % n_images).astype(np.int32))


def plan_of_squares(sides, **kw):
    """A host-only plan over the squares of :func:`plan_inputs` (sdsm_plan_create; with ``n_images`` > 1 sdsm_plan_create_multi)."""
    import ctypes as C
    from . import _capi
    lib = _capi.lib()
    a = plan_inputs(sides, **kw)
    cfg = _capi.make_config(a['cfg'])
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    if len(a['stats']) == 1:
        plan = lib.sdsm_plan_create(int(a['H'][0]), int(a['W'][0]), int(a['n_atoms'][0]), ptr(a['stats'][0]), C.byref(cfg), a['n'], ptr(a['offsets']), ptr(a['labels']))
    else:
        tables = (C.c_void_p * len(a['stats']))(*[st.ctypes.data for st in a['stats']])
        plan = lib.sdsm_plan_create_multi(len(a['stats']), ptr(a['H']), ptr(a['W']), ptr(a['n_atoms']), C.cast(tables, C.c_void_p), C.byref(cfg), a['n'],
                                          ptr(a['offsets']), ptr(a['labels']), ptr(a['image_of']))
    assert plan, lib.sdsm_last_error()
    return plan


PLAN_LIST_NAMES = ('all', 'beyond_1', 'beyond_2', 'group_members', 'row_members', 'setup_small', 'setup_big')
# the plans whose launch lists tests/golden/plan_lists.json records: name -> (sides of plan_of_squares, scheduling modes)
PLAN_LIST_CASES = {
    'clusters': ([30] * 200 + [70] * 20 + [100] * 6 + [180] * 2, (0, 1, 2)),      # groups, row members, latency groups; one setup launch
    'setup_split': ([30] * 300 + [190] * 2, (0,)),                                # the two-launch setup: 300 small regions, 2 beyond the small tables
    'no_groups': ([70] * 8000 + [120] * 40, (0,)),                                # thousands of mid-size regions: no groups, no row members
}


# the plans whose workspace layout, kernel arguments and candidate descriptors tests/golden/plan_layout.json records:
# name -> (sides, scheduling modes, further arguments of plan_inputs).  What each one is there for: tests/test_plan_layout_cpu.py.
PLAN_LAYOUT_CASES = dict({name: (sides, modes, {}) for name, (sides, modes) in PLAN_LIST_CASES.items()},
                         two_images=([30] * 40 + [100] * 2, (0,), dict(n_images=2)),
                         no_deform=([30] * 40 + [100] * 2, (0,), dict(smooth_amount=float('inf'))),
                         dense_grid=([30] * 10 + [100] * 2, (0,), dict(smooth_amount=8, smooth_subsample=4)),
                         stray_labels=([30] * 40 + [100] * 2, (0,), dict(stray=True)),
                         empty=([], (0,), {}))


def plan_cases_text():
    """PLAN_LAYOUT_CASES as the stand-alone check of the plan unit reads them (tests/host/plan_check.cpp): white-space separated numbers, per case
    its name, modes, images (H, W, atoms, statistics), configuration, footprints and image indices -- the very arrays :func:`plan_of_squares` passes."""
    from . import _capi
    words = [len(PLAN_LAYOUT_CASES)]
    for name, (sides, modes, kw) in PLAN_LAYOUT_CASES.items():
        a = plan_inputs(sides, **kw)
        cfg = _capi.make_config(a['cfg'])
        words += [name, len(modes), *modes, len(a['stats']), *a['H'], *a['W'], *a['n_atoms']]
        for st in a['stats']:
            words += st.ravel().tolist()
        words += [repr(float(getattr(cfg, f))) for f in ('scale', 'epsilon', 'alpha', 'smooth_amount', 'gaussian_shape_multiplier', 'background_margin')]
        words += [cfg.smooth_subsample, cfg.init_elliptical, cfg.max_iters, cfg.flags, a['n'], *a['offsets'], *a['labels'], *a['image_of']]
    return ' '.join(str(w) for w in words) + '\n'


def plan_lists(plan, mode):
    """The launch lists of a host-only plan in the given scheduling mode (sdsm_plan_lists): spans as 7 x (first, count), and `order`."""
    import ctypes as C
    from . import _capi
    lib = _capi.lib()
    _capi.check(lib.sdsm_plan_set_latency_mode(plan, mode), 'sdsm_plan_set_latency_mode')
    spans = np.zeros((7, 2), np.int32)
    _capi.check(lib.sdsm_plan_lists(plan, spans.ctypes.data_as(C.c_void_p), None), 'sdsm_plan_lists')
    order = np.zeros(int(spans[:, 1].sum()), np.int32)
    _capi.check(lib.sdsm_plan_lists(plan, spans.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.c_void_p)), 'sdsm_plan_lists')
    return spans, order


def plan_image(plan, n):
    """sdsm_plan_image of a plan of n candidates in its current mode: the kernel arguments over a null workspace (bytes), the descriptors
    (_capi.CAND_DESC_DTYPE)."""
    import ctypes as C
    from . import _capi
    params, cand = np.zeros(_capi.PLAN_PARAMS_BYTES, np.uint8), np.zeros(n, _capi.CAND_DESC_DTYPE)
    _capi.check(_capi.lib().sdsm_plan_image(plan, params.ctypes.data_as(C.c_void_p), params.nbytes, cand.ctypes.data_as(C.c_void_p), cand.nbytes), 'sdsm_plan_image')
    return params, cand


def plan_layout_record(params, cand, sizes, layout):
    """What tests/golden/plan_layout.json keeps of a plan in one mode: the SHA-256 of the parameter blob, one per CandDesc field (the
    column's bytes, so that a difference names the field), the four size queries and the 16 values of sdsm_plan_layout."""
    import hashlib
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return dict(params=sha(params), cand={f: sha(cand[f]) for f in cand.dtype.names},
                workspace_bytes=int(sizes[0]), mask_bytes=int(sizes[1]), total_pixels=int(sizes[2]), xi_count=int(sizes[3]), layout=[int(v) for v in layout])


def plan_layout_of(plan, n):
    """:func:`plan_layout_record` of a host-only plan in its current mode, with the arrays it was made of: (record, params, cand)."""
    import ctypes as C
    from . import _capi
    lib = _capi.lib()
    params, cand = plan_image(plan, n)
    lay = np.zeros(16, np.int64)
    _capi.check(lib.sdsm_plan_layout(plan, lay.ctypes.data_as(C.c_void_p)), 'sdsm_plan_layout')
    sizes = (lib.sdsm_plan_workspace_bytes(plan), lib.sdsm_plan_mask_bytes(plan), lib.sdsm_plan_total_pixels(plan), lib.sdsm_plan_xi_count(plan))
    return plan_layout_record(params, cand, sizes, lay), params, cand


def dice(a_off, a_frag, b_off, b_frag, shape):
    fa = np.zeros(shape, bool)
    fb = np.zeros(shape, bool)
    fa[a_off[0]:a_off[0] + a_frag.shape[0], a_off[1]:a_off[1] + a_frag.shape[1]] = a_frag
    fb[b_off[0]:b_off[0] + b_frag.shape[0], b_off[1]:b_off[1] + b_frag.shape[1]] = b_frag
    den = fa.sum() + fb.sum()
    return 1.0 if den == 0 else 2.0 * (fa & fb).sum() / den


# ---------------------------------------------------------------------------------------------------------
# the cases of the per-object post-processing tests (tests/test_postprocess_gpu.py and tests/test_postprocess_cpu.py): one seeded
# generator and the extended-precision evaluation of the sums the kernel forms.  NumPy / SciPy only.
# ---------------------------------------------------------------------------------------------------------
POST_LDS_BOUNDARY = 12288        # POST_MAX_BOUNDARY of sdsm_post.hip, and the host's `areas > 12288` rule
POST_CONSTANTS = (0.0, 1e2, 1e4, 1e6)
_EPS = float(np.finfo(np.float64).eps)


class PostFragment:
    """What the post-processing entry points take as an object: ``fg_offset``, ``fg_fragment`` and ``fill_foreground``."""

    def __init__(self, off, frag, tag=''):
        self.fg_offset, self.fg_fragment, self.tag = np.asarray(off, int), np.ascontiguousarray(frag, bool), tag
        self.on_boundary, self.energy, self.cvxprog_region_size = False, 0.0, 1.0

    def fill_foreground(self, out, value=True):
        h, w = self.fg_fragment.shape
        r, c = int(self.fg_offset[0]), int(self.fg_offset[1])
        out[r:r + h, c:c + w] = value * self.fg_fragment


def _post_texture(shape, seed, constant=0.0):
    """Positive intensities (no cancellation in any sum) and their Gaussian, both with ``constant`` added."""
    import scipy.ndimage as ndi
    g = 0.2 + 0.6 * np.random.default_rng(seed).random(shape)
    return g + constant, ndi.gaussian_filter(g, 3) + constant


def _ellipse(h, w):
    rr, cc = np.mgrid[:h, :w]
    return ((rr - (h - 1) / 2) / (h / 2)) ** 2 + ((cc - (w - 1) / 2) / (w / 2)) ** 2 <= 1


def _rect(h, w):
    return np.ones((h, w), bool)


def _image(shape, seed, objects, constant=0.0, bg=None):
    g, gs = _post_texture(shape, seed, constant)
    return dict(g=g, gs=gs, objects=[PostFragment(*o) for o in objects], bg=bg)      # bg None: the oracle's background_mask of the objects


def post_comb(teeth, width, extra=0):
    """Teeth of one pixel on every other row, joined by a spine in column 0, ``extra`` teeth one pixel longer: every pixel is a
    boundary pixel, area = boundary count = teeth * width + teeth - 1 + extra."""
    frag = np.zeros((2 * teeth - 1, width + (1 if extra else 0)), bool)
    frag[::2, :width] = True
    frag[:, 0] = True
    for k in range(extra):
        frag[2 * k, width] = True
    return frag


def post_boundary_count(frag):
    """Mask pixels with a 4-neighbour outside the mask (outside the box counts as outside)."""
    p = np.pad(np.asarray(frag, bool), 1)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return int((p[1:-1, 1:-1] & ~inner).sum())


def _random_objects(rng, H, W, n):
    out = []
    for _ in range(n):
        h, w = int(rng.integers(1, min(H, 12) + 1)), int(rng.integers(1, min(W, 12) + 1))
        frag = _ellipse(h, w) if rng.random() < 0.5 else rng.random((h, w)) < 0.7
        if not frag.any():
            frag[0, 0] = True
        out.append(((int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))), frag, 'random'))
    return out


def _geometry_objects():
    ring = _rect(9, 9)
    ring[3:6, 3:6] = False
    two = _rect(5, 11)
    two[:, 4:7] = False
    rim = np.zeros((9, 9), bool)
    rim[3:6, 3:6] = True
    return [((0, 20), _rect(4, 7), 'top'), ((33, 10), _rect(4, 6), 'bottom'), ((15, 0), _rect(6, 3), 'left'), ((12, 49), _rect(5, 4), 'right'),
            ((0, 0), _rect(3, 3), 'corner'), ((0, 50), _rect(3, 3), 'corner'), ((34, 0), _rect(3, 3), 'corner'), ((34, 50), _rect(3, 3), 'corner'),
            ((10, 10), _rect(1, 1), 'pixel'), ((20, 12), _rect(1, 9), '1xN'), ((22, 30), _rect(8, 1), 'Nx1'), ((8, 34), ring, 'holes'),
            ((24, 8), two, 'two parts'), ((18, 38), rim, 'empty rim'), ((5, 25), np.zeros((3, 4), bool), 'empty')]


def _param_objects():
    return [((0, 0), _ellipse(30, 24), 'corner'), ((40, 60), _ellipse(25, 40), ''), ((95, 120), _ellipse(25, 30), 'corner'), ((50, 0), _ellipse(20, 14), 'left'),
            ((0, 70), _ellipse(12, 30), 'top'), ((80, 40), _ellipse(9, 9), ''), ((100, 5), _rect(6, 17), ''), ((20, 110), _ellipse(33, 21), '')]


POST_PARAMETER_SETS = [(0.5, 0, 1e-4, 1, 0.5), (2.5, 0.5, 1e-4, 2, 1.5), (5, 2, 1e-4, 3, 2), (7.3, 5, 1e-4, 5, 3), (5, 6.7, 1e-4, 8, 2), (2.5, 5, 1e-4, 16, 2)]
POST_DEFAULT = (5, 5, 1e-4, 1, 2)
_SET_SHAPES = [(24, 31), (37, 53), (1, 40), (40, 1), (16, 16), (50, 45), (9, 64)]
POST_SET_EMPTY = (0, 15, 16, 31)


def post_set_images(n=35, seed=100):
    """``n`` small images of mixed shapes with 0 .. 3 objects each; those at POST_SET_EMPTY have none."""
    rng = np.random.default_rng(seed)
    images = []
    for i in range(n):
        shape = _SET_SHAPES[i % len(_SET_SHAPES)]
        objs = [] if i in POST_SET_EMPTY else _random_objects(rng, shape[0], shape[1], 1 + i % 3)
        images.append(_image(shape, seed + 1 + i, objs))
    return images


def post_pooled_images():
    """Two images of one set: (small, comb of 12289, small, solid of 12289) and (small, comb of 12289, small)."""
    comb = post_comb(64, 191, 2)
    solid = np.zeros((97, 128), bool)
    solid[:96] = True
    solid[96, 0] = True
    small = lambda r, c: ((r, c), _ellipse(7, 9), 'small')
    return [_image((300, 230), 21, [small(2, 2), ((5, 20), comb, 'comb 12289'), small(140, 3), ((150, 40), solid, 'solid 12289'), ]),
            _image((150, 215), 22, [small(0, 0), ((12, 14), comb, 'comb 12289'), small(141, 100)])]


def post_launches():
    """Every launch of the GPU test: ``name``, ``images`` (``g``, ``gs``, ``objects``, ``bg``) and ``settings`` = (exterior_scale,
    exterior_offset, contrast_epsilon, mask_max_distance, mask_stdamp); ``exact``: ties of the intensity band are exact by construction
    (the guard-band condition does not apply)."""
    L = []
    add = lambda name, images, settings=POST_DEFAULT, exact=False: L.append(dict(name=name, images=images, settings=settings, exact=exact))
    add('geometry', [_image((37, 53), 1, _geometry_objects())], (2.5, 2, 1e-4, 2, 1.5))
    add('whole image', [_image((37, 53), 2, [((0, 0), _rect(37, 53), 'whole')])])
    add('1x1', [_image((1, 1), 3, [((0, 0), _rect(1, 1), 'whole')])])
    add('1x300', [_image((1, 300), 4, [((0, 0), _rect(1, 1), 'pixel'), ((0, 50), _rect(1, 20), '1xN'), ((0, 295), _rect(1, 5), 'end')])], (5, 2, 1e-4, 3, 2))
    add('300x1', [_image((300, 1), 5, [((0, 0), _rect(4, 1), 'end'), ((100, 0), _rect(30, 1), 'Nx1'), ((299, 0), _rect(1, 1), 'pixel')])], (2.5, 0.5, 1e-4, 5, 1.5))
    add('520x696', [_image((520, 696), 6, [((0, 0), _ellipse(80, 80)[40:, 40:], 'corner'), ((480, 656), _ellipse(80, 80)[:40, :40], 'corner'),
                                           ((200, 300), _ellipse(60, 80), ''), ((0, 400), _ellipse(30, 50), 'top'), ((250, 676), _rect(30, 20), 'right')])], (2.5, 5, 1e-4, 16, 2))
    for settings in POST_PARAMETER_SETS:
        add(f'parameters {settings}', [_image((120, 150), 7, _param_objects())], settings)
    add('combs', [_image((160, 230), 8, [((15, 15), post_comb(64, 191, 1), 'comb 12288')]), _image((160, 230), 9, [((15, 15), post_comb(64, 191, 2), 'comb 12289')])], (2.5, 2, 1e-4, 1, 2))
    solid = np.zeros((97, 128), bool)
    solid[:96] = True
    plus = solid.copy()
    plus[96, 5] = True
    add('areas', [_image((140, 170), 10, [((20, 20), solid[:96], 'area 12288')]), _image((140, 170), 11, [((20, 20), plus, 'area 12289')])], (2.5, 2, 1e-4, 2, 2))
    add('pooled', post_pooled_images(), (2.5, 2, 1e-4, 1, 2))
    # degenerate inputs
    add('no background', [_image((40, 50), 12, [((12, 15), _ellipse(14, 18), '')], bg=np.zeros((40, 50), bool))])
    flat = _image((40, 50), 13, [((12, 15), _ellipse(14, 18), '')])
    flat['g'] = np.full((40, 50), 0.5)
    add('constant g', [flat])
    dy = _image((40, 50), 14, [((10, 10), _rect(11, 11), 'plateau')])
    dy['gs'] = np.full((40, 50), 0.25)
    dy['gs'][:, 21:] = 0.5
    dy['gs'][:10] = 0.125
    add('dyadic plateaus', [dy], (5, 5, 1e-4, 2, 2), exact=True)
    for c in POST_CONSTANTS:
        add(f'fields + {c:g}', post_field_images(c))
    return L


POST_FIELD_SEEDS = (31, 32, 33)


def post_field_images(constant):
    """Three images of blobs of 50 .. 700 pixels, intensities with ``constant`` added to ``g`` and to ``g_mask_processing``."""
    specs = [((90, 120), [((5, 8), _ellipse(28, 30), ''), ((50, 60), _ellipse(22, 36), ''), ((0, 90), _ellipse(16, 25), 'corner'), ((60, 0), _ellipse(25, 12), 'left'), ((40, 20), _ellipse(8, 9), '')]),
             ((64, 64), [((10, 10), _ellipse(20, 20), ''), ((40, 30), _ellipse(18, 30), ''), ((2, 45), _rect(9, 7), '')]),
             ((37, 53), [((0, 0), _ellipse(14, 14), 'corner'), ((15, 20), _ellipse(15, 25), ''), ((30, 45), _rect(7, 8), 'corner')])]
    return [_image(shape, seed, objs, constant) for seed, (shape, objs) in zip(POST_FIELD_SEEDS, specs)]


def post_stage_images():
    """Four images for ``Postprocessing.process_many`` (raw intensities only: the stage filters them itself) and the ``postprocess``
    settings of each; the first and third differ from the others in ``exterior_scale``."""
    images = [_image((60, 80), 41, [((5, 8), _ellipse(20, 24), ''), ((30, 40), _ellipse(18, 30), ''), ((0, 60), _ellipse(12, 20), 'corner')]),
              _image((64, 64), 42, [((10, 10), _ellipse(20, 20), ''), ((40, 30), _ellipse(18, 30), '')]),
              _image((37, 53), 43, [((0, 0), _ellipse(14, 14), 'corner'), ((15, 20), _ellipse(15, 25), '')]),
              _image((50, 45), 44, [((20, 10), _ellipse(16, 16), ''), ((2, 25), _rect(9, 12), ''), ((38, 30), _ellipse(10, 14), '')])]
    for im in images:                                      # some objects brighter than others, so that the contrast decides something
        for k, o in enumerate(im['objects']):
            h, w = o.fg_fragment.shape
            im['g'][o.fg_offset[0]:o.fg_offset[0] + h, o.fg_offset[1]:o.fg_offset[1] + w][o.fg_fragment] += (0.0, 0.6, 0.15)[k % 3]
    settings = [dict(exterior_scale=2.5, min_contrast=1.2), dict(min_contrast=1.2), dict(exterior_scale=2.5, min_contrast=1.2), dict(min_contrast=1.2)]
    return images, settings


def post_stage_nan_image():
    """One image for the stage whose only object leaves a rim of 3 pixels: the erosion of the complement by the disk of
    ``exterior_offset`` = 5 is empty, so no pixel may enter the background estimate, the exterior mean is 0 / 0 and the contrast NaN
    (``NaN < min_contrast`` is False: the reference keeps the object, postprocess.py:198).  Returns the image and its settings."""
    return _image((30, 40), 45, [((3, 3), _rect(24, 34), 'no background')]), dict(min_contrast=1.2)


def post_reference(g, gs, bg, off, frag, exterior_scale, exterior_offset, contrast_epsilon, max_distance, stdamp):
    """The sums of the contrast response and of the intensity band (superdsm/postprocess.py:254-266, 316-337, full-image formulation)
    in np.longdouble (x86: 64-bit mantissa, eps = 1.08e-19; the callers assert eps < 1e-18).  Which pixels enter the exterior sum is
    decided in float64, as the reference decides it.  Returns the four fields, the contrast, the counts ``n_in`` / ``n_ext`` of the
    pixels of the two sums, and ``margin`` / ``band``: the smallest distance of a pixel of the band's superset (dilation xor erosion) to
    either threshold, and 4 n eps (|mean| + amp), the uncertainty of a threshold evaluated in float64."""
    import scipy.ndimage as ndi
    from . import _morph
    X = np.longdouble
    mask = np.zeros(g.shape, bool)
    mask[off[0]:off[0] + frag.shape[0], off[1]:off[1] + frag.shape[1]] = frag
    n_in = int(mask.sum())
    out = dict(n_in=n_in, n_ext=0, margin=np.inf, band=0.0)
    if n_in == 0:
        return out
    with np.errstate(all='ignore'):
        gl = g.astype(X)
        gn = gl / np.sqrt(((gl - gl.mean()) ** 2).mean())
        out['interior_mean'] = gn[mask].sum() / n_in
        d = ndi.distance_transform_edt(~mask) if not mask.all() else np.zeros(g.shape)
        ext = ((d - exterior_offset).clip(0, np.inf) / exterior_scale <= 5) & ~mask & np.asarray(bg, bool)
        d2 = np.rint(d[ext] ** 2).astype(X)                                  # the squared distances are integers
        wgt = np.exp(-(np.sqrt(d2) - X(exterior_offset)).clip(0, np.inf) / X(exterior_scale))
        out['n_ext'] = int(ext.sum())
        out['exterior_mean'] = (wgt * gn[ext]).sum() / wgt.sum()
        out['contrast'] = (out['interior_mean'] + X(contrast_epsilon)) / (out['exterior_mean'] + X(contrast_epsilon))
        data = gs[mask].astype(X)
        mean = data.sum() / n_in
        std = np.sqrt(((data - mean) ** 2).sum() / n_in)
        out['fg_mean'], out['fg_std'] = mean, std
        if max_distance > 0 and stdamp > 0:
            se = _morph.disk(max_distance)
            sup = np.logical_xor(_morph.binary_dilation(mask, se), _morph.binary_erosion(mask, se))
            v = gs[sup].astype(X)
            amp = std * X(stdamp)
            out['margin'] = float(min(np.abs(v - (mean - amp)).min(), np.abs(v - (mean + amp)).min())) if v.size else np.inf
            out['band'] = float(4 * (n_in if n_in > 1 else 0) * _EPS * (abs(mean) + amp))     # one pixel: its mean is the pixel, exactly
    return out


# ---------------------------------------------------------------------------------------------------------
# the mask tail of a candidate's solve (tests/test_mask_tail_cpu.py and tests/test_mask_tail_gpu.py): what the foreground bits, the
# fragment box, ``on_boundary`` and the two counts of a record should BE at given parameters.  NumPy and the CPU oracle's region and G~.
# ---------------------------------------------------------------------------------------------------------
TAIL_BAND = 2.0 ** -40


def tail_reference(y, y_mask, atoms, footprint, cfg, theta, xi=None):
    """The result of a candidate at the parameters (theta, xi), pixel by pixel (superdsm/objects.py:198-209, dsm.py:86-94 and 113-128 with
    ``roi.offset = 0``, image.get_pixel_map): at region pixel (r, c) of the H x W image, u = r / max(H - 1, 1), v = c / max(W - 1, 1),

        S = a1 u^2 + a2 v^2 + 2 a3 u v + 2 b1 u + 2 b2 v + c + (G~ xi)[pixel],

    every operation in np.longdouble (x86: 64-bit significand); the pixel is foreground iff S > 0.  The region is the oracle's
    (``oracle.region_mask``), G~ the oracle's CSR matrix (``oracle.smooth_matrix``: float32-exact weights, which the setup tests pin bit for
    bit against the setup kernel).  ``xi`` None or all zero: the polynomial alone (no G~ is built).

    Guard band.  With A = the sum of the absolute values of the six polynomial terms and of every |w xi| product of the pixel, a pixel is
    DECIDED when |S| > 2^-40 A.  The solve kernel evaluates the surface in a candidate-local basis (centre and half extents of the region
    box) and the record's theta is that basis converted back; both evaluations are float64 sums of at most 6 + nnz terms (nnz: entries of
    the pixel's row of G~, a few hundred at the most), each term bounded by the corresponding full-image one, so the kernel's S differs
    from the exact S at the RECORDED parameters by a few hundred * 2^-53 * A.  2^-40 is about 8000 * 2^-53: a wide margin over that, and
    still so narrow that on real scenes no pixel falls inside it (tests/test_mask_tail_cpu.py counts them).  The band follows from the number
    format and the term count alone; it is not fitted to what the kernel returns.

    ``on_boundary`` is the same rule for the polynomial alone (G~ has no rows off the region) on the 2 (W + 2) + 2 (H + 2) positions of the
    one-pixel ring around the image, r in {-1, H} x c in -1 .. W and c in {-1, W} x r in -1 .. H, corners included: 1 if a ring pixel is
    decided positive, 0 if all are decided non-positive, None (undecided) otherwise.

    Returns a dict: ``box`` (r0, c0, h, w) the region's bounding box (None for an empty region); over that box ``region``, ``expected``
    (S > 0), ``decided`` (bool arrays; ``decided`` is False off the region) and ``ratio`` (|S| / A, inf off the region and where A = 0);
    ``fg_box`` (r0, c0, h, w) of the expected bits, None if there is none; ``on_boundary`` and ``ring_ratio`` (smallest |S| / A on the ring);
    ``n_pixels``, ``n_positive`` (region pixels with y > 0) and ``n_negative`` (y < 0; zeros of either sign count in neither)."""
    from oracle import oracle                              # test infrastructure, as this function is
    X = np.longdouble
    assert np.finfo(X).eps < 1e-18, 'np.longdouble must be wider than float64'
    y = np.asarray(y, np.float64)
    H, W = y.shape
    band = X(TAIL_BAND)
    th = [X(float(t)) for t in np.asarray(theta, np.float64).ravel()]
    assert len(th) == 6
    a1, a2, a3, b1, b2, c0 = th
    zu, zv = X(max(H - 1, 1)), X(max(W - 1, 1))

    def poly(r, c):
        u, v = np.asarray(r).astype(X) / zu, np.asarray(c).astype(X) / zv
        terms = (a1 * u * u, a2 * v * v, X(2) * a3 * u * v, X(2) * b1 * u, X(2) * b2 * v, c0 + X(0) * u)
        S, A = terms[0], np.abs(terms[0])
        for t in terms[1:]:
            S, A = S + t, A + np.abs(t)
        return S, A

    region = oracle.region_mask(y, y_mask, atoms, footprint, cfg.get('background_margin', 20))
    rr, cc = np.nonzero(region)                            # raster order: the order of the rows of G~
    yr = y[region]
    out = dict(n_pixels=int(region.sum()), n_positive=int((yr > 0).sum()), n_negative=int((yr < 0).sum()), box=None, fg_box=None)
    # the ring of the image
    ring_r = np.concatenate([np.full(W + 2, -1), np.full(W + 2, H), np.arange(-1, H + 1), np.arange(-1, H + 1)])
    ring_c = np.concatenate([np.arange(-1, W + 1), np.arange(-1, W + 1), np.full(H + 2, -1), np.full(H + 2, W)])
    Sr, Ar = poly(ring_r, ring_c)
    dec = np.abs(Sr) > band * Ar
    out['on_boundary'] = 1 if (dec & (Sr > 0)).any() else (0 if dec.all() else None)
    with np.errstate(divide='ignore', invalid='ignore'):
        out['ring_ratio'] = float(np.where(Ar > 0, np.abs(Sr) / Ar, np.inf).min())
    if out['n_pixels'] == 0:
        return out
    S, A = poly(rr, cc)
    xi = None if xi is None else np.asarray(xi, np.float64).ravel()
    if xi is not None and xi.size and np.any(xi != 0):
        sm = oracle.smooth_matrix(region, cfg.get('smooth_amount', 10), cfg.get('gaussian_shape_multiplier', 2), cfg.get('smooth_subsample', 20))
        assert sm.N == out['n_pixels'] and sm.M == xi.size, (sm.N, sm.M, out['n_pixels'], xi.size)
        prod = sm.data.astype(X) * xi[sm.indices].astype(X)
        row = np.repeat(np.arange(sm.N), np.diff(sm.indptr))
        gs, ga = np.zeros(sm.N, X), np.zeros(sm.N, X)
        np.add.at(gs, row, prod)
        np.add.at(ga, row, np.abs(prod))
        S, A = S + gs, A + ga
    r0, c0b = int(rr.min()), int(cc.min())
    h, w = int(rr.max()) - r0 + 1, int(cc.max()) - c0b + 1
    out['box'] = (r0, c0b, h, w)
    crop = lambda a: a[r0:r0 + h, c0b:c0b + w]
    out['region'] = crop(region).copy()
    expected, decided, ratio = np.zeros((H, W), bool), np.zeros((H, W), bool), np.full((H, W), np.inf)
    expected[rr, cc] = S > 0
    decided[rr, cc] = np.abs(S) > band * A
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio[rr, cc] = np.where(A > 0, np.abs(S) / A, np.inf).astype(np.float64)
    out['expected'], out['decided'], out['ratio'] = crop(expected).copy(), crop(decided).copy(), crop(ratio).copy()
    if expected.any():
        fr, fc = np.flatnonzero(expected.any(axis=1)), np.flatnonzero(expected.any(axis=0))
        out['fg_box'] = (int(fr[0]), int(fc[0]), int(fr[-1] - fr[0] + 1), int(fc[-1] - fc[0] + 1))
    return out


def tail_paste(box, a, shape, fill=False):
    """A box-sized array of :func:`tail_reference` (or of a mask box of a plan) in a full image of ``shape``."""
    out = np.full(shape, fill, np.asarray(a).dtype)
    if box is not None:
        out[box[0]:box[0] + box[2], box[1]:box[1] + box[3]] = a
    return out


def _toy_cfg(**kw):
    return dict(dict(scale=1000, epsilon=1.0, alpha=0.033, smooth_amount=4, smooth_subsample=8, gaussian_shape_multiplier=2,
                     background_margin=8, init='elliptical'), **kw)


def edge_case_scene():
    """96 x 120: a nucleus with a hole of ``y_mask`` inside, a nucleus cut by the image border, a single positive pixel (a trivial
    candidate) and a union of two atoms."""
    rng = np.random.default_rng(5)
    H, W = 96, 120
    rr, cc = np.mgrid[:H, :W]
    y = -0.2 + 0.02 * rng.standard_normal((H, W))
    y = np.minimum(y, -0.01)
    y[((rr - 30) / 11.0) ** 2 + ((cc - 40) / 15.0) ** 2 <= 1] = 0.35          # a nucleus
    y[((rr - 70) / 9.0) ** 2 + ((cc - 4) / 12.0) ** 2 <= 1] = 0.3             # a nucleus cut by the image border
    y[60, 90] = 0.4                                                           # a single positive pixel (noise)
    atoms = np.ones((H, W), np.int32)
    atoms[:, 70:] = 2
    atoms[50:, :35] = 3
    y_mask = np.ones((H, W), bool)
    y_mask[25:35, 38:41] = False                                              # a hole in the mask inside the nucleus
    return dict(name='edge cases', y=y, y_mask=y_mask, atoms=atoms, cfg=_toy_cfg(), footprints=[[1], [2], [3], [1, 3]])


def dense_grid_scene():
    """110 x 120, one candidate, smooth_subsample 3: rows of G~ of ~100 entries and a Hessian envelope beyond the LDS classes."""
    rng = np.random.default_rng(11)
    H, W = 110, 120
    rr, cc = np.mgrid[:H, :W]
    y = -0.15 + 0.03 * rng.standard_normal((H, W))
    blob = ((rr - 55) / 30.0) ** 2 + ((cc - 60) / 36.0) ** 2
    y += 0.5 * np.exp(-1.5 * blob)
    y += 0.25 * np.exp(-(((rr - 40) / 9.0) ** 2 + ((cc - 85) / 7.0) ** 2))       # a bump the ellipse cannot follow
    atoms = np.ones((H, W), np.int32)
    return dict(name='dense grid', y=y, y_mask=None, atoms=atoms, cfg=_toy_cfg(alpha=0.05, smooth_subsample=3, background_margin=6), footprints=[[1]])


def beyond_setup_tables_scene():
    """150 x 170, smooth_subsample 2 on a 17 k-pixel region: more grid points (~4300) than the setup kernel's tables hold, beside an
    ordinary candidate."""
    rng = np.random.default_rng(8)
    H, W = 150, 170
    rr, cc = np.mgrid[:H, :W]
    y = -0.1 + 0.02 * rng.standard_normal((H, W))
    y += 0.4 * np.exp(-(((rr - 75) / 50.0) ** 2 + ((cc - 85) / 58.0) ** 2) ** 2)
    atoms = np.ones((H, W), np.int32)
    atoms[:, 100:] = 2
    atoms[55:95, 70:100] = 3                                # a piece of the blob's flank: an ordinary candidate beside the oversized one
    return dict(name='beyond the setup tables', y=y, y_mask=None, atoms=atoms,
                cfg=_toy_cfg(alpha=0.05, smooth_amount=2, smooth_subsample=2, background_margin=12), footprints=[[1, 2, 3], [3]])


def two_blob_scene(seed=3, H=96, W=128):
    """Two noisy blobs, one atom each: ``(y, atoms)``."""
    rng = np.random.default_rng(seed)
    rr, cc = np.mgrid[:H, :W]
    y = -0.2 + 0.03 * rng.standard_normal((H, W))
    y += 0.55 * np.exp(-(((rr - 46) / 17.0) ** 2 + ((cc - 40) / 21.0) ** 2) ** 1.5)
    y += 0.5 * np.exp(-(((rr - 50) / 15.0) ** 2 + ((cc - 88) / 18.0) ** 2) ** 1.5)
    atoms = np.ones((H, W), np.int32)
    atoms[:, 64:] = 2
    return y, atoms


def straddling_rows_scene():
    """40 x 100, one candidate whose region box is 77 columns wide (> 64, and 77 mod 32 = 13 is coprime with 32: every row of the box
    begins at another bit of a mask word); exact zeros and -0.0 among the region's intensities."""
    rng = np.random.default_rng(21)
    H, W = 40, 100
    rr, cc = np.mgrid[:H, :W]
    y = -0.2 + 0.02 * rng.standard_normal((H, W))
    y += 0.6 * np.exp(-(((rr - 19) / 11.0) ** 2 + ((cc - 46) / 30.0) ** 2) ** 1.5)
    y += 0.2 * np.exp(-(((rr - 12) / 4.0) ** 2 + ((cc - 70) / 5.0) ** 2))
    y[8, 20:25] = 0.0
    y[30, 40:44] = -0.0
    y[19, 10] = 0.0
    atoms = np.full((H, W), 2, np.int32)
    atoms[:, 7:84] = 1
    return dict(name='straddling rows', y=y, y_mask=None, atoms=atoms, cfg=_toy_cfg(smooth_subsample=6, background_margin=40), footprints=[[1]])


TAIL_CRAFTED_SHAPES = ((24, 37), (37, 24))


def tail_crafted_image(shape):
    """An image of one atom whose region is the whole image (positive pixels everywhere within the margin) and the hyper-parameters of
    the crafted cases: ``alpha = inf`` makes every deformable solve fail, so that a candidate with a callable ``dsm/init`` returns its
    initialisation (status FALLBACK) and the mask tail runs at parameters of the caller's choice; M > 0."""
    rng = np.random.default_rng(100 + shape[0])
    y = np.where(rng.random(shape) < 0.4, 0.3, -0.2) + 0.01 * rng.standard_normal(shape)
    return dict(y=y, y_mask=None, atoms=np.ones(shape, np.int32), footprint=[1],
                cfg=_toy_cfg(alpha=np.inf, smooth_amount=2, smooth_subsample=4, background_margin=40))


def _pixel_theta(shape, rr=0.0, cc=0.0, r=0.0, c=0.0, k=0.0):
    """theta of S = rr row^2 + cc col^2 + r row + c col + k, in PIXEL coordinates (small dyadic numbers: S is exact in them)."""
    zu, zv = float(max(shape[0] - 1, 1)), float(max(shape[1] - 1, 1))
    return np.array([rr * zu * zu, cc * zv * zv, 0.0, r * zu / 2, c * zv / 2, k])


def tail_crafted_cases(shape, M):
    """``name -> dict(params = theta (6) + xi (M), mask = 'empty' | 'full' | 'reference', on_boundary = 0 | 1)`` for an image of
    :func:`tail_crafted_image`; what ``mask`` and ``on_boundary`` say is written out by hand here, the reference must agree.

    * a plane positive at ONE ring corner only (0.5 there, -0.5 at its two ring neighbours, falling from there);
    * a plane positive on ONE ring line only (0.5 there, -0.5 on the adjacent line of the image);
    * a concave paraboloid, negative on every ring pixel (its zero ellipse has the half axes (H - 1) / 2 + 0.5 and (W - 1) / 2 + 0.5), which
      alone is negative at the image's corners too -- no quadric is positive on the whole rectangle and negative on the whole ring: the
      ellipse through ring-edge midpoints cannot hold the rectangle's corners --, lifted above zero on every pixel by a constant xi (G~
      has rows on the region only, so the ring does not see it);
    * a constant -0.25 and xi alternating in sign with an amplitude that flips the surface: an intricate mask."""
    H, W = shape
    alt = (-1.0) ** np.arange(M)
    small = alt * 2.0 ** -6                                  # takes every plane through the G~ path without changing a sign (rows of G~ sum to <= 1)
    C = {}
    for rname, sr, kr in (('top', 1.0, 1.0), ('bottom', -1.0, float(H))):            # distance of a row from the ring row: sr * row + kr
        for cname, sc, kc in (('left', 1.0, 1.0), ('right', -1.0, float(W))):
            C[f'corner {rname} {cname}'] = dict(params=np.concatenate([_pixel_theta(shape, r=-sr, c=-sc, k=0.5 - kr - kc), small]), mask='empty', on_boundary=1)
    C['row -1'] = dict(params=np.concatenate([_pixel_theta(shape, r=-1.0, k=-0.5), small]), mask='empty', on_boundary=1)
    C['row H'] = dict(params=np.concatenate([_pixel_theta(shape, r=1.0, k=0.5 - H), small]), mask='empty', on_boundary=1)
    C['column -1'] = dict(params=np.concatenate([_pixel_theta(shape, c=-1.0, k=-0.5), small]), mask='empty', on_boundary=1)
    C['column W'] = dict(params=np.concatenate([_pixel_theta(shape, c=1.0, k=0.5 - W), small]), mask='empty', on_boundary=1)
    # 1 - ((row - (H-1)/2) / (H/2))^2 - ((col - (W-1)/2) / (W/2))^2, times (H W / 4)^2 / 2^14: dyadic coefficients, values within +-4
    ar, ac, mr, mc = W * W / 4.0, H * H / 4.0, (H - 1) / 2.0, (W - 1) / 2.0
    bowl = 2.0 ** -14 * np.array([-ar, -ac, 2 * ar * mr, 2 * ac * mc, (H * W / 4.0) ** 2 - ar * mr * mr - ac * mc * mc])
    C['paraboloid'] = dict(params=np.concatenate([_pixel_theta(shape, *bowl), np.full(M, 64.0)]), mask='full', on_boundary=0)
    flips = (-1.0) ** (np.arange(M) + np.arange(M) // 7)     # (7 divides neither grid width, 10 and 6: no plain stripes)
    C['alternating'] = dict(params=np.concatenate([_pixel_theta(shape, k=-0.25), 64.0 * flips]), mask='reference', on_boundary=0)
    return C


def tail_two_image_cases(M_of):
    """Candidates of a plan over the two crafted images, ``[(image index, name, params, on_boundary)]``: every surface is positive on
    the ring of its own image (or, for the controls, nowhere on it) and non-positive where the ring of the OTHER image would lie -- the
    controls are positive only there.  ``M_of``: the number of columns of G~ of the two images' candidates."""
    (Ha, Wa), (Hb, Wb) = TAIL_CRAFTED_SHAPES
    z = lambda i: np.zeros(M_of[i])
    th = lambda i, **kw: np.concatenate([_pixel_theta(TAIL_CRAFTED_SHAPES[i], **kw), z(i)])
    return [(0, 'column W of the wide image', th(0, c=1.0, k=0.5 - Wa), 1),
            (1, 'row H of the tall image', th(1, r=1.0, k=0.5 - Hb), 1),
            (0, 'corner (-1, W) of the wide image', th(0, r=-1.0, c=1.0, k=-0.5 - Wa), 1),
            (1, 'corner (H, -1) of the tall image', th(1, r=1.0, c=-1.0, k=-0.5 - Hb), 1),
            (0, 'control: row H of the tall image, on the wide one', th(0, r=1.0, k=0.5 - Hb), 0),
            (1, 'control: column W of the wide image, on the tall one', th(1, c=1.0, k=0.5 - Wa), 0)]


# ---------------------------------------------------------------------------------------------------------
# the cases of the exact post-processing steps (tests/test_post_steps_gpu.py and tests/test_post_steps_cpu.py): hole filling, the
# background mask, the glare test.  NumPy only; the CPU file checks what the cases claim about themselves.
# ---------------------------------------------------------------------------------------------------------
FILL_WIDTHS = (31, 32, 33, 64, 65)
FILL_LDS_WORDS = 4096            # POST_FLOOD_WORDS of sdsm_post.hip: h * ceil(w / 32) beyond it floods in global memory


def fill_ring(h=9, w=9, wall=2):
    a = _rect(h, w)
    a[wall:h - wall, wall:w - wall] = False
    return a


def fill_spiral(n=63):
    """Walls with a background corridor of one pixel that winds from the border pixel (1, 0) to the centre: ONE background component,
    whose pixels are up to n^2 / 2 steps from the border."""
    a = _rect(n, n)
    r, c, dr, dc = 1, 0, 0, 1
    a[r, c] = False
    while True:
        moved = False
        while 0 < r + dr < n - 1 and 0 < c + dc < n - 1 and a[r + 2 * dr, c + 2 * dc] if (0 <= r + 2 * dr < n and 0 <= c + 2 * dc < n) else False:
            r, c = r + dr, c + dc
            a[r, c] = False
            moved = True
        if not moved:
            break
        dr, dc = dc, -dr
    return a


def fill_cases():
    """``name -> window`` of the hole-filling test."""
    rng = np.random.default_rng(77)
    C = {'1x1 set': _rect(1, 1), '1x1 clear': ~_rect(1, 1), '1x40': rng.random((1, 40)) < 0.5, '40x1': rng.random((40, 1)) < 0.5}
    for w in FILL_WIDTHS:                                   # rows straddle words (odd heights), the last word is partial
        a = rng.random((7 + 2 * (w % 3), w)) < 0.62
        a[0, 0] = a[-1, -1] = True
        C[f'random {a.shape[0]}x{w}'] = a
        b = _rect(9, w)
        b[2:7, 2:w - 2] = False
        b[4, 4:w - 4] = True
        C[f'frame {w}'] = b
    C['ring'] = fill_ring()
    opened = fill_ring()
    opened[4, 7:] = False
    C['ring open to the border'] = opened
    diag = np.zeros((9, 9), bool)                           # the wall's only gap is diagonal: closed for a 4-connected background
    diag[1:8, 1:8] = fill_ring(7, 7, 1)
    diag[1, 1] = False
    C['ring with a diagonal gap'] = diag
    nested = fill_ring(21, 37, 2)
    nested[6:15, 8:29] = fill_ring(9, 21, 2)
    C['nested rings'] = np.pad(nested, 1)
    C['checkerboard'] = (np.add.outer(np.arange(33), np.arange(35)) % 2).astype(bool)
    C['all ones'] = _rect(13, 70)
    C['all zeros'] = ~_rect(13, 70)
    C['spiral 63'] = fill_spiral(63)
    comb = post_comb(16, 66)
    comb[-1, :] = True                                      # a frame around the teeth would close them: the gaps stay open to the right
    C['comb'] = comb
    closed = np.pad(post_comb(16, 66), 1, constant_values=True)
    C['comb in a frame'] = closed
    big = rng.random((2049, 33)) < 0.7                     # 2049 * 2 words: just above the LDS cut-over
    big[0], big[-1], big[:, 0], big[:, -1] = True, True, True, True
    C['above the cut-over'] = big
    edge = rng.random((2048, 33)) < 0.7                    # 4096 words: the last window flooded in LDS
    C['at the cut-over'] = edge
    return C


def fill_embedded(frag, pads):
    """``frag`` in a larger clear window, ``pads`` = (top, bottom, left, right)."""
    return np.pad(np.asarray(frag, bool), ((pads[0], pads[1]), (pads[2], pads[3])))


FILL_PADS = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 3, 0, 0), (0, 0, 2, 0), (0, 0, 0, 1), (1, 1, 1, 1), (3, 0, 5, 31), (2, 7, 32, 1))


def bg_cases():
    """``name -> (shape, [(offset, fragment), ...])`` of the background-mask test (every case runs at every radius)."""
    rng = np.random.default_rng(78)
    H, W = 45, 83                                           # a width that is no multiple of 64
    corners = [((0, 0), _rect(3, 4)), ((0, W - 5), _rect(6, 5)), ((H - 4, 0), _rect(4, 2)), ((H - 3, W - 3), _rect(3, 3))]
    edges = [((0, 30), _ellipse(5, 9)), ((H - 6, 40), _ellipse(6, 7)), ((20, 0), _ellipse(9, 4)), ((15, W - 3), _rect(8, 3))]
    overlap = [((10, 10), _ellipse(14, 18)), ((15, 20), _rect(12, 12)), ((12, 14), rng.random((10, 20)) < 0.5), ((30, 60), _ellipse(9, 9))]
    return {
        'no objects': ((37, 53), []),
        '1x1': ((1, 1), []),
        '1x1 covered': ((1, 1), [((0, 0), _rect(1, 1))]),
        'corners': ((H, W), corners),
        'edges': ((H, W), edges),
        'corners and edges': ((H, W), corners + edges),
        'overlapping': ((50, 90), overlap),                  # a later box overwrites an earlier one, also with clear bits
        'whole image': ((37, 53), [((0, 0), _rect(37, 53))]),
        'one pixel': ((70, 130), [((35, 64), _rect(1, 1))]),
        '1x200': ((1, 200), [((0, 60), _rect(1, 5)), ((0, 199), _rect(1, 1))]),
        '200x1': ((200, 1), [((100, 0), _rect(3, 1))]),
    }


BG_RADII = (0, 1, 5, 16, 32)
BG_SET = ('corners and edges', 'no objects', 'overlapping')       # three images of different shapes, the one in the middle empty


def _peaks(shape, centres, sigma, heights=None):
    rr, cc = np.mgrid[:shape[0], :shape[1]]
    heights = heights or [1.0] * len(centres)
    return sum(hh * np.exp(-((rr - y) ** 2 + (cc - x) ** 2) / (2.0 * sigma * sigma)) for (y, x), hh in zip(centres, heights))


def glare_cases():
    """``name -> dict(g, offset, fragment, expect)`` of the glare test; ``expect``: what the case is built to give at min_layer 0.5
    with 5 layers (True / False / 'empty' for the ValueError of an empty eroded mask), checked against the oracle on the CPU."""
    C = {}
    shape, off = (60, 90), (7, 11)
    frag = _ellipse(41, 70)
    add = lambda name, g, expect, fragment=frag, offset=off: C.__setitem__(name, dict(g=np.ascontiguousarray(g, np.float64), offset=offset, fragment=fragment, expect=expect))
    add('one peak', _peaks(shape, [(27, 45)], 12), True)
    add('two peaks', _peaks(shape, [(27, 28), (27, 64)], 7), False)
    # the saddle between the peaks lies at 0.88 of the top: only the layer at 0.9 (of 0.5, 0.6, .. 0.9) separates them; the floor of 0 comes
    # from the rest of the mask
    add('two peaks, highest layer only', _peaks(shape, [(27, 38), (27, 53)], 6), False)
    g = np.zeros(shape)
    g[20:25, 30:35] = 1.0
    g[25:30, 35:40] = 1.0                                   # two plateaus that touch at a corner only
    add('diagonal contact', g, False)
    add('border on all sides', _peaks((30, 40), [(15, 20)], 6), True, _rect(30, 40), (0, 0))
    add('constant', np.full(shape, 0.25), True)
    g = _peaks(shape, [(27, 45)], 12)
    g[27, 45] = np.nan
    add('nan inside the mask', g, True)
    add('empty erosion', _peaks(shape, [(27, 45)], 12), 'empty', np.pad(_rect(4, 30), 1), (10, 10))
    wide = _rect(3, 40)
    wide[1, 5] = False
    add('thin', _peaks(shape, [(27, 45)], 12), 'empty', np.pad(wide, 2), (20, 20))
    return C


def glare_tie_search(limit=200000, seed=5):
    """A triple (max, min, prop) of doubles for which (max - min) * prop + min differs between two rounded operations and one fused
    multiply-add, found with exact rational arithmetic; returns (max, min, prop, twice_rounded, fused) or None."""
    from fractions import Fraction
    rng = np.random.default_rng(seed)
    for prop in np.linspace(0.5, 1, 5, endpoint=False)[1:]:
        for _ in range(limit // 4):
            mx, mn = float(rng.random()), float(rng.random()) * 0.5
            if mx <= mn:
                continue
            d = mx - mn
            if Fraction(mx) - Fraction(mn) != Fraction(d):
                continue                                    # keep the subtraction exact, so that only the multiply-add is in question
            twice = float(np.float64(d) * np.float64(prop) + np.float64(mn))
            exact = Fraction(d) * Fraction(float(prop)) + Fraction(mn)
            fused = _round_fraction(exact)
            if fused != twice:
                return mx, mn, float(prop), twice, fused
    return None


def _round_fraction(q):
    """The double nearest to the rational q (ties to even): float(Fraction) divides two integers, which Python rounds correctly."""
    return q.numerator / q.denominator


def glare_tie_case():
    """The tie case: a mask whose eroded pixels hold max, min and one pixel exactly AT the twice-rounded threshold of the layer ``prop``
    (so the pixel is not above it and the layer stays one component), which a fused threshold -- smaller here -- would put above it as a
    second component.  The test runs ONE layer at ``min_layer`` = prop (np.linspace starts at it exactly): at the lower layers the pixel
    is a second component either way.  Returns None when the search finds no triple whose fused threshold is the smaller one."""
    for seed in range(5, 40):
        t = glare_tie_search(seed=seed)
        if t is not None and t[4] < t[3]:
            break
    else:
        return None
    mx, mn, prop, twice, fused = t
    g = np.full((20, 40), mn)
    g[8:12, 8:12] = mx                                      # the top plateau: one component of every layer
    g[10, 30] = twice                                       # at the threshold of layer `prop`: above it only if the threshold is fused
    return dict(g=g, offset=(2, 2), fragment=_rect(16, 36), max=mx, min=mn, prop=prop, twice=twice, fused=fused, min_layer=prop, num_layers=1)


def post_steps_stage_images():
    """Five images for the stage-level test of the device steps and their ``postprocess`` settings: the first without hole filling and
    with the default (infinite) glare radius; the second with hole filling and a finite ``min_glare_radius``; the third shares the
    second's settings, so one launch refines and fills the windows of two images (offsets past the first image's); the last two share
    ``mask_stdamp = 0``: nothing is refined and the original fragments are filled.  Objects with holes, one glare-like object with two
    peaks, contrasts on both sides of ``min_contrast``."""
    ring = _ellipse(21, 25)
    ring[8:13, 9:16] = False
    a = _image((60, 80), 51, [((5, 8), ring, 'holes'), ((30, 40), _ellipse(18, 30), ''), ((0, 60), _ellipse(12, 20), 'corner')])
    two = _ellipse(23, 41)
    two[10:13, 18:23] = False
    b = _image((64, 72), 52, [((6, 6), _ellipse(20, 20), ''), ((34, 20), two, 'two peaks, hole'), ((3, 40), ring, 'holes')])
    dots = _ellipse(27, 33)
    dots[6:9, 10:13] = dots[15:20, 17:19] = False
    c = _image((50, 97), 53, [((20, 60), dots, 'two holes'), ((2, 3), _ellipse(15, 22), ''), ((25, 10), ring, 'holes'), ((0, 70), _rect(9, 27), 'edge')])
    d = _image((45, 66), 54, [((4, 30), dots, 'two holes'), ((20, 2), _ellipse(19, 23), '')])
    e = _image((70, 41), 55, [((1, 1), _ellipse(14, 14), ''), ((40, 8), ring, 'holes'), ((18, 5), dots, 'two holes')])
    for im in (a, b, c, d, e):
        for k, o in enumerate(im['objects']):
            h, w = o.fg_fragment.shape
            im['g'][o.fg_offset[0]:o.fg_offset[0] + h, o.fg_offset[1]:o.fg_offset[1] + w][o.fg_fragment] += (0.6, 0.0, 0.3)[k % 3]
    b['g'] += 0.8 * _peaks((64, 72), [(45, 28), (45, 52)], 4)      # object 1 of the second image: two bright spots
    shared, unrefined = dict(min_contrast=1.2, min_glare_radius=6.0, exterior_offset=3), dict(min_contrast=1.2, mask_stdamp=0)
    return [a, b, c, d, e], [dict(exterior_scale=2.5, min_contrast=1.2, fill_holes=False), shared, dict(shared), unrefined, dict(unrefined)]


# ---------------------------------------------------------------------------------------------------------
# the loss arithmetic of the solve kernels (tests/test_loss_arithmetic_cpu.py and tests/test_loss_arithmetic_gpu.py): the inputs of the
# element-by-element probe (sdsm_probe_loss_arithmetic) and what the scalar functions should return, in np.longdouble (x86: 64-bit
# significand, expl / log1pl; the CPU file checks these references against mpmath).  NumPy only.
# ---------------------------------------------------------------------------------------------------------
LOSS_GUARD = 750.0               # the exp guard of softplus_neg / loss_terms (sdsm_solve.hip)
LOSS_PROBE_MAX = 1 << 20         # SDSM_PROBE_LOSS_MAX of include/sdsm.h
_LN2L = np.log(np.longdouble(2))


def longdouble_is_extended():
    """np.longdouble has at least the 64-bit significand of x87 extended precision (what the references below need)."""
    return np.finfo(np.longdouble).nmant >= 63


def ulp_neighbours(v, k=4):
    """Every double within ``k`` units in the last place of each element of ``v`` (2 k + 1 values per element, v itself included)."""
    v = np.atleast_1d(np.asarray(v, np.float64))
    out = [v]
    lo, hi = v, v
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def loss_table_points():
    """The 65 table points u = j / 64 of log_w and the 64 bin edges (j + 1/2) / 64 between them (exact doubles)."""
    return np.arange(65) / 64.0, (np.arange(64) + 0.5) / 64.0


def loss_probe_inputs(seed=2024):
    """The (y, S) pairs and the values x of the probe, fewer than LOSS_PROBE_MAX of each: ``dict(y, S, x_unit, x_normal)``.
    t = y S is formed on the device; the cases with an exact target (table points, zeros, the guard) use y = 1 or a power of two.

    t:  -ln u for every table point and bin edge of log_w and its neighbours within 4 ulp -- of u, and of w = 1 + u, which decides the
    bin --, and the neighbours within 4 ulp of those t (the exponential moves them by about as many ulp of u: the returned u fall on
    the points and on both sides); +-0 and +-2^-1074;
    the t at which 1 + u starts to round to 1 (u = 2^-52, 2^-53, 2^-54), +-4 ulp; the odd multiples of ln 2 / 2 up to 750 (rint
    switches k), +-4 ulp; 708.4 .. 745.2 (ldexp makes subnormals); 750 and the first doubles on either side; beyond 750 up to 1e300;
    +-inf and NaN (also as 0 * inf); log-uniform and uniform samples; all of them with both signs.  y: 1 where t must be exact,
    else +-2^U(-20, 20) with S = t / y.
    x: uniform on [1, 2] with the end points and their neighbours (``x_unit``: the w = 1 + u of the passes); log-uniform over the
    normal range (``x_normal``)."""
    X = np.longdouble
    rng = np.random.default_rng(seed)
    pts, edges = loss_table_points()
    u = ulp_neighbours(np.concatenate([pts[1:], edges]), 4)               # (u = 0 is reached through the guard: t = 750)
    u = np.concatenate([u, ulp_neighbours(1.0 + np.concatenate([pts, edges]), 4) - 1.0])     # ... and the neighbours of w = 1 + u (an ulp of w is many of u)
    u = u[(u > 0) & (u <= 1)]
    t_tab = ulp_neighbours((-np.log(u.astype(X))).astype(np.float64), 4)
    t_one = ulp_neighbours((np.array([52, 53, 54]) * _LN2L).astype(np.float64), 4)
    m = np.arange(0, 1082)
    t_rint = ulp_neighbours(((2 * m + 1) * (_LN2L / 2)).astype(np.float64), 4)
    t_rint = t_rint[t_rint <= LOSS_GUARD]
    t_sub = np.concatenate([rng.uniform(708.4, 745.2, 20000), ulp_neighbours([708.4, 745.2, 1022 * float(_LN2L), 1074 * float(_LN2L), 1075 * float(_LN2L)], 4)])
    t_guard = np.array([LOSS_GUARD, np.nextafter(LOSS_GUARD, 0), np.nextafter(LOSS_GUARD, np.inf)])
    t_far = np.concatenate([10.0 ** rng.uniform(np.log10(LOSS_GUARD), 300, 2000), [751.0, 1e3, 1e300]])
    t_tiny = np.array([0.0, 2.0 ** -1074])
    exact = np.concatenate([t_tab, t_one, t_rint, t_sub, t_guard, t_far, t_tiny])
    exact = np.concatenate([exact, -exact])
    y_exact = np.ones(exact.size)
    y_exact[1::3] = 2.0 ** rng.integers(-20, 21, y_exact[1::3].size)       # powers of two: y S is still exact (S = t / y; 2^-1074 / y may round: t is what the device forms)
    y_exact[np.abs(exact) < 1e-300] = 1.0
    special = np.array([np.inf, -np.inf, np.nan, np.inf, -np.inf])
    y_special = np.array([1.0, 1.0, 1.0, 0.0, 2.0 ** -20])
    t_rand = np.concatenate([10.0 ** rng.uniform(-320, np.log10(LOSS_GUARD), 150000), rng.uniform(0, LOSS_GUARD, 150000), rng.uniform(0, 40, 150000), rng.uniform(0, 1, 100000)])
    t_rand = t_rand * rng.choice([-1.0, 1.0], t_rand.size)
    y_rand = 2.0 ** rng.uniform(-20, 20, t_rand.size) * rng.choice([-1.0, 1.0], t_rand.size)
    t = np.concatenate([exact, t_rand])
    y = np.concatenate([y_exact, y_rand])
    with np.errstate(all='ignore'):
        S = np.concatenate([t / y, special])
    y = np.concatenate([y, y_special])
    x_unit = np.concatenate([rng.uniform(1, 2, 300000), ulp_neighbours([1.0, 2.0, 1.5], 4)])
    x_unit = x_unit[(x_unit >= 1) & (x_unit <= 2)]
    x_normal = np.concatenate([2.0 ** rng.uniform(-1022, 1024, 300000), [2.0 ** -1022, np.finfo(np.float64).max, 1.0, 4.0]])
    x_normal = x_normal[np.isfinite(x_normal) & (x_normal >= 2.0 ** -1022)]
    assert max(y.size, x_unit.size + x_normal.size) <= LOSS_PROBE_MAX
    return dict(y=y, S=S, x_unit=x_unit, x_normal=x_normal)


def loss_reference(t, y=None):
    """What the scalar functions of the passes should return at the doubles ``t``, in np.longdouble: ``E`` = exp(-min(|t|, 750))
    (exp_neg's argument is clamped by its callers), ``softplus`` = log(1 + exp(-t)) = max(-t, 0) + log1p(exp(-|t|)), ``theta`` =
    1 / (1 + exp(t)) (as exp(-|t|) / (1 + exp(-|t|)) for t >= 0: no overflow) and ``kappa`` = theta (1 - theta) =
    exp(-|t|) / (1 + exp(-|t|))^2 -- none of these forms cancels.  With ``y``: also ``r`` = -y theta and ``dcurv`` = y^2 kappa.
    Non-finite t: NaN everywhere."""
    X = np.longdouble
    t = np.asarray(t, np.float64)
    with np.errstate(all='ignore'):
        tl = np.where(np.isfinite(t), t, np.nan).astype(X)
        a = np.abs(tl)
        E = np.exp(-a)
        out = dict(E=np.exp(-np.minimum(a, X(LOSS_GUARD))), softplus=np.maximum(-tl, X(0)) + np.log1p(E),
                   theta=np.where(tl >= 0, E / (1 + E), 1 / (1 + E)), kappa=E / ((1 + E) * (1 + E)))
        if y is not None:
            yl = np.asarray(y, np.float64).astype(X)
            out['r'], out['dcurv'] = -yl * out['theta'], yl * yl * out['kappa']
    return out


def log_reference(w):
    """log(w) of the doubles ``w`` in np.longdouble, as log1p(w - 1) (w - 1 is exact for 1 <= w <= 2)."""
    w = np.asarray(w, np.float64).astype(np.longdouble)
    return np.log1p(w - 1)


ENERGY_F = np.array([1.0, 1.0, 2.0, 2.0, 2.0, 1.0])     # q = (u^2, v^2, 2 u v, 2 u, 2 v, 1): |q_k| <= ENERGY_F[k] for |u|, |v| <= 1


def energy_reference(y, y_mask, atoms, fp, cfg, theta, xi=None, box=None):
    """psi, its full gradient (theta, then xi) and the 6 x 6 theta block of its Hessian at (theta, xi) in np.longdouble
    (superdsm/dsm.py:298-385: psi = sum_i phi(y_i S_i) + alpha sum_j (sqrt(xi_j^2 + epsilon) - sqrt(epsilon)), clamped at 0), with the
    surface of :func:`tail_reference` -- S = a1 u^2 + a2 v^2 + 2 a3 u v + 2 b1 u + 2 b2 v + c + (G~ xi), u = r / max(H - 1, 1), v =
    c / max(W - 1, 1), over the oracle's region and with the oracle's G~ -- and the loss terms of :func:`loss_reference`.
    ``smooth_amount = inf`` (or ``xi`` None): the elliptical model, M = 0.

    Beside ``psi``, ``grad`` and ``hess_theta`` the dict holds what a bound on a float64 evaluation needs:
    ``phi_sum``, ``reg_sum`` = alpha sum sqrt(xi^2 + epsilon) and ``reg0`` = alpha sqrt(epsilon) M; per pixel (raster order) ``y``,
    ``t``, ``theta_hat`` = 1 / (1 + e^t), ``kappa``, ``nnz`` (entries of the pixel's row of G~) and ``A``: the sum of the absolute values
    of the terms of S in the candidate's LOCAL frame, in which the solve kernels evaluate it (coordinates centred on ``box`` = (r0, c0,
    h, w) -- the candidate's box of the plan; default: the region's bounding box -- and scaled by its half extents, |u|, |v| <= 1;
    theta_local = R theta); ``R`` (6 x 6, theta_local = R @ theta; all
    entries >= 0), ``theta_local`` and ``theta_local_abs`` (the sums of the absolute values of the terms that form each local
    coefficient); ``abs_r`` = sum |y theta_hat|, ``abs_d`` = sum y^2 kappa: every term of a theta-gradient (theta-Hessian) entry in the
    local frame is at most ENERGY_F[k] |r_i| (ENERGY_F[k] ENERGY_F[l] d_i); ``smat`` = (indptr, indices, data) of G~ or None;
    ``yexp``: |y| < 2^yexp over the region; ``N``, ``M``."""
    from oracle import oracle                              # test infrastructure, as this function is
    X = np.longdouble
    assert longdouble_is_extended(), 'np.longdouble must be wider than float64'
    y = np.asarray(y, np.float64)
    Himg, Wimg = y.shape
    region = oracle.region_mask(y, y_mask, atoms, fp, cfg.get('background_margin', 20))
    rr, cc = np.nonzero(region)
    N = rr.size
    yl = y[region].astype(X)
    th = np.asarray(theta, np.float64).ravel().astype(X)
    assert th.size == 6 and N > 0
    deform = np.isfinite(cfg.get('smooth_amount', 10)) and xi is not None
    zu, zv = X(max(Himg - 1, 1)), X(max(Wimg - 1, 1))
    u, v = rr.astype(X) / zu, cc.astype(X) / zv
    q = np.stack([u * u, v * v, 2 * u * v, 2 * u, 2 * v, np.ones(N, X)])
    S = (th[:, None] * q).sum(axis=0)
    # the local frame (sdsm_solve.hip: load_run, reparam): u = O0 + P0 u_loc, v = O1 + P1 v_loc
    r0, c0, bh, bw = (int(rr.min()), int(cc.min()), int(rr.max() - rr.min() + 1), int(cc.max() - cc.min() + 1)) if box is None else [int(b) for b in box]
    assert r0 <= rr.min() and rr.max() < r0 + bh and c0 <= cc.min() and cc.max() < c0 + bw
    hr, hc = X(bh - 1) / 2, X(bw - 1) / 2
    P0, P1 = (hr if hr >= 1 else X(1)) / zu, (hc if hc >= 1 else X(1)) / zv
    O0, O1 = (r0 + hr) / zu, (c0 + hc) / zv
    R = np.zeros((6, 6), X)
    R[0, 0], R[3, 0], R[5, 0] = P0 * P0, P0 * O0, O0 * O0
    R[1, 1], R[4, 1], R[5, 1] = P1 * P1, P1 * O1, O1 * O1
    R[2, 2], R[3, 2], R[4, 2], R[5, 2] = P0 * P1, P0 * O1, P1 * O0, 2 * O0 * O1
    R[3, 3], R[5, 3] = P0, 2 * O0
    R[4, 4], R[5, 4] = P1, 2 * O1
    R[5, 5] = 1
    thl, thl_abs = R @ th, R @ np.abs(th)
    ul, vl = (u - O0) / P0, (v - O1) / P1
    ql = np.abs(np.stack([ul * ul, vl * vl, 2 * ul * vl, 2 * ul, 2 * vl, np.ones(N, X)]))
    A = (np.abs(thl)[:, None] * ql).sum(axis=0)
    out = dict(N=N, M=0, smat=None, R=R, theta_local=thl, theta_local_abs=thl_abs, nnz=np.zeros(N, np.int64))
    M = 0
    if deform:
        sm = oracle.smooth_matrix(region, cfg.get('smooth_amount', 10), cfg.get('gaussian_shape_multiplier', 2), cfg.get('smooth_subsample', 20))
        M = sm.M
        xil = np.asarray(xi, np.float64).ravel().astype(X)
        assert sm.N == N and xil.size == M, (sm.N, N, xil.size, M)
        row = np.repeat(np.arange(N), np.diff(sm.indptr))
        data = sm.data.astype(X)
        prod = data * xil[sm.indices]
        gs, ga = np.zeros(N, X), np.zeros(N, X)
        np.add.at(gs, row, prod)
        np.add.at(ga, row, np.abs(prod))
        S, A = S + gs, A + ga
        out.update(M=M, smat=(sm.indptr.copy(), sm.indices.copy(), sm.data.copy()), nnz=np.diff(sm.indptr))
    t = yl * S
    with np.errstate(all='ignore'):
        a = np.abs(t)
        E = np.exp(-a)
        phi = np.maximum(-t, X(0)) + np.log1p(E)
        theta_hat = np.where(t >= 0, E / (1 + E), 1 / (1 + E))
        kappa = E / ((1 + E) * (1 + E))
    r, d = -yl * theta_hat, yl * yl * kappa
    grad = np.zeros(6 + M, X)
    grad[:6] = (q * r).sum(axis=1)
    hess = np.einsum('ai,bi->ab', q * d, q)
    psi = phi.sum()
    out.update(phi_sum=psi, reg_sum=X(0), reg0=X(0))
    if deform and M > 0:
        np.add.at(grad[6:], sm.indices, data * r[row])
        al, ep = X(float(cfg.get('alpha', 0.5))), X(float(cfg.get('epsilon', 1.0)))
        t2 = np.sqrt(xil * xil + ep)
        grad[6:] += al * xil / t2
        reg_sum, reg0 = al * t2.sum(), al * np.sqrt(ep) * M
        psi = psi + max(reg_sum - reg0, X(0))
        out.update(reg_sum=reg_sum, reg0=reg0)
    ymax = float(np.abs(y[region]).max())
    out.update(psi=psi, grad=grad, hess_theta=hess, y=y[region].copy(), t=t, theta_hat=theta_hat, kappa=kappa, A=A,
               abs_r=np.abs(r).sum(), abs_d=d.sum(), yexp=int(np.frexp(ymax)[1]) if ymax > 0 else -400,
               rows=rr, cols=cc, u_local=ul, v_local=vl)        # (for hessian_reference: image coordinates and local coordinates of the pixels)
    return out


# ---------------------------------------------------------------------------------------------------------
# The Newton step of the solve kernels (sdsm_batch_eval_step): the approximate Hessian, its envelope, the backward error of the
# factorisation.  NumPy only (and the oracle: test infrastructure).
# ---------------------------------------------------------------------------------------------------------
HESS_THR = 0.1                   # the solver's leading rule (BatchParams.hess_thr, ORC_HESS_THR)
PANEL = 4                        # SDSM_PANEL
HZREG = 8                        # SDSM_HZREG: leading entries of a run held in registers


def leading_entries(indptr, data, hess_thr=HESS_THR):
    """Which entries of the rows of G~ are LEADING ones: the oracle's rule (sdsm_oracle.c, energy_eval_chunk), compared in float32 --
    ``(float) w >= (float) hess_thr * (float) wmax`` with wmax the row's largest entry; ``hess_thr`` = 0: all of them."""
    data = np.asarray(data)
    if not hess_thr > 0:
        return np.ones(data.size, bool)
    w32 = data.astype(np.float32)
    wmax = np.maximum.reduceat(w32, indptr[:-1]) if data.size else np.zeros(0, np.float32)
    return w32 >= np.float32(hess_thr) * np.repeat(wmax, np.diff(indptr))


def envelope_reference(rows, cols, M, indptr, indices, lead):
    """The envelope of the approximate Hessian as the setup kernel defines it, from the leading entries of every pixel (region pixels
    in raster order at image coordinates ``rows``, ``cols``): ``fst[a]`` = the smallest column any pixel couples with a column >= a,
    rounded down to a multiple of the panel width (non-decreasing by construction), ``rb[a]`` = the row's base so that entry (a, b) is
    at rb[a] + b, the 6 dense theta rows behind the xi rows, ``rend[p]`` = the last xi row whose first column is <= PANEL p,
    ``env_size``; ``run_hz``: leading entries per RUN (the region pixels of one image row inside one aligned 4-column cell; an entry
    counts once if it is a leading one for any pixel of the run) and ``hzmax``, their maximum."""
    first = np.arange(M)
    runs = {}
    for i in range(len(rows)):
        j = indices[indptr[i]:indptr[i + 1]][lead[indptr[i]:indptr[i + 1]]]
        if j.size:
            first[j] = np.minimum(first[j], j.min())
            runs.setdefault((int(rows[i]), int(cols[i]) >> 2), set()).update(j.tolist())
    fst = (np.minimum.accumulate(first[::-1])[::-1] // PANEL) * PANEL if M else first
    width = np.arange(M) - fst + 1
    start = np.concatenate([[0], np.cumsum(width)])
    exi = int(start[-1])
    rb = np.concatenate([start[:-1] - fst, exi + np.arange(6) * M + np.arange(6) * (np.arange(6) + 1) // 2]).astype(np.int64)
    fst_all = np.concatenate([fst, np.zeros(6, np.int64)]).astype(np.int64)
    rend = np.array([np.flatnonzero(fst <= PANEL * p).max() for p in range((M + PANEL - 1) // PANEL)], np.int64)
    run_hz = np.array([len(v) for v in runs.values()], np.int64)
    return dict(fst=fst_all, rb=rb, rend=rend, env_size=exi + 6 * M + 21, run_hz=run_hz, hzmax=int(run_hz.max()) if run_hz.size else 0)


def lead_gram(q, pw, smat, lead, M):
    """sum_i pw_i J_i J_i^T over the pixels, J_i = (q[:, i], the LEADING entries of row i of G~): the (6 + M)^2 matrix of the solver's
    approximate Hessian for pixel weights ``pw`` (np.longdouble; unknowns theta, then xi).  theta-theta: all pixels; theta-xi and
    xi-xi: only over the entries that are leading for the pixel.  ``smat`` = (indptr, indices, data); ``data`` may be replaced by
    ones to count the pixels that couple two unknowns."""
    X = np.longdouble
    q, pw = np.asarray(q, X), np.asarray(pw, X)
    N, n = q.shape[1], 6 + M
    Hm = np.zeros((n, n), X)
    Hm[:6, :6] = np.einsum('ai,bi->ab', q * pw, q)
    if M == 0:
        return Hm
    indptr, indices, data = smat
    row = np.repeat(np.arange(N), np.diff(indptr))[lead]
    col, w = np.asarray(indices)[lead].astype(np.int64), np.asarray(data)[lead].astype(X)
    for k in range(6):
        tx = np.zeros(M, X)
        np.add.at(tx, col, q[k, row] * pw[row] * w)
        Hm[k, 6:], Hm[6:, k] = tx, tx
    cnt = np.bincount(row, minlength=N)
    start = np.concatenate([[0], np.cumsum(cnt)])
    flat = np.zeros(M * M, X)
    for k in np.unique(cnt[cnt > 0]):                      # pixels with k leading entries: all their pairs at once
        pix = np.flatnonzero(cnt == k)
        e = start[pix][:, None] + np.arange(k)[None, :]
        ck, wk = col[e], w[e]
        val = pw[pix][:, None, None] * wk[:, :, None] * wk[:, None, :]
        np.add.at(flat, (ck[:, :, None] * M + ck[:, None, :]).ravel(), val.ravel())
    Hm[6:, 6:] = flat.reshape(M, M)
    return Hm


def hessian_reference(y, y_mask, atoms, fp, cfg, theta, xi=None, box=None, reg_mu=0.0, hess_thr=HESS_THR):
    """:func:`energy_reference` and, in the candidate's LOCAL frame (``u_local``, ``v_local``; theta_local = R theta), the gradient
    ``grad_local`` and the solver's full approximate Hessian ``hess`` ((6 + M)^2, np.longdouble, unknowns theta then xi):
    theta-theta sum_i d_i q_a q_b over all pixels, q = (u^2, v^2, 2 u v, 2 u, 2 v, 1), d_i = y_i^2 kappa_i; theta-xi and xi-xi only
    over the entries of G~ that are leading for pixel i (:func:`leading_entries`); xi diagonal plus the regulariser's curvature
    max(0, alpha eps / (xi^2 + eps)^(3/2)), blended by ``reg_mu`` towards alpha / sqrt(xi^2 + eps) (sdsm_oracle.c, energy_eval_thr).
    Also ``q_local`` (6 x N), ``r``, ``d`` per pixel, ``lead`` (per entry of ``smat``), ``xi``, ``reg_curv`` (the blended curvature) and
    ``reg_major`` = alpha / sqrt(xi^2 + eps)."""
    X = np.longdouble
    ref = energy_reference(y, y_mask, atoms, fp, cfg, theta, xi, box)
    N, M = ref['N'], ref['M']
    ul, vl = ref['u_local'], ref['v_local']
    ql = np.stack([ul * ul, vl * vl, 2 * ul * vl, 2 * ul, 2 * vl, np.ones(N, X)])
    yl = ref['y'].astype(X)
    r, d = -yl * ref['theta_hat'], yl * yl * ref['kappa']
    lead = leading_entries(ref['smat'][0], ref['smat'][2], hess_thr) if M > 0 else None
    Hm = lead_gram(ql, d, ref['smat'], lead, M)
    grad_local = np.concatenate([(ql * r).sum(axis=1), ref['grad'][6:]])
    ref.update(hess=Hm, grad_local=grad_local, q_local=ql, r=r, d=d, lead=lead, reg_mu=float(reg_mu), xi=np.zeros(0, X))
    if M > 0:
        al, ep = X(float(cfg.get('alpha', 0.5))), X(float(cfg.get('epsilon', 1.0)))
        xil = np.asarray(xi, np.float64).ravel().astype(X)
        t2 = np.sqrt(xil * xil + ep)
        gd = np.maximum(al * ep / (t2 * t2 * t2), X(0))
        gd = gd + X(float(reg_mu)) * (al / t2 - gd)
        Hm[6 + np.arange(M), 6 + np.arange(M)] += gd
        ref.update(reg_curv=gd, reg_major=al / t2, xi=xil)
    return ref


# The Newton step (factor_solve of sdsm_solve.hip) is held by its BACKWARD error, so no condition number enters: with the kernel's own
# float64 H, g and d, r = (H + tau diag H) d + g must satisfy |r_i| <= gamma sqrt(h_ii) sum_j sqrt(h_jj) |d_j|.
# Where gamma comes from (u = 2^-53; Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Lemma 8.4, Theorems 10.3 / 10.4;
# E_RSQRT = 4.2e-15 is rsqrt_f64's relative error, tests/test_loss_arithmetic_gpu.py):
#   * a factor entry is l_ik = (a_ik - sum_{m < k} l_im l_km) rho_k with rho_k the reciprocal pivot: at most k <= n multiply-subtracts
#     (each product and each difference rounds once, or once together as a fused multiply-add) and the scaling -- by Lemma 8.4 the
#     computed factor reproduces A with |dA| <= gamma_n |L| |L^T|, gamma_k = k u / (1 - k u);
#   * the forward substitution rides along as row n of the same loops: gamma_n |L|; the back substitution does the same number of
#     multiply-subtracts per unknown plus two scalings (y~ = y rho, the factor row times rho): gamma_(n + 2) |L^T|;
#     together (Theorem 10.4) (3 n + 2) u |L| |L^T|, and (|L| |L^T|)_ij <= sqrt(a_ii a_jj) (Cauchy-Schwarz on the rows of L);
#   * every value passes through a reciprocal pivot at most three times -- when its factor entry is scaled and once in each substitution
#     --, each within E_RSQRT of 1 / sqrt(pivot): 3 E_RSQRT (an upper bound: the kernel uses the SAME rho_k wherever the pivot
#     enters, so most of this error is a consistent rescaling that cancels);
#   * the shifted diagonal a_ii = fl(h_ii (1 + tau)): one more u on the diagonal, and a_ii <= (1 + tau) h_ii (1 + u).
# gamma = ((3 n + 3) u + 3 E_RSQRT) (1 + tau) (1 + 1e-6); the last factor covers the second-order terms (products of two of the above,
# each < 1e-12).  The elliptical model (M = 0) solves the Jacobi-scaled system S H S + tau I, S = diag(rsqrt(h_ii)), and returns
# d = S z: in unscaled terms the same residual with the same bound (the scaled diagonal is 1 + tau, z_j = sqrt(h_jj) d_j; the error
# of S moves the shift tau h_ii by 2 E_RSQRT of itself, inside the pivot term).
# lam2 = ||L^-1 g||^2 is compared with -g.d in np.longdouble: 2 gamma (sum_j sqrt(h_jj) |d_j|)^2 + n u sum |g_i d_i|.
STEP_E_RSQRT = 4.2e-15


def step_gamma(n, tau):
    u = 2.0 ** -53
    return ((3 * n + 3) * u + 3 * STEP_E_RSQRT) * (1 + tau) * (1 + 1e-6)


def step_residual(Hm, g, d, tau):
    """The backward error of one Newton step in np.longdouble: ``r`` = (H + tau diag H) d + g, its componentwise ``bound``
    gamma sqrt(h_ii) sum_j sqrt(h_jj) |d_j|, ``ratio`` = max |r_i| / bound_i; ``lam2`` = -g.d with ``lam2_bound`` (see above)."""
    X = np.longdouble
    Hm, g, d = np.asarray(Hm, np.float64).astype(X), np.asarray(g, np.float64).astype(X), np.asarray(d, np.float64).astype(X)
    n = g.size
    diag = np.diagonal(Hm).copy()
    r = Hm @ d + X(float(tau)) * diag * d + g
    sd = np.sqrt(np.maximum(diag, X(0)))
    s = (sd * np.abs(d)).sum()
    gamma = X(step_gamma(n, float(tau)))
    bound = gamma * sd * s
    with np.errstate(all='ignore'):
        ratio = np.where(r == 0, X(0), np.abs(r) / bound)
    return dict(r=r, bound=bound, ratio=float(ratio.max()), lam2=-(g * d).sum(), lam2_bound=2 * gamma * s * s + n * X(2.0) ** -53 * np.abs(g * d).sum())
