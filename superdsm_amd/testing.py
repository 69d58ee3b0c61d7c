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
