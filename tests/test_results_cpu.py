"""Label maps and overlays without a GPU: the closed forms of the overlay kernel against the label-by-label host definitions, the host
definitions against fixtures of the reference, the sparse host flood against ``render._watershed``, the new entry points of
include/sdsm.h (binding and argument checks), and the orchestration of ``rasterize_labels_gpu`` / ``_many`` with the device phases
replaced by a host restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

from superdsm_amd import _capi, _morph, render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


class Obj:
    def __init__(self, offset, fragment):
        self.fg_offset, self.fg_fragment = np.asarray(offset, int), np.asarray(fragment, bool)

    def fill_foreground(self, out, value=True):
        h, w = self.fg_fragment.shape
        out[self.fg_offset[0]:self.fg_offset[0] + h, self.fg_offset[1]:self.fg_offset[1] + w][self.fg_fragment] = value


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def disk_min_max(labels, r):
    """mn / mx over the in-image pixels of disk(r): edge replication adds only pixels that are in the image and in the disk."""
    fp = _morph.disk(r).astype(bool)
    return ndi.minimum_filter(labels, footprint=fp, mode='nearest'), ndi.maximum_filter(labels, footprint=fp, mode='nearest')


def random_label_map(shape, n_labels, seed, background=True):
    """Non-overlapping labels: discs painted one over the other, some touching the image border."""
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, np.int32) if background else rng.integers(1, 3, shape).astype(np.int32)
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    for l in range(1, n_labels + 1):
        cy, cx, r = rng.integers(0, shape[0]), rng.integers(0, shape[1]), rng.integers(2, 12)
        lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = l
    return lab


# ---- the closed forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('radius', [1, 2, 3, 4, 5, 16])
def test_closed_forms_equal_the_label_by_label_definitions(radius):
    for seed, shape in enumerate([(60, 75), (41, 37), (1, 50), (35, 90)]):
        lab = random_label_map(shape, 12, 10 * radius + seed, background=seed != 3)
        mn, mx = disk_min_max(lab, radius)
        for bgl in (None, 0, 2):
            borders, background = render.rasterize_regions_host(lab, bgl, radius)
            assert np.array_equal(borders, mn != mx)
            assert np.array_equal(background, (mn == mx) & (mn == bgl) if bgl is not None else np.zeros(shape, bool))
        center = np.zeros(shape, bool)
        inner = np.zeros(shape, bool)
        for l in set(lab.reshape(-1).tolist()) - {0}:
            center |= render.contour_mask_host(lab == l, radius, 'center')
            inner |= render.contour_mask_host(lab == l, radius, 'inner')
        assert np.array_equal(center, (mx > 0) & (mn != mx))
        mn2, mx2 = disk_min_max(lab, 2 * radius)
        assert np.array_equal(inner, (lab > 0) & (mn2 != mx2))


# ---- fixtures of the reference -------------------------------------------------------------------------------------------------------
def _fixture_objects(f):
    return [Obj(f[f'o{k}_offset'], f[f'o{k}_fragment']) for k in range(int(f['n']))]


def test_overlay_host_definitions_against_the_reference():
    f = np.load(os.path.join(GOLDEN, 'overlays.npz'))
    data = {'g_raw': f['g_raw'], 'atoms': f['atoms'], 'clusters': f['clusters']}
    objs = _fixture_objects(f)
    img, mn, mx = render.normalize_image(f['g_raw'], ret_minmax=True)
    assert same(img, f['normalized']) and mn == f['normalized_min'] and mx == f['normalized_max']
    assert same(render.normalize_image(f['g_raw'], spread=0.5), f['normalized_half'])
    assert same(render.render_result_over_image_host(data, objs), f['result_center'])
    assert same(render.render_result_over_image_host(data, objs, border_width=4, border_position='inner', color='y'), f['result_inner'])
    assert same(render.render_result_over_image_host(data, objs, border_width=2, override_img=f['override']), f['result_override'])
    assert same(render.render_result_over_image_host(dict(data, g_rgb=f['g_rgb']), objs, color='r'), f['result_rgb'])
    assert same(render.render_atoms_host(data), f['atoms_overlay'])
    assert same(render.render_foreground_clusters_host(data, border_radius=3), f['clusters_overlay'])
    assert same(render.render_atoms_host(data, normalize_img=False, override_img=f['override']), f['atoms_override'])


# ---- the host flood ------------------------------------------------------------------------------------------------------------------
def _sparse_flood(image, markers, mask):
    """render._watershed through sdsm_flood_sparse: only the unlabelled masked pixels and the markers next to one go in."""
    out = np.where(mask, markers, 0).astype(np.int64)
    todo = mask & (out == 0)
    near = ndi.binary_dilation(todo, structure=ndi.generate_binary_structure(2, 1)) & (out > 0)
    idx = np.nonzero((todo | near).reshape(-1))[0]
    flooded = render.flood_sparse(idx, out.reshape(-1)[idx], np.asarray(image, np.float64).reshape(-1)[idx], *image.shape)
    out.reshape(-1)[idx] = flooded
    return out


@pytest.mark.parametrize('seed', range(12))
def test_sparse_flood_equals_the_watershed_of_the_definition(seed):
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(1, 40)), int(rng.integers(1, 50))
    mask = rng.random((H, W)) < 0.8
    markers = np.where(rng.random((H, W)) < [0.02, 0.1, 0.4][seed % 3], rng.integers(1, 9, (H, W)), 0)
    if seed % 2:                     # distances with many ties: the EDT of a few points (square roots of small integers), or constants
        pts = rng.random((H, W)) < 0.03
        image = ndi.distance_transform_edt(~pts) if pts.any() else np.zeros((H, W))
    else:
        image = rng.integers(0, 3, (H, W)).astype(np.float64)
    want = render._watershed(image, markers, mask)
    assert np.array_equal(_sparse_flood(image, markers, mask), want)


def _sdsm_watershed(image, markers, mask):
    out = np.zeros(image.shape, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    im, mk, ms = np.ascontiguousarray(image, np.float64), np.ascontiguousarray(markers, np.int32), np.ascontiguousarray(mask, np.uint8)
    assert _capi.lib().sdsm_watershed(p(im), p(mk), p(ms), image.shape[0], image.shape[1], p(out)) == 0
    return out


def test_sparse_flood_on_tied_seeds_and_its_argument_check():
    """Constant and two-valued images: every decision is a tie, settled by seed order and push age.  The rule of ``_watershed`` (seed
    ages 0, 1, 2, ...; up, down, left, right) and that of sdsm_watershed (all markers age 0, ties by raster index; up, left, right,
    down) order the heap differently only among pixels pushed by ONE popped pixel, which carry one label, so the two produce the same
    label maps; that is recorded here as an observation on these cases, the definition the flood is held to is ``_watershed``."""
    rng = np.random.default_rng(3)
    agree = 0
    for k in range(60):
        H, W = int(rng.integers(2, 9)), int(rng.integers(2, 9))
        markers = np.where(rng.random((H, W)) < 0.2, rng.integers(1, 5, (H, W)), 0)
        image = rng.integers(0, 2, (H, W)).astype(np.float64) if k % 2 else np.zeros((H, W))
        mask = rng.random((H, W)) < (1.0 if k % 3 else 0.85)
        want = render._watershed(image, markers, mask)
        assert np.array_equal(_sparse_flood(image, markers, mask), want)
        agree += np.array_equal(_sdsm_watershed(image, markers, mask), want)
    assert agree == 60
    # unsorted indices are refused
    assert _capi.lib().sdsm_flood_sparse(2, np.array([3, 1], np.int32).ctypes.data_as(C.c_void_p), None, None, 2, 2, None) == -1


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ['sdsm_render_morph', 'sdsm_render_morph_multi', 'sdsm_render_overlaps', 'sdsm_render_paint', 'sdsm_render_paint_multi',
               'sdsm_render_compact', 'sdsm_render_compact_multi', 'sdsm_flood_sparse', 'sdsm_render_scatter', 'sdsm_render_lost',
               'sdsm_render_lost_multi', 'sdsm_render_fill', 'sdsm_render_fill_multi', 'sdsm_render_finish', 'sdsm_render_overlay',
               'sdsm_render_overlay_multi']
_CTYPES = {'int': C.c_int, 'int64_t': C.c_int64, 'double': C.c_double, 'size_t': C.c_size_t}


def test_new_symbols_resolve_with_the_declared_argument_types():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sdsm.h')).read(), flags=re.S)
    lib = _capi.lib()
    for name in NEW_SYMBOLS:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', text)
        assert m, f'{name} is not declared in include/sdsm.h'
        res, args = _capi.SYMBOLS[name]
        assert res is C.c_int and getattr(lib, name).argtypes == args
        declared = [a.strip() for a in m.group(1).split(',')]
        assert len(declared) == len(args), name
        for d, a in zip(declared, args):
            if '*' in d:
                want = {'const sdsm_set_image': C.POINTER(_capi.SetImage)}.get(d.split('*')[0].strip())
                if a is not C.c_void_p:
                    assert a in (want, C.POINTER(C.c_double), C.POINTER(C.c_int64)) and d.split('*')[0].strip() in ('const sdsm_set_image', 'const double', 'const int64_t'), (name, d)
            else:
                assert a is _CTYPES[d.rsplit(' ', 1)[0].replace('const ', '').strip()], (name, d)
    assert _capi.RENDER_MAX_RADIUS == 16 and '#define SDSM_RENDER_MAX_RADIUS 16' in text
    assert _capi.RENDER_ENTRY_DTYPE.itemsize == 16


def test_argument_checks_come_before_any_device_work():
    lib = _capi.lib()
    one = (_capi.SetImage * 1)()
    one[0].offset, one[0].H, one[0].W = 0, 8, 8
    many = (_capi.SetImage * 33)()
    for k in range(33):
        many[k].offset, many[k].H, many[k].W = 64 * k, 8, 8
    x = C.c_void_p(256)              # never dereferenced: every call below is refused on its arguments
    col = (C.c_double * 3)(0, 1, 0)
    for radius in (17, -17, 0):
        assert lib.sdsm_render_morph(8, 8, 1, x, x, x, radius, x, x, x, None) == -1
        assert b'radius' in lib.sdsm_last_error()
        assert lib.sdsm_render_morph_multi(one, 1, 1, x, x, x, x, radius, x, x, x, None) == -1
    assert lib.sdsm_render_overlay(8, 8, x, x, 1, 1, 17, col, None, 0, x, None) == -1 and b'radius' in lib.sdsm_last_error()
    assert lib.sdsm_render_overlay(8, 8, x, x, 2, 1, 3, col, None, 0, x, None) == -1
    assert lib.sdsm_render_overlay(8, 8, x, x, 1, 4, 3, col, None, 0, x, None) == -1 and lib.sdsm_render_overlay(8, 8, x, None, 1, 2, 3, col, None, 0, x, None) == -1
    cap = (C.c_int64 * 33)()
    for n_images, table in ((33, many), (0, many)):       # more than 32 images, the empty set
        assert lib.sdsm_render_morph_multi(table, n_images, 1, x, x, x, x, 2, x, x, x, None) == -1 and b'32 images' in lib.sdsm_last_error()
        assert lib.sdsm_render_paint_multi(table, n_images, 1, x, x, x, x, x, x, x, x, None) == -1
        assert lib.sdsm_render_compact_multi(table, n_images, x, x, x, cap, x, x, None) == -1
        assert lib.sdsm_render_lost_multi(table, n_images, 1, x, x, x, x, x, 1, x, x, x, None) == -1
        assert lib.sdsm_render_fill_multi(table, n_images, 1, x, x, x, x, x, x, 1, x, x, None) == -1
        assert lib.sdsm_render_overlay_multi(table, n_images, x, x, 1, 1, 3, col, None, 0, x, None) == -1
    assert lib.sdsm_render_finish(64, x, 1, x, None) == -1 and lib.sdsm_render_fill(8, 8, 1, x, x, x, x, x, 65536, x, x, None) == -1
    assert lib.sdsm_render_overlaps(-1, x, x, x, x, x, None) == -1 and lib.sdsm_render_scatter(-1, x, x, x, None) == -1
    assert lib.sdsm_render_overlaps(0, None, None, None, None, None, None) == 0 and lib.sdsm_render_scatter(0, None, None, None, None) == 0
    with pytest.raises(NotImplementedError, match='Limits'):
        render.rasterize_labels_gpu({'g_raw': np.zeros((8, 8))}, [], dilate=17)
    with pytest.raises(NotImplementedError, match='Limits'):
        render.render_result_over_image({'g_raw': np.zeros((8, 8))}, [], border_position='outer')


# ---- orchestration with the device phases restated on the host -------------------------------------------------------------------
class HostSet:
    """The interface of render._GpuSet in NumPy / SciPy, from the definition's own building blocks."""
    created = []

    def __init__(self, shapes):
        self.shapes = [(int(h), int(w)) for h, w in shapes]
        assert 1 <= len(self.shapes) <= _capi.MAX_SET_IMAGES
        sizes = [(h * w + 63) // 64 * 64 for h, w in self.shapes]
        self.offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        self.total = int(sum(sizes))
        self.label = np.zeros(self.total, np.int32)
        HostSet.created.append(self)

    def _view(self, a, i):
        h, w = self.shapes[i]
        return a[self.offsets[i]:self.offsets[i] + h * w].reshape(h, w)

    def load(self, obj_image, boxes, words, packed):
        self.obj_image, self.boxes = np.asarray(obj_image), np.asarray(boxes, np.int64).reshape(-1, 4)
        self.masks = []
        for i, (r0, c0, h, w), bits in zip(obj_image, boxes, packed):
            m = np.zeros(self.shapes[i], bool)
            m[r0:r0 + h, c0:c0 + w] = np.unpackbits(bits, bitorder='little')[:h * w].reshape(h, w).astype(bool)
            self.masks.append(m)

    def morph(self, radius):
        fn = _morph.binary_dilation if radius > 0 else _morph.binary_erosion
        self.masks = [fn(m, _morph.disk(abs(radius))) for m in self.masks]
        from superdsm_amd.postprocess import grown_windows
        H, W = (np.array([s[k] for s in self.shapes], np.int64)[self.obj_image] for k in (0, 1))
        windows = grown_windows(self.boxes, H, W, abs(radius))
        return windows.astype(np.int32), np.array([int(k.sum()) for k in self.masks], np.int64)

    def select(self, keep):
        self.masks = [m for m, k in zip(self.masks, keep) if k]
        self.obj_image = self.obj_image[keep]

    def overlaps(self, pairs):
        return np.array([int((self.masks[a] & self.masks[b]).sum()) for a, b in pairs], np.int64)

    def paint(self, obj_label):
        self.obj_label = np.asarray(obj_label)
        self.cover = np.zeros(self.total, np.uint8)
        for i in range(len(self.shapes)):
            lab, cov = self._view(self.label, i), self._view(self.cover, i)
            ks = np.nonzero(self.obj_image == i)[0]
            for l in sorted(set(self.obj_label[ks].tolist())):
                m = np.any([self.masks[k] for k in ks if self.obj_label[k] == l], axis=0)
                lab[m] = l
                cov[m] += 1
            cov[cov > 2] = 2
            lab[cov == 2] = 0

    def flood_inputs(self, capacity):
        out = []
        for i in range(len(self.shapes)):
            lab, cov = self._view(self.label, i), self._view(self.cover, i)
            dist = ndi.distance_transform_edt(lab == 0)
            take = (cov == 2) | (ndi.binary_dilation(cov == 2, structure=ndi.generate_binary_structure(2, 1)) & (lab > 0))
            idx = np.nonzero(take.reshape(-1))[0]
            assert len(idx) <= capacity[i]
            e = np.zeros(len(idx), _capi.RENDER_ENTRY_DTYPE)
            e['idx'], e['label'], e['dist'] = idx, lab.reshape(-1)[idx], dist.reshape(-1)[idx]
            out.append(e)
        return out

    def scatter(self, pix, lab):
        self.label[pix] = lab

    def lost(self, obj_group, n_groups):
        lost, vmax = np.zeros(n_groups + 1, np.int64), np.zeros(len(self.shapes), np.int64)
        for k, m in enumerate(self.masks):
            lab = self._view(self.label, self.obj_image[k])
            lost[obj_group[k]] += int((lab[m] == 0).sum())
            vmax[self.obj_image[k]] = lab.max()
        return lost, vmax

    def fill(self, sel, new_label):
        any_ = False
        for k in sel:
            lab = self._view(self.label, self.obj_image[k])
            z = self.masks[k] & (lab == 0)
            any_ |= bool(z.any())
            lab[z] = new_label
        return any_

    def finish(self, background_label):
        out = self.label.astype(np.uint16)
        out[self.label == 0] = np.array(background_label).astype('uint16')
        return [self._view(out, i).copy() for i in range(len(self.shapes))]


def discs(shape, n, rmax, seed):
    rng = np.random.default_rng(seed)
    H, W = shape
    objs = []
    for _ in range(n):
        r, cy, cx = int(rng.integers(1, rmax + 1)), int(rng.integers(0, H)), int(rng.integers(0, W))
        r0, r1, c0, c1 = max(0, cy - r), min(H, cy + r + 1), max(0, cx - r), min(W, cx + r + 1)
        yy, xx = np.mgrid[r0:r1, c0:c1]
        objs.append(Obj((r0, c0), (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r))
    return objs


@pytest.fixture
def host_set(monkeypatch):
    monkeypatch.setattr(render, '_GpuSet', HostSet)
    HostSet.created = []
    return HostSet


@pytest.mark.parametrize('thr', [-1, 0, 0.3, 1, np.inf])
@pytest.mark.parametrize('dilate', [-2, 0, 3])
def test_orchestration_single_image(host_set, thr, dilate):
    shape = (48, 60)
    objs = discs(shape, 18, 8, 7)
    objs = objs[:4] + [Obj(objs[2].fg_offset, objs[2].fg_fragment), Obj((5, 5), np.zeros((3, 3), bool))] + objs[4:] + [Obj(objs[2].fg_offset, objs[2].fg_fragment)]
    data = {'g_raw': np.zeros(shape), 'postprocessed_objects': objs}
    for bgl in (0, -1):
        want = render.rasterize_labels(data, merge_overlap_threshold=thr, dilate=dilate, background_label=bgl)
        assert same(render.rasterize_labels_gpu(data, merge_overlap_threshold=thr, dilate=dilate, background_label=bgl), want)
        assert same(render.rasterize_labels_gpu(data, objs, merge_overlap_threshold=thr, dilate=dilate, background_label=bgl), want)


def test_orchestration_sets_and_splitting(host_set):
    shapes = [(20 + k, 50 - k) for k in range(35)]
    datas = [{'g_raw': np.zeros(s), 'objs': discs(s, k % 6, 6, k)} for k, s in enumerate(shapes)]
    got = render.rasterize_labels_many(datas, 'objs', merge_overlap_threshold=0.4)
    assert [len(s.shapes) for s in host_set.created] == [32, 3]
    assert len(got) == 35
    for d, g in zip(datas, got):
        assert same(g, render.rasterize_labels(d, 'objs', merge_overlap_threshold=0.4))
    assert render.rasterize_labels_many([], 'objs') == []
    with pytest.raises(ValueError):
        render.rasterize_labels_many(datas[:2], [datas[0]['objs']])


def test_too_many_labels_is_an_error(host_set, monkeypatch):
    monkeypatch.setattr(render, '_merge_members', lambda n, *a: [[0]] * 65536)
    with pytest.raises(ValueError, match='65535'):
        render.rasterize_labels_gpu({'g_raw': np.zeros((4, 4))}, [Obj((0, 0), np.ones((1, 1), bool))])


def test_packing_helper_is_shared_with_the_post_processing():
    from superdsm_amd import postprocess
    objs = discs((40, 40), 5, 6, 3)
    boxes, words, new_words, packed, areas = postprocess._pack_objects(objs, 40, 40, 2)
    b2, w2, p2, a2 = postprocess.pack_fragments(objs)
    assert np.array_equal(boxes, b2) and np.array_equal(words, w2) and np.array_equal(areas, a2) and all(np.array_equal(x, y) for x, y in zip(packed, p2))
    assert np.array_equal(new_words, postprocess.window_words(postprocess.grown_windows(boxes, 40, 40, 2)))
    assert postprocess.grown_windows([[1, 38, 3, 2]], 40, 40, 2).tolist() == [[0, 36, 6, 4]]
