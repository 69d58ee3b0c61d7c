"""The host definitions of the skeleton tables (superdsm_amd/skeleton.py): the removal rule against the host helper of the C ABI, the
anchors of the definition pixel by pixel, the CPU thinning of the C ABI (the word functions the kernel compiles) against the NumPy
definition across flat-bit and word seams, the invariants of a skeleton (a subset with the same parts and holes, a fixed point) on
exhaustive and random mask families, the label form, padding and shifting, the derived columns and the CSV writer.  No GPU."""
import csv
import math
import os
import subprocess

import numpy as np
import pytest

from test_measure_cpu import Obj, label_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('area', 'n_skeleton', 'n_end', 'n_isolated', 'n_branch', 'n_orth', 'n_diag', 'cycles', 'first_row', 'first_col', 'flags', 'reserved')


def thin_c(mask):
    """(skeleton, cycles) of sdsm_skeleton_thin for a bool mask."""
    from superdsm_amd import _capi
    from superdsm_amd.postprocess import pack_windows, unpack_windows
    dims, off, bits = pack_windows([mask])
    out = np.full_like(bits, 0xff)
    cycles = _capi.lib().sdsm_skeleton_thin(mask.shape[0], mask.shape[1], bits.ctypes.data, out.ctypes.data)
    return unpack_windows(out, off, dims)[0], cycles, out


def all_masks(h, w):
    """Every mask of h x w as a stack (2^(h w), h, w)."""
    codes = np.arange(2 ** (h * w), dtype=np.int64)
    return ((codes[:, None] >> np.arange(h * w)) & 1).astype(bool).reshape(-1, h, w)


def random_masks():
    """1 900 masks with fixed seeds: noise at densities 0.3 .. 0.95, thresholded smoothed noise without and with pepper holes, unions of
    rectangles."""
    from scipy import ndimage as ndi
    rng = np.random.default_rng(20261021)
    out = []
    for k in range(700):
        h, w = rng.integers(3, 22, size=2)
        out.append(rng.random((h, w)) < 0.3 + 0.65 * k / 699)
    for k in range(800):
        h, w = rng.integers(8, 30, size=2)
        m = ndi.gaussian_filter(rng.normal(size=(h, w)), rng.uniform(1, 3)) > rng.uniform(-0.1, 0.1)
        out.append(m & (rng.random((h, w)) > 0.04) if k % 2 else m)
    for k in range(400):
        h, w = rng.integers(8, 30, size=2)
        m = np.zeros((h, w), bool)
        for _ in range(rng.integers(1, 6)):
            r0, c0 = rng.integers(0, h - 1), rng.integers(0, w - 1)
            m[r0:r0 + rng.integers(1, 12), c0:c0 + rng.integers(1, 12)] = True
        out.append(m)
    return out


def topology(mask):
    """(8-connected parts, holes under 4-connected background) by the definitions of the connected parts."""
    from superdsm_amd import parts
    if not mask.any():
        return 0, 0
    return len(parts.label_mask_host(mask, 8)[1]), int(parts.holes_host(mask.astype(np.int32), 8)[1])


def topology_fast(mask):
    """The same two counts straight from SciPy's labelling, for the exhaustive families."""
    from scipy import ndimage as ndi
    return ndi.label(mask, np.ones((3, 3)))[1], ndi.label(~np.pad(mask, 1))[1] - 1


def row_of(mask, offset=(2, 2), shape=None):
    from superdsm_amd import skeleton as sk
    shape = (mask.shape[0] + 4, mask.shape[1] + 4) if shape is None else shape
    table, frags = sk.skeleton_objects_host([Obj(offset, mask)], shape)
    return table[0], frags[0]


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def test_record_layout_is_mirrored():
    from superdsm_amd import _capi, skeleton as sk
    assert _capi.SKELETON_RECORD_DTYPE.itemsize == 48 and _capi.SKELETON_RECORD_DTYPE.names == FIELDS and sk.TABLE_DTYPE.names == ('label',) + FIELDS
    header = open(os.path.join(ROOT, 'include', 'sdsm.h')).read()
    assert f'#define SDSM_SKELETON_LDS_WORDS {_capi.SKELETON_LDS_WORDS} ' in header
    inline = open(os.path.join(ROOT, 'superdsm_amd', 'csrc', 'sdsm_skeleton.h')).read()
    assert f'#define SDSM_SKELETON_LDS_WORDS_INLINE {_capi.SKELETON_LDS_WORDS} ' in inline


def test_the_rule_of_the_c_abi_equals_the_definition_and_has_41_codes_per_direction():
    from superdsm_amd import _capi, skeleton as sk
    helper = _capi.lib().sdsm_skeleton_deletable
    for d in (0, 4, 2, 6):
        want = [sk.deletable(code, d) for code in range(256)]
        assert sum(want) == 41
        assert [helper(code, d) for code in range(256)] == [int(v) for v in want]
    assert [helper(256, 0), helper(-1, 0), helper(3, 1), helper(3, 8), helper(3, -2)] == [-1] * 5
    assert sk.deletable(0b00011100, 0) and not sk.deletable(0b00011101, 0)          # a border pixel on its north side / not one
    assert not sk.deletable(0b00010000, 0) and not sk.deletable(0b00010001, 2)      # an end / a pixel that connects north and south
    with pytest.raises(ValueError):
        sk.deletable(3, 1)
    with pytest.raises(ValueError):
        sk.deletable(256, 0)


def test_the_bit_sliced_rule_of_a_subiteration_equals_the_scalar_rule_for_every_code():
    """Every code as the neighbourhood of the centre of a 3 x 3 mask: the centre goes in the first subiteration that the scalar rule
    names (``_removed`` is the bit-sliced form on arrays; the C side's is checked through sdsm_skeleton_thin below)."""
    from superdsm_amd import skeleton as sk
    for code in range(256):
        m = np.zeros((3, 3), bool)
        m[1, 1] = True
        for k, (dr, dc) in enumerate(sk.RING):
            m[1 + dr, 1 + dc] = (code >> k) & 1
        for d in sk.DIRECTIONS:
            assert bool(sk._removed(m[None], d)[0, 1, 1]) == sk.deletable(code, d), (code, d)


# ---- the anchors ------------------------------------------------------------------------------------------------------------------------
def test_anchors_of_small_full_boxes():
    from superdsm_amd import skeleton as sk
    for shape, want, cycles in (((1, 1), [[1]], 0), ((1, 7), [[1] * 7], 0), ((2, 2), [[0, 0], [1, 1]], 1), ((3, 3), [[0, 0, 0], [1, 1, 1], [0, 0, 0]], 1)):
        S, c = sk.thin_host(np.ones(shape, bool))
        assert S.astype(int).tolist() == want and c == cycles and S.dtype == bool
    S, c = sk.thin_host(np.ones((5, 12), bool))
    want = np.zeros((5, 12), bool)
    want[2, 1:11] = True
    assert np.array_equal(S, want) and c == 2
    row, _ = row_of(np.ones((5, 12), bool))
    assert tuple(row[n] for n in FIELDS) == (60, 10, 2, 0, 0, 9, 0, 2, 4, 3, 0, 0)


def test_anchor_ring_is_a_closed_loop():
    m = np.ones((9, 9), bool)
    m[3:6, 3:6] = False
    row, S = row_of(m)
    want = np.zeros((9, 9), bool)
    want[1, 2:7] = want[7, 2:7] = want[2:7, 1] = want[2:7, 7] = True
    assert np.array_equal(S, want)
    assert tuple(row[n] for n in FIELDS) == (72, 20, 0, 0, 0, 16, 4, 2, 3, 4, 0, 0)


def test_anchor_plus_and_t():
    plus = np.zeros((21, 21), bool)
    plus[8:13] = plus[:, 8:13] = True
    row, S = row_of(plus)
    want = np.zeros((21, 21), bool)
    want[10, 1:20] = want[2:19, 10] = True
    assert np.array_equal(S, want)
    assert tuple(row[n] for n in FIELDS) == (185, 35, 4, 0, 1, 34, 0, 2, 4, 12, 0, 0)
    t = np.zeros((20, 31), bool)
    t[2:7, 1:30] = t[2:19, 13:18] = True
    row, S = row_of(t)
    assert tuple(row[n] for n in FIELDS[:8]) == (205, 38, 3, 0, 1, 35, 2, 3) and S.sum() == 38


def test_anchor_disc_of_radius_30_takes_21_cycles():
    y, x = np.mgrid[:61, :61]
    row, S = row_of((y - 30) ** 2 + (x - 30) ** 2 <= 900)
    assert tuple(row[n] for n in FIELDS[:8]) == (2821, 2, 2, 0, 0, 1, 0, 21) and S.sum() == 2


# ---- sdsm_skeleton_thin equals thin_host ----------------------------------------------------------------------------------------------------
def test_the_c_thinning_equals_the_definition_on_all_3_by_5_masks():
    from superdsm_amd import skeleton as sk
    masks = all_masks(3, 5)
    S, cycles = sk.thin_stack(masks)
    for k in range(len(masks)):
        if not masks[k].any():
            continue
        got, c, _ = thin_c(masks[k])
        assert np.array_equal(got, S[k]) and c == cycles[k], k
    for k in (1, 77, 4097, 32767):                                            # the stack is the single call
        one = sk.thin_host(masks[k])
        assert np.array_equal(one[0], S[k]) and one[1] == cycles[k]


@pytest.mark.parametrize('w', [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200])
def test_the_c_thinning_equals_the_definition_across_flat_bit_and_word_seams(w):
    from superdsm_amd import skeleton as sk
    rng = np.random.default_rng(w)
    for h in (1, 2, 9, 40):
        for density in (0.55, 0.85, 1.0):
            m = rng.random((h, w)) < density
            want, cycles = sk.thin_host(m)
            got, c, raw = thin_c(m)
            assert np.array_equal(got, want) and c == cycles, (h, w, density)
            tail = (h * w) % 32
            assert tail == 0 or raw.view(np.uint32)[-1] >> tail == 0, 'the bits past h w are clear'
    thick = np.zeros((12, w), bool)                                           # a bar three thick along the whole width, and a diagonal
    thick[4:7] = True
    thick |= np.abs(np.arange(12)[:, None] * max(1, w // 12) - np.arange(w)[None]) <= 1
    want, cycles = sk.thin_host(thick)
    got, c, _ = thin_c(thick)
    assert np.array_equal(got, want) and c == cycles


def test_the_c_thinning_refuses_bad_arguments_and_thins_in_place():
    from superdsm_amd import _capi
    thin = _capi.lib().sdsm_skeleton_thin
    bits = np.array([0x1ff], np.uint32)
    assert thin(0, 3, bits.ctypes.data, bits.ctypes.data) == -1 and thin(3, -1, bits.ctypes.data, bits.ctypes.data) == -1
    assert thin(65536, 32768, bits.ctypes.data, bits.ctypes.data) == -1 and thin(3, 3, None, bits.ctypes.data) == -1 and thin(3, 3, bits.ctypes.data, None) == -1
    assert thin(3, 3, bits.ctypes.data, bits.ctypes.data) == 1 and bits[0] == 0b000111000


# ---- invariants ----------------------------------------------------------------------------------------------------------------------------
def check_invariants(P, S, counts):
    assert not (S & ~P).any(), 'S is a subset of P'
    assert counts(S) == counts(P), 'the parts and the holes of S are those of P'


def test_invariants_on_the_random_families():
    from superdsm_amd import skeleton as sk
    masks = random_masks()
    assert len(masks) == 1900
    for k, m in enumerate(masks):
        S, cycles = sk.thin_host(m)
        check_invariants(m, S, topology)
        again = sk.thin_host(S)
        assert np.array_equal(again[0], S) and again[1] == 0, k
        if k % 50 == 0:
            assert topology(m) == topology_fast(m) and topology(S) == topology_fast(S)


@pytest.mark.parametrize('h, w', [(4, 4), (3, 5)])
def test_invariants_on_every_mask_of_a_small_box(h, w):
    """All 65 536 masks of 4 x 4 through the C helper (and every 16th through the NumPy definition too), all 32 768 of 3 x 5 through the
    stacked definition; the counts straight from SciPy's labelling, which ``test_invariants_on_the_random_families`` holds against the
    definitions of the connected parts."""
    from superdsm_amd import _capi, skeleton as sk
    masks = all_masks(h, w)
    if (h, w) == (4, 4):
        thin = _capi.lib().sdsm_skeleton_thin
        words = np.arange(len(masks), dtype=np.uint32)
        out = np.zeros_like(words)
        cycles = np.array([thin(4, 4, words.ctypes.data + 4 * k, out.ctypes.data + 4 * k) for k in range(len(masks))])
        S = ((out[:, None] >> np.arange(16, dtype=np.uint32)) & 1).astype(bool).reshape(-1, 4, 4)
        sub, sub_cycles = sk.thin_stack(masks[::16])
        assert np.array_equal(sub, S[::16]) and np.array_equal(sub_cycles, cycles[::16])
    else:
        S, cycles = sk.thin_stack(masks)
    assert not (S & ~masks).any()
    again, zero = sk.thin_stack(S)
    assert np.array_equal(again, S) and not zero.any()
    known = {}
    for k in range(len(masks)):
        for m in (masks[k], S[k]):
            key = m.tobytes()
            if key not in known:
                known[key] = topology_fast(m)
        assert known[masks[k].tobytes()] == known[S[k].tobytes()], k


# ---- the label form, padding and shifting -----------------------------------------------------------------------------------------------
def test_the_label_form_gives_per_label_the_object_form_in_its_tight_box():
    from superdsm_amd import skeleton as sk
    rng = np.random.default_rng(12)
    labels = label_scene(rng, (70, 90), 12)
    labels[10:16, 5:40], labels[16:20, 5:40] = 20, 21                         # two touching bars
    table, smap = sk.skeleton_labels_host(labels)
    assert smap.dtype == np.int32 and smap.shape == labels.shape and table['label'].tolist() == sorted(set(labels.ravel().tolist()) - {0})
    assert not (smap[labels == 0]).any() and np.array_equal(smap[smap > 0], labels[smap > 0])
    for row in table:
        l = int(row['label'])
        rr, cc = np.nonzero(labels == l)
        box = (labels == l)[rr.min():rr.max() + 1, cc.min():cc.max() + 1]
        t, f = sk.skeleton_objects_host([Obj((rr.min(), cc.min()), box)], labels.shape)
        assert t[0].tobytes()[4:] == row.tobytes()[4:], l
        assert np.array_equal(smap[rr.min():rr.max() + 1, cc.min():cc.max() + 1] == l, f[0])
    # the other labels repainted or removed: a label's row and pixels stay
    other = labels.copy()
    other[(labels != 20) & (labels > 0)] = 7
    alone = np.where(labels == 20, 20, 0)
    for variant in (other, alone):
        t, m = sk.skeleton_labels_host(variant)
        assert t[t['label'] == 20].tobytes() == table[table['label'] == 20].tobytes() and np.array_equal(m == 20, smap == 20)


def test_keep_absent_background_and_empty_inputs():
    from superdsm_amd import skeleton as sk
    labels = np.zeros((9, 12), np.int64)
    labels[1:4, 1:10], labels[5:8, 2:6] = 2, 5
    kept, smap = sk.skeleton_labels_host(labels, keep_absent=True)
    assert kept['label'].tolist() == [0, 1, 2, 3, 4, 5] and kept['area'].tolist() == [0, 0, 27, 0, 0, 12] and kept['n_skeleton'].tolist() == [0, 0, 9, 0, 0, 4]      # bars three thick: the middle row, as 3 x 3
    assert kept[[0, 1, 3, 4]].tobytes() == sk._table([0, 1, 3, 4], np.zeros(4, kept.dtype)).tobytes()
    everything, m0 = sk.skeleton_labels_host(labels, background_label=None)
    assert everything['label'].tolist() == [0, 2, 5] and np.array_equal(m0, smap)      # label 0 is thinned and writes 0
    none, m = sk.skeleton_labels_host(np.zeros((4, 5), np.uint8))
    assert len(none) == 0 and none.dtype == sk.TABLE_DTYPE and not m.any() and m.dtype == np.int32
    table, frags = sk.skeleton_objects_host([], (5, 5))
    assert len(table) == 0 and frags == []
    table, frags = sk.skeleton_objects_host([Obj((1, 1), np.zeros((2, 3)))], (5, 5))
    assert table.tobytes() == np.zeros(1, sk.TABLE_DTYPE).tobytes() and frags[0].shape == (2, 3) and not frags[0].any()


def test_padding_and_shifting_move_the_skeleton_and_change_first_and_flags_only():
    from superdsm_amd import skeleton as sk
    rng = np.random.default_rng(5)
    blob = np.zeros((17, 23), bool)
    blob[2:15, 3:9] = blob[6:10, 3:21] = True
    blob &= rng.random(blob.shape) > 0.05
    rr, cc = np.nonzero(blob)
    blob = blob[rr.min():rr.max() + 1, cc.min():cc.max() + 1]
    base, S = row_of(blob, (5, 6), (60, 70))
    for top, left, bottom, right in ((0, 0, 0, 0), (3, 0, 0, 0), (0, 5, 2, 0), (4, 6, 7, 40), (1, 1, 1, 1)):
        padded = np.pad(blob, ((top, bottom), (left, right)))
        for r0, c0 in ((5 - top, 6 - left), (0, 0), (60 - padded.shape[0], 70 - padded.shape[1])):
            row, f = row_of(padded, (r0, c0), (60, 70))
            assert np.array_equal(f, np.pad(S, ((top, bottom), (left, right))))
            for name in FIELDS[:8] + ('reserved',):
                assert row[name] == base[name], name
            assert (row['first_row'] - (r0 + top), row['first_col'] - (c0 + left)) == (base['first_row'] - 5, base['first_col'] - 6)
            touches = r0 + top == 0 or c0 + left == 0 or r0 + top + blob.shape[0] == 60 or c0 + left + blob.shape[1] == 70
            assert row['flags'] == int(touches)


# ---- arguments -----------------------------------------------------------------------------------------------------------------------------
def test_every_argument_error():
    from superdsm_amd import skeleton as sk
    with pytest.raises(ValueError):
        sk.skeleton_objects_host([Obj((7, 7), np.ones((3, 3)))], (9, 9))               # leaves its image
    with pytest.raises(ValueError):
        sk.skeleton_objects_host([Obj((-1, 0), np.ones((3, 3)))], (9, 9))
    with pytest.raises(ValueError):
        sk.skeleton_objects_host([], (0, 9))
    with pytest.raises(ValueError):
        sk.skeleton_objects_host([], (70000, 9))
    with pytest.raises(TypeError):
        sk.skeleton_labels_host(np.zeros((4, 4)))                                      # a float map
    with pytest.raises(TypeError):
        sk.skeleton_labels_host(np.zeros((4, 4, 2), np.int32))
    with pytest.raises(ValueError, match='labels'):
        sk.skeleton_labels_host(np.array([[0, -1]]))
    with pytest.raises(ValueError, match='labels'):
        sk.skeleton_labels_host(np.array([[0, 65536]]))
    with pytest.raises(ValueError):
        sk.thin_host(np.ones((2, 2, 2), bool))
    with pytest.raises(ValueError):
        sk.thin_stack(np.ones((2, 2), bool))


def test_the_workspace_helper_at_the_limits():
    from superdsm_amd import _capi, skeleton as sk
    ws, cap = _capi.lib().sdsm_skeleton_workspace_words, _capi.SKELETON_LDS_WORDS
    assert cap == 3072
    assert (ws(64, 64), ws(65, 64), ws(64, 65), ws(cap, 64), ws(cap + 1, 64), ws(cap // 2, 128), ws(cap // 2, 129), ws(cap // 2 + 1, 128)) == \
        (0, 0, 0, 0, 2 * (cap + 1), 0, 2 * 3 * (cap // 2), 2 * 2 * (cap // 2 + 1))
    assert (ws(0, 5), ws(5, 0), ws(-1, -1), ws(65535, 32768)) == (0, 0, 0, 2 * 65535 * 512)
    boxes = [(0, 0, 64, 64), (0, 0, 65, 64), (1, 2, cap + 1, 3), (0, 0, 200, 2000), (0, 0, 96, 2048), (0, 0, 97, 2048)]
    assert sk.workspace_words(boxes).tolist() == [ws(b[2], b[3]) for b in boxes] and sk.path_of(boxes).tolist() == [0, 1, 2, 2, 1, 2]


# ---- derived columns and the CSV -----------------------------------------------------------------------------------------------------------
def test_derive_on_hand_computed_rows():
    from superdsm_amd import skeleton as sk
    table = np.zeros(4, sk.TABLE_DTYPE)
    table['label'] = [3, 4, 9, 11]
    table[0] = (3, 72, 20, 0, 0, 0, 16, 4, 2, 3, 4, 0, 0)                     # the ring of the anchors
    table[1] = (4, 185, 35, 4, 0, 1, 34, 0, 2, 4, 12, 1, 0)                   # the plus, on the frame
    table[3] = (11, 1, 1, 0, 1, 0, 0, 0, 0, 7, 7, 0, 0)                       # one pixel
    d = sk.derive(table)
    assert d.dtype == sk.DERIVED_DTYPE and d['label'].tolist() == [3, 4, 9, 11] and d['on_boundary'].tolist() == [False, True, False, False]
    assert d['length'][0] == 16 + math.sqrt(2) * 4 and d['mean_width'][0] == 72 / 20 and (d['ends'][0], d['branch_pixels'][0]) == (0, 0)
    assert d['length'][1] == 34.0 and d['mean_width'][1] == 185 / 35 and (d['ends'][1], d['branch_pixels'][1], d['skeleton_pixels'][1]) == (4, 1, 35)
    assert d['area'][2] == 0 and np.isnan(d['length'][2]) and np.isnan(d['mean_width'][2]) and d['ends'][2] == 0
    assert d['length'][3] == 0.0 and d['mean_width'][3] == 1.0


def test_csv_round_trip(tmp_path):
    from superdsm_amd import skeleton as sk
    t = np.zeros((20, 31), bool)
    t[2:7, 1:30] = t[2:19, 13:18] = True
    table, _ = sk.skeleton_objects_host([Obj((0, 0), t), Obj((25, 3), np.eye(9, dtype=bool)), Obj((30, 30), np.zeros((2, 2)))], (40, 40))
    sk.write_skeleton_csv(tmp_path / 'skeleton.csv', table)
    text = open(tmp_path / 'skeleton.csv').read()
    assert all(field.startswith('"') and field.endswith('"') for line in text.splitlines() for field in line.split(','))
    rows = list(csv.reader(open(tmp_path / 'skeleton.csv')))
    d = sk.derive(table)
    assert len(rows) == 4 and rows[0][:len(d.dtype.names)] == list(d.dtype.names) and len(set(rows[0])) == len(rows[0])
    col = {name: i for i, name in enumerate(rows[0])}
    for k in range(3):
        for name in d.dtype.names:
            v = eval(rows[k + 1][col[name]], {'nan': math.nan, 'inf': math.inf})
            assert v == d[name][k] or (v != v and d[name][k] != d[name][k]), (k, name)
        for name in FIELDS[1:]:
            assert int(rows[k + 1][col[name]]) == table[name][k]
    assert d['length'][1] == math.sqrt(2) * 8 and table['n_end'][1] == 2


# ---- the host code alone under the sanitizers --------------------------------------------------------------------------------------------------
def test_the_host_helpers_alone_under_the_sanitizers(tmp_path):
    """tests/host/skeleton_check.cpp with sdsm_host.cpp as host code only, AddressSanitizer and UndefinedBehaviorSanitizer linked into the
    executable (as tests/test_depth_cpu.py builds its program).  No GPU; a failing compile fails the test."""
    from superdsm_amd import skeleton as sk
    rng = np.random.default_rng(8)
    masks = [rng.random((h, w)) < 0.8 for h, w in ((1, 1), (5, 31), (7, 33), (3, 64), (9, 65), (4, 129), (70, 3), (66, 66))]
    with open(tmp_path / 'cases.txt', 'w') as fp:
        for m in masks:
            fp.write(f'{m.shape[0]} {m.shape[1]} ' + ''.join('1' if v else '0' for v in m.reshape(-1)) + '\n')
    prog = tmp_path / 'skeleton_check'
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    build = subprocess.run([hipcc, '-x', 'hip', '--offload-host-only', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                            '-o', str(prog),
                            os.path.join(ROOT, 'tests', 'host', 'skeleton_check.cpp'), os.path.join(ROOT, 'superdsm_amd', 'csrc', 'sdsm_host.cpp')],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(prog), str(tmp_path / 'cases.txt')], capture_output=True, text=True, timeout=120)
    assert (run.returncode, run.stderr) == (0, ''), (run.returncode, run.stderr)
    lines = run.stdout.splitlines()
    assert len(lines) == len(masks)
    for m, line in zip(masks, lines):
        S, cycles = sk.thin_host(m)
        assert line == f'{cycles} ' + ''.join('1' if v else '0' for v in S.reshape(-1))
