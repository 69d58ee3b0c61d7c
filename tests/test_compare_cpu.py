"""The host side of superdsm_amd/compare.py without a GPU: the contingency table against a double loop, its input errors, the scores
on cases worked by hand in an 8 x 8 image, and the driver that grows the tables of the GPU form, fed by a fake launch."""
import math

import numpy as np
import pytest


def brute_pairs(a, b):
    from superdsm_amd import compare
    rows = []
    for i in sorted(set(a.reshape(-1).tolist())):
        for j in sorted(set(b.reshape(-1).tolist())):
            n = int(((a == i) & (b == j)).sum())
            if n:
                rows.append((i, j, n))
    return np.array(rows, compare.PAIR_DTYPE)


# ---- the definition against brute force --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(17, 23), (1, 1)])
def test_host_table_equals_double_loop(shape):
    from superdsm_amd import compare
    rng = np.random.default_rng(shape[0])
    a, b = rng.integers(0, 7, shape), rng.integers(0, 5, shape).astype(np.uint16)
    got = compare.overlap_pairs_host(a, b)
    assert got.dtype == compare.PAIR_DTYPE and got.tobytes() == brute_pairs(a, b).tobytes()
    assert int(got['count'].sum()) == a.size
    assert (0 in got['a'] or shape == (1, 1)) and sorted(zip(got['a'].tolist(), got['b'].tolist())) == list(zip(got['a'].tolist(), got['b'].tolist()))


def test_empty_maps_give_an_empty_table():
    from superdsm_amd import compare
    got = compare.overlap_pairs_host(np.zeros((0, 5), np.int32), np.zeros((0, 5), np.int64))
    assert got.dtype == compare.PAIR_DTYPE and len(got) == 0


def test_input_errors():
    from superdsm_amd import compare
    ok = np.zeros((4, 4), np.int32)
    with pytest.raises(TypeError):
        compare.overlap_pairs_host(ok.astype(np.float64), ok)
    with pytest.raises(ValueError):
        compare.overlap_pairs_host(ok, np.zeros((4, 5), np.int32))
    with pytest.raises(ValueError):
        compare.overlap_pairs_host(ok[0], ok[0])
    neg = ok.copy()
    neg[1, 2] = -1
    with pytest.raises(ValueError):
        compare.overlap_pairs_host(ok, neg)
    big = ok.astype(np.int64)
    big[0, 0] = 2 ** 31
    with pytest.raises(ValueError):
        compare.overlap_pairs_host(big, ok)
    big[0, 0] = 2 ** 31 - 1                                                   # the largest label passes
    assert compare.overlap_pairs_host(big, ok)['a'].tolist() == [0, 2 ** 31 - 1]


# ---- scores, worked by hand ------------------------------------------------------------------------------------------------------------
def square(c0, c1, label=1, r0=0, r1=4):
    m = np.zeros((8, 8), np.int32)
    m[r0:r1, c0:c1] = label
    return m


def test_identical_maps():
    from superdsm_amd import compare
    m = square(0, 4) + square(5, 8, 2, 4, 8)
    s = compare.compare_labels_host(m, m)
    assert s['seg'] == 1.0 and (s['ap'] == 1.0).all() and s['mean_ap'] == 1.0 and len(s['ap']) == 10
    assert (s['precision'] == 1).all() and (s['recall'] == 1).all() and (s['f1'] == 1).all()
    assert (s['splits'], s['merges'], s['missed'], s['spurious']) == (0, 0, 0, 0)
    assert s['foreground_dice'] == 1.0 and s['foreground_jaccard'] == 1.0 and (s['n_actual'], s['n_expected']) == (2, 2)
    assert s['expected']['best'].tolist() == [1, 2] and s['expected']['jaccard'].tolist() == [1.0, 1.0]
    assert s['expected'].dtype == compare.EXPECTED_DTYPE and s['actual'].dtype == compare.ACTUAL_DTYPE


def test_overlap_of_a_third_is_no_match():
    from superdsm_amd import compare
    s = compare.compare_labels_host(square(2, 6), square(0, 4))
    e = s['expected'][0]
    assert (e['label'], e['area'], e['best'], e['intersection'], e['union']) == (1, 16, 1, 8, 24)
    assert e['jaccard'] == 1 / 3                                              # one division of 8 by 24
    assert e['seg_match'] == -1 and e['seg_jaccard'] == 0 and s['seg'] == 0   # 2 * 8 > 16 is false
    assert s['tp'][0] == 0 and s['thresholds'][0] == 0.5 and s['ap'][0] == 0 and (s['fp'][0], s['fn'][0]) == (1, 1)
    assert s['foreground_dice'] == 0.5 and s['foreground_jaccard'] == 1 / 3
    assert (s['missed'], s['spurious'], s['splits'], s['merges']) == (0, 0, 0, 0)


def test_overlap_of_three_fifths_matches_up_to_its_threshold():
    from superdsm_amd import compare
    s = compare.compare_labels_host(square(1, 5), square(0, 4))
    e, a = s['expected'][0], s['actual'][0]
    assert (e['intersection'], e['union'], e['jaccard']) == (12, 20, 0.6)
    assert e['seg_match'] == 1 and e['seg_jaccard'] == 0.6 and s['seg'] == 0.6
    assert (a['best'], a['intersection'], a['union'], a['seg_match'], a['n_merged']) == (1, 12, 20, 1, 1)
    assert s['tp'].tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0, 0]                 # 0.5, 0.55, 0.6 | 0.65 ...: 12 * 5 >= 3 * 20 in integers
    assert s['mean_ap'] == pytest.approx(0.3)
    # the thresholds as arithmetic hands them over (0.6000000000000001) decide the same
    assert compare.compare_labels_host(square(1, 5), square(0, 4), thresholds=np.arange(0.5, 1.0, 0.05))['tp'].tolist() == s['tp'].tolist()


def test_split_and_merge():
    from superdsm_amd import compare
    whole, halves = square(0, 4), square(0, 2, 1) + square(2, 4, 2)
    s = compare.compare_labels_host(halves, whole)
    assert s['splits'] == 1 and s['merges'] == 0 and s['expected']['n_split'].tolist() == [2]
    assert s['expected']['best'][0] == 1                                      # the tie of 8 against 8 goes to the smaller label
    assert s['expected']['seg_match'][0] == -1 and s['actual']['n_merged'].tolist() == [0, 0]
    assert s['actual']['seg_match'].tolist() == [1, 1]
    m = compare.compare_labels_host(whole, halves)
    assert m['merges'] == 1 and m['splits'] == 0 and m['actual']['n_merged'].tolist() == [2] and m['expected']['n_split'].tolist() == [0, 0]


def test_missed_spurious_and_no_objects():
    from superdsm_amd import compare
    s = compare.compare_labels_host(np.zeros((8, 8), np.int32), square(0, 4))
    assert s['missed'] == 1 and s['spurious'] == 0 and s['expected']['best'].tolist() == [-1] and s['expected']['jaccard'].tolist() == [0.0]
    assert s['seg'] == 0 and s['recall'][0] == 0 and math.isnan(s['precision'][0]) and math.isnan(s['foreground_dice']) is False
    t = compare.compare_labels_host(square(0, 4), np.zeros((8, 8), np.int32))
    assert t['spurious'] == 1 and t['missed'] == 0 and math.isnan(t['seg']) and t['n_expected'] == 0 and len(t['expected']) == 0
    assert math.isnan(t['recall'][0]) and t['precision'][0] == 0
    z = compare.compare_labels_host(np.zeros((8, 8), np.int32), np.zeros((8, 8), np.int32))
    assert math.isnan(z['seg']) and math.isnan(z['ap'][0]) and math.isnan(z['mean_ap']) and math.isnan(z['foreground_dice'])


def test_background_label_and_thresholds():
    from superdsm_amd import compare
    with pytest.raises(ValueError):
        compare.compare_labels_host(square(0, 4), square(0, 4), thresholds=(0.4, 0.5))
    s = compare.compare_labels_host(square(0, 4) + 1, square(0, 4) + 1, background_label=1)     # labels 1 (background) and 2
    assert s['n_expected'] == 1 and s['expected']['label'].tolist() == [2] and s['seg'] == 1


def test_scores_csv(tmp_path):
    import csv
    from superdsm_amd import compare
    s = compare.compare_labels_host(square(0, 2, 1) + square(2, 4, 2), square(0, 4))
    compare.write_scores_csv(tmp_path / 's.csv', s)
    rows = list(csv.reader(open(tmp_path / 's.csv')))
    assert rows[0][:3] == ['table', 'label', 'area'] and rows[0][-2:] == ['n_split', 'n_merged'] and len(rows) == 4
    assert rows[1][0] == 'expected' and rows[1][-2:] == ['2', ''] and rows[2][0] == 'actual' and rows[2][-2:] == ['', '0']


# ---- the driver of the GPU form, with a fake launch ----------------------------------------------------------------------------------
def test_tables_grow_for_the_overflowed_images_alone():
    from superdsm_amd import compare
    calls = []

    def fake(indices, capacities):
        """Image 1 overflows until its table has 64 slots; images 0 and 2 hold two pairs from the start."""
        calls.append((list(indices), list(capacities)))
        out = []
        for i, cap in zip(indices, capacities):
            keys, counts = np.full(cap, 0xffffffffffffffff, np.uint64), np.zeros(cap, np.int64)
            keys[[1, cap - 1]], counts[[1, cap - 1]] = [(7 << 32) | i, 3], [10 + i, 5]
            out.append((keys, counts, np.array([0, 1 if (i == 1 and cap < 64) else 0], np.int32)))
        return out

    tables, caps = compare.grow_tables(fake, 3, 8)
    assert calls == [([0, 1, 2], [8, 8, 8]), ([1], [16]), ([1], [32]), ([1], [64])]
    assert caps == [8, 64, 8]
    for i, (keys, counts) in enumerate(tables):
        assert sorted(zip(keys.tolist(), counts.tolist())) == [(3, 5), ((7 << 32) | i, 10 + i)]
    p = compare._pairs_from_keys(*tables[2])
    assert p.tolist() == [(0, 3, 5), (7, 2, 12)]


def test_a_table_more_than_half_full_is_grown_and_negative_labels_raise():
    from superdsm_amd import compare
    calls = []

    def fake(indices, capacities):
        calls.append(list(capacities))
        out = []
        for cap in capacities:
            keys, counts = np.full(cap, 0xffffffffffffffff, np.uint64), np.ones(cap, np.int64)
            keys[:5] = np.arange(5)
            out.append((keys, counts, np.zeros(2, np.int32)))
        return out

    tables, caps = compare.grow_tables(fake, 1, 8)                            # 5 pairs: 8 slots are more than half full, 16 are not
    assert calls == [[8], [16]] and caps == [16] and tables[0][0].tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match=r"3 pixels of images \['second'\]"):
        compare.grow_tables(lambda idx, caps: [(np.zeros(0, np.uint64), np.zeros(0, np.int64), np.array([3 * i, 0], np.int32)) for i in idx], 2, 8,
                            names=['first', 'second'])


def test_gpu_form_checks_its_arguments_before_any_launch():
    from superdsm_amd import compare
    ok = np.zeros((4, 4), np.int32)
    with pytest.raises(ValueError):
        compare.overlap_pairs(ok, ok, capacity=12)
    with pytest.raises(TypeError):
        compare.overlap_pairs(ok.astype(float), ok)
    with pytest.raises(ValueError):
        compare.overlap_pairs(ok, np.zeros((4, 5), np.int32))
    assert compare.overlap_pairs(np.zeros((0, 5), np.int32), np.zeros((0, 5), np.int32)).tobytes() == b''
    import superdsm_amd
    assert superdsm_amd.compare is compare
