"""The device-side fragment guard of the object kernels (k_measure_objects, k_shape_objects, k_intensity_objects, k_texture): an object
whose box leaves its image gets the kernel's empty result and nothing is read for it.  The Python layer refuses such boxes, so the raw
``*_objects_multi`` entries are called, as the ``objects_gpu_raw`` helpers of the families' own tests do.  Every box is chosen so that a
kernel without the guard would still read inside the packed buffers -- the neighbouring image or the next row -- and give wrong bytes,
not a fault.  (An image index out of range is not tested: without the guard it would index the set passed by value out of bounds.)"""
import numpy as np
import pytest

from test_measure_cpu import Obj

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8), (9, 5), (8, 8)]                # all objects lie in the middle image
SOUND = Obj((3, 1), np.ones((3, 3)))
OUTSIDE = [Obj((-1, 1), np.ones((3, 3))),        # one row above the image
           Obj((3, -1), np.ones((3, 3))),        # one column to its left
           Obj((7, 1), np.ones((3, 3))),         # one row below
           Obj((3, 3), np.ones((3, 3))),         # one column to its right
           Obj((0, 1), np.ones((10, 3)))]        # h > H
OBJECTS = [SOUND] + OUTSIDE
NAN_BITS, INF, EDGES = 0x7ff8000000000000, float('inf'), np.linspace(-150, 150, 7)


@pytest.fixture(scope='module')
def images():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    rng = np.random.default_rng(7)
    return [rng.normal(size=s) * 100 for s in SHAPES]


def packed_objects():
    from superdsm_amd.postprocess import pack_fragments
    boxes, words, packed, _ = pack_fragments(OBJECTS)
    return np.ones(len(boxes), np.int32), boxes, words, packed


def check(recs, host_row, empty, what):
    """Row 0 equals the host definition's row, the others the literal empty record, field by field and byte for byte."""
    for name in recs.dtype.names:
        assert recs[name][:1].tobytes() == host_row[name][:1].tobytes(), f'{what}: field {name} of the sound object: {recs[name][0]!r} != {host_row[name][0]!r}'
        want = np.full(len(OUTSIDE), empty[name], recs.dtype[name])
        assert recs[name][1:].tobytes() == want.tobytes(), f'{what}: field {name} of the boxes outside: {recs[name][1:]!r} != {empty[name]!r}'


def test_measure_objects(images):
    from superdsm_amd import measure
    recs = measure._MeasureSet(SHAPES, images).objects(*packed_objects())
    host = measure.measure_objects_host([SOUND], SHAPES[1], images[1])
    # write_record of a cleared accumulator: area == 0, so every integer is 0 but scale_exp, which is that of the record's image
    empty = dict.fromkeys(recs.dtype.names, 0)
    empty.update(scale_exp=measure.scale_exponent(images[1]), gmin=INF, gmax=-INF)
    assert empty['scale_exp'] != 0
    check(recs, host, empty, 'measure')


def test_shape_objects(images):
    from superdsm_amd import shape as sh
    recs, offsets, vertices = sh._ShapeSet(SHAPES).objects(*packed_objects())
    host, host_offsets, host_vertices = sh.shape_objects_host([SOUND], SHAPES[1])
    check(recs, host, dict.fromkeys(recs.dtype.names, 0), 'shape')               # zero_record
    nv = int(host_offsets[-1])
    assert offsets.tolist() == [0] + [nv] * len(OBJECTS) and vertices.tobytes() == np.asarray(host_vertices, vertices.dtype).tobytes()


def test_intensity_objects(images):
    from superdsm_amd import intensity as it
    fracs = it.quantile_fractions(it.DEFAULT_QUANTILES)
    recs, order = it._IntensitySet(SHAPES, images).objects(*packed_objects(), fracs)
    host, host_order = it.intensity_objects_host([SOUND], SHAPES[1], images[1], it.DEFAULT_QUANTILES)
    # empty_result(out, order, n_q, 0, 0)
    nan = np.array([NAN_BITS], np.uint64).view(np.float64)[0]
    empty = dict(area=0, n_finite=0, sum_p=0, sum_pp_lo=0, sum_pp_hi=0, gmin=INF, gmax=-INF, med_lo=nan, med_hi=nan, mad_lo=nan, mad_hi=nan, range_exp=0, flags=4)
    check(recs, host, empty, 'intensity')
    assert order[:1].tobytes() == np.asarray(host_order, np.float64).tobytes()
    assert (order[1:].view(np.uint64) == NAN_BITS).all()


def test_texture_objects(images):
    from superdsm_amd import texture as tx
    offs = tx.check_offsets(tx.DEFAULT_OFFSETS)
    recs, pairs, entries = tx._TextureSet(SHAPES, images, [tx.check_edges(EDGES)] * 3, offs).objects(*packed_objects())
    host, host_pairs, host_entries = tx.texture_objects_host([SOUND], SHAPES[1], images[1], EDGES)
    # empty_result(out, P, o == 0, levels, 0, 0)
    check(recs, host, dict(area=0, n_finite=0, level_min=len(EDGES) + 1, level_max=-1, flags=4, reserved=0), 'texture')
    assert host_pairs['n_pairs'].sum() > 0 and entries.tobytes() == host_entries.tobytes()
    for name in ('n_pairs', 'n_entries', 'reserved'):
        assert pairs[name][:1].tobytes() == host_pairs[name].tobytes() and not pairs[name][1:].any(), name
    first = np.concatenate([[0], np.cumsum(pairs['n_entries'].reshape(-1))[:-1]]).reshape(pairs.shape)          # (k_texture_scan's)
    assert pairs['first'].tolist() == first.tolist()
