"""What the five table families that take packed objects and label windows -- measure, shape, intensity, texture, depth -- share in front
of their GPU forms: the checks of ``*_objects_many`` and ``*_labels_many`` raise before anything touches the device, so they are tested
here without one."""
import numpy as np
import pytest

from test_measure_cpu import Obj

G = np.zeros((8, 8))
# family: (objects_many(objects_per_image, shapes), labels_many(labels_list)) with the family's other arguments filled in
FAMILIES = {
    'measure': (lambda m, objs, shapes: m.measure_objects_many(objs, shapes), lambda m, labels: m.measure_labels_many(labels)),
    'shape': (lambda m, objs, shapes: m.shape_objects_many(objs, shapes), lambda m, labels: m.shape_labels_many(labels)),
    'intensity': (lambda m, objs, shapes: m.intensity_objects_many(objs, shapes, [G] * len(shapes)),
                  lambda m, labels: m.intensity_labels_many(labels, [G] * len(labels))),
    'texture': (lambda m, objs, shapes: m.texture_objects_many(objs, shapes, [G] * len(shapes), [[0.5]] * len(shapes)),
                lambda m, labels: m.texture_labels_many(labels, [G] * len(labels), [[0.5]] * len(labels))),
    'depth': (lambda m, objs, shapes: m.depth_objects_many(objs, shapes), lambda m, labels: m.depth_labels_many(labels)),
}


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_the_many_forms_check_their_lists_before_the_device(family):
    import importlib
    module = importlib.import_module('superdsm_amd.' + family)
    objects_many, labels_many = FAMILIES[family]
    inside, leaving = Obj((1, 1), np.ones((3, 3), bool)), Obj((6, 6), np.ones((3, 3), bool))
    with pytest.raises(ValueError, match='shapes'):
        objects_many(module, [[inside]], [(8, 8), (8, 8)])                   # one list of objects, two shapes
    with pytest.raises(ValueError, match='shapes'):
        objects_many(module, [[inside], [inside]], [(8, 8)])
    with pytest.raises(ValueError, match='outside its image'):
        objects_many(module, [[inside], [inside, leaving]], [(8, 8), (8, 8)])
    with pytest.raises(TypeError, match='integer'):
        labels_many(module, [np.zeros((8, 8), np.int32), np.zeros((8, 8))])      # the second label map holds floats
