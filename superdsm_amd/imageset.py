"""A set of images on the host: the packed layout every ``*_multi`` entry point takes (``sdsm_set_image``, include/sdsm.h) and the
split of a list into sets.  NumPy and ctypes only: neither PyTorch nor the shared library is needed here."""
import numpy as np

from . import _capi


def in_sets(n):
    """The slices that cut a list of ``n`` images into sets of at most ``_capi.MAX_SET_IMAGES``."""
    return [slice(lo, lo + _capi.MAX_SET_IMAGES) for lo in range(0, n, _capi.MAX_SET_IMAGES)]


class SetLayout:
    """The packed layout of one set of 1 .. ``_capi.MAX_SET_IMAGES`` images of the given ``(H, W)`` shapes: image i starts at element
    ``offsets[i]``, a multiple of ``align``, of a buffer of ``total`` elements; ``table`` is the ``_capi.SetImage`` array of the calls."""

    def __init__(self, shapes, align=64):
        self.shapes = [(int(h), int(w)) for h, w in shapes]
        if not 1 <= len(self.shapes) <= _capi.MAX_SET_IMAGES:
            raise ValueError(f'a set holds 1 .. {_capi.MAX_SET_IMAGES} images')
        self.table = (_capi.SetImage * len(self.shapes))()
        self.total = 0
        for entry, (h, w) in zip(self.table, self.shapes):
            entry.offset, entry.H, entry.W = self.total, h, w
            self.total += (h * w + align - 1) // align * align
        self.offsets = np.array([entry.offset for entry in self.table], np.int64)

    def pack(self, arrays, dtype, channels=1):
        """One zero-padded buffer with the images (H x W, or H x W x ``channels``) at their places."""
        flat = np.zeros(self.total * channels, dtype)
        for o, (h, w), a in zip(self.offsets, self.shapes, arrays):
            flat[o * channels:(o + h * w) * channels] = np.asarray(a).reshape(-1)
        return flat

    def unpack(self, flat, channels=1, tail=()):
        """The images of a packed buffer with ``channels`` values per pixel, each a copy of shape ``(H, W) + tail``."""
        return [flat[channels * o:channels * (o + h * w)].reshape((h, w) + tuple(tail)).copy() for o, (h, w) in zip(self.offsets, self.shapes)]
