"""Texture tables: the grey-level co-occurrence matrix (GLCM) of every object of a segmentation and its Haralick features, from objects
(bit-packed fragments, which may overlap; each is measured alone) or from label maps, for one image or a set of images.

:mod:`measure`, :mod:`shape` and :mod:`intensity` see the size, the outline and the histogram of an object; none of them sees how the
intensities are ARRANGED inside it.  As there, a result holds EXACT integers, the GPU forms (sdsm_texture.hip) give the bytes of the
``*_host`` definitions below, and every float is made in ONE place, :func:`derive`.

**Grey levels.**  The caller gives ``edges``: G - 1 strictly increasing finite float64 values, 1 <= G <= ``_capi.TEXTURE_MAX_LEVELS``.
The level of a finite pixel g is the number of edges <= g (``np.searchsorted(edges, g, side='right')``): comparisons only, -0.0 compares
as 0.0.  A non-finite pixel has no level, takes part in no pair and sets flag bit 1.  G = 1 (no edges): every finite pixel has level 0.
:func:`uniform_edges` and :func:`image_edges` make equally wide levels.  Levels are counted from 0.

**Offsets.**  1 .. ``_capi.TEXTURE_MAX_OFFSETS`` integer pairs (d_row, d_col), none (0, 0), max(|d_row|, |d_col|) <=
``_capi.TEXTURE_MAX_REACH``, none twice and none together with its negative (they give the same table).

**Counts.**  For object k and offset o every pixel p contributes one pair when p and p + o both lie in the object (label form: carry the
same label) and both are finite; with a = level(p), b = level(p + o) the pair adds 1 to the cell (min(a, b), max(a, b)).  The table holds
these UNORDERED counts c(i, j), i <= j, each below 2^31.  The symmetric GLCM of the literature is P(i, j) = P(j, i) = c(i, j) off the
diagonal and 2 c(i, i) on it; its total is 2 n_pairs.

A result is ``(table, pairs, entries)``:

  table[k]       ``sdsm_texture_record`` and ``label``: area, n_finite, level_min, level_max (G and -1 without a finite pixel), flags (bit 0:
                 the bounding box of the pixels touches the image frame; bit 1: a non-finite pixel inside; bit 2: no finite pixel)
  pairs[k, o]    n_pairs (int64), first (int64), n_entries (int32)
  entries        entries[first : first + n_entries] are the non-zero cells of (k, o) as (i: uint16, j: uint16, count: uint32) in ascending
                 (i, j) order; the list is compact: objects and offsets follow each other in order, ``first`` is the running sum of
                 ``n_entries``.

Parity with scikit-image's ``graycoprops``, mahotas' ``haralick`` and CellProfiler's ``MeasureTexture`` is NOT pinned: none of them is
available to the tests (DESIGN.md section 8 lists the known differences)."""
import csv
from functools import partial

import numpy as np

from . import _capi
from .measure import (_check_labels, _check_shape, _keep_absent, _label_count, _label_sets, _label_table, _LabelWindows, _MeasureSet, _object_boxes,
                      _object_sets, _require_intensity, _result_inputs)
from .postprocess import _check_boxes, _exclusive

TABLE_DTYPE = np.dtype([('label', 'i4')] + _capi._TEXTURE_FIELDS)   # 'label': the label, or the index of the object in its image
PAIRS_DTYPE = _capi.TEXTURE_PAIRS_DTYPE
ENTRY_DTYPE = _capi.TEXTURE_ENTRY_DTYPE
POOLED_ENTRY_DTYPE = np.dtype([('i', 'u2'), ('j', 'u2'), ('count', 'u8')])           # the counts of several offsets added
DEFAULT_OFFSETS = ((0, 1), (1, 1), (1, 0), (1, -1))
DEFAULT_LEVELS = 8
FRAME, NONFINITE_INSIDE, NO_FINITE_PIXEL = 1, 2, 4                                  # the flag bits


# ---- levels and offsets ------------------------------------------------------------------------------------------------------------------
def check_edges(edges):
    """``edges`` as a float64 array: G - 1 finite, strictly increasing values, G <= ``_capi.TEXTURE_MAX_LEVELS``."""
    e = np.asarray(edges if edges is not None else [], np.float64)
    if e.ndim != 1:
        raise ValueError(f'edges: a list of values; got {e.ndim} dimensions')
    if len(e) + 1 > _capi.TEXTURE_MAX_LEVELS:
        raise ValueError(f'{len(e)} edges make {len(e) + 1} levels: the texture tables take up to {_capi.TEXTURE_MAX_LEVELS}, see DESIGN.md "Limits"')
    if not np.isfinite(e).all() or not (e[1:] > e[:-1]).all():
        raise ValueError('edges: finite and strictly increasing values required')
    return np.ascontiguousarray(e)


def _edges_many(edges_list, n):
    edges_list = [check_edges(e) for e in edges_list]
    if len(edges_list) != n:
        raise ValueError('edges: one list per image')
    if len(frozenset(len(e) for e in edges_list)) > 1:
        raise ValueError('edges: the lists of one call have the same length (the same number of levels)')
    return edges_list


def check_offsets(offsets):
    """``offsets`` as a list of (d_row, d_col) of Python integers, checked."""
    offs = []
    for o in offsets:
        o = tuple(o)
        if len(o) != 2 or any(int(v) != v for v in o):
            raise ValueError(f'offset {o}: a pair of integers (d_row, d_col) required')
        offs.append((int(o[0]), int(o[1])))
    if not 1 <= len(offs) <= _capi.TEXTURE_MAX_OFFSETS:
        raise ValueError(f'{len(offs)} offsets: the texture tables take 1 .. {_capi.TEXTURE_MAX_OFFSETS} per call, see DESIGN.md "Limits"')
    for k, (dr, dc) in enumerate(offs):
        if (dr, dc) == (0, 0) or max(abs(dr), abs(dc)) > _capi.TEXTURE_MAX_REACH:
            raise ValueError(f'offset {(dr, dc)}: not (0, 0), and max(|d_row|, |d_col|) <= {_capi.TEXTURE_MAX_REACH} required')
        if (dr, dc) in offs[:k] or (-dr, -dc) in offs[:k]:
            raise ValueError(f'offset {(dr, dc)}: listed twice, or together with its negative (they give the same table)')
    return offs


def uniform_edges(lo, hi, levels):
    """The edges of ``levels`` equally wide levels between lo and hi: lo + (hi - lo) * (k / levels), k = 1 .. levels - 1."""
    levels = int(levels)
    if not 1 <= levels <= _capi.TEXTURE_MAX_LEVELS:
        raise ValueError(f'{levels} levels: 1 .. {_capi.TEXTURE_MAX_LEVELS} required')
    with np.errstate(over='ignore', invalid='ignore'):
        e = np.float64(lo) + (np.float64(hi) - np.float64(lo)) * (np.arange(1, levels) / levels)
    if not np.isfinite(e).all() or not (e[1:] > e[:-1]).all():
        raise ValueError(f'the range {lo!r} .. {hi!r} is too narrow (or not finite) for {levels} strictly increasing levels')
    return e


def image_edges(image, levels):
    """:func:`uniform_edges` over the finite minimum and maximum of an image."""
    g = np.asarray(image, np.float64)
    fin = g[np.isfinite(g)]
    if int(levels) == 1:
        return uniform_edges(0.0, 0.0, 1)
    if len(fin) == 0:
        raise ValueError('image_edges: the image has no finite pixel')
    return uniform_edges(fin.min(), fin.max(), levels)


def levels_of(values, edges):
    """The level of every value; -1 for a non-finite one."""
    v = np.asarray(values, np.float64)
    return np.where(np.isfinite(v), np.searchsorted(edges, v, side='right'), -1).astype(np.int64)


# ---- the definitions: NumPy and Python integers ---------------------------------------------------------------------------------------
def _empty_records(n, levels):
    recs = np.zeros(n, _capi.TEXTURE_RECORD_DTYPE)
    recs['level_min'], recs['level_max'], recs['flags'] = levels, -1, NO_FINITE_PIXEL
    return recs


def _fill(rec, frag, r0, c0, shape, g, edges, offs):
    """The record of the pixels ``frag`` (a boolean window whose corner is (r0, c0)) and per offset (n_pairs, i, j, count) of its cells."""
    G = len(edges) + 1
    none = [(0, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)) for _ in offs]
    rr, cc = np.nonzero(frag)
    if len(rr) == 0:
        return none
    h, w = frag.shape
    rec['area'] = len(rr)
    flags = FRAME * int(rr.min() + r0 == 0 or cc.min() + c0 == 0 or rr.max() + r0 + 1 == shape[0] or cc.max() + c0 + 1 == shape[1])
    lev = np.where(frag, levels_of(g[r0:r0 + h, c0:c0 + w], edges), -1)            # -1: not a finite pixel of the object
    fin = lev >= 0
    n = int(fin.sum())
    flags |= NONFINITE_INSIDE * int(n != len(rr))
    if n == 0:
        rec['flags'] = flags | NO_FINITE_PIXEL
        return none
    rec['n_finite'], rec['level_min'], rec['level_max'], rec['flags'] = n, lev[fin].min(), lev[fin].max(), flags
    out = []
    for dr, dc in offs:
        if abs(dr) >= h or abs(dc) >= w:
            out.append(none[0])
            continue
        a = lev[max(0, -dr):h - max(0, dr), max(0, -dc):w - max(0, dc)]            # p
        b = lev[max(0, dr):h - max(0, -dr), max(0, dc):w - max(0, -dc)]            # p + o
        ok = (a >= 0) & (b >= 0)
        i, j = np.minimum(a[ok], b[ok]), np.maximum(a[ok], b[ok])
        key, count = np.unique(i * G + j, return_counts=True)                      # ascending (i, j)
        out.append((int(ok.sum()), key // G, key % G, count.astype(np.int64)))
    return out


_table = partial(_label_table, TABLE_DTYPE)                         # _table(labels, recs)


def _assemble(labels, recs, cells, n_o):
    """(table, pairs, entries) from the records and per row the cells of :func:`_fill`."""
    pairs = np.zeros((len(recs), n_o), PAIRS_DTYPE)
    for k, row in enumerate(cells):
        for o, (n_pairs, i, j, count) in enumerate(row):
            pairs[k, o]['n_pairs'], pairs[k, o]['n_entries'] = n_pairs, len(i)
    pairs['first'] = _exclusive(pairs['n_entries'].reshape(-1)).reshape(pairs.shape)
    entries = np.zeros(int(pairs['n_entries'].sum()), ENTRY_DTYPE)
    flat = [c for row in cells for c in row]
    if len(entries):
        entries['i'], entries['j'], entries['count'] = (np.concatenate([c[f] for c in flat]) for f in (1, 2, 3))
    return _table(labels, recs), pairs, entries


def texture_objects_host(objects, shape, intensity, edges, offsets=DEFAULT_OFFSETS):
    """``(table, pairs, entries)`` of a list of objects (``fg_offset``, ``fg_fragment``) of an image of ``shape`` with the intensities
    ``intensity``, object by object; row k is object k.  Objects may overlap: each is measured alone."""
    shape = _check_shape(shape)
    objects = list(objects)
    _check_boxes(_object_boxes(objects), shape)
    g = _require_intensity(intensity, shape)
    edges, offs = check_edges(edges), check_offsets(offsets)
    recs = _empty_records(len(objects), len(edges) + 1)
    cells = [_fill(recs[k:k + 1], np.asarray(obj.fg_fragment, bool), int(obj.fg_offset[0]), int(obj.fg_offset[1]), shape, g, edges, offs)
             for k, obj in enumerate(objects)]
    return _assemble(np.arange(len(objects)), recs, cells, len(offs))


def texture_labels_host(labels, intensity, edges, offsets=DEFAULT_OFFSETS, background_label=0, keep_absent=False):
    """``(table, pairs, entries)`` of a label map, label by label: the present labels without ``background_label`` (None: all) in
    ascending order; with ``keep_absent`` one row per label 0 .. max, the empty row for an absent label and for the background label.  A
    pair counts only where both pixels carry the label."""
    labels = _check_labels(labels)
    g = _require_intensity(intensity, labels.shape)
    edges, offs = check_edges(edges), check_offsets(offsets)
    n = _label_count(labels)
    recs = _empty_records(n, len(edges) + 1)
    none = [(0, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)) for _ in offs]
    cells = [none] * n
    for l in sorted(frozenset(labels.reshape(-1).tolist())):
        if l != background_label:
            rr, cc = np.nonzero(labels == l)
            r0, c0 = int(rr.min()), int(cc.min())
            cells[l] = _fill(recs[l:l + 1], labels[r0:rr.max() + 1, c0:cc.max() + 1] == l, r0, c0, labels.shape, g, edges, offs)
    ls = np.arange(n) if keep_absent else np.nonzero(recs['area'] > 0)[0]
    return _assemble(ls, recs[ls], [cells[l] for l in ls], len(offs))


# ---- the tables of a result ----------------------------------------------------------------------------------------------------------------
def dense(pairs_row, entries, levels):
    """The symmetric ``levels`` x ``levels`` integer matrix P of one (k, o): ``pairs_row`` = ``pairs[k, o]``.  Its total is 2 n_pairs."""
    first, n = int(pairs_row['first']), int(pairs_row['n_entries'])
    e = entries[first:first + n]
    m = np.zeros((int(levels), int(levels)), np.int64)
    i, j, c = e['i'].astype(np.int64), e['j'].astype(np.int64), e['count'].astype(np.int64)
    np.add.at(m, (i, j), c)
    np.add.at(m, (j, i), c)                                                       # (twice on the diagonal)
    return m


def _owner(pairs):
    """Per entry the flat index k * n_offsets + o of its (object, offset)."""
    return np.repeat(np.arange(pairs.size, dtype=np.int64), pairs['n_entries'].reshape(-1))


def _grouped(key, weight):
    """The distinct keys in ascending order and the integer sum of the weights of each."""
    if len(key) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    order = np.argsort(key, kind='stable')
    ks = key[order]
    starts = np.concatenate([[0], np.flatnonzero(ks[1:] != ks[:-1]) + 1])
    return ks[starts], np.add.reduceat(weight[order].astype(np.int64), starts)


def pooled(pairs, entries):
    """The integer sum of the tables of all offsets of every object -- the direction-independent matrix -- in the same sparse form:
    ``(pairs, entries)`` with one column of ``pairs`` per object and 64-bit counts."""
    n, n_o = pairs.shape
    own = _owner(pairs) // max(1, n_o)
    key, count = _grouped((own << 32) | (entries['i'].astype(np.int64) << 16) | entries['j'].astype(np.int64), entries['count'])
    out = np.zeros((n, 1), PAIRS_DTYPE)
    out['n_pairs'][:, 0] = pairs['n_pairs'].sum(axis=1)
    out['n_entries'][:, 0] = np.bincount(key >> 32, minlength=n)[:n] if n else 0
    out['first'] = _exclusive(out['n_entries'].reshape(-1)).reshape(out.shape)
    e = np.zeros(len(key), POOLED_ENTRY_DTYPE)
    e['i'], e['j'], e['count'] = (key >> 16) & 0xffff, key & 0xffff, count
    return out, e


# ---- derived columns: one function for the host and the GPU forms ----------------------------------------------------------------------
FEATURES = ('asm', 'contrast', 'correlation', 'variance', 'idm', 'sum_average', 'sum_variance', 'sum_entropy', 'entropy', 'difference_variance',
            'difference_entropy', 'imc1', 'imc2', 'dissimilarity', 'energy', 'mean')       # Haralick's f1 .. f13, then the others
DERIVED_DTYPE = np.dtype([('label', 'i4'), ('d_row', 'i4'), ('d_col', 'i4'), ('area', 'i8'), ('n_finite', 'i8'), ('n_pairs', 'i8'), ('on_boundary', '?'),
                          ('nonfinite_inside', '?'), ('no_finite_pixel', '?')] + [(f, 'f8') for f in FEATURES])
U = 2.0 ** -53                                                                     # the unit roundoff of float64


def entropy_bound(terms, value):
    """The absolute error bound of an entropy of ``terms`` summands that :func:`derive` states: (terms + 8) 2^-53 value + 2^-51."""
    return (terms + 8) * U * value + 4 * U


def _quotient(num, den):
    """num / den of two arrays of Python integers, each quotient correctly rounded (``int.__truediv__``); NaN where den == 0."""
    return np.array([n / d if d else np.nan for n, d in zip(num.tolist(), den.tolist())], np.float64).reshape(num.shape)


def _row_sums(rows, values, R):
    """out[r] = the sum of values[rows == r]; ``rows`` ascending."""
    out = np.zeros(R, values.dtype)
    if len(rows):
        starts = np.concatenate([[0], np.flatnonzero(rows[1:] != rows[:-1]) + 1])
        out[rows[starts]] = np.add.reduceat(values, starts)
    return out


def _entropy(rows, counts, total, R):
    """Per row -sum q log2 q over its groups with q = counts / total[row] (bits), and the number of its summands."""
    with np.errstate(divide='ignore', invalid='ignore'):
        q = counts.astype(np.float64) / total[rows].astype(np.float64)
        t = -(q * np.log2(q))
    return _row_sums(rows, t, R) + 0.0, _row_sums(rows, np.ones(len(rows), np.int64), R)     # (-0.0 + 0.0 = +0.0)


def derive(table, pairs, entries, offsets=None):
    """The derived columns of a result (``DERIVED_DTYPE``), one row per object and offset (shape of ``pairs``), on the host from its exact
    integers; vectorised over the entry list.  ``offsets`` fills ``d_row`` / ``d_col`` (None: 0, as for a :func:`pooled` table).

    Notation: N = n_pairs, p = P / (2 N) the symmetric matrix as probabilities, levels from 0, p_x its marginal (= p_y), mu and sigma^2
    the mean and variance of p_x, p_{x+y}(k) and p_{x-y}(d) the distributions of i + j and |i - j|, entropies in bits.  With the integer
    sums over the entries c(i, j) of a row  A = sum (1 + [i = j]) c^2,  C = sum (j - i)^2 c,  D = sum (j - i) c,  M = sum (i + j) c,
    Q = sum (i^2 + j^2) c,  X = sum i j c,  K = sum (i + j)^2 c  (all below 2^63 for N < 2^31, which is required):

      asm (f1) = A / (2 N^2)           contrast (f2) = C / N            dissimilarity = D / N          sum_average (f6) = M / N
      mean mu = M / (2 N)              variance (f4) sigma^2 = (2 N Q - M^2) / (4 N^2)
      correlation (f3) = (4 N X - M^2) / (2 N Q - M^2), NaN where sigma^2 = 0
      sum_variance (f7) = (N K - M^2) / N^2, about the sum average (the corrected form, not the printed one)
      difference_variance (f10) = (N C - D^2) / N^2
    Each of these is ONE quotient of two Python integers, correctly rounded: within 0.5 ulp of the exact rational.  ``energy`` is the
    root of asm: within 1 ulp.

      idm (f5) = sum_d p_{x-y}(d) / (1 + d^2), p_{x-y}(d) = (sum_{j - i = d} c) / N: at most 256 non-negative summands, relative error
      below 260 * 2^-53.
      entropy (f9) HXY = -sum p log2 p over the cells of P; sum_entropy (f8) over p_{x+y}(k) = (sum_{i + j = k} c) / N;
      difference_entropy (f11) over p_{x-y}; HX over p_x(a) = (sum_{i = a} c + sum_{j = a} c) / (2 N).  A probability is one division of
      two integers below 2^53, log2 is taken to be within 1 ulp, the summands are non-negative and added one after the other: an entropy H
      of m summands is within E(m, H) = (m + 8) 2^-53 H + 2^-51 of the exact value (:func:`entropy_bound`); m is the number of entries
      (counting those off the diagonal twice) for f9, at most 2 G - 1 for f8 and G for f11 and HX.
      imc1 (f12) = (HXY - HXY1) / HX with HXY1 = -sum p(a, b) log2(p_x(a) p_y(b)), which for a symmetric matrix is exactly 2 HX: computed
      as (HXY - 2 HX) / HX, a value in -1 .. 0, within 1.01 (E_xy + 3 E_x) / HX + 2^-51; NaN where HX = 0.
      imc2 (f13) = sqrt(1 - 2^(-2 (HXY2 - HXY))) with HXY2 = 2 HX likewise (base 2, as the entropies are in bits); the argument of the root
      is clamped to 0 .. 1; within sqrt(1.4 (E_xy + 2 E_x) + 2^-48) + 2^-52.

    A row with n_pairs = 0 reads NaN throughout."""
    pairs = np.asarray(pairs)
    if pairs.ndim != 2 or pairs.shape[0] != len(table):
        raise ValueError(f'pairs: {len(table)} rows expected for this table, got the shape {pairs.shape}')
    n, n_o = pairs.shape
    if int(pairs['n_entries'].sum()) != len(entries):
        raise ValueError(f'entries: {int(pairs["n_entries"].sum())} expected for these pairs, got {len(entries)}')
    if n and pairs['n_pairs'].max() >= 2 ** 31:
        raise ValueError('n_pairs >= 2^31: derive forms its sums in 64-bit integers')
    out = np.zeros(pairs.shape, DERIVED_DTYPE)
    for f in FEATURES:
        out[f] = np.nan
    for name in ('label', 'area', 'n_finite'):
        out[name] = table[name][:, None]
    out['on_boundary'], out['nonfinite_inside'], out['no_finite_pixel'] = (((table['flags'] & b) != 0)[:, None] for b in (FRAME, NONFINITE_INSIDE, NO_FINITE_PIXEL))
    out['n_pairs'] = pairs['n_pairs']
    if offsets is not None:
        offs = check_offsets(offsets)
        if len(offs) != n_o:
            raise ValueError(f'offsets: {n_o} expected for these pairs, got {len(offs)}')
        out['d_row'], out['d_col'] = [o[0] for o in offs], [o[1] for o in offs]
    R = n * n_o
    if R == 0:
        return out
    N = pairs['n_pairs'].reshape(-1).astype(np.int64)
    rows = _owner(pairs)
    i, j, c = entries['i'].astype(np.int64), entries['j'].astype(np.int64), entries['count'].astype(np.int64)
    d = j - i
    A, Cs, D, M = (_row_sums(rows, v, R) for v in (np.where(d == 0, 2, 1) * c * c, d * d * c, d * c, (i + j) * c))
    Q, X, K = (_row_sums(rows, v, R) for v in ((i * i + j * j) * c, i * j * c, (i + j) * (i + j) * c))
    A, Cs, D, M, Q, X, K, No = (v.astype(object) for v in (A, Cs, D, M, Q, X, K, N))      # Python integers from here on
    F = {}
    F['asm'], F['contrast'], F['dissimilarity'], F['sum_average'] = _quotient(A, 2 * No * No), _quotient(Cs, No), _quotient(D, No), _quotient(M, No)
    F['mean'], F['variance'] = _quotient(M, 2 * No), _quotient(2 * No * Q - M * M, 4 * No * No)
    F['correlation'] = _quotient(4 * No * X - M * M, 2 * No * Q - M * M)
    F['sum_variance'], F['difference_variance'] = _quotient(No * K - M * M, No * No), _quotient(No * Cs - D * D, No * No)
    F['energy'] = np.sqrt(F['asm'])
    # the distributions: integer counts per (row, value), then one division each
    dk, dcount = _grouped(rows * 512 + d, c)
    with np.errstate(divide='ignore', invalid='ignore'):
        F['idm'] = _row_sums(dk // 512, dcount.astype(np.float64) / (1 + (dk % 512) ** 2).astype(np.float64), R) / N.astype(np.float64)
    F['difference_entropy'], _ = _entropy(dk // 512, dcount, N, R)
    sk, scount = _grouped(rows * 512 + i + j, c)
    F['sum_entropy'], _ = _entropy(sk // 512, scount, N, R)
    xk, xcount = _grouped(np.concatenate([rows * 512 + i, rows * 512 + j]), np.concatenate([c, c]))
    HX, _ = _entropy(xk // 512, xcount, 2 * N, R)
    off = d != 0                                                                   # the cells of P: those off the diagonal twice
    rows2 = np.concatenate([rows, rows[off]])
    order = np.argsort(rows2, kind='stable')
    HXY, _ = _entropy(rows2[order], np.concatenate([np.where(off, c, 2 * c), c[off]])[order], 2 * N, R)
    F['entropy'] = HXY
    with np.errstate(divide='ignore', invalid='ignore'):
        F['imc1'] = np.where(HX > 0, (HXY - 2 * HX) / HX, np.nan)
        F['imc2'] = np.sqrt(np.clip(1 - np.exp2(-2 * (2 * HX - HXY)), 0, 1))
    for f in FEATURES:
        out[f] = np.where(N > 0, F[f], np.nan).reshape(n, n_o)
    return out


def entropy_terms(pairs, entries):
    """Per (object, offset) the number of summands of (HXY, sum entropy, difference entropy, HX) in :func:`derive`, for its error bounds."""
    rows = _owner(pairs)
    i, j = entries['i'].astype(np.int64), entries['j'].astype(np.int64)
    R = pairs.size
    count = lambda key: np.bincount(np.unique(key) // 512, minlength=R)[:R]
    m_xy = np.bincount(rows, weights=np.where(i == j, 1, 2), minlength=R)[:R].astype(np.int64)
    return tuple(m.reshape(pairs.shape) for m in (m_xy, count(rows * 512 + i + j), count(rows * 512 + j - i), count(np.concatenate([rows * 512 + i, rows * 512 + j]))))


def write_texture_csv(path, table, pairs, entries, offsets=None):
    """A result with its derived columns as CSV, one line per object and offset, every field quoted (as
    ``measure.write_measurements_csv``); after the derived columns the exact ones: level_min, level_max, n_entries and ``cells``, the
    entries of the line as ``i:j:count`` separated by blanks."""
    d = derive(table, pairs, entries, offsets)
    with open(path, 'w', newline='') as fp:
        w = csv.writer(fp, delimiter=',', quoting=csv.QUOTE_ALL)
        w.writerow(list(d.dtype.names) + ['level_min', 'level_max', 'n_entries', 'cells'])
        for k in range(pairs.shape[0]):
            for o in range(pairs.shape[1]):
                first, n = int(pairs[k, o]['first']), int(pairs[k, o]['n_entries'])
                cells = ' '.join(f'{int(e["i"])}:{int(e["j"])}:{int(e["count"])}' for e in entries[first:first + n])
                w.writerow([repr(v.item()) for v in d[k, o]] + [repr(int(table[k]['level_min'])), repr(int(table[k]['level_max'])), repr(n), cells])


# ---- the GPU forms (sdsm_texture.hip) ---------------------------------------------------------------------------------------------------
class _TextureSet:
    """One set of up to ``_capi.MAX_SET_IMAGES`` images with their intensities and edges on the current device and the two calls of the
    texture kernels."""

    def __init__(self, shapes, intensities, edges_list, offs):
        self.M = _MeasureSet(shapes, intensities)     # (the intensities packed; the label form takes the boxes of the labels from there)
        self.S = S = self.M.S
        self.n_im = len(S.shapes)
        self.levels = len(edges_list[0]) + 1
        self.d_edges = S._up(np.concatenate(edges_list)) if self.levels > 1 else None
        self.n_o = len(offs)
        self.c_offsets = (S.C.c_int32 * (2 * self.n_o))(*[v for o in offs for v in o])

    def slot_offsets(self, boxes):
        """Where every (object, offset) writes its cells before they are gathered: min(h w, G (G + 1) / 2) entries each are always
        enough.  Raises, before anything is launched, where the list passes ``_capi.TEXTURE_MAX_SLOTS``."""
        b = np.asarray(boxes, np.int64).reshape(-1, 4)
        room = np.minimum(np.maximum(b[:, 2], 0) * np.maximum(b[:, 3], 0), self.levels * (self.levels + 1) // 2)
        off = np.concatenate([[0], np.cumsum(np.repeat(room, self.n_o))]).astype(np.int64)
        if int(off[-1]) > _capi.TEXTURE_MAX_SLOTS:
            raise ValueError(f'the cells of {len(b)} objects and {self.n_o} offsets may take {int(off[-1])} entries: the texture tables take up to '
                             f'{_capi.TEXTURE_MAX_SLOTS} per set (fewer levels, offsets or objects per call), see DESIGN.md "Limits"')
        return off

    def buffers(self, n, slots):
        """The workspace and the three outputs of a call; their contents do not matter."""
        S = self.S
        u8 = lambda size: S.torch.empty(max(8, size), dtype=S.torch.uint8, device=S.dev)
        return dict(d_out=u8(n * _capi.TEXTURE_RECORD_DTYPE.itemsize), d_pairs=u8(n * self.n_o * PAIRS_DTYPE.itemsize),
                    d_slots=u8(slots * ENTRY_DTYPE.itemsize), d_entries=u8(slots * ENTRY_DTYPE.itemsize))

    def _download(self, B, n):
        recs = self.S.records(B['d_out'], n, _capi.TEXTURE_RECORD_DTYPE)
        pairs = self.S.records(B['d_pairs'], n * self.n_o, PAIRS_DTYPE).reshape(n, self.n_o)
        total = int(pairs['n_entries'].sum())                                      # (only the cells that exist are downloaded)
        entries = B['d_entries'][:total * ENTRY_DTYPE.itemsize].cpu().numpy().view(ENTRY_DTYPE).copy()
        return recs, pairs, entries

    def objects(self, obj_image, boxes, words, packed, B=None):
        """(records, pairs, entries) of the objects of the set (``packed``: the bit-packed fragments, one uint8 array of whole words each)."""
        S, n = self.S, len(boxes)
        slot_off = self.slot_offsets(boxes)
        B = self.buffers(n, int(slot_off[-1])) if B is None else B
        d_objects, d_slot_off = S.upload_objects(obj_image, boxes, words, packed), S._up(slot_off)
        S.capi.check(S.L.sdsm_texture_objects_multi(S.table, self.n_im, n, *map(S._p, d_objects), S._p(self.M.d_g), self.levels, S._p(self.d_edges), self.n_o,
                                                    self.c_offsets, S._p(d_slot_off), S._p(B['d_slots']), S._p(B['d_out']), S._p(B['d_pairs']),
                                                    S._p(B['d_entries']), S._stream()), 'sdsm_texture_objects_multi')
        return self._download(B, n)

    def labels(self, labels, background_label):
        """Per image (labels measured, number of labels, records, pairs, entries) of the label maps of the set: the windows of the labels
        (``measure._LabelWindows``), then sdsm_texture_labels."""
        S = self.S
        w = _LabelWindows(self.M, labels, background_label, 'texture')
        n = len(w.idx)
        slot_off = self.slot_offsets(w.boxes)
        B = self.buffers(n, int(slot_off[-1]))
        d_slot_off = S._up(slot_off)
        S.capi.check(S.L.sdsm_texture_labels_multi(S.table, self.n_im, *w.args(), S._p(self.M.d_g), self.levels, S._p(self.d_edges), self.n_o, self.c_offsets,
                                                   S._p(d_slot_off), S._p(B['d_slots']), S._p(B['d_out']), S._p(B['d_pairs']), S._p(B['d_entries']),
                                                   S._p(w.d_bad), S._stream()), 'sdsm_texture_labels_multi')
        recs, pairs, entries = self._download(B, n)
        return [(ls, n_labels) + _split(recs, pairs, entries, a, b) for ls, n_labels, a, b in w.per_image()]


def _split(recs, pairs, entries, a, b):
    """The objects a .. b - 1 of a call: (records, pairs with ``first`` from 0, their entries)."""
    p = pairs[a:b].copy()
    lo = int(pairs[a, 0]['first']) if a < len(pairs) else len(entries)
    p['first'] -= lo
    return recs[a:b], p, entries[lo:lo + int(p['n_entries'].sum())]


def texture_objects_many(objects_per_image, shapes, intensities, edges_list, offsets=DEFAULT_OFFSETS):
    """:func:`texture_objects` for a list of images with one list of edges per image (all of the same length): one launch per
    ``_capi.MAX_SET_IMAGES`` images (larger lists are split).  Per image the bytes of :func:`texture_objects_host`."""
    objects_per_image = list(objects_per_image)
    sets = _object_sets(objects_per_image, shapes, intensities, required=True)
    edges_list, offs = _edges_many(edges_list, len(objects_per_image)), check_offsets(offsets)
    out = []
    for part, shapes_part, gs, packed, first in sets:
        recs, pairs, entries = _TextureSet(shapes_part, gs, edges_list[part], offs).objects(*packed)
        for a, b in zip(first[:-1], first[1:]):
            r, p, e = _split(recs, pairs, entries, a, b)
            out.append((_table(np.arange(b - a), r), p, e))
    return out


def texture_objects(objects, shape, intensity, edges, offsets=DEFAULT_OFFSETS):
    """``(table, pairs, entries)`` of a list of objects (``fg_offset``, ``fg_fragment``; they may overlap) of an image of ``shape`` with
    the intensities ``intensity`` on the GPU, one workgroup per object and offset; row k is object k.  The bytes of
    :func:`texture_objects_host`."""
    return texture_objects_many([objects], [shape], [intensity], [edges], offsets)[0]


def texture_labels_many(labels_list, intensities, edges_list, offsets=DEFAULT_OFFSETS, background_label=0, keep_absent=False):
    """:func:`texture_labels` for a list of label maps with one list of edges per image, one launch per ``_capi.MAX_SET_IMAGES`` images."""
    labels_list = list(labels_list)
    sets = _label_sets(labels_list, intensities, required=True)
    edges_list, offs = _edges_many(edges_list, len(labels_list)), check_offsets(offsets)
    out = []
    for part, l32, shapes, gs in sets:
        T = _TextureSet(shapes, gs, edges_list[part], offs)
        for ls, n_labels, recs, pairs, entries in T.labels(l32, background_label):
            if keep_absent:
                full_pairs = np.zeros((n_labels, len(offs)), PAIRS_DTYPE)
                full_pairs[ls] = pairs
                full_pairs['first'] = _exclusive(full_pairs['n_entries'].reshape(-1)).reshape(full_pairs.shape)
                (ls, recs), pairs = _keep_absent(_empty_records(n_labels, T.levels), ls, recs), full_pairs
            out.append((_table(ls, recs), pairs, entries))
    return out


def texture_labels(labels, intensity, edges, offsets=DEFAULT_OFFSETS, background_label=0, keep_absent=False):
    """``(table, pairs, entries)`` of a label map (integer, labels 0 .. 65535) on the GPU: the present labels without
    ``background_label`` (None: all) in ascending order, or with ``keep_absent`` one row per label 0 .. max.  The bytes of
    :func:`texture_labels_host`."""
    return texture_labels_many([labels], [intensity], [edges], offsets, background_label, keep_absent)[0]


def texture_result(data, objects='postprocessed_objects', intensity='g_raw', levels=DEFAULT_LEVELS, offsets=DEFAULT_OFFSETS, edges=None):
    """The texture table of the objects of pipeline data: ``objects`` an output name or a list of objects, ``intensity`` a key of ``data``
    or an image; ``levels`` equally wide levels over the finite range of that image (:func:`image_edges`), or the caller's ``edges``."""
    objs, shape, g = _result_inputs(data, objects, intensity)
    return texture_objects(objs, shape, g, image_edges(g, levels) if edges is None else edges, offsets)
