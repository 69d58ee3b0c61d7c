"""ctypes binding of the C ABI declared in include/sdsm.h (libsdsm_hip.so).

There is no CPU fallback: if the shared library is missing or a symbol cannot be resolved, importing callers
fail loudly here.  PyTorch-ROCm is used only as the owner of device memory (tensors -> raw device pointers)
and of the stream.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SDSM_HIP_LIB', os.path.join(_HERE, 'libsdsm_hip.so'))   # override: diagnostic builds only

SDSM_OK = 0
ATOM_STATS_STRIDE = 6

CAND_OPTIMAL, CAND_FALLBACK, CAND_TRIVIAL, CAND_ERROR, CAND_UNSUPPORTED, CAND_GIVEN_UP = 0, 1, 2, 3, 4, 5


class DsmConfig(C.Structure):
    """sdsm_dsm_config: DSM_CONFIG_DEFAULTS of the reference (superdsm/dsmcfg.py:6-21)."""
    _fields_ = [('scale', C.c_double), ('epsilon', C.c_double), ('alpha', C.c_double), ('smooth_amount', C.c_double),
                ('gaussian_shape_multiplier', C.c_double), ('background_margin', C.c_double),
                ('smooth_subsample', C.c_int32), ('init_elliptical', C.c_int32), ('max_iters', C.c_int32), ('flags', C.c_int32)]


RECORD_DTYPE = np.dtype([
    ('energy', 'f8'), ('theta', 'f8', 6), ('energy_ell', 'f8'),
    ('status', 'i4'), ('flags', 'i4'), ('n_pixels', 'i4'), ('n_deform', 'i4'),
    ('iters_ell', 'i4'), ('iters_dsm', 'i4'), ('evals_value', 'i4'), ('evals_full', 'i4'),
    ('on_boundary', 'i4'), ('fg_r0', 'i4'), ('fg_c0', 'i4'), ('fg_h', 'i4'), ('fg_w', 'i4'), ('n_positive', 'i4'), ('n_negative', 'i4'), ('reserved', 'i4')])
assert RECORD_DTYPE.itemsize == 128
# CandDesc and CandState of csrc/sdsm_common.h, field by field: what the plan uploads per candidate and what the setup kernel writes
CAND_DESC_DTYPE = np.dtype([
    ('crop_off', 'i8'), ('ell_off', 'i8'), ('mask_off', 'i8'), ('xi_off', 'i8'),
    ('N', 'i4'), ('r0', 'i4'), ('c0', 'i4'), ('h', 'i4'), ('w', 'i4'), ('fp_off', 'i4'), ('fp_len', 'i4'), ('Mcap', 'i4'), ('perm_inv', 'u4'), ('wide_g', 'i4'),
    ('hglob_off', 'i8'), ('wide_off', 'i8'), ('image', 'i4'), ('NRcap', 'i4'), ('run_off', 'i8'), ('rows_g', 'i4'), ('pad1', 'i4')])
assert CAND_DESC_DTYPE.itemsize == 112
CAND_STATE_DTYPE = np.dtype([
    ('M', 'i4'), ('status', 'i4'), ('hc', 'i4'), ('wc', 'i4'), ('npos', 'i4'), ('zmax', 'i4'),
    ('sum_r', 'u8'), ('sum_c', 'u8'), ('sum_rr', 'u8'), ('sum_cc', 'u8'),
    ('hzmax', 'i4'), ('env_size', 'i4'), ('nneg', 'i4'), ('yexp', 'i4'), ('NR', 'i4'), ('pad', 'i4', 7)])
assert CAND_STATE_DTYPE.itemsize == 104
# the 16 values of sdsm_plan_layout: byte offsets of workspace blocks, then sizes and counts
PLAN_LAYOUT_NAMES = ('cand', 'state', 'crop_y', 'crop_rc', 'crop_cc', 'run_meta', 'grid_rc', 'ell_im', 'ell_w', 'zcap_run', 'k',
                     'cand_size', 'total_pixels', 'total_ell', 'state_size', 'total_runs')
# BatchParams of csrc/sdsm_common.h, the parameter blob of sdsm_plan_image (pointers as u8: over a null workspace they hold byte offsets)
_IMAGE_REF = np.dtype([('y', 'u8'), ('atoms', 'u8'), ('valid', 'u8'), ('H', 'i4'), ('W', 'i4')])
PLAN_PARAMS_DTYPE = np.dtype(
    [('n', 'i4'), ('n_images', 'i4'), ('n_total', 'i4'), ('latency', 'i4'), ('img', _IMAGE_REF, 16)]
    + [(f, 'i4') for f in ('k', 'R', 'subsample', 'zcap', 'zcap_run', 'zshift', 'no_deform', 'no_trivial_rule', 'init_elliptical', 'max_iters', 'k1_pixmax', 'pad0')]
    + [(f, 'f8') for f in ('scale', 'epsilon', 'alpha', 'reg_unit')] + [('hess_thr', 'f4')]
    + [(f, 'i4') for f in ('boost_pixels', 'light_emax', 'wide_rest', 'rows_mcap', 'solver_diag')]
    + [(f, 'u8') for f in ('cand', 'state', 'fp_labels', 'order', 'crop_y', 'crop_rc', 'run_meta', 'run_q0', 'run_aux', 'tmp_y', 'tmp_rc', 'crop_cc', 'dist', 'inv',
                           'grid_rc', 'ell_w', 'ell_im', 'env_fst', 'env_rb', 'psf', 'wide_pool', 'wide_ticket')]
    + [('wide_timeout', 'i8')] + [(f, 'u8') for f in ('cls_count', 'hglob', 'prof', 'prof2', 'x0')])
PLAN_PARAMS_BYTES = PLAN_PARAMS_DTYPE.itemsize
assert PLAN_PARAMS_BYTES == 856 and PLAN_PARAMS_DTYPE.fields['wide_rest'][1] == 620 and PLAN_PARAMS_DTYPE.fields['solver_diag'][1] == 628
POST_RECORD_DTYPE = np.dtype([('contrast', 'f8'), ('interior_mean', 'f8'), ('exterior_mean', 'f8'), ('fg_mean', 'f8'), ('fg_std', 'f8'),
                              ('area', 'i4'), ('status', 'i4'), ('r0', 'i4'), ('c0', 'i4'), ('h', 'i4'), ('w', 'i4')])
assert POST_RECORD_DTYPE.itemsize == 64
DOH_PEAK_DTYPE = np.dtype([('r', 'i4'), ('c', 'i4'), ('s', 'i4'), ('reserved', 'i4'), ('value', 'f8')])   # sdsm_doh_peak
assert DOH_PEAK_DTYPE.itemsize == 24
DOH_PEAKS_HEADER_BYTES = 16
DOH_MAX_SCALES = 32
MAX_SET_IMAGES = 32          # SDSM_MAX_SET_IMAGES: images per call of a *_multi entry point
RENDER_MAX_RADIUS = 16       # SDSM_RENDER_MAX_RADIUS: largest disk of the label-map and overlay kernels
RENDER_MAX_COLORS = 1024     # SDSM_RENDER_MAX_COLORS: entries of a colour map of the colour-map kernel
RENDER_MAX_SEED_RADIUS = 64  # SDSM_RENDER_MAX_SEED_RADIUS: largest seed disk (with its rim) of the graph kernel
RENDER_ENTRY_DTYPE = np.dtype([('idx', 'i4'), ('label', 'i4'), ('dist', 'f8')])   # sdsm_render_entry
assert RENDER_ENTRY_DTYPE.itemsize == 16
MEASURE_MAX_LABELS = 65536   # SDSM_MEASURE_MAX_LABELS: labels 0 .. 65535 per image of the label form of the measurement tables
_MEASURE_FIELDS = [('area', 'i8'), ('sum_r', 'i8'), ('sum_c', 'i8'), ('sum_rr', 'u8'), ('sum_rc', 'u8'), ('sum_cc', 'u8'),
                   ('r0', 'i4'), ('c0', 'i4'), ('r1', 'i4'), ('c1', 'i4'), ('flags', 'i4'), ('scale_exp', 'i4'),
                   ('n_finite', 'i8'), ('gsum_lo', 'u8'), ('gsum_hi', 'i8'), ('gmin', 'f8'), ('gmax', 'f8')]
MEASURE_RECORD_DTYPE = np.dtype(_MEASURE_FIELDS)                                   # sdsm_measure_record
assert MEASURE_RECORD_DTYPE.itemsize == 112
BOUNDARY_MAX_LABELS = 65536  # SDSM_BOUNDARY_MAX_LABELS: labels 0 .. 65535 per image of the boundary distances
BOUNDARY_TILE = 1024         # SDSM_BOUNDARY_TILE: boundary pixels of the target per LDS tile of the distance kernel
BOUNDARY_CHUNK = 1024        # SDSM_BOUNDARY_CHUNK: query pixels of one work item of the distance kernel
PAIR_DISTANCE_DTYPE = np.dtype([('a', '<i4'), ('b', '<i4'), ('boundary_a', '<i4'), ('boundary_b', '<i4'), ('max_d2_ab', '<i4'), ('max_d2_ba', '<i4'),
                                ('flags', '<i4'), ('reserved', '<i4'), ('sum_q_ab', '<i8'), ('sum_q_ba', '<i8'), ('nsd_num', '<i8'),
                                ('nsd_den', '<i8')])                                 # sdsm_pair_distance
assert PAIR_DISTANCE_DTYPE.itemsize == 64
SHAPE_MAX_CHAIN = 4096              # SDSM_SHAPE_MAX_CHAIN: vertices of one chain of a hull
SHAPE_MAX_WINDOW_WORDS = 1 << 26    # SDSM_SHAPE_MAX_WINDOW_WORDS: words of all label windows of a call of the label form of the shape tables
SHAPE_CHAIN_OVERFLOW = 1 << 30      # flag bit 30 of sdsm_shape_record
_SHAPE_FIELDS = [('area', 'i8'), ('border_pixels', 'i8'), ('edges_r', 'i8'), ('edges_c', 'i8'), ('perim_n1', 'i8'), ('perim_n2', 'i8'), ('perim_n3', 'i8'),
                 ('hull_area2', 'i8'), ('feret_max_d2', 'i8'), ('n_vertices', 'i4'), ('flags', 'i4')]
SHAPE_RECORD_DTYPE = np.dtype(_SHAPE_FIELDS)                                       # sdsm_shape_record
assert SHAPE_RECORD_DTYPE.itemsize == 80
INTENSITY_MAX_QUANTILES = 8         # SDSM_INTENSITY_MAX_QUANTILES: quantiles of one call of the intensity tables
INTENSITY_MAX_DEN = 10 ** 6         # SDSM_INTENSITY_MAX_DEN: largest denominator of a quantile
INTENSITY_LDS_KEYS = 4096           # SDSM_INTENSITY_LDS_KEYS: finite pixels of an object that is selected from LDS
_INTENSITY_FIELDS = [('area', 'i8'), ('n_finite', 'i8'), ('sum_p', 'i8'), ('sum_pp_lo', 'u8'), ('sum_pp_hi', 'u8'), ('gmin', 'f8'), ('gmax', 'f8'),
                     ('med_lo', 'f8'), ('med_hi', 'f8'), ('mad_lo', 'f8'), ('mad_hi', 'f8'), ('range_exp', 'i4'), ('flags', 'i4')]
INTENSITY_RECORD_DTYPE = np.dtype(_INTENSITY_FIELDS)                               # sdsm_intensity_record
assert INTENSITY_RECORD_DTYPE.itemsize == 96
TEXTURE_MAX_LEVELS = 256            # SDSM_TEXTURE_MAX_LEVELS: grey levels of the texture tables
TEXTURE_MAX_OFFSETS = 8             # SDSM_TEXTURE_MAX_OFFSETS: offsets of one call of the texture tables
TEXTURE_MAX_REACH = 32              # SDSM_TEXTURE_MAX_REACH: largest |d_row|, |d_col| of an offset
TEXTURE_MAX_SLOTS = 1 << 26         # SDSM_TEXTURE_MAX_SLOTS: entries of the padded list of a call of the texture tables
_TEXTURE_FIELDS = [('area', 'i8'), ('n_finite', 'i8'), ('level_min', 'i4'), ('level_max', 'i4'), ('flags', 'i4'), ('reserved', 'i4')]
TEXTURE_RECORD_DTYPE = np.dtype(_TEXTURE_FIELDS)                                   # sdsm_texture_record
TEXTURE_PAIRS_DTYPE = np.dtype([('n_pairs', 'i8'), ('first', 'i8'), ('n_entries', 'i4'), ('reserved', 'i4')])   # sdsm_texture_pairs
TEXTURE_ENTRY_DTYPE = np.dtype([('i', 'u2'), ('j', 'u2'), ('count', 'u4')])        # sdsm_texture_entry
assert TEXTURE_RECORD_DTYPE.itemsize == 32 and TEXTURE_PAIRS_DTYPE.itemsize == 24 and TEXTURE_ENTRY_DTYPE.itemsize == 8
NEIGHBOUR_MAX_D2 = 4096             # SDSM_NEIGHBOUR_MAX_D2: largest squared reach of the neighbourhood tables (64 pixels)
NEIGHBOUR_LABEL_DTYPE = np.dtype([('edges_background', '<i8'), ('edges_labels', '<i8'), ('edges_frame', '<i8'), ('area', '<i4'), ('boundary', '<i4'),
                                  ('close', '<i4'), ('reserved', '<i4')])                  # sdsm_neighbour_label
NEIGHBOUR_PAIR_DTYPE = np.dtype([('a', '<i4'), ('b', '<i4'), ('min_d2', '<i4'), ('contact_edges', '<i4')])   # sdsm_neighbour_pair
assert NEIGHBOUR_LABEL_DTYPE.itemsize == 40 and NEIGHBOUR_PAIR_DTYPE.itemsize == 16
ZONE_MAX_D2 = 4096                  # SDSM_ZONE_MAX_D2: largest squared bound of a zone and largest squared reach of the nearest-other transform
ZONE_MAX_ZONES = 8                  # SDSM_ZONE_MAX_ZONES: zones of one call
ZONE_NO_UPPER = 0x7fffffff          # SDSM_ZONE_NO_UPPER: hi_d2 of a zone without an upper bound
ZONE_SIDE_BACKGROUND, ZONE_SIDE_OBJECT = 0, 1
_ZONE_FIELDS = [('side', 'i4'), ('keep_own', 'i4'), ('lo_d2', 'i4'), ('hi_d2', 'i4')]
ZONE_SPEC_DTYPE = np.dtype(_ZONE_FIELDS)                                           # sdsm_zone_spec
assert ZONE_SPEC_DTYPE.itemsize == 16
PARTS_MAX_KEEPS = 8                 # SDSM_PARTS_MAX_KEEPS: selections of one call of the connected parts
KEEP_SPLIT, KEEP_LARGEST, KEEP_MIN_AREA = 0, 1, 2
_PART_FIELDS = [('label', '<i4'), ('area', '<i4'), ('first', '<i4'), ('r0', '<i4'), ('c0', '<i4'), ('r1', '<i4'), ('c1', '<i4'), ('index_in_label', '<i4')]
_PART_LABEL_FIELDS = [('n_parts', '<i4'), ('area', '<i4'), ('largest_area', '<i4'), ('largest_part', '<i4'), ('q1', '<i4'), ('q3', '<i4'), ('qd', '<i4'),
                      ('reserved', '<i4')]
PART_DTYPE = np.dtype(_PART_FIELDS)                                                # sdsm_part_record
PART_LABEL_DTYPE = np.dtype(_PART_LABEL_FIELDS)                                    # sdsm_part_label_record
KEEP_SPEC_DTYPE = np.dtype([('kind', '<i4'), ('min_area', '<i4')])                 # sdsm_keep_spec
assert PART_DTYPE.itemsize == 32 and PART_LABEL_DTYPE.itemsize == 32 and KEEP_SPEC_DTYPE.itemsize == 8
DEPTH_MAX_SHELLS = 32               # SDSM_DEPTH_MAX_SHELLS: shells of one call of the depth tables
DEPTH_LDS_PIXELS = 12288            # SDSM_DEPTH_LDS_PIXELS: pixels of a box whose distance transform is held in LDS
DEPTH_WS_PIXEL_BYTES = 8            # SDSM_DEPTH_WS_PIXEL_BYTES: workspace bytes per pixel of a larger box
DEPTH_NO_WORKSPACE = 1 << 30        # flag bit 30 of sdsm_depth_record
_DEPTH_FIELDS = [('area', 'i8'), ('max_d2', 'i8'), ('max_row', 'i4'), ('max_col', 'i4'), ('n_max', 'i8'), ('sum_d2', 'i8'), ('sum_q', 'i8'),
                 ('med_d2_lo', 'i8'), ('med_d2_hi', 'i8'), ('n_rim', 'i8'), ('flags', 'i4'), ('scale_exp', 'i4')]
_DEPTH_SHELL_FIELDS = [('count', 'i8'), ('n_finite', 'i8'), ('gsum_lo', 'u8'), ('gsum_hi', 'i8')]
DEPTH_RECORD_DTYPE = np.dtype(_DEPTH_FIELDS)                                       # sdsm_depth_record
DEPTH_SHELL_DTYPE = np.dtype(_DEPTH_SHELL_FIELDS)                                  # sdsm_depth_shell_record
assert DEPTH_RECORD_DTYPE.itemsize == 80 and DEPTH_SHELL_DTYPE.itemsize == 32
SKELETON_LDS_WORDS = 3072           # SDSM_SKELETON_LDS_WORDS: 64-bit words (h * ceil(w / 64)) of a box whose thinning is held in LDS
SKELETON_WAVE_SIDE = 64             # a box of at most 64 x 64 is thinned in the registers of one wavefront
SKELETON_NO_WORKSPACE = 1 << 30     # flag bit 30 of sdsm_skeleton_record
_SKELETON_FIELDS = [(name, 'i4') for name in ('area', 'n_skeleton', 'n_end', 'n_isolated', 'n_branch', 'n_orth', 'n_diag', 'cycles', 'first_row', 'first_col',
                                              'flags', 'reserved')]
SKELETON_RECORD_DTYPE = np.dtype(_SKELETON_FIELDS)                                 # sdsm_skeleton_record
assert SKELETON_RECORD_DTYPE.itemsize == 48


class MeasureRecord(C.Structure):
    """sdsm_measure_record: the exact integer sums of one object or label."""
    _fields_ = [(name, {'i8': C.c_int64, 'u8': C.c_uint64, 'i4': C.c_int32, 'f8': C.c_double}[kind]) for name, kind in _MEASURE_FIELDS]


assert C.sizeof(MeasureRecord) == 112 and all(getattr(MeasureRecord, n).offset == MEASURE_RECORD_DTYPE.fields[n][1] for n, _ in _MEASURE_FIELDS)


class SetImage(C.Structure):
    """sdsm_set_image: an image of a set in the packed buffers of a *_multi call."""
    _fields_ = [('offset', C.c_int64), ('H', C.c_int32), ('W', C.c_int32)]


class PostImage(C.Structure):
    """sdsm_post_image: the per-image inputs of sdsm_post_objects_multi."""
    _fields_ = [('d_g', C.c_void_p), ('d_gs', C.c_void_p), ('d_bg', C.c_void_p), ('H', C.c_int32), ('W', C.c_int32),
                ('inv_gstd', C.c_double), ('n_objects', C.c_int32), ('reserved', C.c_int32)]

class PostBgImage(C.Structure):
    """sdsm_post_bg_image: the per-image buffers of sdsm_post_background_multi."""
    _fields_ = [('d_bg', C.c_void_p), ('d_work', C.c_void_p), ('H', C.c_int32), ('W', C.c_int32), ('n_objects', C.c_int32), ('reserved', C.c_int32)]


POST_MAX_BG_RADIUS = 32          # SDSM_POST_MAX_BG_RADIUS
POST_MAX_GLARE_LAYERS = 32       # SDSM_POST_MAX_GLARE_LAYERS
POST_FLOOD_WORDS = 4096          # POST_FLOOD_WORDS of sdsm_post.hip: whole-word rows of a window flooded in LDS

# every entry point of include/sdsm.h: name -> (restype, argtypes)
_vp, _i32, _f64, _sz, _i64 = C.c_void_p, C.c_int, C.c_double, C.c_size_t, C.c_int64
SYMBOLS = {
    'sdsm_version': (_i32, []),
    'sdsm_last_error': (C.c_char_p, []),
    'sdsm_device_count': (_i32, []),
    'sdsm_set_device': (_i32, [_i32]),
    'sdsm_stream_synchronize': (_i32, [_vp]),
    'sdsm_psf': (_i32, [_f64, _f64, _vp]),
    'sdsm_preprocess_workspace_bytes': (_sz, [_i32, _i32, _f64, _f64]),
    'sdsm_preprocess': (_i32, [_vp, _i32, _i32, _f64, _f64, _f64, _i32, _vp, _vp, _sz, _vp]),
    'sdsm_image_workspace_bytes': (_sz, [_i32, _i32]),
    'sdsm_image_prepare': (_i32, [_vp, _vp, _vp, _i32, _i32, _f64, _i32, _vp, _vp, _vp, _sz, _vp]),
    'sdsm_plan_create': (_vp, [_i32, _i32, _i32, _vp, C.POINTER(DsmConfig), _i32, _vp, _vp]),
    'sdsm_plan_create_multi': (_vp, [_i32, _vp, _vp, _vp, _vp, C.POINTER(DsmConfig), _i32, _vp, _vp, _vp]),
    'sdsm_plan_destroy': (None, [_vp]),
    'sdsm_plan_workspace_bytes': (_sz, [_vp]),
    'sdsm_plan_mask_bytes': (_sz, [_vp]),
    'sdsm_plan_describe': (_i32, [_vp, _vp, _vp, _vp]),
    'sdsm_plan_total_pixels': (_i64, [_vp]),
    'sdsm_batch_upload': (_i32, [_vp, _vp, _sz, _vp]),
    'sdsm_batch_launch': (_i32, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    'sdsm_batch_launch_multi': (_i32, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    'sdsm_plan_xi_count': (_i64, [_vp]),
    'sdsm_plan_xi_offsets': (_i32, [_vp, _vp]),
    'sdsm_plan_layout': (_i32, [_vp, _vp]),
    'sdsm_plan_schedule': (_i32, [_vp, _vp, _vp]),
    'sdsm_plan_lists': (_i32, [_vp, _vp, _vp]),
    'sdsm_plan_image': (_i32, [_vp, _vp, _sz, _vp, _sz]),
    'sdsm_plan_solve_classes': (_i32, [_vp, _vp, _vp, _vp, _vp]),
    'sdsm_set_light_envelope_limit': (_i32, [_i32]),
    'sdsm_plan_set_latency_mode': (_i32, [_vp, _i32]),
    'sdsm_post_objects': (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f64, _f64, _f64, _f64, _i32, _f64, _vp, _vp]),
    'sdsm_post_objects_multi': (_i32, [C.POINTER(PostImage), _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f64, _f64, _f64, _i32, _f64, _vp, _vp]),
    'sdsm_post_background_multi': (_i32, [C.POINTER(PostBgImage), _i32, _vp, _vp, _vp, _i32, _vp]),
    'sdsm_post_fill_holes': (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_post_glare_multi': (_i32, [C.POINTER(PostImage), _i32, _vp, _vp, _vp, C.POINTER(C.c_double), _i32, _vp, _vp, _vp, _vp]),
    'sdsm_gaussian_workspace_bytes': (_sz, [_i32, _i32, _f64]),
    'sdsm_gaussian_filter': (_i32, [_vp, _i32, _i32, _f64, _vp, _vp, _sz, _vp]),
    'sdsm_separable_workspace_bytes': (_sz, [_i32, _i32, _i32, _i32]),
    'sdsm_separable_filter': (_i32, [_vp, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _sz, _vp]),
    'sdsm_log_masks_workspace_bytes': (_sz, [_i32, _i32]),
    'sdsm_log_masks': (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    'sdsm_integral_image': (_i32, [_vp, _i32, _i32, _vp, _vp]),
    'sdsm_doh_cube': (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_doh_peaks': (_i32, [_vp, _i32, _i32, _i32, _f64, _vp, _i64, _vp]),
    'sdsm_c2f_markers_workspace_bytes': (_sz, [_i32, _i32]),
    'sdsm_c2f_markers': (_i32, [_vp, _i32, _i32, _f64, _vp, _vp, _vp, _vp, _sz, _vp]),
    'sdsm_edt_exact_workspace_bytes': (_sz, [_i32, _i32]),
    'sdsm_edt_exact': (_i32, [_vp, _i32, _i32, _vp, _vp, _sz, _vp]),
    'sdsm_watershed': (_i32, [_vp, _vp, _vp, _i32, _i32, _vp]),
    'sdsm_c2f_markers_workspace_bytes_multi': (_sz, [C.POINTER(SetImage), _i32]),
    'sdsm_c2f_markers_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, C.POINTER(C.c_double), _vp, _vp, _vp, _vp, _sz, _vp]),
    'sdsm_edt_exact_workspace_bytes_multi': (_sz, [C.POINTER(SetImage), _i32]),
    'sdsm_edt_exact_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, _vp, _vp, _sz, _vp]),
    'sdsm_render_morph': (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    'sdsm_render_morph_multi': (_i32, [C.POINTER(SetImage), _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    'sdsm_render_overlaps': (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_render_paint': (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_render_paint_multi': (_i32, [C.POINTER(SetImage), _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_render_compact': (_i32, [_i32, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    'sdsm_render_compact_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, _vp, _vp, C.POINTER(C.c_int64), _vp, _vp, _vp]),
    'sdsm_flood_sparse': (_i32, [_i64, _vp, _vp, _vp, _i32, _i32, _vp]),
    'sdsm_render_scatter': (_i32, [_i64, _vp, _vp, _vp, _vp]),
    'sdsm_render_lost': (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    'sdsm_render_lost_multi': (_i32, [C.POINTER(SetImage), _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    'sdsm_render_fill': (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    'sdsm_render_fill_multi': (_i32, [C.POINTER(SetImage), _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    'sdsm_render_finish': (_i32, [_i64, _vp, _i32, _vp, _vp]),
    'sdsm_render_overlay': (_i32, [_i32, _i32, _vp, _vp, _i32, _i32, _i32, C.POINTER(C.c_double), C.POINTER(C.c_double), _i32, _vp, _vp]),
    'sdsm_render_overlay_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, _vp, _i32, _i32, _i32, C.POINTER(C.c_double), C.POINTER(C.c_double), _i32, _vp, _vp]),
    'sdsm_render_label_range': (_i32, [_i32, _i32, _vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    'sdsm_render_label_range_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _vp, _vp, _vp]),
    'sdsm_render_colormap': (_i32, [_i32, _i32, _i32, _vp, _vp, _i32, C.POINTER(C.c_double), _vp, _i64, _i32, _vp, C.POINTER(C.c_double), _i32, _vp, _vp, _vp]),
    'sdsm_render_colormap_multi': (_i32, [C.POINTER(SetImage), _i32, _i32, _vp, _vp, _i32, C.POINTER(C.c_double), _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                          _vp, C.POINTER(C.c_double), _i32, _vp, _vp, _vp]),
    'sdsm_render_graph': (_i32, [_i32, _i32, _i32, _vp, _f64, _f64, _i32, _i32, _i32, C.POINTER(C.c_double), _vp, _i32, _vp, _vp, _vp]),
    'sdsm_render_graph_multi': (_i32, [C.POINTER(SetImage), _i32, _i32, _vp, _f64, _f64, _i32, _i32, _i32, C.POINTER(C.c_double), _vp, _i32, _vp, _vp, _vp]),
    'sdsm_measure_objects': (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_measure_objects_multi': (_i32, [C.POINTER(SetImage), _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_measure_labels': (_i32, [_i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_measure_labels_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_shape_vertex_slots': (_i64, [_i32, _i32]),
    'sdsm_shape_objects': (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_shape_objects_multi': (_i32, [C.POINTER(SetImage), _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_shape_labels': (_i32, [_i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_shape_labels_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _vp, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp,
                                       _vp, _vp, _vp, _vp, _vp]),
    'sdsm_quantile_ranks': (_i32, [_i64, _i32, _i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'sdsm_intensity_objects': (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, _vp, _vp]),
    'sdsm_intensity_objects_multi': (_i32, [C.POINTER(SetImage), _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, _vp,
                                            _vp]),
    'sdsm_intensity_labels': (_i32, [_i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, _vp, _vp,
                                     _vp]),
    'sdsm_intensity_labels_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _vp, _i32, _vp, _vp, _vp, _i64, _vp, _vp,
                                           _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, _vp, _vp, _vp]),
    'sdsm_texture_level': (_i32, [C.POINTER(C.c_double), _i32, _f64]),
    'sdsm_texture_cell': (_i32, [_i32, _i32, _i32]),
    'sdsm_texture_objects': (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_texture_objects_multi': (_i32, [C.POINTER(SetImage), _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp,
                                          _vp, _vp]),
    'sdsm_texture_labels': (_i32, [_i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _i32, _vp, _i32, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp]),
    'sdsm_texture_labels_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _vp, _i32, _vp, _vp, _vp, _i64, _vp, _vp,
                                         _i32, _vp, _i32, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_depth_shell': (_i32, [_i64, _i32]),
    'sdsm_depth_workspace_pixels': (_i64, [_i32, _i32]),
    'sdsm_depth_objects': (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _sz, _vp, _vp, _vp]),
    'sdsm_depth_objects_multi': (_i32, [C.POINTER(SetImage), _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _sz, _vp, _vp, _vp]),
    'sdsm_depth_labels': (_i32, [_i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _sz, _vp, _vp, _vp, _vp]),
    'sdsm_depth_labels_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _vp, _i32, _vp, _vp, _vp, _i64, _vp, _vp,
                                       _vp, _vp, _i32, _vp, _vp, _i64, _sz, _vp, _vp, _vp, _vp]),
    'sdsm_skeleton_deletable': (_i32, [_i32, _i32]),
    'sdsm_skeleton_workspace_words': (_i64, [_i32, _i32]),
    'sdsm_skeleton_thin': (_i32, [_i32, _i32, _vp, _vp]),
    'sdsm_skeleton_objects': (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _sz, _vp, _vp, _vp]),
    'sdsm_skeleton_objects_multi': (_i32, [C.POINTER(SetImage), _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _sz, _vp, _vp, _vp]),
    'sdsm_skeleton_labels': (_i32, [_i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _sz, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_skeleton_labels_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _vp, _i32, _vp, _vp, _vp, _i64, _vp, _vp,
                                          _vp, _vp, _i64, _sz, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_overlap_pairs': (_i32, [_i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    'sdsm_overlap_pairs_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _vp, _vp, _vp, _vp]),
    'sdsm_neighbour_halfwidth': (_i32, [_i32, _i32]),
    'sdsm_neighbour_slot': (_i64, [C.c_uint64, _i64]),
    'sdsm_neighbours': (_i32, [_i32, _i32, _vp, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_neighbours_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, _i32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _vp, C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64), _vp, _vp, _vp, _vp, _vp]),
    'sdsm_zones': (_i32, [_i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_zones_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_parts_quad': (_i32, [_i32, _i32, _i32, _i32, _i32]),
    'sdsm_parts_workspace_bytes_multi': (_sz, [C.POINTER(SetImage), _i32, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    'sdsm_parts': (_i32, [_i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'sdsm_parts_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, _i32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'sdsm_parts_table_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _vp, _vp]),
    'sdsm_parts_keep_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _vp, C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int32), _vp, _i32, _vp, _i64, _vp, _vp]),
    'sdsm_label_pixel_counts': (_i32, [_i32, _i32, _vp, _vp, _vp, _vp]),
    'sdsm_label_pixel_counts_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, _vp, _vp, _vp]),
    'sdsm_label_pixel_lists': (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_label_pixel_lists_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_pair_distances': (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp, _vp, _vp]),
    'sdsm_pair_distances_multi': (_i32, [C.POINTER(SetImage), _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp, _vp, _vp]),
    'sdsm_quantised_distance': (_i32, [_vp, _i64, _vp]),
    'sdsm_minsetcover': (_i32, [_i32, _i32, _vp, _vp, _f64, _i32, _i32, _f64, _vp, _vp]),
    'sdsm_minsetcover_multi': (_i32, [_i32, _vp, _vp, _vp, _vp, _f64, _i32, _i32, _f64, _vp, _vp]),
    'sdsm_maxsetpack': (_i32, [_i32, _i32, _vp, _vp, _vp, _vp]),
    'sdsm_count_growth': (_i32, [_i32, _vp, _vp, _vp, _i32, _i64, _vp]),
    'sdsm_unpack_fragments': (_i64, [_vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    'sdsm_plan_eval_param_count': (_i64, [_vp]),
    'sdsm_plan_eval_out_count': (_i64, [_vp]),
    'sdsm_batch_eval': (_i32, [_vp, _vp, _sz, _vp, _vp, _vp]),
    'sdsm_batch_eval_step': (_i32, [_vp, _vp, _sz, _i32, _f64, _f64, _f64, _vp, _vp, _vp, _i64, _vp]),
    'sdsm_probe_loss_arithmetic': (_i32, [_i64, _vp, _vp, _vp, _vp, _vp]),
    'sdsm_batch_deform_counts': (_i32, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    'sdsm_plan_set_start': (_i32, [_vp, _vp]),
    'sdsm_enable_kernel_timing': (_i32, [_i32]),
    'sdsm_last_solve_kernel_ms': (_f64, []),
    'sdsm_last_setup_kernel_ms': (_f64, []),
    'sdsm_set_solver_diagnostics': (_i32, [_i32]),
    'sdsm_batch_solver_counters': (_i32, [_vp, _vp, _vp]),
    'sdsm_set_debug_buffer': (_i32, [_vp]),
    'sdsm_set_group_timeout_us': (_i32, [_f64]),
    'sdsm_side_queues_distinct': (_i32, []),
    'sdsm_side_queue_report': (_i32, [_vp]),
    'sdsm_choose_sides_host': (_i32, [_i32, _vp, _i32, _vp]),
}

_lib = None


class SdsmError(RuntimeError):
    pass


def lib():
    """Loads libsdsm_hip.so and resolves every symbol of include/sdsm.h; raises if anything is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SdsmError(f'{LIB_PATH} is missing: build it with `python __graft_entry__.py` (hipcc, gfx950). '
                            'There is no CPU fallback for the DSM solve path.')
        # PyTorch-ROCm owns the device memory and ships its own HIP runtime (same SONAME as /opt/rocm's): it must be
        # loaded first so that this library binds to the SAME runtime instance instead of bringing up a second one.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)          # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
        assert L.sdsm_version() >= 200
        _lib = L
    return _lib


def check(code, what=''):
    if code != SDSM_OK:
        raise SdsmError(f'{what} failed ({code}): {lib().sdsm_last_error().decode()}')


def make_config(dsm_cfg):
    """dict with the reference's ``dsm/*`` keys (dsmcfg.py:6-21) -> sdsm_dsm_config."""
    d = dict(dsm_cfg)
    sa = d.get('smooth_amount', 10)
    return DsmConfig(scale=float(d.get('scale', 1000)), epsilon=float(d.get('epsilon', 1.0)), alpha=float(d.get('alpha', 0.5)),
                     smooth_amount=float(sa), gaussian_shape_multiplier=float(d.get('gaussian_shape_multiplier', 2)),
                     background_margin=float(d.get('background_margin', 20)), smooth_subsample=int(d.get('smooth_subsample', 20)),
                     init_elliptical=int(not callable(d.get('init', 'elliptical')) and d.get('init', 'elliptical') == 'elliptical'), max_iters=int(d.get('max_iters', 100)), flags=1 if d.get('no_trivial_rule') else 0)
