"""Device-side engine: thin Python over the C ABI (include/sdsm.h).

PyTorch-ROCm tensors own every device buffer; their ``data_ptr()`` and the current stream's handle are passed
to libsdsm_hip.so.  Nothing here computes on the CPU: if the HIP library or a GPU is missing, construction
fails loudly.
"""
import ctypes as C
import itertools
import os
import threading

import numpy as np
import torch

from . import _capi


def _require_gpu():
    if not torch.cuda.is_available():
        raise _capi.SdsmError('no HIP device available: the DSM solve path has no CPU fallback')


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def preprocess(g_raw, sigma1=np.sqrt(2), sigma2=40, offset_clip=3, lower_clip_mean=False, device=None, return_tensor=False):
    """Offset-intensity map ``y`` (reference: Preprocessing.process, superdsm/preprocess.py:39-68)."""
    _require_gpu()
    L = _capi.lib()
    dev = torch.device(device if device is not None else 'cuda')
    g = torch.as_tensor(np.ascontiguousarray(g_raw, dtype=np.float64)).to(dev) if not torch.is_tensor(g_raw) else g_raw.to(dev, torch.float64).contiguous()
    H, W = g.shape
    y = torch.empty_like(g)
    nbytes = L.sdsm_preprocess_workspace_bytes(H, W, float(sigma1), float(sigma2))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _capi.check(L.sdsm_preprocess(_ptr(g), H, W, float(sigma1), float(sigma2), float(offset_clip), int(bool(lower_clip_mean)),
                                      _ptr(y), _ptr(ws), nbytes, _stream()), 'sdsm_preprocess')
    return y if return_tensor else y.cpu().numpy()


PROBE_FIELDS = ('t', 'exp', 'log', 'softplus', 'phi', 'r', 'dcurv', 'rcp', 'rsqrt')      # SDSM_PROBE_* of include/sdsm.h


def probe_loss_arithmetic(y, S, x, device=None):
    """The scalar loss arithmetic of the solve kernels, element by element (sdsm_probe_loss_arithmetic, one launch): ``y``, ``S`` and
    ``x`` of one length n <= 2^20.  Returns a dict of float64 arrays named by PROBE_FIELDS; for parity tests."""
    _require_gpu()
    L = _capi.lib()
    dev = torch.device(device if device is not None else 'cuda')
    arrs = [np.ascontiguousarray(a, np.float64).ravel() for a in (y, S, x)]
    n = arrs[0].size
    if not all(a.size == n for a in arrs):
        raise ValueError('probe_loss_arithmetic: y, S and x must have one length')
    d_in = [torch.from_numpy(a).to(dev) for a in arrs]
    d_out = torch.empty(len(PROBE_FIELDS) * max(n, 1), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _capi.check(L.sdsm_probe_loss_arithmetic(n, _ptr(d_in[0]), _ptr(d_in[1]), _ptr(d_in[2]), _ptr(d_out), _stream()), 'sdsm_probe_loss_arithmetic')
    out = d_out.cpu().numpy()
    return {k: out[i * n:(i + 1) * n].copy() for i, k in enumerate(PROBE_FIELDS)}


class DeviceImage:
    """Per-image device state: y, atoms, the candidate-independent validity mask and per-atom extents.

    Replaces the per-candidate O(H*W) work of Object.get_cvxprog_region (superdsm/objects.py:95-128): the EDT
    term does not depend on the candidate and is evaluated once.
    """

    def __init__(self, y, y_mask, atoms, background_margin, device=None):
        _require_gpu()
        L = _capi.lib()
        self.device = torch.device(device if device is not None else 'cuda')
        as_dev = lambda a, dt: (a.to(self.device, dt).contiguous() if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(self.device))
        self.y = as_dev(y, torch.float64 if torch.is_tensor(y) else np.float64)
        self.atoms = as_dev(atoms, torch.int32 if torch.is_tensor(atoms) else np.int32)
        self.y_mask = None if y_mask is None else as_dev(y_mask, torch.uint8 if torch.is_tensor(y_mask) else np.uint8)
        self.H, self.W = (int(v) for v in self.y.shape)
        assert tuple(self.atoms.shape) == (self.H, self.W)
        self.background_margin = float(background_margin)
        self.n_atoms = int(self.atoms.max().item()) if self.atoms.numel() else 0
        self.valid = torch.empty((self.H, self.W), dtype=torch.uint8, device=self.device)
        stats = torch.empty(((self.n_atoms + 1) * _capi.ATOM_STATS_STRIDE,), dtype=torch.int32, device=self.device)
        nbytes = L.sdsm_image_workspace_bytes(self.H, self.W)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _capi.check(L.sdsm_image_prepare(_ptr(self.y), _ptr(self.y_mask), _ptr(self.atoms), self.H, self.W, self.background_margin,
                                             self.n_atoms, _ptr(self.valid), _ptr(stats), _ptr(ws), nbytes, _stream()), 'sdsm_image_prepare')
        self.atom_stats = np.ascontiguousarray(stats.cpu().numpy())       # host copy used by the planner (synchronises)


_PINNED = {}                       # (device type, index, stream) -> (records staging, masks staging): pinned, grown on demand, shared by the batches of a stream
_PINNED_LOCK = threading.Lock()


class PackedFragments:
    """The bit-packed region-bbox masks of one batch, kept on the host: fragment ``i`` is unpacked when somebody looks at it
    (``Object.fg_fragment``) -- most candidates of a generation are pruned by their energy alone."""

    def __init__(self, records, mask_info, mask_offset, masks):
        self.records, self.mask_info, self.mask_offset, self.masks = records, mask_info, mask_offset, masks

    def get(self, i):
        return fragments_from_masks(self.records[i:i + 1], self.mask_info[i:i + 1], self.mask_offset[i:i + 1], self.masks)[0][1]


def _empty_fragment(records):
    return (records['fg_h'] <= 0) | np.isin(records['status'], (_capi.CAND_TRIVIAL, _capi.CAND_ERROR, _capi.CAND_GIVEN_UP))


def fragments_from_masks(records, mask_info, mask_offset, masks, select=None, lazy=False):
    """Foreground fragments (bool arrays, views into one buffer) and offsets from downloaded records and bit-packed
    region-bbox masks (objects.py:148-174); ``select`` (bool per candidate) skips the others (``(None, None)``).  ``lazy``: the fragment
    as ``(PackedFragments, index)`` -- what ``Object.fg_fragment`` turns into the array on first access; ``masks`` is copied (it may be
    a view of a staging buffer)."""
    L = _capi.lib()
    n = len(records)
    records = np.ascontiguousarray(records)
    mask_info = np.ascontiguousarray(mask_info[:n], np.int32)
    mask_offset = np.ascontiguousarray(mask_offset[:n], np.int64)
    masks = np.ascontiguousarray(masks, np.uint8)
    if lazy and select is None:
        empty = _empty_fragment(records)
        origin = np.stack([np.where(empty, 0, records['fg_r0']), np.where(empty, 0, records['fg_c0'])], axis=1).astype(int)
        src = PackedFragments(records.copy(), mask_info.copy(), mask_offset.copy(), masks.copy())      # (the inputs may be views of staging buffers)
        return [(o, (src, i)) for i, o in enumerate(origin)]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    off = np.zeros(n + 1, np.int64)
    total = L.sdsm_unpack_fragments(ptr(records), ptr(mask_info), ptr(mask_offset), ptr(masks), n, None, ptr(off))
    if total < 0:
        raise _capi.SdsmError('sdsm_unpack_fragments: ' + L.sdsm_last_error().decode())
    buf = np.empty(max(total, 1), np.uint8)
    L.sdsm_unpack_fragments(ptr(records), ptr(mask_info), ptr(mask_offset), ptr(masks), n, ptr(buf), ptr(off))
    off[n] = total
    fb = buf.view(bool)
    empty = _empty_fragment(records)
    fh = np.where(empty, 1, records['fg_h']).tolist()
    fw = np.where(empty, 1, records['fg_w']).tolist()
    origin = np.stack([np.where(empty, 0, records['fg_r0']), np.where(empty, 0, records['fg_c0'])], axis=1).astype(int)
    offs = off.tolist()
    out = []
    for i in range(n):
        if select is not None and not select[i]:
            out.append((None, None))
        else:
            out.append((origin[i], fb[offs[i]:offs[i + 1]].reshape(fh[i], fw[i])))
    return out


def plan_mask_boxes(image, footprints, dsm_cfg):
    """Region bounding boxes (r0, c0, h, w) of candidates, [n, 4] int32: host-only planning from the per-atom statistics
    (sdsm_plan_create + sdsm_plan_describe; no device access).  ``image`` needs H, W, n_atoms, atom_stats, background_margin."""
    L = _capi.lib()
    n = len(footprints)
    offs = np.zeros(n + 1, np.int32)
    np.cumsum(np.fromiter(map(len, footprints), np.int64, n), out=offs[1:])
    labels = np.fromiter(itertools.chain.from_iterable(footprints), np.int32, int(offs[-1]))
    cfg = _capi.make_config(dict(dsm_cfg, background_margin=image.background_margin))
    stats = np.ascontiguousarray(image.atom_stats, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    plan = L.sdsm_plan_create(int(image.H), int(image.W), int(image.n_atoms), p(stats), C.byref(cfg), n, p(offs), p(labels))
    if not plan:
        raise _capi.SdsmError('sdsm_plan_create failed: ' + L.sdsm_last_error().decode())
    info = np.zeros((max(n, 1), 4), np.int32)
    _capi.check(L.sdsm_plan_describe(plan, p(info), None, None), 'sdsm_plan_describe')
    L.sdsm_plan_destroy(plan)
    return info[:n]


# Batches of fewer candidates than this leave most compute units idle: they run in latency mode (256 threads per candidate, regions of
# more than 3072 pixels split over workgroup groups) also when they span several images (lock-step generations of a small image set).
# (1024 until round 3: a lock-step batch of 588 candidates of 4 images then took 23.5 ms -- hundreds of group members, a compute unit
# each -- against 11.6 ms in throughput mode; 8 different BBBC039-like images: 14.4-15.7 -> 13.3-14.2 ms per image with 256.)
LATENCY_MODE_BELOW = int(os.environ.get('SDSM_LATENCY_BELOW', 256))


def mode_for(n_candidates):
    """Latency mode (1: shortest wall clock of ONE batch) for a batch that cannot fill the GPU, else throughput mode (0); same results."""
    return 1 if n_candidates < LATENCY_MODE_BELOW else 0


class Batch:
    """One ``compute_objects`` call: plan, workspace, launch, results.  ``image`` may be a list of :class:`DeviceImage` (a plan
    over several images, sdsm_plan_create_multi): ``image_of[i]`` then names the image of candidate ``i``.  The batch keeps what it was
    built from (``footprints``, ``dsm_cfg``, ``image_of``, ``start``): :meth:`resolve_given_up` builds its second attempt from them."""

    def __init__(self, image, footprints, dsm_cfg, want_xi=False, latency_mode=False, image_of=None, mode=None):
        """mode: 0 throughput (default), 1 latency (``latency_mode=True``: the largest regions get a group of 512-thread
        workgroups, shortest wall clock of ONE batch), 2 no workgroup groups (sdsm_plan_set_latency_mode)."""
        L = _capi.lib()
        self.images = list(image) if isinstance(image, (list, tuple)) else [image]
        self.image = self.images[0]
        assert 1 <= len(self.images) <= 16, 'a plan covers 1 .. 16 images'
        self.footprints, self.dsm_cfg, self.start = footprints, dsm_cfg, None
        self.n = len(footprints)
        lens = np.fromiter(map(len, footprints), np.int64, self.n)
        offs = np.zeros(self.n + 1, np.int32)
        np.cumsum(lens, out=offs[1:])
        labels = np.fromiter(itertools.chain.from_iterable(footprints), np.int32, int(offs[-1]))
        self.image_of = None if image_of is None else np.ascontiguousarray(image_of, np.int32)
        assert len(self.images) == 1 or (self.image_of is not None and len(self.image_of) == self.n)
        margins = {im.background_margin for im in self.images}
        assert len(margins) == 1, 'all images of a plan share the hyper-parameters'
        self.cfg = _capi.make_config(dict(dsm_cfg, background_margin=self.image.background_margin))
        ni = len(self.images)
        Hs = np.array([im.H for im in self.images], np.int32)
        Ws = np.array([im.W for im in self.images], np.int32)
        nas = np.array([im.n_atoms for im in self.images], np.int32)
        stats = (C.c_void_p * ni)(*[im.atom_stats.ctypes.data for im in self.images])
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self.plan = L.sdsm_plan_create_multi(ni, p(Hs), p(Ws), p(nas), stats, C.byref(self.cfg), self.n, p(offs), p(labels),
                                             p(self.image_of) if self.image_of is not None else None)
        if not self.plan:
            raise _capi.SdsmError('sdsm_plan_create failed: ' + L.sdsm_last_error().decode())
        self.mode = (1 if latency_mode else 0) if mode is None else int(mode)
        if self.mode:
            _capi.check(L.sdsm_plan_set_latency_mode(self.plan, self.mode), 'sdsm_plan_set_latency_mode')
        dev = self.image.device
        self.ws_bytes = L.sdsm_plan_workspace_bytes(self.plan)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.records_dev = torch.zeros(max(self.n, 1) * _capi.RECORD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.mask_bytes = L.sdsm_plan_mask_bytes(self.plan)
        self.masks_dev = torch.empty(self.mask_bytes, dtype=torch.uint8, device=dev)
        self.xi_dev = torch.zeros(L.sdsm_plan_xi_count(self.plan), dtype=torch.float64, device=dev) if want_xi else None
        self.mask_info = np.zeros((max(self.n, 1), 4), np.int32)
        self.mask_offset = np.zeros(max(self.n, 1), np.int64)
        self.n_pixels = np.zeros(max(self.n, 1), np.int32)
        _capi.check(L.sdsm_plan_describe(self.plan, p(self.mask_info), p(self.mask_offset), p(self.n_pixels)), 'sdsm_plan_describe')
        self.total_pixels = L.sdsm_plan_total_pixels(self.plan)
        self._ptrs = tuple((C.c_void_p * ni)(*[getattr(im, k).data_ptr() for im in self.images]) for k in ('y', 'atoms', 'valid'))
        with torch.cuda.device(dev):
            _capi.check(L.sdsm_batch_upload(self.plan, _ptr(self.ws), self.ws_bytes, _stream()), 'sdsm_batch_upload')

    def __del__(self):
        plan = getattr(self, 'plan', None)
        if plan and _capi is not None and _capi._lib is not None:
            _capi._lib.sdsm_plan_destroy(plan)
            self.plan = None

    def launch(self):
        """Queues the setup and solve kernels on the current stream (asynchronous)."""
        L = _capi.lib()
        with torch.cuda.device(self.image.device):
            _capi.check(L.sdsm_batch_launch_multi(self.plan, self._ptrs[0], self._ptrs[1], self._ptrs[2], _ptr(self.ws), self.ws_bytes,
                                                  _ptr(self.records_dev), _ptr(self.masks_dev), _ptr(self.xi_dev), _stream()), 'sdsm_batch_launch_multi')

    def deform_counts(self):
        """Number of columns of every candidate's G~ (its grid points; -1: no solve), from a run of the setup kernel alone
        (sdsm_batch_deform_counts; synchronises): what a callable ``dsm/init`` is called with (objects.py:385-386)."""
        L = _capi.lib()
        m = np.full(max(self.n, 1), -1, np.int32)
        with torch.cuda.device(self.image.device):
            _capi.check(L.sdsm_batch_deform_counts(self.plan, self._ptrs[0], self._ptrs[1], self._ptrs[2], _ptr(self.ws), self.ws_bytes,
                                                   m.ctypes.data_as(C.c_void_p), _stream()), 'sdsm_batch_deform_counts')
        return m[:self.n]

    def starting_points(self, init):
        """Callable ``dsm/init`` (objects.py:385-386): ``params = init(number of columns of G~)`` per candidate -- the count is a result of
        the setup kernel, which runs once on its own for it -- set as the starting points of the DSM solves (:meth:`set_start`).  Returns
        the list of vectors (None for candidates without a solve), or None if ``init`` is not callable."""
        if not callable(init):
            return None
        start = []
        for i, m in enumerate(self.deform_counts().tolist()):
            if m < 0:
                start.append(None)
                continue
            p = np.asarray(init(m), np.float64).ravel()
            if p.size != 6 + m or not np.all(np.isfinite(p)):
                raise ValueError(f'dsm/init({m}) must return {6 + m} finite parameters (candidate {i}: got {p.size})')
            start.append(p)
        self.set_start(start)
        return start

    def set_start(self, params):
        """Starting points of the DSM solves of the following launches (sdsm_plan_set_start): ``params[i]`` = theta (6,
        full-image-normalised) + xi (M) of candidate i, or None for a candidate without a solve.  Only for plans with
        ``init`` other than ``'elliptical'``.  Kept as ``self.start``."""
        L = _capi.lib()
        xo = self.xi_offsets()
        buf = np.zeros(L.sdsm_plan_eval_param_count(self.plan))
        for i, p in enumerate(params):
            if p is None:
                continue
            p = np.asarray(p, np.float64).ravel()
            buf[6 * i + xo[i]:6 * i + xo[i] + p.size] = p
        self.x0_dev = torch.from_numpy(buf).to(self.image.device)       # (kept alive by the batch)
        _capi.check(L.sdsm_plan_set_start(self.plan, _ptr(self.x0_dev)), 'sdsm_plan_set_start')
        self.start = list(params)

    def resolve_given_up(self, status=None):
        """The candidates of the last launch whose workgroup group was given up (SDSM_CAND_GIVEN_UP: a scheduling event on an oversubscribed
        GPU, not a solver failure) are solved again in one plan without groups (mode 2) from the same starting points; their record rows and
        mask bytes replace the first attempt's on the device.  ``status``: the statuses if the caller has downloaded them (else they are read
        on the device).  Returns their indices; with none, nothing is touched.  One that is given up again keeps that status."""
        if self.xi_dev is not None:
            raise _capi.SdsmError('resolve_given_up: not for a batch with want_xi (the xi of the second attempt are not copied back)')
        rows = lambda t: t.view(-1, _capi.RECORD_DTYPE.itemsize)
        if status is None:
            status = rows(self.records_dev)[:self.n].view(torch.int32)[:, _capi.RECORD_DTYPE.fields['status'][1] // 4].cpu().numpy()
        again = np.flatnonzero(np.asarray(status)[:self.n] == _capi.CAND_GIVEN_UP)
        if not again.size:
            return again
        sub = Batch(self.images if len(self.images) > 1 else self.image, [self.footprints[i] for i in again], self.dsm_cfg,
                    image_of=None if self.image_of is None else self.image_of[again], mode=2)
        if self.start is not None:
            sub.set_start([self.start[i] for i in again])
        sub.launch()
        with torch.cuda.device(self.image.device):
            rows(self.records_dev)[torch.from_numpy(again).to(self.image.device)] = rows(sub.records_dev)[:len(again)]
            for j, i in enumerate(again):
                nb = 4 * ((int(self.mask_info[i, 2]) * int(self.mask_info[i, 3]) + 31) // 32)
                o, so = int(self.mask_offset[i]), int(sub.mask_offset[j])
                self.masks_dev[o:o + nb] = sub.masks_dev[so:so + nb]
            torch.cuda.current_stream().synchronize()                      # (sub's buffers are released on return)
        return again

    def download(self):
        """Records and bit-packed masks to pinned host staging buffers: two asynchronous copies on the current stream, one
        synchronisation.  Returns (records structured array, masks uint8 array) -- VIEWS of the staging buffers, which are shared
        by all batches of the device AND STREAM and valid until the next download on it (copy what must live longer)."""
        dev = self.image.device
        key = (dev.type, dev.index, torch.cuda.current_stream(dev).cuda_stream)     # per stream: image groups in a pipeline download concurrently
        with _PINNED_LOCK:
            cur = _PINNED.get(key)
            need = (self.records_dev.numel(), self.masks_dev.numel())
            if cur is None or cur[0].numel() < need[0] or cur[1].numel() < need[1]:
                grow = lambda old, n: max(n, 2 * old) if old else max(n, 1 << 16)      # page-locking memory costs milliseconds: amortised
                cur = tuple(torch.empty(grow(0 if cur is None else cur[k].numel(), need[k]), dtype=torch.uint8).pin_memory() for k in range(2))
                _PINNED[key] = cur
        with torch.cuda.device(dev):
            cur[0][:need[0]].copy_(self.records_dev, non_blocking=True)
            cur[1][:need[1]].copy_(self.masks_dev, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        return cur[0].numpy()[:need[0]].view(_capi.RECORD_DTYPE)[:self.n], cur[1].numpy()[:need[1]]

    def solver_counters(self):
        """Event counters of the last launch (sdsm_batch_solver_counters; synchronises): full evaluations served from the sums kept
        at an unchanged iterate."""
        out = np.zeros(4, np.int64)
        with torch.cuda.device(self.image.device):
            _capi.check(_capi.lib().sdsm_batch_solver_counters(self.plan, _ptr(self.ws), out.ctypes.data_as(C.c_void_p)), 'sdsm_batch_solver_counters')
        return dict(evals_reused=int(out[0]))

    def records(self, rows=None):
        """The records on the host (synchronises); ``rows``: only those candidates'."""
        dev = self.records_dev if rows is None else self.records_dev.view(-1, _capi.RECORD_DTYPE.itemsize)[torch.from_numpy(rows).to(self.records_dev.device)]
        return dev.cpu().numpy().reshape(-1).view(_capi.RECORD_DTYPE)[:self.n].copy()

    def xi_offsets(self):
        off = np.zeros(max(self.n, 1), np.int64)
        _capi.check(_capi.lib().sdsm_plan_xi_offsets(self.plan, off.ctypes.data_as(C.c_void_p)), 'sdsm_plan_xi_offsets')
        return off

    def evaluate(self, params):
        """Point evaluation for parity tests (sdsm_batch_eval): ``params[i]`` = theta (6, full-image-normalised) + xi (M) of
        candidate i.  Needs a previous :meth:`launch`.  Returns a list of dicts: psi (full evaluator), psi_value
        (value-only evaluator), grad (6 + M), hess_theta (6 x 6, symmetric)."""
        L = _capi.lib()
        xo = self.xi_offsets()
        buf = np.zeros(L.sdsm_plan_eval_param_count(self.plan))
        for i, p in enumerate(params):
            p = np.asarray(p, np.float64)
            buf[6 * i + xo[i]:6 * i + xo[i] + p.size] = p
        dev = self.image.device
        d_par = torch.from_numpy(buf).to(dev)
        d_out = torch.empty(L.sdsm_plan_eval_out_count(self.plan), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _capi.check(L.sdsm_batch_eval(self.plan, _ptr(self.ws), self.ws_bytes, _ptr(d_par), _ptr(d_out), _stream()), 'sdsm_batch_eval')
        out = d_out.cpu().numpy()
        res = []
        for i, p in enumerate(params):
            m = len(p)
            H = np.zeros((6, 6))
            H[np.tril_indices(6)] = out[2 * self.n + 21 * i:2 * self.n + 21 * i + 21]
            H = H + np.tril(H, -1).T
            g0 = 23 * self.n + 6 * i + xo[i]
            res.append(dict(psi=float(out[2 * i]), psi_value=float(out[2 * i + 1]), grad=out[g0:g0 + m].copy(), hess_theta=H))
        return res

    STEP_LAYOUTS = ('class 1', 'class 1 latency', 'class 1b', 'class 2', 'class 2b', 'class 3', 'light')     # SDSM_STEP_LAYOUT_* of include/sdsm.h, in order

    def evaluate_step(self, layout, params, direction=None, reg_mu=0.0, tau=0.0, t0=1.0, dense=True):
        """One Newton step of the solver, piece by piece, in the layout of one solve class (sdsm_batch_eval_step; ``layout``: a name of
        ``STEP_LAYOUTS``): ``params[i]`` as for :meth:`evaluate`, ``direction`` (same shapes, or None) a search direction for the
        line-search sweep.  Needs a previous :meth:`launch`.  Returns a list of dicts, everything in the candidate's local frame, unknowns
        theta (6) then xi (M): ``rc`` (0 ok, 1 not positive definite, 2 non-finite, -1: not in this layout -- then nothing else),
        ``psi_value``, ``psi``, ``lam2``, ``line`` (4), ``grad``, ``dir`` (the Newton direction), ``env`` (the envelope as stored before
        the factorisation), ``rb``, ``fst``, ``rend`` (int32; envelope order: xi, then theta) and, expanded from those on the host,
        ``hess`` (dense, symmetric, theta first) with ``stored`` (which entries the envelope holds; :func:`expand_envelope`, None
        unless ``dense``)."""
        L = _capi.lib()
        xo = self.xi_offsets()
        states = self.inspect_states()
        need = [10 + 2 * (6 + s['M']) + (s['env_size'] if s['M'] > 0 else 21) + (2 * (6 + s['M']) + (s['M'] + 3) // 4 + 1) // 2 if s['status'] == 0 and s['M'] >= 0 else 10 for s in states]
        stride = max(need)

        def pack(vectors):
            buf = np.zeros(L.sdsm_plan_eval_param_count(self.plan))
            for i, p in enumerate(vectors):
                p = np.asarray(p, np.float64)
                buf[6 * i + xo[i]:6 * i + xo[i] + p.size] = p
            return torch.from_numpy(buf).to(self.image.device)
        d_par, d_dir = pack(params), (pack(direction) if direction is not None else None)
        d_out = torch.empty(self.n * stride, dtype=torch.float64, device=self.image.device)
        with torch.cuda.device(self.image.device):
            _capi.check(L.sdsm_batch_eval_step(self.plan, _ptr(self.ws), self.ws_bytes, self.STEP_LAYOUTS.index(layout), float(reg_mu), float(tau), float(t0),
                                               _ptr(d_par), _ptr(d_dir) if d_dir is not None else None, _ptr(d_out), stride, _stream()), 'sdsm_batch_eval_step')
        out = d_out.cpu().numpy().reshape(self.n, stride)
        res = []
        for i in range(self.n):
            b = out[i]
            if not b[0] >= 0:
                res.append(dict(rc=-1))
                continue
            n, E = int(b[4]), int(b[5])
            M = n - 6
            ints = b[10 + 2 * n + E:need[i]].view(np.int32)
            rb, fst, rend = ints[:n].copy(), ints[n:2 * n].copy(), ints[2 * n:2 * n + (M + 3) // 4].copy()
            env = b[10 + 2 * n:10 + 2 * n + E].copy()
            hess, stored = expand_envelope(env, rb, fst) if dense else (None, None)
            res.append(dict(rc=int(b[0]), psi_value=float(b[1]), psi=float(b[2]), lam2=float(b[3]), line=b[6:10].copy(), grad=b[10:10 + n].copy(),
                            dir=b[10 + n:10 + 2 * n].copy(), env=env, rb=rb, fst=fst, rend=rend, hess=hess, stored=stored))
        return res

    def inspect_states(self):
        """The per-candidate state words of the setup kernel (M, status, envelope size, runs) without the crops / rows of :meth:`inspect`."""
        lay = self.layout()
        state = self.ws[lay['state']:lay['state'] + lay['state_size'] * self.n].cpu().numpy().view(_capi.CAND_STATE_DTYPE)
        return [{f: int(r[f]) for f in ('M', 'status', 'zmax', 'hzmax', 'env_size', 'NR')} for r in state]

    def layout(self):
        """The values of sdsm_plan_layout by name (_capi.PLAN_LAYOUT_NAMES): byte offsets of workspace blocks, then sizes and counts."""
        lay = np.zeros(len(_capi.PLAN_LAYOUT_NAMES), np.int64)
        _capi.check(_capi.lib().sdsm_plan_layout(self.plan, lay.ctypes.data_as(C.c_void_p)), 'sdsm_plan_layout')
        lay = dict(zip(_capi.PLAN_LAYOUT_NAMES, lay.tolist()))
        assert lay['cand_size'] == _capi.CAND_DESC_DTYPE.itemsize and lay['state_size'] == _capi.CAND_STATE_DTYPE.itemsize
        return lay

    def inspect(self):
        """Setup-phase outputs for parity tests: per candidate (N, M, status, pixel coordinates, grid points,
        CSR-like G~ rows and, in ``lead``, which of a row's entries are LEADING ones -- those the approximate Hessian of the solver uses; ``hnz`` counts
        them per pixel, ``run_hnz`` per run, ``hzmax`` is the setup kernel's maximum over the runs), reconstructed PER PIXEL from the run-packed crop (a run = the region pixels of one image row inside one
        aligned 4-column cell; an entry of a run holds the weights of its four pixels for one grid point).  Reads the workspace back
        to the host."""
        lay = self.layout()
        ws = self.ws.cpu().numpy()
        zcap, nell, nruns = lay['zcap_run'], lay['total_ell'], lay['total_runs']
        block = lambda name, dtype, count: ws[lay[name]:lay[name] + np.dtype(dtype).itemsize * count].view(dtype)
        cand, state = block('cand', _capi.CAND_DESC_DTYPE, self.n), block('state', _capi.CAND_STATE_DTYPE, self.n)
        crop_y = block('crop_y', np.float64, 4 * nruns).reshape(-1, 4)
        crop_rc, run_meta = block('crop_rc', np.uint32, nruns), block('run_meta', np.uint32, nruns)
        xi_off = self.xi_offsets()
        grid = ws[lay['grid_rc']:].view(np.uint32)
        ell_im = block('ell_im', np.uint32, nell)
        ell_w = block('ell_w', np.float32, 4 * nell).reshape(-1, 4)
        out = []
        for i in range(self.n):
            N = int(self.n_pixels[i])
            M, status, hc, wc, npos, NR = (int(state[i][f]) for f in ('M', 'status', 'hc', 'wc', 'npos', 'NR'))
            ro, eo = int(cand[i]['run_off']), int(cand[i]['ell_off'])
            g = grid[xi_off[i]:xi_off[i] + M]
            have_runs = status == 0 and NR > 0
            meta = run_meta[ro:ro + NR] if have_runs else np.zeros(0, np.uint32)
            rnnz, rhz, pm = (meta & 0xfff).astype(np.int64), ((meta >> 12) & 0xfff).astype(np.int64), (meta >> 24).astype(np.int64)
            rc = crop_rc[ro:ro + len(meta)]
            rows, cols, ys, nnzs, hnzs, idxs, wts, leads = [], [], [], [], [], [], [], []
            zc = max(zcap, 1)
            for p in range(len(meta)):
                k = int(rnnz[p]) if M > 0 else 0
                im = ell_im[eo + np.arange(k) * NR + p] if k else np.zeros(0, np.uint32)
                w4 = ell_w[eo + np.arange(k) * NR + p] if k else np.zeros((0, 4), np.float32)
                for q in range(4):
                    if not (pm[p] >> q) & 1:
                        continue
                    rows.append(int(rc[p] >> 16)); cols.append(int(rc[p] & 0xffff) + q); ys.append(crop_y[ro + p, q])
                    sel = w4[:, q] != 0                                  # a grid point outside the pixel's window: weight 0
                    ci, cw = (im[sel] & 0xffff).astype(np.int64), w4[sel, q]
                    o2 = np.argsort(ci, kind='stable')                   # report rows by column index
                    col = np.zeros(zc, np.int64); wt = np.zeros(zc, np.float32); ld = np.zeros(zc, bool)
                    col[:len(ci)] = ci[o2]; wt[:len(ci)] = cw[o2]; ld[:len(ci)] = (((im[sel] >> (16 + q)) & 1) != 0)[o2]
                    idxs.append(col); wts.append(wt); nnzs.append(len(ci)); leads.append(ld)
                    hnzs.append(int((((im >> (16 + q)) & 1) != 0).sum()))
            rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
            o = np.lexsort((cols, rows))                                   # the crop is stored by runs in sorted scatter order; report it in raster order
            take = lambda a, dt: (np.asarray(a, dt)[o] if len(a) else np.zeros(0, dt))
            idx = np.stack(idxs, axis=1)[:, o] if idxs else np.zeros((zc, 0), np.int64)
            w = np.stack(wts, axis=1)[:, o] if wts else np.zeros((zc, 0), np.float32)
            lead = np.stack(leads, axis=1)[:, o] if leads else np.zeros((zc, 0), bool)
            out.append(dict(N=N, M=M, status=status, hc=hc, wc=wc, npos=npos, zmax=int(state[i]['zmax']), env_size=int(state[i]['env_size']), NR=NR,
                            y=take(ys, np.float64), r=rows[o] if len(rows) else rows, c=cols[o] if len(cols) else cols,
                            grid_r=(g >> 16).astype(np.int64), grid_c=(g & 0xffff).astype(np.int64), nnz=take(nnzs, np.int64), hnz=take(hnzs, np.int64),
                            run_nnz=rnnz.copy(), run_hnz=rhz.copy(), run_pixels=np.array([bin(int(v)).count('1') for v in pm], np.int64),
                            idx=idx.copy(), w=w.copy(), lead=lead.copy(), hzmax=int(state[i]['hzmax'])))
        return out

    def fragments(self, records, select=None, masks=None, lazy=False):
        """Foreground fragments (bool arrays) and offsets, cropped from the bit-packed region-bbox masks."""
        if masks is None:
            masks = self.masks_dev.cpu().numpy()
        return fragments_from_masks(records, self.mask_info, self.mask_offset, masks, select, lazy)


def expand_envelope(env, rb, fst):
    """The envelope of sdsm_batch_eval_step (row a of the order xi[M], theta[6] holds columns fst[a] .. a at env[rb[a] + column]) as a
    dense symmetric matrix with the unknowns in the order theta, xi, and the mask of the entries the envelope holds."""
    n = len(rb)
    M = n - 6
    var = np.concatenate([6 + np.arange(M), np.arange(6)])              # envelope order -> variable order
    hess, stored = np.zeros((n, n)), np.zeros((n, n), bool)
    for a in range(n):
        cols = np.arange(fst[a], a + 1)
        hess[var[a], var[cols]] = hess[var[cols], var[a]] = env[rb[a] + cols]
        stored[var[a], var[cols]] = stored[var[cols], var[a]] = True
    return hess, stored


def algorithmic_bytes(records, mask_info):
    """bytes_c = E_c (12 N_c + 8 (6 + M_c)) + 12 N_c + ceil(bbox_c / 8) + 128."""
    E = records['evals_value'].astype(np.int64) + records['evals_full'].astype(np.int64)
    N = records['n_pixels'].astype(np.int64)
    M = records['n_deform'].astype(np.int64)
    bbox = (mask_info[:len(records), 2].astype(np.int64) * mask_info[:len(records), 3].astype(np.int64) + 7) // 8
    return int((E * (12 * N + 8 * (6 + M)) + 12 * N + bbox + 128).sum())
