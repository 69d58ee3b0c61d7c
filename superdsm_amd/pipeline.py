"""Stage / Pipeline plugin API (reference: superdsm/pipeline.py:10-265), restated so that the GPU stages drop
into a SuperDSM-style pipeline: same constructor, ``process`` contract, ``configure_ex`` factors, callbacks,
``first_stage`` / ``last_stage`` re-entry and input/output driven ordering."""
import math
import os
import time

from .image import normalize_image
from .output import get_output


class Stage:
    """A pipeline stage: declares ``inputs`` / ``outputs`` and implements ``process``."""

    ENABLED_BY_DEFAULT = True

    def __init__(self, name, cfgns=None, inputs=(), outputs=()):
        self.name = name
        self.cfgns = name if cfgns is None else cfgns
        self.inputs = {key: key for key in inputs}
        self.outputs = {key: key for key in outputs}
        self._callbacks = {}

    def add_callback(self, name, cb):
        self._callbacks.setdefault(name, []).append(cb)

    def remove_callback(self, name, cb):
        if name in self._callbacks:
            self._callbacks[name].remove(cb)

    def _callback(self, name, *args, **kwargs):
        for cb in self._callbacks.get(name, ()):
            cb(name, *args, **kwargs)

    def __call__(self, data, cfg, out=None, log_root_dir=None):
        out = get_output(out)
        cfg = cfg.get(self.cfgns, {})
        if not cfg.get('enabled', self.ENABLED_BY_DEFAULT):
            out.write(f'Skipping disabled stage "{self.name}"')
            self._callback('skip', data)
            return 0
        out.intermediate(f'Starting stage "{self.name}"')
        self._callback('start', data)
        stage_input = {inner: data[outer] for outer, inner in self.inputs.items()}
        t0 = time.time()
        produced = self.process(stage_input, cfg=cfg, out=out, log_root_dir=log_root_dir)
        dt = time.time() - t0
        assert set(produced.keys()) == set(self.outputs), 'stage "%s" generated unexpected output' % self.name
        for inner, outer in self.outputs.items():
            data[outer] = produced[inner]
        self._callback('end', data)
        return dt

    def process(self, input_data, cfg, out, log_root_dir):
        raise NotImplementedError()

    def configure(self, scale):
        radius = scale * math.sqrt(2)
        return self.configure_ex(scale, radius, 2 * radius)

    def configure_ex(self, scale, radius, diameter):
        return {}


class Pipeline:

    def __init__(self):
        self.stages = []

    def find(self, stage_name, not_found_dummy=float('inf')):
        names = [stage.name for stage in self.stages]
        return names.index(stage_name) if stage_name in names else not_found_dummy

    def append(self, stage, after=None):
        if after is None:
            self.stages.append(stage)
        else:
            pos = self.find(after) if isinstance(after, str) else after
            self.stages.insert(pos + 1, stage)

    def init(self, g_raw, cfg):
        data = {}
        if cfg.get('histological', False):
            data['g_rgb'] = g_raw
            g_raw = g_raw.mean(axis=2)
            g_raw = g_raw.max() - g_raw
        data['g_raw'] = normalize_image(g_raw)
        return data

    def _stage_range(self, first_stage, last_stage):
        """``first_stage`` with its ``+`` suffix resolved (the stage after the named one) and the stages that run from it (None: from
        the pipeline's first) up to and including ``last_stage`` (None: to the end); no stages if the range is inverted."""
        if first_stage is not None and first_stage.endswith('+'):
            first_stage = self.stages[1 + self.find(first_stage[:-1])].name
        if first_stage is not None and last_stage is not None and self.find(first_stage) > self.find(last_stage):
            return first_stage, []
        running, selected = first_stage is None, []
        for stage in self.stages:
            if not running and stage.name == first_stage:
                running = True
            if running:
                selected.append(stage)
            if stage.name == last_stage:
                running = False
        return first_stage, selected

    def _from_scratch(self, first_stage, data):
        """Whether an image starts with ``init``: no first stage, or the pipeline's first stage and no data to go on from."""
        return first_stage is None or (first_stage == self.stages[0].name and data is None)

    def process_image(self, g_raw, cfg, first_stage=None, last_stage=None, data=None, out=None, log_root_dir=None):
        cfg = cfg.copy()
        if log_root_dir is not None:
            os.makedirs(log_root_dir, exist_ok=True)
        first_stage, stages = self._stage_range(first_stage, last_stage)
        if not stages:
            return data, cfg, {}
        out = get_output(out)
        if self._from_scratch(first_stage, data):
            data = self.init(g_raw, cfg)
        else:
            assert data is not None, 'data argument must be provided if first_stage is used'
        timings = {stage.name: stage(data, cfg, out=out, log_root_dir=log_root_dir) for stage in stages}
        return data, cfg, timings

    def process_images(self, g_raws, cfg, first_stage=None, last_stage=None, datas=None, out=None, log_root_dirs=None):
        """``process_image`` for a set of images: returns one ``(data, cfg, timings)`` per image, equal to what ``process_image``
        returns for that image (``cfg``, ``datas`` and ``log_root_dirs``: one for all or one per image).  ``first_stage`` /
        ``last_stage`` (with the ``+`` suffix), ``histological``, the stages' ``enabled`` setting and the ``start`` / ``end`` /
        ``skip`` callbacks (fired per image) mean what they mean there.  A stage with a ``process_many`` runs once for the images it
        is enabled for; its wall time is shared evenly among their ``timings``.  The other stages run image by image.

        An image that fails in a stage (``C2FError``, ``CvxprogError``) leaves the set and the others finish; then the failure of the
        lowest image index is raised with ``image_index``, ``image_indices`` (every failed image) and ``results`` (everyone's
        ``(data, cfg, timings)`` so far).  Other exceptions end the call at once."""
        from .c2freganal import C2FError
        from .objects import CvxprogError
        g_raws = list(g_raws)
        n = len(g_raws)
        if n == 0:
            return []
        per_image = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n
        cfgs = [c.copy() for c in per_image(cfg)]
        datas = per_image(datas)
        logs = per_image(log_root_dirs)
        assert len(cfgs) == len(datas) == len(logs) == n, 'one config, data and log directory per image'
        for log in logs:
            if log is not None:
                os.makedirs(log, exist_ok=True)
        first_stage, stages = self._stage_range(first_stage, last_stage)
        if not stages:
            return [(data, c, {}) for data, c in zip(datas, cfgs)]
        out = get_output(out)
        for i in range(n):
            if self._from_scratch(first_stage, datas[i]):
                datas[i] = self.init(g_raws[i], cfgs[i])
            else:
                assert datas[i] is not None, 'data argument must be provided if first_stage is used'
        timings = [{} for _ in range(n)]
        errors = {}
        for stage in stages:
            live = [i for i in range(n) if i not in errors]
            if hasattr(stage, 'process_many'):
                enabled = []
                for i in live:
                    if cfgs[i].get(stage.cfgns, {}).get('enabled', stage.ENABLED_BY_DEFAULT):
                        enabled.append(i)
                    else:
                        timings[i][stage.name] = stage(datas[i], cfgs[i], out=out, log_root_dir=logs[i])    # skips it
                if not enabled:
                    continue
                for i in enabled:
                    out.intermediate(f'Starting stage "{stage.name}"')
                    stage._callback('start', datas[i])
                # the stage writes its outputs into copies: an image without them afterwards has failed
                outer = set(stage.outputs.values())
                subs = [{k: v for k, v in datas[i].items() if k not in outer} for i in enabled]
                t0 = time.time()
                try:
                    dt, error = stage.process_many(subs, [cfgs[i] for i in enabled], out=out, log_root_dirs=[logs[i] for i in enabled]), None
                except (C2FError, CvxprogError) as e:
                    dt, error = time.time() - t0, e
                for j, i in enumerate(enabled):
                    timings[i][stage.name] = dt / len(enabled)
                    if outer <= set(subs[j]):
                        for key in outer:
                            datas[i][key] = subs[j][key]
                        stage._callback('end', datas[i])
                    else:
                        assert error is not None, f'stage "{stage.name}" generated no output for image {i}'
                        errors[i] = getattr(error, 'image_errors', {}).get(j, error)
            else:
                for i in live:
                    try:
                        timings[i][stage.name] = stage(datas[i], cfgs[i], out=out, log_root_dir=logs[i])
                    except (C2FError, CvxprogError) as e:
                        errors[i] = e
        results = [(data, c, t) for data, c, t in zip(datas, cfgs, timings)]
        if errors:
            first = min(errors)
            e = errors[first]
            e.image_index, e.image_indices, e.results = first, sorted(errors), results
            raise e
        return results


def create_pipeline(stages):
    """Orders ``stages`` so that every stage's inputs are produced before it runs (``g_raw`` is given)."""
    available = {'g_raw'}
    pending = list(stages)
    pipeline = Pipeline()
    while pending:
        ready = next((s for s in pending if set(s.inputs) <= available), None)
        if ready is None:
            raise ValueError('failed to resolve total ordering')
        pending.remove(ready)
        pipeline.append(ready)
        available |= set(ready.outputs)
    return pipeline


def create_default_pipeline(extra_stages=()):
    """Preprocessing -> DSM_Config -> [extra stages, e.g. a region-analysis stage producing ``atoms`` and
    ``adjacencies``] -> GlobalEnergyMinimization.  The reference's C2F region analysis and post-processing stages
    are part of this package too (``c2freganal.C2F_RegionAnalysis``, ``postprocess.Postprocessing``, both with their per-image work
    on the GPU): ``create_reference_pipeline`` chains all five."""
    from .dsmcfg import DSM_Config
    from .globalenergymin import GlobalEnergyMinimization
    from .preprocess import Preprocessing
    return create_pipeline([Preprocessing(), DSM_Config(), *extra_stages, GlobalEnergyMinimization()])


def create_reference_pipeline():
    """The reference's five stages (superdsm/pipeline.py:268-285): Preprocessing -> DSM_Config -> C2F_RegionAnalysis ->
    GlobalEnergyMinimization -> Postprocessing."""
    from .c2freganal import C2F_RegionAnalysis
    from .dsmcfg import DSM_Config
    from .globalenergymin import GlobalEnergyMinimization
    from .postprocess import Postprocessing
    from .preprocess import Preprocessing
    return create_pipeline([Preprocessing(), DSM_Config(), C2F_RegionAnalysis(), GlobalEnergyMinimization(), Postprocessing()])
