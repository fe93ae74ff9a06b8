"""Replay of a pipeline evaluation without the per-container Stage bookkeeping.

`Pipeline.get_outputs()` of the reference runs every stage's `compute()` / `apply()` on host
arrays (pisa/core/pipeline.py:537-558, stage.py:536-586).  This build's stages do the same through
device columns and deferred operations -- ~6 000 Python calls, 0.8 ms per evaluation -- although,
for the chain
    loader -> [flux ...] -> osc.prob3 (2-D calc grid) -> aeff.aeff -> utils.hist [-> discr_sys.hypersurfaces]
an evaluation is a handful of kernel launches.

After one ordinary evaluation that took the fused path, `FastPlan` replays exactly those
launches: it compares the parameter change counters (`Param.clock`, `Param._ver`) with what it
saw last and, per stage that moved,
  * osc.prob3: rebuilds the matrices through the stage's own `_matrices()` and launches the planned
    prob3 kernels;
  * aeff.aeff: refreshes the containers' scales through the stage's own `scale_for()`;
  * flux stages, when the flux lives on the oscillation grid (engine.node_flux): runs the moved
    stage(s) on the grid nodes and hands the new node fluxes to the engine (`hist.sync_node_flux`);
  * ONE flux.barr_simple stage with the flux per event (example.cfg's shape): the engine's one-pass
    refresh of the folded flux columns (`HotPathEngine.update_flux_barr`), the stage's own `nu_flux`
    arrays being recomputed only if somebody reads them;
  * discr_sys.hypersurfaces behind the histogram: runs its `compute()` (per-bin factors on the
    host) and passes the factors to the tail kernel (`pisa_hip_finalize_metric_scaled`);
then launches the fused kernel and hands out device-backed Maps (`DeviceMapBlock`).  Anything else
-- a loader parameter or a per-event flux of another shape moved, a Ye value moved, another output key or binning is
asked for, profiling is on, somebody wrote one of the pipeline's containers or reads `pipeline.data`
-- goes through the ordinary Stage protocol, which stays the source of truth (the plan is rebuilt
afterwards).  The bypassed stages' compute memos are invalidated, so the ordinary path never trusts
tables the plan has overwritten.  `PISA_PLAN_DEBUG=1` prints why an evaluation was not replayed.
"""
import ctypes as C
import os
import weakref

import numpy as np

from pisa_amd import _lib
from pisa_amd import kernels as K
from pisa_amd.core.container import Container
from pisa_amd.core.map import Map, MapSet
from pisa_amd.core.param import Param, ParamSet

__all__ = ["FastPlan", "DeviceMapBlock", "DeviceMapSet"]

_DEBUG = bool(os.environ.get("PISA_PLAN_DEBUG"))


class DeviceMapBlock:
    """The maps (and sum of squared weights) of all containers of ONE evaluation, still in HBM."""

    def __init__(self, engine, with_errors, scales=None):
        self.engine = engine
        self.with_errors = with_errors
        # per-(container, bin) factors of a stage behind the histogram (discr_sys.hypersurfaces):
        # device tensor [n_cont, n_bins]; maps = clip(hist * s, 0, inf), errors = sqrt(sumw2) * s
        self.scales = scales
        self.full = (1 << len(engine.cont)) - 1
        self.n_rows = len(engine.cont)
        self._host = None
        self._live = True   # the engine still holds this evaluation
        self._views = {}
        self.rows_published = False   # the hist stage handed rows of this block to the containers

    def detach(self):
        """the engine is about to start another evaluation"""
        if self._host is None and self._live:
            self._fetch()
        self._live = False

    def _fetch(self):
        eng = self.engine
        hist, sumw2 = eng.finalize()
        import torch

        if self.scales is not None:
            # as the stage does it: weights = clip(weights * s, 0, inf), errors = sqrt(sumw2) * s
            sc = self.scales.reshape(hist.shape)
            err = torch.sqrt(sumw2) * sc
            hist, sumw2 = torch.clamp(hist * sc, min=0.0), err * err
        if self.with_errors or self._views or self.rows_published:
            both = torch.stack((hist, sumw2)).cpu().numpy()
            self._host = (both[0], both[1])
        else:
            self._host = (hist.cpu().numpy(), None)
        eng.check_status()

    # -- rows handed to the containers by the hist stage (core/container.py: BlockRow) ---------------
    def row_host(self, row, which):
        """host array of one container's map: which = 0 sum(w), 1 sqrt(sum(w^2)), 2 sum(1^2 w) = sum(w)
        (utils/hist.py:198-209); all rows of the block come home in ONE transfer, at the first request"""
        if self._host is None:
            if not self._live:
                raise RuntimeError("device-backed maps outlived their evaluation")
            self._fetch()
        hist, sumw2 = self._host
        return np.sqrt(sumw2[row]) if which == 1 else hist[row].copy()

    def row_dev(self, row, which):
        """the same row as a device tensor: a view of the engine's finalized maps while the evaluation is
        still the engine's, an upload of the host copy afterwards"""
        import torch

        if self._live and self._host is None:
            hist, sumw2 = self.engine.finalize()
            return torch.sqrt(sumw2[row]) if which == 1 else hist[row].clone()
        return K.to_device(self.row_host(row, which))

    def view(self, with_errors):
        """this block as maps with / without variances (the pipeline's output_key decides, not the stage
        that made the block): the block itself or a cached sibling sharing everything else"""
        if bool(with_errors) == bool(self.with_errors):
            return self
        v = self._views.get(bool(with_errors))
        if v is None:
            v = self._views[bool(with_errors)] = _BlockView(self, bool(with_errors))
        return v

    def host_sum(self, mask, shape, with_errors=None):
        if self._host is None:
            if not self._live:
                raise RuntimeError("device-backed maps outlived their evaluation")
            self._fetch()
        hist, sumw2 = self._host
        if not (self.with_errors if with_errors is None else with_errors):
            sumw2 = None
        rows = [i for i in range(hist.shape[0]) if mask >> i & 1]
        h = hist[rows[0]].copy()
        v = None if sumw2 is None else sumw2[rows[0]].copy()
        for i in rows[1:]:       # index order = the order in which sum() adds Maps
            h += hist[i]
            if v is not None:
                v += sumw2[i]
        return h.reshape(shape), None if v is None else v.reshape(shape)

    def metric(self, mask, kind, data_hist, extra=None, with_errors=None):
        """metric of the TOTAL template against `data_hist` on the device, or None if this block
        cannot provide it (partial sum, already fetched, no longer the engine's evaluation).
        `extra` = (hist, variances or None) host arrays added to the template after the containers."""
        if mask != self.full or not self._live or self._host is not None or kind not in K.METRIC_KIND:
            return None
        if kind == "mod_chi2" and not (self.with_errors if with_errors is None else with_errors):
            return None
        eng = self.engine
        extra_d = None
        if self.scales is not None or extra is not None:
            if not eng.can_fuse_tail():
                return None
            if extra is not None:
                eh = np.asarray(extra[0], dtype=np.float64).ravel()
                ev = np.zeros_like(eh) if extra[1] is None else np.asarray(extra[1], dtype=np.float64).ravel()
                extra_d = eng.upload_extra(np.stack((eh, ev)))
        eng.set_data_cached(np.ascontiguousarray(data_hist, dtype=np.float64).ravel())
        val = eng.tail_host(kind, self.scales, extra_d)
        if val != val:   # NaN: a negative input sets the status word too (stats.py:231-240 raises)
            st = eng.metric_status_host()
            if st != 0:
                _lib.check(st)
        return val


class _BlockView:
    """a DeviceMapBlock seen with the other setting of `with_errors` (see DeviceMapBlock.view)"""

    __slots__ = ("block", "with_errors", "full")

    def __init__(self, block, with_errors):
        self.block, self.with_errors, self.full = block, with_errors, block.full

    def host_sum(self, mask, shape):
        return self.block.host_sum(mask, shape, with_errors=self.with_errors)

    def metric(self, mask, kind, data_hist, extra=None):
        return self.block.metric(mask, kind, data_hist, extra, with_errors=self.with_errors)


class DeviceMapSet(MapSet):
    """MapSet over the rows of a `DeviceMapBlock`; the Map objects are made when first asked for,
    and `total()` -- what `sum(mapset)` gives -- is available without making them"""

    def __init__(self, names, binning, block, name=None):
        self._names, self._binning, self._block = list(names), binning, block
        self._maps = None
        self.name, self.tex, self.collate_by_name = name, None, True

    @property
    def maps(self):
        if self._maps is None:
            self._maps = [Map.device_backed(n, self._binning, self._block, 1 << i)
                          for i, n in enumerate(self._names)]
        return self._maps

    @maps.setter
    def maps(self, value):
        self._maps = list(value)

    names = property(lambda self: list(self._names) if self._maps is None else [m.name for m in self._maps])

    def __len__(self):
        return len(self._names) if self._maps is None else len(self._maps)

    def total(self, name="total"):
        if self._maps is None:
            return Map.device_backed(name, self._binning, self._block, self._block.full)
        out = sum(self._maps)
        out.name = name
        return out

    # copies and pickles are ordinary host MapSets (see Map.__getstate__): the block -- and through
    # it the engine with its HBM tensors and ctypes pointers -- is never copied
    def __reduce_ex__(self, protocol):
        return (MapSet, (list(self.maps), self.name))

    def __deepcopy__(self, memo):
        import copy

        out = MapSet([copy.deepcopy(m, memo) for m in self.maps], name=self.name)
        memo[id(self)] = out
        return out


def _no(reason):
    """ordinary path; PISA_PLAN_DEBUG=1 says why"""
    if _DEBUG:
        print("[evaluation plan] ordinary path:", reason)
    return None


class FastPlan:
    @classmethod
    def build(cls, pipeline):
        """a plan for `pipeline`, or None if its last evaluation did not have the replayable shape:
        loader -> [flux ...] -> osc.prob3 -> aeff.aeff -> utils.hist [-> discr_sys.hypersurfaces]"""
        stages = pipeline._stages
        if not stages or pipeline._profile:
            return None
        ih = [k for k, s in enumerate(stages) if s.service_name == "hist"]
        if len(ih) != 1:
            return _no("no single hist stage")
        hist = stages[ih[0]]
        if not getattr(hist, "fused_last_eval", False):
            return _no("hist stage did not take the fused path")
        post = stages[ih[0] + 1:]
        for s in post:
            # per-bin scale factors behind the histogram: weights = clip(weights * s, 0, inf),
            # errors *= s (hypersurfaces.py:251-259); the uncertainty-propagating variant is not replayed
            if s.service_name != "hypersurfaces" or s.propagate_uncertainty:
                return _no("stage %s after the histogram" % s.service_name)
        osc = [s for s in stages if s.service_name == "prob3"]
        aeff = [s for s in stages if s.service_name == "aeff" and s.stage_name == "aeff"]
        if len(osc) != 1 or len(aeff) != 1 or osc[0].grid is None or hist._engine is None:
            return _no("no prob3 grid / aeff / engine")
        if osc[0].tomography_type is not None:
            return _no("tomography")   # may rebuild the layer plan inside _matrices(): ordinary path only
        if hist._engine.world_size > 1 and hist._engine.n_bins * len(hist._engine.cont) > K.FINALIZE_METRIC_MAX:
            return _no("maps too large for the fused tail on several ranks")
        key = pipeline.output_key
        if key not in ("weights", ("weights", "errors")):
            return _no("output key %r" % (key,))
        if key != "weights" and hist.error_method != "sumw2":
            return _no("errors without sumw2")
        if post and (len(post) != 1 or key == "weights" or any(s.error_method != "sumw2" for s in post)):
            return _no("post-histogram stages not in the supported shape")
        return cls(pipeline, osc[0], aeff[0], hist, post)

    def __init__(self, pipeline, osc, aeff, hist, post=()):
        self.pipeline, self.osc, self.aeff, self.hist = pipeline, osc, aeff, hist
        self.post = list(post)
        self.engine = hist._engine
        self.with_errors = pipeline.output_key != "weights"
        self.binning = pipeline.output_binning
        self.names = [c.name for c in hist.data.containers]
        stages = pipeline._stages
        # flux stages (between the loader and prob3) can be replayed when the flux lives on the
        # oscillation grid: a stage run on 2e4 nodes per container and new node tables, no pass over
        # the events (stages/utils/hist.py, engine.node_flux)
        k_osc = stages.index(osc)
        self.flux_stages = [s for s in stages[:k_osc] if s.stage_name == "flux"] if self.engine.node_flux else []
        # flux held per event and ONE flux.barr_simple stage in an event representation in front of the
        # oscillation (example.cfg's shape): a moved Barr parameter is replayed as the engine's one-pass
        # refresh of the folded flux columns (`update_flux_barr`: nominal fluxes and parameter-free factors
        # in resident order -> folded column, the bits of the stage's launch + the hist stage's fold)
        self.barr_stage, self._barr_ready = None, False
        if not self.engine.node_flux:
            fl = [s for s in stages[:k_osc] if s.stage_name == "flux"]
            if (len(fl) == 1 and fl[0].service_name == "barr_simple" and fl[0].calc_mode == "events"
                    and all(w is not None for w in self.engine._wflux)):
                self.barr_stage = fl[0]
        # one flat list of (param, index of its stage); a parameter shared by stages appears once
        # per stage, so every stage that uses it is seen to change
        self.flat = [(p, k) for k, s in enumerate(stages) for p in s.params]
        self.seen = [p._ver for p, _ in self.flat]
        self.struct_clock = ParamSet.struct_clock
        self.clock = Param.clock
        self._conts = list(hist.data.containers)
        self.container_clock = self._writes()
        self.ye = (osc.YeI, osc.YeO, osc.YeM)
        self._osc_args = None
        self._lib = _lib.lib()
        self.scales = self._read_scales() if self.post else None
        self._dirty = False     # a multi-point sweep has left the single-point tables / scales behind

    def _writes(self):
        """stores into THIS pipeline's containers (the other pipelines of a DistributionMaker write
        their own)"""
        return sum(c.writes for c in self._conts)

    def _read_scales(self):
        """the post-histogram stage's per-bin factors, [n_cont, n_bins] on the device"""
        hs = self.post[0]
        keep = [c.representation for c in self._conts]
        try:
            for c in self._conts:
                c.representation = hs.calc_mode
            # the stage computes the factors on the host: one upload for all containers
            return K.to_device(np.stack([np.asarray(c["hs_scales"], dtype=np.float64) for c in self._conts]))
        finally:
            for c, r in zip(self._conts, keep):
                c.representation = r

    def _changed(self):
        """stages with a moved parameter; None if parameter OBJECTS were exchanged somewhere
        (select_params, update_params): the plan is rebuilt by the ordinary path then"""
        if ParamSet.struct_clock != self.struct_clock:
            return None
        stages = self.pipeline._stages
        out, seen = [], self.seen
        for i, (p, k) in enumerate(self.flat):
            v = p._ver
            if v != seen[i]:
                seen[i] = v
                if stages[k] not in out:
                    out.append(stages[k])
        return out

    def _replay_barr(self):
        """the moved flux.barr_simple parameters -> the engine's folded flux columns, one pass"""
        st, eng = self.barr_stage, self.engine
        if not self._barr_ready:
            cols = []
            keep = [c.representation for c in self._conts]
            try:
                for c in self._conts:
                    c.representation = "events"
                    cols.append((c.device("true_energy"), c.device("true_coszen"), c.device("nu_flux_nominal"),
                                 c.device("nubar_flux_nominal")))
            finally:
                for c, r in zip(self._conts, keep):
                    c.representation = r
            try:
                eng.enable_barr(cols)
            except ValueError:          # an energy that is not positive: the stages keep the reference's answers
                self.barr_stage = None
                return False
            self._barr_ready = True
        p = st.params
        vals = [float(p[n].value.m_as("dimensionless")) for n in
                ("nue_numu_ratio", "nu_nubar_ratio", "delta_index", "Barr_uphor_ratio", "Barr_nu_nubar_ratio")]
        eng.update_flux_barr(*vals)
        st.param_hash = None      # its own nu_flux arrays are those of older values: recomputed if anybody asks
        return True

    def invalidate(self):
        """forget the compute memos of every stage this plan replays (the plan is being dropped after
        an error: whatever it had half applied must be recomputed by the ordinary path)"""
        for s in [self.osc, self.aeff] + self.flux_stages + self.post:
            s.param_hash = None

    def metric_many(self, set_point, n_points, data_hist, kind):
        """The metric of the total template against `data_hist` at `n_points` INDEPENDENT parameter
        points in one sweep of the events (`HotPathEngine.eval_many`) -- what a finite-difference
        minimiser asks for per gradient (pisa/analysis/analysis.py:2493-2670 with the l-bfgs-b / slsqp
        settings).  `set_point(i)` moves the pipeline's parameters to point i.  Per point the value is
        the very number `run()` + `Map.metric_total` give there.  Returns the list of values, or None
        when the points cannot be taken together (a stage other than osc.prob3 / aeff.aeff moves, the
        flux lives on the grid, stages behind the histogram, ...): the caller then goes point by point.
        The pipeline's parameters are left at the last point."""
        osc, eng = self.osc, self.engine
        if self.post or self.flux_stages or self.hist._engine is not eng or osc.pepmu is None:
            return None
        if kind not in K.METRIC_KIND:
            return None
        if kind == "mod_chi2" and not self.with_errors:
            # output_key='weights': the maps carry no errors and Map.metric uses zero variance
            # (DeviceMapBlock.metric has the same guard); the one-sweep tail would hand sumw2 in
            return None
        g = osc.grid
        if (self._writes() != self.container_clock or n_points < 2
                or bool(g["e_major"]) != bool(eng.grid.energy_first)):
            return None
        eng.set_data_cached(np.ascontiguousarray(data_hist, dtype=np.float64).ravel())
        if not eng.multi_capable(g["plan"]):
            return None
        pts = self._collect_points(set_point, n_points)
        if pts is None:
            return None
        params_list, scales = pts
        vals = eng.eval_many(params_list, kind, np.asarray(scales, dtype=np.float64), plan=g["plan"],
                             energy=g["energy"])
        if any(v != v for v in vals):
            st = eng.metric_status_host()
            if st != 0:
                _lib.check(st)
        # the engine's own per-container scales may have been moved by a point-by-point fallback
        self.pipeline._containers_stale = True
        return vals

    def _collect_points(self, set_point, n_points):
        """moves the parameters to each of `n_points` INDEPENDENT points in turn (`set_point(i)`) and collects
        the point's oscillation parameter block and the containers' aeff scales: ([Prob3Params], [[scale per
        container]]), or None when a stage other than osc.prob3 / aeff.aeff moved or Ye moved (the counters are
        then forgotten, so that the next evaluation goes through the Stage protocol).  The parameters are left
        at the last point."""
        osc = self.osc
        params_list, scales = [], []
        self._dirty = True           # from here on the change counters are consumed point by point
        # the containers' aeff scales, recomputed when an aeff parameter moved since they were made (kept from
        # sweep to sweep: twelve `scale_for` cost more host time than a point's launches)
        aeff_key = (ParamSet.struct_clock,) + tuple(prm._ver for prm in self.aeff.params)
        if getattr(self, "_many_scales_key", None) != aeff_key:
            self._many_scales = None

        def abandon():
            # counters of stages this plan cannot take in a sweep have been consumed: forget what was
            # seen, so that the next evaluation finds every stage moved and goes through the Stage
            # protocol (whose own memos compare parameter VALUES)
            self.seen = [None] * len(self.seen)
            return None

        for i in range(n_points):
            set_point(i)
            changed = self._changed()
            if changed is None:
                return abandon()
            for s in changed:
                if s is not osc and s is not self.aeff:
                    return abandon()
            p = osc.params
            ye = (p.YeI.m_in("dimensionless"), p.YeO.m_in("dimensionless"), p.YeM.m_in("dimensionless"))
            if ye != self.ye:
                return abandon()
            params_list.append(_lib.Prob3Params.from_buffer_copy(osc._matrices()))
            if self._many_scales is None or any(s is self.aeff for s in changed):
                self._many_scales = self.aeff.scales_for(self.names)
                self._many_scales_key = (ParamSet.struct_clock,) + tuple(prm._ver for prm in self.aeff.params)
            scales.append(self._many_scales)
        osc.param_hash = None
        self.clock = Param.clock
        return params_list, scales

    def maps_many(self, set_point, n_points):
        """The maps of all containers at `n_points` INDEPENDENT parameter points in one sweep of the events
        (`HotPathEngine.maps_many`; two or more for more than MAX_POINTS points), for the Fisher matrix of a
        `DistributionMaker`.  `set_point(i)` moves the pipeline's parameters to point i.  Per point the rows
        are the bits `run()` gives there.  Returns dict(hist, sumw2 [n_points, n_containers, n_bins] device
        tensors -- sumw2 zero when the pipeline's maps carry no errors --, sweeps), or None when the points
        cannot be taken together (as `metric_many`); the caller then goes point by point.  The parameters are
        left at the last point."""
        osc, eng = self.osc, self.engine
        if self.post or self.flux_stages or self.hist._engine is not eng or osc.pepmu is None:
            return None
        g = osc.grid
        if (self._writes() != self.container_clock or n_points < 2
                or bool(g["e_major"]) != bool(eng.grid.energy_first)):
            return None
        if not eng.sweep_capable(g["plan"]):
            return None
        pts = self._collect_points(set_point, n_points)
        if pts is None:
            return None
        params_list, scales = pts
        out = eng.maps_many(params_list, np.asarray(scales, dtype=np.float64), plan=g["plan"], energy=g["energy"])
        if not self.with_errors:
            out["sumw2"].zero_()     # output_key 'weights': the maps carry no errors
        self.pipeline._containers_stale = True
        return out

    def run(self):
        """device-backed output MapSet, or None: take the ordinary path"""
        osc, eng = self.osc, self.engine
        if self.hist._engine is not eng or osc.pepmu is None:
            return _no("engine replaced")
        if self._writes() != self.container_clock:
            return _no("a container was written")   # e.g. somebody edited a flux column in place
        if Param.clock != self.clock or self._dirty or ParamSet.struct_clock != self.struct_clock:
            # (the structural counter by itself: `select_params` exchanges parameter OBJECTS without setting a value --
            # found by scripts/dev/fuzz_pipeline.py, round 4: a switch of the mass ordering alone was replayed with the
            # old ordering's tables)
            changed = self._changed()
            if changed is None:
                return _no("parameter objects exchanged")
            if self._dirty:
                # `metric_many` evaluated other points through its own tables: whatever the counters
                # say, the oscillation tables and the containers' scales are those of an older point
                changed = list(changed) + [s for s in (osc, self.aeff) if all(s is not c for c in changed)]
                self._dirty = False
            replayable = [osc, self.aeff] + self.flux_stages + self.post + ([self.barr_stage] if self.barr_stage else [])
            for s in changed:
                if all(s is not r for r in replayable):
                    return _no("stage %s.%s moved" % (s.stage_name, s.service_name))
            self.clock = Param.clock
            if osc in changed:
                yp = self.__dict__.get("_ye_params")
                if yp is None or yp[0] != ParamSet.struct_clock:
                    p = osc.params
                    yp = self._ye_params = [ParamSet.struct_clock, (p.YeI, p.YeO, p.YeM), None]
                vers = (yp[1][0]._ver, yp[1][1]._ver, yp[1][2]._ver)
                if vers != yp[2]:                   # (a fit rarely moves them: looked at when one did)
                    ye = tuple(q.value.m_as("dimensionless") for q in yp[1])
                    if ye != self.ye:
                        return _no("Ye moved")          # new layers, new plan: ordinary path
                    yp[2] = vers
            if self.barr_stage is not None and any(self.barr_stage is c for c in changed):
                if not self._replay_barr():
                    return _no("per-event flux refresh not available")
            flux_changed = [s for s in self.flux_stages if any(s is c for c in changed)]
            if flux_changed:
                # the stages' own compute on the grid nodes, in pipeline order from the first one
                # that moved (a later flux stage reads what an earlier one wrote), then new node tables
                first = self.flux_stages.index(flux_changed[0])
                for s in self.flux_stages[first:]:
                    if all(s is not c for c in flux_changed):
                        s.param_hash = None      # reads what an earlier, moved flux stage wrote
                    s.run()
                self.hist.sync_node_flux()
                self.container_clock = self._writes()   # our own writes
            if osc in changed:
                params = osc._matrices()
                osc.param_hash = None    # its tables no longer belong to the memoised values
                a = self._osc_args
                if a is None or a[0] is not osc.pepmu:
                    g = osc.grid
                    a = self._osc_args = (
                        osc.pepmu, g["plan"].handle, C.c_void_p(g["energy"].data_ptr()), g["energy"].numel(),
                        1 if g["e_major"] else 0, None, None,    # full P tables: written by the stages only
                        C.c_void_p(osc.pepmu.data_ptr()))
                _lib.check(self._lib.pisa_hip_prob3_grid_planned(
                    C.byref(params), a[1], a[2], a[3], a[4], a[5], a[6], a[7], K._stream()))
            if self.aeff in changed:
                for name, sc in zip(self.names, self.aeff.scales_for(self.names)):
                    eng.set_scale(name, sc)
            post_changed = [s for s in self.post if any(s is c for c in changed)]
            if post_changed:
                for s in post_changed:
                    s.compute()          # per-bin factors on the host (a few hundred bins)
                self.scales = self._read_scales()
                self.container_clock = self._writes()
        eng.front(osc.pepmu)
        block = DeviceMapBlock(eng, self.with_errors, self.scales)
        eng._out_block = weakref.ref(block)
        self.pipeline._containers_stale = True
        return DeviceMapSet(self.names, self.binning, block, self.pipeline.name)
