"""The inputs of the generalized Poisson-gamma likelihood (counterpart of
pisa/stages/likelihood/generalized_llh_params.py): per container and output bin the number of MC events
`n_mc_events` and the mean adjustment (set-up), then on every apply the per-bin alpha and beta of
arXiv:1902.08831 (`llh_alphas`, `llh_betas`), the weight sums with one pseudo-weight of 0.001 in empty bins
(`weights`) and without it (`old_sum`), in the binned representation.  `utils.stats.generalized_poisson_llh` /
`Map.generalized_poisson_llh` consume them.

The bin masks `bin_<i>_mask` (written by utils.add_indices; a nonzero value selects the event, `kfold_mask` is
multiplied in) are read at set-up into per-bin event lists: one permutation of the selected events when no event is
in two bins, per-bin lists that share events otherwise.  The lists are built again when `kfold_mask` has changed
since (the reference multiplies it in on every apply); `n_mc_events` and the mean adjustment stay the set-up's, as
there, while alpha counts the events the lists hold now.  Every apply reduces Sigma w and Sigma w^2 over
the lists (`pisa_hip_gpllh_bin_sums`) and forms alpha and beta (`pisa_hip_gpllh_params`); a negative weight raises.
var_z is Sigma w^2 / n where the reference adds a two-pass variance to mean^2: the last bits differ."""
import numpy as np

from pisa_amd import FTYPE
from pisa_amd import kernels as K
from pisa_amd.core.binning import MultiDimBinning
from pisa_amd.core.stage import Stage

__all__ = ["generalized_llh_params", "init_test", "PSEUDO_WEIGHT"]

PSEUDO_WEIGHT = 0.001


def event_lists(masks):
    """[n_bins] event masks (any nonzero value selects) -> (index, offsets, disjoint): bin i's events are
    index[offsets[i]:offsets[i + 1]] in event order"""
    sel = [np.flatnonzero(np.asarray(m).ravel() != 0) for m in masks]
    counts = np.array([s.size for s in sel], dtype=np.int64)
    offsets = np.zeros(len(sel) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    n = max((int(np.asarray(m).size) for m in masks), default=0)
    covered = np.zeros(n, dtype=np.int64)
    for s in sel:
        covered[s] += 1
    disjoint = bool(covered.max(initial=0) <= 1)
    if disjoint:
        # one bin-index column, the selected events ordered by it (a stable sort keeps event order within a bin)
        col = np.full(n, -1, dtype=np.int64)
        for i, s in enumerate(sel):
            col[s] = i
        picked = np.flatnonzero(col >= 0)
        index = picked[np.argsort(col[picked], kind="stable")]
    else:
        index = np.concatenate(sel) if sel else np.zeros(0, dtype=np.int64)
    return np.ascontiguousarray(index, dtype=np.int64), offsets, disjoint


def mean_adjustment(n_mc_events):
    """generalized_llh_params.py setup: -(1 - mean) + 1e-3 if fewer than one MC event per bin on average"""
    m = float(np.mean(n_mc_events))
    return -(1.0 - m) + 1.0e-3 if m < 1.0 else 0.0


class generalized_llh_params(Stage):  # pylint: disable=invalid-name
    def __init__(self, **std_kwargs):
        if "apply_mode" not in std_kwargs:
            raise ValueError("Service requires specifying binning for `apply_mode` during init!")
        if not isinstance(std_kwargs["apply_mode"], MultiDimBinning):
            raise ValueError("`apply_mode` must be a MultiDimBinning")
        n_bins = std_kwargs["apply_mode"].tot_num_bins
        super().__init__(expected_params=(),
                         expected_container_keys=["weights"] + ["bin_%d_mask" % i for i in range(n_bins)],
                         supported_reps={"calc_mode": [None, "events", MultiDimBinning], "apply_mode": MultiDimBinning},
                         **std_kwargs)
        self._lists = {}

    def _event_lists(self, container):
        """(events representation) the container's per-bin event lists as device tensors"""
        has_kfold = "kfold_mask" in container.keys
        kfold = np.asarray(container["kfold_mask"]) if has_kfold else None
        masks = []
        for i in range(self.apply_mode.tot_num_bins):
            m = np.asarray(container["bin_%d_mask" % i]) != 0
            if kfold is not None:
                m = m & (kfold != 0)
            masks.append(m)
        index, offsets, disjoint = event_lists(masks)
        n = np.diff(offsets).astype(FTYPE)
        return dict(index=K.to_device(index, dtype=np.int64), offsets=K.to_device(offsets, dtype=np.int64),
                    n=n, n_mc=K.to_device(n), disjoint=disjoint,
                    kfold_version=container.version("kfold_mask") if has_kfold else None)

    def setup_function(self):
        for container in self.data:
            self.data.representation = self.apply_mode
            for key in ("llh_alphas", "llh_betas", "n_mc_events", "old_sum"):
                container[key] = np.zeros(container.size, dtype=FTYPE)
            self.data.representation = "events"
            lists = self._event_lists(container)
            n_mc = lists["n"]
            adj = mean_adjustment(n_mc)
            lists["adjust"] = K.to_device(np.array([adj], dtype=FTYPE))
            self._lists[container.name] = lists
            self.data.representation = self.apply_mode
            container["n_mc_events"] = n_mc
            container.set_aux_data("mean_adjustment", adj)
            if "hs_scales" not in container.keys:
                container["hs_scales"] = np.zeros(container.size, dtype=FTYPE)
                container["errors"] = np.zeros(container.size, dtype=FTYPE)

    def apply_function(self):
        for container in self.data:
            lists = self._lists[container.name]
            self.data.representation = "events"
            container.set_aux_data("pseudo_weight", PSEUDO_WEIGHT)
            if "kfold_mask" in container.keys and container.version("kfold_mask") != lists["kfold_version"]:
                adjust = lists["adjust"]
                lists = self._lists[container.name] = self._event_lists(container)
                lists["adjust"] = adjust
            w = container.device("weights").reshape(-1).contiguous()
            sw, sw2 = K.gpllh_bin_sums(w, lists["index"], lists["offsets"])
            alpha, beta, wsum = K.gpllh_params(sw[None], sw2[None], lists["n_mc"][None], lists["adjust"])
            self.data.representation = self.apply_mode
            container["llh_alphas"] = alpha[0]
            container["llh_betas"] = beta[0]
            container["weights"] = wsum[0]
            container["old_sum"] = sw


def init_test(**param_kwargs):
    """Instantiation example (what pisa_tests/test_services.py calls for every service; the reference's own values)"""
    from pisa_amd.stages.utils.kde import service_test_binning

    return generalized_llh_params(apply_mode=service_test_binning())
