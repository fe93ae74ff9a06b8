"""Device-tensor front-end of the C ABI.

Arguments are ``torch`` CUDA(=HIP) tensors used purely as device buffers
(``data_ptr()`` + current stream are handed to ``libpisa_hip.so``); every
function launches hand-written gfx950 kernels and returns device tensors.
Function names follow the reference functions they replace.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

F8 = torch.float64


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """torch's current HIP stream of the current device as a raw handle.  The raw
    accessor costs ~0.3 us; `torch.cuda.current_stream()` builds a Python Stream
    object (~7 us), which matters in front of the first launch of an evaluation."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous CUDA tensors"
    return C.c_void_p(t.data_ptr())


def device(index=None):
    if not torch.cuda.is_available():
        raise RuntimeError(
            "pisa_amd needs a HIP device (MI355X); none is visible and there is no CPU fallback"
        )
    return torch.device("cuda", torch.cuda.current_device() if index is None else index)


def to_device(a, dtype=np.float64):
    """Host numpy array -> contiguous device tensor.  Small arrays (per-evaluation scale factors, maps of a few
    hundred bins, pseudo-data) go through a page-locked block of torch's caching host allocator and an asynchronous
    copy on the current stream: a pageable source makes the runtime stage and synchronise (~20 us per call);
    the allocator keeps the block alive until the copy has run."""
    arr = np.ascontiguousarray(a, dtype=dtype)
    if 0 < arr.nbytes <= (1 << 18):
        host = torch.empty(arr.shape, dtype=torch.from_numpy(arr[:0].reshape(-1)).dtype, pin_memory=True)
        host.numpy()[...] = arr
        return host.to(device(), non_blocking=True)
    return torch.from_numpy(arr).to(device(), non_blocking=False)


def _status_buffer():
    return torch.zeros(1, dtype=torch.int32, device=device())


# ---------------------------------------------------------------- prob3
def propagate_array(params, nubar, energy, densities, distances, out=None, avg_range=None):
    """`propagate_array` gufunc (numba_osc_hostfuncs.py:56-70).  `avg_range` (device tensor, km: one value per
    element with per-element rows, one value with a shared row): the production-height average over that range of
    the first traversed layer's length (`pisa_hip_propagate_array_avg`); None is the plain call."""
    lib = _lib.lib()
    n = energy.numel()
    per_elem = 1 if densities.dim() == 2 else 0
    n_layers = densities.shape[-1]
    if out is None:
        out = torch.empty((n, 3, 3), dtype=F8, device=energy.device)
    if avg_range is not None:
        assert avg_range.dtype == F8 and avg_range.numel() == (n if per_elem else 1), "one range per row of layers"
        _lib.check(lib.pisa_hip_propagate_array_avg(
            C.byref(params), int(nubar), _ptr(energy), _ptr(densities), _ptr(distances), _ptr(avg_range), n,
            n_layers, per_elem, _ptr(out), _stream()))
        return out
    _lib.check(lib.pisa_hip_propagate_array(
        C.byref(params), int(nubar), _ptr(energy), _ptr(densities), _ptr(distances), n,
        n_layers, per_elem, _ptr(out), _stream()))
    return out


def prob3_grid(params, energy, densities, distances, e_major=True, out_nu=None, out_nubar=None,
               out_pepmu=None, want_pepmu=False):
    """Both 'nu' and 'nubar' linked containers of a 2-D calc grid in one launch
    (prob3.py:452-459, 581-588).  Returns (P_nu, P_nubar[, pepmu])."""
    lib = _lib.lib()
    n_e, n_cz, n_layers = energy.numel(), densities.shape[0], densities.shape[1]
    if out_nu is None:
        out_nu = torch.empty((n_e * n_cz, 3, 3), dtype=F8, device=energy.device)
    if out_nubar is None:
        out_nubar = torch.empty((n_e * n_cz, 3, 3), dtype=F8, device=energy.device)
    if out_pepmu is None and want_pepmu:
        out_pepmu = torch.empty((2, 3, n_e * n_cz, 2), dtype=F8, device=energy.device)
    _lib.check(lib.pisa_hip_prob3_grid(
        C.byref(params), _ptr(energy), n_e, _ptr(densities), _ptr(distances), n_cz, n_layers,
        1 if e_major else 0, _ptr(out_nu), _ptr(out_nubar), _ptr(out_pepmu), _stream()))
    if out_pepmu is not None:
        return out_nu, out_nubar, out_pepmu
    return out_nu, out_nubar


class GridPlan:
    """Per-layer-table plan of the two-stage grid kernels (`pisa_hip_grid_plan`):
    cache matches resolved per coszen row + list of distinct shell densities.  `avg_range` (host array [n_cz], km):
    the range of the first layer's length per row for the production-height average (`set_avg_range`)."""

    def __init__(self, densities, distances, avg_range=None):
        lib = _lib.lib()
        self.n_cz, self.n_layers = densities.shape
        h = C.c_void_p()
        torch.cuda.synchronize()
        _lib.check(lib.pisa_hip_grid_plan_create(_ptr(densities), _ptr(distances), self.n_cz,
                                                 self.n_layers, C.byref(h)))
        self.handle = h
        self.avg_range = None
        if avg_range is not None:
            self.set_avg_range(avg_range)

    def set_avg_range(self, avg_range):
        """attach the per-row range (None clears it): every planned evaluation on this plan then returns the
        production-height average on the rows with a positive range (`pisa_hip_grid_plan_set_avg_range`)"""
        if avg_range is None:
            _lib.check(_lib.lib().pisa_hip_grid_plan_set_avg_range(self.handle, None))
            self.avg_range = None
            return
        r = np.ascontiguousarray(avg_range, dtype=np.float64).ravel()
        if r.size != self.n_cz:
            raise ValueError("avg_range needs one value per coszen row (%d), got %d" % (self.n_cz, r.size))
        _lib.check(_lib.lib().pisa_hip_grid_plan_set_avg_range(self.handle, r.ctypes.data))
        self.avg_range = r

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.lib().pisa_hip_grid_plan_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def prob3_grid_planned(params, plan, energy, e_major=True, out_nu=None, out_nubar=None,
                       out_pepmu=None):
    """Planned grid evaluation (equal to `prob3_grid` to rounding, see csrc/prob3.hip)."""
    lib = _lib.lib()
    n_e = energy.numel()
    n = n_e * plan.n_cz
    if out_nu is None:
        out_nu = torch.empty((n, 3, 3), dtype=F8, device=energy.device)
    if out_nubar is None:
        out_nubar = torch.empty((n, 3, 3), dtype=F8, device=energy.device)
    if out_pepmu is None:
        out_pepmu = torch.empty((2, 3, n, 2), dtype=F8, device=energy.device)
    _lib.check(lib.pisa_hip_prob3_grid_planned(
        C.byref(params), plan.handle, _ptr(energy), n_e, 1 if e_major else 0, _ptr(out_nu),
        _ptr(out_nubar), _ptr(out_pepmu), _stream()))
    return out_nu, out_nubar, out_pepmu


def calc_layers(earth, coszen, max_layers):
    """`extCalcLayers` (layers.py:38-169) -> (n_layers, densities, distances)."""
    lib = _lib.lib()
    n = coszen.numel()
    dev = coszen.device
    n_layers = torch.empty(n, dtype=F8, device=dev)
    dens = torch.empty((n, max_layers), dtype=F8, device=dev)
    dist = torch.empty((n, max_layers), dtype=F8, device=dev)
    st = _status_buffer()
    _lib.check(lib.pisa_hip_calc_layers(
        C.byref(earth), _ptr(coszen), n, max_layers, _ptr(n_layers), _ptr(dens), _ptr(dist),
        _ptr(st), _stream()))
    if int(st.item()) != 0:
        # the reference raises a broadcast ValueError here (layers.py:158)
        raise ValueError("path geometry not representable (detector below the first Earth "
                         "shell boundary, or coszen exactly tangent to a shell)")
    return n_layers, dens, dist


def prob3_events(params, earth, nubar, energy, coszen, out=None):
    """Event-by-event prob3 with in-kernel layer reconstruction."""
    lib = _lib.lib()
    n = energy.numel()
    if out is None:
        out = torch.empty((n, 3, 3), dtype=F8, device=energy.device)
    st = _status_buffer()
    _lib.check(lib.pisa_hip_prob3_events(
        C.byref(params), C.byref(earth), int(nubar), _ptr(energy), _ptr(coszen), n, _ptr(out),
        _ptr(st), _stream()))
    if int(st.item()) != 0:
        raise ValueError("path geometry not representable (see calc_layers)")
    return out


def prob3_events_multi(params, earth, event_sets, status):
    """Event-by-event prob3 for several containers in one launch; each set
    receives its (prob_e, prob_mu) pairs and/or full matrices."""
    lib = _lib.lib()
    arr = event_sets if isinstance(event_sets, C.Array) else (_lib.EventSet * len(event_sets))(*event_sets)
    _lib.check(lib.pisa_hip_prob3_events_multi(C.byref(params), C.byref(earth), arr, len(arr),
                                               _ptr(status), _stream()))


def fill_probs(probability, init_flav, flav, out=None):
    """`fill_probs` (numba_osc_hostfuncs.py:206-221)."""
    lib = _lib.lib()
    n = probability.shape[0]
    if out is None:
        out = torch.empty(n, dtype=F8, device=probability.device)
    _lib.check(lib.pisa_hip_fill_probs(_ptr(probability), int(init_flav), int(flav), n, _ptr(out),
                                       _stream()))
    return out


# ---------------------------------------------------------- translation
def _sample_array(sample):
    arr = (C.c_void_p * len(sample))(*[s.data_ptr() for s in sample])
    for s in sample:
        assert s.is_cuda and s.is_contiguous()
    return arr


def lookup_regular(sample, flat_hist, binning):
    """`lookup` on regular binnings (translation.py:417-501)."""
    lib = _lib.lib()
    n = sample[0].numel()
    width = 1 if flat_hist.dim() == 1 else flat_hist.shape[1]
    out = torch.empty((n,) if flat_hist.dim() == 1 else (n, width), dtype=F8,
                      device=flat_hist.device)
    _lib.check(lib.pisa_hip_lookup_regular(
        C.byref(binning), _sample_array(sample), n, _ptr(flat_hist), width, _ptr(out), _stream()))
    return out


def histogram_regular(sample, weights, binning, averaged=False):
    """`histogram` on regular binnings (translation.py:90-129)."""
    lib = _lib.lib()
    n = sample[0].numel()
    n_bins = int(np.prod([binning.nbins[k] for k in range(binning.ndim)]))
    out = torch.empty(n_bins, dtype=F8, device=sample[0].device)
    _lib.check(lib.pisa_hip_histogram_regular(
        C.byref(binning), _sample_array(sample), n, _ptr(weights), 1 if averaged else 0,
        _ptr(out), _stream()))
    return out


def transform_apply(weights, unc_weights, ptr, col, val, n_out, errors=True):
    """(hist, sumw2, bin_unc2) = weights-in-calc-bins applied to a `hist_transform` given as CSR over
    the output bins (see pisa_hip_transform_apply)"""
    lib = _lib.lib()
    dev = weights.device
    hist = torch.empty(n_out, dtype=F8, device=dev)
    sumw2 = torch.empty(n_out, dtype=F8, device=dev) if errors else None
    unc2 = torch.empty(n_out, dtype=F8, device=dev) if errors else None
    _lib.check(lib.pisa_hip_transform_apply(_ptr(weights), _ptr(unc_weights), _ptr(ptr), _ptr(col), _ptr(val),
                                            int(n_out), _ptr(hist), _ptr(sumw2), _ptr(unc2), _stream()))
    return hist, sumw2, unc2


def event_indices(sample, binning):
    """flat bin index (int32, -1 outside) of every event in a regular binning"""
    lib = _lib.lib()
    n = sample[0].numel()
    out = torch.empty(n, dtype=torch.int32, device=sample[0].device)
    _lib.check(lib.pisa_hip_event_indices(C.byref(binning), _sample_array(sample), n, _ptr(out),
                                          _stream()))
    return out


class HistWorkspace:
    """Limb / map buffers for `reweight_hist` (allocated once, reused)."""

    def __init__(self, n_containers, n_bins, dev=None):
        dev = dev or device()
        self.n_containers, self.n_bins = n_containers, n_bins
        self.limbs = torch.zeros((n_containers, n_bins, 2, _lib.ACC_LIMBS), dtype=torch.int64,
                                 device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.hist = torch.empty((n_containers, n_bins), dtype=F8, device=dev)
        self.sumw2 = torch.empty((n_containers, n_bins), dtype=F8, device=dev)


def reweight_hist(containers, calc_grid, prob_nu, prob_nubar, pepmu, out_binning, ws,
                  clear=True):
    """Fused prob3.apply + aeff.apply + hist.apply(sumw2); fills ws.limbs
    (`clear=False`: adds to them, e.g. after `finalize_metric(..., clear_limbs=True)`)."""
    lib = _lib.lib()
    arr = containers if isinstance(containers, C.Array) else (_lib.Container * len(containers))(*containers)
    fn = lib.pisa_hip_reweight_hist if clear else lib.pisa_hip_reweight_hist_acc
    _lib.check(fn(
        arr, len(arr), C.byref(calc_grid), _ptr(prob_nu), _ptr(prob_nubar), _ptr(pepmu),
        C.byref(out_binning), _ptr(ws.limbs), _ptr(ws.status), _stream()))
    return ws.limbs


def hist_finalize(ws):
    lib = _lib.lib()
    _lib.check(lib.pisa_hip_hist_finalize(_ptr(ws.limbs), ws.n_containers, ws.n_bins,
                                          _ptr(ws.hist), _ptr(ws.sumw2), _ptr(ws.status),
                                          _stream()))
    return ws.hist, ws.sumw2


FINALIZE_METRIC_MAX = 4096


def finalize_metric(ws, kind, actual, total_out, metric_status, clear_limbs=True):
    """`hist_finalize` + `metric` (maps summed over containers) in one launch;
    `total_out` may be a device tensor or a pinned host tensor.  Same bits as the
    two separate calls."""
    lib = _lib.lib()
    _lib.check(lib.pisa_hip_finalize_metric(
        _ptr(ws.limbs), ws.n_containers, ws.n_bins, _ptr(ws.hist), _ptr(ws.sumw2),
        METRIC_KIND[kind], _ptr(actual), total_out.data_ptr(), _ptr(ws.status),
        _ptr(metric_status), 1 if clear_limbs else 0, _stream()))
    return total_out


def apply_osc_weights(nu_flux, prob_e, prob_mu, weights):
    """prob3.apply_function (prob3.py:621-622), in place on `weights`.  `prob_e` / `prob_mu` may be 1-D views with
    the same element stride (columns of one table): read in place."""
    lib = _lib.lib()
    if nu_flux.numel() != 2 * weights.numel():
        # the kernel reads (nue, numu) of event i at nu_flux[2 i], nu_flux[2 i + 1]: anything shorter is read past its end
        raise ValueError("apply_osc_weights: nu_flux needs two columns (nue, numu) per event: %s for %d events"
                         % (tuple(nu_flux.shape), weights.numel()))
    if (prob_e.dim() == 1 and prob_mu.dim() == 1 and prob_e.stride(0) == prob_mu.stride(0) > 1
            and prob_e.is_cuda and prob_mu.is_cuda and prob_e.dtype == prob_mu.dtype == F8
            and prob_e.numel() == prob_mu.numel() == weights.numel()):
        _lib.check(lib.pisa_hip_apply_osc_weights_strided(_ptr(nu_flux), prob_e.data_ptr(), prob_mu.data_ptr(),
                                                          prob_e.stride(0), weights.numel(), _ptr(weights), _stream()))
        return weights
    # (any other view -- different strides, more dimensions -- is compacted first)
    prob_e = prob_e if prob_e.is_contiguous() else prob_e.contiguous()
    prob_mu = prob_mu if prob_mu.is_contiguous() else prob_mu.contiguous()
    _lib.check(lib.pisa_hip_apply_osc_weights(_ptr(nu_flux), _ptr(prob_e), _ptr(prob_mu),
                                              weights.numel(), _ptr(weights), _stream()))
    return weights


def weight_chain_multi(items):
    """The reset -> [osc] -> [aeff] chain of several containers in one launch (`pisa_hip_weight_chain_multi`).
    items: (initial_weights, nu_flux or None, prob_e, prob_mu, weighted_aeff or None, scale) per container, device
    tensors; prob_e / prob_mu may be equal-stride 1-D views.  Returns (flat block of all weights, list of its
    per-container views)."""
    lib = _lib.lib()
    sizes = [int(it[0].numel()) for it in items]
    block = torch.empty(sum(sizes), dtype=F8, device=items[0][0].device)
    sets = (_lib.ChainSet * len(items))()
    keep, views, off = [], [], 0
    for s, (w0, flux, pe, pmu, aeff, scale), n in zip(sets, items, sizes):
        out = block[off:off + n]
        off += n
        views.append(out)
        s.n, s.d_initial_weights, s.d_weights = n, _ptr(w0), out.data_ptr()
        if flux is not None:
            if not (pe.dim() == 1 and pmu.dim() == 1 and pe.stride(0) == pmu.stride(0) >= 1 and pe.numel() == pmu.numel() == n):
                pe, pmu = pe.contiguous().reshape(-1), pmu.contiguous().reshape(-1)
                keep += [pe, pmu]
            s.d_nu_flux, s.d_prob_e, s.d_prob_mu, s.prob_stride = _ptr(flux), pe.data_ptr(), pmu.data_ptr(), max(1, pe.stride(0))
        if aeff is not None:
            s.d_weighted_aeff, s.aeff_scale = _ptr(aeff), float(scale)
    _lib.check(lib.pisa_hip_weight_chain_multi(sets, len(items), _stream()))
    return block, views


def apply_aeff(weighted_aeff, scale, weights):
    """aeff.apply_function (aeff.py:87), in place on `weights`."""
    lib = _lib.lib()
    _lib.check(lib.pisa_hip_apply_aeff(_ptr(weighted_aeff), float(scale), weights.numel(),
                                       _ptr(weights), _stream()))
    return weights


# ------------------------------------------------------------------ KDE
def kde_eval(src, coef, s2, qry, inv_cov):
    """Gaussian kernel sums (see pisa_hip_kde_eval); src [dim, n], qry [dim, m]."""
    lib = _lib.lib()
    dim, n = src.shape
    m = qry.shape[1]
    out = torch.empty(m, dtype=F8, device=qry.device)
    ic = np.ascontiguousarray(inv_cov, dtype=np.float64)
    _lib.check(lib.pisa_hip_kde_eval(dim, _ptr(src), _ptr(coef), _ptr(s2), n, _ptr(qry), m,
                                     ic.ctypes.data, _ptr(out), _stream()))
    return out


KDE_BW = {"silverman": 0, "scott": 1}
KDE_DEFAULT_TOL = 1e-14


class KdeEstimator:
    """`gaussian_kde(x, weights, bw_method, adaptive, alpha)` on the device
    (`pisa_hip_kde_create` / `_evaluate`; cell-list cut-off at kernel value `tol`, 0 = all pairs).
    x [dim, n] device tensor (dimension-major), weights [n] or None."""

    def __init__(self, x, weights=None, bw_method="silverman", adaptive=True, alpha=0.3,
                 tol=KDE_DEFAULT_TOL):
        import ctypes as C

        lib = _lib.lib()
        if bw_method not in KDE_BW:
            raise ValueError("`bw_method` should be 'scott' or 'silverman'")
        x = x.contiguous()
        self.dim, self.n = int(x.shape[0]), int(x.shape[1])
        need = int(lib.pisa_hip_kde_workspace_bytes(self.dim, self.n))
        if need < 0:
            raise ValueError("KDE of %d points in %d dimensions not supported" % (self.n, self.dim))
        work = torch.empty(need, dtype=torch.uint8, device=x.device)
        w = None if weights is None else weights.contiguous()
        h = C.c_void_p()
        _lib.check(lib.pisa_hip_kde_create(self.dim, _ptr(x), None if w is None else _ptr(w), self.n,
                                           KDE_BW[bw_method], 1 if adaptive else 0, float(alpha),
                                           float(tol), _ptr(work), need, C.byref(h), _stream()))
        self._h, self._lib = h, lib
        self._work = work   # holds the estimator's device arrays (torch's caching allocator reuses it)
        info = _lib.KdeInfo()
        _lib.check(lib.pisa_hip_kde_info(h, C.byref(info)))
        d = self.dim
        self.factor, self.norm, self.sum_w = info.factor, info.norm, info.sum_w
        self.covariance = np.array(info.covariance).reshape(3, 3)[:d, :d].copy()
        self.inv_cov = np.array(info.inv_cov).reshape(3, 3)[:d, :d].copy()
        self.mean = np.array(info.mean)[:d].copy()
        self.r_cut, self.cell, self.n_cells = info.r_cut, info.cell, info.n_cells
        self.pairs_pilot, self.n_dense = info.pairs_pilot, info.n_dense
        self.pairs_eval = 0

    def __call__(self, points):
        import ctypes as C

        q = points.contiguous()
        m = int(q.shape[1])
        out = torch.empty(m, dtype=F8, device=q.device)
        if m == 0:
            return out
        need = int(self._lib.pisa_hip_kde_eval_workspace_bytes(self._h, m))
        work = torch.empty(need, dtype=torch.uint8, device=q.device)
        _lib.check(self._lib.pisa_hip_kde_evaluate(self._h, _ptr(q), m, _ptr(work), need, _ptr(out),
                                                   _stream()))
        info = _lib.KdeInfo()
        _lib.check(self._lib.pisa_hip_kde_info(self._h, C.byref(info)))
        self.pairs_eval = info.pairs_eval
        return out

    def evaluate_lattice(self, origin, step, count):
        """densities at the points origin[d] + i_d step[d], 0 <= i_d < count[d], as a flat device
        tensor in numpy.meshgrid(indexing="ij") order (`pisa_hip_kde_evaluate_lattice`)"""
        import ctypes as C

        d = self.dim
        assert len(origin) == len(step) == len(count) == d
        o = (C.c_double * d)(*[float(v) for v in origin])
        st = (C.c_double * d)(*[float(v) for v in step])
        cnt = (C.c_int64 * d)(*[int(v) for v in count])
        if min(int(v) for v in count) < 1:
            raise ValueError("empty lattice %r" % (list(count),))
        m = int(np.prod([int(v) for v in count]))
        out = torch.empty(m, dtype=F8, device=self._work.device)
        need = int(self._lib.pisa_hip_kde_lattice_workspace_bytes(self._h, st, cnt))
        if need < 0:
            raise ValueError("invalid lattice %r x %r" % (list(step), list(count)))
        work = torch.empty(need, dtype=torch.uint8, device=out.device)
        _lib.check(self._lib.pisa_hip_kde_evaluate_lattice(self._h, o, st, cnt, _ptr(work), need, _ptr(out),
                                                           _stream()))
        info = _lib.KdeInfo()
        _lib.check(self._lib.pisa_hip_kde_info(self._h, C.byref(info)))
        self.pairs_eval = info.pairs_eval
        return out

    def arrays(self):
        """(ys [dim, n], coef [n], s2 [n]) in the estimator's cell-sorted source order (copies)"""
        import ctypes as C

        p = [C.c_void_p() for _ in range(3)]
        _lib.check(self._lib.pisa_hip_kde_arrays(self._h, *[C.byref(v) for v in p]))
        base = self._work.data_ptr()
        out = []
        for v, cnt in zip(p, (self.dim * self.n, self.n, self.n)):
            off = v.value - base
            out.append(self._work[off:off + 8 * cnt].view(F8).clone())
        return out[0].view(self.dim, self.n), out[1], out[2]

    def close(self):
        if self._h is not None:
            self._lib.pisa_hip_kde_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------- metric
METRIC_KIND = {"llh": 0, "poisson_llh": 1, "chi2": 2, "mod_chi2": 3}          # the fused tails of an evaluation
# the generalized Poisson-gamma likelihood: a kind of the engine (`HotPathEngine.configure_gpllh`) with entry points of
# its own (`pisa_hip_finalize_gpllh`, `pisa_hip_generalized_poisson_llh`), not one of the finalize_metric* kinds above
GPLLH = "generalized_poisson_llh"
GPLLH_KIND = 9
# `metric()` on maps takes these too (PISA_HIP_METRIC_* of include/pisa_hip.h)
MAP_METRIC_KIND = dict(METRIC_KIND, correct_chi2=4, signed_sqrt_mod_chi2=5, mcllh_mean=6, mcllh_eff=7, conv_llh=8)
VARIANCE_METRICS = ("mod_chi2", "correct_chi2", "signed_sqrt_mod_chi2", "mcllh_mean", "mcllh_eff", "conv_llh")


class KdeLatticeBatch:
    """The estimators of one KDE-stage evaluation on the library's own threads and streams
    (`pisa_hip_kde_lattice_submit` / `_wait`): `submit` queues jobs and returns -- the caller may go on
    producing the inputs of the next ones --, `wait` returns (densities [n_jobs, m] device tensor, [sum of the
    weights used per job], (pairs_pilot, pairs_eval) summed over the jobs).
    A job: (x [dim, n] device tensor, weights device tensor or None, index int64 device tensor or None);
    weights are those of the parent sample when an index is given."""

    def __init__(self, n_jobs, origin, step, count, dev, bw_method="silverman", adaptive=True, alpha=0.3,
                 tol=KDE_DEFAULT_TOL, n_threads=0):
        import ctypes as C

        if bw_method not in KDE_BW:
            raise ValueError("`bw_method` should be 'scott' or 'silverman'")
        d = len(origin)
        assert len(step) == len(count) == d
        if min(int(v) for v in count) < 1:
            raise ValueError("empty lattice %r" % (list(count),))
        self._lib = _lib.lib()
        self.dim, self.capacity, self.n = d, int(n_jobs), 0
        self.out = torch.empty((self.capacity, int(np.prod([int(v) for v in count]))), dtype=F8, device=dev)
        self._arr = (_lib.KdeJob * max(self.capacity, 1))()
        self._keep = []
        self._o = (C.c_double * d)(*[float(v) for v in origin])
        self._st = (C.c_double * d)(*[float(v) for v in step])
        self._cnt = (C.c_int64 * d)(*[int(v) for v in count])
        self._args = (KDE_BW[bw_method], 1 if adaptive else 0, float(alpha), float(tol))
        self._threads = int(n_threads)
        self._waited = False

    def submit(self, jobs):
        import ctypes as C

        first = self.n
        assert first + len(jobs) <= self.capacity and not self._waited
        for x, w, idx in jobs:
            x = x.contiguous()
            assert int(x.shape[0]) == self.dim
            self._keep.append(x)
            j = self._arr[self.n]
            j.d_x, j.n = _ptr(x), int(x.shape[1])
            if w is not None:
                w = w.contiguous()
                self._keep.append(w)
                j.d_weights = _ptr(w)
                if idx is not None:
                    idx = idx.contiguous()
                    assert idx.dtype == torch.int64 and int(idx.numel()) == j.n
                    self._keep.append(idx)
                    j.d_index = _ptr(idx)
                else:
                    assert int(w.numel()) == j.n
            j.d_out = _ptr(self.out[self.n])
            self.n += 1
        if self.n > first:
            sub = C.cast(C.addressof(self._arr) + first * C.sizeof(_lib.KdeJob), C.POINTER(_lib.KdeJob))
            _lib.check(self._lib.pisa_hip_kde_lattice_submit(sub, self.n - first, self.dim, self._args[0], self._args[1],
                                                             self._args[2], self._args[3], self._o, self._st, self._cnt,
                                                             self._threads, _stream()))

    def wait_jobs(self, first, count):
        """returns when jobs first .. first + count - 1 are done (`pisa_hip_kde_lattice_wait_jobs`), whatever else is
        still running: (their densities [count, m] -- a view of the batch's output --, [sum of the weights used per job])"""
        import ctypes as C

        assert 0 <= first and first + count <= self.n
        _lib.check(self._lib.pisa_hip_kde_lattice_wait_jobs(
            C.c_void_p(C.addressof(self._arr) + first * C.sizeof(_lib.KdeJob)), count))
        a = self._arr
        for i in range(first, first + count):
            _lib.check(a[i].status)
        return self.out[first:first + count], [a[i].sum_w for i in range(first, first + count)]

    def wait(self):
        _lib.check(self._lib.pisa_hip_kde_lattice_wait())
        self._waited = True
        for i in range(self.n):
            _lib.check(self._arr[i].status)
        a = self._arr
        return (self.out[:self.n], [a[i].sum_w for i in range(self.n)],
                (sum(a[i].pairs_pilot for i in range(self.n)), sum(a[i].pairs_eval for i in range(self.n))))

    def __del__(self):   # the library holds pointers into this object's job array until the jobs are done
        if self.n and not self._waited:
            try:
                self._lib.pisa_hip_kde_lattice_wait()
            except Exception:   # pylint: disable=broad-except
                pass


def kde_lattice_batch(jobs, origin, step, count, bw_method="silverman", adaptive=True, alpha=0.3,
                      tol=KDE_DEFAULT_TOL, n_threads=0):
    """all jobs of a `KdeLatticeBatch` submitted at once and waited for (`pisa_hip_kde_lattice_batch`)"""
    b = KdeLatticeBatch(len(jobs), origin, step, count, jobs[0][0].device if jobs else device(), bw_method=bw_method,
                        adaptive=adaptive, alpha=alpha, tol=tol, n_threads=n_threads)
    b.submit(jobs)
    return b.wait()


def _check_status(status):
    st = int(status.item())
    if st != 0:
        _lib.check(st)


def _with_status(status, dev, launch):
    """`launch(status word)` with the caller's word, which the caller reads; or with one allocated here and checked when
    the launch has returned"""
    if status is not None:
        launch(status)
        return
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    launch(status)
    _check_status(status)


def metric(kind, actual, expected, sigma2=None, per_bin=False, total_out=None, status=None):
    """Map.metric + nansum (map.py:1572-1604) on device.  `expected` (and
    `sigma2`) may be [n_maps, n_bins]; maps are summed in index order first.
    Returns a 1-element device tensor (and per-bin values if requested);
    `total_out` may also be a pinned (device-mapped) host tensor."""
    lib = _lib.lib()
    n_bins = actual.numel()
    n_maps = 1 if expected.dim() == 1 else expected.shape[0]
    dev = actual.device
    if total_out is None:
        total_out = torch.empty(1, dtype=F8, device=dev)
    pb = torch.empty(n_bins, dtype=F8, device=dev) if per_bin else None
    # (`_with_status` spelled out: this call is on the evaluation path of engine.py, where a closure costs 0.3 us of 7)
    own_status = status is None
    if own_status:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.pisa_hip_metric(
        MAP_METRIC_KIND[kind], _ptr(actual), _ptr(expected), _ptr(sigma2), n_maps, n_bins, _ptr(pb),
        total_out.data_ptr() if not total_out.is_cuda and total_out.is_pinned() else _ptr(total_out),
        _ptr(status), _stream()))
    if own_status:
        _check_status(status)
    return (total_out, pb) if per_bin else total_out


# ------------------------------------------------------------------------- trial ensembles
# the metrics that account for finite MC statistics: their own entry points (csrc/ensemble_mc.hip), one form
ENSEMBLE_MC_KINDS = ("correct_chi2", "mcllh_mean", "mcllh_eff", "conv_llh")


def _maps_args(what, data, expected, sigma2):
    """data [T, B], expected [K, B] and sigma2 (None or [K, B]) checked and made contiguous"""
    if data.dim() != 2 or expected.dim() != 2 or data.dtype != F8 or expected.dtype != F8:
        raise ValueError("%s: data is [n_trials, n_bins] and expected [n_templates, n_bins], both float64" % what)
    if sigma2 is not None and (sigma2.shape != expected.shape or sigma2.dtype != F8):
        raise ValueError("%s: sigma2 has the shape and dtype of expected" % what)
    return data.contiguous(), expected.contiguous(), None if sigma2 is None else sigma2.contiguous()


def _offset_arg(what, offset, n_k):
    if offset is None:
        return None
    if offset.shape != (n_k,) or offset.dtype != F8:
        raise ValueError("%s: offset is float64 [n_templates]" % what)
    return offset.contiguous()


def _ensemble_args(kind, data, expected, sigma2, form):
    if kind not in METRIC_KIND and kind not in ENSEMBLE_MC_KINDS:
        raise ValueError("metric_matrix: metric '%s' not among %s" % (kind, sorted(METRIC_KIND) + list(
            ENSEMBLE_MC_KINDS)))
    if form not in _lib.ENSEMBLE_FORMS:
        raise ValueError("metric_matrix: form '%s' not among %s" % (form, list(_lib.ENSEMBLE_FORMS)))
    if kind in ENSEMBLE_MC_KINDS:
        if form == "product":
            raise ValueError("metric_matrix: '%s' has no product form" % kind)
        if sigma2 is None:
            raise ValueError("metric_matrix: '%s' needs sigma2" % kind)
    data, expected, sigma2 = _maps_args("metric_matrix", data, expected, sigma2)
    # (a mismatch of the bin counts reaches the library as n_bins = 0: PISA_HIP_ERR_INVALID, nothing is launched)
    n_bins = data.shape[1] if data.shape[1] == expected.shape[1] else 0
    return data, expected, sigma2, data.shape[0], expected.shape[0], n_bins


def metric_matrix(kind, data, expected, sigma2=None, form="auto", status=None):
    """Map.metric_total of every data map against every template (`pisa_hip_metric_matrix`): data [T, B], expected
    and sigma2 [K, B] device tensors -> [T, K] device tensor.  form "direct" (every kind), "product" (llh,
    poisson_llh: the fp64 matrix cores) or "auto" (product where it exists).  A negative datum or expectation
    raises ValueError, as `metric` does.  correct_chi2, mcllh_mean, mcllh_eff and conv_llh (`ENSEMBLE_MC_KINDS`) go to
    `pisa_hip_metric_matrix_mc`: sigma2 is required, "product" is refused, a negative sigma2 raises ValueError and a
    negative datum or expectation does for the two mcllh kinds (the other two clip)."""
    data, expected, sigma2, n_t, n_k, n_bins = _ensemble_args(kind, data, expected, sigma2, form)
    dev = data.device
    out = torch.empty((n_t, n_k), dtype=F8, device=dev)

    def launch(status):
        if kind in ENSEMBLE_MC_KINDS:
            _lib.check(_lib.lib().pisa_hip_metric_matrix_mc(
                MAP_METRIC_KIND[kind], _ptr(data), _ptr(expected), _ptr(sigma2), n_t, n_k, n_bins, _ptr(out),
                _ptr(status), _stream()))
        else:
            _lib.check(_lib.lib().pisa_hip_metric_matrix(
                METRIC_KIND[kind], _lib.ENSEMBLE_FORMS.index(form), _ptr(data), _ptr(expected), _ptr(sigma2), n_t,
                n_k, n_bins, _ptr(out), _ptr(status), _stream()))

    _with_status(status, dev, launch)
    return out


def metric_matrix_best(kind, data, expected, sigma2=None, offset=None, k0=0, form="auto", status=None):
    """the matrix of `metric_matrix` (+ offset [K] per column) reduced per trial without being written
    (`pisa_hip_metric_matrix_best`; `pisa_hip_metric_matrix_mc_best` for `ENSEMBLE_MC_KINDS`) -> (best [T]: max over
    k for the llh kinds, min for the chi2 kinds; arg [T] int32: the smallest k attaining it; at [T]: column k0), bit
    for bit the reduction of the full matrix"""
    data, expected, sigma2, n_t, n_k, n_bins = _ensemble_args(kind, data, expected, sigma2, form)
    dev = data.device
    offset = _offset_arg("metric_matrix_best", offset, n_k)
    best = torch.empty(n_t, dtype=F8, device=dev)
    arg = torch.empty(n_t, dtype=torch.int32, device=dev)
    at = torch.empty(n_t, dtype=F8, device=dev)

    def launch(status):
        if kind in ENSEMBLE_MC_KINDS:
            _lib.check(_lib.lib().pisa_hip_metric_matrix_mc_best(
                MAP_METRIC_KIND[kind], _ptr(data), _ptr(expected), _ptr(sigma2), _ptr(offset), int(k0), n_t, n_k,
                n_bins, _ptr(best), _ptr(arg), _ptr(at), _ptr(status), _stream()))
        else:
            _lib.check(_lib.lib().pisa_hip_metric_matrix_best(
                METRIC_KIND[kind], _lib.ENSEMBLE_FORMS.index(form), _ptr(data), _ptr(expected), _ptr(sigma2),
                _ptr(offset), int(k0), n_t, n_k, n_bins, _ptr(best), _ptr(arg), _ptr(at), _ptr(status), _stream()))

    _with_status(status, dev, launch)
    return best, arg, at


def _draw_args(what, mu, sigma, method, n_trials, seed, stream, first_trial, out):
    """the arguments of a draw checked: mu [B], sigma (None where `method` is "poisson", else [B]), the ranges of seed,
    stream and first_trial, and out [n_trials, B] (allocated when None)"""
    if mu.dim() != 1 or mu.dtype != F8:
        raise ValueError("%s: mu is a float64 vector [n_bins]" % what)
    if sigma is None:
        if method != "poisson":
            raise ValueError("%s: method '%s' needs sigma" % (what, method))
    elif sigma.dim() != 1 or sigma.dtype != F8 or sigma.shape != mu.shape or sigma.device != mu.device:
        raise ValueError("%s: sigma is a float64 vector of mu's shape on mu's device" % what)
    seed, stream, first_trial, n_trials = int(seed), int(stream), int(first_trial), int(n_trials)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("%s: the seed %d is outside [0, 2^64)" % (what, seed))
    if not (0 <= stream < 2 ** 32 and 0 <= first_trial < 2 ** 32):
        raise ValueError("%s: stream and first_trial are in [0, 2^32)" % what)
    mu = mu.contiguous()
    sigma = None if sigma is None else sigma.contiguous()
    n_bins = mu.shape[0]
    # (a size outside [1, 2^31 - 1] or trial numbers beyond 2^32 reach the library: PISA_HIP_ERR_INVALID, nothing
    # is launched)
    if out is None:
        out = torch.empty((max(n_trials, 0), n_bins), dtype=F8, device=mu.device)
    elif tuple(out.shape) != (n_trials, n_bins) or out.dtype != F8 or not out.is_contiguous():
        raise ValueError("%s: out is a contiguous float64 [n_trials, n_bins]" % what)
    return mu, sigma, n_bins, n_trials, seed, stream, first_trial, out


def poisson_fluctuate(mu, n_trials, seed, stream=0, first_trial=0, out=None, status=None):
    """Poisson pseudo-data of one template row drawn on the device (`pisa_hip_poisson_fluctuate`): mu [B] float64
    device vector -> [n_trials, B] float64 device tensor, entry (t, b) ~ Poisson(mu[b]) from the counter-based
    generator of csrc/fluctuate.hip.  The entry depends on (seed, stream, first_trial + t, b, mu[b]) alone: calls
    that split the trials through `first_trial` give the rows of one call.  seed in [0, 2^64), stream and
    first_trial in [0, 2^32).  A NaN mean gives NaN, a zero mean 0; a negative, infinite or > 2^52 mean raises
    ValueError."""
    mu, _, n_bins, n_trials, seed, stream, first_trial, out = _draw_args(
        "poisson_fluctuate", mu, None, "poisson", n_trials, seed, stream, first_trial, out)

    def launch(status):
        _lib.check(_lib.lib().pisa_hip_poisson_fluctuate(_ptr(mu), n_bins, n_trials, seed, stream, first_trial,
                                                         _ptr(out), _ptr(status), _stream()))

    _with_status(status, mu.device, launch)
    return out


FLUCTUATE_METHOD = {"poisson": 0, "scaled_poisson": 1, "gauss": 2, "gauss+poisson": 3}     # PISA_HIP_FLUCT_*


def fluctuate_method(method):
    """a method name normalised as `Map.fluctuate` does (strip, lower, spaces removed); its ValueError otherwise"""
    name = str(method).strip().lower().replace(" ", "")
    if name not in FLUCTUATE_METHOD:
        raise ValueError('Map fluctuation method "%s" not recognized! Valid choices are: %s.'
                         % (name, tuple(FLUCTUATE_METHOD)))
    return name


def fluctuate(mu, n_trials, seed, method="poisson", sigma=None, stream=0, first_trial=0, out=None, status=None):
    """Pseudo-data of one template row drawn on the device by one of the methods of `Map.fluctuate`
    (`pisa_hip_fluctuate`; map.py:1118-1254): mu [B] and, for every method but "poisson", sigma [B] float64 device
    vectors -> [n_trials, B] float64 device tensor from the counter-based generator of csrc/fluctuate.hip.
    "poisson" is `poisson_fluctuate`, bit for bit; "gauss" mu + sigma z; "gauss+poisson" Poisson(max(mu + sigma z, 0));
    "scaled_poisson" k s with s = sigma^2 / mu and k ~ Poisson(mu / s), 0 where mu is 0.  The entry depends on (seed,
    stream, first_trial + t, b, mu[b], sigma[b], method) alone.  A NaN mean gives NaN; a NaN, negative or infinite
    sigma, or a Poisson mean without a draw (negative, infinite, > 2^52), raises ValueError."""
    name = fluctuate_method(method)
    mu, sigma, n_bins, n_trials, seed, stream, first_trial, out = _draw_args(
        "fluctuate", mu, sigma, name, n_trials, seed, stream, first_trial, out)

    def launch(status):
        _lib.check(_lib.lib().pisa_hip_fluctuate(_ptr(mu), _ptr(sigma), FLUCTUATE_METHOD[name], n_bins, n_trials,
                                                 seed, stream, first_trial, _ptr(out), _ptr(status), _stream()))

    _with_status(status, mu.device, launch)
    return out


TRUTH_MIN_MASS = 0.25        # the least share of a prior's mass a parameter's box may hold (`fluctuate_linear`)


def _truth_args(what, n_j, scale, shift, lower, upper):
    """the parameters' numbers of `fluctuate_linear` as contiguous float64 host arrays [J] (lower / upper: -inf / +inf
    where None).  A box that holds less than TRUTH_MIN_MASS of its prior's mass raises ValueError: the rejection
    loop of the truth draw then ends within its 256 candidates (0.75^256).  A NaN, a negative scale or lower > upper
    goes on to the library, which refuses it."""
    from scipy.stats import norm

    arrays = []
    for name, a, fill in (("scale", scale, None), ("shift", shift, None), ("lower", lower, -np.inf),
                          ("upper", upper, np.inf)):
        a = np.full(n_j, fill) if a is None and fill is not None else np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (n_j,):
            raise ValueError("%s: %s holds one number per parameter [%d]" % (what, name, n_j))
        arrays.append(a)
    scale, shift, lower, upper = arrays
    with np.errstate(all="ignore"):
        drawn = (scale > 0) & np.isfinite(scale) & np.isfinite(shift) & (lower <= upper)
        s = np.where(drawn, scale, 1.0)
        mass = norm.cdf((upper - shift) / s) - norm.cdf((lower - shift) / s)
    for j in np.nonzero(drawn & (mass < TRUTH_MIN_MASS))[0]:
        raise ValueError("%s: the box [%g, %g] of parameter %d holds %.3g of the mass of its prior N(%g, %g); at least "
                         "%g is needed" % (what, lower[j], upper[j], j, mass[j], shift[j], scale[j], TRUTH_MIN_MASS))
    return arrays


def fluctuate_linear(mu, response, n_trials, seed, scale, shift, lower=None, upper=None, method="poisson", sigma=None,
                     stream=0, first_trial=0):
    """Pseudo-data of a linearised template whose nuisance parameters fluctuate (`pisa_hip_fluctuate_linear`,
    DESIGN.md §4): mu [B], response [J, B] and (for "gauss" and "gauss+poisson") sigma [B] float64 device tensors;
    scale, shift, lower, upper [J] host numbers.  Trial t draws the truth of parameter j from N(shift_j, scale_j)
    truncated to [lower_j, upper_j] (scale_j == 0: shift_j itself; None: no bound on that side) and its data by
    `method` from mu + sum_j response[j] eta_j, a negative mean taken as 0.  -> dict(data [n_trials, B], eta
    [n_trials, J]: device tensors; clipped: the number of means that were negative).  With every scale and shift 0 the
    data are `fluctuate`'s, bit for bit.  Entries and truths depend on (seed, stream, first_trial + t, b or j, the
    inputs) alone.  "scaled_poisson" is refused (ValueError), and so is a box that holds less than `TRUTH_MIN_MASS` of
    its prior's mass; errors of the draws are those of `fluctuate`."""
    name = fluctuate_method(method)
    if name == "scaled_poisson":
        raise ValueError("fluctuate_linear: no scaled_poisson draws from a mean that moves per trial (its row rules "
                         "compare a row's variance with its mean)")
    if response.dim() != 2 or response.dtype != F8 or mu.dim() != 1 or response.shape[1] != mu.shape[0] or (
            response.device != mu.device):
        raise ValueError("fluctuate_linear: response is float64 [n_params, n_bins] on mu's device")
    n_j = response.shape[0]
    if not 1 <= n_j <= _lib.PROFILE_MAX_PARAMS:
        raise ValueError("fluctuate_linear: %d nuisance parameters, 1 to %d are drawn" % (n_j, _lib.PROFILE_MAX_PARAMS))
    mu, sigma, n_bins, n_trials, seed, stream, first_trial, out = _draw_args(
        "fluctuate_linear", mu, sigma, name, n_trials, seed, stream, first_trial, None)
    scale, shift, lower, upper = _truth_args("fluctuate_linear", n_j, scale, shift, lower, upper)
    response = response.contiguous()
    eta = torch.empty((out.shape[0], n_j), dtype=F8, device=mu.device)
    status = torch.zeros(2, dtype=torch.int32, device=mu.device)
    _lib.check(_lib.lib().pisa_hip_fluctuate_linear(
        _ptr(mu), _ptr(sigma), _ptr(response), n_j, scale.ctypes.data, shift.ctypes.data, lower.ctypes.data,
        upper.ctypes.data, FLUCTUATE_METHOD[name], n_bins, n_trials, seed, stream, first_trial, _ptr(out), _ptr(eta),
        _ptr(status), _stream()))
    word, clipped = (int(x) for x in status.cpu().numpy())
    if word == _lib.FLUCT_TRUTH_EXHAUSTED:
        raise ValueError("fluctuate_linear: a truth found no candidate inside its box")
    _lib.check(word)
    return dict(data=out, eta=eta, clipped=clipped & 0xFFFFFFFF)


def fluctuate_linear_mvn(mu, response, n_trials, seed, mean, cov, lower=None, upper=None, method="poisson", sigma=None,
                         stream=0, first_trial=0):
    """`fluctuate_linear` with correlated truths, those of a fit to an observed map (`pisa_hip_fluctuate_linear_mvn`;
    DESIGN.md §4, "pseudo-data at nuisances fitted to the observed data"): mean [J] and cov [J, J] host numbers, the
    fitted displacements and their covariance.  Trial t draws its truths from N(mean, cov) truncated to the box
    [lower, upper] by rejection of the whole vector; a coordinate with cov[j, j] == 0 (one the fit holds on a bound:
    its row and column are zero) stays at mean[j].  -> dict(data [n_trials, B], eta [n_trials, J]: device tensors;
    clipped), with the conventions of `fluctuate_linear`.  With a diagonal cov and no box it is `fluctuate_linear(...,
    scale=sqrt(diag(cov)), shift=mean)`, bit for bit.  Refused (ValueError): "scaled_poisson"; a coordinate whose
    marginal N(mean_j, cov_jj) holds less than `TRUTH_MIN_MASS` inside [lower_j, upper_j].  The library refuses
    (PisaHipError, nothing is launched) a cov that is not finite or has no Cholesky factor on its live coordinates, a
    dead coordinate with a non-zero entry in its row or column, and a mean that is not finite or outside its box."""
    name = fluctuate_method(method)
    if name == "scaled_poisson":
        raise ValueError("fluctuate_linear_mvn: no scaled_poisson draws from a mean that moves per trial (its row "
                         "rules compare a row's variance with its mean)")
    if response.dim() != 2 or response.dtype != F8 or mu.dim() != 1 or response.shape[1] != mu.shape[0] or (
            response.device != mu.device):
        raise ValueError("fluctuate_linear_mvn: response is float64 [n_params, n_bins] on mu's device")
    n_j = response.shape[0]
    if not 1 <= n_j <= _lib.PROFILE_MAX_PARAMS:
        raise ValueError("fluctuate_linear_mvn: %d nuisance parameters, 1 to %d are drawn"
                         % (n_j, _lib.PROFILE_MAX_PARAMS))
    mu, sigma, n_bins, n_trials, seed, stream, first_trial, out = _draw_args(
        "fluctuate_linear_mvn", mu, sigma, name, n_trials, seed, stream, first_trial, None)
    cov = np.ascontiguousarray(cov, dtype=np.float64)
    if cov.shape != (n_j, n_j):
        raise ValueError("fluctuate_linear_mvn: cov is [%d, %d]" % (n_j, n_j))
    with np.errstate(all="ignore"):
        var = np.diagonal(cov)
        scale = np.where(var > 0, np.sqrt(np.where(var > 0, var, 0.0)), 0.0)     # (anything else: the library's)
    _, mean, lower, upper = _truth_args("fluctuate_linear_mvn", n_j, scale, mean, lower, upper)
    response = response.contiguous()
    eta = torch.empty((out.shape[0], n_j), dtype=F8, device=mu.device)
    status = torch.zeros(2, dtype=torch.int32, device=mu.device)
    _lib.check(_lib.lib().pisa_hip_fluctuate_linear_mvn(
        _ptr(mu), _ptr(sigma), _ptr(response), n_j, mean.ctypes.data, cov.ctypes.data, lower.ctypes.data,
        upper.ctypes.data, FLUCTUATE_METHOD[name], n_bins, n_trials, seed, stream, first_trial, _ptr(out), _ptr(eta),
        _ptr(status), _stream()))
    word, clipped = (int(x) for x in status.cpu().numpy())
    if word == _lib.FLUCT_TRUTH_EXHAUSTED:
        raise ValueError("fluctuate_linear_mvn: a trial found no candidate inside the box")
    _lib.check(word)
    return dict(data=out, eta=eta, clipped=clipped & 0xFFFFFFFF)


def fluctuate_linear_at(mu, response, eta, seed, method="poisson", sigma=None, stream=0, first_trial=0):
    """`fluctuate_linear` at truths the caller gives (`pisa_hip_fluctuate_linear_at`): eta [n_trials, J] float64 device
    tensor, row t the truths of trial number first_trial + t (rows of a posterior sample of `posterior_sample`, for
    one); nothing is drawn for them.  -> dict(data [n_trials, B], eta: the tensor that was read, clipped), with the
    conventions of `fluctuate_linear`.  With every row equal to `shift` the data are those of `fluctuate_linear` with
    every scale 0, bit for bit.  A NaN truth gives NaN data.  "scaled_poisson" is refused (ValueError)."""
    name = fluctuate_method(method)
    if name == "scaled_poisson":
        raise ValueError("fluctuate_linear_at: no scaled_poisson draws from a mean that moves per trial (its row rules "
                         "compare a row's variance with its mean)")
    if response.dim() != 2 or response.dtype != F8 or mu.dim() != 1 or response.shape[1] != mu.shape[0] or (
            response.device != mu.device):
        raise ValueError("fluctuate_linear_at: response is float64 [n_params, n_bins] on mu's device")
    n_j = response.shape[0]
    if not 1 <= n_j <= _lib.PROFILE_MAX_PARAMS:
        raise ValueError("fluctuate_linear_at: %d nuisance parameters, 1 to %d are taken"
                         % (n_j, _lib.PROFILE_MAX_PARAMS))
    if eta.dim() != 2 or eta.dtype != F8 or eta.shape[1] != n_j or eta.device != mu.device:
        raise ValueError("fluctuate_linear_at: eta is float64 [n_trials, n_params] on mu's device")
    mu, sigma, n_bins, n_trials, seed, stream, first_trial, out = _draw_args(
        "fluctuate_linear_at", mu, sigma, name, eta.shape[0], seed, stream, first_trial, None)
    response, eta = response.contiguous(), eta.contiguous()
    status = torch.zeros(2, dtype=torch.int32, device=mu.device)
    _lib.check(_lib.lib().pisa_hip_fluctuate_linear_at(
        _ptr(mu), _ptr(sigma), _ptr(response), n_j, _ptr(eta), FLUCTUATE_METHOD[name], n_bins, n_trials, seed, stream,
        first_trial, _ptr(out), _ptr(status), _stream()))
    word, clipped = (int(x) for x in status.cpu().numpy())
    _lib.check(word)
    return dict(data=out, eta=eta, clipped=clipped & 0xFFFFFFFF)


def _profile_args(what, kind, data, expected, response, sigma2, inv_prior_sigma, center, max_iter,
                  most=_lib.PROFILE_MAX_PARAMS):
    if kind in ENSEMBLE_MC_KINDS:
        raise ValueError("%s: '%s' has no profiled form (its per-bin function is not convex in the response)"
                         % (what, kind))
    if kind not in METRIC_KIND:
        raise ValueError("%s: metric '%s' not among %s" % (what, kind, sorted(METRIC_KIND)))
    data, expected, sigma2 = _maps_args(what, data, expected, sigma2)
    if kind == "mod_chi2" and sigma2 is None:
        raise ValueError("%s: mod_chi2 needs sigma2" % what)
    n_k, n_b = expected.shape
    if response.dtype != F8 or response.dim() not in (2, 3) or response.shape[-1] != n_b or (
            response.dim() == 3 and response.shape[0] != n_k):
        raise ValueError("%s: response is float64 [n_templates, n_params, n_bins], or [n_params, n_bins] shared by "
                         "all templates" % what)
    n_j = response.shape[-2]
    if not 1 <= n_j <= most:
        raise ValueError("%s: %d nuisance parameters, 1 to %d are fitted" % (what, n_j, most))
    if inv_prior_sigma is not None and (inv_prior_sigma.shape != (n_j,) or inv_prior_sigma.dtype != F8):
        raise ValueError("%s: inv_prior_sigma is float64 [n_params]" % what)
    if center is not None and (center.shape != (n_k, n_j) or center.dtype != F8):
        raise ValueError("%s: center is float64 [n_templates, n_params]" % what)
    if int(max_iter) < 0:
        raise ValueError("%s: max_iter >= 0" % what)
    response = response.contiguous()
    inv_prior_sigma = None if inv_prior_sigma is None else inv_prior_sigma.contiguous()
    center = None if center is None else center.contiguous()
    stride = n_j * n_b if response.dim() == 3 else 0
    if data.shape[1] != n_b:
        raise ValueError("%s: data has %d bins, expected %d" % (what, data.shape[1], n_b))
    return data, expected, response, sigma2, inv_prior_sigma, center, stride, data.shape[0], n_k, n_b, n_j


def _bound_args(what, lower, upper, n_k, n_j):
    """(lower, upper, stride) of the bounded entry points: float64 device tensors [n_params] (stride 0: shared by all
    templates) or [n_templates, n_params]; either may be None (no bound on that side).  One of each form: the shared
    one is written out per template, since both are read with one stride."""
    for name, b in (("lower", lower), ("upper", upper)):
        if b is not None and (b.dtype != F8 or tuple(b.shape) not in ((n_j,), (n_k, n_j))):
            raise ValueError("%s: %s is float64 [n_params] or [n_templates, n_params]" % (what, name))
    per_template = any(b is not None and b.dim() == 2 for b in (lower, upper))
    out = [None if b is None else (b.expand(n_k, n_j) if per_template else b).contiguous() for b in (lower, upper)]
    return out[0], out[1], n_j if per_template else 0


RESPONSE_FORM = {"linear": _lib.RESPONSE_LINEAR, "loglinear": _lib.RESPONSE_LOGLINEAR}


def _profiled_call(what, wide, kind, data, expected, response, sigma2, inv_prior_sigma, center, max_iter, lower, upper,
                   form="linear"):
    """the checked inputs of a profiled matrix call -> (the entry points' suffix, the arguments they begin with: [kind
    ... center, (the bounds)], n_params, [max_iter, T, K, B], the tensors behind the pointers, data first).  The narrow
    form without bounds goes to the unbounded entry points, with bounds to the `_bounded` ones; the wide entry points
    take the bounds always (NULL: none).  A form other than "linear" (the wide form alone) goes to the `_wide_form`
    entry points, which take the form after the kind."""
    if form not in RESPONSE_FORM or (form != "linear" and not wide):
        raise ValueError("%s: form '%s' is not one of 'linear', 'loglinear'%s"
                         % (what, form, "" if wide else " (the narrow form is linear)"))
    (data, expected, response, sigma2, ips, center, stride, n_t, n_k, n_bins, n_j) = _profile_args(
        what, kind, data, expected, response, sigma2, inv_prior_sigma, center, max_iter,
        _lib.PROFILE_WIDE_MAX_PARAMS if wide else _lib.PROFILE_MAX_PARAMS)
    bounded = lower is not None or upper is not None
    head = [METRIC_KIND[kind], _ptr(data), _ptr(expected), _ptr(sigma2), _ptr(response), stride, _ptr(ips),
            _ptr(center)]
    if bounded:
        lower, upper, b_stride = _bound_args(what, lower, upper, n_k, n_j)
        head += [_ptr(lower), _ptr(upper), b_stride]
    elif wide:
        head += [None, None, 0]
    keep = (data, expected, response, sigma2, ips, center, lower, upper)     # (alive until the launch)
    if form != "linear":
        return "_wide_form", head[:1] + [RESPONSE_FORM[form]] + head[1:], n_j, [int(max_iter), n_t, n_k, n_bins], keep
    return "_wide" if wide else "_bounded" if bounded else "", head, n_j, [int(max_iter), n_t, n_k, n_bins], keep


def _profiled_full(what, wide, kind, data, expected, response, sigma2, inv_prior_sigma, center, max_iter, want_eta,
                   status, lower, upper, form="linear"):
    """the body of `profiled_metric_matrix` and `profiled_metric_matrix_wide`"""
    suffix, head, n_j, sizes, keep = _profiled_call(what, wide, kind, data, expected, response, sigma2, inv_prior_sigma,
                                                    center, max_iter, lower, upper, form)
    n_t, n_k, dev = sizes[1], sizes[2], keep[0].device
    value = torch.empty((n_t, n_k), dtype=F8, device=dev)
    eta = torch.empty((n_t, n_k, n_j), dtype=F8, device=dev) if want_eta else None
    n_iter = torch.empty((n_t, n_k), dtype=torch.int32, device=dev)
    pair_status = torch.empty((n_t, n_k), dtype=torch.int32, device=dev)
    entry = getattr(_lib.lib(), "pisa_hip_profiled_metric_matrix" + suffix)

    def launch(status):
        _lib.check(entry(*head, n_j, *sizes, _ptr(value), _ptr(eta), _ptr(n_iter), _ptr(pair_status), _ptr(status),
                         _stream()))

    _with_status(status, dev, launch)
    return dict(value=value, eta=eta, n_iter=n_iter, status=pair_status)


def _profiled_best(what, wide, kind, data, expected, response, sigma2, inv_prior_sigma, center, offset, k0, max_iter,
                   status, lower, upper, form="linear"):
    """the body of `profiled_metric_matrix_best` and `profiled_metric_matrix_best_wide`"""
    suffix, head, n_j, sizes, keep = _profiled_call(what, wide, kind, data, expected, response, sigma2, inv_prior_sigma,
                                                    center, max_iter, lower, upper, form)
    n_t, n_k, dev = sizes[1], sizes[2], keep[0].device
    offset = _offset_arg(what, offset, n_k)
    best = torch.empty(n_t, dtype=F8, device=dev)
    arg = torch.empty(n_t, dtype=torch.int32, device=dev)
    at = torch.empty(n_t, dtype=F8, device=dev)
    eta_best = torch.empty((n_t, n_j), dtype=F8, device=dev)
    eta_at = torch.empty((n_t, n_j), dtype=F8, device=dev)
    trial_status = torch.empty(n_t, dtype=torch.int32, device=dev)
    entry = getattr(_lib.lib(), "pisa_hip_profiled_metric_matrix_best" + suffix)

    def launch(status):
        _lib.check(entry(*head, _ptr(offset), int(k0), n_j, *sizes, _ptr(best), _ptr(arg), _ptr(at), _ptr(eta_best),
                         _ptr(eta_at), _ptr(trial_status), _ptr(status), _stream()))

    _with_status(status, dev, launch)
    return dict(best=best, arg=arg, at=at, eta_best=eta_best, eta_at=eta_at, status=trial_status)


def profiled_metric_matrix(kind, data, expected, response, sigma2=None, inv_prior_sigma=None, center=None,
                           max_iter=32, want_eta=True, status=None, lower=None, upper=None):
    """`metric_matrix` with linearised nuisance parameters fitted per (trial, template) pair
    (`pisa_hip_profiled_metric_matrix`): the template of pair (t, k) is expected[k] + sum_j response[k, j]
    eta_j with eta minimising the metric's own convex objective plus the Gaussian priors (inv_prior_sigma_j (eta_j +
    center[k, j]))^2.  data [T, B], expected / sigma2 [K, B], response [K, J, B] or [J, B] (shared), inv_prior_sigma
    [J], center [K, J]: float64 device tensors.  -> dict(value [T, K], eta [T, K, J] (None unless want_eta), n_iter
    [T, K] int32, status [T, K] int32: the `_lib.PROFILE_*` bit flags; a flagged pair holds the metric at its last
    accepted eta).  A negative datum or expectation raises ValueError.
    lower / upper (float64 device tensors [J] or [K, J]; either may be None): eta is fitted inside lower <= eta <= upper
    (`pisa_hip_profiled_metric_matrix_bounded`; displacements in the parameter's units, -inf / +inf for no bound,
    lower == upper pins a parameter).  A fitted coordinate on a bound equals the bound; a template with lower > upper
    or a NaN bound gives pairs flagged `_lib.PROFILE_BAD_BOUNDS` that stay at eta = 0.  With both None the call is
    what it was before the arguments existed."""
    return _profiled_full("profiled_metric_matrix", False, kind, data, expected, response, sigma2, inv_prior_sigma,
                          center, max_iter, want_eta, status, lower, upper)


def profiled_metric_matrix_best(kind, data, expected, response, sigma2=None, inv_prior_sigma=None, center=None,
                                offset=None, k0=0, max_iter=32, status=None, lower=None, upper=None):
    """the matrix of `profiled_metric_matrix` (+ offset [K] per column) reduced per trial without being written
    (`pisa_hip_profiled_metric_matrix_best`) -> dict(best [T], arg [T] int32, at [T]: column k0, eta_best and eta_at
    [T, J]: the fitted displacements at both columns, status [T] int32: the flags of the pair at arg OR those of
    the pair at k0), bit for bit the reduction of the full output.  lower / upper: as in `profiled_metric_matrix`
    (`pisa_hip_profiled_metric_matrix_best_bounded`)"""
    return _profiled_best("profiled_metric_matrix_best", False, kind, data, expected, response, sigma2, inv_prior_sigma,
                          center, offset, k0, max_iter, status, lower, upper)


def profiled_metric_matrix_wide(kind, data, expected, response, sigma2=None, inv_prior_sigma=None, center=None,
                                max_iter=32, want_eta=True, status=None, lower=None, upper=None, form="linear"):
    """`profiled_metric_matrix` in the wide form (`pisa_hip_profiled_metric_matrix_wide`, DESIGN.md §4, "Profiled
    trial ensembles: more than 8 parameters"): the same fit, arguments and outputs with 1 to
    `_lib.PROFILE_WIDE_MAX_PARAMS` = 32 nuisance parameters, one wavefront per (trial, template) pair.  With both
    bounds None it is the unbounded fit, otherwise the bounded one; up to 8 parameters the outputs are bit for bit those
    of `profiled_metric_matrix`.
    form="loglinear" (`pisa_hip_profiled_metric_matrix_wide_form`, DESIGN.md §4, "Profiled trial ensembles: the
    log-linear response"): `response` holds rho and the template of pair (t, k) is expected[k] * exp(sum_j rho[k, j]
    eta_j): positive for every eta, with all cross terms of a product of factors.  Everything else is the same fit.
    Any other form than "linear" and "loglinear" raises ValueError."""
    return _profiled_full("profiled_metric_matrix_wide", True, kind, data, expected, response, sigma2, inv_prior_sigma,
                          center, max_iter, want_eta, status, lower, upper, form)


def profiled_metric_matrix_best_wide(kind, data, expected, response, sigma2=None, inv_prior_sigma=None, center=None,
                                     offset=None, k0=0, max_iter=32, status=None, lower=None, upper=None,
                                     form="linear"):
    """`profiled_metric_matrix_best` in the wide form (`pisa_hip_profiled_metric_matrix_best_wide`): the reduction of
    `profiled_metric_matrix_wide` per trial, bit for bit, with 1 to 32 nuisance parameters; form: as there
    (`pisa_hip_profiled_metric_matrix_best_wide_form`)"""
    return _profiled_best("profiled_metric_matrix_best_wide", True, kind, data, expected, response, sigma2,
                          inv_prior_sigma, center, offset, k0, max_iter, status, lower, upper, form)


def profiled_hesse(kind, data, expected, response, eta, k, sigma2=None, inv_prior_sigma=None, center=None, lower=None,
                   upper=None):
    """The covariance of the fitted displacements of `profiled_metric_matrix_best` (`pisa_hip_profiled_hesse`,
    DESIGN.md §4): eta [T, J] float64 device tensor (normally `eta_best` or `eta_at` of that call) and k, the template
    of every trial: an int32 device tensor [T] (normally `arg`) or one int for all.  The other arguments are the
    fit's.  -> dict(cov [T, J, J]: the inverse Hessian of -ln L at eta, the prior terms included (for the chi2 kinds
    2 / the Hessian of chi2), symmetric bit for bit; sigma [T, J] = sqrt(diag cov); status [T] int32).  With lower /
    upper the coordinates the fit holds on a bound have zero rows and columns (sigma 0) and the trial
    `_lib.PROFILE_HELD`; a trial flagged NOT_POSDEF, START_OUTSIDE or BAD_BOUNDS has a NaN covariance.  A negative datum
    or expectation raises ValueError, a k outside the templates `_lib.PisaHipError`."""
    (data, expected, response, sigma2, ips, center, stride, n_t, n_k, n_bins, n_j) = _profile_args(
        "profiled_hesse", kind, data, expected, response, sigma2, inv_prior_sigma, center, 0)
    b_stride = 0
    if lower is not None or upper is not None:
        lower, upper, b_stride = _bound_args("profiled_hesse", lower, upper, n_k, n_j)
    if eta.dtype != F8 or tuple(eta.shape) != (n_t, n_j):
        raise ValueError("profiled_hesse: eta is float64 [n_trials, n_params]")
    eta = eta.contiguous()
    k_of_trial, k0 = None, 0
    if isinstance(k, torch.Tensor):
        if k.dtype != torch.int32 or tuple(k.shape) != (n_t,) or k.device != data.device:
            raise ValueError("profiled_hesse: k is one int, or an int32 tensor [n_trials] on the data's device")
        k_of_trial = k.contiguous()
    else:
        k0 = int(k)
        if not 0 <= k0 < n_k:
            raise ValueError("profiled_hesse: k = %d outside the %d templates" % (k0, n_k))
    dev = data.device
    cov = torch.empty((n_t, n_j, n_j), dtype=F8, device=dev)
    trial_status = torch.empty(n_t, dtype=torch.int32, device=dev)

    def launch(status):
        _lib.check(_lib.lib().pisa_hip_profiled_hesse(
            METRIC_KIND[kind], _ptr(data), _ptr(expected), _ptr(sigma2), _ptr(response), stride, _ptr(ips),
            _ptr(center), _ptr(lower), _ptr(upper), b_stride, n_j, n_t, n_k, n_bins, _ptr(k_of_trial), k0, _ptr(eta),
            _ptr(cov), _ptr(trial_status), _ptr(status), _stream()))

    _with_status(None, dev, launch)
    sigma = bin_sqrt(torch.diagonal(cov, dim1=1, dim2=2).contiguous())
    return dict(cov=cov, sigma=sigma, status=trial_status)


def posterior_n_keep(first_step, n_steps, keep_from=0, thin=1):
    """the number of kept steps of `posterior_sample`: the s of [first_step, first_step + n_steps) with s >= keep_from
    and (s - keep_from) % thin == 0"""
    first_step, n_steps, keep_from, thin = int(first_step), int(n_steps), int(keep_from), int(thin)
    if thin < 1:
        raise ValueError("posterior_sample: thin >= 1")
    s0 = keep_from if first_step <= keep_from else keep_from + -(-(first_step - keep_from) // thin) * thin
    return max(0, -(-(first_step + n_steps - s0) // thin))


def posterior_layout(kind, n_params, n_walkers):
    """how `pisa_hip_posterior_sample` places an ensemble (csrc/posterior.hip) -> dict(problems: the problems of one
    workgroup; stage_bins: the most bins whose rows it keeps in LDS -- longer rows are streamed by every sweep).  The
    results do not depend on either; tests pick their sizes by them."""
    per = min(_lib.POSTERIOR_THREADS // (int(n_walkers) // 2), _lib.POSTERIOR_MAX_PROBLEMS)
    rows = int(n_params) + 2 + (1 if kind == "mod_chi2" else 0)
    return dict(problems=per, stage_bins=_lib.POSTERIOR_STAGE // (per * rows))


def posterior_sample(kind, data, expected, response, x0, n_steps, seed, t_of=None, k_of=None, sigma2=None,
                     inv_prior_sigma=None, center=None, lower=None, upper=None, stream=0, chain_id=None, first_step=0,
                     keep_from=0, thin=1):
    """Samples of the posterior of the linearised nuisance displacements, p(eta | data row, template row), by a
    Goodman-Weare stretch-move ensemble sampler on the device (`pisa_hip_posterior_sample`; DESIGN.md §4, "Trial
    ensembles: the nuisance posterior").  data [T, B], expected / sigma2 [K, B], response [K, J, B] or [J, B],
    inv_prior_sigma [J], center [K, J], lower / upper [J] or [K, J]: the arguments of `profiled_metric_matrix`, and
    ln p(eta) = -Phi(eta) (the llh kinds) or -Phi(eta) / 2 (the chi2 kinds) of its objective Phi, -inf outside the box
    and outside the solver's domain.  x0 [P, W, J]: the starts of P problems of W walkers (W even, 2 J <= W <= 256);
    problem p takes data row t_of[p] and template row k_of[p] (int32 device tensors [P]; None: p itself, or row 0
    where there is one row only) and the random numbers of (seed, stream, chain_id[p]) (chain_id: int tensor [P];
    None: p).  Steps first_step ... first_step + n_steps - 1 are taken; step s is kept iff s >= keep_from and
    (s - keep_from) % thin == 0.
    -> dict(chain [P, n_keep, W, J], logp [P, n_keep, W], accepted [P, W] int32, end [P, W, J], status [P] int32: 0,
    `_lib.PROFILE_START_OUTSIDE` (a walker starts where ln p is -inf or NaN) or `_lib.PROFILE_BAD_BOUNDS`; a flagged
    problem is NaN).  The bits of a problem depend on its rows, its start, (seed, stream, chain_id) and the step numbers
    alone: a call continued from `end` with first_step advanced equals one longer call.  A negative datum or
    expectation raises ValueError, a row index outside its array `_lib.PisaHipError`."""
    what = "posterior_sample"
    (data, expected, response, sigma2, ips, center, stride, n_t, n_k, n_bins, n_j) = _profile_args(
        what, kind, data, expected, response, sigma2, inv_prior_sigma, center, 0)
    b_stride = 0
    if lower is not None or upper is not None:
        lower, upper, b_stride = _bound_args(what, lower, upper, n_k, n_j)
    dev = data.device
    if x0.dim() != 3 or x0.dtype != F8 or x0.shape[2] != n_j or x0.device != dev:
        raise ValueError("%s: x0 is float64 [n_problems, n_walkers, n_params] on the data's device" % what)
    n_p, n_w = int(x0.shape[0]), int(x0.shape[1])
    if n_w % 2 or not max(2, 2 * n_j) <= n_w <= _lib.POSTERIOR_MAX_WALKERS:
        raise ValueError("%s: %d walkers; an even number from %d (twice the parameters) to %d"
                         % (what, n_w, max(2, 2 * n_j), _lib.POSTERIOR_MAX_WALKERS))
    x0 = x0.contiguous()
    index = []
    for name, idx, rows in (("t_of", t_of, n_t), ("k_of", k_of, n_k)):
        if idx is None:
            idx = torch.zeros(n_p, dtype=torch.int32, device=dev) if rows == 1 and n_p > 1 else None
        elif idx.dtype != torch.int32 or tuple(idx.shape) != (n_p,) or idx.device != dev:
            raise ValueError("%s: %s is an int32 tensor [n_problems] on the data's device" % (what, name))
        index.append(None if idx is None else idx.contiguous())
    if chain_id is not None:
        if tuple(chain_id.shape) != (n_p,) or chain_id.device != dev or chain_id.is_floating_point():
            raise ValueError("%s: chain_id is an integer tensor [n_problems] on the data's device" % what)
        if n_p and (int(chain_id.min()) < 0 or int(chain_id.max()) >= 2 ** 32):
            raise ValueError("%s: chain ids are in [0, 2^32)" % what)
        # (the library reads 32-bit words: the low word of a little-endian int64 is the id)
        chain_id = chain_id.to(torch.int64).contiguous().view(torch.int32)[::2].contiguous()
    seed, stream = int(seed), int(stream)
    first_step, n_steps, keep_from, thin = int(first_step), int(n_steps), int(keep_from), int(thin)
    if not 0 <= seed < 2 ** 64 or not 0 <= stream < 2 ** 32:
        raise ValueError("%s: the seed is in [0, 2^64) and stream in [0, 2^32)" % what)
    if first_step < 0 or keep_from < 0 or n_steps < 1 or first_step + n_steps > 2 ** 32:
        raise ValueError("%s: step numbers are in [0, 2^32), and at least one step is taken" % what)
    n_keep = posterior_n_keep(first_step, n_steps, keep_from, thin)
    chain = torch.empty((n_p, n_keep, n_w, n_j), dtype=F8, device=dev)
    logp = torch.empty((n_p, n_keep, n_w), dtype=F8, device=dev)
    accepted = torch.empty((n_p, n_w), dtype=torch.int32, device=dev)
    end = torch.empty((n_p, n_w, n_j), dtype=F8, device=dev)
    problem_status = torch.empty(n_p, dtype=torch.int32, device=dev)

    def launch(status):
        _lib.check(_lib.lib().pisa_hip_posterior_sample(
            METRIC_KIND[kind], _ptr(data), _ptr(expected), _ptr(sigma2), _ptr(response), stride, _ptr(ips),
            _ptr(center), _ptr(lower), _ptr(upper), b_stride, n_j, n_t, n_k, n_bins, n_p, _ptr(index[0]),
            _ptr(index[1]), _ptr(chain_id), n_w, _ptr(x0), seed, stream, first_step, n_steps, keep_from, thin, n_keep,
            _ptr(chain) if n_keep else None, _ptr(logp) if n_keep else None, _ptr(accepted), _ptr(end),
            _ptr(problem_status), _ptr(status), _stream()))

    _with_status(None, dev, launch)
    return dict(chain=chain, logp=logp, accepted=accepted, end=end, status=problem_status)


# --------------------------------------------------- generalized Poisson-gamma likelihood
def gpllh_bin_sums(weights, index, offsets):
    """(Sigma w, Sigma w^2) per bin, bin b's events being weights[index[offsets[b]:offsets[b + 1]]]
    (`pisa_hip_gpllh_bin_sums`); a negative weight among them raises"""
    n_bins = int(offsets.numel()) - 1
    dev = weights.device
    sw = torch.empty(n_bins, dtype=F8, device=dev)
    sw2 = torch.empty(n_bins, dtype=F8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().pisa_hip_gpllh_bin_sums(_ptr(weights), _ptr(index), _ptr(offsets), n_bins, _ptr(sw),
                                                  _ptr(sw2), _ptr(status), _stream()))
    _check_status(status)
    return sw, sw2


def gpllh_params(sumw, sumw2, n_mc, adjust):
    """generalized_llh_params per (container, bin): [n_cont, n_bins] sums and MC counts, [n_cont] mean
    adjustments -> (alpha, beta, weight sums with the pseudo-weight) (`pisa_hip_gpllh_params`)"""
    n_cont, n_bins = sumw.shape
    dev = sumw.device
    out = [torch.empty((n_cont, n_bins), dtype=F8, device=dev) for _ in range(3)]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().pisa_hip_gpllh_params(_ptr(sumw), _ptr(sumw2), _ptr(n_mc), _ptr(adjust), n_cont, n_bins,
                                                _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(status), _stream()))
    _check_status(status)
    return tuple(out)


def gpllh_scratch_k(actual, n_mc, empty=None):
    """the largest data count among the bins that may take the eq. 91 mixture (some container with at most 100
    MC events, not listed empty): the recursion length the metric must make room for"""
    mix = (n_mc <= 100.0).any(dim=0)
    if empty is not None:
        mix &= empty == 0
    if not bool(mix.any()):
        return 0
    k = actual[mix]
    k = k[torch.isfinite(k)]
    return int(k.max().item()) if k.numel() else 0


def gpllh_scratch(n_points, n_bins, scratch_k, dev):
    """the global scratch of mixture bins beyond the LDS (None when every one fits there)"""
    if scratch_k <= _lib.GPLLH_LDS_K:
        return None
    return torch.empty(n_points * n_bins * 2 * (scratch_k + 1), dtype=F8, device=dev)


def generalized_poisson_llh(actual, weights, alpha, beta, n_mc, empty=None):
    """stats.generalized_poisson_llh on device (`pisa_hip_generalized_poisson_llh`): actual [n_bins],
    weights / alpha / beta / n_mc [n_cont, n_bins], empty [n_bins] uint8 or None -> (total [1], per-bin [n_bins])"""
    n_cont, n_bins = weights.shape
    dev = actual.device
    scratch_k = gpllh_scratch_k(actual, n_mc, empty)
    scratch = gpllh_scratch(1, n_bins, scratch_k, dev)
    per_bin = torch.empty(n_bins, dtype=F8, device=dev)
    total = torch.empty(1, dtype=F8, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)     # [status, arrival counter of the total]
    _lib.check(_lib.lib().pisa_hip_generalized_poisson_llh(
        _ptr(actual), _ptr(weights), _ptr(alpha), _ptr(beta), _ptr(n_mc), n_cont, n_bins, _ptr(empty),
        _ptr(scratch), scratch_k, _ptr(per_bin), C.c_void_p(status.data_ptr() + 4), _ptr(total), _ptr(status),
        _stream()))
    status = status[:1]
    _check_status(status)
    return total, per_bin


# --------------------------------------------------------------- Fisher matrix and pulls
def fisher(hist, sumw2, lo, hi, dx, truth=None):
    """Fisher matrix, gradients and pull vector of n_points templates on device (`pisa_hip_fisher`):
    hist / sumw2 [n_points, n_rows, n_bins] (or [n_points, n_bins]: totals), point 0 the fiducial; per parameter
    the point indices lo / hi of its sorted test values and dx = hi - lo; truth [n_bins] or None.
    Returns a dict of device tensors grad [P, n_bins], matrix [P, P], pull [P] (None without truth),
    totals [n_points, n_bins], var0 [n_bins], and host ints nonempty (bins with a nonzero fiducial) and status
    (0, or `_lib.FISHER_ZERO_SIGMA`: a nonempty bin without error)."""
    if hist.dim() == 2:
        hist, sumw2 = hist.unsqueeze(1), sumw2.unsqueeze(1)
    assert hist.shape == sumw2.shape and hist.dtype == sumw2.dtype == F8
    hist, sumw2 = hist.contiguous(), sumw2.contiguous()
    n_points, n_rows, n_bins = hist.shape
    n_par = len(dx)
    if not (len(lo) == len(hi) == n_par):
        raise ValueError("fisher: lo, hi and dx need one entry per parameter")
    dev = hist.device
    grad = torch.empty((max(n_par, 1), n_bins), dtype=F8, device=dev)
    matrix = torch.empty((max(n_par, 1), max(n_par, 1)), dtype=F8, device=dev)
    pull = torch.empty(max(n_par, 1), dtype=F8, device=dev) if truth is not None else None
    totals = torch.empty((n_points, n_bins), dtype=F8, device=dev)
    var0 = torch.empty(n_bins, dtype=F8, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)      # [nonempty, status (low 4 bytes)]
    if truth is not None:
        truth = truth.to(device=dev, dtype=F8).contiguous()
    a_lo = (C.c_int32 * max(n_par, 1))(*[int(i) for i in lo])
    a_hi = (C.c_int32 * max(n_par, 1))(*[int(i) for i in hi])
    a_dx = (C.c_double * max(n_par, 1))(*[float(x) for x in dx])
    _lib.check(_lib.lib().pisa_hip_fisher(
        _ptr(hist), _ptr(sumw2), n_points, n_rows, n_bins, n_par, a_lo, a_hi, a_dx, _ptr(truth), _ptr(grad),
        _ptr(matrix), _ptr(pull), _ptr(totals), _ptr(var0), C.c_void_p(info.data_ptr()),
        C.c_void_p(info.data_ptr() + 8), _stream()))
    nonempty, status = (int(v) for v in info.cpu())
    return dict(grad=grad, matrix=matrix, pull=pull, totals=totals, var0=var0, nonempty=nonempty,
                status=status & 0xFFFFFFFF)


def hypersurface_fit(x, forms, y, sigma, p0, lo, hi, inv_prior_sigma, log_mode, fix_intercept=False, max_iter=200):
    """n_prob independent hypersurface fits in one launch (`pisa_hip_hypersurface_fit`): host x [n_par, n_sets]
    (value - nominal), forms [n_par] names of `_lib.HSFIT_FORMS`, device y / sigma [n_sets, n_prob], host p0 / lo /
    hi / inv_prior_sigma [n_coef] (intercept first; +-inf: no bound; 0: no prior).  Returns a dict of device
    tensors coef [n_prob, C], cov [n_prob, C, C], chi2 [n_sets, n_prob], loss [n_prob], n_iter and status
    [n_prob] (int32; bit flags `_lib.HSFIT_*`)."""
    x = np.ascontiguousarray(x, np.float64)
    if x.ndim != 2 or len(forms) != x.shape[0]:
        raise ValueError("hypersurface_fit: x is [n_par, n_sets] with one form per parameter")
    for f in forms:
        if f not in _lib.HSFIT_FORMS:
            raise ValueError("Hypersurface function '%s' not known; choose from %s" % (f, list(_lib.HSFIT_FORMS)))
    n_par, n_sets = x.shape
    assert y.shape == sigma.shape and y.dim() == 2 and y.shape[0] == n_sets and y.dtype == sigma.dtype == F8
    y, sigma = y.contiguous(), sigma.contiguous()
    n_prob = y.shape[1]
    host = [np.ascontiguousarray(v, np.float64).reshape(-1) for v in (p0, lo, hi, inv_prior_sigma)]
    n_coef = host[0].size
    if any(v.size != n_coef for v in host):
        raise ValueError("hypersurface_fit: p0, lo, hi and inv_prior_sigma need one entry per coefficient")
    dev = y.device
    a_form = (C.c_int32 * max(n_par, 1))(*[_lib.HSFIT_FORMS.index(f) for f in forms])
    work = torch.empty(max(x.size, 1), dtype=F8, device=dev)
    out = dict(coef=torch.empty((n_prob, n_coef), dtype=F8, device=dev),
               cov=torch.empty((n_prob, n_coef, n_coef), dtype=F8, device=dev),
               chi2=torch.empty((n_sets, n_prob), dtype=F8, device=dev),
               loss=torch.empty(n_prob, dtype=F8, device=dev),
               n_iter=torch.empty(n_prob, dtype=torch.int32, device=dev),
               status=torch.empty(n_prob, dtype=torch.int32, device=dev))
    _lib.check(_lib.lib().pisa_hip_hypersurface_fit(
        x.ctypes.data_as(C.c_void_p), a_form, n_par, n_sets, n_prob, _ptr(y), _ptr(sigma),
        *[v.ctypes.data_as(C.c_void_p) for v in host], n_coef, int(bool(log_mode)), int(bool(fix_intercept)),
        int(max_iter), _ptr(work), _ptr(out["coef"]), _ptr(out["cov"]), _ptr(out["chi2"]), _ptr(out["loss"]),
        _ptr(out["n_iter"]), _ptr(out["status"]), _stream()))
    return out


def bin_scale(x, scale=None, scalar=1.0, floor=None, out=None):
    """out = x * scale * scalar [floored]; see `pisa_hip_bin_scale`."""
    lib = _lib.lib()
    if out is None:
        out = torch.empty_like(x)
    _lib.check(lib.pisa_hip_bin_scale(_ptr(x), _ptr(scale), float(scalar), 0 if floor is None else 1,
                                      0.0 if floor is None else float(floor), x.numel(), _ptr(out),
                                      _stream()))
    return out


def lookup_indices(sample, edges):
    """flat bin number (int64) of every event by the bin edges: -1 below, n_bins above (`pisa_hip_lookup_indices`)"""
    lib = _lib.lib()
    n = sample[0].numel()
    ndim = len(sample)
    edges = [e.contiguous() for e in edges]
    n_edges = (C.c_int32 * ndim)(*[e.numel() for e in edges])
    out = torch.empty(n, dtype=torch.int64, device=sample[0].device)
    _lib.check(lib.pisa_hip_lookup_indices(_sample_array(sample), _sample_array(edges), n_edges, ndim, n, _ptr(out),
                                           _stream()))
    return out


def two_nu_osc(nu_flux, theta, deltam31, energy, coszen, flav, weights):
    """weights *= flux x two-flavour probability, in place (`pisa_hip_two_nu_osc`)"""
    lib = _lib.lib()
    assert nu_flux.is_contiguous() and nu_flux.shape == (energy.numel(), 2) and weights.is_contiguous()
    _lib.check(lib.pisa_hip_two_nu_osc(_ptr(nu_flux), float(theta), float(deltam31), _ptr(energy), _ptr(coszen), int(flav),
                                       energy.numel(), _ptr(weights), _stream()))
    return weights


def power_law(energy, pivot, index, norm=1.0, nominal=None, out=None):
    """norm * nominal * (E / pivot)^index (`pisa_hip_power_law`)"""
    lib = _lib.lib()
    if out is None:
        out = torch.empty_like(energy)
    _lib.check(lib.pisa_hip_power_law(_ptr(energy), float(pivot), float(index), float(norm), _ptr(nominal), energy.numel(),
                                      _ptr(out), _stream()))
    return out


def shift_toward(x, target, fraction, clip=None, out=None):
    """x + (target - x) * fraction [clipped]; `target` a device column or a number (`pisa_hip_shift_toward`)"""
    lib = _lib.lib()
    if out is None:
        out = torch.empty_like(x)
    col = target if isinstance(target, torch.Tensor) else None
    _lib.check(lib.pisa_hip_shift_toward(_ptr(x), _ptr(col), 0.0 if col is not None else float(target), float(fraction),
                                         0 if clip is None else 1, 0.0 if clip is None else float(clip[0]),
                                         0.0 if clip is None else float(clip[1]), x.numel(), _ptr(out), _stream()))
    return out


def poly_scale(linear, quad, params, weights, scale=1.0):
    """weights *= max(0, scale * prod_k (1 + (lin_k + quad_k p_k) p_k)), in place (`pisa_hip_poly_scale`)"""
    lib = _lib.lib()
    k = len(linear)
    assert k == len(params) and (quad is None or len(quad) == k) and weights.is_contiguous()
    lin = (C.c_void_p * max(k, 1))(*[t.data_ptr() for t in linear])
    qd = None if quad is None else (C.c_void_p * max(k, 1))(*[None if t is None else t.data_ptr() for t in quad])
    p = (C.c_double * max(k, 1))(*[float(v) for v in params])
    for t in list(linear) + [t for t in (quad or []) if t is not None]:
        assert t.is_cuda and t.is_contiguous() and t.numel() == weights.numel()
    _lib.check(lib.pisa_hip_poly_scale(lin, qd, p, k, float(scale), weights.numel(), _ptr(weights), _stream()))
    return weights


def column_combination(columns, coef, n, mode="exp", out=None, dev=None):
    """f(sum_g coef_g * column_g) per event, f = exp / 1 + / identity (`pisa_hip_column_combination`)"""
    lib = _lib.lib()
    k = len(columns)
    assert k == len(coef)
    for t in columns:
        assert t.is_cuda and t.is_contiguous() and t.numel() == n and t.dtype == F8
    if out is None:
        out = torch.empty(n, dtype=F8, device=columns[0].device if k else (dev or device()))
    cols = (C.c_void_p * max(k, 1))(*[t.data_ptr() for t in columns])
    cf = (C.c_double * max(k, 1))(*[float(v) for v in coef])
    _lib.check(lib.pisa_hip_column_combination(cols, cf, k, {"exp": 0, "one_plus": 1, "sum": 2}[mode], n, _ptr(out), _stream()))
    return out


VECTOR_OPS = {"scale": 0, "mul": 1, "imul": 2, "imul_and_scale": 3, "itruediv": 4, "assign": 5, "pow": 6, "sqrt": 7,
              "replace_where_counts_gt": 8}


def vector_op(op, a, out, b=None, scalar=0.0):
    """the element-wise helpers of pisa/utils/vectorizer.py on device tensors, `out` written in place
    (`pisa_hip_vector_op`)"""
    lib = _lib.lib()
    assert out.is_contiguous() and a.numel() == out.numel() and (b is None or b.numel() == out.numel())
    _lib.check(lib.pisa_hip_vector_op(VECTOR_OPS[op], _ptr(a), _ptr(b), float(scalar), out.numel(), _ptr(out), _stream()))
    return out


def interp_linear(x_knots, y_knots, x, out=None):
    """numpy.interp(x, x_knots, y_knots) on the device; a value outside the knots raises, as scipy's interp1d does
    (`pisa_hip_interp_linear`)"""
    lib = _lib.lib()
    if out is None:
        out = torch.empty_like(x)
    status = torch.zeros(1, dtype=torch.int32, device=x.device)
    _lib.check(lib.pisa_hip_interp_linear(_ptr(x_knots), _ptr(y_knots), x_knots.numel(), _ptr(x), x.numel(), _ptr(out),
                                          _ptr(status), _stream()))
    if int(status.item()):
        raise ValueError("A value in x_new is outside the interpolation range.")
    return out


def decoherence_probs(coef, gamma, delta, two_flavor, energy, baseline, out=None):
    """P[n, 3, 3] of the vacuum decoherence model (`pisa_hip_decoherence_probs`)"""
    lib = _lib.lib()
    n = energy.numel()
    assert baseline.numel() == n
    if out is None:
        out = torch.empty((n, 3, 3), dtype=F8, device=energy.device)
    arr = [(C.c_double * 3)(*[float(v) for v in a]) for a in (coef, gamma, delta)]
    _lib.check(lib.pisa_hip_decoherence_probs(arr[0], arr[1], arr[2], 1 if two_flavor else 0, _ptr(energy), _ptr(baseline), n,
                                              _ptr(out), _stream()))
    return out


def bin_sqrt(x, out=None):
    lib = _lib.lib()
    if out is None:
        out = torch.empty_like(x)
    _lib.check(lib.pisa_hip_bin_sqrt(_ptr(x), x.numel(), _ptr(out), _stream()))
    return out


def flux_2d(table, true_energy, true_coszen, out_nu=None, out_nubar=None):
    """`calculate_2d_flux_weights` (flux_weights.py:267-349) for (nue, numu) and
    (nuebar, numubar) at once; `table` is a `pisa_amd.utils.flux_weights.FluxTable2D`."""
    lib = _lib.lib()
    n = true_energy.numel()
    dev = true_energy.device
    if out_nu is None:
        out_nu = torch.empty((n, 2), dtype=F8, device=dev)
    if out_nubar is None:
        out_nubar = torch.empty((n, 2), dtype=F8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.pisa_hip_flux_2d(C.byref(table.struct), _ptr(true_energy), _ptr(true_coszen), n,
                                    _ptr(out_nu), _ptr(out_nubar), _ptr(status), _stream()))
    if int(status.item()) != 0:
        raise ValueError("Not all coszens found between -1 and 1")  # flux_weights.py:318-319
    return out_nu, out_nubar


def barr_sets(columns):
    """argument block of `barr_simple_multi`: one (true_energy, true_coszen, nu_flux_nominal,
    nubar_flux_nominal, nubar, out) tuple of device tensors per container.  The block holds raw
    pointers: the caller keeps the tensors alive."""
    arr = (_lib.BarrSet * len(columns))()
    for d, (e, cz, nu, nub, nubar, out) in zip(arr, columns):
        d.n = e.numel()
        assert cz.numel() == d.n and nu.numel() == 2 * d.n and nub.numel() == 2 * d.n and out.numel() == 2 * d.n
        d.d_true_energy, d.d_true_coszen = _ptr(e), _ptr(cz)
        d.d_nu_flux_nominal, d.d_nubar_flux_nominal, d.d_out = _ptr(nu), _ptr(nub), _ptr(out)
        d.nubar = int(nubar)
    return arr


def barr_simple_multi(sets, nue_numu_ratio, nu_nubar_ratio, delta_index, Barr_uphor_ratio,
                      Barr_nu_nubar_ratio):
    """`apply_sys_vectorized` for every container of a pipeline in one launch (flux/barr_simple.py:83-104)."""
    _lib.check(_lib.lib().pisa_hip_barr_simple_multi(
        sets, len(sets), float(nue_numu_ratio), float(nu_nubar_ratio), float(delta_index),
        float(Barr_uphor_ratio), float(Barr_nu_nubar_ratio), _stream()))


def barr_simple(true_energy, true_coszen, nu_flux_nominal, nubar_flux_nominal, nubar,
                nue_numu_ratio, nu_nubar_ratio, delta_index, Barr_uphor_ratio,
                Barr_nu_nubar_ratio, out=None):
    """`apply_sys_vectorized` (flux/barr_simple.py:207-233)."""
    lib = _lib.lib()
    n = true_energy.numel()
    if out is None:
        out = torch.empty((n, 2), dtype=F8, device=true_energy.device)
    _lib.check(lib.pisa_hip_barr_simple(
        _ptr(true_energy), _ptr(true_coszen), _ptr(nu_flux_nominal), _ptr(nubar_flux_nominal),
        int(nubar), float(nue_numu_ratio), float(nu_nubar_ratio), float(delta_index),
        float(Barr_uphor_ratio), float(Barr_nu_nubar_ratio), n, _ptr(out), _stream()))
    return out
