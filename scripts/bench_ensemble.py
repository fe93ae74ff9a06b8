"""Time of the trial-ensemble kernels (`kernels.metric_matrix`, `kernels.metric_matrix_best`) and of one
`feldman_cousins`, one JSON line per measurement:

  * kernels, inputs resident, median of 20 launches (HIP events around each call: for the product form that is the
    preparation launch + the contraction), llh and poisson_llh in both forms, chi2 in the direct form, at
    (T, K, B) = (1e4, 1e2, 128) full matrix and reduced, (1e5, 1e3, 128) reduced only, (1e4, 1e3, 4800) full matrix
    and reduced; a form whose launch takes more than half a second is timed over 5 launches (`launches` says so).
    The product form's fraction of the fp64 peak counts 2 T K B flop (llh: 4 T K B, its two products);
  * the same work as a loop over `kernels.metric` on a 100 x 100 corner (all there was before these kernels);
  * the draw kernel alone (`kernels.poisson_fluctuate`), output resident, at (T, B) = (1e4, 128) and (1e4, 4800), with the
    draws per second and the share of the HBM bandwidth its 8 T B bytes of stores come to; then, in the same run, the four
    fluctuation methods through `kernels.fluctuate` (sigma = sqrt(0.3 mu)) with their ratio to that Poisson baseline;
  * end to end: `feldman_cousins` with T = 1e4 on a 30 x 30 grid of 128-bin templates, its wall time split into
    drawing, upload and kernels.  `--generator host` (the default) draws on the host, `device` on the device (no upload:
    the draws are made where the kernels read them), `both` runs the two alternately in this one process.  After a
    warm-up run the measurement is repeated `--e2e-reps` times: median wall time, every run's, and the split of the
    median run.  `--metric` and `--method` choose the metric and the fluctuation method of that run (defaults llh and
    poisson; any other choice gives the templates sumw2 = 0.3 mu);
  * `--mc` (alone: nothing else runs): the MC-uncertainty metrics correct_chi2, mcllh_mean, mcllh_eff and conv_llh, the
    reduced form at (T, K, B) = (1e4, 1e2, 128) with sigma2 = 0.3 mu, median of 5 launches (HIP events: the preparation
    launch + the pair kernel), and in the same run the only way there was before: a loop of `kernels.metric` over the
    pairs of a 64 x 16 sub-block (wall time, synchronised at its end), scaled to the full size by T K / 1024.

  * `--truth` (alone: nothing else runs): the pseudo-data with drawn nuisance truths and the covariance of the fitted
    displacements at (T, K, B, J) = (1e4, 1e2, 128, 8), median of 5 launches, HIP events: `pisa_hip_fluctuate_linear`
    (its two launches, the status not read) against `kernels.fluctuate` of the same run, poisson and gauss+poisson;
    `kernels.profiled_hesse` at the fitted eta_best / arg against `kernels.profiled_metric_matrix_best`, llh and chi2.

  * `--observed` (alone: nothing else runs): the pseudo-data at nuisances fitted to an observed map at (T, K, B, J) =
    (1e4, 1e2, 128, 8), median of 5 launches, HIP events: `pisa_hip_fluctuate_linear_mvn` (its two launches, truths
    N(0, cov) with sigma 0.5 and correlation 0.5 inside +-1.5, the status not read) against `pisa_hip_fluctuate_linear`
    and `kernels.fluctuate` of the same run, poisson and gauss+poisson; then one `feldman_cousins(generator="device")`
    with `nuisance="prior"`, "profiled" and "fitted" over the grid's points (wall time after a warm-up run).

  * `--posterior` (alone: nothing else runs): the nuisance-posterior sampler `kernels.posterior_sample` at K = 64
    points, W = 128 walkers, 128 bins, J = 4 parameters (llh, Gaussian priors, a box of +-1.5), 2000 steps of which
    every 10th is kept, median of 5 launches, HIP events; the time per half step, the log-density sweeps per second
    and the acceptance; then the same at W = 256 and at 4800 bins (rows streamed, not kept in LDS).

    python scripts/bench_ensemble.py [--reps 20] [--skip-e2e] [--skip-kernels] [--skip-draw] [--forms direct,product]
                                     [--true-points N] [--generator host|device|both] [--e2e-reps 3] [--mc] [--truth] [--observed] [--posterior]
                                     [--metric llh] [--method poisson]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_PEAK_TFLOPS = 78.6      # bench.py's FP64 peak: 256 CU x 4 SIMD x 16 lanes x 2 flop x 2.4 GHz (= the matrix cores' fp64 peak)


def _templates(n_k, n_bins, seed=0):
    rs = np.random.RandomState(seed)
    x = np.linspace(0.0, 1.0, n_bins)
    base = 100.0 * (1.0 + 0.5 * np.sin(5.0 * x)) + 5.0 * rs.rand(n_bins)
    a = np.linspace(-0.5, 0.5, n_k)[:, None]
    return base[None, :] * (1.0 + 0.1 * a * np.cos(3.0 * x)[None, :] + 0.05 * rs.rand(n_k, 1) * x[None, :])


def _time(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    if time.perf_counter() - t0 > 0.5:
        reps = min(reps, 5)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(float(np.min(ts)), 4), launches=reps)


def kernel_lines(reps, forms=("direct", "product")):
    import torch

    from pisa_amd import kernels as K

    dev = K.device()
    for (n_t, n_k, n_b), outputs in (((10 ** 4, 10 ** 2, 128), ("matrix", "reduced")),
                                     ((10 ** 5, 10 ** 3, 128), ("reduced",)),
                                     ((10 ** 4, 10 ** 3, 4800), ("matrix", "reduced"))):
        e_host = _templates(n_k, n_b)
        rs = np.random.RandomState(1)
        d = torch.from_numpy(rs.poisson(e_host[rs.randint(0, n_k, n_t)]).astype(np.float64)).to(dev)
        e = torch.from_numpy(e_host).to(dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        for kind in ("llh", "poisson_llh", "chi2"):
            for form in [f for f in forms if f == "direct" or kind != "chi2"]:
                for output in outputs:
                    if output == "matrix":
                        res = _time(lambda: K.metric_matrix(kind, d, e, form=form, status=status), reps)
                    else:
                        res = _time(lambda: K.metric_matrix_best(kind, d, e, k0=n_k // 2, form=form, status=status), reps)
                    line = dict(workload="kernel", T=n_t, K=n_k, B=n_b, kind=kind, form=form, output=output, **res)
                    if form == "product":
                        flop = (4.0 if kind == "llh" else 2.0) * n_t * n_k * n_b
                        line["tflops"] = round(flop / (res["ms_median"] * 1e-3) / 1e12, 3)
                        line["frac_of_fp64_peak"] = round(line["tflops"] / FP64_PEAK_TFLOPS, 4)
                    print(json.dumps(line), flush=True)
        assert int(status.item()) == 0
        if n_t == 10 ** 4 and n_k == 10 ** 2 and "direct" in forms:
            total = torch.empty(1, dtype=torch.float64, device=dev)
            for kind in ("llh", "poisson_llh", "chi2"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for t in range(100):
                    for k in range(100):
                        K.metric(kind, d[t], e[k], total_out=total, status=status)
                torch.cuda.synchronize()
                print(json.dumps(dict(workload="loop_over_kernels_metric", T=100, K=100, B=n_b, kind=kind,
                                      ms=round(1e3 * (time.perf_counter() - t0), 3), launches=10 ** 4)), flush=True)
        del d, e


def profiled_lines(n_params, reps, bounded=None):
    """`profiled_metric_matrix_best` with J = n_params fitted nuisance displacements per pair, every kind, against the
    unprofiled direct reduced form of the same run; iteration counts from the full output on the first trials.
    `bounded` = H: the bounded reduced form (every eta_j inside -H ... +H prior sigmas) is timed in the same run, with
    its own iteration counts, the share of the head's pairs that end with a coordinate on a bound and the time per
    sweep of both forms (ms / (mean Newton steps + 2): the sweeps of the fit and the one of the value).
    Executed flops: per bin of a sweep 2 J (mu) + 2 J (its reach) + 2 J (gradient) + J + J (J + 1) (Hessian) + 20 (the
    terms of phi, a transcendental counted as one), sweeps = Newton steps + 1 (halved steps not counted), + one sweep
    of 2 J + 10 for the value."""
    import torch

    from pisa_amd import kernels as K

    dev = K.device()
    J = int(n_params)
    for n_t, n_k, n_b in ((10 ** 4, 10 ** 2, 128), (10 ** 5, 10 ** 3, 128)):
        e_host = _templates(n_k, n_b)
        rs = np.random.RandomState(1)
        x = (np.arange(n_b) + 0.5) / n_b
        r_host = 0.05 * np.cos((np.arange(J)[:, None] + 1) * np.pi * x[None, :])[None] * e_host[:, None, :]
        mu = e_host + np.einsum("kjb,kj->kb", r_host, 0.5 * rs.randn(n_k, J))
        d = torch.from_numpy(rs.poisson(np.maximum(mu, 1.0)[rs.randint(0, n_k, n_t)]).astype(np.float64)).to(dev)
        e, r = torch.from_numpy(e_host).to(dev), torch.from_numpy(r_host).to(dev)
        s2 = 0.1 * e
        ips = torch.ones(J, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        n_head = min(n_t, 256 * 10 ** 2 // n_k * 8)
        for kind in ("llh", "poisson_llh", "chi2", "mod_chi2"):
            sig = s2 if kind == "mod_chi2" else None
            head = K.profiled_metric_matrix(kind, d[:n_head], e, r, sig, ips, want_eta=False, status=status)
            it = head["n_iter"].double()
            flagged = int((head["status"] != 0).sum().item())
            plain = _time(lambda: K.metric_matrix_best(kind, d, e, sig, k0=n_k // 2, form="direct", status=status), reps)
            res = _time(lambda: K.profiled_metric_matrix_best(kind, d, e, r, sig, ips, k0=n_k // 2, status=status), reps)
            per_bin = 2 * J + 2 * J + 2 * J + J + J * (J + 1) + 20
            flop = float(n_t) * n_k * n_b * ((float(it.mean().item()) + 1.0) * per_bin + 2 * J + 10)
            tflops = flop / (res["ms_median"] * 1e-3) / 1e12
            print(json.dumps(dict(workload="profiled_kernel", T=n_t, K=n_k, B=n_b, J=J, kind=kind, output="reduced", **res,
                                  ms_unprofiled_direct=plain["ms_median"],
                                  ratio_to_unprofiled=round(res["ms_median"] / plain["ms_median"], 2),
                                  iter_mean=round(float(it.mean().item()), 3), iter_max=int(it.max().item()),
                                  flagged_of_head=flagged, head_pairs=int(it.numel()), tflops=round(tflops, 3),
                                  frac_of_fp64_vector_peak=round(tflops / FP64_PEAK_TFLOPS, 4))), flush=True)
            if bounded is not None:
                hi = float(bounded) / ips
                lo = -hi
                head_b = K.profiled_metric_matrix(kind, d[:n_head], e, r, sig, ips, status=status, lower=lo, upper=hi)
                it_b = head_b["n_iter"].double()
                on = ((head_b["eta"] == lo) | (head_b["eta"] == hi)).any(dim=2)
                res_b = _time(lambda: K.profiled_metric_matrix_best(kind, d, e, r, sig, ips, k0=n_k // 2, status=status,
                                                                    lower=lo, upper=hi), reps)
                sweeps, sweeps_b = float(it.mean().item()) + 2.0, float(it_b.mean().item()) + 2.0
                print(json.dumps(dict(workload="profiled_kernel_bounded", T=n_t, K=n_k, B=n_b, J=J, kind=kind,
                                      output="reduced", half_width_sigmas=float(bounded), **res_b,
                                      ms_unbounded=res["ms_median"],
                                      ratio_to_unbounded=round(res_b["ms_median"] / res["ms_median"], 3),
                                      iter_mean=round(float(it_b.mean().item()), 3), iter_max=int(it_b.max().item()),
                                      flagged_of_head=int((head_b["status"] != 0).sum().item()),
                                      on_bound_of_head=round(float(on.double().mean().item()), 4),
                                      ms_per_sweep=round(res_b["ms_median"] / sweeps_b, 3),
                                      ms_per_sweep_unbounded=round(res["ms_median"] / sweeps, 3))), flush=True)
        assert int(status.item()) == 0
        del d, e, r


def profiled_wide_lines(n_params, reps, form="linear"):
    """the protocol of `profiled_lines` with the wide form (`profiled_metric_matrix_best_wide`, one wavefront per pair,
    J up to 32) at (T, K, B) = (1e4, 1e2, 128); iteration counts from the wide full output on the first trials.  With
    J <= 8 the narrow form is timed in the same run: the price of the mapping.
    form="loglinear": the log-linear response rho = 0.05 x cosines (the same shapes without the factor E), the data
    drawn at E exp(rho . eta0); the linear wide form is timed in the same run on the same data with the response rho E,
    and both times go into the line with their ratio."""
    if form == "loglinear":
        return profiled_loglinear_lines(n_params, reps)
    import torch

    from pisa_amd import kernels as K

    dev = K.device()
    J = int(n_params)
    n_t, n_k, n_b = 10 ** 4, 10 ** 2, 128
    e_host = _templates(n_k, n_b)
    rs = np.random.RandomState(1)
    x = (np.arange(n_b) + 0.5) / n_b
    r_host = 0.05 * np.cos((np.arange(J)[:, None] + 1) * np.pi * x[None, :])[None] * e_host[:, None, :]
    mu = e_host + np.einsum("kjb,kj->kb", r_host, 0.5 * rs.randn(n_k, J))
    d = torch.from_numpy(rs.poisson(np.maximum(mu, 1.0)[rs.randint(0, n_k, n_t)]).astype(np.float64)).to(dev)
    e, r = torch.from_numpy(e_host).to(dev), torch.from_numpy(r_host).to(dev)
    s2 = 0.1 * e
    ips = torch.ones(J, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    n_head = 256
    for kind in ("llh", "poisson_llh", "chi2", "mod_chi2"):
        sig = s2 if kind == "mod_chi2" else None
        head = K.profiled_metric_matrix_wide(kind, d[:n_head], e, r, sig, ips, want_eta=False, status=status)
        it = head["n_iter"].double()
        res = _time(lambda: K.profiled_metric_matrix_best_wide(kind, d, e, r, sig, ips, k0=n_k // 2, status=status), reps)
        line = dict(workload="profiled_kernel_wide", T=n_t, K=n_k, B=n_b, J=J, kind=kind, output="reduced", **res,
                    iter_mean=round(float(it.mean().item()), 3), iter_max=int(it.max().item()),
                    flagged_of_head=int((head["status"] != 0).sum().item()), head_pairs=int(it.numel()),
                    ms_per_sweep=round(res["ms_median"] / (float(it.mean().item()) + 2.0), 3))
        if J <= 8:
            narrow = _time(lambda: K.profiled_metric_matrix_best(kind, d, e, r, sig, ips, k0=n_k // 2, status=status), reps)
            line.update(ms_narrow=narrow["ms_median"], ratio_to_narrow=round(res["ms_median"] / narrow["ms_median"], 2))
        print(json.dumps(line), flush=True)
    assert int(status.item()) == 0


def profiled_loglinear_lines(n_params, reps):
    """`profiled_wide_lines` for the log-linear response (`profiled_metric_matrix_best_wide(..., form="loglinear")`):
    unit priors, reduced output, and the linear wide form in the same run"""
    import torch

    from pisa_amd import kernels as K

    dev = K.device()
    J = int(n_params)
    n_t, n_k, n_b = 10 ** 4, 10 ** 2, 128
    e_host = _templates(n_k, n_b)
    rs = np.random.RandomState(1)
    x = (np.arange(n_b) + 0.5) / n_b
    rho_host = np.ascontiguousarray(np.broadcast_to(
        0.05 * np.cos((np.arange(J)[:, None] + 1) * np.pi * x[None, :])[None], (n_k, J, n_b)))
    mu = e_host * np.exp(np.einsum("kjb,kj->kb", rho_host, 0.5 * rs.randn(n_k, J)))
    d = torch.from_numpy(rs.poisson(np.maximum(mu, 1.0)[rs.randint(0, n_k, n_t)]).astype(np.float64)).to(dev)
    e, rho = torch.from_numpy(e_host).to(dev), torch.from_numpy(rho_host).to(dev)
    r = torch.from_numpy(rho_host * e_host[:, None, :]).to(dev)
    s2 = 0.1 * e
    ips = torch.ones(J, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    n_head = 256
    for kind in ("llh", "poisson_llh", "chi2", "mod_chi2"):
        sig = s2 if kind == "mod_chi2" else None
        line = dict(workload="profiled_kernel_loglinear", T=n_t, K=n_k, B=n_b, J=J, kind=kind, output="reduced")
        for name, resp in (("loglinear", rho), ("linear", r)):
            head = K.profiled_metric_matrix_wide(kind, d[:n_head], e, resp, sig, ips, want_eta=False, status=status,
                                                 form=name)
            it = head["n_iter"].double()
            res = _time(lambda: K.profiled_metric_matrix_best_wide(kind, d, e, resp, sig, ips, k0=n_k // 2,
                                                                   status=status, form=name), reps)
            tag = "" if name == "loglinear" else "_linear"
            line.update({"ms_median" + tag: res["ms_median"], "ms_min" + tag: res["ms_min"],
                         "iter_mean" + tag: round(float(it.mean().item()), 3), "iter_max" + tag: int(it.max().item()),
                         "flagged_of_head" + tag: int((head["status"] != 0).sum().item()),
                         "ms_per_sweep" + tag: round(res["ms_median"] / (float(it.mean().item()) + 2.0), 3)})
        line.update(head_pairs=n_head * n_k, reps=reps,
                    ratio_to_linear=round(line["ms_median"] / line["ms_median_linear"], 3),
                    ratio_per_sweep=round(line["ms_per_sweep"] / line["ms_per_sweep_linear"], 3))
        print(json.dumps(line), flush=True)
    assert int(status.item()) == 0


def truth_lines(reps=5):
    """one line per method for `fluctuate_linear` against `fluctuate`, one per kind for `profiled_hesse` against
    `profiled_metric_matrix_best`, at (T, K, B, J) = (1e4, 1e2, 128, 8); the inputs of `profiled_lines`"""
    import torch

    from pisa_amd import _lib
    from pisa_amd import kernels as K

    dev = K.device()
    n_t, n_k, n_b, J = 10 ** 4, 10 ** 2, 128, 8
    e_host = _templates(n_k, n_b)
    rs = np.random.RandomState(1)
    x = (np.arange(n_b) + 0.5) / n_b
    r_host = 0.05 * np.cos((np.arange(J)[:, None] + 1) * np.pi * x[None, :])[None] * e_host[:, None, :]
    e, r = torch.from_numpy(e_host).to(dev), torch.from_numpy(r_host).to(dev)
    k0 = n_k // 2
    mu, sigma, resp = e[k0].contiguous(), torch.sqrt(0.3 * e[k0]).contiguous(), r[k0].contiguous()
    scale, shift = np.full(J, 0.5), np.zeros(J)
    lower, upper = np.full(J, -1.5), np.full(J, 1.5)
    out = torch.empty((n_t, n_b), dtype=torch.float64, device=dev)
    eta = torch.empty((n_t, J), dtype=torch.float64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    lib = _lib.lib()
    for method in ("poisson", "gauss+poisson"):
        sg = None if method == "poisson" else sigma
        code = K.FLUCTUATE_METHOD[method]

        def linear():
            _lib.check(lib.pisa_hip_fluctuate_linear(
                mu.data_ptr(), None if sg is None else sg.data_ptr(), resp.data_ptr(), J, scale.ctypes.data,
                shift.ctypes.data, lower.ctypes.data, upper.ctypes.data, code, n_b, n_t, 1, k0, 0, out.data_ptr(),
                eta.data_ptr(), status.data_ptr(), None))

        base = _time(lambda: K.fluctuate(mu, n_t, 1, method=method, sigma=sg, stream=k0, out=out, status=status[:1]), reps)
        res = _time(linear, reps)
        print(json.dumps(dict(workload="fluctuate_linear", T=n_t, B=n_b, J=J, method=method, **res,
                              ms_fluctuate=base["ms_median"], ratio_to_fluctuate=round(res["ms_median"] / base["ms_median"], 3),
                              clipped=int(status[1].item()))), flush=True)
        assert int(status[0].item()) == 0
        status.zero_()
    drawn = K.fluctuate_linear(mu, resp, n_t, 1, scale, shift, lower, upper, stream=k0)
    ips = torch.ones(J, dtype=torch.float64, device=dev)
    for kind in ("llh", "chi2"):
        fit = K.profiled_metric_matrix_best(kind, drawn["data"], e, r, None, ips, k0=k0)
        base = _time(lambda: K.profiled_metric_matrix_best(kind, drawn["data"], e, r, None, ips, k0=k0, status=status[:1]),
                     reps)
        res = _time(lambda: K.profiled_hesse(kind, drawn["data"], e, r, fit["eta_best"], fit["arg"], None, ips), reps)
        h = K.profiled_hesse(kind, drawn["data"], e, r, fit["eta_best"], fit["arg"], None, ips)
        print(json.dumps(dict(workload="profiled_hesse", T=n_t, K=n_k, B=n_b, J=J, kind=kind, **res,
                              ms_profiled_best=base["ms_median"],
                              ratio_to_profiled_best=round(res["ms_median"] / base["ms_median"], 5),
                              flagged=int((h["status"] != 0).sum().item()))), flush=True)


def observed_lines(reps=5):
    """one line per method for `pisa_hip_fluctuate_linear_mvn` against `pisa_hip_fluctuate_linear` (and `fluctuate`) of
    the same run at (T, K, B, J) = (1e4, 1e2, 128, 8), then one `feldman_cousins(nuisance="fitted")` over the grid
    against `nuisance="prior"` and "profiled" (wall time, synchronised, after a warm-up run with few trials); the inputs
    of `truth_lines`"""
    import torch

    from pisa_amd import _lib
    from pisa_amd import kernels as K
    from pisa_amd.analysis import ensemble as en

    dev = K.device()
    n_t, n_k, n_b, J = 10 ** 4, 10 ** 2, 128, 8
    e_host = _templates(n_k, n_b)
    x = (np.arange(n_b) + 0.5) / n_b
    r_host = 0.05 * np.cos((np.arange(J)[:, None] + 1) * np.pi * x[None, :])[None] * e_host[:, None, :]
    e, r = torch.from_numpy(e_host).to(dev), torch.from_numpy(r_host).to(dev)
    k0 = n_k // 2
    mu, sigma, resp = e[k0].contiguous(), torch.sqrt(0.3 * e[k0]).contiguous(), r[k0].contiguous()
    scale, shift = np.full(J, 0.5), np.zeros(J)
    lower, upper = np.full(J, -1.5), np.full(J, 1.5)
    cov = np.ascontiguousarray(0.25 * (0.5 * np.ones((J, J)) + 0.5 * np.eye(J)))      # sigma 0.5, correlation 0.5
    out = torch.empty((n_t, n_b), dtype=torch.float64, device=dev)
    eta = torch.empty((n_t, J), dtype=torch.float64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    lib = _lib.lib()
    for method in ("poisson", "gauss+poisson"):
        sg = None if method == "poisson" else sigma
        code = K.FLUCTUATE_METHOD[method]

        def call(entry, first, second):          # (scale, shift) of the one entry point, (mean, cov) of the other
            _lib.check(entry(mu.data_ptr(), None if sg is None else sg.data_ptr(), resp.data_ptr(), J,
                             first.ctypes.data, second.ctypes.data, lower.ctypes.data,
                             upper.ctypes.data, code, n_b, n_t, 1, k0, 0, out.data_ptr(), eta.data_ptr(),
                             status.data_ptr(), None))

        base = _time(lambda: K.fluctuate(mu, n_t, 1, method=method, sigma=sg, stream=k0, out=out, status=status[:1]), reps)
        lin = _time(lambda: call(lib.pisa_hip_fluctuate_linear, scale, shift), reps)
        res = _time(lambda: call(lib.pisa_hip_fluctuate_linear_mvn, shift, cov), reps)
        print(json.dumps(dict(workload="fluctuate_linear_mvn", T=n_t, B=n_b, J=J, method=method, **res,
                              ms_fluctuate_linear=lin["ms_median"], ms_fluctuate=base["ms_median"],
                              ratio_to_fluctuate_linear=round(res["ms_median"] / lin["ms_median"], 3),
                              ratio_to_fluctuate=round(res["ms_median"] / base["ms_median"], 3),
                              clipped=int(status[1].item()))), flush=True)
        assert int(status[0].item()) == 0
        status.zero_()
    # end to end: the priors N(0, 0.5) of the lines above, the observed map one draw of point k0 at displaced truths
    grid = en.TemplateGrid(e, None, np.zeros((n_k, 1)), None, None, "llh")
    response = en.NuisanceResponse(["p%d" % j for j in range(J)], r, np.full(J, 2.0), np.zeros((n_k, J)), np.zeros(n_k),
                                   np.zeros((n_k, J)), lower=lower, upper=upper)
    observed = K.fluctuate_linear(mu, resp, 1, 7, np.zeros(J), 0.3 * np.cos(np.arange(J)), stream=k0)["data"]
    fit = en.fit_observed(observed, grid, "llh", response, covariance=True)
    good = [k for k in range(n_k) if not (int(fit["status"][k]) & ~32) and not np.isnan(fit["cov"][k]).any()]
    wall = {}
    for nuisance in ("prior", "profiled", "fitted"):
        kw = dict(generator="device", response=response, nuisance=nuisance, true_points=good)
        if nuisance != "prior":
            kw["observed"] = observed
        en.feldman_cousins(grid, "llh", 64, random_state=1, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        crit, info = en.feldman_cousins(grid, "llh", n_t, random_state=1, **kw)
        torch.cuda.synchronize()
        wall[nuisance] = time.perf_counter() - t0
        print(json.dumps(dict(workload="feldman_cousins_nuisance", nuisance=nuisance, T=n_t, K=n_k, B=n_b, J=J,
                              true_points=len(good), wall_s=round(wall[nuisance], 3),
                              ratio_to_prior=round(wall[nuisance] / wall["prior"], 3),
                              flagged=int(info["flagged"].sum()), crit_68_mean=round(float(crit[:, 0].mean()), 4))),
              flush=True)


def posterior_lines(reps=5):
    """one line per shape for `kernels.posterior_sample` (module docstring)"""
    import torch

    from pisa_amd import kernels as K

    dev = K.device()
    n_k, n_j, n_steps, thin = 64, 4, 2000, 10
    for n_w, n_bins in ((128, 128), (256, 128), (128, 4800)):
        E = _templates(n_k, n_bins)
        x = np.linspace(0.0, 1.0, n_bins)
        R = 0.1 * np.cos((np.arange(n_j)[None, :, None] + 1) * np.pi * x[None, None, :]) * E[:, None, :]
        rs = np.random.RandomState(3)
        D = rs.poisson(E[0]).astype(np.float64)[None, :]
        x0 = 0.05 * rs.randn(n_k, n_w, n_j)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)       # noqa: E731
        args = ("llh", up(D), up(E), up(R), up(x0), n_steps, 7)
        kw = dict(inv_prior_sigma=up(np.full(n_j, 2.0)), lower=up(np.full(n_j, -1.5)), upper=up(np.full(n_j, 1.5)),
                  thin=thin, keep_from=thin - 1)
        out = K.posterior_sample(*args, **kw)
        assert not bool(out["status"].any())
        t = _time(lambda: K.posterior_sample(*args, **kw), reps)
        sweeps = n_k * n_w * n_steps
        print(json.dumps(dict(kernel="posterior_sample", kind="llh", points=n_k, walkers=n_w, bins=n_bins, params=n_j,
                              steps=n_steps, thin=thin, staged_in_lds=bool(n_bins <= K.posterior_layout("llh", n_j, n_w)[
                                  "stage_bins"]), us_per_half_step=round(1e3 * t["ms_median"] / (2 * n_steps), 3),
                              sweeps_per_s=round(sweeps / (1e-3 * t["ms_median"]), 1),
                              ns_per_bin_and_sweep_of_a_wavefront=round(
                                  1e6 * t["ms_median"] / (2 * n_steps * n_bins), 2),
                              acceptance=round(float(out["accepted"].sum().item()) / sweeps, 3), **t)), flush=True)


def mc_lines(reps=5):
    import torch

    from pisa_amd import kernels as K

    dev = K.device()
    n_t, n_k, n_b = 10 ** 4, 10 ** 2, 128
    sub_t, sub_k = 64, 16
    e_host = _templates(n_k, n_b)
    rs = np.random.RandomState(1)
    d = torch.from_numpy(rs.poisson(e_host[rs.randint(0, n_k, n_t)]).astype(np.float64)).to(dev)
    e = torch.from_numpy(e_host).to(dev)
    s2 = 0.3 * e
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    for kind in K.ENSEMBLE_MC_KINDS:
        res = _time(lambda: K.metric_matrix_best(kind, d, e, s2, k0=n_k // 2, status=status), reps)
        full = _time(lambda: K.metric_matrix(kind, d, e, s2, status=status), reps)
        K.metric(kind, d[0], e[0], s2[0], total_out=total, status=status)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(sub_t):
            for k in range(sub_k):
                K.metric(kind, d[t], e[k], s2[k], total_out=total, status=status)
        torch.cuda.synchronize()
        loop_ms = 1e3 * (time.perf_counter() - t0)
        scaled = loop_ms * (n_t * n_k) / (sub_t * sub_k)
        print(json.dumps(dict(workload="mc_kernel", T=n_t, K=n_k, B=n_b, kind=kind, output="reduced", **res,
                              ms_matrix_median=full["ms_median"], loop_pairs=sub_t * sub_k, loop_ms=round(loop_ms, 3),
                              loop_ms_scaled_to_full=round(scaled, 1),
                              ratio_loop_to_reduced=round(scaled / res["ms_median"], 1))), flush=True)
    assert int(status.item()) == 0


HBM_PEAK_TBS = 8.0           # MI355X: 8 TB/s


def draw_lines(reps):
    """the draw kernel alone: means of the end-to-end templates (50 - 150 counts per bin: the rejection sampler)"""
    import torch

    from pisa_amd import kernels as K

    dev = K.device()
    for n_t, n_b in ((10 ** 4, 128), (10 ** 4, 4800)):
        mu = torch.from_numpy(_templates(1, n_b, seed=3)[0]).to(dev)
        out = torch.empty((n_t, n_b), dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        res = _time(lambda: K.poisson_fluctuate(mu, n_t, 1, stream=7, out=out, status=status), reps)
        assert int(status.item()) == 0
        sec = res["ms_median"] * 1e-3
        print(json.dumps(dict(workload="draw_kernel", T=n_t, B=n_b, mean_of_mu=round(float(mu.mean().item()), 2), **res,
                              gdraws_per_s=round(n_t * n_b / sec / 1e9, 3),
                              frac_of_hbm_peak=round(8.0 * n_t * n_b / sec / 1e12 / HBM_PEAK_TBS, 4))), flush=True)
        sigma = torch.sqrt(0.3 * mu)
        for method in K.FLUCTUATE_METHOD:
            m = _time(lambda: K.fluctuate(mu, n_t, 1, method=method, sigma=sigma, stream=7, out=out, status=status), reps)
            assert int(status.item()) == 0
            print(json.dumps(dict(workload="fluctuate_kernel", method=method, T=n_t, B=n_b, **m,
                                  ratio_to_poisson_entry_point=round(m["ms_median"] / res["ms_median"], 3),
                                  gdraws_per_s=round(n_t * n_b / (m["ms_median"] * 1e-3) / 1e9, 3))), flush=True)


class _TimedSolver:
    """`DeviceSolver` with a synchronise after the upload, after the launches and after a draw on the device: their wall
    times, summed"""

    def __init__(self, solver, timings):
        self.solver, self.timings = solver, timings

    def draw(self, mu, n_trials, seed, stream, first_trial=0):
        import torch

        t0 = time.perf_counter()
        out = self.solver.draw(mu, n_trials, seed, stream, first_trial)
        torch.cuda.synchronize()
        self.timings["draw"] = self.timings.get("draw", 0.0) + (time.perf_counter() - t0)
        return out

    def fluctuate(self, mu, sigma, method, n_trials, seed, stream, first_trial=0):
        import torch

        t0 = time.perf_counter()
        out = self.solver.fluctuate(mu, sigma, method, n_trials, seed, stream, first_trial)
        torch.cuda.synchronize()
        self.timings["draw"] = self.timings.get("draw", 0.0) + (time.perf_counter() - t0)
        return out

    def best(self, kind, data, expected, sigma2=None, offset=None, k0=0):
        import torch

        t0 = time.perf_counter()
        dev = [self.solver._up(a) for a in (data, expected, sigma2, offset)]
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = self.solver.best(kind, *dev, k0=k0)
        torch.cuda.synchronize()
        self.timings["upload"] = self.timings.get("upload", 0.0) + (t1 - t0)
        self.timings["kernels"] = self.timings.get("kernels", 0.0) + (time.perf_counter() - t1)
        return out


def _e2e_once(en, grid, n_trials, points, generator, metric="llh", method="poisson"):
    """one timed `feldman_cousins` -> (wall, timings, crit)"""
    import torch

    timings = {"draw": 0.0, "upload": 0.0, "kernels": 0.0}
    draw = en.pseudo_data

    def timed_draw(*a, **k):
        t0 = time.perf_counter()
        out = draw(*a, **k)
        timings["draw"] += time.perf_counter() - t0
        return out

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    en.pseudo_data = timed_draw
    try:
        crit = en.feldman_cousins(grid, metric, n_trials, random_state=1, true_points=points,
                                  solver=_TimedSolver(en.DeviceSolver(), timings), generator=generator, method=method)
    finally:
        en.pseudo_data = draw
    torch.cuda.synchronize()
    return time.perf_counter() - t0, timings, crit


def e2e_lines(n_trials, true_points, generator, reps, metric="llh", method="poisson"):
    from pisa_amd import kernels as K
    from pisa_amd.analysis import ensemble as en

    side, n_b = 30, 128
    hist = _templates(side * side, n_b, seed=3)
    sumw2 = (0.0 if (metric, method) == ("llh", "poisson") else 0.3) * hist
    grid = en.TemplateGrid(K.to_device(hist), K.to_device(sumw2), np.zeros((side * side, 2)), None, None, metric)
    grid._host["hist"], grid._host["sumw2"] = hist, sumw2
    points = None if true_points is None else list(range(0, side * side, max(1, side * side // true_points)))[:true_points]
    generators = ("host", "device") if generator == "both" else (generator,)
    warm = points[:2] if points is not None else [0, 1]
    for g in generators:                   # (first launches, allocator, scipy's first call: the timed shape, two points)
        en.feldman_cousins(grid, metric, n_trials, random_state=1, true_points=warm, generator=g, method=method)
    runs = {g: [] for g in generators}
    for _ in range(reps):                  # the generators alternate: what else the machine does meets both alike
        for g in generators:
            runs[g].append(_e2e_once(en, grid, n_trials, points, g, metric, method))
    for g in generators:
        walls = [r[0] for r in runs[g]]
        wall, timings, crit = sorted(runs[g], key=lambda r: r[0])[len(walls) // 2]
        print(json.dumps(dict(workload="feldman_cousins", generator=g, grid="%dx%d" % (side, side), B=n_b, T=n_trials,
                              metric=metric, method=method, true_points=crit.shape[0], runs=len(walls), wall_s=round(wall, 3),
                              wall_s_all=[round(w, 3) for w in walls], draw_s=round(timings["draw"], 3),
                              upload_s=round(timings["upload"], 3), kernels_s=round(timings["kernels"], 3),
                              other_s=round(wall - timings["draw"] - timings["upload"] - timings["kernels"], 3),
                              crit90_mean=round(float(crit[:, 1].mean()), 6),
                              crit90_first=[round(float(c), 6) for c in crit[:4, 1]])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=float, default=1e4)
    ap.add_argument("--true-points", type=int, default=None, help="only this many true points of the 900 (default: all)")
    ap.add_argument("--forms", default="direct,product", help="the kernel forms to time")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-draw", action="store_true")
    ap.add_argument("--generator", choices=("host", "device", "both"), default="host",
                    help="who draws the pseudo-data of the end-to-end run")
    ap.add_argument("--e2e-reps", type=int, default=3, help="timed end-to-end runs per generator (median)")
    ap.add_argument("--metric", default="llh", help="the metric of the end-to-end run")
    ap.add_argument("--method", default="poisson", help="the fluctuation method of the end-to-end run")
    ap.add_argument("--profiled", type=int, default=0, metavar="J",
                    help="also time the profiled reduced form with J fitted nuisance parameters (1 to 8; with --wide: "
                         "1 to 32)")
    ap.add_argument("--wide", action="store_true",
                    help="with --profiled: time the wide form (one wavefront per pair) at (1e4, 1e2, 128), and for "
                         "J <= 8 the narrow form beside it")
    ap.add_argument("--form", choices=("linear", "loglinear"), default="linear",
                    help="with --profiled J --wide: the form of the response; loglinear times the log-linear kernels "
                         "and the linear wide form in the same run")
    ap.add_argument("--bounded", type=float, default=None, metavar="H",
                    help="with --profiled: also time the bounded reduced form, every displacement inside -H ... +H "
                         "prior sigmas")
    ap.add_argument("--mc", action="store_true",
                    help="time the MC-uncertainty metrics against the loop over kernels.metric, and nothing else")
    ap.add_argument("--truth", action="store_true",
                    help="time fluctuate_linear against fluctuate and profiled_hesse against profiled_metric_matrix_best, "
                         "and nothing else")
    ap.add_argument("--observed", action="store_true",
                    help="time fluctuate_linear_mvn against fluctuate_linear and feldman_cousins(nuisance='fitted') "
                         "against nuisance='prior', and nothing else")
    ap.add_argument("--posterior", action="store_true",
                    help="time the nuisance-posterior sampler (kernels.posterior_sample), and nothing else")
    args = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    if args.posterior:
        posterior_lines()
        return
    if args.mc:
        mc_lines()
        return
    if args.truth:
        truth_lines()
        return
    if args.observed:
        observed_lines()
        return
    if not args.skip_kernels:
        kernel_lines(args.reps, tuple(args.forms.split(",")))
    if args.profiled and args.wide:
        profiled_wide_lines(args.profiled, args.reps, args.form)
    elif args.profiled:
        profiled_lines(args.profiled, args.reps, args.bounded)
    if not args.skip_draw:
        draw_lines(args.reps)
    if not args.skip_e2e:
        e2e_lines(int(args.trials), args.true_points, args.generator, args.e2e_reps, args.metric, args.method)


if __name__ == "__main__":
    main()
