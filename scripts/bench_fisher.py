"""Time of one Fisher matrix (`HotPathEngine.fisher_many`, `get_fisher_matrix`), one JSON line per workload:

  * the headline synthetic workload (1e7 events, 12 containers, dragon 8x8x2 bins, 200x100 calc grid) at
    P = 2, 4 and 7 (2P + 1 points): the one-sweep path against the point-by-point path (the same engine with
    `sweep_capable` forced false), median and minimum ms per matrix;
  * settings/pipeline/example_hip.cfg through `get_fisher_matrix` with free theta23, deltam31, aeff_scale: the
    sweep path, and the fallback (the one-sweep path declining: one get_outputs per point).

    python scripts/bench_fisher.py [--events 1e7] [--reps 20] [--skip-cfg]
    rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/bench_fisher.py --kernel-only   (the kernel's own time)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _sync():
    import torch

    torch.cuda.synchronize()


def _stats(ts):
    return dict(ms_median=round(1e3 * float(np.median(ts)), 4), ms_min=round(1e3 * float(np.min(ts)), 4))


def synthetic_lines(n_events, reps):
    from pisa_amd import synthetic

    wl = synthetic.Workload(n_events=int(n_events), grid=(200, 100), out_binning="dragon", seed=0)
    st = synthetic.DeviceState(wl, compact=True)
    for n_par in (2, 4, 7):
        pts, pairs, dx = [wl.osc_params()], [], []
        for p in range(n_par):
            th = 42.0 + 0.3 * p
            pts += [wl.osc_params(theta23_deg=th + 0.5, dm31=2.45e-3 + 1e-6 * p),
                    wl.osc_params(theta23_deg=th - 0.5, dm31=2.46e-3 - 1e-6 * p)]
            pairs.append((2 + 2 * p, 1 + 2 * p))
            dx.append(1.0)
        out = dict(workload="synthetic_headline", events=wl.n_events, n_bins=wl.n_bins, P=n_par, points=len(pts))
        for path in ("sweep", "point_by_point"):
            if path == "point_by_point":
                st.sweep_capable = lambda plan=None: False
            try:
                ts = []
                for i in range(reps + 3):
                    _sync()
                    t0 = time.perf_counter()
                    res = st.fisher_many(pts, pairs, dx)
                    _sync()
                    if i >= 3:
                        ts.append(time.perf_counter() - t0)
                out[path] = dict(_stats(ts), sweeps=res["sweeps"])
                out[path + "_matrix00"] = float(res["matrix"][0, 0])
            finally:
                st.__dict__.pop("sweep_capable", None)
        out["speedup_median"] = round(out["point_by_point"]["ms_median"] / out["sweep"]["ms_median"], 3)
        print(json.dumps(out), flush=True)


def cfg_line(reps):
    from pisa_amd.core.distribution_maker import DistributionMaker
    from pisa_amd.core.fastplan import FastPlan
    from pisa_amd.utils.fisher_matrix import get_fisher_matrix

    dm = DistributionMaker("settings/pipeline/example_hip.cfg")
    for name in dm.params.free.names:
        if name not in ("theta23", "deltam31", "aeff_scale"):
            dm.params.fix(name)
    dm.get_outputs(return_sum=True)
    start = {p.name: p.value for p in dm.params.free}
    tv = {n: [v * 1.01, v * 0.99] for n, v in start.items()}
    out = dict(workload="example_hip.cfg", P=len(start))
    maps_many = FastPlan.maps_many      # the fallback: the one-sweep path declines, one get_outputs per point
    for path in ("sweep", "fallback"):
        ts = []
        for i in range(reps + 2):
            for n, v in start.items():
                dm.params[n].value = v
            dm.get_outputs(return_sum=True)
            _sync()
            t0 = time.perf_counter()
            if path == "fallback":
                FastPlan.maps_many = lambda self, set_point, n_points: None
            try:
                get_fisher_matrix(dm, tv, 0)
            finally:
                FastPlan.maps_many = maps_many
            _sync()
            if i >= 2:
                ts.append(time.perf_counter() - t0)
        out[path] = _stats(ts)
    out["speedup_median"] = round(out["fallback"]["ms_median"] / out["sweep"]["ms_median"], 3)
    print(json.dumps(out), flush=True)


def kernel_only(reps):
    """`pisa_hip_fisher` alone at 128 and 4 800 bins (12 rows, P = 4, with a truth map), for a kernel trace"""
    from pisa_amd import kernels as K

    rs = np.random.RandomState(0)
    for n_bins in (128, 4800):
        h = K.to_device(rs.gamma(2.0, 5.0, (9, 12, n_bins)))
        v = K.to_device(rs.gamma(2.0, 5.0, (9, 12, n_bins)))
        truth = K.to_device(rs.poisson(60.0, n_bins).astype(np.float64))
        for _ in range(reps):
            res = K.fisher(h, v, [2, 4, 6, 8], [1, 3, 5, 7], [1.0, 0.5, 0.25, 2.0], truth=truth)
        print(json.dumps(dict(workload="kernel_only", n_bins=n_bins, rows=12, P=4, reps=reps,
                              nonempty=res["nonempty"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-cfg", action="store_true")
    ap.add_argument("--skip-synthetic", action="store_true")
    ap.add_argument("--kernel-only", action="store_true", help="only pisa_hip_fisher launches (under a kernel trace)")
    args = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    if args.kernel_only:
        kernel_only(args.reps)
        return
    if not args.skip_synthetic:
        synthetic_lines(args.events, args.reps)
    if not args.skip_cfg:
        cfg_line(max(3, args.reps // 4))


if __name__ == "__main__":
    main()
