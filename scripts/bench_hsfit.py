"""Time of one `pisa_hip_hypersurface_fit` launch, one JSON line per batch size:

  * 1e3, 1e5 and 1e6 problems of 16 sets and 6 coefficients (log mode; quadratic + exponential_scaled +
    logarithmic: the seeded design of tests/hsfit_cases.py, fresh draws per problem), median and minimum of
    20 launches, the inputs resident on the device, each launch ended by a device synchronise;
  * as context, the numpy restatement of the fit (tests/hsfit_cases.py) on the host for the first 1e3 problems.

Every batch size runs in a process of its own under its own time limit; the first one that fails ends the script.

    python scripts/bench_hsfit.py [--reps 20] [--sizes 1000,100000,1000000] [--skip-host]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_SECONDS = 240


def inputs(n_prob, seed=5):
    """the design of `tests.hsfit_cases.case_a`, vectorised over the problems"""
    from tests import hsfit_cases as H

    x = H.case_a(1)[0]
    rs = np.random.RandomState(seed)
    c = np.stack([rs.normal(0.0, 0.05, n_prob), rs.normal(0.0, 0.5, n_prob), rs.normal(0.0, 0.5, n_prob),
                  rs.normal(0.0, 0.1, n_prob), rs.normal(0.4, 0.05, n_prob), rs.normal(0.3, 0.1, n_prob)])
    eta = (c[0] + c[1] * x[0][:, None] + c[2] * x[0][:, None] ** 2
           + (c[3] + 1.0) * (np.exp(c[4] * x[1][:, None]) - 1.0) + np.log(1.0 + c[5] * x[2][:, None]))
    y0 = np.exp(eta)
    sigma = 0.01 * y0 * rs.uniform(0.5, 2.0, y0.shape)
    return x, y0 + sigma * rs.normal(size=y0.shape), sigma


def one_size(n_prob, reps):
    import torch

    from pisa_amd import _lib
    from pisa_amd import kernels as K
    from tests import hsfit_cases as H

    torch.cuda.set_device(0)
    x, y, sigma = inputs(n_prob)
    y, sigma = torch.from_numpy(y).cuda(), torch.from_numpy(sigma).cuda()
    lo, hi = H.free_box(6)
    ts = []
    for i in range(reps + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = K.hypersurface_fit(x, H.FORMS_A, y, sigma, np.zeros(6), lo, hi, np.zeros(6), True)
        torch.cuda.synchronize()
        if i >= 3:
            ts.append(time.perf_counter() - t0)
    status = res["status"].cpu().numpy()
    n_iter = res["n_iter"].cpu().numpy()
    print(json.dumps(dict(workload="hypersurface_fit", n_prob=n_prob, n_sets=16, n_coef=6, reps=reps,
                          ms_median=round(1e3 * float(np.median(ts)), 4), ms_min=round(1e3 * float(np.min(ts)), 4),
                          us_per_problem=round(1e6 * float(np.median(ts)) / n_prob, 4),
                          converged=int(np.count_nonzero(status == 0)),
                          not_converged=int(np.count_nonzero(status & _lib.HSFIT_NOT_CONVERGED)),
                          trial_points_mean=round(float(n_iter.mean()), 2), trial_points_max=int(n_iter.max()))),
          flush=True)


def host_line(n_prob=1000):
    from tests import hsfit_cases as H

    x, y, sigma = inputs(n_prob)
    lo, hi = H.free_box(6)
    t0 = time.perf_counter()
    out = H.batch_solver(x, H.FORMS_A, y, sigma, np.zeros(6), lo, hi, np.zeros(6), True, False)
    dt = time.perf_counter() - t0
    print(json.dumps(dict(workload="numpy_restatement_host", n_prob=n_prob, n_sets=16, n_coef=6,
                          ms=round(1e3 * dt, 1), us_per_problem=round(1e6 * dt / n_prob, 1),
                          converged=int(np.count_nonzero(out["status"] == 0)))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1000,100000,1000000")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--one", type=int, default=0, help="(internal) time this batch size in this process")
    args = ap.parse_args()
    if args.one:
        one_size(args.one, args.reps)
        return
    for n_prob in [int(float(s)) for s in args.sizes.split(",")]:
        # a fresh process per size, under its own limit; nothing more is started after one that fails
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n_prob), "--reps",
                                   str(args.reps)], timeout=STEP_SECONDS)
        except subprocess.TimeoutExpired:
            sys.exit("batch size %d ran into its limit of %d s: stopping" % (n_prob, STEP_SECONDS))
        if done.returncode != 0:
            sys.exit("batch size %d failed with status %d: stopping" % (n_prob, done.returncode))
    if not args.skip_host:
        host_line()


if __name__ == "__main__":
    main()
