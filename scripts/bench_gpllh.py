"""Step time of `llh` against `generalized_poisson_llh` on one engine, one device, one process: the two kinds
alternate point by point (eval_host, the fit loop's call) so that clocks and caches see the same history.
  headline: 1e7 events, 12 containers, 8x8x2 bins, Asimov-like data -- every bin takes the Poisson branch;
  low-MC:   2e4 events on the same binning, data = the template scaled to a largest count of 500 -- every bin
            takes the eq. 91 mixture (a k-step recursion of k / 64 terms per lane and step).
Prints one JSON line per workload.  rocprofv3 --kernel-trace --stats on `--only lowmc` gives the tail kernel's
time and the launches per step."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(name, n_events, k_max, steps, warmup):
    import numpy as np
    import torch

    from pisa_amd import synthetic

    wl = synthetic.Workload(n_events=n_events, out_binning="dragon", seed=0)
    st = synthetic.DeviceState(wl, compact=True)
    p0 = wl.osc_params()
    st.make_pseudo_data(p0, seed=0)
    st.accumulate(p0)
    st.allreduce()
    st.finalize()
    t = st.ws.hist.sum(dim=0).cpu().numpy()
    st.set_data(np.floor(t if k_max is None else t * (k_max / t.max())))
    n_mc, _ = st.configure_gpllh()
    mixture = (n_mc <= 100).any(axis=0)
    pts = [wl.osc_params(theta23_deg=40.0 + 10.0 * i / steps, dm31=2.4e-3) for i in range(steps)]
    for i in range(warmup):
        for kind in ("llh", "generalized_poisson_llh"):
            st.eval_host(pts[i % steps], kind)
    st.check_status()
    t = {"llh": [], "generalized_poisson_llh": []}
    for p in pts:
        for kind in t:
            t0 = time.perf_counter()
            st.eval_host(p, kind)
            t[kind].append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    st.check_status()
    data = st.data.cpu().numpy()
    out = {"workload": name, "events": wl.n_events, "bins": wl.n_bins, "containers": len(wl.events),
           "mixture_bins": int(mixture.sum()), "k_max_mixture": int(data[mixture].max()) if mixture.any() else 0,
           "steps": steps}
    for kind, v in t.items():
        out["%s_us_median" % kind] = round(1e6 * float(np.median(v)), 1)
        out["%s_us_min" % kind] = round(1e6 * float(np.min(v)), 1)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=("headline", "lowmc"), default=None)
    a = ap.parse_args()
    if a.only in (None, "headline"):
        run("headline", 10_000_000, None, a.steps, a.warmup)
    if a.only in (None, "lowmc"):
        run("lowmc", 20_000, 500.0, a.steps, a.warmup)


if __name__ == "__main__":
    main()
