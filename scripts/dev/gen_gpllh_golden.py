"""Writes tests/golden/gpllh_ref.npz: the reference's generalized Poisson-gamma likelihood, its stage's outputs and the
inputs they were computed from (arrays only).  Needs a checkout of the reference (PISA_REFERENCE_ROOT, as
oracle/ref_shim.py) and Cython.  Everything is the reference's own code, imported by path through the
oracle/ref_shim.py importer: poisson_gamma_mixtures.pyx (+ poisson_gamma.c) is compiled into a temporary directory and
registered as pisa.utils.llh_defs.poisson_gamma_mixtures; the stage's setup_function / apply_function
(pisa/stages/likelihood/generalized_llh_params.py) run on duck-typed containers, the metric
(pisa/utils/stats.py generalized_poisson_llh, with llh_defs/poisson.py fast_pgmix) on duck-typed MapSets.  Nothing
built from the reference is kept.

    python scripts/dev/gen_gpllh_golden.py
"""
import importlib
import importlib.util
import os
import shutil
import subprocess
import sys
import sysconfig
import tempfile
import types
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402


def build_mixtures():
    src = os.path.join(ref_shim.REF_ROOT, "pisa", "utils", "llh_defs")
    tmp = tempfile.mkdtemp(prefix="gpllh_")
    for f in ("poisson_gamma_mixtures.pyx", "poisson_gamma.c", "poisson_gamma.h"):
        shutil.copy(os.path.join(src, f), tmp)
    subprocess.check_call([sys.executable, "-m", "cython", "-3", "poisson_gamma_mixtures.pyx"], cwd=tmp)
    ext = sysconfig.get_config_var("EXT_SUFFIX")
    inc = [sysconfig.get_paths()["include"], np.get_include(), tmp]
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", "poisson_gamma_mixtures" + ext,
                           "poisson_gamma_mixtures.c", "poisson_gamma.c"] + ["-I" + i for i in inc] + ["-lm"], cwd=tmp)
    spec = importlib.util.spec_from_file_location("pisa.utils.llh_defs.poisson_gamma_mixtures",
                                                  os.path.join(tmp, "poisson_gamma_mixtures" + ext))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, tmp


def reference_modules(mix):
    """(stats module, stage class) of the reference, imported through the shim"""
    ref_shim.install()
    p = os.path.join(ref_shim.REF_ROOT, "pisa")
    ref_shim._pkg("pisa.utils.llh_defs", os.path.join(p, "utils", "llh_defs"))
    sys.modules["pisa.utils.llh_defs.poisson_gamma_mixtures"] = mix
    sys.modules["pisa.utils.llh_defs"].poisson_gamma_mixtures = mix
    ref_shim._pkg("pisa.stages.likelihood", os.path.join(p, "stages", "likelihood"))
    stats = importlib.import_module("pisa.utils.stats")
    stage = importlib.import_module("pisa.stages.likelihood.generalized_llh_params")
    return stats, stage.generalized_llh_params


class ShimContainer:
    """the Container surface the stage touches: per-representation arrays, aux data, keys, size"""

    def __init__(self, name, n_events, n_bins):
        self.name, self.rep = name, "events"
        self.data = {"events": {}, "binned": {}}
        self.aux = {}
        self.n = {"events": n_events, "binned": n_bins}

    @property
    def size(self):
        return self.n[self.rep]

    @property
    def keys(self):
        return list(self.data[self.rep]) + list(self.aux)

    def __getitem__(self, key):
        if key in self.aux:
            return self.aux[key]
        if self.rep == "binned" and key not in self.data["binned"] and key in self.data["events"]:
            # the real container translates the events to the binning here; the stage only overwrites it
            self.data["binned"][key] = np.zeros(self.n["binned"])
        return self.data[self.rep][key]

    def __setitem__(self, key, val):
        self.data[self.rep][key] = np.asarray(val)

    def set_aux_data(self, key, val):
        self.aux[key] = val

    def mark_changed(self, key):
        pass


class ShimData:
    def __init__(self, containers):
        self.containers = containers

    def __iter__(self):
        return iter(self.containers)

    @property
    def representation(self):
        return self.containers[0].rep

    @representation.setter
    def representation(self, rep):
        for c in self.containers:
            c.rep = "events" if rep == "events" else "binned"


def run_stage(stage_cls, conts, n_bins):
    st = object.__new__(stage_cls)
    st.apply_mode = types.SimpleNamespace(tot_num_bins=n_bins)
    st.data = ShimData(conts)
    st.setup_function()
    st.apply_function()
    st.data.representation = "binned"
    return st


def mapset(rows):
    return types.SimpleNamespace(maps=[types.SimpleNamespace(hist=np.asarray(r, dtype=np.float64)) for r in rows])


def case(rs, ref, n_cont, n_bins, events_per_cont, data_scale, empty=(), kfold=False, zero_weight_bins=0,
         equal_weight_bins=0, const_weight=None, data=None):
    stats, stage_cls, mix = ref
    conts, w_all, bins_all, kf_all = [], [], [], []
    for c in range(n_cont):
        n = events_per_cont[c] if np.ndim(events_per_cont) else events_per_cont
        wts = rs.lognormal(-3.0, 1.0, n) if const_weight is None or c > 0 else np.full(n, const_weight)
        bins = rs.randint(0, n_bins, n)
        for z in range(zero_weight_bins):
            wts[bins == z] = 0.0
        for z in range(zero_weight_bins, zero_weight_bins + equal_weight_bins):
            wts[bins == z] = 0.25
        kf = rs.rand(n) < 0.7 if kfold else np.ones(n, dtype=bool)
        cont = ShimContainer("c%d" % c, n, n_bins)
        cont["weights"] = wts.copy()
        for i in range(n_bins):
            cont["bin_%d_mask" % i] = bins == i
        if kfold:
            cont["kfold_mask"] = kf.copy()
        conts.append(cont)
        w_all.append(wts)
        bins_all.append(bins)
        kf_all.append(kf)
    run_stage(stage_cls, conts, n_bins)
    get = lambda key: np.array([np.asarray(c[key], dtype=np.float64).ravel() for c in conts])
    A, B, W, OLD, nmc = get("llh_alphas"), get("llh_betas"), get("weights"), get("old_sum"), get("n_mc_events")
    adj = np.array([c["mean_adjustment"] for c in conts])
    if data is None:
        data = np.floor(rs.poisson(W.sum(axis=0) * data_scale) + rs.rand(n_bins) * 0.9)
    data = np.asarray(data, dtype=np.float64)
    ev = OrderedDict(weights=mapset(W), llh_alphas=mapset(A), llh_betas=mapset(B), n_mc_events=mapset(nmc))
    with np.errstate(all="ignore"):
        out = stats.generalized_poisson_llh(actual_values=data, expected_values=ev, empty_bins=list(empty))
    # which rule each bin took, and the raw eq. 91 value where the mixture applies (the reference's own function)
    branch = np.where(np.isin(np.arange(n_bins), list(empty)), 0, np.where(np.all(nmc > 100, axis=0), 1, 2))
    ret = np.full(n_bins, np.nan)
    for i in np.flatnonzero(branch == 2):
        m = np.isfinite(A[:, i]) & np.isfinite(B[:, i])
        ret[i] = mix.c_generalized_pg_mixture(int(data[i]), np.ascontiguousarray(A[m, i]), np.ascontiguousarray(B[m, i]))
    return dict(weights=np.concatenate(w_all), bins=np.concatenate(bins_all), kfold=np.concatenate(kf_all),
                has_kfold=np.array([bool(kfold)]), sizes=np.array([len(x) for x in w_all]), n_mc=nmc, adjust=adj,
                alpha=A, beta=B, wsum=W, old_sum=OLD, data=data, empty=np.array(list(empty), dtype=np.int64),
                per_bin=np.asarray(out, dtype=np.float64), ret=ret, branch=branch, total=np.array([np.sum(out)]))


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gpllh_ref.npz"))
    args = ap.parse_args()
    mix, tmp = build_mixtures()
    try:
        stats, stage_cls = reference_modules(mix)
        ref = (stats, stage_cls, mix)
        rs = np.random.RandomState(20190823)
        cases = {
            "lowmc": case(rs, ref, 3, 40, 60, 30.0, empty=(3, 7)),
            "single": case(rs, ref, 1, 16, 40, 5.0),
            "sparse_adj": case(rs, ref, 4, 64, 20, 200.0, zero_weight_bins=2, equal_weight_bins=2),
            "kfold": case(rs, ref, 2, 24, 120, 20.0, kfold=True),
            "highmc": case(rs, ref, 2, 8, 2000, 1.0, empty=(5,)),
            "many": case(rs, ref, 16, 12, [30 * (c + 1) for c in range(16)], 40.0),
            "longk": case(rs, ref, 12, 6, 150, 80.0),
            # prefac underflows to 0 and delta_k overflows: NaN -> +1 (fast_pgmix)
            "nan": case(rs, ref, 2, 2, [20000, 5], 1.0, const_weight=10.0, data=[300.5, 40.0]),
            # k = 0 everywhere in the Poisson branch: the reference gives NaN (0 log 0), the package -sum w
            "zero_k": case(rs, ref, 2, 4, 3000, 1.0, data=[0.0, 0.0, 0.0, 0.0]),
        }
        flat = {}
        for name, d in cases.items():
            for key, v in d.items():
                flat["%s__%s" % (name, key)] = np.asarray(v)
        flat["cases"] = np.array(sorted(cases))
        np.savez_compressed(args.out, **flat)
        for name, d in cases.items():
            print("%-10s k max %5d  branches %s  +1: %d, log(1e-300): %d, NaN: %d" % (
                name, int(d["data"].max()), np.bincount(d["branch"], minlength=3).tolist(),
                int(np.sum(d["per_bin"] == 1.0)), int(np.sum(d["per_bin"] == np.log(1e-300))),
                int(np.sum(np.isnan(d["per_bin"])))))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
