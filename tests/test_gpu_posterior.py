"""The nuisance-posterior sampler on the device (csrc/posterior.hip: `pisa_hip_posterior_sample` through
`kernels.posterior_sample`) against the numpy restatement (tests/posterior_cases.py), its invariances, its status
words, its statistics on exactly known targets, and `pisa_hip_fluctuate_linear_at` (data at given truths) against
`fluctuate_linear` and the restatement of tests/truth_cases.py.

Positions must equal the restatement's bit for bit up to a problem's first marked decision; the share of marked
decisions is held to 1e-5 and at the seeds of the shapes the restatement marks none (asserted here and, without a
GPU, in tests/test_host_posterior.py), so every position is compared.  A stored lp lies inside the window of a log
within `fluctuate_method_cases.LOG_ULPS` of numpy's (`posterior_cases.logp_window`; `==` for the chi2 kinds)."""
import numpy as np
import pytest

from tests import fluctuate_method_cases as fm
from tests import posterior_cases as po
from tests import truth_cases as tc

pytestmark = pytest.mark.gpu

MAX_MARGINAL_SHARE = 1e-5


@pytest.fixture(scope="module")
def K():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from pisa_amd import kernels

    return kernels


def _dev(K, a, dtype=np.float64):
    import torch

    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(K.device())


def _run(K, f, kind, x0, n_steps, **kw):
    """`kernels.posterior_sample` on the raw arrays of a case -> host arrays"""
    ids = kw.pop("chain_id", None)
    out = K.posterior_sample(kind, _dev(K, f["D"]), _dev(K, f["E"]), _dev(K, f["R"]), _dev(K, x0), n_steps, po.SEED,
                             t_of=_dev(K, f["t_of"], np.int32), k_of=_dev(K, f["k_of"], np.int32),
                             sigma2=_dev(K, f["S2"]), inv_prior_sigma=_dev(K, f["ips"]), center=_dev(K, f["c"]),
                             lower=_dev(K, f["lo"]), upper=_dev(K, f["hi"]), chain_id=_dev(K, ids, np.int64), **kw)
    assert all(v.is_cuda for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _sub(f, idx):
    """the problems `idx` of a case (the rows stay where they are)"""
    return dict(f, t_of=f["t_of"][idx], k_of=f["k_of"][idx])


def test_the_layout_the_cases_were_chosen_by(K):
    for kind, J, W in (("mod_chi2", 3, 34), ("poisson_llh", 8, 256), ("mod_chi2", 1, 2), ("llh", 8, 16), ("llh", 1, 16)):
        lay = K.posterior_layout(kind, J, W)
        assert (lay["problems"], lay["stage_bins"]) == po.layout(kind, J, W)


@pytest.mark.parametrize("q", po.GPU_CASES, ids=po.gpu_case_id)
def test_chains_equal_the_restatement(K, q):
    kind, P, B, J, W, bounds, n_steps, first = q
    f, want = po.gpu_want(q)
    got = _run(K, f, kind, f["x0"], n_steps, stream=3, chain_id=np.arange(P) + 11, first_step=first)
    marked = want["n_marginal"] + want["n_edge"]
    assert marked <= MAX_MARGINAL_SHARE * want["n_decisions"]
    assert marked == 0                   # this seed: every position is compared (another seed rather than a window)
    assert np.array_equal(got["status"], want["status"]) and not got["status"].any()
    assert got["chain"].shape == (P, n_steps, W, J)
    assert np.array_equal(got["chain"], want["chain"])
    assert np.array_equal(got["end"], want["end"]) and np.array_equal(got["end"], got["chain"][:, -1])
    assert np.array_equal(got["accepted"], want["accepted"])
    # accepted = the count of moved states
    states = np.concatenate([f["x0"][:, None], got["chain"]], axis=1)
    moved = (states[:, 1:] != states[:, :-1]).any(axis=3).sum(axis=1)
    assert np.array_equal(got["accepted"], moved)
    window = po.logp_window(kind, want["S"])
    err = np.abs(got["logp"] - want["logp"])
    print(po.gpu_case_id(q), "largest lp distance / window:", float(np.max(err / np.maximum(window, 1e-300)))
          if kind in po.LLH_KINDS else float(err.max()))
    assert np.all(err <= window)


def test_invariances(K):
    """a problem alone, in a batch, in a reversed batch; one call against split calls through `end` / `first_step`;
    `thin` / `keep_from` against slices of the full chain; all with =="""
    f = po.case("poisson_llh", 9, 65, 3, 34, "box")
    ids = np.arange(9) + 40
    kw = dict(stream=2, first_step=100)
    full = _run(K, f, "poisson_llh", f["x0"], 20, chain_id=ids, **kw)
    assert not full["status"].any()
    rev = np.arange(9)[::-1].copy()
    back = _run(K, _sub(f, rev), "poisson_llh", f["x0"][rev], 20, chain_id=ids[rev], **kw)
    for name in ("chain", "logp", "accepted", "end"):
        assert np.array_equal(back[name][::-1], full[name]), name
    for p in (0, 4, 8):
        one = np.array([p])
        alone = _run(K, _sub(f, one), "poisson_llh", f["x0"][one], 20, chain_id=ids[one], **kw)
        for name in ("chain", "logp", "accepted", "end"):
            assert np.array_equal(alone[name][0], full[name][p]), (name, p)
    a = _run(K, f, "poisson_llh", f["x0"], 8, chain_id=ids, stream=2, first_step=100)
    b = _run(K, f, "poisson_llh", a["end"], 12, chain_id=ids, stream=2, first_step=108)
    assert np.array_equal(np.concatenate([a["chain"], b["chain"]], axis=1), full["chain"])
    assert np.array_equal(np.concatenate([a["logp"], b["logp"]], axis=1), full["logp"])
    assert np.array_equal(a["accepted"] + b["accepted"], full["accepted"]) and np.array_equal(b["end"], full["end"])
    for keep_from, thin in ((0, 3), (103, 4), (110, 1), (119, 7), (500, 2)):
        part = _run(K, f, "poisson_llh", f["x0"], 20, chain_id=ids, keep_from=keep_from, thin=thin, **kw)
        kept = [i for i in range(20) if 100 + i >= keep_from and (100 + i - keep_from) % thin == 0]
        assert part["chain"].shape[1] == len(kept)
        assert np.array_equal(part["chain"], full["chain"][:, kept]), (keep_from, thin)
        assert np.array_equal(part["logp"], full["logp"][:, kept]) and np.array_equal(part["end"], full["end"])
    # another seed word, stream or chain id: other chains
    other = _run(K, f, "poisson_llh", f["x0"], 20, chain_id=ids + 1, **kw)
    assert not np.array_equal(other["chain"], full["chain"])
    assert not np.array_equal(_run(K, f, "poisson_llh", f["x0"], 20, chain_id=ids, stream=3, first_step=100)["chain"],
                              full["chain"])


def test_status_problems_are_nan_and_disturb_no_neighbour(K):
    f = po.case("poisson_llh", 5, 9, 2, 8, "box")
    lo, hi, x0 = np.array(f["lo"]), np.array(f["hi"]), np.array(f["x0"])
    # every problem its own template row, so that one row can carry bad bounds
    g = dict(f, E=f["E"][f["k_of"]], S2=f["S2"][f["k_of"]], R=f["R"][f["k_of"]], c=f["c"][f["k_of"]],
             lo=lo[f["k_of"]], hi=hi[f["k_of"]], k_of=np.arange(5, dtype=np.int32))
    clean = _run(K, g, "poisson_llh", x0, 6, chain_id=np.arange(5))
    assert not clean["status"].any()
    x0[1, 3, 0] = 9.0                               # a walker outside its box
    g["lo"][2, 1], g["hi"][2, 1] = 1.0, -1.0        # lo > hi
    g["lo"][3], g["hi"][3] = -np.inf, np.inf
    x0[3, 5, 0] = -1e4                              # a walker outside the domain
    got = _run(K, g, "poisson_llh", x0, 6, chain_id=np.arange(5))
    assert list(got["status"]) == [0, po.START_OUTSIDE, po.BAD_BOUNDS, po.START_OUTSIDE, 0]
    for p in (1, 2, 3):
        assert np.isnan(got["chain"][p]).all() and np.isnan(got["logp"][p]).all() and np.isnan(got["end"][p]).all()
        assert not got["accepted"][p].any()
    for p in (0, 4):
        for name in ("chain", "logp", "accepted", "end"):
            assert np.array_equal(got[name][p], clean[name][p]), (name, p)
    want = po.sample(po.problems("poisson_llh", g["D"], g["E"], g["R"], g["S2"], g["ips"], g["c"], g["lo"], g["hi"],
                                 g["t_of"], g["k_of"]), x0, 6, po.SEED, chain_id=np.arange(5))
    assert np.array_equal(got["chain"], want["chain"], equal_nan=True)
    # a negative datum in a row that is read; a row index outside its array
    bad = dict(f, D=np.where(np.arange(9)[None, :] == 4, -1.0, f["D"]))
    with pytest.raises(ValueError):
        _run(K, bad, "poisson_llh", f["x0"], 2)
    from pisa_amd import _lib

    with pytest.raises(_lib.PisaHipError):
        _run(K, dict(f, k_of=np.array([0, 1, 2, 3, 4], dtype=np.int32)), "poisson_llh", f["x0"], 2)
    # the MC-uncertainty metrics have no form here, as in the fit
    with pytest.raises(ValueError, match="no profiled form"):
        _run(K, f, "mcllh_mean", f["x0"], 2)


def test_every_invalid_call_is_refused_before_launch(K):
    from pisa_amd import _lib

    for name, rc in po.invalid_calls(_lib.lib()):
        assert rc == -1, name
    f = po.case("llh", 2, 5, 2, 8, "box")
    for what, kw in (("odd walkers", dict(x0=f["x0"][:, :7])), ("fewer walkers than 2 J", dict(x0=f["x0"][:, :2])),
                     ("steps beyond 2^32", dict(first_step=2 ** 32 - 1)), ("thin 0", dict(thin=0))):
        with pytest.raises(ValueError):
            _run(K, f, "llh", kw.pop("x0", f["x0"]), 2, **kw)


# ------------------------------------------------------------------------------------------ data at given truths
def test_fluctuate_linear_at(K):
    """`==` `fluctuate_linear` with every scale 0 at the shift; `==` the restatement of tests/truth_cases.py on per-trial
    truths at (T, J) in {(1, 1), (65, 3), (257, 8)}, every method; a NaN truth gives a NaN row"""
    B = 65
    mu0, sigma = fm.palette_rows(B)
    entries = flagged = 0
    for i, (T, J) in enumerate(((1, 1), (65, 3), (257, 8))):
        R = tc.responses(J, B, mu0)
        rs = np.random.RandomState(100 + i)
        eta = 0.5 * rs.randn(T, J)
        shift = 0.3 * rs.randn(J)
        first = tc.first_trial_of(T)
        for method in tc.METHODS:
            sg = None if method == "poisson" else _dev(K, sigma)
            same = K.fluctuate_linear_at(_dev(K, mu0), _dev(K, R), _dev(K, np.tile(shift, (T, 1))), tc.SEED,
                                         method=method, sigma=sg, stream=tc.STREAM, first_trial=first)
            ref = K.fluctuate_linear(_dev(K, mu0), _dev(K, R), T, tc.SEED, np.zeros(J), shift, method=method, sigma=sg,
                                     stream=tc.STREAM, first_trial=first)
            assert np.array_equal(same["data"].cpu().numpy(), ref["data"].cpu().numpy(), equal_nan=True), (T, J, method)
            assert same["clipped"] == ref["clipped"]
            out = K.fluctuate_linear_at(_dev(K, mu0), _dev(K, R), _dev(K, eta), tc.SEED, method=method, sigma=sg,
                                        stream=tc.STREAM, first_trial=first)
            got = out["data"].cpu().numpy()
            want, lo, hi, marginal, clipped = tc.block(mu0, sigma, R, eta, method, tc.SEED, tc.STREAM, first)[:5]
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), (T, J, method)
            inside = nan | marginal | ((lo <= got) & (got <= hi))
            assert inside.all(), (T, J, method, np.argwhere(~inside)[:5])
            assert out["clipped"] == clipped
            entries, flagged = entries + int((~nan).sum()), flagged + int((marginal & ~nan).sum())
    assert flagged <= MAX_MARGINAL_SHARE * entries and flagged == 0
    eta = np.zeros((3, 2))
    eta[1, 0] = np.nan
    R = np.ones((2, B))
    got = K.fluctuate_linear_at(_dev(K, mu0), _dev(K, R), _dev(K, eta), tc.SEED)["data"].cpu().numpy()
    assert np.isnan(got[1]).all() and not np.isnan(got[0][~np.isnan(mu0)]).any()
    with pytest.raises(ValueError, match="scaled_poisson"):
        K.fluctuate_linear_at(_dev(K, mu0), _dev(K, R), _dev(K, eta), tc.SEED, method="scaled_poisson",
                              sigma=_dev(K, sigma))


# ------------------------------------------------------------------------------------------------- statistics
def _device_sampler(K):
    def run(pr, x0, n_steps, seed, stream=0, chain_id=None, keep_from=0, marks=False):
        P = x0.shape[0]
        assert seed < 2 ** 63
        out = K.posterior_sample(pr["kind"], _dev(K, pr["d"]), _dev(K, pr["e"]), _dev(K, pr["R"]), _dev(K, x0),
                                 n_steps, seed, inv_prior_sigma=_dev(K, pr["ips"]), center=_dev(K, pr["c"]),
                                 lower=_dev(K, pr["lo"]), upper=_dev(K, pr["hi"]), stream=stream,
                                 chain_id=_dev(K, np.arange(P) if chain_id is None else chain_id, np.int64),
                                 keep_from=keep_from)
        return {k: v.cpu().numpy() for k, v in out.items()}

    return run


def test_truncated_gaussian_posterior_on_the_device(K):
    """the J = 3 target of tests/test_host_posterior.py with its lengths (tau 48.2 steps: burn-in 500, kept 2500) and its
    bounds: five standard errors of 32 replicas, the standard error at most 0.05 posterior sigma"""
    J, W = 3, 16
    arrays, mean, var, sigma = po.gauss_target(J)
    burn, keep = po.LENGTHS[(J, W)]
    m, v, out = po.replica_moments(arrays, "llh", J, W, burn, keep, mean + 0.3 * sigma, sigma,
                                   sampler=_device_sampler(K))
    assert not out["status"].any()
    po.check_moments(m, mean, np.sqrt(var), "device gauss J=3 mean")
    po.check_moments(v, var, var, "device gauss J=3 variance")


@pytest.mark.parametrize("d", (0, 3))
def test_poisson_posterior_of_one_bin_on_the_device(K, d):
    arrays, mean, var = po.poisson_target(d)
    burn, keep = po.LENGTHS[(1, 16)]
    m, v, out = po.replica_moments(arrays, "llh", 1, 16, burn, keep, np.array([mean]), np.array([np.sqrt(var)]),
                                   sampler=_device_sampler(K))
    assert not out["status"].any()
    po.check_moments(m, np.array([mean]), np.sqrt(var), "device poisson d=%d mean" % d)
    po.check_moments(v, np.array([var]), var, "device poisson d=%d variance" % d)


# ------------------------------------------------------------------------------------------- config pipeline
SKEW_ALLOWANCE = 0.1       # of sigma: |posterior mean - mode| of a flag-free interior fit; see the test's docstring


def test_the_posterior_on_the_config_pipeline(K):
    """A 3 x 3 grid (theta23 x deltam31) of example_hip.cfg with aeff_scale and delta_index in a bounded response; the
    observed map is one row of point 4 drawn at displaced truths.
    Interior fits: the sample mean lies within 5 sqrt(cov_jj tau_j / (n_keep W)) of eta_obs (tau_j in kept samples, at
    least 1: the standard error of the mean of n_keep W draws with that autocorrelation) plus SKEW_ALLOWANCE sigma_j,
    the distance between the posterior's mean and its mode.  Measured with the restatement solver on the same inputs
    (tests/posterior_cases.NumpySolver; 200 bins, 4.1e5 counts; 32 walkers, 300 + 400 x 5 steps): |mean - eta_obs| is at
    most 0.028 sigma for aeff_scale and 0.041 sigma for delta_index over the nine points, the chain's own standard
    error of 0.02 to 0.03 sigma included (and the device's chains were those of the restatement bit for bit).  A
    Poisson likelihood of N counts in a normalisation has mean - mode = sigma / sqrt(N), so 0.1 sigma covers every map
    of more than 100 counts.
    A held coordinate (the same response with aeff_scale's upper bound below the fit): its sample has spread and lies
    strictly inside the box, what the Gaussian of nuisance="fitted" (a zero row and column) cannot give.
    `feldman_cousins(truths=sample, generator="device")` is the loop over `pseudo_data` + `delta_metric`, whatever the
    chunks, its data rows equal the restatement's on the sample's rows, and its critical values those of the run on
    the restatement solver within 1e-8 (two metric values of a magnitude below 1e7, each within 4 x 64 eps of it)."""
    from pisa_amd.analysis import ensemble as en
    from pisa_amd.core.distribution_maker import DistributionMaker

    names = ("aeff_scale", "delta_index")
    dm = DistributionMaker("settings/pipeline/example_hip.cfg")
    for name in dm.params.free.names:
        if name not in ("theta23", "deltam31") and name not in names:
            dm.params.fix(name)
    dm.get_outputs(return_sum=True)
    th, dm31 = dm.params["theta23"].value, dm.params["deltam31"].value
    pts = en.grid_points(dm, {"theta23": [th * 0.8, th, th * 1.15], "deltam31": [dm31 * 0.9, dm31, dm31 * 1.1]})
    metric = "llh"
    grid = en.TemplateGrid.from_maker(dm, pts, metric)
    assert len(grid) == 9
    resp = en.NuisanceResponse.from_maker(dm, grid, names, {"aeff_scale": (-0.05, 0.05), "delta_index": (-0.05, 0.05)},
                                          bounded=True)
    displaced = np.array([0.06, 0.03])
    observed = K.fluctuate_linear(grid.hist[4], resp.response[4], 1, 5, np.zeros(2), displaced,
                                  stream=4)["data"].cpu().numpy()[0]
    fit = en.fit_observed(observed, grid, metric, resp, covariance=True)
    assert not fit["status"].any() and not fit["hesse_status"].any()          # every fit interior and flag-free
    W, n_keep, thin = 32, 400, 5
    s = en.posterior_sample(observed, grid, metric, resp, n_keep=n_keep, n_walkers=W, thin=thin, n_burn=300,
                            random_state=21)
    assert s.eta.shape == (9, n_keep * W, 2) and not s.status.any()
    tau_kept = np.maximum(s.tau / thin, 1.0)
    limit = 5.0 * np.sqrt(fit["sigma"] ** 2 * tau_kept / (n_keep * W)) + SKEW_ALLOWANCE * fit["sigma"]
    off = np.abs(s.mean() - fit["eta"])
    print("tau (steps)", np.round(s.tau, 1), "acceptance", np.round(s.acceptance, 2))
    print("|mean - eta_obs| / sigma", np.round(off / fit["sigma"], 3), "limit / sigma", np.round(limit / fit["sigma"], 3))
    assert np.all(off <= limit)
    assert np.all(np.abs(np.sqrt(np.einsum("pjj->pj", s.cov())) / fit["sigma"] - 1.0) < 0.25)
    # the grid and the response as host arrays, for the restatement solver below
    host_grid = en.TemplateGrid(grid.host("hist"), grid.host("sumw2"), grid.points, None, grid.penalty, metric)
    host_resp = en.NuisanceResponse(names, resp.response.cpu().numpy(), resp.inv_prior_sigma, resp.center,
                                    resp.prior_at_point, resp.values, resp.max_iter, resp.lower, resp.upper)
    # a subset of points, and the pilot on the device
    one = en.posterior_sample(observed, grid, metric, resp, points=[4], n_keep=n_keep, n_walkers=W, thin=thin,
                              n_burn=300, random_state=21)
    assert np.array_equal(one.eta[0], s.eta[4])
    auto = en.posterior_sample(observed, grid, metric, resp, points=[4], n_keep=20, n_walkers=W, pilot_steps=400,
                               random_state=21)
    assert auto.n_burn == 400 and auto.thin == int(np.ceil(auto.thin)) >= 1 and not auto.status.any()

    # a coordinate held on a bound
    upper = np.array(resp.upper)
    upper[:, 0] = 0.03                                  # below the fitted aeff_scale displacement of every point
    tight = en.NuisanceResponse(names, resp.response, resp.inv_prior_sigma, resp.center, resp.prior_at_point,
                                resp.values, resp.max_iter, resp.lower, upper)
    held = en.fit_observed(observed, grid, metric, tight, covariance=True)
    assert np.all(held["eta"][4, 0] == 0.03) and held["cov"][4, 0, 0] == 0.0 and held["hesse_status"][4] == 32
    t = en.posterior_sample(observed, grid, metric, tight, points=[4], n_keep=100, n_walkers=W, thin=thin, n_burn=300,
                            random_state=21)
    x = t.eta[0, :, 0]
    print("held coordinate: sample in [%.4f, %.4f], std %.4f" % (x.min(), x.max(), x.std()))
    assert not t.status.any() and x.std() > 0.0 and np.all(x < 0.03) and np.all(x > tight.lower[4, 0])
    assert np.unique(x).size > 0.5 * x.size

    # Feldman-Cousins at the sample
    T, cl, seed, k0 = 64, (0.6827, 0.90), 77, 4
    kw = dict(generator="device", response=resp, truths=s, true_points=[k0])
    crit, info = en.feldman_cousins(grid, metric, T, cl, seed, **kw)
    assert np.array_equal(info["truths_used"], [T])
    d, rows = en.pseudo_data(grid, k0, T, seed, generator="device", response=resp, truths=s, return_truth=True)
    assert d.is_cuda and np.array_equal(rows, s.eta[k0][:T])
    assert np.array_equal(en.critical_values(en.delta_metric(d, grid, metric, k0, response=resp), cl), crit[0])
    for chunk_bytes in (7 * 8 * grid.n_bins, 40 * 8 * grid.n_bins + 5):
        got, _ = en.feldman_cousins(grid, metric, T, cl, seed, chunk_bytes=chunk_bytes, **kw)
        assert np.array_equal(got, crit)
    block = tc.block(host_grid.hist[k0], None, host_resp.response[k0], rows, "poisson", seed, stream=k0)
    got = d.cpu().numpy()
    inside = block[3] | ((block[1] <= got) & (got <= block[2]))
    assert inside.all() and int(block[3].sum()) <= MAX_MARGINAL_SHARE * got.size
    want, _ = en.feldman_cousins(host_grid, metric, T, cl, seed, generator="device", response=host_resp, truths=s,
                                 true_points=[k0], solver=po.NumpySolver())
    print("critical values", crit, "restatement solver", want)
    assert np.all(np.abs(crit - want) <= 1e-8)
    fixed, _ = en.feldman_cousins(grid, metric, T, cl, seed, generator="device", response=resp, true_points=[k0])
    assert not np.array_equal(fixed, crit)
