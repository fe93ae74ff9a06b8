"""Pseudo-data at nuisances fitted to the observed data on the device (csrc/fluctuate_linear.hip:
`pisa_hip_fluctuate_linear_mvn` through `kernels.fluctuate_linear_mvn`) against the numpy restatement
(tests/observed_cases.py), and `nuisance="profiled"` / `"fitted"` of pisa_amd/analysis/ensemble.py with
`generator="device"` on example_hip.cfg.

A trial's truths must lie inside the restatement's window: `==` where every live deviate of the accepted candidate came
from the central branch of AS 241 (at least 0.8^J of the drawn truths per shape, asserted), and otherwise the values a
log within `fluctuate_method_cases.LOG_ULPS` of numpy's reaches, carried through the sum by interval arithmetic; a trial
one of whose candidates lies that close to a box edge is `marginal`, the share is held to 1e-5 and at the seed of the
shapes the restatement marks none (asserted here and, without a GPU, in tests/test_host_observed.py).  No case is
exhausted but the one family built to show the status word.  The data are compared on the kernel's OWN truths, after
that check: every count `==` wherever the restatement does not mark it marginal, with the same cap and the same "this
seed marks none".  The closure gates are those of tests/test_host_observed.py (five standard errors, derived there).
"""
import numpy as np
import pytest

from tests import fluctuate_method_cases as fm
from tests import observed_cases as oc
from tests import truth_cases as tc

pytestmark = pytest.mark.gpu

SEED, STREAM = oc.SEED, oc.STREAM
MAX_MARGINAL_SHARE = 1e-5


@pytest.fixture(scope="module")
def K():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from pisa_amd import kernels

    return kernels


def _dev(K, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(K.device())


def _draw(K, mu0, sigma, R, fit, method, n_trials, seed, stream=0, first_trial=0):
    """(data, eta, clipped) as host arrays; fit = (mean, cov, lower, upper)"""
    out = K.fluctuate_linear_mvn(_dev(K, mu0), _dev(K, R), n_trials, seed, fit[0], fit[1], fit[2], fit[3], method=method,
                                 sigma=None if method == "poisson" else _dev(K, sigma), stream=stream,
                                 first_trial=first_trial)
    assert out["data"].is_cuda and tuple(out["data"].shape) == (n_trials, len(mu0))
    assert out["eta"].is_cuda and tuple(out["eta"].shape) == (n_trials, len(fit[0]))
    return out["data"].cpu().numpy(), out["eta"].cpu().numpy(), out["clipped"]


def _check_truths(eta, tr, what):
    """the kernel's truths against the restatement's dict -> (trials compared with ==, drawn, marginal)"""
    ok = tr["marginal"][:, None] | ((tr["lo"] <= eta) & (eta <= tr["hi"]))
    assert ok.all(), (what, np.argwhere(~ok)[:5])
    drawn = tr["tries"] > 0
    assert np.array_equal(eta[~drawn], tr["eta"][~drawn])
    exact = drawn & ~tr["marginal"] & (tr["lo"] == tr["hi"]).all(axis=1)
    assert np.array_equal(eta[exact], tr["eta"][exact]), what
    return int(exact.sum()), int(drawn.sum()), int(tr["marginal"].sum())


def _check_data(got, block, what):
    want, lo, hi, marginal = block[:4]
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    inside = nan | marginal | ((lo <= got) & (got <= hi))
    assert inside.all(), (what, np.argwhere(~inside)[:5])


@pytest.mark.parametrize("J", (1, 3, 8))
def test_truths_equal_the_restatement_on_every_shape(K, J):
    """T in {1, 63, 64, 65, 257} with every covariance kind x every box kind; the T = 65 cases run their trial numbers
    up to 2^32 - 1; the distance of the truths in the tails is printed"""
    flagged = 0
    worst = 0.0
    for T in sorted({T for T, _ in oc.TRUTH_SHAPES}):
        exact = drawn = 0
        for kinds, fit in oc.cases(J):
            mean, cov, lower, upper = fit
            first = oc.first_trial_of(T)
            _, eta, clipped = _draw(K, np.array([5.0]), None, np.zeros((J, 1)), fit, "poisson", T, SEED, STREAM, first)
            tr = oc.truths_mvn(mean, oc.truth_factor(cov), lower, upper, T, SEED, STREAM, first)
            assert not tr["exhausted"] and clipped == 0
            e, d, m = _check_truths(eta, tr, (T, J, kinds))
            exact, drawn, flagged = exact + e, drawn + d, flagged + m
            assert np.all((lower[None, :] <= eta) & (eta <= upper[None, :])), (T, J, kinds)
            dead = np.diagonal(cov) == 0.0
            assert np.array_equal(eta[:, dead], np.broadcast_to(mean[dead], (T, int(dead.sum()))))
            live = np.broadcast_to(~dead[None, :], eta.shape)
            if live.any():
                worst = max(worst, float(np.max(np.abs(eta - tr["eta"])[live] / np.spacing(np.abs(tr["eta"][live])))))
        print("T %d J %d: %d truths drawn, %d compared with ==" % (T, J, drawn, exact))
        assert drawn > 0 and exact >= 0.8 ** J * drawn, (T, J)
    print("J %d: %d marginal; the others within %.1f ulps" % (J, flagged, worst))
    assert flagged == 0          # this seed: every truth was compared (another seed rather than a wider window)


def _raw(K, lib, mu, sigma, R, fit, method, T, first, out, eta, status, seed=SEED, stream=0, J=None, B=None):
    h = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in fit]
    ptr = [None if a is None else a.ctypes.data for a in h]
    return lib.pisa_hip_fluctuate_linear_mvn(
        None if mu is None else mu.data_ptr(), None if sigma is None else sigma.data_ptr(),
        None if R is None else R.data_ptr(), R.shape[0] if J is None else J, ptr[0], ptr[1], ptr[2], ptr[3], method,
        mu.shape[0] if B is None else B, T, seed, stream, first, None if out is None else out.data_ptr(),
        None if eta is None else eta.data_ptr(), None if status is None else status.data_ptr(), None)


def test_a_box_no_candidate_enters_sets_the_status_word(K):
    """the one exhausted family, through the raw entry point (`kernels.fluctuate_linear_mvn` refuses such a box by its
    mass, and raises for the word): PISA_HIP_FLUCT_TRUTH_EXHAUSTED, every value inside the box and inside the
    restatement's window"""
    import torch

    from pisa_amd import _lib

    fit = oc.exhausting_case(3)
    mean, cov, lower, upper = fit
    T, B, first = 5, 2, 7
    mu, sigma, R = _dev(K, [5.0, 5.0]), _dev(K, [1.0, 1.0]), _dev(K, np.full((3, B), 0.1))
    out = torch.zeros((T, B), dtype=torch.float64, device=mu.device)
    eta = torch.zeros((T, 3), dtype=torch.float64, device=mu.device)
    status = torch.zeros(2, dtype=torch.int32, device=mu.device)
    assert _raw(K, _lib.lib(), mu, sigma, R, fit, 2, T, first, out, eta, status, seed=2 ** 64 - 3, stream=2 ** 32 - 1) == 0
    torch.cuda.synchronize()
    assert int(status.cpu().numpy()[0]) == _lib.FLUCT_TRUTH_EXHAUSTED == 1
    got = eta.cpu().numpy()
    assert np.all((lower[None, :] <= got) & (got <= upper[None, :]))
    tr = oc.truths_mvn(mean, oc.truth_factor(cov), lower, upper, T, 2 ** 64 - 3, 2 ** 32 - 1, first)
    assert tr["exhausted"] and np.all(tr["tries"] == oc.ATTEMPTS)
    assert np.all((tr["lo"] <= got) & (got <= tr["hi"]))
    assert np.isfinite(out.cpu().numpy()).all()
    with pytest.raises(ValueError, match="mass"):
        K.fluctuate_linear_mvn(mu, R, T, 1, mean, cov, lower, upper)


@pytest.mark.parametrize("method", oc.METHODS)
def test_data_equal_the_restatement_on_the_kernels_own_truths(K, method):
    """(T, B) in {1, 65, 257} x {1, 64, 65}, means and sigmas cycling through the palette (NaN and 0 included), J, the
    covariance kind and the box kind cycling; the T = 65 cases run their trial numbers up to 2^32 - 1"""
    entries = flagged = clipped_total = 0
    for i, (T, B) in enumerate(oc.DATA_SHAPES):
        mu0, sigma, R, fit = oc.data_case(T, B, i)
        first = oc.first_trial_of(T)
        got, eta, clipped = _draw(K, mu0, sigma, R, fit, method, T, SEED, STREAM, first)
        tr = oc.truths_mvn(fit[0], oc.truth_factor(fit[1]), fit[2], fit[3], T, SEED, STREAM, first)
        assert not tr["exhausted"] and not tr["marginal"].any()
        _check_truths(eta, tr, (T, B))
        block = tc.block(mu0, sigma, R, eta, method, SEED, STREAM, first)
        _check_data(got, block, (method, T, B))
        assert np.isnan(got[:, np.isnan(mu0)]).all()
        assert clipped == block[4], (T, B)
        live = ~np.isnan(block[0])
        entries, flagged = entries + int(live.sum()), flagged + int((block[3] & live).sum())
        clipped_total += clipped
    print("%s: %d entries, %d marginal, %d means clipped" % (method, entries, flagged, clipped_total))
    assert flagged <= MAX_MARGINAL_SHARE * entries
    assert flagged == 0
    assert clipped_total > 0


def test_identities(K):
    import torch

    B, T = 65, 257
    mu0, sigma = fm.palette_rows(B)
    R = tc.responses(3, B, mu0)
    diagonal = oc.case(3, "diagonal", "none")
    fit = oc.case(3, "dense", "two-sided")
    for method in oc.METHODS:
        d_sigma = None if method == "poisson" else _dev(K, sigma)
        # a diagonal covariance without a box: `kernels.fluctuate_linear`, data and truths, bit for bit
        for first in (0, 2 ** 32 - T):
            got = _draw(K, mu0, sigma, R, diagonal, method, T, SEED, STREAM, first)
            want = K.fluctuate_linear(_dev(K, mu0), _dev(K, R), T, SEED, np.sqrt(np.diagonal(diagonal[1])), diagonal[0],
                                      method=method, sigma=d_sigma, stream=STREAM, first_trial=first)
            assert np.array_equal(got[0], want["data"].cpu().numpy(), equal_nan=True)
            assert np.array_equal(got[1], want["eta"].cpu().numpy()) and got[2] == want["clipped"]
        # rows of a call split by first_trial are the rows of one call
        full = _draw(K, mu0, sigma, R, fit, method, T, SEED, STREAM)
        assert np.array_equal(_draw(K, mu0, sigma, R, fit, method, T, SEED, STREAM)[0], full[0], equal_nan=True)
        for n in (2, 3):
            parts = [_draw(K, mu0, sigma, R, fit, method, len(p), SEED, STREAM, first_trial=int(p[0]))
                     for p in np.array_split(np.arange(T), n)]
            assert np.array_equal(np.concatenate([p[0] for p in parts]), full[0], equal_nan=True), n
            assert np.array_equal(np.concatenate([p[1] for p in parts]), full[1]), n
            assert sum(p[2] for p in parts) == full[2]
        # fewer bins: the same truths and the same entries
        few = _draw(K, mu0[:17], sigma[:17], R[:, :17], fit, method, 5, SEED, STREAM)
        assert np.array_equal(few[0], full[0][:5, :17], equal_nan=True) and np.array_equal(few[1], full[1][:5])
        # another seed (either word of the key) or stream changes the truths
        for other in (_draw(K, mu0, sigma, R, fit, method, T, SEED + 1, STREAM),
                      _draw(K, mu0, sigma, R, fit, method, T, SEED, STREAM + 1),
                      _draw(K, mu0, sigma, R, fit, method, T, SEED + (1 << 32), STREAM)):
            assert np.all(other[1] != full[1])
    torch.cuda.synchronize()


def test_more_trials_than_one_pass(K):
    """2048 x 256 + 100 trials: more than the lanes of the largest grid, so the first lanes take a second trial; single
    rows against the restatement"""
    T, J = 2048 * 256 + 100, 2
    fit = oc.case(J, "tight", "two-sided")
    _, eta, _ = _draw(K, np.array([5.0]), None, np.zeros((J, 1)), fit, "poisson", T, 5)
    L = oc.truth_factor(fit[1])
    for t in (0, 99, 100, 2048 * 256 - 1, 2048 * 256, T - 1):
        _check_truths(eta[t:t + 1], oc.truths_mvn(fit[0], L, fit[2], fit[3], 1, 5, 0, first_trial=t), t)
    assert np.all((fit[2][None, :] <= eta) & (eta <= fit[3][None, :]))
    assert np.corrcoef(eta[:, 0], eta[:, 1])[0, 1] > 0.9


def test_closure_on_the_device(K):
    mean, cov, T, seed, stream = oc.closure_case()
    _, eta, _ = _draw(K, np.array([5.0]), None, np.zeros((3, 1)), (mean, cov, None, None), "poisson", T, seed, stream)
    oc.check_closure(eta, mean, cov)


def test_bad_arguments(K):
    import torch

    from pisa_amd import _lib

    B, J, T = 65, 3, 4
    mu0, sigma = fm.palette_rows(B)
    d_mu, d_sigma, d_R = _dev(K, mu0), _dev(K, sigma), _dev(K, tc.responses(J, B, mu0))
    good = oc.case(J, "dense", "two-sided")
    nan, inf = float("nan"), float("inf")

    def call(**kw):
        a = dict(mu=d_mu, response=d_R, n_trials=T, seed=SEED, mean=good[0], cov=good[1], lower=good[2], upper=good[3])
        a.update(kw)
        return K.fluctuate_linear_mvn(**a)

    def with_at(a, j, v):
        a = np.array(a, dtype=np.float64)
        a[j] = v
        return a

    dead_row = oc.covariance(J, "one-dead")
    dead_row[1, 0] = dead_row[0, 1] = 0.1
    library = (dict(mean=with_at(good[0], 2, nan)), dict(mean=with_at(good[0], 2, inf)),
               dict(lower=with_at(good[2], 0, nan)), dict(upper=with_at(good[3], 0, nan)),
               dict(lower=with_at(good[2], 0, 5.0), upper=with_at(good[3], 0, 4.0)),
               dict(mean=with_at(good[0], 1, good[3][1] + 0.01)),                     # the mean outside its box
               dict(cov=with_at(good[1], (0, 1), nan)), dict(cov=with_at(good[1], (2, 2), inf)),
               dict(cov=with_at(good[1], (1, 1), -1.0)), dict(cov=dead_row),
               dict(cov=np.full((J, J), 1.0), lower=None, upper=None),                # singular
               dict(n_trials=0), dict(first_trial=2 ** 32 - 3))
    for kw in library:
        with pytest.raises(_lib.PisaHipError) as err:
            call(**kw)
        assert err.value.status == -1, kw
    for kw in (dict(method="scaled_poisson", sigma=d_sigma), dict(method="gauss"), dict(method="binomial"),
               dict(response=d_R[:, :64]), dict(response=d_R.float()), dict(response=d_R.cpu()), dict(response=d_R[0]),
               dict(response=_dev(K, np.zeros((9, B)))), dict(mean=good[0][:2]), dict(lower=good[2][:2]),
               dict(cov=good[1][:2, :2]), dict(cov=good[1].ravel()),
               dict(mu=d_mu.float()), dict(seed=-1), dict(seed=2 ** 64), dict(stream=2 ** 32), dict(first_trial=-1),
               dict(method="gauss", sigma=d_sigma[:64]),
               dict(lower=good[0] - 0.1 * oc.stddevs(J), upper=good[0] + 0.1 * oc.stddevs(J))):       # 0.08 of the mass
        with pytest.raises(ValueError):
            call(**kw)
    # a mean without a draw is `fluctuate`'s error
    with pytest.raises(ValueError):
        call(mu=_dev(K, np.full(B, float("inf"))))
    # the raw entry point: nothing is launched, the outputs and the status words stay as they were
    lib = _lib.lib()
    out = torch.zeros((T, B), dtype=torch.float64, device=d_mu.device)
    eta = torch.zeros((T, J), dtype=torch.float64, device=d_mu.device)
    status = torch.zeros(2, dtype=torch.int32, device=d_mu.device)

    def raw(mu=d_mu, sg=d_sigma, R=d_R, fit=good, method=2, T=T, first=0, out=out, eta=eta, st=status, **kw):
        return _raw(K, lib, mu, sg, R, fit, method, T, first, out, eta, st, **kw)

    for kw in (dict(mu=None, B=B), dict(R=None, J=J), dict(out=None), dict(eta=None), dict(st=None),
               dict(fit=(None,) + good[1:]), dict(fit=(good[0], None) + good[2:]), dict(sg=None), dict(sg=None, method=3),
               dict(J=0), dict(J=9), dict(B=0), dict(T=0), dict(B=2 ** 31), dict(T=2 ** 31), dict(first=2 ** 32 - 3),
               dict(method=1), dict(method=-1), dict(method=4)):
        assert raw(**kw) == -1, kw
    for kw in library[:-2]:
        fit = (kw.get("mean", good[0]), kw.get("cov", good[1]), kw.get("lower", good[2]), kw.get("upper", good[3]))
        assert raw(fit=fit) == -1, kw
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any() and not eta.cpu().numpy().any() and not status.cpu().numpy().any()
    # and the good call: NULL bounds are no bounds, NULL sigma is fine for poisson
    assert raw(sg=None, method=0, fit=good[:2] + (None, None), first=2 ** 32 - 4) == 0
    torch.cuda.synchronize()
    want = K.fluctuate_linear_mvn(d_mu, d_R, T, SEED, good[0], good[1], first_trial=2 ** 32 - 4)
    assert np.array_equal(out.cpu().numpy(), want["data"].cpu().numpy(), equal_nan=True)
    assert np.array_equal(eta.cpu().numpy(), want["eta"].cpu().numpy())
    assert int(status.cpu().numpy()[0]) == 0


# ------------------------------------------------------------------ config pipeline
def test_the_observed_fit_on_the_config_pipeline(K):
    """a 3-point theta23 grid of example_hip.cfg with aeff_scale and delta_index in a bounded response; the observed map
    is one `pseudo_data` row of point 1 drawn with displaced truths.  `feldman_cousins(generator="device",
    nuisance="profiled")` and `"fitted"` are the loop over `pseudo_data` + `delta_metric`, whatever the chunk limit,
    and differ from the run with nuisance="fixed"; info["eta_observed"] holds `fit_observed`'s rows"""
    from pisa_amd.analysis import ensemble as en
    from pisa_amd.core.distribution_maker import DistributionMaker

    names = ("aeff_scale", "delta_index")
    dm = DistributionMaker("settings/pipeline/example_hip.cfg")
    for name in dm.params.free.names:
        if name != "theta23" and name not in names:
            dm.params.fix(name)
    dm.get_outputs(return_sum=True)
    th = dm.params["theta23"].value
    pts = en.grid_points(dm, {"theta23": [th * 0.8, th, th * 1.15]})
    metric = "llh"
    grid = en.TemplateGrid.from_maker(dm, pts, metric)
    test_vals = {"aeff_scale": (-0.05, 0.05), "delta_index": (-0.05, 0.05)}
    resp = en.NuisanceResponse.from_maker(dm, grid, names, test_vals, bounded=True)
    assert resp.bounded

    T, cl, seed = 200, (0.6827, 0.90), 77
    R_host = resp.response.cpu().numpy()
    displaced = np.array([0.06, 0.03])
    observed = K.fluctuate_linear(grid.hist[1], resp.response[1], 1, 5, np.zeros(2), displaced,
                                  stream=1)["data"].cpu().numpy()[0]
    fit = en.fit_observed(observed, grid, metric, resp, covariance=True)
    assert fit["eta"].shape == (3, 2) and not (fit["status"] & ~32).any() and not np.isnan(fit["cov"]).any()
    assert np.all(np.abs(fit["eta"][1] - displaced) < 5 * fit["sigma"][1]) and np.all(fit["eta"][1] != 0.0)
    fixed, _ = en.feldman_cousins(grid, metric, T, cl, seed, generator="device", response=resp)
    results = {}
    for nuisance in ("profiled", "fitted"):
        want = []
        entries = flagged = 0
        for k in range(3):
            d, eta = en.pseudo_data(grid, k, T, seed, generator="device", response=resp, nuisance=nuisance,
                                    observed=observed, return_truth=True)
            assert d.is_cuda and tuple(d.shape) == (T, grid.n_bins) and tuple(eta.shape) == (T, 2)
            eta = eta.cpu().numpy()
            _, _, _, lower, upper = en._truth_priors(resp, k)
            if nuisance == "profiled":
                assert np.array_equal(eta, np.tile(fit["eta"][k], (T, 1)))
            else:
                tr = oc.truths_mvn(fit["eta"][k], oc.truth_factor(fit["cov"][k]), lower, upper, T, seed, stream=k)
                _check_truths(eta, tr, k)
                flagged += int(tr["marginal"].sum())
                assert np.all((lower <= eta) & (eta <= upper))
                live = np.diagonal(fit["cov"][k]) > 0
                assert np.all(np.std(eta[:, live], axis=0) > 0.3 * fit["sigma"][k][live])
            block = tc.block(grid.host("hist")[k], None, R_host[k], eta, "poisson", seed, stream=k)
            _check_data(d.cpu().numpy(), block, (nuisance, k))
            entries, flagged = entries + block[0].size, flagged + int(block[3].sum())
            want.append(en.critical_values(en.delta_metric(d, grid, metric, k, response=resp), cl))
        print("%s: %d entries, %d marginal" % (nuisance, entries, flagged))
        assert flagged <= MAX_MARGINAL_SHARE * entries
        want = np.stack(want)
        kw = dict(generator="device", response=resp, nuisance=nuisance, observed=observed)
        crit, info = en.feldman_cousins(grid, metric, T, cl, seed, **kw)
        assert np.array_equal(crit, want) and np.all(crit[:, 1] >= crit[:, 0]) and np.all(crit >= 0)
        assert np.array_equal(info["eta_observed"], fit["eta"])
        assert ("cov_observed" in info) == (nuisance == "fitted")
        if nuisance == "fitted":
            assert np.array_equal(info["cov_observed"], fit["cov"])
        for chunk_bytes in (7 * 8 * grid.n_bins, 64 * 8 * grid.n_bins + 5):
            got, _ = en.feldman_cousins(grid, metric, T, cl, seed, chunk_bytes=chunk_bytes, **kw)
            assert np.array_equal(got, want)
        assert not np.array_equal(fixed, crit)
        results[nuisance] = crit
    assert not np.array_equal(results["profiled"], results["fitted"])
