"""Pseudo-data with drawn nuisance truths on the device (csrc/fluctuate_linear.hip: `pisa_hip_fluctuate_linear` through
`kernels.fluctuate_linear`) against the numpy restatement (tests/truth_cases.py), and `nuisance="prior"` of
pisa_amd/analysis/ensemble.py with `generator="device"` on example_hip.cfg.

A truth must lie inside the restatement's window: `==` where the accepted candidate came from the central branch of
AS 241 (at least 0.8 of the truths drawn, asserted), and in the tails the values a log within
`fluctuate_method_cases.LOG_ULPS` of numpy's reaches; a truth one of whose candidates lies that close to a box edge is
`marginal`, the share is held to 1e-5 and at the seed of the shapes the restatement marks none (asserted here and,
without a GPU, in tests/test_host_truth.py).  The data are compared on the kernel's OWN truths, after that check: every
count `==` wherever the restatement does not mark it marginal, with the same cap and the same "this seed marks none".
"""
import numpy as np
import pytest

from tests import fluctuate_method_cases as fm
from tests import truth_cases as tc

pytestmark = pytest.mark.gpu

SEED, STREAM = tc.SEED, tc.STREAM
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


def _draw(K, mu0, sigma, R, pri, method, n_trials, seed, stream=0, first_trial=0):
    """(data, eta, clipped) as host arrays"""
    out = K.fluctuate_linear(_dev(K, mu0), _dev(K, R), n_trials, seed, pri[0], pri[1], pri[2], pri[3], method=method,
                             sigma=None if method == "poisson" else _dev(K, sigma), stream=stream,
                             first_trial=first_trial)
    assert out["data"].is_cuda and tuple(out["data"].shape) == (n_trials, len(mu0))
    assert out["eta"].is_cuda and tuple(out["eta"].shape) == (n_trials, len(pri[0]))
    return out["data"].cpu().numpy(), out["eta"].cpu().numpy(), out["clipped"]


def _check_truths(eta, tr, what):
    """the kernel's truths against the restatement's dict -> (compared with ==, drawn, marginal)"""
    ok = tr["marginal"] | ((tr["lo"] <= eta) & (eta <= tr["hi"]))
    assert ok.all(), (what, np.argwhere(~ok)[:5])
    drawn = tr["tries"] > 0
    assert np.array_equal(eta[~drawn], tr["eta"][~drawn])
    return int(np.sum(drawn & (tr["lo"] == tr["hi"]))), int(drawn.sum()), int(tr["marginal"].sum())


def _check_data(got, block, what):
    want, lo, hi, marginal = block[:4]
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    inside = nan | marginal | ((lo <= got) & (got <= hi))
    assert inside.all(), (what, np.argwhere(~inside)[:5])


def test_truths_equal_the_restatement_on_every_shape(K):
    """(T, J) in {1, 63, 64, 65, 257} x {1, 3, 8} with every kind of box; the T = 65 cases run their trial numbers up to
    2^32 - 1; the distance of the truths in the tails is printed"""
    exact = drawn = flagged = 0
    worst = 0.0
    for T, J in tc.TRUTH_SHAPES:
        for kind in tc.KINDS:
            pri = tc.priors(J, kind)
            first = tc.first_trial_of(T)
            _, eta, clipped = _draw(K, np.array([5.0]), None, np.zeros((J, 1)), pri, "poisson", T, SEED, STREAM, first)
            tr = tc.truths(*pri, T, SEED, STREAM, first)
            assert not tr["exhausted"] and clipped == 0
            e, d, m = _check_truths(eta, tr, (T, J, kind))
            exact, drawn, flagged = exact + e, drawn + d, flagged + m
            assert np.all((pri[2][None, :] <= eta) & (eta <= pri[3][None, :]) | (pri[0] == 0.0)[None, :])
            live = tr["tries"] > 0
            if live.any():
                worst = max(worst, float(np.max(np.abs(eta - tr["eta"])[live] / np.spacing(np.abs(tr["eta"][live])))))
    print("%d truths drawn, %d compared with ==, %d marginal; the others within %.1f ulps" % (drawn, exact, flagged, worst))
    assert flagged <= MAX_MARGINAL_SHARE * drawn
    assert flagged == 0          # this seed: every truth was compared (another seed rather than a wider window)
    assert exact >= 0.8 * drawn


@pytest.mark.parametrize("method", tc.METHODS)
def test_data_equal_the_restatement_on_the_kernels_own_truths(K, method):
    """(T, B) in {1, 65, 257} x {1, 63, 64, 65, 257}, means and sigmas cycling through the palette (NaN and 0 included), J
    and the kind of box cycling; the T = 65 cases run their trial numbers up to 2^32 - 1"""
    entries = flagged = clipped_total = 0
    for i, (T, B) in enumerate(tc.DATA_SHAPES):
        mu0, sigma, R, pri = tc.data_case(T, B, i)
        first = tc.first_trial_of(T)
        got, eta, clipped = _draw(K, mu0, sigma, R, pri, method, T, SEED, STREAM, first)
        _check_truths(eta, tc.truths(*pri, T, SEED, STREAM, first), (T, B))
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
    zero = (np.zeros(3), np.zeros(3), None, None)
    pri = tc.priors(3, "mixed")
    for method in tc.METHODS:
        # all scales (and shifts) 0: `kernels.fluctuate`, bit for bit
        got, eta, clipped = _draw(K, mu0, sigma, R, zero, method, T, SEED, STREAM)
        want = K.fluctuate(_dev(K, mu0), T, SEED, method=method, sigma=None if method == "poisson" else _dev(K, sigma),
                           stream=STREAM).cpu().numpy()
        assert np.array_equal(got, want, equal_nan=True) and not eta.any() and clipped == 0
        # rows of a call split by first_trial are the rows of one call
        full = _draw(K, mu0, sigma, R, pri, method, T, SEED, STREAM)
        assert np.array_equal(_draw(K, mu0, sigma, R, pri, method, T, SEED, STREAM)[0], full[0], equal_nan=True)
        for n in (2, 3):
            parts = [_draw(K, mu0, sigma, R, pri, method, len(p), SEED, STREAM, first_trial=int(p[0]))
                     for p in np.array_split(np.arange(T), n)]
            assert np.array_equal(np.concatenate([p[0] for p in parts]), full[0], equal_nan=True), n
            assert np.array_equal(np.concatenate([p[1] for p in parts]), full[1]), n
            assert sum(p[2] for p in parts) == full[2]
        # fewer bins: the same truths and the same entries
        few = _draw(K, mu0[:17], sigma[:17], R[:, :17], pri, method, 5, SEED, STREAM)
        assert np.array_equal(few[0], full[0][:5, :17], equal_nan=True) and np.array_equal(few[1], full[1][:5])
        # another seed (either word of the key) or stream changes truths and data
        live = ~np.isnan(full[0][0]) & (mu0 >= 9.0)
        for other in (_draw(K, mu0, sigma, R, pri, method, T, SEED + 1, STREAM),
                      _draw(K, mu0, sigma, R, pri, method, T, SEED, STREAM + 1),
                      _draw(K, mu0, sigma, R, pri, method, T, SEED + (1 << 32), STREAM)):
            assert np.mean(other[0][:, live] != full[0][:, live]) > 0.3
            assert np.all(other[1][:, :3] != full[1][:, :3])
    torch.cuda.synchronize()


def test_more_entries_than_one_pass(K):
    """4100 x 257 entries of gauss+poisson: more than the 2048 x 256 lanes of the largest grid, so every lane strides
    (entry 524 288 is in trial 2040); single rows against the restatement on the kernel's truths"""
    T, B, seed, method = 4100, 257, 5, "gauss+poisson"
    mu0, sigma = fm.palette_rows(B)
    R = tc.responses(8, B, mu0)
    pri = tc.priors(8, "mixed")
    got, eta, clipped = _draw(K, mu0, sigma, R, pri, method, T, seed)
    assert np.isfinite(got[:, ~np.isnan(mu0)]).all() and np.isnan(got[:, np.isnan(mu0)]).all()
    assert clipped == int(tc.means(mu0, R, eta)[1].sum())
    rows = (0, 2039, 2040, 2041, 4099)
    for t in rows:
        _check_truths(eta[t:t + 1], tc.truths(*pri, 1, seed, 0, first_trial=t), t)
        block = tc.block(mu0, sigma, R, eta[t:t + 1], method, seed, 0, first_trial=t)
        assert not block[3].any()
        assert np.array_equal(got[t], block[0][0], equal_nan=True), t
    assert not np.array_equal(got[rows[1]], got[rows[2]], equal_nan=True)


def test_clipping_is_counted_and_is_no_error(K):
    """a response that drives two chosen bins negative in every trial"""
    B, T = 65, 63
    mu0 = np.full(B, 20.0)
    R = np.zeros((2, B))
    R[0, 7], R[1, 40] = -30.0, 50.0
    pri = (np.array([0.01, 0.01]), np.array([1.0, -1.0]), None, None)          # eta near (+1, -1)
    for method in tc.METHODS:
        got, eta, clipped = _draw(K, mu0, np.full(B, 2.0), R, pri, method, T, SEED)      # (no error: `_draw` returned)
        block = tc.block(mu0, np.full(B, 2.0), R, eta, method, SEED)
        assert clipped == block[4] == 2 * T
        _check_data(got, block, method)
        if method == "poisson":
            assert np.all(got[:, [7, 40]] == 0.0) and np.all(got[:, 8] > 0.0)


def test_bad_arguments(K):
    import torch

    from pisa_amd import _lib

    B, J, T = 65, 3, 4
    mu0, sigma = fm.palette_rows(B)
    d_mu, d_sigma, d_R = _dev(K, mu0), _dev(K, sigma), _dev(K, tc.responses(J, B, mu0))
    good = tc.priors(J, "two-sided")
    nan, inf = float("nan"), float("inf")

    def call(**kw):
        a = dict(mu=d_mu, response=d_R, n_trials=T, seed=SEED, scale=good[0], shift=good[1], lower=good[2], upper=good[3])
        a.update(kw)
        return K.fluctuate_linear(**a)

    def with_at(a, j, v):
        a = np.array(a, dtype=np.float64)
        a[j] = v
        return a

    for kw in (dict(scale=with_at(good[0], 1, nan)), dict(scale=with_at(good[0], 1, -1.0)),
               dict(scale=with_at(good[0], 1, inf)), dict(shift=with_at(good[1], 2, nan)),
               dict(shift=with_at(good[1], 2, inf)), dict(lower=with_at(good[2], 0, nan)),
               dict(upper=with_at(good[3], 0, nan)), dict(lower=with_at(good[2], 0, 5.0), upper=with_at(good[3], 0, 4.0)),
               dict(n_trials=0), dict(first_trial=2 ** 32 - 3)):
        with pytest.raises(_lib.PisaHipError) as err:
            call(**kw)
        assert err.value.status == -1, kw
    for kw in (dict(method="scaled_poisson", sigma=d_sigma), dict(method="gauss"), dict(method="binomial"),
               dict(response=d_R[:, :64]), dict(response=d_R.float()), dict(response=d_R.cpu()), dict(response=d_R[0]),
               dict(response=_dev(K, np.zeros((9, B)))), dict(scale=good[0][:2]), dict(lower=good[2][:2]),
               dict(mu=d_mu.float()), dict(seed=-1), dict(seed=2 ** 64), dict(stream=2 ** 32), dict(first_trial=-1),
               dict(method="gauss", sigma=d_sigma[:64]),
               dict(lower=good[1] + 0.7 * good[0], upper=None)):               # sf(0.7) = 0.24 of the mass
        with pytest.raises(ValueError):
            call(**kw)
    assert call(lower=good[1] + 0.6 * good[0], upper=None)["eta"].shape == (T, J)       # sf(0.6) = 0.27: drawn
    # a mean without a draw is `fluctuate`'s error
    with pytest.raises(ValueError):
        call(mu=_dev(K, np.full(B, float("inf"))))
    with pytest.raises(ValueError):
        call(method="gauss", sigma=_dev(K, np.full(B, -1.0)))
    # the raw entry point: nothing is launched, the outputs and the status words stay as they were
    lib = _lib.lib()
    out = torch.full((T, B), -1.0, dtype=torch.float64, device=d_mu.device)
    eta = torch.full((T, J), -1.0, dtype=torch.float64, device=d_mu.device)
    status = torch.zeros(2, dtype=torch.int32, device=d_mu.device)
    h = [np.ascontiguousarray(a, dtype=np.float64) for a in good]
    hp = [a.ctypes.data for a in h]
    p_mu, p_sg, p_R, p_out, p_eta, p_st = (x.data_ptr() for x in (d_mu, d_sigma, d_R, out, eta, status))

    def raw(mu=p_mu, sg=p_sg, R=p_R, J=J, scale=hp[0], shift=hp[1], lower=hp[2], upper=hp[3], method=2, B=B, T=T,
            first=0, out=p_out, eta=p_eta, st=p_st):
        return lib.pisa_hip_fluctuate_linear(mu, sg, R, J, scale, shift, lower, upper, method, B, T, SEED, 0, first, out,
                                             eta, st, None)

    for kw in (dict(mu=None), dict(R=None), dict(out=None), dict(eta=None), dict(st=None), dict(scale=None),
               dict(shift=None), dict(sg=None), dict(sg=None, method=3), dict(J=0), dict(J=9), dict(B=0), dict(T=0),
               dict(B=2 ** 31), dict(T=2 ** 31), dict(first=2 ** 32 - 3), dict(method=1), dict(method=-1),
               dict(method=4)):
        assert raw(**kw) == -1, kw
    bad = np.array([1.0, nan, 1.0])
    assert raw(scale=bad.ctypes.data) == -1 and raw(shift=bad.ctypes.data) == -1 and raw(lower=bad.ctypes.data) == -1
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -1.0) and np.all(eta.cpu().numpy() == -1.0) and not status.cpu().numpy().any()
    # and the good call: NULL bounds are no bounds, NULL sigma is fine for poisson
    assert raw(sg=None, method=0, lower=None, upper=None, first=2 ** 32 - 4) == 0
    torch.cuda.synchronize()
    want = K.fluctuate_linear(d_mu, d_R, T, SEED, good[0], good[1], first_trial=2 ** 32 - 4)
    assert np.array_equal(out.cpu().numpy(), want["data"].cpu().numpy(), equal_nan=True)
    assert np.array_equal(eta.cpu().numpy(), want["eta"].cpu().numpy())
    assert int(status.cpu().numpy()[0]) == 0


# ------------------------------------------------------------------ config pipeline
def test_drawn_truths_on_the_config_pipeline(K):
    """a 3-point theta23 grid of example_hip.cfg with aeff_scale and delta_index in a bounded response:
    `feldman_cousins(generator="device", nuisance="prior")` is the loop over `pseudo_data` + `delta_metric`, whatever
    the chunk limit, and differs from the run with nuisance="fixed"; aeff_scale has a uniform prior and stays at the
    point's value, delta_index is drawn from its Gaussian prior inside its range"""
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
    assert resp.bounded and np.any(resp.inv_prior_sigma > 0)

    T, cl, seed = 200, (0.6827, 0.90), 77
    R_host = resp.response.cpu().numpy()
    data, want = [], []
    entries = flagged = 0
    for k in range(3):
        d, eta = en.pseudo_data(grid, k, T, seed, generator="device", response=resp, nuisance="prior", return_truth=True)
        assert d.is_cuda and tuple(d.shape) == (T, grid.n_bins) and tuple(eta.shape) == (T, 2)
        _, scale, shift, lower, upper = en._truth_priors(resp, k)
        tr = tc.truths(scale, shift, lower, upper, T, seed, stream=k)
        eta = eta.cpu().numpy()
        _check_truths(eta, tr, k)
        assert np.all((lower <= eta) & (eta <= upper)) and np.all(eta[:, scale == 0.0] == 0.0)
        assert np.all(np.std(eta[:, scale > 0.0], axis=0) > 0.3 * scale[scale > 0.0])
        block = tc.block(grid.host("hist")[k], None, R_host[k], eta, "poisson", seed, stream=k)
        _check_data(d.cpu().numpy(), block, k)
        entries, flagged = entries + block[0].size, flagged + int(block[3].sum()) + int(tr["marginal"].sum())
        data.append(d)
        want.append(en.critical_values(en.delta_metric(d, grid, metric, k, response=resp), cl))
    print("%d entries, %d marginal" % (entries, flagged))
    assert flagged <= MAX_MARGINAL_SHARE * entries
    want = np.stack(want)
    crit, info = en.feldman_cousins(grid, metric, T, cl, seed, generator="device", response=resp, nuisance="prior")
    assert np.array_equal(crit, want) and np.all(crit[:, 1] >= crit[:, 0]) and np.all(crit >= 0)
    for chunk_bytes in (7 * 8 * grid.n_bins, 64 * 8 * grid.n_bins + 5):
        got, _ = en.feldman_cousins(grid, metric, T, cl, seed, generator="device", response=resp, nuisance="prior",
                                    chunk_bytes=chunk_bytes)
        assert np.array_equal(got, want)
    fixed, _ = en.feldman_cousins(grid, metric, T, cl, seed, generator="device", response=resp)
    assert not np.array_equal(fixed, crit)
    again, _ = en.feldman_cousins(grid, metric, T, cl, seed, generator="device", response=resp, nuisance="fixed")
    assert np.array_equal(again, fixed)
    assert not np.array_equal(data[0].cpu().numpy(), en.pseudo_data(grid, 0, T, seed, generator="device").cpu().numpy())
