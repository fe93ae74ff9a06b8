"""The fluctuation methods of the device generator on the device (csrc/fluctuate.hip: `pisa_hip_fluctuate` through
`kernels.fluctuate`) against their numpy restatement (tests/fluctuate_method_cases.py), and `method=` of
pisa_amd/analysis/ensemble.py with `generator="device"` on example_hip.cfg.

Counts (poisson, gauss+poisson, scaled_poisson) are compared with `==` on every entry the restatement does not mark
`marginal`; the marginal share is held to 1e-5 and at the seed of the shapes the restatement marks none (asserted here
and, without a GPU, in tests/test_host_fluctuate_methods.py), so there every entry is compared -- but for the bins of a
scaled_poisson row whose Poisson mean lies above 1e6, which `fluctuate_method_cases.wide_window` explains.  A gauss
entry must lie inside the restatement's [lo, hi]: `==` in the central branch of AS 241 (at least 0.8 of the entries,
asserted), and in the tails the values reachable from a log within 4 ulps of numpy's.  The device library's log is
specified to 1 ulp like glibc's; that the two stay within 4 ulps of each other is a supposition this test checks, and
`test_the_deviate_itself` prints the distance it finds.
"""
import numpy as np
import pytest

from tests import fluctuate_cases as fc
from tests import fluctuate_method_cases as fm

pytestmark = pytest.mark.gpu

SEED, STREAM = 1, 3
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


def _draw(K, mu, sigma, method, n_trials, seed, stream=0, first_trial=0, want_status=0):
    """the draws as a host array; the status word is read here (rows with a sigma or a mean without a draw set it)"""
    import torch

    status = torch.zeros(1, dtype=torch.int32, device=K.device())
    out = K.fluctuate(_dev(K, mu), n_trials, seed, method=method, sigma=None if sigma is None else _dev(K, sigma),
                      stream=stream, first_trial=first_trial, status=status)
    assert out.is_cuda and tuple(out.shape) == (n_trials, len(mu))
    assert int(status.item()) == want_status, (method, int(status.item()))
    return out.cpu().numpy()


def _check(got, block, what):
    """a kernel block against the restatement's (values, lo, hi, marginal) -> the number of entries compared with =="""
    want, lo, hi, marginal = block
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    inside = nan | marginal | ((lo <= got) & (got <= hi))
    assert inside.all(), (what, np.argwhere(~inside)[:5])
    return int(np.sum(~nan & ~marginal & (lo == hi)))


@pytest.mark.parametrize("method", fm.METHODS)
def test_kernel_equals_the_restatement_on_every_shape(K, method):
    """(T, B) in {1, 2, 65, 257} x {1, 63, 64, 65, 257}, means and sigmas cycling through the palette (NaN, 0 and
    sigma = 0 included); the (65, 65) case runs its trial numbers up to the last one the counter word holds"""
    from pisa_amd import _lib

    entries = flagged = exact = live = 0
    for T in (1, 2, 65, 257):
        for B in (1, 63, 64, 65, 257):
            mu, sigma = fm.palette_rows(B)
            first = 2 ** 32 - T if (T, B) == (65, 65) else 0
            block = fm.block(mu, sigma, method, T, SEED, STREAM, first)
            want, marginal = block[0], block[3]
            refused = bool(np.any(np.isnan(want[0]) & ~np.isnan(mu)))      # (sigma == 0 with mu != 0, lam > 2^52)
            assert refused == (method == "scaled_poisson" and B > 1)
            got = _draw(K, mu, None if method == "poisson" else sigma, method, T, SEED, STREAM, first,
                        _lib.ERR_NEGATIVE if refused else 0)
            assert np.isnan(got[:, np.isnan(mu)]).all(), (T, B)
            if method != "gauss":
                assert np.all(got[:, mu == 0.0] == 0.0)
            else:
                assert np.all(got[:, sigma == 0.0] == mu[sigma == 0.0][None, :])
            exact += _check(got, block, (method, T, B))
            narrow = ~fm.wide_window(mu, sigma, method)[None, :] & ~np.isnan(want)
            entries, flagged = entries + int(narrow.sum()), flagged + int((marginal & narrow).sum())
            live += int(np.sum(~np.isnan(want)))
    print("%s: %d entries, %d marginal, %d of %d compared with ==" % (method, entries, flagged, exact, live))
    assert flagged <= MAX_MARGINAL_SHARE * entries
    assert flagged == 0          # this seed: every entry was compared (another seed rather than a wider window)
    if method == "gauss":
        assert exact >= 0.8 * live
    if method == "poisson":
        assert exact == live


def test_the_deviate_itself(K):
    """mu = 0 and sigma = 1 give z itself: `==` the restatement in the central branch, and in the tails `==` the chain's
    value at a t within LOG_ULPS ulps of numpy's -log; the distance found is printed (DESIGN.md quotes it)"""
    T, B = 257, 257
    got = _draw(K, np.zeros(B), np.ones(B), "gauss", T, SEED, STREAM)
    t, b = np.meshgrid(np.arange(T), np.arange(B), indexing="ij")
    cand = fm.normal_candidates(fm.deviates(t, b, STREAM, SEED))
    own = cand[fm.LOG_ULPS]
    hit = cand == got[None]
    steps = np.abs(np.arange(-fm.LOG_ULPS, fm.LOG_ULPS + 1))[:, None, None]
    dist = np.where(hit, steps, 99).min(axis=0)               # (99: no t within LOG_ULPS gives the kernel's value)
    ulps = np.abs(got - own) / np.spacing(np.abs(own))
    central = np.all(cand == own[None], axis=0)
    print("%d entries, %d in the tails: -log within %d ulps of numpy's, z within %.1f ulps; %d tail entries differ"
          % (got.size, int((~central).sum()), int(dist.max()), float(ulps.max()), int(np.sum(got != own))))
    assert hit.any(axis=0).all(), "the kernel's log is more than %d ulps from numpy's: z is %.1f ulps off" % (
        fm.LOG_ULPS, float(ulps.max()))
    assert np.array_equal(got[central], own[central]) and central.mean() >= 0.8
    assert abs(float(got.mean())) <= 5.0 / np.sqrt(got.size) and abs(float(got.var()) - 1.0) <= 5.0 * np.sqrt(2.0 / got.size)


def test_more_entries_than_one_pass(K):
    """4100 x 257 entries of gauss+poisson: more than the 2048 x 256 lanes of the largest grid, so every lane strides
    (entry 524 288 is in trial 2040); single rows against the restatement"""
    T, B, seed, method = 4100, 257, 5, "gauss+poisson"
    mu, sigma = fm.palette_rows(B)
    got = _draw(K, mu, sigma, method, T, seed)
    assert np.isfinite(got[:, ~np.isnan(mu)]).all() and np.isnan(got[:, np.isnan(mu)]).all()
    rows = (0, 2039, 2040, 2041, 4099)
    for t in rows:
        block = fm.block(mu, sigma, method, 1, seed, 0, first_trial=t)
        assert not block[3].any()
        assert np.array_equal(got[t], block[0][0], equal_nan=True), t
    assert not np.array_equal(got[rows[1]], got[rows[2]], equal_nan=True)


@pytest.mark.parametrize("method", fm.METHODS[1:])
def test_placement_seed_and_stream(K, method):
    import torch

    from pisa_amd import _lib

    T = 257
    mu, sigma = fm.palette_rows(65)
    st = _lib.ERR_NEGATIVE if method == "scaled_poisson" else 0
    full = _draw(K, mu, sigma, method, T, SEED, STREAM, want_status=st)
    assert np.array_equal(_draw(K, mu, sigma, method, T, SEED, STREAM, want_status=st), full, equal_nan=True)
    for n in (2, 3):
        parts = np.array_split(np.arange(T), n)
        got = np.concatenate([_draw(K, mu, sigma, method, len(p), SEED, STREAM, first_trial=int(p[0]), want_status=st)
                              for p in parts])
        assert np.array_equal(got, full, equal_nan=True), n
    top = _draw(K, mu, sigma, method, 5, SEED, STREAM, first_trial=2 ** 32 - 5, want_status=st)
    assert np.array_equal(top[3:], _draw(K, mu, sigma, method, 2, SEED, STREAM, first_trial=2 ** 32 - 2, want_status=st),
                          equal_nan=True)
    # fewer bins: the same entries; an `out` given by the caller is filled and returned
    few = _draw(K, mu[:17], sigma[:17], method, 5, SEED, STREAM, want_status=st)
    assert np.array_equal(few, full[:5, :17], equal_nan=True)
    out = torch.full((5, 65), -1.0, dtype=torch.float64, device=K.device())
    status = torch.zeros(1, dtype=torch.int32, device=K.device())
    assert K.fluctuate(_dev(K, mu), 5, SEED, method=method, sigma=_dev(K, sigma), stream=STREAM, out=out, status=status) is out
    assert np.array_equal(out.cpu().numpy(), full[:5], equal_nan=True)
    live = ~np.isnan(full[0]) & (mu >= 9.0) & (sigma > 0)
    for other in (_draw(K, mu, sigma, method, T, SEED + 1, STREAM, want_status=st),
                  _draw(K, mu, sigma, method, T, SEED, STREAM + 1, want_status=st),
                  _draw(K, mu, sigma, method, T, SEED + (1 << 32), STREAM, want_status=st)):      # (the key's second word)
        assert np.mean(other[:, live] != full[:, live]) > 0.3
        assert np.array_equal(np.isnan(other), np.isnan(full))


def test_status_and_argument_checks(K):
    import torch

    from pisa_amd import _lib

    mu = fc.palette_row(65)
    mu[0] = 2.0
    with np.errstate(invalid="ignore"):
        sigma = 0.5 * np.sqrt(mu)                            # (every method draws every bin of this row)
    keep = np.arange(65) != 7
    for method in fm.METHODS[1:]:
        clean = _draw(K, mu, sigma, method, 4, SEED)
        for bad_mu, bad_sigma in ((None, -1.0), (None, float("nan")), (None, float("inf")), (-1.0, None),
                                  (float("inf"), None)):
            m, s = mu.copy(), sigma.copy()
            if bad_mu is not None:
                m[7] = bad_mu
            if bad_sigma is not None:
                s[7] = bad_sigma
            refused = not (bad_mu is not None and (method == "gauss" or (method == "gauss+poisson" and bad_mu < 0)))
            if not refused:              # gauss takes any mean; gauss+poisson clips a negative g
                got = _draw(K, m, s, method, 4, SEED)
                assert not np.isnan(got[:, 7]).any()
                continue
            with pytest.raises(ValueError):
                K.fluctuate(_dev(K, m), 4, SEED, method=method, sigma=_dev(K, s))
            # the entry itself is NaN, its neighbours are drawn, the status word holds the code
            got = _draw(K, m, s, method, 4, SEED, want_status=_lib.ERR_NEGATIVE)
            assert np.isnan(got[:, 7]).all() and np.array_equal(got[:, keep], clean[:, keep], equal_nan=True)
    big = _draw(K, np.array([2.0 ** 52] * 64), np.array([2.0 ** 50] * 64), "gauss+poisson", 4, SEED,
                want_status=_lib.ERR_NEGATIVE)                                         # g > 2^52 -> NaN
    want = fm.block(np.array([2.0 ** 52] * 64), np.array([2.0 ** 50] * 64), "gauss+poisson", 4, SEED)[0]
    assert np.array_equal(np.isnan(big), np.isnan(want)) and np.isnan(big).any() and not np.isnan(big).all()
    d_mu, d_sigma = _dev(K, mu), _dev(K, sigma)
    for call in (lambda: K.fluctuate(d_mu, 4, SEED, method="gauss"),                             # no sigma
                 lambda: K.fluctuate(d_mu, 4, SEED, method="gauss", sigma=d_sigma[:64]),
                 lambda: K.fluctuate(d_mu, 4, SEED, method="gauss", sigma=d_sigma.float()),
                 lambda: K.fluctuate(d_mu, 4, SEED, method="gauss", sigma=d_sigma.cpu()),
                 lambda: K.fluctuate(d_mu.reshape(5, 13), 4, SEED), lambda: K.fluctuate(d_mu.float(), 4, SEED),
                 lambda: K.fluctuate(d_mu, 4, -1), lambda: K.fluctuate(d_mu, 4, 2 ** 64),
                 lambda: K.fluctuate(d_mu, 4, SEED, stream=2 ** 32), lambda: K.fluctuate(d_mu, 4, SEED, first_trial=-1),
                 lambda: K.fluctuate(d_mu, 4, SEED, out=torch.empty((4, 64), dtype=torch.float64, device=d_mu.device))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match='Map fluctuation method "binomial" not recognized! Valid choices are'):
        K.fluctuate(d_mu, 4, SEED, method="binomial", sigma=d_sigma)
    assert np.array_equal(K.fluctuate(d_mu, 4, SEED, method=" Gauss + Poisson ", sigma=d_sigma).cpu().numpy(),
                          _draw(K, mu, sigma, "gauss+poisson", 4, SEED), equal_nan=True)
    for call in (lambda: K.fluctuate(d_mu, 0, SEED), lambda: K.fluctuate(d_mu, 4, SEED, first_trial=2 ** 32 - 3)):
        with pytest.raises(_lib.PisaHipError) as err:
            call()
        assert err.value.status == -1
    # the raw entry point: NULLs, bad sizes, an unknown method and a missing sigma are refused before any device access
    lib = _lib.lib()
    out = torch.empty((4, 65), dtype=torch.float64, device=d_mu.device)
    status = torch.zeros(1, dtype=torch.int32, device=d_mu.device)
    p_mu, p_sg, p_out, p_st = d_mu.data_ptr(), d_sigma.data_ptr(), out.data_ptr(), status.data_ptr()
    assert lib.pisa_hip_fluctuate(None, p_sg, 2, 65, 4, 1, 0, 0, p_out, p_st, None) == -1
    assert lib.pisa_hip_fluctuate(p_mu, p_sg, 2, 65, 4, 1, 0, 0, None, p_st, None) == -1
    assert lib.pisa_hip_fluctuate(p_mu, p_sg, 2, 65, 4, 1, 0, 0, p_out, None, None) == -1
    assert lib.pisa_hip_fluctuate(p_mu, p_sg, 2, 0, 4, 1, 0, 0, p_out, p_st, None) == -1
    assert lib.pisa_hip_fluctuate(p_mu, p_sg, 2, 65, 0, 1, 0, 0, p_out, p_st, None) == -1
    assert lib.pisa_hip_fluctuate(p_mu, p_sg, 2, 2 ** 31, 4, 1, 0, 0, p_out, p_st, None) == -1
    assert lib.pisa_hip_fluctuate(p_mu, p_sg, 2, 65, 4, 1, 0, 2 ** 32 - 3, p_out, p_st, None) == -1
    for method in (-1, 4):
        assert lib.pisa_hip_fluctuate(p_mu, p_sg, method, 65, 4, 1, 0, 0, p_out, p_st, None) == -1
    for method in (1, 2, 3):
        assert lib.pisa_hip_fluctuate(p_mu, None, method, 65, 4, 1, 0, 0, p_out, p_st, None) == -1
    assert lib.pisa_hip_fluctuate(p_mu, None, 0, 65, 4, 1, 0, 2 ** 32 - 4, p_out, p_st, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), K.poisson_fluctuate(d_mu, 4, 1, first_trial=2 ** 32 - 4).cpu().numpy(), equal_nan=True)
    assert int(status.item()) == 0


# ------------------------------------------------------------------ config pipeline
def test_methods_with_the_device_generator_on_the_config_pipeline(K):
    """the 3 x 3 grid over theta23 x deltam31 of example_hip.cfg (its hist stage has error_method = sumw2), mcllh_eff,
    gauss+poisson: `pseudo_data(generator="device", method=...)` is the restatement's block of the template row and its
    standard deviations; `feldman_cousins` is `critical_values(delta_metric(...))` of those tensors, whatever the chunk
    limit; method="poisson" is the call without the argument"""
    from pisa_amd.analysis import ensemble as en
    from pisa_amd.core.distribution_maker import DistributionMaker

    free = ("theta23", "deltam31")
    dm = DistributionMaker("settings/pipeline/example_hip.cfg")
    for name in dm.params.free.names:
        if name not in free:
            dm.params.fix(name)
    dm.get_outputs(return_sum=True)
    th, m31 = dm.params["theta23"].value, dm.params["deltam31"].value
    pts = en.grid_points(dm, {"theta23": [th * 0.8, th, th * 1.15], "deltam31": [m31 * 0.85, m31, m31 * 1.2]})
    metric, method = "mcllh_eff", "gauss+poisson"
    grid = en.TemplateGrid.from_maker(dm, pts, metric)
    assert grid.hist.is_cuda and len(grid) == 9 and np.any(grid.host("sumw2") > 0)

    T, cl, seed = 200, (0.6827, 0.90), 77
    entries = flagged = 0
    data = []
    for k in range(9):
        d = en.pseudo_data(grid, k, T, seed, generator="device", method=method)
        assert d.is_cuda and tuple(d.shape) == (T, grid.n_bins)
        block = fm.block(grid.host("hist")[k], np.sqrt(grid.host("sumw2")[k]), method, T, seed, stream=k)
        _check(d.cpu().numpy(), block, k)
        entries, flagged = entries + block[0].size, flagged + int(block[3].sum())
        data.append(d)
    print("%d entries, %d marginal" % (entries, flagged))
    assert flagged <= MAX_MARGINAL_SHARE * entries
    assert not np.array_equal(data[0].cpu().numpy(), data[1].cpu().numpy())
    assert not np.array_equal(data[0].cpu().numpy(), en.pseudo_data(grid, 0, T, seed, generator="device").cpu().numpy())
    want = np.stack([en.critical_values(en.delta_metric(data[k], grid, metric, k), cl) for k in range(9)])
    crit = en.feldman_cousins(grid, metric, T, cl, seed, generator="device", method=method)
    assert np.array_equal(crit, want) and np.all(crit[:, 1] >= crit[:, 0]) and np.all(crit >= 0)
    for chunk_bytes in (7 * 8 * grid.n_bins, 64 * 8 * grid.n_bins + 5):
        assert np.array_equal(en.feldman_cousins(grid, metric, T, cl, seed, generator="device", chunk_bytes=chunk_bytes,
                                                 method=method), want)
    assert np.array_equal(en.feldman_cousins(grid, metric, T, cl, seed, true_points=[5], generator="device", method=method),
                          want[[5]])
    # method="poisson" is the call without the argument, for both generators
    assert np.array_equal(en.pseudo_data(grid, 4, T, seed, generator="device", method="poisson").cpu().numpy(),
                          en.pseudo_data(grid, 4, T, seed, generator="device").cpu().numpy(), equal_nan=True)
    assert np.array_equal(en.feldman_cousins(grid, metric, T, cl, seed, true_points=[5], generator="device", method="poisson"),
                          en.feldman_cousins(grid, metric, T, cl, seed, true_points=[5], generator="device"))
    assert np.array_equal(en.feldman_cousins(grid, metric, 16, cl, seed, true_points=[5], method="poisson"),
                          en.feldman_cousins(grid, metric, 16, cl, seed, true_points=[5]))
    # scaled_poisson on these rows: a scale per bin, through the solver's `fluctuate`
    d = en.pseudo_data(grid, 4, 50, seed, generator="device", method="scaled_poisson").cpu().numpy()
    block = fm.block(grid.host("hist")[4], np.sqrt(grid.host("sumw2")[4]), "scaled_poisson", 50, seed, stream=4)
    _check(d, block, "scaled_poisson")
