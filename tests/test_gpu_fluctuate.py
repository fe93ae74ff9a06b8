"""The device Poisson generator on the device (csrc/fluctuate.hip: `pisa_hip_poisson_fluctuate` through
`kernels.poisson_fluctuate`) against its numpy restatement (tests/fluctuate_cases.py), and `generator="device"` of
pisa_amd/analysis/ensemble.py on example_hip.cfg.

Entries are compared with `==`.  Only exp, ln and lgamma can differ between the kernel and the restatement, so only an
entry the restatement marks `marginal` (a decision within 64 eps of the magnitudes compared) may differ; their share is
held to 1e-5, and at the seeds of the kernel tests the restatement marks none (asserted), so there every entry is
compared.  The distribution of the restatement is validated in tests/test_host_fluctuate.py.
"""
import numpy as np
import pytest

from tests import fluctuate_cases as fc

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


def _draw(K, row, n_trials, seed, stream=0, first_trial=0):
    out = K.poisson_fluctuate(_dev(K, row), n_trials, seed, stream=stream, first_trial=first_trial)
    assert out.is_cuda and tuple(out.shape) == (n_trials, len(row))
    return out.cpu().numpy()


def _same(got, want, marginal):
    """`==` on every entry that is not marginal (NaN where NaN is wanted)"""
    return bool(np.all(marginal | (got == want) | (np.isnan(got) & np.isnan(want))))


def test_kernel_equals_the_restatement_on_every_shape(K):
    """(T, B) in {1, 2, 65, 257} x {1, 63, 64, 65, 257}, the row cycling through the palette of means (NaN included);
    the (65, 65) case runs its trial numbers up to the last one the counter word holds"""
    entries = flagged = 0
    for T in (1, 2, 65, 257):
        for B in (1, 63, 64, 65, 257):
            row = fc.palette_row(B)
            first = 2 ** 32 - T if (T, B) == (65, 65) else 0
            want, marginal = fc.block(row, T, SEED, STREAM, first)
            got = _draw(K, row, T, SEED, STREAM, first)
            assert np.isnan(got[:, np.isnan(row)]).all() and np.isfinite(got[:, ~np.isnan(row)]).all(), (T, B)
            assert np.all(got[:, row == 0.0] == 0.0)
            assert _same(got, want, marginal), (T, B, np.argwhere(~(marginal | (got == want) | np.isnan(want)))[:5])
            entries, flagged = entries + want.size, flagged + int(marginal.sum())
    print("%d entries, %d marginal" % (entries, flagged))
    assert flagged <= MAX_MARGINAL_SHARE * entries
    assert flagged == 0          # this seed: every entry was compared (another seed rather than a wider window)


@pytest.mark.parametrize("T,B,rows", [(70000, 3, (0, 65535, 65536, 69999)),
                                      (4100, 257, (0, 2039, 2040, 2041, 4099))])
def test_more_trials_than_a_grid_dimension_and_more_entries_than_one_pass(K, T, B, rows):
    """70 000 trials (a grid dimension holds 65 535), and 4100 x 257 entries: more than the 2048 x 256 lanes of the
    largest grid, so every lane strides (entry 524 288 is in trial 2040); single rows against the restatement"""
    seed = 5
    row = np.array([0.5, 37.5, 1e3])[np.arange(B) % 3] if B == 3 else fc.palette_row(B)
    got = _draw(K, row, T, seed)
    assert np.isfinite(got[:, ~np.isnan(row)]).all() and np.isnan(got[:, np.isnan(row)]).all()
    for t in rows:
        want, marginal = fc.block(row, 1, seed, 0, first_trial=t)
        assert not marginal.any()
        assert np.array_equal(got[t], want[0], equal_nan=True), t
    # and no row is a copy of its neighbour
    assert not np.array_equal(got[rows[1]], got[rows[2]], equal_nan=True)


def test_placement_seed_and_stream(K):
    T, row = 257, fc.palette_row(65)
    full = _draw(K, row, T, SEED, STREAM)
    assert np.array_equal(_draw(K, row, T, SEED, STREAM), full, equal_nan=True)          # two identical calls
    for n in (2, 3):
        parts = np.array_split(np.arange(T), n)
        got = np.concatenate([_draw(K, row, len(p), SEED, STREAM, first_trial=int(p[0])) for p in parts])
        assert np.array_equal(got, full, equal_nan=True), n
    # fewer bins: the same entries; an `out` given by the caller is filled and returned
    assert np.array_equal(_draw(K, row[:17], 5, SEED, STREAM), full[:5, :17], equal_nan=True)
    import torch

    out = torch.full((5, 65), -1.0, dtype=torch.float64, device=K.device())
    assert K.poisson_fluctuate(_dev(K, row), 5, SEED, stream=STREAM, out=out) is out
    assert np.array_equal(out.cpu().numpy(), full[:5], equal_nan=True)
    live = ~np.isnan(row) & (row >= 1e-3)
    for other in (_draw(K, row, T, SEED + 1, STREAM), _draw(K, row, T, SEED, STREAM + 1),
                  _draw(K, row, T, SEED + (1 << 32), STREAM)):                            # (the key's second word)
        assert np.mean(other[:, live] != full[:, live]) > 0.3
        assert np.array_equal(np.isnan(other), np.isnan(full))


def test_status_and_argument_checks(K):
    import torch

    from pisa_amd import _lib

    row = fc.palette_row(65)
    for bad in (-1.0, -1e-300, float("inf"), 2.0 ** 53, float(np.nextafter(2.0 ** 52, np.inf))):
        r = row.copy()
        r[7] = bad
        with pytest.raises(ValueError):
            _draw(K, r, 4, SEED)
    # the entry itself is NaN, its neighbours are drawn, the status word holds the code
    r = row.copy()
    r[7] = -1.0
    status = torch.zeros(1, dtype=torch.int32, device=K.device())
    got = K.poisson_fluctuate(_dev(K, r), 4, SEED, status=status).cpu().numpy()
    assert int(status.item()) == _lib.ERR_NEGATIVE and np.isnan(got[:, 7]).all()
    keep = np.arange(65) != 7
    assert np.array_equal(got[:, keep], _draw(K, row, 4, SEED)[:, keep], equal_nan=True)
    assert np.isfinite(_draw(K, np.array([2.0 ** 52, 1e15]), 4, SEED)).all()                # the largest mean taken
    mu = _dev(K, row)
    for call in (lambda: K.poisson_fluctuate(mu.reshape(5, 13), 4, SEED), lambda: K.poisson_fluctuate(mu.float(), 4, SEED),
                 lambda: K.poisson_fluctuate(mu, 4, -1), lambda: K.poisson_fluctuate(mu, 4, 2 ** 64),
                 lambda: K.poisson_fluctuate(mu, 4, SEED, stream=2 ** 32),
                 lambda: K.poisson_fluctuate(mu, 4, SEED, first_trial=-1),
                 lambda: K.poisson_fluctuate(mu, 4, SEED, out=torch.empty((4, 64), dtype=torch.float64, device=mu.device))):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: K.poisson_fluctuate(mu, 0, SEED), lambda: K.poisson_fluctuate(mu, 4, SEED, first_trial=2 ** 32 - 3)):
        with pytest.raises(_lib.PisaHipError) as err:
            call()
        assert err.value.status == -1
    # the raw entry point: NULL pointers and bad sizes are refused before any device access
    lib = _lib.lib()
    out = torch.empty((4, 65), dtype=torch.float64, device=mu.device)
    p_mu, p_out, p_st = mu.data_ptr(), out.data_ptr(), status.data_ptr()
    assert lib.pisa_hip_poisson_fluctuate(None, 65, 4, 1, 0, 0, p_out, p_st, None) == -1
    assert lib.pisa_hip_poisson_fluctuate(p_mu, 65, 4, 1, 0, 0, None, p_st, None) == -1
    assert lib.pisa_hip_poisson_fluctuate(p_mu, 65, 4, 1, 0, 0, p_out, None, None) == -1
    assert lib.pisa_hip_poisson_fluctuate(p_mu, 0, 4, 1, 0, 0, p_out, p_st, None) == -1
    assert lib.pisa_hip_poisson_fluctuate(p_mu, 65, 0, 1, 0, 0, p_out, p_st, None) == -1
    assert lib.pisa_hip_poisson_fluctuate(p_mu, 2 ** 31, 4, 1, 0, 0, p_out, p_st, None) == -1
    assert lib.pisa_hip_poisson_fluctuate(p_mu, 65, 4, 1, 0, 2 ** 32 - 3, p_out, p_st, None) == -1
    assert lib.pisa_hip_poisson_fluctuate(p_mu, 65, 4, 1, 0, 2 ** 32 - 4, p_out, p_st, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), _draw(K, row, 4, 1, 0, 2 ** 32 - 4), equal_nan=True)


# ------------------------------------------------------------------ config pipeline
def test_pseudo_data_and_feldman_cousins_with_the_device_generator_on_the_config_pipeline(K):
    """the 3 x 3 grid over theta23 x deltam31 of example_hip.cfg: `pseudo_data(generator="device")` is a device tensor
    whose rows are the restatement's draws of the template row; `feldman_cousins(generator="device")` is
    `critical_values(delta_metric(...))` of those tensors, whatever the chunk limit"""
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
    grid = en.TemplateGrid.from_maker(dm, pts, "llh")
    assert grid.hist.is_cuda and len(grid) == 9

    T, cl, seed = 200, (0.6827, 0.90), 77
    entries = flagged = 0
    data = []
    for k in range(9):
        d = en.pseudo_data(grid, k, T, seed, generator="device")
        assert d.is_cuda and tuple(d.shape) == (T, grid.n_bins)
        want, marginal = fc.block(grid.host("hist")[k], T, seed, stream=k)
        assert _same(d.cpu().numpy(), want, marginal), k
        entries, flagged = entries + want.size, flagged + int(marginal.sum())
        data.append(d)
    print("%d entries, %d marginal" % (entries, flagged))
    assert flagged <= MAX_MARGINAL_SHARE * entries
    assert not np.array_equal(data[0].cpu().numpy(), data[1].cpu().numpy())
    want = np.stack([en.critical_values(en.delta_metric(data[k], grid, "llh", k), cl) for k in range(9)])
    crit = en.feldman_cousins(grid, "llh", T, cl, seed, generator="device")
    assert np.array_equal(crit, want) and np.all(crit[:, 1] >= crit[:, 0]) and np.all(crit >= 0)
    for chunk_bytes in (7 * 8 * grid.n_bins, 64 * 8 * grid.n_bins + 5):
        assert np.array_equal(en.feldman_cousins(grid, "llh", T, cl, seed, generator="device", chunk_bytes=chunk_bytes), want)
    assert np.array_equal(en.feldman_cousins(grid, "llh", T, cl, seed, true_points=[5], generator="device"), want[[5]])
    # the host generator is untouched by all this: the reference's stream, a host array
    assert isinstance(en.pseudo_data(grid, 4, 5, 3), np.ndarray)
    assert np.array_equal(en.feldman_cousins(grid, "llh", 16, cl, seed, true_points=[5]),
                          en.feldman_cousins(grid, "llh", 16, cl, seed, true_points=[5], generator="host"))
