"""The device Poisson generator without a GPU: its numpy restatement (tests/fluctuate_cases.py) against the Philox known
answers, against `scipy.stats.poisson` (goodness of fit, mean, variance), for independence across bins, trials, streams
and seeds, for the placement property, the sampler's own source (csrc/fluctuate_device.hpp) compiled for the host
against the restatement, and `generator="device"` of pisa_amd/analysis/ensemble.py with a solver that
draws through the restatement.  tests/test_gpu_fluctuate.py holds the kernel to the restatement with `==`, so what is
shown here of the restatement's distribution is shown of the kernel's.

The gates are those of a correct sampler, not of this one: chi-square p >= 1e-4, mean and variance within 5 standard
errors (sqrt(mu / N) and sqrt((mu + 2 mu^2) / N)), correlations below 5 / sqrt(N).  Over the 33 cases a correct sampler
misses the p-value gate with probability 0.3 %; the seeds are fixed.  Measured here (`pytest -s` prints every case):
worst p-value 0.0106 (mu = 1e-3, seed 3; the next 0.025), largest |z| of a mean 2.55, of a variance 2.52 (the same
case), largest correlation 1.69 / sqrt(N).
"""
import math

import numpy as np
import pytest
from scipy import stats

from tests import ensemble_cases as ec
from tests import fluctuate_cases as fc

N_TRIALS, N_BINS = 2000, 100
N = N_TRIALS * N_BINS


def test_philox_known_answers():
    F = 0xFFFFFFFF
    for counter, key, want in (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                               ((F, F, F, F), (F, F), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                               ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
                                "d16cfe09 94fdcceb 5001e420 24126ea1")):
        assert " ".join("%08x" % int(w) for w in fc.philox(counter, key)) == want
    # vectorised over entries: the same words per entry
    w = fc.philox((np.array([0, F]), np.array([0, F]), np.array([0, F]), np.array([0, F])), (np.array([0, F]), np.array([0, F])))
    assert [int(x[0]) for x in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(x[1]) for x in w] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # the doubles: 53 bits, [0, 1)
    assert fc.unit(np.uint64(0), np.uint64(0)) == 0.0
    assert fc.unit(np.uint64(F), np.uint64(F)) == 1.0 - 2.0 ** -53
    assert fc.unit(np.uint64(1 << 5), np.uint64(0)) == 2.0 ** -27 and fc.unit(np.uint64(0), np.uint64(1 << 6)) == 2.0 ** -53


def _sample(mu, seed, stream=0):
    """N entries of one mean, addressed as a 2000 x 100 launch addresses them"""
    out, _ = fc.block(np.full(N_BINS, mu), N_TRIALS, seed, stream)
    return out


def _chi2_p(x, mu):
    """goodness of fit against scipy's Poisson(mu): cells merged from the left until each expects >= 5, both tails
    folded into the end cells -> (p-value, number of cells)"""
    lo = max(0, int(math.floor(mu - 12.0 * math.sqrt(mu) - 12.0)))
    hi = int(math.ceil(mu + 12.0 * math.sqrt(mu) + 30.0))
    ks = np.arange(lo, hi + 1)
    expect = N * stats.poisson.pmf(ks, mu)
    expect[0] = N * stats.poisson.cdf(lo, mu)
    expect[-1] = N * stats.poisson.sf(hi - 1, mu)
    seen = np.bincount(np.clip(x, lo, hi).astype(np.int64).ravel() - lo, minlength=ks.size).astype(np.float64)
    cells_e, cells_o, e, o = [], [], 0.0, 0.0
    for ei, oi in zip(expect, seen):
        e, o = e + ei, o + oi
        if e >= 5.0:
            cells_e.append(e), cells_o.append(o)
            e = o = 0.0
    if cells_e:
        cells_e[-1] += e
        cells_o[-1] += o
    else:                                   # (a mean so small that everything is one cell)
        cells_e, cells_o = [e], [o]
    E, O = np.array(cells_e), np.array(cells_o)
    assert abs(E.sum() - N) < 1e-6 * N and O.sum() == N
    if E.size == 1:
        return 1.0 if O[0] == N else 0.0, 1
    return float(stats.chi2.sf(np.sum((O - E) ** 2 / E), E.size - 1)), E.size


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_distribution_of_every_positive_mean(seed):
    for mu in fc.POSITIVE:
        x = _sample(mu, seed)
        assert np.all(x == np.rint(x)) and x.min() >= 0
        p, cells = _chi2_p(x, mu)
        z_mean = (x.mean() - mu) / math.sqrt(mu / N)
        z_var = (x.var(ddof=1) - mu) / math.sqrt((mu + 2.0 * mu * mu) / N)
        print("seed %d mu %-22.17g cells %4d p %.4f z(mean) %+.2f z(var) %+.2f" % (seed, mu, cells, p, z_mean, z_var))
        assert p >= 1e-4, (seed, mu, p)
        assert abs(z_mean) <= 5.0, (seed, mu, z_mean)
        assert abs(z_var) <= 5.0, (seed, mu, z_var)


def test_the_means_without_a_draw():
    row = np.array([0.0, -0.0, np.nan, -1.0, np.inf, 2.0 ** 53, 2.0 ** 52, 5.0])
    out, marginal = fc.block(row, 50, 4)
    assert np.all(out[:, :2] == 0.0) and np.all(np.isnan(out[:, 2:6]))
    assert np.all(np.isfinite(out[:, 6:])) and not marginal[:, :6].any()


def _corr(a, b):
    return float(np.corrcoef(np.ravel(a), np.ravel(b))[0, 1])


@pytest.mark.parametrize("mu", (3.0, 50.0))
def test_independence_of_bins_trials_streams_and_seeds(mu):
    x = _sample(mu, 1)
    pairs = {"adjacent bins": (x[:, :-1], x[:, 1:]), "adjacent trials": (x[:-1], x[1:]),
             "streams 0 and 1": (x, _sample(mu, 1, stream=1)), "seeds 1 and 2": (x, _sample(mu, 2))}
    for what, (a, b) in pairs.items():
        assert not np.array_equal(a, b)
        r = _corr(a, b)
        print("mu %g %s: correlation %+.2f / sqrt(N)" % (mu, what, r * math.sqrt(a.size)))
        assert abs(r) < 5.0 / math.sqrt(a.size), (mu, what, r)


def test_placement_one_block_or_several():
    """T trials as one block == the same trials in 2 and 3 blocks through first_trial; also from a first trial near
    the top of the counter word"""
    row = fc.palette_row(40)
    for T, first in ((23, 0), (23, 2 ** 32 - 23)):
        full, _ = fc.block(row, T, 9, stream=2, first_trial=first)
        assert np.isnan(full[:, np.isnan(row)]).all() and np.isfinite(full[:, ~np.isnan(row)]).all()
        for n in (2, 3):
            parts = np.array_split(np.arange(T), n)
            got = np.concatenate([fc.block(row, len(p), 9, stream=2, first_trial=first + int(p[0]))[0] for p in parts])
            assert np.array_equal(got, full, equal_nan=True), (T, first, n)
    # the number of bins is not part of an entry either
    assert np.array_equal(fc.block(row[:17], 5, 9)[0], fc.block(row, 5, 9)[0][:, :17], equal_nan=True)


# ------------------------------------------------------------- the kernel's own source, compiled for the host
_HOST_MAIN = r"""
// every case of the input file through pisa::fl_draw: (n_bins, n_trials, seed, stream, first_trial) as five uint64,
// then the row of means; the draws of all cases, one after the other, go to the output file
#include "fluctuate_device.hpp"
#include <stdio.h>
#include <vector>
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint64_t head[5];
    int bad_cases = 0;
    while (fread(head, 8, 5, in) == 5) {
        std::vector<double> mu(head[0]), row(head[0]);
        if (fread(mu.data(), 8, mu.size(), in) != mu.size()) return 3;
        bool bad = false;
        for (uint64_t t = 0; t < head[1]; t++) {
            for (uint64_t b = 0; b < head[0]; b++)
                row[b] = pisa::fl_draw(mu[b], (uint32_t)b, (uint32_t)(head[4] + t), (uint32_t)head[3], (uint32_t)head[2],
                                       (uint32_t)(head[2] >> 32), bad);
            fwrite(row.data(), 8, row.size(), out);
        }
        bad_cases += bad;
    }
    fclose(out);
    printf("%d\n", bad_cases);
    return 0;
}
"""


def test_the_kernel_source_on_the_host_equals_the_restatement(tmp_path):
    """csrc/fluctuate_device.hpp (Philox, the doubles, the sampler: what every lane of the kernel runs) compiled with
    g++ under ASan + UBSan and run as a program of its own on the shapes and the seed of the GPU test, on a large seed
    and on the largest means: `==` the restatement on every entry that is not marginal, none marginal on the shapes"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "main.cpp", tmp_path / "fluct_host"
    src.write_text(_HOST_MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(root, "pisa_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    cases = [(fc.palette_row(B), T, 1, 3, 2 ** 32 - T if (T, B) == (65, 65) else 0)
             for T in (1, 2, 65, 257) for B in (1, 63, 64, 65, 257)]
    n_shapes = len(cases)
    cases.append((fc.palette_row(40), 50, 2 ** 64 - 3, 2 ** 32 - 1, 7))
    cases.append((np.array([2.0 ** 52, 1e15, 1e12, 1e9, -1.0, np.inf, 2.0 ** 53, 11.0]), 200, 6, 0, 0))
    with open(tmp_path / "cases.bin", "wb") as fh:
        for row, T, seed, stream, first in cases:
            fh.write(np.array([row.size, T, seed, stream, first], dtype=np.uint64).tobytes())
            fh.write(np.ascontiguousarray(row, dtype=np.float64).tobytes())
    res = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True,
                         text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-3000:]
    assert int(res.stdout) == 1                       # the last case alone holds means without a draw
    got_all = np.fromfile(tmp_path / "out.bin")
    at = 0
    for i, (row, T, seed, stream, first) in enumerate(cases):
        want, marginal = fc.block(row, T, seed, stream, first)
        got = got_all[at:at + want.size].reshape(want.shape)
        at += want.size
        assert np.all(marginal | (got == want) | (np.isnan(got) & np.isnan(want))), (i, T, row.size)
        if i < n_shapes:
            assert not marginal.any(), (T, row.size)
    assert at == got_all.size


# --------------------------------------------------------------------------- the ensemble's plumbing
def _template_maps(hist, sumw2):
    from pisa_amd.core.map import Map

    binning = [dict(name="x", bin_edges=np.linspace(0.0, 1.0, hist.shape[1] // 4 + 1)),
               dict(name="y", bin_edges=np.linspace(0.0, 1.0, 5))]
    shape = (hist.shape[1] // 4, 4)
    return [Map(name="total", hist=h.reshape(shape), binning=binning, error_hist=np.sqrt(v).reshape(shape))
            for h, v in zip(hist, sumw2)]


@pytest.mark.parametrize("metric", ("llh", "mod_chi2"))
def test_feldman_cousins_device_generator_with_the_numpy_solver(metric):
    from pisa_amd.analysis import ensemble as en

    hist, sumw2, points, penalty = ec.toy_grid(metric)
    grid = en.TemplateGrid(hist, sumw2, points, None, penalty, metric)
    T, cl, seed = 64, (0.6827, 0.90), 1
    solver = fc.NumpyDrawSolver()
    crit = en.feldman_cousins(grid, metric, T, cl, seed, solver=solver, generator="device")
    assert crit.shape == (9, 2) and np.all(crit >= 0) and np.all(crit[:, 1] >= crit[:, 0])
    # one draw of all T trials per true point, stream = the true point; then its reduction
    assert solver.calls[:2] == [("draw", T, 0, 0), ("best", metric, (T, hist.shape[1]), hist.shape)]
    assert [c[2] for c in solver.calls if c[0] == "draw"] == list(range(9))
    # what it is made of: the draws of `pseudo_data`, their distances, the quantile rule
    for k0 in (0, 5):
        data = en.pseudo_data(grid, k0, T, seed, generator="device", solver=solver)
        assert np.array_equal(data, fc.block(hist[k0], T, seed, stream=k0)[0])
        assert np.array_equal(en.critical_values(en.delta_metric(data, grid, metric, k0, solver), cl), crit[k0])
    # chunks of 7 rows: the same values, 10 draws per true point with the trial numbers carried on
    chunked = fc.NumpyDrawSolver()
    got = en.feldman_cousins(grid, metric, T, cl, seed, solver=chunked, generator="device",
                             chunk_bytes=7 * 8 * hist.shape[1])
    assert np.array_equal(got, crit)
    assert [c[1:] for c in chunked.calls if c[0] == "draw"][:10] == [(min(7, T - f), 0, f) for f in range(0, T, 7)]
    assert np.array_equal(en.feldman_cousins(grid, metric, T, cl, seed, solver=chunked, generator="device",
                                             chunk_bytes=1), crit)               # (never less than one row)
    # a subset of true points reproduces the full run's rows; a RandomState stands for the seed it gives
    sub = en.feldman_cousins(grid, metric, T, cl, seed, true_points=[7, 2], solver=solver, generator="device")
    assert np.array_equal(sub, crit[[7, 2]])
    drawn = int(np.random.RandomState(5).randint(0, 2 ** 31 - 1))
    assert np.array_equal(
        en.feldman_cousins(grid, metric, T, cl, np.random.RandomState(5), true_points=[3], solver=solver, generator="device"),
        en.feldman_cousins(grid, metric, T, cl, drawn, true_points=[3], solver=solver, generator="device"))
    # another seed: other draws
    assert not np.array_equal(en.feldman_cousins(grid, metric, T, cl, 2, solver=solver, generator="device"), crit)


def test_generator_names_and_solvers_without_draw():
    from pisa_amd.analysis import ensemble as en

    hist, sumw2, points, penalty = ec.toy_grid("llh")
    grid = en.TemplateGrid(hist, sumw2, points, None, penalty, "llh")
    for solver in (fc.NumpyDrawSolver(), ec.NumpySolver()):
        with pytest.raises(ValueError, match="generator"):
            en.feldman_cousins(grid, "llh", 8, random_state=1, solver=solver, generator="philox")
        with pytest.raises(ValueError, match="generator"):
            en.pseudo_data(grid, 0, 8, 1, generator="gpu", solver=solver)
    plain = ec.NumpySolver()
    with pytest.raises(ValueError, match="draw"):
        en.feldman_cousins(grid, "llh", 8, random_state=1, solver=plain, generator="device")
    with pytest.raises(ValueError, match="draw"):
        en.pseudo_data(grid, 0, 8, 1, generator="device", solver=plain)
    assert plain.calls == []
    # the host generator asks nothing of the solver but `best`
    assert en.feldman_cousins(grid, "llh", 8, random_state=1, solver=plain, generator="host").shape == (9, 2)


def test_host_generator_is_still_the_reference_loop_bit_for_bit():
    """generator="host" (named or by default), seed 1: `==` the loop over `Map.fluctuate` with the metric of a pair taken
    from the same numpy restatement the solver runs (an entry's bits depend on its two rows alone)"""
    from pisa_amd.analysis import ensemble as en

    metric = "llh"
    hist, sumw2, points, penalty = ec.toy_grid(metric)
    grid = en.TemplateGrid(hist, sumw2, points, None, penalty, metric)
    maps = _template_maps(hist, sumw2)
    T, cl, seed, true_points = 32, (0.6827, 0.90), 1, [0, 4, 7]

    def metric_total(data_map, k):
        return ec.direct_form(metric, data_map.nominal_values.reshape(1, -1), hist[k][None, :])[0, 0]

    want, _ = ec.loop_feldman_cousins(metric_total, maps, penalty, metric, T, cl, seed, true_points)
    solver = fc.NumpyDrawSolver()
    assert np.array_equal(en.feldman_cousins(grid, metric, T, cl, seed, true_points, solver, generator="host"), want)
    assert np.array_equal(en.feldman_cousins(grid, metric, T, cl, seed, true_points, solver), want)
    assert not any(c[0] == "draw" for c in solver.calls)
    # and `pseudo_data` by default is the host stream
    assert np.array_equal(en.pseudo_data(grid, 4, 5, 3, generator="host"), en.pseudo_data(grid, 4, 5, 3))
    rs = np.random.RandomState(3)
    assert np.array_equal(en.pseudo_data(grid, 4, 5, 3),
                          np.stack([maps[4].fluctuate("poisson", random_state=rs).nominal_values.ravel() for _ in range(5)]))


def test_both_generators_give_the_same_critical_values_statistically():
    """one true point, T = 2000: the critical value from device-style draws lies between the host-drawn sorted
    distances at the indices ceil(cl T) - 1 -+ ceil(4 sqrt(2) sqrt(T cl (1 - cl))): four binomial standard errors of an
    order statistic, sqrt(2) because both samples fluctuate"""
    from pisa_amd.analysis import ensemble as en

    hist, sumw2, points, penalty = ec.toy_grid("llh")
    grid = en.TemplateGrid(hist, sumw2, points, None, penalty, "llh")
    T, cl, k0, seed = 2000, (0.6827, 0.90), 4, 1
    solver = fc.NumpyDrawSolver()
    crit = en.feldman_cousins(grid, "llh", T, cl, seed, true_points=[k0], solver=solver, generator="device")[0]
    host = np.sort(en.delta_metric(en.pseudo_data(grid, k0, T, np.random.RandomState([seed, k0])), grid, "llh", k0, solver))
    for c, got in zip(cl, crit):
        at = int(math.ceil(c * T)) - 1
        width = int(math.ceil(4.0 * math.sqrt(2.0) * math.sqrt(T * c * (1.0 - c))))
        lo, hi = host[max(at - width, 0)], host[min(at + width, T - 1)]
        print("cl %.4f: device-style %.4f, host %.4f in [%.4f, %.4f]" % (c, got, host[at], lo, hi))
        assert lo <= got <= hi, (c, got, lo, hi)
