"""The host decisions of the KDE (pisa_amd/csrc/kde_plan.hpp) without a GPU: tests/host/kde_plan_main.cpp, which
includes that header and nothing else of the library, is built with AddressSanitizer and UBSan and run as a child
process; what it prints is compared with the numpy restatements and constants of tests/kde_cases.py, which until now
only GPU runs tied to the C++."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import kde_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
CLOUDS = ("cloud999", "cloud1000", "cloud1500")
GRID_CASES = [(f, None) for f in kc.SAMPLE_FAMILIES] + [(f, t) for f in CLOUDS for t in kc.TOLS]
# the (da_s, counts, want_r) rows of test_gpu_kde_exact.py::test_lattice_every_strip_length and the (counts, lg) rows of
# ::test_lattice_every_lane_group_width
STRIP_ROWS = [(0.15, (131, 45), 32), (1.5, (67, 33), 32), (2.5, (37, 45), 16), (3.125, (35, 9), 16), (5.0, (19, 45), 8),
              (6.25, (9, 70), 8), (8.0, (7, 45), 0), (0.15, (1, 45), 32), (0.15, (131, 1), 32), (5.0, (1, 1), 8)]
LG_ROWS = [((551, 557), 16), ((787, 769), 32), ((1103, 1109), 64)]
# the lattice's estimator, fixed here: U00 a power of two and max s2 = 4, so that da sqrt(max s2) IS the row's da_s
LAT = dict(n=1500, tol=1e-14, u00=0.5, u11=1.7, s2_max=4.0, step1=0.013)


def _fmt(v):
    return repr(float(v)) if isinstance(v, float) else str(int(v))


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """run(lines) -> the program's JSON, one object per line of commands"""
    d = tmp_path_factory.mktemp("kde_plan")
    exe = str(d / "kde_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "pisa_amd", "csrc"), os.path.join(ROOT, "tests", "host", "kde_plan_main.cpp"), "-o", exe],
                   check=True)
    count = [0]

    def run(lines):
        count[0] += 1
        path = str(d / ("cases%d.txt" % count[0]))
        with open(path, "w") as f:
            f.write("".join(line[0] + " " + " ".join(_fmt(v) for v in line[1:]) + "\n" for line in lines))
        p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, p.stderr.decode()[-4000:]
        out = json.loads(p.stdout)
        assert len(out) == len(lines)
        return out

    return run


def test_constants(plan):
    c, below, at, series = plan([("constants",), ("plan", 0.98, 1e-14, 400, kc.EXPANSION_MIN_N - 1, 2, 1, 64.5, 2),
                                 ("plan", 0.98, 1e-14, 400, kc.EXPANSION_MIN_N, 2, 1, 64.5, 2),
                                 ("plan", 0.98, 1e-14, 400, 5000, 1, 1, 64.5, 2)])
    assert c["Q_CHUNK"] == kc.Q_CHUNK and c["HERMITE_MIN_SERIES"] == kc.HERMITE_MIN_SERIES
    assert c["EXPANSION_MIN_N"] == kc.EXPANSION_MIN_N
    assert (below["expand"], at["expand"]) == (0, 1)
    assert (at["local_ok"], at["dense_min"], at["P"], at["h2l_split"]) == (1, 1, 20, 2)
    assert (series["expand"], series["local_ok"], series["dense_min"]) == (1, 0, kc.HERMITE_MIN_SERIES)


def _fp64_moments(x, w):
    """what the two reduction passes hand to the host, in fp64: sum w, mean, box, sum w^2 and the second moments"""
    x, w = np.asarray(x, dtype=float), np.asarray(w, dtype=float)
    d = x.shape[0]
    sw = float(w.sum())
    mean = (x * w).sum(axis=1) / sw
    xc = x - mean[:, None]
    h2 = [float((w * w).sum())] + [float((w * xc[a] * xc[b]).sum()) for a in range(d) for b in range(a, d)]
    pad = lambda v: [float(t) for t in v] + [0.0] * (3 - d)
    return sw, h2 + [0.0] * (7 - len(h2)), pad(mean), pad(x.min(axis=1)), pad(x.max(axis=1))


def _rel(got, want):
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


# A family whose (hi - lo) / cell is within rounding of an integer in some dimension may differ in that count between
# the restatement (moments rounded from long double) and the program (fp64 moments).  None of the cases is.
ON_A_CELL_BOUNDARY = ()


@pytest.mark.parametrize("fam,tol", GRID_CASES)
def test_grid_and_series_order(plan, fam, tol):
    x, w, kw = kc.family(fam)
    tol = kw["tol"] if tol is None else tol
    d, n = x.shape
    want = kc.grid_rule(x, w, kw["bw_method"], tol)
    sw, h2, mean, lo, hi = _fp64_moments(x, w)
    got, = plan([("grid", d, n, 0 if kw["bw_method"] == "silverman" else 1, tol, sw, *h2, *mean, *lo, *hi)])
    assert got["ok"]
    assert abs(got["cell"] - want["cell"]) <= 1e-14 * want["cell"]      # one ulp of log / sqrt between libm and numpy
    assert abs(got["r_cut"] - want["r_cut"]) <= 1e-14 * want["r_cut"]
    assert got["order"] == want["order"]
    assert fam not in ON_A_CELL_BOUNDARY
    assert got["nc"][:d] == [int(c) for c in want["counts"]] and got["nc"][d:] == [1] * (3 - d)
    assert got["n_cells"] == int(np.prod(want["counts"]))
    if fam == "narrow":     # (correlation 0.999 about a mean of 1e3: x - mean and the whitening lose five digits in fp64,
        return              #  tests/kde_cases.py, G_REF; U and inv_cov are exempt)
    e = kc.exact_moments(x, w, kw["bw_method"])
    assert _rel(np.reshape(got["U"], (3, 3))[:d, :d], e["U"]) <= 1e-12
    assert _rel(np.reshape(got["inv_cov"], (3, 3))[:d, :d], e["inv_cov"]) <= 1e-12
    assert _rel(np.reshape(got["cov"], (3, 3))[:d, :d], e["cov"]) <= 1e-12
    assert abs(got["norm"] - float(e["norm"])) <= 1e-12 * float(e["norm"])


def _lattice_args(da_s, counts):
    step = [da_s / (LAT["u00"] * np.sqrt(LAT["s2_max"])), LAT["step1"]]
    assert LAT["u00"] * step[0] * np.sqrt(LAT["s2_max"]) == da_s
    return step, 2.0 * np.log(1.0 / LAT["tol"])


def test_lattice_strip_and_shape(plan):
    lines, want = [], []
    for da_s, counts, want_r in STRIP_ROWS + [(5.0, c, 8) for c, _ in LG_ROWS]:
        step, rcut2 = _lattice_args(da_s, counts)
        assert kc.lattice_strip(da_s, LAT["tol"]) == want_r
        lines.append(("strip", 2, rcut2, LAT["u00"], LAT["s2_max"], step[0], step[1], counts[0], counts[1], -1))
        want.append(dict(R=want_r))
        if want_r:
            sw, lg, patches = kc.lattice_shape(LAT["n"], LAT["tol"], LAT["u00"], LAT["u11"], step, counts, want_r)
            lines.append(("shape", LAT["n"], rcut2, LAT["u00"], LAT["u11"], want_r, step[0], step[1], counts[0], counts[1]))
            want.append(dict(sw=sw, lg=lg, patches=patches))
    got = plan(lines)
    for g, w_, line in zip(got, want, lines):
        assert {k: g[k] for k in w_} == w_, line
        if "patches" in w_:
            assert g["waves"] == max(6144, w_["patches"])
    assert [g["lg"] for g in got if "lg" in g] == [8] * 9 + [lg for _, lg in LG_ROWS]
    # the development bound on the strip: never, or no longer than
    forced = plan([("strip", 2, 64.5, 0.5, 4.0, 0.15, 0.013, 131, 45, f) for f in (0, 8, 16, 40)])
    assert [g["R"] for g in forced] == [0, 8, 16, 32]
    # not 2-D, no cut-off, a cut-off beyond 1e-30, a step of no length
    off = plan([("strip", 3, 64.5, 0.5, 4.0, 0.15, 0.013, 131, 45, -1), ("strip", 2, 0.0, 0.5, 4.0, 0.15, 0.013, 131, 45, -1),
                ("strip", 2, 139.0, 0.5, 4.0, 0.15, 0.013, 131, 45, -1), ("strip", 2, 64.5, 0.5, 4.0, 0.0, 0.013, 131, 45, -1)])
    assert [g["R"] for g in off] == [0, 0, 0, 0]


def _parts(blocks):
    return [(b[0], b[1]) for b in blocks]


def test_split_evenly(plan):
    table = plan([("split", 0, 300, 256), ("split", 0, 600, 512), ("split", 0, 512, 512), ("split", 0, 513, 512),
                  ("split", 1000, 1300, 256)])
    assert [[b[1] for b in t["blocks"]] for t in table] == [[150, 150], [300, 300], [512], [256, 257], [150, 150]]
    assert _parts(table[4]["blocks"]) == [(1000, 150), (1150, 150)]
    lengths = list(range(1, 2001))
    for chunk in (256, 512):
        for t, length in zip(plan([("split", 7, 7 + length, chunk) for length in lengths]), lengths):
            at = 7
            for begin, count in _parts(t["blocks"]):
                assert begin == at and 0 < count <= chunk
                at += count
            assert at == 7 + length and len(t["blocks"]) == -(-length // chunk)


def test_pilot_blocks_on_clumps(plan):
    x, w, kw = kc.family("clumps")
    g = kc.grid_rule(x, w, kw["bw_method"], kw["tol"])
    counts = [int(c) for c in g["counts"]]
    per_cell = np.bincount(g["cell_of"], minlength=counts[0] * counts[1])
    cell_start = np.concatenate([[0], np.cumsum(per_cell)])
    got, = plan([("blocks", counts[0], counts[1], 1, *cell_start)])
    cells = np.unique(g["cell_of"])
    assert got["cells"] == [int(c) for c in cells]
    assert got["starts"] == [int(cell_start[c]) for c in cells]
    at, big = 0, []
    for q_begin, q_count, cx, cy, cz, head in got["blocks"]:        # every source once, in order
        assert q_begin == at and 0 < q_count <= kc.Q_CHUNK
        cell = int(cells[head])
        assert (cx, cy, cz) == (cell % counts[0], cell // counts[0], 0)
        assert cell_start[cell] <= q_begin and q_begin + q_count <= cell_start[cell + 1]
        if per_cell[cell] >= 700:
            big.append(q_count)
        at += q_count
    assert at == x.shape[1]
    assert len(big) == 2 and big[0] + big[1] == per_cell.max() and abs(big[0] - big[1]) <= 1      # 700: 350 + 350
    assert per_cell.max() != 700 or big == [350, 350]
    # a 3-D table: the cell's coordinates come from the flat index
    got3, = plan([("blocks", 2, 3, 2, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 4)])
    assert got3["cells"] == [1, 11] and got3["starts"] == [0, 1]
    assert got3["blocks"] == [[0, 1, 1, 0, 0, 0], [1, 3, 1, 2, 1, 1]]


@pytest.mark.parametrize("tol", [1e-10, 1e-14])
def test_hankel_table(plan, tol):
    cell = float(np.sqrt(2.0 * np.log(1.0 / tol)) / 8.0)
    cases = [(reach, P) for reach in (4, 9) for P in (14, 20)]
    got = plan([("hankel", reach, P, cell) for reach, P in cases])
    rsqrt2 = LD("0.70710678118654752440084436210485")
    for (reach, P), g in zip(cases, got):
        nh = 2 * P - 1
        want = np.empty((2 * reach + 1, nh))
        for j in range(-reach, reach + 1):
            d = LD(j) * LD(cell) * rsqrt2
            h = [np.exp(-d * d), 2 * d * np.exp(-d * d)]
            for m in range(1, nh - 1):
                h.append(2 * d * h[m] - 2 * LD(m) * h[m - 1])
            want[j + reach] = [float(v) for v in h]
        assert np.array_equal(np.reshape(g["table"], (2 * reach + 1, nh)), want), (reach, P)


@pytest.mark.parametrize("nd,n_heads,n_cells,P,reach", [(7, 7, 30, 14, 4), (3, 9, 40, 20, 9)])
def test_pilot_scratch_layout(plan, nd, n_heads, n_cells, P, reach):
    split = 1 if P <= 16 else 2
    s, = plan([("scratch", P, reach, split, 1, nd, n_heads, n_cells)])
    pp, n_hankel = P * P, (2 * reach + 1) * (2 * P - 1)
    regions = sorted([(8 * s["herm"], 8 * nd * pp), (8 * s["local"], 8 * split * n_heads * pp), (8 * s["hankel"], 8 * n_hankel),
                      (8 * s["V"], 8 * split * n_cells * pp), (8 * s["vflag"], split * n_cells)])
    assert regions[0][0] == 0
    for (a, size), (b, _) in zip(regions, regions[1:]):
        assert a % 8 == 0 and a + size <= b
    assert regions[-1][0] + regions[-1][1] <= s["bytes"]
    # the size pisa_hip_kde_create asked the library scratch for before the layout had a name
    assert s["bytes"] == (nd * pp + split * (n_heads + n_cells) * pp + n_hankel) * 8 + split * n_cells + 8192
    series_only, = plan([("scratch", P, reach, split, 0, nd, n_heads, n_cells)])
    assert series_only["herm"] == 0 and series_only["bytes"] == nd * pp * 8 + 8192
