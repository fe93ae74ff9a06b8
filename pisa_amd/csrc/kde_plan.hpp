// kde_plan.hpp -- what the host decides for the KDE estimator of kde.hip, as plain C++17: the structs the kernels take
// by value, the constants host and kernels share, and every set-up decision as a function of numbers (bandwidth matrix
// and whitening, the cell grid, the series order, the pilot's form and scratch layout, the Hankel table, the
// workgroup split, the tile size, the lattice launch shape, the workspace sizes).  No HIP header and no environment:
// the development knobs of kde.hip come in as arguments.  tests/host/kde_plan_main.cpp runs this file alone under the
// sanitizers (tests/test_host_kde_plan.py), against the numpy restatements of tests/kde_cases.py.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace pisa {

constexpr int KDE_TILE = 1024;
constexpr int KDE_THREADS = 256;
constexpr int RED_BLOCKS = 256;   // fixed reduction geometry => fixed summation order
constexpr int RED_THREADS = 256;
constexpr int Q_PER_THREAD = 2;
constexpr int Q_CHUNK = KDE_THREADS * Q_PER_THREAD;   // queries per workgroup
constexpr int SRC_TILE = 512;                          // sources per LDS tile
constexpr int64_t KEY_OFF = 1 << 20;                   // tile coordinates are stored + 2^20
constexpr int MAX_CELLS = 1 << 22;
constexpr int HERMITE_MIN_DEFAULT = 1;   // with local expansions (see pilot_plan)
constexpr int HERMITE_MIN_SERIES = 24;   // series evaluated per target
constexpr int H2L_MAX_REACH = 12;
constexpr int LAT_GREC = 8;
constexpr int LAT_SHARE = 64;   // sources per share (= the workgroup of kde_lattice_prep_kernel, which writes the share's box)
// (1 000: C3-shaped evaluations of 1e5 / 3e5 events take 11.5 / 27.5 ms with the round-2 threshold of 20 000 sources per
//  estimator -- direct pair sums below it --, 5.7 / 5.9 ms with this one)
constexpr int64_t expansion_min_n = 1000;

// the cell grid never has more than max(4096, 4 n) cells (larger cells beyond that: less pruning,
// same results), so that the workspace scales with the number of sources
static inline int64_t cells_cap(int64_t n) { return std::min<int64_t>(MAX_CELLS, std::max<int64_t>(4096, 4 * n)); }

struct KdeGeom {
    int32_t dim;
    int32_t nc[3];       // cells per dimension (1 for unused dimensions)
    double ylo[3];       // lower corner of the cell grid in whitened coordinates
    double cell, inv_cell;
    double rcut2;        // 2 ln(1/tol); <= 0: no cut-off
    double U[9];         // whitening: y = U (x - mean), upper triangular, row-major 3x3
    double mean[3];
};

struct KdeBlock {        // one workgroup of the pair kernel
    int32_t q_begin, q_count;
    int32_t c0[3], c1[3];   // cell bounds of the queries' tile (inclusive; may lie outside the grid)
    int32_t head;           // index of the tile among the non-empty tiles (sorted order)
};

struct KdeLattice {
    double ya0, yb0;   // whitened coordinates of lattice point (0, 0)
    double da;         // y_a step of index 0 (> 0)
    double sa, db;     // (y_a, y_b) step of index 1
    int32_t n0, n1, strips_a;   // strips_a = ceil(n0 / R)
    int32_t sw, lpw, n_colblk;  // a wavefront's sub-patch: sw strips of lpw consecutive lines (sw lpw = LG lanes, 64 / LG lane groups); column blocks per line
};

// ------------------------------------------------------------------ bandwidth matrix, whitening
struct KdeBandwidth {
    double factor, det, norm;
    double cov[9], inv_cov[9];   // covariance x factor^2 and its inverse, row-major 3x3, zero outside dim x dim
    double U[9];                 // Cholesky inv_cov = L L^T, U = L^T  =>  |U v|^2 = v^T inv_cov v
};

// h2: sum w^2, sum w xc_d xc_e (d <= e) about the weighted mean; sw: sum w.  Unbiased weighted covariance x factor^2.
// false: the matrix is not positive definite.
static inline bool bandwidth_matrix(const double *h2, double sw, int64_t n, int dim, int bw_method, KdeBandwidth &b) {
    const double denom = 1.0 - h2[0] / (sw * sw);
    double cov[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    {
        int idx = 1;
        for (int d = 0; d < dim; d++)
            for (int e = d; e < dim; e++) {
                cov[d][e] = cov[e][d] = h2[idx] / sw / denom;
                idx++;
            }
    }
    b.factor = bw_method == 0 ? pow((double)n * (dim + 2) / 4.0, -1.0 / (dim + 4))   // silverman
                              : pow((double)n, -1.0 / (dim + 4));                      // scott
    double H[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int d = 0; d < dim; d++)
        for (int e = 0; e < dim; e++) H[d][e] = cov[d][e] * b.factor * b.factor;
    const double det = H[0][0] * (H[1][1] * H[2][2] - H[1][2] * H[2][1]) -
                       H[0][1] * (H[1][0] * H[2][2] - H[1][2] * H[2][0]) +
                       H[0][2] * (H[1][0] * H[2][1] - H[1][1] * H[2][0]);
    b.det = det;
    if (!(det > 0.0) || !std::isfinite(det)) return false;
    double inv[3][3];
    inv[0][0] = (H[1][1] * H[2][2] - H[1][2] * H[2][1]) / det;
    inv[0][1] = (H[0][2] * H[2][1] - H[0][1] * H[2][2]) / det;
    inv[0][2] = (H[0][1] * H[1][2] - H[0][2] * H[1][1]) / det;
    inv[1][0] = (H[1][2] * H[2][0] - H[1][0] * H[2][2]) / det;
    inv[1][1] = (H[0][0] * H[2][2] - H[0][2] * H[2][0]) / det;
    inv[1][2] = (H[0][2] * H[1][0] - H[0][0] * H[1][2]) / det;
    inv[2][0] = (H[1][0] * H[2][1] - H[1][1] * H[2][0]) / det;
    inv[2][1] = (H[0][1] * H[2][0] - H[0][0] * H[2][1]) / det;
    inv[2][2] = (H[0][0] * H[1][1] - H[0][1] * H[1][0]) / det;
    b.norm = sqrt(pow(2.0 * M_PI, dim) * det);
    for (int d = 0; d < 3; d++)
        for (int e = 0; e < 3; e++) {
            b.cov[d * 3 + e] = (d < dim && e < dim) ? H[d][e] : 0.0;
            b.inv_cov[d * 3 + e] = (d < dim && e < dim) ? inv[d][e] : 0.0;
        }
    double L[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int i = 0; i < dim; i++)
        for (int j = 0; j <= i; j++) {
            double sum = inv[i][j];
            for (int p = 0; p < j; p++) sum -= L[i][p] * L[j][p];
            if (i == j) {
                if (!(sum > 0.0)) return false;
                L[i][i] = sqrt(sum);
            } else L[i][j] = sum / L[j][j];
        }
    for (int d = 0; d < 3; d++)
        for (int e = 0; e < 3; e++) b.U[d * 3 + e] = (d < dim && e < dim) ? L[e][d] : 0.0;
    return true;
}

// ------------------------------------------------------------------ cell grid
// Cell grid over the whitened bounding box (image of the corners of the x box [xmin, xmax]): cells of r_cut / 8
// (r_cut / 4 in 3-D), grown by factors of 1.25 until the grid fits cells_cap(n) and every coordinate 2^16; without a
// cut-off one cell.  Fills every field of `g`.  false: the box is not finite.
static inline bool cell_grid(const double *U, const double *mean, const double *xmin, const double *xmax, int dim,
                             double tol, int64_t n, KdeGeom &g, int64_t &n_cells, double &r_cut) {
    memset(&g, 0, sizeof(g));
    g.dim = dim;
    for (int d = 0; d < 3; d++) {
        g.mean[d] = mean[d];
        for (int e = 0; e < 3; e++) g.U[d * 3 + e] = U[d * 3 + e];
    }
    double ylo[3] = {0, 0, 0}, yhi[3] = {0, 0, 0};
    for (int d = 0; d < dim; d++) { ylo[d] = INFINITY; yhi[d] = -INFINITY; }
    for (int corner = 0; corner < (1 << dim); corner++) {
        double xc[3] = {0, 0, 0};
        for (int d = 0; d < dim; d++) xc[d] = ((corner >> d) & 1 ? xmax[d] : xmin[d]) - mean[d];
        for (int d = 0; d < dim; d++) {
            double a = 0.0;
            for (int e = d; e < dim; e++) a += g.U[d * 3 + e] * xc[e];
            ylo[d] = std::min(ylo[d], a);
            yhi[d] = std::max(yhi[d], a);
        }
    }
    const bool cut = tol > 0.0;
    g.rcut2 = cut ? 2.0 * log(1.0 / tol) : 0.0;
    r_cut = cut ? sqrt(g.rcut2) : INFINITY;
    double extent = 0.0;
    for (int d = 0; d < dim; d++) extent = std::max(extent, yhi[d] - ylo[d]);
    if (!std::isfinite(extent)) return false;
    double cell = cut ? r_cut / (dim == 3 ? 4.0 : 8.0) : (extent > 0 ? 2.0 * extent : 1.0);
    for (;;) {   // keep the grid below MAX_CELLS and every coordinate below 2^20
        double total = 1.0;
        bool ok = true;
        for (int d = 0; d < dim; d++) {
            const double c = floor((yhi[d] - ylo[d]) / cell) + 1.0;
            total *= c;
            ok = ok && c < (double)(KEY_OFF / 16);
        }
        if (ok && total <= (double)cells_cap(n)) break;
        cell *= 1.25;
    }
    g.cell = cell;
    g.inv_cell = 1.0 / cell;
    n_cells = 1;
    for (int d = 0; d < 3; d++) {
        g.nc[d] = d < dim ? (int)(floor((yhi[d] - ylo[d]) / cell) + 1.0) : 1;
        g.ylo[d] = d < dim ? ylo[d] : 0.0;
        n_cells *= g.nc[d];
    }
    return true;
}

// ------------------------------------------------------------------ the pilot's form
// Order of the Hermite / local series: the smallest of 14, 16, 18, 20 whose truncation bound (kde.hip, "Hermite
// series": 2.3 K^2 (cell / 2)^P / sqrt(P!) of a cell's weight, all of it at a corner of the cell) is within 4 x tol.
// The cells are r_cut / 8 wide, so the bound depends on tol through the cell size as well: 20 at 1e-14 (1.8e-15), 16
// at 1e-12 (2.8e-12; round 4 took 18 there: 3.5e-14, 28 x finer than the cut-off it sits beside), 14 at 1e-10.  The
// pilot's error reaches a density only through lambda = (pilot / g)^-alpha, i.e. scaled by alpha (<= 1).
// The cells are wider than r_cut / 8 where the grid had to fit cells_cap(n) (a far outlier, with or without weight,
// widens the bounding box): if order 20 misses the bound as well the answer is 0 and there is no expansion, the pilot
// is the direct pair sum (n_dense = 0).  Before, 20 was taken unchecked: pilot errors of 5e-6 of a cell's weight at
// cell = 3.8.
static inline int series_order(double cell, double tol) {
    for (int cand : {14, 16, 18, 20}) {
        double bound = 2.3 * 1.09 * 1.09, fact = 1.0;
        for (int i = 1; i <= cand; i++) { bound *= 0.5 * cell; fact *= (double)i; }
        if (bound / sqrt(fact) <= 4.0 * tol) return cand;
    }
    return 0;
}

struct KdePilotPlan {
    bool expand;     // cells of at least dense_min sources get a Hermite series; false: every pair is summed
    int P;           // series order (20 where none meets the bound: sizes only)
    bool local_ok;   // the series are translated into one local expansion per target cell
    int dense_min;
    int reach;       // cells within the cut-off, per direction
    int h2l_split;   // parts the translation passes run in
};

// `expansion`: 0 direct sums, 1 Hermite series per target, 2 + local expansions (pisa_hip_kde_configure);
// `hermite_min`: the smallest cell that gets a series where local expansions run (a development knob of kde.hip)
static inline KdePilotPlan pilot_plan(const KdeGeom &g, int64_t n_cells, int64_t n, double tol, int expansion,
                                      int hermite_min) {
    KdePilotPlan p;
    p.P = series_order(g.cell, tol);
    const bool series_ok = p.P != 0;
    if (!series_ok) p.P = 20;   // (sizes below only)
    p.reach = (int)ceil(sqrt(g.rcut2) * g.inv_cell);
    // local expansions need the intermediate V of every cell of the grid: bounded
    p.local_ok = expansion >= 2 && ceil(sqrt(g.rcut2) * g.inv_cell) <= (double)H2L_MAX_REACH &&
                 (double)n_cells * (p.P * p.P) * 8.0 < 2.0e9;
    // with local expansions a series costs its cell 400 multiply-adds per source and nothing per
    // target, so every non-empty cell gets one; evaluated target by target (no local expansions) a
    // series pays from ~24 sources
    p.dense_min = p.local_ok ? hermite_min : std::max(hermite_min, HERMITE_MIN_SERIES);
    // translation passes: on the matrix cores where the series order allows (<= 16), in one part; else four targets
    // per workgroup on the vector units, in two parts of the source positions (see kde_h2l4_kernel): V, its flags
    // and the local expansions once per part
    p.h2l_split = p.P <= 16 ? 1 : 2;
    // dense cells get a Hermite series (2-D, with a cut-off, enough sources to pay)
    p.expand = expansion && series_ok && g.dim == 2 && tol > 0.0 && n >= expansion_min_n;
    return p;
}

// The library scratch of the expansion pilot, in doubles from its start: Hermite coefficients of the `nd` dense
// cells, local expansions of the `n_heads` non-empty cells, the Hankel table, the intermediate V of every cell, and
// (bytes) V's flags; up to 3.2 KB per cell.  Without local expansions only `herm` is used.
struct KdePilotScratch {
    size_t herm, local, hankel, V, vflag;
    size_t bytes;
};

static inline KdePilotScratch pilot_scratch(const KdePilotPlan &p, int nd, int n_heads, int64_t n_cells) {
    const size_t pp = (size_t)(p.P * p.P);
    const size_t n_hankel = (size_t)((2 * p.reach + 1) * (2 * p.P - 1));
    KdePilotScratch l;
    l.herm = 0;
    l.local = nd * pp;
    l.hankel = l.local + (p.local_ok ? p.h2l_split * n_heads * pp : 0);
    l.V = l.hankel + n_hankel;
    l.vflag = l.V + (p.local_ok ? (size_t)p.h2l_split * n_cells * pp : 0);
    l.bytes = (nd * pp + (p.local_ok ? p.h2l_split * (n_heads + (size_t)n_cells) * pp + n_hankel : 0)) * sizeof(double) +
              (p.local_ok ? (size_t)p.h2l_split * n_cells : 0) + 8192;
    return l;
}

// h_m(d), d = j cell / sqrt 2, j = -reach .. reach, m < 2 P - 1: h_0 = exp(-d^2), h_1 = 2 d h_0,
// h_{m+1} = 2 d h_m - 2 m h_{m-1}, in long double, rounded once
static inline std::vector<double> hankel_table(int reach, int P, double cell) {
    const int nh = 2 * P - 1;
    std::vector<double> hankel((size_t)(2 * reach + 1) * nh);
    for (int j = -reach; j <= reach; j++) {
        const long double d = (long double)j * (long double)cell * 0.70710678118654752440084436210485L;
        long double h0 = expl(-d * d), h1 = 2.0L * d * h0;
        double *row = hankel.data() + (size_t)(j + reach) * nh;
        row[0] = (double)h0;
        row[1] = (double)h1;
        for (int m = 1; m + 1 < nh; m++) {
            const long double h2 = 2.0L * d * h1 - 2.0L * m * h0;
            row[m + 1] = (double)h2;
            h0 = h1;
            h1 = h2;
        }
    }
    return hankel;
}

// ------------------------------------------------------------------ workgroups
// Appends the workgroups of the queries [begin, end) of one tile (`b`: its cell bounds and head), each of `chunk`
// queries at most, in equal shares: 300 queries at chunk 256 become 150 + 150, not 256 + 44.
static inline void split_evenly(int64_t begin, int64_t end, int chunk, KdeBlock b, std::vector<KdeBlock> &blocks) {
    const int64_t parts = (end - begin + chunk - 1) / chunk;
    for (int64_t p = 0; p < parts; p++) {
        const int64_t q0 = begin + (end - begin) * p / parts, q1 = begin + (end - begin) * (p + 1) / parts;
        b.q_begin = (int32_t)q0;
        b.q_count = (int32_t)(q1 - q0);
        blocks.push_back(b);
    }
}

// Pilot estimate at the sources themselves: queries = sorted sources, tiles = cells.  From the cell table
// (`cell_start`, n_cells + 1 entries): the workgroups over the sources of every non-empty cell, and the flat index
// and first source of those cells ("heads"), in cell order.
static inline void pilot_blocks(const int32_t *cell_start, const KdeGeom &g, int64_t n_cells, std::vector<KdeBlock> &blocks,
                                std::vector<int32_t> &cells, std::vector<int32_t> &starts) {
    const int64_t nx = g.nc[0], nxy = (int64_t)g.nc[0] * g.nc[1];
    for (int64_t c = 0; c < n_cells; c++) {
        const int64_t begin = cell_start[c], end = cell_start[c + 1];
        if (end <= begin) continue;
        const int64_t cz = c / nxy, cy = (c - cz * nxy) / nx, cx = c - cz * nxy - cy * nx;
        KdeBlock b;
        b.head = (int32_t)starts.size();
        b.c0[0] = b.c1[0] = (int32_t)cx; b.c0[1] = b.c1[1] = (int32_t)cy; b.c0[2] = b.c1[2] = (int32_t)cz;
        cells.push_back((int32_t)c);
        starts.push_back((int32_t)begin);
        split_evenly(begin, end, Q_CHUNK, b, blocks);
    }
}

// source splits of the pair kernel: enough workgroups for 256 CUs x 4 where there are few blocks of queries
static inline int pick_split(int n_blocks) {
    int n_split = 1;
    if (n_blocks < 1024) n_split = std::min(32, (1024 + n_blocks - 1) / n_blocks);
    return n_split;
}

// Tile size (cells per side) of a point evaluation of m queries.  A tile's queries are cut into equal workgroups of
// <= 256 (one query per thread); per query the cost is ~ (cells within reach of the tile) / (share of the 256 lanes
// in use).  Assumes the queries cover the source grid evenly (a map's bin centres).
static inline int eval_tile(const KdeGeom &g, int64_t n_cells, int64_t m) {
    int tile = 1;
    if (g.rcut2 > 0.0) {
        const double per_cell = (double)m / (double)n_cells;
        const double reach = 1.5 * sqrt(g.rcut2) * g.inv_cell;
        double best = INFINITY;
        for (int t = 1; t <= 64; t++) {
            const double cnt = per_cell * pow((double)t, g.dim);
            const double util = cnt / (KDE_THREADS * ceil(cnt / KDE_THREADS));
            const double cost = pow(t + 2.0 * reach, g.dim) / util;
            if (cost < best) { best = cost; tile = t; }
        }
    }
    return tile;
}

// ------------------------------------------------------------------ lattice launch shape
// Strip length R of the lattice form, 0: the points are written out.  R only if R da sqrt(max s2) <= 50 (see
// kde_lattice_kernel); `forced` (development): < 0 no limit, 0 never, else the longest strip allowed.
static inline int lattice_strip(const KdeGeom &g, double s2_max, const double *step, const int64_t *count, int forced) {
    // (rcut2 <= 138, i.e. tol >= 1e-30: the strip's middle value must stay a normal number, see the kernel)
    if (g.dim != 2 || !(g.rcut2 > 0.0) || g.rcut2 > 138.0 || count[0] * count[1] > 0x7FFFFFF0LL) return 0;
    const double da = g.U[0] * step[0];
    if (!(da > 0.0) || !std::isfinite(da) || !(s2_max > 0.0)) return 0;
    if (forced == 0) return 0;
    const double lim = 50.0 / (da * sqrt(s2_max));
    for (int R : {32, 16, 8})
        if ((double)R <= lim && (forced < 0 || R <= forced)) return R;
    return 0;
}

// Sub-patch of a wavefront: sw strips of lpw consecutive lines, sw lpw = LG lanes (the wavefront's 64 / LG lane groups
// work different shares on the same sub-patch).  A source costs one pass per sub-patch within its reach, whatever the
// number of strips it reaches there, so the sub-patch should be as compact as the kernel discs: the expected number
// of sub-patches a unit-bandwidth source touches (sources spread evenly over the lattice and its margin) picks sw for
// a given LG; LG = 8 (eight shares side by side: scripts/dev/kde_pass_model.py) unless the lattice then has more
// than 4 096 sub-patches (every sub-patch has a wavefront, partial sums and a share list of its own).
static inline int64_t lattice_patches(int R, int sw, int lpw, const int64_t *count) {
    const int64_t strips_a = (count[0] + R - 1) / R;
    return ((strips_a + sw - 1) / sw) * ((count[1] + lpw - 1) / lpw);
}

static inline void lattice_shape(const KdeGeom &g, int64_t n, int R, const double *step, const int64_t *count, int &sw_out,
                                 int &lg_out) {
    const int strips_a = (int)((count[0] + R - 1) / R);
    const double rp = sqrt(g.rcut2) / fabs(g.U[0] * step[0]), rl = sqrt(g.rcut2) / fabs(g.U[4] * step[1]);
    const double n0 = (double)count[0], n1 = (double)count[1];
    for (int lg : {8, 16, 32, 64}) {
        int best = 1;
        double best_cost = INFINITY;
        for (int sw = 1; sw <= lg; sw *= 2) {
            if (sw > 1 && sw / 2 >= strips_a) continue;
            const int lpw = lg / sw;
            double rows = 0.0, cols = 0.0;
            for (int64_t j = 0; j < count[1]; j += lpw)
                rows += std::min(1.0, (2.0 * rl + (double)std::min<int64_t>(lpw, count[1] - j)) / (n1 + 2.0 * rl));
            for (int64_t i = 0; i < count[0]; i += (int64_t)sw * R)
                cols += std::min(1.0, (2.0 * rp + (double)std::min<int64_t>((int64_t)sw * R, count[0] - i)) / (n0 + 2.0 * rp));
            const double cost = rows * cols;
            if (cost < best_cost * (1.0 - 1e-9)) { best_cost = cost; best = sw; }
        }
        sw_out = best;
        lg_out = lg;
        // (every sub-patch also has a list of the shares within reach of it, n_shares entries at most: 256 MB in all)
        const int64_t n_shares = n / LAT_SHARE + 1;
        const int64_t cap = std::min<int64_t>(4096, std::max<int64_t>(1, ((int64_t)64 << 20) / n_shares));
        if (lattice_patches(R, best, lg / best, count) <= cap || lg == 64) return;
    }
}

// Number of wavefronts of the lattice kernel: `waves` or one per patch, whichever is more, with partial sums of
// 128 MB at most.  The product's `waves` is 6 144 = TWICE the wavefronts the chip holds of this kernel (3 per SIMD):
// with exactly one resident set every SIMD's three wavefronts have equal work, the oldest is served first and the
// youngest runs the last third of the launch alone at ~40 % issue rate; with half-size wavefronts the second set
// fills in as the first finishes (round 5: 278 -> 226 us per estimator; 8 192: the same).  (The launch plan gives a
// patch no more wavefronts than it has shares within reach.)
static inline int64_t lattice_waves(int R, int sw, int lpw, const int64_t *count, int waves) {
    const int64_t patches = lattice_patches(R, sw, lpw, count);
    int64_t w = std::max<int64_t>(patches, waves);
    w = std::min<int64_t>(w, std::max<int64_t>(patches, (int64_t)(128 << 20) / (R * sw * lpw * 8)));     // partial sums <= 128 MB
    return w;
}

// ------------------------------------------------------------------ workspace sizes
// bytes of the create-time workspace that stay in use for the lifetime of the estimator
static inline size_t resident_bytes(int dim, int64_t n, int64_t n_cells) {
    auto r = [](size_t b) { return (b + 255) & ~(size_t)255; };
    return r((size_t)dim * n * 8) + 3 * r((size_t)n * 8) + r((size_t)(n_cells + 1) * 4) +
           r((size_t)n_cells * 8) + r(64) + r(64);
}

// split partial sums exist only below 1024 workgroups, i.e. below 2^19 queries
static inline size_t split_bytes(int64_t m) { return (size_t)32 * 8 * (size_t)std::min<int64_t>(m, 1 << 19); }

// `sort_temp`: what the sorts and the selection of n items ask for.  The terms for flags, starts and head keys are
// slack since the pilot's workgroups come from the cell table; the size is kept.
static inline size_t create_workspace_bytes(int dim, int64_t n_src, size_t sort_temp, int hermite_min) {
    const size_t n = (size_t)n_src;
    size_t total = resident_bytes(dim, n_src, cells_cap(n_src)) + (size_t)RED_BLOCKS * 16 * 8;   // moment partials
    total += 4 * n * 8 + n * 8 + 2 * n * 4;              // (y, weight) records, flat keys x2, idx x2
    total += n + n * 4 + n * 8;                          // flags, starts, head keys (slack)
    total += n * 8 + split_bytes(n_src);                 // pilot, split partials
    total += sort_temp + (n / Q_CHUNK + (size_t)cells_cap(n_src)) * sizeof(KdeBlock);
    if (dim == 2)   // cell -> slot map, lists of dense / non-empty cells (the coefficients live in library scratch)
        total += (n / hermite_min + 1) * 4 + (size_t)cells_cap(n_src) * 12 + 4096;   // dense list: one entry per cell at most
    return total + 64 * 256;
}

static inline size_t eval_workspace_bytes(int dim, int64_t m, size_t sort_temp) {
    size_t total = 2 * (size_t)dim * m * 8 + 2 * (size_t)m * 8 + 2 * (size_t)m * 4 + (size_t)m +
                   (size_t)m * 4 + (size_t)m * 8 + split_bytes(m) + (size_t)m * 8 + sort_temp +
                   ((size_t)m / 128 + (size_t)std::min<int64_t>(m, 1 << 22) + 16) * sizeof(KdeBlock);
    return total + 64 * 256;
}

// the lattice form: records, partial sums, share boxes, the lists of the shares within reach of each sub-patch
static inline size_t lattice_workspace_bytes(int64_t n, int R, int lg, size_t waves, size_t patches) {
    return ((size_t)n + LAT_SHARE) * LAT_GREC * 8 + waves * R * lg * 8 + ((size_t)n / LAT_SHARE + 1) * 32 +
           patches * ((size_t)n / LAT_SHARE + 1) * 4 + (patches + 1) * 8 + 4096;
}

}  // namespace pisa
