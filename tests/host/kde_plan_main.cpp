// kde_plan_main.cpp -- runs the host decisions of the KDE (pisa_amd/csrc/kde_plan.hpp, and nothing else of the
// library) on cases read from a text file: one command per line, numbers separated by blanks; prints a JSON list with
// one object per command.  Built with the sanitizers and run as a child process by tests/test_host_kde_plan.py.
//
//   constants
//   grid     dim n bw_method tol sw h2[7] mean[3] xmin[3] xmax[3]
//   plan     cell tol n_cells n expansion hermite_min rcut2 dim
//   scratch  P reach h2l_split local_ok nd n_heads n_cells
//   hankel   reach P cell
//   split    begin end chunk
//   blocks   nc0 nc1 nc2 cell_start[nc0 nc1 nc2 + 1]
//   strip    dim rcut2 u00 s2_max step0 step1 count0 count1 forced
//   shape    n rcut2 u00 u11 R step0 step1 count0 count1
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "kde_plan.hpp"

using namespace pisa;

static std::string num(double v) {
    if (!std::isfinite(v)) return "null";
    char buf[40];
    snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

template <class T, class F>
static std::string list(const T *v, size_t n, F fmt) {
    std::string s = "[";
    for (size_t i = 0; i < n; i++) s += (i ? "," : "") + fmt(v[i]);
    return s + "]";
}
static std::string dlist(const double *v, size_t n) { return list(v, n, num); }
template <class T> static std::string ilist(const T *v, size_t n) {
    return list(v, n, [](T x) { return std::to_string((long long)x); });
}

static std::string block_list(const std::vector<KdeBlock> &blocks) {
    return list(blocks.data(), blocks.size(), [](const KdeBlock &b) {
        const long long f[6] = {b.q_begin, b.q_count, b.c0[0], b.c0[1], b.c0[2], b.head};
        for (int d = 0; d < 3; d++)
            if (b.c0[d] != b.c1[d]) return std::string("null");
        return ilist(f, 6);
    });
}

static std::string run(const std::string &cmd, std::istringstream &in) {
    std::ostringstream o;
    if (cmd == "constants") {
        o << "\"Q_CHUNK\":" << Q_CHUNK << ",\"HERMITE_MIN_SERIES\":" << HERMITE_MIN_SERIES << ",\"EXPANSION_MIN_N\":"
          << expansion_min_n << ",\"KDE_THREADS\":" << KDE_THREADS << ",\"sizeof_KdeBlock\":" << sizeof(KdeBlock);
    } else if (cmd == "grid") {
        int dim, bw_method;
        long long n;
        double tol, sw, h2[7], mean[3], xmin[3], xmax[3];
        in >> dim >> n >> bw_method >> tol >> sw;
        for (double &v : h2) in >> v;
        for (double &v : mean) in >> v;
        for (double &v : xmin) in >> v;
        for (double &v : xmax) in >> v;
        KdeBandwidth b;
        KdeGeom g;
        int64_t n_cells = 0;
        double r_cut = 0;
        const bool ok = in && bandwidth_matrix(h2, sw, n, dim, bw_method, b) &&
                        cell_grid(b.U, mean, xmin, xmax, dim, tol, n, g, n_cells, r_cut);
        o << "\"ok\":" << (ok ? "true" : "false");
        if (ok)
            o << ",\"factor\":" << num(b.factor) << ",\"norm\":" << num(b.norm) << ",\"cov\":" << dlist(b.cov, 9)
              << ",\"inv_cov\":" << dlist(b.inv_cov, 9) << ",\"U\":" << dlist(g.U, 9) << ",\"cell\":" << num(g.cell)
              << ",\"inv_cell\":" << num(g.inv_cell) << ",\"rcut2\":" << num(g.rcut2) << ",\"r_cut\":" << num(r_cut)
              << ",\"ylo\":" << dlist(g.ylo, 3) << ",\"nc\":" << ilist(g.nc, 3) << ",\"n_cells\":" << n_cells
              << ",\"order\":" << series_order(g.cell, tol);
    } else if (cmd == "plan") {
        KdeGeom g;
        memset(&g, 0, sizeof g);
        long long n_cells, n;
        double tol;
        int expansion, hmin;
        in >> g.cell >> tol >> n_cells >> n >> expansion >> hmin >> g.rcut2 >> g.dim;
        g.inv_cell = 1.0 / g.cell;
        const KdePilotPlan p = pilot_plan(g, n_cells, n, tol, expansion, hmin);
        o << "\"expand\":" << p.expand << ",\"P\":" << p.P << ",\"local_ok\":" << p.local_ok << ",\"dense_min\":"
          << p.dense_min << ",\"reach\":" << p.reach << ",\"h2l_split\":" << p.h2l_split;
    } else if (cmd == "scratch") {
        KdePilotPlan p = KdePilotPlan();
        int local_ok, nd, n_heads;
        long long n_cells;
        in >> p.P >> p.reach >> p.h2l_split >> local_ok >> nd >> n_heads >> n_cells;
        p.local_ok = local_ok != 0;
        const KdePilotScratch l = pilot_scratch(p, nd, n_heads, n_cells);
        o << "\"herm\":" << l.herm << ",\"local\":" << l.local << ",\"hankel\":" << l.hankel << ",\"V\":" << l.V
          << ",\"vflag\":" << l.vflag << ",\"bytes\":" << l.bytes;
    } else if (cmd == "hankel") {
        int reach, P;
        double cell;
        in >> reach >> P >> cell;
        const std::vector<double> h = hankel_table(reach, P, cell);
        o << "\"table\":" << dlist(h.data(), h.size());
    } else if (cmd == "split") {
        long long begin, end;
        int chunk;
        in >> begin >> end >> chunk;
        KdeBlock b = KdeBlock();
        std::vector<KdeBlock> blocks;
        split_evenly(begin, end, chunk, b, blocks);
        o << "\"blocks\":" << block_list(blocks);
    } else if (cmd == "blocks") {
        KdeGeom g;
        memset(&g, 0, sizeof g);
        in >> g.nc[0] >> g.nc[1] >> g.nc[2];
        const int64_t n_cells = (int64_t)g.nc[0] * g.nc[1] * g.nc[2];
        std::vector<int32_t> cs((size_t)n_cells + 1), cells, starts;
        for (int32_t &v : cs) in >> v;
        std::vector<KdeBlock> blocks;
        if (in) pilot_blocks(cs.data(), g, n_cells, blocks, cells, starts);
        o << "\"blocks\":" << block_list(blocks) << ",\"cells\":" << ilist(cells.data(), cells.size()) << ",\"starts\":"
          << ilist(starts.data(), starts.size());
    } else if (cmd == "strip" || cmd == "shape") {
        KdeGeom g;
        memset(&g, 0, sizeof g);
        double step[2], s2_max = 0;
        int64_t count[2];
        long long n = 0, c0, c1;
        int R = 0, forced = -1;
        if (cmd == "strip") in >> g.dim >> g.rcut2 >> g.U[0] >> s2_max >> step[0] >> step[1] >> c0 >> c1 >> forced;
        else in >> n >> g.rcut2 >> g.U[0] >> g.U[4] >> R >> step[0] >> step[1] >> c0 >> c1;
        count[0] = c0;
        count[1] = c1;
        if (cmd == "strip") o << "\"R\":" << lattice_strip(g, s2_max, step, count, forced);
        else {
            int sw = 1, lg = 64;
            lattice_shape(g, n, R, step, count, sw, lg);
            o << "\"sw\":" << sw << ",\"lg\":" << lg << ",\"patches\":" << lattice_patches(R, sw, lg / sw, count)
              << ",\"waves\":" << lattice_waves(R, sw, lg / sw, count, 6144);
        }
    } else {
        return "";
    }
    if (!in) return "";
    return "{\"cmd\":\"" + cmd + "\"," + o.str() + "}";
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s CASES\n", argv[0]);
        return 2;
    }
    std::ifstream f(argv[1]);
    if (!f) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line, out = "[";
    for (int n_line = 1; std::getline(f, line); n_line++) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        const std::string r = run(cmd, in);
        if (r.empty()) {
            fprintf(stderr, "line %d: bad command or arguments\n", n_line);
            return 2;
        }
        out += (out.size() > 1 ? ",\n" : "") + r;
    }
    std::cout << out << "]" << std::endl;
    return 0;
}
