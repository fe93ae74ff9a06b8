// prob3_plan_main.cpp -- runs the host decisions of the planned prob3 grid (pisa_amd/csrc/prob3_plan.hpp, and nothing
// else of the library) on cases read from a text file: one command per line, numbers separated by blanks; prints a JSON
// list with one object per command.  Built with the sanitizers and run as a child process by
// tests/test_host_prob3_plan.py.
//
//   layers   n_cz n_layers rho[n_cz n_layers] dist[n_cz n_layers]     the layer table of the commands that follow
//   launch   n_e t4 t2 ragged sorted
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <type_traits>

#include "prob3_plan.hpp"

using namespace pisa;

static std::string num(double v) {
    char buf[40];
    snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

template <class T>
static std::string list(const std::vector<T> &v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); i++) {
        if (i) s += ",";
        if (std::is_floating_point<T>::value) s += num((double)v[i]);
        else s += std::to_string((long long)v[i]);
    }
    return s + "]";
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
    Prob3LayerPlan p;
    bool have = false;
    std::string line, out = "[";
    for (int n_line = 1; std::getline(f, line); n_line++) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        std::ostringstream o;
        if (cmd == "layers") {
            int n_cz = 0, n_layers = 0;
            in >> n_cz >> n_layers;
            if (!in || n_cz < 1 || n_layers < 1) return 2;
            std::vector<double> rho((size_t)n_cz * n_layers), dist(rho.size());
            for (double &v : rho) in >> v;
            for (double &v : dist) in >> v;
            if (!in) return 2;
            prob3_layer_plan(rho.data(), dist.data(), n_cz, n_layers, p);
            have = true;
            o << "\"n_unique\":" << p.n_unique << ",\"n_pairs\":" << p.n_pairs << ",\"n_chain\":" << p.n_chain
              << ",\"n_classes\":" << p.n_classes << ",\"rho\":" << list(p.rho) << ",\"pair_u\":" << list(p.pair_u)
              << ",\"pair_dist\":" << list(p.pair_dist) << ",\"row_start\":" << list(p.row_start) << ",\"row_cnt\":"
              << list(p.row_cnt) << ",\"row_pairs\":" << list(p.row_pairs) << ",\"chain_u\":" << list(p.chain_u)
              << ",\"chain_dist\":" << list(p.chain_dist) << ",\"row_class\":" << list(p.row_class);
        } else if (cmd == "launch" && have) {
            int n_e = 0;
            Prob3PackOpts opt;
            in >> n_e >> opt.t4 >> opt.t2 >> opt.ragged >> opt.sorted;
            if (!in || n_e < 1) return 2;
            Prob3LaunchPlan l;
            const bool ok = prob3_launch_plan(p, n_e, opt, l);
            o << "\"ok\":" << (ok ? "true" : "false") << ",\"n_tiles\":" << l.n_tiles << ",\"r\":" << l.r << ",\"k\":" << l.k
              << ",\"n_blk\":" << l.n_blk << ",\"n_blk_r\":" << l.n_blk_r << ",\"n_slots\":" << l.n_slots << ",\"n_groups\":"
              << l.n_groups << ",\"slots\":" << list(l.slots) << ",\"lanes\":" << list(l.lanes) << ",\"group_rows\":"
              << list(l.group_rows);
        } else {
            fprintf(stderr, "line %d: bad command\n", n_line);
            return 2;
        }
        out += (out.size() > 1 ? ",\n" : "") + ("{\"cmd\":\"" + cmd + "\"," + o.str() + "}");
    }
    std::cout << out << "]" << std::endl;
    return 0;
}
