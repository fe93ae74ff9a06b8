// prob3_plan.hpp -- what the host decides for the planned prob3 grid of prob3_planned.hip, as plain C++17: the
// reference's layer-matrix cache resolved per coszen row, the distinct densities, the pairs and every row's chain
// (prob3_layer_plan), the rows' classes, and for a given number of energies the list of workgroups the chain kernel
// is launched with (prob3_launch_plan): rows packed by their length into four-wave workgroups, the rows of one class
// packed side by side into the lanes of a ragged last energy tile, longest rows first.  No HIP header and no
// environment: the development knobs of prob3_planned.hip come in as arguments.  tests/host/prob3_plan_main.cpp runs
// this file alone under the sanitizers (tests/test_host_prob3_plan.py).
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

namespace pisa {

// ------------------------------------------------------------------ layers -> pairs, chains, classes
struct Prob3LayerPlan {
    int n_cz = 0, n_layers = 0;
    int n_unique = 0;                  // distinct densities (rho has max(n_unique, 1) entries)
    int n_pairs = 0, n_chain = 0;
    std::vector<double> rho;           // [n_unique] distinct densities, in order of first appearance
    std::vector<int32_t> pair_u;       // [n_pairs] distinct-density index of each pair; pairs sorted by density
    std::vector<double> pair_dist;     // [n_pairs] (cache-resolved) layer length of each pair
    std::vector<int32_t> row_start;    // [n_cz] first chain entry of the row
    std::vector<int32_t> row_cnt;      // [n_cz] crossed layers of the row
    std::vector<int32_t> row_pairs;    // [n_chain] pair index per crossed layer, in path order
    std::vector<int32_t> chain_u;      // [n_chain] density index per chain entry
    std::vector<double> chain_dist;    // [n_chain] layer length per chain entry
    std::vector<int32_t> row_class;    // [n_cz] rows of one class run the same steps on other layer lengths
    int n_classes = 0;
};

// `rho`, `dist`: [n_cz][n_layers] densities and lengths of the layers of every row (length <= 0: not crossed)
static inline void prob3_layer_plan(const double *rho, const double *dist, int n_cz, int n_layers, Prob3LayerPlan &p) {
    const size_t n = (size_t)n_cz * n_layers;
    p = Prob3LayerPlan();
    p.n_cz = n_cz;
    p.n_layers = n_layers;
    p.row_start.resize(n_cz);
    p.row_cnt.resize(n_cz);
    std::vector<double> pdist, uniq;
    std::vector<int32_t> pu, chain, layer_pair(n_layers);
    pdist.reserve(n); pu.reserve(n); chain.reserve(n);
    int nu = 0, np = 0, nc = 0;
    for (int r = 0; r < n_cz; r++) {
        const double *rr = rho + (size_t)r * n_layers, *dd = dist + (size_t)r * n_layers;
        p.row_start[r] = nc;
        for (int i = 0; i < n_layers; i++) {
            layer_pair[i] = -1;
            if (!(dd[i] > 0.0)) continue;
            // follow the reference's cache matches (numba_osc_kernels.py:236-249)
            // to the layer whose matrix is actually computed
            int cur = i;
            double cr = rr[i], cd = dd[i];
            while (true) {
                int found = -1;
                for (int j = 0; j < cur; j++)
                    if (dd[j] > 0.0 && fabs(rr[j] - cr) < 1e-5 && fabs(dd[j] - cd) < 1e-5) found = j;
                if (found < 0) break;
                cur = found; cr = rr[cur]; cd = dd[cur];
            }
            if (cur != i) {
                layer_pair[i] = layer_pair[cur];  // the same matrix, stored once
            } else {
                int u = -1;
                for (int k = 0; k < nu; k++)
                    if (uniq[k] == cr) { u = k; break; }
                if (u < 0) { u = nu++; uniq.push_back(cr); }
                pu.push_back(u);
                pdist.push_back(cd);
                layer_pair[i] = np++;
            }
            chain.push_back(layer_pair[i]);
            nc++;
        }
        p.row_cnt[r] = nc - p.row_start[r];
    }
    // renumber the pairs sorted by density so that an item is a run of consecutive pairs
    std::vector<int32_t> order, newid(np);
    order.reserve(np);
    for (int u = 0; u < nu; u++)
        for (int k = 0; k < np; k++)
            if (pu[k] == u) order.push_back(k);
    p.pair_u.resize(np);
    p.pair_dist.resize(np);
    for (int k = 0; k < np; k++) { newid[order[k]] = k; p.pair_dist[k] = pdist[order[k]]; p.pair_u[k] = pu[order[k]]; }
    for (int k = 0; k < nc; k++) chain[k] = newid[chain[k]];
    p.n_unique = nu > 0 ? nu : 1;
    if (nu == 0) uniq.push_back(0.0);
    p.rho = uniq;
    p.n_pairs = np;
    p.n_chain = nc;
    p.row_pairs = chain;
    p.chain_u.resize(nc);
    p.chain_dist.resize(nc);
    for (int k = 0; k < nc; k++) { p.chain_u[k] = p.pair_u[chain[k]]; p.chain_dist[k] = p.pair_dist[chain[k]]; }
    // Classes.  The chain kernel's scalar decisions of a row are its chain length, the density index of every chain
    // entry and, per step s, whether the out-going layer mid + s has the matrix of the in-going layer mid - s (one
    // load feeds both products).  Rows equal in all three run the same instructions and differ in layer lengths only.
    std::map<std::vector<int32_t>, int> classes;
    p.row_class.resize(n_cz);
    for (int r = 0; r < n_cz; r++) {
        const int k0 = p.row_start[r], cnt = p.row_cnt[r], mid = cnt >> 1;
        std::vector<int32_t> key(p.chain_u.begin() + k0, p.chain_u.begin() + k0 + cnt);
        for (int s = 1; s <= mid; s++)
            key.push_back(mid + s < cnt ? (chain[k0 + mid + s] == chain[k0 + mid - s] ? 1 : 0) : -1);
        auto it = classes.find(key);
        if (it == classes.end()) it = classes.emplace(key, (int)classes.size()).first;
        p.row_class[r] = it->second;
    }
    p.n_classes = (int)classes.size();
}

// ------------------------------------------------------------------ the chain kernel's workgroups
// A workgroup of the packed chain launch has four waves and holds `units` by their length: one long unit split over
// four waves, two medium units over two waves each, or four short units with a wave each.  A unit is a row on a full
// energy tile (64 energies = the wave's lanes).  On a RAGGED last tile of r = n_e mod 64 energies, 0 < r <= 32, a unit
// is a group of up to k = 64 / r rows of one class, lane = row-in-group x r + energy: the waves of the tile issue for
// k rows what they issued for one.
//
// A wave's record is four words:
//   code   unit | wave-of-unit << 16 | waves-of-unit << 24, or -1: idle wave.  unit = the row (full tile), the group
//          (ragged tile: index into `lanes`)
//   k0     first chain entry of the row (ragged: of the group's first row, for the scalar look-ups)
//   cnt    chain length
//   tile   energy tile | PROB3_RAGGED_BIT
// `slots` lists the workgroups of one (point, sign) in launch order, 16 words each.
constexpr int32_t PROB3_RAGGED_BIT = 1 << 30;
constexpr int PROB3_MAX_PACKED_ROWS = 0xffff;   // the code's unit field

struct Prob3PackOpts {
    // crossed layers from which a unit gets four / two waves.  Measured again on the fused-amplitude form, headline
    // step: t4 = 16, 18, 20 and t2 = 4 (one wave for the rows of one step, 306 workgroups instead of 386), t2 = 6
    // all lie within the run-to-run spread of 14 / 0 (EXPERIMENTS R11-1)
    int t4 = 14, t2 = 0;
    int ragged = 1;        // pack the rows of a class into the lanes of a ragged last tile
    int sorted = 1;        // units by falling chain length before they are packed, workgroups of all tiles in that order;
                           // 0: units in row order, workgroups tile by tile
};

struct Prob3LaunchPlan {
    int n_e = 0, n_tiles = 0;
    int r = 0, k = 0;               // ragged tile: live energies and rows per wave (0: no ragged tile)
    int n_blk = 0, n_blk_r = 0;     // row blocks of a full tile / of the ragged tile
    int n_slots = 0, n_groups = 0;
    std::vector<int32_t> slots;     // [n_slots][4 waves][4]
    std::vector<int32_t> lanes;     // [n_groups][64][2]: row | energy-in-tile << 16 (-1: dead lane), first chain entry
    std::vector<int32_t> group_rows;  // [n_groups][k] rows of each group (-1: none), for tests
};

static inline int prob3_waves_of(int cnt, const Prob3PackOpts &o) {
    return cnt >= o.t4 ? 4 : (cnt >= o.t2 ? 2 : 1);
}

struct Prob3Unit { int32_t id, k0, cnt; };

// units -> blocks of 16 words (tile word 0), in the order given: first the units of four waves, then of two, then of one
static inline void prob3_pack_blocks(const std::vector<Prob3Unit> &units, const Prob3PackOpts &o, std::vector<int32_t> &blocks) {
    blocks.clear();
    for (int want = 4; want >= 1; want >>= 1) {
        int fill = 0;  // wave slots used in the open workgroup
        for (const Prob3Unit &u : units) {
            if (prob3_waves_of(u.cnt, o) != want) continue;
            if (fill == 0) blocks.resize(blocks.size() + 16, 0);
            for (int gi = 0; gi < want; gi++) {
                int32_t *w = blocks.data() + blocks.size() - 16 + (size_t)(fill + gi) * 4;
                w[0] = u.id | (gi << 16) | (want << 24); w[1] = u.k0; w[2] = u.cnt; w[3] = 0;
            }
            fill += want;
            if (fill == 4) fill = 0;
        }
        for (int k = fill; fill > 0 && k < 4; k++) {
            int32_t *w = blocks.data() + blocks.size() - 16 + (size_t)k * 4;
            w[0] = -1; w[1] = w[2] = w[3] = 0;
        }
    }
}

// false: more rows than the packed form indexes (the caller launches one row per workgroup)
static inline bool prob3_launch_plan(const Prob3LayerPlan &p, int n_e, const Prob3PackOpts &o, Prob3LaunchPlan &l) {
    l = Prob3LaunchPlan();
    l.n_e = n_e;
    l.n_tiles = (n_e + 63) / 64;
    if (p.n_cz > PROB3_MAX_PACKED_ROWS) return false;
    const int r = n_e % 64;
    const bool ragged = o.ragged && r > 0 && r <= 32;
    const int full_tiles = ragged ? l.n_tiles - 1 : l.n_tiles;
    auto by_length = [](const Prob3Unit &a, const Prob3Unit &b) { return a.cnt > b.cnt; };
    // full tiles: a unit is a row
    std::vector<Prob3Unit> units;
    for (int row = 0; row < p.n_cz; row++) units.push_back({row, p.row_start[row], p.row_cnt[row]});
    if (o.sorted) std::stable_sort(units.begin(), units.end(), by_length);
    std::vector<int32_t> blk, blk_r;
    if (full_tiles > 0) prob3_pack_blocks(units, o, blk);
    l.n_blk = (int)(blk.size() / 16);
    if (ragged) {
        // the ragged tile: the rows of a class, in row order, k at a time
        l.r = r;
        l.k = 64 / r;
        std::vector<std::vector<int>> rows_of(p.n_classes);
        for (int row = 0; row < p.n_cz; row++) rows_of[p.row_class[row]].push_back(row);
        std::vector<std::vector<int>> groups;   // in the order of their first rows
        for (int c = 0; c < p.n_classes; c++)
            for (size_t i = 0; i < rows_of[c].size(); i += l.k)
                groups.emplace_back(rows_of[c].begin() + i, rows_of[c].begin() + std::min(rows_of[c].size(), i + l.k));
        std::sort(groups.begin(), groups.end());
        l.n_groups = (int)groups.size();
        l.lanes.assign((size_t)l.n_groups * 128, 0);
        l.group_rows.assign((size_t)l.n_groups * l.k, -1);
        units.clear();
        for (int g = 0; g < l.n_groups; g++) {
            const int row0 = groups[g][0];
            units.push_back({g, p.row_start[row0], p.row_cnt[row0]});
            for (int lane = 0; lane < 64; lane++) {
                const int j = lane / r, e = lane % r;
                const bool live = j < (int)groups[g].size();
                l.lanes[((size_t)g * 64 + lane) * 2] = live ? (groups[g][j] | (e << 16)) : -1;
                l.lanes[((size_t)g * 64 + lane) * 2 + 1] = live ? p.row_start[groups[g][j]] : 0;
            }
            for (size_t j = 0; j < groups[g].size(); j++) l.group_rows[(size_t)g * l.k + j] = groups[g][j];
        }
        if (o.sorted) std::stable_sort(units.begin(), units.end(), by_length);
        prob3_pack_blocks(units, o, blk_r);
        l.n_blk_r = (int)(blk_r.size() / 16);
    }
    // launch order.  Sorted: longest first over all tiles, (chain length of the block's first wave, block, tile).
    // Else tile by tile, the blocks of a tile as they were packed.
    struct Slot { int32_t cnt, ragged, b, tile; };
    std::vector<Slot> order;
    if (o.sorted) {
        for (int b = 0; b < l.n_blk; b++)
            for (int t = 0; t < full_tiles; t++) order.push_back({blk[(size_t)b * 16 + 2], 0, b, t});
    } else {
        for (int t = 0; t < full_tiles; t++)
            for (int b = 0; b < l.n_blk; b++) order.push_back({blk[(size_t)b * 16 + 2], 0, b, t});
    }
    for (int b = 0; b < l.n_blk_r; b++) order.push_back({blk_r[(size_t)b * 16 + 2], 1, b, full_tiles});
    if (o.sorted) std::stable_sort(order.begin(), order.end(), [](const Slot &a, const Slot &b) { return a.cnt > b.cnt; });
    l.n_slots = (int)order.size();
    l.slots.resize((size_t)l.n_slots * 16);
    for (int s = 0; s < l.n_slots; s++) {
        const int32_t *src = (order[s].ragged ? blk_r.data() : blk.data()) + (size_t)order[s].b * 16;
        int32_t *dst = l.slots.data() + (size_t)s * 16;
        for (int w = 0; w < 4; w++) {
            for (int i = 0; i < 3; i++) dst[4 * w + i] = src[4 * w + i];
            dst[4 * w + 3] = order[s].tile | (order[s].ragged ? PROB3_RAGGED_BIT : 0);
        }
    }
    return true;
}

}  // namespace pisa
