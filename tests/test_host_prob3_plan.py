"""The host decisions of the planned prob3 grid (pisa_amd/csrc/prob3_plan.hpp) without a GPU:
tests/host/prob3_plan_main.cpp, which includes that header and nothing else of the library, is built with
AddressSanitizer and UBSan and run as a child process on PREM-12 layer tables; the packing it prints is checked lane by
lane, and against a restatement of the packing the library had before the header (rows in row order, four / two waves
from 14 / 0 crossed layers, every tile alike)."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_E = (1, 8, 63, 64, 65, 72, 96, 97, 200)
N_CZ = (1, 7, 20, 100)
RAGGED_BIT = 1 << 30
NEW = (14, 0, 1, 1)       # t4, t2, ragged, sorted: the library's defaults
OLD = (14, 0, 0, 0)
RAGGED_ONLY = (14, 0, 1, 0)
T2_4 = (14, 4, 1, 1)      # rows of fewer than four layers on one wave, four to a workgroup (development knob)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("prob3_plan")
    exe = str(d / "prob3_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "pisa_amd", "csrc"), os.path.join(ROOT, "tests", "host", "prob3_plan_main.cpp"), "-o", exe],
                   check=True)
    count = [0]

    def run(lines):
        count[0] += 1
        path = str(d / ("cases%d.txt" % count[0]))
        with open(path, "w") as f:
            f.write("".join(" ".join(repr(float(v)) if isinstance(v, float) else str(v) for v in line) + "\n" for line in lines))
        p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, p.stderr.decode()[-4000:]
        out = json.loads(p.stdout)
        assert len(out) == len(lines)
        return out

    return run


@pytest.fixture(scope="module")
def tables(oracle):
    """n_cz -> (densities, distances) of n_cz bin centres in coszen over [-1, 1], PREM 12 layers"""
    from pisa_amd.utils.resources import find_resource

    out = {}
    for n_cz in N_CZ:
        edges = np.linspace(-1.0, 1.0, n_cz + 1)
        lay = oracle.Layers(np.loadtxt(find_resource("osc/PREM_12layer.dat")), 2.0, 20.0)
        lay.setElecFrac(0.4656, 0.4656, 0.4957)
        lay.calcLayers(0.5 * (edges[1:] + edges[:-1]))
        out[n_cz] = (np.asarray(lay.density, dtype=float).reshape(n_cz, -1), np.asarray(lay.distance, dtype=float).reshape(n_cz, -1))
    return out


@pytest.fixture(scope="module")
def results(plan, tables):
    """(n_cz, n_e, opts) -> launch plan; n_cz -> layer plan"""
    layers, launches = {}, {}
    for n_cz in N_CZ:
        dens, dist = tables[n_cz]
        lines = [("layers", n_cz, dens.shape[1], *[float(v) for v in dens.ravel()], *[float(v) for v in dist.ravel()])]
        keys = [(n_e, opts) for n_e in N_E for opts in (NEW, OLD, RAGGED_ONLY, T2_4)]
        lines += [("launch", n_e, *opts) for n_e, opts in keys]
        got = plan(lines)
        layers[n_cz] = got[0]
        for (n_e, opts), g in zip(keys, got[1:]):
            launches[n_cz, n_e, opts] = g
    return layers, launches


def _waves(launch):
    """(slot, wave, unit, g, groups, k0, cnt, tile, ragged) of every wave that is not idle"""
    rec = np.reshape(launch["slots"], (-1, 4, 4))
    for s in range(rec.shape[0]):
        for w in range(4):
            code, k0, cnt, tile = (int(v) for v in rec[s, w])
            if code < 0:
                assert code == -1
                continue
            yield s, w, code & 0xffff, (code >> 16) & 0xff, (code >> 24) & 0xff, k0, cnt, tile & ~RAGGED_BIT, bool(tile & RAGGED_BIT)


def _old_packing(row_start, row_cnt, t4=14, t2=0):
    """the block list of pisa_hip_grid_plan_create before the header, word for word (fourth word 0)"""
    out = []
    for want in (4, 2, 1):
        fill = 0
        for r, c in enumerate(row_cnt):
            if (4 if c >= t4 else (2 if c >= t2 else 1)) != want:
                continue
            if fill == 0:
                out.append([[-1, 0, 0, 0] for _ in range(4)])
            for gi in range(want):
                out[-1][fill + gi] = [r | gi << 16 | want << 24, row_start[r], c, 0]
            fill = (fill + want) % 4
    return out


def test_layer_plan(results, tables):
    """pairs, chains and classes: every crossed layer has a chain entry of its density and (cache-resolved) length;
    rows of a class agree in everything the kernel takes from scalars"""
    layers, _ = results
    for n_cz in N_CZ:
        dens, dist = tables[n_cz]
        p = layers[n_cz]
        rho, chain_u, chain_dist, pairs = np.array(p["rho"]), p["chain_u"], p["chain_dist"], p["row_pairs"]
        assert p["n_chain"] == int((dist > 0).sum()) == len(chain_u)
        assert sorted(p["pair_u"]) == p["pair_u"]
        seen = {}
        for r in range(n_cz):
            k0, cnt = p["row_start"][r], p["row_cnt"][r]
            live = np.nonzero(dist[r] > 0)[0]
            assert cnt == len(live)
            for i, layer in enumerate(live):
                assert abs(rho[chain_u[k0 + i]] - dens[r, layer]) < 1e-5 and abs(chain_dist[k0 + i] - dist[r, layer]) < 1e-5
                assert p["pair_u"][pairs[k0 + i]] == chain_u[k0 + i] and p["pair_dist"][pairs[k0 + i]] == chain_dist[k0 + i]
            mid = cnt // 2
            mirror = [pairs[k0 + mid + s] == pairs[k0 + mid - s] if mid + s < cnt else None for s in range(1, mid + 1)]
            key = (tuple(chain_u[k0:k0 + cnt]), tuple(mirror))
            assert seen.setdefault(key, p["row_class"][r]) == p["row_class"][r]
        assert len(seen) == p["n_classes"] == len(set(p["row_class"]))


@pytest.mark.parametrize("n_cz", N_CZ)
@pytest.mark.parametrize("n_e", N_E)
@pytest.mark.parametrize("opts", [NEW, T2_4])
def test_every_node_once(results, n_cz, n_e, opts):
    layers, launches = results
    p, l = layers[n_cz], launches[n_cz, n_e, opts]
    assert l["ok"] and l["n_tiles"] == -(-n_e // 64)
    r = n_e % 64
    if 0 < r <= 32:
        assert (l["r"], l["k"]) == (r, 64 // r)
    else:
        assert (l["r"], l["k"], l["n_groups"], l["n_blk_r"]) == (0, 0, 0, 0)
    lanes = np.reshape(l["lanes"], (-1, 64, 2))
    groups = np.reshape(l["group_rows"], (-1, max(l["k"], 1)))
    hits = np.zeros((n_cz, n_e), dtype=int)
    leaders = {}
    slot_len = {}
    for s, w, unit, g, n_g, k0, cnt, tile, ragged in _waves(l):
        slot_len.setdefault(s, cnt)
        assert n_g in (1, 2, 4) and g < n_g
        assert n_g == (4 if cnt >= opts[0] else (2 if cnt >= opts[1] else 1))
        leaders.setdefault((s, unit, tile), []).append((w, g))
        if g:
            continue
        if not ragged:
            assert l["r"] == 0 or tile < l["n_tiles"] - 1
            assert (k0, cnt) == (p["row_start"][unit], p["row_cnt"][unit])
            hits[unit, tile * 64:min(n_e, tile * 64 + 64)] += 1
            continue
        assert tile == l["n_tiles"] - 1 and l["r"] > 0
        rows = [int(x) for x in groups[unit] if x >= 0]
        assert 1 <= len(rows) <= l["k"]
        assert (k0, cnt) == (p["row_start"][rows[0]], p["row_cnt"][rows[0]])
        for row in rows:        # one class: chain length, density sequence and mirror pattern
            assert p["row_class"][row] == p["row_class"][rows[0]] and p["row_cnt"][row] == cnt
            a, b = p["row_start"][row], p["row_start"][rows[0]]
            assert p["chain_u"][a:a + cnt] == p["chain_u"][b:b + cnt]
        for lane in range(64):   # the wave codes decode back to the rows
            x, start = (int(v) for v in lanes[unit, lane])
            j, e = divmod(lane, l["r"])
            if j < len(rows):
                assert (x & 0xffff, x >> 16, start) == (rows[j], e, p["row_start"][rows[j]])
                hits[rows[j], tile * 64 + e] += 1
            else:
                assert x == -1
    assert np.all(hits == 1)
    for (s, unit, tile), ws in leaders.items():     # the waves of a unit: consecutive, in order, in one workgroup
        assert [g for _, g in ws] == list(range(len(ws))) and [w for w, _ in ws] == list(range(ws[0][0], ws[0][0] + len(ws)))
    order = [slot_len[s] for s in sorted(slot_len)]
    assert order == sorted(order, reverse=True)      # longest rows first
    assert len(order) == l["n_slots"] == l["n_blk"] * (l["n_tiles"] - (1 if l["r"] else 0)) + l["n_blk_r"]


@pytest.mark.parametrize("n_cz", N_CZ)
def test_unpacked_energies_keep_the_old_packing(results, n_cz):
    """n_e = 64 and 97 (r = 0, r = 33): the ragged packing alone changes no word; every n_e: with every option off the
    slots are the earlier block list, tile by tile.  With the library's defaults the ORDER is another one at every n_e
    (longest rows first: rows sorted before they are packed, blocks of all tiles in one sequence), so for 64 and 97 the
    claim is no more than: no ragged block, and the slots are the blocks of the sorted rows, each once per tile, every
    one a block the old rule forms from those rows (four waves from 14 layers, two below, no row twice)"""
    layers, launches = results
    p = layers[n_cz]
    old = _old_packing(p["row_start"], p["row_cnt"])
    for n_e in N_E:
        l = launches[n_cz, n_e, OLD]
        tiles = -(-n_e // 64)
        want = [[w[:3] + [t] for w in b] for t in range(tiles) for b in old]
        assert np.reshape(l["slots"], (-1, 4, 4)).tolist() == want
        assert (l["n_blk"], l["n_blk_r"], l["lanes"]) == (len(old), 0, [])
    for n_e in (64, 97):
        assert launches[n_cz, n_e, RAGGED_ONLY]["slots"] == launches[n_cz, n_e, OLD]["slots"]
        new = launches[n_cz, n_e, NEW]
        assert new["n_blk_r"] == 0 and new["lanes"] == []
        tiles = -(-n_e // 64)
        per_tile = {}
        for b in np.reshape(new["slots"], (-1, 4, 4)).tolist():
            assert len({w[3] for w in b}) == 1 and 0 <= b[0][3] < tiles
            per_tile.setdefault(b[0][3], []).append([w[:3] for w in b])
        assert sorted(per_tile) == list(range(tiles))
        for t in range(tiles):       # every tile has the same blocks, and they hold every row once, by the old rule
            assert sorted(per_tile[t]) == sorted(per_tile[0]) and len(per_tile[t]) == len(old)
        rows = []
        for b in per_tile[0]:
            for w, (code, k0, cnt) in enumerate(b):
                if code < 0:
                    continue
                row, g, n_g = code & 0xffff, (code >> 16) & 0xff, (code >> 24) & 0xff
                assert (k0, cnt, n_g) == (p["row_start"][row], p["row_cnt"][row], 4 if cnt >= 14 else 2)
                assert b[w - g][0] & 0xffff == row
                rows += [row] if g == 0 else []
        assert sorted(rows) == list(range(n_cz))


def test_headline_grid_counts(results):
    """200 x 100, PREM 12: 19 rows of >= 14 layers and 81 shorter ones made 60 row blocks per tile; the ragged fourth
    tile (8 energies, 8 rows per wave) takes far fewer"""
    layers, launches = results
    cnt = np.array(layers[100]["row_cnt"])
    old, new = launches[100, 200, OLD], launches[100, 200, NEW]
    assert old["n_blk"] == int((cnt >= 14).sum()) + -(-int((cnt < 14).sum()) // 2)
    assert old["n_slots"] == 4 * old["n_blk"]
    assert (new["r"], new["k"]) == (8, 8)
    assert new["n_blk"] == old["n_blk"] and new["n_blk_r"] <= old["n_blk"] // 4
    assert new["n_slots"] == 3 * new["n_blk"] + new["n_blk_r"]
    print("headline: classes", np.bincount(layers[100]["row_class"]).tolist(), "old n_blk", old["n_blk"], "slots", old["n_slots"],
          "new n_blk", new["n_blk"], "n_blk_r", new["n_blk_r"], "slots", new["n_slots"])
