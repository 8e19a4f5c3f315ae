"""CPU: the CTU image format of kernels/ctu_image.h, from a host build of the header itself.  ctu_index and ctu_sample are inverses over all
1536 samples; the 96 sub-blocks cover every sample once and name the 8x8 tile of their origin; Region::index (and block_index) of each of the 21
quadtree nodes and the 96-lane enumeration of each 8x8 CU give exactly the samples of the node's luma square and its two chroma blocks.  The
expected sets come from ctu_index in the probe and, a second time, from the layout as the header's comment states it (luma 32 x 32 at 0, Cb and
Cr 16 x 16 at 1024 and 1280)."""
import subprocess
from collections import defaultdict
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "hevc_amd" / "csrc"

PROBE = r"""
#include <cstdio>
#include "kernels/common.h"
#include "kernels/ctu_image.h"
#include "kernels/residual.h"
using namespace mihevc;
int main()
{
    printf("N %d %d %d\n", CTU_SAMPLES, CTU_SUBBLOCKS, CU8_SAMPLES);
    for (int i = 0; i < CTU_SAMPLES; i++) {
        const CtuSample c = ctu_sample(i);
        printf("S %d %d %d %d %d %d %d\n", i, c.plane, c.x, c.y, c.stride, c.base, ctu_index(c.plane, c.x, c.y));
    }
    for (int sb = 0; sb < CTU_SUBBLOCKS; sb++) {
        const SubBlock b = sub_block(sb);
        printf("B %d %d %d %d %d %d %d\n", sb, b.plane, b.bx, b.by, b.stride, b.at, b.tile);
    }
    for (int node = 0; node < 21; node++) {
        int cx, cy, l2;
        node_geom(node, cx, cy, l2);
        const Region rg{cx, cy, l2};
        printf("G %d %d %d %d %d\n", node, cx, cy, l2, rg.count());
        for (int k = 0; k < rg.count(); k++) printf("R %d %d\n", node, rg.index(k));
        for (int k = 0; k < rg.count() / 8; k++) printf("K %d %d\n", node, rg.block_index(k));
        for (int pl = 0; pl < 3; pl++)
            for (int y = 0; y < (pl ? 1 << (l2 - 1) : 1 << l2); y++)
                for (int x = 0; x < (pl ? 1 << (l2 - 1) : 1 << l2); x++) printf("E %d %d\n", node, ctu_index(pl, (pl ? cx >> 1 : cx) + x, (pl ? cy >> 1 : cy) + y));
        if (l2 != 3) continue;
        for (int lane = 0; lane < CU8_SAMPLES; lane++) {
            const CtuSample c = cu8_sample(cx, cy, lane);
            printf("C %d %d %d %d %d %d %d\n", node, lane, c.plane, c.x, c.y, c.stride, c.base);
        }
    }
}
"""


def index_of(plane, x, y):          # the layout as documented, written out independently of the header
    return y * 32 + x if plane == 0 else 1024 + (plane - 1) * 256 + y * 16 + x


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp("ctu_layout")
    (d / "probe.cpp").write_text(PROBE)
    subprocess.run(["g++", "-std=c++17", "-O1", "-w", "-I", str(CSRC), "-o", str(d / "probe"), str(d / "probe.cpp")], check=True)
    out = subprocess.run([str(d / "probe")], capture_output=True, text=True, check=True).stdout
    r = defaultdict(list)
    for line in out.splitlines():
        f = line.split()
        r[f[0]].append([int(v) for v in f[1:]])
    return r


def test_constants(rows):
    assert rows["N"] == [[1536, 96, 96]]


def test_ctu_index_inverts_ctu_sample_for_all_samples(rows):
    assert [s[0] for s in rows["S"]] == list(range(1536))
    for i, plane, x, y, stride, base, back in rows["S"]:
        assert back == i, (i, back)
        size = 32 if plane == 0 else 16
        assert 0 <= plane < 3 and 0 <= x < size and 0 <= y < size and stride == size, (i, plane, x, y, stride)
        assert base == index_of(plane, 0, 0) and i == base + y * stride + x == index_of(plane, x, y), (i, plane, x, y, base)


def test_sub_blocks_cover_every_sample_once_and_name_their_tile(rows):
    assert [b[0] for b in rows["B"]] == list(range(96))
    seen = []
    for sb, plane, bx, by, stride, at, tile in rows["B"]:
        assert plane == (0 if sb < 64 else 1 if sb < 80 else 2), (sb, plane)               # luma first, then Cb, Cr
        assert bx % 4 == 0 and by % 4 == 0 and stride == (16 if plane else 32) and at == index_of(plane, bx, by), (sb, bx, by, stride, at)
        lx, ly = (2 * bx, 2 * by) if plane else (bx, by)                                     # the origin in luma samples
        assert tile == (ly >> 3) * 4 + (lx >> 3), (sb, tile)
        seen += [at + y * stride + x for y in range(4) for x in range(4)]
    assert sorted(seen) == list(range(1536))


def node_samples(cx, cy, log2n):
    n = 1 << log2n
    out = [index_of(0, cx + x, cy + y) for y in range(n) for x in range(n)]
    return out + [index_of(pl, (cx >> 1) + x, (cy >> 1) + y) for pl in (1, 2) for y in range(n >> 1) for x in range(n >> 1)]


def by_node(rows, key):
    d = defaultdict(list)
    for node, idx in rows[key]:
        d[node].append(idx)
    return d


def test_regions_enumerate_their_square_and_chroma_blocks(rows):
    got, blocks, want = by_node(rows, "R"), by_node(rows, "K"), by_node(rows, "E")
    sample = {s[0]: s for s in rows["S"]}
    assert len(rows["G"]) == 21
    for node, cx, cy, log2n, count in rows["G"]:
        assert count == 3 * (1 << (2 * log2n)) // 2 == len(got[node]), (node, count)
        assert len(set(got[node])) == count, node                                           # no sample twice
        assert sorted(got[node]) == sorted(want[node]) == sorted(node_samples(cx, cy, log2n)), node
        # block_index: the top-left samples of 2 x 4 blocks that tile the same region
        cover = [i + r * sample[i][4] + c for i in blocks[node] for r in range(2) for c in range(4)]
        assert len(blocks[node]) == count // 8 and sorted(cover) == sorted(want[node]), node


def test_cu8_lanes_enumerate_every_8x8_cu(rows):
    want = by_node(rows, "E")
    geom = {g[0]: g for g in rows["G"]}
    lanes = defaultdict(list)
    for node, lane, plane, x, y, stride, base in rows["C"]:
        assert lane == len(lanes[node]) and (plane == 0) == (lane < 64) and stride == (16 if plane else 32) and base == index_of(plane, 0, 0), (node, lane)
        lanes[node].append(index_of(plane, x, y))
    assert sorted(lanes) == list(range(5, 21))
    for node, idx in lanes.items():
        _, cx, cy, log2n, _ = geom[node]
        assert len(idx) == 96 == len(set(idx)) and sorted(idx) == sorted(want[node]) == sorted(node_samples(cx, cy, log2n)), node
        assert idx[:64] == [index_of(0, cx + (k & 7), cy + (k >> 3)) for k in range(64)], node      # luma in raster order: lane k is sample k of the CU
