#!/usr/bin/env python3
"""Search for a B picture in which a CU's list-1 key EQUALS its bi-prediction key while list 0 is dearer (keys[1] == keys[2] < keys[0]): the tie that holds the
order of `k1 <= k2` in `inter_b_block`.  It needs 16 (SATD_1 - SATD_bi) = lambda_sad_q4 (mv_bits_0 - 1), so it is looked for at small multiples of 16: the model of
tests/hevc_inter_cu.py alone is run (no oracle, no kernel) over the b-mix8 / b-mix16 pictures at 64x64 and 136x72, both depths, lambda_sad_q4 16 and 32, seeds
300..399, noise 1..4, and every case that has such a CU is printed with its count.  The case found this way is util.INTER_CASES' "b-tie12-..." entry.

    python tools/find_b_key_tie.py [--jobs N] [--first]"""
import argparse
import itertools
import multiprocessing
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def grid():
    for seed, noise, lam, bd, (w, h), g in itertools.product(range(300, 400), (1, 2, 3, 4), (16, 32), (8, 10), ((64, 64), (136, 72)), (8, 16)):
        yield (w, h, bd, g, seed, noise, lam)


def run(job):
    from tests import hevc_inter_cu as M
    from tests import util
    w, h, bd, g, seed, noise, lam = job
    c = util.inter_case("search", w, h, bd, 8, 27, f"b-mix{g}", seed=seed, noise=noise << (bd - 8), lam=(lam, None))
    want = util.inter_case_want.__wrapped__(c)[0]
    cov = util.INTER_COVERAGE.pop(c.id)
    return job, cov["B key tie", (M.L1, M.BI)], sum(len(t["leaves"]) for t in want.ctus)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--first", action="store_true", help="stop at the first case found")
    a = ap.parse_args()
    cus = 0
    with multiprocessing.Pool(a.jobs) as pool:
        for job, ties, n in pool.imap(run, grid(), chunksize=4):
            cus += n
            if ties:
                print("w %d h %d bit depth %d grid %d seed %d noise %d lambda_sad_q4 %d: %d CUs with list 1 == bi < list 0   (%d CUs searched so far)" % (job + (ties, cus)), flush=True)
                if a.first:
                    pool.terminate()
                    return
    print("%d CUs searched" % cus)


if __name__ == "__main__":
    main()
