#!/usr/bin/env python3
"""Wall-clock cost of the velocity-obstacle feasibility table (metrics.vo_table): the reference's vo.csv,
20 map_ids x 27 settings = 540 worlds x 256 positions x 630 candidates, in three batches (one per agent count).

Per run and per batch the seconds of metrics.vo_feasibility_batch(timings=...): building the worlds (`build_s`: on the host one
after the other, or on the device), the three launches (`geometry_s`, `cones_s`, `count_s`), the D2H / math.asin / H2D round trip
between the first two (`asin_s`: only with --asin host; with --asin device the half angle is taken inside the cones launch, asin_s
is 0 and cones_s covers both) and the host post-processing (`post_s`), each with a device synchronise on both sides -- the
synchronisation of sweeps.survivability_batch(timings=...).  One small table is computed untimed first (code objects, allocator);
then the runs alternate between worlds='device' and host worlds and, with --asin both, between the host and the device asin inside
each of those.  Every run is kept, not a best-of; every run's table must equal the first one's.  The reference's own seconds
per env_metrics(index) call are those the recorder measured when it wrote tests/golden/vo_feasibility.npz (one world each, on the
recording machine's CPU); the table's three fixture entries are checked against the recorded means on the way.

python tools/vo_bench.py --asin both --out profiles/vo_device_asin.json"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--maps', type=int, default=20, help='map_ids 0 .. maps - 1 (the published table: 20)')
    ap.add_argument('--asin', choices=('host', 'device', 'both'), default='device', help='where the cone\'s half angle is taken')
    ap.add_argument('--out', help='write the result here (JSON)')
    args = ap.parse_args()
    import numpy as np
    import torch
    import drone2d_amd  # noqa: F401
    from drone2d_amd import _lib, metrics, sweeps
    hip = _lib.HipBackend()
    paths = ('host', 'device') if args.asin == 'both' else (args.asin,)
    for asin in paths:
        metrics.vo_table(range(1), backend=hip, asin=asin)
        metrics.vo_table(range(1), backend=hip, worlds='device', asin=asin)
    runs = []
    table = None
    for rep in range(args.reps):
        for worlds in ('device', None):
            for asin in paths:
                tm = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = metrics.vo_table(range(args.maps), backend=hip, worlds=worlds, timings=tm, asin=asin)
                torch.cuda.synchronize()
                total = time.perf_counter() - t0
                assert table is None or got == table, (rep, worlds, asin)
                table = got
                rec = dict(rep=rep, worlds='device' if worlds else 'host', asin=asin, n_worlds=tm['worlds'], total_s=total,
                           **{k: tm[k] for k in ('build_s', 'geometry_s', 'asin_s', 'cones_s', 'count_s', 'post_s')}, batches=tm['batches'])
                runs.append(rec)
                print(json.dumps({k: v for k, v in rec.items() if k != 'batches'}), flush=True)
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'vo_feasibility.npz'))
    order = sweeps._table_order(range(args.maps), (10, 20, 30), (5, 10, 15), (20, 40, 60))
    ref = []
    for i in range(int(z['n'])):
        index = json.loads(str(z[f's{i}_index']))
        k = order.index(index) if index in order else None
        same = None if k is None else bool(float(table[k // 27][k % 27]).hex() == float(z[f's{i}_mean']).hex())
        assert same is not False, index
        ref.append(dict(index=index, reference_seconds=float(z[f's{i}_ref_seconds']), mean=float(z[f's{i}_mean']), table_entry_equal=same))
    result = dict(tool='tools/vo_bench.py', reps=args.reps, asin=args.asin, settings=len(order), positions=256, candidates=630,
                  device=torch.cuda.get_device_name(0), reference=ref, runs=runs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
