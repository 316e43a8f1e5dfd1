#!/usr/bin/env python3
"""What choosing among the heat-map modes by bone lengths costs on top of asking for the modes.

    python tools/skeleton_modes_probe.py [--out FILE] [--quick]          # one JSON object on stdout (and in FILE)

RN50 stride 16 h36m (synthetic weights), f16, at 64 and 256 crops.  Three arms INTERLEAVED window by window in one process:
modes (Engine.forward_modes at k = 2, radius = 1), modes + skeleton (Engine.forward_skeleton_modes on the same k and radius: one
more bind, one more launch of one wave per crop, four more small output tensors allocated per call), modes again.
The two outer arms are the same code on the same data: their relative difference (`aa_spread`) is the noise margin the middle
arm has to be read against.  Crops/s from a host clock around `iters` forwards that end in a synchronisation, after 3 warm-up
windows, median of 5 windows.  The launch's own time comes from the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/skeleton_modes_probe.py --quick --batches 64
and `--stats-csv 64=<dir>/.../*_kernel_stats.csv` (repeatable) folds that table's skeleton_modes / heat_modes rows into the JSON
under `kernels`.  Nothing gates on these figures.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from metro_pose3d_amd import ModelSpec, synth  # noqa: E402
from metro_pose3d_amd.engine import Engine  # noqa: E402


def crops_per_s(eng, x, lengths, bufs, windows, iters):
    n = x.shape[0]
    modes = lambda: eng.forward_modes(x, 2, 1, out=bufs['poses'])
    skeleton = lambda: eng.forward_skeleton_modes(x, lengths, 2, 1, out=bufs['poses'], coords01=bufs['coords01'])
    arms = (('modes', modes), ('skeleton', skeleton), ('modes_again', modes))
    res = {k: [] for k, _ in arms}
    for w in range(3 + windows):
        for name, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            if w >= 3:
                res[name].append(n * iters / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in res.items()}
    a = 0.5 * (med['modes'] + med['modes_again'])
    out = {k: {'median': round(med[k], 1), 'windows': [round(v, 1) for v in res[k]]} for k in res}
    out['aa_spread'] = round(abs(med['modes'] - med['modes_again']) / a, 4)
    out['skeleton_over_modes'] = round(med['skeleton'] / a, 4)          # < 1: the choice costs that share
    out['skeleton_extra_us_per_call'] = round((n / med['skeleton'] - n / a) * 1e6, 1)
    return out


def kernel_rows(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get('Name', '')
            if 'skeleton_modes' in name or 'heat_modes' in name:
                rows[name] = {'calls': int(r['Calls']), 'average_ns': float(r['AverageNs'])}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--quick', action='store_true', help='one short window per arm (profiler runs)')
    ap.add_argument('--batches', default='64,256', help='crops per call, comma-separated')
    ap.add_argument('--stats-csv', action='append', default=[], metavar='BATCH=FILE',
                    help='kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of --quick --batches BATCH')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('skeleton_modes_probe: no HIP device visible (there is nothing to measure on a CPU)')
    dev = torch.device('cuda', 0)
    spec = ModelSpec(50, 16, 'h36m')
    params = synth.make_params(50, spec.n_head_channels, 64, seed=0, logit_gain=synth.logit_gain_for(50, 16))
    sk = spec.skeleton
    result = {'config': 'resnet_v2_50 stride 16 h36m f16, k 2, radius 1', 'device': torch.cuda.get_device_name(0), 'batches': {}}
    for n in [int(b) for b in opts.batches.split(',')]:
        eng = Engine(spec, params, 'f16', max_batch=n, device=dev)
        x = torch.from_numpy(synth.make_images(n, spec.proc_side, seed=1)).to(dev)
        lengths = torch.from_numpy(np.random.default_rng(2).uniform(100.0, 500.0, (n, len(sk.edges)))).to(dev)
        bufs = {'poses': torch.empty((n, sk.n_out, 3), device=dev), 'coords01': torch.empty((n, sk.n_head, 3), device=dev)}
        ref = eng.forward(x).clone()
        assert torch.equal(eng.forward_skeleton_modes(x, lengths, 2, 1)[0], ref), 'poses changed with the skeleton'
        assert eng._heat_chunk() == n, 'the probe times one bound forward per call'
        iters = 2 if opts.quick else max(4, 2048 // n)
        result['batches'][str(n)] = crops_per_s(eng, x, lengths, bufs, 1 if opts.quick else 5, iters)
        eng.close()
    for item in opts.stats_csv:
        batch, path = item.split('=', 1)
        result.setdefault('kernels', {})[batch] = kernel_rows(path)
    text = json.dumps(result, indent=1, sort_keys=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
