#!/usr/bin/env python3
"""What asking for the heat-map moments costs, and that not asking costs nothing.

    python tools/heat_moments_probe.py [--out FILE] [--quick]          # one JSON object on stdout (and in FILE)

RN50 stride 16 h36m (synthetic weights), f16, at 64 and 256 crops.  Three arms INTERLEAVED window by window in one process:
plain (Engine.forward), moments (Engine.forward with cov01 / peak), plain again.  The two plain arms are the same code on the
same data: their relative difference (`aa_spread`) is the noise margin the moments arm has to be read against.  Crops/s from a
host clock around `iters` forwards that end in a synchronisation, after 3 warm-up windows, median of 5 windows.
Per-launch times of the head and finalize kernels come from the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/heat_moments_probe.py --quick
and `--stats-csv <dir>/.../*_kernel_stats.csv` folds that table's head_f16 / softargmax_finalize rows into the JSON.
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

import torch  # noqa: E402

from metro_pose3d_amd import ModelSpec, synth  # noqa: E402
from metro_pose3d_amd.engine import Engine  # noqa: E402


def crops_per_s(eng, x, bufs, windows, iters):
    n = x.shape[0]
    plain = lambda: eng.forward(x, out=bufs['poses'])
    moments = lambda: eng.forward(x, out=bufs['poses'], cov01=bufs['cov01'], peak=bufs['peak'])
    arms = (('plain', plain), ('moments', moments), ('plain_again', plain))
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
    a = 0.5 * (med['plain'] + med['plain_again'])
    out = {k: {'median': round(med[k], 1), 'windows': [round(v, 1) for v in res[k]]} for k in res}
    out['aa_spread'] = round(abs(med['plain'] - med['plain_again']) / a, 4)
    out['moments_over_plain'] = round(med['moments'] / a, 4)          # < 1: asking for the moments costs that share
    return out


def kernel_rows(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get('Name', '')
            if 'head_f16' in name or 'softargmax_finalize' in name:
                rows[name] = {'calls': int(r['Calls']), 'average_ns': float(r['AverageNs'])}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--quick', action='store_true', help='one short window per arm (profiler runs)')
    ap.add_argument('--stats-csv', default=None, help='kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of --quick')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('heat_moments_probe: no HIP device visible (there is nothing to measure on a CPU)')
    dev = torch.device('cuda', 0)
    spec = ModelSpec(50, 16, 'h36m')
    params = synth.make_params(50, spec.n_head_channels, 64, seed=0, logit_gain=synth.logit_gain_for(50, 16))
    sk = spec.skeleton
    result = {'config': 'resnet_v2_50 stride 16 h36m f16', 'device': torch.cuda.get_device_name(0), 'batches': {}}
    for n in (64, 256):
        eng = Engine(spec, params, 'f16', max_batch=n, device=dev)
        x = torch.from_numpy(synth.make_images(n, spec.proc_side, seed=1)).to(dev)
        bufs = {'poses': torch.empty((n, sk.n_out, 3), device=dev), 'cov01': torch.empty((n, sk.n_head, 6), device=dev),
                'peak': torch.empty((n, sk.n_head), device=dev)}
        ref = eng.forward(x).clone()
        assert torch.equal(eng.forward(x, cov01=bufs['cov01'], peak=bufs['peak']), ref), 'poses changed with the moments'
        iters = 2 if opts.quick else max(4, 2048 // n)
        result['batches'][str(n)] = crops_per_s(eng, x, bufs, 1 if opts.quick else 5, iters)
        eng.close()
    if opts.stats_csv:
        result['kernels'] = kernel_rows(opts.stats_csv)
    text = json.dumps(result, indent=1, sort_keys=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
