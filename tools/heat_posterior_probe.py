#!/usr/bin/env python3
"""What asking for the heat-map posterior costs, and that not asking costs nothing.

    python tools/heat_posterior_probe.py [--out FILE] [--quick]              # one JSON object on stdout (and in FILE)

RN50 stride 16 h36m (synthetic weights), f16, at 64 and 256 crops.  Three arms INTERLEAVED window by window in one process:
plain (Engine.forward), bound (Engine.forward_posterior with a random positive definite prior per joint: the head also stores its
fp32 logits, one more launch, one small output tensor allocated per call), plain again.
The two plain arms are the same code on the same data: their relative difference (`aa_spread`) is the noise margin the bound
arm has to be read against.  Crops/s from a host clock around `iters` forwards that end in a synchronisation, after 3 warm-up
windows, median of 5 windows.
Per-launch times of the new kernel (and of the head, whose launch gains the logits store) come from the profiler, in a run of
its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/heat_posterior_probe.py --quick --batches 64
(one batch per run: the table averages over all launches of a kernel), and `--stats-csv 64=<dir>/.../*_kernel_stats.csv`
(repeatable) folds that table's heat_posterior / head_f16 rows into the JSON under `kernels`.
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


def random_prior(n, nj, dev):
    rng = np.random.default_rng(2)
    a = rng.standard_normal((n, nj, 3, 3))
    lam = np.einsum('...ab,...cb->...ac', a, a) * 40.0
    words = np.stack([lam[..., 0, 0], lam[..., 1, 1], lam[..., 2, 2], lam[..., 0, 1], lam[..., 0, 2], lam[..., 1, 2]], -1)
    return torch.from_numpy(np.concatenate([rng.uniform(0, 1, (n, nj, 3)), words], -1).astype(np.float32)).to(dev)


def crops_per_s(eng, x, prior, bufs, windows, iters):
    n = x.shape[0]
    plain = lambda: eng.forward(x, out=bufs['poses'])
    bound = lambda: eng.forward_posterior(x, prior, out=bufs['poses'])
    arms = (('plain', plain), ('bound', bound), ('plain_again', plain))
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
    out['bound_over_plain'] = round(med['bound'] / a, 4)          # < 1: asking for the posterior costs that share
    out['bound_extra_us_per_call'] = round((n / med['bound'] - n / a) * 1e6, 1)
    return out


def kernel_rows(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get('Name', '')
            if 'heat_posterior' in name or 'head_f16' in name:
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
        raise SystemExit('heat_posterior_probe: no HIP device visible (there is nothing to measure on a CPU)')
    dev = torch.device('cuda', 0)
    spec = ModelSpec(50, 16, 'h36m')
    params = synth.make_params(50, spec.n_head_channels, 64, seed=0, logit_gain=synth.logit_gain_for(50, 16))
    sk = spec.skeleton
    result = {'config': 'resnet_v2_50 stride 16 h36m f16', 'device': torch.cuda.get_device_name(0), 'batches': {}}
    for n in [int(b) for b in opts.batches.split(',')]:
        eng = Engine(spec, params, 'f16', max_batch=n, device=dev)
        x = torch.from_numpy(synth.make_images(n, spec.proc_side, seed=1)).to(dev)
        prior = random_prior(n, sk.n_out, dev)
        bufs = {'poses': torch.empty((n, sk.n_out, 3), device=dev)}
        ref = eng.forward(x).clone()
        poses, post = eng.forward_posterior(x, prior)
        assert torch.equal(poses, ref), 'poses changed with the prior bound'
        assert bool(torch.isfinite(post).all()), 'a posterior of the probe is not finite'
        assert eng._heat_chunk() == n, 'the probe times one bound forward per call'
        iters = 2 if opts.quick else max(4, 2048 // n)
        result['batches'][str(n)] = crops_per_s(eng, x, prior, bufs, 1 if opts.quick else 5, iters)
        result['batches'][str(n)]['scratch_bytes'] = int(eng.lib.metro_plan_prior_scratch_bytes(eng._plan, n))
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
